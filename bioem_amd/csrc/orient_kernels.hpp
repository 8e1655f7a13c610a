// orient_kernels.hpp -- summaries of the orientation posterior, reduced where the angle table lives
// (bioem_hip_orientation_sums, bioem_hip_debug_orient_sums), and, further down, the same table reduced along
// the particles (bioem_hip_orientation_occupancy).  For entry (o, p) of the [nO][nMaps] table with
// F = forAngles > 0:  l = (log F + ConstAngle) + prior_o, and per particle
//   m = max l, omax = first o attaining it, count,  S0 = sum e^(l-m), S1 = sum e^(l-m)(l-m), S2 = sum e^(2(l-m)),
//   Q = upper triangle of sum e^(l-m) q q^T, q the orientation's quaternion normalised in double.
// Two passes: the maximum first (exact, order-free), then the sums relative to it.  Lanes run along particles (the table
// is orientation-major: a wave reads 64 consecutive 16-byte entries of a row); the orientation range is cut into chunks
// of kOrientChunk, the grid is (particle blocks) x (chunks), partials are folded in chunk order.  No atomics.
// No reference counterpart.  The declarations are for every translation unit; the kernels are compiled by
// kernels_orient.hip only (BIOEM_ORIENT_TU).
#ifndef BIOEM_ORIENT_KERNELS_HPP
#define BIOEM_ORIENT_KERNELS_HPP

#include "engine_types.hpp"

const int kOrientChunk = 256; // orientations per block: depends on nothing, so a particle's bits depend on nO alone
const int kOrientSums = 13;   // S0 S1 S2 Q[10]

struct BioemOrientMax // chunk maximum of a particle, 16 bytes
{
  double m;
  int idx, count; // first orientation (relative to the table) attaining m, -1 when count = 0
};

// doubles of scratch a pass over nO orientations and np particles needs: the chunk maxima, the chunk sums and the
// folded maxima (120 bytes per chunk and particle against 4 096 of table: 2.9 %)
BIOEM_HIDDEN size_t bioem_orient_scratch(int nO, int np);
// qq[n][10] = the ten products q_i q_j of every quaternion, formed once
BIOEM_HIDDEN hipError_t bioem_orient_products_launch(hipStream_t st, const float4 *angles, int n, double *qq);
// out[np] for the particles [p0, p0 + np) of the table pang[nO][nMaps]; o0 = global index of row 0.  prior: null or
// [nO] by row; qq: null (no moments) or [nO][10] by row.  ownOff != null: the own-list instantiation, row k of particle
// p is entry ownOff[p] + k of ownAngles (moments when ownIsQuat), prior and qq unused.
BIOEM_HIDDEN hipError_t bioem_orient_sums_launch(hipStream_t st, const bioem_hip_prob_angle *pang, int nO, int nMaps, int p0,
                                                 int np, int o0, const double *prior, const double *qq,
                                                 const float4 *ownAngles, const int *ownOff, int ownIsQuat,
                                                 double *scratch, bioem_hip_orient_sums *out);

// ---- occupancy of every orientation over the particles (bioem_hip_orientation_occupancy) ----
// The same table reduced along the other axis: per orientation row the sums over the particles [p0, p0 + np) of
//   w(o, p) = e^(orient_key(entry, prior_o) - m_p) / S0_p,
// m_p, S0_p, omax_p the particle's (merged) orientation sums, handed in as m[np], rS0[np] = 1 / S0_p (0: the particle is
// left out) and omax[np] (-1 when left out).  One wave per row, kOccRows rows after one another per wave so that a
// lane reads a particle's normalisers once for them; lane j takes the particles j, j + 64, ... in order, two per trip
// with their eight row loads issued together; the 64 lanes are folded by a fixed butterfly.  A row's bits depend on its entries of the range, its prior and the normalisers only.
const int kOccRows = 4;  // rows a wave walks side by side
const int kOccWaves = 4; // waves of a block
// out[nO] for the rows of pang[nO][nMaps]; o0 = global index of row 0; prior: null or [nO] by row
BIOEM_HIDDEN hipError_t bioem_orient_occ_launch(hipStream_t st, const bioem_hip_prob_angle *pang, int nO, int nMaps, int p0,
                                                int np, int o0, const double *prior, const double *m, const double *rS0,
                                                const int *omax, bioem_hip_orient_occ *out);

#ifdef BIOEM_ORIENT_TU
namespace
{

// the key of an entry: both passes, and the occupancy pass after them, evaluate this one expression, so the entry that
// gave m has l - m = 0 exactly
__device__ inline double orient_key(const bioem_hip_prob_angle a, double prior) { return (log(a.forAngles) + a.ConstAngle) + prior; }

// the ten products of a quaternion normalised in double; the prep kernel and the own-list lanes share the expression
__device__ inline void orient_products(const float4 a, double qq[10])
{
  const double x = (double) a.x, y = (double) a.y, z = (double) a.z, w = (double) a.w;
  const double n2 = ((x * x + y * y) + z * z) + w * w;
  const double n = sqrt(n2);
  const bool ok = n2 > 0. && n2 < INFINITY; // a zero or non-finite entry is no rotation: it adds nothing to Q
  const double q[4] = {ok ? x / n : 0., ok ? y / n : 0., ok ? z / n : 0., ok ? w / n : 0.};
  int k = 0;
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = i; j < 4; j++)
      qq[k++] = q[i] * q[j];
}

__global__ void k_orient_products(const float4 *__restrict__ angles, int n, double *__restrict__ qq)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n)
    return;
  double v[10];
  orient_products(angles[i], v);
#pragma unroll
  for (int k = 0; k < 10; k++)
    qq[(size_t) i * 10 + k] = v[k];
}

// block (particle block x, chunk y), one wave: part[y][np] = the chunk's maximum, its first index and its count
__global__ __launch_bounds__(64) void k_orient_max(const bioem_hip_prob_angle *__restrict__ pang, int nO, int nMaps, int p0,
                                                   int np, const double *__restrict__ prior,
                                                   const int *__restrict__ ownOff, BioemOrientMax *__restrict__ part)
{
  const int p = blockIdx.x * 64 + threadIdx.x;
  if (p >= np)
    return;
  const int io0 = blockIdx.y * kOrientChunk, io1 = min(nO, io0 + kOrientChunk);
  const bioem_hip_prob_angle *col = pang + (size_t) p0 + p;
  const int len = ownOff ? ownOff[p0 + p + 1] - ownOff[p0 + p] : nO; // own lists: rows beyond the list do not count
  BioemOrientMax r = {-INFINITY, -1, 0};
  for (int io = io0; io < io1; io++) // io is wave-uniform: the prior comes by a scalar load
  {
    const bioem_hip_prob_angle a = col[(size_t) io * nMaps];
    const double pr = prior ? prior[io] : 0.;
    if (a.forAngles > 0. && io < len)
    {
      const double l = orient_key(a, pr);
      r.count++;
      if (l > r.m) // strictly: the first index keeps a tie
      {
        r.m = l;
        r.idx = io;
      }
    }
  }
  part[(size_t) blockIdx.y * np + p] = r;
}

// part[y][kOrientSums][np] = the chunk's sums relative to the particle's folded maximum gmax[p], orientation order
template <bool OWN>
__global__ __launch_bounds__(64) void k_orient_sums(const bioem_hip_prob_angle *__restrict__ pang, int nO, int nMaps, int p0,
                                                    int np, const double *__restrict__ prior, const double *__restrict__ qq,
                                                    const float4 *__restrict__ ownAngles, const int *__restrict__ ownOff,
                                                    int moments, const double *__restrict__ gmax, double *__restrict__ part)
{
  const int p = blockIdx.x * 64 + threadIdx.x;
  if (p >= np)
    return;
  const int io0 = blockIdx.y * kOrientChunk, io1 = min(nO, io0 + kOrientChunk);
  const bioem_hip_prob_angle *col = pang + (size_t) p0 + p;
  const double m = gmax[p];
  int first = 0, len = 0;
  if constexpr (OWN)
  {
    first = ownOff[p0 + p];
    len = ownOff[p0 + p + 1] - first;
  }
  double S0 = 0., S1 = 0., S2 = 0., Q[10];
#pragma unroll
  for (int k = 0; k < 10; k++)
    Q[k] = 0.;
  for (int io = io0; io < io1; io++)
  {
    const bioem_hip_prob_angle a = col[(size_t) io * nMaps];
    double pr = 0.;
    if constexpr (!OWN)
      pr = prior ? prior[io] : 0.;
    bool counts = a.forAngles > 0.;
    if constexpr (OWN)
      counts = counts && io < len; // (an entry beyond the list never reads the list)
    if (counts)
    {
      const double d = orient_key(a, pr) - m;
      const double e = exp(d);
      S0 += e;
      S1 = fma(e, d, S1);
      S2 = fma(e, e, S2);
      if (moments) // uniform
      {
        if constexpr (OWN)
        {
          double v[10];
          orient_products(ownAngles[(size_t) first + io], v);
#pragma unroll
          for (int k = 0; k < 10; k++)
            Q[k] = fma(e, v[k], Q[k]);
        }
        else
        {
          const double *v = qq + (size_t) io * 10; // wave-uniform: scalar loads
#pragma unroll
          for (int k = 0; k < 10; k++)
            Q[k] = fma(e, v[k], Q[k]);
        }
      }
    }
  }
  double *o = part + (size_t) blockIdx.y * kOrientSums * np + p;
  o[0] = S0;
  o[(size_t) np] = S1;
  o[(size_t) 2 * np] = S2;
#pragma unroll
  for (int k = 0; k < 10; k++)
    o[(size_t) (3 + k) * np] = Q[k];
}

// the chunks of a particle merged in chunk order.  SUMS = false, after k_orient_max: the maximum (a later chunk wins
// only when strictly greater: the lowest index keeps a tie), the counts added; m into gmax, and m, omax (global), count,
// hasMoments into out.  SUMS = true, after k_orient_sums: the thirteen sums added into out.
template <bool SUMS>
__global__ void k_orient_fold(const void *__restrict__ part, int nChunks, int np, int o0, int moments,
                              double *__restrict__ gmax, bioem_hip_orient_sums *__restrict__ out)
{
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= np)
    return;
  if constexpr (SUMS)
  {
    const double *s = static_cast<const double *>(part) + p;
    double v[kOrientSums];
#pragma unroll
    for (int k = 0; k < kOrientSums; k++)
      v[k] = s[(size_t) k * np];
    for (int c = 1; c < nChunks; c++)
#pragma unroll
      for (int k = 0; k < kOrientSums; k++)
        v[k] += s[((size_t) c * kOrientSums + k) * np];
    out[p].S0 = v[0];
    out[p].S1 = v[1];
    out[p].S2 = v[2];
#pragma unroll
    for (int k = 0; k < 10; k++)
      out[p].Q[k] = v[3 + k];
  }
  else
  {
    const BioemOrientMax *s = static_cast<const BioemOrientMax *>(part) + p;
    BioemOrientMax r = s[0];
    for (int c = 1; c < nChunks; c++)
    {
      const BioemOrientMax t = s[(size_t) c * np];
      r.count += t.count;
      if (t.m > r.m)
      {
        r.m = t.m;
        r.idx = t.idx;
      }
    }
    const double m = r.count ? r.m : MIN_PROB;
    gmax[p] = m;
    out[p].m = m;
    out[p].omax = r.count ? (double) (o0 + r.idx) : -1.;
    out[p].count = (double) r.count;
    out[p].hasMoments = moments ? 1. : 0.;
  }
}

// the butterfly of the occupancy fold: every lane ends with the value of the whole wave, the pairing is fixed
template <class T>
__device__ inline T occ_wave_sum(T v)
{
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1)
    v += __shfl_xor(v, s, 64);
  return v;
}

// block of kOccWaves waves, wave v of block b: rows (b kOccWaves + v) kOccRows ... + kOccRows - 1
__global__ __launch_bounds__(64 * kOccWaves) void k_orient_occ(const bioem_hip_prob_angle *__restrict__ pang, int nO, int nMaps,
                                                               int p0, int np, int o0, const double *__restrict__ prior,
                                                               const double *__restrict__ gm, const double *__restrict__ grS0,
                                                               const int *__restrict__ gomax,
                                                               bioem_hip_orient_occ *__restrict__ out)
{
  const int wave = __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const int r0 = (blockIdx.x * kOccWaves + wave) * kOccRows; // wave-uniform
  if (r0 >= nO)
    return;
  const bioem_hip_prob_angle *row[kOccRows];
  double pr[kOccRows], occ[kOccRows], occ2[kOccRows], wmax[kOccRows];
  int pmax[kOccRows], cnt[kOccRows], hard[kOccRows], glob[kOccRows];
#pragma unroll
  for (int k = 0; k < kOccRows; k++)
  {
    const int r = min(r0 + k, nO - 1); // a row beyond the table re-reads the last one and is not written
    row[k] = pang + (size_t) r * nMaps + p0;
    pr[k] = prior ? prior[r] : 0.; // wave-uniform: a scalar load
    glob[k] = o0 + r;
    occ[k] = occ2[k] = 0.;
    wmax[k] = -1.; // below every w: the first counted entry takes it, w = 0 included
    pmax[k] = 0x7fffffff;
    cnt[k] = hard[k] = 0;
  }
  // Two particles of the lane per trip, j and j + 64.  All eight row loads and the normalisers of both are issued before
  // anything is tested: the body has no branch a load could sink into.  An entry that does not count (F <= 0, or its
  // particle left out, or j + 64 beyond the range, which re-reads j) goes through the arithmetic with d = 0 and adds
  // w = 0, count 0: adding +0 leaves a sum of non-negative terms bit for bit, and no 0 * inf is formed.
  for (int j = lane; j < np; j += 128)
  {
    const bool has2 = j + 64 < np;
    const int jj[2] = {j, has2 ? j + 64 : j};
    bioem_hip_prob_angle a[2][kOccRows];
    double m[2], rs[2];
    int om[2];
#pragma unroll
    for (int h = 0; h < 2; h++)
    {
#pragma unroll
      for (int k = 0; k < kOccRows; k++)
      { // one 16-byte load per entry; the table is read once: non-temporal
        typedef double entry2 __attribute__((ext_vector_type(2)));
        const entry2 v = __builtin_nontemporal_load(reinterpret_cast<const entry2 *>(row[k] + jj[h]));
        a[h][k].forAngles = v.x;
        a[h][k].ConstAngle = v.y;
      }
      m[h] = gm[jj[h]];
      rs[h] = grS0[jj[h]];
      om[h] = gomax[jj[h]];
    }
    if (!has2)
    {
      rs[1] = 0.;
      om[1] = -1;
    }
#pragma unroll
    for (int h = 0; h < 2; h++) // in particle order
#pragma unroll
      for (int k = 0; k < kOccRows; k++)
      {
        const bool counts = (a[h][k].forAngles > 0.) & (rs[h] > 0.); // om = -1 where the particle is left out
        bioem_hip_prob_angle e = a[h][k];
        e.forAngles = counts ? e.forAngles : 1.;
        const double d = counts ? orient_key(e, pr[k]) - m[h] : 0.;
        const double w = counts ? exp(d) * rs[h] : 0.;
        hard[k] += om[h] == glob[k];
        occ[k] += w;
        occ2[k] = fma(w, w, occ2[k]);
        cnt[k] += counts;
        const bool up = counts & (w > wmax[k]); // strictly: the lane's lowest particle keeps a tie
        wmax[k] = up ? w : wmax[k];
        pmax[k] = up ? p0 + jj[h] : pmax[k];
      }
  }
#pragma unroll
  for (int k = 0; k < kOccRows; k++)
  {
    const double s0 = occ_wave_sum(occ[k]), s2 = occ_wave_sum(occ2[k]);
    const int c = occ_wave_sum(cnt[k]), hd = occ_wave_sum(hard[k]);
    double wm = wmax[k];
    int pm = pmax[k];
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1)
    {
      const double ow = __shfl_xor(wm, s, 64);
      const int op = __shfl_xor(pm, s, 64);
      if (ow > wm || (ow == wm && op < pm)) // the lower particle index wins a tie
      {
        wm = ow;
        pm = op;
      }
    }
    if (lane == 0 && r0 + k < nO)
    {
      bioem_hip_orient_occ r;
      r.occ = s0;
      r.occ2 = s2;
      r.wmax = c ? wm : 0.;
      r.pmax = c ? (double) pm : -1.;
      r.count = (double) c;
      r.hard = (double) hd;
      out[r0 + k] = r;
    }
  }
}

} // namespace
#endif // BIOEM_ORIENT_TU

#endif
