// ring_kernels.hpp -- per-ring sums of every particle's spectrum against the spectrum of its best match
// (bioem_hip_best_match_rings, bioem_hip_debug_ring_sums): for the record (o, c, X, Y, norm, mu) of a particle
//   Z = P_o conj(CTF_c) formed in double from the float spectra,
//   M[k1][k2] = norm Z[k1][k2] exp(-2 pi i ((k1 X + k2 Y) mod N) / N), in the columns k2 = 0 and (N even) N / 2 its
//   Hermitian part (M[k1] + conj(M[N - k1])) / 2 along k1, + mu N^2 on the real part of M[0][0]
// (the r2c spectrum of the image bioem_hip_render_best_maps writes), and per ring s of the half spectrum, with the weight
// w of the Hermitian partner, cross = sum w Re(R conj(M)), powParticle = sum w |R|^2, powModel = sum w |M|^2 in double.
// No reference counterpart.  The declarations are for every translation unit; the kernels are compiled by
// kernels_rings.hip only (BIOEM_RING_TU).
#ifndef BIOEM_RING_KERNELS_HPP
#define BIOEM_RING_KERNELS_HPP

#include "engine_types.hpp"

// ring of the coefficient (k1', k2), k1' the signed row frequency: the radius rounded to nearest, decided in integers
__host__ __device__ inline int bioem_ring_index(int a, int k2)
{
  const int r2 = a * a + k2 * k2; // at most 2 * 2560^2: exact in int and in float
  int s = (int) sqrtf((float) r2);
  while (s * s > r2)
    s--;
  while ((s + 1) * (s + 1) <= r2)
    s++;
  return r2 > s * s + s ? s + 1 : s;
}

// one image of a batch: the layout of RenderRecord (render_kernels.hpp); the ring pass does not read src
struct BioemRingRecord
{
  int src, conv, X, Y;
  float norm, mu;
};

const int kRingWaves = 4; // waves of a block, each with a ring table of its own

BIOEM_HIDDEN int bioem_ring_count(int N);  // rings of an N x N image, corners included; 0 for N < 1
BIOEM_HIDDEN int bioem_ring_splits(int N); // blocks an image is split over: a function of N alone
// doubles of scratch the pass needs for a batch of nImg images (block partials, ring tables kept in global memory)
BIOEM_HIDDEN size_t bioem_ring_scratch(int N, int nImg);
// out[nImg][nRings] from specR / specP [nImg][N][N/2+1] (reference layout), the uploaded CTF kernels and the records;
// tw = exp(+2 pi i k / N), N double pairs.  The ring tables of a block live in LDS where kRingWaves of them fit 64 KiB (up
// to 964 pixels), else in scratch; both run the same arithmetic in the same order.
BIOEM_HIDDEN hipError_t bioem_ring_sums_launch(hipStream_t st, const float2 *specR, const float2 *specP, const float2 *ctf,
                                               const BioemRingRecord *rec, int nImg, int N, const double2 *tw,
                                               double *scratch, bioem_hip_ring_sums *out);

#ifdef BIOEM_RING_TU
namespace
{

// ring table entry += v.  LDS: the data-share unit serves a wave's accesses in issue order.  Global memory: lanes of one
// wave hand an entry on to each other between two row chunks, so the accesses go to the device-coherent level (relaxed,
// agent scope) and ring_table_fence() stands between the chunks.  One lane per entry at a time: no atomic addition,
// the order of the additions is the program's.
template <bool GTAB>
__device__ inline void ring_table_add(double *p, double v)
{
  if constexpr (GTAB)
    __hip_atomic_store(p, __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + v, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
  else
    *p += v;
}
template <bool GTAB>
__device__ inline double ring_table_get(const double *p)
{
  if constexpr (GTAB)
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else
    return *p;
}
template <bool GTAB>
__device__ inline void ring_table_fence()
{
  if constexpr (GTAB)
    __threadfence_block();
  else
    __builtin_amdgcn_wave_barrier();
}

// Block (image, split j) of kRingWaves waves; wave w takes the rows k1 = kRingWaves j + w + kRingWaves S i, a lane a
// column k2 of a chunk of 64.  Within a row the ring never decreases with k2, so the lanes of a ring are contiguous: a
// segmented reduction over the fixed tree of distances 1, 2, ... 32 leaves a run's sum in its first lane, which adds it to
// the wave's table.  The block folds its tables in wave order into dst[block][nRings] (the result itself when S = 1,
// else a partial for k_ring_fold).  The split depends on N only, so a particle's sums do not depend on its batch.
// gtab = [blocks][kRingWaves][nRings][3] (GTAB), dynamic LDS = kRingWaves nRings triples otherwise.
template <bool GTAB>
__global__ __launch_bounds__(64 * kRingWaves) void k_ring_sums(const float2 *__restrict__ specR, const float2 *__restrict__ specP,
                                                               const float2 *__restrict__ ctf,
                                                               const BioemRingRecord *__restrict__ rec, int N, int H, int nRings,
                                                               int S, const double2 *__restrict__ tw, double *gtab,
                                                               double *__restrict__ dst)
{
  extern __shared__ double ring_lds[];
  const int img = blockIdx.x / S, j = blockIdx.x - img * S;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const size_t T = 3 * (size_t) nRings, M = (size_t) N * H;
  double *tab;
  if constexpr (GTAB)
    tab = gtab + ((size_t) blockIdx.x * kRingWaves + wave) * T;
  else
    tab = ring_lds + wave * T;
  for (size_t i = lane; i < T; i += 64)
  {
    if constexpr (GTAB)
      __hip_atomic_store(tab + i, 0., __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else
      tab[i] = 0.;
  }
  ring_table_fence<GTAB>();

  const BioemRingRecord r = rec[img];
  const float2 *R = specR + img * M, *P = specP + img * M, *C = ctf + (size_t) r.conv * M;
  const double norm = (double) r.norm, dc = (double) r.mu * (double) N * (double) N;
  // t = (k1 X + k2 Y) mod N kept by additions: every term below is already reduced to [0, N)
  const unsigned uN = (unsigned) N;
  const unsigned xm = (unsigned) ((r.X % N + N) % N), ym = (unsigned) ((r.Y % N + N) % N);
  const int rowStep = kRingWaves * S, row0 = kRingWaves * j + wave;
  const unsigned stepRow = (unsigned) (((unsigned long long) rowStep * xm) % uN);
  const unsigned stepChunk = (unsigned) ((64ull * ym) % uN);
  const unsigned tLane = (unsigned) (((unsigned long long) lane * ym) % uN);
  unsigned tRow = (unsigned) (((unsigned long long) row0 * xm) % uN);
  for (int k1 = row0; k1 < N; k1 += rowStep)
  {
    const int a = k1 <= N / 2 ? k1 : k1 - N;
    unsigned tCol = tLane;
    for (int k2b = 0; k2b < H; k2b += 64)
    {
      const int k2 = k2b + lane;
      int s = 0x7fffffff; // lanes beyond the row: a run of their own that nobody stores
      double cr = 0., pp = 0., pm = 0.;
      if (k2 < H)
      {
        s = bioem_ring_index(a, k2);
        const size_t e = (size_t) k1 * H + k2;
        const float2 x = R[e], p = P[e], c = C[e];
        const double zr = (double) p.x * (double) c.x + (double) p.y * (double) c.y;
        const double zi = (double) p.y * (double) c.x - (double) p.x * (double) c.y;
        unsigned t = tRow + tCol;
        t = t >= uN ? t - uN : t;
        const double2 w = tw[t]; // exp(+i): M takes the conjugate
        double mr = norm * (zr * w.x + zi * w.y);
        double mi = norm * (zi * w.x - zr * w.y);
        const bool selfConj = k2 == 0 || 2 * k2 == N;
        if (selfConj)
        { // a column that is its own Hermitian partner: the c2r of the render keeps the Hermitian part along k1 only, so
          // the image's spectrum is (M[k1] + conj(M[N - k1])) / 2 there (M itself where Z is the spectrum of a real image)
          const size_t ec = (size_t) (k1 ? N - k1 : 0) * H + k2;
          const float2 pc = P[ec], cc = C[ec];
          const double yr = (double) pc.x * (double) cc.x + (double) pc.y * (double) cc.y;
          const double yi = (double) pc.y * (double) cc.x - (double) pc.x * (double) cc.y;
          unsigned tc = (tRow ? uN - tRow : 0u) + tCol;
          tc = tc >= uN ? tc - uN : tc;
          const double2 wc = tw[tc];
          mr = 0.5 * (mr + norm * (yr * wc.x + yi * wc.y));
          mi = 0.5 * (mi - norm * (yi * wc.x - yr * wc.y));
        }
        if ((k1 | k2) == 0)
          mr += dc;
        const double wgt = selfConj ? 1. : 2.;
        const double xr = (double) x.x, xi = (double) x.y;
        cr = wgt * (xr * mr + xi * mi);
        pp = wgt * (xr * xr + xi * xi);
        pm = wgt * (mr * mr + mi * mi);
      }
#pragma unroll
      for (int d = 1; d < 64; d <<= 1)
      {
        const int so = __shfl_down(s, d);
        const double co = __shfl_down(cr, d), po = __shfl_down(pp, d), mo = __shfl_down(pm, d);
        if (lane + d < 64 && so == s)
        {
          cr += co;
          pp += po;
          pm += mo;
        }
      }
      const int sp = __shfl_up(s, 1);
      if (k2 < H && (lane == 0 || sp != s))
      {
        ring_table_add<GTAB>(tab + 3 * (size_t) s, cr);
        ring_table_add<GTAB>(tab + 3 * (size_t) s + 1, pp);
        ring_table_add<GTAB>(tab + 3 * (size_t) s + 2, pm);
      }
      ring_table_fence<GTAB>();
      tCol += stepChunk;
      tCol = tCol >= uN ? tCol - uN : tCol;
    }
    tRow += stepRow;
    tRow = tRow >= uN ? tRow - uN : tRow;
  }
  if constexpr (GTAB)
    __threadfence_block();
  __syncthreads();
  const double *t0 = GTAB ? gtab + (size_t) blockIdx.x * kRingWaves * T : ring_lds;
  double *o = dst + (size_t) blockIdx.x * T;
  for (size_t i = threadIdx.x; i < T; i += 64 * kRingWaves)
  {
    double v = ring_table_get<GTAB>(t0 + i);
#pragma unroll
    for (int w = 1; w < kRingWaves; w++)
      v += ring_table_get<GTAB>(t0 + w * T + i);
    o[i] = v;
  }
}

// out[img][i] = part[img][0][i] + part[img][1][i] + ... in split order; T = 3 nRings doubles per table; a block per image
__global__ void k_ring_fold(const double *__restrict__ part, int S, int T, double *__restrict__ out)
{
  const size_t img = blockIdx.x;
  for (int i = threadIdx.x; i < T; i += blockDim.x)
  {
    const double *p = part + img * S * (size_t) T + i;
    double v = p[0];
    for (int j = 1; j < S; j++)
      v += p[(size_t) j * T];
    out[img * (size_t) T + i] = v;
  }
}

} // namespace
#endif // BIOEM_RING_TU

#endif
