// fold_kernels.hpp -- fold of per-comparison partials into the probability block
// Part of libbioem_hip.so; included by bioem_hip.hip only (one translation unit, anonymous namespace).
#ifndef BIOEM_FOLD_KERNELS_HPP
#define BIOEM_FOLD_KERNELS_HPP

namespace
{

// ------------------------------------------------------------------------------------------------
// WRITE_PROB_ANGLES table: one thread per (particle, orientation of this launch) folds that orientation's CTF
// partials into its angle entry, in CTF order -- the same arithmetic sequence per entry as the reference
// (bioem_algorithm.h:130-141).  The particle entries are then folded by k_fold_wave.  Rows of orientation j:
// [j*convPerOrient, (j+1)*convPerOrient) (native path, segs == null)
// or the run segs[j] = {first row, end row, orientation} (compat ring: every orientation of a launch is ONE run).
// ------------------------------------------------------------------------------------------------
__global__ void k_fold_angles(const Partial *__restrict__ partials, int ldPart, int nOC, int nMaps, int orient0,
                              int convPerOrient, const int4 *__restrict__ segs, int nRuns,
                              bioem_hip_prob_angle *__restrict__ pang, int angO0)
{
  const long long t = (long long) blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long long) nRuns * nMaps)
    return;
  const int j = (int) (t / nMaps), p = (int) (t - (long long) j * nMaps); // particle index fastest: coalesced table
  const Partial *P = partials + (size_t) p * ldPart;
  int ocBegin = j * convPerOrient, ocEnd = min(nOC, (j + 1) * convPerOrient), iOrient = orient0 + j;
  if (segs)
  {
    const int4 sg = segs[j];
    ocBegin = sg.x;
    ocEnd = sg.y;
    iOrient = sg.z;
  }
  // the table holds the orientations [angO0, ...) this handle owns (all of them unless it is a shard)
  bioem_hip_prob_angle pa = pang[(size_t) (iOrient - angO0) * nMaps + p];
  for (int oc = ocBegin; oc < ocEnd; oc++)
  {
    const Partial r = P[oc];
    const double lp = (double) r.best;
    if (pa.ConstAngle < lp)
    {
      pa.forAngles *= exp(-lp + pa.ConstAngle);
      pa.ConstAngle = lp;
    }
    pa.forAngles += r.sumExp * exp(lp - pa.ConstAngle);
  }
  pang[(size_t) (iOrient - angO0) * nMaps + p] = pa;
}

// ------------------------------------------------------------------------------------------------
// wave-parallel fold of the particle entries: one wave per particle; lane l folds a contiguous chunk of
// (orientation, CTF) partials in order, the 64 chunk results are merged by a shuffle reduction that keeps
// the FIRST maximum (lowest index), then combined with the running state exactly like the sequential fold.
// The log-sum-exp merge is associative, so the result equals the sequential fold's (bioem_algorithm.h:94-141 /
// bioem.cpp:1527-1600) up to double rounding: every term is positive, and on its way through a chunk, the shuffle levels,
// the wave merge and the launch-to-launch update a row's term meets one product, at most T + 64 rescales (an exp and a
// multiply: 3 units of 2^-53) and as many additions, so log(Total) + Constoadd lies within 4 (T + 64) 2^-53 of the exact
// log-sum-exp of the launch's T rows (6e-13 for 1 281 rows; tests/test_fold_exact.py holds every fold kernel to it).
// ------------------------------------------------------------------------------------------------
// WPP = 4 (few particles: one wave per particle left the chip to ten waves walking 48 partials each, 40 us per launch):
// the four waves of a block share one particle, wave w the w-th quarter of its partials; their results are merged in
// wave order through LDS by the same first-maximum rule.
template <int WPP>
__global__ __launch_bounds__(256) void k_fold_wave(const Partial *__restrict__ partials, int ldPart, int nOC,
                                                   int nMaps, const bioem_hip_param5 *__restrict__ params,
                                                   const float *__restrict__ sumRef, const int *__restrict__ disp,
                                                   int nd, PD pd, int orient0, int conv0, int convPerOrient,
                                                   const int2 *__restrict__ ids,
                                                   bioem_hip_prob_map *__restrict__ pmap)
{
  static_assert(WPP == 1 || WPP == 4, "one wave or one block per particle");
  __shared__ double shM[4], shS[4];
  __shared__ int shI[4];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int p = WPP == 1 ? blockIdx.x * 4 + wave : blockIdx.x;
  if (p >= nMaps)
    return;
  const Partial *P = partials + (size_t) p * ldPart;
  const int nChunks = 64 * WPP;
  const int chunk = (nOC + nChunks - 1) / nChunks;
  const int b = min(nOC, (WPP == 1 ? lane : (int) threadIdx.x) * chunk), e = min(nOC, b + chunk);
  double m = -INFINITY, sacc = 0.;
  int idx = 0x7fffffff;
#pragma unroll 4
  for (int oc = b; oc < e; oc++)
  {
    const Partial r = P[oc];
    const double lp = (double) r.best;
    if (m < lp)
    {
      sacc = (m == -INFINITY) ? 0. : sacc * exp(m - lp);
      m = lp;
      idx = oc;
    }
    sacc += r.sumExp * exp(lp - m);
  }
  for (int off = 32; off > 0; off >>= 1)
  {
    const double m2 = __shfl_xor(m, off);
    const double s2 = __shfl_xor(sacc, off);
    const int i2 = __shfl_xor(idx, off);
    if (m2 > m || (m2 == m && i2 < idx))
    {
      sacc = ((m == -INFINITY) ? 0. : sacc * exp(m - m2)) + s2;
      m = m2;
      idx = i2;
    }
    else
      sacc += (m2 == -INFINITY) ? 0. : s2 * exp(m2 - m);
  }
  if (WPP == 4)
  {
    if (lane == 0)
    {
      shM[wave] = m;
      shS[wave] = sacc;
      shI[wave] = idx;
    }
    __syncthreads();
    if (threadIdx.x == 0)
      for (int w = 1; w < 4; w++)
      {
        const double m2 = shM[w], s2 = shS[w];
        const int i2 = shI[w];
        if (m2 > m || (m2 == m && i2 < idx))
        {
          sacc = ((m == -INFINITY) ? 0. : sacc * exp(m - m2)) + s2;
          m = m2;
          idx = i2;
        }
        else
          sacc += (m2 == -INFINITY) ? 0. : s2 * exp(m2 - m);
      }
  }
  if (threadIdx.x % (64 * WPP) == 0 && idx != 0x7fffffff)
  {
    bioem_hip_prob_map pm = pmap[p];
    if (pm.Constoadd < m)
    {
      pm.Total *= exp(-m + pm.Constoadd);
      pm.Constoadd = m;
      const Partial r = P[idx];
      const int ix = r.id / nd, iy = r.id - ix * nd;
      pm.max_prob_cent_x = -disp[ix];
      pm.max_prob_cent_y = -disp[iy];
      pm.max_prob_orient = ids ? ids[idx].x : orient0 + idx / convPerOrient;
      pm.max_prob_conv = ids ? ids[idx].y : conv0 + idx % convPerOrient;
      const bioem_hip_param5 q = params[idx];
      const float sumref = sumRef[p];
      const float value = r.value;
      pm.max_prob_norm = -(-q.sumC * sumref + pd.Ntotpi * value) / (q.sumC * q.sumC - q.sumsquareC * pd.Ntotpi);
      pm.max_prob_mu = -(-q.sumC * value + q.sumsquareC * sumref) / (q.sumC * q.sumC - q.sumsquareC * pd.Ntotpi);
    }
    pm.Total += sacc * exp(m - pm.Constoadd);
    pmap[p] = pm;
  }
}

// ------------------------------------------------------------------------------------------------
// own-list pass (bioem_hip_compare_own_orientations): row oc of a launch is row row0 + oc of the flat
// [particle][list entry k][CTF] order -- particle p owns slots off[p] ... off[p + 1], nCTF rows each, the lists may differ
// in length -- and was compared with its own particle only; partials[oc] is its result.  One wave per particle with rows
// in the launch folds exactly those rows, by the rules of k_fold_wave (first maximum = lowest row, log-sum-exp in double,
// norm / mu from the best row); max_prob_orient is the index in that particle's list.  A list that straddles two launches
// is folded in two steps, like two batches of the all-to-all pass; a particle without rows in the launch is not touched.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_fold_own(const Partial *__restrict__ partials, int nOC, int row0,
                                                  const int *__restrict__ off, int nCTF, int pFirst, int pEnd,
                                                  const bioem_hip_param5 *__restrict__ params,
                                                  const float *__restrict__ sumRef, const int *__restrict__ disp, int nd,
                                                  PD pd, bioem_hip_prob_map *__restrict__ pmap)
{
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int p = pFirst + blockIdx.x * 4 + wave;
  if (p >= pEnd)
    return;
  const long long g0 = (long long) off[p] * nCTF, g1 = (long long) off[p + 1] * nCTF; // the particle's rows in the flat order
  const int rb = (int) (max(g0, (long long) row0) - row0), re = (int) (min(g1, (long long) row0 + nOC) - row0);
  if (re <= rb)
    return;
  const int chunk = (re - rb + 63) / 64;
  const int b = min(re, rb + lane * chunk), e = min(re, b + chunk);
  double m = -INFINITY, sacc = 0.;
  int idx = 0x7fffffff;
#pragma unroll 4
  for (int oc = b; oc < e; oc++)
  {
    const Partial r = partials[oc];
    const double lp = (double) r.best;
    if (m < lp)
    {
      sacc = (m == -INFINITY) ? 0. : sacc * exp(m - lp);
      m = lp;
      idx = oc;
    }
    sacc += r.sumExp * exp(lp - m);
  }
  for (int o = 32; o > 0; o >>= 1)
  {
    const double m2 = __shfl_xor(m, o);
    const double s2 = __shfl_xor(sacc, o);
    const int i2 = __shfl_xor(idx, o);
    if (m2 > m || (m2 == m && i2 < idx))
    {
      sacc = ((m == -INFINITY) ? 0. : sacc * exp(m - m2)) + s2;
      m = m2;
      idx = i2;
    }
    else
      sacc += (m2 == -INFINITY) ? 0. : s2 * exp(m2 - m);
  }
  if (lane == 0 && idx != 0x7fffffff)
  {
    bioem_hip_prob_map pm = pmap[p];
    if (pm.Constoadd < m)
    {
      pm.Total *= exp(-m + pm.Constoadd);
      pm.Constoadd = m;
      const Partial r = partials[idx];
      const int ix = r.id / nd, iy = r.id - ix * nd;
      const int local = (int) ((long long) row0 + idx - g0); // k * nCTF + CTF
      pm.max_prob_cent_x = -disp[ix];
      pm.max_prob_cent_y = -disp[iy];
      pm.max_prob_orient = local / nCTF;
      pm.max_prob_conv = local % nCTF;
      const bioem_hip_param5 q = params[idx];
      const float sumref = sumRef[p];
      const float value = r.value;
      pm.max_prob_norm = -(-q.sumC * sumref + pd.Ntotpi * value) / (q.sumC * q.sumC - q.sumsquareC * pd.Ntotpi);
      pm.max_prob_mu = -(-q.sumC * value + q.sumsquareC * sumref) / (q.sumC * q.sumC - q.sumsquareC * pd.Ntotpi);
    }
    pm.Total += sacc * exp(m - pm.Constoadd);
    pmap[p] = pm;
  }
}

// WRITE_PROB_ANGLES of the own-list pass: one thread per slot of the launch -- flat slot s belongs to particle
// slotParticle[s], list entry k = s - off[p] -- folds the slot's CTF rows, in CTF order, into entry (k, p) of the
// [nAngles][nMaps] table: the arithmetic of k_fold_angles.  Entries (k, p) beyond the particle's list are never addressed.
__global__ void k_fold_own_angles(const Partial *__restrict__ partials, int nSlots, int slot0,
                                  const int *__restrict__ off, const int *__restrict__ slotParticle, int nCTF, int nMaps,
                                  bioem_hip_prob_angle *__restrict__ pang)
{
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nSlots)
    return;
  const int s = slot0 + t, p = slotParticle[s], k = s - off[p];
  bioem_hip_prob_angle pa = pang[(size_t) k * nMaps + p];
  for (int oc = t * nCTF; oc < (t + 1) * nCTF; oc++)
  {
    const Partial r = partials[oc];
    const double lp = (double) r.best;
    if (pa.ConstAngle < lp)
    {
      pa.forAngles *= exp(-lp + pa.ConstAngle);
      pa.ConstAngle = lp;
    }
    pa.forAngles += r.sumExp * exp(lp - pa.ConstAngle);
  }
  pang[(size_t) k * nMaps + p] = pa;
}

// ------------------------------------------------------------------------------------------------
// CTF table (bioem_hip_enable_ctf_table): entry (c, p) of the [nCTF][nMaps] table is what particle p's entry would be had
// the run compared CTF set c only -- the fold of the partials of rows (o, c) in orientation order by the rules of
// k_fold_wave (log-sum-exp in double, first maximum = lowest row, norm / mu from the best row), max_prob_conv = c.
// One wave per (CTF, particle) pair; the pair's rows are first, first + stride, ... (count of them), lane l folds a
// contiguous chunk of them in row order, the chunks are merged by the first-maximum shuffle reduction and lane 0
// updates the entry.  Every entry has one writer per launch and launches are ordered on the stream: no atomics, the
// same bits on every run.  With `ids` (compat ring: row oc belongs to CTF ids[oc].y) the lanes walk all rows of the
// launch and take those of their CTF.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void fold_ctf_rows(const Partial *__restrict__ P, int first, int stride, int count,
                                              const int2 *__restrict__ ids, int c, int lane, double &m, double &sacc,
                                              int &idx)
{
  const int chunk = (count + 63) / 64;
  const int b = min(count, lane * chunk), e = min(count, b + chunk);
  m = -INFINITY;
  sacc = 0.;
  idx = 0x7fffffff;
  for (int k = b; k < e; k++)
  {
    const int oc = first + k * stride;
    if (ids && ids[oc].y != c)
      continue;
    const Partial r = P[oc];
    const double lp = (double) r.best;
    if (m < lp)
    {
      sacc = (m == -INFINITY) ? 0. : sacc * exp(m - lp);
      m = lp;
      idx = oc;
    }
    sacc += r.sumExp * exp(lp - m);
  }
  for (int off = 32; off > 0; off >>= 1)
  {
    const double m2 = __shfl_xor(m, off);
    const double s2 = __shfl_xor(sacc, off);
    const int i2 = __shfl_xor(idx, off);
    if (m2 > m || (m2 == m && i2 < idx))
    {
      sacc = ((m == -INFINITY) ? 0. : sacc * exp(m - m2)) + s2;
      m = m2;
      idx = i2;
    }
    else
      sacc += (m2 == -INFINITY) ? 0. : s2 * exp(m2 - m);
  }
}

// shared-list passes.  Native path (ids == null): row oc of the launch is CTF conv0 + oc % convPerOrient, the wave of
// (c, p) walks rows c - conv0, c - conv0 + convPerOrient, ...; nC = convPerOrient pairs per particle.  Compat ring:
// nC = nCTF of the handle, conv0 = 0.  A pair without rows in the launch leaves its entry alone.
__global__ __launch_bounds__(256) void k_fold_ctf(const Partial *__restrict__ partials, int ldPart, int nOC, int nMaps,
                                                  const bioem_hip_param5 *__restrict__ params,
                                                  const float *__restrict__ sumRef, const int *__restrict__ disp,
                                                  int nd, PD pd, int orient0, int conv0, int convPerOrient, int nC,
                                                  const int2 *__restrict__ ids, bioem_hip_prob_map *__restrict__ tab)
{
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long long pair = (long long) blockIdx.x * 4 + wave;
  if (pair >= (long long) nC * nMaps)
    return;
  const int cl = (int) (pair / nMaps), p = (int) (pair - (long long) cl * nMaps); // particle fastest: neighbouring entries
  const int c = conv0 + cl;
  const Partial *P = partials + (size_t) p * ldPart;
  const int first = ids ? 0 : cl, stride = ids ? 1 : convPerOrient;
  const int count = ids ? nOC : (cl < nOC ? (nOC - cl + convPerOrient - 1) / convPerOrient : 0);
  double m, sacc;
  int idx;
  fold_ctf_rows(P, first, stride, count, ids, c, lane, m, sacc, idx);
  if (lane == 0 && idx != 0x7fffffff)
  {
    bioem_hip_prob_map pm = tab[(size_t) c * nMaps + p];
    if (pm.Constoadd < m)
    {
      pm.Total *= exp(-m + pm.Constoadd);
      pm.Constoadd = m;
      const Partial r = P[idx];
      const int ix = r.id / nd, iy = r.id - ix * nd;
      pm.max_prob_cent_x = -disp[ix];
      pm.max_prob_cent_y = -disp[iy];
      pm.max_prob_orient = ids ? ids[idx].x : orient0 + idx / convPerOrient;
      pm.max_prob_conv = c;
      const bioem_hip_param5 q = params[idx];
      const float sumref = sumRef[p];
      const float value = r.value;
      pm.max_prob_norm = -(-q.sumC * sumref + pd.Ntotpi * value) / (q.sumC * q.sumC - q.sumsquareC * pd.Ntotpi);
      pm.max_prob_mu = -(-q.sumC * value + q.sumsquareC * sumref) / (q.sumC * q.sumC - q.sumsquareC * pd.Ntotpi);
    }
    pm.Total += sacc * exp(m - pm.Constoadd);
    tab[(size_t) c * nMaps + p] = pm;
  }
}

// own-list pass: the rows of k_fold_own ([particle][list entry][CTF] flat order, the launch holds rows row0 ... row0 + nOC),
// one wave per (CTF, particle of [pFirst, pEnd)).  A particle's rows begin at a multiple of nCTF, so row row0 + oc is CTF
// (row0 + oc) % nCTF; max_prob_orient is the index in that particle's list.
__global__ __launch_bounds__(256) void k_fold_own_ctf(const Partial *__restrict__ partials, int nOC, int row0,
                                                      const int *__restrict__ off, int nCTF, int nMaps, int pFirst,
                                                      int pEnd, const bioem_hip_param5 *__restrict__ params,
                                                      const float *__restrict__ sumRef, const int *__restrict__ disp,
                                                      int nd, PD pd, bioem_hip_prob_map *__restrict__ tab)
{
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int nP = pEnd - pFirst;
  const long long pair = (long long) blockIdx.x * 4 + wave;
  if (pair >= (long long) nCTF * nP)
    return;
  const int c = (int) (pair / nP), p = pFirst + (int) (pair - (long long) c * nP);
  const long long g0 = (long long) off[p] * nCTF, g1 = (long long) off[p + 1] * nCTF;
  const int rb = (int) (max(g0, (long long) row0) - row0), re = (int) (min(g1, (long long) row0 + nOC) - row0);
  if (re <= rb)
    return;
  const int c0 = (int) (((long long) row0 + rb - g0) % nCTF); // CTF of the particle's first row in the launch
  const int first = rb + (c - c0 + nCTF) % nCTF;
  const int count = first < re ? (re - first + nCTF - 1) / nCTF : 0;
  double m, sacc;
  int idx;
  fold_ctf_rows(partials, first, nCTF, count, nullptr, c, lane, m, sacc, idx);
  if (lane == 0 && idx != 0x7fffffff)
  {
    bioem_hip_prob_map pm = tab[(size_t) c * nMaps + p];
    if (pm.Constoadd < m)
    {
      pm.Total *= exp(-m + pm.Constoadd);
      pm.Constoadd = m;
      const Partial r = partials[idx];
      const int ix = r.id / nd, iy = r.id - ix * nd;
      const int local = (int) ((long long) row0 + idx - g0); // k * nCTF + CTF
      pm.max_prob_cent_x = -disp[ix];
      pm.max_prob_cent_y = -disp[iy];
      pm.max_prob_orient = local / nCTF;
      pm.max_prob_conv = c;
      const bioem_hip_param5 q = params[idx];
      const float sumref = sumRef[p];
      const float value = r.value;
      pm.max_prob_norm = -(-q.sumC * sumref + pd.Ntotpi * value) / (q.sumC * q.sumC - q.sumsquareC * pd.Ntotpi);
      pm.max_prob_mu = -(-q.sumC * value + q.sumsquareC * sumref) / (q.sumC * q.sumC - q.sumsquareC * pd.Ntotpi);
    }
    pm.Total += sacc * exp(m - pm.Constoadd);
    tab[(size_t) c * nMaps + p] = pm;
  }
}

// the table as the reference initialises a particle entry (bioem.cpp:681-687)
__global__ void k_init_ctf_table(bioem_hip_prob_map *__restrict__ tab, size_t n)
{
  for (size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t) gridDim.x * blockDim.x)
  {
    bioem_hip_prob_map m;
    m.Total = 0.0;
    m.Constoadd = MIN_PROB;
    m.max_prob_cent_x = m.max_prob_cent_y = m.max_prob_orient = m.max_prob_conv = 0;
    m.max_prob_norm = m.max_prob_mu = 0.f;
    tab[i] = m;
  }
}

// ------------------------------------------------------------------------------------------------
// shard handles: the angle table never leaves the device
// ------------------------------------------------------------------------------------------------
__global__ void k_init_angles(bioem_hip_prob_angle *__restrict__ pang, size_t n)
{ // bioem.cpp:688-697
  for (size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t) gridDim.x * blockDim.x)
  {
    bioem_hip_prob_angle a;
    a.forAngles = 0.0;
    a.ConstAngle = MIN_PROB;
    pang[i] = a;
  }
}

// order of the reference's std::pair<double, int> heap items (bioem.cpp:1254-1256)
__host__ __device__ inline bool cand_less(double la, int ia, double lb, int ib)
{
  return la < lb || (la == lb && ia < ib);
}

// the writer's key of a table entry (bioem.cpp:1262): every pass of k_topk_angles forms it here, so that equal table
// entries give equal bits wherever they are met
__device__ inline double cand_key(const bioem_hip_prob_angle &pa, double numconst)
{
  return log(pa.forAngles) + pa.ConstAngle + numconst;
}

__device__ inline bioem_hip_angle_candidate cand_make(const bioem_hip_prob_angle &pa, double logp, int orient)
{
  bioem_hip_angle_candidate c;
  c.forAngles = pa.forAngles;
  c.ConstAngle = pa.ConstAngle;
  c.logp = logp;
  c.orient = orient;
  c.pad = 0;
  return c;
}

__device__ inline bioem_hip_angle_candidate cand_unused()
{
  bioem_hip_angle_candidate c;
  c.forAngles = 0.;
  c.ConstAngle = MIN_PROB;
  c.logp = -INFINITY;
  c.orient = -1;
  c.pad = 0;
  return c;
}

// K best orientations per particle among the nO owned ones, by the reference writer's own rule (bioem.cpp:1251-1286):
// walk the orientations in order; fill a K-entry set; afterwards an entry replaces the set's minimum (by (logp,
// orientation)) when the minimum's logp is strictly below its own.  One thread per particle: the table is
// orientation-major, so the 64 particles of a wave read consecutive 16-byte entries of one orientation row.  The set
// lives in the thread's first K output slots; replacements are rare (~K ln(nO/K) per particle), each followed by a scan
// of the K slots for the new minimum.  Slots 0 ... K-1 sorted best first (descending (logp, orientation), the order in
// which the reference prints after emptying its heap).
// A particle owns W >= K slots.  With W > K a second walk adds what a LATER walk over a longer list could still have
// kept from this block: with t the smallest key of the set, the entries of key t among the first K entries of key >= t
// that the first walk rejected or evicted (at most K - 1), in ascending orientation from slot K on.  The writer's loop
// over the shards' lists of width 2K - 1, in orientation order, is the writer's loop over the whole table;
// K slots are enough only while no equal keys meet a shard's threshold.  Unused slots: (0, MIN_PROB, -inf, -1).
__global__ void k_topk_angles(const bioem_hip_prob_angle *__restrict__ pang, int nO, int nMaps, int o0, int K, int W,
                              double numconst, bioem_hip_angle_candidate *__restrict__ out)
{
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= nMaps)
    return;
  bioem_hip_angle_candidate *mine = out + (size_t) p * W;
  int cnt = 0, minSlot = 0;
  double minLogp = 0.;
  int minIo = 0;
  for (int io = 0; io < nO; io++)
  {
    const bioem_hip_prob_angle pa = pang[(size_t) io * nMaps + p];
    const double logp = cand_key(pa, numconst);
    bool rescan = false;
    if (cnt < K)
    {
      mine[cnt++] = cand_make(pa, logp, o0 + io);
      rescan = cnt == K;
    }
    else if (minLogp < logp)
    {
      mine[minSlot] = cand_make(pa, logp, o0 + io);
      rescan = true;
    }
    if (rescan)
    {
      minSlot = 0;
      minLogp = mine[0].logp;
      minIo = mine[0].orient;
      for (int j = 1; j < K; j++)
      {
        const double l = mine[j].logp;
        const int i = mine[j].orient;
        if (cand_less(l, i, minLogp, minIo))
        {
          minSlot = j;
          minLogp = l;
          minIo = i;
        }
      }
    }
  }
  // best first
  for (int a = 0; a < cnt; a++)
  {
    int best = a;
    for (int b = a + 1; b < cnt; b++)
      if (cand_less(mine[best].logp, mine[best].orient, mine[b].logp, mine[b].orient))
        best = b;
    if (best != a)
    {
      const bioem_hip_angle_candidate t = mine[a];
      mine[a] = mine[best];
      mine[best] = t;
    }
  }
  for (int a = cnt; a < K; a++)
    mine[a] = cand_unused();
  if (W == K)
    return;
  // second walk: the set is full only when the block holds more than K - 1 entries; minLogp is then its threshold t
  int extra = K;
  if (cnt == K && nO > K)
  {
    int seen = 0; // entries of key >= t met so far
    for (int io = 0; io < nO && seen < K && extra < W; io++)
    {
      const bioem_hip_prob_angle pa = pang[(size_t) io * nMaps + p];
      const double logp = cand_key(pa, numconst);
      if (logp < minLogp)
        continue;
      seen++;
      if (logp != minLogp)
        continue;
      bool kept = false;
      for (int j = 0; j < K; j++)
        kept = kept || mine[j].orient == o0 + io;
      if (!kept)
        mine[extra++] = cand_make(pa, logp, o0 + io);
    }
  }
  for (int a = extra; a < W; a++)
    mine[a] = cand_unused();
}

// fold of the gathered shards' map entries (bioem.cpp:909-994 restated for one address space): shard s's entries start
// at gathered + s * stride bytes.  Maximum Constoadd wins; ties go to the LOWEST shard (= lowest orientation block,
// the serial first-maximum semantics); Total = sum over shards of Total_s * exp(Constoadd_s - max), in shard order.
__global__ void k_merge_shards(const unsigned char *__restrict__ gathered, int nShards, size_t stride, int nMaps,
                               bioem_hip_prob_map *__restrict__ out)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nMaps)
    return;
  int who = 0;
  double cmax = reinterpret_cast<const bioem_hip_prob_map *>(gathered)[i].Constoadd;
  for (int s = 1; s < nShards; s++)
  {
    const double c = reinterpret_cast<const bioem_hip_prob_map *>(gathered + (size_t) s * stride)[i].Constoadd;
    if (c > cmax)
    {
      cmax = c;
      who = s;
    }
  }
  double tot = 0.;
  for (int s = 0; s < nShards; s++)
  {
    const bioem_hip_prob_map m = reinterpret_cast<const bioem_hip_prob_map *>(gathered + (size_t) s * stride)[i];
    tot += m.Total * exp(m.Constoadd - cmax);
  }
  bioem_hip_prob_map o = reinterpret_cast<const bioem_hip_prob_map *>(gathered + (size_t) who * stride)[i];
  o.Total = tot;
  o.Constoadd = cmax;
  out[i] = o;
}

} // namespace

#endif
