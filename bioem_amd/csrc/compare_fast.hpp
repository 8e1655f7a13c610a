// compare_fast.hpp -- fast comparison kernel (output-pruned 2-D transform fused with the posterior) + Nyquist rows
// Part of libbioem_hip.so; included by bioem_hip.hip and by every kernels_*.hip unit of a comparison family (its
// helpers serve them all; anonymous namespace).
#ifndef BIOEM_COMPARE_FAST_HPP
#define BIOEM_COMPARE_FAST_HPP

#include <type_traits>

namespace
{

// wave-uniform table reads through the constant address space: always scalar loads (the uniform global loads of this
// kernel were otherwise emitted as vector loads, one L2 round trip each)
typedef const float2 __attribute__((address_space(4))) *const_float2_ptr;
__device__ __forceinline__ const_float2_ptr as_constant(const float2 *p)
{
  return (const_float2_ptr) (unsigned long long) p;
}

// A wave-uniform pointer, provably so for the compiler: the 64-bit address arithmetic behind it (base + index * size)
// is done on the vector unit, and a buffer descriptor built from a value the compiler keeps in vector registers makes
// EVERY buffer load a waterfall loop (4 v_readfirstlane + 2 v_cmp + exec juggling per load; found in all
// k_compare_wide2 instantiations of round 2).  Two v_readfirstlane here put it into scalar registers once.
template <typename T>
__device__ __forceinline__ T *uniform_ptr(T *p)
{
  const unsigned long long v = (unsigned long long) p;
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned) v);
  const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned) (v >> 32));
  return (T *) (((unsigned long long) hi << 32) | lo);
}

// ------------------------------------------------------------------------------------------------
// log of a positive float in double precision, cheap: f = m * 2^e, m in [1,2); c ~ 1/m from a 64-entry
// table, r = m*c - 1 exactly rounded by one fma (|r| <= 2^-7), log f = e ln2 - log c + log1p(r) with a
// degree-6 Taylor polynomial (truncation 2^-49/7).  Absolute error ~1e-15, i.e. < 3e-11 after the
// (3-Np)/2 amplification -- far below the float narrowing the reference applies to logpro.
// Table entry = {c, -log(c)} in LDS.
// ------------------------------------------------------------------------------------------------
__device__ __noinline__ double log_slow_path(float f) { return log((double) f); }

__device__ __forceinline__ double log_of_float(float f, const double2 *ltab)
{
  const unsigned int bits = __float_as_uint(f);
  if (!(f > 1.1754944e-38f) || bits >= 0x7f800000u) // zero, negative, subnormal, inf, nan: exact slow path
    return log_slow_path(f);
  const int e = (int) (bits >> 23) - 127;
  const float m = __uint_as_float((bits & 0x007fffffu) | 0x3f800000u);
  const double2 t = ltab[(bits >> 17) & 63];
  const double r = fma((double) m, t.x, -1.0);
  double p = fma(r, -1.0 / 6.0, 1.0 / 5.0);
  p = fma(r, p, -1.0 / 4.0);
  p = fma(r, p, 1.0 / 3.0);
  p = fma(r, p, -1.0 / 2.0);
  p = fma(r * r, p, r);
  return fma((double) e, 0.693147180559945309417232, t.y + p);
}

// exp of a non-positive double difference through the hardware exp2 (relative error ~2e-7 per term; the
// terms are summed in double, so log(Total) moves by < 1e-6)
__device__ __forceinline__ double exp_fast_nonpos(double x) { return (double) __expf((float) x); }

struct LseF
{
  float m;
  double s;
  int id;
  float val;
};

__device__ __forceinline__ void lsef_push(LseF &L, double lp, int id, float val, int algo)
{
  const float lpf = (float) lp;
  const double lpe = (algo == 1) ? (double) lpf : lp;
  if (L.m < lpf)
  {
    L.s = (L.m == -INFINITY) ? 0. : L.s * exp_fast_nonpos((double) L.m - (double) lpf);
    L.m = lpf;
    L.id = id;
    L.val = val;
  }
  else if (L.m == lpf && id < L.id)
  { // equal maxima: the first VISITED displacement wins (ids are visiting ranks; a lane may push out of order)
    L.id = id;
    L.val = val;
  }
  L.s += exp_fast_nonpos(lpe - (double) L.m);
}

__device__ __forceinline__ void lsef_wave_reduce(LseF &L)
{
  for (int off = 32; off > 0; off >>= 1)
  {
    const float m2 = __shfl_xor(L.m, off);
    const double s2 = __shfl_xor(L.s, off);
    const int id2 = __shfl_xor(L.id, off);
    const float v2 = __shfl_xor(L.val, off);
    if (m2 > L.m || (m2 == L.m && id2 < L.id))
    {
      const double sc = (L.m == -INFINITY) ? 0. : L.s * exp_fast_nonpos((double) L.m - (double) m2);
      L.s = sc + s2;
      L.m = m2;
      L.id = id2;
      L.val = v2;
    }
    else
    {
      const double sc = (m2 == -INFINITY) ? 0. : s2 * exp_fast_nonpos((double) m2 - (double) L.m);
      L.s += sc;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// Posterior of a BATCH of B displacements of one lane (bioem_algorithm.h:18-123), written so that the B evaluations are
// independent straight-line chains the scheduler can interleave (one basic block):
//   * cc = acc / N^2 exactly as the reference divides (bioem_algorithm.h:163-164), but as q = a*r, q' = q + r*(a - q*b)
//     with r = RN(1/b): correctly rounded for a correctly rounded reciprocal (Markstein), 3 instructions instead of the
//     11 of the generic IEEE division sequence;
//   * the log-table lookups of all B values are issued together; the exact slow path (non-positive / non-finite
//     argument) is ONE wave-uniform branch per batch instead of a call site per value;
//   * log-sum-exp per batch: the batch maximum first (first visited displacement wins among equal float maxima, as in
//     lsef_push), ONE rescale of the running sum, then B independent exponentials.
// ------------------------------------------------------------------------------------------------
struct PostW
{
  float Np, nn, rnn; // Ntotpi, N^2 and RN(1 / N^2)
  float k0, k1, k2, k3; // sumsqref*sumsquareC, 2*sumref*sumC, sumsqref*sumC*sumC, sumref*sumref*sumsquareC
  double A, t2, prior;
};

__device__ __forceinline__ PostW post_consts(float Np, int N, const bioem_hip_param5 &q, float sumref, float sumsqref,
                                             double t2, double prior)
{
  PostW w;
  w.Np = Np;
  w.nn = (float) (N * N);
  w.rnn = 1.0f / w.nn;
  // sub-expressions of bioem_algorithm.h:32-36 in the reference's association order
  w.k0 = sumsqref * q.sumsquareC;
  w.k1 = 2 * sumref * q.sumC;
  w.k2 = sumsqref * q.sumC * q.sumC;
  w.k3 = sumref * sumref * q.sumsquareC;
  w.A = (double) (3 - Np) * 0.5;
  w.t2 = t2;
  w.prior = prior;
  return w;
}

__device__ __forceinline__ float div_by_nn(float a, const PostW &w)
{
  const float q = a * w.rnn;
  const float r = fmaf(-q, w.nn, a);
  return fmaf(r, w.rnn, q);
}

template <int B>
__device__ __forceinline__ void posterior_batch(LseF &L, const float (&acc)[B], const int (&id)[B], const bool (&ok)[B],
                                                const PostW &w, const double2 *ltab, int algo)
{
  float cc[B], fe[B];
  bool bad = false;
#pragma unroll
  for (int v = 0; v < B; v++)
  {
    cc[v] = div_by_nn(acc[v], w);
    // bioem_algorithm.h:32-36, float expression in the reference's order
    const float f = w.Np * (w.k0 - cc[v] * cc[v]) + w.k1 * cc[v] - w.k2 - w.k3;
    fe[v] = ok[v] ? f : 1.f;
    bad = bad || !(fe[v] > 1.1754944e-38f) || __float_as_uint(fe[v]) >= 0x7f800000u;
  }
  double lg[B];
  if (__builtin_expect(__any(bad), 0))
  { // some lane of the wave holds a non-positive / non-finite argument: the exact per-value path
#pragma unroll
    for (int v = 0; v < B; v++)
      lg[v] = log_of_float(fe[v], ltab);
  }
  else
  {
    double2 t[B];
#pragma unroll
    for (int v = 0; v < B; v++)
      t[v] = ltab[(__float_as_uint(fe[v]) >> 17) & 63];
#pragma unroll
    for (int v = 0; v < B; v++)
    { // same arithmetic as log_of_float
      const unsigned int bits = __float_as_uint(fe[v]);
      const int e = (int) (bits >> 23) - 127;
      const float m = __uint_as_float((bits & 0x007fffffu) | 0x3f800000u);
      const double r = fma((double) m, t[v].x, -1.0);
      double p = fma(r, -1.0 / 6.0, 1.0 / 5.0);
      p = fma(r, p, -1.0 / 4.0);
      p = fma(r, p, 1.0 / 3.0);
      p = fma(r, p, -1.0 / 2.0);
      p = fma(r * r, p, r);
      lg[v] = fma((double) e, 0.693147180559945309417232, t[v].y + p);
    }
  }
  float lpf[B];
  double lpe[B];
#pragma unroll
  for (int v = 0; v < B; v++)
  {
    double lp = w.A * lg[v] + w.t2;
    lp -= w.prior;
    lpf[v] = ok[v] ? (float) lp : -INFINITY;
    lpe[v] = (algo == 1) ? (double) lpf[v] : lp;
  }
  // batch maximum; among equal maxima the first VISITED displacement (smallest id) wins
  float mb = lpf[0], vb = cc[0];
  int ib = ok[0] ? id[0] : 0x7fffffff;
#pragma unroll
  for (int v = 1; v < B; v++)
  {
    const bool t = ok[v] && (lpf[v] > mb || (lpf[v] == mb && id[v] < ib));
    mb = t ? lpf[v] : mb;
    ib = t ? id[v] : ib;
    vb = t ? cc[v] : vb;
  }
  const bool take = mb > L.m || (mb == L.m && ib < L.id);
  const float newm = fmaxf(L.m, mb);
  // running sum rescaled once (exp(-inf) = 0 restarts an empty sum; equal maxima: factor 1 without an exponential)
  double sum = (L.m == newm) ? L.s : L.s * exp_fast_nonpos((double) L.m - (double) newm);
#pragma unroll
  for (int v = 0; v < B; v++)
  {
    const double e = exp_fast_nonpos(lpe[v] - (double) newm);
    sum += ok[v] ? e : 0.;
  }
  L.s = sum;
  L.m = newm;
  L.id = take ? ib : L.id;
  L.val = take ? vb : L.val;
}

// block -> (particle, group of 4 orientation*CTF).  Workgroups go round-robin over the 8 XCDs (each with its own L2).
//   a.pchunk > 0: particle chunks of a.pchunk; inside a chunk the particle index runs fastest, then the group.  With a
//     chunk size that is a multiple of 8 a particle always lands on the same XCD, and the ~96 blocks resident per XCD
//     cover (pchunk/8 particles) x (a few groups): every particle line is then shared through that XCD's L2 by several
//     groups and every conv line by pchunk/8 particles, instead of each particle line being fetched from Infinity
//     Cache/HBM once per group.
//   a.pchunk < 0 (few particles): group g goes to XCD g % 8 with ALL its particles (grid padded to a multiple of 8
//     groups).  With 20 particles the chunk order would spread the 20 blocks of a group over all 8 XCDs, i.e. fetch
//     every conv line into 8 L2s for 2.5 blocks each (measured: 8 GB per launch from the fabric, 33 M/s); the particle
//     spectra are few enough to sit in every L2.
__device__ __forceinline__ bool fast_block_pair(const CompareArgs &a, int &p, int &ocg)
{
  const int ocGroups = (a.nOC + 3) >> 2;
  if (a.pchunk < 0)
  {
    const int x = blockIdx.x & 7, q = blockIdx.x >> 3;
    ocg = (q / a.nMaps) * 8 + x;
    p = q % a.nMaps;
    return ocg < ocGroups;
  }
  const int per = a.pchunk * ocGroups;
  int c = blockIdx.x / per;
  const int nch = (a.nMaps + a.pchunk - 1) / a.pchunk;
  c = min(c, nch - 1);
  const int rem = blockIdx.x - c * per;
  const int pc = min(a.pchunk, a.nMaps - c * a.pchunk);
  ocg = rem / pc;
  p = c * a.pchunk + (rem - ocg * pc);
  return true;
}

// Window accumulation over one block of 64 frequency columns held in LDS as Tl[row = dx + WD][64] float2
// (already weighted by 1 or 2 per column; zero beyond H).  lane = (iy, group); a group owns `nr` consecutive
// displacement rows so that each LDS twiddle read E[ky*dy] feeds nr accumulators; T is read two columns
// at a time (ds_read_b128).  STATIC: nr == NR known at compile time (the +-10 px, grid 1 case).
// NP = number of column pairs: 32 for a block, 1 for the Nyquist column parked in the pad columns 64/65.
// npairs <= NP: column pairs that hold columns of the spectrum (the last block of a size like 224, 160 is not full; the
// columns beyond are zeros whose terms leave every accumulator unchanged, so skipping them is bit-identical).
// (NA >= NR accumulators in the caller's array: the kernels whose static window takes window_accumulate_sym hold 8)
template <int NR, bool STATIC, int NP, int TS, int NA>
__device__ __forceinline__ void window_accumulate(const float2 *Tl, const float2 *twl, int N, int step, int idx0,
                                                  const int (&rowoff)[NR], int nr, float (&acc)[NA], int npairs = NP)
{
  static_assert(NA >= NR, "one accumulator per row of the lane");
  int idx = idx0;
#pragma unroll 2
  for (int kp = 0; kp < npairs; kp++)
  {
    const float2 w0 = twl[idx];
    idx += step;
    if (idx >= N)
      idx -= N;
    const float2 w1 = twl[idx];
    idx += step;
    if (idx >= N)
      idx -= N;
#pragma unroll
    for (int r = 0; r < NR; r++)
    {
      if (STATIC || r < nr)
      {
        // STATIC: the nr rows of a lane are consecutive (unit grid), so one base + compile-time offsets
        const float4 t = *reinterpret_cast<const float4 *>(&Tl[(STATIC ? rowoff[0] + r * TS : rowoff[r]) + 2 * kp]);
        float v = acc[r];
        v = fmaf(t.x, w0.x, v);
        v = fmaf(-t.y, w0.y, v);
        v = fmaf(t.z, w1.x, v);
        v = fmaf(-t.w, w1.y, v);
        acc[r] = v;
      }
    }
  }
}

// Static 21-row window, the same sums over |dy|.  The twiddle of column ky and displacement dy is
// cos(2 pi ky dy / N) + i sin(2 pi ky dy / N), so with
//   A[dx][|dy|] = sum_ky Re T[dx][ky] cos(2 pi ky |dy| / N),   B[dx][|dy|] = sum_ky Im T[dx][ky] sin(2 pi ky |dy| / N)
// cc[dx][+|dy|] = A - B and cc[dx][-|dy|] = A + B: two FMAs per column serve two displacements.  lane = (dx row 0..20,
// group g = 0..2) = 3 row + g; group g owns |dy| = 4 g .. 4 g + 3 window rows (7 + 8 + 6 displacements; the fourth
// entry of group 2 is the table's row of zeros, lane 63 idles), acc[j] = A and acc[4 + j] = B of |dy| = 4 g + j.  Per
// column pair a lane reads its own T row once and four table entries {cos, sin, cos, sin} (compare_args.hpp): every
// address is a lane constant plus an immediate, no per-lane walk through the twiddle table.  The table read has three
// addresses per wave (broadcast).  The T read of row r starts at bank 4 r mod 64 (TS = 66); the four 16-lane groups of
// a 128-bit LDS read each hold at most 8 rows, no two of them 16 apart: no conflict.
template <int TS>
__device__ __forceinline__ void window_accumulate_sym(const float2 *Trow, const float4 *tab, float (&acc)[8], int npairs)
{
#pragma unroll 2
  for (int kp = 0; kp < npairs; kp++)
  {
    const float4 t = *reinterpret_cast<const float4 *>(&Trow[2 * kp]);
#pragma unroll
    for (int j = 0; j < 4; j++)
    {
      const float4 w = tab[kp * kSymEntries + j];
      float va = acc[j], vb = acc[4 + j];
      va = fmaf(t.x, w.x, va);
      vb = fmaf(t.y, w.y, vb);
      va = fmaf(t.z, w.z, va);
      vb = fmaf(t.w, w.w, vb);
      acc[j] = va;
      acc[4 + j] = vb;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// fast comparison kernel: N = R*N1 with R = 32, 16, 8, 4 or 2 (the largest of those dividing N, i.e. any even N),
// 2*maxD+1 <= 2*WD+1 <= 31.
// block = 4 waves = 4 consecutive (orientation*CTF) indices of ONE particle (the particle columns are then
// served to waves 1..3 from L1); blockIdx.x = ocGroup * nMaps + particle, so concurrently resident blocks
// share the same 4 conv spectra in L2.  Columns are processed in blocks of 64 (lane = column): register
// FFTs -> T block in LDS -> window accumulation, so the LDS footprint per wave is (2*WD+1)*64*8 bytes
// (10.5 KiB for +-10 px => 3 blocks per CU, matching the VGPR-limited 3 waves per SIMD).
// ------------------------------------------------------------------------------------------------
// register FFT: radix-2 decimation in time with 6-op butterflies for power-of-two lengths, mixed radix otherwise;
// inputs go to the (bit- or digit-) reversed position, outputs come out in natural order
#define FFT_IN(k) (is_pow2(R) ? bitrevR<R>(k) : DIGITREV<R>.pos[k])
#define FFT_OUT(n) (n)
#define FFT_RUN(xr, xi)                                                                                            \
  do                                                                                                               \
  {                                                                                                                \
    if constexpr (is_pow2(R))                                                                                      \
      fft_inverse_dit<R>(xr, xi);                                                                                  \
    else                                                                                                           \
      fft_inverse_mixed<R>(xr, xi);                                                                                \
  } while (0)
// NYQ (N/2 a multiple of 64, e.g. 128 and 256): the half spectrum has N/2 + 1 columns, one more than fills the
// 64-lane column blocks, and a whole extra block pass for that single Nyquist column would cost 1/2 (128) or 1/3
// (256) of the kernel.  Instead k_nyquist_rows (below) forms the 2*WD+1 column-transform outputs of that column
// for every comparison of the launch by direct summation, and this kernel adds (-1)^dy * Re T[dx][N/2] to its
// window sums (FFTW c2r convention: weight 1, real part only).  The tail is deliberately tiny: anything larger
// (an inlined or called summation) pushes the register allocation of the main loop into scratch.
// GS (1..4): row stride of the window in pixels.  T row m (-WD..WD) holds displacement dx = m*GS, so a coarse
// DISPLACE_CENTER grid whose offsets are all multiples of GS reaches +-15*GS pixels with the same 2*WD+1 rows.
// (27- and 31-row windows: k_compare_fastm, compare_fastm.hpp)
// ARGS: CompareArgs, the all-to-all launch (every particle against every row), or OwnCompareArgs, ONE launch over a batch
// of the own-list pass, rows whose particles differ (kernels_fast_own.hip; the API's label "k_compare_fast_own<...>").
// The variant is a template parameter of the kernel itself and differs at the three sites marked OWN -- the
// block-to-work mapping and the index that addresses the per-row buffers -- never a wrapper around a shared body: that
// changes the code of every instantiation.  Everything a wave computes for a (particle, row) pair is the
// same arithmetic in the same order, so a row's partial equals the per-particle launch's bit for bit.
// LEAN: the instantiation of ONE path through this kernel, the launch of the whole static 21-row window with no split
// last block (the headline launch): symw is a compile-time true, split a compile-time false, and the general window pass,
// the twiddle copy, the general posterior branch and the split block are not instantiated.  The host takes it exactly
// where the run-time tests below would take that path (lean_launch_ok, bioem_hip.hip); what a wave computes is the full
// instantiation's arithmetic in its order, bit for bit.  The paths never taken cost the full instantiation 18 vector
// registers and 47 scalar spills into vector lanes, with 17 lane moves inside the k1 loop (<10, 16, false, 1>).
template <int WD, int R, bool NYQ, int GS, class ARGS = CompareArgs, bool LEAN = false>
__global__ __launch_bounds__(256, 3) void k_compare_fast(const ARGS a)
{
  constexpr bool OWN = !std::is_same<ARGS, CompareArgs>::value;
  static_assert(!LEAN || sym_window_ok(WD, R, NYQ, GS), "the lean variant is the static window pass over |dy| alone");
  static_assert(WD <= 10, "windows of at most 21 rows; 27 / 31 rows: k_compare_fastm");
  constexpr int NW = 2 * WD + 1;
  constexpr int R2 = R / 2;            // rows (k2 pairs) per k1 step
  // depth of the operand ring: must divide R2 so that a ring slot is a compile-time function of the k2 pair
  // (R = 30: a ring of 3, not 5 -- 16 registers the 21-row window of that length needs)
  constexpr int RD = (R2 % 4 == 0) ? 4 : (R2 == 15) ? 3 : (R2 % 5 == 0) ? 5 : (R2 % 3 == 0) ? 3 : (R2 % 2 == 0) ? 2 : 1;
  constexpr int NR = (WD <= 5) ? 3 : 7; // accumulators (window rows) per lane
  // T row stride in float2 (64 columns + 2 pad: row groups land on different banks)
  constexpr int TS = 66;
  // the static 21-row window runs the pass over |dy| (window_accumulate_sym): 8 accumulators per lane, and the head of
  // the LDS holds the slice of the cos | sin table for the current column block instead of the twiddles
  constexpr bool SYM = sym_window_ok(WD, R, NYQ, GS);
  constexpr int NA = SYM ? 8 : NR;
  extern __shared__ __align__(16) unsigned char smem[];
  const int N = a.N, H = a.H, N1 = a.N1;
  const size_t headBytes = fast_head_bytes(N, SYM);
  float2 *twl = reinterpret_cast<float2 *>(smem);                 // N+1 (+pad), or the table slice
  int *displ = reinterpret_cast<int *>(smem + headBytes);         // nd ints (256 B reserved)
  double2 *ltab = reinterpret_cast<double2 *>(smem + headBytes + 256); // 64 entries
  float2 *Tall = reinterpret_cast<float2 *>(smem + headBytes + 256 + 1024);
  // wave index made provably uniform (SGPR) so that per-wave base pointers use scalar addressing
  const int wave = __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6));
  const int lane = threadIdx.x & 63;
  float2 *Tl = Tall + (size_t) wave * NW * TS;

  int *dinv = displ + 32; // visiting rank of window row m (displacement m*GS), index m + mD
  const int mD = LEAN ? WD : a.maxD / GS;
  // (the rows -WD..WD, all of them: what is_static below says of a 21-row window)
  const bool symw = LEAN || (SYM && a.nd == NW && mD == WD);
  if constexpr (!LEAN)
    if (!symw)
      for (int t = threadIdx.x; t <= N; t += blockDim.x)
        twl[t] = a.tw[t];
  for (int t = threadIdx.x; t < a.nd; t += blockDim.x)
  {
    const int dv = a.disp[t];
    displ[t] = dv;
    const int m = dv / GS + mD;
    if (m >= 0 && m < 32)
      dinv[m] = t;
  }
  for (int t = threadIdx.x; t < 64; t += blockDim.x)
    ltab[t] = a.ltab[t];
  __syncthreads();

  // block -> (particle, group of 4 orientation*CTF): particle chunks of a.pchunk; inside a chunk the particle index
  // runs fastest, then the group.  Workgroups go round-robin over the 8 XCDs, so with a chunk size that is a
  // multiple of 8 a particle always lands on the same XCD, and the ~96 blocks resident per XCD cover
  // (pchunk/8 particles) x (a few groups): every particle line is then shared through that XCD's L2 by several
  // groups and every conv line by pchunk/8 particles, instead of each particle line being fetched from Infinity
  // Cache/HBM once per group.
  // OWN: block -> one entry of the block table, {particle, first row, end row, 0} (compare_args.hpp).  blockIdx is
  // uniform, the table is read through the constant address space: scalar loads.  The host builds the table
  // (own_block_table, bioem_hip.hip): every entry lies inside the launch.
  int p, ocFirst, ocEnd; // the block's rows: [ocFirst, ocEnd), at most four
  if constexpr (OWN)
  {
    const own_i32x4 be = *((const_int4_ptr) (unsigned long long) (a.blocks + blockIdx.x));
    p = be.x;
    ocFirst = be.y;
    ocEnd = be.z;
  }
  else
  {
    int ocg;
    if (!fast_block_pair(a, p, ocg))
      return;
    ocFirst = ocg * 4;
    ocEnd = a.nOC;
  }
  const int oc_raw = ocFirst + wave;
  const bool oc_valid = oc_raw < ocEnd;
  const int oc = oc_valid ? oc_raw : ocEnd - 1;
  const int Hp = a.Hp; // row-pair pitch in 16-byte words (H ... H + 15: comparison_pitch in bioem_hip.hip)
  const size_t M = (size_t) N * Hp;
  // buffer descriptors built from wave-uniform values only (blockIdx / readfirstlane'd wave id)
  const auto rsrcF = __builtin_amdgcn_make_buffer_rsrc(uniform_ptr(const_cast<float2 *>(a.ref + (size_t) p * M)), 0,
                                                       (int) (M * sizeof(float2)), 0x00020000);
  // STRIP (strip lanes, below; the lean kernels of 16 k points): ONE conv descriptor for the block, based at its first
  // row and covering its sRows rows
  constexpr bool STRIP = LEAN && R2 % 8 == 0;
  const int sRows = STRIP ? min(4, ocEnd - ocFirst) : 1;
  const auto rsrcC = __builtin_amdgcn_make_buffer_rsrc(
      uniform_ptr(const_cast<float2 *>(a.conv + (size_t) (STRIP ? ocFirst : oc) * M)), 0,
      (int) ((STRIP ? (size_t) sRows : (size_t) 1) * M * sizeof(float2)), 0x00020000);

  // window lanes (LEAN reads none of the general pass's: G ... rowbase stay unreferenced there)
  const int nd = LEAN ? NW : a.nd;
  const int G = 64 / nd;
  const int nr = (nd + G - 1) / G;
  const int iy = lane % nd, grp = lane / nd;
  const bool wactive = grp < G;
  const int dy = displ[iy];
  const int step = dy < 0 ? dy + N : dy;
  // static window (the +-10 px, grid 1 case): the window rows are -mD..mD and every lane group owns exactly
  // NR CONSECUTIVE rows of it in sorted order, whatever the visiting order of the algorithm (ALGO 1 visits
  // 0..maxD, -maxD..-1); dinv[] translates back to visiting ranks for the arg-max bookkeeping
  const bool is_static = (nr == NR) && (nd == G * NR) && (nd == 2 * mD + 1);
  float acc[NA];
#pragma unroll
  for (int r = 0; r < NA; r++)
    acc[r] = 0.f;
  // window_accumulate_sym: lane = 3 * row + group (lane 63 reads row 20 and is dropped later)
  const int srow = min(lane / 3, NW - 1), sgrp = lane % 3;
  const float2 *Trow = Tl + srow * TS;
  const float4 *stab = reinterpret_cast<const float4 *>(smem) + sgrp * 4;
  const float2 *symsrc = a.tw + sym_table_offset(N) + threadIdx.x;
  // T row (in float2 units) of accumulator r of this lane; idle lanes (grp >= G) read rows 0.. and are dropped
  // later.  Only the first is kept live across the column loop: the static window uses base + r*TS, the general
  // one re-reads its rows from the displacement list per block.
  auto row_of = [&](int r) -> int {
    int ix = wactive ? grp * nr + r : r;
    if (ix >= nd)
      ix = nd - 1;
    return (displ[ix] / GS + WD) * TS;
  };
  const int rowbase = is_static ? ((wactive ? grp : 0) * NR - mD + WD) * TS : row_of(0);

  const int nblk = NYQ ? (H - 1 + 63) / 64 : (H + 63) / 64; // (Nyquist split: whole blocks, or a last one of 32 columns)
  // Operand stream (software pipelined across k1 iterations AND column blocks): the (k1, k2-pair) loads of a
  // lane walk t = k1*16 + k2p with a constant stride of H float4; a 4-deep ring of (F, C) pairs keeps 8 dwordx4
  // loads (8 KiB per wave) in flight, re-issued as soon as a slot is consumed.  The ring runs on into the first
  // rows of the NEXT column block, so those loads fly during the T exchange / window phase of this block.
  // Addressing: buffer loads -- 128-bit descriptor (SGPRs), one 32-bit lane offset (VGPR), row offset in an SGPR.
  const unsigned rowbytes = (unsigned) Hp * 16u;
  // Split last block (a.split: it holds at most 32 columns, e.g. 17 of the 81 at 160^2): lane l and lane l + 32 take the
  // SAME column, the low half the k1 steps 0 .. sHalf - 1, the high half sHalf .. N1 - 1 (one past the end with an odd
  // N1: those rows lie beyond the buffer and read as zeros).  Inside the loop both halves use the low half's
  // recombination twiddles -- wave-uniform as everywhere --, w^(dx (k1 + sHalf)) = w^(dx k1) w^(dx sHalf): the high half's
  // sums are turned by w^(dx sHalf) once, after the loop, and the halves added with v_permlane32_swap.  The pass then
  // costs sHalf instead of N1 steps: 1.5 instead of 2 passes at 160^2.
  constexpr bool SPLIT_OK = !LEAN && !(NYQ && R == 32); // (the 32-point Nyquist kernels have no registers left for it)
  const int sHalf = (N1 + 1) >> 1;
  const int hsel = lane >> 5;
  const unsigned halfoff = (unsigned) (hsel * sHalf * R2) * rowbytes;
  // STRIP, strip lanes: during the column pass a lane is (row sq of the block, column sc of a 16-column strip), and in
  // column block b wave w takes columns 64 b + 16 w + sc of ALL rows of the block: the same 64 columns x 4 rows per
  // block, the same k1 steps per wave, and for every (row, column) the arithmetic of the lane = column mapping in its
  // order (the recombination twiddles are wave-uniform either way).  What changes is who asks for the operands.
  //   conv      every lane, through the block's descriptor: lane offset = row sqc M 8 + column 16, sqc = sq clamped to
  //             the block's last row (a ragged last group computes that row again, as a clamped wave does); a request is
  //             four 256-byte runs, eight 128-byte lines as before.
  //   particle  ONE request per group of four row pairs: lane (sq, sc) asks for column sc of row pair 4 g + sq, so a
  //             request is again four 256-byte runs, all of it wanted, a quarter as many requests per wave and per block
  //             a quarter of the L1 accesses (the four waves no longer ask for the same 1 KiB each).  A landed group goes
  //             with one ds_write_b128 (lane l at byte 16 l: row pair r of the group at 256 r + 16 sc) into one of two
  //             1 KiB slots at the head of the wave's OWN T region Tl, idle during the k1 loop, and every lane reads row
  //             pair t + 2 back at (slot, row pair, sc) -- four lanes per address, an LDS broadcast -- into the registers
  //             the product of row pair t has just released.
  // Groups: a step of R2 = 8 row pairs is two groups, so slot and register of a group are compile-time functions of k2p.
  // In the iteration of row pair t = 4 g group g + 1 (requested eight iterations earlier) is written to slot (g + 1) % 2
  // -- whose last reader, row pair 4 g - 1, was read back at t - 3 -- and group g + 3 requested into its registers.
  // No new barrier: Tl of wave w is read by wave w alone (window pass), other waves write it only between the two
  // barriers of a block, the first of which follows every wave's k1 loop (whose last read-backs are in registers by
  // then: the barrier waits for them); in between the scratch is written and read by one wave in its program order.
  const int sq = STRIP ? lane >> 4 : 0, sc = STRIP ? lane & 15 : 0;
  auto lane_offset = [&](int b) -> unsigned { // byte offset of this lane's column (and half) in column block b
    const bool sp = SPLIT_OK && a.split && b == nblk - 1;
    const int kyb = b * 64 + (STRIP ? wave * 16 + sc : sp ? (lane & 31) : lane);
    return (unsigned) (kyb < H ? kyb : H - 1) * 16u + (sp ? halfoff : 0u);
  };
  // No conv request leaves the descriptor's sRows N Hp 8 bytes: a request's offset is that of the one-image case (below,
  // at `nextstart`: it ends inside the image) plus sqc images, sqc <= sRows - 1.
  const unsigned rowsel = STRIP ? (unsigned) min(sq, sRows - 1) * (unsigned) (M * sizeof(float2)) : 0u;
  // (the writers' address is formed from `lane`, the readers' from `sc`: two expressions, so that the compiler, which
  // knows nothing of the other lanes' stores, cannot forward a lane's own store into its read; the wave-scope fences say
  // the same and emit nothing)
  unsigned char *scr = STRIP ? reinterpret_cast<unsigned char *>(Tl) + sc * 16 : nullptr;
  unsigned char *scrw = STRIP ? reinterpret_cast<unsigned char *>(Tl) + lane * 16 : nullptr;
  const unsigned grow = STRIP ? (unsigned) sq * rowbytes : 0u; // the lane's row pair inside a group
  u32x4 rf[RD], rc[RD], fr[2], rg[2];
  if constexpr (STRIP)
  {
    const unsigned lo0 = lane_offset(0);
    const u32x4 g0 = __builtin_amdgcn_raw_buffer_load_b128(rsrcF, lo0 + grow, 0u, 0);
    rg[1] = __builtin_amdgcn_raw_buffer_load_b128(rsrcF, lo0 + grow, 4u * rowbytes, 0);
    rg[0] = __builtin_amdgcn_raw_buffer_load_b128(rsrcF, lo0 + grow, 8u * rowbytes, 0);
#pragma unroll
    for (int t = 0; t < RD; t++)
      rc[t] = __builtin_amdgcn_raw_buffer_load_b128(rsrcC, lo0 + rowsel, (unsigned) t * rowbytes, 0);
    *reinterpret_cast<u32x4 *>(scrw) = g0;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    fr[0] = *reinterpret_cast<const u32x4 *>(scr);
    fr[1] = *reinterpret_cast<const u32x4 *>(scr + 256);
  }
  else
  {
    const unsigned lo0 = lane_offset(0);
#pragma unroll
    for (int t = 0; t < RD; t++)
    {
      rf[t] = __builtin_amdgcn_raw_buffer_load_b128(rsrcF, lo0, (unsigned) t * rowbytes, 0);
      rc[t] = __builtin_amdgcn_raw_buffer_load_b128(rsrcC, lo0, (unsigned) t * rowbytes, 0);
    }
  }
  for (int blk = 0; blk < nblk; blk++)
  {
    const bool split = SPLIT_OK && a.split && blk == nblk - 1;
    const int n1 = split ? sHalf : N1;
    const int ttotal = R2 * n1;
    const int ky = blk * 64 + (STRIP ? wave * 16 + sc : split ? (lane & 31) : lane);
    const unsigned laneoff = lane_offset(blk);
    const unsigned laneoffC = STRIP ? laneoff + rowsel : laneoff; // (STRIP: the conv operand of this lane's row,
    const unsigned laneoffF = STRIP ? laneoff + grow : 0u;        //  the particle operand of its row pair of a group)
    const unsigned laneoff_next = lane_offset(min(blk + 1, nblk - 1));
    const bool has_next = blk + 1 < nblk;
    // LEAN (no split block): a block that has a successor has all 64 lanes live, and the successor's column of a lane
    // is this lane's 1 024 bytes on -- a wave-uniform distance, which goes into the SCALAR offset of a request, so the
    // lane offset is `laneoff` for every request of the block.  Requests issued from this block for the next one cover its
    // first RD row pairs only; a lane whose column there lies beyond H - 1 reads, unclamped, words of the FOLLOWING row
    // pair of the same image, which it never consumes (the lane sits out the next block, EXEC masked, as ever).  After
    // the last block the ring's tail requests are still issued (the wait counts include them): rows 0 .. RD - 1 of this
    // block again, addresses the wave has read before.
    // No request leaves the image's N Hp 8 bytes: the largest offset is row pair RD - 1, plus 1 024 bytes and lane 63,
    // i.e. 127 words and the 16 bytes read; a successor means H > 64, so 128 words are less than two row pairs and the
    // request ends inside row pair RD + 1 <= 6 of the >= 64 a shape with two blocks has.  Without a successor it ends
    // inside row pair RD - 1 <= 4, and N / 2 = N1 R / 2 >= 6 is part of lean_launch_ok (bioem_hip.hip).  Nothing relies
    // on the zeros a descriptor returns out of range.
    // Strip lanes: the columns of a block are the same 64, lane 63's now asked for by lane 15 of wave 3, so the bound
    // holds for the conv requests as it stands, inside the image sqc of the block's descriptor.  A particle request is a
    // group: row pairs 4 g .. 4 g + 3 (the lane's sq rowbytes on top of its column), requested up to two steps ahead.
    // Inside a block the last group asked for is the block's last.  Past it: with a successor, groups 0 .. 2 of the next
    // block, i.e. up to row pair 11 plus 1 024 bytes and the column, under two row pairs: inside row pair 13 of >= 64;
    // without one (and in the prologue), groups 0 .. 2 of this block again, row pairs 0 .. 11 of N / 2 = 8 N1 -- inside
    // the image from N1 = 2 on, and a 21-row window needs N >= 32.  These tail groups are never consumed; should one lie
    // beyond the image (N1 = 1, which no plan of this window has), the one-image descriptor makes no access for it.
    const unsigned nextstart = has_next ? 1024u : 0u;
    float Tr[NW], Ti[NW];
#pragma unroll
    for (int d = 0; d < NW; d++)
    {
      Tr[d] = 0.f;
      Ti[d] = 0.f;
    }
    // table slice of this column block: 24 bytes per thread, requested now and put into the LDS with the T block
    float2 tabv[3] = {};
    if (symw)
    {
#pragma unroll
      for (int u = 0; u < 3; u++)
        tabv[u] = symsrc[blk * kSymSliceFloat2 + u * 256];
    }
    // lanes beyond the last column of the last block sit out the whole transform (EXEC masked once): their
    // loads would only burn vector-memory cycles, and their T columns stay zero
    if (ky < H)
    for (int k1 = 0; k1 < n1; k1++)
    {
      float xr[R], xi[R];
      // the 2*WD+1 recombination twiddles of this k1 are contiguous: a few wide scalar loads, issued early
      float2 wk[NW];
      const float2 *twk = a.twk + (size_t) k1 * NW;
#pragma unroll
      for (int d = 0; d < NW; d++)
        wk[d] = twk[d];
      // LEAN: scalar offset of the step's last RD requests, chosen once per step -- the next step's rows, or from the
      // block's last step the first RD rows of what follows (nextstart)
      const unsigned tailbase = !LEAN ? 0u : k1 + 1 < n1 ? (unsigned) ((k1 + 1) * R2) * rowbytes : nextstart;
      // STRIP: base of the row pairs j steps ahead (a group of particle row pairs is requested up to two steps ahead)
      // (past the block's last step: what follows, `nextstart`, as one wave-uniform correction of the running offset --
      // a select between two loop invariants, where a select between two products became a branch inside the loop)
      const unsigned wrapadj = STRIP ? nextstart - (unsigned) ttotal * rowbytes : 0u;
      auto stepbase = [&](int j) -> unsigned {
        return (unsigned) ((k1 + j) * R2) * rowbytes + (k1 + j < n1 ? 0u : wrapadj);
      };
#pragma unroll
      for (int k2p = 0; k2p < R2; k2p++)
      {
        const float4 f = as_float4(STRIP ? fr[k2p % 2] : rf[k2p % RD]);
        const float4 c = as_float4(rc[k2p % RD]);
        // X = conv * conj(ref)   (bioem.cpp:1452-1455)
        xr[FFT_IN(2 * k2p)] = fmaf(c.x, f.x, c.y * f.y);
        xi[FFT_IN(2 * k2p)] = fmaf(c.y, f.x, -(c.x * f.y));
        xr[FFT_IN(2 * k2p + 1)] = fmaf(c.z, f.z, c.w * f.w);
        xi[FFT_IN(2 * k2p + 1)] = fmaf(c.w, f.z, -(c.z * f.w));
        if constexpr (LEAN)
        { // lane offset constant over the block, everything else in the scalar offset (tailbase above)
          const unsigned so = k2p + RD < R2 ? (unsigned) (k1 * R2 + k2p + RD) * rowbytes
                                            : tailbase + (unsigned) (k2p + RD - R2) * rowbytes;
          if constexpr (STRIP)
          {
            if (k2p % 4 == 0)
            { // group k2p / 4 + 1 of this step into its slot, group k2p / 4 + 3 requested: row pairs k2p + 12 .. + 15
              const int gs = (k2p / 4 + 1) % 2;
              const int rq = k2p + 12, sj = rq / R2;
              const unsigned sog = (sj == 1 ? tailbase : stepbase(sj)) + (unsigned) (rq % R2) * rowbytes;
              *reinterpret_cast<u32x4 *>(scrw + gs * 1024) = rg[gs];
              rg[gs] = __builtin_amdgcn_raw_buffer_load_b128(rsrcF, laneoffF, sog, 0);
              __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            }
            // row pair k2p + 2 back into the registers `f` has just left
            fr[k2p % 2] = *reinterpret_cast<const u32x4 *>(scr + (((k2p + 2) / 4) % 2) * 1024 + ((k2p + 2) % 4) * 256);
          }
          else
            rf[k2p % RD] = __builtin_amdgcn_raw_buffer_load_b128(rsrcF, laneoff, so, 0);
          rc[k2p % RD] = __builtin_amdgcn_raw_buffer_load_b128(rsrcC, laneoffC, so, 0);
        }
        else
        {
          int tn = k1 * R2 + k2p + RD;
          unsigned vo = laneoff;
          // (only the last RD requests of a k1 step can leave the block: the first test folds at compile time)
          if (k2p + RD >= R2 && tn >= ttotal)
          { // last steps of this block: run on into the next block (or re-read the last row at the very end)
            tn = has_next ? tn - ttotal : ttotal - 1;
            vo = has_next ? laneoff_next : laneoff;
          }
          rf[k2p % RD] = __builtin_amdgcn_raw_buffer_load_b128(rsrcF, vo, (unsigned) tn * rowbytes, 0);
          rc[k2p % RD] = __builtin_amdgcn_raw_buffer_load_b128(rsrcC, vo, (unsigned) tn * rowbytes, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      FFT_RUN(xr, xi);
      // recombination of the N1 sub-transforms for the displacement window only:
      //   T[dx] += w_N^(dx*k1) * y_k1[dx mod 32]
#pragma unroll
      for (int d = -WD; d <= WD; d++)
      {
        const int pos = FFT_OUT((((d * GS) % R) + R) % R);
        const float2 w = wk[d + WD];
        float tr = Tr[d + WD], ti = Ti[d + WD];
        tr = fmaf(xr[pos], w.x, tr);
        tr = fmaf(-xi[pos], w.y, tr);
        ti = fmaf(xr[pos], w.y, ti);
        ti = fmaf(xi[pos], w.x, ti);
        Tr[d + WD] = tr;
        Ti[d + WD] = ti;
      }
    }
    // STRIP: slot 0 holds the first group of what follows, and the T exchange below overwrites it: its row pairs 2 and 3,
    // not read back yet, cross the exchange in registers and are put back after this wave's window pass (every lane of a
    // column writes the same 16 bytes; no other wave touches Tl after the second barrier)
    u32x4 carry[2];
    if constexpr (STRIP)
    {
      carry[0] = *reinterpret_cast<const u32x4 *>(scr + 512);
      carry[1] = *reinterpret_cast<const u32x4 *>(scr + 768);
    }
    if constexpr (SPLIT_OK)
    if (split)
    {
      const float2 *ws = a.twk + (size_t) sHalf * NW; // w^(dx sHalf), the table's row sHalf
#pragma unroll
      for (int d = 0; d < NW; d++)
      {
        const float2 w = ws[d];
        const float wx = hsel ? w.x : 1.f, wy = hsel ? w.y : 0.f;
        const float tr = fmaf(-Ti[d], wy, Tr[d] * wx), ti = fmaf(Ti[d], wx, Tr[d] * wy);
        const u32x2 sr = __builtin_amdgcn_permlane32_swap(__float_as_uint(tr), __float_as_uint(tr), false, false);
        const u32x2 si = __builtin_amdgcn_permlane32_swap(__float_as_uint(ti), __float_as_uint(ti), false, false);
        Tr[d] = __uint_as_float(sr.x) + __uint_as_float(sr.y); // low half + high half, in every lane
        Ti[d] = __uint_as_float(si.x) + __uint_as_float(si.y);
      }
    }
    // FFTW c2r convention: columns 0 and N/2 enter once (real part only after the ky pass), others twice
    float wgt = 2.f;
    if (ky == 0 || (((N & 1) == 0) && ky == N / 2))
      wgt = 1.f;
    if (ky >= H || (split && hsel))
      wgt = 0.f;
    // T block of THIS wave only, written and read between block barriers (they keep the 4 waves in lock-step)
    {
      __syncthreads(); // previous window reads are done
      if constexpr (STRIP)
      { // strip lanes: this lane holds T of row sq at column 16 wave + sc of the block -- into row sq's T region, which
        // wave sq reads below (a row beyond the block's last is the clamped copy, as a clamped wave's was)
        float2 *Tq = Tall + (size_t) sq * NW * TS + wave * 16 + sc;
#pragma unroll
        for (int d = 0; d < NW; d++)
          Tq[d * TS] = make_float2(Tr[d] * wgt, Ti[d] * wgt);
      }
      else
      {
#pragma unroll
        for (int d = 0; d < NW; d++)
          Tl[d * TS + lane] = make_float2(Tr[d] * wgt, Ti[d] * wgt);
      }
      if (symw)
      {
#pragma unroll
        for (int u = 0; u < 3; u++)
          twl[u * 256 + threadIdx.x] = tabv[u];
      }
      __syncthreads();
      const int idx0 = LEAN ? 0 : (int) (((long long) (blk * 64) * step) % N);
      const int npairs = min(32, (H - blk * 64 + 1) >> 1); // columns of this block that exist, in pairs
      if constexpr (LEAN)
        window_accumulate_sym<TS>(Trow, stab, acc, npairs);
      else if (symw)
      {
        if constexpr (SYM)
          window_accumulate_sym<TS>(Trow, stab, acc, npairs);
      }
      else if (!SYM && is_static)
      {
        const int rowoff[NR] = {rowbase};
        window_accumulate<NR, true, 32, TS>(Tl, twl, N, step, idx0, rowoff, nr, acc, npairs);
      }
      else
      {
        int rowoff[NR];
#pragma unroll
        for (int r = 0; r < NR; r++)
          rowoff[r] = row_of(r);
        window_accumulate<NR, false, 32, TS>(Tl, twl, N, step, idx0, rowoff, nr, acc, npairs);
      }
      if constexpr (STRIP)
      {
        *reinterpret_cast<u32x4 *>(scr + 512) = carry[0];
        *reinterpret_cast<u32x4 *>(scr + 768) = carry[1];
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      }
    }
  }
  if (NYQ)
  {
    // OWN: one set of Nyquist rows per row of the launch
    const float *tq = a.tnyq + (OWN ? (size_t) oc : (size_t) p * a.ldPart + oc) * NW;
    const float sg = (dy & 1) ? -1.f : 1.f;
    if (symw)
    { // the column's term is real: it enters A only, with the sign of (-1)^|dy|
      if constexpr (SYM)
      {
#pragma unroll
        for (int j = 0; j < 4; j++)
          acc[j] = fmaf((((sgrp * 4 + j) * GS) & 1) ? -1.f : 1.f, tq[srow], acc[j]);
      }
    }
    else if constexpr (!LEAN)
    {
#pragma unroll
      for (int r = 0; r < NR; r++)
        acc[r] = fmaf(sg, tq[is_static ? rowbase / TS + r : row_of(r) / TS], acc[r]);
    }
  }

  const double2 pc = a.postc[oc];
  const PostW pw = post_consts(a.pd.Ntotpi, N, a.params[oc], a.sumRef[p], a.sumsqRef[p], pc.x, pc.y);
  LseF L;
  L.m = -INFINITY;
  L.s = 0.;
  L.id = 0x7fffffff;
  L.val = 0.f;
  {
    // the NR displacements of this lane as one batch (posterior_batch: exact division by N^2 in three instructions,
    // the log-table reads issued together, one log-sum-exp rescale)
    constexpr int PB = NA > 8 ? 8 : NA;
#pragma unroll
    for (int r0 = 0; r0 < NA; r0 += PB)
    {
      float accv[PB];
      int idv[PB];
      bool okv[PB];
      if (symw)
      { // slot 2 q: dy = +(4 g + q) rows, A - B; slot 2 q + 1: dy = -(4 g + q) rows, A + B (dy = 0 once; 4 g + q <= WD)
        if constexpr (SYM)
        {
          const int ixv = dinv[srow];
#pragma unroll
          for (int j = 0; j < 8; j++)
          {
            const int q = j >> 1, m = sgrp * 4 + q;
            const int iyv = dinv[min(max((j & 1) ? mD - m : mD + m, 0), 31)];
            okv[j] = lane < 3 * NW && m <= WD && !((j & 1) && m == 0) && srow < a.ndx && iyv < a.ndy;
            accv[j] = (j & 1) ? acc[q] + acc[4 + q] : acc[q] - acc[4 + q];
            idv[j] = ixv * nd + iyv;
          }
        }
      }
      else if constexpr (!LEAN)
      {
#pragma unroll
        for (int j = 0; j < PB; j++)
        {
          const int r = r0 + j < NR ? r0 + j : NR - 1;
          const int ixs = grp * nr + r; // position in the lane-group order; ix = visiting rank of that displacement
          okv[j] = r0 + j < NR && r < nr && wactive && ixs < a.ndx && iy < a.ndy;
          const int ix = is_static ? dinv[min(ixs, 31)] : ixs;
          accv[j] = acc[r];
          idv[j] = ix * nd + iy;
        }
      }
      posterior_batch<PB>(L, accv, idv, okv, pw, ltab, a.algo);
    }
  }
  lsef_wave_reduce(L);
  if (lane == 0 && oc_valid)
  {
    Partial r;
    r.sumExp = L.s;
    r.best = L.m;
    r.id = L.id;
    r.value = L.val;
    r.pad = 0;
    a.partials[OWN ? (size_t) oc : (size_t) p * a.ldPart + oc] = r; // OWN: one partial per row of the launch
  }
}

// the LEAN instantiation for a registry row (a[4] = 1 behind the K_FAST row of the same arguments), or a null stub where
// the kernel has no window pass over |dy|: find_kernel skips null stubs, such a shape launches the full instantiation
template <int WD, int R, bool NYQ, int GS, class ARGS = CompareArgs>
const void *fast_lean_kernel()
{
  if constexpr (sym_window_ok(WD, R, NYQ, GS))
    return reinterpret_cast<const void *>(k_compare_fast<WD, R, NYQ, GS, ARGS, true>);
  else
    return nullptr;
}

// ------------------------------------------------------------------------------------------------
// Nyquist-column rows for the fast kernel's NYQ mode: thread = one (particle, orientation*CTF) pair, tile of
// 16 x 16 pairs per block (each operand line is shared by 16 threads).
//   tnyq[p][oc][m + WD] = Re sum_kx conv[oc][kx][N/2] * conj(ref[p][kx][N/2]) * w_N^(kx m gs),  m = -WD..WD
// The twiddles are uniform over the block and tabulated per row pair (twnyq): wide scalar loads.
// ------------------------------------------------------------------------------------------------
// Q = 4 (few particles: 16 x 16 pairs per block are 192 blocks for 10 particles x 3 072 spectra, every thread a chain of
// N/2 row pairs): the four waves of a block share its 4 x 16 pairs, wave w the w-th quarter of the row pairs in order
// (the twiddles stay wave-uniform), the quarters added through LDS as (q0 + q1) + (q2 + q3).
// ARGS = OwnNyquistArgs (OWN; the API's label "k_nyquist_rows_own<WD>"): the rows of ONE launch of the own-list pass, row
// oc of the launch against ITS particle -- the four waves of a block share its 64 rows, one thread per row and quarter,
//   tnyq[oc][m + WD] = the sum above with p = slotParticle[(row0 + oc) / nCTF].
// The arithmetic is that of Q = 4 -- the kernel a per-particle launch runs --, so the rows equal that launch's bit for bit.
template <int WD, int Q, class ARGS = CompareArgs>
__global__ __launch_bounds__(256) void k_nyquist_rows(const ARGS a)
{
  constexpr bool OWN = !std::is_same<ARGS, CompareArgs>::value;
  static_assert(Q == 1 || Q == 4, "one thread per pair, or one per pair and wave");
  static_assert(!OWN || Q == 4, "bit identity with a per-particle launch rests on its (q0 + q1) + (q2 + q3) association");
  constexpr int NW = 2 * WD + 1;
  __shared__ float part[Q == 4 ? 2 * 64 * NW : 1];
  const int N = a.N, H = a.H, N1 = a.N1;
  const int R2 = N / (2 * N1);
  const int q = Q == 1 ? 0 : __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6));
  const int t = Q == 1 ? threadIdx.x : threadIdx.x & 63;
  int p, oc;
  bool valid;
  if constexpr (OWN)
  { // OWN: thread -> row oc of the launch and the particle of that row's slot (compare_args.hpp)
    oc = blockIdx.x * 64 + t;
    valid = oc < a.nOC;
    p = valid ? a.slotParticle[(a.row0 + oc) / a.nCTF] : 0;
  }
  else
  {
    const int tilesOC = (a.nOC + 15) / 16;
    const int tp = blockIdx.x / tilesOC, to = blockIdx.x - tp * tilesOC;
    p = tp * (16 / Q) + (t >> 4);
    oc = to * 16 + (t & 15);
    valid = p < a.nMaps && oc < a.nOC;
  }
  const size_t M = (size_t) N * a.Hp; // an image of the comparison layout (Hp >= H: its row-pair pitch)
  const float2 *F = a.ref + (size_t) (valid ? p : 0) * M;
  const float2 *C = a.conv + (size_t) (valid ? oc : 0) * M;
  float acc[NW];
#pragma unroll
  for (int d = 0; d < NW; d++)
    acc[d] = 0.f;
  const int nRP = N1 * R2 / Q; // row pairs of this thread: [q nRP, (q + 1) nRP)
  // row pair = (k1, k2 pair): kx0 = N1*(2 k2p) + k1, kx1 = kx0 + N1.  Eight pairs' operands are fetched at once: every
  // load of a thread is a cache line of its own (one particle, one conv spectrum), and with one pair in flight the
  // kernel was a chain of N/2 memory latencies (58 us for 30 720 comparisons at 128^2); the sums keep their order.
  constexpr int NB = WD > 31 ? 4 : 8; // N/2 is a multiple of 64, a quarter of it of 16
  for (int rp0 = q * nRP; rp0 < (q + 1) * nRP; rp0 += NB)
  {
    float4 cb[NB], fb[NB];
#pragma unroll
    for (int u = 0; u < NB; u++)
    {
      // the two k2 of a pair are adjacent in the comparison layout: one 16-byte load per operand
      const size_t li = ((size_t) (rp0 + u) * a.Hp + N / 2) * 2;
      cb[u] = *reinterpret_cast<const float4 *>(C + li);
      fb[u] = *reinterpret_cast<const float4 *>(F + li);
    }
#pragma unroll
    for (int u = 0; u < NB; u++)
    {
      const float4 c = cb[u], f = fb[u];
      // X = conv * conj(ref)   (bioem.cpp:1452-1455)
      const float x0r = fmaf(c.x, f.x, c.y * f.y), x0i = fmaf(c.y, f.x, -(c.x * f.y));
      const float x1r = fmaf(c.z, f.z, c.w * f.w), x1i = fmaf(c.w, f.z, -(c.z * f.w));
      // twiddles of this row pair: block-uniform, contiguous -> a few wide scalar loads
      const float4 *tw = reinterpret_cast<const float4 *>(a.twnyq + (size_t) (rp0 + u) * NW * 2);
#pragma unroll
      for (int d = 0; d < NW; d++)
      {
        const float4 w = tw[d]; // (w0.re, w0.im, w1.re, w1.im)
        float v = acc[d];
        v = fmaf(x0r, w.x, v);
        v = fmaf(-x0i, w.y, v);
        v = fmaf(x1r, w.z, v);
        v = fmaf(-x1i, w.w, v);
        acc[d] = v;
      }
    }
  }
  if (Q == 4)
  {
    // (q0 + q1) in wave 0, (q2 + q3) in wave 2, then their sum in wave 0
    float *mine = part + ((q >> 1) * 64 + t) * NW;
    if (q & 1)
    {
#pragma unroll
      for (int d = 0; d < NW; d++)
        mine[d] = acc[d];
    }
    __syncthreads();
    if (!(q & 1))
    {
#pragma unroll
      for (int d = 0; d < NW; d++)
        acc[d] += mine[d];
    }
    __syncthreads();
    if (q == 2)
    {
#pragma unroll
      for (int d = 0; d < NW; d++)
        mine[d] = acc[d];
    }
    __syncthreads();
    if (q == 0)
    {
#pragma unroll
      for (int d = 0; d < NW; d++)
        acc[d] += part[(64 + t) * NW + d];
    }
  }
  if (valid && q == 0)
  {
    // OWN: one set of rows per row of the launch
    float *o = a.tnyq + (OWN ? (size_t) oc : (size_t) p * a.ldPart + oc) * NW;
#pragma unroll
    for (int d = 0; d < NW; d++)
      o[d] = acc[d];
  }
}

} // namespace

#endif
