// scan_kernels.hpp -- the log posterior of one (particle, orientation, shift) record under every CTF set of a list handed
// in (bioem_hip_ctf_scan, bioem_hip_debug_ctf_scan): one projection spectrum against many kernels.  Per
// record r and candidate g, with the symbols of window_kernels.hpp:
//   conv = P_r conj(K_g) in float (the expression of k_convolve), sumC its real part at the origin,
//   sumsquareC = the reference's sequential float chain over its Parseval terms, divided as k_parseval_ordered divides,
//   S = sum_k w_ky Re(conv[k] conj(F_r[k]) exp(+2 pi i ((kx dx + ky dy) mod N) / N)), dx = -X_r, dy = -Y_r, in double,
//   cc = (float) S / (float) (N N),  logp = logpro_eval(cc) with logpro_consts of {amp_g, pha_g, env_g, sumC, sumsquareC}.
// Everything of a record that does not depend on the candidate is prepared once, in the WALK ORDER: the order of the
// reference's Parseval sum (rows; inside a row the interior columns, then column 0, then column N / 2 for even N).  The
// scan then is one pass over that order with lane = candidate: the kernels' coefficient is one coalesced 512-byte line,
// the record's coefficients are wave-uniform.  No atomics, no cross-lane operation: a (record, candidate) result depends
// on its own inputs alone and carries the same bits in any chunking, batch or order.
// The declarations are for every translation unit; the kernels are compiled by kernels_scan.hip only (BIOEM_SCAN_TU).
#ifndef BIOEM_SCAN_KERNELS_HPP
#define BIOEM_SCAN_KERNELS_HPP

#include "engine_types.hpp"
#include "window_kernels.hpp"

const int kScanLanes = 64; // candidates of a chunk: the lanes of a wave
// records a wave of k_ctf_scan carries; results do not depend on it.  Measured at 1, 2, 4 (DESIGN 2.17,
// profiles/ctf_scan_measure.txt): 1 is the fastest -- a wave is a chain of memory latencies, more waves hide them better
// than a kernel load shared by several records saves.  A build with -DBIOEM_SCAN_RECORDS=R, loaded through
// BIOEM_HIP_LIBRARY, is the other side of scripts/ctf_scan_measure.py
#ifndef BIOEM_SCAN_RECORDS
#define BIOEM_SCAN_RECORDS 1
#endif
const int kScanRecords = BIOEM_SCAN_RECORDS;

// one record of a batch: its shift as reported (|X|, |Y| < N)
struct BioemScanShift
{
  int X, Y;
};

// packed[chunk0 + c][position][lane] from kernels[nG][N][H] (reference layout), nG <= kScanLanes candidates of chunk c =
// chunk0; lanes beyond nG repeat the last candidate
BIOEM_HIDDEN hipError_t bioem_scan_pack_launch(hipStream_t st, const float2 *kernels, int nG, int N, float2 *packedChunk);
// Pw[n][M] (the projections in walk order) and Z[n][M] = w conj(F) tw[(kx dx + ky dy) mod N] (double pairs, walk order)
// from proj / ref [n][N][H] (reference layout) and the records' shifts; tw = exp(+2 pi i k / N), N double pairs
BIOEM_HIDDEN hipError_t bioem_scan_prep_launch(hipStream_t st, const float2 *proj, const float2 *ref,
                                               const BioemScanShift *shift, int n, int N, const double2 *tw, float2 *Pw,
                                               double2 *Z);
// logp[n][G], cc[n][G], params[n][G] of n prepared records against G packed candidates with ctfParam[G][3]; the
// particles' sums indexed by the records' particle
BIOEM_HIDDEN hipError_t bioem_scan_launch(hipStream_t st, const float2 *packed, const float *ctfParam, int G,
                                          const float2 *Pw, const double2 *Z, const BioemWindowRecord *rec,
                                          const float *sumRef, const float *sumsqRef, const bioem_hip_param_device &pd,
                                          int n, int N, double *logp, float *cc, bioem_hip_param5 *params);

#ifdef BIOEM_SCAN_TU
#include "posterior.hpp"

namespace
{

// wave-uniform reads through the constant address space: scalar loads (arrays no kernel of the launch writes)
typedef const float __attribute__((address_space(4))) *scan_float_ptr;
typedef const double __attribute__((address_space(4))) *scan_double_ptr; // a double2 array as pairs of doubles
// four positions of a record at once (the arrays are aligned as their float2 / double2 elements are)
typedef float scan_float8 __attribute__((ext_vector_type(8), aligned(8)));
typedef double scan_double8 __attribute__((ext_vector_type(8), aligned(16)));
typedef const scan_float8 __attribute__((address_space(4))) *scan_float8_ptr;
typedef const scan_double8 __attribute__((address_space(4))) *scan_double8_ptr;

__device__ __forceinline__ int scan_step(int X, int N)
{ // the displacement -X reduced to [0, N)
  const int d = (-X) % N;
  return d < 0 ? d + N : d;
}

// position q of a row of the walk order -> column: the interior columns 1 .. jend - 1 first, then 0, then N / 2 (even N)
__device__ __forceinline__ int scan_column(int q, int jend, int H) { return q < jend - 1 ? q + 1 : (q == jend - 1 ? 0 : H - 1); }

// grid (tiles of 64 positions), 256 threads: a 64 x 64 tile through LDS, read along the positions, written along the lanes
__global__ __launch_bounds__(256) void k_scan_pack(const float2 *__restrict__ kernels, int nG, int N, int H,
                                                   float2 *__restrict__ packed)
{
  __shared__ float2 tile[kScanLanes][65];
  const int M = N * H, pos0 = blockIdx.x * 64;
  const int jend = (N & 1) ? H : H - 1;
  const int a = threadIdx.x & 63, b = threadIdx.x >> 6;
  const int pos = min(pos0 + a, M - 1);
  const int i = pos / H, j = scan_column(pos - i * H, jend, H);
  for (int g = b; g < kScanLanes; g += 4)
    tile[g][a] = kernels[(size_t) min(g, nG - 1) * M + (size_t) i * H + j];
  __syncthreads();
  for (int p = b; p < 64; p += 4)
    if (pos0 + p < M)
      packed[(size_t) (pos0 + p) * kScanLanes + a] = tile[a][p];
}

// grid (blocks per record, records)
__global__ __launch_bounds__(256) void k_scan_prep(const float2 *__restrict__ proj, const float2 *__restrict__ ref,
                                                   const BioemScanShift *__restrict__ shift, int N, int H,
                                                   const double2 *__restrict__ tw, float2 *__restrict__ Pw,
                                                   double2 *__restrict__ Z)
{
  const int r = blockIdx.y;
  const int M = N * H;
  const int jend = (N & 1) ? H : H - 1;
  const int dx = scan_step(shift[r].X, N), dy = scan_step(shift[r].Y, N);
  const float2 *P = proj + (size_t) r * M, *F = ref + (size_t) r * M;
  for (int pos = blockIdx.x * blockDim.x + threadIdx.x; pos < M; pos += gridDim.x * blockDim.x)
  {
    const int i = pos / H, j = scan_column(pos - i * H, jend, H);
    const int e = i * H + j;
    const float2 f = F[e];
    const double2 t = tw[(int) (((long long) i * dx + (long long) j * dy) % N)];
    const double w = (j == 0 || 2 * j == N) ? 1. : 2.;
    const double fr = (double) f.x, fi = (double) f.y;
    Pw[(size_t) r * M + pos] = P[e];
    Z[(size_t) r * M + pos] = make_double2(w * fma(fr, t.x, fi * t.y), w * fma(fr, t.y, -(fi * t.x))); // w conj(F) tw
  }
}

// grid (chunks of 64 candidates, groups of R records), one wave per block, lane = candidate.  Per position of the walk
// order: one vector load of the 64 kernels' coefficient; per record of the group P and Z by scalar loads, the float
// product, its term added to the lane's own strict chain, and the double sum.  The R chains of a lane are independent and
// every kernel load serves R records (R = kScanRecords).  A group shorter than R repeats its last record and stores
// nothing for the copies; lanes beyond G repeat the last candidate (k_scan_pack) and store nothing.
template <int R>
__global__ __launch_bounds__(64) void k_ctf_scan(const float2 *__restrict__ packed, const float *__restrict__ ctfParam,
                                                 int G, const float2 *__restrict__ Pw, const double2 *__restrict__ Z,
                                                 const BioemWindowRecord *__restrict__ rec,
                                                 const float *__restrict__ sumRef, const float *__restrict__ sumsqRef,
                                                 const PD pd, int n, int N, int H, double *__restrict__ logp,
                                                 float *__restrict__ cc, bioem_hip_param5 *__restrict__ params)
{
  const int lane = threadIdx.x, chunk = blockIdx.x, r0 = blockIdx.y * R;
  const int M = N * H;
  const int jend = (N & 1) ? H : H - 1;
  const float2 *K = packed + (size_t) chunk * M * kScanLanes + lane;
  scan_float_ptr p[R];
  scan_double_ptr z[R];
  float ss[R];
  double S[R];
#pragma unroll
  for (int q = 0; q < R; q++)
  {
    const size_t r = (size_t) min(r0 + q, n - 1);
    p[q] = (scan_float_ptr) (unsigned long long) (Pw + r * M);
    z[q] = (scan_double_ptr) (unsigned long long) (Z + r * M);
    ss[q] = 0.f;
    S[q] = 0.;
  }
  auto step = [&](int pos, bool doubled) {
    const float2 k = K[(size_t) pos * kScanLanes];
#pragma unroll
    for (int q = 0; q < R; q++)
    {
      const float px = p[q][2 * pos], py = p[q][2 * pos + 1];
      const double zx = z[q][2 * pos], zy = z[q][2 * pos + 1];
      float2 o;
      o.x = (px * k.x + py * k.y);
      o.y = (py * k.x - px * k.y);
      const float t = o.x * o.x + o.y * o.y;
      ss[q] += doubled ? t * 2 : t;
      S[q] = fma((double) o.x, zx, S[q]);
      S[q] = fma(-(double) o.y, zy, S[q]);
    }
  };
  // four consecutive interior positions: per record ONE scalar load of the four P and one of the four Z (a wave's scalar
  // loads return one after the other: eight narrow ones per record and block were what the kernel waited for), the
  // kernels' four lines in flight together; inside the block position after position, so the chains keep their order
  auto block4 = [&](int pos) {
    float2 k[4];
#pragma unroll
    for (int u = 0; u < 4; u++)
      k[u] = K[(size_t) (pos + u) * kScanLanes];
#pragma unroll
    for (int q = 0; q < R; q++)
    {
      const scan_float8 pp = *(const scan_float8_ptr) (p[q] + 2 * pos);
      const scan_double8 zz = *(const scan_double8_ptr) (z[q] + 2 * pos);
#pragma unroll
      for (int u = 0; u < 4; u++)
      {
        float2 o;
        o.x = (pp[2 * u] * k[u].x + pp[2 * u + 1] * k[u].y);
        o.y = (pp[2 * u + 1] * k[u].x - pp[2 * u] * k[u].y);
        const float t = o.x * o.x + o.y * o.y;
        ss[q] += t * 2;
        S[q] = fma((double) o.x, zz[2 * u], S[q]);
        S[q] = fma(-(double) o.y, zz[2 * u + 1], S[q]);
      }
    }
  };
  for (int i = 0; i < N; i++)
  {
    const int base = i * H;
    int q = 0;
#pragma unroll 2 // the next block's loads in flight
    for (; q + 4 <= jend - 1; q += 4)
      block4(base + q);
    for (; q < jend - 1; q++)
      step(base + q, true);
    step(base + jend - 1, false); // column 0
    if (!(N & 1))
      step(base + jend, false); // column N / 2
  }
  const int g = chunk * kScanLanes + lane;
  if (g >= G)
    return;
  const float2 k0 = K[(size_t) (jend - 1) * kScanLanes]; // the origin: row 0, column 0
  const float nn = (float) (N * N);
#pragma unroll
  for (int q = 0; q < R; q++)
  {
    const int r = r0 + q;
    if (r >= n)
      break;
    bioem_hip_param5 c;
    c.amp = ctfParam[3 * g + 0];
    c.pha = ctfParam[3 * g + 1];
    c.env = ctfParam[3 * g + 2];
    c.sumC = (p[q][2 * (jend - 1)] * k0.x + p[q][2 * (jend - 1) + 1] * k0.y);
    c.sumsquareC = ss[q] / nn;
    double t2, prior;
    logpro_consts(pd, c, t2, prior);
    const int pt = rec[r].particle;
    const float value = (float) S[q] / nn;
    const size_t o = (size_t) r * G + g;
    logp[o] = logpro_eval(pd, c, value, sumRef[pt], sumsqRef[pt], t2, prior);
    if (cc)
      cc[o] = value;
    if (params)
      params[o] = c;
  }
}

} // namespace
#endif // BIOEM_SCAN_TU

#endif
