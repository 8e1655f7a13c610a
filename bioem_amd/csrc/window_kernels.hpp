// window_kernels.hpp -- the log posterior of every cell of the displacement window for (particle, orientation, CTF)
// requests (bioem_hip_window_posterior, bioem_hip_debug_window).  Per record r of a batch:
//   conv = P conj(CTF) in float (the expression of k_convolve), its Parseval terms laid out for k_parseval_ordered,
//   T[i][ky] = w_ky sum_kx conv[kx][ky] conj(F[kx][ky]) exp(+2 pi i ((kx dx_i) mod N) / N), the product in double,
//   S[i][j] = sum_ky Re(exp(+2 pi i ((ky dy_j) mod N) / N) T[i][ky]),  cc = (float) S / (float) (N N),
//   logp[i][j] = logpro_eval(cc), a double; dx_i = -X_i, dy_j = -X_j, X the reported shifts in ascending order,
//   w = 1 in the columns ky = 0 and (N even) N / 2, else 2.
// The comparison kernels fold this table away inside the kernel; nothing of a run goes through here.  The declarations
// are for every translation unit; the kernels are compiled by kernels_window.hip only (BIOEM_WINDOW_TU).
#ifndef BIOEM_WINDOW_KERNELS_HPP
#define BIOEM_WINDOW_KERNELS_HPP

#include "engine_types.hpp"

// one record of a batch: the first two fields lie as in RenderRecord (k_render_gather reads src); particle indexes the
// sums of the particles the cell pass reads
struct BioemWindowRecord
{
  int src, conv, particle, pad;
  float unused[2];
};

const int kWindowRows = 8; // window rows a wave of the column pass accumulates

// doubles pairs of scratch (T) for a batch of nImg records
BIOEM_HIDDEN size_t bioem_window_scratch(int N, int nd, int nImg);
// conv[n][N][H] (reference layout), terms[n][M4] and params[n] {amp, pha, env, sumC, 0} from the projections proj[n][N][H],
// the CTF kernels and the records' CTF indices
BIOEM_HIDDEN hipError_t bioem_window_prep_launch(hipStream_t st, const float2 *proj, const float2 *ctf, const float *ctfParam,
                                                 const BioemWindowRecord *rec, int n, int N, float2 *conv, float *terms,
                                                 int M4, bioem_hip_param5 *params);
// logp[n][nd][nd] and cc[n][nd][nd] from conv / ref [n][N][H] (reference layout), params[n] (sumsquareC filled in),
// postc[n] = {t2, prior}, the sums of the particles (indexed by the records' particle) and shifts[nd] (device, ascending);
// tw = exp(+2 pi i k / N), N double pairs; T = bioem_window_scratch pairs.  How a record is split over blocks depends
// on (N, nd) alone and every sum runs in a fixed order: the same bits for a record wherever it sits.
BIOEM_HIDDEN hipError_t bioem_window_launch(hipStream_t st, const float2 *conv, const float2 *ref,
                                            const BioemWindowRecord *rec, const bioem_hip_param5 *params,
                                            const double2 *postc, const float *sumRef, const float *sumsqRef,
                                            const bioem_hip_param_device &pd, int n, int N, int nd, const int *shifts,
                                            const double2 *tw, double2 *T, double *logp, float *cc);

#ifdef BIOEM_WINDOW_TU
#include "posterior.hpp"

namespace
{

// wave-uniform table reads through the constant address space: scalar loads (tables no kernel of the launch writes)
typedef const double __attribute__((address_space(4))) *const_double_ptr; // a double2 table as pairs of doubles
typedef const int __attribute__((address_space(4))) *const_int_ptr;

__device__ __forceinline__ int window_step(int X, int N)
{ // the displacement -X reduced to [0, N)
  const int d = (-X) % N;
  return d < 0 ? d + N : d;
}

// grid (blocks per record, records).  The element body is k_convolve's for the reference layout (prep_kernels.hpp): the
// same expression, unfused, so conv and sumC carry its bits; the term of element (i, j) goes to its place in the
// reference's summation order (inside a row the interior columns doubled, then column 0, then column N / 2 for even N).
__global__ __launch_bounds__(256) void k_window_prep(const float2 *__restrict__ proj, const float2 *__restrict__ ctf,
                                                     const float *__restrict__ ctfParam,
                                                     const BioemWindowRecord *__restrict__ rec, int N, int H,
                                                     float2 *__restrict__ conv, float *__restrict__ terms, int M4,
                                                     bioem_hip_param5 *__restrict__ params)
{
  const int r = blockIdx.y, c = rec[r].conv;
  const int M = N * H;
  const float2 *P = proj + (size_t) r * M;
  const float2 *K = ctf + (size_t) c * M;
  float2 *O = conv + (size_t) r * M;
  float *S = terms + (size_t) r * M4;
  const int jend = (N & 1) ? H : H - 1;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < M; e += gridDim.x * blockDim.x)
  {
    const int i = e / H, j = e - i * H;
    const float2 p = P[e], k = K[e];
    float2 o;
    o.x = (p.x * k.x + p.y * k.y);
    o.y = (p.y * k.x - p.x * k.y);
    const float t = o.x * o.x + o.y * o.y;
    int pos;
    if (j >= 1 && j < jend)
      pos = i * H + (j - 1);
    else if (j == 0)
      pos = i * H + (jend - 1);
    else
      pos = i * H + jend; // j == H - 1, even N
    S[pos] = (j >= 1 && j < jend) ? t * 2 : t;
    O[e] = o;
    if (e == 0)
    {
      bioem_hip_param5 q;
      q.amp = ctfParam[3 * c + 0];
      q.pha = ctfParam[3 * c + 1];
      q.env = ctfParam[3 * c + 2];
      q.sumC = o.x;
      q.sumsquareC = 0.f; // k_parseval_ordered
      params[r] = q;
    }
  }
}

// Column pass.  grid (column blocks of 64, row chunks of kWindowRows, records), kWindowSplit waves per block: lane = column
// ky, wave w walks the kx of its quarter [w Q, (w + 1) Q), Q = ceil(N / kWindowSplit), with one coalesced 8-byte load of
// conv and of F per step, forms X = conv conj(F) in double once and adds it into the kWindowRows rows of the chunk, each
// with its wave-uniform twiddle: the index (kx dx) mod N is stepped in scalar registers, the value comes by a scalar load.
// (One wave walking all of kx is a chain of N memory latencies with nothing to hide them behind: a batch is a few hundred
// waves.)  Wave 0 adds the quarters in wave order: the split is a function of N alone, the order fixed.  Rows beyond nd
// repeat the last row and are not stored.
const int kWindowSplit = 4;
__global__ __launch_bounds__(64 * kWindowSplit) void k_window_cols(const float2 *__restrict__ conv,
                                                                   const float2 *__restrict__ ref, int N, int H, int nd,
                                                                   const int *__restrict__ shifts,
                                                                   const double2 *__restrict__ tw, double2 *__restrict__ T)
{
  __shared__ double2 part[kWindowSplit - 1][kWindowRows][64];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int ky = blockIdx.x * 64 + lane, row0 = blockIdx.y * kWindowRows, r = blockIdx.z;
  const size_t M = (size_t) N * H;
  const bool live = ky < H;
  const float2 *C = conv + r * M + (live ? ky : H - 1); // lanes beyond the row read its last column and store nothing
  const float2 *F = ref + r * M + (live ? ky : H - 1);
  const const_int_ptr sh = (const_int_ptr) (unsigned long long) shifts;
  const const_double_ptr w = (const_double_ptr) (unsigned long long) tw;
  const int Q = (N + kWindowSplit - 1) / kWindowSplit;
  const int kx0 = wave * Q, kx1 = min(N, kx0 + Q);
  int step[kWindowRows], t[kWindowRows];
  double ar[kWindowRows], ai[kWindowRows];
#pragma unroll
  for (int j = 0; j < kWindowRows; j++)
  {
    step[j] = window_step(sh[min(row0 + j, nd - 1)], N);
    t[j] = (int) (((long long) kx0 * step[j]) % N);
    ar[j] = ai[j] = 0.;
  }
#pragma unroll 4 // four steps' loads and twiddles in flight
  for (int kx = kx0; kx < kx1; kx++)
  {
    const float2 c = C[(size_t) kx * H], f = F[(size_t) kx * H];
    const double cr = (double) c.x, ci = (double) c.y, fr = (double) f.x, fi = (double) f.y;
    const double zr = fma(cr, fr, ci * fi), zi = fma(ci, fr, -(cr * fi));
#pragma unroll
    for (int j = 0; j < kWindowRows; j++)
    {
      const double2 e = make_double2(w[2 * t[j]], w[2 * t[j] + 1]);
      ar[j] = fma(zr, e.x, ar[j]);
      ar[j] = fma(-zi, e.y, ar[j]);
      ai[j] = fma(zr, e.y, ai[j]);
      ai[j] = fma(zi, e.x, ai[j]);
      t[j] += step[j];
      t[j] = t[j] >= N ? t[j] - N : t[j];
    }
  }
  if (wave)
  {
#pragma unroll
    for (int j = 0; j < kWindowRows; j++)
      part[wave - 1][j][lane] = make_double2(ar[j], ai[j]);
  }
  __syncthreads();
  if (wave || !live)
    return;
  const double wgt = (ky == 0 || 2 * ky == N) ? 1. : 2.;
#pragma unroll
  for (int j = 0; j < kWindowRows; j++)
  {
#pragma unroll
    for (int q = 0; q < kWindowSplit - 1; q++)
    {
      ar[j] += part[q][j][lane].x;
      ai[j] += part[q][j][lane].y;
    }
    if (row0 + j < nd)
      T[((size_t) r * nd + row0 + j) * H + ky] = make_double2(wgt * ar[j], wgt * ai[j]);
  }
}

// Cell pass.  grid (window rows, records), one wave per block: lane = cell j along dy (chunks of 64 for nd > 64), ky
// ascends with T wave-uniform and the lane's twiddle index stepped by dy; then the reference's float rounding and float
// division (bioem_algorithm.h:163-164) and the log posterior, which stays a double.
__global__ __launch_bounds__(64) void k_window_cells(const double2 *__restrict__ T, const BioemWindowRecord *__restrict__ rec,
                                                     const bioem_hip_param5 *__restrict__ params,
                                                     const double2 *__restrict__ postc, const float *__restrict__ sumRef,
                                                     const float *__restrict__ sumsqRef, const PD pd, int N, int H, int nd,
                                                     const int *__restrict__ shifts, const double2 *__restrict__ tw,
                                                     double *__restrict__ logp, float *__restrict__ cc)
{
  const int i = blockIdx.x, r = blockIdx.y, lane = threadIdx.x;
  const double2 *Trow = T + ((size_t) r * nd + i) * H;
  const bioem_hip_param5 q = params[r];
  const double2 pc = postc[r];
  const int p = rec[r].particle;
  const float sr = sumRef[p], ssr = sumsqRef[p];
  const float nn = (float) (N * N);
  for (int j0 = 0; j0 < nd; j0 += 64)
  {
    const int j = j0 + lane;
    const int step = window_step(shifts[min(j, nd - 1)], N);
    int t = 0;
    double S = 0.;
#pragma unroll 8 // eight steps' loads in flight; the sum keeps its order
    for (int ky = 0; ky < H; ky++)
    {
      const double2 v = Trow[ky], e = tw[t];
      S = fma(v.x, e.x, S);
      S = fma(-v.y, e.y, S);
      t += step;
      t = t >= N ? t - N : t;
    }
    if (j < nd)
    {
      const float value = (float) S / nn;
      const size_t o = ((size_t) r * nd + i) * nd + j;
      logp[o] = logpro_eval(pd, q, value, sr, ssr, pc.x, pc.y);
      cc[o] = value;
    }
  }
}

} // namespace
#endif // BIOEM_WINDOW_TU

#endif
