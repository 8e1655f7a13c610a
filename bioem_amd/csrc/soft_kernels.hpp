// soft_kernels.hpp -- posterior-weighted view sums (bioem_hip_view_sums_soft, bioem_hip_debug_view_sums_soft,
// bioem_hip_reconstruct_soft).  A member r = (particle p, group g, CTF set c) carries a table a_r[i][j] of
// doubles over the cells (X_i, X_j) of a shift list X_0 ... X_{nd - 1} and the scalars s2_r, b_r.  With R_p, K~_c and tw
// as in view_kernels.hpp, all in double:
//   U_r[i][k2]  = sum_j a_r[i][j] tw[(k2 X_j) mod N]                 j ascending   (k_soft_cols)
//   W_r[k1][k2] = sum_i tw[(k1 X_i) mod N] U_r[i][k2]                i ascending   (k_soft_rows)
//   num_g[k]   += K~_c[k] (R_p[k] W_r[k] - [k = 0] b_r N^2),  den_g[k] += s2_r |K~_c[k]|^2       (k_soft_accumulate)
// over the members of g in ascending (particle, position in the member list): the sum of view_kernels.hpp averaged over
// the cells, each cell with its own norm and mu (a = w norm, s2 = sum w norm^2, b = sum w norm mu).  Every product and sum
// rounds once (no contraction), twiddle indices are reduced in integers.  No reference counterpart.  The declarations are
// for every translation unit; the kernels are compiled by kernels_soft.hip only (BIOEM_SOFT_TU).
#ifndef BIOEM_SOFT_KERNELS_HPP
#define BIOEM_SOFT_KERNELS_HPP

#include "engine_types.hpp"

// one member of a launch, made by the host
struct BioemSoftMember
{
  int slot; // image of the batch's spectrum buffer
  int conv; // CTF set
  int tab;  // table of the launch's W buffer
  int pad;
  double s2;
  double dc; // b * N * N, rounded once
};

const int kSoftThreads = 256;     // lanes of an accumulation block; each owns two neighbouring coefficients
const int kSoftUnroll = 4;        // members whose loads are in flight before the first is consumed
const int kSoftTableThreads = 128; // lanes of a block of the two table passes; each owns one k2
const int kSoftRows = 4;          // rows k1 of W a block of the row pass carries per load of U
const int kSoftChunk = 256;       // twiddles per row the row pass stages in LDS at a time

// U [n][nd][H] of the n tables cells [n][nd][nd], then W [n][N][H] of U; xm [nd] = X_i mod N in [0, N), tw = N double pairs
// (the host's table of these entries is exact at the multiples of a quarter turn)
BIOEM_HIDDEN hipError_t bioem_soft_cols_launch(hipStream_t st, const double *cells, const int *xm, int n, int nd, int N,
                                               const double2 *tw, double2 *U);
BIOEM_HIDDEN hipError_t bioem_soft_rows_launch(hipStream_t st, const double2 *U, const int *xm, int n, int nd, int N,
                                               const double2 *tw, double2 *W);
// num[g][M] / den[g][M] += the members off[g] ... off[g + 1] - 1 of mem, for g in [0, nGroups): as
// bioem_view_accumulate_launch, with W [tables][M] read where that kernel looks up one twiddle
BIOEM_HIDDEN hipError_t bioem_soft_accumulate_launch(hipStream_t st, const float2 *specR, const float2 *ctf,
                                                     const BioemSoftMember *mem, const int *off, int nGroups, int N,
                                                     const double2 *W, double2 *num, double *den);

#ifdef BIOEM_SOFT_TU
namespace
{

// a 16-byte load of two neighbouring float2: a spectrum of an odd number of coefficients starts at an odd multiple of 8
typedef float soft_pair __attribute__((ext_vector_type(4), aligned(8)));

// v mod N for v < 2^24 (v <= (N - 1)^2 with N <= 4096, checked by the launcher): the quotient estimate is off by one at most
__device__ inline unsigned soft_mod(unsigned v, unsigned N, float rN)
{
  const unsigned q = (unsigned) ((float) v * rN);
  int r = (int) (v - q * N);
  r = r < 0 ? r + (int) N : r;
  r = r >= (int) N ? r - (int) N : r;
  return (unsigned) r;
}

// Block (i, table) of kSoftTableThreads lanes; lane l owns k2 = l, l + kSoftTableThreads, ... of row i of U.  The row of
// the table and the shifts are block-uniform.
__global__ __launch_bounds__(kSoftTableThreads) void k_soft_cols(const double *__restrict__ cells,
                                                                 const int *__restrict__ xm, int nd, int N, int H,
                                                                 const double2 *__restrict__ tw, double2 *__restrict__ U)
{
  const size_t row = (size_t) blockIdx.y * nd + blockIdx.x;
  const double *a = cells + row * nd;
  double2 *u = U + row * H;
  const float rN = 1.f / (float) N;
  for (int k2 = threadIdx.x; k2 < H; k2 += kSoftTableThreads)
  {
    double ur = 0., ui = 0.;
    for (int j = 0; j < nd; j++)
    {
      const double2 t = tw[soft_mod((unsigned) k2 * (unsigned) xm[j], (unsigned) N, rN)];
      const double aj = a[j];
      ur += aj * t.x;
      ui += aj * t.y;
    }
    u[k2] = make_double2(ur, ui);
  }
}

// Block (kSoftRows rows k1, tile of k2, table) of kSoftTableThreads lanes; lane l owns W[k1][tile kSoftTableThreads + l] of
// the block's rows and reads U[i][k2] once for all of them.  The twiddles tw[(k1 X_i) mod N] of the rows are staged in LDS,
// kSoftChunk per row at a time, by the lanes of the block.
__global__ __launch_bounds__(kSoftTableThreads) void k_soft_rows(const double2 *__restrict__ U, const int *__restrict__ xm,
                                                                 int nd, int N, int H, const double2 *__restrict__ tw,
                                                                 double2 *__restrict__ W)
{
  __shared__ double2 t[kSoftRows][kSoftChunk];
  const unsigned k1b = blockIdx.x * kSoftRows;
  const int k2 = blockIdx.y * kSoftTableThreads + threadIdx.x;
  const bool live = k2 < H;
  const double2 *u = U + (size_t) blockIdx.z * nd * H + (live ? k2 : 0);
  const float rN = 1.f / (float) N;
  double wr[kSoftRows], wi[kSoftRows];
#pragma unroll
  for (int r = 0; r < kSoftRows; r++)
    wr[r] = wi[r] = 0.;
  for (int i0 = 0; i0 < nd; i0 += kSoftChunk)
  {
    const int ni = min(kSoftChunk, nd - i0);
    if (i0)
      __syncthreads(); // the chunk before has been read
    for (int e = threadIdx.x; e < kSoftRows * ni; e += kSoftTableThreads)
    {
      const int r = e / ni, i = e - r * ni;
      const unsigned k1 = min(k1b + (unsigned) r, (unsigned) N - 1u); // (a row beyond the image is computed and not stored)
      t[r][i] = tw[soft_mod(k1 * (unsigned) xm[i0 + i], (unsigned) N, rN)];
    }
    __syncthreads();
    if (live)
      for (int i = 0; i < ni; i++)
      {
        const double2 ui = u[(size_t) (i0 + i) * H];
#pragma unroll
        for (int r = 0; r < kSoftRows; r++)
        {
          const double2 ti = t[r][i];
          const double pr = ti.x * ui.x - ti.y * ui.y, pi = ti.x * ui.y + ti.y * ui.x;
          wr[r] += pr;
          wi[r] += pi;
        }
      }
  }
  if (live)
#pragma unroll
    for (int r = 0; r < kSoftRows; r++)
      if (k1b + (unsigned) r < (unsigned) N)
        W[((size_t) blockIdx.z * N + k1b + r) * H + k2] = make_double2(wr[r], wi[r]);
}

// the operands of one member for the lane's two coefficients
struct SoftOperands
{
  soft_pair r, k;
  float2 kc0, kc1; // the kernel at the Hermitian partners of the two coefficients (at the coefficients themselves elsewhere)
  double2 w0, w1;
  double s2, dc;
};

__device__ inline SoftOperands soft_fetch(const BioemSoftMember *__restrict__ m, const float2 *__restrict__ specR,
                                          const float2 *__restrict__ ctf, const double2 *__restrict__ W, size_t M, unsigned ld,
                                          unsigned pa, unsigned pb, size_t e0, size_t e1)
{
  SoftOperands o;
  // block-uniform: scalar loads
  const int slot = m->slot, conv = m->conv, tab = m->tab;
  o.s2 = m->s2;
  o.dc = m->dc;
  // the particle's row is read once: non-temporal; the CTF kernel is shared by the blocks of its set
  o.r = __builtin_nontemporal_load(reinterpret_cast<const soft_pair *>(specR + (size_t) slot * M + ld));
  o.k = *reinterpret_cast<const soft_pair *>(ctf + (size_t) conv * M + ld);
  o.kc0 = ctf[(size_t) conv * M + pa];
  o.kc1 = ctf[(size_t) conv * M + pb];
  const double2 *w = W + (size_t) tab * M;
  o.w0 = w[e0];
  o.w1 = w[e1];
  return o;
}

// num += K~ (R W - dc), den += s2 |K~|^2 for one coefficient, K~ = (K + conj(Kc)) / 2 where self, else K; no contraction:
// every product and sum rounds once
__device__ inline void soft_term(float rx, float ry, float kx, float ky, float2 kc, bool self, double2 w, double s2, double dc,
                                 double &nr, double &ni, double &dn)
{
  const double xr = (double) rx, xi = (double) ry;
  const double ar = (xr * w.x - xi * w.y) - dc, ai = xr * w.y + xi * w.x;
  const double hx = self ? 0.5 * ((double) kx + (double) kc.x) : (double) kx;
  const double hy = self ? 0.5 * ((double) ky - (double) kc.y) : (double) ky;
  nr += hx * ar - hy * ai;
  ni += hx * ai + hy * ar;
  dn += s2 * (hx * hx + hy * hy);
}

// Block (tile, group) of kSoftThreads lanes, the shape of k_view_accumulate: lane l owns the coefficients
// e0 = 2 (tile kSoftThreads + l) and e0 + 1 of the [N][H] spectrum and carries their num / den in registers over the
// group's members of this launch, kSoftUnroll at a time.  Where the spectrum has an odd number of coefficients the last
// lane loads the pair that ends with its coefficient.
__global__ __launch_bounds__(kSoftThreads) void k_soft_accumulate(const float2 *__restrict__ specR,
                                                                  const float2 *__restrict__ ctf,
                                                                  const BioemSoftMember *__restrict__ mem,
                                                                  const int *__restrict__ off, int N, int H,
                                                                  const double2 *__restrict__ W, double2 *__restrict__ num,
                                                                  double *__restrict__ den)
{
  const int g = blockIdx.y;
  const int mb = off[g], me = off[g + 1]; // block-uniform
  if (mb >= me)
    return;
  const size_t M = (size_t) N * H;
  const size_t e0 = 2 * ((size_t) blockIdx.x * kSoftThreads + threadIdx.x);
  if (e0 >= M)
    return;
  const bool two = e0 + 1 < M;
  const unsigned ld = (unsigned) (two ? e0 : e0 - 1); // M >= 2
  const size_t e1 = two ? e0 + 1 : e0;
  const unsigned k1a = (unsigned) (e0 / H), k2a = (unsigned) (e0 - (size_t) k1a * H);
  const unsigned k1b = (unsigned) (e1 / H), k2b = (unsigned) (e1 - (size_t) k1b * H);
  // the columns that are their own Hermitian partner, and the partner's place (k1 -> (N - k1) mod N)
  const bool selfA = k2a == 0 || 2 * k2a == (unsigned) N, selfB = k2b == 0 || 2 * k2b == (unsigned) N;
  const unsigned pa = selfA ? (k1a ? (unsigned) N - k1a : 0u) * (unsigned) H + k2a : (unsigned) e0;
  const unsigned pb = selfB ? (k1b ? (unsigned) N - k1b : 0u) * (unsigned) H + k2b : (unsigned) e1;
  const bool origin = e0 == 0; // the offset lives in coefficient (0, 0) only
  double2 *pn = num + (size_t) g * M + e0;
  double *pd = den + (size_t) g * M + e0;
  double n0r = pn[0].x, n0i = pn[0].y, d0 = pd[0];
  double n1r = 0., n1i = 0., d1 = 0.;
  if (two)
  {
    n1r = pn[1].x;
    n1i = pn[1].y;
    d1 = pd[1];
  }
  auto step = [&](const SoftOperands &o) {
    const float r0x = two ? o.r.x : o.r.z, r0y = two ? o.r.y : o.r.w;
    const float k0x = two ? o.k.x : o.k.z, k0y = two ? o.k.y : o.k.w;
    soft_term(r0x, r0y, k0x, k0y, o.kc0, selfA, o.w0, o.s2, origin ? o.dc : 0., n0r, n0i, d0);
    soft_term(o.r.z, o.r.w, o.k.z, o.k.w, o.kc1, selfB, o.w1, o.s2, 0., n1r, n1i, d1);
  };
  int i = mb;
  for (; i + kSoftUnroll <= me; i += kSoftUnroll)
  {
    SoftOperands o[kSoftUnroll];
#pragma unroll
    for (int u = 0; u < kSoftUnroll; u++)
      o[u] = soft_fetch(mem + i + u, specR, ctf, W, M, ld, pa, pb, e0, e1);
    __builtin_amdgcn_sched_barrier(0); // every load of the trip is issued before the first is waited for
#pragma unroll
    for (int u = 0; u < kSoftUnroll; u++) // in member order
      step(o[u]);
  }
  for (; i < me; i++)
    step(soft_fetch(mem + i, specR, ctf, W, M, ld, pa, pb, e0, e1));
  pn[0] = make_double2(n0r, n0i);
  pd[0] = d0;
  if (two)
  {
    pn[1] = make_double2(n1r, n1i);
    pd[1] = d1;
  }
}

} // namespace
#endif // BIOEM_SOFT_TU

#endif
