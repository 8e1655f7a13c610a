// view_kernels.hpp -- aligned averages of the particles of a view (bioem_hip_view_sums, bioem_hip_view_averages,
// bioem_hip_debug_view_sums).  For the record (c, X, Y, norm, mu), the weight w and the group g of particle p,
// with R_p its float spectrum in reference layout, K_c the CTF kernel and tw[j] = exp(+2 pi i j / N), all in double:
//   A_p[k1][k2] = (R_p[k1][k2] - mu N^2 [k1 = k2 = 0]) tw[(k1 X + k2 Y) mod N]
//   K~_c = K_c, in the columns k2 = 0 and (N even) N / 2 its Hermitian part (K_c[k1] + conj(K_c[(N - k1) mod N])) / 2
//   num_g[k] = sum_p (w norm) K~_c[k] A_p[k],  den_g[k] = sum_p (w norm^2) |K~_c[k]|^2    over the members of g, ascending p
//   P^_g[k]  = num_g[k] / (den_g[k] + tau_g),  tau_g = wiener mean_k den_g[k],  0 where the denominator is 0
// the least-squares estimate of the projection P from R ~ norm P conj(K~) tw[-(k1 X + k2 Y)] + mu N^2 delta, the model of
// the ring pass (ring_kernels.hpp): a particle is a real image, so in the columns that are their own Hermitian partner
// its spectrum carries the Hermitian part of P conj(K) along k1 only (the reference's CTF kernels are not even in k1),
// and with K~ the estimate is Hermitian there as P is.  No reference counterpart.  The declarations are for every
// translation unit; the kernels are compiled by kernels_views.hip only (BIOEM_VIEW_TU).
#ifndef BIOEM_VIEW_KERNELS_HPP
#define BIOEM_VIEW_KERNELS_HPP

#include "engine_types.hpp"

// one member of a batch, made by the host: the scalars are products of doubles, rounded once each as written
struct BioemViewMember
{
  int slot;   // image of the batch's spectrum buffer
  int conv;   // CTF set
  int xm, ym; // X mod N, Y mod N in [0, N)
  double s;   // w * (double) norm
  double s2;  // s * (double) norm
  double dc;  // (double) mu * N * N
};

const int kViewThreads = 256; // lanes of a block; each owns two neighbouring coefficients
const int kViewUnroll = 4;    // members whose loads are in flight before the first is consumed

// num[g][M] / den[g][M] += the members off[g] ... off[g + 1] - 1 of mem, for g in [0, nGroups): specR = [slots][M] float2
// in reference layout, ctf = the uploaded kernels, tw = N double pairs.  The buffers continue over the launches of a
// stream: a lane owns its (group, coefficient), so the order of a group's additions is the order of its members.
BIOEM_HIDDEN hipError_t bioem_view_accumulate_launch(hipStream_t st, const float2 *specR, const float2 *ctf,
                                                     const BioemViewMember *mem, const int *off, int nGroups, int N,
                                                     const double2 *tw, double2 *num, double *den);
// tau[g] = wiener * mean_k den[g][k] (a fixed tree), then dst[g][M] = (float2) (num / (den + tau)), 0 where den + tau is 0
BIOEM_HIDDEN hipError_t bioem_view_wiener_launch(hipStream_t st, const double2 *num, const double *den, int nGroups, int N,
                                                 double wiener, double *tau, float2 *dst);

#ifdef BIOEM_VIEW_TU
namespace
{

// a 16-byte load of two neighbouring float2: a spectrum of an odd number of coefficients starts at an odd multiple of 8
typedef float view_pair __attribute__((ext_vector_type(4), aligned(8)));

// v mod N for v < 2^24 (v <= (N - 1)(N - 1 + N / 2) with N <= 2560): the quotient estimate is off by one at most
__device__ inline unsigned view_mod(unsigned v, unsigned N, float rN)
{
  const unsigned q = (unsigned) ((float) v * rN);
  int r = (int) (v - q * N);
  r = r < 0 ? r + (int) N : r;
  r = r >= (int) N ? r - (int) N : r;
  return (unsigned) r;
}

// the operands of one member for the lane's two coefficients
struct ViewOperands
{
  view_pair r, k;
  float2 kc0, kc1; // the kernel at the Hermitian partners of the two coefficients (at the coefficients themselves elsewhere)
  double2 w0, w1;
  double s, s2, dc;
};

__device__ inline ViewOperands view_fetch(const BioemViewMember *__restrict__ m, const float2 *__restrict__ specR,
                                          const float2 *__restrict__ ctf, const double2 *__restrict__ tw, size_t M,
                                          unsigned ld, unsigned pa, unsigned pb, unsigned k1a, unsigned k2a, unsigned k1b,
                                          unsigned k2b, unsigned N, float rN)
{
  ViewOperands o;
  // block-uniform: scalar loads
  const int slot = m->slot, conv = m->conv;
  const unsigned xm = (unsigned) m->xm, ym = (unsigned) m->ym;
  o.s = m->s;
  o.s2 = m->s2;
  o.dc = m->dc;
  // the particle's row is read once: non-temporal; the CTF kernel is shared by the blocks of its set
  o.r = __builtin_nontemporal_load(reinterpret_cast<const view_pair *>(specR + (size_t) slot * M + ld));
  o.k = *reinterpret_cast<const view_pair *>(ctf + (size_t) conv * M + ld);
  o.kc0 = ctf[(size_t) conv * M + pa];
  o.kc1 = ctf[(size_t) conv * M + pb];
  o.w0 = tw[view_mod(k1a * xm + k2a * ym, N, rN)];
  o.w1 = tw[view_mod(k1b * xm + k2b * ym, N, rN)];
  return o;
}

// num += (s K~) ((R - dc) w), den += s2 |K~|^2 for one coefficient, K~ = (K + conj(Kc)) / 2 where self, else K; no
// contraction: every product and sum rounds once
__device__ inline void view_term(float rx, float ry, float kx, float ky, float2 kc, bool self, double2 w, double s, double s2,
                                 double dc, double &nr, double &ni, double &dn)
{
  const double xr = (double) rx - dc, xi = (double) ry;
  const double ar = xr * w.x - xi * w.y, ai = xr * w.y + xi * w.x;
  const double hx = self ? 0.5 * ((double) kx + (double) kc.x) : (double) kx;
  const double hy = self ? 0.5 * ((double) ky - (double) kc.y) : (double) ky;
  const double kr = s * hx, ki = s * hy;
  nr += kr * ar - ki * ai;
  ni += kr * ai + ki * ar;
  dn += s2 * (hx * hx + hy * hy);
}

// Block (tile, group) of kViewThreads lanes; lane l owns the coefficients e0 = 2 (tile kViewThreads + l) and e0 + 1 of the
// [N][H] spectrum and carries their num / den in registers over the group's members of this launch, kViewUnroll at a
// time: all their loads are issued before the first is consumed.  Where the spectrum has an odd number of coefficients
// the last lane loads the pair that ends with its coefficient.
__global__ __launch_bounds__(kViewThreads) void k_view_accumulate(const float2 *__restrict__ specR,
                                                                  const float2 *__restrict__ ctf,
                                                                  const BioemViewMember *__restrict__ mem,
                                                                  const int *__restrict__ off, int N, int H,
                                                                  const double2 *__restrict__ tw, double2 *__restrict__ num,
                                                                  double *__restrict__ den)
{
  const int g = blockIdx.y;
  const int mb = off[g], me = off[g + 1]; // block-uniform
  if (mb >= me)
    return;
  const size_t M = (size_t) N * H;
  const size_t e0 = 2 * ((size_t) blockIdx.x * kViewThreads + threadIdx.x);
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
  const float rN = 1.f / (float) N;
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
  auto step = [&](const ViewOperands &o) {
    const float r0x = two ? o.r.x : o.r.z, r0y = two ? o.r.y : o.r.w;
    const float k0x = two ? o.k.x : o.k.z, k0y = two ? o.k.y : o.k.w;
    view_term(r0x, r0y, k0x, k0y, o.kc0, selfA, o.w0, o.s, o.s2, origin ? o.dc : 0., n0r, n0i, d0);
    view_term(o.r.z, o.r.w, o.k.z, o.k.w, o.kc1, selfB, o.w1, o.s, o.s2, 0., n1r, n1i, d1);
  };
  int i = mb;
  for (; i + kViewUnroll <= me; i += kViewUnroll)
  {
    ViewOperands o[kViewUnroll];
#pragma unroll
    for (int u = 0; u < kViewUnroll; u++)
      o[u] = view_fetch(mem + i + u, specR, ctf, tw, M, ld, pa, pb, k1a, k2a, k1b, k2b, (unsigned) N, rN);
    __builtin_amdgcn_sched_barrier(0); // every load of the trip is issued before the first is waited for
#pragma unroll
    for (int u = 0; u < kViewUnroll; u++) // in member order
      step(o[u]);
  }
  for (; i < me; i++)
    step(view_fetch(mem + i, specR, ctf, tw, M, ld, pa, pb, k1a, k2a, k1b, k2b, (unsigned) N, rN));
  pn[0] = make_double2(n0r, n0i);
  pd[0] = d0;
  if (two)
  {
    pn[1] = make_double2(n1r, n1i);
    pd[1] = d1;
  }
}

// tau[g] = wiener * (sum_k den[g][k]) / M: lane l adds the coefficients l, l + 256, ... in that order, the block folds
// the 256 lane sums over the fixed tree of distances 128, 64, ... 1; a block per group
__global__ __launch_bounds__(256) void k_view_tau(const double *__restrict__ den, int M, double wiener,
                                                  double *__restrict__ tau)
{
  __shared__ double part[256];
  const double *d = den + (size_t) blockIdx.x * M;
  double v = 0.;
  for (int k = threadIdx.x; k < M; k += 256)
    v += d[k];
  part[threadIdx.x] = v;
  __syncthreads();
  for (int s = 128; s >= 1; s >>= 1)
  {
    if ((int) threadIdx.x < s)
      part[threadIdx.x] += part[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0)
    tau[blockIdx.x] = wiener * (part[0] / (double) M);
}

// dst[g][k] = num[g][k] / (den[g][k] + tau[g]) rounded to float, 0 where the denominator is 0; grid (tiles, groups)
__global__ __launch_bounds__(256) void k_view_wiener(const double2 *__restrict__ num, const double *__restrict__ den,
                                                     const double *__restrict__ tau, int M, float2 *__restrict__ dst)
{
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= M)
    return;
  const size_t e = (size_t) blockIdx.y * M + k;
  const double d = den[e] + tau[blockIdx.y];
  const double2 n = num[e];
  dst[e] = d != 0. ? make_float2((float) (n.x / d), (float) (n.y / d)) : make_float2(0.f, 0.f);
}

} // namespace
#endif // BIOEM_VIEW_TU

#endif
