// ctfgrad_kernels.hpp -- the gradient and the curvature of the log posterior of a request with respect to the CTF triple
// theta = (amp, pha, env) of its CTF set (bioem_hip_ctf_gradient, bioem_hip_debug_ctf_gradient).  CTF mode
// only: the host's kernel (ctf_kernel_one) is then the real closed form
//   k(s; theta) = exp(-env s / 2) (cos(pha s / 2) + rho sin(pha s / 2)),  rho = sqrt(1 - amp^2) / amp,  k(0) = 1,
// of the radial variable s of a stored element: the float the host's expression gives for (rowIdx(row), column), read
// from the table radsq[i^2 + j^2] the host fills with its own float operations (never divided again on the device).
// The conventions are those of scan_kernels.hpp and grad_kernels.hpp: the walk order, Pw the projection's spectrum in it,
// Z = w conj(F) tw in it, M = N H positions, Nt = N N, a, b, g of k_grad_coef.  Per position, in double, every operation
// written down and unfused (a = amp, q2 = 1 - a a, q = sqrt(q2), a2 = a a):
//   rho = q / a,  rho1 = -(1 / (a2 q)),  rho2 = (2 - 3 a2) / ((q2 q) (a2 a))          rho and its two derivatives
//   u = 0.5 s,  u2 = u u,  E = exp(-(0.5 xe)),  S = sin(0.5 xp),  C = cos(0.5 xp),  Eu = E u
// where xe = env s and xp = pha s are the host's FLOAT products, widened: exp, sin and cos are taken at the very arguments
// the host's kernel was made at (its roundings are not differentiated: d xp / d pha = s, d xe / d env = s), so k is the
// kernel the comparison used up to the host's roundings of the value itself.
//   k    = E (C + rho S)
//   D_a  = E (rho1 S)           D_p  = Eu ((rho C) - S)      D_e  = -(u k)
//   D_aa = E (rho2 S)           D_ap = Eu (rho1 C)           D_ae = -(u D_a)
//   D_pp = -(u2 k)              D_pe = -(u D_p)              D_ee = u2 k
//   A = w ((P.re P.re) + (P.im P.im)),  w = 1 in columns 0 and N / 2, else 2;   B = (P.re Z.re) - (P.im Z.im)
// and the twenty terms, t, u over (a, p, e), the pairs in the order aa, ap, ae, pp, pe, ee:
//   0 ss0 = A (k k)      1 cc0 = B k      2 + t  U_t = A (k D_t)      5 + t  V_t = B D_t
//   8 + tu  UU_tu = A ((D_t D_u) + (k D_tu))                           14 + tu  VV_tu = B D_tu
// k_ctfgrad_partials: block = 256 consecutive positions of one request; each term is folded over the 64 lanes of a wave by
// the tree of distances 32, 16, 8, 4, 2, 1 (x[l] = x[l] + x[l ^ d]), then over the four waves as (w0 + w1) + (w2 + w3):
// partial[request][block][20].  A lane without a position has the term +0.0.  theta of the request's set is wave-uniform.
// k_ctfgrad_fold: one lane per (request, sum) adds the blocks in ascending order from +0.0.
// k_ctfgrad_finish: one lane per request: the second derivatives L_bb, L_bg, L_gg of the closed form of k_grad_coef with
// respect to (sumsquareC, cc) at the same linearisation point, the data part and the prior part of gradient and Hessian
// apart, and the row of 38 doubles (include/bioem_hip.h).
// No atomics; a row's bits depend on its request alone, not on the batch, its place in it, the other requests or the run.
// The declarations are for every translation unit; the kernels are compiled by kernels_ctfgrad.hip only (BIOEM_CTFGRAD_TU).
#ifndef BIOEM_CTFGRAD_KERNELS_HPP
#define BIOEM_CTFGRAD_KERNELS_HPP

#include "engine_types.hpp"
#include "grad_kernels.hpp" // (BioemGradRecord)

const int kCtfgSums = 20;   // ss0, cc0, U[3], V[3], UU[6], VV[6]
const int kCtfgDerivs = 10; // k, D_t[3], D_tu[6]
const int kCtfgRow = 38;    // theta[3], the sums, gData[3], gPrior[3], HData[6], HPrior[3]
const int kCtfgBlock = 256; // positions of a block

// blocks of a request: ceil(N H / kCtfgBlock)
BIOEM_HIDDEN int bioem_ctfgrad_blocks(int N);
// sums[n][20] of the n requests from Pw / Z [n][M] (walk order), theta = ctfParam[rec[i].kernel][3]; rowIdx[N] and
// radsq[2 (H - 1)^2 + 1] the host's tables; partial: n bioem_ctfgrad_blocks(N) 20 doubles of staging; derivs [n][M][10] or
// null
BIOEM_HIDDEN hipError_t bioem_ctfgrad_sums_launch(hipStream_t st, const float2 *Pw, const double2 *Z,
                                                  const BioemGradRecord *rec, const float *ctfParam, const int *rowIdx,
                                                  const float *radsq, int n, int N, double *partial, double *sums,
                                                  double *derivs);
// row[n][38] from the sums, the coefficients coef[n][4] of k_grad_coef and the arrays it read
BIOEM_HIDDEN hipError_t bioem_ctfgrad_finish_launch(hipStream_t st, const double *sums, const BioemGradRecord *rec,
                                                    const float *cc, const bioem_hip_param5 *params, const float *sumRef,
                                                    const float *sumsqRef, const double *coef,
                                                    const bioem_hip_param_device &pd, int n, int N, double *row);

#ifdef BIOEM_CTFGRAD_TU

namespace
{

__global__ __launch_bounds__(kCtfgBlock) void k_ctfgrad_partials(const float2 *__restrict__ Pw, const double2 *__restrict__ Z,
                                                                 const BioemGradRecord *__restrict__ rec,
                                                                 const float *__restrict__ ctfParam,
                                                                 const int *__restrict__ rowIdx,
                                                                 const float *__restrict__ radsq, int N, int H,
                                                                 double *__restrict__ partial, double *__restrict__ derivs)
{
  __shared__ double red[4][kCtfgSums];
  const int g = blockIdx.y;
  const int M = N * H;
  const int jend = (N & 1) ? H : H - 1;
  const int at = blockIdx.x * kCtfgBlock + (int) threadIdx.x;
  const bool have = at < M;
  const int pos = have ? at : M - 1; // (a lane without a position reads the last one and drops its terms)
  const int r = pos / H, c = pos - r * H;
  const int j = c < jend - 1 ? c + 1 : (c == jend - 1 ? 0 : H - 1); // the walk order: interior columns, 0, N / 2
  const int i = rowIdx[r];
  const float sf = radsq[i * i + j * j];
  const float2 p = Pw[(size_t) g * M + pos];
  const double2 z = Z[(size_t) g * M + pos];
  const float *th = ctfParam + 3 * (size_t) rec[g].kernel; // wave-uniform: scalar loads
  const double a = (double) th[0], s = (double) sf;
  const double xp = (double) (th[1] * sf), xe = (double) (th[2] * sf); // the host's float products
  const double a2 = a * a, q2 = 1. - a2, q = sqrt(q2);
  const double rho = q / a, rho1 = -(1. / (a2 * q)), rho2 = (2. - 3. * a2) / ((q2 * q) * (a2 * a));
  const double u = 0.5 * s, u2 = u * u;
  const double E = exp(-(0.5 * xe));
  double S, C;
  sincos(0.5 * xp, &S, &C);
  const double Eu = E * u;
  double d[kCtfgDerivs];
  const double k = E * (C + rho * S);
  d[0] = k;
  d[1] = E * (rho1 * S);
  d[2] = Eu * ((rho * C) - S);
  d[3] = -(u * k);
  d[4] = E * (rho2 * S);
  d[5] = Eu * (rho1 * C);
  d[6] = -(u * d[1]);
  d[7] = -(u2 * k);
  d[8] = -(u * d[2]);
  d[9] = u2 * k;
  if (derivs && have)
  {
    double *o = derivs + ((size_t) g * M + pos) * kCtfgDerivs;
#pragma unroll
    for (int t = 0; t < kCtfgDerivs; t++)
      o[t] = d[t];
  }
  const double pr = (double) p.x, pi = (double) p.y;
  const double w = (j == 0 || 2 * j == N) ? 1. : 2.;
  const double A = w * ((pr * pr) + (pi * pi)), B = (pr * z.x) - (pi * z.y);
  double t[kCtfgSums];
  t[0] = A * (k * k);
  t[1] = B * k;
#pragma unroll
  for (int e = 0; e < 3; e++)
  {
    t[2 + e] = A * (k * d[1 + e]);
    t[5 + e] = B * d[1 + e];
  }
  {
    int pair = 0;
#pragma unroll
    for (int e = 0; e < 3; e++)
#pragma unroll
      for (int f = e; f < 3; f++, pair++)
      {
        t[8 + pair] = A * ((d[1 + e] * d[1 + f]) + (k * d[4 + pair]));
        t[14 + pair] = B * d[4 + pair];
      }
  }
#pragma unroll
  for (int e = 0; e < kCtfgSums; e++)
  {
    double y = have ? t[e] : 0.;
#pragma unroll
    for (int dist = 32; dist >= 1; dist >>= 1)
      y = y + __shfl_xor(y, dist, 64);
    t[e] = y;
  }
  if ((threadIdx.x & 63) == 0)
  {
#pragma unroll
    for (int e = 0; e < kCtfgSums; e++)
      red[threadIdx.x >> 6][e] = t[e];
  }
  __syncthreads();
  if (threadIdx.x < kCtfgSums)
  {
    const int e = threadIdx.x;
    partial[((size_t) g * gridDim.x + blockIdx.x) * kCtfgSums + e] = (red[0][e] + red[1][e]) + (red[2][e] + red[3][e]);
  }
}

// grid (ceil(20 n / 64)): lane (request, sum)
__global__ __launch_bounds__(64) void k_ctfgrad_fold(const double *__restrict__ partial, int n, int blocks,
                                                     double *__restrict__ sums)
{
  const int t = blockIdx.x * 64 + threadIdx.x;
  if (t >= kCtfgSums * n)
    return;
  const int g = t / kCtfgSums, e = t - g * kCtfgSums;
  const double *p = partial + (size_t) g * blocks * kCtfgSums + e;
  double y = 0.;
  for (int i = 0; i < blocks; i++)
    y = y + p[(size_t) i * kCtfgSums];
  sums[t] = y;
}

// grid (ceil(n / 64)): lane = request.  The linearisation point is read as k_grad_coef reads it; b and g are its own
__global__ __launch_bounds__(64) void k_ctfgrad_finish(const double *__restrict__ sums, const BioemGradRecord *__restrict__ rec,
                                                       const float *__restrict__ cc,
                                                       const bioem_hip_param5 *__restrict__ params,
                                                       const float *__restrict__ sumRef, const float *__restrict__ sumsqRef,
                                                       const double *__restrict__ coef, const PD pd, int n, double Nt,
                                                       double *__restrict__ row)
{
  const int r = blockIdx.x * 64 + threadIdx.x;
  if (r >= n)
    return;
  const BioemGradRecord q = rec[r];
  const bioem_hip_param5 p = params[q.cell];
  const double s = (double) p.sumC, ssq = (double) p.sumsquareC, c = (double) cc[q.cell];
  const double sr = (double) sumRef[q.sums], ssr = (double) sumsqRef[q.sums];
  const double F = ssq * Nt - s * s;
  const double fe = Nt * (ssr * ssq - c * c) + 2. * sr * s * c - ssr * s * s - sr * sr * ssq;
  const double h1 = (3. - Nt) * 0.5, h2 = Nt * 0.5 - 2.;
  const double fq = Nt * ssr - sr * sr, fc = -2. * Nt * c + 2. * sr * s;
  const double Lbb = -(h1 * (fq * fq) / (fe * fe)) - h2 * (Nt * Nt) / (F * F);
  const double Lbg = -(h1 * (fq * fc) / (fe * fe));
  const double Lgg = h1 * ((-2. * Nt) / fe - (fc * fc) / (fe * fe));
  const double b = coef[4 * r + 1], g = coef[4 * r + 2];
  const double *x = sums + (size_t) r * kCtfgSums;
  double *o = row + (size_t) r * kCtfgRow;
  o[0] = (double) p.amp;
  o[1] = (double) p.pha;
  o[2] = (double) p.env;
#pragma unroll
  for (int e = 0; e < kCtfgSums; e++)
    o[3 + e] = x[e];
  double st[3], ct[3];
#pragma unroll
  for (int e = 0; e < 3; e++)
  {
    st[e] = 2. * x[2 + e] / Nt;
    ct[e] = x[5 + e] / Nt;
    o[23 + e] = b * st[e] + g * ct[e];
  }
  // -prior with the signs of logpro_consts (CTF mode): -env^2 / 2 sB^2 + (pha - c_d)^2 / 2 sD^2 + (amp - c_a)^2 / 2 sA^2
  const double sA = (double) pd.sigmaPrioramp, sD = (double) pd.sigmaPriordefo, sB = (double) pd.sigmaPriorbctf;
  o[26] = (double) (p.amp - pd.Priorampcent) / sA / sA;
  o[27] = (double) (p.pha - pd.Priordefcent) / sD / sD;
  o[28] = -((double) p.env / sB / sB);
  int pair = 0;
#pragma unroll
  for (int e = 0; e < 3; e++)
#pragma unroll
    for (int f = e; f < 3; f++, pair++)
      o[29 + pair] = Lbb * (st[e] * st[f]) + Lbg * (st[e] * ct[f] + st[f] * ct[e]) + Lgg * (ct[e] * ct[f]) +
                     b * (2. * x[8 + pair] / Nt) + g * (x[14 + pair] / Nt);
  o[35] = 1. / sA / sA;
  o[36] = 1. / sD / sD;
  o[37] = -(1. / sB / sB);
}

} // namespace
#endif // BIOEM_CTFGRAD_TU

#endif
