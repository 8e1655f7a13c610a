// pose_kernels.hpp -- the gradient of the log posterior of a request with respect to the orientation matrix of a volume model
// and to the handle's model shifts (bioem_hip_pose_gradient, bioem_hip_debug_pose_sums).  The conventions are
// those of slice_kernels.hpp and vgrad_kernels.hpp: N, H, o, M, the padding P, PN, PH, M_P, C the centred spectrum, R the
// float matrix of the orientation widened to double, and Y [N][H] of a request as k_vgrad_prepare forms it (0 outside the
// disc).  Per stored coefficient (a, b) of the disc a^2 + b^2 <= M^2 with |q_d| < PN, in the forward's own expressions,
// unfused: q_d = P ((a R[0][d]) + (b R[1][d])), c_d = floor(q_d), f_d = q_d - c_d, g_d = 1 - f_d, w_d(t) = d_d ? f_d : g_d over
// the taps t = 4 d0 + 2 d1 + d2 = 0 ... 7, v_t = C(c + d) (conjugated where the third index is negative; a tap outside
// |index_d| <= M_P is selected away).  From 0 + 0i, in ascending t, re and im apart:
//   s    = s + ((w0 w1) w2) v_t               the forward's tap sum before the de-centring twiddle, its bits
//   D_0  = D_0 + (sigma_0(t) (w1 w2)) v_t     sigma_d(t) = +1 where d_d = 1, else -1 (the sign goes onto the weight: exact)
//   D_1  = D_1 + (sigma_1(t) (w0 w2)) v_t
//   D_2  = D_2 + (sigma_2(t) (w0 w1)) v_t
// the gradient of the trilinear interpolant in the cell that floor selects (at f_d = 0 the right-hand derivative).  Then the
// nine terms of the lane, x_0 = a, x_1 = b:
//   J[i][j] = (P x_i) ((Y.re D_j.re) + (Y.im D_j.im))            sums 3 i + j = 0 ... 5
//   T[i]    = (((2 pi) / N) x_i) ((Y.im s.re) - (Y.re s.im))      sums 6, 7: (2 pi x_i / N) Re(conj(Y) i s)
//   dot     = (Y.re s.re) + (Y.im s.im)                           sum 8: Re(conj(Y) s)
// A lane without a coefficient, with one outside the disc or with a coordinate not below PN has the term +0.0.
// k_pose_partials: block = patch of kSlicePatchA x kSlicePatchB coefficients (the patches of k_slice_project, lane l owns
// stored row A pa + l / B and column B pb + l % B) of one request.  Each of the nine terms is folded over the 64 lanes of a
// wave by the tree of distances 32, 16, 8, 4, 2, 1 (x[l] = x[l] + x[l ^ d]: both partners form the same sum), then over the
// four waves as (w0 + w1) + (w2 + w3): partial[request][patch][9].
// k_pose_fold: one lane per (request, sum) adds the patches in ascending order from +0.0 and writes row[request][18] = the
// nine sums, then the nine doubles of R.
// No atomics; a row's bits depend on its request alone, not on the batch, its place in it, the other requests or the run.
// The declarations are for every translation unit; the kernels are compiled by kernels_pose.hip only (BIOEM_POSE_TU).
#ifndef BIOEM_POSE_KERNELS_HPP
#define BIOEM_POSE_KERNELS_HPP

#include "engine_types.hpp"
#include "slice_kernels.hpp" // (the patch shape)

const int kPoseSums = 9;  // J[2][3], T[2], dot
const int kPoseRow = 18;  // the sums, then R[9]

// patches of a request: ceil(N / kSlicePatchA) ceil(H / kSlicePatchB)
BIOEM_HIDDEN int bioem_pose_patches(int N);
// row[i][18] of the n requests (Y[i] [N][H], R[i][9]); partial: n bioem_pose_patches(N) 9 doubles of staging
BIOEM_HIDDEN hipError_t bioem_pose_launch(hipStream_t st, const double2 *C, int pad, const double *R, const double2 *Y, int n,
                                          int N, double *partial, double *row);

#ifdef BIOEM_POSE_TU

namespace
{

// one tap, as slice_tap of slice_kernels.hpp: where it reads, whether it counts and whether it is conjugated.  The address
// is formed from indices that were checked: an outside tap reads element 0 and is dropped
__device__ inline size_t pose_tap(int k0, int k1, int k2, int PN, int PH, int MP, bool &inside, bool &neg)
{
  inside = k0 >= -MP && k0 <= MP && k1 >= -MP && k1 <= MP && k2 >= -MP && k2 <= MP;
  neg = k2 < 0;
  k0 = neg ? -k0 : k0;
  k1 = neg ? -k1 : k1;
  k2 = neg ? -k2 : k2;
  k0 = inside ? k0 : 0;
  k1 = inside ? k1 : 0;
  k2 = inside ? k2 : 0;
  const int r0 = k0 < 0 ? k0 + PN : k0, r1 = k1 < 0 ? k1 + PN : k1;
  return ((size_t) r0 * PN + r1) * PH + k2;
}

__global__ __launch_bounds__(256) void k_pose_partials(const double2 *__restrict__ C, int pad, int PN, int PH, int MP,
                                                       const double *__restrict__ R, const double2 *__restrict__ Y, int N,
                                                       int H, int patchesB, double *__restrict__ partial)
{
  __shared__ double red[4][kPoseSums];
  const int g = blockIdx.y;
  const int pa = blockIdx.x / patchesB, pb = blockIdx.x - pa * patchesB;
  const int ia = kSlicePatchA * pa + (int) threadIdx.x / kSlicePatchB, b = kSlicePatchB * pb + (int) threadIdx.x % kSlicePatchB;
  const int M = (N - 1) / 2;
  const int a = ia <= N / 2 ? ia : ia - N;
  const bool have = ia < N && b < H && a * a + b * b <= M * M;
  const double *Rg = R + 9 * (size_t) g;
  const double da = (double) a, db = (double) b, dp = (double) pad, lim = (double) PN;
  const double q0 = dp * ((da * Rg[0]) + (db * Rg[3])), q1 = dp * ((da * Rg[1]) + (db * Rg[4])),
               q2 = dp * ((da * Rg[2]) + (db * Rg[5]));
  const bool ok = have && fabs(q0) < lim && fabs(q1) < lim && fabs(q2) < lim; // (false for a NaN)
  const double c0 = ok ? floor(q0) : 0., c1 = ok ? floor(q1) : 0., c2 = ok ? floor(q2) : 0.;
  const double f0 = q0 - c0, f1 = q1 - c1, f2 = q2 - c2, g0 = 1. - f0, g1 = 1. - f1, g2 = 1. - f2;
  const int i0 = (int) c0, i1 = (int) c1, i2 = (int) c2;
  double2 v[8];
  bool inside[8], neg[8];
  const double2 y = Y[have ? ((size_t) g * N + ia) * H + b : 0];
#pragma unroll
  for (int t = 0; t < 8; t++)
    v[t] = C[pose_tap(i0 + (t >> 2), i1 + ((t >> 1) & 1), i2 + (t & 1), PN, PH, MP, inside[t], neg[t])];
  __builtin_amdgcn_sched_barrier(0); // (the nine loads are in flight before the first is consumed)
  double sr = 0., si = 0., dr[3] = {0., 0., 0.}, di[3] = {0., 0., 0.};
#pragma unroll
  for (int t = 0; t < 8; t++)
  {
    const bool d0 = t >> 2, d1 = (t >> 1) & 1, d2 = t & 1;
    const double w0 = d0 ? f0 : g0, w1 = d1 ? f1 : g1, w2 = d2 ? f2 : g2;
    const double vr = v[t].x, vi = neg[t] ? -v[t].y : v[t].y;
    const double w01 = w0 * w1, w12 = w1 * w2, w02 = w0 * w2;
    const double wt[4] = {w01 * w2, d0 ? w12 : -w12, d1 ? w02 : -w02, d2 ? w01 : -w01};
    const double tr = sr + wt[0] * vr, ti = si + wt[0] * vi;
    sr = inside[t] ? tr : sr;
    si = inside[t] ? ti : si;
#pragma unroll
    for (int j = 0; j < 3; j++)
    {
      const double ur = dr[j] + wt[j + 1] * vr, ui = di[j] + wt[j + 1] * vi;
      dr[j] = inside[t] ? ur : dr[j];
      di[j] = inside[t] ? ui : di[j];
    }
  }
  const double xa = dp * da, xb = dp * db;
  const double k = (2. * 3.14159265358979323846) / (double) N;
  const double ta = k * da, tb = k * db;
  double x[kPoseSums];
#pragma unroll
  for (int j = 0; j < 3; j++)
  {
    const double c = (y.x * dr[j]) + (y.y * di[j]);
    x[j] = xa * c;
    x[3 + j] = xb * c;
  }
  const double ts = (y.y * sr) - (y.x * si);
  x[6] = ta * ts;
  x[7] = tb * ts;
  x[8] = (y.x * sr) + (y.y * si);
#pragma unroll
  for (int j = 0; j < kPoseSums; j++)
  {
    double z = ok ? x[j] : 0.;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1)
      z = z + __shfl_xor(z, d, 64);
    x[j] = z;
  }
  if ((threadIdx.x & 63) == 0)
  {
#pragma unroll
    for (int j = 0; j < kPoseSums; j++)
      red[threadIdx.x >> 6][j] = x[j];
  }
  __syncthreads();
  if (threadIdx.x < kPoseSums)
  {
    const int j = threadIdx.x;
    partial[((size_t) g * gridDim.x + blockIdx.x) * kPoseSums + j] = (red[0][j] + red[1][j]) + (red[2][j] + red[3][j]);
  }
}

// grid (ceil(9 n / 64)): lane (request, sum)
__global__ __launch_bounds__(64) void k_pose_fold(const double *__restrict__ partial, const double *__restrict__ R, int n,
                                                  int patches, double *__restrict__ row)
{
  const int t = blockIdx.x * 64 + threadIdx.x;
  if (t >= kPoseSums * n)
    return;
  const int g = t / kPoseSums, j = t - g * kPoseSums;
  const double *p = partial + (size_t) g * patches * kPoseSums + j;
  double z = 0.;
  for (int i = 0; i < patches; i++)
    z = z + p[(size_t) i * kPoseSums];
  row[(size_t) g * kPoseRow + j] = z;
  row[(size_t) g * kPoseRow + kPoseSums + j] = R[9 * (size_t) g + j];
}

} // namespace
#endif // BIOEM_POSE_TU

#endif
