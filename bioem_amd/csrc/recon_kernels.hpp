// recon_kernels.hpp -- the 3D density the aligned view sums support (bioem_hip_reconstruct, bioem_hip_debug_reconstruct;
// DESIGN 2.20).  With num_g, den_g [N][H] the normal-equation sums of view g (view_kernels.hpp), R_g the float matrix of
// its orientation (project_rotation.hpp) widened to double, o = (N + 1) / 2, M = (N - 1) / 2, tw[j] = exp(+2 pi i j / N):
//   S_g(a, b) = num_g[a mod N][b] tw[(o (a + b)) mod N] for b >= 0, conj(S_g(-a, -b)) for b < 0, 0 outside |a|, |b| <= M:
//               the slice about the pixel the projection puts the model's origin on; D_g likewise from den_g;
//   q_i       = (R[i][0] k0 + R[i][1] k1) + R[i][2] k2 for the stored voxel (k0, k1, k2), |k0|, |k1| <= N / 2, 0 <= k2 < H;
//   numV[k]  += wz w_t S_g(tap), denV[k] += wz w_t D_g(tap): wz = max(0, 1 - |q2|), the four taps (a, b), (a + 1, b),
//               (a, b + 1), (a + 1, b + 1) about a = floor(q0), b = floor(q1) with their bilinear weights, in that order,
//               the views in ascending g;
//   V^[k]     = numV / (denV + tau) tw[(-o (k0 + k1 + k2)) mod N], tau = wiener mean denV, 0 where the denominator is 0;
//   vol       = c2r3(V^) / N^3 [ / prod_d sinc^2(pi (x_d - o) / N) ], rounded to float.
// k_recon_insert is a gather: a lane owns a voxel and adds its views one after the other into registers.  No atomics
// and no cross-lane arithmetic: a voxel's bits depend on the views alone, not on the chunks they arrive in, the other
// voxels or the run.  The declarations are for every translation unit; the kernels are compiled by kernels_recon.hip
// only (BIOEM_RECON_TU).
#ifndef BIOEM_RECON_KERNELS_HPP
#define BIOEM_RECON_KERNELS_HPP

#include "engine_types.hpp"

const int kReconBrick = 4;      // a wave owns a brick of 4 x 4 x 4 voxels, k2 fastest on the lanes
const int kReconAxisOut = 8;    // outputs along axis 0 a lane of k_recon_axis0 carries
const int kReconTauBlocks = 64; // blocks of the first pass of the mean of denV

// R[i][9] (row major, double) of the n views whose orientation is angles[orient[i]] (orient null: angles[i])
BIOEM_HIDDEN hipError_t bioem_recon_matrices_launch(hipStream_t st, const float4 *angles, const int *orient, int isQuat, int n,
                                                    double *R);
// numV / denV [N][N][H] += the n views (slot[i] of num / den [.][N][H], matrix R[i]) in the order of the list; cull: views
// whose plane stays clear of a brick of voxels are left out for the whole brick (the same bits either way)
BIOEM_HIDDEN hipError_t bioem_recon_insert_launch(hipStream_t st, const double2 *num, const double *den, const int *slot,
                                                  const double *R, int n, int N, const double2 *tw, int cull, double2 *numV,
                                                  double *denV);
// tau[0] = wiener mean denV (part: kReconTauBlocks doubles of scratch), then numV becomes V^ in place
BIOEM_HIDDEN hipError_t bioem_recon_estimate_launch(hipStream_t st, double2 *numV, const double *denV, int N, double wiener,
                                                    const double2 *tw, double *part, double *tau);
// out[x0][k1][k2] = sum_k0 spec[k0][k1][k2] tw[(k0 x0) mod N]
BIOEM_HIDDEN hipError_t bioem_recon_axis0_launch(hipStream_t st, const double2 *spec, int N, const double2 *tw, double2 *out);
// vol[e] = (float) (map[e] / N [ / (sinc2[x0] sinc2[x1] sinc2[x2]) ]): map = [N] planes of c2r / N^2
BIOEM_HIDDEN hipError_t bioem_recon_correct_launch(hipStream_t st, const double *map, int N, const double *sinc2, int correct,
                                                   float *vol);

#ifdef BIOEM_RECON_TU
#include "project_rotation.hpp"

namespace
{

// grid (views / 64), one lane per view
__global__ __launch_bounds__(64) void k_recon_matrices(const float4 *__restrict__ angles, const int *__restrict__ orient,
                                                       int isQuat, int n, double *__restrict__ R)
{
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n)
    return;
  float rotmat[3][3];
  rotation_matrix(angles[orient ? orient[i] : i], isQuat, rotmat);
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++)
      R[9 * (size_t) i + 3 * r + c] = (double) rotmat[r][c];
}

// one tap of a view for one voxel: S and D at (a, b) times the weight c; every product and sum rounds once
__device__ inline void recon_tap(const double2 *__restrict__ num, const double *__restrict__ den,
                                 const double2 *__restrict__ tw, int a, int b, int N, int H, int M, int o, double c, double &nr,
                                 double &ni, double &dn)
{
  const bool inside = a >= -M && a <= M && b >= -M && b <= M;
  const bool neg = b < 0;
  int aa = neg ? -a : a, bb = neg ? -b : b;
  aa = inside ? aa : 0; // a safe place to read; the tap is dropped below
  bb = inside ? bb : 0;
  const int row = aa < 0 ? aa + N : aa;
  int s = aa + bb; // in [-M, 2 M]
  s = s < 0 ? s + N : s;
  const unsigned t = ((unsigned) o * (unsigned) s) % (unsigned) N;
  const size_t e = (size_t) row * H + bb;
  const double2 v = num[e], w = tw[t];
  const double d = den[e];
  if (inside)
  {
    const double sr = v.x * w.x - v.y * w.y;
    double si = v.x * w.y + v.y * w.x;
    si = neg ? -si : si;
    nr += c * sr;
    ni += c * si;
    dn += c * d;
  }
}

// Block = one wave = the brick (blockIdx.z, blockIdx.y, blockIdx.x) of kReconBrick^3 voxels of the [N][N][H] volume; lane
// l owns voxel (4 z + l / 16, 4 y + (l / 4) % 4, 4 x + l % 4).  The views go through in groups of 64.  With cull set, lane
// v of the wave first tests view v of the group against the whole brick: every voxel's q2 lies within 1.5 (|R20| + |R21| +
// |R22|) of the brick centre's, so beyond 1 + that reach (and a slack of 1e-6 against the rounding of the two sums, 1e-12
// at most) every lane has wz = 0 exactly.  The ballot of the survivors, about 3 / N of the views, is walked by a
// wave-uniform loop: a survivor's slot and matrix arrive by scalar loads, and only survivors pay the coordinates, the tap
// addresses and the twelve divergent loads.  A lane with wz = 0 adds nothing in either mode, so culling changes no
// bit.  A brick across the wrap of axis 0 or 1 (index N / 2 -> N / 2 + 1) has no single centre: it takes every view.
__global__ __launch_bounds__(64) void k_recon_insert(const double2 *__restrict__ num, const double *__restrict__ den,
                                                     const int *__restrict__ slot, const double *__restrict__ R, int n, int N,
                                                     int H, const double2 *__restrict__ tw, int cull,
                                                     double2 *__restrict__ numV, double *__restrict__ denV)
{
  const int l = threadIdx.x;
  const int b0 = kReconBrick * blockIdx.z, b1 = kReconBrick * blockIdx.y, b2 = kReconBrick * blockIdx.x;
  const int i0 = b0 + (l >> 4), i1 = b1 + ((l >> 2) & 3), k2 = b2 + (l & 3);
  const bool valid = i0 < N && i1 < N && k2 < H;
  const int M = (N - 1) / 2, o = (N + 1) / 2, half = N / 2;
  const double x0 = (double) (i0 <= half ? i0 : i0 - N), x1 = (double) (i1 <= half ? i1 : i1 - N), x2 = (double) k2;
  // the brick's centre in centred coordinates, where the brick does not span the wrap (indices beyond N - 1 own no voxel)
  const bool flat = (b0 > half || b0 + kReconBrick - 1 <= half) && (b1 > half || b1 + kReconBrick - 1 <= half);
  const double ext = 0.5 * (kReconBrick - 1);
  const double c0 = (double) (b0 <= half ? b0 : b0 - N) + ext, c1 = (double) (b1 <= half ? b1 : b1 - N) + ext;
  const double c2 = (double) b2 + ext;
  const double lim = (double) N;
  const size_t MH = (size_t) N * H;
  const size_t e = valid ? ((size_t) i0 * N + i1) * H + k2 : 0;
  double nr = 0., ni = 0., dn = 0.;
  if (valid)
  {
    const double2 v = numV[e];
    nr = v.x;
    ni = v.y;
    dn = denV[e];
  }
  for (int gb = 0; gb < n; gb += 64)
  {
    bool keep = gb + l < n;
    if (cull && flat && keep)
    {
      const double *Rv = R + 9 * (size_t) (gb + l);
      const double r0 = Rv[6], r1 = Rv[7], r2 = Rv[8];
      const double qc = (r0 * c0 + r1 * c1) + r2 * c2;
      const double reach = 1. + ext * ((fabs(r0) + fabs(r1)) + fabs(r2)) + 1e-6;
      keep = !(fabs(qc) >= reach); // (a NaN stays: the lanes below decide)
    }
    unsigned long long mask = __ballot(keep);
    while (mask)
    {
      const int g = gb + __ffsll((long long) mask) - 1; // wave-uniform
      mask &= mask - 1;
      const double *Rg = R + 9 * (size_t) g;
      const double q2 = (Rg[6] * x0 + Rg[7] * x1) + Rg[8] * x2;
      const double wz = fmax(0., 1. - fabs(q2)); // 0 for a NaN
      const double q0 = (Rg[0] * x0 + Rg[1] * x1) + Rg[2] * x2, q1 = (Rg[3] * x0 + Rg[4] * x1) + Rg[5] * x2;
      // beyond N pixels every tap lies outside the slice (and the conversion to int would overflow)
      if (valid && wz > 0. && fabs(q0) < lim && fabs(q1) < lim)
      {
        const double fa = floor(q0), fb = floor(q1);
        const double f0 = q0 - fa, f1 = q1 - fb, g0 = 1. - f0, g1 = 1. - f1;
        const int a = (int) fa, b = (int) fb;
        const double2 *ng = num + (size_t) slot[g] * MH;
        const double *dg = den + (size_t) slot[g] * MH;
        recon_tap(ng, dg, tw, a, b, N, H, M, o, wz * (g0 * g1), nr, ni, dn);
        recon_tap(ng, dg, tw, a + 1, b, N, H, M, o, wz * (f0 * g1), nr, ni, dn);
        recon_tap(ng, dg, tw, a, b + 1, N, H, M, o, wz * (g0 * f1), nr, ni, dn);
        recon_tap(ng, dg, tw, a + 1, b + 1, N, H, M, o, wz * (f0 * f1), nr, ni, dn);
      }
    }
  }
  if (valid)
  {
    numV[e] = make_double2(nr, ni);
    denV[e] = dn;
  }
}

// part[b] = the sum of the coefficients e = 256 (b + kReconTauBlocks j) + t, j = 0, 1, ...: lane t adds its own in that
// order, the block folds the 256 lane sums over the fixed tree of distances 128, 64, ... 1
__global__ __launch_bounds__(256) void k_recon_tau_part(const double *__restrict__ den, size_t n, double *__restrict__ part)
{
  __shared__ double red[256];
  double v = 0.;
  for (size_t e = 256 * (size_t) blockIdx.x + threadIdx.x; e < n; e += 256 * (size_t) kReconTauBlocks)
    v += den[e];
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = 128; s >= 1; s >>= 1)
  {
    if ((int) threadIdx.x < s)
      red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0)
    part[blockIdx.x] = red[0];
}

// tau = wiener * ((part[0] + part[1] + ...) / n): one lane, block order
__global__ __launch_bounds__(64) void k_recon_tau(const double *__restrict__ part, size_t n, double wiener,
                                                  double *__restrict__ tau)
{
  if (threadIdx.x != 0 || blockIdx.x != 0)
    return;
  double s = 0.;
  for (int b = 0; b < kReconTauBlocks; b++)
    s += part[b];
  tau[0] = wiener * (s / (double) n);
}

// V^ = numV / (denV + tau) tw[(-o (k0 + k1 + k2)) mod N] in place, 0 where the denominator is 0; grid (tiles of a plane, N)
__global__ __launch_bounds__(256) void k_recon_estimate(double2 *__restrict__ numV, const double *__restrict__ denV,
                                                        const double *__restrict__ tau, int N, int H,
                                                        const double2 *__restrict__ tw)
{
  const int c = blockIdx.x * 256 + threadIdx.x, i0 = blockIdx.y;
  if (c >= N * H)
    return;
  const int i1 = c / H, k2 = c - i1 * H;
  const size_t e = (size_t) i0 * N * H + c;
  const unsigned o = (unsigned) (N + 1) / 2, s = (unsigned) (i0 + i1 + k2) % (unsigned) N;
  const unsigned r = (o * s) % (unsigned) N;
  const double2 w = tw[r ? (unsigned) N - r : 0u];
  const double d = denV[e] + tau[0];
  const double2 v = numV[e];
  double2 out = make_double2(0., 0.);
  if (d != 0.)
  {
    const double qr = v.x / d, qi = v.y / d;
    out = make_double2(qr * w.x - qi * w.y, qr * w.y + qi * w.x);
  }
  numV[e] = out;
}

// The N-point inverse along axis 0 by direct summation: a lane owns column c = (k1, k2) and the kReconAxisOut outputs
// x0 = 8 blockIdx.y ... of it, and walks k0 upwards; the twiddle index (k0 x0) mod N is block-uniform (scalar loads),
// the loads of a plane's row coalesce.  grid (columns / 256, N / 8)
__global__ __launch_bounds__(256) void k_recon_axis0(const double2 *__restrict__ spec, int N, int H,
                                                     const double2 *__restrict__ tw, double2 *__restrict__ out)
{
  const int c = blockIdx.x * 256 + threadIdx.x;
  const int xb = kReconAxisOut * blockIdx.y;
  const size_t C = (size_t) N * H;
  if (c >= (int) C)
    return;
  double ar[kReconAxisOut], ai[kReconAxisOut];
  int idx[kReconAxisOut];
#pragma unroll
  for (int u = 0; u < kReconAxisOut; u++)
  {
    ar[u] = ai[u] = 0.;
    idx[u] = 0;
  }
  for (int k0 = 0; k0 < N; k0++)
  {
    const double2 x = spec[(size_t) k0 * C + c];
#pragma unroll
    for (int u = 0; u < kReconAxisOut; u++)
    {
      const double2 w = tw[idx[u]];
      ar[u] = fma(x.x, w.x, ar[u]);
      ar[u] = fma(-x.y, w.y, ar[u]);
      ai[u] = fma(x.y, w.x, ai[u]);
      ai[u] = fma(x.x, w.y, ai[u]);
      idx[u] += (xb + u) % N;
      if (idx[u] >= N)
        idx[u] -= N;
    }
  }
#pragma unroll
  for (int u = 0; u < kReconAxisOut; u++)
    if (xb + u < N)
      out[(size_t) (xb + u) * C + c] = make_double2(ar[u], ai[u]);
}

// grid (tiles of a plane, N): vol = map / N, divided by the transform of the tent where asked for, rounded to float
__global__ __launch_bounds__(256) void k_recon_correct(const double *__restrict__ map, int N, const double *__restrict__ sinc2,
                                                       int correct, float *__restrict__ vol)
{
  const int c = blockIdx.x * 256 + threadIdx.x, x0 = blockIdx.y;
  if (c >= N * N)
    return;
  const int x1 = c / N, x2 = c - x1 * N;
  const size_t e = (size_t) x0 * N * N + c;
  double v = map[e] / (double) N;
  if (correct)
    v = v / ((sinc2[x0] * sinc2[x1]) * sinc2[x2]);
  vol[e] = (float) v;
}

} // namespace
#endif // BIOEM_RECON_TU

#endif
