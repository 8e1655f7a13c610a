// vgrad_kernels.hpp -- the gradient of the log posterior of a request with respect to the voxels of a volume model
// (bioem_hip_volume_gradient, bioem_hip_debug_volume_backproject, bioem_hip_debug_volume_adjoint).  The
// conventions are those of slice_kernels.hpp: N, H, o, M, tw, the padding P, PN, PH, M_P, twP and R_g the float matrix of the
// orientation widened to double.  With G^_P [N][H] the gradient spectrum of a request (grad_kernels.hpp) and w_r its weight:
//   Gamma    = G^_P, but in the self-conjugate column b = 0: Gamma[a, 0] = (G^_P[a, 0] + conj G^_P[-a, 0]) / 2, the Hermitian
//              part that the c2r of k_grad_cols keeps;
//   Y[a, b]  = ((w_r w_b) / N^2) (Gamma[a, b] conj(tw[e(a, b)])), w_b = 1 for b = 0, else 2, e the twiddle index of
//              k_slice_project (the handle's shifts included); 0 outside a^2 + b^2 <= M^2 (k_vgrad_prepare; the debug entry
//              hands Gamma in and scales by w_r alone);
//   A[s]    += wt (neg ? conj Y[a, b] : Y[a, b]) for every request, coefficient and tap of k_slice_project that lands on the
//              stored voxel s of [PN][PN][PH]: the transpose of the slice, under every drop rule of the forward, wt its ((w0
//              w1) w2) from its own expressions for q, c, f, g (k_vgrad_insert).  dL = sum_s Re(conj(A[s]) dC[s]);
//   A_spec[k]= (((A[k] conj(twP[r])) conj(e0)) conj(e1)) conj(e2), the factors of k_slice_centre (k_vgrad_uncentre);
//   gv[x]    = sum_{stored k} Re(A_spec[k] twP[(k.x) mod PN]), x in the N^3 box, the stored entries as they are: three passes
//              of direct summation, axis 0, axis 1, axis 2 (k_vgrad_axis), a lane owns one output and adds its terms in
//              ascending k with fma;
//   gvol[x]  = gv[x] [ / ((sinc2[x0] sinc2[x1]) sinc2[x2]) ] (k_vgrad_finish).
// k_vgrad_insert is a gather: a lane owns a stored voxel and finds, per view, the coefficients whose taps land on it.  For
// a target tau (the voxel s, and -s conjugated where s2 > 0: a tap with a negative third index reads conj C(-k)) the
// coefficients (a, b) with a tap on tau satisfy |P (a R0 + b R1) - tau|_inf <= 1, so with (a*, b*) the least-squares
// solution and G the Gram matrix of rows 0 and 1 of R: |a - a*| <= sqrt(3) sqrt((G^-1)_00) / P, |b - b*| likewise with
// (G^-1)_11.  k_vgrad_views forms G^-1 / P, the two half-widths (widened by 2^-20 relative and absolute against the rounding
// of q, 1e-12 at most) and the unit normal of the plane once per view; a view whose half-width exceeds kVgradHalfCap or
// whose rows 0 and 1 are (nearly) parallel is flagged, and the entries refuse it.  Every candidate is then tested with the
// forward's own q: it counts iff tau - floor(q) is in {0, 1}^3 and the forward counts that tap.  Order within a voxel:
// views ascending, target +s before -s, candidates in ascending (a, b).  No atomics and no cross-lane arithmetic: a voxel's
// bits depend on the views in their order alone, not on the chunks they arrive in, the cull, the other voxels or the run.
// The declarations are for every translation unit; the kernels are compiled by kernels_vgrad.hip only (BIOEM_VGRAD_TU).
#ifndef BIOEM_VGRAD_KERNELS_HPP
#define BIOEM_VGRAD_KERNELS_HPP

#include "engine_types.hpp"

const int kVgradBrick = 4; // a wave owns a brick of 4 x 4 x 4 stored voxels, k2 fastest on the lanes
// The widest half-width served.  A rotation has sqrt(3) / P: 1.74 at pad 1.  The matrix of a quaternion that is not of
// unit length, 1 - 2 (y^2 + z^2) ... (project_rotation.hpp), is no multiple of a rotation: it shrinks unevenly, is singular
// at length sqrt(1 / 2), and the half-width grows without bound towards that length, so every cap refuses a neighbourhood
// of it.  4 serves the lengths from 0.85 (at most 3.9 at pad 1 over 2 000 random axes) through 1.07 (1.74) and beyond, far
// outside the norm deviations the orientation grids carry, at no more than 9 x 9 candidates per target and view.
#define BIOEM_VGRAD_HALF_CAP 4.0
const double kVgradHalfCap = BIOEM_VGRAD_HALF_CAP;
const int kVgradViewDoubles = 8; // per view: (G^-1)_00 / P, _01 / P, _11 / P, half-width a, half-width b, the unit normal

// view[i][8] and flag[i] (0: served, 1: rows 0 and 1 of the matrix rank-deficient or not finite, 2: half-width beyond the
// cap) of the n matrices R[i][9]
BIOEM_HIDDEN hipError_t bioem_vgrad_views_launch(hipStream_t st, const double *R, int n, int pad, double *view, int *flag);
// Y[n][N][H] from spec[n][N][H]; w[n] (null: 1); full: the symmetrisation, w_b and 1 / N^2 (else w alone)
BIOEM_HIDDEN hipError_t bioem_vgrad_prepare_launch(hipStream_t st, const double2 *spec, const double *w, int n, int N,
                                                   const double2 *tw, int shiftX, int shiftY, int full, double2 *Y);
// A [PN][PN][PH] += the n views (Y[i], R[i], view[i]) in the order of the list; first: A starts from 0 instead of what the
// buffer holds; cull: views whose plane stays clear of a brick are left out for the whole brick (the same bits either way)
BIOEM_HIDDEN hipError_t bioem_vgrad_insert_launch(hipStream_t st, const double2 *Y, const double *R, const double *view, int n,
                                                  int N, int pad, int cull, int first, double2 *A);
// dot[i] = sum over the disc of (w_b / N^2) Re(conj(Gamma_i) slice_i), Gamma from spec as k_vgrad_prepare forms it
BIOEM_HIDDEN hipError_t bioem_vgrad_dot_launch(hipStream_t st, const double2 *spec, const double2 *slices, int n, int N,
                                               double *dot, int dotStride);
// A becomes A_spec in place; e: the three tables e0, e1, e2 of PN entries each, as bioem_slice_centre_launch takes them
BIOEM_HIDDEN hipError_t bioem_vgrad_uncentre_launch(hipStream_t st, double2 *A, int PN, int o, const double2 *twP,
                                                    const double2 *e);
// out[o][x][c] = sum_k in[o][k][c] twP[(k x) mod PN], k = 0 ... nIn - 1 ascending, x = 0 ... nOut - 1
BIOEM_HIDDEN hipError_t bioem_vgrad_axis_launch(hipStream_t st, const double2 *in, size_t outer, int nIn, int nOut,
                                                size_t inner, int PN, const double2 *twP, double2 *out);
// gvol[x] = Re(in[x]) [ / ((sinc2[x0] sinc2[x1]) sinc2[x2]) ], [N][N][N]
BIOEM_HIDDEN hipError_t bioem_vgrad_finish_launch(hipStream_t st, const double2 *in, int N, const double *sinc2, int correct,
                                                  double *gvol);

#ifdef BIOEM_VGRAD_TU

namespace
{

// grid (views / 64), one lane per view
__global__ __launch_bounds__(64) void k_vgrad_views(const double *__restrict__ R, int n, double dp,
                                                    double *__restrict__ view, int *__restrict__ flag)
{
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n)
    return;
  const double *Rv = R + 9 * (size_t) i;
  const double a0 = Rv[0], a1 = Rv[1], a2 = Rv[2], b0 = Rv[3], b1 = Rv[4], b2 = Rv[5];
  const double g00 = (a0 * a0 + a1 * a1) + a2 * a2, g01 = (a0 * b0 + a1 * b1) + a2 * b2, g11 = (b0 * b0 + b1 * b1) + b2 * b2;
  const double det = g00 * g11 - g01 * g01; // |R0 x R1|^2
  int f = 0;
  // (sin^2 of the angle between the rows at most 1e-6, a row of length 0, or anything not finite)
  if (!(g00 > 0.) || !(g11 > 0.) || !(det > 1e-6 * (g00 * g11)) || !(det < 1e300))
    f = 1;
  const double i00 = g11 / det, i01 = -g01 / det, i11 = g00 / det;
  const double s3 = 1.7320508075688772;
  const double slack = 1. / 1048576.;
  const double ha = (s3 * sqrt(i00) / dp) * (1. + slack) + slack, hb = (s3 * sqrt(i11) / dp) * (1. + slack) + slack;
  if (!f && !(ha <= kVgradHalfCap && hb <= kVgradHalfCap))
    f = 2;
  const double n0 = a1 * b2 - a2 * b1, n1 = a2 * b0 - a0 * b2, n2 = a0 * b1 - a1 * b0;
  const double nl = sqrt((n0 * n0 + n1 * n1) + n2 * n2);
  double *v = view + kVgradViewDoubles * (size_t) i;
  v[0] = i00 / dp;
  v[1] = i01 / dp;
  v[2] = i11 / dp;
  v[3] = ha;
  v[4] = hb;
  v[5] = n0 / nl;
  v[6] = n1 / nl;
  v[7] = n2 / nl;
  flag[i] = f;
}

// the twiddle index of k_slice_project: (-o (a + b) + shiftX a + shiftY b) mod N, every product reduced in 32 bits
__device__ inline int vgrad_twiddle_index(int a, int b, int N, int o, int shiftX, int shiftY)
{
  int e = (-((o * (a + b)) % N) + ((shiftX % N) * a) % N + ((shiftY % N) * b) % N) % N;
  return e < 0 ? e + N : e;
}

// Gamma of the stored coefficient (ia, b) of a spectrum S [N][H]
__device__ inline double2 vgrad_gamma(const double2 *__restrict__ S, int ia, int b, int N, int H)
{
  const double2 v = S[(size_t) ia * H + b];
  if (b != 0)
    return v;
  const double2 m = S[(size_t) (ia ? N - ia : 0) * H];
  return make_double2((v.x + m.x) * 0.5, (v.y - m.y) * 0.5);
}

// grid (coefficients / 256, views): a lane owns its coefficient; the weight of the view is block-uniform (a scalar load)
__global__ __launch_bounds__(256) void k_vgrad_prepare(const double2 *__restrict__ spec, const double *__restrict__ w, int N,
                                                       int H, const double2 *__restrict__ tw, int shiftX, int shiftY, int full,
                                                       double2 *__restrict__ Y)
{
  const int g = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
  if (c >= N * H)
    return;
  const int ia = c / H, b = c - ia * H;
  const int M = (N - 1) / 2, o = (N + 1) / 2;
  const int a = ia <= N / 2 ? ia : ia - N;
  const size_t at = (size_t) g * N * H + c;
  if (a * a + b * b > M * M)
  {
    Y[at] = make_double2(0., 0.);
    return;
  }
  const double2 *S = spec + (size_t) g * N * H;
  const double2 v = full ? vgrad_gamma(S, ia, b, N, H) : S[c];
  const double2 t = tw[vgrad_twiddle_index(a, b, N, o, shiftX, shiftY)];
  const double wr = w ? w[g] : 1.;
  const double sc = full ? (wr * (b == 0 ? 1. : 2.)) / ((double) N * (double) N) : wr;
  // v conj(t)
  const double zr = v.x * t.x + v.y * t.y, zi = v.y * t.x - v.x * t.y;
  Y[at] = make_double2(sc * zr, sc * zi);
}

// Block = one wave = the brick (blockIdx.z, blockIdx.y, blockIdx.x) of kVgradBrick^3 stored voxels of [PN][PN][PH]; lane l
// owns voxel (4 z + l / 16, 4 y + (l / 4) % 4, 4 x + l % 4) and carries its A in registers over the views of the launch.
// The views go through in groups of 64.  With cull set, lane v of the wave first tests view v of the group against the
// whole brick: a voxel with a tap of the view lies within sqrt(3) of the view's plane (the coefficient's point is within 1
// of it on every axis), every voxel of the brick within 1.5 (|n0| + |n1| + |n2|) of the brick centre's distance, and the
// mirror image -s of the brick lies as far from the plane as the brick itself (the plane holds the origin): beyond that
// reach, and a slack of 1e-6 against the rounding of q (1e-12 at most), no lane has a tap in either target.  The ballot
// of the survivors is walked by a wave-uniform loop: a survivor's matrix, G^-1 and half-widths arrive by scalar loads, the
// candidate counts are wave-uniform, and a candidate that does not count is selected away, not branched around.  A brick
// across the wrap of axis 0 or 1 has no single centre: it takes every view.
__global__ __launch_bounds__(64) void k_vgrad_insert(const double2 *__restrict__ Y, const double *__restrict__ R,
                                                     const double *__restrict__ view, int n, int N, int H, int pad, int PN,
                                                     int PH, int MP, int cull, int first, double2 *__restrict__ A)
{
  const int l = threadIdx.x;
  const int b0 = kVgradBrick * blockIdx.z, b1 = kVgradBrick * blockIdx.y, b2 = kVgradBrick * blockIdx.x;
  const int i0 = b0 + (l >> 4), i1 = b1 + ((l >> 2) & 3), k2 = b2 + (l & 3);
  const bool valid = i0 < PN && i1 < PN && k2 < PH;
  const int M = (N - 1) / 2, half = PN / 2;
  const int s0 = i0 <= half ? i0 : i0 - PN, s1 = i1 <= half ? i1 : i1 - PN;
  // a voxel the forward can reach (for an even PN the index PN / 2 lies beyond M_P: it stays 0)
  const bool reach = valid && s0 >= -MP && s0 <= MP && s1 >= -MP && s1 <= MP && k2 <= MP;
  const bool flat = (b0 > half || b0 + kVgradBrick - 1 <= half) && (b1 > half || b1 + kVgradBrick - 1 <= half);
  const double ext = 0.5 * (kVgradBrick - 1);
  const double c0 = (double) (b0 <= half ? b0 : b0 - PN) + ext, c1 = (double) (b1 <= half ? b1 : b1 - PN) + ext;
  const double c2 = (double) b2 + ext;
  const double dp = (double) pad, lim = (double) PN;
  const size_t MH = (size_t) N * H;
  const size_t e = valid ? ((size_t) i0 * PN + i1) * PH + k2 : 0;
  double ar = 0., ai = 0.;
  if (valid && !first)
  {
    const double2 v = A[e];
    ar = v.x;
    ai = v.y;
  }
  for (int gb = 0; gb < n; gb += 64)
  {
    bool keep = gb + l < n;
    if (cull && flat && keep)
    {
      const double *V = view + kVgradViewDoubles * (size_t) (gb + l);
      const double n0 = V[5], n1 = V[6], n2 = V[7];
      const double dc = (n0 * c0 + n1 * c1) + n2 * c2;
      const double far = 1.7320508075688772 + ext * ((fabs(n0) + fabs(n1)) + fabs(n2)) + 1e-6;
      keep = !(fabs(dc) >= far); // (a NaN stays: the lanes below decide)
    }
    unsigned long long mask = __ballot(keep);
    while (mask)
    {
      const int g = gb + __ffsll((long long) mask) - 1; // wave-uniform
      mask &= mask - 1;
      const double *Rg = R + 9 * (size_t) g;
      const double *V = view + kVgradViewDoubles * (size_t) g;
      const double r00 = Rg[0], r01 = Rg[1], r02 = Rg[2], r10 = Rg[3], r11 = Rg[4], r12 = Rg[5];
      const double m00 = V[0], m01 = V[1], m11 = V[2], ha = V[3], hb = V[4];
      // the integers of an interval of length 2 h: at most floor(2 h) + 1 (h <= kVgradHalfCap: the entries see to it)
      const int Wa = (int) fmin(2. * ha, 2. * kVgradHalfCap) + 1, Wb = (int) fmin(2. * hb, 2. * kVgradHalfCap) + 1;
      const double2 *Yg = Y + (size_t) g * MH;
      for (int sg = 0; sg < 2; sg++) // the target +s, then -s conjugated
      {
        const bool act = reach && (sg == 0 || k2 > 0);
        const double t0 = (double) (sg ? -s0 : s0), t1 = (double) (sg ? -s1 : s1), t2 = (double) (sg ? -k2 : k2);
        const double p0 = (r00 * t0 + r01 * t1) + r02 * t2, p1 = (r10 * t0 + r11 * t1) + r12 * t2;
        const double as = m00 * p0 + m01 * p1, bs = m01 * p0 + m11 * p1;
        // (finite and far inside the range of int: |a*| <= sqrt(3) M_P times the half-width)
        const int aFirst = (int) ceil(as - ha), bFirst = (int) ceil(bs - hb);
        for (int ja = 0; ja < Wa; ja++)
        {
          const int a = aFirst + ja;
          const double da = (double) a;
          for (int jb = 0; jb < Wb; jb++)
          {
            const int b = bFirst + jb;
            const double db = (double) b;
            bool ok = act && b >= 0 && a >= -M && a <= M && b <= M && a * a + b * b <= M * M;
            // the forward's expressions
            const double q0 = dp * ((da * r00) + (db * r10)), q1 = dp * ((da * r01) + (db * r11)),
                         q2 = dp * ((da * r02) + (db * r12));
            ok = ok && fabs(q0) < lim && fabs(q1) < lim && fabs(q2) < lim;
            const double f0 = q0 - floor(q0), f1 = q1 - floor(q1), f2 = q2 - floor(q2);
            const double g0 = 1. - f0, g1 = 1. - f1, g2 = 1. - f2;
            const double d0 = t0 - floor(q0), d1 = t1 - floor(q1), d2 = t2 - floor(q2);
            ok = ok && (d0 == 0. || d0 == 1.) && (d1 == 0. || d1 == 1.) && (d2 == 0. || d2 == 1.);
            const double wt = ((d0 == 1. ? f0 : g0) * (d1 == 1. ? f1 : g1)) * (d2 == 1. ? f2 : g2);
            const int row = a < 0 ? a + N : a;
            const double2 y = Yg[ok ? (size_t) row * H + b : 0];
            const double tr = ar + wt * y.x, ti = ai + wt * (sg ? -y.y : y.y);
            ar = ok ? tr : ar;
            ai = ok ? ti : ai;
          }
        }
      }
    }
  }
  if (valid)
    A[e] = make_double2(ar, ai);
}

// grid (views): lane t adds the coefficients c = t, t + 256, ... of its view in that order, the block folds the 256 lane
// sums over the fixed tree of distances 128, 64, ... 1
__global__ __launch_bounds__(256) void k_vgrad_dot(const double2 *__restrict__ spec, const double2 *__restrict__ slices,
                                                   int N, int H, double *__restrict__ dot, int dotStride)
{
  __shared__ double red[256];
  const int g = blockIdx.x;
  const int M = (N - 1) / 2;
  const double2 *S = spec + (size_t) g * N * H, *X = slices + (size_t) g * N * H;
  const double Nt = (double) N * (double) N;
  double v = 0.;
  for (int c = threadIdx.x; c < N * H; c += 256)
  {
    const int ia = c / H, b = c - ia * H;
    const int a = ia <= N / 2 ? ia : ia - N;
    if (a * a + b * b > M * M)
      continue;
    const double2 G = vgrad_gamma(S, ia, b, N, H), x = X[c];
    v += ((b == 0 ? 1. : 2.) / Nt) * (G.x * x.x + G.y * x.y);
  }
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = 128; s >= 1; s >>= 1)
  {
    if ((int) threadIdx.x < s)
      red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0)
    dot[(size_t) g * dotStride] = red[0];
}

// grid (tiles of a plane, PN): stored (i0, i1, k2), the factors of k_slice_centre conjugated, in its order
__global__ __launch_bounds__(256) void k_vgrad_uncentre(double2 *__restrict__ A, int PN, int PH, int o,
                                                        const double2 *__restrict__ twP, const double2 *__restrict__ e)
{
  const int c = blockIdx.x * 256 + threadIdx.x, i0 = blockIdx.y;
  if (c >= PN * PH)
    return;
  const int i1 = c / PH, k2 = c - i1 * PH;
  const int half = PN / 2;
  const int k0 = i0 <= half ? i0 : i0 - PN, k1 = i1 <= half ? i1 : i1 - PN;
  int s = (k0 + k1 + k2) % PN; // in (-PN, PN)
  s = s < 0 ? s + PN : s;
  const unsigned r = ((unsigned) o * (unsigned) s) % (unsigned) PN;
  const size_t at = (size_t) i0 * PN * PH + c;
  double2 v = A[at];
  const double2 w[4] = {twP[r], e[i0], e[PN + i1], e[2 * PN + k2]};
#pragma unroll
  for (int j = 0; j < 4; j++)
    v = make_double2(v.x * w[j].x + v.y * w[j].y, v.y * w[j].x - v.x * w[j].y);
  A[at] = v;
}

// grid (outputs / 256): output t = (o nOut + x) inner + c
__global__ __launch_bounds__(256) void k_vgrad_axis(const double2 *__restrict__ in, size_t outer, int nIn, int nOut,
                                                    size_t inner, int PN, const double2 *__restrict__ twP,
                                                    double2 *__restrict__ out)
{
  const size_t t = (size_t) blockIdx.x * 256 + threadIdx.x;
  if (t >= outer * (size_t) nOut * inner)
    return;
  const size_t c = t % inner, ox = t / inner;
  const int x = (int) (ox % (size_t) nOut);
  const size_t o = ox / (size_t) nOut;
  const double2 *src = in + o * (size_t) nIn * inner + c;
  const int step = x % PN;
  int idx = 0;
  double ar = 0., ai = 0.;
  for (int k = 0; k < nIn; k++)
  {
    const double2 v = src[(size_t) k * inner], w = twP[idx];
    // v w
    ar = fma(v.x, w.x, ar);
    ar = fma(-v.y, w.y, ar);
    ai = fma(v.y, w.x, ai);
    ai = fma(v.x, w.y, ai);
    idx += step;
    if (idx >= PN)
      idx -= PN;
  }
  out[t] = make_double2(ar, ai);
}

// grid (tiles of a plane, N)
__global__ __launch_bounds__(256) void k_vgrad_finish(const double2 *__restrict__ in, int N, const double *__restrict__ sinc2,
                                                      int correct, double *__restrict__ gvol)
{
  const int c = blockIdx.x * 256 + threadIdx.x, x0 = blockIdx.y;
  if (c >= N * N)
    return;
  const int x1 = c / N, x2 = c - x1 * N;
  const size_t e = (size_t) x0 * N * N + c;
  double v = in[e].x;
  if (correct)
    v = v / ((sinc2[x0] * sinc2[x1]) * sinc2[x2]);
  gvol[e] = v;
}

} // namespace
#endif // BIOEM_VGRAD_TU

#endif
