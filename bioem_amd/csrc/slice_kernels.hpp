// slice_kernels.hpp -- a volume as the model: projections as central slices of its spectrum (bioem_hip_upload_model_volume,
// bioem_hip_upload_model_spectrum, bioem_hip_debug_slices, the volume branch of project_batch).  With N, H =
// N / 2 + 1, o = (N + 1) / 2, M = (N - 1) / 2, tw[j] = exp(+2 pi i j / N) as in recon_kernels.hpp, the padding P in {1, 2},
// PN = P N, PH = PN / 2 + 1, M_P = (PN - 1) / 2, twP[j] = exp(+2 pi i j / PN), and R the float matrix of the orientation
// (project_rotation.hpp) widened to double (k_recon_matrices):
//   spec[k]  = sum_x vol[x] exp(-2 pi i k.x / PN) over the N^3 box in the first octant of the PN^3 box: three passes of
//              direct summation (k_slice_axis: axis 2, axis 1, axis 0), a lane owns one output and adds its N terms in
//              ascending x with fma, the twiddle index (k x) mod PN reduced in integers;
//   C(k')    = (((spec[k' mod PN] twP[(o (k'0 + k'1 + k'2)) mod PN]) e0[k'0]) e1[k'1]) e2[k'2], e_d[k] = exp(+2 pi i k
//              centre_d / PN) from the host's tables: the spectrum about the origin voxel (o, o, o), the density moved by
//              -centre; stored [PN][PN][PH] with wrapped indices on axes 0 and 1 (k_slice_centre);
//   slice    : stored coefficient (a mod N, b), |a| <= N / 2, 0 <= b < H, of orientation g:
//              0 + 0i where a^2 + b^2 > M^2 (written), else with k_j = (a R[0][j]) + (b R[1][j]), k' = P k, c_d =
//              floor(k'_d), f_d = k'_d - c_d, g_d = 1 - f_d the sum over the taps t = 4 d0 + 2 d1 + d2 = 0 ... 7 in
//              ascending t of ((w0 w1) w2) C(c + d), w_d = d_d ? f_d : g_d; a tap whose third index is negative reads
//              conj C(-(c + d)); a tap outside |index_d| <= M_P adds nothing, nor does any tap where a coordinate is
//              not below PN in magnitude (a NaN included); the sum times tw[(-o (a + b) + shiftX a + shiftY b) mod N],
//              rounded once to float2 (the run) or kept in double (bioem_hip_debug_slices).
// k_slice_project is a gather: a lane owns its coefficient.  No atomics and no cross-lane arithmetic: a coefficient's
// bits depend on its orientation alone.  The declarations are for every translation unit; the kernels are compiled by
// kernels_slice.hip only (BIOEM_SLICE_TU).
#ifndef BIOEM_SLICE_KERNELS_HPP
#define BIOEM_SLICE_KERNELS_HPP

#include "engine_types.hpp"

// a block of 256 lanes owns a patch of kSlicePatchA rows x kSlicePatchB columns of coefficients (a, b) of one
// orientation, b fastest (the shape is settled by measurement: DESIGN 2.24)
const int kSlicePatchA = 32, kSlicePatchB = 8;

// out[o][k][c] = sum_x in[o][x][c] conj(twP[(k x) mod PN]), x = 0 ... nIn - 1 ascending, k = 0 ... nOut - 1
BIOEM_HIDDEN hipError_t bioem_slice_axis_launch(hipStream_t st, const double2 *in, size_t outer, int nIn, int nOut,
                                                size_t inner, int PN, const double2 *twP, double2 *out);
// spec [PN][PN][PH] becomes C in place; e: the three tables e0, e1, e2 of PN entries each, indexed by the stored index
BIOEM_HIDDEN hipError_t bioem_slice_centre_launch(hipStream_t st, double2 *spec, int PN, int o, const double2 *twP,
                                                  const double2 *e);
// the slices of the n orientations whose matrices are R[i][9] into outF (float2) or outD (double2), [n][N][H]; tempDen
// (may be null): tempDen[i] = normDen
BIOEM_HIDDEN hipError_t bioem_slice_project_launch(hipStream_t st, const double2 *C, int pad, const double *R, int n, int N,
                                                   const double2 *tw, int shiftX, int shiftY, double normDen, float2 *outF,
                                                   double2 *outD, double *tempDen);

#ifdef BIOEM_SLICE_TU

namespace
{

// grid (outputs / 256): output t = (o nOut + k) inner + c
__global__ __launch_bounds__(256) void k_slice_axis(const double2 *__restrict__ in, size_t outer, int nIn, int nOut,
                                                    size_t inner, int PN, const double2 *__restrict__ twP,
                                                    double2 *__restrict__ out)
{
  const size_t t = (size_t) blockIdx.x * 256 + threadIdx.x;
  if (t >= outer * (size_t) nOut * inner)
    return;
  const size_t c = t % inner, ok = t / inner;
  const int k = (int) (ok % (size_t) nOut);
  const size_t o = ok / (size_t) nOut;
  const double2 *src = in + o * (size_t) nIn * inner + c;
  const int step = k % PN;
  int idx = 0;
  double ar = 0., ai = 0.;
  for (int x = 0; x < nIn; x++)
  {
    const double2 v = src[(size_t) x * inner], w = twP[idx];
    // v conj(w)
    ar = fma(v.x, w.x, ar);
    ar = fma(v.y, w.y, ar);
    ai = fma(v.y, w.x, ai);
    ai = fma(-v.x, w.y, ai);
    idx += step;
    if (idx >= PN)
      idx -= PN;
  }
  out[t] = make_double2(ar, ai);
}

// grid (tiles of a plane, PN): stored (i0, i1, k2)
__global__ __launch_bounds__(256) void k_slice_centre(double2 *__restrict__ spec, int PN, int PH, int o,
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
  double2 v = spec[at];
  const double2 w[4] = {twP[r], e[i0], e[PN + i1], e[2 * PN + k2]};
#pragma unroll
  for (int j = 0; j < 4; j++)
    v = make_double2(v.x * w[j].x - v.y * w[j].y, v.x * w[j].y + v.y * w[j].x);
  spec[at] = v;
}

// one tap: where it reads, whether it counts and whether it is conjugated.  The address is formed from indices that were
// checked: an outside tap reads element 0 and is dropped
__device__ inline size_t slice_tap(int k0, int k1, int k2, int PN, int PH, int MP, bool &inside, bool &neg)
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

// the one rounding to float of a run's slice; bioem_hip_debug_slices keeps the doubles
__device__ inline void slice_store(float2 *p, double re, double im) { *p = make_float2((float) re, (float) im); }
__device__ inline void slice_store(double2 *p, double re, double im) { *p = make_double2(re, im); }

// Block = patch (blockIdx.x) of kSlicePatchA x kSlicePatchB coefficients of orientation blockIdx.y; lane l owns stored row
// ia = A pa + l / B and column b = B pb + l % B.  The six matrix entries of rows 0 and 1 are block-uniform (scalar loads);
// the de-centring twiddle and a lane's eight taps are loaded before the first is consumed; a tap that does not count is
// selected away, not branched around (the sum keeps its bits: nothing is added for it).
template <class Out>
__global__ __launch_bounds__(256) void k_slice_project(const double2 *__restrict__ C, int pad, int PN, int PH, int MP,
                                                       const double *__restrict__ R, int N, int H, int patchesB,
                                                       const double2 *__restrict__ tw, int shiftX, int shiftY,
                                                       double normDen, Out *__restrict__ out, double *__restrict__ tempDen)
{
  const int g = blockIdx.y;
  const int pa = blockIdx.x / patchesB, pb = blockIdx.x - pa * patchesB;
  const int ia = kSlicePatchA * pa + (int) threadIdx.x / kSlicePatchB, b = kSlicePatchB * pb + (int) threadIdx.x % kSlicePatchB;
  if (blockIdx.x == 0 && threadIdx.x == 0 && tempDen)
    tempDen[g] = normDen;
  if (ia >= N || b >= H)
    return;
  const int M = (N - 1) / 2, o = (N + 1) / 2;
  const int a = ia <= N / 2 ? ia : ia - N;
  const size_t at = ((size_t) g * N + ia) * H + b;
  if (a * a + b * b > M * M)
  {
    slice_store(out + at, 0., 0.);
    return;
  }
  // the twiddle index (-o (a + b) + shiftX a + shiftY b) mod N, every product reduced in 32 bits (N < 32768)
  int e = (-((o * (a + b)) % N) + ((shiftX % N) * a) % N + ((shiftY % N) * b) % N) % N;
  e = e < 0 ? e + N : e;
  const double2 w = tw[e];
  const double *Rg = R + 9 * (size_t) g;
  const double da = (double) a, db = (double) b, dp = (double) pad, lim = (double) PN;
  const double q0 = dp * ((da * Rg[0]) + (db * Rg[3])), q1 = dp * ((da * Rg[1]) + (db * Rg[4])),
               q2 = dp * ((da * Rg[2]) + (db * Rg[5]));
  double sr = 0., si = 0.;
  if (fabs(q0) < lim && fabs(q1) < lim && fabs(q2) < lim) // (false for a NaN; beyond, the conversion to int would overflow)
  {
    const double c0 = floor(q0), c1 = floor(q1), c2 = floor(q2);
    const double f0 = q0 - c0, f1 = q1 - c1, f2 = q2 - c2, g0 = 1. - f0, g1 = 1. - f1, g2 = 1. - f2;
    const int i0 = (int) c0, i1 = (int) c1, i2 = (int) c2;
    double2 v[8];
    bool inside[8], neg[8];
#pragma unroll
    for (int t = 0; t < 8; t++)
      v[t] = C[slice_tap(i0 + (t >> 2), i1 + ((t >> 1) & 1), i2 + (t & 1), PN, PH, MP, inside[t], neg[t])];
#pragma unroll
    for (int t = 0; t < 8; t++)
    {
      const double wt = (((t >> 2) ? f0 : g0) * (((t >> 1) & 1) ? f1 : g1)) * ((t & 1) ? f2 : g2);
      const double tr = sr + wt * v[t].x, ti = si + wt * (neg[t] ? -v[t].y : v[t].y);
      sr = inside[t] ? tr : sr;
      si = inside[t] ? ti : si;
    }
  }
  const double xr = sr * w.x - si * w.y, xi = sr * w.y + si * w.x;
  slice_store(out + at, xr, xi);
}

} // namespace
#endif // BIOEM_SLICE_TU

#endif
