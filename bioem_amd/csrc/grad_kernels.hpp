// grad_kernels.hpp -- the gradient of the log posterior of a (particle, orientation, CTF, shift) request with respect to
// the density of every model point (bioem_hip_model_gradient, bioem_hip_debug_grad_image, bioem_hip_debug_grad_gather;
// DESIGN 2.19).  With U the unnormalised projection, T = tempden, P = (NormDen / T) U, conv = P^ conj(K) and the
// reference's log posterior L(s, ssq, cc) at s = sumC, ssq = sumsquareC and the cross-correlation cc of the request:
//   k_grad_coef      a = dL/ds, b = dL/dssq, g = dL/dcc in double, one lane per record;
//   k_grad_spectrum  G^_P[k] = (a Nt [k = 0] + 2 b conv[k] + g F[k] exp(-2 pi i ((kx dx + ky dy) mod N) / N)) K[k], double;
//   k_grad_cols, k_grad_rows   G_P = c2r(G^_P) / Nt: the two exact-DFT passes of render_kernels.hpp on double input, the
//                    Hermitian part taken in the self-conjugate columns as there;
//   k_grad_gather    u_k = v_k sum s_k[di][dj] G_P[i_k + di][j_k + dj]: the adjoint of the splat, one lane per point, on the
//                    pixels and under the skip rules of k_project_coords, the footprint weights of k_project_stamps at
//                    unit density; per tile of 256 points the partial sums of rho_k u_k and v_k rho_k sigma_k;
//   k_grad_norm      m = sum rho_k u_k and T = sum v_k rho_k sigma_k of a record: the tiles' partial sums in tile order;
//   k_grad_fold      dL/drho_k = (NormDen / T) (u_k - v_k sigma_k m / T), one lane per point walking the batch's records in
//                    request order into the weighted sums that a device buffer carries from batch to batch.
// No atomics and no cross-lane operation other than the fixed tree of a block's partial sums: a record's row depends on
// the record alone, the sums on the requests in request order -- the same bits for any batch size, boundary and run.
// The gradient is that of the double closed form at the device's (float) linearisation point: the float roundings of
// the pipeline -- the map narrowed to float, float spectra, cc rounded once, the density inside the float numerator of
// a sphere's weight -- are not differentiated.
// The declarations are for every translation unit; the kernels are compiled by kernels_grad.hip only (BIOEM_GRAD_TU).
#ifndef BIOEM_GRAD_KERNELS_HPP
#define BIOEM_GRAD_KERNELS_HPP

#include "engine_types.hpp"

const int kGradTile = 256; // model points of a block of the gather

// one record: the image of `kern` that holds its CTF kernel, where the particle's sums lie, and where its cc and
// {sumC, sumsquareC} lie in the arrays k_grad_coef reads
struct BioemGradRecord
{
  int kernel, sums, cell, pad;
};

BIOEM_HIDDEN int bioem_grad_tiles(int nPts);
// coef[n][4] = {a, b, g, (m: k_grad_norm)} and, where asked for, the records' parameters side by side
BIOEM_HIDDEN hipError_t bioem_grad_coef_launch(hipStream_t st, const BioemGradRecord *rec, const float *cc,
                                               const bioem_hip_param5 *params, const float *sumRef, const float *sumsqRef,
                                               int n, int N, double *coef, bioem_hip_param5 *paramsOut);
// spec[n][N][H] double pairs (reference layout) from Pw / Z [n][M] in the walk order of the scan's preparation and
// kern[.][N][H] (reference layout); convGiven: Pw holds conv
BIOEM_HIDDEN hipError_t bioem_grad_spectrum_launch(hipStream_t st, const float2 *Pw, const double2 *Z, const float2 *kern,
                                                   const BioemGradRecord *rec, const double *coef, int convGiven, int n,
                                                   int N, double2 *spec);
// map[n][N][N] = c2r(spec) / (N N); cols [n][N][H] double pairs of scratch
BIOEM_HIDDEN hipError_t bioem_grad_inverse_launch(hipStream_t st, const double2 *spec, int n, int N, int A, int B,
                                                  const double2 *tw, double2 *cols, double *map);
// u[n][nPts], vs[n][nPts] = v sigma, part[n][tiles][2] from the maps and the orientations angles[o0 ... o0 + n)
BIOEM_HIDDEN hipError_t bioem_grad_gather_launch(hipStream_t st, const bioem_hip_model_point *pts, int nPts,
                                                 const float4 *angles, int o0, int isQuat, int N, float pixelSize, int shiftX,
                                                 int shiftY, const double *map, int n, double *u, double *vs, double *part);
// the rows grad[n][nPts] (or null), m into coef[.][3], and the records folded into acc[nPts] with weights w[n]
BIOEM_HIDDEN hipError_t bioem_grad_fold_launch(hipStream_t st, const double *u, const double *vs, const double *part,
                                               const double *w, int n, int nPts, float NormDen, double *mT, double *coef,
                                               double *grad, bioem_hip_grad_point *acc);

#ifdef BIOEM_GRAD_TU
#include "project_rotation.hpp"

namespace
{

// grid (records / 64), one lane per record; every division in double
__global__ __launch_bounds__(64) void k_grad_coef(const BioemGradRecord *__restrict__ rec, const float *__restrict__ cc,
                                                  const bioem_hip_param5 *__restrict__ params,
                                                  const float *__restrict__ sumRef, const float *__restrict__ sumsqRef,
                                                  int n, double Nt, double *__restrict__ coef,
                                                  bioem_hip_param5 *__restrict__ paramsOut)
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
  coef[4 * r + 0] = h1 * (2. * sr * c - 2. * ssr * s) / fe + h2 * (-2. * s) / F;
  coef[4 * r + 1] = h1 * (Nt * ssr - sr * sr) / fe + h2 * Nt / F;
  coef[4 * r + 2] = h1 * (-2. * Nt * c + 2. * sr * s) / fe;
  if (paramsOut)
    paramsOut[r] = p;
}

// grid (blocks per record, records).  The record's projection Pw and Z = w conj(F) tw come in the walk order of the scan's
// preparation (scan_kernels.hpp: the twiddle index reduced in integers there), so F conj(tw) = conj(Z) / w exactly; the
// record and its coefficients are wave-uniform (scalar loads); the kernel's coefficient is read, and G^_P stored, in the
// reference layout the inverse passes read
__global__ __launch_bounds__(256) void k_grad_spectrum(const float2 *__restrict__ Pw, const double2 *__restrict__ Z,
                                                       const float2 *__restrict__ kern,
                                                       const BioemGradRecord *__restrict__ rec,
                                                       const double *__restrict__ coef, int convGiven, int N, int H,
                                                       double2 *__restrict__ spec)
{
  const int r = blockIdx.y;
  const int M = N * H;
  const int jend = (N & 1) ? H : H - 1;
  const double a = coef[4 * r + 0], b2 = 2. * coef[4 * r + 1], g = coef[4 * r + 2];
  const double Nt = (double) N * (double) N;
  const float2 *P = Pw + (size_t) r * M, *K = kern + (size_t) rec[r].kernel * M;
  const double2 *Zr = Z + (size_t) r * M;
  double2 *out = spec + (size_t) r * M;
  for (int pos = blockIdx.x * blockDim.x + threadIdx.x; pos < M; pos += gridDim.x * blockDim.x)
  {
    const int i = pos / H, q = pos - i * H;
    const int j = q < jend - 1 ? q + 1 : (q == jend - 1 ? 0 : H - 1); // the walk order: interior columns, 0, N / 2
    const int e = i * H + j;
    const float2 p = P[pos], c = K[e];
    const double2 z = Zr[pos];
    float2 o = p;
    if (!convGiven)
    { // the expression of k_convolve
      o.x = p.x * c.x + p.y * c.y;
      o.y = p.y * c.x - p.x * c.y;
    }
    const double iw = (j == 0 || 2 * j == N) ? 1. : 0.5;
    double cr = fma(g, z.x * iw, b2 * (double) o.x), ci = fma(g, -(z.y * iw), b2 * (double) o.y);
    if (e == 0)
      cr += a * Nt;
    const double kr = (double) c.x, ki = (double) c.y;
    out[e] = make_double2(fma(cr, kr, -(ci * ki)), fma(cr, ki, ci * kr));
  }
}

// column k of record b: N-point inverse along the first axis (k_render_cols on double input).  grid (H, records);
// dynamic LDS 2 N double pairs
__global__ void k_grad_cols(const double2 *__restrict__ spec, int N, int H, int A, int B, const double2 *__restrict__ tw,
                            double2 *__restrict__ colspec)
{
  extern __shared__ double srow[];
  double2 *col = reinterpret_cast<double2 *>(srow);
  double2 *Y = col + N;
  const int k = blockIdx.x, b = blockIdx.y;
  const double2 *S = spec + (size_t) b * N * H;
  for (int i = threadIdx.x; i < N; i += blockDim.x)
    col[i] = S[(size_t) i * H + k];
  __syncthreads();
  for (int e = threadIdx.x; e < N; e += blockDim.x)
  {
    const int j1 = e / B, kb = e - j1 * B;
    double ar = 0., ai = 0.;
    int idx = 0;
    const int step = (A * kb) % N;
    for (int j2 = 0; j2 < B; j2++)
    {
      const double2 w = tw[idx];
      const double2 x = col[A * j2 + j1];
      ar = fma(x.x, w.x, ar);
      ar = fma(-x.y, w.y, ar);
      ai = fma(x.y, w.x, ai);
      ai = fma(x.x, w.y, ai);
      idx += step;
      if (idx >= N)
        idx -= N;
    }
    Y[e] = make_double2(ar, ai);
  }
  __syncthreads();
  for (int u = threadIdx.x; u < N; u += blockDim.x)
  {
    const int kb = u % B;
    double ar = 0., ai = 0.;
    int idx = 0;
    for (int j1 = 0; j1 < A; j1++)
    {
      const double2 w = tw[idx];
      const double2 y = Y[j1 * B + kb];
      ar = fma(y.x, w.x, ar);
      ar = fma(-y.y, w.y, ar);
      ai = fma(y.y, w.x, ai);
      ai = fma(y.x, w.y, ai);
      idx += u;
      if (idx >= N)
        idx -= N;
    }
    colspec[((size_t) b * N + u) * H + k] = make_double2(ar, ai);
  }
}

// row i of record b: Hermitian extension (the imaginary parts of entry 0 and, N even, of entry N / 2 dropped: the
// Hermitian part of the self-conjugate columns), N-point inverse, real part / (N N).  grid (N, records); dynamic LDS 2 N
// double pairs
__global__ void k_grad_rows(const double2 *__restrict__ colspec, int N, int H, int A, int B,
                            const double2 *__restrict__ tw, double *__restrict__ map)
{
  extern __shared__ double srow[];
  double2 *row = reinterpret_cast<double2 *>(srow);
  double2 *Y = row + N;
  const int i = blockIdx.x, b = blockIdx.y;
  const double2 *src = colspec + ((size_t) b * N + i) * H;
  for (int k = threadIdx.x; k < H; k += blockDim.x)
  {
    double2 v = src[k];
    if (k == 0 || 2 * k == N)
      v.y = 0.;
    row[k] = v;
    if (k > 0 && 2 * k != N)
      row[N - k] = make_double2(v.x, -v.y);
  }
  __syncthreads();
  for (int e = threadIdx.x; e < N; e += blockDim.x)
  {
    const int j1 = e / B, kb = e - j1 * B;
    double ar = 0., ai = 0.;
    int idx = 0;
    const int step = (A * kb) % N;
    for (int j2 = 0; j2 < B; j2++)
    {
      const double2 w = tw[idx];
      const double2 x = row[A * j2 + j1];
      ar = fma(x.x, w.x, ar);
      ar = fma(-x.y, w.y, ar);
      ai = fma(x.y, w.x, ai);
      ai = fma(x.x, w.y, ai);
      idx += step;
      if (idx >= N)
        idx -= N;
    }
    Y[e] = make_double2(ar, ai);
  }
  __syncthreads();
  const double Nt = (double) N * (double) N;
  double *dst = map + ((size_t) b * N + i) * N;
  for (int j = threadIdx.x; j < N; j += blockDim.x)
  {
    const int kb = j % B;
    double ar = 0.;
    int idx = 0;
    for (int j1 = 0; j1 < A; j1++)
    {
      const double2 w = tw[idx];
      const double2 y = Y[j1 * B + kb];
      ar = fma(y.x, w.x, ar);
      ar = fma(-y.y, w.y, ar);
      idx += j;
      if (idx >= N)
        idx -= N;
    }
    dst[j] = ar / Nt;
  }
}

// grid (tiles of kGradTile points, records).  The rotation, the pixel and the skip rules are the expressions of
// k_project_coords; the weight is that of k_project_stamps with the density left out of the float numerator.  A sphere's
// cells are walked row by row; sigma is the sum of its weights in that order, whether the point is kept or not.
__global__ __launch_bounds__(kGradTile) void k_grad_gather(const bioem_hip_model_point *__restrict__ pts, int nPts,
                                                           const float4 *__restrict__ angles, int o0, int isQuat, int N,
                                                           float pixelSize, int shiftX, int shiftY,
                                                           const double *__restrict__ maps, double *__restrict__ u,
                                                           double *__restrict__ vs, double *__restrict__ part)
{
  __shared__ double redM[kGradTile], redT[kGradTile];
  const int ob = blockIdx.y, n = blockIdx.x * kGradTile + threadIdx.x;
  const double *G = maps + (size_t) ob * N * N;
  double um = 0., st = 0.;
  if (n < nPts)
  {
    float rotmat[3][3];
    rotation_matrix(angles[o0 + ob], isQuat, rotmat);
    const bioem_hip_model_point p = pts[n];
    float rp[3] = {0.f, 0.f, 0.f};
    for (int k = 0; k < 3; k++)
      for (int j = 0; j < 3; j++)
        rp[k] += rotmat[k][j] * p.pos[j];
    int i = (int) floorf(rp[0] / pixelSize + (float) N / 2.0f + 0.5f);
    int j = (int) floorf(rp[1] / pixelSize + (float) N / 2.0f + 0.5f);
    double uk = 0., sigma = 1.;
    bool ok;
    if (p.radius <= pixelSize)
    {
      ok = !(i < 0 || j < 0 || i >= N || j >= N);
      if (ok)
        uk = G[i * N + j];
    }
    else
    {
      i -= shiftX;
      j -= shiftY;
      const int irad = (int) (p.radius / pixelSize) + 1;
      ok = !(i < irad || j < irad || i >= N - irad || j >= N - irad);
      const float radius = p.radius, rad2 = radius * radius;
      const double den = 4 * M_PI * radius * rad2;
      sigma = 0.;
      for (int di = -irad; di <= irad; di++)
        for (int dj = -irad; dj <= irad; dj++)
        {
          const float dist = ((float) (di) * (di) + (dj) * (dj)) * pixelSize * pixelSize;
          if (dist < rad2)
          {
            const double w = (double) (pixelSize * pixelSize * 2 * sqrtf(rad2 - dist) * 3) / den;
            sigma += w;
            if (ok)
              uk = fma(w, G[(i + di) * N + (j + dj)], uk);
          }
        }
    }
    const double vsig = ok ? sigma : 0.;
    u[(size_t) ob * nPts + n] = uk;
    vs[(size_t) ob * nPts + n] = vsig;
    um = (double) p.density * uk;
    st = (double) p.density * vsig;
  }
  redM[threadIdx.x] = um;
  redT[threadIdx.x] = st;
  __syncthreads();
  for (int s = kGradTile / 2; s > 0; s >>= 1)
  { // a fixed tree: the same bits in every run
    if ((int) threadIdx.x < s)
    {
      redM[threadIdx.x] += redM[threadIdx.x + s];
      redT[threadIdx.x] += redT[threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0)
  {
    double *o = part + 2 * ((size_t) ob * gridDim.x + blockIdx.x);
    o[0] = redM[0];
    o[1] = redT[0];
  }
}

// one lane per record: the tiles in tile order
__global__ __launch_bounds__(64) void k_grad_norm(const double *__restrict__ part, int tiles, int n, double *__restrict__ mT,
                                                  double *__restrict__ coef)
{
  const int r = blockIdx.x * 64 + threadIdx.x;
  if (r >= n)
    return;
  double m = 0., T = 0.;
  for (int t = 0; t < tiles; t++)
  {
    m += part[2 * ((size_t) r * tiles + t)];
    T += part[2 * ((size_t) r * tiles + t) + 1];
  }
  mT[2 * r] = m;
  mT[2 * r + 1] = T;
  coef[4 * r + 3] = m;
}

// one lane per model point, the records of the batch in request order
__global__ __launch_bounds__(256) void k_grad_fold(const double *__restrict__ u, const double *__restrict__ vs,
                                                   const double *__restrict__ mT, const double *__restrict__ w, int n,
                                                   int nPts, double NormDen, double *__restrict__ grad,
                                                   bioem_hip_grad_point *__restrict__ acc)
{
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nPts)
    return;
  bioem_hip_grad_point A = acc[k];
  for (int r = 0; r < n; r++)
  {
    const double m = mT[2 * r], T = mT[2 * r + 1];
    const double uk = u[(size_t) r * nPts + k], vsig = vs[(size_t) r * nPts + k];
    const double gk = (NormDen / T) * (uk - vsig * m / T);
    if (grad)
      grad[(size_t) r * nPts + k] = gk;
    const double wr = w[r], wg = wr * gk;
    A.sum += wg;
    A.sumsq += wg * wg;
    if (vsig != 0.)
    {
      A.sumw += wr;
      A.count += 1;
    }
  }
  acc[k] = A;
}

} // namespace
#endif // BIOEM_GRAD_TU

#endif
