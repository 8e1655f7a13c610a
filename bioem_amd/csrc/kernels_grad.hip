// kernels_grad.hip -- the density gradient of bioem_hip_model_gradient (grad_kernels.hpp) and its launchers
#define BIOEM_GRAD_TU 1
#include "grad_kernels.hpp"

static_assert(sizeof(bioem_hip_grad_point) == 32 && sizeof(BioemGradRecord) == 16, "point / record layout");

int bioem_grad_tiles(int nPts) { return (nPts + kGradTile - 1) / kGradTile; }

hipError_t bioem_grad_coef_launch(hipStream_t st, const BioemGradRecord *rec, const float *cc, const bioem_hip_param5 *params,
                                  const float *sumRef, const float *sumsqRef, int n, int N, double *coef,
                                  bioem_hip_param5 *paramsOut)
{
  if (N < 2 || n < 1)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_grad_coef, dim3((n + 63) / 64), dim3(64), 0, st, rec, cc, params, sumRef, sumsqRef, n,
                     (double) N * (double) N, coef, paramsOut);
  return hipGetLastError();
}

hipError_t bioem_grad_spectrum_launch(hipStream_t st, const float2 *Pw, const double2 *Z, const float2 *kern,
                                      const BioemGradRecord *rec, const double *coef, int convGiven, int n, int N,
                                      double2 *spec)
{
  if (N < 2 || n < 1 || n > 65535)
    return hipErrorInvalidValue;
  const int H = N / 2 + 1;
  const size_t M = (size_t) N * H;
  const unsigned blocks = (unsigned) std::min<size_t>(64, (M + 255) / 256);
  hipLaunchKernelGGL(k_grad_spectrum, dim3(blocks, (unsigned) n), dim3(256), 0, st, Pw, Z, kern, rec, coef, convGiven, N, H, spec);
  return hipGetLastError();
}

hipError_t bioem_grad_inverse_launch(hipStream_t st, const double2 *spec, int n, int N, int A, int B, const double2 *tw,
                                     double2 *cols, double *map)
{
  if (N < 2 || n < 1 || n > 65535 || A * B != N)
    return hipErrorInvalidValue;
  const int H = N / 2 + 1;
  const size_t lds = sizeof(double2) * 2 * (size_t) N;
  // (the attribute belongs to the kernel: images beyond 2 048 pixels need more than 64 KiB)
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_grad_cols), hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds);
  if (e == hipSuccess)
    e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_grad_rows), hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds);
  if (e != hipSuccess)
    return e;
  hipLaunchKernelGGL(k_grad_cols, dim3(H, n), dim3(256), lds, st, spec, N, H, A, B, tw, cols);
  hipLaunchKernelGGL(k_grad_rows, dim3(N, n), dim3(256), lds, st, (const double2 *) cols, N, H, A, B, tw, map);
  return hipGetLastError();
}

hipError_t bioem_grad_gather_launch(hipStream_t st, const bioem_hip_model_point *pts, int nPts, const float4 *angles, int o0,
                                    int isQuat, int N, float pixelSize, int shiftX, int shiftY, const double *map, int n,
                                    double *u, double *vs, double *part)
{
  if (N < 2 || n < 1 || n > 65535 || nPts < 1)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_grad_gather, dim3((unsigned) bioem_grad_tiles(nPts), (unsigned) n), dim3(kGradTile), 0, st, pts, nPts,
                     angles, o0, isQuat, N, pixelSize, shiftX, shiftY, map, u, vs, part);
  return hipGetLastError();
}

hipError_t bioem_grad_fold_launch(hipStream_t st, const double *u, const double *vs, const double *part, const double *w, int n,
                                  int nPts, float NormDen, double *mT, double *coef, double *grad, bioem_hip_grad_point *acc)
{
  if (n < 1 || nPts < 1)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_grad_norm, dim3((n + 63) / 64), dim3(64), 0, st, part, bioem_grad_tiles(nPts), n, mT, coef);
  hipLaunchKernelGGL(k_grad_fold, dim3((nPts + 255) / 256), dim3(256), 0, st, u, vs, (const double *) mT, w, n, nPts,
                     (double) NormDen, grad, acc);
  return hipGetLastError();
}
