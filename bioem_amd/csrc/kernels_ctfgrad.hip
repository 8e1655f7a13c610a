// kernels_ctfgrad.hip -- the gradient and curvature of the log posterior with respect to the CTF triple of a request: the
// twenty sums over the walk order, the rows built from them (ctfgrad_kernels.hpp), and their launchers
#define BIOEM_CTFGRAD_TU 1
#include "ctfgrad_kernels.hpp"

int bioem_ctfgrad_blocks(int N)
{
  const int H = N / 2 + 1;
  return (N * H + kCtfgBlock - 1) / kCtfgBlock;
}

hipError_t bioem_ctfgrad_sums_launch(hipStream_t st, const float2 *Pw, const double2 *Z, const BioemGradRecord *rec,
                                     const float *ctfParam, const int *rowIdx, const float *radsq, int n, int N,
                                     double *partial, double *sums, double *derivs)
{
  if (N < 2 || N >= 32768 || n < 1 || n > 65535)
    return hipErrorInvalidValue;
  const int H = N / 2 + 1, blocks = bioem_ctfgrad_blocks(N);
  hipLaunchKernelGGL(k_ctfgrad_partials, dim3((unsigned) blocks, (unsigned) n), dim3(kCtfgBlock), 0, st, Pw, Z, rec, ctfParam,
                     rowIdx, radsq, N, H, partial, derivs);
  hipLaunchKernelGGL(k_ctfgrad_fold, dim3((unsigned) ((kCtfgSums * n + 63) / 64)), dim3(64), 0, st, partial, n, blocks, sums);
  return hipGetLastError();
}

hipError_t bioem_ctfgrad_finish_launch(hipStream_t st, const double *sums, const BioemGradRecord *rec, const float *cc,
                                       const bioem_hip_param5 *params, const float *sumRef, const float *sumsqRef,
                                       const double *coef, const bioem_hip_param_device &pd, int n, int N, double *row)
{
  if (n < 1)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_ctfgrad_finish, dim3((unsigned) ((n + 63) / 64)), dim3(64), 0, st, sums, rec, cc, params, sumRef,
                     sumsqRef, coef, pd, n, (double) N * (double) N, row);
  return hipGetLastError();
}
