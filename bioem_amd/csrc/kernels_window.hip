// kernels_window.hip -- the window pass of bioem_hip_window_posterior (window_kernels.hpp) and its launchers
#define BIOEM_WINDOW_TU 1
#include "window_kernels.hpp"

size_t bioem_window_scratch(int N, int nd, int nImg) { return (size_t) nImg * (size_t) nd * (size_t) (N / 2 + 1); }

hipError_t bioem_window_prep_launch(hipStream_t st, const float2 *proj, const float2 *ctf, const float *ctfParam,
                                    const BioemWindowRecord *rec, int n, int N, float2 *conv, float *terms, int M4,
                                    bioem_hip_param5 *params)
{
  if (N < 1 || n < 1)
    return hipErrorInvalidValue;
  const int H = N / 2 + 1;
  const size_t M = (size_t) N * H;
  const unsigned blocks = (unsigned) std::min<size_t>(64, (M + 255) / 256); // a function of N alone
  hipLaunchKernelGGL(k_window_prep, dim3(blocks, (unsigned) n), dim3(256), 0, st, proj, ctf, ctfParam, rec, N, H, conv, terms,
                     M4, params);
  return hipGetLastError();
}

hipError_t bioem_window_launch(hipStream_t st, const float2 *conv, const float2 *ref, const BioemWindowRecord *rec,
                               const bioem_hip_param5 *params, const double2 *postc, const float *sumRef,
                               const float *sumsqRef, const bioem_hip_param_device &pd, int n, int N, int nd,
                               const int *shifts, const double2 *tw, double2 *T, double *logp, float *cc)
{
  if (N < 1 || n < 1 || nd < 1)
    return hipErrorInvalidValue;
  const int H = N / 2 + 1;
  const dim3 gridCols((unsigned) ((H + 63) / 64), (unsigned) ((nd + kWindowRows - 1) / kWindowRows), (unsigned) n);
  hipLaunchKernelGGL(k_window_cols, gridCols, dim3(64 * kWindowSplit), 0, st, conv, ref, N, H, nd, shifts, tw, T);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess)
    return e;
  hipLaunchKernelGGL(k_window_cells, dim3((unsigned) nd, (unsigned) n), dim3(64), 0, st, T, rec, params, postc, sumRef,
                     sumsqRef, pd, N, H, nd, shifts, tw, logp, cc);
  return hipGetLastError();
}
