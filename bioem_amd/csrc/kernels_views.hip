// kernels_views.hip -- the accumulation and the Wiener division of the view averages (view_kernels.hpp) and their launchers
#define BIOEM_VIEW_TU 1
#include "view_kernels.hpp"

static_assert(sizeof(BioemViewMember) == 40, "member layout");

hipError_t bioem_view_accumulate_launch(hipStream_t st, const float2 *specR, const float2 *ctf, const BioemViewMember *mem,
                                        const int *off, int nGroups, int N, const double2 *tw, double2 *num, double *den)
{
  if (N < 2 || nGroups < 1 || nGroups > 65535)
    return hipErrorInvalidValue;
  const int H = N / 2 + 1;
  const size_t M = (size_t) N * H, perBlock = 2 * (size_t) kViewThreads;
  hipLaunchKernelGGL(k_view_accumulate, dim3((unsigned) ((M + perBlock - 1) / perBlock), nGroups), dim3(kViewThreads), 0, st,
                     specR, ctf, mem, off, N, H, tw, num, den);
  return hipGetLastError();
}

hipError_t bioem_view_wiener_launch(hipStream_t st, const double2 *num, const double *den, int nGroups, int N, double wiener,
                                    double *tau, float2 *dst)
{
  if (N < 2 || nGroups < 1 || nGroups > 65535)
    return hipErrorInvalidValue;
  const int M = N * (N / 2 + 1);
  hipLaunchKernelGGL(k_view_tau, dim3(nGroups), dim3(256), 0, st, den, M, wiener, tau);
  hipLaunchKernelGGL(k_view_wiener, dim3((M + 255) / 256, nGroups), dim3(256), 0, st, num, den, (const double *) tau, M, dst);
  return hipGetLastError();
}
