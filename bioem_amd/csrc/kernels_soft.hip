// kernels_soft.hip -- the table passes and the accumulation of the posterior-weighted view sums (soft_kernels.hpp) and
// their launchers
#define BIOEM_SOFT_TU 1
#include "soft_kernels.hpp"

static_assert(sizeof(BioemSoftMember) == 32, "member layout");

static bool soft_tables_ok(int n, int nd, int N) { return N >= 2 && N <= 4096 && nd >= 1 && nd <= N && n >= 1 && n <= 65535; }

hipError_t bioem_soft_cols_launch(hipStream_t st, const double *cells, const int *xm, int n, int nd, int N, const double2 *tw,
                                  double2 *U)
{
  if (!soft_tables_ok(n, nd, N))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_soft_cols, dim3(nd, n), dim3(kSoftTableThreads), 0, st, cells, xm, nd, N, N / 2 + 1, tw, U);
  return hipGetLastError();
}

hipError_t bioem_soft_rows_launch(hipStream_t st, const double2 *U, const int *xm, int n, int nd, int N, const double2 *tw,
                                  double2 *W)
{
  if (!soft_tables_ok(n, nd, N))
    return hipErrorInvalidValue;
  const int H = N / 2 + 1;
  hipLaunchKernelGGL(k_soft_rows, dim3((N + kSoftRows - 1) / kSoftRows, (H + kSoftTableThreads - 1) / kSoftTableThreads, n), dim3(kSoftTableThreads), 0, st, U,
                     xm, nd, N, H, tw, W);
  return hipGetLastError();
}

hipError_t bioem_soft_accumulate_launch(hipStream_t st, const float2 *specR, const float2 *ctf, const BioemSoftMember *mem,
                                        const int *off, int nGroups, int N, const double2 *W, double2 *num, double *den)
{
  if (N < 2 || nGroups < 1 || nGroups > 65535)
    return hipErrorInvalidValue;
  const int H = N / 2 + 1;
  const size_t M = (size_t) N * H, perBlock = 2 * (size_t) kSoftThreads;
  hipLaunchKernelGGL(k_soft_accumulate, dim3((unsigned) ((M + perBlock - 1) / perBlock), nGroups), dim3(kSoftThreads), 0, st,
                     specR, ctf, mem, off, N, H, W, num, den);
  return hipGetLastError();
}
