// kernels_slice.hip -- the spectrum of a volume model, its centring and the central slices that stand in for the real-space
// projection and its r2c (slice_kernels.hpp), and their launchers
#define BIOEM_SLICE_TU 1
#include "slice_kernels.hpp"

hipError_t bioem_slice_axis_launch(hipStream_t st, const double2 *in, size_t outer, int nIn, int nOut, size_t inner, int PN,
                                   const double2 *twP, double2 *out)
{
  const size_t total = outer * (size_t) nOut * inner;
  if (nIn < 1 || nOut < 1 || PN < 2 || total < 1 || (total + 255) / 256 > 0x7fffffffull)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_slice_axis, dim3((unsigned) ((total + 255) / 256)), dim3(256), 0, st, in, outer, nIn, nOut, inner, PN,
                     twP, out);
  return hipGetLastError();
}

hipError_t bioem_slice_centre_launch(hipStream_t st, double2 *spec, int PN, int o, const double2 *twP, const double2 *e)
{
  if (PN < 2)
    return hipErrorInvalidValue;
  const int PH = PN / 2 + 1;
  hipLaunchKernelGGL(k_slice_centre, dim3((unsigned) ((PN * PH + 255) / 256), (unsigned) PN), dim3(256), 0, st, spec, PN, PH,
                     o, twP, e);
  return hipGetLastError();
}

hipError_t bioem_slice_project_launch(hipStream_t st, const double2 *C, int pad, const double *R, int n, int N,
                                      const double2 *tw, int shiftX, int shiftY, double normDen, float2 *outF, double2 *outD,
                                      double *tempDen)
{
  if (N < 2 || N >= 32768 || n < 1 || (pad != 1 && pad != 2) || (!outF) == (!outD))
    return hipErrorInvalidValue;
  const int H = N / 2 + 1, PN = pad * N, PH = PN / 2 + 1, MP = (PN - 1) / 2;
  static_assert(kSlicePatchA * kSlicePatchB == 256, "a patch is a block of 256 lanes");
  const int patchesA = (N + kSlicePatchA - 1) / kSlicePatchA, patchesB = (H + kSlicePatchB - 1) / kSlicePatchB;
  const size_t M = (size_t) N * H;
  for (int g0 = 0; g0 < n; g0 += 32768) // (the y extent of a grid)
  {
    const int ng = std::min(32768, n - g0);
    const dim3 grid((unsigned) (patchesA * patchesB), (unsigned) ng);
    double *td = tempDen ? tempDen + g0 : nullptr;
    if (outF)
      hipLaunchKernelGGL(k_slice_project<float2>, grid, dim3(256), 0, st, C, pad, PN, PH, MP, R + 9 * (size_t) g0, N, H,
                         patchesB, tw, shiftX, shiftY, normDen, outF + M * g0, td);
    else
      hipLaunchKernelGGL(k_slice_project<double2>, grid, dim3(256), 0, st, C, pad, PN, PH, MP, R + 9 * (size_t) g0, N, H,
                         patchesB, tw, shiftX, shiftY, normDen, outD + M * g0, td);
  }
  return hipGetLastError();
}
