// kernels_vgrad.hip -- the gradient with respect to the voxels of a volume model: the back-insertion of gradient spectra into
// the model's spectrum, the transpose of the slice, and the transpose of the upload's passes (vgrad_kernels.hpp), and their
// launchers
#define BIOEM_VGRAD_TU 1
#include "vgrad_kernels.hpp"

hipError_t bioem_vgrad_views_launch(hipStream_t st, const double *R, int n, int pad, double *view, int *flag)
{
  if (n < 1 || (pad != 1 && pad != 2))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_vgrad_views, dim3((n + 63) / 64), dim3(64), 0, st, R, n, (double) pad, view, flag);
  return hipGetLastError();
}

hipError_t bioem_vgrad_prepare_launch(hipStream_t st, const double2 *spec, const double *w, int n, int N, const double2 *tw,
                                      int shiftX, int shiftY, int full, double2 *Y)
{
  if (N < 2 || N >= 32768 || n < 1 || n > 65535)
    return hipErrorInvalidValue;
  const int H = N / 2 + 1;
  hipLaunchKernelGGL(k_vgrad_prepare, dim3((unsigned) ((N * H + 255) / 256), (unsigned) n), dim3(256), 0, st, spec, w, N, H, tw,
                     shiftX, shiftY, full, Y);
  return hipGetLastError();
}

hipError_t bioem_vgrad_insert_launch(hipStream_t st, const double2 *Y, const double *R, const double *view, int n, int N,
                                     int pad, int cull, int first, double2 *A)
{
  if (N < 2 || N >= 32768 || n < 1 || (pad != 1 && pad != 2))
    return hipErrorInvalidValue;
  const int H = N / 2 + 1, PN = pad * N, PH = PN / 2 + 1, MP = (PN - 1) / 2;
  const unsigned bN = (unsigned) ((PN + kVgradBrick - 1) / kVgradBrick), bH = (unsigned) ((PH + kVgradBrick - 1) / kVgradBrick);
  if (bN > 65535u)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_vgrad_insert, dim3(bH, bN, bN), dim3(64), 0, st, Y, R, view, n, N, H, pad, PN, PH, MP, cull, first, A);
  return hipGetLastError();
}

hipError_t bioem_vgrad_dot_launch(hipStream_t st, const double2 *spec, const double2 *slices, int n, int N, double *dot,
                                  int dotStride)
{
  if (N < 2 || n < 1)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_vgrad_dot, dim3((unsigned) n), dim3(256), 0, st, spec, slices, N, N / 2 + 1, dot, dotStride);
  return hipGetLastError();
}

hipError_t bioem_vgrad_uncentre_launch(hipStream_t st, double2 *A, int PN, int o, const double2 *twP, const double2 *e)
{
  if (PN < 2 || PN > 65535)
    return hipErrorInvalidValue;
  const int PH = PN / 2 + 1;
  hipLaunchKernelGGL(k_vgrad_uncentre, dim3((unsigned) ((PN * PH + 255) / 256), (unsigned) PN), dim3(256), 0, st, A, PN, PH, o,
                     twP, e);
  return hipGetLastError();
}

hipError_t bioem_vgrad_axis_launch(hipStream_t st, const double2 *in, size_t outer, int nIn, int nOut, size_t inner, int PN,
                                   const double2 *twP, double2 *out)
{
  const size_t total = outer * (size_t) nOut * inner;
  if (nIn < 1 || nIn > PN || nOut < 1 || PN < 2 || total < 1 || (total + 255) / 256 > 0x7fffffffull)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_vgrad_axis, dim3((unsigned) ((total + 255) / 256)), dim3(256), 0, st, in, outer, nIn, nOut, inner, PN,
                     twP, out);
  return hipGetLastError();
}

hipError_t bioem_vgrad_finish_launch(hipStream_t st, const double2 *in, int N, const double *sinc2, int correct, double *gvol)
{
  if (N < 2 || N > 65535)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_vgrad_finish, dim3((unsigned) ((N * N + 255) / 256), (unsigned) N), dim3(256), 0, st, in, N, sinc2,
                     correct, gvol);
  return hipGetLastError();
}
