// kernels_pose.hip -- the gradient with respect to the orientation matrix and the model shifts of a volume model: the nine
// sums of a request over the coefficients of its slice (pose_kernels.hpp), and their launcher
#define BIOEM_POSE_TU 1
#include "pose_kernels.hpp"

int bioem_pose_patches(int N)
{
  const int H = N / 2 + 1;
  return ((N + kSlicePatchA - 1) / kSlicePatchA) * ((H + kSlicePatchB - 1) / kSlicePatchB);
}

hipError_t bioem_pose_launch(hipStream_t st, const double2 *C, int pad, const double *R, const double2 *Y, int n, int N,
                             double *partial, double *row)
{
  if (N < 2 || N >= 32768 || n < 1 || n > 65535 || (pad != 1 && pad != 2))
    return hipErrorInvalidValue;
  const int H = N / 2 + 1, PN = pad * N, PH = PN / 2 + 1, MP = (PN - 1) / 2;
  const int patchesB = (H + kSlicePatchB - 1) / kSlicePatchB, patches = bioem_pose_patches(N);
  hipLaunchKernelGGL(k_pose_partials, dim3((unsigned) patches, (unsigned) n), dim3(256), 0, st, C, pad, PN, PH, MP, R, Y, N, H,
                     patchesB, partial);
  hipLaunchKernelGGL(k_pose_fold, dim3((unsigned) ((kPoseSums * n + 63) / 64)), dim3(64), 0, st, partial, R, n, patches, row);
  return hipGetLastError();
}
