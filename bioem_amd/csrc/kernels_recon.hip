// kernels_recon.hip -- the insertion of view sums into a 3D Fourier volume, its estimate and the passes to the real-space
// volume that the gradient's inverse lacks (recon_kernels.hpp), and their launchers
#define BIOEM_RECON_TU 1
#include "recon_kernels.hpp"

hipError_t bioem_recon_matrices_launch(hipStream_t st, const float4 *angles, const int *orient, int isQuat, int n, double *R)
{
  if (n < 1)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_recon_matrices, dim3((n + 63) / 64), dim3(64), 0, st, angles, orient, isQuat, n, R);
  return hipGetLastError();
}

hipError_t bioem_recon_insert_launch(hipStream_t st, const double2 *num, const double *den, const int *slot, const double *R,
                                     int n, int N, const double2 *tw, int cull, double2 *numV, double *denV)
{
  if (N < 2 || n < 1)
    return hipErrorInvalidValue;
  const int H = N / 2 + 1;
  const unsigned bN = (unsigned) ((N + kReconBrick - 1) / kReconBrick), bH = (unsigned) ((H + kReconBrick - 1) / kReconBrick);
  hipLaunchKernelGGL(k_recon_insert, dim3(bH, bN, bN), dim3(64), 0, st, num, den, slot, R, n, N, H, tw, cull, numV, denV);
  return hipGetLastError();
}

hipError_t bioem_recon_estimate_launch(hipStream_t st, double2 *numV, const double *denV, int N, double wiener,
                                       const double2 *tw, double *part, double *tau)
{
  if (N < 2)
    return hipErrorInvalidValue;
  const int H = N / 2 + 1;
  const size_t n = (size_t) N * N * H;
  hipLaunchKernelGGL(k_recon_tau_part, dim3(kReconTauBlocks), dim3(256), 0, st, denV, n, part);
  hipLaunchKernelGGL(k_recon_tau, dim3(1), dim3(64), 0, st, (const double *) part, n, wiener, tau);
  hipLaunchKernelGGL(k_recon_estimate, dim3((unsigned) ((N * H + 255) / 256), (unsigned) N), dim3(256), 0, st, numV, denV,
                     (const double *) tau, N, H, tw);
  return hipGetLastError();
}

hipError_t bioem_recon_axis0_launch(hipStream_t st, const double2 *spec, int N, const double2 *tw, double2 *out)
{
  if (N < 2)
    return hipErrorInvalidValue;
  const int H = N / 2 + 1;
  const unsigned groups = (unsigned) ((N + kReconAxisOut - 1) / kReconAxisOut);
  hipLaunchKernelGGL(k_recon_axis0, dim3((unsigned) ((N * H + 255) / 256), groups), dim3(256), 0, st, spec, N, H, tw, out);
  return hipGetLastError();
}

hipError_t bioem_recon_correct_launch(hipStream_t st, const double *map, int N, const double *sinc2, int correct, float *vol)
{
  if (N < 2)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_recon_correct, dim3((unsigned) ((N * N + 255) / 256), (unsigned) N), dim3(256), 0, st, map, N, sinc2,
                     correct, vol);
  return hipGetLastError();
}
