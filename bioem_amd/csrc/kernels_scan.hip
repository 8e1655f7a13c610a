// kernels_scan.hip -- the CTF scan of bioem_hip_ctf_scan (scan_kernels.hpp) and its launchers
#define BIOEM_SCAN_TU 1
#include "scan_kernels.hpp"

hipError_t bioem_scan_pack_launch(hipStream_t st, const float2 *kernels, int nG, int N, float2 *packedChunk)
{
  if (N < 2 || nG < 1 || nG > kScanLanes)
    return hipErrorInvalidValue;
  const int H = N / 2 + 1;
  const size_t M = (size_t) N * H;
  hipLaunchKernelGGL(k_scan_pack, dim3((unsigned) ((M + 63) / 64)), dim3(256), 0, st, kernels, nG, N, H, packedChunk);
  return hipGetLastError();
}

hipError_t bioem_scan_prep_launch(hipStream_t st, const float2 *proj, const float2 *ref, const BioemScanShift *shift, int n,
                                  int N, const double2 *tw, float2 *Pw, double2 *Z)
{
  if (N < 2 || n < 1)
    return hipErrorInvalidValue;
  const int H = N / 2 + 1;
  const size_t M = (size_t) N * H;
  const unsigned blocks = (unsigned) std::min<size_t>(64, (M + 255) / 256);
  hipLaunchKernelGGL(k_scan_prep, dim3(blocks, (unsigned) n), dim3(256), 0, st, proj, ref, shift, N, H, tw, Pw, Z);
  return hipGetLastError();
}

hipError_t bioem_scan_launch(hipStream_t st, const float2 *packed, const float *ctfParam, int G, const float2 *Pw,
                             const double2 *Z, const BioemWindowRecord *rec, const float *sumRef, const float *sumsqRef,
                             const bioem_hip_param_device &pd, int n, int N, double *logp, float *cc,
                             bioem_hip_param5 *params)
{
  if (N < 2 || n < 1 || G < 1)
    return hipErrorInvalidValue;
  const dim3 grid((unsigned) ((G + kScanLanes - 1) / kScanLanes), (unsigned) ((n + kScanRecords - 1) / kScanRecords));
  hipLaunchKernelGGL(k_ctf_scan<kScanRecords>, grid, dim3(64), 0, st, packed, ctfParam, G, Pw, Z, rec, sumRef, sumsqRef, pd,
                     n, N, N / 2 + 1, logp, cc, params);
  return hipGetLastError();
}
