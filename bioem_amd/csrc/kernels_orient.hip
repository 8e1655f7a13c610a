// kernels_orient.hip -- the two passes of bioem_hip_orientation_sums, the row pass of bioem_hip_orientation_occupancy
// (orient_kernels.hpp) and their launchers
#define BIOEM_ORIENT_TU 1
#include "orient_kernels.hpp"

static_assert(sizeof(BioemOrientMax) == 16 && sizeof(bioem_hip_orient_sums) == 17 * sizeof(double), "partial / result layout");
static_assert(sizeof(bioem_hip_orient_occ) == 6 * sizeof(double), "occupancy result layout");

namespace
{
int orient_chunks(int nO) { return (nO + kOrientChunk - 1) / kOrientChunk; }
} // namespace

size_t bioem_orient_scratch(int nO, int np)
{
  // [chunks][np] maxima (two doubles each), [chunks][kOrientSums][np] sums, [np] folded maxima
  return (size_t) orient_chunks(nO) * (size_t) np * (2 + kOrientSums) + (size_t) np;
}

hipError_t bioem_orient_products_launch(hipStream_t st, const float4 *angles, int n, double *qq)
{
  if (n < 1)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_orient_products, dim3((n + 255) / 256), dim3(256), 0, st, angles, n, qq);
  return hipGetLastError();
}

hipError_t bioem_orient_sums_launch(hipStream_t st, const bioem_hip_prob_angle *pang, int nO, int nMaps, int p0, int np, int o0,
                                    const double *prior, const double *qq, const float4 *ownAngles, const int *ownOff,
                                    int ownIsQuat, double *scratch, bioem_hip_orient_sums *out)
{
  const int nC = orient_chunks(nO);
  if (nO < 1 || np < 1 || p0 < 0 || p0 + np > nMaps || nC > 65535)
    return hipErrorInvalidValue;
  BioemOrientMax *pmax = reinterpret_cast<BioemOrientMax *>(scratch);
  double *psum = scratch + (size_t) nC * np * 2;
  double *gmax = psum + (size_t) nC * np * kOrientSums;
  const bool own = ownOff != nullptr;
  const int moments = own ? (ownIsQuat != 0) : (qq != nullptr);
  const dim3 grid((np + 63) / 64, nC), block(64), fgrid((np + 255) / 256), fblock(256);
  hipLaunchKernelGGL(k_orient_max, grid, block, 0, st, pang, nO, nMaps, p0, np, own ? nullptr : prior, ownOff, pmax);
  hipLaunchKernelGGL(k_orient_fold<false>, fgrid, fblock, 0, st, (const void *) pmax, nC, np, o0, moments, gmax, out);
  if (own)
    hipLaunchKernelGGL(k_orient_sums<true>, grid, block, 0, st, pang, nO, nMaps, p0, np, (const double *) nullptr,
                       (const double *) nullptr, ownAngles, ownOff, moments, (const double *) gmax, psum);
  else
    hipLaunchKernelGGL(k_orient_sums<false>, grid, block, 0, st, pang, nO, nMaps, p0, np, prior, qq, (const float4 *) nullptr,
                       (const int *) nullptr, moments, (const double *) gmax, psum);
  hipLaunchKernelGGL(k_orient_fold<true>, fgrid, fblock, 0, st, (const void *) psum, nC, np, o0, moments, gmax, out);
  return hipGetLastError();
}

hipError_t bioem_orient_occ_launch(hipStream_t st, const bioem_hip_prob_angle *pang, int nO, int nMaps, int p0, int np, int o0,
                                   const double *prior, const double *m, const double *rS0, const int *omax,
                                   bioem_hip_orient_occ *out)
{
  if (nO < 1 || np < 1 || p0 < 0 || p0 + np > nMaps)
    return hipErrorInvalidValue;
  const int rowsPerBlock = kOccWaves * kOccRows;
  hipLaunchKernelGGL(k_orient_occ, dim3((nO + rowsPerBlock - 1) / rowsPerBlock), dim3(64 * kOccWaves), 0, st, pang, nO, nMaps,
                     p0, np, o0, prior, m, rS0, omax, out);
  return hipGetLastError();
}
