// kernels_rings.hip -- the ring pass of bioem_hip_best_match_rings (ring_kernels.hpp) and its launcher
#define BIOEM_RING_TU 1
#include "ring_kernels.hpp"

namespace
{
const size_t kRingLdsBudget = 64 * 1024; // dynamic LDS a block may take without raising the kernel's limit

// the waves' ring tables of a block: in LDS where they fit (up to 682 rings, 964 pixels), else in global memory
bool ring_tables_global(int nRings) { return sizeof(double) * 3 * (size_t) nRings * kRingWaves > kRingLdsBudget; }
} // namespace

int bioem_ring_count(int N) { return N < 1 ? 0 : bioem_ring_index(N / 2, N / 2) + 1; }

// a block per 32 rows of an image, at most 32 blocks: a function of N alone.  Measured at 224^2, 1 000 records in batches
// of 64, one device: one block per image 3.2 ms for the ring pass, a block per 64 rows 1.6, per 32 rows 1.45, per 16
// rows 1.35 (profiles/best_rings_block_rows.txt); 32 keeps the partials and their fold half the size of 16
const int kRingBlockRows = 32;
int bioem_ring_splits(int N) { return std::max(1, std::min(32, (N + kRingBlockRows - 1) / kRingBlockRows)); }

size_t bioem_ring_scratch(int N, int nImg)
{
  const size_t T = 3 * (size_t) bioem_ring_count(N), S = (size_t) bioem_ring_splits(N);
  return (size_t) nImg * S * T * (kRingWaves + 1); // the waves' tables, when they live in global memory, and the partials
}

hipError_t bioem_ring_sums_launch(hipStream_t st, const float2 *specR, const float2 *specP, const float2 *ctf,
                                  const BioemRingRecord *rec, int nImg, int N, const double2 *tw, double *scratch,
                                  bioem_hip_ring_sums *out)
{
  if (N < 1 || nImg < 1)
    return hipErrorInvalidValue;
  const int H = N / 2 + 1, nRings = bioem_ring_count(N), S = bioem_ring_splits(N);
  const size_t T = 3 * (size_t) nRings;
  double *part = scratch, *gtab = scratch + (size_t) nImg * S * T;
  double *dst = S == 1 ? reinterpret_cast<double *>(out) : part;
  const dim3 grid((unsigned) ((size_t) nImg * S)), block(64 * kRingWaves);
  if (ring_tables_global(nRings))
    hipLaunchKernelGGL(k_ring_sums<true>, grid, block, 0, st, specR, specP, ctf, rec, N, H, nRings, S, tw, gtab, dst);
  else
    hipLaunchKernelGGL(k_ring_sums<false>, grid, block, sizeof(double) * T * kRingWaves, st, specR, specP, ctf, rec, N, H,
                       nRings, S, tw, gtab, dst);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || S == 1)
    return e;
  hipLaunchKernelGGL(k_ring_fold, dim3(nImg), dim3(256), 0, st, part, S, (int) T, reinterpret_cast<double *>(out));
  return hipGetLastError();
}
