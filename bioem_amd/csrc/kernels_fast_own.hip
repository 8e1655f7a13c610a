// kernels_fast_own.hip -- k_compare_fast on OwnCompareArgs ("k_compare_fast_own<...>" in the API's labels): the K_FAST
// lines of kernel_table.inc once more, with the block order of the own-list pass (compare_fast.hpp), and the
// k_nyquist_rows on OwnNyquistArgs ("k_nyquist_rows_own<WD>") that go with them
#include "engine_types.hpp"
#include "posterior.hpp"
#include "fft_registers.hpp"
#include "compare_args.hpp"
#include "compare_fast.hpp"

namespace
{
// Own instantiations that are left out (they spill, use scratch or fail `make check`): such a shape keeps the
// per-particle launches -- a missing kernel costs speed, never correctness.  None at present.
constexpr bool own_left_out(int WD, int R, bool NYQ, int GS) { return false; }

template <int WD, int R, bool NYQ, int GS>
const void *own_kernel()
{
  if constexpr (own_left_out(WD, R, NYQ, GS))
    return nullptr;
  else
    return reinterpret_cast<const void *>(k_compare_fast<WD, R, NYQ, GS, OwnCompareArgs>);
}

// the lean variant of an own instantiation (compare_fast.hpp), where both exist
template <int WD, int R, bool NYQ, int GS>
const void *own_lean_kernel()
{
  if constexpr (own_left_out(WD, R, NYQ, GS))
    return nullptr;
  else
    return fast_lean_kernel<WD, R, NYQ, GS, OwnCompareArgs>();
}
} // namespace

// every line twice, as in kernels_fast.hip: a[4] = 1 holds the lean variant or a null stub
#define K_FAST(WD, R, NYQ, GS)                                                                                          \
  {KF_FAST, {WD, R, NYQ, GS, 0, 0}, own_kernel<WD, R, NYQ, GS>()},                                                      \
      {KF_FAST, {WD, R, NYQ, GS, 1, 0}, own_lean_kernel<WD, R, NYQ, GS>()},
#define BIOEM_FAMILY_FN bioem_kernels_fast_own
#include "kernels_family.inc"

// the Nyquist-column kernel of a k_compare_fast<WD, ..., OwnCompareArgs> launch (windows of 11 and 21 rows)
const void *bioem_nyquist_rows_own(int WD)
{
  switch (WD)
  {
  case 5: return reinterpret_cast<const void *>(k_nyquist_rows<5, 4, OwnNyquistArgs>);
  case 10: return reinterpret_cast<const void *>(k_nyquist_rows<10, 4, OwnNyquistArgs>);
  default: return nullptr;
  }
}
