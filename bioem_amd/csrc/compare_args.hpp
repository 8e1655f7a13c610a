// compare_args.hpp -- argument block shared by the comparison kernels
// Part of libbioem_hip.so; included by bioem_hip.hip and by every kernels_*.hip unit of a comparison family (anonymous
// namespace).
#ifndef BIOEM_COMPARE_ARGS_HPP
#define BIOEM_COMPARE_ARGS_HPP

namespace
{

struct CompareArgs
{
  const float2 *ref;  // [nMaps][M] comparison layout
  const float2 *conv; // [nOC][M]
  const bioem_hip_param5 *params;
  const double2 *postc; // [nOC] {t2, prior} of logpro_consts, evaluated once per row by k_posterior_consts
  const float *sumRef, *sumsqRef;
  const float2 *tw; // N+1
  const int *disp;  // nd
  const double2 *ltab; // 64 x {c, -log c}
  const float2 *twk;   // [N1][2*WD+1] recombination twiddles exp(2 pi i d k1 / N), d = -WD..WD
  const float2 *twnyq; // [N/2][2*WD+1][2] twiddles of k_nyquist_rows (wave-uniform reads: wide scalar loads)
  const float *btab;   // k_compare_fastm2: B operand of the matrix pass, [column pass][16][3][64] (fastm2_btab_floats)
  float *tnyq;         // [nMaps][ldPart][2*WD+1] Nyquist-column rows (fast path with the Nyquist split only)
  Partial *partials; // [nMaps][ldPart]
  int ldPart;
  int N, H, N1, nd, maxD, nOC, nMaps, algo;
  int Hp; // row-pair pitch of ref / conv in 16-byte words: H ... H + 15 (comparison_pitch, bioem_hip.hip)
  int pchunk; // particles per block-order chunk of the fast kernel
  int gs;     // pixels per window row of the fast kernel (template GS)
  // window tiles (wide windows are covered by several launches over phase-shifted conv spectra): only the first
  // ndx rows (sorted order) and the first ndy lanes of the displacement list count; nd for an untiled launch
  int ndx, ndy;
  // k_compare_wide2: row stride of the LDS T block (float2 units); window half width of the k_nyquist_rows
  // instantiation that filled tnyq (its rows run -nyqWD..nyqWD)
  int ts, nyqWD;
  // k_compare_fast: the last column block holds at most 32 columns and its half-waves share them (compare_fast.hpp)
  int split;
  PD pd;
};

// The own-list pass (one orientation list per particle, bioem_hip_compare_own_orientations) runs k_compare_fast and
// k_nyquist_rows over a batch of rows whose particles differ: the same kernels, instantiated on an argument block that
// adds the mapping of the launch (the ARGS template parameter, compare_fast.hpp).
// One block-table entry per block: {particle, first row, end row, 0} -- at most four consecutive rows [first, end) of that
// particle's run in the batch (rows are indices into conv / params / postc / partials / tnyq of the launch)
typedef int __attribute__((ext_vector_type(4))) own_i32x4;
typedef const own_i32x4 __attribute__((address_space(4))) *const_int4_ptr;
struct OwnCompareArgs : CompareArgs
{
  const int4 *__restrict__ blocks; // the block table of the batch (own_block_table, bioem_hip.hip)
};
struct OwnNyquistArgs : CompareArgs
{
  // slotParticle[s] = particle of flat slot s; row oc of the launch is row row0 + oc of the flat order, nCTF rows a slot
  const int *__restrict__ slotParticle;
  int row0, nCTF;
};

// k_compare_fast, static 21-row window: the window pass over |dy| (window_accumulate_sym, compare_fast.hpp) reads
//   symtab[column pair kp][j] = {cos, sin (2 pi (2 kp) j gs / N), cos, sin (2 pi (2 kp + 1) j gs / N)},  j = |dy| / gs
// kSymEntries float4 per column pair (|dy| = 0..10 and one entry of zeros: the third lane group reads four entries as the
// others do), for the pairs of whole 64-column blocks.  The table lies BEHIND the N + 1 twiddles in CompareArgs::tw (the
// argument block stays as it is); a block keeps the slice of its current column block in the LDS.
constexpr int kSymEntries = 12;
constexpr int kSymSliceFloat2 = 32 * kSymEntries * 2; // float2 per column block
constexpr int kSymSliceBytes = kSymSliceFloat2 * 8;
// which instantiations k_compare_fast<WD, R, NYQ, GS> take that pass (the others keep window_accumulate): the 21-row
// kernels, except the register FFTs of 20, 30 and 32 points -- at the 168-register bound of three waves per SIMD already,
// they spill 1, 5 and 12...17 registers with the eighth accumulator and the table prefetch
constexpr bool sym_window_ok(int WD, int R, bool NYQ, int GS) { return WD == 10 && R <= 18; }
// first float2 of the table in CompareArgs::tw
__host__ __device__ constexpr int sym_table_offset(int N) { return (N + 2) & ~1; }
// head of the fast kernels' LDS: the twiddles, or -- a launch of the static window reads none -- the table slice
__host__ __device__ constexpr size_t fast_head_bytes(int N, bool sym)
{
  const size_t twBytes = (size_t) ((N + 2) & ~1) * 8;
  return sym && twBytes < (size_t) kSymSliceBytes ? (size_t) kSymSliceBytes : twBytes;
}

} // namespace

#endif
