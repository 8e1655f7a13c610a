// bioem_hip.hip -- MI355X (gfx950 / CDNA4) implementation of the BioEM compare path behind the
// C ABI of include/bioem_hip.h.  Hand-written HIP, wave64, no vendor FFT/BLAS on the hot path.
//
// Hot path (replaces bioem_cuda::compareRefMaps + cuFFT, /root/reference/bioem_cuda.cu:527-684, and the
// host-side createProjection / createConvolutedProjectionMap, /root/reference/bioem.cpp:1604-1923):
//
//   prep_kernels.hpp     k_project_stamps, k_project_box  model points -> real-space projection: the spheres' footprints
//                          tabulated once per model, one block per orientation with the box of pixels the model can reach
//                          in LDS (ds_add_f64), the box stored; k_project_coords + k_project_bands (records, bands of map
//                          rows in LDS) for models beyond the box, k_project (global double atomics) beyond 426 pixels
//                        k_convolve       proj * conj(CTF) -> conv spectra in the comparison layout, sumC, Parseval terms
//                        k_parseval_ordered  sumsquareC: the reference's sequential float sum, four chains per wave
//                        k_convolve_sums  the two in one kernel (256 particles or fewer), 3...4 orientations per block
//                        k_dft_rows/cols  r2c by exact DFT on the vector units (images beyond 304 pixels)
//   r2c_fft.hpp          k_r2c_fft        r2c of the projections and particle maps (kernels_r2c.hip): one Cooley-Tukey split,
//                          register FFTs of 2...20 points in double; the rows of the projection's box only
//   dft_mfma.hpp         k_dft_rows_mfma / k_dft_cols_mfma  the r2c of image sizes with a prime factor above 19: exact DFT
//                          (double accumulation) as v_mfma_f64_16x16x4_f64 products
//                        k_reorder, k_map_sums: particle-side precompute
//   compare_fast.hpp     k_compare_fast   windows of at most 21 rows; one WAVE per (particle, orientation*CTF) comparison:
//                          spectrum product -> pruned inverse 2-D transform -> displacement-window log posterior
//                          -> wave log-sum-exp/arg-max partial.  The length-N inverse along kx is split as
//                          N = N1*R (R = 32, 16, 8, 4, 2 or a mixed length): N1 register-resident R-point FFTs per
//                          frequency column (lane = column, fft_registers.hpp), recombined only for the window rows that
//                          are consumed (output pruning), so no radix-7 butterfly is ever needed for N = 224.  The
//                          transform along ky is a pruned real DFT evaluated from LDS for the window only.
//                        k_nyquist_rows   the Nyquist column of 128^2 / 256^2 by direct summation
//                        both also on OwnCompareArgs / OwnNyquistArgs (compare_args.hpp; kernels_fast_own.hip): the same
//                          kernels with a block table, one launch per batch of the own-list pass ("k_compare_fast_own",
//                          "k_nyquist_rows_own" in the plan's labels); the other families: one launch per particle
//                        posterior_batch  the log posterior of a batch of displacements (all comparison kernels)
//   compare_fastm.hpp    k_compare_fastm  27- / 31-row windows: the same column pass, the window pass as one 32 x 32 tile of
//                          v_mfma_f32_32x32x2_f32 (exact f32) per comparison on the matrix cores
//   compare_wide2.hpp    k_compare_wide2  wide windows (32..128 rows): four or eight waves per comparison share the
//                          column transforms through LDS, row FFT over row pairs
//   compare_rows.hpp     k_compare_oddfft / k_compare_rows  odd image sizes: register FFT of odd length (3..25) over the
//                          reference layout, or direct column sums when N has no factor 3 or 5
//   compare_generic.hpp  k_compare_generic  same maths by direct pruned DFT (irregular wide displacement sets, N < 8)
//   compare_direct.hpp   k_c2r_cols/rows, k_compare_direct  BIOEM_CC_DIRECT=1 (BASELINE config 4): the cross-correlation as a
//                          sliding window in real space on the f32 matrix cores, no transform of the product
//   window_tiles.hpp     k_phase_shift, k_merge_tiles  wide windows no kernel covers: tiles of a window kernel
//   kernel_select.hpp    kernel table, k_compare_wide2 rules, plan_kernels: which kernel runs which shape
//   posterior.hpp        calc_logpro / calProb semantics (bioem_algorithm.h:18-142)
//   fold_kernels.hpp     k_fold_wave, k_fold_angles: fold the per-comparison partials into the probability block in the
//                          reference's (orientation, CTF) order (bioem_algorithm.h:96-123, bioem.cpp:1527-1600)
//                        k_fold_own, k_fold_own_angles: the same for the own-list pass (one orientation list per particle,
//                          of any length: bioem_hip_compare_own_orientations)
//                        k_fold_ctf, k_fold_own_ctf: the posterior per (CTF set, particle), a second fold of the same
//                          partials into the [nCTF][nMaps] table of bioem_hip_enable_ctf_table (off by default)
//   render_kernels.hpp   k_render_gather, k_render_cols, k_render_rows  bioem_hip_render_best_maps: the calculated image of
//                          every particle's best-match record (bioem.cpp:1925-2085), the full c2r by exact DFT in double
//   ring_kernels.hpp     k_ring_sums, k_ring_fold  bioem_hip_best_match_rings: per Fourier ring the sums of particle x best
//                          match, particle power and best-match power (kernels_rings.hip; declarations only here)
//   view_kernels.hpp     k_view_accumulate, k_view_tau, k_view_wiener  bioem_hip_view_sums / _view_averages: the aligned,
//                          CTF-weighted average of the particles of a view (kernels_views.hip; declarations only here)
//   window_kernels.hpp   k_window_prep, k_window_cols, k_window_cells  bioem_hip_window_posterior: the log posterior of every
//                          cell of the displacement window of a (particle, orientation, CTF) request (kernels_window.hip;
//                          declarations only here)
//   scan_kernels.hpp     k_scan_pack, k_scan_prep, k_ctf_scan  bioem_hip_ctf_scan: the log posterior of a (particle,
//                          orientation, shift) request under every CTF set of a list, lane = candidate (kernels_scan.hip;
//                          declarations only here)
//   grad_kernels.hpp     k_grad_coef, k_grad_spectrum, k_grad_cols, k_grad_rows, k_grad_gather, k_grad_norm, k_grad_fold
//                          bioem_hip_model_gradient: the derivative of a request's log posterior with respect to the
//                          density of every model point (kernels_grad.hip; declarations only here)
//   recon_kernels.hpp    k_recon_matrices, k_recon_insert, k_recon_tau_part, k_recon_tau, k_recon_estimate, k_recon_axis0,
//                          k_recon_correct  bioem_hip_reconstruct: the view sums gathered into a 3D Fourier volume, its
//                          estimate and real-space volume (kernels_recon.hip; declarations only here)
//   slice_kernels.hpp    k_slice_axis, k_slice_centre, k_slice_project  a volume as the model: its padded, centred spectrum
//                          and the central slices that stand in for projection + r2c (kernels_slice.hip; declarations
//                          only here)
//   pose_kernels.hpp     k_pose_partials, k_pose_fold  bioem_hip_pose_gradient: the derivative of a request's log posterior
//                          with respect to the orientation matrix and the model shifts of a volume model (kernels_pose.hip;
//                          declarations only here)
//   ctfgrad_kernels.hpp  k_ctfgrad_partials, k_ctfgrad_fold, k_ctfgrad_finish  bioem_hip_ctf_gradient: gradient and curvature
//                          of a request's log posterior with respect to the CTF triple of its set (kernels_ctfgrad.hip;
//                          declarations only here)
//   soft_kernels.hpp     k_soft_cols, k_soft_rows, k_soft_accumulate  bioem_hip_view_sums_soft / _reconstruct_soft: the view
//                          sums under a table of weighted shifts per (particle, group, CTF set) (kernels_soft.hip;
//                          declarations only here)
//   orient_kernels.hpp   k_orient_max, k_orient_sums, k_orient_fold, k_orient_products  bioem_hip_orientation_sums: the
//                          orientation posterior of every particle reduced where the angle table lives
//                          (kernels_orient.hip; declarations only here); k_orient_occ  bioem_hip_orientation_occupancy:
//                          the same table reduced along the particles, per orientation
//   this file            device context, launch logic, the C ABI
//   kernels_*.hip        one translation unit per comparison-kernel family (the instantiations of kernel_table.inc),
//                          linked into the same library: kernels_fast, kernels_fastm, kernels_wide2_{short,16,long},
//                          kernels_odd; kernels_r2c: the fast r2c; this file keeps the generic kernel, the preparation,
//                          fold and merge kernels
//
// Numerics: float expressions that the reference evaluates in float are written in the same order and the
// file is compiled with -ffp-contract=off (FMAs only where fmaf() is spelled out).  Sums that the reference
// accumulates sequentially in float (sumsquareC, particle sums) are accumulated in the same order.
#define BIOEM_MAIN_TU 1 // the non-template kernels shared headers hold (k_posterior_consts) are compiled here only
#include "engine_types.hpp"

#include <rccl/rccl.h> // types only: the library itself is loaded on the first bioem_hip_merge (dlopen)

#include <dlfcn.h>

#include <map>
#include <memory>
#include <mutex>
#include <queue>
#include <string>
#include <vector>

namespace
{

// ------------------------------------------------------------------------------------------------
// error handling
// ------------------------------------------------------------------------------------------------
struct HipErr
{
  std::string msg;
};

#define HIP_CHECK(h, expr)                                                                                         \
  do                                                                                                               \
  {                                                                                                                \
    hipError_t e_ = (expr);                                                                                        \
    if (e_ != hipSuccess)                                                                                          \
    {                                                                                                              \
      char buf_[512];                                                                                              \
      snprintf(buf_, sizeof(buf_), "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__);     \
      (h)->err = buf_;                                                                                             \
      return 1;                                                                                                    \
    }                                                                                                              \
  } while (0)

} // namespace

#include "prep_kernels.hpp"
#include "dft_mfma.hpp"
#include "posterior.hpp"
#include "fft_registers.hpp"
#include "compare_args.hpp"
#include "compare_fast.hpp"
#include "compare_wide2.hpp"
#include "compare_fastm.hpp"
#include "compare_fastm2.hpp"
#include "compare_generic.hpp"
#include "compare_rows.hpp"
#include "compare_direct.hpp"
#include "kernel_select.hpp"
#include "fold_kernels.hpp"
#include "window_tiles.hpp"
#include "render_kernels.hpp"
#include "ring_kernels.hpp"
#include "view_kernels.hpp"
#include "window_kernels.hpp"
#include "scan_kernels.hpp"
#include "grad_kernels.hpp"
#include "recon_kernels.hpp"
#include "slice_kernels.hpp"
#include "vgrad_kernels.hpp"
#include "pose_kernels.hpp"
#include "ctfgrad_kernels.hpp"
#include "soft_kernels.hpp"
#include "orient_kernels.hpp"

struct bioem_hip_ctx
{
  int device = 0;
  hipStream_t stream = nullptr;
  PD pd;
  int nMaps = 0, nAngles = 0, nCTF = 0, algo = 1;
  int N = 0, H = 0, M = 0;
  int Hp = 0;    // row-pair pitch of the comparison layout in 16-byte words (H ... H + 15: comparison_pitch)
  size_t Mc = 0; // float2 per image of the comparison layout, N * Hp
  KernelPlan plan; // which comparison kernel runs this shape and how (kernel_select.hpp)
  int pchunk = 128;               // particle chunk of the fast kernel's block order (0 = all particles); measured:
                                  // 1 000 particles 6.73 -> 6.56 ms, 10 000 particles (2 GB, beyond the Infinity
                                  // Cache) 78.5 -> 63.2 ms per launch
  int *dDispLocal = nullptr, *dTileCenter = nullptr, *dTileValid = nullptr, *dRankOfRow = nullptr;
  float *dBtab = nullptr;  // k_compare_fastm2: tabulated B operand of the matrix pass
  float2 *dConvShift = nullptr;
  Partial *dPartTiles = nullptr;
  int OB = 0;     // orientations per batch of the native path
  int maxOC = 0;  // capacity of conv/param/partial buffers in (orientation*CTF) units
  int chunkB = 0; // images per DFT chunk

  float2 *dRef = nullptr;
  float *dSumRef = nullptr, *dSumsqRef = nullptr;
  float2 *dCTF = nullptr;
  float *dCtfParam = nullptr;
  bioem_hip_model_point *dPts = nullptr;
  double *dStamp = nullptr; // sphere footprints of the model (k_project_stamps), (2 iradMax + 1)^2 doubles per point
  double modelRadius = 0.;  // max |point| of the model, Angstrom (k_project_box)
  double quatNormDev = 0.;  // max | |q|^2 - 1 | over the uploaded quaternions (0 for Euler angles: always rotations)
  int nPts = 0;
  float NormDen = 0, pixelSize = 0;
  int shiftX = 0, shiftY = 0;
  // a volume as the model (bioem_hip_upload_model_volume / _spectrum; slice_kernels.hpp): the centred spectrum C
  // [PN][PN][PH], PN = volPad N; null with a point model -- a handle holds one kind, an upload replaces the other
  double2 *dVolC = nullptr;
  int volPad = 0;
  // what the upload was given, for the transpose of its passes (bioem_hip_volume_gradient): the centre, the flag word and
  // whether the model came as a spectrum
  double volCentre[3] = {0., 0., 0.};
  int volFlags = 0;
  bool volFromSpectrum = false;
  // bioem_hip_volume_gradient / _debug_volume_backproject / _debug_volume_adjoint (vgrad_kernels.hpp): A beside C (volAPad:
  // the padding it is sized for), the matrices, view parameters and flags of a launch of the scan, Y and the double slices
  // of a batch (allocated at the first call)
  double2 *dVolA = nullptr, *dVgY = nullptr, *dVgSlices = nullptr;
  double *dPosePart = nullptr, *dPoseRows = nullptr; // bioem_hip_pose_gradient (pose_kernels.hpp): a batch's partial sums, a launch's rows
  // bioem_hip_ctf_gradient (ctfgrad_kernels.hpp): a batch's partial sums, a launch's sums and rows; the host's row map and
  // table of the radial variable for ctfgPixel (0: none yet); a batch's triples and derivatives of the debug entry
  double *dCtfgPart = nullptr, *dCtfgSums = nullptr, *dCtfgRows = nullptr, *dCtfgDerivs = nullptr;
  int *dCtfgRowIdx = nullptr;
  float *dCtfgRadsq = nullptr, *dCtfgTheta = nullptr;
  float ctfgPixel = 0.f;
  int volAPad = 0;
  double *dVgR = nullptr, *dVgView = nullptr;
  int *dVgFlag = nullptr;
  // bioem_hip_debug_slices: angles, matrices and slices of a chunk of maxOrientations (allocated at the first call)
  float4 *dSliceAngles = nullptr;
  double *dSliceR = nullptr;
  double2 *dSliceOut = nullptr;
  int iradMax = 0; // widest sphere footprint of the model, pixels (k_project_bands)
  // BIOEM_CC_DIRECT=1 (BASELINE config 4): real-space particles, real-space conv maps of a launch, column pass of the c2r
  bool direct = false;
  float *dMapsReal = nullptr, *dConvReal = nullptr;
  double2 *dDirectZ = nullptr;
  int nCU = 256;   // compute units of the device: size of the resident grids of the preparation kernels
  float4 *dAngles = nullptr;
  int nAnglesUp = 0, isQuat = 1;
  // one orientation list per particle (bioem_hip_upload_particle_orientation_lists, bioem_hip_compare_own_orientations):
  // particle p owns the flat slots ownOff[p] ... ownOff[p + 1]; the all-to-all entries never read this state
  float4 *dOwnAngles = nullptr;        // [slots]
  int *dOwnOff = nullptr;              // [nMaps + 1], ownOff on the device
  int *dSlotParticle = nullptr;        // [slots] particle of a slot
  size_t ownSlotCap = 0;               // slots dOwnAngles / dSlotParticle hold
  std::vector<int> ownOff;             // empty: no lists
  int ownK = 0, ownIsQuat = 1;         // ownK: the longest list
  double ownQuatNormDev = 0.;
  int ownOB = 0;                       // slots (particle, list entry) per batch of the own-list pass
  // the comparison of a batch as ONE launch (k_compare_fast on OwnCompareArgs: plans of k_compare_fast, where
  // bioem_hip_set_own_launch asked for it; ownFnPlan: the plan's own kernel, ownFn: the one in use or null), else one
  // launch of the plan's kernel per particle, the default.  Block table of the batches of particles [ownTabP0, ownTabP1):
  // batch b begins at slot ownTabSlot[b] and owns entries ownTabFirst[b] ... ownTabFirst[b + 1] of dOwnBlocks
  own_kernel_t ownFn = nullptr, ownFnPlan = nullptr;
  own_kernel_t ownFnPlanLean = nullptr; // the lean variant of ownFnPlan, or null (compare_fast.hpp)
  bool lean = true;                     // bioem_hip_set_compare_variant: lean instantiations where a launch qualifies
  nyq_own_kernel_t ownNyqFn = nullptr;
  bool ownXcdOrder = true;
  int4 *dOwnBlocks = nullptr;
  size_t ownBlockCap = 0;
  int ownTabP0 = -1, ownTabP1 = -1;
  std::vector<int> ownTabSlot, ownTabFirst;
  size_t slotImages[2] = {0, 0};       // images the projection buffers of a pipeline slot hold
  size_t slotRows = 0, partRows = 0;   // rows the conv / params / postc buffers of a slot and dPartials (dTnyq) hold
  float2 *dTw = nullptr;   // N+1 entries exp(+2 pi i k/N), float
  double2 *dTwD = nullptr; // N entries, double
  int *dDisp = nullptr;
  double2 *dLtab = nullptr;
  float2 *dTwk = nullptr;   // recombination twiddles exp(2 pi i dx k1 / N) of the comparison kernel, laid out per family
  float2 *dTwNyq = nullptr; // [N/2 row pairs][2*nyqWD+1][2] twiddles of the Nyquist pre-kernel (nyq only)
  float *dTnyq = nullptr; // [nMaps][maxOC][2*nyqWD+1] Nyquist-column rows of the current launch (nyq only)
  Partial *dPartials = nullptr; // [nMaps][maxOC]
  unsigned char *dProb = nullptr;
  size_t probBytes = 0;    // bytes start_run / finish_run move (shard handles: the map entries only)
  size_t devProbBytes = 0; // device block: map entries + the angle table of the owned orientations
  bool shard = false;      // created by bioem_hip_create_shard
  int angO0 = 0, angO1 = 0; // orientations whose angle entries this handle holds ([0, nAngles) unless a shard)
  bioem_hip_angle_candidate *dCand = nullptr; // [nMaps][candK] result of the last top-K selection
  int candK = 0;
  unsigned char *dSend = nullptr, *dRecv = nullptr; // RCCL merge buffers
  size_t sendBytes = 0, recvBytes = 0;
  bioem_hip_prob_map *dMerged = nullptr;
  // bioem_hip_render_best_maps: the records, gathered orientations and maps of one batch (allocated at the first call)
  RenderRecord *dRenderRec = nullptr;
  float4 *dRenderAngles = nullptr;
  float *dRenderOut = nullptr;
  // bioem_hip_best_match_rings / bioem_hip_debug_ring_sums: particle spectra of a batch in reference layout, the scratch of
  // the ring pass and its result (allocated at the first call)
  RenderRecord *dRingRec = nullptr;
  float4 *dRingAngles = nullptr;
  float2 *dRingRef = nullptr;
  double *dRingScratch = nullptr;
  bioem_hip_ring_sums *dRingOut = nullptr;
  // bioem_hip_view_sums / _view_averages / _debug_view_sums: the accumulators of a chunk of groups, their Wiener constants,
  // the members and group offsets of a batch, a CTF buffer of 1 + 0i and the rendered maps (allocated at the first call)
  double2 *dViewNum = nullptr;
  double *dViewDen = nullptr, *dViewTau = nullptr;
  BioemViewMember *dViewMem = nullptr;
  int *dViewOff = nullptr;
  float2 *dViewUnit = nullptr;
  float *dViewMaps = nullptr;
  // bioem_hip_reconstruct / bioem_hip_debug_reconstruct: numV (then V^, then the column pass), denV (then the float
  // volume), the axis-0 pass (then the planes), the slots, orientations, angles and matrices of a chunk of views, the
  // partial sums of the mean, tau and the sinc^2 table (allocated at the first call)
  double2 *dReconNum = nullptr, *dReconWork = nullptr;
  double *dReconDen = nullptr, *dReconR = nullptr, *dReconPart = nullptr, *dReconTau = nullptr, *dReconSinc = nullptr;
  int *dReconSlot = nullptr, *dReconOrient = nullptr;
  float4 *dReconAngles = nullptr;
  // bioem_hip_view_sums_soft / _debug_view_sums_soft / _reconstruct_soft: the tables, U, W and members of a launch of at
  // most maxOrientations members, the shifts mod N and the twiddles, exact at the multiples of a quarter turn (allocated at
  // the first call, grown with the tables: softNd)
  double *dSoftCells = nullptr;
  double2 *dSoftU = nullptr, *dSoftW = nullptr, *dSoftTw = nullptr;
  BioemSoftMember *dSoftMem = nullptr;
  int *dSoftXm = nullptr;
  int softNd = 0;
  // bioem_hip_window_posterior / bioem_hip_debug_window: a batch's records, gathered orientations, particle and conv
  // spectra in reference layout, Parseval terms, parameters, particle sums handed in, the scratch T of the window pass,
  // the window's shifts in ascending order and the results (allocated at the first call)
  BioemWindowRecord *dWinRec = nullptr;
  float4 *dWinAngles = nullptr;
  float2 *dWinRef = nullptr, *dWinConv = nullptr;
  float *dWinTerms = nullptr, *dWinSums = nullptr, *dWinCc = nullptr;
  bioem_hip_param5 *dWinParams = nullptr;
  double2 *dWinPostc = nullptr, *dWinT = nullptr;
  int *dWinShifts = nullptr;
  double *dWinLogp = nullptr;
  // bioem_hip_ctf_scan / bioem_hip_debug_ctf_scan: a batch's shifts; the records, projections and Z in walk order and the
  // sums handed in of the batches one scan launch serves (scan_capacity) and one chunk of candidates as handed in
  // (allocated at the first call, with the window staging the entry shares); the packed candidates, their parameters
  // and the results (grown to the largest G asked for)
  BioemScanShift *dScanShift = nullptr;
  BioemWindowRecord *dScanRec = nullptr;
  float2 *dScanPw = nullptr, *dScanRaw = nullptr, *dScanPacked = nullptr;
  double2 *dScanZ = nullptr;
  float *dScanCtf = nullptr, *dScanCc = nullptr, *dScanSums = nullptr;
  double *dScanLogp = nullptr;
  bioem_hip_param5 *dScanParams = nullptr;
  int scanCapG = 0;
  // bioem_hip_model_gradient / bioem_hip_debug_grad_image / _gather: a batch's records, coefficients {a, b, g, m}, weights,
  // {m, T}, parameters, gradient spectra and maps (allocated at the first call, with the scan staging the entry shares);
  // u, v sigma, the tiles' partial sums and the rows of a batch and the sums per point (grown to the largest model)
  BioemGradRecord *dGradRec = nullptr;
  double *dGradCoef = nullptr, *dGradW = nullptr, *dGradMT = nullptr, *dGradMap = nullptr;
  bioem_hip_param5 *dGradParams = nullptr;
  double2 *dGradSpec = nullptr;
  float4 *dGradAngles = nullptr;
  double *dGradU = nullptr, *dGradVS = nullptr, *dGradPart = nullptr, *dGradRows = nullptr;
  bioem_hip_grad_point *dGradAcc = nullptr;
  int gradCapPts = 0;
  // bioem_hip_orientation_sums: scratch of the two passes, the products q_i q_j of the owned orientations, their priors
  // and the result (allocated at the first call)
  double *dOrientScratch = nullptr, *dOrientQQ = nullptr, *dOrientPrior = nullptr;
  bioem_hip_orient_sums *dOrientOut = nullptr;
  // bioem_hip_orientation_occupancy: the particles' normalisers m, 1 / S0, omax, the priors of the owned orientations and
  // the result (allocated at the first call)
  double *dOccM = nullptr, *dOccRS0 = nullptr, *dOccPrior = nullptr;
  int *dOccOmax = nullptr;
  bioem_hip_orient_occ *dOccOut = nullptr;
  bool refUp = false; // particles uploaded (either entry)
  bool ctfUp = false; // bioem_hip_upload_ctf has run
  // bioem_hip_enable_ctf_table: [nCTF][nMaps] entries, folded beside the particle entries (k_fold_ctf, k_fold_own_ctf);
  // null = off, nothing allocated and nothing launched
  bioem_hip_prob_map *dCtfTab = nullptr;
  bool inRun = false; // between start_run and finish_run

  // two pipeline slots + a second stream: projection/convolution of batch k+1 (prepStream) overlap the comparison of
  // batch k.  Slot 0's projection buffers also stage the particle uploads and the debug hooks.
  struct Slot
  {
    double *projReal = nullptr; // [images][N*N]
    double *tempDen = nullptr;  // [images]
    double2 *rowSpec = nullptr; // [images][N][H]
    float2 *specRef = nullptr;  // [images][M] reference layout
    float *scratch = nullptr;   // [maxOC][M] ordered |X|^2 terms for sumsquareC
    float2 *conv = nullptr;     // [maxOC][M] comparison layout
    bioem_hip_param5 *params = nullptr;
    double2 *postc = nullptr; // [maxOC] {t2, prior} of the log posterior per (orientation, CTF) row (k_posterior_consts)
    // staged device entries (bioem_hip_project / _convolve / _compare_device): what the slot holds
    int stageO0 = 0, stageNO = 0, stageC0 = 0, stageNC = 0;
    hipEvent_t prepDone = nullptr, cmpDone = nullptr;
    bool cmpPending = false;
  };
  Slot slot[2];
  hipStream_t prepStream = nullptr;

  // reference-compatible entry (bioem_hip_compare): the caller hands over a few conv spectra per call (ONE per call
  // in the reference's default ALGO-1 loop, bioem.cpp:534,811-853).  They are staged into a two-half ring -- pinned
  // host rows, H2D copies on their own stream -- and compared with ONE kernel launch per filled half (flush at
  // finish_run), folding in call order through a per-row (orientation, CTF) table.  Half k uses pipeline slot k
  // (conv, params, cmpDone).
  struct CompatHalf
  {
    float2 *hConv = nullptr;          // pinned [ringCap][M], reference layout
    bioem_hip_param5 *hPar = nullptr; // pinned [ringCap]
    int2 *hIds = nullptr;             // pinned [ringCap] {orientation, CTF}
    int4 *hSeg = nullptr;             // pinned [ringCap] runs of equal orientation {first row, end row, orientation, 0}
    float2 *dStage = nullptr;         // device [ringCap][M], reference layout
    int2 *dIds = nullptr;
    int4 *dSeg = nullptr;
    hipEvent_t staged = nullptr;      // H2D copies of this half done (copyStream)
  };
  CompatHalf ring[2];
  int ringCap = 0, ringHalf = 0, ringCount = 0;
  std::vector<int> ringOrients; // orientations with rows in the current half, in first-appearance order
  hipStream_t copyStream = nullptr;

  // every device and pinned-host allocation of the handle (dev_alloc, host_alloc): bioem_hip_destroy frees them
  struct Alloc
  {
    void *p;
    bool pinned;
  };
  std::vector<Alloc> allocs;

  // timing
  // per-batch phase records (bioem_hip_set_phase_timing): the reference's BIOEM_DEBUG_OUTPUT report (timer.cpp:138-165,
  // bioem.cpp:769-889) from HIP events on the streams the phases run on
  struct PhaseEvents
  {
    int phase, o0, o1, c0, c1;
    hipEvent_t a, b;
  };
  bool phaseTiming = false;
  std::vector<PhaseEvents> phasePending;
  std::vector<bioem_hip_phase_record> phaseDone;
  std::vector<hipEvent_t> evPool;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> evPending;
  double compareMs = 0;
  long long launches = 0, comparisons = 0;

  std::string err;
};

namespace
{

// ------------------------------------------------------------------------------------------------
// host helpers
// ------------------------------------------------------------------------------------------------
hipEvent_t get_event(bioem_hip_ctx *h)
{
  if (!h->evPool.empty())
  {
    hipEvent_t e = h->evPool.back();
    h->evPool.pop_back();
    return e;
  }
  hipEvent_t e;
  if (hipEventCreate(&e) != hipSuccess)
    return nullptr;
  return e;
}

void drain_events(bioem_hip_ctx *h)
{
  for (auto &pr : h->evPending)
  {
    float ms = 0.f;
    if (hipEventSynchronize(pr.second) == hipSuccess && hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess)
      h->compareMs += (double) ms;
    h->evPool.push_back(pr.first);
    h->evPool.push_back(pr.second);
  }
  h->evPending.clear();
}

// phase timing: an event pair around a phase of a batch on the stream it runs on (no-ops unless enabled)
int phase_begin(bioem_hip_ctx *h, hipStream_t st, int phase, int o0, int o1, int c0, int c1)
{
  if (!h->phaseTiming)
    return 0;
  bioem_hip_ctx::PhaseEvents e = {phase, o0, o1, c0, c1, get_event(h), get_event(h)};
  if (!e.a || !e.b)
  {
    h->err = "hipEventCreate failed";
    return 1;
  }
  HIP_CHECK(h, hipEventRecord(e.a, st));
  h->phasePending.push_back(e);
  return 0;
}

int phase_end(bioem_hip_ctx *h, hipStream_t st)
{
  if (!h->phaseTiming || h->phasePending.empty())
    return 0;
  HIP_CHECK(h, hipEventRecord(h->phasePending.back().b, st));
  return 0;
}

void drain_phases(bioem_hip_ctx *h)
{
  for (auto &e : h->phasePending)
  {
    float ms = 0.f;
    if (hipEventSynchronize(e.b) == hipSuccess && hipEventElapsedTime(&ms, e.a, e.b) == hipSuccess)
    {
      bioem_hip_phase_record r = {e.phase, e.o0, e.o1, e.c0, e.c1, (double) ms * 1e-3};
      h->phaseDone.push_back(r);
    }
    h->evPool.push_back(e.a);
    h->evPool.push_back(e.b);
  }
  h->phasePending.clear();
}

// allocations recorded on the handle (freed by bioem_hip_destroy)
template <class T>
int dev_alloc(bioem_hip_ctx *h, T *&p, size_t n)
{
  HIP_CHECK(h, hipMalloc(&p, sizeof(T) * n));
  if (p)
    h->allocs.push_back({p, false});
  return 0;
}
template <class T>
int host_alloc(bioem_hip_ctx *h, T *&p, size_t n)
{
  HIP_CHECK(h, hipHostMalloc(&p, sizeof(T) * n, hipHostMallocDefault));
  if (p)
    h->allocs.push_back({p, true});
  return 0;
}
// a device buffer that is replaced: freed now and dropped from the record
template <class T>
void dev_release(bioem_hip_ctx *h, T *&p)
{
  if (!p)
    return;
  for (size_t i = 0; i < h->allocs.size(); i++)
    if (h->allocs[i].p == p)
    {
      h->allocs.erase(h->allocs.begin() + i);
      break;
    }
  hipFree(p);
  p = nullptr;
}
// n host values into a new device buffer
template <class T>
int upload(bioem_hip_ctx *h, T *&p, const T *src, size_t n)
{
  if (dev_alloc(h, p, n))
    return 1;
  HIP_CHECK(h, hipMemcpy(p, src, sizeof(T) * n, hipMemcpyHostToDevice));
  return 0;
}

// exp(2 pi i ((a b) mod N) / N) for ab = a b: the one expression every twiddle table is built from
double2 twiddle_d(long long ab, int N)
{
  const double ang = 2.0 * M_PI * (double) ((ab % N + N) % N) / (double) N;
  return make_double2(cos(ang), sin(ang));
}
float2 twiddle(long long ab, int N)
{
  const double2 w = twiddle_d(ab, N);
  return make_float2((float) w.x, (float) w.y);
}

// the slot's buffers are written by something other than the staged entries: nothing is staged in it any more, and
// bioem_hip_convolve / bioem_hip_compare_device on it return 2 until bioem_hip_project fills it again
void void_slot(bioem_hip_ctx::Slot &s) { s.stageNO = s.stageNC = 0; }

// ids == nullptr: row oc of the launch is (orient0 + oc / convPerOrient, conv0 + oc % convPerOrient) (native path);
// otherwise ids[oc] = {orientation, CTF} and segs[0..nSeg) = runs of equal orientation (compat ring)
// the Nyquist column of the 64-column blocks (N / 2 a multiple of 64): its window rows by direct summation.  With 64
// particles or fewer four threads share a (particle, spectrum) pair (a block per 4 x 16 pairs), else one (16 x 16).
template <int Q>
void launch_nyquist_rows(bioem_hip_ctx *h, const CompareArgs &aw, int WD, int nOC)
{
  const int PB = 16 / Q;
  const dim3 gridq((unsigned) (((size_t) (aw.nMaps + PB - 1) / PB) * ((nOC + 15) / 16)));
  switch (WD)
  {
#define X(W)                                                                                                            \
  case W:                                                                                                               \
    hipLaunchKernelGGL((k_nyquist_rows<W, Q>), gridq, dim3(256), 0, h->stream, aw);                                     \
    break;
    X(5) X(10) X(13) X(15) X(20) X(31) X(42)
#undef X
  }
}
void launch_nyquist(bioem_hip_ctx *h, const CompareArgs &aw, int WD, int nOC)
{
  if (aw.nMaps <= 64)
    launch_nyquist_rows<4>(h, aw, WD, nOC);
  else
    launch_nyquist_rows<1>(h, aw, WD, nOC);
}

// Row-pair pitch, in 16-byte words, of the shapes the H + 15 rule (comparison_pitch, below) leaves alone: H rounded up to
// kPitchAlignWords.  A wave's operand request is 64 lanes x 16 B; the L1 takes it as 16 quads of 64 B and processes one
// access per 128-byte line a quad touches.  At pitch H (16 H bytes: 16-byte aligned, line aligned in every eighth row
// pair only) most quads straddle two lines, at a pitch that is a multiple of 4 words none does (8 848 against
// 6 496 modelled accesses per comparison at 224^2).  At most 15 words are added (debug_convolve_batch sizes for H + 15),
// and never a multiple of 32 words, i.e. 512 B: the channel aliasing the H + 15 rule exists to avoid.
// Measured, default against BIOEM_NO_PITCH_PAD=1 on one device (profiles/lean_operand_ab.txt): 224^2 -1.4 % launch time
// (H + 3 = 116 and H + 11 = 124, 64-byte multiples only, -0.8 % and -0.5 %), 240^2 -1.8 %, 200^2 -1.4 %, 160^2 -0.9 %, ten
// particles at 224^2 -1.5 %; 96^2 (one column block) +0.6 %: the rule starts at 160 pixels, the smallest size that gained.
constexpr int kPitchAlignWords = 8;
constexpr int kLinePitchMinN = 160;
int line_aligned_pitch(int N, int H)
{
  if (N < kLinePitchMinN)
    return H;
  int Hp = (H + kPitchAlignWords - 1) / kPitchAlignWords * kPitchAlignWords;
  if (Hp % 32 == 0)
    Hp += kPitchAlignWords;
  return Hp;
}

// k_compare_fast / k_compare_fastm: a last column block of at most 32 columns is shared by the half-waves
// (with the Nyquist split the blocks hold the H - 1 columns below N / 2: whole ones, or -- 192^2, 320^2, 448^2, which
// were planned that way -- a last one of 32, and then the split is not optional)
int last_block_split(const bioem_hip_ctx *h)
{
  const KernelPlan &P = h->plan;
  const int cols = P.nyq ? h->H - 1 : h->H;
  const int nblkF = (cols + 63) / 64, rem = cols - (nblkF - 1) * 64;
  return (P.family == KF_FAST || P.family == KF_FASTM) && rem <= 32 && P.N1 >= 2 && (P.nyq || !getenv("BIOEM_NO_SPLIT_LAST"));
}

// The lean variant of k_compare_fast is the full instantiation's static, unsplit path and nothing else (compare_fast.hpp):
// a launch takes it exactly where the kernel's own run-time tests would take that path -- the whole window of 2 winD + 1
// rows (symw) and no split last block -- and the handle's variant switch is on.  Decided per launch: `split` reads the
// environment every time, and a tile launch carries its own nd / maxD.
bool lean_launch_ok(const bioem_hip_ctx *h, int nd, int maxD, int split)
{
  const KernelPlan &P = h->plan;
  // (N1 halfR = N / 2 >= 6 row pairs: the lean loop's ring re-reads row pairs 0 .. 4 at the end of the last block)
  return h->lean && !h->direct && P.family == KF_FAST && P.fnLean && sym_window_ok(P.winD, 2 * P.halfR, P.nyq, P.gs) &&
         nd == 2 * P.winD + 1 && maxD / P.gs == P.winD && !split && P.N1 * P.halfR >= 6;
}
fast_kernel_t compare_fn(const bioem_hip_ctx *h, const CompareArgs &a)
{
  return lean_launch_ok(h, a.nd, a.maxD, a.split) ? h->plan.fnLean : h->plan.fn;
}

// argument block, grid and block of a comparison launch: the nOC conv rows of a slot against nMaps particles (the
// handle's, or ONE in the own-list pass, whose launches point ref / sumRef / sumsqRef at that particle)
CompareArgs compare_args(bioem_hip_ctx *h, const bioem_hip_ctx::Slot &bb, int nOC, int nMaps, dim3 &grid, dim3 &block)
{
  const KernelPlan &P = h->plan;
  const int fam = P.family;
  CompareArgs a;
  a.ref = h->dRef;
  a.conv = bb.conv;
  a.params = bb.params;
  a.postc = bb.postc;
  a.sumRef = h->dSumRef;
  a.sumsqRef = h->dSumsqRef;
  a.tw = h->dTw;
  a.disp = h->dDisp;
  a.ltab = h->dLtab;
  a.twk = h->dTwk;
  a.btab = h->dBtab;
  a.tnyq = h->dTnyq;
  a.twnyq = h->dTwNyq;
  a.partials = h->dPartials;
  a.ldPart = h->maxOC;
  a.N = h->N;
  a.H = h->H;
  a.Hp = h->Hp;
  a.N1 = P.N1;
  a.nd = P.nd;
  a.maxD = h->pd.maxDisplaceCenter;
  a.nOC = nOC;
  a.nMaps = nMaps;
  a.algo = h->algo;
  a.pd = h->pd;
  a.gs = P.gs;
  a.ndx = a.ndy = P.nd;
  a.nyqWD = P.nyqWD;
  a.split = last_block_split(h);
  a.pchunk = h->pchunk > 0 ? std::min(h->pchunk, nMaps) : nMaps;
  if (a.pchunk >= 8) // a multiple of 8: a particle then stays on one XCD (65 particles: chunks of 64 + 1, 43.6 -> 45.3 M/s)
    a.pchunk &= ~7;
  const int ocGroups = (nOC + 3) / 4;
  // few particles, k_compare_fast / _fastm / _fastm2: whole groups per XCD (fast_block_pair); the grid is padded to a
  // multiple of 8 groups (measured for 65...200 particles as well: 1-3 % slower than the chunk order there)
  const bool groupPerXcd = nMaps <= 64 && (fam == KF_FAST || fam == KF_FASTM || fam == KF_FASTM2);
  if (groupPerXcd)
    a.pchunk = -1;
  // launch geometry by family: four comparisons per 256-thread block, except k_compare_wide2 (one block of w2NW waves
  // per comparison) and k_compare_generic (genericWaves comparisons per block)
  grid = dim3((unsigned) ((size_t) (groupPerXcd ? (ocGroups + 7) / 8 * 8 : ocGroups) * nMaps));
  block = dim3(256);
  if (fam == KF_WIDE2)
  {
    a.ts = P.w2TS;
    grid = dim3((unsigned) ((size_t) nOC * nMaps));
    block = dim3(64 * P.w2NW);
  }
  else if (fam == KF_GENERIC)
  {
    a.ts = P.genericRows;
    grid = dim3((unsigned) ((size_t) ((nOC + P.genericWaves - 1) / P.genericWaves) * nMaps));
    block = dim3(64 * P.genericWaves);
  }
  return a;
}

int launch_compare_fold(bioem_hip_ctx *h, const bioem_hip_ctx::Slot &bb, int nOC, int orient0, int conv0,
                        int convPerOrient, const int2 *ids = nullptr, const int4 *segs = nullptr, int nSeg = 0)
{
  const KernelPlan &P = h->plan;
  dim3 grid, block;
  const CompareArgs a = compare_args(h, bb, nOC, h->nMaps, grid, block);
  auto launch = [&](const CompareArgs &aw) {
    if (P.nyq)
      launch_nyquist(h, aw, P.nyqWD, nOC);
    hipLaunchKernelGGL(compare_fn(h, aw), grid, block, P.ldsBytes, h->stream, aw);
  };
  hipEvent_t e0 = get_event(h), e1 = get_event(h);
  if (!e0 || !e1)
  {
    if (e0)
      h->evPool.push_back(e0);
    if (e1)
      h->evPool.push_back(e1);
    h->err = "hipEventCreate failed";
    return 1;
  }
  // {t2, prior} of every row of the launch, once per row instead of once per comparison and lane
  hipLaunchKernelGGL(k_posterior_consts, dim3((nOC + 63) / 64), dim3(64), 0, h->stream, bb.params, h->pd, bb.postc, nOC);
  HIP_CHECK(h, hipEventRecord(e0, h->stream));
  if (phase_begin(h, h->stream, BIOEM_HIP_PHASE_COMPARISON, ids ? -1 : orient0, ids ? -1 : orient0 + (nOC + convPerOrient - 1) / convPerOrient,
                  ids ? -1 : conv0, ids ? -1 : conv0 + convPerOrient))
    return 1;
  if (h->direct)
  {
    CompareArgs ad = a;
    ad.gs = h->pd.GridSpaceCenter;
    ad.maxD = h->pd.maxDisplaceCenter;
    hipLaunchKernelGGL(k_c2r_cols, dim3(h->H, nOC), dim3(128), sizeof(double2) * h->N, h->stream, bb.conv, h->N, h->H,
                       P.halfR, P.N1, h->dTwD, h->dDirectZ);
    hipLaunchKernelGGL(k_c2r_rows, dim3(h->N, nOC), dim3(128), sizeof(double2) * h->H, h->stream, h->dDirectZ, h->N,
                       h->H, h->dTwD, h->dConvReal);
    const dim3 gridd((unsigned) ((size_t) nOC * ((h->nMaps + 31) / 32)));
    hipLaunchKernelGGL((k_compare_direct<3, 8>), gridd, dim3(512), direct_lds_bytes(h->N), h->stream, ad, h->dConvReal,
                       h->dMapsReal);
  }
  else if (!P.tileT)
    launch(a);
  else
  { // wide window: one launch per tile on the phase-shifted conv spectra, then merge (window_tiles.hpp)
    const int nT = P.tilesPerAxis;
    const size_t tileStride = (size_t) h->nMaps * h->maxOC;
    const size_t total = (size_t) nOC * h->M;
    CompareArgs at = a;
    at.disp = h->dDispLocal;
    at.nd = P.tileT;
    at.maxD = P.winD * P.gs;
    for (int tx = 0; tx < nT; tx++)
      for (int ty = 0; ty < nT; ty++)
      {
        const int sx = P.gs * P.tileCenter[tx], sy = P.gs * P.tileCenter[ty];
        if (sx == 0 && sy == 0)
          at.conv = bb.conv;
        else
        {
          hipLaunchKernelGGL(k_phase_shift, dim3(2048), dim3(256), 0, h->stream, bb.conv, h->dConvShift, total, h->N,
                             h->H, P.halfR, P.N1, sx, sy, h->dTw);
          at.conv = h->dConvShift;
        }
        at.ndx = P.tileValid[tx];
        at.ndy = P.tileValid[ty];
        at.partials = h->dPartTiles + (size_t) (tx * nT + ty) * tileStride;
        launch(at);
      }
    const long long nt = (long long) nOC * h->nMaps;
    hipLaunchKernelGGL(k_merge_tiles, dim3((unsigned) ((nt + 255) / 256)), dim3(256), 0, h->stream, h->dPartTiles,
                       nT * nT, tileStride, h->maxOC, nOC, h->nMaps, P.tileT, nT, h->dTileCenter,
                       h->pd.maxDisplaceCenter / P.gs, P.nd, h->dRankOfRow, h->dPartials);
  }
  HIP_CHECK(h, hipGetLastError());
  HIP_CHECK(h, hipEventRecord(e1, h->stream));
  h->evPending.push_back({e0, e1});
  h->launches++;
  h->comparisons += (long long) nOC * h->nMaps;
  bioem_hip_prob_map *pmap = reinterpret_cast<bioem_hip_prob_map *>(h->dProb);
  bioem_hip_prob_angle *pang = reinterpret_cast<bioem_hip_prob_angle *>(h->dProb + sizeof(bioem_hip_prob_map) * h->nMaps);
  if (h->pd.writeAngles)
  {
    const int nRuns = ids ? nSeg : (nOC + convPerOrient - 1) / convPerOrient;
    const long long nt = (long long) nRuns * h->nMaps;
    hipLaunchKernelGGL(k_fold_angles, dim3((unsigned) ((nt + 255) / 256)), dim3(256), 0, h->stream, h->dPartials,
                       h->maxOC, nOC, h->nMaps, orient0, convPerOrient, segs, nRuns, pang, h->angO0);
  }
  if (h->nMaps <= 64 && nOC >= 1024)
    hipLaunchKernelGGL(k_fold_wave<4>, dim3(h->nMaps), dim3(256), 0, h->stream, h->dPartials, h->maxOC, nOC, h->nMaps,
                       bb.params, h->dSumRef, h->dDisp, P.nd, h->pd, orient0, conv0, convPerOrient, ids, pmap);
  else
    hipLaunchKernelGGL(k_fold_wave<1>, dim3((h->nMaps + 3) / 4), dim3(256), 0, h->stream, h->dPartials, h->maxOC, nOC,
                       h->nMaps, bb.params, h->dSumRef, h->dDisp, P.nd, h->pd, orient0, conv0, convPerOrient, ids,
                       pmap);
  if (h->dCtfTab)
  { // one wave per (CTF of the launch, particle); the compat ring's rows name their CTF, so every CTF gets a wave
    const int nC = ids ? h->nCTF : convPerOrient;
    const long long pairs = (long long) nC * h->nMaps;
    hipLaunchKernelGGL(k_fold_ctf, dim3((unsigned) ((pairs + 3) / 4)), dim3(256), 0, h->stream, h->dPartials, h->maxOC, nOC,
                       h->nMaps, bb.params, h->dSumRef, h->dDisp, P.nd, h->pd, orient0, conv0, convPerOrient, nC, ids,
                       h->dCtfTab);
  }
  HIP_CHECK(h, hipGetLastError());
  if (phase_end(h, h->stream)) // comparison = the kernels of the launch and the fold behind them (what compareRefMaps does)
    return 1;
  if (h->evPending.size() > 512)
    drain_events(h);
  return 0;
}

// Own-list pass: the nOC conv rows of the slot are rows [slot0 nC, ...) of the flat [particle][list entry][CTF] order;
// every row is compared with its own particle and each particle's rows are folded into its entry.  Row oc of the slot
// leaves its result in partials[oc].
//   k_compare_fast plans after bioem_hip_set_own_launch(BIOEM_HIP_OWN_LAUNCH_BATCH): ONE launch of k_compare_fast on
//     OwnCompareArgs over the batch, its blocks mapped to (particle, four rows) by the block table of the batch
//     (own_block_table); the Nyquist rows by k_nyquist_rows on OwnNyquistArgs.
//   every other family, and the default of all (BIOEM_HIP_OWN_LAUNCH_PARTICLE): the comparison kernels as they are, once
//     per particle with rows in the slot: a launch over that particle's run of rows with nMaps = 1, ref / sumRef /
//     sumsqRef pointed at the particle and conv / params / postc / partials / tnyq at the run -- exactly the launch a
//     handle that holds that particle alone makes (its block order, its k_nyquist_rows).
// The two give the same partials bit for bit: a wave computes one (particle, row) pair by the same instructions in both.
int launch_compare_own(bioem_hip_ctx *h, const bioem_hip_ctx::Slot &bb, int nOC, int slot0, int nC)
{
  const KernelPlan &P = h->plan;
  const int row0 = slot0 * nC;
  hipEvent_t e0 = get_event(h), e1 = get_event(h);
  if (!e0 || !e1)
  {
    if (e0)
      h->evPool.push_back(e0);
    if (e1)
      h->evPool.push_back(e1);
    h->err = "hipEventCreate failed";
    return 1;
  }
  const int nSlots = nOC / nC;
  hipLaunchKernelGGL(k_posterior_consts, dim3((nOC + 63) / 64), dim3(64), 0, h->stream, bb.params, h->pd, bb.postc, nOC);
  HIP_CHECK(h, hipEventRecord(e0, h->stream));
  if (phase_begin(h, h->stream, BIOEM_HIP_PHASE_COMPARISON, slot0, slot0 + nSlots, 0, nC))
    return 1;
  // particles with slots in the batch: off[pFirst] <= slot0 < off[pFirst + 1], off[pEnd] >= the batch's end (particles
  // with an empty list between them have no rows)
  const std::vector<int> &off = h->ownOff;
  const int pFirst = (int) (std::upper_bound(off.begin(), off.end(), slot0) - off.begin()) - 1;
  const int pEnd = (int) (std::lower_bound(off.begin(), off.end(), slot0 + nSlots) - off.begin());
  if (h->ownFn)
  {
    const auto it = std::lower_bound(h->ownTabSlot.begin(), h->ownTabSlot.end(), slot0);
    if (it == h->ownTabSlot.end() || *it != slot0)
    {
      h->err = "compare_own_orientations: no block table for this batch";
      return 1;
    }
    const size_t b = (size_t) (it - h->ownTabSlot.begin());
    const int first = h->ownTabFirst[b], nBlocks = h->ownTabFirst[b + 1] - first;
    dim3 grid, block;
    const CompareArgs a = compare_args(h, bb, nOC, h->nMaps, grid, block);
    if (P.nyq)
      hipLaunchKernelGGL(h->ownNyqFn, dim3((nOC + 63) / 64), dim3(256), 0, h->stream,
                         OwnNyquistArgs{a, h->dSlotParticle, row0, nC});
    const own_kernel_t fn = h->ownFnPlanLean && lean_launch_ok(h, a.nd, a.maxD, a.split) ? h->ownFnPlanLean : h->ownFn;
    hipLaunchKernelGGL(fn, dim3(nBlocks), dim3(256), P.ldsBytes, h->stream, OwnCompareArgs{a, h->dOwnBlocks + first});
  }
  else
    for (int p = pFirst; p < pEnd; p++)
    {
      const long long g0 = (long long) off[p] * nC, g1 = (long long) off[p + 1] * nC;
      const int rb = (int) (std::max<long long>(g0, row0) - row0), n = (int) (std::min<long long>(g1, row0 + nOC) - row0) - rb;
      if (n <= 0)
        continue;
      dim3 grid, block;
      CompareArgs a = compare_args(h, bb, n, 1, grid, block);
      a.ref += (size_t) p * h->Mc;
      a.sumRef += p;
      a.sumsqRef += p;
      a.conv += (size_t) rb * h->Mc;
      a.params += rb;
      a.postc += rb;
      a.partials += rb;
      if (P.nyq)
      {
        a.tnyq += (size_t) rb * (2 * P.nyqWD + 1);
        launch_nyquist(h, a, P.nyqWD, n);
      }
      hipLaunchKernelGGL(compare_fn(h, a), grid, block, P.ldsBytes, h->stream, a);
    }
  HIP_CHECK(h, hipGetLastError());
  HIP_CHECK(h, hipEventRecord(e1, h->stream));
  h->evPending.push_back({e0, e1});
  h->launches++;
  h->comparisons += nOC;
  bioem_hip_prob_map *pmap = reinterpret_cast<bioem_hip_prob_map *>(h->dProb);
  bioem_hip_prob_angle *pang = reinterpret_cast<bioem_hip_prob_angle *>(h->dProb + sizeof(bioem_hip_prob_map) * h->nMaps);
  if (h->pd.writeAngles)
    hipLaunchKernelGGL(k_fold_own_angles, dim3((nSlots + 255) / 256), dim3(256), 0, h->stream, h->dPartials, nSlots, slot0,
                       h->dOwnOff, h->dSlotParticle, nC, h->nMaps, pang);
  hipLaunchKernelGGL(k_fold_own, dim3((pEnd - pFirst + 3) / 4), dim3(256), 0, h->stream, h->dPartials, nOC, row0,
                     h->dOwnOff, nC, pFirst, pEnd, bb.params, h->dSumRef, h->dDisp, P.nd, h->pd, pmap);
  if (h->dCtfTab)
    hipLaunchKernelGGL(k_fold_own_ctf, dim3((unsigned) (((long long) nC * (pEnd - pFirst) + 3) / 4)), dim3(256), 0, h->stream,
                       h->dPartials, nOC, row0, h->dOwnOff, nC, h->nMaps, pFirst, pEnd, bb.params, h->dSumRef, h->dDisp,
                       P.nd, h->pd, h->dCtfTab);
  HIP_CHECK(h, hipGetLastError());
  if (phase_end(h, h->stream))
    return 1;
  if (h->evPending.size() > 512)
    drain_events(h);
  return 0;
}

// batches of the own-list pass over particles [p0, p1): slots (particle, list entry), at most ownOB per batch, at least
// six per call where that leaves 64 or more per batch (the first batch's preparation hides behind nothing), of equal
// size.  Returns the first slot of every batch, and the end.
std::vector<int> own_batches(const bioem_hip_ctx *h, int p0, int p1)
{
  const long long s0 = h->ownOff[p0], s1 = h->ownOff[p1];
  const int per = (int) std::min<long long>(h->ownOB, std::max<long long>(64, (s1 - s0 + 5) / 6));
  std::vector<int> first;
  for (long long s = s0; s < s1; s += per)
    first.push_back((int) s);
  first.push_back((int) s1);
  return first;
}

// Block table of k_compare_fast on OwnCompareArgs for the batches of particles [p0, p1): one entry {particle, first row, end row, 0}
// per block, rows counted from the batch's first row, at most four consecutive rows of ONE particle's run in the batch
// (the groups of four begin at the run's first row, as the per-particle launch forms them).  It depends on the offsets,
// nCTF and the batch cuts only.  Order inside a batch (the order does not change results; DESIGN 2.9 has the
// measurement): plain row order, or -- workgroups go round-robin over the 8 XCDs, each with its own L2 -- a particle's
// blocks at indices congruent mod 8: its spectrum, the only operand several blocks share, then stays in ONE L2.  The runs
// of a batch go to the XCD with the fewest blocks so far; where the eight queues run out unevenly the tail closes up.
int own_block_table(bioem_hip_ctx *h, int p0, int p1)
{
  const std::vector<int> first = own_batches(h, p0, p1);
  const int nb = (int) first.size() - 1, nC = h->nCTF;
  const std::vector<int> &off = h->ownOff;
  std::vector<int4> tab;
  std::vector<int> tabSlot, tabFirst;
  for (int b = 0; b < nb; b++)
  {
    const long long row0 = (long long) first[b] * nC, rowEnd = (long long) first[b + 1] * nC;
    tabSlot.push_back(first[b]);
    tabFirst.push_back((int) tab.size());
    const int pFirst = (int) (std::upper_bound(off.begin(), off.end(), first[b]) - off.begin()) - 1;
    std::vector<int4> q[8];
    for (int p = pFirst; p < h->nMaps && (long long) off[p] * nC < rowEnd; p++)
    {
      const int rb = (int) (std::max<long long>((long long) off[p] * nC, row0) - row0);
      const int re = (int) (std::min<long long>((long long) off[p + 1] * nC, rowEnd) - row0);
      if (re <= rb)
        continue;
      int x = 0;
      if (h->ownXcdOrder)
        for (int k = 1; k < 8; k++)
          if (q[k].size() < q[x].size())
            x = k;
      for (int g = rb; g < re; g += 4)
        q[x].push_back(make_int4(p, g, std::min(g + 4, re), 0));
    }
    size_t longest = 0;
    for (const auto &v : q)
      longest = std::max(longest, v.size());
    for (size_t i = 0; i < longest; i++)
      for (const auto &v : q)
        if (i < v.size())
          tab.push_back(v[i]);
  }
  tabFirst.push_back((int) tab.size());
  // nothing queued may still read the table that is replaced
  HIP_CHECK(h, hipStreamSynchronize(h->stream));
  if (tab.size() > h->ownBlockCap)
  {
    int4 *t = nullptr;
    if (dev_alloc(h, t, tab.size()))
      return 1;
    dev_release(h, h->dOwnBlocks);
    h->dOwnBlocks = t;
    h->ownBlockCap = tab.size();
  }
  h->ownTabP0 = h->ownTabP1 = -1;
  if (!tab.empty())
    HIP_CHECK(h, hipMemcpy(h->dOwnBlocks, tab.data(), sizeof(int4) * tab.size(), hipMemcpyHostToDevice));
  h->ownTabSlot.swap(tabSlot);
  h->ownTabFirst.swap(tabFirst);
  h->ownTabP0 = p0;
  h->ownTabP1 = p1;
  return 0;
}

// the exact-DFT r2c kernels keep one image row / column (and its twiddles) in dynamic LDS: 24 N + 16 and 32 N bytes.
// Above 64 KiB a launch needs the explicit opt-in; 32 N <= 160 KiB bounds the image size at 5120 pixels (the
// reference's MRC reader stops at 5000, mrc.h:128-133).
const int kMaxPixels = 5120;
// the exact-DFT kernels keep a row / column (and their intermediate) in LDS; up to kDftTwLds pixels the twiddle table, too
constexpr int kDftTwLds = 3072;
size_t dft_rows_lds(int N) { return sizeof(double) * ((N <= kDftTwLds ? 5 : 3) * (size_t) N + 2); }
size_t dft_cols_lds(int N) { return sizeof(double2) * (N <= kDftTwLds ? 3 : 2) * (size_t) N; }
void dft_split(int N, int &A, int &B)
{
  A = 1;
  for (int d = 1; d * d <= N; d++)
    if (N % d == 0)
      A = d;
  B = N / A;
}
// the fast transform (r2c_fft.hpp) wherever it has the lengths; BIOEM_R2C=dft keeps the exact-DFT kernels (A/B, tests)
bool r2c_use_fft(int N)
{
  const char *e = getenv("BIOEM_R2C");
  return bioem_r2c_fft_supported(N) && !(e && !strcmp(e, "dft"));
}
bool dft_use_mfma(int N)
{
  int A, B;
  dft_split(N, A, B);
  return dft_mfma_fits(N, A, B);
}
hipError_t dft_allow_lds(int N)
{
  hipError_t e;
  if (dft_use_mfma(N))
  {
    const void *fns[4] = {reinterpret_cast<const void *>(k_dft_rows_mfma<2>),
                          reinterpret_cast<const void *>(k_dft_rows_mfma<kDftMfmaTiles>),
                          reinterpret_cast<const void *>(k_dft_cols_mfma<2>),
                          reinterpret_cast<const void *>(k_dft_cols_mfma<kDftMfmaTiles>)};
    for (int f = 0; f < 4; f++)
    {
      e = hipFuncSetAttribute(fns[f], hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int) (f < 2 ? dft_mfma_rows_lds(N) : dft_mfma_cols_lds(N)));
      if (e != hipSuccess)
        return e;
    }
    return hipSuccess;
  }
  if (N <= kDftTwLds)
  {
    e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_dft_rows<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int) dft_rows_lds(N));
    if (e != hipSuccess)
      return e;
    return hipFuncSetAttribute(reinterpret_cast<const void *>(k_dft_cols<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int) dft_cols_lds(N));
  }
  e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_dft_rows<false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int) dft_rows_lds(N));
  if (e != hipSuccess)
    return e;
  return hipFuncSetAttribute(reinterpret_cast<const void *>(k_dft_cols<false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int) dft_cols_lds(N));
}

// k_convolve_sums keeps two tiles of terms for up to 20 (orientation, CTF) chains in dynamic LDS: 151 KiB
hipError_t conv_allow_lds()
{
  const void *fns[3] = {reinterpret_cast<const void *>(k_convolve_sums<3, 6>), reinterpret_cast<const void *>(k_convolve_sums<3, 5>),
                        reinterpret_cast<const void *>(k_convolve_sums<4, 4>)};
  for (const void *f : fns)
  {
    const hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int) conv_lanes_lds(kLaneRows));
    if (e != hipSuccess)
      return e;
  }
  return hipSuccess;
}

// r2c of nImg images (double projection maps scaled by NormDen / tempden, or float maps) into `out` (reference layout);
// rowSpec holds the row pass (N x H double2 per image).  dft_allow_lds(N) must have run on this device.
hipError_t launch_r2c(hipStream_t st, int nCU, const double *srcD, const float *srcF, const double *tempDen, float NormDen,
                      int N, int nImg, const double2 *tw, double2 *rowSpec, float2 *out, int lo = 0, int side = 0)
{
  side = side ? side : N; // (a box smaller than the map: the fast transform only, see project_batch)
  const int H = N / 2 + 1;
  int A, B;
  dft_split(N, A, B);
  if (r2c_use_fft(N))
    return bioem_r2c_fft_launch(st, nCU, srcD, srcF, tempDen, NormDen, N, nImg, tw, rowSpec, out, lo, side);
  if (dft_use_mfma(N))
  {
    // resident grids: as many blocks as the LDS of the device holds at once
    const int perCU = std::max(1, std::min(4, (int) (160 * 1024 / (dft_mfma_cols_lds(N) + 1024))));
    const int rowUnits = ((N + 15) / 16) * nImg, colUnits = ((H + 15) / 16) * nImg;
    if (A * ((B + 15) / 16) <= 2 * kDftMfmaWaves)
    {
      hipLaunchKernelGGL(k_dft_rows_mfma<2>, dim3(std::min(rowUnits, perCU * nCU)), dim3(kDftMfmaThreads),
                         dft_mfma_rows_lds(N), st, srcD, srcF, tempDen, NormDen, N, H, A, B, nImg, tw, rowSpec);
      hipLaunchKernelGGL(k_dft_cols_mfma<2>, dim3(std::min(colUnits, perCU * nCU)), dim3(kDftMfmaThreads),
                         dft_mfma_cols_lds(N), st, rowSpec, N, H, A, B, nImg, tw, out);
    }
    else
    {
      // registers hold one block of this variant per CU
      hipLaunchKernelGGL(k_dft_rows_mfma<kDftMfmaTiles>, dim3(std::min(rowUnits, nCU)), dim3(kDftMfmaThreads),
                         dft_mfma_rows_lds(N), st, srcD, srcF, tempDen, NormDen, N, H, A, B, nImg, tw, rowSpec);
      hipLaunchKernelGGL(k_dft_cols_mfma<kDftMfmaTiles>, dim3(std::min(colUnits, nCU)), dim3(kDftMfmaThreads),
                         dft_mfma_cols_lds(N), st, rowSpec, N, H, A, B, nImg, tw, out);
    }
  }
  else if (N <= kDftTwLds)
  {
    hipLaunchKernelGGL(k_dft_rows<true>, dim3(N, nImg), dim3(128), dft_rows_lds(N), st, srcD, srcF, tempDen, NormDen, N,
                       H, A, B, tw, rowSpec);
    hipLaunchKernelGGL(k_dft_cols<true>, dim3(H, nImg), dim3(256), dft_cols_lds(N), st, rowSpec, N, H, A, B, tw, out);
  }
  else
  {
    hipLaunchKernelGGL(k_dft_rows<false>, dim3(N, nImg), dim3(128), dft_rows_lds(N), st, srcD, srcF, tempDen, NormDen, N,
                       H, A, B, tw, rowSpec);
    hipLaunchKernelGGL(k_dft_cols<false>, dim3(H, nImg), dim3(256), dft_cols_lds(N), st, rowSpec, N, H, A, B, tw, out);
  }
  return hipGetLastError();
}

int run_r2c(bioem_hip_ctx *h, const bioem_hip_ctx::Slot &bb, hipStream_t st, const double *srcD, const float *srcF, int nImg,
            int lo = 0, int side = 0)
{
  HIP_CHECK(h, launch_r2c(st, h->nCU, srcD, srcF, bb.tempDen, h->NormDen, h->N, nImg, h->dTwD, bb.rowSpec, bb.specRef, lo,
                          side));
  return 0;
}

// the orientation list a projection reads: the shared one, or the per-particle lists as one flat list of slots
struct OrientList
{
  const float4 *d;
  int isQuat;
  double quatNormDev;
};
// a model of either kind: points, or a volume
bool has_model(const bioem_hip_ctx *h) { return h->dPts || h->dVolC; }

OrientList shared_list(const bioem_hip_ctx *h) { return {h->dAngles, h->isQuat, h->quatNormDev}; }
OrientList own_list(const bioem_hip_ctx *h) { return {h->dOwnAngles, h->ownIsQuat, h->ownQuatNormDev}; }

// what a projection of this model under this list takes: kProjectBox (k_project_box), kProjectBands (k_project_coords +
// k_project_bands) or kProjectAtomics (k_project), with the geometry the launch needs
enum
{
  kProjectAuto = 0,
  kProjectBox = 1,
  kProjectBands = 2,
  kProjectAtomics = 3
};
struct ProjectPlan
{
  int path;
  int boxLo, boxSide, compact; // the box the host sizes for the model, whatever the path; compact: the box alone is stored
  int TR;                      // rows of one LDS band
  const char *refused;         // a forced path whose preconditions do not hold: why (path is then kProjectAuto)
};

// force = kProjectAuto: what a run takes; else that path, or `refused` where its preconditions do not hold
ProjectPlan project_plan(const bioem_hip_ctx *h, const OrientList &L, int force)
{
  ProjectPlan P = {};
  const int N = h->N;
  // the pixels a point of the model can reach in any orientation, with its footprint: a box around the map centre
  const double reach = h->modelRadius / (double) h->pixelSize;
  const int boxLo = std::max(0, (int) std::floor(N / 2.0 + 0.5 - reach) - 1 - h->iradMax - std::max(0, std::max(h->shiftX, h->shiftY)));
  const int boxHi = std::min(N - 1, (int) std::floor(N / 2.0 + 0.5 + reach) + 1 + h->iradMax - std::min(0, std::min(h->shiftX, h->shiftY)));
  const int boxSide = boxHi - boxLo + 1;
  P.boxLo = boxLo;
  P.boxSide = boxSide;
  // (orientations that stretch the model -- quaternions that are not of unit length -- take the band kernel: the box
  // has one pixel of margin; the matrix entries of a quaternion with |q|^2 = 1 + e are off by at most ~3 e, and half a
  // pixel is granted to that)
  const bool keepLength = L.quatNormDev * 4.0 * std::max(1.0, reach) < 0.5;
  P.TR = 40960 / (8 * N); // rows of one LDS band: three blocks per CU
  // the record of every (orientation, point) borrows the row-pass buffer of the r2c that follows
  const bool coordsFit = (size_t) h->nPts * sizeof(ProjectRecord) <= (size_t) N * h->H * sizeof(double2);
  const bool boxFits = boxSide >= 1 && (size_t) boxSide * boxSide * sizeof(double) <= 52 * 1024;
  const bool boxOk = h->dStamp && boxFits && N < 32768 && keepLength;
  const bool bandsOk = P.TR >= 12 && h->iradMax <= 16 && h->dStamp && N < 32768 && coordsFit;
  if (force == kProjectBox && !boxOk)
    P.refused = !h->dStamp ? "the model has no footprint table" : !boxFits ? "the model's box does not fit 52 KiB of LDS"
                : !keepLength ? "the list holds quaternions that are not of unit length" : "the image is too large";
  else if (force == kProjectBands && !bandsOk)
    P.refused = !h->dStamp       ? "the model has no footprint table"
                : P.TR < 12      ? "a band of the image holds fewer than 12 rows"
                : h->iradMax > 16 ? "a footprint is wider than 33 pixels"
                : !coordsFit     ? "the records of the points do not fit the row-pass buffer"
                                 : "the image is too large";
  else
    P.path = force != kProjectAuto ? force : boxOk ? kProjectBox : bandsOk ? kProjectBands : kProjectAtomics;
  // with the fast r2c behind it the box kernel stores the box alone and the transform skips everything outside it
  P.compact = P.path == kProjectBox && r2c_use_fft(N);
  return P;
}

// force, taken: bioem_hip_debug_projection_maps; a refused path returns 2 with the reason in h->err and launches nothing
int project_batch(bioem_hip_ctx *h, const bioem_hip_ctx::Slot &bb, hipStream_t st, const OrientList &L, int o0, int nO,
                  int force = kProjectAuto, ProjectPlan *taken = nullptr)
{
  const int N = h->N;
  if (h->dVolC)
  { // a volume model: the slices of its spectrum stand where the r2c stores its result; the matrices borrow the row-pass
    // buffer of the r2c that does not run (9 doubles per image of N H double2)
    double *R = reinterpret_cast<double *>(bb.rowSpec);
    HIP_CHECK(h, bioem_recon_matrices_launch(st, L.d + o0, nullptr, L.isQuat, nO, R));
    HIP_CHECK(h, bioem_slice_project_launch(st, h->dVolC, h->volPad, R, nO, N, h->dTwD, h->shiftX, h->shiftY,
                                            (double) h->NormDen, bb.specRef, nullptr, bb.tempDen));
    return 0;
  }
  const ProjectPlan P = project_plan(h, L, force);
  if (taken)
    *taken = P;
  if (P.refused)
  {
    h->err = std::string("projection path ") + std::to_string(force) + ": " + P.refused;
    return 2;
  }
  const int boxLo = P.boxLo, boxSide = P.boxSide, TR = P.TR;
  if (P.path == kProjectBox)
  {
    const int compact = P.compact;
    hipLaunchKernelGGL(k_project_box, dim3(std::min(nO, 3 * h->nCU)), dim3(256), sizeof(double) * boxSide * boxSide, st,
                       h->dPts, h->nPts, L.d, o0, L.isQuat, N, h->pixelSize, h->shiftX, h->shiftY, h->iradMax,
                       h->dStamp, boxLo, boxSide, nO, compact, bb.projReal, bb.tempDen);
    HIP_CHECK(h, hipGetLastError());
    return compact ? run_r2c(h, bb, st, bb.projReal, nullptr, nO, boxLo, boxSide) : run_r2c(h, bb, st, bb.projReal, nullptr, nO);
  }
  HIP_CHECK(h, hipMemsetAsync(bb.tempDen, 0, sizeof(double) * nO, st)); // (k_project_box writes its sums itself)
  if (P.path == kProjectBands)
  {
    ProjectRecord *coords = reinterpret_cast<ProjectRecord *>(bb.rowSpec);
    hipLaunchKernelGGL(k_project_coords, dim3((h->nPts + 255) / 256, nO), dim3(256), 0, st, h->dPts, h->nPts, L.d,
                       o0, L.isQuat, N, h->pixelSize, h->shiftX, h->shiftY, coords);
    const int units = ((N + TR - 1) / TR) * nO;
    hipLaunchKernelGGL(k_project_bands, dim3(std::min(units, 3 * h->nCU)), dim3(256), sizeof(double) * TR * N, st, coords,
                       h->nPts, nO, N, TR, h->iradMax, h->dStamp, bb.projReal, bb.tempDen);
  }
  else
  {
    HIP_CHECK(h, hipMemsetAsync(bb.projReal, 0, sizeof(double) * (size_t) nO * N * N, st));
    hipLaunchKernelGGL(k_project, dim3((h->nPts + 255) / 256, nO), dim3(256), 0, st, h->dPts, h->nPts, L.d, o0,
                       L.isQuat, N, h->pixelSize, h->shiftX, h->shiftY, bb.projReal, bb.tempDen);
  }
  HIP_CHECK(h, hipGetLastError());
  return run_r2c(h, bb, st, bb.projReal, nullptr, nO);
}

// ---- compat ring (bioem_hip_compare) ----
int compat_alloc(bioem_hip_ctx *h)
{
  if (h->ringCap)
    return 0;
  int cap = 128; // rows per half: 128 x 1 000 particles = 2.6 ms of comparison kernel at 224^2
  if (getenv("BIOEM_COMPAT_RING"))
    cap = atoi(getenv("BIOEM_COMPAT_RING"));
  cap = std::max(1, std::min(cap, h->maxOC));
  const size_t M = (size_t) h->M;
  for (int k = 0; k < 2; k++)
  {
    bioem_hip_ctx::CompatHalf &r = h->ring[k];
    if (host_alloc(h, r.hConv, M * cap) || host_alloc(h, r.hPar, cap) || host_alloc(h, r.hIds, cap) ||
        host_alloc(h, r.hSeg, cap) || dev_alloc(h, r.dStage, M * cap) || dev_alloc(h, r.dIds, cap) ||
        dev_alloc(h, r.dSeg, cap))
      return 1;
    HIP_CHECK(h, hipEventCreateWithFlags(&r.staged, hipEventDisableTiming));
  }
  HIP_CHECK(h, hipStreamCreateWithFlags(&h->copyStream, hipStreamNonBlocking));
  h->ringCap = cap;
  h->ringHalf = 0;
  h->ringCount = 0;
  return 0;
}

// launch the comparison of the rows staged in the current half, then switch halves
int compat_flush(bioem_hip_ctx *h)
{
  const int n = h->ringCount;
  if (n == 0)
    return 0;
  const int half = h->ringHalf;
  bioem_hip_ctx::CompatHalf &r = h->ring[half];
  bioem_hip_ctx::Slot &bb = h->slot[half];
  void_slot(bb);
  // runs of equal orientation (rows arrive in call order; an orientation never returns within a half, see compare)
  int nSeg = 0;
  for (int i = 0; i < n; i++)
  {
    if (nSeg && r.hSeg[nSeg - 1].z == r.hIds[i].x)
      r.hSeg[nSeg - 1].y = i + 1;
    else
      r.hSeg[nSeg++] = make_int4(i, i + 1, r.hIds[i].x, 0);
  }
  HIP_CHECK(h, hipEventRecord(r.staged, h->copyStream));
  HIP_CHECK(h, hipStreamWaitEvent(h->stream, r.staged, 0));
  HIP_CHECK(h, hipMemcpyAsync(bb.params, r.hPar, sizeof(bioem_hip_param5) * n, hipMemcpyHostToDevice, h->stream));
  HIP_CHECK(h, hipMemcpyAsync(r.dIds, r.hIds, sizeof(int2) * n, hipMemcpyHostToDevice, h->stream));
  HIP_CHECK(h, hipMemcpyAsync(r.dSeg, r.hSeg, sizeof(int4) * nSeg, hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(k_reorder, dim3(std::min(2048, 8 * n)), dim3(256), 0, h->stream, r.dStage, bb.conv, n, h->N, h->H,
                     h->plan.halfR, h->plan.N1, h->Hp);
  HIP_CHECK(h, hipGetLastError());
  if (launch_compare_fold(h, bb, n, 0, 0, 1, r.dIds, r.dSeg, nSeg))
    return 1;
  HIP_CHECK(h, hipEventRecord(bb.cmpDone, h->stream));
  bb.cmpPending = true;
  h->ringHalf ^= 1;
  h->ringCount = 0;
  h->ringOrients.clear();
  return 0;
}

// conv spectra of CTFs [c0, c0 + nC) of the nO projected orientations, row ob * nC + (c - c0)
// which of the two convolution paths a batch takes (read per call; bioem_hip_debug_convolve_batch reports it)
bool convolve_fused(const bioem_hip_ctx *h, bool own)
{
  // few particles: the preparation is the longer half of the pipeline and the fused kernel shortens it; many particles:
  // it hides behind the comparison either way, and the one-wave blocks of k_parseval_ordered take less from the
  // comparison kernel than the 16-wave blocks of k_convolve_sums (round 4, the fused kernel with 3-4 orientations per
  // block: 65...200 particles +1...3 %, 400 particles equal, 1 000 particles 52.5 against 53.4 M comparisons/s)
  const char *fe = getenv("BIOEM_CONVOLVE_FUSED");
  // (the own-list pass: a conv spectrum meets one particle, the preparation is the long pole whatever nMaps is, and its
  // batches hold no buffer for the ordered sums of the two-kernel path -- always fused)
  return own || (fe ? atoi(fe) != 0 : h->nMaps <= 256);
}

int convolve_batch(bioem_hip_ctx *h, const bioem_hip_ctx::Slot &bb, hipStream_t st, int nO, int c0, int nC, bool own = false)
{
  if (convolve_fused(h, own))
  {
    // chains on the lanes of the adding wave: 4 orientations x up to 4 CTFs, 3 x 5, or 3 x 6 per block (16, 15, 18
    // products per producing thread and tile: more, and the producers -- ~25 vector instructions per product -- take
    // longer than the 960 additions)
    if (nC <= 4)
      hipLaunchKernelGGL((k_convolve_sums<4, 4>), dim3(1, (nO + 3) / 4), dim3(kConvThreads), conv_lanes_lds(4 * nC), st,
                         bb.specRef, h->dCTF, h->dCtfParam, h->N, h->H, h->plan.halfR, h->plan.N1, c0, nC, nO, 4 * nC, bb.conv, bb.params, h->Hp);
    else if (nC == 5)
      hipLaunchKernelGGL((k_convolve_sums<3, 5>), dim3(1, (nO + 2) / 3), dim3(kConvThreads), conv_lanes_lds(15), st, bb.specRef,
                         h->dCTF, h->dCtfParam, h->N, h->H, h->plan.halfR, h->plan.N1, c0, nC, nO, 15, bb.conv, bb.params, h->Hp);
    else
      hipLaunchKernelGGL((k_convolve_sums<3, 6>), dim3((nC + 5) / 6, (nO + 2) / 3), dim3(kConvThreads), conv_lanes_lds(18), st,
                         bb.specRef, h->dCTF, h->dCtfParam, h->N, h->H, h->plan.halfR, h->plan.N1, c0, nC, nO, 18, bb.conv, bb.params, h->Hp);
    HIP_CHECK(h, hipGetLastError());
    return 0;
  }
  const int M4 = (int) ((h->M + 3) & ~(size_t) 3);
  hipLaunchKernelGGL(k_convolve, dim3(nC, nO), dim3(256), 0, st, bb.specRef, h->dCTF, h->dCtfParam, h->N, h->H,
                     h->plan.halfR, h->plan.N1, c0, bb.conv, bb.scratch, M4, bb.params, h->Hp);
  HIP_CHECK(h, hipGetLastError());
  // the ordered Parseval sums of all nC x nO spectra side by side: four sequential chains per wave
  hipLaunchKernelGGL(k_parseval_ordered, dim3((nC * nO + 3) / 4), dim3(64), 0, st, bb.scratch, (int) h->M, M4, nC * nO,
                     (float) (h->N * h->N), bb.params);
  HIP_CHECK(h, hipGetLastError());
  return 0;
}

// the two-slot pipeline of the fused entries: projection + convolution of batch b + 1 run on prepStream while batch b is
// compared.  first = first orientation of every batch, and the end; own: the orientations are slots (particle, list
// entry) of the per-particle lists and every conv row meets its own particle only (launch_compare_own).
int run_pipeline(bioem_hip_ctx *h, const std::vector<int> &first, int iConvBegin, int nC, bool own)
{
  const OrientList L = own ? own_list(h) : shared_list(h);
  const int nb = (int) first.size() - 1;
  auto prep = [&](int b) -> int {
    bioem_hip_ctx::Slot &bb = h->slot[b & 1];
    const int o0 = first[b];
    const int nO = first[b + 1] - o0;
    void_slot(bb);
    if (bb.cmpPending)
    {
      HIP_CHECK(h, hipStreamWaitEvent(h->prepStream, bb.cmpDone, 0));
      bb.cmpPending = false;
    }
    if (phase_begin(h, h->prepStream, BIOEM_HIP_PHASE_PROJECTION, o0, o0 + nO, 0, 0) ||
        project_batch(h, bb, h->prepStream, L, o0, nO) || phase_end(h, h->prepStream))
      return 1;
    if (phase_begin(h, h->prepStream, BIOEM_HIP_PHASE_CONVOLUTION, o0, o0 + nO, iConvBegin, iConvBegin + nC) ||
        convolve_batch(h, bb, h->prepStream, nO, iConvBegin, nC, own) || phase_end(h, h->prepStream))
      return 1;
    HIP_CHECK(h, hipEventRecord(bb.prepDone, h->prepStream));
    return 0;
  };
  // anything still queued on the main stream that uses slot 0/1 buffers (debug hooks, compat entry) goes first
  for (bioem_hip_ctx::Slot &sl : h->slot)
  {
    HIP_CHECK(h, hipEventRecord(sl.cmpDone, h->stream));
    sl.cmpPending = true;
  }
  if (nb > 0 && prep(0))
    return 1;
  for (int b = 0; b < nb; b++)
  {
    bioem_hip_ctx::Slot &bb = h->slot[b & 1];
    const int o0 = first[b];
    const int nO = first[b + 1] - o0;
    if (b + 1 < nb && prep(b + 1))
      return 1;
    HIP_CHECK(h, hipStreamWaitEvent(h->stream, bb.prepDone, 0));
    if (own ? launch_compare_own(h, bb, nO * nC, o0, nC) : launch_compare_fold(h, bb, nO * nC, o0, iConvBegin, nC))
      return 1;
    HIP_CHECK(h, hipEventRecord(bb.cmpDone, h->stream));
    bb.cmpPending = true;
  }
  // later main-stream work (finish_run, debug hooks) must also see prepStream drained: it is, through prepDone
  return 0;
}

} // namespace

// ================================================================================================
// C ABI
// ================================================================================================
extern "C" {

int bioem_hip_device_count(void)
{
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess)
    return 0;
  return n;
}

size_t bioem_hip_prob_size(int nMaps, int nAngles, int writeAngles)
{
  size_t size = sizeof(bioem_hip_prob_map);
  if (writeAngles)
    size += (size_t) nAngles * sizeof(bioem_hip_prob_angle);
  return (size_t) nMaps * size;
}

const char *bioem_hip_last_error(bioem_hip_handle h) { return h ? h->err.c_str() : "null handle"; }

static int create_impl(bioem_hip_handle *out, int device, const bioem_hip_param_device *pd, int nMaps, int nAngles,
                       int nCTF, int algo, bool shard, int angO0, int angO1)
{
  if (!out || !pd)
    return 2;
  bioem_hip_ctx *h = new bioem_hip_ctx;
  *out = h;
  h->shard = shard;
  h->angO0 = angO0;
  h->angO1 = angO1;
  h->device = device;
  h->pd = *pd;
  h->nMaps = nMaps;
  h->nAngles = nAngles;
  h->nCTF = nCTF;
  h->algo = algo;
  const int N = pd->NumberPixels;
  h->N = N;
  h->H = N / 2 + 1;
  h->M = N * h->H;
  if (N < 2 || nMaps < 1 || nAngles < 1 || nCTF < 1 || pd->maxDisplaceCenter < 0 || pd->GridSpaceCenter < 1 ||
      pd->maxDisplaceCenter >= N / 2)
  {
    h->err = "invalid configuration (need N>=2, nMaps,nAngles,nCTF>=1, 0<=maxD<N/2, grid>=1)";
    return 2;
  }
  if (angO0 < 0 || angO1 > nAngles || angO0 >= angO1)
  {
    h->err = "invalid configuration: orientation range of the shard must be a non-empty part of [0, nAngles)";
    return 2;
  }
  if (N > kMaxPixels)
  {
    h->err = "invalid configuration: images larger than 5120 x 5120 pixels are not supported";
    return 2;
  }
  HIP_CHECK(h, hipSetDevice(device));
  HIP_CHECK(h, hipDeviceGetAttribute(&h->nCU, hipDeviceAttributeMultiprocessorCount, device));
  HIP_CHECK(h, dft_allow_lds(N));
  HIP_CHECK(h, conv_allow_lds());
  {
    int prLow = 0, prHigh = 0;
    HIP_CHECK(h, hipDeviceGetStreamPriorityRange(&prLow, &prHigh));
    HIP_CHECK(h, hipStreamCreateWithPriority(&h->stream, hipStreamNonBlocking, prHigh));
    // projection/convolution are filler work with many particles: lowest priority so that comparison blocks win the
    // CUs.  With few particles they are the longer half of the pipeline and waiting behind every comparison block
    // stretches them four- to sixfold: same priority as the comparison then (20 particles: 8.41 -> 8.25 ms per pass;
    // 1 000 particles: no difference either way).
    HIP_CHECK(h, hipStreamCreateWithPriority(&h->prepStream, hipStreamNonBlocking, nMaps <= 64 ? prHigh : prLow));
  }

  // which kernel runs this shape: kernel_select.hpp (pure function of N and the displacement set)
  const int maxD = pd->maxDisplaceCenter;
  h->plan = plan_kernels(N, maxD, pd->GridSpaceCenter, algo);
  const KernelPlan &P = h->plan;
  if (P.err || !P.fn)
  {
    h->err = P.err ? P.err : "no comparison kernel for this configuration";
    return 2;
  }
  HIP_CHECK(h, hipFuncSetAttribute(reinterpret_cast<const void *>(P.fn), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int) P.ldsBytes));
  if (P.fnLean)
    HIP_CHECK(h, hipFuncSetAttribute(reinterpret_cast<const void *>(P.fnLean), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int) P.ldsBytes));
  const int mD = maxD / P.gs;
  const char *directEnv = getenv("BIOEM_CC_DIRECT");
  h->direct = directEnv && atoi(directEnv) != 0;
  if (h->direct)
  { // compare_direct.hpp: the sliding-window evaluation of the same cross-correlation values
    const int gsd = pd->GridSpaceCenter;
    if (N > kDirectMaxN || gsd < 1 || maxD % gsd != 0 || 2 * (maxD / gsd) + 1 > 24 || P.tileT)
    {
      h->err = "BIOEM_CC_DIRECT: the direct cross-correlation takes images up to 160 pixels and regular windows of at "
               "most 24 offsets per axis";
      return 2;
    }
  }
  // own-list pass: one launch per particle unless bioem_hip_set_own_launch asks for one launch per batch, which the
  // handle can do where the plan's kernel has an own variant (the single launch has no same-box measurement against the
  // per-particle launches yet, DESIGN 2.9: it is not the default of any shape)
  {
    h->ownFnPlan = h->direct ? nullptr : plan_own_kernel(P);
    h->ownFn = nullptr;
    if (h->ownFnPlan)
    {
      h->ownNyqFn = P.nyq ? reinterpret_cast<nyq_own_kernel_t>(const_cast<void *>(bioem_nyquist_rows_own(P.nyqWD))) : nullptr;
      HIP_CHECK(h, hipFuncSetAttribute(reinterpret_cast<const void *>(h->ownFnPlan), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int) P.ldsBytes));
      h->ownFnPlanLean = plan_own_kernel(P, 1);
      if (h->ownFnPlanLean)
        HIP_CHECK(h, hipFuncSetAttribute(reinterpret_cast<const void *>(h->ownFnPlanLean),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int) P.ldsBytes));
    }
  }
  // Pitch of the comparison layout.  A lane block of the fast kernels keeps eight rows of one 64-column block in flight;
  // with N a multiple of 64 a row pair is 16 B more than a multiple of 512 B (4 112 B at 512^2, 2 064 B at 256^2) and all
  // of them start in the same few L2 channels.  Fifteen more words make the pitch an odd number of 256-byte lines
  // (timing build first: 512^2 8.3 -> 10.1 M/s; the real thing, same box, +-5 / +-10 px: 512^2 +20 %, 384^2 +6.7 %, 448^2
  // +7 / +4 %, 256^2 +3 %, 192^2 and 320^2 +2...3.5 %, +0...6 % on the matrix-core families; the headline shape, whose
  // kernel reads one argument more, 54.74 against 54.68 M/s).  64^2 and 128^2 gain nothing, 128^2 loses 1...3 % on
  // few-particle jobs: not padded by this rule.  k_compare_wide2 (operands once per comparison) gains nothing: its plans,
  // the tiled ones, odd sizes and the direct kernel keep Hp = H.
  // Every other shape of the three families from 160 pixels on takes the line-aligned pitch (line_aligned_pitch above:
  // H rounded up to 8 words, for the L1's sake, not the channels'; 224^2: 113 -> 120, profiles/lean_operand_ab.txt).
  // (Other numbers of words: 7 / 15 / 23 / 31 / 47 are within 2 % of each other at 256^2 ... 512^2,
  // profiles/r04_padded_pitch_ab.txt.)
  constexpr int kPitchPadWords = 15;
  const bool padFamily = (P.family == KF_FAST || P.family == KF_FASTM || P.family == KF_FASTM2) && !P.tileT &&
                         !h->direct && !getenv("BIOEM_NO_PITCH_PAD");
  const bool padPitch = padFamily && N % 64 == 0 && N >= 192;
  h->Hp = padPitch ? h->H + kPitchPadWords : padFamily ? line_aligned_pitch(N, h->H) : h->H;
  h->Mc = (size_t) N * h->Hp;

  // batch sizing: conv buffer <= ~96 MiB, partial buffer <= ~128 MiB
  const size_t M = (size_t) h->M;
  size_t ocCap = (96u << 20) / (h->Mc * sizeof(float2));
  // (tiled wide windows keep one partial per tile and comparison besides the merged one)
  const size_t partBuffers = 1 + (P.tileT ? (size_t) P.tilesPerAxis * P.tilesPerAxis : 0);
  size_t partCap = (128u << 20) / ((size_t) nMaps * sizeof(Partial));
  if (partBuffers > 1)
    partCap = std::max<size_t>((size_t) nCTF, (1024u << 20) / ((size_t) nMaps * sizeof(Partial) * partBuffers));
  if (ocCap > partCap)
    ocCap = partCap;
  // Few particles (BASELINE config 1: 10): a batch of 64 orientations is a comparison launch of a few thousand pairs
  // behind a preparation whose duration is set by latencies, not work (the ordered Parseval sum of k_convolve is one
  // sequential float chain per conv spectrum, bit-pinned to bioem.cpp:1896-1914) -- all chains of a batch run side by
  // side, so the batch grows until one launch compares ~320 000 pairs (what 64 orientations are at 1 000 particles x 5
  // CTFs); the conv buffer may then take 1 GiB per pipeline slot instead of 96 MiB.
  int obMax = 64;
  {
    const long long perOrient = (long long) nCTF * nMaps;
    if (perOrient * 64 < 320000)
    {
      obMax = (int) std::min<long long>(2048, ((320000 + perOrient - 1) / perOrient + 63) / 64 * 64);
      ocCap = std::min(partCap, (size_t) (1024u << 20) / (h->Mc * sizeof(float2)));
    }
  }
  int OB = (int) (ocCap / (size_t) nCTF);
  if (OB < 1)
    OB = 1;
  if (OB > obMax)
    OB = obMax;
  if (OB > angO1 - angO0)
    OB = angO1 - angO0;
  h->OB = OB;
  h->maxOC = OB * nCTF;
  h->chunkB = OB > 32 ? OB : 32;

  if (dev_alloc(h, h->dRef, h->Mc * nMaps) || dev_alloc(h, h->dSumRef, nMaps) || dev_alloc(h, h->dSumsqRef, nMaps) ||
      dev_alloc(h, h->dCTF, M * nCTF) || dev_alloc(h, h->dCtfParam, 3 * nCTF) || dev_alloc(h, h->dAngles, nAngles) ||
      dev_alloc(h, h->dPartials, (size_t) nMaps * h->maxOC))
    return 1;
  // the two pipeline slots; slot 0's projection buffers hold chunkB (>= 32) images for the particle uploads
  const size_t scratchFloats = (size_t) ((h->maxOC + 31) & ~31) * ((M + 3) & ~(size_t) 3);
  for (int k = 0; k < 2; k++)
  {
    bioem_hip_ctx::Slot &sl = h->slot[k];
    const size_t nImg = k == 0 ? h->chunkB : h->OB;
    if (dev_alloc(h, sl.projReal, nImg * N * N) || dev_alloc(h, sl.tempDen, nImg) || dev_alloc(h, sl.rowSpec, nImg * M) ||
        dev_alloc(h, sl.specRef, nImg * M) || dev_alloc(h, sl.scratch, scratchFloats) ||
        dev_alloc(h, sl.conv, (size_t) h->maxOC * h->Mc) || dev_alloc(h, sl.params, h->maxOC) ||
        dev_alloc(h, sl.postc, h->maxOC))
      return 1;
    HIP_CHECK(h, hipEventCreateWithFlags(&sl.prepDone, hipEventDisableTiming));
    HIP_CHECK(h, hipEventCreateWithFlags(&sl.cmpDone, hipEventDisableTiming));
    h->slotImages[k] = nImg;
  }
  h->slotRows = (size_t) h->maxOC;
  h->partRows = (size_t) nMaps * h->maxOC;
  if (h->direct)
  {
    if (dev_alloc(h, h->dMapsReal, (size_t) nMaps * N * N) || dev_alloc(h, h->dConvReal, (size_t) h->maxOC * N * N) ||
        dev_alloc(h, h->dDirectZ, (size_t) h->maxOC * M))
      return 1;
    HIP_CHECK(h, hipMemset(h->dMapsReal, 0, sizeof(float) * (size_t) nMaps * N * N));
    HIP_CHECK(h, hipFuncSetAttribute(reinterpret_cast<const void *>(k_compare_direct<3, 8>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int) direct_lds_bytes(N)));
  }
  if (P.nyq && dev_alloc(h, h->dTnyq, (size_t) nMaps * h->maxOC * (2 * P.nyqWD + 1)))
    return 1;
  if (P.tileT)
  {
    const int nT = P.tilesPerAxis;
    std::vector<int> local(P.tileT), rank(2 * mD + 1, 0);
    for (int j = 0; j < P.tileT; j++)
      local[j] = P.gs * (j - P.winD); // sorted local list: the kernel's rows and lanes in the same order
    for (int v = 0; v < P.nd; v++)
      rank[P.disp[v] / P.gs + mD] = v; // visiting rank of window row m in the reference's order
    if (dev_alloc(h, h->dPartTiles, (size_t) nT * nT * nMaps * h->maxOC) || dev_alloc(h, h->dConvShift, (size_t) h->maxOC * M) ||
        upload(h, h->dDispLocal, local.data(), local.size()) || upload(h, h->dRankOfRow, rank.data(), rank.size()) ||
        upload(h, h->dTileCenter, P.tileCenter.data(), nT) || upload(h, h->dTileValid, P.tileValid.data(), nT))
      return 1;
  }
  h->devProbBytes = bioem_hip_prob_size(nMaps, angO1 - angO0, pd->writeAngles);
  h->probBytes = shard ? bioem_hip_prob_size(nMaps, 0, 0) : h->devProbBytes;
  if (dev_alloc(h, h->dProb, h->devProbBytes))
    return 1;

  std::vector<float2> twk; // recombination twiddles of the comparison kernel
  if (P.family == KF_WIDE2)
  { // exp(2 pi i dx k1 / N), dx = (m - mD) gs, laid out per (k1, wave): the NRW window rows a
    // wave folds are contiguous (rows beyond the window: zero)
    const int NRW = P.w2NRW, NWV = P.w2NW, rpw = (P.nd + NWV - 1) / NWV;
    twk.assign((size_t) P.N1 * NWV * NRW, make_float2(0.f, 0.f));
    for (int k1 = 0; k1 < P.N1; k1++)
      for (int w = 0; w < NWV; w++)
        for (int d = 0; d < NRW; d++)
        {
          const int m = w * rpw + d;
          if (m < P.nd)
            twk[((size_t) k1 * NWV + w) * NRW + d] = twiddle((long long) (m - mD) * P.gs * k1, N);
        }
  }
  if (P.family == KF_FASTM2)
  { // k_compare_fastm2<R, NYQ, GS>: [k1 pair s][accumulator a = OFF g + j] = {w^(dx 2s), w^(dx (2s+1))} (two float2)
    // for the LOW-half row dx = (2 OFF g + j - 23) GS (the high half folds the rows OFF further with the same numbers); zero
    // for a k1 beyond N1 - 1 (rows outside the displacement list are masked by their rank in the kernel)
    const int Rl = 2 * P.halfR, off = fastm2_off(Rl, P.gs), nAcc = fastm2_acc(Rl, P.gs);
    const int nS = (P.N1 + 1) / 2;
    twk.assign((size_t) nS * nAcc * 2, make_float2(0.f, 0.f));
    for (int s2 = 0; s2 < nS; s2++)
      for (int ac = 0; ac < nAcc; ac++)
      {
        const long long dx = (long long) (2 * off * (ac / off) + (ac % off) - kFm2WD) * P.gs;
        for (int e = 0; e < 2; e++)
          if (2 * s2 + e < P.N1)
            twk[((size_t) s2 * nAcc + ac) * 2 + e] = twiddle(dx * (2 * s2 + e), N);
      }
    // B operand of the matrix pass: lane l of k-step K, column tile ct supplies (l / 16 odd ? sin : cos)(2 pi ky dy / N),
    // ky = 2 K + l / 32, dy = (16 ct + l % 16 - 23) GS -- the float twiddles exp(2 pi i k / N) every kernel uses
    std::vector<float> bt(fastm2_btab_floats(h->H, P.nyq));
    for (size_t K = 0; K < bt.size() / 192; K++)
      for (int ct = 0; ct < 3; ct++)
        for (int l = 0; l < 64; l++)
        {
          const long long ky = 2 * (long long) K + (l >> 5), dy = (long long) (16 * ct + (l & 15) - kFm2WD) * P.gs;
          const float2 w = twiddle(ky * dy, N);
          bt[(K * 3 + ct) * 64 + l] = ((l >> 4) & 1) ? w.y : w.x;
        }
    if (upload(h, h->dBtab, bt.data(), bt.size()))
      return 1;
  }
  if (P.family == KF_FAST || P.family == KF_FASTM || P.family == KF_ROWS || P.family == KF_ODDFFT)
  { // the window kernels
    const int NW = 2 * P.winD + 1;
    // [N1][2 winD + 1], d = -winD..winD; k_compare_rows: a "register FFT" of length 1, one table row per kx;
    // k_compare_oddfft: N1 = N / oddR
    const int nK1 = P.family == KF_ROWS ? N : P.N1;
    twk.resize((size_t) nK1 * NW);
    for (int k1 = 0; k1 < nK1; k1++)
      for (int d = -P.winD; d <= P.winD; d++)
        twk[(size_t) k1 * NW + d + P.winD] = twiddle((long long) d * P.gs * k1, N);
  }
  if (!twk.empty() && upload(h, h->dTwk, twk.data(), twk.size()))
    return 1;
  if (P.nyq)
  { // Nyquist pre-kernel (every family with the split): per (k1, k2 pair) the 2*nyqWD+1 twiddle pairs w^(kx0 m gs),
    // w^(kx1 m gs), contiguous
    const int NW = 2 * P.nyqWD + 1, R2 = P.halfR;
    std::vector<float2> twn((size_t) (N / 2) * NW * 2);
    for (int k1 = 0; k1 < P.N1; k1++)
      for (int k2p = 0; k2p < R2; k2p++)
        for (int m = -P.nyqWD; m <= P.nyqWD; m++)
          for (int e = 0; e < 2; e++)
          {
            const long long kx = (long long) P.N1 * (2 * k2p + e) + k1;
            twn[(((size_t) (k1 * R2 + k2p) * NW) + (m + P.nyqWD)) * 2 + e] = twiddle(kx * m * P.gs, N);
          }
    if (upload(h, h->dTwNyq, twn.data(), twn.size()))
      return 1;
  }
  std::vector<float2> tw(N + 1);
  std::vector<double2> twd(N);
  for (int k = 0; k <= N; k++)
    tw[k] = twiddle(k, N);
  if (P.family == KF_FAST && sym_window_ok(P.winD, 2 * P.halfR, P.nyq, P.gs))
  { // window pass over |dy| (compare_args.hpp): cos | sin (2 pi ky j gs / N) per column pair, j = 0..10, behind the
    // twiddles; whole column blocks (the columns beyond H meet zeros of T, entry 11 is never used: zeros)
    const size_t nPairs = (size_t) ((h->H + 63) / 64) * 32;
    tw.resize(sym_table_offset(N) + nPairs * kSymEntries * 2, make_float2(0.f, 0.f));
    for (size_t kp = 0; kp < nPairs; kp++)
      for (int j = 0; j <= 10; j++)
        for (int e = 0; e < 2; e++)
          tw[sym_table_offset(N) + (kp * kSymEntries + j) * 2 + e] = twiddle((long long) (2 * kp + e) * j * P.gs, N);
  }
  for (int k = 0; k < N; k++)
    twd[k] = twiddle_d(k, N);
  // log table: bin i of the mantissa interval [1,2): c = 1/centre, entry {c, -log(c)}
  std::vector<double2> lt(64);
  for (int i = 0; i < 64; i++)
  {
    const double c = 1.0 / (1.0 + ((double) i + 0.5) / 64.0);
    lt[i] = make_double2(c, -log(c));
  }
  if (upload(h, h->dTw, tw.data(), tw.size()) || upload(h, h->dTwD, twd.data(), twd.size()) ||
      upload(h, h->dDisp, P.disp.data(), P.disp.size()) || upload(h, h->dLtab, lt.data(), lt.size()))
    return 1;
  // BIOEM_SIGNATURE_LOG=<file>: one line per handle with the comparison-kernel instantiations its launches will use
  // (scripts/check_kernel_coverage.py holds the lines of a test run against the kernels in the code object)
  if (const char *lg = getenv("BIOEM_SIGNATURE_LOG"))
    if (FILE *f = fopen(lg, "a"))
    {
      fprintf(f, "%s\n", bioem_hip_kernel_signature(h));
      if (P.nyq)
        fprintf(f, "k_nyquist_rows<%d, %d>\n", P.nyqWD, h->nMaps <= 64 ? 4 : 1);
      fclose(f);
    }
  return 0;
}

int bioem_hip_create(bioem_hip_handle *out, int device, const bioem_hip_param_device *pd, int nMaps, int nAngles,
                     int nCTF, int algo)
{
  return create_impl(out, device, pd, nMaps, nAngles, nCTF, algo, false, 0, nAngles);
}

int bioem_hip_create_shard(bioem_hip_handle *out, int device, const bioem_hip_param_device *pd, int nMaps, int nAngles,
                           int nCTF, int algo, int iOrientBegin, int iOrientEnd)
{
  return create_impl(out, device, pd, nMaps, nAngles, nCTF, algo, true, iOrientBegin, iOrientEnd);
}

int bioem_hip_destroy(bioem_hip_handle h)
{
  if (!h)
    return 0;
  hipSetDevice(h->device);
  if (h->stream)
    hipStreamSynchronize(h->stream);
  drain_events(h);
  drain_phases(h);
  for (hipEvent_t e : h->evPool)
    hipEventDestroy(e);
  if (h->prepStream)
    hipStreamSynchronize(h->prepStream);
  for (const bioem_hip_ctx::Alloc &al : h->allocs)
    if (al.pinned)
      hipHostFree(al.p);
    else
      hipFree(al.p);
  for (int k = 0; k < 2; k++)
    for (hipEvent_t e : {h->slot[k].prepDone, h->slot[k].cmpDone, h->ring[k].staged})
      if (e)
        hipEventDestroy(e);
  if (h->copyStream)
    hipStreamDestroy(h->copyStream);
  if (h->prepStream)
    hipStreamDestroy(h->prepStream);
  if (h->stream)
    hipStreamDestroy(h->stream);
  delete h;
  return 0;
}

int bioem_hip_upload_particles(bioem_hip_handle h, const float *refFFT, const float *sum, const float *sumsq)
{
  HIP_CHECK(h, hipSetDevice(h->device));
  if (h->direct)
  {
    h->err = "BIOEM_CC_DIRECT needs the particle images: bioem_hip_upload_particle_maps";
    return 2;
  }
  const size_t M = (size_t) h->M;
  bioem_hip_ctx::Slot &s0 = h->slot[0]; // the images pass through slot 0
  void_slot(s0);
  HIP_CHECK(h, hipMemcpyAsync(h->dSumRef, sum, sizeof(float) * h->nMaps, hipMemcpyHostToDevice, h->stream));
  HIP_CHECK(h, hipMemcpyAsync(h->dSumsqRef, sumsq, sizeof(float) * h->nMaps, hipMemcpyHostToDevice, h->stream));
  for (int b = 0; b < h->nMaps; b += h->chunkB)
  {
    const int n = std::min(h->chunkB, h->nMaps - b);
    HIP_CHECK(h, hipMemcpyAsync(s0.specRef, refFFT + 2 * M * (size_t) b, sizeof(float2) * M * n,
                                hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_reorder, dim3(1024), dim3(256), 0, h->stream, s0.specRef, h->dRef + h->Mc * (size_t) b, n, h->N,
                       h->H, h->plan.halfR, h->plan.N1, h->Hp);
    HIP_CHECK(h, hipGetLastError());
    HIP_CHECK(h, hipStreamSynchronize(h->stream));
  }
  h->refUp = true;
  return 0;
}

int bioem_hip_upload_particle_maps(bioem_hip_handle h, const float *maps)
{
  HIP_CHECK(h, hipSetDevice(h->device));
  const int N = h->N;
  bioem_hip_ctx::Slot &s0 = h->slot[0]; // the transforms pass through slot 0
  void_slot(s0);
  float *dMaps = nullptr;
  HIP_CHECK(h, hipMalloc(&dMaps, sizeof(float) * (size_t) h->chunkB * N * N));
  std::unique_ptr<float, hipError_t (*)(void *)> freeMaps(dMaps, hipFree); // scratch: freed on every return
  for (int b = 0; b < h->nMaps; b += h->chunkB)
  {
    const int n = std::min(h->chunkB, h->nMaps - b);
    HIP_CHECK(h, hipMemcpyAsync(dMaps, maps + (size_t) b * N * N, sizeof(float) * (size_t) n * N * N,
                                hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_map_sums, dim3(n), dim3(256), 0, h->stream, dMaps, N * N, h->dSumRef + b, h->dSumsqRef + b);
    HIP_CHECK(h, hipGetLastError());
    if (h->direct)
      HIP_CHECK(h, hipMemcpyAsync(h->dMapsReal + (size_t) b * N * N, dMaps, sizeof(float) * (size_t) n * N * N,
                                  hipMemcpyDeviceToDevice, h->stream));
    if (run_r2c(h, s0, h->stream, nullptr, dMaps, n))
      return 1;
    hipLaunchKernelGGL(k_reorder, dim3(1024), dim3(256), 0, h->stream, s0.specRef, h->dRef + h->Mc * (size_t) b, n, N,
                       h->H, h->plan.halfR, h->plan.N1, h->Hp);
    HIP_CHECK(h, hipGetLastError());
    HIP_CHECK(h, hipStreamSynchronize(h->stream));
  }
  h->refUp = true;
  return 0;
}

int bioem_hip_upload_ctf(bioem_hip_handle h, const float *refCTF, const float *ctfParam3)
{
  HIP_CHECK(h, hipSetDevice(h->device));
  HIP_CHECK(h, hipMemcpy(h->dCTF, refCTF, sizeof(float2) * (size_t) h->M * h->nCTF, hipMemcpyHostToDevice));
  HIP_CHECK(h, hipMemcpy(h->dCtfParam, ctfParam3, sizeof(float) * 3 * h->nCTF, hipMemcpyHostToDevice));
  h->ctfUp = true;
  return 0;
}

int bioem_hip_upload_model(bioem_hip_handle h, const bioem_hip_model_point *pts, int nPts, float NormDen,
                           float pixelSize, int shiftX, int shiftY)
{
  HIP_CHECK(h, hipSetDevice(h->device));
  if (h->dVolC)
  { // the points replace a volume model: nothing queued may still read it
    HIP_CHECK(h, hipDeviceSynchronize());
    dev_release(h, h->dVolC);
    dev_release(h, h->dVolA); // (bioem_hip_volume_gradient's A beside C goes with the volume)
    h->volPad = h->volAPad = 0;
    void_slot(h->slot[0]); // (what a slot holds staged are slices of the volume)
    void_slot(h->slot[1]);
  }
  dev_release(h, h->dPts);
  if (upload(h, h->dPts, pts, (size_t) nPts))
    return 1;
  h->nPts = nPts;
  h->NormDen = NormDen;
  h->pixelSize = pixelSize;
  h->shiftX = shiftX;
  h->shiftY = shiftY;
  h->iradMax = 0;
  for (int n = 0; n < nPts; n++)
    if (pts[n].radius > pixelSize)
      h->iradMax = std::max(h->iradMax, (int) (pts[n].radius / pixelSize) + 1);
  h->modelRadius = 0.;
  for (int n = 0; n < nPts; n++)
    h->modelRadius = std::max(h->modelRadius, std::sqrt((double) pts[n].pos[0] * pts[n].pos[0] + (double) pts[n].pos[1] * pts[n].pos[1] +
                                                        (double) pts[n].pos[2] * pts[n].pos[2]));
  dev_release(h, h->dStamp);
  const size_t cells = (size_t) nPts * (2 * h->iradMax + 1) * (2 * h->iradMax + 1);
  if (h->iradMax <= 16 && nPts > 0 && cells <= ((size_t) 1 << 27)) // at most 1 GiB of footprints, else k_project
  {
    if (dev_alloc(h, h->dStamp, cells))
      return 1;
    hipLaunchKernelGGL(k_project_stamps, dim3((unsigned) ((cells + 255) / 256)), dim3(256), 0, h->stream, h->dPts, nPts,
                       h->iradMax, pixelSize, h->dStamp);
    HIP_CHECK(h, hipGetLastError());
    HIP_CHECK(h, hipStreamSynchronize(h->stream));
  }
  return 0;
}

int bioem_hip_upload_orientations(bioem_hip_handle h, const float *angles4, int n, int isQuat)
{
  HIP_CHECK(h, hipSetDevice(h->device));
  if (n > h->nAngles)
  {
    h->err = "more orientations than the handle was created for";
    return 2;
  }
  HIP_CHECK(h, hipMemcpy(h->dAngles, angles4, sizeof(float4) * (size_t) n, hipMemcpyHostToDevice));
  h->nAnglesUp = n;
  h->isQuat = isQuat;
  // k_project_box relies on the rotated model staying inside its box: the reference's quaternion matrix
  // (bioem.cpp:1632-1646) is a rotation only for unit quaternions; project_batch holds the list's largest deviation
  // against the model's extent and sends a list that stretches the model by a fraction of a pixel to the band kernel
  h->quatNormDev = 0.;
  if (isQuat)
    for (int k = 0; k < n; k++)
    {
      const float *q = angles4 + 4 * (size_t) k;
      const double n2 = (double) q[0] * q[0] + (double) q[1] * q[1] + (double) q[2] * q[2] + (double) q[3] * q[3];
      const double dev = std::fabs(n2 - 1.0);
      h->quatNormDev = dev == dev ? std::max(h->quatNormDev, dev) : 1e30; // (a NaN never passes)
    }
  return 0;
}

// the common path of the two uploads: `what` names the entry in messages
static int upload_own_lists(bioem_hip_handle h, const float *angles4, const long long *offsets, int isQuat, const char *what)
{
  const KernelPlan &P = h->plan;
  auto refuse = [&](const char *why) {
    h->err = std::string(what) + ": " + why;
    return 2;
  };
  if (P.tileT || h->direct || h->shard)
    return refuse(P.tileT    ? "the own-list pass does not take tiled wide windows"
                  : h->direct ? "the own-list pass does not take BIOEM_CC_DIRECT handles"
                              : "the own-list pass does not take shard handles");
  if (!angles4 || !offsets)
    return refuse("null argument");
  if (offsets[0] != 0)
    return refuse("offsets[0] must be 0");
  int K = 0;
  for (int p = 0; p < h->nMaps; p++)
  {
    const long long len = offsets[p + 1] - offsets[p];
    if (len < 0)
      return refuse("offsets must not decrease");
    if (len > h->nAngles)
      return refuse("a list is longer than nAngles of the handle");
    K = std::max(K, (int) len);
  }
  const long long nSlots = offsets[h->nMaps];
  if (nSlots < 1)
    return refuse("the lists are all empty");
  if (nSlots * h->nCTF > 0x7fffffffLL)
    return refuse("more than 2^31 (particle, list entry, CTF) rows");
  // slots per batch: the preparation is the long pole of this pass (a conv spectrum meets ONE particle), so a batch
  // holds up to 1 024 slots (conv buffer <= 1 GiB per pipeline slot) whatever the all-to-all batch of the handle is
  const long long convCap = (long long) ((size_t) (1024u << 20) / (h->Mc * sizeof(float2))) / h->nCTF;
  const int ownOB = (int) std::min<long long>(nSlots, std::max<long long>(h->OB, std::min<long long>(1024, convCap)));
  const size_t rows = (size_t) ownOB * h->nCTF, M = (size_t) h->M, N = (size_t) h->N;
  // nothing queued may still use the buffers that are replaced
  HIP_CHECK(h, hipStreamSynchronize(h->prepStream));
  HIP_CHECK(h, hipStreamSynchronize(h->stream));
  // grow what is too small: every new buffer first, the old ones go when all of them exist -- a failed allocation
  // (return 1) leaves the handle as it was
  {
    struct Grown
    {
      double *projReal = nullptr, *tempDen = nullptr;
      double2 *rowSpec = nullptr, *postc = nullptr;
      float2 *specRef = nullptr, *conv = nullptr;
      bioem_hip_param5 *params = nullptr;
    } g[2];
    Partial *partials = nullptr;
    float *tnyq = nullptr;
    const bool growRows = h->slotRows < rows, growPart = h->partRows < rows;
    bool ok = true;
    for (int k = 0; k < 2 && ok; k++)
    {
      if (h->slotImages[k] < (size_t) ownOB)
        ok = !dev_alloc(h, g[k].projReal, (size_t) ownOB * N * N) && !dev_alloc(h, g[k].tempDen, (size_t) ownOB) &&
             !dev_alloc(h, g[k].rowSpec, (size_t) ownOB * M) && !dev_alloc(h, g[k].specRef, (size_t) ownOB * M);
      if (ok && growRows)
        ok = !dev_alloc(h, g[k].conv, rows * h->Mc) && !dev_alloc(h, g[k].params, rows) && !dev_alloc(h, g[k].postc, rows);
    }
    if (ok && growPart)
      ok = !dev_alloc(h, partials, rows) && (!P.nyq || !dev_alloc(h, tnyq, rows * (size_t) (2 * P.nyqWD + 1)));
    if (!ok)
    {
      for (Grown &x : g)
      {
        dev_release(h, x.projReal);
        dev_release(h, x.tempDen);
        dev_release(h, x.rowSpec);
        dev_release(h, x.specRef);
        dev_release(h, x.conv);
        dev_release(h, x.params);
        dev_release(h, x.postc);
      }
      dev_release(h, partials);
      dev_release(h, tnyq);
      return 1;
    }
    for (int k = 0; k < 2; k++)
    {
      bioem_hip_ctx::Slot &sl = h->slot[k];
      if (g[k].projReal)
      {
        void_slot(sl);
        dev_release(h, sl.projReal);
        dev_release(h, sl.tempDen);
        dev_release(h, sl.rowSpec);
        dev_release(h, sl.specRef);
        sl.projReal = g[k].projReal;
        sl.tempDen = g[k].tempDen;
        sl.rowSpec = g[k].rowSpec;
        sl.specRef = g[k].specRef;
        h->slotImages[k] = (size_t) ownOB;
      }
      if (g[k].conv)
      {
        void_slot(sl);
        dev_release(h, sl.conv);
        dev_release(h, sl.params);
        dev_release(h, sl.postc);
        sl.conv = g[k].conv;
        sl.params = g[k].params;
        sl.postc = g[k].postc;
      }
    }
    if (growRows)
      h->slotRows = rows;
    if (growPart)
    { // (one partial, one set of Nyquist rows per conv row in this pass)
      dev_release(h, h->dPartials);
      dev_release(h, h->dTnyq);
      h->dPartials = partials;
      h->dTnyq = tnyq;
      h->partRows = rows;
    }
  }
  if ((size_t) nSlots > h->ownSlotCap || !h->dOwnOff)
  {
    float4 *lists = nullptr;
    int *slotP = nullptr, *doff = nullptr;
    if (dev_alloc(h, lists, (size_t) nSlots) || dev_alloc(h, slotP, (size_t) nSlots) ||
        (!h->dOwnOff && dev_alloc(h, doff, (size_t) h->nMaps + 1)))
    {
      dev_release(h, lists);
      dev_release(h, slotP);
      dev_release(h, doff);
      return 1;
    }
    dev_release(h, h->dOwnAngles);
    dev_release(h, h->dSlotParticle);
    h->dOwnAngles = lists;
    h->dSlotParticle = slotP;
    if (doff)
      h->dOwnOff = doff;
    h->ownSlotCap = (size_t) nSlots;
    h->ownOff.clear();
  }
  std::vector<int> off(h->nMaps + 1), slotP((size_t) nSlots);
  for (int p = 0; p <= h->nMaps; p++)
    off[p] = (int) offsets[p];
  for (int p = 0; p < h->nMaps; p++)
    for (int s = off[p]; s < off[p + 1]; s++)
      slotP[s] = p;
  h->ownOff.clear(); // (no lists until every piece is in place)
  HIP_CHECK(h, hipMemcpy(h->dOwnAngles, angles4, sizeof(float4) * (size_t) nSlots, hipMemcpyHostToDevice));
  HIP_CHECK(h, hipMemcpy(h->dOwnOff, off.data(), sizeof(int) * off.size(), hipMemcpyHostToDevice));
  HIP_CHECK(h, hipMemcpy(h->dSlotParticle, slotP.data(), sizeof(int) * slotP.size(), hipMemcpyHostToDevice));
  h->ownOff.swap(off);
  h->ownK = K;
  h->ownOB = ownOB;
  h->ownIsQuat = isQuat;
  h->ownQuatNormDev = 0.; // (see bioem_hip_upload_orientations)
  if (isQuat)
    for (long long k = 0; k < nSlots; k++)
    {
      const float *q = angles4 + 4 * (size_t) k;
      const double n2 = (double) q[0] * q[0] + (double) q[1] * q[1] + (double) q[2] * q[2] + (double) q[3] * q[3];
      const double dev = std::fabs(n2 - 1.0);
      h->ownQuatNormDev = dev == dev ? std::max(h->ownQuatNormDev, dev) : 1e30;
    }
  // the block table of a pass over all particles (another range builds its own at the call)
  h->ownTabP0 = h->ownTabP1 = -1;
  if (h->ownFn && own_block_table(h, 0, h->nMaps))
  {
    h->ownOff.clear();
    return 1;
  }
  // BIOEM_SIGNATURE_LOG: the kernels of the single launch, where the pass of this handle will use them
  if (h->ownFn)
    if (const char *lg = getenv("BIOEM_SIGNATURE_LOG"))
      if (FILE *f = fopen(lg, "a"))
      {
        fprintf(f, "%s\n", bioem_hip_own_kernel_signature(h));
        if (P.nyq)
          fprintf(f, "k_nyquist_rows_own<%d>\n", P.nyqWD);
        fclose(f);
      }
  return 0;
}

int bioem_hip_upload_particle_orientation_lists(bioem_hip_handle h, const float *angles4, const long long *offsets, int isQuat)
{
  HIP_CHECK(h, hipSetDevice(h->device));
  return upload_own_lists(h, angles4, offsets, isQuat, "upload_particle_orientation_lists");
}

// lists of one length K: offsets[p] = p K of the same path
int bioem_hip_upload_particle_orientations(bioem_hip_handle h, const float *angles4, int K, int isQuat)
{
  HIP_CHECK(h, hipSetDevice(h->device));
  const KernelPlan &P = h->plan;
  if (!(P.tileT || h->direct || h->shard) && (!angles4 || K < 1 || K > h->nAngles))
  {
    h->err = "upload_particle_orientations: need 1 <= K <= nAngles of the handle";
    return 2;
  }
  std::vector<long long> offsets((size_t) h->nMaps + 1);
  for (int p = 0; p <= h->nMaps; p++)
    offsets[p] = (long long) p * K;
  return upload_own_lists(h, angles4, offsets.data(), isQuat, "upload_particle_orientations");
}

int bioem_hip_set_own_launch(bioem_hip_handle h, int mode)
{
  if (!h)
    return 2;
  if (mode != BIOEM_HIP_OWN_LAUNCH_BATCH && mode != BIOEM_HIP_OWN_LAUNCH_PARTICLE && mode != BIOEM_HIP_OWN_LAUNCH_BATCH_ROWS)
  {
    h->err = "set_own_launch: unknown mode";
    return 2;
  }
  h->ownFn = mode == BIOEM_HIP_OWN_LAUNCH_PARTICLE ? nullptr : h->ownFnPlan;
  h->ownXcdOrder = mode != BIOEM_HIP_OWN_LAUNCH_BATCH_ROWS;
  h->ownTabP0 = h->ownTabP1 = -1; // the block table follows at the next pass
  return 0;
}

// lean = 0: the full instantiations only; 1 (the default of every handle): the lean variant of k_compare_fast where a launch
// qualifies.  Returns 1 if the launches of this handle -- its plan, its shape, the tiles of a tiled plan -- now take a lean
// kernel, else 0 (BIOEM_NO_SPLIT_LAST as it reads now; a launch reads it again).
int bioem_hip_set_compare_variant(bioem_hip_handle h, int lean)
{
  if (!h)
    return 0;
  h->lean = lean != 0;
  const KernelPlan &P = h->plan;
  return lean_launch_ok(h, P.tileT ? P.tileT : P.nd, P.tileT ? P.winD * P.gs : h->pd.maxDisplaceCenter, last_block_split(h)) ? 1 : 0;
}

int bioem_hip_compare_own_orientations(bioem_hip_handle h, int iMapBegin, int iMapEnd)
{
  HIP_CHECK(h, hipSetDevice(h->device));
  if (!h->dOwnAngles || h->ownOff.empty())
  {
    h->err = "compare_own_orientations: no per-particle orientation lists (bioem_hip_upload_particle_orientations)";
    return 2;
  }
  if (!has_model(h) || iMapBegin < 0 || iMapEnd > h->nMaps || iMapBegin > iMapEnd)
  {
    h->err = "compare_own_orientations: model not uploaded or particle range invalid";
    return 2;
  }
  if (compat_flush(h)) // rows staged through the reference-compatible entry go first (call order)
    return 1;
  if (h->ownOff[iMapBegin] == h->ownOff[iMapEnd]) // (no particle, or empty lists only)
    return 0;
  if (h->ownFn && (h->ownTabP0 != iMapBegin || h->ownTabP1 != iMapEnd) && own_block_table(h, iMapBegin, iMapEnd))
    return 1;
  return run_pipeline(h, own_batches(h, iMapBegin, iMapEnd), 0, h->nCTF, true);
}

void *bioem_hip_host_alloc(size_t size)
{
  void *p = nullptr;
  if (hipHostMalloc(&p, size, hipHostMallocDefault) != hipSuccess)
    return nullptr;
  return p;
}

void bioem_hip_host_free(void *ptr)
{
  if (ptr)
    hipHostFree(ptr);
}

int bioem_hip_start_run(bioem_hip_handle h, const void *pProb_host)
{
  HIP_CHECK(h, hipSetDevice(h->device));
  HIP_CHECK(h, hipMemcpyAsync(h->dProb, pProb_host, h->probBytes, hipMemcpyHostToDevice, h->stream));
  if (h->shard && h->pd.writeAngles)
  { // the shard's angle table is initialised where it lives (bioem.cpp:688-697)
    bioem_hip_prob_angle *pang = reinterpret_cast<bioem_hip_prob_angle *>(h->dProb + sizeof(bioem_hip_prob_map) * h->nMaps);
    hipLaunchKernelGGL(k_init_angles, dim3(1024), dim3(256), 0, h->stream, pang, (size_t) (h->angO1 - h->angO0) * h->nMaps);
    HIP_CHECK(h, hipGetLastError());
  }
  if (h->dCtfTab)
  {
    hipLaunchKernelGGL(k_init_ctf_table, dim3(256), dim3(256), 0, h->stream, h->dCtfTab, (size_t) h->nCTF * h->nMaps);
    HIP_CHECK(h, hipGetLastError());
  }
  HIP_CHECK(h, hipStreamSynchronize(h->stream));
  h->inRun = true;
  return 0;
}

int bioem_hip_enable_ctf_table(bioem_hip_handle h, int on)
{
  if (!h)
    return 2;
  if (h->inRun)
  {
    h->err = "enable_ctf_table: called inside a run (between bioem_hip_start_run and bioem_hip_finish_run)";
    return 2;
  }
  HIP_CHECK(h, hipSetDevice(h->device));
  if (!on)
  {
    HIP_CHECK(h, hipStreamSynchronize(h->stream));
    dev_release(h, h->dCtfTab);
    return 0;
  }
  if (h->dCtfTab)
    return 0;
  if (dev_alloc(h, h->dCtfTab, (size_t) h->nCTF * h->nMaps))
    return 1;
  // a table fetched before the first run reads as an untouched one
  hipLaunchKernelGGL(k_init_ctf_table, dim3(256), dim3(256), 0, h->stream, h->dCtfTab, (size_t) h->nCTF * h->nMaps);
  HIP_CHECK(h, hipGetLastError());
  return 0;
}

int bioem_hip_ctf_table(bioem_hip_handle h, bioem_hip_prob_map *out)
{
  if (!h)
    return 2;
  if (!h->dCtfTab || !out)
  {
    h->err = "ctf_table: the table is not enabled on this handle (bioem_hip_enable_ctf_table)";
    return 2;
  }
  HIP_CHECK(h, hipSetDevice(h->device));
  if (compat_flush(h))
    return 1;
  HIP_CHECK(h, hipMemcpyAsync(out, h->dCtfTab, sizeof(bioem_hip_prob_map) * h->nCTF * h->nMaps, hipMemcpyDeviceToHost,
                              h->stream));
  HIP_CHECK(h, hipStreamSynchronize(h->stream));
  return 0;
}

int bioem_hip_compare(bioem_hip_handle h, int iPipeline, int iOrient, int iConvStart, int maxParallelConv,
                      int nTotParallelConv, const float *conv_mapsFFT, const bioem_hip_param5 *comp_params)
{
  HIP_CHECK(h, hipSetDevice(h->device));
  const size_t M = (size_t) h->M;
  if (maxParallelConv < 1 || maxParallelConv > nTotParallelConv || iOrient < h->angO0 || iOrient >= h->angO1 ||
      iConvStart < 0 || iConvStart + maxParallelConv > h->nCTF)
  {
    h->err = "bioem_hip_compare: orientation / convolution range out of bounds";
    return 2;
  }
  if (compat_alloc(h))
    return 1;
  const int k = (iPipeline & 1) * nTotParallelConv; // bioem.cpp:1388
  // with WRITE_PROB_ANGLES every orientation of a launch must be one run of rows: an orientation that returns after
  // another one was staged starts a new launch
  bool seen = false, last = !h->ringOrients.empty() && h->ringOrients.back() == iOrient;
  for (int o : h->ringOrients)
    seen = seen || o == iOrient;
  if (seen && !last && compat_flush(h))
    return 1;
  int done = 0;
  while (done < maxParallelConv)
  {
    if (h->ringCount == h->ringCap && compat_flush(h))
      return 1;
    const int half = h->ringHalf;
    bioem_hip_ctx::CompatHalf &r = h->ring[half];
    bioem_hip_ctx::Slot &sl = h->slot[half];
    if (h->ringCount == 0 && sl.cmpPending)
    { // the launch that last used this half (two flushes ago) must have consumed its staged rows
      HIP_CHECK(h, hipEventSynchronize(sl.cmpDone));
      sl.cmpPending = false;
    }
    const int row0 = h->ringCount;
    const int n = std::min(maxParallelConv - done, h->ringCap - row0);
    // the caller's slot is free again when this returns (bioem_cuda.cu:539-561 makes the caller wait instead)
    memcpy(r.hConv + M * row0, conv_mapsFFT + 2 * M * (size_t) (k + done), sizeof(float2) * M * n);
    for (int i = 0; i < n; i++)
    {
      r.hPar[row0 + i] = comp_params[k + done + i];
      r.hIds[row0 + i] = make_int2(iOrient, iConvStart + done + i);
    }
    HIP_CHECK(h, hipMemcpyAsync(r.dStage + M * row0, r.hConv + M * row0, sizeof(float2) * M * n, hipMemcpyHostToDevice,
                                h->copyStream));
    if (h->ringOrients.empty() || h->ringOrients.back() != iOrient)
      h->ringOrients.push_back(iOrient);
    h->ringCount += n;
    done += n;
  }
  // launch when the half is full -- or earlier when the device has nothing left to do and a launch's worth of rows
  // (32 x nMaps comparisons) is waiting: keeps the GPU busy while a short run ramps up
  bool launch = h->ringCount == h->ringCap;
  if (!launch && h->ringCount >= 32)
  {
    const bioem_hip_ctx::Slot &other = h->slot[h->ringHalf ^ 1];
    launch = !other.cmpPending || hipEventQuery(other.cmpDone) == hipSuccess;
  }
  if (launch && compat_flush(h))
    return 1;
  return 0;
}

int bioem_hip_project_convolve_compare(bioem_hip_handle h, int iOrientBegin, int iOrientEnd)
{
  return bioem_hip_project_convolve_compare_ctf(h, iOrientBegin, iOrientEnd, 0, h ? h->nCTF : 0);
}

int bioem_hip_project_convolve_compare_ctf(bioem_hip_handle h, int iOrientBegin, int iOrientEnd, int iConvBegin,
                                           int iConvEnd)
{
  HIP_CHECK(h, hipSetDevice(h->device));
  if (!has_model(h) || iOrientBegin < 0 || iOrientEnd > h->nAnglesUp || iOrientBegin > iOrientEnd || iConvBegin < 0 ||
      iConvEnd > h->nCTF || iConvBegin >= iConvEnd)
  {
    h->err = "project_convolve_compare: model/orientations not uploaded or range invalid";
    return 2;
  }
  if (iOrientBegin < iOrientEnd && (iOrientBegin < h->angO0 || iOrientEnd > h->angO1))
  {
    h->err = "project_convolve_compare: orientations outside the range this shard handle was created for";
    return 2;
  }
  const int nC = iConvEnd - iConvBegin;
  if (compat_flush(h)) // rows staged through the reference-compatible entry go first (call order)
    return 1;
  // two-slot pipeline: projection + convolution of batch b+1 run on prepStream while batch b is compared
  // orientations per batch: the handle's capacity, but at least six batches per call where that leaves 64 or more per
  // batch -- the preparation of batch b+1 hides behind the comparison of batch b, the first batch's does not
  // (20 particles x 2 304 orientations in 3 batches of 1 060: 11.5 ms per pass, a third of it the exposed first batch;
  // a ramp -- first batches a quarter and a half of the rest -- was measured too: 8.9 against 8.5 ms, more launches
  // cost more than the shorter exposed preparation saves)
  // ... as long as a batch still compares 33 000 ... 65 000 pairs (a job of 23 000 pairs -- BASELINE config 1 -- is one batch:
  // 0.46 ms against 0.57 ms in two)
  // (round 4, with the preparation 2.5x faster than when 32 768 was chosen: 65 536 pairs per batch at least for small
  // images -- 128^2 x 10 particles x 4 608 orientations 63.7 -> 66.2 M/s, x 1 152: 52.5 -> 57.5; 131 072 the same,
  // 16 384 and less lose; at 224^2 32 768 stays: 10 particles 28.6 against 27.3 M/s with 65 536)
  const long long minPairs = h->N <= 160 ? 65536 : 32768;
  const int perBatch = (int) std::min<long long>(h->OB, (minPairs + (long long) nC * h->nMaps - 1) / ((long long) nC * h->nMaps));
  const int OBc = std::min(h->OB, std::max(std::max(64, perBatch), (iOrientEnd - iOrientBegin + 5) / 6));
  // (Round 4 measured batches that shrink towards the END as well -- a half, a quarter of the regular size, so that
  // the last comparison, which nothing overlaps, is short: 7.12 -> 7.66 ms per pass at 20 particles, 0.58 -> 0.74 ms
  // for the config-1 shape.  Equal batches it is.)
  std::vector<int> first; // first orientation of every batch, and the end
  for (int o = iOrientBegin; o < iOrientEnd; o += OBc)
    first.push_back(o);
  first.push_back(iOrientEnd);
  return run_pipeline(h, first, iConvBegin, nC, false);
}

// ---- the three stages of the loop body as separate, asynchronous, batched entries (device-resident hand-over) ----
int bioem_hip_project(bioem_hip_handle h, int iPipeline, int iOrientBegin, int iOrientEnd)
{
  HIP_CHECK(h, hipSetDevice(h->device));
  const int nO = iOrientEnd - iOrientBegin;
  if (!has_model(h) || iOrientBegin < 0 || iOrientEnd > h->nAnglesUp || nO < 1)
  {
    h->err = "bioem_hip_project: model/orientations not uploaded or range invalid";
    return 2;
  }
  if (iOrientBegin < h->angO0 || iOrientEnd > h->angO1)
  {
    h->err = "bioem_hip_project: orientations outside the range this shard handle was created for";
    return 2;
  }
  if (nO > h->OB)
  {
    char buf[160];
    snprintf(buf, sizeof(buf), "bioem_hip_project: at most %d orientations per call with this configuration", h->OB);
    h->err = buf;
    return 2;
  }
  if (compat_flush(h)) // rows staged through the reference-compatible entry go first (call order)
    return 1;
  // the comparison that last read this buffer set goes first (NOT the other set's: that one is what this call overlaps);
  // with none queued, whatever the main stream holds so far (start_run, debug hooks, the compat entry)
  bioem_hip_ctx::Slot &sl = h->slot[iPipeline & 1];
  if (!sl.cmpPending)
    HIP_CHECK(h, hipEventRecord(sl.cmpDone, h->stream));
  HIP_CHECK(h, hipStreamWaitEvent(h->prepStream, sl.cmpDone, 0));
  sl.cmpPending = false;
  void_slot(sl);
  if (phase_begin(h, h->prepStream, BIOEM_HIP_PHASE_PROJECTION, iOrientBegin, iOrientEnd, 0, 0) ||
      project_batch(h, sl, h->prepStream, shared_list(h), iOrientBegin, nO) || phase_end(h, h->prepStream))
    return 1;
  sl.stageO0 = iOrientBegin;
  sl.stageNO = nO;
  return 0;
}

int bioem_hip_convolve(bioem_hip_handle h, int iPipeline, int iConvBegin, int iConvEnd)
{
  HIP_CHECK(h, hipSetDevice(h->device));
  bioem_hip_ctx::Slot &sl = h->slot[iPipeline & 1];
  const int nC = iConvEnd - iConvBegin, nO = sl.stageNO;
  if (nO < 1)
  {
    h->err = "bioem_hip_convolve: no projections in this pipeline slot (call bioem_hip_project first)";
    return 2;
  }
  if (iConvBegin < 0 || iConvEnd > h->nCTF || nC < 1 || (long long) nO * nC > h->maxOC)
  {
    char buf[200];
    snprintf(buf, sizeof(buf), "bioem_hip_convolve: CTF range invalid or more than %d (orientation, CTF) rows per call", h->maxOC);
    h->err = buf;
    return 2;
  }
  if (sl.cmpPending)
  { // a comparison of this slot's previous conv rows is still queued: it reads what this call overwrites
    HIP_CHECK(h, hipStreamWaitEvent(h->prepStream, sl.cmpDone, 0));
    sl.cmpPending = false;
  }
  if (phase_begin(h, h->prepStream, BIOEM_HIP_PHASE_CONVOLUTION, sl.stageO0, sl.stageO0 + nO, iConvBegin, iConvEnd) ||
      convolve_batch(h, sl, h->prepStream, nO, iConvBegin, nC) || phase_end(h, h->prepStream))
    return 1;
  HIP_CHECK(h, hipEventRecord(sl.prepDone, h->prepStream));
  sl.stageC0 = iConvBegin;
  sl.stageNC = nC;
  return 0;
}

int bioem_hip_compare_device(bioem_hip_handle h, int iPipeline)
{
  HIP_CHECK(h, hipSetDevice(h->device));
  bioem_hip_ctx::Slot &sl = h->slot[iPipeline & 1];
  const int nO = sl.stageNO, nC = sl.stageNC;
  if (nO < 1 || nC < 1)
  {
    h->err = "bioem_hip_compare_device: no conv spectra in this pipeline slot (call bioem_hip_project and bioem_hip_convolve first)";
    return 2;
  }
  HIP_CHECK(h, hipStreamWaitEvent(h->stream, sl.prepDone, 0));
  if (launch_compare_fold(h, sl, nO * nC, sl.stageO0, sl.stageC0, nC))
    return 1;
  HIP_CHECK(h, hipEventRecord(sl.cmpDone, h->stream));
  sl.cmpPending = true;
  return 0;
}

int bioem_hip_max_batch(bioem_hip_handle h, int *maxOrientations, int *maxRows)
{
  if (!h)
    return 2;
  if (maxOrientations)
    *maxOrientations = h->OB;
  if (maxRows)
    *maxRows = h->maxOC;
  return 0;
}

int bioem_hip_finish_run(bioem_hip_handle h, void *pProb_host)
{
  HIP_CHECK(h, hipSetDevice(h->device));
  if (compat_flush(h))
    return 1;
  HIP_CHECK(h, hipMemcpyAsync(pProb_host, h->dProb, h->probBytes, hipMemcpyDeviceToHost, h->stream));
  HIP_CHECK(h, hipStreamSynchronize(h->stream));
  h->inRun = false;
  drain_events(h);
  drain_phases(h);
  return 0;
}

int bioem_hip_set_phase_timing(bioem_hip_handle h, int on)
{
  if (!h)
    return 2;
  h->phaseTiming = on != 0;
  return 0;
}

int bioem_hip_phase_records(bioem_hip_handle h, bioem_hip_phase_record *out, int cap, int *n)
{
  if (!h || !n || cap < 0 || (cap > 0 && !out))
    return 2;
  HIP_CHECK(h, hipSetDevice(h->device));
  drain_phases(h);
  const int have = (int) h->phaseDone.size();
  *n = have;
  for (int i = 0; i < have && i < cap; i++)
    out[i] = h->phaseDone[i];
  if (cap >= have)
    h->phaseDone.clear();
  return 0;
}

int bioem_hip_synchronize(bioem_hip_handle h)
{
  HIP_CHECK(h, hipSetDevice(h->device));
  if (compat_flush(h))
    return 1;
  HIP_CHECK(h, hipStreamSynchronize(h->stream));
  return 0;
}

int bioem_hip_merge_host(int nShards, int nMaps, int nAngles, int writeAngles, const void *const *shards, void *out)
{
  if (nShards < 1)
    return 2;
  bioem_hip_prob_map *om = reinterpret_cast<bioem_hip_prob_map *>(out);
  bioem_hip_prob_angle *oa = reinterpret_cast<bioem_hip_prob_angle *>(om + nMaps);
  for (int i = 0; i < nMaps; i++)
  {
    int who = 0;
    double cmax = reinterpret_cast<const bioem_hip_prob_map *>(shards[0])[i].Constoadd;
    for (int s = 1; s < nShards; s++)
    {
      const double c = reinterpret_cast<const bioem_hip_prob_map *>(shards[s])[i].Constoadd;
      if (c > cmax)
      {
        cmax = c;
        who = s;
      }
    }
    double tot = 0.;
    for (int s = 0; s < nShards; s++)
    {
      const bioem_hip_prob_map &m = reinterpret_cast<const bioem_hip_prob_map *>(shards[s])[i];
      tot += m.Total * exp(m.Constoadd - cmax);
    }
    om[i] = reinterpret_cast<const bioem_hip_prob_map *>(shards[who])[i];
    om[i].Total = tot;
    om[i].Constoadd = cmax;
  }
  if (writeAngles)
  {
    const size_t cnt = (size_t) nMaps * nAngles;
    for (size_t e = 0; e < cnt; e++)
    {
      double cmax = MIN_PROB;
      for (int s = 0; s < nShards; s++)
      {
        const bioem_hip_prob_angle *a =
            reinterpret_cast<const bioem_hip_prob_angle *>(reinterpret_cast<const bioem_hip_prob_map *>(shards[s]) + nMaps);
        if (a[e].ConstAngle > cmax)
          cmax = a[e].ConstAngle;
      }
      double tot = 0.;
      for (int s = 0; s < nShards; s++)
      {
        const bioem_hip_prob_angle *a =
            reinterpret_cast<const bioem_hip_prob_angle *>(reinterpret_cast<const bioem_hip_prob_map *>(shards[s]) + nMaps);
        tot += a[e].forAngles * exp(a[e].ConstAngle - cmax);
      }
      oa[e].forAngles = tot;
      oa[e].ConstAngle = cmax;
    }
  }
  return 0;
}


// ---- WRITE_PROB_ANGLES: K best orientations per particle, selected where the table lives ----
// W slots per particle: K (the K best alone) or 2K - 1 (with the tie candidates a merge of shards needs)
static int topk_device(bioem_hip_ctx *h, int K, int W, double numconst)
{
  if (!h->pd.writeAngles || K < 1)
  {
    h->err = "topk_angles: handle was created without WRITE_PROB_ANGLES or K < 1";
    return 2;
  }
  if (h->candK != W)
  {
    dev_release(h, h->dCand);
    h->candK = 0;
    if (dev_alloc(h, h->dCand, (size_t) h->nMaps * W))
      return 1;
    h->candK = W;
  }
  const bioem_hip_prob_angle *pang =
      reinterpret_cast<const bioem_hip_prob_angle *>(h->dProb + sizeof(bioem_hip_prob_map) * h->nMaps);
  hipLaunchKernelGGL(k_topk_angles, dim3((h->nMaps + 63) / 64), dim3(64), 0, h->stream, pang, h->angO1 - h->angO0, h->nMaps,
                     h->angO0, K, W, numconst, h->dCand);
  HIP_CHECK(h, hipGetLastError());
  return 0;
}

static int topk_to_host(bioem_hip_ctx *h, int K, int W, double numconst, bioem_hip_angle_candidate *out)
{
  if (!h)
    return 2;
  HIP_CHECK(h, hipSetDevice(h->device));
  if (!out)
  {
    h->err = "topk_angles: null output";
    return 2;
  }
  if (compat_flush(h))
    return 1;
  if (const int rc = topk_device(h, K, W, numconst))
    return rc;
  HIP_CHECK(h, hipMemcpyAsync(out, h->dCand, sizeof(bioem_hip_angle_candidate) * (size_t) h->nMaps * W, hipMemcpyDeviceToHost,
                              h->stream));
  HIP_CHECK(h, hipStreamSynchronize(h->stream));
  return 0;
}

int bioem_hip_topk_angles(bioem_hip_handle h, int K, double numconst, bioem_hip_angle_candidate *out)
{
  return topk_to_host(h, K, K, numconst, out);
}

int bioem_hip_merge_candidates(bioem_hip_handle h, int K, double numconst, bioem_hip_angle_candidate *out)
{
  return topk_to_host(h, K, 2 * K - 1, numconst, out);
}

int bioem_hip_merge_topk_host_wide(int nShards, int nMaps, int K, int W, const bioem_hip_angle_candidate *const *cands,
                                   bioem_hip_angle_candidate *out)
{
  if (nShards < 1 || K < 1 || W < K || nMaps < 0 || !cands || (nMaps > 0 && !out))
    return 2;
  for (int s = 0; s < nShards; s++)
    if (!cands[s] && nMaps > 0)
      return 2;
  typedef std::pair<double, int> Item; // (logp, index into `all`): the reference's heap item with the orientation
                                       // replaced by a position that is monotone in it
  std::vector<bioem_hip_angle_candidate> all;
  for (int i = 0; i < nMaps; i++)
  {
    all.clear();
    for (int s = 0; s < nShards; s++)
      for (int k = 0; k < W; k++)
        if (cands[s][(size_t) i * W + k].orient >= 0)
          all.push_back(cands[s][(size_t) i * W + k]);
    // the writer walks the orientations in ascending order (bioem.cpp:1257)
    std::sort(all.begin(), all.end(),
              [](const bioem_hip_angle_candidate &a, const bioem_hip_angle_candidate &b) { return a.orient < b.orient; });
    std::priority_queue<Item, std::vector<Item>, std::greater<Item>> q;
    for (int j = 0; j < (int) all.size(); j++)
    {
      if ((int) q.size() < K)
        q.push(Item(all[j].logp, j));
      else if (q.top().first < all[j].logp)
      {
        q.pop();
        q.push(Item(all[j].logp, j));
      }
    }
    bioem_hip_angle_candidate *o = out + (size_t) i * K;
    const int cnt = (int) q.size();
    for (int r = cnt - 1; r >= 0; r--)
    {
      o[r] = all[q.top().second];
      q.pop();
    }
    for (int r = cnt; r < K; r++)
    {
      o[r].forAngles = 0.;
      o[r].ConstAngle = MIN_PROB;
      o[r].logp = -INFINITY;
      o[r].orient = -1;
      o[r].pad = 0;
    }
  }
  return 0;
}

int bioem_hip_merge_topk_host(int nShards, int nMaps, int K, const bioem_hip_angle_candidate *const *cands,
                              bioem_hip_angle_candidate *out)
{
  return bioem_hip_merge_topk_host_wide(nShards, nMaps, K, K, cands, out);
}

// ---- RCCL merge (one process, n GPUs): librccl is large, so it is loaded when the first merge asks for it ----
namespace
{
struct Rccl
{
  void *lib = nullptr;
  ncclResult_t (*CommInitAll)(ncclComm_t *, int, const int *) = nullptr;
  ncclResult_t (*AllGather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*GroupStart)() = nullptr;
  ncclResult_t (*GroupEnd)() = nullptr;
  const char *(*GetErrorString)(ncclResult_t) = nullptr;
  std::map<std::vector<int>, std::vector<ncclComm_t>> comms; // by device list; kept for the life of the process
  std::mutex mu;
};
Rccl g_rccl;

const char *rccl_load()
{
  if (g_rccl.lib)
    return nullptr;
  // a process must hold ONE copy of RCCL (a second one -- e.g. PyTorch's bundled librccl.so next to ROCm's -- ends in
  // a double free at exit): take the copy that is already loaded, if any, before loading one by the name other
  // libraries ask for
  const char *names[] = {"librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so"};
  void *lib = nullptr;
  for (const char *n : {"librccl.so.1", "librccl.so"})
    if ((lib = dlopen(n, RTLD_NOW | RTLD_GLOBAL | RTLD_NOLOAD)))
      break;
  for (const char *n : names)
    if (!lib)
      lib = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
  if (!lib)
    return "librccl.so not found (needed for the multi-GPU merge)";
  g_rccl.CommInitAll = (decltype(g_rccl.CommInitAll)) dlsym(lib, "ncclCommInitAll");
  g_rccl.AllGather = (decltype(g_rccl.AllGather)) dlsym(lib, "ncclAllGather");
  g_rccl.GroupStart = (decltype(g_rccl.GroupStart)) dlsym(lib, "ncclGroupStart");
  g_rccl.GroupEnd = (decltype(g_rccl.GroupEnd)) dlsym(lib, "ncclGroupEnd");
  g_rccl.GetErrorString = (decltype(g_rccl.GetErrorString)) dlsym(lib, "ncclGetErrorString");
  if (!g_rccl.CommInitAll || !g_rccl.AllGather || !g_rccl.GroupStart || !g_rccl.GroupEnd || !g_rccl.GetErrorString)
    return "librccl.so lacks ncclCommInitAll / ncclAllGather / ncclGroupStart / ncclGroupEnd";
  g_rccl.lib = lib;
  return nullptr;
}
} // namespace

#define RCCL_CHECK(h, expr)                                                                                        \
  do                                                                                                               \
  {                                                                                                                \
    ncclResult_t r_ = (expr);                                                                                      \
    if (r_ != ncclSuccess)                                                                                         \
    {                                                                                                              \
      char buf_[512];                                                                                              \
      snprintf(buf_, sizeof(buf_), "%s failed: %s (%s:%d)", #expr, g_rccl.GetErrorString(r_), __FILE__, __LINE__); \
      (h)->err = buf_;                                                                                             \
      return 1;                                                                                                    \
    }                                                                                                              \
  } while (0)

// what follows the all-gather: h0->dRecv holds n payloads of `payload` bytes each (nMaps map entries, then with K > 0
// nMaps lists of 2K - 1 candidates).  The map entries fold on the device, the lists merge on the host; h0's stream is
// idle on return.
static int merge_gathered(bioem_hip_ctx *h0, int n, int K, size_t payload, void *pProbMaps_host,
                          bioem_hip_angle_candidate *cand_host)
{
  const int nMaps = h0->nMaps;
  const size_t mapBytes = sizeof(bioem_hip_prob_map) * (size_t) nMaps;
  HIP_CHECK(h0, hipSetDevice(h0->device));
  if (!h0->dMerged && dev_alloc(h0, h0->dMerged, nMaps))
    return 1;
  hipLaunchKernelGGL(k_merge_shards, dim3((nMaps + 127) / 128), dim3(128), 0, h0->stream, h0->dRecv, n, payload, nMaps,
                     h0->dMerged);
  HIP_CHECK(h0, hipGetLastError());
  HIP_CHECK(h0, hipMemcpyAsync(pProbMaps_host, h0->dMerged, mapBytes, hipMemcpyDeviceToHost, h0->stream));
  std::vector<std::vector<bioem_hip_angle_candidate>> gathered;
  if (K > 0)
  {
    gathered.resize(n);
    for (int s = 0; s < n; s++)
    {
      gathered[s].resize((size_t) nMaps * (2 * K - 1));
      HIP_CHECK(h0, hipMemcpyAsync(gathered[s].data(), h0->dRecv + (size_t) s * payload + mapBytes, payload - mapBytes,
                                   hipMemcpyDeviceToHost, h0->stream));
    }
  }
  HIP_CHECK(h0, hipStreamSynchronize(h0->stream));
  if (K > 0)
  {
    std::vector<const bioem_hip_angle_candidate *> ptrs(n);
    for (int s = 0; s < n; s++)
      ptrs[s] = gathered[s].data();
    return bioem_hip_merge_topk_host_wide(n, nMaps, K, 2 * K - 1, ptrs.data(), cand_host);
  }
  return 0;
}

static size_t merge_payload(int nMaps, int K)
{
  return sizeof(bioem_hip_prob_map) * (size_t) nMaps + (K > 0 ? sizeof(bioem_hip_angle_candidate) * (size_t) nMaps * (2 * K - 1) : 0);
}

static int merge_recv_buffer(bioem_hip_ctx *h, size_t bytes)
{
  if (h->recvBytes < bytes)
  {
    dev_release(h, h->dRecv);
    h->recvBytes = 0;
    if (dev_alloc(h, h->dRecv, bytes))
      return 1;
    h->recvBytes = bytes;
  }
  return 0;
}

int bioem_hip_debug_merge_gathered(bioem_hip_handle h, const void *gathered, int nShards, int K, void *maps_out,
                                   bioem_hip_angle_candidate *cand_out)
{
  if (!h)
    return 2;
  HIP_CHECK(h, hipSetDevice(h->device));
  if (!gathered || !maps_out || nShards < 1 || K < 0 || (K > 0 && !cand_out))
  {
    h->err = "debug_merge_gathered: null argument, nShards < 1 or K < 0";
    return 2;
  }
  if (compat_flush(h))
    return 1;
  const size_t payload = merge_payload(h->nMaps, K);
  if (merge_recv_buffer(h, payload * nShards))
    return 1;
  HIP_CHECK(h, hipMemcpyAsync(h->dRecv, gathered, payload * nShards, hipMemcpyHostToDevice, h->stream));
  return merge_gathered(h, nShards, K, payload, maps_out, cand_out);
}

int bioem_hip_merge(bioem_hip_handle *handles, int n, void *pProbMaps_host, int K, double numconst,
                    bioem_hip_angle_candidate *cand_host)
{
  if (!handles || n < 1 || !handles[0])
    return 2;
  bioem_hip_ctx *h0 = handles[0];
  const int nMaps = h0->nMaps;
  std::vector<int> devs(n);
  for (int i = 0; i < n; i++)
  {
    if (!handles[i] || handles[i]->nMaps != nMaps)
    {
      h0->err = "bioem_hip_merge: handles of different shape";
      return 2;
    }
    devs[i] = handles[i]->device;
    for (int j = 0; j < i; j++)
      if (devs[j] == devs[i])
      {
        h0->err = "bioem_hip_merge: RCCL needs one GPU per shard (two handles share a device; use bioem_hip_merge_host)";
        return 2;
      }
  }
  if (K > 0 && !cand_host)
    return 2;
  std::lock_guard<std::mutex> lock(g_rccl.mu);
  if (const char *e = rccl_load())
  {
    h0->err = e;
    return 1;
  }
  auto it = g_rccl.comms.find(devs);
  if (it == g_rccl.comms.end())
  {
    std::vector<ncclComm_t> c(n);
    RCCL_CHECK(h0, g_rccl.CommInitAll(c.data(), n, devs.data()));
    it = g_rccl.comms.emplace(devs, c).first;
  }
  const std::vector<ncclComm_t> &comm = it->second;
  const size_t mapBytes = sizeof(bioem_hip_prob_map) * (size_t) nMaps;
  const size_t payload = merge_payload(nMaps, K);
  // stage every shard's contribution: its map entries (already on the device) and its list of 2K - 1 candidates
  for (int i = 0; i < n; i++)
  {
    bioem_hip_ctx *h = handles[i];
    HIP_CHECK(h, hipSetDevice(h->device));
    if (compat_flush(h))
      return 1;
    if (h->sendBytes < payload)
    {
      dev_release(h, h->dSend);
      h->sendBytes = 0;
      if (dev_alloc(h, h->dSend, payload))
        return 1;
      h->sendBytes = payload;
    }
    if (merge_recv_buffer(h, payload * n))
      return 1;
    HIP_CHECK(h, hipMemcpyAsync(h->dSend, h->dProb, mapBytes, hipMemcpyDeviceToDevice, h->stream));
    if (K > 0)
    {
      if (const int rc = topk_device(h, K, 2 * K - 1, numconst))
        return rc;
      HIP_CHECK(h, hipMemcpyAsync(h->dSend + mapBytes, h->dCand, payload - mapBytes, hipMemcpyDeviceToDevice, h->stream));
    }
  }
  // the exchange: one all-gather over xGMI
  RCCL_CHECK(h0, g_rccl.GroupStart());
  for (int i = 0; i < n; i++)
  {
    bioem_hip_ctx *h = handles[i];
    HIP_CHECK(h, hipSetDevice(h->device));
    RCCL_CHECK(h, g_rccl.AllGather(h->dSend, h->dRecv, payload, ncclChar, comm[i], h->stream));
  }
  RCCL_CHECK(h0, g_rccl.GroupEnd());
  // fold on the first device, result to the host
  const int rc = merge_gathered(h0, n, K, payload, pProbMaps_host, cand_host);
  for (int i = 1; i < n; i++)
  {
    HIP_CHECK(handles[i], hipSetDevice(handles[i]->device));
    HIP_CHECK(handles[i], hipStreamSynchronize(handles[i]->stream));
  }
  return rc;
}

} // extern "C" (closed around the helpers below: Staging::get is a template, as dev_alloc is)

// ---- what the analysis entries below share: refusals, validation, staging buffers, the batch step ----
namespace
{
// a refusal of an entry: "<entry>: <why>" as the handle's message, return 2
struct Refuse
{
  bioem_hip_ctx *h;
  const char *entry;
  int operator()(const std::string &why) const
  {
    h->err = std::string(entry) + ": " + why;
    return 2;
  }
};

// What is queued ahead of an entry: rows staged through the reference-compatible entry go first (call order), and nothing
// queued may still use buffer set 0.  voidSlot0: the entry writes buffer set 0 itself
int begin_analysis(bioem_hip_ctx *h, bool voidSlot0)
{
  if (compat_flush(h))
    return 1;
  HIP_CHECK(h, hipStreamSynchronize(h->prepStream));
  if (voidSlot0)
    void_slot(h->slot[0]);
  return 0;
}

// the first of the uploads an entry needs that the handle lacks, in the order every entry names them; nullptr: none
enum
{
  NEED_MODEL = 1,
  NEED_CTF = 2,
  NEED_ORIENT = 4,
  NEED_PARTICLES = 8,
  NEED_ALL = 15
};
const char *missing_state(const bioem_hip_ctx *h, int needs, int ownLists)
{
  if ((needs & NEED_MODEL) && !h->dVolC && (!h->dPts || h->nPts < 1))
    return "model not uploaded";
  if ((needs & NEED_CTF) && !h->ctfUp)
    return "CTF kernels not uploaded";
  if ((needs & NEED_ORIENT) && (ownLists ? (!h->dOwnAngles || h->ownOff.empty()) : h->nAnglesUp < 1))
    return ownLists ? "no per-particle orientation lists (bioem_hip_upload_particle_orientation_lists)"
                    : "orientations not uploaded";
  if ((needs & NEED_PARTICLES) && !h->refUp)
    return "particles not uploaded";
  return nullptr;
}

// the list a particle's orientation index runs over: its first entry in the list the batch reads, and its length
void orient_span(const bioem_hip_ctx *h, int ownLists, int particle, int &first, int &len)
{
  first = ownLists ? h->ownOff[(size_t) particle] : 0;
  len = ownLists ? h->ownOff[(size_t) particle + 1] - first : h->nAnglesUp;
}

// a shift outside (-N, N) on either axis would index outside the twiddle table
bool shift_outside(int N, int x, int y) { return x <= -N || x >= N || y <= -N || y >= N; }

// what is wrong with the CTF set or the displacement of a best-match record; nullptr: nothing
const char *bad_match_place(const bioem_hip_ctx *h, const bioem_hip_prob_map &r)
{
  if (r.max_prob_conv < 0 || r.max_prob_conv >= h->nCTF)
    return "max_prob_conv outside [0, nCTF)";
  if (shift_outside(h->N, r.max_prob_cent_x, r.max_prob_cent_y))
    return "displacement of N pixels or more";
  return nullptr;
}

// the best-match records of the particles [p0, p1) as the kernels read them; 0, or the refusal of the first bad one
int match_records(const bioem_hip_ctx *h, const Refuse &refuse, const bioem_hip_prob_map *records, int ownLists, int p0, int p1,
                  std::vector<RenderRecord> &recs)
{
  recs.resize((size_t) (p1 - p0));
  for (int p = p0; p < p1; p++)
  {
    const bioem_hip_prob_map &r = records[p];
    int first, len;
    orient_span(h, ownLists, p, first, len);
    const char *why = r.max_prob_orient < 0 || r.max_prob_orient >= len ? "max_prob_orient outside its orientation list"
                                                                        : bad_match_place(h, r);
    if (why)
    {
      char buf[256];
      snprintf(buf, sizeof(buf), "particle %d: %s (orient %d of %d, conv %d, cent %d %d)", p, why, r.max_prob_orient, len,
               r.max_prob_conv, r.max_prob_cent_x, r.max_prob_cent_y);
      return refuse(buf);
    }
    recs[(size_t) (p - p0)] = {first + r.max_prob_orient, r.max_prob_conv, r.max_prob_cent_x, r.max_prob_cent_y, r.max_prob_norm,
                               r.max_prob_mu};
  }
  return 0;
}

// A request (particle, orientation and, where the entry has them, CTF set and shift; a field it lacks is 0): what is wrong
// with it, or nullptr.  first / len: the list of its particle (orient_span), 0 while the particle itself is out of range
enum
{
  REQ_CONV = 1,
  REQ_SHIFT = 2
};
const char *bad_request(const bioem_hip_ctx *h, const bioem_hip_grad_request &r, int fields, int ownLists, int &first, int &len)
{
  first = len = 0;
  if (r.particle < 0 || r.particle >= h->nMaps)
    return "particle outside [0, nMaps)";
  orient_span(h, ownLists, r.particle, first, len);
  if (r.orient < 0 || r.orient >= len)
    return "orient outside its orientation list";
  if ((fields & REQ_CONV) && (r.conv < 0 || r.conv >= h->nCTF))
    return "conv outside [0, nCTF)";
  if ((fields & REQ_SHIFT) && shift_outside(h->N, r.shiftX, r.shiftY))
    return "shift outside (-N, N)";
  return nullptr;
}

// the refusal of request i: the reason, then the fields the entry has against their ranges
std::string request_refusal(const bioem_hip_ctx *h, int i, const char *why, const bioem_hip_grad_request &r, int fields, int len)
{
  char buf[256];
  int at = snprintf(buf, sizeof(buf), "request %d: %s (particle %d of %d, orient %d of %d", i, why, r.particle, h->nMaps,
                    r.orient, len);
  if (fields & REQ_CONV)
    at += snprintf(buf + at, sizeof(buf) - at, ", conv %d of %d", r.conv, h->nCTF);
  if (fields & REQ_SHIFT)
    at += snprintf(buf + at, sizeof(buf) - at, ", shift %d %d, N %d", r.shiftX, r.shiftY, h->N);
  return std::string(buf) + ")";
}

// the shifts (x, y) of the n records handed to a debug hook; 0, or the refusal of the first outside (-N, N)
int debug_shifts_refused(const bioem_hip_ctx *h, const Refuse &refuse, const int *shiftXY, int n)
{
  for (int i = 0; i < n; i++)
    if (shift_outside(h->N, shiftXY[2 * i], shiftXY[2 * i + 1]))
    {
      char buf[160];
      snprintf(buf, sizeof(buf), "record %d: shift outside (-N, N) (shift %d %d, N %d)", i, shiftXY[2 * i], shiftXY[2 * i + 1],
               h->N);
      return refuse(buf);
    }
  return 0;
}

// Device buffers an entry obtains together, for fields of the handle: either all of them, and commit() hands them to the
// fields (releasing what a field held: a group that grows), or the handle stays exactly as it was and commit() returns 1.
struct Staging
{
  bioem_hip_ctx *h;
  struct Item
  {
    void *field, *fresh;                                           // a T *& of the handle, the T * obtained for it
    void (*take)(bioem_hip_ctx *h, void *field, void *fresh); // the field takes it, as a T * again
  };
  std::vector<Item> items;
  bool failed = false;

  // n elements for a field of the handle
  template <class T>
  T *get(T *&field, size_t n)
  {
    T *p = nullptr;
    failed = failed || dev_alloc(h, p, n);
    items.push_back({&field, p, [](bioem_hip_ctx *h_, void *f, void *fresh) {
                       T *&dst = *static_cast<T **>(f);
                       dev_release(h_, dst);
                       dst = static_cast<T *>(fresh);
                     }});
    return p;
  }
  // an upload that belongs to the transaction (dst: what get() returned)
  void fill(void *dst, const void *src, size_t bytes)
  {
    failed = failed || hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice) != hipSuccess;
  }
  int commit()
  {
    for (Item &it : items)
      if (failed)
        dev_release(h, it.fresh);
      else
        it.take(h, it.field, it.fresh);
    if (failed)
      (void) hipGetLastError();
    return failed;
  }
};

// the orientations the n records on the device name, gathered from src into the contiguous list dAngles
// (records: RenderRecord or BioemWindowRecord, the same 24 bytes with src first)
int gather_matches(bioem_hip_ctx *h, const OrientList &src, const void *dRec, int n, float4 *dAngles)
{
  hipLaunchKernelGGL(k_render_gather, dim3((n + 255) / 256), dim3(256), 0, h->stream, src.d,
                     static_cast<const RenderRecord *>(dRec), n, dAngles);
  HIP_CHECK(h, hipGetLastError());
  return 0;
}

// the projections of the gathered orientations [o0, o0 + n) into buffer set 0: phase 0 of the records [i0, i0 + n)
int project_matches(bioem_hip_ctx *h, const OrientList &src, const float4 *dAngles, int o0, int n, int i0)
{
  const OrientList L = {dAngles, src.isQuat, src.quatNormDev};
  return phase_begin(h, h->stream, BIOEM_HIP_PHASE_PROJECTION, i0, i0 + n, 0, 0) ||
         project_batch(h, h->slot[0], h->stream, L, o0, n) || phase_end(h, h->stream);
}

// a batch of n records (the records [i0, i0 + n) of the call) to the device, their orientations gathered, their projections
// in buffer set 0
int stage_matches(bioem_hip_ctx *h, const OrientList &src, void *dRec, float4 *dAngles, const void *hostRecs, int n, int i0)
{
  HIP_CHECK(h, hipMemcpyAsync(dRec, hostRecs, sizeof(RenderRecord) * n, hipMemcpyHostToDevice, h->stream));
  return gather_matches(h, src, dRec, n, dAngles) || project_matches(h, src, dAngles, 0, n, i0);
}

// the spectra of the particles of nb records back in reference layout, dst[i] for record i: one launch per run of
// consecutive particles
int unreorder_runs(bioem_hip_ctx *h, const BioemWindowRecord *recs, int nb, float2 *dst)
{
  for (int i = 0; i < nb;)
  {
    int j = i + 1;
    while (j < nb && recs[j].particle == recs[j - 1].particle + 1)
      j++;
    hipLaunchKernelGGL(k_unreorder, dim3(std::min(1024, 16 * (j - i))), dim3(256), 0, h->stream,
                       h->dRef + h->Mc * (size_t) recs[i].particle, dst + (size_t) h->M * i, j - i, h->N, h->H, h->plan.halfR,
                       h->plan.N1, h->Hp);
    HIP_CHECK(h, hipGetLastError());
    i = j;
  }
  return 0;
}

// (the attribute belongs to the kernels, not the handle: images beyond 2 048 pixels need more than 64 KiB)
int render_lds_attr(bioem_hip_ctx *h, size_t lds)
{
  HIP_CHECK(h, hipFuncSetAttribute(reinterpret_cast<const void *>(k_render_cols), hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds));
  HIP_CHECK(h, hipFuncSetAttribute(reinterpret_cast<const void *>(k_render_rows), hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds));
  return 0;
}

// a launch failed inside an open phase: the phase is dropped, its events go back to the pool
void drop_open_phase(bioem_hip_ctx *h)
{
  if (!h->phaseTiming || h->phasePending.empty())
    return;
  h->evPool.push_back(h->phasePending.back().a);
  h->evPool.push_back(h->phasePending.back().b);
  h->phasePending.pop_back();
}
} // namespace

extern "C" {

// ---- the calculated image of the best-match records (bioem::printModel, bioem.cpp:624-657, 1925-2085) ----
int bioem_hip_render_best_maps(bioem_hip_handle h, const bioem_hip_prob_map *records, int ownLists, int iMapBegin,
                               int iMapEnd, float *maps_out)
{
  if (!h)
    return 2;
  HIP_CHECK(h, hipSetDevice(h->device));
  const Refuse refuse = {h, "render_best_maps"};
  if (!records || !maps_out)
    return refuse("null argument");
  if (iMapBegin < 0 || iMapEnd > h->nMaps || iMapBegin >= iMapEnd)
    return refuse("particle range empty, reversed or outside [0, nMaps)");
  if (const char *why = missing_state(h, NEED_MODEL | NEED_CTF | NEED_ORIENT, ownLists))
    return refuse(why);
  std::vector<RenderRecord> recs;
  if (const int rc = match_records(h, refuse, records, ownLists, iMapBegin, iMapEnd, recs))
    return rc;
  const int N = h->N, H = h->H;
  const int OB = h->OB; // maxOrientations of bioem_hip_max_batch; slot 0 holds at least that many images
  const size_t NN = (size_t) N * N, lds = sizeof(double2) * 2 * (size_t) N;
  if (!h->dRenderOut)
  {
    Staging st = {h};
    st.get(h->dRenderRec, (size_t) OB);
    st.get(h->dRenderAngles, (size_t) OB);
    st.get(h->dRenderOut, (size_t) OB * NN);
    if (st.commit())
      return 1;
  }
  if (render_lds_attr(h, lds) || begin_analysis(h, true))
    return 1;
  bioem_hip_ctx::Slot &s0 = h->slot[0];
  const OrientList src = ownLists ? own_list(h) : shared_list(h);
  int A, B;
  dft_split(N, A, B);
  for (size_t b0 = 0; b0 < recs.size(); b0 += (size_t) OB)
  {
    const int n = (int) std::min<size_t>((size_t) OB, recs.size() - b0);
    if (stage_matches(h, src, h->dRenderRec, h->dRenderAngles, recs.data() + b0, n, (int) b0))
      return 1;
    if (phase_begin(h, h->stream, BIOEM_HIP_PHASE_CONVOLUTION, (int) b0, (int) b0 + n, 0, 0))
      return 1;
    hipLaunchKernelGGL(k_render_cols, dim3(H, n), dim3(256), lds, h->stream, s0.specRef, h->dCTF, h->dRenderRec, N, H, A, B,
                       h->dTwD, s0.rowSpec);
    HIP_CHECK(h, hipGetLastError());
    if (phase_end(h, h->stream) || phase_begin(h, h->stream, BIOEM_HIP_PHASE_COMPARISON, (int) b0, (int) b0 + n, 0, 0))
      return 1;
    hipLaunchKernelGGL(k_render_rows, dim3(N, n), dim3(256), lds, h->stream, s0.rowSpec, h->dRenderRec, N, H, A, B, h->dTwD,
                       h->dRenderOut);
    HIP_CHECK(h, hipGetLastError());
    if (phase_end(h, h->stream))
      return 1;
    HIP_CHECK(h, hipMemcpyAsync(maps_out + b0 * NN, h->dRenderOut, sizeof(float) * NN * n, hipMemcpyDeviceToHost, h->stream));
    HIP_CHECK(h, hipStreamSynchronize(h->stream));
  }
  drain_phases(h);
  return 0;
}

// ---- Fourier ring sums of the particles against their best-match records (ring_kernels.hpp) ----
static_assert(sizeof(BioemRingRecord) == sizeof(RenderRecord) && sizeof(bioem_hip_ring_sums) == 24, "record / triple layout");

namespace
{
// the staging buffers of the ring entries; a failed allocation (return 1) leaves the handle as it was
int ring_staging(bioem_hip_ctx *h)
{
  if (h->dRingOut)
    return 0;
  const size_t OB = (size_t) h->OB;
  Staging st = {h};
  st.get(h->dRingRec, OB);
  st.get(h->dRingAngles, OB);
  st.get(h->dRingRef, OB * (size_t) h->M);
  st.get(h->dRingScratch, bioem_ring_scratch(h->N, h->OB));
  st.get(h->dRingOut, OB * (size_t) bioem_ring_count(h->N));
  return st.commit();
}

// the ring pass of n staged images (records in dRingRec, particle spectra in dRingRef, projections in slot 0) and
// its copy to the host
int ring_batch(bioem_hip_ctx *h, int n, bioem_hip_ring_sums *out)
{
  HIP_CHECK(h, bioem_ring_sums_launch(h->stream, h->dRingRef, h->slot[0].specRef, h->dCTF,
                                      reinterpret_cast<const BioemRingRecord *>(h->dRingRec), n, h->N, h->dTwD,
                                      h->dRingScratch, h->dRingOut));
  HIP_CHECK(h, hipMemcpyAsync(out, h->dRingOut, sizeof(bioem_hip_ring_sums) * (size_t) n * bioem_ring_count(h->N),
                              hipMemcpyDeviceToHost, h->stream));
  return 0;
}
} // namespace

int bioem_hip_ring_count(int numberPixels) { return bioem_ring_count(numberPixels); }

int bioem_hip_best_match_rings(bioem_hip_handle h, const bioem_hip_prob_map *records, int ownLists, int iMapBegin,
                               int iMapEnd, bioem_hip_ring_sums *out)
{
  if (!h)
    return 2;
  HIP_CHECK(h, hipSetDevice(h->device));
  const Refuse refuse = {h, "best_match_rings"};
  if (!records || !out)
    return refuse("null argument");
  if (iMapBegin < 0 || iMapEnd > h->nMaps || iMapBegin >= iMapEnd)
    return refuse("particle range empty, reversed or outside [0, nMaps)");
  if (const char *why = missing_state(h, NEED_ALL, ownLists))
    return refuse(why);
  std::vector<RenderRecord> recs;
  if (const int rc = match_records(h, refuse, records, ownLists, iMapBegin, iMapEnd, recs))
    return rc;
  if (ring_staging(h) || begin_analysis(h, true))
    return 1;
  const OrientList src = ownLists ? own_list(h) : shared_list(h);
  const int N = h->N, OB = h->OB;
  const size_t nRings = (size_t) bioem_ring_count(N);
  for (size_t b0 = 0; b0 < recs.size(); b0 += (size_t) OB)
  {
    const int n = (int) std::min<size_t>((size_t) OB, recs.size() - b0);
    if (stage_matches(h, src, h->dRingRec, h->dRingAngles, recs.data() + b0, n, (int) b0))
      return 1;
    if (phase_begin(h, h->stream, BIOEM_HIP_PHASE_COMPARISON, (int) b0, (int) b0 + n, 0, 0))
      return 1;
    hipLaunchKernelGGL(k_unreorder, dim3(1024), dim3(256), 0, h->stream, h->dRef + h->Mc * ((size_t) iMapBegin + b0),
                       h->dRingRef, n, N, h->H, h->plan.halfR, h->plan.N1, h->Hp);
    HIP_CHECK(h, hipGetLastError());
    if (ring_batch(h, n, out + b0 * nRings) || phase_end(h, h->stream))
      return 1;
    HIP_CHECK(h, hipStreamSynchronize(h->stream));
  }
  drain_phases(h);
  return 0;
}

int bioem_hip_debug_ring_sums(bioem_hip_handle h, const float *specR, const float *specP, const bioem_hip_prob_map *records,
                              int n, bioem_hip_ring_sums *out)
{
  if (!h)
    return 2;
  HIP_CHECK(h, hipSetDevice(h->device));
  const Refuse refuse = {h, "debug_ring_sums"};
  if (!specR || !specP || !records || !out || n < 1)
    return refuse("null argument or no images");
  if (const char *why = missing_state(h, NEED_CTF, 0))
    return refuse(why);
  const int N = h->N;
  std::vector<RenderRecord> recs((size_t) n);
  for (int p = 0; p < n; p++)
  {
    const bioem_hip_prob_map &r = records[p];
    if (bad_match_place(h, r))
    {
      char buf[160];
      snprintf(buf, sizeof(buf), "image %d: max_prob_conv outside [0, nCTF) or a displacement of N pixels or more (conv %d, cent %d %d)",
               p, r.max_prob_conv, r.max_prob_cent_x, r.max_prob_cent_y);
      return refuse(buf);
    }
    recs[(size_t) p] = {0, r.max_prob_conv, r.max_prob_cent_x, r.max_prob_cent_y, r.max_prob_norm, r.max_prob_mu};
  }
  if (ring_staging(h) || begin_analysis(h, true))
    return 1;
  bioem_hip_ctx::Slot &s0 = h->slot[0];
  const size_t M = (size_t) h->M, nRings = (size_t) bioem_ring_count(N);
  for (int b0 = 0; b0 < n; b0 += h->OB)
  {
    const int nb = std::min(h->OB, n - b0);
    HIP_CHECK(h, hipMemcpyAsync(h->dRingRec, recs.data() + b0, sizeof(RenderRecord) * nb, hipMemcpyHostToDevice, h->stream));
    HIP_CHECK(h, hipMemcpyAsync(h->dRingRef, specR + 2 * M * (size_t) b0, sizeof(float2) * M * nb, hipMemcpyHostToDevice, h->stream));
    HIP_CHECK(h, hipMemcpyAsync(s0.specRef, specP + 2 * M * (size_t) b0, sizeof(float2) * M * nb, hipMemcpyHostToDevice, h->stream));
    if (ring_batch(h, nb, out + (size_t) b0 * nRings))
      return 1;
    HIP_CHECK(h, hipStreamSynchronize(h->stream));
  }
  return 0;
}

// ---- aligned averages of the particles of a view (view_kernels.hpp) ----
namespace
{
// the buffers of the view entries (maps: the chain's renders too); a failed allocation (return 1) leaves the handle as it was
int view_staging(bioem_hip_ctx *h, bool maps)
{
  const size_t OB = (size_t) h->OB, M = (size_t) h->M;
  if (!h->dViewNum)
  {
    const std::vector<float2> ones(M, make_float2(1.f, 0.f));
    Staging st = {h};
    st.get(h->dViewNum, OB * M);
    st.get(h->dViewDen, OB * M);
    st.get(h->dViewTau, OB);
    st.get(h->dViewMem, OB);
    st.get(h->dViewOff, OB + 1);
    st.fill(st.get(h->dViewUnit, M), ones.data(), sizeof(float2) * M);
    if (st.commit())
      return 1;
  }
  if (maps && !h->dViewMaps)
  {
    Staging st = {h};
    st.get(h->dViewMaps, OB * (size_t) h->N * h->N);
    return st.commit();
  }
  return 0;
}

// The arguments every view entry checks, and the members the kernel reads: mem[p] for every particle with a group (slot
// unset).  Returns 0, or 2 with the handle's message set.
int view_members(bioem_hip_ctx *h, const char *what, const bioem_hip_prob_map *records, const double *weights,
                 const int *groupOf, int nP, int nGroups, int g0, int g1, std::vector<BioemViewMember> &mem)
{
  char buf[256];
  const Refuse refuse = {h, what};
  if (nGroups < 1 || g0 < 0 || g1 > nGroups || g0 >= g1)
    return refuse("group range empty, reversed or outside [0, nGroups)");
  if (const char *why = missing_state(h, NEED_CTF, 0))
    return refuse(why);
  const int N = h->N;
  mem.assign((size_t) nP, BioemViewMember{});
  for (int p = 0; p < nP; p++)
  {
    const int g = groupOf[p];
    if (g == -1)
      continue;
    const bioem_hip_prob_map &r = records[p];
    const double w = weights ? weights[p] : 1.;
    const char *why = nullptr;
    if (g < -1 || g >= nGroups)
      why = "group outside [0, nGroups) and not -1";
    else if (!(w >= 0.) || !std::isfinite(w))
      why = "weight negative or not finite";
    else
      why = bad_match_place(h, r);
    if (why)
    {
      snprintf(buf, sizeof(buf), "particle %d: %s (group %d of %d, weight %g, conv %d, cent %d %d)", p, why, g, nGroups, w,
               r.max_prob_conv, r.max_prob_cent_x, r.max_prob_cent_y);
      return refuse(buf);
    }
    BioemViewMember &m = mem[(size_t) p];
    m.conv = r.max_prob_conv;
    m.xm = (r.max_prob_cent_x % N + N) % N;
    m.ym = (r.max_prob_cent_y % N + N) % N;
    m.s = w * (double) r.max_prob_norm;
    m.s2 = m.s * (double) r.max_prob_norm;
    m.dc = (double) r.max_prob_mu * (double) N * (double) N;
  }
  return 0;
}

// num / den of the groups [ga, gb) (at most maxOrientations of them) into dViewNum / dViewDen: zeroed, then one launch per
// batch of maxOrientations particles that holds a member, in particle order on the handle's stream.  specHost: the
// spectra of the caller (reference layout) instead of the handle's particles.
int view_accumulate_chunk(bioem_hip_ctx *h, const float *specHost, const std::vector<BioemViewMember> &mem, const int *groupOf,
                          int nP, int ga, int gb)
{
  const int nG = gb - ga, OB = h->OB, N = h->N;
  const size_t M = (size_t) h->M;
  HIP_CHECK(h, hipMemsetAsync(h->dViewNum, 0, sizeof(double2) * M * nG, h->stream));
  HIP_CHECK(h, hipMemsetAsync(h->dViewDen, 0, sizeof(double) * M * nG, h->stream));
  std::vector<int> off((size_t) nG + 1), cur((size_t) nG);
  std::vector<BioemViewMember> bm;
  for (int b0 = 0; b0 < nP; b0 += OB)
  {
    const int nb = std::min(OB, nP - b0);
    std::fill(off.begin(), off.end(), 0);
    for (int p = b0; p < b0 + nb; p++)
      if (groupOf[p] >= ga && groupOf[p] < gb)
        off[(size_t) (groupOf[p] - ga) + 1]++;
    for (int g = 0; g < nG; g++)
    {
      cur[(size_t) g] = off[(size_t) g];
      off[(size_t) g + 1] += off[(size_t) g];
    }
    if (off[(size_t) nG] == 0)
      continue;
    bm.resize((size_t) off[(size_t) nG]);
    for (int p = b0; p < b0 + nb; p++) // ascending within every group
      if (groupOf[p] >= ga && groupOf[p] < gb)
      {
        BioemViewMember m = mem[(size_t) p];
        m.slot = p - b0;
        bm[(size_t) cur[(size_t) (groupOf[p] - ga)]++] = m;
      }
    HIP_CHECK(h, hipMemcpyAsync(h->dViewMem, bm.data(), sizeof(BioemViewMember) * bm.size(), hipMemcpyHostToDevice, h->stream));
    HIP_CHECK(h, hipMemcpyAsync(h->dViewOff, off.data(), sizeof(int) * off.size(), hipMemcpyHostToDevice, h->stream));
    if (phase_begin(h, h->stream, BIOEM_HIP_PHASE_COMPARISON, b0, b0 + nb, 0, 0))
      return 1;
    if (specHost)
      HIP_CHECK(h, hipMemcpyAsync(h->dRingRef, specHost + 2 * M * (size_t) b0, sizeof(float2) * M * nb, hipMemcpyHostToDevice,
                                  h->stream));
    else
    {
      hipLaunchKernelGGL(k_unreorder, dim3(1024), dim3(256), 0, h->stream, h->dRef + h->Mc * (size_t) b0, h->dRingRef, nb, N,
                         h->H, h->plan.halfR, h->plan.N1, h->Hp);
      HIP_CHECK(h, hipGetLastError());
    }
    HIP_CHECK(h, bioem_view_accumulate_launch(h->stream, h->dRingRef, h->dCTF, h->dViewMem, h->dViewOff, nG, N, h->dTwD,
                                              h->dViewNum, h->dViewDen));
    if (phase_end(h, h->stream))
      return 1;
    HIP_CHECK(h, hipStreamSynchronize(h->stream)); // bm and off are rewritten for the next batch
  }
  return 0;
}

// the sums of the groups [g0, g1) to the host, chunk by chunk; stats on the host in particle order
int view_sums_run(bioem_hip_ctx *h, const float *specHost, const std::vector<BioemViewMember> &mem, const double *weights,
                  const int *groupOf, int nP, int g0, int g1, double *num_out, double *den_out, double *stats_out)
{
  if (ring_staging(h) || view_staging(h, false) || begin_analysis(h, false)) // (buffer set 0 is not written)
    return 1;
  const size_t M = (size_t) h->M;
  for (int ga = g0; ga < g1; ga += h->OB)
  {
    const int gb = std::min(g1, ga + h->OB);
    if (view_accumulate_chunk(h, specHost, mem, groupOf, nP, ga, gb))
      return 1;
    HIP_CHECK(h, hipMemcpyAsync(num_out + 2 * M * (size_t) (ga - g0), h->dViewNum, sizeof(double2) * M * (gb - ga),
                                hipMemcpyDeviceToHost, h->stream));
    HIP_CHECK(h, hipMemcpyAsync(den_out + M * (size_t) (ga - g0), h->dViewDen, sizeof(double) * M * (gb - ga),
                                hipMemcpyDeviceToHost, h->stream));
    HIP_CHECK(h, hipStreamSynchronize(h->stream));
  }
  drain_phases(h);
  for (int g = g0; g < g1; g++)
    stats_out[2 * (size_t) (g - g0)] = stats_out[2 * (size_t) (g - g0) + 1] = 0.;
  for (int p = 0; p < nP; p++)
    if (groupOf[p] >= g0 && groupOf[p] < g1)
    {
      stats_out[2 * (size_t) (groupOf[p] - g0)] += 1.;
      stats_out[2 * (size_t) (groupOf[p] - g0) + 1] += weights ? weights[p] : 1.;
    }
  return 0;
}
} // namespace

int bioem_hip_view_sums(bioem_hip_handle h, const bioem_hip_prob_map *records, const double *weights, const int *groupOf,
                        int nGroups, int g0, int g1, double *num_out, double *den_out, double *stats_out)
{
  if (!h)
    return 2;
  HIP_CHECK(h, hipSetDevice(h->device));
  const Refuse refuse = {h, "view_sums"};
  if (!records || !groupOf || !num_out || !den_out || !stats_out)
    return refuse("null argument");
  std::vector<BioemViewMember> mem;
  if (const int rc = view_members(h, "view_sums", records, weights, groupOf, h->nMaps, nGroups, g0, g1, mem))
    return rc;
  if (const char *why = missing_state(h, NEED_PARTICLES, 0))
    return refuse(why);
  return view_sums_run(h, nullptr, mem, weights, groupOf, h->nMaps, g0, g1, num_out, den_out, stats_out);
}

int bioem_hip_debug_view_sums(bioem_hip_handle h, const float *specR, const bioem_hip_prob_map *records, const double *weights,
                              const int *groupOf, int n, int nGroups, double *num_out, double *den_out, double *stats_out)
{
  if (!h)
    return 2;
  HIP_CHECK(h, hipSetDevice(h->device));
  if (!specR || !records || !groupOf || !num_out || !den_out || !stats_out || n < 1)
    return Refuse{h, "debug_view_sums"}("null argument or no images");
  std::vector<BioemViewMember> mem;
  if (const int rc = view_members(h, "debug_view_sums", records, weights, groupOf, n, nGroups, 0, nGroups, mem))
    return rc;
  return view_sums_run(h, specR, mem, weights, groupOf, n, 0, nGroups, num_out, den_out, stats_out);
}

int bioem_hip_view_averages(bioem_hip_handle h, const bioem_hip_prob_map *records, const double *weights, const int *groupOf,
                            const int *groupOrient, int nGroups, double wiener, int g0, int g1, bioem_hip_ring_sums *rings_out,
                            float *avg_maps_out, float *proj_maps_out)
{
  if (!h)
    return 2;
  HIP_CHECK(h, hipSetDevice(h->device));
  char buf[160];
  const Refuse refuse = {h, "view_averages"};
  if (!records || !groupOf || !groupOrient || !rings_out)
    return refuse("null argument");
  if (!(wiener >= 0.) || !std::isfinite(wiener))
    return refuse("wiener negative or not finite");
  std::vector<BioemViewMember> mem; // (the members' CTF sets are checked against the CTF kernels, so those come first here)
  if (const int rc = view_members(h, "view_averages", records, weights, groupOf, h->nMaps, nGroups, g0, g1, mem))
    return rc;
  if (const char *why = missing_state(h, NEED_MODEL | NEED_ORIENT | NEED_PARTICLES, 0))
    return refuse(why);
  for (int g = g0; g < g1; g++)
    if (groupOrient[g] < -1 || groupOrient[g] >= h->nAnglesUp)
    {
      snprintf(buf, sizeof(buf), "group %d: orientation %d outside the list of %d and not -1", g, groupOrient[g], h->nAnglesUp);
      return refuse(buf);
    }
  const bool maps = avg_maps_out || proj_maps_out;
  if (ring_staging(h) || view_staging(h, maps))
    return 1;
  const int N = h->N, H = h->H, OB = h->OB;
  const size_t M = (size_t) h->M, NN = (size_t) N * N, nRings = (size_t) bioem_ring_count(N);
  const size_t lds = sizeof(double2) * 2 * (size_t) N;
  int A, B;
  dft_split(N, A, B);
  if ((maps && render_lds_attr(h, lds)) || begin_analysis(h, true))
    return 1;
  bioem_hip_ctx::Slot &s0 = h->slot[0];
  std::vector<RenderRecord> recs;
  for (int ga = g0; ga < g1; ga += OB)
  {
    const int gb = std::min(g1, ga + OB), nG = gb - ga;
    if (view_accumulate_chunk(h, nullptr, mem, groupOf, h->nMaps, ga, gb))
      return 1;
    // P^ of the chunk where the ring pass and the render read the particle spectra; P_o of the chunk in buffer set 0.
    // The unit record and the kernel 1 + 0i make M = P_o in the ring pass and leave the renders the plain c2r / N^2.
    HIP_CHECK(h, bioem_view_wiener_launch(h->stream, h->dViewNum, h->dViewDen, nG, N, wiener, h->dViewTau, h->dRingRef));
    recs.assign((size_t) nG, RenderRecord{0, 0, 0, 0, 1.f, 0.f});
    for (int g = ga; g < gb; g++)
      recs[(size_t) (g - ga)].src = std::max(0, groupOrient[g]);
    if (stage_matches(h, shared_list(h), h->dRingRec, h->dRingAngles, recs.data(), nG, ga))
      return 1;
    bioem_hip_ring_sums *ro = rings_out + nRings * (size_t) (ga - g0);
    HIP_CHECK(h, bioem_ring_sums_launch(h->stream, h->dRingRef, s0.specRef, h->dViewUnit,
                                        reinterpret_cast<const BioemRingRecord *>(h->dRingRec), nG, N, h->dTwD, h->dRingScratch,
                                        h->dRingOut));
    HIP_CHECK(h, hipMemcpyAsync(ro, h->dRingOut, sizeof(bioem_hip_ring_sums) * nRings * nG, hipMemcpyDeviceToHost, h->stream));
    for (int which = 0; which < 2; which++)
    {
      float *dst = which ? proj_maps_out : avg_maps_out;
      if (!dst)
        continue;
      hipLaunchKernelGGL(k_render_cols, dim3(H, nG), dim3(256), lds, h->stream, which ? s0.specRef : h->dRingRef, h->dViewUnit,
                         h->dRingRec, N, H, A, B, h->dTwD, s0.rowSpec);
      hipLaunchKernelGGL(k_render_rows, dim3(N, nG), dim3(256), lds, h->stream, s0.rowSpec, h->dRingRec, N, H, A, B, h->dTwD,
                         h->dViewMaps);
      HIP_CHECK(h, hipGetLastError());
      HIP_CHECK(h, hipMemcpyAsync(dst + NN * (size_t) (ga - g0), h->dViewMaps, sizeof(float) * NN * nG, hipMemcpyDeviceToHost,
                                  h->stream));
    }
    HIP_CHECK(h, hipStreamSynchronize(h->stream));
    for (int g = ga; g < gb; g++)
      if (groupOrient[g] < 0)
      { // no projection to compare with
        memset(ro + nRings * (size_t) (g - ga), 0, sizeof(bioem_hip_ring_sums) * nRings);
        if (proj_maps_out)
          memset(proj_maps_out + NN * (size_t) (g - g0), 0, sizeof(float) * NN);
      }
  }
  drain_phases(h);
  return 0;
}

// ---- the 3D density the view sums support (recon_kernels.hpp) ----
namespace
{
// the buffers of the reconstruction; a failed allocation (return 1) leaves the handle as it was.  dReconWork holds N
// planes of [N][N] doubles after the inverse (16 N^2 H >= 8 N^3 bytes), dReconDen the float volume (8 N^2 H >= 4 N^3)
int recon_staging(bioem_hip_ctx *h)
{
  if (h->dReconNum)
    return 0;
  const size_t OB = (size_t) h->OB, N = (size_t) h->N, V = N * (size_t) h->M;
  std::vector<double> sinc2(N);
  for (size_t x = 0; x < N; x++)
  { // the transform of the tent about the origin voxel o = (N + 1) / 2
    const double t = M_PI * ((double) x - (double) ((N + 1) / 2)) / (double) N;
    const double s = t == 0. ? 1. : sin(t) / t;
    sinc2[x] = s * s;
  }
  Staging st = {h};
  st.get(h->dReconNum, V);
  st.get(h->dReconDen, V);
  st.get(h->dReconWork, V);
  st.get(h->dReconR, 9 * OB);
  st.get(h->dReconPart, (size_t) kReconTauBlocks);
  st.get(h->dReconTau, 1);
  st.get(h->dReconSlot, OB);
  st.get(h->dReconOrient, OB);
  st.get(h->dReconAngles, OB);
  st.fill(st.get(h->dReconSinc, N), sinc2.data(), sizeof(double) * N);
  return st.commit();
}

bool recon_flags_known(int flags) { return (flags & ~(BIOEM_HIP_RECON_CORRECT | BIOEM_HIP_RECON_NO_CULL)) == 0; }

int recon_begin(bioem_hip_ctx *h)
{
  const size_t V = (size_t) h->N * h->M;
  HIP_CHECK(h, hipMemsetAsync(h->dReconNum, 0, sizeof(double2) * V, h->stream));
  HIP_CHECK(h, hipMemsetAsync(h->dReconDen, 0, sizeof(double) * V, h->stream));
  return 0;
}

// n views of dViewNum / dViewDen into the volume, in the order of slots[]: their matrices from the orientations orient[]
// of `list`, or (orient null) from the n angles in dReconAngles.  The stream is drained: the caller's lists are free.
int recon_insert_chunk(bioem_hip_ctx *h, const OrientList &list, const int *slots, const int *orient, int n, int flags, int g0)
{
  if (n < 1)
    return 0;
  HIP_CHECK(h, hipMemcpyAsync(h->dReconSlot, slots, sizeof(int) * n, hipMemcpyHostToDevice, h->stream));
  if (orient)
    HIP_CHECK(h, hipMemcpyAsync(h->dReconOrient, orient, sizeof(int) * n, hipMemcpyHostToDevice, h->stream));
  if (phase_begin(h, h->stream, BIOEM_HIP_PHASE_CONVOLUTION, g0, g0 + n, 0, 0))
    return 1;
  HIP_CHECK(h, bioem_recon_matrices_launch(h->stream, list.d, orient ? h->dReconOrient : nullptr, list.isQuat, n, h->dReconR));
  HIP_CHECK(h, bioem_recon_insert_launch(h->stream, h->dViewNum, h->dViewDen, h->dReconSlot, h->dReconR, n, h->N, h->dTwD,
                                         (flags & BIOEM_HIP_RECON_NO_CULL) ? 0 : 1, h->dReconNum, h->dReconDen));
  if (phase_end(h, h->stream))
    return 1;
  HIP_CHECK(h, hipStreamSynchronize(h->stream));
  return 0;
}

// numV / denV as they stand to the host where asked for, then V^, then the volume; tau to *tau_out.  The phase records
// hold the kernels, not the copies to the host.
int recon_finish(bioem_hip_ctx *h, double wiener, int flags, float *vol_out, double *spec_out, double *numV_out,
                 double *denV_out, double *tau_out)
{
  const int N = h->N;
  const size_t V = (size_t) N * h->M, N3 = (size_t) N * N * N;
  if (numV_out)
    HIP_CHECK(h, hipMemcpyAsync(numV_out, h->dReconNum, sizeof(double2) * V, hipMemcpyDeviceToHost, h->stream));
  if (denV_out)
    HIP_CHECK(h, hipMemcpyAsync(denV_out, h->dReconDen, sizeof(double) * V, hipMemcpyDeviceToHost, h->stream));
  if (phase_begin(h, h->stream, BIOEM_HIP_PHASE_PROJECTION, 0, 1, 0, 0))
    return 1;
  HIP_CHECK(h, bioem_recon_estimate_launch(h->stream, h->dReconNum, h->dReconDen, N, wiener, h->dTwD, h->dReconPart,
                                           h->dReconTau));
  if (phase_end(h, h->stream))
    return 1;
  if (spec_out)
    HIP_CHECK(h, hipMemcpyAsync(spec_out, h->dReconNum, sizeof(double2) * V, hipMemcpyDeviceToHost, h->stream));
  if (tau_out)
    HIP_CHECK(h, hipMemcpyAsync(tau_out, h->dReconTau, sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (vol_out)
  {
    int A, B;
    dft_split(N, A, B);
    if (phase_begin(h, h->stream, BIOEM_HIP_PHASE_PROJECTION, 1, 2, 0, 0))
      return 1;
    // axis 0: V^ -> work; the planes: work -> columns (over V^) -> maps (over work); the float volume over denV
    HIP_CHECK(h, bioem_recon_axis0_launch(h->stream, h->dReconNum, N, h->dTwD, h->dReconWork));
    HIP_CHECK(h, bioem_grad_inverse_launch(h->stream, h->dReconWork, N, N, A, B, h->dTwD, h->dReconNum,
                                           reinterpret_cast<double *>(h->dReconWork)));
    float *dVol = reinterpret_cast<float *>(h->dReconDen);
    HIP_CHECK(h, bioem_recon_correct_launch(h->stream, reinterpret_cast<const double *>(h->dReconWork), N, h->dReconSinc,
                                            (flags & BIOEM_HIP_RECON_CORRECT) ? 1 : 0, dVol));
    if (phase_end(h, h->stream))
      return 1;
    HIP_CHECK(h, hipMemcpyAsync(vol_out, dVol, sizeof(float) * N3, hipMemcpyDeviceToHost, h->stream));
  }
  HIP_CHECK(h, hipStreamSynchronize(h->stream));
  drain_phases(h);
  return 0;
}
} // namespace

int bioem_hip_reconstruct(bioem_hip_handle h, const bioem_hip_prob_map *records, const double *weights, const int *groupOf,
                          const int *groupOrient, int nGroups, double wiener, int flags, float *vol_out, double *spec_out,
                          double *den_out, double *stats_out)
{
  if (!h)
    return 2;
  HIP_CHECK(h, hipSetDevice(h->device));
  char buf[160];
  const Refuse refuse = {h, "reconstruct"};
  if (!records || !groupOf || !groupOrient)
    return refuse("null argument");
  if (!vol_out && !spec_out && !den_out && !stats_out)
    return refuse("every output is null");
  if (!recon_flags_known(flags))
    return refuse("unknown flag bits");
  if (!(wiener >= 0.) || !std::isfinite(wiener))
    return refuse("wiener negative or not finite");
  std::vector<BioemViewMember> mem;
  if (const int rc = view_members(h, "reconstruct", records, weights, groupOf, h->nMaps, nGroups, 0, nGroups, mem))
    return rc;
  if (const char *why = missing_state(h, NEED_ORIENT | NEED_PARTICLES, 0))
    return refuse(why);
  for (int g = 0; g < nGroups; g++)
    if (groupOrient[g] < -1 || groupOrient[g] >= h->nAnglesUp)
    {
      snprintf(buf, sizeof(buf), "group %d: orientation %d outside the list of %d and not -1", g, groupOrient[g], h->nAnglesUp);
      return refuse(buf);
    }
  if (ring_staging(h) || view_staging(h, false) || recon_staging(h) || begin_analysis(h, false)) // (set 0 is not written)
    return 1;
  // The views of the call: the groups with an orientation and a member, in ascending order, numbered densely so that
  // every chunk but the last is full -- nothing is accumulated for a group that is not inserted, and the volume is read
  // and written once per maxOrientations views.  viewOf[p]: the view of particle p, or -1.
  std::vector<int> count((size_t) nGroups, 0), view((size_t) nGroups, -1), orient, viewOf((size_t) h->nMaps, -1);
  double stats[4] = {0., 0., 0., 0.};
  for (int p = 0; p < h->nMaps; p++)
    if (groupOf[p] >= 0)
      count[(size_t) groupOf[p]]++;
  for (int g = 0; g < nGroups; g++)
    if (groupOrient[g] >= 0 && count[(size_t) g] > 0)
    {
      view[(size_t) g] = (int) orient.size();
      orient.push_back(groupOrient[g]);
    }
  for (int p = 0; p < h->nMaps; p++)
    if (groupOf[p] >= 0 && view[(size_t) groupOf[p]] >= 0)
    {
      viewOf[(size_t) p] = view[(size_t) groupOf[p]];
      stats[1] += 1.;
      stats[2] += weights ? weights[p] : 1.;
    }
  const int nViews = (int) orient.size();
  stats[0] = (double) nViews;
  if (recon_begin(h))
    return 1;
  std::vector<int> slots((size_t) h->OB);
  for (int i = 0; i < h->OB; i++)
    slots[(size_t) i] = i;
  for (int va = 0; va < nViews; va += h->OB)
  {
    const int vb = std::min(nViews, va + h->OB);
    if (view_accumulate_chunk(h, nullptr, mem, viewOf.data(), h->nMaps, va, vb) ||
        recon_insert_chunk(h, shared_list(h), slots.data(), orient.data() + va, vb - va, flags, va))
      return 1;
  }
  if (recon_finish(h, wiener, flags, vol_out, spec_out, nullptr, den_out, &stats[3]))
    return 1;
  if (stats_out)
    memcpy(stats_out, stats, sizeof(stats));
  return 0;
}

int bioem_hip_debug_reconstruct(bioem_hip_handle h, const double *num, const double *den, const float *angles4, int isQuat,
                                int nViews, double wiener, int flags, float *vol_out, double *spec_out, double *numV_out,
                                double *denV_out)
{
  if (!h)
    return 2;
  HIP_CHECK(h, hipSetDevice(h->device));
  char buf[160];
  const Refuse refuse = {h, "debug_reconstruct"};
  if (!num || !den || !angles4)
    return refuse("null argument");
  if (!vol_out && !spec_out && !numV_out && !denV_out)
    return refuse("every output is null");
  if (!recon_flags_known(flags))
    return refuse("unknown flag bits");
  if (nViews < 1)
    return refuse("no views");
  if (!(wiener >= 0.) || !std::isfinite(wiener))
    return refuse("wiener negative or not finite");
  for (int v = 0; v < nViews; v++)
    for (int c = 0; c < (isQuat ? 4 : 3); c++)
      if (!std::isfinite(angles4[4 * (size_t) v + c]))
      {
        snprintf(buf, sizeof(buf), "view %d: orientation not finite", v);
        return refuse(buf);
      }
  if (view_staging(h, false) || recon_staging(h) || begin_analysis(h, false)) // (buffer set 0 is not written)
    return 1;
  if (recon_begin(h))
    return 1;
  const size_t M = (size_t) h->M;
  const OrientList list = {h->dReconAngles, isQuat ? 1 : 0, 0.};
  std::vector<int> slots;
  for (int va = 0; va < nViews; va += h->OB)
  {
    const int n = std::min(h->OB, nViews - va);
    slots.resize((size_t) n);
    for (int i = 0; i < n; i++)
      slots[(size_t) i] = i;
    HIP_CHECK(h, hipMemcpyAsync(h->dViewNum, num + 2 * M * (size_t) va, sizeof(double2) * M * n, hipMemcpyHostToDevice,
                                h->stream));
    HIP_CHECK(h, hipMemcpyAsync(h->dViewDen, den + M * (size_t) va, sizeof(double) * M * n, hipMemcpyHostToDevice, h->stream));
    HIP_CHECK(h, hipMemcpyAsync(h->dReconAngles, angles4 + 4 * (size_t) va, sizeof(float4) * n, hipMemcpyHostToDevice,
                                h->stream));
    if (recon_insert_chunk(h, list, slots.data(), nullptr, n, flags, va))
      return 1;
  }
  return recon_finish(h, wiener, flags, vol_out, spec_out, numV_out, denV_out, nullptr);
}

// ---- posterior-weighted view sums and their density (soft_kernels.hpp) ----
static_assert(sizeof(bioem_hip_soft_member) == 40, "member layout");

namespace
{
// the buffers of the soft entries for tables of nd x nd cells; a failed allocation (return 1) leaves the handle as it was
int soft_staging(bioem_hip_ctx *h, int nd)
{
  if (h->dSoftW && nd <= h->softNd)
    return 0;
  const size_t OB = (size_t) h->OB, T = (size_t) nd * nd;
  // tw[j] = exp(+2 pi i j / N) as dTwD holds it, but 0 and +-1 where 4 j is a multiple of N: the correctly rounded values
  // there (cos(pi / 2) of the library is 6e-17), so a table of whole shifts of a quarter image multiplies exactly
  const int N = h->N;
  std::vector<double2> tw((size_t) N);
  for (int j = 0; j < N; j++)
  {
    tw[(size_t) j] = twiddle_d(j, N);
    if ((4 * j) % N == 0)
    {
      const int q = 4 * j / N; // quarter turns
      tw[(size_t) j] = make_double2(q == 0 ? 1. : q == 2 ? -1. : 0., q == 1 ? 1. : q == 3 ? -1. : 0.);
    }
  }
  Staging st = {h};
  st.fill(st.get(h->dSoftTw, (size_t) N), tw.data(), sizeof(double2) * N);
  st.get(h->dSoftCells, OB * T);
  st.get(h->dSoftU, OB * (size_t) nd * h->H);
  st.get(h->dSoftW, OB * (size_t) h->M);
  st.get(h->dSoftMem, OB);
  st.get(h->dSoftXm, (size_t) h->N);
  if (st.commit())
    return 1;
  h->softNd = nd;
  return 0;
}

// The arguments every soft entry checks.  order: the members with a group by ascending (particle, position in the list),
// the order of a group's additions; xm: the shifts mod N.  Returns 0, or 2 with the handle's message set.
int soft_members(bioem_hip_ctx *h, const char *what, const bioem_hip_soft_member *members, const double *cells, int n,
                 const int *shifts, int nd, int nGroups, int g0, int g1, int nParticles, std::vector<int> &order,
                 std::vector<int> &xm)
{
  char buf[320];
  const Refuse refuse = {h, what};
  const int N = h->N;
  if (nd < 1 || nd > N)
  {
    snprintf(buf, sizeof(buf), "nd %d outside [1, N] (N %d)", nd, N);
    return refuse(buf);
  }
  xm.resize((size_t) nd);
  for (int i = 0; i < nd; i++)
  {
    if (shifts[i] <= -N || shifts[i] >= N)
    {
      snprintf(buf, sizeof(buf), "shift %d: %d outside (-N, N) (N %d)", i, shifts[i], N);
      return refuse(buf);
    }
    xm[(size_t) i] = (shifts[i] % N + N) % N;
  }
  if (nGroups < 1 || g0 < 0 || g1 > nGroups || g0 >= g1)
    return refuse("group range empty, reversed or outside [0, nGroups)");
  if (const char *why = missing_state(h, NEED_CTF, 0))
    return refuse(why);
  const size_t T = (size_t) nd * nd;
  order.clear();
  for (int r = 0; r < n; r++)
  {
    const bioem_hip_soft_member &m = members[r];
    if (m.group == -1)
      continue;
    const char *why = nullptr;
    if (m.group < -1 || m.group >= nGroups)
      why = "group outside [0, nGroups) and not -1";
    else if (m.particle < 0 || m.particle >= nParticles)
      why = "particle out of range";
    else if (m.conv < 0 || m.conv >= h->nCTF)
      why = "conv outside [0, nCTF)";
    else if (!std::isfinite(m.s2) || !std::isfinite(m.b) || !std::isfinite(m.mass))
      why = "s2, b or mass not finite";
    else if (m.s2 < 0. || m.mass < 0.)
      why = "s2 or mass negative";
    else
      for (size_t c = 0; c < T && !why; c++)
        if (!std::isfinite(cells[(size_t) r * T + c]))
          why = "a cell of the table not finite";
    if (why)
    {
      snprintf(buf, sizeof(buf), "member %d: %s (particle %d of %d, group %d of %d, conv %d of %d, s2 %g, b %g, mass %g)", r, why,
               m.particle, nParticles, m.group, nGroups, m.conv, h->nCTF, m.s2, m.b, m.mass);
      return refuse(buf);
    }
    order.push_back(r);
  }
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return members[a].particle < members[b].particle; });
  return 0;
}

// num / den of the groups [ga, gb) (at most maxOrientations of them) into dViewNum / dViewDen, as view_accumulate_chunk:
// zeroed, then per batch of maxOrientations particles the members of `order` whose groupOf[] lies in the range, at most
// maxOrientations of them per launch of the three kernels, on the handle's stream.  specHost: the spectra of the caller.
int soft_accumulate_chunk(bioem_hip_ctx *h, const float *specHost, const bioem_hip_soft_member *members, const int *groupOf,
                          const double *cells, const std::vector<int> &order, int nd, int nP, int ga, int gb)
{
  const int nG = gb - ga, OB = h->OB, N = h->N;
  const size_t M = (size_t) h->M, T = (size_t) nd * nd;
  const double NN = (double) N * (double) N;
  HIP_CHECK(h, hipMemsetAsync(h->dViewNum, 0, sizeof(double2) * M * nG, h->stream));
  HIP_CHECK(h, hipMemsetAsync(h->dViewDen, 0, sizeof(double) * M * nG, h->stream));
  std::vector<int> off((size_t) nG + 1), cur((size_t) nG), sel;
  std::vector<BioemSoftMember> bm;
  std::vector<double> bc;
  size_t at = 0;
  for (int b0 = 0; b0 < nP; b0 += OB)
  {
    const int nb = std::min(OB, nP - b0);
    sel.clear();
    for (; at < order.size() && members[order[at]].particle < b0 + nb; at++)
      if (groupOf[order[at]] >= ga && groupOf[order[at]] < gb)
        sel.push_back(order[at]);
    if (sel.empty())
      continue;
    if (specHost)
      HIP_CHECK(h, hipMemcpyAsync(h->dRingRef, specHost + 2 * M * (size_t) b0, sizeof(float2) * M * nb, hipMemcpyHostToDevice,
                                  h->stream));
    else
    {
      hipLaunchKernelGGL(k_unreorder, dim3(1024), dim3(256), 0, h->stream, h->dRef + h->Mc * (size_t) b0, h->dRingRef, nb, N,
                         h->H, h->plan.halfR, h->plan.N1, h->Hp);
      HIP_CHECK(h, hipGetLastError());
    }
    for (size_t s0 = 0; s0 < sel.size(); s0 += (size_t) OB)
    {
      const int ns = (int) std::min((size_t) OB, sel.size() - s0);
      std::fill(off.begin(), off.end(), 0);
      for (int i = 0; i < ns; i++)
        off[(size_t) (groupOf[sel[s0 + i]] - ga) + 1]++;
      for (int g = 0; g < nG; g++)
      {
        cur[(size_t) g] = off[(size_t) g];
        off[(size_t) g + 1] += off[(size_t) g];
      }
      bm.resize((size_t) ns);
      bc.resize((size_t) ns * T);
      for (int i = 0; i < ns; i++) // ascending within every group
      {
        const int r = sel[s0 + i];
        const bioem_hip_soft_member &m = members[r];
        bm[(size_t) cur[(size_t) (groupOf[r] - ga)]++] = {m.particle - b0, m.conv, i, 0, m.s2, m.b * NN};
        memcpy(bc.data() + (size_t) i * T, cells + (size_t) r * T, sizeof(double) * T);
      }
      HIP_CHECK(h, hipMemcpyAsync(h->dSoftMem, bm.data(), sizeof(BioemSoftMember) * bm.size(), hipMemcpyHostToDevice, h->stream));
      HIP_CHECK(h, hipMemcpyAsync(h->dViewOff, off.data(), sizeof(int) * off.size(), hipMemcpyHostToDevice, h->stream));
      HIP_CHECK(h, hipMemcpyAsync(h->dSoftCells, bc.data(), sizeof(double) * bc.size(), hipMemcpyHostToDevice, h->stream));
      // phase 0: the column pass, 1: the row pass, 2: the accumulation; iConvEnd = nd tells them from the chain's records
      if (phase_begin(h, h->stream, BIOEM_HIP_PHASE_PROJECTION, b0, b0 + nb, 0, nd))
        return 1;
      HIP_CHECK(h, bioem_soft_cols_launch(h->stream, h->dSoftCells, h->dSoftXm, ns, nd, N, h->dSoftTw, h->dSoftU));
      if (phase_end(h, h->stream) || phase_begin(h, h->stream, BIOEM_HIP_PHASE_CONVOLUTION, b0, b0 + nb, 0, nd))
        return 1;
      HIP_CHECK(h, bioem_soft_rows_launch(h->stream, h->dSoftU, h->dSoftXm, ns, nd, N, h->dSoftTw, h->dSoftW));
      if (phase_end(h, h->stream) || phase_begin(h, h->stream, BIOEM_HIP_PHASE_COMPARISON, b0, b0 + nb, 0, nd))
        return 1;
      HIP_CHECK(h, bioem_soft_accumulate_launch(h->stream, h->dRingRef, h->dCTF, h->dSoftMem, h->dViewOff, nG, N, h->dSoftW,
                                                h->dViewNum, h->dViewDen));
      if (phase_end(h, h->stream))
        return 1;
      HIP_CHECK(h, hipStreamSynchronize(h->stream)); // bm, off and bc are rewritten for the next launch
    }
  }
  return 0;
}

// staging of every soft entry and the shifts of the call on the device
int soft_begin(bioem_hip_ctx *h, const std::vector<int> &xm, bool recon)
{
  if (ring_staging(h) || view_staging(h, false) || soft_staging(h, (int) xm.size()) || (recon && recon_staging(h)) ||
      begin_analysis(h, false)) // (buffer set 0 is not written)
    return 1;
  HIP_CHECK(h, hipMemcpyAsync(h->dSoftXm, xm.data(), sizeof(int) * xm.size(), hipMemcpyHostToDevice, h->stream));
  HIP_CHECK(h, hipStreamSynchronize(h->stream));
  return 0;
}

// the sums of the groups [g0, g1) to the host, chunk by chunk; stats on the host in the order of the additions
int soft_sums_run(bioem_hip_ctx *h, const float *specHost, const bioem_hip_soft_member *members, const double *cells, int n,
                  const std::vector<int> &order, const std::vector<int> &xm, int nP, int g0, int g1, double *num_out,
                  double *den_out, double *stats_out)
{
  if (soft_begin(h, xm, false))
    return 1;
  const size_t M = (size_t) h->M;
  std::vector<int> groupOf((size_t) n);
  for (int r = 0; r < n; r++)
    groupOf[(size_t) r] = members[r].group;
  for (int ga = g0; ga < g1; ga += h->OB)
  {
    const int gb = std::min(g1, ga + h->OB);
    if (soft_accumulate_chunk(h, specHost, members, groupOf.data(), cells, order, (int) xm.size(), nP, ga, gb))
      return 1;
    HIP_CHECK(h, hipMemcpyAsync(num_out + 2 * M * (size_t) (ga - g0), h->dViewNum, sizeof(double2) * M * (gb - ga),
                                hipMemcpyDeviceToHost, h->stream));
    HIP_CHECK(h, hipMemcpyAsync(den_out + M * (size_t) (ga - g0), h->dViewDen, sizeof(double) * M * (gb - ga),
                                hipMemcpyDeviceToHost, h->stream));
    HIP_CHECK(h, hipStreamSynchronize(h->stream));
  }
  drain_phases(h);
  for (int g = g0; g < g1; g++)
    stats_out[2 * (size_t) (g - g0)] = stats_out[2 * (size_t) (g - g0) + 1] = 0.;
  for (int r : order)
    if (members[r].group >= g0 && members[r].group < g1)
    {
      stats_out[2 * (size_t) (members[r].group - g0)] += 1.;
      stats_out[2 * (size_t) (members[r].group - g0) + 1] += members[r].mass;
    }
  return 0;
}
} // namespace

int bioem_hip_view_sums_soft(bioem_hip_handle h, const bioem_hip_soft_member *members, const double *cells, int n,
                             const int *shifts, int nd, int nGroups, int g0, int g1, double *num_out, double *den_out,
                             double *stats_out)
{
  if (!h)
    return 2;
  HIP_CHECK(h, hipSetDevice(h->device));
  const Refuse refuse = {h, "view_sums_soft"};
  if (!members || !cells || !shifts || !num_out || !den_out || !stats_out || n < 1)
    return refuse("null argument or no members");
  std::vector<int> order, xm;
  if (const int rc = soft_members(h, "view_sums_soft", members, cells, n, shifts, nd, nGroups, g0, g1, h->nMaps, order, xm))
    return rc;
  if (const char *why = missing_state(h, NEED_PARTICLES, 0))
    return refuse(why);
  return soft_sums_run(h, nullptr, members, cells, n, order, xm, h->nMaps, g0, g1, num_out, den_out, stats_out);
}

int bioem_hip_debug_view_sums_soft(bioem_hip_handle h, const float *specR, int nSpec, const bioem_hip_soft_member *members,
                                   const double *cells, int n, const int *shifts, int nd, int nGroups, double *num_out,
                                   double *den_out, double *stats_out)
{
  if (!h)
    return 2;
  HIP_CHECK(h, hipSetDevice(h->device));
  if (!specR || !members || !cells || !shifts || !num_out || !den_out || !stats_out || n < 1 || nSpec < 1)
    return Refuse{h, "debug_view_sums_soft"}("null argument, no members or no images");
  std::vector<int> order, xm;
  if (const int rc = soft_members(h, "debug_view_sums_soft", members, cells, n, shifts, nd, nGroups, 0, nGroups, nSpec, order, xm))
    return rc;
  return soft_sums_run(h, specR, members, cells, n, order, xm, nSpec, 0, nGroups, num_out, den_out, stats_out);
}

int bioem_hip_reconstruct_soft(bioem_hip_handle h, const bioem_hip_soft_member *members, const double *cells, int n,
                               const int *shifts, int nd, const int *groupOrient, int nGroups, double wiener, int flags,
                               float *vol_out, double *spec_out, double *den_out, double *stats_out)
{
  if (!h)
    return 2;
  HIP_CHECK(h, hipSetDevice(h->device));
  char buf[160];
  const Refuse refuse = {h, "reconstruct_soft"};
  if (!members || !cells || !shifts || !groupOrient || n < 1)
    return refuse("null argument or no members");
  if (!vol_out && !spec_out && !den_out && !stats_out)
    return refuse("every output is null");
  if (!recon_flags_known(flags))
    return refuse("unknown flag bits");
  if (!(wiener >= 0.) || !std::isfinite(wiener))
    return refuse("wiener negative or not finite");
  std::vector<int> order, xm;
  if (const int rc = soft_members(h, "reconstruct_soft", members, cells, n, shifts, nd, nGroups, 0, nGroups, h->nMaps, order, xm))
    return rc;
  if (const char *why = missing_state(h, NEED_ORIENT | NEED_PARTICLES, 0))
    return refuse(why);
  for (int g = 0; g < nGroups; g++)
    if (groupOrient[g] < -1 || groupOrient[g] >= h->nAnglesUp)
    {
      snprintf(buf, sizeof(buf), "group %d: orientation %d outside the list of %d and not -1", g, groupOrient[g], h->nAnglesUp);
      return refuse(buf);
    }
  if (soft_begin(h, xm, true))
    return 1;
  // the views of the call as in bioem_hip_reconstruct: the groups with an orientation and a member, numbered densely;
  // viewOf[r]: the view of member r, or -1
  std::vector<int> count((size_t) nGroups, 0), view((size_t) nGroups, -1), orient, viewOf((size_t) n, -1);
  double stats[4] = {0., 0., 0., 0.};
  for (int r : order)
    count[(size_t) members[r].group]++;
  for (int g = 0; g < nGroups; g++)
    if (groupOrient[g] >= 0 && count[(size_t) g] > 0)
    {
      view[(size_t) g] = (int) orient.size();
      orient.push_back(groupOrient[g]);
    }
  for (int r : order)
    if (view[(size_t) members[r].group] >= 0)
    {
      viewOf[(size_t) r] = view[(size_t) members[r].group];
      stats[1] += 1.;
      stats[2] += members[r].mass;
    }
  const int nViews = (int) orient.size();
  stats[0] = (double) nViews;
  if (recon_begin(h))
    return 1;
  std::vector<int> slots((size_t) h->OB);
  for (int i = 0; i < h->OB; i++)
    slots[(size_t) i] = i;
  for (int va = 0; va < nViews; va += h->OB)
  {
    const int vb = std::min(nViews, va + h->OB);
    if (soft_accumulate_chunk(h, nullptr, members, viewOf.data(), cells, order, nd, h->nMaps, va, vb) ||
        recon_insert_chunk(h, shared_list(h), slots.data(), orient.data() + va, vb - va, flags, va))
      return 1;
  }
  if (recon_finish(h, wiener, flags, vol_out, spec_out, nullptr, den_out, &stats[3]))
    return 1;
  if (stats_out)
    memcpy(stats_out, stats, sizeof(stats));
  return 0;
}

// ---- log posterior of every cell of the displacement window of a request (window_kernels.hpp) ----
static_assert(sizeof(BioemWindowRecord) == sizeof(RenderRecord) && sizeof(bioem_hip_window_request) == 12,
              "record / request layout");

namespace
{
// the shifts the reference reports for the displacement list of a plan (max_prob_cent = -displacement), ascending
void window_shifts(const KernelPlan &P, std::vector<int> &X)
{
  X.clear();
  for (int d : P.disp)
    X.push_back(-d);
  std::sort(X.begin(), X.end());
}

bool window_arguments_valid(int N, int maxD, int grid, int algo)
{
  return N >= 2 && N <= kMaxPixels && maxD >= 0 && grid >= 1 && maxD < N / 2 && (algo == 1 || algo == 2);
}

// the staging buffers of the window entries; a failed allocation (return 1) leaves the handle as it was
int window_staging(bioem_hip_ctx *h)
{
  if (h->dWinLogp)
    return 0;
  const size_t OB = (size_t) h->OB, M = (size_t) h->M, M4 = (M + 3) & ~(size_t) 3;
  std::vector<int> X;
  window_shifts(h->plan, X);
  const size_t nd = X.size();
  Staging st = {h};
  st.get(h->dWinRec, OB);
  st.get(h->dWinAngles, OB);
  st.get(h->dWinRef, OB * M);
  st.get(h->dWinConv, OB * M);
  st.get(h->dWinTerms, OB * M4);
  st.get(h->dWinSums, 2 * OB);
  st.get(h->dWinCc, OB * nd * nd);
  st.get(h->dWinParams, OB);
  st.get(h->dWinPostc, OB);
  st.get(h->dWinT, bioem_window_scratch(h->N, (int) nd, h->OB));
  int *shifts = st.get(h->dWinShifts, nd);
  st.get(h->dWinLogp, OB * nd * nd);
  st.fill(shifts, X.data(), sizeof(int) * nd);
  return st.commit();
}

// the window pass of n staged records (records in dWinRec, conv spectra in dWinConv, particle spectra in dWinRef,
// parameters complete in dWinParams) and its copies to the host
int window_batch(bioem_hip_ctx *h, int n, const float *sumRef, const float *sumsqRef, double *logp_out, float *cc_out)
{
  const size_t cells = (size_t) h->plan.nd * h->plan.nd * (size_t) n;
  hipLaunchKernelGGL(k_posterior_consts, dim3((n + 63) / 64), dim3(64), 0, h->stream, h->dWinParams, h->pd, h->dWinPostc, n);
  HIP_CHECK(h, hipGetLastError());
  HIP_CHECK(h, bioem_window_launch(h->stream, h->dWinConv, h->dWinRef, h->dWinRec, h->dWinParams, h->dWinPostc, sumRef,
                                   sumsqRef, h->pd, n, h->N, h->plan.nd, h->dWinShifts, h->dTwD, h->dWinT, h->dWinLogp,
                                   h->dWinCc));
  HIP_CHECK(h, hipMemcpyAsync(logp_out, h->dWinLogp, sizeof(double) * cells, hipMemcpyDeviceToHost, h->stream));
  if (cc_out)
    HIP_CHECK(h, hipMemcpyAsync(cc_out, h->dWinCc, sizeof(float) * cells, hipMemcpyDeviceToHost, h->stream));
  return 0;
}
} // namespace

int bioem_hip_window_offsets(int numberPixels, int maxDisplaceCenter, int gridSpaceCenter, int algo, int *shifts, int cap)
{
  if (!window_arguments_valid(numberPixels, maxDisplaceCenter, gridSpaceCenter, algo))
    return 0;
  std::vector<int> X;
  window_shifts(plan_kernels(numberPixels, maxDisplaceCenter, gridSpaceCenter, algo), X);
  for (int i = 0; shifts && i < (int) X.size() && i < cap; i++)
    shifts[i] = X[(size_t) i];
  return (int) X.size();
}

int bioem_hip_window_count(int numberPixels, int maxDisplaceCenter, int gridSpaceCenter, int algo)
{
  return bioem_hip_window_offsets(numberPixels, maxDisplaceCenter, gridSpaceCenter, algo, nullptr, 0);
}

int bioem_hip_window_posterior(bioem_hip_handle h, const bioem_hip_window_request *req, int n, int ownLists, double *logp_out,
                               float *cc_out, bioem_hip_param5 *params_out)
{
  if (!h)
    return 2;
  HIP_CHECK(h, hipSetDevice(h->device));
  const Refuse refuse = {h, "window_posterior"};
  if (!req || !logp_out || n < 1)
    return refuse("null argument or no requests");
  if (const char *why = missing_state(h, NEED_ALL, ownLists))
    return refuse(why);
  std::vector<BioemWindowRecord> recs((size_t) n);
  for (int i = 0; i < n; i++)
  {
    const bioem_hip_grad_request r = {req[i].particle, req[i].orient, req[i].conv, 0, 0};
    int first, len;
    if (const char *why = bad_request(h, r, REQ_CONV, ownLists, first, len))
      return refuse(request_refusal(h, i, why, r, REQ_CONV, len));
    recs[(size_t) i] = {first + r.orient, r.conv, r.particle, 0, {0.f, 0.f}};
  }
  if (window_staging(h) || begin_analysis(h, true))
    return 1;
  bioem_hip_ctx::Slot &s0 = h->slot[0];
  const OrientList src = ownLists ? own_list(h) : shared_list(h);
  const int N = h->N, OB = h->OB;
  const size_t M = (size_t) h->M, cells = (size_t) h->plan.nd * h->plan.nd;
  const int M4 = (int) ((M + 3) & ~(size_t) 3);
  for (int b0 = 0; b0 < n; b0 += OB)
  {
    const int nb = std::min(OB, n - b0);
    if (stage_matches(h, src, h->dWinRec, h->dWinAngles, recs.data() + b0, nb, b0))
      return 1;
    if (phase_begin(h, h->stream, BIOEM_HIP_PHASE_CONVOLUTION, b0, b0 + nb, 0, 0))
      return 1;
    HIP_CHECK(h, bioem_window_prep_launch(h->stream, s0.specRef, h->dCTF, h->dCtfParam, h->dWinRec, nb, N, h->dWinConv,
                                          h->dWinTerms, M4, h->dWinParams));
    hipLaunchKernelGGL(k_parseval_ordered, dim3((nb + 3) / 4), dim3(64), 0, h->stream, h->dWinTerms, (int) M, M4, nb,
                       (float) (N * N), h->dWinParams);
    HIP_CHECK(h, hipGetLastError());
    if (phase_end(h, h->stream) || phase_begin(h, h->stream, BIOEM_HIP_PHASE_COMPARISON, b0, b0 + nb, 0, 0))
      return 1;
    if (unreorder_runs(h, recs.data() + b0, nb, h->dWinRef) ||
        window_batch(h, nb, h->dSumRef, h->dSumsqRef, logp_out + cells * (size_t) b0, cc_out ? cc_out + cells * (size_t) b0 : nullptr))
      return 1;
    if (params_out)
      HIP_CHECK(h, hipMemcpyAsync(params_out + b0, h->dWinParams, sizeof(bioem_hip_param5) * nb, hipMemcpyDeviceToHost, h->stream));
    if (phase_end(h, h->stream))
      return 1;
    HIP_CHECK(h, hipStreamSynchronize(h->stream));
  }
  drain_phases(h);
  return 0;
}

int bioem_hip_debug_window(bioem_hip_handle h, const float *specConv, const float *specRef, const bioem_hip_param5 *params,
                           const float *sumRef, const float *sumsqRef, int n, double *logp_out, float *cc_out)
{
  if (!h)
    return 2;
  HIP_CHECK(h, hipSetDevice(h->device));
  if (!specConv || !specRef || !params || !sumRef || !sumsqRef || !logp_out || n < 1)
    return Refuse{h, "debug_window"}("null argument or no records");
  if (window_staging(h) || begin_analysis(h, false)) // (buffer set 0 is not written)
    return 1;
  const size_t M = (size_t) h->M, cells = (size_t) h->plan.nd * h->plan.nd;
  std::vector<BioemWindowRecord> recs((size_t) std::min(n, h->OB));
  for (size_t i = 0; i < recs.size(); i++)
    recs[i] = {0, 0, (int) i, 0, {0.f, 0.f}};
  for (int b0 = 0; b0 < n; b0 += h->OB)
  {
    const int nb = std::min(h->OB, n - b0);
    HIP_CHECK(h, hipMemcpyAsync(h->dWinRec, recs.data(), sizeof(BioemWindowRecord) * nb, hipMemcpyHostToDevice, h->stream));
    HIP_CHECK(h, hipMemcpyAsync(h->dWinConv, specConv + 2 * M * (size_t) b0, sizeof(float2) * M * nb, hipMemcpyHostToDevice, h->stream));
    HIP_CHECK(h, hipMemcpyAsync(h->dWinRef, specRef + 2 * M * (size_t) b0, sizeof(float2) * M * nb, hipMemcpyHostToDevice, h->stream));
    HIP_CHECK(h, hipMemcpyAsync(h->dWinParams, params + b0, sizeof(bioem_hip_param5) * nb, hipMemcpyHostToDevice, h->stream));
    HIP_CHECK(h, hipMemcpyAsync(h->dWinSums, sumRef + b0, sizeof(float) * nb, hipMemcpyHostToDevice, h->stream));
    HIP_CHECK(h, hipMemcpyAsync(h->dWinSums + h->OB, sumsqRef + b0, sizeof(float) * nb, hipMemcpyHostToDevice, h->stream));
    if (window_batch(h, nb, h->dWinSums, h->dWinSums + h->OB, logp_out + cells * (size_t) b0,
                     cc_out ? cc_out + cells * (size_t) b0 : nullptr))
      return 1;
    HIP_CHECK(h, hipStreamSynchronize(h->stream));
  }
  return 0;
}

// ---- log posterior of a (particle, orientation, shift) record under every CTF set of a list (scan_kernels.hpp) ----
static_assert(sizeof(bioem_hip_scan_request) == 16, "request layout");

namespace
{
// records one launch of the scan serves: as many whole batches as keep Pw and Z within 512 MiB, at most 16 batches or
// 4 096 records (a batch alone is a few hundred waves, each a chain of N H memory latencies: too few to fill the device)
int scan_capacity(const bioem_hip_ctx *h)
{
  const size_t OB = (size_t) h->OB, perRecord = (size_t) h->M * (sizeof(float2) + sizeof(double2));
  const size_t fit = ((size_t) 512 << 20) / perRecord / OB;
  return (int) (OB * std::max<size_t>(1, std::min<size_t>(std::min<size_t>(fit, 16), std::max<size_t>(1, 4096 / OB))));
}

// the staging buffers of the scan entries for G candidates; a failed allocation (return 1) leaves the handle as it was
int scan_staging(bioem_hip_ctx *h, int G)
{
  if (window_staging(h)) // a batch's records for the gather, gathered orientations, particle spectra, spectra handed in
    return 1;
  const size_t OB = (size_t) h->OB, M = (size_t) h->M, cap = (size_t) scan_capacity(h);
  if (!h->dScanZ)
  {
    Staging st = {h};
    st.get(h->dScanShift, OB);
    st.get(h->dScanRec, cap);
    st.get(h->dScanPw, cap * M);
    st.get(h->dScanRaw, (size_t) kScanLanes * M);
    st.get(h->dScanZ, cap * M);
    st.get(h->dScanSums, 2 * cap);
    if (st.commit())
      return 1;
  }
  if (G <= h->scanCapG)
    return 0;
  const size_t chunks = ((size_t) G + kScanLanes - 1) / kScanLanes;
  Staging st = {h}; // the group that grows with G: what it held goes once the larger buffers are all there
  st.get(h->dScanPacked, chunks * kScanLanes * M);
  st.get(h->dScanCtf, 3 * (size_t) G);
  st.get(h->dScanCc, cap * G);
  st.get(h->dScanLogp, cap * G);
  st.get(h->dScanParams, cap * G);
  if (st.commit())
    return 1;
  h->scanCapG = G;
  return 0;
}

// the candidates into the walk order, a chunk of 64 at a time through dScanRaw, and their parameters
int scan_candidates(bioem_hip_ctx *h, const float *kernels, const float *ctfParam3, int G)
{
  const size_t M = (size_t) h->M;
  for (int g0 = 0; g0 < G; g0 += kScanLanes)
  {
    const int nG = std::min(kScanLanes, G - g0);
    HIP_CHECK(h, hipMemcpyAsync(h->dScanRaw, kernels + 2 * M * (size_t) g0, sizeof(float2) * M * nG, hipMemcpyHostToDevice, h->stream));
    HIP_CHECK(h, bioem_scan_pack_launch(h->stream, h->dScanRaw, nG, h->N, h->dScanPacked + M * (size_t) g0));
  }
  HIP_CHECK(h, hipMemcpyAsync(h->dScanCtf, ctfParam3, sizeof(float) * 3 * G, hipMemcpyHostToDevice, h->stream));
  return 0;
}

// the preparation of a batch of nb records (shifts in dScanShift, projections in proj, particle spectra in dWinRef) into
// the places [at, at + nb) of the launch being gathered, with their records (host) -- inside the caller's open phase 1
int scan_prepare(bioem_hip_ctx *h, int at, int nb, const float2 *proj, const BioemWindowRecord *recs)
{
  const size_t M = (size_t) h->M;
  HIP_CHECK(h, hipMemcpyAsync(h->dScanRec + at, recs, sizeof(BioemWindowRecord) * nb, hipMemcpyHostToDevice, h->stream));
  HIP_CHECK(h, bioem_scan_prep_launch(h->stream, proj, h->dWinRef, h->dScanShift, nb, h->N, h->dTwD, h->dScanPw + M * (size_t) at,
                                      h->dScanZ + M * (size_t) at));
  return phase_end(h, h->stream);
}

// the scan of the n records gathered (the requests [r0, r0 + n) of the call: phase 2) and the copies to the host
int scan_flush(bioem_hip_ctx *h, int r0, int n, int G, const float *sumRef, const float *sumsqRef, double *logp_out,
               float *cc_out, bioem_hip_param5 *params_out)
{
  const size_t cells = (size_t) n * G;
  if (phase_begin(h, h->stream, BIOEM_HIP_PHASE_COMPARISON, r0, r0 + n, 0, 0))
    return 1;
  HIP_CHECK(h, bioem_scan_launch(h->stream, h->dScanPacked, h->dScanCtf, G, h->dScanPw, h->dScanZ, h->dScanRec, sumRef, sumsqRef,
                                 h->pd, n, h->N, h->dScanLogp, h->dScanCc, h->dScanParams));
  HIP_CHECK(h, hipMemcpyAsync(logp_out, h->dScanLogp, sizeof(double) * cells, hipMemcpyDeviceToHost, h->stream));
  if (cc_out)
    HIP_CHECK(h, hipMemcpyAsync(cc_out, h->dScanCc, sizeof(float) * cells, hipMemcpyDeviceToHost, h->stream));
  if (params_out)
    HIP_CHECK(h, hipMemcpyAsync(params_out, h->dScanParams, sizeof(bioem_hip_param5) * cells, hipMemcpyDeviceToHost, h->stream));
  if (phase_end(h, h->stream))
    return 1;
  HIP_CHECK(h, hipStreamSynchronize(h->stream));
  return 0;
}
} // namespace

int bioem_hip_ctf_scan(bioem_hip_handle h, const bioem_hip_scan_request *req, int n, int ownLists, const float *kernels,
                       const float *ctfParam3, int G, double *logp_out, float *cc_out, bioem_hip_param5 *params_out)
{
  if (!h)
    return 2;
  HIP_CHECK(h, hipSetDevice(h->device));
  const Refuse refuse = {h, "ctf_scan"};
  if (!req || !logp_out || n < 1)
    return refuse("null argument or no requests");
  if (G < 1)
    return refuse("no candidates (G = " + std::to_string(G) + ")");
  if (!kernels || !ctfParam3)
    return refuse("null candidate kernels or parameters");
  if (const char *why = missing_state(h, NEED_MODEL | NEED_ORIENT | NEED_PARTICLES, ownLists)) // (the CTF sets are handed in)
    return refuse(why);
  const int OB = h->OB;
  std::vector<BioemWindowRecord> recs((size_t) n);
  std::vector<BioemScanShift> shifts((size_t) n);
  for (int i = 0; i < n; i++)
  {
    const bioem_hip_grad_request r = {req[i].particle, req[i].orient, 0, req[i].shiftX, req[i].shiftY};
    int first, len;
    if (const char *why = bad_request(h, r, REQ_SHIFT, ownLists, first, len))
      return refuse(request_refusal(h, i, why, r, REQ_SHIFT, len));
    recs[(size_t) i] = {first + r.orient, 0, r.particle, 0, {0.f, 0.f}};
    shifts[(size_t) i] = {r.shiftX, r.shiftY};
  }
  if (scan_staging(h, G) || begin_analysis(h, true))
    return 1;
  bioem_hip_ctx::Slot &s0 = h->slot[0];
  const OrientList src = ownLists ? own_list(h) : shared_list(h);
  const int cap = scan_capacity(h);
  for (int b0 = 0, r0 = 0; b0 < n; b0 += OB) // r0: the first request of the launch being gathered
  {
    const int nb = std::min(OB, n - b0);
    // (stage_matches with the shifts' copy between its records' copy and its gather, as it always was enqueued)
    HIP_CHECK(h, hipMemcpyAsync(h->dWinRec, recs.data() + b0, sizeof(BioemWindowRecord) * nb, hipMemcpyHostToDevice, h->stream));
    HIP_CHECK(h, hipMemcpyAsync(h->dScanShift, shifts.data() + b0, sizeof(BioemScanShift) * nb, hipMemcpyHostToDevice, h->stream));
    if (gather_matches(h, src, h->dWinRec, nb, h->dWinAngles) || project_matches(h, src, h->dWinAngles, 0, nb, b0))
      return 1;
    if (phase_begin(h, h->stream, BIOEM_HIP_PHASE_CONVOLUTION, b0, b0 + nb, 0, 0))
      return 1;
    if (b0 == 0 && scan_candidates(h, kernels, ctfParam3, G)) // (part of the first batch's preparation)
      return 1;
    if (unreorder_runs(h, recs.data() + b0, nb, h->dWinRef) || scan_prepare(h, b0 - r0, nb, s0.specRef, recs.data() + b0))
      return 1;
    if (b0 + nb - r0 + OB > cap || b0 + nb == n)
    { // no room for another batch, or the last one: one launch over what is gathered
      const size_t o = (size_t) r0 * G;
      if (scan_flush(h, r0, b0 + nb - r0, G, h->dSumRef, h->dSumsqRef, logp_out + o, cc_out ? cc_out + o : nullptr,
                     params_out ? params_out + o : nullptr))
        return 1;
      r0 = b0 + nb;
    }
  }
  drain_phases(h);
  return 0;
}

int bioem_hip_debug_ctf_scan(bioem_hip_handle h, const float *specP, const float *specRef, const float *sumRef,
                             const float *sumsqRef, const int *shiftXY, int n, const float *kernels, const float *ctfParam3,
                             int G, double *logp_out, float *cc_out, bioem_hip_param5 *params_out)
{
  if (!h)
    return 2;
  HIP_CHECK(h, hipSetDevice(h->device));
  const Refuse refuse = {h, "debug_ctf_scan"};
  if (!specP || !specRef || !sumRef || !sumsqRef || !shiftXY || !kernels || !ctfParam3 || !logp_out || n < 1 || G < 1)
    return refuse("null argument, no records or no candidates");
  if (const int rc = debug_shifts_refused(h, refuse, shiftXY, n))
    return rc;
  if (scan_staging(h, G) || begin_analysis(h, false)) // (buffer set 0 is not written)
    return 1;
  const int OB = h->OB;
  const size_t M = (size_t) h->M;
  const int cap = scan_capacity(h);
  std::vector<BioemWindowRecord> recs((size_t) std::min(n, cap)); // a record's sums lie at its place in the launch
  for (size_t i = 0; i < recs.size(); i++)
    recs[i] = {0, 0, (int) i, 0, {0.f, 0.f}};
  if (scan_candidates(h, kernels, ctfParam3, G))
    return 1;
  for (int b0 = 0, r0 = 0; b0 < n; b0 += OB)
  {
    const int nb = std::min(OB, n - b0), at = b0 - r0;
    HIP_CHECK(h, hipMemcpyAsync(h->dScanShift, shiftXY + 2 * (size_t) b0, sizeof(BioemScanShift) * nb, hipMemcpyHostToDevice, h->stream));
    HIP_CHECK(h, hipMemcpyAsync(h->dWinConv, specP + 2 * M * (size_t) b0, sizeof(float2) * M * nb, hipMemcpyHostToDevice, h->stream));
    HIP_CHECK(h, hipMemcpyAsync(h->dWinRef, specRef + 2 * M * (size_t) b0, sizeof(float2) * M * nb, hipMemcpyHostToDevice, h->stream));
    HIP_CHECK(h, hipMemcpyAsync(h->dScanSums + at, sumRef + b0, sizeof(float) * nb, hipMemcpyHostToDevice, h->stream));
    HIP_CHECK(h, hipMemcpyAsync(h->dScanSums + cap + at, sumsqRef + b0, sizeof(float) * nb, hipMemcpyHostToDevice, h->stream));
    if (phase_begin(h, h->stream, BIOEM_HIP_PHASE_CONVOLUTION, b0, b0 + nb, 0, 0) ||
        scan_prepare(h, at, nb, h->dWinConv, recs.data() + at))
      return 1;
    if (at + nb + OB > cap || b0 + nb == n)
    {
      const size_t o = (size_t) r0 * G;
      if (scan_flush(h, r0, at + nb, G, h->dScanSums, h->dScanSums + cap, logp_out + o, cc_out ? cc_out + o : nullptr,
                     params_out ? params_out + o : nullptr))
        return 1;
      r0 = b0 + nb;
    }
  }
  drain_phases(h);
  return 0;
}

// ---- density gradient of the log posterior of a request per model point (grad_kernels.hpp) ----
static_assert(sizeof(bioem_hip_grad_request) == 20, "request layout");

namespace
{
// the staging buffers of the gradient entries; a failed allocation (return 1) leaves the handle as it was
int grad_staging(bioem_hip_ctx *h, int G, int nPts)
{
  if (scan_staging(h, G)) // records, gathered orientations, particle spectra, the scan's preparation and results
    return 1;
  const size_t OB = (size_t) h->OB, M = (size_t) h->M, NN = (size_t) h->N * h->N, cap = (size_t) scan_capacity(h);
  if (!h->dGradMap)
  { // per record of a launch of the scan: records, coefficients, weights, parameters, orientations; the rest per batch
    Staging st = {h};
    st.get(h->dGradRec, cap);
    st.get(h->dGradCoef, 4 * cap);
    st.get(h->dGradW, cap);
    st.get(h->dGradMT, 2 * OB);
    st.get(h->dGradMap, OB * NN);
    st.get(h->dGradParams, cap);
    st.get(h->dGradSpec, OB * M);
    st.get(h->dGradAngles, cap);
    if (st.commit())
      return 1;
  }
  if (nPts <= h->gradCapPts)
    return 0;
  const size_t P = (size_t) nPts, tiles = (size_t) bioem_grad_tiles(nPts);
  Staging st = {h}; // the group that grows with the model: what it held goes once the larger buffers are all there
  st.get(h->dGradU, OB * P);
  st.get(h->dGradVS, OB * P);
  st.get(h->dGradPart, 2 * OB * tiles);
  st.get(h->dGradRows, OB * P);
  st.get(h->dGradAcc, P);
  if (st.commit())
    return 1;
  h->gradCapPts = nPts;
  return 0;
}

// the handle's own CTF sets as the candidates of the scan: packed from the device copy, a chunk of 64 at a time
int grad_candidates(bioem_hip_ctx *h)
{
  const size_t M = (size_t) h->M;
  for (int g0 = 0; g0 < h->nCTF; g0 += kScanLanes)
    HIP_CHECK(h, bioem_scan_pack_launch(h->stream, h->dCTF + M * (size_t) g0, std::min(kScanLanes, h->nCTF - g0), h->N,
                                        h->dScanPacked + M * (size_t) g0));
  HIP_CHECK(h, hipMemcpyAsync(h->dScanCtf, h->dCtfParam, sizeof(float) * 3 * h->nCTF, hipMemcpyDeviceToDevice, h->stream));
  return 0;
}
// the requests of a gradient entry as the front half takes them
struct GradRequests
{
  std::vector<BioemWindowRecord> recs;
  std::vector<BioemScanShift> shifts;
  std::vector<BioemGradRecord> grecs;
  std::vector<double> ws;
};

// looks at every request (and weight; null: all 1) before anything runs; 0, or the refusal's 2 with the request named
int grad_requests(bioem_hip_ctx *h, const Refuse &refuse, const bioem_hip_grad_request *req, const double *weights, int n,
                  int ownLists, GradRequests &q)
{
  const int G = h->nCTF, cap = scan_capacity(h); // records one launch of the scan serves: whole batches
  q.recs.resize((size_t) n);
  q.shifts.resize((size_t) n);
  q.grecs.resize((size_t) n);
  q.ws.assign((size_t) n, 1.);
  for (int i = 0; i < n; i++)
  {
    const bioem_hip_grad_request &r = req[i];
    int first, len;
    const char *why = bad_request(h, r, REQ_CONV | REQ_SHIFT, ownLists, first, len);
    if (!why && weights && !std::isfinite(weights[i]))
      why = "weight not finite";
    if (why)
      return refuse(request_refusal(h, i, why, r, REQ_CONV | REQ_SHIFT, len));
    q.recs[(size_t) i] = {first + r.orient, r.conv, r.particle, 0, {0.f, 0.f}};
    q.shifts[(size_t) i] = {r.shiftX, r.shiftY};
    q.grecs[(size_t) i] = {r.conv, r.particle, (i % cap) * G + r.conv, 0};
    if (weights)
      q.ws[(size_t) i] = weights[i];
  }
  return 0;
}

// The front half of the gradient entries for the requests [g0, g0 + ng) that one launch of the scan serves: the records,
// their orientations gathered into dGradAngles, per batch the projection and the scan's preparation into their places of
// the launch, then the linearisation point: one scan of the launch's records against the handle's own CTF sets, of which
// each record takes its own, and a, b, g (dGradCoef, dGradParams).
int grad_front(bioem_hip_ctx *h, const OrientList &src, const GradRequests &q, int g0, int ng)
{
  bioem_hip_ctx::Slot &s0 = h->slot[0];
  const int N = h->N, OB = h->OB, G = h->nCTF;
  const size_t M = (size_t) h->M;
  HIP_CHECK(h, hipMemcpyAsync(h->dScanRec, q.recs.data() + g0, sizeof(BioemWindowRecord) * ng, hipMemcpyHostToDevice, h->stream));
  HIP_CHECK(h, hipMemcpyAsync(h->dGradRec, q.grecs.data() + g0, sizeof(BioemGradRecord) * ng, hipMemcpyHostToDevice, h->stream));
  HIP_CHECK(h, hipMemcpyAsync(h->dGradW, q.ws.data() + g0, sizeof(double) * ng, hipMemcpyHostToDevice, h->stream));
  if (gather_matches(h, src, h->dScanRec, ng, h->dGradAngles)) // (once per launch of the scan: the back half reads them again)
    return 1;
  for (int b0 = 0; b0 < ng; b0 += OB)
  {
    const int nb = std::min(OB, ng - b0), r0 = g0 + b0;
    HIP_CHECK(h, hipMemcpyAsync(h->dScanShift, q.shifts.data() + r0, sizeof(BioemScanShift) * nb, hipMemcpyHostToDevice, h->stream));
    if (project_matches(h, src, h->dGradAngles, b0, nb, r0))
      return 1;
    if (phase_begin(h, h->stream, BIOEM_HIP_PHASE_CONVOLUTION, r0, r0 + nb, 0, 0))
      return 1;
    if (r0 == 0 && grad_candidates(h)) // (part of the first batch's preparation)
      return 1;
    if (unreorder_runs(h, q.recs.data() + r0, nb, h->dWinRef))
      return 1;
    HIP_CHECK(h, bioem_scan_prep_launch(h->stream, s0.specRef, h->dWinRef, h->dScanShift, nb, N, h->dTwD,
                                        h->dScanPw + M * (size_t) b0, h->dScanZ + M * (size_t) b0));
    if (phase_end(h, h->stream))
      return 1;
  }
  if (phase_begin(h, h->stream, BIOEM_HIP_PHASE_CONVOLUTION, g0, g0 + ng, 0, 0))
    return 1;
  HIP_CHECK(h, bioem_scan_launch(h->stream, h->dScanPacked, h->dScanCtf, G, h->dScanPw, h->dScanZ, h->dScanRec, h->dSumRef,
                                 h->dSumsqRef, h->pd, ng, N, h->dScanLogp, h->dScanCc, h->dScanParams));
  HIP_CHECK(h, bioem_grad_coef_launch(h->stream, h->dGradRec, h->dScanCc, h->dScanParams, h->dSumRef, h->dSumsqRef, ng, N,
                                      h->dGradCoef, h->dGradParams));
  return phase_end(h, h->stream);
}
} // namespace

int bioem_hip_model_gradient(bioem_hip_handle h, const bioem_hip_grad_request *req, const double *weights, int n, int ownLists,
                             double *grad_out, bioem_hip_grad_point *points_out, bioem_hip_param5 *params_out,
                             double *coef_out)
{
  if (!h)
    return 2;
  HIP_CHECK(h, hipSetDevice(h->device));
  const Refuse refuse = {h, "model_gradient"};
  if (h->dVolC)
    return refuse("the model is a volume");
  if (!req || n < 1)
    return refuse("null argument or no requests");
  if (!grad_out && !points_out)
    return refuse("grad_out and points_out both null");
  if (const char *why = missing_state(h, NEED_ALL, ownLists))
    return refuse(why);
  const int N = h->N, OB = h->OB, G = h->nCTF, nPts = h->nPts;
  const int cap = scan_capacity(h); // records one launch of the scan serves: whole batches
  GradRequests q;
  if (const int rc = grad_requests(h, refuse, req, weights, n, ownLists, q))
    return rc;
  if (grad_staging(h, G, nPts) || begin_analysis(h, true))
    return 1;
  bioem_hip_ctx::Slot &s0 = h->slot[0];
  const OrientList src = ownLists ? own_list(h) : shared_list(h);
  const size_t M = (size_t) h->M;
  int A, B;
  dft_split(N, A, B);
  HIP_CHECK(h, hipMemsetAsync(h->dGradAcc, 0, sizeof(bioem_hip_grad_point) * nPts, h->stream));
  for (int g0 = 0; g0 < n; g0 += cap) // the requests one launch of the scan serves
  {
    const int ng = std::min(cap, n - g0);
    if (grad_front(h, src, q, g0, ng))
      return 1;
    for (int b0 = 0; b0 < ng; b0 += OB)
    {
      const int nb = std::min(OB, ng - b0), r0 = g0 + b0;
      if (phase_begin(h, h->stream, BIOEM_HIP_PHASE_COMPARISON, r0, r0 + nb, 0, 0))
        return 1;
      HIP_CHECK(h, bioem_grad_spectrum_launch(h->stream, h->dScanPw + M * (size_t) b0, h->dScanZ + M * (size_t) b0, h->dCTF,
                                              h->dGradRec + b0, h->dGradCoef + 4 * (size_t) b0, 0, nb, N, h->dGradSpec));
      HIP_CHECK(h, bioem_grad_inverse_launch(h->stream, h->dGradSpec, nb, N, A, B, h->dTwD, s0.rowSpec, h->dGradMap));
      if (phase_end(h, h->stream) || phase_begin(h, h->stream, 3, r0, r0 + nb, 0, 0))
        return 1;
      HIP_CHECK(h, bioem_grad_gather_launch(h->stream, h->dPts, nPts, h->dGradAngles, b0, src.isQuat, N, h->pixelSize, h->shiftX,
                                            h->shiftY, h->dGradMap, nb, h->dGradU, h->dGradVS, h->dGradPart));
      HIP_CHECK(h, bioem_grad_fold_launch(h->stream, h->dGradU, h->dGradVS, h->dGradPart, h->dGradW + b0, nb, nPts, h->NormDen,
                                          h->dGradMT, h->dGradCoef + 4 * (size_t) b0, grad_out ? h->dGradRows : nullptr,
                                          h->dGradAcc));
      if (phase_end(h, h->stream))
        return 1;
      if (grad_out)
      { // (the rows' staging is reused by the next batch)
        HIP_CHECK(h, hipMemcpyAsync(grad_out + (size_t) r0 * nPts, h->dGradRows, sizeof(double) * (size_t) nb * nPts,
                                    hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(h, hipStreamSynchronize(h->stream));
      }
    }
    if (params_out)
      HIP_CHECK(h, hipMemcpyAsync(params_out + g0, h->dGradParams, sizeof(bioem_hip_param5) * ng, hipMemcpyDeviceToHost, h->stream));
    if (coef_out)
      HIP_CHECK(h, hipMemcpyAsync(coef_out + 4 * (size_t) g0, h->dGradCoef, sizeof(double) * 4 * ng, hipMemcpyDeviceToHost, h->stream));
    HIP_CHECK(h, hipStreamSynchronize(h->stream));
  }
  if (points_out)
    HIP_CHECK(h, hipMemcpy(points_out, h->dGradAcc, sizeof(bioem_hip_grad_point) * nPts, hipMemcpyDeviceToHost));
  drain_phases(h);
  return 0;
}

int bioem_hip_debug_grad_image(bioem_hip_handle h, const float *specConv, const float *specRef, const float *kernels,
                               const bioem_hip_param5 *params, const float *sumRef, const float *sumsqRef, const int *shiftXY,
                               int n, double *gmap_out, double *coef_out)
{
  if (!h)
    return 2;
  HIP_CHECK(h, hipSetDevice(h->device));
  const Refuse refuse = {h, "debug_grad_image"};
  if (!specConv || !specRef || !kernels || !params || !sumRef || !sumsqRef || !shiftXY || !gmap_out || !coef_out || n < 1)
    return refuse("null argument or no records");
  if (const int rc = debug_shifts_refused(h, refuse, shiftXY, n))
    return rc;
  if (grad_staging(h, 1, std::max(1, h->nPts)) || begin_analysis(h, true))
    return 1;
  bioem_hip_ctx::Slot &s0 = h->slot[0];
  const int N = h->N, OB = h->OB;
  const size_t M = (size_t) h->M, NN = (size_t) N * N;
  int A, B;
  dft_split(N, A, B);
  // cc: the scan of the conv spectra against one candidate, the kernel 1 + 0i (the products reproduce conv)
  std::vector<float2> unit(M, make_float2(1.f, 0.f));
  const float zero3[3] = {0.f, 0.f, 0.f};
  HIP_CHECK(h, hipMemcpyAsync(h->dScanRaw, unit.data(), sizeof(float2) * M, hipMemcpyHostToDevice, h->stream));
  HIP_CHECK(h, bioem_scan_pack_launch(h->stream, h->dScanRaw, 1, N, h->dScanPacked));
  HIP_CHECK(h, hipMemcpyAsync(h->dScanCtf, zero3, sizeof(zero3), hipMemcpyHostToDevice, h->stream));
  HIP_CHECK(h, hipStreamSynchronize(h->stream)); // (unit and zero3 are read by then)
  std::vector<BioemWindowRecord> recs((size_t) OB);
  std::vector<BioemGradRecord> grecs((size_t) OB);
  for (int b0 = 0; b0 < n; b0 += OB)
  {
    const int nb = std::min(OB, n - b0);
    for (int i = 0; i < nb; i++)
    {
      recs[(size_t) i] = {0, 0, i, 0, {0.f, 0.f}};
      grecs[(size_t) i] = {i, i, i, 0};
    }
    HIP_CHECK(h, hipMemcpyAsync(h->dScanRec, recs.data(), sizeof(BioemWindowRecord) * nb, hipMemcpyHostToDevice, h->stream));
    HIP_CHECK(h, hipMemcpyAsync(h->dGradRec, grecs.data(), sizeof(BioemGradRecord) * nb, hipMemcpyHostToDevice, h->stream));
    HIP_CHECK(h, hipMemcpyAsync(h->dScanShift, shiftXY + 2 * (size_t) b0, sizeof(BioemScanShift) * nb, hipMemcpyHostToDevice, h->stream));
    HIP_CHECK(h, hipMemcpyAsync(h->dWinConv, specConv + 2 * M * (size_t) b0, sizeof(float2) * M * nb, hipMemcpyHostToDevice, h->stream));
    HIP_CHECK(h, hipMemcpyAsync(h->dWinRef, specRef + 2 * M * (size_t) b0, sizeof(float2) * M * nb, hipMemcpyHostToDevice, h->stream));
    HIP_CHECK(h, hipMemcpyAsync(s0.specRef, kernels + 2 * M * (size_t) b0, sizeof(float2) * M * nb, hipMemcpyHostToDevice, h->stream));
    HIP_CHECK(h, hipMemcpyAsync(h->dScanSums, sumRef + b0, sizeof(float) * nb, hipMemcpyHostToDevice, h->stream));
    HIP_CHECK(h, hipMemcpyAsync(h->dScanSums + OB, sumsqRef + b0, sizeof(float) * nb, hipMemcpyHostToDevice, h->stream));
    HIP_CHECK(h, bioem_scan_prep_launch(h->stream, h->dWinConv, h->dWinRef, h->dScanShift, nb, N, h->dTwD, h->dScanPw, h->dScanZ));
    HIP_CHECK(h, bioem_scan_launch(h->stream, h->dScanPacked, h->dScanCtf, 1, h->dScanPw, h->dScanZ, h->dScanRec, h->dScanSums,
                                   h->dScanSums + OB, h->pd, nb, N, h->dScanLogp, h->dScanCc, nullptr));
    HIP_CHECK(h, hipMemcpyAsync(h->dGradParams, params + b0, sizeof(bioem_hip_param5) * nb, hipMemcpyHostToDevice, h->stream));
    HIP_CHECK(h, bioem_grad_coef_launch(h->stream, h->dGradRec, h->dScanCc, h->dGradParams, h->dScanSums, h->dScanSums + OB, nb,
                                        N, h->dGradCoef, nullptr));
    HIP_CHECK(h, bioem_grad_spectrum_launch(h->stream, h->dScanPw, h->dScanZ, s0.specRef, h->dGradRec, h->dGradCoef, 1, nb, N,
                                            h->dGradSpec));
    HIP_CHECK(h, bioem_grad_inverse_launch(h->stream, h->dGradSpec, nb, N, A, B, h->dTwD, s0.rowSpec, h->dGradMap));
    HIP_CHECK(h, hipMemcpyAsync(gmap_out + NN * (size_t) b0, h->dGradMap, sizeof(double) * NN * nb, hipMemcpyDeviceToHost, h->stream));
    HIP_CHECK(h, hipStreamSynchronize(h->stream));
    std::vector<double> c4(4 * (size_t) nb);
    HIP_CHECK(h, hipMemcpy(c4.data(), h->dGradCoef, sizeof(double) * 4 * nb, hipMemcpyDeviceToHost));
    for (int i = 0; i < nb; i++)
      for (int q = 0; q < 3; q++)
        coef_out[3 * (size_t) (b0 + i) + q] = c4[4 * (size_t) i + q];
  }
  return 0;
}

int bioem_hip_debug_grad_gather(bioem_hip_handle h, const double *gmaps, int o0, int nO, double *u_out)
{
  if (!h)
    return 2;
  HIP_CHECK(h, hipSetDevice(h->device));
  const Refuse refuse = {h, "debug_grad_gather"};
  if (h->dVolC)
    return refuse("the model is a volume");
  if (!gmaps || !u_out || nO < 1 || o0 < 0 || o0 + nO > h->nAnglesUp)
    return refuse("null argument, or orientations empty or outside the uploaded list");
  if (const char *why = missing_state(h, NEED_MODEL, 0))
    return refuse(why);
  if (grad_staging(h, 1, h->nPts) || begin_analysis(h, false)) // (buffer set 0 is not written)
    return 1;
  const int N = h->N, OB = h->OB, nPts = h->nPts;
  const size_t NN = (size_t) N * N;
  for (int b0 = 0; b0 < nO; b0 += OB)
  {
    const int nb = std::min(OB, nO - b0);
    HIP_CHECK(h, hipMemcpyAsync(h->dGradMap, gmaps + NN * (size_t) b0, sizeof(double) * NN * nb, hipMemcpyHostToDevice, h->stream));
    HIP_CHECK(h, bioem_grad_gather_launch(h->stream, h->dPts, nPts, h->dAngles, o0 + b0, h->isQuat, N, h->pixelSize, h->shiftX,
                                          h->shiftY, h->dGradMap, nb, h->dGradU, h->dGradVS, h->dGradPart));
    HIP_CHECK(h, hipMemcpyAsync(u_out + (size_t) b0 * nPts, h->dGradU, sizeof(double) * (size_t) nb * nPts, hipMemcpyDeviceToHost, h->stream));
    HIP_CHECK(h, hipStreamSynchronize(h->stream));
  }
  return 0;
}

// ---- summaries of the orientation posterior, reduced where the angle table lives (orient_kernels.hpp) ----
int bioem_hip_orientation_sums(bioem_hip_handle h, const double *logPrior, int iMapBegin, int iMapEnd, int ownLists,
                               bioem_hip_orient_sums *out)
{
  if (!h)
    return 2;
  HIP_CHECK(h, hipSetDevice(h->device));
  const Refuse refuse = {h, "orientation_sums"};
  if (!h->pd.writeAngles)
    return refuse("handle was created without WRITE_PROB_ANGLES");
  if (!out)
    return refuse("null argument");
  if (iMapBegin < 0 || iMapEnd > h->nMaps || iMapBegin >= iMapEnd)
    return refuse("particle range empty, reversed or outside [0, nMaps)");
  if (ownLists && (!h->dOwnAngles || h->ownOff.empty()))
    return refuse("no per-particle orientation lists (bioem_hip_upload_particle_orientation_lists)");
  if (ownLists && logPrior)
    return refuse("a prior per orientation does not go with per-particle orientation lists");
  if (!ownLists && h->nAnglesUp < h->angO1)
    return refuse("orientations not uploaded");
  if (compat_flush(h))
    return 1;
  const int nO = h->angO1 - h->angO0, np = iMapEnd - iMapBegin;
  if (!h->dOrientOut)
  {
    Staging st = {h};
    st.get(h->dOrientScratch, bioem_orient_scratch(nO, h->nMaps));
    st.get(h->dOrientQQ, (size_t) nO * 10);
    st.get(h->dOrientPrior, (size_t) nO);
    st.get(h->dOrientOut, (size_t) h->nMaps);
    if (st.commit())
      return 1;
  }
  if (logPrior)
    HIP_CHECK(h, hipMemcpyAsync(h->dOrientPrior, logPrior + h->angO0, sizeof(double) * (size_t) nO, hipMemcpyHostToDevice, h->stream));
  const bool moments = ownLists ? h->ownIsQuat != 0 : h->isQuat != 0;
  const bioem_hip_prob_angle *pang =
      reinterpret_cast<const bioem_hip_prob_angle *>(h->dProb + sizeof(bioem_hip_prob_map) * h->nMaps);
  if (phase_begin(h, h->stream, BIOEM_HIP_PHASE_COMPARISON, iMapBegin, iMapEnd, 0, 0))
    return 1;
  hipError_t le = hipSuccess;
  if (!ownLists && moments)
    le = bioem_orient_products_launch(h->stream, h->dAngles + h->angO0, nO, h->dOrientQQ);
  if (le == hipSuccess)
    le = bioem_orient_sums_launch(h->stream, pang, nO, h->nMaps, iMapBegin, np, ownLists ? 0 : h->angO0,
                                  logPrior ? h->dOrientPrior : nullptr, !ownLists && moments ? h->dOrientQQ : nullptr,
                                  ownLists ? h->dOwnAngles : nullptr, ownLists ? h->dOwnOff : nullptr, h->ownIsQuat,
                                  h->dOrientScratch, h->dOrientOut);
  if (le != hipSuccess || phase_end(h, h->stream))
  {
    drop_open_phase(h);
    if (le != hipSuccess)
      h->err = std::string("orientation_sums: launch failed: ") + hipGetErrorString(le);
    return 1;
  }
  HIP_CHECK(h, hipMemcpyAsync(out, h->dOrientOut, sizeof(bioem_hip_orient_sums) * (size_t) np, hipMemcpyDeviceToHost, h->stream));
  HIP_CHECK(h, hipStreamSynchronize(h->stream));
  drain_phases(h);
  return 0;
}

int bioem_hip_merge_orient_sums_host(int nShards, int nMaps, const bioem_hip_orient_sums *const *sums, bioem_hip_orient_sums *out)
{
  if (nShards < 1 || nMaps < 0 || !sums || !out)
    return 2;
  for (int s = 0; s < nShards; s++)
    if (!sums[s])
      return 2;
  for (int i = 0; i < nMaps; i++)
  {
    int who = -1;
    for (int s = 0; s < nShards; s++) // the maximum, ties to the lowest shard
      if (sums[s][i].count > 0. && (who < 0 || sums[s][i].m > sums[who][i].m))
        who = s;
    bioem_hip_orient_sums r;
    memset(&r, 0, sizeof(r));
    r.m = MIN_PROB;
    r.omax = -1.;
    r.hasMoments = sums[0][i].hasMoments;
    if (who >= 0)
    {
      r.m = sums[who][i].m;
      r.omax = sums[who][i].omax;
      for (int s = 0; s < nShards; s++)
      {
        const bioem_hip_orient_sums &a = sums[s][i];
        if (!(a.count > 0.))
          continue;
        const double d = a.m - r.m, e = exp(d);
        r.count += a.count;
        r.S0 += a.S0 * e;
        r.S1 += (a.S1 + d * a.S0) * e;
        r.S2 += a.S2 * (e * e);
        for (int k = 0; k < 10; k++)
          r.Q[k] += a.Q[k] * e;
      }
    }
    out[i] = r;
  }
  return 0;
}

namespace
{
// device buffers of one debug call
struct OrientDebugBufs
{
  std::vector<void *> p;
  ~OrientDebugBufs()
  {
    for (void *q : p)
      hipFree(q);
  }
  // bytes on the device, filled from src when there is one
  hipError_t get(void *d_, const void *src, size_t bytes)
  {
    void **d = static_cast<void **>(d_);
    *d = nullptr;
    hipError_t e = hipMalloc(d, std::max<size_t>(bytes, 1));
    if (e != hipSuccess)
      return e;
    p.push_back(*d);
    return src && bytes ? hipMemcpy(*d, src, bytes, hipMemcpyHostToDevice) : hipSuccess;
  }
};

int debug_orient(bioem_hip_ctx *h, const char *what, const bioem_hip_prob_angle *table, int nO, int nMaps, const float *angles4,
                 const long long *offsets, int isQuat, const double *logPrior, bioem_hip_orient_sums *out)
{
  if (!h)
    return 2;
  HIP_CHECK(h, hipSetDevice(h->device));
  const Refuse refuse = {h, what};
  if (!table || !out || nO < 1 || nMaps < 1 || (offsets && !angles4))
    return refuse("null argument or an empty table");
  std::vector<int> off;
  if (offsets)
  {
    off.resize((size_t) nMaps + 1);
    for (int p = 0; p <= nMaps; p++)
    {
      if (offsets[p] < 0 || offsets[p] > 0x7fffffffLL || (p && (offsets[p] < offsets[p - 1] || offsets[p] - offsets[p - 1] > nO)))
        return refuse("offsets negative, descending or a list longer than the table");
      off[(size_t) p] = (int) offsets[p];
    }
  }
  OrientDebugBufs B;
  bioem_hip_prob_angle *dTab = nullptr;
  float4 *dAng = nullptr;
  double *dQQ = nullptr, *dPri = nullptr, *dScr = nullptr;
  int *dOff = nullptr;
  bioem_hip_orient_sums *dOut = nullptr;
  const bool moments = angles4 && isQuat;
  const size_t nAng = offsets ? (size_t) off.back() : (size_t) nO;
  HIP_CHECK(h, B.get(&dTab, table, sizeof(bioem_hip_prob_angle) * (size_t) nO * nMaps));
  HIP_CHECK(h, B.get(&dScr, nullptr, sizeof(double) * bioem_orient_scratch(nO, nMaps)));
  HIP_CHECK(h, B.get(&dOut, nullptr, sizeof(bioem_hip_orient_sums) * (size_t) nMaps));
  if (angles4)
    HIP_CHECK(h, B.get(&dAng, angles4, sizeof(float4) * nAng));
  if (offsets)
    HIP_CHECK(h, B.get(&dOff, off.data(), sizeof(int) * off.size()));
  if (logPrior && !offsets)
    HIP_CHECK(h, B.get(&dPri, logPrior, sizeof(double) * (size_t) nO));
  if (moments && !offsets)
  {
    HIP_CHECK(h, B.get(&dQQ, nullptr, sizeof(double) * (size_t) nO * 10));
    HIP_CHECK(h, bioem_orient_products_launch(h->stream, dAng, nO, dQQ));
  }
  HIP_CHECK(h, bioem_orient_sums_launch(h->stream, dTab, nO, nMaps, 0, nMaps, 0, dPri, dQQ, dAng, dOff, moments, dScr, dOut));
  HIP_CHECK(h, hipMemcpyAsync(out, dOut, sizeof(bioem_hip_orient_sums) * (size_t) nMaps, hipMemcpyDeviceToHost, h->stream));
  HIP_CHECK(h, hipStreamSynchronize(h->stream));
  return 0;
}
} // namespace

int bioem_hip_debug_orient_sums(bioem_hip_handle h, const bioem_hip_prob_angle *table, int nO, int nMaps, const float *angles4,
                                int isQuat, const double *logPrior, bioem_hip_orient_sums *out)
{
  return debug_orient(h, "debug_orient_sums", table, nO, nMaps, angles4, nullptr, isQuat, logPrior, out);
}

int bioem_hip_debug_orient_sums_own(bioem_hip_handle h, const bioem_hip_prob_angle *table, int nO, int nMaps,
                                    const float *angles4, const long long *offsets, int isQuat, bioem_hip_orient_sums *out)
{
  if (h && !offsets)
  {
    h->err = "debug_orient_sums_own: null argument";
    return 2;
  }
  return debug_orient(h, "debug_orient_sums_own", table, nO, nMaps, angles4, offsets, isQuat, nullptr, out);
}

// k_topk_angles on a table handed in, with the launch shape of topk_device
int bioem_hip_debug_topk(bioem_hip_handle h, const bioem_hip_prob_angle *table, int nO, int nMaps, int o0, int K, int W,
                         double numconst, bioem_hip_angle_candidate *out)
{
  if (!h)
    return 2;
  HIP_CHECK(h, hipSetDevice(h->device));
  const Refuse refuse = {h, "debug_topk"};
  if (!table || !out || nO < 1 || nMaps < 1 || o0 < 0)
    return refuse("null argument, an empty table or a negative offset");
  if (K < 1 || (W != K && W != 2 * K - 1))
    return refuse("K < 1, or a width that is neither K nor 2K - 1");
  OrientDebugBufs B;
  bioem_hip_prob_angle *dTab = nullptr;
  bioem_hip_angle_candidate *dOut = nullptr;
  const size_t outBytes = sizeof(bioem_hip_angle_candidate) * (size_t) nMaps * W;
  HIP_CHECK(h, B.get(&dTab, table, sizeof(bioem_hip_prob_angle) * (size_t) nO * nMaps));
  HIP_CHECK(h, B.get(&dOut, nullptr, outBytes));
  hipLaunchKernelGGL(k_topk_angles, dim3((nMaps + 63) / 64), dim3(64), 0, h->stream, dTab, nO, nMaps, o0, K, W, numconst, dOut);
  HIP_CHECK(h, hipGetLastError());
  HIP_CHECK(h, hipMemcpyAsync(out, dOut, outBytes, hipMemcpyDeviceToHost, h->stream));
  HIP_CHECK(h, hipStreamSynchronize(h->stream));
  return 0;
}

// ---- occupancy of every orientation over the particles (orient_kernels.hpp: k_orient_occ) ----
namespace
{
// the normalisers of the particles as the kernel reads them: m, 1 / S0 (0: the particle is left out), omax (-1 then)
struct OccNormalisers
{
  std::vector<double> m, rS0;
  std::vector<int> omax;
  explicit OccNormalisers(const bioem_hip_orient_sums *sums, int np) : m((size_t) np), rS0((size_t) np), omax((size_t) np)
  {
    for (int i = 0; i < np; i++)
    {
      const bioem_hip_orient_sums &s = sums[i];
      const bool counts = s.count > 0. && s.S0 > 0. && s.S0 < INFINITY && s.omax >= 0. && s.omax <= 2147483647.;
      m[(size_t) i] = counts ? s.m : 0.;
      rS0[(size_t) i] = counts ? 1. / s.S0 : 0.;
      omax[(size_t) i] = counts ? (int) s.omax : -1;
    }
  }
};
} // namespace

int bioem_hip_orientation_occupancy(bioem_hip_handle h, const double *logPrior, const bioem_hip_orient_sums *sums, int iMapBegin,
                                    int iMapEnd, bioem_hip_orient_occ *out)
{
  if (!h)
    return 2;
  HIP_CHECK(h, hipSetDevice(h->device));
  const Refuse refuse = {h, "orientation_occupancy"};
  if (!h->pd.writeAngles)
    return refuse("handle was created without WRITE_PROB_ANGLES");
  if (!sums || !out)
    return refuse("null argument");
  if (iMapBegin < 0 || iMapEnd > h->nMaps || iMapBegin >= iMapEnd)
    return refuse("particle range empty, reversed or outside [0, nMaps)");
  if (h->dOwnAngles && !h->ownOff.empty())
    return refuse("the handle holds per-particle orientation lists: its rows are list positions, not shared orientations");
  if (h->nAnglesUp < h->angO1)
    return refuse("orientations not uploaded");
  if (compat_flush(h))
    return 1;
  const int nO = h->angO1 - h->angO0, np = iMapEnd - iMapBegin;
  if (!h->dOccOut)
  {
    Staging st = {h};
    st.get(h->dOccM, (size_t) h->nMaps);
    st.get(h->dOccRS0, (size_t) h->nMaps);
    st.get(h->dOccPrior, (size_t) nO);
    st.get(h->dOccOmax, (size_t) h->nMaps);
    st.get(h->dOccOut, (size_t) nO);
    if (st.commit())
      return 1;
  }
  const OccNormalisers N(sums, np);
  // the copies below read N and the caller's buffers asynchronously: whichever way this call ends, the stream is drained
  // before N goes (the guard is destroyed first)
  struct Drain
  {
    hipStream_t st;
    ~Drain() { (void) hipStreamSynchronize(st); }
  } drain = {h->stream};
  HIP_CHECK(h, hipMemcpyAsync(h->dOccM, N.m.data(), sizeof(double) * (size_t) np, hipMemcpyHostToDevice, h->stream));
  HIP_CHECK(h, hipMemcpyAsync(h->dOccRS0, N.rS0.data(), sizeof(double) * (size_t) np, hipMemcpyHostToDevice, h->stream));
  HIP_CHECK(h, hipMemcpyAsync(h->dOccOmax, N.omax.data(), sizeof(int) * (size_t) np, hipMemcpyHostToDevice, h->stream));
  if (logPrior)
    HIP_CHECK(h, hipMemcpyAsync(h->dOccPrior, logPrior + h->angO0, sizeof(double) * (size_t) nO, hipMemcpyHostToDevice, h->stream));
  const bioem_hip_prob_angle *pang =
      reinterpret_cast<const bioem_hip_prob_angle *>(h->dProb + sizeof(bioem_hip_prob_map) * h->nMaps);
  if (phase_begin(h, h->stream, BIOEM_HIP_PHASE_COMPARISON, iMapBegin, iMapEnd, 0, 0))
    return 1;
  const hipError_t le = bioem_orient_occ_launch(h->stream, pang, nO, h->nMaps, iMapBegin, np, h->angO0,
                                                logPrior ? h->dOccPrior : nullptr, h->dOccM, h->dOccRS0, h->dOccOmax, h->dOccOut);
  if (le != hipSuccess || phase_end(h, h->stream))
  {
    drop_open_phase(h);
    if (le != hipSuccess)
      h->err = std::string("orientation_occupancy: launch failed: ") + hipGetErrorString(le);
    return 1;
  }
  HIP_CHECK(h, hipMemcpyAsync(out, h->dOccOut, sizeof(bioem_hip_orient_occ) * (size_t) nO, hipMemcpyDeviceToHost, h->stream));
  HIP_CHECK(h, hipStreamSynchronize(h->stream));
  drain_phases(h);
  return 0;
}

int bioem_hip_debug_orient_occupancy(bioem_hip_handle h, const bioem_hip_prob_angle *table, int nO, int nMaps, const double *logPrior,
                                     const bioem_hip_orient_sums *sums, int p0, int p1, int o0, bioem_hip_orient_occ *out)
{
  if (!h)
    return 2;
  HIP_CHECK(h, hipSetDevice(h->device));
  const Refuse refuse = {h, "debug_orient_occupancy"};
  if (!table || !sums || !out || nO < 1 || nMaps < 1)
    return refuse("null argument or an empty table");
  if (p0 < 0 || p1 > nMaps || p0 >= p1)
    return refuse("particle range empty, reversed or outside [0, nMaps)");
  if (o0 < 0 || o0 > 0x7fffffff - nO)
    return refuse("first orientation index negative or too large");
  const int np = p1 - p0;
  const OccNormalisers N(sums, np);
  OrientDebugBufs B;
  bioem_hip_prob_angle *dTab = nullptr;
  double *dPri = nullptr, *dM = nullptr, *dRS0 = nullptr;
  int *dOmax = nullptr;
  bioem_hip_orient_occ *dOut = nullptr;
  HIP_CHECK(h, B.get(&dTab, table, sizeof(bioem_hip_prob_angle) * (size_t) nO * nMaps));
  HIP_CHECK(h, B.get(&dM, N.m.data(), sizeof(double) * (size_t) np));
  HIP_CHECK(h, B.get(&dRS0, N.rS0.data(), sizeof(double) * (size_t) np));
  HIP_CHECK(h, B.get(&dOmax, N.omax.data(), sizeof(int) * (size_t) np));
  HIP_CHECK(h, B.get(&dOut, nullptr, sizeof(bioem_hip_orient_occ) * (size_t) nO));
  if (logPrior)
    HIP_CHECK(h, B.get(&dPri, logPrior, sizeof(double) * (size_t) nO));
  HIP_CHECK(h, bioem_orient_occ_launch(h->stream, dTab, nO, nMaps, p0, np, o0, dPri, dM, dRS0, dOmax, dOut));
  HIP_CHECK(h, hipMemcpyAsync(out, dOut, sizeof(bioem_hip_orient_occ) * (size_t) nO, hipMemcpyDeviceToHost, h->stream));
  HIP_CHECK(h, hipStreamSynchronize(h->stream));
  return 0;
}

} // extern "C" (closed around the helpers of the volume model)

// ---- a volume as the model (slice_kernels.hpp) ----
namespace
{
// exp(+2 pi i k c / PN) for the stored index i of an axis of PN entries (i <= PN / 2 stands for k = i, a larger one for i -
// PN): made on the host with libm, as the sinc^2 table of the reconstruction
void centre_table(int PN, double c, double2 *e)
{
  for (int i = 0; i < PN; i++)
  {
    const int k = i <= PN / 2 ? i : i - PN;
    const double ang = 2.0 * M_PI * ((double) k * c) / (double) PN;
    e[i] = c == 0. ? make_double2(1., 0.) : make_double2(cos(ang), sin(ang));
  }
}

// spec on the device ([PN][PN][PH], un-centred; owned by the caller, not yet a field of the handle) becomes the handle's
// model: centred, Re C(0) checked, and only then the model it replaces goes.  dSpec is released on every failure.
int volume_commit(bioem_hip_ctx *h, const Refuse &refuse, double2 *dSpec, int pad, const double *centre, int shiftX, int shiftY,
                  int flags, bool fromSpectrum)
{
  const int N = h->N, PN = pad * N, o = (N + 1) / 2;
  std::vector<double2> tab((size_t) 4 * PN);
  for (int j = 0; j < PN; j++)
    tab[(size_t) j] = twiddle_d(j, PN);
  for (int d = 0; d < 3; d++)
    centre_table(PN, centre ? centre[d] : 0., tab.data() + (size_t) (d + 1) * PN);
  double2 *dTab = nullptr;
  double2 c0 = make_double2(0., 0.);
  int rc = upload(h, dTab, tab.data(), tab.size());
  if (!rc)
  {
    hipError_t e = bioem_slice_centre_launch(h->stream, dSpec, PN, o, dTab, dTab + PN);
    if (e == hipSuccess)
      e = hipMemcpyAsync(&c0, dSpec, sizeof(double2), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess)
      e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess)
    {
      h->err = std::string("upload of a volume model failed: ") + hipGetErrorString(e);
      rc = 1;
    }
  }
  dev_release(h, dTab);
  if (rc)
  {
    dev_release(h, dSpec);
    return rc;
  }
  if (!(c0.x > 0.) || !std::isfinite(c0.x))
  {
    dev_release(h, dSpec);
    char buf[128];
    snprintf(buf, sizeof(buf), "the total density Re C(0) = %g is not positive", c0.x);
    return refuse(buf);
  }
  // nothing queued may still read the model that goes
  if (const hipError_t e = hipDeviceSynchronize())
  {
    dev_release(h, dSpec);
    h->err = std::string("upload of a volume model failed: ") + hipGetErrorString(e);
    return 1;
  }
  dev_release(h, h->dVolC);
  if (h->volAPad != pad)
  { // A beside C is kept for a model of the same size only
    dev_release(h, h->dVolA);
    h->volAPad = 0;
  }
  dev_release(h, h->dPts);
  dev_release(h, h->dStamp);
  h->nPts = 0;
  h->iradMax = 0;
  h->modelRadius = 0.;
  h->dVolC = dSpec;
  h->volPad = pad;
  for (int d = 0; d < 3; d++)
    h->volCentre[d] = centre ? centre[d] : 0.;
  h->volFlags = flags;
  h->volFromSpectrum = fromSpectrum;
  h->NormDen = (float) c0.x;
  h->shiftX = shiftX;
  h->shiftY = shiftY;
  void_slot(h->slot[0]);
  void_slot(h->slot[1]);
  return 0;
}

const char *volume_args(int pad, const void *data, const double *centre)
{
  if (pad != 1 && pad != 2)
    return "pad must be 1 or 2";
  if (!data)
    return "null argument";
  if (centre && (!std::isfinite(centre[0]) || !std::isfinite(centre[1]) || !std::isfinite(centre[2])))
    return "centre not finite";
  return nullptr;
}
} // namespace

extern "C" {

int bioem_hip_upload_model_spectrum(bioem_hip_handle h, const double *spec, int pad, const double *centre, int shiftX,
                                    int shiftY)
{
  if (!h)
    return 2;
  HIP_CHECK(h, hipSetDevice(h->device));
  const Refuse refuse = {h, "upload_model_spectrum"};
  if (const char *why = volume_args(pad, spec, centre))
    return refuse(why);
  const size_t PN = (size_t) pad * h->N, V = PN * PN * (PN / 2 + 1);
  for (size_t e = 0; e < 2 * V; e++)
    if (!std::isfinite(spec[e]))
      return refuse("spectrum not finite at coefficient " + std::to_string(e / 2));
  if (begin_analysis(h, false))
    return 1;
  double2 *dSpec = nullptr;
  if (upload(h, dSpec, reinterpret_cast<const double2 *>(spec), V))
  {
    dev_release(h, dSpec);
    (void) hipGetLastError();
    return 1;
  }
  return volume_commit(h, refuse, dSpec, pad, centre, shiftX, shiftY, 0, true);
}

int bioem_hip_upload_model_volume(bioem_hip_handle h, const float *vol, int pad, int flags, const double *centre, int shiftX,
                                  int shiftY)
{
  if (!h)
    return 2;
  HIP_CHECK(h, hipSetDevice(h->device));
  const Refuse refuse = {h, "upload_model_volume"};
  if (const char *why = volume_args(pad, vol, centre))
    return refuse(why);
  if (flags & ~BIOEM_HIP_VOLUME_PRECORRECT)
    return refuse("unknown flag bits");
  const size_t N = (size_t) h->N, PN = (size_t) pad * N, PH = PN / 2 + 1, NNN = N * N * N;
  for (size_t e = 0; e < NNN; e++)
    if (!std::isfinite(vol[e]))
      return refuse("volume not finite at voxel " + std::to_string(e));
  // the density in double, divided by the transform of the trilinear kernel on the padded grid where asked for
  std::vector<double> sinc2(N, 1.);
  if (flags & BIOEM_HIP_VOLUME_PRECORRECT)
    for (size_t x = 0; x < N; x++)
    {
      const double t = M_PI * ((double) x - (double) ((N + 1) / 2)) / (double) PN;
      const double s = t == 0. ? 1. : sin(t) / t;
      sinc2[x] = s * s;
    }
  std::vector<double2> in(NNN);
  for (size_t x0 = 0, e = 0; x0 < N; x0++)
    for (size_t x1 = 0; x1 < N; x1++)
      for (size_t x2 = 0; x2 < N; x2++, e++)
      {
        double v = (double) vol[e];
        if (flags & BIOEM_HIP_VOLUME_PRECORRECT)
          v = v / ((sinc2[x0] * sinc2[x1]) * sinc2[x2]);
        in[e] = make_double2(v, 0.);
      }
  std::vector<double2> twP(PN);
  for (size_t j = 0; j < PN; j++)
    twP[j] = twiddle_d((long long) j, (int) PN);
  if (begin_analysis(h, false))
    return 1;
  // axis 2: [N][N][N] -> [N][N][PH]; axis 1: -> [N][PN][PH]; axis 0: -> [PN][PN][PH]
  double2 *dA = nullptr, *dB = nullptr, *dSpec = nullptr, *dTw = nullptr;
  int rc = dev_alloc(h, dA, std::max(NNN, N * PN * PH)) || dev_alloc(h, dB, N * N * PH) || dev_alloc(h, dSpec, PN * PN * PH) ||
           dev_alloc(h, dTw, PN);
  if (!rc)
  {
    hipError_t e = hipMemcpyAsync(dA, in.data(), sizeof(double2) * NNN, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess)
      e = hipMemcpyAsync(dTw, twP.data(), sizeof(double2) * PN, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess)
      e = bioem_slice_axis_launch(h->stream, dA, N * N, (int) N, (int) PH, 1, (int) PN, dTw, dB);
    if (e == hipSuccess)
      e = bioem_slice_axis_launch(h->stream, dB, N, (int) N, (int) PN, PH, (int) PN, dTw, dA);
    if (e == hipSuccess)
      e = bioem_slice_axis_launch(h->stream, dA, 1, (int) N, (int) PN, PN * PH, (int) PN, dTw, dSpec);
    if (e == hipSuccess)
      e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess)
    {
      h->err = std::string("upload_model_volume failed: ") + hipGetErrorString(e);
      rc = 1;
    }
  }
  else
    (void) hipGetLastError();
  dev_release(h, dA);
  dev_release(h, dB);
  dev_release(h, dTw);
  if (rc)
  {
    dev_release(h, dSpec);
    return 1;
  }
  return volume_commit(h, refuse, dSpec, pad, centre, shiftX, shiftY, flags, false);
}

int bioem_hip_debug_slices(bioem_hip_handle h, const float *angles4, int n, int isQuat, double *out)
{
  if (!h)
    return 2;
  HIP_CHECK(h, hipSetDevice(h->device));
  const Refuse refuse = {h, "debug_slices"};
  if (!angles4 || !out || n < 1)
    return refuse("null argument or no orientations");
  if (!h->dVolC)
    return refuse("the model is not a volume");
  const size_t M = (size_t) h->M, OB = (size_t) h->OB;
  if (!h->dSliceOut)
  {
    Staging st = {h};
    st.get(h->dSliceAngles, OB);
    st.get(h->dSliceR, 9 * OB);
    st.get(h->dSliceOut, OB * M);
    if (st.commit())
    {
      h->err = "debug_slices: device memory";
      return 1;
    }
  }
  if (begin_analysis(h, false))
    return 1;
  for (int g0 = 0; g0 < n; g0 += h->OB)
  {
    const int nb = std::min(h->OB, n - g0);
    HIP_CHECK(h, hipMemcpyAsync(h->dSliceAngles, angles4 + 4 * (size_t) g0, sizeof(float4) * nb, hipMemcpyHostToDevice,
                                h->stream));
    // (poisoned: a bin the kernel leaves unwritten reads back as a NaN)
    HIP_CHECK(h, hipMemsetAsync(h->dSliceOut, 0xff, sizeof(double2) * M * nb, h->stream));
    HIP_CHECK(h, bioem_recon_matrices_launch(h->stream, h->dSliceAngles, nullptr, isQuat ? 1 : 0, nb, h->dSliceR));
    HIP_CHECK(h, bioem_slice_project_launch(h->stream, h->dVolC, h->volPad, h->dSliceR, nb, h->N, h->dTwD, h->shiftX,
                                            h->shiftY, (double) h->NormDen, nullptr, h->dSliceOut, nullptr));
    HIP_CHECK(h, hipMemcpyAsync(out + 2 * M * (size_t) g0, h->dSliceOut, sizeof(double2) * M * nb, hipMemcpyDeviceToHost,
                                h->stream));
    HIP_CHECK(h, hipStreamSynchronize(h->stream));
  }
  return 0;
}

} // extern "C" (closed around the helpers of the volume gradient)

// ---- the gradient with respect to the voxels of a volume model (vgrad_kernels.hpp) ----
namespace
{
// the staging of the volume-gradient entries; a failed allocation (return 1) leaves the handle as it was
int vgrad_staging(bioem_hip_ctx *h, bool withA = true)
{
  const size_t OB = (size_t) h->OB, M = (size_t) h->M, cap = (size_t) scan_capacity(h);
  if (!h->dVgY)
  {
    Staging st = {h};
    st.get(h->dVgY, OB * M);
    st.get(h->dVgSlices, OB * M);
    st.get(h->dVgR, 9 * cap);
    st.get(h->dVgView, (size_t) kVgradViewDoubles * cap);
    st.get(h->dVgFlag, cap);
    if (st.commit())
      return 1;
  }
  if (withA && h->volAPad != h->volPad)
  { // A beside C: 16 PN^2 PH bytes
    const size_t PN = (size_t) h->volPad * h->N;
    Staging st = {h};
    st.get(h->dVolA, PN * PN * (PN / 2 + 1));
    if (st.commit())
      return 1;
    h->volAPad = h->volPad;
  }
  return 0;
}

std::string vgrad_flag_reason(int flag)
{
  if (flag == 1)
    return "rows 0 and 1 of the orientation's matrix are rank-deficient or not finite";
  char buf[128];
  snprintf(buf, sizeof(buf), "the orientation's matrix shrinks too much: candidate half-width beyond %.1f", kVgradHalfCap);
  return buf;
}

// matrices, view parameters and flags of the n orientations angles[0 ... n), left on the device
int vgrad_views(bioem_hip_ctx *h, const float4 *dAngles, int isQuat, int n)
{
  HIP_CHECK(h, bioem_recon_matrices_launch(h->stream, dAngles, nullptr, isQuat ? 1 : 0, n, h->dVgR));
  HIP_CHECK(h, bioem_vgrad_views_launch(h->stream, h->dVgR, n, h->volPad, h->dVgView, h->dVgFlag));
  return 0;
}

// the same, and the flags looked at on the host; first: the first flagged view, or -1
int vgrad_views_checked(bioem_hip_ctx *h, const float4 *dAngles, int isQuat, int n, int &first, int &flag)
{
  std::vector<int> flags((size_t) n);
  if (vgrad_views(h, dAngles, isQuat, n))
    return 1;
  HIP_CHECK(h, hipMemcpyAsync(flags.data(), h->dVgFlag, sizeof(int) * n, hipMemcpyDeviceToHost, h->stream));
  HIP_CHECK(h, hipStreamSynchronize(h->stream));
  first = -1;
  flag = 0;
  for (int i = 0; i < n && first < 0; i++)
    if (flags[(size_t) i])
    {
      first = i;
      flag = flags[(size_t) i];
    }
  return 0;
}

// gvol [N][N][N] on the host from A on the device (which becomes A_spec): the un-centring, the three passes and the
// real part, divided by the sinc^2 product where the model was uploaded as a volume with precorrection
int vgrad_adjoint(bioem_hip_ctx *h, const char *what, double2 *dA, double *vol_out)
{
  const size_t N = (size_t) h->N, PN = (size_t) h->volPad * N, PH = PN / 2 + 1, NNN = N * N * N;
  const int o = (int) ((N + 1) / 2);
  const int correct = (h->volFlags & BIOEM_HIP_VOLUME_PRECORRECT) && !h->volFromSpectrum;
  std::vector<double2> tab(4 * PN);
  for (size_t j = 0; j < PN; j++)
    tab[j] = twiddle_d((long long) j, (int) PN);
  for (int d = 0; d < 3; d++)
    centre_table((int) PN, h->volCentre[d], tab.data() + (size_t) (d + 1) * PN);
  std::vector<double> sinc2(N, 1.);
  if (correct)
    for (size_t x = 0; x < N; x++)
    { // (the table of bioem_hip_upload_model_volume)
      const double t = M_PI * ((double) x - (double) ((N + 1) / 2)) / (double) PN;
      const double s = t == 0. ? 1. : sin(t) / t;
      sinc2[x] = s * s;
    }
  double2 *dT1 = nullptr, *dT2 = nullptr, *dTab = nullptr;
  double *dG = nullptr, *dSinc = nullptr;
  // axis 0: [PN][PN][PH] -> [N][PN][PH]; axis 1: -> [N][N][PH]; axis 2: -> [N][N][N] (in the buffer of the first pass)
  int rc = dev_alloc(h, dT1, std::max(N * PN * PH, NNN)) || dev_alloc(h, dT2, N * N * PH) || dev_alloc(h, dTab, 4 * PN) ||
           dev_alloc(h, dG, NNN) || dev_alloc(h, dSinc, N);
  if (!rc)
  {
    hipError_t e = hipMemcpyAsync(dTab, tab.data(), sizeof(double2) * 4 * PN, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess)
      e = hipMemcpyAsync(dSinc, sinc2.data(), sizeof(double) * N, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess)
      e = bioem_vgrad_uncentre_launch(h->stream, dA, (int) PN, o, dTab, dTab + PN);
    if (e == hipSuccess)
      e = bioem_vgrad_axis_launch(h->stream, dA, 1, (int) PN, (int) N, PN * PH, (int) PN, dTab, dT1);
    if (e == hipSuccess)
      e = bioem_vgrad_axis_launch(h->stream, dT1, N, (int) PN, (int) N, PH, (int) PN, dTab, dT2);
    if (e == hipSuccess)
      e = bioem_vgrad_axis_launch(h->stream, dT2, N * N, (int) PH, (int) N, 1, (int) PN, dTab, dT1);
    if (e == hipSuccess)
      e = bioem_vgrad_finish_launch(h->stream, dT1, (int) N, dSinc, correct, dG);
    if (e == hipSuccess)
      e = hipMemcpyAsync(vol_out, dG, sizeof(double) * NNN, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess)
      e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess)
    {
      h->err = std::string(what) + " failed: " + hipGetErrorString(e);
      rc = 1;
    }
  }
  else
    (void) hipGetLastError();
  dev_release(h, dT1);
  dev_release(h, dT2);
  dev_release(h, dTab);
  dev_release(h, dG);
  dev_release(h, dSinc);
  return rc;
}
} // namespace

extern "C" {

int bioem_hip_volume_gradient(bioem_hip_handle h, const bioem_hip_grad_request *req, const double *weights, int n, int ownLists,
                              double *vol_out, double *spec_out, double *coef_out, bioem_hip_param5 *params_out,
                              double *stats_out)
{
  if (!h)
    return 2;
  HIP_CHECK(h, hipSetDevice(h->device));
  const Refuse refuse = {h, "volume_gradient"};
  if (!req || n < 1)
    return refuse("null argument or no requests");
  if (!vol_out && !spec_out)
    return refuse("vol_out and spec_out both null");
  if (const char *why = missing_state(h, NEED_ALL, ownLists))
    return refuse(why);
  if (!h->dVolC)
    return refuse("the model is a point model");
  const int N = h->N, OB = h->OB, G = h->nCTF, pad = h->volPad;
  const int cap = scan_capacity(h); // records one launch of the scan serves: whole batches
  GradRequests q;
  if (const int rc = grad_requests(h, refuse, req, weights, n, ownLists, q))
    return rc;
  double sumw = 0.;
  for (int i = 0; i < n; i++)
    sumw += q.ws[(size_t) i];
  if (grad_staging(h, G, 0) || vgrad_staging(h) || begin_analysis(h, true))
    return 1;
  const OrientList src = ownLists ? own_list(h) : shared_list(h);
  const size_t M = (size_t) h->M, PN = (size_t) pad * N, V = PN * PN * (PN / 2 + 1);
  // every request's matrix is looked at before anything is inserted: a refusal leaves nothing half done
  for (int g0 = 0; g0 < n; g0 += cap)
  {
    const int ng = std::min(cap, n - g0);
    int bad, flag;
    HIP_CHECK(h, hipMemcpyAsync(h->dScanRec, q.recs.data() + g0, sizeof(BioemWindowRecord) * ng, hipMemcpyHostToDevice, h->stream));
    if (gather_matches(h, src, h->dScanRec, ng, h->dGradAngles) ||
        vgrad_views_checked(h, h->dGradAngles, src.isQuat, ng, bad, flag))
      return 1;
    if (bad >= 0)
    {
      int first, len;
      orient_span(h, ownLists, req[g0 + bad].particle, first, len);
      return refuse(request_refusal(h, g0 + bad, vgrad_flag_reason(flag).c_str(), req[g0 + bad], REQ_CONV | REQ_SHIFT, len));
    }
  }
  std::vector<double> coef(4 * (size_t) std::min(cap, n));
  double notFinite = 0.;
  for (int g0 = 0; g0 < n; g0 += cap) // the requests one launch of the scan serves
  {
    const int ng = std::min(cap, n - g0);
    // the front half of bioem_hip_model_gradient, then the matrices and view parameters of the launch's orientations
    if (grad_front(h, src, q, g0, ng) || vgrad_views(h, h->dGradAngles, src.isQuat, ng))
      return 1;
    for (int b0 = 0; b0 < ng; b0 += OB)
    {
      const int nb = std::min(OB, ng - b0), r0 = g0 + b0;
      // phase 2: the gradient spectrum, Y and <C, A_r> through the adjoint identity, on the double slice of the request
      if (phase_begin(h, h->stream, BIOEM_HIP_PHASE_COMPARISON, r0, r0 + nb, 0, 0))
        return 1;
      HIP_CHECK(h, bioem_grad_spectrum_launch(h->stream, h->dScanPw + M * (size_t) b0, h->dScanZ + M * (size_t) b0, h->dCTF,
                                              h->dGradRec + b0, h->dGradCoef + 4 * (size_t) b0, 0, nb, N, h->dGradSpec));
      HIP_CHECK(h, bioem_vgrad_prepare_launch(h->stream, h->dGradSpec, h->dGradW + b0, nb, N, h->dTwD, h->shiftX, h->shiftY, 1,
                                              h->dVgY));
      HIP_CHECK(h, bioem_slice_project_launch(h->stream, h->dVolC, pad, h->dVgR + 9 * (size_t) b0, nb, N, h->dTwD, h->shiftX,
                                              h->shiftY, (double) h->NormDen, nullptr, h->dVgSlices, nullptr));
      HIP_CHECK(h, bioem_vgrad_dot_launch(h->stream, h->dGradSpec, h->dVgSlices, nb, N, h->dGradCoef + 4 * (size_t) b0 + 3, 4));
      // phase 3: the back-insertion
      if (phase_end(h, h->stream) || phase_begin(h, h->stream, 3, r0, r0 + nb, 0, 0))
        return 1;
      HIP_CHECK(h, bioem_vgrad_insert_launch(h->stream, h->dVgY, h->dVgR + 9 * (size_t) b0,
                                             h->dVgView + (size_t) kVgradViewDoubles * b0, nb, N, pad, 1, r0 == 0, h->dVolA));
      if (phase_end(h, h->stream))
        return 1;
    }
    if (params_out)
      HIP_CHECK(h, hipMemcpyAsync(params_out + g0, h->dGradParams, sizeof(bioem_hip_param5) * ng, hipMemcpyDeviceToHost, h->stream));
    HIP_CHECK(h, hipMemcpyAsync(coef.data(), h->dGradCoef, sizeof(double) * 4 * ng, hipMemcpyDeviceToHost, h->stream));
    HIP_CHECK(h, hipStreamSynchronize(h->stream));
    for (int i = 0; i < ng; i++)
    {
      const double *c = coef.data() + 4 * (size_t) i;
      if (!(std::isfinite(c[0]) && std::isfinite(c[1]) && std::isfinite(c[2])))
        notFinite += 1.;
    }
    if (coef_out)
      memcpy(coef_out + 4 * (size_t) g0, coef.data(), sizeof(double) * 4 * ng);
  }
  if (spec_out)
    HIP_CHECK(h, hipMemcpy(spec_out, h->dVolA, sizeof(double2) * V, hipMemcpyDeviceToHost));
  if (vol_out)
  { // one more record of phase 3 with an empty request range [n, n): the transpose of the upload's passes
    if (phase_begin(h, h->stream, 3, n, n, 0, 0))
      return 1;
    if (vgrad_adjoint(h, "volume_gradient", h->dVolA, vol_out))
    { // (the open record goes; those that closed are delivered)
      drop_open_phase(h);
      drain_phases(h);
      return 1;
    }
    if (phase_end(h, h->stream))
      return 1;
  }
  if (stats_out)
  {
    stats_out[0] = (double) n;
    stats_out[1] = sumw;
    stats_out[2] = notFinite;
  }
  drain_phases(h);
  return 0;
}

int bioem_hip_debug_volume_backproject(bioem_hip_handle h, const float *angles4, int n, int isQuat, const double *gamma,
                                       const double *weights, int cull, double *spec_out)
{
  if (!h)
    return 2;
  HIP_CHECK(h, hipSetDevice(h->device));
  const Refuse refuse = {h, "debug_volume_backproject"};
  if (!angles4 || !gamma || !spec_out || n < 1)
    return refuse("null argument or no views");
  if (!h->dVolC)
    return refuse(h->dPts ? "the model is a point model" : "model not uploaded");
  for (int i = 0; i < n && weights; i++)
    if (!std::isfinite(weights[i]))
      return refuse("view " + std::to_string(i) + ": weight not finite");
  if (grad_staging(h, std::max(1, h->scanCapG), 0) || vgrad_staging(h) || begin_analysis(h, false))
    return 1;
  const int N = h->N, OB = h->OB, pad = h->volPad;
  const size_t M = (size_t) h->M, PN = (size_t) pad * N, V = PN * PN * (PN / 2 + 1);
  for (int pass = 0; pass < 2; pass++) // every view's matrix first, then the insertion
  {
    if (pass)
      HIP_CHECK(h, hipMemsetAsync(h->dVolA, 0xff, sizeof(double2) * V, h->stream)); // (poisoned: the first launch starts from 0)
    for (int g0 = 0; g0 < n; g0 += OB)
    {
      const int nb = std::min(OB, n - g0);
      int bad, flag;
      HIP_CHECK(h, hipMemcpyAsync(h->dGradAngles, angles4 + 4 * (size_t) g0, sizeof(float4) * nb, hipMemcpyHostToDevice, h->stream));
      if (vgrad_views_checked(h, h->dGradAngles, isQuat, nb, bad, flag))
        return 1;
      if (bad >= 0)
        return refuse("view " + std::to_string(g0 + bad) + ": " + vgrad_flag_reason(flag));
      if (!pass)
        continue;
      HIP_CHECK(h, hipMemcpyAsync(h->dGradSpec, gamma + 2 * M * (size_t) g0, sizeof(double2) * M * nb, hipMemcpyHostToDevice,
                                  h->stream));
      if (weights)
        HIP_CHECK(h, hipMemcpyAsync(h->dGradW, weights + g0, sizeof(double) * nb, hipMemcpyHostToDevice, h->stream));
      HIP_CHECK(h, bioem_vgrad_prepare_launch(h->stream, h->dGradSpec, weights ? h->dGradW : nullptr, nb, N, h->dTwD, h->shiftX,
                                              h->shiftY, 0, h->dVgY));
      HIP_CHECK(h, bioem_vgrad_insert_launch(h->stream, h->dVgY, h->dVgR, h->dVgView, nb, N, pad, cull ? 1 : 0, g0 == 0,
                                             h->dVolA));
      HIP_CHECK(h, hipStreamSynchronize(h->stream)); // (the staging is reused by the next chunk)
    }
  }
  HIP_CHECK(h, hipMemcpy(spec_out, h->dVolA, sizeof(double2) * V, hipMemcpyDeviceToHost));
  return 0;
}

int bioem_hip_debug_volume_adjoint(bioem_hip_handle h, const double *spec_in, double *vol_out)
{
  if (!h)
    return 2;
  HIP_CHECK(h, hipSetDevice(h->device));
  const Refuse refuse = {h, "debug_volume_adjoint"};
  if (!spec_in || !vol_out)
    return refuse("null argument");
  if (!h->dVolC)
    return refuse(h->dPts ? "the model is a point model" : "model not uploaded");
  if (grad_staging(h, std::max(1, h->scanCapG), 0) || vgrad_staging(h) || begin_analysis(h, false))
    return 1;
  const size_t PN = (size_t) h->volPad * h->N, V = PN * PN * (PN / 2 + 1);
  HIP_CHECK(h, hipMemcpy(h->dVolA, spec_in, sizeof(double2) * V, hipMemcpyHostToDevice));
  return vgrad_adjoint(h, "debug_volume_adjoint", h->dVolA, vol_out);
}

// ---- the gradient with respect to the orientation matrix and the model shifts of a volume model (pose_kernels.hpp) ----
} // extern "C" (closed around the helper of the pose gradient)

namespace
{
// the staging of the pose entries beside that of the volume gradient (without A); a failed allocation (return 1) leaves
// the handle as it was
int pose_staging(bioem_hip_ctx *h)
{
  if (vgrad_staging(h, false))
    return 1;
  if (h->dPosePart)
    return 0;
  const size_t OB = (size_t) h->OB, cap = (size_t) scan_capacity(h);
  Staging st = {h};
  st.get(h->dPosePart, OB * (size_t) bioem_pose_patches(h->N) * kPoseSums);
  st.get(h->dPoseRows, (size_t) kPoseRow * cap);
  return st.commit();
}
} // namespace

extern "C" {

int bioem_hip_pose_gradient(bioem_hip_handle h, const bioem_hip_grad_request *req, int n, int ownLists, double *pose_out,
                            double *coef_out, bioem_hip_param5 *params_out)
{
  if (!h)
    return 2;
  HIP_CHECK(h, hipSetDevice(h->device));
  const Refuse refuse = {h, "pose_gradient"};
  if (!req || n < 1)
    return refuse("null argument or no requests");
  if (!pose_out)
    return refuse("pose_out null");
  if (const char *why = missing_state(h, NEED_ALL, ownLists))
    return refuse(why);
  if (!h->dVolC)
    return refuse("the model is a point model");
  const int N = h->N, OB = h->OB, G = h->nCTF, pad = h->volPad;
  const int cap = scan_capacity(h); // records one launch of the scan serves: whole batches
  GradRequests q;
  if (const int rc = grad_requests(h, refuse, req, nullptr, n, ownLists, q))
    return rc;
  if (grad_staging(h, G, 0) || pose_staging(h) || begin_analysis(h, true))
    return 1;
  const OrientList src = ownLists ? own_list(h) : shared_list(h);
  const size_t M = (size_t) h->M;
  // every request's matrix is looked at before anything runs
  std::vector<double> mats(9 * (size_t) std::min(cap, n));
  for (int g0 = 0; g0 < n; g0 += cap)
  {
    const int ng = std::min(cap, n - g0);
    HIP_CHECK(h, hipMemcpyAsync(h->dScanRec, q.recs.data() + g0, sizeof(BioemWindowRecord) * ng, hipMemcpyHostToDevice, h->stream));
    if (gather_matches(h, src, h->dScanRec, ng, h->dGradAngles))
      return 1;
    HIP_CHECK(h, bioem_recon_matrices_launch(h->stream, h->dGradAngles, nullptr, src.isQuat ? 1 : 0, ng, h->dVgR));
    HIP_CHECK(h, hipMemcpyAsync(mats.data(), h->dVgR, sizeof(double) * 9 * ng, hipMemcpyDeviceToHost, h->stream));
    HIP_CHECK(h, hipStreamSynchronize(h->stream));
    for (int i = 0; i < 9 * ng; i++)
      if (!std::isfinite(mats[(size_t) i]))
      {
        const int bad = g0 + i / 9;
        int first, len;
        orient_span(h, ownLists, req[bad].particle, first, len);
        return refuse(request_refusal(h, bad, "an entry of the orientation's matrix is not finite", req[bad],
                                      REQ_CONV | REQ_SHIFT, len));
      }
  }
  for (int g0 = 0; g0 < n; g0 += cap) // the requests one launch of the scan serves
  {
    const int ng = std::min(cap, n - g0);
    if (grad_front(h, src, q, g0, ng))
      return 1;
    HIP_CHECK(h, bioem_recon_matrices_launch(h->stream, h->dGradAngles, nullptr, src.isQuat ? 1 : 0, ng, h->dVgR));
    for (int b0 = 0; b0 < ng; b0 += OB)
    {
      const int nb = std::min(OB, ng - b0), r0 = g0 + b0;
      // phase 2: the gradient spectrum and Y; phase 3: the nine sums
      if (phase_begin(h, h->stream, BIOEM_HIP_PHASE_COMPARISON, r0, r0 + nb, 0, 0))
        return 1;
      HIP_CHECK(h, bioem_grad_spectrum_launch(h->stream, h->dScanPw + M * (size_t) b0, h->dScanZ + M * (size_t) b0, h->dCTF,
                                              h->dGradRec + b0, h->dGradCoef + 4 * (size_t) b0, 0, nb, N, h->dGradSpec));
      HIP_CHECK(h, bioem_vgrad_prepare_launch(h->stream, h->dGradSpec, nullptr, nb, N, h->dTwD, h->shiftX, h->shiftY, 1, h->dVgY));
      if (phase_end(h, h->stream) || phase_begin(h, h->stream, 3, r0, r0 + nb, 0, 0))
        return 1;
      HIP_CHECK(h, bioem_pose_launch(h->stream, h->dVolC, pad, h->dVgR + 9 * (size_t) b0, h->dVgY, nb, N, h->dPosePart,
                                     h->dPoseRows + (size_t) kPoseRow * b0));
      if (phase_end(h, h->stream))
        return 1;
    }
    HIP_CHECK(h, hipMemcpyAsync(pose_out + (size_t) kPoseRow * g0, h->dPoseRows, sizeof(double) * kPoseRow * ng,
                                hipMemcpyDeviceToHost, h->stream));
    if (params_out)
      HIP_CHECK(h, hipMemcpyAsync(params_out + g0, h->dGradParams, sizeof(bioem_hip_param5) * ng, hipMemcpyDeviceToHost, h->stream));
    if (coef_out)
      HIP_CHECK(h, hipMemcpyAsync(coef_out + 4 * (size_t) g0, h->dGradCoef, sizeof(double) * 4 * ng, hipMemcpyDeviceToHost, h->stream));
    HIP_CHECK(h, hipStreamSynchronize(h->stream));
    if (coef_out)
      for (int i = 0; i < ng; i++) // (the fourth slot of the device's coefficients is not written by this entry)
        coef_out[4 * (size_t) (g0 + i) + 3] = pose_out[(size_t) kPoseRow * (g0 + i) + 8];
  }
  drain_phases(h);
  return 0;
}

int bioem_hip_debug_pose_sums(bioem_hip_handle h, const float *angles4, int n, int isQuat, const double *gamma,
                              const double *weights, double *pose_out)
{
  if (!h)
    return 2;
  HIP_CHECK(h, hipSetDevice(h->device));
  const Refuse refuse = {h, "debug_pose_sums"};
  if (!angles4 || !gamma || !pose_out || n < 1)
    return refuse("null argument or no views");
  if (!h->dVolC)
    return refuse(h->dPts ? "the model is a point model" : "model not uploaded");
  for (int i = 0; i < n && weights; i++)
    if (!std::isfinite(weights[i]))
      return refuse("view " + std::to_string(i) + ": weight not finite");
  if (grad_staging(h, std::max(1, h->scanCapG), 0) || pose_staging(h) || begin_analysis(h, false))
    return 1;
  const int N = h->N, OB = h->OB;
  const size_t M = (size_t) h->M;
  for (int g0 = 0; g0 < n; g0 += OB)
  {
    const int nb = std::min(OB, n - g0);
    HIP_CHECK(h, hipMemcpyAsync(h->dGradAngles, angles4 + 4 * (size_t) g0, sizeof(float4) * nb, hipMemcpyHostToDevice, h->stream));
    HIP_CHECK(h, hipMemcpyAsync(h->dGradSpec, gamma + 2 * M * (size_t) g0, sizeof(double2) * M * nb, hipMemcpyHostToDevice,
                                h->stream));
    if (weights)
      HIP_CHECK(h, hipMemcpyAsync(h->dGradW, weights + g0, sizeof(double) * nb, hipMemcpyHostToDevice, h->stream));
    HIP_CHECK(h, bioem_recon_matrices_launch(h->stream, h->dGradAngles, nullptr, isQuat ? 1 : 0, nb, h->dVgR));
    HIP_CHECK(h, bioem_vgrad_prepare_launch(h->stream, h->dGradSpec, weights ? h->dGradW : nullptr, nb, N, h->dTwD, h->shiftX,
                                            h->shiftY, 0, h->dVgY));
    // (poisoned: a sum the kernels leave unwritten reads back as a NaN)
    HIP_CHECK(h, hipMemsetAsync(h->dPoseRows, 0xff, sizeof(double) * kPoseRow * nb, h->stream));
    HIP_CHECK(h, bioem_pose_launch(h->stream, h->dVolC, h->volPad, h->dVgR, h->dVgY, nb, N, h->dPosePart, h->dPoseRows));
    HIP_CHECK(h, hipMemcpyAsync(pose_out + (size_t) kPoseRow * g0, h->dPoseRows, sizeof(double) * kPoseRow * nb,
                                hipMemcpyDeviceToHost, h->stream));
    HIP_CHECK(h, hipStreamSynchronize(h->stream)); // (the staging is reused by the next chunk)
  }
  return 0;
}

// ---- gradient and curvature of the log posterior with respect to the CTF triple of a request (ctfgrad_kernels.hpp) ----
} // extern "C" (closed around the helpers of the CTF gradient)

namespace
{
// The host's row map and its table of the radial variable (ctf_kernel_one of the host layer, CTF mode).  The map is what
// replaying the host's loop leaves behind (index i < H is written to rows i and N - 1 - i, the last write wins); the table
// holds, per m = i^2 + j^2, the float of the host's own expression, formed here with the same float operations.
void ctfgrad_tables(int N, float pixelSize, std::vector<int> &rowIdx, std::vector<float> &radsq)
{
  const int H = N / 2 + 1;
  rowIdx.assign((size_t) N, 0);
  for (int i = 0; i < H; i++)
  {
    rowIdx[(size_t) i] = i;
    rowIdx[(size_t) (N - 1 - i)] = i;
  }
  radsq.assign(2 * (size_t) (H - 1) * (H - 1) + 1, 0.f);
  for (int i = 0; i < H; i++)
    for (int j = 0; j < H; j++)
      radsq[(size_t) (i * i + j * j)] = (float) (i * i + j * j) / N / N / pixelSize / pixelSize;
}

// the staging of the CTF gradient entries beside that of the gradient entries, and the tables for pixelSize (uploaded once
// per handle and pixel size); a failed allocation (return 1) leaves the handle as it was
int ctfgrad_staging(bioem_hip_ctx *h, float pixelSize, bool derivs)
{
  const size_t OB = (size_t) h->OB, cap = (size_t) scan_capacity(h), Hm = (size_t) h->H - 1;
  if (!h->dCtfgPart)
  {
    Staging st = {h};
    st.get(h->dCtfgPart, OB * (size_t) bioem_ctfgrad_blocks(h->N) * kCtfgSums);
    st.get(h->dCtfgSums, cap * kCtfgSums);
    st.get(h->dCtfgRows, cap * kCtfgRow);
    st.get(h->dCtfgTheta, 3 * OB);
    st.get(h->dCtfgRowIdx, (size_t) h->N);
    st.get(h->dCtfgRadsq, 2 * Hm * Hm + 1);
    if (st.commit())
      return 1;
    h->ctfgPixel = 0.f;
  }
  if (derivs && !h->dCtfgDerivs)
  {
    Staging st = {h};
    st.get(h->dCtfgDerivs, OB * (size_t) h->M * kCtfgDerivs);
    if (st.commit())
      return 1;
  }
  if (h->ctfgPixel != pixelSize)
  {
    std::vector<int> rowIdx;
    std::vector<float> radsq;
    ctfgrad_tables(h->N, pixelSize, rowIdx, radsq);
    HIP_CHECK(h, hipMemcpyAsync(h->dCtfgRowIdx, rowIdx.data(), sizeof(int) * rowIdx.size(), hipMemcpyHostToDevice, h->stream));
    HIP_CHECK(h, hipMemcpyAsync(h->dCtfgRadsq, radsq.data(), sizeof(float) * radsq.size(), hipMemcpyHostToDevice, h->stream));
    HIP_CHECK(h, hipStreamSynchronize(h->stream)); // (the vectors are read by then)
    h->ctfgPixel = pixelSize;
  }
  return 0;
}

// what the entries refuse about the handle and the pixel size; nullptr: nothing
const char *ctfgrad_refused(const bioem_hip_ctx *h, float pixelSize)
{
  if (h->pd.tousepsf)
    return "the handle is in PSF mode: its kernels are transforms of a real-space function, not the closed form";
  if (!(std::isfinite(pixelSize) && pixelSize > 0.f))
    return "pixelSize not finite or not positive";
  return nullptr;
}

// rho = sqrt(1 - amp^2) / amp is singular at both ends (and the host refuses amp < 1e-10)
bool ctfgrad_amp_outside(float amp) { return !((double) amp > 1e-10 && amp < 1.f); }
} // namespace

extern "C" {

int bioem_hip_ctf_gradient(bioem_hip_handle h, const bioem_hip_grad_request *req, int n, int ownLists, float pixelSize,
                           double *rows_out, double *coef_out, bioem_hip_param5 *params_out)
{
  if (!h)
    return 2;
  HIP_CHECK(h, hipSetDevice(h->device));
  const Refuse refuse = {h, "ctf_gradient"};
  if (!req || n < 1)
    return refuse("null argument or no requests");
  if (!rows_out)
    return refuse("rows_out null");
  if (const char *why = ctfgrad_refused(h, pixelSize))
    return refuse(why);
  if (const char *why = missing_state(h, NEED_ALL, ownLists))
    return refuse(why);
  const int N = h->N, OB = h->OB, G = h->nCTF;
  const int cap = scan_capacity(h); // records one launch of the scan serves: whole batches
  GradRequests q;
  if (const int rc = grad_requests(h, refuse, req, nullptr, n, ownLists, q))
    return rc;
  // every request's amplitude is looked at before anything runs
  std::vector<float> theta(3 * (size_t) G);
  HIP_CHECK(h, hipMemcpy(theta.data(), h->dCtfParam, sizeof(float) * theta.size(), hipMemcpyDeviceToHost));
  for (int i = 0; i < n; i++)
    if (ctfgrad_amp_outside(theta[3 * (size_t) req[i].conv]))
    {
      int first, len;
      orient_span(h, ownLists, req[i].particle, first, len);
      return refuse(request_refusal(h, i, "amp of the CTF set outside (1e-10, 1)", req[i], REQ_CONV | REQ_SHIFT, len));
    }
  if (grad_staging(h, G, 0) || ctfgrad_staging(h, pixelSize, false) || begin_analysis(h, true))
    return 1;
  const OrientList src = ownLists ? own_list(h) : shared_list(h);
  const size_t M = (size_t) h->M;
  for (int g0 = 0; g0 < n; g0 += cap) // the requests one launch of the scan serves
  {
    const int ng = std::min(cap, n - g0);
    if (grad_front(h, src, q, g0, ng))
      return 1;
    for (int b0 = 0; b0 < ng; b0 += OB)
    {
      const int nb = std::min(OB, ng - b0), r0 = g0 + b0;
      // phase 2: the twenty sums; phase 3: the rows
      if (phase_begin(h, h->stream, BIOEM_HIP_PHASE_COMPARISON, r0, r0 + nb, 0, 0))
        return 1;
      HIP_CHECK(h, bioem_ctfgrad_sums_launch(h->stream, h->dScanPw + M * (size_t) b0, h->dScanZ + M * (size_t) b0, h->dGradRec + b0,
                                             h->dCtfParam, h->dCtfgRowIdx, h->dCtfgRadsq, nb, N, h->dCtfgPart,
                                             h->dCtfgSums + (size_t) kCtfgSums * b0, nullptr));
      if (phase_end(h, h->stream) || phase_begin(h, h->stream, 3, r0, r0 + nb, 0, 0))
        return 1;
      HIP_CHECK(h, bioem_ctfgrad_finish_launch(h->stream, h->dCtfgSums + (size_t) kCtfgSums * b0, h->dGradRec + b0, h->dScanCc,
                                               h->dScanParams, h->dSumRef, h->dSumsqRef, h->dGradCoef + 4 * (size_t) b0, h->pd,
                                               nb, N, h->dCtfgRows + (size_t) kCtfgRow * b0));
      if (phase_end(h, h->stream))
        return 1;
    }
    HIP_CHECK(h, hipMemcpyAsync(rows_out + (size_t) kCtfgRow * g0, h->dCtfgRows, sizeof(double) * kCtfgRow * ng,
                                hipMemcpyDeviceToHost, h->stream));
    if (params_out)
      HIP_CHECK(h, hipMemcpyAsync(params_out + g0, h->dGradParams, sizeof(bioem_hip_param5) * ng, hipMemcpyDeviceToHost, h->stream));
    if (coef_out)
      HIP_CHECK(h, hipMemcpyAsync(coef_out + 4 * (size_t) g0, h->dGradCoef, sizeof(double) * 4 * ng, hipMemcpyDeviceToHost, h->stream));
    HIP_CHECK(h, hipStreamSynchronize(h->stream));
    if (coef_out)
      for (int i = 0; i < ng; i++) // (the fourth slot of the device's coefficients is not written by this entry)
        coef_out[4 * (size_t) (g0 + i) + 3] = 0.;
  }
  drain_phases(h);
  return 0;
}

int bioem_hip_debug_ctf_gradient(bioem_hip_handle h, const float *specP, const float *specRef, const int *shiftXY,
                                 const float *triples, int n, float pixelSize, double *rows_out, double *derivs_out)
{
  if (!h)
    return 2;
  HIP_CHECK(h, hipSetDevice(h->device));
  const Refuse refuse = {h, "debug_ctf_gradient"};
  if (!specP || !specRef || !shiftXY || !triples || n < 1)
    return refuse("null argument or no records");
  if (!rows_out)
    return refuse("rows_out null");
  if (const char *why = ctfgrad_refused(h, pixelSize))
    return refuse(why);
  if (const int rc = debug_shifts_refused(h, refuse, shiftXY, n))
    return rc;
  for (int i = 0; i < n; i++)
    if (ctfgrad_amp_outside(triples[3 * (size_t) i]))
      return refuse("record " + std::to_string(i) + ": amp outside (1e-10, 1)");
  if (grad_staging(h, std::max(1, h->scanCapG), 0) || ctfgrad_staging(h, pixelSize, derivs_out != nullptr) ||
      begin_analysis(h, false)) // (buffer set 0 is not written)
    return 1;
  const int N = h->N, H = h->H, OB = h->OB;
  const size_t M = (size_t) h->M;
  const double Nt = (double) N * (double) N;
  std::vector<BioemGradRecord> grecs((size_t) OB);
  for (int i = 0; i < OB; i++)
    grecs[(size_t) i] = {i, i, i, 0};
  HIP_CHECK(h, hipMemcpyAsync(h->dGradRec, grecs.data(), sizeof(BioemGradRecord) * OB, hipMemcpyHostToDevice, h->stream));
  std::vector<double> sums((size_t) kCtfgSums * OB);
  std::vector<bioem_hip_param5> par((size_t) OB);
  std::vector<float> lin(3 * (size_t) OB); // cc, sumRef, sumsqRef of the batch
  for (int b0 = 0; b0 < n; b0 += OB)
  {
    const int nb = std::min(OB, n - b0);
    HIP_CHECK(h, hipMemcpyAsync(h->dScanShift, shiftXY + 2 * (size_t) b0, sizeof(BioemScanShift) * nb, hipMemcpyHostToDevice, h->stream));
    HIP_CHECK(h, hipMemcpyAsync(h->dWinConv, specP + 2 * M * (size_t) b0, sizeof(float2) * M * nb, hipMemcpyHostToDevice, h->stream));
    HIP_CHECK(h, hipMemcpyAsync(h->dWinRef, specRef + 2 * M * (size_t) b0, sizeof(float2) * M * nb, hipMemcpyHostToDevice, h->stream));
    HIP_CHECK(h, hipMemcpyAsync(h->dCtfgTheta, triples + 3 * (size_t) b0, sizeof(float) * 3 * nb, hipMemcpyHostToDevice, h->stream));
    HIP_CHECK(h, bioem_scan_prep_launch(h->stream, h->dWinConv, h->dWinRef, h->dScanShift, nb, N, h->dTwD, h->dScanPw, h->dScanZ));
    // (poisoned: a sum or an entry of a row the kernels leave unwritten reads back as a NaN)
    HIP_CHECK(h, hipMemsetAsync(h->dCtfgSums, 0xff, sizeof(double) * kCtfgSums * nb, h->stream));
    HIP_CHECK(h, hipMemsetAsync(h->dCtfgRows, 0xff, sizeof(double) * kCtfgRow * nb, h->stream));
    HIP_CHECK(h, bioem_ctfgrad_sums_launch(h->stream, h->dScanPw, h->dScanZ, h->dGradRec, h->dCtfgTheta, h->dCtfgRowIdx,
                                           h->dCtfgRadsq, nb, N, h->dCtfgPart, h->dCtfgSums, derivs_out ? h->dCtfgDerivs : nullptr));
    HIP_CHECK(h, hipMemcpyAsync(sums.data(), h->dCtfgSums, sizeof(double) * kCtfgSums * nb, hipMemcpyDeviceToHost, h->stream));
    if (derivs_out)
      HIP_CHECK(h, hipMemcpyAsync(derivs_out + (size_t) kCtfgDerivs * M * b0, h->dCtfgDerivs, sizeof(double) * kCtfgDerivs * M * nb,
                                  hipMemcpyDeviceToHost, h->stream));
    HIP_CHECK(h, hipStreamSynchronize(h->stream));
    // the linearisation point the spectra imply: sumC the projection's origin (k(0) = 1), sumsquareC and cc the sums ss0
    // and cc0 over Nt narrowed to float, the particle's sum its origin and its sum of squares by Parseval's identity
    for (int i = 0; i < nb; i++)
    {
      const float *P = specP + 2 * M * (size_t) (b0 + i), *F = specRef + 2 * M * (size_t) (b0 + i);
      double ssr = 0.;
      for (int e = 0; e < N * H; e++)
      {
        const int j = e % H;
        const double fr = (double) F[2 * e], fi = (double) F[2 * e + 1];
        ssr += ((j == 0 || 2 * j == N) ? 1. : 2.) * (fr * fr + fi * fi);
      }
      const float *t3 = triples + 3 * (size_t) (b0 + i);
      par[(size_t) i] = {t3[0], t3[1], t3[2], P[0], (float) (sums[(size_t) kCtfgSums * i] / Nt)};
      lin[(size_t) i] = (float) (sums[(size_t) kCtfgSums * i + 1] / Nt);
      lin[(size_t) OB + i] = F[0];
      lin[2 * (size_t) OB + i] = (float) (ssr / Nt);
    }
    HIP_CHECK(h, hipMemcpyAsync(h->dGradParams, par.data(), sizeof(bioem_hip_param5) * nb, hipMemcpyHostToDevice, h->stream));
    HIP_CHECK(h, hipMemcpyAsync(h->dScanCc, lin.data(), sizeof(float) * nb, hipMemcpyHostToDevice, h->stream));
    HIP_CHECK(h, hipMemcpyAsync(h->dScanSums, lin.data() + OB, sizeof(float) * 2 * OB, hipMemcpyHostToDevice, h->stream));
    HIP_CHECK(h, bioem_grad_coef_launch(h->stream, h->dGradRec, h->dScanCc, h->dGradParams, h->dScanSums, h->dScanSums + OB, nb,
                                        N, h->dGradCoef, nullptr));
    HIP_CHECK(h, bioem_ctfgrad_finish_launch(h->stream, h->dCtfgSums, h->dGradRec, h->dScanCc, h->dGradParams, h->dScanSums,
                                             h->dScanSums + OB, h->dGradCoef, h->pd, nb, N, h->dCtfgRows));
    HIP_CHECK(h, hipMemcpyAsync(rows_out + (size_t) kCtfgRow * b0, h->dCtfgRows, sizeof(double) * kCtfgRow * nb,
                                hipMemcpyDeviceToHost, h->stream));
    HIP_CHECK(h, hipStreamSynchronize(h->stream)); // (the staging is reused by the next chunk)
  }
  return 0;
}

int bioem_hip_debug_projection(bioem_hip_handle h, int iOrient, float *spec_out)
{
  HIP_CHECK(h, hipSetDevice(h->device));
  bioem_hip_ctx::Slot &s0 = h->slot[0];
  void_slot(s0);
  if (project_batch(h, s0, h->stream, shared_list(h), iOrient, 1))
    return 1;
  HIP_CHECK(h, hipMemcpyAsync(spec_out, s0.specRef, sizeof(float2) * (size_t) h->M, hipMemcpyDeviceToHost, h->stream));
  HIP_CHECK(h, hipStreamSynchronize(h->stream));
  return 0;
}

int bioem_hip_debug_projection_maps(bioem_hip_handle h, int o0, int nO, int path, double *maps_out, double *tempden_out,
                                    float *spec_out, int *info_out)
{
  if (!h)
    return 2;
  HIP_CHECK(h, hipSetDevice(h->device));
  auto refuse = [&](const std::string &why) {
    h->err = "debug_projection_maps: " + why;
    return 2;
  };
  if (!maps_out || !tempden_out || !info_out)
    return refuse("null argument");
  if (h->dVolC)
    return refuse("the model is a volume");
  if (!h->dPts || h->nAnglesUp < 1)
    return refuse("model or orientations not uploaded");
  if (path < kProjectAuto || path > kProjectAtomics)
    return refuse("path must be 0 (as a run), 1 (box), 2 (bands) or 3 (global atomics)");
  if (nO < 1 || nO > h->OB)
    return refuse("between 1 and maxOrientations (" + std::to_string(h->OB) + ") orientations per call");
  if (o0 < 0 || o0 > h->nAnglesUp - nO)
    return refuse("orientations outside the uploaded list");
  bioem_hip_ctx::Slot &s0 = h->slot[0];
  void_slot(s0);
  ProjectPlan P;
  const int rc = project_batch(h, s0, h->stream, shared_list(h), o0, nO, path, &P);
  if (rc == 2)
    return refuse(h->err);
  if (rc)
    return rc;
  const int N = h->N;
  const size_t NN = (size_t) N * N;
  HIP_CHECK(h, hipMemcpyAsync(tempden_out, s0.tempDen, sizeof(double) * (size_t) nO, hipMemcpyDeviceToHost, h->stream));
  if (spec_out)
    HIP_CHECK(h, hipMemcpyAsync(spec_out, s0.specRef, sizeof(float2) * (size_t) h->M * nO, hipMemcpyDeviceToHost, h->stream));
  if (P.compact)
  { // [nO][side][side] on the device: the box goes into place, zeros around it
    const size_t side = (size_t) P.boxSide;
    std::vector<double> box(side * side * nO);
    HIP_CHECK(h, hipMemcpyAsync(box.data(), s0.projReal, sizeof(double) * box.size(), hipMemcpyDeviceToHost, h->stream));
    HIP_CHECK(h, hipStreamSynchronize(h->stream));
    std::fill(maps_out, maps_out + NN * nO, 0.);
    for (int b = 0; b < nO; b++)
      for (size_t r = 0; r < side; r++)
        std::copy(box.begin() + (b * side + r) * side, box.begin() + (b * side + r + 1) * side,
                  maps_out + b * NN + (P.boxLo + r) * N + P.boxLo);
  }
  else
  {
    HIP_CHECK(h, hipMemcpyAsync(maps_out, s0.projReal, sizeof(double) * NN * nO, hipMemcpyDeviceToHost, h->stream));
    HIP_CHECK(h, hipStreamSynchronize(h->stream));
  }
  const int info[6] = {P.path, P.boxLo, P.boxSide, P.compact, P.TR, h->iradMax};
  std::copy(info, info + 6, info_out);
  return 0;
}

int bioem_hip_debug_stamps(bioem_hip_handle h, double *stamps_out, int *iradMax_out)
{
  if (!h)
    return 2;
  HIP_CHECK(h, hipSetDevice(h->device));
  if (h->dVolC)
  {
    h->err = "debug_stamps: the model is a volume";
    return 2;
  }
  if (!iradMax_out || !h->dStamp)
  {
    h->err = !h->dStamp ? "debug_stamps: the model has no footprint table" : "debug_stamps: null argument";
    return 2;
  }
  const size_t S = 2 * (size_t) h->iradMax + 1;
  *iradMax_out = h->iradMax;
  if (stamps_out) // (null: the caller asks for iradMax to size the table)
    HIP_CHECK(h, hipMemcpy(stamps_out, h->dStamp, sizeof(double) * (size_t) h->nPts * S * S, hipMemcpyDeviceToHost));
  return 0;
}

int bioem_hip_debug_convolution(bioem_hip_handle h, int iOrient, int iConv, float *spec_out, float *sumC,
                                float *sumsquareC)
{
  HIP_CHECK(h, hipSetDevice(h->device));
  bioem_hip_ctx::Slot &s0 = h->slot[0];
  void_slot(s0);
  if (project_batch(h, s0, h->stream, shared_list(h), iOrient, 1))
    return 1;
  if (convolve_batch(h, s0, h->stream, 1, 0, h->nCTF))
    return 1;
  const size_t M = (size_t) h->M;
  float2 *tmp = s0.specRef + M; // chunkB >= 32 images; the first holds the projection spectrum
  hipLaunchKernelGGL(k_unreorder, dim3(256), dim3(256), 0, h->stream, s0.conv + h->Mc * (size_t) iConv, tmp, 1, h->N,
                     h->H, h->plan.halfR, h->plan.N1, h->Hp);
  HIP_CHECK(h, hipGetLastError());
  HIP_CHECK(h, hipMemcpyAsync(spec_out, tmp, sizeof(float2) * M, hipMemcpyDeviceToHost, h->stream));
  bioem_hip_param5 q;
  HIP_CHECK(h, hipMemcpyAsync(&q, s0.params + iConv, sizeof(q), hipMemcpyDeviceToHost, h->stream));
  HIP_CHECK(h, hipStreamSynchronize(h->stream));
  *sumC = q.sumC;
  *sumsquareC = q.sumsquareC;
  return 0;
}

int bioem_hip_debug_convolve_batch(bioem_hip_handle h, const float *specP, int nO, int c0, int nC, float *conv_out,
                                   bioem_hip_param5 *params_out, float *raw_out, int *info_out)
{
  if (!h)
    return 2;
  HIP_CHECK(h, hipSetDevice(h->device));
  const Refuse refuse = {h, "debug_convolve_batch"};
  if (!specP || !conv_out || !params_out || !info_out)
    return refuse("null argument");
  if (const char *why = missing_state(h, NEED_CTF, 0))
    return refuse(why);
  if (nO < 1 || nO > h->OB)
    return refuse("between 1 and maxOrientations (" + std::to_string(h->OB) + ") orientations per call");
  if (c0 < 0 || nC < 1 || c0 > h->nCTF - nC)
    return refuse("CTF range empty or outside [0, nCTF)");
  const size_t rows = (size_t) nO * nC; // (at most maxOrientations x nCTF)
  if (rows + 1 > h->slotRows)
    return refuse("the conv rows of a batch (" + std::to_string(h->slotRows) + ") do not hold " + std::to_string(rows) +
                  " rows and a guard row");
  bioem_hip_ctx::Slot &s0 = h->slot[0];
  const bool fused = convolve_fused(h, false);
  if (!fused && (!s0.scratch || rows > (size_t) ((h->maxOC + 31) & ~31)))
    return refuse("the two-kernel path is selected and the batch has no buffer for the ordered sums of " +
                  std::to_string(rows) + " rows");
  if (begin_analysis(h, true))
    return 1;
  const size_t M = (size_t) h->M;
  OrientDebugBufs B;
  float2 *tmp = nullptr; // the rows and the guard row in reference layout
  HIP_CHECK(h, B.get(&tmp, nullptr, sizeof(float2) * M * (rows + 1)));
  HIP_CHECK(h, hipMemcpyAsync(s0.specRef, specP, sizeof(float2) * M * nO, hipMemcpyHostToDevice, h->stream));
  HIP_CHECK(h, hipMemsetAsync(s0.conv, 0xFF, sizeof(float2) * h->Mc * (rows + 1), h->stream));
  HIP_CHECK(h, hipMemsetAsync(s0.params, 0xFF, sizeof(bioem_hip_param5) * (rows + 1), h->stream));
  if (convolve_batch(h, s0, h->stream, nO, c0, nC))
    return 1;
  hipLaunchKernelGGL(k_unreorder, dim3((unsigned) std::min<size_t>(1024, 16 * (rows + 1))), dim3(256), 0, h->stream, s0.conv,
                     tmp, (int) (rows + 1), h->N, h->H, h->plan.halfR, h->plan.N1, h->Hp);
  HIP_CHECK(h, hipGetLastError());
  HIP_CHECK(h, hipMemcpyAsync(conv_out, tmp, sizeof(float2) * M * (rows + 1), hipMemcpyDeviceToHost, h->stream));
  HIP_CHECK(h, hipMemcpyAsync(params_out, s0.params, sizeof(bioem_hip_param5) * (rows + 1), hipMemcpyDeviceToHost, h->stream));
  if (raw_out)
    HIP_CHECK(h, hipMemcpyAsync(raw_out, s0.conv, sizeof(float2) * h->Mc * rows, hipMemcpyDeviceToHost, h->stream));
  HIP_CHECK(h, hipStreamSynchronize(h->stream));
  const int info[6] = {fused ? 1 : 0, h->plan.halfR, h->plan.N1, h->Hp, (int) rows, 1};
  std::copy(info, info + 6, info_out);
  return 0;
}

int bioem_hip_debug_direct_conv(bioem_hip_handle h, const float *specConv, int nRows, double *Z_out, float *real_out)
{
  if (!h)
    return 2;
  HIP_CHECK(h, hipSetDevice(h->device));
  const Refuse refuse = {h, "debug_direct_conv"};
  if (!h->direct)
    return refuse("the handle was not created under BIOEM_CC_DIRECT");
  if (!specConv || !real_out)
    return refuse("null argument");
  if (nRows < 1 || nRows > h->maxOC)
    return refuse("between 1 and the " + std::to_string(h->maxOC) + " conv rows of a batch per call");
  if (begin_analysis(h, true))
    return 1;
  const size_t M = (size_t) h->M, NN = (size_t) h->N * h->N;
  bioem_hip_ctx::Slot &s0 = h->slot[0];
  OrientDebugBufs B;
  float2 *stage = nullptr; // the rows in reference layout, as the staging ring of bioem_hip_compare holds them
  HIP_CHECK(h, B.get(&stage, specConv, sizeof(float2) * M * nRows));
  hipLaunchKernelGGL(k_reorder, dim3(std::min(2048, 8 * nRows)), dim3(256), 0, h->stream, stage, s0.conv, nRows, h->N, h->H,
                     h->plan.halfR, h->plan.N1, h->Hp);
  // the two launches of launch_compare_fold
  hipLaunchKernelGGL(k_c2r_cols, dim3(h->H, nRows), dim3(128), sizeof(double2) * h->N, h->stream, s0.conv, h->N, h->H,
                     h->plan.halfR, h->plan.N1, h->dTwD, h->dDirectZ);
  hipLaunchKernelGGL(k_c2r_rows, dim3(h->N, nRows), dim3(128), sizeof(double2) * h->H, h->stream, h->dDirectZ, h->N,
                     h->H, h->dTwD, h->dConvReal);
  HIP_CHECK(h, hipGetLastError());
  if (Z_out)
    HIP_CHECK(h, hipMemcpyAsync(Z_out, h->dDirectZ, sizeof(double2) * M * nRows, hipMemcpyDeviceToHost, h->stream));
  HIP_CHECK(h, hipMemcpyAsync(real_out, h->dConvReal, sizeof(float) * NN * nRows, hipMemcpyDeviceToHost, h->stream));
  HIP_CHECK(h, hipStreamSynchronize(h->stream));
  return 0;
}

int bioem_hip_debug_particles(bioem_hip_handle h, float *refFFT_out, float *sum_out, float *sumsq_out)
{
  HIP_CHECK(h, hipSetDevice(h->device));
  const size_t M = (size_t) h->M;
  bioem_hip_ctx::Slot &s0 = h->slot[0];
  void_slot(s0);
  for (int b = 0; refFFT_out && b < h->nMaps; b += h->chunkB)
  {
    const int n = std::min(h->chunkB, h->nMaps - b);
    hipLaunchKernelGGL(k_unreorder, dim3(1024), dim3(256), 0, h->stream, h->dRef + h->Mc * (size_t) b, s0.specRef, n, h->N,
                       h->H, h->plan.halfR, h->plan.N1, h->Hp);
    HIP_CHECK(h, hipGetLastError());
    HIP_CHECK(h, hipMemcpyAsync(refFFT_out + 2 * M * (size_t) b, s0.specRef, sizeof(float2) * M * n,
                                hipMemcpyDeviceToHost, h->stream));
    HIP_CHECK(h, hipStreamSynchronize(h->stream));
  }
  HIP_CHECK(h, hipMemcpy(sum_out, h->dSumRef, sizeof(float) * h->nMaps, hipMemcpyDeviceToHost));
  HIP_CHECK(h, hipMemcpy(sumsq_out, h->dSumsqRef, sizeof(float) * h->nMaps, hipMemcpyDeviceToHost));
  return 0;
}

int bioem_hip_kernel_stats(bioem_hip_handle h, double *compare_ms, long long *launches, long long *comparisons)
{
  HIP_CHECK(h, hipSetDevice(h->device));
  if (compat_flush(h))
    return 1;
  HIP_CHECK(h, hipStreamSynchronize(h->stream));
  drain_events(h);
  if (compare_ms)
    *compare_ms = h->compareMs;
  if (launches)
    *launches = h->launches;
  if (comparisons)
    *comparisons = h->comparisons;
  return 0;
}

int bioem_hip_reset_kernel_stats(bioem_hip_handle h)
{
  HIP_CHECK(h, hipSetDevice(h->device));
  HIP_CHECK(h, hipStreamSynchronize(h->stream));
  drain_events(h);
  h->compareMs = 0;
  h->launches = 0;
  h->comparisons = 0;
  return 0;
}

int bioem_hip_uses_fast_path(bioem_hip_handle h)
{ // the families with a register FFT
  const int f = h ? h->plan.family : KF_GENERIC;
  return f == KF_FAST || f == KF_FASTM || f == KF_FASTM2 || f == KF_WIDE2 ? 1 : 0;
}

int bioem_hip_plan(int numberPixels, int maxDisplaceCenter, int gridSpaceCenter, int algo, char *signature, int cap)
{
  if (numberPixels < 2 || numberPixels > kMaxPixels || maxDisplaceCenter < 0 || gridSpaceCenter < 1 ||
      maxDisplaceCenter >= numberPixels / 2 || !signature || cap < 1)
    return 2;
  const KernelPlan P = plan_kernels(numberPixels, maxDisplaceCenter, gridSpaceCenter, algo);
  if (P.err || !P.fn)
    return 1;
  plan_signature(P, signature, (size_t) cap);
  if (P.tileT)
  {
    const size_t n = strlen(signature);
    snprintf(signature + n, (size_t) cap - n, " x %d^2 tiles of %d rows", P.tilesPerAxis, P.tileT);
  }
  return 0;
}

int bioem_hip_plan_own(int numberPixels, int maxDisplaceCenter, int gridSpaceCenter, int algo, char *signature, int cap)
{
  if (numberPixels < 2 || numberPixels > kMaxPixels || maxDisplaceCenter < 0 || gridSpaceCenter < 1 ||
      maxDisplaceCenter >= numberPixels / 2 || !signature || cap < 1)
    return 2;
  const KernelPlan P = plan_kernels(numberPixels, maxDisplaceCenter, gridSpaceCenter, algo);
  if (P.err || !P.fn)
    return 1;
  plan_own_signature(P, plan_own_kernel(P) != nullptr, signature, (size_t) cap);
  if (P.tileT)
  {
    const size_t n = strlen(signature);
    snprintf(signature + n, (size_t) cap - n, " x %d^2 tiles of %d rows", P.tilesPerAxis, P.tileT);
  }
  return 0;
}

const char *bioem_hip_own_kernel_signature(bioem_hip_handle h)
{
  if (!h)
    return "";
  static thread_local char buf[128];
  if (h->direct)
    snprintf(buf, sizeof(buf), "per particle: k_compare_direct<3, 8>");
  else
    plan_own_signature(h->plan, h->ownFn != nullptr, buf, sizeof(buf));
  return buf;
}

const char *bioem_hip_kernel_name(bioem_hip_handle h)
{
  if (!h)
    return "";
  if (h->direct)
    return "k_compare_direct";
  switch (h->plan.family)
  {
  case KF_FAST: return "k_compare_fast";
  case KF_FASTM: return "k_compare_fastm";
  case KF_FASTM2: return "k_compare_fastm2";
  case KF_WIDE2: return "k_compare_wide2";
  case KF_ODDFFT: return "k_compare_oddfft";
  case KF_ROWS: return "k_compare_rows";
  default: return "k_compare_generic";
  }
}

const char *bioem_hip_kernel_signature(bioem_hip_handle h)
{
  if (!h)
    return "";
  static thread_local char buf[96];
  if (h->direct)
    snprintf(buf, sizeof(buf), "k_compare_direct<3, 8>");
  else
    plan_signature(h->plan, buf, sizeof(buf));
  return buf;
}

int bioem_hip_r2c(int device, int N, int nImg, const float *in, float *out)
{
  if (N < 1 || N > kMaxPixels || nImg < 1 || hipSetDevice(device) != hipSuccess || dft_allow_lds(N) != hipSuccess)
    return 1;
  const int H = N / 2 + 1;
  const size_t M = (size_t) N * H;
  int nCU = 256;
  hipDeviceGetAttribute(&nCU, hipDeviceAttributeMultiprocessorCount, device);
  std::vector<double2> twd(N);
  for (int k = 0; k < N; k++)
    twd[k] = twiddle_d(k, N);
  double2 *dTw = nullptr, *dRow = nullptr;
  float *dIn = nullptr;
  float2 *dOut = nullptr;
  int rc = 1;
  if (hipMalloc(&dTw, sizeof(double2) * N) == hipSuccess && hipMalloc(&dRow, sizeof(double2) * M * nImg) == hipSuccess &&
      hipMalloc(&dIn, sizeof(float) * (size_t) N * N * nImg) == hipSuccess &&
      hipMalloc(&dOut, sizeof(float2) * M * nImg) == hipSuccess &&
      hipMemcpy(dTw, twd.data(), sizeof(double2) * N, hipMemcpyHostToDevice) == hipSuccess &&
      hipMemcpy(dIn, in, sizeof(float) * (size_t) N * N * nImg, hipMemcpyHostToDevice) == hipSuccess)
  {
    if (launch_r2c(0, nCU, nullptr, dIn, nullptr, 1.f, N, nImg, dTw, dRow, dOut) == hipSuccess &&
        hipMemcpy(out, dOut, sizeof(float2) * M * nImg, hipMemcpyDeviceToHost) == hipSuccess)
      rc = 0;
  }
  hipFree(dTw);
  hipFree(dRow);
  hipFree(dIn);
  hipFree(dOut);
  return rc;
}

} // extern "C"

