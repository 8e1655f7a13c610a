/* bioem_hip.h -- C ABI of the MI355X-native BioEM likelihood engine (libbioem_hip.so).
 *
 * This is the drop-in boundary for the reference's accelerator plugin (class bioem_cuda,
 * /root/reference/include/bioem_cuda_internal.h:28-85, created by bioem_cuda_create(),
 * /root/reference/include/bioem_cuda.h:20): plain pointers and sizes, no C++/torch types.
 * Every entry point names the reference interface it replaces.  All functions return 0 on
 * success and a non-zero code on failure (bioem_hip_last_error() gives the text); the C++
 * shim (bioem_amd/host) maps non-zero to the reference's print-and-exit (defs.h:18-26).
 *
 * Threading: all entry points of one handle are called from one host thread (the reference
 * calls its plugin from the main thread only, bioem.cpp:853).  One handle drives one GPU.
 */
#ifndef BIOEM_HIP_H
#define BIOEM_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* == bioem_param_device, /root/reference/include/param.h:26-47 (60 bytes, bool tousepsf widened) */
typedef struct
{
  int maxDisplaceCenter;
  int GridSpaceCenter;
  int NumberPixels;
  int NumberFFTPixels1D;
  int NxDisp;
  int NtotDisp;
  float Ntotpi;
  float volu;
  float sigmaPriorbctf;
  float sigmaPriordefo;
  float Priordefcent;
  float sigmaPrioramp;
  float Priorampcent;
  int writeAngles;
  int tousepsf;
} bioem_hip_param_device;

/* == myparam5_t, /root/reference/include/defs.h:128-135 (20 bytes) */
typedef struct
{
  float amp, pha, env, sumC, sumsquareC;
} bioem_hip_param5;

/* == bioem_Probability_map, /root/reference/include/map.h:116-128 (40 bytes) */
typedef struct
{
  double Total;
  double Constoadd;
  int max_prob_cent_x, max_prob_cent_y, max_prob_orient, max_prob_conv;
  float max_prob_norm, max_prob_mu;
} bioem_hip_prob_map;

/* == bioem_Probability_angle, /root/reference/include/map.h:130-135 (16 bytes) */
typedef struct
{
  double forAngles;
  double ConstAngle;
} bioem_hip_prob_angle;

/* == bioem_model::bioem_model_point, /root/reference/include/model.h:23-29 (24 bytes) */
typedef struct
{
  float pos[3];
  float quat4_unused;
  float radius;
  float density;
} bioem_hip_model_point;

/* One of the K most probable orientations of a particle (WRITE_PROB_ANGLES): the angle entry of orientation
 * `orient` (global index) and logp = log(forAngles) + ConstAngle + numconst, the key the reference's writer ranks
 * by (/root/reference/bioem.cpp:1251-1286).  32 bytes. */
typedef struct
{
  double forAngles;
  double ConstAngle;
  double logp;
  int orient;
  int pad;
} bioem_hip_angle_candidate;

typedef struct bioem_hip_ctx *bioem_hip_handle;

/* Number of visible HIP devices (replaces bioem_cuda::selectCudaDevice, bioem_cuda.cu:686-816). */
int bioem_hip_device_count(void);

/* Replaces bioem_cuda::deviceInit (bioem_cuda.cu:818-951): allocate device state for nMaps particles,
 * nAngles orientations, nCTF kernels.  algo = BIOEM_ALGO (1 or 2: displacement set + reduction
 * semantics of bioem_algorithm.h:144-198 / bioem.cpp:1461-1602).  device = HIP ordinal.
 * Environment, read here: BIOEM_CC_DIRECT=1 makes the handle evaluate the cross-correlation of bioem.cpp:1435-1459 as
 * a sliding window in real space instead of through the transform (BASELINE config 4; no counterpart in the
 * reference, doc/index.rst:1658-1663): images up to 160 pixels, regular windows of at most 24 offsets per axis,
 * particles through bioem_hip_upload_particle_maps; create fails with a message otherwise. */
int bioem_hip_create(bioem_hip_handle *out, int device, const bioem_hip_param_device *pd, int nMaps, int nAngles,
                     int nCTF, int algo);
/* Shard variant of bioem_hip_create for orientation-sharded runs (the reference's MPI blocks, bioem.cpp:748-753): this
 * handle only ever compares orientations [iOrientBegin, iOrientEnd) of the nAngles global ones.  With
 * WRITE_PROB_ANGLES its angle table is [iOrientEnd - iOrientBegin][nMaps] (each orientation has one owner) and stays on
 * the device: start_run / finish_run move only the nMaps 40-byte map entries (bioem_hip_prob_size(nMaps, 0, 0)
 * bytes), the K best orientations per particle come from bioem_hip_topk_angles.  Orientation and CTF indices in all
 * calls and results stay GLOBAL. */
int bioem_hip_create_shard(bioem_hip_handle *out, int device, const bioem_hip_param_device *pd, int nMaps, int nAngles,
                           int nCTF, int algo, int iOrientBegin, int iOrientEnd);
int bioem_hip_destroy(bioem_hip_handle h); /* bioem_cuda::deviceExit, bioem_cuda.cu:1023-1053 */
const char *bioem_hip_last_error(bioem_hip_handle h);

/* Particle side.  refFFT = bioem_RefMap::RefMapsFFT [nMaps][N][N/2+1] (re,im), sum/sumsq =
 * sum_RefMap / sumsquare_RefMap (map.h:65-74; uploaded at bioem_cuda.cu:824-846). */
int bioem_hip_upload_particles(bioem_hip_handle h, const float *refFFT, const float *sum, const float *sumsq);
/* North-star variant: real-space maps [nMaps][N][N]; sums (bioem.cpp:2087-2107, same float summation
 * order) and r2c (map.cpp:557-601) run on the device. */
int bioem_hip_upload_particle_maps(bioem_hip_handle h, const float *maps);

/* bioem_param::refCTF [nCTF][N][N/2+1] (re,im) and CtfParam [nCTF] as {amp, phase, env} triples
 * (param.h:76-77, filled at param.cpp:1336-1583). */
int bioem_hip_upload_ctf(bioem_hip_handle h, const float *refCTF, const float *ctfParam3);
/* bioem_model::points / NormDen and the projection parameters used by bioem::createProjection
 * (bioem.cpp:1604-1853). */
int bioem_hip_upload_model(bioem_hip_handle h, const bioem_hip_model_point *pts, int nPts, float NormDen,
                           float pixelSize, int shiftX, int shiftY);
/* bioem_param::angles [n] as {pos0,pos1,pos2,quat4} (defs.h:105-110); isQuat = param.doquater. */
int bioem_hip_upload_orientations(bioem_hip_handle h, const float *angles4, int n, int isQuat);
/* One orientation list per particle: angles4 = [nMaps][K] x {pos0,pos1,pos2,quat4}; K <= nAngles of the handle.
 * No reference counterpart as an interface: it is round 2 of doc/index.rst "modcom", where the reference runs one
 * process per particle with --ReadOrientation <that particle's list>.  Returns 2 (bioem_hip_last_error says why) for
 * K < 1 or K > nAngles and for handles the own-list pass does not take: tiled wide windows, BIOEM_CC_DIRECT=1, shards.
 * The pipeline buffers of the handle grow to the batches of that pass (up to 1 024 list entries each: several GB at
 * large images) and stay that size; when that memory is not there the call returns 1 and the handle is as it was. */
int bioem_hip_upload_particle_orientations(bioem_hip_handle h, const float *angles4, int K, int isQuat);
/* The same with lists of any length: particle p owns entries offsets[p] ... offsets[p + 1] of angles4 (offsets[nMaps + 1],
 * offsets[0] = 0, non-decreasing, every length <= nAngles of the handle).  A particle with an empty list takes no part in
 * the pass: its entries of the probability block stay as bioem_hip_start_run left them.  Returns 2 with a message for
 * offsets[0] != 0, decreasing offsets, a list longer than nAngles, an empty total and the handle kinds refused above; the
 * handle stays usable (and keeps the lists it had).  bioem_hip_upload_particle_orientations is the offsets[p] = p K case
 * of this entry. */
int bioem_hip_upload_particle_orientation_lists(bioem_hip_handle h, const float *angles4, const long long *offsets,
                                                int isQuat);

/* bioem::malloc_device_host / free_device_host (bioem.h:56-57; bioem_cuda.cu:1037-1053): pinned host memory
 * for the probability block. */
void *bioem_hip_host_alloc(size_t size);
void bioem_hip_host_free(void *ptr);
/* size of the probability block, == bioem_Probability::get_size (map.h:156-162) */
size_t bioem_hip_prob_size(int nMaps, int nAngles, int writeAngles);

/* bioem_cuda::deviceStartRun (bioem_cuda.cu:953-1011): upload the (initialised) probability block. */
int bioem_hip_start_run(bioem_hip_handle h, const void *pProb_host);

/* Reference-compatible hot-path entry == bioem::compareRefMaps (bioem.h:52-54; CUDA override
 * bioem_cuda.cu:527-684).  conv_mapsFFT / comp_params are the BASE pointers of the caller's 2-slot buffers;
 * slot offset k = (iPipeline & 1) * nTotParallelConv as in bioem.cpp:1388.  Asynchronous like the CUDA
 * plugin: returns after enqueue; slot k may be overwritten after the next call with the same parity
 * has returned. */
int bioem_hip_compare(bioem_hip_handle h, int iPipeline, int iOrient, int iConvStart, int maxParallelConv,
                      int nTotParallelConv, const float *conv_mapsFFT, const bioem_hip_param5 *comp_params);

/* North-star entry: bioem::createProjection + createConvolutedProjectionMap + compareRefMaps
 * (the body of the run() loop, bioem.cpp:763-891) for orientations [iOrientBegin, iOrientEnd) and all CTFs,
 * entirely on the device. */
int bioem_hip_project_convolve_compare(bioem_hip_handle h, int iOrientBegin, int iOrientEnd);

/* The same for orientations [iOrientBegin, iOrientEnd) and CTFs [iConvBegin, iConvEnd) only: when there are fewer
 * orientations than GPUs the CTF grid is split as well (north_star: "orientations x CTF-envelope grid shard"). */
int bioem_hip_project_convolve_compare_ctf(bioem_hip_handle h, int iOrientBegin, int iOrientEnd, int iConvBegin,
                                           int iConvEnd);

/* project -> convolve -> compare, on the device, of list entries [0, K) x all CTFs of particles [iMapBegin, iMapEnd),
 * each particle against its own list only (bioem_hip_upload_particle_orientations).  Per particle the result equals what
 * bioem_hip_project_convolve_compare gives on a handle that holds that particle alone and its list as the shared list:
 * max_prob_orient is the index in THAT particle's list, and with WRITE_PROB_ANGLES entry (k, p) of the
 * [nAngles][nMaps] table receives list entry k of particle p.  Entries of particles outside the range are not touched.
 * Asynchronous like the fused entry; start_run / finish_run as usual.  Phase records of this pass carry the range of
 * flat slots offsets[p] + k of a batch in iOrientBegin / iOrientEnd.  A batch is compared by one launch per particle, or,
 * after bioem_hip_set_own_launch, by ONE launch of k_compare_fast_own where the shape runs k_compare_fast
 * (bioem_hip_own_kernel_signature says which); the two give the same bits. */
int bioem_hip_compare_own_orientations(bioem_hip_handle h, int iMapBegin, int iMapEnd);
/* How that pass launches its comparison, from the next call on: one launch per particle (the default of every handle),
 * or one launch per batch where the shape has the kernel for it (bioem_hip_plan_own; its block table with a particle's
 * blocks on one XCD, or in plain row order; elsewhere the call changes nothing).  Results do not depend on it, bit for
 * bit.  The single launch is opt-in: it has not been measured against the per-particle launches on one device yet.
 * Returns 2 for an unknown mode. */
#define BIOEM_HIP_OWN_LAUNCH_PARTICLE 0
#define BIOEM_HIP_OWN_LAUNCH_BATCH 1
#define BIOEM_HIP_OWN_LAUNCH_BATCH_ROWS 2
int bioem_hip_set_own_launch(bioem_hip_handle h, int mode);
/* Which instantiation of k_compare_fast the comparison launches of this handle take, from the next launch on.  The kernels
 * with the static 21-row window pass have a lean variant that holds that one path alone -- the whole window, no split last
 * column block -- with fewer registers; a launch that would take that path through the full instantiation computes the same
 * bits in either.  lean = 1, the default of every handle: such launches take the lean variant; lean = 0: the full
 * instantiations only.  Returns 1 if the launches of this handle at its plan and shape now take a lean kernel, else 0.
 * The labels of bioem_hip_kernel_signature / bioem_hip_plan do not depend on it. */
int bioem_hip_set_compare_variant(bioem_hip_handle h, int lean);

/* The same three stages as separate entries, for an integrator who keeps the reference's loop (bioem.cpp:763-891) and
 * replaces its body piece by piece: every call is asynchronous and batched, and what one stage produces stays on the
 * device, in the comparison's layout, for the next.  iPipeline & 1 names one of two buffer sets, as in
 * bioem::compareRefMaps (bioem.cpp:1388): stage calls on one set are ordered, the two sets overlap (projection and
 * convolution of set 1 run beside the comparison of set 0).  Results are bit-identical to
 * bioem_hip_project_convolve_compare over the same (orientation, CTF) rows in the same order.
 *   bioem_hip_project         == bioem::createProjection (bioem.h:61, bioem.cpp:1604-1853) for [iOrientBegin, iOrientEnd),
 *                                at most maxOrientations of bioem_hip_max_batch per call
 *   bioem_hip_convolve        == bioem::createConvolutedProjectionMap (bioem.h:43-45, bioem.cpp:1855-1923) for every
 *                                projection of the set x CTFs [iConvBegin, iConvEnd); rows (orientation-major) <= maxRows
 *   bioem_hip_compare_device  == bioem::compareRefMaps (bioem.h:52-54) for the conv spectra of the set against all particles */
int bioem_hip_project(bioem_hip_handle h, int iPipeline, int iOrientBegin, int iOrientEnd);
int bioem_hip_convolve(bioem_hip_handle h, int iPipeline, int iConvBegin, int iConvEnd);
int bioem_hip_compare_device(bioem_hip_handle h, int iPipeline);
/* capacity of a buffer set: orientations per bioem_hip_project call, (orientation, CTF) rows per bioem_hip_convolve call */
int bioem_hip_max_batch(bioem_hip_handle h, int *maxOrientations, int *maxRows);

/* bioem_cuda::deviceFinishRun (bioem_cuda.cu:1013-1021): synchronise, download the probability block. */
int bioem_hip_finish_run(bioem_hip_handle h, void *pProb_host);

/* The posterior per CTF set and particle (no reference counterpart: the reference would need one process per CTF set).
 * The CTF table is [nCTF][nMaps] bioem_hip_prob_map, CTF index slowest and GLOBAL.  Entry (c, p) is what particle p's
 * entry of the probability block would be had the run compared CTF set c only: the fold, in orientation order, of the
 * comparisons (o, c) by the rules of the particle entries (log-sum-exp in double, first maximum = lowest row,
 * max_prob_conv = c, the other record fields from the best row), with whatever priors the comparisons carry.  It
 * accumulates across batches, launches and calls like the particle entries, through every comparison entry of every
 * handle kind (bioem_hip_compare, the fused and the staged entries, bioem_hip_compare_own_orientations, where
 * max_prob_orient is the index in the particle's own list).  Per particle the log-sum-exp over c of
 * log(Total) + Constoadd equals the particle entry's, and the entry of largest Constoadd (lowest c among equals)
 * carries the particle entry's record.  No atomics: two runs give the same bits.
 * bioem_hip_enable_ctf_table(h, 1) allocates the nCTF x nMaps entries on the device (on = 0 frees them); call it
 * outside a run: between bioem_hip_start_run and bioem_hip_finish_run it returns 2 with a message.  The default is off:
 * a handle that never enables the table allocates nothing and launches nothing for it.  bioem_hip_start_run
 * initialises the entries as the reference initialises a particle entry (Total = 0, Constoadd = MIN_PROB, the rest 0).
 * bioem_hip_ctf_table flushes the rows staged through bioem_hip_compare, synchronises and copies the table to
 * out[nCTF * nMaps]; it returns 2 when the table is not enabled.
 * Shards (orientation blocks, CTF sub-ranges or both): fetch every handle's table and merge them, shards in ascending
 * orientation-block order, with bioem_hip_merge_host(nShards, nCTF * nMaps, 0, 0, tables, out) -- the table is an array
 * of map entries and the merge works entry by entry; an entry a shard never touched drops out of it. */
int bioem_hip_enable_ctf_table(bioem_hip_handle h, int on);
int bioem_hip_ctf_table(bioem_hip_handle h, bioem_hip_prob_map *out);

/* The calculated image of the best match of particles [iMapBegin, iMapEnd): what bioem::printModel writes for ONE
 * hand-copied record (bioem.cpp:624-657, 1925-2085), for every record of a run, on the device.
 * records = [nMaps] bioem_hip_prob_map on the HOST (the block of finish_run, or a merged one: indices are global).
 * ownLists = 0: max_prob_orient indexes the shared list (bioem_hip_upload_orientations);
 * ownLists = 1: it indexes particle p's own list (bioem_hip_upload_particle_orientation_lists).
 * maps_out = [iMapEnd - iMapBegin][N][N] float on the host.
 * For the record (o, c, X, Y, norm, mu): Z = P_o conj(CTF_c) in float (bioem.cpp:1952-1955), conv = the unnormalised c2r
 * of Z (exact DFT, sums in double, rounded to float), out[(k + X) mod N][(j + Y) mod N] = conv[k][j] / N^2 * norm + mu
 * with the float operations in that order (bioem.cpp:2051-2053).  The reference reports the negative of the
 * correlation's displacement, so this is the map the posterior laid over the particle: with Ntotpi = N^2, norm and mu
 * are the least-squares slope and intercept, and the result is the least-squares fit of the particle at the arg-max.
 * Particles go in batches of at most maxOrientations of bioem_hip_max_batch (gather of the records' orientations,
 * projection, two inverse DFT passes, one copy to the host per batch) through buffer set 0, like the debug hooks: call
 * it outside a run; what was staged in set 0 is void afterwards.  Needs no particles and no comparison: every handle kind
 * serves it (shards hold the global list).  The staging buffers are allocated at the first call (1 when the memory is
 * not there; the handle is as it was).  Returns 2 with a message naming the particle, handle still usable, for a record
 * whose max_prob_orient lies outside its list (a particle no run touched), max_prob_conv outside [0, nCTF), |X| or
 * |Y| >= N; for an empty or reversed range, ownLists = 1 without own lists, model / CTFs / orientations not uploaded.
 * With bioem_hip_set_phase_timing the batches leave phase records: phase 0 the projection, 1 the column pass, 2 the row
 * pass, iOrientBegin / iOrientEnd the batch's records relative to iMapBegin. */
int bioem_hip_render_best_maps(bioem_hip_handle h, const bioem_hip_prob_map *records, int ownLists, int iMapBegin,
                               int iMapEnd, float *maps_out);

/* WRITE_PROB_ANGLES without moving the table: selects on the device the K best orientations of every particle among
 * the orientations this handle owns, with the reference writer's own rule (a K-entry min-heap on (logp, orientation)
 * walked in orientation order, bioem.cpp:1251-1286; numconst as computed at bioem.cpp:1141-1150).  out = [nMaps][K],
 * best first; entries beyond the owned orientation count have orient = -1.  Call after finish_run.
 * For a handle that owns the whole list this IS the writer's result.  For shards, the K best of the union of such
 * K-wide lists is the writer's result only while no equal keys meet a shard's threshold: a heap that is full rejects
 * the newest of equal keys and evicts the oldest, so which of them survive depends on what the earlier blocks held.
 * Lists for a merge come from bioem_hip_merge_candidates, which always reproduces the writer. */
int bioem_hip_topk_angles(bioem_hip_handle h, int K, double numconst, bioem_hip_angle_candidate *out);
/* The list a shard contributes to a merge: out = [nMaps][2K - 1].  Slots 0 ... K-1 are exactly what
 * bioem_hip_topk_angles returns.  Slots K ... 2K-2 hold, in ascending orientation, the entries whose key equals the
 * K-th best key t of the block, that lie among the block's first K entries of key >= t, and that the block's own walk
 * rejected or evicted (at most K - 1); unused slots are (0, MIN_PROB, -inf, -1).  The writer's loop over the union of
 * the shards' lists, in orientation order (bioem_hip_merge_topk_host_wide with W = 2K - 1), equals the writer's loop
 * over the whole table for any keys and any cut into blocks. */
int bioem_hip_merge_candidates(bioem_hip_handle h, int K, double numconst, bioem_hip_angle_candidate *out);
/* Merge of the shards' candidate lists (any shard order: the union is sorted by orientation): the writer's heap rule
 * over the union.  cands[s] = [nMaps][W] with W >= K, slots with orient < 0 are skipped; out = [nMaps][K], best
 * first, unused slots (0, MIN_PROB, -inf, -1).  W = 2K - 1 with lists of bioem_hip_merge_candidates reproduces the
 * writer; bioem_hip_merge_topk_host is the same call with W = K, for K-wide lists (see bioem_hip_topk_angles for
 * what those cannot guarantee).  No device.  Returns 2 for nShards < 1, K < 1, W < K or a null argument. */
int bioem_hip_merge_topk_host_wide(int nShards, int nMaps, int K, int W, const bioem_hip_angle_candidate *const *cands,
                                   bioem_hip_angle_candidate *out);
int bioem_hip_merge_topk_host(int nShards, int nMaps, int K, const bioem_hip_angle_candidate *const *cands,
                              bioem_hip_angle_candidate *out);
/* test hooks, no RCCL.  bioem_hip_debug_topk: the selection kernel with the launch shape of the two entries above on a
 * table handed in, table = [nO][nMaps] on the host, o0 the global index of its first row, W = K or 2K - 1,
 * out = [nMaps][W].  bioem_hip_debug_merge_gathered: the half of bioem_hip_merge that follows the all-gather, on
 * `gathered` = nShards payloads of nMaps map entries followed (K > 0) by nMaps lists of 2K - 1 candidates, as the
 * all-gather leaves them, for the handle's nMaps; maps_out = [nMaps] map entries, cand_out = [nMaps][K] (NULL with
 * K = 0).  Both return 2 with a message for a null argument or a shape they do not serve. */
int bioem_hip_debug_topk(bioem_hip_handle h, const bioem_hip_prob_angle *table, int nO, int nMaps, int o0, int K, int W,
                         double numconst, bioem_hip_angle_candidate *out);
int bioem_hip_debug_merge_gathered(bioem_hip_handle h, const void *gathered, int nShards, int K, void *maps_out,
                                   bioem_hip_angle_candidate *cand_out);

/* Log-sum-exp merge of orientation shards (replaces the MPI merge of bioem.cpp:909-1044) on the host:
 * shards = nShards probability blocks of identical shape, out = merged block.  Ties on Constoadd go to
 * the lowest shard (= lowest orientation index, the serial semantics). */
int bioem_hip_merge_host(int nShards, int nMaps, int nAngles, int writeAngles, const void *const *shards, void *out);

/* The path's single exchange step over RCCL / xGMI (replaces the MPI merge of bioem.cpp:909-1044) for n handles on n
 * DIFFERENT GPUs of this process: every device contributes its nMaps map entries -- and, when K > 0, its list of
 * 2K - 1 candidates per particle (bioem_hip_merge_candidates) -- to ONE ncclAllGather; the device of handles[0] folds the
 * gathered shards (log-sum-exp of Total / Constoadd, arg-max record from the lowest shard holding the maximum =
 * lowest orientation index; candidates by the heap rule) and the result is copied to the host.
 * pProbMaps_host = [nMaps] bioem_hip_prob_map, cand_host = [nMaps][K] or NULL when K == 0.  Call after every handle's
 * finish_run.  The communicator is created on first use (ncclCommInitAll) and cached; librccl.so is loaded lazily.
 * Threading: ONE thread hands over all handles of a merge; calls are serialised process-wide (a mutex spans communicator
 * creation and the grouped all-gather), so merges of different handle sets from different threads queue -- they cannot
 * interleave their RCCL group calls. */
int bioem_hip_merge(bioem_hip_handle *handles, int n, void *pProbMaps_host, int K, double numconst,
                    bioem_hip_angle_candidate *cand_host);

/* Stand-alone forward transform (FFTW r2c convention, [N][N/2+1] (re,im)) of nImg real N x N images on
 * `device`; replaces the fftwf_execute_dft_r2c call of the PSF kernel set-up (param.cpp:1521). */
int bioem_hip_r2c(int device, int N, int nImg, const float *in, float *out);

/* The reference's only built-in profile, BIOEM_DEBUG_OUTPUT >= 1 (TimeStat, timer.cpp:138-165; the "Time Projection /
 * Convolution / Comparison" lines of bioem.cpp:769-889): device time of every phase of every batch, from HIP events on
 * the streams the phases run on.  Off by default; records accumulate from set_phase_timing(h, 1) on and are handed over
 * (and dropped) by phase_records after finish_run: *n = records available, the first min(*n, cap) are written. */
enum
{
  BIOEM_HIP_PHASE_PROJECTION = 0, /* bioem::createProjection of orientations [iOrientBegin, iOrientEnd) */
  BIOEM_HIP_PHASE_CONVOLUTION = 1, /* createConvolutedProjectionMap of those x CTFs [iConvBegin, iConvEnd) */
  BIOEM_HIP_PHASE_COMPARISON = 2   /* compareRefMaps of those rows against all particles, fold included */
};
typedef struct
{
  int phase;
  int iOrientBegin, iOrientEnd, iConvBegin, iConvEnd; /* -1: rows handed over through bioem_hip_compare */
  double seconds;
} bioem_hip_phase_record;
int bioem_hip_set_phase_timing(bioem_hip_handle h, int on);
int bioem_hip_phase_records(bioem_hip_handle h, bioem_hip_phase_record *out, int cap, int *n);

/* ---- instrumentation / test hooks (no reference equivalent) ---- */
/* projection spectrum of one orientation in reference layout [N][N/2+1][2] */
int bioem_hip_debug_projection(bioem_hip_handle h, int iOrient, float *spec_out);
/* The real-space projections of orientations [o0, o0 + nO) of the shared list, one batch through buffer set 0 (outside a
 * run; nO <= maxOrientations of bioem_hip_max_batch): maps_out [nO][N][N] double (a box stored compactly on the device
 * is put into place, zeros around it), tempden_out [nO] double, spec_out NULL or [nO][N][N/2+1][2] float in reference
 * layout, info_out [6] int = {path taken, boxLo, boxSide, compact, TR, iradMax}.  path: 0 what a run takes, 1 the box
 * kernel, 2 records + bands, 3 global atomics.  A forced path whose preconditions do not hold (no footprint table, box
 * beyond 52 KiB, a quaternion list not of unit length, bands of fewer than 12 rows, footprints beyond 33 pixels, records
 * that do not fit) and every other invalid argument are refused with 2 and a message; the handle stays usable. */
int bioem_hip_debug_projection_maps(bioem_hip_handle h, int o0, int nO, int path, double *maps_out, double *tempden_out,
                                    float *spec_out, int *info_out);
/* the footprint table of the model, stamps_out [nPts][S][S] double with S = 2 iradMax + 1 (stamps_out NULL: iradMax
 * alone); 2 where the model has none (a footprint beyond 33 pixels, no points) */
int bioem_hip_debug_stamps(bioem_hip_handle h, double *stamps_out, int *iradMax_out);
/* conv spectrum + {sumC, sumsquareC} of (iOrient, iConv) in reference layout */
int bioem_hip_debug_convolution(bioem_hip_handle h, int iOrient, int iConv, float *spec_out, float *sumC,
                                float *sumsquareC);
/* One whole convolution batch as a run launches it, from projection spectra the caller hands in (outside a run): buffer
 * set 0 takes specP [nO][N][N/2+1][2] (reference layout) as its projection spectra, its conv rows [0, nO nC + 1) and the
 * same entries of its parameter list are filled with 0xFF bytes, and the convolution of the nO orientations with the
 * handle's CTF sets [c0, c0 + nC) (bioem_hip_upload_ctf) is launched exactly as a run launches it -- the fused kernel or the
 * two kernels, BIOEM_CONVOLVE_FUSED read at this call.  conv_out [nO nC + 1][N][N/2+1][2]: row o nC + c in reference
 * layout, the last one the guard row no kernel may have written; params_out [nO nC + 1] likewise; raw_out NULL or the
 * nO nC rows as they lie in the comparison layout, [nO nC][N Hp][2] float; info_out [6] int = {fused path (1 / 0), R / 2
 * of the comparison layout (0: reference layout), N1, Hp, rows handed out, guard row present}.  Refused with 2 and a
 * message, the handle usable afterwards: a null argument (raw_out may be), CTF sets not uploaded, nO outside
 * [1, maxOrientations], a CTF range empty or outside [0, nCTF), nO nC + 1 rows more than a batch holds, the two-kernel
 * path selected without a buffer for the ordered sums of nO nC rows. */
int bioem_hip_debug_convolve_batch(bioem_hip_handle h, const float *specP, int nO, int c0, int nC, float *conv_out,
                                   bioem_hip_param5 *params_out, float *raw_out, int *info_out);
/* The c2r of a BIOEM_CC_DIRECT handle (compare_direct.hpp) on conv spectra the caller hands in, outside a run: specConv
 * [nRows][N][N/2+1][2] (reference layout) goes into the conv rows of buffer set 0 through the reorder of
 * bioem_hip_compare, and k_c2r_cols and k_c2r_rows are launched on them with the launch parameters of a run.  Z_out NULL
 * or [nRows][N][N/2+1] double2, the column pass Z[x][ky]; real_out [nRows][N][N] float, the unnormalised real maps the
 * comparison kernel reads.  Refused with 2 and a message, the handle usable afterwards: a handle that is not direct, a
 * null argument (Z_out may be), nRows outside [1, conv rows of a batch]. */
int bioem_hip_debug_direct_conv(bioem_hip_handle h, const float *specConv, int nRows, double *Z_out, float *real_out);
/* download device-side particle precompute (reference layout); refFFT_out may be NULL: the sums alone */
int bioem_hip_debug_particles(bioem_hip_handle h, float *refFFT_out, float *sum_out, float *sumsq_out);
/* accumulated HIP-event time of the comparison kernel on the engine's stream since the last reset:
 * total ms, launches, comparisons processed */
int bioem_hip_kernel_stats(bioem_hip_handle h, double *compare_ms, long long *launches, long long *comparisons);
int bioem_hip_reset_kernel_stats(bioem_hip_handle h);
/* 1 if the LDS-FFT fast path is used for this configuration, 0 for the generic pruned-DFT path */
int bioem_hip_uses_fast_path(bioem_hip_handle h);
/* name of the comparison kernel this configuration runs: "k_compare_fast", "k_compare_wide" (tiled wide window),
 * "k_compare_oddfft" / "k_compare_rows" (odd image size with / without a factor 3 or 5) or "k_compare_generic" */
const char *bioem_hip_kernel_name(bioem_hip_handle h);
/* the same with the template arguments of the instantiation, spelled as rocprofv3 prints them (e.g.
 * "k_compare_fast<10, 32, false, 1>"): lets bench.py tie its live timing to the committed counter profile of exactly
 * this kernel */
const char *bioem_hip_kernel_signature(bioem_hip_handle h);
/* Which comparison kernel a configuration would run, without a device (no reference counterpart; the selection is a
 * pure function of the image size and the displacement set, bioem_amd/csrc/kernel_select.hpp).  Writes the
 * instantiation -- and " x T^2 tiles of R rows" for a tiled wide window -- into signature[cap]; 0 on success, 1 when no
 * kernel fits, 2 on invalid arguments. */
int bioem_hip_plan(int numberPixels, int maxDisplaceCenter, int gridSpaceCenter, int algo, char *signature, int cap);
/* What bioem_hip_compare_own_orientations launches for a configuration once bioem_hip_set_own_launch has asked for one
 * launch per batch, without a device: "k_compare_fast_own<...>" where the shape has that kernel (the label names the
 * OwnCompareArgs instantiation of k_compare_fast with those template arguments), else the signature of
 * bioem_hip_plan prefixed "per particle: " (such a shape keeps per-particle launches in every mode).  Same return codes. */
int bioem_hip_plan_own(int numberPixels, int maxDisplaceCenter, int gridSpaceCenter, int algo, char *signature, int cap);
/* what a handle launches in the mode it is in: "per particle: ..." until bioem_hip_set_own_launch says otherwise */
const char *bioem_hip_own_kernel_signature(bioem_hip_handle h);
int bioem_hip_synchronize(bioem_hip_handle h);

/* ---- Fourier ring sums of every particle against its best match (no reference counterpart) ----
 * For particle p with the record (o, c, X, Y, norm, mu), N = NumberPixels, H = N / 2 + 1, spectra [N][H] (re, im):
 *   R = the particle's spectrum as the handle holds it (bioem_hip_debug_particles), widened to double;
 *   Z = P_o conj(CTF_c) formed in DOUBLE from the float projection spectrum and CTF kernel (bioem_hip_render_best_maps
 *       forms it in float: 2^-24 relative apart);
 *   M[k1][k2] = norm Z[k1][k2] exp(-2 pi i t / N), t = (k1 X + k2 Y) mod N reduced in integers, and mu N^2 added to the real
 *       part of M[0][0].  In the columns that are their own Hermitian partner (k2 = 0 and, N even, k2 = N / 2) M is the
 *       Hermitian part (M[k1][k2] + conj(M[(N - k1) mod N][k2])) / 2 of that expression: what the c2r of the render keeps of a
 *       product that is not the spectrum of a real image (the reference's CTF kernels are not even in k1), and the
 *       expression itself where it is.  So M is the r2c spectrum of the image bioem_hip_render_best_maps writes.
 * Ring of a coefficient: k1' = k1 for k1 <= N / 2 else k1 - N, r2 = k1'^2 + k2^2, s = floor(sqrt(r2)) plus one when
 * r2 > s^2 + s (the radius rounded to nearest, in integers); nRings = s(N / 2, N / 2) + 1, corners included.  Weight of
 * the Hermitian partner: w = 1 in column 0 and, N even, column N / 2, else 2 (sum w = N^2).  Per (particle, ring), in
 * double: cross = sum w Re(R conj(M)), powParticle = sum w |R|^2, powModel = sum w |M|^2.  The host derives the rest:
 * FRC = cross / sqrt(powParticle powModel), residual power = powParticle + powModel - 2 cross (summed over the rings and
 * divided by N^2: sum over pixels of (particle - best map)^2), resolution of ring s >= 1 = N pixelSize / s.
 * No floating-point atomics, and how an image is split over blocks depends on N alone: the same bits on every run,
 * whichever batch a particle sits in. */
typedef struct { double cross, powParticle, powModel; } bioem_hip_ring_sums;   /* 24 bytes */
int bioem_hip_ring_count(int numberPixels);            /* nRings; no device; <= 0 for numberPixels < 1 */
/* Calling rules of bioem_hip_render_best_maps (records on the host, ownLists, batches of at most maxOrientations through
 * buffer set 0, outside a run, every handle kind) and its refusals (2, the particle named, handle usable), plus: 2 when
 * no particles were uploaded.  Per batch: gather and projection as in the render, the batch's particle spectra back in
 * reference layout, one ring pass; nRings x 24 bytes per particle come back.  Staging buffers are allocated at the first
 * call (1 when the memory is not there; the handle is as it was).  Phase records: phase 0 the projection, phase 2 the
 * ring pass, iOrientBegin / iOrientEnd the batch's records relative to iMapBegin. */
int bioem_hip_best_match_rings(bioem_hip_handle h, const bioem_hip_prob_map *records, int ownLists,
                               int iMapBegin, int iMapEnd, bioem_hip_ring_sums *out /* [iMapEnd-iMapBegin][nRings] */);
/* test hook: the same ring kernel on spectra handed in by the caller (specR, specP = [n][N][H] (re, im); records[n]:
 * max_prob_conv, the shift, norm and mu are used, max_prob_orient is ignored; needs the CTF kernels only) */
int bioem_hip_debug_ring_sums(bioem_hip_handle h, const float *specR, const float *specP,
                              const bioem_hip_prob_map *records, int n, bioem_hip_ring_sums *out);

/* ---- Posterior over the displacement window of any (particle, orientation, CTF) match (no reference counterpart) ----
 * The comparison kernels fold the window of every comparison to one partial inside the kernel; this entry delivers the
 * window itself.  For a request (p, o, c), N = NumberPixels, H = N / 2 + 1, spectra [N][H] (re, im):
 *   conv = P_o conj(CTF_c) in float, the expression of the convolution (bioem_hip_debug_convolution delivers its bits and
 *       those of {amp, pha, env, sumC, sumsquareC}); F = the particle's spectrum as the handle holds it;
 *   S(dx, dy) = sum_ky w_ky Re( exp(+2 pi i ((ky dy) mod N) / N) sum_kx conv[kx][ky] conj(F[kx][ky]) exp(+2 pi i ((kx dx) mod N) / N) ),
 *       w = 1 in column 0 and, N even, column N / 2, else 2; the product is formed in double from the float spectra, the
 *       twiddle indices are reduced in integers, the sums run in double in a fixed order;
 *   cc = (float) S / (float) (N N) (one rounding, then the reference's float division, bioem_algorithm.h:163-164);
 *   logp = the reference's calc_logpro at cc, kept in double (narrowed to float for neither ALGO).
 * Cells are indexed by the shift the reference reports: X_0 < X_1 < ... are the values max_prob_cent_x can take for the
 * handle's (NumberPixels, maxDisplaceCenter, GridSpaceCenter, ALGO) -- ALGO 1 with maxDisplaceCenter 5, GridSpaceCenter 2
 * gives {-4, -2, 0, 1, 3, 5} -- and cell [i][j] of a table holds dx = -X_i, dy = -X_j: the arg-max cell of the table of a
 * particle's best (o, c) is (max_prob_cent_x, max_prob_cent_y), and the log-sum-exp over the cells is the pair's
 * log(Total) + Constoadd.  No atomics, a fixed summation order, and a record's split over blocks depends on (N, nd)
 * alone: the same bits on every run, in every batch, at any position of the request list. */
typedef struct { int particle, orient, conv; } bioem_hip_window_request;            /* 12 bytes */
/* nd, the cells per axis; no device; <= 0 on invalid arguments (N < 2, grid < 1, maxD < 0 or >= N / 2, ALGO not 1 or 2) */
int bioem_hip_window_count(int numberPixels, int maxDisplaceCenter, int gridSpaceCenter, int algo);
/* X_0 .. X_{nd-1} into shifts[cap] (as many as fit; shifts may be null); returns nd */
int bioem_hip_window_offsets(int numberPixels, int maxDisplaceCenter, int gridSpaceCenter, int algo, int *shifts, int cap);
/* Calling rules of bioem_hip_best_match_rings: requests on the host, outside a run, every handle kind, batches of at most
 * maxOrientations through buffer set 0; staging allocated at the first call (1 when the memory is not there; the handle is
 * as it was).  Requests are independent: any particle any number of times, in any order.  orient indexes the shared list,
 * or with ownLists = 1 the list of the request's particle.  Refused with 2, the request index named and the handle
 * usable: a null argument or n < 1; particle outside [0, nMaps); orient outside its list; conv outside [0, nCTF); model,
 * CTF kernels, orientations or particles not uploaded; ownLists = 1 without own lists.  A cell whose firstele is not
 * positive and finite holds what the formula gives (NaN or an infinity).  Phase records: 0 the projection, 1 conv and
 * the ordered Parseval sums, 2 the window pass; iOrientBegin / iOrientEnd the batch's requests. */
int bioem_hip_window_posterior(bioem_hip_handle h, const bioem_hip_window_request *req, int n, int ownLists,
                               double *logp_out /* [n][nd][nd] */, float *cc_out /* [n][nd][nd] or NULL */,
                               bioem_hip_param5 *params_out /* [n] or NULL */);
/* test hook: the same window kernels on spectra handed in (specConv, specRef = [n][N][H] (re, im), reference layout;
 * params[n] complete; the particles' sums per record).  Needs only the handle's parameters. */
int bioem_hip_debug_window(bioem_hip_handle h, const float *specConv, const float *specRef, const bioem_hip_param5 *params,
                           const float *sumRef, const float *sumsqRef, int n, double *logp_out, float *cc_out);

/* ---- Posterior over a list of CTF sets at any match: one projection against many kernels (no reference counterpart) ----
 * The counterpart of bioem_hip_window_posterior on the CTF axes: that entry gives every cell of the displacement window
 * for one CTF set of the handle, this one every CTF set of an arbitrary list for one cell.  With the symbols of the
 * section above, for request (p, o, X, Y) and candidate g with kernel K_g and parameters {amp, pha, env}_g:
 *   conv_g = P_o conj(K_g) in float, the unfused expression of the convolution; sumC its real part at the origin;
 *   sumsquareC = the reference's sequential float chain over the Parseval terms in the reference's order (rows; inside a
 *       row the interior columns doubled, then column 0, then column N / 2 for even N), then the division by N N: for a
 *       candidate that is one of the handle's own CTF sets, sumC and sumsquareC carry the bits of
 *       bioem_hip_debug_convolution;
 *   S = sum_k w_ky Re( conv_g[k] conj(F_p[k]) exp(+2 pi i ((kx dx + ky dy) mod N) / N) ), dx = -X, dy = -Y: the products
 *       in double from the float spectra, the twiddle index reduced in integers, the sum in double in a fixed order;
 *   cc = (float) S / (float) (N N);  logp = the reference's calc_logpro at cc with {amp, pha, env, sumC, sumsquareC} of
 *       the candidate (the CTF priors enter as in a run), kept in double for both ALGOs.
 * This is the cell (X, Y) of what bioem_hip_window_posterior would give had K_g been CTF set g of the handle; a shift
 * need not be a cell of the handle's window.  The kernels are taken as handed in (PSF-mode kernels included).  A
 * (request, candidate) result depends on its own inputs alone: the same bits for any G, any order or subset of candidates
 * or requests, and any batch size.
 * Calling rules of bioem_hip_window_posterior (the handle's CTF sets need not be uploaded).  Refused with 2, the request
 * named and the handle usable: a null argument or n < 1; null kernels or ctfParam3; G < 1; particle outside [0, nMaps);
 * orient outside its list; |shiftX| or |shiftY| >= N; model, orientations or particles not uploaded; ownLists = 1 without
 * own lists.  Staging is allocated at the first call and grown to the largest G (1 when the memory is not there; the
 * handle is as it was).  Batches of maxOrientations requests are projected and prepared one after the other; one launch
 * of the scan serves up to 16 of them (as many as keep the prepared spectra within 512 MiB).  Phase records: 0 the
 * projection and 1 the preparation of a batch (with the first batch the packing of the candidates), 2 the scan of the
 * batches gathered; iOrientBegin / iOrientEnd the requests of the batch, for phase 2 of the launch. */
typedef struct { int particle, orient, shiftX, shiftY; } bioem_hip_scan_request;   /* 16 bytes */
int bioem_hip_ctf_scan(bioem_hip_handle h, const bioem_hip_scan_request *req, int n, int ownLists,
                       const float *kernels   /* [G][N][H] (re, im), the layout bioem_hip_upload_ctf takes */,
                       const float *ctfParam3 /* [G] {amp, phase, env} */, int G,
                       double *logp_out /* [n][G] */, float *cc_out /* [n][G] or NULL */,
                       bioem_hip_param5 *params_out /* [n][G] or NULL */);
/* test hook: the same kernels on spectra handed in (specP, specRef = [n][N][H] (re, im), reference layout; the particles'
 * sums per record; needs only the handle's parameters) */
int bioem_hip_debug_ctf_scan(bioem_hip_handle h, const float *specP, const float *specRef, const float *sumRef,
                             const float *sumsqRef, const int *shiftXY /* [n][2] */, int n, const float *kernels,
                             const float *ctfParam3, int G, double *logp_out, float *cc_out,
                             bioem_hip_param5 *params_out);

/* ---- Density gradient of the log posterior per model point (no reference counterpart) ----
 * For request (p, o, c, X, Y) the derivative of the log posterior of that match with respect to the density rho_k of every
 * model point.  N = NumberPixels, Nt = N N.  Projection (createProjection): U = sum_k v_k rho_k s_k placed at the point's
 * pixel, T = sum_k v_k rho_k sigma_k, P = (NormDen / T) U; s_k the footprint of point k at unit density (a single 1 for
 * radius <= pixelSize), sigma_k its sum, v_k = 0 where the reference skips the point.
 *   Linearisation point: sumC, sumsquareC and cc as the CTF scan above delivers them for (p, o, X, Y) with the handle's
 *       own set c as candidate (same bits); sumref, sumsquareref the particle's.  All widened to double:
 *       F  = ssq Nt - s s,   fe = Nt (ssr ssq - cc cc) + 2 sr s cc - ssr s s - sr sr ssq,
 *       a = dL/ds   = (3 - Nt)/2 (2 sr cc - 2 ssr s) / fe + (Nt/2 - 2) (-2 s) / F,
 *       b = dL/dssq = (3 - Nt)/2 (Nt ssr - sr sr) / fe + (Nt/2 - 2) Nt / F,
 *       g = dL/dcc  = (3 - Nt)/2 (-2 Nt cc + 2 sr s) / fe          (the CTF priors are constants);
 *   G^_P[k] = (a Nt [k = 0] + 2 b conv[k] + g F_p[k] exp(-2 pi i ((kx dx + ky dy) mod N) / N)) K_c[k], dx = -X, dy = -Y,
 *       conv = P^ conj(K_c) the float expression of the convolution; G_P = c2r(G^_P) / Nt by two exact-DFT passes in
 *       double, the Hermitian part taken in the self-conjugate columns;
 *   u_k = v_k sum_{di,dj} s_k[di][dj] G_P[i_k + di][j_k + dj] on the pixels and under the skip rules of the projection,
 *   m = sum_k rho_k u_k,   dL/drho_k = (NormDen / T) (u_k - v_k sigma_k m / T), T summed in double from the same s_k.
 * This is the exact derivative of the double closed form at the device's linearisation point.  The float roundings of
 * the pipeline (the map narrowed to float, float spectra, cc rounded once, the density inside the float numerator of a
 * sphere's weight) are not differentiated.  a s + 2 b ssq + g cc = -1 and sum_k rho_k dL/drho_k = 0 hold analytically.
 * A request whose fe or F is not positive and finite gives what the formulas give (sumsq shows it).
 * points_out[k], over the requests in request order with w_r = weights[r] (1 where weights is null), g_rk the gradient:
 *   sum = sum_r w_r g_rk,  sumsq = sum_r (w_r g_rk)^2,  sumw = sum_r w_r v_rk,  count = sum_r v_rk.
 * A row of grad_out depends on its request alone; the sums depend on the requests and their order alone: the same bits
 * for any batch size, batch boundary and run.  Calling rules and refusals of the CTF scan (2, the request named, the
 * handle usable); also refused: conv outside [0, nCTF), CTF kernels not uploaded, grad_out and points_out both null, a
 * weight that is not finite.  Staging is allocated at the first call (1 when the memory is not there).  Requests go in
 * batches of maxOrientations; one launch of the CTF scan serves up to 16 of them (as that entry does).  Phase records: per
 * batch 0 the projection and 1 the scan's preparation; per launch of the scan one more record of phase 1, the
 * linearisation and a, b, g (iOrientBegin / iOrientEnd the requests of the launch); then per batch 2 the gradient
 * spectrum and the inverse transform, 3 the gather and the fold. */
typedef struct { int particle, orient, conv, shiftX, shiftY; } bioem_hip_grad_request;   /* 20 bytes */
typedef struct { double sum, sumsq, sumw; long long count; } bioem_hip_grad_point;       /* 32 bytes */
int bioem_hip_model_gradient(bioem_hip_handle h, const bioem_hip_grad_request *req, const double *weights /* [n] or NULL */,
                             int n, int ownLists, double *grad_out /* [n][nPts] or NULL */,
                             bioem_hip_grad_point *points_out /* [nPts] or NULL */,
                             bioem_hip_param5 *params_out /* [n] or NULL */,
                             double *coef_out /* [n][4] {a, b, g, m} or NULL */);
/* test hook: a, b, g and G_P from conv spectra, particle spectra and kernels handed in ([n][N][H] (re, im) each, reference
 * layout), the parameters {.., sumC, sumsquareC} and the particles' sums per record; cc is the scan's double sum of the
 * record.  Needs only the handle's parameters. */
int bioem_hip_debug_grad_image(bioem_hip_handle h, const float *specConv, const float *specRef, const float *kernels,
                               const bioem_hip_param5 *params, const float *sumRef, const float *sumsqRef,
                               const int *shiftXY /* [n][2] */, int n, double *gmap_out /* [n][N][N] */,
                               double *coef_out /* [n][3] {a, b, g} */);
/* test hook: u_k of the model's points from maps handed in, at the orientations [o0, o0 + nO) of the shared list */
int bioem_hip_debug_grad_gather(bioem_hip_handle h, const double *gmaps /* [nO][N][N] */, int o0, int nO,
                                double *u_out /* [nO][nPts] */);

/* ---- Summaries of the orientation posterior of every particle (WRITE_PROB_ANGLES; no reference counterpart) ----
 * The [orientations][nMaps] table of bioem_hip_prob_angle stays on the device; this entry reduces it there.  Let
 * F = forAngles, C = ConstAngle of entry (o, p).  Only entries with F > 0 count (entries never compared, or beyond a
 * particle's own list, keep F = 0), and for those l_o = (log F + C) + prior_o in double, prior_o = 0 without logPrior:
 * the key the ANG_PROB lines carry, minus their constant.  Per particle, in two passes (the maximum first, exact and
 * order-free; then every sum relative to it, so no term is ever rescaled):
 *   m      max over o of l_o                         (MIN_PROB = -999999 when count is 0)
 *   omax   the lowest orientation index attaining m  (-1 when count is 0); the index is GLOBAL, with own lists the index
 *          in the particle's list
 *   count  entries with F > 0
 *   hasMoments  1 when the orientations are quaternions, else 0 (Euler angles: Q stays 0, the scalar sums are delivered)
 *   S0 = sum e^(l-m),  S1 = sum e^(l-m) (l-m),  S2 = sum e^(2(l-m))
 *   Q[10]  upper triangle (00 01 02 03 11 12 13 22 23 33) of sum e^(l-m) q q^T, q the entry's quaternion in the
 *          reference's (x, y, z, w) storage, widened to double and divided by its length (q and -q give the same q q^T)
 * All fields are double.  The host derives (bioem_amd/orient_stats.py: derive): logZ = m + log S0, the entropy
 * H = log S0 - S1 / S0, nEff = S0^2 / S2, pTop = 1 / S0, the mean orientation = the eigenvector of Q / S0 of the largest
 * eigenvalue lambda, and the spread 2 acos(sqrt(lambda)) (lambda = E[cos^2(theta / 2)] of the rotation angle to the mean).
 * The orientation range is cut into chunks of 256, summed in orientation order and folded in chunk order; no atomics:
 * the same bits on every run, for any nMaps, any particle range and any position of a particle in the table. */
typedef struct { double m, omax, count, hasMoments, S0, S1, S2, Q[10]; } bioem_hip_orient_sums;   /* 136 bytes */
/* Calling rules of bioem_hip_topk_angles (after finish_run, every handle kind that holds an angle table; a shard sums
 * over the orientations it owns and reports global indices).  logPrior: NULL, or nAngles doubles by global orientation
 * index; refused with own lists.  ownLists = 1: the table rows are positions in the particles' own lists
 * (bioem_hip_compare_own_orientations with WRITE_PROB_ANGLES).  Refused with 2, the reason in bioem_hip_last_error and
 * the handle usable: no WRITE_PROB_ANGLES, a particle range that is empty, reversed or outside [0, nMaps), a null
 * `out`, ownLists without lists, logPrior with own lists.  Buffers are allocated at the first call (1 when the memory is
 * not there).  Phase record: one of phase 2 over the call's kernels, iOrientBegin / iOrientEnd the particle range. */
int bioem_hip_orientation_sums(bioem_hip_handle h, const double *logPrior, int iMapBegin, int iMapEnd, int ownLists,
                               bioem_hip_orient_sums *out /* [iMapEnd - iMapBegin] */);
/* Merge of the shards' sums on the host, no device: sums[s] = [nMaps]; per particle the maximum m with ties to the
 * lowest shard (shards in ascending orientation-block order: the lowest index), every shard's sums scaled by
 * e^(m_s - m) and added in shard order, S1 with the extra term (m_s - m) S0_s e^(m_s - m), S2 scaled by
 * e^(2(m_s - m)); counts add; shards with count 0 are left out.  Returns 2 for nShards < 1 or a null argument. */
int bioem_hip_merge_orient_sums_host(int nShards, int nMaps, const bioem_hip_orient_sums *const *sums,
                                     bioem_hip_orient_sums *out);
/* test hooks: the same kernels on a table handed in, table = [nO][nMaps] entries on the host; angles4 = [nO][4] (NULL
 * or isQuat = 0: no moments); logPrior NULL or nO doubles; out = [nMaps].  The _own variant runs the own-list
 * instantiation: angles4 = the flat lists, offsets[nMaps + 1] into them (list lengths at most nO); a table entry with
 * F > 0 beyond its particle's list does not count. */
int bioem_hip_debug_orient_sums(bioem_hip_handle h, const bioem_hip_prob_angle *table, int nO, int nMaps,
                                const float *angles4, int isQuat, const double *logPrior, bioem_hip_orient_sums *out);
int bioem_hip_debug_orient_sums_own(bioem_hip_handle h, const bioem_hip_prob_angle *table, int nO, int nMaps,
                                    const float *angles4, const long long *offsets, int isQuat,
                                    bioem_hip_orient_sums *out);

/* ---- Occupancy of every orientation over the particles (WRITE_PROB_ANGLES; no reference counterpart) ----
 * The same table reduced along the other axis: which views does the data set hold, and how many particles stand behind
 * each?  With the key l = (log F + C) + prior_o of bioem_hip_orientation_sums and a particle's sums m_p, S0_p, omax_p,
 * count_p (for shards: the MERGED sums, which is why the host hands them in), entry (o, p) with F > 0 of a particle with
 * count_p > 0 and S0_p > 0 carries the posterior weight
 *   w(o, p) = e^(l - m_p) / S0_p          (the device multiplies by 1 / S0_p, formed once per particle)
 * -- the key is the expression the sums evaluated, so a particle's arg-max entry gives 1 / S0_p exactly, the pTop of
 * --OrientStats.  Per orientation row, over the particles [iMapBegin, iMapEnd):
 *   occ    sum of w                         (over all rows it adds up to the particles counted)
 *   occ2   sum of w^2                       (occ^2 / occ2: the effective number of particles behind the view)
 *   wmax   the largest w of the row         (0 for an empty row)
 *   pmax   the lowest particle index attaining wmax; the index in the table, -1 for an empty row
 *   count  particles of the range that count and have F > 0 in this row
 *   hard   particles of the range that count and whose omax_p is this row's global index (integer compare)
 * All fields are double.  One wave per row, lane j takes the particles iMapBegin + j, + 64, ... in order, the lanes are
 * folded by a fixed butterfly; no atomics: the same bits on every run, and a row's bits depend on its entries of the
 * range, its prior and the particles' normalisers only -- not on nMaps, iMapBegin (pmax moves with it) or the row's
 * position in the table.  A finite prior as low as -1e6 gives w = 0, never NaN. */
typedef struct { double occ, occ2, wmax, pmax, count, hard; } bioem_hip_orient_occ;   /* 48 bytes */
/* Calling rules of bioem_hip_orientation_sums (after finish_run, every handle kind that holds an angle table; logPrior
 * NULL or nAngles doubles by global orientation index).  sums = [iMapEnd - iMapBegin] on the host, entry i the sums of
 * particle iMapBegin + i.  out = one entry per orientation the handle owns: a shard writes its [o0, o1) block in row
 * order, and the shards' blocks concatenated in block order are the unsharded result.  Refused with 2, the reason in
 * bioem_hip_last_error and the handle usable: no WRITE_PROB_ANGLES, a particle range that is empty, reversed or outside
 * [0, nMaps), a null `sums` or `out`, a handle with per-particle orientation lists (its rows are list positions, not
 * shared orientations).  Buffers are allocated at the first call (1 when the memory is not there).  Phase record: one of
 * phase 2 over the call's kernel, iOrientBegin / iOrientEnd the particle range. */
int bioem_hip_orientation_occupancy(bioem_hip_handle h, const double *logPrior, const bioem_hip_orient_sums *sums,
                                    int iMapBegin, int iMapEnd, bioem_hip_orient_occ *out /* [orientations owned] */);
/* test hook: the same kernel on a table handed in, table = [nO][nMaps] entries on the host; logPrior NULL or nO doubles
 * by row; sums = [p1 - p0] for the particles [p0, p1); o0 = the global index of row 0 (what omax is compared with);
 * out = [nO]. */
int bioem_hip_debug_orient_occupancy(bioem_hip_handle h, const bioem_hip_prob_angle *table, int nO, int nMaps,
                                     const double *logPrior, const bioem_hip_orient_sums *sums, int p0, int p1, int o0,
                                     bioem_hip_orient_occ *out);

/* ---- Aligned averages of the particles of a view (no reference counterpart) ----
 * Particle p has the record (c, X, Y, norm, mu) = (max_prob_conv, max_prob_cent_x, max_prob_cent_y, max_prob_norm,
 * max_prob_mu) (max_prob_orient is not read), a weight w_p >= 0 (weights == NULL: 1) and a group groupOf[p] in
 * [0, nGroups), or -1 for "left out".  With R_p the particle's spectrum as the handle holds it
 * (bioem_hip_debug_particles), K_c the uploaded CTF kernel and tw[j] = exp(+2 pi i j / N), everything in double, [N][H]:
 *   A_p[k1][k2] = (R_p[k1][k2] - mu_p N^2 [k1 = k2 = 0]) tw[(k1 X_p + k2 Y_p) mod N]
 *   K~_c = K_c; in the columns that are their own Hermitian partner (k2 = 0 and, N even, k2 = N / 2) its Hermitian part
 *          (K_c[k1][k2] + conj(K_c[(N - k1) mod N][k2])) / 2: a particle is a real image, so there its spectrum carries
 *          only that part of P conj(K_c) (the convention of M in the ring sums above), and P^ comes out Hermitian as P is
 *   num_g[k] = sum_p (w_p norm_p) K~_c[k] A_p[k]            (re, im)
 *   den_g[k] = sum_p (w_p norm_p^2) |K~_c[k]|^2
 * over the members of g in ascending p, count_g and sumw_g = sum w_p: the normal equations of the model of the ring pass,
 * R ~ norm P conj(K~_c) tw[-(k1 X + k2 Y) mod N] + mu N^2 delta, for the projection P of the view.  The estimate is
 *   P^_g[k] = num_g[k] / (den_g[k] + tau_g),  tau_g = wiener * mean_k den_g[k],  0 where the denominator is 0.
 * One lane owns a (group, coefficient) and adds its members one after the other; accumulators of a group that spans
 * batches of maxOrientations particles continue in device memory.  No atomics: the bits of a group depend on its members
 * alone, not on the batch size, the other groups of the call, the range [g0, g1) or the run.
 * Calling rules as bioem_hip_best_match_rings (outside a run, every handle kind, buffers allocated at the first call: 1
 * when the memory is not there).  Refusals (2, the particle or group named, handle usable): a null argument, an empty or
 * reversed group range, a group >= nGroups or < -1, a negative or non-finite weight, max_prob_conv outside [0, nCTF), a
 * displacement of N pixels or more, groupOrient outside the orientation list, a negative wiener, and particles, CTF
 * kernels or (bioem_hip_view_averages) model or orientations not uploaded.  Records of particles left out are not read.
 * Phase records: phase 2 per particle batch of the accumulation, phase 0 per chunk of projections. */
/* records, weights, groupOf run over all nMaps particles; out for the groups [g0, g1): num [g][N][H] (re, im) doubles,
 * den [g][N][H] doubles, stats [g] {count, sumw}.  Needs the particles and the CTF kernels. */
int bioem_hip_view_sums(bioem_hip_handle h, const bioem_hip_prob_map *records, const double *weights, const int *groupOf,
                        int nGroups, int g0, int g1, double *num_out, double *den_out, double *stats_out);
/* The chain: P^_g as above; groupOrient[g] indexes the shared orientation list, -1 = no projection (that group's rings and
 * projection map are zero).  rings_out [g][nRings]: the sums of bioem_hip_best_match_rings with R = P^_g (rounded to float)
 * and M = P_o, the projection spectrum of groupOrient[g]: powParticle is the power of P^, powModel of P_o.  avg_maps_out /
 * proj_maps_out (each may be NULL): [g][N][N] float, c2r(P^) / N^2 and c2r(P_o) / N^2 in the convention of
 * bioem_hip_render_best_maps.  Groups go through in chunks of at most maxOrientations. */
int bioem_hip_view_averages(bioem_hip_handle h, const bioem_hip_prob_map *records, const double *weights, const int *groupOf,
                            const int *groupOrient, int nGroups, double wiener, int g0, int g1,
                            bioem_hip_ring_sums *rings_out, float *avg_maps_out, float *proj_maps_out);
/* test hook: the accumulation on n spectra handed in (specR [n][N][H] (re, im), reference layout) for all nGroups groups;
 * records, weights, groupOf run over the n spectra; needs the CTF kernels only */
int bioem_hip_debug_view_sums(bioem_hip_handle h, const float *specR, const bioem_hip_prob_map *records, const double *weights,
                              const int *groupOf, int n, int nGroups, double *num_out, double *den_out, double *stats_out);

/* ---- The 3D density the aligned view sums support (no reference counterpart) ----
 * The views' sums num_g, den_g above are put together by the Fourier-slice theorem under the orientations the run
 * assigned.  o = (N + 1) / 2 is the pixel the projection puts the model's origin on, M = (N - 1) / 2, a centred frequency
 * kappa stands for index kappa mod N, everything in double:
 *   S_g(a, b) = num_g[a mod N][b] tw[(o (a + b)) mod N] for b >= 0, conj(S_g(-a, -b)) for b < 0; D_g(a, b) likewise from
 *               den_g (real); both 0 outside |a|, |b| <= M (N even: the Nyquist row and column are left out)
 *   R_g       = the float rotation matrix the projection builds for the orientation, widened
 *   q_i       = (R[i][0] k0 + R[i][1] k1) + R[i][2] k2 for the stored voxel (k0, k1, k2): index i <= N / 2 stands for
 *               kappa = i, a larger one for i - N, on axes 0 and 1; 0 <= k2 < H
 *   numV[k]  += wz w_t S_g(tap), denV[k] += wz w_t D_g(tap) with wz = max(0, 1 - |q2|) and the taps (a, b), (a + 1, b),
 *               (a, b + 1), (a + 1, b + 1) about a = floor(q0), b = floor(q1) of weights (1 - f0)(1 - f1), f0 (1 - f1),
 *               (1 - f0) f1, f0 f1; views in ascending order, taps in this order, weight = wz * (w_t) rounded as written
 *   V^[k]     = numV / (denV + tau) tw[(-o (k0 + k1 + k2)) mod N], tau = wiener * mean_k denV[k], 0 where denV + tau is 0
 *   vol       = c2r3(V^) / N^3: the inverse along axis 0, then every plane through the passes of the gradient image;
 *               with BIOEM_HIP_RECON_CORRECT divided by prod_d sinc^2(pi (x_d - o) / N); rounded to float.  The origin
 *               of the volume is voxel (o, o, o), axes as the model's (x, y, z).
 * A voxel is owned by one lane that adds its views one after the other: no atomics, the bits of a voxel depend on the
 * views alone -- not on the chunks of groups, the other voxels, BIOEM_HIP_RECON_NO_CULL or the run.
 * Outputs, each may be NULL but not all: vol_out [N][N][N] float, spec_out [N][N][H] (re, im) doubles = V^, den_out /
 * denV_out [N][N][H] doubles, numV_out [N][N][H] (re, im) doubles.  The volume buffers (about 40 N^2 H bytes) are allocated
 * at the first call: 1 when the memory is not there.  Phase records: phase 2 per particle batch of the accumulation, phase
 * 1 per chunk of views inserted, phase 0 with iOrientBegin 0 over the estimate and with iOrientBegin 1 over the inverse. */
#define BIOEM_HIP_RECON_CORRECT 1 /* divide the volume by the transform of the interpolation kernel */
#define BIOEM_HIP_RECON_NO_CULL 2 /* test switch: no view is left out for a whole brick of voxels (same bits) */
/* The chain: the accumulation of bioem_hip_view_sums in chunks of at most maxOrientations groups, each chunk inserted while
 * it is on the device.  groupOrient[g] indexes the shared orientation list; groups with groupOrient[g] = -1 or without
 * members are skipped.  stats_out {views used, particles used, sum of their weights, tau}.  Calling rules, handle kinds and
 * refusals as bioem_hip_view_averages (the model is not needed; a negative wiener is refused as there), and refused with 2 as
 * well: all outputs NULL, unknown flag bits, a non-finite wiener.  The views are numbered densely before they are chunked:
 * nothing is accumulated for a skipped group. */
int bioem_hip_reconstruct(bioem_hip_handle h, const bioem_hip_prob_map *records, const double *weights, const int *groupOf,
                          const int *groupOrient, int nGroups, double wiener, int flags, float *vol_out, double *spec_out,
                          double *den_out, double *stats_out);
/* test hook: the kernels alone on nViews sums handed in (num [v][N][H] (re, im), den [v][N][H]) under the orientations
 * angles4 [v][4] (quaternions, or Euler angles with isQuat 0); needs no particles, model or CTF.  Refused with 2, the view
 * named: a null input, all outputs NULL, unknown flag bits, nViews < 1, a non-finite orientation, a negative or non-finite
 * wiener. */
int bioem_hip_debug_reconstruct(bioem_hip_handle h, const double *num, const double *den, const float *angles4, int isQuat,
                                int nViews, double wiener, int flags, float *vol_out, double *spec_out, double *numV_out,
                                double *denV_out);

/* ---- Posterior-weighted view sums and their density (no reference counterpart) ----
 * The sums above align a particle by one record at weight 1.  Here a *member* r is one (particle p, group g, CTF set c)
 * and carries a table a_r[i][j] of doubles over the cells of a shift list X_0 ... X_{nd - 1} handed in -- cell [i][j] is
 * the shift (X_i, X_j), cent_x first, as in bioem_hip_window_posterior -- and three scalars s2_r, b_r, mass_r.  With R_p,
 * K~_c and tw as above, everything in double:
 *   W_r[k1][k2] = sum_i sum_j a_r[i][j] tw[(k1 X_i + k2 X_j) mod N]
 *   num_g[k]   += K~_c[k] (R_p[k] W_r[k] - [k = 0] b_r N^2)
 *   den_g[k]   += s2_r |K~_c[k]|^2
 *   stats_g     = { number of members, sum mass_r }
 * the hard-assignment sum averaged over the cells, each cell with its own least-squares norm and mu under the weight w
 * of the cell: a = w norm, s2 = sum_cells w norm^2, b = sum_cells w norm mu, mass = sum_cells w.  A member whose table
 * has one non-zero cell a = w norm at (X, Y), with s2 = a norm and b = a mu, is a member of the hard sums; a may have
 * either sign.  This is a profile-likelihood convention, not the exact M-step: the posterior the reference integrates
 * marginalises norm and mu analytically, while each cell enters here with its arg-max norm and mu.
 * Summation order: W is separable, U_r[i][k2] = sum_j a_r[i][j] tw[(k2 X_j) mod N] with j ascending, then W_r[k1][k2] =
 * sum_i tw[(k1 X_i) mod N] U_r[i][k2] with i ascending; twiddle indices are reduced in integers, every product and sum
 * rounds once.  The table tw of these entries holds 0 and +-1 exactly where 4 j is a multiple of N (the correctly rounded
 * values), so tables over whole shifts of a quarter image multiply exactly.  A lane owns its (group, coefficient) and
 * adds the group's members in ascending (particle, position in the member list); accumulators of a group that spans particle batches continue in device memory.  No atomics: the bits of a
 * group depend on its own members alone -- not on the batch size, the batch boundaries, the other groups, the range
 * [g0, g1) or the run.  Every handle kind gives the same bytes.
 * Calling rules and outputs as for the hard sums.  Refused with 2, the member or group named and the handle usable: a
 * null argument or n < 1, nd < 1 or nd > N, a shift of N pixels or more, an empty or reversed group range, a group outside
 * [0, nGroups) that is not -1 (-1 leaves the member out; nothing else of it is read), particle or conv out of range, a
 * non-finite cell, s2, b or mass, a negative s2 or mass, and CTF kernels or particles not uploaded.  Phase records per
 * launch of at most maxOrientations members, all with iConvEnd = nd (which tells them from the chain's own records):
 * phase 0 over the column pass, phase 1 over the row pass, phase 2 over the accumulation, iOrientBegin / iOrientEnd the
 * particle batch. */
typedef struct { int particle, group, conv, pad; double s2, b, mass; } bioem_hip_soft_member;   /* 40 bytes */
/* members [n], cells [n][nd][nd], shifts [nd]; out for the groups [g0, g1) as the hard sums deliver them.  Needs the
 * particles and the CTF kernels. */
int bioem_hip_view_sums_soft(bioem_hip_handle h, const bioem_hip_soft_member *members, const double *cells, int n,
                             const int *shifts, int nd, int nGroups, int g0, int g1, double *num_out, double *den_out,
                             double *stats_out);
/* test hook: the same kernels on nSpec spectra handed in (specR [nSpec][N][H] (re, im), reference layout) for all nGroups
 * groups; `particle` indexes specR; needs the CTF kernels only */
int bioem_hip_debug_view_sums_soft(bioem_hip_handle h, const float *specR, int nSpec, const bioem_hip_soft_member *members,
                                   const double *cells, int n, const int *shifts, int nd, int nGroups, double *num_out,
                                   double *den_out, double *stats_out);
/* The chain of the hard reconstruction with this accumulation in place of the hard one: groups with groupOrient[g] = -1 or
 * without members are skipped, the others numbered densely, accumulated chunk by chunk and inserted while on the device.
 * stats_out {views used, members used, sum of their mass, tau}.  Outputs, flags and the further refusals (all outputs
 * NULL, unknown flag bits, a negative or non-finite wiener, groupOrient outside the orientation list, orientations not
 * uploaded) as there. */
int bioem_hip_reconstruct_soft(bioem_hip_handle h, const bioem_hip_soft_member *members, const double *cells, int n,
                               const int *shifts, int nd, const int *groupOrient, int nGroups, double wiener, int flags,
                               float *vol_out, double *spec_out, double *den_out, double *stats_out);

/* ---- A volume as the model: projections as central slices of its spectrum (no reference counterpart) ----
 * A handle holds either a point model (bioem_hip_upload_model) or a volume model; uploading one replaces the other.  With
 * N, H, o, M, tw as above, the padding P = pad in {1, 2}, PN = P N, PH = PN / 2 + 1, M_P = (PN - 1) / 2, axes the model's
 * (x, y, z), the volume's origin at voxel (o, o, o), everything in double:
 *   spec[k]  = sum_x vol[x] exp(-2 pi i k.x / PN) over the N^3 box in the first octant of the PN^3 box, [PN][PN][PH]
 *              (re, im), un-centred: bioem_hip_reconstruct's spec_out at pad = 1
 *   C(k')    = spec[k' mod PN] exp(+2 pi i (k'0 + k'1 + k'2) o / PN) exp(+2 pi i k'.centre / PN): the spectrum about the
 *              origin voxel of the density moved by -centre pixels (NULL: 0), what the handle keeps ([PN][PN][PH] double2,
 *              wrapped indices on axes 0 and 1).  NormDen := Re C(0).
 *   slice    : stored coefficient (a mod N, b), |a| <= N / 2, 0 <= b < H, under the orientation's float matrix R, widened:
 *              0 + 0i where a^2 + b^2 > M^2; else k_j = (a R[0][j]) + (b R[1][j]), k' = P k, trilinear about floor(k'):
 *              the taps t = 4 d0 + 2 d1 + d2 ascending with weights ((w0 w1) w2), w_d = d_d ? f_d : 1 - f_d; a tap with a
 *              negative third index reads conj C(-k'), a tap outside |k'_d| <= M_P (or a NaN coordinate) adds nothing; the
 *              sum times tw[(-o (a + b) + shiftX a + shiftY b) mod N], rounded once to float2 where the r2c of a point
 *              model's projection stores its result.  No NormDen / tempden factor: nothing is skipped.
 * The slice moves the origin to the pixel floor(x / px + N / 2 + 0.5) - shift of the real-space projection.  Every run
 * entry, own-list pass and analysis entry projects through it.  A lane owns its coefficient: the same bits for any batch
 * size, position in the list, handle kind and run.  The entries that need points -- bioem_hip_model_gradient,
 * bioem_hip_debug_grad_gather, bioem_hip_debug_projection_maps, bioem_hip_debug_stamps -- return 2, "the model is a volume".
 * Refused with 2, the cause named and the handle usable with the model it had: pad outside {1, 2}, a null array, unknown
 * flag bits, a non-finite value in spec, vol or centre, Re C(0) <= 0.  1: device memory (C takes 16 PN^2 PH bytes, 722 MB
 * at 224^2 with pad = 2; the volume entry twice that while it runs). */
#define BIOEM_HIP_VOLUME_PRECORRECT 1 /* divide vol by prod_d sinc^2(pi (x_d - o) / PN), the transform of the trilinear kernel */
int bioem_hip_upload_model_spectrum(bioem_hip_handle h, const double *spec, int pad, const double *centre, int shiftX,
                                    int shiftY);
/* vol [N][N][N]; the spectrum is formed on the device by three passes of direct summation (a lane owns its output, fixed
 * order, no atomics), then handled as above */
int bioem_hip_upload_model_volume(bioem_hip_handle h, const float *vol, int pad, int flags, const double *centre, int shiftX,
                                  int shiftY);
/* test hook: the slice kernel alone on n orientations handed in (angles4 [n][4]); out [n][N][H] (re, im) doubles, the
 * slices as they stand before the rounding to float.  Refused with 2: a null argument, n < 1, the model is not a volume. */
int bioem_hip_debug_slices(bioem_hip_handle h, const float *angles4, int n, int isQuat, double *out);

/* ---- Density gradient of the log posterior per voxel of a volume model (no reference counterpart) ----
 * For request (p, o, c, X, Y) with weight w_r the derivative of the log posterior of that match with respect to the array
 * handed to bioem_hip_upload_model_volume, at a fixed centre.  The slice is exactly linear in the stored spectrum C (no
 * NormDen / tempden factor, no skip rule), so the adjoint is: the front half of bioem_hip_model_gradient up to G^_P, the
 * transpose of the slice, the transpose of the upload's passes.  Conventions of the volume model above.
 *   Gamma    = G^_P, but Gamma[a, 0] = (G^_P[a, 0] + conj G^_P[-a, 0]) / 2 in the self-conjugate column;
 *   Y[a, b]  = ((w_r w_b) / N^2) (Gamma[a, b] conj(tw[e(a, b)])), w_b = 1 for b = 0, else 2, e the slice's twiddle index,
 *              used only where a^2 + b^2 <= M^2;
 *   A[s]     = sum wt (neg ? conj Y[a, b] : Y[a, b]) over every request, coefficient and tap of the slice that lands on the
 *              stored voxel s of [PN][PN][PH], under every drop rule of the slice, wt its ((w0 w1) w2); requests ascending,
 *              the target +s before -s, coefficients in ascending (a, b).  dL = sum_s Re(conj(A[s]) dC[s]);
 *   A_spec[k]= A[k] conj(phi[k]), phi the product of the four unit factors that centre the spectrum;
 *   gv[x]    = sum_{stored k} Re(A_spec[k] twP[(k.x) mod PN]) over the N^3 box, the stored entries as they are;
 *   gvol[x]  = gv[x] / prod_d sinc^2(pi (x_d - o) / PN) where the model was uploaded as a volume with precorrection.
 * vol_out [N][N][N] = gvol; spec_out [PN][PN][PH] (re, im) = A, the gradient with respect to C for a model that came in
 * through bioem_hip_upload_model_spectrum (such a model delivers vol_out without the sinc^2 division); coef_out [n][4] =
 * {a, b, g, <C, A_r>}, the last through the adjoint identity as sum (w_b / N^2) Re(conj(Gamma_r) slice_r) on the double
 * slice of the request (w_r left out, as m of the point entry); params_out [n] the linearisation points; stats_out [3] =
 * {n, sum_r w_r, the requests whose a, b or g is not finite}.  Any output but not both of vol_out and spec_out may be NULL.
 * A stays on the device across the batches (16 PN^2 PH bytes beside C).  The back-insertion is a gather without atomics: a
 * voxel's bits depend on the requests in request order alone, the same for any batch size, batch boundary and run.
 * Calling rules, batches, scan launches and refusals of bioem_hip_model_gradient; also refused with 2, the request named
 * and the handle usable: the model is a point model, vol_out and spec_out both null, an orientation whose matrix has rows
 * 0 and 1 rank-deficient, or shrinks so far that the search for the coefficients of a voxel would pass a half-width of 4
 * (a rotation has sqrt(3) / pad; quaternions of length 0.85 to 1.07 stay below 3.9 at pad 1; the matrix of a quaternion
 * of length sqrt(1 / 2) is singular).  Phase records as there through phase 2 (here the gradient
 * spectrum, Y and <C, A_r>); 3 the back-insertion per batch, and one more record of phase 3 with the empty request range
 * [n, n): the passes back to the volume. */
int bioem_hip_volume_gradient(bioem_hip_handle h, const bioem_hip_grad_request *req, const double *weights /* [n] or NULL */,
                              int n, int ownLists, double *vol_out /* [N][N][N] or NULL */,
                              double *spec_out /* [PN][PN][PH][2] or NULL */, double *coef_out /* [n][4] or NULL */,
                              bioem_hip_param5 *params_out /* [n] or NULL */, double *stats_out /* [3] or NULL */);
/* test hook: Y and the back-insertion alone on the spectra gamma [n][N][H] (re, im) handed in as Gamma, under the
 * orientations angles4 [n][4]: Y = weights[i] (Gamma conj(tw[e])) (NULL: 1), without w_b and 1 / N^2; cull: whether
 * views are tested against a brick of voxels first (the same bits either way); the views go through in chunks of
 * maxOrientations into a buffer poisoned with NaNs.  spec_out [PN][PN][PH] (re, im) = A. */
int bioem_hip_debug_volume_backproject(bioem_hip_handle h, const float *angles4, int n, int isQuat, const double *gamma,
                                       const double *weights, int cull, double *spec_out);
/* test hook: the passes from A (spec_in [PN][PN][PH] (re, im)) to gvol (vol_out [N][N][N]) alone */
int bioem_hip_debug_volume_adjoint(bioem_hip_handle h, const double *spec_in, double *vol_out);

/* ---- Pose gradient of the log posterior for a volume model (no reference counterpart) ----
 * For request (p, o, c, X, Y) the derivative of the log posterior of that match with respect to the six entries of rows 0
 * and 1 of the orientation's matrix R (the float matrix widened to double) and to the handle's model shifts shiftX, shiftY
 * taken as real numbers.  With Y[a, b] of the volume gradient at weight 1, q = P (a R[0,:] + b R[1,:]), the cell c =
 * floor(q), its weights and the eight taps v_t under every drop rule of the slice, per coefficient of the disc:
 *   s   = sum_t ((w0 w1) w2) v_t, the slice's tap sum before its twiddle;
 *   D_0 = sum_t sigma_0(t) (w1 w2) v_t, D_1 with (w0 w2), D_2 with (w0 w1), sigma_d(t) = +1 where tap t has d_d = 1, else
 *         -1: the gradient of the trilinear interpolant in the cell (at f_d = 0 the right-hand derivative);
 *   J[i][j] = sum P x_i Re(conj(Y) D_j), x_0 = a, x_1 = b: d log P / d R[i][j];
 *   T[i]    = sum (2 pi x_i / N) Re(conj(Y) i s): d log P / d shiftX, d shiftY;
 *   dot     = sum Re(conj(Y) s) = <C, A_r> of the volume gradient (to rounding, not to the bit).
 * pose_out [n][18] = {J[0][0..2], J[1][0..2], T[0], T[1], dot, R[0..8]}; coef_out [n][4] = {a, b, g, dot}; params_out [n]
 * the linearisation points; the last two may be NULL.  Double throughout, no atomics: a row's bits depend on its request
 * alone, the same for any batch, list, position and run.  Calling rules, batches, scan launches and refusals of
 * bioem_hip_volume_gradient (no cap on the matrix: A and the search of the back-insertion are not needed); also refused
 * with 2, the request named and the handle usable: the model is a point model, pose_out null, an orientation whose matrix
 * has an entry that is not finite.  Phase records as there through phase 2 (the gradient spectrum and Y); 3 the nine sums
 * per batch. */
int bioem_hip_pose_gradient(bioem_hip_handle h, const bioem_hip_grad_request *req, int n, int ownLists,
                            double *pose_out /* [n][18] */, double *coef_out /* [n][4] or NULL */,
                            bioem_hip_param5 *params_out /* [n] or NULL */);
/* test hook: the two kernels alone on the spectra gamma [n][N][H] (re, im) handed in as Gamma under the orientations
 * angles4 [n][4]: Y = weights[i] (Gamma conj(tw[e])) (NULL: 1), without w_b and 1 / N^2, 0 outside the disc; the views go
 * through in chunks of maxOrientations.  pose_out [n][18] as above. */
int bioem_hip_debug_pose_sums(bioem_hip_handle h, const float *angles4, int n, int isQuat, const double *gamma,
                              const double *weights, double *pose_out);

/* ---- CTF gradient and curvature of the log posterior per match (no reference counterpart) ----
 * For request (p, o, c, X, Y) the first and second derivatives of the log posterior of that match with respect to the
 * triple theta = (amp, pha, env) of CTF set c, CTF mode only.  The host's kernel is then the closed form
 *   k(s; theta) = exp(-env s / 2) (cos(pha s / 2) + rho sin(pha s / 2)),  rho = sqrt(1 - amp^2) / amp,  k(0) = 1,
 * of the radial variable s of a stored element: the float of the host's own expression at pixelSize (a table made on the
 * host, uploaded once per handle and pixel size), widened to double.  With P the projection's spectrum, Z = w conj(F) tw,
 * D_t = dk / dtheta_t, D_tu the second derivatives and Nt = N N, twenty sums over the stored elements, in double:
 *   ss0 = sum w |P|^2 k^2, cc0 = sum Re(P Z) k, U_t = sum w |P|^2 k D_t, V_t = sum Re(P Z) D_t,
 *   UU_tu = sum w |P|^2 (D_t D_u + k D_tu), VV_tu = sum Re(P Z) D_tu        (tu = aa, ap, ae, pp, pe, ee)
 * and, with ss_t = 2 U_t / Nt, cc_t = V_t / Nt, ss_tu = 2 UU_tu / Nt, cc_tu = VV_tu / Nt, b and g of the other gradient
 * entries (bit for bit) and L_bb, L_bg, L_gg the second derivatives of the same closed form with respect to (sumsquareC, cc)
 * at the device's float linearisation point:
 *   gData_t  = b ss_t + g cc_t
 *   HData_tu = L_bb ss_t ss_u + L_bg (ss_t cc_u + ss_u cc_t) + L_gg cc_t cc_u + b ss_tu + g cc_tu.
 * sumC does not depend on theta (k(0) = 1).  The prior's part is reported apart, the derivatives of -prior with the signs
 * of the reference's expression: gPrior = ((amp - c_a) / s_a^2, (pha - c_d) / s_d^2, -env / s_b^2), HPrior = (1 / s_a^2,
 * 1 / s_d^2, -1 / s_b^2) -- a caller may leave them out.
 * rows_out [n][38] = {theta[3], the sums in the order above [20], gData[3], gPrior[3], HData[6] (aa, ap, ae, pp, pe, ee),
 * HPrior[3] (its diagonal)}; coef_out [n][4] = {a, b, g, 0}; params_out [n] the linearisation points; the last two may be
 * NULL.  No atomics: a row's bits depend on its request alone, the same for any batch, list, position and run.  Point and
 * volume models alike.  Calling rules, batches, scan launches and request refusals of bioem_hip_model_gradient; also refused
 * with 2, the request named where there is one and the handle usable: a handle in PSF mode, pixelSize not finite or not
 * positive, rows_out null, a request whose set has amp <= 1e-10 or amp >= 1.  Phase records as there through phase 1; 2 the
 * sums of a batch; 3 its rows. */
int bioem_hip_ctf_gradient(bioem_hip_handle h, const bioem_hip_grad_request *req, int n, int ownLists, float pixelSize,
                           double *rows_out /* [n][38] */, double *coef_out /* [n][4] or NULL */,
                           bioem_hip_param5 *params_out /* [n] or NULL */);
/* test hook: the three kernels alone on n pairs of spectra handed in (specP, specRef [n][N][H] (re, im)), the shifts
 * shiftXY [n][2] and a triple per record, triples [n][3].  A record's row is finished at the linearisation point its
 * spectra imply: sumC = Re specP[0][0], sumsquareC = (float) (ss0 / Nt), cc = (float) (cc0 / Nt), the particle's sum
 * Re specRef[0][0] and its sum of squares (float) (sum w |specRef|^2 / Nt).  rows_out [n][38] as above; derivs_out
 * [n][N H][10] or NULL: k, D_a, D_p, D_e, D_aa, D_ap, D_ae, D_pp, D_pe, D_ee per position of the walk order (rows; inside
 * a row the columns 1 ... , then 0, then N / 2 for even N), the device's own values.  Records go through in chunks of
 * maxOrientations. */
int bioem_hip_debug_ctf_gradient(bioem_hip_handle h, const float *specP, const float *specRef, const int *shiftXY,
                                 const float *triples, int n, float pixelSize, double *rows_out, double *derivs_out);

#ifdef __cplusplus
}
#endif
#endif
