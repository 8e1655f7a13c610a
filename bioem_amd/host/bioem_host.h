// bioem_host.h -- C++ host layer of the MI355X BioEM engine: the parts of the reference's driver that
// sit on either side of the device plugin for the compare path (parameter file, orientation lists/grids,
// CTF/PSF kernels, model and particle readers, the run() loop, the Output_Probabilities writer), shaped
// after the reference's classes so that a reference user finds the same hooks:
//
//   InputParams      <-> bioem_param         (/root/reference/include/param.h:49-153)
//   Model            <-> bioem_model         (/root/reference/include/model.h:20-57)
//   ParticleStack    <-> bioem_RefMap        (/root/reference/include/map.h:26-88)
//   Driver           <-> bioem / bioem_cuda  (/root/reference/include/bioem.h:24-99)
//
// All heavy lifting is delegated to libbioem_hip.so through include/bioem_hip.h.  Errors follow the
// reference's behaviour: print "Error - ..." and exit(1) (defs.h:18-26).
#ifndef BIOEM_HOST_H
#define BIOEM_HOST_H

#include <cstdio>
#include <string>
#include <vector>

#include "bioem_hip.h"

namespace bioem_host
{

[[noreturn]] void fatal(const char *fmt, ...);
void warn(const char *fmt, ...);

// a map entry some run compared: no longer as the initialisation of a probability block left it
inline bool has_record(const bioem_hip_prob_map &r) { return !(r.Total == 0.0 && r.Constoadd == -999999.); }

struct InputParams
{
  // parameter-file content (param.cpp:64-627)
  float pixelSize = 0;
  int N = 0;
  int angleGridPointsAlpha = 0, angleGridPointsBeta = 0, GridPointsQuatern = -1;
  bool doquater = false, usepsf = false, writeCTF = false, nocentermass = false, notnormmap = false;
  bool yespriorAngles = false, ignorePDB = false, printrotmod = false, doaaradius = true;
  float elecwavel = 0.019866f;
  float priorMod = 1.f;
  int shiftX = 0, shiftY = 0;
  float startBfactor = 0, endBfactor = 0, startDefocus = 0, endDefocus = 0;
  float startGridEnvelop = 0, endGridEnvelop = 0, startGridCTF_phase = 0, endGridCTF_phase = 0;
  float startGridCTF_amp = 0, endGridCTF_amp = 0;
  int numberGridPointsEnvelop = 0, numberGridPointsCTF_phase = 0, numberGridPointsCTF_amp = 0;
  float gridEnvelop = 0, gridCTF_phase = 0, gridCTF_amp = 0;
  bool notuniformangles = false; // set by --ReadOrientation (bioem.cpp:162)
  bioem_hip_param_device pd{};

  // derived
  std::vector<float> angles; // [n][4] {pos0,pos1,pos2,quat4}
  std::vector<float> angprior;
  int nTotGridAngles = 0;
  float voluang = 0;
  int nTotCTFs = 0;
  std::vector<float> refCTF;   // [nCTF][N][H][2]
  std::vector<float> ctfParam; // [nCTF][3]

  void readParameters(const char *file);          // param.cpp:64-627
  void calculateGridsParam(const char *anglefile); // param.cpp:988-1334
  void calculateRefCTF();                          // param.cpp:1336-1620 (PSF r2c runs through `r2c`)
  // r2c hook used only in PSF mode; supplied by the driver (device transform)
  void (*r2c)(void *ctx, int N, const float *in, float *out) = nullptr;
  void *r2c_ctx = nullptr;
};

// the pure functions (also exported through the C ABI in capi.cpp for tests and bench.py)
int ctf_kernels(int N, float pixelSize, bool usepsf, float startAmp, float endAmp, int nAmp, float startPhase,
                float endPhase, int nPhase, float startEnv, float endEnv, int nEnv, float *refCTF, float *ctfParam,
                float *steps, void (*r2c)(void *, int, const float *, float *), void *ctx);
// the kernels out[G][N][H][2] of G triples {amp, phase, env} handed in: per triple the expression of ctf_kernels, so a
// triple that is a grid point carries the grid kernel's bits
void ctf_kernel_list(int N, float pixelSize, bool usepsf, const float *triples, int G, float *out,
                     void (*r2c)(void *, int, const float *, float *), void *ctx);
// a quaternion list in the format --ReadOrientation reads (header line with the count, four 12-character columns)
std::vector<float> read_quaternion_list(const char *file);
float volume_element(float voluang, int gridSpaceCenter, int maxDisplaceCenter, float pixelSize, int nAmp,
                     float gridEnvelop, float gridPhase, float sigB, float sigDef, float sigAmp);

// MRC header fields used by the readers (include/mrc.h of the reference): endianness guessed from header range
// violations, data start at 1024 + nsymbt bytes
struct MrcHeader
{
  int nc, nr, ns, mode, nsymbt, swap;
};
MrcHeader mrc_read_header(const char *file);
unsigned int mrc_bswap32(unsigned int v);

// the BEST_* file of --PrintBestCalMap (bioem_param::forprintBest, param.cpp:629-907): one best-match record by hand
struct BestParams
{
  float pixelSize = 0;
  int N = 0;
  float angle[4] = {0, 0, 0, 0}; // alpha beta gamma, or q1 q2 q3 q4 with USE_QUATERNIONS
  bool doquater = false, usepsf = false, withnoise = false, doaaradius = true, printrotmod = false;
  float elecwavel = 0.019866f;
  float amp = 0, phase = 0, env = 0; // the one CTF / PSF kernel; phase: the defocus already converted
  int ddx = 0, ddy = 0, shiftX = 0, shiftY = 0;
  float norm = 0, offset = 0, stnoise = 1;
};
// bestmap.cpp: empty string, or the text of the error (the CLI ends with it like the reference does)
std::string read_best_parameters(const char *file, BestParams &b);
// the BESTMAP text of bioem.cpp:2041-2079 for the unshifted map v[N][N]; mapOnly: no MAPddx lines (WITHNOISE)
bool write_bestmap_text(const char *file, const float *v, int N, int ddx, int ddy, bool mapOnly);

// --ProbCTF: the text file of a CTF table tab[nCTF][nMaps] (bioem_hip_ctf_table, merged over shards): the HEADER::
// NOTATION bar of ANG_PROB, one notation line, then one line per (particle, CTF set), particle-major, fixed, 4 decimals:
//  i c k0 k1' k2 logP Separated: log(Total) Constoadd numconst Best: A cx cy norm mu
// k0 k1' k2: the CTF set as the "Maximizing Param" line prints it (ctfParam3[c]; the defocus in micro-m, PSF parameters as
// they are); logP = log(Total) + Constoadd + numconst with numconst = the constant of the particle's LogProb (log(volu)
// included; voluPerMap: map i's own volume element, round 2), so that a particle's lines sum, in log-sum-exp, to its
// LogProb; A: the orientation of the best match under that CTF set (4 numbers with quaternions, else 3) from the list
// max_prob_orient indexes (angles, anglesPerMap, angleOffsets as in Driver::writeProbabilities).
// Returns the empty string, or the error: the file cannot be written, or an entry is still as start_run left it (no
// comparison reached that particle under that CTF set), named by particle and CTF set.
std::string write_ctf_prob(const char *file, const bioem_hip_prob_map *tab, int nCTF, int nMaps, const float *ctfParam3,
                           bool usepsf, float elecwavel, bool doquater, const float *angles, size_t anglesPerMap,
                           const long long *angleOffsets, float Ntotpi, float volu, const float *voluPerMap);
// --BestFRC (bestfrc.cpp): the text file of the ring sums sums[nMaps][nRings] of bioem_hip_best_match_rings.  After the
// HEADER:: NOTATION bar, one notation line and the bar again, per particle one line per ring s >= 0
//  RING p s resolution weight FRC powParticle powModel powResidual
// (resolution = N pixelSize / s in Angstrom, 0 for ring 0; weight = coefficients of the full spectrum in the ring;
// FRC = cross / sqrt(powParticle powModel), 0 where the product is 0; powResidual = powParticle + powModel - 2 cross) and
//  SUMMARY p CCC residualRMS res05 res0143
// (CCC: the same quotient over the sums of rings s >= 1; residualRMS = sqrt(sum_s powResidual / N^4), the RMS over the
// pixels of particle - best map; res05 / res0143: the resolution of the first ring s >= 1 with FRC < 0.5 / < 0.143, -1
// when none).  Floating values with 16 significant digits.  Returns the empty string, or the error.
int frc_ring(int N, int k1, int k2);
std::vector<double> frc_ring_weights(int N);
std::string write_best_frc(const char *file, const bioem_hip_ring_sums *sums, int nMaps, int N, float pixelSize);
// --BestWindow (bestwindow.cpp): the text file of the window tables logp[nMaps][nd][nd] of bioem_hip_window_posterior for
// every particle's best (orientation, CTF) pair; cell [i][j] lies at the reported shift (shifts[i], shifts[j]).  After the
// HEADER:: NOTATION bar, one notation line and the bar again, per particle
//  WINDOW p amp pha env orient logP peakX peakY peakLogp meanX meanY sdX sdY edgeMass nEff skipped nd
// (amp pha env: the CTF columns as --ProbCTF prints them; logP = log-sum-exp of the finite cells + numconst[p], the
// constant of the particle's LogProb; peak: the arg-max cell, the first in row-major order among equals; mean, sd: of the
// posterior over the shift on both axes; edgeMass: the mass on cells whose X or Y is the smallest or largest of the set;
// nEff = 1 / sum w^2; skipped: cells that are not finite, left out of every statistic) followed by nd * nd lines
//  CELL p X Y logp weight
// (logp with numconst[p] added, weight = exp(logp - logP), 0 for a skipped cell).  orient[p] < 0: a particle without a
// table -- orient -1, nd 0, no cells.  Floating values with 16 significant digits, every statistic in double.
// Returns the empty string, or the error.
struct WindowStats
{
  double logP, peakLogp, meanX, meanY, sdX, sdY, edgeMass, nEff;
  int peakX, peakY, skipped;
};
WindowStats window_stats(const double *logp, const int *shifts, int nd);
std::string write_best_window(const char *file, const double *logp, const int *shifts, int nd, int nMaps, const int *orient,
                              const int *conv, const float *ctfParam3, bool usepsf, float elecwavel, const double *numconst);
// --CTFScan (ctfscan.cpp): the posterior of every particle's best record (orientation, shift) over candidate CTF sets that
// refine the parameter file's grid (bioem_hip_ctf_scan).  Candidates: on every axis with n > 1 points the n k values
// (float) i * (g / (float) k) + start, g the grid's step, k = 1, 2, 4, 8 or 16 (every k-th value is a grid value bit for
// bit); an axis with one point keeps it.  Candidate index: amp outermost, envelope innermost, as the CTF sets of a run.
const int kCtfScanMaxCandidates = 4096; // bounds the host's tables; a choice, not a measurement
bool ctf_scan_factor_valid(int k);
// counts[3] and, when triples is given and there are at most kCtfScanMaxCandidates of them, the candidates
// triples[G][3]; returns G
int ctf_scan_refine(const float start[3], const float step[3], const int n[3], int k, int counts[3], float *triples);
// statistics of one particle's logp[G] over the finite candidates, in double and in the units of the triples: logP the
// log-sum-exp, best the arg-max candidate (the first among equals; -1 when none is finite), per axis the mean and sd of the
// marginal posterior and the mass on its two outermost values (on its one value: 1), nEff = 1 / sum w^2
struct CtfScanStats
{
  double logP, mean[3], sd[3], edgeMass[3], nEff;
  int best, skipped;
};
CtfScanStats ctf_scan_stats(const double *logp, const float *triples, const int counts[3]);
// the text file of logp[nMaps][G].  After the HEADER:: NOTATION bar, one notation line and the bar again, per particle
//  SCAN p amp pha env orient shiftX shiftY best logP  nAmp meanAmp sdAmp edgeAmp  nPha meanPha sdPha edgePha
//       nEnv meanEnv sdEnv edgeEnv  skipped G nEff
// (amp pha env: the arg-max candidate as --ProbCTF prints the CTF columns, the phase statistics in that unit; logP with
// numconst[p], the constant of the particle's LogProb, added) followed by G lines
//  CAND p g amp pha env logP weight
// (logP = the candidate's log posterior + numconst[p], weight = its share of the posterior, 0 when not finite).
// orient[p] < 0: a particle without a table -- orient -1, G 0, no candidates.  16 significant digits.  Returns the empty
// string, or the error.
std::string write_ctf_scan(const char *file, const double *logp, const float *triples, const int counts[3], int nMaps,
                           const int *orient, const int *shiftX, const int *shiftY, bool usepsf, float elecwavel,
                           const double *numconst);
// --ModelGradient (modelgrad.cpp): the text file of the sums acc[nPts] of bioem_hip_model_gradient over the particles'
// best records.  After the HEADER:: NOTATION bar, one notation line and the bar again, per model point
//  POINT k x y z radius density sum mean z count
// (sum = sum_r g_rk, mean = sum / sumw or 0 where no request saw the point, z = sum / sqrt(sumsq) or 0) and one line
//  DATASET rho_dot_sum norm nonfinite
// (sum_k rho_k sum_k, which the normalisation of the projection makes 0 analytically; the Euclidean norm of sum; the
// requests whose coefficients were not finite).  17 significant digits.  Returns the empty string, or the error.
std::string write_model_gradient(const char *file, const bioem_hip_model_point *points, const bioem_hip_grad_point *acc, int nPts,
                                 int nonfinite);
// --VolumeGradient (volgrad.cpp): the text file beside the gradient volume gvol [N][N][N] of bioem_hip_volume_gradient over
// the particles' best records, vol the model's density.  After the HEADER:: NOTATION bar, one notation line and the bar
// again, per shell s (the voxels whose distance from the origin voxel (N + 1) / 2 rounds to s) that holds voxels
//  SHELL s voxels sum power vol_dot_g
// (the sums of g, g^2 and vol g over the shell) and one line
//  DATASET vol_dot_g norm requests sumw nonfinite
// (sum_x vol g, analytically -sumw; the Euclidean norm of g; the requests, the sum of their weights and how many had
// coefficients that were not finite).  17 significant digits.  Returns the empty string, or the error.
std::string write_volume_gradient(const char *file, const double *gvol, const float *vol, int N, int nRequests, double sumw,
                                  int nonfinite);
// --PoseGradient (posegrad.cpp): the text file of the rows rows[n][18] = {J[6], T[2], dot, R[9]} of bioem_hip_pose_gradient
// over the particles' best records req[n], angles4[n][4] the four numbers of each record's orientation.  After the HEADER::
// NOTATION bar, one notation line and the bar again, per record
//  POSE particle orient q0 q1 q2 q3 conv shiftX shiftY gw0 gw1 gw2 gdeg T0 T1 dot
// (g_w the derivative with respect to a small rotation in the frame of the image, pose_rotation_gradient; gdeg = |g_w| pi /
// 180, the change of log P per degree along the ascent axis; T the derivative with respect to the model shifts) and one line
//  DATASET particles rms_gdeg rms_T
// 17 significant digits.  Returns the empty string, or the error.
void pose_rotation_gradient(const double *row, double *g);
std::string write_pose_gradient(const char *file, const double *rows, const bioem_hip_grad_request *req, const float *angles4,
                                int n);
// --CTFGradient (ctfgrad.cpp): the text file of the rows rows[n][38] of bioem_hip_ctf_gradient over the particles' best records
// req[n].  After the HEADER:: NOTATION bar, one notation line and the bar again, per record
//  CTFGRAD particle orient conv shiftX shiftY amp defocus env g_amp g_defocus g_env H_aa H_ad H_ae H_dd H_de H_ee
//          newton_defocus sigma_defocus
// (the CTF columns as --ProbCTF prints them, defocus = pha / (2 pi 1e4 lambda) in micro-m; gradient and Hessian of the data's
// part of log P in those units -- the prior's part is left out; the Newton defocus along the defocus axis alone and its Laplace
// error bar sqrt(-1 / H_dd), nan where H_dd is not negative) and one line
//  DATASET particles defined rms_g_defocus
// 17 significant digits.  Returns the empty string, or the error.
std::string write_ctf_gradient(const char *file, const double *rows, const bioem_hip_grad_request *req, int n, float elecwavel);
// --OrientStats (orientstats.cpp): the text file of the sums sums[nMaps] of bioem_hip_orientation_sums.  After the
// HEADER:: NOTATION bar, one notation line (it carries the constant as NumericalConst) and the bar again, per particle
//  ORIENT p count logZ omax A pTop entropy nEff meanq1 meanq2 meanq3 meanq4 spreadDeg
// (count: entries of the angle table that were compared; logZ = m + log S0 + numconst, the constant of ANG_PROB; omax: the
// arg-max orientation and A its 4 numbers with quaternions, else 3, from the list angles4 (angleOffsets: particle p's list
// begins at entry angleOffsets[p]); pTop = 1 / S0; entropy = log S0 - S1 / S0; nEff = S0^2 / S2; mean: the eigenvector of
// Q / S0 of the largest eigenvalue lambda, signed to a non-negative dot product with the arg-max quaternion; spreadDeg =
// 2 acos(sqrt(lambda)) in degrees).  Euler lists print "- -" for the mean and the spread; a particle with count 0 prints
// logZ -inf, omax -1, zeros.  Floating values with 16 significant digits.  Returns the empty string, or the error.
struct OrientStats
{
  long long count;
  int omax;
  bool hasMean;
  double logZ, pTop, entropy, nEff, mean[4], spreadDeg; // logZ without the constant
};
void jacobi4(const double a[4][4], double w[4], double v[4][4]); // eigenvalues descending, v[k] the vector of w[k]
OrientStats orient_derive(const bioem_hip_orient_sums &s, const float *angles4, bool doquater);
std::string write_orient_stats(const char *file, const bioem_hip_orient_sums *sums, int nMaps, const float *angles4,
                               const long long *angleOffsets, bool doquater, double numconst);
// --OrientOccupancy (orientocc.cpp): the text file of the occupancy occ[nO] of bioem_hip_orientation_occupancy (the
// shards' blocks concatenated).  After the HEADER:: NOTATION bar, one notation line and the bar again, per orientation
//  OCC o A count occ fraction nEffParticles hard wmax pmax
// (A: the orientation's 4 numbers with quaternions, else 3; count: particles compared with it; occ = sum over the
// particles of its posterior; fraction = occ / nCounted, nCounted the particles with a posterior at all; nEffParticles =
// occ^2 / occ2, 0 for an empty row; hard: particles whose arg-max it is; wmax and pmax: the largest posterior any
// particle gives it and the lowest such particle, -1 for an empty row), then one line
//  DATASET nCounted nEffViews maxFraction argmax
// (nEffViews = exp of the entropy of the fractions) and, with --FitOrientPrior, one line per EM iteration
//  FIT t logLikelihood nEffViews
// (logLikelihood = sum over the counted particles of m + log S0 under the prior of iteration t, without the numerical
// constant; nEffViews of that prior).  Floating values with 16 significant digits.  Returns the empty string, or the error.
const double kOrientPriorFloor = -1.0e6; // the log prior of an orientation no particle supports: finite, e^it = 0, and
                                         // twelve characters in the list file (-1.00000e+06)
struct OccDataset
{
  long long nCounted;
  double nEffViews, maxFraction;
  int argmax;
};
struct OccFit
{
  double logLikelihood, nEffViews;
};
OccDataset occ_dataset(const bioem_hip_orient_occ *occ, int nO, long long nCounted);
double log_prior_views(const double *logPrior, int nO); // exp of the entropy of e^logPrior
// the EM update: logPrior[o] = log(occ_o / nCounted), kOrientPriorFloor where occ_o = 0
void occ_next_prior(const bioem_hip_orient_occ *occ, int nO, long long nCounted, double *logPrior);
std::string write_orient_occupancy(const char *file, const bioem_hip_orient_occ *occ, int nO, const float *angles4, bool doquater,
                                   long long nCounted, const OccFit *fits, int nFits);
// the orientation list in the --ReadOrientation format (count line, twelve-character columns, angles to eight decimals)
// with the additive log prior as the last column, clamped to [kOrientPriorFloor, 0] and printed as %12.5e: what a run
// with PRIOR_ANGLES --ReadOrientation reads
std::string write_orient_prior(const char *file, const float *angles4, int nO, bool doquater, const double *logPrior);
// --ViewAverages (viewavg.cpp).  view_groups_by_orientation: the particles grouped by the arg-max orientation of their
// records (weight 1): groupOrient = the orientations with at least max(minCount, 1) particles, ascending; groupOf[p] = the
// view of particle p, -1 where its orientation has too few particles or no run compared it.  Returns the number of views.
// write_view_averages: the text file of the ring sums rings[nViews][nRings] of bioem_hip_view_averages.  After the HEADER::
// NOTATION bar, one notation line and the bar again, per view
//  VIEW v o A count CCC res05 res0143
// (o: the orientation and A its 4 numbers with quaternions, else 3; count: its particles; CCC = cross / sqrt(powAverage
// powProjection) over the sums of rings s >= 1; res05 / res0143: the resolution of the first ring s >= 1 with FRC < 0.5 /
// < 0.143, -1 when none) followed by one line per ring s >= 0
//  RING v s resolution weight FRC cross powAverage powProjection
// (resolution = N pixelSize / s in Angstrom, 0 for ring 0; weight = coefficients of the full spectrum in the ring; FRC =
// cross / sqrt(powAverage powProjection), 0 where the product is 0).  Floating values with 16 significant digits.
// Returns the empty string, or the error.
int view_groups_by_orientation(const bioem_hip_prob_map *pmap, int nMaps, int nOrient, int minCount, std::vector<int> &groupOf,
                               std::vector<int> &groupOrient);
std::string write_view_averages(const char *file, const bioem_hip_ring_sums *rings, int nViews, const int *groupOrient,
                                const int *counts, const float *angles4, bool doquater, int N, float pixelSize, int minCount,
                                double wiener);
// --Reconstruct (reconstruct.cpp).  recon_shell_sums: per shell of the rounded |kappa| of the stored half spectra specA, specB
// [N][N][H] (re, im) the number of coefficients of the full spectrum and the sums cross = sum w Re(A conj(B)), powA, powB
// with the Hermitian weights 2 and 1 of the ring sums (the weights add up to N^3).  write_reconstruction: after the HEADER::
// NOTATION bar, one notation line and the bar again, one line per shell s >= 0
//  SHELL s resolution weight FSC cross powHalf1 powHalf2
// (resolution = N pixelSize / s in Angstrom, 0 for shell 0; FSC = cross / sqrt(powHalf1 powHalf2), 0 where the product is 0)
// and one line
//  DATASET views particles tau res05 res0143
// (res05 / res0143: the resolution of the first shell s >= 1 with FSC < 0.5 / < 0.143, -1 when none).  write_mrc_volume: the
// volume [N][N][N] (origin at voxel (N + 1) / 2) as a mode-2 MRC file that --ReadModelMRC reads back with every point where
// the reconstruction has it: file[e] = vol[(e + 1) mod N] on every axis, stated in the file's label.  Each returns the empty
// string, or the error.
void recon_shell_sums(const double *specA, const double *specB, int N, std::vector<double> &weight, std::vector<double> &cross,
                      std::vector<double> &powA, std::vector<double> &powB);
std::string write_reconstruction(const char *file, const std::vector<double> &weight, const std::vector<double> &cross,
                                 const std::vector<double> &powA, const std::vector<double> &powB, int N, float pixelSize,
                                 double wiener, long long views, long long particles, double tau);
std::string write_mrc_volume(const char *file, const float *vol, int N, float pixelSize);
// --ReconstructSoft: appends to the text file of write_reconstruction per particle p one line
//  SOFT p requests n_eff mass_argmax
// (requests: its (orientation, CTF set) pairs; n_eff = 1 / sum w^2 over (orientation, CTF set, cell), 0 without a weight;
// mass_argmax: the largest w) and per shell of the two soft half maps one line
//  SOFTSHELL s resolution weight FSC cross powHalf1 powHalf2
// in the columns of the SHELL lines (bioem_amd/soft_views.py parses both).  Returns the empty string, or the error.
std::string append_reconstruction_soft(const char *file, const int *requests, const double *nEff, const double *massArgmax,
                                       int nMaps, const std::vector<double> &weight, const std::vector<double> &cross,
                                       const std::vector<double> &powA, const std::vector<double> &powB, int N, float pixelSize);
// MRC mode-2 stack nx = ny = N, nz = nMaps in the storage order the --ReadMRC reader expects, written batch by batch
struct MrcStackWriter
{
  FILE *f = nullptr;
  int N = 0, nMaps = 0, written = 0;
  bool open(const char *file, int N, int nMaps);
  bool append(const float *maps, int n); // [n][N][N]
  bool close();                          // false unless nMaps sections went in
  ~MrcStackWriter();
};

struct Model
{
  std::vector<bioem_hip_model_point> points;
  float NormDen = 0;
  bool readPDB = false, readModelMRC = false;
  // --ModelVolume: the MRC density itself is the model (bioem_hip_upload_model_volume), not a point per voxel.  volume
  // [N][N][N] with its origin at voxel (N + 1) / 2, the cyclic one-voxel shift of write_mrc_volume undone; centre: its
  // centre of mass in voxels relative to the origin (0 with NO_CENTEROFMASS); no points
  bool readVolume = false;
  int volumePad = 2;
  std::vector<float> volume;
  double centre[3] = {0., 0., 0.};
  void readVolumeFile(const InputParams &p, const char *file);
  // the model of either kind into handle h; the library's return code
  int upload(bioem_hip_handle h, const InputParams &p) const;
  void readModel(const InputParams &p, const char *file); // model.cpp:674-710
  void readTextFile(const InputParams &p, const char *file);
  void readPDBFile(const char *file);
  void readMRCFile(const InputParams &p, const char *file); // model.cpp:332-416
  void centerDensityMass();
};

struct ParticleStack
{
  int ntot = 0, N = 0;
  std::vector<float> maps; // [ntot][N][N]
  bool readMRC = false, readMultMRC = false;
  void readRefMaps(const InputParams &p, const char *file); // map.cpp:520-555
  void readTextMaps(const char *file);
  void readMRCMaps(const InputParams &p, const char *file);
};

class Driver
{
public:
  Driver();
  ~Driver();
  int configure(int argc, char **argv); // bioem.cpp:438-585
  int run();                            // bioem.cpp:659-1377
  void print_phase_report();            // BIOEM_DEBUG_OUTPUT >= 1: timer.cpp:156-165, bioem.cpp:769-889
  void cleanup();

  InputParams param;
  Model model;
  ParticleStack particles;
  std::string outfileName = "Output_Probabilities";
  std::string refineFile;        // --RefineOrientations: the small grid of round 2 (empty: one round)
  std::vector<float> refineGrid; // its quaternions [G][4], read with the options
  // --RefineSeeds M / --RefineLogWindow W: round 2 around up to M orientations per particle, the best of round 1 and
  // those within W of its log posterior (lists of different lengths); M = 1: the best alone, today's run
  int refineSeeds = 1;
  double refineLogWindow = -1.; // < 0: unlimited
  std::string bestMapsFile;  // --BestMaps: MRC stack of every particle's calculated best-match image (FILE, FILE_Round2)
  std::string probCtfFile;   // --ProbCTF: the posterior per (particle, CTF set) as text (FILE, FILE_Round2)
  std::string bestFrcFile;   // --BestFRC: ring correlation of every particle against its best match (FILE, FILE_Round2)
  std::string bestWindowFile; // --BestWindow: posterior over the displacement window of every best match (FILE, FILE_Round2)
  // --CTFScan FILE / --CTFScanFactor k: the posterior of every best record over the CTF grid refined k-fold (FILE,
  // FILE_Round2); k = 4 is a conventional choice, not a tuned one
  std::string ctfScanFile;
  int ctfScanFactor = 4;
  std::string ctfGradFile;     // --CTFGradient: gradient and curvature with respect to the CTF triple of the best matches (FILE, FILE_Round2)
  std::string poseGradFile;    // --PoseGradient: the pose gradient of the best matches on a volume model (FILE, FILE_Round2)
  std::string volGradFile;     // --VolumeGradient: the density gradient of the best matches per voxel (FILE, FILE.mrc, _Round2)
  std::string modelGradFile;   // --ModelGradient: the density gradient of the best matches per model point (FILE, FILE_Round2)
  std::string orientStatsFile; // --OrientStats: summaries of every particle's orientation posterior (WRITE_PROB_ANGLES)
  std::string orientOccFile;   // --OrientOccupancy: occupancy of every orientation over the data set (WRITE_PROB_ANGLES)
  int fitOrientPrior = 0;      // --FitOrientPrior N: N EM iterations of the orientation prior, FILE_prior
  // --ViewAverages: per view the aligned average of its particles against the projection (FILE, FILE_avg.mrc,
  // FILE_proj.mrc); --ViewMinParticles n: views with fewer particles are left out; --ViewWiener t: tau = t * mean den.
  // Both defaults are conventional values, not tuned ones
  std::string viewAvgFile;
  int viewMinParticles = 2;
  double viewWiener = 0.1;
  // --Reconstruct FILE: the 3D density of the particles under their arg-max orientations (FILE.mrc, FILE_half1.mrc,
  // FILE_half2.mrc) and the shell correlation of the halves (FILE); --ReconstructWiener t: tau = t * mean denV, a
  // conventional default, not a tuned one
  std::string reconFile;
  double reconWiener = 0.1;
  // --ReconstructSoft K with --Reconstruct: the density under the posterior over (K best orientations, CTF set, window
  // cell) of every particle (FILE_soft.mrc, FILE_soft_half1.mrc, FILE_soft_half2.mrc, SOFT / SOFTSHELL lines in FILE); 0: off
  int reconSoftK = 0;
  std::string bestParamFile; // --PrintBestCalMap: the reference's one-record mode, no particles, writes BESTMAP
  BestParams best;
  int printBestCalMap();     // bioem::printModel (bioem.cpp:624-657, 1925-2085)
  std::vector<unsigned char> prob;              // merged map entries [nMaps]
  std::vector<bioem_hip_angle_candidate> cand;  // merged K best orientations [nMaps][K] (WRITE_PROB_ANGLES)

  int algo = 1;
  int debugOutput = 0;
  int nGpus = 1;     // number of shards
  int firstDev = 0;  // GPUDEVICE
  bool splitCTF = false; // fewer orientations than shards: (orientation, CTF) pairs are split instead
  bool useRccl = false;  // one GPU per shard: the merge runs over RCCL (bioem_hip_merge)

private:
  // one unit of the run: orientations [o0, o1) (and, with the CTF split, the run [u0, u1) of orientation-major
  // (orientation, CTF) pairs) on one device, with a private probability block
  struct Shard
  {
    bioem_hip_handle h = nullptr;
    int device = 0, o0 = 0, o1 = 0;
    long long u0 = 0, u1 = 0;
    void *prob = nullptr;
  };
  int readOptions(int argc, char **argv);
  void writeOutput();
  // Output_Probabilities text of a probability block; orientation(i, o) = the four numbers of orientation o of map i
  // (angleOffsets: map i's list begins at entry angleOffsets[i] instead of anglesPerMap * i; voluPerMap: map i's own
  // volume element in the constant of its log posterior -- the lists of round 2 differ in length)
  void writeProbabilities(const std::string &file, const bioem_hip_prob_map *pmap, const bioem_hip_param_device &pd,
                          const float *angles, size_t anglesPerMap, bool angProb, const long long *angleOffsets = nullptr,
                          const float *voluPerMap = nullptr);
  // --BestMaps: the records' images from handle h (bioem_hip_render_best_maps), one batch on the host at a time
  void writeBestMaps(const std::string &file, bioem_hip_handle h, const bioem_hip_prob_map *pmap, int ownLists);
  // --BestFRC: the records' ring sums from handle h (bioem_hip_best_match_rings), written by write_best_frc
  void writeBestFrc(const std::string &file, bioem_hip_handle h, const bioem_hip_prob_map *pmap, int ownLists);
  // --ViewAverages: the records grouped by orientation, the chain on handle h (bioem_hip_view_averages) in chunks of
  // views, written by write_view_averages and two MRC stacks
  void writeViewAverages(const std::string &file, bioem_hip_handle h, const bioem_hip_prob_map *pmap);
  // --Reconstruct: the records grouped by orientation (at least one member), the chain on handle h (bioem_hip_reconstruct)
  // for all particles and for the even and the odd ones, written by write_mrc_volume and write_reconstruction
  void writeReconstruction(const std::string &file, bioem_hip_handle h, const bioem_hip_prob_map *pmap);
  // --ReconstructSoft: the members of the posterior over the window tables from handle h (bioem_hip_window_posterior), the
  // chain on it (bioem_hip_reconstruct_soft) for all particles and the two halves, written by write_mrc_volume and
  // append_reconstruction_soft
  void writeReconstructionSoft(const std::string &file, bioem_hip_handle h, const bioem_hip_prob_map *pmap);
  // --BestWindow: the window tables of the records' (orientation, CTF) pairs from handle h (bioem_hip_window_posterior),
  // written by write_best_window; voluPerMap as for writeProbabilities
  void writeBestWindow(const std::string &file, bioem_hip_handle h, const bioem_hip_prob_map *pmap, int ownLists,
                       const bioem_hip_param_device &pd, const float *voluPerMap = nullptr);
  // --CTFScan: the records' (orientation, shift) against the refined CTF grid from handle h (bioem_hip_ctf_scan), in
  // chunks of candidates, written by write_ctf_scan; voluPerMap as for writeProbabilities
  void writeCtfScan(const std::string &file, bioem_hip_handle h, const bioem_hip_prob_map *pmap, int ownLists,
                    const bioem_hip_param_device &pd, const float *voluPerMap = nullptr);
  // --ModelGradient: the records' gradient per model point from handle h (bioem_hip_model_gradient), written by
  // write_model_gradient
  void writeModelGradient(const std::string &file, bioem_hip_handle h, const bioem_hip_prob_map *pmap, int ownLists);
  // --VolumeGradient: the records' gradient per voxel of the volume model from handle h (bioem_hip_volume_gradient), written
  // as the MRC volume file + ".mrc" (write_mrc_volume: it overlays the model file voxel for voxel) and the text file
  // (write_volume_gradient)
  void writeVolumeGradient(const std::string &file, bioem_hip_handle h, const bioem_hip_prob_map *pmap, int ownLists);
  // --PoseGradient: the records' gradient with respect to the orientation and the model shifts from handle h
  // (bioem_hip_pose_gradient), written by write_pose_gradient; angles: the shared list, or with ownLists the particles'
  // lists (anglesPerMap each, or angleOffsets [nMaps + 1] where they differ in length)
  void writePoseGradient(const std::string &file, bioem_hip_handle h, const bioem_hip_prob_map *pmap, int ownLists,
                         const float *angles, size_t anglesPerMap, const long long *angleOffsets = nullptr);
  // --CTFGradient: the records' gradient and curvature with respect to the triple of their CTF set from handle h
  // (bioem_hip_ctf_gradient), written by write_ctf_gradient
  void writeCtfGradient(const std::string &file, bioem_hip_handle h, const bioem_hip_prob_map *pmap, int ownLists);
  // --OrientStats: the shards' orientation sums (bioem_hip_orientation_sums) merged on the host, written by
  // write_orient_stats; numconst: the constant of ANG_PROB
  void writeOrientStats(const std::string &file, double numconst);
  // every shard's orientation sums under logPrior (null: none), merged on the host in shard order
  void shardOrientSums(const double *logPrior, std::vector<bioem_hip_orient_sums> &sums);
  // --OrientOccupancy / --FitOrientPrior: every shard's sums merged on the host, every shard's occupancy block under the
  // merged sums, written by write_orient_occupancy; nIter EM iterations of the prior, written by write_orient_prior
  void writeOrientOccupancy(const std::string &file, int nIter);
  // one pass under logPrior (null: none): the merged sums and the concatenated occupancy blocks
  void orientOccupancyPass(const double *logPrior, std::vector<bioem_hip_orient_sums> &sums, std::vector<bioem_hip_orient_occ> &occ);
  // --ProbCTF: the tables of the handles merged on the host (shards in ascending order) and written
  void writeCtfProb(const std::string &file, const std::vector<bioem_hip_handle> &hs, const bioem_hip_param_device &pd,
                    const float *angles, size_t anglesPerMap, const long long *angleOffsets = nullptr,
                    const float *voluPerMap = nullptr);
  void runRound2(); // --RefineOrientations: every particle against best (x) grid, OutputFile_Round2
  void runRound2Seeds(); // the same around several seeds per particle (--RefineSeeds >= 2)
  std::vector<Shard> shards;
};

} // namespace bioem_host
#endif
