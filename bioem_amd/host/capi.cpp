// capi.cpp -- C entry points of the host layer for bindings (tests, bench.py): the one-off precompute
// the reference performs on the host before the hot loop.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "bioem_host.h"

extern "C" {

// == bioem_param::CalculateRefCTF kernels part (param.cpp:1336-1583), CTF mode only (no transform needed)
int bioem_host_ctf_kernels(int N, float pixelSize, float startAmp, float endAmp, int nAmp, float startPhase,
                           float endPhase, int nPhase, float startEnv, float endEnv, int nEnv, float *refCTF,
                           float *ctfParam, float *steps)
{
  return bioem_host::ctf_kernels(N, pixelSize, false, startAmp, endAmp, nAmp, startPhase, endPhase, nPhase, startEnv,
                                 endEnv, nEnv, refCTF, ctfParam, steps, nullptr, nullptr);
}

// the kernels of G triples handed in (ctf_kernel_list), CTF mode, or PSF mode through the device transform of `device`
static void capi_r2c_on_device(void *ctx, int N, const float *in, float *out)
{
  if (bioem_hip_r2c(*(int *) ctx, N, 1, in, out))
    bioem_host::fatal("device r2c failed");
}
int bioem_host_ctf_kernel_list(int N, float pixelSize, int usepsf, const float *triples, int G, float *out, int device)
{
  if (N < 2 || G < 1 || !triples || !out)
    return 1;
  bioem_host::ctf_kernel_list(N, pixelSize, usepsf != 0, triples, G, out, usepsf ? capi_r2c_on_device : nullptr, &device);
  return 0;
}

// the grid loop of ctf_kernels in PSF mode, transformed on `device` as the CLI's set-up transforms them
int bioem_host_psf_kernels(int N, float pixelSize, float startAmp, float endAmp, int nAmp, float startPhase, float endPhase,
                           int nPhase, float startEnv, float endEnv, int nEnv, float *refCTF, float *ctfParam, float *steps,
                           int device)
{
  return bioem_host::ctf_kernels(N, pixelSize, true, startAmp, endAmp, nAmp, startPhase, endPhase, nPhase, startEnv, endEnv,
                                 nEnv, refCTF, ctfParam, steps, capi_r2c_on_device, &device);
}

// the --CTFScan candidates (ctf_scan_refine): counts[3] and, when triples is not null, triples[G][3]; returns G, or -1 for
// a factor that is not 1, 2, 4, 8 or 16
int bioem_host_ctf_scan_refine(const float *start3, const float *step3, const int *n3, int k, int *counts3, float *triples)
{
  if (!bioem_host::ctf_scan_factor_valid(k))
    return -1;
  return bioem_host::ctf_scan_refine(start3, step3, n3, k, counts3, triples);
}

// the --CTFScan text of logp[nMaps][G] (write_ctf_scan, bioem_host.h); 0, or 1 with the text in err[cap]
int bioem_host_write_ctf_scan(const char *file, const double *logp, const float *triples, const int *counts3, int nMaps,
                              const int *orient, const int *shiftX, const int *shiftY, int usepsf, float elecwavel,
                              const double *numconst, char *err, int cap)
{
  const std::string e = bioem_host::write_ctf_scan(file, logp, triples, counts3, nMaps, orient, shiftX, shiftY, usepsf != 0,
                                                   elecwavel, numconst);
  if (e.empty())
    return 0;
  if (err && cap > 0)
    snprintf(err, (size_t) cap, "%s", e.c_str());
  return 1;
}

// the --ModelGradient text of acc[nPts] (write_model_gradient, bioem_host.h); 0, or 1 with the text in err[cap]
int bioem_host_write_model_gradient(const char *file, const bioem_hip_model_point *points, const bioem_hip_grad_point *acc,
                                    int nPts, int nonfinite, char *err, int cap)
{
  const std::string e = bioem_host::write_model_gradient(file, points, acc, nPts, nonfinite);
  if (e.empty())
    return 0;
  if (err && cap > 0)
    snprintf(err, (size_t) cap, "%s", e.c_str());
  return 1;
}

// == volume element (param.cpp:1600-1607)
float bioem_host_volume_element(float voluang, int gridSpaceCenter, int maxDisplaceCenter, float pixelSize, int nAmp,
                                float gridEnvelop, float gridPhase, float sigB, float sigDef, float sigAmp)
{
  return bioem_host::volume_element(voluang, gridSpaceCenter, maxDisplaceCenter, pixelSize, nAmp, gridEnvelop,
                                    gridPhase, sigB, sigDef, sigAmp);
}

// == bioem_model::centerDensityMass (model.cpp:604-672); returns NormDen
float bioem_host_center_model(bioem_hip_model_point *pts, int n)
{
  bioem_host::Model m;
  m.points.assign(pts, pts + n);
  m.NormDen = 0.f;
  for (int i = 0; i < n; i++)
    m.NormDen += pts[i].density;
  m.centerDensityMass();
  for (int i = 0; i < n; i++)
    pts[i] = m.points[i];
  return m.NormDen;
}

// ------------------------------------------------------------------------------------------------
// file-level set-up without a device (CTF mode): readParameters + CalculateGridsParam + CalculateRefCTF.
// Used by the CPU tests to compare the host layer with the oracle's restatement on the golden inputs.
// Two-call protocol: sizes first (arrays NULL), then the arrays.
// ------------------------------------------------------------------------------------------------
struct bioem_host_setup
{
  bioem_hip_param_device pd;
  int nAngles, nCTF, isQuat, usepsf, shiftX, shiftY, nocentermass;
  float pixelSize, voluang, elecwavel;
};

int bioem_host_setup_from_files(const char *paramfile, const char *anglefile, bioem_host_setup *out, float *angles4,
                                float *refCTF, float *ctfParam3)
{
  bioem_host::InputParams P;
  P.notuniformangles = (anglefile && anglefile[0]);
  P.readParameters(paramfile);
  P.calculateGridsParam(anglefile ? anglefile : "");
  out->nAngles = P.nTotGridAngles;
  out->isQuat = P.doquater;
  out->usepsf = P.usepsf;
  out->shiftX = P.shiftX;
  out->shiftY = P.shiftY;
  out->nocentermass = P.nocentermass;
  out->pixelSize = P.pixelSize;
  out->voluang = P.voluang;
  out->elecwavel = P.elecwavel;
  out->nCTF = P.numberGridPointsCTF_amp * P.numberGridPointsCTF_phase * P.numberGridPointsEnvelop;
  if (!P.usepsf)
  {
    P.calculateRefCTF();
    if (refCTF)
      for (size_t e = 0; e < P.refCTF.size(); e++)
        refCTF[e] = P.refCTF[e];
    if (ctfParam3)
      for (size_t e = 0; e < P.ctfParam.size(); e++)
        ctfParam3[e] = P.ctfParam[e];
  }
  out->pd = P.pd;
  if (angles4)
    for (size_t e = 0; e < P.angles.size(); e++)
      angles4[e] = P.angles[e];
  return 0;
}

// model readers: returns the number of points (fills up to cap), NormDen through *normden
// isPDB: 0 text, 1 PDB, 2 MRC density map (pixelSize needed for the voxel positions)
int bioem_host_read_model(const char *file, int isPDB, int nocentermass, float pixelSize, bioem_hip_model_point *pts,
                          int cap, float *normden)
{
  bioem_host::InputParams P;
  P.nocentermass = nocentermass;
  P.ignorePDB = true;
  P.pixelSize = pixelSize;
  bioem_host::Model m;
  m.readPDB = (isPDB == 1);
  m.readModelMRC = (isPDB == 2);
  m.readModel(P, file);
  for (int i = 0; i < (int) m.points.size() && i < cap; i++)
    pts[i] = m.points[i];
  *normden = m.NormDen;
  return (int) m.points.size();
}

// the reader of --ModelVolume: vol [N][N][N] with its origin at voxel (N + 1) / 2, the centre of mass in voxels relative to
// it (0 with nocentermass) and the total density; returns N^3
int bioem_host_read_model_volume(const char *file, int N, int nocentermass, float *vol, double *centre, float *normden)
{
  bioem_host::InputParams P;
  P.nocentermass = nocentermass;
  P.N = N;
  bioem_host::Model m;
  m.readVolume = true;
  m.readModel(P, file);
  std::copy(m.volume.begin(), m.volume.end(), vol);
  std::copy(m.centre, m.centre + 3, centre);
  *normden = m.NormDen;
  return (int) m.volume.size();
}

// particle readers: mode 0 text, 1 single MRC, 2 list of MRCs; returns the number of images
int bioem_host_read_particles(const char *file, int mode, int N, int notnormmap, float *maps, int cap)
{
  bioem_host::InputParams P;
  P.N = N;
  P.notnormmap = notnormmap;
  bioem_host::ParticleStack S;
  S.readMRC = mode >= 1;
  S.readMultMRC = mode == 2;
  S.readRefMaps(P, file);
  const size_t sz = (size_t) N * N;
  for (int i = 0; i < S.ntot && i < cap; i++)
    for (size_t e = 0; e < sz; e++)
      maps[(size_t) i * sz + e] = S.maps[(size_t) i * sz + e];
  return S.ntot;
}

// ---- the calculated best-match image on the host side (bestmap.cpp), without a device ----
// the BEST_* file of --PrintBestCalMap as the parser holds it; returns 0, or 1 with the error text in err[cap]
struct bioem_host_best_params
{
  float pixelSize;
  int N;
  float angle[4];
  int doquater, usepsf, withnoise, doaaradius, printrotmod;
  float amp, phase, env;
  int ddx, ddy, shiftX, shiftY;
  float norm, offset, stnoise;
};

int bioem_host_read_best_parameters(const char *file, bioem_host_best_params *out, char *err, int cap)
{
  bioem_host::BestParams b;
  const std::string e = bioem_host::read_best_parameters(file, b);
  if (err && cap > 0)
    snprintf(err, (size_t) cap, "%s", e.c_str());
  if (!e.empty())
    return 1;
  out->pixelSize = b.pixelSize;
  out->N = b.N;
  memcpy(out->angle, b.angle, sizeof(b.angle));
  out->doquater = b.doquater;
  out->usepsf = b.usepsf;
  out->withnoise = b.withnoise;
  out->doaaradius = b.doaaradius;
  out->printrotmod = b.printrotmod;
  out->amp = b.amp;
  out->phase = b.phase;
  out->env = b.env;
  out->ddx = b.ddx;
  out->ddy = b.ddy;
  out->shiftX = b.shiftX;
  out->shiftY = b.shiftY;
  out->norm = b.norm;
  out->offset = b.offset;
  out->stnoise = b.stnoise;
  return 0;
}

// the BESTMAP text (bioem.cpp:2041-2079) of the unshifted map v[N][N]
int bioem_host_write_bestmap(const char *file, const float *v, int N, int ddx, int ddy, int mapOnly)
{
  return bioem_host::write_bestmap_text(file, v, N, ddx, ddy, mapOnly != 0) ? 0 : 1;
}

// the --ProbCTF text of a CTF table tab[nCTF][nMaps] (write_ctf_prob, bioem_host.h); angles: one list for all maps
// (anglesPerMap = 0) or anglesPerMap entries per map; voluPerMap may be NULL.  Returns 0, or 1 with the text in err[cap]
int bioem_host_write_ctf_prob(const char *file, const bioem_hip_prob_map *tab, int nCTF, int nMaps, const float *ctfParam3,
                              int usepsf, float elecwavel, int doquater, const float *angles, int anglesPerMap,
                              float Ntotpi, float volu, const float *voluPerMap, char *err, int cap)
{
  const std::string e = bioem_host::write_ctf_prob(file, tab, nCTF, nMaps, ctfParam3, usepsf != 0, elecwavel, doquater != 0,
                                                   angles, (size_t) anglesPerMap, nullptr, Ntotpi, volu, voluPerMap);
  if (err && cap > 0)
    snprintf(err, (size_t) cap, "%s", e.c_str());
  return e.empty() ? 0 : 1;
}

// the --BestFRC text of ring sums sums[nMaps][nRings] (write_best_frc, bioem_host.h); 0, or 1 with the text in err[cap]
int bioem_host_write_best_frc(const char *file, const bioem_hip_ring_sums *sums, int nMaps, int N, float pixelSize,
                              char *err, int cap)
{
  const std::string e = bioem_host::write_best_frc(file, sums, nMaps, N, pixelSize);
  if (err && cap > 0)
    snprintf(err, (size_t) cap, "%s", e.c_str());
  return e.empty() ? 0 : 1;
}

// the --BestWindow text of window tables logp[nMaps][nd][nd] (write_best_window, bioem_host.h); 0, or 1 with the text in
// err[cap]
int bioem_host_write_best_window(const char *file, const double *logp, const int *shifts, int nd, int nMaps, const int *orient,
                                 const int *conv, const float *ctfParam3, int usepsf, float elecwavel, const double *numconst,
                                 char *err, int cap)
{
  const std::string e = bioem_host::write_best_window(file, logp, shifts, nd, nMaps, orient, conv, ctfParam3, usepsf != 0,
                                                      elecwavel, numconst);
  if (err && cap > 0)
    snprintf(err, (size_t) cap, "%s", e.c_str());
  return e.empty() ? 0 : 1;
}

// the --OrientStats text of sums[nMaps] (write_orient_stats, bioem_host.h): angles4 one list for all maps; 0, or 1 with
// the text in err[cap]
int bioem_host_write_orient_stats(const char *file, const bioem_hip_orient_sums *sums, int nMaps, const float *angles4,
                                  int doquater, double numconst, char *err, int cap)
{
  const std::string e = bioem_host::write_orient_stats(file, sums, nMaps, angles4, nullptr, doquater != 0, numconst);
  if (err && cap > 0)
    snprintf(err, (size_t) cap, "%s", e.c_str());
  return e.empty() ? 0 : 1;
}

// the 4 x 4 Jacobi eigen-solver of --OrientStats: a[16] symmetric, row-major -> w[4] descending, v[4][4] with row k the
// unit eigenvector of w[k]
void bioem_host_jacobi4(const double *a, double *w, double *v)
{
  double A[4][4], V[4][4];
  for (int i = 0; i < 4; i++)
    for (int j = 0; j < 4; j++)
      A[i][j] = a[4 * i + j];
  bioem_host::jacobi4(A, w, V);
  for (int i = 0; i < 4; i++)
    for (int j = 0; j < 4; j++)
      v[4 * i + j] = V[i][j];
}

// the --OrientOccupancy text of occ[nO] (write_orient_occupancy, bioem_host.h); fits = nFits pairs (logLikelihood,
// nEffViews) or NULL; 0, or 1 with the text in err[cap]
int bioem_host_write_orient_occupancy(const char *file, const bioem_hip_orient_occ *occ, int nO, const float *angles4, int doquater,
                                      long long nCounted, const double *fits, int nFits, char *err, int cap)
{
  std::vector<bioem_host::OccFit> F;
  for (int t = 0; fits && t < nFits; t++)
    F.push_back({fits[2 * t], fits[2 * t + 1]});
  const std::string e = bioem_host::write_orient_occupancy(file, occ, nO, angles4, doquater != 0, nCounted, F.data(), (int) F.size());
  if (err && cap > 0)
    snprintf(err, (size_t) cap, "%s", e.c_str());
  return e.empty() ? 0 : 1;
}

// the FILE_prior of --FitOrientPrior (write_orient_prior, bioem_host.h); 0, or 1 with the text in err[cap]
int bioem_host_write_orient_prior(const char *file, const float *angles4, int nO, int doquater, const double *logPrior, char *err,
                                  int cap)
{
  const std::string e = bioem_host::write_orient_prior(file, angles4, nO, doquater != 0, logPrior);
  if (err && cap > 0)
    snprintf(err, (size_t) cap, "%s", e.c_str());
  return e.empty() ? 0 : 1;
}

// the EM update of --FitOrientPrior: logPrior[nO] from occ[nO] (occ_next_prior); returns the floor written for occ = 0
double bioem_host_occ_next_prior(const bioem_hip_orient_occ *occ, int nO, long long nCounted, double *logPrior)
{
  bioem_host::occ_next_prior(occ, nO, nCounted, logPrior);
  return bioem_host::kOrientPriorFloor;
}

// readParameters + CalculateGridsParam as bioem_host_setup_from_files, returning what the reader keeps of the list:
// angles4[cap][4] and, under PRIOR_ANGLES, prior[cap]; returns the number of orientations, *hasPrior set
int bioem_host_read_orientation_list(const char *paramfile, const char *anglefile, float *angles4, float *prior, int cap,
                                     int *hasPrior)
{
  bioem_host::InputParams P;
  P.notuniformangles = (anglefile && anglefile[0]);
  P.readParameters(paramfile);
  P.calculateGridsParam(anglefile ? anglefile : "");
  const int n = P.nTotGridAngles;
  if (hasPrior)
    *hasPrior = P.yespriorAngles ? 1 : 0;
  for (int o = 0; o < n && o < cap; o++)
  {
    for (int i = 0; i < 4 && angles4; i++)
      angles4[4 * (size_t) o + i] = P.angles[4 * (size_t) o + i];
    if (prior && P.yespriorAngles)
      prior[o] = P.angprior[(size_t) o];
  }
  return n;
}

// the grouping of --ViewAverages (view_groups_by_orientation): groupOf[nMaps], groupOrient[cap]; returns the number of views
int bioem_host_view_groups(const bioem_hip_prob_map *pmap, int nMaps, int nOrient, int minCount, int *groupOf, int *groupOrient,
                           int cap)
{
  std::vector<int> go, gor;
  const int n = bioem_host::view_groups_by_orientation(pmap, nMaps, nOrient, minCount, go, gor);
  for (int p = 0; p < nMaps && groupOf; p++)
    groupOf[p] = go[(size_t) p];
  for (int g = 0; g < n && g < cap && groupOrient; g++)
    groupOrient[g] = gor[(size_t) g];
  return n;
}

// the --ViewAverages text of rings[nViews][nRings] (write_view_averages, bioem_host.h); 0, or 1 with the text in err[cap]
int bioem_host_write_view_averages(const char *file, const bioem_hip_ring_sums *rings, int nViews, const int *groupOrient,
                                   const int *counts, const float *angles4, int doquater, int N, float pixelSize, int minCount,
                                   double wiener, char *err, int cap)
{
  const std::string e = bioem_host::write_view_averages(file, rings, nViews, groupOrient, counts, angles4, doquater != 0, N,
                                                        pixelSize, minCount, wiener);
  if (err && cap > 0)
    snprintf(err, (size_t) cap, "%s", e.c_str());
  return e.empty() ? 0 : 1;
}

// the MRC stack of --BestMaps: maps [nMaps][N][N] appended in batches of `batch` images
int bioem_host_write_mrc_stack(const char *file, const float *maps, int nMaps, int N, int batch)
{
  bioem_host::MrcStackWriter w;
  if (batch < 1 || !w.open(file, N, nMaps))
    return 1;
  for (int p = 0; p < nMaps; p += batch)
    if (!w.append(maps + (size_t) p * N * N, nMaps - p < batch ? nMaps - p : batch))
      return 1;
  return w.close() ? 0 : 1;
}

// the --Reconstruct text of the shell sums of two half spectra [N][N][H] (recon_shell_sums, write_reconstruction) and the
// MRC volume (write_mrc_volume); 0, or 1 with the text in err[cap]
int bioem_host_write_reconstruction(const char *file, const double *specA, const double *specB, int N, float pixelSize,
                                    double wiener, long long views, long long particles, double tau, char *err, int cap)
{
  std::vector<double> w, c, pa, pb;
  bioem_host::recon_shell_sums(specA, specB, N, w, c, pa, pb);
  const std::string e = bioem_host::write_reconstruction(file, w, c, pa, pb, N, pixelSize, wiener, views, particles, tau);
  if (err && cap > 0)
    snprintf(err, (size_t) cap, "%s", e.c_str());
  return e.empty() ? 0 : 1;
}

int bioem_host_write_mrc_volume(const char *file, const float *vol, int N, float pixelSize, char *err, int cap)
{
  const std::string e = bioem_host::write_mrc_volume(file, vol, N, pixelSize);
  if (err && cap > 0)
    snprintf(err, (size_t) cap, "%s", e.c_str());
  return e.empty() ? 0 : 1;
}
}
