// driver.cpp -- the bioem-shaped driver: command line, configure(), run(), output files.
// Mirrors the control flow of /root/reference/bioem.cpp (readOptions 170-436, configure 438-585,
// run 659-1377) with the hot loop (createProjection -> createConvolutedProjectionMap -> compareRefMaps,
// bioem.cpp:763-891) delegated to the device through include/bioem_hip.h.  Orientations are sharded over
// the visible GPUs in the same contiguous blocks as the reference's MPI ranks (bioem.cpp:748-753) and the
// shards are merged with the log-sum-exp rule of bioem.cpp:909-1044.
#include <getopt.h>

#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <ctime>
#include <queue>
#include <random>
#include <thread>

#include "bioem_host.h"

namespace bioem_host
{

namespace
{
void r2c_on_device(void *ctx, int N, const float *in, float *out)
{
  const int device = ctx ? *static_cast<const int *>(ctx) : 0; // the device the run itself uses (GPUDEVICE)
  if (bioem_hip_r2c(device, N, 1, in, out))
    fatal("device r2c failed");
}

// The reference's performance knobs (bioem.cpp:99-135, bioem_cuda.cu:216-222) balance a GPU against CPU cores and tune
// its CUDA kernels.  A job script written for the reference may set any of them: they are read, reported and have
// no effect here -- every comparison runs on the device (there is no CPU path to share the work with), the kernels
// pick their own launch shapes, projection and convolution are batched on the device.
void report_reference_knobs()
{
  static const char *const knobs[] = {"GPUWORKLOAD", "GPUASYNC", "GPUDUALSTREAM", "BIOEM_CUDA_THREAD_COUNT",
                                      "BIOEM_PROJ_CONV_AT_ONCE", "OMP_NUM_THREADS"};
  for (const char *k : knobs)
    if (getenv(k))
      printf("Note - %s=%s accepted, no effect (100 %% of the comparisons run on the device)\n", k, getenv(k));
  if (getenv("GPU") && atoi(getenv("GPU")) == 0)
    printf("Note - GPU=0 accepted, no effect: this engine has no CPU path, the run uses the device\n");
}

void check(bioem_hip_handle h, int rc, const char *what)
{
  if (rc)
    fatal("%s: %s", what, bioem_hip_last_error(h));
}

// the constant of a LogProb line for the volume element volu (the arguments stay float: log(volu) as the sites wrote it)
double numconst_of(float Ntotpi, float volu)
{
  return 0.5 * log(M_PI) + (1 - Ntotpi * 0.5) * (log(2 * M_PI) + 1) + log(volu);
}

// the handle's batch (bioem_hip_max_batch), at least 1 and at most `most`
int batch_size(bioem_hip_handle h, int most = INT_MAX)
{
  int batch = 1;
  bioem_hip_max_batch(h, &batch, nullptr);
  return std::max(1, std::min(batch, most));
}

// call(p0, p1) of a best-match entry for one batch; where it refuses a record (returns 2) the batch is retried record by
// record and refused(p) warns and zero-fills each one still refused.  A device error (1) ends the run.
template <class Call, class Refused>
void batch_or_each_record(bioem_hip_handle h, int p0, int p1, const char *what, Call call, Refused refused)
{
  int rc = call(p0, p1);
  if (rc == 2)
  {
    for (int p = p0; p < p1 && rc != 1; p++)
    {
      rc = call(p, p + 1);
      if (rc == 2)
        refused(p);
    }
    rc = rc == 1 ? 1 : 0;
  }
  check(h, rc, what);
}

// the records pmap[nMaps] in order: push(p, record) for each one a run compared, the warning noMatch (a format that takes
// the particle's index) for the others
template <class Push>
void for_each_match(const bioem_hip_prob_map *pmap, int nMaps, const char *noMatch, Push push)
{
  for (int p = 0; p < nMaps; p++)
  {
    if (has_record(pmap[p]))
      push(p, pmap[p]);
    else
      warn(noMatch, p);
  }
}
} // namespace

Driver::Driver()
{
  // environment knobs shared with the reference (bioem.cpp:99-135)
  algo = getenv("BIOEM_ALGO") == NULL ? 1 : atoi(getenv("BIOEM_ALGO"));
  debugOutput = getenv("BIOEM_DEBUG_OUTPUT") == NULL ? 0 : atoi(getenv("BIOEM_DEBUG_OUTPUT"));
}

Driver::~Driver() { cleanup(); }

int Driver::readOptions(int ac, char **av)
{
  std::string infile, modelfile, mapfile, anglefile;
  bool viewOptions = false, scanOptions = false, reconOptions = false, volumeOptions = false;
  std::cout << " ++++++++++++ FROM COMMAND LINE +++++++++++\n\n";
  static const struct option opts[] = {{"Modelfile", required_argument, 0, 0},
                                       {"Particlesfile", required_argument, 0, 0},
                                       {"Inputfile", required_argument, 0, 0},
                                       {"PrintBestCalMap", required_argument, 0, 0},
                                       {"BestMaps", required_argument, 0, 0},
                                       {"ProbCTF", required_argument, 0, 0},
                                       {"BestFRC", required_argument, 0, 0},
                                       {"BestWindow", required_argument, 0, 0},
                                       {"CTFScan", required_argument, 0, 0},
                                       {"CTFScanFactor", required_argument, 0, 0},
                                       {"ModelGradient", required_argument, 0, 0},
                                       {"VolumeGradient", required_argument, 0, 0},
                                       {"PoseGradient", required_argument, 0, 0},
                                       {"CTFGradient", required_argument, 0, 0},
                                       {"OrientStats", required_argument, 0, 0},
                                       {"OrientOccupancy", required_argument, 0, 0},
                                       {"FitOrientPrior", required_argument, 0, 0},
                                       {"ViewAverages", required_argument, 0, 0},
                                       {"ViewMinParticles", required_argument, 0, 0},
                                       {"ViewWiener", required_argument, 0, 0},
                                       {"Reconstruct", required_argument, 0, 0},
                                       {"ReconstructWiener", required_argument, 0, 0},
                                       {"ReconstructSoft", required_argument, 0, 0},
                                       {"ReadOrientation", required_argument, 0, 0},
                                       {"RefineOrientations", required_argument, 0, 0},
                                       {"RefineSeeds", required_argument, 0, 0},
                                       {"RefineLogWindow", required_argument, 0, 0},
                                       {"ReadPDB", no_argument, 0, 0},
                                       {"ReadModelMRC", no_argument, 0, 0},
                                       {"ModelVolume", no_argument, 0, 0},
                                       {"ModelVolumePad", required_argument, 0, 0},
                                       {"ReadMRC", no_argument, 0, 0},
                                       {"ReadMultipleMRC", no_argument, 0, 0},
                                       {"DumpMaps", no_argument, 0, 0},
                                       {"LoadMapDump", no_argument, 0, 0},
                                       {"DumpModel", no_argument, 0, 0},
                                       {"LoadModelDump", no_argument, 0, 0},
                                       {"PrintCOORDREAD", no_argument, 0, 0},
                                       {"OutputFile", required_argument, 0, 0},
                                       {"help", no_argument, 0, 0},
                                       {0, 0, 0, 0}};
  auto usage = []() {
    printf("\nCommand line inputs:\n");
    printf("  --Modelfile arg        (Mandatory) Name of model file\n");
    printf("  --Particlesfile arg    (Mandatory) Name of particle-image file\n");
    printf("  --Inputfile arg        (Mandatory) Name of input parameter file\n");
    printf("  --ReadOrientation arg  (Optional) Read file name containing orientations\n");
    printf("  --RefineOrientations arg (Optional) Second round: file with a small list of quaternions; every particle\n");
    printf("                         is evaluated again on its best orientation x that list (OutputFile_Round2)\n");
    printf("  --RefineSeeds arg      (Optional) Second round around up to arg orientations per particle: the best of the\n");
    printf("                         first round and the next ones in its ranking (default 1)\n");
    printf("  --RefineLogWindow arg  (Optional) ... of which only those within arg of the best log posterior\n");
    printf("  --BestMaps arg         (Optional) Write the calculated image of every particle's best match as an MRC\n");
    printf("                         stack (with --RefineOrientations also arg_Round2)\n");
    printf("  --ProbCTF arg          (Optional) Write the posterior per particle and CTF set (log posterior and best match\n");
    printf("                         under every CTF set; with --RefineOrientations also arg_Round2)\n");
    printf("  --BestFRC arg          (Optional) Write the Fourier ring correlation of every particle against its best match\n");
    printf("                         (per ring: FRC and powers; with --RefineOrientations also arg_Round2)\n");
    printf("  --BestWindow arg       (Optional) Write the posterior over the displacement window of every particle's best match\n");
    printf("                         (is DISPLACE_CENTER wide enough? with --RefineOrientations also arg_Round2)\n");
    printf("  --CTFScan arg          (Optional) Write the posterior of every particle's best match over CTF sets between the points\n");
    printf("                         of the parameter file's grid (is the grid fine and wide enough? with --RefineOrientations\n");
    printf("                         also arg_Round2)\n");
    printf("  --CTFScanFactor arg    (Optional) With --CTFScan: every CTF axis with more than one point is refined arg-fold;\n");
    printf("                         1, 2, 4, 8 or 16 (default 4)\n");
    printf("  --VolumeGradient arg   (Optional) With --ModelVolume: write the gradient of the log posterior of the particles' best\n");
    printf("                         matches per voxel of the model as arg.mrc, and its shells as text to arg\n");
    printf("  --PoseGradient arg     (Optional) With --ModelVolume: write per particle the gradient of the log posterior of its best\n");
    printf("                         match with respect to a small rotation of the orientation and to the model shifts (with\n");
    printf("                         --RefineOrientations also arg_Round2)\n");
    printf("  --CTFGradient arg      (Optional) Write per particle the gradient and the curvature of the log posterior of its best\n");
    printf("                         match with respect to the CTF amplitude, defocus and B-envelope, the Newton defocus and its\n");
    printf("                         error bar (CTF parameters only; with --RefineOrientations also arg_Round2)\n");
    printf("  --ModelGradient arg    (Optional) Write per model point the gradient of the log posterior of the particles' best\n");
    printf("                         matches with respect to its density (which part of the model do the data argue against?\n");
    printf("                         with --RefineOrientations also arg_Round2)\n");
    printf("  --OrientStats arg      (Optional) Write per particle the summaries of its orientation posterior (entropy, effective\n");
    printf("                         number of orientations, mean orientation, spread; needs WRITE_PROB_ANGLES)\n");
    printf("  --OrientOccupancy arg  (Optional) Write per orientation its occupancy over the data set (which views are in it, how\n");
    printf("                         many particles stand behind each; needs WRITE_PROB_ANGLES)\n");
    printf("  --FitOrientPrior arg   (Optional) With --OrientOccupancy: arg EM iterations of the orientation prior, written as\n");
    printf("                         arg_prior of --OrientOccupancy in the --ReadOrientation format for PRIOR_ANGLES\n");
    printf("  --ViewAverages arg     (Optional) Write per view (orientation) the aligned, CTF-corrected average of its particles\n");
    printf("                         against the model's projection: ring correlation in arg, stacks arg_avg.mrc and arg_proj.mrc\n");
    printf("  --ViewMinParticles arg (Optional) With --ViewAverages: views with fewer particles are left out (default 2)\n");
    printf("  --ViewWiener arg       (Optional) With --ViewAverages: the Wiener constant as a fraction of the mean weight (default 0.1)\n");
    printf("  --Reconstruct arg      (Optional) Write the 3D density the particles support under their best orientations: arg.mrc,\n");
    printf("                         the half sets arg_half1.mrc / arg_half2.mrc and their shell correlation in arg; read back\n");
    printf("                         with --ReadModelMRC the volume lies where it was reconstructed (odd NUMBER_PIXELS: half a\n");
    printf("                         pixel beyond it on every axis)\n");
    printf("  --ReconstructWiener arg (Optional) With --Reconstruct: the Wiener constant as a fraction of the mean weight (default 0.1)\n");
    printf("  --ReconstructSoft arg  (Optional) With --Reconstruct: the same density under the posterior instead of its arg-max:\n");
    printf("                         every particle enters with every CTF set and every cell of the displacement window at its\n");
    printf("                         arg best orientations (1: the best one; 2 or more: of the ANG_PROB ranking, needs\n");
    printf("                         WRITE_PROB_ANGLES >= arg), weighted by the posterior: arg_soft.mrc, arg_soft_half1.mrc,\n");
    printf("                         arg_soft_half2.mrc of --Reconstruct and SOFT / SOFTSHELL lines in its text file\n");
    printf("  --PrintBestCalMap arg  (Optional) Only print best calculated map (file of BEST_ parameters). NO BioEM!\n");
    printf("  --ReadPDB              (Optional) If reading model file in PDB format\n");
    printf("  --ReadModelMRC         (Optional) If reading model file in MRC format\n");
    printf("  --ModelVolume          (Optional) The model file is an MRC density (mode 2, cubic, side NUMBER_PIXELS, as --Reconstruct\n");
    printf("                         writes it) used as a volume: projections are central slices of its spectrum\n");
    printf("  --ModelVolumePad arg   (Optional) With --ModelVolume: padding of the spectrum, 1 or 2 (default 2)\n");
    printf("  --ReadMRC              (Optional) If reading particle file in MRC format\n");
    printf("  --ReadMultipleMRC      (Optional) If reading multiple MRCs\n");
    printf("  --OutputFile arg       (Optional) For changing the outputfile name\n");
    printf("  --help                 (Optional) Produce help message\n");
  };
  if (ac < 2)
  {
    printf("Error - Need to specify all mandatory options\n");
    usage();
    return 1;
  }
  optind = 1;
  while (true)
  {
    int idx = 0;
    const int c = getopt_long(ac, av, "", opts, &idx);
    if (c == -1)
      break;
    if (c == '?')
    {
      usage();
      return 1;
    }
    const std::string name = opts[idx].name;
    if (name == "help")
    {
      std::cout << "Usage: options_description [options]\n";
      usage();
      return 1;
    }
    else if (name == "Inputfile")
    {
      std::cout << "Input file is: " << optarg << "\n";
      infile = optarg;
    }
    else if (name == "Modelfile")
    {
      std::cout << "Model file is: " << optarg << "\n";
      modelfile = optarg;
    }
    else if (name == "Particlesfile")
    {
      std::cout << "Particle file is: " << optarg << "\n";
      mapfile = optarg;
    }
    else if (name == "ReadPDB")
    {
      std::cout << "Reading model file in PDB format.\n";
      model.readPDB = true;
    }
    else if (name == "ReadModelMRC")
    {
      std::cout << "Reading model file in MRC format.\n";
      model.readModelMRC = true;
    }
    else if (name == "ModelVolume")
    {
      std::cout << "Reading model file as an MRC density volume.\n";
      model.readVolume = true;
    }
    else if (name == "ModelVolumePad")
    {
      model.volumePad = atoi(optarg);
      volumeOptions = true;
      if (model.volumePad != 1 && model.volumePad != 2)
        fatal("--ModelVolumePad needs 1 or 2");
    }
    else if (name == "ReadOrientation")
    {
      std::cout << "Reading Orientation from file: " << optarg << "\n";
      anglefile = optarg;
      param.notuniformangles = true;
    }
    else if (name == "RefineOrientations")
    {
      std::cout << "Refining orientations (second round) with the list: " << optarg << "\n";
      refineFile = optarg;
    }
    else if (name == "RefineSeeds")
    {
      refineSeeds = atoi(optarg);
      if (refineSeeds < 1)
        fatal("--RefineSeeds needs a positive number");
      std::cout << "Second round around up to " << refineSeeds << " orientations per particle\n";
    }
    else if (name == "RefineLogWindow")
    {
      refineLogWindow = atof(optarg);
      if (!(refineLogWindow >= 0.))
        fatal("--RefineLogWindow needs a non-negative number");
      std::cout << "Second round: seeds within " << refineLogWindow << " of the best log posterior\n";
    }
    else if (name == "BestMaps")
    {
      std::cout << "Writing the best calculated maps to: " << optarg << "\n";
      bestMapsFile = optarg;
    }
    else if (name == "ProbCTF")
    {
      std::cout << "Writing the posterior per CTF set to: " << optarg << "\n";
      probCtfFile = optarg;
    }
    else if (name == "BestFRC")
    {
      std::cout << "Writing the ring correlation of the best matches to: " << optarg << "\n";
      bestFrcFile = optarg;
    }
    else if (name == "BestWindow")
    {
      std::cout << "Writing the posterior over the displacement window of the best matches to: " << optarg << "\n";
      bestWindowFile = optarg;
    }
    else if (name == "CTFScan")
    {
      std::cout << "Writing the posterior over the refined CTF grid of the best matches to: " << optarg << "\n";
      ctfScanFile = optarg;
    }
    else if (name == "CTFScanFactor")
    {
      char *end = nullptr;
      const long k = strtol(optarg, &end, 10);
      scanOptions = true;
      if (end == optarg || *end || !ctf_scan_factor_valid((int) std::max(-1L, std::min(k, 1000L))))
      {
        printf("Error - --CTFScanFactor needs one of 1, 2, 4, 8, 16 (got %s)\n", optarg);
        usage();
        return 1;
      }
      ctfScanFactor = (int) k;
    }
    else if (name == "ModelGradient")
    {
      std::cout << "Writing the density gradient of the best matches per model point to: " << optarg << "\n";
      modelGradFile = optarg;
    }
    else if (name == "VolumeGradient")
    {
      std::cout << "Writing the density gradient of the best matches per voxel of the volume model to: " << optarg << "\n";
      volGradFile = optarg;
    }
    else if (name == "PoseGradient")
    {
      std::cout << "Writing the pose gradient of the best matches on the volume model to: " << optarg << "\n";
      poseGradFile = optarg;
    }
    else if (name == "CTFGradient")
    {
      std::cout << "Writing the CTF gradient and curvature of the best matches to: " << optarg << "\n";
      ctfGradFile = optarg;
    }
    else if (name == "OrientStats")
    {
      std::cout << "Writing the summaries of the orientation posteriors to: " << optarg << "\n";
      orientStatsFile = optarg;
    }
    else if (name == "OrientOccupancy")
    {
      std::cout << "Writing the occupancy of the orientations to: " << optarg << "\n";
      orientOccFile = optarg;
    }
    else if (name == "FitOrientPrior")
    {
      fitOrientPrior = atoi(optarg);
      if (fitOrientPrior < 1)
        fatal("--FitOrientPrior needs a positive number of iterations");
    }
    else if (name == "ViewAverages")
    {
      std::cout << "Writing the view averages to: " << optarg << "\n";
      viewAvgFile = optarg;
    }
    else if (name == "ViewMinParticles")
    {
      viewMinParticles = atoi(optarg);
      viewOptions = true;
      if (viewMinParticles < 1)
        fatal("--ViewMinParticles needs a positive number");
    }
    else if (name == "ViewWiener")
    {
      viewWiener = atof(optarg);
      viewOptions = true;
      if (!(viewWiener >= 0.) || !std::isfinite(viewWiener))
        fatal("--ViewWiener needs a non-negative number");
    }
    else if (name == "Reconstruct")
    {
      std::cout << "Writing the reconstruction to: " << optarg << "\n";
      reconFile = optarg;
    }
    else if (name == "ReconstructWiener")
    {
      reconWiener = atof(optarg);
      reconOptions = true;
      if (!(reconWiener >= 0.) || !std::isfinite(reconWiener))
        fatal("--ReconstructWiener needs a non-negative number");
    }
    else if (name == "ReconstructSoft")
    {
      reconSoftK = atoi(optarg);
      if (reconSoftK < 1)
        fatal("--ReconstructSoft needs a positive number of orientations");
    }
    else if (name == "PrintBestCalMap")
    {
      std::cout << "Reading best parameters from file: " << optarg << "\n";
      bestParamFile = optarg;
    }
    else if (name == "OutputFile")
    {
      std::cout << "Writing OUTPUT to: " << optarg << "\n";
      outfileName = optarg;
    }
    else if (name == "ReadMRC")
    {
      std::cout << "Reading particle file in MRC format.\n";
      particles.readMRC = true;
    }
    else if (name == "ReadMultipleMRC")
    {
      std::cout << "Reading multiple MRCs.\n";
      particles.readMultMRC = true;
    }
    else
      fatal("Option --%s is outside the compare path served by this build (SURVEY.md 8, out of scope)",
            name.c_str());
  }
  if (optind < ac)
  {
    printf("Error - Non-option ARGV-elements: ");
    while (optind < ac)
      printf("%s ", av[optind++]);
    putchar('\n');
    usage();
    return 1;
  }
  if (particles.readMultMRC && !particles.readMRC)
    fatal("For multiple MRCs command --ReadMRC is necessary too");
  if (volumeOptions && !model.readVolume)
    fatal("--ModelVolumePad goes with --ModelVolume");
  if (model.readVolume)
  { // the density itself is the model: nothing that reads or needs points goes with it
    if (model.readPDB)
      fatal("--ModelVolume is not valid with --ReadPDB (a PDB file holds atoms, not a density volume)");
    if (model.readModelMRC)
      fatal("--ModelVolume is not valid with --ReadModelMRC (which turns every voxel into a point; choose one)");
    if (!modelGradFile.empty())
      fatal("--ModelVolume is not valid with --ModelGradient (the gradient is per model point; a volume has none): the "
            "gradient per voxel is --VolumeGradient");
    if (!bestParamFile.empty())
      fatal("--ModelVolume is not valid with --PrintBestCalMap (its one-record mode reads the model as points)");
  }
  if (!volGradFile.empty() && !model.readVolume)
    fatal("--VolumeGradient needs --ModelVolume (the gradient is per voxel of a volume model; per model point it is "
          "--ModelGradient)");
  if (!volGradFile.empty() && !bestParamFile.empty())
    fatal("--PrintBestCalMap goes without --VolumeGradient");
  if (!poseGradFile.empty() && !model.readVolume)
    fatal("--PoseGradient needs --ModelVolume (a point model's projector has no derivative with respect to the orientation)");
  if (!poseGradFile.empty() && !bestParamFile.empty())
    fatal("--PrintBestCalMap goes without --PoseGradient");
  if (!ctfGradFile.empty() && !bestParamFile.empty())
    fatal("--PrintBestCalMap goes without --CTFGradient");
  if (!bestParamFile.empty())
  { // the reference's one-record mode (bioem.cpp:386-433): the BEST_* file stands for the parameter file, one orientation,
    // one CTF / PSF kernel, no particles, no grids
    if (!bestMapsFile.empty() || !refineFile.empty() || !probCtfFile.empty() || !bestFrcFile.empty() || !bestWindowFile.empty() ||
        !ctfScanFile.empty() || !orientStatsFile.empty() || !orientOccFile.empty() || !viewAvgFile.empty() ||
        !modelGradFile.empty() || !reconFile.empty())
      fatal("--PrintBestCalMap goes without --BestMaps, --ProbCTF, --BestFRC, --BestWindow, --CTFScan, --OrientStats, --OrientOccupancy, "
            "--ViewAverages, --ModelGradient, --Reconstruct and --RefineOrientations");
    const std::string err = read_best_parameters(bestParamFile.c_str(), best);
    if (!err.empty())
      fatal("%s", err.c_str());
    param.pixelSize = best.pixelSize;
    param.N = best.N;
    param.doquater = best.doquater;
    param.usepsf = best.usepsf;
    param.elecwavel = best.elecwavel;
    param.doaaradius = best.doaaradius;
    param.printrotmod = best.printrotmod;
    param.shiftX = best.shiftX;
    param.shiftY = best.shiftY;
    param.startGridCTF_amp = param.endGridCTF_amp = best.amp;
    param.startGridCTF_phase = param.endGridCTF_phase = best.phase;
    param.startGridEnvelop = param.endGridEnvelop = best.env;
    param.numberGridPointsCTF_amp = param.numberGridPointsCTF_phase = param.numberGridPointsEnvelop = 1;
    param.pd.maxDisplaceCenter = 0;
    param.pd.GridSpaceCenter = 1;
    param.pd.NumberPixels = best.N;
    param.pd.NumberFFTPixels1D = best.N / 2 + 1;
    param.pd.writeAngles = 0;
    param.pd.tousepsf = best.usepsf ? 1 : 0;
    param.angles.assign(best.angle, best.angle + 4);
    param.nTotGridAngles = 1;
    model.readModel(param, modelfile.c_str());
    return 0;
  }
  if (scanOptions && ctfScanFile.empty())
    fatal("--CTFScanFactor goes with --CTFScan");
  param.readParameters(infile.c_str());
  if (!ctfGradFile.empty() && param.usepsf)
    fatal("--CTFGradient is not valid with PSF parameters (a PSF kernel is the transform of a real-space function, not the "
          "closed form of the CTF that is differentiated)");
  if (refineFile.empty() && (refineSeeds != 1 || refineLogWindow >= 0.))
    fatal("--RefineSeeds / --RefineLogWindow go with --RefineOrientations");
  if (!orientStatsFile.empty())
  { // the summaries are reduced from the angle table: it must exist, and round 2 goes without it
    if (!refineFile.empty())
      fatal("--OrientStats is not valid with --RefineOrientations (which goes without WRITE_PROB_ANGLES)");
    if (!param.pd.writeAngles)
      fatal("--OrientStats needs WRITE_PROB_ANGLES in the parameter file: the summaries are reduced from the angle table");
  }
  if (!ctfScanFile.empty())
  { // the candidates are counted before anything is read or computed for the run
    const int n[3] = {param.numberGridPointsCTF_amp, param.numberGridPointsCTF_phase, param.numberGridPointsEnvelop};
    int counts[3];
    const int G = ctf_scan_refine(nullptr, nullptr, n, ctfScanFactor, counts, nullptr);
    if (G > kCtfScanMaxCandidates)
      fatal("--CTFScan: %d candidate CTF sets (%d x %d x %d, the grid refined %d-fold) are more than the %d this option takes; "
            "use a smaller --CTFScanFactor",
            G, counts[0], counts[1], counts[2], ctfScanFactor, kCtfScanMaxCandidates);
  }
  if (viewOptions && viewAvgFile.empty())
    fatal("--ViewMinParticles / --ViewWiener go with --ViewAverages");
  if (!viewAvgFile.empty() && !refineFile.empty()) // the views are orientations of the shared list
    fatal("--ViewAverages is not valid with --RefineOrientations (own lists share no orientation index)");
  if (reconOptions && reconFile.empty())
    fatal("--ReconstructWiener goes with --Reconstruct");
  if (reconSoftK && reconFile.empty())
    fatal("--ReconstructSoft goes with --Reconstruct");
  if (!reconFile.empty() && !refineFile.empty()) // the views are orientations of the shared list
    fatal("--Reconstruct is not valid with --RefineOrientations (own lists share no orientation index)");
  if (reconSoftK >= 2 && param.pd.writeAngles < reconSoftK) // the orientations beyond the best come from the ANG_PROB ranking
    fatal("--ReconstructSoft %d needs WRITE_PROB_ANGLES %d or more in the parameter file: the orientations are the first of "
          "the ANG_PROB ranking", reconSoftK, reconSoftK);
  if (fitOrientPrior && orientOccFile.empty())
    fatal("--FitOrientPrior is only valid with --OrientOccupancy");
  if (!orientOccFile.empty())
  { // the occupancy is reduced from the angle table: it must exist, and round 2 goes without it
    if (!refineFile.empty())
      fatal("--OrientOccupancy is not valid with --RefineOrientations (which goes without WRITE_PROB_ANGLES)");
    if (!param.pd.writeAngles)
      fatal("--OrientOccupancy needs WRITE_PROB_ANGLES in the parameter file: the occupancy is reduced from the angle table");
  }
  if (!refineFile.empty())
  { // round 2 multiplies quaternions and evaluates lists of its own: no prior per orientation, no ANG_PROB (yet)
    if (!param.doquater)
      fatal("--RefineOrientations needs quaternions (USE_QUATERNIONS): the second round multiplies them");
    if (param.yespriorAngles)
      fatal("--RefineOrientations is not valid with prior for orientations (PRIOR_ANGLES)");
    if (param.pd.writeAngles)
      fatal("--RefineOrientations is not valid with WRITE_PROB_ANGLES");
    refineGrid = read_quaternion_list(refineFile.c_str()); // now: a bad list must not end a run after its first round
  }
  particles.readRefMaps(param, mapfile.c_str());
  model.readModel(param, modelfile.c_str());
  param.calculateGridsParam(anglefile.c_str());
  // several seeds per particle: round 1 keeps its angle table on the device, for the seed selection only (ANG_PROB is
  // not written, OutputFile is what it is without the option)
  if (refineSeeds >= 2)
    param.pd.writeAngles = std::min(refineSeeds, param.nTotGridAngles);
  return 0;
}

int Driver::configure(int ac, char **av)
{
  if (readOptions(ac, av))
    return 1;
  const int ndev = bioem_hip_device_count();
  if (ndev < 1)
    fatal("No HIP device found: this engine has no CPU path");
  report_reference_knobs();
  nGpus = ndev;
  if (getenv("BIOEM_GPUS"))
    nGpus = std::max(1, std::min(ndev, atoi(getenv("BIOEM_GPUS"))));
  // BIOEM_SHARDS=n: n shards dealt round-robin over the selected GPUs (default: one per GPU); more shards than GPUs
  // is only useful to rehearse the multi-GPU control flow and merge on a smaller machine
  int nDevUsed = nGpus;
  int nShards = nGpus;
  if (getenv("BIOEM_SHARDS"))
    nShards = std::max(1, atoi(getenv("BIOEM_SHARDS")));
  firstDev = 0;
  if (getenv("GPUDEVICE") && atoi(getenv("GPUDEVICE")) >= 0) // bioem_cuda.cu:719-732
  {
    firstDev = atoi(getenv("GPUDEVICE"));
    if (!getenv("BIOEM_SHARDS"))
      nShards = 1;
    nDevUsed = 1;
    if (firstDev >= ndev)
      fatal("GPUDEVICE %d out of range (%d devices)", firstDev, ndev);
  }
  param.r2c = r2c_on_device;
  param.r2c_ctx = &firstDev;
  param.calculateRefCTF();
  if (!bestParamFile.empty()) // one handle, made where the map is rendered
    return 0;
  if (getenv("BIOEM_DEBUG_BREAK")) // bioem.cpp:518-525: after volu was computed with the full counts
  {
    const int cut = atoi(getenv("BIOEM_DEBUG_BREAK"));
    if (param.nTotGridAngles > cut)
      param.nTotGridAngles = cut;
    if (param.nTotCTFs > cut)
      param.nTotCTFs = cut;
  }
  // Work split (north_star: "orientations x CTF-envelope grid shard"): orientation blocks as the reference's MPI ranks
  // (bioem.cpp:748-753); with fewer orientations than shards the (orientation, CTF) pairs are split instead, in the
  // serial visiting order (orientation outer, CTF inner), so that shard s still precedes shard s+1
  const int nA = param.nTotGridAngles, nC = param.nTotCTFs;
  splitCTF = nShards > nA;
  if (splitCTF && (long long) nShards > (long long) nA * nC)
    nShards = nA * nC;
  nGpus = nShards;
  nDevUsed = std::min(nDevUsed, nShards);
  const int nMaps = particles.ntot;
  shards.assign(nShards, Shard());
  for (int g = 0; g < nShards; g++)
  {
    Shard &sh = shards[g];
    sh.device = firstDev + g % nDevUsed;
    if (!splitCTF)
    {
      sh.o0 = (int) ((long long) g * nA / nShards);
      sh.o1 = (int) ((long long) (g + 1) * nA / nShards);
      sh.u0 = (long long) sh.o0 * nC;
      sh.u1 = (long long) sh.o1 * nC;
    }
    else
    {
      sh.u0 = (long long) g * nA * nC / nShards;
      sh.u1 = (long long) (g + 1) * nA * nC / nShards;
      sh.o0 = (int) (sh.u0 / nC);
      sh.o1 = (int) ((sh.u1 + nC - 1) / nC);
    }
    bioem_hip_handle h = nullptr;
    // an orientation block owns its angle entries: shard handle (table [o1-o0][nMaps] stays on the device, K best
    // selected there).  With the CTF split an orientation has several owners: plain handles, full (tiny) table,
    // host merge of the angle entries
    const int rc = splitCTF ? bioem_hip_create(&h, sh.device, &param.pd, nMaps, nA, nC, algo)
                            : bioem_hip_create_shard(&h, sh.device, &param.pd, nMaps, nA, nC, algo, sh.o0, sh.o1);
    sh.h = h;
    check(h, rc, "bioem_hip_create");
    check(h, bioem_hip_upload_particle_maps(h, particles.maps.data()), "upload particles");
    check(h, bioem_hip_upload_ctf(h, param.refCTF.data(), param.ctfParam.data()), "upload CTF");
    check(h, model.upload(h, param),
          "upload model");
    check(h, bioem_hip_upload_orientations(h, param.angles.data(), nA, param.doquater ? 1 : 0), "upload orientations");
    if (!probCtfFile.empty())
      check(h, bioem_hip_enable_ctf_table(h, 1), "enable CTF table");
  }
  // RCCL carries the merge when every shard has a GPU of its own
  // (BIOEM_FORCE_RCCL=1: also with a single shard -- a one-rank communicator, to exercise this path on a one-GPU box)
  if (splitCTF && !orientStatsFile.empty())
    fatal("--OrientStats is not valid with more shards than orientations: an orientation's entry is spread over shards");
  if (splitCTF && !orientOccFile.empty())
    fatal("--OrientOccupancy is not valid with more shards than orientations: an orientation's entry is spread over shards");
  useRccl = (nShards > 1 || getenv("BIOEM_FORCE_RCCL")) && nDevUsed == nShards && !splitCTF && !getenv("BIOEM_HOST_MERGE");
  return 0;
}

// BIOEM_DEBUG_OUTPUT >= 1: the reference's per-phase report (bioem.cpp:769-889 "Time Projection / Convolution /
// Comparison" lines, TimeStat::PrintTimeStat timer.cpp:156-165 SUMMARY lines) from the engine's HIP-event records -- device
// time per batch of the pipeline; a shard stands where the reference prints its MPI rank
void Driver::print_phase_report()
{
  static const char *names[4] = {"Total time of projection", "Projection", "Convolution", "Comparison"};
  for (int g = 0; g < (int) shards.size(); g++)
  {
    int n = 0;
    if (bioem_hip_phase_records(shards[g].h, nullptr, 0, &n) || n == 0)
      continue;
    std::vector<bioem_hip_phase_record> rec(n);
    if (bioem_hip_phase_records(shards[g].h, rec.data(), n, &n))
      continue;
    std::vector<double> logs[4];
    double batchTotal = 0.;
    for (int i = 0; i < n; i++)
    {
      const bioem_hip_phase_record &r = rec[i];
      if (r.phase == BIOEM_HIP_PHASE_PROJECTION)
      {
        if (debugOutput >= 2)
          printf("\tTime Projection %d-%d: %f (rank %d)\n", r.iOrientBegin, r.iOrientEnd - 1, r.seconds, g);
        logs[1].push_back(r.seconds);
      }
      else if (r.phase == BIOEM_HIP_PHASE_CONVOLUTION)
      {
        if (debugOutput >= 2)
          printf("\t\tTime Convolution %d-%d %d-%d: %f (rank %d)\n", r.iOrientBegin, r.iOrientEnd - 1, r.iConvBegin,
                 r.iConvEnd - 1, r.seconds, g);
        logs[2].push_back(r.seconds);
      }
      else
      {
        if (debugOutput >= 2)
          printf("\t\tTime Comparison %d-%d %d-%d: %f sec (rank %d)\n", r.iOrientBegin, r.iOrientEnd - 1, r.iConvBegin,
                 r.iConvEnd - 1, r.seconds, g);
        logs[3].push_back(r.seconds);
      }
      batchTotal += r.seconds;
      // a batch ends with its (last) comparison: the reference's "Total time for projection" per orientation
      if (r.phase == BIOEM_HIP_PHASE_COMPARISON && (i + 1 == n || rec[i + 1].phase != BIOEM_HIP_PHASE_COMPARISON))
      {
        logs[0].push_back(batchTotal);
        batchTotal = 0.;
      }
    }
    for (int k = 0; k < 4; k++)
    {
      if (logs[k].empty())
        continue;
      double sum = 0., sq = 0.;
      for (double v : logs[k])
        sum += v;
      const double mean = sum / logs[k].size();
      for (double v : logs[k])
        sq += (v - mean) * (v - mean);
      printf("SUMMARY -> %s: Total %f sec; Mean %f sec; Std.Dev. %f (rank %d)\n", names[k], sum, mean,
             sqrt(sq / logs[k].size()), g);
    }
  }
}

// --BestMaps: every record's calculated image from handle h, batch by batch (one batch of maps on the host at a time)
void Driver::writeBestMaps(const std::string &file, bioem_hip_handle h, const bioem_hip_prob_map *pmap, int ownLists)
{
  const int nMaps = particles.ntot, N = param.N;
  const int batch = batch_size(h, nMaps);
  const size_t NN = (size_t) N * N;
  std::vector<float> buf((size_t) batch * NN);
  MrcStackWriter w;
  if (!w.open(file.c_str(), N, nMaps))
    fatal("Opening %s", file.c_str());
  for (int p0 = 0; p0 < nMaps; p0 += batch)
  {
    const int p1 = std::min(nMaps, p0 + batch);
    // a record without an image (a particle the round never compared): its section is zero, the others are rendered
    batch_or_each_record(
        h, p0, p1, "render best maps",
        [&](int a, int b) { return bioem_hip_render_best_maps(h, pmap, ownLists, a, b, buf.data() + (size_t) (a - p0) * NN); },
        [&](int p) {
          warn("best map of RefMap %d not rendered: %s", p, bioem_hip_last_error(h));
          std::fill(buf.begin() + (size_t) (p - p0) * NN, buf.begin() + (size_t) (p - p0 + 1) * NN, 0.f);
        });
    if (!w.append(buf.data(), p1 - p0))
      fatal("Writing %s", file.c_str());
  }
  if (!w.close())
    fatal("Writing %s", file.c_str());
  std::cout << "Best calculated maps of " << nMaps << " particles written to: " << file << "\n";
}

// --BestFRC: every record's ring sums from handle h, batch by batch, then the text file (write_best_frc)
void Driver::writeBestFrc(const std::string &file, bioem_hip_handle h, const bioem_hip_prob_map *pmap, int ownLists)
{
  const int nMaps = particles.ntot, N = param.N;
  const size_t nRings = (size_t) bioem_hip_ring_count(N);
  const int batch = batch_size(h, nMaps);
  std::vector<bioem_hip_ring_sums> sums((size_t) nMaps * nRings);
  const bioem_hip_ring_sums zero = {0., 0., 0.};
  for (int p0 = 0; p0 < nMaps; p0 += batch)
  { // a record without a best match (a particle the round never compared): its sums are zero, the others are computed
    batch_or_each_record(
        h, p0, std::min(nMaps, p0 + batch), "best match rings",
        [&](int a, int b) { return bioem_hip_best_match_rings(h, pmap, ownLists, a, b, sums.data() + (size_t) a * nRings); },
        [&](int p) {
          warn("ring sums of RefMap %d not computed: %s", p, bioem_hip_last_error(h));
          std::fill(sums.begin() + (size_t) p * nRings, sums.begin() + (size_t) (p + 1) * nRings, zero);
        });
  }
  const std::string err = write_best_frc(file.c_str(), sums.data(), nMaps, N, param.pixelSize);
  if (!err.empty())
    fatal("--BestFRC: %s", err.c_str());
  std::cout << "Ring correlation of " << nMaps << " particles against their best match written to: " << file << "\n";
}

// --ViewAverages: the merged records grouped by their arg-max orientation (weight 1), the chain on handle h chunk by
// chunk of views, then the text file (write_view_averages) and the stacks FILE_avg.mrc / FILE_proj.mrc
void Driver::writeViewAverages(const std::string &file, bioem_hip_handle h, const bioem_hip_prob_map *pmap)
{
  const int nMaps = particles.ntot, N = param.N;
  const size_t nRings = (size_t) bioem_hip_ring_count(N), NN = (size_t) N * N;
  std::vector<int> groupOf, groupOrient;
  const int nViews = view_groups_by_orientation(pmap, nMaps, param.nTotGridAngles, viewMinParticles, groupOf, groupOrient);
  std::vector<int> counts((size_t) nViews, 0);
  for (int p = 0; p < nMaps; p++)
    if (groupOf[(size_t) p] >= 0)
      counts[(size_t) groupOf[(size_t) p]]++;
  if (nViews < 1)
    warn("--ViewAverages: no orientation has %d particles or more; the files hold no view", viewMinParticles);
  const int batch = batch_size(h);
  std::vector<bioem_hip_ring_sums> rings((size_t) nViews * nRings);
  std::vector<float> avg((size_t) batch * NN), proj((size_t) batch * NN);
  const std::string avgFile = file + "_avg.mrc", projFile = file + "_proj.mrc";
  MrcStackWriter wa, wp;
  if (nViews > 0 && (!wa.open(avgFile.c_str(), N, nViews) || !wp.open(projFile.c_str(), N, nViews)))
    fatal("Opening %s / %s", avgFile.c_str(), projFile.c_str());
  for (int g0 = 0; g0 < nViews; g0 += batch)
  {
    const int g1 = std::min(nViews, g0 + batch);
    check(h, bioem_hip_view_averages(h, pmap, nullptr, groupOf.data(), groupOrient.data(), nViews, viewWiener, g0, g1,
                                     rings.data() + (size_t) g0 * nRings, avg.data(), proj.data()),
          "view averages");
    if (!wa.append(avg.data(), g1 - g0) || !wp.append(proj.data(), g1 - g0))
      fatal("Writing %s / %s", avgFile.c_str(), projFile.c_str());
  }
  if (nViews > 0 && (!wa.close() || !wp.close()))
    fatal("Writing %s / %s", avgFile.c_str(), projFile.c_str());
  const std::string err = write_view_averages(file.c_str(), rings.data(), nViews, groupOrient.data(), counts.data(),
                                              param.angles.data(), param.doquater, N, param.pixelSize, viewMinParticles,
                                              viewWiener);
  if (!err.empty())
    fatal("--ViewAverages: %s", err.c_str());
  std::cout << "Averages of " << nViews << " views written to: " << file << ", " << avgFile << ", " << projFile << "\n";
}

// --Reconstruct: the merged records grouped by their arg-max orientation (one member is enough), the chain on handle h
// three times through weights -- all particles, the even and the odd ones -- then the volumes (write_mrc_volume) and the
// shell correlation of the two halves (write_reconstruction)
void Driver::writeReconstruction(const std::string &file, bioem_hip_handle h, const bioem_hip_prob_map *pmap)
{
  const int nMaps = particles.ntot, N = param.N, H = N / 2 + 1;
  const size_t N3 = (size_t) N * N * N, V = (size_t) N * N * H;
  std::vector<int> groupOf, groupOrient;
  const int nViews = view_groups_by_orientation(pmap, nMaps, param.nTotGridAngles, 1, groupOf, groupOrient);
  if (nViews < 1)
    fatal("--Reconstruct: no particle has a record to reconstruct from");
  std::vector<float> vol(N3);
  std::vector<double> spec[2] = {std::vector<double>(2 * V), std::vector<double>(2 * V)}, w((size_t) nMaps);
  double stats[4] = {0., 0., 0., 0.}, half[4];
  const std::string names[3] = {file + ".mrc", file + "_half1.mrc", file + "_half2.mrc"};
  for (int k = 0; k < 3; k++)
  { // k = 0: every particle; 1, 2: the even and the odd ones
    for (int p = 0; p < nMaps; p++)
      w[(size_t) p] = (k == 0 || p % 2 == k - 1) ? 1. : 0.;
    check(h, bioem_hip_reconstruct(h, pmap, w.data(), groupOf.data(), groupOrient.data(), nViews, reconWiener,
                                   BIOEM_HIP_RECON_CORRECT, vol.data(), k ? spec[k - 1].data() : nullptr, nullptr,
                                   k ? half : stats),
          "reconstruction");
    const std::string err = write_mrc_volume(names[k].c_str(), vol.data(), N, param.pixelSize);
    if (!err.empty())
      fatal("--Reconstruct: %s", err.c_str());
  }
  std::vector<double> weight, cross, pa, pb;
  recon_shell_sums(spec[0].data(), spec[1].data(), N, weight, cross, pa, pb);
  const std::string err = write_reconstruction(file.c_str(), weight, cross, pa, pb, N, param.pixelSize, reconWiener,
                                               (long long) stats[0], (long long) stats[1], stats[3]);
  if (!err.empty())
    fatal("--Reconstruct: %s", err.c_str());
  std::cout << "Reconstruction from " << (long long) stats[1] << " particles in " << (long long) stats[0]
            << " views written to: " << file << ", " << names[0] << ", " << names[1] << ", " << names[2] << "\n";
}

// --ReconstructSoft K: per particle with a record the requests (its K best orientations) x (every CTF set), their window
// tables from handle h batch by batch (bioem_hip_window_posterior), the weight, norm and mu of every cell as
// bioem_amd/soft_views.py states them, the members and tables of bioem_hip_reconstruct_soft, the chain three times -- all
// particles, the even and the odd ones -- then the volumes FILE_soft*.mrc and the lines append_reconstruction_soft adds
void Driver::writeReconstructionSoft(const std::string &file, bioem_hip_handle h, const bioem_hip_prob_map *pmap)
{
  const int nMaps = particles.ntot, N = param.N, H = N / 2 + 1, nC = param.nTotCTFs, K = reconSoftK;
  const int Kang = param.pd.writeAngles, nA = param.nTotGridAngles;
  const size_t N3 = (size_t) N * N * N, V = (size_t) N * N * H;
  const int nd = bioem_hip_window_count(N, param.pd.maxDisplaceCenter, param.pd.GridSpaceCenter, algo);
  if (nd < 1)
    fatal("--ReconstructSoft: no displacement window for these parameters");
  std::vector<int> shifts((size_t) nd);
  bioem_hip_window_offsets(N, param.pd.maxDisplaceCenter, param.pd.GridSpaceCenter, algo, shifts.data(), nd);
  const size_t T = (size_t) nd * nd;
  std::vector<bioem_hip_window_request> req;
  for_each_match(pmap, nMaps, "RefMap %d has no member in the soft reconstruction: no run compared it",
                 [&](int p, const bioem_hip_prob_map &r) {
                   for (int k = 0; k < K; k++)
                   {
                     const int o = K == 1 ? r.max_prob_orient : cand[(size_t) p * Kang + k].orient;
                     for (int c = 0; c < nC && o >= 0 && o < nA; c++)
                       req.push_back({p, o, c});
                   }
                 });
  if (req.empty())
    fatal("--ReconstructSoft: no particle has a record to reconstruct from");
  const size_t n = req.size();
  std::vector<float> sumRef((size_t) nMaps), sumsqRef((size_t) nMaps);
  check(h, bioem_hip_debug_particles(h, nullptr, sumRef.data(), sumsqRef.data()), "particle sums");
  // t = logp + log prior, norm and mu of every cell; a cell where one of them is not finite has t = -inf
  std::vector<double> t(n * T), norm(n * T), mu(n * T);
  {
    const int batch = batch_size(h);
    std::vector<float> cc((size_t) batch * T);
    std::vector<bioem_hip_param5> par((size_t) batch);
    const double Ntotpi = (double) param.pd.Ntotpi;
    for (size_t i0 = 0; i0 < n; i0 += (size_t) batch)
    {
      const int nb = (int) std::min((size_t) batch, n - i0);
      check(h, bioem_hip_window_posterior(h, req.data() + i0, nb, 0, t.data() + i0 * T, cc.data(), par.data()), "window posterior");
      for (int i = 0; i < nb; i++)
      {
        const bioem_hip_window_request &q = req[i0 + (size_t) i];
        const double sumC = (double) par[(size_t) i].sumC, sumsqC = (double) par[(size_t) i].sumsquareC;
        const double sumref = (double) sumRef[(size_t) q.particle], d = sumC * sumC - sumsqC * Ntotpi;
        const double prior = param.yespriorAngles ? (double) param.angprior[(size_t) q.orient] : 0.;
        for (size_t c = 0; c < T; c++)
        {
          const size_t e = (i0 + (size_t) i) * T + c;
          const double value = (double) cc[(size_t) i * T + c];
          norm[e] = -(-sumC * sumref + Ntotpi * value) / d;
          mu[e] = -(-sumC * value + sumsqC * sumref) / d;
          t[e] += prior;
          if (!std::isfinite(t[e]) || !std::isfinite(norm[e]) || !std::isfinite(mu[e]))
            t[e] = -INFINITY;
        }
      }
    }
  }
  // per particle (its requests are consecutive): the weights over all cells of all its requests, the members, the summary
  std::vector<bioem_hip_soft_member> members(n);
  std::vector<double> cells(n * T, 0.), nEff((size_t) nMaps, 0.), wMax((size_t) nMaps, 0.);
  std::vector<int> nReq((size_t) nMaps, 0);
  for (size_t r0 = 0; r0 < n;)
  {
    size_t r1 = r0;
    while (r1 < n && req[r1].particle == req[r0].particle)
      r1++;
    const int p = req[r0].particle;
    double top = -INFINITY, Z = 0., s2w = 0.;
    for (size_t e = r0 * T; e < r1 * T; e++)
      top = std::max(top, t[e]);
    for (size_t e = r0 * T; e < r1 * T && top > -INFINITY; e++)
      Z += t[e] > -INFINITY ? std::exp(t[e] - top) : 0.;
    for (size_t r = r0; r < r1; r++)
    {
      bioem_hip_soft_member m = {p, top > -INFINITY ? req[r].orient : -1, req[r].conv, 0, 0., 0., 0.};
      for (size_t e = r * T; e < (r + 1) * T && top > -INFINITY; e++)
      {
        const double w = t[e] > -INFINITY ? std::exp(t[e] - top) / Z : 0.;
        if (w > 0.)
        {
          cells[e] = w * norm[e];
          m.s2 += w * norm[e] * norm[e];
          m.b += w * norm[e] * mu[e];
          m.mass += w;
          s2w += w * w;
          wMax[(size_t) p] = std::max(wMax[(size_t) p], w);
        }
      }
      members[r] = m;
    }
    nReq[(size_t) p] = (int) (r1 - r0);
    nEff[(size_t) p] = s2w > 0. ? 1. / s2w : 0.;
    r0 = r1;
  }
  std::vector<int> groupOrient((size_t) nA);
  for (int o = 0; o < nA; o++)
    groupOrient[(size_t) o] = o;
  std::vector<float> vol(N3);
  std::vector<double> spec[2] = {std::vector<double>(2 * V), std::vector<double>(2 * V)};
  std::vector<bioem_hip_soft_member> half;
  double stats[4] = {0., 0., 0., 0.}, hs[4];
  const std::string names[3] = {file + "_soft.mrc", file + "_soft_half1.mrc", file + "_soft_half2.mrc"};
  for (int k = 0; k < 3; k++)
  { // k = 0: every particle; 1, 2: the even and the odd ones (the others are left out)
    half = members;
    for (size_t r = 0; r < n && k; r++)
      if (half[r].particle % 2 != k - 1)
        half[r].group = -1;
    check(h, bioem_hip_reconstruct_soft(h, half.data(), cells.data(), (int) n, shifts.data(), nd, groupOrient.data(), nA,
                                        reconWiener, BIOEM_HIP_RECON_CORRECT, vol.data(), k ? spec[k - 1].data() : nullptr, nullptr,
                                        k ? hs : stats),
          "soft reconstruction");
    const std::string err = write_mrc_volume(names[k].c_str(), vol.data(), N, param.pixelSize);
    if (!err.empty())
      fatal("--ReconstructSoft: %s", err.c_str());
  }
  std::vector<double> weight, cross, pa, pb;
  recon_shell_sums(spec[0].data(), spec[1].data(), N, weight, cross, pa, pb);
  const std::string err = append_reconstruction_soft(file.c_str(), nReq.data(), nEff.data(), wMax.data(), nMaps, weight, cross,
                                                     pa, pb, N, param.pixelSize);
  if (!err.empty())
    fatal("--ReconstructSoft: %s", err.c_str());
  std::cout << "Soft reconstruction (" << K << " orientation" << (K > 1 ? "s" : "") << " per particle) from " << (long long) stats[1]
            << " members in " << (long long) stats[0] << " views written to: " << file << ", " << names[0] << ", " << names[1]
            << ", " << names[2] << "\n";
}

// --BestWindow: the window table of every record's (orientation, CTF) pair from handle h, batch by batch, then the text
// file (write_best_window).  A particle no run compared has no record: a warning and an empty block.
void Driver::writeBestWindow(const std::string &file, bioem_hip_handle h, const bioem_hip_prob_map *pmap, int ownLists,
                             const bioem_hip_param_device &pd, const float *voluPerMap)
{
  const int nMaps = particles.ntot;
  const int nd = bioem_hip_window_count(pd.NumberPixels, pd.maxDisplaceCenter, pd.GridSpaceCenter, algo);
  if (nd < 1)
    fatal("--BestWindow: no displacement window for these parameters");
  std::vector<int> shifts((size_t) nd);
  bioem_hip_window_offsets(pd.NumberPixels, pd.maxDisplaceCenter, pd.GridSpaceCenter, algo, shifts.data(), nd);
  const size_t cells = (size_t) nd * nd;
  const int batch = batch_size(h);
  std::vector<double> logp(cells * (size_t) nMaps, 0.), table(cells * (size_t) batch), numconst((size_t) nMaps);
  std::vector<int> orient((size_t) nMaps, -1), conv((size_t) nMaps, 0), who;
  std::vector<bioem_hip_window_request> req;
  auto flush = [&]() {
    if (req.empty())
      return;
    check(h, bioem_hip_window_posterior(h, req.data(), (int) req.size(), ownLists, table.data(), nullptr, nullptr),
          "window posterior");
    for (size_t i = 0; i < req.size(); i++)
      std::copy(table.begin() + cells * i, table.begin() + cells * (i + 1), logp.begin() + cells * (size_t) who[i]);
    req.clear();
    who.clear();
  };
  for (int p = 0; p < nMaps; p++)
    numconst[(size_t) p] = numconst_of(pd.Ntotpi, voluPerMap ? voluPerMap[p] : pd.volu);
  for_each_match(pmap, nMaps, "window of RefMap %d not computed: no run compared it", [&](int p, const bioem_hip_prob_map &r) {
    orient[(size_t) p] = r.max_prob_orient;
    conv[(size_t) p] = r.max_prob_conv;
    req.push_back({p, r.max_prob_orient, r.max_prob_conv});
    who.push_back(p);
    if ((int) req.size() == batch)
      flush();
  });
  flush();
  const std::string err = write_best_window(file.c_str(), logp.data(), shifts.data(), nd, nMaps, orient.data(), conv.data(),
                                            param.ctfParam.data(), param.usepsf, param.elecwavel, numconst.data());
  if (!err.empty())
    fatal("--BestWindow: %s", err.c_str());
  std::cout << "Window posterior of " << nMaps << " particles' best matches written to: " << file << "\n";
}

// --CTFScan: every record's (orientation, shift) from handle h against the parameter file's CTF grid refined
// ctfScanFactor-fold, the candidates' kernels made on the host as the run's are and scanned in chunks of at most 256
// (bioem_hip_ctf_scan), then the text file (write_ctf_scan).  A particle no run compared has no record: a warning and an
// empty block.
void Driver::writeCtfScan(const std::string &file, bioem_hip_handle h, const bioem_hip_prob_map *pmap, int ownLists,
                          const bioem_hip_param_device &pd, const float *voluPerMap)
{
  const int nMaps = particles.ntot, N = param.N;
  const float start[3] = {param.startGridCTF_amp, param.startGridCTF_phase, param.startGridEnvelop};
  const float step[3] = {param.gridCTF_amp, param.gridCTF_phase, param.gridEnvelop};
  const int n[3] = {param.numberGridPointsCTF_amp, param.numberGridPointsCTF_phase, param.numberGridPointsEnvelop};
  int counts[3];
  const int G = ctf_scan_refine(start, step, n, ctfScanFactor, counts, nullptr);
  if (G < 1 || G > kCtfScanMaxCandidates)
    fatal("--CTFScan: %d candidate CTF sets", G);
  std::vector<float> triples(3 * (size_t) G);
  ctf_scan_refine(start, step, n, ctfScanFactor, counts, triples.data());
  std::vector<double> logp((size_t) G * nMaps, 0.), numconst((size_t) nMaps);
  std::vector<int> orient((size_t) nMaps, -1), shiftX((size_t) nMaps, 0), shiftY((size_t) nMaps, 0), who;
  std::vector<bioem_hip_scan_request> req;
  for (int p = 0; p < nMaps; p++)
    numconst[(size_t) p] = numconst_of(pd.Ntotpi, voluPerMap ? voluPerMap[p] : pd.volu);
  for_each_match(pmap, nMaps, "CTF scan of RefMap %d not computed: no run compared it", [&](int p, const bioem_hip_prob_map &r) {
    orient[(size_t) p] = r.max_prob_orient;
    shiftX[(size_t) p] = r.max_prob_cent_x;
    shiftY[(size_t) p] = r.max_prob_cent_y;
    req.push_back({p, r.max_prob_orient, r.max_prob_cent_x, r.max_prob_cent_y});
    who.push_back(p);
  });
  const int chunk = 256;
  const size_t M = (size_t) N * (N / 2 + 1);
  std::vector<float> kernels(2 * M * (size_t) std::min(chunk, G));
  std::vector<double> table(req.size() * (size_t) std::min(chunk, G));
  for (int g0 = 0; g0 < G && !req.empty(); g0 += chunk)
  {
    const int nG = std::min(chunk, G - g0);
    ctf_kernel_list(N, param.pixelSize, param.usepsf, triples.data() + 3 * (size_t) g0, nG, kernels.data(), param.r2c,
                    param.r2c_ctx);
    check(h, bioem_hip_ctf_scan(h, req.data(), (int) req.size(), ownLists, kernels.data(), triples.data() + 3 * (size_t) g0, nG,
                                table.data(), nullptr, nullptr),
          "CTF scan");
    for (size_t i = 0; i < req.size(); i++)
      std::copy(table.begin() + (size_t) nG * i, table.begin() + (size_t) nG * (i + 1),
                logp.begin() + (size_t) G * (size_t) who[i] + (size_t) g0);
  }
  const std::string err = write_ctf_scan(file.c_str(), logp.data(), triples.data(), counts, nMaps, orient.data(), shiftX.data(),
                                         shiftY.data(), param.usepsf, param.elecwavel, numconst.data());
  if (!err.empty())
    fatal("--CTFScan: %s", err.c_str());
  std::cout << "CTF scan of " << nMaps << " particles' best matches over " << G << " candidate sets written to: " << file
            << "\n";
}

// --ModelGradient: the gradient of the log posterior of every record (orientation, CTF set, shift) from handle h with
// respect to the density of every model point, summed over the particles with weight 1 (bioem_hip_model_gradient), then
// the text file (write_model_gradient).  A particle no run compared has no record: a warning, and it adds nothing.
void Driver::writeModelGradient(const std::string &file, bioem_hip_handle h, const bioem_hip_prob_map *pmap, int ownLists)
{
  const int nMaps = particles.ntot;
  std::vector<bioem_hip_grad_request> req;
  for_each_match(pmap, nMaps, "Density gradient of RefMap %d not computed: no run compared it",
                 [&](int p, const bioem_hip_prob_map &r) {
                   req.push_back({p, r.max_prob_orient, r.max_prob_conv, r.max_prob_cent_x, r.max_prob_cent_y});
                 });
  std::vector<bioem_hip_grad_point> acc(model.points.size(), bioem_hip_grad_point{0., 0., 0., 0});
  std::vector<double> coef(4 * req.size());
  if (!req.empty())
    check(h, bioem_hip_model_gradient(h, req.data(), nullptr, (int) req.size(), ownLists, nullptr, acc.data(), nullptr, coef.data()),
          "model gradient");
  int nonfinite = 0;
  for (size_t i = 0; i < req.size(); i++)
    nonfinite += !(std::isfinite(coef[4 * i]) && std::isfinite(coef[4 * i + 1]) && std::isfinite(coef[4 * i + 2]));
  const std::string err = write_model_gradient(file.c_str(), model.points.data(), acc.data(), (int) model.points.size(), nonfinite);
  if (!err.empty())
    fatal("--ModelGradient: %s", err.c_str());
  std::cout << "Density gradient of " << req.size() << " particles' best matches over " << model.points.size()
            << " model points written to: " << file << "\n";
}

// --VolumeGradient: the gradient of the log posterior of every record from handle h with respect to every voxel of the
// volume model, summed over the particles with weight 1 (bioem_hip_volume_gradient), then the MRC volume and the text file
void Driver::writeVolumeGradient(const std::string &file, bioem_hip_handle h, const bioem_hip_prob_map *pmap, int ownLists)
{
  const int nMaps = particles.ntot, N = param.N;
  std::vector<bioem_hip_grad_request> req;
  for_each_match(pmap, nMaps, "Density gradient of RefMap %d not computed: no run compared it",
                 [&](int p, const bioem_hip_prob_map &r) {
                   req.push_back({p, r.max_prob_orient, r.max_prob_conv, r.max_prob_cent_x, r.max_prob_cent_y});
                 });
  const size_t NNN = (size_t) N * N * N;
  std::vector<double> gvol(NNN, 0.);
  double stats[3] = {0., 0., 0.};
  if (!req.empty())
    check(h, bioem_hip_volume_gradient(h, req.data(), nullptr, (int) req.size(), ownLists, gvol.data(), nullptr, nullptr, nullptr,
                                       stats),
          "volume gradient");
  std::vector<float> gf(NNN);
  for (size_t e = 0; e < NNN; e++)
    gf[e] = (float) gvol[e];
  std::string err = write_mrc_volume((file + ".mrc").c_str(), gf.data(), N, param.pixelSize);
  if (err.empty())
    err = write_volume_gradient(file.c_str(), gvol.data(), model.volume.data(), N, (int) req.size(), stats[1], (int) stats[2]);
  if (!err.empty())
    fatal("--VolumeGradient: %s", err.c_str());
  std::cout << "Density gradient of " << req.size() << " particles' best matches over the " << N << "^3 voxels of the model written "
            << "to: " << file << " and " << file << ".mrc\n";
}

// --PoseGradient: the gradient of the log posterior of every record from handle h with respect to rows 0 and 1 of its
// orientation matrix and to the model shifts (bioem_hip_pose_gradient), then the text file (write_pose_gradient)
void Driver::writePoseGradient(const std::string &file, bioem_hip_handle h, const bioem_hip_prob_map *pmap, int ownLists,
                               const float *angles, size_t anglesPerMap, const long long *angleOffsets)
{
  const int nMaps = particles.ntot;
  std::vector<bioem_hip_grad_request> req;
  std::vector<float> quats;
  for_each_match(pmap, nMaps, "Pose gradient of RefMap %d not computed: no run compared it",
                 [&](int p, const bioem_hip_prob_map &r) {
                   req.push_back({p, r.max_prob_orient, r.max_prob_conv, r.max_prob_cent_x, r.max_prob_cent_y});
                   const size_t first = !ownLists ? 0 : angleOffsets ? (size_t) angleOffsets[p] : anglesPerMap * (size_t) p;
                   const float *q = angles + 4 * (first + (size_t) r.max_prob_orient);
                   quats.insert(quats.end(), q, q + 4);
                 });
  std::vector<double> rows(18 * req.size());
  if (!req.empty())
    check(h, bioem_hip_pose_gradient(h, req.data(), (int) req.size(), ownLists, rows.data(), nullptr, nullptr), "pose gradient");
  const std::string err = write_pose_gradient(file.c_str(), rows.data(), req.data(), quats.data(), (int) req.size());
  if (!err.empty())
    fatal("--PoseGradient: %s", err.c_str());
  std::cout << "Pose gradient of " << req.size() << " particles' best matches written to: " << file << "\n";
}

// --CTFGradient: gradient and curvature of the log posterior of every record from handle h with respect to the triple of its
// CTF set (bioem_hip_ctf_gradient), then the text file (write_ctf_gradient)
void Driver::writeCtfGradient(const std::string &file, bioem_hip_handle h, const bioem_hip_prob_map *pmap, int ownLists)
{
  const int nMaps = particles.ntot;
  std::vector<bioem_hip_grad_request> req;
  for_each_match(pmap, nMaps, "CTF gradient of RefMap %d not computed: no run compared it",
                 [&](int p, const bioem_hip_prob_map &r) {
                   req.push_back({p, r.max_prob_orient, r.max_prob_conv, r.max_prob_cent_x, r.max_prob_cent_y});
                 });
  std::vector<double> rows(38 * req.size());
  if (!req.empty())
    check(h, bioem_hip_ctf_gradient(h, req.data(), (int) req.size(), ownLists, param.pixelSize, rows.data(), nullptr, nullptr),
          "CTF gradient");
  const std::string err = write_ctf_gradient(file.c_str(), rows.data(), req.data(), (int) req.size(), param.elecwavel);
  if (!err.empty())
    fatal("--CTFGradient: %s", err.c_str());
  std::cout << "CTF gradient of " << req.size() << " particles' best matches written to: " << file << "\n";
}

// every shard's sums over the orientations it owns under logPrior (bioem_hip_orientation_sums), merged on the host in
// shard order
void Driver::shardOrientSums(const double *logPrior, std::vector<bioem_hip_orient_sums> &sums)
{
  const int nMaps = particles.ntot, nShards = (int) shards.size();
  std::vector<std::vector<bioem_hip_orient_sums>> part((size_t) nShards);
  std::vector<const bioem_hip_orient_sums *> ptrs((size_t) nShards);
  for (int g = 0; g < nShards; g++)
  {
    part[(size_t) g].resize((size_t) nMaps);
    check(shards[g].h, bioem_hip_orientation_sums(shards[g].h, logPrior, 0, nMaps, 0, part[(size_t) g].data()), "orientation sums");
    ptrs[(size_t) g] = part[(size_t) g].data();
  }
  sums.resize((size_t) nMaps);
  if (bioem_hip_merge_orient_sums_host(nShards, nMaps, ptrs.data(), sums.data()))
    fatal("merge failed");
}

// --OrientStats: the shards' merged sums (shardOrientSums), then the text file (write_orient_stats)
void Driver::writeOrientStats(const std::string &file, double numconst)
{
  const int nMaps = particles.ntot;
  std::vector<double> prior;
  if (param.yespriorAngles)
    prior.assign(param.angprior.begin(), param.angprior.end());
  std::vector<bioem_hip_orient_sums> sums;
  shardOrientSums(prior.empty() ? nullptr : prior.data(), sums);
  const std::string err = write_orient_stats(file.c_str(), sums.data(), nMaps, param.angles.data(), nullptr, param.doquater, numconst);
  if (!err.empty())
    fatal("--OrientStats: %s", err.c_str());
  std::cout << "Orientation posterior summaries of " << nMaps << " particles written to: " << file << "\n";
}

// one pass of --OrientOccupancy under logPrior: every shard's sums over the orientations it owns merged on the host in
// shard order (as --OrientStats does), then every shard's occupancy block under the merged sums, in block order
void Driver::orientOccupancyPass(const double *logPrior, std::vector<bioem_hip_orient_sums> &sums, std::vector<bioem_hip_orient_occ> &occ)
{
  const int nMaps = particles.ntot, nShards = (int) shards.size(), nO = param.nTotGridAngles;
  shardOrientSums(logPrior, sums);
  occ.assign((size_t) nO, bioem_hip_orient_occ());
  for (int g = 0; g < nShards; g++)
  {
    if (shards[g].o0 < 0 || shards[g].o1 > nO || shards[g].o0 >= shards[g].o1)
      fatal("--OrientOccupancy: a shard without an orientation block");
    check(shards[g].h, bioem_hip_orientation_occupancy(shards[g].h, logPrior, sums.data(), 0, nMaps, occ.data() + shards[g].o0),
          "orientation occupancy");
  }
}

// --OrientOccupancy: the pass under the run's prior (param.angprior under PRIOR_ANGLES) written as OCC / DATASET lines;
// --FitOrientPrior N: N EM iterations pi <- occ / nCounted from the run's prior normalised (uniform without one), one FIT
// line each, the last update written as FILE_prior
void Driver::writeOrientOccupancy(const std::string &file, int nIter)
{
  const int nO = param.nTotGridAngles;
  std::vector<double> prior;
  if (param.yespriorAngles)
    prior.assign(param.angprior.begin(), param.angprior.end());
  std::vector<bioem_hip_orient_sums> sums;
  std::vector<bioem_hip_orient_occ> occ, occIt;
  orientOccupancyPass(prior.empty() ? nullptr : prior.data(), sums, occ);
  auto counted = [](const std::vector<bioem_hip_orient_sums> &s) {
    long long n = 0;
    for (const bioem_hip_orient_sums &x : s)
      n += x.count > 0. && x.S0 > 0.;
    return n;
  };
  const long long nCounted = counted(sums);
  std::vector<OccFit> fits;
  if (nIter > 0)
  {
    std::vector<double> lp((size_t) nO, -log((double) nO));
    if (!prior.empty())
    { // the run's prior minus its log-sum-exp
      double top = prior[0], s = 0.;
      for (double v : prior)
        top = std::max(top, v);
      for (double v : prior)
        s += exp(v - top);
      for (int o = 0; o < nO; o++)
        lp[(size_t) o] = std::max(kOrientPriorFloor, prior[(size_t) o] - (top + log(s)));
    }
    for (int t = 0; t < nIter; t++)
    {
      orientOccupancyPass(lp.data(), sums, occIt);
      OccFit f = {0., log_prior_views(lp.data(), nO)};
      for (const bioem_hip_orient_sums &x : sums)
        if (x.count > 0. && x.S0 > 0.)
          f.logLikelihood += x.m + log(x.S0);
      fits.push_back(f);
      occ_next_prior(occIt.data(), nO, counted(sums), lp.data());
    }
    const std::string perr = write_orient_prior((file + "_prior").c_str(), param.angles.data(), nO, param.doquater, lp.data());
    if (!perr.empty())
      fatal("--FitOrientPrior: %s", perr.c_str());
    std::cout << "Orientation prior after " << nIter << " EM iterations written to: " << file << "_prior\n";
  }
  const std::string err = write_orient_occupancy(file.c_str(), occ.data(), nO, param.angles.data(), param.doquater, nCounted,
                                                 fits.data(), (int) fits.size());
  if (!err.empty())
    fatal("--OrientOccupancy: %s", err.c_str());
  std::cout << "Occupancy of " << nO << " orientations over " << nCounted << " particles written to: " << file << "\n";
}

// --PrintBestCalMap: the record of the BEST_* file rendered on the device and written as the reference's BESTMAP text.
// The reference's file labels the UNSHIFTED map with shifted coordinates (bioem.cpp:2049-2053), so the device renders with
// X = Y = 0 and the writer applies BEST_DX / BEST_DY to the labels.
int Driver::printBestCalMap()
{
  std::cout << "\nAnalysis for printing best projection::: \n \n";
  const int N = param.N;
  bioem_hip_handle h = nullptr;
  check(h, bioem_hip_create(&h, firstDev, &param.pd, 1, 1, 1, algo), "bioem_hip_create");
  check(h, bioem_hip_upload_ctf(h, param.refCTF.data(), param.ctfParam.data()), "upload CTF");
  check(h, model.upload(h, param),
        "upload model");
  check(h, bioem_hip_upload_orientations(h, param.angles.data(), 1, param.doquater ? 1 : 0), "upload orientations");
  bioem_hip_prob_map rec;
  memset(&rec, 0, sizeof(rec));
  rec.max_prob_norm = best.norm;
  rec.max_prob_mu = best.offset;
  std::vector<float> map((size_t) N * N);
  std::cout << "...... Calculating Projection and Convolution on the device .......................\n ";
  check(h, bioem_hip_render_best_maps(h, &rec, 0, 0, 1, map.data()), "render best map");
  bioem_hip_destroy(h);
  if (best.withnoise)
  { // N(0, stnoise) per pixel, seeded by the time like the reference's generator: maps of different runs are uncorrelated
    std::mt19937 gen((unsigned int) std::time(nullptr));
    std::normal_distribution<float> noise(0.f, best.stnoise);
    for (float &v : map)
      v = v + noise(gen);
  }
  if (!write_bestmap_text("BESTMAP", map.data(), N, best.ddx, best.ddy, best.withnoise))
    fatal("Writing BESTMAP");
  std::cout << "\n\nBest map printed in file: BESTMAP with gnuplot format in columns 2, 3 and 4. \n\n\n";
  return 0;
}

int Driver::run()
{
  if (!bestParamFile.empty())
    return printBestCalMap();
  printf("\tInitializing Probabilities\n");
  const int nMaps = particles.ntot, nAngles = param.nTotGridAngles, nC = param.nTotCTFs;
  const int nShards = (int) shards.size();
  const int K = param.pd.writeAngles;
  const double numconst = numconst_of(param.pd.Ntotpi, param.pd.volu);
  // per shard: the host block start_run / finish_run move -- map entries only for orientation-block shards, map
  // entries + the (tiny) full angle table when the CTF grid is split
  const size_t bytes = splitCTF ? bioem_hip_prob_size(nMaps, nAngles, K) : bioem_hip_prob_size(nMaps, 0, 0);
  for (Shard &sh : shards)
  {
    void *p = bioem_hip_host_alloc(bytes); // == bioem::malloc_device_host (map.cpp:637)
    if (!p)
      fatal("Memory allocation");
    sh.prob = p;
    bioem_hip_prob_map *pm = (bioem_hip_prob_map *) p;
    for (int i = 0; i < nMaps; i++) // bioem.cpp:681-699
    {
      memset(&pm[i], 0, sizeof(pm[i]));
      pm[i].Total = 0.0;
      pm[i].Constoadd = -999999.;
    }
    if (K && splitCTF)
    {
      bioem_hip_prob_angle *pa = (bioem_hip_prob_angle *) (pm + nMaps);
      for (size_t e = 0; e < (size_t) nMaps * nAngles; e++)
      {
        pa[e].forAngles = 0.0;
        pa[e].ConstAngle = -999999.;
      }
    }
  }
  if (debugOutput >= 1)
    printf("\tMain Loop GridAngles %d, CTFs %d, RefMaps %d, Shifts (%d/%d)², Pixels %d², Shards %d%s, merge %s\n", nAngles,
           nC, nMaps, 2 * param.pd.maxDisplaceCenter + param.pd.GridSpaceCenter, param.pd.GridSpaceCenter, param.N,
           nShards, splitCTF ? " (orientation x CTF split)" : "", useRccl ? "RCCL" : "host");
  std::vector<std::thread> th;
  std::vector<std::string> errs(nShards);
  for (int g = 0; g < nShards; g++)
  {
    th.emplace_back([&, g]() {
      Shard &sh = shards[g];
      bioem_hip_handle h = sh.h;
      int rc = bioem_hip_set_phase_timing(h, debugOutput >= 1);
      if (!rc)
        rc = bioem_hip_start_run(h, sh.prob);
      if (!rc && !splitCTF)
        rc = bioem_hip_project_convolve_compare(h, sh.o0, sh.o1);
      // CTF split: the shard's run of (orientation, CTF) pairs, one rectangle per orientation it touches
      for (long long u = sh.u0; !rc && splitCTF && u < sh.u1;)
      {
        const int o = (int) (u / nC), c0 = (int) (u % nC);
        const int c1 = (int) std::min<long long>(nC, c0 + (sh.u1 - u));
        rc = bioem_hip_project_convolve_compare_ctf(h, o, o + 1, c0, c1);
        u += c1 - c0;
      }
      if (!rc)
        rc = bioem_hip_finish_run(h, sh.prob);
      if (rc)
        errs[g] = bioem_hip_last_error(h);
    });
  }
  for (auto &t : th)
    t.join();
  for (int g = 0; g < nShards; g++)
    if (!errs[g].empty())
      fatal("shard %d: %s", g, errs[g].c_str());
  if (debugOutput >= 1)
    print_phase_report();

  // ---- the path's single exchange step: merge of the shards (bioem.cpp:909-1044) ----
  prob.assign(sizeof(bioem_hip_prob_map) * (size_t) nMaps, 0);
  cand.assign((size_t) nMaps * K, bioem_hip_angle_candidate());
  if (useRccl)
  { // one GPU per shard: all-gather over xGMI, fold on the first device
    std::vector<bioem_hip_handle> hs;
    for (Shard &sh : shards)
      hs.push_back(sh.h);
    check(hs[0], bioem_hip_merge(hs.data(), nShards, prob.data(), K, numconst, K ? cand.data() : nullptr), "RCCL merge");
  }
  else if (!splitCTF)
  {
    std::vector<const void *> blocks;
    for (Shard &sh : shards)
      blocks.push_back(sh.prob);
    if (bioem_hip_merge_host(nShards, nMaps, 0, 0, blocks.data(), prob.data()))
      fatal("merge failed");
    if (K)
    {
      // lists of 2K - 1: the K best and the tie candidates, so that the merge is the writer's walk over the whole table
      // whatever keys are equal (K-wide lists are not enough then)
      const int W = 2 * K - 1;
      std::vector<std::vector<bioem_hip_angle_candidate>> lists(nShards);
      std::vector<const bioem_hip_angle_candidate *> ptrs(nShards);
      for (int g = 0; g < nShards; g++)
      {
        lists[g].resize((size_t) nMaps * W);
        check(shards[g].h, bioem_hip_merge_candidates(shards[g].h, K, numconst, lists[g].data()), "top-K orientations");
        ptrs[g] = lists[g].data();
      }
      if (bioem_hip_merge_topk_host_wide(nShards, nMaps, K, W, ptrs.data(), cand.data()))
        fatal("merge failed");
    }
  }
  else
  { // CTF split: an orientation's angle entry is spread over shards -> log-sum-exp merge of the full tables, then the
    // writer's selection on the host (bioem.cpp:1251-1286)
    std::vector<unsigned char> full(bytes);
    std::vector<const void *> blocks;
    for (Shard &sh : shards)
      blocks.push_back(sh.prob);
    if (bioem_hip_merge_host(nShards, nMaps, nAngles, K, blocks.data(), full.data()))
      fatal("merge failed");
    memcpy(prob.data(), full.data(), prob.size());
    if (K)
    {
      const bioem_hip_prob_angle *pang = (const bioem_hip_prob_angle *) (full.data() + prob.size());
      typedef std::pair<double, int> Item;
      for (int i = 0; i < nMaps; i++)
      {
        std::priority_queue<Item, std::vector<Item>, std::greater<Item>> q;
        for (int io = 0; io < nAngles; io++)
        {
          const bioem_hip_prob_angle &pa = pang[(size_t) io * nMaps + i];
          const double logp = log(pa.forAngles) + pa.ConstAngle + numconst;
          if ((int) q.size() < K)
            q.push(Item(logp, io));
          else if (q.top().first < logp)
          {
            q.pop();
            q.push(Item(logp, io));
          }
        }
        const int cnt = (int) q.size();
        for (int r = 0; r < K; r++)
          cand[(size_t) i * K + r].orient = -1;
        for (int r = cnt - 1; r >= 0; r--)
        {
          const bioem_hip_prob_angle &pa = pang[(size_t) q.top().second * nMaps + i];
          bioem_hip_angle_candidate &c = cand[(size_t) i * K + r];
          c.forAngles = pa.forAngles;
          c.ConstAngle = pa.ConstAngle;
          c.logp = q.top().first;
          c.orient = q.top().second;
          q.pop();
        }
      }
    }
  }
  writeOutput();
  if (!probCtfFile.empty())
  { // the tables never go through RCCL: fetched from every handle and merged on the host, whatever carried the entries
    std::vector<bioem_hip_handle> hs;
    for (Shard &sh : shards)
      hs.push_back(sh.h);
    writeCtfProb(probCtfFile, hs, param.pd, param.angles.data(), 0);
  }
  if (!orientStatsFile.empty())
    writeOrientStats(orientStatsFile, numconst);
  if (!orientOccFile.empty())
    writeOrientOccupancy(orientOccFile, fitOrientPrior);
  if (!bestMapsFile.empty()) // from the merged records, on the first handle (every handle holds the global list)
    writeBestMaps(bestMapsFile, shards[0].h, (const bioem_hip_prob_map *) prob.data(), 0);
  if (!bestFrcFile.empty())
    writeBestFrc(bestFrcFile, shards[0].h, (const bioem_hip_prob_map *) prob.data(), 0);
  if (!bestWindowFile.empty())
    writeBestWindow(bestWindowFile, shards[0].h, (const bioem_hip_prob_map *) prob.data(), 0, param.pd);
  if (!ctfScanFile.empty())
    writeCtfScan(ctfScanFile, shards[0].h, (const bioem_hip_prob_map *) prob.data(), 0, param.pd);
  if (!modelGradFile.empty())
    writeModelGradient(modelGradFile, shards[0].h, (const bioem_hip_prob_map *) prob.data(), 0);
  if (!volGradFile.empty())
    writeVolumeGradient(volGradFile, shards[0].h, (const bioem_hip_prob_map *) prob.data(), 0);
  if (!poseGradFile.empty())
    writePoseGradient(poseGradFile, shards[0].h, (const bioem_hip_prob_map *) prob.data(), 0, param.angles.data(), 0);
  if (!ctfGradFile.empty())
    writeCtfGradient(ctfGradFile, shards[0].h, (const bioem_hip_prob_map *) prob.data(), 0);
  if (!viewAvgFile.empty())
    writeViewAverages(viewAvgFile, shards[0].h, (const bioem_hip_prob_map *) prob.data());
  if (!reconFile.empty())
    writeReconstruction(reconFile, shards[0].h, (const bioem_hip_prob_map *) prob.data());
  if (!reconFile.empty() && reconSoftK)
    writeReconstructionSoft(reconFile, shards[0].h, (const bioem_hip_prob_map *) prob.data());
  if (!refineFile.empty())
  {
    if (refineSeeds >= 2)
      runRound2Seeds();
    else
      runRound2();
  }
  return 0;
}

// Round 2 of the manual's model comparison (doc/index.rst, "modcom") in the same run: particle p is evaluated again on
// the list best_p (x) grid -- the Hamilton product in (x, y, z, w) storage, the model rotated by best_p first and the
// small rotation applied to the rotated model (bioem_amd/refine.py states and tests the convention) -- through the
// own-list pass of the engine on the first selected device.  The numbers of particle p are those of a run on that
// particle alone with its list through --ReadOrientation: volu of a list of G orientations (param.cpp:1131,1324).
void Driver::runRound2()
{
  const std::vector<float> &grid = refineGrid;
  const int G = (int) (grid.size() / 4), nMaps = particles.ntot, nC = param.nTotCTFs;
  std::cout << "Second round: " << G << " orientations per particle\n";
  const bioem_hip_prob_map *r1 = (const bioem_hip_prob_map *) prob.data();
  std::vector<float> lists((size_t) nMaps * G * 4);
  for (int i = 0; i < nMaps; i++)
  {
    const float *b = param.angles.data() + 4 * (size_t) r1[i].max_prob_orient;
    const double bx = b[0], by = b[1], bz = b[2], bw = b[3];
    for (int k = 0; k < G; k++)
    {
      const float *g = grid.data() + 4 * (size_t) k;
      float *o = lists.data() + ((size_t) i * G + k) * 4;
      if (g[0] == 0.f && g[1] == 0.f && g[2] == 0.f && g[3] == 1.f)
      { // the identity: the round-1 orientation itself, bit for bit
        memcpy(o, b, 4 * sizeof(float));
        continue;
      }
      const double gx = g[0], gy = g[1], gz = g[2], gw = g[3];
      const double q[4] = {bw * gx + bx * gw + by * gz - bz * gy, bw * gy - bx * gz + by * gw + bz * gx,
                           bw * gz + bx * gy - by * gx + bz * gw, bw * gw - bx * gx - by * gy - bz * gz};
      const double nrm = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
      for (int c = 0; c < 4; c++)
        o[c] = (float) (q[c] / nrm);
    }
  }
  bioem_hip_param_device pd2 = param.pd;
  pd2.writeAngles = 0;
  pd2.volu = volume_element((float) (1. / (float) G * param.priorMod), pd2.GridSpaceCenter, pd2.maxDisplaceCenter,
                            param.pixelSize, param.numberGridPointsCTF_amp, param.gridEnvelop, param.gridCTF_phase,
                            pd2.sigmaPriorbctf, pd2.sigmaPriordefo, pd2.sigmaPrioramp);
  bioem_hip_handle h = nullptr;
  check(h, bioem_hip_create(&h, firstDev, &pd2, nMaps, G, nC, algo), "bioem_hip_create (second round)");
  check(h, bioem_hip_upload_particle_maps(h, particles.maps.data()), "upload particles");
  check(h, bioem_hip_upload_ctf(h, param.refCTF.data(), param.ctfParam.data()), "upload CTF");
  check(h, model.upload(h, param),
        "upload model");
  check(h, bioem_hip_upload_particle_orientations(h, lists.data(), G, 1), "upload particle orientations");
  if (!probCtfFile.empty())
    check(h, bioem_hip_enable_ctf_table(h, 1), "enable CTF table");
  std::vector<bioem_hip_prob_map> pm(nMaps);
  for (int i = 0; i < nMaps; i++) // bioem.cpp:681-699
  {
    memset(&pm[i], 0, sizeof(pm[i]));
    pm[i].Total = 0.0;
    pm[i].Constoadd = -999999.;
  }
  check(h, bioem_hip_start_run(h, pm.data()), "start run (second round)");
  check(h, bioem_hip_compare_own_orientations(h, 0, nMaps), "compare own orientations");
  check(h, bioem_hip_finish_run(h, pm.data()), "finish run (second round)");
  if (!bestMapsFile.empty())
    writeBestMaps(bestMapsFile + "_Round2", h, pm.data(), 1);
  if (!bestFrcFile.empty())
    writeBestFrc(bestFrcFile + "_Round2", h, pm.data(), 1);
  if (!bestWindowFile.empty())
    writeBestWindow(bestWindowFile + "_Round2", h, pm.data(), 1, pd2);
  if (!ctfScanFile.empty())
    writeCtfScan(ctfScanFile + "_Round2", h, pm.data(), 1, pd2);
  if (!modelGradFile.empty())
    writeModelGradient(modelGradFile + "_Round2", h, pm.data(), 1);
  if (!volGradFile.empty())
    writeVolumeGradient(volGradFile + "_Round2", h, pm.data(), 1);
  if (!poseGradFile.empty())
    writePoseGradient(poseGradFile + "_Round2", h, pm.data(), 1, lists.data(), (size_t) G);
  if (!ctfGradFile.empty())
    writeCtfGradient(ctfGradFile + "_Round2", h, pm.data(), 1);
  if (!probCtfFile.empty())
    writeCtfProb(probCtfFile + "_Round2", std::vector<bioem_hip_handle>(1, h), pd2, lists.data(), (size_t) G);
  bioem_hip_destroy(h);
  writeProbabilities(outfileName + "_Round2", pm.data(), pd2, lists.data(), (size_t) G, false);
}

// best (x) grid: the Hamilton product in (x, y, z, w) storage, normalised; the identity of the grid gives `best` bit for bit
static void compose_list(const float *b, const std::vector<float> &grid, float *out)
{
  const int G = (int) (grid.size() / 4);
  const double bx = b[0], by = b[1], bz = b[2], bw = b[3];
  for (int k = 0; k < G; k++)
  {
    const float *g = grid.data() + 4 * (size_t) k;
    float *o = out + 4 * (size_t) k;
    if (g[0] == 0.f && g[1] == 0.f && g[2] == 0.f && g[3] == 1.f)
    {
      memcpy(o, b, 4 * sizeof(float));
      continue;
    }
    const double gx = g[0], gy = g[1], gz = g[2], gw = g[3];
    const double q[4] = {bw * gx + bx * gw + by * gz - bz * gy, bw * gy - bx * gz + by * gw + bz * gx,
                         bw * gz + bx * gy - by * gx + bz * gw, bw * gw - bx * gx - by * gy - bz * gz};
    const double nrm = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    for (int c = 0; c < 4; c++)
      o[c] = (float) (q[c] / nrm);
  }
}

// Round 2 around SEVERAL orientations per particle (--RefineSeeds M >= 2, --RefineLogWindow W): the seeds of particle p
// are the first of its M best orientations of round 1 (the ANG_PROB ranking: bioem_hip_topk_angles, or over shards the
// merge of the lists of bioem_hip_merge_candidates, which is that ranking under equal keys too) and those of the others whose log posterior lies within W of the first's, in that order; its list is the
// concatenation of seed (x) grid over its seeds, no duplicates removed (bioem_amd/refine.py: seed_lists).  The lists
// differ in length, and the line of particle p carries ITS constant: volu of a list of K_p orientations, what a run on
// that particle alone with its list through --ReadOrientation prints.
void Driver::runRound2Seeds()
{
  const std::vector<float> &grid = refineGrid;
  const int G = (int) (grid.size() / 4), nMaps = particles.ntot, nC = param.nTotCTFs, K = param.pd.writeAngles;
  std::vector<long long> offsets(1, 0);
  std::vector<float> lists;
  std::vector<float> volu(nMaps);
  int longest = 0;
  for (int i = 0; i < nMaps; i++)
  {
    int nSeeds = 0;
    double first = 0.;
    for (int r = 0; r < K && nSeeds < refineSeeds; r++)
    {
      const bioem_hip_angle_candidate &c = cand[(size_t) i * K + r];
      if (c.orient < 0)
        continue;
      if (nSeeds == 0)
        first = c.logp;
      else if (refineLogWindow >= 0. && !(c.logp >= first - refineLogWindow))
        continue;
      lists.resize(lists.size() + 4 * (size_t) G);
      compose_list(param.angles.data() + 4 * (size_t) c.orient, grid, lists.data() + lists.size() - 4 * (size_t) G);
      nSeeds++;
    }
    const int Kp = nSeeds * G;
    offsets.push_back(offsets.back() + Kp);
    longest = std::max(longest, Kp);
    volu[i] = volume_element((float) (1. / (float) std::max(1, Kp) * param.priorMod), param.pd.GridSpaceCenter,
                             param.pd.maxDisplaceCenter, param.pixelSize, param.numberGridPointsCTF_amp, param.gridEnvelop,
                             param.gridCTF_phase, param.pd.sigmaPriorbctf, param.pd.sigmaPriordefo, param.pd.sigmaPrioramp);
  }
  std::cout << "Second round: " << offsets.back() << " orientations for " << nMaps << " particles, " << G
            << " per seed, at most " << longest << " per particle\n";
  bioem_hip_param_device pd2 = param.pd;
  pd2.writeAngles = 0;
  bioem_hip_handle h = nullptr;
  check(h, bioem_hip_create(&h, firstDev, &pd2, nMaps, std::max(1, longest), nC, algo), "bioem_hip_create (second round)");
  check(h, bioem_hip_upload_particle_maps(h, particles.maps.data()), "upload particles");
  check(h, bioem_hip_upload_ctf(h, param.refCTF.data(), param.ctfParam.data()), "upload CTF");
  check(h, model.upload(h, param),
        "upload model");
  check(h, bioem_hip_upload_particle_orientation_lists(h, lists.data(), offsets.data(), 1), "upload particle orientation lists");
  if (!probCtfFile.empty())
    check(h, bioem_hip_enable_ctf_table(h, 1), "enable CTF table");
  std::vector<bioem_hip_prob_map> pm(nMaps);
  for (int i = 0; i < nMaps; i++) // bioem.cpp:681-699
  {
    memset(&pm[i], 0, sizeof(pm[i]));
    pm[i].Total = 0.0;
    pm[i].Constoadd = -999999.;
  }
  check(h, bioem_hip_start_run(h, pm.data()), "start run (second round)");
  check(h, bioem_hip_compare_own_orientations(h, 0, nMaps), "compare own orientations");
  check(h, bioem_hip_finish_run(h, pm.data()), "finish run (second round)");
  if (!bestMapsFile.empty())
    writeBestMaps(bestMapsFile + "_Round2", h, pm.data(), 1);
  if (!bestFrcFile.empty())
    writeBestFrc(bestFrcFile + "_Round2", h, pm.data(), 1);
  if (!bestWindowFile.empty())
    writeBestWindow(bestWindowFile + "_Round2", h, pm.data(), 1, pd2, volu.data());
  if (!ctfScanFile.empty())
    writeCtfScan(ctfScanFile + "_Round2", h, pm.data(), 1, pd2, volu.data());
  if (!modelGradFile.empty())
    writeModelGradient(modelGradFile + "_Round2", h, pm.data(), 1);
  if (!volGradFile.empty())
    writeVolumeGradient(volGradFile + "_Round2", h, pm.data(), 1);
  if (!poseGradFile.empty())
    writePoseGradient(poseGradFile + "_Round2", h, pm.data(), 1, lists.data(), 0, offsets.data());
  if (!ctfGradFile.empty())
    writeCtfGradient(ctfGradFile + "_Round2", h, pm.data(), 1);
  if (!probCtfFile.empty())
    writeCtfProb(probCtfFile + "_Round2", std::vector<bioem_hip_handle>(1, h), pd2, lists.data(), 0, offsets.data(),
                 volu.data());
  bioem_hip_destroy(h);
  writeProbabilities(outfileName + "_Round2", pm.data(), pd2, lists.data(), 0, false, offsets.data(), volu.data());
}

// --ProbCTF (layout: write_ctf_prob, bioem_host.h)
std::string write_ctf_prob(const char *file, const bioem_hip_prob_map *tab, int nCTF, int nMaps, const float *ctfParam3,
                           bool usepsf, float elecwavel, bool doquater, const float *angles, size_t anglesPerMap,
                           const long long *angleOffsets, float Ntotpi, float volu, const float *voluPerMap)
{
  char buf[200];
  for (int i = 0; i < nMaps; i++)
    for (int c = 0; c < nCTF; c++)
    {
      const bioem_hip_prob_map &e = tab[(size_t) c * nMaps + i];
      if (!has_record(e))
      {
        snprintf(buf, sizeof(buf), "RefMap %d has no comparison under CTF set %d: its entry of the CTF table is untouched", i, c);
        return buf;
      }
    }
  const char *bar = "************************* HEADER:: NOTATION *******************************************\n";
  std::ofstream out;
  out.precision(4);
  out.setf(std::ios::fixed);
  out.open(file);
  out << bar;
  out << " RefMap:  MapNumber - CTF set ; " << (usepsf ? "PSF amp - PSF phase - PSF envelope" : "CTF amp - CTF defocus [micro-m] - CTF B-Env")
      << " - logP - cal log Probability + Constant: Numerical Const. + log (volume) ; Best: "
      << (doquater ? "q1 - q2 - q3 - q4" : "alpha[rad] - beta[rad] - gamma[rad]")
      << " - center x - center y - normalization - offsett\n";
  out << bar;
  for (int i = 0; i < nMaps; i++)
  {
    // the constant of this map's LogProb line (Driver::writeProbabilities), by the same expressions
    const double numconst = numconst_of(Ntotpi, voluPerMap ? voluPerMap[i] : volu);
    const float *A = angles + 4 * (angleOffsets ? (size_t) angleOffsets[i] : anglesPerMap * (size_t) i); // this map's list
    for (int c = 0; c < nCTF; c++)
    {
      const bioem_hip_prob_map &pm = tab[(size_t) c * nMaps + i];
      const double lp = log(pm.Total) + pm.Constoadd + 0.5 * log(M_PI) + (1 - Ntotpi * 0.5) * (log(2 * M_PI) + 1) +
                        log(voluPerMap ? voluPerMap[i] : volu);
      const float *k = ctfParam3 + 3 * (size_t) c;
      const float *a = A + 4 * (size_t) pm.max_prob_orient;
      out << " " << i << " " << c << " " << k[0] << " ";
      if (!usepsf)
        out << k[1] / 2.f / M_PI / elecwavel * 0.0001 << " " << k[2] << " ";
      else
        out << k[1] << " " << k[2] << " ";
      out << lp << " Separated: " << log(pm.Total) << " " << pm.Constoadd << " " << numconst << " Best: " << a[0] << " "
          << a[1] << " " << a[2] << " ";
      if (doquater)
        out << a[3] << " ";
      out << pm.max_prob_cent_x << " " << pm.max_prob_cent_y << " " << pm.max_prob_norm << " " << pm.max_prob_mu << "\n";
    }
  }
  out.close();
  if (!out)
    return std::string("Writing ") + file;
  return "";
}

void Driver::writeCtfProb(const std::string &file, const std::vector<bioem_hip_handle> &hs, const bioem_hip_param_device &pd,
                          const float *angles, size_t anglesPerMap, const long long *angleOffsets, const float *voluPerMap)
{
  const int nMaps = particles.ntot, nC = param.nTotCTFs;
  const size_t n = (size_t) nC * nMaps;
  std::vector<std::vector<bioem_hip_prob_map>> tabs(hs.size(), std::vector<bioem_hip_prob_map>(n));
  std::vector<const void *> ptrs;
  for (size_t g = 0; g < hs.size(); g++)
  {
    check(hs[g], bioem_hip_ctf_table(hs[g], tabs[g].data()), "CTF table");
    ptrs.push_back(tabs[g].data());
  }
  std::vector<bioem_hip_prob_map> merged(n);
  if (bioem_hip_merge_host((int) hs.size(), (int) n, 0, 0, ptrs.data(), merged.data()))
    fatal("merge failed");
  const std::string err = write_ctf_prob(file.c_str(), merged.data(), nC, nMaps, param.ctfParam.data(), param.usepsf,
                                         param.elecwavel, param.doquater, angles, anglesPerMap, angleOffsets, pd.Ntotpi,
                                         pd.volu, voluPerMap);
  if (!err.empty())
    fatal("--ProbCTF: %s", err.c_str());
  std::cout << "Posterior per CTF set of " << nMaps << " particles x " << nC << " CTF sets written to: " << file << "\n";
}

void Driver::cleanup()
{
  for (Shard &sh : shards)
  {
    bioem_hip_host_free(sh.prob);
    if (sh.h)
      bioem_hip_destroy(sh.h);
  }
  shards.clear();
}

// Output_Probabilities and ANG_PROB, text layout of bioem.cpp:1047-1374 (fixed, 4 decimals).
void Driver::writeOutput()
{
  // (--RefineSeeds >= 2 set writeAngles for the seed selection: no ANG_PROB then)
  writeProbabilities(outfileName, (const bioem_hip_prob_map *) prob.data(), param.pd, param.angles.data(), 0,
                     refineSeeds < 2);
}

// angles: the list max_prob_orient indexes -- one for all maps (anglesPerMap = 0) or anglesPerMap entries per map (the
// second round); angProb: ANG_PROB is written beside it when pd.writeAngles asks for it
void Driver::writeProbabilities(const std::string &file, const bioem_hip_prob_map *pmap, const bioem_hip_param_device &pd,
                                const float *angles, size_t anglesPerMap, bool angProb, const long long *angleOffsets,
                                const float *voluPerMap)
{
  const int nMaps = particles.ntot;
  const bool writeAng = angProb && pd.writeAngles;
  const double numconst = numconst_of(pd.Ntotpi, pd.volu);
  const char *bar = "************************* HEADER:: NOTATION *******************************************\n";
  const float *K = param.ctfParam.data();

  std::ofstream ang;
  ang.precision(4);
  ang.setf(std::ios::fixed);
  if (writeAng)
  {
    ang.open("ANG_PROB");
    ang << bar;
    if (!param.doquater)
      ang << " RefMap:  MapNumber ; alpha[rad] - beta[rad] - gamma[rad] - logP - cal log Probability + Constant: "
             "Numerical Const.+ log (volume) + prior ang\n";
    else
      ang << " RefMap:  MapNumber ; q1 - q2 -q3 - logP- cal log Probability + Constant: Numerical Const. + log "
             "(volume) + prior ang\n";
    ang << bar;
  }

  std::ofstream out;
  out.precision(4);
  out.setf(std::ios::fixed);
  out.open(file.c_str());
  out << bar;
  out << "Notation= RefMap:  MapNumber ; LogProb natural logarithm of posterior Probability ; Constant: Numerical "
         "Const. for adding Probabilities \n";
  out << "Notation= RefMap:  MapNumber ; Maximizing Param: MaxLogProb - ";
  if (!param.doquater)
    out << "alpha[rad] - beta[rad] - gamma[rad] - ";
  else
    out << (param.usepsf ? "q1 - q2 - q3 - q4 -" : "q1 - q2 - q3 - q4 - ");
  if (param.usepsf)
    out << (param.doquater ? "PSF amp - PSF phase - PSF envelope" : "PSF amp - PSF phase - PSF envelope");
  else
    out << "CTF amp - CTF defocus - CTF B-Env";
  out << " - center x - center y - normalization - offsett \n";
  if (param.writeCTF)
    out << " RefMap:  MapNumber ; CTFMaxParm: defocus - b-Env (B ref. Penzeck 2010)\n";
  if (param.yespriorAngles)
    out << "**** Remark: Using Prior Proability in Angles ****\n";
  out << bar << "\n";

  for (int i = 0; i < nMaps; i++)
  {
    const bioem_hip_prob_map &pm = pmap[i];
    if (pm.Total > 1.e-38)
    {
      const double lp = log(pm.Total) + pm.Constoadd + 0.5 * log(M_PI) +
                        (1 - pd.Ntotpi * 0.5) * (log(2 * M_PI) + 1) + log(voluPerMap ? voluPerMap[i] : pd.volu);
      out << "RefMap: " << i << " LogProb:  " << lp << " Constant: " << pm.Constoadd << "\n";
      out << "RefMap: " << i << " Maximizing Param: " << lp << " ";
    }
    else
    {
      out << "Warning - RefMap: " << i << "Numerical Integrated Probability without constant = 0.0;\n";
      out << "Warning - RefMap: " << i << "Check that constant is finite: " << pm.Constoadd << "\n";
      out << "Warning - RefMap: i) check model, ii) check refmap , iii) check GPU on/off command inconsitency\n";
    }
    const float *A = angles + 4 * (angleOffsets ? (size_t) angleOffsets[i] : anglesPerMap * (size_t) i); // this map's list
    const float *a = A + 4 * (size_t) pm.max_prob_orient;
    const float *k = K + 3 * (size_t) pm.max_prob_conv;
    out << a[0] << " [] " << a[1] << " [] " << a[2] << " [] ";
    if (param.doquater)
      out << a[3] << " [] ";
    out << k[0] << " [] ";
    if (!param.usepsf)
      out << k[1] / 2.f / M_PI / param.elecwavel * 0.0001 << " [micro-m] " << k[2] << " [A²] ";
    else
      out << k[1] << " [1/A²] " << k[2] << " [1/A²] ";
    out << pm.max_prob_cent_x << " [pix] " << pm.max_prob_cent_y << " [pix] " << pm.max_prob_norm << " [] "
        << pm.max_prob_mu << " [] \n";
    if (param.writeCTF && param.usepsf)
    {
      const float denomi = k[1] * k[1] + k[2] * k[2];
      out << "RefMap: " << i << " CTFMaxParam: " << 2 * M_PI * k[1] / denomi / param.elecwavel * 0.0001
          << " [micro-m] " << 4 * M_PI * M_PI * k[2] / denomi << " [A²] \n";
    }
    if (writeAng)
    {
      // the K best orientations (selected by the reference's min-heap rule, bioem.cpp:1251-1286 -- on the device for
      // orientation-block shards, see Driver::run), best first
      const int Kbest = pd.writeAngles;
      for (int r = 0; r < Kbest; r++)
      {
        const bioem_hip_angle_candidate &c = cand[(size_t) i * Kbest + r];
        if (c.orient < 0)
          break;
        const int io = c.orient;
        double logp = c.logp;
        if (param.yespriorAngles)
          logp += param.angprior[io];
        const float *q4 = A + 4 * (size_t) io;
        ang << " " << i << " " << q4[0] << " " << q4[1] << " " << q4[2] << " ";
        if (param.doquater)
          ang << q4[3] << " ";
        ang << logp << " Separated: " << log(c.forAngles) << " " << c.ConstAngle << " " << numconst;
        if (param.yespriorAngles)
          ang << " " << param.angprior[io];
        ang << "\n";
      }
    }
  }
  if (writeAng)
    ang.close();
  out.close();
}

} // namespace bioem_host
