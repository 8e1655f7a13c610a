// reconstruct.cpp -- the host side of --Reconstruct: the Fourier shell correlation of the two half-set reconstructions the
// device delivers (bioem_hip_reconstruct), the text file of the shells, the lines --ReconstructSoft adds to it and the MRC
// volume a run reads back with --ReadModelMRC.  No reference counterpart.  Nothing here needs a device; bioem_amd/reconstruct.py states the same in numpy.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>

#include "bioem_host.h"

namespace bioem_host
{

void recon_shell_sums(const double *specA, const double *specB, int N, std::vector<double> &weight, std::vector<double> &cross,
                      std::vector<double> &powA, std::vector<double> &powB)
{
  const int H = N / 2 + 1;
  const int nShells = (int) std::floor(std::sqrt(3.) * (double) (N / 2) + 0.5) + 1;
  weight.assign((size_t) nShells, 0.);
  cross.assign((size_t) nShells, 0.);
  powA.assign((size_t) nShells, 0.);
  powB.assign((size_t) nShells, 0.);
  for (int i0 = 0; i0 < N; i0++)
    for (int i1 = 0; i1 < N; i1++)
      for (int k2 = 0; k2 < H; k2++)
      {
        const double k0 = i0 <= N / 2 ? i0 : i0 - N, k1 = i1 <= N / 2 ? i1 : i1 - N;
        const int s = (int) std::floor(std::sqrt(k0 * k0 + k1 * k1 + (double) k2 * k2) + 0.5);
        // the conjugate partner of a coefficient with 0 < k2 < N / 2 is not stored
        const double w = (k2 > 0 && 2 * k2 != N) ? 2. : 1.;
        const size_t e = 2 * (((size_t) i0 * N + i1) * H + k2);
        const double ar = specA[e], ai = specA[e + 1], br = specB[e], bi = specB[e + 1];
        weight[(size_t) s] += w;
        cross[(size_t) s] += w * (ar * br + ai * bi);
        powA[(size_t) s] += w * (ar * ar + ai * ai);
        powB[(size_t) s] += w * (br * br + bi * bi);
      }
}

namespace
{
double shell_quotient(double cross, double pa, double pb)
{
  const double d = pa * pb;
  return d > 0. ? cross / std::sqrt(d) : 0.;
}
} // namespace

std::string write_reconstruction(const char *file, const std::vector<double> &weight, const std::vector<double> &cross,
                                 const std::vector<double> &powA, const std::vector<double> &powB, int N, float pixelSize,
                                 double wiener, long long views, long long particles, double tau)
{
  const int nShells = (int) weight.size();
  if (nShells < 1 || cross.size() != weight.size() || powA.size() != weight.size() || powB.size() != weight.size())
    return "no shells to write";
  FILE *f = fopen(file, "w");
  if (!f)
    return std::string("Opening ") + file;
  const char *bar = "************************* HEADER:: NOTATION *******************************************";
  fprintf(f, "%s\n", bar);
  fprintf(f, " SHELL: shell resolution[A] weight FSC cross powHalf1 powHalf2   DATASET: views particles tau "
             "resolution[A](FSC<0.5) resolution[A](FSC<0.143)   NumberPixels %d PixelSize %.9g Wiener %.9g\n",
          N, (double) pixelSize, wiener);
  fprintf(f, "%s\n", bar);
  const double size = (double) N * (double) pixelSize;
  double r05 = -1., r0143 = -1.;
  for (int s = 0; s < nShells; s++)
  {
    const double fsc = shell_quotient(cross[(size_t) s], powA[(size_t) s], powB[(size_t) s]);
    if (s >= 1 && r05 < 0. && fsc < 0.5)
      r05 = size / s;
    if (s >= 1 && r0143 < 0. && fsc < 0.143)
      r0143 = size / s;
    fprintf(f, "SHELL %d %.15e %.15e %.15e %.15e %.15e %.15e\n", s, s ? size / s : 0., weight[(size_t) s], fsc,
            cross[(size_t) s], powA[(size_t) s], powB[(size_t) s]);
  }
  fprintf(f, "DATASET %lld %lld %.15e %.15e %.15e\n", views, particles, tau, r05, r0143);
  const bool bad = ferror(f) != 0;
  return (fclose(f) != 0 || bad) ? std::string("Writing ") + file : std::string();
}

std::string append_reconstruction_soft(const char *file, const int *requests, const double *nEff, const double *massArgmax,
                                       int nMaps, const std::vector<double> &weight, const std::vector<double> &cross,
                                       const std::vector<double> &powA, const std::vector<double> &powB, int N, float pixelSize)
{
  const int nShells = (int) weight.size();
  if (nShells < 1 || cross.size() != weight.size() || powA.size() != weight.size() || powB.size() != weight.size())
    return "no shells to write";
  FILE *f = fopen(file, "a");
  if (!f)
    return std::string("Opening ") + file;
  for (int p = 0; p < nMaps; p++)
    fprintf(f, "SOFT %d %d %.15e %.15e\n", p, requests[p], nEff[p], massArgmax[p]);
  const double size = (double) N * (double) pixelSize;
  for (int s = 0; s < nShells; s++)
    fprintf(f, "SOFTSHELL %d %.15e %.15e %.15e %.15e %.15e %.15e\n", s, s ? size / s : 0., weight[(size_t) s],
            shell_quotient(cross[(size_t) s], powA[(size_t) s], powB[(size_t) s]), cross[(size_t) s], powA[(size_t) s],
            powB[(size_t) s]);
  const bool bad = ferror(f) != 0;
  return (fclose(f) != 0 || bad) ? std::string("Writing ") + file : std::string();
}

// Model::readMRCFile places file voxel e (from 0, the first file axis slowest) at (e + 1 - N / 2) pixelSize; the volume
// has its origin at voxel o = (N + 1) / 2.  So file[e] = vol[(e + 1) mod N] on every axis: for even N a read-back point
// sits where the reconstruction has it, for odd N half a pixel beyond it (N / 2 is no whole number there).
std::string write_mrc_volume(const char *file, const float *vol, int N, float pixelSize)
{
  if (N < 1 || !vol)
    return "no volume to write";
  FILE *f = fopen(file, "wb");
  if (!f)
    return std::string("Opening ") + file;
  int hdr[256];
  memset(hdr, 0, sizeof(hdr));
  hdr[0] = hdr[1] = hdr[2] = N;
  hdr[3] = 2;
  hdr[7] = hdr[8] = hdr[9] = N;
  const float cell[6] = {(float) N * pixelSize, (float) N * pixelSize, (float) N * pixelSize, 90.f, 90.f, 90.f};
  memcpy(hdr + 10, cell, sizeof(cell));
  hdr[55] = 1; // one label
  char label[80];
  memset(label, ' ', sizeof(label));
  char text[80];
  const int n = snprintf(text, sizeof(text), "bioem_amd reconstruction: file[e] = vol[(e + 1) mod N] per axis, origin voxel %d",
                         (N + 1) / 2);
  memcpy(label, text, (size_t) std::min(n, 80));
  memcpy(hdr + 56, label, sizeof(label));
  bool ok = fwrite(hdr, 4, 256, f) == 256;
  std::vector<float> row((size_t) N);
  for (int e0 = 0; e0 < N && ok; e0++)
    for (int e1 = 0; e1 < N && ok; e1++)
    {
      const float *src = vol + (((size_t) ((e0 + 1) % N)) * N + (size_t) ((e1 + 1) % N)) * N;
      for (int e2 = 0; e2 < N; e2++)
        row[(size_t) e2] = src[(e2 + 1) % N];
      ok = fwrite(row.data(), sizeof(float), (size_t) N, f) == (size_t) N;
    }
  return (fclose(f) != 0 || !ok) ? std::string("Writing ") + file : std::string();
}

} // namespace bioem_host
