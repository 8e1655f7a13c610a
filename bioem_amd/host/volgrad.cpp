// volgrad.cpp -- the --VolumeGradient text file: the gradient of the log posterior of the particles' best matches with
// respect to the voxels of a volume model (bioem_hip_volume_gradient), summarised per shell about the origin voxel.  No
// reference counterpart.  Nothing here needs a device; bioem_amd/volume_gradient.py states the same in numpy.
#include <cmath>
#include <cstdio>
#include <vector>

#include "bioem_host.h"

namespace bioem_host
{

std::string write_volume_gradient(const char *file, const double *gvol, const float *vol, int N, int nRequests, double sumw,
                                  int nonfinite)
{
  if (!gvol || !vol || N < 1)
    return "no gradient to write";
  FILE *f = fopen(file, "w");
  if (!f)
    return std::string("Opening ") + file;
  const char *bar = "************************* HEADER:: NOTATION *******************************************";
  fprintf(f, "%s\n", bar);
  fprintf(f, "Notation: SHELL s voxels sum power vol_dot_g  |  DATASET vol_dot_g norm requests sumw nonfinite\n");
  fprintf(f, "%s\n", bar);
  // shell s holds the voxels whose distance from the origin voxel (o, o, o) rounds to s; the sums run over the voxels in
  // storage order
  const int o = (N + 1) / 2;
  const int nShells = (int) std::floor(std::sqrt(3.) * (double) (N - o > o ? N - o : o) + 0.5) + 1;
  std::vector<double> sum((size_t) nShells, 0.), power((size_t) nShells, 0.), dot((size_t) nShells, 0.);
  std::vector<long long> count((size_t) nShells, 0);
  double total = 0., norm2 = 0.;
  for (int x0 = 0; x0 < N; x0++)
    for (int x1 = 0; x1 < N; x1++)
      for (int x2 = 0; x2 < N; x2++)
      {
        const size_t e = ((size_t) x0 * N + x1) * N + x2;
        const double r2 = (double) ((x0 - o) * (x0 - o) + (x1 - o) * (x1 - o) + (x2 - o) * (x2 - o));
        const int s = (int) std::floor(std::sqrt(r2) + 0.5);
        const double g = gvol[e], vg = (double) vol[e] * g;
        count[(size_t) s]++;
        sum[(size_t) s] += g;
        power[(size_t) s] += g * g;
        dot[(size_t) s] += vg;
        total += vg;
        norm2 += g * g;
      }
  for (int s = 0; s < nShells; s++)
    if (count[(size_t) s])
      fprintf(f, "SHELL %d %lld %.17g %.17g %.17g\n", s, count[(size_t) s], sum[(size_t) s], power[(size_t) s], dot[(size_t) s]);
  fprintf(f, "DATASET %.17g %.17g %d %.17g %d\n", total, std::sqrt(norm2), nRequests, sumw, nonfinite);
  const bool bad = ferror(f) != 0;
  return (fclose(f) != 0 || bad) ? std::string("Writing ") + file : std::string();
}

} // namespace bioem_host
