// modelgrad.cpp -- the --ModelGradient text file: per model point the gradient of the log posterior of the particles' best
// matches with respect to its density, from the sums the device delivers (bioem_hip_model_gradient).  No reference
// counterpart.  Nothing here needs a device.
#include <cmath>
#include <cstdio>

#include "bioem_host.h"

namespace bioem_host
{

std::string write_model_gradient(const char *file, const bioem_hip_model_point *points, const bioem_hip_grad_point *acc, int nPts,
                                 int nonfinite)
{
  if (!points || !acc || nPts < 1)
    return "no gradient to write";
  FILE *f = fopen(file, "w");
  if (!f)
    return std::string("Opening ") + file;
  const char *bar = "************************* HEADER:: NOTATION *******************************************";
  fprintf(f, "%s\n", bar);
  fprintf(f, "Notation: POINT k x y z radius density sum mean z count  |  DATASET rho_dot_sum norm nonfinite\n");
  fprintf(f, "%s\n", bar);
  double dot = 0., norm2 = 0.;
  for (int k = 0; k < nPts; k++)
  {
    const bioem_hip_model_point &p = points[k];
    const bioem_hip_grad_point &a = acc[k];
    const double mean = a.sumw != 0. ? a.sum / a.sumw : 0.;
    const double z = a.sumsq > 0. ? a.sum / std::sqrt(a.sumsq) : 0.;
    fprintf(f, "POINT %d %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %lld\n", k, (double) p.pos[0], (double) p.pos[1],
            (double) p.pos[2], (double) p.radius, (double) p.density, a.sum, mean, z, a.count);
    dot += (double) p.density * a.sum;
    norm2 += a.sum * a.sum;
  }
  fprintf(f, "DATASET %.17g %.17g %d\n", dot, std::sqrt(norm2), nonfinite);
  const bool bad = ferror(f) != 0;
  return (fclose(f) != 0 || bad) ? std::string("Writing ") + file : std::string();
}

} // namespace bioem_host
