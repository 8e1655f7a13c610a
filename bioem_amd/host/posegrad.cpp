// posegrad.cpp -- the --PoseGradient text file: the gradient of the log posterior of the particles' best matches with respect
// to a small rotation of the orientation and to the model shifts, for a volume model (bioem_hip_pose_gradient).  No
// reference counterpart.  Nothing here needs a device; bioem_amd/pose_gradient.py states the same in numpy.
#include <cmath>
#include <cstdio>

#include "bioem_host.h"

namespace bioem_host
{

// g_w = (-J[1].R[2], J[0].R[2], J[1].R[0] - J[0].R[1]) of a row {J[6], T[2], dot, R[9]}, every dot product as (x0 y0 + x1 y1)
// + x2 y2: the chain rule through R' = (I + G(w)) R
void pose_rotation_gradient(const double *row, double *g)
{
  const double *J0 = row, *J1 = row + 3, *R0 = row + 9, *R1 = row + 12, *R2 = row + 15;
  auto dot3 = [](const double *x, const double *y) { return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]; };
  g[0] = -dot3(J1, R2);
  g[1] = dot3(J0, R2);
  g[2] = dot3(J1, R0) - dot3(J0, R1);
}

std::string write_pose_gradient(const char *file, const double *rows, const bioem_hip_grad_request *req, const float *angles4,
                                int n)
{
  if (n > 0 && (!rows || !req || !angles4))
    return "no pose gradient to write";
  FILE *f = fopen(file, "w");
  if (!f)
    return std::string("Opening ") + file;
  const char *bar = "************************* HEADER:: NOTATION *******************************************";
  fprintf(f, "%s\n", bar);
  fprintf(f, "Notation: POSE particle orient q0 q1 q2 q3 conv shiftX shiftY gw0 gw1 gw2 gdeg T0 T1 dot  |  "
             "DATASET particles rms_gdeg rms_T\n");
  fprintf(f, "%s\n", bar);
  double sumG = 0., sumT = 0.;
  for (int i = 0; i < n; i++)
  {
    const double *row = rows + 18 * (size_t) i;
    const float *q = angles4 + 4 * (size_t) i;
    double g[3];
    pose_rotation_gradient(row, g);
    const double gdeg = std::sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]) * (M_PI / 180.0);
    sumG += gdeg * gdeg;
    sumT += row[6] * row[6] + row[7] * row[7];
    fprintf(f, "POSE %d %d %.17g %.17g %.17g %.17g %d %d %d %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", req[i].particle,
            req[i].orient, (double) q[0], (double) q[1], (double) q[2], (double) q[3], req[i].conv, req[i].shiftX, req[i].shiftY,
            g[0], g[1], g[2], gdeg, row[6], row[7], row[8]);
  }
  const double den = (double) (n > 0 ? n : 1);
  fprintf(f, "DATASET %d %.17g %.17g\n", n, std::sqrt(sumG / den), std::sqrt(sumT / den));
  const bool bad = ferror(f) != 0;
  return (fclose(f) != 0 || bad) ? std::string("Writing ") + file : std::string();
}

} // namespace bioem_host
