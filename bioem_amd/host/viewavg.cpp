// viewavg.cpp -- the --ViewAverages text file: per view (an orientation with enough particles behind it) the Fourier ring
// correlation of the aligned average of its particles against the model's projection at that orientation, from the three
// sums per (view, ring) the device delivers (bioem_hip_view_averages), and the grouping of the particles by their arg-max
// orientation.  No reference counterpart.  Nothing here needs a device.
#include <algorithm>
#include <cmath>
#include <cstdio>

#include "bioem_host.h"

namespace bioem_host
{

int view_groups_by_orientation(const bioem_hip_prob_map *pmap, int nMaps, int nOrient, int minCount, std::vector<int> &groupOf,
                               std::vector<int> &groupOrient)
{
  groupOf.assign((size_t) std::max(nMaps, 0), -1);
  groupOrient.clear();
  if (nMaps < 1 || nOrient < 1 || !pmap)
    return 0;
  std::vector<int> count((size_t) nOrient, 0), group((size_t) nOrient, -1);
  auto compared = [&](int p) { // a particle no run compared has no arg-max
    const bioem_hip_prob_map &r = pmap[p];
    return has_record(r) && r.max_prob_orient >= 0 && r.max_prob_orient < nOrient;
  };
  for (int p = 0; p < nMaps; p++)
    if (compared(p))
      count[(size_t) pmap[p].max_prob_orient]++;
  for (int o = 0; o < nOrient; o++) // views in ascending orientation
    if (count[(size_t) o] >= std::max(minCount, 1))
    {
      group[(size_t) o] = (int) groupOrient.size();
      groupOrient.push_back(o);
    }
  for (int p = 0; p < nMaps; p++)
    if (compared(p))
      groupOf[(size_t) p] = group[(size_t) pmap[p].max_prob_orient];
  return (int) groupOrient.size();
}

namespace
{
double view_quotient(double cross, double pp, double pm)
{
  const double d = pp * pm;
  return d > 0. ? cross / std::sqrt(d) : 0.;
}
} // namespace

std::string write_view_averages(const char *file, const bioem_hip_ring_sums *rings, int nViews, const int *groupOrient,
                                const int *counts, const float *angles4, bool doquater, int N, float pixelSize, int minCount,
                                double wiener)
{
  const std::vector<double> w = frc_ring_weights(N);
  const int nRings = (int) w.size();
  if (nRings < 1 || nViews < 0 || (nViews > 0 && (!rings || !groupOrient || !counts || !angles4)))
    return "no view averages to write";
  FILE *f = fopen(file, "w");
  if (!f)
    return std::string("Opening ") + file;
  const char *bar = "************************* HEADER:: NOTATION *******************************************";
  fprintf(f, "%s\n", bar);
  fprintf(f, " VIEW: view orientation %s count CCC resolution[A](FRC<0.5) resolution[A](FRC<0.143)   RING: view ring "
             "resolution[A] weight FRC cross powAverage powProjection   NumberPixels %d PixelSize %.9g MinParticles %d "
             "Wiener %.9g Views %d\n",
          doquater ? "q1 q2 q3 q4" : "alpha beta gamma", N, (double) pixelSize, minCount, wiener, nViews);
  fprintf(f, "%s\n", bar);
  const double size = (double) N * (double) pixelSize;
  for (int v = 0; v < nViews; v++)
  {
    const bioem_hip_ring_sums *t = rings + (size_t) v * nRings;
    double c = 0., pp = 0., pm = 0., r05 = -1., r0143 = -1.;
    for (int s = 1; s < nRings; s++)
    {
      const double frc = view_quotient(t[s].cross, t[s].powParticle, t[s].powModel);
      c += t[s].cross;
      pp += t[s].powParticle;
      pm += t[s].powModel;
      if (r05 < 0. && frc < 0.5)
        r05 = size / s;
      if (r0143 < 0. && frc < 0.143)
        r0143 = size / s;
    }
    const float *a = angles4 + 4 * (size_t) groupOrient[v];
    fprintf(f, "VIEW %d %d", v, groupOrient[v]);
    for (int k = 0; k < (doquater ? 4 : 3); k++)
      fprintf(f, " %.9g", (double) a[k]);
    fprintf(f, " %d %.15e %.15e %.15e\n", counts[v], view_quotient(c, pp, pm), r05, r0143);
    for (int s = 0; s < nRings; s++)
      fprintf(f, "RING %d %d %.15e %.15e %.15e %.15e %.15e %.15e\n", v, s, s ? size / s : 0., w[(size_t) s],
              view_quotient(t[s].cross, t[s].powParticle, t[s].powModel), t[s].cross, t[s].powParticle, t[s].powModel);
  }
  const bool bad = ferror(f) != 0;
  return (fclose(f) != 0 || bad) ? std::string("Writing ") + file : std::string();
}

} // namespace bioem_host
