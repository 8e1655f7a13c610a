// orientocc.cpp -- the --OrientOccupancy text file and the prior file of --FitOrientPrior: per orientation the occupancy
// of the data set (bioem_hip_orientation_occupancy: sum over the particles of the orientation's posterior), what the host
// derives from it, and the orientation list with a fitted log prior in the --ReadOrientation format.  No reference
// counterpart.  Nothing here needs a device.
#include <cmath>
#include <cstdio>

#include "bioem_host.h"

namespace bioem_host
{

OccDataset occ_dataset(const bioem_hip_orient_occ *occ, int nO, long long nCounted)
{
  OccDataset d;
  d.nCounted = nCounted;
  d.nEffViews = 0.;
  d.maxFraction = 0.;
  d.argmax = -1;
  if (nCounted < 1)
    return d;
  double H = 0.;
  for (int o = 0; o < nO; o++)
  {
    const double f = occ[o].occ / (double) nCounted;
    if (f > 0.)
      H -= f * std::log(f);
    if (f > d.maxFraction) // strictly: the lowest index keeps a tie
    {
      d.maxFraction = f;
      d.argmax = o;
    }
  }
  d.nEffViews = std::exp(H);
  return d;
}

double log_prior_views(const double *logPrior, int nO)
{
  double H = 0.;
  for (int o = 0; o < nO; o++)
  {
    const double p = std::exp(logPrior[o]);
    if (p > 0.)
      H -= p * logPrior[o];
  }
  return std::exp(H);
}

std::string write_orient_occupancy(const char *file, const bioem_hip_orient_occ *occ, int nO, const float *angles4, bool doquater,
                                   long long nCounted, const OccFit *fits, int nFits)
{
  if (nO < 1 || !occ || !angles4)
    return "no occupancy to write";
  FILE *f = fopen(file, "w");
  if (!f)
    return std::string("Opening ") + file;
  const char *bar = "************************* HEADER:: NOTATION *******************************************";
  fprintf(f, "%s\n", bar);
  fprintf(f, " OCC: orientation %s count occ fraction nEffParticles hard wmax pmax | DATASET: countedParticles nEffViews "
             "maxFraction argmax | FIT: iteration logLikelihood nEffViews(prior)\n",
          doquater ? "q1 q2 q3 q4" : "alpha[rad] beta[rad] gamma[rad]");
  fprintf(f, "%s\n", bar);
  for (int o = 0; o < nO; o++)
  {
    const bioem_hip_orient_occ &r = occ[o];
    fprintf(f, "OCC %d", o);
    for (int i = 0; i < (doquater ? 4 : 3); i++)
      fprintf(f, " %.9g", (double) angles4[4 * (size_t) o + i]);
    fprintf(f, " %lld %.15e %.15e %.15e %lld %.15e %lld\n", (long long) r.count, r.occ, nCounted > 0 ? r.occ / (double) nCounted : 0.,
            r.occ2 > 0. ? r.occ * r.occ / r.occ2 : 0., (long long) r.hard, r.wmax, (long long) r.pmax);
  }
  const OccDataset d = occ_dataset(occ, nO, nCounted);
  fprintf(f, "DATASET %lld %.15e %.15e %d\n", d.nCounted, d.nEffViews, d.maxFraction, d.argmax);
  for (int t = 0; t < nFits; t++)
    fprintf(f, "FIT %d %.15e %.15e\n", t, fits[t].logLikelihood, fits[t].nEffViews);
  const bool bad = ferror(f) != 0;
  return (fclose(f) != 0 || bad) ? std::string("Writing ") + file : std::string();
}

std::string write_orient_prior(const char *file, const float *angles4, int nO, bool doquater, const double *logPrior)
{
  if (nO < 1 || !angles4 || !logPrior)
    return "no prior to write";
  FILE *f = fopen(file, "w");
  if (!f)
    return std::string("Opening ") + file;
  fprintf(f, "%12d\n", nO);
  for (int o = 0; o < nO; o++)
  {
    for (int i = 0; i < (doquater ? 4 : 3); i++)
      fprintf(f, "%12.8f", (double) angles4[4 * (size_t) o + i]);
    // twelve characters whatever the value: -d.ddddde+dd
    const double lp = std::fmin(0., std::fmax(kOrientPriorFloor, logPrior[o]));
    fprintf(f, "%12.5e\n", lp == 0. ? 0. : lp);
  }
  const bool bad = ferror(f) != 0;
  return (fclose(f) != 0 || bad) ? std::string("Writing ") + file : std::string();
}

void occ_next_prior(const bioem_hip_orient_occ *occ, int nO, long long nCounted, double *logPrior)
{
  for (int o = 0; o < nO; o++)
    logPrior[o] = occ[o].occ > 0. && nCounted > 0 ? std::fmax(kOrientPriorFloor, std::log(occ[o].occ / (double) nCounted))
                                                   : kOrientPriorFloor;
}

} // namespace bioem_host
