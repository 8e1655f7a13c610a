// ctfscan.cpp -- the --CTFScan text file: per particle the posterior of its best record (orientation, shift) over CTF sets
// between the points of the parameter file's grid, from the log posteriors per candidate the device delivers
// (bioem_hip_ctf_scan), with the statistics that tell whether the grid is fine and wide enough.  No reference
// counterpart.  Nothing here needs a device.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <vector>

#include "bioem_host.h"

namespace bioem_host
{

bool ctf_scan_factor_valid(int k) { return k == 1 || k == 2 || k == 4 || k == 8 || k == 16; }

int ctf_scan_refine(const float start[3], const float step[3], const int n[3], int k, int counts[3], float *triples)
{
  for (int a = 0; a < 3; a++)
    counts[a] = n[a] > 1 ? n[a] * k : 1;
  const long long G = (long long) counts[0] * counts[1] * counts[2];
  if (!triples || G > kCtfScanMaxCandidates)
    return (int) std::min<long long>(G, 0x7fffffff);
  // an axis value is (float) i * (g / (float) k) + start: with k a power of two every k-th one is the grid's (float) m * g +
  // start bit for bit; a one-point axis keeps its point
  float fine[3];
  for (int a = 0; a < 3; a++)
    fine[a] = n[a] > 1 ? step[a] / (float) k : 0.f;
  size_t g = 0;
  for (int ia = 0; ia < counts[0]; ia++)
    for (int ip = 0; ip < counts[1]; ip++)
      for (int ie = 0; ie < counts[2]; ie++, g++)
      {
        triples[3 * g + 0] = (float) ia * fine[0] + start[0];
        triples[3 * g + 1] = (float) ip * fine[1] + start[1];
        triples[3 * g + 2] = (float) ie * fine[2] + start[2];
      }
  return (int) G;
}

CtfScanStats ctf_scan_stats(const double *logp, const float *triples, const int counts[3])
{
  CtfScanStats s;
  const double nan = std::nan("");
  const int G = counts[0] * counts[1] * counts[2];
  s.logP = -INFINITY;
  s.best = -1;
  s.nEff = nan;
  s.skipped = 0;
  for (int a = 0; a < 3; a++)
    s.mean[a] = s.sd[a] = s.edgeMass[a] = nan;
  for (int g = 0; g < G; g++)
    if (!std::isfinite(logp[g]))
      s.skipped++;
    else if (s.best < 0 || logp[g] > logp[s.best])
      s.best = g;
  if (s.best < 0)
    return s;
  const double m = logp[s.best];
  double tot = 0.;
  for (int g = 0; g < G; g++)
    if (std::isfinite(logp[g]))
      tot += std::exp(logp[g] - m);
  s.logP = m + std::log(tot);
  // the value of axis a at its index i: that of any candidate with that index
  const int stride[3] = {counts[1] * counts[2], counts[2], 1};
  double w2 = 0.;
  std::vector<double> marg[3];
  for (int a = 0; a < 3; a++)
    marg[a].assign((size_t) counts[a], 0.);
  for (int g = 0; g < G; g++)
  {
    if (!std::isfinite(logp[g]))
      continue;
    const double w = std::exp(logp[g] - m) / tot;
    w2 += w * w;
    for (int a = 0; a < 3; a++)
      marg[a][(size_t) ((g / stride[a]) % counts[a])] += w;
  }
  s.nEff = 1. / w2;
  for (int a = 0; a < 3; a++)
  {
    double mean = 0., var = 0.;
    for (int i = 0; i < counts[a]; i++)
      mean += marg[a][(size_t) i] * (double) triples[3 * (size_t) (i * stride[a]) + a];
    for (int i = 0; i < counts[a]; i++)
    {
      const double d = (double) triples[3 * (size_t) (i * stride[a]) + a] - mean;
      var += marg[a][(size_t) i] * d * d;
    }
    s.mean[a] = mean;
    s.sd[a] = std::sqrt(std::fmax(var, 0.));
    s.edgeMass[a] = counts[a] > 1 ? marg[a][0] + marg[a][(size_t) counts[a] - 1] : marg[a][0];
  }
  return s;
}

std::string write_ctf_scan(const char *file, const double *logp, const float *triples, const int counts[3], int nMaps,
                           const int *orient, const int *shiftX, const int *shiftY, bool usepsf, float elecwavel,
                           const double *numconst)
{
  if (!logp || !triples || !counts || nMaps < 1 || !orient || !shiftX || !shiftY || !numconst || counts[0] < 1 ||
      counts[1] < 1 || counts[2] < 1)
    return "no scan tables to write";
  FILE *f = fopen(file, "w");
  if (!f)
    return std::string("Opening ") + file;
  const size_t G = (size_t) counts[0] * counts[1] * counts[2];
  const char *bar = "************************* HEADER:: NOTATION *******************************************";
  fprintf(f, "%s\n", bar);
  fprintf(f, " SCAN: particle %s orientation shiftX shiftY bestCandidate logP(cal log Probability + Constant) then per axis "
             "(amp, phase, envelope): values mean sd edgeMass; skippedCandidates candidates nEff   CAND: particle candidate "
             "%s logP weight\n",
          usepsf ? "PSFamp PSFphase PSFenvelope" : "CTFamp CTFdefocus[micro-m] CTFB-Env",
          usepsf ? "PSFamp PSFphase PSFenvelope" : "CTFamp CTFdefocus[micro-m] CTFB-Env");
  fprintf(f, "%s\n", bar);
  // the phase column and its statistics in the unit --ProbCTF prints
  const double unit[3] = {1., usepsf ? 1. : 1. / 2.f / M_PI / elecwavel * 0.0001, 1.};
  auto pha = [&](float v) { return usepsf ? (double) v : v / 2.f / M_PI / elecwavel * 0.0001; };
  for (int p = 0; p < nMaps; p++)
  {
    const double nan = std::nan("");
    if (orient[p] < 0)
    { // a particle no run compared: no table
      fprintf(f, "SCAN %d %.15e %.15e %.15e -1 0 0 -1 %.15e", p, 0., 0., 0., -INFINITY);
      for (int a = 0; a < 3; a++)
        fprintf(f, " 0 %.15e %.15e %.15e", nan, nan, nan);
      fprintf(f, " 0 0 %.15e\n", nan);
      continue;
    }
    const double *t = logp + G * (size_t) p;
    const CtfScanStats s = ctf_scan_stats(t, triples, counts);
    const float zero[3] = {0.f, 0.f, 0.f};
    const float *k = s.best >= 0 ? triples + 3 * (size_t) s.best : zero;
    fprintf(f, "SCAN %d %.15e %.15e %.15e %d %d %d %d %.15e", p, (double) k[0], pha(k[1]), (double) k[2], orient[p], shiftX[p],
            shiftY[p], s.best, s.logP + numconst[p]);
    for (int a = 0; a < 3; a++)
      fprintf(f, " %d %.15e %.15e %.15e", counts[a], s.mean[a] * unit[a], s.sd[a] * unit[a], s.edgeMass[a]);
    fprintf(f, " %d %d %.15e\n", s.skipped, (int) G, s.nEff);
    for (size_t g = 0; g < G; g++)
    {
      const double v = t[g];
      const double w = std::isfinite(v) && std::isfinite(s.logP) ? std::exp(v - s.logP) : 0.;
      fprintf(f, "CAND %d %d %.15e %.15e %.15e %.15e %.15e\n", p, (int) g, (double) triples[3 * g], pha(triples[3 * g + 1]),
              (double) triples[3 * g + 2], v + numconst[p], w);
    }
  }
  const bool bad = ferror(f) != 0;
  return (fclose(f) != 0 || bad) ? std::string("Writing ") + file : std::string();
}

} // namespace bioem_host
