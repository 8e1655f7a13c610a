// bestwindow.cpp -- the --BestWindow text file: per particle the posterior over the displacement window of its best
// (orientation, CTF) pair, from the table of log posteriors per cell the device delivers (bioem_hip_window_posterior),
// with the statistics that tell whether the window is wide enough.  No reference counterpart.  Nothing here needs a device.
#include <cmath>
#include <cstdio>
#include <vector>

#include "bioem_host.h"

namespace bioem_host
{

WindowStats window_stats(const double *logp, const int *shifts, int nd)
{
  WindowStats s;
  const double nan = std::nan("");
  s.logP = -INFINITY;
  s.peakX = s.peakY = 0;
  s.peakLogp = s.meanX = s.meanY = s.sdX = s.sdY = s.edgeMass = s.nEff = nan;
  s.skipped = 0;
  int bi = -1, bj = -1;
  for (int i = 0; i < nd; i++)
    for (int j = 0; j < nd; j++)
    {
      const double v = logp[(size_t) i * nd + j];
      if (!std::isfinite(v))
        s.skipped++;
      else if (bi < 0 || v > logp[(size_t) bi * nd + bj])
        bi = i, bj = j;
    }
  if (bi < 0)
    return s;
  const double m = logp[(size_t) bi * nd + bj];
  double tot = 0.;
  for (int e = 0; e < nd * nd; e++)
    if (std::isfinite(logp[e]))
      tot += std::exp(logp[e] - m);
  int lo = shifts[0], hi = shifts[0];
  for (int i = 1; i < nd; i++)
  {
    lo = std::min(lo, shifts[i]);
    hi = std::max(hi, shifts[i]);
  }
  double mx = 0., my = 0., edge = 0., w2 = 0.;
  for (int i = 0; i < nd; i++)
    for (int j = 0; j < nd; j++)
    {
      const double v = logp[(size_t) i * nd + j];
      if (!std::isfinite(v))
        continue;
      const double w = std::exp(v - m) / tot;
      mx += w * shifts[i];
      my += w * shifts[j];
      w2 += w * w;
      if (shifts[i] == lo || shifts[i] == hi || shifts[j] == lo || shifts[j] == hi)
        edge += w;
    }
  double vx = 0., vy = 0.;
  for (int i = 0; i < nd; i++)
    for (int j = 0; j < nd; j++)
    {
      const double v = logp[(size_t) i * nd + j];
      if (!std::isfinite(v))
        continue;
      const double w = std::exp(v - m) / tot;
      vx += w * (shifts[i] - mx) * (shifts[i] - mx);
      vy += w * (shifts[j] - my) * (shifts[j] - my);
    }
  s.logP = m + std::log(tot);
  s.peakX = shifts[bi];
  s.peakY = shifts[bj];
  s.peakLogp = m;
  s.meanX = mx;
  s.meanY = my;
  s.sdX = std::sqrt(std::fmax(vx, 0.));
  s.sdY = std::sqrt(std::fmax(vy, 0.));
  s.edgeMass = edge;
  s.nEff = 1. / w2;
  return s;
}

std::string write_best_window(const char *file, const double *logp, const int *shifts, int nd, int nMaps, const int *orient,
                              const int *conv, const float *ctfParam3, bool usepsf, float elecwavel, const double *numconst)
{
  if (nd < 1 || nMaps < 1 || !logp || !shifts || !orient || !conv || !ctfParam3 || !numconst)
    return "no window tables to write";
  FILE *f = fopen(file, "w");
  if (!f)
    return std::string("Opening ") + file;
  const char *bar = "************************* HEADER:: NOTATION *******************************************";
  fprintf(f, "%s\n", bar);
  fprintf(f, " WINDOW: particle %s orientation logP(cal log Probability + Constant) peakX peakY peakLogp meanX meanY sdX sdY "
             "edgeMass nEff skippedCells cellsPerAxis   CELL: particle X Y logp weight\n",
          usepsf ? "PSFamp PSFphase PSFenvelope" : "CTFamp CTFdefocus[micro-m] CTFB-Env");
  fprintf(f, "%s\n", bar);
  const size_t cells = (size_t) nd * nd;
  for (int p = 0; p < nMaps; p++)
  {
    if (orient[p] < 0)
    { // a particle no run compared: no table
      fprintf(f, "WINDOW %d %.15e %.15e %.15e -1 %.15e 0 0 %.15e %.15e %.15e %.15e %.15e %.15e %.15e 0 0\n", p, 0., 0., 0.,
              -INFINITY, std::nan(""), std::nan(""), std::nan(""), std::nan(""), std::nan(""), std::nan(""), std::nan(""));
      continue;
    }
    const double *t = logp + cells * (size_t) p;
    const WindowStats s = window_stats(t, shifts, nd);
    const float *k = ctfParam3 + 3 * (size_t) conv[p];
    const double pha = usepsf ? (double) k[1] : k[1] / 2.f / M_PI / elecwavel * 0.0001;
    fprintf(f, "WINDOW %d %.15e %.15e %.15e %d %.15e %d %d %.15e %.15e %.15e %.15e %.15e %.15e %.15e %d %d\n", p, (double) k[0],
            pha, (double) k[2], orient[p], s.logP + numconst[p], s.peakX, s.peakY, s.peakLogp + numconst[p], s.meanX, s.meanY,
            s.sdX, s.sdY, s.edgeMass, s.nEff, s.skipped, nd);
    for (int i = 0; i < nd; i++)
      for (int j = 0; j < nd; j++)
      {
        const double v = t[(size_t) i * nd + j];
        const double w = std::isfinite(v) && std::isfinite(s.logP) ? std::exp(v - s.logP) : 0.;
        fprintf(f, "CELL %d %d %d %.15e %.15e\n", p, shifts[i], shifts[j], v + numconst[p], w);
      }
  }
  const bool bad = ferror(f) != 0;
  return (fclose(f) != 0 || bad) ? std::string("Writing ") + file : std::string();
}

} // namespace bioem_host
