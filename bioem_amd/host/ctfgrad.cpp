// ctfgrad.cpp -- the --CTFGradient text file: gradient and curvature of the log posterior of the particles' best matches with
// respect to the CTF amplitude, defocus and B-envelope (bioem_hip_ctf_gradient), the Newton defocus and its error bar.  No
// reference counterpart.  Nothing here needs a device; bioem_amd/ctf_gradient.py states the same in numpy.
#include <cmath>
#include <cstdio>

#include "bioem_host.h"

namespace bioem_host
{

std::string write_ctf_gradient(const char *file, const double *rows, const bioem_hip_grad_request *req, int n, float elecwavel)
{
  if (n > 0 && (!rows || !req))
    return "no CTF gradient to write";
  FILE *f = fopen(file, "w");
  if (!f)
    return std::string("Opening ") + file;
  const char *bar = "************************* HEADER:: NOTATION *******************************************";
  fprintf(f, "%s\n", bar);
  fprintf(f, "Notation: CTFGRAD particle orient conv shiftX shiftY CTFamp CTFdefocus[micro-m] CTFB-Env g_amp g_defocus g_env "
             "H_aa H_ad H_ae H_dd H_de H_ee newton_defocus sigma_defocus  |  DATASET particles defined rms_g_defocus\n");
  fprintf(f, "%s\n", bar);
  // d pha / d defocus[micro-m], the host's conversion of the defocus grid; per axis d theta / d printed
  const double c = M_PI * 2.0 * 10000 * (double) elecwavel;
  const double unit[3] = {1., c, 1.};
  const int pairA[6] = {0, 0, 0, 1, 1, 2}, pairB[6] = {0, 1, 2, 1, 2, 2};
  double sumG = 0.;
  int defined = 0;
  for (int i = 0; i < n; i++)
  {
    const double *row = rows + 38 * (size_t) i, *g = row + 23, *H = row + 29;
    fprintf(f, "CTFGRAD %d %d %d %d %d", req[i].particle, req[i].orient, req[i].conv, req[i].shiftX, req[i].shiftY);
    double ctf[3], gp[3], Hp[6];
    for (int a = 0; a < 3; a++)
    {
      ctf[a] = row[a] / unit[a];
      gp[a] = g[a] * unit[a];
    }
    for (int p = 0; p < 6; p++)
      Hp[p] = H[p] * (unit[pairA[p]] * unit[pairB[p]]);
    double newton = std::nan(""), sigma = std::nan("");
    if (std::isfinite(gp[1]) && std::isfinite(Hp[3]) && Hp[3] < 0.)
    {
      newton = ctf[1] - gp[1] / Hp[3];
      sigma = std::sqrt(-1.0 / Hp[3]);
      defined++;
    }
    sumG += gp[1] * gp[1];
    for (int a = 0; a < 3; a++)
      fprintf(f, " %.17g", ctf[a]);
    for (int a = 0; a < 3; a++)
      fprintf(f, " %.17g", gp[a]);
    for (int p = 0; p < 6; p++)
      fprintf(f, " %.17g", Hp[p]);
    fprintf(f, " %.17g %.17g\n", newton, sigma);
  }
  fprintf(f, "DATASET %d %d %.17g\n", n, defined, std::sqrt(sumG / (double) (n > 0 ? n : 1)));
  const bool bad = ferror(f) != 0;
  return (fclose(f) != 0 || bad) ? std::string("Writing ") + file : std::string();
}

} // namespace bioem_host
