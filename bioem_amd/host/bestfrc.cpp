// bestfrc.cpp -- the --BestFRC text file: per particle the Fourier ring correlation of the particle against the calculated
// image of its best match, with the power of both and of their difference per ring, from the three sums per (particle,
// ring) the device delivers (bioem_hip_best_match_rings).  No reference counterpart.  Nothing here needs a device.
#include <cmath>
#include <cstdio>

#include "bioem_host.h"

namespace bioem_host
{

// the ring of coefficient (k1, k2) of the [N][N/2+1] half spectrum: the radius rounded to nearest, decided in integers
int frc_ring(int N, int k1, int k2)
{
  const long long a = k1 <= N / 2 ? k1 : k1 - N;
  const long long r2 = a * a + (long long) k2 * k2;
  long long s = (long long) std::sqrt((double) r2);
  while (s * s > r2)
    s--;
  while ((s + 1) * (s + 1) <= r2)
    s++;
  return (int) (r2 > s * s + s ? s + 1 : s);
}

// per ring the number of coefficients of the FULL spectrum: weight 1 in column 0 and (N even) column N/2, else 2
std::vector<double> frc_ring_weights(int N)
{
  std::vector<double> w;
  if (N < 1)
    return w;
  w.assign((size_t) frc_ring(N, N / 2, N / 2) + 1, 0.);
  for (int k1 = 0; k1 < N; k1++)
    for (int k2 = 0; k2 <= N / 2; k2++)
      w[(size_t) frc_ring(N, k1, k2)] += (k2 == 0 || 2 * k2 == N) ? 1. : 2.;
  return w;
}

namespace
{
double frc_quotient(double cross, double pp, double pm)
{
  const double d = pp * pm;
  return d > 0. ? cross / std::sqrt(d) : 0.;
}
} // namespace

std::string write_best_frc(const char *file, const bioem_hip_ring_sums *sums, int nMaps, int N, float pixelSize)
{
  const std::vector<double> w = frc_ring_weights(N);
  const int nRings = (int) w.size();
  if (nRings < 1 || nMaps < 1 || !sums)
    return "no ring sums to write";
  FILE *f = fopen(file, "w");
  if (!f)
    return std::string("Opening ") + file;
  const char *bar = "************************* HEADER:: NOTATION *******************************************";
  fprintf(f, "%s\n", bar);
  fprintf(f, " RING: particle ring resolution[A] weight FRC powParticle powModel powResidual   SUMMARY: particle CCC "
             "residualRMS resolution[A](FRC<0.5) resolution[A](FRC<0.143)   NumberPixels %d PixelSize %.9g\n",
          N, (double) pixelSize);
  fprintf(f, "%s\n", bar);
  const double NN = (double) N * (double) N, size = (double) N * (double) pixelSize;
  for (int p = 0; p < nMaps; p++)
  {
    const bioem_hip_ring_sums *t = sums + (size_t) p * nRings;
    double c = 0., pp = 0., pm = 0., resid = 0., r05 = -1., r0143 = -1.;
    for (int s = 0; s < nRings; s++)
    {
      const double frc = frc_quotient(t[s].cross, t[s].powParticle, t[s].powModel);
      const double res = s ? size / s : 0., rs = t[s].powParticle + t[s].powModel - 2. * t[s].cross;
      fprintf(f, "RING %d %d %.15e %.15e %.15e %.15e %.15e %.15e\n", p, s, res, w[(size_t) s], frc, t[s].powParticle,
              t[s].powModel, rs);
      resid += rs;
      if (s)
      {
        c += t[s].cross;
        pp += t[s].powParticle;
        pm += t[s].powModel;
        if (r05 < 0. && frc < 0.5)
          r05 = res;
        if (r0143 < 0. && frc < 0.143)
          r0143 = res;
      }
    }
    fprintf(f, "SUMMARY %d %.15e %.15e %.15e %.15e\n", p, frc_quotient(c, pp, pm), std::sqrt(std::fmax(resid, 0.) / (NN * NN)),
            r05, r0143);
  }
  const bool bad = ferror(f) != 0;
  return (fclose(f) != 0 || bad) ? std::string("Writing ") + file : std::string();
}

} // namespace bioem_host
