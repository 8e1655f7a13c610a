// orientstats.cpp -- the --OrientStats text file: per particle the summaries of its orientation posterior, derived from the
// raw sums the device delivers (bioem_hip_orientation_sums): log evidence, arg-max, its probability, entropy, effective
// number of orientations, mean orientation and angular spread.  No reference counterpart.  Nothing here needs a device.
#include <cmath>
#include <cstdio>

#include "bioem_host.h"

namespace bioem_host
{

// eigenvalues w (descending) and eigenvectors v[k] = the unit vector of w[k] of the symmetric 4 x 4 matrix a, by cyclic
// Jacobi rotations: every sweep annihilates the six off-diagonal pairs in a fixed order; done when they vanish against the
// diagonal (quadratic convergence: a handful of sweeps).  Only the upper triangle of a is read.
void jacobi4(const double a[4][4], double w[4], double v[4][4])
{
  double A[4][4], V[4][4];
  for (int i = 0; i < 4; i++)
    for (int j = 0; j < 4; j++)
    {
      A[i][j] = i <= j ? a[i][j] : a[j][i];
      V[i][j] = i == j ? 1. : 0.;
    }
  for (int sweep = 0; sweep < 64; sweep++)
  {
    double off = 0., diag = 0.;
    for (int i = 0; i < 4; i++)
    {
      diag += A[i][i] * A[i][i];
      for (int j = i + 1; j < 4; j++)
        off += A[i][j] * A[i][j];
    }
    if (!(off > 1e-34 * diag)) // (also ends on a zero or NaN matrix)
      break;
    for (int p = 0; p < 3; p++)
      for (int q = p + 1; q < 4; q++)
      {
        if (A[p][q] == 0.)
          continue;
        // the rotation that zeroes A[p][q] (Golub & Van Loan, Matrix Computations, 8.5.2: the smaller root t)
        const double theta = (A[q][q] - A[p][p]) / (2. * A[p][q]);
        const double t = (theta >= 0. ? 1. : -1.) / (std::fabs(theta) + std::sqrt(theta * theta + 1.));
        const double c = 1. / std::sqrt(t * t + 1.), s = t * c;
        for (int k = 0; k < 4; k++)
        { // A <- A J
          const double akp = A[k][p], akq = A[k][q];
          A[k][p] = c * akp - s * akq;
          A[k][q] = s * akp + c * akq;
        }
        for (int k = 0; k < 4; k++)
        { // A <- J^T A
          const double apk = A[p][k], aqk = A[q][k];
          A[p][k] = c * apk - s * aqk;
          A[q][k] = s * apk + c * aqk;
        }
        for (int k = 0; k < 4; k++)
        { // V <- V J: the columns of V are the eigenvectors
          const double vkp = V[k][p], vkq = V[k][q];
          V[k][p] = c * vkp - s * vkq;
          V[k][q] = s * vkp + c * vkq;
        }
      }
  }
  int order[4] = {0, 1, 2, 3};
  for (int i = 0; i < 4; i++) // descending, the earlier column first among equals
    for (int j = i + 1; j < 4; j++)
      if (A[order[j]][order[j]] > A[order[i]][order[i]])
        std::swap(order[i], order[j]);
  for (int k = 0; k < 4; k++)
  {
    w[k] = A[order[k]][order[k]];
    for (int i = 0; i < 4; i++)
      v[k][i] = V[i][order[k]];
  }
}

OrientStats orient_derive(const bioem_hip_orient_sums &s, const float *angles4, bool doquater)
{
  OrientStats r;
  r.count = (long long) s.count;
  r.omax = (int) s.omax;
  r.hasMean = false;
  r.logZ = -INFINITY;
  r.pTop = r.entropy = r.nEff = r.spreadDeg = 0.;
  r.mean[0] = r.mean[1] = r.mean[2] = r.mean[3] = 0.;
  if (r.count < 1 || !(s.S0 > 0.))
    return r;
  r.logZ = s.m + std::log(s.S0);
  r.entropy = std::log(s.S0) - s.S1 / s.S0;
  r.nEff = s.S0 * s.S0 / s.S2;
  r.pTop = 1. / s.S0;
  if (!doquater || s.hasMoments == 0.)
    return r;
  double a[4][4], w[4], v[4][4];
  int k = 0;
  for (int i = 0; i < 4; i++)
    for (int j = i; j < 4; j++)
      a[i][j] = a[j][i] = s.Q[k++] / s.S0;
  jacobi4(a, w, v);
  // sign: a non-negative dot product with the arg-max quaternion
  double dot = 0.;
  if (angles4 && r.omax >= 0)
    for (int i = 0; i < 4; i++)
      dot += v[0][i] * (double) angles4[4 * (size_t) r.omax + i];
  for (int i = 0; i < 4; i++)
    r.mean[i] = dot < 0. ? -v[0][i] : v[0][i];
  const double lam = std::fmin(1., std::fmax(0., w[0]));
  r.spreadDeg = 2. * std::acos(std::sqrt(lam)) * 180. / M_PI;
  r.hasMean = true;
  return r;
}

std::string write_orient_stats(const char *file, const bioem_hip_orient_sums *sums, int nMaps, const float *angles4,
                               const long long *angleOffsets, bool doquater, double numconst)
{
  if (nMaps < 1 || !sums || !angles4)
    return "no orientation sums to write";
  FILE *f = fopen(file, "w");
  if (!f)
    return std::string("Opening ") + file;
  const char *bar = "************************* HEADER:: NOTATION *******************************************";
  fprintf(f, "%s\n", bar);
  fprintf(f, " ORIENT: particle count logZ(+ Numerical Const. + log (volume)) argmax %s pTop entropy nEff "
             "meanq1 meanq2 meanq3 meanq4 spread[deg]   NumericalConst %.15e\n",
          doquater ? "q1 q2 q3 q4" : "alpha[rad] beta[rad] gamma[rad]", numconst);
  fprintf(f, "%s\n", bar);
  for (int p = 0; p < nMaps; p++)
  {
    const float *A = angles4 + 4 * (size_t) (angleOffsets ? angleOffsets[p] : 0); // this particle's list
    const OrientStats r = orient_derive(sums[p], A, doquater);
    fprintf(f, "ORIENT %d %lld %.15e %d", p, r.count, r.count > 0 ? r.logZ + numconst : r.logZ, r.omax);
    const float zero[4] = {0.f, 0.f, 0.f, 0.f};
    const float *q = r.omax >= 0 ? A + 4 * (size_t) r.omax : zero;
    for (int i = 0; i < (doquater ? 4 : 3); i++)
      fprintf(f, " %.9g", (double) q[i]);
    fprintf(f, " %.15e %.15e %.15e", r.pTop, r.entropy, r.nEff);
    if (r.hasMean)
      fprintf(f, " %.15e %.15e %.15e %.15e %.15e\n", r.mean[0], r.mean[1], r.mean[2], r.mean[3], r.spreadDeg);
    else
      fprintf(f, " - -\n");
  }
  const bool bad = ferror(f) != 0;
  return (fclose(f) != 0 || bad) ? std::string("Writing ") + file : std::string();
}

} // namespace bioem_host
