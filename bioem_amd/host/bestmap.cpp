// bestmap.cpp -- the calculated image of a best match on the host side: the BEST_* parameter file of the reference's
// --PrintBestCalMap mode (bioem_param::forprintBest, param.cpp:629-907), the BESTMAP text file it writes
// (bioem.cpp:2041-2079) and the MRC stack of --BestMaps.  Written from that specification, not transcribed.  The image
// itself comes from the device (bioem_hip_render_best_maps); nothing here needs one.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>

#include "bioem_host.h"

namespace bioem_host
{

namespace
{
std::vector<std::string> tokens_of(const std::string &line)
{
  std::vector<std::string> t;
  std::istringstream in(line);
  std::string w;
  while (std::getline(in, w, ' '))
    if (!w.empty())
      t.push_back(w);
  return t;
}
} // namespace

// Keywords, units and checks of param.cpp:629-907: one value per keyword (atof / atoi of the second token), the defocus in
// micrometres converted to the phase of the CTF kernel (x 2 pi x 10 000 x wavelength, in double, stored as float), PSF
// and CTF keywords exclude each other, every component of a quaternion within [-1, 1].  The echo lines follow the
// reference's.  Returns an empty string, or the text of the reference's error.
std::string read_best_parameters(const char *file, BestParams &b)
{
  b = BestParams();
  std::ifstream input(file);
  if (!input.good())
    return std::string("Opening best parameter file: ") + file;
  std::cout << "\n +++++++++++++++++++++++++++++++++++++++++ \n";
  std::cout << "\n     ONLY READING BEST PARAMETERS \n";
  std::cout << "\n     FOR PRINTING MAXIMIZED MAP \n";
  std::cout << " +++++++++++++++++++++++++++++++++++++++++ \n";
  bool ctfparam = false;
  std::string line, err;
  // keyword -> (what it sets, its echo); flags carry no value
  struct Real
  {
    const char *key;
    float *dst;
    const char *echo;
    bool isCtf, nonNegative;
    const char *negative;
  };
  const Real reals[] = {
      {"PIXEL_SIZE", &b.pixelSize, "Pixel Size ", false, true, "Negative pixel size"},
      {"BEST_ALPHA", &b.angle[0], "Best Alpha ", false, false, nullptr},
      {"BEST_BETA", &b.angle[1], "Best beta ", false, false, nullptr},
      {"BEST_GAMMA", &b.angle[2], "Best Gamma ", false, false, nullptr},
      {"BEST_Q1", &b.angle[0], "Best q1 ", false, false, nullptr},
      {"BEST_Q2", &b.angle[1], "Best q2 ", false, false, nullptr},
      {"BEST_Q3", &b.angle[2], "Best Q3 ", false, false, nullptr},
      {"BEST_Q4", &b.angle[3], "Best Q4 ", false, false, nullptr},
      {"BEST_PSF_ENVELOPE", &b.env, "Best Envelope PSF ", false, true, "Negative START_ENVELOPE"},
      {"BEST_PSF_PHASE", &b.phase, "Best Phase PSF ", false, false, nullptr},
      {"BEST_PSF_AMP", &b.amp, "Best Amplitude PSF ", false, true, "Negative amplitude"},
      {"BEST_CTF_B_ENV", &b.env, "Best B- Env ", true, true, "Negative start B Env."},
      {"BEST_CTF_AMP", &b.amp, "Best Amplitude ", true, true, "Negative amplitude"},
      {"BEST_NORM", &b.norm, "Best norm ", false, false, nullptr},
      {"BEST_OFFSET", &b.offset, "Best offset ", false, false, nullptr},
  };
  struct Whole
  {
    const char *key;
    int *dst;
    const char *echo;
  };
  const Whole wholes[] = {{"BEST_DX", &b.ddx, "Best dx "},
                          {"BEST_DY", &b.ddy, "Best dy "},
                          {"SHIFT_X", &b.shiftX, "Shifting initial model X by "},
                          {"SHIFT_Y", &b.shiftY, "Shifting initial model Y by "}};
  while (std::getline(input, line))
  {
    if (!line.empty() && line.back() == '\r')
      line.pop_back();
    if (line.empty() || line[0] == '#')
      continue;
    const std::vector<std::string> t = tokens_of(line);
    if (t.empty())
      continue;
    const std::string &k = t[0];
    const bool flag = k == "USE_QUATERNIONS" || k == "USE_PSF" || k == "NO_PROJECT_RADIUS" || k == "PRINT_ROTATED_MODELS";
    if (!flag && t.size() < 2)
    {
      bool known = k == "NUMBER_PIXELS" || k == "BEST_CTF_DEFOCUS" || k == "WITHNOISE";
      for (const Real &r : reals)
        known = known || k == r.key;
      for (const Whole &w : wholes)
        known = known || k == w.key;
      if (known)
        return "Missing value for keyword " + k;
      continue;
    }
    const char *val = flag ? "" : t[1].c_str();
    bool done = false;
    for (const Real &r : reals)
      if (k == r.key)
      {
        *r.dst = (float) atof(val);
        if (r.nonNegative && *r.dst < 0)
          return r.negative;
        std::cout << r.echo << *r.dst << "\n";
        ctfparam = ctfparam || r.isCtf;
        done = true;
      }
    for (const Whole &w : wholes)
      if (k == w.key)
      {
        *w.dst = atoi(val);
        std::cout << w.echo << *w.dst << "\n";
        done = true;
      }
    if (done)
      continue;
    if (k == "NUMBER_PIXELS")
    {
      b.N = atoi(val);
      if (b.N < 0)
        return "Negative number of pixels";
      std::cout << "Number of Pixels " << b.N << "\n";
    }
    else if (k == "USE_QUATERNIONS")
    {
      std::cout << "Orientations with Quaternions. \n";
      b.doquater = true;
    }
    else if (k == "USE_PSF")
    {
      b.usepsf = true;
      std::cout << "Important: Using Point Spread Function. Thus, all parameters are in Real Space. \n";
    }
    else if (k == "BEST_CTF_DEFOCUS")
    {
      b.phase = (float) (atof(val) * M_PI * 2.f * 10000 * b.elecwavel);
      std::cout << "Best Defocus " << b.phase << "\n";
      ctfparam = true;
    }
    else if (k == "WITHNOISE")
    {
      b.stnoise = (float) atof(val);
      b.withnoise = true;
      std::cout << "Including noise with standard deviation " << b.stnoise << "\n";
    }
    else if (k == "NO_PROJECT_RADIUS")
    {
      b.doaaradius = false;
      std::cout << "Not projecting corresponding radius \n";
    }
    else if (k == "PRINT_ROTATED_MODELS")
    {
      b.printrotmod = true;
      std::cout << "Printing out rotated models: accepted, no effect (the projection runs on the device)\n";
    }
  }
  if (b.doquater)
    for (int c : {3, 0, 1, 2})
      if (b.angle[c] * b.angle[c] > 1)
      {
        char buf[64];
        snprintf(buf, sizeof(buf), "Quaternion %lf", (double) b.angle[c]);
        return buf;
      }
  if (b.usepsf && ctfparam)
    return "Inconsitent input: using both PSF and CTF?";
  if (b.N < 2)
    return "Input missing: please provide NUMBER_PIXELS";
  if (!(b.pixelSize > 0))
    return "Input missing: please provide PIXEL_SIZE";
  return "";
}

// The BESTMAP text of bioem.cpp:2041-2079, default float formatting of an ofstream (6 significant digits): for every
// (k, j) "\nMAP k+ddx j+ddy v[k][j]"; where k+ddx < N and j+ddy < N also "\nMAPddx k j v[k-ddx][j-ddy]"; " \n" after
// each k.  Deviation: the reference reads v[k-ddx][j-ddy] also where that index lies outside the array; the MAPddx line is
// written only where 0 <= k-ddx < N and 0 <= j-ddy < N.  mapOnly (WITHNOISE): the MAP lines alone, as the reference.
bool write_bestmap_text(const char *file, const float *v, int N, int ddx, int ddy, bool mapOnly)
{
  std::ofstream out(file);
  if (!out.good())
    return false;
  for (int k = 0; k < N; k++)
  {
    for (int j = 0; j < N; j++)
    {
      out << "\nMAP " << k + ddx << " " << j + ddy << " " << v[(size_t) k * N + j];
      const int ks = k - ddx, js = j - ddy;
      if (!mapOnly && k + ddx < N && j + ddy < N && ks >= 0 && ks < N && js >= 0 && js < N)
        out << "\nMAPddx " << k << " " << j << " " << v[(size_t) ks * N + js];
    }
    out << " \n";
  }
  out.close();
  return out.good();
}

// MRC mode-2 stack, little-endian, 1024-byte header, no symmetry bytes: nx = ny = N, nz = nMaps.  Sections are stored
// the way the --ReadMRC reader takes them (it transposes: map[i][j] = section[j][i], map.cpp:824), so the file goes back
// in as a particle stack.  append() may be called batch by batch; close() checks the count.
bool MrcStackWriter::open(const char *file, int N_, int nMaps_)
{
  N = N_;
  nMaps = nMaps_;
  written = 0;
  f = fopen(file, "wb");
  if (!f)
    return false;
  unsigned char hdr[1024];
  memset(hdr, 0, sizeof(hdr));
  auto putI = [&](int word, int v) {
    for (int b = 0; b < 4; b++)
      hdr[4 * word + b] = (unsigned char) (((unsigned int) v >> (8 * b)) & 0xff);
  };
  auto putF = [&](int word, float v) {
    unsigned int u;
    memcpy(&u, &v, 4);
    putI(word, (int) u);
  };
  putI(0, N);
  putI(1, N);
  putI(2, nMaps);
  putI(3, 2); // mode 2: 32-bit float
  putI(7, N);
  putI(8, N);
  putI(9, nMaps);
  putF(10, (float) N);
  putF(11, (float) N);
  putF(12, (float) nMaps);
  for (int w = 13; w < 16; w++)
    putF(w, 90.f);
  putI(16, 1);
  putI(17, 2);
  putI(18, 3);
  memcpy(hdr + 208, "MAP ", 4);
  hdr[212] = 0x44; // machine stamp: little-endian
  hdr[213] = 0x44;
  return fwrite(hdr, 1, sizeof(hdr), f) == sizeof(hdr);
}

bool MrcStackWriter::append(const float *maps, int n)
{
  if (!f || written + n > nMaps)
    return false;
  const size_t NN = (size_t) N * N;
  std::vector<unsigned char> sec(4 * NN);
  for (int s = 0; s < n; s++)
  {
    const float *m = maps + (size_t) s * NN;
    for (int j = 0; j < N; j++)
      for (int i = 0; i < N; i++)
      {
        unsigned int u;
        memcpy(&u, &m[(size_t) i * N + j], 4);
        unsigned char *d = &sec[4 * ((size_t) j * N + i)];
        d[0] = (unsigned char) (u & 0xff);
        d[1] = (unsigned char) ((u >> 8) & 0xff);
        d[2] = (unsigned char) ((u >> 16) & 0xff);
        d[3] = (unsigned char) (u >> 24);
      }
    if (fwrite(sec.data(), 1, sec.size(), f) != sec.size())
      return false;
  }
  written += n;
  return true;
}

bool MrcStackWriter::close()
{
  if (!f)
    return false;
  const bool ok = fclose(f) == 0 && written == nMaps;
  f = nullptr;
  return ok;
}

MrcStackWriter::~MrcStackWriter()
{
  if (f)
    fclose(f);
}

} // namespace bioem_host
