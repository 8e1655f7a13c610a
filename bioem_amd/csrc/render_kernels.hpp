// render_kernels.hpp -- the calculated image of a best-match record (bioem_hip_render_best_maps): what
// bioem::createConvolutedProjectionMap_noFFT writes for one hand-copied record (bioem.cpp:1925-2085), for a batch of
// records on the device.  The c2r of proj * conj(CTF) as two exact-DFT passes with double accumulation, the inverse
// counterparts of k_dft_rows / k_dft_cols (prep_kernels.hpp): the same split N = A * B, the same table
// twD[k] = exp(+2 pi i k / N) with the opposite sign of the exponent, any N (A = 1 for a prime).  The comparison kernels
// never materialise this transform (they prune it to the displacement window); nothing of a run goes through here.
#ifndef BIOEM_RENDER_KERNELS_HPP
#define BIOEM_RENDER_KERNELS_HPP

namespace
{

// one image of a batch: where its orientation lies in the source list, its CTF, and the epilogue
struct RenderRecord
{
  int src;  // index in the list the batch reads (shared list: max_prob_orient; own lists: offsets[p] + max_prob_orient)
  int conv; // max_prob_conv
  int X, Y; // max_prob_cent_x / y
  float norm, mu;
};

// the batch's orientations as one contiguous list for project_batch
__global__ void k_render_gather(const float4 *__restrict__ list, const RenderRecord *__restrict__ rec, int n,
                                float4 *__restrict__ out)
{
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < n)
    out[b] = list[rec[b].src];
}

// column k of image b: Z = P * conj(CTF) in float (bioem.cpp:1952-1955), widened, N-point inverse along the first axis.
// grid (H, nImg); dynamic LDS 2 N double2 (the footprint of k_dft_cols<false>); colspec = [b][i][k] double2
__global__ void k_render_cols(const float2 *__restrict__ spec, const float2 *__restrict__ ctf,
                              const RenderRecord *__restrict__ rec, int N, int H, int A, int B,
                              const double2 *__restrict__ tw, double2 *__restrict__ colspec)
{
  extern __shared__ double srow[];
  double2 *col = reinterpret_cast<double2 *>(srow);
  double2 *Y = col + N;
  const int k = blockIdx.x, b = blockIdx.y;
  const float2 *P = spec + (size_t) b * N * H;
  const float2 *C = ctf + (size_t) rec[b].conv * N * H;
  for (int i = threadIdx.x; i < N; i += blockDim.x)
  {
    const float2 p = P[(size_t) i * H + k], c = C[(size_t) i * H + k];
    const float re = p.x * c.x + p.y * c.y;
    const float im = p.y * c.x - p.x * c.y;
    col[i] = make_double2((double) re, (double) im);
  }
  __syncthreads();
  for (int e = threadIdx.x; e < N; e += blockDim.x)
  {
    const int j1 = e / B, kb = e - j1 * B;
    double ar = 0., ai = 0.;
    int idx = 0;
    const int step = (A * kb) % N;
    for (int j2 = 0; j2 < B; j2++)
    {
      const double2 w = tw[idx];
      const double2 x = col[A * j2 + j1];
      ar = fma(x.x, w.x, ar);
      ar = fma(-x.y, w.y, ar); // inverse: e^{+i}
      ai = fma(x.y, w.x, ai);
      ai = fma(x.x, w.y, ai);
      idx += step;
      if (idx >= N)
        idx -= N;
    }
    Y[e] = make_double2(ar, ai);
  }
  __syncthreads();
  for (int u = threadIdx.x; u < N; u += blockDim.x)
  {
    const int kb = u % B;
    double ar = 0., ai = 0.;
    int idx = 0;
    for (int j1 = 0; j1 < A; j1++)
    {
      const double2 w = tw[idx];
      const double2 y = Y[j1 * B + kb];
      ar = fma(y.x, w.x, ar);
      ar = fma(-y.y, w.y, ar);
      ai = fma(y.y, w.x, ai);
      ai = fma(y.x, w.y, ai);
      idx += u;
      if (idx >= N)
        idx -= N;
    }
    colspec[((size_t) b * N + u) * H + k] = make_double2(ar, ai);
  }
}

// row i of image b: the H stored entries extended to N by Hermitian symmetry (the imaginary parts of entry 0 and, N even,
// of entry N / 2 are dropped: the c2r convention tests/golden/c2r_nonhermitian.npz pins), N-point inverse, real part;
// rounded to float, then / N^2 * norm + mu in float in that order (bioem.cpp:2051-2053), stored at
// ((i + X) mod N, (j + Y) mod N).  grid (N, nImg); dynamic LDS 2 N double2
__global__ void k_render_rows(const double2 *__restrict__ colspec, const RenderRecord *__restrict__ rec, int N, int H,
                              int A, int B, const double2 *__restrict__ tw, float *__restrict__ out)
{
  extern __shared__ double srow[];
  double2 *row = reinterpret_cast<double2 *>(srow);
  double2 *Y = row + N;
  const int i = blockIdx.x, b = blockIdx.y;
  const double2 *src = colspec + ((size_t) b * N + i) * H;
  for (int k = threadIdx.x; k < H; k += blockDim.x)
  {
    double2 v = src[k];
    if (k == 0 || 2 * k == N)
      v.y = 0.;
    row[k] = v;
    if (k > 0 && 2 * k != N)
      row[N - k] = make_double2(v.x, -v.y);
  }
  __syncthreads();
  for (int e = threadIdx.x; e < N; e += blockDim.x)
  {
    const int j1 = e / B, kb = e - j1 * B;
    double ar = 0., ai = 0.;
    int idx = 0;
    const int step = (A * kb) % N;
    for (int j2 = 0; j2 < B; j2++)
    {
      const double2 w = tw[idx];
      const double2 x = row[A * j2 + j1];
      ar = fma(x.x, w.x, ar);
      ar = fma(-x.y, w.y, ar);
      ai = fma(x.y, w.x, ai);
      ai = fma(x.x, w.y, ai);
      idx += step;
      if (idx >= N)
        idx -= N;
    }
    Y[e] = make_double2(ar, ai);
  }
  __syncthreads();
  const RenderRecord r = rec[b];
  const float norm2 = (float) (N * N);
  int io = i + r.X; // |X|, |Y| < N (checked by the entry)
  io = io < 0 ? io + N : io >= N ? io - N : io;
  float *dst = out + ((size_t) b * N + io) * N;
  for (int j = threadIdx.x; j < N; j += blockDim.x)
  {
    const int kb = j % B;
    double ar = 0.;
    int idx = 0;
    for (int j1 = 0; j1 < A; j1++)
    {
      const double2 w = tw[idx];
      const double2 y = Y[j1 * B + kb];
      ar = fma(y.x, w.x, ar);
      ar = fma(-y.y, w.y, ar);
      idx += j;
      if (idx >= N)
        idx -= N;
    }
    int jo = j + r.Y;
    jo = jo < 0 ? jo + N : jo >= N ? jo - N : jo;
    dst[jo] = (float) ar / norm2 * r.norm + r.mu;
  }
}

} // namespace

#endif
