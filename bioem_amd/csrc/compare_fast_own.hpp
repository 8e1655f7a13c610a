// compare_fast_own.hpp -- k_compare_fast with a block order of its own for the own-list pass (one orientation list per
// particle, bioem_hip_compare_own_orientations): ONE launch over a batch of rows whose particles differ
// Part of libbioem_hip.so; included by kernels_fast_own.hip only (anonymous namespace).
//
// k_compare_fast_own is a COPY of k_compare_fast's body (compare_fast.hpp), not a shared function template: the copy
// leaves compare_fast.hpp untouched, so the all-to-all kernels are the parent's instruction for instruction by
// construction.  What differs is marked OWN: the block-to-work mapping and the index that addresses the
// per-row buffers.  Everything a wave computes for a (particle, row) pair is the arithmetic of k_compare_fast in the same
// order, so a row's partial equals the per-particle launch's bit for bit.
#ifndef BIOEM_COMPARE_FAST_OWN_HPP
#define BIOEM_COMPARE_FAST_OWN_HPP

namespace
{

// one entry per block: {particle, first row, end row, 0} -- at most four consecutive rows [first, end) of that
// particle's run in the batch (rows are indices into conv / params / postc / partials / tnyq of the launch)
typedef int __attribute__((ext_vector_type(4))) own_i32x4;
typedef const own_i32x4 __attribute__((address_space(4))) *const_int4_ptr;

template <int WD, int R, bool NYQ, int GS>
__global__ __launch_bounds__(256, 3) void k_compare_fast_own(const CompareArgs a, const int4 *__restrict__ blocks)
{
  static_assert(WD <= 10, "windows of at most 21 rows; 27 / 31 rows: k_compare_fastm");
  constexpr int NW = 2 * WD + 1;
  constexpr int R2 = R / 2;            // rows (k2 pairs) per k1 step
  // depth of the operand ring: must divide R2 so that a ring slot is a compile-time function of the k2 pair
  // (R = 30: a ring of 3, not 5 -- 16 registers the 21-row window of that length needs)
  constexpr int RD = (R2 % 4 == 0) ? 4 : (R2 == 15) ? 3 : (R2 % 5 == 0) ? 5 : (R2 % 3 == 0) ? 3 : (R2 % 2 == 0) ? 2 : 1;
  constexpr int NR = (WD <= 5) ? 3 : 7; // accumulators (window rows) per lane
  // T row stride in float2 (64 columns + 2 pad: row groups land on different banks)
  constexpr int TS = 66;
  // the static 21-row window runs the pass over |dy| (window_accumulate_sym): 8 accumulators per lane, and the head of
  // the LDS holds the slice of the cos | sin table for the current column block instead of the twiddles
  constexpr bool SYM = sym_window_ok(WD, R, NYQ, GS);
  constexpr int NA = SYM ? 8 : NR;
  extern __shared__ __align__(16) unsigned char smem[];
  const int N = a.N, H = a.H, N1 = a.N1;
  const size_t headBytes = fast_head_bytes(N, SYM);
  float2 *twl = reinterpret_cast<float2 *>(smem);                 // N+1 (+pad), or the table slice
  int *displ = reinterpret_cast<int *>(smem + headBytes);         // nd ints (256 B reserved)
  double2 *ltab = reinterpret_cast<double2 *>(smem + headBytes + 256); // 64 entries
  float2 *Tall = reinterpret_cast<float2 *>(smem + headBytes + 256 + 1024);
  // wave index made provably uniform (SGPR) so that per-wave base pointers use scalar addressing
  const int wave = __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6));
  const int lane = threadIdx.x & 63;
  float2 *Tl = Tall + (size_t) wave * NW * TS;

  int *dinv = displ + 32; // visiting rank of window row m (displacement m*GS), index m + mD
  const int mD = a.maxD / GS;
  // (the rows -WD..WD, all of them: what is_static below says of a 21-row window)
  const bool symw = SYM && a.nd == NW && mD == WD;
  if (!symw)
    for (int t = threadIdx.x; t <= N; t += blockDim.x)
      twl[t] = a.tw[t];
  for (int t = threadIdx.x; t < a.nd; t += blockDim.x)
  {
    const int dv = a.disp[t];
    displ[t] = dv;
    const int m = dv / GS + mD;
    if (m >= 0 && m < 32)
      dinv[m] = t;
  }
  for (int t = threadIdx.x; t < 64; t += blockDim.x)
    ltab[t] = a.ltab[t];
  __syncthreads();

  // OWN: block -> one entry of the block table.  blockIdx is uniform, the table is read through the constant address
  // space: scalar loads.  The host builds the table (own_block_table, bioem_hip.hip): every entry lies inside the launch.
  const own_i32x4 be = *((const_int4_ptr) (unsigned long long) (blocks + blockIdx.x));
  const int p = be.x;
  const int oc_raw = be.y + wave;
  const bool oc_valid = oc_raw < be.z;
  const int oc = oc_valid ? oc_raw : be.z - 1;
  const int Hp = a.Hp; // row-pair pitch in 16-byte words (H, or H + 15: comparison_pitch in bioem_hip.hip)
  const size_t M = (size_t) N * Hp;
  // buffer descriptors built from wave-uniform values only (blockIdx / readfirstlane'd wave id)
  const auto rsrcF = __builtin_amdgcn_make_buffer_rsrc(uniform_ptr(const_cast<float2 *>(a.ref + (size_t) p * M)), 0,
                                                       (int) (M * sizeof(float2)), 0x00020000);
  const auto rsrcC = __builtin_amdgcn_make_buffer_rsrc(uniform_ptr(const_cast<float2 *>(a.conv + (size_t) oc * M)), 0,
                                                       (int) (M * sizeof(float2)), 0x00020000);

  // window lanes
  const int nd = a.nd;
  const int G = 64 / nd;
  const int nr = (nd + G - 1) / G;
  const int iy = lane % nd, grp = lane / nd;
  const bool wactive = grp < G;
  const int dy = displ[iy];
  const int step = dy < 0 ? dy + N : dy;
  // static window (the +-10 px, grid 1 case): the window rows are -mD..mD and every lane group owns exactly
  // NR CONSECUTIVE rows of it in sorted order, whatever the visiting order of the algorithm (ALGO 1 visits
  // 0..maxD, -maxD..-1); dinv[] translates back to visiting ranks for the arg-max bookkeeping
  const bool is_static = (nr == NR) && (nd == G * NR) && (nd == 2 * mD + 1);
  float acc[NA];
#pragma unroll
  for (int r = 0; r < NA; r++)
    acc[r] = 0.f;
  // window_accumulate_sym: lane = 3 * row + group (lane 63 reads row 20 and is dropped later)
  const int srow = min(lane / 3, NW - 1), sgrp = lane % 3;
  const float2 *Trow = Tl + srow * TS;
  const float4 *stab = reinterpret_cast<const float4 *>(smem) + sgrp * 4;
  const float2 *symsrc = a.tw + sym_table_offset(N) + threadIdx.x;
  // T row (in float2 units) of accumulator r of this lane; idle lanes (grp >= G) read rows 0.. and are dropped
  // later.  Only the first is kept live across the column loop: the static window uses base + r*TS, the general
  // one re-reads its rows from the displacement list per block.
  auto row_of = [&](int r) -> int {
    int ix = wactive ? grp * nr + r : r;
    if (ix >= nd)
      ix = nd - 1;
    return (displ[ix] / GS + WD) * TS;
  };
  const int rowbase = is_static ? ((wactive ? grp : 0) * NR - mD + WD) * TS : row_of(0);

  const int nblk = NYQ ? (H - 1 + 63) / 64 : (H + 63) / 64; // (Nyquist split: whole blocks, or a last one of 32 columns)
  // Operand stream (software pipelined across k1 iterations AND column blocks): the (k1, k2-pair) loads of a
  // lane walk t = k1*16 + k2p with a constant stride of H float4; a 4-deep ring of (F, C) pairs keeps 8 dwordx4
  // loads (8 KiB per wave) in flight, re-issued as soon as a slot is consumed.  The ring runs on into the first
  // rows of the NEXT column block, so those loads fly during the T exchange / window phase of this block.
  // Addressing: buffer loads -- 128-bit descriptor (SGPRs), one 32-bit lane offset (VGPR), row offset in an SGPR.
  const unsigned rowbytes = (unsigned) Hp * 16u;
  // Split last block (a.split: it holds at most 32 columns, e.g. 17 of the 81 at 160^2): lane l and lane l + 32 take the
  // SAME column, the low half the k1 steps 0 .. sHalf - 1, the high half sHalf .. N1 - 1 (one past the end with an odd
  // N1: those rows lie beyond the buffer and read as zeros).  Inside the loop both halves use the low half's
  // recombination twiddles -- wave-uniform as everywhere --, w^(dx (k1 + sHalf)) = w^(dx k1) w^(dx sHalf): the high half's
  // sums are turned by w^(dx sHalf) once, after the loop, and the halves added with v_permlane32_swap.  The pass then
  // costs sHalf instead of N1 steps: 1.5 instead of 2 passes at 160^2.
  constexpr bool SPLIT_OK = !(NYQ && R == 32); // (the 32-point Nyquist kernels have no registers left for it)
  const int sHalf = (N1 + 1) >> 1;
  const int hsel = lane >> 5;
  const unsigned halfoff = (unsigned) (hsel * sHalf * R2) * rowbytes;
  auto lane_offset = [&](int b) -> unsigned { // byte offset of this lane's column (and half) in column block b
    const bool sp = SPLIT_OK && a.split && b == nblk - 1;
    const int kyb = b * 64 + (sp ? (lane & 31) : lane);
    return (unsigned) (kyb < H ? kyb : H - 1) * 16u + (sp ? halfoff : 0u);
  };
  u32x4 rf[RD], rc[RD];
  {
    const unsigned lo0 = lane_offset(0);
#pragma unroll
    for (int t = 0; t < RD; t++)
    {
      rf[t] = __builtin_amdgcn_raw_buffer_load_b128(rsrcF, lo0, (unsigned) t * rowbytes, 0);
      rc[t] = __builtin_amdgcn_raw_buffer_load_b128(rsrcC, lo0, (unsigned) t * rowbytes, 0);
    }
  }
  for (int blk = 0; blk < nblk; blk++)
  {
    const bool split = SPLIT_OK && a.split && blk == nblk - 1;
    const int n1 = split ? sHalf : N1;
    const int ttotal = R2 * n1;
    const int ky = blk * 64 + (split ? (lane & 31) : lane);
    const unsigned laneoff = lane_offset(blk);
    const unsigned laneoff_next = lane_offset(min(blk + 1, nblk - 1));
    const bool has_next = blk + 1 < nblk;
    float Tr[NW], Ti[NW];
#pragma unroll
    for (int d = 0; d < NW; d++)
    {
      Tr[d] = 0.f;
      Ti[d] = 0.f;
    }
    // table slice of this column block: 24 bytes per thread, requested now and put into the LDS with the T block
    float2 tabv[3] = {};
    if (symw)
    {
#pragma unroll
      for (int u = 0; u < 3; u++)
        tabv[u] = symsrc[blk * kSymSliceFloat2 + u * 256];
    }
    // lanes beyond the last column of the last block sit out the whole transform (EXEC masked once): their
    // loads would only burn vector-memory cycles, and their T columns stay zero
    if (ky < H)
    for (int k1 = 0; k1 < n1; k1++)
    {
      float xr[R], xi[R];
      // the 2*WD+1 recombination twiddles of this k1 are contiguous: a few wide scalar loads, issued early
      float2 wk[NW];
      const float2 *twk = a.twk + (size_t) k1 * NW;
#pragma unroll
      for (int d = 0; d < NW; d++)
        wk[d] = twk[d];
#pragma unroll
      for (int k2p = 0; k2p < R2; k2p++)
      {
        const float4 f = as_float4(rf[k2p % RD]);
        const float4 c = as_float4(rc[k2p % RD]);
        // X = conv * conj(ref)   (bioem.cpp:1452-1455)
        xr[FFT_IN(2 * k2p)] = fmaf(c.x, f.x, c.y * f.y);
        xi[FFT_IN(2 * k2p)] = fmaf(c.y, f.x, -(c.x * f.y));
        xr[FFT_IN(2 * k2p + 1)] = fmaf(c.z, f.z, c.w * f.w);
        xi[FFT_IN(2 * k2p + 1)] = fmaf(c.w, f.z, -(c.z * f.w));
        int tn = k1 * R2 + k2p + RD;
        unsigned vo = laneoff;
        // (only the last RD requests of a k1 step can leave the block: the first test folds at compile time)
        if (k2p + RD >= R2 && tn >= ttotal)
        { // last steps of this block: run on into the next block (or re-read the last row at the very end)
          tn = has_next ? tn - ttotal : ttotal - 1;
          vo = has_next ? laneoff_next : laneoff;
        }
        rf[k2p % RD] = __builtin_amdgcn_raw_buffer_load_b128(rsrcF, vo, (unsigned) tn * rowbytes, 0);
        rc[k2p % RD] = __builtin_amdgcn_raw_buffer_load_b128(rsrcC, vo, (unsigned) tn * rowbytes, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
      FFT_RUN(xr, xi);
      // recombination of the N1 sub-transforms for the displacement window only:
      //   T[dx] += w_N^(dx*k1) * y_k1[dx mod 32]
#pragma unroll
      for (int d = -WD; d <= WD; d++)
      {
        const int pos = FFT_OUT((((d * GS) % R) + R) % R);
        const float2 w = wk[d + WD];
        float tr = Tr[d + WD], ti = Ti[d + WD];
        tr = fmaf(xr[pos], w.x, tr);
        tr = fmaf(-xi[pos], w.y, tr);
        ti = fmaf(xr[pos], w.y, ti);
        ti = fmaf(xi[pos], w.x, ti);
        Tr[d + WD] = tr;
        Ti[d + WD] = ti;
      }
    }
    if (split)
    {
      const float2 *ws = a.twk + (size_t) sHalf * NW; // w^(dx sHalf), the table's row sHalf
#pragma unroll
      for (int d = 0; d < NW; d++)
      {
        const float2 w = ws[d];
        const float wx = hsel ? w.x : 1.f, wy = hsel ? w.y : 0.f;
        const float tr = fmaf(-Ti[d], wy, Tr[d] * wx), ti = fmaf(Ti[d], wx, Tr[d] * wy);
        const u32x2 sr = __builtin_amdgcn_permlane32_swap(__float_as_uint(tr), __float_as_uint(tr), false, false);
        const u32x2 si = __builtin_amdgcn_permlane32_swap(__float_as_uint(ti), __float_as_uint(ti), false, false);
        Tr[d] = __uint_as_float(sr.x) + __uint_as_float(sr.y); // low half + high half, in every lane
        Ti[d] = __uint_as_float(si.x) + __uint_as_float(si.y);
      }
    }
    // FFTW c2r convention: columns 0 and N/2 enter once (real part only after the ky pass), others twice
    float wgt = 2.f;
    if (ky == 0 || (((N & 1) == 0) && ky == N / 2))
      wgt = 1.f;
    if (ky >= H || (split && hsel))
      wgt = 0.f;
    // T block of THIS wave only, written and read between block barriers (they keep the 4 waves in lock-step)
    {
      __syncthreads(); // previous window reads are done
#pragma unroll
      for (int d = 0; d < NW; d++)
        Tl[d * TS + lane] = make_float2(Tr[d] * wgt, Ti[d] * wgt);
      if (symw)
      {
#pragma unroll
        for (int u = 0; u < 3; u++)
          twl[u * 256 + threadIdx.x] = tabv[u];
      }
      __syncthreads();
      const int idx0 = (int) (((long long) (blk * 64) * step) % N);
      const int npairs = min(32, (H - blk * 64 + 1) >> 1); // columns of this block that exist, in pairs
      if (symw)
      {
        if constexpr (SYM)
          window_accumulate_sym<TS>(Trow, stab, acc, npairs);
      }
      else if (!SYM && is_static)
      {
        const int rowoff[NR] = {rowbase};
        window_accumulate<NR, true, 32, TS>(Tl, twl, N, step, idx0, rowoff, nr, acc, npairs);
      }
      else
      {
        int rowoff[NR];
#pragma unroll
        for (int r = 0; r < NR; r++)
          rowoff[r] = row_of(r);
        window_accumulate<NR, false, 32, TS>(Tl, twl, N, step, idx0, rowoff, nr, acc, npairs);
      }
    }
  }
  if (NYQ)
  {
    const float *tq = a.tnyq + (size_t) oc * NW; // OWN: one set of Nyquist rows per row of the launch
    const float sg = (dy & 1) ? -1.f : 1.f;
    if (symw)
    { // the column's term is real: it enters A only, with the sign of (-1)^|dy|
      if constexpr (SYM)
      {
#pragma unroll
        for (int j = 0; j < 4; j++)
          acc[j] = fmaf((((sgrp * 4 + j) * GS) & 1) ? -1.f : 1.f, tq[srow], acc[j]);
      }
    }
    else
    {
#pragma unroll
      for (int r = 0; r < NR; r++)
        acc[r] = fmaf(sg, tq[is_static ? rowbase / TS + r : row_of(r) / TS], acc[r]);
    }
  }

  const double2 pc = a.postc[oc];
  const PostW pw = post_consts(a.pd.Ntotpi, N, a.params[oc], a.sumRef[p], a.sumsqRef[p], pc.x, pc.y);
  LseF L;
  L.m = -INFINITY;
  L.s = 0.;
  L.id = 0x7fffffff;
  L.val = 0.f;
  {
    // the NR displacements of this lane as one batch (posterior_batch: exact division by N^2 in three instructions,
    // the log-table reads issued together, one log-sum-exp rescale)
    constexpr int PB = NA > 8 ? 8 : NA;
#pragma unroll
    for (int r0 = 0; r0 < NA; r0 += PB)
    {
      float accv[PB];
      int idv[PB];
      bool okv[PB];
      if (symw)
      { // slot 2 q: dy = +(4 g + q) rows, A - B; slot 2 q + 1: dy = -(4 g + q) rows, A + B (dy = 0 once; 4 g + q <= WD)
        if constexpr (SYM)
        {
          const int ixv = dinv[srow];
#pragma unroll
          for (int j = 0; j < 8; j++)
          {
            const int q = j >> 1, m = sgrp * 4 + q;
            const int iyv = dinv[min(max((j & 1) ? mD - m : mD + m, 0), 31)];
            okv[j] = lane < 3 * NW && m <= WD && !((j & 1) && m == 0) && srow < a.ndx && iyv < a.ndy;
            accv[j] = (j & 1) ? acc[q] + acc[4 + q] : acc[q] - acc[4 + q];
            idv[j] = ixv * nd + iyv;
          }
        }
      }
      else
      {
#pragma unroll
        for (int j = 0; j < PB; j++)
        {
          const int r = r0 + j < NR ? r0 + j : NR - 1;
          const int ixs = grp * nr + r; // position in the lane-group order; ix = visiting rank of that displacement
          okv[j] = r0 + j < NR && r < nr && wactive && ixs < a.ndx && iy < a.ndy;
          const int ix = is_static ? dinv[min(ixs, 31)] : ixs;
          accv[j] = acc[r];
          idv[j] = ix * nd + iy;
        }
      }
      posterior_batch<PB>(L, accv, idv, okv, pw, ltab, a.algo);
    }
  }
  lsef_wave_reduce(L);
  if (lane == 0 && oc_valid)
  {
    Partial r;
    r.sumExp = L.s;
    r.best = L.m;
    r.id = L.id;
    r.value = L.val;
    r.pad = 0;
    a.partials[oc] = r; // OWN: one partial per row of the launch
  }
}

// ------------------------------------------------------------------------------------------------
// Nyquist-column rows of a launch of k_compare_fast_own: row oc of the launch against ITS particle, rowParticle[oc].
// The arithmetic is k_nyquist_rows<WD, 4>'s -- the kernel a per-particle launch runs --, so the rows equal that launch's
// bit for bit: the four waves of a block share its 64 rows, wave q sums the q-th quarter of the row pairs in order, the
// quarters are added through LDS as (q0 + q1) + (q2 + q3).  One thread per row and quarter.
//   tnyq[oc][m + WD] = Re sum_kx conv[oc][kx][N/2] * conj(ref[p][kx][N/2]) * w_N^(kx m gs),  m = -WD..WD
// ------------------------------------------------------------------------------------------------
template <int WD>
__global__ __launch_bounds__(256) void k_nyquist_rows_own(const CompareArgs a, const int *__restrict__ slotParticle,
                                                          int row0, int nCTF)
{
  constexpr int NW = 2 * WD + 1;
  __shared__ float part[2 * 64 * NW];
  const int N = a.N, N1 = a.N1;
  const int R2 = N / (2 * N1);
  const int q = __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6));
  const int t = threadIdx.x & 63;
  const int oc = blockIdx.x * 64 + t;
  const bool valid = oc < a.nOC;
  // slotParticle[s] = particle of flat slot s; row oc of the launch is row row0 + oc of the flat order, nCTF rows a slot
  const int p = valid ? slotParticle[(row0 + oc) / nCTF] : 0;
  const size_t M = (size_t) N * a.Hp;
  const float2 *F = a.ref + (size_t) p * M;
  const float2 *C = a.conv + (size_t) (valid ? oc : 0) * M;
  float acc[NW];
#pragma unroll
  for (int d = 0; d < NW; d++)
    acc[d] = 0.f;
  const int nRP = N1 * R2 / 4; // row pairs of this thread: [q nRP, (q + 1) nRP)
  constexpr int NB = 8;        // N/2 is a multiple of 64, a quarter of it of 16
  for (int rp0 = q * nRP; rp0 < (q + 1) * nRP; rp0 += NB)
  {
    float4 cb[NB], fb[NB];
#pragma unroll
    for (int u = 0; u < NB; u++)
    {
      const size_t li = ((size_t) (rp0 + u) * a.Hp + N / 2) * 2;
      cb[u] = *reinterpret_cast<const float4 *>(C + li);
      fb[u] = *reinterpret_cast<const float4 *>(F + li);
    }
#pragma unroll
    for (int u = 0; u < NB; u++)
    {
      const float4 c = cb[u], f = fb[u];
      // X = conv * conj(ref)   (bioem.cpp:1452-1455)
      const float x0r = fmaf(c.x, f.x, c.y * f.y), x0i = fmaf(c.y, f.x, -(c.x * f.y));
      const float x1r = fmaf(c.z, f.z, c.w * f.w), x1i = fmaf(c.w, f.z, -(c.z * f.w));
      const float4 *tw = reinterpret_cast<const float4 *>(a.twnyq + (size_t) (rp0 + u) * NW * 2);
#pragma unroll
      for (int d = 0; d < NW; d++)
      {
        const float4 w = tw[d]; // (w0.re, w0.im, w1.re, w1.im)
        float v = acc[d];
        v = fmaf(x0r, w.x, v);
        v = fmaf(-x0i, w.y, v);
        v = fmaf(x1r, w.z, v);
        v = fmaf(-x1i, w.w, v);
        acc[d] = v;
      }
    }
  }
  // (q0 + q1) in wave 0, (q2 + q3) in wave 2, then their sum in wave 0
  float *mine = part + ((q >> 1) * 64 + t) * NW;
  if (q & 1)
  {
#pragma unroll
    for (int d = 0; d < NW; d++)
      mine[d] = acc[d];
  }
  __syncthreads();
  if (!(q & 1))
  {
#pragma unroll
    for (int d = 0; d < NW; d++)
      acc[d] += mine[d];
  }
  __syncthreads();
  if (q == 2)
  {
#pragma unroll
    for (int d = 0; d < NW; d++)
      mine[d] = acc[d];
  }
  __syncthreads();
  if (q == 0)
  {
#pragma unroll
    for (int d = 0; d < NW; d++)
      acc[d] += part[(64 + t) * NW + d];
  }
  if (valid && q == 0)
  {
    float *o = a.tnyq + (size_t) oc * NW;
#pragma unroll
    for (int d = 0; d < NW; d++)
      o[d] = acc[d];
  }
}

} // namespace

#endif
