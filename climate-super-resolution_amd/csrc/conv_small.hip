// The shape-specific forward and data-gradient convs, apart from the dispatch that picks them (conv.hip): the dense
// block's <= 16-output conv (conv_n16), the single-output convs (conv_co1m on MFMA, conv_co1 on VALU), the 1x1
// streaming GEMM (conv_pt), the stride-2 data gradient (conv_dgrad_s2) and the 1 <-> C stencil (dgrad_ci1) with its
// three C entries.  conv.hip reaches the first five through fwd_small_launch / fwd_dgrad_s2_launch (conv_route.h).
#include <atomic>
#include <stdio.h>

#include "common.h"
#include "conv_ep.h"
#include "conv_route.h"

using namespace climsr;

// ------------------------------------------------------------------------------------------
// Dense-block conv with <= 16 output channels (RDB conv1-4, esrgan.py:22-25, and their pull data
// gradients): 3x3, stride 1, pad 1, <= 128 input channels.  One 16-row MFMA tile of outputs leaves the
// generic kernel staging- and latency-bound; this one is built for memory-level parallelism:
//  * workgroups are persistent (grid-stride over 8x16-pixel output tiles, 3 per CU) and the NEXT tile's
//    input is loaded into registers while the current one is computed (one pixel per staging thread,
//    compile-time channel offsets: no per-vector index math);
//  * the 4 waves split the K dimension (32-channel blocks; NCB = blocks) x the tile rows (4/NCB groups),
//    so a wave keeps only its 9 weight fragments in VGPRs (loaded once per workgroup);
//  * a B fragment (16 pixels x 32 channels of one input row) is read from LDS once and feeds the three
//    output rows that use it (ky = 0..2);
//  * the per-channel-block partial sums meet in LDS; each wave finishes 2 output rows (fused epilogue).
// Channels are padded to NCB*32 (zero weights, zero LDS pixels).
// ------------------------------------------------------------------------------------------
constexpr int N16_TPH = N16_TH + 2, N16_TPW = TW + 2;

// EP: epilogue specialisation (the per-tile epilogue is branch- and SALU-heavy when every option is a runtime
// flag): 0 = generic (runtime flags), 1 = forward (bias + leaky relu, bf16 out), 2 = pull (leaky-relu
// derivative from the bf16 activation res1, no bias, bf16 out).  The host picks 1/2 only when they match.
template <int NCB, int EP>
__global__ __launch_bounds__(256, NCB == 4 ? 2 : 3) void conv_n16_kernel(FwdArgs a) {
  const bool has_bias = EP == 1 ? true : EP == 2 ? false : a.bias != nullptr;
  const bool has_r1 = EP == 1 ? false : EP == 2 ? true : a.res1 != nullptr;
  const bool has_r2 = EP != 0 ? false : a.res2 != nullptr;
  const bool has_aux = EP != 0 ? false : a.aux != nullptr;
  const int out_mode = EP != 0 ? 0 : a.out_mode;
  const int act = EP == 1 ? 1 : EP == 2 ? 3 : a.act;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  uint16_t* xs = (uint16_t*)smem;
  float* part = (float*)smem;  // partial sums [cb][row][lane] (aliases the input tile after compute)
  constexpr int CINP = NCB * 32, P = CINP + 16, CV = CINP / 8;  // P == 16 (mod 32): conflict-free fragment reads
  constexpr int RG = 4 / NCB, MW = N16_TH / RG;  // row groups, output rows per wave
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, col = lane & 15;
  const int cb = wave % NCB, rg = wave / NCB;
  const int cvec = a.in_c / 8, cvec32 = (a.in_c + 31) / 32 * 4;  // real / 32-block-rounded 16 B channel groups

  float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
  const int co = g * 4;
  if (has_bias) {
    bv.x = co < a.out_c ? a.bias[co] : 0.f;
    bv.y = co + 1 < a.out_c ? a.bias[co + 1] : 0.f;
    bv.z = co + 2 < a.out_c ? a.bias[co + 2] : 0.f;
    bv.w = co + 3 < a.out_c ? a.bias[co + 3] : 0.f;
  }
  const int ntiles = a.tiles_x * a.tiles_y * a.n;
  const bool valign = EP != 0 || (((a.out_cs | a.out_co) & 3) == 0 && (!a.res1 || ((a.r1_cs | a.r1_co) & 3) == 0) &&
                                   (!a.res2 || ((a.r2_cs | a.r2_co) & 3) == 0) && co + 3 < a.out_c);

  // staging: vector v = tid + 256 i of the tile is (pixel v / CV, channel group v % CV); CV is a power of
  // two, so consecutive lanes read consecutive 16 B of a pixel (coalesced) and the pad groups (>= cvec)
  // are stored as zeros without a load
  constexpr int NPIX = N16_TPH * N16_TPW, NV = (NPIX * CV + 255) / 256;
  uint4 pre[NV];
  // buffer loads: out-of-image / pad-channel vectors take an out-of-range offset and read as zeros, so the
  // next tile's loads stay in flight through the current tile's compute (no branch, no early vmcnt wait)
  const __amdgpu_buffer_rsrc_t xr = buf_rsrc(a.x, (uint32_t)((long)a.n * a.in_h * a.in_w * a.in_cs * 2));
  auto issue = [&](int tile) {  // tile < 0: no next tile, every lane takes the out-of-range offset
    const bool live = tile >= 0;
    int tt = live ? tile : 0;
    const int tx = tt % a.tiles_x;
    tt /= a.tiles_x;
    const int ty = tt % a.tiles_y;
    const int nimg = tt / a.tiles_y;
    const int iy0 = ty * N16_TH - 1, ix0 = tx * TW - 1;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int v = tid + 256 * i;
      const int pix = v / CV, j = v % CV;
      const int py = pix / N16_TPW, px = pix - py * N16_TPW;
      const int iy = iy0 + py, ix = ix0 + px;
      const bool ok = live && v < NPIX * CV && j < cvec && iy >= 0 && iy < a.in_h && ix >= 0 && ix < a.in_w;
      const uint32_t off = (uint32_t)(((((nimg * a.in_h + iy) * a.in_w + ix) * a.in_cs) + a.in_co + j * 8) * 2);
      pre[i] = buf_load16(xr, ok ? off : BUF_OOB);
    }
  };
  const TileWalk walk(ntiles);
  if (walk.first < walk.end) issue(walk.first);
  const __amdgpu_buffer_rsrc_t er1 = opt_rsrc(has_r1 ? a.res1 : nullptr), er2 = opt_rsrc(has_r2 ? a.res2 : nullptr),
                               ery = opt_rsrc(out_mode == 2 ? a.y : nullptr);
  // this wave's A fragments (channel block cb, 9 taps; packed rows are tap-major with CINP channels per
  // tap), loaded once per workgroup straight into VGPRs while the first tile's input is in flight
  bf16x8 af[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) af[t] = *(const bf16x8*)(a.w + (long)col * a.kpk + t * CINP + cb * 32 + g * 8);
  // retire them here: the loop below then has no loop-carried VMEM results, and hipcc's wait counting
  // inside it stays exact (no vmcnt(0) before the prefetch can land)
  __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)

  for (int tile = walk.first; tile < walk.end; tile += walk.step) {
    int tt = tile;
    const int tx = tt % a.tiles_x;
    tt /= a.tiles_x;
    const int ty = tt % a.tiles_y;
    const int nimg = tt / a.tiles_y;
    const int oy0 = ty * N16_TH, ox0 = tx * TW;
    lds_barrier();  // the previous tile's LDS reads (partials) are done
    {
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int v = tid + 256 * i;
        // channel groups of fully padded 32-channel blocks are never read (their waves skip the MFMAs)
        if (v < NPIX * CV && (v % CV) < cvec32) *(uint4*)(xs + (v / CV) * P + (v % CV) * 8) = pre[i];
      }
    }
    issue(tile + walk.step < walk.end ? tile + walk.step : -1);  // lands while this tile computes (unconditional:
                                                                  // a branch around it makes hipcc drain it)
    lds_barrier();
    f32x4 acc[MW];
#pragma unroll
    for (int m = 0; m < MW; ++m) acc[m] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (cb * 32 < a.in_c) {  // a wave whose 32-channel block is all padding adds zeros
      const uint16_t* xb = xs + ((rg * MW) * N16_TPW + col) * P + cb * 32 + g * 8;
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        bf16x8 b[MW + 2];  // all input rows of this kx in flight before the first MFMA
#pragma unroll
        for (int ir = 0; ir < MW + 2; ++ir) b[ir] = *(const bf16x8*)(xb + (ir * N16_TPW + kx) * P);
        __builtin_amdgcn_sched_barrier(0);  // keep the reads batched (the scheduler would re-serialise them)
#pragma unroll
        for (int ir = 0; ir < MW + 2; ++ir)
#pragma unroll
          for (int ky = 0; ky < 3; ++ky) {
            const int m = ir - ky;
            if (m >= 0 && m < MW) acc[m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[ky * 3 + kx], b[ir], acc[m], 0, 0, 0);
          }
      }
    }
    lds_barrier();  // input tile reads done: the partials overwrite it
#pragma unroll
    for (int m = 0; m < MW; ++m) *(f32x4*)(part + ((cb * N16_TH + rg * MW + m) * 64 + lane) * 4) = acc[m];
    lds_barrier();
    // epilogue: wave w finishes output rows 2w, 2w+1; lane owns channels co..co+3 of column ox0 + col
    const int ox = ox0 + col;
    f32x4 sum[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      sum[h] = *(const f32x4*)(part + ((0 * N16_TH + wave * 2 + h) * 64 + lane) * 4);
#pragma unroll
      for (int c = 1; c < NCB; ++c) sum[h] += *(const f32x4*)(part + ((c * N16_TH + wave * 2 + h) * 64 + lane) * 4);
    }
    uint2 r1v[2], r2v[2];
    float4 old[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {  // branch-free (opt_rsrc): both rows' operand loads in flight together
      const int oy = oy0 + wave * 2 + h;
      const bool ld = oy < a.out_h && ox < a.out_w && valign;
      const long pidx = ld ? ((long)nimg * a.out_h + oy) * a.out_w + ox : 0;
      const int c = ld ? co : 0;
      r1v[h] = has_r1 ? buf_load8(er1, (uint32_t)((pidx * a.r1_cs + (ld ? a.r1_co : 0) + c) * 2)) : make_uint2(0, 0);
      r2v[h] = has_r2 ? buf_load8(er2, (uint32_t)((pidx * a.r2_cs + (ld ? a.r2_co : 0) + c) * 2)) : make_uint2(0, 0);
      const uint4 o4 = out_mode == 2 ? buf_load16(ery, (uint32_t)((pidx * a.out_cs + (ld ? a.out_co : 0) + c) * 4))
                                     : make_uint4(0, 0, 0, 0);
      old[h] = make_float4(__uint_as_float(o4.x), __uint_as_float(o4.y), __uint_as_float(o4.z), __uint_as_float(o4.w));
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int oy = oy0 + wave * 2 + h;
      if (oy >= a.out_h || ox >= a.out_w || co >= a.out_c) continue;
      const long pidx = ((long)nimg * a.out_h + oy) * a.out_w + ox;
      const float bb[4] = {bv.x, bv.y, bv.z, bv.w};
      float v[4];
      const long ob = pidx * a.out_cs + a.out_co + co;
      if (valign) {
        const uint4 r1 = make_uint4(r1v[h].x, r1v[h].y, 0, 0), r2 = make_uint4(r2v[h].x, r2v[h].y, 0, 0);
#pragma unroll
        for (int i = 0; i < 4; ++i)
          v[i] = ep_res(act_apply(sum[h][i] + bb[i], act, a.slope), act, a.slope, has_r1, res4_at(r1, false, i), a.alpha1,
                        a.beta1, has_r2, res4_at(r2, false, i), a.alpha2, a.beta2);
        if (out_mode == 0) {
          uint2 pk;
          pk.x = (uint32_t)f2bf(v[0]) | ((uint32_t)f2bf(v[1]) << 16);
          pk.y = (uint32_t)f2bf(v[2]) | ((uint32_t)f2bf(v[3]) << 16);
          *(uint2*)((uint16_t*)a.y + ob) = pk;
        } else {
          *(float4*)((float*)a.y + ob) = make_float4(old[h].x + v[0], old[h].y + v[1], old[h].z + v[2], old[h].w + v[3]);
        }
        if (has_aux) {
          uint2 pk;
          pk.x = (uint32_t)f2bf(a.aux_scale * v[0]) | ((uint32_t)f2bf(a.aux_scale * v[1]) << 16);
          pk.y = (uint32_t)f2bf(a.aux_scale * v[2]) | ((uint32_t)f2bf(a.aux_scale * v[3]) << 16);
          *(uint2*)(a.aux + pidx * a.aux_cs + a.aux_co + co) = pk;
        }
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          if (co + i >= a.out_c) continue;
          const float r1 = a.res1 ? res_at(a.res1, false, pidx * a.r1_cs + a.r1_co + co + i) : 0.f;
          const float r2 = a.res2 ? res_at(a.res2, false, pidx * a.r2_cs + a.r2_co + co + i) : 0.f;
          const float x = ep_res(act_apply(sum[h][i] + bb[i], a.act, a.slope), a.act, a.slope, a.res1 != nullptr, r1, a.alpha1,
                                 a.beta1, a.res2 != nullptr, r2, a.alpha2, a.beta2);
          if (a.out_mode == 0) ((uint16_t*)a.y)[ob + i] = f2bf(x);
          else if (a.out_mode == 2) ((float*)a.y)[ob + i] += x;
          else ((float*)a.y)[ob + i] = x;
          if (a.aux) a.aux[pidx * a.aux_cs + a.aux_co + co + i] = f2bf(a.aux_scale * x);
        }
      }
    }
  }
}

template <int NCB, int EP>
static int launch_n16(const FwdArgs& a, hipStream_t s) {
  auto k = conv_n16_kernel<NCB, EP>;
  size_t lds = (size_t)N16_TPH * N16_TPW * (NCB * 32 + 16) * 2;
  const size_t lds_p = (size_t)NCB * N16_TH * 64 * 16;             // partial sums (aliased)
  if (lds_p > lds) lds = lds_p;
  if (int e = lds_opt_in((const void*)k, 160 * 1024)) return e;
  const int ncu = device_cus();
  static std::atomic<int> occ{0};  // workgroups per CU: a property of the kernel and the architecture
  int per_cu = occ.load(std::memory_order_relaxed);
  if (!per_cu) {
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)k, 256, lds) != hipSuccess || per_cu <= 0) per_cu = 2;
    occ.store(per_cu, std::memory_order_relaxed);
  }
  int ntiles = a.tiles_x * a.tiles_y * a.n;
  int grid = ntiles < per_cu * ncu ? ntiles : per_cu * ncu;
  hipLaunchKernelGGL(k, dim3(grid), dim3(256), lds, s, a);
  return check_launch("conv2d_fwd (n16)");
}

// ------------------------------------------------------------------------------------------
// Single-output-channel conv on MFMA (conv_last 64->1 3x3, srcnn.conv3 32->1 5x5 and the data gradient
// of srcnn.conv1 w.r.t. its first input channel, 64->1 9x9).  The horizontal taps go into the MFMA N
// dimension: per output row y and input column x',
//     T[y][x'][kx] = sum_{ky, ci} x[y + ky - R][x'][ci] * w[ky][kx][ci]        (M = x', N = kx, K = ky x ci)
//     out[y][x]    = sum_kx T[y][x + kx - R][kx]                               (shift-sum through LDS)
// so the 16-wide N tile carries KS useful columns instead of 1 (KS/16 vs 1/16 of the MFMA).  A wave
// computes 4 output rows x 64 columns (5 M-fragments of x'), streaming its 4 + KS - 1 input rows straight
// from global memory (16 B per lane, next row in flight during the current row's MFMAs); every input row
// feeds the up-to-4 output rows it touches.  Weights sit in VGPRs for the whole wave.
// ------------------------------------------------------------------------------------------
constexpr int CO1M_NF = 5, CO1M_COLS = 64, CO1M_ROWS = 4;

template <int KS, int NCH>
__global__ __launch_bounds__(256, 2) void conv_co1m_kernel(FwdArgs a) {
  constexpr int R = KS / 2, NR = CO1M_ROWS + KS - 1;
  __shared__ float sc[4][CO1M_NF * 16][17];  // per-wave T rows (x' x kx), padded pitch
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, col = lane & 15;
  const int x0 = blockIdx.x * CO1M_COLS, y0 = (blockIdx.y * 4 + wave) * CO1M_ROWS, nimg = blockIdx.z;
  // B fragments: B[k = ci][n = kx] of tap row ky, channel block c (packed row 0: k = (ci/cc)*kcpad + tap*cc + ci%cc)
  bf16x8 bw[KS][NCH];
#pragma unroll
  for (int ky = 0; ky < KS; ++ky)
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int ci = c * 32 + g * 8;
      bw[ky][c] = (bf16x8){};
      if (col < KS && ci < a.in_c)
        bw[ky][c] = *(const bf16x8*)(a.w + (long)(ci / a.cc) * a.kcpad + (ky * KS + col) * a.cc + (ci % a.cc));
    }
  f32x4 acc[CO1M_ROWS][CO1M_NF];
#pragma unroll
  for (int r = 0; r < CO1M_ROWS; ++r)
#pragma unroll
    for (int f = 0; f < CO1M_NF; ++f) acc[r][f] = (f32x4){0.f, 0.f, 0.f, 0.f};

  bf16x8 xa[2][CO1M_NF][NCH];
  auto load_row = [&](int buf, int iyr) {
    const int iy = y0 - R + iyr;
    const bool rowok = iy >= 0 && iy < a.in_h;
#pragma unroll
    for (int f = 0; f < CO1M_NF; ++f) {
      const int ix = x0 - R + f * 16 + col;
      const bool ok = rowok && ix >= 0 && ix < a.in_w;
      const long base = (((long)nimg * a.in_h + iy) * a.in_w + ix) * a.in_cs + a.in_co;
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        const int ci = c * 32 + g * 8;
        xa[buf][f][c] = (bf16x8){};
        if (ok && ci < a.in_c) xa[buf][f][c] = *(const bf16x8*)(a.x + base + ci);
      }
    }
  };
  load_row(0, 0);
#pragma unroll
  for (int iyr = 0; iyr < NR; ++iyr) {
    if (iyr + 1 < NR) load_row((iyr + 1) & 1, iyr + 1);
#pragma unroll
    for (int ky = 0; ky < KS; ++ky) {
      const int r = iyr - ky;  // output row fed by input row iyr through tap row ky
      if (r < 0 || r >= CO1M_ROWS) continue;
#pragma unroll
      for (int f = 0; f < CO1M_NF; ++f)
#pragma unroll
        for (int c = 0; c < NCH; ++c)
          acc[r][f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xa[iyr & 1][f][c], bw[ky][c], acc[r][f], 0, 0, 0);
    }
  }
  // shift-sum: out[x0 + l] = sum_kx T[x' = l + kx][kx]; then the fused epilogue (same as conv_co1_kernel)
  const float bias = a.bias ? a.bias[0] : 0.f;
  const bool f1 = a.res_f32 & 1;
#pragma unroll
  for (int r = 0; r < CO1M_ROWS; ++r) {
#pragma unroll
    for (int f = 0; f < CO1M_NF; ++f)
#pragma unroll
      for (int i = 0; i < 4; ++i) sc[wave][f * 16 + g * 4 + i][col] = acc[r][f][i];
    float v = 0.f;
#pragma unroll
    for (int kx = 0; kx < KS; ++kx) v += sc[wave][lane + kx][kx];
    const int oy = y0 + r, ox = x0 + lane;
    if (oy < a.out_h && ox < a.out_w) {
      v = act_apply(v + bias, a.act, a.slope);
      const long pidx = ((long)nimg * a.out_h + oy) * a.out_w + ox;
      const float r1 = a.res1 ? res_at(a.res1, f1, pidx * a.r1_cs + a.r1_co) : 0.f;
      v = ep_res(v, a.act, a.slope, a.res1 != nullptr, r1, a.alpha1, a.beta1, false, 0.f, 1.f, 1.f);
      const long ob = pidx * a.out_cs + a.out_co;
      if (a.out_mode == 0) ((uint16_t*)a.y)[ob] = f2bf(v);
      else if (a.out_mode == 2) ((float*)a.y)[ob] += v;
      else ((float*)a.y)[ob] = v;
      if (a.aux) a.aux[pidx * a.aux_cs + a.aux_co] = f2bf(a.aux_scale * v);
    }
  }
}

template <int KS, int NCH>
static int launch_co1m(const FwdArgs& a, hipStream_t s) {
  dim3 grid(ceil_div(a.out_w, CO1M_COLS), ceil_div(a.out_h, 4 * CO1M_ROWS), a.n);
  hipLaunchKernelGGL((conv_co1m_kernel<KS, NCH>), grid, dim3(256), 0, s, a);
  return check_launch("conv2d_fwd (co1m)");
}

// ------------------------------------------------------------------------------------------
// Single-output-channel conv on VALU (v_dot2_f32_bf16): conv_last (64->1), srcnn.conv3 (32->1) and
// the data gradient of srcnn.conv1 w.r.t. its first input channel (64->1, 9x9).  With Cout = 1 an
// MFMA tile would waste 15 of 16 rows; here each thread owns one output pixel of a 16x16 tile, the
// input tile (CO1_CC channels at a time) sits in LDS and the weights are wave-uniform scalar loads.
// ------------------------------------------------------------------------------------------
constexpr int CO1_CC = 32;

__global__ __launch_bounds__(256) void conv_co1_kernel(FwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  uint16_t* xs = (uint16_t*)smem;
  constexpr int XPITCH = CO1_CC + 8;
  uint16_t* wsm = (uint16_t*)(smem + (size_t)(15 + a.ks) * (15 + a.ks) * XPITCH * 2);  // [tap][CO1_CC]
  const int tid = threadIdx.x;
  int bid = blockIdx.x;
  const int tx = bid % a.tiles_x;
  bid /= a.tiles_x;
  const int ty = bid % a.tiles_y;
  const int nimg = bid / a.tiles_y;
  const int ox0 = tx * 16, oy0 = ty * 16;
  const int py = tid >> 4, px = tid & 15;
  const int tph = 15 + a.ks, tpw = 15 + a.ks;
  const int iy0 = oy0 - a.pad, ix0 = ox0 - a.pad;
  const int kcpad = a.kcpad;
  float acc = 0.f;
  constexpr int cvec = CO1_CC / 8;
  const int nvec = tph * tpw * cvec;
  for (int c0 = 0; c0 < a.in_c; c0 += CO1_CC) {
    __syncthreads();
    for (int base = 0; base < nvec; base += 256 * FWD_MAXV) {
      uint4 buf[FWD_MAXV];
#pragma unroll
      for (int i = 0; i < FWD_MAXV; ++i) {
        const int v = base + tid + i * 256;
        uint4 val = make_uint4(0, 0, 0, 0);
        if (v < nvec) {
          const int pix = v / cvec, cg = v % cvec;  // cvec compile-time
          const int yy = pix / tpw, xx = pix - (pix / tpw) * tpw;
          const int iy = iy0 + yy, ix = ix0 + xx, c = c0 + cg * 8;
          if (iy >= 0 && iy < a.in_h && ix >= 0 && ix < a.in_w && c < a.in_c)
            val = *(const uint4*)(a.x + (((long)nimg * a.in_h + iy) * a.in_w + ix) * a.in_cs + a.in_co + c);
        }
        buf[i] = val;
      }
#pragma unroll
      for (int i = 0; i < FWD_MAXV; ++i) {
        const int v = base + tid + i * 256;
        if (v < nvec) {
          const int pix = v / cvec, cg = v % cvec;
          *(uint4*)(xs + pix * XPITCH + cg * 8) = buf[i];
        }
      }
    }
    // weights of this channel chunk, [tap][CO1_CC] (packed row 0: k = (c/cc)*kcpad + tap*cc + c%cc)
    for (int v = tid; v < a.ks * a.ks * cvec; v += 256) {
      const int tap = v / cvec, cg = v % cvec, c = c0 + cg * 8;
      uint4 val = make_uint4(0, 0, 0, 0);
      if (c < a.in_c) val = *(const uint4*)(a.w + (c / a.cc) * kcpad + tap * a.cc + (c % a.cc));
      *(uint4*)(wsm + tap * CO1_CC + cg * 8) = val;
    }
    __syncthreads();
    const int cn = min(CO1_CC, a.in_c - c0);
    for (int ky = 0; ky < a.ks; ++ky) {
      for (int kx = 0; kx < a.ks; ++kx) {
        const int tap = ky * a.ks + kx;
        const uint16_t* xp = xs + ((py + ky) * tpw + px + kx) * XPITCH;
        const uint16_t* wp = wsm + tap * CO1_CC;
        for (int cg = 0; cg < cn; cg += 8) {
          const uint4 wv = *(const uint4*)(wp + cg);  // same address in every lane: LDS broadcast
          const uint4 xv = *(const uint4*)(xp + cg);
          const uint32_t xw[4] = {xv.x, xv.y, xv.z, xv.w}, ww[4] = {wv.x, wv.y, wv.z, wv.w};
#pragma unroll
          for (int q = 0; q < 4; ++q)
            acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2, xw[q]), __builtin_bit_cast(bf16x2, ww[q]), acc, false);
        }
      }
    }
  }
  const int oy = oy0 + py, ox = ox0 + px;
  if (oy >= a.out_h || ox >= a.out_w) return;
  float v = acc + (a.bias ? a.bias[0] : 0.f);
  v = act_apply(v, a.act, a.slope);
  const long pidx = ((long)nimg * a.out_h + oy) * a.out_w + ox;
  const bool f1 = a.res_f32 & 1, f2 = (a.res_f32 >> 1) & 1;
  const float r1 = a.res1 ? res_at(a.res1, f1, pidx * a.r1_cs + a.r1_co) : 0.f;
  const float r2 = a.res2 ? res_at(a.res2, f2, pidx * a.r2_cs + a.r2_co) : 0.f;
  v = ep_res(v, a.act, a.slope, a.res1 != nullptr, r1, a.alpha1, a.beta1, a.res2 != nullptr, r2, a.alpha2, a.beta2);
  const long ob = pidx * a.out_cs + a.out_co;
  if (a.out_mode == 0) ((uint16_t*)a.y)[ob] = f2bf(v);
  else if (a.out_mode == 2) ((float*)a.y)[ob] += v;
  else ((float*)a.y)[ob] = v;
  if (a.aux) a.aux[pidx * a.aux_cs + a.aux_co] = f2bf(a.aux_scale * v);
}

static int launch_co1(const FwdArgs& a, hipStream_t s) {
  size_t lds = (size_t)(15 + a.ks) * (15 + a.ks) * (CO1_CC + 8) * 2 + (size_t)a.ks * a.ks * CO1_CC * 2;
  hipLaunchKernelGGL(conv_co1_kernel, dim3(a.tiles_x * a.tiles_y * a.n), dim3(256), lds, s, a);
  return check_launch("conv2d_fwd (co1)");
}

// ------------------------------------------------------------------------------------------
// 1x1 conv as a streaming GEMM (srcnn.conv2 64->32 and its 32->64 data gradient with the ReLU mask):
// out[p][co] = epilogue(sum_ci x[p][ci] w[co][ci]).  Nothing is reused across pixels except the weights, so
// nothing goes through LDS: the weight fragments sit in VGPRs, each lane loads its 16 B channel slice of a
// pixel straight into the B fragment (16 pixels x 32 channels per load round), U groups of 16 pixels are in
// flight per wave, and the fused epilogue stores 4 consecutive channels per lane.  HBM-bound by design.
// ------------------------------------------------------------------------------------------
constexpr int PT_U = 4;  // 16-pixel groups per wave iteration

// EP: 0 generic (runtime flags); 3 activation forward (bias + leaky relu / relu, bf16 out); 4 activation backward
// (act' from the bf16 activation res1, no bias, bf16 out) -- srcnn.conv2's forward and data gradient.
template <int NCOF, int NKC, int EP = 0>
__global__ __launch_bounds__(256) void conv_pt_kernel(FwdArgs a, long npix) {
  __shared__ float tsm[NCOF == 4 ? 4 * 16 * 68 : 1];
  const int lane = threadIdx.x & 63, g = lane >> 4, col = lane & 15;
  bf16x8 af[NCOF][NKC];
#pragma unroll
  for (int f = 0; f < NCOF; ++f)
#pragma unroll
    for (int k = 0; k < NKC; ++k) af[f][k] = *(const bf16x8*)(a.w + (long)(f * 16 + col) * a.kpk + k * 32 + g * 8);
  float bb[NCOF][4];
#pragma unroll
  for (int f = 0; f < NCOF; ++f)
#pragma unroll
    for (int i = 0; i < 4; ++i)
      bb[f][i] = ((EP == 3 || (EP == 0 && a.bias)) && f * 16 + g * 4 + i < a.out_c) ? a.bias[f * 16 + g * 4 + i] : 0.f;
  const bool f1 = EP != 0 ? false : (a.res_f32 & 1) != 0, f2 = EP != 0 ? false : ((a.res_f32 >> 1) & 1) != 0;
  const bool has_bias = EP == 3 ? true : EP == 4 ? false : a.bias != nullptr;
  const bool has1 = EP == 3 ? false : EP == 4 ? true : a.res1 != nullptr;
  const bool has2 = EP != 0 ? false : a.res2 != nullptr;
  const bool has_aux = EP != 0 ? false : a.aux != nullptr;
  const int out_mode = EP != 0 ? 0 : a.out_mode;
  const long ngroups = (npix + 15) / 16;
  const long wave_id = ((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const long nwaves = ((long)gridDim.x * blockDim.x) >> 6;
  // input groups are loaded one iteration ahead with range-checked buffer loads (zeros past npix, no branch),
  // so the next group's loads are in flight through this group's epilogue
  const __amdgpu_buffer_rsrc_t xr = buf_rsrc(a.x, (uint32_t)(npix * a.in_cs * 2));
  const __amdgpu_buffer_rsrc_t rr1 = opt_rsrc(has1 ? a.res1 : nullptr), rr2 = opt_rsrc(has2 ? a.res2 : nullptr);
  bf16x8 bn[PT_U][NKC];
  auto ldx = [&](long g0) {
#pragma unroll
    for (int u = 0; u < PT_U; ++u) {
      const long p = (g0 + u) * 16 + col;
#pragma unroll
      for (int k = 0; k < NKC; ++k) {
        const uint4 v = buf_load16(xr, p < npix ? (uint32_t)((p * a.in_cs + a.in_co + k * 32 + g * 8) * 2) : BUF_OOB);
        bn[u][k] = __builtin_bit_cast(bf16x8, v);
      }
    }
  };
  ldx(wave_id * PT_U);
  for (long g0 = wave_id * PT_U; g0 < ngroups; g0 += nwaves * PT_U) {
    bf16x8 bx[PT_U][NKC];
#pragma unroll
    for (int u = 0; u < PT_U; ++u)
#pragma unroll
      for (int k = 0; k < NKC; ++k) bx[u][k] = bn[u][k];
    ldx(g0 + nwaves * PT_U);
#pragma unroll
    for (int u = 0; u < PT_U; ++u) {
      const long p = (g0 + u) * 16 + col;
      f32x4 acc[NCOF];
#pragma unroll
      for (int f = 0; f < NCOF; ++f) {
        acc[f] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < NKC; ++k) acc[f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[f][k], bx[u][k], acc[f], 0, 0, 0);
      }
      if (NCOF == 4) {  // transpose through this wave's LDS so each lane owns 16 channels of one pixel and a store
                        // instruction covers whole lines (the 8 B-per-lane MFMA layout touches 16 lines per store)
        float* tw = tsm + (threadIdx.x >> 6) * (16 * 68);
#pragma unroll
        for (int f = 0; f < NCOF; ++f)
#pragma unroll
          for (int i = 0; i < 4; ++i) tw[col * 68 + f * 16 + g * 4 + i] = acc[f][i];
        const int pp = lane / NCOF, c0 = (lane % NCOF) * 16;  // NCOF lanes per pixel
        const long q = (g0 + u) * 16 + pp;
        float v[16];
        const int ppr = pp < 16 ? pp : 15;  // lanes beyond the 16 pixels (NCOF 2) read a valid row and store nothing
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const f32x4 t4 = *(const f32x4*)(tw + ppr * 68 + c0 + 4 * j);
#pragma unroll
          for (int i = 0; i < 4; ++i) v[4 * j + i] = t4[i];
        }
        const bool okq = pp < 16 && q < npix;
        uint4 r1s[4], r2s[4];  // every residual load of this pixel before the first use (branch-free)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const long qq = okq ? q : 0;
          const int co = okq ? c0 + 4 * j : 0;
          if (EP == 0 || has1) {
            if (f1) r1s[j] = buf_load16(rr1, (uint32_t)((qq * a.r1_cs + (okq ? a.r1_co : 0) + co) * 4));
            else { const uint2 t2 = buf_load8(rr1, (uint32_t)((qq * a.r1_cs + (okq ? a.r1_co : 0) + co) * 2)); r1s[j] = make_uint4(t2.x, t2.y, 0, 0); }
          } else r1s[j] = make_uint4(0, 0, 0, 0);
          if (EP == 0 || has2) {
            if (f2) r2s[j] = buf_load16(rr2, (uint32_t)((qq * a.r2_cs + (okq ? a.r2_co : 0) + co) * 4));
            else { const uint2 t2 = buf_load8(rr2, (uint32_t)((qq * a.r2_cs + (okq ? a.r2_co : 0) + co) * 2)); r2s[j] = make_uint4(t2.x, t2.y, 0, 0); }
          } else r2s[j] = make_uint4(0, 0, 0, 0);
        }
        if (okq) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int co = c0 + 4 * j;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const float bsv = has_bias ? a.bias[co + i] : 0.f;
              v[4 * j + i] = ep_res(act_apply(v[4 * j + i] + bsv, a.act, a.slope), a.act, a.slope, has1, res4_at(r1s[j], f1, i),
                                    a.alpha1, a.beta1, has2, res4_at(r2s[j], f2, i), a.alpha2, a.beta2);
            }
          }
          const long ob = q * a.out_cs + a.out_co + c0;
          if (out_mode == 0) {
            uint4 w0, w1;
            w0.x = (uint32_t)f2bf(v[0]) | ((uint32_t)f2bf(v[1]) << 16);
            w0.y = (uint32_t)f2bf(v[2]) | ((uint32_t)f2bf(v[3]) << 16);
            w0.z = (uint32_t)f2bf(v[4]) | ((uint32_t)f2bf(v[5]) << 16);
            w0.w = (uint32_t)f2bf(v[6]) | ((uint32_t)f2bf(v[7]) << 16);
            w1.x = (uint32_t)f2bf(v[8]) | ((uint32_t)f2bf(v[9]) << 16);
            w1.y = (uint32_t)f2bf(v[10]) | ((uint32_t)f2bf(v[11]) << 16);
            w1.z = (uint32_t)f2bf(v[12]) | ((uint32_t)f2bf(v[13]) << 16);
            w1.w = (uint32_t)f2bf(v[14]) | ((uint32_t)f2bf(v[15]) << 16);
            *(uint4*)((uint16_t*)a.y + ob) = w0;
            *(uint4*)((uint16_t*)a.y + ob + 8) = w1;
          } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
              if (out_mode == 2) o = *(const float4*)((const float*)a.y + ob + 4 * j);
              *(float4*)((float*)a.y + ob + 4 * j) =
                  make_float4(o.x + v[4 * j], o.y + v[4 * j + 1], o.z + v[4 * j + 2], o.w + v[4 * j + 3]);
            }
          }
          if (has_aux) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              uint2 pk;
              pk.x = (uint32_t)f2bf(a.aux_scale * v[4 * j]) | ((uint32_t)f2bf(a.aux_scale * v[4 * j + 1]) << 16);
              pk.y = (uint32_t)f2bf(a.aux_scale * v[4 * j + 2]) | ((uint32_t)f2bf(a.aux_scale * v[4 * j + 3]) << 16);
              *(uint2*)(a.aux + q * a.aux_cs + a.aux_co + c0 + 4 * j) = pk;
            }
          }
        }
        continue;
      }
      uint4 r1s[NCOF], r2s[NCOF];  // all residual loads of this pixel first (branch-free)
#pragma unroll
      for (int f = 0; f < NCOF; ++f) {
        const int co = f * 16 + g * 4;
        const bool okf = p < npix && co < a.out_c;
        const long pp = okf ? p : 0;
        const int cc = okf ? co : 0;
        if (EP == 0 || has1) {
          if (f1) r1s[f] = buf_load16(rr1, (uint32_t)((pp * a.r1_cs + (okf ? a.r1_co : 0) + cc) * 4));
          else { const uint2 t2 = buf_load8(rr1, (uint32_t)((pp * a.r1_cs + (okf ? a.r1_co : 0) + cc) * 2)); r1s[f] = make_uint4(t2.x, t2.y, 0, 0); }
        } else r1s[f] = make_uint4(0, 0, 0, 0);
        if (EP == 0 || has2) {
          if (f2) r2s[f] = buf_load16(rr2, (uint32_t)((pp * a.r2_cs + (okf ? a.r2_co : 0) + cc) * 4));
          else { const uint2 t2 = buf_load8(rr2, (uint32_t)((pp * a.r2_cs + (okf ? a.r2_co : 0) + cc) * 2)); r2s[f] = make_uint4(t2.x, t2.y, 0, 0); }
        } else r2s[f] = make_uint4(0, 0, 0, 0);
      }
      if (p >= npix) continue;
#pragma unroll
      for (int f = 0; f < NCOF; ++f) {
        const int co = f * 16 + g * 4;
        if (co >= a.out_c) continue;
        const uint4 r1 = r1s[f], r2 = r2s[f];
        const long ob = p * a.out_cs + a.out_co + co;
        float v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
          v[i] = ep_res(act_apply(acc[f][i] + bb[f][i], a.act, a.slope), a.act, a.slope, has1, res4_at(r1, f1, i), a.alpha1,
                        a.beta1, has2, res4_at(r2, f2, i), a.alpha2, a.beta2);
        if (out_mode == 0) {
          uint2 pk;
          pk.x = (uint32_t)f2bf(v[0]) | ((uint32_t)f2bf(v[1]) << 16);
          pk.y = (uint32_t)f2bf(v[2]) | ((uint32_t)f2bf(v[3]) << 16);
          *(uint2*)((uint16_t*)a.y + ob) = pk;
        } else {
          float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
          if (out_mode == 2) o = *(const float4*)((const float*)a.y + ob);
          *(float4*)((float*)a.y + ob) = make_float4(o.x + v[0], o.y + v[1], o.z + v[2], o.w + v[3]);
        }
        if (has_aux) {
          uint2 pk;
          pk.x = (uint32_t)f2bf(a.aux_scale * v[0]) | ((uint32_t)f2bf(a.aux_scale * v[1]) << 16);
          pk.y = (uint32_t)f2bf(a.aux_scale * v[2]) | ((uint32_t)f2bf(a.aux_scale * v[3]) << 16);
          *(uint2*)(a.aux + p * a.aux_cs + a.aux_co + co) = pk;
        }
      }
    }
  }
}

template <int NCOF, int NKC>
static int launch_pt(int ep, const FwdArgs& a, hipStream_t s) {
  const long npix = (long)a.n * a.out_h * a.out_w;
  const long groups = (npix + 15) / 16;
  long blocks = (groups + 4 * PT_U - 1) / (4 * PT_U);
  if (blocks > 4096) blocks = 4096;
  if (ep == 3) hipLaunchKernelGGL((conv_pt_kernel<NCOF, NKC, 3>), dim3((unsigned)blocks), dim3(256), 0, s, a, npix);
  else if (ep == 4) hipLaunchKernelGGL((conv_pt_kernel<NCOF, NKC, 4>), dim3((unsigned)blocks), dim3(256), 0, s, a, npix);
  else hipLaunchKernelGGL((conv_pt_kernel<NCOF, NKC, 0>), dim3((unsigned)blocks), dim3(256), 0, s, a, npix);
  return check_launch("conv2d_fwd (pt)");
}

// CO1M, CO1, N16, PT: the instantiation of the route's ids
int climsr::fwd_small_launch(const FwdRoute& r, const FwdArgs& a, hipStream_t s) {
  if (r.family == FAM_CO1) return launch_co1(a, s);
#define CO1M_CASE(KS, NCH) \
  if (r.family == FAM_CO1M && r.ks == KS && r.nch == NCH) return launch_co1m<KS, NCH>(a, s);
#define N16_CASE(NCB, EP) \
  if (r.family == FAM_N16 && r.nch == NCB && r.ep == EP) return launch_n16<NCB, EP>(a, s);
#define PT_CASE(NCOF, NKC) \
  if (r.family == FAM_PT && r.nt == NCOF && r.nch == NKC) return launch_pt<NCOF, NKC>(r.ep, a, s);
  CO1M_CASE(3, 1) CO1M_CASE(3, 2) CO1M_CASE(5, 1) CO1M_CASE(5, 2) CO1M_CASE(9, 1) CO1M_CASE(9, 2)
  N16_CASE(1, 0) N16_CASE(1, 1) N16_CASE(1, 2) N16_CASE(2, 0) N16_CASE(2, 1) N16_CASE(2, 2) N16_CASE(4, 0) N16_CASE(4, 1) N16_CASE(4, 2)
  PT_CASE(1, 1) PT_CASE(1, 2) PT_CASE(1, 4) PT_CASE(2, 1) PT_CASE(2, 2) PT_CASE(2, 4) PT_CASE(4, 1) PT_CASE(4, 2) PT_CASE(4, 4)
#undef CO1M_CASE
#undef N16_CASE
#undef PT_CASE
  set_error("conv2d_fwd: no small-shape kernel for family %d (ks %d, nch %d, nt %d, ep %d)", r.family, r.ks, r.nch, r.nt, r.ep);
  return CLIMSR_EINVAL;
}

// ------------------------------------------------------------------------------------------
// Data gradient of a 3x3 / stride-2 / pad-1 conv (the discriminator's downsampling convs, rfb_esrgan.py:30-48),
// phase-decomposed.  The zero-inserted form (a stride-1 conv over the 2x-upsampled dz, up = -2) spends 3 of every
// 4 MFMAs on inserted zeros; here a dx pixel (2i+a, 2j+b) sums only its own taps: with the transposed, flipped
// weights of wpk_t (tap (ky, kx) = forward tap (2-ky, 2-kx)), tap (ky, kx) feeds phase (ky != 1, kx != 1) from dz
// pixel (i + (ky == 2), j + (kx == 2)).  Every tap is one k-step (32-channel chunks), 9 k-steps per chunk in all.
// Workgroup: 16 x 16 dz positions (32 x 32 dx pixels) x 32 dx channels; wave w owns dz rows 4w..4w+3 and keeps
// 4 phases x 4 rows x 2 channel blocks of accumulators.  The taps are walked grouped by dz offset, so a B fragment
// (16 dz pixels x 32 channels) is read once per offset (4 per chunk, not 9).  dz tile 17 x 17 pixels (+ right /
// bottom halo) and the weight chunk are staged in LDS, the next chunk prefetched into registers during the
// MFMAs.  Epilogue per phase through LDS (fp32), 16 B bf16 stores, optional LeakyReLU/ReLU backward from the
// bf16 activation res1 at the dx pixel (EP 4: the layer-1 data gradient writing layer 0's output gradient).
// ------------------------------------------------------------------------------------------
constexpr int S2D_TPW = 17, S2D_CCP = 48, S2D_WP = 9 * 32 + WPAD;
template <int MW>
constexpr int s2d_lds(int nt) { return (4 * MW + 1) * S2D_TPW * S2D_CCP * 2 + nt * 16 * S2D_WP * 2; }

// MW dz rows per wave x NT 16-channel blocks (MW * NT = 8: 4 x 2 for >= 128 dx channels, 2 x 4 -- whole 128 B
// pixel lines per workgroup -- for 64)
template <int EP, int MW, int NT>
__global__ __launch_bounds__(256, 2) void conv_dgrad_s2_kernel(FwdArgs a) {
  constexpr int TPH = 4 * MW + 1, CO = NT * 16, EPP = CO + 4;
  constexpr int NRX = (TPH * S2D_TPW * 4 + 255) / 256, NRW = (CO * 36 + 255) / 256;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  uint16_t* xs = (uint16_t*)smem;
  uint16_t* ws = (uint16_t*)(smem + TPH * S2D_TPW * S2D_CCP * 2);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, col = lane & 15;
  // XCD-paired order: the channel blocks of one tile are 8 workgroups apart, i.e. on the same XCD (round-robin
  // dispatch) at about the same time, so they share the dz tile in that L2 and complete each other's partial
  // dx lines there (a block writes 64 of a pixel's 128 B at 64 channels)
  const int ncob = a.out_c / CO, grp = blockIdx.x / (8 * ncob), r8 = blockIdx.x % (8 * ncob);
  int bid = grp * 8 + (r8 & 7);
  if (bid >= a.tiles_x * a.tiles_y * a.n) return;
  const int tx = bid % a.tiles_x;
  bid /= a.tiles_x;
  const int ty = bid % a.tiles_y;
  const int nimg = bid / a.tiles_y;
  const int j0 = tx * 16, i0 = ty * 4 * MW, co0 = (r8 >> 3) * CO;

  f32x4 acc[4][MW][NT];
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int m = 0; m < MW; ++m)
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[p][m][t] = (f32x4){0.f, 0.f, 0.f, 0.f};

  uint4 px[NRX], pw[NRW];
  auto issue = [&](int j) {
#pragma unroll
    for (int r = 0; r < NRX; ++r) {
      const int v = tid + 256 * r, pix = v >> 2, cg = v & 3;
      const int yy = i0 + pix / S2D_TPW, xx = j0 + pix % S2D_TPW;
      px[r] = make_uint4(0, 0, 0, 0);
      if (pix < TPH * S2D_TPW && yy < a.in_h && xx < a.in_w)
        px[r] = *(const uint4*)(a.x + (((long)nimg * a.in_h + yy) * a.in_w + xx) * a.in_cs + a.in_co + j * 32 + cg * 8);
    }
#pragma unroll
    for (int r = 0; r < NRW; ++r) {
      const int v = tid + 256 * r, row = v / 36, kv = v % 36;
      pw[r] = make_uint4(0, 0, 0, 0);
      if (row < CO) pw[r] = *(const uint4*)(a.w + (long)(co0 + row) * a.kpk + (long)j * 288 + kv * 8);
    }
  };
  auto stash = [&]() {
#pragma unroll
    for (int r = 0; r < NRX; ++r) {
      const int v = tid + 256 * r, pix = v >> 2, cg = v & 3;
      if (pix < TPH * S2D_TPW) *(uint4*)(xs + pix * S2D_CCP + cg * 8) = px[r];
    }
#pragma unroll
    for (int r = 0; r < NRW; ++r) {
      const int v = tid + 256 * r, row = v / 36, kv = v % 36;
      if (row < CO) *(uint4*)(ws + row * S2D_WP + kv * 8) = pw[r];
    }
  };
  // taps grouped by dz offset (dy, dx): (0,0): ky,kx in {0,1}; (0,1): kx = 2; (1,0): ky = 2; (1,1): (2,2)
  constexpr int TKY[9] = {0, 0, 1, 1, 0, 1, 2, 2, 2}, TKX[9] = {0, 1, 0, 1, 2, 2, 0, 1, 2};
  const uint16_t* xb = xs + (wave * MW * S2D_TPW + col) * S2D_CCP + g * 8;
  const uint16_t* wb = ws + col * S2D_WP + g * 8;
  auto compute = [&]() {
    bf16x8 af[2][NT], bf[2][MW];
    auto lda = [&](int st, int b) {
      const int tap = TKY[st] * 3 + TKX[st];
#pragma unroll
      for (int t = 0; t < NT; ++t) af[b][t] = *(const bf16x8*)(wb + t * 16 * S2D_WP + tap * 32);
    };
    auto ldb = [&](int st, int b) {
      const int off = ((TKY[st] == 2) * S2D_TPW + (TKX[st] == 2)) * S2D_CCP;
#pragma unroll
      for (int m = 0; m < MW; ++m) bf[b][m] = *(const bf16x8*)(xb + m * S2D_TPW * S2D_CCP + off);
    };
    lda(0, 0);
    ldb(0, 0);
    int bb = 0;
#pragma unroll
    for (int st = 0; st < 9; ++st) {
      const bool newb = st + 1 < 9 && (st + 1 == 4 || st + 1 == 6 || st + 1 == 8);
      if (st + 1 < 9) lda(st + 1, (st + 1) & 1);
      if (newb) ldb(st + 1, bb ^ 1);
      const int ph = (TKY[st] != 1) * 2 + (TKX[st] != 1);
#pragma unroll
      for (int m = 0; m < MW; ++m)
#pragma unroll
        for (int t = 0; t < NT; ++t)
          acc[ph][m][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[st & 1][t], bf[bb][m], acc[ph][m][t], 0, 0, 0);
      if (newb) bb ^= 1;
    }
  };
  issue(0);
  for (int j = 0; j < a.nchunk; ++j) {
    __syncthreads();  // chunk j-1's fragment reads are done
    stash();
    if (j + 1 < a.nchunk) issue(j + 1);  // lands while chunk j computes
    __syncthreads();
    compute();
  }

  // epilogue, one phase at a time: fp32 [64 px][32 ch] per wave in LDS, then 8 channels (16 B bf16) per item
  float* eb = (float*)smem + wave * (MW * 16 * EPP);
  constexpr int NG = CO / 8;  // 16 B channel groups per pixel
  const __amdgpu_buffer_rsrc_t rr1 = opt_rsrc(EP == 4 ? a.res1 : nullptr);
  // item (phase ph, k): pixel it / NG of the wave's MW x 16 dz positions, channels (it % NG) * 8, it = lane + 64 k;
  // the activation operand of all 4 phases is loaded up front (one HBM latency, not four)
  auto item_pidx = [&](int ph, int k, bool& ok) -> long {
    const int it = lane + 64 * k, pl = it / NG;
    const int py = 2 * (i0 + wave * MW + (pl >> 4)) + (ph >> 1), pxx = 2 * (j0 + (pl & 15)) + (ph & 1);
    ok = py < a.out_h && pxx < a.out_w;
    return ok ? ((long)nimg * a.out_h + py) * a.out_w + pxx : 0;
  };
  uint4 r1[4][4];
  // EP 10: the BatchNorm-backward partials of the stored dx (store_tile_lds EP 10): z is loaded per phase (not up
  // front like the activation operand: 64 more registers beside the 128 accumulators spilled); the lane's 8
  // channels are the same for all of its items (64 % NG == 0)
  const __amdgpu_buffer_rsrc_t rrz = opt_rsrc(EP == 10 ? (const void*)a.bz : nullptr);
  const int cgl = lane % NG;
  float bmu[8], brs[8], bsc[8], bsh[8], ssum[8], ssq[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    ssum[i] = 0.f;
    ssq[i] = 0.f;
    if constexpr (EP == 10) {
      const int c = co0 + cgl * 8 + i;
      bmu[i] = a.bmean[c];
      brs[i] = a.brstd[c];
      bsc[i] = a.bgamma[c] * brs[i];
      bsh[i] = a.bbeta[c] - bmu[i] * bsc[i];
    }
  }
#pragma unroll
  for (int ph = 0; ph < 4; ++ph)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      r1[ph][k] = make_uint4(0, 0, 0, 0);
      if (EP == 4) {
        bool ok;
        const long pidx = item_pidx(ph, k, ok);
        r1[ph][k] = buf_load16(rr1, (uint32_t)((pidx * a.r1_cs + (ok ? a.r1_co + co0 + ((lane + 64 * k) % NG) * 8 : 0)) * 2));
      }
    }
#pragma unroll
  for (int ph = 0; ph < 4; ++ph) {
    uint4 zv[4];
    if constexpr (EP == 10) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        bool ok;
        const long pidx = item_pidx(ph, k, ok);
        // (opt_rsrc has no range limit: a pixel outside the image reads pixel 0, whose d is 0)
        zv[k] = buf_load16(rrz, (uint32_t)((pidx * a.bz_cs + co0 + cgl * 8) * 2));
      }
    }
    __syncthreads();  // operands (first phase) / the previous phase's reads are done
#pragma unroll
    for (int m = 0; m < MW; ++m)
#pragma unroll
      for (int t = 0; t < NT; ++t) *(f32x4*)(eb + (m * 16 + col) * EPP + t * 16 + g * 4) = acc[ph][m][t];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int it = lane + 64 * k, pl = it / NG, cg = it % NG;
      bool ok;
      const long oidx = item_pidx(ph, k, ok) * a.out_cs + a.out_co + co0 + cg * 8;
      const float4 s0 = *(const float4*)(eb + pl * EPP + cg * 8), s1 = *(const float4*)(eb + pl * EPP + cg * 8 + 4);
      float v[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
      if (EP == 4) {
        Raw8 rr;
        rr.lo = r1[ph][k];
        rr.hi = make_uint4(0, 0, 0, 0);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const float r = raw8_at(rr, false, i);
          v[i] = a.act == 3 ? (r > 0.f ? v[i] : v[i] * a.slope) : (r > 0.f ? v[i] : 0.f);
        }
      }
      const uint4 pk = pack8_bf16(v, 1.f);
      if (ok) *(uint4*)((uint16_t*)a.y + oidx) = pk;
      if constexpr (EP == 10) {
        Raw8 rr, rz;
        rr.lo = pk;
        rz.lo = zv[k];
        rr.hi = rz.hi = make_uint4(0, 0, 0, 0);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const float r = ok ? raw8_at(rr, false, i) : 0.f, z = raw8_at(rz, false, i);
          const float d = fmaf(z, bsc[i], bsh[i]) > 0.f ? r : r * a.bslope;
          ssum[i] += d;
          ssq[i] = fmaf(d, (z - bmu[i]) * brs[i], ssq[i]);
        }
      }
    }
  }
  if constexpr (EP == 10) {
    // lanes with equal lane % NG hold the same 8 channels: xor-shuffles over the other lane bits, then the 4 waves
    // meet in LDS (the staging is free after a barrier) and part[tile][0 / 1][co0 + ch] gets fixed-order fp64 sums
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int m = NG; m < 64; m <<= 1) {
        ssum[i] += __shfl_xor(ssum[i], m);
        ssq[i] += __shfl_xor(ssq[i], m);
      }
    float* red = (float*)smem;
    lds_barrier();  // every wave's reads of the last phase's staging are done
    if (lane < NG) {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        red[wave * 2 * CO + lane * 8 + i] = ssum[i];
        red[wave * 2 * CO + CO + lane * 8 + i] = ssq[i];
      }
    }
    lds_barrier();
    if (tid < CO) {
      float ts = 0.f, tq = 0.f;
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        ts += red[w * 2 * CO + tid];
        tq += red[w * 2 * CO + CO + tid];
      }
      const long tile = ((long)nimg * a.tiles_y + ty) * a.tiles_x + tx;
      double* out = a.bn_part + tile * 2 * a.out_c;
      out[co0 + tid] = (double)ts;
      out[a.out_c + co0 + tid] = (double)tq;
    }
  }
}

template <int MW, int NT>
static int launch_dgrad_s2_t(const FwdRoute& r, const FwdArgs& a, hipStream_t s) {
  dim3 grid(ceil_div(a.tiles_x * a.tiles_y * a.n, 8) * 8 * (a.out_c / (NT * 16)));
  const int lds = s2d_lds<MW>(NT);

  if (r.ep == 4) hipLaunchKernelGGL((conv_dgrad_s2_kernel<4, MW, NT>), grid, dim3(256), lds, s, a);
  else if (r.ep == 10) hipLaunchKernelGGL((conv_dgrad_s2_kernel<10, MW, NT>), grid, dim3(256), lds, s, a);
  else hipLaunchKernelGGL((conv_dgrad_s2_kernel<0, MW, NT>), grid, dim3(256), lds, s, a);
  return check_launch("conv2d_fwd (dgrad s2)");
}

// 2 x 4 (64 dx channels: whole 128 B pixel lines per workgroup) or 4 x 2, as the route chose
int climsr::fwd_dgrad_s2_launch(const FwdRoute& r, const FwdArgs& a, hipStream_t s) {
  if (r.mw == 2) return launch_dgrad_s2_t<2, 4>(r, a, s);
  return launch_dgrad_s2_t<4, 2>(r, a, s);
}

// ------------------------------------------------------------------------------------------
// Data gradient of a conv with ONE output channel (conv_last 64->1 3x3, srcnn.conv3 32->1 5x5; esrgan.py:99,
// srcnn.py:17): g[q][c] = act'(res1[q][c]) * sum_{ky,kx} W[0][c][ky][kx] * dz[q - (ky,kx) + pad].  A 1 -> C
// stencil, not a GEMM (K = ks^2 taps of one channel): one 16x16-pixel tile per workgroup, the dz tile (+halo)
// and the fp32 weights in LDS, each thread one pixel x 8 channels per step (16 B residual load, 16 B store).
// Bound by HBM (the residual read and the output write).  The implicit-GEMM path padded K to 32 and ran the
// epilogue of a 64-output MFMA tile per 2 input channels (conv_last dgrad 222 us, srcnn.conv3 dgrad 144 us).
// ------------------------------------------------------------------------------------------
constexpr int S1_T = 16;
// LPP = C / 8 lanes share a pixel (8 channels each), so a wave's 16 B stores / residual loads cover whole
// 128 B (C = 64) or 64 B (C = 32) pixel rows; weights in LDS as [tap][C] (two 16 B reads per tap).
// FWD: the same stencil as the FORWARD of a 1 -> C conv (the discriminator's features.0, rfb_esrgan.py:28: 1 -> 64,
// 3x3, no bias, LeakyReLU): out[q][c] = act(sum W[c][0][ky][kx] * x[q + (ky,kx) - pad] + bias[c]), act 1 / 2 =
// leaky relu / relu forward.  The implicit-GEMM path pads the single input channel to 8 (K = 72 of 96) and is
// bound by its LDS-staged epilogue (156 us per B=32 256^2 launch for a 268 MB output).
template <int KS, int LPP, bool FWD = false>
__global__ __launch_bounds__(256) void dgrad_ci1_kernel(int n, int h, int w, int pad, const uint16_t* __restrict__ dz, int dz_cs,
                                                        int dz_co, const float* __restrict__ wt, int act, float slope,
                                                        const uint16_t* __restrict__ res1, int r1_cs, int r1_co, uint16_t* __restrict__ out,
                                                        int out_cs, int out_co, const float* __restrict__ bias = nullptr) {
  constexpr int TP = S1_T + KS - 1, C = LPP * 8, PPS = 256 / LPP, NPASS = S1_T * S1_T / PPS;
  __shared__ float dzt[TP * TP];
  __shared__ __attribute__((aligned(16))) float wl[KS * KS * C];
  const int tid = threadIdx.x, cg = tid % LPP, ps = tid / LPP;
  const int tiles_x = (w + S1_T - 1) / S1_T, tiles_y = (h + S1_T - 1) / S1_T;
  int b = blockIdx.x;
  const int bx = b % tiles_x;
  b /= tiles_x;
  const int by = b % tiles_y, img = b / tiles_y;
  const int x0 = bx * S1_T, y0 = by * S1_T;
  // tile row r <-> dz row y0 - (KS - 1) + pad + r (same for columns); forward: x row y0 - pad + r
  const int ry0 = FWD ? y0 - pad : y0 - (KS - 1) + pad, rx0 = FWD ? x0 - pad : x0 - (KS - 1) + pad;
  // every residual load of this thread first (they land while the tile is staged and the sums computed)
  uint4 rv[NPASS];
#pragma unroll
  for (int k = 0; k < NPASS; ++k) {
    const int pix = k * PPS + ps, qy = y0 + pix / S1_T, qx = x0 + pix % S1_T;
    const bool ok = !FWD && act && qy < h && qx < w;
    rv[k] = ok ? *(const uint4*)(res1 + (((long)img * h + qy) * w + qx) * r1_cs + r1_co + cg * 8) : make_uint4(0, 0, 0, 0);
  }
  for (int i = tid; i < TP * TP; i += 256) {
    const int r = i / TP, c = i - r * TP;
    const int yy = ry0 + r, xx = rx0 + c;
    dzt[i] = (yy >= 0 && yy < h && xx >= 0 && xx < w) ? bf2f(dz[(((long)img * h + yy) * w + xx) * dz_cs + dz_co]) : 0.f;
  }
  for (int i = tid; i < C * KS * KS; i += 256) {  // OIHW [c][tap] -> [tap][c]
    const int c = i / (KS * KS), t = i - c * (KS * KS);
    wl[t * C + c] = wt[i];
  }
  __syncthreads();
  // 3x3: this thread's 8 channels x 9 taps of weights held in registers across the passes (72 VGPRs); 5x5 re-reads LDS
  constexpr bool WREG = KS == 3;
  float4 wr0[WREG ? KS * KS : 1], wr1[WREG ? KS * KS : 1];
  if constexpr (WREG) {
#pragma unroll
    for (int t = 0; t < KS * KS; ++t) {
      wr0[t] = *(const float4*)(wl + t * C + cg * 8);
      wr1[t] = *(const float4*)(wl + t * C + cg * 8 + 4);
    }
  }
#pragma unroll
  for (int k = 0; k < NPASS; ++k) {
    const int pix = k * PPS + ps, ty = pix / S1_T, tx = pix % S1_T;
    const int qy = y0 + ty, qx = x0 + tx;
    float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ky = 0; ky < KS; ++ky)
#pragma unroll
      for (int kx = 0; kx < KS; ++kx) {  // out[q] += W[c][ky][kx] * dz[q - (ky, kx) + pad]  (FWD: x[q + (ky, kx) - pad])
        const float d = FWD ? dzt[(ty + ky) * TP + tx + kx] : dzt[(ty + KS - 1 - ky) * TP + tx + KS - 1 - kx];
        const int t = ky * KS + kx;
        const float4 w0 = WREG ? wr0[WREG ? t : 0] : *(const float4*)(wl + t * C + cg * 8);
        const float4 w1 = WREG ? wr1[WREG ? t : 0] : *(const float4*)(wl + t * C + cg * 8 + 4);
        v[0] += w0.x * d; v[1] += w0.y * d; v[2] += w0.z * d; v[3] += w0.w * d;
        v[4] += w1.x * d; v[5] += w1.y * d; v[6] += w1.z * d; v[7] += w1.w * d;
      }
    if (qy >= h || qx >= w) continue;
    if (FWD) {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        if (bias) v[i] += bias[cg * 8 + i];
        v[i] = act_apply(v[i], act, slope);
      }
    } else if (act) {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const uint32_t wd = i < 2 ? rv[k].x : i < 4 ? rv[k].y : i < 6 ? rv[k].z : rv[k].w;
        const float r = bf2f((uint16_t)((i & 1) ? (wd >> 16) : wd));
        v[i] = r > 0.f ? v[i] : (act == 3 ? v[i] * slope : 0.f);
      }
    }
    *(uint4*)(out + (((long)img * h + qy) * w + qx) * out_cs + out_co + cg * 8) = pack8_bf16(v, 1.f);
  }
}

// the shape the data gradient takes (the operands are checked by the entry point), else the error set
static bool dgrad_ci1_shape(int ks, int pad, int c, int act) {
  if ((ks != 3 && ks != 5) || pad != ks / 2 || c <= 0 || c > 64 || c % 8 || (act != 0 && act != 3 && act != 4)) {
    set_error("dgrad_single_output: unsupported arguments (ks %d pad %d c %d act %d)", ks, pad, c, act);
    return false;
  }
  return true;
}

extern "C" const char* climsr_dgrad_single_output_kernel(int ks, int c, int act) {
  static thread_local char name[96];
  name[0] = 0;
  if (dgrad_ci1_shape(ks, ks / 2, c, act)) snprintf(name, sizeof(name), "dgrad_ci1_kernel<%d, %d>", ks, c / 8);
  return name;
}

extern "C" int climsr_dgrad_single_output(int n, int h, int w, int ks, int pad, const uint16_t* dz, int dz_cstride, int dz_coff,
                                          const float* weight, int c, int act, float slope, const uint16_t* res1, int res1_cstride,
                                          int res1_coff, uint16_t* out, int out_cstride, int out_coff, void* stream) {
  if (!dz || !weight || !out || n <= 0 || h <= 0 || w <= 0 || (out_cstride | out_coff) % 8 ||
      (act && (!res1 || (res1_cstride | res1_coff) % 8))) {
    set_error("dgrad_single_output: unsupported arguments (ks %d pad %d c %d act %d)", ks, pad, c, act);
    return CLIMSR_EINVAL;
  }
  if (!dgrad_ci1_shape(ks, pad, c, act)) return CLIMSR_EINVAL;
  const long tiles = (long)n * ((h + S1_T - 1) / S1_T) * ((w + S1_T - 1) / S1_T);
#define CLIMSR_CI1(KS_, LPP_)                                                                                              \
  hipLaunchKernelGGL((dgrad_ci1_kernel<KS_, LPP_>), dim3((unsigned)tiles), dim3(256), 0, (hipStream_t)stream, n, h, w, pad, dz, \
                     dz_cstride, dz_coff, weight, act, slope, res1, res1_cstride, res1_coff, out, out_cstride, out_coff)
  switch (ks * 100 + c / 8) {
    case 308: CLIMSR_CI1(3, 8); break;
    case 304: CLIMSR_CI1(3, 4); break;
    case 508: CLIMSR_CI1(5, 8); break;
    case 504: CLIMSR_CI1(5, 4); break;
    default: set_error("dgrad_single_output: no instance for ks %d, %d channels (32 or 64)", ks, c); return CLIMSR_EINVAL;
  }
#undef CLIMSR_CI1
  return check_launch("dgrad_single_output");
}

extern "C" int climsr_conv_single_input(int n, int h, int w, int ks, int pad, const uint16_t* x, int x_cstride, int x_coff,
                                        const float* weight, const float* bias, int c, int act, float slope, uint16_t* out,
                                        int out_cstride, int out_coff, void* stream) {
  if (!x || !weight || !out || n <= 0 || h <= 0 || w <= 0 || (ks != 3 && ks != 5) || pad != ks / 2 || c % 8 || (c != 32 && c != 64) ||
      (out_cstride | out_coff) % 8 || act < 0 || act > 2) {
    set_error("conv_single_input: unsupported arguments (ks %d pad %d c %d act %d)", ks, pad, c, act);
    return CLIMSR_EINVAL;
  }
  const long tiles = (long)n * ((h + S1_T - 1) / S1_T) * ((w + S1_T - 1) / S1_T);
#define CLIMSR_CI1F(KS_, LPP_)                                                                                                   \
  hipLaunchKernelGGL((dgrad_ci1_kernel<KS_, LPP_, true>), dim3((unsigned)tiles), dim3(256), 0, (hipStream_t)stream, n, h, w, pad, x, \
                     x_cstride, x_coff, weight, act, slope, nullptr, 0, 0, out, out_cstride, out_coff, bias)
  switch (ks * 100 + c / 8) {
    case 308: CLIMSR_CI1F(3, 8); break;
    case 304: CLIMSR_CI1F(3, 4); break;
    case 508: CLIMSR_CI1F(5, 8); break;
    default: CLIMSR_CI1F(5, 4); break;
  }
#undef CLIMSR_CI1F
  return check_launch("conv_single_input");
}
