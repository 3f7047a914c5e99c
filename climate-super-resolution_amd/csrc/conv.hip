// Implicit-GEMM convolution for CDNA4 (gfx950): forward / data-gradient and weight-gradient.
//
// Replaces nn.Conv2d (+ fused F.interpolate(nearest), LeakyReLU/ReLU, residual adds) on the
// ESRGAN hot path: climsr/models/esrgan.py:17-102, srcnn.py:6-18, rfb_esrgan.py:26-61.
//
// Layout: activations NHWC bf16; a conv reads channels [in_coff, in_coff+in_c) of a buffer with
// in_cstride channels per pixel (the RDB dense concatenation is one 128-channel buffer, so
// torch.cat is free).  GEMM view: M = output channels (MFMA A = packed weights), N = output pixels
// (MFMA B = input pixels staged in LDS, im2col done by LDS addressing), K = taps x channels.
// MFMA: v_mfma_f32_16x16x32_bf16.  Lane l: A[row l&15][k 8(l>>4)+j], B[k 8(l>>4)+j][col l&15],
// C[row 4(l>>4)+i][col l&15].
#include <algorithm>
#include <atomic>
#include <mutex>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>

#include "common.h"
#include "conv_ep.h"
#include "conv_route.h"

namespace climsr {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("%s: %s", what, hipGetErrorString(e));
    return CLIMSR_EHIP;
  }
  return CLIMSR_OK;
}

// Per-device launch facts, shared by every dispatcher (one process may drive several devices from several threads):
// the CU count of the CURRENT device and the dynamic-LDS opt-in of a kernel on it, each settled once per device
// under a mutex; readers of a settled entry take no lock.
static constexpr int MAX_DEV = 64;
static std::mutex g_rt_mu;
static std::atomic<int> g_ncu[MAX_DEV];

static int current_device() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAX_DEV) dev = 0;
  return dev;
}

int device_cus() {
  const int dev = current_device();
  int n = g_ncu[dev].load(std::memory_order_acquire);
  if (n > 0) return n;
  std::lock_guard<std::mutex> lk(g_rt_mu);
  n = 0;
  if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
  g_ncu[dev].store(n, std::memory_order_release);
  return n;
}

int lds_opt_in(const void* fn, int bytes) {
  struct Key {
    const void* fn;
    int dev;
  };
  static Key done[1024];
  static std::atomic<int> ndone{0};
  const int dev = current_device();
  const int seen = ndone.load(std::memory_order_acquire);
  for (int i = 0; i < seen; ++i)
    if (done[i].fn == fn && done[i].dev == dev) return CLIMSR_OK;
  std::lock_guard<std::mutex> lk(g_rt_mu);
  const int m = ndone.load(std::memory_order_relaxed);
  for (int i = 0; i < m; ++i)
    if (done[i].fn == fn && done[i].dev == dev) return CLIMSR_OK;
  const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e != hipSuccess) {
    set_error("hipFuncSetAttribute(MaxDynamicSharedMemorySize=%d): %s", bytes, hipGetErrorString(e));
    return CLIMSR_EHIP;
  }
  if (m < 1024) {
    done[m] = Key{fn, dev};
    ndone.store(m + 1, std::memory_order_release);
  }
  return CLIMSR_OK;
}

// ------------------------------------------------------------------------------------------
// Tiling constants
// ------------------------------------------------------------------------------------------
// LDS pitches of the staged operand tiles.  A 16 x 32-channel MFMA fragment is read with ds_read_b128 (lane
// 16g + col: row col, channels 8g..8g+7); its four 16-lane bank groups are conflict-free when the row pitch
// is 16 (mod 32) bf16 elements, and 2-way conflicted at 8 (mod 32) (measured SQ_LDS_BANK_CONFLICT 43 % of
// the LDS cycles of conv5 with the old +8 pads).
static inline int xpitch(int cc) { return cc + ((16 - cc % 32) + 32) % 32; }  // >= cc, == 16 (mod 32)
// Stride 2: a fragment's 16 pixels sit 2 pixels apart in the tile, so the lane pitch is 2 * ccp and ccp == 8 (mod 16)
// keeps it at 16 (mod 32) (the stride-1 pitch left every stride-2 read 4-way conflicted: SQ_LDS_BANK_CONFLICT 35 %).
static inline int xpitch_s2(int cc) { return cc + ((8 - cc % 16) + 16) % 16; }
constexpr int FWD_LDS_BUDGET = 80 * 1024;  // two workgroups per CU

static int fwd_nt(int out_c) {
  int nt = (out_c + 15) / 16;
  return nt > 4 ? 4 : (nt == 3 ? 4 : nt);
}

__device__ inline int climsr_rows_dev(int out_c) {
  int nt = (out_c + 15) / 16;
  nt = nt > 4 ? 4 : (nt == 3 ? 4 : nt);
  return (out_c + nt * 16 - 1) / (nt * 16) * (nt * 16);
}

static void fwd_geom(int in_c, int ks, int stride, int out_c, int cc, int mw, FwdGeom* g) {
  g->mw = mw;
  g->th = 4 * mw;
  g->tph = (g->th - 1) * stride + ks;
  g->tpw = (TW - 1) * stride + ks;
  g->ccp = stride == 2 ? xpitch_s2(cc) : xpitch(cc);
  g->kc = ks * ks * cc;
  g->kcpad = round_up(g->kc, 32);
  g->nchunk = ceil_div(in_c, cc);
  g->kpk = g->nchunk * g->kcpad;
  g->nt = fwd_nt(out_c);
  g->lds_tab = (size_t)(g->kcpad / 8) * 4;
  g->lds_tab = (g->lds_tab + 15) / 16 * 16;
  g->lds_x = (size_t)g->tph * g->tpw * g->ccp * 2;
  g->lds_w = (size_t)g->nt * 16 * (g->kcpad + WPAD) * 2;
  g->lds_total = g->lds_tab + g->lds_x + g->lds_w;
}

}  // namespace climsr

using namespace climsr;

extern "C" const char* climsr_last_error(void) { return g_err; }
extern "C" int climsr_version(void) { return 2; }

// Convs with <= 16 outputs, 3x3 and <= 128 inputs (the residual dense block's conv1-4 and their pull data
// gradients) run on conv_n16_kernel, whose packed K is tap-major with the channels padded to 32 per tap.
static bool n16_shape(int in_c, int ks, int out_c) { return out_c <= 16 && ks == 3 && in_c <= 128; }

static bool pw_fits(int in_c, int ks, int out_c);

extern "C" int climsr_conv_chunk_ex(int in_c, int ks, int out_c, int stride) {
  // <= 4 real input channels (conv_first, srcnn.conv1, VGG conv1_1, RCAN head): taps packed 4 channels apart
  // (conv_pw GEO 2) -- K = ks^2 * 4 instead of ks^2 * 8 (9x9: 11 k-steps instead of 21)
  if (in_c == 4 && stride == 1 && out_c == 64 && (ks == 3 || ks == 9)) return 4;
  if (stride == 1 && n16_shape(in_c, ks, out_c))  // conv_n16: one chunk, padded to 32/64/128
    return in_c <= 32 ? 32 : (in_c <= 64 ? 64 : 128);
  if (stride == 1 && pw_fits(in_c, ks, out_c)) return round_up(in_c, 8);  // conv_pw: the whole K in one chunk
  int cc = round_up(in_c, 8);
  FwdGeom g;
  while (cc > 8) {
    fwd_geom(in_c, ks, 1, out_c, cc, 4, &g);
    if (g.lds_total <= (size_t)FWD_LDS_BUDGET) break;
    cc = round_up((cc + 1) / 2, 8);
  }
  return cc;
}

extern "C" int climsr_conv_chunk(int in_c, int ks, int out_c) { return climsr_conv_chunk_ex(in_c, ks, out_c, 1); }

extern "C" int climsr_conv_packed_k(int in_c, int ks, int cc) {
  return ceil_div(in_c, cc) * round_up(ks * ks * cc, 32);
}

extern "C" int climsr_conv_packed_rows(int out_c) {
  int nt = fwd_nt(out_c);
  return round_up(out_c, nt * 16);
}

// ------------------------------------------------------------------------------------------
// Weight packing: fp32 OIHW -> bf16 [co_pad16][nchunk][kcpad], k' = tap*cc + c (zeros elsewhere)
// ------------------------------------------------------------------------------------------
__global__ void pack_kernel(const float* __restrict__ w, int rows, int kpk, int in_c_real, int out_c_real, int ks, int cc,
                            int kcpad, int tflip, uint16_t* __restrict__ out) {
  long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long total = (long)rows * kpk;
  if (idx >= total) return;
  int co = (int)(idx / kpk);
  int kk = (int)(idx % kpk);
  int j = kk / kcpad;
  int kr = kk % kcpad;
  int tap = kr / cc;
  int c = j * cc + kr % cc;
  float v = 0.f;
  int kk2 = ks * ks;
  if (co < out_c_real && tap < kk2 && c < in_c_real) {
    int ky = tap / ks, kx = tap % ks;
    if (!tflip) {
      v = w[(((long)co * in_c_real + c) * ks + ky) * ks + kx];
    } else {  // src W[c][co][ks-1-ky][ks-1-kx] with src dims [in_c_real][out_c_real]
      v = w[(((long)c * out_c_real + co) * ks + (ks - 1 - ky)) * ks + (ks - 1 - kx)];
    }
  }
  out[idx] = f2bf(v);
}

extern "C" int climsr_pack_conv_weight(const float* w, int out_c, int in_c, int in_c_real, int out_c_real, int ks, int cc,
                                       int transpose_flip, uint16_t* wpk, void* stream) {
  if (!w || !wpk || (in_c % 8 && !(in_c == 4 && cc == 4)) || (cc % 8 && cc != 4) || cc <= 0 || ks <= 0) {
    set_error("pack_conv_weight: bad args (in_c=%d cc=%d ks=%d)", in_c, cc, ks);
    return CLIMSR_EINVAL;
  }
  int rows = climsr_conv_packed_rows(out_c);
  int kcpad = round_up(ks * ks * cc, 32);
  int kpk = climsr_conv_packed_k(in_c, ks, cc);
  long total = (long)rows * kpk;
  hipLaunchKernelGGL(pack_kernel, dim3(ceil_div(total, 256)), dim3(256), 0, (hipStream_t)stream, w, rows, kpk, in_c_real,
                     out_c_real, ks, cc, kcpad, transpose_flip, wpk);
  return check_launch("pack_conv_weight");
}

// Batched form: one launch packs every conv of a network (blockIdx.y = descriptor).  Each thread writes 8
// consecutive packed elements (one 16 B store; cc and kcpad are multiples of 8, so the 8 share the chunk and
// the tap) with 32-bit index math (a packed matrix is < 2^31 elements).
__device__ __forceinline__ uint4 pack8(const float (&v)[8]) {
  uint4 o;
  o.x = (uint32_t)f2bf(v[0]) | ((uint32_t)f2bf(v[1]) << 16);
  o.y = (uint32_t)f2bf(v[2]) | ((uint32_t)f2bf(v[3]) << 16);
  o.z = (uint32_t)f2bf(v[4]) | ((uint32_t)f2bf(v[5]) << 16);
  o.w = (uint32_t)f2bf(v[6]) | ((uint32_t)f2bf(v[7]) << 16);
  return o;
}
__global__ void pack_batched_kernel(const ClimsrPackDesc* __restrict__ descs) {
  const ClimsrPackDesc d = descs[blockIdx.y];
  const int rows = climsr_rows_dev(d.out_c);
  const int kcpad = (d.ks * d.ks * d.cc + 31) / 32 * 32;
  const int kpk = (d.in_c + d.cc - 1) / d.cc * kcpad;
  const int total8 = rows * kpk / 8, kpk8 = kpk / 8, kc8 = kcpad / 8;
  const int kk2 = d.ks * d.ks;
  for (int i8 = blockIdx.x * blockDim.x + threadIdx.x; i8 < total8; i8 += gridDim.x * blockDim.x) {
    const int co = i8 / kpk8, kk8 = i8 - co * kpk8;
    const int j = kk8 / kc8, kr = (kk8 - j * kc8) * 8;
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {  // (cc = 4: the 8 elements span two taps)
      const int tap = (kr + e) / d.cc, c = j * d.cc + (kr + e) - tap * d.cc;
      const bool ok = co < d.out_c_real && tap < kk2;
      const int ky = tap / d.ks, kx = tap - (tap / d.ks) * d.ks;
      v[e] = 0.f;
      if (ok && c < d.in_c_real) {
        if (!d.tflip) v[e] = d.w[((co * d.in_c_real + c) * d.ks + ky) * d.ks + kx];
        else v[e] = d.w[((c * d.out_c_real + co) * d.ks + (d.ks - 1 - ky)) * d.ks + (d.ks - 1 - kx)];
      }
    }
    *(uint4*)(d.out + (long)i8 * 8) = pack8(v);
  }
}

extern "C" int climsr_pack_conv_weights_batched(const ClimsrPackDesc* descs, int ndesc, int64_t max_elems, void* stream) {
  if (!descs || ndesc <= 0 || ndesc > 65535) {
    set_error("pack_conv_weights_batched: bad args");
    return CLIMSR_EINVAL;
  }
  int gx = ceil_div(max_elems / 8, 256);
  if (gx > 64) gx = 64;
  if (gx < 1) gx = 1;
  hipLaunchKernelGGL(pack_batched_kernel, dim3(gx, ndesc), dim3(256), 0, (hipStream_t)stream, descs);
  return check_launch("pack_conv_weights_batched");
}

// Pull data-gradient weights of a residual dense block (see climsr_hip.h), all the pull convs of a network in
// one launch, row-per-workgroup (blockIdx.x strides over the packed rows co, blockIdx.y = descriptor): the
// row's source weights W_s[c][ci_off + co][.][.] are 9 contiguous floats per input channel c, read in
// those runs into an LDS [tap][channel] image (tap flipped), then the packed row is written as coalesced
// 16 B vectors.  (An element-per-thread gather of 8 floats 36*seg_ic bytes apart per output vector took
// 128 us per step for the generator's 165 pull convs.)
constexpr int PULL_ROW_MAX = 4096;  // in_c * ks^2 floats staged per row
__global__ __launch_bounds__(256) void pack_pull_row_kernel(const ClimsrPullPackDesc* __restrict__ descs) {
  __shared__ float img[PULL_ROW_MAX];
  // the segment arrays are indexed dynamically: read them from the descriptor in global memory (a private
  // copy of the struct would live in scratch)
  const ClimsrPullPackDesc* dp = descs + blockIdx.y;
  const ClimsrPullPackDesc d = *dp;
  const int rows = climsr_rows_dev(d.out_c);
  const int kk2 = d.ks * d.ks;
  const int kcpad = (kk2 * d.cc + 31) / 32 * 32;
  const int kpk = (d.in_c + d.cc - 1) / d.cc * kcpad;
  const int kc8 = kcpad / 8;
  const bool staged = d.in_c * kk2 <= PULL_ROW_MAX;
  // source of (channel cabs, source tap t) of row co, 0 past the segments
  auto src_at = [&](int co, int cabs, int t) -> float {
    int c = cabs, s = 0;
    while (s < d.nseg - 1 && c >= dp->seg_oc[s]) c -= dp->seg_oc[s++];
    return c < dp->seg_oc[s] ? dp->seg_w[s][((long)c * dp->seg_ic[s] + d.ci_off + co) * kk2 + t] : 0.f;
  };
  for (int co = blockIdx.x; co < rows; co += gridDim.x) {
    if (staged) {
      __syncthreads();  // the previous row's reads of img are done
      if (co < d.out_c)
        for (int e = threadIdx.x; e < d.in_c * kk2; e += blockDim.x) {
          const int cabs = e / kk2, t = e - cabs * kk2;
          img[(kk2 - 1 - t) * d.in_c + cabs] = src_at(co, cabs, t);  // (ks-1-ky, ks-1-kx) = tap kk2-1-t
        }
      __syncthreads();
    }
    uint16_t* out = d.out + (long)co * kpk;
    for (int i8 = threadIdx.x; i8 < kpk / 8; i8 += blockDim.x) {
      const int j = i8 / kc8, kr = (i8 - j * kc8) * 8;
      const int tap = kr / d.cc, cabs = j * d.cc + kr - tap * d.cc;
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const bool ok = co < d.out_c && tap < kk2 && cabs + e < d.in_c;
        v[e] = !ok ? 0.f : staged ? img[tap * d.in_c + cabs + e] : src_at(co, cabs + e, kk2 - 1 - tap);
      }
      *(uint4*)(out + i8 * 8) = pack8(v);
    }
  }
}

extern "C" int climsr_pack_pull_weights_batched(const ClimsrPullPackDesc* descs, int ndesc, int64_t max_elems, void* stream) {
  if (!descs || ndesc <= 0 || ndesc > 65535) {
    set_error("pack_pull_weights_batched: bad args");
    return CLIMSR_EINVAL;
  }
  (void)max_elems;
  // rows per descriptor are on the device: 64 row slots (the RDB pulls have 16 or 64 rows), more rows loop
  hipLaunchKernelGGL(pack_pull_row_kernel, dim3(64, ndesc), dim3(256), 0, (hipStream_t)stream, descs);
  return check_launch("pack_pull_weights_batched");
}

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
constexpr int N16_TH = 8;
constexpr int N16_TPH = N16_TH + 2, N16_TPW = TW + 2;

static int n16_ncb(int in_c) { return in_c <= 32 ? 1 : (in_c <= 64 ? 2 : 4); }

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

static bool co1m_shape(const ClimsrConvDesc* d) {
  return d->out_c == 1 && d->stride == 1 && d->up == 1 && (d->ks == 3 || d->ks == 5 || d->ks == 9) && d->pad == d->ks / 2 &&
         d->in_c <= 64 && d->in_c % 8 == 0 && d->cc % 8 == 0 && d->out_h == d->in_h && d->out_w == d->in_w;
}

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

// Geometry of the weights-resident persistent conv (conv_pw.hip)
constexpr int PW_PV = 12;  // prefetched 16 B input vectors per thread (tile <= 3072 vectors)

static bool pw_geom(const ClimsrConvDesc* d, int nt, int mw, PwGeom* g, int nw = 4) {
  if (d->stride != 1 || d->cc < d->in_c) return false;
  g->mw = mw;
  g->tph = nw * mw + d->ks - 1;
  g->tpw = TW + d->ks - 1;
  const int ccs = d->cc < 8 ? 8 : d->cc;  // staged channels per pixel (cc 4: 16 B loads, 4 of 8 channels used)
  g->ccp = xpitch(ccs);
  g->kcpad = round_up(d->ks * d->ks * d->cc, 32);
  g->nvx = g->tph * g->tpw * (ccs / 8);
  g->lds_tab = ((size_t)(g->kcpad / (d->cc < 8 ? 4 : 8)) * 4 + 15) / 16 * 16;
  g->lds_w = (size_t)nt * 16 * (g->kcpad + WPAD) * 2;
  g->lds_x = (size_t)g->tph * g->tpw * g->ccp * 2;
  g->lds_ep = (size_t)nw * mw * 16 * (nt * 16 + 4) * 4;
  g->lds_total = g->lds_tab + g->lds_w + (g->lds_x > g->lds_ep ? g->lds_x : g->lds_ep);
  return g->nvx <= 64 * nw * PW_PV && g->lds_total <= 160 * 1024;
}

static bool pw_fits(int in_c, int ks, int out_c) {
  const int nt = fwd_nt(out_c);
  if (out_c <= 16 || out_c > 64 || (nt != 2 && nt != 4)) return false;
  ClimsrConvDesc d{};
  d.in_c = round_up(in_c, 8);
  d.cc = d.in_c;
  d.ks = ks;
  d.stride = 1;
  PwGeom g;
  return pw_geom(&d, nt, 2, &g, 4);
}

// ------------------------------------------------------------------------------------------
// 1x1 conv as a streaming GEMM (srcnn.conv2 64->32 and its 32->64 data gradient with the ReLU mask):
// out[p][co] = epilogue(sum_ci x[p][ci] w[co][ci]).  Nothing is reused across pixels except the weights, so
// nothing goes through LDS: the weight fragments sit in VGPRs, each lane loads its 16 B channel slice of a
// pixel straight into the B fragment (16 pixels x 32 channels per load round), U groups of 16 pixels are in
// flight per wave, and the fused epilogue stores 4 consecutive channels per lane.  HBM-bound by design.
// ------------------------------------------------------------------------------------------
constexpr int PT_U = 4;  // 16-pixel groups per wave iteration

static bool pt_shape(const ClimsrConvDesc* d, const ClimsrEpilogue* ep) {
  return d->ks == 1 && d->stride == 1 && d->up == 1 && d->pad == 0 && !ep->down2 && d->in_c % 32 == 0 && d->in_c <= 128 &&
         d->cc == d->in_c && d->out_c % 16 == 0 && d->out_c <= 64 && d->out_h == d->in_h && d->out_w == d->in_w &&
         ((d->out_cstride | d->out_coff) & 3) == 0 && (!ep->res1 || ((ep->res1_cstride | ep->res1_coff) & 3) == 0) &&
         (!ep->res2 || ((ep->res2_cstride | ep->res2_coff) & 3) == 0);
}

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

static int launch_co1(const FwdArgs& a, hipStream_t s) {
  size_t lds = (size_t)(15 + a.ks) * (15 + a.ks) * (CO1_CC + 8) * 2 + (size_t)a.ks * a.ks * CO1_CC * 2;
  hipLaunchKernelGGL(conv_co1_kernel, dim3(a.tiles_x * a.tiles_y * a.n), dim3(256), lds, s, a);
  return check_launch("conv2d_fwd (co1)");
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
static int launch_dgrad_s2(const FwdRoute& r, const FwdArgs& a, hipStream_t s) {
  if (r.mw == 2) return launch_dgrad_s2_t<2, 4>(r, a, s);
  return launch_dgrad_s2_t<4, 2>(r, a, s);
}

// Epilogue specialisations without residuals (store_tile_lds EP 3 / 6 / 7 / 8), or 0: activation forward with
// (3) / without (6) bias, plain fp32 '=' output (7), plain bf16 output (8).  Needs 8-channel-aligned slices.
static int plain_ep(const ClimsrConvDesc* d, bool bias, const ClimsrEpilogue* ep) {
  if ((d->out_c & 7) || ((d->out_cstride | d->out_coff) & 7) || ep->down2 || ep->res1 || ep->res2 || ep->aux || ep->res_f32) return 0;
  if (ep->out_mode == 0 && (ep->act == 1 || ep->act == 2)) return bias ? 3 : 6;
  if (ep->act == 0 && !bias) return ep->out_mode == 1 ? 7 : ep->out_mode == 0 ? 8 : 0;
  return 0;
}

static bool fwd_s2_shape(const ClimsrConvDesc* d, bool bias, const ClimsrEpilogue* ep, const FwdGeom& g) {
  return d->stride == 2 && d->ks == 3 && d->pad == 1 && d->up == 1 && d->cc == 32 && d->in_c % 32 == 0 && d->out_c % 64 == 0 &&
         d->in_coff % 8 == 0 && d->in_cstride % 8 == 0 && g.kcpad == 288 && plain_ep(d, bias, ep) == 8 &&
         (long)d->n * d->in_h * d->in_w * d->in_cstride * 2 < (1L << 31);  // the kernel's int / 32-bit input offsets
}

static bool dgrad_s2_shape(const ClimsrConvDesc* d, bool bias, const ClimsrEpilogue* ep) {
  const bool act_ok = ep->act == 0 ? !ep->res1 : ((ep->act == 3 || ep->act == 4) && ep->res1 && !(ep->res_f32 & 1) &&
                                                   ((ep->res1_cstride | ep->res1_coff) & 7) == 0);
  return d->up == -2 && d->stride == 1 && d->ks == 3 && d->pad == 1 && d->cc == 32 && d->in_c % 32 == 0 && d->out_c % 32 == 0 &&
         d->in_coff % 8 == 0 && d->in_cstride % 8 == 0 && ((d->out_cstride | d->out_coff) & 7) == 0 && d->out_h == 2 * d->in_h &&
         d->out_w == 2 * d->in_w && ep->out_mode == 0 && !bias && !ep->res2 && !ep->aux && !ep->down2 && act_ok;
}

// channel blocks grouped per tile in the XCD-major order: the largest divisor of ncob (>= 2) whose weight blocks
// together stay within ~2.5 MB of the XCD's 4 MB L2 (they are re-read by every tile of the group), else 0
static int conv_xcd_group(int ncob, long wblk_bytes) {
  if (ncob < 2) return 0;
  for (int gsz = ncob; gsz >= 2; --gsz)
    if (ncob % gsz == 0 && gsz * wblk_bytes <= (5L << 19)) return gsz;
  return 0;
}

// ------------------------------------------------------------------------------------------
// The route
// ------------------------------------------------------------------------------------------
enum { PICK_OK = 0, PICK_CC4, PICK_LDS };  // fwd_pick: a kernel, or why the generic kernel cannot take the conv

// the weights-resident persistent kernel for one-chunk convs with 17..64 outputs (large-pixel-count layers)
static bool pick_pw(const ClimsrConvDesc* d, bool bias, const ClimsrEpilogue* ep, bool cc4, FwdRoute* r) {
  const int nt = fwd_nt(d->out_c);
  const long npx = (long)d->n * d->out_h * d->out_w;
  if (!(r->ncob == 1 && (nt == 4 || nt == 2) && d->up != -2 && (npx >= 4096 || cc4) &&
        (long)d->n * d->in_h * d->in_w * d->in_cstride * 2 < (1L << 31)))  // 32-bit buffer offsets
    return false;
  const bool al8 = (d->out_c & 7) == 0 && ((d->out_cstride | d->out_coff) & 7) == 0, r1 = ep->res1 != nullptr;
  const bool r1al8 = ((ep->res1_cstride | ep->res1_coff) & 7) == 0, bwd = ep->act == 3 || ep->act == 4;
  r->mw = 2; r->nt = nt;
  // 8 waves x 2 rows (two waves per SIMD) when the LDS allows, else 4 waves x 2 rows
  if (pw_geom(d, nt, 2, &r->pg, 8) && r->pg.nvx <= 512 * 7 && (d->out_h >= 16 || cc4)) {
    // epilogue specialisations (store_tile_lds EP 3 / 4): activation forward / activation backward; 5: + down2
    const bool v8 = al8 && !ep->down2 && !ep->res2 && !ep->aux && ep->out_mode == 0 && ep->res_f32 == 0;
    const bool d2 = ep->down2 && d->out_c == 64 && ((d->out_cstride | d->out_coff) & 3) == 0 && !bias && r1 && ep->res_f32 == 0 &&
                    ((ep->res1_cstride | ep->res1_coff) & 3) == 0 && bwd && !ep->res2 && !ep->aux && ep->out_mode == 0;
    r->ep = (v8 && bias && !r1 && (ep->act == 1 || ep->act == 2)) ? 3 : (v8 && !bias && r1 && r1al8 && bwd) ? 4 : d2 ? 5 : 0;
    const int plain = plain_ep(d, bias, ep);
    if (nt == 4 && r->ep == 0 && plain >= 6) r->ep = plain;  // 6 / 7 / 8
    r->nw = 8; r->pv = 7;
  } else if (pw_geom(d, nt, 2, &r->pg, 4)) {
    r->ep = 0; r->nw = 4; r->pv = 12;
  } else {
    return false;
  }
  r->family = FAM_PW;
  // 4-channel taps are staged as 8-channel pixels, one 16 B vector per pixel: the 24 x 24 (9x9) / 18 x 18 (3x3) input
  // tile is <= 2 vectors per thread, and the staging loops run PV iterations of address math whether or not their
  // vectors exist
  if (d->cc == 4) {
    r->geo = 2;
    if (r->pg.nvx <= 2 * 64 * r->nw) r->pv = 2;
  } else if (r->nw * r->mw == 16 && d->ks == 3 && d->cc == 64 && r->pg.kcpad == 9 * 64 && r->pg.ccp == 80 && r->pg.tpw == TW + 2 &&
             r->pg.tph == 18) {
    r->geo = 1;
  }
  r->tiles_y = ceil_div(d->out_h, r->nw * r->mw);
  return true;
}

// the generic kernel: tile shape and prefetch depth, epilogue, GEO form, and the LDS-DMA kernel where that takes over
static void pick_generic(const ClimsrConvDesc* d, bool bias, const ClimsrEpilogue* ep, bool bz, FwdRoute* r) {
  const FwdGeom& g = r->g;
  const bool r1 = ep->res1 != nullptr, r2 = ep->res2 != nullptr, aux = ep->aux != nullptr, bwd = ep->act == 3 || ep->act == 4;
  const bool al8 = (d->out_c & 7) == 0 && ((d->out_cstride | d->out_coff) & 7) == 0;
  const bool r1al8 = ((ep->res1_cstride | ep->res1_coff) & 7) == 0;
  const int plain = plain_ep(d, bias, ep);
  r->family = FAM_FWD; r->mw = g.mw; r->nt = g.nt;
  // (a stride-2 data gradient that only dgrad_s2's operand-size test turned away is still promised its partial rows)
  r->parts = bz && d->up == -2 && plain == 8 && dgrad_s2_shape(d, bias, ep);
  if (g.mw == 4) {
    const int nrx = ceil_div(g.tph * g.tpw * (d->cc / 8), 256), nrw = ceil_div(g.nt * 16 * (g.kcpad / 8), 256);
    r->nt = 4;
    if (g.nchunk > 1 && nrx <= 6 && nrw <= 9) {
      // multi-chunk tiles whose per-thread staging fits 6 input + 9 weight vectors: chunk-pipelined variant
      r->pfx = 6; r->pfw = 9;
      // epilogue specialisations (store_tile_lds EP): residual forward (conv5, trunk_conv) / fp32 pull-x
      const bool v8 = al8 && r1al8 && (!r2 || ((ep->res2_cstride | ep->res2_coff) & 7) == 0) &&
                      (!aux || ((ep->aux_cstride | ep->aux_coff) & 7) == 0) && !ep->down2 && ep->act == 0 && r1;
      if (v8 && bias && ep->res_f32 == 0 && ep->out_mode == 0 && !aux) r->ep = 1;
      else if (v8 && !bias && (ep->res_f32 & 1) && (!r2 || (ep->res_f32 & 2)) && ep->out_mode == 1) r->ep = 2;
      // activation backward from a bf16 activation, bf16 out (the discriminator's layer-1 data gradient)
      else if (!bias && r1 && bwd && ep->res_f32 == 0 && !r2 && !aux && !ep->down2 && ep->out_mode == 0 && al8 && r1al8) r->ep = 4;
      else if (plain == 8) r->ep = bz ? 10 : ep->bn_part ? 9 : 8;
      else r->ep = plain;  // 3 / 6 / 7, or 0
      // BatchNorm partials per 16x16 tile of 64-channel blocks, >= 2 blocks (one block is conv_pw's or conv_n16's)
      r->parts |= (r->ep == 9 || r->ep == 10) && d->out_c % 64 == 0 && d->out_c >= 128 && d->stride == 1 && d->up == 1 && d->ks == 3;
    } else if (g.nchunk > 1 && nrx <= 18 && nrw <= 9) {
      // large input tiles (stride 2: 33x33 pixels per 16x16 outputs) with several chunks: the deeper-prefetch
      // variant (one workgroup per CU already, so the 18 staging vectors per thread cost no occupancy)
      r->pfx = 18; r->pfw = 9; r->ep = plain == 8 ? 8 : 0;
    } else {
      r->ep = plain;
    }
    // the GEO specialisation matching the geometry (conv_fwd_kernel): 16x16 tiles of 3x3 taps over 32-channel chunks
    const bool base = d->cc == 32 && d->ks == 3 && g.kcpad == 9 * 32;
    if (r->pfx != 18 && base && d->stride == 1 && g.tpw == TW + 2 && g.ccp == 48 && d->up == 1 && d->in_c % 32 == 0 &&
        g.nchunk * 32 == d->in_c && (long)d->n * d->in_h * d->in_w * d->in_cstride * 2 < (1L << 31) &&
        (long)r->ncob * r->nt * 16 * g.kpk * 2 < (1L << 31))
      r->geo = 1;
    if (r->pfx == 18 && base && d->stride == 2 && g.tpw == 2 * TW + 1 && g.ccp == 40) r->geo = 2;
  }
  if (r->geo == 1) {
    // the LDS-DMA form for the tiles it fills (32-row tiles: not the 16^2 VGG conv5 layers); with BatchNorm partials
    // (per 16 x 16 tile) only when every 32-row tile holds two whole 16-row tiles
    // RDB conv5 / pull-x (EP 1 / 2: 256 items at B=32 64^2, one round of one workgroup per CU) measured 7 % slower in
    // the GAN step than the two-workgroups-per-CU form (its chunk-0 latency and epilogue are not hidden in a single
    // round)
    const bool fits = (r->ep == 9 || r->ep == 10) ? d->out_h % DMA_TH == 0 : (d->out_h % DMA_TH == 0 || d->out_h >= 3 * DMA_TH);
    if (r->ep != 1 && r->ep != 2 && !ep->down2 && fits) {
      r->family = FAM_DMA;
      r->tiles_y = ceil_div(d->out_h, DMA_TH);
      r->xgrp = conv_xcd_group(r->ncob, (long)64 * g.kpk * 2);
      return;
    }
    r->xgrp = conv_xcd_group(r->ncob, (long)r->nt * 16 * g.kpk * 2);
  }
  const size_t lds_ep = (size_t)4 * r->mw * 16 * (r->nt * 16 + 4) * 4;  // epilogue staging (aliases the operands)
  r->lds = lds_ep > g.lds_total ? lds_ep : g.lds_total;
}

// The kernel of (d, bias, ep): the families in the order they claim a conv.  d->cc > 0.
static int fwd_pick(const ClimsrConvDesc* d, bool bias, const ClimsrEpilogue* ep, FwdRoute* r) {
  *r = FwdRoute{};
  const bool cc4 = d->cc == 4 && d->in_c == 4;  // conv_pw GEO 2 (climsr_conv_chunk_ex)
  const bool bz = ep->bn_part && ep->bn_z, r1 = ep->res1 != nullptr, r2 = ep->res2 != nullptr, aux = ep->aux != nullptr;
  FwdGeom& g = r->g;
  // 16x16 output tiles (64 px per wave) for the 64-channel layers; 8x16 otherwise
  const int mw = (d->out_h >= 12 && fwd_nt(d->out_c) == 4) ? 4 : 2;
  fwd_geom(d->in_c, d->ks, d->stride, d->out_c, d->cc, mw, &g);
  r->ncob = g.nt ? round_up(d->out_c, g.nt * 16) / (g.nt * 16) : 0;  // (the queries pick for unchecked descriptors)
  r->rf = ep->res_f32 != 0;
  r->tiles_x = ceil_div(d->out_w, TW); r->tiles_y = ceil_div(d->out_h, g.th);
  if (d->out_c == 1 && d->stride == 1 && d->up == 1 && !ep->down2 && !r2) {
    if (co1m_shape(d)) {
      r->family = FAM_CO1M; r->ks = d->ks; r->nch = d->in_c <= 32 ? 1 : 2;
    } else {
      r->family = FAM_CO1; r->tiles_x = ceil_div(d->out_w, 16); r->tiles_y = ceil_div(d->out_h, 16);
    }
    return PICK_OK;
  }
  if (n16_shape(d->in_c, d->ks, d->out_c) && d->cc == 32 * n16_ncb(d->in_c) && d->stride == 1 && d->up == 1 && d->pad == 1 &&
      !ep->down2 && !ep->res_f32 && d->out_h == d->in_h && d->out_w == d->in_w &&
      (long)d->n * d->in_h * d->in_w * d->in_cstride * 2 < (1L << 31)) {  // 32-bit buffer offsets
    // epilogue specialisations (see conv_n16_kernel): forward conv1-4 and the pull data gradients
    const bool al = ((d->out_cstride | d->out_coff) & 3) == 0 && d->out_c == 16 && !r2 && !aux && ep->out_mode == 0;
    r->family = FAM_N16; r->nch = d->cc / 32; r->tiles_y = ceil_div(d->out_h, N16_TH);
    r->ep = (al && ep->act == 1 && bias && !r1) ? 1
            : (al && ep->act == 3 && !bias && r1 && !(ep->res_f32 & 1) && ((ep->res1_cstride | ep->res1_coff) & 3) == 0) ? 2 : 0;
    return PICK_OK;
  }
  if (dgrad_s2_shape(d, bias, ep) && (long)d->n * d->out_h * d->out_w * ep->res1_cstride * 2 < (1L << 32) - 64) {
    r->family = FAM_DGRAD_S2;
    r->ep = (ep->act == 3 || ep->act == 4) ? 4 : bz ? 10 : 0;
    // 64 dx channels: one workgroup per 128 B pixel line (layer 1 with LeakyReLU': 158 -> 150 us at B=32; for wider
    // layers the 4 x 2 form is 2-8 % faster)
    r->mw = d->out_c == 64 ? 2 : 4; r->nt = d->out_c == 64 ? 4 : 2;
    r->tiles_x = ceil_div(d->in_w, 16); r->tiles_y = ceil_div(d->in_h, 4 * r->mw);
    r->parts = r->ep == 10 && plain_ep(d, bias, ep) == 8;
    return PICK_OK;
  }
  // the LDS-DMA kernel (conv_dma.hip conv_fwd_s2_dma_kernel); the register-staged 8-wave kernel it replaced measured
  // 352 against 332 us over the four discriminator stride-2 layers at B=32 (tools/perf_s2.py A/B, r04l)
  if (fwd_s2_shape(d, bias, ep, g)) {
    r->family = FAM_FWD_S2; r->ep = ep->bn_part ? 9 : 8;
    r->tiles_x = ceil_div(d->out_w, 16); r->tiles_y = ceil_div(d->out_h, 16);
    r->parts = ep->bn_part && !ep->bn_z;
    return PICK_OK;
  }
  if (pt_shape(d, ep) && (d->out_c == 16 || d->out_c == 32 || d->out_c == 64) && (d->in_c == 32 || d->in_c == 64 || d->in_c == 128)) {
    // epilogue specialisations: activation forward (3) / activation backward from a bf16 activation (4)
    const bool plain = !r2 && !aux && ep->out_mode == 0 && ep->res_f32 == 0;
    r->family = FAM_PT; r->nt = d->out_c / 16; r->nch = d->in_c / 32;
    r->ep = (plain && bias && !r1 && (ep->act == 1 || ep->act == 2)) ? 3 : (plain && !bias && r1 && (ep->act == 3 || ep->act == 4)) ? 4 : 0;
    return PICK_OK;
  }
  // 64 -> 64 3x3: the weights resident in registers, wave-independent tiles (conv_wr.hip)
  if (const int epk = conv_wr_ep(d, ep, bias); epk >= 0 && g.kpk >= 576) {
    r->family = FAM_WR; r->ep = epk;
    return PICK_OK;
  }
  if (pick_pw(d, bias, ep, cc4, r)) return PICK_OK;
  if (cc4) return PICK_CC4;
  if (g.lds_total > 160 * 1024) return PICK_LDS;
  pick_generic(d, bias, ep, bz, r);
  return PICK_OK;
}

// fwd_pick behind the argument checks of climsr_conv2d_fwd, in the order it reports them
static int fwd_route(const ClimsrConvDesc* d, bool bias, const ClimsrEpilogue* ep, FwdRoute* r) {
  if (!d || !ep) {
    set_error("conv2d_fwd: null argument");
    return CLIMSR_EINVAL;
  }
  const bool cc4 = d->cc == 4 && d->in_c == 4;
  if ((d->in_c % 8 && !cc4) || d->in_cstride % 8 || d->in_coff % 8 || (d->cc % 8 && !cc4) || d->cc <= 0 ||
      (d->up != 1 && d->up != 2 && d->up != -2) ||
      (d->stride != 1 && d->stride != 2) || d->ks < 1 || d->n <= 0 || d->out_c <= 0 || d->in_coff + d->in_c > d->in_cstride) {
    set_error("conv2d_fwd: unsupported geometry (in_c=%d cs=%d coff=%d cc=%d up=%d stride=%d ks=%d)", d->in_c, d->in_cstride,
              d->in_coff, d->cc, d->up, d->stride, d->ks);
    return CLIMSR_EINVAL;
  }
  if (ep->down2 && (ep->res2 || ep->res_f32 || bias || ep->act == 1 || ep->act == 2 || (ep->res1 && ep->act < 3) ||
                    (d->out_h & 1) || (d->out_w & 1))) {
    set_error("conv2d_fwd: down2 epilogue: no bias / forward activation / residual (act 3/4 mask only), even output size");
    return CLIMSR_EINVAL;
  }
  if (ep->act < 0 || ep->act > 4 || ((ep->act == 3 || ep->act == 4) && !ep->res1)) {
    set_error("conv2d_fwd: act %d invalid (3/4 need res1 = the activation output)", ep->act);
    return CLIMSR_EINVAL;
  }
  const int pick = fwd_pick(d, bias, ep, r);
  if (ep->ch_part && !(pick == PICK_OK && r->family == FAM_WR && (r->ep == 3 || r->ep == 4))) {
    set_error("conv2d_fwd: per-tile channel sums only from the 64 -> 64 3x3 register-resident conv "
              "(climsr_conv2d_fwd_ch_parts)");
    return CLIMSR_EINVAL;
  }
  if (ep->aux && ((ep->aux_cstride | ep->aux_coff) & 3)) {
    set_error("conv2d_fwd: aux channel stride/offset must be multiples of 4");
    return CLIMSR_EINVAL;
  }
  {  // epilogue operands are read through 32-bit buffer offsets (opt_rsrc)
    const long opx = (long)d->n * d->out_h * d->out_w;
    const long r1b = ep->res1 ? opx * ep->res1_cstride * ((ep->res_f32 & 1) ? 4 : 2) : 0;
    const long r2b = ep->res2 ? opx * ep->res2_cstride * ((ep->res_f32 & 2) ? 4 : 2) : 0;
    const long yb = opx * d->out_cstride * (ep->out_mode == 0 ? 2 : 4);
    if (r1b >= (1L << 32) - 64 || r2b >= (1L << 32) - 64 || yb >= (1L << 32) - 64) {
      set_error("conv2d_fwd: output / residual operand of %ld B exceeds 32-bit buffer addressing (split the batch)",
                r1b > r2b ? (r1b > yb ? r1b : yb) : (r2b > yb ? r2b : yb));
      return CLIMSR_EINVAL;
    }
  }
  if (ep->bn_part && ep->bn_z &&
      (!ep->bn_mean || !ep->bn_rstd || !ep->bn_gamma || !ep->bn_beta || ep->bn_z_cstride < d->out_c || ep->bn_z_cstride % 8 ||
       (long)d->n * d->out_h * d->out_w * ep->bn_z_cstride * 2 >= (1L << 31))) {
    set_error("conv2d_fwd: BatchNorm-backward partials need z (channel stride >= out_c, 8-aligned, < 2 GiB) and its statistics");
    return CLIMSR_EINVAL;
  }
  if (ep->bn_part && !(pick == PICK_OK && r->parts)) {
    set_error("conv2d_fwd: BatchNorm partials only for the 16x16-tile bf16 paths (climsr_conv2d_fwd_bn_parts)");
    return CLIMSR_EINVAL;
  }
  if (pick == PICK_CC4) {
    set_error("conv2d_fwd: 4-channel chunks need the conv_pw path (stride 1, up 1/2, 64 outputs, 32-bit offsets)");
    return CLIMSR_EINVAL;
  }
  if (pick == PICK_LDS) {
    set_error("conv2d_fwd: LDS %zu exceeds 160 KiB (cc=%d)", r->g.lds_total, d->cc);
    return CLIMSR_EINVAL;
  }
  return CLIMSR_OK;
}

// the kernel's name as rocprof reports it
static void fwd_route_name(const FwdRoute& r, char* name, size_t len) {
  const char* rf = r.rf ? "true" : "false";
  switch (r.family) {
    case FAM_CO1M: snprintf(name, len, "conv_co1m_kernel<%d, %d>", r.ks, r.nch); break;
    case FAM_CO1: snprintf(name, len, "conv_co1_kernel"); break;
    case FAM_N16: snprintf(name, len, "conv_n16_kernel<%d, %d>", r.nch, r.ep); break;
    case FAM_DGRAD_S2: snprintf(name, len, "conv_dgrad_s2_kernel<%d, %d, %d>", r.ep, r.mw, r.nt); break;
    case FAM_FWD_S2: snprintf(name, len, "conv_fwd_s2_dma_kernel<%s>", r.ep == 9 ? "true" : "false"); break;
    case FAM_PT: snprintf(name, len, "conv_pt_kernel<%d, %d, %d>", r.nt, r.nch, r.ep); break;
    case FAM_WR: snprintf(name, len, "conv_wr_kernel<%d>", r.ep); break;
    case FAM_PW: snprintf(name, len, "conv_pw_kernel<%d, %d, %d, %s, %d, %d, %d>", r.nw, r.mw, r.nt, rf, r.pv, r.ep, r.geo); break;
    case FAM_DMA: snprintf(name, len, "conv_fwd_dma_kernel<%d, %s>", r.ep, rf); break;
    default:
      snprintf(name, len, "%s<%d, %d, %s, %d, %d, %d, %d, %d>", r.pfx == 18 ? "conv_fwd_wide_kernel" : "conv_fwd_kernel", r.mw, r.nt,
               rf, fwd_mv(r.nt), r.pfx, r.pfw, r.ep, r.geo);
  }
}

// the kernel arguments of route r
static FwdArgs fwd_args(const FwdRoute& r, const ClimsrConvDesc* d, const uint16_t* x, const uint16_t* wpk, const float* bias,
                        const ClimsrEpilogue* ep, void* y) {
  const FwdGeom& g = r.g;
  FwdArgs a{};  // zero: the optional operands (bz, bn_part, the stagger, ...) default to absent
  a.x = x; a.w = wpk; a.bias = bias; a.y = y;
  a.res1 = ep->res1; a.res2 = ep->res2; a.aux = (uint16_t*)ep->aux;
  a.res_f32 = ep->res_f32; a.beta1 = ep->beta1; a.beta2 = ep->beta2;
  a.aux_cs = ep->aux_cstride; a.aux_co = ep->aux_coff; a.aux_scale = ep->aux_scale;
  a.n = d->n; a.in_h = d->in_h; a.in_w = d->in_w; a.in_c = d->in_c; a.in_cs = d->in_cstride; a.in_co = d->in_coff;
  a.up = d->up; a.ks = d->ks; a.stride = d->stride; a.pad = d->pad; a.out_h = d->out_h; a.out_w = d->out_w;
  a.out_c = d->out_c; a.out_cs = d->out_cstride; a.out_co = d->out_coff; a.cc = d->cc;
  a.tph = g.tph; a.tpw = g.tpw; a.ccp = g.ccp; a.kcpad = g.kcpad; a.nchunk = g.nchunk; a.kpk = g.kpk;
  a.tiles_x = r.tiles_x; a.tiles_y = r.tiles_y;
  a.act = ep->act; a.out_mode = ep->out_mode; a.down2 = ep->down2;
  a.slope = ep->slope; a.alpha1 = ep->alpha1; a.alpha2 = ep->alpha2;
  a.r1_cs = ep->res1_cstride; a.r1_co = ep->res1_coff; a.r2_cs = ep->res2_cstride; a.r2_co = ep->res2_coff;
  a.lds_tab = (int)g.lds_tab; a.lds_x = (int)g.lds_x;
  a.bn_part = ep->bn_part;
  a.xgrp = r.xgrp;
  if (ep->bn_part && ep->bn_z) {
    a.bz = ep->bn_z; a.bz_cs = ep->bn_z_cstride; a.bslope = ep->bn_slope;
    a.bmean = ep->bn_mean; a.brstd = ep->bn_rstd; a.bgamma = ep->bn_gamma; a.bbeta = ep->bn_beta;
  }
  if (r.family == FAM_PW) {
    const PwGeom& p = r.pg;
    a.tph = p.tph; a.tpw = p.tpw; a.ccp = p.ccp; a.kcpad = p.kcpad;
    a.lds_tab = (int)p.lds_tab;
    a.lds_x = (int)p.lds_w;  // offset of the input tile = tab + weights
    if (d->cc == 4) a.cc = a.in_c = 8;  // 4-channel taps: staged as 8-channel pixels (16 B loads)
  }
  if (r.family == FAM_DMA) a.nchunk = a.in_c / 32;  // 32-channel chunks (of a 32- or 64-channel packing)
  return a;
}

// CO1M, CO1, N16, PT: the instantiation of the route's ids
static int launch_small(const FwdRoute& r, const FwdArgs& a, hipStream_t s) {
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

extern "C" int climsr_conv2d_fwd(const ClimsrConvDesc* d, const uint16_t* x, const uint16_t* wpk, const float* bias,
                                 const ClimsrEpilogue* ep, void* y, void* stream) {
  if (!d || !x || !wpk || !ep || !y) {
    set_error("conv2d_fwd: null argument");
    return CLIMSR_EINVAL;
  }
  FwdRoute r;
  if (int e = fwd_route(d, bias != nullptr, ep, &r)) return e;
  hipStream_t s = (hipStream_t)stream;
  if (r.family == FAM_WR) return conv_wr_launch(r.ep, d, ep, x, wpk, r.g.kpk, bias, y, s);
  const FwdArgs a = fwd_args(r, d, x, wpk, bias, ep, y);
  switch (r.family) {
    case FAM_PW: return fwd_pw_launch(r, a, s);
    case FAM_DGRAD_S2: return launch_dgrad_s2(r, a, s);
    case FAM_FWD_S2: {
      const int rc = fwd_s2_dma_launch(a, s);
      return rc == CLIMSR_OK ? check_launch("conv2d_fwd (s2 LDS-DMA)") : rc;
    }
    case FAM_FWD:
    case FAM_DMA: return fwd_generic_launch(r, a, s);
    default: return launch_small(r, a, s);
  }
}

extern "C" const char* climsr_conv2d_fwd_kernel(const ClimsrConvDesc* d, const float* bias, const ClimsrEpilogue* ep) {
  static thread_local char name[96];
  name[0] = 0;
  FwdRoute r;
  if (fwd_route(d, bias != nullptr, ep, &r) == CLIMSR_OK) fwd_route_name(r, name, sizeof(name));
  return name;
}

extern "C" int64_t climsr_conv2d_fwd_ch_parts(const ClimsrConvDesc* d, const ClimsrEpilogue* ep, int32_t* tiles_per_image) {
  if (!d || !ep || d->cc <= 0) return 0;
  ClimsrEpilogue e = *ep;
  e.ch_part = (float*)1;  // (only its presence matters to the route)
  FwdRoute r;
  if (fwd_pick(d, false, &e, &r) != PICK_OK || r.family != FAM_WR || (r.ep != 3 && r.ep != 4)) return 0;
  const int tpi = conv_wr_tiles_per_image(d);
  if (tiles_per_image) *tiles_per_image = tpi;
  return (int64_t)tpi * d->n;
}

extern "C" int64_t climsr_conv2d_fwd_bn_parts(const ClimsrConvDesc* d, const ClimsrEpilogue* ep) {
  if (!d || !ep || d->cc % 8 || d->cc <= 0 || d->stride < 1) return 0;
  ClimsrEpilogue e = *ep;
  e.bn_part = (double*)1;  // (only its presence matters to the route)
  FwdRoute r;
  if (fwd_pick(d, false, &e, &r) != PICK_OK || !r.parts) return 0;
  if (d->up == -2) return (int64_t)ceil_div(d->in_w, 16) * ceil_div(d->in_h, 4 * (d->out_c == 64 ? 2 : 4)) * d->n;  // dz tiles
  return (int64_t)ceil_div(d->out_w, TW) * ceil_div(d->out_h, 16) * d->n;
}

// ------------------------------------------------------------------------------------------
// Weight gradient: dW[co][ci][tap] = sum_px dz[px][co] * x[px*stride + tap - pad][ci]
// GEMM: M = co (A = dz^T), N = ci (B = x), K = pixels.  Both operands are pixel-major in NHWC, so
// they are read from LDS with ds_read_b64_tr_b16 (row = pixel, any per-lane pixel address: the
// tap shift of the im2col is free).  WG tile: 16*NTC co x 16 ci x TB taps; the 4 waves split the
// pixels of each 16x16 output-pixel tile and are summed through LDS at the end; splits over
// pixel tiles write disjoint fp32 partial slabs (deterministic, reduced by wgrad_reduce).
// ------------------------------------------------------------------------------------------
constexpr int WG_TH = 16;
constexpr int WG_XP = 24;  // LDS pixel pitch (channels) of the x tile (16 + 8 pad)

struct WgArgs {
  const uint16_t* x;
  const uint16_t* dz;
  float* part;
  float* bpart;
  int n, in_h, in_w, in_c, in_cs, in_co, up, ks, stride, pad, out_h, out_w, out_c, dz_cs;
  int tph, tpw, dzp, tiles_x, tiles_y, ntiles, nsplit, ntapb, ncib, co_rows, kw;
  int lds_x;
  int xcd;  // conv_wgrad64_kernel: 1-D grid in XCD-major (split, channel block) order (else blockIdx.y = split)
};

// CI4 = 1: inputs with <= 4 real channels (srcnn.conv1 / conv_first, 3 channels).  The x tile holds 4
// channels per pixel and a B fragment's 16 columns are (4 taps x 4 channels): in the transposed read
// each lane group p points at its own tap, so 81 taps need 21 fragments instead of 81 mostly-zero ones.
// TB then counts tap groups of 4.
// WS (wave-split taps, CI4 9x9 = srcnn.conv1): one workgroup covers ALL tap groups, wave w owns groups
// [TB w, TB w + TB) over every pixel of the tile, so dz is read once per launch (the tap-blocked form re-reads it
// per block: 1 GB fetched for 0.3 GB of data) and no cross-wave reduction is needed.
template <int NTC, int TB, int CI4, bool WS = false>
__global__ __launch_bounds__(256) void conv_wgrad_kernel(WgArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  uint16_t* xs = (uint16_t*)smem;
  uint16_t* zs = (uint16_t*)(smem + a.lds_x);
  float* red = (float*)smem;  // reused for the cross-wave reduction at the end

  const int tid = threadIdx.x;
  const int wave = tid >> 6;
  const int lane = tid & 63;
  const int g = lane >> 4;
  const int q = (lane & 15) >> 2;
  const int p = lane & 3;
  const int col = lane & 15;

  int bid = blockIdx.x;
  const int tb = bid % a.ntapb;
  bid /= a.ntapb;
  const int cib = bid % a.ncib;
  const int cob = bid / a.ncib;
  const int split = blockIdx.y;
  const int ci0 = cib * 16;
  const int co0 = cob * NTC * 16;
  const int tap0 = (WS ? wave : tb) * TB * (CI4 ? 4 : 1);
  constexpr int XP = CI4 ? 4 : WG_XP;  // LDS x-tile pixel pitch (channels)
  const int ks2 = a.ks * a.ks;
  const bool do_bias = (cib == 0 && tb == 0 && a.bpart != nullptr) && (!WS || wave == 0);

  f32x4 acc[NTC][TB];
  f32x4 accb[NTC];
#pragma unroll
  for (int t = 0; t < NTC; ++t) {
    accb[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int u = 0; u < TB; ++u) acc[t][u] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }
  bf16x8 ones;
#pragma unroll
  for (int i = 0; i < 8; ++i) ones[i] = (__bf16)1.0f;

  int tapoff[TB];  // per-lane LDS offset of fragment u's columns (4p..4p+3)
#pragma unroll
  for (int u = 0; u < TB; ++u) {
    int tap = CI4 ? tap0 + 4 * u + p : tap0 + u;
    if (tap >= ks2) tap = 0;  // weight rows past ks*ks are never written
    tapoff[u] = ((tap / a.ks) * a.tpw + (tap % a.ks)) * XP + (CI4 ? 0 : 4 * p);
  }

  const int lh = a.in_h * a.up, lw = a.in_w * a.up;  // up in {1, 2} here
  const int upsh = a.up == 2 ? 1 : 0;
  constexpr int zvec = NTC * 2;  // 16B vectors of dz per pixel
  constexpr int XSTEP = CI4 ? 256 : 128;  // pixels advanced per 256 staging vectors
  const int x_dy = XSTEP / a.tpw, x_dx = XSTEP - x_dy * a.tpw;
  const int xpix0 = CI4 ? tid : (tid >> 1);
  const int x_ty0 = xpix0 / a.tpw, x_tx0 = xpix0 - x_ty0 * a.tpw;
  const int nvec_x = a.tph * a.tpw * (CI4 ? 1 : 2);
  const int nvec_z = WG_TH * TW * zvec;

  for (int tile = split; tile < a.ntiles; tile += a.nsplit) {
    int tt = tile;
    const int tx = tt % a.tiles_x;
    tt /= a.tiles_x;
    const int ty = tt % a.tiles_y;
    const int nimg = tt / a.tiles_y;
    const int ox0 = tx * TW, oy0 = ty * WG_TH;
    const int iy0 = oy0 * a.stride - a.pad, ix0 = ox0 * a.stride - a.pad;
    __syncthreads();
    // batched staging (all loads of a round in flight before the first LDS store); x-tile pixel
    // coordinates advance incrementally (thread's pixels are (tid>>1) + 128k, channel half tid&1)
    {
      const int h = tid & 1;
      int ty_ = x_ty0, tx_ = x_tx0;
      const int nrx = (nvec_x + 255) / 256;
      for (int base = 0; base < nrx; base += FWD_MAXV) {
        uint4 buf[FWD_MAXV];
        int dst[FWD_MAXV];
#pragma unroll
        for (int i = 0; i < FWD_MAXV; ++i) {
          dst[i] = -1;
          if (base + i < nrx && ty_ < a.tph) {
            const int iy = iy0 + ty_, ix = ix0 + tx_;
            const int c = ci0 + (CI4 ? 0 : h * 8);
            uint4 val = make_uint4(0, 0, 0, 0);
            const bool ok = iy >= 0 && iy < lh && ix >= 0 && ix < lw && c < a.in_c;
            const long src = (((long)nimg * a.in_h + (iy >> upsh)) * a.in_w + (ix >> upsh)) * a.in_cs + a.in_co + c;
            if (CI4) {
              if (ok) {
                uint2 v2 = *(const uint2*)(a.x + src);
                val.x = v2.x;
                val.y = v2.y;
              }
            } else if (ok) {
              val = *(const uint4*)(a.x + src);
            }
            buf[i] = val;
            dst[i] = (ty_ * a.tpw + tx_) * XP + (CI4 ? 0 : h * 8);
          }
          tx_ += x_dx;
          ty_ += x_dy;
          if (tx_ >= a.tpw) { tx_ -= a.tpw; ++ty_; }
        }
#pragma unroll
        for (int i = 0; i < FWD_MAXV; ++i) {
          if (dst[i] < 0) continue;
          if (CI4) *(uint2*)(xs + dst[i]) = make_uint2(buf[i].x, buf[i].y);
          else *(uint4*)(xs + dst[i]) = buf[i];
        }
      }
      const int nrz = nvec_z / 256;  // exact: 256 px x zvec vectors
      for (int base = 0; base < nrz; base += FWD_MAXV) {
        uint4 buf[FWD_MAXV];
#pragma unroll
        for (int i = 0; i < FWD_MAXV; ++i) {
          if (base + i < nrz) {
            const int vz = tid + (base + i) * 256;
            const int pix = vz / zvec;  // zvec = 2*NTC: compile-time power of two
            const int cv = vz - pix * zvec;
            const int oy = oy0 + pix / TW, ox = ox0 + (pix % TW);
            const int c = co0 + cv * 8;
            uint4 val = make_uint4(0, 0, 0, 0);
            if (oy < a.out_h && ox < a.out_w && c < a.dz_cs)
              val = *(const uint4*)(a.dz + (((long)nimg * a.out_h + oy) * a.out_w + ox) * a.dz_cs + c);
            buf[i] = val;
          }
        }
#pragma unroll
        for (int i = 0; i < FWD_MAXV; ++i) {
          if (base + i < nrz) {
            const int vz = tid + (base + i) * 256;
            const int pix = vz / zvec;
            *(uint4*)(zs + pix * a.dzp + (vz - pix * zvec) * 8) = buf[i];
          }
        }
      }
    }
    __syncthreads();
#pragma unroll 2  // (a full unroll of the WS variant's 8 k-steps made hipcc copy the accumulators AGPR<->VGPR)
    for (int s = 0; s < (WS ? 8 : 2); ++s) {
      const int kk = WS ? s : wave * 2 + s;  // k-step: output pixel rows 2kk, 2kk+1 of the tile
      // pixel handled as row q (+4) of this lane's tr reads
      const int k0 = kk * 32 + 8 * g + q;
      const int k1 = k0 + 4;
      const int r0 = k0 >> 4, c0_ = k0 & 15, r1 = k1 >> 4, c1_ = k1 & 15;
      bf16x8 af[NTC];
#pragma unroll
      for (int t = 0; t < NTC; ++t) {
        s16x4 lo = ds_read_tr16(zs + k0 * a.dzp + t * 16 + 4 * p);
        s16x4 hi = ds_read_tr16(zs + k1 * a.dzp + t * 16 + 4 * p);
        short v8[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        af[t] = __builtin_bit_cast(bf16x8, v8);
      }
      const int xb0 = ((r0 * a.stride) * a.tpw + c0_ * a.stride) * XP;
      const int xb1 = ((r1 * a.stride) * a.tpw + c1_ * a.stride) * XP;
      if (do_bias) {
#pragma unroll
        for (int t = 0; t < NTC; ++t) accb[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[t], ones, accb[t], 0, 0, 0);
      }
#pragma unroll
      for (int u = 0; u < TB; ++u) {
        s16x4 lo = ds_read_tr16(xs + xb0 + tapoff[u]);
        s16x4 hi = ds_read_tr16(xs + xb1 + tapoff[u]);
        short v8[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        bf16x8 bfr = __builtin_bit_cast(bf16x8, v8);
#pragma unroll
        for (int t = 0; t < NTC; ++t) acc[t][u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[t], bfr, acc[t][u], 0, 0, 0);
      }
    }
  }

  // cross-wave reduction through LDS (waves 1..3 -> wave 0)
  constexpr int NF = NTC * TB;
  for (int r = 1; r < (WS ? 1 : 4); ++r) {
    __syncthreads();
    if (wave == r) {
#pragma unroll
      for (int t = 0; t < NTC; ++t)
#pragma unroll
        for (int u = 0; u < TB; ++u) *(f32x4*)(red + ((t * TB + u) * 64 + lane) * 4) = acc[t][u];
#pragma unroll
      for (int t = 0; t < NTC; ++t) *(f32x4*)(red + ((NF + t) * 64 + lane) * 4) = accb[t];
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int t = 0; t < NTC; ++t) {
#pragma unroll
        for (int u = 0; u < TB; ++u) acc[t][u] += *(f32x4*)(red + ((t * TB + u) * 64 + lane) * 4);
        accb[t] += *(f32x4*)(red + ((NF + t) * 64 + lane) * 4);
      }
    }
  }
  if (!WS && wave != 0) return;
  const int ci = CI4 ? (col & 3) : ci0 + col;
  float* slab = a.part + (long)split * a.co_rows * a.kw;
#pragma unroll
  for (int t = 0; t < NTC; ++t) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int co = co0 + t * 16 + g * 4 + i;
      if (ci < a.in_c) {
#pragma unroll
        for (int u = 0; u < TB; ++u) {
          const int tap = CI4 ? tap0 + 4 * u + (col >> 2) : tap0 + u;
          if (tap < ks2) slab[(long)co * a.kw + ci * ks2 + tap] = acc[t][u][i];
        }
      }
      if (do_bias && col == 0) a.bpart[(long)split * a.co_rows + co] = accb[t][i];
    }
  }
}

// Weight gradient for 3x3 stride-1 convs with 64k output and 64k input channels (the RDB conv5 / the
// whole-RDB combined GEMM, trunk / upconv / HRconv): workgroup block = 64 co x 64 ci x 9 taps, wave w owns
// ci 16w..16w+15 (4 co fragments x 9 taps = 36 accumulators), so the workgroup's 4 waves never reduce with
// each other; the 8x16-pixel tiles of its split are walked with the NEXT tile's dz / x prefetched into
// registers while the current one is on the MFMA pipe.  Partials: [split][co_rows][in_c*9] (as above).
// Stride 2 (the discriminator's features.2/8/14/20): 4 x 16 output tiles whose (2*4+1) x (2*16+1) input
// footprint is staged whole; tap (r, s) of output pixel k reads tile pixel (2*row(k) + r, 2*col(k) + s).
// LDS pixel pitches (channels).  A transposed fragment read (ds_read_b64_tr_b16) is served 32 lanes at a time:
// with the k-step's pixel rows taken as 4g + q (+16), those 32 lanes read 8 consecutive tile pixels, 32 B each,
// which land in 8 disjoint 8-bank groups when one pixel step is 8 x odd banks: pitch 80 (dz tile; x tile at
// stride 1) or 72 (x tile at stride 2, where a pixel step is two tile pixels).  The old 72 / rows 8g + q left
// SQ_LDS_BANK_CONFLICT at 42 % of the LDS cycles.
constexpr int W64_P = 64 + 8;  // (dzp of the generic wgrad path's descriptor)
constexpr int W64_ZP = 80;
template <int S>
struct W64 {
  static constexpr int TH = S == 1 ? 8 : 4;                    // output tile rows (x TW = 16 columns)
  static constexpr int TPH = S * (TH - 1) + 3, TPW = S * (TW - 1) + 3;  // staged input footprint
  static constexpr int XP = S == 1 ? 80 : 72;                 // x tile pixel pitch
  static constexpr int NZ = TH * TW * 8;                      // 16 B vectors of a dz tile (TH*16 px x 64 ch)
  static constexpr int NX = TPH * TPW * 8;                    // of an x tile
  // + one spare x pixel: the stash's lanes past the tile write there (no branch in the tile loop)
  static constexpr size_t LDS = (size_t)TH * TW * W64_ZP * 2 + (size_t)(TPH * TPW + 1) * XP * 2;
};

// TS = 2: 8 waves, wave w owns ci block w & 3 and taps [0,5) or [5,9) (w >> 2): 20 accumulators instead of 36, so
// two waves share each SIMD (latency hiding) at the price of each wave re-reading the shared dz fragments.
// G (TS 1, S 1): the LDS-DMA form -- see conv_wgrad64_glds_kernel below.
template <int TS, int S, bool G>
__device__ __forceinline__ void wgrad64_body(const WgArgs& a) {
  static_assert(!G || (TS == 1 && S == 1), "LDS-DMA form: 256 threads, stride 1");
  constexpr int NTHR = 256 * TS, NU = TS == 1 ? 9 : 5;
  constexpr int TH = W64<S>::TH, TPW = W64<S>::TPW, NZ = W64<S>::NZ, NX = W64<S>::NX, XP = W64<S>::XP;
  extern __shared__ __attribute__((aligned(16))) char smem[];  // TS 1: two buffers of W64<S>::LDS
  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4;
  const int wave = (tid >> 6) & 3, tg = TS == 1 ? 0 : tid >> 8;  // ci block, tap group
  const int u0 = tg * 5;
  const int q = (lane & 15) >> 2, p = lane & 3, col = lane & 15;
  // (split, 64x64 block): with a.xcd the XCD-major order in which a split's blocks are consecutive on one XCD -- they
  // walk the same pixel tiles at the same time, so each x / dz tile is fetched into that L2 once for all of them
  const int nblk = a.ncib * (a.out_c / 64);
  const int bidx = a.xcd ? xcd_major(blockIdx.x, gridDim.x) : blockIdx.x;
  const int blk = a.xcd ? bidx % nblk : bidx, split = a.xcd ? bidx / nblk : blockIdx.y;
  const int cib = blk % a.ncib, cob = blk / a.ncib;
  const int ci0 = cib * 64, co0 = cob * 64;
  const bool do_bias = cib == 0 && a.bpart != nullptr;
  const int lh = a.in_h * a.up, lw = a.in_w * a.up;
  const int upsh = a.up == 2 ? 1 : 0;

  f32x4 acc[4][NU], accb[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    accb[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int u = 0; u < NU; ++u) acc[t][u] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }
  bf16x8 ones;
#pragma unroll
  for (int i = 0; i < 8; ++i) ones[i] = (__bf16)1.0f;
  int tapoff[NU];
#pragma unroll
  for (int u = 0; u < NU; ++u) {
    if constexpr (TS == 1) {
      tapoff[u] = ((u / 3) * TPW + (u % 3)) * XP + wave * 16 + 4 * p;
    } else {
      const int tp = u0 + u < 9 ? u0 + u : 8;
      tapoff[u] = ((tp / 3) * TPW + (tp % 3)) * XP + wave * 16 + 4 * p;
    }
  }

  constexpr int VZ = NZ / NTHR, VX = (NX + NTHR - 1) / NTHR;
  uint4 pz[VZ], px[VX];
  // Branch-free tile loads: buffer loads whose byte offset is pushed out of range for halo / ragged lanes return
  // zeros (no branch around a load: hipcc waits vmcnt(0) at each one under a condition, and the per-vector 64-bit
  // address arithmetic of the branchy form was ~20 VALU a vector -- VALU-issue-bound at one wave per SIMD).  Every
  // per-vector term that does not depend on the tile is a per-thread constant.
  // dz vector i: pixel row zr + (NTHR / 128) i, column zc of the tile, channels co0 + 8 (tid & 7)
  const int zr = tid >> 7, zc = (tid >> 3) & 15, cg8 = (tid & 7) * 8;
  const uint32_t zrow_b = (uint32_t)a.out_w * a.dz_cs * 2;
  const uint32_t z_lane = (uint32_t)((zc * a.dz_cs + co0 + cg8) * 2) + (uint32_t)zr * zrow_b;
  const __amdgpu_buffer_rsrc_t zrs = buf_rsrc(a.dz, (uint32_t)((long)a.n * a.out_h * a.out_w * a.dz_cs * 2));
  // x vector i: tile pixel (xpy[i], xpx[i]), channels ci0 + 8 (tid & 7) (the upsample-on-load source: pixel >> 1)
  int xpy[VX], xpx[VX];
#pragma unroll
  for (int i = 0; i < VX; ++i) {
    const int pix = (tid + NTHR * i) >> 3;
    xpy[i] = tid + NTHR * i < NX ? pix / TPW : 1 << 20;  // past the tile: never in range
    xpx[i] = pix % TPW;
  }
  const uint32_t ximg_b = (uint32_t)a.in_h * a.in_w * a.in_cs * 2;
  const uint32_t x_lane = (uint32_t)((a.in_co + ci0 + cg8) * 2);
  const __amdgpu_buffer_rsrc_t xrs = buf_rsrc(a.x, (uint32_t)((long)a.n * a.in_h * a.in_w * a.in_cs * 2));
  // split-strided tile walk with incremental coordinates (no per-tile integer divisions on the scalar pipe)
  const int s_x = a.nsplit % a.tiles_x, s_y = (a.nsplit / a.tiles_x) % a.tiles_y, s_n = a.nsplit / (a.tiles_x * a.tiles_y);
  int ntx = split % a.tiles_x, nty = (split / a.tiles_x) % a.tiles_y, nn = split / (a.tiles_x * a.tiles_y);
  auto issue = [&](bool live) {  // the tile at (ntx, nty, nn) (zeros if !live), then advance them by nsplit tiles
    const int tx = ntx, ty = nty, nimg = nn;
    ntx += s_x;
    int c = ntx >= a.tiles_x;
    ntx -= c ? a.tiles_x : 0;
    nty += s_y + c;
    c = nty >= a.tiles_y;
    nty -= c ? a.tiles_y : 0;
    nn += s_n + c;
    const int oy0 = ty * TH, ox0 = tx * TW;
    const uint32_t zt = (uint32_t)(((nimg * a.out_h + oy0) * a.out_w + ox0) * a.dz_cs * 2) + z_lane;
    const bool zok = live && ox0 + zc < a.out_w;
#pragma unroll
    for (int i = 0; i < VZ; ++i) {
      const bool ok = zok && oy0 + zr + (NTHR / 128) * i < a.out_h;
      pz[i] = buf_load16(zrs, ok ? zt + (uint32_t)((NTHR / 128) * i) * zrow_b : BUF_OOB);
    }
    const int iy0 = S * oy0 - a.pad, ix0 = S * ox0 - a.pad;
    const uint32_t xt = (uint32_t)nimg * ximg_b + x_lane;
#pragma unroll
    for (int i = 0; i < VX; ++i) {
      const int iy = iy0 + xpy[i], ix = ix0 + xpx[i];
      const bool ok = live && iy >= 0 && iy < lh && ix >= 0 && ix < lw;
      const uint32_t off = xt + (uint32_t)((((iy >> upsh) * a.in_w) + (ix >> upsh)) * a.in_cs * 2);
      px[i] = buf_load16(xrs, ok ? off : BUF_OOB);
    }
  };
  // buffer b of the staged tiles: dz [TH*16 px][W64_ZP], x [TPH*TPW px][XP]
  auto zbuf = [&](int b) { return (uint16_t*)(smem + b * W64<S>::LDS); };
  auto xbuf = [&](int b) { return (uint16_t*)(smem + b * W64<S>::LDS) + TH * TW * W64_ZP; };
  auto stash = [&](int b) {
    uint16_t* zs = zbuf(b);
    uint16_t* xs = xbuf(b);
#pragma unroll
    for (int i = 0; i < VZ; ++i) {
      const int v = tid + NTHR * i;
      *(uint4*)(zs + (v >> 3) * W64_ZP + (v & 7) * 8) = pz[i];
    }
#pragma unroll
    for (int i = 0; i < VX; ++i) {
      const int v = tid + NTHR * i;
      *(uint4*)(xs + (v < NX ? v >> 3 : W64<S>::TPH * TPW) * XP + (v & 7) * 8) = px[i];  // past the tile: the spare pixel
    }
  };
  // k-step kk = 32 output pixels of the tile; lane group g's 8 k values = pixel rows 4g + q and 16 + 4g + q (a
  // permutation of the k-step's pixels, the same for both operands)
  const bool last_short = TS == 2 && tg == 1;  // tap group 1 has 4 taps (5..8)
  auto frags = [&](int b, int kk, bf16x8 (&af)[4], bf16x8 (&bf)[NU]) {
    const uint16_t* zs = zbuf(b);
    const uint16_t* xs = xbuf(b);
    const int k0 = kk * 32 + 4 * g + q, k1 = k0 + 16;
#pragma unroll
    for (int t = 0; t < 4; ++t)
      af[t] = cat_tr(ds_read_tr16(zs + k0 * W64_ZP + t * 16 + 4 * p), ds_read_tr16(zs + k1 * W64_ZP + t * 16 + 4 * p));
    const int xb0 = (S * (k0 >> 4) * TPW + S * (k0 & 15)) * XP, xb1 = (S * (k1 >> 4) * TPW + S * (k1 & 15)) * XP;
#pragma unroll
    for (int u = 0; u < NU; ++u) bf[u] = cat_tr(ds_read_tr16(xs + xb0 + tapoff[u]), ds_read_tr16(xs + xb1 + tapoff[u]));
  };
  auto mma = [&](const bf16x8 (&af)[4], const bf16x8 (&bf)[NU]) {
    // the bias gradient (sum of dz over the pixels) on every wave: 4 more MFMAs per k-step, but no branch in the tile
    // loop (a wave-uniform branch here made hipcc copy the 144 accumulators between AGPRs and VGPRs every tile);
    // wave 0 of a bias-owning workgroup stores it
#pragma unroll
    for (int t = 0; t < 4; ++t) accb[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[t], ones, accb[t], 0, 0, 0);
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      if (u == NU - 1 && last_short) continue;
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t][u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[t], bf[u], acc[t][u], 0, 0, 0);
    }
  };
  constexpr int NK = TH * TW / 32;  // 4 (stride 1) or 2 (stride 2): even
  int tile = split;
  if constexpr (G) {
    // LDS-DMA staging: buffer_load ... lds writes each wave-instruction's 64 x 16 B straight into LDS at
    // (wave-uniform base + 16 lane), so the tiles need no registers, no ds_write pass and no VALU to move them,
    // and three buffers keep two tiles in flight (the register path held one tile in 40 VGPRs, and with two whole
    // fragment sets its 160 accumulators overflowed into AGPR copies: 4.5 VALU per MFMA).  Images are lane-linear:
    // lane l of an instruction fills pixel slot 8 i + (l >> 3), 16 B position l & 7, with that pixel's channel chunk
    // (l & 7) ^ (column & 7) -- an XOR swizzle chosen on the global (source) side that spreads the 8 pixels of a
    // transposed fragment read over all 64 banks, as the register path's 80-element pitch did.
    constexpr int ZB = TH * TW * 128, XB = 24 * 1024, BUF = ZB + XB, NXP = W64<1>::TPH * TPW;
    const int l8 = lane >> 3, c8 = lane & 7, wv = tid >> 6;
    // dz: wave w issues instructions w + 4 j (j < 4): tile row (w >> 1) + 2 j, column 8 (w & 1) + l8
    const int zcol = 8 * (wv & 1) + l8, zrow0 = wv >> 1;
    const uint32_t zrow_b = (uint32_t)a.out_w * a.dz_cs * 2;
    const uint32_t z_lane = (uint32_t)((zcol * a.dz_cs + co0 + 8 * (c8 ^ (zcol & 7))) * 2) + (uint32_t)zrow0 * zrow_b;
    const __amdgpu_buffer_rsrc_t zrs = buf_rsrc(a.dz, (uint32_t)((long)a.n * a.out_h * a.out_w * a.dz_cs * 2));
    // x: instructions w + 4 j (j < 6): footprint pixel 8 (w + 4 j) + l8 of the 10 x 18 footprint (180 pixels; the
    // slots past it get zeros): (row << 16) | (column << 8) | source chunk
    int xrc[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      const int P = 8 * (wv + 4 * j) + l8, row = P < NXP ? P / TPW : 1023, cx = P % TPW;
      xrc[j] = (row << 16) | (cx << 8) | (c8 ^ (cx & 7));
    }
    const uint32_t ximg_b = (uint32_t)a.in_h * a.in_w * a.in_cs * 2, pxb = (uint32_t)a.in_cs * 2;
    const uint32_t x_ch = (uint32_t)((a.in_co + ci0) * 2);
    const __amdgpu_buffer_rsrc_t xrs = buf_rsrc(a.x, (uint32_t)((long)a.n * a.in_h * a.in_w * a.in_cs * 2));
    const int s_x = a.nsplit % a.tiles_x, s_y = (a.nsplit / a.tiles_x) % a.tiles_y, s_n = a.nsplit / (a.tiles_x * a.tiles_y);
    int ntx = split % a.tiles_x, nty = (split / a.tiles_x) % a.tiles_y, nn = split / (a.tiles_x * a.tiles_y);
    // in asm, not __builtin_amdgcn_raw_ptr_buffer_load_lds: hipcc treats the builtin as an LDS write of unknown
    // extent and waits vmcnt(0) before the next ds_read, i.e. for the tile just requested; hidden from it, the DMAs
    // are counted by hand (vmcnt(10) below) and drained before the epilogue.  M0 (the wave's LDS destination) is set
    // and restored inside the statement.
    const uint32_t lds0 = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) char*)smem;
    const int wvu = __builtin_amdgcn_readfirstlane(wv);  // provably wave-uniform: the LDS destination is an "s" operand
    auto glds = [&](__amdgpu_buffer_rsrc_t r, uint32_t off, uint32_t lds) {
      uint32_t keep;
      asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds\n\ts_mov_b32 m0, %0"
                   : "=&s"(keep) : "v"(off), "s"(r), "s"(lds) : "memory");
    };
    auto issue = [&](bool live, int b) {  // the tile at (ntx, nty, nn) into buffer b (zeros if !live), then advance
      const int tx = ntx, ty = nty, nimg = nn;
      ntx += s_x;
      int c = ntx >= a.tiles_x;
      ntx -= c ? a.tiles_x : 0;
      nty += s_y + c;
      c = nty >= a.tiles_y;
      nty -= c ? a.tiles_y : 0;
      nn += s_n + c;
      const int oy0 = ty * TH, ox0 = tx * TW;
      const uint32_t zb = lds0 + (uint32_t)(b * BUF);
      const uint32_t zt = (uint32_t)(((nimg * a.out_h + oy0) * a.out_w + ox0) * a.dz_cs * 2) + z_lane;
      const bool zok = live & (ox0 + zcol < a.out_w);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool ok = zok & (oy0 + zrow0 + 2 * j < a.out_h);
        glds(zrs, ok ? zt + (uint32_t)(2 * j) * zrow_b : BUF_OOB, zb + (uint32_t)((wvu + 4 * j) * 1024));
      }
      const uint32_t iy0 = (uint32_t)(oy0 - a.pad), ix0 = (uint32_t)(ox0 - a.pad), xt = (uint32_t)nimg * ximg_b + x_ch;
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        const uint32_t iy = iy0 + (uint32_t)(xrc[j] >> 16), ix = ix0 + (uint32_t)((xrc[j] >> 8) & 255);
        const bool ok = live & (iy < (uint32_t)lh) & (ix < (uint32_t)lw);
        const uint32_t off = xt + ((iy >> upsh) * (uint32_t)a.in_w + (ix >> upsh)) * pxb + (uint32_t)((xrc[j] & 7) * 16);
        glds(xrs, ok ? off : BUF_OOB, zb + (uint32_t)(ZB + (wvu + 4 * j) * 1024));
      }
    };
    // fragment reads: k-step kk, lane (g, q, p) = output pixel c0 = 4 g + q of rows 2 kk (k0) and 2 kk + 1 (k1),
    // channels 4 p.. of the 16-channel group: dz group t (chunk 2 t + (p >> 1)), x group wave (chunk 2 wave + (p >> 1))
    const int c0 = 4 * g + q;
    int zoff[4], xoff[3];
#pragma unroll
    for (int t = 0; t < 4; ++t) zoff[t] = c0 * 128 + (((2 * t + (p >> 1)) ^ (c0 & 7)) << 4) + 8 * (p & 1);
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) xoff[dx] = (c0 + dx) * 128 + (((2 * wave + (p >> 1)) ^ ((c0 + dx) & 7)) << 4) + 8 * (p & 1);
    auto ld_af = [&](const char* zb, int kk, bf16x8 (&af)[4]) {
#pragma unroll
      for (int t = 0; t < 4; ++t) af[t] = cat_tr(ds_read_tr16(zb + kk * 32 * 128 + zoff[t]), ds_read_tr16(zb + (kk * 32 + 16) * 128 + zoff[t]));
    };
    auto ld_bf = [&](const char* xb, int kk, int u) {
      const int dy = u / 3, dx = u % 3;
      return cat_tr(ds_read_tr16(xb + (2 * kk + dy) * TPW * 128 + xoff[dx]), ds_read_tr16(xb + (2 * kk + 1 + dy) * TPW * 128 + xoff[dx]));
    };
    issue(tile < a.ntiles, 0);
    issue(tile + a.nsplit < a.ntiles, 1);
    int cur = 0;
    for (; tile < a.ntiles; tile += a.nsplit) {
      // this tile's 10 DMAs (per wave) have landed once at most the next tile's 10 are outstanding; the barrier makes
      // that true for every wave, and every wave is past its reads of the tile before last (buffer (cur + 2) % 3)
      asm volatile("s_waitcnt vmcnt(10)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      issue(tile + 2 * a.nsplit < a.ntiles, cur == 0 ? 2 : cur - 1);
      const char* zb = smem + cur * BUF;
      const char* xb = zb + ZB;
      // the 36 (k-step, tap) groups of 4 MFMAs read their x fragment from a 3-register ring loaded 2 groups ahead,
      // the next k-step's dz fragments half-way through the current one (one whole fragment set: 56 registers)
      bf16x8 af[2][4], bq[3];
      ld_af(zb, 0, af[0]);
      bq[0] = ld_bf(xb, 0, 0);
      bq[1] = ld_bf(xb, 0, 1);
#pragma unroll
      for (int gi = 0; gi < NK * 9; ++gi) {
        const int kk = gi / 9, u = gi % 9, gn = gi + 2;
        if (gn < NK * 9) bq[gn % 3] = ld_bf(xb, gn / 9, gn % 9);
        if (u == 4 && kk + 1 < NK) ld_af(zb, kk + 1, af[(kk + 1) & 1]);
        __builtin_amdgcn_sched_barrier(0);
        if (u == 0) {
#pragma unroll
          for (int t = 0; t < 4; ++t) accb[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[kk & 1][t], ones, accb[t], 0, 0, 0);
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t][u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[kk & 1][t], bq[gi % 3], acc[t][u], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
      cur = cur == 2 ? 0 : cur + 1;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the two DMAs past the last tile (zeros) land before the
                                                        // epilogue staging reuses the buffers
  } else {
  issue(tile < a.ntiles);
  if constexpr (TS == 1) {
    // double-buffered LDS, one barrier per tile: tile t+1 (in registers since tile t-1) is written to the other
    // buffer after the first k-step pair of tile t is on the MFMA pipe, then tile t+2 is requested -- the stash
    // no longer runs between two barriers with the MFMAs idle (one workgroup per CU: nothing else hid it).  The
    // stash and the request are unconditional (past the last tile they move zeros into the idle buffer): no branch
    // inside the tile loop, so the accumulators stay in place (the conditional form made hipcc copy all 144 of
    // them out of and back into the AGPRs every tile).  LDS-only barriers keep the register prefetch in flight.
    stash(0);
    issue(tile + a.nsplit < a.ntiles);
    lds_barrier();
    int cur = 0;
    for (; tile < a.ntiles; tile += a.nsplit) {
      bf16x8 afA[4], bfA[NU], afB[4], bfB[NU];
      frags(cur, 0, afA, bfA);
#pragma unroll
      for (int kk = 0; kk < NK; kk += 2) {
        frags(cur, kk + 1, afB, bfB);
        mma(afA, bfA);
        if (kk == 0) {
          stash(cur ^ 1);
          issue(tile + 2 * a.nsplit < a.ntiles);
        }
        if (kk + 2 < NK) frags(cur, kk + 2, afA, bfA);
        mma(afB, bfB);
      }
      lds_barrier();  // this tile's reads of buffer cur and the stash of buffer cur ^ 1 are done
      cur ^= 1;
    }
  } else {
    for (; tile < a.ntiles; tile += a.nsplit) {
      lds_barrier();  // previous tile's fragment reads done
      stash(0);
      issue(tile + a.nsplit < a.ntiles);
      lds_barrier();
      // two waves per SIMD (256 VGPRs each): one fragment set, the partner wave hides the latency
#pragma unroll 2
      for (int kk = 0; kk < NK; ++kk) {
        bf16x8 af[4], bf[NU];
        frags(0, kk, af, bf);
        mma(af, bf);
      }
    }
  }
  }
  // C[row = co][col = ci]: lane holds co = co0 + 16t + 4g + i, ci = ci0 + 16 wave + col.  The workgroup's slab block
  // (64 co rows x 576 contiguous floats each) is assembled in LDS and written with coalesced 16 B stores (the direct
  // form issued 144 scattered 4 B stores per lane, 36 B apart)
  constexpr int EPW = 9 * 64 + 4;  // staged row pitch (floats)
  float* st = (float*)smem;
  __syncthreads();  // every wave's fragment reads are done (the staging aliases the tiles)
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float* row = st + (t * 16 + g * 4 + i) * EPW + (wave * 16 + col) * 9;
#pragma unroll
      for (int u = 0; u < NU; ++u) {
        if constexpr (TS == 1) row[u] = acc[t][u][i];
        else if (u0 + u < 9) row[u0 + u] = acc[t][u][i];
      }
      if (do_bias && wave == 0 && tg == 0 && col == 0) a.bpart[(long)split * a.co_rows + co0 + t * 16 + g * 4 + i] = accb[t][i];
    }
  __syncthreads();
  float* slab = a.part + (long)split * a.co_rows * a.kw + (long)co0 * a.kw + ci0 * 9;
  for (int f = tid; f < 64 * 144; f += NTHR) {
    const int row = f / 144, c4 = f - row * 144;
    *(float4*)(slab + (long)row * a.kw + c4 * 4) = *(const float4*)(st + row * EPW + c4 * 4);
  }
}
constexpr size_t W64_EP_LDS = (size_t)64 * (9 * 64 + 4) * 4;  // the slab staging of conv_wgrad64_kernel
constexpr size_t W64G_LDS = (size_t)3 * (8 * 16 * 128 + 24 * 1024);  // three LDS-DMA tile buffers (G form)

template <int TS, int S = 1>
__global__ __launch_bounds__(256 * TS, 1) void conv_wgrad64_kernel(WgArgs a) {
  wgrad64_body<TS, S, false>(a);
}
// at most 256 registers (one workgroup per CU either way: 148 KB of LDS): the accumulators stay in VGPRs -- the
// 512-register form kept some of them in AGPRs and shuffled them every tile
__global__ __launch_bounds__(256, 2) void conv_wgrad64_glds_kernel(WgArgs a) { wgrad64_body<1, 1, true>(a); }

// ------------------------------------------------------------------------------------------
// Weight gradient of a 1x1 conv with 64 inputs and <= 64 outputs (srcnn.conv2): dW[co][ci] = sum_p dz[p][co]
// x[p][ci], db = sum_p dz.  One pass over the pixels: each workgroup owns a contiguous pixel range and ALL
// co x ci outputs (wave w = ci block w), 128-pixel chunks staged through LDS (next chunk prefetched into
// registers) and read back transposed (ds_read_tr16_b64) as pixel-major MFMA fragments.  The generic wgrad
// splits co x ci over workgroups that each re-read every pixel (1.6 GB fetched for 0.4 GB of data).
// ------------------------------------------------------------------------------------------
constexpr int WPT_CH = 128;

static bool wpt_shape(const ClimsrConvDesc* d) {
  return d->ks == 1 && d->stride == 1 && d->up == 1 && d->pad == 0 && d->in_c == 64 && d->out_c % 16 == 0 && d->out_c <= 64 &&
         d->out_h == d->in_h && d->out_w == d->in_w;
}

static int wpt_splits(const ClimsrConvDesc* d) {
  const long npix = (long)d->n * d->out_h * d->out_w;
  long ns = npix / (WPT_CH * 8);  // >= 8 chunks per workgroup
  if (ns > 512) ns = 512;
  return ns < 1 ? 1 : (int)ns;
}

template <int NCOF>
__global__ __launch_bounds__(256) void conv_wgrad_pt_kernel(WgArgs a) {
  constexpr int ZP = NCOF * 16 + 8, XP = 64 + 8;
  constexpr int NZV = WPT_CH * NCOF * 2 / 256, NXV = WPT_CH * 8 / 256;  // 16 B vectors per thread
  __shared__ __attribute__((aligned(16))) uint16_t zs[WPT_CH * ZP];
  __shared__ __attribute__((aligned(16))) uint16_t xs[WPT_CH * XP];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4;
  const int q = (lane & 15) >> 2, p = lane & 3, col = lane & 15;
  const long npix = (long)a.n * a.out_h * a.out_w;
  const long p0 = npix * blockIdx.x / gridDim.x, p1 = npix * (blockIdx.x + 1) / gridDim.x;
  const bool do_bias = a.bpart != nullptr && wave == 0;
  f32x4 acc[NCOF], accb[NCOF];
#pragma unroll
  for (int t = 0; t < NCOF; ++t) acc[t] = accb[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
  bf16x8 ones;
#pragma unroll
  for (int i = 0; i < 8; ++i) ones[i] = (__bf16)1.0f;
  uint4 pz[NZV], px[NXV];
  auto issue = [&](long c0) {
#pragma unroll
    for (int i = 0; i < NZV; ++i) {
      const int v = tid + 256 * i, pix = v / (NCOF * 2), cg = v % (NCOF * 2);
      const long pp = c0 + pix;
      pz[i] = pp < p1 ? *(const uint4*)(a.dz + pp * a.dz_cs + cg * 8) : make_uint4(0, 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < NXV; ++i) {
      const int v = tid + 256 * i, pix = v >> 3, cg = v & 7;
      const long pp = c0 + pix;
      px[i] = pp < p1 ? *(const uint4*)(a.x + pp * a.in_cs + a.in_co + cg * 8) : make_uint4(0, 0, 0, 0);
    }
  };
  if (p0 < p1) issue(p0);
  for (long c0 = p0; c0 < p1; c0 += WPT_CH) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NZV; ++i) {
      const int v = tid + 256 * i;
      *(uint4*)(zs + (v / (NCOF * 2)) * ZP + (v % (NCOF * 2)) * 8) = pz[i];
    }
#pragma unroll
    for (int i = 0; i < NXV; ++i) {
      const int v = tid + 256 * i;
      *(uint4*)(xs + (v >> 3) * XP + (v & 7) * 8) = px[i];
    }
    if (c0 + WPT_CH < p1) issue(c0 + WPT_CH);
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < WPT_CH / 32; ++kk) {
      const int k0 = kk * 32 + 8 * g + q, k1 = k0 + 4;
      const s16x4 blo = ds_read_tr16(xs + k0 * XP + wave * 16 + 4 * p), bhi = ds_read_tr16(xs + k1 * XP + wave * 16 + 4 * p);
      const short b8[8] = {blo[0], blo[1], blo[2], blo[3], bhi[0], bhi[1], bhi[2], bhi[3]};
      const bf16x8 b = __builtin_bit_cast(bf16x8, b8);
#pragma unroll
      for (int t = 0; t < NCOF; ++t) {
        const s16x4 lo = ds_read_tr16(zs + k0 * ZP + t * 16 + 4 * p), hi = ds_read_tr16(zs + k1 * ZP + t * 16 + 4 * p);
        const short v8[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        const bf16x8 af = __builtin_bit_cast(bf16x8, v8);
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, b, acc[t], 0, 0, 0);
        if (do_bias) accb[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, ones, accb[t], 0, 0, 0);
      }
    }
  }
  // D[co][ci]: lane holds co = 16t + 4g + i, ci = 16 wave + col
  float* slab = a.part + (long)blockIdx.x * a.co_rows * a.kw;
#pragma unroll
  for (int t = 0; t < NCOF; ++t)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int co = t * 16 + g * 4 + i;
      slab[(long)co * a.kw + wave * 16 + col] = acc[t][i];
      if (do_bias && col == 0) a.bpart[(long)blockIdx.x * a.co_rows + co] = accb[t][i];
    }
}

// ------------------------------------------------------------------------------------------
// Weight gradient of a single-output-channel conv (conv_last 64->1 3x3, srcnn.conv3 32->1 5x5).  The
// generic wgrad puts the one output channel in the MFMA M dimension (1 of 16 rows useful); here the
// horizontal taps take that role instead.  Per dz row y and input row iy = y + ky - R:
//     D_ky[kx][ci] += sum_x' dz[y][x' - kx] * X[iy][x'][ci]           (M = kx, N = ci, K = x')
// A = the dz row shifted by kx (a Toeplitz fragment: 8 consecutive dz values per lane, read 16 B-aligned
// from one of 8 pre-shifted LDS copies of the row), B = the input row transposed by ds_read_tr16_b64.
// A wave streams a segment of SEG dz rows of one 64-column strip; each staged input row feeds the KS
// dz rows it pairs with.  Block partials (4 waves summed in LDS) go to the wgrad_reduce layout
// part[split][16][in_c * ks^2] (row 0), bpart[split][16].
// ------------------------------------------------------------------------------------------
constexpr int WCO1_XT = 96, WCO1_DZL = 128;

static bool wco1_shape(const ClimsrConvDesc* d) {
  return d->out_c == 1 && d->stride == 1 && d->up == 1 && (d->ks == 3 || d->ks == 5) && d->pad == d->ks / 2 &&
         d->in_c % 16 == 0 && d->in_c <= 64 && d->out_h == d->in_h && d->out_w == d->in_w;
}

static int wco1_splits(const ClimsrConvDesc* d) {
  const long rows = (long)d->n * d->out_h * ceil_div(d->out_w, 64);
  long ns = rows / (4 * 8);  // >= 8 dz rows per wave
  if (ns > 512) ns = 512;
  return ns < 1 ? 1 : (int)ns;
}

template <int KS, int NCF>
__global__ __launch_bounds__(256, 2) void conv_wgrad_co1m_kernel(WgArgs a) {
  constexpr int R = KS / 2, CI = NCF * 16, XP = CI + 8, NV = ((64 + KS - 1) * (CI / 8) + 63) / 64;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, col = lane & 15;
  uint16_t* xs = (uint16_t*)smem + wave * (WCO1_XT * XP);                                   // [x'][ci]
  uint16_t* ring = (uint16_t*)smem + 4 * WCO1_XT * XP + wave * (KS * 8 * WCO1_DZL);         // [slot][copy][m]
  for (int i = lane; i < WCO1_XT * XP / 8; i += 64) ((uint4*)xs)[i] = make_uint4(0, 0, 0, 0);
  for (int i = lane; i < KS * 8 * WCO1_DZL / 8; i += 64) ((uint4*)ring)[i] = make_uint4(0, 0, 0, 0);

  f32x4 acc[KS][NCF];
#pragma unroll
  for (int k = 0; k < KS; ++k)
#pragma unroll
    for (int c = 0; c < NCF; ++c) acc[k][c] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float bsum = 0.f;

  const int nstrip = (a.out_w + 63) / 64;
  const int seg_rows = a.tph;  // dz rows per segment (host-chosen)
  const int nrs = (a.out_h + seg_rows - 1) / seg_rows;
  const long nseg = (long)a.n * nstrip * nrs;
  const int gw = blockIdx.x * 4 + wave, nw = gridDim.x * 4;
  for (long seg = gw; seg < nseg; seg += nw) {
    const int rs = (int)(seg % nrs);
    const int strip = (int)((seg / nrs) % nstrip);
    const int nimg = (int)(seg / ((long)nrs * nstrip));
    const int x0 = strip * 64, ya = rs * seg_rows, yb = min(a.out_h, ya + seg_rows);
    for (int iy = ya - R; iy < yb + R; ++iy) {
      // stage input row iy: x' in [0, 64 + KS - 1) <-> input column x0 - R + x'
      uint4 v[NV];
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int e = lane + 64 * i, xq = e / (CI / 8), cg = e % (CI / 8);
        const int ix = x0 - R + xq;
        v[i] = make_uint4(0, 0, 0, 0);
        if (xq < 64 + KS - 1 && iy >= 0 && iy < a.in_h && ix >= 0 && ix < a.in_w && cg * 8 < a.in_c)
          v[i] = *(const uint4*)(a.x + (((long)nimg * a.in_h + iy) * a.in_w + ix) * a.in_cs + a.in_co + cg * 8);
      }
      // the dz row paired with tap row 0 enters the ring: 8 copies, copy q holds D[m - 16 - q]
      const int ynew = iy + R;
      float dzv = 0.f;
      if (ynew >= ya && ynew < yb && x0 + lane < a.out_w)
        dzv = bf2f(a.dz[(((long)nimg * a.out_h + ynew) * a.out_w + x0 + lane) * a.dz_cs]);
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int e = lane + 64 * i, xq = e / (CI / 8), cg = e % (CI / 8);
        if (xq < 64 + KS - 1) *(uint4*)(xs + xq * XP + cg * 8) = v[i];
      }
      if (ynew >= ya && ynew < yb) {
        bsum += dzv;
        uint16_t* slot = ring + (ynew % KS) * (8 * WCO1_DZL);
        const uint16_t b = f2bf(dzv);
#pragma unroll
        for (int q = 0; q < 8; ++q) slot[q * WCO1_DZL + lane + 16 + q] = b;
      }
      // B fragments of this input row (x' = 32 s + 8 g + j, ci = 16 c + col), shared by every tap row
      bf16x8 bx[3][NCF];
#pragma unroll
      for (int st = 0; st < 3; ++st)
#pragma unroll
        for (int c = 0; c < NCF; ++c) {
          const uint16_t* p0 = xs + (st * 32 + g * 8 + (col >> 2)) * XP + c * 16 + (col & 3) * 4;
          const s16x4 lo = ds_read_tr16(p0), hi = ds_read_tr16(p0 + 4 * XP);
          bx[st][c] = __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
        }
#pragma unroll
      for (int ky = 0; ky < KS; ++ky) {
        const int y = iy - ky + R;
        if (y < ya || y >= yb) continue;
        const uint16_t* slot = ring + (y % KS) * (8 * WCO1_DZL);
#pragma unroll
        for (int st = 0; st < 3; ++st) {
          const int aoff = st * 32 + g * 8 - col;  // D index of element j = 0 (lane's kx = col)
          const int q = (-aoff) & 7;
          bf16x8 at = *(const bf16x8*)(slot + q * WCO1_DZL + aoff + 16 + q);
          if (col >= KS) at = (bf16x8){};
#pragma unroll
          for (int c = 0; c < NCF; ++c) acc[ky][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(at, bx[st][c], acc[ky][c], 0, 0, 0);
        }
      }
    }
    // the next segment rewrites every ring position it reads (rows outside [ya, yb) are skipped)
  }
  // block reduction: C[kx = 4g + i][ci = 16c + col] of tap row ky
  for (int o = 32; o > 0; o >>= 1) bsum += __shfl_down(bsum, o);
  __syncthreads();
  float* red = (float*)smem;  // [wave][ky][c][lane][4]
#pragma unroll
  for (int ky = 0; ky < KS; ++ky)
#pragma unroll
    for (int c = 0; c < NCF; ++c) *(f32x4*)(red + (((wave * KS + ky) * NCF + c) * 64 + lane) * 4) = acc[ky][c];
  __shared__ float bred[4];
  if (lane == 0) bred[wave] = bsum;
  __syncthreads();
  const int ks2 = KS * KS;
  float* part = a.part + (long)blockIdx.x * 16 * a.kw;
  constexpr int PER = KS * NCF * 64 * 4;
  for (int e = tid; e < PER; e += 256) {
    const int i = e & 3, ln = (e >> 2) & 63, c = (e >> 8) % NCF, ky = (e >> 8) / NCF;
    const int kx = (ln >> 4) * 4 + i, ci = c * 16 + (ln & 15);
    if (kx >= KS || ci >= a.in_c) continue;
    const float t = red[e] + red[e + PER] + red[e + 2 * PER] + red[e + 3 * PER];
    part[ci * ks2 + ky * KS + kx] = t;
  }
  if (tid == 0 && a.bpart) a.bpart[blockIdx.x * 16] = bred[0] + bred[1] + bred[2] + bred[3];
}

template <int KS, int NCF>
static int launch_wco1(const WgArgs& a, hipStream_t s) {
  auto k = conv_wgrad_co1m_kernel<KS, NCF>;  // (+16 B of static LDS: the dynamic cap leaves room for it)
  const size_t lds_x = (size_t)4 * WCO1_XT * (NCF * 16 + 8) * 2 + (size_t)4 * KS * 8 * WCO1_DZL * 2;
  const size_t lds_r = (size_t)4 * KS * NCF * 64 * 16;
  const size_t lds = lds_x > lds_r ? lds_x : lds_r;
  if (int e = lds_opt_in((const void*)k, 159 * 1024)) return e;
  hipLaunchKernelGGL(k, dim3(a.nsplit), dim3(256), lds, s, a);
  return check_launch("conv2d_wgrad (co1m)");
}

static bool w64_shape(const ClimsrConvDesc* d) {
  return d->ks == 3 && d->pad == 1 && d->out_c % 64 == 0 && d->in_c % 64 == 0 && d->in_c >= 64 &&
         (d->stride == 1 || (d->stride == 2 && d->up == 1));
}
static int w64_th(const ClimsrConvDesc* d) { return d->stride == 2 ? W64<2>::TH : W64<1>::TH; }

struct WgPlan {
  int ntc, tb, ntapb, ncib, ncob, co_rows, tiles_x, tiles_y, ntiles, tph, tpw, dzp, kw, ci4;
  size_t lds_x, lds_z, lds_total;
};

static void wg_plan(const ClimsrConvDesc* d, WgPlan* w) {
  int rows = round_up(d->out_c, 16);
  w->ntc = rows >= 64 ? 4 : (rows >= 32 ? 2 : 1);
  int ks2 = d->ks * d->ks;
  w->ci4 = d->in_c == 4;  // <= 4 real input channels: 4 taps x 4 channels per fragment
  if (w->ci4) {
    int groups = ceil_div(ks2, 4);
    w->tb = groups <= 3 ? 3 : 7;
    w->ntapb = ceil_div(groups, w->tb);
    w->ncib = 1;
  } else {
    w->tb = ks2 >= 9 ? 9 : (ks2 >= 5 ? 5 : 1);
    if (ks2 == 25) w->tb = 5;
    w->ntapb = ceil_div(ks2, w->tb);
    w->ncib = ceil_div(d->in_c, 16);
  }
  w->ncob = ceil_div(rows, w->ntc * 16);
  w->co_rows = w->ncob * w->ntc * 16;
  w->tiles_x = ceil_div(d->out_w, TW);
  w->tiles_y = ceil_div(d->out_h, WG_TH);
  w->ntiles = d->n * w->tiles_x * w->tiles_y;
  w->tph = (WG_TH - 1) * d->stride + d->ks;
  w->tpw = (TW - 1) * d->stride + d->ks;
  w->dzp = w->ntc * 16 + 8;
  w->kw = d->in_c * ks2;
  w->lds_x = (size_t)w->tph * w->tpw * (w->ci4 ? 4 : WG_XP) * 2;
  w->lds_x = (w->lds_x + 15) / 16 * 16;
  w->lds_z = (size_t)WG_TH * TW * w->dzp * 2;
  size_t red = (size_t)(w->ntc * w->tb + w->ntc) * 64 * 16;
  w->lds_total = w->lds_x + w->lds_z;
  if (red > w->lds_total) w->lds_total = red;
}

// The route of a weight gradient: the kernel kind with its template ids, the plan (co_rows / kw = the partial slabs'
// layout for every kind; the tiling for the generic kinds) and the split count climsr_conv2d_wgrad_splits reports.
enum WgKind { WG_PT, WG_CO1M, WG_W64_GLDS, WG_W64_TS, WG_W64_S2, WG_GENERIC, WG_WAVE_SPLIT };

struct WgRoute {
  int kind;
  int ks, ncf;  // WG_CO1M <KS, NCF>; WG_PT <ncf>
  WgPlan w;
  int splits;
};

static WgRoute wg_route(const ClimsrConvDesc* d) {
  WgRoute r{};
  WgPlan& w = r.w;
  wg_plan(d, &w);
  if (wpt_shape(d)) {  // co_rows = out_c rounded to its 16/32/64 tile (wg_plan), kw = in_c
    r.kind = WG_PT; r.ncf = d->out_c / 16 < 4 ? d->out_c / 16 : 4;
    w.kw = d->in_c; r.splits = wpt_splits(d);
  } else if (wco1_shape(d)) {
    r.kind = WG_CO1M; r.ks = d->ks; r.ncf = d->in_c / 16;
    w.co_rows = 16; r.splits = wco1_splits(d);
  } else if (w64_shape(d)) {
    // 8 waves (tap-split) pay off on the large-pixel-count convs (HRconv / upconv at 256^2: +8 %) and lose on the
    // 64^2 dense-block GEMM (-19 %), measured with tools/perf_conv.py
    const bool ts2 = d->stride == 1 && (long)d->n * d->out_h * d->out_w >= (1L << 20);
    r.kind = d->stride == 2 ? WG_W64_S2 : ts2 ? WG_W64_TS : WG_W64_GLDS;
    w.co_rows = d->out_c;
    w.tiles_y = ceil_div(d->out_h, w64_th(d));
    w.ntiles = d->n * w.tiles_x * w.tiles_y;
    // one workgroup per CU: 256 / blocks splits
    int blocks = (d->out_c / 64) * (d->in_c / 64);
    int ns = ceil_div(256, blocks);
    if (ns > w.ntiles) ns = w.ntiles;
    r.splits = ns < 1 ? 1 : ns;
  } else {
    // <= 4 real input channels, 9x9, one 64-row block: all 21 tap groups per workgroup, 6 per wave
    const bool ws = w.ci4 && d->ks == 9 && w.ncob == 1 && w.ntc == 4 && d->stride == 1;
    r.kind = ws ? WG_WAVE_SPLIT : WG_GENERIC;
    int ns = ceil_div(512, ws ? 1 : w.ntapb * w.ncib * w.ncob);
    if (ns > w.ntiles) ns = w.ntiles;
    r.splits = ns < 1 ? 1 : ns;
  }
  return r;
}

extern "C" int climsr_conv2d_wgrad_splits(const ClimsrConvDesc* d) { return wg_route(d).splits; }

extern "C" size_t climsr_conv2d_wgrad_workspace(const ClimsrConvDesc* d, int nsplit) {
  const WgPlan w = wg_route(d).w;
  return (size_t)nsplit * w.co_rows * w.kw + (size_t)nsplit * w.co_rows;
}

// what climsr_conv2d_wgrad refuses of (d, dz_cstride) on route r
static int wg_check(const ClimsrConvDesc* d, int dz_cstride, const WgRoute& r) {
  if ((d->in_c % 8 && d->in_c != 4) || d->in_cstride % 8 || d->in_coff % 8 || dz_cstride % 8 || (d->up != 1 && d->up != 2) ||
      (d->stride != 1 && d->stride != 2)) {
    set_error("conv2d_wgrad: bad args");
    return CLIMSR_EINVAL;
  }
  const bool w64 = r.kind == WG_W64_GLDS || r.kind == WG_W64_TS || r.kind == WG_W64_S2;
  if (w64 && ((long)d->n * d->in_h * d->in_w * d->in_cstride * 2 >= (1L << 31) ||
              (long)d->n * d->out_h * d->out_w * dz_cstride * 2 >= (1L << 31))) {  // 32-bit buffer offsets (BUF_OOB)
    set_error("conv2d_wgrad: operands over 2 GiB (split the batch)");
    return CLIMSR_EINVAL;
  }
  if ((r.kind == WG_GENERIC || r.kind == WG_WAVE_SPLIT) && r.w.lds_total > 160 * 1024) {
    set_error("conv2d_wgrad: LDS %zu too large", r.w.lds_total);
    return CLIMSR_EINVAL;
  }
  return CLIMSR_OK;
}

template <int NTC, int TB, int CI4>
static int launch_wg(const WgArgs& a, int nblk, size_t lds, hipStream_t s) {
  auto k = conv_wgrad_kernel<NTC, TB, CI4>;
  if (int e = lds_opt_in((const void*)k, 160 * 1024)) return e;
  hipLaunchKernelGGL(k, dim3(nblk, a.nsplit), dim3(256), lds, s, a);
  return check_launch("conv2d_wgrad");
}

extern "C" int climsr_conv2d_wgrad(const ClimsrConvDesc* d, const uint16_t* x, const uint16_t* dz, int dz_cstride, float* partial,
                                   float* bias_partial, int nsplit, void* stream) {
  if (!d || !x || !dz || !partial || nsplit <= 0) {
    set_error("conv2d_wgrad: bad args");
    return CLIMSR_EINVAL;
  }
  const WgRoute r = wg_route(d);
  const WgPlan& w = r.w;
  if (int e = wg_check(d, dz_cstride, r)) return e;
  hipStream_t s = (hipStream_t)stream;
  WgArgs a{};
  a.x = x; a.dz = dz; a.part = partial; a.bpart = bias_partial;
  a.n = d->n; a.in_c = d->in_c; a.in_cs = d->in_cstride; a.in_co = d->in_coff; a.out_h = d->out_h; a.out_w = d->out_w;
  a.out_c = d->out_c; a.dz_cs = dz_cstride; a.nsplit = nsplit; a.kw = w.kw; a.co_rows = w.co_rows;
  if (r.kind == WG_PT) {
    switch (r.ncf) {
      case 1: hipLaunchKernelGGL(conv_wgrad_pt_kernel<1>, dim3(nsplit), dim3(256), 0, s, a); break;
      case 2: hipLaunchKernelGGL(conv_wgrad_pt_kernel<2>, dim3(nsplit), dim3(256), 0, s, a); break;
      case 3: hipLaunchKernelGGL(conv_wgrad_pt_kernel<3>, dim3(nsplit), dim3(256), 0, s, a); break;
      default: hipLaunchKernelGGL(conv_wgrad_pt_kernel<4>, dim3(nsplit), dim3(256), 0, s, a); break;
    }
    return check_launch("conv2d_wgrad (1x1)");
  }
  a.in_h = d->in_h; a.in_w = d->in_w; a.ks = d->ks; a.pad = d->pad;
  if (r.kind == WG_CO1M) {
    a.out_c = 1;
    const long rows = (long)d->n * d->out_h * ceil_div(d->out_w, 64);
    a.tph = ceil_div(rows, (long)nsplit * 4);  // dz rows per wave segment (~one segment per wave)
    if (a.tph < 4) a.tph = 4;
    if (a.tph > d->out_h) a.tph = d->out_h;
#define WCO1_CASE(KS, NCF) \
  if (r.ks == KS && r.ncf == NCF) return launch_wco1<KS, NCF>(a, s);
    WCO1_CASE(3, 1) WCO1_CASE(3, 2) WCO1_CASE(3, 3) WCO1_CASE(3, 4) WCO1_CASE(5, 1) WCO1_CASE(5, 2) WCO1_CASE(5, 3)
#undef WCO1_CASE
    return launch_wco1<5, 4>(a, s);
  }
  a.up = d->up; a.stride = d->stride;
  a.tiles_x = w.tiles_x; a.tiles_y = w.tiles_y; a.ntiles = w.ntiles;
  if (r.kind == WG_W64_GLDS || r.kind == WG_W64_TS || r.kind == WG_W64_S2) {
    a.ks = 3; a.pad = 1;
    a.ncib = d->in_c / 64;
    a.dzp = W64_P; a.ntapb = 1; a.lds_x = 0;
    a.xcd = 1;
    const dim3 grid = dim3((d->out_c / 64) * (d->in_c / 64) * nsplit);
    const bool s2 = r.kind == WG_W64_S2, ts = r.kind == WG_W64_TS;
    a.tph = s2 ? W64<2>::TPH : W64<1>::TPH; a.tpw = s2 ? W64<2>::TPW : W64<1>::TPW;
    void (*k)(WgArgs) = s2 ? conv_wgrad64_kernel<1, 2> : ts ? conv_wgrad64_kernel<2, 1> : conv_wgrad64_glds_kernel;
    const size_t lds = std::max(s2 ? 2 * W64<2>::LDS : ts ? W64<1>::LDS : W64G_LDS, W64_EP_LDS);
    if (int e = lds_opt_in((const void*)k, 160 * 1024)) return e;
    hipLaunchKernelGGL(k, grid, dim3(ts ? 512 : 256), lds, s, a);
    return check_launch("conv2d_wgrad (64x64 block)");
  }
  a.tph = w.tph; a.tpw = w.tpw; a.dzp = w.dzp;
  a.ntapb = w.ntapb; a.ncib = w.ncib;
  a.lds_x = (int)w.lds_x;
  int nblk = w.ntapb * w.ncib * w.ncob;
  if (r.kind == WG_WAVE_SPLIT) {
    a.ntapb = 1;
    auto k = conv_wgrad_kernel<4, 6, 1, true>;
    if (int e = lds_opt_in((const void*)k, 160 * 1024)) return e;
    hipLaunchKernelGGL(k, dim3(1, nsplit), dim3(256), w.lds_total, s, a);
    return check_launch("conv2d_wgrad (ci4, wave-split taps)");
  }
#define WG_CASE(NTC, TB, CI4) \
  if (w.ntc == NTC && w.tb == TB && w.ci4 == CI4) return launch_wg<NTC, TB, CI4>(a, nblk, w.lds_total, s);
  WG_CASE(1, 1, 0) WG_CASE(2, 1, 0) WG_CASE(4, 1, 0)
  WG_CASE(1, 5, 0) WG_CASE(2, 5, 0) WG_CASE(4, 5, 0)
  WG_CASE(1, 9, 0) WG_CASE(2, 9, 0) WG_CASE(4, 9, 0)
  WG_CASE(1, 3, 1) WG_CASE(2, 3, 1) WG_CASE(4, 3, 1)
  WG_CASE(1, 7, 1) WG_CASE(2, 7, 1) WG_CASE(4, 7, 1)
#undef WG_CASE
  set_error("conv2d_wgrad: no kernel for ntc=%d tb=%d", w.ntc, w.tb);
  return CLIMSR_EINVAL;
}

extern "C" const char* climsr_conv2d_wgrad_kernel(const ClimsrConvDesc* d) {
  static thread_local char name[96];
  name[0] = 0;
  if (!d) {
    set_error("conv2d_wgrad: bad args");
    return name;
  }
  const WgRoute r = wg_route(d);
  if (wg_check(d, 8, r) != CLIMSR_OK) return name;
  const char* w64[] = {"conv_wgrad64_glds_kernel", "conv_wgrad64_kernel<2, 1>", "conv_wgrad64_kernel<1, 2>"};
  if (r.kind == WG_PT) snprintf(name, sizeof(name), "conv_wgrad_pt_kernel<%d>", r.ncf);
  else if (r.kind == WG_CO1M) snprintf(name, sizeof(name), "conv_wgrad_co1m_kernel<%d, %d>", r.ks, r.ncf);
  else if (r.kind <= WG_W64_S2) snprintf(name, sizeof(name), "%s", w64[r.kind - WG_W64_GLDS]);
  else if (r.kind == WG_WAVE_SPLIT) snprintf(name, sizeof(name), "conv_wgrad_kernel<4, 6, 1, true>");
  else snprintf(name, sizeof(name), "conv_wgrad_kernel<%d, %d, %d, false>", r.w.ntc, r.w.tb, r.w.ci4);
  return name;
}

// 256 threads = 32 consecutive outputs x 8 split groups (8 independent load chains per output,
// coalesced 128 B rows), combined in a fixed order through LDS: deterministic.
// Split group sg's share of the nsplit partials (sg, sg+8, ...): 4 independent chains so the loads are in flight
// together (one chain waited for each load in turn), combined in a fixed order.
__device__ __forceinline__ float sum_splits(const float* src, long sstride, int sg, int nsplit) {
  float a4[4] = {0.f, 0.f, 0.f, 0.f};
  int sp = sg;
  for (; sp + 24 < nsplit; sp += 32) {
#pragma unroll
    for (int u = 0; u < 4; ++u) a4[u] += src[(long)(sp + 8 * u) * sstride];
  }
  for (; sp < nsplit; sp += 8) a4[0] += src[(long)sp * sstride];
  return (a4[0] + a4[1]) + (a4[2] + a4[3]);
}

__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ part, const float* __restrict__ bpart,
                                                          int nsplit, int out_c, int in_c_real, int in_c, int ks2, int co_rows,
                                                          int kw, float* __restrict__ wg, float* __restrict__ bg, int accumulate) {
  __shared__ float red[8][33];
  const int lane = threadIdx.x & 31;
  const int sg = threadIdx.x >> 5;
  long idx = (long)blockIdx.x * 32 + lane;
  long nw = (long)out_c * in_c_real * ks2;
  long total = nw + (bg ? out_c : 0);
  const float* src = nullptr;
  long sstride = 0;
  if (idx < nw) {
    int co = (int)(idx / ((long)in_c_real * ks2));
    int rem = (int)(idx % ((long)in_c_real * ks2));  // ci*ks2 + tap
    src = part + (long)co * kw + rem;
    sstride = (long)co_rows * kw;
  } else if (idx < total) {
    src = bpart + (idx - nw);
    sstride = co_rows;
  }
  red[sg][lane] = src ? sum_splits(src, sstride, sg, nsplit) : 0.f;
  __syncthreads();
  if (sg == 0 && idx < total) {
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) t += red[i][lane];
    float* dst = (idx < nw) ? (wg + idx) : (bg + (idx - nw));
    if (accumulate) *dst += t;
    else *dst = t;
  }
}

// Row-sliced reduction of one wgrad partial matrix into several convs' OIHW gradients (the combined
// residual-dense-block weight gradient: rows [row0, row0 + out_c) of the [co_rows][kw] partial are conv
// d->wgrad's output channels, the first in_c_real*ks2 columns of each row its inputs x taps).
__global__ __launch_bounds__(256) void wgrad_reduce_rows_kernel(const float* __restrict__ part, const float* __restrict__ bpart,
                                                               int nsplit, int co_rows, int kw, int ks2,
                                                               const ClimsrReduceDesc* __restrict__ descs, int accumulate) {
  __shared__ float red[8][33];
  const ClimsrReduceDesc d = descs[blockIdx.y];
  const int lane = threadIdx.x & 31;
  const int sg = threadIdx.x >> 5;
  const long idx = (long)blockIdx.x * 32 + lane;
  const long nw = (long)d.out_c * d.in_c_real * ks2;
  const long total = nw + (d.bias_grad ? d.out_c : 0);
  if ((long)blockIdx.x * 32 >= total) return;
  const float* src = nullptr;
  long sstride = 0;
  if (idx < nw) {
    const int co = (int)(idx / ((long)d.in_c_real * ks2));
    const int rem = (int)(idx % ((long)d.in_c_real * ks2));
    src = part + (long)(d.row0 + co) * kw + rem;
    sstride = (long)co_rows * kw;
  } else if (idx < total) {
    src = bpart + d.row0 + (idx - nw);
    sstride = co_rows;
  }
  red[sg][lane] = src ? sum_splits(src, sstride, sg, nsplit) : 0.f;
  __syncthreads();
  if (sg == 0 && idx < total) {
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) t += red[i][lane];
    float* dst = (idx < nw) ? (d.wgrad + idx) : (d.bias_grad + (idx - nw));
    if (accumulate) *dst += t;
    else *dst = t;
  }
}

extern "C" int climsr_conv2d_wgrad_reduce_rows(const float* partial, const float* bias_partial, int nsplit, int co_rows, int kw,
                                               int ks, const ClimsrReduceDesc* descs, int ndesc, int64_t max_elems,
                                               int accumulate, void* stream) {
  if (!partial || !descs || nsplit <= 0 || ndesc <= 0 || ndesc > 65535 || ks <= 0) {
    set_error("conv2d_wgrad_reduce_rows: bad args");
    return CLIMSR_EINVAL;
  }
  hipLaunchKernelGGL(wgrad_reduce_rows_kernel, dim3(ceil_div(max_elems, 32), ndesc), dim3(256), 0, (hipStream_t)stream, partial,
                     bias_partial, nsplit, co_rows, kw, ks * ks, descs, accumulate);
  return check_launch("conv2d_wgrad_reduce_rows");
}

extern "C" int climsr_conv2d_wgrad_reduce(const float* partial, const float* bias_partial, int nsplit, int out_c, int in_c_real,
                                          int in_c, int ks, float* wgrad, float* bias_grad, int accumulate, void* stream) {
  if (!partial || !wgrad || nsplit <= 0) {
    set_error("conv2d_wgrad_reduce: bad args");
    return CLIMSR_EINVAL;
  }
  int rows = round_up(out_c, 16);
  int ntc = rows >= 64 ? 4 : (rows >= 32 ? 2 : 1);
  int co_rows = ceil_div(rows, ntc * 16) * ntc * 16;
  int ks2 = ks * ks;
  int kw = in_c * ks2;
  long total = (long)out_c * in_c_real * ks2 + (bias_grad ? out_c : 0);
  hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(ceil_div(total, 32)), dim3(256), 0, (hipStream_t)stream, partial, bias_partial,
                     nsplit, out_c, in_c_real, in_c, ks2, co_rows, kw, wgrad, bias_grad, accumulate);
  return check_launch("conv2d_wgrad_reduce");
}
