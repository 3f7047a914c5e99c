// Implicit-GEMM convolution for CDNA4 (gfx950), the host side of forward / data-gradient: errors and launch plumbing,
// geometry, weight packing (the only device code here) and the dispatch (fwd_route, climsr_conv2d_fwd).  The kernels are
// in the units conv_route.h lists; the weight gradients are in conv_wgrad.hip.
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

// Convs with <= 16 outputs, 3x3 and <= 128 inputs (the residual dense block's conv1-4 and their pull data
// gradients) run on conv_n16_kernel, whose packed K is tap-major with the channels padded to 32 per tap.
static bool n16_shape(int in_c, int ks, int out_c) { return out_c <= 16 && ks == 3 && in_c <= 128; }

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
// The shapes the families take (their kernels: conv_small.hip, conv_dma.hip)
// ------------------------------------------------------------------------------------------
// conv_co1m_kernel: one output channel, the horizontal taps in the MFMA N dimension
static bool co1m_shape(const ClimsrConvDesc* d) {
  return d->out_c == 1 && d->stride == 1 && d->up == 1 && (d->ks == 3 || d->ks == 5 || d->ks == 9) && d->pad == d->ks / 2 &&
         d->in_c <= 64 && d->in_c % 8 == 0 && d->cc % 8 == 0 && d->out_h == d->in_h && d->out_w == d->in_w;
}

// conv_pt_kernel: 1x1 as a streaming GEMM
static bool pt_shape(const ClimsrConvDesc* d, const ClimsrEpilogue* ep) {
  return d->ks == 1 && d->stride == 1 && d->up == 1 && d->pad == 0 && !ep->down2 && d->in_c % 32 == 0 && d->in_c <= 128 &&
         d->cc == d->in_c && d->out_c % 16 == 0 && d->out_c <= 64 && d->out_h == d->in_h && d->out_w == d->in_w &&
         ((d->out_cstride | d->out_coff) & 3) == 0 && (!ep->res1 || ((ep->res1_cstride | ep->res1_coff) & 3) == 0) &&
         (!ep->res2 || ((ep->res2_cstride | ep->res2_coff) & 3) == 0);
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
  // the max-pool epilogue (down2 == 2, fwd_route has checked its operands) is EP 3's conv: picked as that one, then
  // EP 11 where the LDS-DMA kernel takes it; left on any other kernel, fwd_route refuses it
  const bool pool = ep->down2 == 2;
  ClimsrEpilogue unpooled = *ep;
  unpooled.down2 = 0;
  const int plain = plain_ep(d, bias, pool ? &unpooled : ep);
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
    // pooled: whole 64-channel blocks only (the direct epilogues store all 64 channels of a block)
    const bool pooled = pool && r->ep == 3 && ep->act == 2 && d->out_c % 64 == 0;
    if (r->ep != 1 && r->ep != 2 && (!ep->down2 || pooled) && fits) {
      if (pooled) r->ep = 11;
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
  if (ep->down2 == 2) {  // bias + ReLU + 2x2 max-pool, only the pooled bf16 map stored (an inference-only forward)
    if (ep->act != 2 || !bias) {
      set_error("conv2d_fwd: max-pool epilogue (down2 = 2) needs a bias and ReLU (act 2), got act %d%s", ep->act, bias ? "" : ", no bias");
      return CLIMSR_EINVAL;
    }
    if (ep->out_mode != 0) {
      set_error("conv2d_fwd: max-pool epilogue (down2 = 2) stores bf16 only (out_mode %d)", ep->out_mode);
      return CLIMSR_EINVAL;
    }
    if (ep->res1 || ep->res2 || ep->res_f32 || ep->aux || ep->bn_part || ep->ch_part) {
      set_error("conv2d_fwd: max-pool epilogue (down2 = 2) takes no residual, aux output, BatchNorm partials or channel sums");
      return CLIMSR_EINVAL;
    }
    if ((d->out_h & 1) || (d->out_w & 1) || d->up != 1 || d->stride != 1) {
      set_error("conv2d_fwd: max-pool epilogue (down2 = 2) needs an even output size (%d x %d), up 1 and stride 1 (up %d, stride %d)",
                d->out_h, d->out_w, d->up, d->stride);
      return CLIMSR_EINVAL;
    }
  }
  if (ep->down2 && ep->down2 != 2 && (ep->res2 || ep->res_f32 || bias || ep->act == 1 || ep->act == 2 || (ep->res1 && ep->act < 3) ||
                    (d->out_h & 1) || (d->out_w & 1))) {
    set_error("conv2d_fwd: down2 epilogue: no bias / forward activation / residual (act 3/4 mask only), even output size");
    return CLIMSR_EINVAL;
  }
  if (ep->act < 0 || ep->act > 4 || ((ep->act == 3 || ep->act == 4) && !ep->res1)) {
    set_error("conv2d_fwd: act %d invalid (3/4 need res1 = the activation output)", ep->act);
    return CLIMSR_EINVAL;
  }
  const int pick = fwd_pick(d, bias, ep, r);
  if (ep->down2 == 2 && !(pick == PICK_OK && ((r->family == FAM_WR && r->ep == 5) || (r->family == FAM_DMA && r->ep == 11)))) {
    set_error("conv2d_fwd: max-pool epilogue (down2 = 2) only from the 64 -> 64 register-resident conv and the LDS-DMA conv "
              "(climsr_conv2d_fwd_kernel names the kernel, or nothing); run the conv and climsr_maxpool2_bf16 instead");
    return CLIMSR_EINVAL;
  }
  if (ep->ch_part &&!(pick == PICK_OK && r->family == FAM_WR && (r->ep == 3 || r->ep == 4))) {
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
    case FAM_DGRAD_S2: return fwd_dgrad_s2_launch(r, a, s);
    case FAM_FWD_S2: {
      const int rc = fwd_s2_dma_launch(a, s);
      return rc == CLIMSR_OK ? check_launch("conv2d_fwd (s2 LDS-DMA)") : rc;
    }
    case FAM_FWD:
    case FAM_DMA: return fwd_generic_launch(r, a, s);
    default: return fwd_small_launch(r, a, s);
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
