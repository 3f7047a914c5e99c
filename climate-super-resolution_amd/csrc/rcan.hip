// RCAN pieces that are not convolutions (climsr/models/rcan.py):
//  * channel attention of an RCAB (CALayer, rcan.py:50-69): global average pool -> 1x1 conv -> ReLU ->
//    1x1 conv -> sigmoid -> x * y, and the block residual (RCAB.forward, rcan.py:104-107) fused with the
//    scaling into one pass that also emits the bf16 copy the next conv reads;
//  * nn.PixelShuffle(r) of the Upsampler (rcan.py:17-47) on NHWC bf16: a pure index map, bit-exact.
// All HBM-bound elementwise / reduction work: 16 B per lane where the layout allows, deterministic
// fixed-order reductions.
#include "common.h"

using namespace climsr;

namespace {
constexpr int POOL_SPLIT = 256;  // pixel slices per image of the pooling pass (>= 1 block per CU for one grid)
}

// part[n][split][c] = sum over the split's pixels of x[n][p][c] (fp32 NHWC, cstride).  A block is
// (c/4 float4 lanes) x (256 / (c/4) pixel lanes); fp32 per-thread sums, fp64 across the block.
__global__ __launch_bounds__(256) void channel_sum_partial_kernel(const float* __restrict__ x, long hw, int c, int cs,
                                                                  double* __restrict__ part) {
  const int nimg = blockIdx.y, sp = blockIdx.x;
  const long p0 = hw * sp / POOL_SPLIT, p1 = hw * (sp + 1) / POOL_SPLIT;
  __shared__ double sh[256 * 4];
  const int cg = c / 4;  // host guarantees c % 4 == 0, cs % 4 == 0, cg <= 256
  const int plan = 256 / cg;
  const int g = threadIdx.x % cg, pl = threadIdx.x / cg;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  if (pl < plan)
    for (long p = p0 + pl; p < p1; p += plan) {
      const float4 v = *(const float4*)(x + ((long)nimg * hw + p) * cs + g * 4);
      acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    }
  sh[threadIdx.x * 4 + 0] = acc.x;
  sh[threadIdx.x * 4 + 1] = acc.y;
  sh[threadIdx.x * 4 + 2] = acc.z;
  sh[threadIdx.x * 4 + 3] = acc.w;
  __syncthreads();
  for (int ch = threadIdx.x; ch < c; ch += 256) {
    const int gg = ch / 4, q = ch % 4;
    double t = 0.0;
    for (int k = 0; k < plan; ++k) t += sh[(k * cg + gg) * 4 + q];
    part[((long)nimg * POOL_SPLIT + sp) * c + ch] = t;
  }
}

// s[n][c] = sigmoid(W2 relu(W1 mean + b1) + b2)  (conv_du of CALayer on the pooled [n, c, 1, 1] map)
__global__ __launch_bounds__(1024) void ca_mlp_kernel(const double* __restrict__ part, long hw, int c, int cr, const float* __restrict__ w1,
                              const float* __restrict__ b1, const float* __restrict__ w2, const float* __restrict__ b2,
                              float* __restrict__ s, float* __restrict__ mean_out) {
  extern __shared__ float sm[];
  float* mean = sm;      // [c]
  float* hid = sm + c;   // [cr]
  constexpr int NT = 1024;
  __shared__ double grp[NT];
  const int nimg = blockIdx.x;
  const int cw = c < NT ? c : NT;  // channels per round
  const int G = NT / cw;           // split groups summed in parallel, then combined in a fixed order
  for (int c0 = 0; c0 < c; c0 += cw) {
    const int i = c0 + (int)threadIdx.x % cw, gi = (int)threadIdx.x / cw;
    double t = 0.0;
    if (i < c && gi < G)
      for (int sp = gi; sp < POOL_SPLIT; sp += G) t += part[((long)nimg * POOL_SPLIT + sp) * c + i];
    grp[threadIdx.x] = t;
    __syncthreads();
    if ((int)threadIdx.x < cw && c0 + (int)threadIdx.x < c) {
      double m = 0.0;
      for (int k = 0; k < G; ++k) m += grp[k * cw + threadIdx.x];
      const float mf = (float)(m / (double)hw);
      mean[c0 + threadIdx.x] = mf;
      if (mean_out) mean_out[(long)nimg * c + c0 + threadIdx.x] = mf;  // kept for the backward (training forward)
    }
    __syncthreads();
  }
  for (int j = threadIdx.x; j < cr; j += blockDim.x) {
    float t = b1 ? b1[j] : 0.f;
    for (int i = 0; i < c; ++i) t += w1[j * c + i] * mean[i];
    hid[j] = t > 0.f ? t : 0.f;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < c; i += blockDim.x) {
    float t = b2 ? b2[i] : 0.f;
    for (int j = 0; j < cr; ++j) t += w2[i * cr + j] * hid[j];
    s[nimg * c + i] = 1.f / (1.f + expf(-t));
  }
}

static int channel_attention_impl(const char* name, const float* u, int n, int64_t hw, int c, int u_cstride, const float* w1,
                                  const float* b1, const float* w2, const float* b2, int cr, double* workspace, float* s,
                                  float* mean, bool need_mean, void* stream) {
  if (!u || !w1 || !w2 || !workspace || !s || (need_mean && !mean) || n <= 0 || hw <= 0 || c <= 0 || cr <= 0 || u_cstride < c ||
      c % 4 || u_cstride % 4 || c > 1024) {
    set_error("%s: bad args (c, u_cstride multiples of 4, c <= 1024)", name);
    return CLIMSR_EINVAL;
  }
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(channel_sum_partial_kernel, dim3(POOL_SPLIT, n), dim3(256), 0, st, u, (long)hw, c, u_cstride, workspace);
  hipLaunchKernelGGL(ca_mlp_kernel, dim3(n), dim3(1024), (size_t)(c + cr) * sizeof(float), st, workspace, (long)hw, c, cr, w1, b1,
                     w2, b2, s, mean);
  return check_launch(name);
}

extern "C" int climsr_channel_attention(const float* u, int n, int64_t hw, int c, int u_cstride, const float* w1, const float* b1,
                                        const float* w2, const float* b2, int cr, double* workspace, float* s, void* stream) {
  return channel_attention_impl("channel_attention", u, n, hw, c, u_cstride, w1, b1, w2, b2, cr, workspace, s, nullptr, false, stream);
}

// the training forward: the same two launches, and mean[n][c] = the pooled mean the scale was computed from
extern "C" int climsr_channel_attention_keep(const float* u, int n, int64_t hw, int c, int u_cstride, const float* w1,
                                             const float* b1, const float* w2, const float* b2, int cr, double* workspace, float* s,
                                             float* mean, void* stream) {
  return channel_attention_impl("channel_attention_keep", u, n, hw, c, u_cstride, w1, b1, w2, b2, cr, workspace, s, mean, true,
                                stream);
}

extern "C" size_t climsr_channel_attention_workspace(int n, int c) { return (size_t)n * POOL_SPLIT * c * sizeof(double); }

// channel_attention from per-tile channel sums: the image's tile rows folded into POOL_SPLIT fp64 slices (slice sp =
// tiles [tpi sp / POOL_SPLIT, tpi (sp + 1) / POOL_SPLIT), summed in order), then ca_mlp_kernel over the slices -- the
// same fixed order every run.  One workgroup per (slice, image): 256 threads = 4 tile lanes x 64 channels per round.
__global__ __launch_bounds__(256) void tile_parts_fold_kernel(const float* __restrict__ part, int tpi, int c, double* __restrict__ out) {
  const int nimg = blockIdx.y, sp = blockIdx.x;
  const long t0 = (long)tpi * sp / POOL_SPLIT, t1 = (long)tpi * (sp + 1) / POOL_SPLIT;
  __shared__ double sh[256];
  for (int c0 = 0; c0 < c; c0 += 64) {
    const int ch = c0 + (threadIdx.x & 63), tl = threadIdx.x >> 6;
    double t = 0.0;
    if (ch < c)
      for (long k = t0 + tl; k < t1; k += 4) t += (double)part[((long)nimg * tpi + k) * c + ch];
    sh[threadIdx.x] = t;
    __syncthreads();
    if (threadIdx.x < 64 && ch < c)
      out[((long)nimg * POOL_SPLIT + sp) * c + ch] = ((sh[threadIdx.x] + sh[64 + threadIdx.x]) + sh[128 + threadIdx.x]) + sh[192 + threadIdx.x];
    __syncthreads();
  }
}

static int channel_attention_parts_impl(const char* name, const float* part, int n, int tiles_per_image, int64_t hw, int c,
                                        const float* w1, const float* b1, const float* w2, const float* b2, int cr,
                                        double* workspace, float* s, float* mean, bool need_mean, void* stream) {
  if (!part || !w1 || !w2 || !s || !workspace || (need_mean && !mean) || n <= 0 || tiles_per_image <= 0 || hw <= 0 || c <= 0 ||
      c > 1024 || cr <= 0) {
    set_error("%s: bad args", name);
    return CLIMSR_EINVAL;
  }
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(tile_parts_fold_kernel, dim3(POOL_SPLIT, n), dim3(256), 0, st, part, tiles_per_image, c, workspace);
  hipLaunchKernelGGL(ca_mlp_kernel, dim3(n), dim3(1024), (size_t)(c + cr) * sizeof(float), st, workspace, (long)hw, c, cr, w1, b1,
                     w2, b2, s, mean);
  return check_launch(name);
}

extern "C" int climsr_channel_attention_parts(const float* part, int n, int tiles_per_image, int64_t hw, int c, const float* w1,
                                              const float* b1, const float* w2, const float* b2, int cr, double* workspace, float* s,
                                              void* stream) {
  return channel_attention_parts_impl("channel_attention_parts", part, n, tiles_per_image, hw, c, w1, b1, w2, b2, cr, workspace, s,
                                      nullptr, false, stream);
}

extern "C" int climsr_channel_attention_parts_keep(const float* part, int n, int tiles_per_image, int64_t hw, int c, const float* w1,
                                                   const float* b1, const float* w2, const float* b2, int cr, double* workspace,
                                                   float* s, float* mean, void* stream) {
  return channel_attention_parts_impl("channel_attention_parts_keep", part, n, tiles_per_image, hw, c, w1, b1, w2, b2, cr, workspace,
                                      s, mean, true, stream);
}

// xres[p][c] = u[p][c] * s[n][c] + xres[p][c];  xb[p][c] = bf16(xres[p][c])   (RCAB: body(x) + x); u fp32 or bf16
template <bool UB>
__global__ __launch_bounds__(256) void ca_scale_add_kernel(const void* __restrict__ u, int u_cs, const float* __restrict__ s,
                                                           float* __restrict__ xres, uint16_t* __restrict__ xb, int xb_cs, long hw,
                                                           int c, long total4) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total4) return;
  const int cg = c / 4;
  const long pix = i / cg;
  const int c0 = (int)(i % cg) * 4;
  const int nimg = (int)(pix / hw);
  float4 uv;
  if constexpr (UB) {
    const uint2 raw = *(const uint2*)((const uint16_t*)u + pix * u_cs + c0);
    uv = make_float4(__uint_as_float(raw.x << 16), __uint_as_float(raw.x & 0xFFFF0000u), __uint_as_float(raw.y << 16),
                     __uint_as_float(raw.y & 0xFFFF0000u));
  } else {
    uv = *(const float4*)((const float*)u + pix * u_cs + c0);
  }
  const float4 sv = *(const float4*)(s + (long)nimg * c + c0);
  float4 r = *(const float4*)(xres + pix * c + c0);
  r.x = uv.x * sv.x + r.x;
  r.y = uv.y * sv.y + r.y;
  r.z = uv.z * sv.z + r.z;
  r.w = uv.w * sv.w + r.w;
  *(float4*)(xres + pix * c + c0) = r;
  uint2 pk;
  pk.x = (uint32_t)f2bf(r.x) | ((uint32_t)f2bf(r.y) << 16);
  pk.y = (uint32_t)f2bf(r.z) | ((uint32_t)f2bf(r.w) << 16);
  *(uint2*)(xb + pix * xb_cs + c0) = pk;
}

extern "C" int climsr_ca_scale_add(const void* u, int u_bf16, int u_cstride, const float* s, float* xres, uint16_t* xb, int xb_cstride,
                                   int n, int64_t hw, int c, void* stream) {
  if (!u || !s || !xres || !xb || n <= 0 || hw <= 0 || c % 4 || u_cstride % 4 || xb_cstride % 4 || u_cstride < c ||
      xb_cstride < c) {
    set_error("ca_scale_add: bad args (c, strides multiples of 4)");
    return CLIMSR_EINVAL;
  }
  const long total4 = (long)n * hw * (c / 4);
  if (u_bf16)
    hipLaunchKernelGGL(ca_scale_add_kernel<true>, dim3(ceil_div(total4, 256)), dim3(256), 0, (hipStream_t)stream, u, u_cstride, s,
                       xres, xb, xb_cstride, (long)hw, c, total4);
  else
    hipLaunchKernelGGL(ca_scale_add_kernel<false>, dim3(ceil_div(total4, 256)), dim3(256), 0, (hipStream_t)stream, u, u_cstride, s,
                       xres, xb, xb_cstride, (long)hw, c, total4);
  return check_launch("ca_scale_add");
}

// nn.PixelShuffle(r) on NHWC: y[n][y*r+i][x*r+j][co] = x[n][y][x][co*r*r + i*r + j]; one thread per output
// (pixel, 8 channels): 8 gathered 2 B reads from one input pixel's channel vector, one 16 B store.
__global__ __launch_bounds__(256) void pixel_shuffle_kernel(const uint16_t* __restrict__ x, int h, int w, int c_out, int r,
                                                            int in_cs, uint16_t* __restrict__ y, int out_cs, long total) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int cg = c_out / 8;
  const long opix = i / cg;
  const int co0 = (int)(i % cg) * 8;
  const int ow = w * r, oh = h * r;
  const int ox = (int)(opix % ow);
  const long t = opix / ow;
  const int oy = (int)(t % oh);
  const long nimg = t / oh;
  const int yy = oy / r, ii = oy - yy * r, xx = ox / r, jj = ox - xx * r;
  const uint16_t* src = x + ((nimg * h + yy) * w + xx) * in_cs + ii * r + jj;
  const int rr = r * r;
  uint32_t v[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = (uint32_t)src[(co0 + 2 * k) * rr] | ((uint32_t)src[(co0 + 2 * k + 1) * rr] << 16);
  *(uint4*)(y + opix * out_cs + co0) = make_uint4(v[0], v[1], v[2], v[3]);
}

extern "C" int climsr_pixel_shuffle_bf16(const uint16_t* x, int n, int h, int w, int c_out, int r, int in_cstride, uint16_t* y,
                                         int out_cstride, void* stream) {
  if (!x || !y || n <= 0 || h <= 0 || w <= 0 || r < 1 || c_out % 8 || out_cstride % 8 || out_cstride < c_out ||
      in_cstride < c_out * r * r) {
    set_error("pixel_shuffle: bad args (c_out, out_cstride multiples of 8; in_cstride >= c_out*r*r)");
    return CLIMSR_EINVAL;
  }
  const long total = (long)n * h * r * w * r * (c_out / 8);
  hipLaunchKernelGGL(pixel_shuffle_kernel, dim3(ceil_div(total, 256)), dim3(256), 0, (hipStream_t)stream, x, h, w, c_out, r,
                     in_cstride, y, out_cstride, total);
  return check_launch("pixel_shuffle");
}

// nn.PixelShuffle(r) backward = pixel unshuffle on NHWC: y[n][y][x][co*r*r + i*r + j] = x[n][y*r+i][x*r+j][co] (the
// inverse index map, bit-exact); one thread per output (pixel, 8 channels): 8 gathered 2 B reads, one 16 B store.
__global__ __launch_bounds__(256) void pixel_unshuffle_kernel(const uint16_t* __restrict__ x, int h, int w, int c_out, int r,
                                                              int in_cs, uint16_t* __restrict__ y, int out_cs, long total) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int rr = r * r;
  const int cg = c_out * rr / 8;
  const long opix = i / cg;  // low-resolution pixel (n, yy, xx)
  const int k0 = (int)(i % cg) * 8;
  const int xx = (int)(opix % w);
  const long t = opix / w;
  const int yy = (int)(t % h);
  const long nimg = t / h;
  const long wr = (long)w * r;
  const uint16_t* src = x + ((nimg * h + yy) * r * wr + (long)xx * r) * in_cs;  // pixel (yy r, xx r) of the r x r block
  uint16_t e[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int ch = k0 + k, co = ch / rr, rem = ch - co * rr, ii = rem / r, jj = rem - ii * r;
    e[k] = src[((long)ii * wr + jj) * in_cs + co];
  }
  *(uint4*)(y + opix * out_cs + k0) = make_uint4((uint32_t)e[0] | ((uint32_t)e[1] << 16), (uint32_t)e[2] | ((uint32_t)e[3] << 16),
                                                 (uint32_t)e[4] | ((uint32_t)e[5] << 16), (uint32_t)e[6] | ((uint32_t)e[7] << 16));
}

extern "C" int climsr_pixel_unshuffle_bf16(const uint16_t* x, int n, int h, int w, int c_out, int r, int in_cstride, uint16_t* y,
                                           int out_cstride, void* stream) {
  if (!x || !y || n <= 0 || h <= 0 || w <= 0 || r < 1 || c_out <= 0 || (c_out * r * r) % 8 || out_cstride % 8 ||
      out_cstride < c_out * r * r || in_cstride < c_out) {
    set_error("pixel_unshuffle: bad args (c_out*r*r, out_cstride multiples of 8; out_cstride >= c_out*r*r; in_cstride >= c_out)");
    return CLIMSR_EINVAL;
  }
  const long total = (long)n * h * w * (c_out * r * r / 8);
  hipLaunchKernelGGL(pixel_unshuffle_kernel, dim3(ceil_div(total, 256)), dim3(256), 0, (hipStream_t)stream, x, h, w, c_out, r,
                     in_cstride, y, out_cstride, total);
  return check_launch("pixel_unshuffle");
}

// ---------------------------------------------------------------------------------------------------------------
// Channel-attention backward (RCAB: x_out = u * s + x_in, s = sigmoid(W2 relu(W1 mean(u) + b1) + b2)).  With G the
// fp32 gradient at x_out:  q[n][c] = sum_p G u;  dpre2 = q s (1 - s);  dW2 += dpre2 (x) hid, db2 += dpre2;
// dhid = W2^T dpre2 where hid > 0;  dW1 += dhid (x) mean, db1 += dhid;  m = W1^T dhid / HW;  dz_u = bf16(G s + m).
// Three launches, no atomics, every sum in a fixed order.
// ---------------------------------------------------------------------------------------------------------------

// launch 1: part[n][split][c] = sum over the split's pixels of G * u.  CPT channels per thread (16 B of u: 8 bf16 or 4
// fp32; G as float4s); a block is (c / CPT channel lanes) x (256 / (c / CPT) pixel lanes); fp32 per-thread sums, fp64
// across the block -- channel_sum_partial_kernel's scheme.
template <bool UB>
__global__ __launch_bounds__(256) void ca_bwd_dot_partial_kernel(const float* __restrict__ g, int g_cs, const void* __restrict__ u,
                                                                 int u_cs, long hw, int c, double* __restrict__ part) {
  constexpr int CPT = UB ? 8 : 4;
  const int nimg = blockIdx.y, sp = blockIdx.x;
  const long p0 = hw * sp / POOL_SPLIT, p1 = hw * (sp + 1) / POOL_SPLIT;
  __shared__ double sh[256 * CPT];
  const int cg = c / CPT;  // host guarantees c % 8 == 0, cg <= 256
  const int plan = 256 / cg;
  const int gi = threadIdx.x % cg, pl = threadIdx.x / cg;
  float acc[CPT];
#pragma unroll
  for (int k = 0; k < CPT; ++k) acc[k] = 0.f;
  if (pl < plan)
    for (long p = p0 + pl; p < p1; p += plan) {
      const long pix = (long)nimg * hw + p;
      const float* gp = g + pix * g_cs + gi * CPT;
      if constexpr (UB) {
        const uint4 raw = *(const uint4*)((const uint16_t*)u + pix * u_cs + gi * 8);
        const float4 a = *(const float4*)gp, b = *(const float4*)(gp + 4);
        acc[0] += a.x * __uint_as_float(raw.x << 16);
        acc[1] += a.y * __uint_as_float(raw.x & 0xFFFF0000u);
        acc[2] += a.z * __uint_as_float(raw.y << 16);
        acc[3] += a.w * __uint_as_float(raw.y & 0xFFFF0000u);
        acc[4] += b.x * __uint_as_float(raw.z << 16);
        acc[5] += b.y * __uint_as_float(raw.z & 0xFFFF0000u);
        acc[6] += b.z * __uint_as_float(raw.w << 16);
        acc[7] += b.w * __uint_as_float(raw.w & 0xFFFF0000u);
      } else {
        const float4 uv = *(const float4*)((const float*)u + pix * u_cs + gi * 4);
        const float4 a = *(const float4*)gp;
        acc[0] += a.x * uv.x; acc[1] += a.y * uv.y; acc[2] += a.z * uv.z; acc[3] += a.w * uv.w;
      }
    }
#pragma unroll
  for (int k = 0; k < CPT; ++k) sh[threadIdx.x * CPT + k] = acc[k];
  __syncthreads();
  for (int ch = threadIdx.x; ch < c; ch += 256) {
    const int gg = ch / CPT, q = ch % CPT;
    double t = 0.0;
    for (int k = 0; k < plan; ++k) t += sh[(k * cg + gg) * CPT + q];
    part[((long)nimg * POOL_SPLIT + sp) * c + ch] = t;
  }
}

// launch 2, one workgroup per image: q from the slices (fixed order, fp64), hid recomputed from the kept mean with the
// forward's formula, then m[n][c] and the image's factors dpre2[n][c], dhid[n][cr], hid[n][cr] (fac) that launch 3
// sums over the images in image order into the four parameter gradients.
__global__ __launch_bounds__(1024) void ca_mlp_bwd_kernel(const double* __restrict__ part, long hw, int c, int cr,
                                                          const float* __restrict__ s, const float* __restrict__ mean,
                                                          const float* __restrict__ w1, const float* __restrict__ b1,
                                                          const float* __restrict__ w2, float* __restrict__ m,
                                                          float* __restrict__ fac) {
  extern __shared__ double smd[];
  double* dpre2 = smd;      // [c]
  double* dhid = smd + c;   // [cr]
  constexpr int NT = 1024;
  __shared__ double grp[NT];
  const int nimg = blockIdx.x;
  const int n = gridDim.x;
  const int cw = c < NT ? c : NT;
  const int G = NT / cw;
  float* f_dpre2 = fac + (long)nimg * c;
  float* f_dhid = fac + (long)n * c + (long)nimg * cr;
  float* f_hid = fac + (long)n * (c + cr) + (long)nimg * cr;
  for (int c0 = 0; c0 < c; c0 += cw) {
    const int i = c0 + (int)threadIdx.x % cw, gi = (int)threadIdx.x / cw;
    double t = 0.0;
    if (i < c && gi < G)
      for (int sp = gi; sp < POOL_SPLIT; sp += G) t += part[((long)nimg * POOL_SPLIT + sp) * c + i];
    grp[threadIdx.x] = t;
    __syncthreads();
    if ((int)threadIdx.x < cw && c0 + (int)threadIdx.x < c) {
      double q = 0.0;
      for (int k = 0; k < G; ++k) q += grp[k * cw + threadIdx.x];
      const double sv = (double)s[(long)nimg * c + c0 + threadIdx.x];
      const double d = q * sv * (1.0 - sv);
      dpre2[c0 + threadIdx.x] = d;
      f_dpre2[c0 + threadIdx.x] = (float)d;
    }
    __syncthreads();
  }
  for (int j = threadIdx.x; j < cr; j += blockDim.x) {
    float t = b1 ? b1[j] : 0.f;
    for (int i = 0; i < c; ++i) t += w1[j * c + i] * mean[(long)nimg * c + i];
    const float hid = t > 0.f ? t : 0.f;
    double d = 0.0;
    if (hid > 0.f)
      for (int i = 0; i < c; ++i) d += (double)w2[i * cr + j] * dpre2[i];
    dhid[j] = d;
    f_dhid[j] = (float)d;
    f_hid[j] = hid;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < c; i += blockDim.x) {
    double t = 0.0;
    for (int j = 0; j < cr; ++j) t += (double)w1[j * c + i] * dhid[j];
    m[(long)nimg * c + i] = (float)(t / (double)hw);
  }
}

// launch 3: blocks [0, nblk_e) write dz_u = bf16(G * s + m), 8 channels per thread (16 B loads and stores); the blocks
// after them sum the images' factors in image order (fp64) into dW1 [cr][c], db1 [cr], dW2 [c][cr], db2 [c].
__global__ __launch_bounds__(256) void ca_bwd_apply_kernel(const float* __restrict__ g, int g_cs, const float* __restrict__ s,
                                                           const float* __restrict__ m, uint16_t* __restrict__ dzu, int dzu_cs,
                                                           long hw, int c, long total8, int nblk_e, int n, int cr,
                                                           const float* __restrict__ mean, const float* __restrict__ fac,
                                                           float* __restrict__ gw1, float* __restrict__ gb1,
                                                           float* __restrict__ gw2, float* __restrict__ gb2, int accumulate) {
  if ((int)blockIdx.x >= nblk_e) {
    const int e = ((int)blockIdx.x - nblk_e) * 256 + (int)threadIdx.x;
    const int nw = cr * c;
    if (e >= 2 * nw + cr + c) return;
    const float* f_dpre2 = fac;
    const float* f_dhid = fac + (long)n * c;
    const float* f_hid = fac + (long)n * (c + cr);
    double t = 0.0;
    float* dst;
    if (e < nw) {  // dW1[j][i] = sum_n dhid[n][j] * mean[n][i]
      const int j = e / c, i = e - j * c;
      for (int k = 0; k < n; ++k) t += (double)f_dhid[(long)k * cr + j] * (double)mean[(long)k * c + i];
      dst = gw1 + e;
    } else if (e < nw + cr) {  // db1[j]
      const int j = e - nw;
      for (int k = 0; k < n; ++k) t += (double)f_dhid[(long)k * cr + j];
      dst = gb1 ? gb1 + j : nullptr;
    } else if (e < 2 * nw + cr) {  // dW2[i][j] = sum_n dpre2[n][i] * hid[n][j]
      const int q = e - nw - cr, i = q / cr, j = q - i * cr;
      for (int k = 0; k < n; ++k) t += (double)f_dpre2[(long)k * c + i] * (double)f_hid[(long)k * cr + j];
      dst = gw2 + q;
    } else {  // db2[i]
      const int i = e - 2 * nw - cr;
      for (int k = 0; k < n; ++k) t += (double)f_dpre2[(long)k * c + i];
      dst = gb2 ? gb2 + i : nullptr;
    }
    if (dst) *dst = accumulate ? *dst + (float)t : (float)t;
    return;
  }
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total8) return;
  const int cg = c / 8;
  const long pix = i / cg;
  const int c0 = (int)(i % cg) * 8;
  const int nimg = (int)(pix / hw);
  const float* gp = g + pix * g_cs + c0;
  const float4 a = *(const float4*)gp, b = *(const float4*)(gp + 4);
  const float4 s0 = *(const float4*)(s + (long)nimg * c + c0), s1 = *(const float4*)(s + (long)nimg * c + c0 + 4);
  const float4 m0 = *(const float4*)(m + (long)nimg * c + c0), m1 = *(const float4*)(m + (long)nimg * c + c0 + 4);
  // g * s is exact in fp64 and the sum rounds once: the value is bf16(fp32(g s + m)) of the exact fp64 expression
  auto z = [](float gv, float sv, float mv) { return (uint32_t)f2bf((float)((double)gv * (double)sv + (double)mv)); };
  uint4 pk;
  pk.x = z(a.x, s0.x, m0.x) | (z(a.y, s0.y, m0.y) << 16);
  pk.y = z(a.z, s0.z, m0.z) | (z(a.w, s0.w, m0.w) << 16);
  pk.z = z(b.x, s1.x, m1.x) | (z(b.y, s1.y, m1.y) << 16);
  pk.w = z(b.z, s1.z, m1.z) | (z(b.w, s1.w, m1.w) << 16);
  *(uint4*)(dzu + pix * dzu_cs + c0) = pk;
}

// bytes: the fp64 slices [n][POOL_SPLIT][c], then the fp32 per-image factors dpre2 [n][c], dhid [n][cr], hid [n][cr]
extern "C" size_t climsr_channel_attention_bwd_workspace(int n, int c, int cr) {
  if (n <= 0 || c <= 0 || cr <= 0) return 0;
  return (size_t)n * POOL_SPLIT * c * sizeof(double) + (size_t)n * (c + 2 * cr) * sizeof(float);
}

extern "C" int climsr_channel_attention_bwd(const float* g, int g_cstride, const void* u, int u_bf16, int u_cstride, const float* s,
                                            const float* mean, int n, int64_t hw, int c, const float* w1, const float* b1,
                                            const float* w2, int cr, void* workspace, float* m, float* gw1, float* gb1, float* gw2,
                                            float* gb2, int accumulate, uint16_t* dzu, int dzu_cstride, void* stream) {
  const int uv = u_bf16 ? 8 : 4;
  if (!g || !u || !s || !mean || !w1 || !w2 || !workspace || !m || !gw1 || !gw2 || !dzu || n <= 0 || hw <= 0 || c <= 0 || cr <= 0 ||
      c % 8 || c > 1024 || cr > c || g_cstride % 4 || g_cstride < c || u_cstride % uv || u_cstride < c || dzu_cstride % 8 ||
      dzu_cstride < c || (long)n * hw > (1L << 40)) {
    set_error("channel_attention_bwd: bad args (c multiple of 8, <= 1024; cr <= c; g_cstride multiple of 4, u_cstride of 4 (fp32) "
              "or 8 (bf16), dzu_cstride of 8; strides >= c)");
    return CLIMSR_EINVAL;
  }
  hipStream_t st = (hipStream_t)stream;
  double* part = (double*)workspace;
  float* fac = (float*)(part + (size_t)n * POOL_SPLIT * c);
  if (u_bf16)
    hipLaunchKernelGGL(ca_bwd_dot_partial_kernel<true>, dim3(POOL_SPLIT, n), dim3(256), 0, st, g, g_cstride, u, u_cstride, (long)hw, c,
                       part);
  else
    hipLaunchKernelGGL(ca_bwd_dot_partial_kernel<false>, dim3(POOL_SPLIT, n), dim3(256), 0, st, g, g_cstride, u, u_cstride, (long)hw,
                       c, part);
  hipLaunchKernelGGL(ca_mlp_bwd_kernel, dim3(n), dim3(1024), (size_t)(c + cr) * sizeof(double), st, part, (long)hw, c, cr, s, mean, w1,
                     b1, w2, m, fac);
  const long total8 = (long)n * hw * (c / 8);
  const int nblk_e = ceil_div(total8, 256), nblk_p = ceil_div(2L * cr * c + cr + c, 256);
  hipLaunchKernelGGL(ca_bwd_apply_kernel, dim3(nblk_e + nblk_p), dim3(256), 0, st, g, g_cstride, s, m, dzu, dzu_cstride, (long)hw, c,
                     total8, nblk_e, n, cr, mean, fac, gw1, gb1, gw2, gb2, accumulate);
  return check_launch("channel_attention_bwd");
}
