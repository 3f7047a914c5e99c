// On-device tile pipeline and validation metrics.
//
// Tile pipeline: the per-sample work of ClimateDataset.__getitem__ / _get_training_sample /
// _get_val_test_sample (climsr/data/sr/climate_dataset.py:144-189, 191-218, 220-275) and the
// MinMaxScaler / StandardScaler arithmetic (climsr/data/normalization.py:37-61, 99-116), done for a
// whole batch of raw tiles already resident in HBM: v-flip, h-flip, rot90, normalisation with NaN
// substitution, land mask, nearest decimation to LR (cv2.INTER_NEAREST with an integer ratio picks
// [::s, ::s]) and the channel concatenation of _concat_if_needed (:95-118).  One thread per HR
// output pixel; every output is written once with unit stride.  HBM-bound byte shuffling: no MFMA.
//
// Metrics: TaskSuperResolutionModule.common_val_test_step + compute_metrics (climsr/core/task.py:
// 262-294, 336-372): denormalise, mask sea pixels to 0, then RegressionAccuracy x8, PSNR, SSIM,
// MAE, MSE, RMSE, MAPE, SMAPE, R2 and the normalised L1, as one fused deterministic reduction (fixed
// block partials, single-block final sum) plus a separable-Gaussian SSIM pass.  Nothing syncs the
// host: SSIM's data range and constants are read from the first pass's device results.
//
// Inference front end (end of the file): the same normalisation for whole raw LR grids plus the static
// elevation / land-mask planes of the reference's two inference datasets.
//
// Built with -ffp-contract=off (Makefile): the normalisation reproduces numpy's one-rounding-per-
// operation arithmetic bit for bit, which a fused multiply-add would break.
#include <math.h>

#include "common.h"

using namespace climsr;

// ------------------------------------------------------------------------------------------
// per-tile nanmin / nanmax (np.nanmin / np.nanmax after missing_indicator -> NaN)
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(1024) tile_minmax_kernel(const float* __restrict__ x, long count, float missing,
                                                           int use_missing, float* __restrict__ out) {
  const float* t = x + (long)blockIdx.x * count;
  float mn = INFINITY, mx = -INFINITY;
  int any = 0;
  for (long i = threadIdx.x; i < count; i += blockDim.x) {
    float v = t[i];
    if (isnan(v) || (use_missing && v == missing)) continue;
    mn = fminf(mn, v);
    mx = fmaxf(mx, v);
    any = 1;
  }
  for (int o = 32; o > 0; o >>= 1) {
    mn = fminf(mn, __shfl_down(mn, o));
    mx = fmaxf(mx, __shfl_down(mx, o));
    any |= __shfl_down(any, o);
  }
  __shared__ float smn[16], smx[16];
  __shared__ int sany[16];
  int wv = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    smn[wv] = mn;
    smx[wv] = mx;
    sany[wv] = any;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < (int)(blockDim.x >> 6); ++i) {
      mn = fminf(mn, smn[i]);
      mx = fmaxf(mx, smx[i]);
      any |= sany[i];
    }
    out[2 * blockIdx.x] = any ? mn : NAN;  // all-NaN slice: numpy returns nan
    out[2 * blockIdx.x + 1] = any ? mx : NAN;
  }
}

extern "C" int climsr_tile_minmax_f32(const float* x, int n, int64_t count, float missing, int use_missing, float* out,
                                      void* stream) {
  if (!x || !out || n <= 0 || count <= 0) {
    set_error("tile_minmax: bad args (n=%d count=%lld)", n, (long long)count);
    return CLIMSR_EINVAL;
  }
  hipLaunchKernelGGL(tile_minmax_kernel, dim3(n), dim3(1024), 0, (hipStream_t)stream, x, (long)count, missing, use_missing, out);
  return check_launch("tile_minmax");
}

// ------------------------------------------------------------------------------------------
// tile pipeline
// ------------------------------------------------------------------------------------------
struct Scale32 {
  float mul, add;
};

// Output pixel (y, x) of the transformed tile -> pixel of the raw tile.  The reference applies, in
// order, np.flipud, np.fliplr, np.rot90(., k) (climate_dataset.py:149-166); invert rot first.
__device__ __forceinline__ void source_of(int y, int x, int h, int w, int code, int& sy, int& sx) {
  int k = (code >> 2) & 3;
  int fy, fx;  // position in the flipped (pre-rotation) array, which is h x w
  if (k == 0) {
    fy = y; fx = x;
  } else if (k == 1) {  // rot90 k=1: out[i, j] = in[j, W-1-i]
    fy = x; fx = w - 1 - y;
  } else if (k == 2) {  // out[i, j] = in[H-1-i, W-1-j]
    fy = h - 1 - y; fx = w - 1 - x;
  } else {              // k=3: out[i, j] = in[H-1-j, i]
    fy = h - 1 - x; fx = y;
  }
  sy = (code & 1) ? h - 1 - fy : fy;
  sx = (code & 2) ? w - 1 - fx : fx;
}

// MinMaxScaler._normalize with min/max given as float64 (the per-file / global stats of the feather
// tables): numpy computes scale and offset in float64 and, under NEP 50 (numpy >= 2), the float32
// tile is promoted by the np.float64 scalars, so the value is rounded to float32 once at the end.
__device__ __forceinline__ float minmax_f64(float v, double scale, double add, float nan_sub) {
  double r = __dadd_rn(__dmul_rn((double)v, scale), add);  // two double roundings, as numpy (no fma)
  float f = (float)r;
  return isnan(f) ? nan_sub : f;
}

// MinMaxScaler._normalize with min/max from np.nanmin/np.nanmax of a float32 array (elevation):
// everything stays float32 under NEP 50, with one rounding per numpy operation.
// Python-float operands (a, b - a, eps) are weak scalars: converted to float32 at each use.
__device__ __forceinline__ Scale32 minmax_f32_params(float mn, float mx, double a, double b, double eps) {
  float range = __fsub_rn(mx, mn);
  float den = __fadd_rn(range, (float)eps);
  float scale = __fdiv_rn((float)(b - a), den);
  float add = __fsub_rn((float)a, __fmul_rn(mn, scale));
  return {scale, add};
}

// StandardScaler._normalize: (arr - mean) / (std + eps) in float64 (np.float64 stats), rounded once.
__device__ __forceinline__ float zscore_f64(float v, double mean, double std, double eps, double nan_sub) {
  double r = __ddiv_rn(__dsub_rn((double)v, mean), __dadd_rn(std, eps));
  float f = (float)r;
  if (isnan(f) && nan_sub != 0.0) f = (float)nan_sub;  // `if self.nan_substitution:`
  return f;
}

// `out_arr * scale; out_arr += min_` on a float32 array with float32 scale / offset, then NaN -> nan_sub.
__device__ __forceinline__ float minmax_f32(float v, Scale32 s, float nan_sub) {
  float f = __fadd_rn(__fmul_rn(v, s.mul), s.add);
  return isnan(f) ? nan_sub : f;
}

__device__ __forceinline__ float normalize_hr(float v, const ClimsrTileDesc& d, double scale, double add) {
  if (d.method == 0) return minmax_f64(v, scale, add, (float)d.nan_sub);
  if (d.method == 1) return zscore_f64(v, d.zs_hr_mean, d.zs_hr_std, d.eps, d.zs_hr_nan_sub);
  return v;
}

__device__ __forceinline__ float normalize_elev(float v, const ClimsrTileDesc& d, Scale32 es) {
  if (v == d.elev_missing) v = NAN;  // `out_arr[arr == missing_indicator] = np.nan`
  if (d.method == 0) return minmax_f32(v, es, (float)d.nan_sub);
  if (d.method == 1) return zscore_f64(v, d.zs_elev_mean, d.zs_elev_std, d.eps, d.zs_elev_nan_sub);
  return v;
}

__global__ void __launch_bounds__(256) tile_prepare_kernel(ClimsrTileDesc d) {
  const int hw = d.h * d.w;
  long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (long)d.n * hw) return;
  const int t = (int)(gid / hw);
  const int rem = (int)(gid - (long)t * hw);
  const int y = rem / d.w, x = rem - (rem / d.w) * d.w;
  const int code = d.xform ? d.xform[t] : 0;
  const float* hr_raw = d.hr_raw + (long)t * hw;
  const float* el_raw = d.elev_raw ? d.elev_raw + (long)t * hw : nullptr;

  double hs = 0.0, ha = 0.0;
  if (d.method == 0) {  // normalization.py:51-56 in float64
    double mn = d.hr_min[t], mx = d.hr_max[t];
    hs = __ddiv_rn(d.range_b - d.range_a, __dadd_rn(__dsub_rn(mx, mn), d.eps));
    ha = __dsub_rn(d.range_a, __dmul_rn(mn, hs));
  }
  Scale32 es = {0.f, 0.f};
  if (el_raw && d.method == 0) es = minmax_f32_params(d.elev_minmax[2 * t], d.elev_minmax[2 * t + 1], d.range_a, d.range_b, d.eps);

  int sy, sx;
  source_of(y, x, d.h, d.w, code, sy, sx);
  const float raw = hr_raw[sy * d.w + sx];
  const float hv = normalize_hr(raw, d, hs, ha);
  const float mv = isnan(raw) ? 0.f : 1.f;  // mask = ~np.isnan(original_image)
  const float ev = el_raw ? normalize_elev(el_raw[sy * d.w + sx], d, es) : 0.f;

  const long o = (long)t * hw + rem;
  d.hr[o] = hv;
  if (d.elev) d.elev[o] = ev;
  if (d.mask) d.mask[o] = mv;

  const int s = d.scale, lh = d.h / s, lw = d.w / s;
  // nearest decimation (A.Resize INTER_NEAREST, integer ratio) and nearest upscale of the LR tile
  const int ny = (y / s) * s, nx = (x / s) * s;
  float near = hv;
  if (ny != y || nx != x) {
    int qy, qx;
    source_of(ny, nx, d.h, d.w, code, qy, qx);
    near = normalize_hr(hr_raw[qy * d.w + qx], d, hs, ha);
  }
  if (d.nearest) d.nearest[o] = near;
  if (d.srcnn) {  // _concat_if_needed, SRCNN branch: [nearest(lr), elev, mask] at HR size
    float* l = d.lr + (long)t * d.lr_c * hw + rem;
    int c = 0;
    l[(long)(c++) * hw] = near;
    if (d.use_elev) l[(long)(c++) * hw] = ev;
    if (d.use_mask) l[(long)(c++) * hw] = mv;
  } else if (ny == y && nx == x) {  // [lr, elev_lr, mask_lr] at LR size
    const int lhw = lh * lw;
    const int lo = (y / s) * lw + (x / s);
    float* l = d.lr + (long)t * d.lr_c * lhw + lo;
    int c = 0;
    l[(long)(c++) * lhw] = hv;
    if (d.use_elev) l[(long)(c++) * lhw] = ev;
    if (d.use_mask) l[(long)(c++) * lhw] = mv;
  }
  if (d.elev_lr && ny == y && nx == x) d.elev_lr[(long)t * lh * lw + (y / s) * lw + (x / s)] = ev;
  if (d.hr_lr && ny == y && nx == x) d.hr_lr[(long)t * lh * lw + (y / s) * lw + (x / s)] = hv;
}

extern "C" int climsr_tile_prepare(const ClimsrTileDesc* d, void* stream) {
  if (!d || !d->hr_raw || !d->hr || !d->lr || d->n <= 0 || d->h <= 0 || d->w <= 0 || d->scale <= 0 ||
      d->h % d->scale || d->w % d->scale) {
    set_error("tile_prepare: bad args (h and w must be positive multiples of scale)");
    return CLIMSR_EINVAL;
  }
  int want_c = 1 + (d->use_elev ? 1 : 0) + (d->use_mask ? 1 : 0);
  if (d->lr_c != want_c || (d->use_elev && !d->elev_raw) || (d->method == 0 && (!d->hr_min || !d->hr_max)) ||
      (d->method == 0 && d->elev_raw && !d->elev_minmax) || d->method < 0 || d->method > 2) {
    set_error("tile_prepare: lr_c=%d (expected %d) / missing elevation, stats or min-max inputs", d->lr_c, want_c);
    return CLIMSR_EINVAL;
  }
  if (d->h != d->w && d->xform) {
    // rot90 with an odd factor changes the shape; the reference tiles are square (128 or 452)
    set_error("tile_prepare: random rotation needs square tiles (got %dx%d)", d->h, d->w);
    return CLIMSR_EINVAL;
  }
  long total = (long)d->n * d->h * d->w;
  hipLaunchKernelGGL(tile_prepare_kernel, dim3(ceil_div(total, 256)), dim3(256), 0, (hipStream_t)stream, *d);
  return check_launch("tile_prepare");
}

// ------------------------------------------------------------------------------------------
// cv2.resize(INTER_CUBIC) upscale, float32 path (the `cubic` baseline of the val/test batch,
// climate_dataset.py:195).  cv2: fx = (dx + 0.5) * (src/dst) - 0.5, sx = floor(fx), A = -0.75,
// taps sx-1..sx+2 clamped to the border (replicate), horizontal pass then vertical, float math.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ void cubic_coeffs(float x, float c[4]) {
  const float A = -0.75f;
  c[0] = ((A * (x + 1) - 5 * A) * (x + 1) + 8 * A) * (x + 1) - 4 * A;
  c[1] = ((A + 2) * x - (A + 3)) * x * x + 1;
  c[2] = ((A + 2) * (1 - x) - (A + 3)) * (1 - x) * (1 - x) + 1;
  c[3] = 1.f - c[0] - c[1] - c[2];
}

__global__ void __launch_bounds__(256) resize_cubic_kernel(const float* __restrict__ src, int n, int sh, int sw,
                                                           float* __restrict__ dst, int dh, int dw) {
  long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long dhw = (long)dh * dw;
  if (gid >= (long)n * dhw) return;
  int t = (int)(gid / dhw);
  int rem = (int)(gid - (long)t * dhw);
  int dy = rem / dw, dx = rem - (rem / dw) * dw;
  float fy = (float)((dy + 0.5) * ((double)sh / dh) - 0.5);
  float fx = (float)((dx + 0.5) * ((double)sw / dw) - 0.5);
  int y0 = (int)floorf(fy), x0 = (int)floorf(fx);
  float cy[4], cx[4];
  cubic_coeffs(fy - y0, cy);
  cubic_coeffs(fx - x0, cx);
  const float* s = src + (long)t * sh * sw;
  float acc = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int yy = min(max(y0 - 1 + i, 0), sh - 1);
    const float* row = s + (long)yy * sw;
    float r = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) r = __fadd_rn(r, __fmul_rn(row[min(max(x0 - 1 + j, 0), sw - 1)], cx[j]));
    acc = __fadd_rn(acc, __fmul_rn(r, cy[i]));
  }
  dst[gid] = acc;
}

extern "C" int climsr_resize_cubic_f32(const float* src, int n, int sh, int sw, float* dst, int dh, int dw, void* stream) {
  if (!src || !dst || n <= 0 || sh <= 0 || sw <= 0 || dh <= 0 || dw <= 0) {
    set_error("resize_cubic: bad args");
    return CLIMSR_EINVAL;
  }
  long total = (long)n * dh * dw;
  hipLaunchKernelGGL(resize_cubic_kernel, dim3(ceil_div(total, 256)), dim3(256), 0, (hipStream_t)stream, src, n, sh, sw, dst,
                     dh, dw);
  return check_launch("resize_cubic");
}

// ------------------------------------------------------------------------------------------
// validation / test metrics
// ------------------------------------------------------------------------------------------
namespace {
constexpr int MET_BLOCKS = 1024;  // 4 blocks of 4 waves per CU: the fused pass is load-latency bound
constexpr int SSIM_BLOCKS = 1024;
constexpr int SSIM_T = 32;                 // output tile edge
constexpr int SSIM_K = 11, SSIM_R = 5;     // torchmetrics SSIM defaults: kernel 11, sigma 1.5
constexpr int SSIM_IN = SSIM_T + 2 * SSIM_R;
// per-block partial slots
enum {
  P_ABS = 0, P_SQ, P_ACC0, P_MAPE = P_ACC0 + 8, P_SMAPE, P_T, P_TT, P_L1N, P_NSUM,
  P_TD_MIN = P_NSUM, P_TD_MAX, P_PN_MIN, P_PN_MAX, P_TN_MIN, P_TN_MAX, P_SLOTS
};
// stats after the first pass (workspace tail)
constexpr int WS_STATS = MET_BLOCKS * P_SLOTS;
constexpr int WS_SSIM = WS_STATS + 32;
}  // namespace

struct Denorm {
  int t = -1;
  double scale = 1.0, add = 0.0;
};

// Pixel i (flat index over the batch) of sample t: the masked normalised pair (pn, tn) and the masked denormalised pair (pd, td).
__device__ __forceinline__ void masked_values_at(const ClimsrMetricsDesc& d, long i, int t, Denorm& dn, float& pn, float& tn,
                                                 double& pd, double& td) {
  const bool land = d.mask[i] != 0.f;  // `(~mask.bool())` -> 0
  const float sr = d.sr[i];
  pn = land ? sr : 0.f;
  tn = land ? d.hr[i] : 0.f;
  double den;
  if (d.method == 0) {  // MinMaxScaler._denormalize with float64 min/max tensors (task.py:281-285)
    if (t != dn.t) {    // per-sample constants, recomputed only when the grid-stride loop crosses a sample
      double mn = d.min[t], mx = d.max[t];
      dn.scale = __ddiv_rn(d.range_b - d.range_a, __dadd_rn(__dsub_rn(mx, mn), d.eps));
      dn.add = __dsub_rn(d.range_a, __dmul_rn(mn, dn.scale));
      dn.t = t;
    }
    den = __ddiv_rn(__dsub_rn((double)sr, dn.add), dn.scale);
  } else if (d.method == 1) {  // StandardScaler._denormalize: float32 tensor * python float
    den = (double)__fadd_rn(__fmul_rn(sr, (float)d.zs_std), (float)d.zs_mean);
  } else {
    den = (double)sr;
  }
  pd = land ? den : 0.0;
  td = land ? (double)d.original[i] : 0.0;
}

__device__ __forceinline__ void masked_values(const ClimsrMetricsDesc& d, long i, Denorm& dn, float& pn, float& tn, double& pd,
                                              double& td) {
  const int hw = d.h * d.w;
  masked_values_at(d, i, (int)(i / hw), dn, pn, tn, pd, td);
}

// One thread's running sums and extrema of the fused pass.
struct PixelAcc {
  double acc[P_NSUM];
  double tdmin, tdmax;
  float pnmin, pnmax, tnmin, tnmax;
};

__device__ __forceinline__ void acc_init(PixelAcc& a) {
#pragma unroll
  for (int k = 0; k < P_NSUM; ++k) a.acc[k] = 0.0;
  a.tdmin = INFINITY;
  a.tdmax = -INFINITY;
  a.pnmin = a.tnmin = INFINITY;
  a.pnmax = a.tnmax = -INFINITY;
}

__device__ __forceinline__ void acc_pixel(const ClimsrMetricsDesc& d, PixelAcc& a, float pn, float tn, double pd, double td) {
  const float MEPS = 1.17e-06f;  // torchmetrics MAPE / SMAPE epsilon
  double dd = pd - td;
  double ad = fabs(dd);
  a.acc[P_ABS] += ad;
  a.acc[P_SQ] += dd * dd;
#pragma unroll
  for (int k = 0; k < 8; ++k) a.acc[P_ACC0 + k] += (ad <= (double)d.acc_eps[k]) ? 1.0 : 0.0;
  float dn = fabsf(pn - tn);
  a.acc[P_MAPE] += (double)(dn / fmaxf(fabsf(tn), MEPS));
  a.acc[P_SMAPE] += ad / fmax(fabs(td) + fabs(pd), (double)MEPS);
  a.acc[P_T] += td;
  a.acc[P_TT] += td * td;
  a.acc[P_L1N] += (double)dn;
  a.tdmin = fmin(a.tdmin, td);
  a.tdmax = fmax(a.tdmax, td);
  a.pnmin = fminf(a.pnmin, pn);
  a.pnmax = fmaxf(a.pnmax, pn);
  a.tnmin = fminf(a.tnmin, tn);
  a.tnmax = fmaxf(a.tnmax, tn);
}

// The 256 threads' PixelAcc -> dst[P_SLOTS]: shuffle tree per wave, then the 4 waves in order.
__device__ __forceinline__ void acc_block_store(const PixelAcc& a, double* __restrict__ dst) {
  __shared__ double sh[P_SLOTS][4];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double v[P_SLOTS];
#pragma unroll
  for (int k = 0; k < P_NSUM; ++k) v[k] = a.acc[k];
  v[P_TD_MIN] = a.tdmin;
  v[P_TD_MAX] = a.tdmax;
  v[P_PN_MIN] = a.pnmin;
  v[P_PN_MAX] = a.pnmax;
  v[P_TN_MIN] = a.tnmin;
  v[P_TN_MAX] = a.tnmax;
#pragma unroll
  for (int k = 0; k < P_SLOTS; ++k) {
    double x = v[k];
    for (int o = 32; o > 0; o >>= 1) {
      double y = __shfl_down(x, o);
      if (k < P_NSUM) x += y;
      else if ((k - P_NSUM) % 2 == 0) x = fmin(x, y);
      else x = fmax(x, y);
    }
    if (lane == 0) sh[k][wv] = x;
  }
  __syncthreads();
  if (threadIdx.x < P_SLOTS) {
    int k = threadIdx.x;
    double x = sh[k][0];
    for (int i = 1; i < 4; ++i) {
      double y = sh[k][i];
      if (k < P_NSUM) x += y;
      else if ((k - P_NSUM) % 2 == 0) x = fmin(x, y);
      else x = fmax(x, y);
    }
    dst[k] = x;
  }
}

__global__ void __launch_bounds__(256) metrics_partial_kernel(ClimsrMetricsDesc d) {
  PixelAcc a;
  acc_init(a);
  const long total = (long)d.n * d.h * d.w;
  Denorm dn_cache;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    float pn, tn;
    double pd, td;
    masked_values(d, i, dn_cache, pn, tn, pd, td);
    acc_pixel(d, a, pn, tn, pd, td);
  }
  acc_block_store(a, d.workspace + (long)blockIdx.x * P_SLOTS);
}

__device__ __forceinline__ double combine(int k, double x, double y) {
  if (k < P_NSUM) return x + y;
  return ((k - P_NSUM) % 2 == 0) ? fmin(x, y) : fmax(x, y);
}

// One block of 16 waves; wave w combines slots w, w+16: lane l folds partials l, l+64, ... in order, then a
// fixed shuffle tree -> deterministic, no block-wide barriers.
__global__ void __launch_bounds__(1024) metrics_stats_kernel(ClimsrMetricsDesc d) {
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int k = wv; k < P_SLOTS; k += 16) {
    double x = d.workspace[(long)lane * P_SLOTS + k];
    for (int b = lane + 64; b < MET_BLOCKS; b += 64) x = combine(k, x, d.workspace[(long)b * P_SLOTS + k]);
    for (int o = 32; o > 0; o >>= 1) x = combine(k, x, __shfl_down(x, o));
    if (lane == 0) d.workspace[WS_STATS + k] = x;
  }
}

// SSIM over the masked normalised maps: 5 Gaussian-filtered maps (p, t, p², t², pt), reflect padding
// (only the cropped interior [5, h-5) x [5, w-5) is averaged, whose windows never touch the pad).
struct SsimLds {
  float sp[SSIM_IN][SSIM_IN + 1], st[SSIM_IN][SSIM_IN + 1];
  float hsum[5][SSIM_IN][SSIM_T + 1];
  float g[SSIM_K];
  double red[4];
};

// The window weights; visible to the block after the barrier that opens ssim_tile.
__device__ __forceinline__ void ssim_gaussian(SsimLds& L) {
  if (threadIdx.x < SSIM_K) {  // torchmetrics _gaussian: exp(-(dist/sigma)^2 / 2), normalised
    float s = 0.f, gv = 0.f;
    for (int i = 0; i < SSIM_K; ++i) {
      float dist = (float)(i - SSIM_R);
      float e = expf(-((dist / 1.5f) * (dist / 1.5f)) / 2.f);
      s += e;
      if (i == (int)threadIdx.x) gv = e;
    }
    L.g[threadIdx.x] = gv / s;
  }
}

// data_range=None: the larger of the two maps' ranges -> the stabilisers c1, c2.
__device__ __forceinline__ void ssim_consts(double pnmin, double pnmax, double tnmin, double tnmax, float& c1, float& c2) {
  const float dr = fmaxf((float)pnmax - (float)pnmin, (float)tnmax - (float)tnmin);
  c1 = (0.01f * dr) * (0.01f * dr);
  c2 = (0.03f * dr) * (0.03f * dr);
}

// The whole block's sum of the threads' `part` (shuffle tree per wave, then the 4 waves in order); valid in thread 0.
__device__ __forceinline__ double ssim_block_sum(SsimLds& L, double part) {
  for (int o = 32; o > 0; o >>= 1) part += __shfl_down(part, o);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) L.red[threadIdx.x >> 6] = part;
  __syncthreads();
  return L.red[0] + L.red[1] + L.red[2] + L.red[3];
}

// One 32x32 tile of sample b's cropped SSIM map, origin (oy0, ox0): each thread adds its pixels' indices to `part`.
__device__ __forceinline__ void ssim_tile(const ClimsrMetricsDesc& d, SsimLds& L, int b, int oy0, int ox0, float c1, float c2,
                                          double& part) {
  auto& sp = L.sp;
  auto& st = L.st;
  auto& hsum = L.hsum;
  auto& g = L.g;
  const int oh = d.h - 2 * SSIM_R, ow = d.w - 2 * SSIM_R;
  __syncthreads();
  for (int e = threadIdx.x; e < SSIM_IN * SSIM_IN; e += blockDim.x) {
    int iy = e / SSIM_IN, ix = e % SSIM_IN;
    int gy = oy0 + iy, gx = ox0 + ix;  // input row/col (crop offset cancels the window radius)
    float pn = 0.f, tn = 0.f;
    if (gy < d.h && gx < d.w) {  // normalised maps only: SSIM never sees the denormalised values
      long i = ((long)b * d.h + gy) * d.w + gx;
      if (d.mask[i] != 0.f) {
        pn = d.sr[i];
        tn = d.hr[i];
      }
    }
    sp[iy][ix] = pn;
    st[iy][ix] = tn;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < SSIM_IN * SSIM_T; e += blockDim.x) {
    int iy = e / SSIM_T, ox = e % SSIM_T;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, a4 = 0.f;
#pragma unroll
    for (int k = 0; k < SSIM_K; ++k) {
      float p = sp[iy][ox + k], q = st[iy][ox + k], w = g[k];
      a0 += w * p;
      a1 += w * q;
      a2 += w * (p * p);
      a3 += w * (q * q);
      a4 += w * (p * q);
    }
    hsum[0][iy][ox] = a0;
    hsum[1][iy][ox] = a1;
    hsum[2][iy][ox] = a2;
    hsum[3][iy][ox] = a3;
    hsum[4][iy][ox] = a4;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < SSIM_T * SSIM_T; e += blockDim.x) {
    int oy = e / SSIM_T, ox = e % SSIM_T;
    if (oy0 + oy >= oh || ox0 + ox >= ow) continue;
    float m[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < SSIM_K; ++k) {
      float w = g[k];
#pragma unroll
      for (int q = 0; q < 5; ++q) m[q] += w * hsum[q][oy + k][ox];
    }
    float mu_p2 = m[0] * m[0], mu_t2 = m[1] * m[1], mu_pt = m[0] * m[1];
    float s_p = m[2] - mu_p2, s_t = m[3] - mu_t2, s_pt = m[4] - mu_pt;
    float upper = 2.f * s_pt + c2, lower = s_p + s_t + c2;
    part += (double)(((2.f * mu_pt + c1) * upper) / ((mu_p2 + mu_t2 + c1) * lower));
  }
}

__global__ void __launch_bounds__(256) ssim_kernel(ClimsrMetricsDesc d) {
  __shared__ SsimLds L;
  const int oh = d.h - 2 * SSIM_R, ow = d.w - 2 * SSIM_R;
  const int tiles_y = (oh + SSIM_T - 1) / SSIM_T, tiles_x = (ow + SSIM_T - 1) / SSIM_T;
  const long ntiles = (long)d.n * tiles_y * tiles_x;
  ssim_gaussian(L);
  float c1, c2;
  const double* stats = d.workspace + WS_STATS;
  ssim_consts(stats[P_PN_MIN], stats[P_PN_MAX], stats[P_TN_MIN], stats[P_TN_MAX], c1, c2);
  double part = 0.0;
  for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int b = (int)(tile / (tiles_y * tiles_x));
    const int r = (int)(tile - (long)b * tiles_y * tiles_x);
    ssim_tile(d, L, b, (r / tiles_x) * SSIM_T, (r % tiles_x) * SSIM_T, c1, c2, part);  // cropped-output origin
  }
  const double sum = ssim_block_sum(L, part);
  if (threadIdx.x == 0) d.workspace[WS_SSIM + blockIdx.x] = sum;
}

// The 17 results of `nimg` samples of h x w from their combined slots s[P_SLOTS] and the sum of their SSIM maps.
__device__ __forceinline__ void metrics_formulas(const ClimsrMetricsDesc& d, const double* s, double ssim_sum, int nimg,
                                                 double* out) {
  const double n = (double)nimg * d.h * d.w;
  for (int k = 0; k < 8; ++k) out[k] = s[P_ACC0 + k] / n;  // RegressionAccuracy: correct / total
  const double mse = s[P_SQ] / n;
  const double range = s[P_TD_MAX] - s[P_TD_MIN];           // PSNR(data_range=None): target max - min
  out[8] = (2.0 * log(range) - log(mse)) * (10.0 / log(10.0));
  out[9] = ssim_sum / ((double)nimg * (d.h - 2 * SSIM_R) * (d.w - 2 * SSIM_R));
  out[10] = s[P_ABS] / n;       // MAE
  out[11] = mse;                // MSE
  out[12] = sqrt(mse);          // RMSE (MeanSquaredError(squared=False))
  out[13] = s[P_MAPE] / n;      // MAPE on the normalised maps
  out[14] = 2.0 * s[P_SMAPE] / n;
  const double mean_t = s[P_T] / n;  // R2Score: 1 - SS_res / (sum t^2 - sum t * mean t)
  out[15] = 1.0 - s[P_SQ] / (s[P_TT] - s[P_T] * mean_t);
  out[16] = s[P_L1N] / n;       // normalised L1 (`{prefix}/normalized_loss`, `{prefix}/loss`)
}

__global__ void __launch_bounds__(SSIM_BLOCKS) metrics_final_kernel(ClimsrMetricsDesc d, int ssim_blocks) {
  __shared__ double sh[SSIM_BLOCKS];
  sh[threadIdx.x] = (int)threadIdx.x < ssim_blocks ? d.workspace[WS_SSIM + threadIdx.x] : 0.0;
  __syncthreads();
  for (int o = SSIM_BLOCKS / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  metrics_formulas(d, d.workspace + WS_STATS, sh[0], d.n, d.out);
}

extern "C" size_t climsr_sr_metrics_workspace(void) { return (size_t)(WS_SSIM + SSIM_BLOCKS) * sizeof(double); }

extern "C" int climsr_sr_metrics(const ClimsrMetricsDesc* d, void* stream) {
  if (!d || !d->sr || !d->hr || !d->original || !d->mask || !d->workspace || !d->out || d->n <= 0 ||
      d->h < SSIM_K || d->w < SSIM_K || (d->method == 0 && (!d->min || !d->max)) || d->method < 0 || d->method > 2) {
    set_error("sr_metrics: bad args (h, w >= %d for the 11x11 SSIM window; min/max needed for minmax)", SSIM_K);
    return CLIMSR_EINVAL;
  }
  hipStream_t s = (hipStream_t)stream;
  const ClimsrMetricsDesc dd = *d;
  hipLaunchKernelGGL(metrics_partial_kernel, dim3(MET_BLOCKS), dim3(256), 0, s, dd);
  hipLaunchKernelGGL(metrics_stats_kernel, dim3(1), dim3(1024), 0, s, dd);
  const int oh = d->h - 2 * SSIM_R, ow = d->w - 2 * SSIM_R;
  long ntiles = (long)d->n * ((oh + SSIM_T - 1) / SSIM_T) * ((ow + SSIM_T - 1) / SSIM_T);
  int sb = (int)(ntiles < SSIM_BLOCKS ? ntiles : SSIM_BLOCKS);
  hipLaunchKernelGGL(ssim_kernel, dim3(sb), dim3(256), 0, s, dd);
  hipLaunchKernelGGL(metrics_final_kernel, dim3(1), dim3(SSIM_BLOCKS), 0, s, dd, sb);
  return check_launch("sr_metrics");
}

// ------------------------------------------------------------------------------------------
// The same 17 results per image (LogImagesCallback._metrics_per_image, core/callbacks.py:223-246): row t is what
// climsr_sr_metrics defines for the one-image batch {t}.  Three launches whatever n: (1) the fused pass, where image t
// is split over pi_blocks(h, w) workgroups whose partials go to workspace slot (t, block); (2) SSIM, one workgroup per
// (t, 32x32 tile), which first folds image t's four range slots and writes its sum to slot (t, tile); (3) one
// workgroup per image folds slots and tile sums in index order and applies the formulas.  The split depends on (h, w)
// only and no workgroup reads another image's slots, so a row does not depend on n or on the image's position.
// ------------------------------------------------------------------------------------------
namespace {
constexpr int PI_PIX = 2048;  // pixels per workgroup of the fused pass (8 per thread)
constexpr long PI_MAX_GROUPS = 1L << 23;  // 256-thread workgroups per launch: thread ids stay below 2^31
inline long pi_blocks(int h, int w) { return ((long)h * w + PI_PIX - 1) / PI_PIX; }
inline long pi_tiles(int h, int w) {
  return (long)((h - 2 * SSIM_R + SSIM_T - 1) / SSIM_T) * ((w - 2 * SSIM_R + SSIM_T - 1) / SSIM_T);
}
}  // namespace

// Slot k over the nb block partials of one image: lane l folds partials l, l + 64, ... in index order, then the fixed
// shuffle tree.  Whole wave; valid in lane 0.
__device__ __forceinline__ double pi_fold(const double* __restrict__ part, int nb, int k, int lane) {
  double x = k < P_NSUM ? 0.0 : ((k - P_NSUM) % 2 == 0 ? (double)INFINITY : -(double)INFINITY);
  for (int b = lane; b < nb; b += 64) x = combine(k, x, part[(long)b * P_SLOTS + k]);
  for (int o = 32; o > 0; o >>= 1) x = combine(k, x, __shfl_down(x, o));
  return x;
}

__global__ void __launch_bounds__(256) pi_partial_kernel(ClimsrMetricsDesc d, int nb, long stride) {
  const int t = blockIdx.x / nb, b = blockIdx.x - t * nb;
  const long hw = (long)d.h * d.w, base = (long)t * hw;
  PixelAcc a;
  acc_init(a);
  Denorm dn_cache;
  for (long p = (long)b * 256 + threadIdx.x; p < hw; p += (long)nb * 256) {
    float pn, tn;
    double pd, td;
    masked_values_at(d, base + p, t, dn_cache, pn, tn, pd, td);
    acc_pixel(d, a, pn, tn, pd, td);
  }
  acc_block_store(a, d.workspace + (long)t * stride + (long)b * P_SLOTS);
}

__global__ void __launch_bounds__(256) pi_ssim_kernel(ClimsrMetricsDesc d, int nb, int tiles, long stride) {
  __shared__ SsimLds L;
  __shared__ double rng[4];
  const int tiles_x = (d.w - 2 * SSIM_R + SSIM_T - 1) / SSIM_T;
  const int t = blockIdx.x / tiles, r = blockIdx.x - t * tiles;
  double* img = d.workspace + (long)t * stride;
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  ssim_gaussian(L);
  const double x = pi_fold(img, nb, P_PN_MIN + wv, lane);  // wave 0..3: pn min, pn max, tn min, tn max
  if (lane == 0) rng[wv] = x;
  __syncthreads();
  float c1, c2;
  ssim_consts(rng[0], rng[1], rng[2], rng[3], c1, c2);
  double part = 0.0;
  ssim_tile(d, L, t, (r / tiles_x) * SSIM_T, (r % tiles_x) * SSIM_T, c1, c2, part);
  const double sum = ssim_block_sum(L, part);
  if (threadIdx.x == 0) img[(long)nb * P_SLOTS + r] = sum;
}

__global__ void __launch_bounds__(256) pi_final_kernel(ClimsrMetricsDesc d, int nb, int tiles, long stride) {
  __shared__ double s[P_SLOTS + 1];
  const int t = blockIdx.x;
  const double* img = d.workspace + (long)t * stride;
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int k = wv; k <= P_SLOTS; k += 4) {  // k == P_SLOTS: the SSIM tile sums
    double x;
    if (k < P_SLOTS) {
      x = pi_fold(img, nb, k, lane);
    } else {
      x = 0.0;
      for (int i = lane; i < tiles; i += 64) x += img[(long)nb * P_SLOTS + i];
      for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o);
    }
    if (lane == 0) s[k] = x;
  }
  __syncthreads();
  if (threadIdx.x == 0) metrics_formulas(d, s, s[P_SLOTS], 1, d.out + (long)t * CLIMSR_SR_METRICS);
}

extern "C" size_t climsr_sr_metrics_per_image_workspace(int n, int h, int w) {
  if (n <= 0 || h < SSIM_K || w < SSIM_K) return 0;
  return (size_t)n * (size_t)(pi_blocks(h, w) * P_SLOTS + pi_tiles(h, w)) * sizeof(double);
}

extern "C" int climsr_sr_metrics_per_image(const ClimsrMetricsDesc* d, void* stream) {
  if (!d || !d->sr || !d->hr || !d->original || !d->mask || !d->workspace || !d->out || d->n <= 0 ||
      d->h < SSIM_K || d->w < SSIM_K || (d->method == 0 && (!d->min || !d->max)) || d->method < 0 || d->method > 2) {
    set_error("sr_metrics_per_image: bad args (h, w >= %d for the 11x11 SSIM window; min/max needed for minmax)", SSIM_K);
    return CLIMSR_EINVAL;
  }
  const long nb = pi_blocks(d->h, d->w), tiles = pi_tiles(d->h, d->w);
  if (d->n * nb > PI_MAX_GROUPS || d->n * tiles > PI_MAX_GROUPS) {
    set_error("sr_metrics_per_image: n=%d images of %dx%d need more than %ld workgroups per launch; split the batch", d->n,
              d->h, d->w, PI_MAX_GROUPS);
    return CLIMSR_EINVAL;
  }
  hipStream_t s = (hipStream_t)stream;
  const ClimsrMetricsDesc dd = *d;
  const long stride = nb * P_SLOTS + tiles;
  hipLaunchKernelGGL(pi_partial_kernel, dim3((unsigned)(d->n * nb)), dim3(256), 0, s, dd, (int)nb, stride);
  hipLaunchKernelGGL(pi_ssim_kernel, dim3((unsigned)(d->n * tiles)), dim3(256), 0, s, dd, (int)nb, (int)tiles, stride);
  hipLaunchKernelGGL(pi_final_kernel, dim3(d->n), dim3(256), 0, s, dd, (int)nb, (int)tiles, stride);
  return check_launch("sr_metrics_per_image");
}

// ------------------------------------------------------------------------------------------
// RegressionAccuracy.update (climsr/metrics/regression_accuracy.py:15-19): count |p - t| <= eps in
// the inputs' float32 arithmetic; int64 counters (exact, order-independent).
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) regression_accuracy_kernel(const float* __restrict__ p, const float* __restrict__ t,
                                                                  long n, float eps, unsigned long long* counts) {
  unsigned long long c = 0;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    c += (fabsf(p[i] - t[i]) <= eps) ? 1ull : 0ull;
  for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(counts, c);
  if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(counts + 1, (unsigned long long)n);
}

extern "C" int climsr_regression_accuracy_update(const float* preds, const float* target, int64_t n, float eps, int64_t* counts,
                                                 void* stream) {
  if (!preds || !target || !counts || n < 0) {
    set_error("regression_accuracy: bad args");
    return CLIMSR_EINVAL;
  }
  if (n == 0) return 0;
  int blocks = (int)((n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024);
  hipLaunchKernelGGL(regression_accuracy_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, preds, target, (long)n, eps,
                     (unsigned long long*)counts);
  return check_launch("regression_accuracy");
}

// ------------------------------------------------------------------------------------------
// Inference output (inference.py:73-80): MinMaxScaler.denormalize of the SR map with the grid's float64
// min / max (numpy float64 arithmetic, one rounding to float32 at the end), NaN where the land mask is 0.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void denormalize_mask_kernel(const float* __restrict__ sr, const float* __restrict__ mask,
                                                               const double* __restrict__ mn, const double* __restrict__ mx,
                                                               double a, double b, double eps, long hw, long total,
                                                               float* __restrict__ out) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int t = (int)(i / hw);
  const double scale = __ddiv_rn(b - a, __dadd_rn(__dsub_rn(mx[t], mn[t]), eps));
  const double add = __dsub_rn(a, __dmul_rn(mn[t], scale));
  const float v = (float)__ddiv_rn(__dsub_rn((double)sr[i], add), scale);
  out[i] = (mask && mask[i] == 0.f) ? NAN : v;
}

extern "C" int climsr_denormalize_mask(const float* sr, const float* mask, const double* min, const double* max, double range_a,
                                       double range_b, int n, int64_t hw, float* out, void* stream) {
  if (!sr || !min || !max || !out || n <= 0 || hw <= 0) {
    set_error("denormalize_mask: bad args");
    return CLIMSR_EINVAL;
  }
  const long total = (long)n * hw;
  hipLaunchKernelGGL(denormalize_mask_kernel, dim3(ceil_div(total, 256)), dim3(256), 0, (hipStream_t)stream, sr, mask, min, max,
                     range_a, range_b, 1e-8, (long)hw, total, out);
  return check_launch("denormalize_mask");
}

// ------------------------------------------------------------------------------------------
// Inference front end: GeoTiffInferenceDataset (geo_tiff_inference_dataset.py:74-96 once per dataset, :98-176 per
// grid) and CRUTSInferenceDataset (cruts_inference_dataset.py:68-107).  Normalisation is element-wise, so the flip
// and the nearest upscale are index maps applied on the way: one thread per HR output pixel reads its raw LR
// pixel, normalises it and writes every output it owns.
// ------------------------------------------------------------------------------------------
namespace {
constexpr long INFER_MAX_THREADS = 1L << 31;  // 2^23 workgroups of 256: block ids and ceil_div stay in int
}

// mask_hr = ~np.isnan(land); elev_hr = np.where(mask, elev, nan), the plane the nanmin / nanmax pass reads.
__global__ void __launch_bounds__(256) infer_static_mask_kernel(const float* __restrict__ elev, const float* __restrict__ land,
                                                                long total, float* __restrict__ elev_hr,
                                                                float* __restrict__ mask_hr) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const bool is_land = !isnan(land[i]);
  mask_hr[i] = is_land ? 1.f : 0.f;
  elev_hr[i] = is_land ? elev[i] : NAN;
}

// elevation_scaler.normalize(masked, missing_indicator=...) in place, and the [::s, ::s] samples of both planes.
__global__ void __launch_bounds__(256) infer_static_norm_kernel(float* __restrict__ elev_hr, const float* __restrict__ mask_hr,
                                                                const float* __restrict__ minmax, int hr_h, int hr_w, int s,
                                                                double a, double b, double eps, int method, float missing,
                                                                double zs_mean, double zs_std, double zs_nan_sub,
                                                                float* __restrict__ elev_lr, float* __restrict__ mask_lr) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)hr_h * hr_w) return;
  const int y = (int)(i / hr_w), x = (int)(i - (long)y * hr_w);
  float v = elev_hr[i];
  if (v == missing) v = NAN;  // `out_arr[arr == missing_indicator] = np.nan`
  if (method == 0) v = minmax_f32(v, minmax_f32_params(minmax[0], minmax[1], a, b, eps), 0.f);
  else if (method == 1) v = zscore_f64(v, zs_mean, zs_std, eps, zs_nan_sub);
  elev_hr[i] = v;
  if (y % s == 0 && x % s == 0) {
    const long lo = (long)(y / s) * (hr_w / s) + x / s;
    elev_lr[lo] = v;
    mask_lr[lo] = mask_hr[i];
  }
}

extern "C" int climsr_infer_static(const float* elev_raw, const float* land_raw, int hr_h, int hr_w, int scale, double range_a,
                                   double range_b, int method, float elev_missing, double zs_mean, double zs_std,
                                   double zs_nan_sub, float* minmax, float* elev_hr, float* mask_hr, float* elev_lr,
                                   float* mask_lr, void* stream) {
  if (!elev_raw || !land_raw || !elev_hr || !mask_hr || !elev_lr || !mask_lr) {
    set_error("infer_static: null pointer (elevation, land raster and the four output planes are required)");
    return CLIMSR_EINVAL;
  }
  if (hr_h <= 0 || hr_w <= 0 || scale <= 0 || hr_h % scale || hr_w % scale) {
    set_error("infer_static: %dx%d must be positive multiples of scale %d", hr_h, hr_w, scale);
    return CLIMSR_EINVAL;
  }
  if (method < 0 || method > 2) {
    set_error("infer_static: method %d outside 0..2", method);
    return CLIMSR_EINVAL;
  }
  if (method == 0 && !minmax) {
    set_error("infer_static: min-max normalisation needs the 2-float minmax scratch");
    return CLIMSR_EINVAL;
  }
  if (elev_hr == elev_raw) {
    set_error("infer_static: elev_hr stages the masked elevation and must not alias elev_raw");
    return CLIMSR_EINVAL;
  }
  const long total = (long)hr_h * hr_w;
  if (total > INFER_MAX_THREADS) {
    set_error("infer_static: %dx%d pixels overflow one launch (limit 2^31)", hr_h, hr_w);
    return CLIMSR_EINVAL;
  }
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(infer_static_mask_kernel, dim3(ceil_div(total, 256)), dim3(256), 0, s, elev_raw, land_raw, total, elev_hr,
                     mask_hr);
  if (method == 0)
    hipLaunchKernelGGL(tile_minmax_kernel, dim3(1), dim3(1024), 0, s, (const float*)elev_hr, total, elev_missing, 1, minmax);
  hipLaunchKernelGGL(infer_static_norm_kernel, dim3(ceil_div(total, 256)), dim3(256), 0, s, elev_hr, (const float*)mask_hr,
                     (const float*)minmax, hr_h, hr_w, scale, range_a, range_b, 1e-8, method, elev_missing, zs_mean, zs_std,
                     zs_nan_sub, elev_lr, mask_lr);
  return check_launch("infer_static");
}

__global__ void __launch_bounds__(256) infer_prepare_kernel(ClimsrInferDesc d) {
  const int hw = d.hr_h * d.hr_w;
  long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (long)d.n * hw) return;
  const int t = (int)(gid / hw);
  const int rem = (int)(gid - (long)t * hw);
  const int y = rem / d.hr_w, x = rem - (rem / d.hr_w) * d.hr_w;
  const int s = d.scale, ly = y / s, lx = x / s;
  const int sy = d.flip_ud ? d.h - 1 - ly : ly;  // np.flipud(raw)
  const float raw = d.lr_raw[((long)t * d.h + sy) * d.w + lx];

  double mn = 0.0, mx = 0.0;  // what the grid is normalised with, as the batch's float64 min / max items
  float v = raw;
  if (d.lr_min) {  // scaler.normalize(img, min, max) with np.float64 min / max: float64, one rounding
    mn = d.lr_min[t];
    mx = d.lr_max[t];
    if (d.method == 0) {
      const double hs = __ddiv_rn(d.range_b - d.range_a, __dadd_rn(__dsub_rn(mx, mn), d.eps));
      v = minmax_f64(raw, hs, __dsub_rn(d.range_a, __dmul_rn(mn, hs)), (float)d.nan_sub);
    }
  } else if (d.lr_minmax) {  // scaler.normalize(img): np.nanmin / np.nanmax of the float32 grid, float32 throughout
    const float fmn = d.lr_minmax[2 * t], fmx = d.lr_minmax[2 * t + 1];
    mn = (double)fmn;
    mx = (double)fmx;
    if (d.method == 0) v = minmax_f32(raw, minmax_f32_params(fmn, fmx, d.range_a, d.range_b, d.eps), (float)d.nan_sub);
  }
  if (d.method == 1) v = zscore_f64(raw, d.zs_mean, d.zs_std, d.eps, d.zs_nan_sub);
  if (rem == 0 && (d.lr_min || d.lr_minmax)) {
    d.out_min[t] = mn;
    d.out_max[t] = mx;
  }

  d.nearest[(long)t * hw + rem] = v;  // nearest x s of the LR grid: out[y][x] = lr[y / s][x / s]
  if (d.srcnn) {                      // _concat_if_needed, SRCNN branch: [nearest, elevation, mask] at HR size
    float* l = d.lr + (long)t * d.lr_c * hw + rem;
    int c = 0;
    l[(long)(c++) * hw] = v;
    if (d.use_elev) l[(long)(c++) * hw] = d.elev_hr[rem];
    if (d.use_mask) l[(long)(c++) * hw] = d.mask_hr[rem];
  } else if (ly * s == y && lx * s == x) {  // [lr, elevation_lr, mask_lr] at LR size
    const int lhw = d.h * d.w, lo = ly * d.w + lx;
    float* l = d.lr + (long)t * d.lr_c * lhw + lo;
    int c = 0;
    l[(long)(c++) * lhw] = v;
    if (d.use_elev) l[(long)(c++) * lhw] = d.elev_lr[lo];
    if (d.use_mask) l[(long)(c++) * lhw] = d.mask_lr[lo];
  }
}

extern "C" int climsr_infer_prepare(const ClimsrInferDesc* d, void* stream) {
  if (!d || !d->lr_raw || !d->lr || !d->nearest) {
    set_error("infer_prepare: null pointer (desc, lr_raw, lr and nearest are required)");
    return CLIMSR_EINVAL;
  }
  if (d->n <= 0 || d->h <= 0 || d->w <= 0 || d->scale <= 0 || (long)d->scale * d->h != d->hr_h ||
      (long)d->scale * d->w != d->hr_w) {
    set_error("infer_prepare: HR size %dx%d is not scale %d x the LR grid %dx%d (n=%d)", d->hr_h, d->hr_w, d->scale, d->h, d->w,
              d->n);
    return CLIMSR_EINVAL;
  }
  if (d->method < 0 || d->method > 2) {
    set_error("infer_prepare: method %d outside 0..2", d->method);
    return CLIMSR_EINVAL;
  }
  const int want_c = 1 + (d->use_elev ? 1 : 0) + (d->use_mask ? 1 : 0);
  if (d->lr_c != want_c) {
    set_error("infer_prepare: lr_c=%d, expected 1 + use_elev + use_mask = %d", d->lr_c, want_c);
    return CLIMSR_EINVAL;
  }
  if ((d->lr_min == nullptr) != (d->lr_max == nullptr)) {
    set_error("infer_prepare: lr_min and lr_max come together");
    return CLIMSR_EINVAL;
  }
  const int routes = (d->lr_min ? 1 : 0) + (d->lr_minmax ? 1 : 0);
  if (routes > 1 || (d->method == 0 && routes != 1)) {
    set_error("infer_prepare: %d statistics routes given; min-max needs exactly one of lr_min / lr_max and lr_minmax", routes);
    return CLIMSR_EINVAL;
  }
  if (routes && (!d->out_min || !d->out_max)) {
    set_error("infer_prepare: null out_min / out_max (required with a statistics route)");
    return CLIMSR_EINVAL;
  }
  if ((d->use_elev && !(d->srcnn ? d->elev_hr : d->elev_lr)) || (d->use_mask && !(d->srcnn ? d->mask_hr : d->mask_lr))) {
    set_error("infer_prepare: null static plane (the %s elevation / mask of climsr_infer_static)", d->srcnn ? "HR" : "LR");
    return CLIMSR_EINVAL;
  }
  const long hw = (long)d->hr_h * d->hr_w;
  if (hw > 0x7fffffffL || d->n > INFER_MAX_THREADS / hw) {
    set_error("infer_prepare: n=%d grids of %dx%d overflow one launch (limit 2^31 HR pixels); split the batch", d->n, d->hr_h,
              d->hr_w);
    return CLIMSR_EINVAL;
  }
  hipLaunchKernelGGL(infer_prepare_kernel, dim3(ceil_div(d->n * hw, 256)), dim3(256), 0, (hipStream_t)stream, *d);
  return check_launch("infer_prepare");
}
