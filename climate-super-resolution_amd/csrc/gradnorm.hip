// Gradient norms over a flat gradient buffer (torch.nn.utils.clip_grad_norm_ / Lightning's track_grad_norm): one
// deterministic segmented reduction gives every parameter's norm, the total, the clip coefficient and a finite flag,
// all left on the device.  Three launches whatever the number of segments:
//   1. items:   one block scans ceil(len_s / CHUNK) over the segments -> item_prefix[nseg + 1]
//   2. partial: block b = work item b finds its segment by binary search in item_prefix and reduces its <= CHUNK
//               elements (never crossing a segment) in fp64; 16 B loads between a scalar head and tail, so a segment
//               may start at any element offset
//   3. final:   one block; each wave folds one segment's items (lane-strided in index order, then a fixed shuffle
//               tree), then the block folds the segments the same way into the total and writes the coefficient
// No floating-point atomics and no order that depends on scheduling: a rerun is bit-identical.
#include <math.h>

#include "common.h"

using namespace climsr;

namespace {

constexpr long GN_CHUNK = 8192;  // elements per work item: 32 KB, 8 x 16 B per lane of a 256-thread block
constexpr int GN_FINAL_THREADS = 1024;

__device__ __forceinline__ double gn_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

// kind 0: a + b.  kind 1: max(a, b) with NaN propagated (fmax alone would drop it).
__device__ __forceinline__ double gn_fold(double a, double b, int kind) {
  if (kind == 0) return a + b;
  return (a != a || b != b) ? gn_nan() : fmax(a, b);
}

__device__ __forceinline__ double gn_term(float x, int kind) {
  const double d = (double)x;
  return kind == 0 ? d * d : fabs(d);  // |NaN| stays NaN
}

__device__ __forceinline__ double gn_wave_fold(double v, int kind) {
  for (int o = 32; o > 0; o >>= 1) v = gn_fold(v, __shfl_down(v, o), kind);
  return v;  // lane 0 holds the wave's value
}

__device__ __forceinline__ long gn_clamp(long v, long n) { return v < 0 ? 0 : (v > n ? n : v); }

__device__ __forceinline__ long gn_items(const int64_t* seg_off, int s, long n) {
  const long lo = gn_clamp(seg_off[s], n), hi = gn_clamp(seg_off[s + 1], n);
  return hi > lo ? (hi - lo + GN_CHUNK - 1) / GN_CHUNK : 0;
}

// item_prefix[s] = work items of the segments before s; item_prefix[nseg] = all of them.  One block of 256 threads:
// thread t owns a contiguous run of segments.
__global__ void gn_items_kernel(const int64_t* __restrict__ seg_off, int nseg, long n, int64_t* __restrict__ item_prefix) {
  __shared__ long run_sum[256];
  const int per = (nseg + 255) / 256;
  const int s0 = min(nseg, (int)threadIdx.x * per), s1 = min(nseg, s0 + per);
  long mine = 0;
  for (int s = s0; s < s1; ++s) mine += gn_items(seg_off, s, n);
  run_sum[threadIdx.x] = mine;
  __syncthreads();
  long base = 0;
  for (int t = 0; t < (int)threadIdx.x; ++t) base += run_sum[t];
  for (int s = s0; s < s1; ++s) {
    item_prefix[s] = base;
    base += gn_items(seg_off, s, n);
  }
  if (threadIdx.x == 255) item_prefix[nseg] = base;  // the last thread's run ends at nseg (possibly empty)
}

__global__ void __launch_bounds__(256) gn_partial_kernel(const float* __restrict__ g, long n, const int64_t* __restrict__ seg_off,
                                                         int nseg, int kind, const int64_t* __restrict__ item_prefix,
                                                         double* __restrict__ partial) {
  __shared__ double sh[4];
  const long b = blockIdx.x;
  if (b >= item_prefix[nseg]) return;  // the grid is the host's upper bound ceil(n / CHUNK) + nseg
  int lo = 0, hi = nseg;               // last s with item_prefix[s] <= b (segments without items share a prefix)
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (item_prefix[mid] <= b) lo = mid; else hi = mid;
  }
  const long seg_lo = gn_clamp(seg_off[lo], n), seg_hi = gn_clamp(seg_off[lo + 1], n);
  const long start = seg_lo + (b - item_prefix[lo]) * GN_CHUNK;
  if (start >= seg_hi) return;  // unreachable with ascending offsets; keeps every read inside [0, n)
  const long len = min(GN_CHUNK, seg_hi - start);
  const float* p = g + start;
  const int t = threadIdx.x;
  long head = (long)((16 - ((uintptr_t)p & 15)) & 15) >> 2;  // elements before the first 16 B boundary
  if (head > len) head = len;
  const long nvec = (len - head) >> 2;
  const long tail0 = head + nvec * 4;
  double acc = 0.0;  // the identity of both folds (|x| >= 0)
  if (t < head) acc = gn_fold(acc, gn_term(p[t], kind), kind);
  const float4* pv = (const float4*)(p + head);
#pragma unroll 4
  for (long i = t; i < nvec; i += 256) {  // a full item: 8 independent 16 B loads per lane
    const float4 q = pv[i];
    acc = gn_fold(acc, gn_term(q.x, kind), kind);
    acc = gn_fold(acc, gn_term(q.y, kind), kind);
    acc = gn_fold(acc, gn_term(q.z, kind), kind);
    acc = gn_fold(acc, gn_term(q.w, kind), kind);
  }
  if (tail0 + t < len) acc = gn_fold(acc, gn_term(p[tail0 + t], kind), kind);
  acc = gn_wave_fold(acc, kind);
  if ((t & 63) == 0) sh[t >> 6] = acc;
  __syncthreads();
  if (t == 0) partial[b] = gn_fold(gn_fold(gn_fold(sh[0], sh[1], kind), sh[2], kind), sh[3], kind);
}

__global__ void __launch_bounds__(GN_FINAL_THREADS) gn_final_kernel(int nseg, int kind, double max_norm,
                                                                    const int64_t* __restrict__ item_prefix,
                                                                    const double* __restrict__ partial, double* seg_val,
                                                                    double* __restrict__ norms, float* __restrict__ clip) {
  __shared__ double sh[GN_FINAL_THREADS / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  constexpr int WAVES = GN_FINAL_THREADS / 64;
  for (int s = wave; s < nseg; s += WAVES) {
    const long i0 = item_prefix[s], i1 = item_prefix[s + 1];
    double acc = 0.0;
    for (long i = i0 + lane; i < i1; i += 64) acc = gn_fold(acc, partial[i], kind);
    acc = gn_wave_fold(acc, kind);
    if (lane == 0) {
      seg_val[s] = acc;
      norms[s] = kind == 0 ? sqrt(acc) : acc;
    }
  }
  __syncthreads();  // seg_val written by this block's waves, read back below
  double acc = 0.0;
  for (int s = threadIdx.x; s < nseg; s += GN_FINAL_THREADS) acc = gn_fold(acc, seg_val[s], kind);
  acc = gn_wave_fold(acc, kind);
  if (lane == 0) sh[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double tot = sh[0];
    for (int w = 1; w < WAVES; ++w) tot = gn_fold(tot, sh[w], kind);
    if (kind == 0) tot = sqrt(tot);
    norms[nseg] = tot;
    // torch.nn.utils.clip_grad_norm_: clamp(max_norm / (total + 1e-6), max=1); a NaN stays NaN, inf gives 0
    double c = 1.0;
    if (max_norm > 0.0) {
      c = max_norm / (tot + 1e-6);
      if (c > 1.0) c = 1.0;
    }
    clip[0] = (float)c;
    clip[1] = (tot - tot == 0.0) ? 1.f : 0.f;  // finite
  }
}

__global__ void scale_kernel(float* __restrict__ g, long n, const float* __restrict__ coef, int vec) {
  const float c = coef[0];
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (vec) {
    const long i4 = i * 4;
    if (i4 + 3 < n) {
      float4 q = *(float4*)(g + i4);
      q.x *= c; q.y *= c; q.z *= c; q.w *= c;
      *(float4*)(g + i4) = q;
    } else {
      for (long k = i4; k < n; ++k) g[k] *= c;
    }
  } else if (i < n) {
    g[i] *= c;
  }
}

}  // namespace

extern "C" int64_t climsr_grad_norm_chunk(void) { return GN_CHUNK; }

// item_prefix int64[nseg + 1] | partial double[ceil(n / CHUNK) + nseg] | seg_val double[nseg]
extern "C" int64_t climsr_grad_norm_workspace(int64_t n, int32_t nseg) {
  if (n <= 0 || nseg <= 0) return 0;
  return 8 * ((int64_t)nseg + 1 + (n + GN_CHUNK - 1) / GN_CHUNK + nseg + nseg);
}

extern "C" int climsr_grad_norm(const float* g, int64_t n, const int64_t* seg_off, int32_t nseg, int32_t kind, double max_norm,
                                void* workspace, double* norms, float* clip, void* stream) {
  if (!g || !seg_off || !workspace || !norms || !clip || n <= 0 || nseg <= 0 || (kind != 0 && kind != 1)) {
    set_error("grad_norm: bad args");
    return CLIMSR_EINVAL;
  }
  const int64_t max_items = (n + GN_CHUNK - 1) / GN_CHUNK + nseg;
  if (max_items > 0x7fffffffLL) {
    set_error("grad_norm: too many work items for one grid");
    return CLIMSR_EINVAL;
  }
  hipStream_t s = (hipStream_t)stream;
  int64_t* item_prefix = (int64_t*)workspace;
  double* partial = (double*)(item_prefix + nseg + 1);
  double* seg_val = partial + max_items;
  hipLaunchKernelGGL(gn_items_kernel, dim3(1), dim3(256), 0, s, seg_off, (int)nseg, (long)n, item_prefix);
  hipLaunchKernelGGL(gn_partial_kernel, dim3((unsigned)max_items), dim3(256), 0, s, g, (long)n, seg_off, (int)nseg, (int)kind,
                     (const int64_t*)item_prefix, partial);
  hipLaunchKernelGGL(gn_final_kernel, dim3(1), dim3(GN_FINAL_THREADS), 0, s, (int)nseg, (int)kind, max_norm,
                     (const int64_t*)item_prefix, (const double*)partial, seg_val, norms, clip);
  return check_launch("grad_norm");
}

extern "C" int climsr_scale_f32(float* g, int64_t n, const float* coef, void* stream) {
  if (!g || !coef || n <= 0) {
    set_error("scale_f32: bad args");
    return CLIMSR_EINVAL;
  }
  const int vec = ((uintptr_t)g % 16 == 0);
  const long threads = vec ? (n + 3) / 4 : n;
  hipLaunchKernelGGL(scale_kernel, dim3(ceil_div(threads, 256)), dim3(256), 0, (hipStream_t)stream, g, (long)n, coef, vec);
  return check_launch("scale_f32");
}
