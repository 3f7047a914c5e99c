#include "conv_fwd_kernel.h"

using namespace climsr;

// ------------------------------------------------------------------------------------------
// Weights-resident persistent conv: one workgroup per CU stages the WHOLE packed weight matrix
// (<= 64 output channels, one channel chunk) into LDS once and walks its share of the output tiles,
// the next tile's input prefetched into registers while the current one is on the MFMA pipe.  For the
// HR-resolution convs (HRconv / upconv1-2 with the upsample on load, srcnn.conv1 9x9 and conv2 5x5,
// their data gradients, trunk_conv / conv_first) the generic kernel restages the weights for every
// 256-pixel tile (8k tiles per launch at 256^2).  Stride 1 only; epilogue = the generic one.
// ------------------------------------------------------------------------------------------
// GEO = 1: 3x3 taps over one 64-channel chunk with 8 waves x 2 rows (the 64 -> 64 HR-resolution / VGG conv1_2
// shapes): the 18 k-steps unrolled with compile-time LDS offsets (no tap table; see conv_fwd_kernel's GEO)
template <int NW, int MW, int NT, bool RF, int PV, int EP = 0, int GEO = 0>
__global__ __launch_bounds__(64 * NW, 1) void conv_pw_kernel(FwdArgs a) {
  constexpr int NTHR = 64 * NW;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int* tab = (int*)smem;
  uint16_t* ws = (uint16_t*)(smem + a.lds_tab);
  uint16_t* xs = (uint16_t*)(smem + a.lds_tab + a.lds_x);  // lds_x carries the weight region size here
  float* ebase = (float*)xs;                               // epilogue staging aliases the input tile

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, col = lane & 15;
  const int wpitch = a.kcpad + WPAD;
  const int ks2 = a.ks * a.ks;
  if constexpr (GEO == 2) {  // 4-channel taps: table of tap offsets, one per 4 k values
    for (int i = tid; i < a.kcpad / 4; i += NTHR) {
      const int tap = i < ks2 ? i : 0, ky = tap / a.ks, kx = tap - ky * a.ks;
      tab[i] = (ky * a.tpw + kx) * a.ccp;
    }
  }
  for (int i = tid; i < (GEO ? 0 : a.kcpad / 8); i += NTHR) {  // tap table (one chunk)
    const int kr = i * 8;
    int tap = kr / a.cc, c = kr - tap * a.cc;
    if (tap >= ks2) { tap = 0; c = 0; }
    const int ky = tap / a.ks, kx = tap - ky * a.ks;
    tab[i] = (ky * a.tpw + kx) * a.ccp + c;
  }
  {  // the whole weight matrix, once: 8 vectors per thread in flight per batch (buffer loads, no branch)
    const int wvec_row = a.kcpad / 8, nvw = NT * 16 * wvec_row;
    const __amdgpu_buffer_rsrc_t wr = buf_rsrc(a.w, 0xFFFFFFFFu);
    for (int v0 = 0; v0 < nvw; v0 += 8 * NTHR) {
      uint4 wv[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int v = v0 + tid + i * NTHR;
        const int r = v / wvec_row, kv = v - r * wvec_row;
        wv[i] = buf_load16(wr, v < nvw ? (uint32_t)((r * a.kpk + kv * 8) * 2) : 0u);
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int v = v0 + tid + i * NTHR;
        const int r = v / wvec_row, kv = v - r * wvec_row;
        if (v < nvw) *(uint4*)(ws + r * wpitch + kv * 8) = wv[i];
      }
    }
  }
  const int ufac = a.up, upsh = a.up == 2 ? 1 : 0;
  const int lh = a.in_h * ufac, lw = a.in_w * ufac;
  const int cvec = a.cc / 8;
  const int nvec_x = a.tph * a.tpw * cvec;
  const int x_dp = NTHR / cvec, x_dc = NTHR - x_dp * cvec;
  const int x_dy = x_dp / a.tpw, x_dx = x_dp - x_dy * a.tpw;
  const int x_pix0 = tid / cvec, x_cg0 = tid - x_pix0 * cvec;
  const int x_ty0 = x_pix0 / a.tpw, x_tx0 = x_pix0 - x_ty0 * a.tpw;
  const int ntiles = a.tiles_x * a.tiles_y * a.n;

  uint4 pre[PV];
  // buffer loads (zeros out of range) and an unconditional call: the next tile's loads stay in flight
  // through this tile's compute (see conv_n16_kernel)
  const __amdgpu_buffer_rsrc_t xr = buf_rsrc(a.x, (uint32_t)((long)a.n * a.in_h * a.in_w * a.in_cs * 2));
  // tile coordinates advance incrementally by the walk's step (no per-tile integer divisions: wave-uniform
  // divisions by runtime tile counts cost ~40 SALU each, 8 per tile, on the CU's shared scalar pipe)
  auto issue = [&](bool live, int tx, int ty, int nimg) {  // !live: nothing to load
    const int iy0 = ty * (NW * MW) - a.pad, ix0 = tx * TW - a.pad;
    int ty_ = x_ty0, tx_ = x_tx0, cg = x_cg0;
#pragma unroll
    for (int i = 0; i < PV; ++i) {
      {
        const int iy = iy0 + ty_, ix = ix0 + tx_;
        const int c = cg * 8;
        const bool ok = live && tid + NTHR * i < nvec_x && iy >= 0 && iy < lh && ix >= 0 && ix < lw && c < a.in_c;
        const uint32_t off = (uint32_t)((((nimg * a.in_h + (iy >> upsh)) * a.in_w + (ix >> upsh)) * a.in_cs + a.in_co + c) * 2);
        pre[i] = buf_load16(xr, ok ? off : BUF_OOB);
      }
      cg += x_dc;
      tx_ += x_dx;
      ty_ += x_dy;
      if (cg >= cvec) { cg -= cvec; ++tx_; }
      if (tx_ >= a.tpw) { tx_ -= a.tpw; ++ty_; }
    }
  };
  const TileWalk walk(ntiles);
  const int s_x = walk.step % a.tiles_x, s_y = (walk.step / a.tiles_x) % a.tiles_y, s_n = walk.step / (a.tiles_x * a.tiles_y);
  auto advance = [&](int& tx, int& ty, int& n) {
    tx += s_x;
    int c = tx >= a.tiles_x;
    tx -= c ? a.tiles_x : 0;
    ty += s_y + c;
    c = ty >= a.tiles_y;
    ty -= c ? a.tiles_y : 0;
    n += s_n + c;
  };
  int ctx = walk.first % a.tiles_x, cty = (walk.first / a.tiles_x) % a.tiles_y, cn = walk.first / (a.tiles_x * a.tiles_y);
  if (walk.first < walk.end) issue(true, ctx, cty, cn);

  int pixbase[MW];
#pragma unroll
  for (int m = 0; m < MW; ++m) pixbase[m] = ((wave * MW + m) * a.tpw + col) * a.ccp;

  for (int tile = walk.first; tile < walk.end; tile += walk.step) {
    const int tx = ctx, ty = cty, nimg = cn;
    advance(ctx, cty, cn);  // the next tile of this workgroup
    const int ox0 = tx * TW, oy0 = ty * (NW * MW);
    lds_barrier();  // previous tile's epilogue reads of the aliased region are done
    {
      int ty_ = x_ty0, tx_ = x_tx0, cg = x_cg0;
#pragma unroll
      for (int i = 0; i < PV; ++i) {
        if (tid + NTHR * i < nvec_x) *(uint4*)(xs + (ty_ * a.tpw + tx_) * a.ccp + cg * 8) = pre[i];
        cg += x_dc;
        tx_ += x_dx;
        ty_ += x_dy;
        if (cg >= cvec) { cg -= cvec; ++tx_; }
        if (tx_ >= a.tpw) { tx_ -= a.tpw; ++ty_; }
      }
    }
    issue(tile + walk.step < walk.end, ctx, cty, cn);  // lands while this tile computes
    lds_barrier();
    f32x4 acc[MW][NT];
#pragma unroll
    for (int m = 0; m < MW; ++m)
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[m][t] = (f32x4){0.f, 0.f, 0.f, 0.f};
    {
      // k-steps two deep: k-step s+1's tap offset and fragments are read while s is on the MFMA pipe (one k-step at
      // a time serialised tab read -> B read -> MFMAs, 3 lgkmcnt waits per 8 MFMAs)
      if constexpr (GEO == 1) {
        static_assert(NW * MW == 16, "GEO 1: 16-row tiles");
        constexpr int TPW = TW + 2, CCP = 80, WP = 9 * 64 + WPAD;
        const uint16_t* xb = xs + ((wave * MW) * TPW + col) * CCP + g * 8;
        const uint16_t* wb = ws + col * WP + g * 8;
        bf16x8 af[2][NT], bf[2][MW];
        auto ldk = [&](int k, int b) {  // k-step k: tap k / 2, channels (k & 1) * 32 + 8 g
          const int tap = k >> 1, off = ((tap / 3) * TPW + tap % 3) * CCP + (k & 1) * 32;
#pragma unroll
          for (int t = 0; t < NT; ++t) af[b][t] = *(const bf16x8*)(wb + t * 16 * WP + k * 32);
#pragma unroll
          for (int m = 0; m < MW; ++m) bf[b][m] = *(const bf16x8*)(xb + m * TPW * CCP + off);
        };
        ldk(0, 0);
#pragma unroll
        for (int k = 0; k < 18; ++k) {
          if (k + 1 < 18) ldk(k + 1, (k + 1) & 1);
          __builtin_amdgcn_sched_barrier(0);  // the next k-step's reads as one burst ahead of this k-step's MFMAs
#pragma unroll
          for (int m = 0; m < MW; ++m)
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[m][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[k & 1][t], bf[k & 1][m], acc[m][t], 0, 0, 0);
          __builtin_amdgcn_sched_barrier(0);
        }
      } else {
      const int nks = a.kcpad / 32;
      bf16x8 afA[NT], bfA[MW], afB[NT], bfB[MW];
      auto ld = [&](int ks, bf16x8 (&af)[NT], bf16x8 (&bf)[MW]) {
#pragma unroll
        for (int t = 0; t < NT; ++t) af[t] = *(const bf16x8*)(ws + (t * 16 + col) * wpitch + ks * 32 + g * 8);
        if constexpr (GEO == 2) {  // k values 8g..8g+7 of the step = taps 8 ks + 2g, +1, 4 channels each
          const int off0 = tab[ks * 8 + 2 * g], off1 = tab[ks * 8 + 2 * g + 1];
#pragma unroll
          for (int m = 0; m < MW; ++m)
            bf[m] = cat_tr(*(const s16x4*)(xs + pixbase[m] + off0), *(const s16x4*)(xs + pixbase[m] + off1));
        } else {
          const int off = tab[ks * 4 + g];
#pragma unroll
          for (int m = 0; m < MW; ++m) bf[m] = *(const bf16x8*)(xs + pixbase[m] + off);
        }
      };
      auto mm = [&](const bf16x8 (&af)[NT], const bf16x8 (&bf)[MW]) {
#pragma unroll
        for (int m = 0; m < MW; ++m)
#pragma unroll
          for (int t = 0; t < NT; ++t) acc[m][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[t], bf[m], acc[m][t], 0, 0, 0);
      };
      ld(0, afA, bfA);
      int ks = 0;
      for (; ks + 2 <= nks; ks += 2) {
        ld(ks + 1, afB, bfB);
        mm(afA, bfA);
        ld(ks + 2 < nks ? ks + 2 : nks - 1, afA, bfA);  // clamped: no branch around the reads
        mm(afB, bfB);
      }
      if (ks < nks) mm(afA, bfA);
      }
    }
    const int ox = ox0 + col;
    if constexpr (EP == 5) {  // 2x2 sum + activation backward (act' of the bf16 low-res activation res1), bf16 out,
                              // 4 channels (8 B) per lane; all operand loads issued before the first store
      const int dh = a.out_h >> 1, dw = a.out_w >> 1;
      const __amdgpu_buffer_rsrc_t rm1 = opt_rsrc(a.res1);
      uint2 r1v[MW / 2][NT];
#pragma unroll
      for (int m = 0; m < MW; m += 2) {
        const int oy = oy0 + wave * MW + m;
        const bool ok = !(col & 1) && oy < a.out_h && ox < a.out_w;
        const long q = ok ? ((long)nimg * dh + (oy >> 1)) * dw + (ox >> 1) : 0;
#pragma unroll
        for (int t = 0; t < NT; ++t) r1v[m / 2][t] = buf_load8(rm1, (uint32_t)((q * a.r1_cs + (ok ? a.r1_co + t * 16 + g * 4 : 0)) * 2));
      }
#pragma unroll
      for (int m = 0; m < MW; m += 2) {
        const int oy = oy0 + wave * MW + m;
        const long pidx = ((long)nimg * dh + (oy >> 1)) * dw + (ox >> 1);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          float v[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            float sm = acc[m][t][i] + acc[m + 1][t][i];
            sm += __shfl_xor(sm, 1);
            v[i] = sm;
          }
          if ((col & 1) || oy >= a.out_h || ox >= a.out_w) continue;
          const uint4 r1 = make_uint4(r1v[m / 2][t].x, r1v[m / 2][t].y, 0, 0);
#pragma unroll
          for (int i = 0; i < 4; ++i) v[i] = ep_res(v[i], a.act, a.slope, true, res4_at(r1, false, i), 1.f, 1.f, false, 0.f, 1.f, 1.f);
          uint2 pk;
          pk.x = (uint32_t)f2bf(v[0]) | ((uint32_t)f2bf(v[1]) << 16);
          pk.y = (uint32_t)f2bf(v[2]) | ((uint32_t)f2bf(v[3]) << 16);
          *(uint2*)((uint16_t*)a.y + pidx * a.out_cs + a.out_co + t * 16 + g * 4) = pk;
        }
      }
      continue;
    }
    if (EP == 0 && a.down2) {  // 2x2 sum (data gradient of the nearest upsample): rows (m, m+1), columns via lane ^ 1
      const int dh = a.out_h >> 1, dw = a.out_w >> 1;
      const bool mask = a.act == 3 || a.act == 4;
#pragma unroll
      for (int m = 0; m < MW; m += 2) {
        const int oy = oy0 + wave * MW + m;
        const long pidx = ((long)nimg * dh + (oy >> 1)) * dw + (ox >> 1);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          float v[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            float sm = acc[m][t][i] + acc[m + 1][t][i];
            sm += __shfl_xor(sm, 1);
            v[i] = sm;
          }
          const int co = t * 16 + g * 4;
          if ((col & 1) || oy >= a.out_h || ox >= a.out_w) continue;
          const long ob = pidx * a.out_cs + a.out_co + co;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            if (co + i >= a.out_c) continue;
            float x = v[i];
            if (mask) x = ep_res(x, a.act, a.slope, true, res_at(a.res1, false, pidx * a.r1_cs + a.r1_co + co + i), 1.f, 1.f, false, 0.f,
                                 1.f, 1.f);
            if (a.out_mode == 0) ((uint16_t*)a.y)[ob + i] = f2bf(x);
            else if (a.out_mode == 2) ((float*)a.y)[ob + i] += x;
            else ((float*)a.y)[ob + i] = x;
            if (a.aux) a.aux[pidx * a.aux_cs + a.aux_co + co + i] = f2bf(a.aux_scale * x);
          }
        }
      }
      continue;
    }
    constexpr int EPP = NT * 16 + 4;
    float* eb = ebase + wave * (MW * 16 * EPP);
    lds_barrier();  // all waves are done reading the input tile (the staging region aliases it)
#pragma unroll
    for (int m = 0; m < MW; ++m)
#pragma unroll
      for (int t = 0; t < NT; ++t) *(f32x4*)(eb + (m * 16 + col) * EPP + t * 16 + g * 4) = acc[m][t];
    lds_barrier();
    store_tile_lds<RF, MW * 16, NT * 16, 64, EP>(a, eb, EPP, lane, nimg, oy0 + wave * MW, ox0, 0);
  }
}

template <int NW, int MW, int NT, int PV, int EP, int GEO>
static int launch_pw_geo(const FwdRoute& r, const FwdArgs& a, hipStream_t s) {
  auto k = r.rf ? conv_pw_kernel<NW, MW, NT, true, PV, EP, GEO> : conv_pw_kernel<NW, MW, NT, false, PV, EP, GEO>;
  if (int e = lds_opt_in((const void*)k, 160 * 1024)) return e;
  const int ncu = device_cus();
  const int ntiles = a.tiles_x * a.tiles_y * a.n;
  const int grid = ntiles < ncu ? ntiles : ncu;
  hipLaunchKernelGGL(k, dim3(grid), dim3(64 * NW), r.pg.lds_total, s, a);
  return check_launch("conv2d_fwd (pw)");
}

// GEO 2 (4-channel taps) runs with the route's PV or 2 staging vectors, GEO 1 exists for the 8-wave form only
template <int NW, int MW, int NT, int PV, int EP = 0>
static int launch_pw(const FwdRoute& r, const FwdArgs& a, hipStream_t s) {
  if (r.geo == 2) return r.pv == 2 ? launch_pw_geo<NW, MW, NT, 2, EP, 2>(r, a, s) : launch_pw_geo<NW, MW, NT, PV, EP, 2>(r, a, s);
  if constexpr (NW * MW == 16) {
    if (r.geo == 1) return launch_pw_geo<NW, MW, NT, PV, EP, 1>(r, a, s);
  }
  return launch_pw_geo<NW, MW, NT, PV, EP, 0>(r, a, s);
}

int climsr::fwd_pw_launch(const FwdRoute& r, const FwdArgs& a, hipStream_t s) {
#define PW_CASE(NW, NT, PV, EP) \
  if (r.nw == NW && r.nt == NT && r.ep == EP) return launch_pw<NW, 2, NT, PV, EP>(r, a, s);
  PW_CASE(8, 4, 7, 0) PW_CASE(8, 4, 7, 3) PW_CASE(8, 4, 7, 4) PW_CASE(8, 4, 7, 5) PW_CASE(8, 4, 7, 6) PW_CASE(8, 4, 7, 7)
  PW_CASE(8, 4, 7, 8) PW_CASE(8, 2, 7, 0) PW_CASE(8, 2, 7, 3) PW_CASE(8, 2, 7, 4) PW_CASE(4, 4, 12, 0) PW_CASE(4, 2, 12, 0)
#undef PW_CASE
  set_error("conv2d_fwd: no conv_pw kernel for nw %d, nt %d, ep %d", r.nw, r.nt, r.ep);
  return CLIMSR_EINVAL;
}

// The generic kernel's 8x16-tile instantiations (MW 2, every epilogue option a runtime flag) are compiled in this unit:
// they and conv_pw's EP 0 forms inline the same store_tile_lds<RF, 32, NT * 16, 64, 0>, and hipcc's interprocedural
// passes run on that helper, with all of the unit's callers in view, before it is inlined -- apart, conv_pw's callers all
// pass co0 = 0 and 21 conv_pw instantiations come out with another instruction order and register allocation.
int climsr::fwd_rows2_launch(const FwdRoute& r, const FwdArgs& a, hipStream_t s) {
  if (r.ep == 0 && r.pfx == 0 && r.geo == 0 && r.nt == 1) return launch_fwd_geo<2, 1, 0, 0, 0, 0>(r, a, s);
  if (r.ep == 0 && r.pfx == 0 && r.geo == 0 && r.nt == 2) return launch_fwd_geo<2, 2, 0, 0, 0, 0>(r, a, s);
  if (r.ep == 0 && r.pfx == 0 && r.geo == 0 && r.nt == 4) return launch_fwd_geo<2, 4, 0, 0, 0, 0>(r, a, s);
  set_error("conv2d_fwd: no 8x16-tile conv_fwd kernel for nt %d, prefetch %d, ep %d, geo %d", r.nt, r.pfx, r.ep, r.geo);
  return CLIMSR_EINVAL;
}
