// The generic forward / data-gradient kernel (conv_fwd_body and its two __global__ forms) with the launcher of one
// instantiation.  Included by the two units that instantiate it: conv_fwd.hip (16x16 tiles, MW 4) and conv_pw.hip (8x16
// tiles, MW 2 -- see there why those live beside conv_pw).
#pragma once
#include "conv_route.h"

// PF > 0: software-pipelined chunks.  Chunk j+1's input and weight vectors (at most PFX + PFW per thread) are
// loaded into registers while chunk j is on the MFMA pipe, so a multi-chunk tile (RDB conv5 / pull-x: four
// 32-channel chunks) pays one staging latency instead of one per chunk.
#ifndef CLIMSR_DIAG_MODE
#define CLIMSR_DIAG_MODE 0  // diagnostic builds only: 4 = GEO k-loop MFMAs without per-k-step fragment reads, 1 = every chunk computed twice, 2 = one staging, compute only,
                            // 3 = staging only (GEO 1)
#endif
// GEO (host-checked geometry specialisation, 0 = runtime geometry): 1 / 2 = 3x3 taps over 32-channel chunks at
// stride 1 / 2 with 16x16 output tiles (MW 4): every tap / row / fragment LDS offset is a compile-time immediate,
// so the unrolled k-steps read their fragments with no address arithmetic and no tap-table lookup (the runtime
// form waited on a dependent ds_read of the table each k-step, and the compiler then issued the fragment reads
// just before their MFMAs: the compute phase alone ran at ~55 % of the MFMA rate).
template <int MW, int NT, bool RF, int MV, int PFX, int PFW, int EP, int GEO>
__device__ __forceinline__ void conv_fwd_body(const FwdArgs& a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int* tab = (int*)smem;
  uint16_t* xs = (uint16_t*)(smem + a.lds_tab);
  uint16_t* ws = (uint16_t*)(smem + a.lds_tab + a.lds_x);

  const int tid = threadIdx.x;
  const int wave = tid >> 6;
  const int lane = tid & 63;
  const int g = lane >> 4;
  const int col = lane & 15;

  // (tile, output-channel block): blockIdx, or with xgrp the XCD-major order in which the xgrp channel blocks of a
  // tile are consecutive on one XCD (the x tile is fetched into that L2 once for all of them, not once per XCD)
  // Stagger: the two workgroups that share a CU run the same program and start together, so they stage (global
  // loads, LDS stores, barriers) and compute (MFMA) in lockstep -- diagnostic builds measured staging + MFMA-only
  // times that simply add (VGG 256 @64^2: 141 + 147 us = 288 us).  The second workgroup of each CU (the second
  // dispatch round, [stag_lo, stag_hi)) starts about half a chunk late; the blocks that replace them inherit the
  // offset.  Speed only: nothing depends on which workgroups share a CU.
  if (a.stag_n && (int)blockIdx.x >= a.stag_lo && (int)blockIdx.x < a.stag_hi)
    for (int i = 0; i < a.stag_n; ++i) __builtin_amdgcn_s_sleep(32);
  int tile_id = blockIdx.x, cob = blockIdx.y;
  if (a.xgrp > 0) {
    const int ntile = a.tiles_x * a.tiles_y * a.n, idx = xcd_major(blockIdx.x, gridDim.x);
    const int grp = idx / (ntile * a.xgrp), rem = idx - grp * (ntile * a.xgrp);
    tile_id = rem / a.xgrp;
    cob = grp * a.xgrp + (rem - tile_id * a.xgrp);
  }
  int bid = tile_id;
  const int tx = bid % a.tiles_x;
  bid /= a.tiles_x;
  const int ty = bid % a.tiles_y;
  const int nimg = bid / a.tiles_y;
  const int ox0 = tx * TW;
  const int oy0 = ty * (4 * MW);
  const int co_blk0 = cob * NT * 16;
  const int wpitch = a.kcpad + WPAD;
  const int ks2 = a.ks * a.ks;

  // tap table: LDS element offset of k-group (8 channels) within a chunk
  for (int i = tid; i < (GEO > 0 ? 0 : a.kcpad / 8); i += 256) {
    int kr = i * 8;
    int tap = kr / a.cc;
    int c = kr - tap * a.cc;
    if (tap >= ks2) { tap = 0; c = 0; }
    int ky = tap / a.ks, kx = tap - (tap / a.ks) * a.ks;
    tab[i] = (ky * a.tpw + kx) * a.ccp + c;
  }

  f32x4 acc[MW][NT];
#pragma unroll
  for (int m = 0; m < MW; ++m)
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[m][t] = (f32x4){0.f, 0.f, 0.f, 0.f};

  int pixbase[MW];
#pragma unroll
  for (int m = 0; m < MW; ++m) pixbase[m] = ((wave * MW + m) * a.stride * a.tpw + col * a.stride) * a.ccp;

  // up = 2: nearest x2 upsample on load (src = j >> 1); up = -2: zero insertion (src = j >> 1 for even j,
  // else 0) = the input of the data gradient of a stride-2 conv
  const int ufac = a.up < 0 ? -a.up : a.up;
  const int lh = a.in_h * ufac, lw = a.in_w * ufac;
  const int iy0 = oy0 * a.stride - a.pad, ix0 = ox0 * a.stride - a.pad;
  const int cvec = a.cc / 8;
  const int dilmask = a.up < 0 ? 1 : 0;
  const int nvec_x = a.tph * a.tpw * cvec;
  const int wvec_row = a.kcpad / 8;
  const int nvec_w = NT * 16 * wvec_row;
  const int upsh = ufac == 2 ? 1 : 0;

  // Staging index math is incremental: each thread's k-th vector is (tid + 256k); the pixel /
  // channel-group / row decomposition of the first one costs a few divisions once per kernel, every
  // later one only adds constants with carries (runtime integer division is ~40 VALU ops).
  const int x_dp = 256 / cvec, x_dc = 256 - x_dp * cvec;  // +256 vectors = x_dp pixels + x_dc groups
  const int x_dy = x_dp / a.tpw, x_dx = x_dp - x_dy * a.tpw;
  const int x_pix0 = tid / cvec, x_cg0 = tid - x_pix0 * cvec;
  const int x_ty0 = x_pix0 / a.tpw, x_tx0 = x_pix0 - x_ty0 * a.tpw;
  const int w_dr = 256 / wvec_row, w_dk = 256 - w_dr * wvec_row;
  const int w_r0 = tid / wvec_row, w_k0 = tid - w_r0 * wvec_row;
  const int nrx = (nvec_x + 255) / 256, nrw = (nvec_w + 255) / 256;
  // k-steps software-pipelined two deep: the fragments of k-step s+1 are read from LDS while the MFMAs of
  // k-step s run (one wave per SIMD pair cannot hide the ds_read latency otherwise)
  auto compute = [&]() {
    if constexpr (GEO > 0) {
      static_assert(MW == 4, "GEO tiles are 16 x 16");
      constexpr int S = GEO, TPW = (TW - 1) * S + 3, CCP = S == 1 ? 48 : 40, WP = 9 * 32 + WPAD;
      const uint16_t* xb = xs + ((wave * MW * TPW + col) * S) * CCP + g * 8;
      const uint16_t* wb = ws + col * WP + g * 8;
      bf16x8 af[2][NT], bf[2][MW];
      auto ld = [&](int k, int b) {
        const int off = ((k / 3) * TPW + (k % 3)) * CCP;
#pragma unroll
        for (int t = 0; t < NT; ++t) af[b][t] = *(const bf16x8*)(wb + t * 16 * WP + k * 32);
#pragma unroll
        for (int m = 0; m < MW; ++m) bf[b][m] = *(const bf16x8*)(xb + m * S * TPW * CCP + off);
      };
      ld(0, 0);
#pragma unroll
      for (int k = 0; k < 9; ++k) {
#if CLIMSR_DIAG_MODE == 4  // diagnostic build 4: the k-step fragments read once per chunk, MFMAs only
        if (k == 0) ld(1, 1);
#else
        if (k + 1 < 9) ld(k + 1, (k + 1) & 1);
#endif
        // the next k-step's NT + MW fragment reads go out as one burst ahead of this k-step's MW x NT MFMAs (the
        // compiler otherwise sinks each read next to its first MFMA and waits lgkmcnt(0) there: the LDS latency was
        // exposed at nearly every k-step of the unrolled loop)
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int m = 0; m < MW; ++m)
#pragma unroll
          for (int t = 0; t < NT; ++t) acc[m][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[k & 1][t], bf[k & 1][m], acc[m][t], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
      return;
    }
    const int nks = a.kcpad / 32;
    bf16x8 afA[NT], bfA[MW], afB[NT], bfB[MW];
    auto ld = [&](int ks, bf16x8(&af)[NT], bf16x8(&bf)[MW]) {
      const int off = tab[ks * 4 + g];
#pragma unroll
      for (int t = 0; t < NT; ++t) af[t] = *(const bf16x8*)(ws + (t * 16 + col) * wpitch + ks * 32 + g * 8);
#pragma unroll
      for (int m = 0; m < MW; ++m) bf[m] = *(const bf16x8*)(xs + pixbase[m] + off);
    };
    auto mm = [&](const bf16x8(&af)[NT], const bf16x8(&bf)[MW]) {
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
      ld(ks + 2 < nks ? ks + 2 : nks - 1, afA, bfA);  // unconditional (clamped): no branch around the reads
      mm(afB, bfB);
    }
    if (ks < nks) mm(afA, bfA);  // odd k-step count: the last one is already loaded
  };

  if constexpr (PFX > 0 && GEO == 1) {
    // Compile-time staging geometry (18 x 18-pixel x tile of 4 x 16 B channel vectors, 64 x 36 weight vectors per
    // chunk): each thread's vector i is (tid + 256 i), so its pixel / channel group / weight row are per-thread
    // constants; the chunk-0 byte offset of every vector is computed once (out-of-image vectors get BUF_OOB, which
    // stays out of range at every chunk), and a chunk's loads are buffer loads at offset + j * chunk bytes -- one add
    // per vector.  The runtime-geometry walk below spent ~570 VALU per chunk on index carries, bounds checks and
    // 64-bit addresses (4 VALU per MFMA: the chunk loop was VALU-issue bound, conv5 / pull-x most of all).
    // The host takes GEO 1 only for up == 1, in_c % 32 == 0 and tensors under 2 GiB.
    constexpr int CV = 4, TPWc = TW + 2, CCPc = 48, NXV = (TW + 2) * (TW + 2) * CV, WV = 36, WPc = 9 * 32 + WPAD, NWV = NT * 16 * WV;
    static_assert(PFX * 256 >= NXV && PFW * 256 >= NWV, "GEO 1 staging: not enough prefetch vectors");
    uint4 px[PFX], pw[PFW];
    const int cg8 = (tid & 3) * 8;  // 256 % CV == 0: every vector of a thread has the same channel group
    const __amdgpu_buffer_rsrc_t xr = buf_rsrc(a.x, (uint32_t)((long)a.n * a.in_h * a.in_w * a.in_cs * 2));
    const __amdgpu_buffer_rsrc_t wr = buf_rsrc(a.w, (uint32_t)((long)(cob + 1) * NT * 16 * a.kpk * 2));
    uint32_t xo[PFX], wo[PFW];
#pragma unroll
    for (int i = 0; i < PFX; ++i) {
      const int v = tid + 256 * i, pix = v >> 2, ty_ = pix / TPWc, tx_ = pix - ty_ * TPWc;
      const int iy = iy0 + ty_, ix = ix0 + tx_;
      const bool ok = v < NXV && iy >= 0 && iy < a.in_h && ix >= 0 && ix < a.in_w;
      xo[i] = ok ? (uint32_t)((((nimg * a.in_h + iy) * a.in_w + ix) * a.in_cs + a.in_co + cg8) * 2) : BUF_OOB;
    }
#pragma unroll
    for (int i = 0; i < PFW; ++i) {
      const int v = tid + 256 * i, r = v / WV, kv = v - r * WV;
      wo[i] = v < NWV ? (uint32_t)(((co_blk0 + r) * a.kpk + kv * 8) * 2) : BUF_OOB;
    }
    auto issue = [&](int j) {
#pragma unroll
      for (int i = 0; i < PFX; ++i) px[i] = buf_load16(xr, xo[i] + (uint32_t)j * 64u);
#pragma unroll
      for (int i = 0; i < PFW; ++i) pw[i] = buf_load16(wr, wo[i] + (uint32_t)j * (uint32_t)(a.kcpad * 2));
    };
    auto stash = [&]() {
      // pixel (v >> 2) = (tid >> 2) + 64 i: compile-time steps; lanes past the tile dump into the pad channels 32..39
      // of pixel 0, which no fragment reads
      const int xl0 = (tid >> 2) * CCPc + cg8;
#pragma unroll
      for (int i = 0; i < PFX; ++i) {
        const int v = tid + 256 * i;
        *(uint4*)(xs + ((NXV % 256 == 0 || v < NXV) ? xl0 + 64 * CCPc * i : 32)) = px[i];
      }
#pragma unroll
      for (int i = 0; i < PFW; ++i) {
        const int v = tid + 256 * i, r = v / WV, kv = v - r * WV;
        if (NWV % 256 == 0 || v < NWV) *(uint4*)(ws + r * WPc + kv * 8) = pw[i];
      }
    };
    issue(0);
#if CLIMSR_DIAG_MODE == 2
    lds_barrier();
    stash();
    lds_barrier();
    for (int j = 0; j < a.nchunk; ++j) compute();
#else
    for (int j = 0; j < a.nchunk; ++j) {
      lds_barrier();  // chunk j-1's fragment reads are done
      stash();
      if (j + 1 < a.nchunk) issue(j + 1);  // lands while chunk j computes
      lds_barrier();
#if CLIMSR_DIAG_MODE != 3  // diagnostic build 3: staging only, no k-loop
      compute();
#endif
    }
#endif
  } else if constexpr (PFX > 0) {
    uint4 px[PFX], pw[PFW];
    auto issue = [&](int j) {
      int ty_ = x_ty0, tx_ = x_tx0, cg = x_cg0;
#pragma unroll
      for (int i = 0; i < PFX; ++i) {
        px[i] = make_uint4(0, 0, 0, 0);
        if (i < nrx && ty_ < a.tph) {
          const int iy = iy0 + ty_, ix = ix0 + tx_;
          const int c = j * a.cc + cg * 8;
          if (iy >= 0 && iy < lh && ix >= 0 && ix < lw && c < a.in_c && !((iy | ix) & dilmask))
            px[i] = *(const uint4*)(a.x + (((long)nimg * a.in_h + (iy >> upsh)) * a.in_w + (ix >> upsh)) * a.in_cs + a.in_co + c);
        }
        cg += x_dc;
        tx_ += x_dx;
        ty_ += x_dy;
        if (cg >= cvec) { cg -= cvec; ++tx_; }
        if (tx_ >= a.tpw) { tx_ -= a.tpw; ++ty_; }
      }
      int r = w_r0, kv = w_k0;
#pragma unroll
      for (int i = 0; i < PFW; ++i) {
        pw[i] = make_uint4(0, 0, 0, 0);
        if (i < nrw && r < NT * 16)
          pw[i] = *(const uint4*)(a.w + (long)(co_blk0 + r) * a.kpk + (long)j * a.kcpad + kv * 8);
        kv += w_dk;
        r += w_dr;
        if (kv >= wvec_row) { kv -= wvec_row; ++r; }
      }
    };
    auto stash = [&]() {
      int ty_ = x_ty0, tx_ = x_tx0, cg = x_cg0;
#pragma unroll
      for (int i = 0; i < PFX; ++i) {
        if (i < nrx && ty_ < a.tph) *(uint4*)(xs + (ty_ * a.tpw + tx_) * a.ccp + cg * 8) = px[i];
        cg += x_dc;
        tx_ += x_dx;
        ty_ += x_dy;
        if (cg >= cvec) { cg -= cvec; ++tx_; }
        if (tx_ >= a.tpw) { tx_ -= a.tpw; ++ty_; }
      }
      int r = w_r0, kv = w_k0;
#pragma unroll
      for (int i = 0; i < PFW; ++i) {
        if (i < nrw && r < NT * 16) *(uint4*)(ws + r * wpitch + kv * 8) = pw[i];
        kv += w_dk;
        r += w_dr;
        if (kv >= wvec_row) { kv -= wvec_row; ++r; }
      }
    };
    issue(0);
#if CLIMSR_DIAG_MODE == 2
    __syncthreads();
    stash();
    __syncthreads();
    for (int j = 0; j < a.nchunk; ++j) compute();
#else
    for (int j = 0; j < a.nchunk; ++j) {
      __syncthreads();  // chunk j-1's fragment reads are done
      stash();
      if (j + 1 < a.nchunk) issue(j + 1);  // lands while chunk j computes
      __syncthreads();
      compute();
#if CLIMSR_DIAG_MODE == 1
      compute();
#endif
    }
#endif
  } else {
  // batched staging: every thread issues up to MV input + MV weight 16 B global loads before the first
  // LDS store, so a chunk pays ~one memory latency instead of one per vector
  const int nbatch = nrx > nrw ? nrx : nrw;
  for (int j = 0; j < a.nchunk; ++j) {
    __syncthreads();
    int ty_ = x_ty0, tx_ = x_tx0, cg = x_cg0;  // input tile (logical coordinates: upsampled / zero-inserted)
    int r = w_r0, kv = w_k0;                  // weight chunk rows [co_blk0, co_blk0 + 16*NT) x kcpad
    for (int base = 0; base < nbatch; base += MV) {
      uint4 bx[MV], bw[MV];
      int dx[MV], dw[MV];
#pragma unroll
      for (int i = 0; i < MV; ++i) {
        dx[i] = -1;
        if (base + i < nrx && ty_ < a.tph) {
          const int iy = iy0 + ty_, ix = ix0 + tx_;
          const int c = j * a.cc + cg * 8;
          uint4 val = make_uint4(0, 0, 0, 0);
          if (iy >= 0 && iy < lh && ix >= 0 && ix < lw && c < a.in_c && !((iy | ix) & dilmask))
            val = *(const uint4*)(a.x + (((long)nimg * a.in_h + (iy >> upsh)) * a.in_w + (ix >> upsh)) * a.in_cs + a.in_co + c);
          bx[i] = val;
          dx[i] = (ty_ * a.tpw + tx_) * a.ccp + cg * 8;
        }
        cg += x_dc;
        tx_ += x_dx;
        ty_ += x_dy;
        if (cg >= cvec) { cg -= cvec; ++tx_; }
        if (tx_ >= a.tpw) { tx_ -= a.tpw; ++ty_; }
      }
#pragma unroll
      for (int i = 0; i < MV; ++i) {
        dw[i] = -1;
        if (base + i < nrw && r < NT * 16) {
          bw[i] = *(const uint4*)(a.w + (long)(co_blk0 + r) * a.kpk + (long)j * a.kcpad + kv * 8);
          dw[i] = r * wpitch + kv * 8;
        }
        kv += w_dk;
        r += w_dr;
        if (kv >= wvec_row) { kv -= wvec_row; ++r; }
      }
#pragma unroll
      for (int i = 0; i < MV; ++i)
        if (dx[i] >= 0) *(uint4*)(xs + dx[i]) = bx[i];
#pragma unroll
      for (int i = 0; i < MV; ++i)
        if (dw[i] >= 0) *(uint4*)(ws + dw[i]) = bw[i];
    }
    __syncthreads();
    compute();
  }
  }

  // ---------------- epilogue ----------------
  // All global reads of the epilogue (bias, residuals, accumulate targets) are issued for every
  // fragment before the first store, so their latencies overlap instead of serialising.
  const int ox = ox0 + col;
  if (EP == 0 && a.down2) {
    // sum the 2x2 block: rows (m, m+1) are in this wave (MW even, oy0 even); columns pair via lane^1.
    // Optional activation backward (act 3/4, res1 = the activation output at the LOW-res pixel), bf16 or
    // fp32 (=, +=) store and a bf16 aux copy.
    const int dh = a.out_h >> 1, dw = a.out_w >> 1;
    const bool mask = a.act == 3 || a.act == 4;
    float4 old[MW / 2][NT];
    uint2 r1v[MW / 2][NT];
    const __amdgpu_buffer_rsrc_t ry2 = opt_rsrc(a.out_mode == 2 ? a.y : nullptr), rm1 = opt_rsrc(mask ? a.res1 : nullptr);
#pragma unroll
    for (int m = 0; m < MW; m += 2) {
      const int oy = oy0 + wave * MW + m;
      const long pidx = ((long)nimg * dh + (oy >> 1)) * dw + (ox >> 1);
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int co = co_blk0 + t * 16 + g * 4;
        const bool ok = (col & 1) == 0 && oy < a.out_h && ox < a.out_w && co + 3 < a.out_c;
        const long q = ok ? pidx : 0;
        const uint4 o4 = buf_load16(ry2, (uint32_t)((q * a.out_cs + (ok ? a.out_co + co : 0)) * 4));
        old[m / 2][t] = make_float4(__uint_as_float(o4.x), __uint_as_float(o4.y), __uint_as_float(o4.z), __uint_as_float(o4.w));
        r1v[m / 2][t] = buf_load8(rm1, (uint32_t)((q * a.r1_cs + (ok ? a.r1_co + co : 0)) * 2));
      }
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
        const int co = co_blk0 + t * 16 + g * 4;
        if ((col & 1) == 0 && oy < a.out_h && ox < a.out_w) {
          const long ob = pidx * a.out_cs + a.out_co + co;
          if (co + 3 < a.out_c) {
            const uint4 r1 = make_uint4(r1v[m / 2][t].x, r1v[m / 2][t].y, 0, 0);
            if (mask) {
#pragma unroll
              for (int i = 0; i < 4; ++i) v[i] = ep_res(v[i], a.act, a.slope, true, res4_at(r1, false, i), 1.f, 1.f, false, 0.f, 1.f, 1.f);
            }
            if (a.out_mode == 0) {
              uint2 pk;
              pk.x = (uint32_t)f2bf(v[0]) | ((uint32_t)f2bf(v[1]) << 16);
              pk.y = (uint32_t)f2bf(v[2]) | ((uint32_t)f2bf(v[3]) << 16);
              *(uint2*)((uint16_t*)a.y + ob) = pk;
            } else {
              float4 o = old[m / 2][t];
              *(float4*)((float*)a.y + ob) = make_float4(o.x + v[0], o.y + v[1], o.z + v[2], o.w + v[3]);
            }
            if (a.aux) {
              uint2 pk;
              pk.x = (uint32_t)f2bf(a.aux_scale * v[0]) | ((uint32_t)f2bf(a.aux_scale * v[1]) << 16);
              pk.y = (uint32_t)f2bf(a.aux_scale * v[2]) | ((uint32_t)f2bf(a.aux_scale * v[3]) << 16);
              *(uint2*)(a.aux + pidx * a.aux_cs + a.aux_co + co) = pk;
            }
          } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              if (co + i >= a.out_c) continue;
              float x = v[i];
              if (mask) x = ep_res(x, a.act, a.slope, true, res_at(a.res1, false, pidx * a.r1_cs + a.r1_co + co + i), 1.f, 1.f, false,
                                   0.f, 1.f, 1.f);
              if (a.out_mode == 0) ((uint16_t*)a.y)[ob + i] = f2bf(x);
              else if (a.out_mode == 2) ((float*)a.y)[ob + i] += x;
              else ((float*)a.y)[ob + i] = x;
              if (a.aux) a.aux[pidx * a.aux_cs + a.aux_co + co + i] = f2bf(a.aux_scale * x);
            }
          }
        }
      }
    }
    return;
  }
  // coalesced epilogue: the wave's MW x 16 pixels x 16 NT channels go through its own LDS region
  constexpr int EPP = NT * 16 + 4;  // LDS pitch (floats) of a staged pixel
  float* eb = (float*)smem + wave * (MW * 16 * EPP);
  __syncthreads();  // every wave is done with the staged operands (the regions alias them)
#pragma unroll
  for (int m = 0; m < MW; ++m)
#pragma unroll
    for (int t = 0; t < NT; ++t) *(f32x4*)(eb + (m * 16 + col) * EPP + t * 16 + g * 4) = acc[m][t];
  __syncthreads();  // orders the staging writes before the transposed reads (they use another vector type)
  if constexpr (EP == 9 || EP == 10) {
    static_assert(MW == 4 && NT == 4, "BatchNorm partials: 16x16 x 64-channel tiles");
    float ssum[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, ssq[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    store_tile_lds<RF, MW * 16, NT * 16, 64, EP>(a, eb, EPP, lane, nimg, oy0 + wave * MW, ox0, co_blk0, ssum, ssq);
    bn_tile_partials(a, ssum, ssq, true, wave, lane, tile_id, co_blk0, (float*)smem);
  } else {
    store_tile_lds<RF, MW * 16, NT * 16, 64, EP>(a, eb, EPP, lane, nimg, oy0 + wave * MW, ox0, co_blk0);
  }
}

// two workgroups per CU (<= 80 KiB LDS each): at most 256 registers so that two waves share each SIMD
template <int MW, int NT, bool RF, int MV, int PFX = 0, int PFW = 0, int EP = 0, int GEO = 0>
__global__ __launch_bounds__(256, 2) void conv_fwd_kernel(FwdArgs a) {
  conv_fwd_body<MW, NT, RF, MV, PFX, PFW, EP, GEO>(a);
}
// large stride-2 input tiles (one workgroup per CU): the deep prefetch may use the whole register file
template <int MW, int NT, bool RF, int MV, int PFX = 0, int PFW = 0, int EP = 0, int GEO = 0>
__global__ __launch_bounds__(256) void conv_fwd_wide_kernel(FwdArgs a) {
  conv_fwd_body<MW, NT, RF, MV, PFX, PFW, EP, GEO>(a);
}

// the second dispatch round of a two-workgroups-per-CU launch starts late (conv_fwd_body 'Stagger')
static void set_stagger(FwdArgs& a) {
  const int ncu = device_cus();
  a.stag_lo = ncu;
  a.stag_hi = 2 * ncu;
  a.stag_n = 2;  // 2 x 2048 cycles: GAN step 25.25 -> 24.98 ms (same box, 2 + 6 runs)
}

template <int MW, int NT, int PFX, int PFW, int EP, int GEO>
static int launch_fwd_geo(const FwdRoute& r, const FwdArgs& a0, hipStream_t s) {
  FwdArgs a = a0;
  set_stagger(a);
  constexpr bool WIDE = PFX == 18;
  if (GEO != 1 || WIDE) a.stag_n = 0;
  const dim3 grid = a.xgrp ? dim3(a.tiles_x * a.tiles_y * a.n * r.ncob) : dim3(a.tiles_x * a.tiles_y * a.n, r.ncob);
  constexpr int MV = fwd_mv(NT);
  void (*kt)(FwdArgs);
  void (*kf)(FwdArgs);
  if constexpr (WIDE) {
    kt = conv_fwd_wide_kernel<MW, NT, true, MV, PFX, PFW, EP, GEO>;
    kf = conv_fwd_wide_kernel<MW, NT, false, MV, PFX, PFW, EP, GEO>;
  } else {
    kt = conv_fwd_kernel<MW, NT, true, MV, PFX, PFW, EP, GEO>;
    kf = conv_fwd_kernel<MW, NT, false, MV, PFX, PFW, EP, GEO>;
  }
  auto k = r.rf ? kt : kf;
  if (int e = lds_opt_in((const void*)k, 160 * 1024)) return e;
  hipLaunchKernelGGL(k, grid, dim3(256), r.lds, s, a);
  return check_launch("conv2d_fwd");
}
