// Shared by the conv translation units, host side: the route a forward conv takes (FwdRoute: decided once by fwd_route()
// in conv.hip from the descriptor and the epilogue alone, no device call) and the launchers of the kernel families,
// each compiled in a unit of its own.
//
//   conv.hip        errors and launch plumbing, geometry, weight packing, fwd_route() and climsr_conv2d_fwd
//   conv_small.hip  the shape-specific kernels: n16, co1m, co1, pt, the stride-2 data gradient, the 1 <-> C stencil
//   conv_fwd.hip    generic forward / data-gradient kernel (conv_fwd_kernel.h), 16x16 tiles
//   conv_pw.hip     weights-resident persistent kernel, and the generic kernel's 8x16 tiles
//   conv_dma.hip    LDS-DMA forms                      conv_wr.hip  register-resident 64 -> 64
//   conv_wgrad.hip  the weight-gradient side (a route of its own, wg_route; from here only FWD_MAXV)
#pragma once
#include "conv_ep.h"

namespace climsr {
constexpr int WPAD = 16;     // k padding of the LDS weight tile rows (kcpad is a multiple of 32)
constexpr int FWD_MAXV = 8;  // 16 B staging vectors per thread held in registers (prefetch)
constexpr int N16_TH = 8;    // output rows of a conv_n16_kernel tile
// 32-channel blocks of conv_n16_kernel's one chunk (its NCB)
static inline int n16_ncb(int in_c) { return in_c <= 32 ? 1 : (in_c <= 64 ? 2 : 4); }

struct FwdGeom {
  int th, tph, tpw, ccp, kc, kcpad, nchunk, kpk, nt, mw;
  size_t lds_tab, lds_x, lds_w, lds_total;
};

struct PwGeom {
  int mw, tph, tpw, ccp, kcpad, nvx;
  size_t lds_tab, lds_w, lds_x, lds_ep, lds_total;
};

// ------------------------------------------------------------------------------------------
// The route of a forward / data-gradient conv: kernel family, the template ids of the instantiation and the
// geometry its launch needs.  Which ids a family reads:
//   CO1M  ks, nch (KS, NCH)              CO1   -                          N16   nch, ep (NCB, EP)
//   DGRAD_S2  ep, mw, nt                 FWD_S2  ep (9 = with partials)   PT    nt, nch, ep (NCOF, NKC, EP)
//   WR    ep                             PW    nw, mw, nt, rf, pv, ep, geo
//   FWD / DMA  mw, nt, rf, pfx, pfw, ep, geo (DMA: ep, rf)
// ------------------------------------------------------------------------------------------
enum FwdFamily { FAM_CO1M, FAM_CO1, FAM_N16, FAM_DGRAD_S2, FAM_FWD_S2, FAM_PT, FAM_WR, FAM_PW, FAM_FWD, FAM_DMA };

struct FwdRoute {
  int family;
  int ks, nch, nw, mw, nt, pv, pfx, pfw, ep, geo;
  bool rf;     // the instantiation that reads fp32 residuals (res_f32 != 0)
  bool parts;  // the kernel writes the BatchNorm partials the epilogue asks for
  FwdGeom g;
  PwGeom pg;   // FAM_PW
  int ncob, tiles_x, tiles_y, xgrp;
  size_t lds;  // dynamic LDS bytes of FAM_FWD (FAM_PW: pg.lds_total; the other families derive it from their template ids)
};

// staging vectors (16 B) per thread of conv_fwd_kernel<.., NT, ..>
constexpr int fwd_mv(int nt) { return nt == 1 ? 6 : (nt == 2 ? 8 : 4); }

// The launchers of the families: each switches on the route's ids to reach the instantiation, CLIMSR_EINVAL
// (+ set_error) for ids without one.
int fwd_small_launch(const FwdRoute& r, const FwdArgs& a, hipStream_t s);     // CO1M, CO1, N16, PT (conv_small.hip)
int fwd_dgrad_s2_launch(const FwdRoute& r, const FwdArgs& a, hipStream_t s);  // conv_small.hip
int fwd_pw_launch(const FwdRoute& r, const FwdArgs& a, hipStream_t s);        // conv_pw.hip
int fwd_generic_launch(const FwdRoute& r, const FwdArgs& a, hipStream_t s);   // FWD, DMA (conv_fwd.hip)
int fwd_rows2_launch(const FwdRoute& r, const FwdArgs& a, hipStream_t s);     // FWD with mw 2 (conv_pw.hip)
// conv_wr.hip: epk = conv_wr_ep(d, ep, bias) >= 0
int conv_wr_launch(int epk, const ClimsrConvDesc* d, const ClimsrEpilogue* ep, const uint16_t* x, const uint16_t* wpk, int kpk,
                   const float* bias, void* y, hipStream_t s);
int conv_wr_tiles_per_image(const ClimsrConvDesc* d);
// the conv_wr epilogue for (d, ep), or -1 when the conv is not that kernel's
int conv_wr_ep(const ClimsrConvDesc* d, const ClimsrEpilogue* ep, bool bias);

}  // namespace climsr
