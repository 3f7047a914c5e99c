// The generic forward / data-gradient kernel's 16x16-tile (MW 4) instantiations and the hand-off to the LDS-DMA conv.
#include "conv_fwd_kernel.h"

using namespace climsr;

// the GEO forms a tile shape has: 1 (stride 1) beside the chunk-pipelined and plain 16x16 tiles, 2 (stride 2) beside
// the deep-prefetch ones, 0 for all
template <int MW, int NT, int PFX = 0, int PFW = 0, int EP = 0>
static int launch_fwd_ep(const FwdRoute& r, const FwdArgs& a, hipStream_t s) {
  if constexpr (MW == 4 && PFX != 18) {
    if (r.geo == 1) return launch_fwd_geo<MW, NT, PFX, PFW, EP, 1>(r, a, s);
  }
  if constexpr (MW == 4 && PFX == 18) {
    if (r.geo == 2) return launch_fwd_geo<MW, NT, PFX, PFW, EP, 2>(r, a, s);
  }
  return launch_fwd_geo<MW, NT, PFX, PFW, EP, 0>(r, a, s);
}

int climsr::fwd_generic_launch(const FwdRoute& r, const FwdArgs& a, hipStream_t s) {
  if (r.family == FAM_DMA) {  // the LDS-DMA conv (conv_dma.hip)
    const int rc = fwd_dma_launch(r.ep, a, r.ncob, s);
    return rc == CLIMSR_OK ? check_launch("conv2d_fwd (LDS-DMA)") : rc;
  }
#define FWD_CASE(PFX, PFW, EP) \
  if (r.mw == 4 && r.pfx == PFX && r.ep == EP) return launch_fwd_ep<4, 4, PFX, PFW, EP>(r, a, s);
  FWD_CASE(6, 9, 0) FWD_CASE(6, 9, 1) FWD_CASE(6, 9, 2) FWD_CASE(6, 9, 3) FWD_CASE(6, 9, 4)
  FWD_CASE(6, 9, 6) FWD_CASE(6, 9, 7) FWD_CASE(6, 9, 8) FWD_CASE(6, 9, 9) FWD_CASE(6, 9, 10)
  FWD_CASE(18, 9, 0) FWD_CASE(18, 9, 8)
  FWD_CASE(0, 0, 0) FWD_CASE(0, 0, 3) FWD_CASE(0, 0, 6) FWD_CASE(0, 0, 7) FWD_CASE(0, 0, 8)
#undef FWD_CASE
  if (r.mw == 2) return fwd_rows2_launch(r, a, s);  // 8x16 tiles: instantiated in conv_pw.hip
  set_error("conv2d_fwd: no conv_fwd kernel for mw %d, nt %d, prefetch %d / %d, ep %d", r.mw, r.nt, r.pfx, r.pfw, r.ep);
  return CLIMSR_EINVAL;
}
