// conv_ws4, quantising prologues (mi355_conv_gemm_args.pre_fq: KittenTTS activation quantisation), bf16 hi+lo, 128- and 64-column tiles.
#include "conv_ws4.h"

using namespace mi355conv;

#define WS4_FQ(PRE, BNV) \
  if (c.bn == BNV && c.pre == PRE) return route_ws4<2, PRE, 0, false, false, 0, BNV, true>(c, feat)

int mi355_conv_ws4_fq(const ws4_call& c, const int feat) {
  if (c.epi != 0) return MI355_ERR_UNSUPPORTED;
  WS4_FQ(P_NONE, 128);
  WS4_FQ(P_LEAKY, 128);
  WS4_FQ(P_SNAKE, 128);
  WS4_FQ(P_NONE, 64);
  WS4_FQ(P_LEAKY, 64);
  WS4_FQ(P_SNAKE, 64);
  return MI355_ERR_UNSUPPORTED;
}
