// conv_ws4, precision 5 instantiations: fp16 hi pass + block-scaled e4m3 lo pass (v_mfma_scale_f32_32x32x64_f8f6f4) on the MX weight image
// (mi355_pack_conv_weight_mx_host).  Conv mode, 128-column tiles: the resblock / upsampler convs of the vocoders.
#include "conv_ws4.h"

using namespace mi355conv;

int mi355_conv_ws4_p5(const ws4_call& c, const int feat) {
  if ((feat & 2) && c.pre == P_SNAKE && c.epi == 0) return route_ws4<5, P_SNAKE, 0, false, false, 0, 128, false, false>(c, feat & 9);   // A / B aid: the 2 x 2 consumer layout
  WS4_CASE(5, P_NONE, 0);
  WS4_CASE(5, P_LEAKY, 0);
  WS4_CASE(5, P_SNAKE, 0);
  return MI355_ERR_UNSUPPORTED;
}
