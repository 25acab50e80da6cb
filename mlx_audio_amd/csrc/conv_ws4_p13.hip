// conv_ws4, single-pass instantiations (precision 1: bf16, precision 3: fp16): the opt-in fast modes of the Kokoro / Whisper engines.
#include "conv_ws4.h"

using namespace mi355conv;

int mi355_conv_ws4_p13(const ws4_call& c, const int feat) {
  if (c.prec == 1) {
    WS4_CASE(1, P_NONE, 0);
    WS4_CASE(1, P_LEAKY, 0);
    WS4_CASE(1, P_SNAKE, 0);
    WS4_GEMM(1, 0);
    WS4_GEMM(1, 1);
    WS4_CASE_N64(1, P_NONE, 0);
    WS4_CASE_N64(1, P_LEAKY, 0);
    WS4_CASE_N64(1, P_SNAKE, 0);
    WS4_GEMM_N64(1, 0);
  } else {
    WS4_CASE(3, P_NONE, 0);
    WS4_CASE(3, P_LEAKY, 0);
    WS4_CASE(3, P_SNAKE, 0);
    WS4_CASE(3, P_NONE, 1);
    WS4_GEMM(3, 0);
    WS4_GEMM(3, 1);
    WS4_CASE_N64(3, P_NONE, 0);
    WS4_CASE_N64(3, P_LEAKY, 0);
    WS4_CASE_N64(3, P_SNAKE, 0);
    WS4_GEMM_N64(3, 0);
  }
  return MI355_ERR_UNSUPPORTED;
}
