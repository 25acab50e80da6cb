// conv_ws4: dispatcher + the bf16 hi+lo (precision 2) instantiations of the wave-specialised kernel (conv_ws4.h), its timing-ablation and
// timeline-probe builds.
#include "conv_ws4.h"

using namespace mi355conv;

namespace {
unsigned long long* g_dbg_buffer = nullptr;  // host copy of the probe buffer pointer (handed to the DBG instantiations through their geometry record)
int g_ws4_resident = 0;                      // mi355_conv_ws4_resident; 0 = a number per CU
}

namespace mi355conv {
unsigned long long* ws4_debug_buffer() { return g_dbg_buffer; }

// persistent: two resident workgroups per CU (128 VGPRs x 8 waves each) walk the tile list; small problems launch one workgroup per tile
unsigned ws4_grid(const int total_ids, const int feat) {
  static int cus = 0;
  if (cus == 0) {
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) cus = prop.multiProcessorCount;
    if (cus <= 0) cus = 256;
  }
  // mi355_conv_ws4_resident(n): the next launches take at most n persistent workgroups (a share of the chip: several convs on separate streams)
  const int resident = g_ws4_resident > 0 ? ((g_ws4_resident + 7) / 8) * 8 : ((cus * conv_knobs().ws_wg_per_cu) / 8) * 8;
  return (unsigned)((feat & 8) || total_ids <= resident ? total_ids : resident);  // feat bit 3: one workgroup per tile (A/B aid)
}
}  // namespace mi355conv

// Process-wide, host-side setting read at launch time: persistent workgroups of the wave-specialised kernel's next launches (0 = the default, two
// per CU).  For running independent convs side by side on several streams, each on a share of the chip (tools/bench_conv_concurrent.py).
extern "C" int mi355_conv_ws4_resident(int wgs) {
  MI355_REQUIRE(wgs >= 0, "conv_ws4_resident: negative count");
  g_ws4_resident = wgs;
  return MI355_OK;
}

bool mi355_conv_ws4_eligible(const mi355_conv_gemm_args& a, const int prec, const bool vec) {
  if (!vec || a.Lin <= 0 || a.flat_valid != 0) return false;   // (flattened strided convs: the producers mask by row, not by flat element index)
  if (prec == 5 || prec == 6)   // conv mode only (K == 1 layers included), K odd with an even number of tap pairs, 128-column tiles
    return a.K % 4 == 3 && 128 + (a.K - 1) * a.dil <= 192 && a.Cout > 64 && !a.pre_fq && (pre_kind(a) == P_NONE || pre_kind(a) == P_LEAKY || pre_kind(a) == P_SNAKE) &&
           epi_family(a) == 0;
  if (!gemm_mode(a) && 128 + (a.K - 1) * a.dil > 192) return false;
  return prec >= 1 && prec <= 4 && pre_kind(a) >= 0;
}

// the timeline probe's buffer: [ceil(grid / 16)][34] uint64 (device memory owned by the caller; nullptr switches the probe off)
extern "C" int mi355_conv_ws4_debug_buffer(void* p) {
  g_dbg_buffer = (unsigned long long*)p;
  return MI355_OK;
}

int mi355_conv_ws4_p2(const ws4_call& c, const int feat) {
  if (c.bn == 128 && (feat & 4) && c.pre == P_SNAKE && c.epi == 0 && !c.gemm) return route_ws4<2, P_SNAKE, 0, false, true>(c, feat);
  if (const int abl = c.bn == 128 ? feat >> 4 : 0) {  // timing ablations (wrong results by design)
    if (c.gemm && c.epi == 0) {   // GEMM mode (round 6: what bounds the wide linears)
      switch (abl) {
        case 1: return route_ws4<2, P_NONE, 0, true, false, 1>(c, feat & 15);
        case 4: return route_ws4<2, P_NONE, 0, true, false, 4>(c, feat & 15);
        case 5: return route_ws4<2, P_NONE, 0, true, false, 5>(c, feat & 15);
      }
    }
    MI355_REQUIRE(c.pre == P_SNAKE && c.epi == 0 && !c.gemm, "conv_gemm(ws4): ablation tiles exist for the precision-2 Snake kernel and the plain GEMM mode only");
    switch (abl) {
      case 1: return route_ws4<2, P_SNAKE, 0, false, false, 1>(c, feat & 15);
      case 2: return route_ws4<2, P_SNAKE, 0, false, false, 2>(c, feat & 15);
      case 3: return route_ws4<2, P_SNAKE, 0, false, false, 3>(c, feat & 15);
      case 4: return route_ws4<2, P_SNAKE, 0, false, false, 4>(c, feat & 15);
      case 7: return route_ws4<2, P_SNAKE, 0, false, false, 7>(c, feat & 15);
    }
    mi355_set_error("conv_gemm(ws4): unknown ablation %d", abl);
    return MI355_ERR_UNSUPPORTED;
  }
  // Kokoro: AdaIN resblocks (Snake), AdainResBlk1d / upsamplers (LeakyReLU), linears (+ GELU: PL-BERT FFN); bf16 codec checkpoints (Mimi: ELU,
  // Qwen3 codec: SnakeBeta, LayerScale / SiLU / GELU-tanh linears)
  WS4_CASE(2, P_NONE, 0);
  WS4_CASE(2, P_LEAKY, 0);
  WS4_CASE(2, P_SNAKE, 0);
  WS4_CASE(2, P_SNAKEBETA, 0);
  WS4_CASE(2, P_ELU, 0);
  WS4_CASE(2, P_NONE, 1);
  WS4_GEMM(2, 0);
  WS4_GEMM(2, 1);
  WS4_GEMM(2, 2);
  WS4_GEMM(2, 3);
  // 64-column tiles: thin tensors (KittenTTS: 64-channel generator stage; codec decoders' late stages)
  WS4_CASE_N64(2, P_NONE, 0);
  WS4_CASE_N64(2, P_LEAKY, 0);
  WS4_CASE_N64(2, P_SNAKE, 0);
  WS4_CASE_N64(2, P_ELU, 0);
  WS4_GEMM_N64(2, 0);
  return MI355_ERR_UNSUPPORTED;
}

int mi355_conv_ws4_route(const mi355_conv_gemm_args& a, const int prec, const int feat, const int bn, conv_route& r) {
  const ws4_call c{a, prec, pre_kind(a), epi_family(a), prec != 5 && prec != 6 && gemm_mode(a), bn, r};
  if (a.pre_fq) return prec == 2 ? mi355_conv_ws4_fq(c, feat & 3) : MI355_ERR_UNSUPPORTED;
  switch (prec) {
    case 2: return mi355_conv_ws4_p2(c, feat);
    case 4: return mi355_conv_ws4_p4(c, feat & 3);
    case 6: return (feat & ~9) ? mi355_conv_ws4_p5_probe(c, feat) : mi355_conv_ws4_p6(c, feat & 9);
    case 5: return (feat & ~11) ? mi355_conv_ws4_p5_probe(c, feat) : mi355_conv_ws4_p5(c, feat & 11);
    case 1:
    case 3: return mi355_conv_ws4_p13(c, feat & 3);
  }
  return MI355_ERR_UNSUPPORTED;
}

int mi355_conv_ws4_no_instantiation(const mi355_conv_gemm_args& a, const int prec, const int bn) {
  mi355_set_error("conv_gemm(ws4): no instantiation for precision %d, prologue %d, epilogue family %d, %d-column tiles", prec, pre_kind(a), epi_family(a), bn);
  return MI355_ERR_UNSUPPORTED;
}
