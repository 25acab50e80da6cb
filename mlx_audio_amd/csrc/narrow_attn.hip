// Narrow-head attention (gfx950): softmax(scale q k^T + key visibility) v for head widths 8 / 16 / 24 / 32 at any T.
// Reference call site: TransformerAttention.__call__ (vad/models/sortformer/sortformer.py:532-564) under TransformerEncoder's mask (621-631):
// the 18 post-LN layers of Sortformer run 8 heads of 24 at T = seconds / 0.08 (1125 frames for 90 s).
//
// The mask.  The reference ADDS -1e4 to the scores of padded keys.  In float32 exp(s - max - 1e4) underflows to exactly 0 whenever one valid key
// exists (scores are O(10), the smallest float32 subnormal is e^-103.3), so its softmax gives padded keys the weight 0.0f and the valid keys
// the weights of a softmax over the valid keys alone.  This kernel never looks at the keys j >= lens[b]: the same function.  lens[b] >= 1 is the
// host's duty (the entry point cannot read device memory; ops.narrow_attention checks it).  Output rows >= lens[b] are written as exact zeros,
// relpos_attention's convention.
//
// The query tile of attn_tile.h (tiling, orientation, key order, log2 domain: stated there) with 32-key stages.  K Q^T takes DH / 2 MFMA steps.
// For P V the V^T operand is ONE 32-row block: row d of the block is head dimension d, and the rows d >= DH are never stored.  Row m of an MFMA result
// depends on row m of the A operand alone, so whatever the lanes c >= DH read (the next key's row, the 32-float tail behind the last one: always
// inside the LDS array) lands only in accumulator rows that nobody reads.  At DH = 24 a quarter of the P V issue slots are idle.
// Plain float32, a fixed summation order, no atomics, no workspace: two calls on the same bytes give the same bits.
#include "attn_tile.h"

namespace {

constexpr int kNarrowKB = 32;   // keys per stage

template <int DH>
__global__ __launch_bounds__(256) void narrow_attn_kernel(const mi355_narrow_attention_args a) {
  constexpr int KB = kNarrowKB;
  constexpr int LD = DH + 1;        // padded LDS row, floats: the K operand's ds_read_b32 (lane = key row) is bank-conflict free
  constexpr int C4 = DH / 4;        // float4 pieces of a row
  constexpr int NLD = KB * C4;      // float4 loads per operand per stage: 64 .. 256, at most one per thread
  __shared__ float Ks[KB * LD];
  __shared__ float Vs[KB * LD + 32];   // + 32: lane c of the V^T read touches row * LD + c for every c < 32

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, c = lane & 31;
  const int h = blockIdx.y, b = blockIdx.z;
  const int len = a.lens ? min(max(a.lens[b], 0), a.T) : a.T;
  const int q0 = blockIdx.x * 128;
  float* obase = a.out + (int64_t)b * a.out_bstride + h * DH;
  if (q0 >= len) {   // a block of padding rows (or lens[b] == 0): zeros
    attn_zero_block<DH>(obase, a.ldo, q0, a.T, tid);
    return;
  }
  const int i0 = q0 + wave * 32;
  const int qi = i0 + c;
  const bool wave_active = i0 < len;
  const int qic = qi < len ? qi : len - 1;

  float qs[DH / 2];
  attn_load_q<DH>(qs, a.q + (int64_t)b * a.q_bstride + (int64_t)qic * a.ldq + h * DH, a.scale * kLog2e, half);

  const float* kbase = a.k + (int64_t)b * a.k_bstride + h * DH;
  const float* vbase = a.v + (int64_t)b * a.v_bstride + h * DH;
  const bool loader = tid < NLD;   // the stage has fewer pieces than the workgroup has threads

  float4 kpre[1] = {make_float4(0.f, 0.f, 0.f, 0.f)}, vpre[1] = {kpre[0]};
  auto prefetch = [&](int kb) {
    if (loader) attn_stage_prefetch<DH, 1>(kpre, vpre, kbase, vbase, a.ldk, a.ldv, kb, len, tid);
  };

  f32x16 o[1];
  attn_zero(o);
  float m = -INFINITY, lsum = 0.f;

  prefetch(0);
  for (int kb = 0; kb < len; kb += KB) {
    __syncthreads();   // everyone is done reading the previous stage
    if (loader) attn_stage_commit<DH, 1>(Ks, Vs, kpre, vpre, tid);
    __syncthreads();
    if (kb + KB < len) prefetch(kb + KB);
    if (!wave_active) continue;
    f32x16 acc = attn_kq<DH>(Ks + c * LD + half, qs);   // S^T block (32 keys x 32 queries)
    // ---- mask (only a stage that touches len), online softmax (per-lane query)
    const bool edge = kb + KB > len;
    float bm = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      if (edge && kb + attn_c_row(r, half) >= len) acc[r] = -INFINITY;
      bm = fmaxf(bm, acc[r]);
    }
    attn_online_softmax<false>(acc, bm, m, lsum, o);   // key kb is valid in every stage
    attn_pv(o, acc, Vs, LD, half, c);                  // lane c is head dimension c of the one block
  }

  if (qi >= a.T) return;
  // padding rows inside a block that has valid ones: zeros
  attn_store_o<DH>(obase + (int64_t)qi * a.ldo, o, attn_inv_sum<false>(lsum), half, qi < len);
}

template <int DH>
int launch_narrow(const mi355_narrow_attention_args& a, hipStream_t st) {
  MI355_CLEAR_ERROR();
  hipLaunchKernelGGL(narrow_attn_kernel<DH>, dim3((unsigned)((a.T + 127) / 128), (unsigned)a.heads, (unsigned)a.B), dim3(256), 0, st, a);
  MI355_LAUNCH_CHECK("narrow_attention");
  return MI355_OK;
}

}  // namespace

extern "C" int mi355_narrow_attention(const mi355_narrow_attention_args* ap, void* stream) {
  MI355_REQUIRE(ap && ap->q && ap->k && ap->v && ap->out, "narrow_attention: null tensor");
  const mi355_narrow_attention_args a = *ap;
  MI355_REQUIRE(a.dh == 8 || a.dh == 16 || a.dh == 24 || a.dh == 32, "narrow_attention: dh must be 8, 16, 24 or 32 (got dh = %d)", a.dh);
  MI355_REQUIRE(a.B > 0 && a.B <= 65535 && a.heads > 0 && a.heads <= 65535 && a.T >= 1, "narrow_attention: bad shape");
  const int64_t hd = (int64_t)a.heads * a.dh;
  MI355_REQUIRE(a.ldq >= hd && a.ldk >= hd && a.ldv >= hd && a.ldo >= hd, "narrow_attention: a row stride is smaller than heads * dh");
  MI355_REQUIRE(a.ldq % 4 == 0 && a.ldk % 4 == 0 && a.ldv % 4 == 0 && a.ldo % 4 == 0 && a.q_bstride % 4 == 0 && a.k_bstride % 4 == 0 &&
                    a.v_bstride % 4 == 0 && a.out_bstride % 4 == 0 && ((uintptr_t)a.q | (uintptr_t)a.k | (uintptr_t)a.v | (uintptr_t)a.out) % 16 == 0,
                "narrow_attention: rows must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  switch (a.dh) {
    case 8: return launch_narrow<8>(a, st);
    case 16: return launch_narrow<16>(a, st);
    case 24: return launch_narrow<24>(a, st);
    default: return launch_narrow<32>(a, st);
  }
}
