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
// relpos_attn_kernel's tiling (conformer.hip) without the band term: one workgroup = 128 queries x one head, 4 waves x 32 queries, 32-key stages
// of K / V through LDS with the next stage's global loads in flight over the current stage's math, both contractions on v_mfma_f32_32x32x2_f32
// in the transposed orientation (a lane owns ONE query column), online softmax in the log2 domain.  K Q^T takes DH / 2 MFMA steps.  For P V the
// V^T operand is ONE 32-row block: row d of the block is head dimension d, and the rows d >= DH are never stored.  Row m of an MFMA result
// depends on row m of the A operand alone, so whatever the lanes c >= DH read (the next key's row, the 32-float tail behind the last one: always
// inside the LDS array) lands only in accumulator rows that nobody reads.  At DH = 24 a quarter of the P V issue slots are idle.
// Plain float32, a fixed summation order, no atomics, no workspace: two calls on the same bytes give the same bits.
#include "common.h"

namespace {

constexpr float kLog2e = 1.4426950408889634f;
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
    for (int e = tid; e < 128 * C4; e += 256) {
      const int r = q0 + e / C4;
      if (r < a.T) *(float4*)(obase + (int64_t)r * a.ldo + (e % C4) * 4) = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    return;
  }
  const int i0 = q0 + wave * 32;
  const int qi = i0 + c;
  const bool wave_active = i0 < len;
  const int qic = qi < len ? qi : len - 1;

  // q pre-scaled into the log2 domain: the B operand of K Q^T; step s needs element 2s + half
  float qs[DH / 2];
  {
    const float* qrow = a.q + (int64_t)b * a.q_bstride + (int64_t)qic * a.ldq + h * DH;
    const float sc = a.scale * kLog2e;
#pragma unroll
    for (int s = 0; s < DH / 2; ++s) {
      const float2 t = *(const float2*)(qrow + 2 * s);
      qs[s] = (half ? t.y : t.x) * sc;
    }
  }

  const float* kbase = a.k + (int64_t)b * a.k_bstride + h * DH;
  const float* vbase = a.v + (int64_t)b * a.v_bstride + h * DH;
  const bool loader = tid < NLD;
  const int lrow = tid / C4, lc4 = tid % C4;   // lrow < KB for every loader

  float4 kpre = make_float4(0.f, 0.f, 0.f, 0.f), vpre = kpre;
  auto prefetch = [&](int kb) {
    if (loader) {
      int j = kb + lrow;
      j = j < len ? j : len - 1;   // clamp: finite data, masked below
      kpre = *(const float4*)(kbase + (int64_t)j * a.ldk + lc4 * 4);
      vpre = *(const float4*)(vbase + (int64_t)j * a.ldv + lc4 * 4);
    }
  };
  auto commit = [&]() {
    if (loader) {
      float* kd = Ks + lrow * LD + lc4 * 4;
      float* vd = Vs + lrow * LD + lc4 * 4;
      kd[0] = kpre.x; kd[1] = kpre.y; kd[2] = kpre.z; kd[3] = kpre.w;
      vd[0] = vpre.x; vd[1] = vpre.y; vd[2] = vpre.z; vd[3] = vpre.w;
    }
  };

  f32x16 o;
#pragma unroll
  for (int r = 0; r < 16; ++r) o[r] = 0.f;
  float m = -INFINITY, lsum = 0.f;

  prefetch(0);
  for (int kb = 0; kb < len; kb += KB) {
    __syncthreads();   // everyone is done reading the previous stage
    commit();
    __syncthreads();
    if (kb + KB < len) prefetch(kb + KB);
    if (!wave_active) continue;
    // ---- S^T block (32 keys x 32 queries)
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const float* krow = Ks + c * LD + half;
#pragma unroll
    for (int s = 0; s < DH / 2; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(krow[2 * s], qs[s], acc, 0, 0, 0);
    // ---- mask (only a stage that touches len), online softmax (per-lane query)
    const bool edge = kb + KB > len;
    float bm = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int jj = (r & 3) + 8 * (r >> 2) + 4 * half;
      if (edge && kb + jj >= len) acc[r] = -INFINITY;
      bm = fmaxf(bm, acc[r]);
    }
    bm = fmaxf(bm, __shfl_xor(bm, 32, 64));
    const float m_new = fmaxf(m, bm);   // finite: key kb is valid in every stage
    const float alpha = exp2f(m - m_new);   // m = -inf -> 0
    float ps = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      acc[r] = exp2f(acc[r] - m_new);   // -inf -> 0
      ps += acc[r];
    }
    lsum = lsum * alpha + ps;
    m = m_new;
#pragma unroll
    for (int r = 0; r < 16; ++r) o[r] *= alpha;
    // ---- O^T += V^T P^T : step s contracts keys (s&3) + 8*(s>>2) + 4*half, which is where acc[s] lives; lane c is head dimension c
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      const float* vrow = Vs + ((s & 3) + 8 * (s >> 2) + 4 * half) * LD + c;
      o = __builtin_amdgcn_mfma_f32_32x32x2f32(vrow[0], acc[s], o, 0, 0, 0);
    }
  }

  if (qi >= a.T) return;
  float* orow = obase + (int64_t)qi * a.ldo;
  lsum += __shfl_xor(lsum, 32, 64);
  const float inv = 1.0f / lsum;   // unused for the padding rows inside a block that has valid ones: zeros
  // accumulator row (r & 3) + 8 (r >> 2) + 4 half is head dimension d: this lane holds d = 8 c4 + 4 half + 0 .. 3; DH is a multiple of 8
#pragma unroll
  for (int c4 = 0; c4 < DH / 8; ++c4)
    *(float4*)(orow + 8 * c4 + 4 * half) = qi < len ? make_float4(o[c4 * 4] * inv, o[c4 * 4 + 1] * inv, o[c4 * 4 + 2] * inv, o[c4 * 4 + 3] * inv)
                                                   : make_float4(0.f, 0.f, 0.f, 0.f);
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
