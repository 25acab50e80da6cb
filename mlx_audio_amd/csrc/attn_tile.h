// The 32 x 32 query tile that flash_attn_kernel, flash_attn16_kernel (flash_attn.hip), relpos_attn_kernel (conformer.hip), narrow_attn_kernel
// (narrow_attn.hip) and mid_attn_kernel (mid_attn.hip) are built on, stated once; gau_attn_kernel (mossformer.hip) uses its orientation, C-row order and the two contraction steps
// with ReLU^2 in place of the softmax step.
//
// Tiling.  One workgroup = 128 queries x one head, 4 waves x 32 queries.  K and V stream through LDS in stages of KB keys; the next stage's global
// loads sit in registers (`prefetch`) over the current stage's math and go to LDS (`commit`) between two barriers.
//
// Orientation.  Both contractions run TRANSPOSED on v_mfma_f32_32x32x2_f32: S^T = K Q^T (A = a key row from LDS, B = the query fragment in
// registers) and O^T += V^T P^T (A = a V column from LDS, B = the probabilities).  Lane l of a wave therefore owns ONE query, column c = l & 31, of
// every accumulator; the two half-waves (half = l >> 5) hold interleaved rows of the same query.  Max, sum and rescale of the online softmax are
// per-lane scalars plus a single xor-32 exchange.
//
// C-row key order.  Accumulator register r of a lane is tile row attn_c_row(r, half) = (r & 3) + 8 (r >> 2) + 4 half.  For S^T that row is a key, so
// register r holds the score of key kb + attn_c_row(r, half); the second contraction takes its keys in the same order (step s contracts the keys
// attn_c_row(s, half) of the two half-waves), so P feeds it straight from the accumulator registers: no shuffle, no LDS round trip.  For O^T the
// row is a head dimension: registers 4 c4 .. 4 c4 + 3 of block d are the channels d * 32 + 8 c4 + 4 half + 0 .. 3, one float4 of the output row.
//
// Log2 domain.  The query fragment is pre-scaled by scale * log2(e), so the softmax is exp2f(s - m) with no multiply per score.
//
// LDS rows are DH + 1 floats.  The A operand of both phases is one ds_read_b32 per lane with the lane index in the ROW (S^T: lane = key row) or
// in the column (O^T: lane = channel); with the odd pitch the 32 rows of the first land on 32 different banks, and the second is contiguous.
//
// Visibility (flash_attn_kernel, flash_attn16_kernel) of key j for query i of item b, where len_q / len_k are the valid rows and the queries are
// the LAST len_q positions, qpos = i + (len_k - len_q):
//   k_start[b] <= j < len_k,   causal: j <= qpos,   window W > 0: j > qpos - W.
// Invisible keys get probability exactly 0 (the reference adds -1e9 / -inf style masks: identical after softmax); a query with no visible key
// gives a zero row.  relpos and narrow see the keys j < lens[b] and nothing else, so key kb of every stage they run is valid (EMPTY = false below).
// mid_attn_kernel applies the rule without k_start and window (its own args struct), with EMPTY = true.
//
// flash_attn16_kernel shares the tile, the key range, the visibility rule, the C-row order and the output store, but NOT attn_online_softmax: its
// VALU-bound softmax skips the mask on interior blocks and the rescale when no maximum moved (both wave-uniform) and calls the bare v_exp_f32.
// Folding it into the shared step would change its bits and its speed.
//
// The helpers add no floating-point operation of their own and reorder none; every flag that selects a form is a template parameter.
#pragma once
#include "common.h"

constexpr float kLog2e = 1.4426950408889634f;

// tile row of accumulator register r in half-wave `half`: the one statement of the C-layout row order
__device__ __forceinline__ int attn_c_row(const int r, const int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

// ---------------------------------------------------------------------------------------------------- key range and visibility (flash, flash16)
// [kbeg, kend): the keys the workgroup of queries q0 .. q0 + 127 has to walk, kbeg rounded down to a stage of KB keys; kstart = k_start[b] or 0
template <int KB>
__device__ __forceinline__ void attn_key_range(const mi355_flash_attn_args& a, const int b, const int q0, const int len_q, const int len_k, int& kbeg, int& kend,
                                               int& kstart) {
  const int qoff = len_k - len_q;
  kend = len_k, kbeg = 0;
  if (a.causal) {
    const int last_q = (q0 + 127 < len_q ? q0 + 127 : len_q - 1) + qoff;
    kend = last_q + 1 < len_k ? last_q + 1 : len_k;
    if (kend < 1) kend = 1;
  }
  if (a.window > 0) {
    kbeg = q0 + qoff - a.window + 1;
    if (kbeg < 0) kbeg = 0;
  }
  kstart = a.k_start ? a.k_start[b] : 0;  // left-padded rows: keys before k_start[b] are padding
  if (kstart > kbeg) kbeg = kstart;
  kbeg &= ~(KB - 1);
}

__device__ __forceinline__ bool attn_visible(const mi355_flash_attn_args& a, const int j, const int len_k, const int kstart, const int qpos) {
  bool vis = j < len_k && j >= kstart;
  if (a.causal) vis = vis && j <= qpos;
  if (a.window > 0) vis = vis && j > qpos - a.window;
  return vis;
}

// ---------------------------------------------------------------------------------------------------- fp32 query fragment and K / V stage
// B operand of S^T = K Q^T: step s needs Q[q][2s + half], pre-scaled by sc = scale * kLog2e
template <int DH>
__device__ __forceinline__ void attn_load_q(float (&q)[DH / 2], const float* qrow, const float sc, const int half) {
#pragma unroll
  for (int s = 0; s < DH / 2; ++s) {
    const float2 t = *(const float2*)(qrow + 2 * s);
    q[s] = (half ? t.y : t.x) * sc;
  }
}

// NLD float4 pieces of K and of V per thread: piece e = i * 256 + tid is row e / (DH / 4), columns 4 (e % (DH / 4)) .. + 3 of the stage at key kb.
// Rows past len are clamped (finite data, masked by the caller).  A stage of fewer than 256 pieces is NLD = 1 under the caller's `tid < pieces`.
template <int DH, int NLD>
__device__ __forceinline__ void attn_stage_prefetch(float4 (&kpre)[NLD], float4 (&vpre)[NLD], const float* kbase, const float* vbase, const int64_t ldk,
                                                    const int64_t ldv, const int kb, const int len, const int tid) {
#pragma unroll
  for (int i = 0; i < NLD; ++i) {
    const int e = i * 256 + tid;
    const int row = e / (DH / 4), c4 = e % (DH / 4);
    int j = kb + row;
    j = j < len ? j : len - 1;
    kpre[i] = *(const float4*)(kbase + j * ldk + c4 * 4);
    vpre[i] = *(const float4*)(vbase + j * ldv + c4 * 4);
  }
}
template <int DH, int NLD>
__device__ __forceinline__ void attn_stage_commit(float* Ks, float* Vs, const float4 (&kpre)[NLD], const float4 (&vpre)[NLD], const int tid) {
  constexpr int LD = DH + 1;
#pragma unroll
  for (int i = 0; i < NLD; ++i) {
    const int e = i * 256 + tid;
    const int row = e / (DH / 4), c4 = e % (DH / 4);
    float* kd = Ks + row * LD + c4 * 4;
    float* vd = Vs + row * LD + c4 * 4;
    kd[0] = kpre[i].x; kd[1] = kpre[i].y; kd[2] = kpre[i].z; kd[3] = kpre[i].w;
    vd[0] = vpre[i].x; vd[1] = vpre[i].y; vd[2] = vpre[i].z; vd[3] = vpre[i].w;
  }
}

// ---------------------------------------------------------------------------------------------------- the two contractions and the softmax step
template <int NDB>
__device__ __forceinline__ void attn_zero(f32x16 (&o)[NDB]) {
#pragma unroll
  for (int d = 0; d < NDB; ++d)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[d][r] = 0.f;
}

// S^T block (32 rows x 32 queries): krow = this lane's LDS row + half (row pitch DH + 1), q = its fragment
template <int DH>
__device__ __forceinline__ f32x16 attn_kq(const float* krow, const float (&q)[DH / 2]) {
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
  for (int s = 0; s < DH / 2; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(krow[2 * s], q[s], acc, 0, 0, 0);
  return acc;
}

// The online-softmax step behind the caller's mask loop: acc holds the masked scores (-inf = invisible) and becomes the probabilities, bm is the
// lane's maximum over acc.  EMPTY = true admits a query with no visible key so far (m stays -inf, everything 0); EMPTY = false needs a finite m_new.
template <bool EMPTY, int NDB>
__device__ __forceinline__ void attn_online_softmax(f32x16& acc, float bm, float& m, float& lsum, f32x16 (&o)[NDB]) {
  bm = fmaxf(bm, __shfl_xor(bm, 32, 64));
  const float m_new = fmaxf(m, bm);
  const float m_safe = EMPTY && m_new == -INFINITY ? 0.f : m_new;
  const float alpha = exp2f(m - m_safe);  // m = -inf -> 0
  float ps = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    acc[r] = exp2f(acc[r] - m_safe);  // -inf -> 0
    ps += acc[r];
  }
  lsum = lsum * alpha + ps;
  m = m_new;
#pragma unroll
  for (int d = 0; d < NDB; ++d)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[d][r] *= alpha;
}

// O^T += V^T P^T over the 32 keys whose V rows start at Vs (row pitch ld): step s contracts the keys attn_c_row(s, half), where p[s] lives;
// lane column c is channel d * 32 + c of block d
template <int NDB>
__device__ __forceinline__ void attn_pv(f32x16 (&o)[NDB], const f32x16& p, const float* Vs, const int ld, const int half, const int c) {
#pragma unroll
  for (int s = 0; s < 16; ++s) {
    const float* vrow = Vs + attn_c_row(s, half) * ld + c;
#pragma unroll
    for (int d = 0; d < NDB; ++d) o[d] = __builtin_amdgcn_mfma_f32_32x32x2f32(vrow[d * 32], p[s], o[d], 0, 0, 0);
  }
}

// ---------------------------------------------------------------------------------------------------- the end of a query row
// 1 / (the row's sum over both half-waves); EMPTY = true gives 0 for a query that saw no key
template <bool EMPTY>
__device__ __forceinline__ float attn_inv_sum(float lsum) {
  lsum += __shfl_xor(lsum, 32, 64);
  return EMPTY ? (lsum > 0.f ? 1.0f / lsum : 0.f) : 1.0f / lsum;
}

// This lane's DH / 8 float4 pieces of output row orow (DH a multiple of 8: a narrow head uses the first DH rows of its one block); live = false
// stores zeros, the padding-row form
template <int DH>
__device__ __forceinline__ void attn_store_o(float* orow, const f32x16* o, const float inv, const int half, const bool live) {
#pragma unroll
  for (int p = 0; p < DH / 8; ++p) {
    const f32x16& od = o[p / 4];
    const int r = (p % 4) * 4;
    *(float4*)(orow + 8 * p + 4 * half) = live ? make_float4(od[r] * inv, od[r + 1] * inv, od[r + 2] * inv, od[r + 3] * inv) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

// zeros for the workgroup's 128 output rows from q0 (those below T): a block of padding rows
template <int DH>
__device__ __forceinline__ void attn_zero_block(float* obase, const int64_t ldo, const int q0, const int T, const int tid) {
  for (int e = tid; e < 128 * (DH / 4); e += 256) {
    const int r = q0 + e / (DH / 4);
    if (r < T) *(float4*)(obase + r * ldo + (e % (DH / 4)) * 4) = make_float4(0.f, 0.f, 0.f, 0.f);
  }
}
