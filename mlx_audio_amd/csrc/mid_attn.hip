// Mid-width attention (gfx950): softmax(scale q k^T + visibility) v for head widths 36 / 40 / 44 / 48 / 52 / 56 / 60, self or cross (Tq != Tk),
// grouped kv heads, optional causal form, plus the partial rotary row kernel that goes in front of it.
// Reference call sites: MoonshineAttention.__call__ (stt/models/moonshine/moonshine.py:96-149) with 8 heads of 36 (tiny) / 52 (base) in the encoder
// (T = 41.6 frames / s), the causal decoder over a growing cache, and the cross attention; apply_rotary_pos_emb (moonshine.py:35-58).
//
// Visibility is attn_tile.h's rule without k_start and window: key j of item b is seen iff j < lens_k[b], and under `causal` additionally
// j <= i + (len_k - len_q) (the queries are the LAST len_q positions).  The reference adds -inf style masks; invisible keys get probability exactly
// 0 here: the same function.  Output rows at and beyond lens_q[b] are written as exact zeros, and so is the row of a query with no visible key.
//
// Two forms, chosen by Tq alone (never by the data):
//   * Tq > 4: the query tile of attn_tile.h (tiling, orientation, key order, log2 domain: stated there) with 32-key stages.  K Q^T takes DH / 2
//     MFMA steps.  For P V the V^T operand is TWO 32-row blocks: lane c of block d is head dimension 32 d + c, and the rows 32 + c >= DH of the
//     second block are never stored.  Row m of an MFMA result depends on row m of the A operand alone, so whatever the lanes c >= DH - 32 of the
//     second block read (the row's zeroed pad float, the next key's row, or the zeroed tail of 64 - (DH + 1) floats behind the last row: always inside the LDS array, always
//     finite) lands only in accumulator rows that nobody reads.  At DH % 8 == 4 the last float4 of an output row belongs to half-wave 0 alone
//     (attn_store_o pairs the half-waves on 8 channels), so that one store is written here.  A stage has 32 * DH / 4 = 288 .. 480 float4 pieces per
//     operand, which the 256 threads do not divide: the stage helpers of attn_tile.h have no guard, so the guarded prefetch / commit live here.
//   * Tq <= 4, the decode step: one wavefront per (query, head, item).  Lanes own keys in chunks of 64 (online maximum and sum across chunks, any
//     Tk), then own channels for P V; the chunk's probabilities are handed over through LDS under wave_lds_fence, as attention.hip does.
// Plain float32, a fixed summation order, no atomics, no workspace: two calls on the same bytes give the same bits.
#include "attn_tile.h"

namespace {

constexpr int kMidKB = 32;   // keys per LDS stage
constexpr int kFewTq = 4;    // Tq up to here takes the one-wavefront-per-query form

// [kbeg = 0, kend): the keys the workgroup of queries q0 .. q0 + 127 has to walk
__device__ __forceinline__ int mid_key_end(const bool causal, const int q0, const int len_q, const int len_k) {
  if (!causal) return len_k;
  const int last = (q0 + 127 < len_q ? q0 + 127 : len_q - 1) + (len_k - len_q);
  return last + 1 < len_k ? last + 1 : len_k;   // may be <= 0: no key is visible to any query of the block
}

// Two waves per SIMD asked for: unbounded, the compiler spends a whole SIMD's registers on hoisted LDS reads (one wave per SIMD).
template <int DH>
__global__ __launch_bounds__(256, 2) void mid_attn_kernel(const mi355_mid_attention_args a) {
  constexpr int KB = kMidKB;
  constexpr int LD = DH + 1;            // padded LDS row, floats (odd for every DH here)
  constexpr int C4 = DH / 4;            // float4 pieces of a row
  constexpr int NP = KB * C4;           // pieces per operand per stage: 288 .. 480
  constexpr int NLD = (NP + 255) / 256; // per thread: 2, the second behind a guard
  constexpr int TAIL = 64 - LD;         // lane c = 31 of the second V^T block touches (KB - 1) * LD + 63
  static_assert(DH > 32 && DH < 64 && DH % 4 == 0 && KB % 32 == 0, "mid_attn_kernel: 32 < DH < 64");
  __shared__ float Ks[KB * LD];
  __shared__ float Vs[KB * LD + TAIL];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, c = lane & 31;
  const int h = blockIdx.y, b = blockIdx.z;
  const int g = h / (a.heads / a.kv_heads);
  const int len_q = a.lens_q ? min(max(a.lens_q[b], 0), a.Tq) : a.Tq;
  const int len_k = a.lens_k ? min(max(a.lens_k[b], 0), a.Tk) : a.Tk;
  const int q0 = blockIdx.x * 128;
  float* obase = a.out + (int64_t)b * a.out_bstride + h * DH;
  const int kend = mid_key_end(a.causal != 0, q0, len_q, len_k);
  if (q0 >= len_q || kend <= 0) {   // a block of padding rows, or of queries that see no key: zeros
    attn_zero_block<DH>(obase, a.ldo, q0, a.Tq, tid);
    return;
  }
  if (tid < TAIL) Vs[KB * LD + tid] = 0.f;   // read by the second block's idle lanes only; visible after the first stage's barrier
  if (tid < KB) Vs[tid * LD + DH] = 0.f;     // the pad float of every row (commit never writes it): what the lane 32 + c == DH reads
  const int qoff = len_k - len_q;
  const int i0 = q0 + wave * 32;
  const int qi = i0 + c;
  const bool wave_active = i0 < len_q;
  const int qic = qi < len_q ? qi : len_q - 1;
  const int qpos = qic + qoff;                                            // absolute position of this lane's query
  const int wave_last = (i0 + 31 < len_q ? i0 + 31 : len_q - 1) + qoff;   // of the wave's last valid query

  float qs[DH / 2];
  attn_load_q<DH>(qs, a.q + (int64_t)b * a.q_bstride + (int64_t)qic * a.ldq + h * DH, a.scale * kLog2e, half);

  const float* kbase = a.k + (int64_t)b * a.k_bstride + g * DH;
  const float* vbase = a.v + (int64_t)b * a.v_bstride + g * DH;

  // attn_tile.h's stage with a guard: piece e = i * 256 + tid exists for e < NP (a row of DH / 4 pieces does not divide the workgroup)
  float4 kpre[NLD], vpre[NLD];
  auto prefetch = [&](int kb) {
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int e = i * 256 + tid;
      if (e < NP) {
        int j = kb + e / C4;
        j = j < len_k ? j : len_k - 1;   // rows past len_k are clamped: finite data, masked below
        kpre[i] = *(const float4*)(kbase + j * (int64_t)a.ldk + (e % C4) * 4);
        vpre[i] = *(const float4*)(vbase + j * (int64_t)a.ldv + (e % C4) * 4);
      }
    }
  };
  auto commit = [&]() {
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int e = i * 256 + tid;
      if (e < NP) {
        float* kd = Ks + (e / C4) * LD + (e % C4) * 4;
        float* vd = Vs + (e / C4) * LD + (e % C4) * 4;
        kd[0] = kpre[i].x; kd[1] = kpre[i].y; kd[2] = kpre[i].z; kd[3] = kpre[i].w;
        vd[0] = vpre[i].x; vd[1] = vpre[i].y; vd[2] = vpre[i].z; vd[3] = vpre[i].w;
      }
    }
  };

  f32x16 o[2];
  attn_zero(o);
  float m = -INFINITY, lsum = 0.f;

  prefetch(0);
  for (int kb = 0; kb < kend; kb += KB) {
    __syncthreads();   // everyone is done reading the previous stage
    commit();
    __syncthreads();
    if (kb + KB < kend) prefetch(kb + KB);
    if (!wave_active) continue;
#pragma unroll
    for (int sub = 0; sub < KB / 32; ++sub) {
      const int kb32 = kb + sub * 32;
      if (kb32 >= kend || (a.causal && kb32 > wave_last)) break;   // wave-uniform: no query of this wave sees the keys from here on
      f32x16 acc = attn_kq<DH>(Ks + (sub * 32 + c) * LD + half, qs);   // S^T block (32 keys x 32 queries)
      // ---- mask (only a block that touches len_k or the causal diagonal of this wave), online softmax (per-lane query)
      const bool full = kb32 + 32 <= len_k && (!a.causal || kb32 + 31 <= i0 + qoff);
      float bm = -INFINITY;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        if (!full) {
          const int j = kb32 + attn_c_row(r, half);
          if (j >= len_k || (a.causal && j > qpos)) acc[r] = -INFINITY;
        }
        bm = fmaxf(bm, acc[r]);
      }
      attn_online_softmax<true>(acc, bm, m, lsum, o);
      attn_pv(o, acc, Vs + sub * 32 * LD, LD, half, c);   // lane c is head dimension c of block 0 and 32 + c of block 1
    }
  }

  if (qi >= a.Tq) return;
  // padding rows inside a block that has valid ones: zeros; a query that saw no key: inv = 0 on a zero accumulator
  const bool live = qi < len_q;
  const float inv = attn_inv_sum<true>(lsum);
  float* orow = obase + (int64_t)qi * a.ldo;
  if constexpr (DH % 8 == 0) {
    attn_store_o<DH>(orow, o, inv, half, live);
  } else {
    attn_store_o<DH - 4>(orow, o, inv, half, live);
    if (half == 0) {   // channels DH - 4 .. DH - 1: piece (DH - 4) / 8, which has no partner in half-wave 1
      constexpr int p = (DH - 4) / 8, r = (p % 4) * 4;
      const f32x16& od = o[p / 4];
      *(float4*)(orow + DH - 4) = live ? make_float4(od[r] * inv, od[r + 1] * inv, od[r + 2] * inv, od[r + 3] * inv) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
}

// ---------------------------------------------------------------------------------------------------- the few-query form
// One wavefront = one (query, head, item).  K and V stream through LDS in chunks of 64 keys exactly as the tile's stages do (coalesced float4
// pieces, the next chunk's loads in registers over the current chunk's math, rows of DH + 1 floats), under wave_lds_fence instead of s_barrier:
// the LDS is this wave's own.  Scores live in the log2 domain like the tile form's.
template <int DH>
__global__ __launch_bounds__(64) void mid_attn_few_kernel(const mi355_mid_attention_args a) {
  constexpr int LD = DH + 1, C4 = DH / 4;   // 64 * C4 pieces per operand per chunk: C4 per lane, no guard
  __shared__ float Ks[64 * LD];
  __shared__ float Vs[64 * LD];
  __shared__ __attribute__((aligned(16))) float ps[64];
  const int lane = threadIdx.x;
  const int qi = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  const int g = h / (a.heads / a.kv_heads);
  const int len_q = a.lens_q ? min(max(a.lens_q[b], 0), a.Tq) : a.Tq;
  const int len_k = a.lens_k ? min(max(a.lens_k[b], 0), a.Tk) : a.Tk;
  float* orow = a.out + (int64_t)b * a.out_bstride + (int64_t)qi * a.ldo + h * DH;
  int klim = len_k;   // the visible keys are exactly j < klim
  if (a.causal) klim = min(klim, qi + (len_k - len_q) + 1);
  if (qi >= len_q || klim <= 0) {   // wave-uniform
    if (lane < DH) orow[lane] = 0.f;
    return;
  }
  float qr[DH];   // the same for every lane (a uniform address: scalar loads), unscaled; the score takes scale * log2 e at its end
  {
    const float* qrow = a.q + (int64_t)b * a.q_bstride + (int64_t)qi * a.ldq + h * DH;
#pragma unroll
    for (int d = 0; d < DH; ++d) qr[d] = qrow[d];
  }
  const float sc = a.scale * kLog2e;
  const float* kbase = a.k + (int64_t)b * a.k_bstride + g * DH;
  const float* vbase = a.v + (int64_t)b * a.v_bstride + g * DH;
  float4 kpre[C4], vpre[C4];
  auto prefetch = [&](int j0) {
#pragma unroll
    for (int i = 0; i < C4; ++i) {
      const int e = i * 64 + lane;
      int j = j0 + e / C4;
      j = j < klim ? j : klim - 1;   // rows past klim are clamped: finite data that meets probability 0
      kpre[i] = *(const float4*)(kbase + j * (int64_t)a.ldk + (e % C4) * 4);
      vpre[i] = *(const float4*)(vbase + j * (int64_t)a.ldv + (e % C4) * 4);
    }
  };
  float m = -INFINITY, lsum = 0.f;
  float o0 = 0.f, o1 = 0.f, o2 = 0.f, o3 = 0.f;   // lane c < DH: channel c over the keys 4 t + 0 .. 3 of every chunk, joined in a fixed order at the end
  const int cc = lane < DH ? lane : 0;
  prefetch(0);
  for (int j0 = 0; j0 < klim; j0 += 64) {
    wave_lds_fence();   // the previous chunk's reads of Ks / Vs / ps are done
#pragma unroll
    for (int i = 0; i < C4; ++i) {
      const int e = i * 64 + lane;
      float* kd = Ks + (e / C4) * LD + (e % C4) * 4;
      float* vd = Vs + (e / C4) * LD + (e % C4) * 4;
      kd[0] = kpre[i].x; kd[1] = kpre[i].y; kd[2] = kpre[i].z; kd[3] = kpre[i].w;
      vd[0] = vpre[i].x; vd[1] = vpre[i].y; vd[2] = vpre[i].z; vd[3] = vpre[i].w;
    }
    wave_lds_fence();
    if (j0 + 64 < klim) prefetch(j0 + 64);
    // ---- lanes own keys: score, online maximum and sum
    float s = 0.f;
    const float* krow = Ks + lane * LD;
#pragma unroll
    for (int d = 0; d < DH; ++d) s = fmaf(qr[d], krow[d], s);
    s = j0 + lane < klim ? s * sc : -INFINITY;
    const float m_new = fmaxf(m, wave_max_fast(s));   // finite: key j0 is visible; all 64 lanes are here
    const float alpha = exp2f(m - m_new);        // m = -inf -> 0
    const float p = exp2f(s - m_new);            // -inf -> 0
    lsum = lsum * alpha + wave_sum_fast(p);      // one value for the wave
    m = m_new;
    ps[lane] = p;
    wave_lds_fence();
    // ---- lanes own channels: O = alpha O + P V over the chunk (the keys past klim carry p = 0 on a clamped, finite V row)
    o0 *= alpha; o1 *= alpha; o2 *= alpha; o3 *= alpha;
    const float* vcol = Vs + cc;
#pragma unroll 4
    for (int jj = 0; jj < 64; jj += 4) {
      const float4 p4 = *(const float4*)(ps + jj);
      o0 = fmaf(p4.x, vcol[jj * LD], o0);
      o1 = fmaf(p4.y, vcol[(jj + 1) * LD], o1);
      o2 = fmaf(p4.z, vcol[(jj + 2) * LD], o2);
      o3 = fmaf(p4.w, vcol[(jj + 3) * LD], o3);
    }
  }
  if (lane < DH) orow[lane] = ((o0 + o1) + (o2 + o3)) / lsum;
}

template <int DH>
int launch_mid_few(const mi355_mid_attention_args& a, hipStream_t st) {
  MI355_CLEAR_ERROR();
  hipLaunchKernelGGL(mid_attn_few_kernel<DH>, dim3((unsigned)a.Tq, (unsigned)a.heads, (unsigned)a.B), dim3(64), 0, st, a);
  MI355_LAUNCH_CHECK("mid_attention");
  return MI355_OK;
}

template <int DH>
int launch_mid(const mi355_mid_attention_args& a, hipStream_t st) {
  MI355_CLEAR_ERROR();
  hipLaunchKernelGGL(mid_attn_kernel<DH>, dim3((unsigned)((a.Tq + 127) / 128), (unsigned)a.heads, (unsigned)a.B), dim3(256), 0, st, a);
  MI355_LAUNCH_CHECK("mid_attention");
  return MI355_OK;
}

// ---------------------------------------------------------------------------------------------------- partial rotary embedding
// One workgroup per (row, item); a thread per channel pair of the first operand's heads, then of the second's.  In place is safe: a thread reads
// its pair before it writes it and no other thread touches that pair.
__global__ __launch_bounds__(256) void partial_rope_kernel(const mi355_partial_rope_args a) {
  const int t = blockIdx.x, b = blockIdx.y;
  if (a.lens && t >= a.lens[b]) return;
  const int hp = a.dh / 2, rp = a.rot / 2;
  const float* cr = a.cos_table + (int64_t)(a.pos0 + t) * rp;
  const float* sr = a.sin_table + (int64_t)(a.pos0 + t) * rp;
  const int n1 = a.heads * hp, n2 = a.x2 ? a.heads2 * hp : 0;
  for (int e = threadIdx.x; e < n1 + n2; e += 256) {
    const bool first = e < n1;
    const int p = first ? e : e - n1;
    const float* x = first ? a.x + (int64_t)b * a.x_bstride + (int64_t)t * a.ldx : a.x2 + (int64_t)b * a.x2_bstride + (int64_t)t * a.ldx2;
    float* y = first ? a.y + (int64_t)b * a.y_bstride + (int64_t)t * a.ldy : a.y2 + (int64_t)b * a.y2_bstride + (int64_t)t * a.ldy2;
    const int i = p % hp;   // pair inside the head
    float2 v = *(const float2*)(x + 2 * p);
    if (i < rp) rope_pair(v.x, v.y, cr[i], sr[i], v.x, v.y);
    *(float2*)(y + 2 * p) = v;
  }
}

}  // namespace

extern "C" int mi355_mid_attention(const mi355_mid_attention_args* ap, void* stream) {
  MI355_REQUIRE(ap && ap->q && ap->k && ap->v && ap->out, "mid_attention: null tensor");
  const mi355_mid_attention_args a = *ap;
  MI355_REQUIRE(a.dh >= 36 && a.dh <= 60 && a.dh % 4 == 0, "mid_attention: dh must be 36, 40, 44, 48, 52, 56 or 60 (got dh = %d)", a.dh);
  MI355_REQUIRE(a.Tq >= 1 && a.Tk >= 1, "mid_attention: Tq and Tk must be at least 1 (got Tq = %d, Tk = %d)", a.Tq, a.Tk);
  MI355_REQUIRE(a.B > 0 && a.B <= 65535 && a.heads > 0 && a.heads <= 65535 && a.kv_heads > 0, "mid_attention: bad shape");
  MI355_REQUIRE(a.heads % a.kv_heads == 0, "mid_attention: heads (%d) must be a multiple of kv_heads (%d)", a.heads, a.kv_heads);
  const int64_t hd = (int64_t)a.heads * a.dh, kd = (int64_t)a.kv_heads * a.dh;
  MI355_REQUIRE(a.ldq >= hd && a.ldo >= hd && a.ldk >= kd && a.ldv >= kd, "mid_attention: a row stride is smaller than heads * dh");
  MI355_REQUIRE(a.ldq % 4 == 0 && a.ldk % 4 == 0 && a.ldv % 4 == 0 && a.ldo % 4 == 0 && a.q_bstride % 4 == 0 && a.k_bstride % 4 == 0 &&
                    a.v_bstride % 4 == 0 && a.out_bstride % 4 == 0 && ((uintptr_t)a.q | (uintptr_t)a.k | (uintptr_t)a.v | (uintptr_t)a.out) % 16 == 0,
                "mid_attention: rows must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  if (a.Tq <= kFewTq) {
    switch (a.dh) {
      case 36: return launch_mid_few<36>(a, st);
      case 40: return launch_mid_few<40>(a, st);
      case 44: return launch_mid_few<44>(a, st);
      case 48: return launch_mid_few<48>(a, st);
      case 52: return launch_mid_few<52>(a, st);
      case 56: return launch_mid_few<56>(a, st);
      default: return launch_mid_few<60>(a, st);
    }
  }
  switch (a.dh) {
    case 36: return launch_mid<36>(a, st);
    case 40: return launch_mid<40>(a, st);
    case 44: return launch_mid<44>(a, st);
    case 48: return launch_mid<48>(a, st);
    case 52: return launch_mid<52>(a, st);
    case 56: return launch_mid<56>(a, st);
    default: return launch_mid<60>(a, st);
  }
}

extern "C" int mi355_partial_rope(const mi355_partial_rope_args* ap, void* stream) {
  MI355_REQUIRE(ap && ap->x && ap->y && ap->cos_table && ap->sin_table, "partial_rope: null tensor");
  const mi355_partial_rope_args a = *ap;
  MI355_REQUIRE(a.dh >= 4 && a.dh % 4 == 0, "partial_rope: dh must be a positive multiple of 4 (got dh = %d)", a.dh);
  MI355_REQUIRE(a.rot >= 2 && a.rot <= a.dh && a.rot % 2 == 0, "partial_rope: rot must be even and in [2, dh = %d] (got rot = %d)", a.dh, a.rot);
  MI355_REQUIRE(a.B > 0 && a.B <= 65535 && a.L >= 1 && a.heads > 0, "partial_rope: bad shape");
  MI355_REQUIRE(a.pos0 >= 0 && (int64_t)a.pos0 + a.L <= a.rope_rows, "partial_rope: positions %d..%lld run past the %d-row rotary tables", a.pos0,
                (long long)a.pos0 + a.L - 1, a.rope_rows);
  const int64_t hd = (int64_t)a.heads * a.dh;
  MI355_REQUIRE(a.ldx >= hd && a.ldy >= hd, "partial_rope: a row stride is smaller than heads * dh");
  MI355_REQUIRE(a.ldx % 2 == 0 && a.ldy % 2 == 0 && a.x_bstride % 2 == 0 && a.y_bstride % 2 == 0 && ((uintptr_t)a.x | (uintptr_t)a.y) % 8 == 0,
                "partial_rope: rows must be 8-byte aligned");
  if (a.x2) {
    const int64_t hd2 = (int64_t)a.heads2 * a.dh;
    MI355_REQUIRE(a.y2 && a.heads2 > 0, "partial_rope: the second operand needs y2 and heads2");
    MI355_REQUIRE(a.ldx2 >= hd2 && a.ldy2 >= hd2, "partial_rope: a row stride is smaller than heads2 * dh");
    MI355_REQUIRE(a.ldx2 % 2 == 0 && a.ldy2 % 2 == 0 && a.x2_bstride % 2 == 0 && a.y2_bstride % 2 == 0 && ((uintptr_t)a.x2 | (uintptr_t)a.y2) % 8 == 0,
                  "partial_rope: rows must be 8-byte aligned");
  }
  MI355_CLEAR_ERROR();
  hipLaunchKernelGGL(partial_rope_kernel, dim3((unsigned)a.L, (unsigned)a.B), dim3(256), 0, (hipStream_t)stream, a);
  MI355_LAUNCH_CHECK("partial_rope");
  return MI355_OK;
}
