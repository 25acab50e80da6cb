// Mixture-of-experts FFN for gfx950 (include/mi355audio.h, "Mixture-of-experts FFN"):
//   moe_route_kernel    group_expert_select of the Ling / Ming router, one wavefront per token
//   moe_count_kernel    one workgroup: per-expert counts (integer LDS atomics), offsets, the tile list
//   moe_place_kernel    one wave per expert: the stable permutation by ballot prefix
//   moe_pack_kernel     [E, Ncols, Kdim] float32 -> bf16 hi + lo images in B-fragment order
//   moe_tile_kernel     the grouped GEMM: one (tile of 32 sorted rows) x (64 columns) per workgroup on v_mfma_f32_32x32x16_bf16
//   moe_combine_kernel  out[t] = sum_slot weights * y + shared + res
//
// The grouped GEMM.  A tile holds up to 32 rows of ONE expert, so a workgroup streams the [K x 64 columns] slab of exactly one expert, straight
// from L2 / HBM into B fragments (every weight element is used by one wave of the workgroup: LDS would only add a hop).  The tile's rows are
// gathered, split into bf16 hi + lo and staged in LDS in A-fragment order, 128 K values at a time.  Four waves: wave (cw, kg) owns columns
// [32 cw, 32 cw + 32) of the workgroup's 64 and K steps [4 kg, 4 kg + 4) of every chunk, so that a decode step (k tiles of one live row) still
// puts ceil(columns / 64) workgroups per expert on the CUs and every wave keeps a chunk's 8 - 16 KiB of weights in flight while the rows are
// staged.  The K groups are joined through LDS in a fixed order.  Three MFMAs per fragment pair (hi.hi, hi.lo, lo.hi) give float32-level
// products: what is dropped is lo.lo and the residual of the two splits, each below 2^-16 of |x| |w|.
#include <limits.h>
#include "moe_common.h"

namespace {

constexpr int TILE = MI355_MOE_TILE_ROWS;
constexpr int KC = 128;               // K values staged per chunk
constexpr int KSTEPS = KC / 16;       // MFMA K steps per chunk
constexpr int KG_STEPS = KSTEPS / 2;  // ... per K group
static_assert(TILE == 32 && MI355_MOE_COL_TILE == 64, "moe_tile_kernel is written for 32-row tiles and 64-column workgroups");

// ------------------------------------------------------------------------------------------------------------------------------ router
__global__ __launch_bounds__(256) void moe_route_kernel(const mi355_moe_route_args a) {
  constexpr int PER = MI355_MOE_MAX_EXPERTS / 64;
  __shared__ float sel_lds[4][MI355_MOE_MAX_EXPERTS];
  __shared__ float orig_lds[4][MI355_MOE_MAX_EXPERTS];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int t = blockIdx.x * 4 + wave;
  if (t >= a.N) return;   // whole waves; no workgroup barrier below
  const int E = a.E;
  const float* x = a.logits + (int64_t)t * a.ld;
  float sc[PER], sel[PER];
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int e = lane + 64 * i;
    sc[i] = e < E ? x[e] : -INFINITY;
  }
  if (a.score_fn == MI355_MOE_SIGMOID) {
#pragma unroll
    for (int i = 0; i < PER; ++i) sc[i] = 1.0f / (1.0f + expf(-sc[i]));
  } else {
    float m = sc[0];
#pragma unroll
    for (int i = 1; i < PER; ++i) m = fmaxf(m, sc[i]);
    m = wave_max(m);
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      sc[i] = lane + 64 * i < E ? expf(sc[i] - m) : 0.f;
      s += sc[i];
    }
    s = wave_sum(s);
#pragma unroll
    for (int i = 0; i < PER; ++i) sc[i] = sc[i] / s;
  }
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int e = lane + 64 * i;
    sel[i] = e < E ? (a.expert_bias ? sc[i] + a.expert_bias[e] : sc[i]) : -INFINITY;
    if (e < E) {
      sel_lds[wave][e] = sel[i];
      orig_lds[wave][e] = sc[i];
    }
  }
  wave_lds_fence();
  if (a.n_group > 1) {
    const int gsz = E / a.n_group;
    float gs = -INFINITY;
    if (lane < a.n_group) {
      float top1 = -INFINITY, top2 = -INFINITY;
      for (int j = 0; j < gsz; ++j) {
        const float v = sel_lds[wave][lane * gsz + j];
        if (v > top1) { top2 = top1; top1 = v; }
        else if (v > top2) top2 = v;
      }
      gs = top1 + top2;
    }
    int below = 0;   // groups that are zeroed before this one: a lower score, or the same score and a higher index
    for (int g = 0; g < a.n_group; ++g) {
      const float o = __shfl(gs, g, 64);
      below += (o < gs || (o == gs && g > lane)) ? 1 : 0;
    }
    const unsigned long long zmask = __ballot(lane < a.n_group && below < a.n_group - a.topk_group);
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int e = lane + 64 * i;
      if (e < E && ((zmask >> (e / gsz)) & 1ull)) sel[i] = 0.0f;
    }
  }
  unsigned taken = 0;
  int my_id = 0;
  for (int j = 0; j < a.k; ++j) {
    float bv = -INFINITY;
    int bi = INT_MAX;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int e = lane + 64 * i;
      if (e < E && !((taken >> i) & 1u) && (bi == INT_MAX || sel[i] > bv)) { bv = sel[i]; bi = e; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (oi != INT_MAX && (bi == INT_MAX || ov > bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; }
    }
    if (bi == INT_MAX) bi = 0;   // unreachable for k <= E; keeps every index in range
    if ((bi & 63) == lane) taken |= 1u << (bi >> 6);
    if (lane == j) my_id = bi;
  }
  float w = lane < a.k ? orig_lds[wave][my_id] : 0.f;
  if (a.k > 1 && a.norm_topk_prob) {
    float s = 0.f;
    for (int j = 0; j < a.k; ++j) s += __shfl(w, j, 64);
    w = w / (s + 1e-20f);
  }
  w *= a.routed_scaling_factor;
  if (lane < a.k) {
    a.ids[(int64_t)t * a.k + lane] = my_id;
    a.weights[(int64_t)t * a.k + lane] = w;
  }
}

// ------------------------------------------------------------------------------------------------------------------------------ plan
__device__ __forceinline__ int clamp_id(int v, int E) { return v < 0 ? 0 : (v >= E ? E - 1 : v); }

__global__ __launch_bounds__(MI355_MOE_MAX_EXPERTS) void moe_count_kernel(const int32_t* ids, int P, int E, int32_t* counts, int32_t* offsets,
                                                                          int4* tiles, int max_tiles) {
  constexpr int NT = MI355_MOE_MAX_EXPERTS;
  __shared__ int cnt[NT];
  __shared__ int2 scan[2][NT];
  const int tid = threadIdx.x;
  cnt[tid] = 0;
  __syncthreads();
  for (int i = tid; i < P; i += NT) atomicAdd(&cnt[clamp_id(ids[i], E)], 1);
  __syncthreads();
  const int c = tid < E ? cnt[tid] : 0;
  const int nt = (c + TILE - 1) / TILE;
  int2 v = make_int2(c, nt);   // inclusive scan of (rows, tiles) over the experts
  int cur = 0;
  scan[0][tid] = v;
  __syncthreads();
  for (int o = 1; o < NT; o <<= 1) {
    if (tid >= o) {
      const int2 u = scan[cur][tid - o];
      v.x += u.x;
      v.y += u.y;
    }
    cur ^= 1;
    scan[cur][tid] = v;
    __syncthreads();
  }
  const int total_tiles = scan[cur][NT - 1].y;
  if (tid < E) {
    const int first = v.x - c, t0 = v.y - nt;
    counts[tid] = c;
    offsets[tid] = first;
    if (tid == E - 1) offsets[E] = v.x;
    for (int j = 0; j < nt; ++j) {
      const int left = c - j * TILE;
      if (t0 + j < max_tiles) tiles[t0 + j] = make_int4(tid, first + j * TILE, left < TILE ? left : TILE, 0);
    }
  }
  for (int i = total_tiles + tid; i < max_tiles; i += NT) tiles[i] = make_int4(0, 0, 0, 0);
}

__global__ __launch_bounds__(256) void moe_place_kernel(const int32_t* ids, int P, int E, const int32_t* counts, const int32_t* offsets, int32_t* perm) {
  const int lane = threadIdx.x & 63;
  const int e = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (e >= E) return;
  const int c = counts[e];
  if (c == 0) return;
  const int base = offsets[e];
  int pos = 0;
  for (int i0 = 0; i0 < P; i0 += 64) {
    const int i = i0 + lane;
    const bool match = i < P && clamp_id(ids[i], E) == e;
    const unsigned long long mask = __ballot(match);
    const int at = pos + __popcll(mask & ((1ull << lane) - 1ull));
    if (match && at < c) perm[base + at] = i;
    pos += __popcll(mask);
  }
}

// ------------------------------------------------------------------------------------------------------------------------------ images
__global__ __launch_bounds__(256) void moe_pack_kernel(const float* w, int E, int Ncols, int Kdim, int NT, int KS, uint4* image, int64_t groups) {
  const int64_t gidx = (int64_t)blockIdx.x * 256 + threadIdx.x;   // one 8-element group of the hi image and its lo twin
  if (gidx >= groups) return;
  const int lane = (int)(gidx & 63);
  int64_t r = gidx >> 6;
  const int ks = (int)(r % KS);
  r /= KS;
  const int nt = (int)(r % NT), e = (int)(r / NT);
  const int n = nt * 32 + (lane & 31), k0 = ks * 16 + (lane >> 5) * 8;
  uint32_t hi[4], lo[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    uint32_t wd[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int kk = k0 + 2 * j + q;
      const float v = (n < Ncols && kk < Kdim) ? w[((int64_t)e * Ncols + n) * Kdim + kk] : 0.f;
      wd[q] = split16_word(v, 2);
    }
    hi[j] = (wd[0] & 0xffffu) | (wd[1] << 16);
    lo[j] = (wd[0] >> 16) | (wd[1] & 0xffff0000u);
  }
  const int64_t rec = (((int64_t)e * NT + nt) * KS + ks) * 2;
  image[(rec + 0) * 64 + lane] = make_uint4(hi[0], hi[1], hi[2], hi[3]);
  image[(rec + 1) * 64 + lane] = make_uint4(lo[0], lo[1], lo[2], lo[3]);
}

// ------------------------------------------------------------------------------------------------------------------------------ grouped GEMM
struct TileArgs {
  const float* a; int64_t lda;          // source rows [*, lda >= Kdim]
  const int32_t* perm; int kdiv;        // gather: source row of sorted row r = perm[r] / kdiv; else r itself
  int gather, scatter;                  // scatter: output row of sorted row r = perm[r]; else r itself
  const int4* tiles;
  const uint4* w0; const uint4* w1;     // images of [E, Ncols, Kdim]; w1 (the up image) for GLU only
  const float* b0; const float* b1;     // [E, Ncols], nullable
  int Kdim, Ncols, KS, NT;
  float* out; int64_t ldo;
};

template <bool GLU>
__global__ __launch_bounds__(256) void moe_tile_kernel(const TileArgs p) {
  constexpr int NI = GLU ? 2 : 1;
  __shared__ __attribute__((aligned(16))) uint16_t a_lds[KSTEPS * 2 * 64 * 8];   // [K step][hi, lo][lane][8]: 16 KiB
  __shared__ float join[2 * NI * 16 * 64];                                       // [cw][image][register][lane]
  __shared__ int src_row[TILE], out_row[TILE];
  const int4 tile = p.tiles[blockIdx.x];
  const int e = tile.x, first = tile.y, rows = tile.z;
  if (rows <= 0) return;   // a surplus record: the whole workgroup leaves
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cw = wave & 1, kg = wave >> 1;
  const int nt = blockIdx.y * 2 + cw;
  const bool live = nt < p.NT;
  if (tid < TILE) {
    const int pr = tid < rows ? ((p.gather || p.scatter) ? p.perm[first + tid] : 0) : -1;
    src_row[tid] = tid < rows ? (p.gather ? pr / p.kdiv : first + tid) : -1;
    out_row[tid] = tid < rows ? (p.scatter ? pr : first + tid) : -1;
  }
  f32x16 acc[NI];
#pragma unroll
  for (int im = 0; im < NI; ++im)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[im][i] = 0.f;
  const int64_t slab = ((int64_t)e * p.NT + (live ? nt : 0)) * p.KS * 128;   // in uint4: 2 images x 64 lanes per K step
  const uint4 zero4 = make_uint4(0, 0, 0, 0);
  for (int k0 = 0; k0 < p.Kdim; k0 += KC) {
    const int ks0 = k0 / 16 + kg * KG_STEPS;
    // this wave's weights of the chunk first: they stay in flight while the rows are staged
    uint4 b[KG_STEPS][2 * NI];
#pragma unroll
    for (int s = 0; s < KG_STEPS; ++s) {
      const bool on = live && ks0 + s < p.KS;
      const int64_t at = slab + (int64_t)(ks0 + s) * 128 + lane;
      b[s][0] = on ? p.w0[at] : zero4;
      b[s][1] = on ? p.w0[at + 64] : zero4;
      if constexpr (GLU) {
        b[s][2] = on ? p.w1[at] : zero4;
        b[s][3] = on ? p.w1[at + 64] : zero4;
      }
    }
    __syncthreads();   // src_row is written; the previous chunk's fragments are read
    for (int i = tid; i < TILE * (KC / 4); i += 256) {
      const int r = i / (KC / 4), q = i % (KC / 4);
      const int kk = k0 + 4 * q, sr = src_row[r];
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (sr >= 0 && kk < p.Kdim) v = *(const float4*)(p.a + (int64_t)sr * p.lda + kk);   // Kdim is a multiple of 4
      const uint32_t w0 = split16_word(v.x, 2), w1 = split16_word(v.y, 2), w2 = split16_word(v.z, 2), w3 = split16_word(v.w, 2);
      const int at = (((q >> 2) * 2) * 64 + ((q >> 1) & 1) * 32 + r) * 8 + (q & 1) * 4;
      *(uint2*)&a_lds[at] = make_uint2((w0 & 0xffffu) | (w1 << 16), (w2 & 0xffffu) | (w3 << 16));
      *(uint2*)&a_lds[at + 512] = make_uint2((w0 >> 16) | (w1 & 0xffff0000u), (w2 >> 16) | (w3 & 0xffff0000u));
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < KG_STEPS; ++s) {
      if (live && ks0 + s < p.KS) {
        const int ksl = kg * KG_STEPS + s;
        const bf16x8 ah = *(const bf16x8*)&a_lds[((ksl * 2 + 0) * 64 + lane) * 8];
        const bf16x8 al = *(const bf16x8*)&a_lds[((ksl * 2 + 1) * 64 + lane) * 8];
#pragma unroll
        for (int im = 0; im < NI; ++im) {
          const bf16x8 bh = __builtin_bit_cast(bf16x8, b[s][2 * im]), bl = __builtin_bit_cast(bf16x8, b[s][2 * im + 1]);
          acc[im] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc[im], 0, 0, 0);
          acc[im] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc[im], 0, 0, 0);
          acc[im] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc[im], 0, 0, 0);
        }
      }
    }
  }
  // K group 1 hands its sums to group 0: group 0 + group 1
  if (kg == 1) {
#pragma unroll
    for (int im = 0; im < NI; ++im)
#pragma unroll
      for (int i = 0; i < 16; ++i) join[((cw * NI + im) * 16 + i) * 64 + lane] = acc[im][i];
  }
  __syncthreads();
  if (kg == 1 || !live) return;
#pragma unroll
  for (int im = 0; im < NI; ++im)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[im][i] += join[((cw * NI + im) * 16 + i) * 64 + lane];
  const int col = nt * 32 + (lane & 31);
  if (col >= p.Ncols) return;
  const float bias0 = p.b0 ? p.b0[(int64_t)e * p.Ncols + col] : 0.f;
  float bias1 = 0.f;
  if constexpr (GLU) bias1 = p.b1 ? p.b1[(int64_t)e * p.Ncols + col] : 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int m = (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5);
    if (m < rows) {
      float v = acc[0][i] + bias0;
      if constexpr (GLU) v = (v / (1.0f + expf(-v))) * (acc[1][i] + bias1);   // silu(gate) * up
      p.out[(int64_t)out_row[m] * p.ldo + col] = v;
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------------------ combine
__global__ __launch_bounds__(256) void moe_combine_kernel(const float* y, const float* weights, int N, int k, int D, const float* shared, int64_t lds_,
                                                          const float* res, int64_t ldr, float* out, int64_t ldo) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int d4 = D / 4;
  if (i >= (int64_t)N * d4) return;
  const int64_t t = i / d4;
  const int c = (int)(i - t * d4) * 4;
  const float* yr = y + t * k * D + c;
  const float* w = weights + t * k;
  float4 v = *(const float4*)yr;
  float4 acc = make_float4(w[0] * v.x, w[0] * v.y, w[0] * v.z, w[0] * v.w);
  for (int s = 1; s < k; ++s) {
    v = *(const float4*)(yr + (int64_t)s * D);
    acc.x = fmaf(w[s], v.x, acc.x);
    acc.y = fmaf(w[s], v.y, acc.y);
    acc.z = fmaf(w[s], v.z, acc.z);
    acc.w = fmaf(w[s], v.w, acc.w);
  }
  if (shared) {
    v = *(const float4*)(shared + t * lds_ + c);
    acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
  }
  if (res) {
    v = *(const float4*)(res + t * ldr + c);
    acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
  }
  *(float4*)(out + t * ldo + c) = acc;
}

}  // namespace

void moe_combine_launch(const float* y, const float* weights, int N, int k, int D, const float* shared, int64_t ld_shared, const float* res, int64_t ld_res,
                        float* out, int64_t ldo, hipStream_t stream) {
  const int64_t n4 = (int64_t)N * (D / 4);
  hipLaunchKernelGGL(moe_combine_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, stream, y, weights, N, k, D, shared, ld_shared, res, ld_res, out, ldo);
}

extern "C" int mi355_moe_route(const mi355_moe_route_args* ap, void* stream) {
  MI355_REQUIRE(ap && ap->logits && ap->ids && ap->weights, "moe_route: null tensor");
  const mi355_moe_route_args a = *ap;
  MI355_REQUIRE(a.N >= 1 && a.E >= 1 && a.ld >= a.E, "moe_route: bad shape (N = %d, E = %d, ld = %lld)", a.N, a.E, (long long)a.ld);
  if (a.E > MI355_MOE_MAX_EXPERTS) {
    mi355_set_error("moe_route: E = %d is above MI355_MOE_MAX_EXPERTS = %d", a.E, MI355_MOE_MAX_EXPERTS);
    return MI355_ERR_UNSUPPORTED;
  }
  if (a.k < 1 || a.k > a.E || a.k > MI355_MOE_MAX_TOPK) {
    mi355_set_error("moe_route: k = %d must lie in [1, min(E = %d, MI355_MOE_MAX_TOPK = %d)]", a.k, a.E, MI355_MOE_MAX_TOPK);
    return MI355_ERR_UNSUPPORTED;
  }
  MI355_REQUIRE(a.score_fn == MI355_MOE_SOFTMAX || a.score_fn == MI355_MOE_SIGMOID, "moe_route: unknown score function %d", a.score_fn);
  MI355_REQUIRE(a.n_group >= 1 && a.n_group <= 64 && a.E % a.n_group == 0, "moe_route: n_group = %d must divide E = %d (and be at most 64)", a.n_group, a.E);
  if (a.n_group > 1) {
    MI355_REQUIRE(a.E / a.n_group >= 2, "moe_route: a group needs at least two experts (E = %d, n_group = %d)", a.E, a.n_group);
    MI355_REQUIRE(a.topk_group >= 1 && a.topk_group <= a.n_group, "moe_route: topk_group = %d must lie in [1, n_group = %d]", a.topk_group, a.n_group);
  }
  MI355_CLEAR_ERROR();
  hipLaunchKernelGGL(moe_route_kernel, dim3((a.N + 3) / 4), dim3(256), 0, (hipStream_t)stream, a);
  MI355_LAUNCH_CHECK("moe_route");
  return MI355_OK;
}

extern "C" int64_t mi355_moe_workspace_bytes(int32_t N, int32_t k, int32_t E, int32_t D, int32_t I) {
  Layout L;
  return moe_layout(N, k, E, D, I, &L) ? L.total : -1;
}

extern "C" int mi355_moe_workspace_layout(int32_t N, int32_t k, int32_t E, int32_t D, int32_t I, int64_t* layout) {
  Layout L;
  MI355_REQUIRE(layout, "moe_workspace_layout: null output");
  MI355_REQUIRE(moe_layout(N, k, E, D, I, &L), "moe_workspace_layout: bad sizes (N = %d, k = %d, E = %d, D = %d, I = %d)", N, k, E, D, I);
  const int64_t v[8] = {L.h, L.y, L.counts, L.offsets, L.perm, L.tiles, L.total, L.max_tiles};
  for (int i = 0; i < 8; ++i) layout[i] = v[i];
  return MI355_OK;
}

extern "C" int mi355_moe_plan(const mi355_moe_plan_args* ap, void* stream) {
  MI355_REQUIRE(ap && ap->ids, "moe_plan: null tensor");
  const mi355_moe_plan_args a = *ap;
  if (a.E > MI355_MOE_MAX_EXPERTS) {
    mi355_set_error("moe_plan: E = %d is above MI355_MOE_MAX_EXPERTS = %d", a.E, MI355_MOE_MAX_EXPERTS);
    return MI355_ERR_UNSUPPORTED;
  }
  Layout L;
  if (const int rc = moe_workspace_check("moe_plan", a.N, a.k, a.E, a.D, a.I, a.workspace, a.workspace_bytes, &L)) return rc;
  char* ws = (char*)a.workspace;
  const int P = a.N * a.k;
  MI355_CLEAR_ERROR();
  hipLaunchKernelGGL(moe_count_kernel, dim3(1), dim3(MI355_MOE_MAX_EXPERTS), 0, (hipStream_t)stream, a.ids, P, a.E, (int32_t*)(ws + L.counts),
                     (int32_t*)(ws + L.offsets), (int4*)(ws + L.tiles), (int)L.max_tiles);
  hipLaunchKernelGGL(moe_place_kernel, dim3((a.E + 3) / 4), dim3(256), 0, (hipStream_t)stream, a.ids, P, a.E, (const int32_t*)(ws + L.counts),
                     (const int32_t*)(ws + L.offsets), (int32_t*)(ws + L.perm));
  MI355_LAUNCH_CHECK("moe_plan");
  return MI355_OK;
}

extern "C" int64_t mi355_moe_image_elems(int32_t E, int32_t Ncols, int32_t Kdim) {
  if (E < 1 || Ncols < 1 || Kdim < 1) return -1;
  return (int64_t)E * ((Ncols + 31) / 32) * ((Kdim + 15) / 16) * 1024;
}

extern "C" int mi355_moe_pack(const float* w, int32_t E, int32_t Ncols, int32_t Kdim, uint16_t* image, void* stream) {
  MI355_REQUIRE(w && image && aligned16(image), "moe_pack: null tensor or misaligned image");
  MI355_REQUIRE(E >= 1 && Ncols >= 1 && Kdim >= 1, "moe_pack: bad shape (E = %d, Ncols = %d, Kdim = %d)", E, Ncols, Kdim);
  const int NT = (Ncols + 31) / 32, KS = (Kdim + 15) / 16;
  const int64_t groups = (int64_t)E * NT * KS * 64;
  MI355_REQUIRE((groups + 255) / 256 <= INT_MAX, "moe_pack: image too large");
  MI355_CLEAR_ERROR();
  hipLaunchKernelGGL(moe_pack_kernel, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, E, Ncols, Kdim, NT, KS, (uint4*)image,
                     groups);
  MI355_LAUNCH_CHECK("moe_pack");
  return MI355_OK;
}

extern "C" int mi355_moe_glu(const mi355_moe_glu_args* ap, void* stream) {
  MI355_REQUIRE(ap && ap->x && ap->w_gate && ap->out, "moe_glu: null tensor");
  const mi355_moe_glu_args a = *ap;
  MI355_REQUIRE(a.mode == 0 || a.mode == 1, "moe_glu: unknown mode %d", a.mode);
  if (a.E > MI355_MOE_MAX_EXPERTS) {
    mi355_set_error("moe_glu: E = %d is above MI355_MOE_MAX_EXPERTS = %d", a.E, MI355_MOE_MAX_EXPERTS);
    return MI355_ERR_UNSUPPORTED;
  }
  Layout L;
  if (const int rc = moe_workspace_check("moe_glu", a.N, a.k, a.E, a.D, a.I, a.workspace, a.workspace_bytes, &L)) return rc;
  MI355_REQUIRE(a.D % 4 == 0 && a.I % 4 == 0, "moe_glu: D = %d and I = %d must be multiples of 4", a.D, a.I);
  const int out_cols = a.mode == 1 ? a.I : a.D;
  MI355_REQUIRE(a.ldx >= a.D && a.ldx % 4 == 0 && aligned16(a.x) && a.ldo >= out_cols && a.ldo % 4 == 0 && aligned16(a.out),
                "moe_glu: misaligned rows (x and out rows must be 16-byte aligned and at least D / %d wide)", out_cols);
  MI355_REQUIRE(aligned16(a.w_gate), "moe_glu: misaligned weight image");
  if (a.mode == 0) {
    MI355_REQUIRE(a.w_up && a.w_down && a.weights && aligned16(a.w_up) && aligned16(a.w_down), "moe_glu: null or misaligned tensor (w_up, w_down, weights)");
    MI355_REQUIRE(!a.shared || (a.ld_shared >= a.D && a.ld_shared % 4 == 0 && aligned16(a.shared)), "moe_glu: misaligned rows (shared)");
    MI355_REQUIRE(!a.res || (a.ld_res >= a.D && a.ld_res % 4 == 0 && aligned16(a.res)), "moe_glu: misaligned rows (res)");
  }
  char* ws = (char*)a.workspace;
  float* h = (float*)(ws + L.h);
  float* y = (float*)(ws + L.y);
  const int32_t* perm = (const int32_t*)(ws + L.perm);
  TileArgs t;
  t.a = a.x; t.lda = a.ldx; t.perm = perm; t.kdiv = a.k; t.gather = 1; t.tiles = (const int4*)(ws + L.tiles);
  t.w0 = (const uint4*)a.w_gate; t.b0 = a.b_gate; t.Kdim = a.D; t.Ncols = a.I; t.KS = (a.D + 15) / 16; t.NT = (a.I + 31) / 32;
  const dim3 grid1((unsigned)L.max_tiles, (unsigned)((a.I + MI355_MOE_COL_TILE - 1) / MI355_MOE_COL_TILE));
  MI355_CLEAR_ERROR();
  if (a.mode == 1) {
    t.scatter = 1; t.w1 = nullptr; t.b1 = nullptr; t.out = a.out; t.ldo = a.ldo;
    hipLaunchKernelGGL(moe_tile_kernel<false>, grid1, dim3(256), 0, (hipStream_t)stream, t);
    MI355_LAUNCH_CHECK("moe_glu (linear)");
    return MI355_OK;
  }
  t.scatter = 0; t.w1 = (const uint4*)a.w_up; t.b1 = a.b_up; t.out = h; t.ldo = a.I;
  hipLaunchKernelGGL(moe_tile_kernel<true>, grid1, dim3(256), 0, (hipStream_t)stream, t);
  TileArgs d = t;
  d.a = h; d.lda = a.I; d.gather = 0; d.scatter = 1; d.w0 = (const uint4*)a.w_down; d.w1 = nullptr; d.b0 = a.b_down; d.b1 = nullptr;
  d.Kdim = a.I; d.Ncols = a.D; d.KS = (a.I + 15) / 16; d.NT = (a.D + 31) / 32; d.out = y; d.ldo = a.D;
  const dim3 grid2((unsigned)L.max_tiles, (unsigned)((a.D + MI355_MOE_COL_TILE - 1) / MI355_MOE_COL_TILE));
  hipLaunchKernelGGL(moe_tile_kernel<false>, grid2, dim3(256), 0, (hipStream_t)stream, d);
  moe_combine_launch(y, a.weights, a.N, a.k, a.D, a.shared, a.ld_shared, a.res, a.ld_res, a.out, a.ldo, (hipStream_t)stream);
  MI355_LAUNCH_CHECK("moe_glu");
  return MI355_OK;
}
