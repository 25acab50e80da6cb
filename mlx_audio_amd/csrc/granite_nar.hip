// Granite Speech NAR (gfx950): the four pieces of the encoder and the projector that the library could not express.
// Reference call sites: ConformerAttention.__call__ (stt/models/granite_speech_nar/encoder.py:80-127: attention inside blocks of context_size
// frames with one Shaw table of relative positions shared by the heads, the zero-padded tail of the last block visible to the softmax), the
// self-conditioning softmax (encoder.py:278-282), _posterior_weighted_pool (encoder.py:302-334) and the window assembly of the projector
// (projector.py:190-215).  All four are plain float32 with a fixed summation order: no atomics, and nothing in the order depends on the launch
// geometry, the batch size or the other items' lengths, so two calls on the same bytes give the same bits and an item of a ragged batch is
// bit-equal to that item alone.
#include "attn_tile.h"
#include "block_reduce.h"

namespace {

// ---------------------------------------------------------------------------------------------------- Shaw block attention
// The query tile of attn_tile.h (tiling, orientation, key order, log2 domain: stated there) with 32-key stages over ONE block of ctx keys, plus
// the position term by the band technique of relpos_attn_kernel (conformer.hip).
//
// The position term.  Score (i, j) takes table row max_pos + (i - j).  With il / jl the positions inside the block, for a wave's 32 queries
// il0 .. il0 + 31 and the stage's 32 keys kb .. kb + 31 those are the 63 consecutive rows R0 .. R0 + 62, R0 = max_pos + il0 - kb - 31, and pair
// (il0 + c, kb + jj) sits at band row 31 + c - jj: the band is read in the table's OWN row order (no flipped copy).  The four waves' bands
// overlap: the workgroup stages the 159 rows from the FIRST wave's R0 once per stage (rows outside the table are clamped: only masked pairs read
// them, max_pos >= ctx - 1 is checked before the launch).  Each wave computes BD^T = table_band Q^T as two 32-row MFMA blocks, writes it to its
// own LDS slab as [band row][query] and reads its entry back at row 31 + c - jj (consecutive lanes hit consecutive banks: the offset is
// const + 33 c).  The table has no head axis, and there are no bias vectors: ONE scaled copy of q feeds both contractions.
//
// Visible zero keys.  Key j of the block with j >= lens[b] is staged as a ZERO k row and a zero v row and is NOT masked: its logit is the
// position term alone and it takes softmax mass, as the reference's zero padding of the last block does.  Only the keys past the block's own
// end (jl >= ctx, in the last stage) are masked.  Memory at and beyond lens[b] is never read.
constexpr int kShawKB = 32;                       // keys per stage
constexpr int kShawBand = kShawKB + 127;          // table rows the four waves of a stage need
template <int DH>
constexpr int shaw_lds_floats() { return (2 * kShawKB + kShawBand) * (DH + 1) + 4 * 64 * 32; }

template <int DH>
__global__ __launch_bounds__(256) void shaw_block_attn_kernel(const mi355_shaw_block_attention_args a, const int ntiles) {
  constexpr int KB = kShawKB;
  constexpr int LD = DH + 1;   // padded LDS row, floats: the A-operand ds_read_b32 of every phase is bank-conflict free
  constexpr int NDB = DH / 32;
  constexpr int NLD = (KB * DH / 4) / 256;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* Ks = smem;
  float* Vs = Ks + KB * LD;
  float* Ps = Vs + KB * LD;
  float* Bs = Ps + kShawBand * LD;   // [wave][64 band rows][32 queries]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, c = lane & 31;
  const int h = blockIdx.y, b = blockIdx.z;
  const int blk_m = blockIdx.x / ntiles, q0l = (blockIdx.x % ntiles) * 128;   // the block of ctx frames, the tile's first query inside it
  const int len = a.lens ? min(max(a.lens[b], 0), a.T) : a.T;
  const int base = blk_m * a.ctx;            // the block's first frame
  const int q0 = base + q0l;
  float* obase = a.out + (int64_t)b * a.out_bstride + h * DH;
  if (q0 >= len) {   // a tile of padding rows: zeros for its rows of this block below T
    const int rend = min(min(q0 + 128, base + a.ctx), a.T);
    for (int e = tid; e < 128 * (DH / 4); e += 256) {
      const int r = q0 + e / (DH / 4);
      if (r < rend) *(float4*)(obase + r * (int64_t)a.ldo + (e % (DH / 4)) * 4) = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    return;
  }
  const int il0 = q0l + wave * 32;
  const int il = il0 + c, qi = base + il;
  const bool wave_active = il0 < a.ctx && base + il0 < len;
  const int qic = qi < len ? qi : len - 1;

  // q pre-scaled into the log2 domain: the B operand of K Q^T and of table_band Q^T; step s needs element 2s + half
  float q[DH / 2];
  attn_load_q<DH>(q, a.q + (int64_t)b * a.q_bstride + (int64_t)qic * a.ldq + h * DH, a.scale * kLog2e, half);

  const float* kbase = a.k + (int64_t)b * a.k_bstride + h * DH;
  const float* vbase = a.v + (int64_t)b * a.v_bstride + h * DH;

  float4 kpre[NLD], vpre[NLD];
  auto prefetch = [&](int kb) {   // piece order of attn_stage_prefetch; a row at or beyond len is a zero key and a zero value
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int e = i * 256 + tid;
      const int row = e / (DH / 4), c4 = e % (DH / 4);
      const int j = base + kb + row;
      const bool real = j < len;
      kpre[i] = real ? *(const float4*)(kbase + j * (int64_t)a.ldk + c4 * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
      vpre[i] = real ? *(const float4*)(vbase + j * (int64_t)a.ldv + c4 * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  auto commit = [&](int kb) {
    attn_stage_commit<DH, NLD>(Ks, Vs, kpre, vpre, tid);
    // the stage's band of the table: LDS row x holds table row rlo + x (the first wave's R0 first)
    const int rlo = a.max_pos + q0l - kb - 31;
    for (int e = tid; e < kShawBand * (DH / 4); e += 256) {
      const int x = e / (DH / 4), c4 = e % (DH / 4);
      const int r = min(max(rlo + x, 0), a.rows - 1);
      const float4 t = *(const float4*)(a.table + (int64_t)r * a.ldt + c4 * 4);
      float* pd = Ps + x * LD + c4 * 4;
      pd[0] = t.x; pd[1] = t.y; pd[2] = t.z; pd[3] = t.w;
    }
  };

  f32x16 o[NDB];
  attn_zero(o);
  float m = -INFINITY, lsum = 0.f;
  float* bw = Bs + wave * (64 * 32);

  prefetch(0);
  for (int kb = 0; kb < a.ctx; kb += KB) {
    __syncthreads();   // everyone is done reading the previous stage (K, V, the band and the wave's own slab)
    commit(kb);
    __syncthreads();
    if (kb + KB < a.ctx) prefetch(kb + KB);
    if (!wave_active) continue;
    // ---- BD^T: band rows x0 .. x0 + 63 of the stage (this wave's R0 is 32 wave rows behind the stage's first row)
    const int x0 = 32 * wave;
#pragma unroll
    for (int blk = 0; blk < 2; ++blk) {
      // band row 63 (x = 159 for wave 3) is never read back
      const f32x16 bd = attn_kq<DH>(Ps + min(x0 + blk * 32 + c, kShawBand - 1) * LD + half, q);
#pragma unroll
      for (int r = 0; r < 16; ++r) bw[(blk * 32 + attn_c_row(r, half)) * 32 + c] = bd[r];
    }
    f32x16 acc = attn_kq<DH>(Ks + c * LD + half, q);   // S^T block (32 keys x 32 queries); exactly 0 for a zero key
    wave_lds_fence();   // the slab is this wave's own
    // ---- + the skewed position term, mask (only the stage that crosses the block's end), online softmax (per-lane query)
    const bool edge = kb + KB > a.ctx;
    float bm = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int jj = attn_c_row(r, half);
      acc[r] += bw[(31 + c - jj) * 32 + c];
      if (edge && kb + jj >= a.ctx) acc[r] = -INFINITY;
      bm = fmaxf(bm, acc[r]);
    }
    attn_online_softmax<false>(acc, bm, m, lsum, o);   // key kb is inside the block in every stage
    attn_pv(o, acc, Vs, LD, half, c);
  }

  if (il >= a.ctx || qi >= a.T) return;   // the next block's rows, rows past the tensor
  float* orow = obase + (int64_t)qi * a.ldo;
  if (qi >= len) {   // padding rows inside a tile that has valid ones
    attn_store_o<DH>(orow, o, 0.f, half, false);
    return;
  }
  attn_store_o<DH>(orow, o, attn_inv_sum<false>(lsum), half, true);
}

// ---------------------------------------------------------------------------------------------------- self-conditioning rows
// probs = softmax(logits) and p_blank = probs[:, 0].  NT threads own one row (NT = 64: one wave, four rows per workgroup; NT = 256: the
// workgroup): thread t takes the columns t, t + NT, ... in ascending order for the exact maximum and for the sum of expf(x - max), the sums are
// joined by the wave butterfly and, for NT = 256, (w0 + w1) + (w2 + w3); the last pass recomputes expf(x - max) (the same bits) and divides.
template <int NT>
__global__ __launch_bounds__(256) void selfcond_rows_kernel(const mi355_selfcond_rows_args a) {
  __shared__ float red[4];
  const int t = NT == 64 ? (threadIdx.x & 63) : threadIdx.x;
  const int64_t row = NT == 64 ? (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6) : blockIdx.x;
  if (NT == 64 && row >= a.rows) return;   // a whole wave, and this form has no barrier
  const float* xr = a.logits + row * a.ld;
  float m = -INFINITY;
  for (int c = t; c < a.V; c += NT) m = fmaxf(m, xr[c]);
  m = wave_max(m);
  if constexpr (NT == 256) m = block_join_max<4>(m, red);
  float s = 0.f;
  for (int c = t; c < a.V; c += NT) s += expf(xr[c] - m);
  s = wave_sum(s);
  if constexpr (NT == 256) s = block_join_sum<4>(s, red);
  float* pr = a.probs + row * a.ld_probs;
  for (int c = t; c < a.V; c += NT) {
    const float p = expf(xr[c] - m) / s;
    pr[c] = p;
    if (c == 0) a.p_blank[row] = p;
  }
}

// ---------------------------------------------------------------------------------------------------- posterior-weighted pooling
// One workgroup per (window, item); every thread forms the window's weights itself (the sum of 1 - p_blank over the window's real frames in
// ascending order, then one division per frame) and walks its channels c, c + 256, ... with an fmaf chain from zero over the frames ascending.
// Frames at and beyond lens[b] have weight 0 and are not read.
__global__ __launch_bounds__(256) void posterior_pool_kernel(const mi355_posterior_pool_args a) {
  const int n = blockIdx.x, b = blockIdx.y;
  const int len = a.lens ? min(max(a.lens[b], 0), a.T) : a.T;
  const int t0 = n * a.window;
  const int t1 = min(t0 + a.window, len);   // the real frames of the window
  const float* pb = a.p_blank + (int64_t)b * a.pb_bstride;
  float sum = 0.f;
  for (int t = t0; t < t1; ++t) sum += 1.0f - pb[t];
  const float den = fmaxf(sum, 1e-6f);
  const float* hb = a.h + (int64_t)b * a.h_bstride;
  float* yr = a.out + (int64_t)b * a.out_bstride + (int64_t)n * a.ldo;
  for (int c = threadIdx.x; c < a.C; c += 256) {
    float acc = 0.f;
    for (int t = t0; t < t1; ++t) acc = fmaf(hb[(int64_t)t * a.ldh + c], (1.0f - pb[t]) / den, acc);
    yr[c] = acc;
  }
}

// ---------------------------------------------------------------------------------------------------- Q-Former window assembly
// One workgroup per (window, item): row r of the window is frame n * block + r of h, zero at and beyond lens[b] (not read); kv = row +
// positions[r]; query g = query[g] + (the sum of the rows g * rate .. g * rate + rate - 1 in ascending order) / rate.
__global__ __launch_bounds__(256) void qformer_windows_kernel(const mi355_qformer_windows_args a, const int nblocks) {
  const int n = blockIdx.x, b = blockIdx.y;
  const int len = a.lens ? min(max(a.lens[b], 0), a.T) : a.T;
  const int nq = a.block / a.rate;
  const float* hb = a.h + (int64_t)b * a.h_bstride;
  const int64_t w = (int64_t)b * nblocks + n;
  float* qo = a.queries + w * nq * a.C;
  float* ko = a.kv + w * a.block * a.C;
  const float rate = (float)a.rate;
  for (int c = threadIdx.x; c < a.C; c += 256) {
    for (int g = 0; g < nq; ++g) {
      float sum = 0.f;
      for (int i = 0; i < a.rate; ++i) {
        const int r = g * a.rate + i, t = n * a.block + r;
        const float x = t < len ? hb[(int64_t)t * a.ldh + c] : 0.f;
        ko[(int64_t)r * a.C + c] = x + a.positions[(int64_t)r * a.C + c];
        sum += x;
      }
      qo[(int64_t)g * a.C + c] = a.query[(int64_t)g * a.C + c] + sum / rate;
    }
  }
}

template <int DH>
int launch_shaw(const mi355_shaw_block_attention_args& a, hipStream_t st) {
  static bool attr_set = false;
  constexpr int lds = shaw_lds_floats<DH>() * (int)sizeof(float);
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute((const void*)shaw_block_attn_kernel<DH>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    MI355_REQUIRE(e == hipSuccess, "shaw_block_attention: cannot reserve %d bytes of LDS: %s", lds, hipGetErrorString(e));
    attr_set = true;
  }
  const int ntiles = (a.ctx + 127) / 128, nblocks = (a.T + a.ctx - 1) / a.ctx;
  MI355_CLEAR_ERROR();
  hipLaunchKernelGGL(shaw_block_attn_kernel<DH>, dim3((unsigned)(ntiles * nblocks), (unsigned)a.heads, (unsigned)a.B), dim3(256), lds, st, a, ntiles);
  MI355_LAUNCH_CHECK("shaw_block_attention");
  return MI355_OK;
}

}  // namespace

extern "C" int mi355_shaw_block_attention(const mi355_shaw_block_attention_args* ap, void* stream) {
  MI355_REQUIRE(ap && ap->q && ap->k && ap->v && ap->table && ap->out, "shaw_block_attention: null tensor");
  const mi355_shaw_block_attention_args a = *ap;
  MI355_REQUIRE(a.B > 0 && a.B <= 65535 && a.heads > 0 && a.heads <= 65535 && a.T >= 1, "shaw_block_attention: bad shape");
  if (a.dh != 64 && a.dh != 128) {
    mi355_set_error("shaw_block_attention: dh must be 64 or 128 (got %d)", a.dh);
    return MI355_ERR_UNSUPPORTED;
  }
  MI355_REQUIRE(a.ctx >= 1, "shaw_block_attention: ctx must be at least 1 (got %d)", a.ctx);
  MI355_REQUIRE(a.max_pos >= a.ctx - 1, "shaw_block_attention: max_pos = %d does not hold the distances -(ctx - 1) .. ctx - 1 of ctx = %d", a.max_pos, a.ctx);
  MI355_REQUIRE(a.rows == 2 * (int64_t)a.max_pos + 1, "shaw_block_attention: the table has %d rows, max_pos = %d needs %lld", a.rows, a.max_pos,
                2 * (long long)a.max_pos + 1);
  const int hd = a.heads * a.dh;
  MI355_REQUIRE(a.ldq >= hd && a.ldk >= hd && a.ldv >= hd && a.ldo >= hd && a.ldt >= a.dh, "shaw_block_attention: a row stride is smaller than its row");
  MI355_REQUIRE(a.ldq % 4 == 0 && a.ldk % 4 == 0 && a.ldv % 4 == 0 && a.ldo % 4 == 0 && a.ldt % 4 == 0 && a.q_bstride % 4 == 0 && a.k_bstride % 4 == 0 &&
                    a.v_bstride % 4 == 0 && a.out_bstride % 4 == 0 &&
                    (((uintptr_t)a.q | (uintptr_t)a.k | (uintptr_t)a.v | (uintptr_t)a.out | (uintptr_t)a.table) & 15) == 0,
                "shaw_block_attention: rows must be 16-byte aligned");
  const int64_t tiles = (int64_t)((a.ctx + 127) / 128) * ((a.T + (int64_t)a.ctx - 1) / a.ctx);
  MI355_REQUIRE(tiles <= 0x7fffffff, "shaw_block_attention: too many query tiles");
  return a.dh == 64 ? launch_shaw<64>(a, (hipStream_t)stream) : launch_shaw<128>(a, (hipStream_t)stream);
}

extern "C" int mi355_selfcond_rows(const mi355_selfcond_rows_args* ap, void* stream) {
  MI355_REQUIRE(ap && ap->logits && ap->probs && ap->p_blank, "selfcond_rows: null tensor");
  const mi355_selfcond_rows_args a = *ap;
  MI355_REQUIRE(a.rows > 0 && a.rows <= 0x7fffffff && a.V >= 1, "selfcond_rows: bad shape");
  MI355_REQUIRE(a.ld >= a.V && a.ld_probs >= a.V, "selfcond_rows: a row stride is smaller than V");
  MI355_CLEAR_ERROR();
  if (a.V <= MI355_SELFCOND_WAVE_MAX_V)
    hipLaunchKernelGGL(selfcond_rows_kernel<64>, dim3((unsigned)((a.rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(selfcond_rows_kernel<256>, dim3((unsigned)a.rows), dim3(256), 0, (hipStream_t)stream, a);
  MI355_LAUNCH_CHECK("selfcond_rows");
  return MI355_OK;
}

extern "C" int mi355_posterior_pool(const mi355_posterior_pool_args* ap, void* stream) {
  MI355_REQUIRE(ap && ap->h && ap->p_blank && ap->out, "posterior_pool: null tensor");
  const mi355_posterior_pool_args a = *ap;
  MI355_REQUIRE(a.B > 0 && a.B <= 65535 && a.T >= 1 && a.C >= 1, "posterior_pool: bad shape");
  MI355_REQUIRE(a.window >= 1, "posterior_pool: window must be at least 1 (got %d)", a.window);
  MI355_REQUIRE(a.ldh >= a.C && a.ldo >= a.C && a.pb_bstride >= a.T, "posterior_pool: a row stride is smaller than its row");
  const int nw = (a.T + a.window - 1) / a.window;
  MI355_CLEAR_ERROR();
  hipLaunchKernelGGL(posterior_pool_kernel, dim3((unsigned)nw, (unsigned)a.B), dim3(256), 0, (hipStream_t)stream, a);
  MI355_LAUNCH_CHECK("posterior_pool");
  return MI355_OK;
}

extern "C" int mi355_qformer_windows(const mi355_qformer_windows_args* ap, void* stream) {
  MI355_REQUIRE(ap && ap->h && ap->query && ap->positions && ap->queries && ap->kv, "qformer_windows: null tensor");
  const mi355_qformer_windows_args a = *ap;
  MI355_REQUIRE(a.B > 0 && a.B <= 65535 && a.T >= 1 && a.C >= 1 && a.ldh >= a.C, "qformer_windows: bad shape");
  MI355_REQUIRE(a.block >= 1 && a.rate >= 1 && a.block % a.rate == 0, "qformer_windows: block = %d must be a positive multiple of rate = %d", a.block, a.rate);
  const int nblocks = (a.T + a.block - 1) / a.block;
  MI355_CLEAR_ERROR();
  hipLaunchKernelGGL(qformer_windows_kernel, dim3((unsigned)nblocks, (unsigned)a.B), dim3(256), 0, (hipStream_t)stream, a, nblocks);
  MI355_LAUNCH_CHECK("qformer_windows");
  return MI355_OK;
}
