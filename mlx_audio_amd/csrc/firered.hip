// FireRedASR2-AED (gfx950): the four pieces the library could not express.
// Reference call sites: Conv2dSubsampling.__call__ (stt/models/fireredasr2/fireredasr2.py:17-39: two dense 3 x 3 / stride 2 convs, no padding),
// ConformerConvolution.__call__ between its pointwise convs (:111-116: GLU -> depthwise conv -> LayerNorm over 2 d_model channels -> swish), one
// step of TransformerDecoder.beam_search (:404-446) and DecoderMultiHeadAttention (:272-279) for one query per beam over a cache that stays where
// it was written.  All four are plain float32 with a fixed summation order: no atomics, and nothing in the order depends on the launch geometry, the
// batch size or the other items' lengths, so two calls on the same bytes give the same bits and an item of a ragged batch equals that item alone.
#include <atomic>
#include "block_reduce.h"
#include "dw_window.h"

namespace {

__device__ __forceinline__ float fr_sigmoid(const float x) { return 1.0f / (1.0f + expf(-x)); }

// Raises a kernel's dynamic-LDS cap once per DEVICE: `done` holds one bit per device ordinal (ordinals of 64 and above set it on every call).  Two
// threads that meet here both make the call, which is idempotent; a launch never runs on a device whose cap this thread has not seen raised.
inline hipError_t raise_lds_cap(const void* kernel, const int bytes, std::atomic<uint64_t>& done) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  const uint64_t bit = (dev >= 0 && dev < 64) ? (1ull << dev) : 0ull;
  if (bit && (done.load(std::memory_order_acquire) & bit)) return hipSuccess;
  e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e == hipSuccess && bit) done.fetch_or(bit, std::memory_order_release);
  return e;
}

// ---------------------------------------------------------------------------------------------------- dense 3 x 3 / stride 2, valid padding
// One workgroup = rpb output rows of one item (8, halved while the launch would have fewer than 512 workgroups: every output is computed on its own,
// so the bits do not depend on it); its threads walk the (row, frequency, four output channels) triples of the group, 256 at a time.
// The weights sit in LDS as [tap][ci][co]: the threads of a wave that differ in co read adjacent 16-byte pieces, the others the same address (a
// broadcast).  Per output: the bias, then one fmaf per (kh, kw, ci) in that order.
constexpr int kSubRows = 8;   // the most rows per workgroup

__global__ __launch_bounds__(256) void subsample2d_k3s2_kernel(const mi355_subsample2d_k3s2_args a, const int To, const int Fo, const int rpb) {
  extern __shared__ __attribute__((aligned(16))) float wl[];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int Cin = a.Cin, Cout = a.Cout, q = Cout >> 2;
  const int len_in = a.lens_in ? min(max(a.lens_in[b], 0), a.T) : a.T;
  const int len_out = a.lens_out ? min(max(a.lens_out[b], 0), To) : To;
  const int tfirst = blockIdx.x * rpb;
  const int rows = min(rpb, To - tfirst);
  if (tfirst < len_out) {   // block-uniform: a group of padding rows needs no weights
    const int nw = Cout * 9 * Cin;
    for (int i = tid; i < nw; i += 256) {   // w [co][tap][ci] -> wl [tap][ci][co]
      const int ci = i % Cin, tap = (i / Cin) % 9, c = i / (9 * Cin);
      wl[(tap * Cin + ci) * Cout + c] = a.w[i];
    }
    __syncthreads();
  }
  const float* xb = a.x + (int64_t)b * a.x_bstride;
  float* yb = a.y + (int64_t)b * a.y_bstride;
  for (int e = tid; e < rows * Fo * q; e += 256) {
    const int co = (e % q) * 4, f = (e / q) % Fo, t = tfirst + e / (q * Fo);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (t < len_out) {
      if (a.bias) acc = *(const float4*)(a.bias + co);
      for (int kh = 0; kh < 3; ++kh) {
        const int ti = 2 * t + kh;
        const bool ok = ti < len_in;
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
          const float* xp = xb + ((int64_t)ti * a.F + (2 * f + kw)) * Cin;
          const float* wp = wl + (kh * 3 + kw) * Cin * Cout + co;
          if (Cin == 1) {
            const float xv = ok ? xp[0] : 0.f;
            const float4 w4 = *(const float4*)wp;
            acc.x = fmaf(w4.x, xv, acc.x); acc.y = fmaf(w4.y, xv, acc.y); acc.z = fmaf(w4.z, xv, acc.z); acc.w = fmaf(w4.w, xv, acc.w);
          } else {
            for (int ci = 0; ci < Cin; ci += 4) {
              const float4 x4 = ok ? *(const float4*)(xp + ci) : make_float4(0.f, 0.f, 0.f, 0.f);
              const float xs[4] = {x4.x, x4.y, x4.z, x4.w};
#pragma unroll
              for (int u = 0; u < 4; ++u) {
                const float4 w4 = *(const float4*)(wp + (ci + u) * Cout);
                acc.x = fmaf(w4.x, xs[u], acc.x); acc.y = fmaf(w4.y, xs[u], acc.y); acc.z = fmaf(w4.z, xs[u], acc.z); acc.w = fmaf(w4.w, xs[u], acc.w);
              }
            }
          }
        }
      }
      if (a.relu) { acc.x = fmaxf(acc.x, 0.f); acc.y = fmaxf(acc.y, 0.f); acc.z = fmaxf(acc.z, 0.f); acc.w = fmaxf(acc.w, 0.f); }
    }
    if (a.out_cf) {
      float* yp = yb + ((int64_t)t * Cout + co) * Fo + f;
      yp[0] = acc.x; yp[Fo] = acc.y; yp[2 * Fo] = acc.z; yp[3 * Fo] = acc.w;
    } else {
      *(float4*)(yb + ((int64_t)t * Fo + f) * Cout + co) = acc;
    }
  }
}

// ---------------------------------------------------------------------------------------------------- GLU -> depthwise conv -> LayerNorm -> swish
// One workgroup of NT threads owns RUN rows (kRun, or half of it for small launches: launch_glu_ln) of one item across all C channels; thread i runs the register window of dw_window.h over the channels
// i, i + NT, ... one after the other and keeps their RUN outputs z in registers (NCH * RUN of them: 160 at 2560 channels, 512 threads and 32 rows, which
// leaves two waves per SIMD; 256 threads with ten channels each would hold 320 and leave one).
// The row statistics: per thread over its channels ascending, wave_sum_fast, block_join_sum_rows; the mean first, then the squared deviations.
// The RUN outputs of channel J * NT + threadIdx.x (zero beyond C).  One instantiation per J instead of a loop over the channels: a loop of this size
// is beyond what the compiler unrolls, and z must be indexed by constants to stay in registers.
template <int KMAX, int NT, int NCH, int RUN, int J>
__device__ __forceinline__ void glu_dw_channels(float (&z)[NCH][RUN], const mi355_glu_dwconv_ln_swish_args& a, const float* xb, const int t0, const int len) {
  if constexpr (J < NCH) {
    const int c = J * NT + threadIdx.x;
    if (c < a.C) {
      const int shift = dw_tap_shift<KMAX>(a.K);
      float w[KMAX];
#pragma unroll
      for (int jj = 0; jj < KMAX; ++jj) {
        const int k = jj - shift;
        w[jj] = (k >= 0 && k < a.K) ? a.w[(int64_t)c * a.K + k] : 0.f;
      }
      float win[RUN + KMAX - 1];
      const auto row = [xc = xb + c, ldx = a.ldx, C = a.C](const int r) {
        const float* xr = xc + (int64_t)r * ldx;
        return xr[0] * fr_sigmoid(xr[C]);
      };
#pragma unroll
      for (int i = 0; i < RUN + KMAX - 1; ++i) win[i] = dw_window_row<KMAX>(i, t0, len, row);
#pragma unroll
      for (int i = 0; i < RUN; ++i) z[J][i] = dw_tap_sum<KMAX, RUN>(w, win, i, 0.f);
    } else {
#pragma unroll
      for (int i = 0; i < RUN; ++i) z[J][i] = 0.f;
    }
    glu_dw_channels<KMAX, NT, NCH, RUN, J + 1>(z, a, xb, t0, len);
  }
}

template <int KMAX, int NT, int NCH, int RUN>
__global__ __launch_bounds__(NT) void glu_dwconv_ln_swish_kernel(const mi355_glu_dwconv_ln_swish_args a) {
  constexpr int NW = NT / 64;
  __shared__ float red[NW * RUN];
  const int tid = threadIdx.x, b = blockIdx.y, t0 = blockIdx.x * RUN;
  const int C = a.C;
  const int len = dw_len(a.lens, b, a.L);
  float* yb = a.y + (int64_t)b * a.y_bstride;
  if (t0 >= len) {   // a tile of padding rows: zeros
    const int rows = min(RUN, a.L - t0);
    for (int i = tid; i < rows * (C >> 2); i += NT) {
      const int r = i / (C >> 2), c4 = i % (C >> 2);
      *(float4*)(yb + (int64_t)(t0 + r) * a.ldy + c4 * 4) = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    return;
  }
  const float* xb = a.x + (int64_t)b * a.x_bstride;
  float z[NCH][RUN];
  glu_dw_channels<KMAX, NT, NCH, RUN, 0>(z, a, xb, t0, len);
  const float invC = 1.0f / (float)C;
  float part[RUN], mean[RUN], rstd[RUN];
#pragma unroll
  for (int i = 0; i < RUN; ++i) {
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < NCH; ++j) s += z[j][i];   // channels beyond C hold zero
    part[i] = wave_sum_fast(s);
  }
  block_join_sum_rows<NW, RUN>(part, red, mean);
#pragma unroll
  for (int i = 0; i < RUN; ++i) {
    mean[i] *= invC;
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
      const float d = z[j][i] - mean[i];
      z[j][i] = d;
      s = (j * NT + tid < C) ? fmaf(d, d, s) : s;
    }
    part[i] = wave_sum_fast(s);
  }
  block_join_sum_rows<NW, RUN>(part, red, rstd);
#pragma unroll
  for (int i = 0; i < RUN; ++i) rstd[i] = 1.0f / sqrtf(rstd[i] * invC + a.eps);
#pragma unroll
  for (int j = 0; j < NCH; ++j) {
    const int c = j * NT + tid;
    if (c >= C) continue;
    const float lw = a.ln_w[c], lb = a.ln_b[c];
#pragma unroll
    for (int i = 0; i < RUN; ++i) {
      const int t = t0 + i;
      if (t < a.L) {
        const float n = fmaf(z[j][i] * rstd[i], lw, lb);
        yb[(int64_t)t * a.ldy + c] = t < len ? n * fr_sigmoid(n) : 0.f;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------- one beam-search step
// One workgroup per utterance.  Per live beam: the exact max of u = logit / smoothing, the sum of exp(u - max) (thread i over the columns i, i + 256,
// ... ascending; wave butterfly; (w0 + w1) + (w2 + w3)), then B rounds of block_argmax over the columns other than eos: a round takes the largest
// (logit, lowest id) that comes after the previous round's winner in that order, so nothing is marked.  Thread 0 evaluates t for the B winners and
// eos, inserts eos, then picks the B best of the B x B sums; all threads move the histories.
__device__ __forceinline__ float beam_t(const float logit, const float sm, const float M, const float S) {
  return logf(expf(logit / sm - M) / S + 1e-10f);
}

__global__ __launch_bounds__(256) void beam_step_kernel(const mi355_beam_step_args a) {
  constexpr int BM = MI355_BEAM_MAX;
  __shared__ float redv[4];
  __shared__ int redi[4];
  __shared__ int s_state[2], s_fin[BM];
  __shared__ float s_nsc[BM];
  __shared__ float s_ct[BM * BM];   // the candidates [beam][rank]: written and read by thread 0 alone
  __shared__ int s_cid[BM * BM];
  __shared__ int s_bidx[BM], s_tok[BM];
  __shared__ float s_conf[BM];
  const int n = blockIdx.x, tid = threadIdx.x, B = a.B, V = a.V, eos = a.eos_id;
  if (tid == 0) { s_state[0] = a.done[n]; s_state[1] = a.step[n]; }
  if (tid < B) s_fin[tid] = a.finished[n * B + tid];
  __syncthreads();
  if (s_state[0] != 0) return;   // a frozen utterance: nothing of it is written
  const int st = s_state[1];
  if (st < 1 || st >= a.Tmax) {
    if (tid == 0) a.done[n] = 1;
    return;
  }
  const float sm = a.softmax_smoothing;
  for (int i = 0; i < B; ++i) {
    if (s_fin[i] != 0) {   // block-uniform
      if (tid == 0)
        for (int r = 0; r < B; ++r) { s_ct[i * BM + r] = r == 0 ? 0.f : -1e10f; s_cid[i * BM + r] = eos; }
      continue;
    }
    const float* xr = a.logits + ((int64_t)n * B + i) * a.ld;
    float m = -INFINITY;
    for (int c = tid; c < V; c += 256) m = fmaxf(m, xr[c] / sm);
    const float M = block_join_max<4>(wave_max(m), redv);
    float s = 0.f;
    for (int c = tid; c < V; c += 256) s += expf(xr[c] / sm - M);
    const float S = block_join_sum<4>(wave_sum(s), redv);
    float wt[BM];   // the B largest logits other than eos as t, best first (compile-time indices)
    int wid[BM];
    ArgMax prev;
    prev.v = INFINITY;
    prev.i = -1;
#pragma unroll
    for (int r = 0; r < BM; ++r) {
      wt[r] = -INFINITY;
      wid[r] = eos;
      if (r >= B) continue;   // block-uniform
      ArgMax am;
      am.v = -INFINITY;
      am.i = 0x7fffffff;
      for (int c = tid; c < V; c += 256) {
        const float x = xr[c];
        const bool after = x < prev.v || (x == prev.v && c > prev.i);
        if (after && c != eos && (x > am.v || am.i == 0x7fffffff)) { am.v = x; am.i = c; }
      }
      prev = block_argmax<4>(am, redv, redi);
      wt[r] = beam_t(prev.v, sm, M, S);
      wid[r] = min(prev.i, V - 1);
    }
    if (tid == 0) {
      // eos goes in front of the first entry it beats: a larger t, or an equal t and the lower token id
      const float te = beam_t(xr[eos], sm, M, S) * a.eos_penalty;
      int pe = B;
#pragma unroll
      for (int r = BM - 1; r >= 0; --r)
        if (r < B && (te > wt[r] || (te == wt[r] && eos < wid[r]))) pe = r;
#pragma unroll
      for (int r = 0; r < BM; ++r) {
        if (r >= B) continue;
        const float tb = r > 0 ? wt[r > 0 ? r - 1 : 0] : 0.f;
        const int ib = r > 0 ? wid[r > 0 ? r - 1 : 0] : 0;
        s_ct[i * BM + r] = r < pe ? wt[r] : (r == pe ? te : tb);
        s_cid[i * BM + r] = r < pe ? wid[r] : (r == pe ? eos : ib);
      }
    }
  }
  if (tid == 0) {
    float pv = INFINITY;           // the previous pick in the order (sum desc, beam asc, token asc, rank asc)
    int pi = -1, pid = -1, pr = -1, nfin = 0;
    for (int j = 0; j < B; ++j) {
      float bv = -INFINITY, bt = -INFINITY;
      int bi = -1, bid = eos, br = 0;
      for (int i = 0; i < B; ++i) {
        const float sci = a.scores[n * B + i];
        for (int r = 0; r < B; ++r) {
          const float v = sci + s_ct[i * BM + r];
          const int id = s_cid[i * BM + r];
          const bool after = v < pv || (v == pv && (i > pi || (i == pi && (id > pid || (id == pid && r > pr)))));
          if (!after) continue;
          const bool wins = bi < 0 || v > bv || (v == bv && (i < bi || (i == bi && (id < bid || (id == bid && r < br)))));
          if (wins) { bv = v; bi = i; bid = id; br = r; bt = s_ct[i * BM + r]; }
        }
      }
      if (bi < 0) bi = 0;   // NaN scores only: every index stays valid
      pv = bv; pi = bi; pid = bid; pr = br;
      s_bidx[j] = bi; s_tok[j] = bid; s_conf[j] = expf(bt);
      nfin += bid == eos;
      s_nsc[j] = bv;
    }
    for (int j = 0; j < B; ++j) {   // after every score has been read
      a.scores[n * B + j] = s_nsc[j];
      a.finished[n * B + j] = s_tok[j] == eos;
      a.beam_idx[n * B + j] = s_bidx[j];
      a.new_tokens[n * B + j] = s_tok[j];
      if (a.new_conf) a.new_conf[n * B + j] = s_conf[j];
    }
    if (nfin == B || st + 1 == a.max_steps[n]) a.done[n] = 1;
    a.step[n] = st + 1;
  }
  __syncthreads();
  const int64_t hb = (int64_t)n * B * a.Tmax;
  for (int e = tid; e < B * (st + 1); e += 256) {
    const int j = e / (st + 1), s = e % (st + 1);
    const int64_t dst = hb + (int64_t)j * a.Tmax + s, src = hb + (int64_t)s_bidx[j] * a.Tmax + s;
    const bool last = s == st;
    a.tokens_out[dst] = last ? s_tok[j] : a.tokens_in[src];
    a.ind_out[dst] = last ? j : a.ind_in[src];
    if (a.conf_out) a.conf_out[dst] = last ? s_conf[j] : a.conf_in[src];
  }
}

// ---------------------------------------------------------------------------------------------------- attention over the unmoved cache
// One wave per (utterance, beam, head), four heads per workgroup; the waves share nothing (wave_lds_fence, no barrier).  Per wave in LDS: the query,
// the scores / probabilities of the keys and the slot of each key.
template <int DH>
__global__ __launch_bounds__(256) void beam_attention_kernel(const mi355_beam_attention_args a, const int tkp) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int h = blockIdx.x * 4 + wave, nb = blockIdx.y;
  if (h >= a.heads) return;
  const int n = nb / a.B;
  float* qs = smem + wave * (DH + 2 * tkp);
  float* sc = qs + DH;
  int* sl = (int*)(sc + tkp);
  constexpr int PL = DH / 64;   // output channels per lane
  float* orow = a.out + (int64_t)nb * a.ldo + h * DH + lane * PL;
  const int p = a.pos[n];
  if (p < 0) {
#pragma unroll
    for (int u = 0; u < PL; ++u) orow[u] = 0.f;
    return;
  }
  const int nk = min(p, a.Tk - 1) + 1;
  const float* qrow = a.q + (int64_t)nb * a.ldq + h * DH;
#pragma unroll
  for (int u = 0; u < PL; ++u) qs[lane + 64 * u] = qrow[lane + 64 * u];
  wave_lds_fence();
  const int32_t* irow = a.ind + (int64_t)nb * a.ld_ind;
  float mx = -INFINITY;
  for (int s = lane; s < nk; s += 64) {
    const int slot = min(max(irow[s], 0), a.B - 1);
    const float* kr = a.k + ((int64_t)n * a.B + slot) * a.k_sstride + (int64_t)s * a.ldk + h * DH;
    float acc = 0.f;
#pragma unroll
    for (int d = 0; d < DH; d += 4) {
      const float4 kk = *(const float4*)(kr + d);
      const float4 qq = *(const float4*)(qs + d);
      acc = fmaf(qq.x, kk.x, acc); acc = fmaf(qq.y, kk.y, acc); acc = fmaf(qq.z, kk.z, acc); acc = fmaf(qq.w, kk.w, acc);
    }
    acc *= a.scale;
    sc[s] = acc;
    sl[s] = slot;
    mx = fmaxf(mx, acc);
  }
  mx = wave_max(mx);
  float ls = 0.f;
  for (int s = lane; s < nk; s += 64) {
    const float e = expf(sc[s] - mx);
    sc[s] = e;
    ls += e;
  }
  const float S = wave_sum(ls);
  for (int s = lane; s < nk; s += 64) sc[s] = sc[s] / S;
  wave_lds_fence();
  float acc[PL];
#pragma unroll
  for (int u = 0; u < PL; ++u) acc[u] = 0.f;
  const float* vb = a.v + (int64_t)n * a.B * a.v_sstride + h * DH + lane * PL;
#pragma unroll 4
  for (int s = 0; s < nk; ++s) {
    const float* vr = vb + (int64_t)sl[s] * a.v_sstride + (int64_t)s * a.ldv;
    const float pr = sc[s];
    if constexpr (PL == 2) {
      const float2 vv = *(const float2*)vr;
      acc[0] = fmaf(pr, vv.x, acc[0]);
      acc[1] = fmaf(pr, vv.y, acc[1]);
    } else {
      acc[0] = fmaf(pr, vr[0], acc[0]);
    }
  }
#pragma unroll
  for (int u = 0; u < PL; ++u) orow[u] = acc[u];
}

// The row tile against the halo re-read: a tile of RUN rows gates RUN + K - 1 window rows per channel, so 32 rows cost 2 x the gating of the
// compulsory rows at 33 taps and 16 rows 3 x -- but a launch of fewer workgroups than CUs leaves CUs idle, and there the shorter tile's twice as
// many workgroups are worth its larger halo (docs/BENCH_LINES.md).  Every output and every row statistic is computed the same way under both, so the
// bits do not depend on the choice.
template <int KMAX, int NT, int NCH>
void launch_glu_ln(const mi355_glu_dwconv_ln_swish_args& a, hipStream_t st) {
  constexpr int kShort = MI355_GLU_DWCONV_LN_ROWS / 2;
  if ((int64_t)((a.L + kRun - 1) / kRun) * a.B < 256)
    hipLaunchKernelGGL((glu_dwconv_ln_swish_kernel<KMAX, NT, NCH, kShort>), dim3((unsigned)((a.L + kShort - 1) / kShort), (unsigned)a.B), dim3(NT), 0, st, a);
  else
    hipLaunchKernelGGL((glu_dwconv_ln_swish_kernel<KMAX, NT, NCH, kRun>), dim3((unsigned)((a.L + kRun - 1) / kRun), (unsigned)a.B), dim3(NT), 0, st, a);
}

// Up to 1024 channels: 256 threads with up to four channels each.  Wider rows: 512 threads with up to five each, so that two waves share a SIMD.
// The geometry is a function of C alone (it fixes the order of the row sums).
template <int KMAX>
void launch_glu_ln_k(const mi355_glu_dwconv_ln_swish_args& a, hipStream_t st) {
  if (a.C <= 256) launch_glu_ln<KMAX, 256, 1>(a, st);
  else if (a.C <= 512) launch_glu_ln<KMAX, 256, 2>(a, st);
  else if (a.C <= 1024) launch_glu_ln<KMAX, 256, 4>(a, st);
  else if (a.C <= 1536) launch_glu_ln<KMAX, 512, 3>(a, st);
  else if (a.C <= 2048) launch_glu_ln<KMAX, 512, 4>(a, st);
  else launch_glu_ln<KMAX, 512, 5>(a, st);
}

template <int DH>
int launch_beam_attention(const mi355_beam_attention_args& a, hipStream_t st) {
  static std::atomic<uint64_t> configured{0};   // per instantiation and device: the cap of the largest Tk
  const int tkp = (a.Tk + 63) / 64 * 64;
  constexpr int cap = 4 * (DH + 2 * MI355_BEAM_ATTN_MAX_TK) * (int)sizeof(float);
  const hipError_t e = raise_lds_cap((const void*)beam_attention_kernel<DH>, cap, configured);
  MI355_REQUIRE(e == hipSuccess, "beam_attention: cannot reserve %d bytes of LDS: %s", cap, hipGetErrorString(e));
  const int lds = 4 * (DH + 2 * tkp) * (int)sizeof(float);
  MI355_CLEAR_ERROR();
  hipLaunchKernelGGL(beam_attention_kernel<DH>, dim3((unsigned)((a.heads + 3) / 4), (unsigned)(a.N * a.B)), dim3(256), lds, st, a, tkp);
  MI355_LAUNCH_CHECK("beam_attention");
  return MI355_OK;
}

}  // namespace

extern "C" int mi355_subsample2d_k3s2(const mi355_subsample2d_k3s2_args* ap, void* stream) {
  MI355_REQUIRE(ap && ap->x && ap->w && ap->y, "subsample2d_k3s2: null tensor");
  const mi355_subsample2d_k3s2_args a = *ap;
  MI355_REQUIRE(a.B > 0 && a.B <= 65535 && a.T >= 3 && a.F >= 3, "subsample2d_k3s2: bad shape (T and F must be at least 3)");
  MI355_REQUIRE(a.Cout >= 4 && a.Cout % 4 == 0 && a.Cout <= MI355_SUBSAMPLE2D_MAX_COUT, "subsample2d_k3s2: Cout must be a multiple of 4, <= %d (got %d)",
                MI355_SUBSAMPLE2D_MAX_COUT, a.Cout);
  MI355_REQUIRE(a.Cin == 1 || a.Cin == a.Cout, "subsample2d_k3s2: Cin is 1 or Cout (got %d)", a.Cin);
  const int To = (a.T - 3) / 2 + 1, Fo = (a.F - 3) / 2 + 1;
  MI355_REQUIRE((int64_t)a.T * a.F * a.Cin <= a.x_bstride && (int64_t)To * Fo * a.Cout <= a.y_bstride, "subsample2d_k3s2: a batch stride is smaller than an item");
  MI355_REQUIRE(((uintptr_t)a.y | (uintptr_t)a.bias) % 16 == 0 && a.y_bstride % 4 == 0 && (a.Cin == 1 || ((uintptr_t)a.x % 16 == 0 && a.x_bstride % 4 == 0)),
                "subsample2d_k3s2: channel rows and the bias must be 16-byte aligned");
  int rpb = kSubRows;
  while (rpb > 1 && (int64_t)((To + rpb - 1) / rpb) * a.B < 512) rpb >>= 1;
  const int64_t gy = ((int64_t)To + rpb - 1) / rpb;
  MI355_REQUIRE(gy <= 0x7fffffff, "subsample2d_k3s2: sequence too long");
  const int lds = a.Cout * 9 * a.Cin * (int)sizeof(float);
  static std::atomic<uint64_t> configured{0};
  constexpr int cap = MI355_SUBSAMPLE2D_MAX_COUT * MI355_SUBSAMPLE2D_MAX_COUT * 9 * (int)sizeof(float);
  const hipError_t e = raise_lds_cap((const void*)subsample2d_k3s2_kernel, cap, configured);
  MI355_REQUIRE(e == hipSuccess, "subsample2d_k3s2: cannot reserve %d bytes of LDS: %s", cap, hipGetErrorString(e));
  MI355_CLEAR_ERROR();
  hipLaunchKernelGGL(subsample2d_k3s2_kernel, dim3((unsigned)gy, (unsigned)a.B), dim3(256), lds, (hipStream_t)stream, a, To, Fo, rpb);
  MI355_LAUNCH_CHECK("subsample2d_k3s2");
  return MI355_OK;
}

extern "C" int mi355_glu_dwconv_ln_swish(const mi355_glu_dwconv_ln_swish_args* ap, void* stream) {
  MI355_REQUIRE(ap && ap->x && ap->w && ap->ln_w && ap->ln_b && ap->y, "glu_dwconv_ln_swish: null tensor");
  const mi355_glu_dwconv_ln_swish_args a = *ap;
  MI355_REQUIRE(a.B > 0 && a.B <= 65535 && a.L > 0, "glu_dwconv_ln_swish: bad shape");
  MI355_REQUIRE(a.C >= 4 && a.C % 4 == 0 && a.C <= MI355_GLU_DWCONV_LN_MAX_C, "glu_dwconv_ln_swish: C must be a multiple of 4, <= %d (got %d)", MI355_GLU_DWCONV_LN_MAX_C,
                a.C);
  MI355_REQUIRE(a.K >= 1 && a.K <= MI355_GLU_DWCONV_LN_MAX_TAPS && (a.K & 1) == 1, "glu_dwconv_ln_swish: K must be odd and <= %d (got %d)", MI355_GLU_DWCONV_LN_MAX_TAPS,
                a.K);
  MI355_REQUIRE(a.ldx >= 2 * a.C && a.ldy >= a.C, "glu_dwconv_ln_swish: a row stride is too small (x rows hold 2 C values)");
  MI355_REQUIRE(a.ldy % 4 == 0 && a.y_bstride % 4 == 0 && (uintptr_t)a.y % 16 == 0, "glu_dwconv_ln_swish: y rows must be 16-byte aligned");
  MI355_REQUIRE((const void*)a.y != (const void*)a.x, "glu_dwconv_ln_swish: y must not alias x (a step reads its neighbours' values)");
  MI355_REQUIRE(((int64_t)a.L + kRun - 1) / kRun <= 0x7fffffff, "glu_dwconv_ln_swish: sequence too long");
  MI355_CLEAR_ERROR();
  // the register window holds 1, 15 or 33 taps; a shorter kernel is centred in the next larger one (its other taps are zero)
  if (a.K == 1) launch_glu_ln_k<1>(a, (hipStream_t)stream);
  else if (a.K <= 15) launch_glu_ln_k<15>(a, (hipStream_t)stream);
  else launch_glu_ln_k<MI355_GLU_DWCONV_LN_MAX_TAPS>(a, (hipStream_t)stream);
  MI355_LAUNCH_CHECK("glu_dwconv_ln_swish");
  return MI355_OK;
}

extern "C" int mi355_beam_step(const mi355_beam_step_args* ap, void* stream) {
  MI355_REQUIRE(ap && ap->logits && ap->scores && ap->finished && ap->step && ap->max_steps && ap->done && ap->tokens_in && ap->tokens_out && ap->ind_in &&
                    ap->ind_out && ap->beam_idx && ap->new_tokens,
                "beam_step: null tensor");
  const mi355_beam_step_args a = *ap;
  MI355_REQUIRE(a.N > 0 && a.Tmax >= 2, "beam_step: bad shape");
  if (a.B < 1 || a.B > MI355_BEAM_MAX) {
    mi355_set_error("beam_step: 1 <= B <= %d (got %d)", MI355_BEAM_MAX, a.B);
    return MI355_ERR_UNSUPPORTED;
  }
  if (a.V > MI355_BEAM_MAX_V) {
    mi355_set_error("beam_step: V <= %d (got %d)", MI355_BEAM_MAX_V, a.V);
    return MI355_ERR_UNSUPPORTED;
  }
  MI355_REQUIRE(a.V > a.B && a.ld >= a.V, "beam_step: V must exceed B and the row stride must hold V (V %d, B %d, ld %lld)", a.V, a.B, (long long)a.ld);
  MI355_REQUIRE(a.eos_id >= 0 && a.eos_id < a.V, "beam_step: eos_id %d is outside [0, %d)", a.eos_id, a.V);
  MI355_REQUIRE(a.softmax_smoothing > 0.f, "beam_step: softmax_smoothing must be positive");
  MI355_REQUIRE((a.conf_in == nullptr) == (a.conf_out == nullptr), "beam_step: conf_in and conf_out must come together");
  MI355_REQUIRE((const void*)a.tokens_in != (const void*)a.tokens_out && (const void*)a.ind_in != (const void*)a.ind_out &&
                    (!a.conf_in || (const void*)a.conf_in != (const void*)a.conf_out),
                "beam_step: a history is read from one buffer and written to a second");
  MI355_CLEAR_ERROR();
  hipLaunchKernelGGL(beam_step_kernel, dim3((unsigned)a.N), dim3(256), 0, (hipStream_t)stream, a);
  MI355_LAUNCH_CHECK("beam_step");
  return MI355_OK;
}

extern "C" int mi355_beam_attention(const mi355_beam_attention_args* ap, void* stream) {
  MI355_REQUIRE(ap && ap->q && ap->k && ap->v && ap->ind && ap->pos && ap->out, "beam_attention: null tensor");
  const mi355_beam_attention_args a = *ap;
  if (a.dh != 64 && a.dh != 128) {
    mi355_set_error("beam_attention: dh must be 64 or 128 (got %d)", a.dh);
    return MI355_ERR_UNSUPPORTED;
  }
  if (a.B < 1 || a.B > MI355_BEAM_MAX) {
    mi355_set_error("beam_attention: 1 <= B <= %d (got %d)", MI355_BEAM_MAX, a.B);
    return MI355_ERR_UNSUPPORTED;
  }
  MI355_REQUIRE(a.N > 0 && (int64_t)a.N * a.B <= 65535 && a.heads > 0, "beam_attention: bad shape");
  MI355_REQUIRE(a.Tk >= 1 && a.Tk <= MI355_BEAM_ATTN_MAX_TK && a.Tk <= a.ld_ind, "beam_attention: 1 <= Tk <= min(%d, ld_ind) (got Tk %d, ld_ind %d)",
                MI355_BEAM_ATTN_MAX_TK, a.Tk, a.ld_ind);
  const int hd = a.heads * a.dh;
  MI355_REQUIRE(a.ldq >= hd && a.ldk >= hd && a.ldv >= hd && a.ldo >= hd, "beam_attention: a row stride is smaller than heads * dh");
  MI355_REQUIRE(a.k_sstride >= (int64_t)a.Tk * a.ldk && a.v_sstride >= (int64_t)a.Tk * a.ldv, "beam_attention: a slot stride is smaller than Tk rows");
  MI355_REQUIRE(a.ldq % 4 == 0 && a.ldk % 4 == 0 && a.ldv % 4 == 0 && a.ldo % 4 == 0 && a.k_sstride % 4 == 0 && a.v_sstride % 4 == 0 &&
                    ((uintptr_t)a.q | (uintptr_t)a.k | (uintptr_t)a.v | (uintptr_t)a.out) % 16 == 0,
                "beam_attention: rows must be 16-byte aligned");
  return a.dh == 64 ? launch_beam_attention<64>(a, (hipStream_t)stream) : launch_beam_attention<128>(a, (hipStream_t)stream);
}
