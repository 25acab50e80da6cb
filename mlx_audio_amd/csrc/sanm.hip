// SenseVoice-Small (gfx950): the encoder's input assembly and the CTC head behind the ctc_lo GEMM.
// Reference call sites: _apply_lfr / _apply_cmvn / SenseVoiceSmall.__call__'s two concatenations / SenseVoiceEncoder.__call__'s scale and
// SinusoidalPositionEncoder (stt/models/sensevoice/sensevoice.py:47-80,106-122,322-324,426-433), nn.log_softmax + mx.argmax (:437,451) and the
// collapse loop of _greedy_ctc_decode (:450-463).  All three are plain float32 with a fixed summation order: no atomics, and nothing in the order
// depends on the launch geometry, so two calls on the same bytes give the same bits.
#include "block_reduce.h"

namespace {

// One workgroup per (output row, item); the threads walk the m * D columns.  The float32 operations are the reference's, one rounding each
// (no contraction): (f + mean) * istd, then * scale, then + pe.
__global__ __launch_bounds__(256) void sanm_input_kernel(const mi355_sanm_input_args a, const int rows) {
  const int r = blockIdx.x, b = blockIdx.y;
  const int W = a.lfr_m * a.D;
  const int len = a.lens ? min(max(a.lens[b], 1), a.T) : a.T;   // lens[b] >= 1 is the caller's contract; the clamp keeps every index inside feats
  const int valid = 4 + (len + a.lfr_n - 1) / a.lfr_n;
  if (r == 0 && threadIdx.x == 0) a.out_lens[b] = valid;
  float* xr = a.x + (int64_t)b * a.x_bstride + (int64_t)r * a.ldx;
  if (r >= valid) {
    for (int c = threadIdx.x; c < W; c += 256) xr[c] = 0.f;
    return;
  }
  const float* per = a.pe ? a.pe + (int64_t)r * W : nullptr;
  if (r < 4) {
    const int q = min(max(a.qids[b * 4 + r], 0), 15);
    const float* e = a.embed + (int64_t)q * W;
    for (int c = threadIdx.x; c < W; c += 256) {
      const float v = __fmul_rn(e[c], a.scale);
      xr[c] = per ? __fadd_rn(v, per[c]) : v;
    }
    return;
  }
  const float* fb = a.feats + (int64_t)b * a.feats_bstride;
  const int first = (r - 4) * a.lfr_n - (a.lfr_m - 1) / 2;     // frame under column block 0: negative -> frame 0, beyond the item -> its last frame
  for (int c = threadIdx.x; c < W; c += 256) {
    const int j = c / a.D, d = c - j * a.D;
    const int f = min(max(first + j, 0), len - 1);
    float v = fb[(int64_t)f * a.ldf + d];
    if (a.means) v = __fmul_rn(__fadd_rn(v, a.means[c]), a.istd[c]);
    v = __fmul_rn(v, a.scale);
    xr[c] = per ? __fadd_rn(v, per[c]) : v;
  }
}

// One workgroup per row, thread t owns the columns t, t + 256, ... in ascending order.  Per thread: the running maximum with its first index, the
// largest value at any other index, and the online sum of exp(x - running maximum).  Then the shared joins: block_argmax (first maximum on ties),
// a maximum for the runner-up, and the sum of the threads' sums rescaled to the row maximum (xor butterfly per wave, (w0 + w1) + (w2 + w3)).
__global__ __launch_bounds__(256) void ctc_rows_kernel(const mi355_ctc_rows_args a) {
  __shared__ float redv[4];
  __shared__ int redi[4];
  const int64_t row = blockIdx.x;
  const float* xr = a.logits + row * a.ld;
  const int V = a.V;
  float m = -INFINITY, s = 0.f, second = -INFINITY;
  int mi = 0x7fffffff;
  for (int c = threadIdx.x; c < V; c += 256) {
    const float x = xr[c];
    if (mi == 0x7fffffff) {  // the thread's first column
      m = x;
      mi = c;
      s = 1.f;
    } else if (x > m) {      // a later equal value does not replace the first maximum; it is the runner-up
      s = s * expf(m - x) + 1.f;
      second = m;
      m = x;
      mi = c;
    } else {
      s += expf(x - m);
      second = fmaxf(second, x);
    }
  }
  ArgMax am;
  am.v = m;
  am.i = mi;
  const ArgMax top = block_argmax<4>(am, redv, redi);
  const float other = top.i == mi ? second : m;     // this thread's largest value at an index other than the arg-max
  const float runner = block_join_max<4>(wave_max(other), redv);
  const float part = mi == 0x7fffffff ? 0.f : s * expf(m - top.v);
  const float S = block_join_sum<4>(wave_sum(part), redv);
  const float logS = logf(S);
  if (threadIdx.x == 0) {
    a.ids[row] = top.i;
    a.gap[row] = V > 1 ? top.v - runner : 0.f;
    a.lp[row] = -logS;
  }
  if (a.logp) {   // the second pass over the row (just read: it comes from the caches); may be in place (logp == logits, ld_logp == ld)
    float* yr = a.logp + row * a.ld_logp;
    for (int c = threadIdx.x; c < V; c += 256) yr[c] = (xr[c] - top.v) - logS;
  }
}

// One wave per item walks its rows 64 at a time: a row is kept when it is no repeat of the row before it (row `skip` has none) and no blank; the
// kept rows of a chunk are placed by the ballot's prefix count.  The slots behind counts[b] are filled with -1.
__global__ __launch_bounds__(64) void ctc_collapse_kernel(const mi355_ctc_collapse_args a) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int len = a.lens ? min(max(a.lens[b], 0), a.T) : a.T;
  const int32_t* ids = a.ids + (int64_t)b * a.ld_ids;
  int32_t* tok = a.tokens + (int64_t)b * a.T;
  int32_t* frm = a.frames ? a.frames + (int64_t)b * a.T : nullptr;
  int base = 0;
  for (int t0 = a.skip; t0 < len; t0 += 64) {   // wave-uniform bounds
    const int t = t0 + lane;
    bool keep = false;
    int id = 0;
    if (t < len) {
      id = ids[t];
      keep = id != a.blank && (t == a.skip || ids[t - 1] != id);
    }
    const unsigned long long mask = __ballot(keep);
    if (keep) {
      const int pos = base + __popcll(mask & ((1ull << lane) - 1ull));
      tok[pos] = id;
      if (frm) frm[pos] = t;
    }
    base += __popcll(mask);
  }
  if (lane == 0) a.counts[b] = base;
  for (int p = base + lane; p < a.T; p += 64) {
    tok[p] = -1;
    if (frm) frm[p] = -1;
  }
}

}  // namespace

extern "C" int mi355_sanm_input(const mi355_sanm_input_args* ap, void* stream) {
  MI355_REQUIRE(ap && ap->feats && ap->embed && ap->qids && ap->x && ap->out_lens, "sanm_input: null tensor");
  const mi355_sanm_input_args a = *ap;
  MI355_REQUIRE(a.B > 0 && a.B <= 65535 && a.T > 0 && a.D > 0, "sanm_input: bad shape");
  MI355_REQUIRE(a.lfr_m >= 1 && a.lfr_n >= 1 && (int64_t)a.lfr_m * a.D <= (1 << 20), "sanm_input: bad lfr_m / lfr_n (got %d / %d)", a.lfr_m, a.lfr_n);
  MI355_REQUIRE((a.means == nullptr) == (a.istd == nullptr), "sanm_input: means and istd must come together");
  const int rows = 4 + (a.T + a.lfr_n - 1) / a.lfr_n;
  MI355_REQUIRE(a.ldf >= a.D && a.ldx >= a.lfr_m * a.D, "sanm_input: a row stride is smaller than its row");
  MI355_REQUIRE(!a.pe || a.pe_rows >= rows, "sanm_input: the position table holds %d rows, the batch needs %d", a.pe_rows, rows);
  MI355_CLEAR_ERROR();
  hipLaunchKernelGGL(sanm_input_kernel, dim3((unsigned)rows, (unsigned)a.B), dim3(256), 0, (hipStream_t)stream, a, rows);
  MI355_LAUNCH_CHECK("sanm_input");
  return MI355_OK;
}

extern "C" int mi355_ctc_rows(const mi355_ctc_rows_args* ap, void* stream) {
  MI355_REQUIRE(ap && ap->logits && ap->ids && ap->gap && ap->lp, "ctc_rows: null tensor");
  const mi355_ctc_rows_args a = *ap;
  MI355_REQUIRE(a.rows > 0 && a.rows <= 0x7fffffff && a.V >= 1, "ctc_rows: bad shape");
  MI355_REQUIRE(a.ld >= a.V && (!a.logp || a.ld_logp >= a.V), "ctc_rows: a row stride is smaller than V");
  MI355_REQUIRE(!a.logp || (const void*)a.logp != (const void*)a.logits || a.ld_logp == a.ld, "ctc_rows: in place needs ld_logp == ld");
  MI355_CLEAR_ERROR();
  hipLaunchKernelGGL(ctc_rows_kernel, dim3((unsigned)a.rows), dim3(256), 0, (hipStream_t)stream, a);
  MI355_LAUNCH_CHECK("ctc_rows");
  return MI355_OK;
}

extern "C" int mi355_ctc_collapse(const mi355_ctc_collapse_args* ap, void* stream) {
  MI355_REQUIRE(ap && ap->ids && ap->tokens && ap->counts, "ctc_collapse: null tensor");
  const mi355_ctc_collapse_args a = *ap;
  MI355_REQUIRE(a.B > 0 && a.T > 0 && a.ld_ids >= a.T && a.skip >= 0, "ctc_collapse: bad shape");
  MI355_CLEAR_ERROR();
  hipLaunchKernelGGL(ctc_collapse_kernel, dim3((unsigned)a.B), dim3(64), 0, (hipStream_t)stream, a);
  MI355_LAUNCH_CHECK("ctc_collapse");
  return MI355_OK;
}
