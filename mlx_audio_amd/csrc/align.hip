// Whisper word-level timestamps on the device (stt/models/whisper/timing.py:111-181 of the reference):
//   align_qk_softmax   cross-attention probabilities of the alignment heads (the flash kernels never materialise them)
//   align_matrix       standardise over tokens, median filter over frames (reflect padding), mean over heads, negate
//   dtw                the dynamic-time-warping path (timing.py:52-99), one workgroup per item walking the skewed wavefront
//   softmax_prob_rows  softmax(logits[r])[token[r]]; with one token for every row it is mi355_softmax_prob_at (the decode loop's no-speech probability)
// Every kernel takes B items with per-item lengths and touches nothing beyond them.
// A frame whose standard deviation over the tokens is 0 standardises to NaN; the median of a window that holds a NaN is NaN, as np.median's is.
#include "block_reduce.h"

namespace {

constexpr int kAT = 256;   // threads of the qk / matrix kernels
constexpr int kTT = 8;     // token rows a qk workgroup holds in LDS

// 8 consecutive key elements -> floats
template <int KV>
__device__ __forceinline__ void load_k8(const void* base, int64_t idx, float (&f)[8]) {
  if constexpr (KV == MI355_KV_F32) {
    const float4 a = *(const float4*)((const float*)base + idx);
    const float4 b = *(const float4*)((const float*)base + idx + 4);
    f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
  } else {
    const uint4 u = *(const uint4*)((const uint16_t*)base + idx);
    const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if constexpr (KV == MI355_KV_F16) {
        f[2 * i] = (float)__builtin_bit_cast(_Float16, (uint16_t)(w[i] & 0xffffu));
        f[2 * i + 1] = (float)__builtin_bit_cast(_Float16, (uint16_t)(w[i] >> 16));
      } else {
        f[2 * i] = __builtin_bit_cast(float, w[i] << 16);
        f[2 * i + 1] = __builtin_bit_cast(float, w[i] & 0xffff0000u);
      }
    }
  }
}

// One workgroup: kTT token rows of one (item, head).  Each thread owns the keys f = tid, tid + 256, ...: it reads a key once, takes its product with
// the kTT query rows held in LDS (broadcast reads), and parks the raw scores in w itself; the second and third sweeps re-read the thread's OWN
// stores (exp and sum, then the division), so no score crosses threads except through the two block reductions.
template <int KV, int DH>
__global__ __launch_bounds__(kAT) void align_qk_softmax_kernel(const mi355_align_qk_args a) {
  __shared__ __align__(16) float qs[kTT][DH];
  __shared__ float red[kTT][4];
  const int b = blockIdx.z, pair = blockIdx.y, t0 = blockIdx.x * kTT, tid = threadIdx.x;
  const int Tb = a.lens_t ? min(a.lens_t[b], a.T) : a.T;
  const int Fb = a.lens_f ? min(a.lens_f[b], a.F) : a.F;
  if (t0 >= Tb || Fb <= 0) return;
  const int head = a.pairs[2 * pair], slot = a.pairs[2 * pair + 1];
  const int nt = min(kTT, Tb - t0);
  for (int i = tid; i < kTT * DH; i += kAT) {
    const int r = i / DH, c = i - r * DH;
    qs[r][c] = r < nt ? a.q[(int64_t)b * a.q_bstride + (int64_t)(t0 + r) * a.ldq + head * DH + c] : 0.f;
  }
  __syncthreads();
  const int64_t kbase = (int64_t)b * a.k_bstride + (a.k_hstride ? (int64_t)head * a.k_hstride : (int64_t)head * DH);
  float* wrow = a.w + (int64_t)b * a.w_bstride + (int64_t)slot * a.w_astride + (int64_t)t0 * a.ldw;
  float mx[kTT];
#pragma unroll
  for (int r = 0; r < kTT; ++r) mx[r] = -INFINITY;
  for (int f = tid; f < Fb; f += kAT) {
    float acc[kTT][8];   // eight partial sums per row (one per element of a 16-byte key piece), joined pairwise: the error of a blocked host dot product
#pragma unroll
    for (int r = 0; r < kTT; ++r)
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[r][i] = 0.f;
    const int64_t kr = kbase + (int64_t)f * a.ldk;
#pragma unroll 2
    for (int c = 0; c < DH; c += 8) {
      float kf[8];
      load_k8<KV>(a.k, kr + c, kf);
#pragma unroll
      for (int r = 0; r < kTT; ++r) {
        const float4 q0 = *(const float4*)&qs[r][c];
        const float4 q1 = *(const float4*)&qs[r][c + 4];
        acc[r][0] = fmaf(q0.x, kf[0], acc[r][0]); acc[r][1] = fmaf(q0.y, kf[1], acc[r][1]);
        acc[r][2] = fmaf(q0.z, kf[2], acc[r][2]); acc[r][3] = fmaf(q0.w, kf[3], acc[r][3]);
        acc[r][4] = fmaf(q1.x, kf[4], acc[r][4]); acc[r][5] = fmaf(q1.y, kf[5], acc[r][5]);
        acc[r][6] = fmaf(q1.z, kf[6], acc[r][6]); acc[r][7] = fmaf(q1.w, kf[7], acc[r][7]);
      }
    }
#pragma unroll
    for (int r = 0; r < kTT; ++r) {
      if (r < nt) {
        const float d = ((acc[r][0] + acc[r][1]) + (acc[r][2] + acc[r][3])) + ((acc[r][4] + acc[r][5]) + (acc[r][6] + acc[r][7]));
        const float s = (d * a.scale) * a.qk_scale;
        wrow[(int64_t)r * a.ldw + f] = s;
        mx[r] = fmaxf(mx[r], s);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < kTT; ++r) mx[r] = block_join_max<4>(wave_max(mx[r]), red[r]);
  float sum[kTT];
#pragma unroll
  for (int r = 0; r < kTT; ++r) sum[r] = 0.f;
  for (int f = tid; f < Fb; f += kAT) {
#pragma unroll
    for (int r = 0; r < kTT; ++r) {
      if (r < nt) {
        const float e = expf(wrow[(int64_t)r * a.ldw + f] - mx[r]);
        wrow[(int64_t)r * a.ldw + f] = e;
        sum[r] += e;
      }
    }
  }
  __syncthreads();   // red is reused
#pragma unroll
  for (int r = 0; r < kTT; ++r) sum[r] = block_join_sum<4>(wave_sum(sum[r]), red[r]);
  for (int f = tid; f < Fb; f += kAT) {
#pragma unroll
    for (int r = 0; r < kTT; ++r)
      if (r < nt) wrow[(int64_t)r * a.ldw + f] = wrow[(int64_t)r * a.ldw + f] / sum[r];
  }
}

// mean and population standard deviation over the tokens, one thread per (item, head, frame); a frame's loads coalesce across the wave
__global__ __launch_bounds__(kAT) void align_stats_kernel(const mi355_align_matrix_args a) {
  const int b = blockIdx.z, h = blockIdx.y, f = blockIdx.x * kAT + threadIdx.x;
  const int Tb = a.lens_t ? min(a.lens_t[b], a.T) : a.T;
  const int Fb = a.lens_f ? min(a.lens_f[b], a.F) : a.F;
  if (f >= Fb || Tb <= 0) return;
  const float* w = a.w + (int64_t)b * a.w_bstride + (int64_t)h * a.w_astride + f;
  float s = 0.f;
  for (int t = 0; t < Tb; ++t) s += w[(int64_t)t * a.ldw];
  const float mean = s / (float)Tb;
  float v = 0.f;
  for (int t = 0; t < Tb; ++t) {
    const float d = w[(int64_t)t * a.ldw] - mean;
    v = fmaf(d, d, v);
  }
  float* st = a.stats + (((int64_t)b * a.A + h) * a.F + f) * 2;
  st[0] = mean;
  st[1] = sqrtf(v / (float)Tb);
}

// One thread per (item, kept token row, frame): for each head the (standardised) window of medfilt_width frames around f with reflect padding, its
// median by rank selection in registers, then the mean over the heads.
template <int W>
__global__ __launch_bounds__(kAT) void align_matrix_kernel(const mi355_align_matrix_args a) {
  const int b = blockIdx.z, n = blockIdx.y, f = blockIdx.x * kAT + threadIdx.x;
  const int Tb = a.lens_t ? min(a.lens_t[b], a.T) : a.T;
  const int Fb = a.lens_f ? min(a.lens_f[b], a.F) : a.F;
  const int t = a.row_begin + n;
  if (f >= Fb || t >= Tb - a.row_trim) return;
  const int width = W ? W : a.medfilt_width;
  const int pad = width / 2;
  const bool filt = Fb > pad;   // timing.py:19-21: rows no longer than the padding pass unfiltered
  float acc = 0.f;
  for (int h = 0; h < a.A; ++h) {
    const float* w = a.w + (int64_t)b * a.w_bstride + (int64_t)h * a.w_astride + (int64_t)t * a.ldw;
    const float* st = a.stats + (((int64_t)b * a.A + h) * a.F) * 2;
    float win[W ? W : 15];
    const int cnt = filt ? width : 1;
#pragma unroll
    for (int i = 0; i < (W ? W : 15); ++i) {
      if (i < cnt) {
        int g = filt ? f - pad + i : f;
        g = g < 0 ? -g : (g >= Fb ? 2 * (Fb - 1) - g : g);
        float v = w[g];
        if (a.standardize) v = (v - st[2 * g]) / st[2 * g + 1];
        win[i] = v;
      }
    }
    float med = win[0];
    bool has_nan = false;   // np.median gives NaN for a window that holds one (a frame whose standard deviation over the tokens is 0)
    if (filt) {   // selection by rank (ties broken by position): the element with exactly `pad` others before it in sorted order
#pragma unroll
      for (int i = 0; i < (W ? W : 15); ++i) {
        if (i < cnt) {
          int rank = 0;
#pragma unroll
          for (int j = 0; j < (W ? W : 15); ++j)
            if (j < cnt) rank += (win[j] < win[i] || (win[j] == win[i] && j < i)) ? 1 : 0;
          if (rank == pad) med = win[i];
          has_nan |= win[i] != win[i];
        }
      }
    }
    acc += has_nan ? __builtin_nanf("") : med;
  }
  const float m = acc / (float)a.A;
  a.out[(int64_t)b * a.out_bstride + (int64_t)n * a.ldo + f] = a.negate ? -m : m;
}

// timing.py:76-99.  Thread i owns token row i + 1 of the (N + 1) x (M + 1) table; step s holds the cells with (i - 1) + (j - 1) = s.  A cell needs the
// row above at steps s - 1 (c1) and s - 2 (c0) and its own row at step s - 1 (c2): three rotating LDS rows, one barrier per step.  The trace goes to the
// workspace in [step][row] order (a step's stores are consecutive bytes); lane 0 walks it back and the workgroup copies the path out in forward order.
__global__ __launch_bounds__(1024) void dtw_kernel(const mi355_dtw_args a, int64_t ws_item) {
#pragma clang fp contract(off)
  __shared__ float ring[3][1024];
  __shared__ int plen;
  const int b = blockIdx.x, tid = threadIdx.x, nthr = blockDim.x;
  const int n = a.lens_n ? min(a.lens_n[b], a.N) : a.N;
  const int m = a.lens_m ? min(a.lens_m[b], a.M) : a.M;
  if (n <= 0 || m <= 0) {
    if (tid == 0) a.path_len[b] = 0;
    return;
  }
  uint8_t* trace = (uint8_t*)a.ws + (int64_t)b * ws_item;
  int32_t* rev = (int32_t*)(trace + (((int64_t)(a.N + a.M) * a.N + 15) & ~(int64_t)15));   // the path, backwards: 2 * (N + M) int32
  const float* x = a.cost + (int64_t)b * a.cost_bstride + (int64_t)tid * a.ldc;
  ring[0][tid] = ring[1][tid] = ring[2][tid] = INFINITY;
  __syncthreads();
  float own = INFINITY;   // cost[i][j - 1]; column 0 is inf
  const int steps = n + m - 1;
  for (int s = 0; s < steps; ++s) {
    const int j = s - tid;   // 0-based frame of this row's cell at step s
    const bool act = tid < n && j >= 0 && j < m;
    float cur = INFINITY;
    if (act) {
      float c0, c1;
      if (tid == 0) {
        c0 = j == 0 ? 0.f : INFINITY;   // cost[0][0] = 0, the rest of row 0 is inf
        c1 = INFINITY;
      } else {
        c1 = ring[(s + 2) % 3][tid - 1];   // step s - 1
        c0 = ring[(s + 1) % 3][tid - 1];   // step s - 2
      }
      const float c2 = own;
      float c;
      uint8_t tr;
      if (c0 < c1 && c0 < c2) { c = c0; tr = 0; }
      else if (c1 < c0 && c1 < c2) { c = c1; tr = 1; }
      else { c = c2; tr = 2; }
      cur = x[j] + c;
      own = cur;
      trace[(int64_t)s * a.N + tid] = tr;
    }
    ring[s % 3][tid] = cur;
    __syncthreads();
  }
  __threadfence_block();
  __syncthreads();
  if (tid == 0) {
    int i = n, j = m, L = 0;
    while (i > 0 || j > 0) {
      rev[2 * L] = i - 1;
      rev[2 * L + 1] = j - 1;
      ++L;
      const int tr = i == 0 ? 2 : (j == 0 ? 1 : trace[(int64_t)(i + j - 2) * a.N + (i - 1)]);   // trace[0, :] = 2, trace[:, 0] = 1
      if (tr == 0) { --i; --j; }
      else if (tr == 1) --i;
      else --j;
    }
    plen = L;
    a.path_len[b] = L;
  }
  __syncthreads();
  const int L = plen;
  for (int p = tid; p < L; p += nthr) {
    a.text_idx[(int64_t)b * a.path_cap + p] = rev[2 * (L - 1 - p)];
    a.time_idx[(int64_t)b * a.path_cap + p] = rev[2 * (L - 1 - p) + 1];
  }
}

// out[r] = softmax(logits[r])[token of row r]: tokens[r], or the scalar `token` for every row when tokens is null
__global__ __launch_bounds__(1024) void softmax_prob_rows_kernel(const float* logits, int64_t ld, int V, const int32_t* tokens, int token, float* out) {
  __shared__ float red[16];
  const int r = blockIdx.x, tid = threadIdx.x;
  const float* lg = logits + (int64_t)r * ld;
  const int tk = tokens ? tokens[r] : token;
  float mx = -INFINITY;
  for (int v = tid; v < V; v += 1024) mx = fmaxf(mx, lg[v]);
  mx = block_join_max<16>(wave_max(mx), red);
  float s = 0.f;
  for (int v = tid; v < V; v += 1024) s += expf(lg[v] - mx);
  s = block_join_sum<16>(wave_sum(s), red);
  if (tid == 0) out[r] = (tk >= 0 && tk < V) ? expf(lg[tk] - mx) / s : 0.f;
}

template <int KV>
void launch_qk(const mi355_align_qk_args& a, dim3 grid, hipStream_t st) {
  if (a.dh == 64) hipLaunchKernelGGL((align_qk_softmax_kernel<KV, 64>), grid, dim3(kAT), 0, st, a);
  else hipLaunchKernelGGL((align_qk_softmax_kernel<KV, 128>), grid, dim3(kAT), 0, st, a);
}

int64_t dtw_item_bytes(int64_t N, int64_t M) {
  return (((N + M) * N + 15) & ~(int64_t)15) + 2 * (N + M) * (int64_t)sizeof(int32_t);
}

}  // namespace

extern "C" int mi355_align_qk_softmax(const mi355_align_qk_args* ap, void* stream) {
  MI355_REQUIRE(ap && ap->q && ap->k && ap->w && ap->pairs, "align_qk_softmax: null tensor");
  const mi355_align_qk_args a = *ap;
  MI355_REQUIRE(a.dh == 64 || a.dh == 128, "align_qk_softmax: dh must be 64 or 128 (got %d)", (int)a.dh);
  MI355_REQUIRE(a.kv_dtype == MI355_KV_F32 || a.kv_dtype == MI355_KV_BF16 || a.kv_dtype == MI355_KV_F16, "align_qk_softmax: bad kv_dtype");
  MI355_REQUIRE(a.B > 0 && a.T > 0 && a.F > 0 && a.n_pairs > 0 && a.n_pairs <= a.A && a.n_pairs <= 65535 && a.B <= 65535, "align_qk_softmax: bad shape");
  MI355_REQUIRE(a.ldw >= a.F && a.heads > 0 && a.ldq >= a.heads * a.dh, "align_qk_softmax: bad strides");
  // 16-byte key loads: every key row starts on a multiple of 8 (16-bit) / 4 (float32) elements
  const int64_t al = a.kv_dtype == MI355_KV_F32 ? 4 : 8;
  MI355_REQUIRE(a.ldk % al == 0 && a.k_bstride % al == 0 && a.k_hstride % al == 0 && ((uintptr_t)a.k & 15) == 0, "align_qk_softmax: k rows must be 16-byte aligned");
  MI355_CLEAR_ERROR();
  const dim3 grid((a.T + kTT - 1) / kTT, a.n_pairs, a.B);
  if (a.kv_dtype == MI355_KV_F32) launch_qk<MI355_KV_F32>(a, grid, (hipStream_t)stream);
  else if (a.kv_dtype == MI355_KV_BF16) launch_qk<MI355_KV_BF16>(a, grid, (hipStream_t)stream);
  else launch_qk<MI355_KV_F16>(a, grid, (hipStream_t)stream);
  MI355_LAUNCH_CHECK("align_qk_softmax");
  return MI355_OK;
}

extern "C" int mi355_align_matrix(const mi355_align_matrix_args* ap, void* stream) {
  MI355_REQUIRE(ap && ap->w && ap->out && (ap->stats || !ap->standardize), "align_matrix: null tensor");
  const mi355_align_matrix_args a = *ap;
  MI355_REQUIRE(a.medfilt_width >= 1 && a.medfilt_width <= 15 && (a.medfilt_width & 1), "align_matrix: medfilt_width must be odd and <= 15 (got %d)", (int)a.medfilt_width);
  MI355_REQUIRE(a.B > 0 && a.B <= 65535 && a.A > 0 && a.A <= 65535 && a.T > 0 && a.F > 0 && a.row_begin >= 0 && a.row_trim >= 0, "align_matrix: bad shape");
  MI355_REQUIRE(a.ldw >= a.F && a.ldo >= a.F, "align_matrix: bad strides");
  const int rows = a.T - a.row_trim - a.row_begin;
  MI355_CLEAR_ERROR();
  if (rows <= 0) return MI355_OK;
  MI355_REQUIRE(rows <= 65535, "align_matrix: more than 65535 rows");
  const int fb = (a.F + kAT - 1) / kAT;
  if (a.standardize) hipLaunchKernelGGL(align_stats_kernel, dim3(fb, a.A, a.B), dim3(kAT), 0, (hipStream_t)stream, a);
  if (a.medfilt_width == 7) hipLaunchKernelGGL(align_matrix_kernel<7>, dim3(fb, rows, a.B), dim3(kAT), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(align_matrix_kernel<0>, dim3(fb, rows, a.B), dim3(kAT), 0, (hipStream_t)stream, a);
  MI355_LAUNCH_CHECK("align_matrix");
  return MI355_OK;
}

extern "C" int64_t mi355_dtw_ws_bytes(int32_t N, int32_t M, int32_t B) {
  if (N <= 0 || M <= 0 || B <= 0) return 0;
  return dtw_item_bytes(N, M) * B;
}

extern "C" int mi355_dtw(const mi355_dtw_args* ap, void* stream) {
  MI355_REQUIRE(ap && ap->cost && ap->text_idx && ap->time_idx && ap->path_len && ap->ws, "dtw: null tensor");
  const mi355_dtw_args a = *ap;
  MI355_REQUIRE(a.B > 0 && a.N > 0 && a.M > 0 && a.ldc >= a.M, "dtw: bad shape");
  MI355_REQUIRE(a.N <= 1024, "dtw: N = %d token rows, at most 1024 (one thread per row)", (int)a.N);
  MI355_REQUIRE(a.path_cap >= a.N + a.M, "dtw: path capacity below N + M");
  MI355_REQUIRE(a.ws_bytes >= mi355_dtw_ws_bytes(a.N, a.M, a.B) && ((uintptr_t)a.ws & 15) == 0, "dtw: workspace too small or misaligned");
  MI355_CLEAR_ERROR();
  const int threads = ((a.N + 63) / 64) * 64;
  hipLaunchKernelGGL(dtw_kernel, dim3(a.B), dim3(threads), 0, (hipStream_t)stream, a, dtw_item_bytes(a.N, a.M));
  MI355_LAUNCH_CHECK("dtw");
  return MI355_OK;
}

extern "C" int mi355_softmax_prob_rows(const float* logits, int64_t ld, int32_t V, int32_t R, const int32_t* tokens, float* out, void* stream) {
  MI355_REQUIRE(logits && tokens && out, "softmax_prob_rows: null tensor");
  MI355_REQUIRE(R > 0 && V > 0 && ld >= V, "softmax_prob_rows: bad shape");
  MI355_CLEAR_ERROR();
  hipLaunchKernelGGL(softmax_prob_rows_kernel, dim3(R), dim3(1024), 0, (hipStream_t)stream, logits, ld, (int)V, tokens, 0, out);
  MI355_LAUNCH_CHECK("softmax_prob_rows");
  return MI355_OK;
}

extern "C" int mi355_softmax_prob_at(const float* logits, int32_t ld, int32_t V, int32_t B, int32_t token, float* out, void* stream) {
  MI355_REQUIRE(logits && out && B > 0 && V > 0 && token >= 0 && token < V, "softmax_prob_at: bad arguments");
  MI355_CLEAR_ERROR();
  hipLaunchKernelGGL(softmax_prob_rows_kernel, dim3(B), dim3(1024), 0, (hipStream_t)stream, logits, (int64_t)ld, (int)V, (const int32_t*)nullptr, (int)token, out);
  MI355_LAUNCH_CHECK("softmax_prob_at");
  return MI355_OK;
}
