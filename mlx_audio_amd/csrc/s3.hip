// S3 speech tokenizer v2 (gfx950): the FSMN memory block and the FSQ head.
// Reference call sites: FSMNMultiHeadAttention.forward_fsmn (codec/models/s3/model_v2.py:152-172: a 31-tap depthwise conv over time on the
// value projection, masked before and after, plus the masked values), FSQCodebook.encode (:82-96: Linear(n_state, 8) -> tanh -> * 0.999 ->
// round half to even -> + 1 -> base-3 digits).  Both are plain float32 with a fixed summation order: no atomics, and nothing in the order
// depends on the launch geometry, so two calls on the same bytes give the same bits.
#include "dw_window.h"

namespace {

constexpr int kTaps = MI355_FSMN_MAX_TAPS;   // the register window is sized for the reference's 31 taps; shorter kernels are centred in it
constexpr int kHalf = (kTaps - 1) / 2;

// The register-window run of dw_window.h over the value projection, plus the values themselves and the residual stream.
__global__ __launch_bounds__(256) void fsmn_memory_kernel(const mi355_fsmn_memory_args a) {
  int c, t0, b;
  if (!dw_decode(a.C, a.L, c, t0, b)) return;
  const int len = dw_len(a.lens, b, a.L);
  const float* vb = a.v + (int64_t)b * a.v_bstride + c;
  float w[kTaps];
  const int shift = dw_tap_shift<kTaps>(a.K);
#pragma unroll
  for (int j = 0; j < kTaps; ++j) {
    const int k = j - shift;
    w[j] = (k >= 0 && k < a.K) ? a.w[(int64_t)c * a.K + k] : 0.f;
  }
  float win[kRun + kTaps - 1];
  const auto row = [vb, ldv = a.ldv](const int r) { return vb[(int64_t)r * ldv]; };
#pragma unroll
  for (int i = 0; i < kRun + kTaps - 1; ++i) win[i] = dw_window_row<kTaps>(i, t0, len, row);
  // the residual stream is requested WITH the window, before any store: y may be add, so behind a store the compiler must keep every later load of
  // add in program order -- one exposed memory round trip per time step
  const float* ab = a.add ? a.add + (int64_t)b * a.add_bstride + c : nullptr;
  float res[kRun];
#pragma unroll
  for (int i = 0; i < kRun; ++i) res[i] = (ab && t0 + i < a.L) ? ab[(int64_t)(t0 + i) * a.add_ld] : 0.f;
  float* yb = a.y + (int64_t)b * a.y_bstride + c;
#pragma unroll
  for (int i = 0; i < kRun; ++i) {
    const int t = t0 + i;
    if (t >= a.L) break;
    float s = dw_tap_sum<kTaps>(w, win, i, 0.f);
    s += win[i + kHalf];
    float o = res[i];
    if (t < len) o += s;
    yb[(int64_t)t * a.ldy] = o;
  }
}

// One wave per row, a lane holds its 4 * NCH channels of all eight weight rows in registers for every row the wave walks: x is read once (16 bytes per
// lane and chunk), w once per wave.  Per output: the lane's products in channel order (fma), then the fixed DPP wave sum, then + b.
template <int NCH>
__global__ __launch_bounds__(256) void fsq_encode_kernel(const mi355_fsq_encode_args a) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * 4;
  float4 w[8][NCH];
#pragma unroll
  for (int d = 0; d < 8; ++d)
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int c = i * 256 + lane * 4;
      w[d][i] = c < a.C ? *(const float4*)(a.w + (int64_t)d * a.C + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  float bias[8];
#pragma unroll
  for (int d = 0; d < 8; ++d) bias[d] = a.b ? a.b[d] : 0.f;
  for (int64_t row = wave; row < a.rows; row += nwaves) {   // wave-uniform: all 64 lanes stay active for the DPP sums
    bool valid = true;
    if (a.lens) {
      const int bi = (int)(row / a.L), t = (int)(row - (int64_t)bi * a.L);
      valid = t < a.lens[bi];
    }
    if (!valid) {   // wave-uniform
      if (lane == 0) a.codes[row] = 0;
      if (a.h && lane < 8) a.h[row * 8 + lane] = 0.f;
      continue;
    }
    const float* xr = a.x + row * a.ldx;
    float4 x[NCH];
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int c = i * 256 + lane * 4;
      x[i] = c < a.C ? *(const float4*)(xr + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    float h[8];
#pragma unroll
    for (int d = 0; d < 8; ++d) {
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < NCH; ++i) {
        s = fmaf(w[d][i].x, x[i].x, s); s = fmaf(w[d][i].y, x[i].y, s); s = fmaf(w[d][i].z, x[i].z, s); s = fmaf(w[d][i].w, x[i].w, s);
      }
      h[d] = wave_sum_fast(s) + bias[d];
    }
    int code = 0, p = 1;
#pragma unroll
    for (int d = 0; d < 8; ++d) {
      const float q = rintf(tanhf(h[d]) * 0.9990000128746033f);   // round half to even; -1, 0 or 1
      code += ((int)q + 1) * p;
      p *= 3;
    }
    if (lane == 0) a.codes[row] = code;
    if (a.h) {
      float hv = h[0];
#pragma unroll
      for (int d = 1; d < 8; ++d) hv = lane == d ? h[d] : hv;
      if (lane < 8) a.h[row * 8 + lane] = hv;
    }
  }
}

}  // namespace

extern "C" int mi355_fsmn_memory(const mi355_fsmn_memory_args* ap, void* stream) {
  MI355_REQUIRE(ap && ap->v && ap->w && ap->y, "fsmn_memory: null tensor");
  const mi355_fsmn_memory_args a = *ap;
  MI355_REQUIRE(a.B > 0 && a.B <= 65535 && a.C > 0 && a.L > 0, "fsmn_memory: bad shape");
  MI355_REQUIRE(a.K >= 1 && a.K <= kTaps && (a.K & 1) == 1, "fsmn_memory: K must be odd and <= %d (got %d)", kTaps, a.K);
  MI355_REQUIRE(a.ldv >= a.C && a.ldy >= a.C && (!a.add || a.add_ld >= a.C), "fsmn_memory: a row stride is smaller than C");
  MI355_REQUIRE((const void*)a.y != (const void*)a.v, "fsmn_memory: y must not alias v (a step reads its neighbours' values)");
  dim3 grid;
  if (const int rc = dw_grid("fsmn_memory", a.C, a.L, a.B, &grid)) return rc;
  MI355_CLEAR_ERROR();
  hipLaunchKernelGGL(fsmn_memory_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
  MI355_LAUNCH_CHECK("fsmn_memory");
  return MI355_OK;
}

extern "C" int mi355_fsq_encode(const mi355_fsq_encode_args* ap, void* stream) {
  MI355_REQUIRE(ap && ap->x && ap->w && ap->codes, "fsq_encode: null tensor");
  const mi355_fsq_encode_args a = *ap;
  MI355_REQUIRE(a.rows > 0 && a.C > 0 && a.C % 4 == 0 && a.C <= 1280, "fsq_encode: C must be a multiple of 4 and <= 1280 (got %d)", a.C);
  MI355_REQUIRE(a.ldx >= a.C && a.ldx % 4 == 0 && ((uintptr_t)a.x) % 16 == 0 && ((uintptr_t)a.w) % 16 == 0, "fsq_encode: x / w rows must be 16-byte aligned");
  MI355_REQUIRE(!a.lens || (a.L > 0 && a.rows % a.L == 0), "fsq_encode: with lens, rows must be B * L");
  const int64_t blocks = min((int64_t)1024, (a.rows + 31) / 32);   // >= 8 rows per wave once there are enough rows: the weights are fetched once per wave
  MI355_CLEAR_ERROR();
  if (a.C <= 256) hipLaunchKernelGGL(fsq_encode_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(fsq_encode_kernel<5>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
  MI355_LAUNCH_CHECK("fsq_encode");
  return MI355_OK;
}
