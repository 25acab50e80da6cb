// DeepFilterNet2 / 3 around its GRUs (sts/models/deepfilternet; gfx950): the feature front end, the fused conv block, the mask + deep-filter back end.
// Built with -ffp-contract=off: the two running normalisations are written as the reference writes them in float32
// (state = x * (1 - alpha) + state * alpha: two products, one sum) and must not be contracted into FMAs.
//
//   dfn_band_db_kernel   one workgroup per (frame, item): scales the spectrum, leaves |.|^2 in LDS and the ERB bands' dB values in feat_erb;
//   dfn_norm_kernel      the two running normalisations (first-order recurrences over the frames) and the look-ahead shift: one thread per band / bin,
//                        sequential over the item's frames with eight frames loaded ahead of the dependent chain.
//   dfn_conv2d_kernel    a workgroup holds 256 / max(Cmid, Cout) output positions x the channels: thread (p, c) computes channel c of the
//                        (dense / grouped / depthwise, strided or frequency-transposed) conv at position p, the Cmid values of a position meet in
//                        LDS for the pointwise conv, and the folded BatchNorm, the activation and the skip tensor are the epilogue:
//                        x is read once (through L1 / L2 for the taps) and y written once, nothing in between goes to memory.
//   dfn_apply_kernel     one thread per (item, frame, bin).
#include "common.h"

namespace {

__device__ __forceinline__ int dfn_len(const int32_t* lens, int b, int T) {
  const int n = lens ? lens[b] : T;
  return n < 0 ? 0 : (n > T ? T : n);
}

// numpy.linspace(start, stop, num, dtype=float32): float64 arithmetic, the last point is `stop` itself
__device__ __forceinline__ float dfn_linspace(double start, double stop, int num, int i) {
  if (num <= 1) return (float)start;
  if (i == num - 1) return (float)stop;
  return (float)((double)i * ((stop - start) / (double)(num - 1)) + start);
}

// pass 1, one workgroup per (frame, item): spec_out = spec * wnorm, and the band's dB value 10 log10(energy + 1e-10) left in feat_erb[b, t, e] for pass 2.
// Thread (part, e) sums every NP-th bin of band e (all F bins against the filterbank column, or the band's own bins), the NP partial sums meet in
// LDS and are added in part order: a fixed sum whatever the launch.
__global__ __launch_bounds__(256) void dfn_band_db_kernel(const mi355_dfn_features_args a, const int NP) {
  extern __shared__ float sm[];
  float* mag2 = sm;            // [F]
  float* part = sm + a.F;      // [NP][E]
  const int tid = threadIdx.x, t = blockIdx.x, b = blockIdx.y;
  const int n = dfn_len(a.lens, b, a.T);
  const float* sp = a.spec + (int64_t)b * a.spec_bstride + (int64_t)t * a.F * 2;
  float* so = a.spec_out + (int64_t)b * a.spec_out_bstride + (int64_t)t * a.F * 2;
  if (t >= n) {   // padding: zeros
    for (int i = tid; i < 2 * a.F; i += 256) so[i] = 0.f;
    return;
  }
  for (int f = tid; f < a.F; f += 256) {
    const float re = sp[2 * f] * a.wnorm, im = sp[2 * f + 1] * a.wnorm;
    so[2 * f] = re;
    so[2 * f + 1] = im;
    mag2[f] = re * re + im * im;
  }
  __syncthreads();
  const int e = tid % a.E, pt = tid / a.E;
  int f0 = 0, f1 = a.F;
  if (!a.erb_fb) {   // clamped: nothing outside the frame is read whatever the table holds; an empty band has energy 0
    f0 = a.erb_start[e] < 0 ? 0 : a.erb_start[e];
    f1 = a.erb_start[e + 1] > a.F ? a.F : a.erb_start[e + 1];
  }
  if (pt < NP) {
    float s = 0.f;
    if (a.erb_fb) {
      for (int f = f0 + pt; f < f1; f += NP) s += mag2[f] * a.erb_fb[(int64_t)f * a.E + e];
    } else {
      for (int f = f0 + pt; f < f1; f += NP) s += mag2[f];
    }
    part[pt * a.E + e] = s;
  }
  __syncthreads();
  if (tid < a.E) {
    float en = 0.f;
    for (int q = 0; q < NP; ++q) en += part[q * a.E + tid];
    if (!a.erb_fb) en = f1 > f0 ? en / (float)(f1 - f0) : 0.f;
    a.feat_erb[((int64_t)b * a.T + t) * a.E + tid] = 10.0f * log10f(en + 1e-10f);
  }
}

// pass 2, the two running normalisations: workgroup (item, 0) walks the dB values of its E bands, workgroup (item, 1) the D bins of spec_out, one
// thread per band / bin, sequential over the frames in the reference's float32 order, eight frames loaded ahead of the dependent chain.  feat_erb
// is rewritten in place: the value of frame t goes to row t - la <= t, and a chunk's rows are all read before any of them is written.
__global__ __launch_bounds__(256) void dfn_norm_kernel(const mi355_dfn_features_args a) {
  constexpr int CH = 8;
  const int tid = threadIdx.x, b = blockIdx.x, which = blockIdx.y;
  const int n = dfn_len(a.lens, b, a.T);
  const int la = n > a.lookahead ? a.lookahead : 0;   // DfNet._apply_lookahead leaves a clip of at most `lookahead` frames unshifted
  if (which == 0) {
    if (tid >= a.E) return;
    float* fe = a.feat_erb + (int64_t)b * a.T * a.E + tid;
    float st = dfn_linspace(-60.0, -90.0, a.E, tid);
    for (int t0 = 0; t0 < n; t0 += CH) {
      float x[CH];
#pragma unroll
      for (int i = 0; i < CH; ++i) x[i] = t0 + i < n ? fe[(int64_t)(t0 + i) * a.E] : 0.f;
#pragma unroll
      for (int i = 0; i < CH; ++i) {
        if (t0 + i < n) {
          st = x[i] * a.one_minus_alpha + st * a.alpha;
          if (t0 + i - la >= 0) fe[(int64_t)(t0 + i - la) * a.E] = (x[i] - st) / 40.0f;
        }
      }
    }
    for (int t = n - la; t < a.T; ++t) fe[(int64_t)t * a.E] = 0.f;   // the frames the shift leaves empty and the padding
  } else {
    if (tid >= a.D) return;
    const float* so = a.spec_out + (int64_t)b * a.spec_out_bstride + 2 * tid;
    float* fd = a.feat_df + ((int64_t)b * a.T * a.D + tid) * 2;
    float st = dfn_linspace(0.001, 0.0001, a.D, tid);
    for (int t0 = 0; t0 < n; t0 += CH) {
      float re[CH], im[CH];
#pragma unroll
      for (int i = 0; i < CH; ++i) {
        re[i] = t0 + i < n ? so[(int64_t)(t0 + i) * a.F * 2] : 0.f;
        im[i] = t0 + i < n ? so[(int64_t)(t0 + i) * a.F * 2 + 1] : 0.f;
      }
#pragma unroll
      for (int i = 0; i < CH; ++i) {
        if (t0 + i < n) {
          const float mag = sqrtf(re[i] * re[i] + im[i] * im[i]);
          st = mag * a.one_minus_alpha + st * a.alpha;
          const float den = sqrtf(st);
          if (t0 + i - la >= 0) {
            fd[(int64_t)(t0 + i - la) * a.D * 2] = re[i] / den;
            fd[(int64_t)(t0 + i - la) * a.D * 2 + 1] = im[i] / den;
          }
        }
      }
    }
    for (int t = n - la; t < a.T; ++t) { fd[(int64_t)t * a.D * 2] = 0.f; fd[(int64_t)t * a.D * 2 + 1] = 0.f; }
  }
}

__global__ __launch_bounds__(256) void dfn_conv2d_kernel(const mi355_dfn_conv2d_args a, const int Fo, const int CM, const int P) {
  __shared__ float mid[256];
  const int tid = threadIdx.x, b = blockIdx.y;
  const int p = tid / CM, c = tid - p * CM;
  const int64_t pos = (int64_t)blockIdx.x * P + p;
  const bool valid = p < P && pos < (int64_t)a.T * Fo;
  const int t = valid ? (int)(pos / Fo) : 0, fo = valid ? (int)(pos - (int64_t)t * Fo) : 0;
  const int n = dfn_len(a.lens, b, a.T);
  const float* x = a.x + (int64_t)b * a.x_bstride;
  const int cin_g = a.Cin / a.groups, cm_g = a.Cmid / a.groups, ktf = a.kt * a.kf;
  float acc = 0.f;
  if (valid && c < a.Cmid && t < n) {
    const int g = c / cm_g;
    for (int dt = 0; dt < a.kt; ++dt) {
      const int ti = a.transposed ? t + a.kt - 1 - dt : t + dt - (a.kt - 1 - a.lookahead);
      if (ti < 0 || ti >= n) continue;
      for (int df = 0; df < a.kf; ++df) {
        int fi;
        if (a.transposed) {
          const int num = fo + a.kf / 2 - df;
          if (num < 0 || num % a.fstride) continue;
          fi = num / a.fstride;
        } else {
          fi = fo * a.fstride + df - a.kf / 2;
        }
        if (fi < 0 || fi >= a.F) continue;
        const float* xr = x + ((int64_t)ti * a.F + fi) * a.Cin + g * cin_g;
        if (a.transposed) {
          const float* wr = a.w + ((int64_t)(g * cin_g) * cm_g + (c - g * cm_g)) * ktf + dt * a.kf + df;
          for (int ci = 0; ci < cin_g; ++ci) acc += xr[ci] * wr[(int64_t)ci * cm_g * ktf];
        } else {
          const float* wr = a.w + (int64_t)c * cin_g * ktf + dt * a.kf + df;
          for (int ci = 0; ci < cin_g; ++ci) acc += xr[ci] * wr[ci * ktf];
        }
      }
    }
  }
  if (a.pw) {
    if (p < P && c < a.Cmid) mid[p * a.Cmid + c] = acc;
    __syncthreads();
  }
  if (!valid || c >= a.Cout) return;
  float v = acc;
  if (a.pw) {
    v = 0.f;
    const float* pr = a.pw + (int64_t)c * a.Cmid;
    const float* mr = mid + p * a.Cmid;
    for (int cm = 0; cm < a.Cmid; ++cm) v += pr[cm] * mr[cm];
  }
  if (a.scale) v = v * a.scale[c];
  if (a.shift) v = v + a.shift[c];
  if (a.act == 1) v = v > 0.f ? v : 0.f;
  else if (a.act == 2) v = 1.0f / (1.0f + expf(-v));
  const int64_t o = ((int64_t)t * Fo + fo) * a.Cout + c;
  if (a.add) v += a.add[(int64_t)b * a.add_bstride + o];
  a.y[(int64_t)b * a.y_bstride + o] = t < n ? v : 0.f;
}

__global__ __launch_bounds__(256) void dfn_apply_kernel(const mi355_dfn_apply_args a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int b = blockIdx.y;
  if (i >= (int64_t)a.T * a.F) return;
  const int t = (int)(i / a.F), f = (int)(i - (int64_t)t * a.F);
  const int n = dfn_len(a.lens, b, a.T);
  const float* sp = a.spec + (int64_t)b * a.spec_bstride;
  float* o = a.out + (int64_t)b * a.out_bstride + i * 2;
  if (t >= n) { o[0] = 0.f; o[1] = 0.f; return; }
  auto gain = [&](const int tt) {
    const float* m = a.m + ((int64_t)b * a.T + tt) * a.E;
    float g = 0.f;
    for (int e = 0; e < a.E; ++e) g += m[e] * a.erb_inv_fb[(int64_t)e * a.F + f];
    return g;
  };
  float re, im;
  if (f >= a.D) {
    const float g = gain(t);
    re = sp[i * 2] * g;
    im = sp[i * 2 + 1] * g;
  } else {
    re = 0.f;
    im = 0.f;
    const float* cf = a.coef + (((int64_t)b * a.T + t) * a.D + f) * a.order * 2;
    for (int k = 0; k < a.order; ++k) {
      const int tt = t + k - (a.order - 1 - a.df_lookahead);
      if (tt < 0 || tt >= n) continue;
      float sr = sp[((int64_t)tt * a.F + f) * 2], si = sp[((int64_t)tt * a.F + f) * 2 + 1];
      if (a.mask_first) {
        const float g = gain(tt);
        sr = sr * g;
        si = si * g;
      }
      const float cr = cf[2 * k], ci = cf[2 * k + 1];
      re = re + (sr * cr - si * ci);
      im = im + (sr * ci + si * cr);
    }
  }
  o[0] = re / a.wnorm;
  o[1] = im / a.wnorm;
}

}  // namespace

extern "C" int mi355_dfn_features(const mi355_dfn_features_args* ap, void* stream) {
  MI355_REQUIRE(ap && ap->spec && ap->spec_out && ap->feat_erb && ap->feat_df, "dfn_features: null tensor");
  const mi355_dfn_features_args a = *ap;
  MI355_REQUIRE((a.erb_fb != nullptr) != (a.erb_start != nullptr), "dfn_features: exactly one of erb_fb and erb_start must be given");
  MI355_REQUIRE(a.B >= 1 && a.T >= 1 && a.F >= 1 && a.E >= 1 && a.D >= 1 && a.D <= a.F && a.E <= MI355_DFN_MAX_BANDS && a.D <= MI355_DFN_MAX_BANDS &&
                    a.F <= 8192 && a.lookahead >= 0,
                "dfn_features: bad shape (B %d, T %d, F %d, E %d, D %d, lookahead %d)", a.B, a.T, a.F, a.E, a.D, a.lookahead);
  MI355_REQUIRE(a.spec_bstride >= (int64_t)a.T * a.F * 2 && a.spec_out_bstride >= (int64_t)a.T * a.F * 2, "dfn_features: bad strides");
  MI355_REQUIRE(a.B <= 65535, "dfn_features: at most 65535 items");
  const int NP = 256 / a.E;   // E <= 256: at least one thread per band
  MI355_CLEAR_ERROR();
  hipLaunchKernelGGL(dfn_band_db_kernel, dim3(a.T, a.B), dim3(256), sizeof(float) * (size_t)(a.F + NP * a.E), (hipStream_t)stream, a, NP);
  MI355_LAUNCH_CHECK("dfn_features(band dB)");
  hipLaunchKernelGGL(dfn_norm_kernel, dim3(a.B, 2), dim3(256), 0, (hipStream_t)stream, a);
  MI355_LAUNCH_CHECK("dfn_features");
  return MI355_OK;
}

extern "C" int32_t mi355_dfn_conv2d_fo(int32_t F, int32_t kf, int32_t fstride, int32_t transposed) {
  if (F < 1 || (kf != 1 && kf != 3) || (fstride != 1 && fstride != 2)) return -1;
  return transposed ? (F - 1) * fstride + kf - kf / 2 : (F + 2 * (kf / 2) - kf) / fstride + 1;
}

extern "C" int mi355_dfn_conv2d(const mi355_dfn_conv2d_args* ap, void* stream) {
  MI355_REQUIRE(ap && ap->x && ap->w && ap->y, "dfn_conv2d: null tensor");
  const mi355_dfn_conv2d_args a = *ap;
  MI355_REQUIRE(a.B >= 1 && a.B <= 65535 && a.T >= 1 && a.F >= 1 && a.Cin >= 1 && a.Cmid >= 1 && a.Cout >= 1 && a.Cin <= MI355_DFN_MAX_CH &&
                    a.Cmid <= MI355_DFN_MAX_CH && a.Cout <= MI355_DFN_MAX_CH,
                "dfn_conv2d: bad shape (B %d, T %d, F %d, channels %d -> %d -> %d; at most %d)", a.B, a.T, a.F, a.Cin, a.Cmid, a.Cout, MI355_DFN_MAX_CH);
  MI355_REQUIRE(a.groups >= 1 && a.Cin % a.groups == 0 && a.Cmid % a.groups == 0, "dfn_conv2d: groups %d must divide %d and %d", a.groups, a.Cin, a.Cmid);
  MI355_REQUIRE(a.pw || a.Cout == a.Cmid, "dfn_conv2d: without a pointwise conv Cout (%d) must equal Cmid (%d)", a.Cout, a.Cmid);
  MI355_REQUIRE(a.kt >= 1 && a.kt <= 5 && (a.kf == 1 || a.kf == 3) && a.lookahead >= 0 && a.lookahead <= a.kt - 1 && (a.fstride == 1 || a.fstride == 2) &&
                    a.act >= 0 && a.act <= 2 && (!a.transposed || a.lookahead == 0),
                "dfn_conv2d: kt 1..5, kf 1 or 3, lookahead 0..kt-1 (0 when transposed), fstride 1 or 2, act 0..2 (got kt %d, kf %d, lookahead %d, fstride %d, act %d)",
                a.kt, a.kf, a.lookahead, a.fstride, a.act);
  const int Fo = mi355_dfn_conv2d_fo(a.F, a.kf, a.fstride, a.transposed);
  MI355_REQUIRE(Fo >= 1, "dfn_conv2d: no output bins");
  MI355_REQUIRE(a.x_bstride >= (int64_t)a.T * a.F * a.Cin && a.y_bstride >= (int64_t)a.T * Fo * a.Cout && (!a.add || a.add_bstride >= (int64_t)a.T * Fo * a.Cout),
                "dfn_conv2d: bad strides");
  const int CM = a.Cmid > a.Cout ? a.Cmid : a.Cout, P = 256 / CM;
  const int64_t blocks = ((int64_t)a.T * Fo + P - 1) / P;
  MI355_REQUIRE(blocks <= 0x7fffffff, "dfn_conv2d: too many positions");
  MI355_CLEAR_ERROR();
  hipLaunchKernelGGL(dfn_conv2d_kernel, dim3((unsigned)blocks, a.B), dim3(256), 0, (hipStream_t)stream, a, Fo, CM, P);
  MI355_LAUNCH_CHECK("dfn_conv2d");
  return MI355_OK;
}

extern "C" int mi355_dfn_apply(const mi355_dfn_apply_args* ap, void* stream) {
  MI355_REQUIRE(ap && ap->spec && ap->m && ap->erb_inv_fb && ap->coef && ap->out, "dfn_apply: null tensor");
  const mi355_dfn_apply_args a = *ap;
  MI355_REQUIRE(a.B >= 1 && a.B <= 65535 && a.T >= 1 && a.F >= 1 && a.E >= 1 && a.D >= 1 && a.D <= a.F && a.order >= 1 && a.df_lookahead >= 0 &&
                    a.df_lookahead <= a.order - 1,
                "dfn_apply: bad shape (B %d, T %d, F %d, E %d, D %d, order %d, lookahead %d)", a.B, a.T, a.F, a.E, a.D, a.order, a.df_lookahead);
  MI355_REQUIRE(a.wnorm > 0.f, "dfn_apply: wnorm must be positive");
  MI355_REQUIRE(a.spec_bstride >= (int64_t)a.T * a.F * 2 && a.out_bstride >= (int64_t)a.T * a.F * 2, "dfn_apply: bad strides");
  const int64_t blocks = ((int64_t)a.T * a.F + 255) / 256;
  MI355_REQUIRE(blocks <= 0x7fffffff, "dfn_apply: too many elements");
  MI355_CLEAR_ERROR();
  hipLaunchKernelGGL(dfn_apply_kernel, dim3((unsigned)blocks, a.B), dim3(256), 0, (hipStream_t)stream, a);
  MI355_LAUNCH_CHECK("dfn_apply");
  return MI355_OK;
}
