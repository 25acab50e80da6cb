// GroupNorm with one group (gfx950): per-sample statistics -> per-(sample, channel) affine coefficients -> apply.
// Reference call sites: EncodecConv1d / EncodecConvTranspose1d with norm_type = "time_group_norm"
// (codec/models/encodec/encodec.py:172-291: nn.GroupNorm(1, C, pytorch_compatible=True) behind every conv of the 48 kHz model),
// EncodecResnetBlock (:305-337: shortcut_norm(shortcut(x)) + norm2(conv2(...)) -- the two-operand apply).
#include "block_reduce.h"

namespace {

constexpr int kPart = MI355_GN_PART_ELEMS;   // elements per workgroup of the statistics pass
constexpr int kVecPerLane = kPart / 4 / 256; // float4 per lane
static_assert(kPart % 1024 == 0, "a part is a whole number of float4 per lane");

// The block sums below have a fixed association (DPP wave sums, respectively shuffle sums in float64, then the four wave shares in order).

// Statistics of one part: flat elements [e0, e1) of sample b (the valid rows are contiguous when ldx == C; otherwise the element index is
// mapped to (row, channel) and read 4 bytes at a time).  The part is read ONCE into registers; sums are taken on deviations from the part's
// first element (a pivot), so a large common offset does not cost the fp32 sums their low bits, then M2 on deviations from the part's mean.
__global__ __launch_bounds__(256) void group_norm_stats_kernel(const mi355_group_norm_stats_args a) {
  __shared__ float red[4];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int len = a.lens ? min(max(a.lens[b], 0), a.L) : a.L;
  const int64_t total = (int64_t)len * a.C;
  const int64_t e0 = (int64_t)blockIdx.x * kPart;
  if (e0 >= total) return;   // workgroup-uniform
  const int n = (int)min((int64_t)kPart, total - e0);
  const float* xb = a.x + (int64_t)b * a.x_bstride;
  float v[kVecPerLane * 4];
  bool ok[kVecPerLane * 4];
  float pivot;
  if (a.ldx == a.C) {
    const float* p = xb + e0;
    pivot = p[0];
    // lane tid owns elements 4 (tid + 256 j) .. + 3 of the part WHATEVER the sample's alignment (16-byte loads when the part starts on a 16-byte
    // boundary, 4-byte loads otherwise): the sums' association does not depend on where a sample lies, so equal samples give equal bits
    const bool al = (((uintptr_t)p) & 15) == 0;   // workgroup-uniform (a part is a multiple of 16 bytes: the sample's alignment)
#pragma unroll
    for (int j = 0; j < kVecPerLane; ++j) {
      const int base = (tid + j * 256) * 4;
      if (al && base + 4 <= n) {
        const float4 q = *(const float4*)(p + base);
        v[j * 4 + 0] = q.x; v[j * 4 + 1] = q.y; v[j * 4 + 2] = q.z; v[j * 4 + 3] = q.w;
        ok[j * 4 + 0] = ok[j * 4 + 1] = ok[j * 4 + 2] = ok[j * 4 + 3] = true;
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          ok[j * 4 + k] = base + k < n;
          v[j * 4 + k] = p[ok[j * 4 + k] ? base + k : 0];   // clamped load, selected below: never past the part
        }
      }
    }
  } else {
    pivot = xb[(e0 / a.C) * a.ldx + (e0 % a.C)];
#pragma unroll
    for (int i = 0; i < kVecPerLane * 4; ++i) {
      const int k = tid + i * 256;
      ok[i] = k < n;
      const int64_t e = e0 + (ok[i] ? k : 0);
      v[i] = xb[(e / a.C) * a.ldx + (e % a.C)];
    }
  }
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < kVecPerLane * 4; ++i) s += ok[i] ? v[i] - pivot : 0.f;
  s = block_join_sum<4>(wave_sum_fast(s), red);
  const float dmean = s / (float)n;   // part mean - pivot
  float m2 = 0.f;
#pragma unroll
  for (int i = 0; i < kVecPerLane * 4; ++i) {
    const float d = (v[i] - pivot) - dmean;
    m2 += ok[i] ? d * d : 0.f;
  }
  m2 = block_join_sum<4>(wave_sum_fast(m2), red);
  if (tid == 0) {
    double* out = a.partials + (int64_t)b * a.partials_bstride + (int64_t)blockIdx.x * 2;
    out[0] = (double)pivot * (double)n + (double)s;
    out[1] = (double)m2;
  }
}

// One workgroup per sample: merge the partial (sum, M2) pairs in float64 (two sweeps: total -> mean, then Chan's decomposition of the sum of
// squared deviations), then write the coefficient rows.  CONV: the pairs are a conv epilogue's [nblk][C] floats, each over the rows of one
// 64-row block of one channel; otherwise the doubles of group_norm_stats_kernel, each over up to kPart elements.
template <bool CONV>
__global__ __launch_bounds__(256) void group_norm_coef_kernel(const mi355_group_norm_coef_args a) {
  __shared__ double red[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int len = a.lens ? min(max(a.lens[b], 0), a.L) : a.L;
  const int64_t total = (int64_t)len * a.C;
  const int64_t npairs = CONV ? (int64_t)((len + MI355_STATS_ROWS - 1) / MI355_STATS_ROWS) * a.C : (total + kPart - 1) / kPart;
  const float* pf = (const float*)a.partials + (int64_t)b * a.partials_bstride;
  const double* pd = (const double*)a.partials + (int64_t)b * a.partials_bstride;
  auto cnt_of = [&](int64_t i) -> double {
    if (CONV) return (double)min(MI355_STATS_ROWS, len - (int)(i / a.C) * MI355_STATS_ROWS);
    return (double)min((int64_t)kPart, total - i * kPart);
  };
  double s = 0.0;
  for (int64_t i = tid; i < npairs; i += 256) s += CONV ? (double)pf[i * 2] : pd[i * 2];
  const double tot = block_join_sum<4>(wave_sum_d(s), red);
  const double mean = total > 0 ? tot / (double)total : 0.0;
  double m2 = 0.0;
  for (int64_t i = tid; i < npairs; i += 256) {
    const double si = CONV ? (double)pf[i * 2] : pd[i * 2], qi = CONV ? (double)pf[i * 2 + 1] : pd[i * 2 + 1];
    const double c = cnt_of(i), d = si / c - mean;
    m2 += qi + d * d * c;
  }
  m2 = block_join_sum<4>(wave_sum_d(m2), red);
  const double var = total > 0 ? m2 / (double)total : 0.0;
  const double rstd = 1.0 / sqrt(var + (double)a.eps);
  if (tid == 0 && a.mean_rstd) { a.mean_rstd[b * 2] = (float)mean; a.mean_rstd[b * 2 + 1] = (float)rstd; }
  const int rep = a.rep > 0 ? a.rep : 1;
  for (int j = tid; j < a.out_ld; j += 256) {
    float sc = 0.f, sh = 0.f;
    if (j < rep * a.C) {
      const int c = j % a.C;
      const double w = a.weight ? (double)a.weight[c] : 1.0, be = a.bias ? (double)a.bias[c] : 0.0;
      const double scd = w * rstd;
      sc = (float)scd;
      sh = (float)(be - mean * scd);
    }
    a.scale[(int64_t)b * a.out_ld + j] = sc;
    a.shift[(int64_t)b * a.out_ld + j] = sh;
  }
}

// y = x0 * scale0 + shift0 (+ x1 * scale1 + shift1 | + x1).  VEC: four channels per lane and access (16 bytes); a lane takes four such groups
// 256 apart, so a wave has four independent 1-KB requests in flight per operand.  grid (ceil(groups / 1024), B).
template <bool VEC>
__global__ __launch_bounds__(256) void group_norm_apply_kernel(const mi355_group_norm_apply_args a) {
  constexpr int W = VEC ? 4 : 1;
  const int b = blockIdx.y;
  const int gpr = a.C / W;   // groups per row
  const int64_t ngroups = (int64_t)a.L * gpr;
  const float* x0 = a.x0 + (int64_t)b * a.x0_bstride + (int64_t)a.row_off0 * a.ldx0;
  const float* x1 = a.x1 ? a.x1 + (int64_t)b * a.x1_bstride + (int64_t)a.row_off1 * a.ldx1 : nullptr;
  float* y = a.y + (int64_t)b * a.y_bstride;
  const float* sc0 = a.scale0 + (int64_t)b * a.coef_ld;
  const float* sh0 = a.shift0 + (int64_t)b * a.coef_ld;
  const float* sc1 = a.scale1 ? a.scale1 + (int64_t)b * a.coef_ld : nullptr;
  const float* sh1 = a.scale1 ? a.shift1 + (int64_t)b * a.coef_ld : nullptr;
  const int64_t g0 = (int64_t)blockIdx.x * 1024 + threadIdx.x;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int64_t g = g0 + j * 256;
    if (g >= ngroups) break;
    const int64_t row = g / gpr;
    const int c = (int)(g - row * gpr) * W;
    if (VEC) {
      const float4 v = *(const float4*)(x0 + row * a.ldx0 + c);
      const float4 s = *(const float4*)(sc0 + c), h = *(const float4*)(sh0 + c);
      float4 o = make_float4(fmaf(v.x, s.x, h.x), fmaf(v.y, s.y, h.y), fmaf(v.z, s.z, h.z), fmaf(v.w, s.w, h.w));
      if (x1) {
        const float4 u = *(const float4*)(x1 + row * a.ldx1 + c);
        if (sc1) {
          const float4 s1 = *(const float4*)(sc1 + c), h1 = *(const float4*)(sh1 + c);
          o.x += fmaf(u.x, s1.x, h1.x); o.y += fmaf(u.y, s1.y, h1.y); o.z += fmaf(u.z, s1.z, h1.z); o.w += fmaf(u.w, s1.w, h1.w);
        } else {
          o.x += u.x; o.y += u.y; o.z += u.z; o.w += u.w;
        }
      }
      *(float4*)(y + row * a.ldy + c) = o;
    } else {
      float o = fmaf(x0[row * a.ldx0 + c], sc0[c], sh0[c]);
      if (x1) {
        const float u = x1[row * a.ldx1 + c];
        o += sc1 ? fmaf(u, sc1[c], sh1[c]) : u;
      }
      y[row * a.ldy + c] = o;
    }
  }
}

bool aligned16(const void* p) { return ((uintptr_t)p) % 16 == 0; }

}  // namespace

extern "C" int mi355_group_norm_stats(const mi355_group_norm_stats_args* ap, void* stream) {
  MI355_REQUIRE(ap && ap->x && ap->partials, "group_norm_stats: null tensor");
  const mi355_group_norm_stats_args a = *ap;
  MI355_REQUIRE(a.B > 0 && a.B <= 65535 && a.C > 0 && a.L > 0 && a.ldx >= a.C, "group_norm_stats: bad shape");
  const int64_t nparts = ((int64_t)a.L * a.C + kPart - 1) / kPart;
  MI355_REQUIRE(nparts <= 0x7fffffff, "group_norm_stats: sample too long");
  MI355_REQUIRE(a.partials_bstride >= nparts * 2 && ((uintptr_t)a.partials) % 8 == 0, "group_norm_stats: partials buffer too small or unaligned");
  MI355_CLEAR_ERROR();
  hipLaunchKernelGGL(group_norm_stats_kernel, dim3((unsigned)nparts, a.B), dim3(256), 0, (hipStream_t)stream, a);
  MI355_LAUNCH_CHECK("group_norm_stats");
  return MI355_OK;
}

extern "C" int mi355_group_norm_coef(const mi355_group_norm_coef_args* ap, void* stream) {
  MI355_REQUIRE(ap && ap->partials && ap->scale && ap->shift, "group_norm_coef: null tensor");
  const mi355_group_norm_coef_args a = *ap;
  const int rep = a.rep > 0 ? a.rep : 1;
  MI355_REQUIRE(a.B > 0 && a.C > 0 && a.L > 0 && a.rep >= 0 && (int64_t)rep * a.C <= a.out_ld, "group_norm_coef: bad shape (out_ld must hold rep * C columns)");
  MI355_REQUIRE(((uintptr_t)a.partials) % 8 == 0, "group_norm_coef: partials must be 8-byte aligned");
  if (a.conv_partials) MI355_REQUIRE(a.partials_bstride >= (int64_t)((a.L + MI355_STATS_ROWS - 1) / MI355_STATS_ROWS) * a.C * 2, "group_norm_coef: conv partials buffer too small");
  else MI355_REQUIRE(a.partials_bstride >= (((int64_t)a.L * a.C + kPart - 1) / kPart) * 2, "group_norm_coef: partials buffer too small");
  MI355_CLEAR_ERROR();
  if (a.conv_partials) hipLaunchKernelGGL(group_norm_coef_kernel<true>, dim3(a.B), dim3(256), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(group_norm_coef_kernel<false>, dim3(a.B), dim3(256), 0, (hipStream_t)stream, a);
  MI355_LAUNCH_CHECK("group_norm_coef");
  return MI355_OK;
}

extern "C" int mi355_group_norm_apply(const mi355_group_norm_apply_args* ap, void* stream) {
  MI355_REQUIRE(ap && ap->x0 && ap->scale0 && ap->shift0 && ap->y, "group_norm_apply: null tensor");
  const mi355_group_norm_apply_args a = *ap;
  MI355_REQUIRE(a.B > 0 && a.B <= 65535 && a.C > 0 && a.L > 0 && a.ldx0 >= a.C && a.ldy >= a.C && a.coef_ld >= a.C && a.row_off0 >= 0, "group_norm_apply: bad shape");
  MI355_REQUIRE((a.scale1 == nullptr) == (a.shift1 == nullptr), "group_norm_apply: scale1 / shift1 must come together");
  MI355_REQUIRE(a.x1 || !a.scale1, "group_norm_apply: coefficients of a second operand without the operand");
  MI355_REQUIRE(!a.x1 || (a.ldx1 >= a.C && a.row_off1 >= 0), "group_norm_apply: bad second operand");
  bool vec = a.C % 4 == 0 && a.ldx0 % 4 == 0 && a.ldy % 4 == 0 && a.coef_ld % 4 == 0 && a.x0_bstride % 4 == 0 && a.y_bstride % 4 == 0 &&
             aligned16(a.x0) && aligned16(a.y) && aligned16(a.scale0) && aligned16(a.shift0);
  if (a.x1) vec = vec && a.ldx1 % 4 == 0 && a.x1_bstride % 4 == 0 && aligned16(a.x1);
  if (a.scale1) vec = vec && aligned16(a.scale1) && aligned16(a.shift1);
  const int64_t ngroups = (int64_t)a.L * (a.C / (vec ? 4 : 1));
  const int64_t gx = (ngroups + 1023) / 1024;
  MI355_REQUIRE(gx <= 0x7fffffff, "group_norm_apply: tensor too large");
  MI355_CLEAR_ERROR();
  if (vec) hipLaunchKernelGGL(group_norm_apply_kernel<true>, dim3((unsigned)gx, a.B), dim3(256), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(group_norm_apply_kernel<false>, dim3((unsigned)gx, a.B), dim3(256), 0, (hipStream_t)stream, a);
  MI355_LAUNCH_CHECK("group_norm_apply");
  return MI355_OK;
}
