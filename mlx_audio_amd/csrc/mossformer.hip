// MossFormer2 SE 48K (gfx950): the token shift with ScaleNorm, the FLASH gated single-head attention and the gated FSMN memory.
// Reference call sites: FLASH_ShareA_FFConvM.__call__ / cal_attention (sts/models/mossformer2_se/flash_sharea_ffconvm.py:119-188,191-378),
// ScaleNorm (scalenorm.py:35-41), OffsetScale (offsetscale.py:40-57), the rotary embedding of mossformerblock_gfsmn.py:61-63, the ReLU^2 kernel of
// flash_attention_kernels.py:107-132, Gated_FSMN (gated_fsmn.py:105-116) and UniDeepFsmn (unideepfsmn.py:96-123).  Contracts: include/mi355audio.h.
//
// The attention.  Composed from tensor ops, a layer writes its [B, groups, 256, 256] score tensor to memory twice (once for v, once for u).  Here
// one workgroup owns 128 query rows of a group and `cols` columns of v together with the same columns of u -- the pair the output gate needs --
// on the query tile of attn_tile.h (orientation, C-row order: stated there).  The ReLU^2 stands where the online softmax stood: no running
// maximum, no rescale, no row sum.  The global linear term lin_q kv has the shape of one more P V product (the 128 rows of kv are its "keys",
// the lin_q fragment its "probabilities"), so it runs first through the same attn_pv step and the quadratic term accumulates on top of it.
// A key row at or beyond lens[b] is staged as zeros: its score is relu(0)^2 = 0 and its vu row is zero, so it adds exactly nothing.
//
// Budget per lane (NDB = cols / 16 accumulator blocks): 16 NDB accumulator registers (128 at cols = 128), 64 for the query fragment (the lin_q
// fragment lives in the same registers before it), 16 for the score block.  LDS: 32 keys x 129 floats of K and 32 x 2 cols floats of v | u:
// 48.1 KiB at cols = 128.  S costs as much as 128 columns of O, so a workgroup of `cols` = 128 (256 columns of v | u) spends a third of its MFMA
// steps on S, one of cols = 64 a half; the entry point takes 64 only while its workgroups fit the 256 CUs in one round.
//
// Plain float32, fixed summation orders, no atomics, nothing allocated.
#include <initializer_list>
#include <math.h>
#include "attn_tile.h"

namespace {

constexpr int kD = MI355_GAU_DIM;       // 128
constexpr int kGroup = MI355_GAU_GROUP; // 256
constexpr int kKB = 32;                 // keys (rows) per LDS stage
constexpr int kLDK = kD + 1;            // K row pitch: the S^T operand's ds_read_b32 (lane = key row) is bank-conflict free

__device__ __forceinline__ int item_len(const int32_t* lens, const int b, const int T) { return lens ? min(max(lens[b], 0), T) : T; }

// columns 4 c4 .. 4 c4 + 3 of head h at the row whose qk row is qkrow and whose rope rows are cs / sn: gam / bet are the head's 128 columns
__device__ __forceinline__ float4 gau_head4(const float* qkrow, const float* gam, const float* bet, const float* cs, const float* sn, const int c4) {
  const float4 x = *(const float4*)(qkrow + 4 * c4), g = *(const float4*)(gam + 4 * c4), b = *(const float4*)(bet + 4 * c4);
  float4 z = make_float4(fmaf(x.x, g.x, b.x), fmaf(x.y, g.y, b.y), fmaf(x.z, g.z, b.z), fmaf(x.w, g.w, b.w));
  if (c4 < MI355_GAU_ROPE_DIMS / 4) {
    const int pc = c4 ^ 4;   // the piece 16 columns away
    const float4 xp = *(const float4*)(qkrow + 4 * pc), gp = *(const float4*)(gam + 4 * pc), bp = *(const float4*)(bet + 4 * pc);
    const float4 zp = make_float4(fmaf(xp.x, gp.x, bp.x), fmaf(xp.y, gp.y, bp.y), fmaf(xp.z, gp.z, bp.z), fmaf(xp.w, gp.w, bp.w));
    const float4 co = *(const float4*)(cs + 4 * (c4 & 3)), si = *(const float4*)(sn + 4 * (c4 & 3));
    const bool lo = c4 < 4;   // this piece is the first of its pairs
    float y0, y1;
    rope_pair(lo ? z.x : zp.x, lo ? zp.x : z.x, co.x, si.x, y0, y1); z.x = lo ? y0 : y1;
    rope_pair(lo ? z.y : zp.y, lo ? zp.y : z.y, co.y, si.y, y0, y1); z.y = lo ? y0 : y1;
    rope_pair(lo ? z.z : zp.z, lo ? zp.z : z.z, co.z, si.z, y0, y1); z.z = lo ? y0 : y1;
    rope_pair(lo ? z.w : zp.w, lo ? zp.w : z.w, co.w, si.w, y0, y1); z.w = lo ? y0 : y1;
  }
  return z;
}

// ---------------------------------------------------------------------------------------------------- shift + ScaleNorm
__global__ __launch_bounds__(256) void shift_scalenorm_kernel(const mi355_shift_scalenorm_args a, const float cscale) {
  const int lane = threadIdx.x & 63, t = blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y;
  if (t >= a.T) return;
  const int len = item_len(a.lens, b, a.T);
  const int np = a.C / 4, hp = a.C / 8;   // float4 pieces of a row, of its shifted half
  float* yrow = a.y + (int64_t)b * a.y_bstride + (int64_t)t * a.ldy;
  if (t >= len) {
    for (int p = lane; p < np; p += 64) *(float4*)(yrow + 4 * p) = make_float4(0.f, 0.f, 0.f, 0.f);
    return;
  }
  const float* xrow = a.x + (int64_t)b * a.x_bstride + (int64_t)t * a.ldx;
  float4 v[8];
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int p = lane + 64 * i;
    v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (p < np) {
      if (a.shift && p < hp) {
        if (t > 0) v[i] = *(const float4*)(xrow - a.ldx + 4 * p);
      } else {
        v[i] = *(const float4*)(xrow + 4 * p);
      }
    }
    ss = fmaf(v[i].x, v[i].x, ss); ss = fmaf(v[i].y, v[i].y, ss); ss = fmaf(v[i].z, v[i].z, ss); ss = fmaf(v[i].w, v[i].w, ss);
  }
  ss = wave_sum(ss);
  const float f = (a.g ? *a.g : 1.0f) / fmaxf(sqrtf(ss) * cscale, a.eps);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int p = lane + 64 * i;
    if (p < np) *(float4*)(yrow + 4 * p) = make_float4(v[i].x * f, v[i].y * f, v[i].z * f, v[i].w * f);
  }
}

// ---------------------------------------------------------------------------------------------------- gated FSMN memory
constexpr int kFsmnRows = 32, kFsmnCh = 64;

__global__ __launch_bounds__(256) void gated_fsmn_kernel(const mi355_gated_fsmn_args a) {
  __shared__ float Ps[(kFsmnRows + MI355_GATED_FSMN_MAX_TAPS - 1) * kFsmnCh];
  __shared__ float Ws[kFsmnCh * MI355_GATED_FSMN_MAX_TAPS];   // pitch K (odd): lane = channel reads are bank-conflict free
  const int tid = threadIdx.x, cc = tid & 63, rl = tid >> 6;
  const int t0 = blockIdx.x * kFsmnRows, c0 = blockIdx.y * kFsmnCh, b = blockIdx.z;
  const int len = item_len(a.lens, b, a.T);
  const int K = a.K, left = (K - 1) / 2, c = c0 + cc;
  float* ybase = a.y + (int64_t)b * a.y_bstride;
  if (t0 >= len) {   // a tile of padding rows
    for (int i = 0; i < kFsmnRows / 4; ++i) {
      const int t = t0 + rl + 4 * i;
      if (t < a.T && c < a.C) ybase[(int64_t)t * a.ldy + c] = 0.f;
    }
    return;
  }
  const float* pbase = a.p + (int64_t)b * a.p_bstride;
  for (int e = tid; e < (kFsmnRows + K - 1) * kFsmnCh; e += 256) {
    const int t = t0 - left + e / kFsmnCh, ch = c0 + (e % kFsmnCh);
    Ps[e] = (t >= 0 && t < len && ch < a.C) ? pbase[(int64_t)t * a.ldp + ch] : 0.f;
  }
  for (int e = tid; e < kFsmnCh * K; e += 256) {
    const int ch = c0 + e / K;
    Ws[e] = ch < a.C ? a.w[(int64_t)ch * K + (e % K)] : 0.f;
  }
  __syncthreads();
  if (c >= a.C) return;
  const float* xu = a.xu + (int64_t)b * a.xu_bstride;
  const float* xv = a.xv + (int64_t)b * a.xv_bstride;
  const float* res = a.res + (int64_t)b * a.res_bstride;
  for (int i = 0; i < kFsmnRows / 4; ++i) {
    const int r = rl + 4 * i, t = t0 + r;
    if (t >= a.T) break;
    float y = 0.f;
    if (t < len) {
      float acc = 0.f;
      for (int j = 0; j < K; ++j) acc = fmaf(Ws[cc * K + j], Ps[(r + j) * kFsmnCh + cc], acc);
      const float m = (xu[(int64_t)t * a.ldxu + c] + Ps[(r + left) * kFsmnCh + cc]) + acc;
      y = fmaf(xv[(int64_t)t * a.ldxv + c], m, res[(int64_t)t * a.ldres + c]);
    }
    ybase[(int64_t)t * a.ldy + c] = y;
  }
}

// ---------------------------------------------------------------------------------------------------- kv: per-group partials, then their sum
// One workgroup = one group of 256 rows x 64 columns of vu; wave w owns the rows d = 32 w .. 32 w + 31 of kv.  O^T orientation: A = a vu column
// block from LDS (row m = column e), B = lin_k (column n = d), so lane c holds d = 32 w + c and four consecutive e per register quad.
__global__ __launch_bounds__(256) void gau_kv_partial_kernel(const mi355_gau_kv_args a) {
  __shared__ float Ks[kKB * kD];
  __shared__ float Vs[kKB * 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, c = lane & 31;
  const int e0 = blockIdx.x * 64, g = blockIdx.y, b = blockIdx.z;
  const int len = item_len(a.lens, b, a.T);
  const int g0 = g * kGroup;
  if (g0 >= len) return;   // the sum never reads this group's partial
  const int gend = min(g0 + kGroup, len);
  const float* qk = a.qk + (int64_t)b * a.qk_bstride;
  const float* vu = a.vu + (int64_t)b * a.vu_bstride + e0;
  const float* gam = a.gamma + 3 * kD;
  const float* bet = a.beta + 3 * kD;
  f32x16 o[2];
  attn_zero(o);
  for (int kb = g0; kb < gend; kb += kKB) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kKB * (kD / 4) / 256; ++i) {
      const int e = i * 256 + tid, row = e / (kD / 4), c4 = e % (kD / 4), t = kb + row;
      float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
      if (t < len) z = gau_head4(qk + (int64_t)t * a.ldqk, gam, bet, a.rope_cos + (int64_t)t * 16, a.rope_sin + (int64_t)t * 16, c4);
      *(float4*)(Ks + row * kD + 4 * c4) = z;
    }
#pragma unroll
    for (int i = 0; i < kKB * 16 / 256; ++i) {
      const int e = i * 256 + tid, row = e / 16, c4 = e % 16, t = kb + row;
      *(float4*)(Vs + row * 64 + 4 * c4) = t < len ? *(const float4*)(vu + (int64_t)t * a.ldvu + 4 * c4) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < kKB / 2; ++s) {
      const int r = 2 * s + half;
      const float kval = Ks[r * kD + 32 * wave + c];
      o[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(Vs[r * 64 + c], kval, o[0], 0, 0, 0);
      o[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(Vs[r * 64 + 32 + c], kval, o[1], 0, 0, 0);
    }
  }
  const int G = (a.T + kGroup - 1) / kGroup;
  float* w = a.ws + (((int64_t)b * G + g) * kD + 32 * wave + c) * a.E + e0;
#pragma unroll
  for (int blk = 0; blk < 2; ++blk)
#pragma unroll
    for (int q = 0; q < 4; ++q)
      *(float4*)(w + blk * 32 + 8 * q + 4 * half) = make_float4(o[blk][4 * q], o[blk][4 * q + 1], o[blk][4 * q + 2], o[blk][4 * q + 3]);
}

__global__ __launch_bounds__(256) void gau_kv_sum_kernel(const mi355_gau_kv_args a) {
  const int b = blockIdx.y;
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;   // float4 piece of the item's [128, E]
  if (e >= (int64_t)kD * a.E / 4) return;
  const int len = item_len(a.lens, b, a.T);
  const int G = (a.T + kGroup - 1) / kGroup, ng = (len + kGroup - 1) / kGroup;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int g = 0; g < ng; ++g) {
    const float4 p = *(const float4*)(a.ws + ((int64_t)b * G + g) * kD * a.E + 4 * e);
    s.x += p.x; s.y += p.y; s.z += p.z; s.w += p.w;
  }
  if (len > 0) {
    const float n = (float)len;
    s.x /= n; s.y /= n; s.z /= n; s.w /= n;
  }
  *(float4*)(a.kv + (int64_t)b * a.kv_bstride + 4 * e) = s;
}

// ---------------------------------------------------------------------------------------------------- the attention and its gate
template <int NDB>   // accumulator blocks of 32 columns: NDB / 2 of v, NDB / 2 of u
__global__ __launch_bounds__(256) void gau_attn_kernel(const mi355_gau_attention_args a) {
  constexpr int W = NDB * 16;    // columns of v (and of u) this workgroup owns
  constexpr int LDV = 2 * W;     // V stage pitch: the O^T operand reads lanes-contiguous
  constexpr int VP = 2 * W / 4;  // float4 pieces of a V stage row
  __shared__ float Ks[kKB * kLDK];
  __shared__ float Vs[kKB * LDV];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, c = lane & 31;
  const int q0 = blockIdx.x * 128, c0 = blockIdx.y * W, b = blockIdx.z;
  const int H = a.E / 2;
  const int len = item_len(a.lens, b, a.T);
  float* obase = a.out + (int64_t)b * a.out_bstride + c0;
  if (q0 >= len) {   // a block of padding rows
    for (int e = tid; e < 128 * (W / 4); e += 256) {
      const int r = q0 + e / (W / 4);
      if (r < a.T) *(float4*)(obase + (int64_t)r * a.ldo + (e % (W / 4)) * 4) = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    return;
  }
  const int i0 = q0 + wave * 32, qi = i0 + c;
  const bool wave_active = i0 < len;
  const int qic = qi < len ? qi : len - 1;
  const float* qk = a.qk + (int64_t)b * a.qk_bstride;
  const float* vu = a.vu + (int64_t)b * a.vu_bstride;
  const float* qrow = qk + (int64_t)qic * a.ldqk;
  const float* cs = a.rope_cos + (int64_t)qic * 16;
  const float* sn = a.rope_sin + (int64_t)qic * 16;
  // source column of V stage column pc: the v columns c0 .. c0 + W - 1, then the same columns of u
  auto src_col = [&](int pc) { return pc < W ? c0 + pc : H + c0 + (pc - W); };

  f32x16 o[NDB];
  attn_zero(o);
  float qf[kD / 2];

  // ---- the linear term: o^T = kv^T lin_q^T.  Stage db holds the rows d = 32 db .. 32 db + 31 of kv; step s of attn_pv contracts the rows
  // attn_c_row(s, half), so this lane's fragment entry 16 db + s is lin_q[d = 32 db + attn_c_row(s, half)].
  if (wave_active) {
    const float* gam = a.gamma + kD;
    const float* bet = a.beta + kD;
#pragma unroll
    for (int n = 0; n < kD / 2; ++n) {
      const int d = 32 * (n >> 4) + attn_c_row(n & 15, half);
      qf[n] = fmaf(qrow[d], gam[d], bet[d]);
    }
#pragma unroll
    for (int n = 0; n < 8; ++n) {   // d < 16 and its partner d + 16 are the entries n and n + 8
      const int i = attn_c_row(n, half);
      float y0, y1;
      rope_pair(qf[n], qf[n + 8], cs[i], sn[i], y0, y1);
      qf[n] = y0, qf[n + 8] = y1;
    }
  }
  const float* kvb = a.kv + (int64_t)b * a.kv_bstride;
#pragma unroll
  for (int db = 0; db < kD / kKB; ++db) {
    __syncthreads();
    for (int e = tid; e < kKB * VP; e += 256) {
      const int row = e / VP, p4 = e % VP;
      *(float4*)(Vs + row * LDV + 4 * p4) = *(const float4*)(kvb + (int64_t)(db * kKB + row) * a.E + src_col(4 * p4));
    }
    __syncthreads();
    if (!wave_active) continue;
    f32x16 p;
#pragma unroll
    for (int s = 0; s < 16; ++s) p[s] = qf[16 * db + s];
    attn_pv(o, p, Vs, LDV, half, c);
  }

  // ---- the quadratic term over the keys of this row's group
  if (wave_active) {
    const float* gam = a.gamma;
    const float* bet = a.beta;
#pragma unroll
    for (int s = 0; s < kD / 2; ++s) {
      const int d = 2 * s + half;
      qf[s] = fmaf(qrow[d], gam[d], bet[d]);
    }
#pragma unroll
    for (int s = 0; s < 8; ++s) {   // columns 2 s + half < 16 and their partners, 16 columns = 8 steps away
      const int i = 2 * s + half;
      float y0, y1;
      rope_pair(qf[s], qf[s + 8], cs[i], sn[i], y0, y1);
      qf[s] = y0, qf[s + 8] = y1;
    }
#pragma unroll
    for (int s = 0; s < kD / 2; ++s) qf[s] *= 1.0f / kGroup;   // a power of two: the same bits as scaling the score
  }
  const int g0 = (q0 / kGroup) * kGroup, gend = min(g0 + kGroup, len);
  const float* kgam = a.gamma + 2 * kD;
  const float* kbet = a.beta + 2 * kD;
  for (int kb = g0; kb < gend; kb += kKB) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kKB * (kD / 4) / 256; ++i) {
      const int e = i * 256 + tid, row = e / (kD / 4), c4 = e % (kD / 4), j = kb + row;
      float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
      if (j < len) z = gau_head4(qk + (int64_t)j * a.ldqk, kgam, kbet, a.rope_cos + (int64_t)j * 16, a.rope_sin + (int64_t)j * 16, c4);
      float* kd = Ks + row * kLDK + 4 * c4;
      kd[0] = z.x; kd[1] = z.y; kd[2] = z.z; kd[3] = z.w;
    }
    for (int e = tid; e < kKB * VP; e += 256) {
      const int row = e / VP, p4 = e % VP, j = kb + row;
      *(float4*)(Vs + row * LDV + 4 * p4) = j < len ? *(const float4*)(vu + (int64_t)j * a.ldvu + src_col(4 * p4)) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    __syncthreads();
    if (!wave_active) continue;
    f32x16 acc = attn_kq<kD>(Ks + c * kLDK + half, qf);   // S^T block (32 keys x 32 queries), already / 256
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float s = fmaxf(acc[r], 0.f);
      acc[r] = s * s;
    }
    attn_pv(o, acc, Vs, LDV, half, c);
  }

  if (qi >= a.T) return;
  float* orow = obase + (int64_t)qi * a.ldo;
  const float* vrow = vu + (int64_t)qic * a.ldvu + c0;
#pragma unroll
  for (int d = 0; d < NDB / 2; ++d)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int col = d * 32 + 8 * q + 4 * half;
      float4 y = make_float4(0.f, 0.f, 0.f, 0.f);
      if (qi < len) {
        const float4 v4 = *(const float4*)(vrow + col), u4 = *(const float4*)(vrow + H + col);
        const f32x16& av = o[d];
        const f32x16& au = o[NDB / 2 + d];
        y.x = (au[4 * q] * v4.x) * (1.0f / (1.0f + expf(-(av[4 * q] * u4.x))));
        y.y = (au[4 * q + 1] * v4.y) * (1.0f / (1.0f + expf(-(av[4 * q + 1] * u4.y))));
        y.z = (au[4 * q + 2] * v4.z) * (1.0f / (1.0f + expf(-(av[4 * q + 2] * u4.z))));
        y.w = (au[4 * q + 3] * v4.w) * (1.0f / (1.0f + expf(-(av[4 * q + 3] * u4.w))));
      }
      *(float4*)(orow + col) = y;
    }
}

template <int NDB>
int launch_gau_attn(const mi355_gau_attention_args& a, hipStream_t st) {
  MI355_CLEAR_ERROR();
  hipLaunchKernelGGL(gau_attn_kernel<NDB>, dim3((unsigned)((a.T + 127) / 128), (unsigned)(a.E / 2 / (NDB * 16)), (unsigned)a.B), dim3(256), 0, st, a);
  MI355_LAUNCH_CHECK("gau_attention");
  return MI355_OK;
}

bool aligned4(std::initializer_list<int64_t> strides, std::initializer_list<const void*> ptrs) {
  for (int64_t s : strides)
    if (s % 4) return false;
  for (const void* p : ptrs)
    if ((uintptr_t)p % 16) return false;
  return true;
}

}  // namespace

extern "C" int mi355_shift_scalenorm(const mi355_shift_scalenorm_args* ap, void* stream) {
  MI355_REQUIRE(ap && ap->x && ap->y, "shift_scalenorm: null tensor");
  const mi355_shift_scalenorm_args a = *ap;
  MI355_REQUIRE(a.B > 0 && a.B <= 65535 && a.T >= 1, "shift_scalenorm: bad shape");
  MI355_REQUIRE(a.C >= 8 && a.C % 8 == 0 && a.C <= 2048, "shift_scalenorm: C must be a multiple of 8 in [8, 2048] (got C = %d)", a.C);
  MI355_REQUIRE(a.ldx >= a.C && a.ldy >= a.C, "shift_scalenorm: a row stride is smaller than C");
  MI355_REQUIRE(aligned4({a.ldx, a.ldy, a.x_bstride, a.y_bstride}, {a.x, a.y}), "shift_scalenorm: rows must be 16-byte aligned");
  MI355_REQUIRE(!(a.shift && (const float*)a.y == a.x), "shift_scalenorm: y must not alias x when shift is on");
  MI355_CLEAR_ERROR();
  hipLaunchKernelGGL(shift_scalenorm_kernel, dim3((unsigned)((a.T + 3) / 4), (unsigned)a.B), dim3(256), 0, (hipStream_t)stream, a,
                     (float)pow((double)a.C, -0.5));
  MI355_LAUNCH_CHECK("shift_scalenorm");
  return MI355_OK;
}

extern "C" int mi355_gated_fsmn(const mi355_gated_fsmn_args* ap, void* stream) {
  MI355_REQUIRE(ap && ap->p && ap->xu && ap->xv && ap->res && ap->w && ap->y, "gated_fsmn: null tensor");
  const mi355_gated_fsmn_args a = *ap;
  MI355_REQUIRE(a.B > 0 && a.B <= 65535 && a.T >= 1 && a.C >= 1, "gated_fsmn: bad shape");
  MI355_REQUIRE(a.K >= 1 && a.K % 2 == 1 && a.K <= MI355_GATED_FSMN_MAX_TAPS, "gated_fsmn: K must be odd and at most %d (got K = %d)",
                MI355_GATED_FSMN_MAX_TAPS, a.K);
  MI355_REQUIRE(a.ldp >= a.C && a.ldxu >= a.C && a.ldxv >= a.C && a.ldres >= a.C && a.ldy >= a.C, "gated_fsmn: a row stride is smaller than C");
  MI355_REQUIRE((const float*)a.y != a.p, "gated_fsmn: y must not alias p");
  MI355_CLEAR_ERROR();
  hipLaunchKernelGGL(gated_fsmn_kernel, dim3((unsigned)((a.T + kFsmnRows - 1) / kFsmnRows), (unsigned)((a.C + kFsmnCh - 1) / kFsmnCh), (unsigned)a.B),
                     dim3(256), 0, (hipStream_t)stream, a);
  MI355_LAUNCH_CHECK("gated_fsmn");
  return MI355_OK;
}

extern "C" int mi355_gau_kv(const mi355_gau_kv_args* ap, void* stream) {
  MI355_REQUIRE(ap && ap->qk && ap->vu && ap->gamma && ap->beta && ap->rope_cos && ap->rope_sin && ap->ws && ap->kv, "gau_kv: null tensor");
  const mi355_gau_kv_args a = *ap;
  MI355_REQUIRE(a.B > 0 && a.B <= 65535 && a.T >= 1, "gau_kv: bad shape");
  MI355_REQUIRE(a.E >= 64 && a.E % 64 == 0 && a.E <= MI355_GAU_MAX_E, "gau_kv: E must be a multiple of 64 in [64, %d] (got E = %d)", MI355_GAU_MAX_E, a.E);
  MI355_REQUIRE(a.rope_rows >= a.T, "gau_kv: the rope tables have %d rows, T = %d", a.rope_rows, a.T);
  MI355_REQUIRE(a.ldqk >= kD && a.ldvu >= a.E && a.kv_bstride >= (int64_t)kD * a.E, "gau_kv: a stride is smaller than its width");
  const int64_t G = (a.T + kGroup - 1) / kGroup;
  MI355_REQUIRE(G <= 65535 && a.ws_floats >= (int64_t)a.B * G * kD * a.E, "gau_kv: the workspace needs B * ceil(T / 256) * 128 * E floats");
  MI355_REQUIRE(aligned4({a.ldqk, a.ldvu, a.qk_bstride, a.vu_bstride, a.kv_bstride}, {a.qk, a.vu, a.gamma, a.beta, a.rope_cos, a.rope_sin, a.ws, a.kv}),
                "gau_kv: rows must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  MI355_CLEAR_ERROR();
  hipLaunchKernelGGL(gau_kv_partial_kernel, dim3((unsigned)(a.E / 64), (unsigned)G, (unsigned)a.B), dim3(256), 0, st, a);
  MI355_LAUNCH_CHECK("gau_kv (partials)");
  hipLaunchKernelGGL(gau_kv_sum_kernel, dim3((unsigned)((kD * a.E / 4 + 255) / 256), (unsigned)a.B), dim3(256), 0, st, a);
  MI355_LAUNCH_CHECK("gau_kv (sum)");
  return MI355_OK;
}

extern "C" int mi355_gau_attention(const mi355_gau_attention_args* ap, void* stream) {
  MI355_REQUIRE(ap && ap->qk && ap->vu && ap->kv && ap->gamma && ap->beta && ap->rope_cos && ap->rope_sin && ap->out, "gau_attention: null tensor");
  const mi355_gau_attention_args a = *ap;
  if (a.causal || a.qk_dim != kD || a.group != kGroup) {
    mi355_set_error("gau_attention: only the non-causal form with qk_dim = %d and group = %d is built (got causal = %d, qk_dim = %d, group = %d)", kD,
                    kGroup, a.causal, a.qk_dim, a.group);
    return MI355_ERR_UNSUPPORTED;
  }
  MI355_REQUIRE(a.B > 0 && a.B <= 65535 && a.T >= 1, "gau_attention: bad shape");
  MI355_REQUIRE(a.E >= 64 && a.E % 64 == 0 && a.E <= MI355_GAU_MAX_E, "gau_attention: E must be a multiple of 64 in [64, %d] (got E = %d)",
                MI355_GAU_MAX_E, a.E);
  MI355_REQUIRE(a.rope_rows >= a.T, "gau_attention: the rope tables have %d rows, T = %d", a.rope_rows, a.T);
  const int H = a.E / 2;
  MI355_REQUIRE(a.ldqk >= kD && a.ldvu >= a.E && a.ldo >= H && a.kv_bstride >= (int64_t)kD * a.E, "gau_attention: a stride is smaller than its width");
  MI355_REQUIRE(aligned4({a.ldqk, a.ldvu, a.ldo, a.qk_bstride, a.vu_bstride, a.kv_bstride, a.out_bstride},
                         {a.qk, a.vu, a.kv, a.gamma, a.beta, a.rope_cos, a.rope_sin, a.out}),
                "gau_attention: rows must be 16-byte aligned");
  MI355_REQUIRE((const float*)a.out != a.vu, "gau_attention: out must not alias vu");
  int cols = a.cols;
  if (cols == 0) {
    // 128 columns per workgroup spend a third of the MFMA steps on S, 64 a half: take 64 only while its workgroups still fit the 256 CUs in one
    // round (measured at E = 2048: 1 x 496 frames 80 us against 112 us; 1 x 2496 frames 181 us against 135 us).  The choice moves columns between
    // workgroups, never the order of a sum.
    const int64_t tiles = (int64_t)((a.T + 127) / 128) * a.B;
    cols = (H % 128 == 0 && tiles * (H / 64) > 256) ? 128 : (H % 64 == 0 ? 64 : 32);
  }
  MI355_REQUIRE((cols == 32 || cols == 64 || cols == 128) && H % cols == 0, "gau_attention: cols must be 0, 32, 64 or 128 and divide E / 2 (got cols = %d, E = %d)",
                a.cols, a.E);
  hipStream_t st = (hipStream_t)stream;
  switch (cols) {
    case 32: return launch_gau_attn<2>(a, st);
    case 64: return launch_gau_attn<4>(a, st);
    default: return launch_gau_attn<8>(a, st);
  }
}
