// The routed expert FFN of Ling / Ming on MLX's affine group-quantised expert weights (QuantizedSwitchLinear; include/mi355audio.h:
// mi355_moe_qglu): the grouped GEMM of moe.hip with the PACKED CODES as its weight operand.  Plan, workspace, tile list and combine are those of
// moe.hip; only the two tile launches are here.
//
//   out[r, n] = sum_groups fmaf(scale[e, n, group], S, zero[e, n, group] * X[r, group]) + bias[e, n],   S = sum x q,  X = sum x   (fp32, fixed order)
//
// moe_qtile_kernel.  A workgroup is one tile (up to 32 sorted rows of ONE expert e) x 32 output columns, four waves: wave (c = wave & 1,
// p = wave >> 1) owns the 16 columns [16 c, 16 c + 16) and the groups p, p + 2, ... of K.  A decode step (k tiles of one live row) so starts
// ceil(columns / 32) workgroups per tile -- 264 for Ling-lite's gate | up (k 6, I 1408), 384 for its down, against 132 / 192 of the float
// kernel's 64-column workgroups on 256 CUs -- and every wave streams its own slab of codes: 16 rows of [E, Ncols, Kdim bits / 32], selected by
// the expert and the column, straight from HBM into registers.  Lane (i = lane & 15, kg = lane >> 4) loads the g / 4 codes
// q[e, n0 + i][group start + kg g / 4 ..) and every eight of them are one A operand of v_mfma_f32_16x16x32_f16 (codes_operand of qcodes.h:
// OR into 0x6400, one packed subtract; the eight sit in qperm order).  The codes are exact in fp16, so two products per step suffice (x hi,
// x lo) where the float kernel needs three.  The codes and the four (scale, zero) pairs of a wave's NEXT group are requested before the current
// group is multiplied.
// The tile's rows are gathered through perm (launch 1: perm[r] / k; launch 2: sorted order), split once per workgroup into fp16 hi + lo
// (split_hi_lo<true>) and staged in LDS in B-fragment order [group][step][kg][row] x 16 bytes with the contraction index in qperm order, 256 K
// values at a time (36 KiB of LDS with the sums: four workgroups a CU); the same pass leaves the eight-column partial sums from which
// X[row, group] is added up once per workgroup.  After the g / 32 steps of a group the per-group accumulator is folded in the MFMA C layout
// (lane: input row i, columns 4 kg + r).  The two K parts are joined through LDS, part 0 + part 1.  GLU launch: the gate and the up streams
// share the staged x and X; h = silu(gate + b_gate) * (up + b_up).  A tile of <= 16 rows stages and multiplies one 16-row block, a taller
// one two: the same kernel, and per output element the same arithmetic.
#include "linear_common.h"
#include "moe_common.h"
#include "qcodes.h"

namespace {

constexpr int TILE = MI355_MOE_TILE_ROWS;
constexpr int QCOLS = MI355_MOE_QCOL_TILE;
constexpr int kChunkK = 256;   // K values of the tile's rows staged at a time
static_assert(TILE == 32 && QCOLS == 32, "moe_qtile_kernel is written for 32-row tiles and 32-column workgroups");

struct QProj {
  const uint32_t* q; const void* sz; const float* bias;   // [E, Ncols, wpr] words, [E, Ncols, gpr] pairs, [E, Ncols] or null
};

struct QTileArgs {
  const float* a; int64_t lda;          // source rows [*, lda >= Kdim]
  const int32_t* perm; int kdiv;        // gather: source row of sorted row r = perm[r] / kdiv; else r itself
  int gather, scatter;                  // scatter: output row of sorted row r = perm[r]; else r itself
  const int4* tiles;
  QProj w0, w1;                         // w1 (the up projection) for GLU only
  int sz_dtype, Ncols, wpr, gpr, gc;    // words / groups per weight row; groups per staged chunk
  float* out; int64_t ldo;
};

template <int BITS, int G, bool GLU>
__global__ __launch_bounds__(256) void moe_qtile_kernel(const QTileArgs p) {
  extern __shared__ __attribute__((aligned(16))) uint4 planes[];   // hi | lo [group][step][kg][row] pieces, part8 [row][KC / 8], xsum [group][row]
  constexpr int NI = GLU ? 2 : 1;
  constexpr int SPG = G / 32, LW = G / 4 * BITS / 32, WPM = BITS / 4;   // MFMA steps a group, words a lane and group, words an operand
  __shared__ float join[2 * NI * 2 * 4 * 64];                           // [c][image][row block][register][lane]
  __shared__ int src_row[TILE], out_row[TILE];
  const int4 tile = p.tiles[blockIdx.x];
  const int e = tile.x, first = tile.y, rows = tile.z;
  if (rows <= 0) return;   // a surplus record: the whole workgroup leaves
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, kg = lane >> 4;
  const int cw = wave & 1, kp = wave >> 1;
  const int RB = rows <= 16 ? 16 : TILE, mtiles = RB >> 4, KC = p.gc * G, gpr = p.gpr;
  const int n0 = blockIdx.y * QCOLS + cw * 16;
  const int img = RB * KC / 8;
  float* part8 = (float*)(planes + 2 * img);
  float* xsum = part8 + RB * (KC / 8);
  if (tid < TILE) {
    const int pr = tid < rows ? ((p.gather || p.scatter) ? p.perm[first + tid] : 0) : -1;
    src_row[tid] = tid < rows ? (p.gather ? pr / p.kdiv : first + tid) : -1;
    out_row[tid] = tid < rows ? (p.scatter ? pr : first + tid) : -1;
  }
  // ---- this lane's slab: row n0 + li of expert e (a tail or dead wave reads the last row and stores nothing)
  const int64_t erow = (int64_t)e * p.Ncols;
  const int64_t qoff = (erow + (n0 + li < p.Ncols ? n0 + li : p.Ncols - 1)) * p.wpr + kg * LW;
  int64_t szrow[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) szrow[r] = (erow + (n0 + 4 * kg + r < p.Ncols ? n0 + 4 * kg + r : p.Ncols - 1)) * gpr;
  const QProj* const proj[2] = {&p.w0, &p.w1};

  uint32_t wc[NI][LW], wn[NI][LW];
  float csc[NI][4], czr[NI][4], nsc[NI][4], nzr[NI][4];
  auto issue = [&](const int gi, uint32_t (&w)[NI][LW], float (&sc)[NI][4], float (&zr)[NI][4]) {
#pragma unroll
    for (int im = 0; im < NI; ++im) {
      load_words<LW>(proj[im]->q + qoff + (int64_t)gi * (G * BITS / 32), w[im]);
#pragma unroll
      for (int r = 0; r < 4; ++r) load_sz(proj[im]->sz, szrow[r] + gi, p.sz_dtype, sc[im][r], zr[im][r]);
    }
  };
  if (kp < gpr) issue(kp, wc, csc, czr);

  f32x4 acc[NI][2];
#pragma unroll
  for (int im = 0; im < NI; ++im) acc[im][0] = acc[im][1] = f32x4{0.f, 0.f, 0.f, 0.f};
  int gi = kp;
  for (int g0 = 0; g0 < gpr; g0 += p.gc) {
    const int gcn = gpr - g0 < p.gc ? gpr - g0 : p.gc, kc8 = gcn * (G / 8);
    __syncthreads();   // src_row is written; the previous chunk's readers are done
    // ---- stage: 16 rows x consecutive 8-column fragments (16 lanes write 256 contiguous bytes)
    for (int f = tid; f < RB * kc8; f += 256) {
      const int rest = f >> 4, c8 = rest % kc8, row = (rest / kc8) * 16 + (f & 15), sr = src_row[row];
      float xv[8];
      if (sr >= 0) {
        const float* xp = p.a + (int64_t)sr * p.lda + (int64_t)g0 * G + 8 * c8;
        const float4 u = *(const float4*)xp, v = *(const float4*)(xp + 4);
        xv[0] = u.x; xv[1] = u.y; xv[2] = u.z; xv[3] = u.w; xv[4] = v.x; xv[5] = v.y; xv[6] = v.z; xv[7] = v.w;
      } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) xv[i] = 0.f;
      }
      const int k = 8 * c8, gl = k / G, within = k % G, kgi = within / (G / 4), j = (within % (G / 4)) >> 3;
      const int piece = ((gl * SPG + j) * 4 + kgi) * RB + row;
      uint4 hi, lo;
      split_hi_lo<true>(xv[qperm(BITS, 0)], xv[qperm(BITS, 1)], hi.x, lo.x);
      split_hi_lo<true>(xv[qperm(BITS, 2)], xv[qperm(BITS, 3)], hi.y, lo.y);
      split_hi_lo<true>(xv[qperm(BITS, 4)], xv[qperm(BITS, 5)], hi.z, lo.z);
      split_hi_lo<true>(xv[qperm(BITS, 6)], xv[qperm(BITS, 7)], hi.w, lo.w);
      planes[piece] = hi;
      planes[img + piece] = lo;
      part8[row * (KC / 8) + c8] = ((xv[0] + xv[1]) + (xv[2] + xv[3])) + ((xv[4] + xv[5]) + (xv[6] + xv[7]));
    }
    __syncthreads();
    for (int t = tid; t < RB * gcn; t += 256) {   // X[row, group]: once per workgroup, the eight-column partials in column order
      const int row = t % RB, gl = t / RB;
      const float* pp = part8 + row * (KC / 8) + gl * (G / 8);
      float s = 0.f;
#pragma unroll
      for (int c = 0; c < G / 8; ++c) s += pp[c];
      xsum[gl * RB + row] = s;
    }
    __syncthreads();
    // ---- this wave's groups inside the chunk
    for (; gi < g0 + gcn; gi += 2) {
      if (gi + 2 < gpr) issue(gi + 2, wn, nsc, nzr);
      const int gl = gi - g0;
      f32x4 accg[NI][2];
#pragma unroll
      for (int im = 0; im < NI; ++im) accg[im][0] = accg[im][1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < SPG; ++j) {
        uint4 A[NI];
#pragma unroll
        for (int im = 0; im < NI; ++im) A[im] = codes_operand<BITS>(wc[im] + j * WPM);
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
          if (mt < mtiles) {
            const int at = ((gl * SPG + j) * 4 + kg) * RB + mt * 16 + li;
            const uint4 xh = planes[at], xl = planes[img + at];
#pragma unroll
            for (int im = 0; im < NI; ++im) {
              accg[im][mt] = mfma_16x16x32<true>(A[im], xh, accg[im][mt]);
              accg[im][mt] = mfma_16x16x32<true>(A[im], xl, accg[im][mt]);
            }
          }
        }
      }
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) {   // fold in the C layout: lane = input row mt 16 + li, columns n0 + 4 kg + r
        if (mt < mtiles) {
          const float X = xsum[gl * RB + mt * 16 + li];
#pragma unroll
          for (int im = 0; im < NI; ++im)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[im][mt][r] += fmaf(csc[im][r], accg[im][mt][r], czr[im][r] * X);
        }
      }
#pragma unroll
      for (int im = 0; im < NI; ++im) {
#pragma unroll
        for (int i = 0; i < LW; ++i) wc[im][i] = wn[im][i];
#pragma unroll
        for (int r = 0; r < 4; ++r) { csc[im][r] = nsc[im][r]; czr[im][r] = nzr[im][r]; }
      }
    }
  }
  // ---- K part 1 hands its sums to part 0: part 0 + part 1
  if (kp == 1) {
#pragma unroll
    for (int im = 0; im < NI; ++im)
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) join[((((cw * NI + im) * 2 + mt) * 4) + r) * 64 + lane] = acc[im][mt][r];
  }
  __syncthreads();
  const int col = n0 + 4 * kg;   // Ncols is a multiple of 4: the lane's four columns are inside the matrix together
  if (kp == 1 || col >= p.Ncols) return;
  float b0[4], b1[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    b0[r] = p.w0.bias ? p.w0.bias[erow + col + r] : 0.f;
    b1[r] = (GLU && p.w1.bias) ? p.w1.bias[erow + col + r] : 0.f;
  }
#pragma unroll
  for (int mt = 0; mt < 2; ++mt) {
    const int m = mt * 16 + li;
    if (m >= rows) continue;   // (and so mt < mtiles)
    float v[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      v[r] = (acc[0][mt][r] + join[((((cw * NI + 0) * 2 + mt) * 4) + r) * 64 + lane]) + b0[r];
      if constexpr (GLU) {
        const float u = (acc[1][mt][r] + join[((((cw * NI + 1) * 2 + mt) * 4) + r) * 64 + lane]) + b1[r];
        v[r] = linear_glu_value(v[r], u);   // silu(gate) * up
      }
    }
    *(float4*)(p.out + (int64_t)out_row[m] * p.ldo + col) = make_float4(v[0], v[1], v[2], v[3]);
  }
}

// ---------------------------------------------------------------------------------------------- validate, launch
#define MQ_UNSUPPORTED(cond, ...)        \
  do {                                   \
    if (cond) {                          \
      mi355_set_error(__VA_ARGS__);      \
      return MI355_ERR_UNSUPPORTED;      \
    }                                    \
  } while (0)

int qproj_check(const char* name, const void* q, const void* sz, int bits, int group, int dt, int Kdim) {
  MQ_UNSUPPORTED(bits != 4 && bits != 8, "moe_qglu: %s bits = %d is not built (4 and 8 are)", name, bits);
  MQ_UNSUPPORTED(group != 32 && group != 64 && group != 128, "moe_qglu: %s group_size = %d is not built (32, 64 and 128 are)", name, group);
  MI355_REQUIRE(q && sz, "moe_qglu: null tensor (%s codes or pairs)", name);
  MI355_REQUIRE(dt == MI355_KV_F32 || dt == MI355_KV_BF16 || dt == MI355_KV_F16, "moe_qglu: %s sz_dtype = %d", name, dt);
  MI355_REQUIRE(aligned16(q), "moe_qglu: %s codes must be 16-byte aligned", name);
  MI355_REQUIRE((((uintptr_t)sz) & (dt == MI355_KV_F32 ? 7 : 3)) == 0, "moe_qglu: %s (scale, zero) pairs are not aligned", name);
  MI355_REQUIRE(Kdim % group == 0, "moe_qglu: %s Kdim = %d is not a multiple of group_size = %d", name, Kdim, group);
  return MI355_OK;
}

template <int BITS, int G>
void qtile_launch_g(const QTileArgs& t, bool glu, dim3 grid, int lds, hipStream_t st) {
  if (glu) hipLaunchKernelGGL((moe_qtile_kernel<BITS, G, true>), grid, dim3(256), lds, st, t);
  else hipLaunchKernelGGL((moe_qtile_kernel<BITS, G, false>), grid, dim3(256), lds, st, t);
}

// one tile launch over [E, Ncols, Kdim] in (bits, group): fills the format-dependent fields of t
void qtile_launch(QTileArgs t, int bits, int group, int Kdim, bool glu, int max_tiles, hipStream_t st) {
  t.wpr = Kdim / 32 * bits;
  t.gpr = Kdim / group;
  t.gc = t.gpr < kChunkK / group ? t.gpr : kChunkK / group;
  const int KC = t.gc * group;
  const int lds = TILE * KC * 4 + TILE * (KC / 8) * 4 + t.gc * TILE * 4;   // hi + lo images, eight-column partials, X
  const dim3 grid((unsigned)max_tiles, (unsigned)((t.Ncols + QCOLS - 1) / QCOLS));
  if (bits == 4) {
    if (group == 32) qtile_launch_g<4, 32>(t, glu, grid, lds, st);
    else if (group == 64) qtile_launch_g<4, 64>(t, glu, grid, lds, st);
    else qtile_launch_g<4, 128>(t, glu, grid, lds, st);
  } else {
    if (group == 32) qtile_launch_g<8, 32>(t, glu, grid, lds, st);
    else if (group == 64) qtile_launch_g<8, 64>(t, glu, grid, lds, st);
    else qtile_launch_g<8, 128>(t, glu, grid, lds, st);
  }
}

}  // namespace

extern "C" int mi355_moe_qglu(const mi355_moe_qglu_args* ap, void* stream) {
  MI355_REQUIRE(ap && ap->x && ap->out, "moe_qglu: null tensor");
  const mi355_moe_qglu_args a = *ap;
  MI355_REQUIRE(a.mode == 0 || a.mode == 1, "moe_qglu: unknown mode %d", a.mode);
  MQ_UNSUPPORTED(a.E > MI355_MOE_MAX_EXPERTS, "moe_qglu: E = %d is above MI355_MOE_MAX_EXPERTS = %d", a.E, MI355_MOE_MAX_EXPERTS);
  if (const int rc = qproj_check("gate", a.q_gate, a.sz_gate, a.bits_gate, a.group_gate, a.szdt_gate, a.D)) return rc;
  if (a.mode == 0) {
    if (const int rc = qproj_check("up", a.q_up, a.sz_up, a.bits_up, a.group_up, a.szdt_up, a.D)) return rc;
    MQ_UNSUPPORTED(a.bits_up != a.bits_gate || a.group_up != a.group_gate || a.szdt_up != a.szdt_gate,
                   "moe_qglu: gate and up must share one format (gate: bits = %d, group_size = %d, sz_dtype = %d; up: bits = %d, group_size = %d, sz_dtype = %d)",
                   a.bits_gate, a.group_gate, a.szdt_gate, a.bits_up, a.group_up, a.szdt_up);
    if (const int rc = qproj_check("down", a.q_down, a.sz_down, a.bits_down, a.group_down, a.szdt_down, a.I)) return rc;
  }
  Layout L;
  if (const int rc = moe_workspace_check("moe_qglu", a.N, a.k, a.E, a.D, a.I, a.workspace, a.workspace_bytes, &L)) return rc;
  MI355_REQUIRE(a.D % 4 == 0 && a.I % 4 == 0, "moe_qglu: D = %d and I = %d must be multiples of 4", a.D, a.I);
  const int out_cols = a.mode == 1 ? a.I : a.D;
  MI355_REQUIRE(a.ldx >= a.D && a.ldx % 4 == 0 && aligned16(a.x) && a.ldo >= out_cols && a.ldo % 4 == 0 && aligned16(a.out),
                "moe_qglu: misaligned rows (x and out rows must be 16-byte aligned and at least D / %d wide)", out_cols);
  if (a.mode == 0) {
    MI355_REQUIRE(a.weights, "moe_qglu: null tensor (weights)");
    MI355_REQUIRE(!a.shared || (a.ld_shared >= a.D && a.ld_shared % 4 == 0 && aligned16(a.shared)), "moe_qglu: misaligned rows (shared)");
    MI355_REQUIRE(!a.res || (a.ld_res >= a.D && a.ld_res % 4 == 0 && aligned16(a.res)), "moe_qglu: misaligned rows (res)");
  }
  char* ws = (char*)a.workspace;
  float* h = (float*)(ws + L.h);
  float* y = (float*)(ws + L.y);
  QTileArgs t{};
  t.a = a.x; t.lda = a.ldx; t.perm = (const int32_t*)(ws + L.perm); t.kdiv = a.k; t.gather = 1; t.tiles = (const int4*)(ws + L.tiles);
  t.w0 = QProj{a.q_gate, a.sz_gate, a.b_gate}; t.sz_dtype = a.szdt_gate; t.Ncols = a.I;
  MI355_CLEAR_ERROR();
  if (a.mode == 1) {
    t.scatter = 1; t.out = a.out; t.ldo = a.ldo;
    qtile_launch(t, a.bits_gate, a.group_gate, a.D, false, (int)L.max_tiles, (hipStream_t)stream);
    MI355_LAUNCH_CHECK("moe_qglu (linear)");
    return MI355_OK;
  }
  t.scatter = 0; t.w1 = QProj{a.q_up, a.sz_up, a.b_up}; t.out = h; t.ldo = a.I;
  qtile_launch(t, a.bits_gate, a.group_gate, a.D, true, (int)L.max_tiles, (hipStream_t)stream);
  QTileArgs d = t;
  d.a = h; d.lda = a.I; d.gather = 0; d.scatter = 1; d.w0 = QProj{a.q_down, a.sz_down, a.b_down}; d.w1 = QProj{}; d.sz_dtype = a.szdt_down;
  d.Ncols = a.D; d.out = y; d.ldo = a.D;
  qtile_launch(d, a.bits_down, a.group_down, a.I, false, (int)L.max_tiles, (hipStream_t)stream);
  moe_combine_launch(y, a.weights, a.N, a.k, a.D, a.shared, a.ld_shared, a.res, a.ld_res, a.out, a.ldo, (hipStream_t)stream);
  MI355_LAUNCH_CHECK("moe_qglu");
  return MI355_OK;
}
