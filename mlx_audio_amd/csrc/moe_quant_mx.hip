// The routed expert FFN of Ling / Ming on MLX's block-scaled floating-point expert weights (QuantizedSwitchLinear with mode = mxfp4 / nvfp4 /
// mxfp8; include/mi355audio.h: mi355_moe_qglu_mx; the format is stated there at mi355_qlinear_mx).  Plan, workspace, tile list and combine are
// those of moe.hip; only the two tile launches are here.
//
//   out[r, n] = sum_k x[r, k] * value(code[e, n, k]) * value(scale[e, n, k / g]) + bias[e, n]      (fp32, fixed order)
//
// A kernel of its own beside moe_qtile_kernel (moe_quant.hip), for the reason qlinear_mx.hip gives: there is no zero term, so the X[row, group]
// sums, their two LDS passes and their LDS are gone; the scale is one BYTE per group; the codes are decoded by the gfx950 conversions in element
// order, so x is staged as it is (no qperm).
//
// moe_qtile_mx_kernel<MODE, GLU>.  A workgroup is one tile (up to 32 sorted rows of ONE expert e) x 32 output columns, four waves: wave
// (c = wave & 1, p = wave >> 1) owns the 16 columns [16 c, 16 c + 16) and the RUNS p, p + 2, ... of K.  A run is 128 codes = four 32-code steps
// of v_mfma_f32_16x16x32_f16, so that the scale bytes of a run are four consecutive bytes (eight at nvfp4) and arrive as one (two) 32-bit loads.
// Lane (i = lane & 15, kg = lane >> 4) streams weight row n0 + i of [E, Ncols, .] straight from HBM into registers: per step the one (4 bits) or
// two (8 bits) words that hold codes [8 kg, 8 kg + 8), which mx_operand turns into the A operand -- no dequantised float in memory, no LDS hop.
// The words and scale words of the wave's NEXT run are requested before the current run is multiplied: 4 x 16 rows x 16 (32) bytes a wave in
// flight, four times what a group-32 wave of the affine kernel keeps in flight.
// The tile's rows are gathered through perm (launch 1: perm[r] / k; launch 2: sorted order), split once per workgroup into fp16 hi + lo
// (split_hi_lo<true>) and staged in LDS in B-fragment order [run][step][kg][row] x 16 bytes, 256 K values (two runs, one per K part) at a time;
// columns past Kdim inside the last run are zeros.
//   mxfp4 / mxfp8: a group is one step.  Two MFMAs (x hi, x lo) into a zeroed tile, then acc = fmaf(2^e, tile, acc) in the C layout (lane: input
//                  row i, columns 4 kg + r; exact, a power of two); the lane's four columns each bring the run's four E8M0 bytes in one load.
//   nvfp4:         a step holds two groups with E4M3 scales, so nothing can be folded after the MFMA: the lane's own scale (group 2 step +
//                  (kg >> 1) of row n0 + i) is picked out of the run's scale words by v_perm_b32, converted into both halves of a register and
//                  multiplied into the operand by four packed fp16 multiplies (E2M1 x E4M3 is an exact normal fp16 value); the MFMAs accumulate
//                  directly.  A last half step (Kdim % 32 == 16) has no words for kg >= 2: those lanes contribute zero operands.
// The two K parts are joined through LDS (over the staged images, once every reader is done), part 0 + part 1.  GLU launch: the gate and the up
// streams share the staged x; h = silu(gate + b_gate) * (up + b_up).  A tile of <= 16 rows stages and multiplies one 16-row block, a taller one
// two: the same kernel, and per output element the same arithmetic.
// LDS.  Without part8 / xsum and with the join laid over the images a workgroup holds 32 KiB of images and 256 bytes of row indices, where the
// affine kernel holds 36 KiB + 8 KiB of join.  The freed LDS is spent on MORE WORKGROUPS PER CU (four fit in 160 KiB where the affine kernel's
// 44 KiB admit three), not on a larger staged chunk: the weight stream already runs across chunk boundaries (the next run is in flight over the
// barrier), so a longer chunk would only save barriers, while at prefill sizes a further resident workgroup hides the staging loads of its
// neighbours.  Neither choice has been measured against the other.
// Bounds: a tail or dead wave reads the LAST weight row and stores nothing; no word or scale byte past a row's end is read (absent ones are
// zeros); a surplus tile record (rows = 0) leaves at once.
#include "linear_common.h"
#include "moe_common.h"
#include "qcodes.h"

namespace {

constexpr int TILE = MI355_MOE_TILE_ROWS;
constexpr int QCOLS = MI355_MOE_QCOL_TILE;
constexpr int kRunK = 128;     // K values of one run: four steps of 32 codes
constexpr int kChunkK = 256;   // K values of the tile's rows staged at a time: one run per K part
constexpr int kChunkRuns = kChunkK / kRunK;
static_assert(TILE == 32 && QCOLS == 32, "moe_qtile_mx_kernel is written for 32-row tiles and 32-column workgroups");

constexpr int mode_bits(const int mode) { return mode == MI355_QMODE_MXFP8 ? 8 : 4; }

struct MXProj {
  const uint32_t* q; const uint8_t* sc; const float* bias;   // [E, Ncols, wpr] words, [E, Ncols, gpr] bytes, [E, Ncols] or null
};

struct MXTileArgs {
  const float* a; int64_t lda;          // source rows [*, lda >= Kdim]
  const int32_t* perm; int kdiv;        // gather: source row of sorted row r = perm[r] / kdiv; else r itself
  int gather, scatter;                  // scatter: output row of sorted row r = perm[r]; else r itself
  const int4* tiles;
  MXProj w0, w1;                        // w1 (the up projection) for GLU only
  int Ncols, Kdim, wpr, gpr;            // words / scale bytes per weight row
  int nsteps, nruns, rc;                // 32-code steps (at nvfp4 the last may hold one group) and runs of a row; runs per staged chunk
  int wide;                             // a run's scale bytes come as 32-bit loads (load_scale_word)
  float* out; int64_t ldo;
};

template <int MODE, bool GLU>
__global__ __launch_bounds__(256) void moe_qtile_mx_kernel(const MXTileArgs p) {
  extern __shared__ __attribute__((aligned(16))) uint4 planes[];   // hi | lo [run][step][kg][row] pieces of eight fp16; then the join
  constexpr int NI = GLU ? 2 : 1;
  constexpr int BITS = mode_bits(MODE), WPL = BITS / 4;            // words of one operand: a lane's share of a step
  constexpr bool NV = MODE == MI355_QMODE_NVFP4;
  constexpr int SW = NV ? 2 : 4;                                   // scale words a lane holds per run and stream
  __shared__ int src_row[TILE], out_row[TILE];
  const int4 tile = p.tiles[blockIdx.x];
  const int e = tile.x, first = tile.y, rows = tile.z;
  if (rows <= 0) return;   // a surplus record: the whole workgroup leaves
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, kg = lane >> 4;
  const int cw = wave & 1, kp = wave >> 1;
  const int RB = rows <= 16 ? 16 : TILE, mtiles = RB >> 4;
  const int n0 = blockIdx.y * QCOLS + cw * 16;
  const int img = RB * p.rc * (kRunK / 8);
  if (tid < TILE) {
    const int pr = tid < rows ? ((p.gather || p.scatter) ? p.perm[first + tid] : 0) : -1;
    src_row[tid] = tid < rows ? (p.gather ? pr / p.kdiv : first + tid) : -1;
    out_row[tid] = tid < rows ? (p.scatter ? pr : first + tid) : -1;
  }
  // ---- this lane's weight row n0 + li of expert e (a tail or dead wave reads the last row and stores nothing) and its scale rows: at mxfp4 /
  //      mxfp8 the rows of its four C columns, at nvfp4 ([0]) the row of its A operand
  const int64_t erow = (int64_t)e * p.Ncols;
  const int nA = n0 + li < p.Ncols ? n0 + li : p.Ncols - 1;
  const int64_t qoff = (erow + nA) * p.wpr;
  int64_t soff[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) soff[r] = (erow + (NV ? nA : (n0 + 4 * kg + r < p.Ncols ? n0 + 4 * kg + r : p.Ncols - 1))) * p.gpr;
  const uint32_t nvsel = (kg >> 1) ? 0x03030101u : 0x02020000u;   // bytes (h, h, 2 + h, 2 + h) of a scale word: this lane's group of two steps
  const MXProj* const proj[2] = {&p.w0, &p.w1};

  uint32_t wc[NI][4][WPL], wn[NI][4][WPL], cs[NI][SW], ns[NI][SW];
  auto issue = [&](const int run, uint32_t (&w)[NI][4][WPL], uint32_t (&s)[NI][SW]) {
#pragma unroll
    for (int im = 0; im < NI; ++im) {
#pragma unroll
      for (int st = 0; st < 4; ++st) {
        const int wi = (4 * run + st) * BITS + kg * WPL;   // a step is BITS words of the row
        if (wi + WPL <= p.wpr) load_words<WPL>(proj[im]->q + qoff + wi, w[im][st]);   // past the row's end (a last half step, a run's missing steps): zeros
        else
#pragma unroll
          for (int i = 0; i < WPL; ++i) w[im][st][i] = 0u;
      }
#pragma unroll
      for (int r = 0; r < SW; ++r)
        s[im][r] = NV ? load_scale_word(proj[im]->sc + soff[0], 8 * run + 4 * r, p.gpr, p.wide) : load_scale_word(proj[im]->sc + soff[r], 4 * run, p.gpr, p.wide);
    }
  };
  int run = kp;
  if (run < p.nruns) issue(run, wc, cs);

  f32x4 acc[NI][2];
#pragma unroll
  for (int im = 0; im < NI; ++im) acc[im][0] = acc[im][1] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int r0 = 0; r0 < p.nruns; r0 += p.rc) {
    const int rcn = p.nruns - r0 < p.rc ? p.nruns - r0 : p.rc, kc8 = rcn * (kRunK / 8);
    __syncthreads();   // src_row is written; the previous chunk's readers are done
    // ---- stage whole runs (columns past Kdim are zeros): 16 rows x consecutive 8-column fragments (16 lanes write 256 contiguous bytes)
    for (int f = tid; f < RB * kc8; f += 256) {
      const int rest = f >> 4, c8 = rest % kc8, row = (rest / kc8) * 16 + (f & 15), sr = src_row[row], k = r0 * kRunK + 8 * c8;
      float4 u = make_float4(0.f, 0.f, 0.f, 0.f), v = u;
      if (sr >= 0 && k < p.Kdim) {   // Kdim is a multiple of 16: a fragment is inside the row or past it
        const float* xp = p.a + (int64_t)sr * p.lda + k;
        u = *(const float4*)xp; v = *(const float4*)(xp + 4);
      }
      uint4 hi, lo;
      split_hi_lo<true>(u.x, u.y, hi.x, lo.x);
      split_hi_lo<true>(u.z, u.w, hi.y, lo.y);
      split_hi_lo<true>(v.x, v.y, hi.z, lo.z);
      split_hi_lo<true>(v.z, v.w, hi.w, lo.w);
      const int piece = c8 * RB + row;   // c8 = (run, step, kg)
      planes[piece] = hi;
      planes[img + piece] = lo;
    }
    __syncthreads();
    // ---- this wave's runs inside the chunk
    for (; run < r0 + rcn; run += 2) {
      if (run + 2 < p.nruns) issue(run + 2, wn, ns);
#pragma unroll
      for (int st = 0; st < 4; ++st) {
        if (4 * run + st < p.nsteps) {
          const int p0 = (((run - r0) * 4 + st) * 4 + kg) * RB + li;
          uint4 A[NI];
          float sc[NI][4];
#pragma unroll
          for (int im = 0; im < NI; ++im) {
            A[im] = mx_operand<BITS>(wc[im][st]);
            if constexpr (NV) {
              const uint32_t pair = __builtin_amdgcn_perm(cs[im][st >> 1], cs[im][st >> 1], nvsel);
              A[im] = operand_scaled(A[im], (st & 1) ? __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(pair, 1.f, true))
                                                     : __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(pair, 1.f, false)));
            } else {
#pragma unroll
              for (int r = 0; r < 4; ++r) sc[im][r] = e8m0_f32((cs[im][r] >> (8 * st)) & 255u);
            }
          }
#pragma unroll
          for (int mt = 0; mt < 2; ++mt) {
            if (mt < mtiles) {
              const uint4 xh = planes[p0 + mt * 16], xl = planes[img + p0 + mt * 16];
#pragma unroll
              for (int im = 0; im < NI; ++im) {
                if constexpr (NV) {
                  acc[im][mt] = mfma_16x16x32<true>(A[im], xh, acc[im][mt]);
                  acc[im][mt] = mfma_16x16x32<true>(A[im], xl, acc[im][mt]);
                } else {
                  f32x4 accg = f32x4{0.f, 0.f, 0.f, 0.f};
                  accg = mfma_16x16x32<true>(A[im], xh, accg);
                  accg = mfma_16x16x32<true>(A[im], xl, accg);
#pragma unroll
                  for (int r = 0; r < 4; ++r) acc[im][mt][r] = fmaf(sc[im][r], accg[r], acc[im][mt][r]);   // lane = input row mt 16 + li, column n0 + 4 kg + r
                }
              }
            }
          }
        }
      }
#pragma unroll
      for (int im = 0; im < NI; ++im) {
#pragma unroll
        for (int st = 0; st < 4; ++st)
#pragma unroll
          for (int i = 0; i < WPL; ++i) wc[im][st][i] = wn[im][st][i];
#pragma unroll
        for (int r = 0; r < SW; ++r) cs[im][r] = ns[im][r];
      }
    }
  }
  // ---- K part 1 hands its sums to part 0 over the images (every reader is done): part 0 + part 1
  __syncthreads();
  float* join = (float*)planes;   // [c][stream][row block][register][lane]: 2 NI 2 4 64 floats, at most 8 KiB of the 16 KiB the launch always has
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
#define MQX_UNSUPPORTED(cond, ...)       \
  do {                                   \
    if (cond) {                          \
      mi355_set_error(__VA_ARGS__);      \
      return MI355_ERR_UNSUPPORTED;      \
    }                                    \
  } while (0)

int mxproj_check(const char* name, const void* q, const void* sc, int qmode, int Kdim) {
  MQX_UNSUPPORTED(qmode != MI355_QMODE_MXFP4 && qmode != MI355_QMODE_NVFP4 && qmode != MI355_QMODE_MXFP8,
                  "moe_qglu_mx: %s qmode = %d is not built (mxfp4 = 1, nvfp4 = 2 and mxfp8 = 3 are)", name, qmode);
  const int g = qmode == MI355_QMODE_NVFP4 ? 16 : 32;
  MQX_UNSUPPORTED(Kdim < g || Kdim % g != 0, "moe_qglu_mx: %s Kdim = %d is not a multiple of %d", name, Kdim, g);
  MI355_REQUIRE(q && sc, "moe_qglu_mx: null tensor (%s codes or scales)", name);
  MI355_REQUIRE(aligned16(q), "moe_qglu_mx: %s codes must be 16-byte aligned", name);
  return MI355_OK;
}

template <int MODE>
void mxtile_launch_m(const MXTileArgs& t, bool glu, dim3 grid, int lds, hipStream_t st) {
  if (glu) hipLaunchKernelGGL((moe_qtile_mx_kernel<MODE, true>), grid, dim3(256), lds, st, t);
  else hipLaunchKernelGGL((moe_qtile_mx_kernel<MODE, false>), grid, dim3(256), lds, st, t);
}

// one tile launch over [E, Ncols, Kdim] in qmode: fills the format-dependent fields of t
void mxtile_launch(MXTileArgs t, int qmode, int Kdim, bool glu, int max_tiles, hipStream_t st) {
  const int bits = mode_bits(qmode), g = qmode == MI355_QMODE_NVFP4 ? 16 : 32;
  t.Kdim = Kdim;
  t.wpr = Kdim / 8 * (bits / 4);
  t.gpr = Kdim / g;
  t.nsteps = (Kdim + 31) / 32;
  t.nruns = (Kdim + kRunK - 1) / kRunK;
  t.rc = t.nruns < kChunkRuns ? t.nruns : kChunkRuns;
  t.wide = t.gpr % 4 == 0 && (((uintptr_t)t.w0.sc) & 3) == 0 && (!glu || (((uintptr_t)t.w1.sc) & 3) == 0);
  const int lds = TILE * t.rc * kRunK * 4;   // hi + lo images of 32 rows: 16 KiB a run (the join of 8 KiB at most lies over them)
  const dim3 grid((unsigned)max_tiles, (unsigned)((t.Ncols + QCOLS - 1) / QCOLS));
  if (qmode == MI355_QMODE_MXFP4) mxtile_launch_m<MI355_QMODE_MXFP4>(t, glu, grid, lds, st);
  else if (qmode == MI355_QMODE_NVFP4) mxtile_launch_m<MI355_QMODE_NVFP4>(t, glu, grid, lds, st);
  else mxtile_launch_m<MI355_QMODE_MXFP8>(t, glu, grid, lds, st);
}

}  // namespace

extern "C" int mi355_moe_qglu_mx(const mi355_moe_qglu_mx_args* ap, void* stream) {
  MI355_REQUIRE(ap && ap->x && ap->out, "moe_qglu_mx: null tensor");
  const mi355_moe_qglu_mx_args a = *ap;
  MI355_REQUIRE(a.mode == 0 || a.mode == 1, "moe_qglu_mx: unknown mode %d", a.mode);
  MQX_UNSUPPORTED(a.E > MI355_MOE_MAX_EXPERTS, "moe_qglu_mx: E = %d is above MI355_MOE_MAX_EXPERTS = %d", a.E, MI355_MOE_MAX_EXPERTS);
  if (const int rc = mxproj_check("gate", a.q_gate, a.s_gate, a.qmode_gate, a.D)) return rc;
  if (a.mode == 0) {
    MQX_UNSUPPORTED(a.qmode_up != a.qmode_gate, "moe_qglu_mx: gate and up must share one mode (gate: qmode = %d; up: qmode = %d)", a.qmode_gate, a.qmode_up);
    if (const int rc = mxproj_check("up", a.q_up, a.s_up, a.qmode_up, a.D)) return rc;
    if (const int rc = mxproj_check("down", a.q_down, a.s_down, a.qmode_down, a.I)) return rc;
  }
  Layout L;
  if (const int rc = moe_workspace_check("moe_qglu_mx", a.N, a.k, a.E, a.D, a.I, a.workspace, a.workspace_bytes, &L)) return rc;
  MI355_REQUIRE(a.D % 4 == 0 && a.I % 4 == 0, "moe_qglu_mx: D = %d and I = %d must be multiples of 4", a.D, a.I);
  const int out_cols = a.mode == 1 ? a.I : a.D;
  MI355_REQUIRE(a.ldx >= a.D && a.ldx % 4 == 0 && aligned16(a.x) && a.ldo >= out_cols && a.ldo % 4 == 0 && aligned16(a.out),
                "moe_qglu_mx: misaligned rows (x and out rows must be 16-byte aligned and at least D / %d wide)", out_cols);
  if (a.mode == 0) {
    MI355_REQUIRE(a.weights, "moe_qglu_mx: null tensor (weights)");
    MI355_REQUIRE(!a.shared || (a.ld_shared >= a.D && a.ld_shared % 4 == 0 && aligned16(a.shared)), "moe_qglu_mx: misaligned rows (shared)");
    MI355_REQUIRE(!a.res || (a.ld_res >= a.D && a.ld_res % 4 == 0 && aligned16(a.res)), "moe_qglu_mx: misaligned rows (res)");
  }
  char* ws = (char*)a.workspace;
  float* h = (float*)(ws + L.h);
  float* y = (float*)(ws + L.y);
  MXTileArgs t{};
  t.a = a.x; t.lda = a.ldx; t.perm = (const int32_t*)(ws + L.perm); t.kdiv = a.k; t.gather = 1; t.tiles = (const int4*)(ws + L.tiles);
  t.w0 = MXProj{a.q_gate, a.s_gate, a.b_gate}; t.Ncols = a.I;
  MI355_CLEAR_ERROR();
  if (a.mode == 1) {
    t.scatter = 1; t.out = a.out; t.ldo = a.ldo;
    mxtile_launch(t, a.qmode_gate, a.D, false, (int)L.max_tiles, (hipStream_t)stream);
    MI355_LAUNCH_CHECK("moe_qglu_mx (linear)");
    return MI355_OK;
  }
  t.scatter = 0; t.w1 = MXProj{a.q_up, a.s_up, a.b_up}; t.out = h; t.ldo = a.I;
  mxtile_launch(t, a.qmode_gate, a.D, true, (int)L.max_tiles, (hipStream_t)stream);
  MXTileArgs d = t;
  d.a = h; d.lda = a.I; d.gather = 0; d.scatter = 1; d.w0 = MXProj{a.q_down, a.s_down, a.b_down}; d.w1 = MXProj{};
  d.Ncols = a.D; d.out = y; d.ldo = a.D;
  mxtile_launch(d, a.qmode_down, a.I, false, (int)L.max_tiles, (hipStream_t)stream);
  moe_combine_launch(y, a.weights, a.N, a.k, a.D, a.shared, a.ld_shared, a.res, a.ld_res, a.out, a.ldo, (hipStream_t)stream);
  MI355_LAUNCH_CHECK("moe_qglu_mx");
  return MI355_OK;
}
