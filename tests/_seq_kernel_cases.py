"""TEST INFRASTRUCTURE shared by tests/test_seq_kernel_edges_gpu.py and tests/test_seq_kernel_refs_cpu.py: the reference statements of the recurrence and
search kernels (csrc/lstm.hip, csrc/lstm_seq.hip with the LSTM epilogue of csrc/gemm_rows.hip, mi355_aa_activation of csrc/glue.hip, csrc/rvq.hip), each
written from the formulas of include/mi355audio.h and evaluated in whatever dtype the caller asks for, the case tables, the seeded input builders and the
deliberately wrong variants ("mutants") of every statement.  The CPU file holds the statements to known-good implementations, asserts every case
precondition and shows that each mutant misses the bar of the case it is evaluated on.  CPU only: nothing here touches ``mlx_audio_amd.ops`` (the
weight generator of the Kokoro synthetic checkpoint is plain torch)."""
import math

import torch

from mlx_audio_amd.tts.models.kokoro.synthetic import _Gen

F16_SUB = 2.0 ** -24   # the spacing of IEEE-half subnormals: the absolute floor of one rounding to half


def bf16r(t):
    return t.to(torch.bfloat16).to(torch.float32)


def f16r(t):
    return t.to(torch.float16).to(torch.float32)


def bar_of(ref64, ref32):
    """(e32, peak, bar) of one comparison: bar = 4 * e32 + 1e-6 * peak (docs/PARITY.md, "transform kernels, launch branches")."""
    if ref64.numel() == 0:
        return 0.0, 0.0, 0.0
    e32 = float((ref32.double() - ref64.double()).abs().max())
    peak = float(ref64.abs().max())
    return e32, peak, 4.0 * e32 + 1e-6 * peak


# ----------------------------------------------------------------------------------------------------------------- lstm_bidir
def fq_u8(h):
    """fake_quant_dynamic_u8 of ONE hidden vector (extrema over its H values, joined with 0), in float32 like the reference and the kernel; returned in
    the dtype of ``h``.  Also returns the distance of the closest element from a rounding boundary, in grid steps."""
    x = h.to(torch.float32)
    zero = torch.zeros((), dtype=torch.float32)
    mn, mx = torch.minimum(x.min(), zero), torch.maximum(x.max(), zero)
    scale = (mx - mn) / 255.0
    if float(scale) == 0.0:
        return torch.zeros_like(h), 0.5
    zp = torch.clamp(torch.round(-mn / scale), 0.0, 255.0)
    pos = x / scale + zp
    q = torch.clamp(torch.round(pos), 0.0, 255.0)
    return ((q - zp) * scale).to(h.dtype), float(((pos - torch.floor(pos)) - 0.5).abs().min())


def lstm_bidir_stmt(xp, wh_f, wh_b, lens, dtype, quant_h=False, variant=None, margins=None):
    """out[b, t, d H : (d + 1) H] = h_t of direction d (0 forward over t = 0 .. len - 1, 1 backward over t = len - 1 .. 0, len = lens[b] or L):
    pre = xp[b, t, d 4H : (d + 1) 4H] + Wh_d @ hq, gates i | f | g | o = sigmoid, sigmoid, tanh, sigmoid of the four H-blocks of pre,
    c = f c + i g, h = o tanh(c); hq = h of the previous step, or fq_u8(h) with ``quant_h`` (the emitted h is not quantised); h = c = 0 at the start of
    every (direction, item).  Rows >= len stay zero.  ``wh_*`` [4H, H] hold exactly the 16-bit values of the image.
    Mutants (``variant``): "fo_swap" (f and o gates exchanged), "start_L" (the backward pass walks L - 1 .. L - len), "carry" (h and c of item b enter
    item b + 1), "quant_emit" (the emitted h is the quantised one)."""
    B, L, H8 = xp.shape
    H = H8 // 8
    out = torch.zeros(B, L, 2 * H, dtype=dtype)
    for d, wh in enumerate((wh_f, wh_b)):
        w = wh.to(dtype)
        h, c = torch.zeros(H, dtype=dtype), torch.zeros(H, dtype=dtype)
        for b in range(B):
            n = L if lens is None else int(lens[b])
            if variant != "carry":
                h, c = torch.zeros(H, dtype=dtype), torch.zeros(H, dtype=dtype)
            hq = h
            for s in range(n):
                t = s if d == 0 else ((L if variant == "start_L" else n) - 1 - s)
                pre = xp[b, t, d * 4 * H:(d + 1) * 4 * H].to(dtype) + w @ hq
                i, f, g, o = torch.sigmoid(pre[:H]), torch.sigmoid(pre[H:2 * H]), torch.tanh(pre[2 * H:3 * H]), torch.sigmoid(pre[3 * H:])
                if variant == "fo_swap":
                    f, o = o, f
                c = f * c + i * g
                h = o * torch.tanh(c)
                hq = h
                if quant_h:
                    hq, m = fq_u8(h)
                    if margins is not None:
                        margins.append(m)
                out[b, t, d * H:(d + 1) * H] = hq if variant == "quant_emit" else h
    return out


def lstm_weights(H, seed, image):
    """(Wh_forward, Wh_backward) [4H, H], uniform in +-1 / sqrt(H), holding exactly the values of ``image``: "bf16" or "f16"."""
    g = torch.Generator().manual_seed(1000 * H + seed)
    rnd = bf16r if image == "bf16" else f16r
    s = 1.0 / math.sqrt(H)
    return tuple(rnd((torch.rand(4 * H, H, generator=g) * 2 - 1) * s) for _ in range(2))


LSTM_H = [32, 64, 128, 256]
LSTM_IMAGES = ["bf16", "f16", "scaled"]   # "scaled": the bf16 values as a half image times a power of two: bit-equal to "bf16"
LSTM_RAGGED_L = 9
LSTM_RAGGED = [LSTM_RAGGED_L, 1, 0, LSTM_RAGGED_L - 1, 2]


def lstm_shapes():
    """(name, B, L, lens): L = 1 (both directions at t = 0), 2, 7, 8 without lens (the ``lens == NULL -> L`` branch); the ragged batch of five with a
    full item, lens 1, lens 0, L - 1 and 2; nine items (more workgroups than the 2 x 8 of any other case) with lens that repeat."""
    return [(f"L{L}", 2, L, None) for L in (1, 2, 7, 8)] + [("ragged", 5, LSTM_RAGGED_L, LSTM_RAGGED), ("B9", 9, 3, [3, 1, 2, 3, 0, 3, 2, 1, 3])]


def lstm_xp(H, B, L, seed):
    """Gate pre-activations [B, L, 8H] of unit variance (what x @ Wx^T + b gives the text encoder)."""
    return torch.randn(B, L, 8 * H, generator=torch.Generator().manual_seed(77 * H + 13 * L + B + seed))


# quant_h, tight form: (H, In, L, seed) of a CPU search; x ~ N(0, 1) from manual_seed(100 + seed), weights _Gen(seed).lstm("l", In, H); the float32
# oracle's smallest distance from a rounding boundary (grid steps) as measured by that search -- re-asserted above QUANT_MARGIN by the CPU file
QUANT_TIGHT = [(32, 48, 12, 3), (64, 96, 10, 2), (128, 40, 5, 2), (256, 64, 4, 1)]
QUANT_MARGIN = 2e-4
QUANT_BAR = 2e-5


def quant_case(H, In, L, seed):
    """(weights dict, x [1, L, In], xp [1, L, 8H] float32, Wh_f, Wh_b): xp = fq(x) @ Wx^T + b_ih + b_hh evaluated in float64 and rounded once to float32,
    so that the statement in every dtype and the kernel start from the same pre-activations."""
    g = _Gen(seed)
    g.lstm("l", In, H)
    w = g.w
    x = torch.randn(1, L, In, generator=torch.Generator().manual_seed(100 + seed))
    xq, _ = fq_u8(x)
    wx = torch.cat([w["l.Wx_forward"], w["l.Wx_backward"]], 0).double()
    b = torch.cat([w["l.bias_ih_forward"].double() + w["l.bias_hh_forward"].double(), w["l.bias_ih_backward"].double() + w["l.bias_hh_backward"].double()])
    xp = (xq.double() @ wx.t() + b).to(torch.float32)
    return w, x, xp, w["l.Wh_forward"], w["l.Wh_backward"]


# ----------------------------------------------------------------------------------------------------------------- lstm_seq
def seq_sigmoid(x):
    """The reference's gate function: 1 / (1 + exp(-|x|)), mirrored for x < 0."""
    y = 1.0 / (1.0 + torch.exp(-x.abs()))
    return torch.where(x < 0, 1.0 - y, y)


def lstm_seq_stmt(xproj, wh, h0, c0, dtype, variant=None, split_width=0.0, split_floor=0.0):
    """pre_t = xproj[:, t] + h_{t-1} @ Wh^T (gate blocks i | f | g | o of H rows each), c_t = f c_{t-1} + i g, h_t = o tanh(c_t), out[:, t] = h_t;
    returns (out [B, T, H], h_T, c_T) and, when ``split_width`` > 0, a fourth value: the first-order bound of what a hi + lo split of h_{t-1} in the
    weights' 16-bit type moves each of the three (see ``seq_split_term``).  Mutants: "no_c0" (c0 ignored), "stride" (gate block g read at row
    g (H + 1) of Wh and column g (H + 1) of xproj)."""
    B, T, H4 = xproj.shape
    H = H4 // 4
    w = wh.to(dtype)
    h = torch.zeros(B, H, dtype=dtype) if h0 is None else h0.to(dtype).clone()
    c = torch.zeros(B, H, dtype=dtype) if c0 is None or variant == "no_c0" else c0.to(dtype).clone()
    st = H + 1 if variant == "stride" else H
    rows = torch.cat([(g * st + torch.arange(H)).clamp(max=4 * H - 1) for g in range(4)])
    aw = w.abs()
    dh, dc = torch.zeros(B, H, dtype=dtype), torch.zeros(B, H, dtype=dtype)
    out, dout = [], []
    for t in range(T):
        pre = (xproj[:, t].to(dtype) + h @ w.t())[:, rows]
        i, f, g, o = seq_sigmoid(pre[:, :H]), seq_sigmoid(pre[:, H:2 * H]), torch.tanh(pre[:, 2 * H:3 * H]), seq_sigmoid(pre[:, 3 * H:])
        if split_width > 0.0:
            dpre = (torch.clamp(split_width * h.abs(), min=split_floor) + dh) @ aw.t()
            di, df, dg, do = i * (1 - i) * dpre[:, :H], f * (1 - f) * dpre[:, H:2 * H], (1 - g * g) * dpre[:, 2 * H:3 * H], o * (1 - o) * dpre[:, 3 * H:]
            dc = f * dc + c.abs() * df + g.abs() * di + i * dg
        c = f * c + i * g
        th = torch.tanh(c)
        if split_width > 0.0:
            dh = th.abs() * do + o * (1 - th * th) * dc
            dout.append(dh)
        h = o * th
        out.append(h)
    res = (torch.stack(out, 1), h, c)
    return res + ((torch.stack(dout, 1), dh, dc),) if split_width > 0.0 else res


def seq_route(B, H, fused):
    """Which arithmetic a step's product runs on: "mfma" (the matrix pipe: gemm_rows in the one-launch form at any B and in the two-launch form from 9
    rows on, gemv_mfma at 5 .. 8 rows with H % 64 == 0 and H <= 2048) or "fma" (the fp32 GEMV kernels: h enters the product unsplit)."""
    if fused or B >= 9:
        return "mfma"
    return "mfma" if (5 <= B <= 8 and H % 64 == 0 and H <= 2048) else "fma"


def seq_split_term(f16):
    """(width, floor) of the hi + lo split of h on the matrix-pipe routes (csrc/linear_common.h split_hi_lo: hi = round16(h), lo = round16(h - hi)): what is
    left of h is one rounding of lo, |lo| <= 2^-8 |h| (bf16: 8 significant bits) or 2^-11 |h| (half: 11), so at most 2^-8 * 2^-8 = 2^-16 |h| resp.
    2^-11 * 2^-11 = 2^-22 |h| -- and, for half only, one subnormal spacing of 2^-24 where that is more: lo falls into half's subnormal range from
    |h| < 2^-3 on (bf16 has float32's exponent range: no floor)."""
    return (2.0 ** -22, F16_SUB) if f16 else (2.0 ** -16, 0.0)


def _seq(H, B, T, image, fused, tag="", h0=False, view=False):
    return dict(H=H, B=B, T=T, image=image, fused=fused, tag=tag, h0=h0, view=view)


def seq_cases():
    """- H 8 / 24 / 72 / 200 x B 1 / 4 / 8 x both images: H % 64 != 0 has only the two-launch form (GEMV kernels with K = 8 .. 200);
    - H = 64, B 8 | 9 (GEMV kernels | gemm_rows in the two-launch form), 16 | 17 and 32 | 33 (MR = 1 | 2 | 4), 64; both forms, both images;
    - B = 33, H = 320: KC = 256 at MR = 4, so the second K chunk holds 64 of its 256 columns; both forms;
    - H = 2112, B = 2 and 33, T = 2, one-launch form, half: 528 tiles on 512 workgroups -- a second tile-group pass (and at B = 33, T = 2 tiles per
      workgroup: tile j = 1 valid in the first pass, absent in the second);
    - T 1 / 2 / 5 (odd: the final state comes back from the scratch buffer of the one-launch form);
    - non-zero h0 / c0 in both forms; xproj and out as column views with padded batch strides."""
    cases = []
    for H in (8, 24, 72, 200):
        for B in (1, 4, 8):
            for image in ("bf16", "f16"):
                cases.append(_seq(H, B, 3, image, False, h0=(B == 4), view=(B == 8)))
    for B in (8, 9, 16, 17, 32, 33, 64):
        for image in ("bf16", "f16"):
            for fused in (True, False):
                cases.append(_seq(64, B, 3, image, fused, h0=(B in (9, 33)), view=(B in (8, 17))))
    for fused in (True, False):
        cases.append(_seq(320, 33, 2, "f16", fused, tag="chunk-tail"))
        cases.append(_seq(320, 33, 2, "bf16", fused, tag="chunk-tail"))
    cases.append(_seq(2112, 2, 2, "f16", True, tag="second-pass"))
    cases.append(_seq(2112, 33, 2, "f16", True, tag="second-pass", h0=True))
    for T in (1, 2, 5):
        for fused in (True, False):
            cases.append(_seq(64, 3, T, "f16", fused, tag="steps", h0=True, view=True))
    return cases


def seq_id(c):
    return f"H{c['H']}-B{c['B']}-T{c['T']}-{c['image']}-{'one' if c['fused'] else 'two'}" + ("-h0" if c["h0"] else "") + ("-view" if c["view"] else "") + \
        (f"-{c['tag']}" if c["tag"] else "")


def seq_inputs(c):
    """(Wh [4H, H] holding the image's values, xproj [B, T, 4H], h0, c0 or None)."""
    H, B, T = c["H"], c["B"], c["T"]
    g = torch.Generator().manual_seed(7 * H + 31 * B + T + (1 if c["image"] == "f16" else 0))
    rnd = f16r if c["image"] == "f16" else bf16r
    wh = rnd(torch.randn(4 * H, H, generator=g) / math.sqrt(H))
    xproj = torch.randn(B, T, 4 * H, generator=g)
    h0 = c0 = None
    if c["h0"]:
        h0 = torch.tanh(torch.randn(B, H, generator=g))
        c0 = torch.randn(B, H, generator=g)
    return wh, xproj, h0, c0


# (name, match of mi355_last_error, overrides of a valid B = 2, T = 2, H = 64 call)
SEQ_REFUSALS = [
    ("B9-H72", "more than 8 sequences", dict(B=9, H=72)),
    ("H12", "multiple of 8", dict(H=12)),
    ("B65", r"1\.\.64 sequences", dict(B=65)),
    ("interleaved-without-h2", "h2 scratch", dict(gate_interleaved=1, h2=None)),
    ("ld_out<H", "bad strides", dict(ld_out_short=True)),
]


# ----------------------------------------------------------------------------------------------------------------- aa_activation
def aa_activation_stmt(x, fu, fd, alpha, inv_beta, lens, dtype, variant=None):
    """Per item on its first n = lens[b] rows (x [B, L, C] channels-last; rows >= n of the result stay zero), with clamp(i) = min(max(i, 0), size - 1):
      u[m] = 2 * sum over the k of the parity of m + 15 of fu[k] * x[clamp((m + 15 - k) / 2 - 5)],   m in [0, 2n)   (edge pad 5, transposed 12-tap
             conv at stride 2, x 2, 15 trimmed on each side)
      a[m] = u[m] + inv_beta[c] * sin(alpha[c] * u[m])^2
      y[t] = sum_k fd[k] * a[clamp(2 t + k - 5)],   t in [0, n)                                                  (edge pad 5 / 6, stride 2)
    Mutants: "zero_pad" (samples outside [0, size) are zero instead of the edge sample), "phase" (the taps' parity taken from m instead of m + 15)."""
    B, L, C = x.shape
    y = torch.zeros(B, L, C, dtype=dtype)
    fu, fd, al, ib = fu.to(dtype), fd.to(dtype), alpha[:C].to(dtype), inv_beta[:C].to(dtype)
    zero = torch.zeros((), dtype=dtype)
    for b in range(B):
        n = L if lens is None else int(lens[b])
        if n == 0:
            continue
        xb = x[b, :n].to(dtype)

        def take(v, idx):
            rows = v[idx.clamp(0, v.shape[0] - 1)]
            return torch.where(((idx >= 0) & (idx < v.shape[0]))[:, None], rows, zero) if variant == "zero_pad" else rows

        m = torch.arange(2 * n)
        par = (m if variant == "phase" else m + 15) & 1
        u = torch.zeros(2 * n, C, dtype=dtype)
        for q in range(6):
            k = par + 2 * q
            u = u + fu[k][:, None] * take(xb, torch.div(m + 15 - k, 2, rounding_mode="floor") - 5)
        u = u * 2
        a = u + ib * torch.sin(al * u) ** 2
        t = torch.arange(n)
        acc = torch.zeros(n, C, dtype=dtype)
        for k in range(12):
            acc = acc + fd[k] * take(a, 2 * t + k - 5)
        y[b, :n] = acc
    return y


def aa_filter():
    from oracle.bigvgan_ref import kaiser_sinc_filter1d

    return kaiser_sinc_filter1d(0.25, 0.3, 12)


# C -> (CT, rows per workgroup T) as mi355_aa_activation picks them
AA_CLASSES = {4: (8, 512), 24: (8, 512), 48: (16, 256), 96: (32, 128), 12: (64, 64), 136: (64, 64)}


def aa_tile(C):
    """The dispatch of mi355_aa_activation restated: CT = 64 for C % 64 == 0 or C > 128, else the widest of 32 / 16 / 8 that divides C, 8 for C < 8,
    64 otherwise; T = 4096 / CT."""
    if C % 64 == 0 or C > 128:
        ct = 64
    elif C % 32 == 0:
        ct = 32
    elif C % 16 == 0:
        ct = 16
    elif C % 8 == 0 or C < 8:
        ct = 8
    else:
        ct = 64
    return ct, 4096 // ct


def aa_cases():
    """Per dispatch class (C = 4: CT 8 with four dead lanes per row; 24: CT 8; 48: CT 16; 96: CT 32; 12: the CT 64 fallback; 136: CT 64 with a ragged
    third channel tile): full-length items at T - 1, T, T + 1 (and 2 T + 2 for CT 64) rows, and one ragged batch [T + 1, T, 1, 2 T] in a [4, 2 T] tensor
    -- a length on the tile boundary (the second tile returns early), T + 1 (a one-row last tile, clamped on both sides), 1, and two full tiles."""
    cases = []
    for C, (ct, T) in AA_CLASSES.items():
        for L in (T - 1, T, T + 1) + ((2 * T + 2,) if ct == 64 else ()):
            cases.append(dict(C=C, B=1, L=L, lens=None))
        cases.append(dict(C=C, B=4, L=2 * T, lens=[T + 1, T, 1, 2 * T]))
    return cases


def aa_id(c):
    return f"C{c['C']}-B{c['B']}-L{c['L']}" + ("-ragged" if c["lens"] else "")


def aa_inputs(c):
    """x [B, L, C] of scale 1.5, alpha and beta = exp(0.3 N(0, 1)) (the reference's log-scale parameters), inv_beta = 1 / (beta + 1e-9)."""
    g = torch.Generator().manual_seed(3 * c["C"] + c["L"] + c["B"])
    x = torch.randn(c["B"], c["L"], c["C"], generator=g) * 1.5
    alpha = torch.exp(torch.randn(c["C"], generator=g) * 0.3)
    beta = torch.exp(torch.randn(c["C"], generator=g) * 0.3)
    return x, alpha, 1.0 / (beta + 1e-9)


DELTA_SIN = 1e-6     # csrc/glue.hip: "~1e-6 absolute, as in the conv prologues"


def aa_sine_term(fd, inv_beta):
    """What a sine that is off by DELTA_SIN moves an output: d/ds of inv_beta * s^2 is at most 2 inv_beta, and an output sums 12 activated samples."""
    return float(fd.double().abs().sum()) * 2.0 * inv_beta.double() * DELTA_SIN


# ----------------------------------------------------------------------------------------------------------------- rvq_encode
def rvq_stmt(x, tables, c2, dtype, variant=None):
    """Per layer l: score[b] = c2[l, b] - r . tables[l, b], code = the FIRST b at which the score is smallest, r <- r - tables[l, code]; r starts as x.
    Returns (codes int64 [rows, n], gaps [rows, n] = smallest score among the OTHER bins - best score: 0 at an exact tie, max|score| per layer [n]).
    Mutant: "last" (the last minimum wins)."""
    r = x.to(dtype).clone()
    n, bins, _ = tables.shape
    ar = torch.arange(bins)[None, :]
    codes, gaps, peaks = [], [], []
    for l in range(n):
        e = tables[l].to(dtype)
        s = c2[l].to(dtype)[None, :] - r @ e.t()
        best = s.min(1, keepdim=True).values
        hit = s == best
        idx = torch.where(hit, ar, -1).max(1).values if variant == "last" else torch.where(hit, ar, bins).min(1).values
        other = s.masked_fill(ar == idx[:, None], float("inf"))
        codes.append(idx)
        gaps.append(other.min(1).values - best[:, 0])
        peaks.append(s.abs().max())
        r = r - e[idx]
    return torch.stack(codes, 1), torch.stack(gaps, 1), torch.stack(peaks)


RVQ_THR = 1e-4      # a decision is compared when its float64 gap is at least RVQ_THR * max|score| of its layer (tests/test_codec_encode_gpu.py's rule)
RVQ_CAP = 0.02      # at most this share of a case's decisions may go uncompared


def rvq_compared(gaps64, peaks64):
    """[rows, n] bool: the decisions of a frame, in layer order, up to (not including) the first whose float64 gap is below the threshold."""
    clear = gaps64 >= RVQ_THR * peaks64[None, :]
    return torch.cumprod(clear.to(torch.int64), dim=1).bool()


def _rvq(name, rows, D, bins, kind="random", view=False, chunks=False):
    return dict(name=name, rows=rows, D=D, bins=bins, layers=2, kind=kind, view=view, chunks=chunks)


# duplicated codewords of the tie table (bins = 600; thread = b % 256, wave = thread / 64): (copies, the merge in which they meet)
RVQ_TIES = [((10, 266), "thread"), ((70, 100), "wave"), ((5, 200), "block"), ((33, 289, 450), "triple")]


# bins of the narrow-D cases: 64 codewords on a line or in space lie so close together that most decisions fall under the threshold whatever the
# seed (D = 1: 71 % of them), so the tables of D = 1 / 3 hold as many codewords as keep the float64 statement inside RVQ_CAP
RVQ_NARROW_BINS = {1: 4, 3: 16, 6: 64, 516: 64}


def rvq_cases():
    """- bins 2 / 63 / 64 / 65 / 100 / 256 / 257 / 1000 at D = 8 (threads without a bin, a partly filled wave, one bin into the second round of a thread);
    - "ties": rows that ARE a duplicated codeword (RVQ_TIES), alone (the one-frame kernel) and as the first and the last four of 2050 rows (R = 4: the
      merges of the several-frames kernel; the last two sit in a workgroup with ``nr`` = 2);
    - D 1 / 3 / 6 / 516 with x a [:, :D] view of a [rows, D + 1] buffer at 1025 and 4097 rows: the one-frame kernel whatever the row count (``!can``);
    - rows 1023 / 1024 / 1025, 2047 / 2049, 4095 / 4097 at D = 8, bins = 64: the R = 1 | 2 | 4 | 8 switches with ``nr < R`` tails;
    - D = 8 on an ``ldx = 9`` view at 1025 rows: ``ldx % 4 != 0`` alone sends a call that would take R = 2 to the one-frame kernel."""
    cases = [_rvq(f"bins{b}", 37, 8, b) for b in (2, 63, 64, 65, 100, 256, 257, 1000)]
    cases.append(_rvq("ties", len(RVQ_TIES), 8, 600, kind="ties"))
    cases.append(_rvq("ties-rows2050", 2050, 8, 600, kind="ties", chunks=True))
    cases += [_rvq(f"D{D}-rows{rows}", rows, D, RVQ_NARROW_BINS[D], view=True, chunks=True) for D in (1, 3, 6, 516) for rows in (1025, 4097)]
    cases += [_rvq(f"rows{rows}", rows, 8, 64, chunks=True) for rows in (1023, 1024, 1025, 2047, 2049, 4095, 4097)]
    cases.append(_rvq("D8-ldx9-rows1025", 1025, 8, 64, view=True, chunks=True))
    return cases


# name -> seed where the default (500 + the position in rvq_cases) leaves more than RVQ_CAP of the decisions under the threshold (searched upwards
# from 600 on the CPU: with four codewords on a line the share hangs on where the two nearest of them fall)
RVQ_SEEDS = {"D1-rows4097": 600}


def rvq_inputs(c):
    """(x [rows, D], tables [2, bins, D], c2 [2, bins] = |e|^2 / 2 in float32).  The second layer's table is a quarter the size of the first's, like a
    trained residual quantiser's."""
    names = [k["name"] for k in rvq_cases()]
    g = torch.Generator().manual_seed(RVQ_SEEDS.get(c["name"], 500 + names.index(c["name"])))
    D, bins = c["D"], c["bins"]
    tables = torch.randn(2, bins, D, generator=g) * torch.tensor([1.0, 0.25])[:, None, None]
    if c["kind"] == "ties":
        for copies, _ in RVQ_TIES:
            for b in copies[1:]:
                tables[0, b] = tables[0, copies[0]]
        tie = torch.stack([tables[0, copies[0]] for copies, _ in RVQ_TIES]).clone()
        x = torch.randn(c["rows"], D, generator=g) * 1.5
        x[:len(RVQ_TIES)] = tie
        x[-len(RVQ_TIES):] = tie
    else:
        x = torch.randn(c["rows"], D, generator=g) * 1.5
    c2 = (tables * tables).sum(-1) * 0.5
    return x, tables, c2
