"""TEST INFRASTRUCTURE shared by tests/test_lm_row_kernel_edges_gpu.py and tests/test_lm_row_refs_cpu.py: the reference statements of the row kernels of
csrc/transformer.hip (each written from the formulas of include/mi355audio.h, evaluated in whatever dtype the caller asks for) and the case tables of
the depthwise conv and of the sampler, with the sampler's input preconditions.  The CPU file holds the statements to known-good implementations and
asserts the preconditions of every sampler case, so a failure of the GPU file cannot be the reference's or the inputs' fault.  CPU only: nothing
here touches ``mlx_audio_amd.ops``."""
import math

import torch
import torch.nn.functional as F

from oracle import sampling_ref as R
from oracle.lm_ref import apply_rope
from test_lm_kernels_gpu import SAMPLE_CASES   # the reference's parameter sets: one table for both sampler files

THR = 1e-3     # tests/_margin.py THR: the smallest top-2 gap at which two float32 builds must pick the same token
P_MARGIN = 1e-4  # distance of every cumulative probability / log-probability from its threshold (float64)


# ----------------------------------------------------------------------------------------------------------------- statements
def rmsnorm_stmt(x, w, eps, dtype):
    """y = x * rsqrt(mean(x^2) + eps) * weight over the channel axis."""
    x = x.to(dtype)
    y = x * torch.rsqrt((x * x).mean(-1, keepdim=True) + eps)
    return y if w is None else y * w.to(dtype)


def rope_positions(B, L, rope_rows, pos=None, pos0=0, pos_sub=None):
    """position of row l = (pos ? pos[b, l] : pos0 + l) - (pos_sub ? pos_sub[b] : 0), clamped to the rows of the tables."""
    p = pos[:, :L].long() if pos is not None else (pos0 + torch.arange(L))[None, :].expand(B, L)
    if pos_sub is not None:
        p = p - pos_sub.long()[:, None]
    return p.clamp(0, rope_rows - 1)


def rope_stmt(x, cos_rows, sin_rows, interleaved):
    """The header's pairs, index by index: rope_mode 0 rotates (i, i + dh/2), rope_mode 1 rotates (2i, 2i + 1); pair (x0, x1) with the angle of
    column i becomes (x0 c - x1 s, x1 c + x0 s).  x [B, L, H, dh]; cos_rows / sin_rows [B, L, dh/2] (one table row per token)."""
    half = x.shape[-1] // 2
    i0 = 2 * torch.arange(half) if interleaved else torch.arange(half)
    i1 = i0 + 1 if interleaved else i0 + half
    c, s = cos_rows[:, :, None, :].to(x.dtype), sin_rows[:, :, None, :].to(x.dtype)
    x0, x1 = x[..., i0], x[..., i1]
    y = torch.empty_like(x)
    y[..., i0] = x0 * c - x1 * s
    y[..., i1] = x1 * c + x0 * s
    return y


def head_norm_rope_ref(x, heads, dh, nw, eps, cos, sin, p, interleaved, dtype):
    """Per-head RMSNorm (``nw`` [dh] or None) then oracle.lm_ref.apply_rope with row p[b, l] of the float32 tables upcast to ``dtype`` (``cos`` None: no
    rotation).  x [B, L, >= heads * dh] -> [B, L, heads * dh]."""
    B, L = x.shape[:2]
    xr = x[:, :, :heads * dh].reshape(B, L, heads, dh).to(dtype)
    if nw is not None:
        xr = xr * torch.rsqrt((xr * xr).mean(-1, keepdim=True) + eps) * nw.to(dtype)
    if cos is not None:
        xr = torch.cat([apply_rope(xr[b:b + 1], cos[p[b]].to(dtype), sin[p[b]].to(dtype), interleaved) for b in range(B)])
    return xr.reshape(B, L, heads * dh)


def swiglu_stmt(x, dtype):
    """y[r, i] = silu(x[r, 2i]) * x[r, 2i + 1], silu(g) = g / (1 + exp(-g))."""
    g, u = x[..., 0::2].to(dtype), x[..., 1::2].to(dtype)
    return g / (1 + torch.exp(-g)) * u


def embed_sum_stmt(table, ids, slot_offset, add, scale, dtype):
    """y[b, l] = scale * (add[b, l] + sum_q table[slot_offset[q] + ids[b, l, q]]) in the kernel's documented order: acc = add (or 0), the slots
    ascending with one add each (ids < 0 skip the slot), then one multiply by scale (0 means 1).  In float32 these are the kernel's IEEE operations."""
    B, L, Q = ids.shape
    C = table.shape[1]
    acc = add.to(dtype).clone() if add is not None else torch.zeros((B, L, C), dtype=dtype)
    for q in range(Q):
        i = ids[:, :, q].long()
        off = int(slot_offset[q]) if slot_offset is not None else 0
        rows = table[i.clamp(min=0) + off].to(dtype)
        acc = torch.where((i >= 0)[:, :, None], acc + rows, acc)
    return acc * torch.tensor(1.0 if scale == 0 else scale, dtype=dtype)


def dwconv_stmt(x, w, bias, *, pad, dil, Lout, lens_in=None, alpha=None, inv=None, dtype=torch.float64):
    """y[b, n, c] = bias[c] + sum_k w[c, k] * snake(x[b, n + k * dil - pad, c]), x zero outside [0, lens_in[b]) (the padding stays zero: snake(0) = 0),
    snake(v) = v + inv[c] * sin(alpha[c] * v)^2, dil 0 meaning 1.  x [B, Lin, C] -> [B, Lout, C]."""
    B, Lin, C = x.shape
    K = w.shape[1]
    dil = dil if dil > 0 else 1
    xd = x.to(dtype)
    if alpha is not None:
        xd = xd + inv.to(dtype) * torch.sin(alpha.to(dtype) * xd) ** 2
    t = torch.arange(Lout)[:, None] + torch.arange(K)[None, :] * dil - pad
    lens = torch.tensor([Lin] * B if lens_in is None else list(lens_in))
    ok = (t >= 0)[None] & (t[None] < lens[:, None, None])
    taps = torch.where(ok[..., None], xd[:, t.clamp(0, Lin - 1)], torch.zeros((), dtype=dtype))   # [B, Lout, K, C]
    y = torch.einsum("blkc,ck->blc", taps, w.to(dtype))
    return y if bias is None else y + bias.to(dtype)


def dwconv_t_stmt(x, w, bias, *, stride, pad, Lout, lens_in=None, dtype=torch.float64):
    """y[b, n, c] = bias[c] + sum over (t, k) with t * stride + k - pad == n of w[c, k] * x[b, t, c], t < lens_in[b]."""
    B, Lin, C = x.shape
    y = torch.zeros((B, Lout, C), dtype=dtype)
    for b in range(B):
        n_in = Lin if lens_in is None else lens_in[b]
        for t in range(n_in):
            for k in range(w.shape[1]):
                n = t * stride + k - pad
                if 0 <= n < Lout:
                    y[b, n] += w[:, k].to(dtype) * x[b, t].to(dtype)
    return y if bias is None else y + bias.to(dtype)


def dwconv_t_ref(x, w, bias, *, stride, pad, Lout, lens_in=None, dtype=torch.float64):
    """F.conv_transpose1d (groups = C) of each item's first lens_in[b] rows, ``pad`` outputs trimmed at the front, padded with zeros or trimmed to Lout."""
    B, Lin, C = x.shape
    out = torch.zeros((B, Lout, C), dtype=dtype)
    for b in range(B):
        n_in = Lin if lens_in is None else lens_in[b]
        if n_in > 0:
            full = F.conv_transpose1d(x[b:b + 1, :n_in].transpose(1, 2).to(dtype), w.to(dtype)[:, None, :], None, stride=stride, groups=C)[0, :, pad:]
            m = min(Lout, full.shape[1])
            out[b, :m] = full[:, :m].transpose(0, 1)
    return out if bias is None else out + bias.to(dtype)


# ----------------------------------------------------------------------------------------------------------------- dwconv cases
def _comb(dil, snake, pad, Lin, Lout, C=40, B=1, lens=None, bias=True, tag="same"):
    return dict(K=7, dil=dil, snake=snake, pad=pad, Lin=Lin, Lout=Lout, C=C, B=B, lens=lens, bias=bias, tag=tag)


def comb_cases():
    """The K = 7 comb path: dil 1 / 3 / 9 x Snake on / off x same-length (pad 3 dil; L = 1, 7, 8 dil, 8 dil + 1, 16 dil + 5: one comb row partly filled,
    exactly filled, one output into the second, two and a part), causal (pad 6 dil), valid (pad 0, Lout = Lin - 6 dil); Lout < dil (phases without an
    output); dil = 0; C = 1 / 64 / 70 (one channel, one wave, a block boundary inside a row); ragged lens_in with a 0 and a length below the padding;
    no bias."""
    cases = []
    for dil in (1, 3, 9):
        for snake in (False, True):
            for L in sorted({1, 7, 8 * dil, 8 * dil + 1, 16 * dil + 5}):
                cases.append(_comb(dil, snake, 3 * dil, L, L))
            L = 16 * dil + 5
            cases.append(_comb(dil, snake, 6 * dil, L, L, tag="causal"))
            cases.append(_comb(dil, snake, 0, L, L - 6 * dil, tag="valid"))
    for snake in (False, True):
        cases.append(_comb(9, snake, 27, 5, 5, tag="Lout<dil"))
        cases.append(_comb(3, snake, 9, 25, 25, C=64, B=3, lens=[25, 0, 2], tag="ragged"))
        cases.append(_comb(1, snake, 3, 9, 9, C=70, B=3, lens=[9, 0, 2], tag="ragged"))
    cases.append(_comb(0, True, 3, 9, 9, tag="dil0"))
    for C in (1, 64, 70):
        cases.append(_comb(3, True, 9, 25, 25, C=C, tag="width"))
    cases.append(_comb(3, True, 9, 25, 25, bias=False, tag="nobias"))
    return cases


def generic_cases():
    """The generic kernel, plain: K 1 / 3 / 5 / 9 x dil 1 / 2 x Snake on / off, same-length padding, B = 2 with lens_in = [13, 4]."""
    return [dict(K=K, dil=dil, snake=snake, pad=(K - 1) // 2 * dil, Lin=13, Lout=13, C=40, B=2, lens=[13, 4], bias=True, tag="generic")
            for K in (1, 3, 5, 9) for dil in (1, 2) for snake in (False, True)]


def transposed_cases(Lin=9):
    """(K, stride, pad, Lout): Mimi's causal upsampler and its untrimmed tail, K = stride, stride 1, a centred k8 s4, and K not a multiple of the stride;
    each with bias and full lengths, and without bias with ragged lens_in (one row and none)."""
    shapes = [(4, 2, 0, 2 * Lin), (4, 2, 0, 2 * Lin + 2), (2, 2, 0, 2 * Lin), (3, 1, 1, Lin), (8, 4, 2, 4 * Lin), (5, 3, 0, 3 * Lin + 2)]
    cases = []
    for K, s, p, Lout in shapes:
        cases.append(dict(K=K, stride=s, pad=p, Lin=Lin, Lout=Lout, C=40, B=2, lens=None, bias=True))
        cases.append(dict(K=K, stride=s, pad=p, Lin=Lin, Lout=Lout, C=70, B=3, lens=[Lin, 1, 0], bias=False))
    return cases


def dwconv_id(c):
    return "-".join(f"{k}{v}" for k, v in c.items() if k not in ("lens", "bias") and v is not False) + ("-ragged" if c.get("lens") else "")


def dwconv_inputs(c):
    """x [B, Lin, C] of unit variance, w [C, K], bias [C], alpha in [0.5, 1.5] and inv = 1 / (alpha + 1e-9) in float32 (|alpha x| stays below 16 rad)."""
    g = torch.Generator().manual_seed(sum((i + 1) * int(v) for i, v in enumerate((c["K"], c["dil"] if "dil" in c else c["stride"], c["pad"], c["Lin"], c["C"]))))
    x = torch.randn(c["B"], c["Lin"], c["C"], generator=g)
    w = torch.randn(c["C"], c["K"], generator=g)
    bias = torch.randn(c["C"], generator=g) if c["bias"] else None
    alpha = inv = None
    if c.get("snake"):
        alpha = torch.rand(c["C"], generator=g) + 0.5
        inv = 1.0 / (alpha + 1e-9)
        assert float((alpha * x.abs().amax((0, 1))).max()) <= 16.0
    return x, w, bias, alpha, inv


# ----------------------------------------------------------------------------------------------------------------- sampler cases
DEFAULTS = SAMPLE_CASES[0]
OFF = dict(temperature=0.9, top_k=0, top_p=1.0, min_p=0.0, repetition_penalty=1.0)
SAMPLER_V = [1, 2, 63, 64, 65, 1023, 1024, 1025, 4100, 8192]   # wave and block edges, all eight kill[] slots of a thread at kMaxV, one entry


# Logits have scale 1 (at scale 4 the filters leave one to four survivors per row, which tests next to nothing) -- with one exception that arithmetic
# forces.  top_p keeps the entries whose ascending cumulative probability exceeds 1 - top_p, and consecutive cumulative probabilities differ by one
# entry's probability; P_MARGIN on both sides of the threshold therefore needs an entry of probability >= 2e-4 astride it.  At V = 8192 without top-k
# (temperature 0.7, top_p 0.9) unit-scale logits put entries of ~5e-5 there (the entry at the 10 % point of a log-normal with sigma = 1 / 0.7 carries
# 1.24 / (8192 * 2.78) of the mass), so no seed can satisfy the margin (nor at scale 2: 300 seeds searched); at scale 2.5 seeds exist and
# min_p = 0.05 still leaves 8 or more survivors per row.  top_p = 0.999 runs at V = 65 for the same reason (the lowest entries of 1025 carry
# ~1e-5 each).
WIDE_SCALE = 2.5


def _spec(name, V, kw, kind="general", B=4, seed=None, **extra):
    return dict(name=name, V=V, B=B, kw=kw, kind=kind, seed=1000 + V if seed is None else seed, **extra)


def sampler_specs():
    specs = [_spec(f"V{V}-defaults", V, DEFAULTS, B=2 if V == 1 else 4) for V in SAMPLER_V]
    specs += [_spec(f"V{V}-set{i}", V, SAMPLE_CASES[i], scale=WIDE_SCALE if (V, i) == (8192, 2) else 1.0) for V in (65, 1025, 8192) for i in (1, 2, 3, 4)]
    for V in (65, 1025):
        specs += [_spec(f"V{V}-top_k{k}", V, dict(OFF, top_k=k)) for k in (1, V - 1, V, V + 5)]
    specs += [_spec(f"top_p{p}", 65 if p == 0.999 else 1025, dict(OFF, top_p=p)) for p in (0.01, 0.999, 0.0, 1.0)]
    specs += [
        _spec("ties-straddle", 1100, dict(OFF, top_k=10), kind="ties", B=2),     # five equal values, two places left: the serial tid == 0 branch
        _spec("ties-fill", 1100, dict(OFF, top_k=13), kind="ties", B=2),         # five equal values, five places left
        _spec("few-finite", 300, dict(OFF, top_k=50), kind="few_finite", B=2),   # three finite entries under top_k = 50
        _spec("min_p1", 1025, dict(OFF, min_p=1.0), kind="minp1", B=2),
        _spec("top_p-exact-half", 2, dict(OFF, top_p=0.5), kind="exact_half", B=3),   # cum == 1 - top_p exactly: the rule is a strict ">"
        _spec("temperature1", 1025, dict(DEFAULTS, temperature=1.0, top_p=0.9)),
        _spec("no-gumbel", 1025, DEFAULTS, gumbel=False),
        _spec("n_hist", 1025, dict(DEFAULTS, repetition_penalty=1.3), kind="n_hist"),
        _spec("long-history", 1025, dict(DEFAULTS, repetition_penalty=1.3), kind="long_hist", B=2),
        _spec("done-rows", 65, DEFAULTS, B=3, done=[0, 1, 0], done_token=2150),
    ]
    return specs


# seeds other than 1000 + V: the first seed (searched upwards from 1000 + V on the CPU) at which sampler_preconditions holds
SEEDS = {"V65-set2": 1067, "V1025-set2": 2027, "V8192-set2": 9203, "top_p0.999": 1068}

TIE_ABOVE = [10, 200, 400, 600, 800, 900, 1000, 1050]
TIE_AT = [3, 70, 500, 1030, 1090]      # in five different waves, on both sides of the 1024-thread round
MINP_TOP = [4, 512, 1024]
FEW_FINITE = [5, 150, 299]


def build_case(spec):
    """The inputs of one sampler case: logits of scale 1 [B, V], Gumbel noise (or None), per-row histories, suppress list, parameters, and the survivors a
    case knows without the oracle (``alive`` / ``dead``: indices per row)."""
    V, B, kind = spec["V"], spec["B"], spec["kind"]
    g = torch.Generator().manual_seed(SEEDS.get(spec["name"], spec["seed"]))
    logits = torch.randn(B, V, generator=g) * spec.get("scale", 1.0)
    u = torch.rand(B, V, generator=g).clamp_(1e-9, 1 - 1e-9)
    case = dict(spec, logits=logits, gumbel=-torch.log(-torch.log(u)) if spec.get("gumbel", True) else None, hist=None, hist_mode="len", suppress=[],
                alive=None, dead=None)
    if kind == "general":
        case["hist"] = [torch.randint(0, V, (n,), generator=g).tolist() for n in (0, 5, 40, 300)[:B]]
        case["suppress"] = list(range(V // 2, V // 2 + 8)) if V >= 64 else []
    elif kind == "ties":
        logits.clamp_(max=3.0)
        for j, i in enumerate(TIE_ABOVE):
            logits[:, i] = 5.0 + 0.125 * j
        logits[:, TIE_AT] = 4.0
        places = spec["kw"]["top_k"] - len(TIE_ABOVE)
        case["alive"], case["dead"] = TIE_AT[:places], TIE_AT[places:]
    elif kind == "few_finite":
        case["suppress"] = [v for v in range(V) if v not in FEW_FINITE]
        case["alive"] = FEW_FINITE
    elif kind == "minp1":
        logits[:, MINP_TOP] = logits.max(-1, keepdim=True).values + 0.5
        case["alive"] = MINP_TOP
    elif kind == "exact_half":   # two equal logits per row: probabilities 2^-1 each, exactly, in float32 and in float64
        logits[:] = torch.tensor([0.0, 0.75, -1.3])[:, None]
        case["alive"], case["dead"] = [1], [0]
    elif kind == "n_hist":
        case["hist"] = [torch.randint(0, V, (40,), generator=g).tolist() for _ in range(B)]
        case["hist_mode"] = "n"
    elif kind == "long_hist":   # 3000 entries: three rounds of the 1024-thread block; duplicates (3000 draws of 1225 ids) and ids >= V
        case["hist"] = [torch.randint(0, V + 200, (3000,), generator=g).tolist() for _ in range(B)]
    else:
        raise KeyError(kind)
    kw = spec["kw"]
    general = kind in ("general", "n_hist", "long_hist") and V >= 63 and kw["temperature"] > 0 and not 0.0 < kw["top_p"] < 0.5
    case["min_alive"] = (min(8, kw["top_k"]) if 0 < kw["top_k"] < V else 8) if general else 0
    return case


def oracle_run(case, dtype=torch.float32):
    """(filtered logits, tokens) of oracle/sampling_ref.py in ``dtype``; a ``done`` row emits ``done_token``."""
    args = dict(generated=case["hist"], suppress_tokens=case["suppress"], **case["kw"])
    lg = case["logits"].to(dtype)
    f = R.filter_logits(lg, **args)
    tok = R.sample(lg, None if case["gumbel"] is None else case["gumbel"].to(dtype), **args)
    if case.get("done"):
        tok = torch.where(torch.tensor(case["done"]) != 0, torch.tensor(case["done_token"]), tok)
    return f, tok


def sampler_preconditions(case):
    """The knife edges a comparison may not hide behind, asserted on the CPU (returns the measured margins):
    - the float32 and the float64 run of the oracle leave the same survivors;
    - float64: every finite entry's cumulative probability is at least P_MARGIN from 1 - top_p -- except in the one case built to sit ON the threshold
      ("top_p-exact-half": two equal logits, top_p = 0.5), where the lower index's cumulative probability is 2^-1 = 1 - top_p exactly in float32 and in
      float64 (asserted), so the reference's strict ``cum > 1 - top_p`` drops it; any exp / log that rounds faithfully gives 0.5 or the float below it
      for exp(-log 2), and both drop it too;
    - float64: every finite entry's log-probability is at least P_MARGIN from the min_p threshold -- except entries bit-equal to the row maximum, whose
      distance is log(min_p) exactly in every precision (0 at min_p = 1: they compare equal to themselves, no rounding is involved);
    - float64: the top-2 gap of filtered (+ gumbel) is at least THR."""
    kw, V = case["kw"], case["V"]
    f32, _ = oracle_run(case, torch.float32)
    f64, _ = oracle_run(case, torch.float64)
    assert torch.equal(torch.isinf(f32), torch.isinf(f64)), (case["name"], "float32 and float64 survivors differ")
    margins = dict(alive=int(torch.isfinite(f64).sum(-1).min()))
    assert margins["alive"] >= max(case["min_alive"], 1), (case["name"], margins)
    use_p = 0.0 < kw["top_p"] < 1.0
    if kw["temperature"] > 0 and (use_p or kw["min_p"] > 0.0):
        pre = R.filter_logits(case["logits"].double(), generated=case["hist"], suppress_tokens=case["suppress"], **dict(kw, top_p=1.0, min_p=0.0))
        lp = torch.log_softmax(pre, dim=-1)
        if use_p:
            order = torch.argsort(lp, dim=-1, stable=True)
            cum = torch.empty_like(lp).scatter_(-1, order, torch.cumsum(torch.gather(torch.exp(lp), -1, order), dim=-1))
            margins["top_p"] = float((cum - (1 - kw["top_p"])).abs()[torch.isfinite(lp)].min())
            if case["kind"] == "exact_half":
                assert bool((cum[:, 0] == 0.5).all()) and bool((cum[:, 1] == 1.0).all()), (case["name"], cum)
            else:
                assert margins["top_p"] >= P_MARGIN, (case["name"], margins)
            lp = R.apply_top_p(lp, kw["top_p"])
        if kw["min_p"] > 0.0:
            top = lp.max(-1, keepdim=True).values
            sel = torch.isfinite(lp) & (lp != top)
            if bool(sel.any()):
                margins["min_p"] = float((lp - (top + math.log(kw["min_p"]))).abs()[sel].min())
                assert margins["min_p"] >= P_MARGIN, (case["name"], margins)
    score = f64 if case["gumbel"] is None or kw["temperature"] <= 0 else f64 + case["gumbel"].double()
    if V >= 2:
        top2 = torch.topk(score, 2, dim=-1).values
        margins["gap"] = float((top2[:, 0] - top2[:, 1]).min())
        assert margins["gap"] >= THR, (case["name"], margins)
    return margins
