"""Case tables, the restated dispatcher, float64 statements, structured inputs and bounds of the attention branch parity suite
(tests/test_attn_refs_cpu.py, tests/test_attn_kernel_edges_gpu.py).  No GPU import: everything here runs on the CPU.

route()       restates mi355_flash_attention's decision (csrc/flash_attn.hip): which of the 24 instantiations a call launches, plus the flags
              split / fused / slabs / planes / head_major.
attn_stmt()   the rule of include/mi355audio.h and csrc/attn_tile.h in float64 (float32 twin: the same code with dtype = float32): GQA, queries
              as the LAST lens_q[b] positions, k_start, causal, window, a zero row for a query without a visible key, K / V already rounded to
              the cache type.
fused_stmt()  the fused decode step: slab sum in slab order, * wscale, + bias, per-head RMSNorm, rope, rounding to the cache type, attention
              over the updated cache, the new cache row.
Bounds        per element, from the float64 trajectory only (nothing is taken from the kernel):
                fp32 routes (flash_attn_kernel, every attn_decode_kernel: a 16-bit cache is read exactly and the arithmetic is fp32):
                    4 * e32 + 1e-6 * peak                       e32 = max |float32 twin - float64 statement|, as _seq_kernel_cases.bar_of
                random-input cases: every bound above is capped at the bar test_transformer_kernels_gpu.py asserts (2e-5, bf16 prefill 3e-5, of the
                    peak); the structured cases (monotone / offset scores of magnitude 80 - 90) are not: there the formulas give up to 2.5 x that bar
                    on the fp32 routes, 8 x on the f16 and 150 x on the bf16 prefill kernel (docs/PARITY.md)
                16-bit prefill (flash_attn16_kernel): the same + EPS16 * (sum_j p_j d_j |v_j - o| + sum_j p_j |v_j|), d_j = scale * sum |q||k_j|:
                    the first-order effect of the hi + lo images of Q (a relative score perturbation) and of P; EPS16 = 2^-16 (bf16), 2^-21 (f16,
                    truncating pack)
                fused step: e32 of the twin already carries the float32 slab-sum chain; rsqrtf is taken at the library's documented 1 ulp for
                    its result plus half an ulp for its argument: RSQRT_REL = 1.5 * 2^-23 of |q| and |k| rows, propagated as a score perturbation;
                    the stored k row additionally half an ulp of the cache type; the stored v row is bit-equal (integer inputs, power-of-two scales)
                planes: hi + lo within 2^-16 (bf16) / 2^-22 (f16) of |value| on top of the row's bound; hi bit-equal to the rounding of `out`.
                    (The f16 lo image is subnormal below 2^-14 and so has an ABSOLUTE floor of 2^-25: every planes case keeps |out| >= 1, V being
                    positive integers, which puts that floor under the relative bound.)
"""
import math
import os
import re

import torch

SENTINEL = -777.25
ENV_KNOBS = ("MI355_ATTN_ONE_WAVE",)
KV = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
KVT = {"f32": 0, "bf16": 1, "f16": 2}
EPS16 = {"bf16": 2.0 ** -16, "f16": 2.0 ** -21}
PLANES_EPS = {False: 2.0 ** -16, True: 2.0 ** -22}
RSQRT_REL = 1.5 * 2.0 ** -23
SLACK = 3   # cache rows past Tk inside the same allocation
HIP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "mlx_audio_amd", "csrc", "flash_attn.hip")
FLAGS = ("split", "fused", "slabs", "planes", "head_major")


def rnd(t, kv):
    """what a cache of type kv hands back"""
    return t.float().to(KV[kv]).float()


# ------------------------------------------------------------------------------------------------------------ the dispatcher, restated
def route(a):
    """(kernel instantiation, frozenset of flags) of a call.  a: dict(mode, Tq, Tk, kv, dh, nsplit, ws (workspace given), fused, in_kgroups,
    planes, head_major)."""
    dh, kvt = a["dh"], KVT[a["kv"]]
    assert dh in (64, 128)
    fused = bool(a.get("fused"))
    flags = set()
    nsplit_req, ws = a.get("nsplit", 0), bool(a.get("ws"))
    if fused:   # new_k forces nsplit = 1 and drops the workspace
        nsplit_req, ws = 1, False
        flags.add("fused")
        if a.get("in_kgroups", 0) > 1:
            flags.add("slabs")
    if a.get("planes"):
        flags.add("planes")
    if a.get("head_major"):
        flags.add("head_major")
    decode = a["mode"] == 2 or (a["mode"] == 0 and a["Tq"] <= 8)
    if decode:
        nsplit = 1
        if ws and nsplit_req != 1:
            if nsplit_req > 1:
                nsplit = nsplit_req
            nsplit = max(1, min(8, nsplit))
        if nsplit > 1:
            flags.add("split")
        wide = a["Tk"] > 256
        one = a["Tk"] <= 64 and nsplit == 1
        nw = 16 if wide else (1 if one else 4)
        kern = f"attn_decode_kernel<{dh}, {nw}, {kvt}>"
    elif kvt == 0:
        kern = f"flash_attn_kernel<{dh}, 0>"
    else:
        kern = f"flash_attn16_kernel<{dh}, {kvt}>"
    return kern, frozenset(flags)


def label(r):
    return r[0] + "".join("+" + f for f in FLAGS if f in r[1])


def case_route(c, **over):
    a = dict(mode=c["mode"], Tq=c["Tq"], Tk=c["Tk"], kv=c["kv"], dh=c["dh"], nsplit=c.get("nsplit", 0), fused=c["fam"] == "fused",
             in_kgroups=c.get("in_kgroups", 0), planes=c.get("planes_R", 0) > 0, head_major=c.get("hm", False))
    a.update(over)
    # ops.flash_attention hands the workspace over exactly when the caller asks for a split of a decode-sized call
    a["ws"] = (a["nsplit"] > 1 or bool(a.get("ws"))) and a["Tq"] <= 8 and a["mode"] != 1   # (or when the test forces it: split_workspace)
    return route(a)


def launch_sites(path=HIP):
    """the instantiations mi355_flash_attention can launch: hipLaunchKernelGGL((name<...>) sites, the two *_CASE macros expanded over the types
    they are invoked for"""
    text = open(path).read()
    text = text.replace("\\\n", " ")
    macros = {}
    for m in re.finditer(r"#define (MI355_\w+_CASE)\(KVT\)(.*)", text):
        macros[m.group(1)] = m.group(2)
    body = re.sub(r"#define MI355_\w+_CASE\(KVT\).*", "", text)
    for name, mbody in macros.items():
        body = re.sub(name + r"\((\d)\)", lambda m: re.sub(r"\bKVT\b", m.group(1), mbody), body)
    sites = re.findall(r"hipLaunchKernelGGL\(\((\w+<[^>]*>)\)", body)
    return sorted({re.sub(r"\s*,\s*", ", ", s) for s in sites})


# ------------------------------------------------------------------------------------------------------------ the statement
def visible(lq, lk, ks, causal, window, variant=None):
    """[lq, lk] bool: key j visible to query i (the last lq positions of lk keys)"""
    i = torch.arange(lq)[:, None] + (0 if variant == "no_causal_offset" else lk - lq)
    j = torch.arange(lk)[None, :]
    vis = ((j >= (0 if variant == "no_k_start" else ks)) & (j < lk)).expand(lq, lk).clone()
    if causal:
        vis = vis & (j <= i)
    if window > 0:
        w = window + (1 if variant == "window_wide" else (-1 if variant == "window_narrow" else 0))
        vis = vis & (j > i - w)
    return vis


def _lens(c, key, full):
    v = c.get(key)
    return [full] * c["B"] if v is None else list(v)


def attn_stmt(q, k, v, c, dtype=torch.float64, variant=None, want_extra=False):
    """q [B, Tq, H dh], k / v [B, Tk, G dh] (values a cache of c['kv'] holds) -> out [B, Tq, H dh] in dtype; rows at and past lens_q[b] are zero
    and mean nothing.  want_extra: also the per-element first-order factor of the 16-bit prefill bound (to be multiplied by EPS16)."""
    B, Tq, Tk, H, G, dh = c["B"], c["Tq"], c["Tk"], c["H"], c["G"], c["dh"]
    scale = c.get("scale", dh ** -0.5)
    lq_, lk_, ks_ = _lens(c, "lens_q", Tq), _lens(c, "lens_k", Tk), _lens(c, "k_start", 0)
    out = torch.zeros(B, Tq, H * dh, dtype=dtype)
    extra = torch.zeros(B, Tq, H * dh, dtype=dtype) if want_extra else None
    r = H // G
    for b in range(B):
        lq, lk = lq_[b], lk_[b]
        if lq == 0 or lk == 0:
            continue
        vis = visible(lq, lk, ks_[b], c["causal"], c.get("window", 0), variant)
        for h in range(H):
            g = h % r if variant == "gqa_mod" else h // r
            g = min(g, G - 1)
            qq = q[b, :lq, h * dh:(h + 1) * dh].to(dtype)
            kk = k[b, :lk, g * dh:(g + 1) * dh].to(dtype)
            vv = v[b, :lk, g * dh:(g + 1) * dh].to(dtype)
            if variant == "c_row_identity":   # the tile restated with P fed to the second contraction in REGISTER order: register r of half-wave h
                idx = torch.arange(lk)           # holds the probability of key c_row(r, h) but meets the value row r + 16 h of its 32-key block
                for kb in range(0, lk - lk % 32, 32):
                    for rr in range(16):
                        for hh in (0, 1):
                            idx[kb + (rr & 3) + 8 * (rr >> 2) + 4 * hh] = kb + rr + 16 * hh
                vv = vv[idx]
            s = ((qq @ kk.T) * scale).masked_fill(~vis, -float("inf"))
            m = s.amax(1, keepdim=True)
            m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
            e = torch.exp(s - m)
            L = e.sum(1, keepdim=True)
            p = torch.where(L > 0, e / torch.where(L > 0, L, torch.ones_like(L)), torch.zeros_like(e))
            o = p @ vv
            out[b, :lq, h * dh:(h + 1) * dh] = o
            if want_extra:
                pd = p * (scale * (qq.abs() @ kk.abs().T))
                t1 = torch.stack([(pd[i, :, None] * (vv - o[i][None, :]).abs()).sum(0) for i in range(lq)])
                extra[b, :lq, h * dh:(h + 1) * dh] = t1 + p @ vv.abs()
    return (out, extra) if want_extra else out


def bar_of(ref64, ref32):
    """(e32, peak, bar): bar = 4 * e32 + 1e-6 * peak (tests/_seq_kernel_cases.py::bar_of)"""
    e32 = float((ref32.double() - ref64.double()).abs().max()) if ref64.numel() else 0.0
    peak = float(ref64.abs().max()) if ref64.numel() else 0.0
    return e32, peak, 4.0 * e32 + 1e-6 * peak


def attn_bound(q, k, v, c, kernel):
    """(float64 statement, per-element bound) for a launch that runs `kernel`"""
    flash16 = kernel.startswith("flash_attn16")
    r64 = attn_stmt(q, k, v, c, torch.float64, want_extra=flash16)
    r64, extra = r64 if flash16 else (r64, None)
    r32 = attn_stmt(q, k, v, c, torch.float32)
    _, _, bar = bar_of(r64, r32)
    bound = torch.full_like(r64, bar)
    if flash16:
        bound = bound + EPS16[c["kv"]] * extra
    if c.get("kind", "random") == "random" and r64.numel():   # never above the bar tests/test_transformer_kernels_gpu.py asserts on random inputs
        bound = bound.clamp(max=existing_bar(c, kernel) * float(r64.abs().max()))
    return r64, bound


def existing_bar(c, kernel):
    """max error / max want that test_transformer_kernels_gpu.py asserts for the route: 3e-5 for the bf16 prefill kernel, 2e-5 elsewhere"""
    return 3e-5 if (kernel.startswith("flash_attn16") and c["kv"] == "bf16") else 2e-5


def valid_rows(c):
    """[B, Tq] bool: rows the kernel writes (i < lens_q[b])"""
    lq = torch.tensor(_lens(c, "lens_q", c["Tq"]))
    return torch.arange(c["Tq"])[None, :] < lq[:, None]


# ------------------------------------------------------------------------------------------------------------ inputs
def _gen(c):
    return torch.Generator().manual_seed(1000 + sum(ord(ch) for ch in c["name"]))


def _score_keys(c, s):
    """q, k with natural-unit score (before the cache rounding of k) s[b, j] * f_h for every query: q = f_h * u, k_j = s_j / scale * u, |u| = 1"""
    B, Tq, Tk, H, G, dh = c["B"], c["Tq"], c["Tk"], c["H"], c["G"], c["dh"]
    scale = c.get("scale", dh ** -0.5)
    # u is a random direction, not the constant one: with equal power-of-two elements the float32 twin's dot product would be exact, and e32 would
    # understate the rounding any float32 evaluation of these scores makes
    u = torch.randn(dh, generator=torch.Generator().manual_seed(dh), dtype=torch.float64)
    u = u / u.norm()
    f = torch.tensor([1.0, 0.75, 0.5, 0.875][:H], dtype=torch.float64)
    q = (f[:, None] * u[None, :]).reshape(1, 1, H * dh).expand(B, Tq, H * dh).float().contiguous()
    k = (s.double()[:, :, None] / scale * u[None, None, :]).float().repeat(1, 1, G)
    return q, rnd(k, c["kv"])


def make_inputs(c):
    """dict(q [B, Tq, H dh], k, v [B, Tk, G dh]) float32, k / v holding values of the cache type"""
    B, Tq, Tk, H, G, dh, kv = c["B"], c["Tq"], c["Tk"], c["H"], c["G"], c["dh"], c["kv"]
    g = _gen(c)
    kind = c.get("kind", "random")
    q = torch.randn(B, Tq, H * dh, generator=g)
    k = rnd(torch.randn(B, Tk, G * dh, generator=g), kv)
    v = rnd(torch.randn(B, Tk, G * dh, generator=g), kv)
    if kind == "uniform":   # q = 0: every visible key has probability exactly 1 / n; v one-hot small integers: sum p v is an exact integer / n
        q = torch.zeros_like(q)
        j = torch.arange(Tk)
        v = torch.zeros(B, Tk, G, dh)
        for b in range(B):
            for gg in range(G):
                v[b, j, gg, j % dh] = ((j * 5 + 3 * b + gg) % 7 + 1).float()
        v = v.reshape(B, Tk, G * dh)
    elif kind in ("mono_up", "mono_down"):
        s = torch.linspace(0.0, 90.0, Tk) if Tk > 1 else torch.zeros(1)
        if kind == "mono_down":
            s = s.flip(0)
        q, k = _score_keys(c, s[None, :].expand(B, Tk))
    elif kind in ("offset_pos", "offset_neg"):
        s = (80.0 if kind == "offset_pos" else -80.0) + torch.randn(B, Tk, generator=g)
        q, k = _score_keys(c, s)
    return dict(q=q, k=k, v=v)


def uniform_expect(c, v):
    """(count [B, Tq, H dh] float64 integers, n [B, Tq] visible keys) of a uniform case: out = count / n exactly"""
    B, Tq, Tk, H, G, dh = c["B"], c["Tq"], c["Tk"], c["H"], c["G"], c["dh"]
    lq_, lk_, ks_ = _lens(c, "lens_q", Tq), _lens(c, "lens_k", Tk), _lens(c, "k_start", 0)
    cnt = torch.zeros(B, Tq, H * dh, dtype=torch.float64)
    n = torch.zeros(B, Tq, dtype=torch.int64)
    for b in range(B):
        lq, lk = lq_[b], lk_[b]
        if lq == 0 or lk == 0:
            continue
        vis = visible(lq, lk, ks_[b], c["causal"], c.get("window", 0)).double()
        n[b, :lq] = vis.sum(1).long()
        for h in range(H):
            gg = h // (H // G)
            cnt[b, :lq, h * dh:(h + 1) * dh] = vis @ v[b, :lk, gg * dh:(gg + 1) * dh].double()
    return cnt, n


def block_max_moves(c, q, k):
    """per (b, h): list of bools, block t (32 keys) raises the running float32 maximum of the last query's scores"""
    dh, H, G = c["dh"], c["H"], c["G"]
    res = []
    for b in range(c["B"]):
        for h in range(H):
            gg = h // (H // G)
            s = (k[b, :, gg * dh:(gg + 1) * dh] @ q[b, -1, h * dh:(h + 1) * dh]) * c.get("scale", dh ** -0.5)
            m, moves = -float("inf"), []
            for t in range(0, c["Tk"], 32):
                bm = float(s[t:t + 32].max())
                moves.append(bm > m)
                m = max(m, bm)
            res.append(moves)
    return res


def poison_plan(c):
    """(nan_rows, big_rows): [B, Tk + SLACK] bool masks.  NaN goes to rows j >= lens_k[b] (slack rows included); +-big goes to rows inside
    [0, lens_k[b]) no query of the item can see (left padding, beyond every causal diagonal, left of every window)."""
    B, Tq, Tk = c["B"], c["Tq"], c["Tk"]
    lq_, lk_, ks_ = _lens(c, "lens_q", Tq), _lens(c, "lens_k", Tk), _lens(c, "k_start", 0)
    nan_rows = torch.zeros(B, Tk + SLACK, dtype=torch.bool)
    big_rows = torch.zeros(B, Tk + SLACK, dtype=torch.bool)
    for b in range(B):
        nan_rows[b, lk_[b]:] = True
        if lk_[b] > 0:
            seen = visible(lq_[b], lk_[b], ks_[b], c["causal"], c.get("window", 0)).any(0) if lq_[b] > 0 else torch.zeros(lk_[b], dtype=torch.bool)
            big_rows[b, :lk_[b]] = ~seen
    return nan_rows, big_rows


def big_value(kv):
    return 6.0e4 if kv == "f16" else 1.0e30   # float16 holds nothing larger


def apply_poison(c, k, v):
    """k, v [B, Tk, G dh] -> [B, Tk + SLACK, G dh] copies with the plan applied (alternating signs)"""
    nan_rows, big_rows = poison_plan(c)
    outs = []
    for t, flip in ((k, 1.0), (v, -1.0)):
        buf = torch.zeros(c["B"], c["Tk"] + SLACK, t.shape[2])
        buf[:, :c["Tk"]] = t
        sign = flip * (1.0 - 2.0 * (torch.arange(t.shape[2]) % 2).float())
        buf = torch.where(big_rows[:, :, None], (big_value(c["kv"]) * sign)[None, None, :].expand_as(buf), buf)
        buf = torch.where(nan_rows[:, :, None], torch.full_like(buf, float("nan")), buf)
        outs.append(buf)
    return outs


# ------------------------------------------------------------------------------------------------------------ the fused step
def rope_rows(n, dh):
    inv = 1.0 / (10000.0 ** (torch.arange(0, dh, 2, dtype=torch.float32) / dh))
    ang = torch.arange(n, dtype=torch.float32)[:, None] * inv[None, :]
    return torch.cos(ang), torch.sin(ang)


def fused_position(c, b):
    lk = c["lens_k"][b] if c.get("lens_k") is not None else None
    pos = (lk - 1 if lk is not None else c["rope_pos"]) - (0 if c.get("k_start") is None else c["k_start"][b])
    return pos


def fused_stmt(x, c, dtype=torch.float64, variant=None, raw_k=False):
    """x: dict(slabs [S, B, (H + 2 G) dh] raw q | k | v projections, cache_k, cache_v [B, Tk, G dh], qw, kw [dh] or None, cos, sin or None,
    q_bias / k_bias / v_bias / q_wscale / k_wscale / v_wscale or None).  Returns (out [B, 1, H dh], new k row [B, G dh], new v row, q row)."""
    B, Tk, H, G, dh, kv = c["B"], c["Tk"], c["H"], c["G"], c["dh"], c["kv"]
    slabs = x["slabs"].to(dtype)
    order = range(slabs.shape[0] - 1, -1, -1) if variant == "slab_reversed" else range(slabs.shape[0])
    acc = None
    for s in order:   # slab order: a sequential chain
        acc = slabs[s].clone() if acc is None else acc + slabs[s]
    nq, nk = H * dh, G * dh
    parts = []
    for name, lo, hi in (("q", 0, nq), ("k", nq, nq + nk), ("v", nq + nk, nq + 2 * nk)):
        t = acc[:, lo:hi]
        ws, bias = x.get(name + "_wscale"), x.get(name + "_bias")
        if variant == "bias_first":
            if bias is not None:
                t = t + bias.to(dtype)
            if ws is not None:
                t = t * ws.to(dtype)
        else:
            if ws is not None:
                t = t * ws.to(dtype)
            if bias is not None:
                t = t + bias.to(dtype)
        parts.append(t)
    qr, kr, vr = parts

    def norm_rope(t, heads, w):
        t = t.reshape(B, heads, dh)
        if w is not None:
            t = t * torch.rsqrt((t * t).mean(-1, keepdim=True) + c.get("eps", 1e-6)) * w.to(dtype)
        if x.get("cos") is not None:
            rows = x["cos"].shape[0]
            res = []
            for b in range(B):
                pos = fused_position(c, b) + ((0 if c.get("k_start") is None else c["k_start"][b]) if variant == "rope_no_k_start" else 0)
                pos = min(max(pos, 0), rows - 1)
                cs, sn = x["cos"][pos].to(dtype), x["sin"][pos].to(dtype)
                tb = t[b]
                if c["rope_mode"] == 1:
                    x0, x1 = tb[:, 0::2], tb[:, 1::2]
                    res.append(torch.stack([x0 * cs - x1 * sn, x1 * cs + x0 * sn], -1).reshape(heads, dh))
                else:
                    x0, x1 = tb[:, :dh // 2], tb[:, dh // 2:]
                    res.append(torch.cat([x0 * cs - x1 * sn, x1 * cs + x0 * sn], -1))
            t = torch.stack(res)
        return t.reshape(B, heads * dh)

    qn = norm_rope(qr, H, x.get("qw"))
    kn = norm_rope(kr, G, x.get("kw"))
    k_new, v_new = rnd(kn, kv).to(dtype), rnd(vr, kv).to(dtype)
    ck, cv = x["cache_k"].to(dtype).clone(), x["cache_v"].to(dtype).clone()
    lk_ = _lens(c, "lens_k", Tk)
    for b in range(B):
        ck[b, lk_[b] - 1], cv[b, lk_[b] - 1] = k_new[b], v_new[b]
    cc = dict(c, Tq=1, causal=True, lens_q=None)
    out = attn_stmt(qn[:, None, :], ck, cv, cc, dtype)
    return (out, k_new, v_new, qn, kn) if raw_k else (out, k_new, v_new, qn)


def fused_bound(x, c):
    """(out64, UNROUNDED k row 64, v row 64, out bound, k row bound): see the module docstring.  The stored k row is compared with the unrounded
    float64 row: a float32-level difference may cross a rounding boundary of the cache type and move the stored element by a whole ulp."""
    o64, k64, v64, q64, k64u = fused_stmt(x, c, torch.float64, raw_k=True)
    o32, _, _, _, k32u = fused_stmt(x, c, torch.float32, raw_k=True)
    _, _, bar = bar_of(o64, o32)
    # rsqrtf: a relative perturbation RSQRT_REL of the whole q row and the whole new k row = of every score by at most RSQRT_REL * |s| (twice for
    # the new key); propagated like the 16-bit prefill term: sum_j p_j d_j |v_j - o| with d_j = 2 * RSQRT_REL * scale * sum |q||k_j|
    ck, cv = x["cache_k"].double().clone(), x["cache_v"].double().clone()
    lk_ = _lens(c, "lens_k", c["Tk"])
    for b in range(c["B"]):
        ck[b, lk_[b] - 1], cv[b, lk_[b] - 1] = k64[b], v64[b]
    _, extra = attn_stmt(q64[:, None, :], ck, cv, dict(c, Tq=1, causal=True, lens_q=None), torch.float64, want_extra=True)
    ob = bar + 2.0 * RSQRT_REL * extra
    t = 4.0 * float((k32u.double() - k64u).abs().max()) + 1e-6 * float(k64u.abs().max()) + RSQRT_REL * k64u.abs()   # the float32 row before the store
    kb = t + half_ulp(k64u.abs() + t, c["kv"])
    return o64, k64u, v64, ob, kb


def half_ulp(x, kv):
    """half an ulp of the cache type at magnitude x (0 for float32: the row is stored as computed)"""
    if kv == "f32":
        return torch.zeros_like(x)
    e = torch.floor(torch.log2(x.clamp(min=2.0 ** -60)))
    return torch.exp2(e - 8) if kv == "bf16" else torch.exp2(e.clamp(min=-14) - 11)


def decode_planes(planes, R, K, f16, variant=None):
    """hi + lo planes (fragment order of mi355_rows_gemm; tests/test_linear_kernel_edges_gpu.py::decode_planes) -> (hi, lo) float64 [R, K];
    column = 64 s + 16 group + 8 half + e"""
    raw = planes[: 2 * R * K].cpu().view(torch.float16 if f16 else torch.bfloat16).double().reshape(K // 64, 2, 2, 4, R, 8)
    if variant == "planes_swapped":   # hh and gq exchanged: column = 64 s + 32 half + 8 group + e (a wrong reading of the order)
        return tuple(raw[:, i].permute(3, 0, 1, 2, 4).reshape(R, K) for i in (0, 1))
    return tuple(raw[:, i].permute(3, 0, 2, 1, 4).reshape(R, K) for i in (0, 1))


def encode_planes(rows, R, f16):
    """the inverse, for the CPU tests: rows [B, K] float -> int16 planes [2 R K] (hi = round to nearest, lo = round of the remainder)"""
    B, K = rows.shape
    dt = torch.float16 if f16 else torch.bfloat16
    full = torch.zeros(R, K, dtype=torch.float32)
    full[:B] = rows.float()
    hi = full.to(dt)
    lo = (full - hi.float()).to(dt)
    img = torch.stack([hi, lo]).reshape(2, R, K // 64, 4, 2, 8).permute(2, 0, 4, 3, 1, 5).contiguous()   # [s, img, hh, gq, R, e]
    return img.view(torch.int16).reshape(-1)


def fused_inputs(c):
    B, Tk, H, G, dh, kv = c["B"], c["Tk"], c["H"], c["G"], c["dh"], c["kv"]
    g = _gen(c)
    S = max(1, c.get("in_kgroups", 0))
    W = (H + 2 * G) * dh
    slabs = torch.randn(S, B, W, generator=g) / math.sqrt(S)
    # the v columns: small integers whose slab sum, power-of-two scale and integer bias are exact in float32 (and in every cache type)
    slabs[:, :, (H + G) * dh:] = torch.randint(0, 3, (S, B, G * dh), generator=g).float()
    slabs[0, :, (H + G) * dh:] += 1.0
    if c.get("zero_slabs"):
        slabs[1:] = 0.0
    x = dict(slabs=slabs)
    x["cache_k"] = rnd(torch.randn(B, Tk, G * dh, generator=g), kv)
    x["cache_v"] = torch.randint(1, 8, (B, Tk, G * dh), generator=g).float()
    x["qw"] = 1.0 + 0.1 * torch.randn(dh, generator=g) if c.get("qw") else None
    x["kw"] = 1.0 + 0.1 * torch.randn(dh, generator=g) if c.get("kw") else None
    if c.get("rope_mode") is not None:
        x["cos"], x["sin"] = rope_rows(c.get("rope_rows", Tk + 4), dh)
    for name, n in (("q", H * dh), ("k", G * dh), ("v", G * dh)):
        if c.get("bias"):
            x[name + "_bias"] = torch.randint(1, 4, (n,), generator=g).float() if name == "v" else torch.randn(n, generator=g)
        if c.get("wscale"):
            x[name + "_wscale"] = torch.full((n,), 2.0) if name == "v" else 0.5 + torch.rand(n, generator=g)
    return x


# ------------------------------------------------------------------------------------------------------------ case tables
def _c(fam, name, kernel, tag, **kw):
    base = dict(fam=fam, name=name, kernel=kernel, tag=tag, B=2, H=2, G=1, causal=False, window=0, lens_q=None, lens_k=None, k_start=None,
                mode=0, nsplit=0, hm=False, kind="random")
    base.update(kw)
    return base


def _dk(dh, nw, kv):
    return f"attn_decode_kernel<{dh}, {nw}, {KVT[kv]}>"


def _fk(dh, kv):
    return f"flash_attn_kernel<{dh}, 0>" if kv == "f32" else f"flash_attn16_kernel<{dh}, {KVT[kv]}>"


TYPES = [(dh, kv) for dh in (64, 128) for kv in ("f32", "bf16", "f16")]
NW_AT = {1: 1, 63: 1, 64: 1, 65: 4, 256: 4, 257: 16, 1025: 16}   # written out by hand: the wave count each key count must get


def decode_cases():
    cs = []
    for ti, (dh, kv) in enumerate(TYPES):
        for ki, (Tk, nw) in enumerate(NW_AT.items()):
            Tq = (1, 3, 8)[(ki + ti) % 3]
            cs.append(_c("decode", f"d{dh}{kv}-k{Tk}-q{Tq}", _dk(dh, nw, kv), f"Tk={Tk} boundary, NW={nw}", dh=dh, kv=kv, Tq=Tq, Tk=Tk,
                         causal=(ki + ti) % 2 == 0))
    t = lambda i: TYPES[i % 6]
    X = []
    dh, kv = t(0)
    X.append(_c("decode", "ragged", _dk(dh, 4, kv), "ragged lens, lens_q < Tq rows untouched, causal lens_q > lens_k", dh=dh, kv=kv, B=3, H=4, G=2, Tq=3, Tk=100,
                causal=True, lens_q=[3, 1, 2], lens_k=[100, 37, 1]))
    dh, kv = t(4)
    X.append(_c("decode", "ragged16", _dk(dh, 16, kv), "ragged lens on 16 waves, lens_q = 0 item", dh=dh, kv=kv, B=3, Tq=2, Tk=300, causal=True, lens_q=[2, 0, 1],
                lens_k=[300, 200, 65]))
    for i, (Tk, ks, nw) in enumerate([(100, [5, 63], 4), (100, [64, 99], 4), (300, [70, 299], 16), (40, [39, 41], 1)]):
        dh, kv = t(i + 1)
        X.append(_c("decode", f"kstart{i}", _dk(dh, nw, kv), "k_start inside / past the first chunk, k_start = Tk - 1, k_start > qpos (no visible key)", dh=dh, kv=kv,
                    Tq=1, Tk=Tk, causal=True, k_start=ks))
    for i, w in enumerate([1, 5, 64, 70]):
        for j, (Tk, nw) in enumerate([(131, 4), (300, 16)]):
            dh, kv = t(2 * i + j)
            X.append(_c("decode", f"win{w}-k{Tk}", _dk(dh, nw, kv), f"window {w}: kbeg unaligned", dh=dh, kv=kv, Tq=(1, 3)[j], Tk=Tk, causal=True, window=w))
    for i, (Tk, nw) in enumerate([(50, 1), (130, 4), (333, 16)]):
        for j in range(2):
            dh, kv = t(2 * i + j + 1)
            X.append(_c("decode", f"hm-k{Tk}-{j}", _dk(dh, nw, kv), "head-major K / V", dh=dh, kv=kv, H=4, G=2, Tq=1 + 2 * j, Tk=Tk, causal=bool(j), hm=True))
    for i in range(2):
        dh, kv = t(3 * i + 2)
        X.append(_c("decode", f"mode2-q12-{i}", _dk(dh, 4, kv), "mode = 2 forces the decode kernel past the auto switch", dh=dh, kv=kv, Tq=12, Tk=70, causal=True, mode=2))
    splits = [(65, 8, 1, False, "a split without a key"), (700, 8, 1, False, "every split has keys"), (300, 3, 3, True, "causal rows end in different splits"),
              (130, 2, 1, True, "two splits"), (40, 2, 1, False, "Tk <= 64 but split: 4 waves"), (1025, 9, 1, False, "nsplit 9 clamps to 8"),
              (257, 3, 3, True, "split, dh / type rotation")]
    for i, (Tk, ns, Tq, causal, why) in enumerate(splits):
        dh, kv = t(i)
        X.append(_c("decode", f"split{ns}-k{Tk}", _dk(dh, 16 if Tk > 256 else 4, kv), why, dh=dh, kv=kv, H=4, G=2, Tq=Tq, Tk=Tk, causal=causal, nsplit=ns,
                    hm=(i == 1)))
    # structured inputs
    for i, (Tk, nw, Tq, causal, w, ks) in enumerate([(64, 1, 1, False, 0, None), (65, 4, 3, True, 0, None), (257, 16, 1, True, 70, None), (128, 4, 8, True, 0, [3, 64]),
                                                      (300, 16, 2, False, 0, [0, 100]), (200, 4, 1, True, 128, None)]):
        dh, kv = t(i)
        X.append(_c("decode", f"uniform{i}", _dk(dh, nw, kv), "uniform scores: the visible set itself", dh=dh, kv=kv, Tq=Tq, Tk=Tk, causal=causal, window=w, k_start=ks,
                    kind="uniform"))
    for i, kind in enumerate(["mono_up", "mono_down", "offset_pos", "offset_neg"]):
        for j, (Tk, nw) in enumerate([(130, 4), (300, 16)]):
            dh, kv = t(2 * i + j)
            X.append(_c("decode", f"{kind}-k{Tk}", _dk(dh, nw, kv), "structured scores", dh=dh, kv=kv, Tq=1, Tk=Tk, causal=True, kind=kind))
    dh, kv = t(5)
    X.append(_c("decode", "zero-k", _dk(dh, 4, kv), "lens_k = 0: zero rows; lens_q = 0: nothing written", dh=dh, kv=kv, B=3, Tq=3, Tk=70, causal=True, lens_q=[3, 0, 2],
                lens_k=[0, 70, 33]))
    dh, kv = t(3)
    X.append(_c("decode", "split-uniform", _dk(dh, 4, kv), "uniform scores through the split merge", dh=dh, kv=kv, Tq=1, Tk=256, nsplit=4, kind="uniform"))
    return cs + X


def flash_cases():
    cs = []
    TQ = [9, 32, 33, 96, 97, 128, 129, 257]
    TK = [31, 33, 63, 65, 127, 129]
    for ti, (dh, kv) in enumerate(TYPES):
        for qi, Tq in enumerate(TQ):
            Tk = TK[(qi + ti) % 6]
            cs.append(_c("flash", f"f{dh}{kv}-q{Tq}-k{Tk}", _fk(dh, kv), f"Tq={Tq} (inactive waves), Tk={Tk} stage edge", dh=dh, kv=kv, Tq=Tq, Tk=Tk, causal=qi % 2 == 1))
    t = lambda i: TYPES[i % 6]
    X = []
    for i, Tq in enumerate([1, 8, 1, 8, 1, 8]):
        dh, kv = t(i)
        X.append(_c("flash", f"mode1-q{Tq}-{dh}{kv}", _fk(dh, kv), "mode = 1 forces the flash kernel below the auto switch", dh=dh, kv=kv, Tq=Tq, Tk=70, causal=True, mode=1))
    for i in range(6):
        dh, kv = t(i)
        X.append(_c("flash", f"tq-gt-tk-{dh}{kv}", _fk(dh, kv), "Tq > Tk causal: first queries see nothing", dh=dh, kv=kv, Tq=40, Tk=20, causal=True))
        X.append(_c("flash", f"ragged-{dh}{kv}", _fk(dh, kv), "lens_q 0 / 1 / 33 / 128 in one batch", dh=dh, kv=kv, B=4, H=4, G=2, Tq=128, Tk=140, causal=True,
                    lens_q=[0, 1, 33, 128], lens_k=[50, 140, 33, 129]))
    for i, w in enumerate([1, 31, 32, 33, 64, 65, 200]):
        dh, kv = t(i)
        T = 257 if w == 200 else 140
        X.append(_c("flash", f"win{w}-{dh}{kv}", _fk(dh, kv), f"window {w}", dh=dh, kv=kv, Tq=T, Tk=T, causal=True, window=w))
        dh, kv = t(i + 3)
        X.append(_c("flash", f"win{w}u-{dh}{kv}", _fk(dh, kv), f"window {w}, uniform scores", dh=dh, kv=kv, Tq=T, Tk=T, causal=True, window=w, kind="uniform"))
    for i, ks in enumerate([[0, 1, 31], [32, 63, 64], [65, 99, 80]]):
        for j in range(2):
            dh, kv = t(2 * i + j)
            X.append(_c("flash", f"kstart{i}-{dh}{kv}", _fk(dh, kv), "k_start at stage edges, = lens_k - 1, hiding every key from the first queries", dh=dh, kv=kv,
                        B=3, Tq=40, Tk=100, causal=True, k_start=ks, kind=("random", "uniform")[j]))
    for i, kind in enumerate(["mono_up", "mono_down", "offset_pos", "offset_neg"]):
        for j in range(3):
            dh, kv = t(i + 2 * j)
            X.append(_c("flash", f"{kind}-{dh}{kv}", _fk(dh, kv), "structured scores: the rescale arms / the max subtraction", dh=dh, kv=kv, Tq=33, Tk=160,
                        causal=False, kind=kind))
    for i in range(6):
        dh, kv = t(i)
        X.append(_c("flash", f"zero-k-{dh}{kv}", _fk(dh, kv), "lens_k = 0: zero rows", dh=dh, kv=kv, B=3, Tq=130, Tk=40, causal=bool(i % 2), lens_q=[130, 9, 0],
                    lens_k=[0, 40, 0]))
    for i in range(6):
        dh, kv = t(i)
        X.append(_c("flash", f"hm-{dh}{kv}", _fk(dh, kv), "head-major K / V", dh=dh, kv=kv, H=4, G=2, Tq=40, Tk=97, causal=True, hm=True))
    return cs + X


def fused_cases():
    cs = []
    tks = {1: [1, 40, 64], 4: [65, 130, 256], 16: [257, 300, 513]}
    i = 0
    for dh in (64, 128):
        for nw in (1, 4, 16):
            for ki, kv in enumerate(("f32", "bf16", "f16")):
                Tk = tks[nw][(ki + (dh == 128)) % 3]
                row = i // 3   # rope, slot form and k_start rotate against the cache type: every type meets every rope mode and every form
                slot = (i + 2 * row) % 3 == 1
                kg = (0, 1, 2, 4, 5, 9)[i % 6]
                pr = (0, 16, 32, 64, 0, 16)[(i + 1) % 6]
                c = _c("fused", f"fu{dh}-{nw}-{kv}-k{Tk}", _dk(dh, nw, kv), f"NW={nw} {kv}, in_kgroups={kg}, planes_R={pr}", dh=dh, kv=kv, B=3, H=4, G=2, Tq=1, Tk=Tk,
                       causal=True, mode=(0, 2)[i % 2], qw=i % 2 == 0, kw=i % 4 < 2, rope_mode=(None, 0, 1)[(i + row) % 3],
                       rope_pos=Tk + (9 if i % 6 == 5 else 2), lens_k=[Tk, max(1, Tk - 7), max(1, Tk // 2)] if slot else None,
                       k_start=[0, min(2, Tk - 1), 0] if ((i + 2 * row) % 3 == 2 and Tk > 1) else None, in_kgroups=kg, bias=i % 2 == 1, wscale=i % 4 >= 2,
                       planes_R=pr, planes_f16=(i // 2) % 2 == 1, out_null=(pr > 0 and i % 2 == 0), hm=(i % 5 == 3))
                cs.append(c)
                i += 1
    return cs


def fused_equal_cases():
    """the fused step against head_norm_rope + store + plain decode attention: raw projections (no slabs, scale, bias), every cache type with no
    rope, half-split and interleaved rope, k_start > 0, at both dh; rope_pos differs from Tk - 1"""
    cs = []
    j = 0
    for dh in (64, 128):
        for kv in ("f32", "bf16", "f16"):
            for rm in (None, 0, 1):
                Tk = (40, 130, 300, 1)[(j + (dh == 128)) % 4]
                nw = 1 if Tk <= 64 else (4 if Tk <= 256 else 16)
                cs.append(_c("fused", f"eq{dh}-{kv}-rope{rm}-k{Tk}", _dk(dh, nw, kv), "fused step == separate kernels", dh=dh, kv=kv, B=3, H=4, G=2, Tq=1, Tk=Tk,
                             causal=True, qw=rm is None or j % 3 != 2, kw=rm is None or j % 4 != 3, rope_mode=rm, rope_pos=Tk + 1,
                             k_start=[0, 2, 1] if (j % 2 == 1 and Tk > 2) else None, in_kgroups=0, bias=False, wscale=False, planes_R=0, planes_f16=False,
                             out_null=False))
                j += 1
    return cs


def case_id(c):
    return c["name"]
