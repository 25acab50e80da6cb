"""GPU half of the attention branch parity suite: every instantiation mi355_flash_attention can launch, at the key-count, query-count, window,
k_start and length edges of tests/_attn_cases.py, against the float64 statement at per-element bounds computed from that statement alone.

Every operand is a view into a larger buffer: q has NaN guard columns (and, in poisoned runs, NaN rows at and past lens_q[b]); K / V live in a
cache with SLACK rows past Tk; outputs are NaN-filled views inside sentinel-filled buffers whose guard columns, guard row and rows at or past
lens_q[b] must stay untouched.  Each case runs clean and poisoned (NaN in cache rows j >= lens_k[b], +-1e30 -- the largest float16 for that type --
in rows no query of the item can see) and the two runs must agree bit for bit.  Worst error / bound is printed per case as
``ATTN <route> <case> ratio=...``; nothing but ratio <= 1 is asserted about it.

The A/B knob of the decode dispatch is read once per process: it must be unset (asserted at import)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _attn_cases as S

assert [k for k in S.ENV_KNOBS if k in os.environ] == [], "MI355_ATTN_ONE_WAVE must be unset for this suite"

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    from mlx_audio_amd import ops as _ops

    _ops.require_gpu()
    return _ops


def sync():
    """a device fault ends the session: nothing more is launched on a device that has faulted"""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"device error, session ended: {e}", returncode=3)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def kv_buffers(c, k, v, poison, hm):
    """device (k view, v view, whole buffer) of cache type: [B, Tk + SLACK] rows, packed k | v rows or head-major planes"""
    B, Tk, G, dh = c["B"], c["Tk"], c["G"], c["dh"]
    if poison:
        kp, vp = S.apply_poison(c, k, v)
    else:
        kp, vp = (torch.cat([t, torch.zeros(B, S.SLACK, G * dh)], 1) for t in (k, v))
    dt = S.KV[c["kv"]]
    if hm:
        buf = torch.stack([kp, vp]).reshape(2, B, Tk + S.SLACK, G, dh).permute(0, 1, 3, 2, 4).contiguous().to(dt).to(DEV)
        return buf[0][:, :, :Tk], buf[1][:, :, :Tk], buf
    buf = torch.cat([kp, vp], 2).to(dt).to(DEV)
    return buf[:, :Tk, :G * dh], buf[:, :Tk, G * dh:], buf


def run_attn(ops, c, x, *, poison=False, hm=None, nsplit=None, mode=None, ws=False):
    """one launch of case c on inputs x -> out [B, Tq, H dh] on the CPU (rows at and past lens_q[b] NaN), all guards checked"""
    B, Tq, Tk, H, G, dh = c["B"], c["Tq"], c["Tk"], c["H"], c["G"], c["dh"]
    hm = c["hm"] if hm is None else hm
    nsplit = c["nsplit"] if nsplit is None else nsplit
    mode = c["mode"] if mode is None else mode
    rows = S.valid_rows(c)
    qb = torch.full((B, Tq, H * dh + 8), float("nan"))
    qb[:, :, :H * dh] = x["q"]
    if poison:
        qb[~rows] = float("nan")
    qd = qb.to(DEV)
    kd, vd, _ = kv_buffers(c, x["k"], x["v"], poison, hm)
    buf = torch.full((B, Tq + 1, H * dh + 8), S.SENTINEL, device=DEV)
    out = buf[:, :Tq, :H * dh]
    out.fill_(float("nan"))
    ti = lambda l: None if l is None else torch.tensor(l, dtype=torch.int32, device=DEV)
    ops.flash_attention(qd[:, :, :H * dh], kd, vd, out, heads=H, kv_heads=G, dh=dh, scale=c.get("scale"), causal=c["causal"], window=c["window"],
                        lens_q=ti(c["lens_q"]), lens_k=ti(c["lens_k"]), k_start=ti(c["k_start"]), mode=mode, head_major=hm, nsplit=nsplit, split_workspace=ws)
    sync()
    if (nsplit > 1 or ws) and Tq <= 8 and mode != 1:
        _, cnt = ops.attn_split_workspace(torch.device(DEV), B * H * Tq, dh)
        assert int(cnt.abs().sum()) == 0, "split_cnt must be left zeroed"
    whole = buf.cpu()
    assert bool((whole[:, Tq] == S.SENTINEL).all()) and bool((whole[:, :, H * dh:] == S.SENTINEL).all()), "guard row / guard columns written"
    got = whole[:, :Tq, :H * dh]
    assert bool(torch.isnan(got[~rows]).all()), "rows at or past lens_q[b] must stay untouched"
    assert bool(torch.isfinite(got[rows]).all()), "a written row is not finite"
    return got


def check_case(ops, c, **over):
    """the case against its statement; returns the clean output"""
    r = S.case_route(c, **{k: v for k, v in over.items() if k in ("mode", "nsplit")}, **({"head_major": over["hm"]} if "hm" in over else {}))
    if not over:
        assert r[0] == c["kernel"], (r, c["kernel"])
    x = S.make_inputs(c)
    got = run_attn(ops, c, x, **over)
    rows = S.valid_rows(c)
    if c["kind"] == "uniform":
        cnt, n = S.uniform_expect(c, x["v"])
        nn = n.clamp(min=1)[:, :, None].double()
        want = torch.where(n[:, :, None] > 0, cnt / nn, torch.zeros_like(cnt))
        want32 = want.float()
        ulp = torch.from_numpy(np.spacing(want32.abs().numpy())).double()
        bound = 2.0 * ulp                                                      # two roundings: 1 / n, then the product
        pow2 = ((n & (n - 1)) == 0)[:, :, None].expand_as(want) & rows[:, :, None]
        assert torch.equal(got[pow2], want32[pow2]), "a power-of-two key count is bit-equal"
        err = (got.double() - want).abs()[rows]
        ratio = float((err / bound[rows].clamp(min=1e-300)).max()) if err.numel() else 0.0
        assert bool((err[bound[rows] == 0] == 0).all())
    else:
        ref, bound = S.attn_bound(x["q"], x["k"], x["v"], c, r[0])
        err = (got.double() - ref).abs()[rows]
        ratio = float((err / bound[rows]).max()) if err.numel() else 0.0
    print(f"ATTN {S.label(r)} {c['name']} ratio={ratio:.3f}")
    assert ratio <= 1.0, (c["name"], S.label(r), ratio)
    return x, got


def sub_case(c, b):
    pick = lambda l: None if l is None else [l[b]]
    return dict(c, B=1, lens_q=pick(c["lens_q"]), lens_k=pick(c["lens_k"]), k_start=pick(c["k_start"]), name=c["name"])


def all_equalities(ops, c, x, got):
    assert same_bits(run_attn(ops, c, x, poison=True), got), "poisoned run differs from the clean run"
    if c["hm"]:
        assert same_bits(run_attn(ops, c, x, hm=False), got), "packed K / V differ from head-major"
    if c["lens_q"] is not None or c["lens_k"] is not None or c["k_start"] is not None:   # an item alone == the item inside its batch
        for b in range(c["B"]):
            xb = {k: t[b:b + 1] for k, t in x.items()}
            assert same_bits(run_attn(ops, sub_case(c, b), xb), got[b:b + 1]), f"item {b} alone differs from the batch"


@pytest.mark.parametrize("c", S.decode_cases(), ids=S.case_id)
def test_decode_branches(ops, c):
    x, got = check_case(ops, c)
    all_equalities(ops, c, x, got)
    if c["nsplit"] > 1:   # split against unsplit: both inside the bound of the one statement (not bit-equal: the merge order differs)
        check_case(ops, c, nsplit=0)
        plain = run_attn(ops, c, x, nsplit=0)   # no workspace
        for ns in (1, 0):   # the workspace PRESENT with nsplit = 1 (off) and nsplit = 0 (the library never splits on its own): the unsplit launch
            assert S.case_route(c, nsplit=ns, ws=True) == S.case_route(c, nsplit=0)
            assert same_bits(run_attn(ops, c, x, nsplit=ns, ws=True), plain), f"workspace with nsplit = {ns} differs from the call without one"
    if c["name"].startswith("d") and c["Tk"] in (63, 257):
        assert same_bits(run_attn(ops, c, x), got), "a second run differs"


@pytest.mark.parametrize("c", S.flash_cases(), ids=S.case_id)
def test_flash_branches(ops, c):
    x, got = check_case(ops, c)
    all_equalities(ops, c, x, got)
    if c["mode"] == 1:    # flash against decode on the same inputs: each within its own bound of the one statement
        check_case(ops, c, mode=2)
    if c["Tq"] in (33, 129):
        assert same_bits(run_attn(ops, c, x), got), "a second run differs"


# ------------------------------------------------------------------------------------------------------------ the fused step
def run_fused(ops, c, x, *, in_kgroups=None, planes=True):
    """-> dict(out (or None), cache before / after (whole buffers, CPU), planes before / after)"""
    B, Tk, H, G, dh, kv = c["B"], c["Tk"], c["H"], c["G"], c["dh"], c["kv"]
    nq, nk, W = H * dh, G * dh, (H + 2 * G) * dh
    kg = c["in_kgroups"] if in_kgroups is None else in_kgroups
    S_ = x["slabs"].shape[0]
    sl = torch.full((S_ + 1, B, W), float("nan"))   # one more slab of NaN behind the last: a loop that runs one too far shows
    sl[:S_] = x["slabs"]
    sl = sl.to(DEV)
    lk_ = S._lens(c, "lens_k", Tk)
    ck = torch.full((B, Tk + S.SLACK, nk), float("nan"))
    cv = torch.full((B, Tk + S.SLACK, nk), float("nan"))
    for b in range(B):   # rows [0, lens_k[b] - 1) are the cache; the new row and everything behind it hold NaN
        ck[b, :lk_[b] - 1], cv[b, :lk_[b] - 1] = x["cache_k"][b, :lk_[b] - 1], x["cache_v"][b, :lk_[b] - 1]
    dt = S.KV[kv]
    if c["hm"]:
        cache = torch.stack([ck, cv]).reshape(2, B, Tk + S.SLACK, G, dh).permute(0, 1, 3, 2, 4).contiguous().to(dt).to(DEV)
        kd, vd = cache[0][:, :, :Tk], cache[1][:, :, :Tk]
    else:
        cache = torch.cat([ck, cv], 2).to(dt).to(DEV)
        kd, vd = cache[:, :Tk, :nk], cache[:, :Tk, nk:]
    before = cache.cpu().clone()
    d = lambda t: None if t is None else t.to(DEV).contiguous()
    fused = dict(new_k=sl[0][:, nq:nq + nk], new_v=sl[0][:, nq + nk:], q_norm_w=d(x.get("qw")), k_norm_w=d(x.get("kw")), eps=1e-6, cos=d(x.get("cos")),
                 sin=d(x.get("sin")), rope_mode=c["rope_mode"] or 0, pos=c["rope_pos"], in_kgroups=kg, in_kg_stride=B * W)
    for n in ("q", "k", "v"):
        fused[n + "_bias"], fused[n + "_wscale"] = d(x.get(n + "_bias")), d(x.get(n + "_wscale"))
    R = c["planes_R"] if planes else 0
    pl = pl0 = None
    if R:
        pl = torch.full((2 * R * nq + 64,), 0x1234, dtype=torch.int16, device=DEV)
        pl0 = pl.cpu().clone()
    buf = out = None
    if not (R and c["out_null"]):
        buf = torch.full((B, 2, nq + 8), S.SENTINEL, device=DEV)
        out = buf[:, :1, :nq]
        out.fill_(float("nan"))
    ti = lambda l: None if l is None else torch.tensor(l, dtype=torch.int32, device=DEV)
    ops.flash_attention(sl[0][:, None, :nq], kd, vd, out, heads=H, kv_heads=G, dh=dh, causal=True, lens_k=ti(c["lens_k"]), k_start=ti(c["k_start"]),
                        mode=c["mode"], head_major=c["hm"], fused=fused, out_planes=pl, planes_R=R, planes_f16=c["planes_f16"])
    sync()
    res = dict(before=before, after=cache.cpu(), planes=None if pl is None else pl.cpu(), planes0=pl0, out=None)
    if buf is not None:
        whole = buf.cpu()
        assert bool((whole[:, 1] == S.SENTINEL).all()) and bool((whole[:, :, nq:] == S.SENTINEL).all()), "guard row / guard columns written"
        res["out"] = whole[:, :1, :nq]
        assert bool(torch.isfinite(res["out"]).all())
    return res


def cache_rows(c, whole):
    """(k [B, Tk + SLACK, G dh], v) of a whole cache buffer, as float64"""
    B, Tk, G, dh = c["B"], c["Tk"], c["G"], c["dh"]
    if c["hm"]:
        t = whole.permute(0, 1, 3, 2, 4).reshape(2, B, Tk + S.SLACK, G * dh)
        return t[0], t[1]
    return whole[:, :, :G * dh], whole[:, :, G * dh:]


@pytest.mark.parametrize("c", S.fused_cases(), ids=S.case_id)
def test_fused_step_branches(ops, c):
    r = S.case_route(c)
    assert r[0] == c["kernel"]
    B, Tk, H, G, dh = c["B"], c["Tk"], c["H"], c["G"], c["dh"]
    x = S.fused_inputs(c)
    o64, k64, v64, ob, kb = S.fused_bound(x, c)
    res = run_fused(ops, c, x)
    lk_ = S._lens(c, "lens_k", Tk)
    kb4, vb4 = cache_rows(c, res["before"])
    ka, va = cache_rows(c, res["after"])
    ratio_k = 0.0
    for b in range(B):
        row = lk_[b] - 1
        keep = torch.arange(Tk + S.SLACK) != row
        assert same_bits(ka[b][keep], kb4[b][keep]) and same_bits(va[b][keep], vb4[b][keep]), "a cache row other than the new one changed"
        assert torch.equal(va[b, row].double(), v64[b]), "the stored v row is exact"
        ratio_k = max(ratio_k, float(((ka[b, row].double() - k64[b]).abs() / kb[b]).max()))
    ratio_o = ratio_p = 0.0
    if res["out"] is not None:
        ratio_o = float(((res["out"].double() - o64).abs() / ob).max())
    if res["planes"] is not None:
        R, f16 = c["planes_R"], c["planes_f16"]
        assert torch.equal(res["planes"][2 * R * H * dh:], res["planes0"][2 * R * H * dh:]), "planes written past their end"
        hi, lo = S.decode_planes(res["planes"], R, H * dh, f16)
        hi0, lo0 = S.decode_planes(res["planes0"], R, H * dh, f16)
        assert torch.equal(hi[B:], hi0[B:]) and torch.equal(lo[B:], lo0[B:]), "plane rows >= B written"
        assert float(o64.abs().min()) >= 1.0   # (see tests/_attn_cases.py on the float16 lo image)
        ratio_p = float((((hi + lo)[:B] - o64[:, 0]).abs() / (ob[:, 0] + S.PLANES_EPS[f16] * o64[:, 0].abs())).max())
        if res["out"] is not None:
            assert torch.equal(hi[:B].float(), res["out"][:, 0].to(torch.float16 if f16 else torch.bfloat16).float()), "hi is the rounding of the out row"
    print(f"ATTN {S.label(r)} {c['name']} ratio={max(ratio_o, ratio_k, ratio_p):.3f} (out {ratio_o:.3f}, k row {ratio_k:.3f}, planes {ratio_p:.3f})")
    assert max(ratio_o, ratio_k, ratio_p) <= 1.0
    if Tk == 1 and res["out"] is not None:   # no cached key: the output IS the new v row
        assert torch.equal(res["out"][:, 0].double().reshape(B, H, dh), v64.reshape(B, G, 1, dh).expand(B, G, H // G, dh).reshape(B, H, dh))
    if c["in_kgroups"] > 1:   # slabs that are all zero but the first == in_kgroups = 1
        xz = S.fused_inputs(dict(c, zero_slabs=True))
        a, b1 = run_fused(ops, c, xz), run_fused(ops, c, xz, in_kgroups=1)
        assert same_bits(a["after"], b1["after"]) and (a["out"] is None or same_bits(a["out"], b1["out"]))
        assert a["planes"] is None or torch.equal(a["planes"], b1["planes"])


@pytest.mark.parametrize("c", S.fused_equal_cases() + [c for c in S.fused_cases() if c["in_kgroups"] <= 1 and not c["bias"] and not c["wscale"] and not c["hm"]
                               and c["lens_k"] is None and c["rope_pos"] < c["Tk"] + 4], ids=S.case_id)
def test_fused_step_equals_separate_kernels(ops, c):
    """head_norm_rope (q in place, k into a scratch row) + the store + mode = 2 attention on the same values: the cache row is bit-equal (the
    arithmetic the kernel comments hold equal); the output adds the new key as one more softmax update BEHIND the cached keys instead of inside
    the last chunk, so it agrees within the two bounds, not bit for bit."""
    assert S.case_route(c)[0] == c["kernel"]
    B, Tk, H, G, dh, kv = c["B"], c["Tk"], c["H"], c["G"], c["dh"], c["kv"]
    nq, nk = H * dh, G * dh
    x = S.fused_inputs(c)
    o64, _, _, ob, _ = S.fused_bound(x, c)
    res = run_fused(ops, c, x, planes=False)
    raw = x["slabs"][0].to(DEV)
    q_ref, kv_ref = raw[:, None, :nq].clone(), raw[:, None, nq:].clone()
    d = lambda t: None if t is None else t.to(DEV).contiguous()
    ks = None if c["k_start"] is None else torch.tensor(c["k_start"], dtype=torch.int32, device=DEV)
    ops.head_norm_rope(q_ref, q_ref, heads=H, dh=dh, norm_weight=d(x["qw"]), eps=1e-6, cos=d(x.get("cos")), sin=d(x.get("sin")), pos0=c["rope_pos"],
                       interleaved=c["rope_mode"] == 1, pos_sub=ks, second=(kv_ref[:, :, :nk], kv_ref[:, :, :nk], G, d(x["kw"])))
    cache = res["before"].to(DEV)
    cache[:, Tk - 1] = kv_ref[:, 0].to(S.KV[kv])
    out = torch.empty(B, 1, nq, device=DEV)
    ops.flash_attention(q_ref, cache[:, :Tk, :nk], cache[:, :Tk, nk:], out, heads=H, kv_heads=G, dh=dh, causal=True, k_start=ks, mode=2)
    sync()
    assert same_bits(cache.cpu()[:, Tk - 1], res["after"][:, Tk - 1]), "the fused cache row differs from head_norm_rope's"
    assert float(((out.cpu().double() - o64).abs() / ob).max()) <= 1.0 and float(((res["out"].double() - o64).abs() / ob).max()) <= 1.0
    if Tk == 1:
        assert same_bits(out.cpu(), res["out"])


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals(ops):
    """Every MI355_REQUIRE of mi355_flash_attention a caller can trip, through the raw struct: the argument error, a message, nothing launched."""
    from mlx_audio_amd import _lib

    lib = _lib.load()
    B, H, dh, Tk = 17, 2, 64, 16
    out = torch.full((B, 2, H * dh), S.SENTINEL, device=DEV)
    q = torch.zeros(B, 2, H * dh + 4, device=DEV)
    cache = torch.full((B, Tk, 2 * H * dh + 8), 3.0, device=DEV)
    cache16 = torch.full((B, Tk, 2 * H * dh + 8), 3.0, dtype=torch.bfloat16, device=DEV)
    new = torch.zeros(2, B, 2 * H * dh, device=DEV)
    pl = torch.full((2 * 64 * H * dh,), 0x1234, dtype=torch.int16, device=DEV)
    tab = torch.zeros(Tk, dh // 2, device=DEV)
    lens = torch.ones(B, dtype=torch.int32, device=DEV)
    ws, cnt = ops.attn_split_workspace(torch.device(DEV), B * H * 2, dh)
    p = lambda t: t.data_ptr()
    base = dict(q=p(q), q_bstride=q.stride(0), ldq=q.stride(1), k=p(cache), k_bstride=cache.stride(0), ldk=cache.stride(1), v=p(cache) + 4 * H * dh,
                v_bstride=cache.stride(0), ldv=cache.stride(1), heads=H, kv_heads=H, dh=dh, Tq=1, Tk=Tk, causal=1, window=0, scale=0.125, B=2, mode=0,
                out=p(out), out_bstride=out.stride(0), ldo=out.stride(1), nsplit=0, kv_dtype=0)
    planes = dict(out_planes=p(pl), planes_R=16, planes_dtype=0)
    fused = dict(new_k=p(new), new_v=p(new) + 4 * H * dh, new_bstride=new.stride(1))
    split = dict(split_ws=p(ws), split_cnt=p(cnt))
    k16 = dict(k=p(cache16), v=p(cache16) + 2 * H * dh, kv_dtype=1, Tq=9)
    need = "a planes output needs"
    step = "the fused norm / rope step"
    table = [
        (dict(planes, Tq=2), need), (dict(planes, mode=1), need), (dict(planes, nsplit=2, **split), need), (dict(planes, B=17), need),
        (dict(planes, planes_R=48), need), (dict(planes, planes_dtype=2), need),
        (dict(fused, lens_q=p(lens)), step), (dict(fused, causal=0), step), (dict(fused, Tq=2), step), (dict(fused, mode=1), step),
        (dict(fused, nsplit=2, **split), step), (dict(fused, new_v=None), step),
        (dict(fused, rope_cos=p(tab), rope_rows=Tk), "rope tables incomplete"), (dict(fused, rope_cos=p(tab), rope_sin=p(tab), rope_rows=0), "rope tables incomplete"),
        (dict(in_kgroups=2, in_kg_stride=64), "slab inputs exist"), (dict(fused, in_kgroups=2, in_kg_stride=0), "slab inputs exist"),
        (dict(k16, ldk=cache16.stride(1) + 4, ldv=cache16.stride(1) + 4), "16-byte aligned for the prefill kernel"),
        (dict(k16, k=p(cache16) + 8), "16-byte aligned"),
        (dict(dh=96), "head dim must be 64 or 128"), (dict(heads=3, kv_heads=2), "multiple of kv_heads"), (dict(B=0), "bad shape"), (dict(Tk=0), "bad shape"),
        (dict(ldq=q.stride(1) + 2), "multiples of 4 floats"), (dict(q=p(q) + 4), "16-byte aligned"), (dict(window=-1), "window must be >= 0"),
        (dict(kv_dtype=3), "kv_dtype must be"), (dict(out=None), "null tensor"), (dict(k=None), "null tensor"),
    ]
    before = cache.clone()
    for kw, fragment in table:
        a = dict(base)
        a.update(kw)
        st = _lib.STRUCTS["mi355_flash_attn_args"](**{k: v for k, v in a.items() if v is not None})
        rc = lib.mi355_flash_attention(ctypes.byref(st), None)
        msg = lib.mi355_last_error().decode()
        assert rc == -1 and msg and fragment in msg, (kw, fragment, rc, msg)   # MI355_ERR_ARG
    sync()
    assert bool((out == S.SENTINEL).all()) and torch.equal(cache, before) and bool((pl == 0x1234).all()) and int(cnt.abs().sum()) == 0
