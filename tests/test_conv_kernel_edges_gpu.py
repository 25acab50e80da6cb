"""Dispatch-branch parity of ``mi355_conv_gemm``: the 4-wave kernels, split-K with both finish kernels and every instantiation of the wave-specialised
(ws4) kernel (csrc/conv_gemm.hip, conv_ws4.h, conv_ws4*.hip).

tests/test_kernels_gpu.py, test_conv_mx_gpu.py and test_transformer_kernels_gpu.py hold these kernels at the workloads' shapes with Gaussian inputs and one
number per tensor; this file walks the branches between those shapes with inputs on which ONE wrong element shows.  Case tables, the restated dispatcher
and scheduler, statements, mutants and bounds live in tests/_conv_cases.py; tests/test_conv_refs_cpu.py holds them on the CPU (exactness preconditions,
mutants, route coverage against the instantiation lists of the sources, the scheduler).

1. Exact cases: integer / dyadic operands make every partial sum exactly representable whatever the order, so EVERY route a case is eligible for must be
   bit-equal (``torch.equal``) to the float64 convolution.  The input buffer holds NaN in its pad columns and in the rows past an item's length; the
   output is the corner of a sentinel-filled buffer whose rows >= lens_out[b], columns >= Cout and guard row must come back untouched.
2. Float cases (transcendental prologues / epilogues): per element ``|got - want| <= bound`` (tests/_conv_cases.py) under the existing per-tensor caps;
   each test prints ``CONV <case> p<precision> tile <code> ratio=<largest error / bound>`` (``pytest -s``).
3. Bit equality between branches on the same inputs, float cases included: feature digits 1, 2, 8 against 0, tile 0 against the code it resolves to,
   128- against 64-column ws4 tiles, an item in a ragged batch against the item alone, a second run.
4. The persistent walk at small shapes under ``mi355_conv_ws4_resident(8 / 16)``, the glog boundaries, refusals, the ws4 fall-through.

WHICH kernel a launch runs is checked, not predicted: ``run()`` asks the library's own routing function (``ops.conv_route`` -> ``mi355_conv_gemm_route``:
the validation and decision steps ``mi355_conv_gemm`` itself goes through, then launches from) with the very tensors and keywords of the launch and asserts
its label and split-K group count against ``route()`` of tests/_conv_cases.py, so a case cannot silently run on another kernel than the one its coverage
is counted for.  tests/test_conv_refs_cpu.py holds ``route()`` to the same function on the CPU for every launch of the case tables (ws4 geometry included)
and its instantiation lists to the sources.  What stays unseen from here: the grid of a ws4 launch, sized at launch time from the CU count and
``mi355_conv_ws4_resident`` (``test_persistent_walk_small`` compares its effect).  The pair "feature digit 8 against 0" is two different launches only at
precisions 2, 5 and 6 -- the dispatcher masks that bit off at 1, 3 and 4 (``feat & 3``) -- where ``test_persistent_walk_small`` carries the
walk-against-one-workgroup-per-tile comparison instead.

The library's A/B knobs are read once per process: none may be set (asserted at import)."""
import os

import pytest
import torch
import torch.nn.functional as F

import _conv_cases as S

assert [k for k in S.ENV_KNOBS if k in os.environ] == [], "the A/B knobs of the conv kernels must be unset for this suite"

pytestmark = pytest.mark.gpu
DEV = "cuda"
_RESIDENT = [0]      # what this module last handed to mi355_conv_ws4_resident (process-wide setting)


@pytest.fixture(scope="module")
def ops():
    from mlx_audio_amd import ops as _ops

    _ops.require_gpu()
    return _ops


@pytest.fixture(scope="module", autouse=True)
def resident_restored(ops):
    yield
    assert _RESIDENT[0] == 0, "a test left mi355_conv_ws4_resident set"


@pytest.fixture
def resident(ops):
    """Setter of the process-wide persistent-workgroup share; 0 (two workgroups per CU) is restored whatever the test does."""
    lib = ops._lib.load()

    def set_(n):
        ops._lib.check(lib.mi355_conv_ws4_resident(int(n)), "mi355_conv_ws4_resident")
        _RESIDENT[0] = int(n)

    try:
        yield set_
    finally:
        lib.mi355_conv_ws4_resident(0)
        _RESIDENT[0] = 0


_DEV_CACHE = {}


def device_inputs(ops, c, prec):
    fl = S.case_flavour(c, prec)
    kind = "mx1" if prec == 5 else ("mx2" if prec == 6 else ("f16" if prec in (3, 4) else "bf16"))
    key = (c["name"], fl)
    if key not in _DEV_CACHE:
        inp = S.inputs(c, fl)
        B, L, Cin = c["B"], c["L"], c["Cin"]
        s0 = 1 if c["unaligned"] else 0
        ld = S.round_up(s0 + c["x_off"] + Cin, 4) + c["x_extra"]
        xb = torch.full((B, L, ld), float("nan"))
        for b, n in enumerate(c["lens"]):           # pad columns and the rows past an item's length hold NaN: the kernel must not let them in
            xb[b, :n, s0 + c["x_off"]: s0 + c["x_off"] + Cin] = inp["x"][b, :n]
        d = dict(x=xb.to(DEV)[:, :, s0: s0 + Cin], packs={})
        for k in ("res", "old", "colscale"):
            d[k] = None if inp[k] is None else inp[k].to(DEV)
        for k in ("sc_c", "sh_c", "alpha_c", "inv_beta_c"):
            d[k] = inp[k].float().to(DEV) if inp.get(k) is not None else None
        d["lens_in"] = torch.tensor(c["lens"], dtype=torch.int32, device=DEV)
        d["lens_out"] = torch.tensor(c["lens_out"], dtype=torch.int32, device=DEV)
        d["fq"] = torch.tensor([[127.0, 128.0]] * B, device=DEV) if c["fq"] else None
        _DEV_CACHE[key] = d
    d = _DEV_CACHE[key]
    if kind not in d["packs"]:
        inp = S.inputs(c, fl)
        d["packs"][kind] = ops.pack_conv(inp["w"].float(), inp["bias"], DEV, f16=kind == "f16", mx={"mx1": 1, "mx2": 2}.get(kind, False))
    return d, d["packs"][kind]


ACT = dict(NONE="ACT_NONE", LEAKY="ACT_LEAKY", SNAKE="ACT_SNAKE", SNAKEBETA="ACT_SNAKE", ELU="ACT_ELU")
POST = dict(none="ACT_NONE", leaky="ACT_LEAKY", gelu="ACT_GELU", silu="ACT_SILU", gelu_tanh="ACT_GELU_TANH")


def run(ops, c, prec, tile, only=None, extra=None):
    """One launch of the case -> per-item CPU outputs [lens_out[b], Cout]; asserts that everything outside them still holds the sentinel."""
    d, pc = device_inputs(ops, c, prec)
    items = list(range(c["B"])) if only is None else [only]
    sl = slice(None) if only is None else slice(only, only + 1)
    L, Cout = c["L"], c["Cout"]
    ldy = S.round_up(Cout, 4) + c["y_extra"]
    buf = torch.full((len(items), L + 1, ldy), S.SENTINEL, device=DEV)
    y = buf[:, :L, :Cout]
    if d["old"] is not None:
        for i, b in enumerate(items):
            y[i, :c["lens_out"][b]] = d["old"][b, :c["lens_out"][b]]
    kw = dict(dil=c["dil"], pad=c["pad"], lout=c["Lout"], precision=prec, tile=tile, x_off=c["x_off"], out_scale=c["out_scale"], accumulate=c["accumulate"],
              pre_act=getattr(ops, ACT[c["pre"]]), pre_slope=c["pre_slope"], post_act=getattr(ops, POST[c["post"]]), post_slope=c["post_slope"])
    if c["ragged"]:
        kw.update(lens_in=d["lens_in"][sl], lens_out=d["lens_out"][sl])
    if c["affine"]:
        kw.update(pre=(d["sc_c"][sl], d["sh_c"][sl]))
    if d["alpha_c"] is not None:
        kw.update(pre_alpha=d["alpha_c"], pre_inv_beta=d["inv_beta_c"])
    if d["res"] is not None:
        kw.update(res=d["res"][sl], res_shift=c["res_shift"])
    if d["colscale"] is not None:
        kw.update(colscale=d["colscale"])
    if d["fq"] is not None:
        kw.update(pre_fq=d["fq"][sl].contiguous())
    kw.update(extra or {})
    rec = ops.conv_route(d["x"][sl], pc, y, **kw)        # a host call: which kernel the library runs for exactly this launch
    lab, facts = S.route(S.case_launch(c, prec, tile, only=only))
    assert S.record_label(rec) == lab and rec["groups"] == (facts["groups"] if "splitk/" in lab else 0), (S.case_id(c), prec, tile, only, lab, rec)
    ops.conv_gemm(d["x"][sl], pc, y, **kw)
    torch.cuda.synchronize()
    out = buf.cpu()
    assert bool((out[:, L] == S.SENTINEL).all()) and bool((out[:, :, Cout:] == S.SENTINEL).all()), (S.case_id(c), prec, tile, "guard row / columns written")
    got = []
    for i, b in enumerate(items):
        n = c["lens_out"][b]
        assert bool((out[i, n:L] == S.SENTINEL).all()), (S.case_id(c), prec, tile, b, "rows past lens_out written")
        got.append(out[i, :n, :Cout].clone())
    return got


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def check_pairs(c, prec, outs, calls):
    """Bit equality between the branches of one case at one precision (``outs``: tile code -> outputs)."""
    labels = {t: (l, f) for t, l, f in calls}
    for base in (S.WS, S.WS64):
        for digit in (1, 2, 8):
            t = digit * 10000000 + base
            if t in outs and base in outs:
                assert same(outs[t], outs[base]), (S.case_id(c), prec, f"feature digit {digit} vs 0 on {base}")
    if 0 in outs:      # tile 0 against the explicit code route() says it resolves to
        lab0, f0 = labels[0]
        for t in outs:
            if t and t // 10000000 == 0 and labels[t][0] == lab0 and ("splitk" not in lab0 or labels[t][1] == f0):
                assert same(outs[t], outs[0]), (S.case_id(c), prec, f"tile 0 vs {t} ({lab0})")
    if S.WS in outs and S.WS64 in outs and c["Cout"] <= 64:
        assert same(outs[S.WS], outs[S.WS64]), (S.case_id(c), prec, "128- vs 64-column ws4 tiles")


# ----------------------------------------------------------------------------------------------------------------- 1. exact cases on every route
EXACT = S.exact_cases()


@pytest.mark.parametrize("c", EXACT, ids=S.case_id)
def test_exact_on_every_route(ops, c):
    for prec in c["precs"]:
        want = [w.float() for w in S.expected(c, prec)]
        calls = S.tile_calls(c, prec)
        outs = {}
        for tile, lab, _ in calls:
            outs[tile] = run(ops, c, prec, tile)
            for b, (g, w) in enumerate(zip(outs[tile], want)):
                assert torch.equal(g, w), (S.case_id(c), prec, tile, lab, b, int((g != w).sum()), float((g.double() - w.double()).abs().max()))
        check_pairs(c, prec, outs, calls)


# ----------------------------------------------------------------------------------------------------------------- 2. float cases
@pytest.mark.parametrize("c", S.float_cases(), ids=S.case_id)
def test_float_cases_per_element(ops, c):
    for prec in c["precs"]:
        want = S.expected(c, prec)
        bound, e32, peak = S.float_bound(c, prec)
        calls = S.tile_calls(c, prec)
        outs = {}
        for tile, lab, _ in calls:
            outs[tile] = run(ops, c, prec, tile)
            on_mx = lab.startswith("ws4/p5") or lab.startswith("ws4/p6")
            ref = want if (prec not in (5, 6) or on_mx) else S.statement(c, S.inputs(c, "m"))      # MX fallbacks run the precision-4 arithmetic
            bnd = bound if (prec not in (5, 6) or on_mx) else S.float_bound_p4_of_mx(c)
            ratio = worst = 0.0
            for b in range(c["B"]):
                if ref[b].numel():
                    err = (outs[tile][b].double() - ref[b]).abs()
                    ratio = max(ratio, float((err / bnd[b]).max()))
                    worst = max(worst, float(err.max()))
            print(f"CONV {S.case_id(c)} p{prec} tile {tile} {lab} ratio={ratio:.3f} worst={worst:.3e} peak={peak:.3e}")
            assert ratio <= 1.0, (S.case_id(c), prec, tile, lab, ratio)
            # the caps: the per-tensor bars of test_kernels_gpu.py / test_conv_mx_gpu.py, which are bars against the EXACT float64 convolution
            exact = ref if prec not in (5, 6) else S.statement(c, S.inputs(c, "m"))
            cap = max(float((outs[tile][b].double() - exact[b]).abs().max()) for b in range(c["B"]) if exact[b].numel())
            assert cap <= S.TILE_CAPS[prec if on_mx or prec < 5 else 4] * peak, (S.case_id(c), prec, tile, cap / peak)
        check_pairs(c, prec, outs, calls)


# ----------------------------------------------------------------------------------------------------------------- 3. an item alone, a second run
RAGGED = [c for c in S.exact_cases() + S.float_cases() if c["ragged"]]


@pytest.mark.parametrize("c", RAGGED, ids=S.case_id)
def test_item_alone_and_second_run(ops, c):
    for prec in c["precs"]:
        calls = [t for t, lab, _ in S.tile_calls(c, prec) if lab.startswith("ws4/") and t // 10000000 == 0]
        for tile in calls[:2]:
            batch = run(ops, c, prec, tile)
            assert same(run(ops, c, prec, tile), batch), (S.case_id(c), prec, tile, "second run")
            for b in range(c["B"]):
                if c["lens_out"][b] and S.route(S.case_launch(c, prec, tile, only=b))[0].startswith("ws4/"):
                    alone = run(ops, c, prec, tile, only=b)
                    assert torch.equal(alone[0], batch[b]), (S.case_id(c), prec, tile, b, "item alone vs in the batch")


# ----------------------------------------------------------------------------------------------------------------- 4. the persistent walk, glog
@pytest.mark.parametrize("c", S.walk_cases(), ids=S.case_id)
def test_persistent_walk_small(ops, resident, c):
    """9 .. 40 virtual ids on 8 / 16 persistent workgroups == one workgroup per tile == the exact result."""
    for prec in c["precs"]:
        want = [w.float() for w in S.expected(c, prec)]
        for tile in c["tiles"]:
            lab, f = S.route(S.case_launch(c, prec, tile))
            if not lab.startswith("ws4/"):
                continue
            assert not f["walk"]
            resident(0)
            base = run(ops, c, prec, tile)
            assert same(base, want), (S.case_id(c), prec, tile, "one workgroup per tile")
            for n in (8, 16):
                resident(n)
                got = run(ops, c, prec, tile)
                resident(0)
                assert same(got, base), (S.case_id(c), prec, tile, f"{n} resident workgroups")


@pytest.mark.parametrize("c", S.glog_cases(), ids=S.case_id)
def test_glog_boundaries(ops, c):
    for prec in c["precs"]:
        want = [w.float() for w in S.expected(c, prec)]
        for tile, lab, f in S.tile_calls(c, prec):
            assert not tile or (lab.startswith("ws4/") and f["glog"] == c["claims"]["glog"])     # (tile 0 below 128 tiles: a 4-wave launch)
            assert same(run(ops, c, prec, tile), want), (S.case_id(c), prec, tile)


# ----------------------------------------------------------------------------------------------------------------- 4. fused statistics
@pytest.mark.parametrize("c", S.stats_cases(), ids=S.case_id)
def test_fused_statistics_on_integer_outputs(ops, c):
    """stats_partial of an exact case: the stored output stays bit-equal, and per 64-row block and channel (sum, M2) of the VALID rows agree with float64.
    The kernels keep (count, mean, M2) per lane about a shift (the lane's first value) and merge them with Chan's formula, sum = mean x count: every
    rounding is relative to a partial sum (<= sum |y|) or to count x shift (<= 64 max |y|), at most 16 of them on the way to one sum --
    sum: 2^-20 (sum |y| + 64 max |y|); M2, the float bound: 2^-18 sum y^2 (no merge of partial M2s exceeds it).  Blocks past an item's last row keep the
    sentinel or hold the (0, 0) of an empty block; the guard block behind the buffer keeps the sentinel."""
    nblk = (c["L"] + 63) // 64
    for prec in c["precs"]:
        want = S.expected(c, prec)
        for tile, lab, _ in S.tile_calls(c, prec):
            st = torch.full((c["B"], nblk + 1, c["Cout"], 2), S.SENTINEL, device=DEV)
            got = run(ops, c, prec, tile, extra=dict(stats=st))
            assert same(got, [w.float() for w in want]), (S.case_id(c), prec, tile, lab)
            raw = st.cpu()
            stc = raw.double()
            worst = 0.0
            for b, n in enumerate(c["lens_out"]):
                live = (n + 63) // 64
                for blk in range(live):
                    v = want[b][blk * 64: min(n, blk * 64 + 64)]
                    s_want, m2_want = v.sum(0), ((v - v.mean(0)) ** 2).sum(0)
                    bs = 2.0 ** -20 * (v.abs().sum(0) + 64.0 * v.abs().max(0).values) + 1e-30
                    bm = 2.0 ** -18 * (v ** 2).sum(0) + 1e-30
                    worst = max(worst, float(((stc[b, blk, :, 0] - s_want).abs() / bs).max()), float(((stc[b, blk, :, 1] - m2_want).abs() / bm).max()))
                dead = raw[b, live:nblk]
                assert bool(((dead == S.SENTINEL) | (dead == 0)).all()), (S.case_id(c), prec, tile, lab, b, "a block past the item's end holds statistics")
                assert bool((raw[b, nblk] == S.SENTINEL).all()), (S.case_id(c), prec, tile, lab, b, "guard block written")
            print(f"CONV stats {S.case_id(c)} p{prec} tile {tile} {lab} ratio={worst:.3f}")
            assert worst <= 1.0, (S.case_id(c), prec, tile, lab, worst)


# ----------------------------------------------------------------------------------------------------------------- 4. polyphase store
@pytest.mark.parametrize("tile", [0, S.WS, 80000000 + S.WS, 128128, 2064128])
@pytest.mark.parametrize("prec", [2, 4])
def test_polyphase_store_exact(ops, tile, prec):
    """conv_transpose as a polyphase conv (up_s, up_row_off, lens_up) behind a LeakyReLU(0.25) prologue on integers: bit-equal to conv_transpose1d in
    float64; the row in front of the slot (row_off), the rows past lens_up[b] and the guard row keep the sentinel.  Item 0 has interior tiles (the
    polyphase fast epilogue), item 1 is short."""
    g = torch.Generator().manual_seed(17)
    cin, cout, k, s, B, L, row_off = 128, 32, 8, 4, 2, 300, 1
    lens = [300, 77]
    p, kp = (k - s) // 2, k // s
    w_t = torch.randint(-4, 5, (cout, k, cin), generator=g).float()
    bias = torch.randint(-8, 9, (cout,), generator=g).float()
    t = torch.randint(-4, 5, (B, L, cin), generator=g).float()
    wide = torch.rand((B, L, cin), generator=g) < 0.01
    t = torch.where(wide, (2049.0 + 2.0 * torch.randint(0, 1024, (B, L, cin), generator=g)) * torch.where(torch.rand((B, L, cin), generator=g) < 0.5, -1.0, 1.0), t)
    x = torch.where(t < 0, t * 4.0, t)
    lout = (L - 1) * s - 2 * p + k
    lens_up = [(n - 1) * s - 2 * p + k for n in lens]
    res = torch.randint(-8, 9, (B, lout + row_off, cout), generator=g).float()
    pc = ops.pack_conv_transpose(w_t, bias, s, DEV, f16=prec == 4)
    xb = torch.full((B, L, cin), float("nan"))
    for b, n in enumerate(lens):
        xb[b, :n] = x[b, :n]
    buf = torch.full((B, lout + row_off + 1, cout + 4), S.SENTINEL, device=DEV)
    y = buf[:, : lout + row_off, :cout]
    ops.conv_gemm(xb.to(DEV), pc, y, pad=kp - 1, lout=L + kp - 1, pre_act=ops.ACT_LEAKY, pre_slope=0.25, res=res.to(DEV), precision=prec, tile=tile,
                  lens_in=torch.tensor(lens, dtype=torch.int32, device=DEV), lens_out=torch.tensor([n + kp - 1 for n in lens], dtype=torch.int32, device=DEV),
                  up=dict(s=s, p=p, cout=cout, row_off=row_off, lout=lout, lens=torch.tensor(lens_up, dtype=torch.int32, device=DEV)))
    torch.cuda.synchronize()
    out = buf.cpu()
    for b, n in enumerate(lens):
        want = F.conv_transpose1d(t[b, :n].double().t()[None], w_t.permute(2, 0, 1).double(), bias.double(), stride=s, padding=p)[0].t()
        assert want.shape[0] == lens_up[b]
        want = (want + res[b, row_off: row_off + lens_up[b]].double()).float()
        got = out[b, row_off: row_off + lens_up[b], :cout]
        assert torch.equal(got, want), (b, int((got != want).sum()))
        assert bool((out[b, :row_off] == S.SENTINEL).all()) and bool((out[b, row_off + lens_up[b]:] == S.SENTINEL).all()) and bool((out[b, :, cout:] == S.SENTINEL).all())


# ----------------------------------------------------------------------------------------------------------------- 4. refusals, fall-through
def test_refusals_leave_outputs_untouched(ops, monkeypatch):
    """Every MI355_REQUIRE of mi355_conv_gemm a Python caller can reach raises and leaves y, stats and ext untouched."""
    g = torch.Generator().manual_seed(3)
    B, L, C = 1, 200, 128
    w = torch.randint(-4, 5, (C, 5, 64), generator=g).float()
    x = torch.randint(-4, 5, (B, L, 64), generator=g).float().to(DEV)
    pcs = dict(bf16=ops.pack_conv(w, None, DEV), f16=ops.pack_conv(w, None, DEV, f16=True), mx=ops.pack_conv(w[:, :3].contiguous(), None, DEV, mx=1))
    mm = torch.tensor([[127.0, 128.0]], device=DEV)
    orig = ops._lib.call_struct
    override = {}
    monkeypatch.setattr(ops._lib, "call_struct", lambda fn, sn, st, **kw: orig(fn, sn, st, **{**kw, **override}))
    sbuf = torch.full((B * 4 * C * 2 + 1,), S.SENTINEL, device=DEV)
    stats_odd = sbuf[1:].view(B, 4, C, 2)            # 4 bytes past an 8-byte boundary
    stats_ok = torch.full((B, 4, C, 2), S.SENTINEL, device=DEV)
    ext = torch.full((B, 4, C, 2), S.SENTINEL, device=DEV)
    table = [
        ("the explicit ws4 tile with a window > 192", "bf16", dict(tile=S.WS, dil=17, pad=34), {}, "window"),
        ("the explicit 64-column ws4 tile with a window > 192", "bf16", dict(tile=S.WS64, dil=17, pad=34), {}, "window"),
        ("the MX image on the 64-column tile", "mx", dict(tile=S.WS64, pad=1), {}, "MX"),
        ("split-K without a workspace", "bf16", dict(tile=2064128, pad=2), dict(split_ws=None, split_ws_bytes=0), "workspace"),
        ("precision 5 with pre_fq", "mx", dict(pad=1, pre_fq=mm), {}, "quantising"),
        ("x_split != precision", "bf16", dict(pad=2, x_split=True), dict(x_split=4), "x_split"),
        ("y_split with accumulate", "bf16", dict(pad=2, y_split=True, accumulate=True), {}, "y_split"),
        ("stats not 8-byte aligned", "bf16", dict(pad=2, stats=stats_odd), {}, "aligned"),
        ("a polyphase store with stats", "bf16", dict(pad=2, stats=stats_ok, up=dict(s=2, p=0, cout=C // 2, lout=2 * L)), {}, "statistics"),
        ("ext on a launch that cannot write it", "bf16", dict(pad=2, ext=ext), {}, "ext_partial"),
        ("a quantising prologue behind ELU", "bf16", dict(pad=2, pre_fq=mm, pre_act=ops.ACT_ELU), {}, "quantising"),
    ]
    for what, pk, kw, ov, word in table:
        y = torch.full((B, L, C), S.SENTINEL, device=DEV)
        override.clear()
        override.update(ov)
        with pytest.raises(ops._lib.Mi355Error) as e:
            ops.conv_gemm(x, pcs[pk], y, **kw)
        torch.cuda.synchronize()
        assert word in str(e.value), (what, str(e.value))
        assert bool((y == S.SENTINEL).all()) and bool((sbuf == S.SENTINEL).all()) and bool((stats_ok == S.SENTINEL).all()) and bool((ext == S.SENTINEL).all()), what
    override.clear()


@pytest.mark.parametrize("prec", [1, 3])
def test_ws4_unsupported_falls_through_to_the_4wave_route(ops, prec):
    """An ELU prologue has no precision-1 / 3 ws4 instantiation: tile 0 with >= 128 tiles takes mi355_conv_ws4_route's MI355_ERR_UNSUPPORTED and must land
    on the 4-wave kernel route() names, with the right result and no error left behind.  Strictly positive integers: ELU is the identity on them, so the
    result is exact."""
    g = torch.Generator().manual_seed(9)
    B, L, Cin, Cout, K = 130, 5, 64, 128, 3
    a = S.launch(B=B, L=L, Cin=Cin, Cout=Cout, K=K, pad=1, pre="ELU", precision=prec)
    assert S.ws4_eligible(a, prec) and S.ws4_launch(a, prec, 0, 128) is None and S.route(a)[0] == f"4wave/p{prec}/64x128/vec"
    x = torch.randint(1, 5, (B, L, Cin), generator=g).float()
    w = torch.randint(-4, 5, (Cout, K, Cin), generator=g).float()
    pc = ops.pack_conv(w, None, DEV, f16=prec == 3)
    y = torch.full((B, L, Cout), S.SENTINEL, device=DEV)
    ops.conv_gemm(x.to(DEV), pc, y, pad=1, pre_act=ops.ACT_ELU, precision=prec)
    explicit = torch.full((B, L, Cout), S.SENTINEL, device=DEV)
    ops.conv_gemm(x.to(DEV), pc, explicit, pad=1, pre_act=ops.ACT_ELU, precision=prec, tile=64128)
    torch.cuda.synchronize()
    want = torch.stack([S.conv_rows(x[b].double(), w.double(), 1, 1, L) for b in range(B)]).float()
    assert torch.equal(y.cpu(), want) and torch.equal(explicit.cpu(), want)
