"""CPU half of the attention branch parity suite (tests/_attn_cases.py): the statements are held to torch, the case tables are held to the launch
sites of csrc/flash_attn.hip, every structured generator's precondition is checked, and mutants of the statement show that the named cases
would catch them by more than their bounds."""
import math

import pytest
import torch
import torch.nn.functional as F

import _attn_cases as S

ALL = S.decode_cases() + S.flash_cases() + S.fused_cases()
BY_NAME = {c["name"]: c for c in ALL}


def test_names_are_unique_and_tables_are_small():
    assert len(BY_NAME) == len(ALL)
    for c in ALL:
        assert c["B"] <= 4 and c["H"] <= 4 and c["H"] % c["G"] == 0, c["name"]
    for fam in ("decode", "flash", "fused"):
        assert any(c["fam"] == fam and c["H"] > c["G"] for c in ALL)


# ------------------------------------------------------------------------------------------------------------ statements held to torch
def _sdpa(q, k, v, c):
    B, Tq, Tk, H, G, dh = c["B"], c["Tq"], c["Tk"], c["H"], c["G"], c["dh"]
    out = torch.zeros(B, Tq, H * dh, dtype=torch.float64)
    lq_, lk_, ks_ = S._lens(c, "lens_q", Tq), S._lens(c, "lens_k", Tk), S._lens(c, "k_start", 0)
    for b in range(B):
        lq, lk = lq_[b], lk_[b]
        if lq == 0 or lk == 0:
            continue
        mask = S.visible(lq, lk, ks_[b], c["causal"], c["window"])
        qq = q[b, :lq].double().reshape(lq, H, dh).transpose(0, 1)
        kk = k[b, :lk].double().reshape(lk, G, dh).transpose(0, 1).repeat_interleave(H // G, 0)
        vv = v[b, :lk].double().reshape(lk, G, dh).transpose(0, 1).repeat_interleave(H // G, 0)
        o = F.scaled_dot_product_attention(qq[None], kk[None], vv[None], attn_mask=mask[None, None])[0]
        out[b, :lq] = o.transpose(0, 1).reshape(lq, H * dh)
    return out


def _all_see(c):
    lq_, lk_, ks_ = S._lens(c, "lens_q", c["Tq"]), S._lens(c, "lens_k", c["Tk"]), S._lens(c, "k_start", 0)
    return all(lq == 0 or (lk > 0 and bool(S.visible(lq, lk, ks, c["causal"], c["window"]).any(1).all())) for lq, lk, ks in zip(lq_, lk_, ks_))


SDPA_CASES = [c for c in ALL if c["fam"] != "fused" and c["kind"] == "random" and c["Tk"] <= 300 and _all_see(c)]


def test_statement_equals_sdpa():
    assert len(SDPA_CASES) > 40
    for c in SDPA_CASES:
        x = S.make_inputs(c)
        got, want = S.attn_stmt(x["q"], x["k"], x["v"], c), _sdpa(x["q"], x["k"], x["v"], c)
        assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max())), c["name"]


def test_statement_equals_ref_attention_of_the_transformer_suite():
    import test_transformer_kernels_gpu as T

    for (B, Tq, Tk, heads, kvh, dh, causal, window, ragged, mode) in T.ATT_CASES:
        g = torch.Generator().manual_seed(Tq * 7 + Tk + heads)
        q, k, v = (torch.randn(B, n, w, generator=g) for n, w in ((Tq, heads * dh), (Tk, kvh * dh), (Tk, kvh * dh)))
        lens_q = lens_k = None
        if ragged:
            lens_k = [max(1, Tk - 13 * i) for i in range(B)]
            lens_q = [min(Tq, lens_k[i]) - (i % 2) * min(2, Tq - 1) for i in range(B)]
        c = dict(B=B, Tq=Tq, Tk=Tk, H=heads, G=kvh, dh=dh, causal=causal, window=window, lens_q=lens_q, lens_k=lens_k, k_start=None, kv="f32")
        want = T.ref_attention(q, k, v, heads, kvh, dh, dh ** -0.5, causal, window, lens_q, lens_k)
        assert float((S.attn_stmt(q, k, v, c) - want).abs().max()) <= 1e-12


def test_fused_statement_equals_torch_norm_rope_then_plain_statement():
    from oracle.lm_ref import apply_rope

    for c in S.fused_cases():
        x = S.fused_inputs(c)
        B, Tk, H, G, dh = c["B"], c["Tk"], c["H"], c["G"], c["dh"]
        out, k_new, v_new, _ = S.fused_stmt(x, c)
        acc = x["slabs"].double().sum(0)
        parts = {}
        for name, lo, hi in (("q", 0, H * dh), ("k", H * dh, (H + G) * dh), ("v", (H + G) * dh, (H + 2 * G) * dh)):
            t = acc[:, lo:hi]
            if x.get(name + "_wscale") is not None:
                t = t * x[name + "_wscale"].double()
            if x.get(name + "_bias") is not None:
                t = t + x[name + "_bias"].double()
            parts[name] = t
        res = {}
        for name, heads, w in (("q", H, x["qw"]), ("k", G, x["kw"])):
            t = parts[name].reshape(B, 1, heads, dh)
            if w is not None:
                t = F.rms_norm(t, (dh,), w.double(), eps=1e-6)
            if x.get("cos") is not None:
                rows = []
                for b in range(B):
                    pos = min(max(S.fused_position(c, b), 0), x["cos"].shape[0] - 1)
                    rows.append(apply_rope(t[b:b + 1], x["cos"][pos:pos + 1].double(), x["sin"][pos:pos + 1].double(), c["rope_mode"] == 1))
                t = torch.cat(rows)
            res[name] = t.reshape(B, heads * dh)
        kr, vr = S.rnd(res["k"], c["kv"]).double(), S.rnd(parts["v"], c["kv"]).double()
        ck, cv = x["cache_k"].double().clone(), x["cache_v"].double().clone()
        for b, lk in enumerate(S._lens(c, "lens_k", Tk)):
            ck[b, lk - 1], cv[b, lk - 1] = kr[b], vr[b]
        want = S.attn_stmt(res["q"][:, None, :], ck, cv, dict(c, Tq=1, lens_q=None))
        tol = 1e-9 if c["kv"] == "f32" else 2e-2   # (a float64 difference of 1e-16 may cross a rounding boundary of the 16-bit k row)
        assert float((out - want).abs().max()) <= tol and float((k_new - kr).abs().max()) <= tol and torch.equal(v_new, vr), c["name"]
        assert torch.equal(vr, parts["v"]), "the v row of every fused case is exact in the cache type"


def test_random_case_bounds_sit_under_the_existing_bars():
    n = 0
    for c in ALL:
        if c["fam"] == "fused" or c["kind"] != "random" or c["Tk"] > 300:
            continue
        x = S.make_inputs(c)
        ref, bound = S.attn_bound(x["q"], x["k"], x["v"], c, c["kernel"])
        if float(ref.abs().max()) > 0:
            assert float(bound.max()) <= S.existing_bar(c, c["kernel"]) * float(ref.abs().max()) * (1 + 1e-12), c["name"]
            n += 1
    assert n > 100


# ------------------------------------------------------------------------------------------------------------ coverage
def test_every_instantiation_and_every_flag_is_some_cases_route():
    sites = S.launch_sites()
    assert len(sites) == 24, sites
    want = {f"flash_attn_kernel<{dh}, 0>" for dh in (64, 128)} | {f"flash_attn16_kernel<{dh}, {t}>" for dh in (64, 128) for t in (1, 2)} \
        | {f"attn_decode_kernel<{dh}, {nw}, {t}>" for dh in (64, 128) for nw in (1, 4, 16) for t in (0, 1, 2)}
    assert set(sites) == want
    routes = {}
    for c in ALL:
        r = S.case_route(c)
        assert r[0] == c["kernel"], (c["name"], r, c["kernel"])   # the hand-written kernel of the table against the restated dispatcher
        routes.setdefault(r[0], []).append(c)
    assert set(routes) == want, want - set(routes)
    flags = set().union(*(S.case_route(c)[1] for c in ALL))
    assert flags == set(S.FLAGS), set(S.FLAGS) - flags
    for fam in ("decode", "flash", "fused"):   # per family, every (dh, type)
        assert {(c["dh"], c["kv"]) for c in ALL if c["fam"] == fam} == set(S.TYPES)
    fused = {(c["kernel"]) for c in ALL if c["fam"] == "fused"}
    assert len(fused) == 18
    assert {c.get("in_kgroups") for c in S.fused_cases()} >= {1, 2, 4, 5, 9} and {c["planes_R"] for c in S.fused_cases()} >= {16, 32, 64}
    assert {(c["planes_f16"], c["planes_R"]) for c in S.fused_cases() if c["planes_R"]} >= {(f, r) for f in (False, True) for r in (16, 32, 64)}


def test_route_clamps_and_switches():
    base = dict(mode=0, Tq=1, Tk=1025, kv="f32", dh=64, nsplit=9, ws=True)
    assert S.route(base) == ("attn_decode_kernel<64, 16, 0>", frozenset({"split"}))
    assert S.route(dict(base, ws=False))[1] == frozenset()                               # no workspace, no split
    assert S.route(dict(base, nsplit=0))[1] == frozenset()                               # the split is opt-in
    assert S.route(dict(base, fused=True))[1] == frozenset({"fused"})                    # new_k forces nsplit = 1
    assert S.route(dict(base, Tk=64, nsplit=2))[0] == "attn_decode_kernel<64, 4, 0>"     # a split range never takes the one-wave kernel
    assert S.route(dict(base, Tk=64, nsplit=1))[0] == "attn_decode_kernel<64, 1, 0>"
    assert S.route(dict(base, Tq=9))[0] == "flash_attn_kernel<64, 0>" and S.route(dict(base, Tq=9, mode=2))[0].startswith("attn_decode")
    assert S.route(dict(base, mode=1, kv="f16", dh=128))[0] == "flash_attn16_kernel<128, 2>"


# ------------------------------------------------------------------------------------------------------------ generator preconditions
def test_uniform_cases_are_integer_exact():
    n_cases = 0
    for c in ALL:
        if c["kind"] != "uniform":
            continue
        n_cases += 1
        x = S.make_inputs(c)
        assert not bool(x["q"].any()) and torch.equal(x["v"], x["v"].round()) and float(x["v"].abs().sum(1).max()) < 2 ** 24
        assert torch.equal(S.rnd(x["v"], c["kv"]), x["v"])
        cnt, n = S.uniform_expect(c, x["v"])
        want = torch.where(n[:, :, None] > 0, cnt / n.clamp(min=1)[:, :, None].double(), torch.zeros_like(cnt))
        assert float((S.attn_stmt(x["q"], x["k"], x["v"], c) - want).abs().max()) < 1e-13
        # one key more or less visible changes some count by at least 1: the count is what the case pins
        assert int(n.max()) >= 1 and float(cnt.max()) >= 1
    assert n_cases >= 15


def test_monotone_cases_move_the_block_maximum_as_named():
    seen = set()
    for c in ALL:
        if not c["kind"].startswith("mono"):
            continue
        x = S.make_inputs(c)
        for moves in S.block_max_moves(c, x["q"], x["k"]):
            assert moves[0] and len(moves) >= 4
            assert all(moves[1:]) if c["kind"] == "mono_up" else not any(moves[1:]), (c["name"], moves)
        s = (x["k"][0, :, :c["dh"]] @ x["q"][0, 0, :c["dh"]]) * c["dh"] ** -0.5
        assert 85.0 < float(s.max() - s.min()) < 95.0 and bool(torch.isinf(torch.exp(s.float().max())))   # overflows without the max subtraction
        seen.add((c["kind"], c["kernel"].split("<")[0]))
    assert {("mono_up", "flash_attn16_kernel"), ("mono_down", "flash_attn16_kernel")} <= seen


def test_offset_cases_overflow_without_the_max_subtraction():
    for c in ALL:
        if not c["kind"].startswith("offset"):
            continue
        x = S.make_inputs(c)
        s = (x["k"][0, :, :c["dh"]] @ x["q"][0, 0, :c["dh"]]) * c["dh"] ** -0.5
        assert 75.0 < abs(float(s.mean())) < 85.0
        e = torch.exp(s.float()).sum() * torch.exp(s.float()).sum()   # exp(160) / exp(-160): a float32 softmax that forms exp(s) and squares or
        assert bool(torch.isinf(e)) or float(e) == 0.0                  # multiplies two of them leaves the range; the monotone cases reach exp(90) = inf
        assert math.isfinite(float(S.attn_stmt(x["q"], x["k"], x["v"], c).abs().max()))


def test_poison_sits_only_in_invisible_rows():
    n_big = 0
    for c in ALL:
        if c["fam"] == "fused":
            continue
        nan_rows, big_rows = S.poison_plan(c)
        lq_, lk_, ks_ = S._lens(c, "lens_q", c["Tq"]), S._lens(c, "lens_k", c["Tk"]), S._lens(c, "k_start", 0)
        for b in range(c["B"]):
            assert bool(nan_rows[b, lk_[b]:].all()) and not bool(nan_rows[b, :lk_[b]].any()) and not bool(big_rows[b, lk_[b]:].any())
            if lq_[b] > 0 and lk_[b] > 0:
                seen = S.visible(lq_[b], lk_[b], ks_[b], c["causal"], c["window"]).any(0)
                assert not bool((big_rows[b, :lk_[b]] & seen).any())
        n_big += int(big_rows.sum() > 0)
        if c["Tk"] <= 140 and c["kind"] == "random":   # the statement itself masks them: same result on the poisoned buffers
            x = S.make_inputs(c)
            kp, vp = S.apply_poison(c, x["k"], x["v"])
            assert torch.equal(S.attn_stmt(x["q"], kp[:, :c["Tk"]], vp[:, :c["Tk"]], c), S.attn_stmt(x["q"], x["k"], x["v"], c)), c["name"]
    assert n_big >= 25


# ------------------------------------------------------------------------------------------------------------ mutants
def _ratio(c, variant):
    x = S.make_inputs(c)
    ref, bound = S.attn_bound(x["q"], x["k"], x["v"], c, c["kernel"])
    mut = S.attn_stmt(x["q"], x["k"], x["v"], c, variant=variant)
    rows = S.valid_rows(c)[:, :, None].expand_as(ref)
    return float(((mut - ref).abs() / bound)[rows].max())


@pytest.mark.parametrize("variant,names", [
    ("window_wide", ["win33-128f32", "win5-k131", "win1-64f32", "win64u-64bf16"]),
    ("window_narrow", ["win33-128f32", "win5-k131", "win65-128f16", "win64u-64bf16"]),
    ("no_causal_offset", ["f64f32-q32-k33", "d64f32-k64-q8", "ragged"]),
    ("no_k_start", ["kstart0-64f32", "kstart1", "uniform3"]),
    ("gqa_mod", ["ragged-64f32", "ragged", "hm-128f16"]),
    ("c_row_identity", ["f64f32-q33-k63", "f128f32-q33-k129", "f64bf16-q33-k65", "f128f16-q33-k33"]),
])
def test_statement_mutants_are_caught(variant, names):
    for n in names:
        r = _ratio(BY_NAME[n], variant)
        print(f"ATTN mutant {variant} {n} ratio={r:.3g}")
        assert r > 1.0, (variant, n, r)


def test_uniform_cases_catch_one_key():
    """one wrongly visible key moves a uniform case by a whole count: far outside 2 ulp"""
    c = BY_NAME["win32u-128f16"]
    x = S.make_inputs(c)
    cnt, n = S.uniform_expect(c, x["v"])
    mut = S.attn_stmt(x["q"], x["k"], x["v"], c, variant="window_wide")
    want = cnt / n.clamp(min=1)[:, :, None]
    assert float((mut - want).abs().max()) > 1e-3


def test_c_row_identity_mutant():
    """the tile restated: register r of half-wave `half` holds key attn_c_row(r, half); feeding P to the second contraction in register order
    instead pairs probabilities with the wrong value rows"""
    g = torch.Generator().manual_seed(3)
    p = torch.softmax(torch.randn(32, generator=g, dtype=torch.float64) * 3, 0)
    v = torch.randn(32, 64, generator=g, dtype=torch.float64)
    c_row = lambda r, half: (r & 3) + 8 * (r >> 2) + 4 * half
    assert sorted(c_row(r, h) for r in range(16) for h in (0, 1)) == list(range(32))
    tile = sum(p[c_row(r, h)] * v[c_row(r, h)] for r in range(16) for h in (0, 1))
    ident = sum(p[c_row(r, h)] * v[r + 16 * h] for r in range(16) for h in (0, 1))
    assert float((tile - p @ v).abs().max()) < 1e-14
    assert float((ident - p @ v).abs().max()) > 1e-2 * float((p @ v).abs().max())


@pytest.mark.parametrize("name", ["f64bf16-q33-k65", "f128f16-q33-k33", "f64f16-q33-k127"])
def test_dropped_lo_image_of_q_is_caught(name):
    c = BY_NAME[name]
    x = S.make_inputs(c)
    ref, bound = S.attn_bound(x["q"], x["k"], x["v"], c, c["kernel"])
    sc = c["dh"] ** -0.5 * 1.4426950408889634
    q_hi = (x["q"] * sc).to(S.KV[c["kv"]]).float() / sc   # the hi image alone
    mut = S.attn_stmt(q_hi, x["k"], x["v"], c)
    r = float(((mut - ref).abs() / bound).max())
    print(f"ATTN mutant q_lo_dropped {name} ratio={r:.3g}")
    assert r > 1.0


def _fused_case(pred):
    return next(c for c in S.fused_cases() if pred(c))


def test_fused_mutants_are_caught():
    # bias before scale
    c = _fused_case(lambda c: c["bias"] and c["wscale"])
    x = S.fused_inputs(c)
    o64, k64, v64, ob, kb = S.fused_bound(x, c)
    om, km, vm, _ = S.fused_stmt(x, c, variant="bias_first")
    assert float(((om - o64).abs() / ob).max()) > 1.0 and float(((km - k64).abs() / kb).max()) > 1.0 and not torch.equal(vm, v64)
    # rope position without - k_start
    c = _fused_case(lambda c: c["k_start"] is not None and c["rope_mode"] is not None)
    x = S.fused_inputs(c)
    o64, k64, v64, ob, kb = S.fused_bound(x, c)
    om, km, _, _ = S.fused_stmt(x, c, variant="rope_no_k_start")
    assert float(((km - k64).abs() / kb)[1].max()) > 1.0 and float(((km - k64).abs() / kb)[0].max()) <= 1.0   # item 1 is the padded one
    # slab order reversed, on values whose float32 sum depends on the order: the float32 twin in the kernel's order is exact, reversed it is not
    c = _fused_case(lambda c: c["in_kgroups"] == 4 and not c["wscale"])
    x = S.fused_inputs(c)
    nq = c["H"] * c["dh"]
    small = torch.randint(1, 9, (c["B"], nq)).float()
    x["slabs"][0, :, :nq], x["slabs"][1, :, :nq], x["slabs"][2, :, :nq], x["slabs"][3, :, :nq] = 2.0 ** 26, -2.0 ** 26, small, 0.0
    o64, _, _, ob, _ = S.fused_bound(x, c)
    o32 = S.fused_stmt(x, c, torch.float32)[0].double()
    o32r = S.fused_stmt(x, c, torch.float32, variant="slab_reversed")[0].double()
    assert float(((o32 - o64).abs() / ob).max()) <= 1.0 and float(((o32r - o64).abs() / ob).max()) > 1.0


def test_planes_decoder_and_its_mutant():
    g = torch.Generator().manual_seed(11)
    for f16 in (False, True):
        for R in (16, 32, 64):
            rows = 1.0 + 6.0 * torch.rand(3, 256, generator=g)
            pl = S.encode_planes(rows, R, f16)
            hi, lo = S.decode_planes(pl, R, 256, f16)
            assert torch.equal(hi[:3].float(), rows.to(torch.float16 if f16 else torch.bfloat16).float()) and not bool(hi[3:].any())
            assert bool(((hi + lo)[:3] - rows.double()).abs().le(S.PLANES_EPS[f16] * rows.double().abs()).all())
            hs, ls = S.decode_planes(pl, R, 256, f16, variant="planes_swapped")
            assert float(((hs + ls)[:3] - rows.double()).abs().max()) > 0.1
    # the order itself, against the store of attn_decode_kernel: lane c of head h builds channels 8 c .. 8 c + 7 of column k = h * dh + 8 c
    k = torch.arange(0, 256, 8)
    s, gq, hh = k >> 6, (k & 63) >> 4, (k >> 3) & 1
    R, b = 16, 2
    idx = (((s * 2 + 0) * 2 + hh) * 4 + gq) * R + b   # uint4 index of the hi piece
    img = torch.zeros(2 * R * 256, dtype=torch.bfloat16)
    for piece, kk in zip(idx.tolist(), k.tolist()):
        img[piece * 8: piece * 8 + 8] = torch.arange(kk, kk + 8).to(torch.bfloat16)
    hi, _ = S.decode_planes(img.view(torch.int16), R, 256, False)
    assert torch.equal(hi[b], torch.arange(256).double())
