"""Everything about the conv-kernel suite that can be checked without a GPU (tests/_conv_cases.py; the GPU half is tests/test_conv_kernel_edges_gpu.py):
the statements against torch's own conv1d, the exactness preconditions of the exact cases (the CPU proof that a GPU mismatch is the kernel's), the mutants,
route coverage against the instantiation lists parsed from the sources, route() against the library's own routing function (``mi355_conv_gemm_route``, which
needs no device) launch by launch, the claimed branch facts, and the tile scheduler."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _conv_cases as S
from oracle import mx_ref

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "mlx_audio_amd", "csrc")
EXACT = S.exact_cases() + S.glog_cases() + S.walk_cases() + S.stats_cases()
FLOAT = S.float_cases()


def _torch_conv(t, w, dil, pad, n_out):
    """F.conv1d in float64 on one item: t [n, Cin] -> [n_out, Cout] (rows past the input are zero padding)."""
    K = w.shape[1]
    right = max(0, n_out - 1 - pad + (K - 1) * dil - (t.shape[0] - 1))
    xp = F.pad(t.t()[None].double(), (pad, right))
    return F.conv1d(xp, w.permute(0, 2, 1).double(), None, dilation=dil)[0].t()[:n_out]


# ----------------------------------------------------------------------------------------------------------------- statements
@pytest.mark.parametrize("c", EXACT + FLOAT, ids=S.case_id)
def test_statement_is_torch_conv1d(c):
    for fl in S.flavours(c):
        inp = S.inputs(c, fl)
        got = S.statement(c, inp)
        for b in range(c["B"]):
            n, n_out = c["lens"][b], c["lens_out"][b]
            if n_out == 0:
                assert got[b].shape == (0, c["Cout"])
                continue
            v = _torch_conv(S.prologue(inp["x"][b, :n], c, inp, b), inp["w"], c["dil"], c["pad"], n_out)
            if inp["bias"] is not None:
                v = v + inp["bias"].double()
            v = S.post_act(v, c)
            if inp["colscale"] is not None:
                v = v * inp["colscale"].double()
            if inp["res"] is not None:
                v = v + inp["res"][b, torch.arange(n_out) >> c["res_shift"]].double()
            if inp["old"] is not None:
                v = v + inp["old"][b, :n_out].double()
            v = v * c["out_scale"]
            if c["exact"]:
                assert torch.equal(got[b], v), (S.case_id(c), fl, b)
            else:
                assert float((got[b] - v).abs().max()) <= 1e-12 * max(1.0, float(v.abs().max())), (S.case_id(c), b)


def test_polyphase_statement_is_conv_transpose1d():
    """The polyphase repack the conv_transpose launches use (ops._polyphase_weight restated): conv_rows on the repacked taps, scattered to rows
    u * s + r - p, equals F.conv_transpose1d in float64 on integers."""
    g = torch.Generator().manual_seed(5)
    cin, cout, k, s, L = 32, 8, 8, 4, 37
    p, kp = (k - s) // 2, k // s
    w_t = torch.randint(-4, 5, (cout, k, cin), generator=g).double()
    x = torch.randint(-4, 5, (L, cin), generator=g).double()
    w = torch.empty((s * cout, kp, cin), dtype=torch.float64)
    for r in range(s):
        for tp in range(kp):
            w[r * cout:(r + 1) * cout, tp] = w_t[:, r + (kp - 1 - tp) * s]
    rows = S.conv_rows(x, w, 1, kp - 1, L + kp - 1)
    lout = (L - 1) * s - 2 * p + k
    got = torch.zeros((lout, cout), dtype=torch.float64)
    for u in range(L + kp - 1):
        for r in range(s):
            n = u * s + r - p
            if 0 <= n < lout:
                got[n] = rows[u, r * cout:(r + 1) * cout]
    want = F.conv_transpose1d(x.t()[None], w_t.permute(2, 0, 1), None, stride=s, padding=p)[0].t()
    assert torch.equal(got, want)


# ----------------------------------------------------------------------------------------------------------------- exactness preconditions
@pytest.mark.parametrize("c", EXACT, ids=S.case_id)
def test_exact_case_preconditions(c):
    for prec in c["precs"]:
        fl = S.flavour(prec)
        inp = S.inputs(c, fl)
        s, q = S.budget(c, fl)
        assert s / q < 2 ** 24, (S.case_id(c), prec, s, q)
        w = inp["w"]
        assert torch.equal(w.float().to(torch.bfloat16).double(), w) and torch.equal(w.float().to(torch.float16).double(), w)
        want = S.statement(c, inp)
        for b in range(c["B"]):
            t = S.prologue(inp["x"][b, :c["lens"][b]], c, inp, b)
            assert torch.equal(t, torch.round(t * 4) / 4) and torch.equal(t.float().double(), t)
            hi = S.hi_image(t, prec)
            lo = t - hi
            if prec in (1, 3):
                assert torch.equal(hi, t), (S.case_id(c), prec)                     # one pass holds the value
            elif prec in (2, 4):
                assert torch.equal(S.hi_image(lo, prec), lo), (S.case_id(c), prec)  # hi + lo holds it ...
                assert not c["lens"][b] or c["fq"] or bool((lo != 0).any()), (S.case_id(c), prec, b)    # ... and the lo image is needed
            assert torch.equal(want[b].float().double(), want[b])
        if prec in (5, 6):      # mx_ref's own arithmetic is exact on the case: weights on the grid with the expected scales, residuals on their blocks' grids
            wn = w.numpy().astype(np.float32)
            assert np.array_equal((mx_ref.quantise_weights if prec == 5 else mx_ref.quantise_weights4)(wn), wn.astype(np.float64))
            got = S.mx_statement(c, inp, prec)
            for b in range(c["B"]):
                assert torch.equal(got[b], want[b]), (S.case_id(c), prec, b)
                assert not c["lens"][b] or bool((S.prologue(inp["x"][b, :c["lens"][b]], c, inp, b).abs() >= 8192).any())


def test_fq_snake_palette_is_far_from_every_rounding_step():
    v = S.SNAKE_PALETTE
    s = v + (1.0 / 0.75) * torch.sin(0.75 * v) ** 2
    s32 = v.float() + (1.0 / torch.tensor(0.75)) * torch.sin(torch.tensor(0.75) * v.float()) ** 2
    assert len(v) >= 16 and float((s - torch.floor(s) - 0.5).abs().min()) >= 0.05 and float((s32.double() - s).abs().max()) < 1e-4
    # excluded share of the quantising cases: none


# ----------------------------------------------------------------------------------------------------------------- mutants
def _mutant_results(c, prec, m):
    inp = S.inputs(c, S.case_flavour(c, prec))
    if prec in (5, 6):
        return S.mx_statement(c, inp, prec, mutant=m)
    return S.statement(c, inp, prec=prec, mutant=m)


def _differs(a, b):
    return any(not torch.equal(torch.nan_to_num(x, nan=1e30), torch.nan_to_num(y, nan=1e30)) for x, y in zip(a, b))


@pytest.mark.parametrize("c", EXACT, ids=S.case_id)
def test_every_claimed_mutant_changes_the_exact_result(c):
    for prec in c["precs"]:
        want = S.expected(c, prec)
        for m in c["covers"]:
            if m in ("lo_drop", "cross_drop") and prec in (1, 3):
                continue            # single-image formats have no lo image
            if m in ("mx_scale", "mx_tap_swap") and prec not in (5, 6):
                continue
            assert _differs(_mutant_results(c, prec, m), want), (S.case_id(c), prec, m)


def test_no_mutant_passes_all_exact_cases():
    alive = set(S.MUTANTS)
    for c in EXACT:
        for m in c["covers"]:
            alive.discard(m)
    assert not alive, alive
    covered = {m: [S.case_id(c) for c in EXACT if m in c["covers"]] for m in S.MUTANTS}
    assert all(len(v) >= 2 for v in covered.values()), covered


@pytest.mark.parametrize("c", FLOAT, ids=S.case_id)
def test_float_cases_bound_margin_and_mutants(c):
    """The float32 evaluation of the statement stays within half a bound; every claimed mutant misses by more than ten bounds."""
    for prec in c["precs"]:
        inp = S.inputs(c, S.case_flavour(c, prec))
        bound, e32, peak = S.float_bound(c, prec)
        want = S.expected(c, prec)
        w32 = S.statement(c, inp, dt=torch.float32)
        ref = S.statement(c, inp)
        for b in range(c["B"]):
            if want[b].numel():
                assert bool(((w32[b].double() - ref[b]).abs() <= 0.5 * bound[b]).all()), (S.case_id(c), prec)
        for m in c["covers"]:
            mut = _mutant_results(c, prec, m)
            worst = max(float(((mut[b] - want[b]).abs() / bound[b]).max()) for b in range(c["B"]) if want[b].numel())
            assert worst > 10.0, (S.case_id(c), prec, m, worst)
        # the mutants of the lo pass: beyond ten bounds as well (precisions 5 / 6: under the bound that carries the MX image's rounding steps)
        for m in {2: ("lo_drop",), 4: ("lo_drop",), 5: ("lo_drop", "mx_scale", "mx_tap_swap"), 6: ("lo_drop", "mx_scale", "mx_tap_swap")}.get(prec, ()):
            mut = _mutant_results(c, prec, m)
            worst = max(float(((mut[b] - want[b]).abs() / bound[b]).max()) for b in range(c["B"]) if want[b].numel())
            print(f"CONV mutant {S.case_id(c)} p{prec} {m}: {worst:.1f} bounds")
            assert worst > 10.0, (S.case_id(c), prec, m, worst)


# ----------------------------------------------------------------------------------------------------------------- routes
def _parse_ws4_lists():
    """The WS4_CASE / WS4_GEMM / WS4_*_N64 / WS4_FQ lines of the six .hip files -> the labels route() must be able to emit."""
    labels = []
    for fn in ("conv_ws4.hip", "conv_ws4_p4.hip", "conv_ws4_p13.hip", "conv_ws4_p5.hip", "conv_ws4_p6.hip", "conv_ws4_fq.hip"):
        text = open(os.path.join(CSRC, fn)).read()
        for m in re.finditer(r"^\s*WS4_(CASE|GEMM|CASE_N64|GEMM_N64|FQ)\(([^)]*)\);", text, re.M):
            kind, a = m.group(1), [s.strip() for s in m.group(2).split(",")]
            if kind == "FQ":
                labels.append(S.ws4_label(2, "conv", a[0][2:], 0, int(a[1]), fq=True))
            elif kind.startswith("CASE"):
                labels.append(S.ws4_label(int(a[0]), "conv", a[1][2:], int(a[2]), 64 if kind.endswith("N64") else 128))
            else:
                labels.append(S.ws4_label(int(a[0]), "gemm", "NONE", int(a[1]), 64 if kind.endswith("N64") else 128))
        for m in re.finditer(r"return route_ws4<5, P_SNAKE, 0, false, false, 0, 128, false, false>", text):
            labels.append(S.ws4_label(5, "conv", "SNAKE", 0, 128, two_by_two=True))
    return labels


def _parse_4wave():
    """The one list of 4-wave / split-K instantiations (launcher_of<PREC>, conv_gemm.hip) times the precisions of its dispatch."""
    text = open(os.path.join(CSRC, "conv_gemm.hip")).read()
    body = text[text.index("conv_launch_fn launcher_of(const conv_route& r) {\n  const int tile"):text.index("// The tile code, decoded once.")]
    precs = re.findall(r"return launcher_of<(\d)>\(r\);", body)
    no_novec = re.findall(r"if constexpr \(PREC != (\d)\) return launch<64, 64, PREC, false>;", body)
    assert len(precs) == 4 and len(no_novec) == 1
    out = []
    for bm, bn, v in re.findall(r"return launch<(\d+), (\d+), PREC, (true|false)>;", body):
        out += [f"4wave/p{p}/{bm}x{bn}/{'vec' if v == 'true' else 'novec'}" for p in precs if v == "true" or p not in no_novec]
    for bm, bn in re.findall(r"launch_split<(\d+), (\d+), PREC>", body):
        out += [f"splitk/p{p}/{bm}x{bn}" for p in precs]
    return out


def gpu_labels():
    """Every label of every call tests/test_conv_kernel_edges_gpu.py makes on the tile codes of the case tables."""
    seen = {}
    for c in S.all_cases():
        for prec in c["precs"]:
            for tile, lab, facts in S.tile_calls(c, prec):
                seen.setdefault(lab, []).append((S.case_id(c), prec, tile))
    return seen


def test_restated_lists_are_the_sources():
    assert sorted(_parse_ws4_lists()) == sorted(S.all_ws4_labels())
    assert sorted(_parse_4wave()) == sorted(S.all_4wave_labels())
    assert len(S.all_ws4_labels()) == 62


def test_every_instantiation_is_reached():
    seen = gpu_labels()
    strip = lambda l: l.replace("mx->p4 fallback ", "")
    base = {strip(l) for l in seen} | {strip(l).rsplit("/", 1)[0] for l in seen if strip(l).startswith("splitk/")}
    unreached = [l for l in _parse_ws4_lists() + _parse_4wave() if l not in base]
    assert unreached == [], unreached
    # both finish kernels of split-K, the MX fallback on 4-wave and on split-K, and an exact case on every label
    assert any(l.endswith("/lean") for l in seen) and any(l.endswith("/general") for l in seen)
    assert any(l.startswith("mx->p4 fallback 4wave") for l in seen) and any(l.startswith("mx->p4 fallback splitk") for l in seen)


def _window_limit_launches():
    win196 = next(c for c in EXACT if c["name"] == "k5 d17 window 196")
    d = {("win196", prec, tile): S.case_launch(win196, prec, tile) for prec in (1, 2, 3, 4) for tile in (S.WS, S.WS64)}
    d["tile 0 window 196"] = S.launch(B=130, L=5, Cin=64, Cout=128, K=5, dil=17, pad=34, split_ws=False)
    d["elu p1"] = S.launch(B=130, L=5, Cin=64, Cout=128, K=3, pad=1, pre="ELU", precision=1, split_ws=False)
    d["ws4 p2"] = S.launch(B=130, L=5, Cin=64, Cout=128, K=3, pad=1, precision=2)
    d["ws4 p3 thin"] = S.launch(B=130, L=5, Cin=64, Cout=64, K=3, pad=1, precision=3)
    d["mx ws64"] = S.launch(Cin=64, Cout=128, K=3, precision=5, tile=S.WS64, L=200)
    d["splitk no workspace"] = S.launch(Cin=64, Cout=128, K=3, tile=2064128, L=200, split_ws=False)
    return d


def test_window_limit_and_fallthrough_routes():
    d = _window_limit_launches()
    for prec in (1, 2, 3, 4):
        assert S.route(d["win196", prec, S.WS])[0].startswith("refuse:the wave-specialised tile")
        assert S.route(d["win196", prec, S.WS64])[0].startswith("refuse:the wave-specialised tile")
    # tile 0 with >= 128 tiles and a window past the limit: a 4-wave launch
    assert S.route(d["tile 0 window 196"])[0] == "4wave/p2/64x128/vec"
    # the ws4 MI355_ERR_UNSUPPORTED fall-through: an ELU prologue at precision 1 has no instantiation -> the 4-wave kernel tile 0 names
    a = d["elu p1"]
    assert S.ws4_eligible(a, 1) and S.ws4_launch(a, 1, 0, 128) is None and S.route(a)[0] == "4wave/p1/64x128/vec"
    assert S.route(d["ws4 p2"])[0] == "ws4/p2/conv/NONE/epi0/bn128"
    assert S.route(d["ws4 p3 thin"])[0] == "ws4/p3/conv/NONE/epi0/bn64"
    assert S.route(d["mx ws64"])[0].startswith("refuse:MX images")
    assert S.route(d["splitk no workspace"])[0].startswith("refuse:the split-K tiles")


def _suite_launches():
    """Every launch of the GPU suite's case tables as route() sees it -- each case at each of its precisions on each tile code in_suite admits, the whole
    batch and each item alone -- plus the launches of test_window_limit_and_fallthrough_routes and of the GPU suite's test_polyphase_store_exact."""
    for c in S.all_cases():
        for prec in c["precs"]:
            for tile in (c["tiles"] or S.EVERY):
                if S.in_suite(prec, tile):
                    for only in [None] + list(range(c["B"])):
                        yield (S.case_id(c), prec, tile, only), S.case_launch(c, prec, tile, only=only)
    for key, a in _window_limit_launches().items():
        yield key, a
    for a in S.polyphase_launches():
        yield ("polyphase", a["precision"], a["tile"]), a


def test_route_is_the_librarys_routing_function_launch_by_launch(capsys):
    """route() of tests/_conv_cases.py against ``mi355_conv_gemm_route`` on every launch of ``_suite_launches``: where route() names a kernel the library
    returns 0 and its record formats to exactly that label, with the split-K group count and the ws4 geometry of route()'s facts; where route() refuses,
    the library refuses and leaves the record alone.  The environment knobs must be unset (route() restates the defaults)."""
    import ctypes

    from mlx_audio_amd import _lib, ops

    assert [k for k in S.ENV_KNOBS if k in os.environ] == []
    lib = _lib.load()
    fields = [f for f, _ in _lib._STRUCT_DECLS["mi355_conv_route"]]
    n = refused = 0
    for key, a in _suite_launches():
        label, facts = S.route(a)
        args = _lib.STRUCTS["mi355_conv_gemm_args"](**{k: v for k, v in S.route_args(a, ops).items() if v is not None})
        out = _lib.STRUCTS["mi355_conv_route"](**{f: -1 for f in fields})
        rc = lib.mi355_conv_gemm_route(ctypes.byref(args), ctypes.byref(out))
        rec = {f: getattr(out, f) for f in fields}
        n += 1
        if label.startswith("refuse:"):
            refused += 1
            assert rc != 0 and lib.mi355_last_error() and all(v == -1 for v in rec.values()), (key, label, rc, rec)
            continue
        assert rc == 0, (key, label, rc, lib.mi355_last_error())
        assert S.record_label(rec) == label, (key, label, rec)
        if label.startswith("splitk/") or label.startswith("mx->p4 fallback splitk/"):
            assert rec["groups"] == facts["groups"], (key, label, rec, facts)
        elif label.startswith("ws4/"):
            assert {f: rec[f] for f in S.ROUTE_GEOMETRY} == {f: facts[f] for f in S.ROUTE_GEOMETRY}, (key, label, rec, facts)
        else:
            assert facts is None
    with capsys.disabled():
        print(f"\nCONV route: {n} launches compared with mi355_conv_gemm_route ({refused} of them refusals), 0 left out")
    assert n > 40000


@pytest.mark.parametrize("c", S.all_cases(), ids=S.case_id)
def test_branch_facts_are_as_claimed(c):
    for prec in c["precs"]:
        ws = [(t, l, f) for t, l, f in S.tile_calls(c, prec) if l.startswith("ws4/")]
        for key, val in c["claims"].items():
            assert ws, (S.case_id(c), prec)
            for tile, lab, f in ws:
                if key in ("interior", "masked"):
                    fast = "/gemm/" in lab or "/NONE/" in lab or "/LEAKY/" in lab or prec in (5, 6)
                    if key == "interior" and (tile // 10000000) & 2 and prec not in (5, 6):
                        assert not f["interior"]            # feature digit 2: masked body only
                    elif key == "masked" or (fast and "/fq/" not in lab):
                        assert f[key] == val, (S.case_id(c), prec, tile, key, f)
                elif key == "odd_nch":
                    assert f[key] == val or "/conv/" in lab, (S.case_id(c), prec, tile)
                else:
                    assert f[key] == val, (S.case_id(c), prec, tile, key, f)


def test_walk_cases_walk_and_skip():
    """Under 8 / 16 resident workgroups every walk case has a workgroup with >= 2 live tiles, and (ragged ones) an id skipped between two live tiles."""
    for c in S.walk_cases():
        for prec in c["precs"]:
            for tile in c["tiles"]:
                for resident in (8, 16):
                    lab, f = S.route(S.case_launch(c, prec, tile, resident=resident))
                    if not lab.startswith("ws4/"):
                        continue
                    assert 9 <= f["total_ids"] <= 40 or f["live_tiles"] >= 9, (S.case_id(c), f)
                    if not f["walk"]:
                        assert resident == 16 and f["total_ids"] <= 16
                        continue
                    walks = [S.workgroup_tiles(wg, f["grid"], f["total_ids"], f["P"], f["NT"], f["glog"], f["tiles_per_item"], c["lens_out"]) for wg in range(f["grid"])]
                    assert sum(len(w) for w in walks) == f["live_tiles"] and max(len(w) for w in walks) >= 2
                    if c["ragged"]:
                        assert any(b[0] - a[0] > f["grid"] for w in walks for a, b in zip(w, w[1:])) or any(w and w[0][0] >= f["grid"] for w in walks), S.case_id(c)


# ----------------------------------------------------------------------------------------------------------------- scheduler
def _visits_once(P, NT, mutant=None):
    p, ny = S.ids_to_p(P, NT, mutant)
    live = p >= 0
    if (p[live] >= P).any():
        return False
    key = p[live] * NT + ny[live]
    return len(key) == P * NT and len(np.unique(key)) == P * NT


def test_scheduler_visits_every_tile_once():
    """decode_tile over all virtual ids of a launch is a bijection onto (row tile, column tile) for P = 1 .. 2100, NT = 1 .. 4.  A persistent launch hands
    id i to workgroup i mod grid whatever the grid size is, so this part does not depend on the grid; the literal walk below does."""
    for P in range(1, 2101):
        for NT in (1, 2, 3, 4):
            assert _visits_once(P, NT), (P, NT)


@pytest.mark.parametrize("P", [1, 7, 9] + list(S.GLOG_P) + [2100])
def test_scheduler_literal_walk(P):
    """The literal next_work walk of every workgroup, for EVERY grid size 8 .. 512 in steps of 8 (as ws4_grid clamps it to the id count) and NT 1 .. 4,
    at every glog boundary of P: each live tile exactly once over all workgroups, a workgroup's ids all on its own XCD, ragged items whose dead tiles
    (and one empty item) are skipped."""
    tpi = 3 if P % 3 == 0 else 1
    B = P // tpi
    lens = [tpi * 128 - (37 * b) % 128 for b in range(B)]       # every item reaches its last tile (partly filled) ...
    if tpi == 3:
        lens[B // 2], lens[-1] = 0, 130                          # ... but an empty item and one that ends a tile early: ids next_work must skip
    live = sum((n + 127) // 128 for n in lens)
    glog = 3 if P >= 512 else (2 if P >= 256 else (1 if P >= 128 else 0))
    for NT in (1, 2, 3, 4):
        total = len(S.ids_to_p(P, NT)[0])
        table = [S.decode_tile(i, P, NT, glog, tpi, lens) for i in range(total)]
        for grid in (range(8, 513, 8) if P <= 520 else (8, 16, 24, 256, 504, 512)):
            g = min(grid, total)
            seen = set()
            for wg in range(g):
                for i, tile in S.workgroup_tiles(wg, g, total, P, NT, glog, tpi, lens, table=table):
                    assert i & 7 == wg & 7 and tile not in seen
                    seen.add(tile)
            assert len(seen) == live * NT, (P, NT, grid)


def test_scheduler_mutants_fail():
    for m in ("glog", "nocut"):
        bad = [(P, NT) for P in (1, 7, 9, 127, 128, 129, 255, 256, 300, 511, 512, 520, 2100) for NT in (1, 2) if not _visits_once(P, NT, m)]
        assert bad, m
    assert not _visits_once(9, 1, "nocut") and not _visits_once(7, 1, "glog") and not _visits_once(20, 2, "glog")
