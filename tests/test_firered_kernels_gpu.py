"""``csrc/firered.hip`` against the float64 statements of ``_ops_emu_fireredasr2.py`` on the same float32 inputs: ``subsample2d_k3s2``,
``glu_dwconv_ln_swish``, ``beam_step`` and ``beam_attention``.  The bars are the per-element float32 rounding bounds derived there (not tuned); every
test prints its largest error / bound ratio (docs/COVERAGE.md records them).  Decisions (beam indices, tokens, histories, flags) are compared exactly,
on inputs whose decision margins the float64 statement itself asserts.  Common to all four: outputs start as NaN (or a sentinel), padded rows are
exactly zero, an item of a ragged batch is bit-equal to that item alone, a repeat is bit-equal, and a refused call leaves its outputs untouched."""
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import _ops_emu_fireredasr2 as E  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops():
    from mlx_audio_amd import ops

    ops.require_gpu()
    return ops


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def _ratio(got, val, bound):
    assert not np.isnan(got).any()
    return float((np.abs(got - val) / (bound + 1e-300)).max()) if got.size else 0.0


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


# ------------------------------------------------------------------ subsample2d_k3s2
def _sub_chain(ops, x, w1, b1, w2, b2, lens_in, lens1, lens2):
    """conv1 (one input channel -> C, channels-last) then conv2 (C -> C, written as [B, To, C, Fo])."""
    B, T, F = x.shape
    C = w1.shape[0]
    T1, F1 = E.sub_out(T), E.sub_out(F)
    y1 = ops.subsample2d_k3s2(x, w1, b1, _nan(B, T1, F1, C), lens_in=lens_in, lens_out=lens1)
    y2 = None
    if T1 >= 3 and F1 >= 3:
        y2 = ops.subsample2d_k3s2(y1, w2, b2, _nan(B, E.sub_out(T1), C, E.sub_out(F1)), out_cf=True, lens_in=lens1, lens_out=lens2)
    return y1, y2


@pytest.mark.parametrize("F,C", [(7, 8), (80, 32)])
@pytest.mark.parametrize("T", [7, 8, 10, 11, 107])
def test_subsample2d(ops, T, F, C):
    """Both convs of the subsampler at B = 3 with ragged ``lens_in`` (the full length, the six-zero-frames case ``lens_in = T - 6`` with the output
    length of T, and the shortest item that still gives a row): within the bound, padded rows zero, items bit-equal alone, a repeat bit-equal."""
    g = torch.Generator().manual_seed(1000 * T + F)
    x = torch.randn(3, T, F, generator=g)
    w1, b1 = 0.4 * torch.randn(C, 3, 3, 1, generator=g), 0.2 * torch.randn(C, generator=g)
    w2, b2 = 0.1 * torch.randn(C, 3, 3, C, generator=g), 0.2 * torch.randn(C, generator=g)
    lin = [T, max(T - 6, 1), min(T, 7)]
    l1 = [E.sub_out(T), E.sub_out(T), E.sub_out(lin[2])]          # item 1: its frames plus six zero frames of right context
    l2 = [E.sub_out(v) if v >= 3 else 0 for v in l1]
    d = lambda t: t.to(DEV)
    y1, y2 = _sub_chain(ops, d(x), d(w1), d(b1), d(w2), d(b2), _i32(lin), _i32(l1), _i32(l2))
    z1, z2 = _sub_chain(ops, d(x), d(w1), d(b1), d(w2), d(b2), _i32(lin), _i32(l1), _i32(l2))
    assert torch.equal(y1, z1) and (y2 is None or torch.equal(y2, z2))
    v1, bd1 = E.subsample2d(x.numpy(), w1.numpy(), b1.numpy(), lin, l1)
    worst = _ratio(y1.cpu().double().numpy(), v1, bd1)
    for b in range(3):
        assert not y1[b, l1[b]:].any()
    if y2 is not None:
        v2, bd2 = E.subsample2d(y1.cpu().numpy(), w2.numpy(), b2.numpy(), l1, l2, out_cf=True)
        worst = max(worst, _ratio(y2.cpu().double().numpy(), v2, bd2))
        for b in range(3):
            assert not y2[b, l2[b]:].any()
    # items alone: item 0 as it is, item 2 cut to its own frames
    for b, Tb in ((0, T), (2, lin[2])):
        a1, a2 = _sub_chain(ops, d(x[b:b + 1, :Tb]), d(w1), d(b1), d(w2), d(b2), None, None, None)
        assert torch.equal(a1[0], y1[b, :l1[b]])
        if a2 is not None:
            assert torch.equal(a2[0], y2[b, :l2[b]])
    print(f"subsample2d T={T} F={F} C={C}: worst error / bound = {worst:.3f}")
    assert worst <= 1.0


def test_subsample2d_refusals(ops):
    from mlx_audio_amd import _lib

    x, y = torch.zeros(1, 9, 9, device=DEV), _nan(1, 4, 4, 8)
    for w, xx, yy in ((torch.zeros(6, 3, 3, 1, device=DEV), x, _nan(1, 4, 4, 6)),                       # Cout % 4
                      (torch.zeros(68, 3, 3, 1, device=DEV), x, _nan(1, 4, 4, 68)),                     # Cout > 64
                      (torch.zeros(8, 3, 3, 4, device=DEV), torch.zeros(1, 9, 9, 4, device=DEV), y)):   # Cin is neither 1 nor Cout
        with pytest.raises(_lib.Mi355Error, match="subsample2d_k3s2"):
            ops.subsample2d_k3s2(xx, w, None, yy)
        assert torch.isnan(yy).all()


# ------------------------------------------------------------------ glu_dwconv_ln_swish
def _glu_inputs(B, L, C, K, seed, pad=0):
    """Rows with a floor on the standard deviation of z: every channel's value carries an independent unit-variance part, and the taps' centre is
    at least 0.5, so var_c z stays of order 0.1 and the LayerNorm bound is finite."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, L, 2 * C + pad, generator=g)
    x[..., :C] += 0.5 * torch.randn(B, L, 1, generator=g)
    w = torch.randn(C, K, generator=g) / math.sqrt(K)
    w[:, (K - 1) // 2] = 0.5 + w[:, (K - 1) // 2].abs()
    return x, w, 1.0 + 0.2 * torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g)


@pytest.mark.parametrize("K", [1, 15, 33])
@pytest.mark.parametrize("C", [128, 256, 2560])
def test_glu_dwconv_ln_swish(ops, C, K):
    """L = 1, 2, 16, 17 and the row tile - 1, the row tile, the row tile + 1 at both tile heights (32 and, in launches as small as these, 16; plus 70), B = 3 ragged (the full length, about half,
    one row: items shorter than the halo), a padded row stride: within the bound, padded rows zero, items bit-equal alone, a repeat bit-equal."""
    R = ops.GLU_DWCONV_LN_ROWS
    worst = 0.0
    for L in (1, 2, R // 2 - 1, 16, 17, R - 1, R, R + 1, 70):
        x, w, lw, lb = _glu_inputs(3, L, C, K, seed=C + 97 * K + L, pad=8 if L % 2 else 0)
        lens = [L, max(1, L // 2), 1]
        xd = x.to(DEV)[..., :2 * C]
        args = (w.to(DEV), lw.to(DEV), lb.to(DEV))
        y = ops.glu_dwconv_ln_swish(xd, *args, _nan(3, L, C), eps=1e-5, lens=_i32(lens))
        y2 = ops.glu_dwconv_ln_swish(xd, *args, _nan(3, L, C + 4)[..., :C], eps=1e-5, lens=_i32(lens))
        assert torch.equal(y, y2)
        val, bound = E.glu_dwconv_ln_swish(x[..., :2 * C].numpy(), w.numpy(), lw.numpy(), lb.numpy(), 1e-5, lens)
        worst = max(worst, _ratio(y.cpu().double().numpy(), val, bound))
        for b, n in enumerate(lens):
            assert not y[b, n:].any()
            alone = ops.glu_dwconv_ln_swish(xd[b:b + 1, :n].contiguous(), *args, _nan(1, n, C), eps=1e-5)
            assert torch.equal(alone[0], y[b, :n])
    print(f"glu_dwconv_ln_swish C={C} K={K}: worst error / bound = {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("C", [260, 512, 516, 1024, 1028, 1536, 2048, 2052])
def test_glu_dwconv_ln_swish_geometries(ops, C):
    """The widths at which the launch changes its geometry (256 threads x 1 / 2 / 4 channels up to 1024 channels, 512 threads x 3 / 4 / 5 above),
    each just at and just above a boundary, so that the last channel group is full or nearly empty; both tap windows (K 15 and 33), L = the row
    tile + 1, B = 2 ragged."""
    worst, L = 0.0, ops.GLU_DWCONV_LN_ROWS + 1
    for K in (15, 33):
        x, w, lw, lb = _glu_inputs(2, L, C, K, seed=3 * C + K)
        lens = [L, 7]
        args = (w.to(DEV), lw.to(DEV), lb.to(DEV))
        y = ops.glu_dwconv_ln_swish(x.to(DEV), *args, _nan(2, L, C), eps=1e-5, lens=_i32(lens))
        val, bound = E.glu_dwconv_ln_swish(x.numpy(), w.numpy(), lw.numpy(), lb.numpy(), 1e-5, lens)
        worst = max(worst, _ratio(y.cpu().double().numpy(), val, bound))
        assert not y[1, 7:].any()
        alone = ops.glu_dwconv_ln_swish(x.to(DEV)[1:, :7].contiguous(), *args, _nan(1, 7, C), eps=1e-5)
        assert torch.equal(alone[0], y[1, :7])
    print(f"glu_dwconv_ln_swish geometry C={C}: worst error / bound = {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("C,B,L", [(128, 64, 130), (512, 64, 130), (1024, 64, 130), (1536, 86, 96), (2048, 86, 96), (2560, 86, 96)])
def test_glu_dwconv_ln_swish_full_tile(ops, C, B, L):
    """Launches of at least 256 full-height row tiles run the full tile (the cases above, being small, all run the half-height one): within the bound
    on the first two items, and every checked item bit-equal to that item alone, which runs the half-height tile -- the bits do not depend on it."""
    assert -(-L // ops.GLU_DWCONV_LN_ROWS) * B >= 256
    K = 33
    g = torch.Generator(device=DEV).manual_seed(C + B)
    x = torch.randn(B, L, 2 * C, generator=g, device=DEV)
    x[..., :C] += 0.5 * torch.randn(B, L, 1, generator=g, device=DEV)
    _, w, lw, lb = _glu_inputs(1, 1, C, K, seed=C)
    lens = [L, L - 37] + [L - (b % 5) for b in range(2, B)]
    args = (w.to(DEV), lw.to(DEV), lb.to(DEV))
    y = ops.glu_dwconv_ln_swish(x, *args, _nan(B, L, C), eps=1e-5, lens=_i32(lens))
    assert torch.equal(y, ops.glu_dwconv_ln_swish(x, *args, _nan(B, L, C), eps=1e-5, lens=_i32(lens)))
    val, bound = E.glu_dwconv_ln_swish(x[:2].cpu().numpy(), w.numpy(), lw.numpy(), lb.numpy(), 1e-5, lens[:2])
    worst = _ratio(y[:2].cpu().double().numpy(), val, bound)
    for b in (0, 1, B - 1):
        n = lens[b]
        assert not y[b, n:].any()
        alone = ops.glu_dwconv_ln_swish(x[b:b + 1, :n].contiguous(), *args, _nan(1, n, C), eps=1e-5)
        assert torch.equal(alone[0], y[b, :n])
    print(f"glu_dwconv_ln_swish full tile C={C} B={B} L={L}: worst error / bound = {worst:.3f}")
    assert worst <= 1.0


def test_glu_dwconv_ln_swish_refusals(ops):
    from mlx_audio_amd import _lib

    def call(C, K, alias=False):
        x = torch.zeros(1, 4, 2 * C, device=DEV)
        y = x[..., :C] if alias else _nan(1, 4, C)
        with pytest.raises(_lib.Mi355Error, match="glu_dwconv_ln_swish"):
            ops.glu_dwconv_ln_swish(x, torch.zeros(C, K, device=DEV), torch.ones(C, device=DEV), torch.zeros(C, device=DEV), y)
        assert alias or torch.isnan(y).all()

    call(128, 35)        # more taps than MI355_GLU_DWCONV_LN_MAX_TAPS
    call(128, 4)         # even
    call(2564, 3)        # wider than MI355_GLU_DWCONV_LN_MAX_C
    call(130, 3)         # not a multiple of 4
    call(128, 3, alias=True)


# ------------------------------------------------------------------ beam_step
def _spaced_logits(rows, V, g, spacing=0.37, top=None):
    """Every row a permutation of V values `spacing` apart (so every candidate is decided by a wide margin: the spacing shrinks with V to keep the
    row's range, which the rounding bound grows with, near 30), shifted so the row maximum is `top`."""
    x = torch.stack([torch.randperm(V, generator=g).float() for _ in range(rows)]) * min(spacing, 30.0 / V)
    return x - x.max(-1, keepdim=True).values + (3.0 if top is None else top)


def _state(ops, N, B, Tmax, steps, max_steps, scores, finished, done, g, eos_id):
    st = ops.beam_state(N, B, Tmax, max_steps, sos_id=1, device=DEV)
    st.scores.copy_(torch.tensor(scores, dtype=torch.float32).view(N, B))
    st.finished.copy_(torch.tensor(finished, dtype=torch.int32).view(N, B))
    st.step.copy_(torch.tensor(steps, dtype=torch.int32))
    st.done.copy_(torch.tensor(done, dtype=torch.int32))
    st.tokens[0].copy_(torch.randint(0, 50, (N, B, Tmax), generator=g, dtype=torch.int32))
    st.ind[0].copy_(torch.randint(0, B, (N, B, Tmax), generator=g, dtype=torch.int32))
    st.conf[0].copy_(torch.rand(N, B, Tmax, generator=g))
    st.tokens[1].fill_(-7)
    st.ind[1].fill_(-7)
    st.conf[1].fill_(float("nan"))
    st.beam_idx.fill_(-7)
    st.new_tokens.fill_(-7)
    st.new_conf.fill_(float("nan"))
    return st


def _run_step(ops, logits, st, eos_id, smoothing, pen, min_margin=4.0):
    """One kernel step against the statement: decisions and histories exact, values within the bound; returns (worst ratio, state after)."""
    n_ = lambda t: t.cpu().numpy().copy()
    before = dict(scores=n_(st.scores), finished=n_(st.finished), step=n_(st.step), max_steps=n_(st.max_steps), done=n_(st.done),
                  tokens=n_(st.tokens[st.cur]), ind=n_(st.ind[st.cur]), conf=n_(st.conf[st.cur]))
    want = E.beam_step(logits.cpu().numpy(), eos_id=eos_id, smoothing=smoothing, eos_penalty=pen, **before)
    assert (want["margin"] >= min_margin).all(), f"the test's own inputs leave a decision within {min_margin} bounds: {want['margin']}"
    ops.beam_step(logits, st, eos_id=eos_id, softmax_smoothing=smoothing, eos_penalty=pen)
    cur = st.cur
    for name, got in (("finished", st.finished), ("step", st.step), ("done", st.done), ("beam_idx", st.beam_idx), ("new_tokens", st.new_tokens),
                      ("tokens", st.tokens[cur]), ("ind", st.ind[cur])):
        assert np.array_equal(n_(got), want[name]), (name, n_(got), want[name])
    worst = 0.0
    for name, got, bound in (("scores", st.scores, want["score_bound"]), ("new_conf", st.new_conf, want["conf_bound"])):
        got = n_(got).astype(np.float64)
        live = ~np.isnan(want[name])
        assert np.array_equal(np.isnan(got), ~live), name           # untouched entries are still NaN
        if name == "scores":
            frozen = before["done"] != 0
            assert np.array_equal(got[frozen], before["scores"][frozen].astype(np.float64))
            live = live & ~frozen[:, None]
        worst = max(worst, _ratio(got[live], want[name][live], bound[live]))
    gc, wc = n_(st.conf[cur]).astype(np.float64), want["conf"]
    assert np.array_equal(np.isnan(gc), np.isnan(wc))
    N, B = before["scores"].shape
    for n in range(N):
        if before["done"][n] or not (1 <= before["step"][n] < gc.shape[2]):
            continue
        s = int(before["step"][n])
        assert np.array_equal(gc[n, :, :s], wc[n, :, :s])              # moved, not recomputed
        assert np.array_equal(gc[n, :, s], n_(st.new_conf)[n].astype(np.float64))
    return worst


@pytest.mark.parametrize("V", ["B+1", 1000, 8667])
@pytest.mark.parametrize("B", [1, 2, 3, 5, 8])
def test_beam_step(ops, B, V):
    """N = 4 and N = 1, eos at 0 and at V - 1, eos_penalty 1.0 and 1.5: the first step (scores [0, -1e10, ...]), one beam finished, B - 1 beams
    finished, a frozen item (untouched), then every item alone (bit-equal to the batch) and a repeat (bit-equal)."""
    V = B + 1 if V == "B+1" else V
    Tmax, worst = 12, 0.0
    for eos_id in (0, V - 1):
        for pen in (1.0, 1.5):
            g = torch.Generator().manual_seed(B * 100003 + V + eos_id + int(pen * 10))
            logits = _spaced_logits(4 * B, V, g).to(DEV)
            live = (-torch.rand(B, generator=g).sort().values * 5).tolist()
            fin1 = [0] * B
            fin1[B // 2] = 1
            scores = [0.0] + [-1e10] * (B - 1) + live + live + live
            finished = [0] * B + fin1 + [0] + [1] * (B - 1) + [0] * B
            steps, done, ms = [1, 5, 10, 4], [0, 0, 0, 1], [Tmax, Tmax, Tmax, Tmax]
            mk = lambda gg: _state(ops, 4, B, Tmax, steps, ms, scores, finished, done, gg, eos_id)
            st = mk(torch.Generator().manual_seed(5))
            worst = max(worst, _run_step(ops, logits, st, eos_id, 1.25, pen))
            assert st.done.tolist()[3] == 1 and st.step.tolist() == [2, 6, 11, 4]
            assert (st.tokens[1][3] == -7).all() and (st.ind[1][3] == -7).all() and torch.isnan(st.conf[1][3]).all()       # the frozen item
            assert (st.tokens[1][0, :, 2:] == -7).all() and (st.tokens[1][1, :, 6:] == -7).all()                           # nothing beyond `step`
            st2 = mk(torch.Generator().manual_seed(5))
            ops.beam_step(logits, st2, eos_id=eos_id, softmax_smoothing=1.25, eos_penalty=pen)
            for a, b in ((st.scores, st2.scores), (st.new_conf, st2.new_conf), (st.conf[1], st2.conf[1])):
                assert torch.equal(torch.nan_to_num(a, nan=-3.0), torch.nan_to_num(b, nan=-3.0))
            assert torch.equal(st.tokens[1], st2.tokens[1]) and torch.equal(st.ind[1], st2.ind[1])
            for n in range(3):   # each live item alone
                sa = ops.beam_state(1, B, Tmax, [Tmax], sos_id=1, device=DEV)
                full = mk(torch.Generator().manual_seed(5))
                for name in ("scores", "finished", "step", "done"):
                    getattr(sa, name).copy_(getattr(full, name)[n:n + 1])
                for name in ("tokens", "ind", "conf"):
                    getattr(sa, name)[0].copy_(getattr(full, name)[0][n:n + 1])
                ops.beam_step(logits[n * B:(n + 1) * B], sa, eos_id=eos_id, softmax_smoothing=1.25, eos_penalty=pen)
                assert torch.equal(sa.scores[0], st.scores[n]) and torch.equal(sa.new_conf[0], st.new_conf[n])
                assert torch.equal(sa.tokens[1][0, :, :steps[n] + 1], st.tokens[1][n, :, :steps[n] + 1]) and torch.equal(sa.beam_idx[0], st.beam_idx[n])
    print(f"beam_step B={B} V={V}: worst error / bound = {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("B", [1, 3, 8])
def test_beam_step_done_rules(ops, B):
    """All beams finished -> done; ``step + 1 == max_steps`` -> done; a step outside [1, Tmax) -> done and nothing else; and eos moving out of the
    top B under ``eos_penalty`` 1.5 (second-best logit: kept at 1.0, dropped or demoted at 1.5)."""
    V, Tmax = 40, 8
    g = torch.Generator().manual_seed(B)
    logits = _spaced_logits(3 * B, V, g).to(DEV)
    scores = (-torch.rand(3 * B, generator=g) * 3).tolist()
    st = _state(ops, 3, B, Tmax, [3, 6, 8], [Tmax, 7, Tmax], scores, [1] * B + [0] * (2 * B), [0, 0, 0], g, 2)
    _run_step(ops, logits, st, 2, 1.25, 1.0)
    assert st.done.tolist() == [1, 1, 1] and st.step.tolist() == [4, 7, 8]
    assert (st.new_tokens[0] == 2).all() and (st.tokens[1][2] == -7).all() and (st.beam_idx[2] == -7).all()
    assert st.new_conf[0].tolist() == [1.0] * B
    # eos as the second-largest logit of every row, close behind the best
    eos = 7
    x = _spaced_logits(B, V, g, spacing=0.5)
    srt = x.sort(-1, descending=True)
    for r in range(B):
        a, b = int(srt.indices[r, 1]), eos
        x[r, a], x[r, b] = x[r, b].clone(), x[r, a].clone()
    ranks = {}
    for pen in (1.0, 1.5):
        st = _state(ops, 1, B, Tmax, [2], [Tmax], [0.0] + [-50.0 * (i + 1) for i in range(B - 1)], [0] * B, [0], torch.Generator().manual_seed(1), eos)
        _run_step(ops, x.to(DEV), st, eos, 1.25, pen)
        ranks[pen] = st.new_tokens[0].tolist()
    if B > 1:
        assert ranks[1.0][1] == eos and (eos not in ranks[1.5] or ranks[1.5].index(eos) > 1), ranks
    else:
        assert ranks[1.0][0] != eos


def test_beam_step_ties(ops):
    """The documented rule on exact ties: equal logits inside a row -> the lower token id first; equal sums across beams -> the lower beam first, then
    the lower token id; eos with the same logit as another token (penalty 1) -> the lower id."""
    B, V, Tmax, eos = 3, 20, 6, 19
    x = torch.full((B, V), -4.0)
    x[:, 11] = x[:, 5] = 2.0            # the two best of every row tie
    x[:, 8] = 1.0
    x[2, 19] = 2.0                      # row 2: eos ties with them too
    st = _state(ops, 1, B, Tmax, [2], [Tmax], [-1.0, -1.0, -3.0], [0, 0, 0], [0], torch.Generator().manual_seed(0), eos)
    _run_step(ops, x.to(DEV), st, eos, 1.25, 1.0)
    assert st.beam_idx[0].tolist() == [0, 0, 1] and st.new_tokens[0].tolist() == [5, 11, 5]
    st = _state(ops, 1, B, Tmax, [2], [Tmax], [-3.0, -3.0, -1.0], [0, 0, 0], [0], torch.Generator().manual_seed(0), eos)
    _run_step(ops, x.to(DEV), st, eos, 1.25, 1.0)
    assert st.beam_idx[0].tolist() == [2, 2, 2] and st.new_tokens[0].tolist() == [5, 11, 19] and st.finished[0].tolist() == [0, 0, 1]
    # the first step: beams 1 .. B - 1 all sit at -1e10 + t = -1e10 in float32 -> beam 0's B candidates win, in t order
    st = _state(ops, 1, B, Tmax, [1], [Tmax], [0.0, -1e10, -1e10], [0, 0, 0], [0], torch.Generator().manual_seed(0), eos)
    _run_step(ops, x.to(DEV), st, eos, 1.25, 1.0)
    assert st.beam_idx[0].tolist() == [0, 0, 0] and st.new_tokens[0].tolist() == [5, 11, 8]


def test_beam_step_refusals(ops):
    from mlx_audio_amd import _lib

    def refused(B, V, match, **kw):
        st = _state(ops, 1, B, 6, [2], [6], [0.0] * B, [0] * B, [0], torch.Generator().manual_seed(0), 0)
        snap = [t.clone() for t in (st.scores, st.step, st.done, st.tokens[1], st.ind[1], st.beam_idx)]
        with pytest.raises(_lib.Mi355Error, match=match):
            ops.beam_step(torch.zeros(B, V, device=DEV), st, **{**dict(eos_id=0, softmax_smoothing=1.25), **kw})
        assert all(torch.equal(a, b) for a, b in zip(snap, (st.scores, st.step, st.done, st.tokens[1], st.ind[1], st.beam_idx)))
        assert torch.isnan(st.conf[1]).all() and torch.isnan(st.new_conf).all()

    refused(9, 100, r"\(-3\)")                     # MI355_ERR_UNSUPPORTED: beams above 8
    refused(3, 3, "V must exceed B")
    refused(3, 10, "eos_id", eos_id=10)
    refused(3, 10, "smoothing", softmax_smoothing=0.0)


# ------------------------------------------------------------------ beam_attention
def _attn_case(N, B, Tcap, heads, dh, g, Tmax=None):
    C = heads * dh
    q = torch.randn(N * B, C, generator=g)
    k = torch.randn(N * B, Tcap, C, generator=g)
    v = torch.randn(N * B, Tcap, C, generator=g)
    return q, k, v


@pytest.mark.parametrize("heads", [2, 20])
@pytest.mark.parametrize("dh", [64, 128])
def test_beam_attention(ops, dh, heads):
    """Tk = 1, 2, 63, 64, 65, 300 with N = 4 items at different ``pos`` (the last row, the middle, 0 and -1: a zero row), B = 3, ``ind`` the
    identity and a random permutation per position: within the bound, bit-equal on a repeat and for each item alone."""
    worst, B, N = 0.0, 3, 4
    for Tk in (1, 2, 63, 64, 65, 300):
        g = torch.Generator().manual_seed(dh * 7 + heads + Tk)
        q, k, v = _attn_case(N, B, Tk, heads, dh, g)
        pos = [Tk - 1, Tk // 2, 0, -1]
        for kind in ("identity", "permutation"):
            if kind == "identity":
                ind = torch.arange(B, dtype=torch.int32)[None, :, None].expand(N, B, Tk + 3).contiguous()
            else:
                ind = torch.stack([torch.stack([torch.randperm(B, generator=g) for _ in range(Tk + 3)], -1) for _ in range(N)]).to(torch.int32).contiguous()
            d = lambda t: t.to(DEV)
            run = lambda qq, kk, vv, ii, pp: ops.beam_attention(d(qq), d(kk), d(vv), d(ii), _i32(pp), _nan(qq.shape[0], heads * dh), beams=B, heads=heads, dh=dh)
            out = run(q, k, v, ind, pos)
            assert torch.equal(out, run(q, k, v, ind, pos))
            val, bound = E.beam_attention(q.numpy(), k.numpy(), v.numpy(), ind.numpy(), pos, beams=B, heads=heads, dh=dh, scale=1.0 / math.sqrt(dh))
            worst = max(worst, _ratio(out.cpu().double().numpy(), val, bound))
            assert not out[3 * B:].any()
            for n in range(3):
                sl = slice(n * B, (n + 1) * B)
                assert torch.equal(run(q[sl], k[sl], v[sl], ind[n:n + 1], pos[n:n + 1]), out[sl])
    print(f"beam_attention dh={dh} heads={heads}: worst error / bound = {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("dh", [64, 128])
def test_beam_attention_after_beam_steps(ops, dh):
    """20 seeded ``beam_step`` reorders: the caches stay where each beam wrote them and ``ind`` (the kernel's own) says where each beam's history
    lives; the result equals plain float64 attention over caches that are physically gathered by ``beam_idx`` after every step."""
    N, B, V, heads, steps = 2, 3, 50, 2, 20
    Tmax, C = steps + 2, heads * dh
    g = torch.Generator().manual_seed(dh)
    st = ops.beam_state(N, B, Tmax, [Tmax] * N, sos_id=1, device=DEV)
    k, v = torch.zeros(N * B, Tmax, C), torch.zeros(N * B, Tmax, C)
    kd, vd = k.to(DEV), v.to(DEV)
    pk, pv = k.numpy().astype(np.float64).copy(), v.numpy().astype(np.float64).copy()     # the physically gathered caches
    ident = np.arange(B, dtype=np.int32)[None, :, None].repeat(N, 0).repeat(Tmax, 2)
    worst, moved = 0.0, 0
    for t in range(steps):
        nk, nv, q = torch.randn(N * B, C, generator=g), torch.randn(N * B, C, generator=g), torch.randn(N * B, C, generator=g)
        kd[:, t], vd[:, t] = nk.to(DEV), nv.to(DEV)
        pk[:, t], pv[:, t] = nk.numpy(), nv.numpy()
        out = ops.beam_attention(q.to(DEV), kd, vd, st.ind[st.cur], _i32([t] * N), _nan(N * B, C), beams=B, heads=heads, dh=dh)
        val, bound = E.beam_attention(q.numpy(), pk, pv, ident, [t] * N, beams=B, heads=heads, dh=dh, scale=1.0 / math.sqrt(dh))
        worst = max(worst, _ratio(out.cpu().double().numpy(), val, bound))
        logits = 2.0 * torch.randn(N * B, V, generator=g)
        logits[:, 0] = -60.0                                   # eos never wins: all 20 steps stay live
        ops.beam_step(logits.to(DEV), st, eos_id=0)
        bi = st.beam_idx.cpu().numpy()
        moved += int((bi != np.arange(B)[None]).sum())
        src = (bi + B * np.arange(N)[:, None]).reshape(-1)
        pk, pv = pk[src].copy(), pv[src].copy()
    assert moved > steps                                       # the beams did reorder
    assert st.done.tolist() == [0] * N and st.step.tolist() == [steps + 1] * N
    print(f"beam_attention after {steps} beam_step reorders, dh={dh}: worst error / bound = {worst:.3f}")
    assert worst <= 1.0


def test_beam_attention_refusals(ops):
    from mlx_audio_amd import _lib

    def refused(dh, B, match, Tk=None, Tcap=4):
        q, k = torch.zeros(B, 2 * dh, device=DEV), torch.zeros(B, Tcap, 2 * dh, device=DEV)
        out = _nan(B, 2 * dh)
        with pytest.raises(_lib.Mi355Error, match=match):
            ops.beam_attention(q, k, k, torch.zeros(1, B, 4, dtype=torch.int32, device=DEV), _i32([0]), out, beams=B, heads=2, dh=dh, Tk=Tk)
        assert torch.isnan(out).all()

    refused(32, 3, "dh must be 64 or 128")
    refused(64, 9, r"\(-3\)")
    refused(64, 3, "ld_ind", Tcap=6, Tk=6)      # more positions than the table holds
