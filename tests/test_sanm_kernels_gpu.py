"""``csrc/sanm.hip`` against float64 on the host, on the same float32 inputs: ``sanm_input``, ``ctc_rows`` and ``ctc_collapse``.  The bars are
per-element float32 rounding bounds, derived below and not tuned (U = 2^-24); every test prints its largest error / bound ratio (docs/COVERAGE.md
records them).  Integer outputs (ids, tokens, counts, frames) and the top-2 gaps are compared exactly."""
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import _sensevoice_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24


@pytest.fixture(scope="module")
def ops():
    from mlx_audio_amd import ops

    ops.require_gpu()
    return ops


# ------------------------------------------------------------------ sanm_input
def _input_ref(feats, lens, means, istd, embed, qids, pe, m, n, scale):
    """(value, bound) in float64.  The kernel rounds four times: a = f + mean, b = a * istd, c = b * scale, r = c + pe; to first order the error is
    at most U (|c| + |c| + |c| + |r|) (each product's error carried through the later exact-in-float64 factors)."""
    B, T, D = feats.shape
    rows, W = 4 + -(-T // n), m * D
    val, bound = np.zeros((B, rows, W)), np.zeros((B, rows, W))
    s = float(np.float32(scale))
    for b in range(B):
        L = int(lens[b])
        u = R.apply_lfr(feats[b, :L].astype(np.float64), m, n)
        if means is not None:
            u = (u + means.astype(np.float64)) * istd.astype(np.float64)
        u = np.concatenate([embed.astype(np.float64)[qids[b]], u]) * s
        r = u + (pe[:u.shape[0]].astype(np.float64) if pe is not None else 0.0)
        val[b, :u.shape[0]], bound[b, :u.shape[0]] = r, U * (3 * np.abs(u) + np.abs(r)) * 1.001
    return val, bound


@pytest.mark.parametrize("T,m,n,D", [(1, 7, 6, 80), (5, 7, 6, 80), (6, 7, 6, 80), (7, 7, 6, 80), (13, 7, 6, 80), (300, 7, 6, 80), (50, 5, 3, 40), (9, 1, 1, 16)])
def test_sanm_input(ops, T, m, n, D):
    """Ragged lens at B = 3 (the full length, about half, one frame), row stride > D and == D, with and without CMVN, with and without positions:
    within the rounding bound, ``out_lens`` equal, rows at and beyond ``out_lens`` exactly zero, two calls bit-equal."""
    from mlx_audio_amd.stt.models.sensevoice.sensevoice import position_table

    g = torch.Generator().manual_seed(T * 131 + m)
    W, rows = m * D, 4 + -(-T // n)
    worst = 0.0
    for lens in ([T, max(1, T // 2), 1], [T, T, T]):
        for strided in (False, True):
            for cmvn in (True, False):
                for with_pe in (True, False):
                    base = 12.0 + 4.0 * torch.randn(3, T, D + (8 if strided else 0), generator=g)
                    feats = base.to(DEV)[:, :, :D]
                    means, istd = (-12.0 + torch.randn(W, generator=g), 0.25 + 0.05 * torch.rand(W, generator=g)) if cmvn else (None, None)
                    embed = 0.5 * torch.randn(16, W, generator=g)
                    qids = torch.randint(0, 16, (3, 4), generator=g, dtype=torch.int32)
                    pe = position_table(rows + 3, W) if with_pe else None
                    scale = math.sqrt(512.0)
                    dv = lambda t: None if t is None else t.to(DEV)
                    args = dict(lfr_m=m, lfr_n=n, scale=scale, lens=torch.tensor(lens, dtype=torch.int32, device=DEV), means=dv(means), istd=dv(istd))
                    x, ol = ops.sanm_input(feats, dv(embed), dv(qids), dv(pe), **args)
                    x2, _ = ops.sanm_input(feats, dv(embed), dv(qids), dv(pe), x=torch.full((3, rows, W + 4), 7.0, device=DEV)[:, :, :W], **args)
                    assert torch.equal(x, x2)
                    assert ol.tolist() == [4 + -(-L // n) for L in lens]
                    np_ = lambda t: None if t is None else t.numpy()
                    val, bound = _input_ref(base[:, :, :D].numpy(), lens, np_(means), np_(istd), embed.numpy(), qids.numpy(), np_(pe), m, n, scale)
                    got = x.cpu().double().numpy()
                    for b, L in enumerate(lens):
                        assert not got[b, 4 + -(-L // n):].any()
                    worst = max(worst, float((np.abs(got - val) / (bound + 1e-300)).max()))
    print(f"sanm_input T={T} m={m} n={n} D={D}: worst error / bound = {worst:.3f}")
    assert worst <= 1.0


def test_sanm_input_refuses_bad_arguments(ops):
    from mlx_audio_amd import _lib

    f, e, q = torch.zeros(1, 10, 80, device=DEV), torch.zeros(16, 560, device=DEV), torch.zeros(1, 4, dtype=torch.int32, device=DEV)
    with pytest.raises(_lib.Mi355Error, match="position table"):
        ops.sanm_input(f, e, q, torch.zeros(5, 560, device=DEV), lfr_m=7, lfr_n=6, scale=1.0)
    with pytest.raises(AssertionError):
        ops.sanm_input(f, e, q, None, lfr_m=7, lfr_n=6, scale=1.0, means=torch.zeros(560, device=DEV))


# ------------------------------------------------------------------ ctc_rows
def _rows_case(rows, V, ld, seed):
    """Logits with the edge rows the issue lists: the maximum at column 0 and at V - 1, exact ties (first index wins, gap 0), an all-equal row,
    magnitudes of +-80."""
    g = torch.Generator().manual_seed(seed)
    x = 3.0 * torch.randn(rows, ld, generator=g)
    kinds = ["max0", "maxlast", "tie", "equal", "big", "bigtie"]
    for r in range(rows):
        kind = kinds[r % 8] if r % 8 < len(kinds) else "plain"
        if kind == "max0":
            x[r, 0] = 40.0
        elif kind == "maxlast":
            x[r, V - 1] = 40.0
        elif kind == "tie" and V > 1:
            c = sorted(set(int(v) for v in torch.randint(0, V, (3,), generator=g)) | {V - 1})
            x[r, c] = 25.0
        elif kind == "equal":
            x[r, :V] = -1.5
        elif kind == "big":
            x[r, :V] = 160.0 * torch.rand(V, generator=g) - 80.0
        elif kind == "bigtie" and V > 2:
            x[r, :V] = 160.0 * torch.rand(V, generator=g) - 80.0
            x[r, V // 2] = x[r, V - 1] = 80.0
    return x


def _rows_ref(x):
    """float64 on the float32 logits: ids (first maximum), gap (float32-rounded: the difference of two floats is exact in float64), lp, logp and
    their bounds.  The kernel's sum S = sum exp(x - M): every term carries U |x - m| from its rounded argument, 2 U from expf and one multiply
    when the thread's running maximum is raised (the raises of one thread climb at most D = max - min in total) and again when the thread's sum is
    rescaled to the row maximum; a thread adds n = ceil(V / 256) terms in sequence and the joins add 8 more: dS / S <= U (2 D + 5 n + 16).
    lp = -log S adds logf's rounding, 2 U |log S|; logp = (x - M) - log S adds U (|x - M| + |logp|)."""
    rows, V = x.shape
    M = x.max(-1)
    ids = (x == M[:, None]).argmax(-1)
    other = x.copy()
    other[np.arange(rows), ids] = -np.inf
    gap = (M - other.max(-1)).astype(np.float32) if V > 1 else np.zeros(rows, dtype=np.float32)
    S = np.exp(x - M[:, None]).sum(-1)
    D = M - x.min(-1)
    b_lp = U * (2 * D + 5 * math.ceil(V / 256) + 16 + 2 * np.abs(np.log(S)))
    logp = (x - M[:, None]) - np.log(S)[:, None]
    return ids, gap, -np.log(S), b_lp, logp, b_lp[:, None] + U * (np.abs(x - M[:, None]) + np.abs(logp))


@pytest.mark.parametrize("V", [1, 2, 63, 64, 65, 255, 256, 257, 1024, 25055])
def test_ctc_rows(ops, V):
    """rows 1, 5 and 300, row stride == V and > V, with and without the ``logp`` output (also in place): ids and gaps exact on every row, the
    arg-max log-probability and ``logp`` within the bound, two calls bit-equal."""
    worst_lp = worst_logp = 0.0
    for rows in (1, 5, 300):
        for ld in (V, V + 9):
            xh = _rows_case(rows, V, ld, seed=V * 7 + rows)
            x = xh.to(DEV)[:, :V]
            ids, gap, lp = ops.ctc_rows(x)
            logp = torch.full((rows, V + 3), 9.0, device=DEV)[:, :V]
            ids2, gap2, lp2 = ops.ctc_rows(x, logp=logp)
            assert torch.equal(ids, ids2) and torch.equal(gap, gap2) and torch.equal(lp, lp2)
            inplace = x.clone() if ld == V else xh.to(DEV)[:, :V]
            ops.ctc_rows(inplace, logp=inplace)
            assert torch.equal(inplace, logp)
            w_ids, w_gap, w_lp, b_lp, w_logp, b_logp = _rows_ref(xh[:, :V].double().numpy())
            assert ids.dtype == torch.int32 and np.array_equal(ids.cpu().numpy(), w_ids), (V, rows, ld)
            assert np.array_equal(gap.cpu().numpy(), w_gap), (V, rows, ld)
            worst_lp = max(worst_lp, float((np.abs(lp.cpu().double().numpy() - w_lp) / b_lp).max()))
            worst_logp = max(worst_logp, float((np.abs(logp.cpu().double().numpy() - w_logp) / b_logp).max()))
    print(f"ctc_rows V={V}: worst error / bound: lp {worst_lp:.3f}, logp {worst_logp:.3f}")
    assert worst_lp <= 1.0 and worst_logp <= 1.0


def test_ctc_rows_fills_slices_of_caller_buffers(ops):
    x = _rows_case(40, 300, 300, seed=2).to(DEV)
    ids, gap, lp = ops.ctc_rows(x)
    ids2 = torch.full((50,), -7, dtype=torch.int32, device=DEV)
    gap2, lp2 = torch.zeros(50, device=DEV), torch.zeros(50, device=DEV)
    ops.ctc_rows(x[:13], ids=ids2[:13], gap=gap2[:13], lp=lp2[:13])
    ops.ctc_rows(x[13:], ids=ids2[13:40], gap=gap2[13:40], lp=lp2[13:40])
    assert torch.equal(ids2[:40], ids) and torch.equal(gap2[:40], gap) and torch.equal(lp2[:40], lp) and bool((ids2[40:] == -7).all())


# ------------------------------------------------------------------ ctc_collapse
def _collapse_ref(ids, lens, skip, blank):
    B, T = ids.shape
    tokens, frames, counts = np.full((B, T), -1, dtype=np.int32), np.full((B, T), -1, dtype=np.int32), np.zeros(B, dtype=np.int32)
    for b in range(B):
        n = T if lens is None else lens[b]
        toks, frs = R.collapse(ids[b, skip:n].tolist(), blank, return_frames=True) if n > skip else ([], [])
        counts[b] = len(toks)
        tokens[b, :len(toks)], frames[b, :len(toks)] = toks, [f + skip for f in frs]
    return tokens, counts, frames


def _check_collapse(ops, ids, lens, skip, blank, strided=False):
    ids = np.asarray(ids, dtype=np.int32)
    B, T = ids.shape
    dev_ids = torch.from_numpy(np.pad(ids, ((0, 0), (0, 5)), constant_values=blank + 1) if strided else ids).to(DEV)[:, :T]
    ld = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
    tokens, counts, frames = ops.ctc_collapse(dev_ids, lens=ld, skip=skip, blank=blank, return_frames=True)
    t2, c2 = ops.ctc_collapse(dev_ids, lens=ld, skip=skip, blank=blank)
    w_tok, w_cnt, w_frm = _collapse_ref(ids, lens, skip, blank)
    assert np.array_equal(counts.cpu().numpy(), w_cnt), (counts.tolist(), w_cnt.tolist())
    assert np.array_equal(tokens.cpu().numpy(), w_tok) and np.array_equal(frames.cpu().numpy(), w_frm)
    assert torch.equal(tokens, t2) and torch.equal(counts, c2)
    return w_tok, w_cnt


def test_ctc_collapse_scripted_rows(ops):
    """``a, blank, a`` keeps both a; all blank; a repeat across frames 63 / 64 and a change there; ``skip`` 4 with ``lens`` <= 4; row ``skip`` equal
    to row ``skip - 1`` still counts."""
    tok, cnt = _check_collapse(ops, [[5, 0, 5, 0, 6, 6, 0, 5]], None, 0, 0)
    assert tok[0, :cnt[0]].tolist() == [5, 5, 6, 5]
    _check_collapse(ops, [[0] * 70, [3] * 70], None, 0, 0)
    row = [0] * 129
    row[62:66] = [7, 7, 7, 7]            # a repeat across the chunk boundary 63 / 64: one token, first frame 62
    row2 = [0] * 129
    row2[63], row2[64] = 7, 8            # a change there: two tokens
    row3 = [9] * 129                     # one run over three chunks
    row4 = [(t // 2) % 3 for t in range(129)]
    tok, cnt = _check_collapse(ops, [row, row2, row3, row4], None, 0, 0)
    assert tok[0, :cnt[0]].tolist() == [7] and tok[1, :cnt[1]].tolist() == [7, 8] and tok[2, :cnt[2]].tolist() == [9]
    ids = [[4, 4, 4, 4, 4, 4, 0, 2], [1, 2, 3, 9, 9, 0, 0, 9], [1, 1, 1, 1, 1, 1, 1, 1], [5, 5, 5, 5, 5, 5, 5, 5]]
    tok, cnt = _check_collapse(ops, ids, [8, 8, 4, 3], 4, 0)
    assert tok[0, :cnt[0]].tolist() == [4, 2] and tok[1, :cnt[1]].tolist() == [9, 9] and cnt[2] == 0 and cnt[3] == 0
    _check_collapse(ops, ids, [8, 8, 4, 3], 4, 9, strided=True)   # another blank id


@pytest.mark.parametrize("T", [1, 64, 65, 129])
def test_ctc_collapse_random_rows(ops, T):
    g = np.random.default_rng(T)
    for B, skip in ((1, 0), (5, 0), (5, 4), (37, 2)):
        ids = g.integers(0, 4, (B, T)).astype(np.int32)
        ids[g.random((B, T)) < 0.4] = 0
        lens = [int(v) for v in g.integers(0, T + 1, B)]
        lens[0] = T
        _check_collapse(ops, ids, lens, skip, 0)
        _check_collapse(ops, ids, None, skip, 0, strided=True)
