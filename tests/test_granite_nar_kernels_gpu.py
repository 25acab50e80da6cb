"""``csrc/granite_nar.hip`` against the float64 statements of ``_ops_emu_granite_nar.py`` on the same float32 inputs: ``shaw_block_attention``,
``selfcond_rows``, ``posterior_pool`` and ``qformer_windows``.  The bars are the per-element float32 rounding bounds derived there (not tuned); every
test prints its largest error / bound ratio (docs/COVERAGE.md records them).  Common to all four: outputs start as NaN, rows at and beyond ``lens``
are exactly zero, an item of a ragged batch is bit-equal to that item alone, a repeat is bit-equal, and a refused call leaves its outputs untouched."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import _ops_emu_granite_nar as E  # noqa: E402

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


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------ shaw_block_attention
@pytest.mark.parametrize("ctx", E.SHAW_CTX)
@pytest.mark.parametrize("heads", [1, 3])
@pytest.mark.parametrize("dh", [64, 128])
def test_shaw_block_attention(ops, dh, heads, ctx):
    """T = 1, ctx - 1, ctx, ctx + 1 and 2 ctx + 37 with ``max_pos`` = ctx - 1 (the exact fit) and 512, a batch of four with the lengths 1, ctx,
    ctx + 1 and T (cut to T): within the bound (zero keys of the last block visible), rows beyond ``lens`` zero, a repeat bit-equal, the same call
    on thirds of a fused q | k | v buffer with a wider output bit-equal, every item bit-equal to that item alone at T = its own length."""
    worst, hd = 0.0, heads * dh
    for T in E.shaw_lengths(ctx):
        for max_pos in (ctx - 1, 512):
            q, k, v, table = E.shaw_inputs(dh, heads, ctx, T, max_pos)
            lens = E.shaw_ragged(ctx, T)
            kw = dict(heads=heads, dh=dh, ctx=ctx, max_pos=max_pos)
            qd, kd, vd, td = _d(q), _d(k), _d(v), _d(table)
            out = ops.shaw_block_attention(qd, kd, vd, td, _nan(4, T, hd), lens=_i32(lens), **kw)
            assert torch.equal(out, ops.shaw_block_attention(qd, kd, vd, td, _nan(4, T, hd), lens=_i32(lens), **kw)), "two calls on the same bytes differ"
            fused = torch.cat([qd, kd, vd, _nan(4, T, 4)], -1)
            wide = _nan(4, T, hd + 8)
            ops.shaw_block_attention(fused[..., :hd], fused[..., hd:2 * hd], fused[..., 2 * hd:3 * hd], td, wide[..., :hd], lens=_i32(lens), **kw)
            assert torch.equal(wide[..., :hd], out) and torch.isnan(wide[..., hd:]).all()
            val, bound = E.shaw_block_attention(q, k, v, table, lens=lens, **kw)
            worst = max(worst, _ratio(out.cpu().double().numpy(), val, bound))
            for b, n in enumerate(lens):
                assert not out[b, n:].any(), "rows beyond lens are not exactly zero"
                alone = ops.shaw_block_attention(qd[b:b + 1, :n].contiguous(), kd[b:b + 1, :n].contiguous(), vd[b:b + 1, :n].contiguous(), td,
                                                 _nan(1, n, hd), **kw)
                assert torch.equal(alone[0], out[b, :n]), (T, max_pos, b)
    print(f"shaw_block_attention dh={dh} heads={heads} ctx={ctx}: worst error / bound = {worst:.3f}")
    assert worst <= 1.0


def test_shaw_block_attention_zero_length(ops):
    """``lens[b] == 0``: the item's rows are zeros and nothing of it is read."""
    q, k, v, table = E.shaw_inputs(64, 1, 8, 20, 7, B=2)
    q[0] = np.nan
    out = ops.shaw_block_attention(_d(q), _d(q), _d(q), _d(table), _nan(2, 20, 64), heads=1, dh=64, ctx=8, max_pos=7, lens=_i32([0, 20]))
    assert not out[0].any() and torch.isfinite(out[1]).all()


def test_shaw_block_attention_refusals(ops):
    from mlx_audio_amd import _lib

    def refused(match, dh=64, ctx=8, max_pos=7, rows=None, lens=None, T=10):
        q = torch.zeros(2, T, 2 * dh, device=DEV)
        out = _nan(2, T, 2 * dh)
        table = torch.zeros(2 * max_pos + 1 if rows is None else rows, dh, device=DEV)
        with pytest.raises(_lib.Mi355Error, match=match):
            ops.shaw_block_attention(q, q, q, table, out, heads=2, dh=dh, ctx=ctx, max_pos=max_pos, lens=lens)
        assert torch.isnan(out).all()

    refused("dh must be 64 or 128", dh=32)
    refused("ctx must be at least 1", ctx=0)
    refused("max_pos", ctx=9, max_pos=7)                 # the reference's index would leave the table
    refused("the table has", rows=16)
    refused("the table has", rows=14)
    refused("lens must lie", lens=_i32([3, 11]))
    refused("lens must lie", lens=_i32([-1, 4]))
    # the exact fit passes
    q = torch.randn(1, 9, 64, device=DEV)
    out = ops.shaw_block_attention(q, q, q, torch.randn(17, 64, device=DEV), _nan(1, 9, 64), heads=1, dh=64, ctx=9, max_pos=8)
    assert torch.isfinite(out).all()


# ------------------------------------------------------------------ selfcond_rows
@pytest.mark.parametrize("V", [2, 64, 65, 348, 1024])
def test_selfcond_rows(ops, V):
    """rows = 1, 4, 5 and 131 (the wave form packs four rows into a workgroup), a padded row stride, logits of a range near 20: the probabilities within
    the bound, ``p_blank`` the bits of column 0, a repeat bit-equal, every row bit-equal to that row alone."""
    worst = 0.0
    for rows in (1, 4, 5, 131):
        g = torch.Generator().manual_seed(V * 1000 + rows)
        x = 3.0 * torch.randn(rows, V + 3, generator=g)
        xd = x.to(DEV)[:, :V]
        probs, pb = ops.selfcond_rows(xd, probs=_nan(rows, V + 5)[:, :V], p_blank=_nan(rows))
        p2, pb2 = ops.selfcond_rows(xd, probs=_nan(rows, V), p_blank=_nan(rows))
        assert torch.equal(probs, p2) and torch.equal(pb, pb2) and torch.equal(pb, probs[:, 0])
        val, vb, bound = E.selfcond_rows(x[:, :V].numpy(), ops.SELFCOND_WAVE_MAX_V)
        worst = max(worst, _ratio(probs.cpu().double().numpy(), val, bound))
        for r in (0, rows - 1):
            pa, ba = ops.selfcond_rows(xd[r:r + 1].contiguous())
            assert torch.equal(pa[0], probs[r]) and torch.equal(ba[0], pb[r])
    print(f"selfcond_rows V={V}: worst error / bound = {worst:.3f}")
    assert worst <= 1.0


def test_selfcond_rows_refusals(ops):
    from mlx_audio_amd import _lib

    x = torch.zeros(3, 8, device=DEV)
    probs, pb = _nan(3, 8), _nan(3)
    with pytest.raises(_lib.Mi355Error, match="selfcond_rows"):
        _lib.call_struct("mi355_selfcond_rows", "mi355_selfcond_rows_args", 0, logits=x.data_ptr(), ld=8, rows=3, V=9, probs=probs.data_ptr(), ld_probs=8,
                         p_blank=pb.data_ptr())
    with pytest.raises(_lib.Mi355Error, match="selfcond_rows"):
        _lib.call_struct("mi355_selfcond_rows", "mi355_selfcond_rows_args", 0, logits=x.data_ptr(), ld=8, rows=3, V=0, probs=probs.data_ptr(), ld_probs=8,
                         p_blank=pb.data_ptr())
    assert torch.isnan(probs).all() and torch.isnan(pb).all()


# ------------------------------------------------------------------ posterior_pool
@pytest.mark.parametrize("window", [1, 4, 5])
def test_posterior_pool(ops, window):
    """T with ``T % window`` in {0, 1, window - 1} at two sizes each, C = 130 and 260 (one and two channels per thread, the last group partial), a
    ragged batch (the full length, a length inside a window, one frame, zero), blank probabilities that include exact 1 (a window of weight 0 meets
    the 1e-6 floor): within the bound, windows beyond the item zero, items bit-equal alone, a repeat bit-equal."""
    worst = 0.0
    for rem in sorted({0, 1 % window, window - 1}):
        for T in (window + rem, 7 * window + rem):
            for C in (130, 260):
                g = torch.Generator().manual_seed(window * 100 + T * 7 + C)
                h = torch.randn(4, T, C + 2, generator=g)
                pb = torch.rand(4, T, generator=g)
                pb[:, :min(window, T)] = 1.0                        # the first window: all blank
                pb[0, -1] = 1.0
                lens = [T, max(T - window // 2 - 1, 1), 1, 0]
                hd, pd = h.to(DEV)[..., :C], pb.to(DEV)
                nw = -(-T // window)
                out = ops.posterior_pool(hd, pd, window, lens=_i32(lens), out=_nan(4, nw, C))
                assert torch.equal(out, ops.posterior_pool(hd, pd, window, lens=_i32(lens), out=_nan(4, nw, C + 4)[..., :C]))
                val, bound = E.posterior_pool(h[..., :C].numpy(), pb.numpy(), window, lens)
                worst = max(worst, _ratio(out.cpu().double().numpy(), val, bound))
                for b, n in enumerate(lens):
                    assert not out[b, -(-n // window):].any(), "windows beyond the item are not exactly zero"
                    if n:
                        alone = ops.posterior_pool(hd[b:b + 1, :n].contiguous(), pd[b:b + 1, :n].contiguous(), window)
                        assert torch.equal(alone[0], out[b, :alone.shape[1]])
    print(f"posterior_pool window={window}: worst error / bound = {worst:.3f}")
    assert worst <= 1.0


def test_posterior_pool_refusals(ops):
    from mlx_audio_amd import _lib

    h, pb, out = torch.zeros(1, 6, 8, device=DEV), torch.zeros(1, 6, device=DEV), _nan(1, 1, 8)
    with pytest.raises(_lib.Mi355Error, match="window must be at least 1"):
        ops.posterior_pool(h, pb, 0, out=out)
    assert torch.isnan(out).all()


# ------------------------------------------------------------------ qformer_windows
@pytest.mark.parametrize("block,rate", [(15, 5), (4, 2)])
def test_qformer_windows(ops, block, rate):
    """T = 1, block - 1, block, block + 1 (and 3 block + 2), C = 130 and 516, a ragged batch (the full length, one frame less, one frame, zero): both
    outputs within the bound, padded rows equal to the bare positions / query, items bit-equal alone, a repeat bit-equal."""
    worst, nq = 0.0, block // rate
    for T in (1, block - 1, block, block + 1, 3 * block + 2):
        for C in (130, 516):
            g = torch.Generator().manual_seed(block * 1000 + T * 10 + C)
            h = torch.randn(4, T, C + 6, generator=g)
            query, pos = torch.randn(nq, C, generator=g), torch.randn(block, C, generator=g)
            lens = [T, max(T - 1, 1), 1, 0]
            hd, qd, pd = h.to(DEV)[..., :C], query.to(DEV), pos.to(DEV)
            nb = -(-T // block)
            run = lambda hh, ll: ops.qformer_windows(hh, qd, pd, block=block, rate=rate, lens=ll, queries=_nan(hh.shape[0] * -(-hh.shape[1] // block), nq, C),
                                                     kv=_nan(hh.shape[0] * -(-hh.shape[1] // block), block, C))
            qs, kv = run(hd, _i32(lens))
            q2, kv2 = run(hd, _i32(lens))
            assert torch.equal(qs, q2) and torch.equal(kv, kv2)
            vq, vk, bq, bk = E.qformer_windows(h[..., :C].numpy(), query.numpy(), pos.numpy(), block, rate, lens)
            worst = max(worst, _ratio(qs.cpu().double().numpy(), vq, bq), _ratio(kv.cpu().double().numpy(), vk, bk))
            kv4 = kv.view(4, nb * block, C)
            for b, n in enumerate(lens):
                assert torch.equal(kv4[b, n:], pd.repeat(nb, 1)[n:]), "a padded row is not the bare position row"
                if n:
                    aq, ak = run(hd[b:b + 1, :n].contiguous(), None)
                    na = aq.shape[0]
                    assert torch.equal(aq, qs[b * nb:b * nb + na]) and torch.equal(ak, kv[b * nb:b * nb + na])
            assert torch.equal(qs[3 * nb:], qd[None].expand(nb, nq, C))           # the empty item: the learned query alone
    print(f"qformer_windows block={block} rate={rate}: worst error / bound = {worst:.3f}")
    assert worst <= 1.0


def test_qformer_windows_refusals(ops):
    from mlx_audio_amd import _lib

    h = torch.zeros(1, 6, 8, device=DEV)
    queries, kv = _nan(2, 2, 8), _nan(2, 5, 8)
    with pytest.raises(_lib.Mi355Error, match="qformer_windows"):
        ops.qformer_windows(h, torch.zeros(2, 8, device=DEV), torch.zeros(5, 8, device=DEV), block=5, rate=2, queries=queries, kv=kv)
    with pytest.raises(_lib.Mi355Error, match="multiple of rate"):
        _lib.call_struct("mi355_qformer_windows", "mi355_qformer_windows_args", 0, h=h.data_ptr(), h_bstride=48, ldh=8, B=1, T=6, C=8, block=5, rate=2,
                         query=h.data_ptr(), positions=h.data_ptr(), queries=queries.data_ptr(), kv=kv.data_ptr())
    assert torch.isnan(queries).all() and torch.isnan(kv).all()
