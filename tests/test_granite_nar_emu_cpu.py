"""Two kinds of test, no GPU.  The first checks the change itself: the header's declarations, the struct layouts and the constants of ``ops``.  The
others check the TEST SIDE: the float64 statements of ``_ops_emu_granite_nar.py``, which ``test_granite_nar_kernels_gpu.py`` holds the kernels to,
against plain restatements of the reference's lines (the block reshaping and the einsum of encoder.py:80-127, the softmax of :280-281,
``_posterior_weighted_pool`` of :302-334, the window assembly of projector.py:190-215) -- so that a mistake in a statement cannot pass as the
kernel's contract -- and the MUTANT check: on the GPU test's own inputs, the statement that masks the padded keys of the last block differs from
the true one by far more than the test's bound, so the test does tell the two rules apart."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import _ops_emu_granite_nar as E  # noqa: E402


def test_entry_points_declared_and_constants_match_the_header():
    from mlx_audio_amd import _lib, ops

    names = _lib.declared_functions()
    for fn in ("mi355_shaw_block_attention", "mi355_selfcond_rows", "mi355_posterior_pool", "mi355_qformer_windows"):
        assert fn in names and callable(getattr(ops, fn[len("mi355_"):]))
    header = open(_lib.HEADER).read()
    assert int(re.search(r"#define MI355_SELFCOND_WAVE_MAX_V (\d+)", header).group(1)) == ops.SELFCOND_WAVE_MAX_V
    assert _lib.ABI_VERSION == 37                     # additive: the version stays
    fields = lambda name: [f for f, _ in _lib.STRUCTS[name]._fields_]
    assert fields("mi355_shaw_block_attention_args") == ["q", "q_bstride", "ldq", "k", "k_bstride", "ldk", "v", "v_bstride", "ldv", "table", "ldt", "rows",
                                                         "max_pos", "lens", "B", "T", "heads", "dh", "ctx", "scale", "out", "out_bstride", "ldo"]
    assert fields("mi355_selfcond_rows_args") == ["logits", "ld", "rows", "V", "probs", "ld_probs", "p_blank"]
    assert fields("mi355_posterior_pool_args") == ["h", "h_bstride", "ldh", "p_blank", "pb_bstride", "window", "lens", "B", "T", "C", "out", "out_bstride",
                                                   "ldo"]
    assert fields("mi355_qformer_windows_args") == ["h", "h_bstride", "ldh", "lens", "B", "T", "C", "block", "rate", "query", "positions", "queries", "kv"]
    # the C compiler's layout of the same declarations (natural alignment, 8-byte pointers)
    assert ctypes.sizeof(_lib.STRUCTS["mi355_shaw_block_attention_args"]) == 152
    assert ctypes.sizeof(_lib.STRUCTS["mi355_selfcond_rows_args"]) == 56
    assert ctypes.sizeof(_lib.STRUCTS["mi355_posterior_pool_args"]) == 96
    assert ctypes.sizeof(_lib.STRUCTS["mi355_qformer_windows_args"]) == 88


# ------------------------------------------------------------------ the reference's lines, restated in float64 numpy
def _reference_attention(q, k, v, table, heads, dh, ctx, max_pos):
    """encoder.py:86-126 for one item from the projections on: pad to a multiple of ctx with ZERO rows (to_q / to_kv have no bias, so the padded rows
    of h project to zeros), reshape into blocks and heads, q k^T, the Shaw lookup ``rel[i, j] = table[clip(i - j, -ctx, ctx) + max_pos]`` and the
    einsum "bmhcd,crd->bmhcr", one scale on both, softmax over all ctx keys, @ v, trim."""
    T = q.shape[0]
    pad = (ctx - (T % ctx)) % ctx
    padz = lambda z: np.concatenate([z, np.zeros((pad, z.shape[1]))], 0) if pad else z
    n_blocks = (T + pad) // ctx
    resh = lambda z: padz(z).reshape(1, n_blocks, ctx, heads, dh).transpose(0, 1, 3, 2, 4)
    q5, k5, v5 = resh(q), resh(k), resh(v)
    scale = dh ** -0.5
    logits = (q5 @ k5.transpose(0, 1, 2, 4, 3)) * scale
    idx = np.arange(ctx)
    dist = np.clip(idx[:, None] - idx[None, :], -ctx, ctx) + max_pos
    rel = table[dist]                                                  # [ctx, ctx, dh]
    logits = logits + np.einsum("bmhcd,crd->bmhcr", q5, rel) * scale
    e = np.exp(logits - logits.max(-1, keepdims=True))
    attn = e / e.sum(-1, keepdims=True)
    out = (attn @ v5).transpose(0, 1, 3, 2, 4).reshape(n_blocks * ctx, heads * dh)
    return out[:T]


@pytest.mark.parametrize("dh,heads,ctx,max_pos", [(64, 2, 8, 7), (64, 1, 33, 512), (128, 3, 50, 64)])
def test_shaw_statement_is_the_reference_attention(dh, heads, ctx, max_pos):
    for T in (1, ctx - 1, ctx, ctx + 1, 2 * ctx + 5):
        q, k, v, table = (t.astype(np.float64) for t in E.shaw_inputs(dh, heads, ctx, T, max_pos, B=3))
        lens = [T, max(T // 2, 1), 1]
        val, bound = E.shaw_block_attention(q, k, v, table, heads=heads, dh=dh, ctx=ctx, max_pos=max_pos, lens=lens)
        assert (bound >= 0).all()
        for b, n in enumerate(lens):
            ref = _reference_attention(q[b, :n], k[b, :n], v[b, :n], table, heads, dh, ctx, max_pos)
            assert np.abs(val[b, :n] - ref).max() < 1e-12 and not val[b, n:].any()


def test_shaw_mutant_masking_the_padded_keys_is_told_apart():
    """On the GPU test's inputs (every case whose last block has padded keys), the statement that masks those keys misses the true one by more than
    10 bounds somewhere in every such case (the closest, one padded key of 128, by about 50); where no block is padded the two agree exactly."""
    for dh, heads in ((64, 1), (128, 3)):
        for ctx in E.SHAW_CTX:
            for T in E.shaw_lengths(ctx):
                max_pos = ctx - 1
                q, k, v, table = E.shaw_inputs(dh, heads, ctx, T, max_pos)
                lens = E.shaw_ragged(ctx, T)
                kw = dict(heads=heads, dh=dh, ctx=ctx, max_pos=max_pos, lens=lens)
                true, bound = E.shaw_block_attention(q, k, v, table, **kw)
                mutant, _ = E.shaw_block_attention(q, k, v, table, mask_padded=True, **kw)
                for b, n in enumerate(lens):
                    ratio = float((np.abs(mutant[b, :n] - true[b, :n]) / bound[b, :n]).max())
                    if n % ctx:
                        assert ratio > 10.0, (dh, heads, ctx, T, b, ratio)
                    else:
                        assert ratio == 0.0


def test_selfcond_statement_is_the_reference_softmax():
    import torch

    x = 3.0 * torch.randn(7, 348, generator=torch.Generator().manual_seed(0), dtype=torch.float64)
    p, pb, bound = E.selfcond_rows(x.numpy())
    ref = torch.softmax(x, -1).numpy()
    assert np.abs(p - ref).max() < 1e-15 and np.array_equal(pb, p[:, 0]) and (bound > 0).all()


def _reference_pool(h, blank_probs, window):
    """encoder.py:310-334 for one item."""
    T, C = h.shape
    n_full = T // window
    tail = T - n_full * window
    if tail == 0:
        importance = (1.0 - blank_probs).reshape(n_full, window)
        weights = importance / np.maximum(importance.sum(-1, keepdims=True), 1e-6)
        return (h.reshape(n_full, window, C) * weights[..., None]).sum(1)
    pad = window - tail
    h_p = np.concatenate([h, np.zeros((pad, C))], 0)
    imp = np.concatenate([1.0 - blank_probs, np.zeros(pad)], 0)
    n = (T + pad) // window
    imp_w = imp.reshape(n, window)
    weights = imp_w / np.maximum(imp_w.sum(-1, keepdims=True), 1e-6)
    return (h_p.reshape(n, window, C) * weights[..., None]).sum(1)


@pytest.mark.parametrize("window", [1, 4, 5])
def test_pool_statement_is_the_reference_pool(window):
    rng = np.random.default_rng(window)
    for T in (1, window, window + 1, 3 * window - 1, 4 * window):
        h, pb = rng.standard_normal((3, T, 10)), rng.random((3, T))
        pb[:, :min(window, T)] = 1.0                                    # a window of weight 0: the 1e-6 floor
        lens = [T, max(T - 2, 1), 0]
        val, bound = E.posterior_pool(h, pb, window, lens)
        assert (bound >= 0).all()
        for b, n in enumerate(lens):
            nw = -(-n // window)
            if n:
                assert np.abs(val[b, :nw] - _reference_pool(h[b, :n], pb[b, :n], window)).max() < 1e-13
            assert not val[b, nw:].any()


def _reference_windows(h, query, positions, block, rate):
    """projector.py:190-215 for one item: h [T, C]."""
    T, C = h.shape
    pad = (block - (T % block)) % block
    if pad:
        h = np.concatenate([h, np.zeros((pad, C))], 0)
    nblocks = (T + pad) // block
    h = h.reshape(nblocks, block, C)
    mean_pool = h.reshape(nblocks, block // rate, rate, C).mean(-2)
    return query[None] + mean_pool, h + positions[None]


@pytest.mark.parametrize("block,rate", [(15, 5), (4, 2)])
def test_windows_statement_is_the_reference_assembly(block, rate):
    rng = np.random.default_rng(block)
    for T in (1, block - 1, block, block + 1, 3 * block + 2):
        h = rng.standard_normal((3, T, 12))
        query, pos = rng.standard_normal((block // rate, 12)), rng.standard_normal((block, 12))
        lens = [T, max(T - 1, 1), 1]
        vq, vk, bq, bk = E.qformer_windows(h, query, pos, block, rate, lens)
        nb = -(-T // block)
        assert vq.shape == (3 * nb, block // rate, 12) and vk.shape == (3 * nb, block, 12) and (bq >= 0).all() and (bk >= 0).all()
        for b, n in enumerate(lens):
            rq, rk = _reference_windows(h[b, :n], query, pos, block, rate)
            na = rq.shape[0]
            assert np.abs(vq[b * nb:b * nb + na] - rq).max() < 1e-14 and np.abs(vk[b * nb:b * nb + na] - rk).max() < 1e-14
            assert np.array_equal(vk[b * nb + na:(b + 1) * nb], np.broadcast_to(pos, (nb - na, block, 12)))


def test_stand_ins_write_what_the_statements_say():
    import torch

    from mlx_audio_amd import ops

    q, k, v, table = (torch.from_numpy(t) for t in E.shaw_inputs(64, 2, 8, 13, 7, B=2))
    lens = torch.tensor([13, 5], dtype=torch.int32)
    with E.patched():
        out = ops.shaw_block_attention(q, k, v, table, torch.full((2, 13, 128), float("nan")), heads=2, dh=64, ctx=8, max_pos=7, lens=lens)
        probs, pb = ops.selfcond_rows(torch.randn(5, 9))
        pooled = ops.posterior_pool(torch.randn(2, 13, 6), torch.rand(2, 13), 4, lens=lens)
        qs, kv = ops.qformer_windows(torch.randn(2, 13, 6), torch.zeros(2, 6), torch.zeros(4, 6), block=4, rate=2, lens=lens)
    val, _ = E.shaw_block_attention(q.numpy(), k.numpy(), v.numpy(), table.numpy(), heads=2, dh=64, ctx=8, max_pos=7, lens=[13, 5])
    assert np.abs(out.double().numpy() - val).max() < 1e-6 and not out[1, 5:].any()
    assert probs.shape == (5, 9) and torch.equal(pb, probs[:, 0]) and pooled.shape == (2, 4, 6) and qs.shape == (8, 2, 6) and kv.shape == (8, 4, 6)
    assert ops.shaw_block_attention is not E._t_shaw_block_attention          # restored
