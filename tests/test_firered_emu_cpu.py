"""Two kinds of test, no GPU.  The first and the last check the change itself: the header's declarations, the constants of ``ops`` and the buffer
parity of ``ops.BeamState``.  The five in between check the TEST SIDE: the float64 statements of ``_ops_emu_fireredasr2.py``, which
``test_firered_kernels_gpu.py`` holds the kernels to, against plain restatements of the reference's lines (torch's conv2d / conv1d / layer_norm in
float64, the whole ``beam_search`` loop of fireredasr2.py:385-446 step by step, attention over gathered caches) -- so that a mistake in a statement
cannot pass as the kernel's contract.  They say nothing about the kernels on their own."""
import os
import re
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import _ops_emu_fireredasr2 as E  # noqa: E402


def test_entry_points_declared_and_constants_match_the_header():
    from mlx_audio_amd import _lib, ops

    names = _lib.declared_functions()
    for fn in ("mi355_subsample2d_k3s2", "mi355_glu_dwconv_ln_swish", "mi355_beam_step", "mi355_beam_attention"):
        assert fn in names
    header = open(_lib.HEADER).read()
    for macro, value in (("MI355_SUBSAMPLE2D_MAX_COUT", ops.SUBSAMPLE2D_MAX_COUT), ("MI355_GLU_DWCONV_LN_MAX_TAPS", ops.GLU_DWCONV_LN_MAX_TAPS),
                         ("MI355_GLU_DWCONV_LN_MAX_C", ops.GLU_DWCONV_LN_MAX_C), ("MI355_GLU_DWCONV_LN_ROWS", ops.GLU_DWCONV_LN_ROWS),
                         ("MI355_BEAM_MAX", ops.BEAM_MAX), ("MI355_BEAM_MAX_V", ops.BEAM_MAX_V), ("MI355_BEAM_ATTN_MAX_TK", ops.BEAM_ATTN_MAX_TK)):
        assert int(re.search(rf"#define {macro} (\d+)", header).group(1)) == value, macro
    assert ops.subsample2d_out(7) == 3 and ops.subsample2d_out(3) == 1 and ops.subsample2d_out(80) == 39


def test_subsample2d_statement_is_the_reference_subsampler():
    """Conv2dSubsampling.__call__ (fireredasr2.py:27-37): two valid 3 x 3 / stride 2 convs with ReLU, then (N, T, D, C) -> (N, T, C * D)."""
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 23, 17, generator=g, dtype=torch.float64)
    w1, b1 = torch.randn(8, 3, 3, 1, generator=g, dtype=torch.float64), torch.randn(8, generator=g, dtype=torch.float64)
    w2, b2 = torch.randn(8, 3, 3, 8, generator=g, dtype=torch.float64), torch.randn(8, generator=g, dtype=torch.float64)
    conv = lambda t, w, b: torch.relu(torch.nn.functional.conv2d(t, w.permute(0, 3, 1, 2), b, stride=2))
    ref = conv(conv(x[:, None], w1, b1), w2, b2)                      # NCHW: [N, C, T, D]
    ref = ref.permute(0, 2, 1, 3).reshape(2, ref.shape[2], -1)       # [N, T, C * D]
    y1, _ = E.subsample2d(x.numpy(), w1.numpy(), b1.numpy())
    y2, bound = E.subsample2d(y1, w2.numpy(), b2.numpy(), out_cf=True)
    assert y2.shape == (2, 5, 8, 3) and np.abs(y2.reshape(2, 5, -1) - ref.numpy()).max() < 1e-12 and (bound >= 0).all()
    # rows at and beyond lens_in read as zero == the reference's explicit zero frames; rows at and beyond lens_out are zero
    xz = x.clone()
    xz[0, 17:] = 0.0
    a, _ = E.subsample2d(x.numpy(), w1.numpy(), b1.numpy(), lens_in=[17, 23], lens_out=[11, 4])
    b, _ = E.subsample2d(xz.numpy(), w1.numpy(), b1.numpy())
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1, :4], b[1, :4]) and not a[1, 4:].any()


def test_glu_dwconv_ln_swish_statement_is_the_reference_module():
    """ConformerConvolution.__call__ between the pointwise convs (fireredasr2.py:111-116)."""
    g = torch.Generator().manual_seed(1)
    C, K, L = 24, 7, 19
    x = torch.randn(2, L, 2 * C, generator=g, dtype=torch.float64)
    w = torch.randn(C, K, generator=g, dtype=torch.float64)
    lw, lb = torch.randn(C, generator=g, dtype=torch.float64), torch.randn(C, generator=g, dtype=torch.float64)
    a, b = x[..., :C], x[..., C:]
    out = (a * torch.sigmoid(b)).transpose(1, 2)
    out = torch.nn.functional.conv1d(out, w[:, None, :], padding=(K - 1) // 2, groups=C).transpose(1, 2)
    out = torch.nn.functional.layer_norm(out, (C,), lw, lb, 1e-5)
    ref = out * torch.sigmoid(out)
    y, bound = E.glu_dwconv_ln_swish(x.numpy(), w.numpy(), lw.numpy(), lb.numpy(), 1e-5)
    assert np.abs(y - ref.numpy()).max() < 1e-12 and (bound > 0).all() and bound.max() < 1e-3
    # an item of a ragged batch is that item alone; its padded rows are zero
    yr, _ = E.glu_dwconv_ln_swish(x.numpy(), w.numpy(), lw.numpy(), lb.numpy(), 1e-5, lens=[L, 5])
    ya, _ = E.glu_dwconv_ln_swish(x.numpy()[1:, :5], w.numpy(), lw.numpy(), lb.numpy(), 1e-5)
    assert np.array_equal(yr[1, :5], ya[0]) and not yr[1, 5:].any() and np.array_equal(yr[0], y[0])


def _reference_beam_search(logits_per_step, B, eos_id, smoothing, eos_penalty):
    """TransformerDecoder.beam_search's bookkeeping (fireredasr2.py:385-446) in numpy float64 on given logits [steps, B, V]; argsort stands in for
    the reference's _topk (the inputs are tie-free)."""
    INF = 1e10
    ys = np.full((B, 1), 1, dtype=np.int64)
    scores = np.array([0.0] + [-INF] * (B - 1)).reshape(B, 1)
    fin = np.zeros((B, 1))
    conf = np.zeros((B, 1))
    trace = []
    for logits in logits_per_step:
        z = logits / smoothing
        p = np.exp(z - z.max(-1, keepdims=True))
        t = np.log(p / p.sum(-1, keepdims=True) + 1e-10)
        if eos_penalty != 1.0:
            t[:, eos_id] *= eos_penalty
        idx = np.argsort(-t, axis=-1)[:, :B]
        top = np.take_along_axis(t, idx, -1)
        mask = np.repeat(np.array([0.0] + [-INF] * (B - 1)).reshape(1, B), B, 0)
        top = top * (1 - fin) + mask * fin
        idx = idx * (1 - fin.astype(np.int64)) + eos_id * fin.astype(np.int64)
        allsc = (scores + top).reshape(B * B)
        best = np.argsort(-allsc, kind="stable")[:B]
        scores = allsc[best].reshape(B, 1)
        bi = best // B
        new = idx.reshape(B * B)[best].reshape(B, 1)
        ys = np.concatenate([ys[bi], new], 1)
        conf = np.concatenate([conf[bi], np.exp(top.reshape(B * B)[best]).reshape(B, 1)], 1)
        fin = (new == eos_id).astype(np.float64)
        trace.append((bi.copy(), new[:, 0].copy(), scores[:, 0].copy()))
        if fin.sum() == B:
            break
    return ys, conf, trace


def test_beam_step_statement_is_the_reference_loop():
    for B, pen, seed in ((3, 1.0, 0), (3, 1.5, 1), (1, 1.0, 2), (5, 1.0, 3), (8, 1.5, 4)):
        rng = np.random.default_rng(seed)
        V, steps, eos, Tmax = 30, 9, 4, 12
        logits = (rng.standard_normal((steps, B, V)) * 3).astype(np.float32)
        logits[5:, :, eos] += 12.0                                         # the beams end after a few tokens
        ys, conf, trace = _reference_beam_search(logits.astype(np.float64), B, eos, float(np.float32(1.25)), pen)
        st = dict(scores=np.array([[0.0] + [-1e10] * (B - 1)]), finished=np.zeros((1, B), np.int32), step=np.ones(1, np.int32),
                  max_steps=np.array([Tmax], np.int32), done=np.zeros(1, np.int32), tokens=np.full((1, B, Tmax), 1, np.int32),
                  ind=np.zeros((1, B, Tmax), np.int32), conf=np.zeros((1, B, Tmax)))
        st["ind"][0, :, 0] = np.arange(B)
        n = 0
        while not st["done"][0]:
            o = E.beam_step(logits[n], eos_id=eos, smoothing=1.25, eos_penalty=pen, **st)
            assert o["margin"][0] > 100.0
            bi, new, sc = trace[n]
            assert np.array_equal(o["beam_idx"][0], bi) and np.array_equal(o["new_tokens"][0], new)
            live = sc > -1e9
            assert np.allclose(o["scores"][0][live], sc[live], rtol=0, atol=1e-9) and np.allclose(o["scores"][0], sc, rtol=1e-6)
            s = int(st["step"][0])
            assert (o["ind"][0, :, s] == np.arange(B)).all() and np.array_equal(o["ind"][0, :, :s], st["ind"][0][bi][:, :s])
            for key in ("tokens", "ind", "conf"):      # the untouched tail of the other buffer is not part of the state
                o[key][0, :, s + 1:] = st[key][0, :, s + 1:]
            st = {k: o.get(k, st[k]) for k in st}
            n += 1
        assert n == len(trace) and int(st["step"][0]) == ys.shape[1]
        assert np.array_equal(st["tokens"][0, :, :ys.shape[1]], ys) and np.allclose(st["conf"][0, :, :ys.shape[1]], conf, atol=1e-12)


def test_beam_step_statement_freezes_and_stops():
    B, V, Tmax = 2, 9, 5
    rng = np.random.default_rng(0)
    logits = rng.standard_normal((2 * B, V)).astype(np.float32) * 4
    st = dict(scores=np.array([[-0.5, -1.0], [-0.2, -0.9]]), finished=np.zeros((2, B), np.int32), step=np.array([3, 2], np.int32),
              max_steps=np.array([4, 5], np.int32), done=np.array([0, 1], np.int32), tokens=np.ones((2, B, Tmax), np.int32),
              ind=np.zeros((2, B, Tmax), np.int32), conf=np.zeros((2, B, Tmax)))
    o = E.beam_step(logits, eos_id=0, smoothing=1.25, eos_penalty=1.0, **st)
    assert o["done"].tolist() == [1, 1] and o["step"].tolist() == [4, 2]              # step + 1 == max_steps; the frozen item keeps its step
    assert (o["tokens"][1] == -7).all() and np.isnan(o["conf"][1]).all() and np.array_equal(o["scores"][1], st["scores"][1])


def test_beam_attention_statement_is_attention_over_gathered_caches():
    rng = np.random.default_rng(3)
    N, B, T, H, dh = 2, 3, 7, 2, 8
    scale = float(np.float32(dh ** -0.5))          # the kernel's scale is a float32
    q, k, v = rng.standard_normal((N * B, H * dh)), rng.standard_normal((N * B, T, H * dh)), rng.standard_normal((N * B, T, H * dh))
    ind = rng.integers(0, B, (N, B, T)).astype(np.int32)
    out, bound = E.beam_attention(q, k, v, ind, [T - 1, 3], beams=B, heads=H, dh=dh, scale=scale)
    for nb in range(N * B):
        n, j = divmod(nb, B)
        nk = [T, 4][n]
        kk = np.stack([k[n * B + ind[n, j, s], s] for s in range(nk)]).reshape(nk, H, dh)
        vv = np.stack([v[n * B + ind[n, j, s], s] for s in range(nk)]).reshape(nk, H, dh)
        att = np.einsum("hd,shd->hs", q[nb].reshape(H, dh), kk) * scale          # scale, softmax, then @ v (fireredasr2.py:272-278)
        att = np.exp(att - att.max(-1, keepdims=True))
        att /= att.sum(-1, keepdims=True)
        assert np.abs(np.einsum("hs,shd->hd", att, vv).reshape(-1) - out[nb]).max() < 1e-12
    assert (bound > 0).all() and bound.max() < 1e-4
    z, _ = E.beam_attention(q, k, v, ind, [-1, 0], beams=B, heads=H, dh=dh, scale=1.0)
    assert not z[:B].any() and np.allclose(z[B], v[B + ind[1, 0, 0], 0])


def test_beam_state_final_picks_the_buffer_of_the_last_live_step():
    from mlx_audio_amd import ops

    st = ops.beam_state(3, 2, 6, [6, 6, 6], sos_id=1, device="cpu")
    assert st.scores.tolist() == [[0.0, -1e10]] * 3 and st.step.tolist() == [1, 1, 1] and st.ind[0][:, :, 0].tolist() == [[0, 1]] * 3
    # item 0 never stepped, item 1 stopped after one call (its history is in buffer 1), item 2 after two calls (buffer 0)
    st.tokens[0][1], st.tokens[1][1], st.tokens[0][2], st.tokens[1][2] = 10, 11, 20, 21
    st.step.copy_(torch.tensor([1, 2, 3], dtype=torch.int32))
    tok, _, _ = st.final()
    assert tok[0, 0, 0] == 1 and (tok[1] == 11).all() and (tok[2] == 20).all()
