"""Float64 statements of the four kernels of ``csrc/granite_nar.hip`` (``shaw_block_attention``, ``selfcond_rows``, ``posterior_pool``,
``qformer_windows``), each with the per-element float32 rounding bound of the kernel's own operation order, and the same contracts as CPU stand-ins
for ``mlx_audio_amd.ops`` (torch in, torch out).  U is the float32 unit round-off; every bound carries a factor 1.05 for the second-order terms."""
import math

import numpy as np

U = 2.0 ** -24


def _lens(lens, B, T):
    return [T] * B if lens is None else [min(max(int(n), 0), T) for n in lens]


# ------------------------------------------------------------------ shaw_block_attention
def shaw_block_attention(q, k, v, table, *, heads, dh, ctx, max_pos, scale=None, lens=None, mask_padded=False):
    """q / k / v [B, T, >= heads dh], table [2 max_pos + 1, dh] -> (out [B, T, heads dh], bound).

    For query i < L of block m the keys are ALL ctx frames of the block; a frame at or beyond L is a zero key with a zero value and stays visible
    (``mask_padded=True`` is the MUTANT that drops those keys instead: the rule ``relpos_attention`` would apply).

    The bound.  The kernel scales q by fl(fl(scale) fl(log2 e)) once (a rounding each for the scale, the constant, their product and the scaled q:
    4 U), forms q . k and q . table as two MFMA chains of
    dh terms each and adds them: es = (dh + 4) U scale (|q| . |k| + |q| . |t|) + U |s|.  exp2(s - m) carries es + em (the maximum's own error, at
    most max es) + U |s - m| in its argument and 2 U of its own; the online softmax multiplies by exp2(m_old - m_new) once per stage of 32 keys
    (3 U each, and U times the distance the maximum travelled, at most the row's range).  The row sum adds 16 terms per stage and lane and the
    stages: (16 + nst + 1) U; 1 / sum and the final product one each.  out is an MFMA chain over the ctx keys, rescaled once per stage:
    (ctx + nst + 2) U sum |p v|."""
    q, k, v, table = (np.asarray(t, dtype=np.float64) for t in (q, k, v, table))
    B, T = q.shape[:2]
    assert dh in (64, 128) and ctx >= 1 and max_pos >= ctx - 1 and table.shape[0] == 2 * max_pos + 1, "mi355_shaw_block_attention refuses this call"
    sc = float(dh ** -0.5 if scale is None else scale)
    hd = heads * dh
    out, bound = np.zeros((B, T, hd)), np.zeros((B, T, hd))
    nst = -(-ctx // 32)
    jl = np.arange(ctx)
    for b, L in enumerate(_lens(lens, B, T)):
        for m0 in range(0, L, ctx):
            n_q = min(ctx, L - m0)                       # real queries of the block
            n_k = min(ctx, L - m0)                       # real keys; the rest of the block is zero keys
            for h in range(heads):
                sl = slice(h * dh, (h + 1) * dh)
                qq = q[b, m0:m0 + n_q, sl]
                kk, vv = np.zeros((ctx, dh)), np.zeros((ctx, dh))
                kk[:n_k], vv[:n_k] = k[b, m0:m0 + n_k, sl], v[b, m0:m0 + n_k, sl]
                idx = max_pos + np.arange(n_q)[:, None] - jl[None, :]                       # table row of pair (i, j)
                pos = np.take_along_axis(qq @ table[:, :dh].T, idx, axis=1)
                apos = np.take_along_axis(np.abs(qq) @ np.abs(table[:, :dh]).T, idx, axis=1)
                s = (qq @ kk.T + pos) * sc
                es = (dh + 4) * U * sc * (np.abs(qq) @ np.abs(kk).T + apos) + U * np.abs(s)
                if mask_padded:
                    s[:, n_k:] = -np.inf
                mx = s.max(-1, keepdims=True)
                e = np.exp(s - mx)
                p = e / e.sum(-1, keepdims=True)
                fin = np.isfinite(s)
                d = np.where(fin, mx - s, 0.0)
                rel = es + es.max(-1, keepdims=True) + U * (d + 2) + nst * 3 * U + U * d.max(-1, keepdims=True)
                rel_p = rel + (rel * p).sum(-1, keepdims=True) + U * (16 + 2 * nst + 3)
                out[b, m0:m0 + n_q, sl] = p @ vv
                bound[b, m0:m0 + n_q, sl] = ((p * rel_p) @ np.abs(vv) + (ctx + nst + 2) * U * (p @ np.abs(vv))) * 1.05
    return out, bound


SHAW_CTX = (8, 33, 128, 129, 200)


def shaw_lengths(ctx):
    """The sequence lengths of the kernel test for one context size."""
    return (1, ctx - 1, ctx, ctx + 1, 2 * ctx + 37)


def shaw_ragged(ctx, T):
    """The ragged batch of the kernel test: lengths 1, ctx, ctx + 1 and T (cut to T)."""
    return [min(n, T) for n in (1, ctx, ctx + 1, T)]


def shaw_inputs(dh, heads, ctx, T, max_pos, B=4):
    """The float32 inputs of the kernel test (shared with the CPU mutant check): unit-variance q / k / v and a table of standard deviation 0.5."""
    rng = np.random.default_rng(((dh * 7 + heads) * 1009 + ctx) * 1013 + T * 3 + (max_pos == ctx - 1))
    hd = heads * dh
    q, k, v = (rng.standard_normal((B, T, hd)).astype(np.float32) for _ in range(3))
    table = (0.5 * rng.standard_normal((2 * max_pos + 1, dh))).astype(np.float32)
    return q, k, v, table


# ------------------------------------------------------------------ selfcond_rows
def selfcond_rows(logits, wave_max_v=256):
    """logits [rows, V] -> (probs, p_blank, bound of probs).  exp(x - m): U |x - m| in the argument and 2 U of expf; the sum holds ceil(V / NT) terms
    per thread (NT = 64 up to ``wave_max_v`` columns, 256 above), 6 butterfly levels and 2 joins; the division one more."""
    x = np.asarray(logits, dtype=np.float64)
    V = x.shape[1]
    nt = 64 if V <= wave_max_v else 256
    m = x.max(-1, keepdims=True)
    e = np.exp(x - m)
    p = e / e.sum(-1, keepdims=True)
    rel = U * (np.abs(x - m) + 2)
    rel_p = rel + (rel * p).sum(-1, keepdims=True) + U * (math.ceil(V / nt) + 6 + 2 + 1)
    return p, p[:, 0].copy(), p * rel_p * 1.05


# ------------------------------------------------------------------ posterior_pool
def posterior_pool(h, p_blank, window, lens=None):
    """h [B, T, C], p_blank [B, T] -> (out [B, ceil(T / window), C], bound).  A weight is (1 - pb) / max(sum, 1e-6): U for the difference, window U for
    the sum, U for the rounded constant and U for the division; the pooled value is an fmaf chain over the window's real frames."""
    h, pb = np.asarray(h, dtype=np.float64), np.asarray(p_blank, dtype=np.float64)
    B, T, C = h.shape
    nw = -(-T // window)
    out, bound = np.zeros((B, nw, C)), np.zeros((B, nw, C))
    for b, L in enumerate(_lens(lens, B, T)):
        for n in range(nw):
            t0, t1 = n * window, min((n + 1) * window, L)
            if t1 <= t0:
                continue
            imp = 1.0 - pb[b, t0:t1]
            w = imp / max(imp.sum(), 1e-6)
            out[b, n] = w @ h[b, t0:t1]
            bound[b, n] = (window + 3 + (t1 - t0)) * U * (np.abs(w) @ np.abs(h[b, t0:t1])) * 1.05
    return out, bound


# ------------------------------------------------------------------ qformer_windows
def qformer_windows(h, query, positions, block, rate, lens=None):
    """h [B, T, C] -> (queries [B nblocks, block / rate, C], kv [B nblocks, block, C], bound_q, bound_kv).  kv is one addition; a query is a sum of
    ``rate`` terms, a division and an addition."""
    h, query, positions = (np.asarray(t, dtype=np.float64) for t in (h, query, positions))
    B, T, C = h.shape
    assert block >= 1 and rate >= 1 and block % rate == 0, "mi355_qformer_windows refuses this call"
    nb, nq = -(-T // block), block // rate
    win = np.zeros((B, nb * block, C))
    for b, L in enumerate(_lens(lens, B, T)):
        win[b, :L] = h[b, :L]
    win = win.reshape(B * nb, block, C)
    kv = win + positions[None]
    grp = win.reshape(B * nb, nq, rate, C)
    queries = query[None] + grp.mean(2)
    bq = U * (np.abs(queries) + (rate + 1) * np.abs(grp).sum(2) / rate) * 1.05
    return queries, kv, bq, U * np.abs(kv) * 1.05


# ------------------------------------------------------------------ the same contracts as stand-ins for ``mlx_audio_amd.ops`` (torch in, torch out)
def _t_shaw_block_attention(q, k, v, table, out, *, heads, dh, ctx, max_pos, scale=None, lens=None, check_lens=True):
    import torch

    val, _ = shaw_block_attention(q.double().numpy(), k.double().numpy(), v.double().numpy(), table.double().numpy(), heads=heads, dh=dh, ctx=ctx,
                                  max_pos=max_pos, scale=scale, lens=None if lens is None else lens.tolist())
    out[..., :heads * dh] = torch.from_numpy(val).to(out.dtype)
    return out


def _t_selfcond_rows(logits, *, probs=None, p_blank=None):
    import torch

    p, pb, _ = selfcond_rows(logits.double().numpy())
    p, pb = torch.from_numpy(p).float(), torch.from_numpy(pb).float()
    if probs is not None:
        probs.copy_(p)
    if p_blank is not None:
        p_blank.copy_(pb)
    return (p if probs is None else probs), (pb if p_blank is None else p_blank)


def _t_posterior_pool(h, p_blank, window, *, lens=None, out=None):
    import torch

    val, _ = posterior_pool(h.double().numpy(), p_blank.double().numpy(), window, None if lens is None else lens.tolist())
    val = torch.from_numpy(val).float()
    if out is None:
        return val
    out.copy_(val)
    return out


def _t_qformer_windows(h, query, positions, *, block, rate, lens=None, queries=None, kv=None):
    import torch

    qv, kvv, _, _ = qformer_windows(h.double().numpy(), query.double().numpy(), positions.double().numpy(), block, rate,
                                    None if lens is None else lens.tolist())
    qv, kvv = torch.from_numpy(qv).float(), torch.from_numpy(kvv).float()
    if queries is not None:
        queries.copy_(qv)
    if kv is not None:
        kv.copy_(kvv)
    return (qv if queries is None else queries), (kvv if kv is None else kv)


# What the Granite Speech NAR host schedule uses beyond these four comes from the existing emulation modules, imported unchanged and only when
# ``patched_model`` is entered: conv_gemm and the packers (``_ops_emu``), layernorm and head_norm_rope (``_ops_emu_s3``), glu_dwconv_silu
# (``_ops_emu_parakeet``), ctc_rows / ctc_collapse (``_ops_emu_sensevoice``), swiglu (``_ops_emu_moonshine``).  ``rmsnorm``, ``flash_attention`` with
# grouped kv heads and per-item lengths, and the fused log-mel front end in its Whisper mode are stated here as this model uses them.
def _t_rmsnorm(x, y, weight, eps=1e-6, lens=None):
    assert lens is None, "not emulated"
    d = x.double()
    v = d / (d.pow(2).mean(-1, keepdim=True) + eps).sqrt()
    y.copy_((v if weight is None else v * weight.double()).to(y.dtype))
    return y


def _t_flash_attention(q, k, v, out, *, heads, kv_heads=None, dh, scale=None, lens_q=None, lens_k=None, **kw):
    import torch

    assert not kw, kw
    kvh = heads if kv_heads is None else kv_heads
    B, Tq, Tk = q.shape[0], q.shape[1], k.shape[1]
    scale = dh ** -0.5 if scale is None else scale
    for b in range(B):
        nq = Tq if lens_q is None else min(max(int(lens_q[b]), 0), Tq)
        nk = Tk if lens_k is None else min(max(int(lens_k[b]), 0), Tk)
        q4 = q[b, :nq, :heads * dh].double().reshape(nq, heads, dh).transpose(0, 1)
        k4, v4 = (t[b, :nk, :kvh * dh].double().reshape(nk, kvh, dh).transpose(0, 1).repeat_interleave(heads // kvh, dim=0) for t in (k, v))
        p = torch.softmax(q4 @ k4.transpose(1, 2) * scale, -1)
        out[b, :nq, :heads * dh] = (p @ v4).transpose(0, 1).reshape(nq, heads * dh).to(out.dtype)
        out[b, nq:, :heads * dh] = 0
    return out


def _t_logmel(x, n_fft, hop, window, pad_mode, n_frames, fb, mode, log_guard=0.0, fixed_max=None):
    """``mi355_logmel`` in mode 0 with reflect padding: |STFT|^2 -> mel -> log10(max(., 1e-10)) on ``n_frames`` frames, clamped at the item's own
    maximum - 8, (y + 4) / 4."""
    import torch

    assert mode == 0 and pad_mode == 1 and fixed_max is None
    out = []
    for row in x.double().numpy():
        xp = np.pad(row, n_fft // 2, mode="reflect")
        frames = np.stack([xp[i * hop:i * hop + n_fft] for i in range(n_frames)]) * window.double().numpy()
        mel = (np.abs(np.fft.rfft(frames, axis=-1)) ** 2) @ fb.double().numpy().T
        y = np.log10(np.maximum(mel, 1e-10))
        out.append((np.maximum(y, y.max() - 8.0) + 4.0) / 4.0)
    return torch.from_numpy(np.stack(out)).float()


def patched_model():
    """Context manager: every ``ops`` entry point the Granite Speech NAR host schedule calls, as float64 CPU statements (``device="cpu"``)."""
    import contextlib

    import _ops_emu_moonshine
    import _ops_emu_s3
    import _ops_emu_sensevoice
    from mlx_audio_amd import ops

    @contextlib.contextmanager
    def cm():
        names = dict(rmsnorm=_t_rmsnorm, flash_attention=_t_flash_attention, logmel=_t_logmel, swiglu=_ops_emu_moonshine.swiglu,
                     head_norm_rope=_ops_emu_s3.head_norm_rope, layernorm=_ops_emu_s3.layernorm)
        saved = {k: getattr(ops, k) for k in names}
        with _ops_emu_sensevoice.patched(), patched():
            try:
                for k, v in names.items():
                    setattr(ops, k, v)
                yield
            finally:
                for k, v in saved.items():
                    setattr(ops, k, v)

    return cm()


def patched():
    """Context manager: ``mlx_audio_amd.ops`` with the four entry points above replaced by their float64 statements."""
    import contextlib

    from mlx_audio_amd import ops

    @contextlib.contextmanager
    def cm():
        names = dict(shaw_block_attention=_t_shaw_block_attention, selfcond_rows=_t_selfcond_rows, posterior_pool=_t_posterior_pool,
                     qformer_windows=_t_qformer_windows)
        saved = {k: getattr(ops, k) for k in names}
        try:
            for k, v in names.items():
                setattr(ops, k, v)
            yield
        finally:
            for k, v in saved.items():
                setattr(ops, k, v)

    return cm()
