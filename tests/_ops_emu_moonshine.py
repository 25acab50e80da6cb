"""TEST INFRASTRUCTURE: float64 CPU emulations of the CONTRACTS of ``mid_attention``, ``partial_rope`` (``include/mi355audio.h``) and ``swiglu``; the
``gemv`` as the decoder uses it, ``conv_gemm``'s ``stats=`` epilogue and ``group_norm_coef`` on conv partials; the
rest of what the Moonshine host schedule uses comes from ``tests/_ops_emu_gn.py`` (conv_gemm, the GroupNorm entry points), ``_ops_emu_sortformer.py``
(layernorm) and ``_ops_emu_sensevoice.py`` (ctc_rows), imported unchanged.  Not a fallback: nothing under ``mlx_audio_amd/`` imports it."""
import contextlib

import torch

import _ops_emu
import _ops_emu_gn
import _ops_emu_sensevoice
import _ops_emu_sortformer
from mlx_audio_amd import _lib, ops


def mid_attention(q, k, v, out, *, heads, dh, kv_heads=None, scale=None, causal=False, lens_q=None, lens_k=None, check_lens=True):
    B, Tq, Tk = q.shape[0], q.shape[1], k.shape[1]
    KH = heads if kv_heads is None else kv_heads
    if dh not in ops.MID_ATTENTION_WIDTHS:
        raise _lib.Mi355Error(f"mid_attention: dh must be 36, 40, 44, 48, 52, 56 or 60 (got dh = {dh})")
    assert heads % KH == 0 and all(t.stride(1) % 4 == 0 and t.storage_offset() % 4 == 0 for t in (q, k, v, out)), "mi355_mid_attention refuses this call"
    if lens_k is not None and check_lens and (int(lens_k.min()) < 1 or int(lens_k.max()) > Tk):
        raise _lib.Mi355Error("mid_attention: lens_k must lie in [1, Tk]")
    scale = dh ** -0.5 if scale is None else scale
    for b in range(B):
        nq = Tq if lens_q is None else min(max(int(lens_q[b]), 0), Tq)
        nk = Tk if lens_k is None else min(max(int(lens_k[b]), 0), Tk)
        out[b, :, :heads * dh] = 0
        if nq == 0 or nk == 0:
            continue
        q4 = q[b, :nq, :heads * dh].double().reshape(nq, heads, dh).transpose(0, 1)
        k4, v4 = (t[b, :nk, :KH * dh].double().reshape(nk, KH, dh).transpose(0, 1).repeat_interleave(heads // KH, 0) for t in (k, v))
        s = q4 @ k4.transpose(1, 2) * scale
        vis = torch.ones((nq, nk), dtype=torch.bool)
        if causal:
            vis = torch.arange(nk)[None, :] <= torch.arange(nq)[:, None] + (nk - nq)
        p = torch.softmax(s.masked_fill(~vis, -float("inf")), -1)
        p = torch.where(vis.any(1)[None, :, None], p, torch.zeros((), dtype=torch.float64))   # a query with no visible key: a zero row
        out[b, :nq, :heads * dh] = (p @ v4).transpose(0, 1).reshape(nq, heads * dh).to(out.dtype)
    return out


def partial_rope(x, y, *, heads, dh, rot, cos, sin, pos0=0, lens=None, second=None):
    B, L = x.shape[0], x.shape[1]
    if pos0 < 0 or pos0 + L > cos.shape[0]:
        raise _lib.Mi355Error(f"partial_rope: positions {pos0}..{pos0 + L - 1} run past the {cos.shape[0]}-row rotary tables")
    assert rot % 2 == 0 and 2 <= rot <= dh and dh % 4 == 0 and cos.shape[1] == rot // 2
    c = cos[pos0:pos0 + L].double().repeat_interleave(2, dim=1)[:, None, :]
    s = sin[pos0:pos0 + L].double().repeat_interleave(2, dim=1)[:, None, :]
    for src, dst, H in [(x, y, heads)] + ([] if second is None else [second]):
        for b in range(B):
            n = L if lens is None else min(max(int(lens[b]), 0), L)
            v = src[b, :n, :H * dh].double().reshape(n, H, dh)
            xr = v[..., :rot]
            rh = torch.stack([-xr[..., 1::2], xr[..., 0::2]], dim=-1).reshape(xr.shape)
            dst[b, :n, :H * dh] = torch.cat([xr * c[:n] + rh * s[:n], v[..., rot:]], dim=-1).reshape(n, H * dh).to(dst.dtype)
    return y


def swiglu(x, y):
    assert x.shape[-1] == 2 * y.shape[-1]
    y.copy_((torch.nn.functional.silu(x[..., 0::2].double()) * x[..., 1::2].double()).to(y.dtype))
    return y


def gemv(x, rw, y, *, post_act=0, post_slope=0.0, res=None, **kw):
    """mi355_gemv for what the Moonshine decoder asks of it: y[m, :] = act(x[m, :] W^T + b) (+ res[m, :]) for 1 .. 8 rows."""
    assert not kw and x.dim() == 2 and y.dim() == 2 and 1 <= x.shape[0] <= 8 and x.shape[1] == rw.k and rw.k % 8 == 0 and y.shape == (x.shape[0], rw.n)
    v = x.double() @ rw.w.double().T
    if rw.bias is not None:
        v = v + rw.bias.double()
    v = _ops_emu._act(v, post_act, post_slope)
    if res is not None:
        v = v + res.double()
    y.copy_(v.to(y.dtype))
    return y


def conv_gemm(x, pc, y, *, stats=None, lens_out=None, lout=None, **kw):
    """``tests/_ops_emu.conv_gemm`` plus the ``stats=`` epilogue: per block of 64 stored output rows and per channel (sum, sum of squared deviations
    from the block's mean) over the rows below ``lens_out[b]``, float32."""
    _ops_emu.conv_gemm(x, pc, y, lens_out=lens_out, lout=lout, **kw)
    if stats is not None:
        B, Lout = y.shape[0], (lout if lout is not None else y.shape[1])
        assert stats.shape[0] == B and stats.shape[1] >= (Lout + 63) // 64 and stats.shape[2] == pc.cout and stats.dtype == torch.float32
        for b in range(B):
            n = Lout if lens_out is None else min(max(int(lens_out[b]), 0), Lout)
            for blk in range((n + 63) // 64):
                v = y[b, blk * 64:min(blk * 64 + 64, n), :pc.cout].double()
                stats[b, blk, :, 0], stats[b, blk, :, 1] = v.sum(0).float(), ((v - v.mean(0)) ** 2).sum(0).float()
    return y


def group_norm_coef(partials, L, C, weight, bias, *, eps=1e-5, lens=None, rep=1, return_stats=False):
    """``tests/_ops_emu_gn.group_norm_coef`` plus the conv-partials form: [B, blocks, C, 2] merged over blocks and channels (Chan's formula)."""
    if partials.dim() == 3:
        return _ops_emu_gn.group_norm_coef(partials, L, C, weight, bias, eps=eps, lens=lens, rep=rep, return_stats=return_stats)
    assert partials.dim() == 4 and partials.shape[2] == C and partials.shape[3] == 2 and not return_stats
    B = partials.shape[0]
    ld = ops.round_up(rep * C, 32)
    scale, shift = torch.zeros((B, ld)), torch.zeros((B, ld))
    for b in range(B):
        n = L if lens is None else min(max(int(lens[b]), 0), L)
        nb = (n + 63) // 64
        cnt = torch.tensor([min(64, n - k * 64) for k in range(nb)], dtype=torch.float64)[:, None]
        s, q = partials[b, :nb, :, 0].double(), partials[b, :nb, :, 1].double()
        mean = s.sum() / (n * C)
        var = (q + cnt * (s / cnt - mean) ** 2).sum() / (n * C)
        rstd = 1.0 / torch.sqrt(var + eps)
        sc = (torch.ones(C, dtype=torch.float64) if weight is None else weight.double()) * rstd
        sh = (torch.zeros(C, dtype=torch.float64) if bias is None else bias.double()) - mean * sc
        scale[b, :rep * C], shift[b, :rep * C] = sc.repeat(rep).float(), sh.repeat(rep).float()
    return scale, shift


@contextlib.contextmanager
def patched():
    names = dict(mid_attention=mid_attention, partial_rope=partial_rope, swiglu=swiglu, layernorm=_ops_emu_sortformer.layernorm,
                 ctc_rows=_ops_emu_sensevoice.ctc_rows, gemv=gemv, conv_gemm=conv_gemm, group_norm_coef=group_norm_coef,
                 new_stats=lambda B, L, C, device: torch.zeros((B, (L + 63) // 64, C, 2), dtype=torch.float32))
    saved = {k: getattr(ops, k) for k in names}
    with _ops_emu_gn.patched():
        try:
            for k, v in names.items():
                setattr(ops, k, v)
            yield
        finally:
            for k, v in saved.items():
                setattr(ops, k, v)
