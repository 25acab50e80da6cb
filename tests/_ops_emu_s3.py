"""TEST INFRASTRUCTURE: float64 CPU emulations of the CONTRACTS of the operators the S3 tokenizer's host schedule uses beyond ``tests/_ops_emu.py``:
``layernorm``, ``head_norm_rope`` (rotate-half, two tensors in one launch), ``flash_attention`` with ``lens_k``, and the two entry points of
``csrc/s3.hip``, ``fsmn_memory`` and ``fsq_encode`` (``include/mi355audio.h``).  Not a fallback: nothing under ``mlx_audio_amd/`` imports it."""
import contextlib

import numpy as np
import torch

import _ops_emu
from mlx_audio_amd import ops


def layernorm(x, y, *, weight=None, bias=None, ada_gb=None, res=None, eps=1e-5, lens=None, post_act=0, post_slope=0.0, split=0):
    assert ada_gb is None and res is None and post_act == 0 and split == 0, "not emulated"
    d = x.double()
    v = (d - d.mean(-1, keepdim=True)) / torch.sqrt(d.var(-1, unbiased=False, keepdim=True) + eps)
    if weight is not None:
        v = v * weight.double() + (0 if bias is None else bias.double())
    if lens is None:
        y.copy_(v.to(y.dtype))
    else:
        for b in range(x.shape[0]):
            y[b, :int(lens[b])] = v[b, :int(lens[b])].to(y.dtype)
    return y


def head_norm_rope(x, y, *, heads, dh, norm_weight=None, eps=1e-6, cos=None, sin=None, pos=None, pos0=0, interleaved=False, lens=None, second=None,
                   pos_sub=None):
    assert norm_weight is None and pos is None and pos_sub is None and not interleaved and lens is None, "not emulated"
    assert cos.shape[1] == dh // 2 and pos0 + x.shape[1] <= cos.shape[0]

    def one(src, dst, n):
        B, L = src.shape[0], src.shape[1]
        t = src[:, :, :n * dh].double().reshape(B, L, n, dh)
        c, s = cos[pos0:pos0 + L].double()[None, :, None, :], sin[pos0:pos0 + L].double()[None, :, None, :]
        a, b = t[..., :dh // 2], t[..., dh // 2:]
        dst[:, :, :n * dh] = torch.cat([a * c - b * s, b * c + a * s], -1).reshape(B, L, n * dh).to(dst.dtype)

    one(x, y, heads)
    if second is not None:
        x2, y2, heads2, nw2 = second
        assert nw2 is None
        one(x2, y2, heads2)
    return y


def flash_attention(q, k, v, out, *, heads, kv_heads=None, dh, scale=None, causal=False, window=0, lens_q=None, lens_k=None, mode=0, k_start=None,
                    head_major=False, nsplit=0, fused=None):
    assert kv_heads in (None, heads) and not causal and window == 0 and lens_q is None and k_start is None and not head_major and fused is None, "not emulated"
    B, T = q.shape[0], q.shape[1]
    q4, k4, v4 = (t[:, :, :heads * dh].double().reshape(B, -1, heads, dh) for t in (q, k, v))
    sc = torch.einsum("bqhd,bkhd->bhqk", q4, k4) * (dh ** -0.5 if scale is None else scale)
    if lens_k is not None:
        ok = torch.arange(k.shape[1])[None, :] < lens_k.reshape(-1, 1)
        sc = sc.masked_fill(~ok[:, None, None, :], float("-inf"))
    out[:, :, :heads * dh] = torch.einsum("bhqk,bkhd->bqhd", torch.softmax(sc, -1), v4).reshape(B, T, heads * dh).to(out.dtype)
    return out


def fsmn_memory(v, w, y, *, add=None, lens=None):
    """mi355_fsmn_memory, restated: y = add + m(t) * (sum_j w[:, j] * (m v)[t + j - left] + (m v)[t])."""
    B, L, C = v.shape
    K = w.shape[1]
    assert K % 2 == 1 and K <= ops.FSMN_MAX_TAPS and y.shape == v.shape and y.data_ptr() != v.data_ptr()
    left = (K - 1) // 2
    m = torch.ones((B, L), dtype=torch.float64) if lens is None else (torch.arange(L)[None, :] < lens.reshape(-1, 1).clamp(0, L)).double()
    vm = v.double() * m[:, :, None]
    xp = torch.zeros((B, L + K - 1, C), dtype=torch.float64)
    xp[:, left:left + L] = vm
    acc = torch.zeros((B, L, C), dtype=torch.float64)
    for j in range(K):
        acc += xp[:, j:j + L] * w[:, j].double()
    r = (acc + vm) * m[:, :, None]
    if add is not None:
        r = r + add.double()
    y.copy_(r.to(y.dtype))
    return y


def fsq_encode(x, w, b, *, lens=None, return_h=False):
    """mi355_fsq_encode, restated (h in float64, the decision on its float32 value)."""
    h = x.double() @ w.double().t() + (0 if b is None else b.double())
    t = (torch.tanh(h.float()) * np.float32(ops.FSQ_SCALE)).numpy()
    codes = torch.from_numpy(((np.rint(t).astype(np.int64) + 1) * (3 ** np.arange(8))).sum(-1).astype(np.int32))
    h = h.float()
    if lens is not None:
        ok = torch.arange(x.shape[1])[None, :] < lens.reshape(-1, 1)
        codes, h = codes * ok, h * ok[:, :, None]
    return (codes.to(torch.int32), h) if return_h else codes.to(torch.int32)


@contextlib.contextmanager
def patched():
    names = dict(layernorm=layernorm, head_norm_rope=head_norm_rope, flash_attention=flash_attention, fsmn_memory=fsmn_memory, fsq_encode=fsq_encode)
    saved = {k: getattr(ops, k) for k in names}
    with _ops_emu.patched():
        try:
            for k, v in names.items():
                setattr(ops, k, v)
            yield
        finally:
            for k, v in saved.items():
                setattr(ops, k, v)
