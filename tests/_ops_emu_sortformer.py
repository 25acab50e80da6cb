"""TEST INFRASTRUCTURE: float64 CPU emulations of the CONTRACTS of what the Sortformer host schedule uses beyond ``tests/_ops_emu_parakeet.py``:
``narrow_attention`` (``include/mi355audio.h``: the keys at and beyond ``lens[b]`` are not looked at, output rows there are zero, the widths and the
``lens`` range it refuses) and ``layernorm`` with ``res=`` (normalise ``x + res``).  Not a fallback: nothing under ``mlx_audio_amd/`` imports it."""
import contextlib

import torch

import _ops_emu_parakeet
import _ops_emu_s3
from mlx_audio_amd import _lib, ops


def narrow_attention(q, k, v, out, *, heads, dh, scale=None, lens=None, check_lens=True):
    B, T = q.shape[0], q.shape[1]
    hd = heads * dh
    if dh not in (8, 16, 24, 32):
        raise _lib.Mi355Error(f"narrow_attention: dh must be 8, 16, 24 or 32 (got dh = {dh})")
    if lens is not None and check_lens and (int(lens.min()) < 1 or int(lens.max()) > T):
        raise _lib.Mi355Error("narrow_attention: lens must lie in [1, T]")
    scale = dh ** -0.5 if scale is None else scale
    for b in range(B):
        n = T if lens is None else min(max(int(lens[b]), 0), T)
        out[b, :, :hd] = 0
        if n == 0:
            continue
        q4, k4, v4 = (t[b, :n, :hd].double().reshape(n, heads, dh).transpose(0, 1) for t in (q, k, v))
        out[b, :n, :hd] = (torch.softmax(q4 @ k4.transpose(1, 2) * scale, -1) @ v4).transpose(0, 1).reshape(n, hd).to(out.dtype)
    return out


def layernorm(x, y, *, weight=None, bias=None, ada_gb=None, res=None, eps=1e-5, lens=None, post_act=0, post_slope=0.0, split=0):
    if res is not None:
        x = x.double() + res.double()
    return _ops_emu_s3.layernorm(x, y, weight=weight, bias=bias, ada_gb=ada_gb, eps=eps, lens=lens, post_act=post_act, post_slope=post_slope, split=split)


@contextlib.contextmanager
def patched():
    names = dict(narrow_attention=narrow_attention, layernorm=layernorm)
    saved = {k: getattr(ops, k) for k in names}
    with _ops_emu_parakeet.patched():
        try:
            for k, v in names.items():
                setattr(ops, k, v)
            yield
        finally:
            for k, v in saved.items():
                setattr(ops, k, v)
