"""TEST INFRASTRUCTURE: float64 CPU emulations of the CONTRACTS of the three entry points of ``csrc/conformer.hip`` (``include/mi355audio.h``):
``relpos_attention`` (by the header's index formula ``p[center - (i - j)]``), ``glu_dwconv_silu`` and ``stencil2d_k3s2``; everything else the Parakeet
host schedule uses comes from ``tests/_ops_emu.py`` and ``tests/_ops_emu_s3.py``, imported unchanged.  Not a fallback: nothing under ``mlx_audio_amd/``
imports it."""
import contextlib

import torch

import _ops_emu_s3
from mlx_audio_amd import ops


def _len(lens, b, full):
    return full if lens is None else min(max(int(lens[b]), 0), full)


def relpos_attention(q, k, v, p, bias_u, bias_v, out, *, heads, dh, center, scale=None, lens=None):
    B, T = q.shape[0], q.shape[1]
    hd = heads * dh
    assert dh in (64, 128) and center - (T - 1) >= 0 and center + T - 1 < p.shape[0], "mi355_relpos_attention refuses this call"
    scale = dh ** -0.5 if scale is None else scale
    u, vb = bias_u.double().reshape(heads, 1, dh), bias_v.double().reshape(heads, 1, dh)
    for b in range(B):
        n = _len(lens, b, T)
        out[b, :, :hd] = 0
        if n == 0:
            continue
        q4, k4, v4 = (t[b, :n, :hd].double().reshape(n, heads, dh).transpose(0, 1) for t in (q, k, v))
        i, j = torch.arange(n)[:, None], torch.arange(n)[None, :]
        pr = p[:, :hd].double().reshape(-1, heads, dh)[center - (i - j)]                   # [n, n, H, dh]
        s = (q4 + u) @ k4.transpose(1, 2) + torch.einsum("hid,ijhd->hij", q4 + vb, pr)
        out[b, :n, :hd] = (torch.softmax(s * scale, -1) @ v4).transpose(0, 1).reshape(n, hd).to(out.dtype)
    return out


def glu_dwconv_silu(x, w, b, y, *, lens=None):
    B, L, C2 = x.shape
    C, K = w.shape
    assert C2 == 2 * C and C % 4 == 0 and K % 2 == 1 and K <= ops.GLU_DWCONV_MAX_TAPS and y.data_ptr() != x.data_ptr()
    left = (K - 1) // 2
    m = torch.ones((B, L), dtype=torch.float64) if lens is None else (torch.arange(L)[None, :] < lens.reshape(-1, 1).clamp(0, L)).double()
    xd = x.double()
    g = xd[:, :, :C] * torch.sigmoid(xd[:, :, C:]) * m[:, :, None]
    gp = torch.zeros((B, L + K - 1, C), dtype=torch.float64)
    gp[:, left:left + L] = g
    z = torch.zeros((B, L, C), dtype=torch.float64) + (0 if b is None else b.double())
    for k in range(K):
        z = z + gp[:, k:k + L] * w[:, k].double()
    y.copy_((z * torch.sigmoid(z) * m[:, :, None]).to(y.dtype))
    return y


def stencil2d_k3s2(x, w, bias, y, *, relu=False, lens_in=None, lens_out=None):
    B, T, F = x.shape[:3]
    C = w.shape[0]
    To, Fo = ops.stencil2d_out(T), ops.stencil2d_out(F)
    assert tuple(y.shape) == (B, To, Fo, C) and tuple(w.shape) == (C, 3, 3)
    xd = x.double() if x.dim() == 4 else x.double()[..., None].expand(B, T, F, C)
    mi = torch.ones((B, T), dtype=torch.float64) if lens_in is None else (torch.arange(T)[None, :] < lens_in.reshape(-1, 1).clamp(0, T)).double()
    xp = torch.zeros((B, 2 * To + 1, 2 * Fo + 1, C), dtype=torch.float64)
    xp[:, 1:T + 1, 1:F + 1] = xd * mi[:, :, None, None]
    acc = torch.zeros((B, To, Fo, C), dtype=torch.float64) + (0 if bias is None else bias.double())
    for kh in range(3):
        for kw in range(3):
            acc = acc + xp[:, kh:kh + 2 * To:2, kw:kw + 2 * Fo:2] * w[:, kh, kw].double()
    if relu:
        acc = acc.clamp_min(0)
    mo = torch.ones((B, To), dtype=torch.float64) if lens_out is None else (torch.arange(To)[None, :] < lens_out.reshape(-1, 1).clamp(0, To)).double()
    y.copy_((acc * mo[:, :, None, None]).to(y.dtype))
    return y


@contextlib.contextmanager
def patched():
    names = dict(relpos_attention=relpos_attention, glu_dwconv_silu=glu_dwconv_silu, stencil2d_k3s2=stencil2d_k3s2)
    saved = {k: getattr(ops, k) for k in names}
    with _ops_emu_s3.patched():
        try:
            for k, v in names.items():
                setattr(ops, k, v)
            yield
        finally:
            for k, v in saved.items():
                setattr(ops, k, v)
