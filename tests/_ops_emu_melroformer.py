"""TEST INFRASTRUCTURE: float64 CPU emulations of the CONTRACTS of the operators Mel-Band RoFormer's host schedule uses beyond ``tests/_ops_emu.py``:
the three new ones -- ``band_split``, ``band_merge``, ``head_gate`` (``csrc/bandsplit.hip``) -- and ``rmsnorm``, ``head_norm_rope``,
``flash_attention`` (no masks), ``stft_frames`` with reflect padding and ``istft_frames``.  Each restates ``include/mi355audio.h``, in float64 and
stored as the buffers' float32.  The ``*64`` forms return float64 and, for the band kernels, the sum of the absolute terms of every output: what
the kernel tests hold the device to.  Not a fallback: nothing under ``mlx_audio_amd/`` imports it."""
import contextlib
import math

import numpy as np
import torch

import _ops_emu
import _ops_emu_dfn
from mlx_audio_amd import ops


def _planes(spec):
    s = torch.view_as_real(spec) if spec.is_complex() else spec
    return s.double()                                                            # [B2, T, F, 2]


def band_split64(spec, tab, wt, gamma, bias):
    """-> (y [B, T, Nb, D] float64, mag: sum_k |W[d, k] v[k]| + |bias[d]| per output)."""
    s = _planes(spec)
    B2, T, F, _ = s.shape
    Nb, D = tab.num_bands, bias.shape[1]
    cac = torch.zeros(B2 // 2, T, 2 * F + 1, 2, dtype=torch.float64)              # [B, T, j, (re, im)]; the extra slot reads as zero
    cac[:, :, 0:2 * F:2] = s[0::2]
    cac[:, :, 1:2 * F:2] = s[1::2]
    y = torch.zeros(B2 // 2, T, Nb, D, dtype=torch.float64)
    mag = torch.zeros_like(y)
    for n in range(Nb):
        p0, p1 = int(tab.band_ptr[n]), int(tab.band_ptr[n + 1])
        bd = 2 * (p1 - p0)
        ix = torch.from_numpy(tab.band_idx[p0:p1].astype(np.int64))
        ix = torch.where((ix >= 0) & (ix < 2 * F), ix, torch.full_like(ix, 2 * F))
        u = cac[:, :, ix].reshape(B2 // 2, T, bd)
        nrm = torch.sqrt((u * u).sum(-1, keepdim=True))
        v = u / torch.clamp(nrm, min=1e-12) * math.sqrt(bd) * gamma[2 * p0:2 * p1].double()
        w = wt[D * 2 * p0:D * 2 * p1].double().reshape(bd, D)
        y[:, :, n] = v @ w + bias[n].double()
        mag[:, :, n] = v.abs() @ w.abs() + bias[n].double().abs()
    return y, mag


def band_split(spec, tab, wt, gamma, bias, y=None):
    r = band_split64(spec, tab, wt, gamma, bias)[0].float()
    if y is None:
        return r
    y.copy_(r)
    return y


def band_merge64(h, tab, spec):
    """-> (out complex128 [B * 2, F, T], mag: the sum of the absolute products behind each of re / im, [B * 2, F, T])."""
    s = _planes(spec)
    B2, T, F, _ = s.shape
    hd = h.double()
    inv_ptr, inv_col, inv_bd = ops.band_inverse_host(tab.band_ptr, tab.band_idx, 2 * F)
    m = torch.zeros(B2 // 2, T, 2 * F, 2, dtype=torch.float64)
    ma = torch.zeros_like(m)
    for j in range(2 * F):
        c0, c1 = int(inv_ptr[j]), int(inv_ptr[j + 1])
        for c in range(c0, c1):                                                  # ascending band order
            col, bd = int(inv_col[c]), int(inv_bd[c])
            t = hd[:, :, col:col + 2] * torch.sigmoid(hd[:, :, col + bd:col + bd + 2])
            m[:, :, j] += t
            ma[:, :, j] += t.abs()
        m[:, :, j] /= max(c1 - c0, 1)
        ma[:, :, j] /= max(c1 - c0, 1)
    out = torch.zeros(B2, F, T, dtype=torch.complex128)
    mag = torch.zeros(B2, F, T, dtype=torch.float64)
    for ch in range(2):
        x = torch.view_as_complex(s[ch::2].contiguous())                         # [B, T, F]
        mk = torch.view_as_complex(m[:, :, ch::2].contiguous())
        out[ch::2] = (x * mk).transpose(1, 2)
        mag[ch::2] = ((s[ch::2, :, :, 0].abs() + s[ch::2, :, :, 1].abs()) * (ma[:, :, ch::2, 0] + ma[:, :, ch::2, 1])).transpose(1, 2)
    return out, mag


def band_merge(h, tab, spec, out=None):
    r = torch.view_as_real(band_merge64(h, tab, spec)[0].to(torch.complex64))
    if out is None:
        return torch.view_as_complex(r.contiguous())
    out.copy_(r)
    return torch.view_as_complex(out)


def head_gate64(x, g, heads, dh):
    B, L = x.shape[:2]
    v = x[:, :, :heads * dh].double().reshape(B, L, heads, dh) * torch.sigmoid(g[:, :, :heads].double())[..., None]
    return v.reshape(B, L, heads * dh)


def head_gate(x, g, *, heads, dh):
    x[:, :, :heads * dh] = head_gate64(x, g, heads, dh).float()
    return x


def rmsnorm(x, y, weight, eps=1e-6, lens=None):
    assert lens is None, "not emulated"
    v = x.double()
    r = v * torch.rsqrt((v * v).mean(-1, keepdim=True) + eps)
    y.copy_((r * weight.double() if weight is not None else r).float())
    return y


def head_norm_rope(x, y, *, heads, dh, norm_weight=None, eps=1e-6, cos=None, sin=None, pos=None, pos0=0, interleaved=False, lens=None, second=None,
                   pos_sub=None):
    assert norm_weight is None and pos is None and lens is None and pos_sub is None and interleaved and cos is not None, "not emulated"

    def rot(src, dst, nh):
        B, L = src.shape[:2]
        v = src[:, :, :nh * dh].double().reshape(B, L, nh, dh // 2, 2)
        c, s = cos[pos0:pos0 + L].double()[None, :, None, :], sin[pos0:pos0 + L].double()[None, :, None, :]
        r = torch.stack([v[..., 0] * c - v[..., 1] * s, v[..., 1] * c + v[..., 0] * s], dim=-1)
        dst[:, :, :nh * dh] = r.reshape(B, L, nh * dh).float()

    rot(x, y, heads)
    if second is not None:
        x2, y2, heads2, nw2 = second
        assert nw2 is None
        rot(x2, y2, heads2)
    return y


def flash_attention(q, k, v, out, *, heads, kv_heads=None, dh, scale=None, causal=False, window=0, lens_q=None, lens_k=None, mode=0, k_start=None,
                    head_major=False, nsplit=0, fused=None):
    assert not causal and window == 0 and lens_q is None and lens_k is None and k_start is None and not head_major and fused is None, "not emulated"
    assert kv_heads in (None, heads)
    B, Tq = q.shape[:2]
    Tk = k.shape[1]
    sp = lambda t, L: t[:, :, :heads * dh].double().reshape(B, L, heads, dh).transpose(1, 2)
    s = sp(q, Tq) @ sp(k, Tk).transpose(-1, -2) * (1.0 / math.sqrt(dh) if scale is None else scale)
    o = torch.softmax(s, dim=-1) @ sp(v, Tk)
    out[:, :, :heads * dh] = o.transpose(1, 2).reshape(B, Tq, heads * dh).float()
    return out


def stft_frames(x, n_fft, hop, window, pad_mode, n_frames):
    if pad_mode == 0:
        return _ops_emu_dfn.stft_frames(x, n_fft, hop, window, pad_mode, n_frames)
    assert pad_mode == 1, "not emulated"
    p = n_fft // 2
    xp = torch.cat([x[:, 1:p + 1].flip(1), x, x[:, -(p + 1):-1].flip(1)], dim=1)
    return _ops_emu_dfn.stft_frames(xp, n_fft, hop, window, 0, n_frames)


@contextlib.contextmanager
def patched():
    names = dict(band_split=band_split, band_merge=band_merge, head_gate=head_gate, rmsnorm=rmsnorm, head_norm_rope=head_norm_rope,
                 flash_attention=flash_attention, stft_frames=stft_frames, istft_frames=_ops_emu_dfn.istft_frames)
    saved = {k: getattr(ops, k) for k in names}
    with _ops_emu.patched():
        try:
            for k, v in names.items():
                setattr(ops, k, v)
            yield
        finally:
            for k, v in saved.items():
                setattr(ops, k, v)
