"""TEST INFRASTRUCTURE: float64 CPU emulations of the CONTRACTS of the operators DeepFilterNet's host schedule uses beyond ``tests/_ops_emu.py``:
``gru_seq`` (``csrc/gru.hip``), ``dfn_features``, ``dfn_conv2d`` and ``dfn_apply`` (``csrc/dfn.hip``), and ``stft_frames`` / ``istft_frames`` without
padding modes.  Each restates ``include/mi355audio.h``, in float64 and stored as the buffers' float32.  Not a fallback: nothing under
``mlx_audio_amd/`` imports it."""
import contextlib

import numpy as np
import torch

import _gru_ref
import _ops_emu
from mlx_audio_amd import ops


def _lens(lens, B, T):
    return [T] * B if lens is None else [min(max(int(n), 0), T) for n in lens]


def gru_seq(xproj, wh, bhn, out, *, h0=None, lens=None, return_state=False):
    B, T, _ = xproj.shape
    w = wh.w.view(torch.float16).double().view(wh.h // 8, 3 * wh.h, 8).permute(1, 0, 2).reshape(3 * wh.h, wh.h) * wh.scale   # what the image holds
    o, hT = _gru_ref.gru_seq(xproj.double().numpy(), w.numpy(), bhn.double().numpy(), None if h0 is None else h0.double().numpy(),
                             None if lens is None else _lens(lens, B, T))
    out.copy_(torch.from_numpy(o).to(out.dtype))
    return (out, torch.from_numpy(hT).float()) if return_state else out


def dfn_features(spec, *, wnorm, alpha, one_minus_alpha, nb_erb, nb_df, lookahead=0, erb_fb=None, erb_start=None, lens=None):
    B, T, F, _ = spec.shape
    s = spec.double() * wnorm
    fe, fd = torch.zeros(B, T, nb_erb, 1), torch.zeros(B, T, nb_df, 2)
    out = torch.zeros(B, T, F, 2)
    for b, n in enumerate(_lens(lens, B, T)):
        la = lookahead if n > lookahead else 0
        out[b, :n] = s[b, :n].float()
        mag2 = s[b, :n, :, 0] ** 2 + s[b, :n, :, 1] ** 2
        if erb_fb is not None:
            e = mag2 @ erb_fb.double()
        else:
            st = [int(v) for v in erb_start]
            e = torch.stack([mag2[:, st[i]:st[i + 1]].mean(1) for i in range(nb_erb)], 1)
        db = 10.0 * torch.log10(e + 1e-10)
        se = torch.linspace(-60.0, -90.0, nb_erb, dtype=torch.float64)
        sd = torch.linspace(0.001, 0.0001, nb_df, dtype=torch.float64)
        mag = torch.sqrt(mag2[:, :nb_df])
        for t in range(n):
            se = db[t] * one_minus_alpha + se * alpha
            sd = mag[t] * one_minus_alpha + sd * alpha
            if t - la >= 0:
                fe[b, t - la, :, 0] = ((db[t] - se) / 40.0).float()
                fd[b, t - la] = (s[b, t, :nb_df] / torch.sqrt(sd)[:, None]).float()
    return out, fe, fd


def dfn_conv2d(x, cv, *, add=None, lens=None):
    B, T, F, C = x.shape
    kt, kf = cv.kt, cv.kf
    ys = []
    for b, n in enumerate(_lens(lens, B, T)):
        xb = x[b].double().clone()
        xb[n:] = 0.0
        xt = xb.permute(2, 0, 1)[None]                                        # [1, C, T, F]
        w = cv.w.double()
        if cv.transposed:
            y = torch.nn.functional.conv_transpose2d(xt, w, stride=(1, cv.fstride), padding=(kt - 1, kf // 2), output_padding=(0, kf // 2), groups=cv.groups)
        else:
            xp = torch.nn.functional.pad(xt, (kf // 2, kf // 2, kt - 1 - cv.lookahead, cv.lookahead))
            y = torch.nn.functional.conv2d(xp, w, stride=(1, cv.fstride), groups=cv.groups)
        if cv.pw is not None:
            y = torch.einsum("oc,nctf->notf", cv.pw.double(), y)
        y = y[0].permute(1, 2, 0)                                             # [T, Fo, Cout]
        if cv.scale is not None:
            y = y * cv.scale.double()
        if cv.shift is not None:
            y = y + cv.shift.double()
        if cv.act == ops.DFN_ACT_RELU:
            y = torch.relu(y)
        elif cv.act == ops.DFN_ACT_SIGMOID:
            y = torch.sigmoid(y)
        if add is not None:
            y = y + add[b].double()
        y[n:] = 0.0
        ys.append(y.float())
    return torch.stack(ys)


def dfn_apply(spec, m, erb_inv_fb, coef, *, order, df_lookahead, mask_first, wnorm, lens=None):
    return dfn_apply64(spec, m, erb_inv_fb, coef, order=order, df_lookahead=df_lookahead, mask_first=mask_first, wnorm=wnorm, lens=lens).to(torch.complex64)


def dfn_apply64(spec, m, erb_inv_fb, coef, *, order, df_lookahead, mask_first, wnorm, lens=None):
    """complex128: what the kernel tests hold the device to."""
    B, T, F, _ = spec.shape
    D = coef.shape[2]
    out = torch.zeros(B, T, F, dtype=torch.complex128)
    for b, n in enumerate(_lens(lens, B, T)):
        s = torch.view_as_complex(spec[b, :n].double().contiguous())          # [n, F]
        gain = m[b, :n].reshape(n, -1).double() @ erb_inv_fb.double()
        masked = s * gain
        src = (masked if mask_first else s)[:, :D]
        left = order - 1 - df_lookahead
        pad = torch.cat([torch.zeros(left, D, dtype=src.dtype), src, torch.zeros(df_lookahead, D, dtype=src.dtype)])
        c = torch.view_as_complex(coef[b, :n].double().contiguous())          # [n, D, order]
        df = sum(pad[k:k + n] * c[:, :, k] for k in range(order))
        out[b, :n] = torch.cat([df, masked[:, D:]], 1) / wnorm
    return out


def stft_frames(x, n_fft, hop, window, pad_mode, n_frames):
    assert pad_mode == 0, "not emulated"
    idx = torch.arange(n_frames)[:, None] * hop + torch.arange(n_fft)[None, :]
    return torch.fft.rfft(x.double()[:, idx] * window.double(), dim=-1).to(torch.complex64)


def istft_frames(spec, n_fft, hop, window, norm, norm_mode, clamp, trim, out_len):
    assert norm_mode == 1 and not clamp, "not emulated"
    B, n_frames = spec.shape[:2]
    fr = torch.fft.irfft(spec.to(torch.complex128), n=n_fft, dim=-1) * window.double()
    y = torch.zeros(B, (n_frames - 1) * hop + n_fft, dtype=torch.float64)
    for t in range(n_frames):
        y[:, t * hop:t * hop + n_fft] += fr[:, t]
    nd = norm.double()
    y = torch.where(nd > 1e-10, y / nd, y)
    return y[:, trim:trim + out_len].float()


@contextlib.contextmanager
def patched():
    names = dict(gru_seq=gru_seq, dfn_features=dfn_features, dfn_conv2d=dfn_conv2d, dfn_apply=dfn_apply, stft_frames=stft_frames, istft_frames=istft_frames)
    saved = {k: getattr(ops, k) for k in names}
    with _ops_emu.patched():
        try:
            for k, v in names.items():
                setattr(ops, k, v)
            yield
        finally:
            for k, v in saved.items():
                setattr(ops, k, v)
