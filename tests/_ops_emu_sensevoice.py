"""TEST INFRASTRUCTURE: float64 CPU emulations of the CONTRACTS of the three entry points of ``csrc/sanm.hip`` (``include/mi355audio.h``):
``sanm_input`` (by the header's clamp formula), ``ctc_rows`` and ``ctc_collapse``; the fbank comes from ``oracle/dsp_ref.compute_fbank_kaldi`` and
everything else the SenseVoice host schedule uses from ``tests/_ops_emu_sortformer.py`` (which chains ``_ops_emu_parakeet.py``, ``_ops_emu_s3.py`` and
``_ops_emu.py``), imported unchanged.  Not a fallback: nothing under ``mlx_audio_amd/`` imports it."""
import contextlib

import numpy as np
import torch

import _ops_emu_sortformer
from mlx_audio_amd import dsp, ops


def sanm_input(feats, embed, qids, pe, *, lfr_m, lfr_n, scale, lens=None, means=None, istd=None, x=None):
    B, T, D = feats.shape
    W, rows = lfr_m * D, ops.sanm_rows(T, lfr_n)
    assert tuple(embed.shape) == (16, W) and tuple(qids.shape) == (B, 4) and (means is None) == (istd is None)
    assert pe is None or (pe.shape[1] == W and pe.shape[0] >= rows), "mi355_sanm_input refuses this call"
    out = torch.zeros((B, rows, W), dtype=torch.float64)
    out_lens = torch.empty((B,), dtype=torch.int32)
    left = (lfr_m - 1) // 2
    for b in range(B):
        n = T if lens is None else int(lens[b])
        assert 1 <= n <= T, "lens[b] in [1, T] is the caller's contract"
        r = 4 + -(-n // lfr_n)
        idx = (torch.arange(r - 4)[:, None] * lfr_n + torch.arange(lfr_m)[None, :] - left).clamp(0, n - 1)
        u = feats[b].double()[idx].reshape(r - 4, W)
        if means is not None:
            u = (u + means.double()) * istd.double()
        u = torch.cat([embed.double()[qids[b].long()], u]) * float(np.float32(scale))
        out[b, :r] = u if pe is None else u + pe[:r].double()
        out_lens[b] = r
    if x is None:
        x = torch.empty((B, rows, W), dtype=torch.float32)
    x.copy_(out.to(x.dtype))
    return x, out_lens


def ctc_rows(logits, *, ids=None, gap=None, lp=None, logp=None):
    rows, V = logits.shape
    x = logits.double()
    first = (x == x.max(-1, keepdim=True).values).double().argmax(-1)
    other = x.clone()
    other[torch.arange(rows), first] = -float("inf")
    g = (x.max(-1).values - other.max(-1).values) if V > 1 else torch.zeros(rows, dtype=torch.float64)
    lse = torch.logsumexp(x, -1)
    res = []
    for buf, val, dt in ((ids, first, torch.int32), (gap, g, torch.float32), (lp, x.max(-1).values - lse, torch.float32)):
        if buf is None:
            buf = torch.empty((rows,), dtype=dt)
        buf.copy_(val.to(dt))
        res.append(buf)
    if logp is not None:
        logp.copy_((x - lse[:, None]).to(logp.dtype))
    return tuple(res)


def ctc_collapse(ids, *, lens=None, skip=0, blank=0, return_frames=False):
    B, T = ids.shape
    tokens, frames = torch.full((B, T), -1, dtype=torch.int32), torch.full((B, T), -1, dtype=torch.int32)
    counts = torch.zeros((B,), dtype=torch.int32)
    for b in range(B):
        n = T if lens is None else min(max(int(lens[b]), 0), T)
        k = 0
        for t in range(skip, n):
            i = int(ids[b, t])
            if i != blank and (t == skip or int(ids[b, t - 1]) != i):
                tokens[b, k], frames[b, k] = i, t
                k += 1
        counts[b] = k
    return (tokens, counts, frames) if return_frames else (tokens, counts)


def compute_fbank_kaldi(waveform, **kw):
    from oracle import dsp_ref

    return torch.from_numpy(dsp_ref.compute_fbank_kaldi(torch.as_tensor(waveform).numpy(), **kw))


@contextlib.contextmanager
def patched():
    names = dict(sanm_input=sanm_input, ctc_rows=ctc_rows, ctc_collapse=ctc_collapse)
    saved = {k: getattr(ops, k) for k in names}
    saved_fbank = dsp.compute_fbank_kaldi
    with _ops_emu_sortformer.patched():
        try:
            for k, v in names.items():
                setattr(ops, k, v)
            dsp.compute_fbank_kaldi = compute_fbank_kaldi
            yield
        finally:
            for k, v in saved.items():
                setattr(ops, k, v)
            dsp.compute_fbank_kaldi = saved_fbank
