"""TEST INFRASTRUCTURE: float64 CPU emulations of the CONTRACTS of the three group-norm entry points (``include/mi355audio.h``: ``mi355_group_norm_stats``
/ ``_coef`` / ``_apply``), on top of ``tests/_ops_emu.py`` -- to dry-run the ``time_group_norm`` host schedule of the EnCodec engine on the CPU suite.
Not a fallback: nothing under ``mlx_audio_amd/`` imports it."""
import contextlib

import torch

import _ops_emu
from mlx_audio_amd import ops

PART = ops.GN_PART_ELEMS


def group_norm_stats(x, lens=None):
    """[B, parts, 2] float64 = (sum, sum of squared deviations from the part's mean) per part of PART consecutive valid elements."""
    B, L, C = x.shape
    parts = torch.zeros((B, (L * C + PART - 1) // PART, 2), dtype=torch.float64)
    for b in range(B):
        n = L if lens is None else int(lens[b])
        flat = x[b, :n].double().reshape(-1)
        for p in range((flat.numel() + PART - 1) // PART):
            v = flat[p * PART:(p + 1) * PART]
            parts[b, p, 0], parts[b, p, 1] = v.sum(), ((v - v.mean()) ** 2).sum()
    return parts


def group_norm_coef(partials, L, C, weight, bias, *, eps=1e-5, lens=None, rep=1, return_stats=False):
    assert partials.dim() == 3 and partials.dtype == torch.float64, "conv partials are not emulated"
    B = partials.shape[0]
    ld = ops.round_up(rep * C, 32)
    scale, shift, mr = torch.zeros((B, ld)), torch.zeros((B, ld)), torch.zeros((B, 2))
    for b in range(B):
        total = (L if lens is None else int(lens[b])) * C
        npart = (total + PART - 1) // PART
        cnt = torch.tensor([min(PART, total - p * PART) for p in range(npart)], dtype=torch.float64)
        s, q = partials[b, :npart, 0], partials[b, :npart, 1]
        mean = s.sum() / total
        var = (q + cnt * (s / cnt - mean) ** 2).sum() / total
        rstd = 1.0 / torch.sqrt(var + eps)
        sc = (torch.ones(C, dtype=torch.float64) if weight is None else weight.double()) * rstd
        sh = (torch.zeros(C, dtype=torch.float64) if bias is None else bias.double()) - mean * sc
        scale[b, :rep * C], shift[b, :rep * C] = sc.repeat(rep).float(), sh.repeat(rep).float()
        mr[b, 0], mr[b, 1] = mean, rstd
    return (scale, shift, mr) if return_stats else (scale, shift)


def group_norm_apply(x0, coef0, y, x1=None, coef1=None, *, row_off0=0, row_off1=0):
    B, L, C = y.shape
    assert x0.shape[1] >= L + row_off0
    v = x0[:, row_off0:row_off0 + L].double() * coef0[0][:, None, :C].double() + coef0[1][:, None, :C].double()
    if x1 is not None:
        assert x1.shape[1] >= L + row_off1
        u = x1[:, row_off1:row_off1 + L].double()
        v = v + (u if coef1 is None else u * coef1[0][:, None, :C].double() + coef1[1][:, None, :C].double())
    else:
        assert coef1 is None
    y[:] = v.to(y.dtype)
    return y


@contextlib.contextmanager
def patched():
    names = dict(group_norm_stats=group_norm_stats, group_norm_coef=group_norm_coef, group_norm_apply=group_norm_apply)
    saved = {k: getattr(ops, k) for k in names}
    with _ops_emu.patched():
        try:
            for k, v in names.items():
                setattr(ops, k, v)
            yield
        finally:
            for k, v in saved.items():
                setattr(ops, k, v)
