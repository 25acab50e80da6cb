"""``mi355_shift_scalenorm`` and ``mi355_gated_fsmn`` against their float64 contracts (``tests/_ops_emu_mossformer2.py``) on the same float32
inputs, within the per-element bounds derived there.  Each test prints the largest error / bound ratio (docs/COVERAGE.md records them)."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import _ops_emu_mossformer2 as E64  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _ratio(got, want, bound):
    err = (got.double().cpu() - want).abs()
    assert torch.isfinite(err).all()
    assert bool((err <= bound).all()), f"largest error {float(err.max()):.3e}, largest error / bound {float((err / bound.clamp(min=1e-300)).max()):.3f}"
    return float((err / bound.clamp(min=1e-300)).max())


@pytest.mark.parametrize("shift", [True, False])
@pytest.mark.parametrize("T,C", [(1, 64), (7, 64), (5, 512), (9, 1024), (3, 2048)])
def test_shift_scalenorm_against_float64(T, C, shift):
    from mlx_audio_amd import ops

    B = 2
    g = torch.Generator().manual_seed(T * 10000 + C)
    buf = torch.randn(B, T, C + 8, generator=g)
    x = buf[:, :, :C]
    if T > 2:
        x[1, 2] = 0           # shift: the row's second half is zero, its first half comes from row 1; no shift: an all-zero row
        if shift:
            x[1, 1, :C // 2] = 0
    gv = torch.tensor([1.7])
    lens = [T, max(T - 1, 1)]
    want, bound = E64.shift_scalenorm64(x, gv, 1e-5, shift, lens)
    ybuf = torch.full((B, T, C + 16), float("nan"), device=DEV)
    y = ops.shift_scalenorm(buf.to(DEV)[:, :, :C], ybuf[:, :, :C], g=gv.to(DEV), eps=1e-5, shift=shift, lens=torch.tensor(lens, dtype=torch.int32, device=DEV))
    r = _ratio(y, want, bound)
    print(f"shift_scalenorm T={T} C={C} shift={shift}: largest error / bound {r:.3f}")
    if T > 2 and lens[1] > 2:
        assert not y[1, 2].any()          # an all-zero row gives exactly zero
    if shift:
        assert not y[:, 0, :C // 2].any()  # nothing before row 0
    for b, n in enumerate(lens):
        assert not y[b, n:].any()
    assert torch.isnan(ybuf[:, :, C:]).all()
    # g = NULL is g = 1; two calls give the same bits
    y1 = ops.shift_scalenorm(buf.to(DEV)[:, :, :C], torch.empty((B, T, C), device=DEV), shift=shift)
    want1, bound1 = E64.shift_scalenorm64(x, None, 1e-8, shift, None)
    _ratio(y1, want1, bound1)
    assert torch.equal(y1, ops.shift_scalenorm(buf.to(DEV)[:, :, :C], torch.empty((B, T, C), device=DEV), shift=shift))


def test_shift_scalenorm_below_eps_and_refusals():
    from mlx_audio_amd import _lib, ops

    x = torch.full((1, 2, 64), 1e-9)
    want, bound = E64.shift_scalenorm64(x, None, 1e-5, False, None)
    y = ops.shift_scalenorm(x.to(DEV), torch.empty((1, 2, 64), device=DEV), eps=1e-5, shift=False)
    _ratio(y, want, bound)
    assert float(y.max()) < 1e-3   # divided by eps, not by the norm
    for C in (60, 4, 2056):
        with pytest.raises(_lib.Mi355Error, match="multiple of 8"):
            ops.shift_scalenorm(torch.zeros((1, 2, C), device=DEV), torch.empty((1, 2, C), device=DEV))
    xd = torch.zeros((1, 2, 64), device=DEV)
    with pytest.raises(_lib.Mi355Error, match="alias"):
        ops.shift_scalenorm(xd, xd, shift=True)


@pytest.mark.parametrize("K", [39, 3])
@pytest.mark.parametrize("T", [1, 19, 20, 40])
def test_gated_fsmn_against_float64(T, K):
    """T = 19 / 20 sit on either side of the 39-tap filter's half width + 1 (every tap of row 0 inside / one outside); T = 40 spans two row tiles;
    C = 80 leaves a partial channel block."""
    from mlx_audio_amd import ops

    B, C = 3, 80
    g = torch.Generator().manual_seed(T * 100 + K)
    bufs = [torch.randn(B, T, C + 4 * i, generator=g) for i in range(4)]
    p, xu, xv, res = [b[:, :, :C] for b in bufs]
    w = torch.randn(C, K, generator=g) / K ** 0.5
    lens = [T, max(T - 3, 1), 1]
    want, bound = E64.gated_fsmn64(p, xu, xv, res, w, lens)
    lens_dev = torch.tensor(lens, dtype=torch.int32, device=DEV)
    dp, dxu, dxv, dres = [b.to(DEV)[:, :, :C] for b in bufs]
    ybuf = torch.full((B, T, C + 8), float("nan"), device=DEV)
    y = ops.gated_fsmn(dp, dxu, dxv, dres, w.to(DEV), ybuf[:, :, :C], lens=lens_dev)
    r = _ratio(y, want, bound)
    print(f"gated_fsmn T={T} K={K}: largest error / bound {r:.3f}")
    for b, n in enumerate(lens):
        assert not y[b, n:].any()
    assert torch.isnan(ybuf[:, :, C:]).all()
    # y aliasing res: the same bits
    ops.gated_fsmn(dp, dxu, dxv, dres, w.to(DEV), dres, lens=lens_dev)
    assert torch.equal(dres, y)
    # each item alone: the same bits
    for b, n in enumerate(lens):
        one = [t.to(DEV)[b:b + 1, :n, :C].contiguous() for t in bufs]
        y1 = ops.gated_fsmn(*one, w.to(DEV), torch.empty((1, n, C), device=DEV))
        assert torch.equal(y1[0], y[b, :n]), b


def test_gated_fsmn_refusals():
    from mlx_audio_amd import _lib, ops

    x = torch.zeros((1, 4, 8), device=DEV)
    for K in (4, 65):
        with pytest.raises(_lib.Mi355Error, match="K must be odd"):
            ops.gated_fsmn(x, x, x, x, torch.zeros((8, K), device=DEV), torch.empty_like(x))
    with pytest.raises(_lib.Mi355Error, match="alias"):
        ops.gated_fsmn(x, x, x, x, torch.zeros((8, 3), device=DEV), x)
