"""``csrc/s3.hip`` against float64 on the host: ``fsmn_memory`` and ``fsq_encode``.  The bars are the float32 summation bounds, derived and not tuned; the
measured maxima are written next to them."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
EDGE = math.atanh(0.5 / 0.9990000128746033)


def _fsmn_case(B, L, C, K, lens, strided, with_add, seed):
    g = torch.Generator().manual_seed(seed)
    if strided:
        buf = torch.randn(B, L, 3 * C, generator=g).to(DEV)
        v = buf[:, :, 2 * C:]
    else:
        v = torch.randn(B, L, C, generator=g).to(DEV)
    w = (0.1 * torch.randn(C, K, generator=g)).to(DEV)
    add = torch.randn(B, L, C, generator=g).to(DEV) if with_add else None
    return v, w, add, None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)


def _fsmn_ref(v, w, add, lens):
    """(value, bound base) in float64: bound base = sum_j |w_j v_j| + |v| + |add|."""
    B, L, C = v.shape
    K = w.shape[1]
    left = (K - 1) // 2
    vd, wd = v.double().cpu(), w.double().cpu()
    m = torch.ones(B, L, dtype=torch.float64) if lens is None else (torch.arange(L)[None, :] < lens.cpu()[:, None]).double()
    vm = vd * m[:, :, None]
    xp = torch.zeros(B, L + K - 1, C, dtype=torch.float64)
    xp[:, left:left + L] = vm
    acc, mag = torch.zeros(B, L, C, dtype=torch.float64), torch.zeros(B, L, C, dtype=torch.float64)
    for j in range(K):
        t = xp[:, j:j + L] * wd[:, j]
        acc += t
        mag += t.abs()
    val = (acc + vm) * m[:, :, None]
    mag = (mag + vm.abs()) * m[:, :, None]
    if add is not None:
        val, mag = val + add.double().cpu(), mag + add.double().cpu().abs()
    return val, mag, m


def _lens_for(B, L):
    base = [0, L, max(L // 2, 1), max(L - 1, 0), 1, min(17, L)]
    return [base[i % len(base)] for i in range(B)]


@pytest.mark.parametrize("C", [64, 128, 1280, 1000])
@pytest.mark.parametrize("L", [1, 15, 16, 31, 250, 751])
@pytest.mark.parametrize("K", [31, 3])
def test_fsmn_memory(C, L, K):
    """Bar per element: 2 (K + 3) 2^-24 (sum_j |w_j v_j| + |v| + |add|); positions beyond ``lens`` equal ``add`` exactly (0 without it).
    Measured on MI355X: the largest error / bar ratio over all cases is 0.26 (K = 3, where the bar is tightest), 0.02 - 0.07 for K = 31."""
    from mlx_audio_amd import ops

    B = 4
    worst = 0.0
    for strided in (True, False):
        for with_add in (True, False):
            for lens in (_lens_for(B, L), None):
                v, w, add, ld = _fsmn_case(B, L, C, K, lens, strided, with_add, seed=C + L + K)
                y = torch.full((B, L, C), float("nan"), device=DEV)
                ops.fsmn_memory(v, w, y, add=add, lens=ld)
                y2 = torch.full((B, L, C), float("nan"), device=DEV)
                ops.fsmn_memory(v, w, y2, add=add, lens=ld)
                torch.cuda.synchronize()
                assert torch.equal(y, y2), "two calls on the same bytes differ"
                val, mag, m = _fsmn_ref(v, w, add, ld)
                err = (y.double().cpu() - val).abs()
                bound = 2 * (K + 3) * U * mag
                assert bool((err <= bound).all()), (strided, with_add, lens, float((err - bound).max()))
                worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
                pad = m[:, :, None].expand_as(val) == 0
                if pad.any():
                    want = add.cpu()[pad] if with_add else torch.zeros(int(pad.sum()))
                    assert torch.equal(y.cpu()[pad], want)
    print(f"fsmn_memory C={C} L={L} K={K}: worst error / bound = {worst:.3f}")


def test_fsmn_memory_refuses_bad_arguments():
    from mlx_audio_amd import _lib, ops

    v, w = torch.randn(1, 8, 64, device=DEV), torch.randn(64, 4, device=DEV)
    with pytest.raises(_lib.Mi355Error, match="odd"):
        ops.fsmn_memory(v, w, torch.empty_like(v))
    with pytest.raises(_lib.Mi355Error, match="odd"):
        ops.fsmn_memory(v, torch.randn(64, 33, device=DEV), torch.empty_like(v))
    with pytest.raises(_lib.Mi355Error, match="alias"):
        ops.fsmn_memory(v, torch.randn(64, 3, device=DEV), v)


def _fsq_ref(x, w, b):
    xd, wd = x.double().cpu(), w.double().cpu()
    h = xd @ wd.t() + b.double().cpu()
    mag = xd.abs() @ wd.abs().t() + b.double().cpu().abs()
    digits = torch.round(torch.tanh(h) * 0.9990000128746033) + 1   # float64 decision (half to even)
    codes = (digits * (3.0 ** torch.arange(8, dtype=torch.float64))).sum(-1).to(torch.int64)
    return h, mag, codes


@pytest.mark.parametrize("C", [128, 1280])
@pytest.mark.parametrize("rows", [1, 3, 250, 4097, 16000])
def test_fsq_encode(C, rows):
    """``h`` within (C + 2) 2^-24 (sum_i |w_i x_i| + |b|) of float64; every code whose float64 margin exceeds its row's bound equals the float64 decision,
    the rest are counted (< 5 % of the rows).  Measured on MI355X: |h error| <= 1.4e-6 = 0.0095 of the bound at C = 128 and 0.0004 at C = 1280; rows
    inside the bound of an edge: 348 of 16 000 (2.2 %) at C = 1280, where the worst-case bound is 2.7e-3 wide."""
    from mlx_audio_amd import ops

    g = torch.Generator().manual_seed(C + rows)
    x = torch.randn(rows, C, generator=g).to(DEV)
    w = (2.0 * torch.randn(8, C, generator=g) / math.sqrt(C)).to(DEV)
    b = (0.1 * torch.randn(8, generator=g)).to(DEV)
    codes, h = ops.fsq_encode(x, w, b, return_h=True)
    codes2, h2 = ops.fsq_encode(x, w, b, return_h=True)
    only = ops.fsq_encode(x, w, b)
    torch.cuda.synchronize()
    assert codes.dtype == torch.int32 and codes.shape == (rows,) and h.shape == (rows, 8)
    assert torch.equal(codes, codes2) and torch.equal(h, h2) and torch.equal(codes, only), "two calls on the same bytes differ"
    hr, mag, cr = _fsq_ref(x, w, b)
    bound = (C + 2) * U * mag
    err = (h.double().cpu() - hr).abs()
    assert bool((err <= bound).all()), float((err / bound).max())
    margin = ((hr.abs() - EDGE).abs() - bound).min(-1).values   # > 0: no digit of the row can flip within the bound
    sure = margin > 0
    assert torch.equal(codes.cpu().to(torch.int64)[sure], cr[sure])
    unsure = int((~sure).sum())
    assert unsure < max(1, 0.05 * rows), (unsure, rows)
    assert int(codes.min()) >= 0 and int(codes.max()) < 6561
    print(f"fsq_encode C={C} rows={rows}: worst h error / bound = {float((err / bound).max()):.4f}, max |err| = {float(err.max()):.2e}, rows inside the bound of an edge: {unsure}")


def test_fsq_encode_fixed_points_and_lens():
    from mlx_audio_amd import ops

    C, B, L = 128, 3, 40
    w = torch.randn(8, C, device=DEV)
    z = ops.fsq_encode(torch.zeros(B, L, C, device=DEV), w, torch.zeros(8, device=DEV))
    assert z.shape == (B, L) and bool((z == 3280).all())   # all digits 1
    assert bool((ops.fsq_encode(torch.zeros(5, C, device=DEV), w, None) == 3280).all())
    # saturated digits: h = +-20
    sign = torch.tensor([1.0, -1.0, 1.0, 1.0, -1.0, -1.0, 1.0, -1.0], device=DEV)
    c, h = ops.fsq_encode(torch.zeros(4, C, device=DEV), w, 20.0 * sign, return_h=True)
    want = int(sum((int(s) + 1) * 3 ** d for d, s in enumerate(sign.tolist())))
    assert bool((c == want).all()) and torch.equal(h, (20.0 * sign).expand(4, 8))
    # rows at and beyond lens: code 0, h 0
    lens = torch.tensor([40, 0, 13], dtype=torch.int32, device=DEV)
    x = torch.randn(B, L, C, device=DEV)
    c, h = ops.fsq_encode(x, w, torch.zeros(8, device=DEV), lens=lens, return_h=True)
    full = ops.fsq_encode(x, w, torch.zeros(8, device=DEV))
    for b, n in enumerate(lens.tolist()):
        assert torch.equal(c[b, :n], full[b, :n]) and not c[b, n:].any() and not h[b, n:].any()
    # a strided view: the hidden state as the first third of a wider buffer
    wide = torch.randn(B, L, 3 * C, device=DEV)
    assert torch.equal(ops.fsq_encode(wide[:, :, :C], w, None), ops.fsq_encode(wide[:, :, :C].contiguous(), w, None))
