"""``csrc/conformer.hip`` against float64 on the host: ``relpos_attention``, ``glu_dwconv_silu`` and ``stencil2d_k3s2``.  The bars are derived, not
tuned; the measured maxima are written next to them."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24


# ---------------------------------------------------------------------------------------------------- relpos_attention
def rel_shift_literal(x):
    """attention.py:82-91 restated with pad / reshape (NOT the index formula the kernel uses): [H, Tq, pos_len] -> [H, Tq, pos_len]."""
    H, Tq, pos_len = x.shape
    x = torch.nn.functional.pad(x, (1, 0))
    x = x.reshape(H, pos_len + 1, Tq)[:, 1:, :]
    return x.reshape(H, Tq, pos_len)


def relpos_ref_item(q, k, v, p, u, vb, center, H, dh, scale):
    """One un-padded item in float64: q / k / v [n, H dh], the module's own order of operations."""
    n = q.shape[0]
    q4, k4, v4 = (t.double().reshape(n, H, dh).transpose(0, 1) for t in (q, k, v))           # [H, n, dh]
    pos = p[center - (n - 1):center + n].double().reshape(2 * n - 1, H, dh).transpose(0, 1)   # row m = distance n - 1 - m
    ac = (q4 + u.double().reshape(H, 1, dh)) @ k4.transpose(1, 2)
    bd = rel_shift_literal((q4 + vb.double().reshape(H, 1, dh)) @ pos.transpose(1, 2))[:, :, :n]
    w = torch.softmax((ac + bd) * scale, -1)
    return (w @ v4).transpose(0, 1).reshape(n, H * dh)


REL_T = [1, 2, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 200, 255, 256, 257]   # the kernel's tiles: 32 keys / 32 queries per wave, 128 per block


@pytest.mark.parametrize("dh", [64, 128])
@pytest.mark.parametrize("T", REL_T)
def test_relpos_attention(dh, T):
    """max |got - want| / max |want| < 4e-6 per call (twice the 2e-6 of the f32 flash kernel in test_lm_kernels_gpu.py: the score is the sum of two
    dh-long contractions); rows at and beyond ``lens`` exactly zero; two calls bitwise equal.
    Measured on MI355X: the largest ratio over the 36 cases is 1.33e-6 (dh = 128, T = 64); 1.2e-6 at T = 255 for both head widths."""
    from mlx_audio_amd import ops

    H, B = 2, 3
    hd = H * dh
    g = torch.Generator().manual_seed(1000 * dh + T)
    P = 2 * T - 1 + 37
    center = T - 1 + 11   # off-centre, with slack on both sides
    p = torch.randn(P, hd, generator=g).to(DEV)
    u, vb = (0.5 * torch.randn(hd, generator=g)).to(DEV), (0.5 * torch.randn(hd, generator=g)).to(DEV)
    worst = 0.0
    for fused in (True, False):
        if fused:
            buf = torch.randn(B, T, 3 * hd, generator=g).to(DEV)
            q, k, v = buf[:, :, :hd], buf[:, :, hd:2 * hd], buf[:, :, 2 * hd:]
        else:
            q, k, v = (torch.randn(B, T, hd, generator=g).to(DEV) for _ in range(3))
        for lens in ([T, max(T // 2, 1), 1], None):
            ld = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
            out = torch.full((B, T, hd), float("nan"), device=DEV)
            ops.relpos_attention(q, k, v, p, u, vb, out, heads=H, dh=dh, center=center, lens=ld)
            out2 = torch.full((B, T, hd), float("nan"), device=DEV)
            ops.relpos_attention(q, k, v, p, u, vb, out2, heads=H, dh=dh, center=center, lens=ld)
            torch.cuda.synchronize()
            assert torch.equal(out, out2), "two calls on the same bytes differ"
            got = out.double().cpu()
            err = peak = 0.0
            for b in range(B):
                n = T if lens is None else lens[b]
                want = relpos_ref_item(q[b, :n].cpu(), k[b, :n].cpu(), v[b, :n].cpu(), p.cpu(), u.cpu(), vb.cpu(), center, H, dh, dh ** -0.5)
                err = max(err, float((got[b, :n] - want).abs().max()))
                peak = max(peak, float(want.abs().max()))
                assert not got[b, n:].any(), "rows beyond lens are not exactly zero"
            worst = max(worst, err / peak)
            assert err / peak < 4e-6, (fused, lens, err / peak)
    print(f"relpos_attention dh={dh} T={T}: worst max|err| / max|want| = {worst:.2e}")


def test_relpos_attention_refuses_a_short_table():
    from mlx_audio_amd import _lib, ops

    H, dh, T = 2, 64, 40
    q = torch.randn(1, T, H * dh, device=DEV)
    u = torch.zeros(H * dh, device=DEV)
    out = torch.full_like(q, 7.0)
    for P, center in ((2 * T - 1, T), (2 * T - 1, T - 2), (2 * T - 2, T - 1), (T, 0)):
        with pytest.raises(_lib.Mi355Error, match="position table"):
            ops.relpos_attention(q, q, q, torch.randn(P, H * dh, device=DEV), u, u, out, heads=H, dh=dh, center=center)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()), "a refused call wrote its output"
    with pytest.raises(_lib.Mi355Error, match="dh"):
        ops.relpos_attention(q, q, q, torch.randn(2 * T - 1, H * dh, device=DEV), u, u, out, heads=4, dh=32, center=T - 1)
    ops.relpos_attention(q, q, q, torch.randn(2 * T - 1, H * dh, device=DEV), u, u, out, heads=H, dh=dh, center=T - 1)   # the exact fit passes
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and not bool((out == 7.0).all())


# ---------------------------------------------------------------------------------------------------- glu_dwconv_silu
def _lens_for(B, L):
    base = [0, L, max(L // 2, 1), max(L - 1, 0), 1, min(17, L)]
    return [base[i % len(base)] for i in range(B)]


def _glu_ref(x, w, b, lens):
    """(y, sum_k |w g| + |b|, mask) in float64."""
    B, L, C2 = x.shape
    C, K = w.shape
    left = (K - 1) // 2
    xd, wd, bd = x.double().cpu(), w.double().cpu(), b.double().cpu()
    m = torch.ones(B, L, dtype=torch.float64) if lens is None else (torch.arange(L)[None, :] < lens.cpu()[:, None]).double()
    gt = xd[:, :, :C] * torch.sigmoid(xd[:, :, C:]) * m[:, :, None]
    xp = torch.zeros(B, L + K - 1, C, dtype=torch.float64)
    xp[:, left:left + L] = gt
    z, mag = bd.expand(B, L, C).clone(), bd.abs().expand(B, L, C).clone()
    for k in range(K):
        t = xp[:, k:k + L] * wd[:, k]
        z += t
        mag += t.abs()
    return z * torch.sigmoid(z) * m[:, :, None], mag, m


@pytest.mark.parametrize("C", [64, 128, 1024, 520])
@pytest.mark.parametrize("T", [1, 4, 5, 8, 9, 17, 250])
@pytest.mark.parametrize("K", [5, 9, 31])
def test_glu_dwconv_silu(C, T, K):
    """Bar per element, u = 2^-24: 2 (K + 8) u (sum_k |w g| + |b|) + 8 u |y| -- the K-term sum, a few ulp for each expf-based sigmoid, and
    |d silu / dz| <= 1.1; rows beyond ``lens`` exactly zero; two calls bitwise equal.
    Measured on MI355X: the largest error / bar ratio over the 84 cases is 0.153 (K = 5, where the bar is tightest)."""
    from mlx_audio_amd import ops

    B = 4
    worst = 0.0
    g = torch.Generator().manual_seed(C + 7 * T + 1000 * K)
    for lens in (_lens_for(B, T), None):
        x = torch.randn(B, T, 2 * C, generator=g).to(DEV)
        w = (torch.randn(C, K, generator=g) / K ** 0.5).to(DEV)
        b = (0.3 * torch.randn(C, generator=g)).to(DEV)
        ld = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
        y = torch.full((B, T, C), float("nan"), device=DEV)
        ops.glu_dwconv_silu(x, w, b, y, lens=ld)
        y2 = torch.full((B, T, C), float("nan"), device=DEV)
        ops.glu_dwconv_silu(x, w, b, y2, lens=ld)
        torch.cuda.synchronize()
        assert torch.equal(y, y2), "two calls on the same bytes differ"
        val, mag, m = _glu_ref(x, w, b, ld)
        err = (y.double().cpu() - val).abs()
        bound = 2 * (K + 8) * U * mag + 8 * U * val.abs()
        assert bool((err <= bound).all()), (lens, float((err / bound.clamp_min(1e-300)).max()))
        worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
        pad = m[:, :, None].expand_as(val) == 0
        assert not y.cpu()[pad].any(), "rows beyond lens are not exactly zero"
    print(f"glu_dwconv_silu C={C} T={T} K={K}: worst error / bound = {worst:.3f}")


def test_glu_dwconv_silu_refuses_bad_arguments():
    from mlx_audio_amd import _lib, ops

    x = torch.randn(1, 8, 128, device=DEV)
    y = torch.empty(1, 8, 64, device=DEV)
    with pytest.raises(_lib.Mi355Error, match="odd"):
        ops.glu_dwconv_silu(x, torch.randn(64, 4, device=DEV), None, y)
    with pytest.raises(_lib.Mi355Error, match="odd"):
        ops.glu_dwconv_silu(x, torch.randn(64, 33, device=DEV), None, y)
    with pytest.raises(_lib.Mi355Error, match="multiple of 4"):
        ops.glu_dwconv_silu(torch.randn(1, 8, 12, device=DEV), torch.randn(6, 3, device=DEV), None, torch.empty(1, 8, 6, device=DEV))


# ---------------------------------------------------------------------------------------------------- stencil2d_k3s2
def _stencil_ref(x, w, bias, relu, lens_in, lens_out):
    """(y, sum |w x| + |bias|) in float64 through conv2d on the zero-filled input."""
    B, T, F = x.shape[:3]
    C = w.shape[0]
    xd = x.double().cpu()
    if lens_in is not None:
        xd = xd * (torch.arange(T)[None, :] < lens_in.cpu()[:, None]).double().reshape(B, T, *([1] * (xd.dim() - 2)))
    xin = xd[:, None] if xd.dim() == 3 else xd.permute(0, 3, 1, 2)   # [B, 1 | C, T, F]
    wd = w.double().cpu()[:, None]                                   # [C, 1, 3, 3]
    groups = 1 if xd.dim() == 3 else C
    val = torch.nn.functional.conv2d(xin, wd, bias.double().cpu(), stride=2, padding=1, groups=groups)
    mag = torch.nn.functional.conv2d(xin.abs(), wd.abs(), bias.double().cpu().abs(), stride=2, padding=1, groups=groups)
    if relu:
        val = val.clamp_min(0)
    val, mag = val.permute(0, 2, 3, 1), mag.permute(0, 2, 3, 1)
    To = val.shape[1]
    m = torch.ones(B, To, dtype=torch.float64) if lens_out is None else (torch.arange(To)[None, :] < lens_out.cpu()[:, None]).double()
    return val * m[:, :, None, None], mag, m


@pytest.mark.parametrize("T", [1, 2, 3, 8, 9, 203])
@pytest.mark.parametrize("F", [1, 5, 16, 80])
@pytest.mark.parametrize("C", [32, 256])
def test_stencil2d_k3s2(T, F, C):
    """Bar per element: 2 (9 + 3) 2^-24 (sum |w x| + |bias|); output rows beyond ``lens_out`` exactly zero, input rows beyond ``lens_in`` read as
    zero; two calls bitwise equal.  Measured on MI355X: the largest error / bar ratio over the 48 cases is 0.183."""
    from mlx_audio_amd import ops

    B = 3
    To, Fo = (T - 1) // 2 + 1, (F - 1) // 2 + 1
    g = torch.Generator().manual_seed(T + 300 * F + C)
    worst = 0.0
    for depthwise in (False, True):
        for relu in (False, True):
            for lens in ([T, max(T // 2, 1), 1], None):
                x = torch.randn((B, T, F, C) if depthwise else (B, T, F), generator=g).to(DEV)
                w = (torch.randn(C, 3, 3, generator=g) / 3).to(DEV)
                bias = (0.3 * torch.randn(C, generator=g)).to(DEV)
                li = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
                lo = None if lens is None else torch.tensor([(n - 1) // 2 + 1 for n in lens], dtype=torch.int32, device=DEV)
                y = torch.full((B, To, Fo, C), float("nan"), device=DEV)
                ops.stencil2d_k3s2(x, w, bias, y, relu=relu, lens_in=li, lens_out=lo)
                y2 = torch.full((B, To, Fo, C), float("nan"), device=DEV)
                ops.stencil2d_k3s2(x, w, bias, y2, relu=relu, lens_in=li, lens_out=lo)
                torch.cuda.synchronize()
                assert torch.equal(y, y2), "two calls on the same bytes differ"
                val, mag, m = _stencil_ref(x, w, bias, relu, li, lo)
                err = (y.double().cpu() - val).abs()
                bound = 2 * (9 + 3) * U * mag
                assert bool((err <= bound).all()), (depthwise, relu, lens, float((err / bound.clamp_min(1e-300)).max()))
                worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
                pad = m[:, :, None, None].expand_as(val) == 0
                assert not y.cpu()[pad].any(), "rows beyond lens_out are not exactly zero"
    print(f"stencil2d_k3s2 T={T} F={F} C={C}: worst error / bound = {worst:.3f}")
