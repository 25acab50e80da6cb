"""The one-group GroupNorm kernels (csrc/group_norm.hip: statistics -> coefficients -> apply) against float64 numpy / torch on the host."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    from mlx_audio_amd import ops as _ops

    _ops.require_gpu()
    return _ops


def rel_err(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def host_coef(x, lens, w, b, eps=1e-5):
    """float64: per sample (mean, rstd), scale [B, C], shift [B, C] over the valid rows."""
    out = []
    for i in range(x.shape[0]):
        v = x[i, :int(lens[i])].double().cpu()
        mean, var = v.mean(), v.var(unbiased=False)
        rstd = 1.0 / torch.sqrt(var + eps)
        sc = w.double().cpu() * rstd
        out.append((mean, rstd, sc, b.double().cpu() - mean * sc))
    return out


def run_case(ops, x, lens_t, w, b, coef_bar, val_bar, what):
    B, L, C = x.shape
    lens = [L] * B if lens_t is None else lens_t.tolist()
    parts = ops.group_norm_stats(x, lens_t)
    sc, sh, mr = ops.group_norm_coef(parts, L, C, w, b, lens=lens_t, rep=2, return_stats=True)
    y = torch.full((B, L, C), float("nan"), device=DEV)
    ops.group_norm_apply(x, (sc, sh), y)
    torch.cuda.synchronize()
    assert sc.shape == sh.shape == (B, (2 * C + 31) // 32 * 32)
    worst = [0.0, 0.0, 0.0]
    for i, (mean, rstd, wsc, wsh) in enumerate(host_coef(x, lens, w, b)):
        for q in range(2):   # the row repeated `rep` times, the padding columns zero
            worst[0] = max(worst[0], rel_err(sc[i, q * C:(q + 1) * C], wsc))
            worst[1] = max(worst[1], rel_err(sh[i, q * C:(q + 1) * C], wsh))
        assert float(sc[i, 2 * C:].abs().max() if sc.shape[1] > 2 * C else 0.0) == 0.0
        assert abs(float(mr[i, 0]) - float(mean)) <= 2e-6 * max(abs(float(mean)), 1.0 / float(rstd)) and abs(float(mr[i, 1]) / float(rstd) - 1) < 2e-6
        n = lens[i]
        want = x[i, :n].double().cpu() * wsc + wsh
        worst[2] = max(worst[2], float((y[i, :n].cpu().double() - want).abs().max() / max(1.0, float(w.abs().max()))))
    print(f"group_norm {what}: scale {worst[0]:.2e} shift {worst[1]:.2e} (bar {coef_bar:.0e}), normalised values {worst[2]:.2e} (bar {val_bar:.0e})")
    assert worst[0] < coef_bar and worst[1] < coef_bar and worst[2] < val_bar, worst
    return sc, sh, y


@pytest.mark.parametrize("B,L,C,ragged", [(1, 48000, 32, False), (3, 150, 512, False), (2, 9601, 2, False), (4, 777, 24, True)])
def test_group_norm_stats_coef_apply_vs_float64(ops, B, L, C, ragged):
    """Direct pass: coefficients within 2e-6 (relative), normalised unit-variance values within 2e-5 (absolute) -- the instance-norm kernels' bars."""
    g = torch.Generator().manual_seed(L + C)
    x = (torch.randn(B, L, C, generator=g) * (0.5 + torch.rand(B, 1, 1, generator=g)) + torch.randn(B, 1, 1, generator=g)).to(DEV)
    w = (1 + 0.2 * torch.randn(C, generator=g)).to(DEV)
    b = (0.1 * torch.randn(C, generator=g)).to(DEV)
    lens = torch.tensor([777, 1, 400, 65], dtype=torch.int32, device=DEV) if ragged else None
    run_case(ops, x, lens, w, b, 2e-6, 2e-5, f"[{B}, {L}, {C}]{' ragged' if ragged else ''}")


def test_group_norm_large_mean(ops):
    """mean = 100 x std: the block-centred float64 merge keeps the direct pass's bars; the naive fp32 E[x^2] - E[x]^2 is off by ~1e-3 here."""
    g = torch.Generator().manual_seed(5)
    B, L, C = 2, 20000, 32
    x = (100.0 + torch.randn(B, L, C, generator=g)).to(DEV)
    w, b = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
    run_case(ops, x, None, w, b, 2e-6, 2e-5, "mean = 100 std")
    xf = x[0].cpu().float().reshape(-1)
    naive = float((xf * xf).mean() - xf.mean() ** 2)
    exact = float(x[0].double().var(unbiased=False))
    print(f"naive fp32 variance {naive:.6f} vs {exact:.6f}")
    assert abs(naive / exact - 1) > 1e-4   # the case has teeth


def test_group_norm_strided_views_and_two_operand_apply(ops):
    """Row offset (the transposed conv's trim), a batch-strided input view, the two-operand sum and the raw second operand; an unaligned channel count."""
    g = torch.Generator().manual_seed(9)
    for C in (16, 6):
        B, Lf, off, L = 3, 210, 3, 200
        a, c = torch.randn(B, Lf, C, generator=g).to(DEV), torch.randn(B, L, C, generator=g).to(DEV)
        wa, ba = torch.randn(C, generator=g).to(DEV), torch.randn(C, generator=g).to(DEV)
        ca = ops.group_norm_coef(ops.group_norm_stats(a), Lf, C, wa, ba)
        cc = ops.group_norm_coef(ops.group_norm_stats(c), L, C, None, None)
        y2, y1 = torch.empty(B, L, C, device=DEV), torch.empty(B, L, C, device=DEV)
        ops.group_norm_apply(a, ca, y2, c, cc, row_off0=off)
        ops.group_norm_apply(a[:, off:off + L], ca, y1, c)
        # statistics of a view [B, L, C] inside the larger tensor (ldx == C, batch stride Lf * C)
        cv = ops.group_norm_coef(ops.group_norm_stats(a[:, off:off + L]), L, C, wa, ba)
        torch.cuda.synchronize()
        ha, hc = host_coef(a, [Lf] * B, wa, ba), host_coef(c, [L] * B, torch.ones(C), torch.zeros(C))
        hv = host_coef(a[:, off:off + L], [L] * B, wa, ba)
        for i in range(B):
            na = a[i, off:off + L].double().cpu() * ha[i][2] + ha[i][3]
            nc = c[i].double().cpu() * hc[i][2] + hc[i][3]
            assert float((y2[i].cpu().double() - (na + nc)).abs().max()) < 5e-5 * float(wa.abs().max() + 1)
            assert float((y1[i].cpu().double() - (na + c[i].double().cpu())).abs().max()) < 5e-5 * float(wa.abs().max() + 1)
            assert rel_err(cv[0][i, :C], hv[i][2]) < 2e-6 and rel_err(cv[1][i, :C], hv[i][3]) < 2e-6


@pytest.mark.parametrize("tile", [128128, 6128128])
def test_group_norm_coef_from_conv_partials(ops, tile):
    """Coefficients from the ``stats_partial`` buffer a real conv launch wrote (merged over row blocks AND channels) equal those of the direct pass over
    the stored output and float64 on the host, to the bar the instance-norm partials are held to (2e-5); ragged batch, mean >> std."""
    g = torch.Generator().manual_seed(21)
    B, L, C, K = 3, 700, 128, 3
    lens = torch.tensor([700, 65, 333], dtype=torch.int32).to(DEV)
    w = (torch.randn(C, K, C, generator=g) / math.sqrt(K * C)).to(torch.bfloat16).float()
    bias = torch.randn(C, generator=g) * 0.1 + 7.0
    x = torch.randn(B, L, C, generator=g).to(DEV)
    pc = ops.pack_conv(w, bias, DEV)
    y = torch.zeros(B, L, C, device=DEV)
    st = ops.new_stats(B, L, C, DEV)
    st.fill_(float("nan"))
    ops.conv_gemm(x, pc, y, pad=1, lens_in=lens, lens_out=lens, tile=tile, stats=st)
    gw, gb = (1 + 0.2 * torch.randn(C, generator=g)).to(DEV), (0.1 * torch.randn(C, generator=g)).to(DEV)
    sc, sh = ops.group_norm_coef(st, L, C, gw, gb, lens=lens)
    sc_d, sh_d = ops.group_norm_coef(ops.group_norm_stats(y, lens), L, C, gw, gb, lens=lens)
    torch.cuda.synchronize()
    assert torch.isfinite(sc).all() and torch.isfinite(sh).all()
    e = (rel_err(sc[:, :C], sc_d[:, :C]), rel_err(sh[:, :C], sh_d[:, :C]))
    print(f"group_norm coefficients from conv partials (tile {tile}) vs the direct pass: scale {e[0]:.2e} shift {e[1]:.2e}")
    assert max(e) < 2e-5, e
    for i, (_, _, wsc, wsh) in enumerate(host_coef(y, lens.tolist(), gw, gb)):
        assert rel_err(sc[i, :C], wsc) < 2e-5 and rel_err(sh[i, :C], wsh) < 2e-5
        assert rel_err(sc_d[i, :C], wsc) < 2e-6 and rel_err(sh_d[i, :C], wsh) < 2e-6


def test_group_norm_identical_samples_repeatable(ops):
    """B identical samples in one batch, twice in a row: every sample carries the same partials, coefficients and outputs, bit for bit, run after run."""
    g = torch.Generator().manual_seed(3)
    for B, L, C in ((8, 5000, 32), (16, 333, 6)):
        x = torch.randn(1, L, C, generator=g).expand(B, -1, -1).contiguous().to(DEV)
        w, b = torch.randn(C, generator=g).to(DEV), torch.randn(C, generator=g).to(DEV)
        first = None
        for rep in range(3):
            parts = ops.group_norm_stats(x)
            sc, sh = ops.group_norm_coef(parts, L, C, w, b)
            y = torch.zeros(B, L, C, device=DEV)
            ops.group_norm_apply(x, (sc, sh), y, x, (sc, sh))
            torch.cuda.synchronize()
            for t in (parts, sc, sh, y):
                assert torch.equal(t, t[0:1].expand_as(t)), (B, L, C, rep)
            if first is None:
                first = (parts.clone(), sc.clone(), sh.clone(), y.clone())
            else:
                assert all(torch.equal(a, b_) for a, b_ in zip(first, (parts, sc, sh, y))), rep


def test_group_norm_argument_checks(ops):
    from mlx_audio_amd import _lib

    x = torch.zeros(1, 8, 4, device=DEV)
    parts = ops.group_norm_stats(x)
    with pytest.raises(_lib.Mi355Error, match="rep"):
        _lib.call_struct("mi355_group_norm_coef", "mi355_group_norm_coef_args", None, partials=parts.data_ptr(), partials_bstride=2, C=4, L=8, B=1, rep=3,
                         scale=x.data_ptr(), shift=x.data_ptr(), out_ld=8)
