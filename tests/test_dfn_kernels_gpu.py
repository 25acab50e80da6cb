"""``csrc/dfn.hip`` against float64 on the host (``tests/_ops_emu_dfn.py``): ``dfn_features``, ``dfn_conv2d`` and ``dfn_apply``.  The bars are float32 rounding
bounds (u = 2^-24), derived in the docstrings and not tuned; the measured maxima are written next to them."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _ops_emu_dfn as E  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
ALPHA, OMA = float(np.float32(0.99)), float(np.float32(1.0 - 0.99))
RATIOS = {}


def _note(name, ratio):
    RATIOS[name] = max(RATIOS.get(name, 0.0), ratio)
    print(f"{name}: error / bar = {ratio:.3f} (largest so far {RATIOS[name]:.3f})")


def _dev(t):
    return None if t is None else t.to(DEV)


def _widths(F, nb):
    from mlx_audio_amd.sts.models.deepfilternet.model import default_erb_widths
    return default_erb_widths(F, nb)


# ---------------------------------------------------------------------------------------------------------------- dfn_features
@pytest.mark.parametrize("form", ["fb", "widths"])
@pytest.mark.parametrize("with_lens", [True, False])
@pytest.mark.parametrize("la", [0, 2])
@pytest.mark.parametrize("T", [1, 2, 3, 50])
@pytest.mark.parametrize("F,nb_erb,nb_df", [(481, 32, 96), (241, 16, 48)])
def test_dfn_features(F, nb_erb, nb_df, T, la, with_lens, form):
    """Bars, per element, with x the dB value of a band (|x| <= 100) and a the running-mean coefficient:
      * spec_out: one product, 2 u |v|;
      * band energy: a sum of at most F non-negative products, relative error (F + 3) u, so the dB value is off by dx = (10 / ln 10)(F + 3) u + 4 u 100
        (log10f to 2 ulp of a value below 100); the state obeys d_t <= a d_{t-1} + (1 - a) dx + 3 u max(|x|, |state|) (two products and a sum per
        step), so d <= dx + 3 u 100 / (1 - a), and the feature (x - state) / 40 is off by (2 dx + 3 u 100 / (1 - a)) / 40 + 2 u |feat|;
      * DF feature: |spec| to 3 u relative, its state likewise to ds = 3 u smax / (1 - a) + 3 u smax (smax = the largest magnitude or state of the
        bin), and re / sqrt(state) to (ds / (2 smin) + 4 u) |feat| with smin the bin's smallest state.
    Measured on MI355X over all 64 cases: largest error / bar 0.026 (feat_erb), 0.024 (feat_df), 0.67 (spec_out).
    A stretch of exact zeros (frames 20..29 of item 0 at T = 50), ``lens`` below T and at most the look-ahead (the shift is then skipped)."""
    from mlx_audio_amd import ops

    B = 3
    g = torch.Generator().manual_seed(F + 7 * T + la)
    wnorm = 1.0 / (960 * 960 / 960.0)
    spec = torch.randn(B, T, F, 2, generator=g) * (torch.rand(B, T, 1, 1, generator=g) * 3 + 0.2)
    if T == 50:
        spec[0, 20:30] = 0.0
    lens = [T, min(T, 2), max(1, T - 1)] if with_lens else None
    widths = _widths(F, nb_erb)
    from mlx_audio_amd.sts.models.deepfilternet.model import erb_filterbanks
    fb = erb_filterbanks(widths, F)[0] if form == "fb" else None
    start = torch.tensor(np.concatenate([[0], np.cumsum(widths)]), dtype=torch.int32) if form == "widths" else None
    kw = dict(wnorm=wnorm, alpha=ALPHA, one_minus_alpha=OMA, nb_erb=nb_erb, nb_df=nb_df, lookahead=la)
    ref_s, ref_e, ref_d = E.dfn_features(spec, erb_fb=fb, erb_start=start, lens=lens, **kw)
    lens_d = torch.tensor(lens, dtype=torch.int32, device=DEV) if with_lens else None
    outs = [ops.dfn_features(spec.to(DEV), erb_fb=_dev(fb), erb_start=_dev(start), lens=lens_d, **kw) for _ in range(2)]
    torch.cuda.synchronize()
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    s, fe, fd = (t.cpu() for t in outs[0])
    assert fe.shape == (B, T, nb_erb, 1) and fd.shape == (B, T, nb_df, 2)
    _note("features.spec_out", float(((s.double() - ref_s.double()).abs() / (3 * U * ref_s.double().abs() + 1e-300)).max()))
    assert torch.all((s.double() - ref_s.double()).abs() <= 3 * U * ref_s.double().abs())          # 2 u + the float32 store of the reference
    dx = 10 / math.log(10) * (F + 3) * U + 4 * U * 100
    bar_e = (2 * dx + 3 * U * 100 / (1 - ALPHA)) / 40 + 3 * U * ref_e.double().abs()
    err_e = (fe.double() - ref_e.double()).abs()
    _note("features.feat_erb", float((err_e / bar_e).max()))
    assert torch.all(err_e <= bar_e)
    # the bin's state range, from the float64 recurrence
    for b in range(B):
        n = T if lens is None else lens[b]
        shift = la if n > la else 0
        mag = torch.sqrt((ref_s[b, :n, :nb_df].double() ** 2).sum(-1))
        st = torch.linspace(0.001, 0.0001, nb_df, dtype=torch.float64)
        smin, smax = st.clone(), torch.maximum(st, mag.max(0).values if n else st)
        for t in range(n):
            st = mag[t] * OMA + st * ALPHA
            smin = torch.minimum(smin, st)
        ds = 3 * U * smax / (1 - ALPHA) + 3 * U * smax
        rel = ds / (2 * smin) + 5 * U
        err = (fd[b, :n - shift].double() - ref_d[b, :n - shift].double()).abs()
        bar = rel[None, :, None] * ref_d[b, :n - shift].double().abs() + 1e-30
        if n - shift > 0:
            _note("features.feat_df", float((err / bar).max()))
            assert torch.all(err <= bar), b
        assert not fe[b, n - shift:].any() and not fd[b, n - shift:].any() and not s[b, n:].any()   # behind the shift and behind lens: zeros


# ---------------------------------------------------------------------------------------------------------------- dfn_conv2d
def _geometries(C):
    """(name, F, cin, cmid, cout, groups, (kt, kf), fstride, transposed, pointwise, act, add, lookahead) -- every block geometry of the model, and two
    with frames of look-ahead inside the conv (``ConvBlock``'s ``lookahead``, which the model's own blocks leave at 0)."""
    O2 = 10
    return [
        ("inp_dense_3x3_from_1", 32, 1, C, C, 1, (3, 3), 1, False, False, 1, False, 0),
        ("inp_grouped_3x3_from_2", 96, 2, C, C, 2, (3, 3), 1, False, True, 1, False, 0),
        ("dw_1x3_s1", 8, C, C, C, C, (1, 3), 1, False, True, 1, False, 0),
        ("dw_1x3_s2_32", 32, C, C, C, C, (1, 3), 2, False, True, 1, False, 0),
        ("dw_1x3_s2_16", 16, C, C, C, C, (1, 3), 2, False, True, 1, False, 0),
        ("dw_1x3_s2_96", 96, C, C, C, C, (1, 3), 2, False, True, 1, False, 0),
        ("dwT_1x3_s2_8", 8, C, C, C, C, (1, 3), 2, True, True, 1, False, 0),
        ("pathway_1x1_add", 16, C, C, C, C, (1, 1), 1, False, False, 1, True, 0),
        ("df_pathway_5x1", 96, C, O2, O2, math.gcd(C, O2), (5, 1), 1, False, True, 1, False, 0),
        ("out_to_1_sigmoid", 32, C, 1, 1, 1, (1, 3), 1, False, False, 2, False, 0),
        ("inp_dense_3x3_lookahead_1", 32, 1, C, C, 1, (3, 3), 1, False, False, 1, False, 1),
        ("df_pathway_5x1_lookahead_2", 96, C, O2, O2, math.gcd(C, O2), (5, 1), 1, False, True, 0, False, 2),
    ]


@pytest.mark.parametrize("with_lens", [True, False])
@pytest.mark.parametrize("T", [1, 2, 7])
@pytest.mark.parametrize("C", [16, 8])
@pytest.mark.parametrize("gi", range(12))
def test_dfn_conv2d(gi, C, T, with_lens):
    """Bar per element: with n1 = (Cin / groups) kt kf terms in the conv and Cmid in the pointwise conv, a float32 sum of n terms is off by at most
    n u sum|terms|, so the value before the activation is off by (n1 + Cmid + 4) u (|pw| conv(|x|, |w|) |scale| + |shift|); ReLU and the sigmoid are
    1-Lipschitz (+ 2 u for expf and the division), the skip sum adds u |y|: bar = (n1 + Cmid + 8) u (|pw| conv(|x|, |w|) |scale| + |shift| + |add| + 1).
    Measured on MI355X over all 144 cases: largest error / bar 0.14 (the depthwise stride-2 block at F = 96).  Frames at and beyond ``lens`` are exactly zero; two runs give the same bits."""
    from mlx_audio_amd import ops

    name, F, cin, cmid, cout, groups, (kt, kf), fstride, transposed, has_pw, act, has_add, look = _geometries(C)[gi]
    B = 2
    g = torch.Generator().manual_seed(100 * gi + C + T)
    r = lambda *s: torch.randn(*s, generator=g)
    x = r(B, T, F, cin)
    w = r(cin, cmid // groups, kt, kf) if transposed else r(cmid, cin // groups, kt, kf)
    w = w / math.sqrt(max(1, (cin // groups) * kt * kf))
    pw = r(cout, cmid) / math.sqrt(cmid) if has_pw else None
    scale, shift = 1 + 0.2 * r(cout), 0.3 * r(cout)
    lens = [T, T // 2] if with_lens else None
    mk = lambda w_, pw_, sc, sh, a: ops.DfnConv(w=w_, cin=cin, cmid=cmid, cout=cout, groups=groups, kt=kt, kf=kf, fstride=fstride, transposed=transposed,
                                                 lookahead=look, pw=pw_, scale=sc, shift=sh, act=a)
    Fo = ops.dfn_conv2d_fo(F, kf, fstride, transposed)
    add = r(B, T, Fo, cout) if has_add else None
    ref = E.dfn_conv2d(x, mk(w, pw, scale, shift, act), add=add, lens=lens).double()
    mag = E.dfn_conv2d(x.abs(), mk(w.abs(), None if pw is None else pw.abs(), scale.abs(), shift.abs(), 0), add=None if add is None else add.abs(), lens=lens).double()
    n1 = (cin // groups) * kt * kf
    bar = (n1 + cmid + 8) * U * (mag + 1.0)
    cv = mk(_dev(w), _dev(pw), _dev(scale), _dev(shift), act)
    lens_d = torch.tensor(lens, dtype=torch.int32, device=DEV) if with_lens else None
    ys = [ops.dfn_conv2d(x.to(DEV), cv, add=_dev(add), lens=lens_d) for _ in range(2)]
    torch.cuda.synchronize()
    assert torch.equal(ys[0], ys[1])
    y = ys[0].cpu()
    assert y.shape == (B, T, Fo, cout) == ref.shape
    err = (y.double() - ref).abs()
    _note(f"conv2d.{name}", float((err / bar).max()))
    assert torch.all(err <= bar)
    assert float(ref.abs().max()) > 0.05
    if with_lens:
        assert not y[1, T // 2:].any()


# ---------------------------------------------------------------------------------------------------------------- dfn_apply
@pytest.mark.parametrize("with_lens", [True, False])
@pytest.mark.parametrize("mask_first", [False, True])
@pytest.mark.parametrize("la", [0, 2])
@pytest.mark.parametrize("T", [1, 4, 9])
@pytest.mark.parametrize("F,nb_erb,nb_df", [(481, 32, 96), (241, 16, 48)])
def test_dfn_apply(F, nb_erb, nb_df, T, la, mask_first, with_lens):
    """Bar per complex component: the gain is a sum of E products ((E + 1) u sum|m fb|), a filter tap is a complex product (two products and a sum per
    component) of a spectrum value that may carry the gain, accumulated over ``order`` taps, then one division: (E + 3 order + 8) u
    sum_k (|re| + |im|)(|cr| + |ci|) gmag / wnorm with gmag = sum_e |m fb| (1 where the filter sees the unmasked spectrum); bins at and beyond nb_df:
    (E + 8) u (|re| + |im|) gmag / wnorm.  Measured on MI355X over all 48 cases: largest error / bar 0.07.
    T = 1 and 4 lie below the order (5); bins at and beyond nb_df do not depend on the coefficients (bit for bit)."""
    from mlx_audio_amd import ops
    from mlx_audio_amd.sts.models.deepfilternet.model import erb_filterbanks

    B, order = 3, 5
    g = torch.Generator().manual_seed(F + T + 10 * la + mask_first)
    wnorm = 1.0 / 960.0
    spec = torch.randn(B, T, F, 2, generator=g) * 1e-3
    m = torch.rand(B, T, nb_erb, generator=g)
    inv = erb_filterbanks(_widths(F, nb_erb), F)[1]
    coef = torch.randn(B, T, nb_df, order, 2, generator=g) * 0.5
    lens = [T, 1, max(1, T - 2)] if with_lens else None
    kw = dict(order=order, df_lookahead=la, mask_first=mask_first, wnorm=wnorm)
    ref = torch.view_as_real(E.dfn_apply64(spec, m, inv, coef, lens=lens, **kw))
    mag = E.dfn_apply64(torch.stack([spec.abs().sum(-1), torch.zeros(B, T, F)], -1), m, inv, torch.stack([coef.abs().sum(-1), torch.zeros(B, T, nb_df, order)], -1),
                        lens=lens, **kw).real
    bar = ((nb_erb + 3 * order + 8) * U * mag + 1e-30)[..., None]
    lens_d = torch.tensor(lens, dtype=torch.int32, device=DEV) if with_lens else None
    run = lambda c: ops.dfn_apply(spec.to(DEV), m.to(DEV), inv.to(DEV), c.to(DEV), lens=lens_d, **kw)
    a, b, other = run(coef), run(coef), run(coef * -0.7 + 0.1)
    torch.cuda.synchronize()
    assert a.dtype == torch.complex64 and a.shape == (B, T, F) and torch.equal(torch.view_as_real(a), torch.view_as_real(b))
    got = torch.view_as_real(a).cpu().double()
    err = (got - ref).abs()
    _note("apply", float((err / bar).max()))
    assert torch.all(err <= bar)
    assert torch.equal(torch.view_as_real(a)[:, :, nb_df:], torch.view_as_real(other)[:, :, nb_df:])
    assert not torch.equal(torch.view_as_real(a)[:, :, :nb_df], torch.view_as_real(other)[:, :, :nb_df])
    if with_lens:
        assert not got[1, 1:].any() and not got[2, max(1, T - 2):].any()

