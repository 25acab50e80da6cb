"""``ops.shortconv`` (shortconv.hip) against the float64 statement of its contract (``_ref`` below).

Exact cases: integer inputs, weights, biases and states, taps +-2^-1 .. 2^1, two non-zero weights per C row.  ``_ref`` asserts every
intermediate (u, Bx, conv, y) below 2^24 units of 2^-2, so no product or addition rounds in any order and both forms must return the float64
result bit for bit.

Float cases: per element, u = 2^-24, on the same 16-bit-rounded weights.  For each slab e_u = (H + 8) u (|x| @ |w|^T + |b|) + split: H additions
a term can pass through (step: H / 32 FMAs of its lane, 3 shuffles, 2 wave sums; tile: 2 x 32 terms per MFMA step, H / 64 steps of its wave, the
join), the bias and slack; split (tile form only) = x - (its 16-bit images) <= 2^-22 |x| + 2^-25 in fp16 (hi + lo), 2^-24 |x| in bf16 (three images), times |w|.  Then through
the two products and the L taps: e_Bx = |B| e_x + |x| e_B + e_B e_x + u |Bx|, e_conv = sum |tap| e_z + (L + 1) u (sum |tap z| + |bias|),
e_y = |C| e_conv + |conv| e_C + e_C e_conv + u |y|."""
import pytest
import torch

from mlx_audio_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
U = 2.0 ** -24


def _ref(xn, w, taps, state_in, lens, in_bias, conv_bias, e_u=None):
    """float64 (y, state_out, largest |intermediate|); with ``e_u`` (the error of u): (y, state_out, (bound on y, bound on state_out))."""
    B, T, H = xn.shape
    L = taps.shape[1]
    u = xn.double() @ w.double().T + (0 if in_bias is None else in_bias.double())
    ub, uc, ux = u[..., :H], u[..., H:2 * H], u[..., 2 * H:]
    valid = (torch.arange(T)[None, :] < lens[:, None])[..., None]
    st = torch.zeros(B, L - 1, H, dtype=torch.float64) if state_in is None else state_in.double()
    z = torch.cat([st, ub * ux * valid], 1)
    cb = 0 if conv_bias is None else conv_bias.double()
    conv = sum(taps[:, j].double() * z[:, j:j + T] for j in range(L)) + cb
    y = uc * conv * valid
    so = torch.stack([z[b, int(lens[b]):int(lens[b]) + L - 1] for b in range(B)])
    big = max(float(v.abs().max()) for v in (u, z, conv, y))
    if e_u is None:
        return y, so, big
    eb, ec, ex = e_u[..., :H], e_u[..., H:2 * H], e_u[..., 2 * H:]
    ez = torch.cat([torch.zeros_like(st), (ub.abs() * ex + ux.abs() * eb + eb * ex + U * (ub * ux).abs()) * valid], 1)
    az = sum(taps[:, j].abs().double() * z[:, j:j + T].abs() for j in range(L)) + (0 if conv_bias is None else conv_bias.abs().double())
    econv = sum(taps[:, j].abs().double() * ez[:, j:j + T] for j in range(L)) + (L + 1) * U * az
    eso = torch.stack([ez[b, int(lens[b]):int(lens[b]) + L - 1] for b in range(B)])   # carried rows of state_in are copies: bound 0
    return y, so, ((uc.abs() * econv + conv.abs() * ec + ec * econv + U * y.abs()) * valid, eso)


def _run(xn, rw, taps, state_in, lens, in_bias, conv_bias):
    """Strided xn; y and state_out NaN-initialised inside sentinel guards, at addresses that are not 16-byte aligned; checks the guards."""
    B, T, H = xn.shape
    L = taps.shape[1]
    d = lambda t: None if t is None else t.to(DEV)
    xb = torch.full((B, T + 1, H + 4), 3.5, device=DEV)
    xb[:, :T, :H] = xn
    yb = torch.full((B, T, H + 9), 7.25, device=DEV)
    y = yb[:, :, 3:3 + H]
    y.fill_(float("nan"))
    n = B * (L - 1) * H
    sb = torch.full((n + 10,), 7.25, device=DEV)
    sb[3:3 + n] = float("nan")
    ops.shortconv(xb[:, :T, :H], rw, d(taps), y, state_in=d(state_in), state_out=sb[3:3 + n].view(B, L - 1, H), lens=d(lens), in_bias=d(in_bias),
                  conv_bias=d(conv_bias))
    assert bool((yb[:, :, :3] == 7.25).all()) and bool((yb[:, :, 3 + H:] == 7.25).all()) and bool((sb[:3] == 7.25).all()) and bool((sb[3 + n:] == 7.25).all())
    return y.cpu().clone(), sb[3:3 + n].view(B, L - 1, H).cpu().clone()


def _exact_inputs(H, L, B, T, seed):
    g = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()
    w = ri(-1, 1, 3 * H, H)
    wc = torch.zeros(H, H)
    wc.scatter_(1, torch.randint(0, H, (H, 2), generator=g), 1.0)
    w[H:2 * H] = wc * (1 - 2 * ri(0, 1, H, 1))
    taps = torch.pow(2.0, ri(-1, 1, H, L)) * (1 - 2 * ri(0, 1, H, L))
    return ri(-2, 2, B, T, H), w, taps, ri(-8, 8, B, L - 1, H), ri(-3, 3, 3 * H), ri(-4, 4, H)


ROWS = (1, 2, 8, 9, 15, 16, 17, 33)   # both sides of the form switch; the row-tile edge inside a block; a halo that crosses blocks


@pytest.mark.parametrize("H,L", [(H, L) for H in (64, 96, 160) for L in (2, 3, 4)])
def test_exact_cases_are_bit_equal(H, L):
    i = H + L
    xn, w, taps, st, ib, cb = _exact_inputs(H, L, 1, ROWS[-1], i)
    rw = ops.pack_rowmajor16(w, None, DEV, f16=bool(i & 1))
    for n, T in enumerate(ROWS):
        opt = (st if (n + i) & 1 else None, ib if (n + i) & 2 else None, cb if (n + i) & 4 else None)   # every operand present and absent in both forms
        lens = torch.tensor([T], dtype=torch.int32)
        y, so, big = _ref(xn[:, :T], w, taps, opt[0], lens, opt[1], opt[2])
        assert 4 * big < 2 ** 24   # the precondition of bit-equality (units of 2^-2)
        got = _run(xn[:, :T], rw, taps, opt[0], None, opt[1], opt[2])
        assert torch.equal(got[0].double(), y) and torch.equal(got[1].double(), so), (T, opt)
        again = _run(xn[:, :T], rw, taps, opt[0], None, opt[1], opt[2])
        assert torch.equal(got[0], again[0]) and torch.equal(got[1], again[1])


@pytest.mark.parametrize("H,L", [(64, 4), (96, 3), (160, 2)])
def test_ragged_batch_equals_its_items_alone_and_the_reference(H, L):
    T, lens = 17, torch.tensor([17, 5, 1, 0], dtype=torch.int32)
    xn, w, taps, st, ib, cb = _exact_inputs(H, L, 4, T, 7 * H + L)
    rw = ops.pack_rowmajor16(w, None, DEV)
    y, so, big = _ref(xn, w, taps, st, lens, ib, cb)
    assert 4 * big < 2 ** 24
    gy, gs = _run(xn, rw, taps, st, lens, ib, cb)
    assert torch.equal(gy.double(), y) and torch.equal(gs.double(), so)   # rows past lens are exact zeros (the reference's are), NaN nowhere
    assert bool((gy[1, 5:] == 0).all()) and bool((gy[3] == 0).all()) and torch.equal(gs[3], st[3]) and torch.equal(gs[2, :L - 2], st[2, 1:])
    for b, n in enumerate(lens.tolist()[:3]):
        ay, as_ = _run(xn[b:b + 1, :n], rw, taps, st[b:b + 1], None, ib, cb)
        assert torch.equal(ay[0], gy[b, :n]) and torch.equal(as_[0], gs[b]), b


@pytest.mark.parametrize("H,L,f16", [(64, 3, False), (160, 4, True)])
def test_one_call_equals_prefill_plus_steps_through_the_carried_state(H, L, f16):
    xn, w, taps, st, ib, cb = _exact_inputs(H, L, 1, 17, H * L)
    rw = ops.pack_rowmajor16(w, None, DEV, f16=f16)
    y, s = _run(xn, rw, taps, st, None, ib, cb)                     # tile form
    y15, s15 = _run(xn[:, :15], rw, taps, st, None, ib, cb)          # tile form, then two runs of the step form
    y16, s16 = _run(xn[:, 15:16], rw, taps, s15, None, ib, cb)
    y17, s17 = _run(xn[:, 16:17], rw, taps, s16, None, ib, cb)
    assert torch.equal(torch.cat([y15, y16, y17], 1), y) and torch.equal(s17, s)


WORST = {}   # form -> largest error / bound seen (printed: the docs/COVERAGE.md row quotes the MI355X figures)


@pytest.mark.parametrize("H,L,B,T,f16", [(256, 3, 1, 1, False), (256, 4, 2, 4, True), (256, 3, 2, 33, False), (256, 2, 1, 17, True), (2048, 3, 1, 9, False),
                                         (2048, 3, 1, 8, True)])
def test_float_cases_stay_within_the_derived_bound(H, L, B, T, f16):
    g = torch.Generator().manual_seed(H + L + T)
    xn, taps, st = torch.randn(B, T, H, generator=g), torch.randn(H, L, generator=g) / L ** 0.5, torch.randn(B, L - 1, H, generator=g)
    ib, cb = 0.1 * torch.randn(3 * H, generator=g), 0.1 * torch.randn(H, generator=g)
    w = (torch.randn(3 * H, H, generator=g) / H ** 0.5).to(torch.float16 if f16 else torch.bfloat16).float()
    lens = torch.tensor([T, max(T - 3, 0)][:B], dtype=torch.int32)
    tile = B * T > 8
    split = ((2.0 ** -22 * xn.double().abs() + 2.0 ** -25) if f16 else 2.0 ** -24 * xn.double().abs()) @ w.double().abs().T
    e_u = (H + 8) * U * (xn.double().abs() @ w.double().abs().T + ib.double().abs()) + (split if tile else 0)
    y, so, (bound, sbound) = _ref(xn, w, taps, st, lens, ib, cb, e_u)
    gy, gs = _run(xn, ops.pack_rowmajor16(w, None, DEV, f16=f16), taps, st, lens, ib, cb)
    err = (gy.double() - y).abs()
    assert bool((err <= bound).all()) and bool((gy[1, int(lens[1]):] == 0).all() if B > 1 else True)
    ratio = float((err / bound.clamp_min(1e-300)).max())
    form = "tile" if tile else "step"
    WORST[form] = max(WORST.get(form, 0.0), ratio)
    print(f"shortconv {form} H={H} L={L} B={B} T={T} f16={f16}: error / bound = {ratio:.4f} (worst so far {WORST[form]:.4f})")
    assert bool(((gs.double() - so).abs() <= sbound).all())


def test_refusals_name_the_reason_and_leave_the_outputs_untouched():
    H = 64
    xn, w, taps, st, ib, cb = _exact_inputs(H, 3, 1, 4, 1)
    rw = ops.pack_rowmajor16(w, None, DEV)
    fp8 = ops.pack_rowmajor_fp8(w, None, DEV)[0]
    x, wide = xn.to(DEV), torch.zeros(1, 4, H + 4, device=DEV)
    y, s_in, s_out = torch.full((1, 4, H), 9.0, device=DEV), st.to(DEV), torch.full((1, 2, H), 9.0, device=DEV)
    t = lambda L: torch.ones(H, L, device=DEV)
    cases = [(dict(taps=t(5), state_in=None, state_out=torch.full((1, 4, H), 9.0, device=DEV)), "L = 5 is not built", -3),
             (dict(state_in=s_out), "must be different buffers", -1),
             (dict(xn=wide[:, :, 1:1 + H]), "16-byte aligned", -1),
             (dict(w_in=fp8), "quantised weights are not built", -3)]
    for over, text, rc in cases:
        kw = dict(xn=x, w_in=rw, taps=t(3), state_in=s_in, state_out=s_out)
        kw.update(over)
        with pytest.raises(_lib.Mi355Error, match=text) as e:
            ops.shortconv(kw.pop("xn"), kw.pop("w_in"), kw.pop("taps"), y, **kw)
        assert f"({rc})" in str(e.value) and bool((y == 9.0).all()) and bool((kw["state_out"] == 9.0).all())
    w48 = ops.pack_rowmajor16(torch.ones(144, 48), None, DEV)
    y48 = torch.full((1, 1, 48), 9.0, device=DEV)
    with pytest.raises(_lib.Mi355Error, match="H = 48 is not a multiple of 32"):
        ops.shortconv(torch.zeros(1, 1, 48, device=DEV), w48, torch.ones(48, 3, device=DEV), y48, state_in=None, state_out=torch.zeros(1, 2, 48, device=DEV))
    assert bool((y48 == 9.0).all())
    with pytest.raises(NotImplementedError, match="quantised weights are not built"):
        ops.shortconv(x, ops.QuantizedLinear(None, None, None, 3 * H, H, 4, 64), t(3), y, state_in=s_in, state_out=s_out)
