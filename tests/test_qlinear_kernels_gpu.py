"""``ops.qlinear`` / ``ops.dequantize_affine`` (qlinear.hip) against plain float64 torch on the dequantised weights float64(scale) * q + float64(zero).

Exact cases: x = small integers times a power of two per row, scales = +-2^-2 .. 2^0, zeros = integer multiples of the scale, random codes.  Every
term of every partial sum is then a multiple of 2^(e_row - 2), so with sum_groups(|scale| sum|x q| + |zero| sum|x|) below 2^24 of those units (asserted
from the float64 side) no addition rounds, in any order: both forms must return the float64 result bit for bit.

Float cases: the bound is derived, per element, on B = sum_groups(|scale| sum|x q| + |zero| sum|x|) -- NOT on sum|x||w|: with zero ~ -scale * 2^(bits - 1)
the two terms cancel and a bound in |w| would be missed for no fault of the kernel.  u = 2^-24:
  accumulation  depth * u * B, depth = the additions a term can pass through.  Stream: g FMAs of its group, ceil(groups / 32) folds of its lane,
                3 shuffles, 2 wave sums, the fold's product and add, the store: g + ceil(groups / 32) + 8.  Tile: g / 32 steps x (hi, lo) MFMAs of
                32 terms each (counted as 2 g sequential additions), groups / 4 folds of its wave, the same tail: 2 g + ceil(groups / 4) + 8
  split         tile form only: x - (hi + lo) <= 2^-22 |x| while lo is a normal fp16, 2^-25 absolute below: sum_k (2^-22 |x_k| + 2^-25) |scale| q_k
"""
import pytest
import torch

from mlx_audio_amd import ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
NS, MS = (1, 15, 16, 17, 33), (1, 2, 4, 5, 8, 9, 16, 17, 33, 65)
SZ_DTYPES = (torch.float16, torch.bfloat16, torch.float32)
U = 2.0 ** -24


def _image(codes, scale, zero, bits, g, dt, bias=None):
    return ops.pack_quantized(ops.pack_codes(codes, bits), scale.to(dt), zero.to(dt), bias, DEV, group_size=g, bits=bits)


def _rows(ql, n):
    """The image of the first n output columns (leading rows of the packed words and of the pairs)."""
    return ops.QuantizedLinear(ql.q[:n], ql.sz[:n], None if ql.bias is None else ql.bias[:n], n, ql.k, ql.bits, ql.group_size)


def _run(x, ql, **kw):
    """Strided x and y, y NaN-initialised inside sentinel guards (and at an address that is not 16-byte aligned); returns y after checking the guards."""
    M, K = x.shape
    xb = torch.full((M, K + 4), 3.5, device=DEV)
    xb[:, :K] = x
    n_y = ql.n - (kw["y2"].shape[1] if kw.get("y2") is not None else 0)
    yb = torch.full((M, n_y + 9), 7.25, device=DEV)
    y = yb[:, 3:3 + n_y]
    y.fill_(float("nan"))
    ops.qlinear(xb[:, :K], ql, y, **kw)
    assert bool((yb[:, :3] == 7.25).all()) and bool((yb[:, 3 + n_y:] == 7.25).all())
    return y.clone()


def _terms(x, codes, scale, zero, g):
    """float64: the reference x @ w^T and B = sum_groups(|scale| sum|x q| + |zero| sum|x|), both [M, N]."""
    s, z, q, xd = scale.double().repeat_interleave(g, 1), zero.double().repeat_interleave(g, 1), codes.double(), x.double()
    return xd @ (s * q + z).T, xd.abs() @ (s.abs() * q + z.abs()).T


def _exact_inputs(bits, g, K, seed, extreme=False):
    gen = torch.Generator().manual_seed(seed)
    e = torch.randint(-3, 4, (MS[-1],), generator=gen)
    x = torch.randint(-4, 5, (MS[-1], K), generator=gen).float() * torch.pow(2.0, e.float())[:, None]
    x[3] = 0
    codes = torch.randint(0, 1 << bits, (NS[-1], K), generator=gen)
    if extreme:   # the largest code beside zeros in every group, at every position of a word in turn: a dropped high nibble or byte shows
        codes = torch.zeros_like(codes).reshape(NS[-1], K // g, g)
        pos = (torch.arange(NS[-1])[:, None] + 3 * torch.arange(K // g)[None, :]) % g
        codes.scatter_(2, pos[..., None], (1 << bits) - 1)
        codes = codes.reshape(NS[-1], K)
    scale = torch.pow(2.0, torch.randint(-2, 1, (NS[-1], K // g), generator=gen).float()) * (1 - 2 * torch.randint(0, 2, (NS[-1], K // g), generator=gen))
    zero = scale * torch.randint(-(1 << (bits - 1)), (1 << (bits - 1)) + 1, (NS[-1], K // g), generator=gen)
    ref, B = _terms(x, codes, scale, zero, g)
    assert float((B * torch.pow(2.0, 2 - e.double())[:, None]).max()) < 2 ** 24   # the precondition of bit-equality
    return x, codes, scale, zero, ref


EXACT = [(bits, g, K, False) for bits in (4, 8) for g in (32, 64, 128) for K in (g, 2 * g, 3 * g, 1280)] + [(4, 64, 192, True), (8, 32, 96, True)]


@pytest.mark.parametrize("bits,g,K,extreme", EXACT, ids=lambda v: str(v))
def test_exact_cases_are_bit_equal(bits, g, K, extreme):
    i = EXACT.index((bits, g, K, extreme))
    x, codes, scale, zero, ref = _exact_inputs(bits, g, K, 100 + i, extreme)
    ql = _image(codes, scale, zero, bits, g, SZ_DTYPES[i % 3])
    xd = x.to(DEV)
    for N in NS:
        for M in MS:
            y = _run(xd[:M], _rows(ql, N))
            assert torch.equal(y.double().cpu(), ref[:M, :N]), (N, M)
    assert torch.equal(_run(xd[:8], ql), _run(xd[:8], ql)) and torch.equal(_run(xd[:33], ql), _run(xd[:33], ql))   # a second run, bit-equal


FLOAT = [(4, 64, 1280, 33), (8, 64, 1280, 17), (4, 32, 96, 33), (8, 128, 384, 16), (4, 128, 5120, 17), (8, 32, 5120, 15), (4, 64, 5120, 33)]
WORST = {}   # form -> largest error / bound seen (printed: docs/COVERAGE.md row x2 quotes the MI355X figures)


@pytest.mark.parametrize("bits,g,K,N", FLOAT, ids=lambda v: str(v))
def test_float_cases_stay_within_the_derived_bound(bits, g, K, N):
    gen = torch.Generator().manual_seed(K + g + bits)
    x = torch.randn(MS[-1], K, generator=gen)
    wq, scale, zero = ops.quantize_affine(torch.randn(N, K, generator=gen) / K ** 0.5, g, bits)
    codes = ops.unpack_codes(wq, bits)
    ql = _image(codes, scale, zero, bits, g, torch.float32)
    ref, B = _terms(x, codes, scale, zero, g)
    split = (2.0 ** -22 * x.double().abs() + 2.0 ** -25) @ (scale.double().abs().repeat_interleave(g, 1) * codes).T
    groups, xd, ys = K // g, x.to(DEV), {}
    for M in MS:
        ys[M] = _run(xd[:M], ql)
        bound = (g + -(-groups // 32) + 8) * U * B[:M] if M <= 8 else (2 * g + -(-groups // 4) + 8) * U * B[:M] + split[:M]
        ratio = float(((ys[M].double().cpu() - ref[:M]).abs() / bound).max())
        form = "stream" if M <= 8 else "tile"
        WORST[form] = max(WORST.get(form, 0.0), ratio)
        print(f"qlinear {form} bits={bits} g={g} K={K} N={N} M={M}: error / bound = {ratio:.4f} (worst so far {WORST[form]:.4f})")
        assert ratio <= 1.0, (M, ratio)
    # a row does not depend on the rows beside it, within a form and instantiation
    assert torch.equal(ys[5], ys[8][:5]) and torch.equal(ys[9], ys[16][:9]) and torch.equal(ys[17], ys[33][:17]) and torch.equal(ys[33], ys[65][:33])


@pytest.mark.parametrize("M,kv", [(4, torch.bfloat16), (8, torch.float16), (9, torch.float16), (33, torch.bfloat16)])
def test_epilogue_bias_gelu_res_and_a_16_bit_second_destination(M, kv):
    bits, g, K, N, split = 4, 64, 256, 40, 24
    gen = torch.Generator().manual_seed(M)
    x, res, bias, cs = torch.randn(M, K, generator=gen), torch.randn(M, N, generator=gen), torch.randn(N, generator=gen), torch.rand(N, generator=gen) + 0.5
    wq, scale, zero = ops.quantize_affine(torch.randn(N, K, generator=gen) / K ** 0.5, g, bits)
    codes = ops.unpack_codes(wq, bits)
    ql = _image(codes, scale, zero, bits, g, torch.float32, bias=bias)
    y2 = torch.full((M, N - split + 2), 9.0, dtype=kv, device=DEV)
    y = _run(x.to(DEV), ql, post_act=ops.ACT_GELU, res=res.to(DEV), colscale=cs.to(DEV), out_scale=0.5, y2=y2[:, :N - split])
    s, B = _terms(x, codes, scale, zero, g)
    v = s + bias.double()
    ref = (torch.nn.functional.gelu(v) * cs.double() + res.double()) * 0.5
    split_err = (2.0 ** -22 * x.double().abs() + 2.0 ** -25) @ (scale.double().abs().repeat_interleave(g, 1) * codes).T
    # the sum's bound through GELU (slope <= 1.13) and colscale, plus a few float32 roundings of the tail (erff: 4 ulp of a value <= |v| + 1)
    tol = 0.5 * (1.13 * cs.double() * ((2 * g + 8) * U * B + split_err + U * v.abs()) + 8 * 2 * U * (v.abs() + 1) * cs.double() + 2 * U * res.double().abs())
    got = torch.cat([y.double().cpu(), y2[:, :N - split].double().cpu()], 1)
    tol[:, split:] += ref[:, split:].abs() * (2.0 ** -8 if kv == torch.bfloat16 else 2.0 ** -11) + 2.0 ** -24   # the slot's own rounding: half a unit of 8 / 11 significant bits
    assert bool(((got - ref).abs() <= tol).all()), float(((got - ref).abs() / tol).max())
    assert bool((y2[:, N - split:] == 9.0).all())


@pytest.mark.parametrize("bits,g,dt", [(4, 64, torch.float16), (8, 32, torch.bfloat16), (4, 128, torch.float32)])
def test_dequantize_affine_is_the_torch_expression_bit_for_bit(bits, g, dt):
    gen = torch.Generator().manual_seed(bits + g)
    N, K = 70, 3 * g
    wq, scale, zero = ops.quantize_affine(torch.randn(N, K, generator=gen).to(dt), g, bits)
    want = scale.float().repeat_interleave(g, 1) * ops.unpack_codes(wq, bits).float() + zero.float().repeat_interleave(g, 1)
    assert torch.equal(ops.dequantize_affine(ops.pack_quantized(wq, scale, zero, None, DEV, group_size=g, bits=bits)).cpu(), want)
    rows = torch.tensor([[69, 0, 5], [5, 68, 1]], dtype=torch.int32)
    pos = torch.randn(3, K, generator=gen)
    got = ops.dequantize_affine(ops.pack_quantized(wq, scale, zero, None, DEV, group_size=g, bits=bits), rows.to(DEV), add=pos.to(DEV))
    assert torch.equal(got.cpu(), want[rows.reshape(-1).long()] + pos.repeat(2, 1))
