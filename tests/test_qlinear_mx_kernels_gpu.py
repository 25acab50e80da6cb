"""``ops.qlinear`` on MX images / ``ops.dequantize_mx`` (qlinear_mx.hip) against plain float64 torch on w = value(code) * value(scale).

Exact cases: x = small integers times a power of two per row; every w is a multiple of a power of two ``wunit`` (mxfp4: 2^-1 elements, E8M0 bytes
124 .. 127, wunit 2^-4; mxfp8: elements that are multiples of 2^-2 up to 16, wunit 2^-5; nvfp4: scales from {0.5, 0.75, 1, 1.5, 1.75}, wunit 2^-3;
the extreme cases take the smallest element's own unit).  With sum|x||w| below 2^24 of the units 2^e_row * wunit (asserted from the float64 side) no
addition rounds, in any order: both forms must return the float64 result bit for bit.  The extreme cases hold the largest-magnitude code and the
smallest non-zero one alone beside zeros in each group; each of them (asserted) reaches every position of a word: a dropped nibble or byte, or a
flushed subnormal, shows in either half of a packed conversion.

Float cases: per element, on B = sum|x||w|, u = 2^-24:
  accumulation  depth * u * B.  Stream: g FMAs of a group, the lane's folds (128 / g per run; of every staged chunk of rc runs -- the route's chunk_k /
                128 -- a lane takes ceil(rc / 32), so lane_runs = sum over the chunks), 3 shuffles, 2 wave sums, the store: g + 128 / g * lane_runs + 8.
                Tile, mxfp4 / mxfp8: two MFMAs of 32 terms into the group's tile (64 sequential additions), the wave's folds 4 ceil(runs / 4), the same tail: 64 + 4 ceil(runs / 4) + 8.  Tile, nvfp4: every MFMA of the wave adds
                into one accumulator: 64 * 4 ceil(runs / 4) + 8.  runs = ceil(K / 128).
  split         tile form only: x - (hi + lo) <= 2^-22 |x| while lo is a normal fp16, 2^-25 absolute below: sum_k (2^-22 |x_k| + 2^-25) |w_k|
"""
import pytest
import torch

from mlx_audio_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
NS, MS = (1, 15, 16, 17, 33), (1, 2, 4, 5, 8, 9, 16, 17, 33, 65)
MODES = tuple(ops.QMODES)
U = 2.0 ** -24


def _image(codes, scales, mode, bias=None):
    return ops.pack_quantized_mx(ops.pack_codes(codes, ops.QMODES[mode][1]), scales, bias, DEV, mode=mode)


def _rows(ql, n):
    """The image of the first n output columns."""
    return ops.QuantizedLinearMX(ql.q[:n], ql.scales[:n], None if ql.bias is None else ql.bias[:n], n, ql.k, ql.mode, ql.bits, ql.group_size)


def _run(x, ql, **kw):
    """Strided x and y, y NaN-initialised inside sentinel guards (and at an address that is not 16-byte aligned); returns y after checking the guards."""
    M, K = x.shape
    xb = torch.full((M, K + 4), 3.5, device=DEV)
    xb[:, :K] = x
    yb = torch.full((M, ql.n + 9), 7.25, device=DEV)
    y = yb[:, 3:3 + ql.n]
    y.fill_(float("nan"))
    ops.qlinear_mx(xb[:, :K], ql, y, **kw)
    assert bool((yb[:, :3] == 7.25).all()) and bool((yb[:, 3 + ql.n:] == 7.25).all())
    return y.clone()


def _terms(x, codes, scales, mode):
    """float64: w, the reference x @ w^T and B = |x| @ |w|^T."""
    w = ops.mx_code_values(codes, mode).double() * ops.mx_scale_values(scales, mode).double().repeat_interleave(ops.QMODES[mode][2], 1)
    return w, x.double() @ w.T, x.double().abs() @ w.abs().T


def _exact_inputs(mode, K, seed, extreme):
    _, bits, g = ops.QMODES[mode]
    gen = torch.Generator().manual_seed(seed)
    N, M = NS[-1], MS[-1]
    e = torch.randint(-3, 4, (M,), generator=gen)
    x = torch.randint(-2, 3, (M, K), generator=gen).float() if extreme else torch.randint(-4, 5, (M, K), generator=gen).float()
    x = x * torch.pow(2.0, e.float())[:, None]
    x[3] = 0
    if mode == "nvfp4":
        scales = torch.tensor([0.5, 0.75, 1.0, 1.5, 1.75]).to(torch.float8_e4m3fn).view(torch.uint8)[torch.randint(0, 5, (N, K // g), generator=gen)]
    else:
        scales = torch.randint(124, 128, (N, K // g), generator=gen).to(torch.uint8)
    if extreme:   # one non-zero code per group: the largest (either sign) or the smallest, its position moving with the row and the group
        big, small = ((0x7E, 0xFE), 0x01) if bits == 8 else ((7, 15), 1)
        n, gi = torch.arange(N)[:, None], torch.arange(K // g)[None, :]
        pick = torch.tensor([big[0], big[1], small])[(n + gi) % 3]   # a cycle of three against positions that step by one: free of the position's parity
        pos = (n + 3 * gi) % g
        codes = torch.zeros(N, K // g, g, dtype=torch.int64).scatter_(2, pos[..., None], pick[..., None]).reshape(N, K)
        for c in (big[0], big[1], small):   # each of the three codes reaches both halves of a packed conversion, at every byte of a word
            assert {int(v) % 8 for v in pos[pick == c]} == set(range(8)), c
        wunit = 2.0 ** (-9 - 3) if bits == 8 else 2.0 ** (-1 - 3)
    elif bits == 8:
        allv = ops.mx_code_values(torch.arange(256), mode)
        subset = torch.nonzero(torch.isfinite(allv) & (allv.abs() <= 16) & (allv * 4 == torch.round(allv * 4)))[:, 0]
        codes = subset[torch.randint(0, subset.numel(), (N, K), generator=gen)]
        wunit = 2.0 ** -5
    else:
        codes = torch.randint(0, 16, (N, K), generator=gen)   # all sixteen: 0.5 and -0 occur
        wunit = 2.0 ** -4
    _, ref, B = _terms(x, codes, scales, mode)
    assert float((B / (torch.pow(2.0, e.double())[:, None] * wunit)).max()) < 2 ** 24   # the precondition of bit-equality
    return x, codes, scales, ref


EXACT = [(mode, m * ops.QMODES[mode][2], False) for mode in MODES for m in (1, 2, 3)] + [(mode, 1280, False) for mode in MODES] + [
    (mode, 3 * ops.QMODES[mode][2], True) for mode in MODES]


@pytest.mark.parametrize("mode,K,extreme", EXACT, ids=lambda v: str(v))
def test_exact_cases_are_bit_equal(mode, K, extreme):
    x, codes, scales, ref = _exact_inputs(mode, K, 200 + EXACT.index((mode, K, extreme)), extreme)
    ql = _image(codes, scales, mode)
    xd = x.to(DEV)
    for N in NS:
        for M in MS:
            y = _run(xd[:M], _rows(ql, N))
            assert torch.equal(y.double().cpu(), ref[:M, :N]), (N, M)
    assert torch.equal(_run(xd[:8], ql), _run(xd[:8], ql)) and torch.equal(_run(xd[:33], ql), _run(xd[:33], ql))   # a second run, bit-equal


FLOAT = [("mxfp4", 5120, 17), ("nvfp4", 5120, 15), ("mxfp8", 5120, 33), ("nvfp4", 48, 33), ("mxfp4", 1280, 16)]
WORST = {}   # form -> largest error / bound seen (printed: docs/COVERAGE.md row x3 quotes the MI355X figures)


@pytest.mark.parametrize("mode,K,N", FLOAT, ids=lambda v: str(v))
def test_float_cases_stay_within_the_derived_bound(mode, K, N):
    _, bits, g = ops.QMODES[mode]
    gen = torch.Generator().manual_seed(K + N)
    x = torch.randn(MS[-1], K, generator=gen)
    wq, scales = ops.quantize_mx(torch.randn(N, K, generator=gen) / K ** 0.5, mode)
    codes = ops.unpack_codes(wq, bits)
    ql = _image(codes, scales, mode)
    w, ref, B = _terms(x, codes, scales, mode)
    split = (2.0 ** -22 * x.double().abs() + 2.0 ** -25) @ w.abs().T
    runs, xd, ys = -(-K // 128), x.to(DEV), {}
    tile_depth = 64 * 4 * -(-runs // 4) + 8 if mode == "nvfp4" else 64 + 4 * -(-runs // 4) + 8
    for M in MS:
        ys[M] = _run(xd[:M], ql)
        rc = ops.qlinear_mx_route(M, N, K, mode)["chunk_k"] // 128   # runs per staged chunk: a lane takes ceil(chunk's runs / 32) of every chunk
        lane_runs = (runs // rc) * -(-rc // 32) + -(-(runs % rc) // 32)
        bound = (g + 128 // g * lane_runs + 8) * U * B[:M] if M <= 8 else tile_depth * U * B[:M] + split[:M]
        ratio = float(((ys[M].double().cpu() - ref[:M]).abs() / bound).max())
        form = "stream" if M <= 8 else "tile"
        WORST[form] = max(WORST.get(form, 0.0), ratio)
        print(f"qlinear_mx {form} {mode} K={K} N={N} M={M}: error / bound = {ratio:.4f} (worst so far {WORST[form]:.4f})")
        assert ratio <= 1.0, (M, ratio)
    # a row does not depend on the rows beside it, within a form and instantiation
    assert torch.equal(ys[5], ys[8][:5]) and torch.equal(ys[9], ys[16][:9]) and torch.equal(ys[17], ys[33][:17]) and torch.equal(ys[33], ys[65][:33])


@pytest.mark.parametrize("mode", MODES)
def test_dequantize_mx_is_the_torch_expression_bit_for_bit(mode):
    """Every non-NaN element code under E8M0 bytes 87 .. 167 / every non-negative finite E4M3 scale byte; a gather with ``add`` once."""
    _, bits, g = ops.QMODES[mode]
    sb = torch.arange(0, 0x7F) if mode == "nvfp4" else torch.arange(87, 168)
    K = 256 if bits == 8 else 2 * g
    row = torch.arange(K) % (1 << bits)
    row[(row & 0x7F) == 0x7F] = 0   # the two E4M3 NaN codes (no 4-bit code has all seven low bits set)
    codes, scales = row[None].repeat(sb.numel(), 1), sb.to(torch.uint8)[:, None].repeat(1, K // g)
    want = ops.mx_code_values(codes, mode) * ops.mx_scale_values(scales, mode).repeat_interleave(g, 1)
    ql = _image(codes, scales, mode)
    assert torch.equal(ops.dequantize_mx(ql).cpu(), want)
    rows = torch.tensor([[80, 0, 5], [5, 79, 1]], dtype=torch.int32)
    pos = torch.randn(3, K, generator=torch.Generator().manual_seed(bits))
    got = ops.dequantize_mx(ql, rows.to(DEV), add=pos.to(DEV))
    assert torch.equal(got.cpu(), want[rows.reshape(-1).long()] + pos.repeat(2, 1))


REFUSALS = [(dict(mode=7), -3, "mode = 7"), (dict(group_size=64), -3, "group_size = 64"), (dict(bits=8), -3, "bits = 8"),
            (dict(K=48, ldx=48), -3, "K = 48 is not a multiple of 32"), (dict(mode=2, group_size=16, K=24, ldx=24), -3, "K = 24 is not a multiple of 16"),
            (dict(norm=1), -3, "norm"), (dict(glu=1), -3, "glu"), (dict(rope_cos=1), -3, "rope"), (dict(x_ids=1), -3, "x_ids"),
            (dict(scales=0), -1, "null pointer"), (dict(ldx=60), -1, "at least K long"), (dict(ldy=16), -1, "shorter than N")]


@pytest.mark.parametrize("fields,rc,fragment", REFUSALS, ids=lambda v: "-".join(f"{k}{x}" for k, x in v.items()) if isinstance(v, dict) else None)
def test_refusals_launch_nothing_and_leave_y_untouched(fields, rc, fragment):
    M, N, K = 4, 17, 64
    x, y = torch.ones(M, K, device=DEV), torch.full((M, N), 7.25, device=DEV)
    ql = _image(torch.ones(N, K, dtype=torch.int64), torch.full((N, 2), 127, dtype=torch.uint8), "mxfp4")
    kw = dict(x=x.data_ptr(), ldx=K, M=M, K=K, N=N, q=ql.q.data_ptr(), scales=ql.scales.data_ptr(), mode=1, bits=4, group_size=32, y=y.data_ptr(), ldy=N)
    kw.update({k: (x.data_ptr() if v == 1 and k in ("rope_cos", "x_ids") else v) for k, v in fields.items()})
    with pytest.raises(_lib.Mi355Error, match=rf"\({rc}\).*{fragment}"):
        _lib.call_struct("mi355_qlinear_mx", "mi355_qlinear_mx_args", torch.cuda.current_stream().cuda_stream, **kw)
    torch.cuda.synchronize()
    assert bool((y == 7.25).all())
