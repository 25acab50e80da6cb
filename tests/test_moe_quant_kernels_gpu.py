"""``csrc/moe_quant.hip`` (the grouped expert GEMM on MLX's packed 4 / 8-bit codes) against float64 torch on float64(scale) * q + float64(zero).
Exact cases (``ops.switch_linear``, mode 1: one launch of the tile kernel): x = small integers times a power of two per row, scales +-2^-2 .. 2^0,
zeros integer multiples of the scale, integer biases; with sum_groups(|scale| sum|x q| + |zero| sum|x|) + |bias| below 2^24 granules (asserted) no
addition rounds in any order, so the kernel must return the float64 result bit for bit.
Float cases (``ops.switch_glu``, mode 0, with biases, ``shared`` and ``res``): qlinear's tile bound per element, depth u B + split + ulp with u = 2^-24,
B = |a| @ (|scale| q + |zero|)^T + |bias| (NOT |a| @ |w|^T: scale q and zero cancel), depth = 2 g + ceil(groups / 2) + 8 (the (hi, lo) MFMAs as
sequential chains, the folds of one of the two K parts, join, bias, store), split = (2^-22 |a| + 2^-25) @ (|scale| q)^T; carried through SiLU, the
product, the down projection and the combine as tests/test_moe_kernels_gpu.py lines 99-107 do.  Largest error / bound is printed (``pytest -s``)."""
from dataclasses import replace

import pytest
import torch

from mlx_audio_amd import ops
from mlx_audio_amd._lib import Mi355Error

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = -777.25
U = 2.0 ** -24
SZ_DTYPES = (torch.float16, torch.bfloat16, torch.float32)
_ULP = lambda v: torch.pow(2.0, torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -126))) - 23)


def _ids(N, E, k, g, kind="rand"):
    """[N, k] int32, distinct per token.  ``one``: every pair on expert E - 2; ``hole``: expert 1 gets no token."""
    if kind == "one":
        return torch.full((N, k), max(E - 2, 0), dtype=torch.int32)
    pool = [e for e in range(E) if not (kind == "hole" and e == 1)]
    return torch.stack([torch.tensor(pool)[torch.randperm(len(pool), generator=g)[:k]] for _ in range(N)]).to(torch.int32)


def _pack(codes, scale, zero, bias, bits, g, dt):
    """codes [E, n, K], scale / zero [E, n, K / g] -> the device container."""
    E, n, K = codes.shape
    wq = ops.pack_codes(codes.reshape(E * n, K), bits).view(torch.int32).reshape(E, n, -1)
    return ops.pack_quantized_switch_linear(wq, scale.to(dt), zero.to(dt), bias, DEV, group_size=g, bits=bits)


def _guarded(N, k, C):
    buf = torch.full((N + 2, k, C + 4), SENT, device=DEV)
    buf[1:-1, :, :C] = float("nan")
    return buf, buf[1:-1, :, :C]


def _intact(buf, C):
    return bool((buf[0] == SENT).all() and (buf[-1] == SENT).all() and (buf[1:-1, :, C:] == SENT).all())


# (bits, g, Kdim, Ncols, E, k, N, ids kind, extreme codes).  Kdim: one group (32 at g 32, 128 at g 128), three groups (an odd count over the two K
# parts), 288 / 320 / 384 (past the 256 values staged at a time; 288 at g 32: a last chunk of one group); Ncols 16, 48 (a tail wave), 80 (a dead
# wave beside a live one); 65 rows on one expert (three tiles, the last of one row); an expert without a token.
EXACT = [(4, 32, 32, 16, 1, 1, 1, "rand", False), (8, 128, 128, 48, 4, 2, 5, "rand", False), (4, 64, 192, 80, 64, 6, 17, "rand", False),
         (8, 64, 320, 48, 4, 2, 33, "hole", False), (4, 128, 384, 16, 4, 1, 65, "one", False), (8, 32, 288, 80, 64, 6, 1, "rand", False),
         (4, 64, 192, 48, 4, 2, 5, "rand", True), (8, 32, 96, 80, 4, 2, 17, "hole", True)]


@pytest.mark.parametrize("bits,g,K,n,E,k,N,kind,extreme", EXACT, ids=lambda v: str(v))
def test_switch_linear_on_codes_is_bit_equal(bits, g, K, n, E, k, N, kind, extreme):
    i = EXACT.index((bits, g, K, n, E, k, N, kind, extreme))
    gen = torch.Generator().manual_seed(200 + i)
    e2 = torch.randint(-3, 4, (N,), generator=gen)
    x = torch.randint(-4, 5, (N, K), generator=gen).float() * torch.pow(2.0, e2.float())[:, None]
    codes = torch.randint(0, 1 << bits, (E, n, K), generator=gen)
    if extreme:   # the largest code beside zeros in every group, at every position of a word in turn: a dropped high nibble or byte shows
        pos = (torch.arange(E)[:, None, None] + torch.arange(n)[None, :, None] + 3 * torch.arange(K // g)[None, None, :]) % g
        codes = torch.zeros(E, n, K // g, g, dtype=torch.int64).scatter_(3, pos[..., None], (1 << bits) - 1).reshape(E, n, K)
    scale = torch.pow(2.0, torch.randint(-2, 1, (E, n, K // g), generator=gen).float()) * (1 - 2 * torch.randint(0, 2, (E, n, K // g), generator=gen))
    zero = scale * torch.randint(-(1 << (bits - 1)), (1 << (bits - 1)) + 1, (E, n, K // g), generator=gen)
    bias = torch.randint(-8, 9, (E, n), generator=gen).float()
    ids = _ids(N, E, k, gen, kind)
    s, z = scale.double().repeat_interleave(g, 2), zero.double().repeat_interleave(g, 2)
    w, wabs = s * codes + z, s.abs() * codes + z.abs()
    sel = ids.long()
    want = torch.einsum("tk,tsnk->tsn", x.double(), w[sel]) + bias.double()[sel]
    B = torch.einsum("tk,tsnk->tsn", x.double().abs(), wabs[sel]) + bias.double().abs()[sel]
    granule = torch.pow(2.0, (e2 - 2).clamp(max=0).double())[:, None, None]   # the biases are integers
    assert float((B / granule).max()) < 2 ** 24   # the precondition of bit-equality
    lin = _pack(codes, scale, zero, bias, bits, g, SZ_DTYPES[i % 3])
    xd, idd = x.to(DEV), ids.to(DEV)
    buf, out = _guarded(N, k, n)
    ops.switch_linear(xd, lin, idd, out)
    got = out.cpu()
    assert _intact(buf, n) and torch.equal(got.double(), want)
    assert torch.equal(ops.switch_linear(xd, lin, idd).cpu(), got)   # a repeat
    for t in {0, N // 2, N - 1}:
        assert torch.equal(ops.switch_linear(xd[t:t + 1], lin, idd[t:t + 1]).cpu()[0], got[t]), t


def _tile_terms(a, da, lin):
    """float64, for rows a [n, K] known to |da| and one expert's (codes, scale, zero, bias, g): the product, and the bound on the kernel's error."""
    codes, scale, zero, bias, g = lin
    s, z = scale.double().repeat_interleave(g, 1), zero.double().repeat_interleave(g, 1)
    w, up = s * codes + z, a.abs() + da
    val = a @ w.T + bias.double()
    depth = 2 * g + -(-(codes.shape[1] // g) // 2) + 8
    err = da @ w.abs().T + depth * U * (up @ (s.abs() * codes + z.abs()).T + bias.double().abs()) + (2.0 ** -22 * up + 2.0 ** -25) @ (s.abs() * codes).T
    return val, err + _ULP(val)


# (D, I, E, k, N, gate | up format, down format, pair dtype)
GLU = [(192, 128, 8, 2, 17, (4, 64), (4, 64), torch.float16), (256, 192, 64, 6, 1, (8, 32), (4, 64), torch.bfloat16),
       (256, 192, 64, 6, 5, (4, 128), (8, 64), torch.float32)]


@pytest.mark.parametrize("D,I,E,k,N,fgu,fd,dt", GLU, ids=lambda v: str(v))
def test_switch_glu_on_codes_stays_within_the_derived_bound(D, I, E, k, N, fgu, fd, dt):
    gen = torch.Generator().manual_seed(D + I + N)
    x = torch.randn(N, D, generator=gen) * 1.5 + 0.2
    ids, wts = _ids(N, E, k, gen), torch.rand(N, k, generator=gen) + 0.1
    shared, res = torch.randn(N, D, generator=gen), torch.randn(N, D, generator=gen)
    host, dev = [], []
    for (bits, g), (n, K) in zip((fgu, fgu, fd), ((I, D), (I, D), (D, I))):
        wq, scale, zero = ops.quantize_affine((torch.randn(E * n, K, generator=gen) / K ** 0.5).to(dt), g, bits)
        codes, bias = ops.unpack_codes(wq, bits).reshape(E, n, K), torch.randn(E, n, generator=gen) * 0.1
        host.append((codes, scale.reshape(E, n, -1), zero.reshape(E, n, -1), bias, g))
        dev.append(_pack(codes, host[-1][1], host[-1][2], bias, bits, g, dt))
    ex = ops.PackedQuantizedExperts(*dev)
    want, bound = torch.zeros(N, D, dtype=torch.float64), torch.zeros(N, D, dtype=torch.float64)
    mag = shared.double().abs() + res.double().abs()
    one = lambda p, e: (p[0][e], p[1][e], p[2][e], p[3][e], p[4])
    for t in range(N):
        xt = x[t:t + 1].double()
        for s, e in enumerate(ids[t].tolist()):
            G, dG = _tile_terms(xt, torch.zeros_like(xt), one(host[0], e))
            Uv, dU = _tile_terms(xt, torch.zeros_like(xt), one(host[1], e))
            S = G * torch.sigmoid(G)
            dS = 1.1 * dG + 8 * U * S.abs()
            h = S * Uv
            dh = dS * (Uv.abs() + dU) + S.abs() * dU + U * h.abs()
            y, dy = _tile_terms(h, dh, one(host[2], e))
            want[t] += wts[t, s].double() * y[0]
            bound[t] += wts[t, s].double() * dy[0]
            mag[t] += (wts[t, s].double() * y[0]).abs()
    want = want + shared.double() + res.double()
    bound = bound + (k + 2) * U * mag + _ULP(want)
    args = (x.to(DEV), ex, ids.to(DEV), wts.to(DEV))
    buf, out = _guarded(N, 1, D)
    ops.switch_glu(*args, out[:, 0], shared=shared.to(DEV), res=res.to(DEV))
    got = out[:, 0].cpu()
    assert _intact(buf, D)
    ratio = float(((got.double() - want).abs() / bound).max())
    print(f"MOE quantised switch_glu D={D} I={I} E={E} k={k} N={N} gate|up={fgu} down={fd} {dt}: error / bound = {ratio:.4f}")
    assert ratio <= 1.0
    alone = torch.full((1, D), float("nan"), device=DEV)   # the last token routed alone
    ops.switch_glu(x[-1:].to(DEV), ex, ids[-1:].to(DEV), wts[-1:].to(DEV), alone, shared=shared[-1:].to(DEV), res=res[-1:].to(DEV))
    assert torch.equal(alone.cpu()[0], got[-1])


def test_refusals_launch_nothing():
    N, k, E, D, I = 3, 2, 4, 192, 64
    gen = torch.Generator().manual_seed(0)
    mk = lambda n, K: _pack(torch.randint(0, 16, (E, n, K), generator=gen), torch.ones(E, n, K // 64), torch.zeros(E, n, K // 64), None, 4, 64, torch.float16)
    gate, up, down = mk(I, D), mk(I, D), mk(D, I)
    x, ids, wts = torch.zeros(N, D, device=DEV), _ids(N, E, k, gen).to(DEV), torch.ones(N, k, device=DEV)
    out, lin_out = torch.full((N, D), SENT, device=DEV), torch.full((N, k, I), SENT, device=DEV)

    def refused(status, text, fn):
        with pytest.raises(Mi355Error, match=rf"\({status}\).*{text}"):
            fn()
        torch.cuda.synchronize()
        assert bool((out == SENT).all()) and bool((lin_out == SENT).all())

    refused(-3, "bits = 3", lambda: ops.switch_linear(x, replace(gate, bits=3), ids, lin_out))
    refused(-3, "group_size = 16", lambda: ops.switch_linear(x, replace(gate, group_size=16), ids, lin_out))
    refused(-1, "Kdim = 192 is not a multiple of group_size = 128", lambda: ops.switch_linear(x, replace(gate, group_size=128), ids, lin_out))
    refused(-3, "gate and up must share one format", lambda: ops.switch_glu(x, ops.PackedQuantizedExperts(gate, replace(up, group_size=32), down), ids, wts, out))
    off = torch.zeros(gate.q.numel() + 1, dtype=torch.int32, device=DEV)[1:].view(gate.q.shape)   # four bytes past a 16-byte boundary
    refused(-1, "codes must be 16-byte aligned", lambda: ops.switch_linear(x, replace(gate, q=off), ids, lin_out))
    short = ops.MoeWorkspace(N, k, E, D, I, DEV, nbytes=ops.MoeWorkspace(N, k, E, D, I, DEV).nbytes - 16)
    refused(-1, "workspace of", lambda: ops.switch_glu(x, ops.PackedQuantizedExperts(gate, up, down), ids, wts, out, ws=short))
