"""``csrc/moe_quant_mx.hip`` against float64 on ``ops.mx_code_values * ops.mx_scale_values``.  Exact cases (``ops.switch_linear``): x = integers in [-4, 4] times a
power of two per row; every E2M1 code (mxfp8: E4M3 multiples of 2^-2 up to 8); E8M0 bytes 125 .. 129 (nvfp4: E4M3 bytes worth 2^j or 1.5 2^j, j in -2 .. 2);
integer biases: every product is a multiple of one unit u per row and sum |product| + |bias| < 2^24 u (asserted), so the result must be bit-equal.  Float cases
(``ops.switch_glu``): the bound of tests/test_moe_quant_kernels_gpu.py without its zero term; depth = the longest chain of fp32 additions behind one output:
mxfp4 / mxfp8 64 (one step's hi and lo MFMAs) + the steps of one K part (folds) + 8 (join, bias, store); nvfp4 2 x the K values of one K part + 8."""
import pytest
import torch

import test_moe_quant_kernels_gpu as Q   # shared with the affine kernel's suite: _ids, _guarded, _intact, SENT, U, _ULP
from mlx_audio_amd import _lib, ops
from mlx_audio_amd._lib import Mi355Error

pytestmark = pytest.mark.gpu
DEV = Q.DEV


def _pack(codes, scales, bias, mode):   # codes [E, n, K] int64, scale bytes [E, n, K / g] -> the device container
    wq = ops.pack_codes(codes.reshape(-1, codes.shape[2]), ops.QMODES[mode][1]).view(torch.int32).reshape(*codes.shape[:2], -1)
    return ops.pack_quantized_switch_linear_mx(wq, scales.to(torch.uint8), bias, DEV, mode=mode)


_values = lambda codes, scales, mode: ops.mx_code_values(codes, mode).double() * ops.mx_scale_values(scales, mode).double().repeat_interleave(ops.QMODES[mode][2], -1)


# (mode, Kdim, Ncols, E, k, N, ids kind, extreme codes).  Kdim: one group, three groups, 128 (one run), 160 (a run and a step: both K parts, below the 256
# values staged at a time), 144 at nvfp4 (a last half step), 256 (the staged chunk), 288 / 320 / 384 (past it: a second chunk of one step, two steps, a run);
# Ncols 16, 48 (a tail wave), 80 (a dead wave beside a live one); 65 rows on one expert (three tiles, the last of one row); an expert without a token.
EXACT = [("mxfp4", 32, 16, 1, 1, 1, "rand", False), ("mxfp4", 96, 48, 4, 2, 5, "rand", False), ("mxfp4", 128, 80, 64, 6, 17, "rand", False),
         ("mxfp4", 160, 48, 4, 2, 33, "hole", False), ("mxfp4", 256, 16, 4, 1, 65, "one", False), ("mxfp4", 384, 80, 64, 6, 1, "rand", False),
         ("nvfp4", 16, 16, 1, 1, 1, "rand", False), ("nvfp4", 48, 80, 64, 6, 5, "rand", False), ("nvfp4", 128, 48, 4, 2, 17, "hole", False),
         ("nvfp4", 160, 16, 4, 1, 65, "one", False), ("nvfp4", 144, 48, 4, 2, 33, "rand", False), ("nvfp4", 256, 80, 64, 6, 1, "rand", False),
         ("nvfp4", 288, 48, 4, 2, 17, "rand", False),
         ("mxfp8", 32, 48, 4, 2, 1, "rand", False), ("mxfp8", 96, 16, 1, 1, 17, "rand", False), ("mxfp8", 128, 48, 4, 1, 65, "one", False),
         ("mxfp8", 160, 80, 64, 6, 5, "rand", False), ("mxfp8", 256, 48, 4, 2, 33, "hole", False), ("mxfp8", 320, 80, 64, 6, 17, "rand", False),
         ("mxfp4", 96, 48, 4, 2, 5, "rand", True), ("nvfp4", 48, 48, 4, 2, 5, "hole", True), ("mxfp8", 96, 80, 4, 2, 17, "rand", True)]


@pytest.mark.parametrize("i", range(len(EXACT)), ids=[str(c) for c in EXACT])
def test_switch_linear_on_mx_codes_is_bit_equal(i):
    (mode, K, n, E, k, N, kind, extreme), (_, bits, g) = EXACT[i], ops.QMODES[EXACT[i][0]]
    gen = torch.Generator().manual_seed(300 + i)
    e2 = torch.randint(-3, 4, (N,), generator=gen)
    x = torch.randint(-1 if extreme else -4, 2 if extreme else 5, (N, K), generator=gen).float() * torch.pow(2.0, e2.float())[:, None]
    every, vals = torch.arange(1 << bits), ops.mx_code_values(torch.arange(1 << bits), mode)
    allowed, cu = (every, 0.5) if bits == 4 else (every[(vals.abs() <= 8) & (vals * 4 == torch.round(vals * 4))], 0.25)
    codes = allowed[torch.randint(0, allowed.numel(), (E, n, K), generator=gen)]
    if extreme:   # per group the largest code of either sign or the smallest non-zero one, alone beside zeros, at every position in turn
        picks, cu = ((7, 15, 1), 0.5) if bits == 4 else ((0x7E, 0xFE, 0x01), 2.0 ** -9)   # 6, -6, 0.5 / 448, -448, 2^-9
        gi, ni = torch.arange(K // g)[None, None, :], torch.arange(n)[None, :, None]
        pick = torch.tensor(picks)[(gi + ni) % 3].expand(E, n, K // g)
        codes = torch.zeros(E, n, K // g, g, dtype=torch.int64).scatter_(3, ((torch.arange(E)[:, None, None] + ni + 3 * gi) % g)[..., None], pick[..., None]).reshape(E, n, K)
    if mode == "nvfp4":
        ok = torch.arange(128)[torch.isin(ops.mx_scale_values(torch.arange(128), mode), torch.tensor([m * 2.0 ** j for m in (1.0, 1.5) for j in range(-2, 3)]))]
        scales, su = ok[torch.randint(0, ok.numel(), (E, n, K // g), generator=gen)], 2.0 ** -3
    else:
        scales, su = torch.randint(125, 130, (E, n, K // g), generator=gen), 2.0 ** -2
    bias = torch.randint(-8, 9, (E, n), generator=gen).float()
    ids = Q._ids(N, E, k, gen, kind)
    w, sel = _values(codes, scales, mode), ids.long()
    want = torch.einsum("tk,tsnk->tsn", x.double(), w[sel]) + bias.double()[sel]
    B = torch.einsum("tk,tsnk->tsn", x.double().abs(), w.abs()[sel]) + bias.double().abs()[sel]
    u = torch.pow(2.0, e2.double())[:, None, None] * cu * su   # at most 1: the integer biases are multiples of it too
    assert float((B / u).max()) < 2 ** 24 and float(u.max()) <= 1   # the precondition of bit-equality
    lin, xd, idd = _pack(codes, scales, bias, mode), x.to(DEV), ids.to(DEV)
    buf, out = Q._guarded(N, k, n)
    ops.switch_linear(xd, lin, idd, out)
    got = out.cpu()
    assert Q._intact(buf, n) and torch.equal(got.double(), want)
    assert torch.equal(ops.switch_linear(xd, lin, idd).cpu(), got)   # a repeat
    for t in {0, N // 2, N - 1}:
        assert torch.equal(ops.switch_linear(xd[t:t + 1], lin, idd[t:t + 1]).cpu()[0], got[t]), t


def _tile_terms(a, da, w, bias, sel, mode):
    """float64: rows a [N, k, K] known to |da| times the experts sel [N, k] of dequantised w [E, cols, K]: the products, and the bound on the kernel's error."""
    part = 128 * -(-(-(-w.shape[2] // 128)) // 2)   # K values of the longer K part: whole runs
    depth, up, W, b = (2 * part if mode == "nvfp4" else 64 + part // 32) + 8, a.abs() + da, w[sel].abs(), bias.double()[sel]
    mm = lambda p, q: torch.einsum("tsk,tsnk->tsn", p, q)
    val = mm(a, w[sel]) + b
    return val, mm(da, W) + depth * Q.U * (mm(up, W) + b.abs()) + mm(2.0 ** -22 * up + 2.0 ** -25, W) + Q._ULP(val)


@pytest.mark.parametrize("mode", list(ops.QMODES))
def test_switch_glu_on_mx_codes_stays_within_the_derived_bound(mode):
    D, I, E, k, N = 64, 96, 4, 2, 37   # 74 pairs on four experts: tiles of one and of two 16-row blocks
    gen = torch.Generator().manual_seed(D + I + N)
    x, ids, wts = torch.randn(N, D, generator=gen) * 1.5 + 0.2, Q._ids(N, E, k, gen), torch.rand(N, k, generator=gen) + 0.1
    shared, res = torch.randn(N, D, generator=gen), torch.randn(N, D, generator=gen)
    host, dev = [], []
    for n, K in ((I, D), (I, D), (D, I)):
        wq, scales = ops.quantize_mx(torch.randn(E * n, K, generator=gen) / K ** 0.5, mode)
        codes, bias = ops.unpack_codes(wq, ops.QMODES[mode][1]).reshape(E, n, K), torch.randn(E, n, generator=gen) * 0.1
        host.append((_values(codes, scales.reshape(E, n, -1), mode), bias))
        dev.append(_pack(codes, scales.reshape(E, n, -1), bias, mode))
    ex, sel, xs = ops.PackedQuantizedExpertsMX(*dev), ids.long(), x.double()[:, None, :].expand(N, k, D)
    (G, dG), (Uv, dU) = (_tile_terms(xs, torch.zeros_like(xs), *host[j], sel, mode) for j in (0, 1))
    S = G * torch.sigmoid(G)
    dS, h = 1.1 * dG + 8 * Q.U * S.abs(), S * Uv
    y, dy = _tile_terms(h, dS * (Uv.abs() + dU) + S.abs() * dU + Q.U * h.abs(), *host[2], sel, mode)
    wy, wdy = wts.double()[..., None] * y, wts.double()[..., None] * dy
    want = wy.sum(1) + shared.double() + res.double()
    bound = wdy.sum(1) + (k + 2) * Q.U * (wy.abs().sum(1) + shared.double().abs() + res.double().abs()) + Q._ULP(want)
    buf, out = Q._guarded(N, 1, D)
    ops.switch_glu(x.to(DEV), ex, ids.to(DEV), wts.to(DEV), out[:, 0], shared=shared.to(DEV), res=res.to(DEV))
    got = out[:, 0].cpu()
    ratio = float(((got.double() - want).abs() / bound).max())
    print(f"MOE MX switch_glu {mode} D={D} I={I} E={E} k={k} N={N}: error / bound = {ratio:.4f}")
    assert Q._intact(buf, D) and ratio <= 1.0
    alone = torch.full((1, D), float("nan"), device=DEV)   # the last token routed alone
    ops.switch_glu(x[-1:].to(DEV), ex, ids[-1:].to(DEV), wts[-1:].to(DEV), alone, shared=shared[-1:].to(DEV), res=res[-1:].to(DEV))
    assert torch.equal(alone.cpu()[0], got[-1])


# (status, message, fields of mi355_moe_qglu_mx_args changed in an otherwise good SwitchGLU call at N 3, k 2, E 4, D 64, I 96 in mxfp4)
OFF, SHORT = "q_gate + 4", "workspace_bytes - 16"
REFUSALS = [(-3, "gate qmode = 0 is not built", dict(qmode_gate=0)), (-3, "down qmode = 7 is not built", dict(qmode_down=7)),
            (-3, "gate and up must share one mode .gate: qmode = 1; up: qmode = 3", dict(qmode_up=3)),
            (-3, "gate Kdim = 48 is not a multiple of 32", dict(D=48)), (-3, "down Kdim = 80 is not a multiple of 32", dict(I=80)),
            (-3, "gate Kdim = 24 is not a multiple of 16", dict(D=24, qmode_gate=2, qmode_up=2)),
            (-1, "D = 64 and I = 62 must be multiples of 4", dict(I=62, mode=1)), (-1, "null tensor .up codes or scales", dict(s_up=None)),
            (-1, "gate codes must be 16-byte aligned", dict(q_gate=OFF)), (-1, "workspace of", dict(workspace_bytes=SHORT)),
            (-1, "misaligned rows", dict(ldx=66)), (-1, "misaligned rows .res", dict(ld_res=60)), (-1, "unknown mode 2", dict(mode=2)),
            (-3, "E = 513 is above MI355_MOE_MAX_EXPERTS = 512", dict(E=513))]


@pytest.mark.parametrize("status,text,change", REFUSALS, ids=[r[1] for r in REFUSALS])
def test_refusals_launch_nothing(status, text, change):
    N, k, E, D, I = 3, 2, 4, 64, 96
    gen = torch.Generator().manual_seed(0)
    mk = lambda n, K: _pack(torch.randint(0, 16, (E, n, K), generator=gen), torch.full((E, n, K // 32), 127), None, "mxfp4")
    parts = dict(gate=mk(I, D), up=mk(I, D), down=mk(D, I))
    x, ids, wts = torch.zeros(N, D, device=DEV), Q._ids(N, E, k, gen).to(DEV), torch.ones(N, k, device=DEV)
    out, ws = torch.full((N * k, 128), Q.SENT, device=DEV), ops.moe_plan(ids, E, D, I)   # out: wide enough for either mode
    kw = dict(x=x.data_ptr(), ldx=D, N=N, k=k, E=E, D=D, I=I, weights=wts.data_ptr(), res=x.data_ptr(), ld_res=D, out=out.data_ptr(), ldo=128,
              workspace=ws.buf.data_ptr(), workspace_bytes=ws.nbytes, mode=0)
    for m, p in parts.items():
        kw.update(ops._qproj_mx(m, p))
    kw.update({f: {OFF: kw["q_gate"] + 4, SHORT: ws.nbytes - 16}.get(v, v) for f, v in change.items()})
    with pytest.raises(Mi355Error, match=rf"\({status}\).*{text}"):
        _lib.call_struct("mi355_moe_qglu_mx", "mi355_moe_qglu_mx_args", ops._stream(), **kw)
    torch.cuda.synchronize()
    assert bool((out == Q.SENT).all())
