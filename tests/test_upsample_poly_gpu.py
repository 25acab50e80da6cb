"""The generator up-samplers on their dedicated kernel (``ops.upsample_polyphase`` -> ``mi355_upsample_polyphase``): LeakyReLU(0.1) -> transposed conv
(stride u, 2 u taps, padding u / 2) -> + x_source, against ``torch.nn.functional.conv_transpose1d`` in float64 on the CPU and against the launch it
replaces (``ops.conv_gemm(..., up=...)`` on the wave-specialised kernel, tile code 6128128: the kernel the engine's batches run), which is this
file's reference kernel, not the code under test.

Shapes: both instantiations -- 512 -> 256, u = 10, row_off = 0 (row blocks of H = 32 GEMM rows) and 256 -> 128, u = 6, row_off = 1 plus the row-0
rule (H = 64) -- at L in {1, 2, H - 1, H, H + 1, 2 H + 3}; B = 3 with lens = [L, an item ending inside a block, 1]; x, x_source and the output are
column ranges of wider buffers (row stride > C).  Weights are bf16-valued with std 0.02.

Parity rules: bit-equal to the general launch (the kernel keeps its order of additions); max |y - f64| <= 3e-5 of the output's peak, the precision-2
bar of DESIGN section 2.  Measured on MI355X: see docs/PARITY.md (generator up-samplers)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
SLOPE = 0.1
SENTINEL = -777.0
BAR = 3e-5
WS4_TILE = 6128128
STAGES = {0: dict(cin=512, cout=256, u=10, row_off=0), 1: dict(cin=256, cout=128, u=6, row_off=1)}


@pytest.fixture(scope="module")
def ops():
    from mlx_audio_amd import ops as _ops

    _ops.require_gpu()
    return _ops


def _bf16_valued(t):
    return t.to(torch.bfloat16).to(torch.float32)


def _wide(B, L, C, fill=None, gen=None):
    """[B, L, C] as columns [16, 16 + C) of a [B, L, C + 32] buffer: 16-byte aligned rows with a row stride > C."""
    buf = torch.full((B, L, C + 32), SENTINEL if fill is None else fill)
    if gen is not None:
        buf[:, :, 16:16 + C] = torch.randn(B, L, C, generator=gen)
    return buf


def _lens(L, H):
    mid = max(1, L - max(1, H // 2))
    if mid % H == 0 and mid > 1:
        mid -= 1
    return [L, mid, 1]


def general_launch(ops, x, pc, xsrc, y, u, row_off, lens, precision=2, tile=WS4_TILE):
    """The path the kernel replaces: the polyphase conv_gemm call of the engine, then the copy of the pad row."""
    L, kp, cout = x.shape[1], pc.k, pc.cout // u
    ops.conv_gemm(x, pc, y, pad=kp - 1, lout=L + kp - 1, lens_in=lens, lens_out=None if lens is None else lens + (kp - 1), pre_act=ops.ACT_LEAKY,
                  pre_slope=SLOPE, res=xsrc, precision=precision, tile=tile,
                  up=dict(s=u, p=(kp * u - u) // 2, cout=cout, row_off=row_off, lout=L * u, lens=None if lens is None else lens * u))
    if row_off:
        y[:, 0, :].copy_(xsrc[:, 0, :])
    return y


def upsample_f64(x, w_t, b, xsrc, u, row_off, lens, slope=SLOPE):
    """conv_transpose1d(leaky_relu(x)) + bias + x_source per item in float64; w_t [Cout, K, Cin].  One [lens * u + row_off, Cout] array per item."""
    k = w_t.shape[1]
    wt = w_t.double().permute(2, 0, 1).contiguous()   # torch: [Cin, Cout, K]
    outs = []
    for i, n in enumerate(lens):
        xa = torch.nn.functional.leaky_relu(x[i, :n].double(), slope).t()[None]
        y = torch.nn.functional.conv_transpose1d(xa, wt, b.double(), stride=u, padding=(k - u) // 2)[0].t()
        assert y.shape[0] == n * u
        full = xsrc[i, :n * u + row_off].double().clone()
        full[row_off:] += y
        outs.append(full.numpy())
    return outs


class Case:
    """One input batch, its float64 statement and both device results (computed once per module)."""

    def __init__(self, ops, stage, L, seed, cin=None, cout=None, u=None, row_off=None, f16=False, precision=2, tile=WS4_TILE):
        s = STAGES[stage] if stage is not None else dict(cin=cin, cout=cout, u=u, row_off=row_off)
        self.cin, self.cout, self.u, self.row_off = s["cin"], s["cout"], s["u"], s["row_off"]
        self.H = ops.UPSAMPLE_POLY_SHAPES.get((self.cin, self.cout, self.u), 64)
        self.L, self.precision = L, precision
        g = torch.Generator().manual_seed(seed)
        B, Lo = 3, L * self.u + self.row_off
        self.w_t = _bf16_valued(torch.randn(self.cout, 2 * self.u, self.cin, generator=g) * 0.02)
        self.b = torch.randn(self.cout, generator=g) * 0.1
        self.pc = ops.pack_conv_transpose(self.w_t, self.b, self.u, DEV, f16=f16)
        self.x = _wide(B, L, self.cin, gen=g)[:, :, 16:16 + self.cin]
        self.xsrc = _wide(B, Lo, self.cout, gen=g)[:, :, 16:16 + self.cout]
        self.lens = _lens(L, self.H)
        self.xd, self.sd = self._dev(self.x), self._dev(self.xsrc)
        self.ld = torch.tensor(self.lens, dtype=torch.int32, device=DEV)
        self.ref = upsample_f64(self.x, self.w_t, self.b, self.xsrc, self.u, self.row_off, self.lens)
        self.new = ops.upsample_polyphase(self.xd, self.pc, self.sd, self.new_y(), self.u, row_off=self.row_off, lens=self.ld, pre_slope=SLOPE,
                                          precision=precision).cpu()
        self.old = general_launch(ops, self.xd, self.pc, self.sd, self.new_y(), self.u, self.row_off, self.ld, precision=precision, tile=tile).cpu()
        torch.cuda.synchronize()

    @staticmethod
    def _dev(view):
        """The same column range of the same wide buffer, on the device."""
        C = view.shape[2]
        return view._base.to(DEV)[:, :, 16:16 + C] if view._base is not None else view.to(DEV)

    def new_y(self):
        return _wide(3, self.L * self.u + self.row_off, self.cout).to(DEV)[:, :, 16:16 + self.cout]

    def error(self, got):
        peak = max(float(np.abs(r).max()) for r in self.ref)
        return max(float(np.abs(got[i, :len(r)].double().numpy() - r).max()) for i, r in enumerate(self.ref)) / peak, peak


_CASES = {}


def _case(ops, stage, lname):
    H = ops.UPSAMPLE_POLY_SHAPES[(STAGES[stage]["cin"], STAGES[stage]["cout"], STAGES[stage]["u"])]
    L = {"1": 1, "2": 2, "H-1": H - 1, "H": H, "H+1": H + 1, "2H+3": 2 * H + 3}[lname]
    if (stage, L) not in _CASES:
        _CASES[(stage, L)] = Case(ops, stage, L, 10 * stage + L)
    return _CASES[(stage, L)]


LNAMES = ["1", "2", "H-1", "H", "H+1", "2H+3"]


@pytest.mark.parametrize("lname", LNAMES)
@pytest.mark.parametrize("stage", [0, 1])
def test_bit_equal_to_the_general_launch(ops, stage, lname):
    c = _case(ops, stage, lname)
    assert ops.upsample_polyphase_eligible(c.pc, c.u)
    assert torch.equal(c.new, c.old), float((c.new - c.old).abs().max())


@pytest.mark.parametrize("lname", LNAMES)
@pytest.mark.parametrize("stage", [0, 1])
def test_against_float64(ops, stage, lname):
    c = _case(ops, stage, lname)
    en, peak = c.error(c.new)
    eo, _ = c.error(c.old)
    print(f"upsample_polyphase stage {stage} L {c.L} lens {c.lens}: new {en:.3e}  general launch {eo:.3e}  of peak {peak:.3f}  (bar {BAR:.0e})")
    assert np.isfinite(en) and peak > 0.5
    assert en <= BAR, (en, BAR)


@pytest.mark.parametrize("lname", LNAMES)
@pytest.mark.parametrize("stage", [0, 1])
def test_untouched_rows_and_pad_row(ops, stage, lname):
    c = _case(ops, stage, lname)
    for i, n in enumerate(c.lens):
        valid = n * c.u + c.row_off
        assert bool((c.new[i, valid:] == SENTINEL).all()), i
        assert not bool((c.new[i, :valid] == SENTINEL).any()), i
        if c.row_off:
            assert torch.equal(c.new[i, 0], c.xsrc[i, 0]), i


@pytest.mark.parametrize("stage", [0, 1])
def test_identical_items_repeat_and_batch_invariance(ops, stage):
    c = _case(ops, stage, "2H+3")
    x3 = c.xd[:1].expand(3, -1, -1).contiguous()
    s3 = c.sd[:1].expand(3, -1, -1).contiguous()
    run = lambda x, s, lens: ops.upsample_polyphase(x, c.pc, s, torch.full((x.shape[0], c.L * c.u + c.row_off, c.cout), SENTINEL, device=DEV), c.u,
                                                    row_off=c.row_off, lens=lens, pre_slope=SLOPE).cpu()
    a1, a2 = run(x3, s3, None), run(x3, s3, None)
    assert torch.equal(a1[0], a1[1]) and torch.equal(a1[0], a1[2])
    assert torch.equal(a1, a2)
    assert not bool((a1 == SENTINEL).any())
    assert torch.equal(a1[0], c.new[0])                       # the full-length item of the ragged batch, uniform and without lens
    alone = run(c.xd[1:2].contiguous(), c.sd[1:2].contiguous(), c.ld[1:2].contiguous())
    assert torch.equal(alone[0], c.new[1])                    # an item alone = the same item inside the batch


def test_fallback_is_the_general_launch(ops):
    # an fp16 image (the hi + lo fp16 passes) of the stage-1 shape, and a stride the kernel has no instantiation for: the general launch
    for kw in (dict(stage=1, f16=True, precision=4), dict(stage=None, cin=64, cout=32, u=4, row_off=1)):
        c = Case(ops, kw.pop("stage"), 37, 5, tile=0, **kw)
        assert not ops.upsample_polyphase_eligible(c.pc, c.u, precision=c.precision)
        assert torch.equal(c.new, c.old)
        e, peak = c.error(c.new)
        print(f"upsample_polyphase fallback {c.cin} -> {c.cout} u {c.u} precision {c.precision}: {e:.3e} of peak {peak:.3f}")
        assert e <= BAR, (e, BAR)
        for i, n in enumerate(c.lens):
            assert bool((c.new[i, n * c.u + c.row_off:] == SENTINEL).all()), i
