"""Dispatch-branch parity of the LM-side row kernels of csrc/transformer.hip (rmsnorm, head_norm_rope, swiglu, embed_sum, dwconv) and of the sampler of
csrc/sampler.hip.

tests/test_lm_kernels_gpu.py calls each of these kernels at essentially one shape; this file walks the branches that shape does not reach (lane rounds,
workgroup tails, slot blocks of eight, the two depthwise kernels and their comb tails, device-side position clamps, the sampler's wave / block edges,
its serial tie branch and its history routes).  It follows the conventions of tests/test_row_kernel_edges_gpu.py: every test states the operation in
torch from the formulas of include/mi355audio.h (the statements live in tests/_lm_row_cases.py, and tests/test_lm_row_refs_cpu.py holds them to
F.conv1d / F.conv_transpose1d / oracle.lm_ref.apply_rope on the CPU), evaluates it in float64 (the reference) and in float32 on the CPU (``e32``, the
statement's own rounding error) and compares the kernel with the float64 result.

Bars.  Float outputs: ``4 * e32 + 1e-6 * peak`` of the float64 result (the factor covers a different summation tree, the second term a few float32
roundings of the largest value).  embed_sum: bit-equal to the float32 statement, which performs the kernel's IEEE operations in the kernel's order.
Snake prologue of dwconv: the float bar plus ``sum_k |w[c, k]| * 2 * delta / alpha_c`` with delta = 1e-6, the absolute accuracy csrc/glue.hip states
for the hardware sine (d/ds of inv * s^2 is at most 2 / alpha).  Sampler: survivor pattern and token equal to oracle/sampling_ref.py, finite values to
rtol 2e-6 / atol 1e-6 (tests/test_lm_kernels_gpu.py), with the knife edges excluded by preconditions on the INPUTS that are asserted, not skipped.
Outputs are views into larger buffers filled with an exactly representable sentinel: everything outside the view, and every row >= lens[b], must be
bit-equal to the sentinel afterwards.  Every comparison prints ``EDGE <kernel> <case> err e32 peak bar`` before it asserts (``pytest -s``).
"""

import pytest
import torch

import _lm_row_cases as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from mlx_audio_amd import ops as _ops

    _ops.require_gpu()
    return _ops


DEV = "cuda"
SENTINEL = -777.25   # exactly representable; no kernel here produces it
DELTA_SIN = 1e-6     # csrc/glue.hip: "~1e-6 absolute, as in the conv prologues"


def check(name, case, got, ref64, ref32, extra=None):
    """``got`` (float32, cpu) against the float64 statement; bar = 4 * e32 + 1e-6 * peak (+ ``extra``, a tensor that broadcasts against ``got``)."""
    ref64 = ref64.double()
    diff = (got.double() - ref64).abs()
    err = float(diff.max()) if diff.numel() else 0.0
    e32 = float((ref32.double() - ref64).abs().max()) if diff.numel() else 0.0
    peak = float(ref64.abs().max()) if diff.numel() else 0.0
    bar = 4.0 * e32 + 1e-6 * peak
    more = "" if extra is None else f" +snake={float(extra.max()):.3e}"
    print(f"EDGE {name} {case} err={err:.3e} e32={e32:.3e} peak={peak:.3e} bar={bar:.3e}{more}")
    assert bool(torch.isfinite(got).all()), (name, case)
    over = diff - bar if extra is None else diff - bar - extra.double()
    assert diff.numel() == 0 or float(over.max()) <= 0.0, (name, case, err, e32, bar)
    return err, e32


def sentinel_like(*shape):
    return torch.full(shape, SENTINEL, device=DEV)


def is_sentinel(t):
    return bool((t == SENTINEL).all())


# ----------------------------------------------------------------------------------------------------------------- rmsnorm
RMS_SHAPES = [(1, 1, 4), (1, 5, 252), (2, 5, 256), (3, 3, 260), (3, 7, 1280), (1, 9, 4096)]


# measured on an MI355X, worst over the 56 comparisons (absolute): kernel 1.08e-6, e32 1.28e-6; closest to its bar (2, 5, 256) with weight, ragged: 6.6e-7
# against 8.0e-6, 0.08 of the bar.
@pytest.mark.parametrize("weight", [True, False])
@pytest.mark.parametrize("B,L,C", RMS_SHAPES)
def test_rmsnorm_edges(ops, B, L, C, weight):
    """mi355_rmsnorm (one wave per row, four rows per workgroup, float4 lanes in rounds of 256 columns):
    - C = 4 (one live lane), 252 / 256 / 260 (one lane short of a round, exactly one, one lane into the second), 1280 (five rounds), 4096 (sixteen);
    - B * L = 1, 5, 10, 9, 21, 9: never a multiple of 4, so the last workgroup has dead waves (``row >= B * L``);
    - weight on and off (``weight = None``: the multiply by 1);
    - no lens, and ragged lens with an item of length 0 ([0], [L // 2 + 1, 0], [L, 0, 1]): rows >= lens[b] keep the sentinel;
    - x a [:, :, :C] slice of a buffer 8 columns wider (ldx > C), y the [:, :L, :C] corner of a sentinel-filled [B, L + 2, C + 12] buffer
      (ldy > C, y_bstride > L * ldy): everything outside the view keeps the sentinel;
    - in place (y = x), the way the stacks call it."""
    g = torch.Generator().manual_seed(7 * C + B)
    eps = 1e-6
    x = torch.randn(B, L, C, generator=g) * 1.5 + 0.25
    w = torch.randn(C, generator=g) if weight else None
    xbuf0 = torch.randn(B, L, C + 8, generator=g)
    xbuf0[:, :, :C] = x
    xbuf = xbuf0.to(DEV)
    wd = None if w is None else w.to(DEV)
    ref64, ref32 = S.rmsnorm_stmt(x, w, eps, torch.float64), S.rmsnorm_stmt(x, w, eps, torch.float32)
    ragged = {1: [0], 2: [L // 2 + 1, 0], 3: [L, 0, 1]}[B]
    for lens in (None, ragged):
        ybuf = sentinel_like(B, L + 2, C + 12)
        ops.rmsnorm(xbuf[:, :, :C], ybuf[:, :L, :C], wd, eps=eps, lens=None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV))
        torch.cuda.synchronize()
        got = ybuf.cpu()
        assert torch.equal(xbuf.cpu(), xbuf0)
        assert is_sentinel(got[:, L:]) and is_sentinel(got[:, :, C:])
        for b in range(B):
            n = L if lens is None else lens[b]
            check("rmsnorm", (B, L, C, weight, "ragged" if lens else "full", b), got[b, :n, :C], ref64[b, :n], ref32[b, :n])
            assert is_sentinel(got[b, n:])
    z = xbuf[:, :, :C]
    ops.rmsnorm(z, z, wd, eps=eps)
    torch.cuda.synchronize()
    got = xbuf.cpu()
    check("rmsnorm", (B, L, C, weight, "in place"), got[:, :, :C], ref64, ref32)
    assert torch.equal(got[:, :, C:], xbuf0[:, :, C:])


# ----------------------------------------------------------------------------------------------------------------- head_norm_rope
ROPE_ROWS = 32


# measured on an MI355X, worst over the 248 comparisons (absolute): kernel 8.9e-7, e32 1.33e-6; closest to its bar dh 64, interleaved, norm + rope, "pos0_sub":
# 8.8e-7 (e32 3.8e-7) against 6.6e-6, 0.13 of the bar.
@pytest.mark.parametrize("mode", ["norm+rope", "rope", "norm"])
@pytest.mark.parametrize("interleaved", [False, True], ids=["rotate-half", "interleaved"])
@pytest.mark.parametrize("dh", [64, 128])
def test_head_norm_rope_edges(ops, dh, interleaved, mode):
    """mi355_head_norm_rope (one wave per (row, head), four per workgroup), dh 64 / 128 x rotate-half / interleaved x norm + rope / rope only / norm only
    (``cos = None``).  Reference: per-head RMSNorm, then oracle.lm_ref.apply_rope on rows of the float32 rope_tables upcast to float64, so only the
    kernel's arithmetic is measured.  Tables of 32 rows.
    - "tiny": B = 1, L = 3, heads = 1, no second tensor: 3 waves, a partly filled workgroup; pos0 = 5;
    - "ragged": B = 3, L = 5, heads = 2, lens = [5, 0, 2]: rows >= lens[b] and the 8 columns behind the heads keep the sentinel; x is a slice of a
      wider buffer;
    - "pos": explicit positions [B, L + 3] (pos_ld > L), non-monotonic;
    - "pos_sub": explicit positions minus the left padding, falling below 0 and above rope_rows - 1: rows 0 and 31 of the tables, as the header
      states; and "pos0_sub": host positions pos0 + l = 28 .. 31 minus pos_sub = [30, 0, 2];
    - "second": a second tensor with its own ldx2, heads2 = 1, written into the middle third of a sentinel-filled cache slot (7 waves per row);
    - "nw2-none" / "nw1-none" (modes with norm): the second tensor's norm weight absent while the first has one, and the reverse."""
    from oracle.lm_ref import StackConfig, rope_tables

    cfg = StackConfig(d_model=64, n_layers=1, n_heads=2, n_kv_heads=2, head_dim=dh, d_ff=64, rope_theta=10000.0, max_pos=ROPE_ROWS)
    cos, sin = rope_tables(cfg)
    rope, norm = mode != "norm", mode != "rope"
    cosd, sind = (cos.to(DEV), sin.to(DEV)) if rope else (None, None)
    g = torch.Generator().manual_seed(dh + 2 * interleaved + 11 * len(mode))
    eps = 1e-6
    tag = (dh, "il" if interleaved else "rh", mode)

    def run(name, B, L, heads, lens=None, pos=None, pos0=0, pos_sub=None, second=False, nw1=norm, nw2=norm):
        D = heads * dh
        x = torch.randn(B, L, D + 16, generator=g)
        nw = torch.randn(dh, generator=g) if nw1 else None
        ybuf = sentinel_like(B, L, D + 8)
        kw, x2, nwk, slot = {}, None, None, None
        if second:
            x2 = torch.randn(B, L, dh + 16, generator=g)
            nwk = torch.randn(dh, generator=g) if nw2 else None
            slot = sentinel_like(B, L, 3 * dh)
            kw["second"] = (x2.to(DEV)[:, :, :dh], slot[:, :, dh:2 * dh], 1, None if nwk is None else nwk.to(DEV))
        i32 = lambda v: None if v is None else torch.tensor(v, dtype=torch.int32, device=DEV)   # noqa: E731
        ops.head_norm_rope(x.to(DEV)[:, :, :D], ybuf[:, :, :D], heads=heads, dh=dh, norm_weight=None if nw is None else nw.to(DEV), eps=eps, cos=cosd,
                           sin=sind, pos=i32(pos), pos0=pos0, interleaved=interleaved, lens=i32(lens), pos_sub=i32(pos_sub), **kw)
        torch.cuda.synchronize()
        p = S.rope_positions(B, L, ROPE_ROWS, pos=None if pos is None else torch.tensor(pos), pos0=pos0, pos_sub=None if pos_sub is None else torch.tensor(pos_sub))
        ct, st = (cos, sin) if rope else (None, None)
        got = ybuf.cpu()
        assert is_sentinel(got[:, :, D:])
        outs = [("q", got[:, :, :D], x, heads, nw)]
        if second:
            gs = slot.cpu()
            assert is_sentinel(gs[:, :, :dh]) and is_sentinel(gs[:, :, 2 * dh:])
            outs.append(("k", gs[:, :, dh:2 * dh], x2, 1, nwk))
        for which, o, xin, h, wgt in outs:
            r64 = S.head_norm_rope_ref(xin, h, dh, wgt, eps, ct, st, p, interleaved, torch.float64)
            r32 = S.head_norm_rope_ref(xin, h, dh, wgt, eps, ct, st, p, interleaved, torch.float32)
            for b in range(B):
                n = L if lens is None else lens[b]
                check("head_norm_rope", tag + (name, which, b), o[b, :n], r64[b, :n], r32[b, :n])
                assert is_sentinel(o[b, n:])
        return p

    run("tiny", 1, 3, 1, pos0=5)
    run("ragged", 3, 5, 2, lens=[5, 0, 2])
    run("second", 2, 3, 6, pos0=3, second=True)
    if rope:
        run("pos", 2, 4, 2, pos=[[9, 2, 31, 0, 99, 99, 99], [17, 17, 1, 30, 99, 99, 99]])
        p = run("pos_sub", 3, 4, 2, pos=[[0, 1, 2, 3], [30, 31, 32, 35], [40, 3, 50, 2]], pos_sub=[2, 0, 4], second=True)
        assert p.tolist() == [[0, 0, 0, 1], [30, 31, 31, 31], [31, 0, 31, 0]]
        p = run("pos0_sub", 3, 4, 1, pos0=28, pos_sub=[30, 0, 2])
        assert p.tolist() == [[0, 0, 0, 1], [28, 29, 30, 31], [26, 27, 28, 29]]
    if norm:
        run("nw2-none", 2, 3, 2, pos0=1, second=True, nw1=True, nw2=False)
        run("nw1-none", 2, 3, 2, pos0=1, second=True, nw1=False, nw2=True)


# ----------------------------------------------------------------------------------------------------------------- swiglu
GATES = [0.0, -100.0, 100.0, 1e-30, -1e-30, 20.0, -20.0]


# measured on an MI355X, worst over the cases: kernel 3.81e-6, e32 3.81e-6 (the gate of 100, peak ~ 1e2); at most 0.035 of the bar (1.3e-6 against 3.75e-5).
@pytest.mark.parametrize("I,B,L", [(1, 1, 5), (1, 2, 128), (3, 1, 100), (96, 1, 8), (96, 2, 5), (257, 1, 3)])
def test_swiglu_edges(ops, I, B, L):
    """mi355_swiglu (one thread per output, 256 per workgroup): rows * I = 5 (below a workgroup), 256 and 768 (exactly one and three), 300, 960 and 771
    (a partly filled last workgroup; I = 3 and 257 put row boundaries inside a wave).  x is a [:, :, :2I] slice of a buffer 6 columns wider
    (ldx > 2I), y a [:, :, :I] slice of a sentinel-filled buffer 3 columns wider (ldy > I).  The first gates are 0, -100, 100, +-1e-30, +-20: outputs
    must be finite (expf(100) overflows to +inf; silu(-100) * u is then -0 against -3.7e-42 * u, compared in absolute terms like everything else)."""
    g = torch.Generator().manual_seed(I * 1000 + L)
    x = torch.randn(B, L, 2 * I, generator=g)
    n = min(len(GATES), B * L * I)
    x.view(-1, 2)[:n, 0] = torch.tensor(GATES[:n])
    xbuf = torch.randn(B, L, 2 * I + 6, generator=g)
    xbuf[:, :, :2 * I] = x
    ybuf = sentinel_like(B, L, I + 3)
    ops.swiglu(xbuf.to(DEV)[:, :, :2 * I], ybuf[:, :, :I])
    torch.cuda.synchronize()
    got = ybuf.cpu()
    assert is_sentinel(got[:, :, I:])
    check("swiglu", (I, B, L), got[:, :, :I], S.swiglu_stmt(x, torch.float64), S.swiglu_stmt(x, torch.float32))


# ----------------------------------------------------------------------------------------------------------------- embed_sum
EMBED_CASES = [(Q, 64) for Q in (1, 7, 8, 9, 16, 17, 33)] + [(9, C) for C in (4, 1024, 1028, 2052)]


# measured on an MI355X: all 88 comparisons bit-equal.
@pytest.mark.parametrize("Q,C", EMBED_CASES)
def test_embed_sum_edges(ops, Q, C):
    """mi355_embed_sum (one workgroup per row, slots in blocks of eight with a clamped tail, float4 lanes in rounds of 1024 columns):
    - Q = 1, 7 (a block of clamped tail slots), 8 (exactly one block), 9 (one slot into the second), 16, 17, 33 (CSM: four full blocks and one slot);
    - C = 4 (one lane), 1024 (exactly one round), 1028 (one lane into the second), 2052 (one into the third); the table's rows are 4 floats longer;
    - masks (-1) in the first slot of a row, in the last slot of another, in every slot of a third;
    - "full": slot_offset, add (rows 4 floats longer), scale 0.5, lens = [3, 1], ids a permuted [B, Q, L] tensor (qstride = L);
    - "bare": none of them, scale 0 (means 1), contiguous ids: the all-masked row comes back as zeros;
    - "alias": add aliasing y with a negated table, scale 1 (the DAC / SNAC residual update);
    - "column": ids one column of a wider int32 tensor, ``row[:, i:i + 1].unsqueeze(1)`` as the talkers pass it (L = Q = 1).
    y is the [:, :L, :C] corner of a sentinel-filled [B, L + 1, C + 8] buffer.  Bar: bit-equal to the float32 statement (acc = add, the slots
    ascending with one float32 add each, one multiply by scale)."""
    g = torch.Generator().manual_seed(Q * 10000 + C)
    B, L, rows = 2, 3, 11
    tbuf = torch.randn(rows * Q, C + 4, generator=g)
    table = tbuf[:, :C]
    ids_ql = torch.randint(0, rows, (B, Q, L), generator=g, dtype=torch.int32)
    ids_ql[0, 0, 0] = -1
    ids_ql[0, Q - 1, 1] = -1
    ids_ql[1, :, 2] = -1
    ids = ids_ql.permute(0, 2, 1)          # [B, L, Q]
    offs = torch.arange(Q, dtype=torch.int32) * rows
    abuf = torch.randn(B, L, C + 4, generator=g)
    add = abuf[:, :, :C]
    td, idsd = tbuf.to(DEV)[:, :C], ids_ql.to(DEV).permute(0, 2, 1)
    assert idsd.stride(2) == L

    def finish(name, ybuf, want, lens=None):
        torch.cuda.synchronize()
        got = ybuf.cpu()
        assert is_sentinel(got[:, want.shape[1]:]) and is_sentinel(got[:, :, C:])
        for b in range(B):
            n = want.shape[1] if lens is None else lens[b]
            diff = float((got[b, :n, :C] - want[b, :n]).abs().max())
            print(f"EDGE embed_sum {(Q, C, name, b)} err={diff:.3e} e32=0 peak={float(want[b, :n].abs().max()):.3e} bar=0 (bit-equal)")
            assert torch.equal(got[b, :n, :C], want[b, :n]), (Q, C, name, b, diff)
            assert is_sentinel(got[b, n:want.shape[1]])

    ybuf = sentinel_like(B, L + 1, C + 8)
    ops.embed_sum(td, idsd, ybuf[:, :L, :C], slot_offset=offs.to(DEV), add=abuf.to(DEV)[:, :, :C], scale=0.5, lens=torch.tensor([3, 1], dtype=torch.int32, device=DEV))
    finish("full", ybuf, S.embed_sum_stmt(table, ids, offs, add, 0.5, torch.float32), lens=[3, 1])

    ybuf = sentinel_like(B, L + 1, C + 8)
    ops.embed_sum(td, idsd.contiguous(), ybuf[:, :L, :C], scale=0.0)
    want = S.embed_sum_stmt(table, ids, None, None, 0.0, torch.float32)
    assert float(want[1, 2].abs().max()) == 0.0
    finish("bare", ybuf, want)

    ybuf = sentinel_like(B, L + 1, C + 8)
    ybuf[:, :L, :C] = add.to(DEV)
    neg = (-tbuf).to(DEV)[:, :C]
    ops.embed_sum(neg, idsd, ybuf[:, :L, :C], slot_offset=offs.to(DEV), add=ybuf[:, :L, :C])
    finish("alias", ybuf, S.embed_sum_stmt(-table, ids, offs, add, 1.0, torch.float32))

    wide = torch.randint(0, rows, (B, 5), generator=g, dtype=torch.int32)
    col = wide.to(DEV)[:, 3:4].unsqueeze(1)
    assert tuple(col.shape) == (B, 1, 1) and col.stride(0) == 5
    ybuf = sentinel_like(B, 2, C + 8)
    ops.embed_sum(td, col, ybuf[:, :1, :C], scale=1.0)
    finish("column", ybuf, S.embed_sum_stmt(table, wide[:, 3:4].unsqueeze(1), None, None, 1.0, torch.float32))


# ----------------------------------------------------------------------------------------------------------------- dwconv
def run_dwconv(ops, c, name):
    """One launch of ops.dwconv on channel-slice views: x is columns 2 .. 2 + C of a random buffer 6 columns wider (rows past lens_in[b] hold data
    that must not be read into a result), y rows 0 .. Lout, columns 3 .. 3 + C of a sentinel-filled [B, Lout + 2, C + 5] buffer."""
    x, w, bias, alpha, inv = S.dwconv_inputs(c)
    B, Lin, C, Lout = c["B"], c["Lin"], c["C"], c["Lout"]
    xbuf = torch.randn(B, Lin, C + 6, generator=torch.Generator().manual_seed(Lin))
    xbuf[:, :, 2:2 + C] = x
    ybuf = sentinel_like(B, Lout + 2, C + 5)
    lens = c["lens"]
    transpose = "stride" in c
    kw = dict(stride=c["stride"], transpose=True) if transpose else dict(dil=c["dil"], pre_alpha=None if alpha is None else alpha.to(DEV),
                                                                          pre_inv=None if inv is None else inv.to(DEV))
    ops.dwconv(xbuf.to(DEV)[:, :, 2:2 + C], w.to(DEV), None if bias is None else bias.to(DEV), ybuf[:, :Lout, 3:3 + C], pad=c["pad"],
               lens_in=None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV), **kw)
    torch.cuda.synchronize()
    got = ybuf.cpu()
    assert is_sentinel(got[:, Lout:]) and is_sentinel(got[:, :, :3]) and is_sentinel(got[:, :, 3 + C:])
    if transpose:
        args = dict(stride=c["stride"], pad=c["pad"], Lout=Lout, lens_in=lens)
        r64, r32 = S.dwconv_t_ref(x, w, bias, dtype=torch.float64, **args), S.dwconv_t_ref(x, w, bias, dtype=torch.float32, **args)
        extra = None
    else:
        args = dict(pad=c["pad"], dil=c["dil"], Lout=Lout, lens_in=lens, alpha=alpha, inv=inv)
        r64, r32 = S.dwconv_stmt(x, w, bias, dtype=torch.float64, **args), S.dwconv_stmt(x, w, bias, dtype=torch.float32, **args)
        extra = None if alpha is None else (w.double().abs().sum(1) * 2.0 * DELTA_SIN / alpha.double())[None, None, :]
    return check(name, S.dwconv_id(c), got[:, :Lout, 3:3 + C], r64, r32, extra)


# measured on an MI355X, worst over the cases (absolute).  Plain: kernel 1.76e-6, e32 2.30e-6, at most 0.082 of the bar (dil 9, L = 149: 1.5e-6 against 1.8e-5).
# Snake on the hardware sine: kernel 1.98e-6, e32 2.81e-6, at most 0.039 of the bar with its sine term (1.8e-6 against 4.6e-5): at |alpha x| <= ~7 rad the
# hardware sine does not show above the float32 noise of the taps.
@pytest.mark.parametrize("c", S.comb_cases(), ids=S.dwconv_id)
def test_dwconv_comb_edges(ops, c):
    """mi355_dwconv, K = 7 plain: dwconv7_comb_kernel<8> (eight outputs n0 + j * dil per thread, Snake on the hardware sine).  Cases: _lm_row_cases.comb_cases
    -- dil 1 / 3 / 9 (and 0 = 1) x Snake on / off x same-length at L = 1, 7, 8 dil, 8 dil + 1, 16 dil + 5 (Lout not a multiple of 8 dil: the ``n >= Lout``
    break), causal (pad 6 dil), valid (pad 0, Lout = Lin - 6 dil), Lout < dil (phases with no output), C = 1 / 40 / 64 / 70, B = 3 with lens_in =
    [L, 0, 2] (2 < pad), bias = None."""
    run_dwconv(ops, c, "dwconv.comb")


# measured on an MI355X, worst over the cases (absolute).  Plain: kernel 8.5e-7, e32 1.26e-6, at most 0.066 of the bar.  Snake on sinf: kernel 1.13e-6, e32 1.29e-6,
# at most 0.027 of the bar with its sine term (the comb path's hardware sine: 0.039, above).
@pytest.mark.parametrize("c", S.generic_cases(), ids=S.dwconv_id)
def test_dwconv_generic_edges(ops, c):
    """mi355_dwconv, K != 7 plain: dwconv_kernel with K = 1 / 3 / 5 / 9, dil 1 / 2, Snake on (sinf, a different sine from the comb path: same bar, and it
    must come in far below it) / off, lens_in = [13, 4]."""
    run_dwconv(ops, c, "dwconv.generic")


# measured on an MI355X, worst over the cases: kernel 5.1e-7, e32 6.6e-7, at most 0.049 of the bar.
@pytest.mark.parametrize("c", S.transposed_cases(), ids=S.dwconv_id)
def test_dwconv_transposed_edges(ops, c):
    """mi355_dwconv, transposed: (K, stride, pad, Lout) = (4, 2, 0, 2 Lin) (Mimi), (4, 2, 0, 2 Lin + 2) (the whole tail), (2, 2, 0, 2 Lin), (3, 1, 1, Lin),
    (8, 4, 2, 4 Lin), (5, 3, 0, 3 Lin + 2); with bias, and without bias at lens_in = [Lin, 1, 0].  Reference: F.conv_transpose1d in float64, trimmed /
    padded to Lout."""
    run_dwconv(ops, c, "dwconv.transposed")


# ----------------------------------------------------------------------------------------------------------------- refusals
def test_refusals(ops):
    """Arguments the entry points refuse before any launch: the outputs keep their sentinel."""
    from mlx_audio_amd import _lib

    E = _lib.Mi355Error
    f = lambda *s: torch.zeros(*s, device=DEV)   # noqa: E731
    y = sentinel_like(1, 2, 8)
    with pytest.raises(E, match="multiple of 4"):
        ops.rmsnorm(f(1, 2, 8)[:, :, :6], y[:, :, :6], None)
    ya = sentinel_like(1, 2, 128)
    cos, sin = f(8, 48), f(8, 48)
    with pytest.raises(E, match="64 or 128"):
        ops.head_norm_rope(f(1, 2, 96), ya[:, :, :96], heads=1, dh=96, cos=cos, sin=sin)
    cos, sin = f(8, 32), f(8, 32)
    with pytest.raises(ValueError, match="run past"):
        ops.head_norm_rope(f(1, 2, 64), ya[:, :, :64], heads=1, dh=64, cos=cos, sin=sin, pos0=7)
    x = f(1, 2, 64)
    base = dict(x=x.data_ptr(), x_bstride=128, ldx=64, heads=1, dh=64, L=2, B=1, eps=1e-6, y=ya.data_ptr(), y_bstride=256, ldy=128, rope_rows=8)
    with pytest.raises(E, match="run past"):   # the same check at the ABI
        _lib.call_struct("mi355_head_norm_rope", "mi355_head_rope_args", ops._stream(), cos_table=cos.data_ptr(), sin_table=sin.data_ptr(), pos0=7, **base)
    with pytest.raises(E, match="come together"):
        _lib.call_struct("mi355_head_norm_rope", "mi355_head_rope_args", ops._stream(), cos_table=cos.data_ptr(), **base)
    with pytest.raises(E, match="bad shape"):
        ops.embed_sum(f(4, 8)[:, :6], torch.zeros(1, 2, 1, dtype=torch.int32, device=DEV), y[:, :, :6])
    out = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    with pytest.raises(E, match="vocabulary"):
        ops.sample(f(1, 8193), out)
    with pytest.raises(E, match="top_p / min_p"):
        ops.sample(f(1, 64), out, temperature=0.9, top_p=1.5)
    with pytest.raises(E, match="top_p / min_p"):
        ops.sample(f(1, 64), out, temperature=0.9, min_p=-0.1)
    xc, w, al = f(1, 6, 8), f(8, 4), f(8) + 1.0
    yc = sentinel_like(1, 12, 8)
    with pytest.raises(E, match="plain depthwise conv only"):
        ops.dwconv(xc, w, None, yc, stride=2, transpose=True, dil=2)
    with pytest.raises(E, match="plain depthwise conv only"):
        ops.dwconv(xc, w, None, yc, stride=2, transpose=True, pre_alpha=al, pre_inv=al)
    with pytest.raises(E, match="pre_alpha without pre_inv"):
        ops.dwconv(xc, w, None, yc[:, :6], pad=1, pre_alpha=al)
    with pytest.raises(E, match="no stride"):   # the kernel has no stride for the plain conv; it used to be ignored silently
        ops.dwconv(xc, w, None, yc[:, :3], pad=1, stride=2)
    torch.cuda.synchronize()
    assert is_sentinel(y) and is_sentinel(ya) and is_sentinel(yc) and int(out[0]) == -7


# ----------------------------------------------------------------------------------------------------------------- sampler
# measured on an MI355X: 44 cases, no survivor pattern differs, every finite filtered value bit-equal to the oracle's (value error 0), every token equal.
@pytest.mark.parametrize("spec", S.sampler_specs(), ids=lambda s: s["name"])
def test_sampler_edges(ops, spec):
    """mi355_sample against oracle/sampling_ref.py (pinned to the reference's own chain).  Cases: _lm_row_cases.sampler_specs --
    - V = 1, 2, 63 / 64 / 65 (wave edge), 1023 / 1024 / 1025 (block edge), 4100, 8192 (kMaxV: all eight kill[] slots) at the reference defaults;
      V = 65 / 1025 / 8192 at the other parameter sets of SAMPLE_CASES (the greedy one included);
    - top_k = 1, V - 1, V, V + 5 (the last two: off); five equal values straddling the k-th place with two places left (the serial tid == 0 branch:
      the two lowest indices survive) and with five places left; all but three entries suppressed under top_k = 50;
    - top_p = 0.01, 0.999, 0.0 / 1.0 (off); min_p = 1.0 (the maximum and its exact ties); temperature = 1.0;
    - two equal logits at top_p = 0.5: the lower index's cumulative probability equals 1 - top_p exactly and the strict ``>`` drops it;
    - gumbel = None with temperature > 0 (the arg-max of the filtered row); history through n_hist without hist_len; a 3000-entry history with
      duplicates and ids >= V; done rows.
    Every case: logits of scale 1 (one exception, explained at _lm_row_cases.WIDE_SCALE) in a [B, V + 5] buffer whose padding columns hold +1e30, ``filtered``
    and the other columns of the int32 [B, 17] ``out`` buffer filled with sentinels that must survive; ``out`` is column 5 of that buffer, the way
    every engine calls it.  The input preconditions (tests/_lm_row_cases.py::sampler_preconditions; also asserted on the CPU by
    tests/test_lm_row_refs_cpu.py) are asserted first and fail rather than skip: with them no entry is excluded from any comparison."""
    case = S.build_case(spec)
    margins = S.sampler_preconditions(case)
    expf, exp_tok = S.oracle_run(case)
    V, B, kw = case["V"], case["B"], case["kw"]
    ld = V + 5
    lgd = torch.full((B, ld), 1e30)
    lgd[:, :V] = case["logits"]
    args = dict(V=V, filtered=sentinel_like(B, ld), **kw)
    if case["gumbel"] is not None:
        gd = torch.zeros(B, ld)
        gd[:, :V] = case["gumbel"]
        args["gumbel"] = gd.to(DEV)
    if case["suppress"]:
        sm = torch.zeros(V)
        sm[case["suppress"]] = -float("inf")
        args["suppress_mask"] = sm.to(DEV)
    if case["hist"] is not None:
        H = max(1, max(len(h) for h in case["hist"]))
        hd = torch.full((B, H), -1, dtype=torch.int32)
        for b, h in enumerate(case["hist"]):
            hd[b, :len(h)] = torch.tensor(h, dtype=torch.int32)
        args["history"] = hd.to(DEV)
        if case["hist_mode"] == "n":
            assert all(len(h) == H for h in case["hist"])
            args["n_hist"] = H
        else:
            args["hist_len"] = torch.tensor([len(h) for h in case["hist"]], dtype=torch.int32, device=DEV)
    if case.get("done"):
        args.update(done=torch.tensor(case["done"], dtype=torch.int32, device=DEV), done_token=case["done_token"])
    outbuf = torch.full((B, 17), -7, dtype=torch.int32, device=DEV)
    ops.sample(lgd.to(DEV), outbuf[:, 5], **args)
    torch.cuda.synchronize()
    filt = args["filtered"].cpu()
    got, tok = filt[:, :V], outbuf.cpu()
    fin = torch.isfinite(expf)
    diff = float((got[fin] - expf[fin]).abs().max())
    flips = int((torch.isinf(got) != torch.isinf(expf)).sum())
    print(f"EDGE sample {spec['name']} survivors/row>={margins['alive']} pattern_flips={flips} value_err={diff:.3e} bar=rtol 2e-6 + 1e-6 "
          f"tokens={tok[:, 5].tolist()} want={exp_tok.tolist()} margins={margins}")
    assert is_sentinel(filt[:, V:])
    assert bool((tok[:, :5] == -7).all()) and bool((tok[:, 6:] == -7).all())
    assert flips == 0, "filter pattern differs"
    torch.testing.assert_close(got[fin], expf[fin], rtol=2e-6, atol=1e-6)
    assert tok[:, 5].tolist() == exp_tok.tolist()
    for key, want in (("alive", True), ("dead", False)):
        if case[key] is not None:
            assert bool((torch.isfinite(got[:, case[key]]) == want).all()), (spec["name"], key)
