"""Dispatch-branch parity of the recurrence and search kernels: mi355_lstm_bidir (csrc/lstm.hip), mi355_lstm_seq (csrc/lstm_seq.hip and the LSTM epilogue
of csrc/gemm_rows.hip), mi355_aa_activation (csrc/glue.hip) and mi355_rvq_encode (csrc/rvq.hip).

The model tests call these kernels at a handful of shapes under one global bound; this file walks the launch branches those shapes do not reach (the
``lens == NULL`` branch, H = 32 on every image, items of length 0 / 1, the two-launch step at H % 64 != 0, bf16 images, the row-count switches of both
step forms, a K chunk tail, a second tile-group pass, every channel-tile class of the activation at its tile boundary, exact ties and partly filled
waves of the search, its ``!can`` fallback at large row counts).  It follows tests/test_lm_row_kernel_edges_gpu.py: every operation is stated in torch
from the formulas of include/mi355audio.h (tests/_seq_kernel_cases.py; tests/test_seq_kernel_refs_cpu.py holds the statements to the oracles, asserts
the preconditions of every case and shows that deliberately wrong statements miss these bars), evaluated in float64 (the reference) and in float32
on the CPU (``e32``, the statement's own rounding error), and the kernel is compared with the float64 result element by element.

Bars.  Float outputs: ``4 * e32 + 1e-6 * peak`` (docs/PARITY.md).  Added terms, each computed per case from the float64 trajectory:
(a) aa_activation: ``sum_k |fd[k]| * 2 * inv_beta[c] * 1e-6`` for the hardware sine (csrc/glue.hip: "~1e-6 absolute");
(b) lstm_seq on the matrix-pipe routes (gemm_rows in the one-launch form and from 9 rows on, gemv_mfma at 5 .. 8 rows with H % 64 == 0): the product
    sees h through a hi + lo split in the weights' type (csrc/linear_common.h split_hi_lo), which leaves at most w |h[k]| of h[k] behind, w = 2^-16
    (bf16) or 2^-22 (half; never less than one subnormal spacing 2^-24).  A pre-activation then moves by at most
    dpre[n] = sum_k |Wh[n, k]| (w |h[k]| + dh[k]), the gates by their derivatives (s (1 - s) dpre for a sigmoid, (1 - g^2) dpre for tanh),
    dc' = f dc + |c| df + |g| di + i dg and dh' = |tanh c'| do + o (1 - tanh^2 c') dc', carried from step to step with dh = dc = 0 at the start
    (_seq_kernel_cases.lstm_seq_stmt).
Outer caps: 5e-5 absolute (lstm_bidir), 2e-5 of the peak (lstm_seq on half images), 2e-5 * max(1, peak) (aa_activation); bf16 lstm_seq has no bar
in the project other than the derived one.  ``quant_h``: the 2e-5 of tests/test_kitten_gpu.py on cases whose margins the CPU file asserts, every
element compared.  rvq_encode: codes equal to the float64 statement, per frame in layer order up to (not including) the first decision whose float64
gap is below 1e-4 max|score| (at most 2 % of a case's decisions, asserted on the CPU); exact ties go to the lower index with a margin of exactly 0.
Outputs are views into larger buffers filled with an exactly representable sentinel: everything outside the view, and every row >= lens[b], must be
bit-equal to the sentinel afterwards.  Every comparison prints ``EDGE <kernel> <case> err e32 peak bar`` before it asserts (``pytest -s``).
"""

import math

import pytest
import torch

import _seq_kernel_cases as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from mlx_audio_amd import ops as _ops

    _ops.require_gpu()
    return _ops


DEV = "cuda"
SENTINEL = -777.25   # exactly representable; no kernel here produces it
F64 = torch.float64


def check(name, case, got, ref64, ref32, extra=None, cap=None, fixed_bar=None):
    """``got`` (float32, cpu) against the float64 statement, element by element: bar = 4 * e32 + 1e-6 * peak (+ ``extra``, a tensor that broadcasts
    against ``got``), or ``fixed_bar``; ``cap`` is the outer bound no element may exceed whatever the bar says."""
    if got.numel() == 0:
        return 0.0, 0.0
    ref64 = ref64.double()
    diff = (got.double() - ref64).abs()
    err = float(diff.max())
    e32, peak, bar = S.bar_of(ref64, ref32)
    if fixed_bar is not None:
        bar = fixed_bar
    full = torch.full_like(diff, bar) if extra is None else bar + extra.double().expand_as(diff)
    more = "" if extra is None else f" +term={float(extra.max()):.3e}"
    print(f"EDGE {name} {case} err={err:.3e} e32={e32:.3e} peak={peak:.3e} bar={bar:.3e}{more} of_bar={float((diff / full).max()):.3f}")
    assert bool(torch.isfinite(got).all()), (name, case)
    assert float((diff - full).max()) <= 0.0, (name, case, err, e32, bar)
    if cap is not None:
        assert err <= cap, (name, case, err, cap)
    return err, e32


def sentinel_like(*shape):
    return torch.full(shape, SENTINEL, device=DEV)


def is_sentinel(t):
    return bool((t == SENTINEL).all())


# ----------------------------------------------------------------------------------------------------------------- lstm_bidir
def run_bidir(ops, xp, img, H, lens, quant_h=False):
    """One launch on views: xp is columns 8 .. 8 + 8H of a [B, L + 1, 8H + 24] buffer (ldxp > 8H, xp_bstride > L * ldxp), out columns 16 .. 16 + 2H of a
    sentinel-filled [B, L + 2, 2H + 32] buffer (ldo = 2H + 32).  Returns the output view on the CPU after the sentinel checks."""
    B, L, _ = xp.shape
    xbuf = torch.randn(B, L + 1, 8 * H + 24, generator=torch.Generator().manual_seed(L))
    xbuf[:, :L, 8:8 + 8 * H] = xp
    obuf = sentinel_like(B, L + 2, 2 * H + 32)
    wh, f16, scale = img
    ops.lstm_bidir(xbuf.to(DEV)[:, :L, 8:8 + 8 * H], wh, H, obuf[:, :L, 16:16 + 2 * H], lens=None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV),
                   quant_h=quant_h, wh_f16=f16, wh_scale=scale)
    torch.cuda.synchronize()
    got = obuf.cpu()
    assert is_sentinel(got[:, L:]) and is_sentinel(got[:, :, :16]) and is_sentinel(got[:, :, 16 + 2 * H:])
    for b in range(B):
        n = L if lens is None else lens[b]
        assert is_sentinel(got[b, n:])
    return got[:, :L, 16:16 + 2 * H]


def lstm_images(ops, H, seed):
    """{image: ((device image, wh_f16, wh_scale), (Wh_forward, Wh_backward))}: bf16, IEEE half, and the bf16 values as a scaled half image."""
    bw, hw = S.lstm_weights(H, seed, "bf16"), S.lstm_weights(H, seed, "f16")
    scaled = ops.pack_lstm_wh_scaled(bw[0], bw[1], DEV)
    assert scaled is not None and scaled[1] > 0 and math.log2(scaled[1]) == round(math.log2(scaled[1]))
    return {"bf16": ((ops.pack_lstm_wh(bw[0], bw[1], DEV), False, 0.0), bw), "f16": ((ops.pack_lstm_wh(hw[0], hw[1], DEV, f16=True), True, 0.0), hw),
            "scaled": ((scaled[0], True, scaled[1]), bw)}


LSTM_KERNELS = [(H, oct) for H in S.LSTM_H for oct in (("1", "0") if H >= 64 else ("0",))]


# measured on an MI355X, worst over the 280 comparisons (absolute): kernel 1.68e-7, e32 1.27e-7; closest to its bar H = 64, octet kernel, B = 9, bf16 image: 1.68e-7
# against 9.6e-7, 0.17 of the bar.  The scaled-half image bit-equal to the bf16 image in all 42 launches; every item alone and every second run bit-equal.
@pytest.mark.parametrize("H,oct", LSTM_KERNELS, ids=[f"H{H}-{'oct' if o == '1' else 'plain'}" for H, o in LSTM_KERNELS])
def test_lstm_bidir_edges(ops, monkeypatch, H, oct):
    """mi355_lstm_bidir, both kernels (lstm_oct_kernel, the default for H >= 64; lstm_kernel under MI355_LSTM_OCT=0, the only one H = 32 has) x the
    bf16, IEEE-half and scaled-half images x _seq_kernel_cases.lstm_shapes():
    - L = 1 / 2 / 7 / 8 with ``lens = None`` (both directions at t = 0; the ``lens == NULL -> L`` branch of both kernels);
    - the ragged batch [9, 1, 0, 8, 2] at L = 9: rows >= lens[b], the whole item of length 0 and every column outside the output view keep the
      sentinel; each item is bit-equal to the same item run alone (B = 1, L = lens[b], no lens), and a second run is bit-equal to the first;
    - B = 9;
    - xp and out are column views of wider buffers with padded batch strides in every launch;
    - the scaled-half image is bit-equal to the bf16 image's output in every case, H = 32 included."""
    monkeypatch.setenv("MI355_LSTM_OCT", oct)
    imgs = lstm_images(ops, H, 0)
    for name, B, L, lens in S.lstm_shapes():
        xp = S.lstm_xp(H, B, L, 0)
        outs = {}
        for image in S.LSTM_IMAGES:
            img, (wf, wb) = imgs[image]
            got = outs[image] = run_bidir(ops, xp, img, H, lens)
            if image == "scaled":
                print(f"EDGE lstm_bidir {(H, oct, name, image)} err={float((got - outs['bf16']).abs().max()):.3e} e32=0 peak=- bar=0 (bit-equal to the bf16 image)")
                assert torch.equal(got, outs["bf16"]), (H, oct, name, "the scaled half image differs from the bf16 image")
                continue
            r64, r32 = S.lstm_bidir_stmt(xp, wf, wb, lens, F64), S.lstm_bidir_stmt(xp, wf, wb, lens, torch.float32)
            for b in range(B):
                n = L if lens is None else lens[b]
                check("lstm_bidir", (H, oct, name, image, b), got[b, :n], r64[b, :n], r32[b, :n], cap=5e-5)
            if name == "ragged":
                assert torch.equal(run_bidir(ops, xp, img, H, lens), got), (H, oct, image, "a second run differs")
                for b, n in enumerate(lens):
                    if n:
                        alone = run_bidir(ops, xp[b:b + 1, :n], img, H, None)
                        assert torch.equal(alone[0], got[b, :n]), (H, oct, image, b, "the item alone differs from the item in the batch")


# measured on an MI355X: worst of the 7 runs 9.5e-8 (H = 64, plain kernel) against 2e-5; scaled-half image bit-equal
QUANT_KERNELS = [(c, oct) for c in S.QUANT_TIGHT for oct in (("1", "0") if c[0] >= 64 else ("0",))]


@pytest.mark.parametrize("case,oct", QUANT_KERNELS, ids=[f"H{c[0]}-{'oct' if o == '1' else 'plain'}" for c, o in QUANT_KERNELS])
def test_lstm_bidir_quant_h_tight(ops, monkeypatch, case, oct):
    """``quant_h`` on the cases whose trajectories stay 2e-4 grid steps clear of every rounding boundary (margins asserted by the CPU file): every
    element within 2e-5 of the float64 statement, none excluded; the scaled-half image bit-equal to the bf16 one; and next to an item of length 1
    (its own extrema, its own backward start) the full item keeps its bits."""
    monkeypatch.setenv("MI355_LSTM_OCT", oct)
    H, In, L, seed = case
    _, _, xp, wf, wb = S.quant_case(H, In, L, seed)
    scaled = ops.pack_lstm_wh_scaled(wf, wb, DEV)
    assert scaled is not None
    img = (ops.pack_lstm_wh(wf, wb, DEV), False, 0.0)
    r64 = S.lstm_bidir_stmt(xp, wf, wb, None, F64, quant_h=True)
    r32 = S.lstm_bidir_stmt(xp, wf, wb, None, torch.float32, quant_h=True)
    got = run_bidir(ops, xp, img, H, None, quant_h=True)
    check("lstm_bidir.quant_h", (H, oct), got, r64, r32, fixed_bar=S.QUANT_BAR)
    assert torch.equal(run_bidir(ops, xp, (scaled[0], True, scaled[1]), H, None, quant_h=True), got)
    xp2 = torch.cat([xp, xp], 0)
    got2 = run_bidir(ops, xp2, img, H, [L, 1], quant_h=True)
    assert torch.equal(got2[0], got[0])
    check("lstm_bidir.quant_h", (H, oct, "len1"), got2[1, :1], S.lstm_bidir_stmt(xp2, wf, wb, [L, 1], F64, quant_h=True)[1, :1],
          S.lstm_bidir_stmt(xp2, wf, wb, [L, 1], torch.float32, quant_h=True)[1, :1], cap=5e-5)


# ----------------------------------------------------------------------------------------------------------------- lstm_seq
def run_seq(ops, c, wh, xproj, h0, c0):
    """One call of ops.lstm_seq; with ``view`` xproj is columns 4 .. 4 + 4H of a [B, T + 1, 4H + 12] buffer and out columns 8 .. 8 + H of a
    sentinel-filled [B, T + 2, H + 20] buffer.  Returns (out, h_T, c_T) on the CPU."""
    H, B, T, f16 = c["H"], c["B"], c["T"], c["image"] == "f16"
    if c["fused"]:
        img = ops.pack_lstm_seq_wh(wh, DEV, f16=f16)
        assert img.interleaved
    else:
        img = ops.pack_rowmajor16(wh, None, DEV, f16=f16)
        assert not img.interleaved
    if c["view"]:
        xbuf = torch.randn(B, T + 1, 4 * H + 12, generator=torch.Generator().manual_seed(T))
        xbuf[:, :T, 4:4 + 4 * H] = xproj
        xd = xbuf.to(DEV)[:, :T, 4:4 + 4 * H]
        obuf = sentinel_like(B, T + 2, H + 20)
        out = obuf[:, :T, 8:8 + H]
    else:
        xd = xproj.to(DEV)
        obuf = sentinel_like(B, T, H)
        out = obuf
    hT, cT = ops.lstm_seq(xd, img, out, h0=None if h0 is None else h0.to(DEV), c0=None if c0 is None else c0.to(DEV))
    torch.cuda.synchronize()
    got = obuf.cpu()
    if c["view"]:
        assert is_sentinel(got[:, T:]) and is_sentinel(got[:, :, :8]) and is_sentinel(got[:, :, 8 + H:])
        got = got[:, :T, 8:8 + H]
    return got, hT.cpu(), cT.cpu()


# measured on an MI355X, worst over the comparisons of out / h_T / c_T (absolute).  fp32 GEMV routes (81): kernel 3.6e-7, e32 3.6e-7, at most 0.13 of the bar.
# Matrix pipe, bf16 image (48): kernel 1.94e-6 (H = 64, B = 33, one launch, c_T; e32 3.0e-7: the float bar alone is 1.2e-6 there, the split of h shows) under a
# split term of up to 2.6e-5: at most 0.089 of bar + term.  Matrix pipe, half image (63): kernel 6.1e-7 (H = 2112, B = 33, c_T), e32 5.8e-7, at most 0.090 of
# bar + term; 3.8e-7 of the peak at most against the 2e-5 cap.
@pytest.mark.parametrize("c", S.seq_cases(), ids=S.seq_id)
def test_lstm_seq_edges(ops, c):
    """mi355_lstm_seq over _seq_kernel_cases.seq_cases(): the two-launch step at H = 8 / 24 / 72 / 200 (B = 1 / 4 / 8), both step forms at H = 64 across
    the row switches 8 | 9, 16 | 17, 32 | 33 and at 64 rows, the K chunk tail (B = 33, H = 320), the second tile-group pass (H = 2112), T = 1 / 2 / 5,
    carried h0 / c0, column views; bf16 and half images.  ``out``, ``h_T`` and ``c_T`` are all compared; bar and split term: the module docstring."""
    wh, xproj, h0, c0 = S.seq_inputs(c)
    f16 = c["image"] == "f16"
    mfma = S.seq_route(c["B"], c["H"], c["fused"]) == "mfma"
    width, floor = S.seq_split_term(f16)
    r64 = S.lstm_seq_stmt(xproj, wh, h0, c0, F64, split_width=width, split_floor=floor)
    r32 = S.lstm_seq_stmt(xproj, wh, h0, c0, torch.float32)
    got = run_seq(ops, c, wh, xproj, h0, c0)
    for k, what in enumerate(("out", "hT", "cT")):
        cap = 2e-5 * float(r64[k].abs().max()) if f16 else None
        check("lstm_seq", (S.seq_id(c), what, "mfma" if mfma else "fma"), got[k], r64[k], r32[k], extra=r64[3][k] if mfma else None, cap=cap)
    assert torch.equal(got[0][:, -1], got[1])   # the final state is the last output row, whichever buffer the last step wrote


def _seq_args(ops, B=2, T=2, H=64, gate_interleaved=0, h2="alloc", ld_out_short=False):
    t = dict(xproj=torch.zeros(B, T, 4 * H, device=DEV), wh=torch.zeros(4 * H, H, dtype=torch.int16, device=DEV), h=sentinel_like(B, H), c=sentinel_like(B, H),
             pre=sentinel_like(B, 4 * H), out=sentinel_like(B, T, H), h2=sentinel_like(B, H) if h2 == "alloc" else None)
    kw = dict(xproj=t["xproj"].data_ptr(), xproj_bstride=T * 4 * H, ld_xproj=4 * H, wh=t["wh"].data_ptr(), wdtype=ops.W_F16, h=t["h"].data_ptr(),
              c=t["c"].data_ptr(), pre=t["pre"].data_ptr(), out=t["out"].data_ptr(), out_bstride=T * H, ld_out=H - 8 if ld_out_short else H, B=B, T=T, H=H,
              gate_interleaved=gate_interleaved, h2=None if t["h2"] is None else t["h2"].data_ptr())
    return t, kw


@pytest.mark.parametrize("name,match,over", S.SEQ_REFUSALS, ids=[r[0] for r in S.SEQ_REFUSALS])
def test_lstm_seq_refusals(ops, name, match, over):
    """Arguments mi355_lstm_seq refuses before any launch (called through _lib.call_struct as ops.lstm_seq calls it, past the wrapper's own asserts):
    the error names the rule; out, h, c (and pre, h2) keep their sentinels."""
    from mlx_audio_amd import _lib

    t, kw = _seq_args(ops, **over)
    with pytest.raises(_lib.Mi355Error, match=match):
        _lib.call_struct("mi355_lstm_seq", "mi355_lstm_seq_args", ops._stream(), **kw)
    torch.cuda.synchronize()
    for k in ("out", "h", "c", "pre", "h2"):
        assert t[k] is None or is_sentinel(t[k]), (name, k)


# ----------------------------------------------------------------------------------------------------------------- aa_activation
# measured on an MI355X, worst over the 44 comparisons (absolute): kernel 1.61e-6, e32 1.59e-6 (C = 48, L = 255); closest to its bar C = 4, L = 511: 1.37e-6 against
# 7.8e-6 + a sine term of 2.7e-6, 0.13 of it.
@pytest.mark.parametrize("c", S.aa_cases(), ids=S.aa_id)
def test_aa_activation_edges(ops, c):
    """mi355_aa_activation over _seq_kernel_cases.aa_cases(): every channel-tile class (C = 4 / 24: aa_act_kernel<8> with and without dead lanes, 48: <16>,
    96: <32>, 12: the <64> fallback, 136: <64> with a ragged last channel tile) at T - 1 / T / T + 1 rows (T = 4096 / CT rows per workgroup), and a
    ragged batch [T + 1, T, 1, 2 T]: the item of length T meets the early return of its second tile, T + 1 gives a one-row last tile clamped on both
    sides.  x is columns 2 .. 2 + C of a wider buffer whose rows past lens[b] hold values that must not be read into a result; y columns 3 .. 3 + C
    of a sentinel-filled [B, L + 2, C + 5] buffer."""
    x, alpha, ib = S.aa_inputs(c)
    B, L, C, lens = c["B"], c["L"], c["C"], c["lens"]
    filt = S.aa_filter()
    xbuf = torch.randn(B, L + 1, C + 6, generator=torch.Generator().manual_seed(L)) * 50.0
    xbuf[:, :L, 2:2 + C] = x
    if lens is not None:
        for b, n in enumerate(lens):
            xbuf[b, n:L, 2:2 + C] = 1e4      # rows >= lens[b]: the edge clamp must stop at lens[b] - 1
    ybuf = sentinel_like(B, L + 2, C + 5)
    ops.aa_activation(xbuf.to(DEV)[:, :L, 2:2 + C], ybuf[:, :L, 3:3 + C], filt.to(DEV), filt.to(DEV), alpha.to(DEV), ib.to(DEV),
                      lens=None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    got = ybuf.cpu()
    assert is_sentinel(got[:, L:]) and is_sentinel(got[:, :, :3]) and is_sentinel(got[:, :, 3 + C:])
    r64 = S.aa_activation_stmt(x, filt, filt, alpha, ib, lens, F64)
    r32 = S.aa_activation_stmt(x, filt, filt, alpha, ib, lens, torch.float32)
    extra = S.aa_sine_term(filt, ib)[None, :]
    for b in range(B):
        n = L if lens is None else lens[b]
        peak = float(r64[b, :n].abs().max())
        check("aa_activation", (S.aa_id(c), b, n), got[b, :n, 3:3 + C], r64[b, :n], r32[b, :n], extra=extra, cap=2e-5 * max(1.0, peak))
        assert is_sentinel(got[b, n:])


def test_aa_activation_in_place_is_refused(ops):
    from mlx_audio_amd import _lib

    _, alpha, ib = S.aa_inputs(dict(C=48, B=1, L=9))
    filt = S.aa_filter().to(DEV)
    y = sentinel_like(1, 9, 48)
    with pytest.raises(_lib.Mi355Error, match="in-place"):
        ops.aa_activation(y, y, filt, filt, alpha.to(DEV), ib.to(DEV))
    torch.cuda.synchronize()
    assert is_sentinel(y)


# ----------------------------------------------------------------------------------------------------------------- rvq_encode
CODE_SENTINEL = -7


def run_rvq(ops, x, tables, c2, view, pad=3):
    """One call through _lib.call_struct with ld_codes = n_layers + ``pad``: (codes, margins) on the CPU after the pad columns' sentinel check.  ``view``:
    x is the [:, :D] corner of a [rows, D + 1] buffer (ldx = D + 1)."""
    from mlx_audio_amd import _lib

    rows, D = x.shape
    n, bins, _ = tables.shape
    if view:
        xbuf = torch.full((rows, D + 1), 1e4)
        xbuf[:, :D] = x
        xd = xbuf.to(DEV)[:, :D]
    else:
        xd = x.to(DEV)
    td, ttd, c2d = tables.to(DEV), tables.transpose(1, 2).contiguous().to(DEV), c2.to(DEV)
    codes = torch.full((rows, n + pad), CODE_SENTINEL, dtype=torch.int32, device=DEV)
    mg = sentinel_like(rows, n + pad)
    _lib.call_struct("mi355_rvq_encode", "mi355_rvq_encode_args", ops._stream(), x=xd.data_ptr(), rows=rows, ldx=xd.stride(0), D=D, tables=td.data_ptr(),
                     tables_t=ttd.data_ptr(), c2=c2d.data_ptr(), bins=bins, n_layers=n, codes=codes.data_ptr(), ld_codes=n + pad, margins=mg.data_ptr())
    torch.cuda.synchronize()
    codes, mg = codes.cpu(), mg.cpu()
    assert bool((codes[:, n:] == CODE_SENTINEL).all()) and is_sentinel(mg[:, n:])
    return codes[:, :n], mg[:, :n]


# measured on an MI355X: 26 cases, no compared code differs (98.05 % .. 100 % of a case's decisions compared), every tie to the lower index with margin 0; the margins'
# worst error equals the float32 statement's own in 23 cases, else at most 0.24 of the bar (D = 516: 1.6e-4 against 6.7e-4 at scores of up to 416).
@pytest.mark.parametrize("c", S.rvq_cases(), ids=lambda c: c["name"])
def test_rvq_encode_edges(ops, c):
    """mi355_rvq_encode over _seq_kernel_cases.rvq_cases(): bins 2 .. 1000, exact ties meeting in each of the three merges (per thread, wave shuffle,
    four waves) of both kernels, D = 1 / 3 / 6 / 516 on an ``ldx = D + 1`` view at 1025 and 4097 rows (the one-frame kernel whatever the row count),
    the R = 1 | 2 | 4 | 8 switches with ``nr < R`` tails.  ld_codes = n_layers + 3 in every call: the pad columns of codes and margins keep their
    sentinels.  Codes against rvq_stmt in float64 under the margin rule (the compared share is printed); margins of the compared decisions under the
    float bar, with peak = max|score|; the large calls bit-equal, codes and margins, to the same rows in calls of 700."""
    x, tables, c2 = S.rvq_inputs(c)
    codes, mg = run_rvq(ops, x, tables, c2, c["view"])
    want, gaps, peaks = S.rvq_stmt(x, tables, c2, F64)
    g32 = S.rvq_stmt(x, tables, c2, torch.float32)[1]
    if c["kind"] == "ties":
        n = len(S.RVQ_TIES)
        for rows in (slice(0, n), slice(x.shape[0] - n, x.shape[0])):
            assert codes[rows, 0].tolist() == [copies[0] for copies, _ in S.RVQ_TIES], "a tie did not go to the lower index"
            assert bool((mg[rows, 0] == 0.0).all()), "the margin of an exact tie is not 0"
        gaps = gaps.clone()
        gaps[:n, 0] = gaps[-n:, 0] = float("inf")
    cmp = S.rvq_compared(gaps, peaks)
    share = float(cmp.float().mean())
    wrong = int((codes.long() != want)[cmp].sum())
    fin = cmp & torch.isfinite(gaps)
    merr = (mg.double() - gaps)[fin].abs()
    e32 = (g32.double() - gaps)[fin].abs()
    bar = 4.0 * float(e32.max()) + 1e-6 * float(peaks.max())
    print(f"EDGE rvq_encode {c['name']} compared={share:.4f} wrong_codes={wrong} err={float(merr.max()):.3e} e32={float(e32.max()):.3e} "
          f"peak={float(peaks.max()):.3e} bar={bar:.3e}")
    assert share >= 1.0 - S.RVQ_CAP
    assert wrong == 0
    assert float(merr.max()) <= bar
    if c["chunks"]:
        parts = [run_rvq(ops, x[i:i + 700], tables, c2, c["view"]) for i in range(0, x.shape[0], 700)]
        assert torch.equal(torch.cat([p[0] for p in parts]), codes) and torch.equal(torch.cat([p[1] for p in parts]), mg)
