"""Dispatch-branch parity of the decode-side linear kernels: mi355_gemv (gemv1_stream / gemv1_splitk / gemv_kernel of csrc/gemv.hip, gemv_mfma.hip,
gemv_mfma_fp8.hip, gemm_rows.hip) and the row pipeline mi355_rows_gemm / mi355_rows_finish (csrc/rows_pipe.hip).

tests/test_transformer_kernels_gpu.py holds these kernels at the workloads' shapes with random inputs and a global-max relative bar; this file walks
the branches between those shapes.  Case tables, the restated dispatcher, reference statements and bounds live in tests/_linear_cases.py, and
tests/test_linear_refs_cpu.py holds them on the CPU (exact representability, the 2^24 budget, label coverage, both mutants).

1. Integer-exact cases: small integers in x, w and bias make every partial sum exactly representable whatever the order, so EVERY kernel family must
   be bit-equal (``torch.equal``) to the int64 product.  x rows and y are strided views; y is NaN-initialised inside a sentinel-filled buffer whose
   eight guard columns and guard row must stay untouched; M > 1 cases carry a zero input row and one power of two per row; M = 1 cases run under
   both weight-load policies; one case per family runs twice and must repeat bit for bit.  SwiGLU cases compare with the kernel's expression in
   float32 on the exact sums at 4 ulp.
2. Rounding cases: float inputs against float64, per element ``|got - want| <= bound[m, n]`` (the input split, the accumulation chain, the fused
   norm's two-pass statistics); each test prints ``LINEAR <what> <case> ratio=<largest error / bound>`` (``pytest -s``), none may exceed 1.
3. Refusals: every argument check a caller can trip returns MI355_ERR_ARG with a message and leaves the sentinel-filled outputs untouched.

The library's A/B knobs are read once per process: none may be set (asserted at import)."""
import ctypes
import os

import pytest
import torch

import _linear_cases as S

assert [k for k in S.ENV_KNOBS if k in os.environ] == [], "the A/B knobs of the linear kernels must be unset for this suite"

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN16 = {False: 0x7FC0, True: 0x7E00}   # a NaN of the planes' element type


@pytest.fixture(scope="module")
def ops():
    from mlx_audio_amd import ops as _ops

    _ops.require_gpu()
    return _ops


def image(ops, w, wt, bias=None):
    """The row-major weight image of float32 CPU weights that are exactly representable in it (asserted)."""
    if wt == "fp8":
        rw, wq = ops.pack_rowmajor_fp8(w, None, DEV)
        assert torch.equal(wq, w.float())
    else:
        rw = ops.pack_rowmajor16(w, None, DEV, f16=wt == "fp16")
        assert torch.equal(rw.w.cpu().view(torch.float16 if wt == "fp16" else torch.bfloat16).float(), w.float())
    rw.bias = None if bias is None else bias.float().to(DEV)
    return rw


def strided(x):
    """x [M, K] (CPU float32) as the [:, :K] view of a device buffer 8 columns wider whose pad holds NaN."""
    buf = torch.full((x.shape[0], x.shape[1] + 8), float("nan"), device=DEV)
    buf[:, : x.shape[1]] = x.to(DEV)
    return buf[:, : x.shape[1]]


def guarded(M, N):
    """(buffer, view): y is the NaN-filled [:M, :N] corner of a sentinel-filled [M + 1, N + 8] buffer."""
    buf = torch.full((M + 1, N + 8), S.SENTINEL, device=DEV)
    buf[:M, :N] = float("nan")
    return buf, buf[:M, :N]


def guards_untouched(buf, M, N):
    return bool((buf[M] == S.SENTINEL).all()) and bool((buf[:M, N:] == S.SENTINEL).all())


def glu_close(got, pre):
    want = S.glu_value32(pre)
    return bool(((got.double() - want.double()).abs() <= 4 * S.ulp32(want)).all())


# ----------------------------------------------------------------------------------------------------------------- 1. integer-exact, mi355_gemv
INT_CASES = S.int_cases()


@pytest.mark.parametrize("c", INT_CASES, ids=S.case_id)
def test_gemv_integer_exact(ops, c):
    """Every kernel family, bit-equal to the int64 product (the branch each case crosses is its ``branch`` entry in tests/_linear_cases.py)."""
    x, e, w, bias = S.int_inputs(c)
    M, N, K = c["M"], c["N"], c["K"]
    xs = (x.double() * torch.pow(2.0, e.double())[:, None]).float()
    ref = S.int_reference(x, e, w, bias)
    rw = image(ops, w.float(), c["wt"], bias)
    n_out = N // 2 if c["glu"] else N
    kw = dict(glu=c["glu"], use_bias=bias is not None)
    if c["x_ids"]:   # x is a table; the input row is table[x_ids[0] + x_id_offset]
        g = torch.Generator().manual_seed(K)
        table = torch.randint(-4, 5, (6, K), generator=g).float()
        table[4] = xs[0]
        xv = strided(table)
        kw.update(x_ids=torch.tensor([1], dtype=torch.int32, device=DEV), x_id_offset=3)
    else:
        xv = strided(xs)
    outs = []
    for pol in ((0, 1) if M == 1 else (0,)):
        for _ in range(2 if c["repeat"] else 1):
            buf, y = guarded(M, n_out)
            ops.gemv(xv, rw, y, w_policy=pol, **kw)
            torch.cuda.synchronize()
            assert guards_untouched(buf, M, n_out), (S.case_id(c), pol)
            outs.append(y.cpu())
    for got in outs:
        if c["glu"]:
            assert glu_close(got, ref), S.case_id(c)
        else:
            assert torch.equal(got, ref.float()), (S.case_id(c), int((got != ref.float()).sum()))
    for got in outs[1:]:   # both policies, and the repeat, bit for bit (NaN-free: compared above)
        assert torch.equal(got, outs[0]), S.case_id(c)


# ----------------------------------------------------------------------------------------------------------------- 1. integer-exact, the row pipeline
def decode_planes(planes, R, K, f16):
    """hi + lo planes (fragment order, see mi355audio.h) -> (hi, lo) float64 [R, K]."""
    raw = planes[: 2 * R * K].cpu().view(torch.float16 if f16 else torch.bfloat16).double().reshape(K // 64, 2, 2, 4, R, 8)
    return tuple(raw[:, i].permute(3, 0, 2, 1, 4).reshape(R, K) for i in (0, 1))   # column = 64 step + 16 group + 8 half + e


def nan_planes(ops, R, K, f16):
    p = ops.rows_planes(R, K, DEV)
    p.fill_(NAN16[f16])
    return p


def to_planes(ops, x, R, f16, norm=None):
    """fp32 rows -> planes by mi355_rows_finish as converter; the planes are NaN-filled first (rows >= M must never reach a stored result)."""
    M, K = x.shape
    p = nan_planes(ops, R, K, f16)
    ops.rows_finish(strided(x), M, K, planes=p, R=R, f16=f16, norm=norm)
    return p


ROWS_CASES = S.rows_cases()


@pytest.mark.parametrize("c", ROWS_CASES, ids=S.rows_case_id)
def test_rows_pipeline_integer_exact(ops, c):
    """rows_finish (converter) -> rows_gemm -> rows_finish, bit-equal to the int64 product: R 16 / 32 / 64 with M = 1, R - 1, R; 31 / 32 / 33 and
    2047 / 2048 tiles (T 1 -> 2 -> 4); kgroups 1, 2, mi355_rows_kgroups and the cap K / 256; all three tile images; lean and generic epilogue;
    SwiGLU in the epilogue and fused into the GEMM (planes out)."""
    x, e, w, bias = S.rows_inputs(c)
    R, M, N, K, wt = c["R"], c["M"], c["N"], c["K"], c["wt"]
    f16 = wt == "fp16"
    xs = (x.double() * torch.pow(2.0, e.double())[:, None]).float()
    ref = S.int_reference(x, e, w, bias)
    rm = image(ops, w.float(), wt, bias)
    tl = ops.tiles16_from_rowmajor(rm)
    planes = to_planes(ops, xs, R, f16)
    hi, lo = decode_planes(planes, R, K, f16)
    assert torch.equal(hi[:M], xs.double()) and bool((lo[:M] == 0).all()) and bool(torch.isnan(hi[M:]).all())
    if c["kg"] == "auto":
        assert ops.rows_kgroups(N, K) == S.rows_kgroups_stmt(N, K)
    kg = S.rows_kg(c)
    if c["fused"]:
        po = nan_planes(ops, R, N // 2, False)
        ops.rows_gemm(planes, tl, None, M, R, kgroups=1, glu_planes_out=po, glu_bias=rm.bias)
        torch.cuda.synchronize()
        ohi, olo = decode_planes(po, R, N // 2, False)
        assert bool(torch.isnan(ohi[M:]).all()) and bool(torch.isnan(olo[M:]).all())
        want = S.glu_value32(ref).double()
        # hi + lo of a float32 value in bf16: both images rounded to nearest, 2^-8 * 2^-8 of the value (or the smallest normal's share of it)
        assert bool(((ohi[:M] + olo[:M] - want).abs() <= 4 * S.ulp32(want) + 2.0 ** -16 * want.abs() + 2.0 ** -126).all())
        return
    ld = ops.round_up(N, 8) + 8
    part = torch.full((kg, M + 1, ld), S.SENTINEL, device=DEV)
    part[:, :M, :N] = float("nan")
    assert ops.rows_gemm(planes, tl, part, M, R, kgroups=kg) == kg
    torch.cuda.synchronize()
    assert bool((part[:, M] == S.SENTINEL).all()) and bool((part[:, :M, N:] == S.SENTINEL).all())
    n_out = N // 2 if c["glu"] else N
    buf, y = guarded(M, n_out)
    ops.rows_finish(part, M, N, kg, bias=rm.bias, glu=c["glu"], wscale=rm.scale, y=y)
    torch.cuda.synchronize()
    assert guards_untouched(buf, M, n_out)
    if c["glu"]:
        assert glu_close(y.cpu(), ref)
    else:
        assert torch.equal(y.cpu(), ref.float()), int((y.cpu() != ref.float()).sum())


@pytest.mark.parametrize("kg", [1, 3, 5])
@pytest.mark.parametrize("No,what,f16", S.FINISH_RUNS)
def test_rows_finish_integer_exact(ops, No, what, f16, kg):
    """mi355_rows_finish on integer slabs: lean NP 1 / 2, generic, No % 8 != 0, the 16-column-block cap; 1, 3 and 5 slabs (the four-slab unrolled sum
    and its remainder); bias, power-of-two LayerScale, residual; planes out where No % 64 == 0, bf16 and fp16 for each of lean NP 1, lean NP 2 and
    the generic kernel, decode to y exactly; a bias pointer 4 bytes off alignment takes the generic kernel and must equal the aligned call bit for
    bit.  (tests/_linear_cases.py::finish_labels names the kernels of exactly these calls for the CPU file's coverage assertion.)"""
    M = 5
    g = torch.Generator().manual_seed(No + kg)
    ld = ops.round_up(No, 8) + 8
    slabs = torch.randint(-20, 21, (kg, M, No), generator=g)
    bias, res = torch.randint(-8, 9, (No,), generator=g), torch.randint(-30, 31, (M, No), generator=g)
    cs = torch.pow(2.0, torch.randint(-2, 3, (No,), generator=g).double())
    want = ((slabs.sum(0) + bias).double() * cs + res.double())
    assert float(want.abs().max()) * 4 < 2 ** 16 and torch.equal(want.float().double(), want)
    part = torch.full((kg, M + 1, ld), float("nan"), device=DEV)
    part[:, :M, :No] = slabs.float().to(DEV)
    part[:, :M, No:ops.round_up(No, 8)] = 99.0           # the pad of the last piece is read and must be dropped
    bias_buf = torch.zeros(No + 4, device=DEV)
    bias_buf[1:No + 1] = bias.float().to(DEV)
    bias_al = bias.float().to(DEV)
    resd = strided(res.float())
    got = []
    for b in (bias_al, bias_buf[1:No + 1]):
        buf, y = guarded(M, No)
        planes = nan_planes(ops, 16, No, f16) if No % 64 == 0 else None
        ops.rows_finish(part, M, No, kg, bias=b, colscale=cs.float().to(DEV), res=resd, y=y, planes=planes, R=16 if planes is not None else 0, f16=f16)
        torch.cuda.synchronize()
        assert guards_untouched(buf, M, No), what
        assert torch.equal(y.cpu(), want.float()), (what, int((y.cpu() != want.float()).sum()))
        if planes is not None:
            hi, lo = decode_planes(planes, 16, No, f16)
            assert torch.equal(hi[:M] + lo[:M], want) and bool(torch.isnan(hi[M:]).all())
        got.append(y.cpu())
    assert torch.equal(got[0], got[1])


@pytest.mark.parametrize("kvd", [torch.float32, torch.bfloat16, torch.float16])
def test_rows_finish_split_and_glu_destinations(ops, kvd):
    """A y2 split into each element type (integers: exact in all three), SwiGLU in the epilogue at 4 ulp, and fp16 planes out."""
    M, N, split, kg = 7, 208, 72, 2   # (glu rows come in whole 8-output pieces: N % 16 == 0)
    g = torch.Generator().manual_seed(11)
    slabs, bias = torch.randint(-8, 9, (kg, M, N), generator=g), torch.randint(-8, 9, (N,), generator=g)
    want = (slabs.sum(0) + bias).double()
    part = slabs.float().to(DEV).contiguous()
    buf, y = guarded(M, split)
    slot = torch.full((M, 3, N - split + 8), S.SENTINEL, dtype=kvd, device=DEV)
    ops.rows_finish(part, M, N, kg, bias=bias.float().to(DEV), y=y, y2=slot[:, 1, : N - split])
    torch.cuda.synchronize()
    assert guards_untouched(buf, M, split) and torch.equal(y.cpu(), want[:, :split].float())
    assert torch.equal(slot[:, 1, : N - split].double().cpu(), want[:, split:])
    assert bool((slot[:, 0] == S.SENTINEL).all()) and bool((slot[:, 2] == S.SENTINEL).all()) and bool((slot[:, 1, N - split:] == S.SENTINEL).all())
    buf, y = guarded(M, N // 2)
    ops.rows_finish(part, M, N, kg, bias=bias.float().to(DEV), glu=True, y=y)
    torch.cuda.synchronize()
    assert guards_untouched(buf, M, N // 2) and glu_close(y.cpu(), want)
    p16 = nan_planes(ops, 16, 192, True)
    ops.rows_finish(part[:, :, :192].contiguous(), M, 192, kg, planes=p16, R=16, f16=True)
    torch.cuda.synchronize()
    hi, lo = decode_planes(p16, 16, 192, True)
    assert torch.equal(hi[:M], slabs.sum(0)[:, :192].double()) and bool((lo[:M] == 0).all()) and bool(torch.isnan(hi[M:]).all())


# ----------------------------------------------------------------------------------------------------------------- 2. rounding
def run_family(ops, fam, wt, x, w, bias, norm=None, x_id_row=None):
    """y = norm(x) @ w^T + bias through the family's entry point: mi355_gemv, or converter -> rows_gemm -> rows_finish for 'rows'."""
    M, K = x.shape
    N = w.shape[0]
    rw = image(ops, w, wt, bias)
    dn = None if norm is None else (norm[0], None if norm[1] is None else norm[1].to(DEV), None if norm[2] is None else norm[2].to(DEV), norm[3])
    if fam != "rows":
        if x_id_row is not None:
            buf, y = guarded(1, N)
            ops.gemv(strided(x), rw, y, norm=dn, x_ids=torch.tensor([x_id_row - 1], dtype=torch.int32, device=DEV), x_id_offset=1)
            M = 1
        else:
            buf, y = guarded(M, N)
            ops.gemv(strided(x), rw, y, norm=dn)
        torch.cuda.synchronize()
        assert guards_untouched(buf, M, N)
        return y.cpu(), 1
    R, f16 = ops.rows_R(M), wt == "fp16"
    tl = ops.tiles16_from_rowmajor(rw)
    planes = to_planes(ops, x, R, f16, norm=dn)
    kg = S.case_kgroups(fam, N, K)
    assert kg == ops.rows_kgroups(N, K)
    part = torch.full((kg, M, ops.round_up(N, 8)), float("nan"), device=DEV)
    ops.rows_gemm(planes, tl, part, M, R, kgroups=kg)
    buf, y = guarded(M, N)
    ops.rows_finish(part, M, N, kg, bias=rw.bias, wscale=rw.scale, y=y)
    torch.cuda.synchronize()
    assert guards_untouched(buf, M, N)
    return y.cpu(), kg


# measured on an MI355X, largest error / bound per family: see docs/COVERAGE.md rows a21, a23-a24
@pytest.mark.parametrize("case", S.ROUND_CASES, ids=lambda c: "-".join(map(str, c)))
def test_split_rounding_per_element(ops, case):
    """Float inputs, float64 reference on the same inputs, ``|got - want| <= bound[m, n]`` per element (tests/_linear_cases.py::output_bound).  On
    these very inputs the mutant that drops the lo image misses by more than ten bounds (tests/test_linear_refs_cpu.py)."""
    fam, M, N, K, wt = case
    x, w, bias = S.round_inputs(fam, M, N, K, wt)
    want = x.double() @ w.double().T + bias.double()
    got, kg = run_family(ops, fam, wt, x, w, bias)
    bound = S.output_bound(fam, wt, x.double(), w.double(), want, kgroups=kg)
    ratio = float(((got.double() - want).abs() / bound).max())
    print(f"LINEAR split {'-'.join(map(str, case))} ratio={ratio:.3f}")
    assert bool(torch.isfinite(got).all()) and ratio <= 1.0, ratio


@pytest.mark.parametrize("case", S.NORM_CASES, ids=lambda c: "-".join(map(str, c)))
def test_fused_norm_per_element(ops, case):
    """LayerNorm / RMSNorm fused into every family (statistics from registers, the LDS copy, the k loop, fp64 sums, the converter), with a row of
    mean 1000 and unit spread, a constant row and a zero row; the M = 1 kernel takes each row in a call of its own, one of them through x_ids."""
    fam, M, N, K, wt, mode, has_w, has_b = case
    M_in = S.norm_rows(M)
    x, w, bias, nw, nb, eps = S.norm_inputs(fam, M_in, N, K, wt, mode, has_w, has_b)
    xh = S.norm_stmt(x, mode, nw, nb, eps)
    want = xh @ w.double().T + bias.double()
    norm = (mode, nw, nb, eps)
    if M == 1:
        rows = [run_family(ops, fam, wt, x[m:m + 1] if m != 1 else x, w, bias, norm=norm, x_id_row=1 if m == 1 else None) for m in range(M_in)]
        got, kg = torch.cat([r[0] for r in rows], 0), 1
    else:
        got, kg = run_family(ops, fam, wt, x, w, bias, norm=norm)
    bound = S.output_bound(fam, wt, xh, w.double(), want, xh_err=S.norm_error_bound(x, mode, nw, nb, eps, fam, wt), kgroups=kg)
    per_row = ((got.double() - want).abs() / bound).amax(1)
    print(f"LINEAR norm {'-'.join(map(str, case))} ratio={float(per_row.max()):.3f} mean1000 / constant / zero rows: "
          + " ".join(f"{float(r):.3f}" for r in per_row[:3]))
    assert bool(torch.isfinite(got).all()) and float(per_row.max()) <= 1.0, per_row


@pytest.mark.parametrize("case", S.WIDE_CASES, ids=lambda c: "-".join(map(str, c)))
def test_wide_range_integer_exact(ops, case):
    """One product of 2^14 beside seven products of 1 in every group of eight columns (tests/_linear_cases.py::WIDE_CASES): every sum is exact, so
    every family must be bit-equal to the float64 product.  A matrix instruction that aligns the eight products of one operand to their largest
    loses the small ones: the first form of gemv_mfma_fp8_kernel (v_mfma_f32_16x16x32_fp8_fp8) was short by exactly seven per group."""
    fam, M, N, K, wt = case
    x, w, bias = S.wide_inputs(fam, M, N, K, wt)
    want = x.double() @ w.double().T + bias.double()
    got, _ = run_family(ops, fam, wt, x, w, bias)
    assert torch.equal(got, want.float()), (case, float((got.double() - want).abs().max()))


# ----------------------------------------------------------------------------------------------------------------- 3. refusals
def _refused(fn, struct, kw, fragment):
    from mlx_audio_amd import _lib

    lib = _lib.load()
    st = _lib.STRUCTS[struct](**{k: v for k, v in kw.items() if v is not None})
    rc = getattr(lib, fn)(ctypes.byref(st), None)
    msg = lib.mi355_last_error().decode()
    assert rc == -1 and msg and fragment in msg, (fn, fragment, rc, msg)   # MI355_ERR_ARG


def test_gemv_refusals(ops):
    """Every MI355_REQUIRE of mi355_gemv a caller can trip, through the raw struct: MI355_ERR_ARG, a message, nothing launched (outputs keep the sentinel)."""
    K, N = 128, 32
    y, y2 = torch.full((64, N), S.SENTINEL, device=DEV), torch.full((64, N), S.SENTINEL, device=DEV)
    bufs = dict(x=torch.zeros(64, K, device=DEV), w16=torch.zeros(N, K, dtype=torch.int16, device=DEV), w8=torch.zeros(N, K, dtype=torch.uint8, device=DEV),
                ws=torch.ones(N, device=DEV), aux=torch.ones(256, device=DEV), ids=torch.zeros(1, dtype=torch.int32, device=DEV), y=y, y2=y2)
    for kw, fragment in S.gemv_refusals({k: t.data_ptr() for k, t in bufs.items()}):
        _refused("mi355_gemv", "mi355_gemv_args", kw, fragment)
    torch.cuda.synchronize()
    assert bool((y == S.SENTINEL).all()) and bool((y2 == S.SENTINEL).all())


def test_rows_refusals(ops):
    """The same for mi355_rows_gemm and mi355_rows_finish."""
    K, N, R, M = 320, 128, 16, 9
    part = torch.full((5, M, N), S.SENTINEL, device=DEV)
    po = torch.full((2 * R * N,), 0x1234, dtype=torch.int16, device=DEV)
    y, y2 = torch.full((M, 8200), S.SENTINEL, device=DEV), torch.full((M, N), S.SENTINEL, device=DEV)
    bufs = dict(wt=torch.zeros(N * K, dtype=torch.int16, device=DEV), planes=ops.rows_planes(R, K, DEV), part=part, po=po, aux=torch.ones(8200, device=DEV), y=y, y2=y2)
    P = {k: t.data_ptr() for k, t in bufs.items()}
    for kw, fragment in S.rows_gemm_refusals(P):
        _refused("mi355_rows_gemm", "mi355_rows_gemm_args", kw, fragment)
    for kw, fragment in S.rows_finish_refusals(P):
        _refused("mi355_rows_finish", "mi355_rows_finish_args", kw, fragment)
    torch.cuda.synchronize()
    assert bool((y == S.SENTINEL).all()) and bool((y2 == S.SENTINEL).all()) and bool((part == S.SENTINEL).all()) and bool((po == 0x1234).all())
