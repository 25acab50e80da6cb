"""The case tables, reference statements and bounds of tests/test_linear_kernel_edges_gpu.py held on the CPU: the preconditions that make every
integer case bit-exact (representability in the case's weight image and input image, the 2^24 budget of every partial sum), the dispatcher restated as
``route`` with the assertion that every kernel instantiation and both sides of every switch are reached by a case, the run lengths of the stream
kernel for every resident workgroup count, and the rounding bounds: a bit-level emulation of the input split stays within one bound while the
mutant that drops the lo image misses by more than ten, a float32 two-pass norm stays within its bound while the one-pass
variance misses by more than ten on the mean-1000 row.  Tables and statements live in tests/_linear_cases.py, which both files import."""
import ctypes
import os

import pytest
import torch

import _linear_cases as S
from oracle.lm_ref import dequantize_rows_fp8_ref, quantize_rows_fp8_ref

INT_CASES = S.int_cases()
ROWS_CASES = S.rows_cases()


def test_no_ab_knob_is_set():
    assert [k for k in S.ENV_KNOBS if k in os.environ] == []


def _exact_in(t, wt):
    """t (float64) survives the round trip through the image type."""
    if wt == "fp8":
        w = t.float()
        return torch.equal(dequantize_rows_fp8_ref(*quantize_rows_fp8_ref(w)), w)
    dt = torch.float16 if wt == "fp16" else torch.bfloat16
    return torch.equal(t.float().to(dt).double(), t)


def _check_int_preconditions(x, e, w, bias, wt):
    assert int(x.abs().max()) <= 4 and int(w.abs().max()) <= 7 and (w.shape[0] < 3 or bool((w == 0).all(1).any()))
    assert bias is None or int(bias.abs().max()) <= 8
    assert _exact_in(w.double(), wt)
    xs = x.double() * torch.pow(2.0, e.double())[:, None]
    assert torch.equal(xs.float().double(), xs)
    for img in ("bf16", "fp16"):                       # the hi image of either split
        assert _exact_in(xs, img)
    assert torch.equal(xs.float().to(torch.float8_e4m3fn).double(), xs)   # one e4m3 term holds them too
    assert S.int_budget(x, e, w, bias) < 2 ** 24
    ref = S.int_reference(x, e, w, bias)
    assert torch.equal(ref.float().double(), ref)


@pytest.mark.parametrize("c", INT_CASES, ids=S.case_id)
def test_integer_case_preconditions(c):
    x, e, w, bias = S.int_inputs(c)
    _check_int_preconditions(x, e, w, bias, c["wt"])
    if c["M"] > 1:
        assert bool((x == 0).all(1).any()) and len(set(e.tolist())) > 1


def test_fp8_image_is_exact_up_to_5_by_8192():
    g = torch.Generator().manual_seed(5)
    w = torch.randint(-7, 8, (5, 8192), generator=g).float()
    w[2] = 0
    assert torch.equal(dequantize_rows_fp8_ref(*quantize_rows_fp8_ref(w)), w)
    assert 28 * 8192 * 64 + 8 < 2 ** 24


@pytest.mark.parametrize("c", ROWS_CASES, ids=S.rows_case_id)
def test_rows_case_preconditions(c):
    x, e, w, bias = S.rows_inputs(c)
    _check_int_preconditions(x, e, w, bias, c["wt"])
    assert S.kgroups_valid(c["K"], S.rows_kg(c)), (c, S.rows_kg(c))
    assert not c["fused"] or (S.rows_kg(c) == 1 and c["N"] % 128 == 0)


def test_case_tables_cover_the_dispatcher():
    """Every instantiation and both sides of every switch (required_labels) is reached: integer cases (M = 1 under both weight policies), and the
    norm cases for the three statistics paths of gemv_kernel."""
    hit = set()
    for c in INT_CASES:
        for pol in ((0, 1) if c["M"] == 1 else (0,)):
            labels = S.route(c["M"], c["N"], c["K"], c["wt"], glu=c["glu"], x_ids=c["x_ids"], w_policy=pol)
            assert labels[0].startswith(c["fam"].replace("stream", "gemv1_stream").replace("splitk", "gemv1_splitk")), (c, labels)
            hit.update(labels)
    norm_hit = set()
    for fam, M, N, K, wt, mode, _, _ in S.NORM_CASES:
        if fam != "rows":
            labels = S.route(M, N, K, wt, norm=True)
            assert labels[0].startswith(fam.replace("stream", "gemv1_stream")), (fam, M, K, labels)
            norm_hit.update(labels)
    for fam, M, N, K, wt in S.ROUND_CASES + S.WIDE_CASES:
        if fam != "rows":
            assert S.route(M, N, K, wt)[0].startswith(fam.replace("stream", "gemv1_stream").replace("splitk", "gemv1_splitk")), (fam, M, K)
    missing = [r for r in S.required_labels() if r not in hit | norm_hit]
    assert missing == []
    assert {"gemv_kernel/norm/LDS copy", "gemv_kernel/norm/registers", "gemv_kernel/norm/k loop"} <= norm_hit
    # every family repeats one case bit for bit
    assert {c["fam"] for c in INT_CASES if c["repeat"]} == {"stream", "splitk", "gemv_kernel", "gemv_mfma", "gemv_mfma_fp8", "gemm_rows"}


def test_issue_cases_are_in_the_table():
    has = {(c["fam"], c["M"], c["N"], c["K"], c["wt"]) for c in INT_CASES}
    ks = lambda fam, **kw: {c["K"] for c in INT_CASES if c["fam"] == fam and all(c[k] == v for k, v in kw.items())}   # noqa: E731
    ns = lambda fam, **kw: {c["N"] for c in INT_CASES if c["fam"] == fam and all(c[k] == v for k, v in kw.items())}   # noqa: E731
    assert {8, 16, 504, 512, 520, 1016, 1024, 1032, 2040, 2048} <= ks("stream")
    assert {1, 2, 3, 5, 63, 64, 65, 257, 4095, 4096, 4097} <= ns("stream", glu=False) and {2, 6, 130} <= ns("stream", glu=True)
    assert {(8191, 64), (16385, 64), (66001, 64), (700001, 8)} <= {(c["N"], c["K"]) for c in INT_CASES if c["fam"] == "stream"}
    assert ("stream", 1, 300001, 16, "fp8") in has
    assert {2056, 2560, 4096, 4104, 8192} <= ks("splitk") and {1, 3, 4, 5, 1021} <= ns("splitk")
    assert any(c["x_ids"] for c in INT_CASES if c["fam"] == "splitk") and any(c["x_ids"] for c in INT_CASES if c["fam"] == "stream")
    assert ("gemv_kernel", 1, 6, 2112, "bf16") in has
    assert {4088, 4096, 4104, 8200} <= ks("gemv_kernel", M=2)
    for M in (3, 4):
        assert {2040, 2048, 2056, 4104} <= ks("gemv_kernel", M=M)
    for M in (5, 6, 7, 8):
        assert {8, 72, 1016, 1032, 2056, 2112, 4096} <= ks("gemv_kernel", M=M)
    assert ("gemv_kernel", 6, 9, 80, "fp8") in has
    assert {1, 3, 4, 5, 7, 8, 9} <= ns("gemv_kernel", K=72) and {16383, 16384, 16385} <= ns("gemv_kernel", M=2, K=8)
    assert {64, 128, 192, 1984, 2048} <= ks("gemv_mfma") and {1, 15, 16, 17, 33} <= ns("gemv_mfma")
    assert {c["M"] for c in INT_CASES if c["fam"] == "gemv_mfma"} == {5, 6, 7, 8}
    assert {64, 2048, 2112, 4096, 4160} <= ks("gemv_mfma_fp8") and {1, 17, 8176, 8177, 8193, 16368, 16369, 16400} <= ns("gemv_mfma_fp8", K=64)
    assert {9, 15, 16, 17, 31, 32, 33, 63, 64} <= {c["M"] for c in INT_CASES if c["fam"] == "gemm_rows"}
    assert {64, 960, 1024, 1088} <= ks("gemm_rows", M=9) and {512, 576} <= ks("gemm_rows", M=17) and {256, 320} <= ks("gemm_rows", M=63)
    assert {1, 511, 512, 513, 1025} <= {(n + 15) // 16 for n in ns("gemm_rows", K=64)}


def test_stream_ladder_reaches_every_run_length():
    """gpw depends on the compiled register count, so it is not routed: for every resident workgroup count the chip can report, the stream cases
    give runs of 1 and 2, an odd run of at least 3 (re-reads its last group), an even run of at least 4, a ragged last wave and dead waves."""
    stream = [c for c in INT_CASES if c["fam"] == "stream"]
    for resident in range(256, 2049):
        runs, ragged, dead, capped = set(), False, False, False
        for c in stream:
            r = S.stream_runs(c["N"], c["K"], c["wt"], resident, glu=c["glu"])
            runs |= r["runs"]
            ragged |= r["ragged"]
            dead |= r["dead_waves"]
            capped |= r["capped"]
            assert r["gpw"] <= 64
        assert {1, 2} <= runs and any(g >= 3 and g % 2 for g in runs) and any(g >= 4 and g % 2 == 0 for g in runs) and ragged and dead, (resident, sorted(runs))
        assert capped, resident


def test_rows_tables_cover_their_dispatch():
    hit = {S.route_rows_gemm(c["R"], c["N"], c["wt"]) for c in ROWS_CASES}
    hit |= S.finish_labels()   # the kernels of exactly the calls test_rows_finish_integer_exact makes
    missing = [r for r in S.required_rows_labels() if r not in hit]
    assert missing == []
    assert {(c["R"], c["M"]) for c in ROWS_CASES} >= {(R, M) for R in (16, 32, 64) for M in (1, R - 1, R)}
    assert {(c["N"] + 15) // 16 for c in ROWS_CASES} >= {31, 32, 33, 2047, 2048}
    assert {c["kg"] for c in ROWS_CASES} >= {1, 2, "auto", "cap"}
    assert S.route_rows_finish(2048, aligned=False) == "rows_finish<bf16>" and S.route_rows_finish(4104) == "rows_finish<bf16>"
    assert S.route_rows_finish(13) == "rows_finish<bf16>" and S.route_rows_finish(2056) == "rows_finish_lean<bf16,NP=2>"


# ----------------------------------------------------------------------------------------------------------------- rounding
@pytest.mark.parametrize("case", S.ROUND_CASES, ids=lambda c: "-".join(map(str, c)))
def test_split_emulation_within_one_bound_and_mutant_beyond_ten(case):
    fam, M, N, K, wt = case
    kg = S.case_kgroups(fam, N, K)
    x, w, bias = S.round_inputs(fam, M, N, K, wt)
    assert torch.equal(S.round_weights(w, wt), w)
    want = x.double() @ w.double().T + bias.double()
    bound = S.output_bound(fam, wt, x.double(), w.double(), want, kgroups=kg)
    efam, ewt = (fam, wt) if fam != "rows" else ("rows", "fp16" if wt == "fp16" else "bf16")
    got = S.split_emulate(x, efam, ewt) @ w.double().T + bias.double()
    ratio = float(((got - want).abs() / bound).max())
    assert ratio <= 1.0, ratio
    if S.split_gamma(fam, wt)[0] > 0:
        mut = S.split_emulate(x, efam, ewt, drop_last=True) @ w.double().T + bias.double()
        miss = float(((mut - want).abs() / bound).max())
        assert miss > 10.0, miss
        # the measured residual of the full split on these inputs
        res = float(((S.split_emulate(x, efam, ewt) - x.double()).abs() / x.double().abs()).max())
        assert res <= S.split_gamma(fam, wt)[0] + (2.0 ** -25 / float(x.abs().min()) if wt == "fp16" else 0.0), res


@pytest.mark.parametrize("case", S.NORM_CASES, ids=lambda c: "-".join(map(str, c)))
def test_norm_float32_within_bound_and_one_pass_mutant_beyond_ten(case):
    fam, M, N, K, wt, mode, has_w, has_b = case
    x, w, bias, nw, nb, eps = S.norm_inputs(fam, S.norm_rows(M), N, K, wt, mode, has_w, has_b)   # the GPU test's own inputs
    xh = S.norm_stmt(x, mode, nw, nb, eps)
    xerr = S.norm_error_bound(x, mode, nw, nb, eps, fam, wt)
    x32 = S.norm_stmt(x, mode, nw, nb, eps, dtype=torch.float32, stats64=fam == "gemm_rows").double()   # (gemm_rows sums in float64)
    assert float(((x32 - xh).abs() / xerr.clamp_min(1e-300)).max()) <= 1.0
    want = xh @ w.double().T + bias.double()
    bound = S.output_bound(fam, wt, xh, w.double(), want, xh_err=xerr, kgroups=S.case_kgroups(fam, N, K))
    got = x32 @ w.double().T + bias.double()
    assert float(((got - want).abs() / bound).max()) <= 1.0
    if mode == "layer":   # the one-pass variance in float32, on the mean-1000 row
        m32 = S.norm_stmt(x[:1], mode, nw, nb, eps, dtype=torch.float32, one_pass=True).double()
        mut = m32 @ w.double().T + bias.double()
        miss = float(((mut - want[:1]).abs() / bound[:1]).max())
        assert miss > 10.0, miss


# ----------------------------------------------------------------------------------------------------------------- refusals
def test_refusal_tables_are_refused_before_any_device_work():
    """The argument checks read no memory and come before any launch: on made-up (aligned) addresses every entry of the refusal tables returns
    MI355_ERR_ARG with the expected message, without a GPU."""
    from mlx_audio_amd import _lib

    lib = _lib.load()
    names = ("x", "w16", "w8", "ws", "aux", "ids", "y", "y2", "wt", "planes", "part", "po")
    P = {n: 0x10000000 + 0x100000 * i for i, n in enumerate(names)}
    n = 0
    for fn, struct, table in (("mi355_gemv", "mi355_gemv_args", S.gemv_refusals(P)), ("mi355_rows_gemm", "mi355_rows_gemm_args", S.rows_gemm_refusals(P)),
                              ("mi355_rows_finish", "mi355_rows_finish_args", S.rows_finish_refusals(P))):
        for kw, fragment in table:
            st = _lib.STRUCTS[struct](**{k: v for k, v in kw.items() if v is not None})
            rc = getattr(lib, fn)(ctypes.byref(st), None)
            msg = lib.mi355_last_error().decode()
            assert rc == -1 and fragment in msg, (fn, kw, fragment, rc, msg)
            n += 1
    assert n == 96


@pytest.mark.parametrize("case", S.WIDE_CASES, ids=lambda c: "-".join(map(str, c)))
def test_wide_range_case_preconditions(case):
    """Exact in every image, every partial sum an integer below 2^24, and every group of eight columns holds one product of 2^14 beside seven of 1."""
    fam, M, N, K, wt = case
    x, w, bias = S.wide_inputs(fam, M, N, K, wt)
    assert _exact_in(w.double(), wt) and _exact_in(x.double(), "bf16") and _exact_in(x.double(), "fp16")
    assert float((x.abs().double() @ w.abs().double().T).max()) + 8 < 2 ** 24
    prod = (x[:1, None, :] * w[None, :, :]).abs().reshape(1, N, K // 8, 8)
    assert bool(((prod == 2.0 ** 14).sum(-1) == 1).all()) and bool(((prod == 1.0).sum(-1) == 7).all())
