"""The reference statements of tests/test_seq_kernel_edges_gpu.py held to known-good implementations, every precondition of its cases, and the mutants:
deliberately wrong variants of each statement, evaluated on the suite's own inputs, must miss the case's bar by a factor of ten -- so a kernel that is
wrong in the same way cannot pass the GPU file.  All on the CPU: a knife-edge input or a toothless case fails here, before any GPU run.  Statements
and case tables live in tests/_seq_kernel_cases.py, which both files import."""
import pytest
import torch

import _ops_emu
import _seq_kernel_cases as S

F64 = torch.float64


def _close(a, b, tol=1e-12):
    return float((a.double() - b.double()).abs().max()) <= tol * max(1.0, float(b.abs().max()))


def _rows(lens, L, B):
    return [L if lens is None else lens[b] for b in range(B)]


def _worst_gap(a, b, lens):
    """max |a - b| over the rows < lens[b] (the rows the GPU file compares)."""
    B, L = a.shape[:2]
    return max((float((a[i, :n] - b[i, :n]).abs().max()) for i, n in enumerate(_rows(lens, L, B)) if n), default=0.0)


# ----------------------------------------------------------------------------------------------------------------- lstm_bidir
@pytest.mark.parametrize("quant", [False, True], ids=["plain", "quant_h"])
@pytest.mark.parametrize("H,In,L,seed", S.QUANT_TIGHT)
def test_lstm_bidir_statement_is_the_oracle(H, In, L, seed, quant):
    """lstm_bidir_stmt in float64 against oracle.kokoro_ref.bilstm, item by item of a ragged batch [L, 1, 0, L - 1], with and without ``quant_modules``
    (the oracle then quantises each item's x and every step's h; the statement gets the same x-projection, in float64)."""
    from oracle import kokoro_ref as K

    w, x, _, wf, wb = S.quant_case(H, In, L, seed)
    lens = [L, 1, 0, L - 1]
    wx = torch.cat([w["l.Wx_forward"], w["l.Wx_backward"]], 0).double()
    bias = torch.cat([w["l.bias_ih_forward"].double() + w["l.bias_hh_forward"].double(), w["l.bias_ih_backward"].double() + w["l.bias_hh_backward"].double()])
    xp = torch.zeros(4, L, 8 * H, dtype=F64)
    for b, n in enumerate(lens):
        if n:
            xi = S.fq_u8(x[0, :n])[0] if quant else x[0, :n]
            xp[b, :n] = xi.double() @ wx.t() + bias
    got = S.lstm_bidir_stmt(xp, wf, wb, lens, F64, quant_h=quant)
    p = K.P(w, "l.", dtype=F64, quant_modules=("l",) if quant else ())
    for b, n in enumerate(lens):
        if n:
            assert _close(got[b, :n], K.bilstm(p, x[:, :n].double())[0]), (b, n)
        if n < L:
            assert float(got[b, n:].abs().max()) == 0.0


@pytest.mark.parametrize("H,In,L,seed", S.QUANT_TIGHT)
def test_lstm_quant_h_margins(H, In, L, seed):
    """The tight ``quant_h`` cases stay clear of every rounding boundary: the float32 oracle's smallest distance (the KittenTTS test's rule) and the
    float64 statement's own, on the x-projection the kernel gets, both above 2e-4 grid steps."""
    from oracle import kokoro_ref as K

    w, x, xp, wf, wb = S.quant_case(H, In, L, seed)
    K.FQ_MARGINS = []
    try:
        K.bilstm(K.P(w, "l.", quant_modules=("l",)), x)
        oracle_margin = min(K.FQ_MARGINS)
    finally:
        K.FQ_MARGINS = None
    mine = []
    S.lstm_bidir_stmt(xp, wf, wb, None, F64, quant_h=True, margins=mine)
    print(f"QUANT-PRE H={H} oracle margin {oracle_margin:.2e} statement margin {min(mine):.2e}")
    assert oracle_margin > S.QUANT_MARGIN and min(mine) > S.QUANT_MARGIN


@pytest.mark.parametrize("H", S.LSTM_H)
def test_lstm_bidir_mutants_miss_the_bar(H):
    """On the ragged batch: f / o exchanged, the backward pass started at L - 1, the state carried into the next item -- each at least 10x the bar away."""
    wf, wb = S.lstm_weights(H, 0, "bf16")
    name, B, L, lens = S.lstm_shapes()[4]
    assert name == "ragged" and lens == [L, 1, 0, L - 1, 2]
    xp = S.lstm_xp(H, B, L, 0)
    r64, r32 = S.lstm_bidir_stmt(xp, wf, wb, lens, F64), S.lstm_bidir_stmt(xp, wf, wb, lens, torch.float32)
    _, _, bar = S.bar_of(r64, r32)
    assert bar <= 5e-5
    for variant in ("fo_swap", "start_L", "carry"):
        gap = _worst_gap(S.lstm_bidir_stmt(xp, wf, wb, lens, F64, variant=variant), r64, lens)
        print(f"MUTANT lstm_bidir H={H} {variant} gap={gap:.3e} bar={bar:.3e}")
        assert gap >= 10 * bar, (variant, gap, bar)


@pytest.mark.parametrize("H,In,L,seed", S.QUANT_TIGHT)
def test_lstm_quant_emit_mutant_misses_the_bar(H, In, L, seed):
    """``quant_h`` quantising the emitted h as well, and ``quant_h`` ignored: both at least 10x the 2e-5 bar away."""
    _, _, xp, wf, wb = S.quant_case(H, In, L, seed)
    r64 = S.lstm_bidir_stmt(xp, wf, wb, None, F64, quant_h=True)
    gap = float((S.lstm_bidir_stmt(xp, wf, wb, None, F64, quant_h=True, variant="quant_emit") - r64).abs().max())
    print(f"MUTANT lstm_bidir quant_h H={H} quant_emit gap={gap:.3e} bar={S.QUANT_BAR:.1e}")
    assert gap >= 10 * S.QUANT_BAR
    assert float((S.lstm_bidir_stmt(xp, wf, wb, None, F64) - r64).abs().max()) >= 10 * S.QUANT_BAR


# ----------------------------------------------------------------------------------------------------------------- lstm_seq
def test_seq_gate_function_is_the_oracles():
    from oracle.encodec_ref import lstm_sigmoid

    x = torch.cat([torch.linspace(-30, 30, 601, dtype=F64), torch.tensor([0.0, -0.0, 1e-300, -1e-300, 700.0, -700.0], dtype=F64)])
    assert torch.equal(S.seq_sigmoid(x), lstm_sigmoid(x))
    assert _close(S.seq_sigmoid(x), torch.sigmoid(x))


@pytest.mark.parametrize("H,B,T,carried", [(8, 1, 1, False), (24, 4, 5, True), (64, 9, 2, True), (72, 3, 3, False)])
def test_lstm_seq_statement_is_nn_lstm(H, B, T, carried):
    """lstm_seq_stmt in float64 against torch.nn.LSTM (input = the x-projection through an identity W_ih, no biases): out, h_T and c_T."""
    c = dict(H=H, B=B, T=T, image="f16", h0=carried)
    wh, xproj, h0, c0 = S.seq_inputs(c)
    m = torch.nn.LSTM(4 * H, H, batch_first=True, bias=False, dtype=F64)
    with torch.no_grad():
        m.weight_ih_l0.copy_(torch.eye(4 * H, dtype=F64))
        m.weight_hh_l0.copy_(wh.double())
        st = None if not carried else (h0.double()[None], c0.double()[None])
        want, (hT, cT) = m(xproj.double(), st)
    out, h, cc = S.lstm_seq_stmt(xproj, wh, h0, c0, F64)
    assert _close(out, want) and _close(h, hT[0]) and _close(cc, cT[0])


SEQ_CASES = S.seq_cases()


def test_seq_case_table_covers_the_issue():
    ids = [S.seq_id(c) for c in SEQ_CASES]
    assert len(set(ids)) == len(ids)
    have = {(c["H"], c["B"], c["image"], c["fused"]) for c in SEQ_CASES}
    for H in (8, 24, 72, 200):
        for B in (1, 4, 8):
            assert (H, B, "bf16", False) in have and (H, B, "f16", False) in have
    for B in (8, 9, 16, 17, 32, 33, 64):
        for image in ("bf16", "f16"):
            assert (64, B, image, True) in have and (64, B, image, False) in have
    assert (320, 33, "f16", True) in have and (2112, 2, "f16", True) in have and (2112, 33, "f16", True) in have
    assert {c["T"] for c in SEQ_CASES} >= {1, 2, 5}
    for fused in (True, False):
        assert any(c["h0"] and c["fused"] == fused for c in SEQ_CASES) and any(c["view"] and c["fused"] == fused for c in SEQ_CASES)
    assert all(not c["fused"] or c["H"] % 64 == 0 for c in SEQ_CASES) and all(c["B"] <= 8 or c["H"] % 64 == 0 for c in SEQ_CASES)
    # the launch arithmetic the cases rely on (csrc/gemm_rows.hip): KC = 1024 / MR columns per chunk; 512 workgroups; H / 4 tiles
    assert 320 % (1024 // 4) == 64 and 512 < 2112 // 4 < 1024
    assert [S.seq_route(B, 64, False) for B in (4, 5, 8, 9)] == ["fma", "mfma", "mfma", "mfma"] and S.seq_route(8, 72, False) == "fma"


@pytest.mark.parametrize("c", [c for c in SEQ_CASES if c["H"] <= 320], ids=S.seq_id)
def test_lstm_seq_mutants_miss_the_bar(c):
    """Gate blocks read at stride H + 1 (every case) and c0 ignored (the cases with a carried state): at least 10x the bar of the case -- the split
    term of the matrix-pipe routes included -- away from the float64 statement in ``out``."""
    wh, xproj, h0, c0 = S.seq_inputs(c)
    width, floor = S.seq_split_term(c["image"] == "f16")
    r64 = S.lstm_seq_stmt(xproj, wh, h0, c0, F64, split_width=width, split_floor=floor)
    r32 = S.lstm_seq_stmt(xproj, wh, h0, c0, torch.float32)
    mfma = S.seq_route(c["B"], c["H"], c["fused"]) == "mfma"
    _, _, bar = S.bar_of(r64[0], r32[0])
    bar += float(r64[3][0].max()) if mfma else 0.0
    for variant in ("stride",) + (("no_c0",) if c["h0"] else ()):
        gap = float((S.lstm_seq_stmt(xproj, wh, h0, c0, F64, variant=variant)[0] - r64[0]).abs().max())
        print(f"MUTANT lstm_seq {S.seq_id(c)} {variant} gap={gap:.3e} bar={bar:.3e}")
        assert gap >= 10 * bar, (variant, gap, bar)


# ----------------------------------------------------------------------------------------------------------------- aa_activation
AA_CASES = S.aa_cases()


def test_aa_case_table_covers_every_dispatch_class():
    for C, want in S.AA_CLASSES.items():
        assert S.aa_tile(C) == want
    assert {S.aa_tile(C)[0] for C in S.AA_CLASSES} == {8, 16, 32, 64}
    assert 136 % 64 != 0 and 136 > 128 and 4 < 8 and 12 % 8 != 0
    for C, (_, T) in S.AA_CLASSES.items():
        Ls = {c["L"] for c in AA_CASES if c["C"] == C and c["lens"] is None}
        assert {T - 1, T, T + 1} <= Ls
        ragged = [c for c in AA_CASES if c["C"] == C and c["lens"]]
        assert len(ragged) == 1 and {T, T + 1, 1} <= set(ragged[0]["lens"]) and ragged[0]["L"] > T   # a second tile exists for the item of length T


@pytest.mark.parametrize("c", AA_CASES, ids=S.aa_id)
def test_aa_statement_is_the_oracle_and_mutants_miss_the_bar(c):
    """aa_activation_stmt in float64 against oracle/bigvgan_ref.py (F.conv_transpose1d / F.conv1d on replicate-padded rows), item by item; the sine's
    argument stays below 16 rad; zero padding and the wrong tap parity each miss the bar (with its sine term) by 10x."""
    from oracle import bigvgan_ref as R

    x, alpha, ib = S.aa_inputs(c)
    filt = S.aa_filter()
    got = S.aa_activation_stmt(x, filt, filt, alpha, ib, c["lens"], F64)
    r32 = S.aa_activation_stmt(x, filt, filt, alpha, ib, c["lens"], torch.float32)
    for b, n in enumerate(_rows(c["lens"], c["L"], c["B"])):
        u = R.upsample2(x[b:b + 1, :n].double(), filt.double())
        assert float((alpha.double() * u.abs()).max()) <= 16.0
        want = R.downsample2(u + ib.double() * torch.sin(u * alpha.double()) ** 2, filt.double())[0]
        assert _close(got[b, :n], want), (b, n)
        if n < c["L"]:
            assert float(got[b, n:].abs().max()) == 0.0
    e32, peak, bar = S.bar_of(got, r32)
    bar += float(S.aa_sine_term(filt, ib).max())
    assert bar <= 2e-5 * max(1.0, peak)
    for variant in ("zero_pad", "phase"):
        gap = _worst_gap(S.aa_activation_stmt(x, filt, filt, alpha, ib, c["lens"], F64, variant=variant), got, c["lens"])
        print(f"MUTANT aa_activation {S.aa_id(c)} {variant} gap={gap:.3e} bar={bar:.3e}")
        assert gap >= 10 * bar, (variant, gap, bar)


# ----------------------------------------------------------------------------------------------------------------- rvq_encode
RVQ_CASES = S.rvq_cases()


@pytest.mark.parametrize("bins", [2, 65, 300])
def test_rvq_statement_is_the_emulation(bins):
    """rvq_stmt in float64 against tests/_ops_emu.py::rvq_encode.  The emulation works in float32, so the inputs sit on a dyadic grid (multiples of 1/8
    up to 3, D = 8) on which every float32 product, sum and residual is exact: gaps to 1e-12, codes equal up to a frame's first exact tie."""
    g = torch.Generator().manual_seed(bins)
    tables = torch.randint(-24, 25, (3, bins, 8), generator=g).float() / 8
    x = torch.randint(-24, 25, (50, 8), generator=g).float() / 8
    c2 = (tables * tables).sum(-1) * 0.5
    codes, gaps, _ = S.rvq_stmt(x, tables, c2, F64)
    ecodes, emg = _ops_emu.rvq_encode(x, tables, tables.transpose(1, 2).contiguous(), c2, margins=True)
    decided = torch.cumprod((gaps > 0).to(torch.int64), 1).bool()
    first_tie = decided | torch.cat([torch.ones(50, 1, dtype=torch.bool), decided[:, :-1]], 1)   # the gap of a frame's first tie is still comparable
    assert _close(gaps[first_tie], emg[first_tie])
    assert float(decided.float().mean()) > 0.5
    assert torch.equal(codes[decided], ecodes.long()[decided])


def test_rvq_tie_layout_meets_in_the_intended_merges():
    """Thread = bin % 256, wave = thread / 64 (csrc/rvq.hip: a thread owns bins tid, tid + 256, ...): the copies of each duplicated codeword meet in the
    per-thread scan, in one wave's shuffle tree, in the four-wave merge -- and the triple in all three."""
    thread = lambda b: b % 256          # noqa: E731
    wave = lambda b: thread(b) // 64    # noqa: E731
    kinds = {}
    for copies, kind in S.RVQ_TIES:
        assert list(copies) == sorted(copies) and copies[-1] < 600
        kinds[kind] = copies
    a, b = kinds["thread"]
    assert thread(a) == thread(b)
    a, b = kinds["wave"]
    assert thread(a) != thread(b) and wave(a) == wave(b)
    a, b = kinds["block"]
    assert wave(a) != wave(b)
    a, b, c = kinds["triple"]
    assert thread(a) == thread(b) and wave(c) != wave(a)
    used = [b for copies, _ in S.RVQ_TIES for b in copies]
    assert len(set(used)) == len(used)


@pytest.mark.parametrize("c", RVQ_CASES, ids=lambda c: c["name"])
def test_rvq_case_preconditions(c):
    """Every rvq case on the float64 statement alone: at most 2 % of the decisions lie behind a gap below 1e-4 max|score|; the tie rows ARE ties of
    gap exactly 0 in float64 and in float32, the lower copy wins, and the last-minimum mutant picks another code."""
    x, tables, c2 = S.rvq_inputs(c)
    codes, gaps, peaks = S.rvq_stmt(x, tables, c2, F64)
    if c["kind"] == "ties":
        n = len(S.RVQ_TIES)
        g32 = S.rvq_stmt(x, tables, c2, torch.float32)[1]
        last = S.rvq_stmt(x, tables, c2, F64, variant="last")[0]
        for rows in (slice(0, n), slice(x.shape[0] - n, x.shape[0])):
            assert codes[rows, 0].tolist() == [copies[0] for copies, _ in S.RVQ_TIES]
            assert float(gaps[rows, 0].abs().max()) == 0.0 and float(g32[rows, 0].abs().max()) == 0.0
            assert last[rows, 0].tolist() == [copies[-1] for copies, _ in S.RVQ_TIES]
        gaps = gaps.clone()
        gaps[:n, 0] = gaps[-n:, 0] = float("inf")   # the ties are compared exactly, not by the margin rule
    share = 1.0 - float(S.rvq_compared(gaps, peaks).float().mean())
    print(f"RVQ-PRE {c['name']} uncompared share {share:.4f}")
    assert share <= S.RVQ_CAP, (c["name"], share)
