"""TEST INFRASTRUCTURE shared by tests/test_linear_kernel_edges_gpu.py and tests/test_linear_refs_cpu.py: the case tables of the decode-side linear
kernels (csrc/gemv.hip, gemv_mfma.hip, gemv_mfma_fp8.hip, gemm_rows.hip, rows_pipe.hip), the dispatcher restated as a pure function, the reference
statements and the per-element bounds of the rounding cases.  CPU only: nothing here touches ``mlx_audio_amd.ops``, a device or the environment.

Integer cases.  x holds integers in [-4, 4] (times one power of two per row, 2^-6 .. 2^6, for M > 1), w integers in [-7, 7] with one all-zero row,
bias integers in [-8, 8] (the zero row from N = 3 on).  Such weights are exact in the bf16, fp16 and e4m3 + power-of-two-row-scale images, the inputs are exact in the hi image
of either split, and 28 K 2^6 + 8 < 2^24 up to K = 8192: every partial sum, in any order, on the FMA units or on the
matrix pipe, is an exactly representable number, so every kernel family must be BIT-EQUAL to the int64 product (tests/test_linear_refs_cpu.py
asserts these preconditions case by case).

Rounding cases.  Float inputs against float64 on the same inputs, per element:

    bound[m, n] = (g_split + g_acc) * sum_k |xh[m, k]| |w[n, k]| + (absolute split term) + (fused-norm term) + ulp32(|want[m, n]|)

with xh the (normalised) input row, g_acc = (L + 8) 2^-24 and L the family's longest dependent chain of float32 additions (``chain_length``), and
g_split the residual of the input split (``split_gamma``).  The eight extra roundings are the bias add, the joins of the four waves' partial sums
through LDS and the scale multiplies.
"""
import math

import torch

WTS = ("bf16", "fp16", "fp8")
SENTINEL = -777.25          # exactly representable; no case produces it
ROW_EXP = (-6, 6, 0, -3, 3, 1, -1, 5)   # per-row powers of two of the M > 1 cases, cycled
ENV_KNOBS = ("MI355_GEMV_NT", "MI355_GEMV_MFMA", "MI355_GEMV_MFMA_FP8", "MI355_GEMM_ROWS_WGS", "MI355_GEMM_ROWS_DBG", "MI355_ROWS_T", "MI355_ROWS_KG",
             "MI355_ROWS_WGS", "MI355_ROWS_FINISH_OLD")   # read once per process by the library: the suite asserts at import that none is set


# ----------------------------------------------------------------------------------------------------------------- the dispatcher, restated
def _gemv_kc(mt):
    """x elements staged per row and chunk by gemv_kernel (gemv.hip:126)."""
    return 1024 if mt >= 8 else (2048 if mt == 4 else 4096)


def route(M, N, K, wt, *, glu=False, norm=False, rope=False, x_ids=False, w_policy=0):
    """mi355_gemv's dispatch (gemv.hip:678-790, gemv_mfma.hip:206-218, gemv_mfma_fp8.hip:204-234, gemm_rows.hip:265-302) for aligned operands:
    the labels a call carries = the kernel instantiation it launches, then the side of each switch inside that family it sits on."""
    assert wt in WTS and 1 <= M <= 64
    sixteen = wt != "fp8"
    if M > 8:                                                         # gemm_rows.hip:288-302
        assert sixteen and K % 64 == 0 and not rope and not x_ids
        mr = 1 if M <= 16 else (2 if M <= 32 else 4)
        kc, nt = 1024 // mr, (N + 15) // 16
        return (f"gemm_rows<MR={mr},{wt}>", f"gemm_rows/MR={mr}/" + ("one chunk" if K <= kc else ("chunk ring refilled" if K > 2 * kc else "two chunks")),
                "gemm_rows/" + ("tiles<512" if nt < 512 else ("tiles=512" if nt == 512 else ("tiles>T*512" if nt > (1 if mr == 1 else 2) * 512 else "tiles>512"))))
    if 5 <= M <= 8 and not rope and sixteen and K % 64 == 0 and 64 <= K <= 2048:        # gemv_mfma.hip:206-218
        return (f"gemv_mfma<{wt}>", "gemv_mfma/" + ("idle waves" if K < 256 else "every wave has a step"))
    if wt == "fp8" and 5 <= M <= 8 and not rope and not x_ids and K % 64 == 0 and K >= 64 and not (K > 2048 and norm):   # gemv_mfma_fp8.hip:204-234
        nt = (N + 15) // 16
        tpw = 4 if nt >= 1024 else (2 if nt >= 512 else 1)
        return (f"gemv_mfma_fp8<TPW={tpw}>", "gemv_mfma_fp8/" + ("one chunk" if K <= 2048 else "chunks"),
                "gemv_mfma_fp8/" + ("last workgroup short" if nt % tpw else "whole workgroups"))
    if M == 1 and (K <= 2048 or (not norm and not glu and not rope)):                  # gemv.hip:734, 678-714
        nt_ = int(w_policy == 1)
        if K <= 2048:
            nc = 2 if (glu or rope or N >= 4096) else 1
            return (f"gemv1_stream<NC={nc},{wt},NT={nt_},HALF={int(K <= 1024)}>",)
        return (f"gemv1_splitk<{wt},NT={nt_}>",)
    assert not x_ids
    mt = 1 if M == 1 else (2 if M == 2 else (4 if M <= 4 else 8))                       # gemv.hip:735-738
    nc = 2 if (glu or rope or mt >= 8 or N >= 16384) else 1                             # gemv.hip:723
    kc = _gemv_kc(mt)
    out = [f"gemv_kernel<MT={mt},NC={nc},{wt}>", f"gemv_kernel/MT={mt}/" + ("one chunk" if K <= kc else "chunks")]
    if norm:                                                                            # gemv.hip:163-200
        out.append("gemv_kernel/norm/" + ("LDS copy" if K <= kc else ("registers" if K <= 2048 else "k loop")))
    return tuple(out)


def stream_runs(N, K, wt, resident, glu=False):
    """(gpw, runs) of gemv1_stream_kernel for a chip that holds ``resident`` workgroups (gemv.hip:690-701, 322-324): the run length of every full
    wave and the set of run lengths G that occur (the last wave's run may be shorter)."""
    ngroups = (N + 1) // 2 if (glu or N >= 4096) else N
    want = -(-ngroups // (resident * 4))
    gpw = min(want, 64)
    waves = -(-ngroups // gpw)
    tail = ngroups - (waves - 1) * gpw
    blocks = -(-ngroups // (4 * gpw))
    return dict(gpw=gpw, runs={gpw, tail} if waves > 1 else {tail}, capped=want > 64, ragged=tail < gpw, dead_waves=blocks * 4 > waves)


def tiles_per_wg(N):
    nt = (N + 15) // 16
    return 4 if nt >= 2048 else (2 if nt >= 32 else 1)              # rows_pipe.hip:188-196


def rows_kgroups_stmt(N, K):
    """mi355_rows_kgroups (rows_pipe.hip:522-535) without its A/B knobs."""
    steps, T = K // 64, tiles_per_wg(N)
    ng = ((N + 15) // 16 + T - 1) // T
    kg = max(1, min((512 + ng // 2) // ng, max(steps // 4, 1)))
    spg = (steps + kg - 1) // kg
    return (steps + spg - 1) // spg


def kgroups_valid(K, kg):
    steps = K // 64
    spg = (steps + kg - 1) // kg
    return 1 <= kg <= steps and (steps + spg - 1) // spg == kg       # rows_pipe.hip:547-551


def route_rows_gemm(R, N, wt):
    return f"rows_gemm<MR={R // 16},T={tiles_per_wg(N)},{wt}>"


def route_rows_finish(No, *, glu=False, y2=False, f16=False, aligned=True, planes=False):
    """rows_pipe.hip:579-600: the straight-line kernel for whole 8-column pieces, <= 4096 outputs and aligned operands, else the generic one."""
    f = "fp16" if (planes and f16) else "bf16"
    if not glu and not y2 and No % 8 == 0 and No <= 4096 and aligned:
        return f"rows_finish_lean<{f},NP={2 if No > 2048 else 1}>"
    return f"rows_finish<{f}>"


# ----------------------------------------------------------------------------------------------------------------- integer cases
def _c(fam, M, N, K, wt, branch, **kw):
    d = dict(fam=fam, M=M, N=N, K=K, wt=wt, branch=branch, glu=False, bias=True, x_ids=False, repeat=False)
    d.update(kw)
    assert wt != "fp8" or K % 16 == 0, d
    return d


def _wts(K):
    return WTS if K % 16 == 0 else WTS[:2]


def int_cases():
    """Every integer-exact case of mi355_gemv, each with the branch it crosses."""
    out = []
    # ---- gemv1_stream_kernel: M = 1, K <= 2048
    for i, K in enumerate((8, 16, 504, 512, 520, 1016, 1024, 1032, 2040, 2048)):
        for j, wt in enumerate(_wts(K)):
            out.append(_c("stream", 1, (65, 5, 257)[j], K, wt, f"K = {K}: lanes clamped / slice edges / HALF switch at 1024", bias=(i + j) % 2 == 0))
    for N in (1, 2, 3, 5, 63, 64, 65, 257):
        out.append(_c("stream", 1, N, 520, "bf16", f"N = {N}: one column per wave, dead waves of the last workgroup"))
        out.append(_c("stream", 1, N, 1024, "fp16", f"N = {N}: one column per wave"))
        out.append(_c("stream", 1, N, 16, "fp8", f"N = {N}: one column per wave, one live lane"))
    for N in (4095, 4096, 4097):
        out.append(_c("stream", 1, N, 1032, "bf16", f"N = {N}: one -> two columns per wave, odd N"))
        out.append(_c("stream", 1, N, 2048, "fp16", f"N = {N}: one -> two columns per wave, odd N", bias=False))
        out.append(_c("stream", 1, N, 64, "fp8", f"N = {N}: one -> two columns per wave, odd N"))
    for N in (2, 6, 130):
        out.append(_c("stream", 1, N, 520, "bf16", f"glu, N = {N}", glu=True))
        out.append(_c("stream", 1, N, 2048, "fp16", f"glu, N = {N}", glu=True, bias=False))
        out.append(_c("stream", 1, N, 1024, "fp8", f"glu, N = {N}", glu=True))
    out.append(_c("stream", 1, 4097, 1040, "fp8", "two columns per wave, fp8, K > 1024"))
    for N, K, wt in LADDER:
        out.append(_c("stream", 1, N, K, wt, "run-length ladder", bias=N % 2 == 1))
    out.append(_c("stream", 1, 65, 1024, "fp16", "x_ids", x_ids=True, repeat=True))
    out.append(_c("stream", 1, 9, 2040, "bf16", "x_ids", x_ids=True))
    out.append(_c("stream", 1, 4097, 512, "fp8", "x_ids, two columns", x_ids=True))
    # ---- gemv1_splitk_kernel: M = 1, K > 2048, plain input side
    for K in (2056, 2560, 4096, 4104, 8192):
        for j, wt in enumerate(_wts(K)):
            out.append(_c("splitk", 1, 5, K, wt, f"K = {K}: slices per wave, a wave with no slices at K = 2056 / 2560", bias=j != 1))
    for N in (1, 3, 4, 5, 1021):
        out.append(_c("splitk", 1, N, 2560, "bf16", f"N = {N}: columns of the last workgroup", repeat=N == 1021))
        out.append(_c("splitk", 1, N, 4104, "fp16", f"N = {N}"))
        out.append(_c("splitk", 1, N, 4096, "fp8", f"N = {N}"))
    out.append(_c("splitk", 1, 7, 4096, "bf16", "x_ids", x_ids=True))
    out.append(_c("splitk", 1, 7, 4096, "fp8", "x_ids", x_ids=True))
    out.append(_c("gemv_kernel", 1, 6, 2112, "bf16", "M = 1, K > 2048 with glu: gemv_kernel<1, 2>", glu=True))
    out.append(_c("gemv_kernel", 1, 6, 2112, "fp8", "M = 1, K > 2048 with glu: gemv_kernel<1, 2>", glu=True))
    # ---- gemv_kernel
    for K in (4088, 4096, 4104, 8200):
        for wt in _wts(K):
            out.append(_c("gemv_kernel", 2, 5, K, wt, f"M = 2, K = {K}: chunk edge KC = 4096", repeat=(K, wt) == (4104, "bf16")))
    for M in (3, 4):
        for K in (2040, 2048, 2056, 4104):
            for wt in _wts(K):
                out.append(_c("gemv_kernel", M, 7 if M == 3 else 9, K, wt, f"M = {M} on the 4-row kernel, K = {K}: chunk edge KC = 2048", bias=K != 2056))
    for i, M in enumerate((5, 6, 7, 8)):
        for K in (8, 72, 1016, 1032, 2056):
            out.append(_c("gemv_kernel", M, 9, K, ("bf16", "fp16")[(i + K // 8) % 2], f"M = {M} off the matrix pipe (K % 64 != 0), K = {K}: chunk edge KC = 1024"))
        for K in (2112, 4096):
            out.append(_c("gemv_kernel", M, 3, K, "bf16", f"M = {M}, K = {K} > 2048: 16-bit weights stay on the FMA kernel"))
    out.append(_c("gemv_kernel", 6, 9, 80, "fp8", "fp8 off the matrix pipe"))
    out.append(_c("gemv_kernel", 3, 6, 2048, "fp16", "glu on the 4-row kernel: two columns per wave", glu=True))
    out.append(_c("gemv_kernel", 7, 10, 1032, "bf16", "glu on the 8-row kernel", glu=True))
    for N in (1, 3, 4, 5, 7, 8, 9):
        out.append(_c("gemv_kernel", 2, N, 72, "bf16", f"N = {N}: columns of the last workgroup, one column per wave"))
        out.append(_c("gemv_kernel", 8, N, 72, "fp16", f"N = {N}: columns of the last workgroup, two columns per wave"))
        out.append(_c("gemv_kernel", 4, N, 80, "fp8", f"N = {N}: columns of the last workgroup"))
    for N in (16383, 16384, 16385):
        out.append(_c("gemv_kernel", 2, N, 8, "bf16", f"N = {N}: one -> two columns per wave at 2..4 rows"))
        out.append(_c("gemv_kernel", 3, N, 16, "fp8", f"N = {N}: one -> two columns per wave at 2..4 rows"))
    # ---- gemv_mfma_kernel
    for i, K in enumerate((64, 128, 192, 1984, 2048)):
        for j, N in enumerate((1, 15, 16, 17, 33)):
            out.append(_c("gemv_mfma", 5 + (i + j) % 4, N, K, ("bf16", "fp16")[(i + j) % 2], f"K = {K} (k steps per wave), N = {N} (ragged 16-column tile)",
                          bias=(i * 5 + j) % 3 != 0, repeat=(K, N) == (1984, 33)))
    out.append(_c("gemv_mfma", 6, 34, 192, "bf16", "glu", glu=True))
    out.append(_c("gemv_mfma", 5, 18, 64, "fp16", "glu", glu=True))
    # ---- gemv_mfma_fp8_kernel
    for i, K in enumerate((64, 2048, 2112, 4096, 4160)):
        out.append(_c("gemv_mfma_fp8", 5 + i % 4, 33, K, "fp8", f"K = {K}: chunks of 2048", repeat=K == 2112))
    for i, N in enumerate((1, 17, 8176, 8177, 8193, 16368, 16369, 16400)):
        out.append(_c("gemv_mfma_fp8", 5 + i % 4, N, 64, "fp8", f"N = {N}: {(N + 15) // 16} tiles, tpw 1 / 2 / 4", bias=i % 2 == 0))
    out.append(_c("gemv_mfma_fp8", 8, 8210, 128, "fp8", "glu, two tiles per workgroup", glu=True))
    # ---- gemm_rows_kernel
    for i, M in enumerate((9, 15, 16, 17, 31, 32, 33, 63, 64)):
        ks = (64, 960, 1024, 1088, 2112) if M <= 16 else ((512, 576, 1088) if M <= 32 else (256, 320, 576))
        for j, K in enumerate(ks):
            out.append(_c("gemm_rows", M, (33, 48, 17)[(i + j) % 3], K, ("bf16", "fp16")[(i + j) % 2], f"M = {M}, K = {K}: chunk edge of MR", bias=j != 1,
                          repeat=(M, K) == (33, 320)))
    for i, N in enumerate((9, 8170, 8192, 8200, 16395)):
        for M in (12, 20, 40):
            out.append(_c("gemm_rows", M, N, 64, ("bf16", "fp16")[(i + M // 4) % 2], f"N = {N}: {(N + 15) // 16} tiles against the 512-workgroup cap"))
    out.append(_c("gemm_rows", 24, 8210, 128, "bf16", "glu, tile groups", glu=True))
    return out


# the run-length ladder of the stream kernel: (N, K, wt).  Whatever resident_workgroups returns between 256 and 2048 these give runs of 1 and 2,
# an odd run of at least 3, an even run of at least 4, a ragged last wave and the cap of 64 groups (asserted for every count on the CPU)
# (8193, 45001 and 1050001 are there for the counts the issue's five leave without a run of 2, an even run, or -- above 1367 -- the cap)
LADDER = [(8191, 64, "bf16"), (16385, 64, "fp16"), (66001, 64, "bf16"), (700001, 8, "bf16"), (300001, 16, "fp8"), (8193, 64, "fp16"), (45001, 64, "bf16"),
          (1050001, 8, "bf16")]


def case_id(c):
    f = "".join(k[0] for k in ("glu", "x_ids") if c.get(k)) + ("" if c.get("bias", True) else "nb")
    return f"{c['fam']}-M{c['M']}-N{c['N']}-K{c['K']}-{c['wt']}" + (f"-{f}" if f else "")


def _gen(c):
    return torch.Generator().manual_seed(1000003 * c["M"] + 7919 * c["N"] + 31 * c["K"] + WTS.index(c["wt"]) + 17 * int(c["glu"]))


def int_inputs(c):
    """(x int64 [M, K], row exponents [M], w int64 [N, K], bias int64 [N] or None).  One all-zero weight row; M > 1: one all-zero input row and a
    power of two per row.  The input row of the kernel is x * 2^e."""
    g = _gen(c)
    M, N, K = c["M"], c["N"], c["K"]
    x = torch.randint(-4, 5, (M, K), generator=g)
    w = torch.randint(-7, 8, (N, K), generator=g)
    if N >= 3:
        w[N // 2] = 0                             # (N < 3: a zero row would be the whole case)
    w[0, 0], w[N - 1, K - 1] = 7, -7              # the extremes are present: the first and the last element of the image
    x[0, 0], x[0, K - 1] = 4, -4
    bias = torch.randint(-8, 9, (N,), generator=g) if c["bias"] else None
    e = torch.zeros(M, dtype=torch.int64)
    if M > 1:
        e = torch.tensor([ROW_EXP[m % len(ROW_EXP)] for m in range(M)])
        x[M // 2] = 0
    return x, e, w, bias


def int_reference(x, e, w, bias):
    """(x.long() @ w.long().T) * 2^e + bias in float64 (exact: every value is below 2^53), as the float32 the kernels must equal bit for bit."""
    s = (x.long() @ w.long().T).double() * torch.pow(2.0, e.double())[:, None]
    if bias is not None:
        s = s + bias.double()
    return s


def glu_value32(pre):
    """silu(g) * u of the (gate, up) column pairs in float32, the kernel's expression (linear_common.h:92): (g / (1 + exp(-g))) * u."""
    p = pre.float()
    g, u = p[:, 0::2], p[:, 1::2]
    return (g / (1.0 + torch.exp(-g))) * u


def ulp32(v):
    """Spacing of float32 at |v| (float64 tensor), at least the smallest normal's."""
    v = v.double().abs().clamp_min(2.0 ** -126)
    return torch.pow(2.0, torch.floor(torch.log2(v)) - 23)


def int_budget(x, e, w, bias):
    """Largest |partial sum| of a case in units of its row's granule (2^min(e, 0)): must stay below 2^24."""
    s = (x.abs().long() @ w.abs().long().T).double() * torch.pow(2.0, e.double())[:, None]
    if bias is not None:
        s = s + bias.abs().double()
    return float((s / torch.pow(2.0, e.clamp(max=0).double())[:, None]).max())


# ----------------------------------------------------------------------------------------------------------------- integer cases, wide range
# One product of 2^14 (x = 2^7, w = 2^7) beside seven products of +-1 in every group of eight columns: exact in every image and every sum, far
# below 2^24 -- and what a matrix instruction that aligns the products of one 8-byte operand to their largest loses (v_mfma_f32_16x16x32_fp8_fp8
# drops what lies 2^14 or more below it: the first form of gemv_mfma_fp8_kernel was short by exactly the seven small products of each group).
WIDE_CASES = [("stream", 1, 20, 64, "bf16"), ("stream", 1, 20, 64, "fp8"), ("splitk", 1, 9, 2112, "fp16"), ("splitk", 1, 9, 2112, "fp8"),
              ("gemv_kernel", 3, 20, 64, "fp8"), ("gemv_kernel", 7, 20, 72, "bf16"), ("gemv_mfma", 6, 20, 64, "bf16"), ("gemv_mfma", 8, 20, 256, "fp16"),
              ("gemv_mfma_fp8", 6, 20, 64, "fp8"), ("gemv_mfma_fp8", 8, 20, 256, "fp8"), ("gemv_mfma_fp8", 5, 20, 2112, "fp8"),
              ("gemm_rows", 12, 20, 64, "bf16"), ("gemm_rows", 40, 20, 320, "fp16"), ("rows", 12, 32, 64, "fp8"), ("rows", 33, 32, 256, "bf16")]


def wide_inputs(fam, M, N, K, wt):
    """x, w float32 of +-1 with 2^7 at one column of every group of eight (the same column in x and w), integer bias."""
    g = torch.Generator().manual_seed(K + 3 * M + WTS.index(wt))
    x = (torch.randint(0, 2, (M, K), generator=g) * 2 - 1).float()
    w = (torch.randint(0, 2, (N, K), generator=g) * 2 - 1).float()
    big = torch.arange(0, K, 8) + torch.randint(0, 8, (K // 8,), generator=g)
    x[:, big] = 128.0
    w[:, big] = 128.0 * (torch.randint(0, 2, (N, K // 8), generator=g) * 2 - 1).float()
    return x, w, torch.randint(-8, 9, (N,), generator=g).float()


# ----------------------------------------------------------------------------------------------------------------- rows pipeline (integer)
def rows_cases():
    """rows_finish (converter) -> rows_gemm -> rows_finish.  kg: 1, 2, 'auto' (mi355_rows_kgroups) or 'cap' (K / 256)."""
    out = []
    i = 0
    for R in (16, 32, 64):
        for M in (1, R - 1, R):
            for N, K, kg in ((496, 256, 1), (512, 512, 2), (528, 1024, "auto"), (40, 1024, "cap"), (519, 64, 1)):
                out.append(dict(R=R, M=M, N=N, K=K, kg=kg, wt=WTS[i % 3], bias=i % 2 == 0, glu=False, fused=False))
                i += 1
    for N in (32752, 32768):                    # 2047 / 2048 tiles: T 2 -> 4, every row count and weight type
        for R, M in ((16, 9), (64, 64), (32, 17)):
            for wt in WTS:
                out.append(dict(R=R, M=M, N=N, K=64, kg=1, wt=wt, bias=wt != "fp16", glu=False, fused=False))
    out.append(dict(R=32, M=20, N=512, K=256, kg=1, wt="bf16", bias=True, glu=True, fused=False))
    out.append(dict(R=16, M=9, N=256, K=128, kg=2, wt="fp8", bias=True, glu=True, fused=False))
    out.append(dict(R=32, M=31, N=256, K=128, kg=1, wt="bf16", bias=True, glu=True, fused=True))
    out.append(dict(R=64, M=33, N=384, K=64, kg=1, wt="fp8", bias=False, glu=True, fused=True))
    return out


def rows_case_id(c):
    return f"R{c['R']}-M{c['M']}-N{c['N']}-K{c['K']}-kg{c['kg']}-{c['wt']}" + ("-glu" if c["glu"] else "") + ("-fused" if c["fused"] else "")


def rows_kg(c):
    return {"auto": rows_kgroups_stmt(c["N"], c["K"]), "cap": max(c["K"] // 256, 1)}.get(c["kg"], c["kg"])


def rows_inputs(c):
    d = dict(c, fam="rows", x_ids=False)
    x, _, w, bias = int_inputs(d)
    M = c["M"]
    e = torch.tensor([ROW_EXP[m % len(ROW_EXP)] for m in range(M)])
    if M > 1:
        x[M // 2] = 0
    return x, e, w, bias


# rows_finish on its own: (No, what, f16 planes).  lean NP 1 / 2, generic, ragged pieces, the 16-column-block cap of the generic grid; planes go out
# where No % 64 == 0, in both element types for the lean NP = 1 / NP = 2 and the generic kernel.  Every entry runs twice: aligned operands, and a bias
# pointer 4 bytes off (the generic kernel): ``finish_labels`` names the kernels of exactly these calls.
FINISH_RUNS = [(8, "lean NP = 1, one piece", False), (2048, "lean NP = 1, every thread one piece", False), (2048, "lean NP = 1, fp16 planes", True),
               (2056, "lean NP = 2", False), (4096, "lean NP = 2, full", False), (4096, "lean NP = 2, fp16 planes", True), (4104, "generic: above 4096", False),
               (4160, "generic, planes out", False), (4160, "generic, fp16 planes out", True), (33000, "generic: 16 column blocks, strided pieces", False),
               (33024, "generic: 16 column blocks, fp16 planes out", True), (2052, "generic: No % 8 != 0", False), (13, "generic: No % 8 != 0", False)]


def finish_labels():
    out = set()
    for No, _, f16 in FINISH_RUNS:
        for aligned in (True, False):
            out.add(route_rows_finish(No, f16=f16, aligned=aligned, planes=No % 64 == 0))
    return out


# ----------------------------------------------------------------------------------------------------------------- rounding cases
def chain_length(fam, K, wt, M=1, kgroups=1):
    """L: the longest dependent chain of float32 additions behind one output."""
    epl = 16 if wt == "fp8" else 8                       # weight elements per 16-byte lane piece (gemv.hip:123)
    sl = 64 * epl
    if fam == "stream":       # gemv.hip:423-433: a lane's NIT slices of EPL fmaf each, then the 6 steps of wave_sum_fast
        return -(-K // sl) * epl + 6
    if fam == "splitk":       # gemv.hip:603-605, 650-658: ceil(slices / 4) slices per wave, the wave sum, three LDS joins
        return -(-(-(-K // sl)) // 4) * epl + 6 + 3
    if fam == "gemv_kernel":  # gemv.hip:146, 260-271, 112-116: every slice of the row in one lane, then the wave sum
        return -(-K // sl) * epl + 6
    # matrix pipe (gemv_mfma.hip:179-193, gemv_mfma_fp8.hip:159-173, gemm_rows.hip:199-236, rows_pipe.hip:87-154 + slab sums 239-250): L = K
    return K + kgroups


def split_gamma(fam, wt):
    """(relative, absolute) residual of the input split per element of the normalised input row, split_hi_lo rounding both images to nearest
    (linear_common.h:27-39): bf16 leaves 2^-8 * 2^-8 of |x|; fp16 2^-11 * 2^-11 of |x| plus half the subnormal spacing 2^-25 where the lo image
    underflows.  The FMA kernels multiply the float32 input itself."""
    if fam in ("stream", "splitk", "gemv_kernel"):
        return 0.0, 0.0
    if wt == "fp16":
        return 2.0 ** -22, 2.0 ** -25
    return 2.0 ** -16, 0.0      # bf16 planes: gemv_mfma_fp8 and the fp8 tile images of the rows pipeline decode the weight bytes to bf16


def split_emulate(xh, fam, wt, drop_last=False):
    """Bit-level emulation of the kernel's input split with torch's casts: the float64 value of the images a matrix-pipe kernel multiplies.
    ``drop_last``: the mutant that loses the lo image.  xh float32 [M, K]."""
    xh = xh.float()
    if fam in ("stream", "splitk", "gemv_kernel"):
        return xh.double()
    dt = torch.float16 if wt == "fp16" else torch.bfloat16
    hi = xh.to(dt).float()
    lo = (xh - hi).to(dt).float()
    return hi.double() if drop_last else hi.double() + lo.double()


def round_weights(w, wt):
    """float32 weights exactly representable in the case's image: bf16 / fp16 rounding, or the dequantised e4m3 + power-of-two-row-scale image."""
    if wt == "fp8":
        from oracle.lm_ref import dequantize_rows_fp8_ref, quantize_rows_fp8_ref

        return dequantize_rows_fp8_ref(*quantize_rows_fp8_ref(w))
    return w.to(torch.float16 if wt == "fp16" else torch.bfloat16).float()


def stat_chain(fam, K, wt):
    """Depth of the chain of float32 additions behind a row sum of the fused norm (its mean, and likewise its centred second moment), the final
    division included:
      stream         a lane adds its own elements one by one, ceil(K / (64 EPL)) slices of EPL (gemv.hip:374-379), then six wave steps
      gemv_kernel    norm_row_stats (linear_common.h:57-69; the register path of gemv.hip:184-187 has the same shape): a lane adds one float4 piece
                     per 256 columns, two levels inside a piece, six wave steps
      gemv_mfma(_fp8) eight values of a thread in three levels, six wave steps, four waves in two levels (gemv_mfma.hip:86-99)
      gemm_rows      float64 sums (gemm_rows.hip:64-83): what is left is the rounding of the mean to float32
      rows           the converter rows_finish: eight outputs of a piece one by one, up to four pieces per thread, six wave steps, four waves in
                     two levels (rows_pipe.hip:264-275, 322-331)."""
    epl = 16 if wt == "fp8" else 8
    if fam == "stream":
        return -(-K // (64 * epl)) * epl + 6 + 1
    if fam in ("gemv_kernel", "splitk"):
        return -(-K // 256) + 2 + 6 + 1
    if fam in ("gemv_mfma", "gemv_mfma_fp8"):
        return 3 + 6 + 2 + 1
    if fam == "gemm_rows":
        return 1
    return 8 + -(-K // 2048) + 6 + 2 + 1


def lane_sum32(t):
    """Row sums of t [M, K] (K % 4 == 0) in float32 in the order of norm_row_stats (linear_common.h:57-69): lane l adds its float4 pieces at
    k = 4 l, 4 l + 256, ... as (x + y) + (z + w), then the 64 lanes meet in a tree."""
    t = t.float()
    M, K = t.shape
    pad = (-K) % 256
    t = torch.cat([t, torch.zeros(M, pad)], 1).reshape(M, -1, 64, 4)
    acc = torch.zeros(M, 64)
    for i in range(t.shape[1]):
        acc = acc + ((t[:, i, :, 0] + t[:, i, :, 1]) + (t[:, i, :, 2] + t[:, i, :, 3]))
    n = 64
    while n > 1:
        n //= 2
        acc = acc[:, :n] + acc[:, n:2 * n]
    return acc


def norm_stmt(x, mode, nw, nb, eps, dtype=torch.float64, one_pass=False, stats64=False):
    """The fused input norm, two-pass: mean, then the centred second moment (RMSNorm: mean = 0); xh = (x - mean) * rstd * weight + bias.
    ``one_pass``: the mutant with var = E[x^2] - mean^2, its two sums in float32 in a kernel's order (``lane_sum32``).  ``stats64``: mean and
    variance from float64 sums, rounded to ``dtype`` (gemm_rows)."""
    x64 = x.double()
    x = x.to(dtype)
    mean = x.mean(-1, keepdim=True) if mode == "layer" else torch.zeros_like(x[:, :1])
    if stats64:
        mean = (x64.mean(-1, keepdim=True) if mode == "layer" else torch.zeros_like(x64[:, :1]))
        var = ((x64 - mean) ** 2).mean(-1, keepdim=True).to(dtype)
        mean = mean.to(dtype)
    elif one_pass:
        assert dtype == torch.float32
        K = x.shape[-1]
        mean = lane_sum32(x) / K if mode == "layer" else mean
        var = (lane_sum32(x * x) / K - mean * mean).clamp_min(0)
    else:
        var = ((x - mean) ** 2).mean(-1, keepdim=True)
    y = (x - mean) * torch.rsqrt(var + eps)
    if nw is not None:
        y = y * nw.to(dtype)
    if nb is not None:
        y = y + nb.to(dtype)
    return y


def norm_error_bound(x, mode, nw, nb, eps, fam, wt):
    """Per-element bound [M, K] of a float32 two-pass evaluation of ``norm_stmt`` against float64, u = 2^-24, c = stat_chain(fam, K, wt):
      mean:   |dmean| <= c u sum|x| / K                                   (a sum of K terms by a chain of c additions, the division among them)
      d = x - mean:  |dd| <= |dmean| + u |d|
      var = sum d^2 / K:  the computed d are the true ones shifted by dmean, and the true d sum to zero, so the shift enters in second order:
              |dvar| <= dmean^2 + (c + 4) u (var + dmean^2)                (the shift; the squares, the chain, the division)
      rstd = (var + eps)^-1/2:  relative 0.5 |dvar| / (var + eps) + 3 u   (the add, and the square root + division or the 1-ulp rsqrt)
      xh = d rstd w + b:  |w| rstd |dd| + |d rstd w| (rel(rstd) + 2 u) + u |xh|."""
    u = 2.0 ** -24
    x = x.double()
    K = x.shape[-1]
    c = stat_chain(fam, K, wt)
    mean = x.mean(-1, keepdim=True) if mode == "layer" else torch.zeros_like(x[:, :1])
    dmean = c * u * x.abs().sum(-1, keepdim=True) / K if mode == "layer" else torch.zeros_like(mean)
    d = x - mean
    var = (d * d).mean(-1, keepdim=True)
    dvar = dmean ** 2 + (c + 4) * u * (var + dmean ** 2)
    rstd = torch.rsqrt(var + eps)
    rel = 0.5 * dvar / (var + eps) + 3 * u
    w = torch.ones(K, dtype=torch.float64) if nw is None else nw.double().abs()
    core = d.abs() * rstd * w
    xh = norm_stmt(x, mode, nw, nb, eps).abs()
    return w * rstd * (dmean + u * d.abs()) + core * (rel + 2 * u) + u * xh


def output_bound(fam, wt, xh, w, want, *, xh_err=None, kgroups=1, chain_K=None):
    """bound[m, n] of the module docstring.  xh float64 [M, K] (the normalised input), w float64 [N, K], want float64 [M, N] (pre-bias products +
    bias); ``xh_err`` the fused norm's per-element bound."""
    K = xh.shape[1]
    g_rel, g_abs = split_gamma(fam, wt)
    g_acc = (chain_length(fam, chain_K or K, wt, kgroups=kgroups) + 8) * 2.0 ** -24
    aw = w.abs()
    b = (g_rel + g_acc) * (xh.abs() @ aw.T) + ulp32(want)
    if g_abs:
        b = b + g_abs * aw.sum(1)[None, :]
    if xh_err is not None:
        b = b + (1 + g_rel + g_acc) * (xh_err @ aw.T)
    return b


# (family, M, N, K, wt): float inputs, K <= 256 where the family allows it (split K exists above K = 2048 only)
ROUND_CASES = [
    ("stream", 1, 37, 256, "bf16"), ("stream", 1, 37, 200, "fp16"), ("stream", 1, 37, 256, "fp8"),
    ("splitk", 1, 9, 2056, "bf16"), ("splitk", 1, 9, 2056, "fp16"), ("splitk", 1, 9, 2064, "fp8"),
    ("gemv_kernel", 3, 21, 256, "bf16"), ("gemv_kernel", 7, 21, 200, "fp16"), ("gemv_kernel", 4, 21, 256, "fp8"),
    ("gemv_mfma", 5, 37, 256, "bf16"), ("gemv_mfma", 8, 37, 256, "fp16"), ("gemv_mfma", 6, 20, 64, "bf16"),
    ("gemv_mfma_fp8", 7, 37, 256, "fp8"), ("gemv_mfma_fp8", 5, 20, 64, "fp8"),
    ("gemm_rows", 12, 37, 256, "bf16"), ("gemm_rows", 33, 37, 256, "fp16"), ("gemm_rows", 20, 37, 192, "bf16"),
    ("rows", 12, 40, 256, "bf16"), ("rows", 33, 40, 256, "fp16"), ("rows", 20, 40, 256, "fp8"),
]


def case_kgroups(fam, N, K):
    """K groups whose slabs the row epilogue adds: mi355_rows_kgroups for the rows pipeline (what the GPU test passes), 1 elsewhere."""
    return rows_kgroups_stmt(N, K) if fam == "rows" else 1


SPLIT_FAMILIES = ("gemv_mfma", "gemv_mfma_fp8", "gemm_rows", "rows")


def round_inputs(fam, M, N, K, wt):
    """x [M, K] float32.  Even rows: the suite's x = 1.5 randn + 0.2.  Odd rows of the families that split their input: x = c (1 + delta) with c a
    power of two times 1 .. 1.75 and delta just under half an ulp of the hi type; w >= 0 in these families, so the residual of a dropped image is
    coherent along the row.  w float32 [N, K] exactly representable in the image; bias float32 [N]."""
    g = torch.Generator().manual_seed(97 * M + 13 * N + K + WTS.index(wt))
    x = torch.randn(M, K, generator=g) * 1.5 + 0.2
    w = torch.randn(N, K, generator=g) / math.sqrt(K)
    if fam in SPLIT_FAMILIES:
        w = w.abs()
        rows = len(range(1, M, 2))
        half_ulp = 2.0 ** -12 if wt == "fp16" else 2.0 ** -9      # of the planes' type (bf16 planes under fp8 weight images)
        c = (1.0 + 0.25 * torch.randint(0, 4, (rows, K), generator=g)) * torch.pow(2.0, torch.randint(-2, 2, (rows, K), generator=g).float())
        x[1::2] = (c.double() * (1.0 + 0.97 * half_ulp)).float()
    return x, round_weights(w, wt), torch.randn(N, generator=g) * 0.1


# (family, M, N, K, wt, mode, weight, bias): the fused norm's statistics come from different code in every family and on each side of these K
NORM_CASES = [
    ("stream", 1, 19, 256, "bf16", "layer", True, True), ("stream", 1, 19, 1032, "fp16", "rms", True, False), ("stream", 1, 19, 2048, "fp8", "layer", False, False),
    ("gemv_kernel", 2, 19, 256, "bf16", "layer", True, True),      # the LDS copy (K <= KC = 4096)
    ("gemv_kernel", 4, 19, 2056, "fp16", "rms", False, False),     # MT = 4, K > KC = 2048: the k loop
    ("gemv_kernel", 8, 19, 1032, "bf16", "layer", True, False),    # MT = 8, KC = 1024 < K <= 2048: registers
    ("gemv_kernel", 6, 19, 1016, "fp16", "rms", True, False),      # MT = 8, K <= KC: the LDS copy
    ("gemv_kernel", 3, 19, 4104, "bf16", "layer", False, False),   # the k loop
    ("gemv_mfma", 5, 19, 256, "bf16", "layer", True, True), ("gemv_mfma", 8, 19, 2048, "fp16", "rms", True, False),
    ("gemv_mfma_fp8", 6, 19, 256, "fp8", "layer", True, True), ("gemv_mfma_fp8", 7, 19, 2048, "fp8", "rms", False, False),
    ("gemm_rows", 12, 19, 256, "bf16", "layer", True, True), ("gemm_rows", 40, 19, 320, "fp16", "rms", True, False),
    ("stream", 1, 19, 1024, "bf16", "rms", False, False), ("stream", 1, 19, 528, "fp8", "layer", True, False),
    ("gemv_mfma", 7, 19, 192, "fp16", "layer", False, False), ("gemv_mfma", 6, 19, 64, "bf16", "rms", False, False),
    ("gemv_mfma_fp8", 5, 19, 64, "fp8", "rms", True, False), ("gemv_mfma_fp8", 8, 19, 1984, "fp8", "layer", False, False),
    ("gemm_rows", 20, 19, 576, "bf16", "rms", False, False), ("gemm_rows", 64, 19, 192, "fp16", "layer", False, False), ("gemm_rows", 9, 19, 1088, "bf16", "layer", True, True),
    ("rows", 12, 24, 256, "bf16", "layer", True, True), ("rows", 33, 24, 2112, "fp16", "rms", True, False), ("rows", 20, 24, 4160, "bf16", "layer", False, False),
]


def norm_rows(M):
    """Rows of a norm case's input: an M = 1 case carries four (the three special rows and a plain one), each run in a call of its own."""
    return 4 if M == 1 else M


def norm_inputs(fam, M, N, K, wt, mode, has_w, has_b):
    """Rows: 0 = mean 1000 and unit spread, 1 = constant (M > 1), 2 = zero (M > 2: the eps alone), the rest x = 1.5 randn + 0.2.  The GPU test
    runs an M = 1 case once per special row (``row=``)."""
    g = torch.Generator().manual_seed(131 * M + 7 * N + K + WTS.index(wt))
    x = torch.randn(M, K, generator=g) * 1.5 + 0.2
    # the mean-1000 row.  In float32 E[x^2] and mean^2 are near 10^6, where the spacing is 1 / 16, so a one-pass variance of a unit-spread row is
    # off by a few sixteenths -- or, by luck, by nothing.  The row is drawn again until the float32 one-pass variance (sums in a kernel's order) is
    # at least 5 % off: the row on which that mutant shows
    for _ in range(64):
        x[0] = 1000.0 + torch.randn(K, generator=g)
        v1 = float(lane_sum32(x[:1] * x[:1]) / K - (lane_sum32(x[:1]) / K) ** 2)
        if abs(v1 / float(x[0].double().var(unbiased=False)) - 1.0) >= 0.05:
            break
    else:
        raise AssertionError("no mean-1000 row with a visible one-pass error")
    if M > 1:
        x[1] = 3.25
    if M > 2:
        x[2] = 0.0
    w = torch.randn(N, K, generator=g) / math.sqrt(K)
    nw = torch.randn(K, generator=g) if has_w else None
    nb = torch.randn(K, generator=g) * 0.1 if has_b else None
    # output column 0 is matched to row 0: it weighs the elements more than one spread from the row's mean, each with the sign of its normalised
    # value, so every product of that sum is positive and a relative error of row 0's 1 / std shows in full there
    d0 = x[0] - x[0].mean() if mode == "layer" else x[0]
    w[0] = w[0].abs() * torch.sign(d0 * (nw if has_w else 1.0)) * (d0.abs() > d0.std()).float()
    w = round_weights(w, wt)
    return x, w, torch.randn(N, generator=g) * 0.1, nw, nb, (1e-5 if mode == "layer" else 1e-6)


# ----------------------------------------------------------------------------------------------------------------- refusals
# (struct fields, fragment of the message) of every argument check a caller can trip; P maps a name to the address of a buffer (the checks read
# no memory: the CPU file runs them on made-up addresses, the GPU file on real sentinel-filled buffers).  Shapes: gemv K = 128, N = 32;
# rows K = 320 (5 k steps), N = 128, R = 16, M = 9.
def gemv_refusals(P):
    K, N = 128, 32
    base = dict(x=P["x"], ldx=K, M=1, K=K, w=P["w16"], ldw=K, wdtype=0, N=N, y=P["y"], ldy=N)
    fp8 = dict(base, w=P["w8"], wdtype=2, wscale=P["ws"])
    rope = dict(rope_cos=P["aux"], rope_sin=P["aux"], rope_dh=16, rope_cols=32)
    attn = dict(attn_k=P["aux"], attn_v=P["aux"], attn_Tk=4, attn_heads=2, attn_kv_heads=2, attn_dh=64, attn_ld=128, attn_scale=1.0)
    return [
        (dict(base, x=None), "null tensor"), (dict(base, y=None), "null tensor"),
        (dict(base, M=65), "M must be in [1, 64]"), (dict(base, M=0), "M must be in [1, 64]"),
        (dict(base, M=9, K=72, ldw=72, ldx=72), "9..64 rows need"), (dict(fp8, M=9), "9..64 rows need"), (dict(base, M=9, x_ids=P["ids"]), "9..64 rows need"),
        (dict(base, M=2, x_ids=P["ids"]), "gathered input"), (dict(base, K=2112, ldw=2112, ldx=2112, x_ids=P["ids"], norm=2), "gathered input"),
        (dict(base, K=12, ldw=16), "multiple of 8"), (dict(base, N=0), "multiple of 8"),
        (dict(base, ldw=K + 4), "weight rows"), (dict(base, w=P["w16"] + 2), "weight rows"), (dict(base, ldw=K - 8), "weight rows"),
        (dict(base, ldx=K + 2), "x rows"), (dict(base, x=P["x"] + 4), "x rows"),
        (dict(base, wdtype=3), "wdtype must be"),
        (dict(fp8, K=24, ldw=32), "fp8 weights need"), (dict(fp8, wscale=None), "fp8 weights need"), (dict(base, wscale=P["ws"]), "wscale belongs"),
        (dict(base, glu=1, N=31), "glu needs"), (dict(base, glu=1, res=P["y2"], ldr=N), "glu needs"), (dict(base, glu=1, colscale=P["ws"]), "glu needs"),
        (dict(base, glu=1, post_act=3), "glu needs"), (dict(base, glu=1, y2=P["y2"], ldy2=N, split=16), "glu needs"),
        (dict(base, norm=3), "norm must be"), (dict(base, norm=-1), "norm must be"),
        (dict(base, norm=1, norm_weight=P["aux"] + 4), "norm weight / bias"), (dict(base, norm=2, norm_bias=P["aux"] + 8), "norm weight / bias"),
        (dict(base, y2=P["y2"], ldy2=N, split=0), "split must be inside"), (dict(base, y2=P["y2"], ldy2=N, split=N), "split must be inside"),
        (dict(base, y2=P["y2"], ldy2=N, split=8, y2_dtype=3), "y2_dtype"), (dict(base, y2_dtype=-1), "y2_dtype"),
        (dict(base, M=5, **rope), "fused rope"), (dict(base, **dict(rope, rope_sin=None)), "fused rope"), (dict(base, **dict(rope, rope_dh=15)), "fused rope"),
        (dict(base, **dict(rope, rope_cols=40)), "fused rope"), (dict(base, glu=1, **rope), "fused rope"), (dict(base, post_act=3, **rope), "fused rope"),
        (dict(base, y2=P["y2"], ldy2=N, split=7, **rope), "fused rope"),
        (dict(base, **dict(attn, attn_Tk=65)), "attention prologue"), (dict(base, M=2, **attn), "attention prologue"), (dict(base, norm=2, **attn), "attention prologue"),
        (dict(base, **dict(attn, attn_dh=32, attn_heads=4, attn_kv_heads=4)), "attention prologue"), (dict(base, **dict(attn, attn_v=None)), "attention prologue"),
        (dict(base, w_policy=2), "w_policy"),
    ]


def rows_gemm_refusals(P):
    K, N, R, M = 320, 128, 16, 9
    g = dict(wt=P["wt"], wdtype=0, N=N, K=K, planes=P["planes"], M=M, R=R, part=P["part"], ldp=N, kg_stride=M * N, kgroups=1)
    return [
        (dict(g, wt=None), "null tensor"), (dict(g, part=None), "null tensor"),
        (dict(g, part=None, glu_planes_out=P["po"], kgroups=2), "fused SwiGLU"), (dict(g, part=None, glu_planes_out=P["po"], N=192), "fused SwiGLU"),
        (dict(g, part=None, glu_planes_out=P["po"] + 2), "fused SwiGLU"),
        (dict(g, wdtype=3), "wdtype must be"), (dict(g, K=72), "multiple of 64"), (dict(g, K=0), "multiple of 64"), (dict(g, N=0), "multiple of 64"),
        (dict(g, R=48), "16, 32 or 64 rows"), (dict(g, M=17), "M must be in [1, R]"), (dict(g, M=0), "M must be in [1, R]"),
        (dict(g, wt=P["wt"] + 2), "16-byte aligned"), (dict(g, planes=P["planes"] + 4), "16-byte aligned"),
        (dict(g, ldp=N - 1), "bad slab geometry"), (dict(g, kgroups=0), "bad slab geometry"), (dict(g, kgroups=6), "bad slab geometry"),
        (dict(g, kgroups=2, kg_stride=M * N - 4), "slabs overlap"),
        (dict(g, kgroups=4), "leave empty slabs"),          # 5 k steps in groups of 2: three groups hold steps
    ]


def rows_finish_refusals(P):
    K, N, R, M = 320, 128, 16, 9
    f = dict(part=P["part"], kgroups=1, kg_stride=M * N, ldp=N, M=M, N=N, y=P["y"], ldy=8200)
    return [
        (dict(f, part=None), "null input"), (dict(f, M=0), "bad shape"), (dict(f, N=0), "bad shape"), (dict(f, kgroups=0), "bad shape"),
        (dict(f, ldp=N + 2), "16-byte aligned"), (dict(f, kg_stride=M * N + 2), "16-byte aligned"), (dict(f, part=P["part"] + 4), "16-byte aligned"),
        (dict(f, glu=1, N=127), "glu needs"), (dict(f, glu=1, res=P["y2"], ldr=N), "glu needs"), (dict(f, glu=1, colscale=P["aux"]), "glu needs"),
        (dict(f, glu=1, post_act=3), "glu needs"), (dict(f, glu=1, y2=P["y2"], ldy2=N, split=8), "glu needs"),
        (dict(f, N=13, ldp=12), "whole 8-column pieces"), (dict(f, glu=1, N=120), "whole 8-column pieces"),
        (dict(f, N=8200, ldp=8200, norm=1), "a normalised row has at most"), (dict(f, glu=1, N=16400, ldp=16400, norm=2), "a normalised row has at most"),
        (dict(f, norm=1, norm_weight=P["aux"] + 4), "norm weight / bias"), (dict(f, norm=2, norm_bias=P["aux"] + 8), "norm weight / bias"),
        (dict(f, norm=3), "norm must be"),
        (dict(f, y2=P["y2"], ldy2=N, split=0), "split destination"), (dict(f, y2=P["y2"], ldy2=N, split=N), "split destination"),
        (dict(f, y2=P["y2"], ldy2=N, split=8, planes=P["po"], R=16), "split destination"), (dict(f, y2=P["y2"], ldy2=N, split=8, norm=1), "split destination"),
        (dict(f, yn=P["y2"], ldyn=N), "yn without a norm"),
        (dict(f, y2=P["y2"], ldy2=N, split=8, y2_dtype=3), "y2_dtype"),
        (dict(f, planes=P["po"], R=48), "planes need"), (dict(f, planes=P["po"], R=16, M=9, N=72, ldp=72), "planes need"), (dict(f, planes=P["po"], R=16, planes_dtype=2), "planes need"),
        (dict(f, planes=P["po"] + 2, R=16), "planes need"), (dict(f, planes=P["po"], R=16, M=17), "planes need"),
        (dict(f, y=None), "no destination"),
    ]


# ----------------------------------------------------------------------------------------------------------------- required labels
def required_labels():
    """Family x instantiation x both sides of each switch: every label here must be carried by at least one case."""
    req = [f"gemv1_stream<NC={nc},{wt},NT={nt},HALF={h}>" for nc in (1, 2) for wt in WTS for nt in (0, 1) for h in (0, 1)]
    req += [f"gemv1_splitk<{wt},NT={nt}>" for wt in WTS for nt in (0, 1)]
    req += [f"gemv_kernel<MT=1,NC=2,{wt}>" for wt in ("bf16", "fp8")]
    req += [f"gemv_kernel<MT=2,NC={nc},{wt}>" for nc in (1, 2) for wt in ("bf16",)] + ["gemv_kernel<MT=2,NC=1,fp16>", "gemv_kernel<MT=2,NC=1,fp8>"]
    req += [f"gemv_kernel<MT=4,NC=1,{wt}>" for wt in WTS] + ["gemv_kernel<MT=4,NC=2,fp16>", "gemv_kernel<MT=4,NC=2,fp8>"]
    req += [f"gemv_kernel<MT=8,NC=2,{wt}>" for wt in WTS]
    req += [f"gemv_kernel/MT={mt}/{s}" for mt in (2, 4, 8) for s in ("one chunk", "chunks")]
    req += [f"gemv_kernel/norm/{s}" for s in ("LDS copy", "registers", "k loop")]
    req += [f"gemv_mfma<{wt}>" for wt in ("bf16", "fp16")] + ["gemv_mfma/idle waves", "gemv_mfma/every wave has a step"]
    req += [f"gemv_mfma_fp8<TPW={t}>" for t in (1, 2, 4)] + ["gemv_mfma_fp8/one chunk", "gemv_mfma_fp8/chunks", "gemv_mfma_fp8/last workgroup short",
                                                              "gemv_mfma_fp8/whole workgroups"]
    req += [f"gemm_rows<MR={mr},{wt}>" for mr in (1, 2, 4) for wt in ("bf16", "fp16")]
    req += [f"gemm_rows/MR={mr}/{s}" for mr in (1, 2, 4) for s in ("one chunk", "two chunks", "chunk ring refilled")]
    req += [f"gemm_rows/{s}" for s in ("tiles<512", "tiles=512", "tiles>512", "tiles>T*512")]
    return req


def required_rows_labels():
    req = [f"rows_gemm<MR={mr},T={t},{wt}>" for mr in (1, 2, 4) for t in (1, 2, 4) for wt in WTS]
    req += [f"rows_finish_lean<{f},NP={p}>" for f in ("bf16", "fp16") for p in (1, 2)] + ["rows_finish<bf16>", "rows_finish<fp16>"]
    return req
