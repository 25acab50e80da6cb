"""TEST INFRASTRUCTURE shared by tests/test_conv_kernel_edges_gpu.py and tests/test_conv_refs_cpu.py: the case tables of ``mi355_conv_gemm`` (csrc/conv_gemm.hip,
conv_ws4.h, conv_ws4*.hip), its dispatcher and the tile scheduler of the wave-specialised kernel restated as pure functions, the reference statements, their
mutants and the per-element bounds of the float cases.  CPU only: nothing here touches ``mlx_audio_amd.ops``, a device or the environment.

Exact cases.  The prologue output t, the weights and every epilogue operand are integers (or dyadic numbers) such that every product and every partial sum
of the kernel's arithmetic is exactly representable in float32: sum |t| |w| over a receptive field, the epilogue operands included and counted in units of
the smallest quantum a case can produce, stays below 2^24 (``budget``; tests/test_conv_refs_cpu.py asserts it case by case).  The result is then
independent of the accumulation order, of the tile shape and of the kernel family, and must equal the float64 convolution BIT FOR BIT.  Three flavours
of t, by what the launch's activation format holds exactly:

  'n'  precisions 1 and 3: integers in [-4, 4] (negative ones times 4 under a LeakyReLU prologue) -- one bf16 / fp16 image holds them;
  'w'  precisions 2 and 4: the same, with sparse WIDE elements +-(2049 .. 4095, odd; negative ones times 4 under LeakyReLU): 12 .. 14 significant
       bits, more than a bf16 (8) or fp16 (11) hi image holds, so a dropped or misplaced lo image changes the sum;
  'm'  precisions 5 and 6: sparse wide elements +-(8192 + 8 j + r), r in +-{1, 2, 3}: fp16 hi part 8192 + 8 j, residual r on the e4m3 / e2m1 grid of
       its row-and-chunk block whatever the block's maximum is (1, 2 or 3).
Weights: integers from {0, +-1, +-2, +-3, +-4, +-6}, every column with |w[n, 0, 0]| in {4, 6} (the FP4 column scale is then 1, the e4m3 one 2^-5) except
one all-zero column.  x is derived from t through the inverse of the case's AdaIN affine (integer shifts, scales from {1, -1, 2, -2}).

Float cases cover what cannot be made exact (Snake, SnakeBeta, ELU prologues; GELU, SiLU, GELU-tanh epilogues): per element

    bound = 4 e32 + 1e-6 peak + g(precision) * sum |t| |w| * |d epilogue|        (docs/PARITY.md; e32 = the statement's own float32 evaluation error)

with g = 2^-16 (precision 2), 2^-22 (4), 2^-9 (1: one bf16 rounding), 2^-12 (3: one fp16 rounding) and the existing per-tensor bars as caps.
Precisions 5 / 6 compare with oracle/mx_ref on the float64 prologue value: 4 e32 + 1e-6 peak plus ``mx_prologue_term`` -- the MX image is a step function
of t, and the kernel's float32 Snake may sit on the other side of a step.
"""
import math
import zlib

import numpy as np
import torch

SENTINEL = -777.25          # exactly representable; no case produces it
ENV_KNOBS = ("MI355_CONV_SPLIT", "MI355_CONV_SPLIT_MINSTEPS", "MI355_CONV_FINISH_OLD", "MI355_CONV_NOVEC_FLAT", "MI355_CONV_WS_FEAT", "MI355_CONV_WS_MIN_TILES",
             "MI355_CONV_NO_WS", "MI355_CONV_NO_WS64", "MI355_CONV_WS_WG_PER_CU", "MI355_CONV_SPLIT_WS_MB")   # read once per process: none may be set
POSTS = {"none": 0, "leaky": 0, "gelu": 1, "silu": 2, "gelu_tanh": 3}       # epi_family (conv_ws4.h)
TILE_CAPS = {1: 1.5e-2, 2: 3e-5, 3: 2e-3, 4: 3e-6, 5: 3e-5, 6: 2e-4}       # the per-tensor bars of tests/test_kernels_gpu.py / test_conv_mx_gpu.py: kept as caps
G_FORMAT = {1: 2.0 ** -9, 2: 2.0 ** -16, 3: 2.0 ** -12, 4: 2.0 ** -22}
WS_MIN_TILES = 128
SPLIT_WS_BYTES = 96 << 20    # ops.SPLIT_WS_BYTES without its knob

# ----------------------------------------------------------------------------------------------------------------- instantiation lists, restated
# (mode, PRE, epilogue family, tile columns); tests/test_conv_refs_cpu.py parses the WS4_* lines of the six .hip files and compares


def _ws4_list(conv128, gemm128, conv64, gemm64):
    return ([("conv", p, e, 128) for p, e in conv128] + [("gemm", "NONE", e, 128) for e in gemm128] + [("conv", p, 0, 64) for p in conv64] +
            [("gemm", "NONE", e, 64) for e in gemm64])


_FULL = [("NONE", 0), ("LEAKY", 0), ("SNAKE", 0), ("SNAKEBETA", 0), ("ELU", 0), ("NONE", 1)]
_THREE = [("NONE", 0), ("LEAKY", 0), ("SNAKE", 0)]
WS4_LISTS = {
    2: _ws4_list(_FULL, (0, 1, 2, 3), ("NONE", "LEAKY", "SNAKE", "ELU"), (0,)),
    4: _ws4_list(_FULL, (0, 1, 2, 3), ("NONE", "LEAKY", "SNAKE", "ELU"), (0,)),
    1: _ws4_list(_THREE, (0, 1), ("NONE", "LEAKY", "SNAKE"), (0,)),
    3: _ws4_list(_THREE + [("NONE", 1)], (0, 1), ("NONE", "LEAKY", "SNAKE"), (0,)),
    5: _ws4_list(_THREE, (), (), ()),
    6: _ws4_list(_THREE, (), (), ()),
}
WS4_FQ_LIST = [(p, bn) for bn in (128, 64) for p in ("NONE", "LEAKY", "SNAKE")]


def ws4_label(prec, mode, pre, epi, bn, fq=False, two_by_two=False):
    if fq:
        return f"ws4/p2/fq/{pre}/bn{bn}"
    return f"ws4/p{prec}/{mode}/{pre}/epi{epi}/bn{bn}" + ("/2x2" if two_by_two else "")


def all_ws4_labels():
    out = [ws4_label(p, m, pre, e, bn) for p, lst in WS4_LISTS.items() for m, pre, e, bn in lst]
    out += [ws4_label(2, "conv", p, 0, bn, fq=True) for p, bn in WS4_FQ_LIST]
    out.append(ws4_label(5, "conv", "SNAKE", 0, 128, two_by_two=True))     # mi355_conv_ws4_p5, feature digit 2
    return out


def all_4wave_labels():
    out = [f"4wave/p{p}/{t}/vec" for p in (1, 2, 3, 4) for t in ("128x128", "64x128", "64x64")]
    out += [f"4wave/p{p}/64x64/novec" for p in (2, 3, 4)]
    out += [f"splitk/p{p}/{t}" for p in (1, 2, 3, 4) for t in ("64x128", "64x64")]
    return out


# ----------------------------------------------------------------------------------------------------------------- the dispatcher, restated
def launch(**kw):
    """One call of ops.conv_gemm as the dispatcher sees it (defaults = the keyword defaults of ops.conv_gemm on aligned, contiguous tensors)."""
    d = dict(B=1, L=1, Lout=None, Cin=32, Cout=32, K=1, dil=1, pad=0, precision=2, tile=0, pre="NONE", affine=False, fq=False, post="none", res=False,
             res_shift=0, accumulate=False, colscale=False, up_s=0, stats=False, stats_aligned=True, vec=True, split_ws=True, x_split=False,
             y_split=False, lens_in=None, lens_out=None, out_aligned=True, resident=0, cus=256)
    assert set(kw) <= set(d), set(kw) - set(d)
    d.update(kw)
    if d["Lout"] is None:
        d["Lout"] = d["L"]
    return d


def gemm_mode(a):
    return a["K"] == 1 and a["Cin"] >= 64 and a["pre"] == "NONE" and not a["affine"] and not a["fq"]       # gemm_mode (conv_ws4.h)


def ws4_eligible(a, prec):
    """mi355_conv_ws4_eligible (conv_ws4.hip); flattened strided convs are not part of this suite."""
    if not a["vec"] or a["L"] <= 0:
        return False
    win = 128 + (a["K"] - 1) * a["dil"]
    if prec in (5, 6):
        return a["K"] % 4 == 3 and win <= 192 and a["Cout"] > 64 and not a["fq"] and a["pre"] in ("NONE", "LEAKY", "SNAKE") and POSTS[a["post"]] == 0
    if not gemm_mode(a) and win > 192:
        return False
    return 1 <= prec <= 4


def ws4_facts(a, prec, mode, pre, bn, feat, fq):
    """The geometry route_ws4 decides, the grid ws4_grid sizes at launch time (conv_ws4.h, conv_ws4.hip) and the run-time branches the launch's tiles take."""
    chunks32 = (a["Cin"] + 31) >> 5
    gemm = mode == "gemm"
    nch = (chunks32 + 1) >> 1 if gemm else chunks32
    R = 256 if gemm else 128 + (a["K"] - 1) * a["dil"]
    tpi = (a["Lout"] + 127) // 128
    P, NT = a["B"] * tpi, (a["Cout"] + bn - 1) // bn
    fold = int((a["res"] or a["accumulate"]) and a["post"] == "none" and a["up_s"] == 0 and a["res_shift"] == 0 and not a["colscale"])
    glog = 3 if P >= 512 else (2 if P >= 256 else (1 if P >= 128 else 0))
    per = 8 << glog
    total = (P + per - 1) // per * per * NT
    resident = (a["resident"] + 7) // 8 * 8 if a["resident"] > 0 else (a["cus"] * 2) // 8 * 8
    grid = total if (feat & 8) or total <= resident else resident
    mxp = prec in (5, 6)
    fastw = not fq and (mxp or gemm or pre in ("NONE", "LEAKY"))
    fastw_off = (not mxp) and bool(feat & 2)
    lens_in = a["lens_in"] or [a["L"]] * a["B"]
    lens_out = a["lens_out"] or [a["Lout"]] * a["B"]
    interior = masked = 0
    tiles = 0
    for b in range(a["B"]):
        for l0 in range(0, lens_out[b], 128):
            tiles += 1
            for ci in range(nch):
                if gemm:
                    it = l0 + 128 <= lens_in[b] and l0 + 128 <= a["L"] and ci * 64 + 64 <= a["Cin"]
                else:
                    r0 = l0 - a["pad"]
                    it = r0 >= 0 and r0 + R <= lens_in[b] and r0 + R <= a["L"] and ci * 32 + 32 <= a["Cin"]
                if fastw and not fastw_off and it:
                    interior += 1
                else:
                    masked += 1
    return dict(tiles_per_item=tpi, P=P, NT=NT, fold=fold, glog=glog, total_ids=total, nch=nch, R=R, grid=grid, walk=grid < total, feat=feat, bn=bn,
                interior=interior > 0, masked=masked > 0, live_tiles=tiles * NT, odd_nch=gemm and chunks32 % 2 == 1)


def ws4_launch(a, prec, feat, bn):
    """mi355_conv_ws4_route and the per-precision lists (conv_ws4.hip, conv_ws4_{p4,p13,p5,p6,fq}.hip) -> (label, facts) or None (MI355_ERR_UNSUPPORTED)."""
    pre, epi = a["pre"], POSTS.get(a["post"], -1)
    assert feat < 16 and not (prec == 2 and feat & 4) and not (prec == 6 and feat & ~9) and not (prec == 5 and feat & ~11), "ablation / probe builds are not part of this suite"
    if a["fq"]:
        if prec != 2 or epi != 0 or (pre, bn) not in WS4_FQ_LIST:
            return None
        feat &= 3
        return ws4_label(2, "conv", pre, 0, bn, fq=True), ws4_facts(a, 2, "conv", pre, bn, feat, True)
    mode = "gemm" if (gemm_mode(a) and prec not in (5, 6)) else "conv"
    if prec == 5 and (feat & 2) and pre == "SNAKE" and epi == 0:
        return ws4_label(5, "conv", pre, 0, 128, two_by_two=True), ws4_facts(a, 5, "conv", pre, 128, feat & 9, False)
    feat &= {2: 15, 4: 3, 1: 3, 3: 3, 5: 11, 6: 9}[prec]
    key = (mode, "NONE" if mode == "gemm" else pre, epi, bn)
    if key not in WS4_LISTS[prec]:
        return None
    return ws4_label(prec, *key), ws4_facts(a, prec, mode, key[1], bn, feat, False)


def split_groups(wgs, nchunks, K, rows_total, Cout, ws_bytes, forced):
    """split_groups (conv_gemm.hip) without its knobs."""
    if nchunks < 2:
        return 0
    min_chunks = 1 if K >= 4 else (4 + K - 1) // K
    ks = forced
    if ks <= 0:
        if forced == 0 and ((wgs > 128 and not (wgs < 256 and nchunks * K >= 24)) or nchunks * K < 8):
            return 0
        ks = max(2, (512 + wgs - 1) // wgs)
    ks = min(ks, nchunks // min_chunks)
    per = rows_total * ((Cout + 3) & ~3) * 4
    if per <= 0 or ws_bytes // per < 2:
        return 0
    ks = min(ks, ws_bytes // per)
    if ks < 2:
        return 0
    cpz = (nchunks + ks - 1) // ks
    ks = (nchunks + cpz - 1) // cpz
    return ks if ks >= 2 else 0


def _lds_ok(a, prec, bm, bn):
    R = bm + (a["K"] - 1) * a["dil"]
    return R * 64 * (2 if prec in (2, 4) else 1) + 2 * (bn // 32) * 2048 <= 64 * 1024                     # conv_lds_bytes (conv_gemm.hip)


def _split(a, prec, wide, ks):
    if not _lds_ok(a, prec, 64, 128 if wide else 64):
        return "refuse:window too large for LDS", None
    lean = not a["up_s"] and a["Cout"] % 4 == 0 and a["out_aligned"]                                       # conv_decide's `lean` (conv_gemm.hip)
    return f"splitk/p{prec}/{'64x128' if wide else '64x64'}/" + ("lean" if lean else "general"), dict(groups=ks)


def route(a):
    """mi355_conv_gemm's dispatch (conv_validate and conv_decide, conv_gemm.hip) -> (label, facts).  facts is the ws4 geometry for a ws4 label, the group count for a split-K
    label, else None.  Labels: ws4/..., 4wave/p<P>/<BM>x<BN>/vec|novec, splitk/p<P>/<tile>/lean|general, each prefixed 'mx->p4 fallback ' when an MX image
    runs the precision-4 arithmetic, or refuse:<reason>."""
    prec = a["precision"] or 2
    if prec in (5, 6) and a["fq"]:
        return "refuse:precisions 5 / 6 have no quantising prologue", None
    if a["fq"] and a["pre"] not in ("NONE", "LEAKY", "SNAKE"):
        return "refuse:pre_fq prologue", None
    vec, tile = a["vec"], a["tile"]
    assert tile // 100000000 == 0, "ablation builds are not part of this suite"
    code, digit = tile % 10000000, tile // 10000000
    if a["stats"]:
        if a["up_s"]:
            return "refuse:fused statistics need a plain store", None
        if not a["stats_aligned"]:
            return "refuse:stats_partial must be 8-byte aligned", None
    split_ws = a["split_ws"] and a["B"] * a["Lout"] <= 65536
    if a["y_split"]:
        if a["accumulate"]:
            return "refuse:y_split cannot accumulate", None
        split_ws = False
    if a["x_split"]:
        if prec not in (2, 4):       # (ops.conv_gemm passes x_split = precision)
            return "refuse:x_split must equal the precision, 2 or 4", None
        if a["pre"] != "NONE" or a["affine"] or a["fq"] or not ws4_eligible(a, prec):
            return "refuse:x_split needs the wave-specialised kernel", None
        r = ws4_launch(a, prec, 0, 64) if a["Cout"] <= 64 else ws4_launch(a, prec, digit if code == 6128128 else 0, 128)
        return r if r else ("refuse:no instantiation", None)
    mx = ""
    if prec in (5, 6):
        wgs128 = a["B"] * ((a["Lout"] + 127) // 128) * ((a["Cout"] + 127) // 128)
        want = code == 6128128 or (tile == 0 and a["Cout"] > 64 and wgs128 >= WS_MIN_TILES and a["Cin"] >= 64)
        if want and ws4_eligible(a, prec):
            r = ws4_launch(a, prec, 0 if tile == 0 else digit, 128)
            if r:
                return r
        if code == 6128128:
            return "refuse:precisions 5 / 6 on the wave-specialised tile", None
        mx, prec = "mx->p4 fallback ", 4
    if tile == 0:
        bn = 64 if a["Cout"] <= 64 else 128
        wgs128 = a["B"] * ((a["Lout"] + 127) // 128) * ((a["Cout"] + bn - 1) // bn)
        bm = 128 if (bn == 128 and wgs128 >= 512) else 64
        code = bm * 1000 + bn
        if not mx and bn == 128 and wgs128 >= WS_MIN_TILES and (a["Cin"] >= 64 or wgs128 >= 2048) and ws4_eligible(a, prec):
            r = ws4_launch(a, prec, 0, 128)
            if r:
                return r
        if not mx and bn == 64 and wgs128 >= WS_MIN_TILES and a["Cin"] >= 32 and ws4_eligible(a, prec):
            r = ws4_launch(a, prec, 0, 64)
            if r:
                return r
        if bn == 128 and wgs128 >= 512:
            code = 64128
        if split_ws and vec:
            wgs64 = a["B"] * ((a["Lout"] + 63) // 64) * ((a["Cout"] + bn - 1) // bn)
            ks = split_groups(wgs64, (a["Cin"] + 31) >> 5, a["K"], a["B"] * a["Lout"], a["Cout"], SPLIT_WS_BYTES, 0)
            if ks:
                lab, f = _split(a, prec, bn == 128, ks)
                return mx + lab if f else lab, f
    if code in (2064128, 2064064):
        if not (vec and split_ws):
            return "refuse:the split-K tiles need the aligned input path and a workspace", None
        wide = code == 2064128
        wgs64 = a["B"] * ((a["Lout"] + 63) // 64) * ((a["Cout"] + (127 if wide else 63)) // (128 if wide else 64))
        ks = split_groups(wgs64, (a["Cin"] + 31) >> 5, a["K"], a["B"] * a["Lout"], a["Cout"], SPLIT_WS_BYTES, digit if digit else -1)
        if ks < 2:
            return "refuse:nothing to split", None
        lab, f = _split(a, prec, wide, ks)
        return mx + lab if f else lab, f
    if code == 6128064:
        if mx:
            return "refuse:MX images have no 128 x 64 wave-specialised tile", None
        if not ws4_eligible(a, prec):
            return "refuse:the wave-specialised tile needs aligned rows and a window of <= 192 rows", None
        r = ws4_launch(a, prec, digit & 11, 64)
        return r if r else ("refuse:no instantiation", None)
    if code == 6128128:
        if not ws4_eligible(a, prec):
            return "refuse:the wave-specialised tile needs aligned rows and a window of <= 192 rows", None
        r = ws4_launch(a, prec, digit, 128)
        return r if r else ("refuse:no instantiation", None)
    if a["stats"]:
        if not vec:
            return "refuse:fused statistics need the aligned input path", None
        code = 128128
    if not vec:
        p = prec if prec in (3, 4) else 2
        return (mx + f"4wave/p{p}/64x64/novec", None) if _lds_ok(a, p, 64, 64) else ("refuse:window too large for LDS", None)
    if code not in (128128, 64128, 64064):
        return f"refuse:unsupported tile {code}", None
    bm, bn = code // 1000, code % 1000
    if not _lds_ok(a, prec, bm, bn):
        return "refuse:window too large for LDS", None
    return mx + f"4wave/p{prec}/{bm}x{bn}/vec", None


# ----------------------------------------------------------------------------------------------------------------- route() against the library
PRE_NAMES = ("NONE", "LEAKY", "SNAKE", "SNAKEBETA", "ELU")         # mi355_conv_route.pre
PRE_ACTS = dict(NONE="ACT_NONE", LEAKY="ACT_LEAKY", SNAKE="ACT_SNAKE", SNAKEBETA="ACT_SNAKE", ELU="ACT_ELU")
POST_ACTS = dict(none="ACT_NONE", leaky="ACT_LEAKY", gelu="ACT_GELU", silu="ACT_SILU", gelu_tanh="ACT_GELU_TANH")
ROUTE_GEOMETRY = ("tiles_per_item", "P", "NT", "nch", "R", "fold", "glog", "total_ids", "bn", "feat")


def route_args(a, acts):
    """A ``launch(**kw)`` dict as the keywords of ``mi355_conv_gemm_args`` for ``mi355_conv_gemm_route``, which follows no pointer: the addresses are made
    up -- 16-byte aligned where the dict says aligned, 4 bytes past that for ``vec=False`` / ``out_aligned=False`` / ``stats_aligned=False``, None where
    the dict says absent.  ``acts``: where the MI355_ACT_* values come from (``mlx_audio_amd.ops``).  Rows are dense: ld = the channel count rounded up
    to 4.  The workspace follows the rule of ``ops.conv_gemm`` (B * Lout <= 65536)."""
    at = lambda n: 0x10000000 + (n << 20)
    B, L, Lout, Cin, Cout, prec = a["B"], a["L"], a["Lout"], a["Cin"], a["Cout"], a["precision"]
    ldx, ldy = round_up(Cin, 4), round_up(Cout, 4)
    snake = a["pre"] in ("SNAKE", "SNAKEBETA")
    kw = dict(x=at(1) + (0 if a["vec"] else 4), x_bstride=L * ldx, ldx=ldx, x_off=0, Cin=Cin, Lin=L, lens_in=at(2) if a["lens_in"] else None, flat_valid=0, w=at(3), Cout=Cout,
              K=a["K"], dil=a["dil"], pad=a["pad"], pre_act=getattr(acts, PRE_ACTS[a["pre"]]), pre_slope=0.25, pre_alpha=at(4) if snake else None,
              pre_inv_beta=at(5) if a["pre"] == "SNAKEBETA" else None, bias=at(6), post_act=getattr(acts, POST_ACTS[a["post"]]), post_slope=0.5, out_scale=1.0,
              accumulate=int(a["accumulate"]), y=at(7) + (0 if a["out_aligned"] else 4), y_bstride=Lout * ldy, ldy=ldy, Lout=Lout, lens_out=at(8) if a["lens_out"] else None, B=B,
              precision=prec, tile=a["tile"], post_colscale=at(9) if a["colscale"] else None, x_split=prec if a["x_split"] else 0, y_split=prec if a["y_split"] else 0)
    if a["affine"]:
        kw.update(pre_scale=at(10), pre_shift=at(11), pre_ld=round_up(Cin, 32))
    if a["fq"]:
        kw.update(pre_fq=at(12))
    if a["res"]:
        kw.update(res=at(13), res_bstride=Lout * ldy, ldr=ldy, res_shift=a["res_shift"])
    if a["up_s"]:
        kw.update(up_s=a["up_s"], up_p=0, up_cout=Cout // a["up_s"], up_row_off=0, up_Lout=Lout * a["up_s"])
    if a["stats"]:
        kw.update(stats_partial=at(14) + (0 if a["stats_aligned"] else 4), stats_bstride=((Lout + 63) // 64) * Cout * 2)
    if a["split_ws"] and B * Lout <= 65536:
        kw.update(split_ws=at(15), split_ws_bytes=SPLIT_WS_BYTES)
    return kw


def record_label(r):
    """A ``mi355_conv_route`` record (dict) in the label format of route()."""
    mx = "mx->p4 fallback " if r["mx_fallback"] else ""
    if r["family"] == 2:
        assert not mx and not r["dbg"] and not r["abl"], r
        return ws4_label(r["precision"], "gemm" if r["gemm"] else "conv", PRE_NAMES[r["pre"]], r["epi"], r["bn"], fq=bool(r["fq"]), two_by_two=bool(r["two_by_two"]))
    if r["family"] == 1:
        return mx + f"splitk/p{r['precision']}/{r['bm']}x{r['bn']}/" + ("lean" if r["lean"] else "general")
    return mx + f"4wave/p{r['precision']}/{r['bm']}x{r['bn']}/" + ("vec" if r["vec"] else "novec")


def polyphase_launches():
    """The launches of tests/test_conv_kernel_edges_gpu.py::test_polyphase_store_exact as route() sees them."""
    return [launch(B=2, L=300, Lout=301, Cin=128, Cout=128, K=2, pad=1, pre="LEAKY", res=True, precision=prec, tile=tile, up_s=4, lens_in=[300, 77], lens_out=[301, 78])
            for prec in (2, 4) for tile in (0, WS, 80000000 + WS, 128128, 2064128)]


# ----------------------------------------------------------------------------------------------------------------- the tile scheduler, restated
def decode_tile(i, P, NT, glog, tpi, lens_out, mutant=None):
    """decode_tile (conv_ws4.h): virtual id -> (item, first row, column tile) or None."""
    kq = i >> 3
    ny, pg = kq % NT, kq // NT
    g = glog + 1 if mutant == "glog" else glog
    p = ((((pg >> g) << 3) + (i & 7)) << g) | (pg & ((1 << g) - 1))
    if p >= P and mutant != "nocut":
        return None
    b = p // tpi
    l0 = (p - b * tpi) * 128
    if b < len(lens_out) and l0 >= lens_out[b]:
        return None
    return b, l0, ny


def workgroup_tiles(wg, grid, total_ids, P, NT, glog, tpi, lens_out, mutant=None, table=None):
    """The tiles one persistent workgroup visits: its first id with work, then next_work until -1 (conv_ws4.h).  ``table``:
    decode_tile of every id, computed once by the caller (the walk itself stays literal)."""
    dec = (lambda i: table[i]) if table is not None else (lambda i: decode_tile(i, P, NT, glog, tpi, lens_out, mutant))
    out = []
    i = wg - grid
    while True:
        i += grid
        while i < total_ids and dec(i) is None:
            i += grid
        if i >= total_ids:
            return out
        out.append((i, dec(i)))


def ids_to_p(P, NT, mutant=None):
    """Vectorised decode of every virtual id of a launch of P row tiles x NT column tiles -> (p, ny) arrays (p < 0 where the id is cut)."""
    glog = 3 if P >= 512 else (2 if P >= 256 else (1 if P >= 128 else 0))
    per = 8 << glog
    total = (P + per - 1) // per * per * NT
    i = np.arange(total)
    kq = i >> 3
    ny, pg = kq % NT, kq // NT
    g = glog + 1 if mutant == "glog" else glog
    p = ((((pg >> g) << 3) + (i & 7)) << g) | (pg & ((1 << g) - 1))
    if mutant != "nocut":
        p = np.where(p >= P, -1, p)
    return p, ny


# ----------------------------------------------------------------------------------------------------------------- statements
def ulp32(v):
    v = torch.as_tensor(v, dtype=torch.float64).abs().clamp_min(2.0 ** -126)
    return torch.pow(2.0, torch.floor(torch.log2(v)) - 23)


def hi_image(t, prec):
    """The hi image of the launch's activation format (float64 in and out): bf16 for precisions 1 / 2, fp16 for 3 .. 6."""
    t32 = t.float()
    return (t32.to(torch.bfloat16) if prec in (1, 2) else t32.clamp(-65504.0, 65504.0).to(torch.float16)).double()


def prologue(x, c, inp, b, dt=torch.float64):
    """t = act(x * scale[b] + shift[b]) for one item; x [L, Cin]."""
    t = x.to(dt)
    if c["affine"]:
        t = t * inp["sc"][b].to(dt) + inp["sh"][b].to(dt)
    pre = c["pre"]
    if pre == "LEAKY":
        t = torch.where(t >= 0, t, t * c["pre_slope"])
    elif pre == "SNAKE":
        al = inp["alpha"].to(dt)
        t = t + (1.0 / al) * torch.sin(al * t) ** 2
    elif pre == "SNAKEBETA":
        t = t + inp["inv_beta"].to(dt) * torch.sin(inp["alpha"].to(dt) * t) ** 2
    elif pre == "ELU":
        t = torch.where(t > 0, t, torch.expm1(torch.clamp(t, max=0.0)))
    if c["fq"]:   # dynamic uint8 fake quantisation with the case's extrema {-min, max} = {127, 128}: scale exactly 1, zero point 127
        t = torch.clamp(torch.round(t + 127.0), 0, 255) - 127.0
    return t


def post_act(v, c):
    post = c["post"]
    if post == "leaky":
        return torch.where(v >= 0, v, v * c["post_slope"])
    if post == "gelu":
        return 0.5 * v * (1.0 + torch.erf(v / math.sqrt(2.0)))
    if post == "silu":
        return v * torch.sigmoid(v)
    if post == "gelu_tanh":
        return 0.5 * v * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (v + 0.044715 * v ** 3)))
    return v


MUTANTS = ("halo_clamp", "chan_pad_read", "last_tap_drop", "lo_drop", "cross_drop", "res_shift_ignored", "rows_127_128", "mx_scale", "mx_tap_swap")


def conv_rows(t, w, dil, pad, len_out, mutant=None, lo=None):
    """sum_k t[l - pad + k dil] w[:, k]^T for l < len_out, rows outside [0, len(t)) zero.  t [len_in, Cin], w [Cout, K, Cin] -> [len_out, Cout].
    ``lo``: an optional second image added tap by tap (the mutants of the lo pass act on it)."""
    n, K = t.shape[0], w.shape[1]
    y = torch.zeros((len_out, w.shape[0]), dtype=t.dtype)
    if n == 0:
        return y
    l = torch.arange(len_out)
    for k in range(K):
        rows = l - pad + k * dil
        ok = (rows >= 0) & (rows < n)
        if mutant == "halo_clamp":      # a halo row clamped where it should be zero
            rows, ok = rows.clamp(0, n - 1), torch.ones_like(ok)
        if mutant == "last_tap_drop" and k == K - 1:   # the last tap loses the item's last row
            ok = ok & (rows != n - 1)
        wk = w[:, k, :].to(t.dtype).t()
        y[ok] += t[rows[ok]] @ wk
        if lo is not None and not (mutant == "cross_drop" and k == K // 2):
            kk = k ^ 1 if (mutant == "mx_tap_swap" and (k ^ 1) < K) else k       # the two tap halves of an MX tap pair swapped
            y[ok] += (lo[rows[ok]] * (2.0 if mutant == "mx_scale" else 1.0)) @ w[:, kk, :].to(t.dtype).t()
    return y


def epilogue(acc, c, inp, b, n_out, mutant=None, dt=torch.float64):
    """y = (act(acc + bias) * colscale + res[row >> res_shift] + old y) * out_scale (include/mi355audio.h)."""
    if mutant == "rows_127_128" and n_out > 128:    # rows 127 and 128 of an item exchanged (the seam of its first two tiles)
        acc = acc.clone()
        acc[[127, 128]] = acc[[128, 127]]
    v = acc
    if inp["bias"] is not None:
        v = v + inp["bias"].to(dt)
    v = post_act(v, c)
    if inp["colscale"] is not None:
        v = v * inp["colscale"].to(dt)
    if inp["res"] is not None:
        rr = torch.arange(n_out) >> (0 if mutant == "res_shift_ignored" else c["res_shift"])
        v = v + inp["res"][b, rr].to(dt)
    if inp["old"] is not None:
        v = v + inp["old"][b, :n_out].to(dt)
    return v * c["out_scale"]


def statement(c, inp, prec=None, mutant=None, dt=torch.float64, only=None, absolute=False):
    """The whole launch in ``dt``: list over items of [len_out[b], Cout] (``only``: that item alone).  ``prec`` matters to the mutants of the hi + lo
    split only (None: the exact product).  ``absolute``: sum |t| |w| instead (the budget / the format term), without the epilogue."""
    out = []
    w = inp["w"]
    for b in range(c["B"]) if only is None else (only,):
        n_in, n_out = c["lens"][b], c["lens_out"][b]
        x = inp["x"][b, :n_in]
        t = prologue(x, c, inp, b, dt)
        if absolute:
            out.append(conv_rows(t.abs(), w.abs(), c["dil"], c["pad"], n_out))
            continue
        lo = None
        if mutant in ("lo_drop", "cross_drop", "mx_scale", "mx_tap_swap"):
            hi = hi_image(t, prec).to(dt)
            lo = None if mutant == "lo_drop" else t - hi
            t = hi
        if mutant == "chan_pad_read" and c["Cin"] % 32:
            # channels [Cin, Cin padded to 32) read instead of dropped, against the zero weights the packed image holds there: what is read is the input
            # buffer of tests/test_conv_kernel_edges_gpu.py -- NaN in the row's pad columns, and past the row's end the following memory (finite: stood in
            # for by channel 0) -- so only a buffer WITH pad columns shows the mutant (0 * NaN)
            cp = round_up(c["Cin"], 32)
            ld = round_up(int(c["unaligned"]) + c["x_off"] + c["Cin"], 4) + c["x_extra"]
            tp = t[:, :1].expand(-1, cp).clone()
            tp[:, :c["Cin"]] = t
            tp[:, c["Cin"]: max(c["Cin"], min(cp, ld - int(c["unaligned"]) - c["x_off"]))] = float("nan")
            wp = torch.zeros((w.shape[0], w.shape[1], cp), dtype=w.dtype)
            wp[:, :, :c["Cin"]] = w
            acc = conv_rows(tp, wp, c["dil"], c["pad"], n_out)
        else:
            acc = conv_rows(t, w, c["dil"], c["pad"], n_out, mutant, lo)
        out.append(epilogue(acc, c, inp, b, n_out, mutant, dt))
    return out


def mx_statement(c, inp, prec, mutant=None, only=None):
    """Precisions 5 / 6 through oracle/mx_ref's own conv_mx / conv_mx4 (same-length convs), then the epilogue in float64.  The MX mutants restate the lo
    pass from mx_ref's split_activation / quantise_weights."""
    from oracle import mx_ref

    out = []
    w = inp["w"].numpy().astype(np.float32)
    for b in range(c["B"]) if only is None else (only,):
        n = c["lens"][b]
        assert n == c["lens_out"][b]
        t = prologue(inp["x"][b, :n], c, inp, b).float().numpy()
        if n == 0:
            acc = torch.zeros((0, c["Cout"]), dtype=torch.float64)
        elif mutant is None:
            acc = torch.from_numpy((mx_ref.conv_mx if prec == 5 else mx_ref.conv_mx4)(t, w, c["dil"], c["pad"]))
        else:
            cp = (c["Cin"] + 31) // 32 * 32
            tp = np.zeros((n, cp), dtype=np.float32)
            tp[:, :c["Cin"]] = t
            hi, lo = (mx_ref.split_activation if prec == 5 else mx_ref.split_activation4)(tp)
            wq = (mx_ref.quantise_weights if prec == 5 else mx_ref.quantise_weights4)(w)
            hi, lo = torch.from_numpy(hi[:, :c["Cin"]]), torch.from_numpy(lo[:, :c["Cin"]])
            acc = conv_rows(hi, torch.from_numpy(w.astype(np.float16).astype(np.float64)), c["dil"], c["pad"], n, mutant if mutant in ("halo_clamp", "last_tap_drop") else None)
            if mutant != "lo_drop":
                zero = torch.zeros_like(lo)
                acc = acc + conv_rows(zero, torch.from_numpy(wq), c["dil"], c["pad"], n, mutant, lo)
        out.append(epilogue(acc, c, inp, b, n, mutant, torch.float64))
    return out


def flavour(prec):
    return {1: "n", 3: "n", 2: "w", 4: "w", 5: "m", 6: "m"}[prec]


# ----------------------------------------------------------------------------------------------------------------- cases
def _case(name, B, L, Cin, Cout, K, *, dil=1, pad=None, lens=None, pre="NONE", pre_slope=0.25, affine=False, fq=False, post="none", post_slope=0.5, bias=True,
          res=False, res_shift=0, accumulate=False, out_scale=1.0, colscale=False, precs=(1, 2, 3, 4), tiles=None, covers=(), claims=(), x_off=0, x_extra=0,
          y_extra=0, unaligned=False, exact=True, same=True, stats=False):
    pad = (K * dil - dil) // 2 if pad is None else pad
    lens = list(lens) if lens is not None else [L] * B
    assert len(lens) == B and max(lens) <= L
    # 'same' convs: len_out = len_in; otherwise a 'valid'-plus-pad length (even K: the right edge lacks context)
    lens_out = list(lens) if same else [max(0, n + 2 * pad - (K - 1) * dil) for n in lens]
    return dict(name=name, B=B, L=L, Cin=Cin, Cout=Cout, K=K, dil=dil, pad=pad, lens=lens, lens_out=lens_out, Lout=L if same else max(1, max(lens_out)), ragged=lens != [L] * B,
                pre=pre, pre_slope=pre_slope, affine=affine, fq=fq, post=post, post_slope=post_slope, bias=bias, res=res, res_shift=res_shift, accumulate=accumulate,
                out_scale=out_scale, colscale=colscale, precs=tuple(precs), tiles=tiles, covers=tuple(covers), claims=dict(claims), x_off=x_off, x_extra=x_extra,
                y_extra=y_extra, unaligned=unaligned, exact=exact, stats=stats)


WS, WS64 = 6128128, 6128064
WS_ALL = (WS, 10000000 + WS, 20000000 + WS, 80000000 + WS)          # feature digits 0, 1, 2 (masked body only), 8 (one workgroup per tile)
WS64_ALL = (WS64, 10000000 + WS64, 20000000 + WS64, 80000000 + WS64)
FOUR = (128128, 64128, 64064)
SPLITS = (2064128, 2064064)
EVERY = (0,) + WS_ALL + WS64_ALL + FOUR + SPLITS


def exact_cases():
    """Every exact case: the shapes at which each branch can still go wrong, each on every tile code in ``tiles`` that route() does not refuse."""
    E = "halo_clamp", "last_tap_drop"
    out = [
        # conv mode, 128-column tiles: seams, halos, interior + edge tiles, ragged channel counts
        _case("seam k3", 1, 257, 64, 128, 3, covers=E + ("lo_drop", "cross_drop", "rows_127_128"), claims=dict(interior=True, masked=True), tiles=EVERY),
        _case("seam k7 d3 leaky", 2, 400, 96, 130, 7, dil=3, pre="LEAKY", affine=True, res=True, accumulate=True, out_scale=0.5, covers=E + ("lo_drop", "cross_drop", "rows_127_128"),
              claims=dict(interior=True, masked=True, fold=1), tiles=EVERY, x_extra=8, y_extra=4),
        _case("res_shift 1", 2, 258, 64, 200, 3, res=True, res_shift=1, post="leaky", colscale=True, covers=E + ("res_shift_ignored", "rows_127_128", "lo_drop"),
              claims=dict(fold=0), tiles=EVERY),
        _case("k1 conv mode cin40", 1, 129, 40, 65, 1, covers=("chan_pad_read", "last_tap_drop", "lo_drop"), tiles=EVERY, x_extra=4),
        _case("k2 even", 2, 131, 96, 50, 2, pad=1, lens=(131, 64), covers=E + ("lo_drop",), tiles=EVERY),
        _case("valid k7 d3 no pad", 2, 300, 64, 128, 7, dil=3, pad=0, lens=(300, 150), same=False, covers=("last_tap_drop", "lo_drop", "rows_127_128"),
              claims=dict(interior=True, masked=True), tiles=EVERY, res=True),      # lens_out = lens_in - 18: the output is shorter than the input
        _case("k4 d2 cin160", 1, 129, 160, 22, 4, dil=2, pad=3, covers=E + ("lo_drop", "rows_127_128"), tiles=EVERY, y_extra=2),
        _case("k5 d16 window 192", 1, 260, 64, 128, 5, dil=16, covers=E + ("lo_drop", "cross_drop"), tiles=EVERY),
        _case("k5 d17 window 196", 1, 260, 64, 128, 5, dil=17, covers=E + ("lo_drop",), tiles=EVERY),      # the first shape past the window limit
        _case("k11 cin 7 chunks", 1, 130, 218, 64, 11, covers=E + ("chan_pad_read", "lo_drop", "cross_drop"), tiles=EVERY, x_extra=8),
        _case("L1", 3, 1, 64, 128, 3, covers=("halo_clamp",), tiles=EVERY),
        _case("L2 k3", 2, 2, 32, 64, 3, covers=E, tiles=EVERY),
        _case("L63..65 ragged", 4, 65, 64, 65, 7, lens=(63, 64, 65, 0), covers=E + ("lo_drop",), tiles=EVERY),
        _case("L127..129 ragged", 5, 129, 64, 128, 3, lens=(127, 128, 129, 1, 0), covers=E + ("lo_drop", "rows_127_128"), tiles=EVERY, accumulate=True),
        _case("L 128+pad+-1", 3, 132, 64, 128, 7, lens=(130, 131, 132), covers=E + ("lo_drop", "rows_127_128", "res_shift_ignored"), tiles=EVERY, res=True, res_shift=1),
        _case("x_off ldx", 2, 140, 64, 130, 3, x_off=4, x_extra=12, y_extra=8, covers=E + ("lo_drop", "rows_127_128"), tiles=EVERY, pre="LEAKY", pre_slope=0.5, post="leaky"),
        _case("unaligned view", 2, 70, 40, 50, 3, unaligned=True, x_extra=4, covers=E + ("chan_pad_read",), precs=(2, 3, 4), tiles=(0,) + FOUR + (WS, WS64, 2064064)),
        _case("ldx not a multiple of 4", 1, 66, 40, 65, 3, x_extra=2, covers=E + ("chan_pad_read",), tiles=(0,) + FOUR + (WS, 2064128)),
        # GEMM mode: 2, 3 and 5 chunks of 32 (an odd count leaves a half-empty super-chunk), interior and ragged rows
        _case("gemm 2 chunks", 2, 257, 64, 128, 1, lens=(257, 130), covers=("last_tap_drop", "lo_drop", "rows_127_128"), claims=dict(interior=True, masked=True), tiles=EVERY),
        _case("gemm 3 chunks", 1, 130, 96, 200, 1, covers=("last_tap_drop", "lo_drop", "rows_127_128"), claims=dict(odd_nch=True), tiles=EVERY, res=True, out_scale=2.0),
        _case("gemm 5 chunks cin150", 3, 64, 150, 64, 1, lens=(64, 1, 33), covers=("chan_pad_read", "last_tap_drop", "lo_drop"), claims=dict(odd_nch=True), tiles=EVERY, x_extra=4, post="leaky"),
        # MX images: K = 3 (mod 4) on the wave-specialised kernel, everything else on the precision-4 arithmetic of the 4-wave kernels
        _case("mx k3", 2, 257, 64, 128, 3, lens=(257, 129), precs=(5, 6), covers=E + ("lo_drop", "cross_drop", "mx_scale", "mx_tap_swap", "rows_127_128"),
              claims=dict(interior=True, masked=True), tiles=(0,) + WS_ALL + FOUR + SPLITS + (WS64,)),
        _case("mx k7 d3 leaky cin96", 2, 200, 96, 130, 7, dil=3, lens=(200, 77), pre="LEAKY", affine=True, res=True, accumulate=True, out_scale=0.5, precs=(5, 6),
              covers=E + ("lo_drop", "cross_drop", "mx_scale", "mx_tap_swap", "rows_127_128"), tiles=(0,) + WS_ALL + FOUR),
        _case("mx k11", 1, 129, 64, 200, 11, precs=(5, 6), covers=E + ("lo_drop", "mx_scale", "mx_tap_swap"), tiles=(WS, 80000000 + WS, 128128)),
        _case("mx k5 fallback", 1, 130, 64, 128, 5, precs=(5, 6), covers=E + ("lo_drop",), tiles=(0, 64128, 2064128)),
        # quantising prologues whose quantised values are exact: extrema {127, 128} give scale 1 and zero point 127
        _case("fq none", 2, 258, 64, 128, 3, lens=(258, 131), fq=True, precs=(2,), covers=E + ("rows_127_128",), tiles=(WS, 80000000 + WS, WS64, 128128, 64064, 2064128)),
        _case("fq leaky", 2, 258, 64, 128, 3, lens=(258, 131), fq=True, pre="LEAKY", pre_slope=0.5, precs=(2,), covers=E + ("rows_127_128",), tiles=(WS, WS64, 64128)),
        _case("fq snake", 2, 258, 64, 128, 3, lens=(258, 131), fq=True, pre="SNAKE", precs=(2,), covers=E + ("rows_127_128",), tiles=(WS, WS64, 64128)),
    ]
    return out


GLOG_P = (127, 128, 129, 255, 256, 511, 512, 520)


def glog_cases():
    """P = B x ceil(L / 128) at the glog boundaries: items of at most 5 rows (ragged, some empty), C_in 64, K 3, one and two column tiles."""
    out = []
    for i, P in enumerate(GLOG_P):
        for cout in (128, 130):
            lens = [(5, 0, 1, 3, 4, 2, 5)[(j + i) % 7] for j in range(P)]
            lens[0], lens[-1] = 5, 4        # the first and the last row tile are live
            out.append(_case(f"glog P{P} cout{cout}", P, 5, 64, cout, 3, lens=lens, precs=(2, 4) if cout == 128 else (1, 3), covers=("halo_clamp", "last_tap_drop"),
                             claims=dict(glog=(0, 1, 1, 1, 2, 2, 3, 3)[i], NT=1 if cout == 128 else 2), tiles=(0, WS, 80000000 + WS)))
        # ... and the 64-column tile (C_out <= 64) at every boundary: glog 2 and 3 on bn = 64 have no other small case
        out.append(_case(f"glog P{P} cout50", P, 5, 64, 50, 3, lens=lens, precs=(2, 3), covers=("halo_clamp", "last_tap_drop"),
                         claims=dict(glog=(0, 1, 1, 1, 2, 2, 3, 3)[i], NT=1), tiles=(0, WS64, 80000000 + WS64)))
    return out


def walk_cases():
    """9 .. 40 tiles under mi355_conv_ws4_resident(8) / (16): every workgroup walks several tiles; middle items empty or one row long make next_work skip
    ids on the producer and on the consumer side."""
    return [
        _case("walk 9 tiles", 3, 384, 64, 128, 3, covers=("halo_clamp",), precs=(1, 2, 3, 4), tiles=(WS, WS64)),
        _case("walk ragged 20 ids", 10, 200, 64, 130, 7, dil=3, lens=(200, 0, 1, 129, 0, 0, 128, 1, 200, 64), pre="LEAKY", affine=True, res=True, covers=("halo_clamp",),
              precs=(1, 2, 3, 4), tiles=(WS, WS64)),
        _case("walk gemm 40 ids", 5, 500, 96, 200, 1, lens=(500, 1, 0, 257, 384), covers=("last_tap_drop",), precs=(1, 2, 3, 4), tiles=(WS, WS64)),
        _case("walk mx 24 ids", 4, 300, 64, 200, 3, lens=(300, 0, 1, 257), precs=(5, 6), covers=("halo_clamp",), tiles=(WS,)),
    ]


def stats_cases():
    """Fused instance-norm statistics (stats_partial) on integer outputs: ragged items with a partly filled last block; only the 128-row kernels carry them."""
    return [
        _case("stats c128", 3, 200, 128, 128, 3, lens=(200, 65, 129), res=True, out_scale=0.5, covers=("halo_clamp",), tiles=(0, WS, 80000000 + WS, 128128, 2064128), stats=True),
        _case("stats c64", 2, 130, 64, 64, 7, dil=3, lens=(130, 64), pre="LEAKY", affine=True, covers=("halo_clamp",), tiles=(0, WS64, 80000000 + WS64, WS, 64064), stats=True),
    ]


def float_cases():
    """The branches that cannot be made exact: transcendental prologues and epilogues (float inputs, per-element bound)."""
    f = dict(exact=False)
    return [
        _case("snake k7 d3", 2, 200, 96, 130, 7, dil=3, lens=(200, 131), pre="SNAKE", affine=True, res=True, out_scale=0.5, tiles=(0, WS, 80000000 + WS, 20000000 + WS, WS64, 64128, 2064128),
              covers=("halo_clamp", "last_tap_drop", "rows_127_128"), **f),
        _case("snake thin", 2, 140, 64, 50, 3, lens=(140, 64), pre="SNAKE", tiles=(WS64, 80000000 + WS64, WS, 64064), covers=("halo_clamp", "rows_127_128"), **f),
        _case("snakebeta", 1, 257, 64, 128, 3, pre="SNAKEBETA", precs=(2, 4), tiles=(WS, 80000000 + WS, 128128), covers=("halo_clamp", "rows_127_128"), **f),
        _case("elu", 2, 140, 64, 128, 7, lens=(140, 3), pre="ELU", tiles=(0, WS, WS64, 64128), covers=("halo_clamp", "rows_127_128"), **f),     # precisions 1 / 3: no ws4 instantiation
        _case("elu thin", 1, 130, 32, 40, 3, pre="ELU", precs=(2, 4), tiles=(WS64, 64064), covers=("halo_clamp",), **f),
        _case("conv gelu", 1, 130, 64, 128, 3, post="gelu", precs=(2, 3, 4), tiles=(WS, 80000000 + WS, 64128), covers=("halo_clamp", "rows_127_128"), **f),
        _case("gemm gelu", 2, 130, 96, 200, 1, lens=(130, 7), post="gelu", tiles=(WS, 80000000 + WS, 64128, 2064128), covers=("last_tap_drop",), **f),
        _case("gemm silu", 1, 129, 160, 128, 1, post="silu", colscale=True, res=True, precs=(2, 4), tiles=(WS, 128128), covers=("last_tap_drop",), **f),
        _case("gemm gelu_tanh", 1, 129, 64, 130, 1, post="gelu_tanh", precs=(2, 4), tiles=(WS, 64064), covers=("last_tap_drop",), **f),
        _case("mx snake", 2, 200, 64, 128, 7, dil=3, lens=(200, 131), pre="SNAKE", affine=True, precs=(5, 6), tiles=(WS, 20000000 + WS, 80000000 + WS, 0), covers=("halo_clamp", "rows_127_128"), **f),
    ]


def all_cases():
    return exact_cases() + glog_cases() + walk_cases() + stats_cases() + float_cases()


def case_id(c):
    return c["name"].replace(" ", "_")


def _gen(c, salt=""):
    return torch.Generator().manual_seed(zlib.crc32((c["name"] + salt).encode()))


_INPUT_CACHE = {}


def inputs(c, fl):
    """CPU tensors of one case in flavour ``fl`` ('n', 'w', 'm'; float cases: 'f'): x [B, L, Cin] float32, w [Cout, K, Cin], bias, colscale, res, old, sc, sh,
    alpha, inv_beta (None where the case has none).  Cached and never modified."""
    key = (c["name"], fl)
    if key in _INPUT_CACHE:
        return _INPUT_CACHE[key]
    g = _gen(c)
    B, L, Cin, Cout, K = c["B"], c["L"], c["Cin"], c["Cout"], c["K"]
    d = dict(alpha=None, inv_beta=None, sc=None, sh=None)
    ri = lambda lo, hi, shape: torch.randint(lo, hi + 1, shape, generator=g).double()
    if c["exact"]:
        w = torch.tensor([0, 1, -1, 2, -2, 3, -3, 4, -4, 6, -6], dtype=torch.float64)[torch.randint(0, 11, (Cout, K, Cin), generator=g)]
        w[:, 0, 0] = torch.tensor([4.0, -6.0, 6.0, -4.0])[torch.arange(Cout) % 4]
        if Cout >= 3:
            w[1] = 0.0
        if c["fq"]:
            t = ri(-127, 128, (B, L, Cin))
            t[:, 0, 0], t[:, 0, 1] = -127.0, 128.0
        else:
            t = ri(-4, 4, (B, L, Cin))
            if fl in ("w", "m"):
                dens = min(1.0 / 97, 5.0 / (K * Cin))
                wide = torch.rand((B, L, Cin), generator=g) < dens
                for b, n in enumerate(c["lens"]):          # forced: an item's first and last row, the rows at the tile seam, the last channel
                    for r, ch in ((0, 0), (n - 1, Cin - 1), (127, Cin // 2), (128, 1), (n // 2, Cin - 1)):
                        if 0 <= r < n:
                            wide[b, r, ch] = True
                sign = torch.where(torch.rand((B, L, Cin), generator=g) < 0.5, -1.0, 1.0).double()
                if fl == "w":
                    val = 2049.0 + 2.0 * ri(0, 1023, (B, L, Cin))
                else:
                    r3 = ri(1, 3, (B, L, Cin)) * torch.where(torch.rand((B, L, Cin), generator=g) < 0.5, -1.0, 1.0).double()
                    val = 8192.0 + 8.0 * ri(0, 1023, (B, L, Cin)) + r3
                t = torch.where(wide, sign * val, t)
        pre_inv = t
        if c["pre"] == "LEAKY":           # negative prologue inputs are multiples of 1 / slope
            pre_inv = torch.where(t < 0, t / c["pre_slope"], t)
        elif c["pre"] == "SNAKE":         # fq snake: a palette whose Snake values lie far from every rounding step (asserted on the CPU)
            d["alpha"] = torch.full((round_up(Cin, 32),), 0.75)
            pre_inv = SNAKE_PALETTE[torch.randint(0, len(SNAKE_PALETTE), (B, L, Cin), generator=g)]
        if c["affine"]:
            sc = torch.tensor([1.0, -1.0, 2.0, -2.0], dtype=torch.float64)[torch.randint(0, 4, (B, round_up(Cin, 32)), generator=g)]
            sh = ri(-8, 8, (B, round_up(Cin, 32)))
            pre_inv = (pre_inv - sh[:, None, :Cin]) / sc[:, None, :Cin]
            d.update(sc=sc.float(), sh=sh.float())
        x = pre_inv.float()
        assert torch.equal(x.double(), pre_inv)
        bias = ri(-8, 8, (Cout,)) if c["bias"] else None
        cs = torch.tensor([1.0, 2.0, -1.0])[torch.randint(0, 3, (Cout,), generator=g)] if c["colscale"] else None
        res = ri(-8, 8, (B, L, Cout)) if c["res"] else None
        old = ri(-8, 8, (B, L, Cout)) if c["accumulate"] else None
    else:
        w = (torch.randn((Cout, K, Cin), generator=g) / math.sqrt(K * Cin)).to(torch.bfloat16).double()
        x = torch.randn((B, L, Cin), generator=g)
        if fl == "m":
            x = x * (1.0 + 3.0 * torch.randn((B, L, Cin), generator=g) ** 2)
        if c["affine"]:
            d.update(sc=torch.rand((B, round_up(Cin, 32)), generator=g) + 0.5, sh=torch.randn((B, round_up(Cin, 32)), generator=g) * 0.3)
        if c["pre"] in ("SNAKE", "SNAKEBETA"):
            d["alpha"] = torch.rand((round_up(Cin, 32),), generator=g) + 0.5
        if c["pre"] == "SNAKEBETA":
            d["inv_beta"] = torch.rand((round_up(Cin, 32),), generator=g) + 0.5
        bias = torch.randn((Cout,), generator=g) * 0.1 if c["bias"] else None
        cs = torch.rand((Cout,), generator=g) + 0.5 if c["colscale"] else None
        res = torch.randn((B, L, Cout), generator=g) if c["res"] else None
        old = torch.randn((B, L, Cout), generator=g) if c["accumulate"] else None
    if d["alpha"] is not None:
        d["alpha_c"] = d["alpha"]
        d["alpha"] = d["alpha"][:Cin]
    if d["inv_beta"] is not None:
        d["inv_beta_c"] = d["inv_beta"]
        d["inv_beta"] = d["inv_beta"][:Cin]
    if d["sc"] is not None:
        d["sc_c"], d["sh_c"] = d["sc"], d["sh"]
        d["sc"], d["sh"] = d["sc"][:, :Cin], d["sh"][:, :Cin]
    f32 = lambda v: None if v is None else v.float()
    d.update(x=x.float(), w=w, bias=f32(bias), colscale=f32(cs), res=f32(res), old=f32(old))
    _INPUT_CACHE[key] = d
    return d


def round_up(x, m):
    return (x + m - 1) // m * m


def _snake_palette():
    v = torch.arange(-40, 41, dtype=torch.float64) * 0.375
    s = v + (1.0 / 0.75) * torch.sin(0.75 * v) ** 2
    keep = ((s - torch.floor(s) - 0.5).abs() > 0.05) & (s > -126) & (s < 127)
    return v[keep]


SNAKE_PALETTE = _snake_palette()      # prologue inputs whose Snake(alpha = 0.75) value is >= 0.05 from every half-integer: the uint8 rounding cannot flip


def flavours(c):
    return sorted({flavour(p) for p in c["precs"]}) if c["exact"] else (["m"] if set(c["precs"]) <= {5, 6} else ["f"])


def case_flavour(c, prec):
    return flavour(prec) if c["exact"] else ("m" if prec in (5, 6) else "f")


def expected(c, prec):
    """What the kernel must produce at ``prec``: the float64 statement (exact cases and float cases of precisions 1 .. 4) or mx_ref's (float cases of 5 / 6)."""
    key = (c["name"], "want", case_flavour(c, prec), prec if (not c["exact"] and prec in (5, 6)) else 0)
    if key not in _INPUT_CACHE:
        inp = inputs(c, case_flavour(c, prec))
        _INPUT_CACHE[key] = mx_statement(c, inp, prec) if key[3] else statement(c, inp)
    return _INPUT_CACHE[key]


def budget(c, fl):
    """(largest sum |t| |w| plus epilogue operands, quantum): the exact cases need budget / quantum < 2^24."""
    inp = inputs(c, fl)
    s = max([float(v.max()) for v in statement(c, inp, absolute=True) if v.numel()] + [0.0])
    s = (s + 8.0) * (2.0 if c["colscale"] else 1.0) + 16.0
    q = min(1.0, c["out_scale"]) * (c["post_slope"] if c["post"] == "leaky" else 1.0)
    return s, q


def prologue_delta(x, c, inp, b):
    """Per element, how far the kernel's float32 prologue value may lie from the float64 one: four times the statement's own float32 error, one ulp of the
    value, and for Snake / SnakeBeta the hardware sine (v_sin_f32 on revolutions: 1e-6 absolute plus the rounding of its argument, through d sin^2 <= 2)."""
    t64, t32 = prologue(x, c, inp, b), prologue(x, c, inp, b, torch.float32).double()
    d = 4.0 * (t32 - t64).abs() + ulp32(t64)
    if c["pre"] in ("SNAKE", "SNAKEBETA"):
        u = x.double()
        if c["affine"]:
            u = u * inp["sc"][b].double() + inp["sh"][b].double()
        al = inp["alpha"].double()
        amp = inp["inv_beta"].double() if c["pre"] == "SNAKEBETA" else 1.0 / al
        d = d + 2.0 * amp * (1e-6 + 2.0 ** -23 * (al * u).abs())
    return d


def mx_prologue_term(c, inp, prec, b):
    """The first-order effect of the prologue's float32 error on the MX image, per output element of item ``b``: the image hi + q(lo) of mx_ref is a step
    function of t (an e4m3 / e2m1 rounding of the residual flips, a block's scale moves with its maximum), so t -> t +- delta changes an element by up
    to a whole grid step.  D = the larger change of the image under t + delta and t - delta (at least delta itself); the term is sum D |w|."""
    from oracle import mx_ref

    n = c["lens"][b]
    if n == 0:
        return torch.zeros((0, c["Cout"]), dtype=torch.float64)
    x = inp["x"][b, :n]
    t, d = prologue(x, c, inp, b), prologue_delta(x, c, inp, b)
    cp = round_up(c["Cin"], 32)
    split = mx_ref.split_activation if prec == 5 else mx_ref.split_activation4

    def image(v):
        tp = np.zeros((n, cp), dtype=np.float32)
        tp[:, :c["Cin"]] = v.float().numpy()
        hi, lo = split(tp)
        return torch.from_numpy((hi + lo)[:, :c["Cin"]])

    base = image(t)
    D = torch.maximum(torch.maximum((image(t + d) - base).abs(), (image(t - d) - base).abs()), d)
    return conv_rows(D, inp["w"].abs(), c["dil"], c["pad"], c["lens_out"][b])


def float_bound(c, prec):
    """Per item: (bound [len_out, Cout], e32, peak) of a float case at ``prec`` (precisions 5 / 6, against mx_ref: the same flat term plus ``mx_prologue_term``)."""
    key = (c["name"], "bound", prec)
    if key in _INPUT_CACHE:
        return _INPUT_CACHE[key]
    inp = inputs(c, case_flavour(c, prec))
    want = expected(c, prec)
    w32 = statement(c, inp, dt=torch.float32)
    w64 = statement(c, inp)
    live = [i for i in range(c["B"]) if want[i].numel()]
    e32 = max(float((w32[i].double() - w64[i]).abs().max()) for i in live)
    peak = max(float(want[i].abs().max()) for i in live)
    flat = 4.0 * e32 + 1e-6 * peak
    absw = statement(c, inp, absolute=True)
    out = []
    for i in range(c["B"]):
        if prec in (5, 6):
            out.append(flat + mx_prologue_term(c, inp, prec, i) * abs(c["out_scale"]))
            continue
        # d epilogue / d accumulator: the activations here have slope <= 1.13 (GELU), the column scale and out_scale multiply it
        gain = 1.13 * (float(inp["colscale"].abs().max()) if inp["colscale"] is not None else 1.0) * abs(c["out_scale"])
        out.append(flat + G_FORMAT[prec] * absw[i] * gain)
    _INPUT_CACHE[key] = (out, e32, peak)
    return _INPUT_CACHE[key]


def in_suite(prec, tile):
    """False for the tile codes that select an ablation or timeline-probe build (wrong by design): a hundred-millions digit, feature bit 2 at precision 2,
    any feature bit the precision-5 / 6 lists do not carry (mi355_conv_ws4_route: everything outside 0, 1, 3 at precision 5 and outside 0, 3 at precision 6)."""
    code, digit = tile % 10000000, tile // 10000000
    if code != 6128128:
        return True
    return digit < 10 and not (digit & 4) and not (prec == 6 and digit & 2)


def float_bound_p4_of_mx(c):
    """The bound of an MX float case on a launch that falls back to the precision-4 arithmetic (against the float64 statement on the same inputs)."""
    key = (c["name"], "bound", "mx->p4")
    if key not in _INPUT_CACHE:
        inp = inputs(c, "m")
        w64, w32, absw = statement(c, inp), statement(c, inp, dt=torch.float32), statement(c, inp, absolute=True)
        live = [i for i in range(c["B"]) if w64[i].numel()]
        e32 = max(float((w32[i].double() - w64[i]).abs().max()) for i in live)
        peak = max(float(w64[i].abs().max()) for i in live)
        _INPUT_CACHE[key] = [4.0 * e32 + 1e-6 * peak + G_FORMAT[4] * 1.13 * abs(c["out_scale"]) * a for a in absw]
    return _INPUT_CACHE[key]


def tile_calls(c, prec):
    """[(tile, label, facts)] of every tile code the case runs at ``prec`` and the dispatcher accepts."""
    out = []
    for tile in (c["tiles"] or EVERY):
        if not in_suite(prec, tile):
            continue
        lab, facts = route(case_launch(c, prec, tile))
        if not lab.startswith("refuse:"):
            out.append((tile, lab, facts))
    return out


def case_launch(c, prec, tile, resident=0, only=None):
    B = c["B"] if only is None else 1
    lens = c["lens"] if only is None else [c["lens"][only]]
    lens_out = c["lens_out"] if only is None else [c["lens_out"][only]]
    y_al = (round_up(c["Cout"], 4) + c["y_extra"]) % 4 == 0
    ld = round_up(int(c["unaligned"]) + c["x_off"] + c["Cin"], 4) + c["x_extra"]      # the input buffer of tests/test_conv_kernel_edges_gpu.py
    vec = not c["unaligned"] and ld % 4 == 0 and c["x_off"] % 4 == 0 and (c["L"] * ld) % 4 == 0
    return launch(B=B, L=c["L"], Lout=c["Lout"], Cin=c["Cin"], Cout=c["Cout"], K=c["K"], dil=c["dil"], pad=c["pad"], precision=prec, tile=tile, pre=c["pre"], affine=c["affine"],
                  fq=c["fq"], post=c["post"], res=c["res"], res_shift=c["res_shift"], accumulate=c["accumulate"], colscale=c["colscale"], vec=vec,
                  lens_in=lens, lens_out=lens_out, out_aligned=y_al, resident=resident, stats=c["stats"])
