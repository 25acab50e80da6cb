"""Thin torch-tensor front end of the C ABI (include/mi355audio.h).

PyTorch is plumbing only: it owns device memory (caching allocator) and streams; every compute op
below is a hand-written gfx950 kernel reached through ctypes.  All activations are float32,
channels-last ``[B, L, C]`` views whose last stride is 1 (slices of wider buffers are fine: that is
how channel concatenation is fused away).
"""
from __future__ import annotations

import ctypes
import math
import os
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib

ACT_NONE, ACT_LEAKY, ACT_SNAKE, ACT_GELU, ACT_ELU, ACT_SILU, ACT_GELU_TANH, ACT_TANH = 0, 1, 2, 3, 4, 5, 6, 7

# bench.py's roofline leg: when a list is installed here every conv_gemm launch is bracketed by
# events on the launch stream and (algorithmic flops, algorithmic bytes, start, end) is appended.
PROFILE = None


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def profile_finalize(entries):
    """PROFILE entries -> [(algorithmic flops, algorithmic bytes, start event, end event, (cin, cout, k, dil, rows))] after a synchronize.

    Algorithmic bytes of one launch = every operand once: fp32 input rows, fp32 output rows, the 16-bit weight image, plus one more fp32
    output-shaped read per residual operand and per ``accumulate`` (the launch must read what it adds to) -- the figure the PMC traffic is
    compared with."""
    torch.cuda.synchronize()
    out = []
    for rows, cin, cout, k, dil, extra_reads, e0, e1 in entries:
        rows = int(rows)
        flops = 2.0 * rows * cout * k * cin
        byts = 4.0 * rows * (cin + cout * (1 + extra_reads)) + 2.0 * cout * k * cin
        out.append((flops, byts, e0, e1, (cin, cout, k, dil, rows)))
    return out


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _nlc(t: torch.Tensor) -> Tuple[int, int, int, int, int]:
    """(B, L, C, bstride, ld) of a channels-last view."""
    assert t.dim() == 3 and t.stride(2) == 1 and t.dtype == torch.float32 and t.is_cuda, (t.shape, t.stride(), t.dtype)
    return t.shape[0], t.shape[1], t.shape[2], t.stride(0), t.stride(1)


def require_gpu():
    if not torch.cuda.is_available():
        raise _lib.Mi355Error("mlx_audio_amd needs a ROCm device (MI355X / gfx950); there is no CPU fallback")
    _lib.load()


def round_up(x: int, m: int) -> int:
    return (x + m - 1) // m * m


# --------------------------------------------------------------------------------------- weights
@dataclass
class PackedConv:
    """bf16 weights of one conv / linear in MFMA fragment order plus its fp32 bias (device)."""

    w: torch.Tensor  # int16 view of the packed bf16 data, on device
    bias: Optional[torch.Tensor]
    cout: int
    k: int
    cin: int
    f16: bool = False  # packed as fp16 for the single-pass fp16 MFMA mode (precision 3)
    mx: int = 0        # 1: MX image: fp16 tap slices + e4m3 tap-pair slices + E8M0 column scales (precision 5); 2: MX4 image, FP4 (e2m1) tap-pair slices (precision 6)


def mx_eligible(cout: int, k: int, cin: int) -> bool:
    """Shapes the wave-specialised kernel takes at precision 5 (``mi355_conv_ws4_eligible``): K = 3 (mod 4), more than 64 outputs, >= 64 inputs."""
    return k % 4 == 3 and cout > 64 and cin >= 64


def mx_pays(cout: int, k: int, cin: int) -> bool:
    """... and for which it is the faster arithmetic (profiles/r4_conv_prec_ab_b32_call3.txt): from 7 taps on.  The 3-tap convs are bound by HBM and
    by the producers' VALU work, where the bf16 split is the cheapest prologue (cvt_pk + shift / mask): they stay on the bf16 hi + lo pass."""
    return mx_eligible(cout, k, cin) and k >= 7


def pack_conv(w: torch.Tensor, bias: Optional[torch.Tensor], device, f16: bool = False, mx=False) -> PackedConv:
    """``w``: float32 CPU tensor ``[Cout, K, Cin]`` (MLX conv layout) or ``[Cout, Cin]`` (linear).  ``mx``: True / 1 = the image of precision 5 (e4m3 lo
    slices), 2 = the MX4 image of precision 6 (FP4 lo slices)."""
    if w.dim() == 2:
        w = w[:, None, :]
    w = w.detach().to(torch.float32).contiguous().cpu()
    cout, k, cin = w.shape
    lib = _lib.load()
    if mx:
        nb = lib.mi355_packed_conv_weight_mx_bytes(cout, k, cin)
        out8 = np.empty(nb, dtype=np.uint8)
        fn = "mi355_pack_conv_weight_mx4_host" if int(mx) == 2 else "mi355_pack_conv_weight_mx_host"
        rc = getattr(lib, fn)(w.numpy().ctypes.data, cout, k, cin, out8.ctypes.data)
        _lib.check(rc, fn)
        wd = torch.from_numpy(out8).to(device)
        bd = None if bias is None else bias.detach().to(torch.float32).contiguous().to(device)
        return PackedConv(wd, bd, cout, k, cin, True, 2 if int(mx) == 2 else 1)
    n = lib.mi355_packed_conv_weight_elems(cout, k, cin)
    out = np.empty(n, dtype=np.uint16)
    rc = lib.mi355_pack_conv_weight_host_dt(w.numpy().ctypes.data, cout, k, cin, 1 if f16 else 0, out.ctypes.data)
    _lib.check(rc, "mi355_pack_conv_weight_host_dt")
    wd = torch.from_numpy(out.view(np.int16)).to(device)
    bd = None if bias is None else bias.detach().to(torch.float32).contiguous().to(device)
    return PackedConv(wd, bd, cout, k, cin, f16)


def pack_conv_transpose(w_t: torch.Tensor, bias: Optional[torch.Tensor], stride: int, device, f16: bool = False) -> PackedConv:
    """Polyphase repack of a transposed conv.  ``w_t``: ``[Cout, K, Cin]`` as ``mx.conv_transpose1d``
    takes it (out[n] += x[t] * w_t[:, k, :] for n = t*stride + k - pad); K must be a multiple of
    stride.  Returns the equivalent stride-1 conv with K/stride taps and ``stride*Cout`` outputs:
    GEMM row u, column r*Cout+co  ->  out[u*stride + r - pad, co]."""
    return pack_conv(_polyphase_weight(w_t.to(torch.float32), stride), bias, device, f16)


def _polyphase_weight(w_t: torch.Tensor, stride: int) -> torch.Tensor:
    """[Cout, K, Cin] transposed-conv weight -> [stride*Cout, K/stride, Cin] stride-1 conv weight (host logic)."""
    cout, k, cin = w_t.shape
    assert k % stride == 0, "polyphase conv_transpose needs K % stride == 0"
    kp = k // stride
    w = torch.empty((stride * cout, kp, cin), dtype=w_t.dtype)
    for r in range(stride):
        for tp in range(kp):
            w[r * cout:(r + 1) * cout, tp, :] = w_t[:, r + (kp - 1 - tp) * stride, :]
    return w


@dataclass
class RowMajor16:
    """Row-major 16-bit weight image [N, K] for the decode-step GEMV (checkpoint dtype: bf16 or fp16)."""

    w: torch.Tensor  # int16 [N, K] on device (uint8 [N, K] for the fp8 image)
    bias: Optional[torch.Tensor]
    n: int
    k: int
    f16: bool
    scale: Optional[torch.Tensor] = None  # fp8 image only: per-row power-of-two dequantisation scale [N] fp32 (device)
    interleaved: bool = False             # recurrent weights of mi355_lstm_seq with their rows ordered by hidden unit (row 4 j + gate): the one-launch step

    @property
    def wdtype(self) -> int:
        return W_FP8 if self.scale is not None else (W_F16 if self.f16 else W_BF16)


def pack_rowmajor16(w: torch.Tensor, bias: Optional[torch.Tensor], device, f16: bool = False) -> RowMajor16:
    """``w``: float32 CPU tensor [N, K] (nn.Linear weight layout)."""
    w = w.detach().to(torch.float32).contiguous().cpu()
    n, k = w.shape
    assert k % 8 == 0, "gemv needs K % 8 == 0"
    lib = _lib.load()
    out = np.empty(n * k, dtype=np.uint16)
    rc = lib.mi355_pack_rowmajor16_host(w.numpy().ctypes.data, n * k, 1 if f16 else 0, out.ctypes.data)
    _lib.check(rc, "mi355_pack_rowmajor16_host")
    wd = torch.from_numpy(out.view(np.int16).reshape(n, k)).to(device)
    bd = None if bias is None else bias.detach().to(torch.float32).contiguous().to(device)
    return RowMajor16(wd, bd, n, k, f16)


W_BF16, W_F16, W_FP8 = 0, 1, 2  # MI355_W_* of the header


def quantize_rows_fp8(w: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """float32 [N, K] (CPU) -> (uint8 [N, K] OCP e4m3fn codes, float32 [N] power-of-two row scales) through the library's host packer
    (``mi355_pack_rowmajor_fp8_host``): w ~= decode(code) * scale, and decode(code) * scale is exactly representable in bf16."""
    w = w.detach().to(torch.float32).contiguous().cpu()
    n, k = w.shape
    assert k % 16 == 0, "fp8 GEMV images need K % 16 == 0"
    lib = _lib.load()
    codes = np.empty((n, k), dtype=np.uint8)
    scale = np.empty(n, dtype=np.float32)
    rc = lib.mi355_pack_rowmajor_fp8_host(w.numpy().ctypes.data, n, k, codes.ctypes.data, scale.ctypes.data)
    _lib.check(rc, "mi355_pack_rowmajor_fp8_host")
    return torch.from_numpy(codes), torch.from_numpy(scale)


def dequantize_rows_fp8(codes: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """The float32 weights an fp8 image stands for (exact): used to build the bf16 MFMA image of the SAME quantised Linear for prefill."""
    return codes.view(torch.float8_e4m3fn).to(torch.float32) * scale[:, None]


def pack_rowmajor_fp8(w: torch.Tensor, bias: Optional[torch.Tensor], device) -> Tuple[RowMajor16, torch.Tensor]:
    """fp8 GEMV image of an nn.Linear weight [N, K]; also returns the dequantised float32 weights (CPU) it represents."""
    codes, scale = quantize_rows_fp8(w)
    bd = None if bias is None else bias.detach().to(torch.float32).contiguous().to(device)
    rw = RowMajor16(codes.to(device), bd, codes.shape[0], codes.shape[1], False, scale.to(device))
    return rw, dequantize_rows_fp8(codes, scale)


def gemv(x: torch.Tensor, rw: RowMajor16, y: torch.Tensor, *, post_act: int = ACT_NONE, post_slope: float = 0.0,
         res: Optional[torch.Tensor] = None, colscale: Optional[torch.Tensor] = None, out_scale: float = 1.0, glu: bool = False,
         use_bias: bool = True, norm: Optional[tuple] = None, y2: Optional[torch.Tensor] = None, rope: Optional[tuple] = None,
         x_ids: Optional[torch.Tensor] = None, x_id_offset: int = 0, w_policy: int = 0):
    """y[m, :] = epilogue(norm(x[m, :]) @ W^T) for 1..8 rows (any weight image) or 9..64 rows (16-bit images, K % 64 == 0); x / y / res are 2-D fp32 views with unit inner stride.
    ``norm`` = (mode, weight, bias, eps) with mode "layer" | "rms" fuses the input normalisation; ``y2``: columns >= y.shape[1] go there."""
    assert x.dim() == 2 and y.dim() == 2 and x.stride(1) == 1 and y.stride(1) == 1 and x.dtype == torch.float32 and y.dtype == torch.float32
    M = x.shape[0] if x_ids is None else 1   # x_ids int32 [1] (device): x is then a TABLE and the input row is x[x_ids[0] + x_id_offset]
    n_y = rw.n // 2 if glu else (rw.n if y2 is None else rw.n - y2.shape[1])
    assert x.shape[1] == rw.k and y.shape[0] == M and y.shape[1] == n_y, (x.shape, y.shape, rw.n, rw.k)
    kw = dict(x=_ptr(x), ldx=x.stride(0), M=M, K=rw.k, w=_ptr(rw.w), ldw=rw.w.stride(0), wdtype=rw.wdtype, wscale=_ptr(rw.scale), N=rw.n,
              bias=_ptr(rw.bias) if use_bias else None, post_act=post_act, post_slope=post_slope, colscale=_ptr(colscale),
              out_scale=out_scale, glu=int(glu), y=_ptr(y), ldy=y.stride(0), w_policy=int(w_policy))
    if res is not None:
        assert res.dim() == 2 and res.stride(1) == 1
        kw.update(res=_ptr(res), ldr=res.stride(0))
    if norm is not None:
        mode, nw, nb, eps = norm
        kw.update(norm={"layer": 1, "rms": 2}[mode], norm_weight=_ptr(nw), norm_bias=_ptr(nb), norm_eps=eps)
    if y2 is not None:
        assert y2.dim() == 2 and y2.stride(1) == 1 and y2.shape[0] == M and y2.dtype in KV_DTYPES
        kw.update(y2=_ptr(y2), ldy2=y2.stride(0), split=n_y, y2_dtype=KV_DTYPES[y2.dtype])
    if x_ids is not None:
        assert x_ids.dtype == torch.int32 and x_ids.numel() == 1 and x_ids.is_cuda
        kw.update(x_ids=_ptr(x_ids), x_id_offset=int(x_id_offset))
    if rope is not None:  # (cos_row [dh / 2], sin_row [dh / 2], dh, cols): interleaved rotary pairs on the first ``cols`` output columns
        cos_row, sin_row, dh, cols = rope
        assert cos_row.is_contiguous() and sin_row.is_contiguous() and cos_row.numel() >= dh // 2
        kw.update(rope_cos=_ptr(cos_row), rope_sin=_ptr(sin_row), rope_dh=dh, rope_cols=cols)
    _lib.call_struct("mi355_gemv", "mi355_gemv_args", _stream(), **kw)
    return y


# --------------------------------------------------------------------------------------- decode steps for 9..64 sequences (rows_pipe.hip)
@dataclass
class Tiles16:
    """Tile image of a [N, K] Linear for ``mi355_rows_gemm``: [ceil(N / 16)][K / 64][4 groups][16 rows][16 elements] 16-bit elements."""

    w: torch.Tensor  # int16 (fp8 image: uint8), flat, on the device
    n: int
    k: int
    f16: bool
    scale: Optional[torch.Tensor] = None  # fp8 image only: per-row power-of-two dequantisation scale [N] fp32 (device)

    @property
    def wdtype(self) -> int:
        return W_FP8 if self.scale is not None else (W_F16 if self.f16 else W_BF16)


def tiles16_from_rowmajor(rm: RowMajor16) -> Tiles16:
    """The tile image of a row-major 16-bit image, permuted on the device (== ``mi355_pack_tiles16_host`` of the same weights, element for element)."""
    assert rm.k % 64 == 0, "tile images need K % 64 == 0"   # an fp8 image (uint8 codes + per-row scales) is permuted the same way, one byte per element
    nt = (rm.n + 15) // 16
    w = rm.w[:, : rm.k]
    if nt * 16 != rm.n:
        w = torch.cat([w, torch.zeros((nt * 16 - rm.n, rm.k), dtype=w.dtype, device=w.device)], 0)
    t = w.reshape(nt, 16, rm.k // 64, 4, 16).permute(0, 2, 3, 1, 4).contiguous().reshape(-1)
    return Tiles16(t, rm.n, rm.k, rm.f16, rm.scale)


def pack_tiles8_host(codes: torch.Tensor) -> np.ndarray:
    """``mi355_pack_tiles8_host`` on uint8 e4m3 codes [N, K] (CPU): uint8 [ceil(N / 16) * 16 * K]."""
    c = codes.detach().to(torch.uint8).contiguous().cpu()
    n, k = c.shape
    out = np.empty(((n + 15) // 16) * 16 * k, dtype=np.uint8)
    rc = _lib.load().mi355_pack_tiles8_host(c.numpy().ctypes.data, n, k, out.ctypes.data)
    _lib.check(rc, "mi355_pack_tiles8_host")
    return out


def pack_tiles16_host(w: torch.Tensor, f16: bool = False) -> np.ndarray:
    """``mi355_pack_tiles16_host`` on float32 CPU weights [N, K]: uint16 [ceil(N / 16) * 16 * K]."""
    w = w.detach().to(torch.float32).contiguous().cpu()
    n, k = w.shape
    out = np.empty(((n + 15) // 16) * 16 * k, dtype=np.uint16)
    rc = _lib.load().mi355_pack_tiles16_host(w.numpy().ctypes.data, n, k, 1 if f16 else 0, out.ctypes.data)
    _lib.check(rc, "mi355_pack_tiles16_host")
    return out


def rows_R(M: int) -> int:
    """Rows of the planes that carry ``M`` sequences: 16, 32 or 64."""
    assert 1 <= M <= 64
    return 16 if M <= 16 else (32 if M <= 32 else 64)


def rows_kgroups(n: int, k: int) -> int:
    return int(_lib.load().mi355_rows_kgroups(n, k))


def rows_planes(R: int, k: int, device) -> torch.Tensor:
    """Storage of the planes of R rows x k columns (hi + lo images: 4 bytes per element)."""
    return torch.zeros(2 * R * k, dtype=torch.int16, device=device)


def rows_gemm(planes: torch.Tensor, tl: Tiles16, part: Optional[torch.Tensor], M: int, R: int, kgroups: Optional[int] = None, *,
              glu_planes_out: Optional[torch.Tensor] = None, glu_bias: Optional[torch.Tensor] = None):
    """part[g, :M, :N] = partial products of the g-th range of k steps; ``part`` is fp32 [kgroups, rows >= M, ld >= N] (contiguous slabs).
    ``glu_planes_out`` (one K group): silu(gate + b) * (up + b) of the (gate, up) column pairs leaves as planes instead."""
    kg = rows_kgroups(tl.n, tl.k) if kgroups is None else kgroups
    if glu_planes_out is not None:
        assert kg == 1 and glu_planes_out.numel() * glu_planes_out.element_size() >= 4 * R * (tl.n // 2)
        _lib.call_struct("mi355_rows_gemm", "mi355_rows_gemm_args", _stream(), wt=_ptr(tl.w), wdtype=tl.wdtype, N=tl.n, K=tl.k, planes=_ptr(planes), M=M, R=R,
                         kgroups=1, glu_planes_out=_ptr(glu_planes_out), glu_bias=_ptr(glu_bias), wscale=_ptr(tl.scale))
        return 1
    assert part.dtype == torch.float32 and part.dim() == 3 and part.shape[0] >= kg and part.shape[1] >= M and part.shape[2] >= tl.n and part.stride(2) == 1
    assert planes.numel() * planes.element_size() >= 4 * R * tl.k
    _lib.call_struct("mi355_rows_gemm", "mi355_rows_gemm_args", _stream(), wt=_ptr(tl.w), wdtype=tl.wdtype, N=tl.n, K=tl.k, planes=_ptr(planes), M=M, R=R,
                     part=_ptr(part), ldp=part.stride(1), kg_stride=part.stride(0), kgroups=kg)
    return kg


def rows_finish(part: torch.Tensor, M: int, N: int, kgroups: int = 1, *, bias=None, post_act: int = ACT_NONE, post_slope: float = 0.0, colscale=None,
                res: Optional[torch.Tensor] = None, out_scale: float = 1.0, glu: bool = False, wscale: Optional[torch.Tensor] = None,
                y: Optional[torch.Tensor] = None, y2: Optional[torch.Tensor] = None, norm: Optional[tuple] = None, yn: Optional[torch.Tensor] = None,
                planes: Optional[torch.Tensor] = None, R: int = 0, f16: bool = False):
    """Row epilogue of ``rows_gemm`` (see ``mi355_rows_finish_args``).  ``part``: fp32 [kgroups, rows, ld] slabs, or a 2-D fp32 matrix (kgroups = 1:
    the converter rows -> planes).  ``y`` / ``y2`` / ``yn`` are 2-D views with unit inner stride; ``norm`` = (mode, weight, bias, eps)."""
    if part.dim() == 2:
        part = part.unsqueeze(0)
    assert part.dtype == torch.float32 and part.stride(2) == 1 and part.shape[0] >= kgroups
    kw = dict(part=_ptr(part), kgroups=kgroups, kg_stride=part.stride(0) if kgroups > 1 else 0, ldp=part.stride(1), M=M, N=N, bias=_ptr(bias),
              post_act=post_act, post_slope=post_slope, colscale=_ptr(colscale), out_scale=out_scale, glu=int(glu), wscale=_ptr(wscale))
    n_out = N // 2 if glu else N
    if res is not None:
        assert res.dim() == 2 and res.stride(1) == 1
        kw.update(res=_ptr(res), ldr=res.stride(0))
    if y2 is not None:
        assert y is not None and y2.dim() == 2 and y2.stride(1) == 1 and y2.dtype in KV_DTYPES
        kw.update(y2=_ptr(y2), ldy2=y2.stride(0), split=n_out - y2.shape[1], y2_dtype=KV_DTYPES[y2.dtype])
    if y is not None:
        assert y.dim() == 2 and y.stride(1) == 1 and y.dtype == torch.float32
        kw.update(y=_ptr(y), ldy=y.stride(0))
    if norm is not None:
        mode, nw, nb, eps = norm
        kw.update(norm={"layer": 1, "rms": 2}[mode], norm_weight=_ptr(nw), norm_bias=_ptr(nb), norm_eps=eps)
    if yn is not None:
        assert yn.dim() == 2 and yn.stride(1) == 1 and yn.dtype == torch.float32
        kw.update(yn=_ptr(yn), ldyn=yn.stride(0))
    if planes is not None:
        assert R in (16, 32, 64) and planes.numel() * planes.element_size() >= 4 * R * n_out
        kw.update(planes=_ptr(planes), R=R, planes_dtype=W_F16 if f16 else W_BF16)
    _lib.call_struct("mi355_rows_finish", "mi355_rows_finish_args", _stream(), **kw)


def pack_lstm_wh(wh_f: torch.Tensor, wh_b: torch.Tensor, device, f16: bool = False) -> torch.Tensor:
    """Recurrent weights of both directions in the persistent kernel's layout; ``f16``: IEEE half instead of bf16 values (float32 checkpoints; pass
    ``wh_f16=True`` to ``lstm_bidir``)."""
    H = wh_f.shape[1]
    lib = _lib.load()
    out = np.empty(2 * 4 * H * H, dtype=np.uint16)
    a = wh_f.detach().to(torch.float32).contiguous().cpu().numpy()
    b = wh_b.detach().to(torch.float32).contiguous().cpu().numpy()
    rc = lib.mi355_pack_lstm_wh16_host(a.ctypes.data, b.ctypes.data, H, int(bool(f16)), out.ctypes.data)
    _lib.check(rc, "mi355_pack_lstm_wh16_host")
    return torch.from_numpy(out.view(np.int16)).to(device)


def pack_lstm_wh_scaled(wh_f: torch.Tensor, wh_b: torch.Tensor, device):
    """bf16-valued recurrent weights as an IEEE-half image scaled by a power of two into half's normal range: (image, wh_scale) for
    ``lstm_bidir(wh_f16=True, wh_scale=...)``, or ``None`` when some value would not be held exactly (then use the bf16 image).  Exact because a bf16
    value has 8 significant bits and half holds 11 in its normal range; the kernel's fp32 sums then equal the bf16 image's times 2^k, bit for bit."""
    w = torch.cat([wh_f.detach().to(torch.float32).reshape(-1), wh_b.detach().to(torch.float32).reshape(-1)]).cpu()
    amax = float(w.abs().max())
    if amax == 0.0 or not math.isfinite(amax):
        return None
    k = int(math.floor(math.log2(32768.0 / amax)))
    ws = w * (2.0 ** k)
    if not bool((ws.to(torch.float16).to(torch.float32) == ws).all()) or float(ws.abs().max()) > 65504.0:
        return None
    nz = ws[ws != 0].abs()
    if nz.numel() and float(nz.min()) < 2.0 ** -14:      # a subnormal half would still be exact here, but fma_mix may flush it: stay in the normal range
        return None
    img = pack_lstm_wh(wh_f.detach().to(torch.float32) * (2.0 ** k), wh_b.detach().to(torch.float32) * (2.0 ** k), device, f16=True)
    return img, 2.0 ** -k


def pack_lstm_seq_wh(wh: torch.Tensor, device, f16: bool = False) -> RowMajor16:
    """Recurrent weights ``Wh`` [4H, H] (gate blocks i | f | g | o, the reference's layout) for ``lstm_seq``.  For H % 64 == 0 the rows are re-ordered by
    hidden unit (row 4 j + g): a 16-row tile of the step's GEMM then holds the four gates of four units and the whole step is ONE launch (gates in the
    GEMM's epilogue); other sizes keep the block order and the two-launch step.  ``MI355_LSTM_SEQ_FUSED=0`` keeps the block order everywhere (A/B)."""
    wh = wh.detach().to(torch.float32).cpu()
    h4, h = wh.shape
    assert h4 == 4 * h, wh.shape
    fused = h % 64 == 0 and os.environ.get("MI355_LSTM_SEQ_FUSED", "1") != "0"
    if fused:
        wh = wh.view(4, h, h).permute(1, 0, 2).reshape(4 * h, h).contiguous()
    rm = pack_rowmajor16(wh, None, device, f16=f16)
    rm.interleaved = fused
    return rm


def lstm_seq(xproj: torch.Tensor, wh: RowMajor16, out: torch.Tensor, h0: Optional[torch.Tensor] = None, c0: Optional[torch.Tensor] = None):
    """Unidirectional LSTM recurrence of any hidden size (``mi355_lstm_seq``): ``xproj`` [B, T, 4H] = x @ Wx^T + b (gate order i | f | g | o), ``wh`` the
    row-major 16-bit image of Wh [4H, H] (``pack_lstm_seq_wh``), ``out`` [B, T, H].  Returns (h_T, c_T)."""
    B, T, H4 = xproj.shape
    H = H4 // 4
    assert wh.n == H4 and wh.k == H and wh.scale is None and out.shape == (B, T, H) and xproj.stride(2) == 1 and out.stride(2) == 1
    h = torch.zeros((B, H), dtype=torch.float32, device=xproj.device) if h0 is None else h0.to(torch.float32).contiguous().clone()
    c = torch.zeros((B, H), dtype=torch.float32, device=xproj.device) if c0 is None else c0.to(torch.float32).contiguous().clone()
    pre = torch.empty((B, H4), dtype=torch.float32, device=xproj.device)
    h2 = torch.empty_like(h) if wh.interleaved else None
    _lib.call_struct("mi355_lstm_seq", "mi355_lstm_seq_args", _stream(), xproj=_ptr(xproj), xproj_bstride=xproj.stride(0), ld_xproj=xproj.stride(1),
                     wh=_ptr(wh.w), wdtype=wh.wdtype, h=_ptr(h), c=_ptr(c), pre=_ptr(pre), out=_ptr(out), out_bstride=out.stride(0), ld_out=out.stride(1),
                     B=B, T=T, H=H, gate_interleaved=int(wh.interleaved), h2=_ptr(h2))
    return h, c


GRU_SEQ_HIDDEN = (64, 128, 256)


@dataclass
class GruWh:
    """Recurrent weights of ``gru_seq``: ``w`` the IEEE-half image of Wh / scale ([H/8][3H] 16-byte groups), ``scale`` a power of two."""
    w: torch.Tensor
    scale: float
    h: int


def round_gru_wh(wh: torch.Tensor) -> Tuple[torch.Tensor, int]:
    """(the float32 values the 16-bit image of ``wh`` holds, k): wh * 2^k rounded to IEEE half (nearest even) with 2^k the largest power of two that keeps
    the largest magnitude at or below 32768 -- the scheme of ``pack_lstm_wh_scaled``, except that float32 checkpoints are ROUNDED to half's 11 significant
    bits rather than refused.  fp16- or bf16-representable values no smaller than 2^-28 of the largest magnitude are held exactly."""
    w = wh.detach().to(torch.float32).cpu()
    amax = float(w.abs().max())
    if not math.isfinite(amax):
        raise ValueError("gru: non-finite recurrent weights")
    k = int(math.floor(math.log2(32768.0 / amax))) if amax > 0.0 else 0
    k = max(-126, min(126, k))
    return (w * (2.0 ** k)).to(torch.float16).to(torch.float32) * (2.0 ** -k), k


def pack_gru_wh(wh: torch.Tensor, device) -> GruWh:
    """Recurrent weights ``Wh`` [3H, H] (gate blocks r | z | n, the layout of MLX nn.GRU and of PyTorch's weight_hh) for ``gru_seq``."""
    h3, h = wh.shape
    assert h3 == 3 * h and h % 8 == 0, wh.shape
    wr, k = round_gru_wh(wh)
    img = (wr * (2.0 ** k)).to(torch.float16).view(h3, h // 8, 8).permute(1, 0, 2).contiguous()   # exact: already half values
    return GruWh(img.view(torch.int16).reshape(-1).to(device), 2.0 ** -k, h)


def gru_seq(xproj: torch.Tensor, wh: GruWh, bhn: torch.Tensor, out: torch.Tensor, *, h0: Optional[torch.Tensor] = None, lens: Optional[torch.Tensor] = None,
            return_state: bool = False):
    """Unidirectional GRU recurrence over whole sequences (``mi355_gru_seq``, MLX nn.GRU semantics): ``xproj`` [B, T, 3H] = x @ Wx^T + b (gate blocks
    r | z | n), ``wh`` from ``pack_gru_wh``, ``bhn`` [H], ``out`` [B, T, H]; both may be column views of wider buffers.  ``h0`` [B, H] (default zeros);
    rows at and beyond ``lens[b]`` are written as zeros.  ``return_state``: also returns the state after step ``lens[b]`` [B, H]."""
    B, T, H3 = xproj.shape
    H = wh.h
    assert H3 == 3 * H and out.shape == (B, T, H) and xproj.stride(2) == 1 and out.stride(2) == 1 and xproj.dtype == out.dtype == torch.float32
    assert bhn.shape == (H,) and bhn.dtype == torch.float32 and bhn.is_contiguous()
    assert h0 is None or (h0.shape == (B, H) and h0.dtype == torch.float32 and h0.is_contiguous())
    hT = torch.empty((B, H), dtype=torch.float32, device=xproj.device) if return_state else None
    _lib.call_struct("mi355_gru_seq", "mi355_gru_seq_args", _stream(), xproj=_ptr(xproj), xproj_bstride=xproj.stride(0), ld_xproj=xproj.stride(1),
                     wh=_ptr(wh.w), wh_scale=float(wh.scale), bhn=_ptr(bhn), h0=_ptr(h0), lens=_lens_arg(lens, B), B=B, T=T, H=H,
                     out=_ptr(out), out_bstride=out.stride(0), ld_out=out.stride(1), hT=_ptr(hT))
    return (out, hT) if return_state else out


# --------------------------------------------------------------------------------------- DeepFilterNet (dfn.hip)
DFN_MAX_BANDS, DFN_MAX_CH = 256, 64   # MI355_DFN_MAX_BANDS / MI355_DFN_MAX_CH
DFN_ACT_NONE, DFN_ACT_RELU, DFN_ACT_SIGMOID = 0, 1, 2


def _spec4(t: torch.Tensor):
    assert t.dim() == 4 and t.shape[3] == 2 and t.dtype == torch.float32 and t[0].is_contiguous(), (t.shape, t.stride(), t.dtype)
    return t.stride(0)


def dfn_features(spec: torch.Tensor, *, wnorm: float, alpha: float, one_minus_alpha: float, nb_erb: int, nb_df: int, lookahead: int = 0,
                 erb_fb: Optional[torch.Tensor] = None, erb_start: Optional[torch.Tensor] = None, lens: Optional[torch.Tensor] = None):
    """spec [B, T, F, 2] (re, im) -> (spec * wnorm [B, T, F, 2], feat_erb [B, T, E, 1], feat_df [B, T, D, 2]) (``mi355_dfn_features``): the ERB energies
    (``erb_fb`` [F, E], or band means over ``erb_start`` [E + 1] int32), 10 log10, both running normalisations and the look-ahead shift per item."""
    B, T, F, _ = spec.shape
    sbs = _spec4(spec)
    assert (erb_fb is None) != (erb_start is None)
    assert erb_fb is None or (erb_fb.shape == (F, nb_erb) and erb_fb.is_contiguous() and erb_fb.dtype == torch.float32)
    assert erb_start is None or (erb_start.shape == (nb_erb + 1,) and erb_start.dtype == torch.int32 and erb_start.is_contiguous())
    out = torch.empty((B, T, F, 2), dtype=torch.float32, device=spec.device)
    fe = torch.empty((B, T, nb_erb, 1), dtype=torch.float32, device=spec.device)
    fd = torch.empty((B, T, nb_df, 2), dtype=torch.float32, device=spec.device)
    _lib.call_struct("mi355_dfn_features", "mi355_dfn_features_args", _stream(), spec=_ptr(spec), spec_bstride=sbs, wnorm=float(wnorm), alpha=float(alpha),
                     one_minus_alpha=float(one_minus_alpha), erb_fb=_ptr(erb_fb), erb_start=_ptr(erb_start), lens=_lens_arg(lens, B), B=B, T=T, F=F,
                     E=nb_erb, D=nb_df, lookahead=lookahead, spec_out=_ptr(out), spec_out_bstride=out.stride(0), feat_erb=_ptr(fe), feat_df=_ptr(fd))
    return out, fe, fd


@dataclass
class DfnConv:
    """One fused conv block of ``dfn_conv2d``: the conv weight in its PyTorch layout ([Cmid, Cin / groups, kt, kf], or [Cin, Cmid / groups, kt, kf] when
    ``transposed``), the optional pointwise [Cout, Cmid], the BatchNorm folded to ``scale`` / ``shift`` [Cout], the activation."""
    w: torch.Tensor
    cin: int
    cmid: int
    cout: int
    groups: int
    kt: int
    kf: int
    fstride: int = 1
    transposed: bool = False
    lookahead: int = 0
    pw: Optional[torch.Tensor] = None
    scale: Optional[torch.Tensor] = None
    shift: Optional[torch.Tensor] = None
    act: int = DFN_ACT_NONE


def dfn_conv2d_fo(F: int, kf: int, fstride: int, transposed: bool) -> int:
    return (F - 1) * fstride + kf - kf // 2 if transposed else (F + 2 * (kf // 2) - kf) // fstride + 1


def dfn_conv2d(x: torch.Tensor, cv: DfnConv, *, add: Optional[torch.Tensor] = None, lens: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x [B, T, F, Cin] -> act(BN(pw(conv(x)))) + add, [B, T, Fo, Cout] (``mi355_dfn_conv2d``); frames at and beyond ``lens`` read as zero and are
    written as zeros."""
    B, T, F, C = x.shape
    assert C == cv.cin and x.dtype == torch.float32 and x[0].is_contiguous()
    Fo = dfn_conv2d_fo(F, cv.kf, cv.fstride, cv.transposed)
    y = torch.empty((B, T, Fo, cv.cout), dtype=torch.float32, device=x.device)
    if add is not None:
        assert add.shape == y.shape and add.dtype == torch.float32 and add[0].is_contiguous()
    _lib.call_struct("mi355_dfn_conv2d", "mi355_dfn_conv2d_args", _stream(), x=_ptr(x), x_bstride=x.stride(0), w=_ptr(cv.w), pw=_ptr(cv.pw),
                     scale=_ptr(cv.scale), shift=_ptr(cv.shift), add=_ptr(add), add_bstride=0 if add is None else add.stride(0), lens=_lens_arg(lens, B),
                     B=B, T=T, F=F, Cin=cv.cin, Cmid=cv.cmid, Cout=cv.cout, groups=cv.groups, kt=cv.kt, kf=cv.kf, lookahead=cv.lookahead,
                     fstride=cv.fstride, transposed=int(cv.transposed), act=cv.act, y=_ptr(y), y_bstride=y.stride(0))
    return y


def dfn_apply(spec: torch.Tensor, m: torch.Tensor, erb_inv_fb: torch.Tensor, coef: torch.Tensor, *, order: int, df_lookahead: int, mask_first: bool,
              wnorm: float, lens: Optional[torch.Tensor] = None) -> torch.Tensor:
    """spec [B, T, F, 2], mask m [B, T, E], ``erb_inv_fb`` [E, F], coef [B, T, D, order, 2] -> the enhanced spectrum / wnorm as complex64 [B, T, F]
    (``mi355_dfn_apply``): the layout ``istft_frames`` takes."""
    B, T, F, _ = spec.shape
    sbs = _spec4(spec)
    E, D = erb_inv_fb.shape[0], coef.shape[2]
    assert m.shape[:2] == (B, T) and m.numel() == B * T * E and m.is_contiguous() and erb_inv_fb.shape == (E, F) and erb_inv_fb.is_contiguous()
    assert coef.shape == (B, T, D, order, 2) and coef.is_contiguous() and m.dtype == coef.dtype == erb_inv_fb.dtype == torch.float32
    out = torch.empty((B, T, F, 2), dtype=torch.float32, device=spec.device)
    _lib.call_struct("mi355_dfn_apply", "mi355_dfn_apply_args", _stream(), spec=_ptr(spec), spec_bstride=sbs, m=_ptr(m), erb_inv_fb=_ptr(erb_inv_fb),
                     coef=_ptr(coef), lens=_lens_arg(lens, B), B=B, T=T, F=F, E=E, D=D, order=order, df_lookahead=df_lookahead, mask_first=int(bool(mask_first)),
                     wnorm=float(wnorm), out=_ptr(out), out_bstride=out.stride(0))
    return torch.view_as_complex(out)


# --------------------------------------------------------------------------------------- Mel-Band RoFormer band kernels
BAND_MAX_DIM = 960   # MI355_BAND_MAX_DIM


def band_inverse_host(band_ptr: np.ndarray, band_idx: np.ndarray, n_cac: int):
    """The gather form of ``BandSplit.merge``: for every CaC index j < ``n_cac`` its contributors in ascending band order, as (inv_ptr [n_cac + 1],
    inv_col, inv_bd) int32: ``inv_col`` = the column of the contributor's real part in the ragged row (band n starts at column 4 band_ptr[n]:
    bd_n values, then bd_n gates), ``inv_bd`` = bd_n.  Indices outside [0, n_cac) contribute nowhere."""
    band_ptr, band_idx = np.asarray(band_ptr, dtype=np.int64), np.asarray(band_idx, dtype=np.int64)
    lists = [[] for _ in range(n_cac)]
    for n in range(len(band_ptr) - 1):
        p0, p1 = int(band_ptr[n]), int(band_ptr[n + 1])
        for m in range(p1 - p0):
            j = int(band_idx[p0 + m])
            if 0 <= j < n_cac:
                lists[j].append((4 * p0 + 2 * m, 2 * (p1 - p0)))
    inv_ptr = np.zeros(n_cac + 1, dtype=np.int32)
    inv_ptr[1:] = np.cumsum([len(c) for c in lists])
    flat = [e for c in lists for e in c]
    inv_col = np.array([e[0] for e in flat], dtype=np.int32)
    inv_bd = np.array([e[1] for e in flat], dtype=np.int32)
    return inv_ptr, inv_col, inv_bd


@dataclass
class BandTables:
    """The CSR band tables of ``band_split`` / ``band_merge`` on the host (int32 numpy) and on the device."""
    band_ptr: np.ndarray
    band_idx: np.ndarray
    freq_bins: int
    ptr_d: torch.Tensor
    idx_d: torch.Tensor
    inv_ptr_d: torch.Tensor
    inv_col_d: torch.Tensor
    inv_bd_d: torch.Tensor
    n_inv: int

    @property
    def num_bands(self) -> int:
        return len(self.band_ptr) - 1

    @property
    def band_dims(self):
        return [int(2 * (self.band_ptr[n + 1] - self.band_ptr[n])) for n in range(self.num_bands)]

    @property
    def h_cols(self) -> int:
        return int(4 * self.band_ptr[-1])


def band_tables(band_indices, freq_bins: int, device) -> BandTables:
    """``band_indices``: one list of CaC indices (2 * bin + channel) per band, any order, any overlap."""
    ptr = np.zeros(len(band_indices) + 1, dtype=np.int32)
    ptr[1:] = np.cumsum([len(ix) for ix in band_indices])
    idx = np.concatenate([np.asarray(ix, dtype=np.int32).reshape(-1) for ix in band_indices]).astype(np.int32) if ptr[-1] else np.zeros(0, np.int32)
    inv_ptr, inv_col, inv_bd = band_inverse_host(ptr, idx, 2 * freq_bins)
    up = lambda v: torch.from_numpy(np.ascontiguousarray(v if v.size else np.zeros(1, np.int32))).to(device)   # never a null pointer for an empty list
    return BandTables(ptr, idx, freq_bins, up(ptr), up(idx), up(inv_ptr), up(inv_col), up(inv_bd), int(inv_ptr[-1]))


def pack_band_split(weights, gammas, biases, device):
    """Per-band ``Linear`` weights [D, bd_n], RMSNorm scales [bd_n] and biases [D] -> (wt, gamma, bias) of ``band_split``: the ragged concatenation
    of the transposed weights, the ragged scales, bias [Nb, D]."""
    f = lambda t: torch.as_tensor(t).detach().to(torch.float32).cpu()
    wt = torch.cat([f(w).t().contiguous().reshape(-1) for w in weights])
    return wt.to(device), torch.cat([f(g).reshape(-1) for g in gammas]).to(device), torch.stack([f(b) for b in biases]).contiguous().to(device)


def _spec_planes(spec: torch.Tensor):
    """complex64 [B2, T, F] (or float32 [B2, T, F, 2]) -> (float view, B2, T, F, channel stride, frame stride)."""
    s = torch.view_as_real(spec) if spec.is_complex() else spec
    assert s.dim() == 4 and s.shape[3] == 2 and s.dtype == torch.float32 and s.is_cuda and s.stride(3) == 1 and s.stride(2) == 2, (s.shape, s.stride(), s.dtype)
    return s, s.shape[0], s.shape[1], s.shape[2], s.stride(0), s.stride(1)


def band_split(spec: torch.Tensor, tab: BandTables, wt: torch.Tensor, gamma: torch.Tensor, bias: torch.Tensor, y: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The STFT of B * 2 channel items (``stft_frames``: complex64 [B * 2, T, F]) -> y [B, T, Nb, D] (``mi355_band_split``): per band the gather of
    its CaC entries, ``x / max(||x||, 1e-12) * sqrt(bd) * gamma`` and the band's Linear, one launch."""
    s, B2, T, F, cs, ts = _spec_planes(spec)
    Nb, D = tab.num_bands, bias.shape[1]
    assert B2 % 2 == 0 and F == tab.freq_bins and bias.shape == (Nb, D) and bias.is_contiguous() and wt.is_contiguous() and gamma.is_contiguous()
    assert wt.numel() == D * 2 * int(tab.band_ptr[-1]) and gamma.numel() == 2 * int(tab.band_ptr[-1]) and wt.dtype == gamma.dtype == bias.dtype == torch.float32
    if y is None:
        y = torch.empty((B2 // 2, T, Nb, D), dtype=torch.float32, device=s.device)
    assert y.shape == (B2 // 2, T, Nb, D) and y.dtype == torch.float32 and y[0].is_contiguous()
    _lib.call_struct("mi355_band_split", "mi355_band_split_args", _stream(), spec=_ptr(s), spec_cstride=cs, spec_tstride=ts, band_ptr=_ptr(tab.ptr_d),
                     band_idx=_ptr(tab.idx_d), n_idx=int(tab.band_ptr[-1]), max_band_dim=max(tab.band_dims), wt=_ptr(wt), gamma=_ptr(gamma), bias=_ptr(bias),
                     B=B2 // 2, T=T, F=F, Nb=Nb, D=D, y=_ptr(y), y_bstride=y.stride(0))
    return y


def band_merge(h: torch.Tensor, tab: BandTables, spec: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """h [B, T, >= 4 * sum(index counts)] (the ragged output of the last per-band Linear: band n's bd_n values, then its bd_n gates, from column
    4 band_ptr[n]) and the input spectrum -> the masked spectrum, complex64 [B * 2, F, T] (``mi355_band_merge``): GLU, the scatter as a gather in
    ascending band order, the overlap average and the complex product.  ``out``: a float32 [B * 2, F, T, 2] view to fill (any f / t strides, e.g.
    the transpose of a [B * 2, T, F, 2] buffer)."""
    s, B2, T, F, cs, ts = _spec_planes(spec)
    B, Th, _, hbs, ldh = _nlc(h)
    assert 2 * B == B2 and Th == T and F == tab.freq_bins and h.shape[2] >= tab.h_cols
    if out is None:
        out = torch.empty((B2, F, T, 2), dtype=torch.float32, device=s.device)
    assert out.shape == (B2, F, T, 2) and out.dtype == torch.float32 and out.stride(3) == 1
    _lib.call_struct("mi355_band_merge", "mi355_band_merge_args", _stream(), h=_ptr(h), h_bstride=hbs, ldh=ldh, h_cols=tab.h_cols, inv_ptr=_ptr(tab.inv_ptr_d),
                     inv_col=_ptr(tab.inv_col_d), inv_bd=_ptr(tab.inv_bd_d), n_inv=tab.n_inv,
                     spec=_ptr(s), spec_cstride=cs, spec_tstride=ts, B=B, T=T, F=F, out=_ptr(out), out_cstride=out.stride(0), out_fstride=out.stride(1),
                     out_tstride=out.stride(2))
    return torch.view_as_complex(out)


def head_gate(x: torch.Tensor, g: torch.Tensor, *, heads: int, dh: int) -> torch.Tensor:
    """x[b, l, h * dh + i] *= sigmoid(g[b, l, h]) in place (``mi355_head_gate``); x [B, L, >= heads * dh] and g [B, L, >= heads] channels-last views."""
    B, L, Cx, xbs, ldx = _nlc(x)
    Bg, Lg, Cg, gbs, ldg = _nlc(g)
    assert Bg == B and Lg == L
    if Cx < heads * dh or Cg < heads:
        raise _lib.Mi355Error(f"head_gate: {heads} heads of {dh} do not fit views of {Cx} and {Cg} columns")
    _lib.call_struct("mi355_head_gate", "mi355_head_gate_args", _stream(), x=_ptr(x), x_bstride=xbs, ldx=ldx, g=_ptr(g), g_bstride=gbs, ldg=ldg,
                     heads=heads, dh=dh, L=L, B=B)
    return x


# --------------------------------------------------------------------------------------- conv / linear
def _conv_gemm_args(x, pc, y, dil, pad, lens_in, lens_out, lout, pre, pre_act, pre_slope, pre_alpha, post_act, post_slope, res, res_shift, out_scale, accumulate, up,
                    precision, tile, flat, use_bias, stats, pre_inv_beta, colscale, x_off, flatten, pre_fq, ext, x_split, y_split):
    """The ``mi355_conv_gemm_args`` fields of one ``conv_gemm`` call (its arguments, in its order), after the ``flatten`` rewrite."""
    if flatten and pc.k == 1 and up is None and flat is None and res_shift == 0 and stats is None and pre is None and pre_fq is None and x.shape[0] > 1:
        ts = [x, y] + ([res] if res is not None else [])
        if all(t.dim() == 3 and t.shape[:2] == x.shape[:2] and t.stride(0) == t.shape[1] * t.stride(1) for t in ts):
            fl = lambda t: t.as_strided((1, t.shape[0] * t.shape[1], t.shape[2]), (t.shape[0] * t.shape[1] * t.stride(1), t.stride(1), 1))
            return _conv_gemm_args(fl(x), pc, fl(y), 1, 0, None, None, None, None, pre_act, pre_slope, pre_alpha, post_act, post_slope, None if res is None else fl(res), 0,
                                   out_scale, accumulate, None, precision, tile, None, use_bias, None, pre_inv_beta, colscale, x_off, False, None, None, x_split, y_split)
    B, Lin, Cx, xbs, ldx = _nlc(x)
    By, Ly, Cy, ybs, ldy = _nlc(y)
    assert B == By
    if pc.mx:
        precision = 6 if pc.mx == 2 else 5  # the weight image decides
    elif pc.f16:
        if precision not in (3, 4):
            precision = 4 if precision in (5, 6) else 3  # fp16-packed weights only fit the fp16 MFMA paths (3 single, 4 hi+lo; mode 5 = hi+lo where no MX image exists)
    elif precision in (3, 4, 5, 6):
        raise _lib.Mi355Error("conv_gemm: precision 3 / 4 need weights packed with f16=True, precision 5 / 6 with mx=True / mx=2")
    kw = dict(x=_ptr(x), x_bstride=xbs, ldx=ldx, x_off=x_off, Cin=pc.cin, Lin=Lin, lens_in=_ptr(lens_in), flat_valid=0,
              w=_ptr(pc.w), Cout=pc.cout, K=pc.k, dil=dil, pad=pad, pre_act=pre_act, pre_slope=pre_slope,
              pre_alpha=_ptr(pre_alpha), bias=_ptr(pc.bias) if use_bias else None, post_act=post_act,
              post_slope=post_slope, out_scale=out_scale, accumulate=int(accumulate), y=_ptr(y), y_bstride=ybs, ldy=ldy,
              Lout=lout if lout is not None else Ly, lens_out=_ptr(lens_out), B=B, precision=precision, tile=tile,
              pre_inv_beta=_ptr(pre_inv_beta), post_colscale=_ptr(colscale))
    if x_split or y_split:
        if precision not in (2, 4):
            raise _lib.Mi355Error("conv_gemm: split activations exist for the hi + lo precisions 2 and 4 only")
        kw.update(x_split=precision if x_split else 0, y_split=precision if y_split else 0)
    if pre_fq is not None:  # [B, 2] from fake_quant_extrema (same prologue arguments): the prologue ends with the dynamic uint8 fake quantisation
        assert pre_fq.dtype == torch.float32 and pre_fq.shape == (B, 2) and pre_fq.is_contiguous()
        kw.update(pre_fq=_ptr(pre_fq))
    if flat is not None:  # flattened strided conv: taps are contiguous in memory (C_in small)
        kw.update(ldx=flat["ldx"], x_off=flat["x_off"], flat_valid=flat["channels"])
    else:
        assert Cx >= pc.cin or ldx >= pc.cin, (Cx, pc.cin)
    if pre is not None:
        sc, sh = pre
        assert sc.dim() == 2 and sc.stride(1) == 1 and sc.stride(0) == sh.stride(0)
        kw.update(pre_scale=_ptr(sc), pre_shift=_ptr(sh), pre_ld=sc.stride(0))
    if res is not None:
        _, _, _, rbs, ldr = _nlc(res)
        kw.update(res=_ptr(res), res_bstride=rbs, ldr=ldr, res_shift=res_shift)
    if up is not None:
        kw.update(up_s=up["s"], up_p=up["p"], up_cout=up["cout"], up_row_off=up.get("row_off", 0),
                  up_Lout=up["lout"], lens_up=_ptr(up.get("lens")))
    if ext is not None:
        assert ext.dtype == torch.float32 and ext.dim() == 4 and ext.is_contiguous() and ext.shape[0] == B and ext.shape[2] == pc.cout
        assert ext.shape[1] >= (kw["Lout"] + STATS_ROWS - 1) // STATS_ROWS
        kw.update(ext_partial=_ptr(ext), ext_bstride=ext.stride(0))
    if stats is not None:  # [B, ceil(Lout / 64), Cout, 2] float32: per-row-block (sum, M2) of the stored output
        assert stats.dtype == torch.float32 and stats.dim() == 4 and stats.is_contiguous()
        assert stats.shape[0] == B and stats.shape[1] >= (kw["Lout"] + STATS_ROWS - 1) // STATS_ROWS and stats.shape[2] == pc.cout
        kw.update(stats_partial=_ptr(stats), stats_bstride=stats.stride(0))
    if SPLIT_WS_BYTES and B * kw["Lout"] <= 65536:   # only small launches can split: do not even create the scratch for a large batch
        st = _stream()
        kw.update(split_ws=_conv_split_ws(x.device, st).data_ptr(), split_ws_bytes=SPLIT_WS_BYTES)
    return kw


def conv_gemm(x: torch.Tensor, pc: PackedConv, y: torch.Tensor, *, dil: int = 1, pad: int = 0,
              lens_in: Optional[torch.Tensor] = None, lens_out: Optional[torch.Tensor] = None,
              lout: Optional[int] = None, pre: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
              pre_act: int = ACT_NONE, pre_slope: float = 0.0, pre_alpha: Optional[torch.Tensor] = None,
              post_act: int = ACT_NONE, post_slope: float = 0.0, res: Optional[torch.Tensor] = None,
              res_shift: int = 0, out_scale: float = 1.0, accumulate: bool = False,
              up: Optional[dict] = None, precision: int = 2, tile: int = 0,
              flat: Optional[dict] = None, use_bias: bool = True, stats: Optional[torch.Tensor] = None,
              pre_inv_beta: Optional[torch.Tensor] = None, colscale: Optional[torch.Tensor] = None, x_off: int = 0,
              flatten: bool = False, pre_fq: Optional[torch.Tensor] = None, ext: Optional[torch.Tensor] = None,
              x_split: bool = False, y_split: bool = False):
    """y = epilogue(conv1d(prologue(x)))  -- see mi355_conv_gemm_args in the header.

    ``x_split`` / ``y_split``: the float32 tensors ``x`` / ``y`` hold SPLIT words (16-bit hi | lo << 16 of each value in the type of the launch's
    precision, 2 or 4: ``split16``, ``layernorm(split=...)`` or another launch's ``y_split``) -- the conversion is then done once by the producer
    instead of once per column tile of this launch.

    ``ext`` ([B, ceil(Lout / 64), Cout, 2] from ``new_ext``): the launch also leaves the per-block, per-channel (min, max) of what it stores, for
    ``fake_quant_extrema_from_partials`` -- only launches ``conv_ext_supported`` accepts (a quantising prologue on the wave-specialised kernel).

    ``flatten``: the caller states that this is a per-row linear layer (K == 1) whose padding rows (rows >= lens[b]) may be
    computed and written like any other row (nothing downstream reads them as valid): ``[B, L, C]`` operands whose items are
    row-contiguous are then handed over as ONE item of B*L rows, so the 128-row tiles are full instead of one partly
    filled tile per utterance (PL-BERT at T = 80: 62 % -> 100 % useful rows)."""
    kw = _conv_gemm_args(x, pc, y, dil, pad, lens_in, lens_out, lout, pre, pre_act, pre_slope, pre_alpha, post_act, post_slope, res, res_shift, out_scale, accumulate, up,
                         precision, tile, flat, use_bias, stats, pre_inv_beta, colscale, x_off, flatten, pre_fq, ext, x_split, y_split)
    if PROFILE is not None:
        # no host synchronisation here (a .item() on the ragged lengths would drain the queue before every launch: the start event would then
        # be stamped on an idle GPU and the interval would include the host's submission latency); the row count stays a device scalar and
        # profile_finalize() resolves it after the step
        rows = (kw["Lout"] * kw["B"]) if kw["lens_out"] is None else lens_out.sum()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _lib.call_struct("mi355_conv_gemm", "mi355_conv_gemm_args", _stream(), **kw)
        e1.record()
        PROFILE.append((rows, pc.cin, pc.cout, pc.k, kw["dil"], int(res is not None) + int(bool(accumulate)), e0, e1))
        return y
    _lib.call_struct("mi355_conv_gemm", "mi355_conv_gemm_args", _stream(), **kw)
    return y


def conv_route(x: torch.Tensor, pc: PackedConv, y: torch.Tensor, *, dil: int = 1, pad: int = 0,
               lens_in: Optional[torch.Tensor] = None, lens_out: Optional[torch.Tensor] = None,
               lout: Optional[int] = None, pre: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
               pre_act: int = ACT_NONE, pre_slope: float = 0.0, pre_alpha: Optional[torch.Tensor] = None,
               post_act: int = ACT_NONE, post_slope: float = 0.0, res: Optional[torch.Tensor] = None,
               res_shift: int = 0, out_scale: float = 1.0, accumulate: bool = False,
               up: Optional[dict] = None, precision: int = 2, tile: int = 0,
               flat: Optional[dict] = None, use_bias: bool = True, stats: Optional[torch.Tensor] = None,
               pre_inv_beta: Optional[torch.Tensor] = None, colscale: Optional[torch.Tensor] = None, x_off: int = 0,
               flatten: bool = False, pre_fq: Optional[torch.Tensor] = None, ext: Optional[torch.Tensor] = None,
               x_split: bool = False, y_split: bool = False):
    """Which kernel ``conv_gemm`` with these arguments runs, and on what geometry: the ``mi355_conv_route`` record of the header as a dict.  Launches
    nothing; a call ``conv_gemm`` refuses raises the same error."""
    kw = _conv_gemm_args(x, pc, y, dil, pad, lens_in, lens_out, lout, pre, pre_act, pre_slope, pre_alpha, post_act, post_slope, res, res_shift, out_scale, accumulate, up,
                         precision, tile, flat, use_bias, stats, pre_inv_beta, colscale, x_off, flatten, pre_fq, ext, x_split, y_split)
    return _lib.call_struct_out("mi355_conv_gemm_route", "mi355_conv_gemm_args", "mi355_conv_route", **kw)


def adain_coef(x: torch.Tensor, gb: Optional[torch.Tensor], lens: Optional[torch.Tensor] = None, eps: float = 1e-5, sums: Optional[torch.Tensor] = None,
               reuse: bool = False):
    """Instance-norm stats of ``x`` [B, L, C] + AdaIN coefficients -> (scale, shift) each [B, C padded to 32].
    ``sums`` (float64 [B * C * 2]) + ``reuse=True``: the statistics of this same ``x`` are already in ``sums`` (an earlier call): only the coefficients
    for another ``gb`` are computed -- one statistics pass for all blocks that normalise the same input."""
    B, L, C, xbs, ldx = _nlc(x)
    cp = round_up(C, 32)
    if sums is None:
        assert not reuse
        sums = torch.empty(B * C * 2, dtype=torch.float64, device=x.device)
    scale = torch.empty((B, cp), dtype=torch.float32, device=x.device)
    shift = torch.empty((B, cp), dtype=torch.float32, device=x.device)
    _lib.call_struct("mi355_adain_coef", "mi355_adain_coef_args", _stream(), x=_ptr(x), x_bstride=xbs, ldx=ldx, C=C, L=L,
                     lens=_ptr(lens), B=B, sums=_ptr(sums), gb=_ptr(gb), gb_ld=0 if gb is None else gb.stride(0), eps=eps,
                     scale=_ptr(scale), shift=_ptr(shift), out_ld=cp, reuse_sums=int(reuse))
    return scale, shift


STATS_ROWS = 64  # MI355_STATS_ROWS

# scratch of mi355_conv_gemm's split-K path (launches of few output tiles: one utterance per call), one per (device, stream): launches on a stream
# are ordered, so consecutive convs can share it.  A fixed 96 MB (MI355_CONV_SPLIT_WS_MB): the dispatcher caps the group count by what fits, so a
# smaller workspace only means fewer groups.  NOTE (round-3 advisor): whether a launch splits depends on its tile count B * L_out, so one utterance
# takes a different fp32 summation order alone than inside a batch -- deterministic per shape, equal across shapes only to rounding; code that
# asserts integer results across batch sizes (durations, token ids) must do so under a margin (tests/test_kokoro_gpu.py, tests/_margin.py)
SPLIT_WS_BYTES = int(os.environ.get("MI355_CONV_SPLIT_WS_MB", "96")) << 20
_CONV_SPLIT_WS = {}


def _conv_split_ws(device: torch.device, stream: int) -> torch.Tensor:
    key = (device.index, stream)
    ws = _CONV_SPLIT_WS.get(key)
    if ws is None:
        ws = _CONV_SPLIT_WS[key] = torch.empty(SPLIT_WS_BYTES, dtype=torch.uint8, device=device)
    return ws


def new_stats(B: int, L: int, C: int, device) -> torch.Tensor:
    """Buffer for the fused instance-norm statistics of a conv output [B, L, C] (see conv_gemm(stats=...))."""
    return torch.empty((B, (L + STATS_ROWS - 1) // STATS_ROWS, C, 2), dtype=torch.float32, device=device)


def new_ext(B: int, L: int, C: int, device) -> torch.Tensor:
    """Buffer for the per-block extrema a conv launch leaves (``conv_gemm(ext=...)``): [B, ceil(L / 64), C, 2] = (min, max)."""
    return torch.empty((B, (L + STATS_ROWS - 1) // STATS_ROWS, C, 2), dtype=torch.float32, device=device)


def conv_ext_supported(x: torch.Tensor, pc: PackedConv, *, B: int, lout: int, dil: int = 1, pre_act: int = ACT_NONE, post_act: int = ACT_NONE,
                       up: Optional[dict] = None, flat: Optional[dict] = None, precision: int = 2, min_tiles: int = 128) -> bool:
    """Will ``conv_gemm(..., pre_fq=..., ext=...)`` of this shape be taken by the kernel that writes extrema partials -- AND would the dispatcher have
    chosen that kernel anyway (at least ``min_tiles`` 128-row tiles: the rule of ``mi355_conv_gemm``'s automatic choice), so that asking for the
    partials does not change which kernel computes the conv?"""
    if up is not None or flat is not None or pc.f16 or pc.mx or precision != 2 or pc.k == 1:
        return False
    _, _, _, xbs, ldx = _nlc(x)
    bn = 64 if pc.cout <= 64 else 128
    if B * ((lout + 127) // 128) * ((pc.cout + bn - 1) // bn) < min_tiles:
        return False
    return bool(_lib.call_struct_ret("mi355_conv_gemm_ext_supported", "mi355_conv_gemm_args", x=_ptr(x), x_bstride=xbs, ldx=ldx, Cin=pc.cin, Lin=x.shape[1],
                                     w=_ptr(pc.w), Cout=pc.cout, K=pc.k, dil=dil, pre_act=pre_act, post_act=post_act, Lout=lout, B=B, precision=2,
                                     pre_alpha=_ptr(pc.w), pre_fq=_ptr(pc.w), y=_ptr(pc.w)))   # the probe reads shapes, flags and x's alignment; the other pointers only have to be set


def fake_quant_extrema_from_partials(ext: torch.Tensor, L: int, *, lens=None, pre=None, pre_act: int = ACT_NONE, pre_slope: float = 0.0,
                                     pre_alpha: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``[B, 2]`` = {-min, max} of ``act(scale * x + shift)`` per utterance from the per-block, per-channel (min, max) of x that the conv producing x
    left (``conv_gemm(ext=...)``): what ``fake_quant_extrema`` computes by reading x again."""
    B, nblk, C, two = ext.shape
    assert two == 2 and ext.is_contiguous() and nblk >= (L + STATS_ROWS - 1) // STATS_ROWS
    mm = torch.empty((B, 2), dtype=torch.float32, device=ext.device)
    sc, sh = pre if pre is not None else (None, None)
    _lib.call_struct("mi355_fake_quant_extrema_from_partials", "mi355_fake_quant_args", _stream(), x=_ptr(ext), x_bstride=ext.stride(0), ldx=2 * C, C=C, L=L,
                     lens=_ptr(lens), B=B, pre_scale=_ptr(sc), pre_shift=_ptr(sh), pre_ld=sc.stride(0) if sc is not None else 0, pre_act=pre_act,
                     pre_slope=pre_slope, pre_alpha=_ptr(pre_alpha), minmax=_ptr(mm))
    return mm


def adain_from_partials(stats: torch.Tensor, L: int, gb: Optional[torch.Tensor], lens: Optional[torch.Tensor] = None, eps: float = 1e-5):
    """AdaIN (scale, shift) from the per-row-block partial statistics a conv_gemm epilogue wrote."""
    B, _, C, _ = stats.shape
    cp = round_up(C, 32)
    scale = torch.empty((B, cp), dtype=torch.float32, device=stats.device)
    shift = torch.empty((B, cp), dtype=torch.float32, device=stats.device)
    _lib.call_struct("mi355_adain_from_partials", "mi355_adain_partials_args", _stream(), partials=_ptr(stats), bstride=stats.stride(0),
                     C=C, L=L, lens=_ptr(lens), B=B, gb=_ptr(gb), gb_ld=0 if gb is None else gb.stride(0), eps=eps,
                     scale=_ptr(scale), shift=_ptr(shift), out_ld=cp)
    return scale, shift


GN_PART_ELEMS = 4096  # MI355_GN_PART_ELEMS


def group_norm_stats(x: torch.Tensor, lens: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Per-sample partial statistics of ``x`` [B, L, C] for a one-group GroupNorm (``mi355_group_norm_stats``): float64
    [B, ceil(L * C / GN_PART_ELEMS), 2] = (sum, sum of squared deviations from the part's mean) per part of consecutive elements."""
    B, L, C, xbs, ldx = _nlc(x)
    assert x.dtype == torch.float32
    parts = torch.empty((B, (L * C + GN_PART_ELEMS - 1) // GN_PART_ELEMS, 2), dtype=torch.float64, device=x.device)
    _lib.call_struct("mi355_group_norm_stats", "mi355_group_norm_stats_args", _stream(), x=_ptr(x), x_bstride=xbs, ldx=ldx, C=C, L=L, lens=_ptr(lens), B=B,
                     partials=_ptr(parts), partials_bstride=parts.stride(0))
    return parts


def group_norm_coef(partials: torch.Tensor, L: int, C: int, weight: Optional[torch.Tensor], bias: Optional[torch.Tensor], *, eps: float = 1e-5,
                    lens: Optional[torch.Tensor] = None, rep: int = 1, return_stats: bool = False):
    """GroupNorm(1, C) coefficients (scale, shift), each [B, rep * C padded to 32] -- the ``pre=`` operands of ``conv_gemm`` -- from the partials of
    ``group_norm_stats`` (float64 [B, parts, 2]) or from the ``stats=`` buffer a conv epilogue wrote (float32 [B, blocks, C, 2], merged over blocks and
    channels).  ``rep``: the coefficient row repeated for a strided conv that reads regrouped rows [rows / rep, rep * C].
    ``return_stats`` adds the per-sample (mean, rstd) [B, 2]."""
    conv = partials.dim() == 4
    assert partials.is_contiguous() and partials.dtype == (torch.float32 if conv else torch.float64)
    assert (partials.shape[2] == C and partials.shape[3] == 2) if conv else partials.shape[2] == 2
    B = partials.shape[0]
    ld = round_up(rep * C, 32)
    scale = torch.empty((B, ld), dtype=torch.float32, device=partials.device)
    shift = torch.empty((B, ld), dtype=torch.float32, device=partials.device)
    mr = torch.empty((B, 2), dtype=torch.float32, device=partials.device) if return_stats else None
    _lib.call_struct("mi355_group_norm_coef", "mi355_group_norm_coef_args", _stream(), partials=_ptr(partials), partials_bstride=partials.stride(0),
                     conv_partials=int(conv), C=C, L=L, lens=_ptr(lens), B=B, weight=_ptr(weight), bias=_ptr(bias), eps=eps, rep=rep,
                     scale=_ptr(scale), shift=_ptr(shift), out_ld=ld, mean_rstd=_ptr(mr))
    return (scale, shift, mr) if return_stats else (scale, shift)


def group_norm_apply(x0: torch.Tensor, coef0, y: torch.Tensor, x1: Optional[torch.Tensor] = None, coef1=None, *, row_off0: int = 0, row_off1: int = 0):
    """``y = x0[:, row_off0:] * scale0 + shift0 (+ x1[:, row_off1:] * scale1 + shift1, or + x1 when coef1 is None)`` over the rows of ``y`` [B, L, C]
    (``mi355_group_norm_apply``); ``coef*`` = (scale, shift) of ``group_norm_coef``."""
    B, L, C, ybs, ldy = _nlc(y)
    B0, L0, C0, x0bs, ldx0 = _nlc(x0)
    sc0, sh0 = coef0
    assert B0 == B and C0 == C and row_off0 >= 0 and L0 >= L + row_off0 and sc0.stride(0) == sh0.stride(0) and sc0.shape[0] == B and sc0.stride(1) == 1
    kw = dict(x0=_ptr(x0), x0_bstride=x0bs, ldx0=ldx0, row_off0=row_off0, scale0=_ptr(sc0), shift0=_ptr(sh0), coef_ld=sc0.stride(0), C=C, L=L, B=B,
              y=_ptr(y), y_bstride=ybs, ldy=ldy)
    if x1 is not None:
        B1, L1, C1, x1bs, ldx1 = _nlc(x1)
        assert B1 == B and C1 == C and row_off1 >= 0 and L1 >= L + row_off1
        kw.update(x1=_ptr(x1), x1_bstride=x1bs, ldx1=ldx1, row_off1=row_off1)
        if coef1 is not None:
            sc1, sh1 = coef1
            assert sc1.stride(0) == sc0.stride(0) and sh1.stride(0) == sc0.stride(0) and sc1.shape[0] == B
            kw.update(scale1=_ptr(sc1), shift1=_ptr(sh1))
    else:
        assert coef1 is None
    _lib.call_struct("mi355_group_norm_apply", "mi355_group_norm_apply_args", _stream(), **kw)
    return y


def layernorm(x: torch.Tensor, y: torch.Tensor, *, weight=None, bias=None, ada_gb=None, res=None, eps=1e-5,
              lens=None, post_act=ACT_NONE, post_slope=0.0, split: int = 0):
    """``split`` = 2 / 4: ``y`` receives SPLIT words (``conv_gemm(..., x_split=True)`` at that precision reads them) instead of floats."""
    B, L, C, xbs, ldx = _nlc(x)
    _, _, _, ybs, ldy = _nlc(y)
    kw = dict(x=_ptr(x), x_bstride=xbs, ldx=ldx, C=C, L=L, lens=_ptr(lens), B=B, weight=_ptr(weight), bias=_ptr(bias),
              ada_gb=_ptr(ada_gb), ada_ld=0 if ada_gb is None else ada_gb.stride(0), eps=eps, post_act=post_act,
              post_slope=post_slope, y=_ptr(y), y_bstride=ybs, ldy=ldy, y_split=int(split))
    if res is not None:
        _, _, _, rbs, ldr = _nlc(res)
        kw.update(res=_ptr(res), res_bstride=rbs, ldr=ldr)
    _lib.call_struct("mi355_layernorm", "mi355_layernorm_args", _stream(), **kw)
    return y


def split16(x: torch.Tensor, fmt: int, y: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 -> SPLIT words (16-bit hi | lo << 16; ``fmt`` 2 = bfloat16, 4 = IEEE half) of a contiguous float32 tensor, for ``conv_gemm(..., x_split=True)`` at
    precision ``fmt``; ``y`` defaults to a fresh tensor (``y is x``: in place).  The words travel in a float32 tensor: read them with ``.view(torch.int32)``."""
    assert x.dtype == torch.float32 and x.is_contiguous() and x.numel() % 4 == 0
    if y is None:
        y = torch.empty_like(x)
    assert y.dtype == torch.float32 and y.is_contiguous() and y.numel() == x.numel()
    lib = _lib.load()
    _lib.check(lib.mi355_split16(_ptr(x), _ptr(y), x.numel(), int(fmt), _stream()), "mi355_split16")
    return y


def lstm_bidir(xp: torch.Tensor, wh: torch.Tensor, H: int, out: torch.Tensor, lens=None, quant_h: bool = False, wh_f16: bool = False,
               wh_scale: float = 0.0):
    B, L, _, xbs, ldxp = _nlc(xp)
    _, _, _, obs, ldo = _nlc(out)
    _lib.call_struct("mi355_lstm_bidir", "mi355_lstm_args", _stream(), xp=_ptr(xp), xp_bstride=xbs, ldxp=ldxp, wh=_ptr(wh),
                     H=H, L=L, lens=_ptr(lens), B=B, out=_ptr(out), out_bstride=obs, ldo=ldo, quant_h=int(bool(quant_h)), wh_f16=int(bool(wh_f16)),
                     wh_scale=float(wh_scale))
    return out


def fake_quant_u8(x: torch.Tensor, y: Optional[torch.Tensor] = None, *, lens=None, pre=None, pre_act: int = ACT_NONE, pre_slope: float = 0.0,
                  pre_alpha: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``fake_quant_dynamic_u8`` (tts/models/kitten_tts/quant.py) of ``act(scale * x + shift)`` per utterance: x [B, L, C] -> y (a fresh
    tensor unless given; ``y is x`` quantises in place)."""
    B, L, C, xbs, ldx = _nlc(x)
    if y is None:  # channel-padded like every conv input of the engines (rows past lens[b] and the pad columns stay zero)
        y = torch.zeros((B, L, round_up(C, 32)), dtype=torch.float32, device=x.device)[:, :, :C]
    _, _, _, ybs, ldy = _nlc(y)
    mm = torch.empty((B, 2), dtype=torch.float32, device=x.device)
    sc, sh = pre if pre is not None else (None, None)
    _lib.call_struct("mi355_fake_quant_u8", "mi355_fake_quant_args", _stream(), x=_ptr(x), x_bstride=xbs, ldx=ldx, C=C, L=L, lens=_ptr(lens), B=B,
                     pre_scale=_ptr(sc), pre_shift=_ptr(sh), pre_ld=sc.stride(0) if sc is not None else 0, pre_act=pre_act, pre_slope=pre_slope,
                     pre_alpha=_ptr(pre_alpha), y=_ptr(y), y_bstride=ybs, ldy=ldy, minmax=_ptr(mm))
    return y


def rvq_encode(x: torch.Tensor, tables: torch.Tensor, tables_t: torch.Tensor, c2: torch.Tensor, margins: bool = False):
    """Residual VQ encode of the projected frames ``x`` [rows, D] over ``tables`` [n, bins, D] (+ transposed copy [n, D, bins] and |e|^2 / 2 [n, bins]):
    codes int32 [rows, n] (and the best-vs-second score gaps when ``margins``)."""
    assert x.dim() == 2 and x.stride(1) == 1 and tables.is_contiguous() and tables_t.is_contiguous() and c2.is_contiguous()
    rows, D = x.shape
    n, bins, D2 = tables.shape
    assert D2 == D and tuple(tables_t.shape) == (n, D, bins) and tuple(c2.shape) == (n, bins)
    codes = torch.empty((rows, n), dtype=torch.int32, device=x.device)
    mg = torch.empty((rows, n), dtype=torch.float32, device=x.device) if margins else None
    _lib.call_struct("mi355_rvq_encode", "mi355_rvq_encode_args", _stream(), x=_ptr(x), rows=rows, ldx=x.stride(0), D=D, tables=_ptr(tables), tables_t=_ptr(tables_t),
                     c2=_ptr(c2), bins=bins, n_layers=n, codes=_ptr(codes), ld_codes=n, margins=_ptr(mg))
    return (codes, mg) if margins else codes


def ecapa_rows(x: torch.Tensor, y: torch.Tensor, *, pad: int = 0, gate: Optional[torch.Tensor] = None, res: Optional[torch.Tensor] = None,
               pre_tanh: bool = False) -> torch.Tensor:
    """``y[b, r] = f(x[b, s]) * sigmoid(gate[b]) + res[b, s]``, ``s = reflect(r - pad)``: x / res [B, T, C] (channel slices of wider buffers are fine),
    gate [B, C] logits, y [B, T + 2 * pad, C] -- see mi355_ecapa_rows_args."""
    B, T, C, xbs, ldx = _nlc(x)
    By, Ty, Cy, ybs, ldy = _nlc(y)
    assert (By, Ty, Cy) == (B, T + 2 * pad, C), ((By, Ty, Cy), (B, T, C), pad)
    kw = dict(x=_ptr(x), x_bstride=xbs, ldx=ldx, pre_tanh=int(pre_tanh), y=_ptr(y), y_bstride=ybs, ldy=ldy, B=B, T=T, C=C, pad=pad)
    if gate is not None:
        assert gate.dtype == torch.float32 and gate.shape == (B, C) and gate.stride(1) == 1
        kw.update(gate=_ptr(gate), gate_ld=gate.stride(0))
    if res is not None:
        Br, Tr, Cr, rbs, ldr = _nlc(res)
        assert (Br, Tr, Cr) == (B, T, C)
        kw.update(res=_ptr(res), res_bstride=rbs, ldr=ldr)
    _lib.call_struct("mi355_ecapa_rows", "mi355_ecapa_rows_args", _stream(), **kw)
    return y


def time_moments(x: torch.Tensor, eps: float = 0.0, want_std: bool = True):
    """(mean [B, C], sqrt(biased variance + eps) [B, C] or None) over the time axis of ``x`` [B, T, C]."""
    B, T, C, xbs, ldx = _nlc(x)
    mean = torch.empty((B, C), dtype=torch.float32, device=x.device)
    std = torch.empty((B, C), dtype=torch.float32, device=x.device) if want_std else None
    _lib.call_struct("mi355_time_moments", "mi355_time_moments_args", _stream(), x=_ptr(x), x_bstride=xbs, ldx=ldx, B=B, T=T, C=C, eps=eps,
                     mean=_ptr(mean), std=_ptr(std), out_ld=C)
    return mean, std


def attentive_pool(x: torch.Tensor, logits: torch.Tensor, eps: float = 1e-12) -> torch.Tensor:
    """Softmax over time of ``logits`` per channel; [B, 2C] = (weighted mean | sqrt(max(weighted variance, eps))) of ``x`` -- mi355_attentive_pool_args."""
    B, T, C, xbs, ldx = _nlc(x)
    Bl, Tl, Cl, lbs, ldl = _nlc(logits)
    assert (Bl, Tl, Cl) == (B, T, C)
    out = torch.empty((B, 2 * C), dtype=torch.float32, device=x.device)
    _lib.call_struct("mi355_attentive_pool", "mi355_attentive_pool_args", _stream(), x=_ptr(x), x_bstride=xbs, ldx=ldx, logits=_ptr(logits), l_bstride=lbs,
                     ldl=ldl, B=B, T=T, C=C, eps=eps, out=_ptr(out), out_ld=2 * C)
    return out


def fake_quant_extrema(x: torch.Tensor, *, lens=None, pre=None, pre_act: int = ACT_NONE, pre_slope: float = 0.0,
                       pre_alpha: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Extrema pass alone: ``[B, 2]`` = {-min, max} of ``act(scale * x + shift)`` per utterance (joined with 0) for ``conv_gemm(pre_fq=...)``,
    which quantises inside its prologue -- the quantised tensor is never written."""
    B, L, C, xbs, ldx = _nlc(x)
    mm = torch.empty((B, 2), dtype=torch.float32, device=x.device)
    sc, sh = pre if pre is not None else (None, None)
    _lib.call_struct("mi355_fake_quant_extrema", "mi355_fake_quant_args", _stream(), x=_ptr(x), x_bstride=xbs, ldx=ldx, C=C, L=L, lens=_ptr(lens), B=B,
                     pre_scale=_ptr(sc), pre_shift=_ptr(sh), pre_ld=sc.stride(0) if sc is not None else 0, pre_act=pre_act, pre_slope=pre_slope,
                     pre_alpha=_ptr(pre_alpha), minmax=_ptr(mm))
    return mm


def attention(qkv: torch.Tensor, heads: int, dh: int, out: torch.Tensor, lens=None):
    B, T, _, bs, ld = _nlc(qkv)
    _, _, _, obs, ldo = _nlc(out)
    _lib.call_struct("mi355_attention", "mi355_attention_args", _stream(), qkv=_ptr(qkv), bstride=bs, ld=ld, heads=heads,
                     dh=dh, T=T, lens=_ptr(lens), B=B, out=_ptr(out), out_bstride=obs, ldo=ldo)
    return out


_SPLIT_WS = {}  # (device index, stream) -> (float workspace, zeroed int32 tickets) of the key-split decode attention


def attn_split_workspace(device, n_records: int, dh: int):
    """Persistent workspace for mi355_flash_attn_args.split_ws / split_cnt: ``n_records`` = B * heads * Tq.  The tickets must be zero before
    the first launch and every launch leaves them zero, so one allocation per (device, stream) serves all calls."""
    key = (torch.device(device).index or 0, _stream())
    need_ws, need_cnt = n_records * 8 * (dh + 2), n_records
    cur = _SPLIT_WS.get(key)
    if cur is None or cur[0].numel() < need_ws or cur[1].numel() < need_cnt:
        cur = (torch.empty(max(need_ws, 1 << 16), dtype=torch.float32, device=device),
               torch.zeros(max(need_cnt, 1 << 10), dtype=torch.int32, device=device))
        _SPLIT_WS[key] = cur
    return cur


KV_DTYPES = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}  # MI355_KV_F32 / MI355_KV_BF16 / MI355_KV_F16


def kv_head_major16(kv: torch.Tensor, groups: int, heads: int, dh: int, dtype: torch.dtype) -> torch.Tensor:
    """float32 ``kv[B, T, >= groups * heads * dh]`` (k | v projection rows) -> ``[groups, B, heads, T, dh]`` in ``dtype`` (float16 / bfloat16): the head-major 16-bit
    blocks the decode-step attention streams, in one pass (``mi355_kv_head_major16``)."""
    B, T, C, bs, ld = _nlc(kv)
    assert C >= groups * heads * dh and dtype in (torch.float16, torch.bfloat16)
    out = torch.empty((groups, B, heads, T, dh), dtype=dtype, device=kv.device)
    lib = _lib.load()
    _lib.check(lib.mi355_kv_head_major16(_ptr(kv), bs, ld, B, T, groups, heads, dh, _ptr(out), KV_DTYPES[dtype], _stream()), "mi355_kv_head_major16")
    return out


def flash_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, out: torch.Tensor, *, heads: int, kv_heads: Optional[int] = None,
                    dh: int, scale: Optional[float] = None, causal: bool = False, window: int = 0, lens_q=None, lens_k=None,
                    mode: int = 0, k_start=None, head_major: bool = False, nsplit: int = 0, fused: Optional[dict] = None):
    """softmax(scale * q k^T + visibility) v.  q/out [B, Tq, >= heads*dh], k/v [B, Tk, >= kv_heads*dh] channels-last views
    (a KV cache is just the buffer k / v point into); see mi355_flash_attn_args for the visibility rule.
    ``fused`` (single-query decode step): dict(new_k, new_v [B, kv_heads * dh] raw projections of the new position, q_norm_w, k_norm_w, eps,
    cos, sin [rows, dh / 2], rope_mode, pos) -- q / k norms, rotary embedding and the cache store of row Tk - 1 happen inside the attention kernel."""
    B, Tq, _, qbs, ldq = _nlc(q)
    _, To, _, obs, ldo = _nlc(out)
    khs = vhs = 0
    if head_major:  # k / v [B, kv_heads, Tk, dh]: a head's keys contiguous (the layout for long key ranges: one L2 channel sweep per head)
        assert k.dim() == 4 and v.dim() == 4 and k.stride(3) == 1 and v.stride(3) == 1 and k.shape == v.shape
        Bk, _, Tk, _ = k.shape
        Tv, kbs, khs, ldk, vbs, vhs, ldv = Tk, k.stride(0), k.stride(1), k.stride(2), v.stride(0), v.stride(1), v.stride(2)
    else:
        assert k.dim() == 3 and v.dim() == 3 and k.stride(2) == 1 and v.stride(2) == 1 and k.is_cuda and v.is_cuda
        Bk, Tk, kbs, ldk = k.shape[0], k.shape[1], k.stride(0), k.stride(1)
        Tv, vbs, ldv = v.shape[1], v.stride(0), v.stride(1)
    assert Bk == B and Tv == Tk and To == Tq
    assert k.dtype == v.dtype and k.dtype in KV_DTYPES, "k / v must both be float32, bfloat16 or float16"
    fkw = {}
    if fused is not None:
        nk, nv = fused["new_k"], fused["new_v"]
        assert nk.dim() == 2 and nv.dim() == 2 and nk.stride(1) == 1 and nv.stride(1) == 1 and nk.stride(0) == nv.stride(0) and nk.dtype == torch.float32
        cos, sin = fused.get("cos"), fused.get("sin")
        fkw = dict(new_k=_ptr(nk), new_v=_ptr(nv), new_bstride=nk.stride(0), q_norm_w=_ptr(fused.get("q_norm_w")), k_norm_w=_ptr(fused.get("k_norm_w")),
                   norm_eps=fused.get("eps", 1e-6), rope_cos=_ptr(cos), rope_sin=_ptr(sin), rope_rows=0 if cos is None else cos.shape[0],
                   rope_mode=fused.get("rope_mode", 0), rope_pos=fused.get("pos", Tk - 1))
    sws = scnt = None
    if nsplit > 1 and Tq <= 8 and mode != 1:
        sws, scnt = attn_split_workspace(q.device, B * heads * Tq, dh)  # key-split decode (flash-decoding), opt-in: measured slower than the unsplit kernel
    _lib.call_struct("mi355_flash_attention", "mi355_flash_attn_args", _stream(), q=_ptr(q), q_bstride=qbs, ldq=ldq, k=_ptr(k),
                     k_bstride=kbs, ldk=ldk, v=_ptr(v), v_bstride=vbs, ldv=ldv, heads=heads, kv_heads=kv_heads or heads, dh=dh,
                     Tq=Tq, Tk=Tk, lens_q=_ptr(lens_q), lens_k=_ptr(lens_k), causal=int(causal), window=window,
                     scale=(1.0 / math.sqrt(dh)) if scale is None else scale, B=B, mode=mode, out=_ptr(out), out_bstride=obs, ldo=ldo,
                     k_start=_ptr(k_start), k_hstride=khs, v_hstride=vhs, split_ws=_ptr(sws), split_cnt=_ptr(scnt), nsplit=nsplit,
                     kv_dtype=KV_DTYPES[k.dtype], **fkw)
    return out


def whisper_greedy_step(logits: torch.Tensor, tokens: torch.Tensor, n: int, sample_begin: int, sum_logprobs: torch.Tensor, *,
                        V: Optional[int] = None, suppress_mask=None, blank_ids=None, timestamp_rules: bool = False,
                        timestamp_begin: int = 0, eot: int = 0, no_timestamps: int = -1, max_initial_timestamp_index: int = -1,
                        gumbel=None, temperature: float = 0.0, filtered=None, forced_next=None, split_ws=None):
    """One decode step of decoding.py's filter chain + GreedyDecoder.update, in place on ``tokens[:, n]`` / ``sum_logprobs``."""
    assert logits.dim() == 2 and logits.stride(1) == 1 and logits.dtype == torch.float32
    assert tokens.dtype == torch.int32 and tokens.dim() == 2 and tokens.stride(1) == 1
    B = logits.shape[0]
    _lib.call_struct("mi355_whisper_greedy_step", "mi355_whisper_step_args", _stream(), logits=_ptr(logits), ld=logits.stride(0),
                     V=V or logits.shape[1], B=B, tokens=_ptr(tokens), tokens_ld=tokens.stride(0), n=n, sample_begin=sample_begin,
                     suppress_mask=_ptr(suppress_mask), blank_ids=_ptr(blank_ids), n_blank=0 if blank_ids is None else blank_ids.numel(),
                     timestamp_rules=int(timestamp_rules), timestamp_begin=timestamp_begin, eot=eot, no_timestamps=no_timestamps,
                     max_initial_timestamp_index=max_initial_timestamp_index, gumbel=_ptr(gumbel), temperature=temperature,
                     sum_logprobs=_ptr(sum_logprobs), filtered=_ptr(filtered), forced_next=_ptr(forced_next),
                     split_ws=None if split_ws is None else _ptr(split_ws[0]), split_cnt=None if split_ws is None else _ptr(split_ws[1]))


def whisper_step_workspace(device, B: int):
    """(float32 [B * 16 * 12], int32 [B] zeroed): the scratch of the multi-workgroup decode-rules step (mi355_whisper_step_args.split_ws / split_cnt)."""
    return (torch.empty(B * 16 * 12, dtype=torch.float32, device=device), torch.zeros(B, dtype=torch.int32, device=device))


def softmax_prob_at(logits: torch.Tensor, token: int, V: Optional[int] = None) -> torch.Tensor:
    assert logits.dim() == 2 and logits.stride(1) == 1 and logits.dtype == torch.float32
    out = torch.empty((logits.shape[0],), dtype=torch.float32, device=logits.device)
    lib = _lib.load()
    rc = lib.mi355_softmax_prob_at(_ptr(logits), logits.stride(0), V or logits.shape[1], logits.shape[0], token, _ptr(out), _stream())
    _lib.check(rc, "mi355_softmax_prob_at")
    return out


# --------------------------------------------------------------------------------------- Whisper word-level timestamps (align.hip)
def softmax_prob_rows(logits: torch.Tensor, tokens: torch.Tensor, V: Optional[int] = None) -> torch.Tensor:
    """out[r] = softmax(logits[r, :V])[tokens[r]] (timing.py:135-139): the per-row sibling of ``softmax_prob_at``."""
    assert logits.dim() == 2 and logits.stride(1) == 1 and logits.dtype == torch.float32
    assert tokens.dtype == torch.int32 and tokens.dim() == 1 and tokens.is_contiguous() and tokens.numel() == logits.shape[0]
    out = torch.empty((logits.shape[0],), dtype=torch.float32, device=logits.device)
    lib = _lib.load()
    rc = lib.mi355_softmax_prob_rows(_ptr(logits), logits.stride(0), V or logits.shape[1], logits.shape[0], _ptr(tokens), _ptr(out), _stream())
    _lib.check(rc, "mi355_softmax_prob_rows")
    return out


def align_qk_softmax(q: torch.Tensor, k: torch.Tensor, w: torch.Tensor, pairs: torch.Tensor, *, heads: int, dh: int, scale: Optional[float] = None,
                     qk_scale: float = 1.0, lens_t=None, lens_f=None, head_major: bool = False, F: Optional[int] = None) -> torch.Tensor:
    """w[b, slot, t, f] = softmax_f(qk_scale * scale * q[b, t, head] . k[b, f, head]) for the ``pairs`` [n, 2] = (head, slot) of one decoder
    layer (a host list, range-checked here, or an int32 device tensor the CALLER has checked: the kernel trusts it).  q [B, T, >= heads * dh] float32; k rows [B, Tk, >= heads * dh] or head-major [B, heads, Tk, dh] (float32 / bfloat16 / float16) as
    ``flash_attention`` takes them; w float32 [B, A, Tmax, Fmax] (last stride 1).  Keys 0 .. F (default: all Tk), cut per item by ``lens_f``."""
    B, T, _, qbs, ldq = _nlc(q)
    khs = 0
    if head_major:
        assert k.dim() == 4 and k.stride(3) == 1
        Tk, kbs, khs, ldk = k.shape[2], k.stride(0), k.stride(1), k.stride(2)
    else:
        assert k.dim() == 3 and k.stride(2) == 1
        Tk, kbs, ldk = k.shape[1], k.stride(0), k.stride(1)
    assert k.is_cuda and k.shape[0] == B and k.dtype in KV_DTYPES
    assert w.dim() == 4 and w.dtype == torch.float32 and w.is_cuda and w.stride(3) == 1 and w.shape[0] == B
    if not isinstance(pairs, torch.Tensor):   # a host list is checked here: the device validates neither the heads nor the slots
        assert len(pairs) > 0 and all(0 <= int(h) < heads and 0 <= int(sl) < w.shape[1] for h, sl in pairs), "align_qk_softmax: (head, slot) out of range"
        pairs = torch.tensor([[int(h), int(sl)] for h, sl in pairs], dtype=torch.int32, device=q.device)
    assert pairs.dtype == torch.int32 and pairs.dim() == 2 and pairs.shape[1] == 2 and pairs.is_contiguous() and pairs.is_cuda
    F = Tk if F is None else F
    assert 0 < F <= Tk and T <= w.shape[2] and F <= w.shape[3]
    _lib.call_struct("mi355_align_qk_softmax", "mi355_align_qk_args", _stream(), q=_ptr(q), q_bstride=qbs, ldq=ldq, k=_ptr(k), k_bstride=kbs,
                     k_hstride=khs, ldk=ldk, kv_dtype=KV_DTYPES[k.dtype], dh=dh, B=B, T=T, F=F, lens_t=_ptr(lens_t), lens_f=_ptr(lens_f),
                     pairs=_ptr(pairs), n_pairs=pairs.shape[0], heads=heads, scale=(1.0 / math.sqrt(dh)) if scale is None else scale,
                     qk_scale=qk_scale, w=_ptr(w), w_bstride=w.stride(0), w_astride=w.stride(1), ldw=w.stride(2), A=w.shape[1])
    return w


def align_matrix(w: torch.Tensor, out: torch.Tensor, *, T: Optional[int] = None, F: Optional[int] = None, lens_t=None, lens_f=None,
                 medfilt_width: int = 7, standardize: bool = True, negate: bool = True, row_begin: int = 0, row_trim: int = 1,
                 stats: Optional[torch.Tensor] = None) -> torch.Tensor:
    """timing.py:148-154 on w [B, A, T, F]: standardise over the tokens, median filter over the frames (reflect padding), mean over the A heads;
    out[b, n, f] = -(that) for the token rows ``row_begin <= t < lens_t[b] - row_trim``.  ``standardize=False, negate=False, row_trim=0`` on one head
    is the plain median filter."""
    assert w.dim() == 4 and w.dtype == torch.float32 and w.is_cuda and w.stride(3) == 1
    assert out.dim() == 3 and out.dtype == torch.float32 and out.is_cuda and out.stride(2) == 1 and out.shape[0] == w.shape[0]
    B, A = w.shape[0], w.shape[1]
    T = w.shape[2] if T is None else T
    F = w.shape[3] if F is None else F
    assert T <= w.shape[2] and F <= w.shape[3] and F <= out.shape[2] and T - row_trim - row_begin <= out.shape[1]
    if standardize and stats is None:
        stats = torch.empty(B * A * F * 2, dtype=torch.float32, device=w.device)
    _lib.call_struct("mi355_align_matrix", "mi355_align_matrix_args", _stream(), w=_ptr(w), w_bstride=w.stride(0), w_astride=w.stride(1), ldw=w.stride(2),
                     A=A, B=B, T=T, F=F, lens_t=_ptr(lens_t), lens_f=_ptr(lens_f), medfilt_width=medfilt_width, standardize=int(standardize),
                     negate=int(negate), row_begin=row_begin, row_trim=row_trim, stats=_ptr(stats), out=_ptr(out), out_bstride=out.stride(0),
                     ldo=out.stride(1))
    return out


def dtw_workspace_bytes(N: int, M: int, B: int) -> int:
    return int(_lib.load().mi355_dtw_ws_bytes(N, M, B))


def dtw(cost: torch.Tensor, *, N: Optional[int] = None, M: Optional[int] = None, lens_n=None, lens_m=None, ws: Optional[torch.Tensor] = None):
    """timing.py:52-99 on cost [B, N, M] float32 (per-item sizes ``lens_n`` / ``lens_m``): (text_idx, time_idx int32 [B, N + M], path_len int32 [B]),
    the warping path in forward order -- given the same float32 input, the reference's path bit for bit.  N <= 1024."""
    assert cost.dim() == 3 and cost.dtype == torch.float32 and cost.is_cuda and cost.stride(2) == 1
    B = cost.shape[0]
    N = cost.shape[1] if N is None else N
    M = cost.shape[2] if M is None else M
    assert N <= cost.shape[1] and M <= cost.shape[2]
    cap = N + M
    text = torch.empty((B, cap), dtype=torch.int32, device=cost.device)
    time = torch.empty((B, cap), dtype=torch.int32, device=cost.device)
    plen = torch.zeros((B,), dtype=torch.int32, device=cost.device)
    need = dtw_workspace_bytes(N, M, B)
    if ws is None or ws.numel() * ws.element_size() < need:
        ws = torch.empty(max(need, 16), dtype=torch.uint8, device=cost.device)
    _lib.call_struct("mi355_dtw", "mi355_dtw_args", _stream(), cost=_ptr(cost), cost_bstride=cost.stride(0), ldc=cost.stride(1), B=B, N=N, M=M,
                     lens_n=_ptr(lens_n), lens_m=_ptr(lens_m), text_idx=_ptr(text), time_idx=_ptr(time), path_cap=cap, path_len=_ptr(plen),
                     ws=_ptr(ws), ws_bytes=ws.numel() * ws.element_size())
    return text, time, plen


def rmsnorm(x: torch.Tensor, y: torch.Tensor, weight: Optional[torch.Tensor], eps: float = 1e-6, lens=None):
    B, L, C, xbs, ldx = _nlc(x)
    _, _, _, ybs, ldy = _nlc(y)
    _lib.call_struct("mi355_rmsnorm", "mi355_rmsnorm_args", _stream(), x=_ptr(x), x_bstride=xbs, ldx=ldx, C=C, L=L, lens=_ptr(lens), B=B,
                     weight=_ptr(weight), eps=eps, y=_ptr(y), y_bstride=ybs, ldy=ldy)
    return y


def head_norm_rope(x: torch.Tensor, y: torch.Tensor, *, heads: int, dh: int, norm_weight: Optional[torch.Tensor] = None, eps: float = 1e-6,
                   cos: Optional[torch.Tensor] = None, sin: Optional[torch.Tensor] = None, pos: Optional[torch.Tensor] = None, pos0: int = 0,
                   interleaved: bool = False, lens=None, second: Optional[tuple] = None, pos_sub: Optional[torch.Tensor] = None):
    """Per-head RMSNorm (optional) + RoPE (optional) of ``heads`` heads starting at column 0 of ``x`` into ``y`` (may be a cache slot).
    ``pos_sub`` int32 [B]: left padding of each row, subtracted from its positions (its first real token is position 0)."""
    B, L, _, xbs, ldx = _nlc(x)
    _, _, _, ybs, ldy = _nlc(y)
    if cos is not None:
        assert cos.dim() == 2 and cos.shape[1] == dh // 2 and cos.is_contiguous() and sin.is_contiguous() and cos.shape == sin.shape
    if pos is not None:
        assert pos.dtype == torch.int32 and pos.dim() == 2 and pos.stride(1) == 1
    elif cos is not None and pos0 + L > cos.shape[0]:
        raise ValueError(f"head_norm_rope: positions {pos0}..{pos0 + L - 1} run past the {cos.shape[0]}-row rotary tables")
    kw = {}
    if second is not None:  # (x2, y2, heads2, norm_weight2): e.g. the k heads, rotated straight into their KV-cache slot
        x2, y2, heads2, nw2 = second
        B2, L2, _, x2bs, ldx2 = _nlc(x2)
        _, _, _, y2bs, ldy2 = _nlc(y2)
        assert B2 == B and L2 == L
        kw = dict(x2=_ptr(x2), x2_bstride=x2bs, ldx2=ldx2, heads2=heads2, norm_weight2=_ptr(nw2), y2=_ptr(y2), y2_bstride=y2bs, ldy2=ldy2)
    _lib.call_struct("mi355_head_norm_rope", "mi355_head_rope_args", _stream(), x=_ptr(x), x_bstride=xbs, ldx=ldx, heads=heads, dh=dh, L=L,
                     lens=_ptr(lens), B=B, norm_weight=_ptr(norm_weight), eps=eps, cos_table=_ptr(cos), sin_table=_ptr(sin), pos=_ptr(pos),
                     pos_ld=0 if pos is None else pos.stride(0), pos0=pos0, pos_sub=_ptr(pos_sub), rope_rows=0 if cos is None else cos.shape[0],
                     rope_mode=int(interleaved), y=_ptr(y), y_bstride=ybs, ldy=ldy, **kw)
    return y


def swiglu(x: torch.Tensor, y: torch.Tensor):
    """y[..., i] = silu(x[..., 2i]) * x[..., 2i+1] on contiguous-row 3-D views [B, L, 2I] -> [B, L, I] (both dense over B, L)."""
    B, L, C2, xbs, ldx = _nlc(x)
    _, _, I, ybs, ldy = _nlc(y)
    assert C2 == 2 * I and xbs == L * ldx and ybs == L * ldy
    lib = _lib.load()
    rc = lib.mi355_swiglu(_ptr(x), ldx, _ptr(y), ldy, B * L, I, _stream())
    _lib.check(rc, "mi355_swiglu")
    return y


def embed_sum(table: torch.Tensor, ids: torch.Tensor, y: torch.Tensor, *, slot_offset: Optional[torch.Tensor] = None,
              add: Optional[torch.Tensor] = None, scale: float = 1.0, lens=None):
    """y[b, l] = scale * (add[b, l] + sum_q table[slot_offset[q] + ids[b, l, q]]); ``ids`` int32 [B, L, Q] (any strides)."""
    B, L, C, ybs, ldy = _nlc(y)
    assert ids.dtype == torch.int32 and ids.dim() == 3 and ids.shape[0] == B and ids.shape[1] == L
    assert table.dim() == 2 and table.stride(1) == 1 and table.dtype == torch.float32
    kw = dict(table=_ptr(table), ld_table=table.stride(0), slot_offset=_ptr(slot_offset), ids=_ptr(ids), ids_bstride=ids.stride(0),
              ids_ld=ids.stride(1), ids_qstride=ids.stride(2), Q=ids.shape[2], scale=scale, C=C, L=L, lens=_ptr(lens), B=B, y=_ptr(y),
              y_bstride=ybs, ldy=ldy)
    if add is not None:
        _, _, _, abs_, ald = _nlc(add)
        kw.update(add=_ptr(add), add_bstride=abs_, add_ld=ald)
    _lib.call_struct("mi355_embed_sum", "mi355_embed_sum_args", _stream(), **kw)
    return y


def dwconv(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], y: torch.Tensor, *, pad: int = 0, stride: int = 1,
           transpose: bool = False, lens_in=None, dil: int = 1, pre_alpha: Optional[torch.Tensor] = None, pre_inv: Optional[torch.Tensor] = None):
    """Depthwise conv / conv_transpose, channels-last; ``w`` [C, K] float32.  ``dil`` and the per-channel Snake prologue
    (``pre_alpha``, ``pre_inv`` = 1 / (alpha + 1e-9), each [>= C]) apply to the plain conv."""
    B, Lin, C, xbs, ldx = _nlc(x)
    _, Lout, _, ybs, ldy = _nlc(y)
    assert w.dim() == 2 and w.shape[0] == C and w.is_contiguous() and w.dtype == torch.float32
    _lib.call_struct("mi355_dwconv", "mi355_dwconv_args", _stream(), x=_ptr(x), x_bstride=xbs, ldx=ldx, Lin=Lin, lens_in=_ptr(lens_in),
                     w=_ptr(w), bias=_ptr(bias), C=C, K=w.shape[1], pad=pad, stride=stride, transpose=int(transpose), B=B, y=_ptr(y),
                     y_bstride=ybs, ldy=ldy, Lout=Lout, dil=dil, pre_alpha=_ptr(pre_alpha), pre_inv=_ptr(pre_inv))
    return y


FSMN_MAX_TAPS = 31  # MI355_FSMN_MAX_TAPS
FSQ_SCALE = 0.9990000128746033  # FSQCodebook.encode (codec/models/s3/model_v2.py:89)


def fsmn_memory(v: torch.Tensor, w: torch.Tensor, y: torch.Tensor, *, add: Optional[torch.Tensor] = None, lens: Optional[torch.Tensor] = None):
    """``y[b, t] = add[b, t] + m(b, t) * (sum_j w[:, j] * m(b, t + j - left) * v[b, t + j - left] + v[b, t])`` (``mi355_fsmn_memory``): the FSMN memory
    block of the S3 tokenizer's attention.  ``v`` / ``add`` / ``y`` channels-last views [B, L, C] (``v`` may be a third of a fused q|k|v buffer), ``w``
    [C, K] float32 as ``dwconv`` takes it (K odd, <= ``FSMN_MAX_TAPS``), ``lens`` int32 [B].  ``y`` must not alias ``v``."""
    B, L, C, vbs, ldv = _nlc(v)
    By, Ly, Cy, ybs, ldy = _nlc(y)
    assert (By, Ly, Cy) == (B, L, C)
    assert w.dim() == 2 and w.shape[0] == C and w.is_contiguous() and w.dtype == torch.float32
    kw = dict(v=_ptr(v), v_bstride=vbs, ldv=ldv, w=_ptr(w), K=w.shape[1], C=C, L=L, lens=_ptr(lens), B=B, y=_ptr(y), y_bstride=ybs, ldy=ldy)
    if lens is not None:
        assert lens.dtype == torch.int32 and lens.numel() == B and lens.is_contiguous()
    if add is not None:
        Ba, La, Ca, abs_, ald = _nlc(add)
        assert (Ba, La, Ca) == (B, L, C)
        kw.update(add=_ptr(add), add_bstride=abs_, add_ld=ald)
    _lib.call_struct("mi355_fsmn_memory", "mi355_fsmn_memory_args", _stream(), **kw)
    return y


def fsq_encode(x: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor], *, lens: Optional[torch.Tensor] = None, return_h: bool = False):
    """FSQ codes of ``x`` [B, L, C] (rows contiguous over B and L) or [rows, C]: int32 ``sum_d (rint(tanh(h_d) * FSQ_SCALE) + 1) * 3^d`` with
    ``h = x w^T + b``, ``w`` [8, C], ``b`` [8] (``mi355_fsq_encode``); zero at and beyond ``lens[b]``.  ``return_h`` adds the pre-activations [..., 8]."""
    assert x.dtype == torch.float32 and x.is_cuda and x.stride(-1) == 1
    if x.dim() == 3:
        assert x.stride(0) == x.shape[1] * x.stride(1), "fsq_encode: the rows of a batch must be evenly spaced"
        lead, L, ldx = (x.shape[0], x.shape[1]), x.shape[1], x.stride(1)
    else:
        assert x.dim() == 2 and lens is None
        lead, L, ldx = (x.shape[0],), 0, x.stride(0)
    C = x.shape[-1]
    rows = int(np.prod(lead))
    assert w.shape == (8, C) and w.is_contiguous() and w.dtype == torch.float32 and (b is None or (b.numel() == 8 and b.is_contiguous() and b.dtype == torch.float32))
    if lens is not None:
        assert lens.dtype == torch.int32 and lens.numel() == lead[0] and lens.is_contiguous()
    codes = torch.empty(lead, dtype=torch.int32, device=x.device)
    h = torch.empty(lead + (8,), dtype=torch.float32, device=x.device) if return_h else None
    _lib.call_struct("mi355_fsq_encode", "mi355_fsq_encode_args", _stream(), x=_ptr(x), ldx=ldx, rows=rows, C=C, w=_ptr(w), b=_ptr(b), lens=_ptr(lens), L=L,
                     codes=_ptr(codes), h=_ptr(h))
    return (codes, h) if return_h else codes


GLU_DWCONV_MAX_TAPS = 31  # MI355_GLU_DWCONV_MAX_TAPS


def _lens_arg(lens: Optional[torch.Tensor], B: int):
    if lens is not None:
        assert lens.dtype == torch.int32 and lens.numel() == B and lens.is_contiguous() and lens.is_cuda
    return _ptr(lens)


def relpos_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, p: torch.Tensor, bias_u: torch.Tensor, bias_v: torch.Tensor, out: torch.Tensor, *,
                     heads: int, dh: int, center: int, scale: Optional[float] = None, lens: Optional[torch.Tensor] = None):
    """``out_i = sum_j softmax_j(scale ((q_i + u) . k_j + (q_i + v) . p[center - (i - j)])) v_j`` over ``j < lens[b]`` (``mi355_relpos_attention``):
    the Conformer's relative-position attention behind its projections.  ``q`` / ``k`` / ``v`` / ``out`` channels-last views [B, T, heads * dh]
    (thirds of a fused buffer or contiguous), ``p`` the projected position table [P, heads * dh] whose row ``center`` is distance 0, ``bias_u`` /
    ``bias_v`` [heads * dh].  Rows at and beyond ``lens[b]`` come back zero.  The table must hold the distances -(T - 1) .. T - 1."""
    B, T, C, qbs, ldq = _nlc(q)
    Bk, Tk, Ck, kbs, ldk = _nlc(k)
    Bv, Tv, Cv, vbs, ldv = _nlc(v)
    Bo, To, Co, obs, ldo = _nlc(out)
    hd = heads * dh
    assert (Bk, Tk) == (B, T) and (Bv, Tv) == (B, T) and (Bo, To) == (B, T) and min(C, Ck, Cv, Co) >= hd
    assert p.dim() == 2 and p.stride(1) == 1 and p.shape[1] >= hd and p.dtype == torch.float32 and p.is_cuda
    for t in (bias_u, bias_v):
        assert t.dtype == torch.float32 and t.numel() == hd and t.is_contiguous() and t.is_cuda
    _lib.call_struct("mi355_relpos_attention", "mi355_relpos_attention_args", _stream(), q=_ptr(q), q_bstride=qbs, ldq=ldq, k=_ptr(k), k_bstride=kbs,
                     ldk=ldk, v=_ptr(v), v_bstride=vbs, ldv=ldv, p=_ptr(p), ldp=p.stride(0), P=p.shape[0], center=center, bias_u=_ptr(bias_u),
                     bias_v=_ptr(bias_v), lens=_lens_arg(lens, B), B=B, T=T, heads=heads, dh=dh, scale=dh ** -0.5 if scale is None else scale,
                     out=_ptr(out), out_bstride=obs, ldo=ldo)
    return out


NARROW_ATTENTION_WIDTHS = (8, 16, 24, 32)


def narrow_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, out: torch.Tensor, *, heads: int, dh: int, scale: Optional[float] = None,
                     lens: Optional[torch.Tensor] = None, check_lens: bool = True):
    """``out_i = sum_j softmax_j(scale q_i . k_j) v_j`` over ``j < lens[b]`` (``mi355_narrow_attention``): attention for heads of 8 / 16 / 24 / 32
    at any T (Sortformer's Transformer encoder: 8 heads of 24).  ``q`` / ``k`` / ``v`` / ``out`` channels-last views [B, T, heads * dh] (thirds of
    a fused buffer or contiguous).  Rows at and beyond ``lens[b]`` come back zero; every ``lens[b]`` must be in ``[1, T]``: checked here with one
    device read of ``lens``, which a caller that built ``lens`` from host integers it has already checked turns off (``check_lens=False``)."""
    B, T, C, qbs, ldq = _nlc(q)
    Bk, Tk, Ck, kbs, ldk = _nlc(k)
    Bv, Tv, Cv, vbs, ldv = _nlc(v)
    Bo, To, Co, obs, ldo = _nlc(out)
    hd = heads * dh
    assert (Bk, Tk) == (B, T) and (Bv, Tv) == (B, T) and (Bo, To) == (B, T) and min(C, Ck, Cv, Co) >= hd
    lp = _lens_arg(lens, B)
    if lens is not None and check_lens:
        lo, hi = int(lens.min()), int(lens.max())
        if lo < 1 or hi > T:
            raise _lib.Mi355Error(f"narrow_attention: lens must lie in [1, T = {T}] (got min {lo}, max {hi})")
    _lib.call_struct("mi355_narrow_attention", "mi355_narrow_attention_args", _stream(), q=_ptr(q), q_bstride=qbs, ldq=ldq, k=_ptr(k), k_bstride=kbs,
                     ldk=ldk, v=_ptr(v), v_bstride=vbs, ldv=ldv, lens=lp, B=B, T=T, heads=heads, dh=dh, scale=dh ** -0.5 if scale is None else scale,
                     out=_ptr(out), out_bstride=obs, ldo=ldo)
    return out


MID_ATTENTION_WIDTHS = (36, 40, 44, 48, 52, 56, 60)
MID_ATTENTION_FEW_TQ = 4   # Tq up to here runs one wavefront per (query, head, item): the decode step


def mid_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, out: torch.Tensor, *, heads: int, dh: int, kv_heads: Optional[int] = None,
                  scale: Optional[float] = None, causal: bool = False, lens_q: Optional[torch.Tensor] = None, lens_k: Optional[torch.Tensor] = None,
                  check_lens: bool = True):
    """``out_i = sum_j softmax_j(scale q_i . k_j) v_j`` over the visible keys (``mi355_mid_attention``): attention for heads of 36 - 60 (Moonshine:
    8 x 36 and 8 x 52), self or cross (``Tq != Tk``), grouped kv heads, optional causal form.  ``q`` / ``out`` channels-last views
    [B, Tq, >= heads * dh], ``k`` / ``v`` [B, Tk, >= kv_heads * dh] (thirds of a fused buffer, a cache slice, or contiguous).  Key ``j`` is visible
    iff ``j < lens_k[b]`` and, under ``causal``, ``j <= i + (lens_k[b] - lens_q[b])``.  Rows at and beyond ``lens_q[b]`` come back zero; ``lens_q`` is not checked: the kernel clamps it to ``[0, Tq]``.  Every
    ``lens_k[b]`` must be in ``[1, Tk]``: checked here with one device read, which a caller that built the lengths from host integers it has
    already checked turns off (``check_lens=False``)."""
    B, Tq, C, qbs, ldq = _nlc(q)
    Bk, Tk, Ck, kbs, ldk = _nlc(k)
    Bv, Tv, Cv, vbs, ldv = _nlc(v)
    Bo, To, Co, obs, ldo = _nlc(out)
    kvh = heads if kv_heads is None else kv_heads
    assert Bk == B and (Bv, Tv) == (B, Tk) and (Bo, To) == (B, Tq) and min(C, Co) >= heads * dh and min(Ck, Cv) >= kvh * dh
    if lens_k is not None and check_lens:
        _lens_arg(lens_k, B)
        lo, hi = int(lens_k.min()), int(lens_k.max())
        if lo < 1 or hi > Tk:
            raise _lib.Mi355Error(f"mid_attention: lens_k must lie in [1, Tk = {Tk}] (got min {lo}, max {hi})")
    _lib.call_struct("mi355_mid_attention", "mi355_mid_attention_args", _stream(), q=_ptr(q), q_bstride=qbs, ldq=ldq, k=_ptr(k), k_bstride=kbs, ldk=ldk,
                     v=_ptr(v), v_bstride=vbs, ldv=ldv, lens_q=_lens_arg(lens_q, B), lens_k=_lens_arg(lens_k, B), B=B, Tq=Tq, Tk=Tk, heads=heads,
                     kv_heads=kvh, dh=dh, causal=int(causal), scale=dh ** -0.5 if scale is None else scale, out=_ptr(out), out_bstride=obs, ldo=ldo)
    return out


def moonshine_rope_tables(rot: int, rows: int, *, base: float = 10000.0, pos0: int = 0, device=None):
    """(cos, sin) float32 [rows, rot / 2] for positions ``pos0 .. pos0 + rows - 1``, computed as the reference's rotary embedding computes them
    (moonshine.py:35-58): ``inv_freq = 1 / base ** (arange(0, rot, 2) / rot)`` in float32, ``float32(pos) * inv_freq``, then cos / sin in float32.
    As many rows as the call needs: ``max_position_embeddings`` bounds nothing in the reference."""
    assert rot >= 2 and rot % 2 == 0 and rows >= 1
    inv_freq = (np.float32(1.0) / np.power(np.float32(base), np.arange(0, rot, 2, dtype=np.float32) / np.float32(rot))).astype(np.float32)
    ang = np.arange(pos0, pos0 + rows, dtype=np.float32)[:, None] * inv_freq[None, :]
    cos, sin = torch.from_numpy(np.cos(ang).astype(np.float32)), torch.from_numpy(np.sin(ang).astype(np.float32))
    return (cos, sin) if device is None else (cos.to(device), sin.to(device))


def partial_rope(x: torch.Tensor, y: torch.Tensor, *, heads: int, dh: int, rot: int, cos: torch.Tensor, sin: torch.Tensor, pos0: int = 0,
                 lens: Optional[torch.Tensor] = None, second: Optional[tuple] = None):
    """Rotary embedding on the first ``rot`` channels of every head, interleaved pairs (``mi355_partial_rope``): ``x`` [B, L, >= heads * dh] into
    ``y`` (``y is x``: in place; or a cache slot); channels ``rot .. dh - 1`` are copied.  Row ``l`` takes row ``pos0 + l`` of the ``cos`` / ``sin``
    tables [rows, rot / 2] (``moonshine_rope_tables``); positions past the tables are refused.  ``second = (x2, y2, heads2)``: another operand (the
    k heads, into their cache row) in the same launch.  Rows at and beyond ``lens[b]`` are left untouched."""
    B, L, C, xbs, ldx = _nlc(x)
    By, Ly, Cy, ybs, ldy = _nlc(y)
    assert (By, Ly) == (B, L) and min(C, Cy) >= heads * dh
    assert cos.dim() == 2 and cos.shape == sin.shape and cos.shape[1] == rot // 2 and cos.is_contiguous() and sin.is_contiguous()
    assert cos.dtype == sin.dtype == torch.float32 and cos.is_cuda and sin.is_cuda
    kw = {}
    if second is not None:
        x2, y2, heads2 = second
        B2, L2, C2, x2bs, ldx2 = _nlc(x2)
        By2, Ly2, Cy2, y2bs, ldy2 = _nlc(y2)
        assert (B2, L2) == (B, L) and (By2, Ly2) == (B, L) and min(C2, Cy2) >= heads2 * dh
        kw = dict(x2=_ptr(x2), x2_bstride=x2bs, ldx2=ldx2, heads2=heads2, y2=_ptr(y2), y2_bstride=y2bs, ldy2=ldy2)
    _lib.call_struct("mi355_partial_rope", "mi355_partial_rope_args", _stream(), x=_ptr(x), x_bstride=xbs, ldx=ldx, heads=heads, y=_ptr(y),
                     y_bstride=ybs, ldy=ldy, dh=dh, rot=rot, B=B, L=L, pos0=pos0, rope_rows=cos.shape[0], lens=_lens_arg(lens, B),
                     cos_table=_ptr(cos), sin_table=_ptr(sin), **kw)
    return y


def glu_dwconv_silu(x: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor], y: torch.Tensor, *, lens: Optional[torch.Tensor] = None):
    """``silu(b + sum_k w[:, k] * g[t + k - (K - 1) / 2])`` with ``g = x[..., :C] * sigmoid(x[..., C:])`` (``mi355_glu_dwconv_silu``): the middle of the
    Conformer's convolution module, ``x`` [B, L, 2 C] -> ``y`` [B, L, C]; ``w`` [C, K] (K odd, <= ``GLU_DWCONV_MAX_TAPS``) and ``b`` [C] carry the
    depthwise bias and the folded BatchNorm.  ``g`` is zero outside ``[0, lens[b])`` and the rows of ``y`` at and beyond ``lens[b]`` are zero."""
    B, L, C2, xbs, ldx = _nlc(x)
    By, Ly, C, ybs, ldy = _nlc(y)
    assert (By, Ly) == (B, L) and C2 == 2 * C
    assert w.dim() == 2 and w.shape[0] == C and w.is_contiguous() and w.dtype == torch.float32 and (b is None or (b.numel() == C and b.is_contiguous() and b.dtype == torch.float32))
    _lib.call_struct("mi355_glu_dwconv_silu", "mi355_glu_dwconv_silu_args", _stream(), x=_ptr(x), x_bstride=xbs, ldx=ldx, w=_ptr(w), b=_ptr(b),
                     K=w.shape[1], C=C, L=L, lens=_lens_arg(lens, B), B=B, y=_ptr(y), y_bstride=ybs, ldy=ldy)
    return y


def stencil2d_out(n: int) -> int:
    """k = 3, stride 2, pad 1."""
    return (n - 1) // 2 + 1


def stencil2d_k3s2(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], y: torch.Tensor, *, relu: bool = False,
                   lens_in: Optional[torch.Tensor] = None, lens_out: Optional[torch.Tensor] = None):
    """3 x 3 / stride 2 / pad 1 over (time, frequency), channels-last (``mi355_stencil2d_k3s2``): ``x`` [B, T, F] (one input channel feeding every
    output channel) or [B, T, F, C] (depthwise), ``w`` [C, 3, 3], ``y`` [B, To, Fo, C].  Input rows at and beyond ``lens_in[b]`` read as zero, output
    rows at and beyond ``lens_out[b]`` are written as zero."""
    assert x.dtype == torch.float32 and x.is_cuda and y.dtype == torch.float32 and y.dim() == 4 and x.dim() in (3, 4)
    B, T, F = x.shape[:3]
    C = y.shape[3]
    assert x[0].is_contiguous() and y[0].is_contiguous() and (x.dim() == 3 or x.shape[3] == C)
    assert tuple(y.shape) == (B, stencil2d_out(T), stencil2d_out(F), C), (tuple(y.shape), tuple(x.shape))
    assert tuple(w.shape) == (C, 3, 3) and w.is_contiguous() and w.dtype == torch.float32 and (bias is None or (bias.numel() == C and bias.is_contiguous()))
    _lib.call_struct("mi355_stencil2d_k3s2", "mi355_stencil2d_k3s2_args", _stream(), x=_ptr(x), x_bstride=x.stride(0) if B > 1 else x[0].numel(), w=_ptr(w),
                     bias=_ptr(bias), B=B, T=T, F=F, C=C, in_cstride=int(x.dim() == 4), relu=int(relu), lens_in=_lens_arg(lens_in, B),
                     lens_out=_lens_arg(lens_out, B), y=_ptr(y), y_bstride=y.stride(0) if B > 1 else y[0].numel())
    return y


def sanm_rows(T: int, lfr_n: int) -> int:
    """Rows of ``sanm_input``'s output for ``T`` frames: the four query rows and ``ceil(T / lfr_n)`` stacked frames."""
    return 4 + (T + lfr_n - 1) // lfr_n


def sanm_input(feats: torch.Tensor, embed: torch.Tensor, qids: torch.Tensor, pe: Optional[torch.Tensor], *, lfr_m: int, lfr_n: int, scale: float,
               lens: Optional[torch.Tensor] = None, means: Optional[torch.Tensor] = None, istd: Optional[torch.Tensor] = None,
               x: Optional[torch.Tensor] = None):
    """SenseVoice's encoder input in one launch (``mi355_sanm_input``): ``feats`` [B, T, D] (the fbank; ``lens`` int32 [B], every one in [1, T]) ->
    ``(x [B, 4 + ceil(T / lfr_n), lfr_m * D], out_lens int32 [B])``.  Rows 0..3 are ``embed[qids[b]]`` (``embed`` [16, W], ``qids`` int32 [B, 4]), row
    ``4 + i`` the low-frame-rate stack of ``lfr_m`` frames at hop ``lfr_n`` (edge frames repeated, the right edge being the item's own last frame) after
    ``(. + means) * istd``; every valid row is ``row * scale + pe[row]`` (``pe`` [>= rows, W] or None) and the rows at and beyond ``out_lens[b]`` are zero."""
    B, T, D, fbs, ldf = _nlc(feats)
    W, rows = lfr_m * D, sanm_rows(T, lfr_n)
    f32 = lambda t, n: t.dtype == torch.float32 and t.is_cuda and t.is_contiguous() and t.numel() == n
    assert f32(embed, 16 * W) and qids.dtype == torch.int32 and qids.is_cuda and qids.is_contiguous() and tuple(qids.shape) == (B, 4)
    assert (means is None) == (istd is None) and (means is None or (f32(means, W) and f32(istd, W)))
    if pe is not None:
        assert pe.dim() == 2 and pe.shape[1] == W and pe.is_contiguous() and pe.dtype == torch.float32 and pe.is_cuda
        if pe.shape[0] < rows:
            raise _lib.Mi355Error(f"sanm_input: the position table holds {pe.shape[0]} rows, the batch needs {rows}")
    if x is None:
        x = torch.empty((B, rows, W), dtype=torch.float32, device=feats.device)
    Bx, Rx, Wx, xbs, ldx = _nlc(x)
    assert (Bx, Rx, Wx) == (B, rows, W)
    out_lens = torch.empty((B,), dtype=torch.int32, device=feats.device)
    _lib.call_struct("mi355_sanm_input", "mi355_sanm_input_args", _stream(), feats=_ptr(feats), feats_bstride=fbs, ldf=ldf, lens=_lens_arg(lens, B),
                     means=_ptr(means), istd=_ptr(istd), embed=_ptr(embed), qids=_ptr(qids), pe=_ptr(pe), pe_rows=0 if pe is None else pe.shape[0],
                     lfr_m=lfr_m, lfr_n=lfr_n, scale=scale, B=B, T=T, D=D, x=_ptr(x), x_bstride=xbs, ldx=ldx, out_lens=_ptr(out_lens))
    return x, out_lens


def ctc_rows(logits: torch.Tensor, *, ids: Optional[torch.Tensor] = None, gap: Optional[torch.Tensor] = None, lp: Optional[torch.Tensor] = None,
             logp: Optional[torch.Tensor] = None):
    """Per row of ``logits`` [rows, V] (row stride >= V), one read (``mi355_ctc_rows``): ``(ids int32, gap, lp)`` [rows] each -- the arg-max (first
    maximum on ties), the distance to the largest value at any other index, and the arg-max's log-probability.  ``ids`` / ``gap`` / ``lp``: contiguous
    [rows] outputs to fill (slices of a caller's buffers: the head runs in row chunks); ``logp`` [rows, V] also receives ``logits - logsumexp`` and may be
    ``logits`` itself."""
    assert logits.dim() == 2 and logits.stride(1) == 1 and logits.dtype == torch.float32 and logits.is_cuda
    rows, V = logits.shape
    dev = logits.device
    ids = torch.empty((rows,), dtype=torch.int32, device=dev) if ids is None else ids
    gap = torch.empty((rows,), dtype=torch.float32, device=dev) if gap is None else gap
    lp = torch.empty((rows,), dtype=torch.float32, device=dev) if lp is None else lp
    for t, dt in ((ids, torch.int32), (gap, torch.float32), (lp, torch.float32)):
        assert t.dtype == dt and t.is_cuda and t.is_contiguous() and t.numel() == rows
    kw = {}
    if logp is not None:
        assert logp.shape == logits.shape and logp.stride(1) == 1 and logp.dtype == torch.float32 and logp.is_cuda
        kw = dict(logp=_ptr(logp), ld_logp=logp.stride(0) if rows > 1 else max(logp.stride(0), V))
    _lib.call_struct("mi355_ctc_rows", "mi355_ctc_rows_args", _stream(), logits=_ptr(logits), ld=logits.stride(0) if rows > 1 else max(logits.stride(0), V),
                     rows=rows, V=V, ids=_ptr(ids), gap=_ptr(gap), lp=_ptr(lp), **kw)
    return ids, gap, lp


def ctc_collapse(ids: torch.Tensor, *, lens: Optional[torch.Tensor] = None, skip: int = 0, blank: int = 0, return_frames: bool = False):
    """Greedy CTC collapse of ``ids`` int32 [B, T] over the rows ``skip .. lens[b] - 1`` (``mi355_ctc_collapse``): repeats of the previous row's id
    dropped, then blanks -> ``(tokens int32 [B, T], counts int32 [B])`` on the device, -1 behind ``counts[b]``; ``return_frames`` adds each kept id's row."""
    assert ids.dim() == 2 and ids.stride(1) == 1 and ids.dtype == torch.int32 and ids.is_cuda
    B, T = ids.shape
    tokens = torch.empty((B, T), dtype=torch.int32, device=ids.device)
    counts = torch.empty((B,), dtype=torch.int32, device=ids.device)
    frames = torch.empty((B, T), dtype=torch.int32, device=ids.device) if return_frames else None
    _lib.call_struct("mi355_ctc_collapse", "mi355_ctc_collapse_args", _stream(), ids=_ptr(ids), ld_ids=ids.stride(0) if B > 1 else max(ids.stride(0), T),
                     lens=_lens_arg(lens, B), skip=skip, blank=blank, B=B, T=T, tokens=_ptr(tokens), counts=_ptr(counts), frames=_ptr(frames))
    return (tokens, counts, frames) if return_frames else (tokens, counts)


GAU_DIM = 128            # MI355_GAU_DIM
GAU_GROUP = 256          # MI355_GAU_GROUP
GAU_ROPE_DIMS = 32       # MI355_GAU_ROPE_DIMS
GAU_MAX_E = 2048         # MI355_GAU_MAX_E
GATED_FSMN_MAX_TAPS = 63  # MI355_GATED_FSMN_MAX_TAPS


def gau_rope_tables(rows: int, device=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(cos, sin)`` [rows, 16] float32 of ``nn.RoPE(dims=32, traditional=False, base=10000)``: the angle of row ``t``, pair ``i`` is
    ``t * 10000^(-i / 16)``, computed in float64 on the host and rounded once."""
    t = torch.arange(rows, dtype=torch.float64)[:, None]
    inv = torch.pow(torch.tensor(10000.0, dtype=torch.float64), -torch.arange(GAU_ROPE_DIMS // 2, dtype=torch.float64) / (GAU_ROPE_DIMS // 2))
    ang = t * inv[None, :]
    cos, sin = torch.cos(ang).float().contiguous(), torch.sin(ang).float().contiguous()
    return (cos, sin) if device is None else (cos.to(device), sin.to(device))


def shift_scalenorm(x: torch.Tensor, y: torch.Tensor, *, g: Optional[torch.Tensor] = None, eps: float = 1e-8, shift: bool = True,
                    lens: Optional[torch.Tensor] = None):
    """``y = s * g / max(||s||_2 * C^-1/2, eps)`` per row (``mi355_shift_scalenorm``), ``s`` = ``x`` with the first half of its columns taken from the
    row before (zero at row 0) when ``shift``, ``x`` itself otherwise.  ``x`` / ``y`` channels-last views [B, T, C], ``C`` a multiple of 8 up to 2048;
    ``g`` a one-element device tensor or None (= 1).  Rows at and beyond ``lens[b]`` come back zero."""
    B, T, C, xbs, ldx = _nlc(x)
    By, Ty, Cy, ybs, ldy = _nlc(y)
    assert (By, Ty, Cy) == (B, T, C)
    if g is not None:
        assert g.dtype == torch.float32 and g.is_cuda and g.numel() == 1
    _lib.call_struct("mi355_shift_scalenorm", "mi355_shift_scalenorm_args", _stream(), x=_ptr(x), x_bstride=xbs, ldx=ldx, g=_ptr(g), eps=eps,
                     shift=int(shift), lens=_lens_arg(lens, B), B=B, T=T, C=C, y=_ptr(y), y_bstride=ybs, ldy=ldy)
    return y


def _gau_common(qk, vu, gamma, beta, rope):
    B, T, Cq, qbs, ldq = _nlc(qk)
    Bv, Tv, E, vbs, ldv = _nlc(vu)
    assert (Bv, Tv) == (B, T) and Cq == GAU_DIM, (qk.shape, vu.shape)
    for t in (gamma, beta):
        assert t.dtype == torch.float32 and t.is_cuda and t.is_contiguous() and tuple(t.shape) == (4, GAU_DIM)
    cos, sin = rope
    for t in (cos, sin):
        assert t.dtype == torch.float32 and t.is_cuda and t.is_contiguous() and t.dim() == 2 and t.shape[1] == GAU_ROPE_DIMS // 2
    assert cos.shape == sin.shape
    return B, T, E, dict(qk=_ptr(qk), qk_bstride=qbs, ldqk=ldq, vu=_ptr(vu), vu_bstride=vbs, ldvu=ldv, gamma=_ptr(gamma), beta=_ptr(beta),
                         rope_cos=_ptr(cos), rope_sin=_ptr(sin), rope_rows=cos.shape[0], B=B, T=T, E=E)


def gau_kv_workspace_floats(B: int, T: int, E: int) -> int:
    return B * ((T + GAU_GROUP - 1) // GAU_GROUP) * GAU_DIM * E


def gau_kv(qk: torch.Tensor, vu: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, rope, *, lens: Optional[torch.Tensor] = None,
           kv: Optional[torch.Tensor] = None, ws: Optional[torch.Tensor] = None):
    """``kv[b] = lin_k[b]^T vu[b] / lens[b]`` [B, 128, E] over the rows below ``lens[b]`` (``mi355_gau_kv``): the global linear-attention matrix of
    the FLASH layer.  ``qk`` [B, T, 128] and ``vu`` [B, T, E] channels-last views, ``gamma`` / ``beta`` [4, 128], ``rope`` = ``gau_rope_tables``
    with at least ``T`` rows.  ``ws``: at least ``gau_kv_workspace_floats(B, T, E)`` floats for the per-group partial sums."""
    B, T, E, kw = _gau_common(qk, vu, gamma, beta, rope)
    if kv is None:
        kv = torch.empty((B, GAU_DIM, E), dtype=torch.float32, device=qk.device)
    assert kv.dtype == torch.float32 and kv.is_cuda and tuple(kv.shape) == (B, GAU_DIM, E) and kv[0].is_contiguous()
    need = gau_kv_workspace_floats(B, T, E)
    if ws is None:
        ws = torch.empty((need,), dtype=torch.float32, device=qk.device)
    assert ws.dtype == torch.float32 and ws.is_cuda and ws.is_contiguous()
    _lib.call_struct("mi355_gau_kv", "mi355_gau_kv_args", _stream(), lens=_lens_arg(lens, B), ws=_ptr(ws), ws_floats=ws.numel(), kv=_ptr(kv),
                     kv_bstride=kv.stride(0) if B > 1 else GAU_DIM * E, **kw)
    return kv


def gau_attention(qk: torch.Tensor, vu: torch.Tensor, kv: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, rope, out: torch.Tensor, *,
                  lens: Optional[torch.Tensor] = None, causal: bool = False, qk_dim: int = GAU_DIM, group: int = GAU_GROUP, cols: int = 0):
    """The FLASH layer's attention and output gate (``mi355_gau_attention``): per group of 256 rows ``relu(quad_q quad_k^T / 256)^2 vu`` plus
    ``lin_q kv``, then ``out = (A_u * v) * sigmoid(A_v * u)`` [B, T, E / 2].  Arguments as ``gau_kv``; ``kv`` its result.  Rows at and beyond
    ``lens[b]`` come back zero.  ``causal``, another ``qk_dim`` or ``group`` are refused; ``cols`` (0 = the library chooses) pins how many columns of
    ``v`` one workgroup owns and never changes a bit of the result."""
    B, T, E, kw = _gau_common(qk, vu, gamma, beta, rope)
    Bo, To, Ho, obs, ldo = _nlc(out)
    assert (Bo, To, Ho) == (B, T, E // 2)
    assert kv.dtype == torch.float32 and kv.is_cuda and tuple(kv.shape) == (B, GAU_DIM, E) and kv[0].is_contiguous()
    _lib.call_struct("mi355_gau_attention", "mi355_gau_attention_args", _stream(), kv=_ptr(kv), kv_bstride=kv.stride(0) if B > 1 else GAU_DIM * E,
                     lens=_lens_arg(lens, B), qk_dim=qk_dim, group=group, causal=int(causal), cols=cols, out=_ptr(out), out_bstride=obs, ldo=ldo, **kw)
    return out


def gated_fsmn(p: torch.Tensor, xu: torch.Tensor, xv: torch.Tensor, res: torch.Tensor, w: torch.Tensor, y: torch.Tensor, *,
               lens: Optional[torch.Tensor] = None):
    """``y = xv * (xu + p + sum_j w[:, j] * p[t + j - (K - 1) / 2]) + res`` (``mi355_gated_fsmn``): the gated FSMN memory of MossFormer2.  All five
    tensors channels-last views [B, T, C]; ``w`` [C, K] float32 (K odd, <= ``GATED_FSMN_MAX_TAPS``).  ``p`` reads as zero outside ``[0, lens[b])``;
    rows at and beyond ``lens[b]`` come back zero.  ``y`` may be ``res``."""
    B, T, C, pbs, ldp = _nlc(p)
    kw = {}
    for name, t in (("xu", xu), ("xv", xv), ("res", res), ("y", y)):
        Bt, Tt, Ct, bs, ld = _nlc(t)
        assert (Bt, Tt, Ct) == (B, T, C), (name, t.shape)
        kw.update({name: _ptr(t), name + "_bstride": bs, "ld" + name: ld})
    assert w.dim() == 2 and w.shape[0] == C and w.is_contiguous() and w.dtype == torch.float32 and w.is_cuda
    _lib.call_struct("mi355_gated_fsmn", "mi355_gated_fsmn_args", _stream(), p=_ptr(p), p_bstride=pbs, ldp=ldp, w=_ptr(w), K=w.shape[1],
                     lens=_lens_arg(lens, B), B=B, T=T, C=C, **kw)
    return y


def sample(logits: torch.Tensor, out: torch.Tensor, *, V: Optional[int] = None, suppress_mask=None, history=None, n_hist: int = 0,
           hist_len=None, repetition_penalty: float = 1.0, temperature: float = 0.0, top_k: int = 0, top_p: float = 1.0, min_p: float = 0.0,
           gumbel=None, done=None, done_token: int = 0, filtered=None):
    """Samples one token per row of ``logits`` [B, ld] into ``out`` (int32 view with B elements, any stride)."""
    assert logits.dim() == 2 and logits.stride(1) == 1 and logits.dtype == torch.float32 and out.dtype == torch.int32
    B = logits.shape[0]
    out_ld = out.stride(0) if out.dim() >= 1 and out.shape[0] == B and B > 1 else 1
    kw = dict(logits=_ptr(logits), ld=logits.stride(0), V=V or logits.shape[1], B=B, suppress_mask=_ptr(suppress_mask),
              repetition_penalty=repetition_penalty, temperature=temperature, top_k=top_k, top_p=top_p, min_p=min_p, gumbel=_ptr(gumbel),
              done=_ptr(done), done_token=done_token, out=_ptr(out), out_ld=out_ld, filtered=_ptr(filtered))
    if history is not None:
        assert history.dtype == torch.int32 and history.dim() == 2 and history.stride(1) == 1
        kw.update(history=_ptr(history), hist_ld=history.stride(0), n_hist=n_hist, hist_len=_ptr(hist_len))
    if gumbel is not None:
        assert gumbel.stride(0) == logits.stride(0)
    if filtered is not None:
        assert filtered.stride(0) == logits.stride(0)
    _lib.call_struct("mi355_sample", "mi355_sample_args", _stream(), **kw)
    return out


def gather_rows(table: torch.Tensor, idx: torch.Tensor, y: torch.Tensor, *, per_batch: bool = False, pos_table=None,
                add_row=None, lens=None):
    B, L, C, ybs, ldy = _nlc(y)
    assert idx.dtype == torch.int32 and idx.dim() == 2 and idx.stride(1) == 1
    if per_batch:
        assert table.dim() == 3 and table.stride(2) == 1
        tbs, ldt = table.stride(0), table.stride(1)
    else:
        assert table.dim() == 2 and table.stride(1) == 1
        tbs, ldt = 0, table.stride(0)
    _lib.call_struct("mi355_gather_rows", "mi355_gather_rows_args", _stream(), table=_ptr(table), ld_table=ldt,
                     table_bstride=tbs, pos_table=_ptr(pos_table), ld_pos=0 if pos_table is None else pos_table.stride(0),
                     add_row=_ptr(add_row), idx=_ptr(idx), idx_ld=idx.stride(0), C=C, L=L, lens=_ptr(lens), B=B, y=_ptr(y),
                     y_bstride=ybs, ldy=ldy)
    return y


def broadcast_rows(v: torch.Tensor, y: torch.Tensor, lens=None):
    B, L, C, ybs, ldy = _nlc(y)
    assert v.dim() == 2 and v.stride(1) == 1
    lib = _lib.load()
    rc = lib.mi355_broadcast_rows(_ptr(v), v.stride(0), C, _ptr(y), ybs, ldy, L, _ptr(lens), B, _stream())
    _lib.check(rc, "mi355_broadcast_rows")
    return y


def duration_align(logits: Optional[torch.Tensor], T: int, B: int, speed: float, idx_cap: int, device, lens=None,
                   forced: Optional[torch.Tensor] = None, bins: int = 50, max_frames: int = 0):
    dur = torch.empty((B, T), dtype=torch.int32, device=device)
    raw = torch.zeros((B, T), dtype=torch.float32, device=device)
    frames = torch.empty((B,), dtype=torch.int32, device=device)
    idx = torch.zeros((B, idx_cap), dtype=torch.int32, device=device)
    kw = dict(T=T, lens=_ptr(lens), B=B, speed=speed, forced_dur=_ptr(forced), dur=_ptr(dur), dur_raw=_ptr(raw),
              frames=_ptr(frames), idx=_ptr(idx), idx_ld=idx_cap, bins=bins, max_frames=max_frames)
    if logits is not None:
        _, _, _, bs, ld = _nlc(logits)
        kw.update(logits=_ptr(logits), bstride=bs, ld=ld)
    _lib.call_struct("mi355_duration_align", "mi355_duration_args", _stream(), **kw)
    return dur, raw, frames, idx


def adain_pool_up2(x: torch.Tensor, scale, shift, slope: float, w: torch.Tensor, bias: torch.Tensor, y: torch.Tensor, lens=None):
    B, L, C, xbs, ldx = _nlc(x)
    _, _, _, ybs, ldy = _nlc(y)
    _lib.call_struct("mi355_adain_pool_up2", "mi355_pool_up2_args", _stream(), x=_ptr(x), x_bstride=xbs, ldx=ldx, C=C, L=L,
                     lens=_ptr(lens), B=B, scale=_ptr(scale), shift=_ptr(shift), pre_ld=scale.stride(0), slope=slope,
                     w=_ptr(w), bias=_ptr(bias), y=_ptr(y), y_bstride=ybs, ldy=ldy)
    return y


def aa_activation(x: torch.Tensor, y: torch.Tensor, up_filter: torch.Tensor, down_filter: torch.Tensor, alpha: torch.Tensor, inv_beta: torch.Tensor, lens=None):
    """BigVGAN's anti-aliased SnakeBeta (``Activation1d``, codec/models/bigvgan/resample.py:157-177): x [B, L, C] -> y [B, L, C]."""
    B, L, C, xbs, ldx = _nlc(x)
    _, _, _, ybs, ldy = _nlc(y)
    assert up_filter.numel() == 12 and down_filter.numel() == 12 and alpha.numel() >= C and inv_beta.numel() >= C
    _lib.call_struct("mi355_aa_activation", "mi355_aa_act_args", _stream(), x=_ptr(x), x_bstride=xbs, ldx=ldx, C=C, L=L, lens=_ptr(lens), B=B,
                     up_filter=_ptr(up_filter), down_filter=_ptr(down_filter), alpha=_ptr(alpha), inv_beta=_ptr(inv_beta), y=_ptr(y), y_bstride=ybs, ldy=ldy)
    return y


def resample_poly(x: torch.Tensor, table: torch.Tensor, up: int, down: int, first: int, n_out: int, y: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Polyphase FIR rate conversion of the rows of x [rows, n_in] (``scipy.signal.resample_poly(..., padtype="edge")`` as ``mlx_audio/resample.py:40-47``
    calls it) with the tap-major float64 table [K, up] of ``mlx_audio_amd.resample.polyphase_table``."""
    assert x.dim() == 2 and x.dtype == torch.float32 and x.stride(1) == 1 and table.dtype == torch.float64 and table.is_contiguous() and table.shape[1] == up
    rows, n_in = x.shape
    if y is None:
        y = torch.empty(rows, n_out, device=x.device, dtype=torch.float32)
    assert y.shape == (rows, n_out) and y.stride(1) == 1 and y.dtype == torch.float32
    _lib.call_struct("mi355_resample_poly", "mi355_resample_args", _stream(), x=_ptr(x), x_bstride=x.stride(0), n_in=n_in, rows=rows, table=_ptr(table),
                     up=up, down=down, K=table.shape[0], first=first, y=_ptr(y), y_bstride=y.stride(0), n_out=n_out)
    return y


def conv1d_c1_k3s2(x: torch.Tensor, w3, bias: float, y: torch.Tensor, col: int, lens_in=None):
    """x [B, Lin] -> y[b, l, col] (Decoder.F0_conv / N_conv)."""
    assert x.dim() == 2 and x.stride(1) == 1
    B, Lout, _, ybs, ldy = _nlc(y)
    lib = _lib.load()
    rc = lib.mi355_conv1d_c1_k3s2(_ptr(x), x.stride(0), x.shape[1], _ptr(lens_in), float(w3[0]), float(w3[1]), float(w3[2]),
                                  float(bias), _ptr(y), ybs, ldy, col, Lout, B, _stream())
    _lib.check(rc, "mi355_conv1d_c1_k3s2")
    return y


# --------------------------------------------------------------------------------------- source / stft heads
def sine_source(f0: torch.Tensor, rand_ini: torch.Tensor, noise: torch.Tensor, lin_w: torch.Tensor, lin_b: float, up: int,
                lens2=None, sr: float = 24000.0, sine_amp: float = 0.1, noise_std: float = 0.003, voiced_thr: float = 10.0, quant: bool = False,
                coarse_f32: bool = False):
    B, L2 = f0.shape
    H = rand_ini.shape[1]
    assert f0.stride(1) == 1 and noise.is_contiguous() and tuple(noise.shape) == (B, L2 * up, H)
    ws = torch.empty((B, H, L2 + 1), dtype=torch.float32, device=f0.device)
    out = torch.zeros((B, L2 * up), dtype=torch.float32, device=f0.device)
    _lib.call_struct("mi355_sine_source", "mi355_sine_source_args", _stream(), f0=_ptr(f0), ld_f0=f0.stride(0), L2=L2,
                     lens2=_ptr(lens2), B=B, up=up, H=H, sr=sr, sine_amp=sine_amp, noise_std=noise_std, voiced_thr=voiced_thr,
                     rand_ini=_ptr(rand_ini), noise=_ptr(noise), lin_w=_ptr(lin_w), lin_b=lin_b, phase_ws=_ptr(ws),
                     out=_ptr(out), ld_out=out.stride(0),
                     quant_ws=_ptr(torch.empty((B, 2), dtype=torch.float32, device=f0.device)) if quant else None, coarse_f32=int(bool(coarse_f32)))
    return out


def stft_magphase(x: torch.Tensor, n_fft: int, hop: int, window: torch.Tensor, y: torch.Tensor, lens=None):
    assert x.dim() == 2 and x.stride(1) == 1
    B, _, _, ybs, ldy = _nlc(y)
    _lib.call_struct("mi355_stft_magphase", "mi355_stft_magphase_args", _stream(), x=_ptr(x), ldx=x.stride(0), L=x.shape[1],
                     lens=_ptr(lens), B=B, n_fft=n_fft, hop=hop, window=_ptr(window), y=_ptr(y), y_bstride=ybs, ldy=ldy)
    return y


def istft_head(x: torch.Tensor, n_fft: int, hop: int, window: torch.Tensor, audio: torch.Tensor, lens=None):
    B, Fr, _, xbs, ldx = _nlc(x)
    _lib.call_struct("mi355_istft_head", "mi355_istft_head_args", _stream(), x=_ptr(x), x_bstride=xbs, ldx=ldx, Fr=Fr,
                     lens=_ptr(lens), B=B, n_fft=n_fft, hop=hop, window=_ptr(window), audio=_ptr(audio),
                     ld_audio=audio.stride(0))
    return audio


def conv_post_istft_eligible(pc: PackedConv, n_fft: int, hop: int, *, dil: int = 1, pad: int = 3, pre_act: int = ACT_LEAKY, precision: int = 2,
                             pre_fq=None) -> bool:
    """Shapes ``mi355_conv_post_istft`` takes (the header's list).  Nothing here looks at the batch or at the number of frames: an utterance takes the
    same path alone and inside a batch."""
    return (pc.cin % 32 == 0 and pc.k == 7 and dil == 1 and pad == 3 and n_fft == 20 and hop == 5 and pc.cout == n_fft + 2 and pc.cout <= 32
            and pre_act == ACT_LEAKY and precision == 2 and not pc.f16 and not pc.mx and pre_fq is None)


def conv_post_istft(x: torch.Tensor, pc: PackedConv, n_fft: int, hop: int, window: torch.Tensor, audio: torch.Tensor, *, lens=None,
                    dil: int = 1, pad: int = 3, pre_act: int = ACT_LEAKY, pre_slope: float = 0.01, precision: int = 2, pre_fq=None):
    """The generator tail: ``audio = istft_head(conv_post(act(x)))``, x [B, L, Cin] -> audio [B, (L - 1) * hop].  One launch
    (``mi355_conv_post_istft``) where ``conv_post_istft_eligible``; every other call runs ``conv_gemm`` into a scratch ``post`` tensor and
    ``istft_head`` on it, the two launches the fused kernel stands for."""
    B, L, _, xbs, ldx = _nlc(x)
    if conv_post_istft_eligible(pc, n_fft, hop, dil=dil, pad=pad, pre_act=pre_act, precision=precision, pre_fq=pre_fq):
        assert audio.dim() == 2 and audio.stride(1) == 1 and audio.dtype == torch.float32 and audio.shape[1] >= (L - 1) * hop
        if PROFILE is not None:   # the conv's entry of the per-launch table (conv_gemm above); the interval also holds the head's work
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            PROFILE.append(((L * B) if lens is None else lens.sum(), pc.cin, pc.cout, pc.k, dil, 0, e0, e1))
        _lib.call_struct("mi355_conv_post_istft", "mi355_conv_post_istft_args", _stream(), x=_ptr(x), x_bstride=xbs, ldx=ldx, Cin=pc.cin, L=L,
                         lens=_ptr(lens), B=B, w=_ptr(pc.w), bias=_ptr(pc.bias), Cout=pc.cout, K=pc.k, dil=dil, pad=pad, pre_act=pre_act,
                         pre_slope=pre_slope, precision=precision, n_fft=n_fft, hop=hop, window=_ptr(window), audio=_ptr(audio),
                         ld_audio=audio.stride(0))
        if PROFILE is not None:
            e1.record()
        return audio
    post = torch.empty((B, L, round_up(pc.cout, 4)), dtype=torch.float32, device=x.device)[:, :, :pc.cout]
    conv_gemm(x, pc, post, dil=dil, pad=pad, lens_in=lens, lens_out=lens, pre_act=pre_act, pre_slope=pre_slope, precision=precision, pre_fq=pre_fq)
    return istft_head(post, n_fft, hop, window, audio, lens=lens)


# (Cin, Cout, stride) instantiations of mi355_upsample_polyphase (the header's list) -> GEMM rows a workgroup owns (upsample_poly.hip)
UPSAMPLE_POLY_SHAPES = {(512, 256, 10): 32, (256, 128, 6): 64}


def upsample_polyphase_eligible(pc: PackedConv, stride: int, *, pre_act: int = ACT_LEAKY, precision: int = 2, res=True, pre_fq=None) -> bool:
    """Up-samplers ``mi355_upsample_polyphase`` takes: a bf16 polyphase image (``pack_conv_transpose``) with two taps per phase and one of the
    instantiated (Cin, Cout, stride) sets, a LeakyReLU prologue and a residual.  Nothing here looks at the batch or at the length."""
    return (pc.k == 2 and stride > 0 and pc.cout % stride == 0 and (pc.cin, pc.cout // stride, stride) in UPSAMPLE_POLY_SHAPES
            and pre_act == ACT_LEAKY and precision == 2 and not pc.f16 and not pc.mx and res is not None and pre_fq is None)


def upsample_polyphase(x: torch.Tensor, pc: PackedConv, res: torch.Tensor, y: torch.Tensor, stride: int, *, row_off: int = 0, lens=None,
                       pre_act: int = ACT_LEAKY, pre_slope: float = 0.1, precision: int = 2, pre_fq=None):
    """One generator up-sampler: ``y[:, row_off:] = conv_transpose1d(leaky_relu(x), stride, K = 2 stride, padding = stride / 2) + res[:, row_off:]``
    (and ``y[:, 0] = res[:, 0]`` for ``row_off = 1``), x [B, L, Cin] -> y [B, L * stride + row_off, Cout]; ``pc`` from ``pack_conv_transpose``.
    One launch of the dedicated kernel (``mi355_upsample_polyphase``) where ``upsample_polyphase_eligible``; every other call runs the polyphase
    ``conv_gemm`` (and the row copy) it stands for (the kernel is bit-equal to that launch on the wave-specialised conv kernel)."""
    B, L, _, xbs, ldx = _nlc(x)
    u = stride
    cout = pc.cout // u
    kfull = pc.k * u
    p = (kfull - u) // 2
    Lo = L * u + row_off
    assert y.shape[0] == B and y.shape[1] >= Lo and y.shape[2] == cout and res.shape[0] == B and res.shape[1] >= Lo and res.shape[2] == cout
    if upsample_polyphase_eligible(pc, u, pre_act=pre_act, precision=precision, res=res, pre_fq=pre_fq) and row_off in (0, 1):
        _, _, _, rbs, ldr = _nlc(res)
        _, _, _, ybs, ldy = _nlc(y)
        assert pc.w.numel() >= _lib.load().mi355_packed_conv_weight_elems(pc.cout, pc.k, pc.cin)
        if PROFILE is not None:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            PROFILE.append((((L + 1) * B) if lens is None else (lens + 1).sum(), pc.cin, pc.cout, pc.k, 1, 1, e0, e1))
        _lib.call_struct("mi355_upsample_polyphase", "mi355_upsample_polyphase_args", _stream(), x=_ptr(x), x_bstride=xbs, ldx=ldx, Cin=pc.cin, L=L,
                         lens=_ptr(lens), B=B, w=_ptr(pc.w), bias=_ptr(pc.bias), Cout=cout, K=kfull, u=u, p=p, row_off=row_off, slope=pre_slope,
                         precision=precision, res=_ptr(res), res_bstride=rbs, ldr=ldr, y=_ptr(y), y_bstride=ybs, ldy=ldy)
        if PROFILE is not None:
            e1.record()
        return y
    kp = pc.k
    conv_gemm(x, pc, y, pad=kp - 1, lout=L + kp - 1, lens_in=lens, lens_out=None if lens is None else lens + (kp - 1), pre_act=pre_act,
              pre_slope=pre_slope, res=res, precision=precision, pre_fq=pre_fq,
              up=dict(s=u, p=p, cout=cout, row_off=row_off, lout=L * u, lens=None if lens is None else lens * u))
    if row_off:
        y[:, :row_off, :].copy_(res[:, :row_off, :])
    return y


# --------------------------------------------------------------------------------------- generic dsp
def stft_frames(x: torch.Tensor, n_fft: int, hop: int, window: torch.Tensor, pad_mode: int, n_frames: int):
    """x [B, L] -> complex64 [B, n_frames, n_fft//2+1]."""
    assert x.dim() == 2 and x.stride(1) == 1 and x.dtype == torch.float32
    B, L = x.shape
    out = torch.empty((B, n_frames, n_fft // 2 + 1, 2), dtype=torch.float32, device=x.device)
    _lib.call_struct("mi355_stft", "mi355_stft_args", _stream(), x=_ptr(x), ldx=x.stride(0), L=L, B=B, n_fft=n_fft, hop=hop,
                     window=_ptr(window), pad_mode=pad_mode, n_frames=n_frames, out=_ptr(out))
    return torch.view_as_complex(out)


def logmel(x: torch.Tensor, n_fft: int, hop: int, window: torch.Tensor, pad_mode: int, n_frames: int, fb: torch.Tensor,
           mode: int, log_guard: float = 0.0, fixed_max: Optional[float] = None):
    """Fused STFT -> power -> mel -> log (``mi355_logmel``).  ``mode`` 0 clamps to (max - 8) and rescales like Whisper: the maximum is the global one of
    every item, or ``fixed_max`` when given (Voxtral Realtime's ``global_log_mel_max``); ``mode`` 4 = ln(mel + ``log_guard``) (NeMo)."""
    assert x.dim() == 2 and x.stride(1) == 1 and fb.is_contiguous()
    B, L = x.shape
    n_mels = fb.shape[0]
    out = torch.empty((B, n_frames, n_mels), dtype=torch.float32, device=x.device)
    gmax = torch.empty((B,), dtype=torch.float32, device=x.device) if mode == 0 else None
    _lib.call_struct("mi355_logmel", "mi355_logmel_args", _stream(), x=_ptr(x), ldx=x.stride(0), L=L, B=B, n_fft=n_fft,
                     hop=hop, window=_ptr(window), pad_mode=pad_mode, n_frames=n_frames, fb=_ptr(fb), n_mels=n_mels,
                     mode=mode, out=_ptr(out), gmax=None if fixed_max is not None else _ptr(gmax), log_guard=float(log_guard))
    if mode == 0:
        if fixed_max is not None:
            gmax.fill_(float(fixed_max))
        lib = _lib.load()
        rc = lib.mi355_logmel_finish(_ptr(out), n_frames * n_mels, _ptr(gmax), B, _stream())
        _lib.check(rc, "mi355_logmel_finish")
    return out


def kaldi_frames(x: torch.Tensor, win: int, shift: int, pad: int, n_fft: int, n_frames: int, window: torch.Tensor, preemph: float,
                 noise: Optional[torch.Tensor] = None, dither: float = 0.0) -> torch.Tensor:
    """x [L] -> Kaldi frames [n_frames, n_fft] (DC removed, pre-emphasised, windowed, zero-padded)."""
    assert x.dim() == 1 and x.is_contiguous() and x.dtype == torch.float32 and window.numel() == win
    out = torch.empty((n_frames, n_fft), dtype=torch.float32, device=x.device)
    if noise is not None:
        assert noise.is_contiguous() and tuple(noise.shape) == (n_frames, win)
    _lib.call_struct("mi355_kaldi_frames", "mi355_kaldi_frames_args", _stream(), x=_ptr(x), L=x.numel(), win=win, shift=shift, pad=pad, n_fft=n_fft,
                     n_frames=n_frames, window=_ptr(window), noise=_ptr(noise), dither=dither, preemph=preemph, frames=_ptr(out))
    return out


def polar_spec(x: torch.Tensor, nb: int, clip: float = 1e2) -> torch.Tensor:
    """x [B, Fr, 2 nb] (log-magnitude | phase) -> complex64 [B, Fr, nb] = min(exp(m), clip) * exp(i p)  (Vocos ISTFTHead)."""
    B, Fr, C, xbs, ldx = _nlc(x)
    assert C >= 2 * nb
    spec = torch.empty((B, Fr, nb), dtype=torch.complex64, device=x.device)
    lib = _lib.load()
    rc = lib.mi355_polar_spec(_ptr(x), xbs, ldx, Fr, nb, B, float(clip), _ptr(torch.view_as_real(spec)), _stream())
    _lib.check(rc, "mi355_polar_spec")
    return spec


def istft_frames(spec: torch.Tensor, n_fft: int, hop: int, window: torch.Tensor, norm: torch.Tensor, norm_mode: int,
                 clamp: bool, trim: int, out_len: int):
    """spec complex64 [B, n_frames, nb] -> [B, out_len]."""
    sr = torch.view_as_real(spec.contiguous())
    B, n_frames = spec.shape[0], spec.shape[1]
    ws = torch.empty((B, (n_frames + 1) // 2 * 2, n_fft), dtype=torch.float32, device=spec.device)
    out = torch.empty((B, out_len), dtype=torch.float32, device=spec.device)
    _lib.call_struct("mi355_istft", "mi355_istft_args", _stream(), spec=_ptr(sr), n_frames=n_frames, B=B, n_fft=n_fft,
                     hop=hop, window=_ptr(window), norm=_ptr(norm), norm_mode=norm_mode, clamp=int(clamp), trim=trim,
                     out_len=out_len, frames_ws=_ptr(ws), out=_ptr(out), ld_out=out.stride(0))
    return out


# ---------------------------------------------------------------------------------------------- FireRedASR2-AED (csrc/firered.hip)
SUBSAMPLE2D_MAX_COUT = 64        # MI355_SUBSAMPLE2D_MAX_COUT
GLU_DWCONV_LN_MAX_TAPS = 33      # MI355_GLU_DWCONV_LN_MAX_TAPS
GLU_DWCONV_LN_MAX_C = 2560       # MI355_GLU_DWCONV_LN_MAX_C
GLU_DWCONV_LN_ROWS = 32          # MI355_GLU_DWCONV_LN_ROWS
BEAM_MAX = 8                     # MI355_BEAM_MAX
BEAM_MAX_V = 65536               # MI355_BEAM_MAX_V
BEAM_ATTN_MAX_TK = 4096          # MI355_BEAM_ATTN_MAX_TK


def subsample2d_out(n: int) -> int:
    """k = 3, stride 2, no padding."""
    return (n - 3) // 2 + 1


def subsample2d_k3s2(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], y: torch.Tensor, *, relu: bool = True, out_cf: bool = False,
                     lens_in: Optional[torch.Tensor] = None, lens_out: Optional[torch.Tensor] = None):
    """Dense 3 x 3 / stride 2 conv without padding over (time, frequency) (``mi355_subsample2d_k3s2``): ``x`` [B, T, F] (one input channel) or
    channels-last [B, T, F, Cin], ``w`` [Cout, 3, 3, Cin], ``y`` [B, To, Fo, Cout], or [B, To, Cout, Fo] with ``out_cf`` (rows in the ``c * Fo + f`` order
    the subsampler's ``out`` linear reads).  Input rows at and beyond ``lens_in[b]`` read as zero, output rows at and beyond ``lens_out[b]`` are zero."""
    assert x.dtype == torch.float32 and x.is_cuda and y.dtype == torch.float32 and y.is_cuda and y.dim() == 4 and x.dim() in (3, 4)
    B, T, F = x.shape[:3]
    Cin = 1 if x.dim() == 3 else x.shape[3]
    Cout = w.shape[0]
    To, Fo = subsample2d_out(T), subsample2d_out(F)
    assert x[0].is_contiguous() and y[0].is_contiguous()
    assert tuple(y.shape) == ((B, To, Cout, Fo) if out_cf else (B, To, Fo, Cout)), (tuple(y.shape), tuple(x.shape))
    assert tuple(w.shape) == (Cout, 3, 3, Cin) and w.is_contiguous() and w.dtype == torch.float32 and w.is_cuda
    assert bias is None or (bias.numel() == Cout and bias.is_contiguous() and bias.dtype == torch.float32 and bias.is_cuda)
    _lib.call_struct("mi355_subsample2d_k3s2", "mi355_subsample2d_k3s2_args", _stream(), x=_ptr(x), x_bstride=x.stride(0) if B > 1 else x[0].numel(),
                     w=_ptr(w), bias=_ptr(bias), B=B, T=T, F=F, Cin=Cin, Cout=Cout, relu=int(relu), out_cf=int(out_cf), lens_in=_lens_arg(lens_in, B),
                     lens_out=_lens_arg(lens_out, B), y=_ptr(y), y_bstride=y.stride(0) if B > 1 else y[0].numel())
    return y


def glu_dwconv_ln_swish(x: torch.Tensor, w: torch.Tensor, ln_w: torch.Tensor, ln_b: torch.Tensor, y: torch.Tensor, *, eps: float = 1e-5,
                        lens: Optional[torch.Tensor] = None):
    """``swish(LayerNorm_C(sum_k w[:, k] * g[t + k - (K - 1) / 2]))`` with ``g = x[..., :C] * sigmoid(x[..., C:])`` (``mi355_glu_dwconv_ln_swish``): the
    middle of FireRedASR2's convolution module in one launch, ``x`` [B, L, 2 C] -> ``y`` [B, L, C]; ``w`` [C, K] (K odd, <= ``GLU_DWCONV_LN_MAX_TAPS``),
    ``ln_w`` / ``ln_b`` [C], C a multiple of 4 up to ``GLU_DWCONV_LN_MAX_C``.  ``g`` is zero outside ``[0, lens[b])``; rows at and beyond ``lens[b]`` are zero."""
    B, L, C2, xbs, ldx = _nlc(x)
    By, Ly, C, ybs, ldy = _nlc(y)
    assert (By, Ly) == (B, L) and C2 == 2 * C
    f32 = lambda t, n: t.dtype == torch.float32 and t.is_cuda and t.is_contiguous() and t.numel() == n
    assert w.dim() == 2 and w.shape[0] == C and f32(w, w.numel()) and f32(ln_w, C) and f32(ln_b, C)
    _lib.call_struct("mi355_glu_dwconv_ln_swish", "mi355_glu_dwconv_ln_swish_args", _stream(), x=_ptr(x), x_bstride=xbs, ldx=ldx, w=_ptr(w), ln_w=_ptr(ln_w),
                     ln_b=_ptr(ln_b), eps=eps, K=w.shape[1], C=C, L=L, lens=_lens_arg(lens, B), B=B, y=_ptr(y), y_bstride=ybs, ldy=ldy)
    return y


@dataclass
class BeamState:
    """The device state of ``beam_step`` for N utterances of B beams.  ``tokens`` / ``ind`` / ``conf`` are pairs of [N, B, Tmax] buffers: a step reads
    ``[cur]`` and writes ``[1 - cur]``, then ``cur`` flips.  An utterance that is done is left untouched by later steps, so its final histories are in
    the buffer its last live step wrote: index ``step[n] % 2 == 0`` -> buffer 1, else buffer 0 when ``cur`` started at 0 (``final()`` does this)."""
    scores: torch.Tensor
    finished: torch.Tensor
    step: torch.Tensor
    max_steps: torch.Tensor
    done: torch.Tensor
    tokens: Tuple[torch.Tensor, torch.Tensor]
    ind: Tuple[torch.Tensor, torch.Tensor]
    conf: Tuple[torch.Tensor, torch.Tensor]
    beam_idx: torch.Tensor
    new_tokens: torch.Tensor
    new_conf: torch.Tensor
    cur: int = 0

    def final(self):
        """``(tokens, conf, ind)`` [N, B, Tmax] as each utterance's last live step left them (histories start with <sos> at index 0)."""
        sel = (self.step % 2 == 0).view(-1, 1, 1)     # step s was written by the call that started at step s - 1 = the (s - 1)-th call
        pick = lambda pair: torch.where(sel, pair[1], pair[0])
        return pick(self.tokens), pick(self.conf), pick(self.ind)


def beam_state(N: int, B: int, Tmax: int, max_steps, *, sos_id: int, device) -> BeamState:
    """The state before the first step: scores ``[0, -1e10, ...]``, nothing finished, ``step = 1`` with <sos> at index 0 of every history and
    ``ind[n, j, 0] = j``.  ``max_steps`` [N] (ints or a tensor): an utterance is done once its history holds that many entries (<sos> included)."""
    i32 = dict(dtype=torch.int32, device=device)
    scores = torch.full((N, B), -1e10, dtype=torch.float32, device=device)
    scores[:, 0] = 0.0
    tokens = torch.full((N, B, Tmax), sos_id, **i32)
    ind = torch.zeros((N, B, Tmax), **i32)
    ind[:, :, 0] = torch.arange(B, **i32)[None, :]
    conf = torch.zeros((N, B, Tmax), dtype=torch.float32, device=device)
    ms = torch.as_tensor(max_steps, dtype=torch.int32).to(device).contiguous()
    assert ms.numel() == N
    return BeamState(scores=scores, finished=torch.zeros((N, B), **i32), step=torch.ones((N,), **i32), max_steps=ms, done=torch.zeros((N,), **i32),
                     tokens=(tokens, tokens.clone()), ind=(ind, ind.clone()), conf=(conf, conf.clone()), beam_idx=torch.zeros((N, B), **i32),
                     new_tokens=torch.zeros((N, B), **i32), new_conf=torch.zeros((N, B), dtype=torch.float32, device=device))


def beam_step(logits: torch.Tensor, st: BeamState, *, eos_id: int, softmax_smoothing: float = 1.25, eos_penalty: float = 1.0) -> BeamState:
    """One step of FireRedASR2's beam search for every utterance that is not done (``mi355_beam_step``): ``logits`` [N * B, V] (row stride >= V) ->
    the state advanced in place (scores, finished, step, done, beam_idx, new_tokens, new_conf) and the histories written to the other buffer of each
    pair.  Ties: the lower beam first, then the lower token id."""
    assert logits.dim() == 2 and logits.stride(1) == 1 and logits.dtype == torch.float32 and logits.is_cuda
    N, B = st.scores.shape
    Tmax = st.tokens[0].shape[2]
    assert logits.shape[0] == N * B
    V = logits.shape[1]
    src, dst = st.cur, 1 - st.cur
    _lib.call_struct("mi355_beam_step", "mi355_beam_step_args", _stream(), logits=_ptr(logits), ld=logits.stride(0) if N * B > 1 else max(logits.stride(0), V),
                     N=N, B=B, V=V, Tmax=Tmax, eos_id=eos_id, softmax_smoothing=softmax_smoothing, eos_penalty=eos_penalty, scores=_ptr(st.scores),
                     finished=_ptr(st.finished), step=_ptr(st.step), max_steps=_ptr(st.max_steps), done=_ptr(st.done), tokens_in=_ptr(st.tokens[src]),
                     tokens_out=_ptr(st.tokens[dst]), ind_in=_ptr(st.ind[src]), ind_out=_ptr(st.ind[dst]), conf_in=_ptr(st.conf[src]),
                     conf_out=_ptr(st.conf[dst]), beam_idx=_ptr(st.beam_idx), new_tokens=_ptr(st.new_tokens), new_conf=_ptr(st.new_conf))
    st.cur = dst
    return st


def beam_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, ind: torch.Tensor, pos: torch.Tensor, out: torch.Tensor, *, beams: int, heads: int,
                   dh: int, scale: Optional[float] = None, Tk: Optional[int] = None):
    """Decoder self-attention of one query per (utterance, beam) over a cache that is never re-gathered (``mi355_beam_attention``): ``q`` / ``out``
    [N * B, heads * dh], ``k`` / ``v`` [N * B, Tcap, heads * dh] (row ``s`` of slot ``n * B + i`` = position ``s`` as beam ``i`` wrote it), ``ind`` int32
    [N, B, Tmax] the slot of every position per beam (``beam_step`` maintains it), ``pos`` int32 [N] the last position to attend to (negative: a zero
    row).  ``Tk`` (default: the caches' rows) bounds the positions read."""
    assert q.dim() == 2 and out.dim() == 2 and q.stride(1) == 1 and out.stride(1) == 1 and q.dtype == torch.float32 and out.dtype == torch.float32
    NB = q.shape[0]
    _, Tcap, C, kss, ldk = _nlc(k)
    _, Tv, Cv, vss, ldv = _nlc(v)
    assert NB % beams == 0 and k.shape[0] == NB and v.shape[0] == NB and Tv == Tcap and C == heads * dh == Cv == q.shape[1] == out.shape[1] and out.shape[0] == NB
    N = NB // beams
    assert ind.dtype == torch.int32 and ind.is_cuda and ind.is_contiguous() and ind.dim() == 3 and tuple(ind.shape[:2]) == (N, beams)
    assert pos.dtype == torch.int32 and pos.is_cuda and pos.is_contiguous() and pos.numel() == N and q.is_cuda and out.is_cuda
    Tk = Tcap if Tk is None else Tk
    assert 1 <= Tk <= Tcap
    one = lambda t, s: s if t.shape[0] > 1 else max(s, t.shape[1])
    _lib.call_struct("mi355_beam_attention", "mi355_beam_attention_args", _stream(), q=_ptr(q), ldq=one(q, q.stride(0)), k=_ptr(k),
                     k_sstride=kss if NB > 1 else max(kss, Tcap * ldk), ldk=ldk, v=_ptr(v), v_sstride=vss if NB > 1 else max(vss, Tcap * ldv), ldv=ldv,
                     ind=_ptr(ind), ld_ind=ind.shape[2], pos=_ptr(pos), N=N, B=beams, Tk=Tk, heads=heads, dh=dh,
                     scale=(1.0 / math.sqrt(dh)) if scale is None else scale, out=_ptr(out), ldo=one(out, out.stride(0)))
    return out


# --------------------------------------------------------------------------------------- Granite Speech NAR (granite_nar.hip)
SELFCOND_WAVE_MAX_V = 256   # MI355_SELFCOND_WAVE_MAX_V


def shaw_block_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, table: torch.Tensor, out: torch.Tensor, *, heads: int, dh: int, ctx: int,
                         max_pos: int, scale: Optional[float] = None, lens: Optional[torch.Tensor] = None, check_lens: bool = True):
    """``out_i = sum_j softmax_j(scale (q_i . k_j + q_i . table[max_pos + i - j])) v_j`` over the ``ctx`` keys of query ``i``'s own block
    ``[m ctx, (m + 1) ctx)``, ``m = i // ctx`` (``mi355_shaw_block_attention``): Granite Speech NAR's block-local attention with Shaw relative
    positions behind its projections.  ``q`` / ``k`` / ``v`` / ``out`` channels-last views [B, T, heads * dh] (thirds of a fused buffer or contiguous),
    NOT padded to a multiple of ``ctx``; ``table`` [2 max_pos + 1, dh], one for all heads, row ``max_pos + d`` holding distance ``d = i - j``.  A key
    of the block at or beyond ``lens[b]`` counts as a zero key with a zero value and is NOT masked (the reference's zero padding of the last block);
    rows at and beyond ``lens[b]`` come back zero.  Every ``lens[b]`` must be in ``[0, T]``: checked here with one device read of ``lens``, which a
    caller that built ``lens`` from host integers it has already checked turns off (``check_lens=False``)."""
    B, T, C, qbs, ldq = _nlc(q)
    Bk, Tk, Ck, kbs, ldk = _nlc(k)
    Bv, Tv, Cv, vbs, ldv = _nlc(v)
    Bo, To, Co, obs, ldo = _nlc(out)
    hd = heads * dh
    assert (Bk, Tk) == (B, T) and (Bv, Tv) == (B, T) and (Bo, To) == (B, T) and min(C, Ck, Cv, Co) >= hd
    assert table.dim() == 2 and table.stride(1) == 1 and table.shape[1] >= dh and table.dtype == torch.float32 and table.is_cuda
    lp = _lens_arg(lens, B)
    if lens is not None and check_lens:
        lo, hi = int(lens.min()), int(lens.max())
        if lo < 0 or hi > T:
            raise _lib.Mi355Error(f"shaw_block_attention: lens must lie in [0, T = {T}] (got min {lo}, max {hi})")
    _lib.call_struct("mi355_shaw_block_attention", "mi355_shaw_block_attention_args", _stream(), q=_ptr(q), q_bstride=qbs, ldq=ldq, k=_ptr(k),
                     k_bstride=kbs, ldk=ldk, v=_ptr(v), v_bstride=vbs, ldv=ldv, table=_ptr(table), ldt=table.stride(0), rows=table.shape[0],
                     max_pos=max_pos, lens=lp, B=B, T=T, heads=heads, dh=dh, ctx=ctx, scale=dh ** -0.5 if scale is None else scale, out=_ptr(out),
                     out_bstride=obs, ldo=ldo)
    return out


def selfcond_rows(logits: torch.Tensor, *, probs: Optional[torch.Tensor] = None, p_blank: Optional[torch.Tensor] = None):
    """Per row of ``logits`` [rows, V] (row stride >= V): ``(probs [rows, V], p_blank [rows])`` -- the float32 softmax probabilities and column 0
    of them (``mi355_selfcond_rows``): the self-conditioning step of Granite Speech NAR's encoder.  One wave per row up to
    ``SELFCOND_WAVE_MAX_V`` columns, one workgroup above."""
    assert logits.dim() == 2 and logits.stride(1) == 1 and logits.dtype == torch.float32 and logits.is_cuda
    rows, V = logits.shape
    dev = logits.device
    probs = torch.empty((rows, V), dtype=torch.float32, device=dev) if probs is None else probs
    p_blank = torch.empty((rows,), dtype=torch.float32, device=dev) if p_blank is None else p_blank
    assert probs.shape == logits.shape and probs.stride(1) == 1 and probs.dtype == torch.float32 and probs.is_cuda
    assert p_blank.dtype == torch.float32 and p_blank.is_cuda and p_blank.is_contiguous() and p_blank.numel() == rows
    one = lambda t: t.stride(0) if rows > 1 else max(t.stride(0), V)
    _lib.call_struct("mi355_selfcond_rows", "mi355_selfcond_rows_args", _stream(), logits=_ptr(logits), ld=one(logits), rows=rows, V=V, probs=_ptr(probs),
                     ld_probs=one(probs), p_blank=_ptr(p_blank))
    return probs, p_blank


def posterior_pool(h: torch.Tensor, p_blank: torch.Tensor, window: int, *, lens: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None):
    """``_posterior_weighted_pool`` of Granite Speech NAR's encoder (``mi355_posterior_pool``): ``h`` [B, T, C], ``p_blank`` [B, T] ->
    [B, ceil(T / window), C], every window's frames weighted by ``(1 - p_blank) / max(sum, 1e-6)``.  Frames at and beyond ``lens[b]`` weigh 0 (a
    partial last window weights only its real frames); a window wholly beyond the item comes back zero."""
    B, T, C, hbs, ldh = _nlc(h)
    assert p_blank.dim() == 2 and tuple(p_blank.shape) == (B, T) and p_blank.stride(1) == 1 and p_blank.dtype == torch.float32 and p_blank.is_cuda
    nw = (T + window - 1) // window if window >= 1 else 1
    if out is None:
        out = torch.empty((B, nw, C), dtype=torch.float32, device=h.device)
    Bo, No, Co, obs, ldo = _nlc(out)
    assert (Bo, No, Co) == (B, nw, C)
    _lib.call_struct("mi355_posterior_pool", "mi355_posterior_pool_args", _stream(), h=_ptr(h), h_bstride=hbs, ldh=ldh, p_blank=_ptr(p_blank),
                     pb_bstride=p_blank.stride(0) if B > 1 else max(p_blank.stride(0), T), window=window, lens=_lens_arg(lens, B), B=B, T=T, C=C,
                     out=_ptr(out), out_bstride=obs, ldo=ldo)
    return out


def qformer_windows(h: torch.Tensor, query: torch.Tensor, positions: torch.Tensor, *, block: int, rate: int, lens: Optional[torch.Tensor] = None,
                    queries: Optional[torch.Tensor] = None, kv: Optional[torch.Tensor] = None):
    """The window assembly of Granite Speech NAR's projector in one launch (``mi355_qformer_windows``): ``h`` [B, T, C] ->
    ``(queries [B nblocks, block / rate, C], kv [B nblocks, block, C])`` with ``nblocks = ceil(T / block)``.  Every window is right-padded with
    zero rows from ``lens[b]`` on; ``queries`` = ``query`` [block / rate, C] + the mean over each group of ``rate`` rows, ``kv`` = the window +
    ``positions`` [block, C]."""
    B, T, C, hbs, ldh = _nlc(h)
    if block < 1 or rate < 1 or block % rate:
        raise _lib.Mi355Error(f"qformer_windows: block = {block} must be a positive multiple of rate = {rate}")
    nq, nb = block // rate, (T + block - 1) // block
    f32 = lambda t, shape: t.dtype == torch.float32 and t.is_cuda and t.is_contiguous() and tuple(t.shape) == shape
    assert f32(query, (nq, C)) and f32(positions, (block, C))
    if queries is None:
        queries = torch.empty((B * nb, nq, C), dtype=torch.float32, device=h.device)
    if kv is None:
        kv = torch.empty((B * nb, block, C), dtype=torch.float32, device=h.device)
    assert f32(queries, (B * nb, nq, C)) and f32(kv, (B * nb, block, C))
    _lib.call_struct("mi355_qformer_windows", "mi355_qformer_windows_args", _stream(), h=_ptr(h), h_bstride=hbs, ldh=ldh, lens=_lens_arg(lens, B), B=B, T=T,
                     C=C, block=block, rate=rate, query=_ptr(query), positions=_ptr(positions), queries=_ptr(queries), kv=_ptr(kv))
    return queries, kv
