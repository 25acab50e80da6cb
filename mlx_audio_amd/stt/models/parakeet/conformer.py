"""NeMo FastConformer encoder on MI355X (stt/models/parakeet/conformer.py + attention.py): mel [B, T, feat_in] -> hidden [B, T', d_model].

The reference runs ONE un-padded sequence per call (attention.py:119 reshapes the batch-1 position projection to the batch size, and no layer gets a
mask).  What is built here is the module's meaning for a right-padded batch with ``lengths``: item ``b`` of a batch equals the reference on that item
alone.  Every padded frame reads as zero into the subsampler's convs and into the convolution module's depthwise conv, and is masked as a key.

Host schedule:

  * subsampler (``DwStridingSubsampling``): ``stencil2d_k3s2`` (one input channel, ReLU), then per further stage ``stencil2d_k3s2`` (depthwise) and
    the 1 x 1 conv as a ``conv_gemm`` over the B * T * F rows with ReLU; the output linear reads the channels-last [T', F' * C] view, its weight
    columns permuted from the reference's ``c * F' + f`` order at load time; ``xscaling`` is its ``out_scale``.  ``subsampling_factor == 1`` is a plain
    linear pre-encode;
  * positions: the sinusoidal table for the distances T' - 1 .. -(T' - 1) of the batch's longest item (attention.py:155-168), projected through each
    layer's ``linear_pos`` once per call; row ``T' - 1`` is distance 0 for every item (rel_shift is out[i, j] = bd[i, T - 1 - i + j]);
  * layer: LayerNorm -> linear1 (SiLU) -> linear2 with ``res=`` (the half-step's 0.5 folded into its weight and bias: exact) -> LayerNorm -> one fused
    q | k | v GEMM -> ``relpos_attention`` -> out projection with ``res=`` -> LayerNorm -> pointwise conv 1 -> ``glu_dwconv_silu`` (depthwise bias and
    the BatchNorm running statistics folded into its taps in float64) -> pointwise conv 2 with ``res=`` -> the second feed-forward -> LayerNorm.

Weights travel as fp16 images with fp16 hi + lo activations (precision 4) like every other engine here; the depthwise taps, the 3 x 3 stencils, the
LayerNorm parameters and the position biases stay float32.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import torch

from .... import ops
from ....ops import ACT_LEAKY, ACT_SILU

BN_EPS = 1e-5   # mlx.nn.BatchNorm's default


@dataclass
class ConformerArgs:
    feat_in: int  # mel-log
    n_layers: int
    d_model: int
    n_heads: int
    ff_expansion_factor: int
    subsampling_factor: int
    self_attention_model: str
    subsampling: str
    conv_kernel_size: int
    subsampling_conv_channels: int
    pos_emb_max_len: int
    causal_downsampling: bool = False
    use_bias: bool = True
    xscaling: bool = False
    pos_bias_u: Optional[torch.Tensor] = None
    pos_bias_v: Optional[torch.Tensor] = None
    subsampling_conv_chunking_factor: int = 1


def subsampled_len(n: int) -> int:
    """k = 3, stride 2, pad 1 (conformer.py:241-247), in integers."""
    return (n - 1) // 2 + 1


def n_stages(args: ConformerArgs) -> int:
    return int(math.log(args.subsampling_factor, 2)) if args.subsampling_factor > 1 else 0


def final_freq_dim(args: ConformerArgs) -> int:
    f = args.feat_in
    for _ in range(n_stages(args)):
        f = subsampled_len(f)
    return f


def rel_positions(T: int, d_model: int) -> torch.Tensor:
    """RelPositionalEncoding (attention.py:155-187) for ``input_len == T``: [2 T - 1, d_model], row m is distance T - 1 - m, float32 on the host."""
    positions = torch.arange(T - 1, -T, -1, dtype=torch.int32)[:, None].to(torch.float32)
    div_term = torch.exp(torch.arange(0, d_model, 2, dtype=torch.float32) * -(math.log(10000.0) / d_model))
    pe = torch.zeros((2 * T - 1, d_model), dtype=torch.float32)
    pe[:, 0::2] = torch.sin(positions * div_term)
    pe[:, 1::2] = torch.cos(positions * div_term)
    return pe


def expected_shapes(args: ConformerArgs, prefix: str = "encoder.") -> Dict[str, Tuple[int, ...]]:
    """Parameter name -> shape of ``Conformer(args)`` (the reference's names, MLX conv layouts)."""
    d, ff, H, K, C = args.d_model, args.d_model * args.ff_expansion_factor, args.n_heads, args.conv_kernel_size, args.subsampling_conv_channels
    s: Dict[str, Tuple[int, ...]] = {}

    def lin(name, n, k, bias=True):
        s[name + ".weight"] = (n, k)
        if bias:
            s[name + ".bias"] = (n,)

    def conv(name, shape, bias=True):
        s[name + ".weight"] = shape
        if bias:
            s[name + ".bias"] = (shape[0],)

    if args.subsampling_factor > 1:
        conv(prefix + "pre_encode.conv.0", (C, 3, 3, 1))
        for i in range(n_stages(args) - 1):
            conv(prefix + f"pre_encode.conv.{2 + 3 * i}", (C, 3, 3, 1))
            conv(prefix + f"pre_encode.conv.{3 + 3 * i}", (C, 1, 1, C))
        lin(prefix + "pre_encode.out", d, C * final_freq_dim(args))
    else:
        lin(prefix + "pre_encode", d, args.feat_in)
    for i in range(args.n_layers):
        p = prefix + f"layers.{i}."
        for n in ("norm_feed_forward1", "norm_self_att", "norm_conv", "norm_feed_forward2", "norm_out"):
            s[p + n + ".weight"], s[p + n + ".bias"] = (d,), (d,)
        for f in ("feed_forward1", "feed_forward2"):
            lin(p + f + ".linear1", ff, d, args.use_bias)
            lin(p + f + ".linear2", d, ff, args.use_bias)
        for n in ("linear_q", "linear_k", "linear_v", "linear_out"):
            lin(p + "self_attn." + n, d, d, args.use_bias)
        lin(p + "self_attn.linear_pos", d, d, False)
        s[p + "self_attn.pos_bias_u"], s[p + "self_attn.pos_bias_v"] = (H, d // H), (H, d // H)
        conv(p + "conv.pointwise_conv1", (2 * d, 1, d), args.use_bias)
        conv(p + "conv.depthwise_conv", (d, K, 1), args.use_bias)
        for n in ("weight", "bias", "running_mean", "running_var"):
            s[p + "conv.batch_norm." + n] = (d,)
        conv(p + "conv.pointwise_conv2", (d, 1, d), args.use_bias)
    return s


def check_args(args: ConformerArgs):
    if args.self_attention_model != "rel_pos":
        raise ValueError(f"Conformer: self_attention_model {args.self_attention_model!r}: only 'rel_pos' can run (the reference's plain attention reads an "
                         "attribute that is never set)")
    if args.subsampling_factor > 1 and (args.subsampling != "dw_striding" or args.causal_downsampling):
        raise NotImplementedError("Other subsampling haven't been implemented yet!")
    if args.subsampling_factor < 1 or args.subsampling_factor & (args.subsampling_factor - 1):
        raise ValueError(f"Conformer: subsampling_factor {args.subsampling_factor} is not a power of two")
    if args.conv_kernel_size % 2 == 0 or args.conv_kernel_size > ops.GLU_DWCONV_MAX_TAPS:
        raise ValueError(f"Conformer: conv_kernel_size {args.conv_kernel_size} must be odd and at most {ops.GLU_DWCONV_MAX_TAPS}")
    if args.d_model % args.n_heads or args.d_model // args.n_heads not in (64, 128):
        raise ValueError(f"Conformer: head width {args.d_model}/{args.n_heads} is not 64 or 128 (the widths relpos_attention is built for)")
    if args.subsampling_factor > 1 and final_freq_dim(args) < 1:
        raise ValueError("Non-positive final frequency dimension!")


class Conformer:
    """``Conformer(args)`` of the reference as an engine: ``__call__(mel [B, T, feat_in], lengths) -> (hidden [B, T', d_model], out_lengths int32 [B])``.
    ``weights``: the model's checkpoint under the reference's names; the encoder's parameters are the ones below ``prefix``."""

    def __init__(self, args: ConformerArgs, weights: Dict[str, torch.Tensor], device="cuda:0", prefix: str = "encoder.", precision: int = 4):
        check_args(args)
        ops.require_gpu()
        assert precision in (3, 4)
        self.args, self.device, self.prefix, self.precision = args, torch.device(device), prefix, precision
        self._pos_cache: Optional[Tuple[int, List[torch.Tensor]]] = None
        self.load_weights(weights)

    # ------------------------------------------------------------------ checkpoint handling
    def load_weights(self, weights: Dict[str, torch.Tensor]):
        a, dev, pre = self.args, self.device, self.prefix
        shapes = expected_shapes(a, pre)
        w = {k: torch.as_tensor(v).detach().to(torch.float32).cpu() for k, v in dict(weights).items() if k.startswith(pre)}
        miss = [k for k in shapes if k not in w]
        if miss:
            raise ValueError(f"Conformer.load_weights: missing parameters {miss[:4]}{' ...' if len(miss) > 4 else ''}")
        extra = [k for k in w if k not in shapes]
        if extra:
            raise ValueError(f"Conformer.load_weights: unexpected parameters {extra[:4]}{' ...' if len(extra) > 4 else ''}")
        for k, s in shapes.items():
            if tuple(w[k].shape) != s:
                raise ValueError(f"Conformer.load_weights: {k} has shape {tuple(w[k].shape)}, expected {s}")
        d, C = a.d_model, a.subsampling_conv_channels

        def lin(name, scale=1.0):
            wt, b = w[pre + name + ".weight"], w.get(pre + name + ".bias")
            wt = wt.reshape(wt.shape[0], -1)   # [n, 1, k] pointwise convs are linears
            return ops.pack_conv(wt * scale, None if b is None else b * scale, dev, f16=True)

        def vec(name):
            return w[pre + name].contiguous().to(dev)

        if a.subsampling_factor > 1:
            F = final_freq_dim(a)
            self.sub_first = (w[pre + "pre_encode.conv.0.weight"].reshape(C, 3, 3).contiguous().to(dev), vec("pre_encode.conv.0.bias"))
            self.sub_stages = []
            for i in range(n_stages(a) - 1):
                dw, pw = f"pre_encode.conv.{2 + 3 * i}", f"pre_encode.conv.{3 + 3 * i}"
                self.sub_stages.append((w[pre + dw + ".weight"].reshape(C, 3, 3).contiguous().to(dev), vec(dw + ".bias"), lin(pw)))
            wo = w[pre + "pre_encode.out.weight"].reshape(d, C, F).transpose(1, 2).reshape(d, F * C)   # column c * F + f -> f * C + c
            self.sub_out = ops.pack_conv(wo, w[pre + "pre_encode.out.bias"], dev, f16=True)
        else:
            self.sub_out = lin("pre_encode")
        self.layers = []
        for i in range(a.n_layers):
            p = f"layers.{i}."
            cat = lambda names, suf: torch.cat([w[pre + p + n + suf] for n in names])
            qkv_names = ("self_attn.linear_q", "self_attn.linear_k", "self_attn.linear_v")
            # BatchNorm on running statistics and the depthwise bias, folded in float64 (conformer.py:85-86)
            bn = {n: w[pre + p + "conv.batch_norm." + n].double() for n in ("weight", "bias", "running_mean", "running_var")}
            s = bn["weight"] / torch.sqrt(bn["running_var"] + BN_EPS)
            b_dw = w[pre + p + "conv.depthwise_conv.bias"].double() if a.use_bias else torch.zeros(d, dtype=torch.float64)
            dw_w = (s[:, None] * w[pre + p + "conv.depthwise_conv.weight"][:, :, 0].double()).to(torch.float32).contiguous().to(dev)
            dw_b = (s * (b_dw - bn["running_mean"]) + bn["bias"]).to(torch.float32).contiguous().to(dev)
            self.layers.append(dict(
                norm_ff1=(vec(p + "norm_feed_forward1.weight"), vec(p + "norm_feed_forward1.bias")),
                ff1_a=lin(p + "feed_forward1.linear1"), ff1_b=lin(p + "feed_forward1.linear2", 0.5),
                norm_att=(vec(p + "norm_self_att.weight"), vec(p + "norm_self_att.bias")),
                qkv=ops.pack_conv(cat(qkv_names, ".weight"), cat(qkv_names, ".bias") if a.use_bias else None, dev, f16=True),
                pos=lin(p + "self_attn.linear_pos"), out=lin(p + "self_attn.linear_out"),
                bias_u=vec(p + "self_attn.pos_bias_u").reshape(-1), bias_v=vec(p + "self_attn.pos_bias_v").reshape(-1),
                norm_conv=(vec(p + "norm_conv.weight"), vec(p + "norm_conv.bias")),
                pw1=lin(p + "conv.pointwise_conv1"), dw_w=dw_w, dw_b=dw_b, pw2=lin(p + "conv.pointwise_conv2"),
                norm_ff2=(vec(p + "norm_feed_forward2.weight"), vec(p + "norm_feed_forward2.bias")),
                ff2_a=lin(p + "feed_forward2.linear1"), ff2_b=lin(p + "feed_forward2.linear2", 0.5),
                norm_out=(vec(p + "norm_out.weight"), vec(p + "norm_out.bias"))))
        self._pos_cache = None
        return self

    # ------------------------------------------------------------------ forward
    def _f(self, *shape):
        return torch.empty(shape, dtype=torch.float32, device=self.device)

    def out_lengths(self, lengths: List[int]) -> List[int]:
        for _ in range(n_stages(self.args)):
            lengths = [subsampled_len(n) for n in lengths]
        return lengths

    def _pre_encode(self, mel: torch.Tensor, lens: List[int]) -> Tuple[torch.Tensor, List[int]]:
        a, dev, prec = self.args, self.device, self.precision
        B, T, F = mel.shape
        i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
        scale = math.sqrt(a.d_model) if a.xscaling else 1.0
        if a.subsampling_factor == 1:
            x = self._f(B, T, a.d_model)
            ops.conv_gemm(mel, self.sub_out, x, out_scale=scale, precision=prec)
            return x, lens
        C = a.subsampling_conv_channels
        lens1 = [subsampled_len(n) for n in lens]
        T1, F1 = subsampled_len(T), subsampled_len(F)
        y = self._f(B, T1, F1, C)
        ops.stencil2d_k3s2(mel, self.sub_first[0], self.sub_first[1], y, relu=True, lens_in=i32(lens), lens_out=i32(lens1))
        lens, T, F = lens1, T1, F1
        for dw_w, dw_b, pw in self.sub_stages:
            lens1 = [subsampled_len(n) for n in lens]
            T1, F1 = subsampled_len(T), subsampled_len(F)
            z = self._f(B, T1, F1, C)
            ops.stencil2d_k3s2(y, dw_w, dw_b, z, lens_in=i32(lens), lens_out=i32(lens1))
            y = self._f(B, T1, F1, C)
            ops.conv_gemm(z.view(B, T1 * F1, C), pw, y.view(B, T1 * F1, C), post_act=ACT_LEAKY, post_slope=0.0, flatten=True, precision=prec)   # ReLU
            lens, T, F = lens1, T1, F1
        x = self._f(B, T, a.d_model)
        ops.conv_gemm(y.view(B, T, F * C), self.sub_out, x, out_scale=scale, precision=prec)
        return x, lens

    def _positions(self, T: int) -> List[torch.Tensor]:
        """Every layer's projected position table [2 T - 1, d_model] for a batch whose longest item has T frames."""
        if self._pos_cache is not None and self._pos_cache[0] == T:
            return self._pos_cache[1]
        pe = rel_positions(T, self.args.d_model).to(self.device)[None]
        tables = []
        for blk in self.layers:
            p = self._f(1, 2 * T - 1, self.args.d_model)
            ops.conv_gemm(pe, blk["pos"], p, precision=self.precision)
            tables.append(p[0])
        self._pos_cache = (T, tables)
        return tables

    def __call__(self, mel: torch.Tensor, lengths=None, *, return_layers: bool = False):
        """``return_layers``: a third result, dict(pre_encode, layers [n_layers], attn0, conv0) -- the subsampler's output (after ``xscaling``), every
        layer's output, and layer 0's attention-module and convolution-module outputs (before their residual adds)."""
        x, lens = self.pre_encode(mel, lengths)
        taps = dict(pre_encode=x.clone()) if return_layers else None
        out = self.encode(x, lens, return_layers=return_layers, inplace=True)
        if return_layers:
            taps.update(out[2])
            return out[0], out[1], taps
        return out

    def pre_encode(self, mel: torch.Tensor, lengths=None) -> Tuple[torch.Tensor, List[int]]:
        """The subsampler alone: mel [B, T, feat_in] -> (embeddings [B, T', d_model] after ``xscaling``, the items' T' as host integers)."""
        mel = torch.as_tensor(mel, dtype=torch.float32)
        if mel.dim() != 3 or mel.shape[2] != self.args.feat_in:
            raise ValueError(f"Conformer: mel must be [B, T, {self.args.feat_in}], got {tuple(mel.shape)}")
        B, T, _ = mel.shape
        lens0 = [T] * B if lengths is None else [int(v) for v in torch.as_tensor(lengths).reshape(-1).tolist()]
        if len(lens0) != B or min(lens0) < 1 or max(lens0) > T:
            raise ValueError(f"Conformer: lengths {lens0} do not fit a mel of shape {tuple(mel.shape)}")
        return self._pre_encode(mel.to(self.device).contiguous(), lens0)

    def encode(self, x: torch.Tensor, lens, *, return_layers: bool = False, inplace: bool = False):
        """The layers alone: pre-encoded embeddings ``x`` [B, T', d_model] (what ``_pre_encode`` returns, or a caller's own: a streaming state) and the
        items' valid frames ``lens`` -> (hidden [B, T', d_model], lengths int32 [B] on the device).  The layers work in place: ``inplace=True`` hands
        ``x`` over as their buffer, otherwise they run on a copy.  ``return_layers``: a third result, dict(layers, attn0, conv0)."""
        a, dev, prec = self.args, self.device, self.precision
        if x.dim() != 3 or x.shape[2] != a.d_model or x.dtype != torch.float32:
            raise ValueError(f"Conformer.encode: embeddings must be float32 [B, T, {a.d_model}], got {tuple(x.shape)}")
        lens = [int(v) for v in (lens.reshape(-1).tolist() if isinstance(lens, torch.Tensor) else lens)]
        if len(lens) != x.shape[0] or min(lens) < 1 or max(lens) > x.shape[1]:
            raise ValueError(f"Conformer.encode: lengths {lens} do not fit embeddings of shape {tuple(x.shape)}")
        x = x.to(dev).contiguous()
        if not inplace:
            x = x.clone()
        B = x.shape[0]
        Tp, d, H = x.shape[1], a.d_model, a.n_heads
        dh = d // H
        lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
        tables = self._positions(Tp)
        taps = dict(layers=[]) if return_layers else None
        xn, h, mid, qkv, att, pw = self._f(B, Tp, d), self._f(B, Tp, d), self._f(B, Tp, d * a.ff_expansion_factor), self._f(B, Tp, 3 * d), self._f(B, Tp, d), self._f(B, Tp, 2 * d)
        for i, blk in enumerate(self.layers):
            ops.layernorm(x, h, weight=blk["norm_ff1"][0], bias=blk["norm_ff1"][1])
            ops.conv_gemm(h, blk["ff1_a"], mid, post_act=ACT_SILU, precision=prec)
            ops.conv_gemm(mid, blk["ff1_b"], x, res=x, precision=prec)
            ops.layernorm(x, h, weight=blk["norm_att"][0], bias=blk["norm_att"][1])
            ops.conv_gemm(h, blk["qkv"], qkv, precision=prec)
            ops.relpos_attention(qkv[:, :, 0:d], qkv[:, :, d:2 * d], qkv[:, :, 2 * d:], tables[i], blk["bias_u"], blk["bias_v"], att, heads=H, dh=dh,
                                 center=Tp - 1, scale=dh ** -0.5, lens=lens_d)
            if return_layers and i == 0:
                taps["attn0"] = ops.conv_gemm(att, blk["out"], self._f(B, Tp, d), precision=prec)
            ops.conv_gemm(att, blk["out"], x, res=x, precision=prec)
            ops.layernorm(x, h, weight=blk["norm_conv"][0], bias=blk["norm_conv"][1])
            ops.conv_gemm(h, blk["pw1"], pw, precision=prec)
            ops.glu_dwconv_silu(pw, blk["dw_w"], blk["dw_b"], att, lens=lens_d)
            if return_layers and i == 0:
                taps["conv0"] = ops.conv_gemm(att, blk["pw2"], self._f(B, Tp, d), precision=prec)
            ops.conv_gemm(att, blk["pw2"], x, res=x, precision=prec)
            ops.layernorm(x, h, weight=blk["norm_ff2"][0], bias=blk["norm_ff2"][1])
            ops.conv_gemm(h, blk["ff2_a"], mid, post_act=ACT_SILU, precision=prec)
            ops.conv_gemm(mid, blk["ff2_b"], x, res=x, precision=prec)
            ops.layernorm(x, xn, weight=blk["norm_out"][0], bias=blk["norm_out"][1])
            x, xn = xn, x
            if return_layers:
                taps["layers"].append(x.clone())
        return (x, lens_d, taps) if return_layers else (x, lens_d)
