"""The mask estimator of MossFormer2 SE as a host schedule: ``MossFormer_MaskNet`` -> ``Computation_Block`` -> ``MossFormerM`` ->
``MossFormerBlock_GFSMN`` (mossformer_masknet.py:122-205, computation_block.py:71-100, mossformerm.py:72-88, mossformerblock_gfsmn.py:89-106,
flash_sharea_ffconvm.py:119-188, gated_fsmn_block.py:129-160).  Activations stay channels-last ``[B, T, C]``; ``lens`` (int32 [B], None for equal
lengths) marks the valid rows of a right-padded batch and every launch that mixes rows takes it, so padding never reaches a valid row.

Per layer (FLASH, then the Gated-FSMN block):
  shift_scalenorm -> conv_gemm x 2 (to_hidden, to_qk: SiLU; each branch's ScaleNorm g is the GEMM's input scale) into one [4 C + 128] row ->
  ONE dwconv for both ConvModules (k = 17, the residual folded into the centre tap) -> gau_kv -> gau_attention (gate included) ->
  shift_scalenorm(shift = 0, g) -> conv_gemm + SiLU -> dwconv -> residual add;
  conv_gemm + PReLU (LEAKY at the learned slope) -> layernorm(1e-8) -> affine-free layernorm(1e-5) -> conv_gemm x 2 (to_u, to_v: each branch's
  LayerNorm weight / bias is the GEMM's input scale / shift) into one 512 row -> ONE dwconv -> conv_gemm + ReLU (fsmn.linear) -> conv_gemm
  (fsmn.project) -> gated_fsmn (in place on the block's normalised input, its residual) -> layernorm(1e-8) -> conv_gemm with the residual epilogue.
The per-branch norm parameters ride as ``pre_scale`` / ``pre_shift`` instead of being multiplied into the weights: the linears run on fp16 weight
images (precision 4) and a product g * W would be rounded to fp16 once more.  The residual add behind ``to_out`` is ``group_norm_apply`` with unit
coefficients.  ``conv1d_out`` computes speaker 0's ``out_channels`` columns only: the reference computes both speakers and returns the first.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, List, Optional

import numpy as np
import torch

from .... import ops
from .config import MossFormer2SEConfig

INNER = 256          # Gated_FSMN_Block(inner_channels=256) (mossformerblock_gfsmn.py:67-69)
LORDER = 20          # Gated_FSMN(lorder=20): 2 * 20 - 1 = 39 taps (gated_fsmn_block.py:102-107, unideepfsmn.py:58)
DW_TAPS = 17         # ConvModule(kernel_size=17) (convmodule.py:28)
QK = ops.GAU_DIM     # query_key_dim
NORM_EPS = 1e-8      # ScaleNorm, CLayerNorm, MossFormerM.norm, GroupNorm and GlobalLayerNorm
LN_EPS = 1e-5        # nn.LayerNorm of Gated_FSMN's FFConvM branches
P = "model.mossformer."


def expected_shapes(c: MossFormer2SEConfig) -> Dict[str, tuple]:
    """Every parameter of the reference's module tree below ``MossFormer2SEModel.model`` (what ``load_weights`` updates), in a fixed order.
    ``pos_enc.inv_freq`` is a plain array attribute there, so it is a parameter too."""
    C, s = c.out_channels, {}
    s[P + "norm.weight"], s[P + "norm.bias"] = (c.in_channels, 1), (c.in_channels, 1)
    s[P + "conv1d_encoder.weight"] = (C, 1, c.in_channels)
    s[P + "pos_enc.scale"], s[P + "pos_enc.inv_freq"] = (1,), (C // 2,)

    def ffconvm(p, din, dout, layernorm):
        if layernorm:
            s[p + "norm.weight"], s[p + "norm.bias"] = (din,), (din,)
        else:
            s[p + "norm.g"] = (1,)
        s[p + "linear.weight"], s[p + "linear.bias"] = (dout, din), (dout,)
        s[p + "conv_module.weight"] = (dout, DW_TAPS, 1)

    m = P + "mdl.intra_mdl.mossformerM."
    for i in range(c.num_blocks):
        f = f"{m}layers.{i}."
        ffconvm(f + "to_hidden.", C, 4 * C, False)
        ffconvm(f + "to_qk.", C, QK, False)
        s[f + "qk_offset_scale.gamma"], s[f + "qk_offset_scale.beta"] = (4, QK), (4, QK)
        ffconvm(f + "to_out.", 2 * C, C, False)
    for i in range(c.num_blocks):
        f = f"{m}fsmn.{i}."
        s[f + "conv1.weight"], s[f + "conv1.bias"] = (INNER, 1, C), (INNER,)
        s[f + "prelu.weight"] = (1,)
        for n in ("norm1", "norm2"):
            s[f + n + ".weight"], s[f + n + ".bias"] = (INNER,), (INNER,)
        ffconvm(f + "gated_fsmn.to_u.", INNER, INNER, True)
        ffconvm(f + "gated_fsmn.to_v.", INNER, INNER, True)
        s[f + "gated_fsmn.fsmn.linear.weight"], s[f + "gated_fsmn.fsmn.linear.bias"] = (INNER, INNER), (INNER,)
        s[f + "gated_fsmn.fsmn.project.weight"] = (INNER, INNER)
        s[f + "gated_fsmn.fsmn.conv1.weight"] = (INNER, 2 * LORDER - 1, 1, 1)
        s[f + "conv2.weight"], s[f + "conv2.bias"] = (C, 1, INNER), (C,)
    s[P + "mdl.intra_mdl.norm.weight"], s[P + "mdl.intra_mdl.norm.bias"] = (C,), (C,)
    s[P + "mdl.intra_norm.weight"], s[P + "mdl.intra_norm.bias"] = (C,), (C,)
    s[P + "conv1d_out.weight"], s[P + "conv1d_out.bias"] = (2 * C, 1, C), (2 * C,)
    s[P + "conv1_decoder.weight"] = (c.out_channels_final, 1, C)
    s[P + "prelu.weight"] = (1,)
    for n in ("output", "output_gate"):
        s[P + n + ".weight"], s[P + n + ".bias"] = (C, 1, C), (C,)
    return s


def sinu_inv_freq(dim: int) -> np.ndarray:
    """ScaledSinuEmbedding's buffer (scaledsinuembedding.py:34-35), float32."""
    return (1.0 / (np.float32(10000.0) ** (np.arange(0, dim, 2, dtype=np.float32) / np.float32(dim)))).astype(np.float32)


def make_mossformer2_weights(config: MossFormer2SEConfig, seed: int = 0, gain: float = 1.0, qk_gain: float = 2.0) -> Dict[str, torch.Tensor]:
    """A seeded checkpoint under the reference's names: matrices uniform in +-sqrt(3 / fan_in) * ``gain`` (``to_qk`` times ``qk_gain`` more, so that
    the ReLU^2 term carries weight beside the linear one), depthwise filters uniform in +-sqrt(3 / taps), biases 0.1 N(0, 1), norm weights and the
    ScaleNorm g 1 + 0.1 N(0, 1), OffsetScale gamma 1 + 0.1 N(0, 1) / beta 0.1 N(0, 1), PReLU slopes 0.25.  ``output.bias`` is centred on 1 and ``conv1_decoder.weight`` on 0.3 sqrt(64 / C) of its half-width: the tail is
    tanh x sigmoid into a bias-free ReLU, and with centred weights about half of the 961 mask columns stay at zero for a whole clip; so shifted, every
    column moves and one to two per cent of the mask are exact zeros.  float32 tensors holding fp16 values."""
    g = torch.Generator().manual_seed(seed)
    w: Dict[str, torch.Tensor] = {}
    for name, shape in expected_shapes(config).items():
        if name.endswith("inv_freq"):
            w[name] = torch.from_numpy(sinu_inv_freq(config.out_channels))
            continue
        if name.endswith("prelu.weight"):
            t = torch.full(shape, 0.25)
        elif name.endswith("pos_enc.scale"):
            t = torch.full(shape, 0.5)
        elif name.endswith(".bias") or name.endswith(".beta"):
            t = 0.1 * torch.randn(shape, generator=g) + (1.0 if name == P + "output.bias" else 0.0)
        elif name.endswith((".g", ".gamma")) or (name.endswith(".weight") and (len(shape) == 1 or shape[-1] == 1 and len(shape) == 2)):
            t = 1.0 + 0.1 * torch.randn(shape, generator=g)
        elif "conv_module" in name or "fsmn.conv1" in name:
            t = (torch.rand(shape, generator=g) * 2 - 1) * math.sqrt(3.0 / shape[1])
        else:
            t = (torch.rand(shape, generator=g) * 2 - 1) * math.sqrt(3.0 / shape[-1]) * gain * (qk_gain if "to_qk.linear.weight" in name else 1.0)
            if name == P + "conv1_decoder.weight":
                t = t + 0.3 * math.sqrt(64.0 / shape[-1]) * math.sqrt(3.0 / shape[-1])   # the same zero share at every width
        w[name] = t.to(torch.float16).to(torch.float32)
    return w


@dataclass
class _Flash:
    to_hidden: ops.PackedConv
    to_qk: ops.PackedConv
    g_hidden: tuple
    g_qk: tuple
    hq_dw: torch.Tensor
    gamma: torch.Tensor
    beta: torch.Tensor
    g_out: torch.Tensor
    to_out: ops.PackedConv
    out_dw: torch.Tensor


@dataclass
class _Fsmn:
    conv1: ops.PackedConv
    slope: float
    norm1: tuple
    to_u: ops.PackedConv
    to_v: ops.PackedConv
    ln_u: tuple
    ln_v: tuple
    uv_dw: torch.Tensor
    linear: ops.PackedConv
    project: ops.PackedConv
    memory: torch.Tensor
    norm2: tuple
    conv2: ops.PackedConv


class MossFormerMaskNet:
    """features [B, T, in_channels] -> mask [B, T, out_channels_final] on the device."""

    def __init__(self, config: MossFormer2SEConfig, device):
        c = config
        if c.out_channels % 16 or not 16 <= c.out_channels <= ops.GAU_MAX_E // 4:
            raise ValueError(f"MossFormer2: out_channels must be a multiple of 16 in [16, {ops.GAU_MAX_E // 4}] (got {c.out_channels})")
        self.config, self.device = config, torch.device(device)
        self._rope = (None, None, 0)
        self._pos = {}
        self._pre_rows = {}
        self.flash: List[_Flash] = []
        self.fsmn: List[_Fsmn] = []

    # ------------------------------------------------------------------ checkpoint
    def load(self, w: Dict[str, torch.Tensor]):
        c, dev = self.config, self.device
        C = c.out_channels

        def lin(name, bias=True, rows=None):
            wt = w[name + ".weight"]
            wt = wt.reshape(wt.shape[0], -1) if wt.dim() == 3 else wt
            b = w[name + ".bias"] if bias else None
            if rows is not None:
                wt, b = wt[:rows], (None if b is None else b[:rows])
            return ops.pack_conv(wt.contiguous(), b, dev, f16=True)

        def vec(name):
            return w[name].reshape(-1).contiguous().to(dev)

        def dw(*names):
            """The ConvModules of ``names`` side by side: [sum of channels, 17] with x + dw(x) folded into the centre tap."""
            t = torch.cat([w[n + ".conv_module.weight"].reshape(-1, DW_TAPS) for n in names]).clone()
            t[:, DW_TAPS // 2] += 1.0
            return t.contiguous().to(dev)

        def pre(scale, shift, n):
            """(scale, shift) rows for conv_gemm's prologue, one row shared by every item."""
            ld = ops.round_up(n, 32)
            sc, sh = torch.zeros(1, ld), torch.zeros(1, ld)
            sc[0, :n], sh[0, :n] = scale, shift
            return sc.to(dev), sh.to(dev)

        self.in_norm = (vec(P + "norm.weight"), vec(P + "norm.bias"))
        self.encoder = lin(P + "conv1d_encoder", bias=False)
        self.pos_scale = float(w[P + "pos_enc.scale"].reshape(-1)[0])
        self.inv_freq = w[P + "pos_enc.inv_freq"].reshape(-1).numpy().astype(np.float32) if P + "pos_enc.inv_freq" in w else sinu_inv_freq(C)
        self._pos, self._pre_rows = {}, {}
        m = P + "mdl.intra_mdl.mossformerM."
        self.flash, self.fsmn = [], []
        for i in range(c.num_blocks):
            f = f"{m}layers.{i}."
            self.flash.append(_Flash(lin(f + "to_hidden.linear"), lin(f + "to_qk.linear"), pre(float(w[f + "to_hidden.norm.g"][0]), 0.0, C),
                                     pre(float(w[f + "to_qk.norm.g"][0]), 0.0, C), dw(f + "to_hidden", f + "to_qk"),
                                     w[f + "qk_offset_scale.gamma"].contiguous().to(dev), w[f + "qk_offset_scale.beta"].contiguous().to(dev),
                                     vec(f + "to_out.norm.g"), lin(f + "to_out.linear"), dw(f + "to_out")))
            f = f"{m}fsmn.{i}."
            gf = f + "gated_fsmn."
            self.fsmn.append(_Fsmn(lin(f + "conv1"), float(w[f + "prelu.weight"].reshape(-1)[0]), (vec(f + "norm1.weight"), vec(f + "norm1.bias")),
                                   lin(gf + "to_u.linear"), lin(gf + "to_v.linear"),
                                   pre(w[gf + "to_u.norm.weight"], w[gf + "to_u.norm.bias"], INNER), pre(w[gf + "to_v.norm.weight"], w[gf + "to_v.norm.bias"], INNER),
                                   dw(gf + "to_u", gf + "to_v"), lin(gf + "fsmn.linear"), lin(gf + "fsmn.project", bias=False),
                                   w[gf + "fsmn.conv1.weight"].reshape(INNER, 2 * LORDER - 1).contiguous().to(dev),
                                   (vec(f + "norm2.weight"), vec(f + "norm2.bias")), lin(f + "conv2")))
        self.mdl_norm = (vec(P + "mdl.intra_mdl.norm.weight"), vec(P + "mdl.intra_mdl.norm.bias"))
        self.intra_norm = (vec(P + "mdl.intra_norm.weight"), vec(P + "mdl.intra_norm.bias"))
        self.out_slope = float(w[P + "prelu.weight"].reshape(-1)[0])
        self.conv_out = lin(P + "conv1d_out", rows=C)           # speaker 0's columns
        self.output, self.output_gate = lin(P + "output"), lin(P + "output_gate")
        self.decoder = lin(P + "conv1_decoder", bias=False)
        ld = ops.round_up(C, 32)
        self._unit = (torch.ones(1, ld, device=dev), torch.zeros(1, ld, device=dev))

    # ------------------------------------------------------------------ tables
    def _rope_tables(self, n: int):
        cos, sin, rows = self._rope
        if rows < n:
            rows = ops.round_up(n, ops.GAU_GROUP)
            cos, sin = ops.gau_rope_tables(rows, self.device)
            self._rope = (cos, sin, rows)
        return cos, sin

    def _pos_table(self, B: int, T: int) -> torch.Tensor:
        """ScaledSinuEmbedding (scaledsinuembedding.py:66-83): float32 products of position and inverse frequency, sines then cosines, times scale."""
        if (B, T) not in self._pos:
            ang = np.arange(T, dtype=np.float32)[:, None] * self.inv_freq[None, :]
            emb = np.concatenate([np.sin(ang), np.cos(ang)], axis=-1).astype(np.float32) * np.float32(self.pos_scale)
            self._pos = {(B, T): torch.from_numpy(emb).to(self.device)[None].expand(B, -1, -1).contiguous()}   # one row block per item: conv_gemm's res
        return self._pos[(B, T)]

    def _rows(self, pr, B: int):
        """A one-row (scale, shift) pair as B contiguous rows (conv_gemm takes one coefficient row per item), kept per batch size."""
        key = (id(pr[0]), B)
        if key not in self._pre_rows:
            if len(self._pre_rows) > 4096:
                self._pre_rows.clear()
            self._pre_rows[key] = (pr[0].expand(B, -1).contiguous(), pr[1].expand(B, -1).contiguous())
        return self._pre_rows[key]

    def _f(self, *shape):
        return torch.empty(shape, dtype=torch.float32, device=self.device)

    # ------------------------------------------------------------------ forward
    def forward(self, feats: torch.Tensor, lens: Optional[torch.Tensor] = None, stages: Optional[dict] = None) -> torch.Tensor:
        c = self.config
        B, T, Cin = feats.shape
        C, E = c.out_channels, 4 * c.out_channels
        SILU, LEAKY, TANH = ops.ACT_SILU, ops.ACT_LEAKY, ops.ACT_TANH
        ex = lambda pr: self._rows(pr, B)
        rope = self._rope_tables(T)
        # GlobalLayerNorm over (channels, frames) of each item, folded into the encoder's prologue; then the positional table
        coef = ops.group_norm_coef(ops.group_norm_stats(feats, lens), T, Cin, self.in_norm[0], self.in_norm[1], eps=NORM_EPS, lens=lens)
        x0 = self._f(B, T, C)
        ops.conv_gemm(feats, self.encoder, x0, pre=coef, res=self._pos_table(B, T), precision=4)
        x = x0.clone()
        n, hq, vq, att, att_n = self._f(B, T, C), self._f(B, T, E + QK), self._f(B, T, E + QK), self._f(B, T, 2 * C), self._f(B, T, 2 * C)
        t1, t2 = self._f(B, T, C), self._f(B, T, C)
        kv, ws = self._f(B, QK, E), self._f(ops.gau_kv_workspace_floats(B, T, E))
        a, n1, ln, uv0, uv = self._f(B, T, INNER), self._f(B, T, INNER), self._f(B, T, INNER), self._f(B, T, 2 * INNER), self._f(B, T, 2 * INNER)
        f1, p, n2 = self._f(B, T, INNER), self._f(B, T, INNER), self._f(B, T, INNER)
        vu, qk = vq[:, :, :E], vq[:, :, E:]
        xu, xv = uv[:, :, :INNER], uv[:, :, INNER:]
        for i, (L, F) in enumerate(zip(self.flash, self.fsmn)):
            # ---- FLASH_ShareA_FFConvM
            ops.shift_scalenorm(x, n, eps=NORM_EPS, shift=True, lens=lens)
            ops.conv_gemm(n, L.to_hidden, hq[:, :, :E], pre=ex(L.g_hidden), post_act=SILU, precision=4)
            ops.conv_gemm(n, L.to_qk, hq[:, :, E:], pre=ex(L.g_qk), post_act=SILU, precision=4)
            ops.dwconv(hq, L.hq_dw, None, vq, pad=DW_TAPS // 2, lens_in=lens)
            ops.gau_kv(qk, vu, L.gamma, L.beta, rope, lens=lens, kv=kv, ws=ws)
            ops.gau_attention(qk, vu, kv, L.gamma, L.beta, rope, att, lens=lens)
            ops.shift_scalenorm(att, att_n, g=L.g_out, eps=NORM_EPS, shift=False, lens=lens)
            ops.conv_gemm(att_n, L.to_out, t1, post_act=SILU, precision=4)
            ops.dwconv(t1, L.out_dw, None, t2, pad=DW_TAPS // 2, lens_in=lens)
            ops.group_norm_apply(t2, ex(self._unit), x, x1=x)                       # x += to_out(...)
            if stages is not None and i == 0:
                stages["flash0"] = x.clone()
            # ---- Gated_FSMN_Block
            ops.conv_gemm(x, F.conv1, a, post_act=LEAKY, post_slope=F.slope, precision=4)
            ops.layernorm(a, n1, weight=F.norm1[0], bias=F.norm1[1], eps=NORM_EPS)
            ops.layernorm(n1, ln, eps=LN_EPS)
            ops.conv_gemm(ln, F.to_u, uv0[:, :, :INNER], pre=ex(F.ln_u), post_act=SILU, precision=4)
            ops.conv_gemm(ln, F.to_v, uv0[:, :, INNER:], pre=ex(F.ln_v), post_act=SILU, precision=4)
            ops.dwconv(uv0, F.uv_dw, None, uv, pad=DW_TAPS // 2, lens_in=lens)
            ops.conv_gemm(xu, F.linear, f1, post_act=LEAKY, post_slope=0.0, precision=4)   # ReLU
            ops.conv_gemm(f1, F.project, p, precision=4)
            ops.gated_fsmn(p, xu, xv, n1, F.memory, n1, lens=lens)
            ops.layernorm(n1, n2, weight=F.norm2[0], bias=F.norm2[1], eps=NORM_EPS)
            ops.conv_gemm(n2, F.conv2, x, res=x, precision=4)
            if stages is not None and i == 0:
                stages["fsmn0"] = x.clone()
        # MossFormerM.norm, Computation_Block's GroupNorm(1, C) and its skip
        ops.layernorm(x, n, weight=self.mdl_norm[0], bias=self.mdl_norm[1], eps=NORM_EPS)
        coef = ops.group_norm_coef(ops.group_norm_stats(n, lens), T, C, self.intra_norm[0], self.intra_norm[1], eps=NORM_EPS, lens=lens)
        ops.group_norm_apply(n, coef, t1, x1=x0)
        # PReLU, speaker 0 of conv1d_out, tanh(output) * sigmoid(output_gate), decoder + ReLU
        ops.conv_gemm(t1, self.conv_out, t2, pre_act=LEAKY, pre_slope=self.out_slope, precision=4)
        ops.conv_gemm(t2, self.output, n, post_act=TANH, precision=4)
        ops.conv_gemm(t2, self.output_gate, t1, precision=4)
        ops.head_gate(n, t1, heads=C, dh=1)
        mask = self._f(B, T, c.out_channels_final)
        ops.conv_gemm(n, self.decoder, mask, post_act=LEAKY, post_slope=0.0, precision=4)
        return mask   # rows at and beyond lens[b] are padding: the caller slices each item
