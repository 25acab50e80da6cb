"""Moonshine ASR on MI355X (stt/models/moonshine/moonshine.py): raw waveform -> three strided convs -> Transformer encoder with partial rotary
attention -> causal Transformer decoder with cross-attention -> greedy (or sampled) tokens.  Head widths are ``hidden_size / heads`` = 36 (tiny) and
52 (base): ``csrc/mid_attn.hip``.

The reference runs one clip per call.  ``generate_batch`` (new here) runs right-padded clips with lengths in lockstep; each item equals that item
alone.  ``generate`` is a batch of one.

Host schedule:

  * stem: the three valid, strided convs run as few-tap convs over regrouped rows ``[rows / s, s * C]`` with the tap count rounded up to a multiple
    of the stride by ZERO weights (conv1: 127 -> 128 taps = 2 taps of 64 samples; conv2: 7 -> 9 = 3 taps of 3 rows; conv3: 3 -> 4 = 2 taps of 2
    rows).  A zero weight times a non-finite value is NaN, so every buffer a regrouped conv reads is zero-filled first.  conv1 carries tanh as its
    epilogue and leaves the per-block statistics of what it stores (``stats=``, each item's ``T1`` valid rows only: ``lens_out``); ``GroupNorm(1, d)``
    is ``group_norm_coef(..., lens=, rep=3)`` on those partials, whose rows are the ``pre=`` operands of conv2 (the normalised tensor is never
    written); conv2 and conv3 carry the exact GELU;
  * encoder layer: ``layernorm`` (weight only) -> fused q | k | v ``conv_gemm`` -> ``partial_rope`` on q and k in place -> ``mid_attention`` under the
    items' frame counts -> ``o_proj`` with ``res=`` -> ``layernorm`` -> ``fc1`` (GELU) -> ``fc2`` with ``res=``; a final ``layernorm``;
  * decoder: the cross k | v of every layer are projected ONCE per utterance (the reference recomputes them every step); per step and layer
    q | k | v -> ``partial_rope`` with k rotated straight into its cache row -> causal ``mid_attention`` over ``cache[:, :pos + T]`` (the one-wavefront
    form at ``T <= 4``) -> ``o_proj`` -> cross ``mid_attention(lens_k = frames)`` -> ``fc2(silu(gate) * x)`` as ``swiglu`` over an ``fc1`` whose rows
    are interleaved at load (row 2 i = gate row I + i, row 2 i + 1 = row i); logits from the tied table (or ``proj_out``), arg-max and top-2 gap
    from ``ctc_rows``.  Caches are preallocated ``[B, max_tokens + 1, 2 kv_heads dh]`` (k | v side by side).  A row that emitted EOS keeps stepping
    with its token frozen and is cut on the host.  Linears are ``conv_gemm`` at precision 4 on fp16 weight images; the decoder's, at up to 8 rows
    (the decode step of up to 8 clips, a short teacher-forced call), are ``gemv`` on row-major fp16 images of the same weights, as
    ``WhisperEngine._linear`` chooses.

Not built, each raising by name: hub download, bf16 / quantised checkpoints, ``encoder_hidden_act`` other than ``gelu``, a head width outside
36 - 60 (64 and 128 are refused too: ``flash_attention`` is not routed here), audio shorter than 895 samples (no encoder frame).  Deliberately
absent from ``MODEL_REMAPPING`` and the generic loader, like Parakeet and SenseVoice.
"""
from __future__ import annotations

import json
import math
import time
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from .... import ops
from ....ops import ACT_GELU, ACT_TANH
from ..base import STTOutput
from .config import ModelConfig

LN_EPS = 1e-5       # mlx.nn.LayerNorm / GroupNorm default
GEMV_ROWS = 8       # rows up to which a decoder linear takes the GEMV (WhisperEngine._linear's choice for a decode step)
MIN_SAMPLES = 895   # the shortest clip with one encoder frame: T1 = 13, T2 = 3, T3 = 1


def stem_lengths(n: int) -> Tuple[int, int, int]:
    """Frames behind conv1 (K 127, stride 64), conv2 (K 7, stride 3) and conv3 (K 3, stride 2), all valid; 0s when the clip is too short."""
    t1 = (n - 127) // 64 + 1 if n >= 127 else 0
    t2 = (t1 - 7) // 3 + 1 if t1 >= 7 else 0
    t3 = (t2 - 3) // 2 + 1 if t2 >= 3 else 0
    return t1, t2, t3


def rotary_ndims(head_dim: int, factor: float) -> int:
    r = int(head_dim * factor)
    return r - (r % 2)


def expected_shapes(c: ModelConfig) -> Dict[str, Tuple[int, ...]]:
    """Parameter name -> shape of the reference's ``Model(config)`` (MLX conv layout [C_out, K, C_in])."""
    d, I, V = c.hidden_size, c.intermediate_size, c.vocab_size
    s: Dict[str, Tuple[int, ...]] = {}

    def attn(p, H, KH):
        dh = d // H
        for n, rows in (("q_proj", H * dh), ("k_proj", KH * dh), ("v_proj", KH * dh)):
            s[f"{p}.{n}.weight"] = (rows, d)
            if c.attention_bias:
                s[f"{p}.{n}.bias"] = (rows,)
        s[f"{p}.o_proj.weight"] = (d, H * dh)

    s["encoder.conv1.weight"] = (d, 127, 1)
    s["encoder.groupnorm.weight"], s["encoder.groupnorm.bias"] = (d,), (d,)
    s["encoder.conv2.weight"], s["encoder.conv2.bias"] = (2 * d, 7, d), (2 * d,)
    s["encoder.conv3.weight"], s["encoder.conv3.bias"] = (d, 3, 2 * d), (d,)
    for i in range(c.encoder_num_hidden_layers):
        p = f"encoder.layers.{i}"
        attn(p + ".self_attn", c.encoder_num_attention_heads, c.encoder_num_key_value_heads)
        s[p + ".mlp.fc1.weight"], s[p + ".mlp.fc1.bias"] = (I, d), (I,)
        s[p + ".mlp.fc2.weight"], s[p + ".mlp.fc2.bias"] = (d, I), (d,)
        s[p + ".input_layernorm.weight"] = s[p + ".post_attention_layernorm.weight"] = (d,)
    s["encoder.layer_norm.weight"] = (d,)
    s["decoder.embed_tokens.weight"] = (V, d)
    for i in range(c.decoder_num_hidden_layers):
        p = f"decoder.layers.{i}"
        attn(p + ".self_attn", c.decoder_num_attention_heads, c.decoder_num_key_value_heads)
        attn(p + ".encoder_attn", c.decoder_num_attention_heads, c.decoder_num_key_value_heads)
        s[p + ".mlp.fc1.weight"], s[p + ".mlp.fc1.bias"] = (2 * I, d), (2 * I,)
        s[p + ".mlp.fc2.weight"], s[p + ".mlp.fc2.bias"] = (d, I), (d,)
        s[p + ".input_layernorm.weight"] = s[p + ".post_attention_layernorm.weight"] = s[p + ".final_layernorm.weight"] = (d,)
    s["decoder.norm.weight"] = (d,)
    if not c.tie_word_embeddings:
        s["proj_out.weight"] = (V, d)
    return s


def make_moonshine_weights(config: ModelConfig, seed: int = 0, logit_gain: float = 6.0, eos_gain: float = 1.0) -> Dict[str, torch.Tensor]:
    """A seeded checkpoint under the reference's parameter names: matrices N(0, 1 / fan_in), biases 0.1 N(0, 1), norm weights 1 + 0.1 N(0, 1); the
    output table (the tied embedding, or ``proj_out``) ``logit_gain`` N(0, 1) / sqrt(d) with its EOS row scaled by ``eos_gain``.  float32 tensors
    holding fp16-representable values, like a checkpoint published in fp16 (the engine packs fp16 weight images)."""
    g = torch.Generator().manual_seed(seed)
    w: Dict[str, torch.Tensor] = {}
    out_name = "decoder.embed_tokens.weight" if config.tie_word_embeddings else "proj_out.weight"
    for name, shape in expected_shapes(config).items():
        if name.endswith(".bias") and "groupnorm" not in name:
            t = 0.1 * torch.randn(shape, generator=g)
        elif "norm" in name:
            t = (0.0 if name.endswith(".bias") else 1.0) + 0.1 * torch.randn(shape, generator=g)
        elif name == out_name:
            t = logit_gain * torch.randn(shape, generator=g) / math.sqrt(shape[-1])
            t[config.eos_token_id] *= eos_gain
        elif name == "decoder.embed_tokens.weight":
            t = torch.randn(shape, generator=g)
        else:
            fan_in = shape[-1] if len(shape) == 2 else shape[1] * shape[2]
            t = torch.randn(shape, generator=g) / math.sqrt(fan_in)
        w[name] = t.to(torch.float16).to(torch.float32)
    return w


class Model:
    """``Model(config)`` of the reference as an engine; ``weights`` omitted = a seeded checkpoint (the reference: freshly initialised)."""

    def __init__(self, config: Union[ModelConfig, dict], weights: Optional[Dict[str, torch.Tensor]] = None, device="cuda:0", seed: int = 0,
                 precision: int = 4):
        if isinstance(config, dict):
            config = ModelConfig.from_dict(config)
        c = config
        if c.encoder_hidden_act != "gelu":
            raise NotImplementedError(f"Moonshine: encoder_hidden_act {c.encoder_hidden_act!r} is not built (only 'gelu'; none of the published configs use another)")
        for side, H, KH in (("encoder", c.encoder_num_attention_heads, c.encoder_num_key_value_heads),
                            ("decoder", c.decoder_num_attention_heads, c.decoder_num_key_value_heads)):
            if c.hidden_size % H or H % KH:
                raise ValueError(f"Moonshine: {side} heads {H} / kv heads {KH} do not divide hidden_size {c.hidden_size}")
            if c.hidden_size // H not in ops.MID_ATTENTION_WIDTHS:
                raise NotImplementedError(f"Moonshine: {side} head width {c.hidden_size // H} is not one of {ops.MID_ATTENTION_WIDTHS} "
                                          "(the widths mid_attention is built for; 64 and 128 are not routed to flash_attention here)")
        ops.require_gpu()
        assert precision in (3, 4)
        self.config, self.device, self.precision = c, torch.device(device), precision
        self._tokenizer = None
        self._rope: Dict[int, Tuple[torch.Tensor, torch.Tensor]] = {}
        self.load_weights(make_moonshine_weights(c, seed) if weights is None else weights)

    @property
    def sample_rate(self) -> int:
        return 16000

    # ------------------------------------------------------------------ checkpoint handling
    def sanitize(self, weights: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        """The reference's rules: the ``model.`` prefix of encoder / decoder keys is stripped, ``proj_out.`` is dropped under tied embeddings, 3-D
        conv weights [C_out, C_in, K] (PyTorch) become [C_out, K, C_in] (MLX)."""
        out = {}
        for key, value in weights.items():
            new_key = key
            if key.startswith("model.encoder.") or key.startswith("model.decoder."):
                new_key = key[len("model."):]
            elif key.startswith("proj_out.") and self.config.tie_word_embeddings:
                continue
            value = torch.as_tensor(value)
            if "conv" in new_key and "weight" in new_key and value.dim() == 3:
                value = value.permute(0, 2, 1)
            out[new_key] = value
        return out

    def load_weights(self, weights, strict: bool = True):
        c, dev = self.config, self.device
        weights = dict(weights)
        for k, v in weights.items():
            dt = torch.as_tensor(v).dtype
            if dt == torch.bfloat16:
                raise NotImplementedError("Moonshine.load_weights: bf16 checkpoints are not built (the weight images are fp16)")
            if not dt.is_floating_point:
                raise NotImplementedError(f"Moonshine.load_weights: quantised checkpoints are not built ({k} is {dt})")
        w = {k: torch.as_tensor(v).detach().to(torch.float32).cpu() for k, v in weights.items()}
        shapes = expected_shapes(c)
        miss = [k for k in shapes if k not in w]
        if miss:
            raise ValueError(f"Moonshine.load_weights: missing parameters {miss[:4]}{' ...' if len(miss) > 4 else ''}")
        extra = [k for k in w if k not in shapes]
        if extra and strict:
            raise ValueError(f"Moonshine.load_weights: unexpected parameters {extra[:4]}{' ...' if len(extra) > 4 else ''}")
        for k, s in shapes.items():
            if tuple(w[k].shape) != s:
                raise ValueError(f"Moonshine.load_weights: {k} has shape {tuple(w[k].shape)}, expected {s}")
        d, I = c.hidden_size, c.intermediate_size
        pack = lambda wt, b=None: ops.pack_conv(wt.contiguous(), b, dev, f16=True)
        vec = lambda n: w[n].contiguous().to(dev)
        # a decoder linear: the MFMA image for many rows and the row-major image for the GEMV at up to GEMV_ROWS rows
        dlin = lambda wt, b=None: (pack(wt, b), ops.pack_rowmajor16(wt.contiguous(), b, dev, f16=True))

        def regroup(wt, stride):   # [C_out, K, C] -> taps padded with zeros to a multiple of the stride -> [C_out, K' / s, s C]
            co, K, ci = wt.shape
            Kp = -(-K // stride) * stride
            z = torch.zeros((co, Kp, ci), dtype=torch.float32)
            z[:, :K] = wt
            return z.reshape(co, Kp // stride, stride * ci)

        def cat_lin(p, names):
            wt = torch.cat([w[f"{p}.{n}.weight"] for n in names], 0)
            b = torch.cat([w[f"{p}.{n}.bias"] for n in names], 0) if c.attention_bias else None
            return dlin(wt, b) if p.startswith("decoder.") else pack(wt, b)

        self.conv1 = pack(regroup(w["encoder.conv1.weight"], 64))
        self.gn = (vec("encoder.groupnorm.weight"), vec("encoder.groupnorm.bias"))
        self.conv2 = pack(regroup(w["encoder.conv2.weight"], 3), w["encoder.conv2.bias"])
        self.conv3 = pack(regroup(w["encoder.conv3.weight"], 2), w["encoder.conv3.bias"])
        self.enc_layers = []
        for i in range(c.encoder_num_hidden_layers):
            p = f"encoder.layers.{i}"
            self.enc_layers.append(dict(ln1=vec(p + ".input_layernorm.weight"), qkv=cat_lin(p + ".self_attn", ("q_proj", "k_proj", "v_proj")),
                                        o=pack(w[p + ".self_attn.o_proj.weight"]), ln2=vec(p + ".post_attention_layernorm.weight"),
                                        fc1=pack(w[p + ".mlp.fc1.weight"], w[p + ".mlp.fc1.bias"]), fc2=pack(w[p + ".mlp.fc2.weight"], w[p + ".mlp.fc2.bias"])))
        self.enc_norm = vec("encoder.layer_norm.weight")
        self.embed = vec("decoder.embed_tokens.weight")
        self.dec_layers = []
        for i in range(c.decoder_num_hidden_layers):
            p = f"decoder.layers.{i}"
            f1w, f1b = self.interleave_fc1(w[p + ".mlp.fc1.weight"], w[p + ".mlp.fc1.bias"])
            self.dec_layers.append(dict(ln1=vec(p + ".input_layernorm.weight"), qkv=cat_lin(p + ".self_attn", ("q_proj", "k_proj", "v_proj")),
                                        o=dlin(w[p + ".self_attn.o_proj.weight"]), ln2=vec(p + ".post_attention_layernorm.weight"),
                                        cq=cat_lin(p + ".encoder_attn", ("q_proj",)), ckv=cat_lin(p + ".encoder_attn", ("k_proj", "v_proj")),
                                        co=dlin(w[p + ".encoder_attn.o_proj.weight"]), ln3=vec(p + ".final_layernorm.weight"),
                                        fc1=dlin(f1w, f1b), fc2=dlin(w[p + ".mlp.fc2.weight"], w[p + ".mlp.fc2.bias"])))
        self.dec_norm = vec("decoder.norm.weight")
        self.head = dlin(w["decoder.embed_tokens.weight"] if c.tie_word_embeddings else w["proj_out.weight"])
        return self

    @staticmethod
    def interleave_fc1(weight: torch.Tensor, bias: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """The decoder MLP is ``fc2(silu(gate) * x)`` with ``x, gate = split(fc1(h), 2)``; ``ops.swiglu`` computes ``silu(y[2 i]) * y[2 i + 1]``:
        row ``2 i`` = gate row ``I + i``, row ``2 i + 1`` = row ``i``."""
        I = weight.shape[0] // 2
        wi = torch.stack([weight[I:], weight[:I]], dim=1).reshape(2 * I, -1)
        bi = torch.stack([bias[I:], bias[:I]], dim=1).reshape(2 * I)
        return wi.contiguous(), bi.contiguous()

    @classmethod
    def post_load_hook(cls, model: "Model", model_path) -> "Model":
        """The tokenizer of a local directory, if ``transformers`` and the files are there; any failure is ignored (as in the reference)."""
        try:
            from transformers import AutoTokenizer

            model._tokenizer = AutoTokenizer.from_pretrained(str(Path(model_path)), local_files_only=True)
        except Exception:
            pass
        return model

    @classmethod
    def from_pretrained(cls, path: Union[str, Path], *, device="cuda:0") -> "Model":
        """A LOCAL directory holding ``config.json`` and ``model.safetensors`` (the reference's or the PyTorch names)."""
        from safetensors.torch import load_file

        p = Path(path)
        if not (p / "config.json").exists() or not (p / "model.safetensors").exists():
            raise FileNotFoundError(f"{path}: Moonshine.from_pretrained needs a local directory with config.json and model.safetensors "
                                    "(hub download is not built)")
        with open(p / "config.json") as f:
            config = ModelConfig.from_dict(json.load(f))
        model = cls.__new__(cls)
        model.config = config
        weights = cls.sanitize(model, load_file(str(p / "model.safetensors")))
        model = cls(config, weights=weights, device=device)
        return cls.post_load_hook(model, p)

    # ------------------------------------------------------------------ helpers
    def _f(self, *shape):
        return torch.empty(shape, dtype=torch.float32, device=self.device)

    def _z(self, *shape):
        return torch.zeros(shape, dtype=torch.float32, device=self.device)

    def _lens(self, lens: Sequence[int]) -> torch.Tensor:
        return torch.tensor(list(lens), dtype=torch.int32, device=self.device)

    def _tables(self, rot: int, rows: int):
        t = self._rope.get(rot)
        if t is None or t[0].shape[0] < rows:
            cap = max(256, 1 << (rows - 1).bit_length())
            t = self._rope[rot] = ops.moonshine_rope_tables(rot, cap, base=self.config.rope_theta, device=self.device)
        return t

    @staticmethod
    def _rows(t: torch.Tensor) -> Optional[torch.Tensor]:
        """[B, L, C] view -> its [B L, C] rows when they are evenly spaced (a slice of a dense buffer), else None."""
        B, L, C = t.shape
        if B > 1 and t.stride(0) != L * t.stride(1):
            return None
        return t.as_strided((B * L, C), (t.stride(1), 1))

    def _lin(self, x, lin, y, *, post_act: int = 0, res=None, **kw):
        """``y = act(x W^T + b) (+ res)`` on [B, L, C] views: ``conv_gemm``, or for a decoder linear (``(MFMA image, row-major image)``) of up to
        ``GEMV_ROWS`` rows the GEMV."""
        if isinstance(lin, tuple):
            pc, rm = lin
            if x.shape[0] * x.shape[1] <= GEMV_ROWS and not kw:
                rows = [self._rows(t) for t in (x, y) + (() if res is None else (res,))]
                if all(r is not None for r in rows):
                    ops.gemv(rows[0], rm, rows[1], post_act=post_act, res=None if res is None else rows[2])
                    return y
        else:
            pc = lin
        return ops.conv_gemm(x, pc, y, precision=self.precision, post_act=post_act, res=res, **kw)

    def _ln(self, x, weight, y=None):
        return ops.layernorm(x, self._f(*x.shape) if y is None else y, weight=weight, eps=LN_EPS)

    # ------------------------------------------------------------------ encoder
    def _pad_audio(self, audios: Sequence[torch.Tensor]) -> Tuple[torch.Tensor, List[int]]:
        ns = [int(a.numel()) for a in audios]
        for n in ns:
            if n < MIN_SAMPLES:
                raise ValueError(f"Moonshine: audio of {n} samples is shorter than {MIN_SAMPLES}, the shortest clip with one encoder frame")
        t1m = max(stem_lengths(n)[0] for n in ns)
        rows = t1m + 1                                     # output row t reads sample rows t and t + 1; samples behind them are never read
        buf = torch.zeros((len(ns), rows * 64), dtype=torch.float32)
        for b, a in enumerate(audios):
            m = min(ns[b], rows * 64)
            buf[b, :m] = a.reshape(-1)[:m].to(torch.float32).cpu()
        return buf.to(self.device), ns

    def stem(self, audio: torch.Tensor, ns: Sequence[int], *, return_stages: bool = False):
        """Zero-padded samples [B, 64 (T1max + 1)] on the device and the items' sample counts -> (x [B, T3max, d], T3 per item)."""
        c = self.config
        d, B = c.hidden_size, audio.shape[0]
        L = [stem_lengths(n) for n in ns]
        t1m, t2m, t3m = (max(l[i] for l in L) for i in range(3))
        assert audio.shape[1] == 64 * (t1m + 1)
        r1, r2 = 3 * (t2m + 2), 2 * (t3m + 1)                # rows of the zero-filled buffers the regrouped convs read: >= T1max, T2max
        assert r1 >= t1m and r2 >= t2m
        y1, y2, y3 = self._z(B, r1, d), self._z(B, r2, 2 * d), self._f(B, t3m, d)
        lens1 = self._lens([l[0] for l in L])
        parts = ops.new_stats(B, t1m, d, self.device)
        self._lin(audio.view(B, t1m + 1, 64), self.conv1, y1, lout=t1m, lens_out=lens1, post_act=ACT_TANH, stats=parts)   # rows >= T1_b stay zero
        coef = ops.group_norm_coef(parts, t1m, d, self.gn[0], self.gn[1], eps=LN_EPS, lens=lens1, rep=3)
        self._lin(y1.view(B, r1 // 3, 3 * d), self.conv2, y2, lout=t2m, pre=coef, post_act=ACT_GELU)
        self._lin(y2.view(B, r2 // 2, 4 * d), self.conv3, y3, lout=t3m, post_act=ACT_GELU)
        if not return_stages:
            return y3, [l[2] for l in L]
        coef1 = ops.group_norm_coef(parts, t1m, d, self.gn[0], self.gn[1], eps=LN_EPS, lens=lens1, rep=1)
        gn = ops.group_norm_apply(y1[:, :t1m], coef1, self._f(B, t1m, d))
        return y3, [l[2] for l in L], dict(tanh=y1[:, :t1m], gn=gn, conv2=y2[:, :t2m], conv3=y3, lens=L)

    def _attn_block(self, x, blk, H, KH, *, lens_d, pos0, cache=None, causal=False):
        """q | k | v of ``x`` [B, T, d], rotary embedding, attention; returns the heads' output [B, T, H dh] (before ``o_proj``)."""
        c = self.config
        B, T, d = x.shape
        dh = d // H
        rot = rotary_ndims(dh, c.partial_rotary_factor)
        qkv = self._lin(x, blk["qkv"], self._f(B, T, (H + 2 * KH) * dh))
        q, k, v = qkv[:, :, :H * dh], qkv[:, :, H * dh:(H + KH) * dh], qkv[:, :, (H + KH) * dh:]
        cos, sin = self._tables(rot, pos0 + T)
        att = self._f(B, T, H * dh)
        if cache is None:
            ops.partial_rope(q, q, heads=H, dh=dh, rot=rot, cos=cos, sin=sin, pos0=pos0, lens=lens_d, second=(k, k, KH))
            return ops.mid_attention(q, k, v, att, heads=H, kv_heads=KH, dh=dh, lens_q=lens_d, lens_k=lens_d, check_lens=False)
        ops.partial_rope(q, q, heads=H, dh=dh, rot=rot, cos=cos, sin=sin, pos0=pos0, second=(k, cache[:, pos0:pos0 + T, :KH * dh], KH))
        cache[:, pos0:pos0 + T, KH * dh:] = v
        return ops.mid_attention(q, cache[:, :pos0 + T, :KH * dh], cache[:, :pos0 + T, KH * dh:], att, heads=H, kv_heads=KH, dh=dh, causal=causal)

    def encode_frames(self, x: torch.Tensor, frames: Sequence[int], *, return_layers: bool = False):
        """The stem's output [B, T, d] and the items' frame counts -> the encoder's output [B, T, d] (rows beyond an item's frames are meaningless)."""
        c = self.config
        H, KH = c.encoder_num_attention_heads, c.encoder_num_key_value_heads
        B, T, d = x.shape
        lens_d = self._lens(frames)
        x = x.clone()
        h, mid = self._f(B, T, d), self._f(B, T, c.intermediate_size)
        taps = dict(layers=[]) if return_layers else None
        for i, blk in enumerate(self.enc_layers):
            att = self._attn_block(self._ln(x, blk["ln1"], h), blk, H, KH, lens_d=lens_d, pos0=0)
            if return_layers and i == 0:
                taps["attn0"] = self._lin(att, blk["o"], self._f(B, T, d))
            self._lin(att, blk["o"], x, res=x)
            self._lin(self._ln(x, blk["ln2"], h), blk["fc1"], mid, post_act=ACT_GELU)
            self._lin(mid, blk["fc2"], x, res=x)
            if return_layers:
                taps["layers"].append(x.clone())
        out = self._ln(x, self.enc_norm)
        return (out, taps) if return_layers else out

    def _load(self, audio) -> torch.Tensor:
        if isinstance(audio, (str, Path)):
            from ...utils import load_audio

            return torch.from_numpy(np.ascontiguousarray(load_audio(str(audio), sr=self.sample_rate), dtype=np.float32))
        if isinstance(audio, (np.ndarray, torch.Tensor, list, tuple)):
            return torch.as_tensor(np.asarray(audio) if isinstance(audio, (list, tuple)) else audio, dtype=torch.float32).reshape(-1)
        raise TypeError(f"Unsupported audio type: {type(audio)}")

    def encode(self, audios, *, return_stages: bool = False):
        """One clip (array / tensor / path) or a list of clips -> (encoder output [B, T3max, d], frames per item)."""
        if not isinstance(audios, (list, tuple)) or (len(audios) and isinstance(audios[0], (int, float))):
            audios = [audios]
        buf, ns = self._pad_audio([self._load(a) for a in audios])
        if not return_stages:
            x, frames = self.stem(buf, ns)
            return self.encode_frames(x, frames), frames
        x, frames, st = self.stem(buf, ns, return_stages=True)
        out, taps = self.encode_frames(x, frames, return_layers=True)
        return out, frames, dict(st, **taps)

    # ------------------------------------------------------------------ decoder
    def new_cache(self, encoder_out: torch.Tensor, frames: Optional[Sequence[int]] = None, capacity: int = 201) -> dict:
        """Preallocated self-attention caches and the cross k | v of every layer, projected once."""
        c = self.config
        B, T, d = encoder_out.shape
        KH, dh = c.decoder_num_key_value_heads, d // c.decoder_num_attention_heads
        frames = [T] * B if frames is None else list(frames)
        if len(frames) != B or min(frames) < 1 or max(frames) > T:
            raise ValueError(f"Moonshine: frame counts {frames} do not fit an encoder output of {B} x {T} frames")
        cross = [self._lin(encoder_out, blk["ckv"], self._f(B, T, 2 * KH * dh)) for blk in self.dec_layers]
        return dict(pos=0, cap=capacity, cross=cross, lens=self._lens(frames), self_kv=[self._z(B, capacity, 2 * KH * dh) for _ in self.dec_layers])

    def __call__(self, tokens, encoder_out: torch.Tensor, cache: Optional[dict] = None, *, frames: Optional[Sequence[int]] = None):
        """The decoder: ``tokens`` int [B, T] (T >= 1) behind the ``cache['pos']`` positions already in the cache -> (hidden [B, T, d], cache)."""
        c = self.config
        H, KH = c.decoder_num_attention_heads, c.decoder_num_key_value_heads
        tokens = torch.as_tensor(tokens).to(self.device).long()
        B, T = tokens.shape
        d = c.hidden_size
        dh = d // H
        if cache is None:
            cache = self.new_cache(encoder_out, frames, capacity=max(201, T))
        pos0 = cache["pos"]
        if pos0 + T > cache["cap"]:
            raise ValueError(f"Moonshine: {pos0} + {T} positions do not fit a cache of {cache['cap']}")
        x = self.embed[tokens].contiguous()
        h, I = self._f(B, T, d), c.intermediate_size
        for blk, kv, ckv in zip(self.dec_layers, cache["self_kv"], cache["cross"]):
            att = self._attn_block(self._ln(x, blk["ln1"], h), blk, H, KH, lens_d=None, pos0=pos0, cache=kv, causal=True)
            self._lin(att, blk["o"], x, res=x)
            cq = self._lin(self._ln(x, blk["ln2"], h), blk["cq"], self._f(B, T, H * dh))
            ops.mid_attention(cq, ckv[:, :, :KH * dh], ckv[:, :, KH * dh:], att, heads=H, kv_heads=KH, dh=dh, lens_k=cache["lens"], check_lens=False)
            self._lin(att, blk["co"], x, res=x)
            gate = self._lin(self._ln(x, blk["ln3"], h), blk["fc1"], self._f(B, T, 2 * I))
            self._lin(ops.swiglu(gate, self._f(B, T, I)), blk["fc2"], x, res=x)
        cache["pos"] = pos0 + T
        return self._ln(x, self.dec_norm), cache

    def _get_logits(self, hidden: torch.Tensor) -> torch.Tensor:
        """hidden [..., d] -> logits [..., V] (the tied table as a linear layer, or ``proj_out``)."""
        V = self.config.vocab_size
        flat = hidden.reshape(1, -1, hidden.shape[-1])
        if not flat.is_contiguous():
            flat = flat.contiguous()
        ws = self._f(1, flat.shape[1], ops.round_up(V, 64))
        self._lin(flat, self.head, ws[:, :, :V])
        lg = ws[0, :, :V]
        return lg if hidden.dim() == 2 else lg.reshape(*hidden.shape[:-1], V)

    def _decode_tokens(self, tokens: List[int]) -> str:
        if self._tokenizer is not None:
            return self._tokenizer.decode(tokens, skip_special_tokens=True)
        return "".join(chr(t) if t < 128 else f"<{t}>" for t in tokens)

    def decode_greedy(self, encoder_out: torch.Tensor, frames: Sequence[int], *, max_tokens: int = 200, temperature: float = 0.0, seed: int = 0,
                      return_trace: bool = False):
        """Lockstep decoding of a batch: one token list per item (cut before its EOS); with ``return_trace`` also each step's logits rows [B, V]
        and top-2 gaps [B]."""
        c = self.config
        B, V = encoder_out.shape[0], c.vocab_size
        cache = self.new_cache(encoder_out, frames, capacity=max_tokens + 1)
        cur = torch.full((B, 1), c.decoder_start_token_id, dtype=torch.int32, device=self.device)
        ids, gap = torch.empty((B,), dtype=torch.int32, device=self.device), self._f(B)
        out: List[List[int]] = [[] for _ in range(B)]
        done = [False] * B
        trace = dict(logits=[], gap=[]) if return_trace else None
        g = torch.Generator().manual_seed(seed) if temperature > 0 else None
        for _ in range(max_tokens):
            hidden, cache = self(cur, encoder_out, cache)
            logits = self._get_logits(hidden[:, -1, :])
            ops.ctc_rows(logits, ids=ids, gap=gap)
            if temperature > 0:
                u = torch.rand((B, logits.stride(0)), generator=g).clamp_(1e-20, 1.0)
                ops.sample(logits, ids, V=V, temperature=temperature, gumbel=(-torch.log(-torch.log(u))).to(self.device))
            host = ids.cpu().tolist()
            if return_trace:
                trace["logits"].append(logits.cpu().clone())
                trace["gap"].append(gap.cpu().clone())
            for b in range(B):
                if done[b]:
                    continue
                if host[b] == c.eos_token_id:
                    done[b] = True
                else:
                    out[b].append(host[b])
                    cur[b, 0] = host[b]
            if all(done):
                break
        return (out, trace) if return_trace else out

    def generate_batch(self, audios: Sequence, *, max_tokens: int = 200, temperature: float = 0.0, verbose: bool = False, seed: int = 0,
                       **kwargs) -> List[STTOutput]:
        """Right-padded clips decoded in lockstep; each result equals ``generate`` on that clip alone."""
        for k in ("generation_stream", "language", "source_lang", "target_lang", "stream", "dtype"):
            kwargs.pop(k, None)
        start = time.time()
        enc, frames = self.encode(list(audios))
        toks = self.decode_greedy(enc, frames, max_tokens=max_tokens, temperature=temperature, seed=seed)
        total = time.time() - start
        res = []
        for generated in toks:
            text = self._decode_tokens(generated)
            if verbose:
                print(f"Generated {len(generated)} tokens in {total:.2f}s")
                print(f"Text: {text}")
            res.append(STTOutput(text=text.strip(), segments=[{"text": text.strip(), "start": 0.0, "end": 0.0}], prompt_tokens=1,
                                 generation_tokens=len(generated), total_tokens=1 + len(generated), total_time=total,
                                 prompt_tps=1 / total if total > 0 else 0, generation_tps=len(generated) / total if total > 0 else 0))
        return res

    def generate(self, audio, *, max_tokens: int = 200, temperature: float = 0.0, verbose: bool = False, **kwargs) -> STTOutput:
        return self.generate_batch([audio], max_tokens=max_tokens, temperature=temperature, verbose=verbose, **kwargs)[0]
