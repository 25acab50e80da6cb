"""Granite Speech 4.1 2B NAR on MI355X (stt/models/granite_speech_nar): log-mel pairs -> Conformer encoder with block-local Shaw attention and a
self-conditioning CTC head -> posterior-weighted BPE hypothesis -> windowed Q-Former projector -> ONE bidirectional pass of the Granite editor over
``[audio | hypothesis with insertion slots]`` -> a second CTC collapse.  There is no token loop: every stage is one wide launch per layer.

The reference runs one clip per call.  What is built here is the model's meaning for a right-padded batch with per-item lengths: item ``b`` of a batch
equals the reference on that item alone.  ``generate_batch`` / ``transcribe_batch`` are the batched entry points; ``generate`` /
``_transcribe_tokens`` are a batch of one.

Host schedule:

  * front end: reflect pad 256, periodic Hann(400) centred in 512, hop 160, 80 HTK mels from the float64 filterbank, ``log10(max(., 1e-10))`` on the
    first ``l = 2 (n // 320)`` frames, clamped at the clip's own maximum - 8, ``/ 4 + 1`` (the fused log-mel kernel per clip, per-item maximum), pairs
    stacked to 160 columns; then rounded to bfloat16 values as the reference's ``_transcribe_tokens`` does, and on in float32;
  * encoder block: LayerNorm -> up (SiLU) -> down with ``res=`` (the half step folded into the weights: exact) -> LayerNorm -> one q | k | v GEMM ->
    ``shaw_block_attention`` under the items' lengths -> ``to_out`` with ``res=`` -> LayerNorm -> pointwise up -> ``glu_dwconv_silu`` (the BatchNorm's
    running statistics folded into the taps in float64; the depthwise conv has no bias) -> pointwise down with ``res=`` -> the second FFN -> LayerNorm.
    At ``self_conditioning_layer``: ``out`` -> ``selfcond_rows`` -> ``out_mid`` with ``res=``.  A hidden state the projector reads is normalised by its
    projector LayerNorm straight into its quarter of the fused [B, T, 4 d] buffer when it is produced: no concatenation copy;
  * BPE head: ``posterior_pool`` -> ``out_bpe`` -> ``ctc_rows`` -> ``ctc_collapse`` (dedup, then blanks);
  * projector: ``layer_projector`` (GELU) -> ``qformer_windows`` -> per layer LayerNorm, q and k | v GEMMs, ``flash_attention`` of ``block / rate`` queries
    over ``block`` keys per window, o with ``res=``, LayerNorm, fc1 (SiLU), fc2 with ``res=`` -> ``out_norm`` -> ``out_linear``; the windows' GEMMs
    run ``flatten``ed (a window holds 3 or 15 rows: one row tile per window would be nearly empty);
  * editor: per item ``[audio | text]`` right-padded to the batch's longest; RMSNorm -> one q | k | v GEMM -> ``head_norm_rope`` (half rotation, no
    norm weights) -> ``flash_attention`` (non-causal, grouped kv heads, ``scale = attention_multiplier``, ``lens_q`` / ``lens_k``) -> o with ``res=``
    and the residual multiplier as ``colscale`` -> RMSNorm -> gate | up interleaved -> ``swiglu`` -> down likewise; the tied head on the text rows only.

Weights travel as fp16 images with fp16 hi + lo activations (precision 4) like the other engines; norms, depthwise taps, the Shaw tables, the learned
query and the window positions stay float32.

Not built, each raising by name: hub download, bf16 and quantised checkpoints, ``dim_head`` other than 64 / 128 in the encoder or the editor, and
projector head widths other than the 64 / 128 of ``flash_attention``.  The model is not registered with the generic loader.
"""
from __future__ import annotations

import math
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from .... import ops
from ....ops import ACT_GELU, ACT_SILU
from ..base import STTOutput
from .config import ModelConfig

SAMPLING_RATE = 16000
N_FFT = 512
WIN_LENGTH = 400
HOP_LENGTH = 160
N_MELS = 80
LN_EPS = 1e-5          # the encoder's LayerNorms
BN_EPS = 1e-5          # EvalBatchNorm's default
FLASH_WIDTHS = (64, 128)


# ---------------------------------------------------------------------------------------------------- decoding utilities (decoding.py)
def ctc_collapse_decode(tokens: Sequence[int], blank_id: int) -> List[int]:
    """Standard CTC greedy collapse on the host: adjacent repeats dropped, then blanks (the device path is ``ops.ctc_collapse``)."""
    out, prev = [], None
    for t in tokens:
        t = int(t)
        if t != prev and t != blank_id:
            out.append(t)
        prev = t
    return out


def add_insertion_slots(token_ids: Sequence[int], blank_id: int, min_len: int = 8) -> List[int]:
    """N hypothesis tokens -> ``max(2 N + 1, min_len)`` ids: the tokens at the odd indices 1, 3, ..., 2 N - 1, blanks everywhere else."""
    ids = [int(t) for t in token_ids]
    out = [blank_id] * max(2 * len(ids) + 1, min_len)
    out[1:2 * len(ids):2] = ids
    return out


# ---------------------------------------------------------------------------------------------------- parameters
def _layer_indices(config: ModelConfig) -> List[int]:
    n = config.encoder.num_layers + 1
    return [i % n for i in config.encoder_layer_indices]


def expected_shapes(config: ModelConfig) -> Dict[str, Tuple[int, ...]]:
    """Parameter name -> shape of the reference's ``Model(config)`` (its names, MLX conv layouts)."""
    e, p, t = config.encoder, config.projector, config.text
    s: Dict[str, Tuple[int, ...]] = {}

    def lin(name, n, k, bias=True):
        s[name + ".weight"] = (n, k)
        if bias:
            s[name + ".bias"] = (n,)

    def norm(name, n, bias=True):
        s[name + ".weight"] = (n,)
        if bias:
            s[name + ".bias"] = (n,)

    d, inner, ci = e.hidden_dim, e.num_heads * e.dim_head, e.hidden_dim * e.conv_expansion_factor
    lin("encoder.input_linear", d, e.input_dim)
    for i in range(e.num_layers):
        q = f"encoder.layers.{i}."
        for f in ("ff1", "ff2"):
            norm(q + f + ".pre_norm", d)
            lin(q + f + ".up_proj", d * e.feedforward_mult, d)
            lin(q + f + ".down_proj", d, d * e.feedforward_mult)
        norm(q + "attn.pre_norm", d)
        lin(q + "attn.to_q", inner, d, False)
        lin(q + "attn.to_kv", 2 * inner, d, False)
        lin(q + "attn.to_out", d, inner)
        s[q + "attn.rel_pos_emb.weight"] = (2 * e.max_pos_emb + 1, e.dim_head)
        norm(q + "conv.norm", d)
        s[q + "conv.up_conv.weight"], s[q + "conv.up_conv.bias"] = (2 * ci, 1, d), (2 * ci,)
        s[q + "conv.depth_conv.weight"] = (ci, e.conv_kernel_size, 1)
        for n in ("weight", "bias", "running_mean", "running_var"):
            s[q + "conv.bn." + n] = (ci,)
        s[q + "conv.down_conv.weight"], s[q + "conv.down_conv.bias"] = (d, 1, ci), (d,)
        norm(q + "post_norm", d)
    lin("encoder.out", e.output_dim, d)
    lin("encoder.out_mid", d, e.output_dim)
    lin("encoder.out_bpe", e.bpe_output_dim, d)

    H = p.hidden_size
    for i in range(p.num_encoder_layers):
        norm(f"projector.layer_norms.{i}", p.encoder_dim)
    lin("projector.layer_projector", H, p.num_encoder_layers * p.encoder_dim, p.mlp_bias)
    s["projector.query"] = (1, p.block_size // p.downsample_rate, H)
    s["projector.window_positions"] = (1, p.block_size, H)
    for i in range(p.num_layers):
        q = f"projector.qformer.layers.{i}."
        norm(q + "attn_norm", H)
        for n in ("q_proj", "k_proj", "v_proj", "o_proj"):
            lin(q + "cross_attention." + n, H, H)
        norm(q + "mlp_norm", H)
        lin(q + "mlp.fc1", H * p.mlp_ratio, H)
        lin(q + "mlp.fc2", H, H * p.mlp_ratio)
    norm("projector.out_norm", H)
    lin("projector.out_linear", p.llm_dim, H)

    Ht, dh = t.hidden_size, t.hidden_size // t.num_attention_heads
    s["editor.embed_tokens.weight"] = (t.vocab_size, Ht)
    for i in range(t.num_hidden_layers):
        q = f"editor.layers.{i}."
        norm(q + "input_layernorm", Ht, False)
        lin(q + "self_attn.q_proj", t.num_attention_heads * dh, Ht, False)
        lin(q + "self_attn.k_proj", t.num_key_value_heads * dh, Ht, False)
        lin(q + "self_attn.v_proj", t.num_key_value_heads * dh, Ht, False)
        lin(q + "self_attn.o_proj", Ht, t.num_attention_heads * dh, False)
        norm(q + "post_attention_layernorm", Ht, False)
        lin(q + "mlp.gate_proj", t.intermediate_size, Ht, False)
        lin(q + "mlp.up_proj", t.intermediate_size, Ht, False)
        lin(q + "mlp.down_proj", Ht, t.intermediate_size, False)
    norm("editor.norm", Ht, False)
    return s


def make_granite_nar_weights(config: ModelConfig, seed: int = 0, head_gain: float = 4.0, blank_bias: float = 0.0, bpe_blank_bias: float = 0.0,
                             embed_gain: float = 1.0) -> Dict[str, torch.Tensor]:
    """A seeded checkpoint under the reference's parameter names: matrices N(0, 1 / fan_in), biases 0.1 N(0, 1), norm weights 1 + 0.1 N(0, 1), running
    variances in [0.5, 1.5], depthwise taps N(0, 1 / K), Shaw tables 0.5 N(0, 1), the learned query and window positions 0.5 N(0, 1), the token
    embedding ``embed_gain`` N(0, 1); the two CTC heads ``head_gain`` N(0, 1) / sqrt(d) with ``blank_bias`` / ``bpe_blank_bias`` added to the bias of
    their blank.  float32 tensors holding fp16-representable values, like a checkpoint published in 16 bits (the engine packs fp16 weight images)."""
    g = torch.Generator().manual_seed(seed)
    w: Dict[str, torch.Tensor] = {}
    for name, shape in expected_shapes(config).items():
        if name.endswith("running_var"):
            t = 0.5 + torch.rand(shape, generator=g)
        elif name.endswith("depth_conv.weight"):
            t = torch.randn(shape, generator=g) / math.sqrt(shape[1])
        elif name.endswith("rel_pos_emb.weight") or name in ("projector.query", "projector.window_positions"):
            t = 0.5 * torch.randn(shape, generator=g)
        elif name == "editor.embed_tokens.weight":
            t = embed_gain * torch.randn(shape, generator=g)
        elif name.endswith(".bias") or name.endswith("running_mean"):
            t = 0.1 * torch.randn(shape, generator=g)
        elif len(shape) == 1:
            t = 1.0 + 0.1 * torch.randn(shape, generator=g)
        elif name in ("encoder.out.weight", "encoder.out_bpe.weight"):
            t = head_gain * torch.randn(shape, generator=g) / math.sqrt(shape[-1])
        else:
            t = torch.randn(shape, generator=g) / math.sqrt(shape[-1])
        if name == "encoder.out.bias":
            t[0] += blank_bias
        if name == "encoder.out_bpe.bias":
            t[config.blank_token_id] += bpe_blank_bias
        w[name] = t.to(torch.float16).to(torch.float32)
    return w


def _pow2(x: float) -> bool:
    return x > 0 and math.frexp(x)[0] == 0.5


class Model:
    """``Model(config)`` of the reference as an engine; ``weights`` omitted = a seeded checkpoint (the reference: freshly initialised)."""

    def __init__(self, config: ModelConfig, weights: Optional[Dict[str, torch.Tensor]] = None, device="cuda:0", seed: int = 0, precision: int = 4):
        e, p, t = config.encoder, config.projector, config.text
        if e.dim_head not in FLASH_WIDTHS:
            raise NotImplementedError(f"GraniteSpeechNar: encoder dim_head {e.dim_head} is not built (shaw_block_attention runs heads of 64 / 128)")
        if t.hidden_size % t.num_attention_heads or t.hidden_size // t.num_attention_heads not in FLASH_WIDTHS:
            raise NotImplementedError(f"GraniteSpeechNar: editor head width {t.hidden_size}/{t.num_attention_heads} is not built "
                                      "(flash_attention runs heads of 64 / 128)")
        if p.hidden_size % p.num_heads or p.hidden_size // p.num_heads not in FLASH_WIDTHS:
            raise NotImplementedError(f"GraniteSpeechNar: projector head width {p.hidden_size}/{p.num_heads} is not built (neither flash_attention "
                                      "nor narrow_attention covers cross attention of that width)")
        if e.max_pos_emb < e.context_size - 1:
            raise ValueError(f"GraniteSpeechNar: max_pos_emb {e.max_pos_emb} does not hold the distances of context_size {e.context_size}")
        if e.conv_kernel_size % 2 == 0 or e.conv_kernel_size > ops.GLU_DWCONV_MAX_TAPS:
            raise ValueError(f"GraniteSpeechNar: conv_kernel_size {e.conv_kernel_size} must be odd and at most {ops.GLU_DWCONV_MAX_TAPS}")
        if p.block_size % p.downsample_rate or p.encoder_dim != e.hidden_dim or p.num_encoder_layers != len(config.encoder_layer_indices):
            raise ValueError("GraniteSpeechNar: the projector's block_size / downsample_rate / encoder_dim / num_encoder_layers do not fit the encoder")
        if p.llm_dim != t.hidden_size or t.num_attention_heads % t.num_key_value_heads or not 1 <= e.self_conditioning_layer <= e.num_layers:
            raise ValueError("GraniteSpeechNar: llm_dim / kv heads / self_conditioning_layer do not fit")
        if e.input_dim != 2 * N_MELS:
            raise ValueError(f"GraniteSpeechNar: input_dim {e.input_dim} is not two stacked frames of {N_MELS} mels")
        ops.require_gpu()
        assert precision in (3, 4)
        self.config, self.device, self.precision = config, torch.device(device), precision
        self._tokenizer = None
        self._rope: Optional[Tuple[torch.Tensor, torch.Tensor]] = None
        self._front: Optional[Tuple[torch.Tensor, torch.Tensor]] = None
        self.load_weights(make_granite_nar_weights(config, seed) if weights is None else weights)

    # ------------------------------------------------------------------ checkpoint handling
    @staticmethod
    def sanitize(weights: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        """Drops the BatchNorm ``num_batches_tracked`` counters; the conv kernels already lie in the MLX layout."""
        return {k: v for k, v in weights.items() if not k.endswith("num_batches_tracked")}

    def model_quant_predicate(self, p: str, m=None) -> bool:
        """The reference's answer (the editor alone is quantised); quantised checkpoints themselves are not built."""
        return p.startswith("editor.")

    def load_weights(self, weights, strict: bool = True):
        c, dev = self.config, self.device
        e, p, t = c.encoder, c.projector, c.text
        weights = dict(weights)
        if any(k.endswith(".scales") or k.endswith(".biases") for k in weights):
            raise NotImplementedError("GraniteSpeechNar.load_weights: quantised checkpoints are not built")
        if any(torch.as_tensor(v).dtype == torch.bfloat16 for v in weights.values()):
            raise NotImplementedError("GraniteSpeechNar.load_weights: bf16 checkpoints are not built (the weight images are fp16)")
        w = {k: torch.as_tensor(v).detach().to(torch.float32).cpu() for k, v in weights.items()}
        shapes = expected_shapes(c)
        miss = [k for k in shapes if k not in w]
        if miss:
            raise ValueError(f"GraniteSpeechNar.load_weights: missing parameters {miss[:4]}{' ...' if len(miss) > 4 else ''}")
        extra = [k for k in w if k not in shapes]
        if extra and strict:
            raise ValueError(f"GraniteSpeechNar.load_weights: unexpected parameters {extra[:4]}{' ...' if len(extra) > 4 else ''}")
        for k, s in shapes.items():
            if tuple(w[k].shape) != s:
                raise ValueError(f"GraniteSpeechNar.load_weights: {k} has shape {tuple(w[k].shape)}, expected {s}")

        def lin(name, scale=1.0):
            wt, b = w[name + ".weight"], w.get(name + ".bias")
            wt = wt.reshape(wt.shape[0], -1)   # [n, 1, k] pointwise convs are linears
            return ops.pack_conv(wt * scale, None if b is None else b * scale, dev, f16=True)

        vec = lambda name: w[name].contiguous().to(dev)
        norm = lambda name: (vec(name + ".weight"), vec(name + ".bias"))

        self.input_linear = lin("encoder.input_linear")
        self.enc_layers = []
        for i in range(e.num_layers):
            q = f"encoder.layers.{i}."
            bn = {n: w[q + "conv.bn." + n].double() for n in ("weight", "bias", "running_mean", "running_var")}
            s = bn["weight"] / torch.sqrt(bn["running_var"] + BN_EPS)   # BatchNorm on running statistics, folded in float64 (encoder.py:148-149)
            self.enc_layers.append(dict(
                ff1_norm=norm(q + "ff1.pre_norm"), ff1_up=lin(q + "ff1.up_proj"), ff1_down=lin(q + "ff1.down_proj", 0.5),
                attn_norm=norm(q + "attn.pre_norm"),
                qkv=ops.pack_conv(torch.cat([w[q + "attn.to_q.weight"], w[q + "attn.to_kv.weight"]]), None, dev, f16=True),
                to_out=lin(q + "attn.to_out"), table=vec(q + "attn.rel_pos_emb.weight"),
                conv_norm=norm(q + "conv.norm"), pw1=lin(q + "conv.up_conv"),
                dw_w=(s[:, None] * w[q + "conv.depth_conv.weight"][:, :, 0].double()).to(torch.float32).contiguous().to(dev),
                dw_b=(bn["bias"] - s * bn["running_mean"]).to(torch.float32).contiguous().to(dev),
                pw2=lin(q + "conv.down_conv"),
                ff2_norm=norm(q + "ff2.pre_norm"), ff2_up=lin(q + "ff2.up_proj"), ff2_down=lin(q + "ff2.down_proj", 0.5),
                post_norm=norm(q + "post_norm")))
        self.out, self.out_mid, self.out_bpe = lin("encoder.out"), lin("encoder.out_mid"), lin("encoder.out_bpe")

        self.proj_norms = [norm(f"projector.layer_norms.{i}") for i in range(p.num_encoder_layers)]
        self.layer_projector = lin("projector.layer_projector")
        self.query, self.window_positions = vec("projector.query")[0].contiguous(), vec("projector.window_positions")[0].contiguous()
        self.q_layers = []
        for i in range(p.num_layers):
            q = f"projector.qformer.layers.{i}."
            ca = q + "cross_attention."
            self.q_layers.append(dict(
                attn_norm=norm(q + "attn_norm"), q=lin(ca + "q_proj"),
                kv=ops.pack_conv(torch.cat([w[ca + "k_proj.weight"], w[ca + "v_proj.weight"]]), torch.cat([w[ca + "k_proj.bias"], w[ca + "v_proj.bias"]]),
                                 dev, f16=True),
                o=lin(ca + "o_proj"), mlp_norm=norm(q + "mlp_norm"), fc1=lin(q + "mlp.fc1"), fc2=lin(q + "mlp.fc2")))
        self.out_norm, self.out_linear = norm("projector.out_norm"), lin("projector.out_linear")

        self.embed = vec("editor.embed_tokens.weight")
        self.head = lin("editor.embed_tokens")
        self.ed_layers = []
        for i in range(t.num_hidden_layers):
            q = f"editor.layers.{i}."
            sa = q + "self_attn."
            gate, up = w[q + "mlp.gate_proj.weight"], w[q + "mlp.up_proj.weight"]
            self.ed_layers.append(dict(
                in_norm=vec(q + "input_layernorm.weight"),
                qkv=ops.pack_conv(torch.cat([w[sa + "q_proj.weight"], w[sa + "k_proj.weight"], w[sa + "v_proj.weight"]]), None, dev, f16=True),
                o=lin(sa + "o_proj"), post_norm=vec(q + "post_attention_layernorm.weight"),
                gate_up=ops.pack_conv(torch.stack([gate, up], dim=1).reshape(2 * gate.shape[0], gate.shape[1]), None, dev, f16=True),   # rows g0 u0 g1 u1 ..
                down=lin(q + "mlp.down_proj")))
        self.ed_norm = vec("editor.norm.weight")
        self.res_scale = torch.full((t.hidden_size,), float(t.residual_multiplier), dtype=torch.float32, device=dev)
        self._rope = None
        return self

    @staticmethod
    def post_load_hook(model: "Model", model_path) -> "Model":
        """Attaches the tokenizer of a LOCAL directory (``local_files_only``); anything else is refused before ``transformers`` is called."""
        if not isinstance(model_path, (str, Path)) or not Path(model_path).is_dir():
            raise FileNotFoundError(f"{model_path}: GraniteSpeechNar.post_load_hook needs an existing local directory (hub download is not built)")
        from transformers import AutoTokenizer

        model._tokenizer = AutoTokenizer.from_pretrained(str(model_path), local_files_only=True)
        return model

    @classmethod
    def from_pretrained(cls, path: Union[str, Path], *, device="cuda:0") -> "Model":
        """A LOCAL directory holding ``config.json``, ``model.safetensors`` (the reference's parameter names, float32 or float16) and the tokenizer's
        files."""
        p = Path(path)
        if not p.is_dir() or not (p / "config.json").exists() or not (p / "model.safetensors").exists():
            raise FileNotFoundError(f"{path}: GraniteSpeechNar.from_pretrained needs a local directory with config.json and model.safetensors "
                                    "(hub download and checkpoint conversion are not built)")
        from safetensors.torch import load_file

        model = cls(ModelConfig.from_pretrained(p), weights=cls.sanitize(load_file(str(p / "model.safetensors"))), device=device)
        return cls.post_load_hook(model, p)

    # ------------------------------------------------------------------ front end
    def _f(self, *shape):
        """A float32 buffer whose rows are padded to a multiple of 64 columns (16-byte aligned rows for any width)."""
        ld = ops.round_up(shape[-1], 64)
        return torch.empty(shape[:-1] + (ld,), dtype=torch.float32, device=self.device)[..., :shape[-1]]

    def _load(self, audio) -> torch.Tensor:
        if isinstance(audio, (str, Path)):
            from .... import audio_io

            wav, sr = audio_io.read(str(audio), always_2d=False, dtype="float32")
            if wav.ndim > 1:
                wav = wav.mean(axis=1)
            if sr != SAMPLING_RATE:
                raise ValueError(f"audio must be {SAMPLING_RATE} Hz; got {sr}")
            return torch.from_numpy(np.ascontiguousarray(wav, dtype=np.float32))
        if isinstance(audio, (np.ndarray, torch.Tensor, list, tuple)):
            return torch.as_tensor(np.asarray(audio, dtype=np.float32) if not isinstance(audio, torch.Tensor) else audio, dtype=torch.float32).reshape(-1)
        raise TypeError(f"Unsupported audio type: {type(audio)}")

    def _compute_features(self, waveform) -> torch.Tensor:
        """1-D 16 kHz mono waveform -> [T_enc, 160] stacked log-mel features on the device (float32, before the bfloat16 rounding)."""
        from .... import dsp

        x = torch.as_tensor(waveform, dtype=torch.float32).reshape(-1)
        n = x.numel()
        l = 2 * (n // (2 * HOP_LENGTH))
        if l < 2 or n <= N_FFT // 2:
            raise ValueError(f"GraniteSpeechNar: audio of {n} samples is too short for one encoder frame ({2 * HOP_LENGTH} samples) behind the reflect pad")
        if self._front is None:
            lpad = (N_FFT - WIN_LENGTH) // 2
            win = torch.zeros(N_FFT, dtype=torch.float32)
            win[lpad:lpad + WIN_LENGTH] = dsp.hanning(WIN_LENGTH, periodic=True).to(torch.float32).cpu()
            self._front = (win.to(self.device), dsp.mel_filters(SAMPLING_RATE, N_FFT, N_MELS, precise=True).to(self.device).contiguous())
        win, fb = self._front
        mel = ops.logmel(x.to(self.device)[None].contiguous(), N_FFT, HOP_LENGTH, win, 1, l, fb, 0)   # log10, clamp at the item's max - 8, / 4 + 1
        return mel[0].reshape(l // 2, 2 * N_MELS)

    def _pad(self, items: Sequence[torch.Tensor]) -> Tuple[torch.Tensor, List[int]]:
        lens = [int(t.shape[0]) for t in items]
        batch = torch.zeros((len(items), max(lens), items[0].shape[1]), dtype=torch.float32, device=self.device)
        for i, t in enumerate(items):
            batch[i, :lens[i]] = t
        return batch, lens

    # ------------------------------------------------------------------ encoder
    def encode(self, feats: torch.Tensor, lens: List[int], *, taps: Optional[dict] = None):
        """Features [B, T, 160] (bfloat16-representable float32) and the items' frames -> dict(fused [B, T, 4 d]: the projector's normalised inputs,
        probs [B, T, V], p_blank [B, T], pooled [B, W, d], bpe_ids / bpe_gap [B, W], hyp: one id list per item).  ``taps``: a dict that receives
        ``input_linear``, per block ``attn{i}`` (the attention module's output) and ``block{i}``."""
        c, prec, dev = self.config, self.precision, self.device
        e = c.encoder
        B, T, _ = feats.shape
        d, H, dh, ctx = e.hidden_dim, e.num_heads, e.dim_head, e.context_size
        inner, ci, ff = H * dh, d * e.conv_expansion_factor, d * e.feedforward_mult
        lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
        slots = _layer_indices(c)
        fused = self._f(B, T, len(slots) * d)

        def tap_for_projector(x, index):
            for slot, want in enumerate(slots):
                if want == index:
                    ops.layernorm(x, fused[..., slot * d:(slot + 1) * d], weight=self.proj_norms[slot][0], bias=self.proj_norms[slot][1],
                                  eps=c.projector.layernorm_eps)

        x, xn, h = self._f(B, T, d), self._f(B, T, d), self._f(B, T, d)
        mid, qkv, att, pw, cv = self._f(B, T, ff), self._f(B, T, 3 * inner), self._f(B, T, inner), self._f(B, T, 2 * ci), self._f(B, T, ci)
        ops.conv_gemm(feats, self.input_linear, x, precision=prec)
        if taps is not None:
            taps["input_linear"] = x.clone()
        tap_for_projector(x, 0)
        res = {}
        for i, blk in enumerate(self.enc_layers, start=1):
            ops.layernorm(x, h, weight=blk["ff1_norm"][0], bias=blk["ff1_norm"][1], eps=LN_EPS)
            ops.conv_gemm(h, blk["ff1_up"], mid, post_act=ACT_SILU, precision=prec)
            ops.conv_gemm(mid, blk["ff1_down"], x, res=x, precision=prec)
            ops.layernorm(x, h, weight=blk["attn_norm"][0], bias=blk["attn_norm"][1], eps=LN_EPS)
            ops.conv_gemm(h, blk["qkv"], qkv, precision=prec)
            ops.shaw_block_attention(qkv[..., :inner], qkv[..., inner:2 * inner], qkv[..., 2 * inner:], blk["table"], att, heads=H, dh=dh, ctx=ctx,
                                     max_pos=e.max_pos_emb, scale=dh ** -0.5, lens=lens_d, check_lens=False)   # lens come from checked host integers
            if taps is not None:
                taps[f"attn{i}"] = ops.conv_gemm(att, blk["to_out"], self._f(B, T, d), precision=prec)
            ops.conv_gemm(att, blk["to_out"], x, res=x, precision=prec)
            ops.layernorm(x, h, weight=blk["conv_norm"][0], bias=blk["conv_norm"][1], eps=LN_EPS)
            ops.conv_gemm(h, blk["pw1"], pw, precision=prec)
            ops.glu_dwconv_silu(pw, blk["dw_w"], blk["dw_b"], cv, lens=lens_d)
            ops.conv_gemm(cv, blk["pw2"], x, res=x, precision=prec)
            ops.layernorm(x, h, weight=blk["ff2_norm"][0], bias=blk["ff2_norm"][1], eps=LN_EPS)
            ops.conv_gemm(h, blk["ff2_up"], mid, post_act=ACT_SILU, precision=prec)
            ops.conv_gemm(mid, blk["ff2_down"], x, res=x, precision=prec)
            ops.layernorm(x, xn, weight=blk["post_norm"][0], bias=blk["post_norm"][1], eps=LN_EPS)
            x, xn = xn, x
            if taps is not None:
                taps[f"block{i}"] = x.clone()
            if i == e.self_conditioning_layer:
                V = e.output_dim
                logits = self._f(B * T, V)
                ops.conv_gemm(x, self.out, logits.as_strided((B, T, V), (T * logits.stride(0), logits.stride(0), 1)), precision=prec)
                probs, pb = self._f(B * T, V), torch.empty((B * T,), dtype=torch.float32, device=dev)
                ops.selfcond_rows(logits, probs=probs, p_blank=pb)
                res["probs"], res["p_blank"] = probs.as_strided((B, T, V), (T * probs.stride(0), probs.stride(0), 1)), pb.view(B, T)
                ops.conv_gemm(res["probs"], self.out_mid, x, res=x, precision=prec)
            tap_for_projector(x, i)
        window = e.bpe_pooling_window
        W = (T + window - 1) // window
        res["pooled"] = ops.posterior_pool(x, res["p_blank"], window, lens=lens_d, out=self._f(B, W, d))
        Vb = e.bpe_output_dim
        bpe = self._f(B * W, Vb)
        ops.conv_gemm(res["pooled"], self.out_bpe, bpe.as_strided((B, W, Vb), (W * bpe.stride(0), bpe.stride(0), 1)), precision=prec)
        ids, gap, _ = ops.ctc_rows(bpe)
        wlens = [(n + window - 1) // window for n in lens]
        tokens, counts = ops.ctc_collapse(ids.view(B, W), lens=torch.tensor(wlens, dtype=torch.int32, device=dev), blank=c.blank_token_id)
        host = torch.cat([counts[:, None], tokens], dim=1).cpu()
        res.update(fused=fused, hidden=x, bpe_ids=ids.view(B, W), bpe_gap=gap.view(B, W), bpe_lens=wlens,
                   hyp=[host[b, 1:1 + int(host[b, 0])].tolist() for b in range(B)])
        return res

    # ------------------------------------------------------------------ projector
    def project(self, fused: torch.Tensor, lens: List[int], *, taps: Optional[dict] = None) -> Tuple[torch.Tensor, List[int]]:
        """The normalised, fused encoder states [B, T, 4 d] -> (audio embeddings [B, nblocks * nq, llm_dim], each item's rows)."""
        c, prec, dev = self.config, self.precision, self.device
        p = c.projector
        B, T, _ = fused.shape
        Hp, block, rate = p.hidden_size, p.block_size, p.downsample_rate
        nq, nb = block // rate, (T + block - 1) // block
        heads, dh = p.num_heads, Hp // p.num_heads
        hp = self._f(B, T, Hp)
        ops.conv_gemm(fused, self.layer_projector, hp, post_act=ACT_GELU, precision=prec)
        qs, kv = ops.qformer_windows(hp, self.query, self.window_positions, block=block, rate=rate, lens=torch.tensor(lens, dtype=torch.int32, device=dev))
        if taps is not None:
            taps["proj_queries"], taps["proj_kv"] = qs.clone(), kv.clone()
        N = B * nb
        qn, qp, kvp, att, mid = self._f(N, nq, Hp), self._f(N, nq, Hp), self._f(N, block, 2 * Hp), self._f(N, nq, Hp), self._f(N, nq, Hp * p.mlp_ratio)
        for blk in self.q_layers:
            ops.layernorm(qs, qn, weight=blk["attn_norm"][0], bias=blk["attn_norm"][1], eps=p.layernorm_eps)
            ops.conv_gemm(qn, blk["q"], qp, flatten=True, precision=prec)
            ops.conv_gemm(kv, blk["kv"], kvp, flatten=True, precision=prec)
            ops.flash_attention(qp, kvp[..., :Hp], kvp[..., Hp:], att, heads=heads, dh=dh, scale=dh ** -0.5)
            ops.conv_gemm(att, blk["o"], qs, res=qs, flatten=True, precision=prec)
            ops.layernorm(qs, qn, weight=blk["mlp_norm"][0], bias=blk["mlp_norm"][1], eps=p.layernorm_eps)
            ops.conv_gemm(qn, blk["fc1"], mid, post_act=ACT_SILU, flatten=True, precision=prec)
            ops.conv_gemm(mid, blk["fc2"], qs, res=qs, flatten=True, precision=prec)
        ops.layernorm(qs, qn, weight=self.out_norm[0], bias=self.out_norm[1], eps=p.layernorm_eps)
        audio = torch.empty((N, nq, p.llm_dim), dtype=torch.float32, device=dev)
        ops.conv_gemm(qn, self.out_linear, audio, flatten=True, precision=prec)
        return audio.view(B, nb * nq, p.llm_dim), [((n + block - 1) // block) * nq for n in lens]

    # ------------------------------------------------------------------ editor
    def _rope_tables(self, rows: int) -> Tuple[torch.Tensor, torch.Tensor]:
        if self._rope is None or self._rope[0].shape[0] < rows:
            t = self.config.text
            dh = t.hidden_size // t.num_attention_heads
            cap = max(256, 1 << (rows - 1).bit_length())
            freqs = 1.0 / (t.rope_theta ** (torch.arange(0, dh, 2, dtype=torch.float32) / dh))
            ang = torch.arange(cap, dtype=torch.float32)[:, None] * freqs[None, :]
            self._rope = (torch.cos(ang).contiguous().to(self.device), torch.sin(ang).contiguous().to(self.device))
        return self._rope

    def edit(self, audio: torch.Tensor, alens: List[int], text_ids: List[List[int]], *, taps: Optional[dict] = None):
        """Audio embeddings [B, A, llm_dim] (the projector's output, NOT yet divided by ``embedding_multiplier``), each item's audio rows and slotted
        hypothesis -> (ids int32 [B, maxN] blank-padded, gap [B, maxN], tail logits [sum N, V]); item ``b`` runs over its own
        ``[audio_b | text_b]`` rows."""
        c, prec, dev = self.config, self.precision, self.device
        t = c.text
        B = audio.shape[0]
        Ht, Hq, Hkv = t.hidden_size, t.num_attention_heads, t.num_key_value_heads
        dh, I, m = Ht // Hq, t.intermediate_size, float(t.embedding_multiplier)
        nlens = [len(ids) for ids in text_ids]
        slens = [a + n for a, n in zip(alens, nlens)]
        S = max(slens)
        x = torch.zeros((B, S, Ht), dtype=torch.float32, device=dev)
        for b in range(B):
            a = audio[b, :alens[b]]
            # the reference divides the audio rows by the multiplier and the editor multiplies every row by it: a power of two folds exactly
            x[b, :alens[b]] = a if _pow2(m) else (a / m) * m
            x[b, alens[b]:slens[b]] = self.embed[torch.tensor(text_ids[b], dtype=torch.long, device=dev)] * m
        if taps is not None:
            taps["editor_in"] = x.clone()
        lens_d = torch.tensor(slens, dtype=torch.int32, device=dev)
        cos, sin = self._rope_tables(S)
        h, qkv = self._f(B, S, Ht), self._f(B, S, (Hq + 2 * Hkv) * dh)
        qr, kr, att = self._f(B, S, Hq * dh), self._f(B, S, Hkv * dh), self._f(B, S, Hq * dh)
        gu, act = torch.empty((B, S, 2 * I), dtype=torch.float32, device=dev), torch.empty((B, S, I), dtype=torch.float32, device=dev)   # swiglu: dense rows
        for i, blk in enumerate(self.ed_layers):
            ops.rmsnorm(x, h, blk["in_norm"], eps=t.rms_norm_eps)
            ops.conv_gemm(h, blk["qkv"], qkv, precision=prec)
            ops.head_norm_rope(qkv[..., :Hq * dh], qr, heads=Hq, dh=dh, cos=cos, sin=sin, second=(qkv[..., Hq * dh:(Hq + Hkv) * dh], kr, Hkv, None))
            ops.flash_attention(qr, kr, qkv[..., (Hq + Hkv) * dh:], att, heads=Hq, kv_heads=Hkv, dh=dh, scale=float(t.attention_multiplier),
                                lens_q=lens_d, lens_k=lens_d)
            ops.conv_gemm(att, blk["o"], x, res=x, colscale=self.res_scale, precision=prec)
            ops.rmsnorm(x, h, blk["post_norm"], eps=t.rms_norm_eps)
            ops.conv_gemm(h, blk["gate_up"], gu, precision=prec)
            ops.swiglu(gu, act)
            ops.conv_gemm(act, blk["down"], x, res=x, colscale=self.res_scale, precision=prec)
            if taps is not None:
                taps[f"editor{i}"] = x.clone()
        ops.rmsnorm(x, h, self.ed_norm, eps=t.rms_norm_eps)
        tail = torch.cat([h[b, alens[b]:slens[b]] for b in range(B)], dim=0)[None].contiguous()      # the text rows only (logits_start)
        V, R = t.vocab_size, tail.shape[1]
        logits = self._f(R, V)
        ops.conv_gemm(tail, self.head, logits[None], out_scale=1.0 / float(t.logits_scaling), use_bias=False, precision=prec)
        ids, gap, _ = ops.ctc_rows(logits)
        maxn = max(nlens)
        pad_ids = torch.full((B, maxn), c.blank_token_id, dtype=torch.int32, device=dev)
        pad_gap = torch.zeros((B, maxn), dtype=torch.float32, device=dev)
        r0 = 0
        for b, n in enumerate(nlens):
            pad_ids[b, :n], pad_gap[b, :n] = ids[r0:r0 + n], gap[r0:r0 + n]
            r0 += n
        return pad_ids, pad_gap, logits, nlens

    # ------------------------------------------------------------------ inference
    def _check_lens(self, lens, B: int, T: int) -> List[int]:
        lens = [T] * B if lens is None else [int(v) for v in torch.as_tensor(lens).reshape(-1).tolist()]
        if len(lens) != B or min(lens) < 1 or max(lens) > T:
            raise ValueError(f"GraniteSpeechNar: lengths {lens} do not fit a batch of {B} items of {T} frames (every item needs at least one frame)")
        return lens

    def transcribe_batch(self, features, lens=None, *, return_stages: bool = False):
        """Features [B, T, 160] right-padded, the items' frames -> one list of final token ids per item (and, ``return_stages``, a dict of every
        stage).  Each item equals ``_transcribe_tokens`` on that item alone."""
        c, dev = self.config, self.device
        feats = torch.as_tensor(features, dtype=torch.float32)
        if feats.dim() != 3 or feats.shape[2] != c.encoder.input_dim:
            raise ValueError(f"GraniteSpeechNar: features must be [B, T, {c.encoder.input_dim}], got {tuple(feats.shape)}")
        lens = self._check_lens(lens, feats.shape[0], feats.shape[1])
        x = self._f(*feats.shape)
        x.copy_(feats.to(dev).to(torch.bfloat16).to(torch.float32))     # the reference's astype(bfloat16): the values, then on in float32
        taps = {} if return_stages else None
        enc = self.encode(x, lens, taps=taps)
        audio, alens = self.project(enc["fused"], lens, taps=taps)
        text_ids = [add_insertion_slots(hyp, c.blank_token_id, c.min_edit_sequence_length) for hyp in enc["hyp"]]
        ids, gap, logits, nlens = self.edit(audio, alens, text_ids, taps=taps)
        tokens, counts = ops.ctc_collapse(ids, lens=torch.tensor(nlens, dtype=torch.int32, device=dev), blank=c.blank_token_id)
        host = torch.cat([counts[:, None], tokens], dim=1).cpu()
        final = [host[b, 1:1 + int(host[b, 0])].tolist() for b in range(host.shape[0])]
        if not return_stages:
            return final
        taps.update(features=x, probs=enc["probs"], p_blank=enc["p_blank"], pooled=enc["pooled"], bpe_ids=enc["bpe_ids"], bpe_gap=enc["bpe_gap"],
                    bpe_lens=enc["bpe_lens"], hidden=enc["hidden"], hyp=enc["hyp"], audio=audio, audio_lens=alens, text_ids=text_ids, edit_ids=ids,
                    edit_gap=gap, tail_logits=logits, text_lens=nlens, final=final)
        return final, taps

    def _transcribe_tokens(self, input_features) -> List[int]:
        """Features [T, 160] (or [1, T, 160]) of one clip -> its final token ids."""
        f = torch.as_tensor(input_features, dtype=torch.float32)
        return self.transcribe_batch(f[None] if f.dim() == 2 else f)[0]

    def generate_batch(self, audios: Sequence, *, verbose: bool = False, **kwargs) -> List[STTOutput]:
        """One pass over all clips (paths, numpy arrays or tensors, 16 kHz mono); each result equals ``generate`` on that clip alone."""
        if self._tokenizer is None:
            raise RuntimeError("Tokenizer not loaded — attach one through post_load_hook (or set an object with decode(ids, skip_special_tokens=True)).")
        feats, lens = self._pad([self._compute_features(self._load(a)) for a in audios])
        out = []
        for ids in self.transcribe_batch(feats, lens):
            text = self._tokenizer.decode([int(t) for t in ids], skip_special_tokens=True)
            if verbose:
                print(text)
            out.append(STTOutput(text=text))
        return out

    def generate(self, audio, *, verbose: bool = False, generation_stream=None, **kwargs) -> STTOutput:
        return self.generate_batch([audio], verbose=verbose, **kwargs)[0]
