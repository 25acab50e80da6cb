"""Sortformer speaker diarization on MI355X (vad/models/sortformer/sortformer.py): log-mel -> FastConformer encoder -> projection -> BART-style
post-LN Transformer encoder -> speaker sigmoids, plus the host logic around it (segments, silence trim, the v1 streaming state).

  * features: NeMo FilterbankFeatures for a batch of waveforms in one fused kernel launch (``extract_mel_features``, sortformer.py:36-123);
  * FastConformer encoder: the engine of ``stt/models/parakeet/conformer.py`` (``relpos_attention``, ``glu_dwconv_silu``, ``stencil2d_k3s2``) under
    a name adapter (``adapt_fc_weights``).  The reference applies ``scale_input`` in ``FastConformerEncoder.encode`` (473-494), not in the
    subsampler, and its streaming state holds UNSCALED pre-encoded embeddings: the ``Conformer`` is built with ``xscaling=False`` and the scale is
    applied here, in front of ``Conformer.encode``;
  * Transformer encoder (517-633): learned positions added by the projection's ``res=``; per layer one fused q | k | v ``conv_gemm`` (zeros in
    the k slice of the bias when ``k_proj_bias`` is false), ``narrow_attention`` (heads of 24: ``csrc/narrow_attn.hip``), the out projection,
    ``layernorm(res=)`` (LN(x + res): the post-LN step), fc1 with ReLU, fc2, ``layernorm(res=)``;
  * head (658-670): ReLU as the prologue of ``first_hidden_to_hidden``, ReLU, ``single_hidden_to_spks``, sigmoid; rows at and beyond an item's
    length are zero.  ``hidden_to_spks`` is loaded and unused, as in the reference.

Weights travel as fp16 images with fp16 hi + lo activations (precision 4) like the Conformer's.

Batches.  ``Model.__call__`` takes a right-padded batch with ``lengths`` and item ``b`` equals the reference on that item alone (the Conformer's
stated batch semantics).  The reference's own padded batch gives its FastConformer layers no mask, so padding attends and convolves into the valid
frames there; that behaviour is not copied.

Streaming is v1: ``_compress_spkcache_simple``.  ``use_aosc=True`` (v2.1: AOSC compression, left / right context, the silence profile) raises
``NotImplementedError`` on every streaming entry point; the offline call does not depend on it.
"""
from __future__ import annotations

import json
import math
import time
from dataclasses import dataclass
from pathlib import Path
from typing import Dict, Generator, Iterable, List, Optional, Tuple, Union

import numpy as np
import torch

from .... import ops
from ....frontends import nemo_log_mel, per_feature_norm
from ....ops import ACT_LEAKY
from ....stt.models.parakeet import conformer as _conformer
from ....stt.models.parakeet.conformer import Conformer, ConformerArgs
from .config import FCEncoderConfig, ModelConfig, ModulesConfig, ProcessorConfig, TFEncoderConfig  # noqa: F401

_LOG_GUARD = 2 ** -24
_NORM_CONSTANT = 1e-5


def preemphasis_filter(waveform: torch.Tensor, coeff: float = 0.97) -> torch.Tensor:
    """y[n] = x[n] - coeff * x[n-1], first sample kept (sortformer.py:36-40)."""
    return torch.cat([waveform[..., :1], waveform[..., 1:] - coeff * waveform[..., :-1]], dim=-1)


def extract_mel_features(waveform, sample_rate: int = 16000, n_fft: int = 512, hop_length: int = 160, win_length: int = 400, n_mels: int = 80,
                         preemphasis_coeff: float = 0.97, normalize: Optional[str] = "per_feature", pad_to: int = 16) -> torch.Tensor:
    """``[num_samples]`` or ``[batch, num_samples]`` -> ``[batch, n_mels, num_frames]`` (frames zero-padded to a multiple of ``pad_to``)."""
    y = nemo_log_mel(waveform, sample_rate, n_fft, hop_length, win_length, n_mels, "hann", preemphasis_coeff, _LOG_GUARD)   # [B, frames, mels]
    feats = y.transpose(1, 2)
    if normalize == "per_feature":
        feats = per_feature_norm(feats, dim=2, eps=_NORM_CONSTANT)
    if pad_to > 0 and feats.shape[2] % pad_to:
        feats = torch.nn.functional.pad(feats, (0, pad_to - feats.shape[2] % pad_to))
    return feats.contiguous()


# ---------------------------------------------------------------------------------------------------- checkpoint names
FC_PREFIX, TF_PREFIX, MOD_PREFIX = "fc_encoder.", "tf_encoder.", "sortformer_modules."
# the Conformer engine's name fragment -> the reference Sortformer's
_FC_RENAMES = (("pre_encode.out.", "subsampling.linear."), ("pre_encode.conv.", "subsampling.layers_"), ("self_attn.linear_q.", "self_attn.q_proj."),
               ("self_attn.linear_k.", "self_attn.k_proj."), ("self_attn.linear_v.", "self_attn.v_proj."), ("self_attn.linear_out.", "self_attn.o_proj."),
               ("self_attn.linear_pos.", "self_attn.relative_k_proj."), ("self_attn.pos_bias_u", "self_attn.bias_u"),
               ("self_attn.pos_bias_v", "self_attn.bias_v"), ("conv.batch_norm.", "conv.norm."))
_ATT_BIASES = tuple(f"self_attn.{n}_proj.bias" for n in "qkvo")


def conformer_args(fc: FCEncoderConfig) -> ConformerArgs:
    """The ``ConformerArgs`` of ``FastConformerEncoder(fc)``.  ``use_bias`` stays True: ``attention_bias`` removes only the q / k / v / o biases in
    the reference (its feed-forward and convolution modules always have theirs), and the adapter supplies zeros for those four."""
    if fc.subsampling_conv_kernel_size != 3 or fc.subsampling_conv_stride != 2 or fc.subsampling_factor != 8:
        raise NotImplementedError(f"Sortformer: subsampling kernel {fc.subsampling_conv_kernel_size} / stride {fc.subsampling_conv_stride} / factor "
                                  f"{fc.subsampling_factor}: only the 3 x 3 / stride 2 / factor 8 dw-striding subsampler is built")
    if fc.intermediate_size % fc.hidden_size:
        raise ValueError(f"Sortformer: intermediate_size {fc.intermediate_size} is not a multiple of hidden_size {fc.hidden_size}")
    return ConformerArgs(feat_in=fc.num_mel_bins, n_layers=fc.num_hidden_layers, d_model=fc.hidden_size, n_heads=fc.num_attention_heads,
                         ff_expansion_factor=fc.intermediate_size // fc.hidden_size, subsampling_factor=fc.subsampling_factor,
                         self_attention_model="rel_pos", subsampling="dw_striding", conv_kernel_size=fc.conv_kernel_size,
                         subsampling_conv_channels=fc.subsampling_conv_channels, pos_emb_max_len=fc.max_position_embeddings, use_bias=True, xscaling=False)


def _to_reference_name(name: str) -> str:
    for ours, theirs in _FC_RENAMES:
        if ours in name:
            return name.replace(ours, theirs)
    return name


def adapt_fc_weights(weights: Dict[str, torch.Tensor], fc: FCEncoderConfig) -> Dict[str, torch.Tensor]:
    """``fc_encoder.*`` parameters under the names ``conformer.expected_shapes(args, "encoder.")`` wants:
    ``subsampling.layers_0/2/3/5/6`` -> ``pre_encode.conv.0/2/3/5/6``, ``subsampling.linear`` -> ``pre_encode.out``, ``self_attn.{q,k,v,o}_proj`` ->
    ``linear_{q,k,v,out}``, ``relative_k_proj`` -> ``linear_pos``, ``bias_u/v`` -> ``pos_bias_u/v``, ``conv.norm.*`` -> ``conv.batch_norm.*``; with
    ``attention_bias=False`` the four missing attention biases become zeros (adding 0 is exact)."""
    out: Dict[str, torch.Tensor] = {}
    for k, v in weights.items():
        if not k.startswith(FC_PREFIX):
            continue
        name = k[len(FC_PREFIX):]
        for ours, theirs in _FC_RENAMES:
            if theirs in name:
                name = name.replace(theirs, ours)
                break
        out["encoder." + name] = v
    if not fc.attention_bias:
        for i in range(fc.num_hidden_layers):
            for n in ("linear_q", "linear_k", "linear_v", "linear_out"):
                out.setdefault(f"encoder.layers.{i}.self_attn.{n}.bias", torch.zeros(fc.hidden_size))
    return out


def expected_shapes(config: ModelConfig) -> Dict[str, Tuple[int, ...]]:
    """Parameter name -> shape of the reference's ``Model(config)`` (its names, MLX conv layouts)."""
    fc, tf, mc = config.fc_encoder_config, config.tf_encoder_config, config.modules_config
    s: Dict[str, Tuple[int, ...]] = {}
    for name, shape in _conformer.expected_shapes(conformer_args(fc), "").items():
        ref = _to_reference_name(name)
        if not fc.attention_bias and ref.endswith(_ATT_BIASES):
            continue
        s[FC_PREFIX + ref] = shape

    def lin(name, n, k, bias=True):
        s[name + ".weight"] = (n, k)
        if bias:
            s[name + ".bias"] = (n,)

    d = tf.d_model
    s[TF_PREFIX + "embed_positions.weight"] = (tf.max_source_positions, d)
    for i in range(tf.encoder_layers):
        p = TF_PREFIX + f"layers.{i}."
        lin(p + "self_attn.q_proj", d, d)
        lin(p + "self_attn.k_proj", d, d, tf.k_proj_bias)
        lin(p + "self_attn.v_proj", d, d)
        lin(p + "self_attn.out_proj", d, d)
        for n in ("self_attn_layer_norm", "final_layer_norm"):
            s[p + n + ".weight"], s[p + n + ".bias"] = (d,), (d,)
        lin(p + "fc1", tf.encoder_ffn_dim, d)
        lin(p + "fc2", d, tf.encoder_ffn_dim)
    lin(MOD_PREFIX + "encoder_proj", mc.tf_d_model, mc.fc_d_model)
    lin(MOD_PREFIX + "first_hidden_to_hidden", mc.tf_d_model, mc.tf_d_model)
    lin(MOD_PREFIX + "single_hidden_to_spks", mc.num_speakers, mc.tf_d_model)
    lin(MOD_PREFIX + "hidden_to_spks", mc.num_speakers, 2 * mc.tf_d_model)
    return s


def make_sortformer_weights(config: ModelConfig, seed: int = 0, head_gain: float = 4.0, head_bias: float = 0.0) -> Dict[str, torch.Tensor]:
    """A seeded checkpoint under the reference's parameter names and MLX conv layouts, with the distributions of ``make_parakeet_weights``: matrices
    N(0, 1 / fan_in), biases 0.1 N(0, 1), LayerNorm / BatchNorm weights 1 + 0.1 N(0, 1), BatchNorm running mean 0.3 N(0, 1) and running variance
    in [0.5, 1.5], position biases 0.2 N(0, 1), learned positions 0.3 N(0, 1), the speaker head ``single_hidden_to_spks`` ``head_gain`` N(0, 1) /
    sqrt(d) with ``head_bias`` added to its bias.  float32 tensors holding fp16-representable values."""
    g = torch.Generator().manual_seed(seed)
    w: Dict[str, torch.Tensor] = {}
    for name, shape in expected_shapes(config).items():
        if name.endswith("running_var"):
            t = 0.5 + torch.rand(shape, generator=g)
        elif name.endswith("running_mean"):
            t = 0.3 * torch.randn(shape, generator=g)
        elif name.endswith(("self_attn.bias_u", "self_attn.bias_v")):
            t = 0.2 * torch.randn(shape, generator=g)
        elif name.endswith("embed_positions.weight"):
            t = 0.3 * torch.randn(shape, generator=g)
        elif name.endswith(".bias"):
            t = 0.1 * torch.randn(shape, generator=g)
            if name == MOD_PREFIX + "single_hidden_to_spks.bias":
                t = t + head_bias
        elif ".norm_" in name or ".conv.norm." in name or "layer_norm." in name:
            t = 1.0 + 0.1 * torch.randn(shape, generator=g)
        elif name == MOD_PREFIX + "single_hidden_to_spks.weight":
            t = head_gain * torch.randn(shape, generator=g) / math.sqrt(shape[-1])
        else:
            fan_in = 1
            for n in shape[1:]:
                fan_in *= n
            t = torch.randn(shape, generator=g) / math.sqrt(fan_in)
        w[name] = t.to(torch.float16).to(torch.float32)
    return w


# ---------------------------------------------------------------------------------------------------- output types
@dataclass
class DiarizationSegment:
    """A single diarization segment."""

    start: float
    end: float
    speaker: int


@dataclass
class DiarizationOutput:
    """Output from the diarization model."""

    segments: List[DiarizationSegment]
    speaker_probs: Optional[torch.Tensor] = None
    num_speakers: int = 0
    total_time: float = 0.0
    state: Optional["StreamingState"] = None

    @property
    def text(self) -> str:
        """RTTM-like text output."""
        lines = []
        for seg in self.segments:
            duration = seg.end - seg.start
            lines.append(f"SPEAKER audio 1 {seg.start:.3f} {duration:.3f} <NA> <NA> speaker_{seg.speaker} <NA> <NA>")
        return "\n".join(lines)


@dataclass
class StreamingState:
    """State between streaming chunks (sortformer.py:721-753): two buffers of UNSCALED pre-encoded embeddings (behind the subsampler, in front of the
    Conformer layers) with the predictions last made for them.  ``spkcache`` is the long-term context, compressed when full; ``fifo`` the recent
    one, whose oldest frames roll into ``spkcache``.  Tensors live on the model's device."""

    spkcache: torch.Tensor  # (1, cache_frames, emb_dim)
    spkcache_preds: torch.Tensor  # (1, cache_frames, n_spk)
    fifo: torch.Tensor  # (1, fifo_frames, emb_dim)
    fifo_preds: torch.Tensor  # (1, fifo_frames, n_spk)
    frames_processed: int  # total diarization frames emitted so far
    mean_sil_emb: torch.Tensor  # (1, emb_dim): the AOSC silence profile (v2.1), carried and never updated here
    n_sil_frames: torch.Tensor  # (1,)

    @property
    def spkcache_len(self) -> int:
        return self.spkcache.shape[1]

    @property
    def fifo_len(self) -> int:
        return self.fifo.shape[1]


def _aosc_not_built(what: str):
    raise NotImplementedError(f"Sortformer {what}: use_aosc=True (v2.1 streaming: AOSC speaker-cache compression, left / right chunk context, the "
                              "silence profile) is not built; v1 streaming (use_aosc=False) and the offline call are")


# ---------------------------------------------------------------------------------------------------- Transformer encoder + head
class TransformerEncoder:
    """``encoder_proj`` + ``TransformerEncoder(tf)`` + ``forward_speaker_sigmoids`` of the reference as an engine over [B, T, fc_d_model] rows."""

    def __init__(self, tf: TFEncoderConfig, mc: ModulesConfig, weights: Dict[str, torch.Tensor], device, precision: int = 4):
        ops.require_gpu()
        self.tf, self.mc, self.device, self.precision = tf, mc, torch.device(device), precision
        d, H = tf.d_model, tf.encoder_attention_heads
        if d % H or d // H not in ops.NARROW_ATTENTION_WIDTHS:
            raise ValueError(f"Sortformer: head width {d}/{H} is not one of {ops.NARROW_ATTENTION_WIDTHS} (the widths narrow_attention is built for)")
        if tf.activation_function != "relu":
            raise NotImplementedError(f"Sortformer: activation_function {tf.activation_function!r}: the reference's layer is ReLU")
        if mc.tf_d_model != d:
            raise ValueError(f"Sortformer: modules tf_d_model {mc.tf_d_model} != tf_encoder d_model {d}")
        dev = self.device
        w = weights
        lin = lambda name: ops.pack_conv(w[name + ".weight"], w.get(name + ".bias"), dev, f16=True)
        vec = lambda name: w[name].contiguous().to(dev)
        self.positions = vec(TF_PREFIX + "embed_positions.weight")
        self.layers = []
        for i in range(tf.encoder_layers):
            p = TF_PREFIX + f"layers.{i}.self_attn."
            kb = w[p + "k_proj.bias"] if tf.k_proj_bias else torch.zeros(d)
            qkv_w = torch.cat([w[p + "q_proj.weight"], w[p + "k_proj.weight"], w[p + "v_proj.weight"]])
            qkv_b = torch.cat([w[p + "q_proj.bias"], kb, w[p + "v_proj.bias"]])
            q = TF_PREFIX + f"layers.{i}."
            self.layers.append(dict(qkv=ops.pack_conv(qkv_w, qkv_b, dev, f16=True), out=lin(p + "out_proj"),
                                    ln1=(vec(q + "self_attn_layer_norm.weight"), vec(q + "self_attn_layer_norm.bias")),
                                    fc1=lin(q + "fc1"), fc2=lin(q + "fc2"),
                                    ln2=(vec(q + "final_layer_norm.weight"), vec(q + "final_layer_norm.bias"))))
        self.proj = lin(MOD_PREFIX + "encoder_proj")
        self.h2h = lin(MOD_PREFIX + "first_hidden_to_hidden")
        self.h2s = lin(MOD_PREFIX + "single_hidden_to_spks")

    def _f(self, *shape):
        return torch.empty(shape, dtype=torch.float32, device=self.device)

    def __call__(self, hidden: torch.Tensor, lens: List[int], lens_d: torch.Tensor, *, return_layers: bool = False):
        """FastConformer output [B, T, fc_d_model] -> preds [B, T, n_spk] (rows at and beyond ``lens[b]`` zero).  ``return_layers``: a second result,
        dict(encoder_proj, layers [n_layers], logits)."""
        tf, prec = self.tf, self.precision
        B, T, _ = hidden.shape
        if T > tf.max_source_positions:
            raise ValueError(f"Sortformer: {T} frames exceed max_source_positions = {tf.max_source_positions} (the learned position table)")
        d, H = tf.d_model, tf.encoder_attention_heads
        dh = d // H
        taps = dict(layers=[]) if return_layers else None
        x, x1, h = self._f(B, T, d), self._f(B, T, d), self._f(B, T, d)
        qkv, att, mid = self._f(B, T, 3 * d), self._f(B, T, d), self._f(B, T, tf.encoder_ffn_dim)
        if return_layers:
            taps["encoder_proj"] = ops.conv_gemm(hidden, self.proj, self._f(B, T, d), precision=prec)
        ops.conv_gemm(hidden, self.proj, x, res=self.positions[:T][None].expand(B, T, d), precision=prec)   # + embed_positions[:T]
        for blk in self.layers:
            ops.conv_gemm(x, blk["qkv"], qkv, precision=prec)
            ops.narrow_attention(qkv[:, :, 0:d], qkv[:, :, d:2 * d], qkv[:, :, 2 * d:], att, heads=H, dh=dh, scale=dh ** -0.5, lens=lens_d,
                                 check_lens=False)   # ``lens`` are host integers, checked by the caller
            ops.conv_gemm(att, blk["out"], h, precision=prec)
            ops.layernorm(h, x1, weight=blk["ln1"][0], bias=blk["ln1"][1], res=x, eps=tf.layer_norm_eps)
            ops.conv_gemm(x1, blk["fc1"], mid, post_act=ACT_LEAKY, post_slope=0.0, precision=prec)   # ReLU
            ops.conv_gemm(mid, blk["fc2"], h, precision=prec)
            ops.layernorm(h, x, weight=blk["ln2"][0], bias=blk["ln2"][1], res=x1, eps=tf.layer_norm_eps)
            if return_layers:
                taps["layers"].append(x.clone())
        ops.conv_gemm(x, self.h2h, h, pre_act=ACT_LEAKY, pre_slope=0.0, post_act=ACT_LEAKY, post_slope=0.0, precision=prec)
        logits = ops.conv_gemm(h, self.h2s, self._f(B, T, self.mc.num_speakers), precision=prec)
        mask = torch.arange(T, device=self.device)[None, :] < lens_d[:, None]
        preds = torch.sigmoid(logits) * mask[:, :, None]
        if return_layers:
            taps["logits"] = logits
            return preds, taps
        return preds


# ---------------------------------------------------------------------------------------------------- the model
class Model:
    """``Model(config)`` of the reference as an engine.  ``weights``: a checkpoint under the reference's names (MLX conv layouts); None: a seeded one
    (``make_sortformer_weights(config, seed)``)."""

    def __init__(self, config: ModelConfig, weights: Optional[Dict[str, torch.Tensor]] = None, device="cuda:0", seed: int = 0, precision: int = 4):
        self.config = config
        self.device, self.precision = torch.device(device), precision
        self._processor_config = config.processor_config
        if config.modules_config.fc_d_model != config.fc_encoder_config.hidden_size:
            raise ValueError(f"Sortformer: modules fc_d_model {config.modules_config.fc_d_model} != fc_encoder hidden_size {config.fc_encoder_config.hidden_size}")
        self.load_weights(make_sortformer_weights(config, seed) if weights is None else weights)

    # ------------------------------------------------------------------ checkpoint handling
    def load_weights(self, weights, strict: bool = True):
        """``weights``: a dict or a list of (name, tensor) pairs.  Missing or wrongly shaped parameters raise; unexpected ones raise under ``strict``."""
        cfg = self.config
        w = {k: torch.as_tensor(v).detach().to(torch.float32).cpu() for k, v in dict(weights).items()}
        shapes = expected_shapes(cfg)
        miss = [k for k in shapes if k not in w]
        if miss:
            raise ValueError(f"Sortformer.load_weights: missing parameters {miss[:4]}{' ...' if len(miss) > 4 else ''}")
        extra = [k for k in w if k not in shapes]
        if extra and strict:
            raise ValueError(f"Sortformer.load_weights: unexpected parameters {extra[:4]}{' ...' if len(extra) > 4 else ''}")
        for k, s in shapes.items():
            if tuple(w[k].shape) != s:
                raise ValueError(f"Sortformer.load_weights: {k} has shape {tuple(w[k].shape)}, expected {s}")
        w = {k: w[k] for k in shapes}
        self.fc_encoder = Conformer(conformer_args(cfg.fc_encoder_config), adapt_fc_weights(w, cfg.fc_encoder_config), device=self.device, prefix="encoder.",
                                    precision=self.precision)
        self.tf_encoder = TransformerEncoder(cfg.tf_encoder_config, cfg.modules_config, w, self.device, self.precision)
        return self

    def eval(self):
        return self

    @staticmethod
    def sanitize(weights: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        """HuggingFace names / PyTorch conv layouts -> the reference's (sortformer.py:2013-2065); a converted checkpoint (``subsampling.layers_N``
        keys) passes through unchanged."""
        sanitized = {}
        already_converted = any("subsampling.layers_" in k for k in weights)
        for k, v in weights.items():
            if "num_batches_tracked" in k:
                continue
            new_k = k
            if not already_converted:
                if "fc_encoder.subsampling.layers." in new_k:
                    new_k = new_k.replace("subsampling.layers.", "subsampling.layers_")
                if "subsampling" in new_k and "weight" in new_k and "linear" not in new_k:
                    if v.ndim == 4:   # Conv2d: (O, I, H, W) -> (O, H, W, I)
                        v = torch.as_tensor(v).permute(0, 2, 3, 1)
                if any(n in new_k for n in ("pointwise_conv1", "pointwise_conv2", "depthwise_conv")) and "weight" in new_k:
                    if v.ndim == 3:   # Conv1d: (O, I, K) -> (O, K, I)
                        v = torch.as_tensor(v).permute(0, 2, 1)
            sanitized[new_k] = v
        return sanitized

    @classmethod
    def from_pretrained(cls, path_or_hf_repo: str, *, device="cuda:0"):
        """A LOCAL directory holding ``config.json`` and ``model.safetensors``."""
        from safetensors.torch import load_file

        p = Path(path_or_hf_repo)
        if not (p / "config.json").exists() or not (p / "model.safetensors").exists():
            raise FileNotFoundError(f"{path_or_hf_repo}: Sortformer.from_pretrained needs a local directory (no hub access in this build)")
        with open(p / "config.json") as f:
            config = ModelConfig.from_dict(json.load(f))
        return cls(config, weights=cls.sanitize(load_file(str(p / "model.safetensors"))), device=device)

    # ------------------------------------------------------------------ forward
    def forward_embs(self, embs: torch.Tensor, lens: List[int], *, return_layers: bool = False):
        """UNSCALED pre-encoded embeddings [B, T', fc hidden] with the items' valid frames -> preds [B, T', n_spk]: ``scale_input``, the Conformer
        layers, the projection, the Transformer encoder, the head (``FastConformerEncoder.encode`` + the rest of ``Model.__call__``)."""
        fc = self.config.fc_encoder_config
        if embs.shape[1] > self.config.tf_encoder_config.max_source_positions:
            raise ValueError(f"Sortformer: {embs.shape[1]} frames exceed max_source_positions = {self.config.tf_encoder_config.max_source_positions} "
                             "(the learned position table)")
        x = embs * math.sqrt(fc.hidden_size) if fc.scale_input else embs.clone()
        out = self.fc_encoder.encode(x, lens, return_layers=return_layers, inplace=True)
        hidden, lens_d = out[0], out[1]
        res = self.tf_encoder(hidden, lens, lens_d, return_layers=return_layers)
        if return_layers:
            preds, taps = res
            taps["fc_layers"] = out[2]["layers"]
            return preds, taps
        return res

    def __call__(self, audio_signal: torch.Tensor, audio_signal_length=None, *, return_layers: bool = False):
        """features [B, n_mels, T] with ``lengths`` [B] (the valid mel frames of a right-padded batch; None: T) -> preds [B, T', n_spk] on the device,
        rows at and beyond an item's T' zero.  Item ``b`` equals the reference on that item alone; the reference's own padded batch lets the padding
        attend and convolve inside its FastConformer encoder, which is not copied."""
        feats = torch.as_tensor(audio_signal, dtype=torch.float32)
        if feats.dim() != 3 or feats.shape[1] != self.config.fc_encoder_config.num_mel_bins:
            raise ValueError(f"Sortformer: features must be [B, {self.config.fc_encoder_config.num_mel_bins}, T], got {tuple(feats.shape)}")
        embs, lens = self.fc_encoder.pre_encode(feats.to(self.device).transpose(1, 2), audio_signal_length)
        return self.forward_embs(embs, lens, return_layers=return_layers)

    def _features(self, waveform: torch.Tensor, **kw) -> torch.Tensor:
        proc = self._processor_config
        return extract_mel_features(waveform.to(self.device), sample_rate=proc.sampling_rate, n_fft=proc.n_fft, hop_length=proc.hop_length,
                                    win_length=proc.win_length, n_mels=proc.feature_size, preemphasis_coeff=proc.preemphasis, **kw)

    def _frame_duration(self) -> float:
        proc = self._processor_config
        return (proc.hop_length * self.config.fc_encoder_config.subsampling_factor) / proc.sampling_rate

    def generate(self, audio, *, sample_rate: int = 16000, threshold: float = 0.5, min_duration: float = 0.0, merge_gap: float = 0.0,
                 verbose: bool = False) -> DiarizationOutput:
        """Speaker diarization of a file path or a waveform in one piece (sortformer.py:811-900)."""
        start_time = time.time()
        waveform, sample_rate = self._load_audio(audio, sample_rate)
        proc = self._processor_config
        waveform, trim_offset = self._trim_silence(waveform, proc.sampling_rate)
        trim_offset_sec = trim_offset / proc.sampling_rate
        waveform = (1.0 / (waveform.abs().max() + 1e-3)) * waveform
        features = self._features(waveform)
        if verbose:
            print(f"Audio: {waveform.shape[-1] / proc.sampling_rate:.2f}s")
            if trim_offset > 0:
                print(f"Trimmed {trim_offset_sec:.2f}s leading silence")
            print(f"Features: {tuple(features.shape)}")
        preds = self(features, [features.shape[2]])
        segments = self._preds_to_segments(preds[0], frame_duration=self._frame_duration(), threshold=threshold, min_duration=min_duration,
                                           merge_gap=merge_gap)
        if trim_offset > 0:
            segments = [DiarizationSegment(start=seg.start + trim_offset_sec, end=seg.end + trim_offset_sec, speaker=seg.speaker) for seg in segments]
        active_speakers = set(seg.speaker for seg in segments)
        elapsed = time.time() - start_time
        if verbose:
            print(f"Found {len(segments)} segments with {len(active_speakers)} speakers")
            print(f"Processing time: {elapsed:.2f}s")
        return DiarizationOutput(segments=segments, speaker_probs=preds[0], num_speakers=len(active_speakers), total_time=elapsed)

    # ------------------------------------------------------------------ streaming (v1)
    def init_streaming_state(self) -> StreamingState:
        if self.config.modules_config.use_aosc:
            _aosc_not_built("init_streaming_state")
        emb_dim, n_spk = self.config.fc_encoder_config.hidden_size, self.config.modules_config.num_speakers
        z = lambda *s: torch.zeros(s, dtype=torch.float32, device=self.device)
        return StreamingState(spkcache=z(1, 0, emb_dim), spkcache_preds=z(1, 0, n_spk), fifo=z(1, 0, emb_dim), fifo_preds=z(1, 0, n_spk),
                              frames_processed=0, mean_sil_emb=z(1, emb_dim), n_sil_frames=z(1))

    def streaming_step(self, chunk_features: torch.Tensor, chunk_length, state: StreamingState,
                       right_context_embs: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, StreamingState]:
        """One chunk of mel features [1, n_mels, frames] (sortformer.py:926-1024): pre-encode it, run ``[spkcache + fifo + chunk]`` through the whole
        encoder, return the predictions of the new chunk alone [chunk frames, n_spk] and the state with the chunk pushed into the FIFO.  Left / right
        context is v2.1 only: ``right_context_embs`` is accepted and unused, as in the reference with ``use_aosc=False``."""
        if self.config.modules_config.use_aosc:
            _aosc_not_built("streaming_step")
        chunk_embs, lens = self.fc_encoder.pre_encode(torch.as_tensor(chunk_features, dtype=torch.float32).to(self.device).transpose(1, 2), chunk_length)
        chunk_diar_len = lens[0]
        chunk_embs = chunk_embs[:, :chunk_diar_len, :]
        parts = [t for t in (state.spkcache, state.fifo) if t.shape[1] > 0] + [chunk_embs]
        all_embs = torch.cat(parts, dim=1)
        all_preds = self.forward_embs(all_embs, [all_embs.shape[1]])
        chunk_start = state.spkcache_len + state.fifo_len
        chunk_preds = all_preds[:, chunk_start:chunk_start + chunk_diar_len, :]
        updated_cache_preds = all_preds[:, :state.spkcache_len, :]
        updated_fifo_preds = all_preds[:, state.spkcache_len:state.spkcache_len + state.fifo_len, :]
        new_state = self._update_streaming_state(state, chunk_embs, chunk_preds, updated_cache_preds, updated_fifo_preds)
        return chunk_preds[0], new_state

    def generate_stream(self, audio, *, state: Optional[StreamingState] = None, sample_rate: int = 16000, chunk_duration: float = 5.0,
                        threshold: float = 0.5, min_duration: float = 0.0, merge_gap: float = 0.0, spkcache_max: int = 188, fifo_max: int = 188,
                        verbose: bool = False) -> Generator[DiarizationOutput, None, None]:
        """Chunked diarization (sortformer.py:1026-1247), three input modes: a file path or a whole waveform (features normalised over the whole
        audio, fixed-duration chunks); an iterable of waveform chunks (each normalised alone: ``feed``); one chunk plus ``state`` (one result, with
        the new state attached)."""
        if self.config.modules_config.use_aosc:
            _aosc_not_built("generate_stream")
        is_array = isinstance(audio, (np.ndarray, torch.Tensor))
        if state is not None and is_array:
            result, new_state = self.feed(audio, state, sample_rate=sample_rate, threshold=threshold, min_duration=min_duration, merge_gap=merge_gap,
                                          spkcache_max=spkcache_max, fifo_max=fifo_max)
            result.state = new_state
            yield result
            return
        if not isinstance(audio, (str, Path)) and not is_array:
            yield from self._stream_from_chunks(audio, sample_rate=sample_rate, threshold=threshold, min_duration=min_duration, merge_gap=merge_gap,
                                                spkcache_max=spkcache_max, fifo_max=fifo_max, verbose=verbose)
            return
        waveform, sample_rate = self._load_audio(audio, sample_rate)
        proc = self._processor_config
        waveform, trim_offset = self._trim_silence(waveform, proc.sampling_rate)
        trim_offset_sec = trim_offset / proc.sampling_rate
        waveform = (1.0 / (waveform.abs().max() + 1e-3)) * waveform
        features = self._features(waveform)
        total_mel_frames = features.shape[2]
        subsampling_factor = self.config.fc_encoder_config.subsampling_factor
        frame_duration = self._frame_duration()
        chunk_mel = round(chunk_duration * proc.sampling_rate / proc.hop_length / subsampling_factor) * subsampling_factor
        chunk_mel = max(chunk_mel, subsampling_factor)
        if verbose:
            print(f"Streaming: {waveform.shape[-1] / proc.sampling_rate:.2f}s audio in {math.ceil(total_mel_frames / chunk_mel)} chunks "
                  f"({chunk_duration:.1f}s each)")
        state = self.init_streaming_state()
        offset_mel = chunk_idx = 0
        while offset_mel < total_mel_frames:
            end_mel = min(offset_mel + chunk_mel, total_mel_frames)
            chunk_feat = features[:, :, offset_mel:end_mel]
            chunk_preds, state = self.streaming_step(chunk_feat, [chunk_feat.shape[2]], state)
            chunk_time_offset = (offset_mel * proc.hop_length) / proc.sampling_rate
            segments = self._preds_to_segments(chunk_preds, frame_duration=frame_duration, threshold=threshold, min_duration=min_duration,
                                               merge_gap=merge_gap)
            segments = [DiarizationSegment(start=seg.start + chunk_time_offset + trim_offset_sec, end=seg.end + chunk_time_offset + trim_offset_sec,
                                           speaker=seg.speaker) for seg in segments]
            active_speakers = set(seg.speaker for seg in segments)
            if verbose:
                chunk_idx += 1
                t0 = chunk_time_offset + trim_offset_sec
                print(f"  Chunk {chunk_idx}: {t0:.2f}s-{t0 + chunk_preds.shape[0] * frame_duration:.2f}s  {len(segments)} segments, "
                      f"context={state.spkcache_len}+{state.fifo_len} frames")
            yield DiarizationOutput(segments=segments, speaker_probs=chunk_preds, num_speakers=len(active_speakers))
            state = self._maybe_compress_state(state, spkcache_max, fifo_max, self.config.modules_config)
            offset_mel = end_mel

    def _stream_from_chunks(self, audio_chunks: Iterable, *, sample_rate: int = 16000, threshold: float = 0.5, min_duration: float = 0.0,
                            merge_gap: float = 0.0, spkcache_max: int = 188, fifo_max: int = 188,
                            verbose: bool = False) -> Generator[DiarizationOutput, None, None]:
        state = self.init_streaming_state()
        chunk_idx = 0
        for raw_chunk in audio_chunks:
            result, state = self.feed(raw_chunk, state, sample_rate=sample_rate, threshold=threshold, min_duration=min_duration, merge_gap=merge_gap,
                                      spkcache_max=spkcache_max, fifo_max=fifo_max)
            if verbose:
                chunk_idx += 1
                print(f"  Chunk {chunk_idx}: {len(result.segments)} segments, context={state.spkcache_len}+{state.fifo_len} frames")
            yield result

    def feed(self, chunk, state: StreamingState, *, sample_rate: int = 16000, threshold: float = 0.5, min_duration: float = 0.0,
             merge_gap: float = 0.0, spkcache_max: int = 188, fifo_max: int = 188) -> Tuple[DiarizationOutput, StreamingState]:
        """One waveform chunk (mono float samples) as it arrives (sortformer.py:1287-1393): peak-normalised and feature-extracted on its own
        (``per_feature``, no frame padding), one ``streaming_step``, then the FIFO overflow moves into the speaker cache."""
        if self.config.modules_config.use_aosc:
            _aosc_not_built("feed")
        proc = self._processor_config
        frame_duration = self._frame_duration()
        chunk_t = torch.as_tensor(chunk).to(torch.float32).cpu()
        if chunk_t.dim() > 1:
            chunk_t = chunk_t.mean(dim=-1)
        if sample_rate != proc.sampling_rate:
            chunk_t = self._resample(chunk_t, sample_rate, proc.sampling_rate)
        chunk_time_offset = state.frames_processed * frame_duration
        chunk_t = (1.0 / (chunk_t.abs().max() + 1e-3)) * chunk_t
        features = self._features(chunk_t, normalize="per_feature", pad_to=0)
        chunk_preds, state = self.streaming_step(features, [features.shape[2]], state)
        segments = self._preds_to_segments(chunk_preds, frame_duration=frame_duration, threshold=threshold, min_duration=min_duration,
                                           merge_gap=merge_gap)
        segments = [DiarizationSegment(start=seg.start + chunk_time_offset, end=seg.end + chunk_time_offset, speaker=seg.speaker) for seg in segments]
        state = self._maybe_compress_state(state, spkcache_max, fifo_max, self.config.modules_config)
        active_speakers = set(seg.speaker for seg in segments)
        return DiarizationOutput(segments=segments, speaker_probs=chunk_preds, num_speakers=len(active_speakers)), state

    @staticmethod
    def _update_streaming_state(state: StreamingState, chunk_embs: torch.Tensor, chunk_preds: torch.Tensor, updated_cache_preds: torch.Tensor,
                                updated_fifo_preds: torch.Tensor) -> StreamingState:
        """Push the chunk into the FIFO; the context's predictions become the re-attended ones (sortformer.py:1395-1426)."""
        spkcache_preds = updated_cache_preds if state.spkcache_len > 0 else state.spkcache_preds
        fifo_preds = updated_fifo_preds if state.fifo_len > 0 else state.fifo_preds
        new_fifo = torch.cat([state.fifo, chunk_embs], dim=1)
        new_fifo_preds = torch.cat([fifo_preds, chunk_preds], dim=1)
        return StreamingState(spkcache=state.spkcache, spkcache_preds=spkcache_preds, fifo=new_fifo, fifo_preds=new_fifo_preds,
                              frames_processed=state.frames_processed + chunk_preds.shape[1], mean_sil_emb=state.mean_sil_emb,
                              n_sil_frames=state.n_sil_frames)

    @staticmethod
    def _maybe_compress_state(state: StreamingState, spkcache_max: int, fifo_max: int, modules_cfg: Optional[ModulesConfig] = None) -> StreamingState:
        """Move the FIFO's overflow into the speaker cache and compress the cache when it is over ``spkcache_max`` (sortformer.py:1428-1500)."""
        if modules_cfg is not None and modules_cfg.use_aosc:
            _aosc_not_built("_maybe_compress_state")
        if state.fifo_len <= fifo_max:
            return state
        pop_len = state.fifo_len - fifo_max
        new_cache = torch.cat([state.spkcache, state.fifo[:, :pop_len, :]], dim=1)
        new_cache_preds = torch.cat([state.spkcache_preds, state.fifo_preds[:, :pop_len, :]], dim=1)
        if new_cache.shape[1] > spkcache_max:
            new_cache, new_cache_preds = Model._compress_spkcache_simple(new_cache, new_cache_preds, spkcache_max)
        return StreamingState(spkcache=new_cache, spkcache_preds=new_cache_preds, fifo=state.fifo[:, pop_len:, :], fifo_preds=state.fifo_preds[:, pop_len:, :],
                              frames_processed=state.frames_processed, mean_sil_emb=state.mean_sil_emb, n_sil_frames=state.n_sil_frames)

    @staticmethod
    def _simple_keep_indices(preds: torch.Tensor, target_len: int) -> torch.Tensor:
        """The frames the v1 compression keeps, ascending: the ``target_len`` largest of sum_spk log(clip(preds, 1e-7, 1)) (sortformer.py:1819-1823).
        The scores are computed where ``preds`` live; the top-k runs over a few hundred values."""
        frame_scores = torch.log(torch.clamp(preds[0], 1e-7, 1.0)).sum(dim=-1)
        return torch.sort(torch.argsort(-frame_scores, stable=True)[:target_len]).values

    @staticmethod
    def _compress_spkcache_simple(embs: torch.Tensor, preds: torch.Tensor, target_len: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """v1 compression: keep the frames with the highest total speaker activity, in time order (sortformer.py:1800-1829)."""
        top = Model._simple_keep_indices(preds, target_len)
        return embs[:, top, :], preds[:, top, :]

    # ------------------------------------------------------------------ host logic
    @staticmethod
    def _preds_to_segments(preds, frame_duration: float, threshold: float = 0.5, min_duration: float = 0.0,
                           merge_gap: float = 0.0) -> List[DiarizationSegment]:
        """Frame-level probabilities [frames, speakers] -> time segments sorted by start (sortformer.py:1831-1905), on the host."""
        p = torch.as_tensor(preds).detach().to(torch.float32).cpu()
        _, num_speakers = p.shape
        segments: List[DiarizationSegment] = []
        for spk in range(num_speakers):
            activity = p[:, spk] > threshold
            if not bool(activity.any()):
                continue
            padded = torch.cat([torch.zeros(1, dtype=torch.bool), activity, torch.zeros(1, dtype=torch.bool)])
            changes_list = (padded[1:].to(torch.int32) - padded[:-1].to(torch.int32)).tolist()
            starts = [i for i, v in enumerate(changes_list) if v == 1]
            ends = [i for i, v in enumerate(changes_list) if v == -1]
            spk_segments = []
            for s, e in zip(starts, ends):
                start_time = s * frame_duration
                end_time = e * frame_duration
                duration = end_time - start_time
                if duration >= min_duration:
                    spk_segments.append(DiarizationSegment(start=start_time, end=end_time, speaker=spk))
            if merge_gap > 0 and len(spk_segments) > 1:
                merged = [spk_segments[0]]
                for seg in spk_segments[1:]:
                    if seg.start - merged[-1].end <= merge_gap:
                        merged[-1] = DiarizationSegment(start=merged[-1].start, end=seg.end, speaker=seg.speaker)
                    else:
                        merged.append(seg)
                spk_segments = merged
            segments.extend(spk_segments)
        segments.sort(key=lambda s: s.start)
        return segments

    @staticmethod
    def _trim_silence(waveform: torch.Tensor, sample_rate: int, frame_ms: int = 30, energy_ratio: float = 0.01,
                      min_speech_sec: float = 0.5) -> Tuple[torch.Tensor, int]:
        """Trim leading / trailing silence by frame energy (sortformer.py:1907-1967): (trimmed waveform, the samples cut off the front)."""
        frame_len = int(sample_rate * frame_ms / 1000)
        min_speech_frames = max(3, int(min_speech_sec * 1000 / frame_ms))
        num_frames = waveform.shape[0] // frame_len
        if num_frames < min_speech_frames * 2:
            return waveform, 0
        frames = waveform[:num_frames * frame_len].reshape(num_frames, frame_len)
        energy = torch.sqrt(torch.mean(frames ** 2, dim=1))
        threshold_val = energy.max().item() * energy_ratio
        speech_list = (energy > threshold_val).tolist()
        start_frame = 0
        for i in range(num_frames - min_speech_frames + 1):
            if all(speech_list[i:i + min_speech_frames]):
                start_frame = i
                break
        end_frame = num_frames
        for i in range(num_frames - 1, min_speech_frames - 2, -1):
            if all(speech_list[i - min_speech_frames + 1:i + 1]):
                end_frame = i + 1
                break
        start_sample = start_frame * frame_len
        end_sample = min(end_frame * frame_len, waveform.shape[0])
        if start_sample == 0 and end_sample == waveform.shape[0]:
            return waveform, 0
        return waveform[start_sample:end_sample], start_sample

    def _load_audio(self, audio, sample_rate: int) -> Tuple[torch.Tensor, int]:
        """A file path (``audio_io.read``), a numpy array or a tensor -> (mono float32 waveform on the host at the model's rate, that rate)."""
        if isinstance(audio, (str, Path)):
            from ....audio_io import read as audio_read

            waveform_np, sample_rate = audio_read(str(audio), dtype="float32")
            waveform = torch.from_numpy(np.ascontiguousarray(waveform_np))
        else:
            waveform = torch.as_tensor(audio).to(torch.float32).cpu()
        if waveform.dim() > 1:
            waveform = waveform.mean(dim=-1)
        proc = self._processor_config
        if sample_rate != proc.sampling_rate:
            waveform = self._resample(waveform, sample_rate, proc.sampling_rate)
        return waveform, proc.sampling_rate

    @staticmethod
    def _resample(waveform: torch.Tensor, orig_sr: int, target_sr: int) -> torch.Tensor:
        if orig_sr == target_sr:
            return waveform
        from ....utils import resample_audio

        return torch.as_tensor(resample_audio(waveform, orig_sr, target_sr)).to(torch.float32)
