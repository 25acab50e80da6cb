"""SenseVoice-Small on MI355X (stt/models/sensevoice/sensevoice.py): Kaldi fbank -> low-frame-rate stacking + CMVN + four query rows + sinusoidal
positions -> SAN-M encoder -> CTC head over the 25 055-entry vocabulary -> greedy collapse, language / emotion / event tags from the query rows.

The reference runs one un-padded clip per call.  What is built here is the model's meaning for a right-padded batch with per-item lengths: item ``b``
of a batch equals the reference on that item alone (padded frames are masked as keys, zeroed into and out of the FSMN conv, and never reach the
collapse).  ``generate_batch`` is the batched entry point; ``generate`` is a batch of one.

Host schedule:

  * input: ``dsp.compute_fbank_kaldi`` per clip (two launches), then ONE ``sanm_input`` for the batch: stacking (``lfr_m`` frames, hop ``lfr_n``), CMVN,
    the query embeddings ``[language, 1, 2, textnorm]``, ``* sqrt(output_size)`` and the position table (host float32, the reference's operation order,
    width ``input_size``; cached and grown on demand);
  * layer (``encoders0`` + ``encoders``, ``after_norm``, ``tp_encoders``, ``tp_norm``): LayerNorm -> one fused q | k | v GEMM -> ``fsmn_memory`` on the value
    third with ``add =`` the residual stream (the first layer, 560 -> 512, has none) -> attention under the items' lengths (``flash_attention`` for heads
    of 64 / 128, ``narrow_attention`` for 8 / 16 / 24 / 32) -> the out projection with ``res =`` the FSMN result -> LayerNorm -> w_1 (ReLU) -> w_2 with
    ``res=``.  ``sanm_shift > 0`` is folded into the packed taps: a left padding of ``(K - 1) / 2 + shift`` is a centred kernel of ``K + 2 shift`` taps
    whose last ``2 shift`` taps are zero;
  * head: ``ctc_lo`` as a ``conv_gemm`` over ``CTC_CHUNK_ROWS`` rows at a time into a fixed logits workspace, ``ctc_rows`` on the chunk (arg-max, top-2
    gap, arg-max log-probability), ``ctc_collapse`` on the ids; one device-to-host copy per batch.  The [rows, V] matrix exists only when ``__call__`` is
    asked for the log-probabilities.

Weights travel as fp16 images with fp16 hi + lo activations (precision 4) like the Parakeet and Mel-RoFormer engines; FSMN taps, LayerNorm parameters,
the query embeddings and the CMVN vectors stay float32.

Not built: hub download and checkpoint conversion (``from_pretrained`` takes a local directory in the reference's MLX layout), the ``fun_asr_nano``
family (its encoder is this one; its LLM side is missing) and bf16 checkpoints.
"""
from __future__ import annotations

import json
import math
import re
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from .... import ops
from ....ops import ACT_LEAKY
from ..base import STTOutput
from .config import ModelConfig

LN_EPS = 1e-5          # mlx.nn.LayerNorm's default
FLASH_WIDTHS = (64, 128)
CTC_CHUNK_ROWS = 2048  # rows of the logits workspace (206 MB at the published vocabulary).  Measured at 64 x 171 rows (profiles/sanm_kernels_vs_torch.jsonl):
                       # 256 / 512 / 1024 / 2048 / 4096 / all rows -> 5130 / 2742 / 1480 / 1162 / 1192 / 1126 us for the GEMM + ctc_rows
BPE_MODEL = "chn_jpn_yue_eng_ko_spectok.bpe.model"

LID_DICT = {"auto": 0, "zh": 3, "en": 4, "yue": 7, "ja": 11, "ko": 12, "nospeech": 13}
TEXTNORM_DICT = {"withitn": 14, "woitn": 15}
EMO_DICT = {"unk": 25009, "happy": 25001, "sad": 25002, "angry": 25003, "neutral": 25004}
LID_MAP = {24884: "zh", 24885: "en", 24888: "yue", 24892: "ja", 24896: "ko", 24992: "nospeech"}
EMO_MAP = {25001: "happy", 25002: "sad", 25003: "angry", 25004: "neutral", 25005: "fearful", 25006: "disgusted", 25007: "surprised", 25008: "other",
           25009: "unk"}
EVENT_MAP = {24993: "Speech", 24995: "BGM", 24997: "Laughter", 24999: "Applause"}


def _parse_am_mvn(path: str) -> Tuple[List[float], List[float]]:
    """The Kaldi-nnet ``am.mvn`` file: the ``<AddShift>`` row (negative means) and the ``<Rescale>`` row (inverse standard deviations)."""
    with open(path) as f:
        text = f.read()
    out = []
    for tag in ("AddShift", "Rescale"):
        m = re.search(rf"<{tag}>.*?<LearnRateCoef>\s+\d+\s+\[(.*?)\]", text, re.DOTALL)
        if not m:
            raise ValueError(f"Could not parse {tag} from am.mvn")
        out.append([float(x) for x in m.group(1).split()])
    return out[0], out[1]


def position_table(rows: int, width: int) -> torch.Tensor:
    """``SinusoidalPositionEncoder`` (sensevoice.py:106-122) for positions 1 .. rows: float32 [rows, width] on the host, in the reference's operation
    order -- sines in the first half of the columns, cosines in the second."""
    if width % 2 or width < 4:
        raise ValueError(f"SenseVoice: the position encoding needs an even input width of at least 4 (got {width})")
    half = width // 2
    inc = math.log(10000) / (half - 1)
    inv = torch.exp(torch.arange(half, dtype=torch.float32) * torch.tensor(-inc, dtype=torch.float32))
    t = torch.arange(1, rows + 1, dtype=torch.float32)[:, None] * inv[None, :]
    return torch.cat([torch.sin(t), torch.cos(t)], dim=1).contiguous()


def fold_fsmn_taps(w: torch.Tensor, shift: int) -> torch.Tensor:
    """[C, K] taps applied behind a left padding of ``(K - 1) / 2 + shift`` -> the centred [C, K + 2 shift] kernel ``fsmn_memory`` takes."""
    C, K = w.shape
    if K % 2 == 0:
        raise ValueError(f"SenseVoice: kernel_size {K} must be odd")
    if shift < 0 or shift > (K - 1) // 2:
        raise ValueError(f"SenseVoice: sanm_shift {shift} leaves a negative right padding for kernel_size {K}")
    if K + 2 * shift > ops.FSMN_MAX_TAPS:
        raise ValueError(f"SenseVoice: kernel_size {K} with sanm_shift {shift} needs {K + 2 * shift} taps, MI355_FSMN_MAX_TAPS is {ops.FSMN_MAX_TAPS}")
    return torch.cat([w, torch.zeros((C, 2 * shift), dtype=w.dtype)], dim=1).contiguous()


def layer_names(config: ModelConfig) -> List[Tuple[str, int]]:
    """(parameter prefix, input width) of every encoder layer in execution order."""
    enc = config.encoder_conf
    d = enc.output_size
    return ([("encoder.encoders0.0.", config.input_size)] + [(f"encoder.encoders.{i}.", d) for i in range(enc.num_blocks - 1)]
            + [(f"encoder.tp_encoders.{i}.", d) for i in range(enc.tp_blocks)])


def expected_shapes(config: ModelConfig) -> Dict[str, Tuple[int, ...]]:
    """Parameter name -> shape of ``SenseVoiceSmall(config)`` (the reference's names, MLX conv layout)."""
    enc = config.encoder_conf
    d, ff, K = enc.output_size, enc.linear_units, enc.kernel_size
    s: Dict[str, Tuple[int, ...]] = {}

    def lin(name, n, k):
        s[name + ".weight"], s[name + ".bias"] = (n, k), (n,)

    for p, din in layer_names(config):
        s[p + "norm1.weight"], s[p + "norm1.bias"] = (din,), (din,)
        lin(p + "self_attn.linear_q_k_v", 3 * d, din)
        s[p + "self_attn.fsmn_block.weight"] = (d, K, 1)
        lin(p + "self_attn.linear_out", d, d)
        s[p + "norm2.weight"], s[p + "norm2.bias"] = (d,), (d,)
        lin(p + "feed_forward.w_1", ff, d)
        lin(p + "feed_forward.w_2", d, ff)
    for n in ("encoder.after_norm", "encoder.tp_norm"):
        s[n + ".weight"], s[n + ".bias"] = (d,), (d,)
    lin("ctc_lo", config.vocab_size, d)
    s["embed.weight"] = (16, config.input_size)
    return s


def make_sensevoice_weights(config: ModelConfig, seed: int = 0, head_gain: float = 4.0, blank_bias: float = 0.0) -> Dict[str, torch.Tensor]:
    """A seeded checkpoint under the reference's parameter names: matrices N(0, 1 / fan_in), biases 0.1 N(0, 1), LayerNorm weights 1 + 0.1 N(0, 1), FSMN
    taps N(0, 1 / K), query embeddings 0.5 N(0, 1), the CTC head ``head_gain`` N(0, 1) / sqrt(d) with ``blank_bias`` added to the blank's (id 0) bias.
    float32 tensors holding fp16-representable values, like a checkpoint published in fp16 (the engine packs fp16 weight images)."""
    g = torch.Generator().manual_seed(seed)
    w: Dict[str, torch.Tensor] = {}
    for name, shape in expected_shapes(config).items():
        if name.endswith("fsmn_block.weight"):
            t = torch.randn(shape, generator=g) / math.sqrt(shape[1])
        elif name == "embed.weight":
            t = 0.5 * torch.randn(shape, generator=g)
        elif name.endswith(".bias"):
            t = 0.1 * torch.randn(shape, generator=g)
        elif "norm" in name:
            t = 1.0 + 0.1 * torch.randn(shape, generator=g)
        elif name.startswith("ctc_lo."):
            t = head_gain * torch.randn(shape, generator=g) / math.sqrt(shape[-1])
        else:
            t = torch.randn(shape, generator=g) / math.sqrt(shape[-1])
        if name == "ctc_lo.bias":
            t[0] += blank_bias
        w[name] = t.to(torch.float16).to(torch.float32)
    return w


class SenseVoiceSmall:
    """``SenseVoiceSmall(config)`` of the reference as an engine; ``weights`` omitted = a seeded checkpoint (the reference: freshly initialised)."""

    def __init__(self, config: ModelConfig, weights: Optional[Dict[str, torch.Tensor]] = None, device="cuda:0", seed: int = 0, precision: int = 4,
                 ctc_chunk_rows: int = CTC_CHUNK_ROWS):
        enc, fc = config.encoder_conf, config.frontend_conf
        d, H = enc.output_size, enc.attention_heads
        if d % H or d // H not in FLASH_WIDTHS + ops.NARROW_ATTENTION_WIDTHS:
            raise ValueError(f"SenseVoice: head width {d}/{H} is none of {FLASH_WIDTHS} (flash_attention) or {ops.NARROW_ATTENTION_WIDTHS} (narrow_attention)")
        if config.input_size != fc.lfr_m * fc.n_mels:
            raise ValueError(f"SenseVoice: input_size {config.input_size} is not lfr_m * n_mels = {fc.lfr_m} * {fc.n_mels}")
        if enc.num_blocks < 1 or enc.tp_blocks < 0 or ctc_chunk_rows < 1:
            raise ValueError("SenseVoice: num_blocks must be at least 1, tp_blocks and ctc_chunk_rows non-negative")
        fold_fsmn_taps(torch.zeros((1, enc.kernel_size)), enc.sanm_shift)
        position_table(1, config.input_size)
        ops.require_gpu()
        assert precision in (3, 4)
        self.config, self.device, self.precision, self.ctc_chunk_rows = config, torch.device(device), precision, int(ctc_chunk_rows)
        self.lid_dict, self.textnorm_dict, self.emo_dict = dict(LID_DICT), dict(TEXTNORM_DICT), dict(EMO_DICT)
        self.blank_id = 0
        self._cmvn_means: Optional[torch.Tensor] = None
        self._cmvn_istd: Optional[torch.Tensor] = None
        self._tokenizer = None
        self._token_list: Optional[List[str]] = None
        self._pe: Optional[torch.Tensor] = None
        self._ctc_ws: Optional[torch.Tensor] = None
        self.load_weights(make_sensevoice_weights(config, seed) if weights is None else weights)

    # ------------------------------------------------------------------ checkpoint handling
    @staticmethod
    def sanitize(weights: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        """The reference's two rules: ``ctc.ctc_lo.`` -> ``ctc_lo.``, and a 3-d ``fsmn_block.weight`` [C, 1, K] (PyTorch) -> [C, K, 1] (MLX)."""
        out = {}
        for k, v in weights.items():
            k = k.replace("ctc.ctc_lo.", "ctc_lo.")
            if "fsmn_block.weight" in k and v.dim() == 3:
                v = v.transpose(1, 2)
            out[k] = v
        return out

    def load_weights(self, weights, strict: bool = True):
        c, dev = self.config, self.device
        enc = c.encoder_conf
        weights = dict(weights)
        if any(torch.as_tensor(v).dtype == torch.bfloat16 for v in weights.values()):
            raise NotImplementedError("SenseVoiceSmall.load_weights: bf16 checkpoints are not built (the weight images are fp16)")
        w = {k: torch.as_tensor(v).detach().to(torch.float32).cpu() for k, v in weights.items()}
        shapes = expected_shapes(c)
        miss = [k for k in shapes if k not in w]
        if miss:
            raise ValueError(f"SenseVoiceSmall.load_weights: missing parameters {miss[:4]}{' ...' if len(miss) > 4 else ''}")
        extra = [k for k in w if k not in shapes]
        if extra and strict:
            raise ValueError(f"SenseVoiceSmall.load_weights: unexpected parameters {extra[:4]}{' ...' if len(extra) > 4 else ''}")
        for k, s in shapes.items():
            if tuple(w[k].shape) != s:
                raise ValueError(f"SenseVoiceSmall.load_weights: {k} has shape {tuple(w[k].shape)}, expected {s}")

        lin = lambda n: ops.pack_conv(w[n + ".weight"], w[n + ".bias"], dev, f16=True)
        norm = lambda n: (w[n + ".weight"].contiguous().to(dev), w[n + ".bias"].contiguous().to(dev))
        self.layers = []
        for p, din in layer_names(c):
            self.layers.append(dict(din=din, norm1=norm(p + "norm1"), qkv=lin(p + "self_attn.linear_q_k_v"),
                                    fsmn=fold_fsmn_taps(w[p + "self_attn.fsmn_block.weight"][:, :, 0], enc.sanm_shift).to(dev),
                                    out=lin(p + "self_attn.linear_out"), norm2=norm(p + "norm2"), w1=lin(p + "feed_forward.w_1"),
                                    w2=lin(p + "feed_forward.w_2")))
        self.after_norm, self.tp_norm = norm("encoder.after_norm"), norm("encoder.tp_norm")
        self.ctc_lo = lin("ctc_lo")
        self.embed = w["embed.weight"].contiguous().to(dev)
        return self

    def set_cmvn(self, means: Optional[Sequence[float]], istd: Optional[Sequence[float]]):
        if means is None or istd is None:
            self._cmvn_means = self._cmvn_istd = None
            return self
        m, s = torch.tensor(list(means), dtype=torch.float32), torch.tensor(list(istd), dtype=torch.float32)
        if m.numel() != self.config.input_size or s.numel() != self.config.input_size:
            raise ValueError(f"SenseVoice: CMVN vectors of {m.numel()} / {s.numel()} entries for an input width of {self.config.input_size}")
        self._cmvn_means, self._cmvn_istd = m.to(self.device), s.to(self.device)
        return self

    @staticmethod
    def post_load_hook(model: "SenseVoiceSmall", model_path) -> "SenseVoiceSmall":
        """CMVN from ``am.mvn`` (else from the config's statistics), the tokenizer from the sentencepiece model when sentencepiece is importable and
        the file is there, else the ``tokens.json`` list, else none (ids joined by spaces)."""
        model_path = Path(model_path)
        if (model_path / "am.mvn").exists():
            model.set_cmvn(*_parse_am_mvn(str(model_path / "am.mvn")))
        if model._cmvn_means is None and model.config.cmvn_means is not None:
            model.set_cmvn(model.config.cmvn_means, model.config.cmvn_istd)
        bpe_path, tokens_path = model_path / BPE_MODEL, model_path / "tokens.json"
        if bpe_path.exists():
            try:
                import sentencepiece as spm

                sp = spm.SentencePieceProcessor()
                sp.Load(str(bpe_path))
                model._tokenizer = sp
            except ImportError:
                pass
        if model._tokenizer is None and tokens_path.exists():
            with open(tokens_path) as f:
                model._token_list = json.load(f)
        return model

    @classmethod
    def from_pretrained(cls, path: Union[str, Path], *, device="cuda:0") -> "SenseVoiceSmall":
        """A LOCAL directory holding ``config.json`` and ``model.safetensors`` (the reference's parameter names), optionally ``am.mvn``, the
        sentencepiece model and ``tokens.json``."""
        from safetensors.torch import load_file

        p = Path(path)
        if not (p / "config.json").exists() or not (p / "model.safetensors").exists():
            raise FileNotFoundError(f"{path}: SenseVoiceSmall.from_pretrained needs a local directory with config.json and model.safetensors "
                                    "(hub download and checkpoint conversion are not built)")
        with open(p / "config.json") as f:
            config = ModelConfig.from_dict(json.load(f))
        config.model_path = str(p)
        model = cls(config, weights=cls.sanitize(load_file(str(p / "model.safetensors"))), device=device)
        return cls.post_load_hook(model, p)

    # ------------------------------------------------------------------ input
    def _f(self, *shape):
        return torch.empty(shape, dtype=torch.float32, device=self.device)

    def _positions(self, rows: int) -> torch.Tensor:
        if self._pe is None or self._pe.shape[0] < rows:
            cap = max(256, 1 << (rows - 1).bit_length())
            self._pe = position_table(cap, self.config.input_size).to(self.device)
        return self._pe

    def _fbank(self, audio) -> torch.Tensor:
        """Waveform in [-1, 1] -> Kaldi fbank [T, n_mels] on the device (``_compute_fbank``: the samples scaled by 2^15, hamming, pre-emphasis 0.97)."""
        from .... import dsp

        fc = self.config.frontend_conf
        x = torch.as_tensor(audio, dtype=torch.float32).reshape(-1) * float(1 << 15)
        fb = dsp.compute_fbank_kaldi(x, sample_rate=fc.fs, win_len=int(fc.fs * fc.frame_length / 1000), win_inc=int(fc.fs * fc.frame_shift / 1000),
                                     num_mels=fc.n_mels, win_type=fc.window, preemphasis=0.97, dither=0.0, snip_edges=True, low_freq=20.0, high_freq=0.0)
        if fb.shape[0] < 1:
            raise ValueError(f"SenseVoice: audio of {x.numel()} samples is too short for one {fc.frame_length} ms frame")
        return fb

    def _qids(self, batch_size: int, language, use_itn: bool) -> torch.Tensor:
        langs = [language] * batch_size if isinstance(language, str) else list(language)
        if len(langs) != batch_size:
            raise ValueError(f"SenseVoice: {len(langs)} languages for a batch of {batch_size}")
        tn = self.textnorm_dict["withitn" if use_itn else "woitn"]
        return torch.tensor([[self.lid_dict.get(l, 0), 1, 2, tn] for l in langs], dtype=torch.int32)

    def _build_query(self, batch_size: int, language="auto", use_itn: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
        """(textnorm_query [B, 1, W], input_query [B, 3, W]): the embedding rows the reference concatenates around the features.  ``language``: one
        string for the batch or one per item."""
        q = self.embed[self._qids(batch_size, language, use_itn).to(self.device).long()]
        return q[:, 3:4], q[:, 0:3]

    def _pad(self, items: Sequence[torch.Tensor]) -> Tuple[torch.Tensor, List[int]]:
        lens = [int(t.shape[0]) for t in items]
        if len(items) == 1:
            return items[0][None].contiguous(), lens
        batch = torch.zeros((len(items), max(lens), items[0].shape[1]), dtype=torch.float32, device=self.device)
        for i, t in enumerate(items):
            batch[i, :lens[i]] = t
        return batch, lens

    def _check_lens(self, lens, B: int, T: int) -> List[int]:
        lens = [T] * B if lens is None else [int(v) for v in torch.as_tensor(lens).reshape(-1).tolist()]
        if len(lens) != B or min(lens) < 1 or max(lens) > T:
            raise ValueError(f"SenseVoice: lengths {lens} do not fit a batch of {B} items of {T} frames (every item needs at least one frame)")
        return lens

    def _assemble(self, feats: torch.Tensor, lens: List[int], language, use_itn: bool, *, stacked: bool, positions: bool = True):
        """fbank [B, T, n_mels] (or, ``stacked``, features already stacked and normalised [B, T, input_size]) -> (x [B, R, input_size], out_lens)."""
        fc = self.config.frontend_conf
        B, T = feats.shape[0], feats.shape[1]
        m, n = (1, 1) if stacked else (fc.lfr_m, fc.lfr_n)
        cmvn = not stacked and self._cmvn_means is not None and self._cmvn_istd is not None
        pe = self._positions(ops.sanm_rows(T, n)) if positions else None
        return ops.sanm_input(feats, self.embed, self._qids(B, language, use_itn).to(self.device), pe, lfr_m=m, lfr_n=n,
                              scale=math.sqrt(self.config.encoder_conf.output_size) if positions else 1.0,
                              lens=torch.tensor(lens, dtype=torch.int32, device=self.device), means=self._cmvn_means if cmvn else None,
                              istd=self._cmvn_istd if cmvn else None)

    def _extract_features(self, audio) -> torch.Tensor:
        """Waveform -> the stacked, normalised features [ceil(T / lfr_n), input_size] (the reference's ``_extract_features``: no query rows, no scale,
        no positions), through the same kernel as the fused path."""
        fb = self._fbank(audio)[None]
        x, _ = self._assemble(fb, [fb.shape[1]], "auto", False, stacked=False, positions=False)
        return x[0, 4:]

    # ------------------------------------------------------------------ encoder
    def _attention(self, q, k, v, out, lens_d):
        enc = self.config.encoder_conf
        H, dh = enc.attention_heads, enc.output_size // enc.attention_heads
        if dh in FLASH_WIDTHS:
            return ops.flash_attention(q, k, v, out, heads=H, dh=dh, scale=dh ** -0.5, lens_k=lens_d)
        if dh in ops.NARROW_ATTENTION_WIDTHS:
            return ops.narrow_attention(q, k, v, out, heads=H, dh=dh, scale=dh ** -0.5, lens=lens_d, check_lens=False)   # lens come from checked host integers
        raise ValueError(f"SenseVoice: no attention kernel for heads of {dh}")

    def encode(self, x: torch.Tensor, lens_d: torch.Tensor, *, return_layers: bool = False):
        """Assembled input [B, R, input_size] (``sanm_input``'s output) and the items' valid rows int32 [B] -> hidden [B, R, output_size]; with
        ``return_layers`` also dict(layers: every layer's output, attn0: the first layer's attention-module output)."""
        c, prec = self.config, self.precision
        enc = c.encoder_conf
        B, R, _ = x.shape
        d = enc.output_size
        nb = enc.normalize_before
        h, qkv, mem, att, mid = self._f(B, R, d), self._f(B, R, 3 * d), self._f(B, R, d), self._f(B, R, d), self._f(B, R, enc.linear_units)
        taps = dict(layers=[]) if return_layers else None
        if self.layers[0]["din"] == d:
            x = x.clone()   # layers of equal width work in place: the caller keeps its input
        for i, blk in enumerate(self.layers):
            if i == enc.num_blocks:
                x = ops.layernorm(x, self._f(B, R, d), weight=self.after_norm[0], bias=self.after_norm[1], eps=LN_EPS)
            same = blk["din"] == d
            src = x
            if nb:
                src = ops.layernorm(x, h if same else self._f(B, R, blk["din"]), weight=blk["norm1"][0], bias=blk["norm1"][1], eps=LN_EPS)
            ops.conv_gemm(src, blk["qkv"], qkv, precision=prec)
            q, k, v = qkv[:, :, 0:d], qkv[:, :, d:2 * d], qkv[:, :, 2 * d:]
            self._attention(q, k, v, att, lens_d)
            if return_layers and i == 0:
                bare = ops.fsmn_memory(v, blk["fsmn"], self._f(B, R, d), lens=lens_d)
                taps["attn0"] = ops.conv_gemm(att, blk["out"], self._f(B, R, d), res=bare, precision=prec)
            ops.fsmn_memory(v, blk["fsmn"], mem, add=x if same else None, lens=lens_d)
            if not same:
                x = self._f(B, R, d)    # the first layer changes the width and has no attention residual
            ops.conv_gemm(att, blk["out"], x, res=mem, precision=prec)   # (x +) out(att) + fsmn
            src = ops.layernorm(x, h, weight=blk["norm2"][0], bias=blk["norm2"][1], eps=LN_EPS) if nb else x
            ops.conv_gemm(src, blk["w1"], mid, post_act=ACT_LEAKY, post_slope=0.0, precision=prec)   # ReLU
            ops.conv_gemm(mid, blk["w2"], x, res=x, precision=prec)
            if return_layers:
                taps["layers"].append(x.clone())
        if enc.tp_blocks == 0:
            x = ops.layernorm(x, self._f(B, R, d), weight=self.after_norm[0], bias=self.after_norm[1], eps=LN_EPS)
        x = ops.layernorm(x, self._f(B, R, d), weight=self.tp_norm[0], bias=self.tp_norm[1], eps=LN_EPS)
        return (x, taps) if return_layers else x

    # ------------------------------------------------------------------ CTC head
    def _workspace(self, rows: int) -> torch.Tensor:
        ld = ops.round_up(self.config.vocab_size, 64)
        if self._ctc_ws is None or self._ctc_ws.shape[0] < rows:
            self._ctc_ws = self._f(rows, ld)
        return self._ctc_ws

    def head(self, hidden: torch.Tensor, *, return_logp: bool = False):
        """hidden [B, R, d] -> (ids int32 [B, R], gap [B, R], lp [B, R]) on the device (and, ``return_logp``, the log-probabilities [B, R, V]), the
        ``ctc_lo`` GEMM and ``ctc_rows`` running over ``ctc_chunk_rows`` rows at a time."""
        B, R, d = hidden.shape
        V, rows = self.config.vocab_size, B * R
        assert hidden.is_contiguous()
        flat = hidden.view(1, rows, d)
        ids = torch.empty((rows,), dtype=torch.int32, device=self.device)
        gap, lp = self._f(rows), self._f(rows)
        logp = self._f(rows, V) if return_logp else None
        chunk = min(self.ctc_chunk_rows, rows)
        ws = None if return_logp else self._workspace(chunk)
        for r0 in range(0, rows, chunk):
            r1 = min(r0 + chunk, rows)
            lo = logp[r0:r1] if return_logp else ws[:r1 - r0, :V]
            ops.conv_gemm(flat[:, r0:r1], self.ctc_lo, lo[None], precision=self.precision)
            ops.ctc_rows(lo, ids=ids[r0:r1], gap=gap[r0:r1], lp=lp[r0:r1], logp=lo if return_logp else None)
        out = (ids.view(B, R), gap.view(B, R), lp.view(B, R))
        return out + (logp.view(B, R, V),) if return_logp else out

    def __call__(self, feats, language="auto", use_itn: bool = False, *, lengths=None) -> torch.Tensor:
        """Stacked, normalised features [B, T, input_size] (``_extract_features``' output) -> log-probabilities [B, 4 + T, V] on the device.
        ``lengths`` (extra): the valid frames of a right-padded batch; rows at and beyond ``4 + lengths[b]`` are then meaningless."""
        feats = torch.as_tensor(feats, dtype=torch.float32)
        if feats.dim() != 3 or feats.shape[2] != self.config.input_size:
            raise ValueError(f"SenseVoice: feats must be [B, T, {self.config.input_size}], got {tuple(feats.shape)}")
        lens = self._check_lens(lengths, feats.shape[0], feats.shape[1])
        x, out_lens = self._assemble(feats.to(self.device).contiguous(), lens, language, use_itn, stacked=True)
        return self.head(self.encode(x, out_lens), return_logp=True)[3]

    # ------------------------------------------------------------------ decoding
    def _decode_tokens(self, token_ids: List[int]) -> str:
        if self._tokenizer is not None:
            return self._tokenizer.decode(token_ids)
        if self._token_list is not None:
            pieces = [self._token_list[t] for t in token_ids if 0 <= t < len(self._token_list)]
            return "".join(pieces).replace("▁", " ").strip()
        return " ".join(str(t) for t in token_ids)

    def _row_ids(self, log_probs) -> torch.Tensor:
        lp = torch.as_tensor(log_probs, dtype=torch.float32).to(self.device)
        return ops.ctc_rows(lp.reshape(-1, lp.shape[-1]).contiguous())[0]

    def _greedy_ctc_decode(self, log_probs) -> Tuple[List[int], str]:
        """log-probabilities (or logits) [T, V] -> (token ids, text): arg-max per row, repeats dropped, then blanks."""
        tokens, counts = ops.ctc_collapse(self._row_ids(log_probs)[None], blank=self.blank_id)
        token_ids = tokens[0, :int(counts[0])].tolist()
        return token_ids, self._decode_tokens(token_ids)

    @staticmethod
    def _rich_info(ids: Sequence[int]) -> Dict[str, str]:
        lid, emo, event = int(ids[0]), int(ids[1]), int(ids[2])
        return dict(language=LID_MAP.get(lid, "unknown"), emotion=EMO_MAP.get(emo, f"token_{emo}"), event=EVENT_MAP.get(event, f"token_{event}"))

    def _extract_rich_info(self, log_probs) -> Dict[str, str]:
        """The arg-max of the first three rows (language, emotion, event) through the tag tables."""
        return self._rich_info(self._row_ids(log_probs)[:3].tolist())

    def transcribe_fbank(self, fbanks: Sequence[torch.Tensor], language="auto", use_itn: bool = False, *, return_layers: bool = False) -> dict:
        """fbanks: one [T_i, n_mels] device tensor per item -> dict(x: the assembled input, out_lens, hidden, ids / gap / lp [B, R], tokens: one id list
        per item, rich: one tag dict per item, and with ``return_layers`` the encoder's taps).  One device-to-host copy."""
        feats, lens = self._pad([torch.as_tensor(f, dtype=torch.float32).to(self.device) for f in fbanks])
        if feats.dim() != 3 or feats.shape[2] != self.config.frontend_conf.n_mels:
            raise ValueError(f"SenseVoice: fbank items must be [T, {self.config.frontend_conf.n_mels}], got {tuple(feats.shape[1:])}")
        lens = self._check_lens(lens, feats.shape[0], feats.shape[1])
        x, out_lens = self._assemble(feats, lens, language, use_itn, stacked=False)
        r = dict(x=x, out_lens=out_lens)
        if return_layers:
            r["hidden"], r["taps"] = self.encode(x, out_lens, return_layers=True)
        else:
            r["hidden"] = self.encode(x, out_lens)
        r["ids"], r["gap"], r["lp"] = self.head(r["hidden"])
        tokens, counts = ops.ctc_collapse(r["ids"], lens=out_lens, skip=4, blank=self.blank_id)
        host = torch.cat([r["ids"][:, :3], counts[:, None], tokens], dim=1).cpu()
        r["tokens"] = [host[b, 4:4 + int(host[b, 3])].tolist() for b in range(host.shape[0])]
        r["rich"] = [self._rich_info(host[b, :3].tolist()) for b in range(host.shape[0])]
        return r

    def _load(self, audio) -> torch.Tensor:
        if isinstance(audio, (str, Path)):
            from ...utils import load_audio

            return torch.from_numpy(np.ascontiguousarray(load_audio(str(audio), sr=self.config.frontend_conf.fs), dtype=np.float32))
        if isinstance(audio, (np.ndarray, torch.Tensor)):
            return torch.as_tensor(audio, dtype=torch.float32)
        raise TypeError(f"Unsupported audio type: {type(audio)}")

    def generate_batch(self, audios: Sequence, *, language="auto", use_itn: bool = False, verbose: bool = False, **kwargs) -> List[STTOutput]:
        """One encoder pass over all clips (paths, numpy arrays or tensors); each result equals ``generate`` on that clip alone.  ``language``: one
        string or one per clip."""
        for k in ("max_tokens", "generation_stream", "dtype"):
            kwargs.pop(k, None)
        r = self.transcribe_fbank([self._fbank(self._load(a)) for a in audios], language, use_itn)
        out = []
        for token_ids, info in zip(r["tokens"], r["rich"]):
            text = self._decode_tokens(token_ids)
            if verbose:
                print(f"Language: {info['language']}\nEmotion: {info['emotion']}\nEvent: {info['event']}\nText: {text}")
            out.append(STTOutput(text=text, language=info["language"],
                                 segments=[dict(text=text, language=info["language"], emotion=info["emotion"], event=info["event"])]))
        return out

    def generate(self, audio, *, language: str = "auto", use_itn: bool = False, verbose: bool = False, **kwargs) -> STTOutput:
        return self.generate_batch([audio], language=language, use_itn=use_itn, verbose=verbose, **kwargs)[0]
