"""FireRedASR2-AED on MI355X (stt/models/fireredasr2/fireredasr2.py): Kaldi fbank -> CMVN -> Conv2dSubsampling -> Conformer encoder (relative-position
attention, a 33-tap convolution module normalised by a LayerNorm over 2 d_model channels) -> Transformer decoder driven by beam search.

The reference runs one clip per call.  ``generate_batch`` (new here) runs right-padded clips with lengths in lockstep; each item equals that item
alone.  ``generate`` is a batch of one.

Host schedule:

  * front end: ``dsp.compute_fbank_kaldi`` per clip (x 32768 when the waveform lies in [-1, 1]), CMVN, then the batch as one zero-padded
    ``[N, Tmax + 6, idim]`` buffer with ``lens``: ``subsample2d_k3s2`` reads rows at and beyond ``lens[b]`` as zero, which is each item's own six
    zero frames of right context; the second conv writes ``[N, T', C, F']`` so the ``out`` linear reads rows of ``C F'`` without a transposed copy;
  * encoder layer: FFN (``layernorm`` -> ``net_1`` with swish as its epilogue -> ``net_4`` with ``res=``; the block's ``0.5 x + 0.5 ffn(x)`` is
    ``x + 0.5 net_4(...)``, the 0.5 folded into ``net_4`` at load, exactly) -> three ``layernorm`` launches (q, k, v norms of one input) and three
    projections into one fused buffer -> ``relpos_attention`` against the layer's projected position table (row ``T' - 1`` is distance 0 for every
    item) -> ``fc`` with ``res=`` -> ``layernorm`` -> pointwise conv 1 -> ``glu_dwconv_ln_swish`` -> pointwise conv 2 with ``res=`` -> FFN ->
    ``layernorm``;
  * decoder: the cross k | v of every layer are projected ONCE per utterance and shared by its beams (``flash_attention`` with the B beams of an
    utterance as B query rows over the same keys); per step and layer the new position's k | v go into slot (utterance, beam) of a cache that is
    never re-gathered, ``beam_attention`` reads each beam's history through the indirection table ``beam_step`` maintains; logits from
    ``tgt_word_prj``; ``beam_step`` advances every live utterance and freezes the finished ones; ``done`` is polled every ``POLL`` steps;
  * the GNMT length penalty and the final pick are a few tensor ops per utterance on the host.

Linears are ``conv_gemm`` at precision 4 on fp16 weight images; the decoder's, at up to 8 rows, are ``gemv`` on row-major fp16 images of the same
weights, as ``WhisperEngine._linear`` chooses.  The decoder keeps k / v per layer, not layer outputs as the reference does: the same values.

Not built, each raising by name: hub download, bf16 / quantised checkpoints, head widths other than 64 / 128, beams above 8, the reference's README
extras beyond ``generate``.  Deliberately absent from ``MODEL_REMAPPING`` and the generic loader, like Moonshine.
"""
from __future__ import annotations

import json
import math
import re
import time
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from .... import ops
from ....ops import ACT_GELU, ACT_SILU
from ..base import STTOutput
from .config import ModelConfig

LN_EPS = 1e-5       # mlx.nn.LayerNorm default
GEMV_ROWS = 8       # rows up to which a decoder linear takes the GEMV (WhisperEngine._linear's choice for a decode step)
SUB_C = 32          # Conv2dSubsampling's out_channels
CONTEXT = 7         # left 3 + current + right 3: the encoder pads CONTEXT - 1 zero frames on the right
POLL = 4            # beam-search steps between two reads of the ``done`` flags
INF = 1e10


def sub_len(n: int) -> int:
    """Rows behind one 3 x 3 / stride 2 conv without padding; 0 when there are fewer than 3."""
    return (n - 3) // 2 + 1 if n >= 3 else 0


def encoder_frames(n_fbank: int) -> int:
    """Encoder rows of a clip of ``n_fbank`` fbank frames (six zero frames appended, two convs)."""
    return sub_len(sub_len(n_fbank + CONTEXT - 1))


def rel_pe_table(T: int, d: int) -> torch.Tensor:
    """RelPositionalEncoding.__call__ (fireredasr2.py:42-66) for T rows: [2 T - 1, d], row T - 1 + p holds position -p (row T - 1 is distance 0),
    built with the reference's float32 numpy operations."""
    pos = np.arange(0, T, dtype=np.float32)[:, None]
    div = np.exp(np.arange(0, d, 2, dtype=np.float32) * -(math.log(10000.0) / d))
    pp, pn = np.zeros((T, d), dtype=np.float32), np.zeros((T, d), dtype=np.float32)
    pp[:, 0::2], pp[:, 1::2] = np.sin(pos * div), np.cos(pos * div)
    pn[:, 0::2], pn[:, 1::2] = np.sin(-pos * div), np.cos(-pos * div)
    return torch.from_numpy(np.concatenate([pp[::-1].copy(), pn[1:]], axis=0))


def abs_pe_table(rows: int, d: int) -> torch.Tensor:
    """PositionalEncoding (fireredasr2.py:236-249): [rows, d]."""
    pos = np.arange(0, rows, dtype=np.float32)[:, None]
    div = np.exp(np.arange(0, d, 2, dtype=np.float32) * -(math.log(10000.0) / d))
    pe = np.zeros((rows, d), dtype=np.float32)
    pe[:, 0::2], pe[:, 1::2] = np.sin(pos * div), np.cos(pos * div)
    return torch.from_numpy(pe)


def expected_shapes(c: ModelConfig) -> Dict[str, Tuple[int, ...]]:
    """Parameter name -> shape of the reference's ``Model(config)`` (MLX layouts: Conv2d [out, 3, 3, in], Conv1d [out, K, in])."""
    e, dc = c.encoder, c.decoder
    d, K, H = e.d_model, e.kernel_size, e.n_head
    s: Dict[str, Tuple[int, ...]] = {}

    def ln(p, n):
        s[p + ".weight"], s[p + ".bias"] = (n,), (n,)

    def lin(p, o, i, bias=True):
        s[p + ".weight"] = (o, i)
        if bias:
            s[p + ".bias"] = (o,)

    ip = "encoder.input_preprocessor"
    s[ip + ".conv1.weight"], s[ip + ".conv1.bias"] = (SUB_C, 3, 3, 1), (SUB_C,)
    s[ip + ".conv2.weight"], s[ip + ".conv2.bias"] = (SUB_C, 3, 3, SUB_C), (SUB_C,)
    lin(ip + ".out", d, SUB_C * (((c.idim - 1) // 2 - 1) // 2))
    for i in range(e.n_layers):
        p = f"encoder.layer_stack.{i}"
        for f in ("ffn1", "ffn2"):
            ln(f"{p}.{f}.net_0", d)
            lin(f"{p}.{f}.net_1", 4 * d, d)
            lin(f"{p}.{f}.net_4", d, 4 * d)
        for n in ("w_qs", "w_ks", "w_vs", "fc", "linear_pos"):
            lin(f"{p}.mhsa.{n}", d, d, False)
        for n in ("layer_norm_q", "layer_norm_k", "layer_norm_v"):
            ln(f"{p}.mhsa.{n}", d)
        s[p + ".mhsa.pos_bias_u"] = s[p + ".mhsa.pos_bias_v"] = (H, d // H)
        ln(p + ".conv.pre_layer_norm", d)
        s[p + ".conv.pointwise_conv1.weight"] = (4 * d, 1, d)
        s[p + ".conv.depthwise_conv.weight"] = (2 * d, K, 1)
        ln(p + ".conv.batch_norm", 2 * d)
        s[p + ".conv.pointwise_conv2.weight"] = (d, 1, 2 * d)
        ln(p + ".layer_norm", d)
    dd = dc.d_model
    s["decoder.tgt_word_emb.weight"] = (c.odim, dd)
    for i in range(dc.n_layers):
        p = f"decoder.layer_stack.{i}"
        for a in ("self_attn", "cross_attn"):
            ln(f"{p}.{a}_norm", dd)
            lin(f"{p}.{a}.w_qs", dd, dd)
            lin(f"{p}.{a}.w_ks", dd, dd, False)
            lin(f"{p}.{a}.w_vs", dd, dd)
            lin(f"{p}.{a}.fc", dd, dd)
        ln(p + ".mlp_norm", dd)
        lin(p + ".mlp.w_1", 4 * dd, dd)
        lin(p + ".mlp.w_2", dd, 4 * dd)
    ln("decoder.layer_norm_out", dd)
    s["decoder.tgt_word_prj.weight"] = (c.odim, dd)
    return s


def make_fireredasr2_weights(config: ModelConfig, seed: int = 0, logit_gain: float = 6.0, eos_gain: float = 1.0) -> Dict[str, torch.Tensor]:
    """A seeded checkpoint under the reference's parameter names: matrices N(0, 1 / fan_in), biases 0.1 N(0, 1), norm weights 1 + 0.1 N(0, 1), the
    position biases 0.1 N(0, 1), the embedding N(0, 1) / sqrt(d) (the decoder scales it by sqrt(d)); the output projection ``logit_gain`` N(0, 1) /
    sqrt(d) with its EOS row scaled by ``eos_gain``.  float32 tensors holding fp16-representable values, like a checkpoint published in fp16."""
    g = torch.Generator().manual_seed(seed)
    w: Dict[str, torch.Tensor] = {}
    for name, shape in expected_shapes(config).items():
        if "norm" in name or "net_0" in name:
            t = (0.0 if name.endswith(".bias") else 1.0) + 0.1 * torch.randn(shape, generator=g)
        elif name.endswith(".bias") or "pos_bias" in name:
            t = 0.1 * torch.randn(shape, generator=g)
        elif name == "decoder.tgt_word_prj.weight":
            t = logit_gain * torch.randn(shape, generator=g) / math.sqrt(shape[-1])
            t[config.eos_id] *= eos_gain
        elif name == "decoder.tgt_word_emb.weight":
            t = torch.randn(shape, generator=g) / math.sqrt(shape[-1])
        else:
            fan_in = int(np.prod(shape[1:]))
            t = torch.randn(shape, generator=g) / math.sqrt(fan_in)
        w[name] = t.to(torch.float16).to(torch.float32)
    return w


class FireRedASR2:
    """``FireRedASR2(config)`` of the reference as an engine; ``weights`` omitted = a seeded checkpoint (the reference: freshly initialised)."""

    def __init__(self, config: Union[ModelConfig, dict], weights: Optional[Dict[str, torch.Tensor]] = None, device="cuda:0", seed: int = 0,
                 precision: int = 4):
        if isinstance(config, dict):
            config = ModelConfig.from_dict(config)
        c = config
        for side, cfg in (("encoder", c.encoder), ("decoder", c.decoder)):
            if cfg.d_model % cfg.n_head:
                raise ValueError(f"FireRedASR2: {side} heads {cfg.n_head} do not divide d_model {cfg.d_model}")
            if cfg.d_model // cfg.n_head not in (64, 128):
                raise NotImplementedError(f"FireRedASR2: {side} head width {cfg.d_model // cfg.n_head} is not built (relpos_attention, flash_attention "
                                          "and beam_attention take heads of 64 or 128)")
        if c.encoder.d_model != c.decoder.d_model:
            raise NotImplementedError("FireRedASR2: encoder and decoder widths differ (the cross-attention keys are projected from d_model)")
        if 2 * c.encoder.d_model > ops.GLU_DWCONV_LN_MAX_C or c.encoder.kernel_size > ops.GLU_DWCONV_LN_MAX_TAPS or c.encoder.kernel_size % 2 == 0:
            raise NotImplementedError(f"FireRedASR2: d_model {c.encoder.d_model} / kernel_size {c.encoder.kernel_size} is beyond glu_dwconv_ln_swish "
                                      f"({ops.GLU_DWCONV_LN_MAX_C // 2} channels, {ops.GLU_DWCONV_LN_MAX_TAPS} odd taps)")
        ops.require_gpu()
        assert precision in (3, 4)
        self.config, self.device, self.precision = c, torch.device(device), precision
        self._tokenizer: Optional[List[str]] = None
        self._sp = None
        self._cmvn: Optional[Tuple[torch.Tensor, torch.Tensor]] = None
        self._pos_cache = None
        self.load_weights(make_fireredasr2_weights(c, seed) if weights is None else weights)

    @property
    def sample_rate(self) -> int:
        return 16000

    # ------------------------------------------------------------------ checkpoint handling
    def sanitize(self, weights: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        """The reference's rules (fireredasr2.py:618-656): ``conv.0`` / ``conv.2`` of the subsampler become ``conv1`` / ``conv2``, ``.net.N.`` becomes
        ``.net_N.``, Conv1d weights [out, in, K] become [out, K, in], 4-D subsampler weights [out, in, H, W] become [out, H, W, in], and a missing
        ``decoder.tgt_word_prj.weight`` is tied to the embedding."""
        out = {}
        for k, v in weights.items():
            nk = k.replace("input_preprocessor.conv.0.", "input_preprocessor.conv1.").replace("input_preprocessor.conv.2.", "input_preprocessor.conv2.")
            nk = re.sub(r"\.net\.(\d+)\.", r".net_\1.", nk)
            v = torch.as_tensor(v)
            if "pointwise_conv1.weight" in nk or "pointwise_conv2.weight" in nk or "depthwise_conv.weight" in nk:
                v = v.permute(0, 2, 1)
            elif "input_preprocessor.conv" in nk and "weight" in nk and v.dim() == 4:
                v = v.permute(0, 2, 3, 1)
            out[nk] = v
        if "decoder.tgt_word_prj.weight" not in out and "decoder.tgt_word_emb.weight" in out:
            out["decoder.tgt_word_prj.weight"] = out["decoder.tgt_word_emb.weight"]
        return out

    def load_weights(self, weights, strict: bool = True):
        c, dev = self.config, self.device
        weights = {k: v for k, v in dict(weights).items() if not k.endswith("positional_encoding.pe")}   # tables, rebuilt here
        for k, v in weights.items():
            dt = torch.as_tensor(v).dtype
            if dt == torch.bfloat16:
                raise NotImplementedError("FireRedASR2.load_weights: bf16 checkpoints are not built (the weight images are fp16)")
            if not dt.is_floating_point:
                raise NotImplementedError(f"FireRedASR2.load_weights: quantised checkpoints are not built ({k} is {dt})")
        w = {k: torch.as_tensor(v).detach().to(torch.float32).cpu() for k, v in weights.items()}
        shapes = expected_shapes(c)
        miss = [k for k in shapes if k not in w]
        if miss:
            raise ValueError(f"FireRedASR2.load_weights: missing parameters {miss[:4]}{' ...' if len(miss) > 4 else ''}")
        extra = [k for k in w if k not in shapes]
        if extra and strict:
            raise ValueError(f"FireRedASR2.load_weights: unexpected parameters {extra[:4]}{' ...' if len(extra) > 4 else ''}")
        for k, s in shapes.items():
            if tuple(w[k].shape) != s:
                raise ValueError(f"FireRedASR2.load_weights: {k} has shape {tuple(w[k].shape)}, expected {s}")
        pack = lambda wt, b=None: ops.pack_conv(wt.contiguous(), b, dev, f16=True)
        vec = lambda n: w[n].contiguous().to(dev)
        ln = lambda p: (vec(p + ".weight"), vec(p + ".bias"))
        lin = lambda p, scale=1.0: pack(w[p + ".weight"].reshape(w[p + ".weight"].shape[0], -1) * scale,
                                        w[p + ".bias"] * scale if p + ".bias" in w else None)
        dlin = lambda p: (lin(p), ops.pack_rowmajor16(w[p + ".weight"].contiguous(), w.get(p + ".bias"), dev, f16=True))
        ip = "encoder.input_preprocessor"
        self.sub = dict(w1=vec(ip + ".conv1.weight"), b1=vec(ip + ".conv1.bias"), w2=vec(ip + ".conv2.weight"), b2=vec(ip + ".conv2.bias"),
                        out=lin(ip + ".out"))
        self.enc_layers = []
        for i in range(c.encoder.n_layers):
            p = f"encoder.layer_stack.{i}"
            ffn = lambda f: dict(ln=ln(f"{p}.{f}.net_0"), up=lin(f"{p}.{f}.net_1"), down=lin(f"{p}.{f}.net_4", 0.5))   # 0.5 x + 0.5 ffn(x): exact in the weights
            self.enc_layers.append(dict(
                ffn1=ffn("ffn1"), ffn2=ffn("ffn2"),
                lnq=ln(p + ".mhsa.layer_norm_q"), lnk=ln(p + ".mhsa.layer_norm_k"), lnv=ln(p + ".mhsa.layer_norm_v"),
                wq=lin(p + ".mhsa.w_qs"), wk=lin(p + ".mhsa.w_ks"), wv=lin(p + ".mhsa.w_vs"), fc=lin(p + ".mhsa.fc"), pos=lin(p + ".mhsa.linear_pos"),
                bias_u=vec(p + ".mhsa.pos_bias_u").reshape(-1), bias_v=vec(p + ".mhsa.pos_bias_v").reshape(-1),
                cln=ln(p + ".conv.pre_layer_norm"), pw1=lin(p + ".conv.pointwise_conv1"), dw=w[p + ".conv.depthwise_conv.weight"][:, :, 0].contiguous().to(dev),
                bn=ln(p + ".conv.batch_norm"), pw2=lin(p + ".conv.pointwise_conv2"), ln=ln(p + ".layer_norm")))
        self.embed = vec("decoder.tgt_word_emb.weight")
        self.dec_pe = abs_pe_table(c.decoder.pe_maxlen, c.decoder.d_model).to(dev)
        self.dec_layers = []
        for i in range(c.decoder.n_layers):
            p = f"decoder.layer_stack.{i}"
            kv_w = torch.cat([w[p + ".self_attn.w_ks.weight"], w[p + ".self_attn.w_vs.weight"]], 0)
            d = c.decoder.d_model
            zb = torch.zeros(d)
            qkv_w = torch.cat([w[p + ".self_attn.w_qs.weight"], kv_w], 0)
            qkv_b = torch.cat([w[p + ".self_attn.w_qs.bias"], zb, w[p + ".self_attn.w_vs.bias"]], 0)
            ckv_w = torch.cat([w[p + ".cross_attn.w_ks.weight"], w[p + ".cross_attn.w_vs.weight"]], 0)
            ckv_b = torch.cat([zb, w[p + ".cross_attn.w_vs.bias"]], 0)
            self.dec_layers.append(dict(
                ln1=ln(p + ".self_attn_norm"), qkv=(pack(qkv_w, qkv_b), ops.pack_rowmajor16(qkv_w.contiguous(), qkv_b, dev, f16=True)),
                o=dlin(p + ".self_attn.fc"), ln2=ln(p + ".cross_attn_norm"), cq=dlin(p + ".cross_attn.w_qs"), ckv=pack(ckv_w, ckv_b),
                co=dlin(p + ".cross_attn.fc"), ln3=ln(p + ".mlp_norm"), w1=dlin(p + ".mlp.w_1"), w2=dlin(p + ".mlp.w_2")))
        self.dec_norm = ln("decoder.layer_norm_out")
        self.head = dlin("decoder.tgt_word_prj")
        self._pos_cache = None
        return self

    def set_cmvn(self, means, istd):
        self._cmvn = (torch.as_tensor(means, dtype=torch.float32).to(self.device), torch.as_tensor(istd, dtype=torch.float32).to(self.device))

    def _load_cmvn(self, model_path):
        p = Path(model_path) / "cmvn.json"
        if p.exists():
            with open(p) as f:
                data = json.load(f)
            self.set_cmvn(data["means"], data["istd"])

    def _load_tokenizer(self, model_path):
        """``dict.txt``: one token per line, the first field; ``<space>`` is a blank (fireredasr2.py:501-526).  ``train_bpe1000.model`` is loaded by the
        reference but never used to detokenise; it is not read here."""
        p = Path(model_path) / "dict.txt"
        if p.exists():
            id2word = []
            with open(p, encoding="utf8") as f:
                for line in f:
                    tokens = line.strip().split()
                    word = tokens[0] if tokens else " "
                    id2word.append(" " if word == "<space>" else word)
            self._tokenizer = id2word

    def _detokenize(self, ids) -> str:
        if self._tokenizer is None:
            return ""
        text = "".join(self._tokenizer[int(i)] for i in ids if 0 <= int(i) < len(self._tokenizer))
        text = text.replace("▁", " ").strip()
        return re.sub(r"(<blank>)|(<sil>)", "", text).lower()

    @staticmethod
    def post_load_hook(model: "FireRedASR2", model_path) -> "FireRedASR2":
        model._load_cmvn(str(model_path))
        model._load_tokenizer(str(model_path))
        return model

    @classmethod
    def from_pretrained(cls, path: Union[str, Path], *, device="cuda:0") -> "FireRedASR2":
        """A LOCAL directory holding ``config.json`` and ``model.safetensors`` (the reference's or the PyTorch names), optionally ``cmvn.json`` and
        ``dict.txt``."""
        from safetensors.torch import load_file

        p = Path(path)
        if not (p / "config.json").exists() or not (p / "model.safetensors").exists():
            raise FileNotFoundError(f"{path}: FireRedASR2.from_pretrained needs a local directory with config.json and model.safetensors "
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

    def _lens(self, lens: Sequence[int]) -> torch.Tensor:
        return torch.tensor(list(lens), dtype=torch.int32, device=self.device)

    @staticmethod
    def _rows(t: torch.Tensor) -> Optional[torch.Tensor]:
        """[B, L, C] view -> its [B L, C] rows when they are evenly spaced (a slice of a dense buffer), else None."""
        B, L, C = t.shape
        if B > 1 and t.stride(0) != L * t.stride(1):
            return None
        return t.as_strided((B * L, C), (t.stride(1), 1))

    def _lin(self, x, lin, y, *, post_act: int = 0, res=None):
        """``y = act(x W^T + b) (+ res)`` on [B, L, C] views: ``conv_gemm``, or for a decoder linear (``(MFMA image, row-major image)``) of up to
        ``GEMV_ROWS`` rows the GEMV."""
        if isinstance(lin, tuple):
            pc, rm = lin
            if x.shape[0] * x.shape[1] <= GEMV_ROWS:
                rows = [self._rows(t) for t in (x, y) + (() if res is None else (res,))]
                if all(r is not None for r in rows):
                    ops.gemv(rows[0], rm, rows[1], post_act=post_act, res=None if res is None else rows[2])
                    return y
        else:
            pc = lin
        return ops.conv_gemm(x, pc, y, precision=self.precision, post_act=post_act, res=res)

    def _ln(self, x, wb, y=None, lens=None):
        return ops.layernorm(x, self._f(*x.shape) if y is None else y, weight=wb[0], bias=wb[1], eps=LN_EPS, lens=lens)

    # ------------------------------------------------------------------ front end
    def _load(self, audio) -> torch.Tensor:
        if isinstance(audio, (str, Path)):
            from ...utils import load_audio

            return torch.from_numpy(np.ascontiguousarray(load_audio(str(audio), sr=self.sample_rate), dtype=np.float32))
        if isinstance(audio, (np.ndarray, torch.Tensor, list, tuple)):
            return torch.as_tensor(np.asarray(audio) if isinstance(audio, (list, tuple)) else audio, dtype=torch.float32).reshape(-1)
        raise TypeError(f"Unsupported audio type: {type(audio)}")

    def _extract_fbank(self, audio) -> torch.Tensor:
        """Waveform -> Kaldi fbank [T, 80] on the device; a waveform within [-1, 1] is scaled to the int16 range first (fireredasr2.py:540-557)."""
        from .... import dsp

        x = self._load(audio)
        if x.numel() and float(x.abs().max()) <= 1.0:
            x = x * 32768.0
        return dsp.compute_fbank_kaldi(x, sample_rate=16000, win_len=400, win_inc=160, num_mels=80, snip_edges=True, dither=0.0)

    def features(self, audios: Sequence) -> Tuple[torch.Tensor, List[int]]:
        """Clips -> (CMVN-normalised fbank, zero-padded [N, Tmax + 6, idim], frames per item)."""
        fbs = []
        for a in audios:
            fb = self._extract_fbank(a)
            if fb.shape[0] < 1:
                raise ValueError("FireRedASR2: audio shorter than one fbank frame (400 samples)")
            if self._cmvn is not None:
                fb = (fb - self._cmvn[0]) * self._cmvn[1]
            fbs.append(fb)
        ns = [int(f.shape[0]) for f in fbs]
        buf = torch.zeros((len(fbs), max(ns) + CONTEXT - 1, self.config.idim), dtype=torch.float32, device=self.device)
        for b, f in enumerate(fbs):
            buf[b, :ns[b]] = f
        return buf, ns

    # ------------------------------------------------------------------ encoder
    def _positions(self, T: int) -> List[torch.Tensor]:
        """Every layer's projected position table [2 T - 1, d_model] for a batch whose longest item has T rows."""
        if self._pos_cache is not None and self._pos_cache[0] == T:
            return self._pos_cache[1]
        d = self.config.encoder.d_model
        pe = rel_pe_table(T, d).to(self.device)[None]
        tables = []
        for blk in self.enc_layers:
            p = self._f(1, 2 * T - 1, d)
            self._lin(pe, blk["pos"], p)
            tables.append(p[0])
        self._pos_cache = (T, tables)
        return tables

    def subsample(self, feats: torch.Tensor, ns: Sequence[int]):
        """Padded features [N, Tmax + 6, idim] and frame counts -> (x [N, T', d_model], rows per item)."""
        N, Tp, F = feats.shape
        l1 = [sub_len(n + CONTEXT - 1) for n in ns]
        l2 = [sub_len(v) for v in l1]
        T1, F1 = sub_len(Tp), sub_len(F)
        T2, F2 = sub_len(T1), sub_len(F1)
        y1 = ops.subsample2d_k3s2(feats, self.sub["w1"], self.sub["b1"], self._f(N, T1, F1, SUB_C), lens_in=self._lens(ns), lens_out=self._lens(l1))
        y2 = ops.subsample2d_k3s2(y1, self.sub["w2"], self.sub["b2"], self._f(N, T2, SUB_C, F2), out_cf=True, lens_in=self._lens(l1),
                                  lens_out=self._lens(l2))
        x = self._lin(y2.view(N, T2, SUB_C * F2), self.sub["out"], self._f(N, T2, self.config.encoder.d_model))
        return x, l2

    def _ffn(self, x, f, h, mid, lens_d):
        self._lin(self._ln(x, f["ln"], h, lens_d), f["up"], mid, post_act=ACT_SILU)
        self._lin(mid, f["down"], x, res=x)

    def encode_rows(self, x: torch.Tensor, rows: Sequence[int], *, return_layers: bool = False):
        """The subsampler's output [N, T, d] and the items' row counts -> the encoder's output [N, T, d] (rows beyond an item's count are
        meaningless)."""
        e = self.config.encoder
        N, T, d = x.shape
        H, dh = e.n_head, d // e.n_head
        lens_d = self._lens(rows)
        tables = self._positions(T)
        x = x.clone()
        h, mid, qkv, att = self._f(N, T, d), self._f(N, T, 4 * d), self._f(N, T, 3 * d), self._f(N, T, d)
        cv, xb = self._f(N, T, 2 * d), self._f(N, T, d)
        taps = dict(layers=[]) if return_layers else None
        for i, blk in enumerate(self.enc_layers):
            self._ffn(x, blk["ffn1"], h, mid, lens_d)
            for j, (n, wn) in enumerate((("lnq", "wq"), ("lnk", "wk"), ("lnv", "wv"))):
                self._lin(self._ln(x, blk[n], h, lens_d), blk[wn], qkv[:, :, j * d:(j + 1) * d])
            ops.relpos_attention(qkv[:, :, 0:d], qkv[:, :, d:2 * d], qkv[:, :, 2 * d:], tables[i], blk["bias_u"], blk["bias_v"], att, heads=H, dh=dh,
                                 center=T - 1, scale=dh ** -0.5, lens=lens_d)
            self._lin(att, blk["fc"], x, res=x)
            if return_layers and i == 0:
                taps["attn0"] = x.clone()
            self._lin(self._ln(x, blk["cln"], h, lens_d), blk["pw1"], mid)
            ops.glu_dwconv_ln_swish(mid, blk["dw"], blk["bn"][0], blk["bn"][1], cv, eps=LN_EPS, lens=lens_d)
            self._lin(cv, blk["pw2"], x, res=x)
            if return_layers and i == 0:
                taps["conv0"] = x.clone()
            self._ffn(x, blk["ffn2"], h, mid, lens_d)
            x, xb = self._ln(x, blk["ln"], xb, lens_d), x
            if return_layers:
                taps["layers"].append(x.clone())
        return (x, taps) if return_layers else x

    def encode(self, audios, *, return_stages: bool = False):
        """One clip (array / tensor / path) or a list of clips -> (encoder output [N, T', d], rows per item)."""
        if not isinstance(audios, (list, tuple)) or (len(audios) and isinstance(audios[0], (int, float))):
            audios = [audios]
        feats, ns = self.features(audios)
        return self.encode_features(feats, ns, return_stages=return_stages)

    def encode_features(self, feats: torch.Tensor, ns: Sequence[int], *, return_stages: bool = False):
        x, rows = self.subsample(feats, ns)
        if not return_stages:
            return self.encode_rows(x, rows), rows
        out, taps = self.encode_rows(x, rows, return_layers=True)
        return out, rows, dict(taps, sub=x)

    # ------------------------------------------------------------------ decoder
    def beam_search(self, enc: torch.Tensor, rows: Sequence[int], *, beam_size: int = 3, max_len: int = 0, softmax_smoothing: float = 1.25,
                    length_penalty: float = 0.6, eos_penalty: float = 1.0, return_trace: bool = False):
        """Lockstep beam search over a batch (fireredasr2.py:369-464 per utterance): a list of ``(tokens without <sos>, confidences)`` per utterance,
        the best beam after the GNMT length penalty; with ``return_trace`` also each step's (beam_idx, tokens, scores, done-before) on the host."""
        c, dc = self.config, self.config.decoder
        if not 1 <= beam_size <= ops.BEAM_MAX:
            raise NotImplementedError(f"FireRedASR2: beam_size {beam_size} is not built (1 .. {ops.BEAM_MAX})")
        if c.odim <= beam_size:
            raise ValueError(f"FireRedASR2: beam_size {beam_size} needs a vocabulary larger than {c.odim}")
        N, T, d = enc.shape
        B, H, dh, V = beam_size, dc.n_head, d // dc.n_head, c.odim
        rows = list(rows)
        steps = [max_len if max_len > 0 else r for r in rows]
        cap = max(steps)
        if cap + 1 > dc.pe_maxlen:
            raise ValueError(f"FireRedASR2: {cap} decoding steps exceed pe_maxlen {dc.pe_maxlen}")
        dev = self.device
        st = ops.beam_state(N, B, cap + 1, [s + 1 for s in steps], sos_id=c.sos_id, device=dev)
        lens_k = self._lens(rows)
        cross = [self._lin(enc, blk["ckv"], self._f(N, T, 2 * d)) for blk in self.dec_layers]
        caches = [torch.zeros((N * B, cap, 2 * d), dtype=torch.float32, device=dev) for _ in self.dec_layers]
        x, h, qkv, att = self._f(N * B, 1, d), self._f(N * B, 1, d), self._f(N * B, 1, 3 * d), self._f(N * B, 1, d)
        cq, mid = self._f(N, B, d), self._f(N * B, 1, 4 * d)
        logits = self._f(1, N * B, ops.round_up(V, 64))
        scale = float(d) ** 0.5
        trace = [] if return_trace else None
        neg = torch.full((N,), -1, dtype=torch.int32, device=dev)
        for t in range(cap):
            tok = st.tokens[st.cur][:, :, t].reshape(-1).long()
            x[:, 0] = self.embed[tok] * scale + self.dec_pe[t]
            pos = torch.where(st.done != 0, neg, torch.full_like(neg, t))
            ind = st.ind[st.cur]
            for blk, kv, ckv in zip(self.dec_layers, caches, cross):
                self._lin(self._ln(x, blk["ln1"], h), blk["qkv"], qkv)
                kv[:, t] = qkv[:, 0, d:]
                ops.beam_attention(qkv[:, 0, :d], kv[:, :, :d], kv[:, :, d:], ind, pos, att[:, 0], beams=B, heads=H, dh=dh, Tk=t + 1)
                self._lin(att, blk["o"], x, res=x)
                self._lin(self._ln(x, blk["ln2"], h), blk["cq"], cq.view(N * B, 1, d))
                ops.flash_attention(cq, ckv[:, :, :d], ckv[:, :, d:], att.view(N, B, d), heads=H, dh=dh, scale=dh ** -0.5, lens_k=lens_k)
                self._lin(att, blk["co"], x, res=x)
                self._lin(self._ln(x, blk["ln3"], h), blk["w1"], mid, post_act=ACT_GELU)
                self._lin(mid, blk["w2"], x, res=x)
            self._lin(self._ln(x, self.dec_norm, h).view(1, N * B, d), self.head, logits[:, :, :V])
            if return_trace:
                before = st.done.cpu().clone()
            ops.beam_step(logits[0, :, :V], st, eos_id=c.eos_id, softmax_smoothing=softmax_smoothing, eos_penalty=eos_penalty)
            if return_trace:
                trace.append(dict(done_before=before, beam_idx=st.beam_idx.cpu().clone(), tokens=st.new_tokens.cpu().clone(), scores=st.scores.cpu().clone(),
                                  logits=logits[0, :, :V].cpu().clone()))
            if (t + 1) % POLL == 0 and bool((st.done != 0).all()):
                break
        # the GNMT length penalty and the final pick, once per utterance
        tokens, conf, _ = st.final()
        tokens, conf, scores, length = tokens.cpu(), conf.cpu(), st.scores.cpu(), st.step.cpu().tolist()
        out = []
        for n in range(N):
            ys = tokens[n, :, :length[n]]
            sc = scores[n]
            if length_penalty > 0.0:
                ys_len = (ys != c.eos_id).sum(-1).to(torch.float32)
                sc = sc / torch.pow((5.0 + ys_len) / 6.0, length_penalty)
            best = int(torch.argmax(sc))
            out.append((ys[best, 1:].tolist(), conf[n, best, 1:length[n]].tolist()))
        return (out, trace) if return_trace else out

    def generate_batch(self, audios: Sequence, beam_size: int = 3, **kwargs) -> List[STTOutput]:
        """Right-padded clips decoded in lockstep; each result equals ``generate`` on that clip alone."""
        start = time.time()
        enc, rows = self.encode(list(audios))
        hyps = self.beam_search(enc, rows, beam_size=beam_size, max_len=kwargs.get("max_len", 0), softmax_smoothing=kwargs.get("softmax_smoothing", 1.25),
                                length_penalty=kwargs.get("length_penalty", 0.6), eos_penalty=kwargs.get("eos_penalty", 1.0))
        total = time.time() - start
        res = []
        for seq, conf in hyps:
            if self.config.eos_id in seq:
                seq = seq[:seq.index(self.config.eos_id)]
            text = self._detokenize(seq)
            confidence = float(np.mean(np.asarray(conf[:len(seq)], dtype=np.float32))) if seq else 0.0
            res.append(STTOutput(text=text, segments=[{"text": text, "confidence": round(confidence, 3)}], total_time=round(total, 3),
                                 generation_tokens=len(seq)))
        return res

    def generate(self, audio_or_path, beam_size: int = 3, **kwargs) -> STTOutput:
        return self.generate_batch([audio_or_path], beam_size=beam_size, **kwargs)[0]


Model = FireRedASR2
