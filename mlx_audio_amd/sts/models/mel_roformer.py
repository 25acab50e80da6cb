"""Mel-Band RoFormer vocal separation, waveform to waveform on the device (``mlx_audio/sts/models/mel_roformer``: ``config.py`` + ``model.py``).

    [B, 2, samples] -> STFT -> band split -> depth x (time transformer, frequency transformer) -> per-band mask MLP -> band merge -> iSTFT

One module file, not a package directory: ``sts/loader.get_available_models()`` lists directories and this family is, as in the reference, loaded
through ``MelRoFormer.from_pretrained``, not through the kind loader.  The exports are the reference's: ``MelRoFormer``, ``MelRoFormerConfig``,
``MelRoFormerResult``.

Host schedule.  The activations live in ONE buffer ``x [B, T, Nb, D]`` that no launch transposes:
  * ``ops.band_split`` reads the STFT as ``ops.stft_frames`` leaves it (complex64 [B * 2, T, F]) and writes ``x``;
  * every per-row op (RMSNorm, the q | k | v | gates projection, the gate, the out projection, the feed-forward) runs on the flat ``[1, B T Nb, .]``
    view; ``to_gates`` rides as ``heads`` extra output columns of the q | k | v GEMM and ``ops.head_gate`` applies it;
  * time-axis attention takes, per item, the ``[Nb, T, .]`` view (sequence stride D-rows: ``bstride = ld``, ``ld = Nb * ld``), frequency-axis
    attention the contiguous ``[B T, Nb, .]`` view; interleaved-pair RoPE is ``head_norm_rope(interleaved=True)`` on q and k in one launch;
  * the mask MLP runs one ``conv_gemm`` per band and layer on the strided band column of ``x`` (``ldx = Nb * D``), the last one writing its band's
    ``2 * bd_n`` columns of the ragged row; ``ops.band_merge`` turns that row and the input spectrum into the masked spectrum, stored frame-major as
    ``istft_frames`` reads it.
The wide linears are fp16 hi + lo MFMA passes (``precision = 4``), as for every float32 checkpoint in this package.

Not built, each raising ``NotImplementedError`` by name: checkpoint conversion (``convert_checkpoint``: ``.ckpt`` unpickling, license detection,
content addressing -- the reference's ``convert.py``), hub download (``from_pretrained`` of anything but a local directory) and chunked overlap-add
over whole songs (``separate_long``; the reference's ``__call__`` has none either: ``chunk_size`` / ``num_overlap`` are carried, not used)."""
from __future__ import annotations

import json
import math
import re
from dataclasses import dataclass, fields
from pathlib import Path
from typing import Dict, List, Optional, Union

import numpy as np
import torch

from ... import ops
from ...dsp import _ola_envelope, mel_filters

__all__ = ["MelRoFormer", "MelRoFormerConfig", "MelRoFormerResult"]

# ops.rmsnorm computes x * rsqrt(mean(x^2) + eps) * w; the reference's RMSNorm (model.py:26-42) is x / max(||x||, 1e-12) * sqrt(C) * w, which for
# ||x|| >= 1e-12 is x * rsqrt(mean(x^2)) * w.  With eps = 1e-36 (a normal float32) the two differ by a factor sqrt(1 + eps / mean(x^2)): below 1e-8
# relative for every row with mean(x^2) > 1e-28, i.e. ||x|| > 1e-14 sqrt(C) -- transformer rows are O(1) (a residual stream fed by biased
# projections), and an all-zero row gives 0 on both sides.  The band split's own norm, where digital silence does produce zero rows, is the exact
# clamp inside ops.band_split.
NORM_EPS = 1e-36


@dataclass
class MelRoFormerConfig:
    """The reference's ``MelRoFormerConfig`` (config.py): fields, derived properties and the five checkpoint-family presets.  There is no default
    preset: name the family of the checkpoint (``kim_vocal_2``, ``viperx_vocals``, ``zfturbo_bs_roformer``, ``zfturbo_vocals_v1``) or give the
    hyperparameters of a community variant to the keyword-only ``custom``."""
    dim: int = 384
    depth: int = 6
    heads: int = 8
    dim_head: int = 64
    num_bands: int = 60
    num_stems: int = 1
    ff_mult: int = 4
    mlp_expansion_factor: int = 4
    mask_estimator_depth: int = 2
    n_fft: int = 2048
    hop_length: int = 441
    win_length: int = 2048
    sample_rate: int = 44100
    chunk_size: int = 352800
    num_overlap: int = 2
    checkpoint_family: Optional[str] = None

    @property
    def dim_inner(self) -> int:
        return self.heads * self.dim_head

    @property
    def ff_dim(self) -> int:
        return self.dim * self.ff_mult

    @property
    def mlp_hidden(self) -> int:
        return self.dim * self.mlp_expansion_factor

    @property
    def freq_bins(self) -> int:
        return self.n_fft // 2 + 1

    @classmethod
    def kim_vocal_2(cls) -> "MelRoFormerConfig":
        return cls(depth=6, checkpoint_family="kim_vocal_2")

    @classmethod
    def viperx_vocals(cls) -> "MelRoFormerConfig":
        return cls(depth=12, checkpoint_family="viperx_vocals")

    @classmethod
    def zfturbo_bs_roformer(cls) -> "MelRoFormerConfig":
        return cls(depth=12, checkpoint_family="zfturbo_bs_roformer")

    @classmethod
    def zfturbo_vocals_v1(cls) -> "MelRoFormerConfig":
        return cls(dim=192, depth=8, hop_length=512, mask_estimator_depth=1, checkpoint_family="zfturbo_vocals_v1")

    @classmethod
    def custom(cls, *, depth: int, num_bands: int = 60, dim: int = 384, heads: int = 8, dim_head: int = 64, n_fft: int = 2048, hop_length: int = 441,
               sample_rate: int = 44100, **kwargs) -> "MelRoFormerConfig":
        return cls(depth=depth, num_bands=num_bands, dim=dim, heads=heads, dim_head=dim_head, n_fft=n_fft, hop_length=hop_length,
                   sample_rate=sample_rate, checkpoint_family="custom", **kwargs)


@dataclass
class MelRoFormerResult:
    """``MelRoFormerResult`` of the reference: one separated stem and its timing."""
    vocals: torch.Tensor
    sample_rate: int
    duration_seconds: float
    processing_time_seconds: float


# ------------------------------------------------------------------------------------------------ band tables
def mel_band_indices(config: MelRoFormerConfig) -> List[np.ndarray]:
    """``MelFilterbank`` (model.py:63-140): the Slaney filterbank of ``dsp.mel_filters``, DC forced into band 0 and Nyquist into the last band,
    binarised; band i's CaC indices are (2 bin, 2 bin + 1) for each of its bins in ascending order; an empty band falls back to bin i."""
    fb = mel_filters(sample_rate=config.sample_rate, n_fft=config.n_fft, n_mels=config.num_bands, mel_scale="slaney").numpy().astype(np.float32)
    fb[0, 0] = 1.0
    fb[-1, -1] = 1.0
    out = []
    for i in range(config.num_bands):
        bins = np.where(fb[i] > 0)[0]
        if len(bins) == 0:
            bins = np.array([i])
        out.append(np.stack([2 * bins, 2 * bins + 1], axis=1).reshape(-1).astype(np.int32))
    return out


def band_dims(config: MelRoFormerConfig) -> List[int]:
    return [2 * len(ix) for ix in mel_band_indices(config)]


# ------------------------------------------------------------------------------------------------ checkpoints
def expected_shapes(config: MelRoFormerConfig) -> Dict[str, tuple]:
    """Every parameter under the names the reference's module tree gives it (what ``sanitize`` produces), in a fixed order."""
    c, s = config, {}
    for n, bd in enumerate(band_dims(c)):
        s[f"band_split.to_features.{n}.0.weight"] = (bd,)
        s[f"band_split.to_features.{n}.1.weight"] = (c.dim, bd)
        s[f"band_split.to_features.{n}.1.bias"] = (c.dim,)
    for lv in range(c.depth):
        for ax in range(2):
            p = f"layers.{lv}.{ax}."
            a, f = p + "layers.0.0.", p + "layers.0.1.net."
            s[a + "norm.weight"] = (c.dim,)
            for nm in ("to_q", "to_k", "to_v"):
                s[a + nm + ".weight"] = (c.dim_inner, c.dim)
            s[a + "to_gates.weight"] = (c.heads, c.dim)
            s[a + "to_gates.bias"] = (c.heads,)
            s[a + "to_out.weight"] = (c.dim, c.dim_inner)
            s[f + "0.weight"] = (c.dim,)
            s[f + "1.weight"] = (c.ff_dim, c.dim)
            s[f + "1.bias"] = (c.ff_dim,)
            s[f + "4.weight"] = (c.dim, c.ff_dim)
            s[f + "4.bias"] = (c.dim,)
            s[p + "norm.weight"] = (c.dim,)
    for n, bd in enumerate(band_dims(c)):
        widths = [c.dim] + [c.mlp_hidden] * c.mask_estimator_depth + [2 * bd]
        for i in range(c.mask_estimator_depth + 1):
            s[f"mask_estimators.0.to_freqs.{n}.{i}.0.weight"] = (widths[i + 1], widths[i])
            s[f"mask_estimators.0.to_freqs.{n}.{i}.0.bias"] = (widths[i + 1],)
    return s


def make_melroformer_weights(config: MelRoFormerConfig, seed: int = 0, torch_names: bool = False) -> Dict[str, torch.Tensor]:
    """A seeded checkpoint: matrices uniform in +-sqrt(3 / fan_in), biases 0.1 N(0, 1), RMSNorm scales 1 + 0.1 N(0, 1); float32 tensors holding
    fp16-representable values, like a checkpoint published in fp16 (the engine packs fp16 weight images).  ``torch_names``: the same tensors under
    the names of a PyTorch checkpoint -- packed ``to_qkv``, ``.gamma``, ``to_out.0``, ``nn.Sequential`` indices 0, 2, 4 in the mask MLPs and a
    ``rotary_embed.freqs`` buffer per attention -- which ``MelRoFormer.sanitize`` turns back into the first form."""
    g = torch.Generator().manual_seed(seed)
    w: Dict[str, torch.Tensor] = {}
    for name, shape in expected_shapes(config).items():
        if name.endswith(".bias"):
            t = 0.1 * torch.randn(shape, generator=g)
        elif len(shape) == 1:
            t = 1.0 + 0.1 * torch.randn(shape, generator=g)
        else:
            t = (torch.rand(shape, generator=g) * 2 - 1) * math.sqrt(3.0 / shape[1])
        w[name] = t.to(torch.float16).to(torch.float32)
    if not torch_names:
        return w
    out: Dict[str, torch.Tensor] = {}
    for name, t in w.items():
        m = re.match(r"^(mask_estimators\.\d+\.to_freqs\.\d+)\.(\d+)\.0\.(weight|bias)$", name)
        if name.endswith("to_q.weight"):
            p = name[:-len("to_q.weight")]
            out[p + "to_qkv.weight"] = torch.cat([t, w[p + "to_k.weight"], w[p + "to_v.weight"]])
            out[p + "rotary_embed.freqs"] = torch.zeros(config.dim_head // 2)
        elif name.endswith(("to_k.weight", "to_v.weight")):
            continue
        elif m:
            out[f"{m.group(1)}.0.{2 * int(m.group(2))}.{m.group(3)}"] = t
        elif name.endswith("to_out.weight"):
            out[name[:-len("weight")] + "0.weight"] = t
        elif len(t.shape) == 1 and name.endswith(".weight") and not name.endswith("to_gates.weight"):
            out[name[:-len("weight")] + "gamma"] = t
        else:
            out[name] = t
    return out


_MASK_MLP_RE = re.compile(r"^(mask_estimators\.\d+\.to_freqs\.\d+)\.0\.(\d+)\.(weight|bias)$")


def sanitize(weights: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """``MelRoFormer.sanitize`` (model.py:648-698), per key: packed ``to_qkv`` -> ``to_q`` / ``to_k`` / ``to_v`` (thirds of axis 0);
    ``rotary_embed.freqs`` dropped; the mask MLPs' ``nn.Sequential`` positions 0, 2, 4 -> list positions 0, 1, 2; ``to_out.0.weight`` ->
    ``to_out.weight``; a trailing ``.gamma`` -> ``.weight``."""
    out = {}
    for key, value in weights.items():
        if "to_qkv.weight" in key:
            prefix, third = key.replace("to_qkv.weight", ""), value.shape[0] // 3
            out[prefix + "to_q.weight"], out[prefix + "to_k.weight"], out[prefix + "to_v.weight"] = value[:third], value[third:2 * third], value[2 * third:]
            continue
        if key.endswith("rotary_embed.freqs"):
            continue
        m = _MASK_MLP_RE.match(key)
        if m:
            key = f"{m.group(1)}.{int(m.group(2)) // 2}.0.{m.group(3)}"
        if key.endswith("to_out.0.weight"):
            key = key[:-len(".0.weight")] + ".weight"
        if key.endswith(".gamma"):
            key = key[:-len(".gamma")] + ".weight"
        out[key] = value
    return out


def convert_checkpoint(*args, **kwargs):
    raise NotImplementedError("mel_roformer.convert_checkpoint is not built: the reference's convert.py (.ckpt unpickling, license detection, "
                              "content-addressed output names) is missing; convert with the reference and load the .safetensors it writes")


_PRIORITY = ("mel_roformer_vocals.safetensors", "weights.safetensors", "model.safetensors")


@dataclass
class _Transformer:
    attn_norm: torch.Tensor
    qkvg: ops.PackedConv
    out: ops.PackedConv
    ff_norm: torch.Tensor
    ff1: ops.PackedConv
    ff2: ops.PackedConv
    norm: torch.Tensor


class MelRoFormer:
    """``MelRoFormer`` of the reference as an engine.  ``weights``: a checkpoint under the reference's parameter names or a PyTorch checkpoint's
    (``sanitize`` is applied either way); None: a seeded one (``make_melroformer_weights(config, seed)``)."""

    def __init__(self, config: MelRoFormerConfig, weights: Optional[Dict[str, torch.Tensor]] = None, device="cuda:0", seed: int = 0, strict: bool = True):
        c = config
        if c.dim_head not in (64, 128):
            raise NotImplementedError(f"MelRoFormer: dim_head {c.dim_head} is not built (head_norm_rope / flash_attention take 64 or 128)")
        if c.num_stems != 1:
            raise NotImplementedError(f"MelRoFormer: num_stems {c.num_stems} is not built (the reference runs mask_estimators[0] only)")
        if c.win_length != c.n_fft:
            raise ValueError(f"MelRoFormer: win_length {c.win_length} must equal n_fft {c.n_fft} (the reference windows whole frames)")
        self.config = config
        self.device = torch.device(device)
        ops.require_gpu()
        self.band_indices = mel_band_indices(c)
        self.tables = ops.band_tables(self.band_indices, c.freq_bins, self.device)
        if max(self.tables.band_dims) > ops.BAND_MAX_DIM:
            raise NotImplementedError(f"MelRoFormer: a band of {max(self.tables.band_dims)} entries; band_split takes at most {ops.BAND_MAX_DIM}")
        self._window = np.hanning(c.n_fft + 1)[:-1].astype(np.float32)            # model.py:585
        self._window_d = torch.from_numpy(self._window).to(self.device)
        half = c.dim_head // 2
        self._rope_freqs = (1.0 / (10000.0 ** (np.arange(0, half, dtype=np.float32) / half))).astype(np.float32)   # model.py:165-168
        self._rope = (None, None, 0)
        self.load_weights(make_melroformer_weights(c, seed) if weights is None else weights, strict=strict)

    # ------------------------------------------------------------------ checkpoint handling
    sanitize = staticmethod(sanitize)

    def load_weights(self, weights, strict: bool = True):
        """``weights``: a dict or a list of (name, tensor) pairs; ``sanitize`` is applied first.  A missing or wrongly shaped parameter is refused, an
        unknown one too unless ``strict=False`` (the reference loads with ``strict=False``)."""
        c, dev = self.config, self.device
        w = {k: torch.as_tensor(np.asarray(v) if not isinstance(v, torch.Tensor) else v).detach().to(torch.float32).cpu() for k, v in sanitize(dict(weights)).items()}
        shapes = expected_shapes(c)
        miss = [k for k in shapes if k not in w]
        if miss:
            raise ValueError(f"MelRoFormer.load_weights: missing parameters {miss[:4]}{' ...' if len(miss) > 4 else ''}")
        extra = [k for k in w if k not in shapes]
        if extra and strict:
            raise ValueError(f"MelRoFormer.load_weights: unexpected parameters {extra[:4]}{' ...' if len(extra) > 4 else ''}")
        for k, s in shapes.items():
            if tuple(w[k].shape) != s:
                raise ValueError(f"MelRoFormer.load_weights: {k} has shape {tuple(w[k].shape)}, expected {s}")

        def lin(wt, bias=None):
            return ops.pack_conv(wt, bias, dev, f16=True)

        def vec(name):
            return w[name].contiguous().to(dev)

        Nb = c.num_bands
        bs = "band_split.to_features."
        self.split_wt, self.split_gamma, self.split_bias = ops.pack_band_split([w[f"{bs}{n}.1.weight"] for n in range(Nb)], [w[f"{bs}{n}.0.weight"] for n in range(Nb)],
                                                                               [w[f"{bs}{n}.1.bias"] for n in range(Nb)], dev)
        self.layers = []
        for lv in range(c.depth):
            pair = []
            for ax in range(2):
                p = f"layers.{lv}.{ax}."
                a, f = p + "layers.0.0.", p + "layers.0.1.net."
                qkvg = torch.cat([w[a + "to_q.weight"], w[a + "to_k.weight"], w[a + "to_v.weight"], w[a + "to_gates.weight"]])
                qkvg_b = torch.cat([torch.zeros(3 * c.dim_inner), w[a + "to_gates.bias"]])
                pair.append(_Transformer(vec(a + "norm.weight"), lin(qkvg, qkvg_b), lin(w[a + "to_out.weight"]), vec(f + "0.weight"),
                                         lin(w[f + "1.weight"], w[f + "1.bias"]), lin(w[f + "4.weight"], w[f + "4.bias"]), vec(p + "norm.weight")))
            self.layers.append(pair)
        me = "mask_estimators.0.to_freqs."
        self.mask_estimators = [[[lin(w[f"{me}{n}.{i}.0.weight"], w[f"{me}{n}.{i}.0.bias"]) for i in range(c.mask_estimator_depth + 1)] for n in range(Nb)]]
        return self

    def eval(self):
        return self

    @classmethod
    def from_pretrained(cls, model_path: Union[str, Path], config: Optional[MelRoFormerConfig] = None, *, device="cuda:0") -> "MelRoFormer":
        """model.py:700-787 for a LOCAL directory.  Weights: the first of ``mel_roformer_vocals.safetensors``, ``weights.safetensors``,
        ``model.safetensors`` that exists, else the first ``*.safetensors`` in name order.  Config: the argument, else ``<weights>.config.json``
        beside the weights file, else ``config.json`` in the directory (unknown keys dropped), else ``ValueError``: no default is assumed."""
        path = Path(str(model_path)).expanduser()
        if not path.is_dir():
            raise NotImplementedError(f"MelRoFormer.from_pretrained: hub download is not built; {model_path!r} is not a local directory")
        found = sorted(path.glob("*.safetensors"))
        if not found:
            raise FileNotFoundError(f"No .safetensors file found in {path}")
        weight_file = next((path / n for n in _PRIORITY if (path / n).exists()), found[0])
        if config is None:
            companion, plain = weight_file.with_suffix(".config.json"), path / "config.json"
            src = companion if companion.exists() else (plain if plain.exists() else None)
            if src is None:
                raise ValueError(f"No config provided and no companion config.json found at {companion} or {plain}. Pass an explicit preset, e.g. "
                                 "`MelRoFormer.from_pretrained(path, config=MelRoFormerConfig.kim_vocal_2())`.")
            valid = {f.name for f in fields(MelRoFormerConfig)}
            config = MelRoFormerConfig(**{k: v for k, v in json.loads(src.read_text()).items() if k in valid})
        from safetensors.torch import load_file

        return cls(config, weights=load_file(str(weight_file)), device=device, strict=False)   # strict=False: model.py:786

    # ------------------------------------------------------------------ forward
    def n_frames(self, n_samples: int) -> int:
        return 1 + n_samples // self.config.hop_length

    def _rope_tables(self, n: int):
        cos, sin, rows = self._rope
        if rows < n:
            ang = np.arange(n, dtype=np.float32)[:, None] * self._rope_freqs[None, :]   # float32 products (model.py:177-180)
            cos, sin = torch.from_numpy(np.cos(ang).astype(np.float32)).to(self.device), torch.from_numpy(np.sin(ang).astype(np.float32)).to(self.device)
            self._rope = (cos, sin, n)
        return cos, sin

    def _f(self, *shape):
        return torch.empty(shape, dtype=torch.float32, device=self.device)

    def _transformer(self, p: _Transformer, x: torch.Tensor, bufs, time_axis: bool):
        c = self.config
        B, T, Nb, D = x.shape
        H, dh, inner = c.heads, c.dim_head, c.dim_inner
        h, qkv, att, mid = bufs
        xf = x.view(1, B * T * Nb, D)
        ldq = qkv.shape[2]
        ops.rmsnorm(xf, h, p.attn_norm, eps=NORM_EPS)
        ops.conv_gemm(h, p.qkvg, qkv, precision=4)
        cos, sin = self._rope_tables(max(T, Nb))
        if time_axis:   # per item: the bands are the batch, the frames the sequence
            views = [(qkv.view(B, T, Nb, ldq)[b].permute(1, 0, 2), att.view(B, T, Nb, inner)[b].permute(1, 0, 2)) for b in range(B)]
        else:
            views = [(qkv.view(B * T, Nb, ldq), att.view(B * T, Nb, inner))]
        for s, o in views:
            q, k, v = s[:, :, :inner], s[:, :, inner:2 * inner], s[:, :, 2 * inner:3 * inner]
            ops.head_norm_rope(q, q, heads=H, dh=dh, cos=cos, sin=sin, interleaved=True, second=(k, k, H, None))
            ops.flash_attention(q, k, v, o, heads=H, dh=dh, scale=1.0 / math.sqrt(dh))
        ops.head_gate(att, qkv[:, :, 3 * inner:3 * inner + H], heads=H, dh=dh)
        ops.conv_gemm(att, p.out, xf, res=xf, precision=4)
        ops.rmsnorm(xf, h, p.ff_norm, eps=NORM_EPS)
        ops.conv_gemm(h, p.ff1, mid, post_act=ops.ACT_GELU, precision=4)
        ops.conv_gemm(mid, p.ff2, xf, res=xf, precision=4)
        ops.rmsnorm(xf, xf, p.norm, eps=NORM_EPS)

    def _run(self, audio, return_stages: bool = False):
        c = self.config
        a = torch.as_tensor(np.asarray(audio) if not isinstance(audio, torch.Tensor) else audio).detach().to(torch.float32)
        if a.dim() != 3 or a.shape[1] != 2:
            raise ValueError(f"MelRoFormer: audio must be [B, 2, samples] stereo, got {tuple(a.shape)}")
        B, _, S = a.shape
        if S <= c.n_fft // 2:
            raise ValueError(f"Input is too short (length={S + 2 * (c.n_fft // 2)}) for n_fft={c.n_fft} with hop_length={c.hop_length} and center=True.")
        T, Nb, D, tab = self.n_frames(S), c.num_bands, c.dim, self.tables
        inner, ldq = c.dim_inner, ops.round_up(3 * c.dim_inner + c.heads, 4)
        spec = ops.stft_frames(a.reshape(B * 2, S).contiguous().to(self.device), c.n_fft, c.hop_length, self._window_d, 1, T)   # complex64 [B * 2, T, F]
        x = ops.band_split(spec, tab, self.split_wt, self.split_gamma, self.split_bias)
        stages = dict(split=x.clone(), tf=[]) if return_stages else None
        R = B * T * Nb
        bufs = (self._f(1, R, D), self._f(1, R, ldq), self._f(1, R, inner), self._f(1, R, c.ff_dim))
        for lv, (time_tf, freq_tf) in enumerate(self.layers):
            self._transformer(time_tf, x, bufs, True)
            if return_stages and lv == 0:
                stages["tf"].append(x.clone())
            self._transformer(freq_tf, x, bufs, False)
            if return_stages and lv == 0:
                stages["tf"].append(x.clone())
        del bufs
        # mask MLP: one launch per band and layer on the band's strided column of x; the last layer fills the band's columns of the ragged row
        xb = x.view(1, B * T, Nb * D)
        hid = [self._f(1, B * T, c.mlp_hidden) for _ in range(min(2, c.mask_estimator_depth))]
        rag = self._f(B, T, tab.h_cols)
        ragf = rag.view(1, B * T, tab.h_cols)
        for n, mlp in enumerate(self.mask_estimators[0]):
            cur = xb[:, :, n * D:(n + 1) * D]
            for i, pc in enumerate(mlp[:-1]):
                cur = ops.conv_gemm(cur, pc, hid[i % 2], post_act=ops.ACT_TANH, precision=4)
            ops.conv_gemm(cur, mlp[-1], ragf[:, :, 4 * int(tab.band_ptr[n]):4 * int(tab.band_ptr[n + 1])], precision=4)
        masked = self._f(B * 2, T, c.freq_bins, 2)                                  # frame-major, as istft_frames reads it
        ops.band_merge(rag, tab, spec, out=masked.permute(0, 2, 1, 3))
        if return_stages:
            ones = torch.zeros((B * 2, T, c.freq_bins, 2), dtype=torch.float32, device=self.device)
            ones[..., 0] = 1.0
            m = ops.band_merge(rag, tab, ones)                                      # spectrum 1 + 0j: the merged mask itself, [B * 2, F, T]
            stages["mask"] = torch.view_as_real(m.reshape(B, 2, c.freq_bins, T).permute(0, 2, 1, 3).reshape(B, 2 * c.freq_bins, T).contiguous())
            stages["spec"], stages["masked"] = spec, torch.view_as_complex(masked)
        # dsp.istft(center=True, length=None, normalized=True) (model.py:507-523): window^2 envelope, n_fft / 2 stripped from both ends
        total, trim = (T - 1) * c.hop_length + c.n_fft, c.n_fft // 2
        env = torch.from_numpy(_ola_envelope(self._window.tobytes(), c.n_fft, T, c.hop_length, True)).to(self.device)
        y = ops.istft_frames(torch.view_as_complex(masked), c.n_fft, c.hop_length, self._window_d, env, 1, False, trim, total - 2 * trim)
        out = torch.zeros((B * 2, S), dtype=torch.float32, device=y.device)       # pad with zeros or trim to the input length (model.py:530-534)
        n = min(S, y.shape[1])
        out[:, :n] = y[:, :n]
        out = out.view(B, 2, S)
        return (out, stages) if return_stages else out

    def __call__(self, audio, *, return_stages: bool = False):
        """``audio`` [B, 2, samples] stereo at ``config.sample_rate`` -> the vocal stem [B, 2, samples] (float32, on the device)."""
        return self._run(audio, return_stages)

    def separate_long(self, *args, **kwargs):
        raise NotImplementedError("MelRoFormer.separate_long is not built: chunked overlap-add over whole songs (config.chunk_size / num_overlap) is "
                                  "missing, as in the reference's __call__; call the model on chunks of at most a few seconds")
