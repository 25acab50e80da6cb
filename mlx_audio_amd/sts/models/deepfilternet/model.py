"""DeepFilterNet2 / DeepFilterNet3 speech enhancement, waveform to waveform on the device (``mlx_audio/sts/models/deepfilternet/model.py``).

The reference's framing is kept: one hop of zeros in front (libDF's analysis memory), ``fft_size`` zeros behind, a Vorbis window, ``center=False``,
``wnorm`` on the way in and out, an inverse STFT with ``normalized=True``, delay compensation ``fft_size - hop_size`` and a clip to [-1, 1].
``enhance_batch`` is new here: one right-padded batch with lengths through every kernel; each item equals that item run alone.

Not built, each raising ``NotImplementedError``: the streaming runtime (``create_streamer``, ``enhance_array_streaming``,
``enhance_file_streaming``; the reference's ``streaming.py``) and DeepFilterNet 1 (``model_version == "DeepFilterNet"``, ``network_df1.py``).
``from_pretrained`` reads a local directory only."""
from __future__ import annotations

import json
import math
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Union

import numpy as np
import torch

from .... import audio_io, ops
from ....dsp import _ola_envelope
from .config import DeepFilterNet2Config, DeepFilterNet3Config, DeepFilterNetConfig
from .network import DfNet, check_config, expected_shapes

DEFAULT_SUBFOLDER = "v3"
VERSION_SUBFOLDER = {1: "v1", 2: "v2", 3: "v3"}
DEFAULT_CONFIGS = {"DeepFilterNet": DeepFilterNetConfig, "DeepFilterNet2": DeepFilterNet2Config, "DeepFilterNet3": DeepFilterNet3Config}


def default_erb_widths(freq_bins: int, nb_erb: int, min_width: int = 2) -> List[int]:
    """A deterministic ERB-like partition of ``freq_bins`` into ``nb_erb`` bands of at least ``min_width`` bins that widen with frequency (for seeded
    checkpoints; published ones carry their own filterbanks)."""
    if freq_bins < min_width * nb_erb:
        raise ValueError(f"{freq_bins} bins cannot hold {nb_erb} bands of {min_width}")
    spare = freq_bins - min_width * nb_erb
    wt = np.arange(nb_erb, dtype=np.float64) ** 2
    extra = np.floor(spare * wt / max(wt.sum(), 1.0)).astype(np.int64)
    extra[-1] += spare - int(extra.sum())
    return [int(min_width + e) for e in extra]


def erb_filterbanks(widths: Sequence[int], freq_bins: int):
    """(erb_fb [F, E] with 1 / width inside a band, erb_inv_fb [E, F] with 1 inside a band): libDF's normalised filterbank and its inverse."""
    if sum(widths) != freq_bins:
        raise ValueError(f"erb_widths sum to {sum(widths)}, not to the {freq_bins} frequency bins")
    fb, inv = torch.zeros(freq_bins, len(widths)), torch.zeros(len(widths), freq_bins)
    start = 0
    for e, wd in enumerate(widths):
        fb[start:start + wd, e] = 1.0 / wd
        inv[e, start:start + wd] = 1.0
        start += wd
    return fb, inv


def make_dfn_weights(config: DeepFilterNetConfig, seed: int = 0, fp16: bool = True) -> Dict[str, torch.Tensor]:
    """A seeded checkpoint under the PyTorch names the reference's loader accepts: conv / linear / GRU matrices uniform in +-1 / sqrt(fan_in), biases
    0.1 N(0, 1), BatchNorm weights 1 + 0.1 N(0, 1), running mean 0.1 N(0, 1) and running variance in [0.5, 1.5], the two filterbanks built from
    ``erb_widths`` (``default_erb_widths`` when the config has none).  float32 tensors holding fp16-representable values (``fp16=False``: unrounded)."""
    g = torch.Generator().manual_seed(seed)
    widths = config.erb_widths or default_erb_widths(config.freq_bins, config.nb_erb)
    fb, inv = erb_filterbanks(widths, config.freq_bins)
    w: Dict[str, torch.Tensor] = {}
    for name, shape in expected_shapes(config).items():
        if name == "erb_fb":
            t = fb
        elif name == "mask.erb_inv_fb":
            t = inv
        elif name.endswith("running_var"):
            t = 0.5 + torch.rand(shape, generator=g)
        elif name.endswith("running_mean"):
            t = 0.1 * torch.randn(shape, generator=g)
        elif name.endswith(".bias") or ".bias_" in name:
            t = 0.1 * torch.randn(shape, generator=g)
        elif len(shape) == 1:                                  # BatchNorm weight
            t = 1.0 + 0.1 * torch.randn(shape, generator=g)
        else:
            if len(shape) == 3:                                # grouped linear [G, ws, hs]
                fan_in = shape[1]
            elif len(shape) == 4:
                fan_in = shape[1] * shape[2] * shape[3]
            else:
                fan_in = shape[1]
            t = (torch.rand(shape, generator=g) * 2 - 1) * math.sqrt(3.0 / fan_in)
        w[name] = t.to(torch.float16).to(torch.float32) if fp16 else t.to(torch.float32)
    return w


def _not_built(what: str):
    raise NotImplementedError(f"DeepFilterNet {what} is not built: the streaming runtime of the reference (streaming.py: per-hop analysis memory, rolling "
                              "feature and GRU states) is missing; use enhance_array / enhance_batch / enhance_file on whole clips")


class DeepFilterNetModel:
    """``DeepFilterNetModel`` of the reference as an engine.  ``weights``: a checkpoint under the PyTorch names (``expected_shapes``); None: a seeded
    one (``make_dfn_weights(config, seed)``)."""

    def __init__(self, config: DeepFilterNetConfig, weights: Optional[Dict[str, torch.Tensor]] = None, device="cuda:0", seed: int = 0,
                 model_dir: Optional[Path] = None):
        check_config(config)
        self.config = config
        self.device = torch.device(device)
        self.model_dir = Path(model_dir) if model_dir is not None else None
        self.model_version = config.model_version
        self.wnorm = 1.0 / (config.fft_size * config.fft_size / (2.0 * config.hop_size))   # libDF
        self._vorbis = self._vorbis_window(config.fft_size)
        self._window_d = torch.from_numpy(self._vorbis).to(self.device)
        self.load_weights(make_dfn_weights(config, seed) if weights is None else weights)

    # ------------------------------------------------------------------ checkpoint handling
    def load_weights(self, weights, strict: bool = True):
        """``weights``: a dict or a list of (name, tensor) pairs.  ``num_batches_tracked`` and ``.h0`` entries are ignored like the reference's loader
        does; every other unknown name is refused (``strict=False``: dropped), as is a missing or wrongly shaped one.  ``erb_fb`` may be absent when
        the config carries ``erb_widths`` (band means then replace the filterbank product)."""
        cfg = self.config
        w = {k: torch.as_tensor(np.asarray(v) if not isinstance(v, torch.Tensor) else v).detach().to(torch.float32).cpu()
             for k, v in dict(weights).items() if "num_batches_tracked" not in k and not k.endswith(".h0")}
        has_fb = "erb_fb" in w
        if not has_fb and cfg.erb_widths is None:
            raise ValueError("DeepFilterNet.load_weights: missing both the ERB filterbank (erb_fb) and the config's erb_widths")
        shapes = expected_shapes(cfg, with_erb_fb=has_fb)
        miss = [k for k in shapes if k not in w]
        if miss:
            raise ValueError(f"DeepFilterNet.load_weights: missing parameters {miss[:4]}{' ...' if len(miss) > 4 else ''}")
        extra = [k for k in w if k not in shapes]
        if extra and strict:
            raise ValueError(f"DeepFilterNet.load_weights: unexpected parameters {extra[:4]}{' ...' if len(extra) > 4 else ''}")
        for k, s in shapes.items():
            if tuple(w[k].shape) != s:
                raise ValueError(f"DeepFilterNet.load_weights: {k} has shape {tuple(w[k].shape)}, expected {s}")
        self.model = DfNet(cfg, {k: w[k] for k in shapes}, self.device)
        self.erb_fb = w["erb_fb"].contiguous().to(self.device) if has_fb else None
        self.erb_start = None
        if not has_fb:
            if sum(cfg.erb_widths) != cfg.freq_bins or len(cfg.erb_widths) != cfg.nb_erb:
                raise ValueError(f"DeepFilterNet: erb_widths must hold {cfg.nb_erb} widths that sum to {cfg.freq_bins}")
            self.erb_start = torch.tensor(np.concatenate([[0], np.cumsum(cfg.erb_widths)]), dtype=torch.int32, device=self.device)
        return self

    def eval(self):
        return self

    def post_load_hook(self, model_path) -> "DeepFilterNetModel":
        self.model_dir = Path(model_path)
        return self

    @classmethod
    def from_pretrained(cls, model_name_or_path: str, subfolder: Optional[str] = DEFAULT_SUBFOLDER, version: Optional[int] = None, *,
                        device="cuda:0") -> "DeepFilterNetModel":
        """A LOCAL directory (or its ``subfolder``) holding ``config.json`` and ``model.safetensors``; ``version`` 1, 2 or 3 selects ``v1`` / ``v2`` / ``v3``."""
        if version is not None:
            subfolder = VERSION_SUBFOLDER.get(version)
            if subfolder is None:
                raise ValueError(f"Unsupported version={version}. Choose from 1, 2, or 3.")
        local = Path(model_name_or_path).expanduser().resolve()
        if not local.exists():
            raise FileNotFoundError(f"{model_name_or_path}: DeepFilterNetModel.from_pretrained needs a local directory (no hub access in this build)")
        if not local.is_dir():
            raise ValueError(f"Local model path must be a directory containing config.json and model.safetensors: {local}")
        model_dir = local / subfolder if subfolder else local
        config_path, weights_path = model_dir / "config.json", model_dir / "model.safetensors"
        if not config_path.exists():
            raise FileNotFoundError(f"Missing config.json in model directory: {model_dir}")
        if not weights_path.exists():
            raise FileNotFoundError(f"Missing model.safetensors in: {model_dir}")
        from safetensors.torch import load_file

        with open(config_path, encoding="utf-8") as f:
            config_dict = json.load(f)
        version_name = config_dict.get("model_version") or "DeepFilterNet3"
        config = DEFAULT_CONFIGS.get(version_name, DeepFilterNetConfig).from_dict(config_dict)
        return cls(config, weights=load_file(str(weights_path)), device=device, model_dir=model_dir)

    # ------------------------------------------------------------------ host constants
    @staticmethod
    def _vorbis_window(size: int) -> np.ndarray:
        """libDF's Vorbis window sin(pi/2 sin^2(pi (n + 0.5) / N)), float32 like the reference computes it."""
        n = np.arange(size, dtype=np.float32)
        inner = np.sin(0.5 * np.pi * (n + 0.5) / (size // 2))
        return np.sin(0.5 * np.pi * inner * inner).astype(np.float32)

    def _norm_alpha(self) -> float:
        """df.utils.get_norm_alpha: exp(-hop / sr) rounded to the fewest decimals (from 3) that stay below 1."""
        a_raw = math.exp(-self.config.hop_size / self.config.sample_rate)
        precision, a = 3, 1.0
        while a >= 1.0:
            a = round(a_raw, precision)
            precision += 1
        return a

    # ------------------------------------------------------------------ forward
    def n_frames(self, n_samples: int) -> int:
        return 1 + (n_samples + self.config.hop_size) // self.config.hop_size

    def _run(self, clips: List[np.ndarray], return_stages: bool = False):
        p = self.config
        lens_s = [int(c.shape[0]) for c in clips]
        frames = [self.n_frames(n) for n in lens_s]
        B, T, Lp = len(clips), max(frames), max(lens_s) + p.hop_size + p.fft_size
        x = torch.zeros((B, Lp), dtype=torch.float32)
        for b, c in enumerate(clips):
            x[b, p.hop_size:p.hop_size + lens_s[b]] = torch.from_numpy(c)
        lens_d = torch.tensor(frames, dtype=torch.int32, device=self.device) if B > 1 else None
        spec = torch.view_as_real(ops.stft_frames(x.to(self.device), p.fft_size, p.hop_size, self._window_d, 0, T))
        alpha = self._norm_alpha()
        spec, feat_erb, feat_df = ops.dfn_features(spec, wnorm=self.wnorm, alpha=float(np.float32(alpha)), one_minus_alpha=float(np.float32(1.0 - alpha)),
                                                   nb_erb=p.nb_erb, nb_df=p.nb_df, lookahead=p.conv_lookahead, erb_fb=self.erb_fb, erb_start=self.erb_start,
                                                   lens=lens_d)
        res = self.model(spec, feat_erb, feat_df, lens_d, wnorm=self.wnorm, return_stages=return_stages)
        out, stages = res if return_stages else (res, None)
        spec_e = out[0]
        d = p.fft_size - p.hop_size
        if p.fft_size <= 2 * p.hop_size or len(set(frames)) == 1:
            # frames at and beyond an item's own count start behind every sample it keeps, so the batch's overlap-add envelope is the item's own there
            env = torch.from_numpy(_ola_envelope(self._vorbis.tobytes(), p.fft_size, T, p.hop_size, True)).to(self.device)
            y = ops.istft_frames(spec_e, p.fft_size, p.hop_size, self._window_d, env, 1, False, 0, (T - 1) * p.hop_size + p.fft_size)
            ys = [y[b, d:d + lens_s[b]] for b in range(B)]
        else:
            ys = []
            for b in range(B):
                env = torch.from_numpy(_ola_envelope(self._vorbis.tobytes(), p.fft_size, frames[b], p.hop_size, True)).to(self.device)
                y = ops.istft_frames(spec_e[b:b + 1, :frames[b]], p.fft_size, p.hop_size, self._window_d, env, 1, False, 0, (frames[b] - 1) * p.hop_size + p.fft_size)
                ys.append(y[0, d:d + lens_s[b]])
        outs = [np.clip(y.detach().cpu().numpy().astype(np.float32), -1.0, 1.0) for y in ys]
        if return_stages:
            stages.update(feat_erb=feat_erb, feat_df=feat_df, spec=spec, spec_e=spec_e, frames=frames)
            return outs, stages
        return outs

    @staticmethod
    def _clip_of(audio) -> np.ndarray:
        x = np.asarray(audio.detach().cpu() if isinstance(audio, torch.Tensor) else audio, dtype=np.float32)
        if x.ndim != 1:
            raise ValueError(f"DeepFilterNet: a clip is a 1-D array of samples, got shape {x.shape}")
        return np.ascontiguousarray(x)

    def enhance_array(self, audio, *, return_stages: bool = False):
        """float samples at ``config.sample_rate`` [L] -> the enhanced clip, float32 [L] in [-1, 1]."""
        x = self._clip_of(audio)
        if x.shape[0] == 0:
            return x
        res = self._run([x], return_stages)
        return (res[0][0], res[1]) if return_stages else res[0]

    def enhance_batch(self, audios: Sequence, *, return_stages: bool = False):
        """A list of clips of any lengths -> the list of enhanced clips, run as ONE right-padded batch; each equals ``enhance_array`` of that clip."""
        clips = [self._clip_of(a) for a in audios]
        if not clips:
            return []
        if any(c.shape[0] == 0 for c in clips):
            raise ValueError("DeepFilterNet.enhance_batch: empty clip")
        return self._run(clips, return_stages)

    def enhance_file(self, input_path: Union[str, Path], output_path: Union[str, Path]) -> Path:
        input_path, output_path = Path(input_path), Path(output_path)
        audio, sr = audio_io.read(str(input_path), always_2d=False, dtype="float32")
        if sr != self.config.sample_rate:
            raise ValueError(f"Expected {self.config.sample_rate} Hz audio, got {sr} Hz: {input_path}")
        if audio.ndim > 1:
            audio = audio[:, 0]
        audio_io.write(str(output_path), self.enhance_array(audio), self.config.sample_rate)
        return output_path

    # ------------------------------------------------------------------ not built
    def create_streamer(self, **kw):
        _not_built("create_streamer")

    def enhance_array_streaming(self, audio, chunk_samples=None, **kw):
        _not_built("enhance_array_streaming")

    def enhance_file_streaming(self, input_path, output_path, chunk_samples=None, **kw):
        _not_built("enhance_file_streaming")
