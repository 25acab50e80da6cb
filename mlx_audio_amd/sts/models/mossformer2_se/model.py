"""MossFormer2 SE 48K speech enhancement, waveform to waveform on the device (``mlx_audio/sts/models/mossformer2_se/model.py``).

    samples * 32768 -> Kaldi fbank + delta + delta-delta [T, 180] -> mask estimator (network.py) -> mask [T, 961] x STFT -> iSTFT / 32768

``MossFormer2SEModel`` keeps the reference's surface: ``enhance`` (path / numpy / tensor, the shape rules, the auto-chunk threshold),
``_decode_one_audio`` with its segmented path, ``_decode_chunked``, ``_process_chunk``, ``warmup``, ``load_weights`` under the reference's
parameter names and ``from_pretrained`` of a local directory.  New here, as in DeepFilterNet: ``enhance_batch`` runs a list of clips as ONE
right-padded batch, and the equal-length windows of one segmented or chunked call run as one batch instead of a Python loop.

The front end (``dsp.compute_fbank_kaldi``, ``dsp.compute_deltas_kaldi``, ``dsp.stft``), the mask product and ``ISTFTCache.istft`` run per clip or
on the equal-length batch; the network always runs on the whole batch.  ``dither`` is Kaldi's default 1.0, as in the reference (whose draws come
from its own generator); pass ``dither=0.0`` for repeatable output, or set ``noise_rng`` to a numpy generator to supply the draws.

Not built, each raising ``NotImplementedError`` by name: hub download, quantised checkpoints (``quantization_config`` with ``bits < 16``),
``causal=True`` and ``MossFormerM2`` (``use_mossformer2=True``)."""
from __future__ import annotations

import json
import time
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from .... import dsp, ops
from .config import MossFormer2SEConfig
from .network import MossFormerMaskNet, expected_shapes, make_mossformer2_weights

MAX_WAV_VALUE = 32768.0
DEFAULT_REPO = "starkdmi/MossFormer2_SE_48K_MLX"


# ------------------------------------------------------------------------------------------------ reassembly plans (host integers only)
def segment_plan(t: int, window_size: int) -> Tuple[int, List[Tuple[int, int, int]]]:
    """The segmented path of ``_decode_one_audio`` (model.py:241-284): -> (padded length, [(window start, keep_lo, keep_hi)]) where
    ``window[keep_lo:keep_hi]`` lands at ``start + keep_lo``.  The three padding cases as the reference computes them -- the third pads by
    ``t - (t - window) // stride * stride`` samples, more than the next window boundary needs."""
    stride = int(window_size * 0.75)
    if t < window_size:
        padded = window_size
    elif t < window_size + stride:
        padded = window_size + stride
    elif (t - window_size) % stride != 0:
        padded = t + (t - (t - window_size) // stride * stride)
    else:
        padded = t
    give_up = (window_size - stride) // 2
    plan, idx = [], 0
    while idx + window_size <= padded:
        plan.append((idx, 0 if idx == 0 else give_up, window_size - give_up))
        idx += stride
    return padded, plan


def chunk_plan(n: int, chunk_samples: int, overlap_samples: int, produced=lambda length: length) -> List[Tuple[int, int, int, int]]:
    """``_decode_chunked`` (model.py:317-375) for ``n > chunk_samples``: [(chunk start, chunk length, keep_start, kept samples)]; the kept samples
    ``chunk[keep_start : keep_start + kept]`` land at ``start + keep_start``.  ``produced(length)``: how many samples a chunk of ``length`` gives
    back (the reference measures the RESULT: its frames may cover less than the chunk)."""
    stride, give_up = chunk_samples - overlap_samples, overlap_samples // 2
    starts, idx = [], 0
    while idx + chunk_samples <= n:
        starts.append((idx, chunk_samples))
        idx += stride
    if idx < n:
        starts.append((idx, n - idx))
    plan = []
    for i, (start, length) in enumerate(starts):
        first, last = i == 0, i == len(starts) - 1
        got = produced(length)
        if last and got < chunk_samples:
            keep_start, keep_end = (0 if first else give_up), got
        else:
            keep_start, keep_end = (0 if first else give_up), got - give_up
        out_start, out_end = start + keep_start, min(start + keep_end, n)
        plan.append((start, length, keep_start, max(out_end - out_start, 0)))
    return plan


class MossFormer2SEModel:
    def __init__(self, config: Optional[MossFormer2SEConfig] = None, weights: Optional[Dict[str, torch.Tensor]] = None, device="cuda:0", seed: int = 0,
                 dither: float = 1.0, causal: bool = False, use_mossformer2: bool = False):
        if causal:
            raise NotImplementedError("MossFormer2SEModel: causal=True is not built (mi355_gau_attention is the non-causal form; the checkpoint is non-causal)")
        if use_mossformer2:
            raise NotImplementedError("MossFormer2SEModel: MossFormerM2 (use_mossformer2=True) is not built; the SE 48K checkpoint uses MossFormerM")
        self.config = config or MossFormer2SEConfig()
        self.device = torch.device(device)
        self.dither = float(dither)
        self.noise_rng: Optional[np.random.Generator] = None   # set: the dither draws come from it, [frames, win_len] standard normals per clip
        ops.require_gpu()
        self.net = MossFormerMaskNet(self.config, self.device)
        self._istft_cache = dsp.ISTFTCache()
        self._warmed_up = False
        self.load_weights(make_mossformer2_weights(self.config, seed) if weights is None else weights, strict=True)

    # ------------------------------------------------------------------ checkpoint
    def load_weights(self, weights, strict: bool = False):
        """``weights``: a dict or (name, tensor) pairs under the reference's parameter names (``model.mossformer. ...``).  A missing or wrongly
        shaped parameter is refused (``pos_enc.inv_freq``, a constant, may be absent); an unknown one only under ``strict``."""
        w = {k: torch.as_tensor(np.asarray(v) if not isinstance(v, torch.Tensor) else v).detach().to(torch.float32).cpu() for k, v in dict(weights).items()}
        shapes = expected_shapes(self.config)
        miss = [k for k in shapes if k not in w and not k.endswith("pos_enc.inv_freq")]
        if miss:
            raise ValueError(f"MossFormer2SEModel.load_weights: missing parameters {miss[:4]}{' ...' if len(miss) > 4 else ''}")
        extra = [k for k in w if k not in shapes]
        if extra and strict:
            raise ValueError(f"MossFormer2SEModel.load_weights: unexpected parameters {extra[:4]}{' ...' if len(extra) > 4 else ''}")
        for k, s in shapes.items():
            if k in w and w[k].numel() != int(np.prod(s)):
                raise ValueError(f"MossFormer2SEModel.load_weights: {k} has shape {tuple(w[k].shape)}, expected {s}")
        self.net.load({k: w[k].reshape(shapes[k]) for k in shapes if k in w})
        return self

    def eval(self):
        return self

    @classmethod
    def from_pretrained(cls, model_name_or_path: str = DEFAULT_REPO, *, device="cuda:0", **kwargs) -> "MossFormer2SEModel":
        """model.py:75-142 for a LOCAL directory holding ``config.json`` and ``model.safetensors``."""
        path = Path(str(model_name_or_path)).expanduser()
        if not path.is_dir():
            raise NotImplementedError(f"MossFormer2SEModel.from_pretrained: hub download is not built; {model_name_or_path!r} is not a local directory")
        with open(path / "config.json") as f:
            config_dict = json.load(f)
        quant = config_dict.pop("quantization_config", None)
        if quant and quant.get("bits", 32) < 16:
            raise NotImplementedError(f"MossFormer2SEModel.from_pretrained: quantised checkpoints are not built (quantization_config bits = {quant.get('bits')})")
        weights_path = path / "model.safetensors"
        if not weights_path.exists():
            raise FileNotFoundError(f"Missing model.safetensors in {path}")
        from safetensors.torch import load_file

        return cls(MossFormer2SEConfig.from_dict(config_dict), weights=load_file(str(weights_path)), device=device, **kwargs)

    # ------------------------------------------------------------------ one batch through the front end, the network and the back end
    def features(self, audio: torch.Tensor) -> torch.Tensor:
        """[L] scaled samples -> fbank | delta | delta-delta [T, 3 * num_mels] (model.py:384-398)."""
        c = self.config
        noise = None
        if self.noise_rng is not None and self.dither != 0.0 and audio.numel() >= c.win_len:
            frames = 1 + (audio.numel() - c.win_len) // c.win_inc
            noise = torch.from_numpy(self.noise_rng.standard_normal((frames, c.win_len)).astype(np.float32))
        fb = dsp.compute_fbank_kaldi(audio, sample_rate=c.sample_rate, win_len=c.win_len, win_inc=c.win_inc, num_mels=c.num_mels, win_type=c.win_type,
                                     preemphasis=c.preemphasis, dither=self.dither, noise=noise)
        if fb.shape[0] == 0:
            raise ValueError(f"MossFormer2SEModel: a clip of {audio.numel()} samples is shorter than one window of {c.win_len}")
        d1 = dsp.compute_deltas_kaldi(fb.t(), win_length=5)
        d2 = dsp.compute_deltas_kaldi(d1, win_length=5)
        return torch.cat([fb, d1.t(), d2.t()], dim=1)

    def produced(self, length: int) -> int:
        """Samples ``_process_chunk`` returns for a clip of ``length``: what its frames cover, at most ``length``."""
        c = self.config
        return min((1 + (length - c.win_len) // c.win_inc - 1) * c.win_inc + c.fft_len, length)

    def _process_batch(self, clips: Sequence[torch.Tensor], stages: Optional[dict] = None) -> List[torch.Tensor]:
        """``clips``: scaled float32 clips on the device -> the enhanced clips (still scaled), each of its input's length or, like the reference,
        of the length its frames cover when that is shorter."""
        c = self.config
        feats = [self.features(x) for x in clips]
        frames = [f.shape[0] for f in feats]
        B, T = len(clips), max(frames)
        ragged = min(frames) != T
        fbuf = torch.zeros((B, T, c.in_channels), dtype=torch.float32, device=self.device)
        for b, f in enumerate(feats):
            fbuf[b, :f.shape[0]] = f
        lens = torch.tensor(frames, dtype=torch.int32, device=self.device) if ragged else None
        mask = self.net.forward(fbuf, lens, stages)
        if stages is not None:
            stages["feats"], stages["mask"], stages["frames"] = fbuf, mask, frames
        window = dsp.hamming(c.win_len, periodic=False)
        groups = [list(range(B))] if len({x.numel() for x in clips}) == 1 else [[b] for b in range(B)]
        out: List[Optional[torch.Tensor]] = [None] * B
        for idx in groups:
            n, Tb = clips[idx[0]].numel(), frames[idx[0]]
            spec = dsp.stft(torch.stack([clips[b] for b in idx]), c.fft_len, c.win_inc, c.win_len, window, center=False)      # [b, T, F]
            masked = spec * mask[idx, :Tb]                                                                                   # the mask is real
            y = self._istft_cache.istft(masked.real.transpose(1, 2), masked.imag.transpose(1, 2), c.fft_len, c.win_inc, c.win_len, window, center=False,
                                        audio_length=n)
            for j, b in enumerate(idx):
                out[b] = y[j]
        return out

    def _process_chunk(self, audio_segment, window=None, chunk_length: Optional[int] = None) -> torch.Tensor:
        """model.py:379-436: one scaled clip -> its enhanced samples (``window`` is the reference's argument; the model's own Hamming is used)."""
        x = torch.as_tensor(np.asarray(audio_segment) if not isinstance(audio_segment, torch.Tensor) else audio_segment).to(torch.float32).to(self.device)
        y = self._process_batch([x.reshape(-1)])[0]
        return y if chunk_length is None else y[:chunk_length]

    # ------------------------------------------------------------------ the reference's decode paths
    @staticmethod
    def _mono(inputs) -> np.ndarray:
        a = inputs.detach().cpu().numpy() if isinstance(inputs, torch.Tensor) else np.asarray(inputs)
        return a[0, :] if a.ndim == 2 else a

    def _scaled(self, a: np.ndarray) -> torch.Tensor:
        return torch.from_numpy(np.ascontiguousarray(a * MAX_WAV_VALUE, dtype=np.float32)).to(self.device)

    def _decode_one_audio(self, inputs) -> np.ndarray:
        c = self.config
        a = self._mono(inputs)
        n = a.shape[0]
        if n > c.sample_rate * c.one_time_decode_length:
            window_size = int(c.sample_rate * c.decode_window)
            if self.produced(window_size) != window_size:
                raise ValueError(f"MossFormer2SEModel: decode_window of {window_size} samples is not a whole number of frames (the reference's "
                                 "segment reassembly needs win_len + k * win_inc samples)")
            padded, plan = segment_plan(n, window_size)
            x = self._scaled(np.concatenate([a, np.zeros(padded - n, dtype=a.dtype)]))
            segs = self._process_batch([x[s:s + window_size] for s, _, _ in plan])        # equal lengths: one batch
            out = np.zeros(padded, dtype=np.float64)
            for (s, lo, hi), seg in zip(plan, segs):
                out[s + lo:s + hi] = seg[lo:hi].cpu().numpy()
            out = out[:n]
        else:
            out = self._process_batch([self._scaled(a)])[0].cpu().numpy().astype(np.float64)
        return out / MAX_WAV_VALUE

    def _decode_chunked(self, inputs) -> np.ndarray:
        c = self.config
        a = self._mono(inputs)
        n = a.shape[0]
        chunk_samples = int(c.sample_rate * c.chunk_seconds)
        overlap = int(chunk_samples * c.chunk_overlap)
        if n <= chunk_samples:
            return self._process_batch([self._scaled(a)])[0].cpu().numpy().astype(np.float64) / MAX_WAV_VALUE
        x = self._scaled(a)
        plan = chunk_plan(n, chunk_samples, overlap, self.produced)
        full = [p for p in plan if p[1] == chunk_samples]
        outs = self._process_batch([x[s:s + ln] for s, ln, _, _ in full])                 # the full chunks: one batch
        if len(full) < len(plan):
            s, ln, _, _ = plan[-1]
            outs += self._process_batch([x[s:s + ln]])                                    # the partial last chunk
        out = np.zeros(n, dtype=np.float64)
        for (s, ln, ks, kept), y in zip(plan, outs):
            out[s + ks:s + ks + kept] = y[ks:ks + kept].cpu().numpy()
        return out / MAX_WAV_VALUE

    def _load(self, audio_input) -> np.ndarray:
        if isinstance(audio_input, (str, Path)):
            from ....audio_io import read as audio_read

            a, sr = audio_read(str(audio_input))
            a = np.asarray(a, dtype=np.float32)
            a = a.mean(axis=1) if a.ndim == 2 else a
            if sr != self.config.sample_rate:
                from ....utils import resample_audio

                a = resample_audio(a, sr, self.config.sample_rate)
            return a.reshape(1, -1)
        a = audio_input.detach().cpu().numpy() if isinstance(audio_input, torch.Tensor) else np.asarray(audio_input)
        if a.ndim == 1:
            a = a.reshape(1, -1)
        elif a.ndim == 2 and a.shape[0] > a.shape[1]:
            a = a.T[0:1]
        return a

    def enhance(self, audio_input, chunked: Optional[bool] = None) -> np.ndarray:
        """model.py:169-217: a file path, a numpy array or a tensor ([L], [1, L] or [L, channels]: the first channel) -> the enhanced samples.
        ``chunked`` None picks the chunked mode from ``auto_chunk_threshold`` seconds on."""
        a = self._load(audio_input)
        duration = a.shape[1] / self.config.sample_rate
        use_chunked = chunked if chunked is not None else duration >= self.config.auto_chunk_threshold
        return self._decode_chunked(a) if use_chunked else self._decode_one_audio(a)

    def enhance_batch(self, clips: Sequence, return_stages: bool = False):
        """A list of clips (each as ``enhance`` takes it, any lengths of at least one window) as ONE right-padded batch through the network: the
        whole-clip path of ``_decode_one_audio`` for every item.  -> a list of float64 arrays, each equal to that clip run alone (to rounding: the
        GEMM launches see other row counts)."""
        xs = [self._scaled(self._mono(self._load(c))) for c in clips]
        stages = {} if return_stages else None
        outs = [y.cpu().numpy().astype(np.float64) / MAX_WAV_VALUE for y in self._process_batch(xs, stages)]
        return (outs, stages) if return_stages else outs

    def warmup(self, chunked: bool = False) -> None:
        """model.py:144-167: one pass on 1 s (chunked) or 0.5 s of uniform noise."""
        t0 = time.time()
        g = torch.Generator().manual_seed(0)
        n = 48000 if chunked else 24000
        x = (torch.rand(n, generator=g) * 0.2 - 0.1).numpy()
        if chunked:
            self._process_chunk(torch.from_numpy(x), None, n)
        else:
            self._decode_one_audio(x.reshape(1, -1))
        torch.cuda.synchronize()
        self._warmed_up = True
        print(f"Warmup complete: {time.time() - t0:.2f}s")
