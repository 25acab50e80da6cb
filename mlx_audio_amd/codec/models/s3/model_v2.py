"""S3 speech tokenizer v2 on MI355X (codec/models/s3/model_v2.py): mel -> 25 Hz FSQ speech tokens (3^8 = 6561 codes).

The model is Whisper's encoder with three differences -- rotary positions on q / k, the FSMN memory block beside the attention, and a finite-scalar
quantizer as the head -- so the host schedule is ``WhisperEngine.encode``'s with two more launches per block and one at the end:

  * stem: both convs are k = 3, stride 2, pad 1; each runs as a stride-1, 2-tap conv over PAIRS of frames (rows of 2 * C channels, a free view) with
    GELU in the epilogue.  The mel is zeroed beyond ``mel_len`` on the way into its channels-last buffer; conv1 stores only the valid rows of a
    zero-filled buffer (``lens_out``), which is the reference's second mask;
  * block: LayerNorm(eps 1e-6) -> one fused q | k | v GEMM (key bias zero) -> ``head_norm_rope`` on q and k in one launch (rotate-half, host tables)
    -> ``fsmn_memory(v, add = x)`` -> ``flash_attention(lens_k = lens)`` -> the out projection with ``res =`` the FSMN result (x + out(wv) + fsmn in one
    epilogue) -> LayerNorm(eps 1e-5) -> MLP (GELU in the first linear's epilogue, the residual in the second's);
  * head: ``fsq_encode`` on the last hidden state, zero beyond ``code_len``.

All sequences of a call are ONE right-padded batch with an int32 ``lens`` on the device.  Every padded position is zeroed before each conv, masked as a
key and zeroed into and out of the FSMN conv, so the valid frames of a sequence inside a batch equal that sequence run alone at its own length.  (The
reference builds its attention mask as [B, 1, T] against scores [B, H, T, T] (model_v2.py:316-317), which only broadcasts for B == 1 or B == H: as
written it runs one un-padded sequence per call.  What is built here is the module's meaning; the oracle for batches is the reference at B == 1.)

Weights travel as fp16 images (``pack_conv(f16=True)``, like every other engine here) with fp16 hi + lo activations (precision 4); K | V, the FSMN
taps, the LayerNorm parameters and the FSQ projection stay float32: the output is a discrete decision.
"""
from __future__ import annotations

import math
import re
from dataclasses import dataclass
from pathlib import Path
from typing import Dict, List, Optional, Tuple

import torch

from .... import ops
from ....ops import ACT_GELU
from .utils import merge_tokenized_segments

ROPE_DIM = 64          # precompute_freqs_cis(64, 1024 * 2) is hard-wired in AudioEncoderV2 (model_v2.py:285)
ROPE_POSITIONS = 2048
FSMN_TAPS = 31
MAX_FRAMES = 3000      # 30 s of 100 Hz mel frames: longer items take the sliding-window path
WINDOW_STRIDE = 2600   # 30 s windows, 4 s overlap
OVERLAP_S = 4
TOKEN_RATE = 25


@dataclass
class ModelConfig:
    n_mels: int = 128
    n_audio_ctx: int = 1500
    n_audio_state: int = 1280
    n_audio_head: int = 20
    n_audio_layer: int = 6
    n_codebook_size: int = 3**8


def precompute_freqs_cis(dim: int, end: int, theta: float = 10000.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """model_v2.py:25-40 in float32 on the host: (cos, sin) [end, dim / 2] -- the reference concatenates each with itself, the kernel reads one half."""
    freqs = 1.0 / (theta ** (torch.arange(0, dim, 2)[: dim // 2].to(torch.float32) / dim))
    f = torch.outer(torch.arange(end).to(torch.float32), freqs).to(torch.float32)
    return torch.cos(f).contiguous(), torch.sin(f).contiguous()


def conv_out_len(n: int) -> int:
    """k = 3, pad = 1, stride = 2 (model_v2.py:305, 312)."""
    return (n + 2 - 2 - 1) // 2 + 1


def expected_shapes(config: ModelConfig) -> Dict[str, Tuple[int, ...]]:
    """Parameter name -> shape of ``S3TokenizerV2(config)`` (the reference's names, MLX layouts)."""
    na, nm = config.n_audio_state, config.n_mels
    s: Dict[str, Tuple[int, ...]] = {"encoder.conv1.weight": (na, 3, nm), "encoder.conv1.bias": (na,), "encoder.conv2.weight": (na, 3, na), "encoder.conv2.bias": (na,)}
    for i in range(config.n_audio_layer):
        p = f"encoder.blocks.{i}."
        s.update({p + "attn.query.weight": (na, na), p + "attn.query.bias": (na,), p + "attn.key.weight": (na, na), p + "attn.value.weight": (na, na),
                  p + "attn.value.bias": (na,), p + "attn.out.weight": (na, na), p + "attn.out.bias": (na,), p + "attn.fsmn_block.weight": (na, FSMN_TAPS, 1),
                  p + "attn_ln.weight": (na,), p + "attn_ln.bias": (na,), p + "mlp_ln.weight": (na,), p + "mlp_ln.bias": (na,),
                  p + "mlp.layers.0.weight": (4 * na, na), p + "mlp.layers.0.bias": (4 * na,), p + "mlp.layers.2.weight": (na, 4 * na), p + "mlp.layers.2.bias": (na,)})
    s.update({"quantizer.fsq_codebook.project_down.weight": (8, na), "quantizer.fsq_codebook.project_down.bias": (8,)})
    return s


def make_s3_weights(config: ModelConfig = ModelConfig(), seed: int = 0) -> Dict[str, torch.Tensor]:
    """A seeded checkpoint under the reference's parameter names and MLX layouts: matrices N(0, 1 / fan_in) with fan_in = in_features * taps, FSMN taps
    0.1 N(0, 1), biases 0.1 N(0, 1), LayerNorm weights 1 + 0.1 N(0, 1).  float32 tensors holding fp16-representable values, like a checkpoint published
    in fp16 (the engine packs fp16 weight images)."""
    g = torch.Generator().manual_seed(seed)
    w: Dict[str, torch.Tensor] = {}
    for name, shape in expected_shapes(config).items():
        if name.endswith("fsmn_block.weight"):
            t = 0.1 * torch.randn(shape, generator=g)
        elif name.endswith("_ln.weight"):
            t = 1.0 + 0.1 * torch.randn(shape, generator=g)
        elif name.endswith(".bias"):
            t = 0.1 * torch.randn(shape, generator=g)
        else:
            fan_in = shape[-1] * (shape[1] if len(shape) == 3 else 1)
            t = torch.randn(shape, generator=g) / math.sqrt(fan_in)
        w[name] = t.to(torch.float16).to(torch.float32)
    return w


def _pair_taps(w3: torch.Tensor) -> torch.Tensor:
    """[Cout, 3, Cin] (stride 2, pad 1) -> [Cout, 2, 2 Cin] over rows of frame pairs r[t] = (x[2t], x[2t + 1]):
    out[t] = W0 x[2t - 1] + W1 x[2t] + W2 x[2t + 1] = tap0 . r[t - 1] (second half only) + tap1 . r[t]."""
    cout, _, cin = w3.shape
    wp = torch.zeros(cout, 2, 2 * cin)
    wp[:, 0, cin:] = w3[:, 0, :]
    wp[:, 1, :cin] = w3[:, 1, :]
    wp[:, 1, cin:] = w3[:, 2, :]
    return wp


class S3TokenizerV2:
    """``S3TokenizerV2(name, config)`` of the reference; ``weights`` omitted = a freshly initialised model (seeded), as for the other codec classes."""

    def __init__(self, name: str = "speech_tokenizer_v2_25hz", config: ModelConfig = ModelConfig(), weights: Optional[Dict[str, torch.Tensor]] = None,
                 device="cuda:0", seed: int = 0, precision: int = 4):
        if "v1" not in name:
            if "v2" not in name:
                raise ValueError(f"S3TokenizerV2: the model name {name!r} names neither v1 nor v2")
            config.n_codebook_size = 3**8
        if config.n_audio_state % config.n_audio_head or config.n_audio_state // config.n_audio_head != ROPE_DIM:
            raise ValueError(f"S3TokenizerV2: head width {config.n_audio_state}/{config.n_audio_head} is not {ROPE_DIM} (the rotary tables are built for {ROPE_DIM})")
        if config.n_codebook_size != 3**8:
            raise ValueError("S3TokenizerV2: the FSQ head has 3^8 codes")
        ops.require_gpu()
        assert precision in (3, 4)
        self.name = name
        self.config = config
        self.device = torch.device(device)
        self.precision = precision
        cos, sin = precompute_freqs_cis(ROPE_DIM, ROPE_POSITIONS)
        self.cos, self.sin = cos.to(self.device), sin.to(self.device)
        self.load_weights(make_s3_weights(config, seed) if weights is None else weights)

    # ------------------------------------------------------------------ checkpoint handling
    def sanitize(self, weights: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        """model_v2.py:543-587: torch-style keys and conv layouts -> the names and layouts of this model; idempotent."""
        shapes = expected_shapes(self.config)
        out: Dict[str, torch.Tensor] = {}
        for key, value in weights.items():
            if "freqs_cis" in key or "_mel_filters" in key or key.startswith("onnx::"):
                continue
            k = key.replace("quantizer._codebook.", "quantizer.fsq_codebook.").replace("quantizer.codebook.", "quantizer.fsq_codebook.")
            k = re.sub(r"\.mlp\.(\d+)\.", r".mlp.layers.\1.", k)
            if (".conv1." in k or ".conv2." in k or ".fsmn_block." in k) and "weight" in k and value.dim() == 3:
                if k in shapes and tuple(value.shape) != shapes[k]:
                    value = value.swapaxes(1, 2)
            out[k] = value
        return out

    def load_weights(self, weights, strict: bool = True):
        c, dev = self.config, self.device
        w = {k: torch.as_tensor(v).detach().to(torch.float32).cpu() for k, v in dict(weights).items()}
        shapes = expected_shapes(c)
        if strict:
            miss = [k for k in shapes if k not in w]
            if miss:
                raise ValueError(f"S3TokenizerV2.load_weights: missing parameters {miss[:4]}{' ...' if len(miss) > 4 else ''}")
            extra = [k for k in w if k not in shapes]
            if extra:
                raise ValueError(f"S3TokenizerV2.load_weights: unexpected parameters {extra[:4]}{' ...' if len(extra) > 4 else ''}")
        for k, s in shapes.items():
            if k in w and tuple(w[k].shape) != s:
                raise ValueError(f"S3TokenizerV2.load_weights: {k} has shape {tuple(w[k].shape)}, expected {s}")
        na = c.n_audio_state

        def lin(wt, bias):
            return ops.pack_conv(wt, bias, dev, f16=True)

        def vec(name):
            return w[name].contiguous().to(dev)

        self.conv1 = lin(_pair_taps(w["encoder.conv1.weight"]), w["encoder.conv1.bias"])
        self.conv2 = lin(_pair_taps(w["encoder.conv2.weight"]), w["encoder.conv2.bias"])
        self.blocks = []
        for i in range(c.n_audio_layer):
            p = f"encoder.blocks.{i}."
            wq, wk, wv = w[p + "attn.query.weight"], w[p + "attn.key.weight"], w[p + "attn.value.weight"]
            self.blocks.append(dict(
                attn_ln=(vec(p + "attn_ln.weight"), vec(p + "attn_ln.bias")),
                qkv=lin(torch.cat([wq, wk, wv]), torch.cat([w[p + "attn.query.bias"], torch.zeros(na), w[p + "attn.value.bias"]])),
                fsmn=w[p + "attn.fsmn_block.weight"][:, :, 0].contiguous().to(dev),   # [C, 31, 1] -> [C, K]
                out=lin(w[p + "attn.out.weight"], w[p + "attn.out.bias"]),
                mlp_ln=(vec(p + "mlp_ln.weight"), vec(p + "mlp_ln.bias")),
                mlp1=lin(w[p + "mlp.layers.0.weight"], w[p + "mlp.layers.0.bias"]),
                mlp2=lin(w[p + "mlp.layers.2.weight"], w[p + "mlp.layers.2.bias"])))
        self.fsq_w = vec("quantizer.fsq_codebook.project_down.weight")
        self.fsq_b = vec("quantizer.fsq_codebook.project_down.bias")
        return self

    @classmethod
    def from_pretrained(cls, name: str, path: str, config: Optional[ModelConfig] = None, device="cuda:0") -> "S3TokenizerV2":
        """model_v2.py:589-605 for a LOCAL directory holding ``{name}.safetensors`` (the reference's ``fetch_from_hub`` needs the network)."""
        from safetensors.torch import load_file

        p = Path(path)
        if not (p / f"{name}.safetensors").exists():
            raise FileNotFoundError(f"{p / (name + '.safetensors')}: S3TokenizerV2.from_pretrained needs a local directory (no hub access in this build)")
        config = config or ModelConfig()
        return cls(name, config, weights=_sanitized(cls, config, load_file(str(p / f"{name}.safetensors"))), device=device)

    # ------------------------------------------------------------------ encoder + quantizer
    def _f(self, *shape):
        return torch.empty(shape, dtype=torch.float32, device=self.device)

    def _z(self, *shape):
        return torch.zeros(shape, dtype=torch.float32, device=self.device)

    def encode(self, mel: torch.Tensor, mel_len, *, return_layers: bool = False, return_h: bool = False) -> dict:
        """One batched pass (every item at most 2048 code frames): dict(codes int32 [B, T'], code_len int32 [B], and on request ``h`` [B, T', 8] -- the
        FSQ pre-activations --, ``layers`` -- the hidden state after the stem and after every block --, ``fsmn0`` -- block 0's FSMN term -- and ``v0`` -- the value projection it was
        taken from)."""
        c = self.config
        mel = torch.as_tensor(mel, dtype=torch.float32)
        if mel.dim() != 3 or mel.shape[1] != c.n_mels:
            raise ValueError(f"S3TokenizerV2: mel must be [B, {c.n_mels}, T], got {tuple(mel.shape)}")
        B, nm, T = mel.shape
        lens0 = [int(v) for v in torch.as_tensor(mel_len).reshape(-1).tolist()]
        if len(lens0) != B or min(lens0) < 1 or max(lens0) > T:
            raise ValueError(f"S3TokenizerV2: mel_len {lens0} does not fit a mel of shape {tuple(mel.shape)}")
        lens1 = [conv_out_len(n) for n in lens0]
        lens2 = [conv_out_len(n) for n in lens1]
        T1 = conv_out_len(T)
        T2 = conv_out_len(T1)
        if T2 > ROPE_POSITIONS:
            raise ValueError(f"S3TokenizerV2: {T2} code frames, the rotary tables hold {ROPE_POSITIONS} positions (use quantize() for long audio)")
        dev, na, H, dh = self.device, c.n_audio_state, c.n_audio_head, ROPE_DIM
        i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
        len1_d, len2_d = i32(lens1), i32(lens2)
        # mel -> channels-last, zero beyond mel_len, an even number of rows (the pair view)
        x0 = self._z(B, 2 * T1, nm)
        keep = torch.arange(T, device=dev)[None, :, None] < i32(lens0)[:, None, None]
        x0[:, :T] = torch.where(keep, mel.to(dev).transpose(1, 2), torch.zeros((), dtype=torch.float32, device=dev))
        y1 = self._z(B, 2 * T2, na)   # rows at and beyond lens1 stay zero: conv1 stores the valid rows only
        ops.conv_gemm(x0.view(B, T1, 2 * nm), self.conv1, y1, pad=1, post_act=ACT_GELU, lout=T1, lens_out=len1_d, precision=self.precision)
        x = self._f(B, T2, na)
        ops.conv_gemm(y1.view(B, T2, 2 * na), self.conv2, x, pad=1, post_act=ACT_GELU, precision=self.precision)
        layers = [x.clone()] if return_layers else None
        fsmn0 = v0 = None
        h, qkv, mem, att, mid = self._f(B, T2, na), self._f(B, T2, 3 * na), self._f(B, T2, na), self._f(B, T2, na), self._f(B, T2, 4 * na)
        for i, blk in enumerate(self.blocks):
            ops.layernorm(x, h, weight=blk["attn_ln"][0], bias=blk["attn_ln"][1], eps=1e-6)
            ops.conv_gemm(h, blk["qkv"], qkv, precision=self.precision)
            q, k, v = qkv[:, :, 0:na], qkv[:, :, na:2 * na], qkv[:, :, 2 * na:]
            ops.head_norm_rope(q, q, heads=H, dh=dh, cos=self.cos, sin=self.sin, second=(k, k, H, None))
            if return_layers and i == 0:
                fsmn0, v0 = ops.fsmn_memory(v, blk["fsmn"], self._f(B, T2, na), lens=len2_d), v.clone()
            ops.fsmn_memory(v, blk["fsmn"], mem, add=x, lens=len2_d)
            ops.flash_attention(q, k, v, att, heads=H, dh=dh, scale=dh ** -0.5, lens_k=len2_d)
            ops.conv_gemm(att, blk["out"], x, res=mem, precision=self.precision)     # x + out(wv) + fsmn
            ops.layernorm(x, h, weight=blk["mlp_ln"][0], bias=blk["mlp_ln"][1], eps=1e-5)
            ops.conv_gemm(h, blk["mlp1"], mid, post_act=ACT_GELU, precision=self.precision)
            ops.conv_gemm(mid, blk["mlp2"], x, res=x, precision=self.precision)
            if return_layers:
                layers.append(x.clone())
        out = ops.fsq_encode(x, self.fsq_w, self.fsq_b, lens=len2_d, return_h=return_h)
        r = dict(codes=out[0] if return_h else out, code_len=len2_d)
        if return_h:
            r["h"] = out[1]
        if return_layers:
            r["layers"], r["fsmn0"], r["v0"] = layers, fsmn0, v0
        return r

    def __call__(self, mel, mel_len):
        return self.quantize(mel, mel_len)

    def quantize(self, mel, mel_len) -> Tuple[torch.Tensor, torch.Tensor]:
        """mel [B, n_mels, T], mel_len [B] -> (codes int32 [B, T'], code_len int32 [B]) on the device; items longer than 30 s take the sliding windows."""
        lens = torch.as_tensor(mel_len).reshape(-1)
        long_mask = lens > MAX_FRAMES
        if bool(long_mask.any()):
            return self._quantize_mixed_batch(mel, lens, long_mask, MAX_FRAMES)
        return self.quantize_simple(mel, lens)

    def quantize_simple(self, mel, mel_len) -> Tuple[torch.Tensor, torch.Tensor]:
        r = self.encode(mel, mel_len)
        return r["codes"], r["code_len"]

    @staticmethod
    def _segments(lens: List[int], long_mask: List[bool], max_frames: int = MAX_FRAMES, stride: int = WINDOW_STRIDE) -> List[Tuple[int, int, int]]:
        """(item, first frame, frames) of every window of a call (model_v2.py:408-463): a short item is one segment, a long one a window every
        ``stride`` frames while the start lies inside the audio."""
        segs = []
        for b, (n, is_long) in enumerate(zip(lens, long_mask)):
            if not is_long:
                segs.append((b, 0, n))
                continue
            start = 0
            while start < n:
                segs.append((b, start, min(start + max_frames, n) - start))
                start += stride
        return segs

    def _quantize_mixed_batch(self, mel, mel_len, long_audio_mask, max_frames: int = MAX_FRAMES) -> Tuple[torch.Tensor, torch.Tensor]:
        """model_v2.py:378-529: every segment of every item in ONE batched encoder call at its true length, codes trimmed to each segment's
        ``code_len``, the segments of a long item merged with ``merge_tokenized_segments(overlap = 4, token_rate = 25)``, rows zero-padded."""
        mel = torch.as_tensor(mel, dtype=torch.float32)
        B = mel.shape[0]
        lens = [int(v) for v in torch.as_tensor(mel_len).reshape(-1).tolist()]
        is_long = [bool(v) for v in torch.as_tensor(long_audio_mask).reshape(-1).tolist()]
        segs = self._segments(lens, is_long, max_frames, max_frames - OVERLAP_S * 100)
        if not segs:
            return torch.zeros((B, 0), dtype=torch.int32, device=self.device), torch.zeros((B,), dtype=torch.int32, device=self.device)
        Tmax = max(n for _, _, n in segs)
        batch = torch.zeros((len(segs), mel.shape[1], Tmax), dtype=torch.float32, device=mel.device)
        for i, (b, s, n) in enumerate(segs):
            batch[i, :, :n] = mel[b, :, s:s + n]
        r = self.encode(batch, [n for _, _, n in segs])
        codes, code_len = r["codes"].cpu(), r["code_len"].cpu().tolist()
        per_item: Dict[int, List[List[int]]] = {}
        for i, (b, _, _) in enumerate(segs):
            per_item.setdefault(b, []).append(codes[i, :code_len[i]].tolist())
        rows = []
        for b in range(B):
            rows.append(merge_tokenized_segments(per_item[b], overlap=OVERLAP_S, token_rate=TOKEN_RATE) if is_long[b] else per_item[b][0])
        out = torch.zeros((B, max(len(r_) for r_ in rows)), dtype=torch.int32)
        for b, r_ in enumerate(rows):
            out[b, :len(r_)] = torch.tensor(r_, dtype=torch.int32)
        return out.to(self.device), torch.tensor([len(r_) for r_ in rows], dtype=torch.int32, device=self.device)


def _sanitized(cls, config, weights):
    """``sanitize`` needs only the config's shapes: run it without building a model first."""
    probe = cls.__new__(cls)
    probe.config = config
    return cls.sanitize(probe, weights)
