"""Parakeet CTC on MI355X (stt/models/parakeet/parakeet.py): log-mel -> FastConformer encoder -> CTC head -> greedy collapse with token times.

``ParakeetCTC`` keeps the reference's surface (``decode`` / ``decode_chunk`` / ``generate`` / ``from_config`` / ``from_pretrained``); ``decode``
additionally takes a real right-padded batch with ``lengths``, which the reference cannot run (see ``conformer.py``).  The encoder and the head run on
the device and only the [B, T'] frame ids come to the host, where the collapse is the reference's loop restated:

  * a blank frame is skipped WITHOUT resetting the previous token, so the frames ``a, blank, a`` emit ``a`` once (parakeet.py:761-799) -- this is not
    textbook CTC and is reproduced;
  * a token's time is ``t * subsampling_factor / sample_rate * hop_length``, in that order, in Python floats; the last token ends behind the last
    non-blank frame.

Not built: the TDT / RNNT decoders (the encoder they share is this one; TDT needs ``mi355_lstm_seq`` for the prediction network plus a joint step), and
the chunked and streaming ``generate`` paths (they need the chunk-merging helpers of ``nemo/alignment.py`` and the attention caches).
"""
from __future__ import annotations

import dataclasses
import json
import math
import typing
from dataclasses import dataclass
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Union

import torch

from ..nemo.alignment import AlignedResult, AlignedToken, sentences_to_result, tokens_to_sentences
from . import tokenizer
from .audio import PreprocessArgs, log_mel_spectrogram
from .conformer import Conformer, ConformerArgs, expected_shapes
from .ctc import AuxCTCArgs, ConvASRDecoder, ConvASRDecoderArgs, n_classes  # noqa: F401

CTC_TARGET = "nemo.collections.asr.models.ctc_bpe_models.EncDecCTCModelBPE"
RNNT_TARGET = "nemo.collections.asr.models.rnnt_bpe_models.EncDecRNNTBPEModel"
HYBRID_TARGET = "nemo.collections.asr.models.hybrid_rnnt_ctc_bpe_models.EncDecHybridRNNTCTCBPEModel"


@dataclass
class CTCDecodingArgs:
    greedy: Optional[dict]


@dataclass
class ParakeetCTCArgs:
    preprocessor: PreprocessArgs
    encoder: ConformerArgs
    decoder: ConvASRDecoderArgs
    decoding: CTCDecodingArgs


def _from_dict(cls, data: dict):
    """A (nested) dataclass from a config dict: keys the dataclass does not declare are ignored, dataclass-typed fields recurse."""
    hints = typing.get_type_hints(cls)
    kw = {}
    for f in dataclasses.fields(cls):
        if f.name not in data:
            continue
        v, t = data[f.name], hints.get(f.name)
        kw[f.name] = _from_dict(t, v) if dataclasses.is_dataclass(t) and isinstance(v, dict) else v
    return cls(**kw)


def ctc_collapse(ids: Sequence[int], vocabulary: List[str], time_per_frame) -> List[AlignedToken]:
    """``ParakeetCTC.decode``'s loop over one item's frame ids (parakeet.py:757-833).  ``time_per_frame(t)`` is the time of frame ``t``."""
    blank = len(vocabulary)
    tokens: List[AlignedToken] = []
    prev, prev_start = -1, 0

    def emit(token, first_frame, end_frame):
        start = time_per_frame(first_frame)
        tokens.append(AlignedToken(token, start=start, duration=time_per_frame(end_frame) - start, text=tokenizer.decode([token], vocabulary)))

    for t, tok in enumerate(ids):
        tok = int(tok)
        if tok == blank or tok == prev:
            continue   # a blank does not reset ``prev``
        if prev != -1 and not tokenizer.is_special_token(prev, vocabulary):
            emit(prev, prev_start, t)
        prev, prev_start = tok, t
    if prev != -1 and not tokenizer.is_special_token(prev, vocabulary):
        n = len(ids)
        last = n - 1   # the last non-blank frame behind the token's first one (the last frame when there is none)
        for t in range(n - 1, prev_start, -1):
            if int(ids[t]) != blank:
                last = t
                break
        emit(prev, prev_start, last + 1)
    return tokens


def make_parakeet_weights(args: ParakeetCTCArgs, seed: int = 0, head_gain: float = 4.0, blank_bias: float = 0.0) -> Dict[str, torch.Tensor]:
    """A seeded checkpoint under the reference's parameter names and MLX conv layouts: matrices N(0, 1 / fan_in), biases 0.1 N(0, 1), LayerNorm /
    BatchNorm weights 1 + 0.1 N(0, 1), BatchNorm running mean 0.3 N(0, 1) and running variance in [0.5, 1.5], position biases 0.2 N(0, 1), CTC head
    ``head_gain`` N(0, 1) / sqrt(d) with ``blank_bias`` added to the blank's bias.  float32 tensors holding fp16-representable values, like a
    checkpoint published in fp16 (the engine packs fp16 weight images)."""
    g = torch.Generator().manual_seed(seed)
    enc = args.encoder
    shapes = dict(expected_shapes(enc, "encoder."))
    V = n_classes(args.decoder)
    shapes["decoder.decoder_layers.0.weight"] = (V, 1, args.decoder.feat_in)
    shapes["decoder.decoder_layers.0.bias"] = (V,)
    w: Dict[str, torch.Tensor] = {}
    for name, shape in shapes.items():
        if name.endswith("running_var"):
            t = 0.5 + torch.rand(shape, generator=g)
        elif name.endswith("running_mean"):
            t = 0.3 * torch.randn(shape, generator=g)
        elif "pos_bias_" in name:
            t = 0.2 * torch.randn(shape, generator=g)
        elif name.endswith(".bias"):
            t = 0.1 * torch.randn(shape, generator=g)
        elif ".norm_" in name or ".batch_norm." in name:
            t = 1.0 + 0.1 * torch.randn(shape, generator=g)
        elif name.startswith("decoder."):
            t = head_gain * torch.randn(shape, generator=g) / math.sqrt(shape[-1])
        else:
            fan_in = 1
            for s in shape[1:]:
                fan_in *= s
            t = torch.randn(shape, generator=g) / math.sqrt(fan_in)
        if name == "decoder.decoder_layers.0.bias":
            t[-1] += blank_bias
        w[name] = t.to(torch.float16).to(torch.float32)
    return w


class Model:
    """The surface every Parakeet variant shares (parakeet.py:131-486)."""

    def __init__(self, preprocess_args: PreprocessArgs):
        self.preprocessor_config = preprocess_args

    def decode(self, mel, lengths=None) -> List[AlignedResult]:
        raise NotImplementedError

    def decode_chunk(self, audio_data, verbose: bool = False) -> AlignedResult:
        mel = log_mel_spectrogram(audio_data, self.preprocessor_config)
        result = self.decode(mel)[0]
        if verbose:
            print(result.text)
        return result

    def generate(self, audio: Union[str, Path, torch.Tensor], *, dtype=torch.float32, chunk_duration: Optional[float] = None,
                 overlap_duration: Optional[float] = None, chunk_callback=None, stream: bool = False, **kwargs) -> AlignedResult:
        """Transcribes a file or a waveform in one piece.  ``stream=True`` and a ``chunk_duration`` shorter than the audio raise: those paths are
        not built."""
        verbose = kwargs.pop("verbose", False)
        if stream:
            raise NotImplementedError("Parakeet generate(stream=True): streaming needs the encoder's attention caches (cache=) and the chunk merging of "
                                      "nemo/alignment.py, neither of which is built")
        if isinstance(audio, (str, Path)):
            from ...utils import load_audio

            audio = torch.from_numpy(load_audio(str(audio), self.preprocessor_config.sample_rate))
        audio = torch.as_tensor(audio, dtype=torch.float32).reshape(-1)
        if chunk_duration is not None:
            overlap_duration = 2.0 if overlap_duration is None else overlap_duration
            if overlap_duration >= chunk_duration:
                raise ValueError(f"overlap_duration ({overlap_duration}s) must be less than chunk_duration ({chunk_duration}s).")
            if audio.numel() / self.preprocessor_config.sample_rate > chunk_duration:
                raise NotImplementedError("Parakeet generate(chunk_duration=...) on audio longer than one chunk: the chunk merging "
                                          "(merge_longest_contiguous / merge_longest_common_subsequence of nemo/alignment.py) is not built")
        return self.decode_chunk(audio, verbose)

    @classmethod
    def from_config(cls, config: dict, weights: Optional[Dict[str, torch.Tensor]] = None, device="cuda:0", seed: int = 0):
        """The model a NeMo ``config.json`` names; without ``weights`` a seeded checkpoint (the reference: randomised weights)."""
        target, tdt = config.get("target"), config.get("model_defaults", {}).get("tdt_durations") is not None
        if target == CTC_TARGET:
            args = _from_dict(ParakeetCTCArgs, config)
            return ParakeetCTC(args, weights if weights is not None else make_parakeet_weights(args, seed), device=device)
        if target in (RNNT_TARGET, HYBRID_TARGET):
            kind = "ParakeetTDTCTC" if target == HYBRID_TARGET else ("ParakeetTDT" if tdt else "ParakeetRNNT")
            raise NotImplementedError(f"{kind}: the transducer decoders are not built.  The FastConformer encoder they share is ready "
                                      "(mlx_audio_amd.stt.models.parakeet.conformer.Conformer); what is missing is the prediction network "
                                      "(an LSTM: mi355_lstm_seq) and the joint step of the greedy loop")
        raise ValueError("Model is not supported yet!")

    @classmethod
    def from_pretrained(cls, path_or_hf_repo: str, *, device="cuda:0"):
        """A LOCAL directory holding ``config.json`` and ``model.safetensors`` (the reference's parameter names, MLX conv layouts, float32)."""
        from safetensors.torch import load_file

        p = Path(path_or_hf_repo)
        if not (p / "config.json").exists() or not (p / "model.safetensors").exists():
            raise FileNotFoundError(f"{path_or_hf_repo}: Parakeet.from_pretrained needs a local directory (no hub access in this build)")
        with open(p / "config.json") as f:
            config = json.load(f)
        return cls.from_config(config, weights=load_file(str(p / "model.safetensors")), device=device)


class ParakeetCTC(Model):
    def __init__(self, args: ParakeetCTCArgs, weights: Optional[Dict[str, torch.Tensor]] = None, device="cuda:0", seed: int = 0):
        super().__init__(args.preprocessor)
        self.args = args
        self.encoder_config = args.encoder
        self.vocabulary = args.decoder.vocabulary
        weights = make_parakeet_weights(args, seed) if weights is None else weights
        extra = [k for k in weights if not (k.startswith("encoder.") or k.startswith("decoder."))]
        if extra:
            raise ValueError(f"ParakeetCTC: unexpected parameters {extra[:4]}{' ...' if len(extra) > 4 else ''}")
        self.encoder = Conformer(args.encoder, weights, device=device, prefix="encoder.")
        self.decoder = ConvASRDecoder(args.decoder, weights, device=device, prefix="decoder.")
        if n_classes(args.decoder) != len(self.vocabulary) + 1:
            raise ValueError(f"ParakeetCTC: {n_classes(args.decoder)} classes for a vocabulary of {len(self.vocabulary)} (the blank is the class behind the vocabulary)")

    def frame_time(self, t: int) -> float:
        return t * self.encoder_config.subsampling_factor / self.preprocessor_config.sample_rate * self.preprocessor_config.hop_length

    def frame_ids(self, mel, lengths=None, *, return_hidden: bool = False):
        """mel [B, T, features] (or [T, features]) -> (ids int64 [B, T'] on the host, out_lengths list); the only device-to-host copy of a decode."""
        mel = torch.as_tensor(mel, dtype=torch.float32)
        if mel.dim() == 2:
            mel = mel[None]
        hidden, out_len = self.encoder(mel, lengths)
        ids = self.decoder.frame_ids(hidden).cpu()
        lens = out_len.cpu().tolist()
        return (ids, lens, hidden) if return_hidden else (ids, lens)

    def decode(self, mel, lengths=None) -> List[AlignedResult]:
        """Greedy CTC over a batch: one ``AlignedResult`` per item.  ``lengths`` [B]: the valid mel frames of a right-padded batch."""
        ids, lens = self.frame_ids(mel, lengths)
        return [sentences_to_result(tokens_to_sentences(ctc_collapse(ids[b, :n].tolist(), self.vocabulary, self.frame_time))) for b, n in enumerate(lens)]


def _not_built(name: str):
    class _Stub(Model):
        def __init__(self, *a, **k):
            raise NotImplementedError(f"{name}: the transducer decoders are not built; the FastConformer encoder they share is ready "
                                      "(mlx_audio_amd.stt.models.parakeet.conformer.Conformer)")

    _Stub.__name__ = _Stub.__qualname__ = name
    return _Stub


ParakeetTDT, ParakeetRNNT, ParakeetTDTCTC = _not_built("ParakeetTDT"), _not_built("ParakeetRNNT"), _not_built("ParakeetTDTCTC")
