"""CTC head of the Parakeet models (stt/models/parakeet/ctc.py): a 1 x 1 conv to ``num_classes + 1`` logits (the blank is the last class) and a
log-softmax.  On the device the conv is a ``conv_gemm``; the frame arg-max is taken there too, so only [B, T'] ids travel to the host."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List

import torch

from .... import ops


@dataclass
class ConvASRDecoderArgs:
    feat_in: int
    num_classes: int
    vocabulary: List[str]


@dataclass
class AuxCTCArgs:
    decoder: ConvASRDecoderArgs


def n_classes(args: ConvASRDecoderArgs) -> int:
    """Logit count of ``ConvASRDecoder(args)``: the classes (the vocabulary's size when ``num_classes <= 0``) plus the blank."""
    return (len(args.vocabulary) if args.num_classes <= 0 else args.num_classes) + 1


class ConvASRDecoder:
    """``ConvASRDecoder(args)`` of the reference as an engine; ``weights`` holds ``{prefix}decoder_layers.0.weight`` [V + 1, 1, feat_in] and ``.bias``."""

    temperature = 1.0

    def __init__(self, args: ConvASRDecoderArgs, weights: Dict[str, torch.Tensor], device="cuda:0", prefix: str = "decoder.", precision: int = 4):
        ops.require_gpu()
        self.args, self.device, self.precision = args, torch.device(device), precision
        self.classes = n_classes(args)
        w, b = weights[prefix + "decoder_layers.0.weight"], weights[prefix + "decoder_layers.0.bias"]
        if tuple(w.shape) != (self.classes, 1, args.feat_in) or tuple(b.shape) != (self.classes,):
            raise ValueError(f"ConvASRDecoder: weight {tuple(w.shape)} / bias {tuple(b.shape)}, expected {(self.classes, 1, args.feat_in)} / {(self.classes,)}")
        self.head = ops.pack_conv(torch.as_tensor(w, dtype=torch.float32).reshape(self.classes, args.feat_in), torch.as_tensor(b, dtype=torch.float32), self.device, f16=True)

    def logits(self, x: torch.Tensor) -> torch.Tensor:
        y = torch.empty((x.shape[0], x.shape[1], self.classes), dtype=torch.float32, device=self.device)
        return ops.conv_gemm(x, self.head, y, out_scale=1.0 / self.temperature, precision=self.precision)

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        """hidden [B, T', feat_in] -> log-probabilities [B, T', V + 1] on the device."""
        return torch.log_softmax(self.logits(x), dim=-1)

    def frame_ids(self, x: torch.Tensor) -> torch.Tensor:
        """The arg-max class of every frame, int64 [B, T'] on the device."""
        return torch.argmax(self(x), dim=-1)
