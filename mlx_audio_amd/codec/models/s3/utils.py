"""S3 speech tokenizer front end (codec/models/s3/utils.py:8-42): Whisper's log-mel with a periodic Hann window, 128 mels and every frame kept;
and the reference's host helpers (masks, batching, merging of overlapping windows) on torch tensors."""
from typing import List, Tuple

import torch

from ....frontends import whisper_style_log_mel


def log_mel_spectrogram(audio, sample_rate: int = 16_000, n_mels: int = 128, n_fft: int = 400, hop_length: int = 160, padding: int = 0) -> torch.Tensor:
    """``[L]`` samples -> ``[n_mels, n_frames]``."""
    x = torch.as_tensor(audio, dtype=torch.float32).reshape(-1)
    if padding > 0:
        x = torch.nn.functional.pad(x, (0, padding))
    return whisper_style_log_mel(x, sample_rate, n_fft, hop_length, n_mels, periodic_window=True, drop_last=False)[0].t().contiguous()


def make_non_pad_mask(lengths, max_len: int = 0) -> torch.Tensor:
    """utils.py:45-80: bool [B, max_len], True on the first ``lengths[b]`` positions of row b (``max_len`` 0 = the longest)."""
    lengths = torch.as_tensor(lengths).reshape(-1)
    n = int(max_len) if max_len > 0 else int(lengths.max())
    return torch.arange(n, dtype=torch.int32, device=lengths.device)[None, :] < lengths[:, None]


def mask_to_bias(mask: torch.Tensor, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """utils.py:83-92: True -> 0, False -> -1e10, as an additive attention bias."""
    assert mask.dtype == torch.bool, "Input mask must be boolean type"
    assert dtype in (torch.float32, torch.bfloat16, torch.float16), "dtype must be a floating point type"
    return (1.0 - mask.to(dtype)) * -1.0e10


def padding(data: List[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
    """utils.py:95-122: a list of mels [n_mels, T_i] -> (zero-padded [B, n_mels, max T], int32 lengths [B])."""
    assert isinstance(data, list), "Input must be a list of arrays"
    lens = torch.tensor([int(s.shape[1]) for s in data], dtype=torch.int32)
    out = torch.zeros((len(data), data[0].shape[0], int(lens.max())), dtype=data[0].dtype, device=data[0].device)
    for i, feat in enumerate(data):
        out[i, :, :feat.shape[1]] = feat
    return out, lens


def merge_tokenized_segments(tokenized_segments: List[List[int]], overlap: int, token_rate: int) -> List[int]:
    """utils.py:125-147: overlapping windows' tokens joined by dropping half of the overlap (``overlap // 2`` seconds of tokens) from each inner edge."""
    drop = (overlap // 2) * token_rate
    last = len(tokenized_segments) - 1
    merged: List[int] = []
    for i, tokens in enumerate(tokenized_segments):
        merged.extend(tokens[(drop if i > 0 else 0):(-drop if i != last else len(tokens))])
    return merged
