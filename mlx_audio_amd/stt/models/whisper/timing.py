"""Word-level timestamps (reference ``stt/models/whisper/timing.py``): cross-attention alignment + dynamic time warping.

Everything before the word bookkeeping runs on MI355X (``csrc/align.hip`` through ``WhisperEngine.align``): the cross-attention probabilities of
the alignment heads, their standardisation over tokens, the width-7 median filter over frames, the mean over heads (timing.py:143-154) and the DTW
path through the negated matrix (timing.py:52-99 -- a doubly nested host loop of up to 448 x 1500 cells in the reference).  Only the path and the
per-token probabilities come back; the host part below is the reference's: jump times and word boundaries (timing.py:157-181), punctuation merging
(:184-215), the median-duration truncation rules and the per-segment word lists (:218-327).

``median_filter`` and ``dtw`` are the device kernels behind the reference's signatures.  There is no host implementation: without a ROCm device they
raise.
"""
from __future__ import annotations

import itertools
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np
import torch

from .audio import HOP_LENGTH, SAMPLE_RATE, TOKENS_PER_SECOND


def median_filter(x, filter_width: int):
    """timing.py:17-49: median filter of odd width ``filter_width`` along the last dimension with reflect padding; rows no longer than
    ``filter_width // 2`` come back unchanged.  Tensor in -> tensor out (same device), array in -> array out; computed by ``mi355_align_matrix``."""
    from .... import ops

    assert filter_width > 0 and filter_width % 2 == 1, "`filter_width` should be an odd number"
    is_np = not isinstance(x, torch.Tensor)
    t = torch.as_tensor(np.asarray(x, dtype=np.float32)) if is_np else x
    if t.shape[-1] <= filter_width // 2:
        return x
    ops.require_gpu()
    src = t.to("cuda", torch.float32).contiguous()
    F = src.shape[-1]
    rows = src.reshape(1, 1, -1, F)
    out = torch.empty((1, rows.shape[2], F), dtype=torch.float32, device=src.device)
    for r0 in range(0, rows.shape[2], 32768):   # a launch holds up to 65535 rows
        blk = rows[:, :, r0:r0 + 32768]
        ops.align_matrix(blk, out[:, r0:r0 + 32768], medfilt_width=filter_width, standardize=False, negate=False, row_begin=0, row_trim=0)
    out = out.reshape(src.shape)
    return out.cpu().numpy() if is_np else out.to(t.device)


def dtw(x) -> np.ndarray:
    """timing.py:76-99: the warping path through the cost matrix ``x`` [N, M] as an int array [2, path length] (text indices, time indices), computed
    by ``mi355_dtw`` in float32 with the reference's comparison chain."""
    from .... import ops

    ops.require_gpu()
    c = (x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x, dtype=np.float32))).to("cuda", torch.float32).contiguous()
    assert c.dim() == 2
    text, time, plen = ops.dtw(c[None])
    L = int(plen[0])
    return torch.stack([text[0, :L], time[0, :L]]).cpu().numpy().astype(np.int64)


@dataclass
class WordTiming:
    word: str
    tokens: List[int]
    start: float
    end: float
    probability: float


def words_from_path(tokenizer, text_tokens: Sequence[int], text_indices: np.ndarray, time_indices: np.ndarray, text_token_probs: np.ndarray) -> List[WordTiming]:
    """timing.py:157-181: the host half of ``find_alignment``."""
    words, word_tokens = tokenizer.split_to_word_tokens(list(text_tokens) + [tokenizer.eot])
    if len(word_tokens) <= 1:  # eot only
        return []
    word_boundaries = np.pad(np.cumsum([len(t) for t in word_tokens[:-1]]), (1, 0))
    jumps = np.pad(np.diff(text_indices), (1, 0), constant_values=1).astype(bool)
    jump_times = time_indices[jumps] / TOKENS_PER_SECOND
    start_times = jump_times[word_boundaries[:-1]]
    end_times = jump_times[word_boundaries[1:]]
    word_probabilities = [np.mean(text_token_probs[i:j]) for i, j in zip(word_boundaries[:-1], word_boundaries[1:])]
    return [WordTiming(word, tokens, start, end, probability)
            for word, tokens, start, end, probability in zip(words, word_tokens, start_times, end_times, word_probabilities)]


def find_alignment(model, tokenizer, text_tokens: List[int], mel: torch.Tensor, num_frames: int, *, medfilt_width: int = 7,
                   qk_scale: float = 1.0, audio_features: Optional[torch.Tensor] = None) -> List[WordTiming]:
    """timing.py:111-181.  ``mel`` is one padded window [N_FRAMES, n_mels]; ``audio_features`` [n_audio_ctx, n_audio_state]: the encoder output of
    that window when the caller already has it (``generate`` passes the decode result's), so the encoder does not run a second time."""
    if len(text_tokens) == 0:
        return []
    eng = model._need_engine()
    tokens = [*tokenizer.sot_sequence, tokenizer.no_timestamps, *text_tokens, tokenizer.eot]
    if audio_features is not None:
        xa = audio_features[None] if audio_features.dim() == 2 else audio_features
    else:
        xa = eng.encode(mel[None] if mel.dim() == 2 else mel)
    (text_indices, time_indices, probs), = eng.align(xa, [tokens], [num_frames], model.alignment_heads.tolist(), sot_len=len(tokenizer.sot_sequence),
                                                     eot=tokenizer.eot, medfilt_width=medfilt_width, qk_scale=qk_scale)
    return words_from_path(tokenizer, text_tokens, text_indices, time_indices, probs)


def merge_punctuations(alignment: List[WordTiming], prepended: str, appended: str):
    """timing.py:184-215."""
    i = len(alignment) - 2
    j = len(alignment) - 1
    while i >= 0:
        previous = alignment[i]
        following = alignment[j]
        if previous.word.startswith(" ") and previous.word.strip() in prepended:
            following.word = previous.word + following.word
            following.tokens = previous.tokens + following.tokens
            previous.word = ""
            previous.tokens = []
        else:
            j = i
        i -= 1
    i = 0
    j = 1
    while j < len(alignment):
        previous = alignment[i]
        following = alignment[j]
        if not previous.word.endswith(" ") and following.word in appended:
            previous.word = previous.word + following.word
            previous.tokens = previous.tokens + following.tokens
            following.word = ""
            following.tokens = []
        else:
            i = j
        j += 1


def add_word_timestamps(*, segments: List[dict], model, tokenizer, mel: torch.Tensor, num_frames: int,
                        prepend_punctuations: str = "\"'\u201c\u00bf([{-", append_punctuations: str = "\"'.\u3002,\uff0c!\uff01?\uff1f:\uff1a\u201d)]}\u3001",
                        last_speech_timestamp: float, **kwargs):
    """timing.py:218-327: aligns the text tokens of one window's segments and files the words into them (``segment["words"]``), adjusting the segment
    bounds like the reference."""
    if len(segments) == 0:
        return
    text_tokens_per_segment = [[token for token in segment["tokens"] if token < tokenizer.eot] for segment in segments]
    text_tokens = list(itertools.chain.from_iterable(text_tokens_per_segment))
    alignment = find_alignment(model, tokenizer, text_tokens, mel, num_frames, **kwargs)
    word_durations = np.array([t.end - t.start for t in alignment])
    word_durations = word_durations[word_durations.nonzero()]
    median_duration = np.median(word_durations) if len(word_durations) > 0 else 0.0
    median_duration = min(0.7, float(median_duration))
    max_duration = median_duration * 2

    if len(word_durations) > 0:  # timing.py:246-256: words at sentence boundaries are no longer than twice the median duration
        sentence_end_marks = ".\u3002!\uff01?\uff1f"
        for i in range(1, len(alignment)):
            if alignment[i].end - alignment[i].start > max_duration:
                if alignment[i].word in sentence_end_marks:
                    alignment[i].end = alignment[i].start + max_duration
                elif alignment[i - 1].word in sentence_end_marks:
                    alignment[i].start = alignment[i].end - max_duration

    merge_punctuations(alignment, prepend_punctuations, append_punctuations)

    time_offset = segments[0]["seek"] * HOP_LENGTH / SAMPLE_RATE
    word_index = 0
    for segment, text_tokens in zip(segments, text_tokens_per_segment):
        saved_tokens = 0
        words = []
        while word_index < len(alignment) and saved_tokens < len(text_tokens):
            timing = alignment[word_index]
            if timing.word:
                words.append(dict(word=timing.word, start=float(round(time_offset + timing.start, 2)), end=float(round(time_offset + timing.end, 2)),
                                  probability=float(timing.probability)))
            saved_tokens += len(timing.tokens)
            word_index += 1

        if len(words) > 0:
            # timing.py:283-301: the first and second word after a pause are no longer than twice the median duration
            if words[0]["end"] - last_speech_timestamp > median_duration * 4 and (
                    words[0]["end"] - words[0]["start"] > max_duration
                    or (len(words) > 1 and words[1]["end"] - words[0]["start"] > max_duration * 2)):
                if len(words) > 1 and words[1]["end"] - words[1]["start"] > max_duration:
                    boundary = max(words[1]["end"] / 2, words[1]["end"] - max_duration)
                    words[0]["end"] = words[1]["start"] = boundary
                words[0]["start"] = max(0, words[0]["end"] - max_duration)
            # timing.py:303-312: the segment-level start wins when the first word is too long
            if segment["start"] < words[0]["end"] and segment["start"] - 0.5 > words[0]["start"]:
                words[0]["start"] = max(0, min(words[0]["end"] - median_duration, segment["start"]))
            else:
                segment["start"] = words[0]["start"]
            # timing.py:314-323: likewise the segment-level end
            if segment["end"] > words[-1]["start"] and segment["end"] + 0.5 < words[-1]["end"]:
                words[-1]["end"] = max(words[-1]["start"] + median_duration, segment["end"])
            else:
                segment["end"] = words[-1]["end"]
            last_speech_timestamp = segment["end"]

        segment["words"] = words
