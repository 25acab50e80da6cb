"""``MossFormer2SEConfig`` of the reference (sts/models/mossformer2_se/config.py): the same fields, defaults, ``from_dict`` / ``to_dict`` and alias."""
from __future__ import annotations

from dataclasses import asdict, dataclass, fields


@dataclass
class MossFormer2SEConfig:
    # audio and STFT
    sample_rate: int = 48000
    win_len: int = 1920
    win_inc: int = 384
    fft_len: int = 1920
    win_type: str = "hamming"
    # Kaldi fbank features
    num_mels: int = 60
    preemphasis: float = 0.97
    # whole-clip decoding up to one_time_decode_length seconds, windows of decode_window seconds above it
    one_time_decode_length: int = 20
    decode_window: int = 4
    # chunked mode
    chunk_seconds: float = 4.0
    chunk_overlap: float = 0.25
    auto_chunk_threshold: float = 60.0
    # network widths (the reference's TestNet hard-wires 180 / 512 / 961 / 24: the defaults)
    in_channels: int = 180
    out_channels: int = 512
    out_channels_final: int = 961
    num_blocks: int = 24

    @classmethod
    def from_dict(cls, config_dict: dict) -> "MossFormer2SEConfig":
        """Unknown keys are ignored."""
        known = {f.name for f in fields(cls)}
        return cls(**{k: v for k, v in config_dict.items() if k in known})

    def to_dict(self) -> dict:
        return asdict(self)

    @property
    def sampling_rate(self) -> int:
        return self.sample_rate
