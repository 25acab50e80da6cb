"""DeepFilterNet configuration (``mlx_audio/sts/models/deepfilternet/config.py``): field for field the reference's dataclasses, so a ``config.json``
written for it loads here unchanged."""
from __future__ import annotations

from dataclasses import dataclass, field, fields
from typing import List, Optional

# the keys ``to_dict`` writes, in the reference's order (it leaves ``df_pathway_kernel_size_t`` out)
_DICT_KEYS = ("sample_rate", "model_version", "fft_size", "hop_size", "nb_erb", "erb_widths", "nb_df", "df_order", "df_lookahead", "conv_lookahead", "conv_ch",
              "conv_k_enc", "conv_k_dec", "conv_width_factor", "conv_dec_mode", "conv_depthwise", "convt_depthwise", "conv_kernel", "convt_kernel",
              "conv_kernel_inp", "emb_hidden_dim", "emb_num_layers", "df_hidden_dim", "df_num_layers", "emb_gru_skip", "emb_gru_skip_enc", "df_gru_skip",
              "gru_groups", "linear_groups", "enc_linear_groups", "group_shuffle", "mask_pf", "pf_beta", "enc_concat", "dfop_method", "lsnr_max", "lsnr_min",
              "lsnr_dropout", "chunk_seconds", "chunk_overlap", "auto_chunk_threshold")


@dataclass
class DeepFilterNetConfig:
    model_version: str = "DeepFilterNet3"
    sample_rate: int = 48000
    # STFT
    fft_size: int = 960
    hop_size: int = 480
    # ERB bands and deep filtering
    nb_erb: int = 32
    erb_widths: Optional[List[int]] = None
    nb_df: int = 96
    df_order: int = 5
    df_lookahead: int = 0
    conv_lookahead: int = 0
    # architecture
    conv_ch: int = 16
    conv_k_enc: int = 1
    conv_k_dec: int = 1
    conv_width_factor: int = 1
    conv_dec_mode: str = "transposed"
    conv_depthwise: bool = True
    convt_depthwise: bool = True
    conv_kernel: List[int] = field(default_factory=lambda: [1, 3])
    convt_kernel: List[int] = field(default_factory=lambda: [1, 3])
    conv_kernel_inp: List[int] = field(default_factory=lambda: [3, 3])
    emb_hidden_dim: int = 256
    emb_num_layers: int = 2
    df_hidden_dim: int = 256
    df_num_layers: int = 3
    df_pathway_kernel_size_t: int = 5
    # skip connections
    emb_gru_skip: str = "none"
    emb_gru_skip_enc: str = "none"
    df_gru_skip: str = "none"
    # grouped linears
    gru_groups: int = 8
    linear_groups: int = 8
    enc_linear_groups: int = 16
    group_shuffle: bool = False
    # post filter
    mask_pf: bool = False
    pf_beta: float = 0.02
    # other
    enc_concat: bool = False
    dfop_method: str = "real_unfold"
    lsnr_max: int = 35
    lsnr_min: int = -15
    lsnr_dropout: bool = False
    # processing
    chunk_seconds: float = 4.0
    chunk_overlap: float = 0.25
    auto_chunk_threshold: float = 60.0

    @property
    def freq_bins(self) -> int:
        return self.fft_size // 2 + 1

    @property
    def sr(self) -> int:
        return self.sample_rate

    @classmethod
    def from_dict(cls, config_dict: dict) -> "DeepFilterNetConfig":
        known = {f.name for f in fields(cls)}
        return cls(**{k: v for k, v in config_dict.items() if k in known})

    def to_dict(self) -> dict:
        return {k: getattr(self, k) for k in _DICT_KEYS}


@dataclass
class DeepFilterNet2Config(DeepFilterNetConfig):
    model_version: str = "DeepFilterNet2"


@dataclass
class DeepFilterNet3Config(DeepFilterNetConfig):
    model_version: str = "DeepFilterNet3"
