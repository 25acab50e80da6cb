"""``stt/models/sensevoice/config.py``: the three config dataclasses with every field and their ``from_dict`` rules (unknown keys ignored, nested
dicts converted, and the upstream checkpoints' ``sanm_shfit`` spelling accepted when ``sanm_shift`` itself is absent)."""
from __future__ import annotations

import dataclasses
from dataclasses import dataclass
from typing import Any, Dict, List, Optional


def _known(cls, params: Dict[str, Any]) -> Dict[str, Any]:
    names = {f.name for f in dataclasses.fields(cls)}
    return {k: v for k, v in params.items() if k in names}


@dataclass
class EncoderConfig:
    output_size: int = 512
    attention_heads: int = 4
    linear_units: int = 2048
    num_blocks: int = 50
    tp_blocks: int = 20
    dropout_rate: float = 0.1
    positional_dropout_rate: float = 0.1
    attention_dropout_rate: float = 0.1
    kernel_size: int = 11
    sanm_shift: int = 0
    normalize_before: bool = True

    @classmethod
    def from_dict(cls, params: Dict[str, Any]) -> "EncoderConfig":
        valid = _known(cls, params)
        if "sanm_shfit" in params and "sanm_shift" not in params:   # the spelling of the published config files
            valid["sanm_shift"] = params["sanm_shfit"]
        return cls(**valid)


@dataclass
class FrontendConfig:
    fs: int = 16000
    window: str = "hamming"
    n_mels: int = 80
    frame_length: int = 25
    frame_shift: int = 10
    lfr_m: int = 7
    lfr_n: int = 6

    @classmethod
    def from_dict(cls, params: Dict[str, Any]) -> "FrontendConfig":
        return cls(**_known(cls, params))


@dataclass
class ModelConfig:
    model_type: str = "sensevoice"
    vocab_size: int = 25055
    input_size: int = 560
    encoder_conf: Optional[EncoderConfig] = None
    frontend_conf: Optional[FrontendConfig] = None
    cmvn_means: Optional[List[float]] = None   # used when the model directory holds no am.mvn
    cmvn_istd: Optional[List[float]] = None
    model_path: Optional[str] = None

    def __post_init__(self):
        if self.encoder_conf is None:
            self.encoder_conf = EncoderConfig()
        elif isinstance(self.encoder_conf, dict):
            self.encoder_conf = EncoderConfig.from_dict(self.encoder_conf)
        if self.frontend_conf is None:
            self.frontend_conf = FrontendConfig()
        elif isinstance(self.frontend_conf, dict):
            self.frontend_conf = FrontendConfig.from_dict(self.frontend_conf)

    @classmethod
    def from_dict(cls, params: Dict[str, Any]) -> "ModelConfig":
        """Like the reference's, ``encoder_conf`` / ``frontend_conf`` are POPPED from ``params``."""
        encoder_conf = params.pop("encoder_conf", None)
        frontend_conf = params.pop("frontend_conf", None)
        config = cls(**_known(cls, params))
        if encoder_conf is not None:
            config.encoder_conf = EncoderConfig.from_dict(encoder_conf) if isinstance(encoder_conf, dict) else encoder_conf
        if frontend_conf is not None:
            config.frontend_conf = FrontendConfig.from_dict(frontend_conf) if isinstance(frontend_conf, dict) else frontend_conf
        return config
