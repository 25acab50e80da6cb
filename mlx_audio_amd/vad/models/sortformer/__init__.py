from .config import FCEncoderConfig, ModelConfig, ModulesConfig, ProcessorConfig, TFEncoderConfig  # noqa: F401
from .sortformer import (DiarizationOutput, DiarizationSegment, Model, StreamingState, extract_mel_features,  # noqa: F401
                         make_sortformer_weights, preemphasis_filter)

DETECTION_HINTS = {
    "architectures": ["SortformerOffline"],
    "config_keys": ["fc_encoder_config", "tf_encoder_config", "sortformer_modules"],
}

__all__ = ["FCEncoderConfig", "TFEncoderConfig", "ModulesConfig", "ModelConfig", "Model", "DETECTION_HINTS"]
