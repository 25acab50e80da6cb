"""Configuration of Granite Speech NAR under the JSON keys of the checkpoint's ``config.json`` (stt/models/granite_speech_nar/config.py): the
Conformer encoder, the windowed Q-Former projector and the Granite editor, each a section of its own, plus the model-level fields."""
from __future__ import annotations

import dataclasses
import json
from dataclasses import dataclass
from pathlib import Path
from typing import Any, Dict, List, Union


def _take(cls, d: Dict[str, Any], rename=None):
    """The dataclass ``cls`` from the keys of ``d`` it declares (a missing key is a KeyError, as in the reference); ``rename``: field -> getter."""
    rename = rename or {}
    return cls(**{f.name: (rename[f.name](d) if f.name in rename else d[f.name]) for f in dataclasses.fields(cls)})


@dataclass(frozen=True)
class EncoderConfig:
    num_layers: int
    hidden_dim: int
    num_heads: int
    dim_head: int
    input_dim: int
    output_dim: int
    bpe_output_dim: int
    bpe_pooling_window: int
    conv_kernel_size: int
    conv_expansion_factor: int
    feedforward_mult: int
    max_pos_emb: int
    context_size: int
    self_conditioning_layer: int
    blank_token_id: int
    dropout: float
    pred_dropout: float
    initializer_range: float

    @classmethod
    def from_dict(cls, d: Dict[str, Any]) -> "EncoderConfig":
        return _take(cls, d)


@dataclass(frozen=True)
class ProjectorConfig:
    num_layers: int
    num_encoder_layers: int
    hidden_size: int
    num_heads: int
    block_size: int
    downsample_rate: int
    encoder_dim: int
    llm_dim: int
    mlp_ratio: int
    mlp_bias: bool
    attn_bias: bool
    dropout_prob: float
    layernorm_eps: float

    @classmethod
    def from_dict(cls, d: Dict[str, Any]) -> "ProjectorConfig":
        return _take(cls, d)


@dataclass(frozen=True)
class TextConfig:
    hidden_size: int
    intermediate_size: int
    num_hidden_layers: int
    num_attention_heads: int
    num_key_value_heads: int
    vocab_size: int
    max_position_embeddings: int
    rms_norm_eps: float
    rope_theta: float
    tie_word_embeddings: bool
    attention_multiplier: float
    embedding_multiplier: float
    logits_scaling: float
    residual_multiplier: float
    bos_token_id: int
    eos_token_id: int
    pad_token_id: int

    @classmethod
    def from_dict(cls, d: Dict[str, Any]) -> "TextConfig":
        return _take(cls, d, dict(rope_theta=lambda x: x["rope_parameters"]["rope_theta"]))


@dataclass(frozen=True)
class ModelConfig:
    encoder: EncoderConfig
    projector: ProjectorConfig
    text: TextConfig
    encoder_layer_indices: List[int]
    blank_token_id: int
    scale_projected_embeddings: bool
    min_edit_sequence_length: int
    tie_word_embeddings: bool

    @classmethod
    def from_dict(cls, d: Dict[str, Any]) -> "ModelConfig":
        return _take(cls, d, dict(encoder=lambda x: EncoderConfig.from_dict(x["encoder_config"]),
                                  projector=lambda x: ProjectorConfig.from_dict(x["projector_config"]),
                                  text=lambda x: TextConfig.from_dict(x["text_config"]),
                                  encoder_layer_indices=lambda x: list(x["encoder_layer_indices"])))

    def to_dict(self) -> Dict[str, Any]:
        """The JSON shape ``from_dict`` reads."""
        text = dataclasses.asdict(self.text)
        text["rope_parameters"] = dict(rope_theta=text.pop("rope_theta"))
        return dict(encoder_config=dataclasses.asdict(self.encoder), projector_config=dataclasses.asdict(self.projector), text_config=text,
                    encoder_layer_indices=list(self.encoder_layer_indices), blank_token_id=self.blank_token_id,
                    scale_projected_embeddings=self.scale_projected_embeddings, min_edit_sequence_length=self.min_edit_sequence_length,
                    tie_word_embeddings=self.tie_word_embeddings)

    @classmethod
    def from_pretrained(cls, path: Union[str, Path]) -> "ModelConfig":
        return cls.from_dict(json.loads((Path(path) / "config.json").read_text()))
