"""DeepFilterNet2 / DeepFilterNet3 speech enhancement (``mlx_audio/sts/models/deepfilternet``)."""
from .config import DeepFilterNet2Config, DeepFilterNet3Config, DeepFilterNetConfig
from .model import DeepFilterNetModel, make_dfn_weights  # noqa: F401

Model = DeepFilterNetModel
ModelConfig = DeepFilterNetConfig

__all__ = ["DeepFilterNetModel", "DeepFilterNetConfig", "DeepFilterNet2Config", "DeepFilterNet3Config", "Model", "ModelConfig"]
