"""MossFormer2 SE 48K speech enhancement (``mlx_audio/sts/models/mossformer2_se``)."""
from .config import MossFormer2SEConfig
from .model import MossFormer2SEModel
from .network import make_mossformer2_weights  # noqa: F401

Model = MossFormer2SEModel
ModelConfig = MossFormer2SEConfig

__all__ = ["MossFormer2SEModel", "MossFormer2SEConfig", "Model", "ModelConfig"]
