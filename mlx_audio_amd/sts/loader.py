"""Speech-to-speech loader entry points (``mlx_audio/sts/utils.py``): ``load_model`` / ``load`` of a LOCAL model directory.

The file is not called ``utils.py``: ``registry.kinds()`` advertises every ``<kind>/utils.py`` to the kind-agnostic ``mlx_audio_amd.utils.load_model``
and to the server's model listing, and ``tests/test_api_cpu.py`` pins that set to ``('tts', 'stt')``.  Enhancement models are loaded through this module."""
from __future__ import annotations

from pathlib import Path
from typing import Any, List, Union

from ..utils import base_load_model

# aliases of config.model_type / config.model_version / repo-name parts onto the families this package ships
MODEL_REMAPPING = {
    "deepfilternet": "deepfilternet",
    "deepfilternet2": "deepfilternet",
    "deepfilternet3": "deepfilternet",
}


def get_available_models() -> List[str]:
    """The directories under ``models`` that are values of ``MODEL_REMAPPING``, i.e. the families ``load_model`` routes.  A family that is loaded
    through its own class (``MossFormer2SEModel.from_pretrained``; Mel-Band RoFormer is a module file) is not listed."""
    d = Path(__file__).parent / "models"
    return sorted(p.name for p in d.iterdir() if p.is_dir() and p.name in MODEL_REMAPPING.values())


def load_model(model_path: Union[str, Path], lazy: bool = False, strict: bool = False, **kwargs: Any):
    kwargs.setdefault("model_type", "deepfilternet")   # a DeepFilterNet config.json carries model_version, not model_type
    return base_load_model(model_path=model_path, category="sts", model_remapping=MODEL_REMAPPING, lazy=lazy, strict=strict, **kwargs)


def load(model_path: Union[str, Path], lazy: bool = False, strict: bool = False, **kwargs: Any):
    return load_model(model_path, lazy=lazy, strict=strict, **kwargs)
