# ``Model`` is deliberately not exported here: the registry and ``utils.get_model_class`` take a family whose package has a ``Model`` as loadable
# through ``stt.load``, and the generic loader does not build FireRedASR2.  ``mlx_audio_amd.stt.models.fireredasr2.fireredasr2.Model.from_pretrained``
# is the entry point, as ``moonshine.moonshine`` is Moonshine's.
from .config import DecoderConfig, EncoderConfig, ModelConfig  # noqa: F401
from .fireredasr2 import expected_shapes, make_fireredasr2_weights  # noqa: F401
