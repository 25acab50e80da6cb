# ``Model`` is deliberately not exported here: the registry and ``utils.get_model_class`` take a family whose package has a ``Model`` as loadable
# through ``stt.load``, and the generic loader does not build Moonshine.  ``mlx_audio_amd.stt.models.moonshine.moonshine.Model.from_pretrained`` is
# the entry point, as ``parakeet.parakeet`` is Parakeet's.
from .config import ModelConfig  # noqa: F401
from .moonshine import expected_shapes, make_moonshine_weights, stem_lengths  # noqa: F401
