# ``Model`` is deliberately not bound here: the registry advertises a family whose package exports ``Model`` as loadable through ``stt.load``, and the
# generic loader does not build SenseVoice (``SenseVoiceSmall.from_pretrained`` is the entry point), as for Parakeet.
from .config import EncoderConfig, FrontendConfig, ModelConfig  # noqa: F401
from .sensevoice import SenseVoiceSmall, make_sensevoice_weights  # noqa: F401
