# The reference's ``Model`` is bound here as ``GraniteSpeechNar``, deliberately not under its own name: the registry advertises a family whose package
# exports ``Model`` as loadable through ``stt.load``, and the generic loader does not build this model (``GraniteSpeechNar.from_pretrained`` on a local
# directory is the entry point), as for Parakeet and SenseVoice.
from .config import EncoderConfig, ModelConfig, ProjectorConfig, TextConfig  # noqa: F401
from .granite_speech_nar import Model as GraniteSpeechNar  # noqa: F401
from .granite_speech_nar import add_insertion_slots, ctc_collapse_decode, make_granite_nar_weights  # noqa: F401
