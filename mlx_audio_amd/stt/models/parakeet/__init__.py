# ``Model`` is deliberately not bound here: the registry advertises a family whose package exports ``Model`` as loadable through ``stt.load``, and the
# generic loader does not build Parakeet (``parakeet.Model.from_pretrained`` / ``ParakeetCTC`` are the entry points).
from .audio import PreprocessArgs, log_mel_spectrogram  # noqa: F401
from .conformer import Conformer, ConformerArgs  # noqa: F401
from .ctc import AuxCTCArgs, ConvASRDecoder, ConvASRDecoderArgs  # noqa: F401
from .parakeet import CTCDecodingArgs, ParakeetCTC, ParakeetCTCArgs, ParakeetRNNT, ParakeetTDT, ParakeetTDTCTC, make_parakeet_weights  # noqa: F401
