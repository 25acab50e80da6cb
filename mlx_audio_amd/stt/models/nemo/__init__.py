from .alignment import AlignedResult, AlignedSentence, AlignedToken, sentences_to_result, tokens_to_sentences  # noqa: F401
