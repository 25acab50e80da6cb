"""Vocabulary helpers of the Parakeet decoders (stt/models/parakeet/tokenizer.py): SentencePiece pieces to text, host-side Python."""
from typing import List

WORD_START = "▁"   # SentencePiece's word-boundary mark


def _is_special_piece(piece: str) -> bool:
    return piece in ("<unk>", "<pad>") or (piece.startswith("<|") and piece.endswith("|>"))


def is_special_token(token_id: int, vocabulary: List[str]) -> bool:
    """Ids outside the vocabulary (the CTC blank among them) are not special."""
    return 0 <= token_id < len(vocabulary) and _is_special_piece(vocabulary[token_id])


def decode(tokens: List[int], vocabulary: List[str]) -> str:
    """The pieces of the in-vocabulary, non-special ids joined, the word-boundary mark turned into a space."""
    pieces = (vocabulary[t] for t in tokens if 0 <= t < len(vocabulary))
    return "".join(p.replace(WORD_START, " ") for p in pieces if not _is_special_piece(p))
