"""Token / sentence / result records of the NeMo-family decoders (stt/models/nemo/alignment.py), host-side Python: the same public names, fields and
behaviour.  The chunk-merging helpers of the reference (``merge_longest_contiguous`` / ``merge_longest_common_subsequence``) belong to the chunked
``generate`` path, which is not built yet."""
from dataclasses import dataclass
from typing import List

SENTENCE_ENDS = ("!", "?", "。", "？", "！")


@dataclass
class AlignedToken:
    id: int
    text: str
    start: float
    duration: float
    end: float = 0.0   # always start + duration

    def __post_init__(self) -> None:
        self.end = self.start + self.duration


@dataclass
class AlignedSentence:
    text: str
    tokens: List[AlignedToken]
    start: float = 0.0      # the three below follow from the tokens
    end: float = 0.0
    duration: float = 0.0

    def __post_init__(self) -> None:
        self.tokens = sorted(self.tokens, key=lambda t: t.start)
        self.start = self.tokens[0].start
        self.end = self.tokens[-1].end
        self.duration = self.end - self.start


@dataclass
class AlignedResult:
    text: str
    sentences: List[AlignedSentence]

    def __post_init__(self) -> None:
        self.text = self.text.strip()


def _closes_sentence(tokens: List[AlignedToken], i: int) -> bool:
    """A token closes a sentence when it holds one of ``SENTENCE_ENDS``, or a full stop that is the last token or is followed by a token that starts a
    new word (holds a space)."""
    text = tokens[i].text
    if any(mark in text for mark in SENTENCE_ENDS):
        return True
    return "." in text and (i == len(tokens) - 1 or " " in tokens[i + 1].text)


def tokens_to_sentences(tokens: List[AlignedToken]) -> List[AlignedSentence]:
    sentences: List[AlignedSentence] = []
    run: List[AlignedToken] = []
    for i, token in enumerate(tokens):
        run.append(token)
        if _closes_sentence(tokens, i):
            sentences.append(AlignedSentence(text="".join(t.text for t in run), tokens=run))
            run = []
    if run:
        sentences.append(AlignedSentence(text="".join(t.text for t in run), tokens=run))
    return sentences


def sentences_to_result(sentences: List[AlignedSentence]) -> AlignedResult:
    return AlignedResult("".join(s.text for s in sentences), sentences)
