"""Host side of Whisper's word-level timestamps against ``tests/golden/ref_whisper_timing.json`` (the reference's own ``timing.py`` / ``whisper.py`` run by
``tests/golden/make_whisper_timing_fixtures.py``): tokenizer word splitting, punctuation merging, ``add_word_timestamps`` and the
``generate(word_timestamps=True, hallucination_silence_threshold=...)`` loop with a scripted alignment, ``set_alignment_heads``, and the C entry points'
argument checks.  No GPU."""
import base64
import copy
import gzip
import json
import os
import sys

import numpy as np
import pytest
import torch

import _whisper_timing_ref as R
from mlx_audio_amd.stt.models.whisper import Model, ModelDimensions
from mlx_audio_amd.stt.models.whisper import timing as T
from mlx_audio_amd.stt.models.whisper.audio import N_FRAMES
from mlx_audio_amd.stt.models.whisper.decoding import DecodingOptions, DecodingResult
from mlx_audio_amd.stt.models.whisper.tokenizer import Tokenizer, get_tokenizer

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLD)
import whisper_timing_cases as C  # noqa: E402


@pytest.fixture(scope="module")
def meta():
    return json.load(open(os.path.join(GOLD, "ref_whisper_timing.json")))


def _tok(meta, language="en"):
    return get_tokenizer(True, language=language, task="transcribe", codec=R.ToyCodec(meta["table"]))


def test_fixture_table_is_the_helpers(meta):
    assert meta["table"] == R.toy_table() and meta["dims"] == C.DIMS


def test_split_to_word_tokens_matches_the_reference(meta):
    assert len(meta["split"]) == len(C.SPLIT_CASES)
    seen_ja = seen_replacement = False
    for case in meta["split"]:
        tok = _tok(meta, case["language"])
        words, groups = tok.split_to_word_tokens(list(case["tokens"]))
        assert words == case["words"] and [list(g) for g in groups] == case["groups"], (case, words, groups)
        # ... and the helper's restatement agrees
        dec = tok.codec.decode
        hw, hg = (R.split_on_unicode(dec, case["tokens"]) if case["language"] in ("ja", "zh") else R.split_on_spaces(dec, case["tokens"], tok.eot))
        assert hw == case["words"] and [list(g) for g in hg] == case["groups"]
        seen_ja |= case["language"] in ("ja", "zh")
        seen_replacement |= any("\ufffd" in w for w in words)
    assert seen_ja and seen_replacement
    assert [600, 601] in meta["split"][0]["groups"] or any(600 in g and 601 in g for g in meta["split"][0]["groups"])   # the split character is one group
    assert _tok(meta).decode_with_timestamps([300, 50364]) == " w00<|50364|>"


def test_word_splitting_needs_a_vocabulary():
    t = Tokenizer()
    for call in (lambda: t.split_to_word_tokens([1, 2]), lambda: t.decode_with_timestamps([1]), lambda: t.encode("a")):
        with pytest.raises(RuntimeError, match="no vocabulary available"):
            call()


def test_merge_punctuations():
    W = T.WordTiming
    al = [W(" (", [1], 0.0, 0.1, 1.0), W(" a", [2], 0.1, 0.2, 1.0), W(")", [3], 0.2, 0.3, 1.0), W(",", [4], 0.3, 0.4, 1.0), W(" -", [5], 0.4, 0.5, 1.0),
          W(" \"", [6], 0.5, 0.6, 1.0), W(" b", [7], 0.6, 0.7, 1.0), W(".", [8], 0.7, 0.8, 1.0)]
    T.merge_punctuations(al, "\"'\u201c\u00bf([{-", "\"'.\u3002,\uff0c!\uff01?\uff1f:\uff1a\u201d)]}\u3001")
    assert [(w.word, w.tokens) for w in al] == [("", []), (" ( a),", [1, 2, 3, 4]), ("", []), ("", []), ("", []), ("", []), (" - \" b.", [5, 6, 7, 8]), ("", [])]
    assert [(w.start, w.end) for w in al][1] == (0.1, 0.2)    # times stay with the word


def _scripted(spec):
    return lambda model, tokenizer, text_tokens, mel, num_frames, **kw: R.scripted_alignment(tokenizer, text_tokens, spec, T.WordTiming)


def _same_words(got, want, where):
    assert len(got) == len(want), (where, got, want)
    for g, w in zip(got, want):
        assert g["word"] == w["word"], (where, g, w)
        assert g["start"] == pytest.approx(w["start"], abs=1e-9) and g["end"] == pytest.approx(w["end"], abs=1e-9), (where, g, w)
        assert g["probability"] == pytest.approx(w["probability"], abs=1e-12), (where, g, w)


def test_add_word_timestamps_matches_the_reference(meta, monkeypatch):
    assert len(meta["add_words"]) == len(C.ADD_WORDS_CASES)
    for ci, (case, want) in enumerate(zip(C.ADD_WORDS_CASES, meta["add_words"])):
        monkeypatch.setattr(T, "find_alignment", _scripted(case["alignment"]))
        segs = copy.deepcopy(case["segments"])
        T.add_word_timestamps(segments=segs, model=None, tokenizer=_tok(meta), mel=None, num_frames=3000, last_speech_timestamp=case["last_speech_timestamp"])
        for g, w in zip(segs, want["segments"]):
            assert g["start"] == pytest.approx(w["start"], abs=1e-9) and g["end"] == pytest.approx(w["end"], abs=1e-9), (ci, g, w)
            _same_words(g["words"], w["words"], ci)
    # the cases do hit what they are there for: a merged "( ... )," group, a truncated sentence end, and a first word pulled to the segment's start
    words0 = [w["word"] for w in meta["add_words"][0]["segments"][0]["words"]]
    assert " ( w01)," in words0 and any(w.endswith(".") for w in words0)
    T.add_word_timestamps(segments=[], model=None, tokenizer=_tok(meta), mel=None, num_frames=3000, last_speech_timestamp=0.0)   # no segments: nothing to do


def test_set_alignment_heads_input_forms():
    m = Model(ModelDimensions(**C.DIMS), device="cpu")
    default = m.alignment_heads
    assert default.tolist() == [[l, h] for l in (2, 3) for h in range(4)]       # every head of the last half of the decoder layers
    m.set_alignment_heads([[1, 0], [3, 2]])
    assert m.alignment_heads.tolist() == [[1, 0], [3, 2]]
    m.set_alignment_heads(np.array([[0, 3]]))
    assert m.alignment_heads.tolist() == [[0, 3]]
    mask = np.zeros((4, 4), dtype=bool)
    mask[1, 2] = mask[3, 0] = mask[3, 3] = True
    m.set_alignment_heads(base64.b85encode(gzip.compress(mask.tobytes())))
    assert m.alignment_heads.tolist() == [[1, 2], [3, 0], [3, 3]]
    with pytest.raises(ValueError, match="Invalid type"):
        m.set_alignment_heads("abc")


def _gen_dims():
    return ModelDimensions(n_mels=80, n_audio_ctx=1500, n_audio_state=64, n_audio_head=2, n_audio_layer=1, n_vocab=51865, n_text_ctx=448, n_text_state=64,
                           n_text_head=2, n_text_layer=1)


class Stub(Model):
    """A ramp mel, a script of DecodingResults, and a placeholder engine so that the word-timestamp gate opens (the alignment itself is scripted)."""

    def __init__(self, case, table):
        super().__init__(_gen_dims(), device="cpu")
        self.codec = R.ToyCodec(table)
        self.engine = object()
        self.case = case
        self.script = list(case["script"])
        self.calls = []

    def _prepare_audio(self, audio, padding=0):
        n = self.case["frames"] + N_FRAMES
        return torch.arange(1, n + 1, dtype=torch.float32)[:, None].expand(n, 80).clone(), self.case["frames"]

    def decode(self, mel, options=DecodingOptions(), **kw):
        spec = self.script.pop(0)
        self.calls.append(dict(first=float(mel[0, 0]), prompt=[int(t) for t in (options.prompt or [])]))
        return DecodingResult(audio_features=None, language="en", tokens=list(spec["tokens"]), text="", avg_logprob=-0.1, no_speech_prob=0.0,
                              temperature=float(options.temperature), compression_ratio=1.0)


def test_generate_with_word_timestamps_matches_the_reference(meta, monkeypatch):
    assert len(meta["generate"]) == len(C.GENERATE_CASES)
    for case, want in zip(C.GENERATE_CASES, meta["generate"]):
        ascript = list(case["alignments"])
        monkeypatch.setattr(T, "find_alignment", lambda model, tokenizer, text_tokens, mel, num_frames, **kw: R.scripted_alignment(
            tokenizer, text_tokens, ascript.pop(0), T.WordTiming))
        m = Stub(case, meta["table"])
        out = m.generate(np.zeros(16000, np.float32), language="en", temperature=0.0, **case["kw"])
        assert m.calls == want["calls"], (m.calls, want["calls"])                      # the seeks (first mel frame of each window) and the prompts
        assert len(m.script) == want["unused_script"] == 0 and len(ascript) == want["unused_alignments"] == 0
        assert out.text == want["text"].strip()      # this package's STTOutput.text is stripped (as before this feature); the words keep their spaces
        assert len(out.segments) == len(want["segments"])
        for g, w in zip(out.segments, want["segments"]):
            assert (g["id"], g["seek"], g["tokens"], g["text"]) == (w["id"], w["seek"], w["tokens"], w["text"]), (g, w)
            assert g["start"] == pytest.approx(w["start"], abs=1e-9) and g["end"] == pytest.approx(w["end"], abs=1e-9), (g, w)
            _same_words(g["words"], w["words"], case["name"])
        # what the case is there for: one window thrown away by the anomaly rule (more decode calls than windows that kept segments), and a seek
        # that follows the last word's end (560 = 5.6 s) instead of the last timestamp token (800)
        firsts = [c["first"] for c in want["calls"]]
        assert 561.0 in firsts and len(firsts) > len({s["seek"] for s in want["segments"]})


def test_word_timestamps_warn_on_translate_and_keep_raising_without_an_engine(meta, monkeypatch):
    case = C.GENERATE_CASES[0]
    ascript = list(case["alignments"])
    monkeypatch.setattr(T, "find_alignment", lambda model, tokenizer, text_tokens, mel, num_frames, **kw: R.scripted_alignment(
        tokenizer, text_tokens, ascript.pop(0), T.WordTiming))
    with pytest.warns(UserWarning, match="translations may not be reliable"):
        Stub(case, meta["table"]).generate(np.zeros(16000, np.float32), language="en", temperature=0.0, task="translate", word_timestamps=True)
    m = Stub(case, meta["table"])
    m.engine = None
    for kw in (dict(word_timestamps=True), dict(hallucination_silence_threshold=2.0)):
        with pytest.raises(NotImplementedError, match="device engine"):
            m.generate(np.zeros(16000, np.float32), language="en", **kw)
    assert m.calls == []                                                                # raised before anything was decoded
    m.engine = object()
    with pytest.raises(NotImplementedError):
        m.generate(np.zeros(16000, np.float32), language="en", stream=True)


def test_new_symbols_and_abi():
    from mlx_audio_amd import _lib, ops
    from mlx_audio_amd.stt.models.whisper import whisper as W
    from mlx_audio_amd.stt.models.whisper.engine import WhisperEngine

    for name in ("mi355_align_qk_softmax", "mi355_align_matrix", "mi355_dtw", "mi355_dtw_ws_bytes", "mi355_softmax_prob_rows"):
        assert name in _lib.declared_functions()
    for name in ("align_qk_softmax", "align_matrix", "dtw", "dtw_workspace_bytes", "softmax_prob_rows"):
        assert callable(getattr(ops, name))
    for name in ("median_filter", "dtw", "WordTiming", "find_alignment", "merge_punctuations", "add_word_timestamps"):
        assert hasattr(T, name)
    for name in ("word_anomaly_score", "is_segment_anomaly", "next_words_segment", "_get_end"):
        assert callable(getattr(W, name))
    assert callable(WhisperEngine.align)
    lib = _lib.load()
    assert lib.mi355_abi_version() == 37 == _lib.ABI_VERSION


def test_entry_points_refuse_null_arguments_without_a_device():
    from mlx_audio_amd import _lib

    lib = _lib.load()
    S = _lib.STRUCTS
    import ctypes

    def err():
        return lib.mi355_last_error().decode()

    for fn, st in (("mi355_align_qk_softmax", "mi355_align_qk_args"), ("mi355_align_matrix", "mi355_align_matrix_args"), ("mi355_dtw", "mi355_dtw_args")):
        assert getattr(lib, fn)(None, None) == -1 and "null" in err(), fn
        assert getattr(lib, fn)(ctypes.byref(S[st]()), None) == -1 and "null" in err(), fn     # a zeroed struct: every tensor pointer is null
    assert lib.mi355_softmax_prob_rows(None, 4, 4, 1, None, None, None) == -1 and "null" in err()
    assert lib.mi355_dtw_ws_bytes(0, 5, 1) == 0 and lib.mi355_dtw_ws_bytes(448, 1500, 2) >= 2 * 448 * (448 + 1500 - 1)


def test_word_anomaly_helpers():
    from mlx_audio_amd.stt.models.whisper import whisper as W

    assert W.word_anomaly_score(dict(start=0.0, end=0.5, probability=0.9)) == 0.0
    assert W.word_anomaly_score(dict(start=0.0, end=0.033, probability=0.1)) == pytest.approx(1.0 + 0.1 * 15)
    assert W.word_anomaly_score(dict(start=0.0, end=3.0, probability=0.9)) == pytest.approx(1.0)
    seg = dict(end=0.7, words=[dict(word=",", start=0, end=0.01, probability=0.0), dict(word=" a", start=0.0, end=0.5, probability=0.9)])
    assert not W.is_segment_anomaly(seg, ",") and not W.is_segment_anomaly(None, ",") and not W.is_segment_anomaly(dict(words=[]), ",")
    assert W.is_segment_anomaly(dict(words=[dict(word=" a", start=0.0, end=0.01, probability=0.0)]), ",")
    assert W.next_words_segment([dict(words=[]), seg]) is seg and W.next_words_segment([]) is None
    assert W._get_end([dict(end=4.0, words=[])]) == 4.0 and W._get_end([seg]) == 0.5 and W._get_end([]) is None
