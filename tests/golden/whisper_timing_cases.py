"""Inputs of the Whisper word-timing fixtures, shared by ``make_whisper_timing_fixtures.py`` (which runs the reference on them) and the tests (which run
this package on them).  Token ids are those of ``tests/_whisper_timing_ref.toy_table()``; ``TB`` is the first timestamp token."""
import numpy as np

TB = 50364
EOT = 50257
SEED_W = 5
# the cross-attention keys are a Linear(n_state, n_state) over the ENCODER's features (whisper.py:342-345), so both states are 256 wide: 4 decoder layers x 4
# heads of 64 give the 8 default alignment heads
DIMS = dict(n_mels=80, n_audio_ctx=150, n_audio_state=256, n_audio_head=4, n_audio_layer=2, n_vocab=51865, n_text_ctx=64, n_text_state=256,
            n_text_head=4, n_text_layer=4)

# (name, kind, N, M, seed)
MATRICES = (("random", "random", 9, 31, 1), ("integer", "integer", 12, 40, 2), ("zero", "zero", 5, 17, 0), ("narrow", "random", 6, 3, 4))


def make_matrix(kind, N, M, seed):
    g = np.random.default_rng(seed)
    if kind == "random":
        return g.standard_normal((N, M)).astype(np.float32)
    if kind == "integer":
        return g.integers(-2, 3, size=(N, M)).astype(np.float32)
    return np.zeros((N, M), np.float32)


# (language, tokens): 600 + 601 are the two halves of one three-byte character, 601 alone is a stray continuation byte
SPLIT_CASES = (("en", (300, 301, 400, 500, 302, 600, 601, 303, 501, EOT)),
               ("en", (601, 304, 505, 305, 506, 507, 306, 504, EOT)),
               ("ja", (300, 600, 601, 602, 400, EOT)),
               ("zh", (600, 300)),
               ("en", (EOT,)))

ALIGN_CASES = (dict(tokens=(300, 301, 400, 500, 302, 303, 401, 304, 502, 305, 503, 501), num_frames=300, mel_seed=40, certify=True),
               dict(tokens=(306, 600, 601, 307, 504), num_frames=171, mel_seed=60),
               dict(tokens=(), num_frames=300, mel_seed=61),
               dict(tokens=(308, 400, 402), num_frames=300, mel_seed=62))

# add_word_timestamps with a scripted alignment: one (start, end, probability) per word of the tokenizer's split, times relative to the window
ADD_WORDS_CASES = (
    # every punctuation merge (" (" prepended; ")", ",", "." appended) and the sentence-boundary truncation (a long "." and a long word after it)
    dict(last_speech_timestamp=0.0,
         segments=[dict(seek=0, start=0.0, end=5.0, tokens=[TB, 300, 502, 301, 503, 500, 302, 501, 303, TB + 250])],
         alignment=[(0.5, 0.9, 0.9), (0.9, 1.0, 0.8), (1.0, 1.4, 0.7), (1.4, 1.5, 0.6), (1.5, 1.6, 0.5), (1.6, 2.0, 0.9), (2.0, 4.5, 0.4), (4.5, 7.5, 0.3)]),
    # two segments in a later window: a long first word after a pause, and a last word running past the segment's end
    dict(last_speech_timestamp=10.0,
         segments=[dict(seek=3000, start=32.0, end=36.0, tokens=[TB + 100, 304, 305, TB + 300]),
                   dict(seek=3000, start=36.0, end=42.0, tokens=[TB + 300, 306, 401, 307, TB + 600])],
         alignment=[(0.2, 3.0, 0.9), (3.0, 5.5, 0.8), (6.2, 6.6, 0.7), (6.6, 13.5, 0.6)]),
    # the segment-level start wins over a first word that begins long before it; no pause before it
    dict(last_speech_timestamp=34.9,
         segments=[dict(seek=3000, start=35.0, end=40.0, tokens=[TB + 250, 308, 309, 310, TB + 500])],
         alignment=[(3.0, 6.0, 0.9), (6.0, 6.4, 0.8), (6.4, 6.8, 0.7)]),
)

# generate(word_timestamps=True, hallucination_silence_threshold=2.0): scripted decode results and one scripted alignment per add_word_timestamps call
GENERATE_CASES = (
    dict(name="seek_to_last_word_and_anomaly_skip", frames=9000, kw=dict(word_timestamps=True, hallucination_silence_threshold=2.0),
         script=[dict(tokens=[TB, 300, 301, TB + 200, TB + 200, 302, 303, TB + 400, TB + 400, 304]),     # open tail: seek follows the last word's end
                 dict(tokens=[TB + 150, 305, TB + 250, TB + 250, 306, 307, TB + 600]),                    # improbable, very short first word after a gap: skipped
                 dict(tokens=[TB, 308, 309, TB + 300]),
                 dict(tokens=[TB, 310, TB + 1500]),
                 dict(tokens=[TB, 311, 400, 501, TB + 1000])],
         alignments=[[(0.4, 0.9, 0.9), (1.0, 1.6, 0.8), (4.2, 4.8, 0.9), (5.0, 5.6, 0.9)],
                     [(3.2, 3.25, 0.05), (5.2, 5.8, 0.9), (6.0, 6.5, 0.9)],
                     [(0.3, 0.8, 0.9), (0.9, 1.5, 0.9)],
                     [(1.0, 1.5, 0.9)],
                     [(0.5, 1.0, 0.9), (1.0, 1.1, 0.9)]]),
)
