#!/usr/bin/env python
"""Runs the reference's OWN ``stt/models/whisper/timing.py`` and ``whisper.py`` (unmodified, imported from where they lie through
``make_reference_fixtures.import_whisper``) over the numpy stand-in for MLX and stores what they compute in ``tests/golden/ref_whisper_timing.npz``
and ``.json``.

  * model: float32, ``make_whisper_weights`` on 150 audio positions, 256-wide 4-head 2-layer encoder, 64 text positions, 256-wide 4-head 4-layer decoder
    (8 default alignment heads, head dim 64);
  * tokenizer: the reference's ``HFTokenizerWrapper`` over a scripted vocabulary (``tests/_whisper_timing_ref.ToyCodec`` on ``toy_table()``);
  * ``find_alignment`` cases (12 tokens / 300 frames, 5 tokens / 171 frames, no tokens, a single word): the [N, F] matrix handed to ``dtw``, the path, the
    per-token probabilities, the ``WordTiming`` records; ``e_ref`` = max |reference float32 matrix - float64 restatement on the same q, k|; for the
    12-token case the path is certified stable under 32 seeded uniform perturbations of amplitude 64 * e_ref (else the next mel seed is tried);
  * ``median_filter`` / ``dtw`` on ready-made matrices (random, integer-valued, all-zero);
  * the tokenizer's word splitting; ``add_word_timestamps`` and ``Model.generate(word_timestamps=True, hallucination_silence_threshold=2.0)`` with a
    scripted alignment (``tests/_whisper_timing_ref.scripted_alignment``) and scripted decode results.
The mels are NOT stored: ``synthetic.make_mel`` regenerates them from their seeds.

Only runs where the reference lies: ``python tests/golden/make_whisper_timing_fixtures.py``."""
import copy
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_reference_fixtures as M  # noqa: E402  (installs the stand-in)
import _whisper_timing_ref as R  # noqa: E402
import whisper_timing_cases as C  # noqa: E402

mx = M.mx

SPECIAL = {"<|startoftranscript|>": 50258, "<|translate|>": 50358, "<|transcribe|>": 50359, "<|startoflm|>": 50360, "<|startofprev|>": 50361,
           "<|nospeech|>": 50362, "<|notimestamps|>": 50363, "<|0.00|>": 50364}


class FakeHF:
    """What HFTokenizerWrapper (whisper.py:46-245) asks of a HuggingFace tokenizer, over the toy vocabulary."""
    eos_token_id = 50257
    unk_token_id = 50257

    def __init__(self, languages):
        self.codec = R.ToyCodec(R.toy_table())
        self.ids = dict(SPECIAL)
        for i, code in enumerate(languages):
            self.ids[f"<|{code}|>"] = 50259 + i

    def encode(self, text, add_special_tokens=False):
        return self.codec.encode(text)

    def decode(self, tokens, skip_special_tokens=False):
        return self.codec.decode(tokens, skip_special_tokens=skip_special_tokens)

    def convert_tokens_to_ids(self, name):
        return self.ids.get(name, self.unk_token_id)


def wt_dict(t):
    return dict(word=t.word, tokens=[int(x) for x in t.tokens], start=float(t.start), end=float(t.end), probability=float(t.probability))


def main():
    from mlx_audio_amd.stt.models.whisper import synthetic as WS

    M.import_reference()
    wh, dec = M.import_whisper()
    timing = sys.modules["mlx_audio.stt.models.whisper.timing"]
    languages = list(sys.modules["mlx_audio.stt.models.whisper.tokenizer"].LANGUAGES.keys())

    def tokenizer(language="en", task="transcribe"):
        return wh.HFTokenizerWrapper(FakeHF(languages), multilingual=True, num_languages=99, language=language, task=task)

    npz, meta = {}, dict(table=R.toy_table(), dims=C.DIMS, seed_w=C.SEED_W)

    # ---------------------------------------------------------------- ready-made matrices
    meta["matrices"] = []
    for name, kind, N, Mm, seed in C.MATRICES:
        x = C.make_matrix(kind, N, Mm, seed)
        npz[f"mat_{name}"] = x
        npz[f"mat_{name}_medfilt"] = np.asarray(timing.median_filter(mx.array(x[None]), 7), dtype=np.float32)[0]   # 3-D in: its 2-D branch pads a 4-D array with 3 pairs
        npz[f"mat_{name}_path"] = np.asarray(timing.dtw(x)).astype(np.int64)
        meta["matrices"].append(name)

    # ---------------------------------------------------------------- tokenizer word splitting
    meta["split"] = []
    for lang, toks in C.SPLIT_CASES:
        words, groups = tokenizer(lang).split_to_word_tokens(list(toks))
        meta["split"].append(dict(language=lang, tokens=list(toks), words=words, groups=[[int(t) for t in g] for g in groups]))

    # ---------------------------------------------------------------- find_alignment on the small model
    dims = WS.ModelDimensions(**C.DIMS)
    w = WS.make_whisper_weights(dims, seed=C.SEED_W)
    model = wh.Model(wh.ModelDimensions(**C.DIMS), dtype=mx.float32)
    model.load_weights([(k, v.numpy()) for k, v in w.items()])
    missing, unexpected, mism = model._load_report
    assert not missing and not unexpected and not mism, (missing[:5], unexpected[:5], mism[:5])
    model.eval()
    tok = tokenizer()
    sot = len(tok.sot_sequence)
    heads = np.asarray(model.alignment_heads).tolist()
    assert len(heads) == 8
    meta["alignment_heads"] = heads
    rec = {}
    MHA = wh.MultiHeadAttention
    orig_attn, orig_dtw = MHA.qkv_attention, timing.dtw

    def spy_attn(self, q, k, v, mask=None):
        for i, blk in enumerate(model.decoder.blocks):
            if blk.cross_attn is self:
                rec.setdefault("qk", {})[i] = (np.asarray(q).copy(), np.asarray(k).copy())
        return orig_attn(self, q, k, v, mask)

    def spy_dtw(x):
        rec["matrix"] = np.asarray(x, dtype=np.float32).copy()
        rec["path"] = np.asarray(orig_dtw(x)).astype(np.int64)
        return rec["path"]

    MHA.qkv_attention, timing.dtw = spy_attn, spy_dtw
    meta["cases"] = []
    try:
        for ci, case in enumerate(C.ALIGN_CASES):
            toks, nf = list(case["tokens"]), case["num_frames"]
            seed = case["mel_seed"]
            while True:
                rec.clear()
                mel = WS.make_mel(1, seed=seed, n_frames=2 * dims.n_audio_ctx)[0].numpy()
                words = timing.find_alignment(model, tok, toks, mx.array(mel), nf)
                entry = dict(tokens=toks, num_frames=nf, mel_seed=seed, words=[wt_dict(t) for t in words], has_matrix="matrix" in rec)
                if "matrix" not in rec:
                    break
                # e_ref: the float64 restatement on the q, k the reference itself fed its attention
                F = nf // 2
                w64 = []
                for l, h in heads:
                    q, k = rec["qk"][l]
                    w64.append(R.qk_softmax(q[0, :, h * 64:(h + 1) * 64], k[0, :F, h * 64:(h + 1) * 64], 64 ** -0.5, 1.0, np.float64))
                m64 = R.align_matrix(np.stack(w64), 7, sot, 1, np.float64)
                e_ref = float(np.abs(rec["matrix"].astype(np.float64) - m64).max())
                np.testing.assert_array_equal(R.dtw(rec["matrix"]), rec["path"])
                entry["e_ref"] = e_ref
                if case.get("certify"):
                    amp = 64 * e_ref
                    g = np.random.default_rng(1234)
                    stable = all(np.array_equal(R.dtw(rec["matrix"] + g.uniform(-amp, amp, rec["matrix"].shape).astype(np.float32)), rec["path"])
                                 for _ in range(32))
                    if not stable:
                        seed += 1
                        continue
                    entry["certified_amplitude"] = amp
                    entry["mel_seed"] = seed
                break
            if "matrix" in rec:
                npz[f"case{ci}_matrix"], npz[f"case{ci}_path"] = rec["matrix"], rec["path"]
            meta["cases"].append(entry)
        # per-token probabilities: timing.py:133-140 restated on the reference model's own logits
        for ci, (case, entry) in enumerate(zip(C.ALIGN_CASES, meta["cases"])):
            if not entry["tokens"]:
                continue
            toks = entry["tokens"]
            full = [*tok.sot_sequence, tok.no_timestamps, *toks, tok.eot]
            mel = WS.make_mel(1, seed=entry["mel_seed"], n_frames=2 * dims.n_audio_ctx)[0].numpy()
            logits, _ = model.forward_with_cross_qk(mx.array(mel)[None], mx.array(np.asarray(full, np.int32))[None])
            lg = np.asarray(logits)[0][sot:-2, :tok.eot]
            npz[f"case{ci}_probs"] = R.softmax_prob_rows(lg, toks, tok.eot, np.float64)
    finally:
        MHA.qkv_attention, timing.dtw = orig_attn, orig_dtw

    # ---------------------------------------------------------------- add_word_timestamps with a scripted alignment
    orig_find = timing.find_alignment
    meta["add_words"] = []
    try:
        for case in C.ADD_WORDS_CASES:
            timing.find_alignment = lambda model, tokenizer, text_tokens, mel, num_frames, _s=case["alignment"], **kw: R.scripted_alignment(
                tokenizer, text_tokens, _s, timing.WordTiming)
            segs = copy.deepcopy(case["segments"])
            timing.add_word_timestamps(segments=segs, model=None, tokenizer=tok, mel=None, num_frames=3000,
                                       last_speech_timestamp=case["last_speech_timestamp"])
            meta["add_words"].append(dict(segments=segs))

        # ------------------------------------------------------------ generate(word_timestamps=True, hallucination_silence_threshold=2.0)
        meta["generate"] = []
        u = sys.modules["mlx_audio.utils"]
        for name in ("base_load_model", "get_model_path", "load_config"):   # as run_whisper_generate: stt/utils.py imports them, generate uses none
            setattr(u, name, None)
        M._load("mlx_audio.stt.utils", f"{M.REF}/stt/utils.py")
        big = wh.ModelDimensions(n_mels=80, n_audio_ctx=1500, n_audio_state=64, n_audio_head=2, n_audio_layer=1, n_vocab=51865, n_text_ctx=448,
                                 n_text_state=64, n_text_head=2, n_text_layer=1)
        for case in C.GENERATE_CASES:
            gm = wh.Model(big, dtype=mx.float32)
            gm.get_tokenizer = lambda language=None, task="transcribe": tokenizer(language or "en", task)
            n = case["frames"] + 3000
            gmel = mx.array(np.broadcast_to(np.arange(1, n + 1, dtype=np.float32)[:, None], (n, 80)).copy())
            gm._prepare_audio = lambda audio, padding=0, gmel=gmel, case=case: (gmel, case["frames"])
            script, ascript, calls = list(case["script"]), list(case["alignments"]), []

            def decode(segment, options, script=script, calls=calls):
                spec = script.pop(0)
                calls.append(dict(first=float(np.asarray(segment)[0, 0]), prompt=[int(t) for t in (options.prompt or [])]))
                return dec.DecodingResult(audio_features=None, language="en", tokens=list(spec["tokens"]), text="", avg_logprob=-0.1, no_speech_prob=0.0,
                                          temperature=float(options.temperature), compression_ratio=1.0)

            def find(model, tokenizer, text_tokens, mel, num_frames, ascript=ascript, **kw):
                return R.scripted_alignment(tokenizer, text_tokens, ascript.pop(0), timing.WordTiming)

            gm.decode = decode
            timing.find_alignment = find
            res = gm.generate(np.zeros(16000, np.float32), language="en", temperature=0.0, **case["kw"])
            segs = [dict(id=s["id"], seek=int(s["seek"]), start=float(s["start"]), end=float(s["end"]), tokens=[int(t) for t in s["tokens"]], text=s["text"],
                         words=s["words"]) for s in res.segments]
            meta["generate"].append(dict(name=case["name"], calls=calls, segments=segs, text=res.text, unused_script=len(script), unused_alignments=len(ascript)))
    finally:
        timing.find_alignment = orig_find

    np.savez_compressed(os.path.join(HERE, "ref_whisper_timing.npz"), **npz)
    with open(os.path.join(HERE, "ref_whisper_timing.json"), "w") as f:
        json.dump(meta, f, ensure_ascii=True, indent=0)
    for e in meta["cases"]:
        print("case", len(e["tokens"]), e["num_frames"], "seed", e["mel_seed"], "e_ref", e.get("e_ref"), "cert", e.get("certified_amplitude"),
              [(w["word"], w["start"], w["end"]) for w in e["words"]])
    for g in meta["generate"]:
        print(g["name"], [c["first"] for c in g["calls"]], [(s["seek"], s["start"], s["end"], len(s["words"])) for s in g["segments"]], g["unused_script"])


if __name__ == "__main__":
    main()
