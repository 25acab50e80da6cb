#!/usr/bin/env python
"""Runs the reference's OWN ``stt/models/granite_speech_nar`` files (``encoder.py``, ``projector.py``, ``editor.py``, ``decoding.py``, ``config.py`` and
the feature and transcribe lines of ``granite_speech_nar.py``), unmodified and imported from where they lie, over the numpy stand-in for MLX
(``mlx_shim.py``, left as it is) on seeded float32 checkpoints from ``make_granite_nar_weights`` and stores what they compute in
``tests/golden/ref_granite_nar.npz`` / ``.json``.

The stand-in has no bfloat16 (its ``bfloat16`` is float32), so the ``astype(mx.bfloat16)`` of ``_transcribe_tokens`` would round nothing: the features
are rounded to bfloat16 VALUES here (torch) and fed widened to float32, which is what the reference computes with float32 weights behind that cast.

Per configuration of ``tests/_granite_nar_ref.py`` (A and B) and per clip (400 samples, 1 s, 1.3 s, 3 s, 5 s -> 1, 50, 65, 150, 250 frames) every stage
is stored: the features (before the rounding; the rounded ones as bfloat16 bit patterns, shared by both configurations), ``input_linear``, each
block's attention-module output and block output, the self-conditioning probabilities, the pooled rows, the BPE ids and gaps, the hypothesis, the
projector's queries / kv / output, the editor's input, each editor layer, the tail logits with their gaps, and the final ids.  Frame-indexed stages of
the clips longer than 10 frames keep the rows ``rows`` (every 7th or 25th, the rows around the block boundaries and the last), the projector stages the
first and the last window, the editor stages the first and the last audio row and every text row: the file stays under 1 MB.

Asserted before anything is written, on the reference alone: the stepped modules reproduce ``Model._transcribe_tokens``; EVERY BPE frame decision and
every edited-position decision has a top-2 gap of at least ``tests/_margin.THR`` (a seed that fails is rejected); the runs hold an empty hypothesis,
one with ``2 N + 1 > min_len`` and adjacent repeats that collapse.

Only runs where the reference lies: ``python tests/golden/make_granite_nar_fixtures.py``."""
import json
import os
import sys

import numpy as np
import torch
from transformers import AutoTokenizer  # noqa: F401  (granite_speech_nar.py imports it; loaded BEFORE the stand-in takes the name ``mlx``, which transformers probes)

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_reference_fixtures as M  # noqa: E402  (installs the stand-in)
import _granite_nar_ref as R  # noqa: E402
import _margin  # noqa: E402

mx, nn, _np = M.mx, M.nn, M._np


def load_reference():
    M.import_reference()
    base = "mlx_audio.stt.models.granite_speech_nar"
    for pkg, path in (("mlx_audio.stt", "stt"), ("mlx_audio.stt.models", "stt/models"), (base, "stt/models/granite_speech_nar")):
        if pkg not in sys.modules:
            M._pkg(pkg, f"{M.REF}/{path}")
    M._load("mlx_audio.stt.models.base", f"{M.REF}/stt/models/base.py")
    mods = {}
    for name in ("config", "decoding", "encoder", "projector", "editor", "granite_speech_nar"):
        mods[name] = M._load(f"{base}.{name}", f"{M.REF}/stt/models/granite_speech_nar/{name}.py")
    return mods


def bf16_values(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(torch.bfloat16)


def kept_rows(T, ctx, step=None):
    """The stored rows of a frame-indexed stage: all of a short clip, else every ``step``-th row, the rows around the block boundaries and the last."""
    if T <= 10:
        return np.arange(T)
    step = step or (7 if T <= 50 else 25)
    edges = [r for m in range(ctx, T, ctx) for r in (m - 1, m)]
    return np.unique(np.r_[0:T:step, edges, T - 1]).astype(np.int64)


def kept_windows(nb):
    """The stored projector windows of a clip: the first and the last (the padded one)."""
    return np.unique([0, nb - 1]).astype(np.int64)


def top2_gap(logits):
    s = np.sort(np.asarray(logits, dtype=np.float32), axis=-1)
    return (s[:, -1] - s[:, -2]).astype(np.float32)


class Recorder:
    """Stands where ``projector.qformer`` stood for one call: keeps the arguments, then calls the module."""

    def __init__(self, inner):
        self.inner, self.seen = inner, None

    def __call__(self, query, kv):
        self.seen = (_np(query).copy(), _np(kv).copy())
        return self.inner(query, kv)


def run_clip(G, model, feats_rounded):
    """The reference on ONE clip's (bfloat16-valued) features, its modules stepped in the order of their own ``__call__`` so that every stage can be
    kept; the result is checked against ``Model._transcribe_tokens``."""
    cfg = model.config
    enc, proj, ed = model.encoder, model.projector, model.editor
    out = {}
    x = mx.array(feats_rounded)[None]
    h = enc.input_linear(x)
    out["input_linear"] = _np(h)[0].copy()
    states = [h]
    for i, layer in enumerate(enc.layers, start=1):
        out[f"attn{i}"] = _np(layer.attn(0.5 * layer.ff1(h) + h))[0].copy()
        h = layer(h)
        out[f"block{i}"] = _np(h)[0].copy()
        if i == enc.self_conditioning_layer:
            char_logits = enc.out(h)
            probs = mx.softmax(char_logits.astype(mx.float32), axis=-1)
            blank_probs = probs[..., 0]
            h = h + enc.out_mid(probs.astype(h.dtype))
            out["probs"] = _np(probs)[0].copy()
        states.append(h)
    pooled = G["encoder"]._posterior_weighted_pool(h, blank_probs, enc.bpe_pooling_window)
    bpe_logits = enc.out_bpe(pooled)
    out["pooled"] = _np(pooled)[0].copy()
    out["bpe_ids"] = _np(bpe_logits)[0].argmax(-1).astype(np.int32)
    out["bpe_gap"] = top2_gap(_np(bpe_logits)[0])
    eo = enc(x)
    assert np.array_equal(_np(eo.bpe_logits), _np(bpe_logits)), "the stepped encoder is not the module's own call"
    hyp = G["decoding"].ctc_collapse_decode(mx.array(out["bpe_ids"]), blank_id=cfg.blank_token_id)
    out["hyp"] = np.asarray(_np(hyp), dtype=np.int32).reshape(-1)

    fused = mx.concatenate([states[idx] for idx in cfg.encoder_layer_indices], axis=-1)
    rec = Recorder(proj.qformer)
    proj.qformer = rec
    try:
        audio = proj(fused)
    finally:
        proj.qformer = rec.inner
    nq = proj.cfg.block_size // proj.cfg.downsample_rate
    wins = kept_windows(rec.seen[0].shape[0])
    out["windows"] = wins.astype(np.int32)
    out["proj_queries"], out["proj_kv"] = rec.seen[0][wins], rec.seen[1][wins]
    out["audio"] = _np(audio)[0].reshape(-1, nq, audio.shape[-1])[wins].copy()
    audio = audio / cfg.text.embedding_multiplier
    text_ids = G["decoding"].add_insertion_slots(hyp, blank_id=cfg.blank_token_id, min_len=cfg.min_edit_sequence_length)
    out["text_ids"] = np.asarray(_np(text_ids), dtype=np.int32).reshape(-1)
    flat = mx.concatenate([audio[0], ed.embed_tokens(text_ids).astype(audio.dtype)], axis=0)[None]
    audio_len = audio.shape[1]
    g = flat * ed.embedding_multiplier
    erows = np.r_[0, audio_len - 1:flat.shape[1]].astype(np.int64)          # the first and the last audio row, every text row
    erows = np.unique(erows)
    out["editor_rows"] = erows.astype(np.int32)
    out["editor_in"] = _np(g)[0][erows].copy()
    for i, layer in enumerate(ed.layers):
        g = layer(g)
        out[f"editor{i}"] = _np(g)[0][erows].copy()
    logits = ed.embed_tokens.as_linear(ed.norm(g)[:, audio_len:, :]) / ed.logits_scaling
    own = ed(inputs_embeds=flat, position_ids=mx.arange(flat.shape[1], dtype=mx.int32), logits_start=audio_len)
    assert np.array_equal(_np(own), _np(logits)), "the stepped editor is not the module's own call"
    out["tail_logits"] = _np(logits)[0].copy()
    out["edit_ids"] = out["tail_logits"].argmax(-1).astype(np.int32)
    out["edit_gap"] = top2_gap(out["tail_logits"])
    final = G["decoding"].ctc_collapse_decode(mx.array(out["edit_ids"]), blank_id=cfg.blank_token_id)
    out["final"] = np.asarray(_np(final), dtype=np.int32).reshape(-1)
    whole = model._transcribe_tokens(mx.array(feats_rounded))
    assert np.array_equal(np.asarray(_np(whole), dtype=np.int32).reshape(-1), out["final"]), "the stepped pipeline is not _transcribe_tokens"
    return out


FRAME_STAGES = ("input_linear", "probs")


def main():
    from mlx_audio_amd.stt.models.granite_speech_nar import ModelConfig, make_granite_nar_weights

    G = load_reference()
    S = G["granite_speech_nar"]
    out, meta = {}, dict(clips=[list(c) for c in R.CLIPS], configs={})
    feats = []
    for i, (n, seed) in enumerate(R.CLIPS):
        f = _np(S._compute_features(mx.array(R.synth_audio(n, seed)))).astype(np.float32)
        assert f.shape == (2 * (n // 320) // 2, 160), f.shape
        feats.append(f)
        out[f"feat{i}_bf16"] = bf16_values(f).view(torch.int16).numpy().copy()          # the rounded features, exactly
        out[f"feat{i}_rows"] = kept_rows(f.shape[0], 10 ** 6, step=20).astype(np.int32)
        out[f"feat{i}"] = f[out[f"feat{i}_rows"]]                                        # before the rounding: for the front end's own check
    hyps, gaps = [], []
    for tag in "AB":
        d = R.config_dict(tag)
        cfg = G["config"].ModelConfig.from_dict(d)
        model = S.Model(cfg)
        w = make_granite_nar_weights(ModelConfig.from_dict(d), **R.WEIGHTS[tag])
        model.load_weights([(k, mx.array(v.numpy())) for k, v in w.items()], strict=True)
        model.eval()
        ctx = cfg.encoder.context_size
        meta["configs"][tag] = dict(cfg=d, weights=R.WEIGHTS[tag], decode=[])
        for i, f in enumerate(feats):
            r = run_clip(G, model, bf16_values(f).to(torch.float32).numpy())
            T = f.shape[0]
            rows = kept_rows(T, ctx)
            out[f"{tag}{i}_rows"] = rows.astype(np.int32)
            for k, v in r.items():
                frame = k in FRAME_STAGES or k.startswith("attn") or k.startswith("block")
                out[f"{tag}{i}_{k}"] = np.asarray(v)[rows] if frame else np.asarray(v)
            meta["configs"][tag]["decode"].append(dict(hyp=r["hyp"].tolist(), text_ids=r["text_ids"].tolist(), final=r["final"].tolist()))
            hyps.append(r["hyp"])
            gaps += [r["bpe_gap"], r["edit_gap"]]
            print(tag, i, T, "frames; hyp", r["hyp"].tolist(), "-> final", r["final"].tolist(), "min gaps", float(r["bpe_gap"].min()), float(r["edit_gap"].min()))
            meta["configs"][tag].setdefault("bpe_ids", []).append(r["bpe_ids"].tolist())
    gap = np.concatenate(gaps)
    assert gap.min() >= _margin.THR, f"a decision of the stored runs has a top-2 gap of {gap.min()} < {_margin.THR}: choose another seed"
    assert any(len(h) == 0 for h in hyps), "no empty hypothesis in the stored runs"
    assert any(2 * len(h) + 1 > 8 for h in hyps), "no hypothesis with 2 N + 1 > min_len"
    repeat = any(bool(((np.asarray(b)[1:] == np.asarray(b)[:-1]) & (np.asarray(b)[1:] != R.BLANK)).any())
                 for c in meta["configs"].values() for b in c["bpe_ids"] if len(b) > 1)
    assert repeat, "no adjacent repeats that collapse"
    path = os.path.join(HERE, "ref_granite_nar.npz")
    np.savez_compressed(path, **out)
    with open(os.path.join(HERE, "ref_granite_nar.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= 1_000_000


if __name__ == "__main__":
    main()
