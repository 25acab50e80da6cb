#!/usr/bin/env python
"""Runs the reference's OWN ``vad/models/sortformer/sortformer.py`` and ``config.py``, unmodified and imported from where they lie, over the numpy
stand-in for MLX (``mlx_shim.py``, left as it is) on seeded checkpoints and stores what they compute in ``tests/golden/ref_sortformer.npz`` / ``.json``.

The stand-in lacks ``nn.Conv2d`` (taken from ``make_parakeet_fixtures.py``, which adds it at run time); ``mlx_audio.base`` is the reference's own
file; ``mlx_audio.audio_io`` gets an empty stand-in (no file is read: every waveform is an array).

The reference is run on ONE un-padded clip per call.

  * config ``A``: FC 16 mels, d 128, 2 heads, 2 layers, K 9, 32 conv channels; TF d 48, 2 heads (dh 24), 2 layers, FFN 96, 256 positions, 4 speakers;
    features of 1601, 203, 41 and 9 frames;
  * config ``B``: TF d 64, 8 heads (dh 8), ``k_proj_bias``; FC ``attention_bias=False``; 203 and 64 frames;
  * per clip: ``encoder_proj``'s output, every TF layer's output, the pre-sigmoid logits, ``preds``, the segments of ``_preds_to_segments`` at the two
    settings of ``_sortformer_ref.SEGMENT_SETTINGS``;
  * one waveform through ``generate`` (segments, trim offset) and a ``feed`` sequence of 8 chunks with ``spkcache_max = fifo_max = 16``: per step the
    chunk preds, the state lengths, ``frames_processed``, the indices the compression kept and the gap between the last kept and the first dropped
    frame score;
  * scripted rows for ``_preds_to_segments`` (empty, touching segments, a merge across a gap, a min_duration drop), ``_trim_silence`` and ``sanitize``.
The inputs are NOT stored: they are regenerated from their seeds; the file holds each one's float64 sum and sum of squares.

Asserted before anything is written: at most 2 % of all (frame, speaker) logits have |z| < ``tests/_margin.THR``; between 20 % and 80 % of the
decisions are active; every speaker has a segment in at least one clip; every compression's kept / dropped gap exceeds ``_margin.THR``; the
compression ran at least twice.

Only runs where the reference lies: ``python tests/golden/make_sortformer_fixtures.py``."""
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_parakeet_fixtures as MP  # noqa: E402  (installs the stand-in, adds nn.Conv2d)
import _margin  # noqa: E402
import _sortformer_ref as R  # noqa: E402

M = MP.M
mx, nn, _np = M.mx, M.nn, M._np


def load_reference():
    M.import_reference()
    M._load("mlx_audio.base", f"{M.REF}/base.py")
    if "mlx_audio.audio_io" not in sys.modules:
        mod = types.ModuleType("mlx_audio.audio_io")
        mod.read = None
        sys.modules["mlx_audio.audio_io"] = mod
    for pkg, path in (("mlx_audio.vad", "vad"), ("mlx_audio.vad.models", "vad/models"), ("mlx_audio.vad.models.sortformer", "vad/models/sortformer")):
        if pkg not in sys.modules:
            M._pkg(pkg, f"{M.REF}/{path}")
    base = f"{M.REF}/vad/models/sortformer"
    cfg = M._load("mlx_audio.vad.models.sortformer.config", f"{base}/config.py")
    return cfg, M._load("mlx_audio.vad.models.sortformer.sortformer", f"{base}/sortformer.py")


def build(cfg_mod, S, c):
    from mlx_audio_amd.vad.models.sortformer import make_sortformer_weights

    model = S.Model(cfg_mod.ModelConfig.from_dict(R.config_dict(c["fc"], c["tf"])))
    ours = R.make_config(c["fc"], c["tf"])
    w = make_sortformer_weights(ours, c["seed_w"], head_gain=c["head_gain"], head_bias=c["head_bias"])
    model.load_weights([(k, mx.array(v.numpy())) for k, v in w.items()], strict=True)
    missing, unexpected, mism = model._load_report
    assert not missing and not unexpected and not mism, (missing, unexpected, mism)
    model.eval()
    return model, ours, w


def run_clip(S, model, feats):
    """The reference on ONE un-padded clip, features [n_mels, T]: ``Model.__call__`` stepped through its own modules so that intermediate tensors can be
    kept, checked against the module's own call."""
    x = mx.array(feats[None])
    length = mx.array(np.array([feats.shape[1]], dtype=np.int32))
    preds = _np(model(mx.array(feats[None].copy()), length)).copy()[0]
    emb, emb_len = model.fc_encoder(x, length)
    emb = mx.transpose(emb, axes=(0, 2, 1))
    proj = model.sortformer_modules.encoder_proj(emb)
    T = proj.shape[1]
    mask = S.SortformerModules.length_to_mask(emb_len, T)
    tf = model.tf_encoder
    y = proj + tf.embed_positions(mx.arange(T))
    attn_mask = (~mask)[:, None, None, :].astype(proj.dtype) * -1e4
    layers = []
    for layer in tf.layers:
        y = layer(y, mask=attn_mask)
        layers.append(_np(y).copy()[0])
    assert np.array_equal(layers[-1], _np(tf(encoder_states=proj, encoder_mask=mask))[0]), "the stepped encoder is not the module's own call"
    mods = model.sortformer_modules
    h = nn.relu(mods.first_hidden_to_hidden(nn.relu(y)))
    logits = _np(mods.single_hidden_to_spks(h)).copy()[0]
    assert np.array_equal(_np(mx.sigmoid(mx.array(logits))), preds), "the stepped head is not the module's own call"
    out = dict(encoder_proj=_np(proj).copy()[0], layers=np.stack(layers), logits=logits, preds=preds, out_len=int(np.asarray(emb_len)[0]))
    assert out["out_len"] == T == preds.shape[0]
    segs = [R.segments_list(model._preds_to_segments(mx.array(preds), frame_duration=0.08, threshold=t, min_duration=d, merge_gap=g))
            for t, d, g in R.SEGMENT_SETTINGS]
    return out, segs


def run_stream(S, model):
    """``feed`` over the chunks of one seeded waveform; the reference's ``_compress_spkcache_simple`` wrapped to keep what it decided."""
    k = R.STREAM
    wave = R.synth_wave(k["seed"], k["chunks"] * k["chunk_samples"])
    kept = []
    orig = S.Model._compress_spkcache_simple

    def spy(embs, preds, target_len):
        scores = np.log(np.clip(np.asarray(preds[0], dtype=np.float32), np.float32(1e-7), np.float32(1.0))).sum(-1)
        order = np.argsort(-scores, kind="stable")
        idx = np.sort(order[:target_len])
        ce, cp = orig(embs, preds, target_len)
        assert np.array_equal(_np(ce), _np(embs)[:, idx, :]) and np.array_equal(_np(cp), _np(preds)[:, idx, :]), "the spy's indices are not the reference's"
        kept.append(dict(indices=[int(i) for i in idx], n=int(len(scores)), gap=float(scores[order[target_len - 1]] - scores[order[target_len]])))
        return ce, cp

    S.Model._compress_spkcache_simple = staticmethod(spy)
    try:
        state = model.init_streaming_state()
        steps, preds = [], {}
        for i in range(k["chunks"]):
            n0 = len(kept)
            chunk = wave[i * k["chunk_samples"]:(i + 1) * k["chunk_samples"]]
            res, state = model.feed(chunk, state, spkcache_max=k["spkcache_max"], fifo_max=k["fifo_max"])
            preds[f"stream_preds{i}"] = _np(res.speaker_probs).copy()
            steps.append(dict(spkcache_len=int(state.spkcache_len), fifo_len=int(state.fifo_len), frames_processed=int(state.frames_processed),
                              segments=R.segments_list(res.segments), compress=kept[n0:]))
    finally:
        S.Model._compress_spkcache_simple = staticmethod(orig)
    return wave, steps, preds, kept


def scripted(S, model):
    P = lambda rows: mx.array(np.array(rows, dtype=np.float32))
    on, off = 0.9, 0.1
    rows = dict(empty=[[off, off]] * 5,
                touching=[[on, off], [on, off], [off, on], [off, on], [on, off], [off, off]],
                merge_gap=[[on, off], [off, off], [on, off], [off, off], [off, off], [off, off], [on, on]],
                min_duration=[[on, off], [off, off], [on, on], [on, on], [on, off], [off, off]],
                whole=[[on, on]] * 4,
                at_threshold=[[0.5, 0.5000001], [0.6, 0.4]])
    settings = ((0.5, 0.0, 0.0), (0.5, 0.1, 0.0), (0.5, 0.0, 0.1), (0.5, 0.15, 0.25))
    out = dict(segments={name: dict(preds=r, results=[R.segments_list(model._preds_to_segments(P(r), frame_duration=0.08, threshold=t, min_duration=d,
                                                                                                merge_gap=g)) for t, d, g in settings])
                         for name, r in rows.items()}, settings=[list(s) for s in settings])
    # _trim_silence: (leading zeros, speech, trailing zeros) in samples at 16 kHz, plus a burst shorter than min_speech_sec in front
    trims = []
    for lead, speech, trail, burst in ((8000, 24000, 8000, 0), (0, 32000, 0, 0), (16000, 16000, 0, 0), (4000, 4000, 4000, 0), (12000, 20000, 9000, 2400),
                                       (100, 300, 100, 0)):
        w = np.zeros(lead + speech + trail, dtype=np.float32)
        w[lead:lead + speech] = 0.5 * np.sin(np.arange(speech, dtype=np.float32) * 0.3)
        if burst:
            w[1000:1000 + burst] = 0.5
        tw, off_s = model._trim_silence(mx.array(w), 16000)
        trims.append(dict(lead=lead, speech=speech, trail=trail, burst=burst, offset=int(off_s), length=int(tw.shape[0])))
    out["trim"] = trims
    # sanitize: HuggingFace names with PyTorch layouts, and an already converted checkpoint
    g = np.random.default_rng(5)
    hf = {"fc_encoder.subsampling.layers.0.weight": g.standard_normal((4, 1, 3, 3)).astype(np.float32),
          "fc_encoder.subsampling.layers.2.weight": g.standard_normal((4, 1, 3, 3)).astype(np.float32),
          "fc_encoder.subsampling.layers.0.bias": g.standard_normal((4,)).astype(np.float32),
          "fc_encoder.subsampling.linear.weight": g.standard_normal((6, 8)).astype(np.float32),
          "fc_encoder.layers.0.conv.pointwise_conv1.weight": g.standard_normal((8, 4, 1)).astype(np.float32),
          "fc_encoder.layers.0.conv.depthwise_conv.weight": g.standard_normal((4, 1, 9)).astype(np.float32),
          "fc_encoder.layers.0.conv.norm.num_batches_tracked": np.zeros((), dtype=np.float32),
          "fc_encoder.layers.0.conv.norm.running_mean": g.standard_normal((4,)).astype(np.float32),
          "tf_encoder.layers.0.fc1.weight": g.standard_normal((6, 4)).astype(np.float32)}
    conv = {"fc_encoder.subsampling.layers_0.weight": g.standard_normal((4, 3, 3, 1)).astype(np.float32),
            "fc_encoder.layers.0.conv.depthwise_conv.weight": g.standard_normal((4, 9, 1)).astype(np.float32)}
    out["sanitize"] = {}
    for tag, wts in (("hf", hf), ("converted", conv)):
        res = S.Model.sanitize({k: mx.array(v) for k, v in wts.items()})
        out["sanitize"][tag] = {k: dict(shape=list(v.shape), sum=float(np.asarray(v, dtype=np.float64).sum()),
                                        first=float(np.asarray(v).reshape(-1)[min(5, np.asarray(v).size - 1)])) for k, v in res.items()}
    return out


def main():
    cfg_mod, S = load_reference()
    out, meta = {}, dict(configs={}, segment_settings=[list(s) for s in R.SEGMENT_SETTINGS])
    all_logits, spk_seen, first = [], set(), None
    for tag, c in R.CONFIGS.items():
        model, ours, _ = build(cfg_mod, S, c)
        first = first or model
        meta["configs"][tag] = dict(fc=c["fc"], tf=c["tf"], seed_w=c["seed_w"], head_gain=c["head_gain"], head_bias=c["head_bias"],
                                    clips=[list(x) for x in c["clips"]], segments=[])
        for i, (frames, seed) in enumerate(c["clips"]):
            feats = np.ascontiguousarray(R.synth_mel(seed, c["fc"]["num_mel_bins"], frames).T)
            out[f"{tag}{i}_featsum"] = np.array([feats.astype(np.float64).sum(), (feats.astype(np.float64) ** 2).sum()])
            r, segs = run_clip(S, model, feats)
            for k, v in r.items():
                out[f"{tag}{i}_{k}"] = np.asarray(v)
            meta["configs"][tag]["segments"].append(segs)
            all_logits.append(r["logits"].reshape(-1))
            spk_seen |= {s[2] for s in segs[0]}
            print(tag, i, frames, "->", r["out_len"], "frames;", len(segs[0]), "segments; active", float((r["preds"] > 0.5).mean()))
    # generate + the feed sequence on config A
    model = first
    k = R.GENERATE
    wave = R.synth_wave(k["seed"], int(k["seconds"] * 16000))
    wave[:12000] *= 1e-4   # leading near-silence: the trim takes it
    res = model.generate(mx.array(wave))
    probs = _np(res.speaker_probs)
    out["generate_wavesum"] = np.array([wave.astype(np.float64).sum(), (wave.astype(np.float64) ** 2).sum()])
    out["generate_preds"] = probs.copy()
    _, trim = model._trim_silence(mx.array(wave), 16000)
    meta["generate"] = dict(segments=R.segments_list(res.segments), trim_offset=int(trim), num_speakers=int(res.num_speakers), text=res.text)
    assert trim > 0
    swave, steps, spreds, kept = run_stream(S, model)
    out["stream_wavesum"] = np.array([swave.astype(np.float64).sum(), (swave.astype(np.float64) ** 2).sum()])
    out.update(spreds)
    meta["stream"] = dict(steps=steps, **R.STREAM)
    meta["scripted"] = scripted(S, model)

    z = np.concatenate(all_logits)
    knife, active = float((np.abs(z) < _margin.THR).mean()), float((z > 0).mean())
    print("decisions", len(z), "|z| <", _margin.THR, ":", knife, " active:", active, " speakers with a segment:", sorted(spk_seen), " compressions:", len(kept),
          " smallest kept / dropped gap:", min(c["gap"] for c in kept))
    assert len(z) >= 400 and knife <= 0.02, knife
    assert 0.2 <= active <= 0.8, active
    assert spk_seen == set(range(4)), spk_seen
    assert len(kept) >= 2 and all(c["gap"] > _margin.THR for c in kept), kept
    path = os.path.join(HERE, "ref_sortformer.npz")
    np.savez_compressed(path, **out)
    with open(os.path.join(HERE, "ref_sortformer.json"), "w") as f:
        json.dump(meta, f, ensure_ascii=False, indent=1)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= 550_000


if __name__ == "__main__":
    main()
