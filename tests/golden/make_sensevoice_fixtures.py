#!/usr/bin/env python
"""Runs the reference's OWN ``stt/models/sensevoice/sensevoice.py`` and ``config.py``, unmodified and imported from where they lie, over the numpy
stand-in for MLX (``mlx_shim.py``, left as it is) on seeded checkpoints and stores what they compute in ``tests/golden/ref_sensevoice.npz`` / ``.json``.

``sensevoice.py`` imports ``mlx_audio.stt.utils`` (the audio loader, the hub client behind it) at module level; it is not on the path taken here and
gets an empty stand-in module, as in the Parakeet maker.  ``mlx_audio.dsp`` and ``stt/models/base.py`` are the reference's own files.

  * config ``A``: 80 mels, LFR 7 / 6 (input 560), width 128, 2 heads (64), FFN 256, 3 + 2 layers, K 5, vocabulary 100, no CMVN;
  * config ``B``: 40 mels, LFR 5 / 3 (input 200), width 256, 2 heads (128), FFN 512, 2 + 1 layers, K 11, ``sanm_shfit`` 2, vocabulary 300, CMVN from a
    written ``am.mvn``;
  * clips of 1, 5, 6, 7, 13 and 300 fbank frames (one frame is exactly 400 samples), language ``en``, ``use_itn=True``;
  * per clip: the assembled encoder input (behind the scale and the position term), every layer's output (on the rows ``layer_rows``: all of them, or
    for the 300-frame clips every second row and the last, to keep the file under 1 MiB), layer 0's attention-module output, the encoder's output, the frame arg-max ids, the float32 top-2 gaps, the rich-info triple, the token ids and the text through a ``tokens.json``, and
    ``generate``'s segment;
  * ``_apply_lfr`` on the ``arange`` input of the reference's own ``test_left_padding``.
The audio is NOT stored: it is regenerated from its seeds (``tests/_sensevoice_ref.synth_audio``); the file holds each clip's float64 sum and sum of
squares.  The ``ctc_lo`` bias of the blank is raised so that the ids hold repeats, blanks and an ``a, blank, a`` pattern.

Asserted before anything is written, on the reference alone: at most 2 % of all frames have a top-2 gap below ``tests/_margin.THR``; between 20 % and
80 % of the frames are blank; the ids hold a repeat of a non-blank id and an ``a, blank ..., a`` pattern; the stepped encoder equals the module's own
call.

Only runs where the reference lies: ``python tests/golden/make_sensevoice_fixtures.py``."""
import json
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_reference_fixtures as M  # noqa: E402  (installs the stand-in)
import _margin  # noqa: E402
import _sensevoice_ref as R  # noqa: E402

mx, nn, _np = M.mx, M.nn, M._np


def load_reference():
    M.import_reference()
    for pkg, path in (("mlx_audio.stt", "stt"), ("mlx_audio.stt.models", "stt/models"), ("mlx_audio.stt.models.sensevoice", "stt/models/sensevoice")):
        if pkg not in sys.modules:
            M._pkg(pkg, f"{M.REF}/{path}")
    if "mlx_audio.stt.utils" not in sys.modules:
        mod = types.ModuleType("mlx_audio.stt.utils")
        mod.load_audio = None
        sys.modules["mlx_audio.stt.utils"] = mod
    M._load("mlx_audio.stt.models.base", f"{M.REF}/stt/models/base.py")
    cfg = M._load("mlx_audio.stt.models.sensevoice.config", f"{M.REF}/stt/models/sensevoice/config.py")
    sv = M._load("mlx_audio.stt.models.sensevoice.sensevoice", f"{M.REF}/stt/models/sensevoice/sensevoice.py")
    return cfg, sv


def build(C, S, c, workdir):
    from mlx_audio_amd.stt.models.sensevoice import make_sensevoice_weights

    d = dict(c["cfg"], encoder_conf=dict(c["cfg"]["encoder_conf"]), frontend_conf=dict(c["cfg"]["frontend_conf"]))
    config = C.ModelConfig.from_dict(d)
    assert config.encoder_conf.sanm_shift == c["cfg"]["encoder_conf"].get("sanm_shfit", 0)
    model = S.SenseVoiceSmall(config)
    w = make_sensevoice_weights(R.make_config(c["cfg"]), c["seed_w"], head_gain=R.HEAD_GAIN, blank_bias=c["blank_bias"])
    model.load_weights([(k, mx.array(v.numpy())) for k, v in w.items()], strict=True)
    missing, unexpected, mism = model._load_report
    assert not missing and not unexpected and not mism, (missing, unexpected, mism)
    model.eval()
    os.makedirs(workdir, exist_ok=True)
    if c["cmvn_seed"] is not None:
        with open(os.path.join(workdir, "am.mvn"), "w") as f:
            f.write(R.am_mvn_text(*R.make_cmvn(c["cmvn_seed"], config.input_size)))
    with open(os.path.join(workdir, "tokens.json"), "w") as f:
        json.dump(R.token_list(config.vocab_size), f, ensure_ascii=False)
    S.SenseVoiceSmall.post_load_hook(model, workdir)
    assert (model._cmvn_means is not None) == (c["cmvn_seed"] is not None) and model._token_list is not None and model._tokenizer is None
    return model


def run_clip(model, audio):
    """The reference on ONE clip: ``_extract_features`` and ``__call__`` stepped through the encoder's own modules so that intermediate tensors can be
    kept, checked against the module's own call; then ``generate``."""
    enc = model.encoder
    feats = model._extract_features(mx.array(audio))
    textnorm_query, input_query = model._build_query(1, R.LANGUAGE, R.USE_ITN)
    speech = mx.concatenate([input_query, mx.concatenate([textnorm_query, feats[None, :, :]], axis=1)], axis=1)
    xs = enc.embed(speech * (enc._output_size**0.5))
    out = dict(x=_np(xs).copy()[0])
    layers = []
    stack = list(enc.encoders0) + list(enc.encoders)
    for i, layer in enumerate(stack + list(enc.tp_encoders)):
        if i == len(stack):
            xs = enc.after_norm(xs)
        if i == 0:
            out["attn0"] = _np(layer.self_attn(layer.norm1(mx.array(_np(xs).copy())))).copy()[0]
        xs = layer(mx.array(_np(xs).copy()))
        layers.append(_np(xs).copy()[0])
    if not enc.tp_encoders:
        xs = enc.after_norm(xs)
    hidden = _np(enc.tp_norm(xs)).copy()[0]
    assert np.array_equal(hidden, _np(enc(speech))[0]), "the stepped encoder is not the module's own call"
    logp = _np(model(feats[None, :, :], language=R.LANGUAGE, use_itn=R.USE_ITN)).astype(np.float32)[0]
    top = np.sort(logp, axis=-1)
    rows = np.arange(hidden.shape[0]) if hidden.shape[0] <= 32 else np.unique(np.r_[0:hidden.shape[0]:2, hidden.shape[0] - 1])   # file size
    out.update(layers=np.stack(layers)[:, rows], layer_rows=rows.astype(np.int32), hidden=hidden, ids=logp.argmax(-1).astype(np.int32), gap=(top[:, -1] - top[:, -2]).astype(np.float32))
    rich = model._extract_rich_info(mx.array(logp[:4]))
    token_ids, text = model._greedy_ctc_decode(mx.array(logp[4:]))
    res = model.generate(np.asarray(audio), language=R.LANGUAGE, use_itn=R.USE_ITN)
    assert res.text == text and res.language == rich["language"] and res.segments[0]["emotion"] == rich["emotion"]
    return out, dict(rich=rich, tokens=[int(t) for t in token_ids], text=text, segments=res.segments)


def aba(s, blank=0):
    last, seen_blank = None, False
    for t in s.tolist():
        if t == blank:
            seen_blank = last is not None
            continue
        if seen_blank and t == last:
            return True
        last, seen_blank = t, False
    return False


def main():
    C, S = load_reference()
    out, meta = {}, dict(language=R.LANGUAGE, use_itn=R.USE_ITN, configs={})
    out["lfr_arange"] = _np(S._apply_lfr(mx.arange(20).reshape(20, 1).astype(mx.float32), lfr_m=7, lfr_n=6))
    all_ids, all_gap = [], []
    with tempfile.TemporaryDirectory() as tmp:
        for tag, c in R.CONFIGS.items():
            model = build(C, S, c, os.path.join(tmp, tag))
            meta["configs"][tag] = dict(cfg=c["cfg"], seed_w=c["seed_w"], blank_bias=c["blank_bias"], clips=[list(x) for x in c["clips"]], decode=[])
            for i, (frames, seed) in enumerate(c["clips"]):
                audio = R.synth_audio(seed, frames)
                out[f"{tag}{i}_audiosum"] = np.array([audio.astype(np.float64).sum(), (audio.astype(np.float64) ** 2).sum()])
                r, dec = run_clip(model, audio)
                assert r["x"].shape[0] == 4 + -(-frames // c["cfg"]["frontend_conf"]["lfr_n"]), r["x"].shape
                for k, v in r.items():
                    out[f"{tag}{i}_{k}"] = np.asarray(v)
                meta["configs"][tag]["decode"].append(dec)
                all_ids.append(r["ids"][4:])
                all_gap.append(r["gap"])
                print(tag, i, frames, "->", r["x"].shape[0], "rows;", dec["rich"], dec["tokens"][:12], repr(dec["text"][:40]))
    ids, gap = np.concatenate(all_ids), np.concatenate(all_gap)
    share, blank_share = float((gap < _margin.THR).mean()), float((ids == 0).mean())
    repeat = any(bool(((s[1:] == s[:-1]) & (s[1:] != 0)).any()) for s in all_ids if len(s) > 1)
    print("frames", len(gap), "gap <", _margin.THR, ":", share, " blank share:", blank_share, " repeat:", repeat, " a-blank-a:", any(aba(s) for s in all_ids))
    assert share <= 0.02, share
    assert 0.2 <= blank_share <= 0.8, blank_share
    assert repeat and any(aba(s) for s in all_ids)
    path = os.path.join(HERE, "ref_sensevoice.npz")
    np.savez_compressed(path, **out)
    with open(os.path.join(HERE, "ref_sensevoice.json"), "w") as f:
        json.dump(meta, f, ensure_ascii=False, indent=1)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= 1_000_000


if __name__ == "__main__":
    main()
