"""Sortformer on the device against the reference's own runs (``tests/golden/ref_sortformer.npz`` / ``.json``: one un-padded clip per call) and against
itself (a padded batch against its items alone at the published widths, ``generate_stream`` against a manual ``streaming_step`` loop)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
GOLD = os.path.join(HERE, "golden")

import _margin  # noqa: E402
import _sortformer_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
THR_H = 3e-4   # of each tensor's peak: the bar of test_parakeet_gpu.py and test_s3_gpu.py
FAMILY = "sortformer"


def rel_peak(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLD, "ref_sortformer.npz"))


@pytest.fixture(scope="module")
def meta():
    with open(os.path.join(GOLD, "ref_sortformer.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def engines(meta):
    """tag -> (engine, [features [n_mels, T]])."""
    from mlx_audio_amd.vad.models.sortformer import Model

    return {tag: (Model(cfg, w), feats) for tag, (cfg, w, feats) in R.load_models(meta).items()}


def test_fixture_parity(fx, meta, engines):
    """Both configs, every clip alone and all clips of a config as one padded batch: ``encoder_proj``'s output, every Transformer layer's output, the
    logits and ``preds`` within 3e-4 of each tensor's peak on the valid frames; padded rows of ``preds`` exactly zero; the activity decisions
    ``preds > 0.5`` through the margin rule with |z| as the margin (at least 95 % of at least 400 compared); the segments equal for every clip with
    no decision under the threshold.
    Measured on MI355X: worst stage distance 1.5e-6 of the peak (preds; encoder_proj 7.0e-7, layers 6.3e-7, logits 1.3e-6); 2150 of 2152 decisions compared."""
    compared = total = 0
    worst = {}
    for tag, (eng, feats) in engines.items():
        batch, lens = R.pad_batch(feats)
        runs = [(eng(torch.from_numpy(f)[None], None, return_layers=True), 0, i, "alone") for i, f in enumerate(feats)]
        rb = eng(batch, lens, return_layers=True)
        runs += [(rb, i, i, "batch") for i in range(len(feats))]
        for (preds, taps), row, i, how in runs:
            n = int(fx[f"{tag}{i}_out_len"])
            got = dict(encoder_proj=taps["encoder_proj"][row, :n], layers=torch.stack(taps["layers"])[:, row, :n], logits=taps["logits"][row, :n],
                       preds=preds[row, :n])
            for k, v in got.items():
                e = rel_peak(v.cpu().numpy(), fx[f"{tag}{i}_{k}"])
                worst[k] = max(worst.get(k, 0.0), e)
                print(f"sortformer {tag}{i} {how} {k}: {e:.2e}")
                assert e < THR_H, (tag, i, how, k, e)
            assert preds.shape[1] >= n and not bool(preds[row, n:].any()), "padded rows of preds are not exactly zero"
            z = fx[f"{tag}{i}_logits"]
            compared += _margin.walk_resync(FAMILY, (got["preds"].cpu().numpy() > 0.5).reshape(-1), (fx[f"{tag}{i}_preds"] > 0.5).reshape(-1),
                                            np.abs(z).reshape(-1), where=(tag, i, how))
            total += z.size
            if (np.abs(z) < _margin.THR).any():
                continue
            for (t, d, g), want in zip(R.SEGMENT_SETTINGS, meta["configs"][tag]["segments"][i]):
                segs = eng._preds_to_segments(got["preds"], frame_duration=0.08, threshold=t, min_duration=d, merge_gap=g)
                assert R.same_segments(R.segments_list(segs), want), (tag, i, how, t)
    print(f"sortformer fixture parity: worst stage distances {({k: float(f'{v:.2e}') for k, v in worst.items()})}; {compared} of {total} decisions compared")
    assert total >= 400 and compared >= 0.95 * total, (compared, total)


def test_feed_sequence(fx, meta, engines, monkeypatch):
    """The fixture's 8 ``feed`` chunks with ``spkcache_max = fifo_max = 16`` (the device front end, the compression running five times): chunk preds
    within 3e-4 of the peak, state lengths, ``frames_processed`` and the indices every compression kept equal to the reference's.
    Measured on MI355X: worst chunk distance 3.1e-6 of the peak (the device log-mel front end in front of the model); 5 compressions."""
    from mlx_audio_amd.vad.models.sortformer import Model

    eng, _ = engines["A"]
    k = meta["stream"]
    wave = R.synth_wave(k["seed"], k["chunks"] * k["chunk_samples"])
    kept = []
    orig = Model._simple_keep_indices
    monkeypatch.setattr(Model, "_simple_keep_indices", staticmethod(lambda preds, n: kept.append(orig(preds, n)) or kept[-1]))
    state = eng.init_streaming_state()
    worst = 0.0
    for i, want in enumerate(k["steps"]):
        n0 = len(kept)
        res, state = eng.feed(wave[i * k["chunk_samples"]:(i + 1) * k["chunk_samples"]], state, spkcache_max=k["spkcache_max"], fifo_max=k["fifo_max"])
        e = rel_peak(res.speaker_probs.cpu().numpy(), fx[f"stream_preds{i}"])
        worst = max(worst, e)
        print(f"sortformer feed chunk {i}: {e:.2e}")
        assert e < THR_H, (i, e)
        assert (state.spkcache_len, state.fifo_len, state.frames_processed) == (want["spkcache_len"], want["fifo_len"], want["frames_processed"]), i
        assert [t.tolist() for t in kept[n0:]] == [c["indices"] for c in want["compress"]], i
    print(f"sortformer feed: worst chunk distance {worst:.2e}; {len(kept)} compressions")
    assert len(kept) >= 2


def test_generate_stream_file_mode_equals_a_manual_loop(engines):
    """``generate_stream`` on a whole waveform (features normalised over the whole audio, 1 s chunks, small buffers so that the cache compresses)
    against ``streaming_step`` + ``_maybe_compress_state`` called by hand on the same features: bitwise equal chunk preds, equal segments."""
    from mlx_audio_amd.vad.models.sortformer import extract_mel_features

    eng, _ = engines["A"]
    wave = torch.from_numpy(R.synth_wave(433, 5 * 16000))
    outs = list(eng.generate_stream(wave, chunk_duration=1.0, spkcache_max=16, fifo_max=16))
    w, trim = eng._trim_silence(wave, 16000)   # the tail behind the last whole 30 ms frame goes at least
    w = (1.0 / (w.abs().max() + 1e-3)) * w
    feats = extract_mel_features(w.to(eng.device), n_mels=16)
    state, off, manual = eng.init_streaming_state(), 0, []
    while off < feats.shape[2]:
        end = min(off + 96, feats.shape[2])   # round(1.0 * 16000 / 160 / 8) * 8 mel frames
        p, state = eng.streaming_step(feats[:, :, off:end], [end - off], state)
        manual.append((p, off))
        state = eng._maybe_compress_state(state, 16, 16, eng.config.modules_config)
        off = end
    assert len(outs) == len(manual) >= 5 and state.spkcache_len == 16
    for out, (p, off) in zip(outs, manual):
        assert torch.equal(out.speaker_probs, p)
        t0 = (off * 160) / 16000 + trim / 16000
        want = [[s.start + t0, s.end + t0, s.speaker] for s in eng._preds_to_segments(p, frame_duration=0.08)]
        assert R.same_segments(R.segments_list(out.segments), want)


@pytest.fixture(scope="module")
def wide():
    from mlx_audio_amd.vad.models.sortformer import Model, make_sortformer_weights

    cfg = R.make_config(R.FC_WIDE, R.TF_WIDE)
    eng = Model(cfg, make_sortformer_weights(cfg, 93, head_gain=6.0, head_bias=-3.0))
    feats = [np.ascontiguousarray(R.synth_mel(440 + i, 80, frames).T) for i, frames in enumerate((801, 200, 517, 1040))]   # 2 - 10 s
    return eng, feats


def test_padded_batch_equals_items_alone_at_published_widths(wide):
    """FC d 512 / 8 heads of 64 / K 9 / 80 mels / 256 conv channels and TF d 192 / 8 heads of 24 / FFN 768, two layers each, four clips of 2 - 10 s on
    seeded weights: ``preds`` and the logits of the padded batch within 3e-4 of the peak of each item run alone, the decisions by the margin rule
    (|z| taken from the item's own run).
    Measured on MI355X: worst distance 2.1e-6; 1284 of 1284 decisions compared."""
    eng, feats = wide
    batch, lens = R.pad_batch(feats)
    pb, tb = eng(batch, lens, return_layers=True)
    worst, compared, total = 0.0, 0, 0
    for i, f in enumerate(feats):
        p1, t1 = eng(torch.from_numpy(f)[None], None, return_layers=True)
        n = p1.shape[1]
        assert n == eng.fc_encoder.out_lengths([f.shape[1]])[0] and not bool(pb[i, n:].any())
        for a, b in ((pb[i, :n], p1[0]), (tb["logits"][i, :n], t1["logits"][0])):
            e = rel_peak(a.cpu().numpy(), b.cpu().numpy())
            worst = max(worst, e)
            assert e < THR_H, (i, e)
        z = t1["logits"][0].abs().cpu().numpy().reshape(-1)
        compared += _margin.walk_resync(FAMILY, (pb[i, :n] > 0.5).cpu().numpy().reshape(-1), (p1[0] > 0.5).cpu().numpy().reshape(-1), z, where=("wide", i))
        total += z.size
    print(f"sortformer wide batch vs alone: worst distance {worst:.2e}; {compared} of {total} decisions compared")
    assert compared >= 0.95 * total


def test_two_calls_are_bitwise_equal(engines, wide):
    for eng, feats in list(engines.values()) + [wide]:
        batch, lens = R.pad_batch(feats[-2:])
        p1 = eng(batch, lens).clone()
        assert torch.equal(p1, eng(batch, lens))


def test_generate_on_a_waveform(engines, fx, meta):
    """``generate`` on a seeded 6 s waveform whose first 0.75 s is near-silent: a ``DiarizationOutput`` equal to ``__call__`` + ``_preds_to_segments``
    on the same features, the trim offset and the probabilities (within 3e-4 of the peak) the reference's; the segments the reference's when no
    decision of its run is under the margin.
    Measured on MI355X: preds distance 2.3e-6."""
    from mlx_audio_amd.vad.models.sortformer import DiarizationOutput, extract_mel_features

    eng, _ = engines["A"]
    k = R.GENERATE
    wave = R.synth_wave(k["seed"], int(k["seconds"] * 16000))
    wave[:12000] *= 1e-4
    res = eng.generate(wave)
    assert isinstance(res, DiarizationOutput) and res.text.startswith("SPEAKER audio 1 ")
    w, off = eng._trim_silence(torch.from_numpy(wave), 16000)
    assert off == meta["generate"]["trim_offset"] == 12000
    w = (1.0 / (w.abs().max() + 1e-3)) * w
    feats = extract_mel_features(w.to(eng.device), n_mels=16)
    preds = eng(feats, [feats.shape[2]])
    assert torch.equal(res.speaker_probs, preds[0])
    want = [[s.start + off / 16000, s.end + off / 16000, s.speaker] for s in eng._preds_to_segments(preds[0], frame_duration=0.08)]
    assert R.same_segments(R.segments_list(res.segments), want) and res.num_speakers == len({s[2] for s in want})
    ref = fx["generate_preds"]
    e = rel_peak(res.speaker_probs.cpu().numpy(), ref)
    print(f"sortformer generate: preds distance {e:.2e}")
    assert e < THR_H
    zmin = float(np.abs(np.log(ref / (1.0 - ref))).min())   # |z| of the reference's own decisions
    if zmin >= 10 * _margin.THR:   # the front end's own distance (up to 5e-4 of the features) sits in front of these logits
        assert R.same_segments(R.segments_list(res.segments), meta["generate"]["segments"])
