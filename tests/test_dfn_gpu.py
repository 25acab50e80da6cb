"""DeepFilterNet on the device, waveform to waveform, against the reference's own runs (``tests/golden/ref_dfn.npz``) and against the float64 helper
``tests/_dfn_ref.py`` on longer clips.  Only the committed fixtures are read."""
import json
import os
import sys
import wave

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
GOLD = os.path.join(HERE, "golden")

import _dfn_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
STAGES = ("feat_erb", "feat_df", "emb", "m", "lsnr", "df_coefs")
BAR = 3e-4   # of each tensor's peak: the standing bar of test_parakeet_gpu.py / test_s3_gpu.py


def rel_peak(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


@pytest.fixture(scope="module")
def fx():
    with open(os.path.join(GOLD, "ref_dfn.json")) as f:
        meta = json.load(f)
    return np.load(os.path.join(GOLD, "ref_dfn.npz")), meta


@pytest.fixture(scope="module")
def engines(fx):
    from mlx_audio_amd.sts.models.deepfilternet import DeepFilterNetModel, config as C, make_dfn_weights

    _, meta = fx
    out = {}
    for tag, c in meta["configs"].items():
        cfg = getattr(C, c["cls"])(**c["kw"])
        w = make_dfn_weights(cfg, meta["seed_w"])
        clips = [R.synth_clip(seed, n, cfg.sample_rate, tuple(z) if z else None) for seed, n, z in c["clips"]]
        out[tag] = (cfg, w, clips, DeepFilterNetModel(cfg, weights=w, device="cuda:0"))
    return out


def _check(npz, meta, tag, i, y, st, row, T, worst):
    for k in STAGES:
        v = st[k][row, :T].cpu().numpy()
        if k == "df_coefs" and T > meta["coef_stride_above"]:
            v = v[::meta["coef_stride"]]
        want = npz[f"{tag}{i}_{k}"]
        d = rel_peak(v.reshape(want.shape), want)
        worst[k] = max(worst.get(k, 0.0), d)
        assert d < BAR, (tag, i, k, d)
    d = rel_peak(y, npz[f"{tag}{i}_wave"])
    worst["wave"] = max(worst.get("wave", 0.0), d)
    assert d < BAR, (tag, i, "wave", d)


@pytest.mark.parametrize("tag", ["A", "B"])
def test_fixture_parity_alone_and_batched(fx, engines, tag):
    """Every clip alone, then all clips of the config as ONE ``enhance_batch``: stage tensors and waveform within 3e-4 of each tensor's peak of the
    reference's float32 runs.  Measured on MI355X (largest distance / peak over both configs, alone and batched): feat_erb 1.4e-6, feat_df 1.6e-7,
    emb 7.1e-7, m 2.4e-7, lsnr 8.0e-7, df_coefs 4.2e-7, waveform 4.4e-7."""
    npz, meta = fx
    cfg, _, clips, eng = engines[tag]
    frames = meta["configs"][tag]["frames"]
    worst = {}
    for i, x in enumerate(clips):
        y, st = eng.enhance_array(x, return_stages=True)
        assert st["frames"] == [frames[i]] and y.dtype == np.float32 and y.shape == x.shape
        _check(npz, meta, tag, i, y, st, 0, frames[i], worst)
    ys, st = eng.enhance_batch(clips, return_stages=True)
    assert st["frames"] == frames
    for i, x in enumerate(clips):
        assert ys[i].shape == x.shape and ys[i].dtype == np.float32
        _check(npz, meta, tag, i, ys[i], st, i, frames[i], worst)
        for k in ("feat_erb", "feat_df", "emb", "m", "df_coefs"):
            assert not st[k][i, frames[i]:].any(), (i, k)
    print(f"config {tag}: largest distance / peak", {k: f"{v:.2e}" for k, v in worst.items()})


def test_seeded_long_clips_against_the_float64_helper(engines):
    """Config A on seeded weights, a 3 s and a 1.5 s clip as one batch and alone, against ``_dfn_ref.enhance``: same bar.
    Measured on MI355X: waveform 3.8e-7 (3 s) and 3.7e-7 (1.5 s), emb 6.8e-7 and 9.6e-7 of peak."""
    cfg, w, _, eng = engines["A"]
    wn = {k: v.numpy() for k, v in w.items()}
    clips = [R.synth_clip(31, 144000), R.synth_clip(32, 72000, zero_span=(30000, 36000))]
    refs = [R.enhance(cfg, wn, x) for x in clips]
    ys, st = eng.enhance_batch(clips, return_stages=True)
    assert st["frames"] == [302, 152]
    for i, (yr, sr) in enumerate(refs):
        T = st["frames"][i]
        d = {k: rel_peak(st[k][i, :T].cpu().numpy().reshape(sr[k].shape), sr[k]) for k in ("emb", "m", "df_coefs")}
        d["wave"] = rel_peak(ys[i], yr)
        print(f"{len(clips[i]) / 48000:.1f} s clip: distance / peak", {k: f"{v:.2e}" for k, v in d.items()})
        assert max(d.values()) < BAR, d
        assert 1e-3 < float(np.abs(yr).max()) < 0.9
    alone = eng.enhance_array(clips[1])
    assert rel_peak(alone, refs[1][0]) < BAR and rel_peak(alone, ys[1]) < BAR


def test_two_calls_are_bitwise_equal(engines):
    _, _, clips, eng = engines["A"]
    a, b = eng.enhance_batch(clips[:3]), eng.enhance_batch(clips[:3])
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert np.array_equal(eng.enhance_array(clips[0]), eng.enhance_array(clips[0]))


def test_enhance_file_round_trip_and_wrong_rate(engines, tmp_path):
    from mlx_audio_amd import audio_io

    _, _, clips, eng = engines["A"]
    src, dst = tmp_path / "in.wav", tmp_path / "out.wav"
    audio_io.write(str(src), clips[0], 48000)
    assert eng.enhance_file(src, dst) == dst
    got, sr = audio_io.read(str(dst), dtype="float32")
    back, _ = audio_io.read(str(src), dtype="float32")                          # the 16-bit PCM the engine was given
    want = eng.enhance_array(back)
    assert sr == 48000 and got.shape == want.shape == clips[0].shape and got.dtype == np.float32
    again = tmp_path / "want.wav"
    audio_io.write(str(again), want, 48000)
    assert np.array_equal(got, audio_io.read(str(again), dtype="float32")[0])   # the same samples through the same 16-bit writer
    assert float(np.abs(got - want).max()) <= 2.0 / 32767   # one step of the 16-bit writer plus the writer / reader scale difference (|v| / 32768)
    with wave.open(str(dst)) as f:
        assert (f.getnchannels(), f.getframerate(), f.getnframes()) == (1, 48000, len(clips[0]))
    bad = tmp_path / "in16k.wav"
    audio_io.write(str(bad), clips[0], 16000)
    with pytest.raises(ValueError, match="Expected 48000 Hz audio, got 16000 Hz"):
        eng.enhance_file(bad, dst)
