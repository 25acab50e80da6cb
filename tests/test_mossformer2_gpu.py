"""MossFormer2 SE on the device, waveform to waveform: first against the reference's OWN runs (``tests/golden/ref_mossformer2.npz`` / ``.json``, made by
``tests/golden/make_mossformer2_fixtures.py`` with Kaldi's dither on and its draws seeded) -- features, layer 0's FLASH and Gated-FSMN outputs, mask and
waveform of every call, and ``enhance`` through the segmented and the chunked path --, then against the float64 restatement of the reference's module tree (``tests/_mossformer2_ref.py``)
fed with the engine's own Kaldi features, and a float64 STFT -> mask -> iSTFT back end stated here.  Config A is width 64, 2 blocks, the real front end
and the 961 mask columns; frame counts 1, 2, 58, 256, 257 and 300 give one row, the token shift's first row, one exactly full group and one group
of a single row.  Bars: 3e-4 of each tensor's peak against the float64 reference (the project's bar for a precision-4 chain), 1e-5 of the peak
wherever only the launch shapes differ."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import _mossformer2_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
BAR = 3e-4
BATCH = 1e-5
FRAMES = [1, 2, 58, 256, 257, 300]
WIN, HOP = 1920, 384


GOLD = os.path.join(HERE, "golden")


@pytest.fixture(scope="module")
def fx():
    import json

    with open(os.path.join(GOLD, "ref_mossformer2.json")) as f:
        meta = json.load(f)
    return np.load(os.path.join(GOLD, "ref_mossformer2.npz")), meta


def _engine(meta, tag, extra=None):
    from mlx_audio_amd.sts.models.mossformer2_se import MossFormer2SEConfig, MossFormer2SEModel, make_mossformer2_weights

    c = meta["configs"][tag]
    cfg = MossFormer2SEConfig.from_dict({**c["kw"], **(extra or {})})
    return MossFormer2SEModel(cfg, weights=make_mossformer2_weights(cfg, c["seed_w"]), device="cuda:0", dither=1.0)


def _clip(npz, key, seed, n):
    clip = R.synth_clip(seed, n)
    d = clip.astype(np.float64)
    assert np.allclose([d.sum(), (d ** 2).sum()], npz[key], rtol=1e-12, atol=1e-12), "the seeded clip is not the fixture's clip"
    return clip


@pytest.mark.parametrize("tag", ["A", "B"])
def test_fixture_parity_stage_by_stage(fx, tag):
    """Every call of the reference's own run, dither on with the same draws: the assembled 180-column features, layer 0's FLASH output and Gated-FSMN
    output, the mask and the waveform within 3e-4 of each tensor's peak (stored tensors are subsampled as the fixture's .json says).
    Measured on MI355X (largest distance / peak, config A / B): features 1.5e-6 / 7.7e-7, FLASH 3.1e-6 / 7.5e-6, Gated-FSMN 4.8e-6 / 6.7e-6, mask 2.7e-6 / 1.7e-6,
    waveform 1.8e-6 / 2.5e-6."""
    npz, meta = fx
    eng = _engine(meta, tag)
    S, SA, MC, WS, FF = meta["stride"], meta["stride_above"], meta["mask_col_stride"], meta["wave_stride"], meta["feat_full"]
    worst = {}
    for i, (seed, frames) in enumerate(meta["configs"][tag]["calls"]):
        clip = _clip(npz, f"{tag}{i}_clipsum", seed, samples(frames))
        eng.noise_rng = np.random.default_rng(meta["noise_seed"] + seed)
        outs, st = eng.enhance_batch([clip], return_stages=True)
        assert st["frames"] == [frames] and outs[0].shape == clip.shape
        sub = lambda v: v[::S] if frames > SA else v
        got = dict(feats=st["feats"][0].cpu().numpy() if frames <= FF else sub(st["feats"][0].cpu().numpy()),
                   flash0=sub(st["flash0"][0].cpu().numpy()), fsmn0=sub(st["fsmn0"][0].cpu().numpy()),
                   mask=sub(st["mask"][0].cpu().numpy())[:, ::MC] if frames > SA else st["mask"][0].cpu().numpy(),
                   wave=outs[0][::WS] if frames > SA else outs[0])
        for k, v in got.items():
            ref = npz[f"{tag}{i}_{k}"]
            assert v.shape == ref.shape, (k, v.shape, ref.shape)
            d = rel_peak(v, ref)
            worst[k] = max(worst.get(k, 0.0), d)
            print(f"config {tag} call {i} ({frames} frames) {k}: distance / peak {d:.2e}")
            assert d < BAR, (tag, i, k, d)
    print(f"config {tag}: largest distance / peak", {k: f"{v:.2e}" for k, v in worst.items()})


def test_both_long_audio_paths_against_the_reference_enhance(fx):
    """``enhance`` through the segmented path of ``_decode_one_audio`` and through ``_decode_chunked`` (picked by the auto threshold), decode lengths
    scaled down as the fixture's .json says, against the reference's own ``enhance`` output on the same clip and the same dither draws.
    Measured on MI355X: segmented 2.7e-6, chunked 3.8e-6 of the peak."""
    npz, meta = fx
    eng = _engine(meta, "A", meta["long"]["config"])
    seed, n = meta["long"]["clip"]
    clip = _clip(npz, "long_clipsum", seed, n)
    for key, chunked in (("long_segmented", False), ("long_chunked", None)):
        eng.noise_rng = np.random.default_rng(meta["noise_seed"] + seed)
        got = eng.enhance(clip, chunked=chunked)
        assert got.shape == clip.shape
        d = rel_peak(got[::meta["wave_stride"]], npz[key])
        print(f"{key}: distance / peak {d:.2e}")
        assert d < BAR, (key, d)


def rel_peak(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def samples(frames):
    return WIN + (frames - 1) * HOP


def backend64(x, mask):
    """x [L] float32 clip (already * 32768), mask [T, 961] float64 -> float64 samples: Hamming STFT without centring, the mask on both planes, the
    windowed inverse overlap-added and divided by the overlap-added squared window (model.py:405-436, dsp.py:612-752)."""
    n = np.arange(WIN)
    w = (0.54 - 0.46 * np.cos(2 * np.pi * n / (WIN - 1))).astype(np.float32).astype(np.float64)
    T = mask.shape[0]
    fr = np.stack([x[t * HOP:t * HOP + WIN].astype(np.float64) * w for t in range(T)])
    y = np.fft.irfft(np.fft.rfft(fr, axis=1) * mask, n=WIN, axis=1) * w
    out, env = np.zeros((T - 1) * HOP + WIN), np.zeros((T - 1) * HOP + WIN)
    for t in range(T):
        out[t * HOP:t * HOP + WIN] += y[t]
        env[t * HOP:t * HOP + WIN] += w * w
    return (out / np.maximum(env, 1e-10))[:x.shape[0]]


@pytest.fixture(scope="module")
def cfg_a():
    from mlx_audio_amd.sts.models.mossformer2_se import MossFormer2SEConfig, MossFormer2SEModel, make_mossformer2_weights

    cfg = MossFormer2SEConfig(out_channels=64, num_blocks=2)
    w = make_mossformer2_weights(cfg, 11)
    eng = MossFormer2SEModel(cfg, weights=w, device="cuda:0", dither=0.0)
    clips = [R.synth_clip(100 + i, samples(f)) for i, f in enumerate(FRAMES)]
    outs, st = eng.enhance_batch(clips, return_stages=True)       # ONE ragged batch
    ref = []
    for b, f in enumerate(FRAMES):
        s = {}
        s["mask"] = R.masknet(st["feats"][b, :f].cpu(), w, cfg.num_blocks, s)
        s["wave"] = backend64(clips[b] * np.float32(32768.0), s["mask"].numpy()) / 32768.0
        ref.append(s)
    return cfg, w, eng, clips, outs, st, ref


def test_ragged_batch_stage_by_stage_against_float64(cfg_a):
    """Layer 0's FLASH output and Gated-FSMN output, the mask and the waveform of every item of the ragged batch.
    Measured on MI355X (largest distance / peak over the six items): FLASH 6.1e-6, Gated-FSMN 7.4e-6, mask 9.0e-6, waveform 6.3e-6."""
    cfg, w, eng, clips, outs, st, ref = cfg_a
    assert st["frames"] == FRAMES
    p = ref[5]["parts"]
    assert p["quad"] > 0.1 * p["lin"] and p["lin"] > 0.1 * p["quad"], p           # both attention terms carry weight
    worst = {}
    for b, f in enumerate(FRAMES):
        for k in ("flash0", "fsmn0", "mask"):
            r = ref[b][k].numpy()
            assert np.isfinite(r).all()
            d = rel_peak(st[k][b, :f].cpu().numpy(), r)
            worst[k] = max(worst.get(k, 0.0), d)
            print(f"{f} frames {k}: distance / peak {d:.2e}")
            assert d < BAR, (f, k, d)
        assert outs[b].shape == clips[b].shape
        d = rel_peak(outs[b], ref[b]["wave"])
        worst["wave"] = max(worst.get("wave", 0.0), d)
        print(f"{f} frames wave: distance / peak {d:.2e}")
        assert d < BAR, (f, d)
        m = ref[b]["mask"]
        assert float((m == 0).double().mean()) > 0.001 and float((m > 0).double().mean()) > 0.01    # the final ReLU is exercised
        assert np.abs(ref[b]["wave"] - clips[b]).max() > 0.1 * np.abs(ref[b]["wave"]).max()           # the mask does something
    print("largest distance / peak", {k: f"{v:.2e}" for k, v in worst.items()})


def test_batch_items_equal_the_items_alone(cfg_a):
    """Every item of the ragged batch against ``enhance`` of that clip alone: 1e-5 of the peak (conv_gemm's tiles see other row counts; the four
    MossFormer2 kernels themselves are bit-equal, tests/test_gau_kernels_gpu.py).  Prints whether the waveforms are bit-equal.
    Measured on MI355X: bit-equal on all six items."""
    cfg, w, eng, clips, outs, st, ref = cfg_a
    equal = True
    for b, f in enumerate(FRAMES):
        alone = eng.enhance(clips[b])
        d = rel_peak(outs[b], alone)
        equal = equal and np.array_equal(outs[b], alone)
        print(f"{f} frames: batched vs alone, distance / peak {d:.2e}")
        assert d < BATCH, (f, d)
    print("enhance_batch bit-equal to the items alone:", equal)
    again = eng.enhance_batch(clips)
    assert all(np.array_equal(a, b) for a, b in zip(again, outs))      # two calls: the same bits


def test_digital_silence_gives_a_finite_mask_and_an_exactly_zero_waveform(cfg_a):
    cfg, w, eng = cfg_a[:3]
    outs, st = eng.enhance_batch([np.zeros(samples(58), dtype=np.float32), np.zeros(samples(3), dtype=np.float32)], return_stages=True)
    assert torch.isfinite(st["mask"][0]).all() and torch.isfinite(st["mask"][1, :3]).all()
    assert all(not o.any() and np.isfinite(o).all() for o in outs)


def test_enhance_takes_the_shapes_the_reference_takes(cfg_a, tmp_path):
    """[L], [1, L], a tensor and [L, channels] (the first channel) give the same samples; a file path is read, mixed to mono and resampled."""
    from mlx_audio_amd import audio_io

    cfg, w, eng, clips = cfg_a[:4]
    clip = clips[2]
    want = eng.enhance(clip)
    assert want.shape == clip.shape and want.dtype == np.float64
    assert np.array_equal(eng.enhance(clip.reshape(1, -1)), want)
    assert np.array_equal(eng.enhance(torch.from_numpy(clip)), want)
    assert np.array_equal(eng.enhance(np.stack([clip, -clip], axis=1)), want)
    path = str(tmp_path / "clip.wav")
    audio_io.write(path, clip, 24000)                      # 16-bit PCM at half the rate: the path goes through the resampler
    got = eng.enhance(path)
    assert got.ndim == 1 and abs(got.shape[0] - 2 * clip.shape[0]) <= 2 and np.isfinite(got).all() and got.any()
    with pytest.raises(ValueError, match="shorter than one window"):
        eng.enhance(np.zeros(1000, dtype=np.float32))


def test_segmented_and_chunked_paths_equal_their_windows_run_one_by_one(cfg_a):
    """Scaled-down decode lengths (windows and chunks of 59 frames, 0.504 s; whole-clip limit 1 s; clip 2.3 s): ``enhance`` through the segmented path and
    through ``_decode_chunked`` (a partial last chunk included) against the same windows pushed through ``_process_chunk`` one at a time and laid
    out by the reference's index arithmetic (held on its own in tests/test_mossformer2_cpu.py)."""
    from mlx_audio_amd.sts.models.mossformer2_se import MossFormer2SEConfig, MossFormer2SEModel
    from mlx_audio_amd.sts.models.mossformer2_se.model import chunk_plan, segment_plan

    cfg0, w = cfg_a[0], cfg_a[1]
    cfg = MossFormer2SEConfig(**{**cfg0.to_dict(), "one_time_decode_length": 1, "decode_window": 24192 / 48000, "chunk_seconds": 24192 / 48000,
                                 "auto_chunk_threshold": 2.0})
    eng = MossFormer2SEModel(cfg, weights=w, device="cuda:0", dither=0.0)
    clip = R.synth_clip(7, int(2.3 * 48000))
    n, W = clip.shape[0], 24192      # 1920 + 58 * 384: a whole number of frames, as the reference's reassembly needs
    x = np.ascontiguousarray(clip * 32768.0, dtype=np.float32)
    # segmented
    padded, plan = segment_plan(n, W)
    xp = np.concatenate([x, np.zeros(padded - n, dtype=np.float32)])
    want = np.zeros(padded)
    for s, lo, hi in plan:
        want[s + lo:s + hi] = eng._process_chunk(xp[s:s + W], None, W).cpu().numpy()[lo:hi]
    got = eng.enhance(clip, chunked=False)
    assert len(plan) > 2 and got.shape == (n,)
    d = rel_peak(got, want[:n] / 32768.0)
    print(f"segmented path: {len(plan)} windows as one batch vs one by one, distance / peak {d:.2e}")
    assert d < BATCH
    # chunked, picked by the auto threshold
    cplan = chunk_plan(n, W, int(W * cfg.chunk_overlap), eng.produced)
    assert cplan[-1][1] < W
    want = np.zeros(n)
    for s, ln, ks, kept in cplan:
        want[s + ks:s + ks + kept] = eng._process_chunk(x[s:s + ln], None, ln).cpu().numpy()[ks:ks + kept]
    got = eng.enhance(clip)
    d = rel_peak(got, want / 32768.0)
    print(f"chunked path: {len(cplan)} chunks vs one by one, distance / peak {d:.2e}")
    assert d < BATCH and np.array_equal(got, eng.enhance(clip, chunked=True))


def test_two_blocks_at_the_published_widths_against_float64():
    """512 / 961 with 2 blocks on 300 frames, one item: stages, mask and waveform at the same bar.
    Measured on MI355X: FLASH 3.9e-6, Gated-FSMN 3.8e-6, mask 5.5e-6, waveform 1.6e-6 of the peak."""
    from mlx_audio_amd.sts.models.mossformer2_se import MossFormer2SEConfig, MossFormer2SEModel, make_mossformer2_weights

    cfg = MossFormer2SEConfig(num_blocks=2)
    w = make_mossformer2_weights(cfg, 21)
    eng = MossFormer2SEModel(cfg, weights=w, device="cuda:0", dither=0.0)
    clip = R.synth_clip(9, samples(300))
    outs, st = eng.enhance_batch([clip], return_stages=True)
    s = {}
    s["mask"] = R.masknet(st["feats"][0].cpu(), w, 2, s)
    for k in ("flash0", "fsmn0", "mask"):
        d = rel_peak(st[k][0].cpu().numpy(), s[k].numpy())
        print(f"published widths {k}: distance / peak {d:.2e}")
        assert d < BAR, (k, d)
    d = rel_peak(outs[0], backend64(clip * np.float32(32768.0), s["mask"].numpy()) / 32768.0)
    print(f"published widths wave: distance / peak {d:.2e}")
    assert d < BAR
    assert s["parts"]["quad"] > 0.1 * s["parts"]["lin"] and s["parts"]["lin"] > 0.1 * s["parts"]["quad"], s["parts"]
