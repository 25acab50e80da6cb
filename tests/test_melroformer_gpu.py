"""Mel-Band RoFormer on the device, waveform to waveform, against the reference's own runs (``tests/golden/ref_melroformer.npz``) and, at the
``kim_vocal_2`` widths, against the float64 helper ``tests/_melroformer_ref.py``.  Only the committed fixtures are read."""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
GOLD = os.path.join(HERE, "golden")

import _melroformer_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
BAR = 3e-4     # of each tensor's peak: the project's bar for a precision-4 chain against reference-run fixtures (test_dfn_gpu.py, test_parakeet_gpu.py)
BATCH = 1e-5   # of the peak: the project's bound wherever the launch size picks the kernel


def rel_peak(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


@pytest.fixture(scope="module")
def fx():
    with open(os.path.join(GOLD, "ref_melroformer.json")) as f:
        meta = json.load(f)
    return np.load(os.path.join(GOLD, "ref_melroformer.npz")), meta


@pytest.fixture(scope="module")
def engines(fx):
    from mlx_audio_amd.sts.models.mel_roformer import MelRoFormer, MelRoFormerConfig, make_melroformer_weights

    _, meta = fx
    out = {}
    for tag, c in meta["configs"].items():
        cfg = MelRoFormerConfig.custom(**c["kw"])
        w = make_melroformer_weights(cfg, meta["seed_w"])
        calls = [np.stack([R.synth_clip(seed, n, zero) for seed, n, zero in call]) for call in c["calls"]]
        out[tag] = (cfg, w, calls, MelRoFormer(cfg, weights=w, device="cuda:0"))
    return out


def _stages(st):
    return dict(split=st["split"], tf0=st["tf"][0], tf1=st["tf"][1], mask=st["mask"])


@pytest.mark.parametrize("tag", ["A", "B"])
def test_fixture_parity_stage_by_stage(fx, engines, tag):
    """Every fixture call: the band-split output, both transformers of level 0, the merged mask and the waveform within 3e-4 of each tensor's peak
    of the reference's float32 runs; the silent frames' split rows are the bias rows exactly.
    Measured on MI355X (largest distance / peak over both configs): band split 4.0e-7, time transformer 8.2e-7, frequency transformer 8.1e-7, merged mask
    1.4e-6, waveform 8.6e-7."""
    npz, meta = fx
    cfg, _, calls, eng = engines[tag]
    worst = {}
    for i, x in enumerate(calls):
        y, st = eng(x, return_stages=True)
        T = meta["configs"][tag]["frames"][i]
        assert y.shape == x.shape and y.dtype == torch.float32 and st["split"].shape[1] == T
        for k, v in _stages(st).items():
            v = v.cpu().numpy()
            if k != "mask" and T > meta["stride_above"]:
                v = v[:, ::meta["stride"]]
            d = rel_peak(v, npz[f"{tag}{i}_{k}"])
            worst[k] = max(worst.get(k, 0.0), d)
            print(f"config {tag} call {i} {k}: distance / peak {d:.2e}")
            assert d < BAR, (tag, i, k, d)
        d = rel_peak(y.cpu().numpy(), npz[f"{tag}{i}_wave"])
        worst["wave"] = max(worst.get("wave", 0.0), d)
        print(f"config {tag} call {i} wave: distance / peak {d:.2e}")
        assert d < BAR, (tag, i, "wave", d)
        silent = meta["configs"][tag].get("silent_frames", {}).get(str(i))
        if silent:
            assert torch.equal(st["split"][0, silent], eng.split_bias.expand(len(silent), -1, -1))
    print(f"config {tag}: largest distance / peak", {k: f"{v:.2e}" for k, v in worst.items()})


@pytest.mark.parametrize("tag", ["A", "B"])
def test_batch_items_equal_the_items_alone(fx, engines, tag):
    """The ``B = 2`` call against each item alone: 1e-5 of the peak (the GEMM tiles and the attention launches see other row counts).
    Measured on MI355X: bit-equal on both configs."""
    _, meta = fx
    _, _, calls, eng = engines[tag]
    x = next(c for c in calls if c.shape[0] == 2)
    y = eng(x).cpu().numpy()
    for b in range(2):
        d = rel_peak(eng(x[b:b + 1]).cpu().numpy(), y[b:b + 1])
        print(f"config {tag} item {b}: alone vs batched, distance / peak {d:.2e}")
        assert d < BATCH, (tag, b, d)


def test_silence_gives_exact_zeros_and_two_calls_the_same_bits(engines):
    _, _, calls, eng = engines["A"]
    z = eng(np.zeros((2, 2, 500), dtype=np.float32))
    assert z.shape == (2, 2, 500) and not z.any() and torch.isfinite(z).all()
    for x in (calls[2], calls[4]):
        a, b = eng(x), eng(x)
        assert torch.equal(a, b)


def test_full_width_pass_against_the_float64_helper():
    """One pass at the ``kim_vocal_2`` widths (dim 384, 8 heads of 64, 60 bands of 24 to 520 entries, n_fft 2048, hop 441, mask MLP of 1536) at depth 1
    on 0.25 s of stereo audio, one item, against ``_melroformer_ref.forward`` on the same seeded checkpoint: stages and waveform, the same bar.
    Measured on MI355X: waveform 3.2e-6 of peak; band split 5.4e-5, transformers 4.8e-5 and 5.1e-5, merged mask 7.7e-5 -- the float32 STFT's rounding in the
    near-empty high bands of the seeded clip, which the per-band norm scales to unit size (the fixture configs, whose bands all carry signal, sit at 1e-6)."""
    from mlx_audio_amd.sts.models.mel_roformer import MelRoFormer, MelRoFormerConfig, make_melroformer_weights

    cfg = MelRoFormerConfig.custom(depth=1)
    assert (cfg.dim, cfg.heads, cfg.num_bands, cfg.n_fft, cfg.hop_length, cfg.mlp_hidden) == (384, 8, 60, 2048, 441, 1536)
    w = make_melroformer_weights(cfg, 5)
    eng = MelRoFormer(cfg, weights=w, device="cuda:0")
    assert (min(eng.tables.band_dims), max(eng.tables.band_dims), sum(eng.tables.band_dims)) == (24, 520, 7916)
    x = R.synth_clip(51, 11025)[None]
    y, st = eng(x, return_stages=True)
    yr, sr = R.forward(cfg, {k: v.numpy() for k, v in w.items()}, x, idx=[ix.astype(np.int64) for ix in eng.band_indices])
    d = {k: rel_peak(v.cpu().numpy(), dict(split=sr["split"], tf0=sr["tf"][0], tf1=sr["tf"][1], mask=sr["mask"])[k]) for k, v in _stages(st).items()}
    d["wave"] = rel_peak(y.cpu().numpy(), yr)
    print("full width: distance / peak", {k: f"{v:.2e}" for k, v in d.items()})
    assert max(d.values()) < BAR, d
    assert float(np.abs(yr).max()) > 1e-3 and float(np.abs(yr - x).max()) > 0.05
