"""Parakeet CTC on the device against the reference's own runs (``tests/golden/ref_parakeet_ctc.npz`` / ``.json``: one un-padded clip per call) and
against itself (a padded batch against its items alone at the published widths)."""
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
import _parakeet_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
THR_H = 3e-4   # of each tensor's peak: the bar of test_s3_gpu.py and test_whisper_gpu.py::test_tiny_encoder_layers
FAMILY = "parakeet_ctc"


def rel_peak(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLD, "ref_parakeet_ctc.npz"))


@pytest.fixture(scope="module")
def meta():
    with open(os.path.join(GOLD, "ref_parakeet_ctc.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def engines(meta):
    """tag -> (engine, [mel])."""
    from mlx_audio_amd.stt.models.parakeet import ParakeetCTC

    return {tag: (ParakeetCTC(args, w), mels) for tag, (args, w, mels) in R.load_models(meta).items()}


def test_fixture_parity(fx, meta, engines):
    """Both configs, every clip alone and all clips of a config as one padded batch: ``out_lengths`` equal; the subsampler's output, every layer's
    output and layer 0's attention / convolution module outputs within 3e-4 of each tensor's peak on the valid frames; frame ids through the margin
    rule (at least 95 % of at least 400 frames compared); the decode result equal for every clip without a frame under the threshold.
    Measured on MI355X: worst stage distance 8.2e-7 of the peak (conv0; pre_encode 5.7e-7, attn0 7.9e-7, layers 5.5e-7 / 4.5e-7); 540 of 540 frame ids compared."""
    compared = total = 0
    worst = {}
    for tag, (eng, mels) in engines.items():
        batch, lens = R.pad_batch(mels)
        runs = [(eng.encoder(torch.from_numpy(m)[None], None, return_layers=True), 0, i, "alone") for i, m in enumerate(mels)]
        rb = eng.encoder(batch, lens, return_layers=True)
        runs += [(rb, i, i, "batch") for i in range(len(mels))]
        for (hidden, out_len, taps), row, i, how in runs:
            n = int(fx[f"{tag}{i}_out_len"])
            assert out_len.dtype == torch.int32 and int(out_len[row]) == n, (tag, i, how)
            if f"{tag}{i}_layers" in fx:
                got = dict(pre_encode=taps["pre_encode"], attn0=taps["attn0"], conv0=taps["conv0"], **{f"layer{j}": t for j, t in enumerate(taps["layers"])})
                want = dict(pre_encode=fx[f"{tag}{i}_pre_encode"], attn0=fx[f"{tag}{i}_attn0"], conv0=fx[f"{tag}{i}_conv0"],
                            **{f"layer{j}": t for j, t in enumerate(fx[f"{tag}{i}_layers"])})
                for k in want:
                    e = rel_peak(got[k][row, :n].cpu().numpy(), want[k])
                    worst[k] = max(worst.get(k, 0.0), e)
                    print(f"parakeet {tag}{i} {how} {k}: {e:.2e}")
                    assert e < THR_H, (tag, i, how, k, e)
            ids = eng.decoder.frame_ids(hidden)[row, :n].cpu().numpy()
            compared += _margin.walk_resync(FAMILY, ids, fx[f"{tag}{i}_ids"], fx[f"{tag}{i}_gap"], where=(tag, i, how))
            total += n
        alone = [eng.decode(torch.from_numpy(m)[None])[0] for m in mels]
        together = eng.decode(batch, lens)
        for i, want in enumerate(meta["configs"][tag]["decode"]):
            if (fx[f"{tag}{i}_gap"] < _margin.THR).any():
                continue
            assert R.same_decode(R.result_dict(alone[i]), want) and R.same_decode(R.result_dict(together[i]), want), (tag, i)
    print(f"parakeet fixture parity: worst stage distances {({k: float(f'{v:.2e}') for k, v in worst.items()})}; {compared} of {total} frame ids compared")
    assert total >= 400 and compared >= 0.95 * total, (compared, total)


@pytest.fixture(scope="module")
def wide():
    from mlx_audio_amd.stt.models.parakeet import ParakeetCTC, make_parakeet_weights

    args = R.make_args(R.ENC_WIDE)
    eng = ParakeetCTC(args, make_parakeet_weights(args, 91, head_gain=R.HEAD_GAIN, blank_bias=4.0))
    mels = [R.synth_mel(400 + i, R.ENC_WIDE["feat_in"], frames) for i, frames in enumerate((801, 200, 517, 333, 640, 264))]   # 2 - 8 s
    return eng, mels


def test_padded_batch_equals_items_alone_at_published_widths(wide):
    """d_model 1024 / 8 heads / K 9 / feat_in 128 / 256 conv channels, two layers, six clips of 2 - 8 s on seeded weights: the hidden states of the
    padded batch within 3e-4 of the peak of each item run alone, the frame ids by the margin rule (the gap taken from the item's own run).
    Measured on MI355X: worst hidden distance 5.6e-7; 346 of 346 frame ids compared."""
    eng, mels = wide
    batch, lens = R.pad_batch(mels)
    hb, lb = eng.encoder(batch, lens)
    logp_b = eng.decoder(hb)
    worst, compared, total = 0.0, 0, 0
    for i, m in enumerate(mels):
        h1, l1 = eng.encoder(torch.from_numpy(m)[None])
        n = int(l1[0])
        assert int(lb[i]) == n == eng.encoder.out_lengths([m.shape[0]])[0]
        e = rel_peak(hb[i, :n].cpu().numpy(), h1[0].cpu().numpy())
        worst = max(worst, e)
        assert e < THR_H, (i, e)
        logp = eng.decoder(h1)[0]
        top = torch.topk(logp, 2, dim=-1).values
        compared += _margin.walk_resync(FAMILY, logp_b[i, :n].argmax(-1).cpu().numpy(), logp.argmax(-1).cpu().numpy(), (top[:, 0] - top[:, 1]).cpu().numpy(), where=("wide", i))
        total += n
    print(f"parakeet wide batch vs alone: worst hidden distance {worst:.2e}; {compared} of {total} frame ids compared")
    assert compared >= 0.95 * total


def test_two_calls_are_bitwise_equal(engines, wide):
    for eng, mels in list(engines.values()) + [wide]:
        batch, lens = R.pad_batch(mels[-2:])
        h1, _ = eng.encoder(batch, lens)
        ids1 = eng.decoder.frame_ids(h1)
        h1 = h1.clone()
        h2, _ = eng.encoder(batch, lens)
        assert torch.equal(h1, h2) and torch.equal(ids1, eng.decoder.frame_ids(h2))


def test_generate_runs_from_samples(engines):
    """``generate`` on a waveform: the device log-mel front end into ``decode``; equal to ``decode`` on the same mel."""
    from mlx_audio_amd.stt.models.nemo.alignment import AlignedResult
    from mlx_audio_amd.stt.models.parakeet import log_mel_spectrogram

    eng, _ = engines["A"]
    audio = 0.1 * torch.randn(16000, generator=torch.Generator().manual_seed(3))
    res = eng.generate(audio)
    assert isinstance(res, AlignedResult)
    mel = log_mel_spectrogram(audio, eng.preprocessor_config)
    assert mel.shape[2] == eng.encoder_config.feat_in
    assert R.result_dict(eng.decode(mel)[0]) == R.result_dict(res)
