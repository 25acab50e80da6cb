"""Granite Speech NAR on the device against the runs of the reference's own files stored by ``tests/golden/make_granite_nar_fixtures.py``: every
stored stage within the project's device bar of 3e-4 of the stage's peak (docs/COVERAGE.md records the measured values), every BPE frame decision,
every edited-position decision, the final ids and the decoded text equal -- for each clip alone and for the five clips as one right-padded batch;
``generate_batch`` from waveforms against the items alone; digital silence."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import _granite_nar_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DEVICE_BAR = 3e-4
BATCH_BAR = 1e-5


@pytest.fixture(scope="module")
def fixture():
    return R.load_fixture()


@pytest.fixture(scope="module", params=["A", "B"])
def case(request):
    return request.param, R.build_model(request.param, DEV)


def test_stored_stages_and_decisions(fixture, case):
    fx, meta = fixture
    tag, model = case
    worst = {}
    feats = [R.stored_features(fx, i) for i in range(len(R.CLIPS))]
    for i, f in enumerate(feats):
        final, st = model.transcribe_batch(f[None], return_stages=True)
        want = meta["configs"][tag]["decode"][i]["final"]
        assert final[0] == want == model._transcribe_tokens(f)
        assert model._tokenizer.decode(final[0]) == " ".join(f"t{t}" for t in want)
        for k, v in R.compare_clip(st, fx, tag, i).items():
            worst[k] = max(worst.get(k, 0.0), v)
    fb, lens = model._pad([f.to(DEV) for f in feats])
    final, st = model.transcribe_batch(fb, lens, return_stages=True)
    for i in range(len(feats)):
        for k, v in R.compare_clip(st, fx, tag, i, b=i).items():
            worst[k] = max(worst.get(k, 0.0), v)
    print(f"config {tag}: worst error / peak per stage:", {k: f"{v:.1e}" for k, v in worst.items()})
    assert max(worst.values()) <= DEVICE_BAR, worst


def test_front_end_and_generate_batch_against_the_items_alone(fixture, case):
    fx, meta = fixture
    tag, model = case
    clips = [R.synth_audio(n, s) for n, s in R.CLIPS]
    worst = 0.0
    feats = []
    for i, c in enumerate(clips):
        f = model._compute_features(c)
        want = torch.from_numpy(fx[f"feat{i}"]).to(DEV)
        worst = max(worst, float((f[torch.from_numpy(fx[f"feat{i}_rows"].astype(np.int64)).to(DEV)] - want).abs().max() / want.abs().max()))
        feats.append(f)
    print(f"config {tag}: features worst error / peak = {worst:.1e}")
    assert worst <= DEVICE_BAR
    outs = model.generate_batch(clips)
    alone = [model.generate(c) for c in clips]
    assert [o.text for o in outs] == [o.text for o in alone]
    assert [o.text for o in outs] == [" ".join(f"t{t}" for t in d["final"]) for d in meta["configs"][tag]["decode"]]
    fb, lens = model._pad(feats)
    _, st = model.transcribe_batch(fb, lens, return_stages=True)
    bit_equal, err = True, 0.0
    for i, f in enumerate(feats):
        _, sa = model.transcribe_batch(f[None], return_stages=True)
        assert sa["final"][0] == st["final"][i] and sa["hyp"][0] == st["hyp"][i]
        a, b = sa["hidden"][0], st["hidden"][i, :lens[i]]
        bit_equal = bit_equal and torch.equal(a, b)
        err = max(err, float((a - b).abs().max() / a.abs().max()))
    print(f"config {tag}: encoder output of a batch item against the item alone: worst error / peak = {err:.1e}, bit-equal: {bit_equal}")
    assert err <= BATCH_BAR


def test_digital_silence(case):
    tag, model = case
    final, st = model.transcribe_batch(model._compute_features(np.zeros(16000, dtype=np.float32))[None], return_stages=True)
    for k in ("hidden", "probs", "pooled", "audio", "tail_logits"):
        assert torch.isfinite(st[k]).all(), k
    assert isinstance(model.generate(np.zeros(16000, dtype=np.float32)).text, str)


def test_published_widths_against_the_float64_restatement():
    """One pass at the published widths (``_granite_nar_ref.published_config_dict``: encoder 1024 = 8 x 128 at context 200, four fused layers to 4096,
    projector 2048 = 32 x 64, editor 2048 with 16 heads of 128 over 4 kv heads and the multipliers 1 / 128, 12, 8, 0.22; one layer each, vocabulary
    4096) on 3 s of audio against ``reference_forward``: the stages within the device bar, every decision equal (the restatement's own top-2 gaps
    are asserted to be at least ``_margin.THR`` first)."""
    import _margin
    from mlx_audio_amd.stt.models.granite_speech_nar import GraniteSpeechNar as Model, ModelConfig, make_granite_nar_weights

    cfg = ModelConfig.from_dict(R.published_config_dict())
    w = make_granite_nar_weights(cfg, seed=1, head_gain=6.0, bpe_blank_bias=3.0, embed_gain=0.02)
    model = Model(cfg, w, device=DEV)
    feats = model._compute_features(R.synth_audio(48000, 21)).to(torch.bfloat16).to(torch.float32).cpu()
    assert feats.shape == (150, 160)
    ref = R.reference_forward(cfg, w, feats)
    assert float(ref["bpe_gap"].min()) >= _margin.THR and float(ref["edit_gap"].min()) >= _margin.THR, "the test's own inputs leave a decision on a knife edge"
    final, st = model.transcribe_batch(feats[None], return_stages=True)
    N = len(ref["edit_ids"])
    assert st["bpe_ids"][0].tolist() == ref["bpe_ids"] and st["hyp"][0] == ref["hyp"] and st["edit_ids"][0, :N].tolist() == ref["edit_ids"]
    assert final[0] == ref["final"]
    A = st["audio_lens"][0]
    got = dict(hidden=st["hidden"][0], probs=st["probs"][0], pooled=st["pooled"][0], audio=st["audio"][0, :A], editor_out=st["editor0"][0],
               tail_logits=st["tail_logits"])
    errs = {k: float((v.cpu().double() - ref[k]).abs().max() / ref[k].abs().max()) for k, v in got.items()}
    print("published widths: error / peak per stage:", {k: f"{v:.1e}" for k, v in errs.items()})
    assert max(errs.values()) <= DEVICE_BAR, errs
