"""FireRedASR2 on the device against the reference's own runs (``tests/golden/ref_fireredasr2.npz`` / ``.json``): every stored stage at 3e-4 of its
peak (the bar the sibling models use), every beam decision before the first knife edge through ``_margin.walk``, texts and confidences;
``generate_batch`` of the four clips against the items alone; ``from_pretrained`` on a written directory; one 1 + 1-layer pass at the published
widths against the float64 restatement."""
import json

import numpy as np
import pytest
import torch

import _fireredasr2_ref as R
import _margin
from mlx_audio_amd.stt.models.fireredasr2 import make_fireredasr2_weights
from mlx_audio_amd.stt.models.fireredasr2.fireredasr2 import Model, encoder_frames

pytestmark = pytest.mark.gpu
BAR = 3e-4
DEV = "cuda:0"


def build(tag, ending, tmp):
    cc = R.CONFIGS[tag]
    c = R.make_config(cc["cfg"])
    w = R.eos_variant(make_fireredasr2_weights(c, cc["seed_w"], logit_gain=cc["logit_gain"], eos_gain=cc["eos_gain"]), c, ending)
    R.write_side_files(tag, str(tmp), c)
    return Model.post_load_hook(Model(c, w, device=DEV), tmp)


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    return {(tag, e): build(tag, e, tmp_path_factory.mktemp(f"fr_{tag}_{e}")) for tag in R.CONFIGS for e in R.ENDINGS}


@pytest.mark.parametrize("tag", ["A", "B"])
def test_against_the_reference_runs(models, tag):
    """From the waveform: the device fbank and CMVN, every stored stage, then every stored ``generate`` run (three endings, every beam size)."""
    z, meta = R.load_fixtures()
    encs = {}
    for i, (n, seed) in enumerate(R.CONFIGS[tag]["clips"]):
        audio = R.synth_audio(seed, n)
        s = np.array([audio.astype(np.float64).sum(), (audio.astype(np.float64) ** 2).sum()])
        assert np.allclose(s, z[f"{tag}{i}_audiosum"], rtol=1e-12), "the regenerated clip is not the maker's"
        feats, ns = models[(tag, "late")].features([audio])
        assert ns[0] == z[f"{tag}{i}_feats"].shape[0]
        assert R.rel_err(feats[0, :ns[0]].cpu().numpy(), z[f"{tag}{i}_feats"]) < BAR
        encs[i] = R.check_encoder(models[(tag, "late")], z, tag, i, BAR, feats=feats[0, :ns[0]])
    total = [0, 0]
    for run in meta["configs"][tag]["runs"]:
        enc, rows = encs[run["clip"]]
        n, m = R.check_run(models[(tag, run["ending"])], z, run, enc, rows, "fireredasr2")
        total[0] += n
        total[1] += m
    assert total[0] >= 0.8 * total[1], total


@pytest.mark.parametrize("tag", ["A", "B"])
def test_generate_text_and_confidence(models, tag):
    z, meta = R.load_fixtures()
    model = models[(tag, "late")]
    for run in meta["configs"][tag]["runs"]:
        if run["ending"] != "late" or run["clip"] not in (1, 2) or "max_len" in run or float(z[run["key"] + "_margin"].min()) < 10 * _margin.THR:
            continue
        n, seed = R.CONFIGS[tag]["clips"][run["clip"]]
        res = model.generate(R.synth_audio(seed, n), beam_size=run["beam"])
        assert res.text == run["text"] and res.generation_tokens == run["generation_tokens"], (run["key"], res.text, run["text"])
        assert abs(res.segments[0]["confidence"] - run["confidence"]) <= 2e-3


def test_generate_batch_equals_the_items_alone(models):
    model = models[("A", "late")]
    clips = [R.synth_audio(seed, n) for n, seed in R.CONFIGS["A"]["clips"]]
    feats, ns = model.features(clips)
    out, rows = model.encode_features(feats, ns)
    hyps = model.beam_search(out, rows, beam_size=3)
    batch = model.generate_batch(clips, beam_size=3)
    for b, a in enumerate(clips):
        f1, n1 = model.features([a])
        o1, r1 = model.encode_features(f1, n1)
        assert r1[0] == rows[b] == encoder_frames(ns[b])
        assert R.rel_err(out[b, :rows[b]].cpu().numpy(), o1[0, :r1[0]].cpu().numpy()) < 1e-5
        h1 = model.beam_search(o1, r1, beam_size=3)
        assert h1[0][0] == hyps[b][0], (b, h1[0][0], hyps[b][0])
        one = model.generate(a, beam_size=3)
        assert one.text == batch[b].text and one.generation_tokens == batch[b].generation_tokens and one.segments == batch[b].segments


def test_from_pretrained_on_a_written_directory(models, tmp_path):
    from safetensors.torch import save_file

    cc = R.CONFIGS["B"]
    c = R.make_config(cc["cfg"])
    w = R.eos_variant(make_fireredasr2_weights(c, cc["seed_w"], logit_gain=cc["logit_gain"], eos_gain=cc["eos_gain"]), c, "late")
    save_file(R.to_torch_checkpoint(w, tied=False), str(tmp_path / "model.safetensors"))     # PyTorch names and layouts, as published
    with open(tmp_path / "config.json", "w") as f:
        json.dump(c.to_dict(), f)
    R.write_side_files("B", str(tmp_path), c)
    model = Model.from_pretrained(tmp_path, device=DEV)
    n, seed = cc["clips"][1]
    a = R.synth_audio(seed, n)
    got, want = model.generate(a, beam_size=5), models[("B", "late")].generate(a, beam_size=5)
    assert got.text == want.text and got.segments == want.segments and got.text != ""
    with pytest.raises(NotImplementedError, match="beam_size 9"):
        model.generate(a, beam_size=9)


def test_published_widths_one_layer_each():
    """1 + 1 layers at the published widths (1280 wide, 20 heads of 64, K 33, odim 8667) on a 2 s clip against the float64 restatement: the encoder at
    3e-4 of its peak, the beam decisions of eight steps through the margin rule."""
    cfg = dict(encoder=dict(n_layers=1), decoder=dict(n_layers=1))
    c = R.make_config(cfg)
    w = make_fireredasr2_weights(c, 5, logit_gain=20.0)
    model = Model(c, w, device=DEV)
    feats, ns = model.features([R.synth_audio(77, 32000)])
    out, rows, st = model.encode_features(feats, ns, return_stages=True)
    want = R.encode(w, c, feats[0, :ns[0]].cpu())
    assert rows[0] == want["out"].shape[0] == encoder_frames(ns[0])
    for key, got in (("sub", st["sub"]), ("attn0", st["attn0"]), ("conv0", st["conv0"]), ("out", out)):
        assert R.rel_err(got[0, :rows[0]].cpu().numpy(), want[key].numpy()) < BAR, key
    res = R.beam_search(w, c, want["out"], beam_size=3, max_len=8)
    hyps, trace = model.beam_search(out, rows, beam_size=3, max_len=8, return_trace=True)
    got, exp, mar = [], [], []
    for s, step in enumerate(res["steps"]):
        got += trace[s]["beam_idx"][0].tolist() + trace[s]["tokens"][0].tolist()
        exp += step["beam_idx"] + step["tokens"]
        mar += [step["margin"]] * 6
    if _margin.walk("fireredasr2", got, exp, mar, where="published widths") == len(mar):
        assert [t for t in hyps[0][0]][:len(res["seq"])] == res["seq"]
