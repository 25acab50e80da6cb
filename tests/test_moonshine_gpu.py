"""Moonshine on the device against the reference's own runs (``tests/golden/ref_moonshine.npz`` / ``.json``, ``make_moonshine_fixtures.py``) at 3e-4
of the peak -- the project's bar for reference-run fixtures on the device -- and against the float64 restatement ``tests/_moonshine_ref.py``."""
import json

import numpy as np
import pytest
import torch

import _moonshine_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAR = 3e-4
BATCH_BAR = 1e-5   # the project's batch-vs-single bar; conv_gemm picks tiles by row count, so bit-equality is not asked


def build(tag, **kw):
    from mlx_audio_amd.stt.models.moonshine.moonshine import Model, make_moonshine_weights

    cc = R.CONFIGS[tag]
    c = R.make_config(dict(cc["cfg"], **kw))
    w = make_moonshine_weights(c, cc["seed_w"], logit_gain=cc["logit_gain"], eos_gain=cc["eos_gain"])
    return Model(c, w, device=DEV), c, w


@pytest.fixture(scope="module")
def fixtures():
    return R.load_fixtures()


@pytest.fixture(scope="module", params=["A", "B"])
def built(request):
    return (request.param,) + build(request.param)


def test_every_stored_stage_tokens_logits_and_text(built, fixtures):
    """Measured on MI355X: see the printed lines (recorded in docs/COVERAGE.md).  Both endings (EOS, max_tokens) are in the stored clips."""
    tag, model, c, w = built
    z, meta = fixtures
    worst = {}
    for i in range(len(R.CONFIGS[tag]["clips"])):
        for k, v in R.check_clip(model, z, meta, tag, i, BAR, "moonshine", report=print).items():
            worst[k] = max(worst.get(k, 0.0), v)
    print(f"moonshine {tag} worst: " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    decs = [d for t in meta["configs"].values() for d in t["decode"]]
    assert any(d["eos"] and len(d["tokens"]) >= 3 for d in decs) and any(not d["eos"] for d in decs)


def test_generate_batch_equals_its_items(built, fixtures):
    tag, model, c, w = built
    z, meta = fixtures
    clips = [R.clip_audio(z, tag, i) for i in range(4)]
    out, frames = model.encode(clips)
    res = model.generate_batch(clips, max_tokens=meta["max_tokens"])
    for i, a in enumerate(clips):
        one, f1 = model.encode(a)
        assert f1 == [frames[i]]
        err = float((out[i, :frames[i]] - one[0]).abs().max() / one.abs().max())
        print(f"moonshine {tag}{i}: batch vs single encoder output {err:.1e}")
        assert err < BATCH_BAR
        dec = meta["configs"][tag]["decode"][i]
        assert res[i].text == dec["text"] and res[i].generation_tokens == dec["generation_tokens"]
        assert model.generate(a, max_tokens=meta["max_tokens"]).text == res[i].text


def test_from_pretrained_and_sampling(tmp_path, fixtures):
    from safetensors.torch import save_file

    from mlx_audio_amd.stt.models.moonshine.moonshine import Model

    z, meta = fixtures
    model, c, w = build("A")
    with open(tmp_path / "config.json", "w") as f:
        json.dump(dict(R.CONFIGS["A"]["cfg"], model_type="moonshine"), f)
    save_file({("model." + k): (v.permute(0, 2, 1).contiguous() if v.dim() == 3 else v.contiguous()) for k, v in w.items()}, str(tmp_path / "model.safetensors"))
    loaded = Model.from_pretrained(tmp_path, device=DEV)
    audio = R.clip_audio(z, "A", 2)
    assert loaded.generate(audio, max_tokens=8).text == model.generate(audio, max_tokens=8).text
    enc, frames = model.encode(audio)
    a = model.decode_greedy(enc, frames, max_tokens=8, temperature=0.9, seed=5)
    b = model.decode_greedy(enc, frames, max_tokens=8, temperature=0.9, seed=5)
    assert a == b and all(0 <= t < c.vocab_size for t in a[0])


def test_tiny_published_widths_against_the_restatement():
    """288 wide, 8 heads of 36, 6 + 6 layers, vocabulary 32768, 2 s of audio, 8 tokens: encoder output, the 8 greedy logits rows and tokens."""
    from mlx_audio_amd.stt.models.moonshine.moonshine import Model, ModelConfig, make_moonshine_weights

    c = ModelConfig()
    w = make_moonshine_weights(c, 21, logit_gain=6.0)
    model = Model(c, w, device=DEV)
    audio = R.synth_audio(31, 32000)
    out, frames = model.encode(audio)
    w64 = R.to64(w)
    want = R.encoder64(w64, c, audio)
    err = float((out[0].double().cpu() - want).abs().max() / want.abs().max())
    toks, trace = model.decode_greedy(out, frames, max_tokens=8, return_trace=True)
    wt, rows, gaps = R.greedy64(w64, c, want, max_tokens=8)
    n = min(len(rows), len(trace["logits"]))
    lerr = max(float((trace["logits"][s][0].double() - rows[s]).abs().max() / rows[s].abs().max()) for s in range(n))
    print(f"moonshine tiny widths: {frames[0]} frames, encoder {err:.1e}, logits {lerr:.1e}, min gap {min(gaps):.3f}")
    assert err < BAR and lerr < BAR
    if min(gaps) > 1e-3:
        assert toks[0] == wt


def test_grouped_decoder_kv_heads_against_the_restatement():
    """Config B with DECODER kv heads 2 (4 query heads on 2 cached kv heads), which the reference cannot step: a ragged batch of three clips, each
    item's encoder output, greedy logits rows and tokens, and the T = 3 then T = 2 decoder call against ``tests/_moonshine_ref.py``."""
    model, c, w = build("B", decoder_num_key_value_heads=2)
    w64 = R.to64(w)
    clips = [R.synth_audio(40 + j, n) for j, n in enumerate((895, 9000, 4000))]
    out, frames = model.encode(clips)
    toks, trace = model.decode_greedy(out, frames, max_tokens=8, return_trace=True)
    for b, a in enumerate(clips):
        want = R.encoder64(w64, c, a)
        err = float((out[b, :frames[b]].double().cpu() - want).abs().max() / want.abs().max())
        wt, rows, gaps = R.greedy64(w64, c, want, max_tokens=8)
        n = len(rows)   # the batch steps on while another item is unfinished: this item's rows are its first n
        lerr = max(float((trace["logits"][s][b].double() - rows[s]).abs().max() / rows[s].abs().max()) for s in range(n))
        e = out[b:b + 1, :frames[b]].contiguous()
        h1, cache = model(torch.tensor([R.FORCED[:3]]), e)
        h2, _ = model(torch.tensor([R.FORCED[3:]]), e, cache)
        wh = R.decoder64(w64, c, R.FORCED, want)
        ferr = float((torch.cat([h1[0], h2[0]]).double().cpu() - wh).abs().max() / wh.abs().max())
        print(f"moonshine grouped decoder item {b} ({frames[b]} frames): encoder {err:.1e}, logits {lerr:.1e}, forced {ferr:.1e}, min gap {min(gaps):.3f}")
        assert err < BAR and lerr < BAR and ferr < BAR
        if min(gaps) > 1e-3:
            assert toks[b] == wt, (b, toks[b], wt)
