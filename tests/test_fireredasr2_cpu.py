"""FireRedASR2's host schedule on the CPU: ``mlx_audio_amd/stt/models/fireredasr2`` over float64 emulations of the entry points' contracts
(``tests/_ops_emu_fireredasr2.py`` and the modules it chains) against the reference's own runs (``tests/golden/ref_fireredasr2.npz`` / ``.json``) at
2e-5 of the peak -- the project's bar for this layer -- with every step decision whose margin is at least ``_margin.THR`` equal; the float64
restatement ``tests/_fireredasr2_ref.py`` against the same runs; parameter names, config round trips, the sanitize rules, ``from_pretrained`` from a
written directory, the reference's own test intent (shapes; ``beam_size=1, max_len=10``) and every refusal by name."""
import json
import os

import numpy as np
import pytest
import torch

import _fireredasr2_ref as R
import _margin
import _ops_emu_fireredasr2 as EMU
from mlx_audio_amd.stt.models.fireredasr2 import DecoderConfig, EncoderConfig, ModelConfig, expected_shapes, make_fireredasr2_weights
from mlx_audio_amd.stt.models.fireredasr2.fireredasr2 import FireRedASR2, Model, encoder_frames

BAR = 2e-5


def build(tag, ending="late", tmp=None):
    cc = R.CONFIGS[tag]
    c = R.make_config(cc["cfg"])
    w = R.eos_variant(make_fireredasr2_weights(c, cc["seed_w"], logit_gain=cc["logit_gain"], eos_gain=cc["eos_gain"]), c, ending)
    model = Model(c, w, device="cpu")
    if tmp is not None:
        R.write_side_files(tag, str(tmp), c)
        Model.post_load_hook(model, tmp)
    return model, c, w


@pytest.mark.parametrize("tag", ["A", "B"])
def test_schedule_against_the_reference_runs(tag, tmp_path):
    z, meta = R.load_fixtures()
    with EMU.patched():
        models = {e: build(tag, e, tmp_path)[0] for e in R.ENDINGS}
        encs = {}
        for i in range(len(R.CONFIGS[tag]["clips"])):
            encs[i] = R.check_encoder(models["late"], z, tag, i, BAR)
        total = [0, 0]
        for run in meta["configs"][tag]["runs"]:
            enc, rows = encs[run["clip"]]
            n, m = R.check_run(models[run["ending"]], z, run, enc, rows, "fireredasr2_cpu")
            total[0] += n
            total[1] += m
        assert total[0] >= 0.9 * total[1], total


@pytest.mark.parametrize("tag", ["A", "B"])
def test_restatement_against_the_reference_runs(tag):
    """The float64 restatement from the stored features: stages at 2e-5 of the peak (the reference ran in float32), decisions through the margin
    rule, final sequence length and confidence where no knife edge was met."""
    z, meta = R.load_fixtures()
    cc = R.CONFIGS[tag]
    c = R.make_config(cc["cfg"])
    base = make_fireredasr2_weights(c, cc["seed_w"], logit_gain=cc["logit_gain"], eos_gain=cc["eos_gain"])
    encs = {}
    for i in range(len(cc["clips"])):
        st = R.encode(base, c, z[f"{tag}{i}_feats"])
        assert st["out"].shape[0] == encoder_frames(z[f"{tag}{i}_feats"].shape[0])
        for key, got in (("sub", st["sub"]), ("attn0", st["attn0"]), ("conv0", st["conv0"]), ("enc", st["out"])):
            assert R.rel_err(got.numpy()[z[f"{tag}{i}_{key}_rows"]], z[f"{tag}{i}_{key}"]) < BAR, (tag, i, key)
        for l, got in enumerate(st["layers"]):
            assert R.rel_err(got.numpy()[z[f"{tag}{i}_enc_rows"]], z[f"{tag}{i}_layer{l}"]) < BAR, (tag, i, l)
        encs[i] = st["out"]
    for run in meta["configs"][tag]["runs"]:
        if run["clip"] == 3:
            continue   # 75 steps of the full-prefix restatement: the shorter clips cover every ending
        key, B = run["key"], run["beam"]
        res = R.beam_search(R.eos_variant(base, c, run["ending"]), c, encs[run["clip"]], beam_size=B, max_len=run.get("max_len", 0))
        got, exp, mar = [], [], []
        for s, step in enumerate(res["steps"][:len(z[f"{key}_margin"])]):
            got += step["beam_idx"] + step["tokens"]
            exp += z[f"{key}_beam_idx"][s].tolist() + z[f"{key}_tokens"][s].tolist()
            mar += [float(z[f"{key}_margin"][s])] * (2 * B)
        if _margin.walk("fireredasr2_restatement", got, exp, mar, where=key) == len(mar):
            assert len(res["seq"]) == run["generation_tokens"] and abs(res["confidence"] - run["confidence"]) <= 2e-3, (key, res["seq"], run)
            assert R.detokenize([" " if t == "<space>" else t for t in R.make_dict(c.odim)], res["seq"]) == run["text"]


def test_a_ragged_batch_equals_its_items():
    """``generate_batch``'s path on three clips of different lengths: encoder rows and every beam decision of an item inside the batch equal the
    item alone (the emulations are float64: equal to rounding)."""
    with EMU.patched():
        model, c, w = build("A")
        z, _ = R.load_fixtures()
        feats = [torch.from_numpy(z[f"A{i}_feats"]) for i in (1, 0, 2)]
        ns = [f.shape[0] for f in feats]
        buf = torch.zeros((3, max(ns) + 6, c.idim))
        for b, f in enumerate(feats):
            buf[b, :ns[b]] = f
        out, rows = model.encode_features(buf, ns)
        hyps = model.beam_search(out, rows, beam_size=3)
        for b, f in enumerate(feats):
            one = torch.zeros((1, ns[b] + 6, c.idim))
            one[0, :ns[b]] = f
            o1, r1 = model.encode_features(one, [ns[b]])
            assert r1[0] == rows[b] == encoder_frames(ns[b])
            assert R.rel_err(out[b, :rows[b]].numpy(), o1[0, :r1[0]].numpy()) < 1e-6
            h1 = model.beam_search(o1, r1, beam_size=3)
            assert h1[0][0] == hyps[b][0] and np.allclose(h1[0][1], hyps[b][1], atol=1e-6)


def test_reference_test_intent_shapes_and_short_beam():
    """stt/tests/test_fireredasr2.py: the encoder output is [1, T', d_model]; ``beam_size=1, max_len=10`` gives at most 10 tokens."""
    with EMU.patched():
        model, c, w = build("B")
        z, _ = R.load_fixtures()
        f = torch.from_numpy(z["B2_feats"])
        buf = torch.zeros((1, f.shape[0] + 6, c.idim))
        buf[0, :f.shape[0]] = f
        out, rows = model.encode_features(buf, [f.shape[0]])
        assert tuple(out.shape) == (1, encoder_frames(f.shape[0]), c.encoder.d_model)
        seq, conf = model.beam_search(out, rows, beam_size=1, max_len=10)[0]
        assert len(seq) <= 10 and len(conf) == len(seq) and all(0.0 <= v <= 1.0 for v in conf)


def test_parameter_names_and_shapes_are_the_reference_module_s():
    _, meta = R.load_fixtures()
    for tag, cc in R.CONFIGS.items():
        assert sorted(expected_shapes(R.make_config(cc["cfg"]))) == meta["configs"][tag]["names"]


def test_config_round_trips():
    c = ModelConfig.from_dict(dict(odim=77, bogus=1, encoder=dict(n_layers=3, n_head=4, d_model=256, kernel_size=15, junk=2), decoder=dict(n_layers=5)))
    assert (c.odim, c.encoder.n_layers, c.encoder.kernel_size, c.decoder.n_layers, c.decoder.d_model, c.sos_id, c.eos_id) == (77, 3, 15, 5, 1280, 3, 4)
    assert ModelConfig.from_dict(c.to_dict()) == c
    d = ModelConfig()
    assert (d.model_type, d.idim, d.odim, d.d_model, d.pad_id, d.blank_id) == ("fireredasr2", 80, 8667, 1280, 2, 0)
    assert d.encoder == EncoderConfig(16, 20, 1280, 33, 5000) and d.decoder == DecoderConfig(16, 20, 1280, 5000)


def test_sanitize_rules():
    t = torch.zeros
    w = {"encoder.input_preprocessor.conv.0.weight": t(32, 1, 3, 3), "encoder.input_preprocessor.conv.2.weight": t(32, 32, 3, 3),
         "encoder.input_preprocessor.conv.0.bias": t(32), "encoder.layer_stack.0.ffn1.net.1.weight": t(8, 2), "encoder.layer_stack.0.ffn2.net.4.bias": t(2),
         "encoder.layer_stack.0.conv.pointwise_conv1.weight": t(8, 2, 1), "encoder.layer_stack.0.conv.depthwise_conv.weight": t(4, 1, 33),
         "encoder.layer_stack.0.conv.pointwise_conv2.weight": t(2, 4, 1), "decoder.tgt_word_emb.weight": torch.arange(6.0).reshape(3, 2)}
    s = FireRedASR2.sanitize(None, w)
    assert tuple(s["encoder.input_preprocessor.conv1.weight"].shape) == (32, 3, 3, 1) and tuple(s["encoder.input_preprocessor.conv2.weight"].shape) == (32, 3, 3, 32)
    assert "encoder.input_preprocessor.conv1.bias" in s and "encoder.layer_stack.0.ffn1.net_1.weight" in s and "encoder.layer_stack.0.ffn2.net_4.bias" in s
    assert tuple(s["encoder.layer_stack.0.conv.pointwise_conv1.weight"].shape) == (8, 1, 2)
    assert tuple(s["encoder.layer_stack.0.conv.depthwise_conv.weight"].shape) == (4, 33, 1)
    assert tuple(s["encoder.layer_stack.0.conv.pointwise_conv2.weight"].shape) == (2, 1, 4)
    assert torch.equal(s["decoder.tgt_word_prj.weight"], w["decoder.tgt_word_emb.weight"])          # the weight tying
    s2 = FireRedASR2.sanitize(None, dict(w, **{"decoder.tgt_word_prj.weight": t(3, 2)}))
    assert not s2["decoder.tgt_word_prj.weight"].any()                                              # an own projection is kept


def test_from_pretrained_from_a_written_directory(tmp_path):
    from safetensors.torch import save_file

    cc = R.CONFIGS["B"]
    c = R.make_config(cc["cfg"])
    w = make_fireredasr2_weights(c, cc["seed_w"])
    torch_names = {}
    for k, v in w.items():      # back to the PyTorch checkpoint's names and layouts, the projection left out (tied)
        if k == "decoder.tgt_word_prj.weight":
            continue
        nk = k.replace("input_preprocessor.conv1.", "input_preprocessor.conv.0.").replace("input_preprocessor.conv2.", "input_preprocessor.conv.2.")
        nk = nk.replace(".net_", ".net.")
        if "pointwise_conv" in k or "depthwise_conv" in k:
            v = v.permute(0, 2, 1)
        elif "input_preprocessor.conv" in k and v.dim() == 4:
            v = v.permute(0, 3, 1, 2)
        torch_names[nk] = v.contiguous()
    save_file(torch_names, str(tmp_path / "model.safetensors"))
    with open(tmp_path / "config.json", "w") as f:
        json.dump(c.to_dict(), f)
    R.write_side_files("B", str(tmp_path), c)
    with EMU.patched():
        model = Model.from_pretrained(tmp_path, device="cpu")
        assert model.config == c and model._cmvn is not None and model._tokenizer[5] == " " and len(model._tokenizer) == c.odim
        assert torch.equal(model.embed, w["decoder.tgt_word_emb.weight"])
        assert model._detokenize([7, 9, 0, 6, 100000]) == R.detokenize(model._tokenizer, [7, 9, 0, 6])
        with pytest.raises(FileNotFoundError, match="hub download is not built"):
            Model.from_pretrained(tmp_path / "nowhere", device="cpu")


def test_refusals_by_name():
    cfg = lambda **kw: dict(odim=50, encoder=dict(n_layers=1, n_head=kw.get("eh", 2), d_model=128), decoder=dict(n_layers=1, n_head=kw.get("dh", 2), d_model=128))
    with EMU.patched():
        with pytest.raises(NotImplementedError, match="head width 32"):
            Model(cfg(eh=4), device="cpu")
        with pytest.raises(NotImplementedError, match="decoder head width 16"):
            Model(cfg(dh=8), device="cpu")
        model = Model(cfg(), device="cpu")
        enc = torch.zeros((1, 3, 128))
        with pytest.raises(NotImplementedError, match="beam_size 9"):
            model.beam_search(enc, [3], beam_size=9)
        w = make_fireredasr2_weights(model.config)
        with pytest.raises(NotImplementedError, match="bf16 checkpoints are not built"):
            model.load_weights({k: v.to(torch.bfloat16) for k, v in w.items()})
        with pytest.raises(NotImplementedError, match="quantised checkpoints are not built"):
            model.load_weights(dict(w, **{"decoder.tgt_word_emb.weight": torch.zeros((50, 128), dtype=torch.uint8)}))
        with pytest.raises(ValueError, match="missing parameters"):
            model.load_weights({k: v for k, v in w.items() if "layer_norm_out" not in k})
        with pytest.raises(ValueError, match="shorter than one fbank frame"):
            model.features([np.zeros(100, dtype=np.float32)])
