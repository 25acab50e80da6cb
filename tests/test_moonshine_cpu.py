"""Moonshine's host schedule on the CPU: ``mlx_audio_amd/stt/models/moonshine`` over float64 emulations of the entry points' contracts
(``tests/_ops_emu_moonshine.py``) against the reference's own runs (``tests/golden/ref_moonshine.npz`` / ``.json``) at 2e-5 of the peak -- the
project's bar for this layer (``test_mossformer2_cpu.py``) -- and against the float64 restatement ``tests/_moonshine_ref.py``; parameter names,
config, sanitize rules, the fc1 interleave, the length arithmetic and every refusal by name."""
import numpy as np
import pytest
import torch

import _moonshine_ref as R
import _ops_emu_moonshine
from mlx_audio_amd.stt.models.moonshine.moonshine import Model, ModelConfig, expected_shapes, make_moonshine_weights, stem_lengths

BAR = 2e-5


def build(tag, **kw):
    cc = R.CONFIGS[tag]
    c = R.make_config(dict(cc["cfg"], **kw))
    w = make_moonshine_weights(c, cc["seed_w"], logit_gain=cc["logit_gain"], eos_gain=cc["eos_gain"])
    return Model(c, w, device="cpu"), c, w


@pytest.mark.parametrize("tag", ["A", "B"])
def test_schedule_against_the_reference_runs(tag):
    z, meta = R.load_fixtures()
    with _ops_emu_moonshine.patched():
        model, c, w = build(tag)
        for i in range(len(R.CONFIGS[tag]["clips"])):
            R.check_clip(model, z, meta, tag, i, BAR, "moonshine_cpu", report=print)


@pytest.mark.parametrize("tag,kw", [("A", {}), ("B", dict(decoder_num_key_value_heads=2)), ("A", dict(attention_bias=True))])
def test_schedule_against_the_restatement(tag, kw):
    """Also what the reference cannot run: grouped kv heads in the decoder (it concatenates unrepeated keys to a repeated cache) and attention biases;
    a ragged batch of three clips against its items."""
    with _ops_emu_moonshine.patched():
        model, c, w = build(tag, **kw)
        w64 = R.to64(w)
        clips = [R.synth_audio(7 + j, n) for j, n in enumerate((895, 3000, 1500))]
        out, frames = model.encode(clips)
        assert frames == [stem_lengths(len(a))[2] for a in clips]
        toks = model.decode_greedy(out, frames, max_tokens=6)
        for b, a in enumerate(clips):
            st = {}
            want = R.encoder64(w64, c, a, st)
            got = out[b, :frames[b]].double()
            assert float((got - want).abs().max() / want.abs().max()) < BAR
            wt, rows, gaps = R.greedy64(w64, c, want, max_tokens=6)
            if min(gaps) > 1e-3:
                assert toks[b] == wt, (b, toks[b], wt)
            h1, cache = model(torch.tensor([R.FORCED[:3]]), out[b:b + 1, :frames[b]].contiguous())
            h2, _ = model(torch.tensor([R.FORCED[3:]]), out[b:b + 1, :frames[b]].contiguous(), cache)
            wh = R.decoder64(w64, c, R.FORCED, want)
            assert float((torch.cat([h1[0], h2[0]]).double() - wh).abs().max() / wh.abs().max()) < BAR


def test_parameter_names_and_shapes_are_the_reference_module_s():
    z, meta = R.load_fixtures()
    for tag, cc in R.CONFIGS.items():
        names = sorted(expected_shapes(R.make_config(cc["cfg"])))
        assert names == meta["configs"][tag]["names"]   # the reference's load_weights(strict=True) took exactly these, shapes checked by it
    assert len(expected_shapes(R.make_config(R.CONFIGS["A"]["cfg"]))) == 60
    assert len(expected_shapes(R.make_config(R.CONFIGS["B"]["cfg"]))) == 61


def test_config_defaults_and_from_dict():
    c = ModelConfig()
    assert (c.vocab_size, c.hidden_size, c.intermediate_size, c.encoder_num_hidden_layers, c.decoder_num_hidden_layers) == (32768, 288, 1152, 6, 6)
    assert c.encoder_num_key_value_heads == c.decoder_num_key_value_heads == 8 and c.partial_rotary_factor == 0.9 and c.rope_theta == 10000.0
    assert (c.bos_token_id, c.eos_token_id, c.decoder_start_token_id, c.tie_word_embeddings, c.max_position_embeddings) == (1, 2, 1, True, 512)
    c = ModelConfig.from_dict(dict(hidden_size=416, decoder_num_key_value_heads=4, not_a_field=3))
    assert c.hidden_size == 416 and c.decoder_num_key_value_heads == 4 and c.encoder_num_key_value_heads == 8 and not hasattr(c, "not_a_field")


def test_sanitize_rules():
    with _ops_emu_moonshine.patched():
        model, c, w = build("A")
        raw = {"model.encoder.conv2.weight": torch.zeros(4, 3, 7), "model.decoder.norm.weight": torch.ones(3), "proj_out.weight": torch.ones(2, 2),
               "other": torch.ones(1)}
        s = model.sanitize(raw)
        assert set(s) == {"encoder.conv2.weight", "decoder.norm.weight", "other"} and tuple(s["encoder.conv2.weight"].shape) == (4, 7, 3)
        untied, _, _ = build("B")
        assert "proj_out.weight" in untied.sanitize(raw)
        pt = {("model." + k if k.startswith(("encoder.", "decoder.")) else k): (v.permute(0, 2, 1) if v.dim() == 3 else v) for k, v in w.items()}
        again = model.sanitize(pt)
        assert set(again) == set(w) and all(torch.equal(again[k], w[k]) for k in w)


def test_fc1_interleave_is_exact_against_the_split_form():
    g = torch.Generator().manual_seed(3)
    I, d = 10, 8
    # small integers: every product and sum is exact in float32, so the comparison does not depend on how a BLAS orders a row's sum
    wt, b, h = (torch.randint(-4, 5, sh, generator=g).float() for sh in ((2 * I, d), (2 * I,), (5, d)))
    wi, bi = Model.interleave_fc1(wt, b)
    y = h @ wt.T + b
    x, gate = y[:, :I], y[:, I:]
    yi = h @ wi.T + bi
    assert torch.equal(yi[:, 0::2], gate) and torch.equal(yi[:, 1::2], x)
    out = torch.empty(1, 5, I)
    assert torch.equal(_ops_emu_moonshine.swiglu(yi[None], out)[0], (torch.nn.functional.silu(gate.double()) * x.double()).float())


def test_length_arithmetic():
    assert stem_lengths(894) == (12, 2, 0) and stem_lengths(895) == (13, 3, 1) and stem_lengths(896) == (13, 3, 1)
    assert stem_lengths(1086) == (15, 3, 1) and stem_lengths(1087) == (16, 4, 1)
    for n in (895, 896, 1086, 1087, 1279, 5000, 16000):   # against the convolutions themselves
        x = torch.zeros(1, 1, n)
        for k, s, ch in ((127, 64, 1), (7, 3, 1), (3, 2, 1)):
            x = torch.nn.functional.conv1d(x, torch.zeros(1, ch, k), stride=s)
        assert x.shape[2] == stem_lengths(n)[2]
    assert stem_lengths(480000) == (7499, 2498, 1248)   # 30 s: 41.6 frames / s


def test_refusals_by_name():
    with _ops_emu_moonshine.patched():
        with pytest.raises(NotImplementedError, match="encoder_hidden_act 'silu'"):
            build("A", encoder_hidden_act="silu")
        for heads, width in ((2, 72), (9, 16)):
            with pytest.raises(NotImplementedError, match=f"head width {width}"):
                build("A", encoder_num_attention_heads=heads, encoder_num_key_value_heads=heads)
        with pytest.raises(NotImplementedError, match="head width 64"):
            build("A", hidden_size=256)
        model, c, w = build("A")
        with pytest.raises(ValueError, match="894 samples is shorter than 895"):
            model.generate(np.zeros(894, dtype=np.float32))
        with pytest.raises(NotImplementedError, match="bf16"):
            model.load_weights({k: v.to(torch.bfloat16) for k, v in w.items()})
        with pytest.raises(NotImplementedError, match="quantised"):
            model.load_weights(dict(w, **{"encoder.conv1.weight": torch.zeros(144, 127, 1, dtype=torch.uint8)}))
        with pytest.raises(FileNotFoundError, match="hub download is not built"):
            Model.from_pretrained("someone/moonshine-tiny")
        with pytest.raises(ValueError, match="missing parameters"):
            model.load_weights({k: v for k, v in w.items() if k != "decoder.norm.weight"})
        with pytest.raises(TypeError, match="Unsupported audio type"):
            model.generate({"audio": 1})
        assert model._decode_tokens([65, 66, 127, 128, 300]) == "AB\x7f<128><300>" and model.sample_rate == 16000


def test_abi_is_unchanged():
    from mlx_audio_amd import _lib

    assert _lib.load().mi355_abi_version() == 37 == _lib.ABI_VERSION


def test_the_generic_loader_and_the_registry_do_not_build_moonshine():
    """Like Parakeet and SenseVoice: the package exports no ``Model``, so neither the registry's scan nor ``get_model_class`` takes the family."""
    import mlx_audio_amd.stt.models.moonshine as pkg
    from mlx_audio_amd import registry
    from mlx_audio_amd.stt.utils import MODEL_REMAPPING
    from mlx_audio_amd.utils import get_model_class

    assert not hasattr(pkg, "Model") and "moonshine" not in MODEL_REMAPPING and "moonshine" not in MODEL_REMAPPING.values()
    assert "moonshine" not in registry.supported_model_types("stt")
    with pytest.raises(ValueError, match="Model type moonshine not supported for stt"):
        get_model_class("moonshine", None, "stt", MODEL_REMAPPING)
    with pytest.raises(ValueError, match="Model type sensevoice not supported for stt"):
        get_model_class("sensevoice", None, "stt", MODEL_REMAPPING)
