"""Granite Speech NAR without a GPU: the host schedule of ``stt/models/granite_speech_nar`` over float64 statements of every kernel it calls
(``_ops_emu_granite_nar.patched_model``) against the runs of the reference's own files stored by ``tests/golden/make_granite_nar_fixtures.py`` -- every
stage within the project's CPU bar of 2e-5 of the stage's peak, every decision and the final ids equal -- and the package's own surface: configs,
``sanitize``, ``from_pretrained`` on a written directory with a local tokenizer, the refusals by name, the slot / collapse utilities."""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import _granite_nar_ref as R  # noqa: E402
import _ops_emu_granite_nar as E  # noqa: E402

from mlx_audio_amd.stt.models.granite_speech_nar import (EncoderConfig, GraniteSpeechNar as Model, ModelConfig, ProjectorConfig, TextConfig, add_insertion_slots,  # noqa: E402
                                                         ctc_collapse_decode, make_granite_nar_weights)

CPU_BAR = 2e-5


@pytest.fixture(scope="module")
def fixture():
    return R.load_fixture()


@pytest.mark.parametrize("tag", ["A", "B"])
def test_host_schedule_reproduces_the_stored_runs(fixture, tag):
    fx, meta = fixture
    worst = {}
    with E.patched_model():
        model = R.build_model(tag, "cpu")
        feats = [R.stored_features(fx, i) for i in range(len(R.CLIPS))]
        for i, f in enumerate(feats):
            final, st = model.transcribe_batch(f[None], return_stages=True)
            assert final[0] == meta["configs"][tag]["decode"][i]["final"] == model._transcribe_tokens(f)
            for k, v in R.compare_clip(st, fx, tag, i).items():
                worst[k] = max(worst.get(k, 0.0), v)
        # the five clips as ONE right-padded batch: every item as that item alone
        fb, lens = model._pad(feats)
        final, st = model.transcribe_batch(fb, lens, return_stages=True)
        for i in range(len(feats)):
            for k, v in R.compare_clip(st, fx, tag, i, b=i).items():
                worst[k] = max(worst.get(k, 0.0), v)
    print(f"config {tag}: worst error / peak per stage:", {k: f"{v:.1e}" for k, v in worst.items()})
    assert max(worst.values()) <= CPU_BAR, worst


def test_front_end_reproduces_the_stored_features(fixture):
    fx, _ = fixture
    with E.patched_model():
        model = R.build_model("A", "cpu")
        for i, (n, seed) in enumerate(R.CLIPS):
            f = model._compute_features(R.synth_audio(n, seed))
            assert f.shape == (n // 320, 160)
            want = fx[f"feat{i}"]
            assert float((f[fx[f"feat{i}_rows"].astype(np.int64)] - torch.from_numpy(want)).abs().max()) <= CPU_BAR * float(np.abs(want).max())
        out = model.generate(R.synth_audio(*R.CLIPS[1]))
        assert out.text == " ".join(f"t{t}" for t in fx["A1_final"])
        with pytest.raises(ValueError, match="too short"):
            model._compute_features(np.zeros(300, dtype=np.float32))


def test_config_round_trips():
    for tag in "AB":
        d = R.config_dict(tag)
        cfg = ModelConfig.from_dict(d)
        assert isinstance(cfg.encoder, EncoderConfig) and isinstance(cfg.projector, ProjectorConfig) and isinstance(cfg.text, TextConfig)
        assert cfg.text.rope_theta == d["text_config"]["rope_parameters"]["rope_theta"] and cfg.encoder.context_size == d["encoder_config"]["context_size"]
        assert cfg.to_dict() == d and ModelConfig.from_dict(json.loads(json.dumps(cfg.to_dict()))) == cfg
    bad = R.config_dict("A")
    del bad["encoder_config"]["max_pos_emb"]
    with pytest.raises(KeyError):
        ModelConfig.from_dict(bad)


def test_sanitize_and_quant_predicate():
    w = {"encoder.layers.0.conv.bn.num_batches_tracked": torch.zeros(()), "encoder.layers.0.conv.bn.weight": torch.ones(4)}
    assert list(Model.sanitize(w)) == ["encoder.layers.0.conv.bn.weight"]
    assert Model.model_quant_predicate(None, "editor.layers.0.mlp.up_proj") and not Model.model_quant_predicate(None, "encoder.out")


def test_from_pretrained_on_a_written_directory(tmp_path, fixture):
    from safetensors.torch import save_file
    from tokenizers import Tokenizer, models, pre_tokenizers
    from transformers import PreTrainedTokenizerFast

    fx, _ = fixture
    cfg = ModelConfig.from_dict(R.config_dict("A"))
    w = make_granite_nar_weights(cfg, **R.WEIGHTS["A"])
    w["encoder.layers.0.conv.bn.num_batches_tracked"] = torch.zeros((), dtype=torch.int64)
    (tmp_path / "config.json").write_text(json.dumps(cfg.to_dict()))
    save_file({k: v.contiguous() for k, v in w.items()}, str(tmp_path / "model.safetensors"))
    tok = Tokenizer(models.WordLevel({f"w{i}": i for i in range(R.VOCAB - 1)} | {"<blank>": R.BLANK}, unk_token="<blank>"))
    tok.pre_tokenizer = pre_tokenizers.Whitespace()
    PreTrainedTokenizerFast(tokenizer_object=tok, unk_token="<blank>").save_pretrained(str(tmp_path))
    with E.patched_model():
        model = Model.from_pretrained(tmp_path, device="cpu")
        assert ModelConfig.from_pretrained(tmp_path) == cfg and model._tokenizer is not None
        out = model.generate(R.synth_audio(*R.CLIPS[1]))
        assert out.text == " ".join(f"w{t}" for t in fx["A1_final"])
        path = tmp_path / "clip.wav"
        from mlx_audio_amd import audio_io

        audio_io.write(str(path), R.synth_audio(*R.CLIPS[1]), 8000)
        with pytest.raises(ValueError, match="audio must be 16000 Hz; got 8000"):
            model.generate(str(path))
        with pytest.raises(FileNotFoundError, match="hub download is not built"):
            Model.post_load_hook(model, "ibm-granite/granite-speech-nar")
        with pytest.raises(FileNotFoundError, match="hub download"):
            Model.from_pretrained("ibm-granite/granite-speech-nar", device="cpu")


def test_refusals_by_name():
    d = R.config_dict("A")
    with E.patched_model():
        cfg = ModelConfig.from_dict(d)
        w = make_granite_nar_weights(cfg, seed=0)
        with pytest.raises(NotImplementedError, match="bf16 checkpoints are not built"):
            Model(cfg, {k: v.to(torch.bfloat16) for k, v in w.items()}, device="cpu")
        with pytest.raises(NotImplementedError, match="quantised checkpoints are not built"):
            Model(cfg, dict(w, **{"editor.layers.0.mlp.up_proj.scales": torch.zeros(1)}), device="cpu")
        with pytest.raises(ValueError, match="missing parameters"):
            Model(cfg, {k: v for k, v in w.items() if k != "encoder.out.bias"}, device="cpu")
        for section, field, value, match in (("encoder_config", "dim_head", 32, "encoder dim_head 32 is not built"),
                                             ("text_config", "num_attention_heads", 4, "editor head width 128/4 is not built"),
                                             ("projector_config", "num_heads", 4, "projector head width 128/4 is not built")):
            bad = json.loads(json.dumps(d))
            bad[section][field] = value
            with pytest.raises(NotImplementedError, match=match):
                Model(ModelConfig.from_dict(bad), device="cpu")
        model = Model(cfg, w, device="cpu")
        with pytest.raises(RuntimeError, match="Tokenizer not loaded"):
            model.generate(np.zeros(16000, dtype=np.float32))
        with pytest.raises(ValueError, match="features must be"):
            model.transcribe_batch(torch.zeros(1, 4, 80))
        with pytest.raises(ValueError, match="lengths"):
            model.transcribe_batch(torch.zeros(2, 4, 160), [4, 0])
    import mlx_audio_amd.stt.utils as U

    assert "granite_speech_nar" not in json.dumps(sorted(map(str, getattr(U, "MODEL_REMAPPING", {}).items())))


def test_insertion_slots_and_collapse_on_scripted_ids():
    B = 9
    assert add_insertion_slots([], B, 8) == [B] * 8                               # n == 0: min_len blanks
    assert add_insertion_slots([5], B, 8) == [B, 5, B, B, B, B, B, B]             # 2 N + 1 < min_len: padded with blanks
    assert add_insertion_slots([1, 2, 3, 4], B, 8) == [B, 1, B, 2, B, 3, B, 4, B]  # 2 N + 1 > min_len
    assert add_insertion_slots([7, 7], B, 3) == [B, 7, B, 7, B]
    assert ctc_collapse_decode([], B) == [] and ctc_collapse_decode([B, B, B], B) == []
    assert ctc_collapse_decode([1, 1, B, 1, 2, 2, B, B, 3], B) == [1, 1, 2, 3]   # dedup, THEN blanks: a, blank, a keeps both
    assert ctc_collapse_decode(add_insertion_slots([4, 4, 5], B, 8), B) == [4, 4, 5]


@pytest.mark.parametrize("tag,clip", [("A", 2), ("A", 4), ("B", 1), ("B", 4)])
def test_float64_restatement_reproduces_the_stored_runs(fixture, tag, clip):
    """The TEST SIDE: ``_granite_nar_ref.reference_forward`` (what the published-width GPU test holds the device to) against the stored runs of the
    reference's own files: decisions equal, stages within the float32 rounding of the stored run."""
    fx, _ = fixture
    cfg = ModelConfig.from_dict(R.config_dict(tag))
    r = R.reference_forward(cfg, make_granite_nar_weights(cfg, **R.WEIGHTS[tag]), R.stored_features(fx, clip))
    key = lambda k: fx[f"{tag}{clip}_{k}"]
    assert r["bpe_ids"] == key("bpe_ids").tolist() and r["hyp"] == key("hyp").tolist() and r["edit_ids"] == key("edit_ids").tolist()
    assert r["final"] == key("final").tolist()
    for k in ("pooled", "tail_logits"):
        want = torch.from_numpy(key(k)).double()
        assert float((r[k] - want).abs().max() / want.abs().max()) <= CPU_BAR, k
    wins = key("windows").astype(np.int64)
    want = torch.from_numpy(key("audio")).double()
    assert float((r["audio"].reshape(-1, 3, want.shape[-1])[wins] - want).abs().max() / want.abs().max()) <= CPU_BAR
