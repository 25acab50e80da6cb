"""Sortformer without a GPU: the float64 restatement and the engine's host schedule (over CPU emulations of the operator contracts) against the
reference's own runs (``tests/golden/ref_sortformer.npz`` / ``.json``), the host logic on the reference's scripted rows, the configs and the refusals."""
import dataclasses
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
GOLD = os.path.join(HERE, "golden")

import _margin  # noqa: E402
import _sortformer_ref as R  # noqa: E402


def rel_peak(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLD, "ref_sortformer.npz"))


@pytest.fixture(scope="module")
def meta():
    with open(os.path.join(GOLD, "ref_sortformer.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def models(meta):
    return R.load_models(meta)


def test_inputs_regenerate(fx, models):
    for tag, (_, _, feats) in models.items():
        for i, f in enumerate(feats):
            s = np.array([f.astype(np.float64).sum(), (f.astype(np.float64) ** 2).sum()])
            assert np.allclose(s, fx[f"{tag}{i}_featsum"], rtol=1e-12, atol=0), (tag, i)
    k = R.STREAM
    w = R.synth_wave(k["seed"], k["chunks"] * k["chunk_samples"]).astype(np.float64)
    assert np.allclose([w.sum(), (w ** 2).sum()], fx["stream_wavesum"], rtol=1e-12, atol=0)


def test_seeded_weights_have_the_reference_names_and_fp16_values(models):
    from mlx_audio_amd.vad.models.sortformer.sortformer import expected_shapes

    cfg, w, _ = models["A"]
    assert all(torch.equal(v, v.to(torch.float16).to(torch.float32)) for v in w.values())
    assert set(w) == set(expected_shapes(cfg))
    for name in ("fc_encoder.subsampling.layers_0.weight", "fc_encoder.subsampling.layers_6.bias", "fc_encoder.subsampling.linear.weight",
                 "fc_encoder.layers.1.self_attn.relative_k_proj.weight", "fc_encoder.layers.0.self_attn.bias_u", "fc_encoder.layers.0.conv.norm.running_var",
                 "tf_encoder.embed_positions.weight", "tf_encoder.layers.1.self_attn.out_proj.bias", "sortformer_modules.hidden_to_spks.weight"):
        assert name in w, name
    assert "tf_encoder.layers.0.self_attn.k_proj.bias" not in w and w["fc_encoder.layers.0.conv.depthwise_conv.weight"].shape == (128, 9, 1)
    cfg_b, w_b, _ = models["B"]
    assert "tf_encoder.layers.0.self_attn.k_proj.bias" in w_b and "fc_encoder.layers.0.self_attn.q_proj.bias" not in w_b
    assert "fc_encoder.layers.0.feed_forward1.linear1.bias" in w_b   # attention_bias removes the attention biases alone


def test_restatement_pinned_to_the_reference_runs(fx, models):
    """float64 against the reference's float32 runs: stage tensors within 2e-5 of the peak, decisions equal wherever |z| is at least THR."""
    for tag, (cfg, w, feats) in models.items():
        for i, f in enumerate(feats):
            r = R.forward(cfg, w, f)
            assert r["preds"].shape[0] == int(fx[f"{tag}{i}_out_len"])
            for got, key in ((r["encoder_proj"], "encoder_proj"), (r["tf_layers"], "layers"), (r["logits"], "logits"), (r["preds"], "preds")):
                assert rel_peak(got.numpy(), fx[f"{tag}{i}_{key}"]) < 2e-5, (tag, i, key)
            z = fx[f"{tag}{i}_logits"]
            ok = np.abs(z) >= _margin.THR
            assert np.array_equal((r["preds"].numpy() > 0.5)[ok], (fx[f"{tag}{i}_preds"] > 0.5)[ok])


def test_host_schedule_dry_run(fx, meta, models):
    """The engine's host schedule (the name adapter, the scale in front of ``Conformer.encode``, positions through ``res=``, the fused q | k | v views
    with a zero k bias, LN(x + res), the ReLU prologue of the head, the row mask) over CPU emulations of the operator contracts, against the
    reference's runs: every clip alone and all clips of a config as one padded batch; then the segments."""
    import _ops_emu_sortformer
    from mlx_audio_amd.vad.models.sortformer import Model

    with _ops_emu_sortformer.patched():
        for tag, (cfg, w, feats) in models.items():
            eng = Model(cfg, w, device="cpu")
            batch, lens = R.pad_batch(feats)
            runs = [(eng(torch.from_numpy(f)[None], None, return_layers=True), 0, i) for i, f in enumerate(feats)]
            rb = eng(batch, lens, return_layers=True)
            runs += [(rb, i, i) for i in range(len(feats))]
            for (preds, taps), row, i in runs:
                n = int(fx[f"{tag}{i}_out_len"])
                got = dict(encoder_proj=taps["encoder_proj"][row, :n], layers=torch.stack(taps["layers"])[:, row, :n], logits=taps["logits"][row, :n],
                           preds=preds[row, :n])
                for k, v in got.items():
                    assert rel_peak(v.numpy(), fx[f"{tag}{i}_{k}"]) < 2e-5, (tag, i, k)
                assert not preds[row, n:].any()
                z = fx[f"{tag}{i}_logits"]
                ok = np.abs(z) >= _margin.THR
                assert np.array_equal((got["preds"].numpy() > 0.5)[ok], (fx[f"{tag}{i}_preds"] > 0.5)[ok])
                if (np.abs(z) < _margin.THR).any():
                    continue
                for (t, d, g), want in zip(R.SEGMENT_SETTINGS, meta["configs"][tag]["segments"][i]):
                    segs = eng._preds_to_segments(got["preds"], frame_duration=0.08, threshold=t, min_duration=d, merge_gap=g)
                    assert R.same_segments(R.segments_list(segs), want), (tag, i, t)


def test_feed_state_bookkeeping(fx, meta, models, monkeypatch):
    """``feed`` over the fixture's 8 chunks with ``spkcache_max = fifo_max = 16`` under the emulations (the features from the numpy restatement of the
    front end): chunk preds within 2e-4 of the peak, state lengths, ``frames_processed`` and the indices every compression kept equal to the
    reference's."""
    import _ops_emu_sortformer
    from mlx_audio_amd.vad.models.sortformer import Model
    from oracle import dsp_ref

    cfg, w, _ = models["A"]
    k = meta["stream"]
    wave = R.synth_wave(k["seed"], k["chunks"] * k["chunk_samples"])
    kept = []
    orig = Model._simple_keep_indices
    monkeypatch.setattr(Model, "_simple_keep_indices", staticmethod(lambda preds, n: kept.append(orig(preds, n).tolist()) or torch.tensor(kept[-1])))
    with _ops_emu_sortformer.patched():
        eng = Model(cfg, w, device="cpu")
        proc = cfg.processor_config
        eng._features = lambda x, **kw: torch.from_numpy(dsp_ref.sortformer_mel_features(x.numpy(), proc.sampling_rate, proc.n_fft, proc.hop_length,
                                                                                         proc.win_length, proc.feature_size, proc.preemphasis, **kw))
        state = eng.init_streaming_state()
        for i, want in enumerate(k["steps"]):
            n0 = len(kept)
            res, state = eng.feed(wave[i * k["chunk_samples"]:(i + 1) * k["chunk_samples"]], state, spkcache_max=k["spkcache_max"], fifo_max=k["fifo_max"])
            assert rel_peak(res.speaker_probs.numpy(), fx[f"stream_preds{i}"]) < 2e-4, i
            assert (state.spkcache_len, state.fifo_len, state.frames_processed) == (want["spkcache_len"], want["fifo_len"], want["frames_processed"]), i
            assert state.spkcache_preds.shape[1] == state.spkcache_len and state.fifo_preds.shape[1] == state.fifo_len
            assert kept[n0:] == [c["indices"] for c in want["compress"]], i
    assert sum(len(s["compress"]) for s in k["steps"]) >= 2


def test_scripted_segments_trim_and_sanitize(meta):
    from mlx_audio_amd.vad.models.sortformer import Model

    s = meta["scripted"]
    for name, row in s["segments"].items():
        for (t, d, g), want in zip(s["settings"], row["results"]):
            got = Model._preds_to_segments(torch.tensor(row["preds"], dtype=torch.float32), frame_duration=0.08, threshold=t, min_duration=d, merge_gap=g)
            assert R.same_segments(R.segments_list(got), want), (name, t, d, g)
    for c in s["trim"]:
        w = np.zeros(c["lead"] + c["speech"] + c["trail"], dtype=np.float32)
        w[c["lead"]:c["lead"] + c["speech"]] = 0.5 * np.sin(np.arange(c["speech"], dtype=np.float32) * 0.3)
        if c["burst"]:
            w[1000:1000 + c["burst"]] = 0.5
        tw, off = Model._trim_silence(torch.from_numpy(w), 16000)
        assert (int(off), int(tw.shape[0])) == (c["offset"], c["length"]), c
        assert torch.equal(tw, torch.from_numpy(w)[off:off + tw.shape[0]])
    g = np.random.default_rng(5)   # the generator's checkpoints, in its order
    hf = {"fc_encoder.subsampling.layers.0.weight": (4, 1, 3, 3), "fc_encoder.subsampling.layers.2.weight": (4, 1, 3, 3), "fc_encoder.subsampling.layers.0.bias": (4,),
          "fc_encoder.subsampling.linear.weight": (6, 8), "fc_encoder.layers.0.conv.pointwise_conv1.weight": (8, 4, 1),
          "fc_encoder.layers.0.conv.depthwise_conv.weight": (4, 1, 9), "fc_encoder.layers.0.conv.norm.num_batches_tracked": None,
          "fc_encoder.layers.0.conv.norm.running_mean": (4,), "tf_encoder.layers.0.fc1.weight": (6, 4)}
    hf = {k: torch.zeros(()) if v is None else torch.from_numpy(g.standard_normal(v).astype(np.float32)) for k, v in hf.items()}
    conv = {"fc_encoder.subsampling.layers_0.weight": (4, 3, 3, 1), "fc_encoder.layers.0.conv.depthwise_conv.weight": (4, 9, 1)}
    conv = {k: torch.from_numpy(g.standard_normal(v).astype(np.float32)) for k, v in conv.items()}
    for tag, wts in (("hf", hf), ("converted", conv)):
        got = Model.sanitize(wts)
        want = s["sanitize"][tag]
        assert set(got) == set(want), tag
        for k, v in got.items():
            v = v.contiguous()
            assert list(v.shape) == want[k]["shape"] and abs(float(v.double().sum()) - want[k]["sum"]) < 1e-9, (tag, k)
            assert float(v.reshape(-1)[min(5, v.numel() - 1)]) == want[k]["first"], (tag, k)


def test_config_round_trips():
    from mlx_audio_amd.vad.models.sortformer import DETECTION_HINTS, FCEncoderConfig, ModelConfig, ModulesConfig, ProcessorConfig, TFEncoderConfig

    d = ModelConfig()
    assert (d.fc_encoder_config.hidden_size, d.fc_encoder_config.num_hidden_layers, d.fc_encoder_config.conv_kernel_size) == (512, 18, 9)
    assert (d.tf_encoder_config.d_model, d.tf_encoder_config.encoder_attention_heads, d.tf_encoder_config.encoder_ffn_dim) == (192, 8, 768)
    assert d.tf_encoder_config.max_source_positions == 1500 and d.tf_encoder_config.k_proj_bias is False
    assert (d.modules_config.num_speakers, d.modules_config.spkcache_len, d.modules_config.use_aosc) == (4, 188, False)
    assert (d.processor_config.feature_size, d.processor_config.hop_length, d.processor_config.preemphasis) == (80, 160, 0.97)
    raw = R.config_dict(R.FC_A, R.TF_A)
    raw["unknown_key"] = 1
    raw["fc_encoder_config"]["another_unknown"] = 2
    cfg = ModelConfig.from_dict(raw)
    assert isinstance(cfg.fc_encoder_config, FCEncoderConfig) and isinstance(cfg.tf_encoder_config, TFEncoderConfig)
    assert isinstance(cfg.modules_config, ModulesConfig) and isinstance(cfg.processor_config, ProcessorConfig)
    assert cfg.fc_encoder_config.hidden_size == 128 and cfg.tf_encoder_config.d_model == 48 and cfg.processor_config.feature_size == 16
    again = ModelConfig.from_dict(dataclasses.asdict(cfg))
    assert again == cfg
    assert DETECTION_HINTS["architectures"] == ["SortformerOffline"]


def test_refusals(models):
    import _ops_emu_sortformer
    from mlx_audio_amd.vad.models.sortformer import Model, StreamingState

    cfg, w, feats = models["A"]
    with _ops_emu_sortformer.patched():
        eng = Model(cfg, w, device="cpu")
        with pytest.raises(ValueError, match="max_source_positions"):
            eng(torch.zeros(1, 16, 8 * 257))   # 257 frames against 256 learned positions
        with pytest.raises(ValueError, match="features must be"):
            eng(torch.zeros(1, 17, 64))
        with pytest.raises(ValueError, match="missing"):
            Model(cfg, {k: v for k, v in w.items() if "embed_positions" not in k}, device="cpu")
        with pytest.raises(ValueError, match="unexpected"):
            Model(cfg, dict(w, extra=torch.zeros(1)), device="cpu")
        with pytest.raises(ValueError, match="head width"):
            Model(R.make_config(R.FC_A, dict(R.TF_A, encoder_attention_heads=4)), w, device="cpu")   # heads of 12
        aosc = R.make_config(R.FC_A, R.TF_A)
        aosc.modules_config.use_aosc = True
        eng2 = Model(aosc, w, device="cpu")
        assert eng2(torch.from_numpy(feats[2])[None]).shape == (1, 6, 4)   # the offline call does not depend on it
        z = torch.zeros(1, 0, 128)
        st = StreamingState(z, torch.zeros(1, 0, 4), z, torch.zeros(1, 0, 4), 0, torch.zeros(1, 128), torch.zeros(1))
        for call in (eng2.init_streaming_state, lambda: eng2.streaming_step(torch.zeros(1, 16, 64), [64], st), lambda: eng2.feed(np.zeros(8000, np.float32), st),
                     lambda: next(eng2.generate_stream(np.zeros(8000, np.float32))), lambda: Model._maybe_compress_state(st, 4, 4, aosc.modules_config)):
            with pytest.raises(NotImplementedError, match="AOSC"):
                call()
    with pytest.raises(FileNotFoundError, match="local directory"):
        Model.from_pretrained("mlx-community/diar_sortformer_4spk-v1-fp32")


def test_from_pretrained_and_load_model(tmp_path, models):
    import _ops_emu_sortformer
    from safetensors.torch import save_file

    from mlx_audio_amd.vad.models.sortformer import Model
    from mlx_audio_amd.vad.loader import load_model

    cfg, w, feats = models["A"]
    c = R.CONFIGS["A"]
    d = tmp_path / "sortformer-tiny"
    d.mkdir()
    save_file({k: v.contiguous() for k, v in w.items()}, str(d / "model.safetensors"))
    with open(d / "config.json", "w") as f:
        json.dump(R.config_dict(c["fc"], c["tf"]), f)
    x = torch.from_numpy(feats[2])[None]
    with _ops_emu_sortformer.patched():
        want = Model(cfg, w, device="cpu")(x)
        assert torch.equal(Model.from_pretrained(str(d), device="cpu")(x), want)
        eng = load_model(d, device="cpu")
        assert isinstance(eng, Model) and torch.equal(eng(x), want)


def test_entry_point_declared_and_refuses_null():
    from mlx_audio_amd import _lib

    lib = _lib.load()
    assert "mi355_narrow_attention" in _lib.declared_functions() and "mi355_narrow_attention_args" in _lib.STRUCTS
    st = _lib.STRUCTS["mi355_narrow_attention_args"]()
    assert lib.mi355_narrow_attention(__import__("ctypes").byref(st), None) != 0 and b"null" in lib.mi355_last_error()
