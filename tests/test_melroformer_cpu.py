"""Mel-Band RoFormer without a GPU: the config values the reference's own tests pin (``tests/sts/test_mel_roformer.py``), the band tables,
``sanitize``, ``from_pretrained``'s file priority / config resolution / errors, the float64 helper ``tests/_melroformer_ref.py`` held to the
reference's runs (``tests/golden/ref_melroformer.npz``, made by ``tests/golden/make_melroformer_fixtures.py``), the engine's host schedule dry-run
over CPU emulations of the operator contracts against the same runs, what is not built, and the three new C entry points of ``csrc/bandsplit.hip``."""
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

BAND_FUNCS = ("mi355_band_split", "mi355_band_merge", "mi355_head_gate")
BAND_STRUCTS = ("mi355_band_split_args", "mi355_band_merge_args", "mi355_head_gate_args")
STAGES = ("split", "tf0", "tf1", "mask")
BAR = 2e-5   # of each tensor's peak: float32 rounding of the reference's run through two transformers (the bar test_dfn_cpu.py / test_s3_cpu.py use)


def rel_peak(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


@pytest.fixture(scope="module")
def fx():
    with open(os.path.join(GOLD, "ref_melroformer.json")) as f:
        meta = json.load(f)
    return np.load(os.path.join(GOLD, "ref_melroformer.npz")), meta


def setup_config(meta, tag):
    from mlx_audio_amd.sts.models.mel_roformer import MelRoFormerConfig, make_melroformer_weights

    c = meta["configs"][tag]
    cfg = MelRoFormerConfig.custom(**c["kw"])
    calls = [np.stack([R.synth_clip(seed, n, zero) for seed, n, zero in call]) for call in c["calls"]]
    return cfg, make_melroformer_weights(cfg, meta["seed_w"]), calls


def stored(meta, key, value, T):
    """``value`` subsampled like the fixture's tensor."""
    v = np.asarray(value)
    return v[:, ::meta["stride"]] if key != "mask" and T > meta["stride_above"] else v


def stage_dict(st):
    """The engine's / helper's stages under the fixture's names."""
    g = lambda t: t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return dict(split=g(st["split"]), tf0=g(st["tf"][0]), tf1=g(st["tf"][1]), mask=g(st["mask"]))


# ------------------------------------------------------------------------------------------------ config
def test_config_defaults_properties_and_presets():
    """The numbers of the reference's ``TestMelRoFormerConfig``, and the fourth preset's (config.py:137-143)."""
    from mlx_audio_amd.sts.models import mel_roformer as M
    from mlx_audio_amd.sts.models.mel_roformer import MelRoFormer, MelRoFormerConfig, MelRoFormerResult  # noqa: F401  the reference's import path

    assert M.__all__ == ["MelRoFormer", "MelRoFormerConfig", "MelRoFormerResult"]
    c = MelRoFormerConfig()
    assert (c.dim, c.depth, c.heads, c.dim_head, c.num_bands, c.n_fft, c.hop_length, c.sample_rate) == (384, 6, 8, 64, 60, 2048, 441, 44100)
    assert (c.num_stems, c.ff_mult, c.mlp_expansion_factor, c.mask_estimator_depth, c.win_length, c.chunk_size, c.num_overlap, c.checkpoint_family) == \
        (1, 4, 4, 2, 2048, 352800, 2, None)
    assert (c.dim_inner, c.ff_dim, c.mlp_hidden, c.freq_bins) == (512, 1536, 1536, 1025)
    k, v, z, z1 = MelRoFormerConfig.kim_vocal_2(), MelRoFormerConfig.viperx_vocals(), MelRoFormerConfig.zfturbo_bs_roformer(), MelRoFormerConfig.zfturbo_vocals_v1()
    assert (k.depth, k.dim, k.checkpoint_family) == (6, 384, "kim_vocal_2")
    assert (v.depth, v.dim, v.checkpoint_family) == (12, 384, "viperx_vocals")
    assert (z.depth, z.checkpoint_family) == (12, "zfturbo_bs_roformer")
    assert (z1.dim, z1.depth, z1.hop_length, z1.mask_estimator_depth, z1.checkpoint_family) == (192, 8, 512, 1, "zfturbo_vocals_v1")
    cu = MelRoFormerConfig.custom(depth=8, num_bands=48)
    assert (cu.depth, cu.num_bands, cu.checkpoint_family) == (8, 48, "custom")
    assert MelRoFormerConfig.custom(depth=1, ff_mult=2).ff_dim == 768
    with pytest.raises(TypeError):
        MelRoFormerConfig.custom(8)                                            # keyword-only
    assert not hasattr(MelRoFormerConfig, "default")
    r = MelRoFormerResult(vocals=torch.zeros(1, 2, 4), sample_rate=44100, duration_seconds=1.0, processing_time_seconds=0.1)
    assert r.sample_rate == 44100 and r.vocals.shape == (1, 2, 4)


def test_family_is_a_module_file_outside_the_kind_loader():
    from mlx_audio_amd import registry
    from mlx_audio_amd.sts import loader

    assert "mel_roformer" not in loader.get_available_models() and "sts" not in registry.kinds()
    import mlx_audio_amd.sts.models.mel_roformer as M
    assert os.path.basename(M.__file__) == "mel_roformer.py"


# ------------------------------------------------------------------------------------------------ band tables
@pytest.mark.parametrize("tag", ["A", "B"])
def test_band_tables_match_the_reference(fx, tag):
    from mlx_audio_amd import ops
    from mlx_audio_amd.sts.models.mel_roformer import MelRoFormerConfig, band_dims, mel_band_indices

    npz, meta = fx
    cfg = MelRoFormerConfig.custom(**meta["configs"][tag]["kw"])
    idx = mel_band_indices(cfg)
    ptr = np.concatenate([[0], np.cumsum([len(ix) for ix in idx])])
    assert np.array_equal(ptr, npz[f"{tag}_band_ptr"]) and np.array_equal(np.concatenate(idx), npz[f"{tag}_band_idx"])
    assert band_dims(cfg) == meta["configs"][tag]["widths"] == {"A": [8, 8, 8, 12, 20, 28, 48, 80], "B": [4, 4, 8, 12, 24, 48]}[tag]
    assert all(np.array_equal(a, b) for a, b in zip(idx, R.band_indices(cfg)))
    inv_ptr, inv_col, inv_bd = ops.band_inverse_host(ptr, np.concatenate(idx), 2 * cfg.freq_bins)
    count = np.diff(inv_ptr)
    assert np.array_equal(np.maximum(count, 1).astype(np.float32), npz[f"{tag}_count"]) and {1, 2} <= set(count.tolist())
    for j in range(2 * cfg.freq_bins):                                          # contributors in ascending band order, each pointing at its own entry
        cols = inv_col[inv_ptr[j]:inv_ptr[j + 1]]
        assert np.all(np.diff(cols) > 0)
        for col, bd in zip(cols, inv_bd[inv_ptr[j]:inv_ptr[j + 1]]):
            n = int(np.searchsorted(4 * ptr, col, side="right") - 1)
            assert bd == 2 * (ptr[n + 1] - ptr[n]) and idx[n][(col - 4 * ptr[n]) // 2] == j


def test_band_tables_at_the_default_config():
    """The figures of the issue: bd_n from 24 to 520, sum 7 916, 954 of the 1 025 bins in two bands, none uncovered."""
    from mlx_audio_amd import ops
    from mlx_audio_amd.sts.models.mel_roformer import MelRoFormerConfig, band_dims, mel_band_indices

    cfg = MelRoFormerConfig.kim_vocal_2()
    bd = band_dims(cfg)
    assert len(bd) == 60 and min(bd) == 24 and max(bd) == 520 and sum(bd) == 7916 and max(bd) <= ops.BAND_MAX_DIM
    cover = np.bincount(np.concatenate(mel_band_indices(cfg)) // 2, minlength=cfg.freq_bins) // 2
    assert int((cover == 2).sum()) == 954 and cover.min() == 1 and cover.max() == 2


def test_empty_band_falls_back_to_its_own_bin():
    """model.py:118-119: with more bands than the filterbank can separate, some triangles hold no bin."""
    from mlx_audio_amd.sts.models.mel_roformer import MelRoFormerConfig, mel_band_indices

    cfg = MelRoFormerConfig.custom(depth=1, num_bands=40, n_fft=32, win_length=32, hop_length=8)
    idx = mel_band_indices(cfg)
    assert all(len(ix) >= 2 for ix in idx) and all(np.array_equal(a, b) for a, b in zip(idx, R.band_indices(cfg)))
    from mlx_audio_amd.dsp import mel_filters
    fb = mel_filters(cfg.sample_rate, cfg.n_fft, 40, mel_scale="slaney").numpy()
    empty = [i for i in range(1, 39) if not (fb[i] > 0).any()]
    assert empty and all(np.array_equal(idx[i], [2 * i, 2 * i + 1]) for i in empty)


# ------------------------------------------------------------------------------------------------ sanitize / checkpoints
def test_sanitize_rules():
    """The reference test's qkv split, plus ``.gamma``, ``to_out.0``, the mask-MLP index remap and the dropped rotary buffer."""
    from mlx_audio_amd.sts.models.mel_roformer import MelRoFormer, MelRoFormerConfig, expected_shapes, make_melroformer_weights, sanitize

    cfg = MelRoFormerConfig.kim_vocal_2()
    inner = cfg.dim_inner
    packed = torch.randn(inner * 3, cfg.dim)
    raw = {"layers.0.0.layers.0.0.to_qkv.weight": packed, "layers.0.0.layers.0.0.to_out.weight": torch.randn(cfg.dim, inner)}
    s = MelRoFormer.sanitize(raw)
    p = "layers.0.0.layers.0.0."
    assert set(s) == {p + "to_q.weight", p + "to_k.weight", p + "to_v.weight", p + "to_out.weight"}
    assert all(s[p + n].shape == (inner, cfg.dim) for n in ("to_q.weight", "to_k.weight", "to_v.weight"))
    assert torch.equal(s[p + "to_k.weight"], packed[inner:2 * inner])
    s = sanitize({"band_split.to_features.3.0.gamma": 1, p + "to_out.0.weight": 2, p + "rotary_embed.freqs": 3, "layers.1.1.norm.gamma": 4,
                  "mask_estimators.0.to_freqs.7.0.0.weight": 5, "mask_estimators.0.to_freqs.7.0.2.bias": 6, "mask_estimators.0.to_freqs.7.0.4.weight": 7,
                  p + "to_gates.bias": 8})
    assert s == {"band_split.to_features.3.0.weight": 1, p + "to_out.weight": 2, "layers.1.1.norm.weight": 4, "mask_estimators.0.to_freqs.7.0.0.weight": 5,
                 "mask_estimators.0.to_freqs.7.1.0.bias": 6, "mask_estimators.0.to_freqs.7.2.0.weight": 7, p + "to_gates.bias": 8}
    small = MelRoFormerConfig.custom(depth=1, dim=32, heads=1, num_bands=6, n_fft=32, win_length=32, hop_length=8)
    w, wt = make_melroformer_weights(small, 3), make_melroformer_weights(small, 3, torch_names=True)
    assert set(w) == set(expected_shapes(small)) and set(w) != set(wt) and any(k.endswith("rotary_embed.freqs") for k in wt)
    back = sanitize(wt)
    assert set(back) == set(w) and all(torch.equal(back[k], w[k]) for k in w)
    assert all(torch.equal(v, v.to(torch.float16).to(torch.float32)) for v in w.values())   # fp16-representable
    assert sanitize(w).keys() == w.keys()                                       # idempotent on the reference's names


def test_from_pretrained_priority_config_resolution_and_errors(tmp_path):
    import _ops_emu_melroformer
    from safetensors.torch import save_file

    from mlx_audio_amd.sts.models.mel_roformer import MelRoFormer, MelRoFormerConfig, make_melroformer_weights

    kw = dict(depth=1, dim=32, heads=1, num_bands=6, n_fft=32, win_length=32, hop_length=8, mask_estimator_depth=1)
    cfg = MelRoFormerConfig.custom(**kw)
    w0, w1 = make_melroformer_weights(cfg, 0, torch_names=True), make_melroformer_weights(cfg, 1)
    cfg_json = dict(kw, checkpoint_family="custom", not_a_field=1)
    with _ops_emu_melroformer.patched():
        with pytest.raises(NotImplementedError, match="hub download"):
            MelRoFormer.from_pretrained("someone/mel-roformer", device="cpu")
        with pytest.raises(FileNotFoundError, match=r"No \.safetensors file found in"):
            MelRoFormer.from_pretrained(tmp_path, device="cpu")
        save_file(w0, str(tmp_path / "zz.abcdef12.float32.safetensors"))
        with pytest.raises(ValueError, match="No config provided and no companion config.json found at .*Pass an explicit preset"):
            MelRoFormer.from_pretrained(tmp_path, device="cpu")
        m = MelRoFormer.from_pretrained(tmp_path, config=cfg, device="cpu")       # 1. the argument
        assert m.config is cfg and len(m.layers) == 1 and len(m.mask_estimators) == 1
        (tmp_path / "config.json").write_text(json.dumps(dict(cfg_json, depth=3)))
        with pytest.raises(ValueError, match="missing parameters"):             # 3. the directory's config.json: depth 3 needs more layers
            MelRoFormer.from_pretrained(tmp_path, device="cpu")
        (tmp_path / "zz.abcdef12.float32.config.json").write_text(json.dumps(cfg_json))
        m = MelRoFormer.from_pretrained(tmp_path, device="cpu")                   # 2. the companion wins over config.json
        assert m.config.depth == 1 and m.config.checkpoint_family == "custom" and not hasattr(m.config, "not_a_field")
        gate0 = m.layers[0][0].qkvg.bias[-1].item()
        assert gate0 == pytest.approx(w0["layers.0.0.layers.0.0.to_gates.bias"][-1].item())
        # file priority: any known name beats the sorted-first file; among the known names the reference's order
        for seed, name in ((2, "model.safetensors"), (3, "weights.safetensors"), (4, "mel_roformer_vocals.safetensors")):
            ws = make_melroformer_weights(cfg, seed)
            save_file(ws, str(tmp_path / name))
            (tmp_path / name.replace(".safetensors", ".config.json")).write_text(json.dumps(cfg_json))
            m = MelRoFormer.from_pretrained(tmp_path, device="cpu")
            assert m.layers[0][0].qkvg.bias[-1].item() == pytest.approx(ws["layers.0.0.layers.0.0.to_gates.bias"][-1].item()), name
        save_file({k: v for k, v in w1.items() if "to_gates" not in k}, str(tmp_path / "mel_roformer_vocals.safetensors"))
        with pytest.raises(ValueError, match="missing parameters"):
            MelRoFormer.from_pretrained(tmp_path, device="cpu")


def test_checkpoint_shapes_are_checked():
    import _ops_emu_melroformer
    from mlx_audio_amd.sts.models.mel_roformer import MelRoFormer, MelRoFormerConfig, make_melroformer_weights

    cfg = MelRoFormerConfig.custom(depth=1, dim=32, heads=1, num_bands=6, n_fft=32, win_length=32, hop_length=8, mask_estimator_depth=1)
    w = make_melroformer_weights(cfg, 0)
    with _ops_emu_melroformer.patched():
        with pytest.raises(ValueError, match="unexpected parameters"):
            MelRoFormer(cfg, weights=dict(w, stray=torch.zeros(1)), device="cpu")
        MelRoFormer(cfg, weights=dict(w, stray=torch.zeros(1)), device="cpu", strict=False)
        bad = dict(w)
        bad["band_split.to_features.0.1.weight"] = torch.zeros(32, 6)
        with pytest.raises(ValueError, match="has shape"):
            MelRoFormer(cfg, weights=bad, device="cpu")


def test_not_built_entry_points_raise_by_name():
    import _ops_emu_melroformer
    from mlx_audio_amd.sts.models import mel_roformer as M

    with pytest.raises(NotImplementedError, match="convert_checkpoint"):
        M.convert_checkpoint("model.ckpt", "out")
    with pytest.raises(NotImplementedError, match="hub download"):
        M.MelRoFormer.from_pretrained("KimberleyJSN/melbandroformer")
    cfg = M.MelRoFormerConfig.custom(depth=1, dim=32, heads=1, num_bands=6, n_fft=32, win_length=32, hop_length=8, mask_estimator_depth=1)
    with _ops_emu_melroformer.patched():
        m = M.MelRoFormer(cfg, device="cpu")
        with pytest.raises(NotImplementedError, match="separate_long"):
            m.separate_long(np.zeros((1, 2, 100)))
        with pytest.raises(ValueError, match="stereo"):
            m(np.zeros((1, 1, 100), dtype=np.float32))
        with pytest.raises(ValueError, match="too short"):
            m(np.zeros((1, 2, 16), dtype=np.float32))
        with pytest.raises(NotImplementedError, match="dim_head"):
            M.MelRoFormer(M.MelRoFormerConfig.custom(depth=1, dim_head=32), device="cpu")


# ------------------------------------------------------------------------------------------------ parity with the reference's runs
def test_clips_regenerate(fx):
    """The clips are not stored: a drifted generator must fail loudly."""
    npz, meta = fx
    for tag in meta["configs"]:
        _, _, calls = setup_config(meta, tag)
        for i, x in enumerate(calls):
            assert np.allclose([x.astype(np.float64).sum(), (x.astype(np.float64) ** 2).sum()], npz[f"{tag}{i}_clipsum"], rtol=1e-12), (tag, i)
    assert not R.synth_clip(34, 416, 128)[:, :128].any()


@pytest.mark.parametrize("tag", ["A", "B"])
def test_ref_helper_matches_the_reference(fx, tag):
    """``_melroformer_ref.forward`` (float64) against the reference's float32 runs: stages and waveform within 2e-5 of each tensor's peak."""
    npz, meta = fx
    cfg, w, calls = setup_config(meta, tag)
    wn = {k: v.numpy() for k, v in w.items()}
    for i, x in enumerate(calls):
        y, st = R.forward(cfg, wn, x)
        T = meta["configs"][tag]["frames"][i]
        assert st["split"].shape[1] == T
        for k, v in stage_dict(st).items():
            assert rel_peak(stored(meta, k, v, T), npz[f"{tag}{i}_{k}"]) < BAR, (tag, i, k)
        assert rel_peak(y, npz[f"{tag}{i}_wave"]) < BAR, (tag, i)


@pytest.mark.parametrize("tag", ["A", "B"])
def test_engine_dry_run_matches_the_reference(fx, tag):
    """The engine on ``device="cpu"`` through the emulations: every call against the fixtures (bar 2e-5 of peak); the items of the ``B = 2`` call
    equal the items alone; the silent frames' split output is the bias rows; a silent clip gives exact zeros."""
    import _ops_emu_melroformer
    from mlx_audio_amd.sts.models.mel_roformer import MelRoFormer

    npz, meta = fx
    cfg, w, calls = setup_config(meta, tag)
    with _ops_emu_melroformer.patched():
        eng = MelRoFormer(cfg, weights=w, device="cpu")
        for i, x in enumerate(calls):
            y, st = eng(x, return_stages=True)
            T = meta["configs"][tag]["frames"][i]
            assert y.shape == x.shape and y.dtype == torch.float32 and eng.n_frames(x.shape[2]) == T
            for k, v in stage_dict(st).items():
                assert rel_peak(stored(meta, k, v, T), npz[f"{tag}{i}_{k}"]) < BAR, (tag, i, k)
            assert rel_peak(y.numpy(), npz[f"{tag}{i}_wave"]) < BAR, (tag, i)
            silent = meta["configs"][tag].get("silent_frames", {}).get(str(i))
            if silent:
                assert torch.equal(st["split"][0, silent], eng.split_bias.expand(len(silent), -1, -1))
            if x.shape[0] == 2:
                for b in range(2):
                    assert rel_peak(eng(x[b:b + 1]).numpy(), y[b:b + 1].numpy()) < 1e-6, b
        z = eng(np.zeros((1, 2, 300), dtype=np.float32))
        assert z.shape == (1, 2, 300) and not z.any()


def test_emulated_contracts_agree_with_the_restatement():
    """``band_split`` / ``band_merge`` of ``_ops_emu_melroformer`` (the header's contracts: CSR tables, the inverse table, the frame-major STFT) against
    ``_melroformer_ref`` (the reference's layouts), on a table with a bin covered three times, an uncovered bin and non-contiguous indices."""
    import _ops_emu_melroformer as E
    from mlx_audio_amd import ops

    F, T, B, D = 9, 5, 2, 8
    bands = [[0, 1], [2, 3, 4, 5, 10, 11], [4, 5, 16, 17, 8, 9], [4, 5, 12, 13, 14, 15]]   # bin 2 three times, bin 3 never, bin 8 / 4 out of order
    tab = ops.band_tables(bands, F, "cpu")
    g = torch.Generator().manual_seed(0)
    spec = torch.randn(B * 2, T, F, 2, generator=g)
    w = {}
    for n, ix in enumerate(bands):
        bd = 2 * len(ix)
        w[f"band_split.to_features.{n}.0.weight"] = 1 + 0.1 * torch.randn(bd, generator=g)
        w[f"band_split.to_features.{n}.1.weight"] = torch.randn(D, bd, generator=g)
        w[f"band_split.to_features.{n}.1.bias"] = torch.randn(D, generator=g)
    pk = ops.pack_band_split(*[[w[f"band_split.to_features.{n}.{s}"] for n in range(4)] for s in ("1.weight", "0.weight", "1.bias")], "cpu")
    rep = torch.stack([spec[0::2], spec[1::2]], dim=3).permute(0, 2, 3, 1, 4).reshape(B, 2 * F, T, 2).double().numpy()   # [B, 2 F, T, 2], j = 2 f + c
    want = R.band_split(rep, [np.array(ix) for ix in bands], {k: v.double().numpy() for k, v in w.items()})
    assert rel_peak(E.band_split64(spec, tab, *pk)[0].numpy(), want) < 1e-12
    h = torch.randn(B, T, tab.h_cols, generator=g)
    masks = []
    for n, ix in enumerate(bands):
        c0, bd = 4 * int(tab.band_ptr[n]), 2 * len(ix)
        masks.append((h[:, :, c0:c0 + bd].double() * torch.sigmoid(h[:, :, c0 + bd:c0 + 2 * bd].double())).numpy())
    mask = R.band_merge(masks, [np.array(ix) for ix in bands], 2 * F)
    assert not mask[:, 6:8].any()                                               # the uncovered bin
    full = (rep[..., 0] + 1j * rep[..., 1]) * (mask[..., 0] + 1j * mask[..., 1])   # [B, 2 F, T]
    want = full.reshape(B, F, 2, T).transpose(0, 2, 1, 3).reshape(B * 2, F, T)
    got = E.band_merge64(h, tab, spec)[0].numpy()
    assert np.abs(got - want).max() < 1e-12 * np.abs(want).max()


def test_abi_declares_the_band_entry_points():
    """Additive: three new functions and structs, the ABI number unchanged; the library (when built) exports them."""
    from mlx_audio_amd import _lib

    structs, funcs = _lib.parse_header()
    assert all(f in funcs for f in BAND_FUNCS) and all(s in structs for s in BAND_STRUCTS)
    assert _lib.ABI_VERSION == 37
    names = [f for f, _ in structs["mi355_band_split_args"]]
    assert names[:3] == ["spec", "spec_cstride", "spec_tstride"] and "max_band_dim" in names
    if os.path.exists(_lib.LIBPATH):
        import ctypes
        lib = ctypes.CDLL(_lib.LIBPATH)
        assert all(hasattr(lib, f) for f in BAND_FUNCS)
