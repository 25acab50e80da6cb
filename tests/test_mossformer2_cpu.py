"""MossFormer2 SE without a GPU: the config behaviours the reference's ``sts/tests/test_mossformer2_se.py`` pins, the parameter names and shapes, the
reassembly index arithmetic of both long-audio paths, ``from_pretrained`` from a temporary directory, what is not built, the four new C entry points
of ``csrc/mossformer.hip``, and the network's host schedule dry-run over the float64 operator contracts (``tests/_ops_emu_mossformer2.py``) against the
independent float64 restatement of the reference's module tree (``tests/_mossformer2_ref.py``)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import _mossformer2_ref as R  # noqa: E402

FUNCS = ("mi355_shift_scalenorm", "mi355_gau_kv", "mi355_gau_attention", "mi355_gated_fsmn")
STRUCTS = ("mi355_shift_scalenorm_args", "mi355_gau_kv_args", "mi355_gau_attention_args", "mi355_gated_fsmn_args")
BAR = 2e-5   # of each tensor's peak: float32 storage between float64 operators through two layers (the bar of test_melroformer_cpu.py)


def rel_peak(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def small_config(**kw):
    from mlx_audio_amd.sts.models.mossformer2_se import MossFormer2SEConfig

    return MossFormer2SEConfig(**{**dict(out_channels=64, num_blocks=2), **kw})


# ------------------------------------------------------------------------------------------------ config
def test_config_defaults_from_dict_to_dict_and_alias():
    from mlx_audio_amd.sts.models import mossformer2_se as M
    from mlx_audio_amd.sts.models.mossformer2_se import MossFormer2SEConfig

    assert M.Model is M.MossFormer2SEModel and M.ModelConfig is MossFormer2SEConfig
    c = MossFormer2SEConfig()
    assert (c.sample_rate, c.win_len, c.win_inc, c.fft_len, c.win_type, c.num_mels, c.preemphasis) == (48000, 1920, 384, 1920, "hamming", 60, 0.97)
    assert (c.one_time_decode_length, c.decode_window, c.chunk_seconds, c.chunk_overlap, c.auto_chunk_threshold) == (20, 4, 4.0, 0.25, 60.0)
    assert (c.in_channels, c.out_channels, c.out_channels_final, c.num_blocks) == (180, 512, 961, 24)
    assert c.sampling_rate == c.sample_rate == 48000
    d = MossFormer2SEConfig.from_dict({"sample_rate": 16000, "num_mels": 40, "unknown_key": 1, "model_type": "mossformer2_se"})
    assert (d.sample_rate, d.num_mels, d.win_len, d.sampling_rate) == (16000, 40, 1920, 16000)
    t = c.to_dict()
    assert set(t) == {"sample_rate", "win_len", "win_inc", "fft_len", "num_mels", "win_type", "preemphasis", "one_time_decode_length", "decode_window",
                      "chunk_seconds", "chunk_overlap", "auto_chunk_threshold", "in_channels", "out_channels", "out_channels_final", "num_blocks"}
    assert MossFormer2SEConfig.from_dict(t) == c and t["win_len"] == 1920 and t["chunk_overlap"] == 0.25


@pytest.fixture(scope="module")
def fx():
    with open(os.path.join(HERE, "golden", "ref_mossformer2.json")) as f:
        meta = json.load(f)
    return np.load(os.path.join(HERE, "golden", "ref_mossformer2.npz")), meta


def test_parameter_names_and_shapes(fx):
    """The names and shapes equal those of the reference's own full-size ``MossFormer2SE`` (its flattened parameters, stored by the fixture maker);
    then counted per block and spot-checked."""
    from mlx_audio_amd.sts.models.mossformer2_se import MossFormer2SEConfig
    from mlx_audio_amd.sts.models.mossformer2_se.network import expected_shapes, make_mossformer2_weights

    s = expected_shapes(MossFormer2SEConfig())
    ref = fx[1]["parameters"]
    assert set(s) == set(ref), sorted(set(s) ^ set(ref))[:8]
    assert all(tuple(ref[k]) == s[k] for k in s)
    m = "model.mossformer.mdl.intra_mdl.mossformerM."
    assert sum(k.startswith(m + "layers.0.") for k in s) == 14 and sum(k.startswith(m + "fsmn.0.") for k in s) == 23
    assert len(s) == 5 + 24 * (14 + 23) + 4 + 8
    assert s[m + "layers.23.to_hidden.linear.weight"] == (2048, 512) and s[m + "layers.0.to_out.linear.weight"] == (512, 1024)
    assert s[m + "layers.0.to_qk.conv_module.weight"] == (128, 17, 1) and s[m + "layers.0.qk_offset_scale.gamma"] == (4, 128)
    assert s[m + "fsmn.5.gated_fsmn.fsmn.conv1.weight"] == (256, 39, 1, 1) and s[m + "fsmn.5.conv2.weight"] == (512, 1, 256)
    assert s["model.mossformer.conv1d_out.weight"] == (1024, 1, 512) and s["model.mossformer.conv1_decoder.weight"] == (961, 1, 512)
    assert s["model.mossformer.norm.weight"] == (180, 1) and s["model.mossformer.pos_enc.inv_freq"] == (256,)
    cfg = small_config()
    w = make_mossformer2_weights(cfg, 3)
    assert set(w) == set(expected_shapes(cfg)) and all(tuple(w[k].shape) == v for k, v in expected_shapes(cfg).items())
    assert all(torch.equal(v, v.to(torch.float16).float()) for k, v in w.items() if not k.endswith("inv_freq"))


# ------------------------------------------------------------------------------------------------ reassembly arithmetic
def _segmented_literal(t, window_size):
    """The reference's loop (model.py:241-291) on sample indices instead of samples: which input index each output sample comes from (-1: zero)."""
    stride = int(window_size * 0.75)
    idx = np.arange(t)
    if t < window_size:
        idx = np.concatenate([idx, np.full(window_size - t, -1)])
    elif t < window_size + stride:
        idx = np.concatenate([idx, np.full(window_size + stride - t, -1)])
    elif (t - window_size) % stride != 0:
        idx = np.concatenate([idx, np.full(t - (t - window_size) // stride * stride, -1)])
    tt, give_up, cur = idx.shape[0], (window_size - stride) // 2, 0
    out = np.full(tt, -2)
    while cur + window_size <= tt:
        seg = idx[cur:cur + window_size] * 10 + (cur // stride) % 10       # tag each sample with the window that produced it
        if cur == 0:
            out[cur:cur + window_size - give_up] = seg[:-give_up]
        else:
            out[cur + give_up:cur + window_size - give_up] = seg[give_up:-give_up]
        cur += stride
    return tt, out[:t]


@pytest.mark.parametrize("t", [900, 1000, 1500, 1749, 1750, 2000, 2500, 3301])
def test_segment_plan_follows_the_reference_on_every_padding_branch(t):
    """window 1000, stride 750: t < window; window <= t < window + stride; the remainder branch; an exact fit."""
    from mlx_audio_amd.sts.models.mossformer2_se.model import segment_plan

    W = 1000
    padded, plan = segment_plan(t, W)
    tt, want = _segmented_literal(t, W)
    assert padded == tt
    src = np.concatenate([np.arange(t), np.full(padded - t, -1)])
    out = np.full(padded, -2)
    for k, (s, lo, hi) in enumerate(plan):
        out[s + lo:s + hi] = src[s + lo:s + hi] * 10 + k % 10
    assert np.array_equal(out[:t], want)


@pytest.mark.parametrize("n", [1001, 1750, 1751, 2499, 2500, 2600, 4000])
def test_chunk_plan_follows_the_reference(n):
    """chunk 1000, overlap 250 (stride 750, give-up 125): full chunks only, and a partial last chunk of every kind."""
    from mlx_audio_amd.sts.models.mossformer2_se.model import chunk_plan

    C, O = 1000, 250
    stride, give_up = C - O, O // 2
    # the reference's loops (model.py:336-375) on index arrays
    chunks, starts, cur = [], [], 0
    while cur + C <= n:
        chunks.append(np.arange(cur, cur + C)), starts.append(cur)
        cur += stride
    if cur < n:
        chunks.append(np.arange(cur, n)), starts.append(cur)
    want = np.full(n, -1)
    for i, (ch, st) in enumerate(zip(chunks, starts)):
        first, last = i == 0, i == len(chunks) - 1
        if last and len(ch) < C:
            ks, ke = (give_up if not first else 0), len(ch)
        else:
            ks, ke = (0 if first else give_up), len(ch) - give_up
        os_, oe = st + ks, min(st + ke, n)
        want[os_:oe] = (ch * 10 + i % 10)[ks:ks + (oe - os_)]
    got = np.full(n, -1)
    plan = chunk_plan(n, C, O)
    assert [p[0] for p in plan] == starts and [p[1] for p in plan] == [len(c) for c in chunks]
    for i, (s, ln, ks, kept) in enumerate(plan):
        got[s + ks:s + ks + kept] = (np.arange(s, s + ln) * 10 + i % 10)[ks:ks + kept]
    assert np.array_equal(got, want)


# ------------------------------------------------------------------------------------------------ host schedule over the operator contracts
@pytest.fixture(scope="module")
def dry():
    """Config A of the GPU suite (width 64, 2 blocks, 961 mask columns) on seeded features: the reference restatement per item, computed once."""
    from mlx_audio_amd.sts.models.mossformer2_se.network import make_mossformer2_weights

    cfg = small_config()
    w = make_mossformer2_weights(cfg, 11)
    g = torch.Generator().manual_seed(5)
    frames = [1, 2, 58, 257]
    feats = [torch.randn(T, cfg.in_channels, generator=g) * 3.0 + 1.0 for T in frames]
    ref = []
    for f in feats:
        st = {}
        st["mask"] = R.masknet(f, w, cfg.num_blocks, st)
        ref.append(st)
    return cfg, w, frames, feats, ref


def test_host_schedule_over_the_contracts_matches_the_restated_reference(dry):
    """One ragged batch of 1, 2, 58 and 257 frames (one row, the token shift's first row, less than a group, a group plus one row) and the longest
    item alone: layer 0's FLASH output, its Gated-FSMN output and the mask within 2e-5 of each tensor's peak."""
    import _ops_emu_mossformer2 as E
    from mlx_audio_amd.sts.models.mossformer2_se.network import MossFormerMaskNet

    cfg, w, frames, feats, ref = dry
    assert ref[3]["parts"]["quad"] > 0.1 * ref[3]["parts"]["lin"] and ref[3]["parts"]["lin"] > 0.1 * ref[3]["parts"]["quad"], ref[3]["parts"]
    with E.patched():
        net = MossFormerMaskNet(cfg, "cpu")
        net.load(w)
        T = max(frames)
        fbuf = torch.zeros(len(frames), T, cfg.in_channels)
        for b, f in enumerate(feats):
            fbuf[b, :f.shape[0]] = f
        st = {}
        mask = net.forward(fbuf, torch.tensor(frames, dtype=torch.int32), st)
        st1 = {}
        mask1 = net.forward(feats[3][None].contiguous(), None, st1)
    for b, n in enumerate(frames):
        for k, got in (("flash0", st["flash0"]), ("fsmn0", st["fsmn0"]), ("mask", mask)):
            d = rel_peak(got[b, :n].numpy(), ref[b][k].numpy())
            print(f"item {b} ({n} frames) {k}: distance / peak {d:.2e}")
            assert d < BAR, (b, k, d)
    for k, got in (("flash0", st1["flash0"]), ("fsmn0", st1["fsmn0"]), ("mask", mask1)):
        assert rel_peak(got[0].numpy(), ref[3][k].numpy()) < BAR
    m = ref[3]["mask"]
    assert float((m == 0).double().mean()) > 0.01 and float((m > 0).double().mean()) > 0.01     # the final ReLU is exercised


@pytest.mark.parametrize("call", [0, 1, 2])
def test_fixture_stages_through_the_host_schedule_and_the_restatement(fx, call):
    """The reference's own runs of config A whose features are stored whole (1, 2 and 58 frames): fed with those features, the host schedule over
    the float64 contracts and the float64 restatement ``_mossformer2_ref.masknet`` both give layer 0's FLASH output, its Gated-FSMN output and the
    mask within 2e-5 of each tensor's peak of the reference's float32 run."""
    import _ops_emu_mossformer2 as E
    from mlx_audio_amd.sts.models.mossformer2_se import MossFormer2SEConfig, make_mossformer2_weights
    from mlx_audio_amd.sts.models.mossformer2_se.network import MossFormerMaskNet

    npz, meta = fx
    c = meta["configs"]["A"]
    cfg = MossFormer2SEConfig.from_dict(c["kw"])
    w = make_mossformer2_weights(cfg, c["seed_w"])
    frames = c["calls"][call][1]
    feats = torch.from_numpy(npz[f"A{call}_feats"])
    assert feats.shape == (frames, cfg.in_channels)
    sub = lambda v: v[::meta["stride"]] if frames > meta["stride_above"] else v
    msub = lambda v: sub(v)[:, ::meta["mask_col_stride"]] if frames > meta["stride_above"] else v
    st_r = {}
    st_r["mask"] = R.masknet(feats, w, cfg.num_blocks, st_r)
    with E.patched():
        net = MossFormerMaskNet(cfg, "cpu")
        net.load(w)
        st_e = {}
        st_e["mask"] = net.forward(feats[None].contiguous(), None, st_e)[0]
        st_e["flash0"], st_e["fsmn0"] = st_e["flash0"][0], st_e["fsmn0"][0]
    for name, st in (("host schedule", st_e), ("restatement", st_r)):
        for k in ("flash0", "fsmn0", "mask"):
            v = st[k].detach().numpy()
            d = rel_peak(msub(v) if k == "mask" else sub(v), npz[f"A{call}_{k}"])
            print(f"{name}, {frames} frames, {k}: distance / peak {d:.2e}")
            assert d < BAR, (name, k, d)


# ------------------------------------------------------------------------------------------------ loading, refusals, symbols
def test_from_pretrained_from_a_directory_and_what_is_not_built(tmp_path):
    import _ops_emu_mossformer2 as E
    from safetensors.torch import save_file

    from mlx_audio_amd.sts import loader
    from mlx_audio_amd.sts.models.mossformer2_se import MossFormer2SEConfig, MossFormer2SEModel, make_mossformer2_weights

    cfg = small_config(num_blocks=1)
    w = make_mossformer2_weights(cfg, 2)
    (tmp_path / "config.json").write_text(json.dumps({**cfg.to_dict(), "model_type": "mossformer2_se", "extra": 1}))
    with E.patched():
        with pytest.raises(FileNotFoundError, match="model.safetensors"):
            MossFormer2SEModel.from_pretrained(str(tmp_path), device="cpu")
        save_file({k: v.contiguous() for k, v in w.items()}, str(tmp_path / "model.safetensors"))
        m = MossFormer2SEModel.from_pretrained(str(tmp_path), device="cpu")
        assert m.config == cfg and isinstance(m.config, MossFormer2SEConfig)
        with pytest.raises(ValueError, match="missing parameters"):
            m.load_weights({k: v for k, v in w.items() if "to_qk.norm.g" not in k})
        with pytest.raises(ValueError, match="unexpected parameters"):
            m.load_weights({**w, "model.mossformer.nope": torch.zeros(1)}, strict=True)
        m.load_weights(list({**w, "model.mossformer.nope": torch.zeros(1)}.items()))       # the reference loads with strict=False
        m.load_weights({k: v for k, v in w.items() if not k.endswith("inv_freq")})          # a constant: may be absent
        with pytest.raises(NotImplementedError, match="hub download"):
            MossFormer2SEModel.from_pretrained("starkdmi/MossFormer2_SE_48K_MLX")
        (tmp_path / "config.json").write_text(json.dumps({**cfg.to_dict(), "quantization_config": {"bits": 4, "group_size": 64}}))
        with pytest.raises(NotImplementedError, match="quantised"):
            MossFormer2SEModel.from_pretrained(str(tmp_path), device="cpu")
        (tmp_path / "config.json").write_text(json.dumps({**cfg.to_dict(), "quantization_config": {"bits": 16}}))
        MossFormer2SEModel.from_pretrained(str(tmp_path), device="cpu")
        with pytest.raises(NotImplementedError, match="causal"):
            MossFormer2SEModel(cfg, weights=w, device="cpu", causal=True)
        with pytest.raises(NotImplementedError, match="MossFormerM2"):
            MossFormer2SEModel(cfg, weights=w, device="cpu", use_mossformer2=True)
    assert "mossformer2_se" not in loader.MODEL_REMAPPING      # loaded through its class, like Mel-Band RoFormer


def test_the_four_entry_points_are_declared_and_exported():
    from mlx_audio_amd import _lib

    structs, funcs = _lib.parse_header()
    assert all(f in funcs for f in FUNCS) and all(s in structs for s in STRUCTS)
    assert _lib.ABI_VERSION == 37
    text = open(_lib.HEADER).read()
    for f in FUNCS:
        assert text.count(f + "(") == 1
    lib = _lib.load()                                   # builds the library first where it is missing (hipcc cross-compiles without a GPU)
    assert lib.mi355_abi_version() == 37 and all(hasattr(lib, f) for f in FUNCS)
