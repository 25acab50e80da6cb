"""DeepFilterNet without a GPU: the config values the reference's own tests pin, the host constants, the float64 helper ``tests/_dfn_ref.py`` held to the
reference's runs (``tests/golden/ref_dfn.npz``, made by ``tests/golden/make_dfn_fixtures.py``), the engine's host schedule dry-run over CPU emulations
of the operator contracts against the same runs (alone and as one padded batch), the loader's error paths, what is not built, the checkpoint checks,
and the three new C entry points of ``csrc/dfn.hip``."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
GOLD = os.path.join(HERE, "golden")
HEADER = os.path.join(os.path.dirname(HERE), "include", "mi355audio.h")

import _dfn_ref as R  # noqa: E402

DFN_FUNCS = ("mi355_dfn_features", "mi355_dfn_conv2d", "mi355_dfn_apply")
DFN_STRUCTS = ("mi355_dfn_features_args", "mi355_dfn_conv2d_args", "mi355_dfn_apply_args")
STAGES = ("feat_erb", "feat_df", "emb", "m", "lsnr", "df_coefs")
BAR = 2e-5   # of each tensor's peak: the bar test_s3_cpu.py holds its restated helper to


def rel_peak(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


@pytest.fixture(scope="module")
def fx():
    with open(os.path.join(GOLD, "ref_dfn.json")) as f:
        meta = json.load(f)
    return np.load(os.path.join(GOLD, "ref_dfn.npz")), meta


def setup_config(meta, tag):
    from mlx_audio_amd.sts.models.deepfilternet import config as C, make_dfn_weights

    c = meta["configs"][tag]
    cfg = getattr(C, c["cls"])(**c["kw"])
    clips = [R.synth_clip(seed, n, cfg.sample_rate, tuple(z) if z else None) for seed, n, z in c["clips"]]
    return cfg, make_dfn_weights(cfg, meta["seed_w"]), clips


def stored(fx_npz, meta, tag, i, key, value, T):
    """``value`` laid out and subsampled like the fixture's tensor."""
    v = np.asarray(value)
    if key == "df_coefs" and T > meta["coef_stride_above"]:
        v = v[::meta["coef_stride"]]
    return v.reshape(fx_npz[f"{tag}{i}_{key}"].shape)


def test_config_defaults_and_dict_round_trip():
    """The values of the reference's own tests (``sts/tests/test_deepfilternet.py``: ``test_defaults`` -- 48000 / 960 / 480 / 32 / 96 / 481 -- and
    ``test_from_dict_and_to_dict`` -- sample_rate 44100, nb_df 64, df_order 3 in and out), and more."""
    from mlx_audio_amd.sts.models.deepfilternet import DeepFilterNet2Config, DeepFilterNet3Config, DeepFilterNetConfig, Model, ModelConfig, DeepFilterNetModel
    import mlx_audio_amd.sts.models.deepfilternet as D

    c = DeepFilterNetConfig()
    assert (c.sample_rate, c.sr, c.fft_size, c.hop_size, c.freq_bins, c.nb_erb, c.nb_df, c.df_order) == (48000, 48000, 960, 480, 481, 32, 96, 5)
    assert (c.conv_ch, c.emb_hidden_dim, c.df_hidden_dim, c.emb_num_layers, c.df_num_layers, c.linear_groups, c.enc_linear_groups) == (16, 256, 256, 2, 3, 8, 16)
    assert (c.model_version, DeepFilterNet2Config().model_version, DeepFilterNet3Config().model_version) == ("DeepFilterNet3", "DeepFilterNet2", "DeepFilterNet3")
    c1 = DeepFilterNetConfig.from_dict({"sample_rate": 44100, "nb_df": 64, "df_order": 3})
    assert (c1.sample_rate, c1.nb_df, c1.df_order) == (44100, 64, 3)
    assert (c1.to_dict()["sample_rate"], c1.to_dict()["nb_df"], c1.to_dict()["df_order"]) == (44100, 64, 3)
    c2 = DeepFilterNetConfig.from_dict({"sample_rate": 16000, "fft_size": 320, "hop_size": 160, "nb_df": 64, "unknown_field": 1})
    assert (c2.sample_rate, c2.fft_size, c2.hop_size, c2.nb_df, c2.freq_bins) == (16000, 320, 160, 64, 161)
    d = c2.to_dict()
    assert d["sample_rate"] == 16000 and d["nb_df"] == 64 and "unknown_field" not in d and "df_pathway_kernel_size_t" not in d and len(d) == 41
    assert DeepFilterNetConfig.from_dict(d) == c2
    assert Model is DeepFilterNetModel and ModelConfig is DeepFilterNetConfig
    assert D.__all__ == ["DeepFilterNetModel", "DeepFilterNetConfig", "DeepFilterNet2Config", "DeepFilterNet3Config", "Model", "ModelConfig"]


def test_window_and_norm_alpha():
    from mlx_audio_amd.sts.models.deepfilternet import DeepFilterNet3Config, DeepFilterNetModel

    w = DeepFilterNetModel._vorbis_window(960)
    assert w.dtype == np.float32 and w.shape == (960,) and 0.0 < w.min() and w.max() <= 1.0 and np.allclose(w, w[::-1], atol=1e-6)
    assert np.allclose(w[:480] ** 2 + w[480:] ** 2, 1.0, atol=1e-6)            # power complementary at hop = N / 2
    m = DeepFilterNetModel.__new__(DeepFilterNetModel)
    m.config = DeepFilterNet3Config()
    assert m._norm_alpha() == 0.99
    m.config = DeepFilterNet3Config(hop_size=1, sample_rate=48000)            # exp(-1 / 48000) rounds to 1.0 at 3 and 4 decimals: the loop goes on
    assert m._norm_alpha() == 0.99998
    assert np.allclose(R.vorbis_window(960), w.astype(np.float64)) and R.norm_alpha(480, 48000) == 0.99


def test_clips_regenerate(fx):
    """The clips are not stored: a drifted generator must fail loudly."""
    npz, meta = fx
    for tag in meta["configs"]:
        _, _, clips = setup_config(meta, tag)
        for i, x in enumerate(clips):
            assert np.allclose([x.astype(np.float64).sum(), (x.astype(np.float64) ** 2).sum()], npz[f"{tag}{i}_clipsum"], rtol=1e-12), (tag, i)


@pytest.mark.parametrize("tag", ["A", "B"])
def test_ref_helper_matches_the_reference(fx, tag):
    """``_dfn_ref.enhance`` (float64) against the reference's float32 runs: stages and waveform within 2e-5 of each tensor's peak."""
    npz, meta = fx
    cfg, w, clips = setup_config(meta, tag)
    wn = {k: v.numpy() for k, v in w.items()}
    for i, x in enumerate(clips):
        y, st = R.enhance(cfg, wn, x)
        T = meta["configs"][tag]["frames"][i]
        assert st["emb"].shape[0] == T
        for k in STAGES:
            assert rel_peak(stored(npz, meta, tag, i, k, st[k], T), npz[f"{tag}{i}_{k}"]) < BAR, (tag, i, k)
        assert rel_peak(y, npz[f"{tag}{i}_wave"]) < BAR, (tag, i)


@pytest.mark.parametrize("tag", ["A", "B"])
def test_engine_dry_run_matches_the_reference(fx, tag):
    """The engine on ``device="cpu"`` through the emulations: every clip alone against the fixtures (bar 2e-5 of peak), then all clips of the config as
    ONE padded batch, whose items must equal the single runs (exactly: the emulations compute each item from its own frames; ``lsnr`` to float32
    rounding, its one-column float64 product is summed in an order that depends on the row count)."""
    import _ops_emu_dfn
    from mlx_audio_amd.sts.models.deepfilternet import DeepFilterNetModel

    npz, meta = fx
    cfg, w, clips = setup_config(meta, tag)
    with _ops_emu_dfn.patched():
        eng = DeepFilterNetModel(cfg, weights=w, device="cpu")
        alone = []
        for i, x in enumerate(clips):
            y, st = eng.enhance_array(x, return_stages=True)
            T = meta["configs"][tag]["frames"][i]
            assert st["frames"] == [T] and y.dtype == np.float32 and y.shape == x.shape
            for k in STAGES:
                assert rel_peak(stored(npz, meta, tag, i, k, st[k][0].numpy(), T), npz[f"{tag}{i}_{k}"]) < BAR, (tag, i, k)
            assert rel_peak(y, npz[f"{tag}{i}_wave"]) < BAR, (tag, i)
            alone.append((y, st))
        ys, stb = eng.enhance_batch(clips, return_stages=True)
        for i, (y, st) in enumerate(alone):
            T = st["frames"][0]
            assert np.array_equal(ys[i], y), i
            for k in STAGES:
                if k == "lsnr":
                    assert float((stb[k][i, :T] - st[k][0]).abs().max()) < 1e-5, i
                else:
                    assert torch.equal(stb[k][i, :T], st[k][0]), (i, k)
            for k in ("feat_erb", "feat_df", "emb", "m", "df_coefs"):
                assert not stb[k][i, T:].any(), (i, k)                    # rows behind an item's frames are zeros
        spec_e, m, lsnr, coefs = eng.model(stb["spec"], stb["feat_erb"], stb["feat_df"], torch.tensor(stb["frames"], dtype=torch.int32), wnorm=eng.wnorm)
        B, T = len(clips), max(stb["frames"])
        assert spec_e.shape == (B, T, cfg.freq_bins) and m.shape == (B, 1, T, cfg.nb_erb) and lsnr.shape == (B, T, 1)
        assert coefs.shape == (B, cfg.df_order, T, cfg.nb_df, 2)                # the reference's layouts


def test_band_width_form_and_float32_unrounded_checkpoint():
    """A checkpoint without ``erb_fb`` runs on the config's ``erb_widths`` (band means); the result is the filterbank product's, to rounding."""
    import _ops_emu_dfn
    from mlx_audio_amd.sts.models.deepfilternet import DeepFilterNet2Config, DeepFilterNetModel, make_dfn_weights
    from mlx_audio_amd.sts.models.deepfilternet.model import default_erb_widths, erb_filterbanks

    kw = dict(enc_concat=True, fft_size=480, hop_size=240, nb_erb=16, nb_df=48, conv_ch=8, emb_hidden_dim=64, df_hidden_dim=64, enc_linear_groups=8)
    widths = default_erb_widths(241, 16)
    assert sum(widths) == 241 and min(widths) >= 2 and widths == sorted(widths)
    fb, inv = erb_filterbanks(widths, 241)
    assert torch.allclose(fb.sum(0), torch.ones(16)) and torch.equal(inv.sum(0), torch.ones(241))
    cfg = DeepFilterNet2Config(erb_widths=widths, **kw)
    w = make_dfn_weights(cfg, 3)
    x = R.synth_clip(5, 5000)
    with _ops_emu_dfn.patched():
        a = DeepFilterNetModel(cfg, weights=w, device="cpu").enhance_array(x)
        b = DeepFilterNetModel(cfg, weights={k: v for k, v in w.items() if k != "erb_fb"}, device="cpu").enhance_array(x)
        with pytest.raises(ValueError, match="missing both"):
            DeepFilterNetModel(DeepFilterNet2Config(**kw), weights={k: v for k, v in w.items() if k != "erb_fb"}, device="cpu")
    assert rel_peak(b, a) < 1e-5 and float(np.abs(a).max()) > 1e-3
    y, _ = R.enhance(cfg, {k: v.numpy() for k, v in w.items() if k != "erb_fb"}, x)
    assert rel_peak(b, y) < BAR


def test_df_gru_skip_groupedlinear():
    """``df_gru_skip = "groupedlinear"`` (``DfDecoder.df_skip``, network.py:450-468): the skip product accumulates into the GRU stack's output."""
    import _ops_emu_dfn
    from mlx_audio_amd.sts.models.deepfilternet import DeepFilterNet2Config, DeepFilterNetModel, make_dfn_weights

    kw = dict(enc_concat=True, fft_size=480, hop_size=240, nb_erb=16, nb_df=48, conv_ch=8, emb_hidden_dim=64, df_hidden_dim=64, enc_linear_groups=8)
    cfg = DeepFilterNet2Config(df_gru_skip="groupedlinear", **kw)
    w = make_dfn_weights(cfg, 4)
    assert tuple(w["df_dec.df_skip.weight"].shape) == (8, 8, 8) and "df_dec.df_skip.weight" not in make_dfn_weights(DeepFilterNet2Config(**kw), 4)
    x = R.synth_clip(6, 4000)
    with _ops_emu_dfn.patched():
        y, st = DeepFilterNetModel(cfg, weights=w, device="cpu").enhance_array(x, return_stages=True)
    yr, sr = R.enhance(cfg, {k: v.numpy() for k, v in w.items()}, x)
    assert rel_peak(st["df_coefs"][0].numpy(), sr["df_coefs"]) < BAR and rel_peak(y, yr) < BAR
    plain = {k: v for k, v in w.items() if k != "df_dec.df_skip.weight"}
    assert rel_peak(R.enhance(DeepFilterNet2Config(**kw), {k: v.numpy() for k, v in plain.items()}, x)[1]["df_coefs"], sr["df_coefs"]) > 1e-2   # it matters


def test_checkpoint_names_are_checked(fx):
    import _ops_emu_dfn
    from mlx_audio_amd.sts.models.deepfilternet import DeepFilterNetModel

    _, meta = fx
    cfg, w, _ = setup_config(meta, "B")
    with _ops_emu_dfn.patched():
        ok = dict(w)
        ok["enc.erb_conv0.2.num_batches_tracked"] = torch.zeros(())
        ok["enc.emb_gru.gru.h0"] = torch.zeros(1, 1, 64)
        DeepFilterNetModel(cfg, weights=ok, device="cpu")                       # both ignored like the reference's loader does
        with pytest.raises(ValueError, match="unexpected parameters.*enc.bogus.weight"):
            DeepFilterNetModel(cfg, weights={**w, "enc.bogus.weight": torch.zeros(1)}, device="cpu")
        DeepFilterNetModel(cfg, weights=w, device="cpu").load_weights({**w, "enc.bogus.weight": torch.zeros(1)}, strict=False)
        with pytest.raises(ValueError, match="missing parameters.*df_dec.df_out.0.weight"):
            DeepFilterNetModel(cfg, weights={k: v for k, v in w.items() if k != "df_dec.df_out.0.weight"}, device="cpu")
        with pytest.raises(ValueError, match="has shape"):
            DeepFilterNetModel(cfg, weights={**w, "enc.lsnr_fc.0.bias": torch.zeros(2)}, device="cpu")
    for k, v in w.items():
        assert torch.equal(v.half().float(), v), k                               # fp16-representable
        if k.endswith("running_var"):
            assert 0.5 <= float(v.min()) and float(v.max()) <= 1.5


def test_loader_paths(fx, tmp_path):
    import _ops_emu_dfn
    from safetensors.torch import save_file
    from mlx_audio_amd.sts import loader
    from mlx_audio_amd.sts.models.deepfilternet import DeepFilterNetModel

    _, meta = fx
    cfg, w, clips = setup_config(meta, "B")
    with pytest.raises(FileNotFoundError, match="no hub access"):
        DeepFilterNetModel.from_pretrained(str(tmp_path / "nowhere"))
    f = tmp_path / "file.bin"
    f.write_bytes(b"x")
    with pytest.raises(ValueError, match="must be a directory"):
        DeepFilterNetModel.from_pretrained(str(f))
    with pytest.raises(ValueError, match="Unsupported version=4"):
        DeepFilterNetModel.from_pretrained(str(tmp_path), version=4)
    with pytest.raises(FileNotFoundError, match="Missing config.json"):
        DeepFilterNetModel.from_pretrained(str(tmp_path), version=2)
    d = tmp_path / "v2"
    d.mkdir()
    (d / "config.json").write_text(json.dumps(cfg.to_dict()))
    with pytest.raises(FileNotFoundError, match="Missing model.safetensors"):
        DeepFilterNetModel.from_pretrained(str(tmp_path), version=2)
    save_file({k: v.contiguous() for k, v in w.items()}, str(d / "model.safetensors"))
    with _ops_emu_dfn.patched():
        direct = DeepFilterNetModel(cfg, weights=w, device="cpu").enhance_array(clips[0])
        a = DeepFilterNetModel.from_pretrained(str(tmp_path), version=2, device="cpu")
        assert a.model_dir == d and a.config == cfg and np.array_equal(a.enhance_array(clips[0]), direct)
        b = DeepFilterNetModel.from_pretrained(str(d), subfolder=None, device="cpu")
        assert np.array_equal(b.enhance_array(clips[0]), direct)
        c = loader.load_model(d, device="cpu")
        assert isinstance(c, DeepFilterNetModel) and np.array_equal(c.enhance_array(clips[0]), direct)
    assert loader.get_available_models() == ["deepfilternet"]


def test_what_is_not_built(fx):
    import _ops_emu_dfn
    from mlx_audio_amd.sts.models.deepfilternet import DeepFilterNetConfig, DeepFilterNetModel

    _, meta = fx
    cfg, w, clips = setup_config(meta, "B")
    with _ops_emu_dfn.patched():
        eng = DeepFilterNetModel(cfg, weights=w, device="cpu")
        with pytest.raises(NotImplementedError, match="create_streamer.*streaming runtime"):
            eng.create_streamer()
        with pytest.raises(NotImplementedError, match="enhance_array_streaming.*streaming runtime"):
            eng.enhance_array_streaming(clips[0])
        with pytest.raises(NotImplementedError, match="enhance_file_streaming.*streaming runtime"):
            eng.enhance_file_streaming("a.wav", "b.wav")
        with pytest.raises(NotImplementedError, match="DfNetV1"):
            DeepFilterNetModel(DeepFilterNetConfig(model_version="DeepFilterNet"), device="cpu")
        with pytest.raises(NotImplementedError, match="hidden sizes"):
            DeepFilterNetModel(DeepFilterNetConfig(emb_hidden_dim=96), device="cpu")
        with pytest.raises(ValueError, match="1-D"):
            eng.enhance_array(np.zeros((2, 100), dtype=np.float32))
        assert eng.enhance_batch([]) == [] and eng.enhance_array(np.zeros(0, dtype=np.float32)).shape == (0,)


def test_entry_points_declared_exported_and_refuse_bad_arguments():
    from mlx_audio_amd import _lib, ops

    lib = _lib.load()
    assert lib.mi355_abi_version() == 37 == _lib.ABI_VERSION   # additive entry points: no layout changed, no bump
    for f, s in zip(DFN_FUNCS, DFN_STRUCTS):
        assert f in _lib.declared_functions() and hasattr(lib, f), f
        assert getattr(lib, f)(ctypes.byref(_lib.STRUCTS[s]()), None) == -1 and b"null tensor" in lib.mi355_last_error(), f
        assert getattr(lib, f)(None, None) == -1
    for F, kf, fs, tr, want in ((32, 3, 1, 0, 32), (32, 3, 2, 0, 16), (96, 3, 2, 0, 48), (8, 3, 2, 1, 16), (7, 3, 2, 0, 4), (5, 1, 2, 0, 3), (5, 1, 2, 1, 9),
                                (5, 2, 1, 0, -1), (5, 3, 3, 0, -1)):
        assert lib.mi355_dfn_conv2d_fo(F, kf, fs, tr) == want, (F, kf, fs, tr)
        if want > 0:
            assert ops.dfn_conv2d_fo(F, kf, fs, bool(tr)) == want
    buf = (ctypes.c_float * 64)()   # host memory: every case below must be refused before a launch could touch it
    p = ctypes.addressof(buf)

    def call(fn, st, **kw):
        return getattr(lib, fn)(ctypes.byref(_lib.STRUCTS[st](**kw)), None), lib.mi355_last_error()

    conv = dict(x=p, x_bstride=64, w=p, B=1, T=1, F=4, Cin=2, Cmid=2, Cout=2, groups=1, kt=1, kf=3, fstride=1, y=p, y_bstride=64)
    for bad, msg in ((dict(Cin=65), b"bad shape"), (dict(groups=3), b"groups"), (dict(Cout=4), b"pointwise"), (dict(kt=6), b"kt 1..5"), (dict(kf=2), b"kt 1..5"),
                     (dict(fstride=3), b"kt 1..5"), (dict(act=3), b"kt 1..5"), (dict(lookahead=1), b"kt 1..5"), (dict(x_bstride=7), b"strides"),
                     (dict(y_bstride=7), b"strides"), (dict(add=p, add_bstride=1), b"strides")):
        rc, err = call("mi355_dfn_conv2d", "mi355_dfn_conv2d_args", **{**conv, **bad})
        assert rc == -1 and msg in err, (bad, err)
    feat = dict(spec=p, spec_bstride=64, erb_fb=p, B=1, T=1, F=8, E=2, D=4, spec_out=p, spec_out_bstride=64, feat_erb=p, feat_df=p)
    for bad, msg in ((dict(erb_start=p), b"exactly one"), (dict(erb_fb=None), b"exactly one"), (dict(E=257), b"bad shape"), (dict(D=9), b"bad shape"),
                     (dict(lookahead=-1), b"bad shape"), (dict(spec_bstride=15), b"strides")):
        rc, err = call("mi355_dfn_features", "mi355_dfn_features_args", **{**feat, **bad})
        assert rc == -1 and msg in err, (bad, err)
    app = dict(spec=p, spec_bstride=64, m=p, erb_inv_fb=p, coef=p, B=1, T=1, F=8, E=2, D=4, order=5, df_lookahead=2, wnorm=1.0, out=p, out_bstride=64)
    for bad, msg in ((dict(D=9), b"bad shape"), (dict(df_lookahead=5), b"bad shape"), (dict(order=0), b"bad shape"), (dict(wnorm=0.0), b"wnorm"),
                     (dict(out_bstride=15), b"strides")):
        rc, err = call("mi355_dfn_apply", "mi355_dfn_apply_args", **{**app, **bad})
        assert rc == -1 and msg in err, (bad, err)


def test_struct_layouts_match_c(tmp_path):
    from mlx_audio_amd import _lib, ops

    src = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){"]
    for name in DFN_STRUCTS:
        src.append(f'printf("{name} %zu\\n", sizeof({name}));')
        for f, _ in _lib._STRUCT_DECLS[name]:
            src.append(f'printf("{name}.{f} %zu\\n", offsetof({name}, {f}));')
    src.append('printf("bands %d\\nch %d\\n", MI355_DFN_MAX_BANDS, MI355_DFN_MAX_CH);')
    src.append("return 0;}")
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", str(c), "-o", str(exe)], check=True)
    want = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.strip().splitlines())
    for name in DFN_STRUCTS:
        st = _lib.STRUCTS[name]
        assert ctypes.sizeof(st) == int(want[name]), name
        for f, _ in _lib._STRUCT_DECLS[name]:
            assert getattr(st, f).offset == int(want[f"{name}.{f}"]), (name, f)
    assert (int(want["bands"]), int(want["ch"])) == (ops.DFN_MAX_BANDS, ops.DFN_MAX_CH) == (256, 64)
