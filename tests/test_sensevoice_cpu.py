"""SenseVoice-Small without a GPU: the float64 restatement pinned to the reference's runs (``tests/golden/ref_sensevoice.npz`` / ``.json``), the engine's
host schedule dry-run over emulated operators, the ``sanm_shift`` fold, the config / checkpoint / loader rules, the C ABI of the three new entry points,
and the reference's own ``stt/tests/test_sensevoice.py`` cases restated against this package."""
import ctypes
import json
import math
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

import _margin  # noqa: E402
import _sensevoice_ref as R  # noqa: E402

FUNCS = ("mi355_sanm_input", "mi355_ctc_rows", "mi355_ctc_collapse")
STRUCTS = ("mi355_sanm_input_args", "mi355_ctc_rows_args", "mi355_ctc_collapse_args")


def rel_peak(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLD, "ref_sensevoice.npz"))


@pytest.fixture(scope="module")
def meta():
    with open(os.path.join(GOLD, "ref_sensevoice.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def models(meta):
    return R.load_models(meta)


def test_audio_regenerates(fx, models):
    for tag, (_, _, audios, _) in models.items():
        for i, a in enumerate(audios):
            assert a.shape[0] == R.n_samples(R.FRAMES[i])
            s = np.array([a.astype(np.float64).sum(), (a.astype(np.float64) ** 2).sum()])
            assert np.allclose(s, fx[f"{tag}{i}_audiosum"], rtol=1e-12), (tag, i)


def test_restatement_pinned_to_the_reference_runs(fx, meta, models):
    """float64 against the reference's float32 runs: stage tensors within 2e-5 of the peak, ids equal wherever the stored gap is at least THR
    (Parakeet's bars for the same comparison); tokens equal for every clip without a knife edge."""
    for tag, (cfg, w, audios, cmvn) in models.items():
        for i, a in enumerate(audios):
            r = R.forward(cfg, w, a, cmvn)
            rows = fx[f"{tag}{i}_layer_rows"]
            assert rel_peak(r["x"], fx[f"{tag}{i}_x"]) < 2e-5, (tag, i)
            assert rel_peak(r["attn0"].numpy(), fx[f"{tag}{i}_attn0"]) < 2e-5 and rel_peak(r["hidden"].numpy(), fx[f"{tag}{i}_hidden"]) < 2e-5, (tag, i)
            for j, lay in enumerate(fx[f"{tag}{i}_layers"]):
                assert rel_peak(r["layers"][j].numpy()[rows], lay) < 2e-5, (tag, i, j)
            ok = fx[f"{tag}{i}_gap"] >= _margin.THR
            assert np.array_equal(r["ids"].numpy()[ok], fx[f"{tag}{i}_ids"][ok])
            assert np.abs(r["gap"].numpy() - fx[f"{tag}{i}_gap"]).max() < 1e-4
            if ok.all():
                assert r["tokens"] == meta["configs"][tag]["decode"][i]["tokens"], (tag, i)


def test_apply_lfr_on_the_reference_test_input(fx):
    """``test_left_padding`` of the reference's stt/tests/test_sensevoice.py: arange(20) as one feature, LFR 7 / 6."""
    want = fx["lfr_arange"]
    got = R.apply_lfr(np.arange(20, dtype=np.float32).reshape(20, 1), 7, 6)
    assert want.shape == (4, 7) and np.array_equal(got, want)
    assert want[0].tolist() == [0, 0, 0, 0, 1, 2, 3] and want[3].tolist() == [15, 16, 17, 18, 19, 19, 19]


def _engine(cfg, w, cmvn, tmp=None):
    from mlx_audio_amd.stt.models.sensevoice import SenseVoiceSmall

    eng = SenseVoiceSmall(cfg, w, device="cpu")
    if cmvn is not None:
        eng.set_cmvn(*cmvn)
    eng._token_list = R.token_list(cfg.vocab_size)
    return eng


def test_host_schedule_dry_run(fx, meta, models):
    """The engine's host schedule (one ``sanm_input`` for the batch, the fused q | k | v views, the FSMN result as the out projection's residual, the
    first layer without its attention residual, the folded ``sanm_shift`` taps, the chunked head, one collapse) over CPU emulations of the operator
    contracts, against the reference's runs at 1e-4 of the peak: every clip alone and all clips of a config as one padded batch."""
    import _ops_emu_sensevoice

    with _ops_emu_sensevoice.patched():
        for tag, (cfg, w, audios, cmvn) in models.items():
            eng = _engine(cfg, w, cmvn)
            eng.ctc_chunk_rows = 7   # several chunks, the last one partial
            fbs = [eng._fbank(torch.from_numpy(a)) for a in audios]
            runs = [(eng.transcribe_fbank([f], R.LANGUAGE, R.USE_ITN, return_layers=True), 0, i) for i, f in enumerate(fbs)]
            rb = eng.transcribe_fbank(fbs, R.LANGUAGE, R.USE_ITN, return_layers=True)
            runs += [(rb, i, i) for i in range(len(fbs))]
            for r, row, i in runs:
                want_x = fx[f"{tag}{i}_x"]
                n = want_x.shape[0]
                assert r["out_lens"].dtype == torch.int32 and int(r["out_lens"][row]) == n
                assert rel_peak(r["x"][row, :n], want_x) < 1e-4 and not r["x"][row, n:].any(), (tag, i)
                assert rel_peak(r["taps"]["attn0"][row, :n], fx[f"{tag}{i}_attn0"]) < 1e-4 and rel_peak(r["hidden"][row, :n], fx[f"{tag}{i}_hidden"]) < 1e-4
                rows = fx[f"{tag}{i}_layer_rows"]
                for j, lay in enumerate(fx[f"{tag}{i}_layers"]):
                    assert rel_peak(r["taps"]["layers"][j][row, :n][rows], lay) < 1e-4, (tag, i, j)
                ok = fx[f"{tag}{i}_gap"] >= _margin.THR
                assert np.array_equal(r["ids"][row, :n].numpy()[ok], fx[f"{tag}{i}_ids"][ok]), (tag, i)
                assert np.abs(r["gap"][row, :n].numpy() - fx[f"{tag}{i}_gap"]).max() < 1e-3
                want = meta["configs"][tag]["decode"][i]
                if ok.all():
                    assert r["tokens"][row] == want["tokens"] and r["rich"][row] == want["rich"], (tag, i)
                    assert eng._decode_tokens(r["tokens"][row]) == want["text"]
            outs = eng.generate_batch([torch.from_numpy(a) for a in audios], language=R.LANGUAGE, use_itn=R.USE_ITN)
            for i, (o, a) in enumerate(zip(outs, audios)):
                want = meta["configs"][tag]["decode"][i]
                if (fx[f"{tag}{i}_gap"] >= _margin.THR).all():
                    assert o.text == want["text"] and o.segments == want["segments"] and o.language == want["rich"]["language"]
                    one = eng.generate(a, language=R.LANGUAGE, use_itn=R.USE_ITN, max_tokens=5, generation_stream=None, dtype=None)
                    assert one == o


def test_call_returns_log_probabilities_and_the_surface_methods_agree(fx, models):
    """``__call__`` on ``_extract_features``' output (the reference's two-step path) equals the fused path; ``_greedy_ctc_decode`` and
    ``_extract_rich_info`` on its rows give the fused path's tokens and tags; a language per item."""
    import _ops_emu_sensevoice

    cfg, w, audios, cmvn = models["B"]
    with _ops_emu_sensevoice.patched():
        eng = _engine(cfg, w, cmvn)
        a = torch.from_numpy(audios[4])
        feats = eng._extract_features(a)
        assert tuple(feats.shape) == (math.ceil(13 / 3), 200)
        want = R.apply_lfr(R.fbank(audios[4], cfg).astype(np.float64), 5, 3)
        want = (want + np.float32(cmvn[0]).astype(np.float64)) * np.float32(cmvn[1]).astype(np.float64)
        assert rel_peak(feats, want) < 1e-6
        logp = eng(feats[None], language=R.LANGUAGE, use_itn=R.USE_ITN)
        assert tuple(logp.shape) == (1, 4 + feats.shape[0], 300) and np.allclose(torch.logsumexp(logp.double(), -1).numpy(), 0, atol=1e-5)
        r = eng.transcribe_fbank([eng._fbank(a)], R.LANGUAGE, R.USE_ITN)
        assert np.array_equal(logp[0].argmax(-1).numpy(), r["ids"][0].numpy())
        toks, text = eng._greedy_ctc_decode(logp[0, 4:])
        assert toks == r["tokens"][0] and text == eng._decode_tokens(toks) and eng._extract_rich_info(logp[0, :4]) == r["rich"][0]
        tq, iq = eng._build_query(2, ["ja", "xx"], False)
        assert tuple(tq.shape) == (2, 1, 200) and tuple(iq.shape) == (2, 3, 200)
        assert torch.equal(iq[0, 0], eng.embed[11]) and torch.equal(iq[1, 0], eng.embed[0]) and torch.equal(iq[0, 1:], eng.embed[1:3]) and torch.equal(tq[0, 0], eng.embed[15])
        with pytest.raises(ValueError, match="languages"):
            eng._build_query(3, ["en", "zh"])
        eng._token_list = None
        assert eng._decode_tokens([5, 7]) == "5 7"


def test_sanm_shift_fold_equals_the_literal_asymmetric_pad():
    """A left padding of (K - 1) / 2 + shift is a centred kernel of K + 2 shift taps whose extra taps are zero: ``fold_fsmn_taps`` through the
    ``fsmn_memory`` contract against ``_forward_fsmn``'s literal pad."""
    import _ops_emu_s3
    from mlx_audio_amd.stt.models.sensevoice.sensevoice import fold_fsmn_taps

    g = torch.Generator().manual_seed(5)
    for K, shift, T in ((11, 2, 37), (5, 1, 3), (5, 2, 9), (11, 0, 20), (1, 0, 4)):
        v, taps = torch.randn(2, T, 12, generator=g), torch.randn(12, K, generator=g)
        folded = fold_fsmn_taps(taps, shift)
        assert tuple(folded.shape) == (12, K + 2 * shift) and torch.equal(folded[:, :K], taps) and not folded[:, K:].any()
        y = _ops_emu_s3.fsmn_memory(v, folded, torch.empty(2, T, 12, dtype=torch.float64))
        for b in range(2):
            assert rel_peak(y[b], R.fsmn(v[b].double(), taps.double(), shift)) < 1e-12, (K, shift)
    with pytest.raises(ValueError, match="MI355_FSMN_MAX_TAPS"):
        fold_fsmn_taps(torch.zeros(4, 29), 2)
    with pytest.raises(ValueError, match="right padding"):
        fold_fsmn_taps(torch.zeros(4, 5), 3)
    with pytest.raises(ValueError, match="odd"):
        fold_fsmn_taps(torch.zeros(4, 6), 0)


def test_position_table_is_the_reference_formula():
    from mlx_audio_amd.stt.models.sensevoice.sensevoice import position_table

    pe = position_table(300, 560)
    assert pe.dtype == torch.float32 and tuple(pe.shape) == (300, 560)
    assert np.abs(pe.double().numpy() - R.positions(300, 560)).max() < 2e-5   # float32 arguments up to 300 rad: 300 * 2^-24 in the angle
    assert abs(float(pe[0, 0]) - math.sin(1.0)) < 1e-7 and abs(float(pe[0, 280]) - math.cos(1.0)) < 1e-7
    with pytest.raises(ValueError, match="even"):
        position_table(4, 7)


def test_config_from_dict():
    from mlx_audio_amd.stt.models.sensevoice import EncoderConfig, FrontendConfig, ModelConfig

    c = ModelConfig()
    assert (c.model_type, c.vocab_size, c.input_size) == ("sensevoice", 25055, 560)
    assert (c.encoder_conf.output_size, c.encoder_conf.num_blocks, c.encoder_conf.tp_blocks, c.encoder_conf.kernel_size) == (512, 50, 20, 11)
    assert (c.encoder_conf.attention_heads, c.encoder_conf.linear_units, c.encoder_conf.sanm_shift, c.encoder_conf.normalize_before) == (4, 2048, 0, True)
    assert (c.encoder_conf.dropout_rate, c.encoder_conf.positional_dropout_rate, c.encoder_conf.attention_dropout_rate) == (0.1, 0.1, 0.1)
    fc = c.frontend_conf
    assert (fc.fs, fc.window, fc.n_mels, fc.frame_length, fc.frame_shift, fc.lfr_m, fc.lfr_n) == (16000, "hamming", 80, 25, 10, 7, 6)
    assert c.cmvn_means is None and c.cmvn_istd is None and c.model_path is None
    d = {"model_type": "sensevoice", "vocab_size": 25055, "input_size": 560, "unknown_key": 1,
         "encoder_conf": {"output_size": 512, "attention_heads": 4, "linear_units": 2048, "num_blocks": 50, "tp_blocks": 20, "kernel_size": 11,
                          "sanm_shfit": 3, "input_layer": "pe"},
         "frontend_conf": {"fs": 16000, "n_mels": 80, "lfr_m": 7, "lfr_n": 6, "cmvn_file": None}}
    c = ModelConfig.from_dict(d)
    assert c.encoder_conf.sanm_shift == 3 and c.frontend_conf.lfr_m == 7 and "encoder_conf" not in d   # popped, like the reference
    assert EncoderConfig.from_dict({"sanm_shfit": 3, "sanm_shift": 1}).sanm_shift == 1
    assert FrontendConfig.from_dict({"n_mels": 40, "x": 2}).n_mels == 40
    assert ModelConfig(encoder_conf={"sanm_shfit": 2}, frontend_conf={"lfr_n": 3}).encoder_conf.sanm_shift == 2
    assert isinstance(ModelConfig.from_dict({"encoder_conf": EncoderConfig(kernel_size=5)}).encoder_conf, EncoderConfig)


def test_sanitize_follows_the_two_rules():
    from mlx_audio_amd.stt.models.sensevoice import SenseVoiceSmall

    w = {"ctc.ctc_lo.weight": torch.zeros(100, 64), "ctc.ctc_lo.bias": torch.zeros(100), "embed.weight": torch.zeros(16, 560),
         "encoder.encoders.0.self_attn.fsmn_block.weight": torch.arange(64 * 11, dtype=torch.float32).reshape(64, 1, 11)}
    s = SenseVoiceSmall.sanitize(w)
    assert "ctc_lo.weight" in s and "ctc_lo.bias" in s and "ctc.ctc_lo.weight" not in s and "embed.weight" in s
    f = s["encoder.encoders.0.self_attn.fsmn_block.weight"]
    assert tuple(f.shape) == (64, 11, 1) and torch.equal(f[:, :, 0], w["encoder.encoders.0.self_attn.fsmn_block.weight"][:, 0, :])


def test_am_mvn_parsing_and_loader_priority(tmp_path, models):
    """``am.mvn`` takes priority over the config's statistics; sentencepiece only when importable AND the model file is there, else ``tokens.json``,
    else ids joined by spaces; hub names and bf16 checkpoints raise by name."""
    import _ops_emu_sensevoice
    from safetensors.torch import save_file

    from mlx_audio_amd.stt.models.sensevoice import SenseVoiceSmall
    from mlx_audio_amd.stt.models.sensevoice.sensevoice import BPE_MODEL, _parse_am_mvn

    cfg, w, audios, cmvn = models["B"]
    (tmp_path / "am.mvn").write_text(R.am_mvn_text(*cmvn))
    means, istd = _parse_am_mvn(str(tmp_path / "am.mvn"))
    assert means == cmvn[0] and istd == cmvn[1] and len(means) == 200
    (tmp_path / "bad.mvn").write_text("<Nnet>\n<Rescale> 2 2\n<LearnRateCoef> 0 [ 1 2 ]\n")
    with pytest.raises(ValueError, match="AddShift"):
        _parse_am_mvn(str(tmp_path / "bad.mvn"))
    conf = dict(R.CFG_B, encoder_conf=dict(R.CFG_B["encoder_conf"]), frontend_conf=dict(R.CFG_B["frontend_conf"]), cmvn_means=[0.5] * 200, cmvn_istd=[2.0] * 200)
    (tmp_path / "config.json").write_text(json.dumps(conf))
    save_file({k.replace("ctc_lo.", "ctc.ctc_lo."): (v.transpose(1, 2) if "fsmn_block" in k else v).contiguous() for k, v in w.items()}, str(tmp_path / "model.safetensors"))
    with _ops_emu_sensevoice.patched():
        eng = SenseVoiceSmall.from_pretrained(str(tmp_path), device="cpu")
        assert eng.config.encoder_conf.sanm_shift == 2 and eng.config.model_path == str(tmp_path)
        assert np.allclose(eng._cmvn_means.numpy(), np.float32(cmvn[0])) and np.allclose(eng._cmvn_istd.numpy(), np.float32(cmvn[1]))   # am.mvn wins
        assert eng._token_list is None and eng._tokenizer is None and eng._decode_tokens([3, 9]) == "3 9"
        os.remove(tmp_path / "am.mvn")
        (tmp_path / "tokens.json").write_text(json.dumps(R.token_list(300), ensure_ascii=False))
        (tmp_path / BPE_MODEL).write_bytes(b"")
        have_spm = True
        try:
            import sentencepiece  # noqa: F401
        except ImportError:
            have_spm = False
        if not have_spm:   # the file alone does not make a tokenizer: tokens.json is used
            eng = SenseVoiceSmall.from_pretrained(str(tmp_path), device="cpu")
            assert eng._tokenizer is None and eng._token_list == R.token_list(300)
        os.remove(tmp_path / BPE_MODEL)
        eng = SenseVoiceSmall.from_pretrained(str(tmp_path), device="cpu")
        assert float(eng._cmvn_means[0]) == 0.5 and float(eng._cmvn_istd[-1]) == 2.0 and eng._token_list == R.token_list(300)   # the config's statistics
        ref = _engine(cfg, w, ([0.5] * 200, [2.0] * 200))
        a = torch.from_numpy(audios[3])
        assert eng.generate(a, language="en").segments == ref.generate(a, language="en").segments
        with pytest.raises(ValueError, match="missing"):
            SenseVoiceSmall(cfg, {k: v for k, v in w.items() if "fsmn" not in k}, device="cpu")
        with pytest.raises(ValueError, match="unexpected"):
            SenseVoiceSmall(cfg, dict(w, extra=torch.zeros(1)), device="cpu")
        with pytest.raises(NotImplementedError, match="bf16"):
            SenseVoiceSmall(cfg, {k: v.to(torch.bfloat16) for k, v in w.items()}, device="cpu")
    with pytest.raises(FileNotFoundError, match="hub download"):
        SenseVoiceSmall.from_pretrained("mlx-community/SenseVoiceSmall")


def test_value_errors_and_registry(models):
    import _ops_emu_sensevoice
    import mlx_audio_amd.stt.models.sensevoice as pkg
    from mlx_audio_amd.stt.models.sensevoice import ModelConfig, SenseVoiceSmall

    assert not hasattr(pkg, "Model") and pkg.SenseVoiceSmall is SenseVoiceSmall and pkg.ModelConfig is ModelConfig
    cfg, w, audios, _ = models["A"]
    mk = lambda **enc: R.make_config(dict(R.CFG_A, encoder_conf=dict(R.CFG_A["encoder_conf"], **enc)))
    with _ops_emu_sensevoice.patched():
        with pytest.raises(ValueError, match="head width"):
            SenseVoiceSmall(mk(attention_heads=8, output_size=320), device="cpu")   # heads of 40
        with pytest.raises(ValueError, match="MI355_FSMN_MAX_TAPS"):
            SenseVoiceSmall(mk(kernel_size=29, sanm_shfit=2), device="cpu")
        with pytest.raises(ValueError, match="input_size"):
            SenseVoiceSmall(R.make_config(dict(R.CFG_A, input_size=512)), device="cpu")
        eng = SenseVoiceSmall(cfg, w, device="cpu")
        with pytest.raises(ValueError, match="too short"):
            eng.generate(torch.zeros(399))
        with pytest.raises(TypeError, match="Unsupported audio type"):
            eng.generate([0.0] * 800)
        with pytest.raises(ValueError, match="lengths"):
            eng(torch.zeros(2, 5, 560), lengths=[5, 0])
        with pytest.raises(ValueError, match="feats must be"):
            eng(torch.zeros(2, 5, 80))


def test_entry_points_declared_exported_and_refuse_null():
    from mlx_audio_amd import _lib

    lib = _lib.load()
    assert lib.mi355_abi_version() == 37 == _lib.ABI_VERSION   # three additive entry points: no layout changed, no bump
    for f, s in zip(FUNCS, STRUCTS):
        assert f in _lib.declared_functions() and hasattr(lib, f), f
        st = _lib.STRUCTS[s]()
        assert getattr(lib, f)(ctypes.byref(st), None) == -1 and b"null tensor" in lib.mi355_last_error(), f
        assert getattr(lib, f)(None, None) == -1


def test_struct_layouts_match_c(tmp_path):
    from mlx_audio_amd import _lib, ops

    src = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){"]
    for name in STRUCTS:
        src.append(f'printf("{name} %zu\\n", sizeof({name}));')
        for f, _ in _lib._STRUCT_DECLS[name]:
            src.append(f'printf("{name}.{f} %zu\\n", offsetof({name}, {f}));')
    src.append('printf("taps %d\\n", MI355_FSMN_MAX_TAPS);')
    src.append("return 0;}")
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", str(c), "-o", str(exe)], check=True)
    want = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.strip().splitlines())
    for name in STRUCTS:
        st = _lib.STRUCTS[name]
        assert ctypes.sizeof(st) == int(want[name]), name
        for f, _ in _lib._STRUCT_DECLS[name]:
            assert getattr(st, f).offset == int(want[f"{name}.{f}"]), (name, f)
    assert int(want["taps"]) == ops.FSMN_MAX_TAPS == 31


# ------------------------------------------------------------------ the reference's stt/tests/test_sensevoice.py, restated against this package
SMALL = dict(vocab_size=100, input_size=560, encoder_conf=dict(output_size=64, attention_heads=2, linear_units=128, num_blocks=3, tp_blocks=2, kernel_size=5))


@pytest.fixture(scope="module")
def small_model():
    """The reference tests' width-64 / 2-head model: heads of 32, the ``narrow_attention`` route."""
    import _ops_emu_sensevoice
    from mlx_audio_amd.stt.models.sensevoice import SenseVoiceSmall

    with _ops_emu_sensevoice.patched():
        eng = SenseVoiceSmall(R.make_config(SMALL), device="cpu", seed=3)
    return eng


def test_reference_cases_forward_shape_and_narrow_route(small_model):
    import _ops_emu_sensevoice
    from mlx_audio_amd import ops

    cfg = small_model.config
    calls = []
    with _ops_emu_sensevoice.patched():
        narrow = ops.narrow_attention
        ops.narrow_attention = lambda *a, **k: (calls.append(k["dh"]), narrow(*a, **k))[1]
        log_probs = small_model(torch.zeros(1, 10, 560), language="en")
        assert tuple(log_probs.shape) == (1, 14, 100)   # 4 query tokens + 10 feature frames
        assert calls == [32] * 5
        hidden = small_model.encode(*small_model._assemble(torch.zeros(1, 10, 560), [10], "auto", False, stacked=True))
        assert tuple(hidden.shape) == (1, 14, 64)
        x = torch.randn(1, 9, 560, generator=torch.Generator().manual_seed(1))
        want = R.encode(cfg, make_weights_small(), R.assemble_stacked(cfg, make_weights_small(), x[0].numpy(), "zh", False))
        got = small_model(x, language="zh")
        assert rel_peak(got[0], want["logp"].numpy()) < 1e-4


def make_weights_small():
    from mlx_audio_amd.stt.models.sensevoice import make_sensevoice_weights

    return make_sensevoice_weights(R.make_config(SMALL), 3)


def test_reference_cases_lfr_cmvn_and_positions():
    assert R.apply_lfr(np.ones((100, 80), dtype=np.float32), 7, 6).shape == (math.ceil(100 / 6), 560)
    assert R.apply_lfr(np.ones((10, 80), dtype=np.float32), 7, 6).shape == (math.ceil(10 / 6), 560)
    first = R.apply_lfr(np.arange(20, dtype=np.float32).reshape(20, 1), 7, 6)[0]
    assert first[:5].tolist() == [0.0, 0.0, 0.0, 0.0, 1.0]
    from mlx_audio_amd.stt.models.sensevoice.sensevoice import position_table

    assert tuple(position_table(10, 512).shape) == (10, 512) and bool(position_table(5, 64).any())
    # TestCMVN.test_basic through the sanm_input contract: zero means and unit inverse deviations leave the features alone
    import _ops_emu_sensevoice

    x, n = _ops_emu_sensevoice.sanm_input(torch.ones(1, 10, 560), torch.zeros(16, 560), torch.zeros(1, 4, dtype=torch.int32), None, lfr_m=1, lfr_n=1, scale=1.0,
                                          means=torch.zeros(560), istd=torch.ones(560))
    assert tuple(x.shape) == (1, 14, 560) and n.tolist() == [14] and bool((x[0, 4:] == 1).all()) and not x[0, :4].any()
