"""Parakeet CTC without a GPU: the float64 restatement pinned to the reference's runs (``tests/golden/ref_parakeet_ctc.npz`` / ``.json``), the engine's host
schedule dry-run over emulated operators, the C ABI of the three new entry points, and the host-side decode pieces."""
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

import _margin  # noqa: E402
import _parakeet_ref as R  # noqa: E402

FUNCS = ("mi355_relpos_attention", "mi355_glu_dwconv_silu", "mi355_stencil2d_k3s2")
STRUCTS = ("mi355_relpos_attention_args", "mi355_glu_dwconv_silu_args", "mi355_stencil2d_k3s2_args")
STAGES = ("pre_encode", "layers", "attn0", "conv0")


def rel_peak(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLD, "ref_parakeet_ctc.npz"))


@pytest.fixture(scope="module")
def meta():
    with open(os.path.join(GOLD, "ref_parakeet_ctc.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def models(meta):
    return R.load_models(meta)


pad_batch = R.pad_batch


def test_mels_regenerate(fx, models):
    for tag, (_, _, mels) in models.items():
        for i, m in enumerate(mels):
            s = np.array([m.astype(np.float64).sum(), (m.astype(np.float64) ** 2).sum()])
            assert np.allclose(s, fx[f"{tag}{i}_melsum"], rtol=1e-12), (tag, i)


def test_seeded_weights_have_the_reference_names_and_fp16_values(models):
    args, w, _ = models["A"]
    assert all(torch.equal(v, v.to(torch.float16).to(torch.float32)) for v in w.values())
    p = "encoder.layers.0."
    assert tuple(w[p + "conv.depthwise_conv.weight"].shape) == (128, 9, 1) and tuple(w["encoder.pre_encode.conv.3.weight"].shape) == (32, 1, 1, 32)
    assert tuple(w["encoder.pre_encode.out.weight"].shape) == (128, 64) and tuple(w["decoder.decoder_layers.0.weight"].shape) == (len(R.VOCAB) + 1, 1, 128)
    assert float(w[p + "conv.batch_norm.running_mean"].abs().max()) > 0.1 and float((w[p + "conv.batch_norm.running_var"] - 1).abs().max()) > 0.1
    assert float(w[p + "self_attn.pos_bias_u"].abs().min()) > 0 and float(w[p + "self_attn.pos_bias_v"].abs().min()) > 0
    assert not any(k.endswith(".bias") and ".norm_" not in k and "batch_norm" not in k and k.startswith("encoder.layers") for k in models["B"][1])


def test_restatement_pinned_to_the_reference_runs(fx, models):
    """float64 against the reference's float32 runs: stage tensors within 2e-5 of the peak, ids equal wherever the stored gap is at least THR."""
    for tag, (args, w, mels) in models.items():
        for i, m in enumerate(mels):
            r = R.forward(args, w, m)
            assert r["out_len"] == int(fx[f"{tag}{i}_out_len"])
            for k in STAGES:
                if f"{tag}{i}_{k}" in fx:
                    assert rel_peak(r[k].numpy(), fx[f"{tag}{i}_{k}"]) < 2e-5, (tag, i, k)
            ok = fx[f"{tag}{i}_gap"] >= _margin.THR
            assert np.array_equal(r["ids"].numpy()[ok], fx[f"{tag}{i}_ids"][ok])
            assert np.abs(r["gap"].numpy() - fx[f"{tag}{i}_gap"]).max() < 1e-4


def test_host_schedule_dry_run(fx, meta, models):
    """The engine's host schedule (channels-last stencil stages, the permuted output linear, the folded half-steps and BatchNorm, the fused q | k | v
    views, one position table for a ragged batch) over CPU emulations of the operator contracts, against the reference's runs: every clip alone and
    all clips of a config as one padded batch; then the decode results."""
    import _ops_emu_parakeet
    from mlx_audio_amd.stt.models.parakeet import ParakeetCTC

    with _ops_emu_parakeet.patched():
        for tag, (args, w, mels) in models.items():
            eng = ParakeetCTC(args, w, device="cpu")
            batch, lens = pad_batch(mels)
            runs = [(eng.encoder(torch.from_numpy(m)[None], None, return_layers=True), 0, i) for i, m in enumerate(mels)]
            rb = eng.encoder(batch, lens, return_layers=True)
            runs += [(rb, i, i) for i in range(len(mels))]
            for (hidden, out_len, taps), row, i in runs:
                n = int(fx[f"{tag}{i}_out_len"])
                assert out_len.dtype == torch.int32 and int(out_len[row]) == n
                if f"{tag}{i}_layers" in fx:
                    assert rel_peak(taps["pre_encode"][row, :n], fx[f"{tag}{i}_pre_encode"]) < 1e-4, (tag, i)
                    for j, lay in enumerate(fx[f"{tag}{i}_layers"]):
                        assert rel_peak(taps["layers"][j][row, :n], lay) < 1e-4, (tag, i, j)
                    assert rel_peak(taps["attn0"][row, :n], fx[f"{tag}{i}_attn0"]) < 1e-4 and rel_peak(taps["conv0"][row, :n], fx[f"{tag}{i}_conv0"]) < 1e-4
                ids = eng.decoder.frame_ids(hidden)[row, :n].numpy()
                ok = fx[f"{tag}{i}_gap"] >= _margin.THR
                assert np.array_equal(ids[ok], fx[f"{tag}{i}_ids"][ok]), (tag, i)
            alone = [eng.decode(torch.from_numpy(m)[None])[0] for m in mels]
            together = eng.decode(batch, lens)
            for i, want in enumerate(meta["configs"][tag]["decode"]):
                if (fx[f"{tag}{i}_gap"] < _margin.THR).any():
                    continue
                for got in (alone[i], together[i]):
                    assert R.same_decode(R.result_dict(got), want), (tag, i)


def test_subsampling_factor_one_is_a_linear_pre_encode(models):
    import _ops_emu_parakeet
    from mlx_audio_amd.stt.models.parakeet import ParakeetCTC, make_parakeet_weights

    args = R.make_args(dict(R.ENC_A, subsampling_factor=1, n_layers=1))
    w = make_parakeet_weights(args, 5)
    assert tuple(w["encoder.pre_encode.weight"].shape) == (128, 16) and not any("pre_encode.conv" in k for k in w)
    mels = [R.synth_mel(7, 16, 37), R.synth_mel(8, 16, 12)]
    with _ops_emu_parakeet.patched():
        eng = ParakeetCTC(args, w, device="cpu")
        batch, lens = pad_batch(mels)
        hidden, out_len = eng.encoder(batch, lens)
        assert out_len.tolist() == [37, 12]
        for i, m in enumerate(mels):
            assert rel_peak(hidden[i, :lens[i]], R.forward(args, w, m)["layers"][-1].numpy()) < 1e-5


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
    src.append('printf("taps %d\\n", MI355_GLU_DWCONV_MAX_TAPS);')
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
    assert int(want["taps"]) == ops.GLU_DWCONV_MAX_TAPS == 31


def test_value_errors(models):
    import _ops_emu_parakeet
    from mlx_audio_amd.stt.models.parakeet import ParakeetCTC

    args, w, _ = models["A"]
    with _ops_emu_parakeet.patched():
        with pytest.raises(ValueError, match="rel_pos"):
            ParakeetCTC(R.make_args(dict(R.ENC_A, self_attention_model="abs_pos")), w, device="cpu")
        with pytest.raises(ValueError, match="odd"):
            ParakeetCTC(R.make_args(dict(R.ENC_A, conv_kernel_size=8)), w, device="cpu")
        with pytest.raises(ValueError, match="head width"):
            ParakeetCTC(R.make_args(dict(R.ENC_A, n_heads=4)), w, device="cpu")
        with pytest.raises(NotImplementedError, match="subsampling"):
            ParakeetCTC(R.make_args(dict(R.ENC_A, subsampling="striding")), w, device="cpu")
        with pytest.raises(ValueError, match="missing"):
            ParakeetCTC(args, {k: v for k, v in w.items() if "linear_pos" not in k}, device="cpu")
        eng = ParakeetCTC(args, w, device="cpu")
        with pytest.raises(ValueError, match="lengths"):
            eng.decode(torch.zeros(2, 20, 16), [20, 21])
        with pytest.raises(NotImplementedError, match="stream"):
            eng.generate(torch.zeros(16000), stream=True)
        with pytest.raises(NotImplementedError, match="chunk"):
            eng.generate(torch.zeros(3 * 16000), chunk_duration=1.0, overlap_duration=0.5)


def test_ctc_collapse_and_timestamps_on_scripted_rows(meta):
    """``a, blank, a`` emits ``a`` once (a blank does not reset the previous token); an all-blank row is empty; a trailing special token is dropped;
    one frame; against what the reference's own ``decode`` made of the same rows."""
    from mlx_audio_amd.stt.models.nemo.alignment import sentences_to_result, tokens_to_sentences
    from mlx_audio_amd.stt.models.parakeet.parakeet import ctc_collapse

    frame_time = lambda t: t * 8 / 16000 * 160
    rows = meta["scripted"]["collapse"]
    assert {"a_blank_a", "all_blank", "trailing_special", "single"} <= set(rows)
    for name, row in rows.items():
        got = R.result_dict(sentences_to_result(tokens_to_sentences(ctc_collapse(row["frames"], R.VOCAB, frame_time))))
        want = row["result"]
        assert R.same_decode(got, want), name
    assert rows["a_blank_a"]["result"]["ids"] == [5, 6, 5] and rows["all_blank"]["result"]["ids"] == [] and rows["trailing_special"]["result"]["ids"] == [1, 5]


def test_tokenizer_and_alignment_helpers(meta):
    from mlx_audio_amd.stt.models.nemo.alignment import AlignedToken, sentences_to_result, tokens_to_sentences
    from mlx_audio_amd.stt.models.parakeet import tokenizer

    s, V = meta["scripted"], len(R.VOCAB)
    assert [tokenizer.is_special_token(i, R.VOCAB) for i in range(-1, V + 2)] == s["special"]
    assert tokenizer.decode(list(range(-1, V + 2)), R.VOCAB) == s["decode_all"] and tokenizer.decode([1, 5, 3, 4, 0, 15, 2, 6], R.VOCAB) == s["decode_some"]
    toks = [AlignedToken(i, tokenizer.decode([i], R.VOCAB), 0.08 * n, 0.08) for n, i in enumerate(s["sentences_in"])]
    assert toks[3].end == toks[3].start + toks[3].duration
    got = R.result_dict(sentences_to_result(tokens_to_sentences(toks)))
    assert got == s["sentences"] and len(got["sentences"]) > 3
    assert R.result_dict(sentences_to_result(tokens_to_sentences([]))) == s["sentences_empty"]


def test_from_pretrained_local_directory(tmp_path, models):
    import _ops_emu_parakeet
    from safetensors.torch import save_file

    from mlx_audio_amd.stt.models.parakeet import ParakeetCTC
    from mlx_audio_amd.stt.models.parakeet.parakeet import Model

    args, w, mels = models["A"]
    (tmp_path / "config.json").write_text(json.dumps(R.config_dict(R.ENC_A)))
    save_file({k: v.contiguous() for k, v in w.items()}, str(tmp_path / "model.safetensors"))
    with _ops_emu_parakeet.patched():
        eng = Model.from_pretrained(str(tmp_path), device="cpu")
        assert isinstance(eng, ParakeetCTC) and eng.vocabulary == R.VOCAB and eng.encoder_config.conv_kernel_size == 9
        a = R.result_dict(eng.decode(torch.from_numpy(mels[2])[None])[0])
        b = R.result_dict(ParakeetCTC(args, w, device="cpu").decode(torch.from_numpy(mels[2])[None])[0])
        assert a == b
    with pytest.raises(FileNotFoundError, match="local directory"):
        Model.from_pretrained("mlx-community/parakeet-ctc-0.6b")


def test_transducer_configs_raise(models):
    from mlx_audio_amd.stt.models.parakeet import ParakeetRNNT, ParakeetTDT, ParakeetTDTCTC
    from mlx_audio_amd.stt.models.parakeet.parakeet import Model

    rnnt = "nemo.collections.asr.models.rnnt_bpe_models.EncDecRNNTBPEModel"
    hybrid = "nemo.collections.asr.models.hybrid_rnnt_ctc_bpe_models.EncDecHybridRNNTCTCBPEModel"
    for cfg, name in ((dict(target=rnnt, model_defaults=dict(tdt_durations=[0, 1, 2])), "ParakeetTDT"), (dict(target=rnnt), "ParakeetRNNT"),
                      (dict(target=hybrid, model_defaults=dict(tdt_durations=[0, 1])), "ParakeetTDTCTC")):
        with pytest.raises(NotImplementedError, match=name + ".*encoder"):
            Model.from_config(cfg)
    for cls in (ParakeetTDT, ParakeetRNNT, ParakeetTDTCTC):
        with pytest.raises(NotImplementedError, match="encoder"):
            cls(None)
    with pytest.raises(ValueError, match="not supported"):
        Model.from_config(dict(target="something.else"))
