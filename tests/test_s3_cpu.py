"""S3 speech tokenizer v2 without a GPU: the float64 helper ``tests/_s3_ref.py`` pinned to the reference's own runs (``tests/golden/ref_s3_v2.npz``, made by
``tests/golden/make_s3_fixtures.py``), the batch meaning proved on those numbers, the host helpers, ``sanitize``, the window arithmetic of the long path,
the package surface, the two new C entry points, and a dry run of the engine's host schedule over CPU emulations of the operator contracts."""
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

import _s3_ref as R  # noqa: E402

S3_FUNCS = ("mi355_fsmn_memory", "mi355_fsq_encode")
S3_STRUCTS = ("mi355_fsmn_memory_args", "mi355_fsq_encode_args")


def rel_peak(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLD, "ref_s3_v2.npz"))


@pytest.fixture(scope="module")
def tiny(fx):
    from mlx_audio_amd.codec.models.s3.model_v2 import ModelConfig, make_s3_weights

    cfg = ModelConfig(**json.loads(str(fx["config"])))
    w = make_s3_weights(cfg, int(fx["seed_w"]))
    mels = [R.synth_mel(int(seed), cfg.n_mels, int(frames)) for frames, seed in fx["clips"]]
    return cfg, w, mels


def ref_forward(cfg, w, mel, lens):
    return R.forward({k: v.numpy() for k, v in w.items()}, cfg.n_audio_state, cfg.n_audio_head, cfg.n_audio_layer, mel, lens)


def test_mels_regenerate(fx, tiny):
    """The mels are not stored: a drifted generator must fail loudly."""
    cfg, _, mels = tiny
    for i, mel in enumerate(mels):
        got = np.array([mel.astype(np.float64).sum(), (mel.astype(np.float64) ** 2).sum()])
        assert np.allclose(got, fx[f"clip{i}_melsum"], rtol=1e-12), i
    frames, seed = fx["long"]
    mel = R.synth_mel(int(seed), cfg.n_mels, int(frames))
    assert np.allclose([mel.astype(np.float64).sum(), (mel.astype(np.float64) ** 2).sum()], fx["long_melsum"], rtol=1e-12)


def test_seeded_weights_have_the_reference_names_and_fp16_values(tiny):
    from mlx_audio_amd.codec.models.s3.model_v2 import expected_shapes

    cfg, w, _ = tiny
    assert {k: tuple(v.shape) for k, v in w.items()} == expected_shapes(cfg)
    assert w["encoder.blocks.0.attn.fsmn_block.weight"].shape == (128, 31, 1) and w["encoder.conv1.weight"].shape == (128, 3, 128)
    assert "encoder.blocks.0.attn.key.bias" not in w and "encoder.blocks.1.mlp.layers.2.bias" in w
    for k, v in w.items():
        assert torch.equal(v, v.to(torch.float16).to(torch.float32)), k


def test_helper_pinned_to_the_reference_runs(fx, tiny):
    """``_s3_ref.forward`` at B == 1 against every stored tensor (the reference ran in float32: 2e-5 of the peak), codes by the margin rule at 1e-4."""
    cfg, w, mels = tiny
    for i, mel in enumerate(mels):
        r = ref_forward(cfg, w, mel[None], [mel.shape[1]])
        n = int(fx[f"clip{i}_code_len"])
        assert int(r["code_len"][0]) == n == R.conv_len(R.conv_len(mel.shape[1])) and r["h"].shape[1] == n
        assert np.abs(r["h"][0] - fx[f"clip{i}_h"]).max() < 1e-4, i   # float32 reference against float64: |h| up to ~8
        if f"clip{i}_layers" in fx:
            for j, lay in enumerate(fx[f"clip{i}_layers"]):
                assert rel_peak(r["layers"][j][0], lay) < 2e-5, (i, j)
            assert rel_peak(r["fsmn0"][0], fx[f"clip{i}_fsmn0"]) < 2e-5, i
        ok = R.margins(fx[f"clip{i}_h"]) >= 1e-3
        assert ok.mean() > 0.97 and np.array_equal(r["codes"][0][ok], fx[f"clip{i}_codes"][ok]), i
        assert np.array_equal(R.fsq_codes(fx[f"clip{i}_h"]), fx[f"clip{i}_codes"])


def test_padded_batch_equals_each_item_alone(fx, tiny):
    """The meaning that is built: the valid frames of a sequence inside a right-padded batch equal that sequence run alone -- on the reference's numbers."""
    cfg, w, mels = tiny
    T = max(m.shape[1] for m in mels)
    batch = np.zeros((3, cfg.n_mels, T), dtype=np.float32)
    g = np.random.default_rng(1)
    for i, m in enumerate(mels):
        batch[i, :, :m.shape[1]] = m
        batch[i, :, m.shape[1]:] = g.standard_normal((cfg.n_mels, T - m.shape[1]))   # what lies in the padding must not matter
    r = ref_forward(cfg, w, batch, [m.shape[1] for m in mels])
    for i in range(3):
        n = int(fx[f"clip{i}_code_len"])
        assert int(r["code_len"][i]) == n
        assert np.abs(r["h"][i, :n] - fx[f"clip{i}_h"]).max() < 1e-4, i
        assert not r["codes"][i, n:].any()
        if f"clip{i}_layers" in fx:
            for j, lay in enumerate(fx[f"clip{i}_layers"]):
                assert rel_peak(r["layers"][j][i, :n], lay) < 2e-5, (i, j)
            assert rel_peak(r["fsmn0"][i, :n], fx[f"clip{i}_fsmn0"]) < 2e-5 and not r["fsmn0"][i, n:].any()


def test_utils_helpers(fx):
    from mlx_audio_amd.codec.models.s3 import make_non_pad_mask, mask_to_bias, merge_tokenized_segments, padding

    lens = torch.from_numpy(fx["util_lens"])
    m = make_non_pad_mask(lens)
    assert m.dtype == torch.bool and np.array_equal(m.numpy(), fx["util_mask"])
    assert np.array_equal(make_non_pad_mask(lens, 9).numpy(), fx["util_mask_max9"])
    assert np.array_equal(mask_to_bias(m, torch.float32).numpy(), fx["util_bias"])
    with pytest.raises(AssertionError):
        mask_to_bias(m.to(torch.float32))
    feats = [torch.arange(3 * n, dtype=torch.float32).reshape(3, n) + 1 for n in (4, 2, 6)]
    pf, pl = padding(feats)
    assert np.array_equal(pf.numpy(), fx["util_padded"]) and np.array_equal(pl.numpy(), fx["util_padded_lens"]) and pl.dtype == torch.int32
    assert np.array_equal(merge_tokenized_segments(json.loads(str(fx["util_merge_in"])), overlap=4, token_rate=25), fx["util_merge_out"])
    assert np.array_equal(merge_tokenized_segments([list(range(7))], overlap=4, token_rate=25), fx["util_merge_one"])


def test_sanitize(fx, tiny):
    from mlx_audio_amd.codec.models.s3.model_v2 import S3TokenizerV2, _sanitized

    cfg, _, _ = tiny
    shapes = json.loads(str(fx["sanitize_in"]))
    g = np.random.default_rng(5)
    sw = {k: torch.from_numpy(g.standard_normal(s).astype(np.float32)) for k, s in shapes.items()}
    res = _sanitized(S3TokenizerV2, cfg, sw)
    assert {k: list(v.shape) for k, v in res.items()} == json.loads(str(fx["sanitize_out"]))
    assert np.array_equal(sw["encoder.conv1.weight"].numpy(), fx["sanitize_conv1_in"]) and np.array_equal(res["encoder.conv1.weight"].numpy(), fx["sanitize_conv1"])
    again = _sanitized(S3TokenizerV2, cfg, res)   # idempotent
    assert all(torch.equal(again[k], res[k]) for k in res) and again.keys() == res.keys()


def test_package_surface():
    import mlx_audio_amd.codec.models.s3 as S3

    assert S3.__all__ == ["S3TokenizerV2", "ModelConfig", "log_mel_spectrogram", "make_non_pad_mask", "mask_to_bias", "padding", "merge_tokenized_segments",
                          "S3_SR", "S3_HOP", "S3_TOKEN_HOP", "S3_TOKEN_RATE", "SPEECH_VOCAB_SIZE"]
    assert (S3.S3_SR, S3.S3_HOP, S3.S3_TOKEN_HOP, S3.S3_TOKEN_RATE, S3.SPEECH_VOCAB_SIZE) == (16000, 160, 640, 25, 6561)
    c = S3.ModelConfig()
    assert (c.n_mels, c.n_audio_ctx, c.n_audio_state, c.n_audio_head, c.n_audio_layer, c.n_codebook_size) == (128, 1500, 1280, 20, 6, 6561)
    for name in ("__call__", "quantize", "quantize_simple", "_quantize_mixed_batch", "sanitize", "load_weights", "from_pretrained"):
        assert hasattr(S3.S3TokenizerV2, name), name


def test_entry_points_declared_exported_and_refuse_null():
    from mlx_audio_amd import _lib

    lib = _lib.load()
    assert lib.mi355_abi_version() == 37 == _lib.ABI_VERSION   # two additive entry points: no layout changed, no bump
    for f, s in zip(S3_FUNCS, S3_STRUCTS):
        assert f in _lib.declared_functions() and hasattr(lib, f), f
        st = _lib.STRUCTS[s]()
        assert getattr(lib, f)(ctypes.byref(st), None) == -1 and b"null tensor" in lib.mi355_last_error(), f
        assert getattr(lib, f)(None, None) == -1


def test_struct_layouts_match_c(tmp_path):
    from mlx_audio_amd import _lib, ops

    src = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){"]
    for name in S3_STRUCTS:
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
    for name in S3_STRUCTS:
        st = _lib.STRUCTS[name]
        assert ctypes.sizeof(st) == int(want[name]), name
        for f, _ in _lib._STRUCT_DECLS[name]:
            assert getattr(st, f).offset == int(want[f"{name}.{f}"]), (name, f)
    assert int(want["taps"]) == ops.FSMN_MAX_TAPS == 31


def test_value_errors(tiny):
    import _ops_emu_s3
    from mlx_audio_amd.codec.models.s3 import ModelConfig, S3TokenizerV2

    cfg, w, _ = tiny
    with _ops_emu_s3.patched():
        with pytest.raises(ValueError, match="head width"):
            S3TokenizerV2("speech_tokenizer_v2_25hz", ModelConfig(n_audio_state=128, n_audio_head=4, n_audio_layer=1), device="cpu")
        with pytest.raises(ValueError, match="neither v1 nor v2"):
            S3TokenizerV2("speech_tokenizer_25hz", cfg, weights=w, device="cpu")
        eng = S3TokenizerV2("speech_tokenizer_v2_25hz", cfg, weights=w, device="cpu")
        with pytest.raises(ValueError, match="2048"):
            eng.quantize_simple(torch.zeros(1, cfg.n_mels, 4 * 2048 + 1), [4 * 2048 + 1])
        with pytest.raises(ValueError, match="missing"):
            S3TokenizerV2("speech_tokenizer_v2_25hz", cfg, weights={k: v for k, v in w.items() if "fsmn" not in k}, device="cpu")


def test_host_schedule_dry_run(fx, tiny):
    """The engine's host schedule (pair views of the strided convs, the masks, the fused q | k | v views, rope on q and k in one call, the FSMN result as
    the out projection's residual, the FSQ head) over CPU emulations of the operator contracts, against the reference's runs: alone and as one batch."""
    import _ops_emu_s3
    from mlx_audio_amd.codec.models.s3 import S3TokenizerV2, padding

    cfg, w, mels = tiny
    with _ops_emu_s3.patched():
        eng = S3TokenizerV2("speech_tokenizer_v2_25hz", cfg, weights=w, device="cpu")
        batch, lens = padding([torch.from_numpy(m) for m in mels])
        runs = [(eng.encode(torch.from_numpy(m)[None], [m.shape[1]], return_layers=True, return_h=True), 0, i) for i, m in enumerate(mels)]
        rb = eng.encode(batch, lens, return_layers=True, return_h=True)
        runs += [(rb, i, i) for i in range(3)]
        for r, row, i in runs:
            n = int(fx[f"clip{i}_code_len"])
            assert r["codes"].dtype == torch.int32 and r["code_len"].dtype == torch.int32 and int(r["code_len"][row]) == n
            assert np.abs(r["h"][row, :n].numpy() - fx[f"clip{i}_h"]).max() < 1e-4, i
            if f"clip{i}_layers" in fx:
                for j, lay in enumerate(fx[f"clip{i}_layers"]):
                    assert rel_peak(r["layers"][j][row, :n], lay) < 2e-5, (i, j)
                assert rel_peak(r["fsmn0"][row, :n], fx[f"clip{i}_fsmn0"]) < 2e-5
            ok = R.margins(fx[f"clip{i}_h"]) >= 1e-3
            assert np.array_equal(r["codes"][row, :n].numpy()[ok], fx[f"clip{i}_codes"][ok])
            assert not r["codes"][row, n:].any()
        codes, code_len = eng(batch, lens)
        assert torch.equal(codes, rb["codes"]) and torch.equal(code_len, rb["code_len"])


def test_long_path_windows_and_merge(fx, tiny):
    """``_quantize_mixed_batch`` with the encoder replaced by a stub that hands back the reference's per-segment codes: the windows (3000 frames every
    2600), one batched call with true lengths, trimming, the merge and the zero padding, against the reference's own merge."""
    import _ops_emu_s3
    from mlx_audio_amd.codec.models.s3 import S3TokenizerV2

    cfg, w, _ = tiny
    frames = int(fx["long"][0])
    segs = [tuple(int(v) for v in s) for s in fx["long_segments"]]
    assert S3TokenizerV2._segments([frames, 400], [True, False]) == [(0, s, e - s) for s, e in segs] + [(1, 0, 400)]
    assert [e - s for s, e in segs] == [3000, 3000, 2300]
    seen = {}

    def stub(mel, mel_len, **kw):
        seen["shape"], seen["lens"] = tuple(mel.shape), list(mel_len)
        n = [R.conv_len(R.conv_len(v)) for v in mel_len]
        codes = torch.zeros((len(n), R.conv_len(R.conv_len(mel.shape[2]))), dtype=torch.int32)
        for j in range(3):
            codes[j, :n[j]] = torch.from_numpy(fx[f"long_seg{j}_codes"])
        codes[3, :n[3]] = 7
        codes[3, n[3]:] = 9999   # beyond code_len: must be trimmed away
        return dict(codes=codes, code_len=torch.tensor(n, dtype=torch.int32))

    with _ops_emu_s3.patched():
        eng = S3TokenizerV2("speech_tokenizer_v2_25hz", cfg, weights=w, device="cpu")
        eng.encode = stub
        mel = torch.zeros(2, cfg.n_mels, frames)
        codes, code_len = eng(mel, torch.tensor([frames, 400], dtype=torch.int32))
    assert seen["shape"] == (4, cfg.n_mels, 3000) and seen["lens"] == [3000, 3000, 2300, 400]
    merged = fx["long_merged"]
    assert codes.dtype == torch.int32 and code_len.tolist() == [len(merged), 100] and codes.shape == (2, len(merged))
    assert np.array_equal(codes[0].numpy(), merged)
    assert (codes[1, :100] == 7).all() and not codes[1, 100:].any()


def test_from_pretrained_local_directory(tmp_path, tiny):
    """A local directory holding ``{name}.safetensors`` with torch-style keys and conv layouts loads through ``sanitize``; a missing file is an error."""
    safetensors = pytest.importorskip("safetensors.torch")
    import _ops_emu_s3
    from mlx_audio_amd.codec.models.s3 import S3TokenizerV2

    cfg, w, mels = tiny
    name = "speech_tokenizer_v2_25hz"
    tw = {}
    for k, v in w.items():
        k2 = k.replace(".mlp.layers.", ".mlp.").replace("quantizer.fsq_codebook.", "quantizer._codebook.")
        tw[k2] = (v.swapaxes(1, 2) if v.dim() == 3 else v).contiguous()
    tw["encoder._freqs_cis"] = torch.zeros(4, 4)
    safetensors.save_file(tw, str(tmp_path / f"{name}.safetensors"))
    with _ops_emu_s3.patched():
        a = S3TokenizerV2.from_pretrained(name, str(tmp_path), config=cfg, device="cpu")
        b = S3TokenizerV2(name, cfg, weights=w, device="cpu")
        m = torch.from_numpy(mels[2])[None]
        ca, la = a(m, [m.shape[2]])
        cb, lb = b(m, [m.shape[2]])
        assert torch.equal(ca, cb) and torch.equal(la, lb) and la.tolist() == [10]
        with pytest.raises(FileNotFoundError):
            S3TokenizerV2.from_pretrained("speech_tokenizer_v2_50hz", str(tmp_path), config=cfg, device="cpu")
