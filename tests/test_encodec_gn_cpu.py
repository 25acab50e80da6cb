"""CPU checks of the ``time_group_norm`` EnCodec (the 48 kHz model's GroupNorm behind every conv): the restated helper against the reference's own run,
the ABI of the three group-norm entry points, and the synthetic-weight makers (existing seeds must keep their tensors)."""
import ctypes
import hashlib
import json
import os
import subprocess

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
HEADER = os.path.join(ROOT, "include", "mi355audio.h")
GN_STRUCTS = ("mi355_group_norm_stats_args", "mi355_group_norm_coef_args", "mi355_group_norm_apply_args")
GN_FUNCS = ("mi355_group_norm_stats", "mi355_group_norm_coef", "mi355_group_norm_apply")

ENCODEC_TINY = dict(audio_channels=1, num_filters=8, kernel_size=7, num_residual_layers=1, dilation_growth_rate=2, codebook_size=64, codebook_dim=32,
                    hidden_size=32, num_lstm_layers=2, residual_kernel_size=3, use_causal_conv=True, normalize=False, pad_mode="reflect",
                    norm_type="weight_norm", last_kernel_size=7, trim_right_ratio=1.0, compress=2, upsampling_ratios=[4, 2, 2],
                    target_bandwidths=[15.0, 60.0], sampling_rate=24000)
ENCODEC_ENC_STEREO = dict(audio_channels=2, num_filters=8, kernel_size=7, num_residual_layers=1, dilation_growth_rate=2, codebook_size=64, codebook_dim=32,
                          hidden_size=32, num_lstm_layers=1, residual_kernel_size=3, use_causal_conv=False, normalize=True, pad_mode="reflect",
                          norm_type="weight_norm", last_kernel_size=7, trim_right_ratio=1.0, compress=2, upsampling_ratios=[5, 2, 2],
                          target_bandwidths=[18.0, 60.0], sampling_rate=24000, chunk_length_s=0.05, overlap=0.2)


def gn_model_weights(fx):
    from mlx_audio_amd.codec.models.encodec import make_encodec_encoder_weights, make_encodec_weights

    c = json.loads(str(fx["config"]))
    w = make_encodec_weights(c, seed=int(fx["seed_w"]))
    w.update(make_encodec_encoder_weights(c, seed=int(fx["seed_w"])))
    return c, w


def rel_peak(a, b):
    a, b = torch.as_tensor(np.asarray(a)).double(), torch.as_tensor(np.asarray(b)).double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max() / b.abs().max())


def normalised_chunks(c, x, m, chunk, stride):
    """The chunks of ``Encodec.encode`` with the loudness normalisation of ``_encode_frame`` applied (encodec.py:556-583)."""
    step = chunk - stride
    for off in range(0, x.shape[1] - step, stride):
        xc, mc = x[:, off:off + chunk], m[:, off:off + chunk]
        if c["normalize"]:
            xc = xc * mc[..., None].to(xc.dtype)
            mono = xc.sum(dim=2, keepdim=True) / xc.shape[2]
            xc = xc / (torch.sqrt((mono ** 2).mean(dim=1, keepdim=True)) + 1e-8)
        yield xc


def test_gn_helper_reproduces_the_reference_run():
    """``tests/_encodec_gn_ref.py`` against ``ref_encodec_gn_stereo.npz`` (the reference's unmodified encodec.py over the numpy stand-in): per-chunk
    embeddings, the decoder's stage tensors and the decoded audio within 2e-5 of the peak, every code equal (a decision whose stored reference gap is
    below the embeddings' deviation times the bound's safety factor would be a knife edge; none may be needed beyond those)."""
    from _encodec_gn_ref import EncodecGNRef

    fx = np.load(os.path.join(GOLD, "ref_encodec_gn_stereo.npz"))
    c, w = gn_model_weights(fx)
    assert c["norm_type"] == "time_group_norm" and sum(k.endswith(".norm.weight") for k in w) == sum(k.endswith(".conv.weight") for k in w)
    ref = EncodecGNRef(w, c)
    x, m = torch.from_numpy(fx["inputs"]), torch.from_numpy(fx["masks"])
    chunk, stride = ref.chunk_length, ref.chunk_stride
    embs = [ref.encoder(xc) for xc in normalised_chunks(c, x, m, chunk, stride)]
    assert len(embs) == fx["embeddings"].shape[0] == 3
    for ci, e in enumerate(embs):
        err = rel_peak(e, fx["embeddings"][ci])
        print(f"chunk {ci}: embeddings {err:.2e} of the peak")
        assert err < 2e-5, (ci, err)
    for bw in c["target_bandwidths"]:
        codes, scales = ref.encode(x, m, bandwidth=bw)
        want, gaps = fx[f"codes_bw{bw}"], fx[f"gaps_bw{bw}"]
        assert rel_peak(torch.stack(scales), fx[f"scales_bw{bw}"]) < 1e-6
        diff = codes.numpy() != want
        # a code may differ only at a knife edge of the reference itself: gap below the helper's own deviation on the embeddings (2e-5 of the peak)
        edge = 2e-5 * float(np.abs(fx["embeddings"]).max()) * 3.0
        first = np.zeros_like(diff)
        for ci in range(diff.shape[0]):
            for t in range(diff.shape[3]):
                nz = np.nonzero(diff[ci, 0, :, t])[0]
                if nz.size:
                    first[ci, 0, nz[0], t] = True      # later layers of that frame follow another residual
        assert (gaps[first] < edge).all(), (bw, gaps[first])
        print(f"bandwidth {bw}: {int(first.sum())} of {diff.size} decisions at a reference knife edge (gap < {edge:.1e})")
    dec = {}
    z = ref.quantizer_decode(torch.from_numpy(fx[f"codes_bw{c['target_bandwidths'][-1]}"][0]).long())
    assert rel_peak(z, fx["dec_z"]) < 1e-6
    out, st = ref.decoder(torch.from_numpy(fx["dec_z"]), return_stages=True)
    st["out"] = out
    for k, v in st.items():
        dec[k] = rel_peak(v, fx["dec_" + k])
    print("decoder stages:", {k: f"{v:.1e}" for k, v in dec.items()})
    assert max(dec.values()) < 2e-5, dec
    bw = c["target_bandwidths"][-1]
    audio = ref.decode(torch.from_numpy(fx[f"codes_bw{bw}"]).long(), [torch.from_numpy(s) for s in fx[f"scales_bw{bw}"]], m)
    err = rel_peak(audio, fx["decoded"])
    print(f"decoded audio: {err:.2e} of the peak")
    assert err < 2e-5, err


def test_gn_helper_float64_matches_float32():
    """The helper runs in float64 too (the GPU tests of the real 48 kHz shapes use it as the exact side)."""
    from _encodec_gn_ref import EncodecGNRef

    fx = np.load(os.path.join(GOLD, "ref_encodec_gn_stereo.npz"))
    c, w = gn_model_weights(fx)
    a = EncodecGNRef(w, c).decoder(torch.from_numpy(fx["dec_z"]))
    b = EncodecGNRef(w, c, dtype=torch.float64).decoder(torch.from_numpy(fx["dec_z"]).double())
    assert b.dtype == torch.float64 and rel_peak(a, b) < 2e-5


def test_group_norm_abi():
    from mlx_audio_amd import _lib

    lib = _lib.load()
    assert lib.mi355_abi_version() == 37 == _lib.ABI_VERSION
    for f in GN_FUNCS:
        assert f in _lib.declared_functions() and hasattr(lib, f), f
    # null arguments are refused before any launch
    for f, s in zip(GN_FUNCS, GN_STRUCTS):
        st = _lib.STRUCTS[s]()
        assert getattr(lib, f)(ctypes.byref(st), None) == -1 and b"null tensor" in lib.mi355_last_error(), f
        assert getattr(lib, f)(None, None) == -1


def test_group_norm_struct_layouts_match_c(tmp_path):
    from mlx_audio_amd import _lib

    src = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){"]
    for name in GN_STRUCTS:
        src.append(f'printf("{name} %zu\\n", sizeof({name}));')
        for f, _ in _lib._STRUCT_DECLS[name]:
            src.append(f'printf("{name}.{f} %zu\\n", offsetof({name}, {f}));')
    src.append('printf("part %d\\n", MI355_GN_PART_ELEMS);')
    src.append("return 0;}")
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", str(c), "-o", str(exe)], check=True)
    want = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.strip().splitlines())
    for name in GN_STRUCTS:
        st = _lib.STRUCTS[name]
        assert ctypes.sizeof(st) == int(want[name]), name
        for f, _ in _lib._STRUCT_DECLS[name]:
            assert getattr(st, f).offset == int(want[f"{name}.{f}"]), (name, f)
    from mlx_audio_amd import ops

    assert int(want["part"]) == ops.GN_PART_ELEMS


def _hash(w):
    d = hashlib.sha256()
    for k in sorted(w):
        d.update(k.encode())
        d.update(str(tuple(w[k].shape)).encode())
        d.update(w[k].contiguous().numpy().tobytes())
    return d.hexdigest()[:16]


# sha256 (first 16 hex digits) of make_encodec_weights + make_encodec_encoder_weights on the commit BEFORE the norm parameters existed
PARENT_HASHES = {"tiny:3": "d2c4adab730648f3", "tiny:41": "07b4d6cd46ae1bc1", "tiny:43": "94066bf6dbc2295c",
                 "stereo:3": "42fd339fae24003c", "stereo:41": "94c0640f422b22b4", "stereo:43": "cd1de3545ae1fb0c"}


def test_weight_makers_keep_existing_seeds():
    """``weight_norm`` configs: bit-identical tensors to the parent commit's; ``time_group_norm``: the SAME conv / LSTM / codebook tensors plus the norm
    parameters (from a generator of their own), one (weight, bias) pair per conv, away from the identity."""
    from mlx_audio_amd.codec.models.encodec import make_encodec_encoder_weights, make_encodec_weights

    for cn, c in (("tiny", ENCODEC_TINY), ("stereo", ENCODEC_ENC_STEREO)):
        for seed in (3, 41, 43):
            w = {**make_encodec_weights(c, seed), **make_encodec_encoder_weights(c, seed)}
            assert not any(".norm." in k for k in w)
            assert _hash(w) == PARENT_HASHES[f"{cn}:{seed}"], (cn, seed)
            g = dict(c, norm_type="time_group_norm")
            wg = {**make_encodec_weights(g, seed), **make_encodec_encoder_weights(g, seed)}
            assert _hash({k: v for k, v in wg.items() if ".norm." not in k}) == PARENT_HASHES[f"{cn}:{seed}"]
            convs = [k[:-len(".conv.weight")] for k in wg if k.endswith(".conv.weight")]
            for n in convs:
                nw, nb = wg[n + ".norm.weight"], wg[n + ".norm.bias"]
                assert nw.shape == nb.shape == (wg[n + ".conv.weight"].shape[0],)
            allw = torch.cat([wg[n + ".norm.weight"] for n in convs])
            assert float((allw - 1).abs().mean()) > 0.05 and float(torch.cat([wg[n + ".norm.bias"] for n in convs]).abs().mean()) > 0.02
    # the reference's parameter names (encodec.py:340-437 module indices)
    g = dict(ENCODEC_ENC_STEREO, norm_type="time_group_norm")
    wg = {**make_encodec_weights(g, 1), **make_encodec_encoder_weights(g, 1)}
    for k in ("encoder.layers.0.norm.weight", "encoder.layers.1.block.1.norm.weight", "encoder.layers.1.shortcut.norm.weight", "decoder.layers.3.norm.weight",
              "decoder.layers.0.norm.bias"):
        assert k in wg, k


def test_gn_host_schedule_dry_run():
    """The engine's ``time_group_norm`` schedule (pending norms as conv prologues, the untrimmed transposed conv with a row offset, two-operand applies,
    all chunks as one batch) over CPU emulations of the operator contracts (tests/_ops_emu.py, tests/_ops_emu_gn.py), against the reference's own run;
    and the variants the fixture does not reach (zero padding, no conv shortcut) against the restated helper."""
    import _ops_emu_gn
    from _encodec_gn_ref import EncodecGNRef
    from mlx_audio_amd.codec.models.encodec import Encodec, make_encodec_encoder_weights, make_encodec_weights

    fx = np.load(os.path.join(GOLD, "ref_encodec_gn_stereo.npz"))
    c, w = gn_model_weights(fx)
    x, m = torch.from_numpy(fx["inputs"]), torch.from_numpy(fx["masks"])
    with _ops_emu_gn.patched():
        eng = Encodec(c, weights=w, device="cpu")
        for ci, xc in enumerate(normalised_chunks(c, x, m, eng.chunk_length, eng.chunk_stride)):
            assert rel_peak(eng._encoder(xc), fx["embeddings"][ci]) < 3e-5, ci
        for bw in c["target_bandwidths"]:
            codes, scales = eng.encode(x, m, bandwidth=bw)
            assert codes.dtype == torch.int64 and np.array_equal(codes.numpy(), fx[f"codes_bw{bw}"]), bw
            assert rel_peak(torch.stack(scales), fx[f"scales_bw{bw}"]) < 1e-6
        out, st = eng._decoder(torch.from_numpy(fx["dec_z"]), return_stages=True)
        st["out"] = out
        for k, v in st.items():
            assert rel_peak(v, fx["dec_" + k]) < 3e-5, k
        audio = eng.decode(codes, scales, m)
        assert rel_peak(audio, fx["decoded"]) < 5e-5
        w2 = {k: v for k, v in w.items() if k != "encoder.layers.1.shortcut.norm.bias"}
        try:
            Encodec(c, weights=w2, device="cpu")
            raise AssertionError("strict loading accepted a checkpoint without encoder.layers.1.shortcut.norm.bias")
        except KeyError as e:
            assert "encoder.layers.1.shortcut.norm.bias" in str(e)
        c2 = dict(ENCODEC_TINY, norm_type="time_group_norm", pad_mode="constant", use_conv_shortcut=False)
        w2 = {**make_encodec_weights(c2, 41), **make_encodec_encoder_weights(c2, 41)}
        eng2, ref2 = Encodec(c2, weights=w2, device="cpu"), EncodecGNRef(w2, c2)
        g = torch.Generator().manual_seed(3)
        xa = 0.3 * torch.randn(2, 16 * 13, 1, generator=g)
        _, est = ref2.encoder(xa, return_stages=True)
        _, gst = eng2._encoder(xa, return_stages=True)
        for k in est:
            assert rel_peak(gst[k], est[k]) < 3e-5, k
        z = torch.randn(2, 9, 32, generator=g)
        want, dst = ref2.decoder(z, return_stages=True)
        got, dgs = eng2._decoder(z, return_stages=True)
        for k in dst:
            assert rel_peak(dgs[k], dst[k]) < 3e-5, k
        assert rel_peak(got, want) < 3e-5
