"""EnCodec with ``norm_type = "time_group_norm"`` (the 48 kHz model: GroupNorm(1, C) behind every conv) on the device: against the reference's own run
(tests/golden/ref_encodec_gn_stereo.npz) and, at the real 48 kHz sizes, against the restated helper tests/_encodec_gn_ref.py."""
import json
import os

import numpy as np
import pytest
import torch

import _margin

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

CFG48 = dict(audio_channels=2, num_filters=32, kernel_size=7, num_residual_layers=1, dilation_growth_rate=2, codebook_size=1024, codebook_dim=128,
             hidden_size=128, num_lstm_layers=2, residual_kernel_size=3, use_causal_conv=False, normalize=True, pad_mode="reflect",
             norm_type="time_group_norm", last_kernel_size=7, trim_right_ratio=1.0, compress=2, upsampling_ratios=[8, 5, 4, 2],
             target_bandwidths=[3.0, 6.0, 12.0, 24.0], sampling_rate=48000, chunk_length_s=1.0, overlap=0.01)


def rel_peak(a, b):
    a, b = torch.as_tensor(np.asarray(a.cpu() if torch.is_tensor(a) else a)).double(), torch.as_tensor(np.asarray(b)).double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max() / b.abs().max())


def snr_db(got, want):
    got, want = got.double().cpu(), want.double().cpu()
    return float(10 * torch.log10((want ** 2).sum() / ((got - want) ** 2).sum().clamp_min(1e-300)))


def weights_of(c, seed):
    from mlx_audio_amd.codec.models.encodec import make_encodec_encoder_weights, make_encodec_weights

    return {**make_encodec_weights(c, seed=seed), **make_encodec_encoder_weights(c, seed=seed)}


def normalised(c, xc, mc):
    if c["normalize"]:
        xc = xc * mc[..., None].to(xc.dtype)
        mono = xc.sum(dim=2, keepdim=True) / xc.shape[2]
        xc = xc / (torch.sqrt((mono ** 2).mean(dim=1, keepdim=True)) + 1e-8)
    return xc


def resync(eng, emb, bw, want, wm, thr, what, forced_count):
    """Margin rule with re-synchronisation (tests/_margin.py walk_forced, family "encodec_encode"): the reference's code is forced wherever ITS top-2 gap
    is below ``thr``; every other decision must equal the reference's; the gap difference on the compared decisions stays below ``thr``."""
    want, wm = torch.as_tensor(want).long().cpu(), torch.as_tensor(wm).cpu()
    mask = wm < thr
    got, gm = eng.quantizer.encode(emb, bw, return_margins=True, force=(mask, want))
    torch.cuda.synchronize()
    got, gm = got.cpu(), gm.cpu()
    assert tuple(got.shape) == tuple(want.shape)
    noise = float((gm - wm)[~mask].abs().max()) if (~mask).any() else 0.0
    print(f"encodec_encode {what}: {int(mask.sum())} of {mask.numel()} decisions forced (reference gap < {thr:.1e}); gap difference on the rest: max {noise:.2e}")
    assert noise < thr, (what, noise, thr)
    for b in range(got.shape[0]):
        for t in range(got.shape[2]):
            _margin.walk_forced("encodec_encode", got[b, :, t].tolist(), want[b, :, t].tolist(), mask[b, :, t].tolist(), where=(what, b, t))
    forced_count[0] += int(mask.sum())
    forced_count[1] += mask.numel()


def test_gn_engine_vs_the_reference_run():
    """Encoder embeddings < 2e-3 of the peak, scales < 1e-5, decoder stage tensors < 2e-3, decoded audio within 2e-3 of the peak and >= 50 dB; codes under
    the margin rule (forced where the REFERENCE's stored gap < 2e-3 * peak(embeddings) * 3; at most 5 % of the decisions forced)."""
    from mlx_audio_amd.codec.models.encodec import Encodec

    fx = np.load(os.path.join(GOLD, "ref_encodec_gn_stereo.npz"))
    c = json.loads(str(fx["config"]))
    eng = Encodec(c, weights=weights_of(c, int(fx["seed_w"])), device=DEV)
    x, m = torch.from_numpy(fx["inputs"]), torch.from_numpy(fx["masks"])
    chunk, stride = eng.chunk_length, eng.chunk_stride
    forced = [0, 0]
    embs = []
    for ci, off in enumerate(range(0, x.shape[1] - (chunk - stride), stride)):
        emb = eng._encoder(normalised(c, x[:, off:off + chunk], m[:, off:off + chunk]))
        torch.cuda.synchronize()
        e = rel_peak(emb, fx["embeddings"][ci])
        print(f"time_group_norm encoder chunk {ci} vs the reference run: {e:.2e} of the peak")
        assert e < 2e-3, (ci, e)
        embs.append(emb)
    for bw in c["target_bandwidths"]:
        want = torch.from_numpy(fx[f"codes_bw{bw}"]).long()
        codes, scales = eng.encode(x, m, bandwidth=bw)
        torch.cuda.synchronize()
        assert tuple(codes.shape) == tuple(want.shape) and codes.dtype == torch.int64 and len(scales) == want.shape[0]
        assert rel_peak(torch.stack(scales), fx[f"scales_bw{bw}"]) < 1e-5
        for ci in range(want.shape[0]):
            thr = 2e-3 * float(np.abs(fx["embeddings"][ci]).max()) * 3.0
            resync(eng, embs[ci], bw, want[ci], fx[f"gaps_bw{bw}"][ci], thr, f"reference run bw {bw} chunk {ci}", forced)
        agree = float((codes.cpu() == want).float().mean())
        print(f"time_group_norm encode bw {bw}: {100 * agree:.1f} % of all codes equal the reference's (free-running, batched chunks)")
    assert forced[0] <= 0.05 * forced[1], forced
    bw = c["target_bandwidths"][-1]
    want_codes = torch.from_numpy(fx[f"codes_bw{bw}"]).long()
    _, gst = eng._decoder(torch.from_numpy(fx["dec_z"]).to(DEV), return_stages=True)
    out, _ = eng._decoder(torch.from_numpy(fx["dec_z"]).to(DEV), return_stages=True)
    gst["out"] = out
    torch.cuda.synchronize()
    errs = {k: rel_peak(v, fx["dec_" + k]) for k, v in gst.items()}
    print("time_group_norm decoder stages vs the reference run:", {k: f"{v:.1e}" for k, v in errs.items()})
    assert max(errs.values()) < 2e-3, errs
    got = eng.decode(want_codes, [torch.from_numpy(s) for s in fx[f"scales_bw{bw}"]], m).cpu()
    want = torch.from_numpy(fx["decoded"])
    err, peak = float((got - want).abs().max()), float(want.abs().max())
    print(f"time_group_norm decode vs the reference run: max-abs {err:.2e} (peak {peak:.2f}), SNR {snr_db(got, want):.1f} dB")
    assert got.shape == want.shape and err <= 2e-3 * peak and snr_db(got, want) >= 50.0


def make_audio48(n, seed):
    g = np.random.default_rng(seed)
    t = np.arange(n) / 48000.0
    raw = np.stack([0.5 * np.sin(2 * np.pi * (210 + 130 * ch) * t) * (0.6 + 0.4 * np.sin(2 * np.pi * 9 * t)) + 0.15 * g.standard_normal(n) for ch in range(2)], axis=1)
    return torch.from_numpy(raw.astype(np.float32))


@pytest.fixture(scope="module")
def model48():
    from _encodec_gn_ref import EncodecGNRef
    from mlx_audio_amd.codec.models.encodec import Encodec

    # conv / LSTM weights on the fp16 grid: the engine holds float32 checkpoints as fp16 MFMA images, which is then exact (the practice of the 24 kHz
    # twin, tests/test_codec_encode_gpu.py test_encodec_24khz_encode_stages_and_codes_vs_oracle) -- the comparison is of the arithmetic, not of the storage format
    w = {k: (v.half().float() if v.is_floating_point() and "codebook" not in k else v) for k, v in weights_of(CFG48, 7).items()}
    return Encodec(CFG48, weights=w, device=DEV), EncodecGNRef(w, CFG48), w


def test_gn_48khz_one_chunk(model48):
    """The real 48 kHz config (32 filters, rates 8 / 5 / 4 / 2, two 512-wide LSTM layers, 16 codebooks of 1024 x 128), one 1 s stereo chunk against the
    float32 helper: embeddings, codes under the margin rule, scales, decoded audio."""
    eng, ref, _ = model48
    assert eng.chunk_length == 48000 and eng.chunk_stride == 47520 and eng.quantizer.num_quantizers == 16 and eng.enc["lstm"][0]["H"] == 512
    x = make_audio48(48000, 1)[None]
    m = torch.ones(1, 48000, dtype=torch.bool)
    bw = 6.0
    xn = normalised(CFG48, x, m)
    er = ref.encoder(xn)
    emb = eng._encoder(xn)
    torch.cuda.synchronize()
    e = rel_peak(emb, er)
    print(f"48 kHz encoder, one chunk: {e:.2e} of the peak")
    assert emb.shape == (1, 150, 128) and e < 2e-3, e
    wc, wm = ref.quantizer_encode(er, bw, return_margins=True)
    forced = [0, 0]
    resync(eng, emb, bw, wc, wm, 2e-3 * float(er.abs().max()) * 3.0, "48 kHz one chunk", forced)
    assert forced[0] <= 0.05 * forced[1], forced
    codes, scales = eng.encode(x, m, bandwidth=bw)
    wcodes, wscales = ref.encode(x, m, bandwidth=bw)
    assert codes.shape == wcodes.shape == (1, 1, 4, 150) and rel_peak(torch.stack(scales), torch.stack(wscales)) < 1e-5
    got = eng.decode(wcodes, wscales, m).cpu()
    want = ref.decode(wcodes, wscales, m)
    err, peak = float((got - want).abs().max()), float(want.abs().max())
    print(f"48 kHz decode, one chunk: max-abs {err:.2e} (peak {peak:.2f}), SNR {snr_db(got, want):.1f} dB")
    assert got.shape == want.shape == (1, 48000, 2) and err <= 2e-3 * peak and snr_db(got, want) >= 50.0


def test_gn_48khz_batched_chunks(model48):
    """B = 2 clips of different lengths x 3 chunks through ``preprocess_audio`` -> ``encode`` -> ``decode``: all chunks run as ONE batch of 6 samples.
    Against the helper (same bars), and against a chunk-by-chunk run of the same engine (2e-3 of the peak, 50 dB: kernel choice depends on tile count)."""
    from mlx_audio_amd.codec.models.encodec.encodec import preprocess_audio

    eng, ref, _ = model48
    chunk, stride = eng.chunk_length, eng.chunk_stride
    raw = [make_audio48(2 * stride + 30000, 2), make_audio48(2 * stride + 9000, 3)]
    x, m = preprocess_audio(raw, 48000, chunk, stride)
    assert x.shape == (2, 2 * stride + chunk, 2)
    bw = 6.0
    offs = list(range(0, x.shape[1] - (chunk - stride), stride))
    assert len(offs) == 3
    xs = torch.cat([normalised(CFG48, x[:, o:o + chunk], m[:, o:o + chunk]) for o in offs])   # [chunks * B, chunk, 2], chunk-major
    er = ref.encoder(xs)
    emb = eng._encoder(xs)                                         # one batch of 6
    looped = torch.cat([eng._encoder(xs[i:i + 1]) for i in range(xs.shape[0])])
    torch.cuda.synchronize()
    e, eb = rel_peak(emb, er), rel_peak(emb, looped.cpu())
    print(f"48 kHz encoder, 2 x 3 chunks batched: {e:.2e} of the peak vs the helper, {eb:.2e} vs the same engine sample by sample")
    assert e < 2e-3 and eb < 2e-3, (e, eb)
    wc, wm = ref.quantizer_encode(er, bw, return_margins=True)
    forced = [0, 0]
    resync(eng, emb, bw, wc, wm, 2e-3 * float(er.abs().max()) * 3.0, "48 kHz 2 x 3 chunks", forced)
    assert forced[0] <= 0.05 * forced[1], forced
    codes, scales = eng.encode(x, m, bandwidth=bw)
    wcodes, wscales = ref.encode(x, m, bandwidth=bw)
    torch.cuda.synchronize()
    assert codes.shape == wcodes.shape == (3, 2, 4, 150) and len(scales) == 3 and scales[0].shape == (2, 1, 1)
    assert rel_peak(torch.stack(scales), torch.stack(wscales)) < 1e-5
    got = eng.decode(wcodes, wscales, m)
    want = ref.decode(wcodes, wscales, m)
    frames = [eng._decode_frame(wcodes[ci, b:b + 1], wscales[ci][b:b + 1]) for ci in range(3) for b in range(2)]   # chunk by chunk, sample by sample
    single = eng._linear_overlap_add([torch.cat(frames[2 * ci:2 * ci + 2]) for ci in range(3)], stride)[:, :m.shape[1]]
    torch.cuda.synchronize()
    got, single = got.cpu(), single.cpu()
    err, peak = float((got - want).abs().max()), float(want.abs().max())
    errb = float((got - single).abs().max())
    print(f"48 kHz decode, 2 x 3 chunks batched: max-abs {err:.2e} (peak {peak:.2f}), SNR {snr_db(got, want):.1f} dB; vs chunk by chunk {errb:.2e}, {snr_db(got, single):.1f} dB")
    assert got.shape == want.shape == (2, 2 * stride + chunk, 2) and err <= 2e-3 * peak and snr_db(got, want) >= 50.0
    assert errb <= 2e-3 * peak and snr_db(got, single) >= 50.0


def test_gn_zero_padding_materialises():
    """``pad_mode = "constant"`` (mono, causal): a padded 0 must stay 0 -- the norm cannot ride in the consumer's prologue.  Against the helper (the
    reference itself cannot run this pad mode, see tests/golden/make_encodec_gn_fixtures.py)."""
    from _encodec_gn_ref import EncodecGNRef
    from mlx_audio_amd.codec.models.encodec import Encodec

    c = dict(audio_channels=1, num_filters=8, kernel_size=7, num_residual_layers=1, dilation_growth_rate=2, codebook_size=64, codebook_dim=32, hidden_size=32,
             num_lstm_layers=2, residual_kernel_size=3, use_causal_conv=True, normalize=False, pad_mode="constant", norm_type="time_group_norm",
             last_kernel_size=7, trim_right_ratio=1.0, compress=2, upsampling_ratios=[4, 2, 2], target_bandwidths=[15.0, 60.0], sampling_rate=24000,
             use_conv_shortcut=False)
    w = weights_of(c, 41)
    eng, ref = Encodec(c, weights=w, device=DEV), EncodecGNRef(w, c)
    g = torch.Generator().manual_seed(3)
    x = 0.3 * torch.randn(2, 16 * 61, 1, generator=g)
    er, est = ref.encoder(x, return_stages=True)
    emb, gst = eng._encoder(x, return_stages=True)
    torch.cuda.synchronize()
    errs = {k: rel_peak(gst[k], est[k]) for k in est}
    print("time_group_norm, zero padding, no conv shortcut: encoder stages", {k: f"{v:.1e}" for k, v in errs.items()})
    assert max(errs.values()) < 2e-3, errs
    z = torch.randn(2, 20, 32, generator=g)
    want, dst = ref.decoder(z, return_stages=True)
    got, dgs = eng._decoder(z.to(DEV), return_stages=True)
    torch.cuda.synchronize()
    errs = {k: rel_peak(dgs[k], dst[k]) for k in dst}
    errs["out"] = rel_peak(got, want)
    print("decoder stages", {k: f"{v:.1e}" for k, v in errs.items()})
    assert max(errs.values()) < 2e-3 and snr_db(got, want) >= 50.0, errs


def test_gn_from_pretrained_strict_and_weight_norm_untouched(tmp_path):
    from safetensors.torch import save_file

    from mlx_audio_amd.codec.models.encodec import Encodec

    fx = np.load(os.path.join(GOLD, "ref_encodec_gn_stereo.npz"))
    c = json.loads(str(fx["config"]))
    w = weights_of(c, int(fx["seed_w"]))
    save_file({k: v.contiguous() for k, v in w.items()}, str(tmp_path / "model.safetensors"))
    (tmp_path / "config.json").write_text(json.dumps(dict(c, architectures=["EncodecModel"], some_unknown_field=1)))
    model, processor = Encodec.from_pretrained(str(tmp_path), device=DEV)
    assert model.gn and model.chunk_length == 1200
    x, m = processor(torch.from_numpy(fx["raw"]))
    assert torch.equal(x, torch.from_numpy(fx["inputs"])) and torch.equal(m, torch.from_numpy(fx["masks"]))
    bw = c["target_bandwidths"][0]
    codes, scales = model.encode(x, m, bandwidth=bw)
    direct = Encodec(c, weights=w, device=DEV)
    codes2, scales2 = direct.encode(x, m, bandwidth=bw)
    audio = model.decode(codes, scales, m)
    torch.cuda.synchronize()
    assert torch.equal(codes, codes2) and all(torch.equal(a, b) for a, b in zip(scales, scales2))
    assert audio.shape == (1, x.shape[1], 2) and torch.isfinite(audio).all()
    # strict loading reports a missing norm parameter
    w2 = {k: v for k, v in w.items() if k != "decoder.layers.3.norm.bias"}
    with pytest.raises(KeyError, match="decoder.layers.3.norm.bias"):
        Encodec(c, weights=w2, device=DEV)
    with pytest.raises(ValueError, match="norm_type"):
        Encodec(dict(c, norm_type="layer_norm"), weights=w, device=DEV)
    # a weight_norm model still constructs and decodes (its parity lives in tests/test_encodec_gpu.py)
    cw = dict(c, norm_type="weight_norm")
    ww = weights_of(cw, 3)
    assert not any(".norm." in k for k in ww)
    ew = Encodec(cw, weights=ww, device=DEV)
    assert not ew.gn
    out = ew.decode(codes, scales, m)
    torch.cuda.synchronize()
    assert out.shape == audio.shape and torch.isfinite(out).all()
