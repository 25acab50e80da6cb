"""Mimi codec decode on the HIP path vs the CPU oracle; shape pin of the reference's own test
(codec/tests/test_mimi.py:11-21: codes (1, 32, 63) -> audio (1, 1, 120960)).  Needs a real MI355X: ``pytest -m gpu``."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def rel_peak(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def snr_db(got, ref):
    got, ref = got.double().cpu(), ref.double().cpu()
    return float(10 * torch.log10(ref.pow(2).sum() / ((got - ref).pow(2).sum() + 1e-30)))


def _pair(cfg, seed):
    from mlx_audio_amd.codec.models.mimi import mimi as M
    from oracle.mimi_ref import MimiConfig as RC
    from oracle.mimi_ref import MimiDecoderRef

    w = M.make_mimi_decoder_weights(cfg, seed=seed)
    rcfg = RC(**{k: getattr(cfg, k) for k in RC.__dataclass_fields__})
    return M.MimiDecoder(w, cfg, device=DEV), MimiDecoderRef(w, rcfg), M


def test_tiny_stages_waveform_and_causality():
    from mlx_audio_amd.codec.models.mimi.mimi import tiny_mimi_config

    cfg = tiny_mimi_config()
    eng, ref, M = _pair(cfg, 1)
    codes = M.make_codes(2, 45, cfg, seed=2)   # 90 transformer positions > context 20: the window mask is exercised
    exp, est = ref(codes, return_stages=True)
    got, gst = eng(codes, return_stages=True)
    torch.cuda.synchronize()
    for k in est:
        assert rel_peak(gst[k], est[k]) < 3e-4, (k, rel_peak(gst[k], est[k]))
    peak = float(exp.abs().max())
    assert float((got.cpu() - exp).abs().max()) <= 2e-3 * peak and snr_db(got, exp) >= 50.0
    # streaming equivalence (decode_step per frame == decode, conv.py:245-331): causal => a prefix decodes to the same samples
    part = eng(codes[..., :20])
    torch.cuda.synchronize()
    n = 20 * eng.total_upsample
    assert float((got[..., :n] - part).abs().max()) <= 1e-4 * peak


def test_codes_past_the_codebook_add_nothing():
    """A CSM head is three columns wider than the Mimi codebooks (audio_vocab_size 2051 / 2048 bins; 67 / 64 in the tiny configs) and may emit a code
    with no entry.  Such a code is masked, not looked up (the table ends there): with entry 5 of every codebook set to zero, codes >= bins decode bit
    for bit like code 5, through the one-shot and the streaming decoder."""
    from mlx_audio_amd.codec.models.mimi.mimi import tiny_mimi_config

    cfg = tiny_mimi_config()
    eng, _, M = _pair(cfg, 1)
    bins = cfg.quantizer_bins
    for table, _, _, n in eng.rvq:
        for i in range(n):
            table[i * bins + 5].zero_()
    codes = M.make_codes(2, 9, cfg, seed=3)
    inside = codes.clone()
    for b, q, t, past in ((0, 0, 2, 0), (1, cfg.quantizer_nq - 1, 5, 2), (0, cfg.quantizer_nq - 1, 8, 1), (1, 1, 0, 1)):
        codes[b, q, t], inside[b, q, t] = bins + past, 5
    got, want = eng(codes), eng(inside)
    st = eng.new_stream(2)
    step = torch.cat([eng.decode_step(codes[..., t:t + 3], st) for t in range(0, 9, 3)], dim=-1)
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    assert float((step - want).abs().max()) <= 1e-4 * float(want.abs().max())


def test_mimi_202407_reference_shape_pin_and_values():
    from mlx_audio_amd.codec.models.mimi.mimi import mimi_202407

    cfg = mimi_202407(32)
    eng, ref, M = _pair(cfg, 0)
    assert eng.total_upsample == 1920
    codes = M.make_codes(1, 63, cfg, seed=1)
    got, gst = eng(codes, return_stages=True)
    torch.cuda.synchronize()
    assert tuple(got.shape) == (1, 1, 120960)            # codec/tests/test_mimi.py:11-21
    exp, est = ref(codes, return_stages=True)
    for k in est:
        assert rel_peak(gst[k], est[k]) < 3e-4, (k, rel_peak(gst[k], est[k]))
    peak = float(exp.abs().max())
    assert float((got.cpu() - exp).abs().max()) <= 2e-3 * peak and snr_db(got, exp) >= 50.0


def test_mimi_202407_encode_shape_pin_and_stages():
    """ENCODE at the real sizes: the reference's own shape pin (codec/tests/test_mimi.py:13-18: 120 000 samples -> codes (1, 32, 63) -> audio
    (1, 1, 120 960)) and, on a 1.2 s clip, every stage in front of the quantiser against the oracle (3e-4 of the stage's peak) + the codes under the
    margin rule (2048-entry codebooks: near ties exist)."""
    import _margin
    from mlx_audio_amd.codec.models.mimi import mimi as M
    from oracle.mimi_ref import MimiConfig as RC
    from oracle.mimi_ref import MimiEncoderRef

    cfg = M.mimi_202407(32)
    w = {**M.make_mimi_decoder_weights(cfg, seed=0), **M.make_mimi_encoder_weights(cfg, seed=0)}
    # float32 codebook statistics that are NOT bf16 values (real checkpoints: kyutai Mimi, the Qwen3 speech tokenizer): the encoder must build its
    # tables from the checkpoint values -- rounding them to bf16 first moves codewords by 2^-9 and flips arg-min decisions (round-3 advisor finding)
    gq = torch.Generator().manual_seed(99)
    for k in list(w):
        if ".codebook.embedding_sum" in k and k.startswith("quantizer."):
            w[k] = (w[k].float() * (1.0 + 3e-3 * torch.randn(w[k].shape, generator=gq))).float()
    assert any((w[k].float() != w[k].to(torch.bfloat16).float()).any() for k in w if ".codebook.embedding_sum" in k and k.startswith("quantizer."))
    both = M.Mimi(w, cfg, device=DEV)
    codes = both.encode(torch.zeros(1, 1, 120_000))
    torch.cuda.synchronize()
    assert tuple(codes.shape) == (1, 32, 63) and codes.dtype == torch.int64
    assert tuple(both.decode(codes).shape) == (1, 1, 120_960)
    pcm = M.make_pcm(2, 28_800 + 333, seed=3)
    ref = MimiEncoderRef(w, RC(**{k: getattr(cfg, k) for k in RC.__dataclass_fields__}))
    zr, est = ref.latent(pcm, return_stages=True)
    z, gst = both.encoder.latent(pcm, return_stages=True)
    torch.cuda.synchronize()
    for k in est:
        assert rel_peak(gst[k], est[k]) < 3e-4, (k, rel_peak(gst[k], est[k]))
    want, wm = ref.quantize(zr, return_margins=True)
    got, gm = both.encoder.quantize(z, return_margins=True)
    torch.cuda.synchronize()
    got, gm = got.cpu(), gm.cpu()
    thr = 2e-3 * float(zr.abs().max()) * 3.0   # a latent error of 3e-4 of peak moves a score by about |e| times that
    for b in range(got.shape[0]):
        for t in range(got.shape[2]):
            _margin.walk("mimi_encode", got[b, :1, t].tolist(), want[b, :1, t].tolist(), torch.minimum(gm, wm)[b, :1, t].tolist(), thr=thr, where=(b, t, 0))
            _margin.walk("mimi_encode", got[b, 1:, t].tolist(), want[b, 1:, t].tolist(), torch.minimum(gm, wm)[b, 1:, t].tolist(), thr=thr, where=(b, t))


@pytest.mark.parametrize("full", [False, True])
def test_streaming_decode_equals_one_shot(full):
    """``decode_step`` with carried state (mimi.py:171-176, modules/conv.py:245-331): the concatenation of the chunks' audio is the one-shot decode of
    the concatenated codes -- every stage, chunk sizes 1 .. 7, more transformer positions than the attention window (tiny config: context 20)."""
    from mlx_audio_amd.codec.models.mimi import mimi as M

    cfg = M.mimi_202407(32) if full else M.tiny_mimi_config()
    eng, _, _ = _pair(cfg, 3)
    n = 23 if full else 41
    codes = M.make_codes(2, n, cfg, seed=5)
    want, wst = eng(codes, return_stages=True)
    st = eng.new_stream(2)
    pieces, stages, pos = [], {}, 0
    for size in [1, 4, 3, 7, 2, 1, 5, 100]:
        if pos >= n:
            break
        a, g = eng.decode_step(codes[:, :, pos:pos + size], st, return_stages=True)
        assert a.shape[-1] == min(size, n - pos) * (want.shape[-1] // n)
        pieces.append(a)
        for k, v in g.items():
            stages.setdefault(k, []).append(v)
        pos += size
    torch.cuda.synchronize()
    assert st.frames == n
    for k, v in stages.items():
        assert rel_peak(torch.cat(v, 1), wst[k]) < 2e-5, (k, rel_peak(torch.cat(v, 1), wst[k]))
    got = torch.cat(pieces, -1)
    assert got.shape == want.shape
    # Not bit-equal, by construction of the library and not of the streaming state: conv_gemm / attention pick their kernel by launch size (a chunk of
    # a few rows takes the 4-wave or split-K kernels, the one-shot pass the wave-specialised one), and those sum in a different order -- the same
    # float32-rounding-level differences tests/test_kokoro_gpu.py::test_kokoro_batch_equals_single bounds at 5e-5.  Measured: 3-6e-6 of the peak.
    print(f"mimi streaming vs one-shot ({'202407' if full else 'tiny'}): {rel_peak(got, want):.2e} of the peak")
    assert rel_peak(got, want) < 2e-5, rel_peak(got, want)
    # the reference's wrapper (MimiStreamingDecoder.decode_frames) over the same state machine
    both = M.Mimi({**M.make_mimi_decoder_weights(cfg, seed=3)}, cfg, device=DEV)
    sd = M.MimiStreamingDecoder(both)
    a1, a2 = sd.decode_frames(codes[:, :, :9]), sd.decode_frames(codes[:, :, 9:])
    torch.cuda.synchronize()
    assert rel_peak(torch.cat([a1, a2], -1), want) < 2e-5
    sd.reset()
    assert rel_peak(sd.decode_frames(codes[0, :, :6]), want[:1, :, : 6 * (want.shape[-1] // n)]) < 2e-5   # [C, T] input, fresh state
