"""A quantised (MLX `-4bit` / `-8bit`) Whisper checkpoint loaded through ``Model.load_weights`` against the float engine on the same dequantised
weights.  The checkpoint is made fp16-exact so that the float engine is a fair reference: per group of 64 the scale is a power of two >=
2 max|w| / (2^bits - 1) (hence >= range / (2^bits - 1)), zero = -2^(bits - 1) scale, codes by rounding; scale * q + zero is then a small integer
times a power of two.  Without the feature the load fails with "missing parameter".

Measured on MI355X (largest logit difference / peak over the prompt and the three steps; bar 3e-4): see docs/COVERAGE.md row x2."""
import pytest
import torch

from _margin import THR
from mlx_audio_amd import ops
from mlx_audio_amd.stt.models.whisper.engine import WhisperEngine
from mlx_audio_amd.stt.models.whisper.synthetic import make_mel, make_whisper_weights, tiny_dims
from mlx_audio_amd.stt.models.whisper.whisper import Model

pytestmark = pytest.mark.gpu
G = 64
BAR = 3e-4   # of the peak: the project's standing stage bar


def _quantize(w, bits):
    g = w.reshape(w.shape[0], -1, G)
    scale = torch.pow(2.0, torch.ceil(torch.log2(2 * g.abs().amax(-1).clamp_min(2.0 ** -14) / ((1 << bits) - 1))))
    zero = -(1 << (bits - 1)) * scale
    codes = torch.round((g - zero[..., None]) / scale[..., None]).clamp_(0, (1 << bits) - 1).to(torch.int64)
    deq = (scale[..., None] * codes + zero[..., None]).reshape(w.shape)
    assert torch.equal(deq.half().float(), deq)
    return ops.pack_codes(codes.reshape(w.shape), bits), scale.half(), zero.half(), deq


@pytest.mark.parametrize("bits,parts", [(4, ("encoder.", "decoder.")), (8, ("encoder.", "decoder.")), (4, ("decoder.",))], ids=["4bit", "8bit", "4bit-decoder-only"])
def test_quantized_checkpoint_matches_the_float_engine_on_its_dequantisation(bits, parts):
    dims = tiny_dims()
    fw = make_whisper_weights(dims, seed=3)
    qw = {}
    for k, v in list(fw.items()):
        if v.dim() == 2 and k.endswith(".weight") and k.startswith(parts) and not k.endswith("_ln.weight"):
            wq, s, z, fw[k] = _quantize(v, bits)
            qw.update({k: wq, k[:-7] + ".scales": s, k[:-7] + ".biases": z})
        else:
            qw[k] = v.half()
    model = Model(dims)
    A = model.load_weights(model.sanitize(qw)).engine
    Bf = WhisperEngine(fw, dims)
    assert A.quantized_decoder and not A.native_decode and A.tok_emb is None and A.dec_blocks[0].qkv.ql.bits == bits and A.enc_blocks[0].qkv.ql is None
    worst, steps, clear = 0.0, 0, 0
    for B in (1, 9):
        mel = make_mel(B, seed=B, n_frames=2 * dims.n_audio_ctx)
        xa, xb = A.encode(mel), Bf.encode(mel)
        assert float((xa - xb).abs().max()) <= 1e-5 * float(xb.abs().max())   # the same fp16 images: bit-equal unless conv_gemm picks another tile
        sa, sb = A.new_state(xa), Bf.new_state(xb)
        tok = torch.randint(0, dims.n_vocab, (B, 4), generator=torch.Generator().manual_seed(B)).to(torch.int32).to(A.device)
        for _ in range(4):   # the 4-token prompt, then three one-token steps on the float engine's greedy token
            la = A.logits(A.decoder_step(tok, sa))[:, -1, :dims.n_vocab]
            lb = Bf.logits(Bf.decoder_step(tok, sb))[:, -1, :dims.n_vocab]
            d = float((la - lb).abs().max()) / float(lb.abs().max())
            worst = max(worst, d)
            print(f"whisper {bits}-bit {parts} B={B} rows={tok.numel()}: logits differ by {d:.3e} of the peak")
            assert d <= BAR
            top = lb.topk(2, dim=-1)
            sure = (top.values[:, 0] - top.values[:, 1]) >= THR
            assert torch.equal(la.argmax(-1)[sure], top.indices[:, 0][sure])
            steps, clear = steps + B, clear + int(sure.sum())
            tok = top.indices[:, :1].to(torch.int32).contiguous()
    assert clear >= 0.9 * steps, (clear, steps)
