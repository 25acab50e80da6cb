"""`-mxfp4` / `-mxfp8` / `-nvfp4` Whisper checkpoints made with ``ops.quantize_mx`` and loaded through ``Model.load_weights``, against the float engine
on the same dequantised weights (fp16-exact for these weights, asserted).  Without the feature the load fails with "missing parameter".

Measured on MI355X (largest logit difference / peak over the prompt and the three steps; bar 3e-4): see docs/COVERAGE.md row x3."""
import pytest
import torch

from mlx_audio_amd import ops
from mlx_audio_amd.stt.models.whisper.engine import WhisperEngine
from mlx_audio_amd.stt.models.whisper.synthetic import make_mel, make_whisper_weights, tiny_dims
from mlx_audio_amd.stt.models.whisper.whisper import Model

pytestmark = pytest.mark.gpu
BAR = 3e-4   # of the peak: the project's standing stage bar


@pytest.mark.parametrize("mode", tuple(ops.QMODES))
def test_mx_checkpoint_matches_the_float_engine_on_its_dequantisation(mode):
    _, bits, g = ops.QMODES[mode]
    dims = tiny_dims()
    fw = make_whisper_weights(dims, seed=3)
    qw = {}
    for k, v in list(fw.items()):
        if v.dim() == 2 and k.endswith(".weight") and not k.endswith("_ln.weight"):
            wq, s = ops.quantize_mx(v, mode)
            fw[k] = ops.mx_code_values(ops.unpack_codes(wq, bits), mode) * ops.mx_scale_values(s, mode).repeat_interleave(g, 1)
            assert torch.equal(fw[k].half().float(), fw[k])
            qw.update({k: wq, k[:-7] + ".scales": s})
        else:
            qw[k] = v.half()
    model = Model(dims)
    A = model.load_weights(model.sanitize(qw), quantization={"mode": mode, "group_size": g, "bits": bits}).engine
    Bf = WhisperEngine(fw, dims)
    assert A.quantized_decoder and not A.native_decode and A.tok_emb is None and A.dec_blocks[0].qkv.ql.mode == mode and A.enc_blocks[0].qkv.ql is None
    for wrong in ("mxfp8" if mode != "mxfp8" else "mxfp4", "affine"):
        with pytest.raises(ValueError, match="contradicts the shapes"):
            model.load_weights(model.sanitize(qw), quantization={"mode": wrong})
    steps, clear = 0, 0
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
            print(f"whisper {mode} B={B} rows={tok.numel()}: logits differ by {d:.3e} of the peak")
            assert d <= BAR
            top = lb.topk(2, dim=-1)
            sure = (top.values[:, 0] - top.values[:, 1]) >= 1e-3
            assert torch.equal(la.argmax(-1)[sure], top.indices[:, 0][sure])
            steps, clear = steps + B, clear + int(sure.sum())
            tok = top.indices[:, :1].to(torch.int32).contiguous()
    assert clear >= 0.9 * steps, (clear, steps)


def test_a_checkpoint_directory_is_held_to_its_config_mode(tmp_path):
    """The directory loader hands the config's ``quantization`` to ``load_weights``: the right mode loads, a wrong one is refused by name, and so is a
    non-affine mode beside affine parameters."""
    import dataclasses
    import json

    from safetensors.torch import save_file

    from mlx_audio_amd.stt.utils import load_model

    dims = tiny_dims()
    fw = make_whisper_weights(dims, seed=3)
    k = "decoder.blocks.0.mlp1.weight"
    wq, s = ops.quantize_mx(fw[k], "nvfp4")
    aq, asc, ab = ops.quantize_affine(fw[k].half(), 64, 4)
    mx = {**{n: v.half() for n, v in fw.items() if n != k}, k: wq, k[:-7] + ".scales": s}
    affine = {**mx, k: aq, k[:-7] + ".scales": asc, k[:-7] + ".biases": ab}
    for weights, mode, refused in ((mx, "nvfp4", False), (mx, "mxfp4", True), (mx, "affine", True), (affine, "affine", False), (affine, "mxfp4", True)):
        d = tmp_path / f"{len(weights)}-{mode}"
        d.mkdir()
        save_file({n: v.contiguous() for n, v in weights.items()}, str(d / "model.safetensors"))
        (d / "config.json").write_text(json.dumps({"model_type": "whisper", **dataclasses.asdict(dims), "quantization": {"mode": mode, "group_size": 64, "bits": 4}}))
        if refused:
            with pytest.raises(ValueError, match="contradicts the shapes"):
                load_model(d)
        else:
            assert load_model(d).engine.dec_blocks[0].mlp1.ql is not None
