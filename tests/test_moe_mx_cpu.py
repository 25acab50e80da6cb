"""Loading a `-mxfp4` / `-nvfp4` / `-mxfp8` Ling / Ming checkpoint, the parts that need no device: ``lm.moe.sanitize`` stacks the per-expert ``weight`` / uint8
``scales``, the mode comes from the shapes and must agree with the config's, and ``.scales`` of any other dtype without ``.biases`` keeps its refusal."""
import pytest
import torch

import _bailing_moe_ref as R
from mlx_audio_amd.lm import moe

BASE = dict(R.CONFIGS["A"], num_shared_experts=0)   # 4 experts, one dense layer in front
P = "model.layers.1.mlp"
SHAPES = {"mxfp4": (16, 4), "nvfp4": (16, 8), "mxfp8": (32, 4)}   # packed words and scale bytes of a row of K = 128
_args = lambda quantization=None: moe.ModelArgs.from_dict(dict(BASE, quantization=quantization))


def _experts(mode, scale_dtype=torch.uint8):
    return {f"{P}.experts.{e}.{m}.{k}": torch.full((64, n), v + e).to(dt) for e in range(4) for m in ("gate_proj", "up_proj", "down_proj")
            for k, n, v, dt in (("weight", SHAPES[mode][0], 0, torch.int32), ("scales", SHAPES[mode][1], 120, scale_dtype))}


@pytest.mark.parametrize("mode", sorted(SHAPES))
@pytest.mark.parametrize("named", [False, True], ids=["shapes", "config"])
def test_sanitize_stacks_uint8_scales(mode, named):
    w = moe.sanitize(_experts(mode), _args({"mode": mode, "group_size": 32, "bits": 4} if named else None))
    for m in ("gate_proj", "up_proj", "down_proj"):
        q, s = w[f"{P}.switch_mlp.{m}.weight"], w[f"{P}.switch_mlp.{m}.scales"]
        assert q.shape == (4, 64, SHAPES[mode][0]) and s.shape == (4, 64, SHAPES[mode][1]) and s.dtype == torch.uint8 and q[3, 0, 0] == 3 and s[2, 5, 1] == 122
    assert not any(".experts." in k or k.endswith(".biases") for k in w)


def test_the_mode_comes_from_the_shapes_and_must_agree_with_the_config():
    up, res = f"{P}.switch_mlp.up_proj", moe.resolve_quantization_mx
    assert all(res(None, up, *wg) == m and res({"mode": m}, up, *wg) == m for m, wg in SHAPES.items())
    q = {"mode": "mxfp4", "group_size": 32, "bits": 4, up: {"mode": "mxfp8"}, "lm_head": {"group_size": 64, "bits": 8}}
    assert res(q, up, 32, 4) == "mxfp8" and res(q, "lm_head", 16, 4) == "mxfp4"   # a per-path mode; an entry without one leaves it to the shapes
    assert moe.resolve_quantization(q, "lm_head", 32, 2) == moe.resolve_quantization(q, f"{P}.gate.gate_proj", 32, 2) == (8, 64)   # affine ones beside them
    for quantization in ({"mode": "nvfp4"}, {"mode": "mxfp8", f"{P}.switch_mlp.gate_proj": {"mode": "affine"}}):   # a contradiction, global or per path
        with pytest.raises(ValueError, match=rf"{P}.switch_mlp.gate_proj: quantization mode '(nvfp4|affine)' contradicts the shapes.*uint8 scales is mxfp4"):
            moe.sanitize(_experts("mxfp4"), _args(quantization))


def test_other_scales_without_biases_keep_their_refusal():
    with pytest.raises(NotImplementedError, match=r"quantised experts \(QuantizedSwitchLinear\) in a non-affine mode are not built .*scales has no .biases"):
        moe.sanitize(_experts("mxfp4", torch.float16), _args())
