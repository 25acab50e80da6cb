"""Loading a quantised Ling / Ming checkpoint, the parts that need no device: ``lm.moe.sanitize`` stacks the per-expert ``weight`` / ``scales`` /
``biases``, what is still not built is refused by name, and bits / group size come from the config's ``quantization`` or from the shapes."""
import pytest
import torch

import _bailing_moe_ref as R
from mlx_audio_amd.lm import moe

BASE = dict(R.CONFIGS["A"], num_shared_experts=0)   # 4 experts, one dense layer in front
P = "model.layers.1.mlp"


def _experts(words=16, groups=2, dtype=torch.int32, biases=True):
    """Per-expert gate / up / down tensors over K = 128: ``words`` packed words and ``groups`` scales a row (16 and 2: 4 bits, group 64)."""
    ck = {}
    for e in range(4):
        for m in ("gate_proj", "up_proj", "down_proj"):
            ck[f"{P}.experts.{e}.{m}.weight"] = torch.full((64, words), e).to(dtype)
            ck[f"{P}.experts.{e}.{m}.scales"] = torch.full((64, groups), float(e)).half()
            if biases:
                ck[f"{P}.experts.{e}.{m}.biases"] = torch.full((64, groups), -float(e)).half()
    return ck


def test_sanitize_stacks_weight_scales_and_biases():
    a = moe.ModelArgs.from_dict(BASE)
    w = moe.sanitize(dict(_experts(), **{f"{P}.gate.{k}": torch.zeros(4, 2) for k in ("weight", "scales", "biases")}), a)
    assert not any(".experts." in k for k in w) and f"{P}.gate.gate_proj.scales" in w and f"{P}.gate.scales" not in w
    for m in ("gate_proj", "up_proj", "down_proj"):
        q, s, b = (w[f"{P}.switch_mlp.{m}.{k}"] for k in ("weight", "scales", "biases"))
        assert q.shape == (4, 64, 16) and q.dtype == torch.int32 and s.shape == b.shape == (4, 64, 2) and s.dtype == torch.float16
        assert q[3, 0, 0] == 3 and s[2, 5, 1] == 2.0 and b[1, 0, 0] == -1.0


@pytest.mark.parametrize("ck,quantization,text", [
    (_experts(biases=False), None, "non-affine mode"),
    (_experts(dtype=torch.float32), None, "packed uint32 codes"),
    (_experts(words=12), {"group_size": 64, "bits": 3}, "bits = 3"),
    (_experts(words=16, groups=8), {"group_size": 16, "bits": 4}, "group_size = 16"),
], ids=["scales-without-biases", "float-weight", "bits-3", "group-16"])
def test_what_is_not_built_is_refused_by_name(ck, quantization, text):
    a = moe.ModelArgs.from_dict(dict(BASE, quantization=quantization))
    with pytest.raises(NotImplementedError, match=rf"quantised experts \(QuantizedSwitchLinear\).*{text}"):
        moe.sanitize(ck, a)


def test_bits_and_group_come_from_the_config_or_the_shapes():
    gate, res = "model.layers.1.mlp.gate.gate_proj", moe.resolve_quantization
    q = {"group_size": 64, "bits": 4, gate: {"group_size": 64, "bits": 8}}
    assert res(q, gate, 32, 2) == (8, 64) and res(q, "model.layers.1.mlp.switch_mlp.up_proj", 16, 2) == (4, 64)   # the router's per-path override
    assert res({"group_size": 32, "bits": 8}, "lm_head", 32, 4) == (8, 32) and res(None, "lm_head", 32, 4) == (4, 64)   # same shapes: MLX's default group
    assert res(None, "lm_head", 32, 2) == (8, 64) and res(None, "lm_head", 16, 4) == (4, 32)
    assert moe.ModelArgs.from_dict(dict(BASE, quantization_config=q)).quantization == q
    with pytest.raises(ValueError, match="do not match"):
        res({"group_size": 64, "bits": 8}, "lm_head", 16, 2)
