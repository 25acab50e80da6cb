"""Bailing MoE on the host: the float64 restatement ``tests/_bailing_moe_ref.py`` held to the reference's own stored runs
(``tests/golden/ref_bailing_moe.npz``, made by ``tests/golden/make_bailing_moe_fixtures.py`` from the unmodified ``bailing_moe.py`` /
``switch_layers.py``), and config / ``sanitize`` / refusal behaviour by name."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _bailing_moe_ref as R  # noqa: E402
import _margin  # noqa: E402


@pytest.mark.parametrize("name", sorted(R.CONFIGS))
def test_restatement_against_the_reference_runs(name):
    ref = np.load(R.GOLDEN)
    args, w, ids = R.setup(name)
    assert np.array_equal(ref[f"{name}.ids"], ids.numpy())
    got = R.forward(args, w, ids)
    i = args.first_k_dense_replace
    sure = ref[f"{name}.router{i}.gap"] >= _margin.THR
    assert sure.sum() >= 12, int(sure.sum())
    assert np.array_equal(got[f"router{i}.ids"].numpy()[sure], ref[f"{name}.router{i}.ids"][sure])
    for k in ("layer0", "layer1", "logits", f"router{i}.wsum"):
        want = ref[f"{name}.{k}"].astype(np.float64)
        rows = sure if k != "layer0" else slice(None)
        err = np.abs(got[k].numpy() - want)[rows].max() / np.abs(want).max()
        assert err <= 2e-5, (k, err)


def test_config_sanitize_and_refusals():
    from mlx_audio_amd.lm import moe

    base = R.CONFIGS["A"]
    a = moe.ModelArgs.from_dict(dict(base, unknown_field=1))
    assert (a.score_function, a.n_group, a.topk_group, a.routed_scaling_factor, a.use_bias, a.partial_rotary_factor) == ("softmax", 1, 4, 1.0, False, 1.0)
    with pytest.raises(NotImplementedError, match="rope_scaling"):
        moe.ModelArgs.from_dict(dict(base, rope_scaling={"type": "yarn", "factor": 2.0}))
    with pytest.raises(NotImplementedError, match="head width 32"):
        moe.ModelArgs.from_dict(dict(base, num_attention_heads=4))
    with pytest.raises(NotImplementedError, match="hub download"):
        moe.from_pretrained("inclusionAI/Ling-lite")
    p = "model.layers.1.mlp"
    ck = {f"{p}.experts.{e}.{m}.weight": torch.full((2, 3), float(e)) for e in range(4) for m in ("gate_proj", "up_proj", "down_proj")}
    ck.update({f"{p}.gate.weight": torch.zeros(4, 3), "lm_head.weight": torch.ones(5, 3), "model.layers.0.mlp.gate_proj.weight": torch.zeros(2, 3)})
    w = moe.sanitize(ck, a)
    assert w[f"{p}.switch_mlp.up_proj.weight"].shape == (4, 2, 3) and w[f"{p}.switch_mlp.up_proj.weight"][3, 0, 0] == 3.0
    assert f"{p}.gate.gate_proj.weight" in w and f"{p}.gate.weight" not in w and not any(".experts." in k for k in w)
    assert "lm_head.weight" in w and "lm_head.weight" not in moe.sanitize(ck, moe.ModelArgs.from_dict(dict(base, tie_word_embeddings=True)))
    with pytest.raises(NotImplementedError, match="QuantizedSwitchLinear"):
        moe.sanitize(dict(ck, **{f"{p}.switch_mlp.gate_proj.scales": torch.zeros(1)}), a)
