"""``lm.lfm2`` without a device: config arithmetic, ``sanitize``, cache kinds, refusals by name, ``ops.shortconv_route`` on made-up addresses, and
the float64 restatement ``tests/_lfm2_ref.py`` against the reference's own stored runs (2e-5 of the peak: the project's CPU bar)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _lfm2_ref as R  # noqa: E402

from mlx_audio_amd import _lib, ops  # noqa: E402
from mlx_audio_amd.lm import lfm2  # noqa: E402
from mlx_audio_amd.lm.cache import ConvState  # noqa: E402
from mlx_audio_amd.lm.stack import KVCache  # noqa: E402


def test_config_arithmetic():
    a, b = (lfm2.ModelArgs.from_dict(R.CONFIGS[n]) for n in "AB")
    assert a.full_attn_idxs == [2] and a.rope_theta == 1000000.0 and a.ff_dim == 192       # 256 -> int(512 / 3) = 170 -> up to 64s
    assert b.full_attn_idxs == [0] and b.rope_theta == 10000.0 and b.ff_dim == 320         # rope_parameters overrides; no adjustment
    big = lfm2.ModelArgs.from_dict(dict(R.CONFIGS["A"], hidden_size=2048, num_attention_heads=32, block_ff_dim=12288, block_multiple_of=256))
    assert big.ff_dim == 8192 and lfm2.ModelArgs.from_dict(dict(R.CONFIGS["A"], block_ff_dim=12288, block_ffn_dim_multiplier=1.3)).ff_dim == 10688
    assert lfm2.ModelArgs.from_dict(dict(R.CONFIGS["A"], num_key_value_heads=None)).num_key_value_heads == 2


def test_sanitize_turns_a_torch_conv_weight():
    w = {"model.layers.0.conv.conv.weight": torch.arange(24.0).reshape(8, 1, 3), "model.layers.0.conv.in_proj.weight": torch.zeros(24, 8)}
    s = lfm2.sanitize(w)
    assert s["model.layers.0.conv.conv.weight"].shape == (8, 3, 1) and torch.equal(s["model.layers.0.conv.conv.weight"][:, :, 0], w["model.layers.0.conv.conv.weight"][:, 0])
    assert torch.equal(lfm2.sanitize(s)["model.layers.0.conv.conv.weight"], s["model.layers.0.conv.conv.weight"]) and s["model.layers.0.conv.in_proj.weight"].shape == (24, 8)


def test_cache_kinds_follow_the_layer_types():
    a = lfm2.ModelArgs.from_dict(R.CONFIGS["A"])
    m = lfm2.Lfm2Model.__new__(lfm2.Lfm2Model)
    m.args, m.device = a, torch.device("cpu")
    m.layers = [(None, (lfm2.Attention if i in a.full_attn_idxs else lfm2.ShortConv).__new__(lfm2.Attention if i in a.full_attn_idxs else lfm2.ShortConv), None, None)
                for i in range(a.num_hidden_layers)]
    kinds = [type(c) for c in m.make_cache()]
    assert kinds == [ConvState, ConvState, KVCache, ConvState]
    st = ConvState(2, 8, "cpu")
    assert st.state is None and st.empty()
    first = st.next_state(3)
    st.swap(5)
    assert st.state is first and st.offset == 5 and st.next_state(3) is not first and st.next_state(3).shape == (3, 2, 8)


def test_refusals_by_name():
    with pytest.raises(NotImplementedError, match="hub download"):
        lfm2.from_pretrained("LiquidAI/LFM2-1.2B")
    with pytest.raises(NotImplementedError, match="lfm_audio"):
        lfm2.lfm_audio()
    with pytest.raises(NotImplementedError, match="head width 32"):
        lfm2.ModelArgs.from_dict(dict(R.CONFIGS["A"], num_attention_heads=4))
    with pytest.raises(NotImplementedError, match="quantised checkpoints"):
        lfm2._check_checkpoint({"model.layers.0.conv.in_proj.scales": torch.zeros(2)})
    with pytest.raises(NotImplementedError, match="16-bit checkpoints"):
        lfm2._check_checkpoint({"model.embed_tokens.weight": torch.zeros(2, dtype=torch.bfloat16)})


@pytest.mark.parametrize("B,T,H,L,want", [(1, 1, 1024, 3, (ops.SHORTCONV_STEP, 1, 128, 1, 1, 4096)), (8, 1, 2048, 3, (ops.SHORTCONV_STEP, 8, 256, 1, 1, 57344)),
                                          (2, 4, 128, 4, (ops.SHORTCONV_STEP, 8, 16, 1, 1, 4096)), (9, 1, 128, 3, (ops.SHORTCONV_TILE, 16, 4, 1, 9, 53376)),
                                          (1, 14, 128, 3, (ops.SHORTCONV_TILE, 16, 4, 1, 1, 53376)), (1, 15, 128, 3, (ops.SHORTCONV_TILE, 32, 4, 1, 1, 53376)),
                                          (4, 61, 2048, 4, (ops.SHORTCONV_TILE, 32, 64, 3, 4, 53376))])
def test_shortconv_route_on_made_up_addresses(B, T, H, L, want):
    r = ops.shortconv_route(B, T, H, L)
    assert (r["form"], r["rows"], r["grid_x"], r["grid_y"], r["grid_z"], r["lds_bytes"]) == want
    assert r["row_step"] == (B * T if r["form"] == ops.SHORTCONV_STEP else r["rows"] - (L - 1))


@pytest.mark.parametrize("over,text,rc", [(dict(L=1), "L = 1 is not built", -3), (dict(L=5), "L = 5 is not built", -3), (dict(H=48), "H = 48 is not a multiple of 32", -3),
                                          (dict(wdtype=ops.W_FP8), "quantised weights are not built", -3), (dict(state_in=0x50000000), "different buffers", -1),
                                          (dict(w_in=0x20000008), "16-byte aligned", -1), (dict(ldx=124), "shorter than H", -1), (dict(ldw=64), "at least H long", -1)])
def test_shortconv_route_refuses_by_name(over, text, rc):
    kw = dict(B=1, T=1, H=128, L=3)
    kw.update({k: over.pop(k) for k in list(over) if k in kw})
    with pytest.raises(_lib.Mi355Error, match=text) as e:
        ops.shortconv_route(kw["B"], kw["T"], kw["H"], kw["L"], **over)
    assert f"({rc})" in str(e.value)


@pytest.mark.parametrize("name", sorted(R.CONFIGS))
def test_float64_restatement_against_the_stored_reference_runs(name):
    args, w, ids = R.setup(name)
    ref = np.load(R.GOLDEN)
    assert np.array_equal(ref[f"{name}.ids"], ids.numpy())
    out = R.forward(args, w, ids)
    for k, got in out.items():
        want = ref[f"{name}.{k}"]
        err = float(np.abs(got.numpy() - want).max() / np.abs(want).max())
        assert err <= 2e-5, (k, err)
    assert float(np.abs(ref[f"{name}.stepped"] - ref[f"{name}.logits"]).max() / np.abs(ref[f"{name}.logits"]).max()) <= 2e-5   # the reference's own caches
