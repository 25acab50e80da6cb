"""A quantised (MLX `-4bit`, router at 8 bits) Ling / Ming checkpoint through ``sanitize`` + ``Model`` against the float ``Model`` on the same
dequantised weights.  The checkpoints are fp16-exact by the recipe of tests/test_whisper_quantized_gpu.py (group 64, scale a power of two, zero =
-2^(bits - 1) scale), so the float engine's images hold them exactly.  Configs A and B of tests/_bailing_moe_ref.py, B with moe_intermediate_size 64
(no group divides its 48); written as per-expert tensors, so ``sanitize`` does the stacking.  Measured on MI355X: docs/COVERAGE.md row f3."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _bailing_moe_ref as R  # noqa: E402
from _margin import THR  # noqa: E402

from mlx_audio_amd import ops  # noqa: E402
from mlx_audio_amd.lm import moe  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = 64
BAR = 3e-4   # of the peak: the project's standing stage bar


def _quantize(w, bits):
    g = w.reshape(*w.shape[:-1], -1, G)
    scale = torch.pow(2.0, torch.ceil(torch.log2(2 * g.abs().amax(-1).clamp_min(2.0 ** -14) / ((1 << bits) - 1))))
    zero = -(1 << (bits - 1)) * scale
    codes = torch.round((g - zero[..., None]) / scale[..., None]).clamp_(0, (1 << bits) - 1).to(torch.int64)
    deq = (scale[..., None] * codes + zero[..., None]).reshape(w.shape)
    assert torch.equal(deq.half().float(), deq)
    words = ops.pack_codes(codes.reshape(-1, w.shape[-1]), bits).view(torch.int32).reshape(*w.shape[:-1], -1)
    return words, scale.half(), zero.half(), deq


def _checkpoints(name, everything):
    """(args, the quantised checkpoint with per-expert tensors, the float checkpoint of its dequantised weights)."""
    cfg = dict(R.CONFIGS[name], moe_intermediate_size=64)
    if everything:
        cfg["quantization"] = {"group_size": G, "bits": 4, "model.layers.1.mlp.gate.gate_proj": {"group_size": G, "bits": 8}}
    args = moe.ModelArgs.from_dict(cfg)
    w = {k: v.to(torch.bfloat16).float() for k, v in moe.make_moe_weights(args, R.SEEDS[name]).items()}
    ck, ref = {}, {}
    for key, v in w.items():
        base = key[:-len(".weight")]
        expert = ".switch_mlp." in key
        if not key.endswith(".weight") or v.dim() < 2 or not (expert or everything):
            ck[key] = ref[key] = v
            continue
        words, scales, biases, deq = _quantize(v, 8 if base.endswith("gate.gate_proj") else 4)
        ref[key] = deq
        parts = {"weight": words, "scales": scales, "biases": biases}
        if expert:   # as the checkpoint files have them: one set per expert, and the router under its file name
            for e in range(args.num_experts):
                ck.update({base.replace("switch_mlp.", f"experts.{e}.") + "." + k: t[e] for k, t in parts.items()})
        else:
            ck.update({base.replace("gate.gate_proj", "gate") + "." + k: t for k, t in parts.items()})
    for key in [k for k in ck if ".switch_mlp." in k and k.endswith(".bias")]:
        stacked = ck.pop(key)
        ck.update({key.replace("switch_mlp.", f"experts.{e}."): stacked[e] for e in range(args.num_experts)})
    return args, ck, ref


@pytest.mark.parametrize("name,everything", [("A", False), ("B", False), ("A", True), ("B", True)], ids=["A-experts", "B-experts", "A-all", "B-all"])
def test_quantized_checkpoint_matches_the_float_model_on_its_dequantisation(name, everything):
    args, ck, ref = _checkpoints(name, everything)
    qm, fm = moe.Model(args, moe.sanitize(ck, args), DEV), moe.Model(args, ref, DEV)
    assert isinstance(qm.model.layers[1][3].switch_mlp.experts, ops.PackedQuantizedExperts)
    assert isinstance(qm.lm_head, ops.QuantizedLinear) == everything
    ids = torch.randint(0, args.vocab_size, (R.TOKENS,), generator=torch.Generator().manual_seed(R.SEEDS[name]))
    L, i, k = ids.numel(), args.first_k_dense_replace, args.num_experts_per_tok
    tq, tf = {}, {}
    got, want = qm(ids[None], trace=tq)[0], fm(ids[None], trace=tf)[0]
    steps = [(m(ids[None, :L - 2], c), m(ids[None, L - 2:L - 1], c), m(ids[None, L - 1:], c)) for m, c in ((qm, qm.make_cache()), (fm, fm.make_cache()))]
    got_s, want_s = (torch.cat(s, 1)[0] for s in steps)
    for what, a, b in (("prefill", got, want), ("15 + 2 steps", got_s, want_s)):
        err = float((a - b).abs().max() / b.abs().max())
        print(f"BAILING quantised {name} {'all' if everything else 'experts'} {what}: logits err/peak {err:.2e}")
        assert err <= BAR, (what, err)
    # router: the same experts wherever the float model's own selection is not on a knife edge
    bias = qm.model.layers[i][3].gate.expert_bias
    sel = R._select(tf[f"router_logits{i}"].double().cpu(), None if bias is None else bias.double().cpu(), args)[1].sort(-1, descending=True).values
    sure = (sel[:, k - 1] - sel[:, k]) >= THR
    print(f"BAILING quantised {name}: router rows compared {int(sure.sum())} of {L}")
    assert int(sure.sum()) >= 0.9 * L
    assert torch.equal(tq[f"ids{i}"].cpu().sort(-1).values[sure], tf[f"ids{i}"].cpu().sort(-1).values[sure])
    top2 = want.cpu().topk(2, -1).values
    clear = (top2[:, 0] - top2[:, 1]) >= THR
    assert torch.equal(got.cpu().argmax(-1)[clear], want.cpu().argmax(-1)[clear])
