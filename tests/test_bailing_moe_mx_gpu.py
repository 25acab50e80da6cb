"""A `-mxfp4` / `-nvfp4` / `-mxfp8` Ling / Ming checkpoint (``moe.quantize_checkpoint_mx``: per-expert tensors, so ``sanitize`` does the stacking) through
``sanitize`` + ``Model`` against the float ``Model`` on the same dequantised weights (at most six significant bits times a power of two: the float engine's
images hold them exactly).  Configs A and B of tests/_bailing_moe_ref.py; B keeps its moe_intermediate_size of 48 at nvfp4 (a last half step in every down
projection) and takes 64 at the 32-code modes.  Measured on MI355X: docs/COVERAGE.md row f3."""
import pytest
import torch

import _bailing_moe_ref as R
from _margin import THR
from mlx_audio_amd import ops
from mlx_audio_amd.lm import moe

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAR = 3e-4   # of the peak: the project's standing stage bar
ROUTER = "model.layers.1.mlp.gate.gate_proj"


def _checkpoints(name, mode, form, config_mode=None):
    """(args, checkpoint, float checkpoint of its dequantised weights).  ``form``: ``experts``, ``all`` (every matrix) or ``router8`` (all, the router affine)."""
    cfg = dict(R.CONFIGS[name]) if mode == "nvfp4" else dict(R.CONFIGS[name], moe_intermediate_size=64)
    if form != "experts" or config_mode:
        cfg["quantization"] = {"mode": config_mode or mode, "group_size": ops.QMODES[mode][2], "bits": ops.QMODES[mode][1]}
    args = moe.ModelArgs.from_dict(cfg)
    w = {k: v.to(torch.bfloat16).float() for k, v in moe.make_moe_weights(args, R.SEEDS[name]).items()}
    return (args, *moe.quantize_checkpoint_mx(w, args, mode, everything=form != "experts", affine8=(ROUTER,) if form == "router8" else ()))


CASES = [(n, m, f) for m in ops.QMODES for n, f in (("A", "experts"), ("B", "experts"), ("A", "all"), ("B", "all"))] + [("A", "mxfp4", "router8")]


@pytest.mark.parametrize("name,mode,form", CASES, ids=["-".join(c) for c in CASES])
def test_mx_checkpoint_matches_the_float_model_on_its_dequantisation(name, mode, form):
    args, ck, ref = _checkpoints(name, mode, form)
    qm, fm = moe.Model(args, moe.sanitize(ck, args), DEV), moe.Model(args, ref, DEV)
    block, dense = qm.model.layers[1][3], (ops.QuantizedLinearMX if form != "experts" else type(fm.lm_head))
    assert isinstance(block.switch_mlp.experts, ops.PackedQuantizedExpertsMX) and block.switch_mlp.experts.gate.mode == mode
    assert type(qm.lm_head) is dense and isinstance(qm.model.word_embeddings, ops.QuantizedLinearMX) == (form != "experts")
    assert type(block.gate.lin) is (ops.QuantizedLinear if form == "router8" else dense)
    assert (qm.lm_head is qm.model.word_embeddings) == (form != "experts" and args.tie_word_embeddings)
    ids = torch.randint(0, args.vocab_size, (R.TOKENS,), generator=torch.Generator().manual_seed(R.SEEDS[name]))
    L, i, k = ids.numel(), args.first_k_dense_replace, args.num_experts_per_tok
    tq, tf = {}, {}
    got, want = qm(ids[None], trace=tq)[0], fm(ids[None], trace=tf)[0]
    steps = [(m(ids[None, :L - 2], c), m(ids[None, L - 2:L - 1], c), m(ids[None, L - 1:], c)) for m, c in ((qm, qm.make_cache()), (fm, fm.make_cache()))]
    for what, a, b in (("prefill", got, want), ("15 + 2 steps", *(torch.cat(s, 1)[0] for s in steps))):
        err = float((a - b).abs().max() / b.abs().max())
        print(f"BAILING MX {name} {mode} {form} {what}: logits err/peak {err:.2e}")
        assert err <= BAR, (what, err)
    bias = block.gate.expert_bias   # router: the same experts wherever the float model's own selection is not on a knife edge
    sel = R._select(tf[f"router_logits{i}"].double().cpu(), None if bias is None else bias.double().cpu(), args)[1].sort(-1, descending=True).values
    sure = (sel[:, k - 1] - sel[:, k]) >= THR
    assert torch.equal(tq[f"ids{i}"].cpu().sort(-1).values[sure], tf[f"ids{i}"].cpu().sort(-1).values[sure])
    assert torch.equal(got.cpu().argmax(-1), want.cpu().argmax(-1))


def test_a_config_mode_that_contradicts_the_shapes_is_refused_by_name():
    args, ck, _ = _checkpoints("A", "mxfp4", "experts", config_mode="mxfp8")
    with pytest.raises(ValueError, match=r"switch_mlp.gate_proj: quantization mode 'mxfp8' contradicts the shapes.*uint8 scales is mxfp4"):
        moe.Model(args, moe.sanitize(ck, args), DEV)
