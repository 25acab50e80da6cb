"""The device ``lm.moe.Model`` against the reference's own stored runs (``tests/golden/ref_bailing_moe.npz``), stage by stage: router ids exact
wherever the stored selection gap is at least ``_margin.THR`` (the count is printed and asserted), layer outputs and logits within 3e-4 of the peak;
prefill of L tokens against L - 2 prefill + 2 decode steps (1e-5 of the peak); a right-padded batch against its items alone."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _bailing_moe_ref as R  # noqa: E402
import _margin  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", params=sorted(R.CONFIGS))
def case(request):
    from mlx_audio_amd.lm import moe

    args, w, ids = R.setup(request.param)
    return request.param, args, moe.Model(args, w, DEV), ids


def test_stages_against_the_reference_runs(case):
    name, args, model, ids = case
    ref = np.load(R.GOLDEN)
    trace = {}
    logits = model(ids[None], trace=trace)[0].cpu().numpy()
    i = args.first_k_dense_replace
    sure = ref[f"{name}.router{i}.gap"] >= _margin.THR
    print(f"BAILING {name}: router rows compared {int(sure.sum())} of {sure.size}")
    assert sure.sum() >= 12
    got_ids = np.sort(trace[f"ids{i}"].cpu().numpy(), -1)
    assert np.array_equal(got_ids[sure], ref[f"{name}.router{i}.ids"][sure])
    stages = {"layer0": (trace["layer0"][0].cpu().numpy(), slice(None)), "layer1": (trace["layer1"][0].cpu().numpy(), sure), "logits": (logits, sure),
              f"router{i}.wsum": (trace[f"weights{i}"].sum(-1).cpu().numpy(), sure)}
    for k, (got, rows) in stages.items():
        want = ref[f"{name}.{k}"]
        err = float(np.abs(got.astype(np.float64) - want)[rows].max() / np.abs(want).max())
        print(f"BAILING {name} {k}: err/peak {err:.2e}")
        assert err <= 3e-4, (k, err)


def test_prefill_equals_shorter_prefill_plus_two_decode_steps(case):
    _, _, model, ids = case
    L = ids.numel()
    full = model(ids[None])[0]
    cache = model.make_cache()
    parts = [model(ids[None, :L - 2], cache), model(ids[None, L - 2:L - 1], cache), model(ids[None, L - 1:], cache)]
    assert cache[0].offset == L
    err = float((torch.cat(parts, 1)[0] - full).abs().max() / full.abs().max())
    print(f"BAILING prefill vs prefill + 2 steps: {err:.2e}")
    assert err <= 1e-5


def test_padded_batch_against_its_items(case):
    _, args, model, ids = case
    lens = [ids.numel(), 5, 1]
    batch = torch.zeros(len(lens), max(lens), dtype=ids.dtype)
    for b, n in enumerate(lens):
        batch[b, :n] = ids.flip(0)[:n] if b else ids
    out = model(batch)
    for b, n in enumerate(lens):   # causal attention: right padding cannot reach an item's own rows
        alone = model(batch[b:b + 1, :n])[0]
        err = float((out[b, :n] - alone).abs().max() / alone.abs().max())
        assert err <= 1e-5, (b, err)
