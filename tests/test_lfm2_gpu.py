"""The device ``lm.lfm2.Model`` against the reference's own stored runs (``tests/golden/ref_lfm2.npz``): every layer output and the logits within
3e-4 of the peak, arg-max tokens equal wherever the stored top-2 gap is at least ``_margin.THR``; prefill of 17 tokens against 15 + 2 steps and a
right-padded batch against its items alone (1e-5 of the peak); ``input_embeddings`` against the token path."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _lfm2_ref as R  # noqa: E402
import _margin  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", params=sorted(R.CONFIGS))
def case(request):
    from mlx_audio_amd.lm import lfm2

    args, w, ids = R.setup(request.param)
    return request.param, args, lfm2.Model(args, lfm2.sanitize(w), DEV), ids, w


def test_stages_against_the_reference_runs(case):
    name, args, model, ids, _ = case
    ref = np.load(R.GOLDEN)
    trace = {}
    logits = model(ids[None], trace=trace)[0].cpu().numpy()
    for k, got in [(f"layer{i}", trace[f"layer{i}"][0].cpu().numpy()) for i in range(args.num_hidden_layers)] + [("logits", logits)]:
        want = ref[f"{name}.{k}"]
        err = float(np.abs(got.astype(np.float64) - want).max() / np.abs(want).max())
        print(f"LFM2 {name} {k}: err/peak {err:.2e}")
        assert err <= 3e-4, (k, err)
    sure = ref[f"{name}.gap"] >= _margin.THR
    print(f"LFM2 {name}: arg-max rows compared {int(sure.sum())} of {sure.size}")
    assert sure.sum() >= 12 and np.array_equal(logits.argmax(-1)[sure], ref[f"{name}.logits"].argmax(-1)[sure])


def test_prefill_equals_shorter_prefill_plus_two_decode_steps(case):
    name, _, model, ids, _ = case
    full = model(ids[None])[0]
    cache = model.make_cache()
    parts = [model(ids[None, :R.PREFILL], cache)] + [model(ids[None, t:t + 1], cache) for t in range(R.PREFILL, R.TOKENS)]
    assert all(c.offset == R.TOKENS for c in cache)
    stepped = torch.cat(parts, 1)[0]
    err = float((stepped - full).abs().max() / full.abs().max())
    want = np.load(R.GOLDEN)[f"{name}.stepped"]
    err_ref = float(np.abs(stepped.cpu().numpy() - want).max() / np.abs(want).max())
    print(f"LFM2 {name} prefill vs prefill + 2 steps: {err:.2e}; steps vs the reference's: {err_ref:.2e}")
    assert err <= 1e-5 and err_ref <= 3e-4


def test_padded_batch_against_its_items(case):
    _, args, model, ids, _ = case
    lens = [ids.numel(), 5, 1]
    batch = torch.zeros(len(lens), max(lens), dtype=ids.dtype)
    for b, n in enumerate(lens):
        batch[b, :n] = ids.flip(0)[:n] if b else ids
    cache = model.make_cache()
    out = model(batch, cache, lengths=lens)
    for b, n in enumerate(lens):   # causal attention and a causal conv: right padding cannot reach an item's own rows; lengths keep its state its own
        alone_cache = model.make_cache()
        alone = model(batch[b:b + 1, :n], alone_cache)[0]
        err = float((out[b, :n] - alone).abs().max() / alone.abs().max())
        assert err <= 1e-5, (b, err)
        for c, ca in zip(cache, alone_cache):
            if hasattr(c, "state"):
                assert float((c.state[b] - ca.state[0]).abs().max()) <= 1e-5 * float(ca.state.abs().max()), b


def test_input_embeddings_equal_the_token_path(case):
    _, _, model, ids, w = case
    emb = w["model.embed_tokens.weight"][ids][None]
    assert torch.equal(model(None, input_embeddings=emb), model(ids[None]))
