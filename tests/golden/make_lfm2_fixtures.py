#!/usr/bin/env python
"""Runs the reference's OWN ``lm/models/lfm2.py``, unmodified and imported from where it lies, over the numpy stand-in for MLX (``mlx_shim.py``, which
lacks nothing this model calls) on the seeded checkpoints of ``make_lfm2_weights`` (values rounded to bfloat16, which
every weight image holds exactly) and stores, per configuration of ``tests/_lfm2_ref.py``: the token ids, every decoder layer's output and the
logits of ONE 17-token pass through fresh caches, the logits of 15 tokens followed by two one-row steps through the reference's caches
(``KVCache`` / ``ArraysCache``), and the top-2 gap of every logits row -- in ``tests/golden/ref_lfm2.npz`` / ``.json``.

Only runs where the reference lies: ``python tests/golden/make_lfm2_fixtures.py``."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_reference_fixtures as M  # noqa: E402  (installs the stand-in)
import _lfm2_ref as R  # noqa: E402

mx, _np = M.mx, M._np


def main():
    M.import_reference()
    M.import_lm_and_mimi()
    F = M._load("mlx_audio.lm.models.lfm2", f"{M.REF}/lm/models/lfm2.py")
    arrays, meta = {}, {}
    for name in R.CONFIGS:
        args, w, ids = R.setup(name)
        rargs = F.ModelArgs.from_dict(R.CONFIGS[name])
        assert rargs.full_attn_idxs == args.full_attn_idxs and rargs.rope_theta == args.rope_theta
        model = F.Model(rargs)
        # conv.weight as a torch checkpoint holds it, [H, 1, L]: the reference's own sanitize turns it
        ck = model.sanitize({k: mx.array((v.permute(0, 2, 1) if "conv.weight" in k else v).numpy()) for k, v in w.items()})
        model.load_weights(list(ck.items()), strict=True)
        assert model.layers[[i for i in range(args.num_hidden_layers) if i not in args.full_attn_idxs][0]].feed_forward.w1.weight.shape[0] == args.ff_dim
        tok = mx.array(ids.numpy()[None])
        cache = model.make_cache()
        h = model.model.embed_tokens(tok)
        for i, (layer, c) in enumerate(zip(model.layers, cache)):
            h = layer(h, "causal" if layer.is_attention_layer else None, cache=c)
            arrays[f"{name}.layer{i}"] = _np(h)[0].astype(np.float32)
        logits = _np(model(tok, model.make_cache()))[0].astype(np.float32)
        walked = _np(model.model.embed_tokens.as_linear(model.model.embedding_norm(h)))[0]
        assert np.allclose(walked, logits, atol=1e-5), "the stepped layers do not reproduce Model.__call__"
        cache = model.make_cache()
        parts = [model(tok[:, :R.PREFILL], cache)] + [model(tok[:, t:t + 1], cache) for t in range(R.PREFILL, R.TOKENS)]
        stepped = np.concatenate([_np(p)[0] for p in parts]).astype(np.float32)
        top = np.sort(logits.astype(np.float64), -1)
        arrays[f"{name}.ids"], arrays[f"{name}.logits"], arrays[f"{name}.stepped"] = ids.numpy().astype(np.int32), logits, stepped
        arrays[f"{name}.gap"] = (top[:, -1] - top[:, -2]).astype(np.float32)
        meta[name] = dict(config=R.CONFIGS[name], seed=R.SEEDS[name], tokens=R.TOKENS, prefill=R.PREFILL, ff_dim=args.ff_dim,
                          stepped_vs_one_pass=float(np.abs(stepped - logits).max()))
    np.savez_compressed(os.path.join(HERE, "ref_lfm2.npz"), **arrays)
    with open(os.path.join(HERE, "ref_lfm2.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    print({k: v.shape for k, v in arrays.items()}, meta)


if __name__ == "__main__":
    main()
