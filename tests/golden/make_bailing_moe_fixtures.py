#!/usr/bin/env python
"""Runs the reference's OWN ``lm/models/bailing_moe.py`` and ``switch_layers.py``, unmodified and imported from where they lie, over the numpy
stand-in for MLX (``mlx_shim.py`` + ``mlx_shim_moe.py``) on the seeded checkpoints of ``make_moe_weights`` (values rounded to bfloat16, which
every weight image holds exactly) and stores, per configuration of ``tests/_bailing_moe_ref.py``: the token ids, every decoder layer's output, the
router's ids (sorted: the reference's ``argpartition`` leaves their order open) with the selection gap of every token, the block's routed weights
summed per token, and the logits -- of ONE causal pass without a cache, in ``tests/golden/ref_bailing_moe.npz`` / ``.json``.  The reference's
``sanitize`` runs on a checkpoint with per-expert tensors and the stacked result is what the model loads.

Only runs where the reference lies: ``python tests/golden/make_bailing_moe_fixtures.py``."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_reference_fixtures as M  # noqa: E402  (installs the stand-in)
import mlx_shim_moe  # noqa: E402
import _bailing_moe_ref as R  # noqa: E402

mx, _np = M.mx, M._np
mlx_shim_moe.install(mx, M.nn)


def main():
    M.import_reference()
    M.import_lm_and_mimi()
    M._load("mlx_audio.lm.models.switch_layers", f"{M.REF}/lm/models/switch_layers.py")
    B = M._load("mlx_audio.lm.models.bailing_moe", f"{M.REF}/lm/models/bailing_moe.py")
    arrays, meta = {}, {}
    for name in R.CONFIGS:
        args, w, ids = R.setup(name)
        rargs = B.ModelArgs.from_dict(R.CONFIGS[name])
        model = B.Model(rargs)
        # per-expert tensors in, the reference's own sanitize stacks them
        ck = {}
        for k, v in w.items():
            if ".switch_mlp." in k and k.endswith(".weight"):   # (the reference stacks weights only; expert biases come stacked)
                for e in range(args.num_experts):
                    ck[k.replace(".switch_mlp.", f".experts.{e}.")] = mx.array(v[e].numpy())
            else:
                ck[k] = mx.array(v.numpy())
        ck = model.sanitize(ck)
        assert sorted(ck) == sorted(w), (sorted(set(ck) ^ set(w)))
        model.load_weights(list(ck.items()), strict=True)
        seen = {}
        for i, layer in enumerate(model.model.layers):
            if hasattr(layer.mlp, "gate"):
                gate = layer.mlp.gate

                def spy(x, gate=gate, i=i):
                    inds, sc = type(gate).__call__(gate, x)
                    g = _np(gate.gate_proj(x)).astype(np.float64)[0]
                    seen[i] = (np.sort(_np(inds)[0].astype(np.int64), -1), _np(sc)[0].sum(-1), R.selection_gap(g, gate, args))
                    return inds, sc

                layer.mlp.gate = spy
        h = model.model.word_embeddings(mx.array(ids.numpy()[None]))
        for i, layer in enumerate(model.model.layers):
            h = layer(h, "causal", None)
            arrays[f"{name}.layer{i}"] = _np(h)[0].astype(np.float32)
        for i, layer in enumerate(model.model.layers):   # the spies off again: the whole-model call below must run the reference untouched
            if i in seen:
                layer.mlp.gate = layer.mlp.gate.__defaults__[0]
        logits = _np(model(mx.array(ids.numpy()[None])))[0].astype(np.float32)
        stepped = _np(model.lm_head(model.model.norm(h)) if not rargs.tie_word_embeddings else model.model.word_embeddings.as_linear(model.model.norm(h)))[0]
        assert np.allclose(stepped, logits, atol=1e-5), "the stepped layers do not reproduce Model.__call__"
        arrays[f"{name}.ids"], arrays[f"{name}.logits"] = ids.numpy().astype(np.int32), logits
        for i, (inds, wsum, gap) in seen.items():
            arrays[f"{name}.router{i}.ids"], arrays[f"{name}.router{i}.wsum"], arrays[f"{name}.router{i}.gap"] = inds, wsum.astype(np.float32), gap.astype(np.float32)
        meta[name] = dict(config=R.CONFIGS[name], seed=R.SEEDS[name], tokens=int(ids.numel()), sparse_layers=sorted(seen))
    np.savez_compressed(os.path.join(HERE, "ref_bailing_moe.npz"), **arrays)
    with open(os.path.join(HERE, "ref_bailing_moe.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    print({k: v.shape for k, v in arrays.items()})


if __name__ == "__main__":
    main()
