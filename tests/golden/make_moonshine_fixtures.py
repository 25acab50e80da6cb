#!/usr/bin/env python
"""Runs the reference's OWN ``stt/models/moonshine/moonshine.py`` and ``config.py``, unmodified and imported from where they lie, over the numpy
stand-in for MLX (``mlx_shim.py``, left as it is) on seeded checkpoints (``make_moonshine_weights``) and stores what they compute in
``tests/golden/ref_moonshine.npz`` / ``.json``.

The stand-in has no ``nn.GroupNorm``; it is defined here (one group: the two conventions of MLX's module agree).  ``mlx_audio.stt.utils`` (the audio
loader, the hub client behind it) gets an empty stand-in module, as in the other STT makers.

Configs and clips: ``tests/_moonshine_ref.CONFIGS`` (A: 4 heads of 36, tied; B: 4 heads of 52, ENCODER kv heads 2, untied ``proj_out`` -- the reference's decoder cannot step with grouped kv heads: it caches the
repeated k / v and concatenates the next step's unrepeated ones to them (moonshine.py:127-137), so decoder kv heads 2 is held to
``tests/_moonshine_ref.py`` instead; 2 + 2
layers; clips of 895 samples = one frame, ~0.3 s, 1 s, 3 s).  The audio is NOT stored: it is regenerated from its seeds; the file holds each clip's
float64 sum and sum of squares.  Per clip: the stem stages (after tanh, after GroupNorm, conv2, conv3), layer 0's attention output, every layer's
output, the encoder output (long stages on at most 24 rows: ``*_rows``), the greedy tokens at ``max_tokens`` = 24 with each step's logits row and
top-2 gap, the decoder's hidden states for a T = 3 call and then a T = 2 call over its cache, and ``generate``'s text and counters.

Asserted before anything is written, on the reference alone: no stored decision has a top-2 gap below ``tests/_margin.THR``; at least one sequence
ends by EOS after three or more tokens and at least one runs to ``max_tokens``; the stepped encoder equals the module's own call; the manual greedy
loop equals ``generate``.

Only runs where the reference lies: ``python tests/golden/make_moonshine_fixtures.py``."""
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_reference_fixtures as M  # noqa: E402  (installs the stand-in)
import _margin  # noqa: E402
import _moonshine_ref as R  # noqa: E402

mx, nn, _np = M.mx, M.nn, M._np


class GroupNorm(nn.Module):
    def __init__(self, num_groups, dims, eps=1e-5, affine=True, pytorch_compatible=False):
        super().__init__()
        assert num_groups == 1 and affine
        self.eps = eps
        self.weight = mx.ones((dims,))
        self.bias = mx.zeros((dims,))

    def __call__(self, x):
        x = np.asarray(x)
        d = x.astype(np.float64)
        ax = tuple(range(1, d.ndim))
        y = (d - d.mean(axis=ax, keepdims=True)) / np.sqrt(d.var(axis=ax, keepdims=True) + self.eps)
        return mx.array((y * np.asarray(self.weight).astype(np.float64) + np.asarray(self.bias).astype(np.float64)).astype(x.dtype))


nn.GroupNorm = GroupNorm


def load_reference():
    M.import_reference()
    for pkg, path in (("mlx_audio.stt", "stt"), ("mlx_audio.stt.models", "stt/models"), ("mlx_audio.stt.models.moonshine", "stt/models/moonshine")):
        if pkg not in sys.modules:
            M._pkg(pkg, f"{M.REF}/{path}")
    if "mlx_audio.stt.utils" not in sys.modules:
        mod = types.ModuleType("mlx_audio.stt.utils")
        mod.load_audio = None
        sys.modules["mlx_audio.stt.utils"] = mod
    M._load("mlx_audio.stt.models.base", f"{M.REF}/stt/models/base.py")
    cfg = M._load("mlx_audio.stt.models.moonshine.config", f"{M.REF}/stt/models/moonshine/config.py")
    ms = M._load("mlx_audio.stt.models.moonshine.moonshine", f"{M.REF}/stt/models/moonshine/moonshine.py")
    return cfg, ms


def sub(a):
    """At most 24 rows of a [T, C] stage (all of a short one), with their indices."""
    T = a.shape[0]
    rows = np.arange(T) if T <= 24 else np.unique(np.r_[0:T:-(-T // 23), T - 1])
    return a[rows].astype(np.float32), rows.astype(np.int32)


def run_clip(model, c, audio):
    enc = model.encoder
    x = mx.array(audio)[None, :, None]
    st = {}
    x = mx.tanh(enc.conv1(x)); st["tanh"] = _np(x)[0].copy()
    x = enc.groupnorm(x); st["gn"] = _np(x)[0].copy()
    x = nn.gelu(enc.conv2(x)); st["conv2"] = _np(x)[0].copy()
    x = nn.gelu(enc.conv3(x)); st["conv3"] = _np(x)[0].copy()
    pos = mx.arange(x.shape[1])[None, :]
    layers = []
    for i, layer in enumerate(enc.layers):
        if i == 0:
            st["attn0"] = _np(layer.self_attn(layer.input_layernorm(mx.array(_np(x).copy())), position_ids=pos)[0])[0].copy()
        x = layer(mx.array(_np(x).copy()), position_ids=pos)
        layers.append(_np(x)[0].copy())
    enc_out = enc.layer_norm(x)
    assert np.array_equal(_np(enc_out), _np(enc(mx.array(audio)))), "the stepped encoder is not the module's own call"
    st["enc"] = _np(enc_out)[0].copy()
    out = {}
    for k, v in st.items():
        out[k], out[k + "_rows"] = sub(v)
    for i, l in enumerate(layers):
        out[f"layer{i}"], _ = sub(l)
    # the greedy loop of generate(), keeping each step's logits row
    tokens, cache, rows, gaps, eos = [c.decoder_start_token_id], None, [], [], False
    for _ in range(R.MAX_TOKENS):
        hidden, cache = model.decoder(mx.array([[tokens[-1]]], dtype=mx.int32), enc_out, cache=cache)
        lg = _np(model._get_logits(hidden[:, -1, :])).astype(np.float32)[0]
        top = np.sort(lg)
        rows.append(lg.copy())
        gaps.append(float(top[-1] - top[-2]))
        nxt = int(lg.argmax())
        if nxt == c.eos_token_id:
            eos = True
            break
        tokens.append(nxt)
    res = model.generate(np.asarray(audio), max_tokens=R.MAX_TOKENS)
    text = model._decode_tokens(tokens[1:])
    assert res.text == text.strip() and res.generation_tokens == len(tokens) - 1 and res.total_tokens == len(tokens) and res.prompt_tokens == 1
    h1, cache = model.decoder(mx.array([R.FORCED[:3]], dtype=mx.int32), enc_out, cache=None)
    h2, _ = model.decoder(mx.array([R.FORCED[3:]], dtype=mx.int32), enc_out, cache=cache)
    out.update(logits=np.stack(rows), gap=np.array(gaps, dtype=np.float32), forced=np.concatenate([_np(h1)[0], _np(h2)[0]]).astype(np.float32))
    return out, dict(tokens=[int(t) for t in tokens[1:]], eos=eos, text=res.text, segments=res.segments, prompt_tokens=res.prompt_tokens,
                     generation_tokens=res.generation_tokens, total_tokens=res.total_tokens)


def main():
    from mlx_audio_amd.stt.models.moonshine import expected_shapes, make_moonshine_weights

    C, S = load_reference()
    out, meta = {}, dict(max_tokens=R.MAX_TOKENS, forced=R.FORCED, configs={})
    all_gaps, decs = [], []
    for tag, cc in R.CONFIGS.items():
        config = C.ModelConfig.from_dict(dict(cc["cfg"]))
        model = S.Model(config)
        mine = R.make_config(cc["cfg"])
        w = make_moonshine_weights(mine, cc["seed_w"], logit_gain=cc["logit_gain"], eos_gain=cc["eos_gain"])
        model.load_weights([(k, mx.array(v.numpy())) for k, v in w.items()], strict=True)
        missing, unexpected, mism = model._load_report
        assert not missing and not unexpected and not mism, (missing, unexpected, mism)
        assert {k: tuple(v.shape) for k, v in w.items()} == expected_shapes(mine)
        model.eval()
        meta["configs"][tag] = dict(cfg=cc["cfg"], names=sorted(w), decode=[])
        for i, (n, seed) in enumerate(cc["clips"]):
            audio = R.synth_audio(seed, n)
            out[f"{tag}{i}_audiosum"] = np.array([audio.astype(np.float64).sum(), (audio.astype(np.float64) ** 2).sum()])
            r, dec = run_clip(model, config, audio)
            for k, v in r.items():
                out[f"{tag}{i}_{k}"] = np.asarray(v)
            meta["configs"][tag]["decode"].append(dec)
            all_gaps += list(r["gap"])
            decs.append(dec)
            print(tag, i, n, "frames", r["enc"].shape, "tokens", len(dec["tokens"]), "eos" if dec["eos"] else "max", "min gap %.4f" % min(r["gap"]), repr(dec["text"][:30]))
    assert min(all_gaps) >= _margin.THR, min(all_gaps)
    assert any(d["eos"] and len(d["tokens"]) >= 3 for d in decs), "no sequence ends by EOS after three or more tokens"
    assert any(not d["eos"] and len(d["tokens"]) == R.MAX_TOKENS for d in decs), "no sequence runs to max_tokens"
    path = os.path.join(HERE, "ref_moonshine.npz")
    np.savez_compressed(path, **out)
    with open(os.path.join(HERE, "ref_moonshine.json"), "w") as f:
        json.dump(meta, f, ensure_ascii=False, indent=1)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= 1_000_000


if __name__ == "__main__":
    main()
