#!/usr/bin/env python
"""Runs the reference's OWN ``stt/models/fireredasr2/fireredasr2.py`` and ``config.py``, unmodified and imported from where they lie, over the numpy
stand-in for MLX (``mlx_shim.py``, left as it is) on seeded checkpoints (``make_fireredasr2_weights``) and stores what they compute in
``tests/golden/ref_fireredasr2.npz`` / ``.json``.

The stand-in has no ``nn.Conv2d``; it is defined here (NHWC input, weight [out, kh, kw, in], no padding: what ``Conv2dSubsampling`` uses).
``mlx_audio.stt.utils`` (the audio loader, the hub client behind it) gets an empty stand-in module, as in the other STT makers.

Configs and clips: ``tests/_fireredasr2_ref.CONFIGS`` (A: d_model 128, 2 heads of 64, K 33, 2 + 2 layers, odim 200, beam 3; B: d_model 256, 2 heads
of 128, K 15, 1 + 2 layers, odim 500, beams 1 and 5, ``cmvn.json`` and ``dict.txt`` written to a directory and loaded by ``post_load_hook``; clips of
400 samples = one fbank frame, 0.3 s, 1 s, 3 s).  The audio is NOT stored: it is regenerated from its seeds.  Per clip: the fbank features after
CMVN (the restatement's input), the subsampler output, layer 0's attention and conv-module outputs, every layer's output and the encoder output
(long stages on at most 24 rows: ``*_rows``); per (clip, ending, beam) run -- endings ``late`` (the seeded checkpoint), and on the 1 s clip ``first``
(EOS wins the first step) and ``limit`` (EOS never enters a beam: the ``T_enc`` step limit) -- every step's chosen ``beam_idx``, tokens, scores and
decision margin, taken from the arguments and results of the reference's own ``_topk`` calls inside ``generate``, and ``generate``'s text,
confidence and token count.  The decision margin of a step is the smallest gap between neighbours in the sorted top B + 1 of the B x B
candidates and of each live beam's ``t``.

Asserted before anything is written, on the reference alone: at most 5 % of all steps have a margin below ``tests/_margin.THR``; at least one run
ends by EOS after three or more tokens, one at the first step and one at the step limit.

Only runs where the reference lies: ``python tests/golden/make_fireredasr2_fixtures.py``."""
import json
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_reference_fixtures as M  # noqa: E402  (installs the stand-in)
import _margin  # noqa: E402
import _fireredasr2_ref as R  # noqa: E402

mx, nn, _np = M.mx, M.nn, M._np


class Conv2d(nn.Module):
    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, bias=True):
        super().__init__()
        assert padding == 0
        k = (kernel_size, kernel_size) if isinstance(kernel_size, int) else tuple(kernel_size)
        self.stride = (stride, stride) if isinstance(stride, int) else tuple(stride)
        self.weight = mx.zeros((out_channels, k[0], k[1], in_channels))
        if bias:
            self.bias = mx.zeros((out_channels,))

    def __call__(self, x):
        x, w = np.asarray(x), np.asarray(self.weight)
        N, H, W, C = x.shape
        O, kh, kw, _ = w.shape
        sh, sw = self.stride
        Ho, Wo = (H - kh) // sh + 1, (W - kw) // sw + 1
        y = np.zeros((N, Ho, Wo, O), dtype=np.float32)
        for i in range(kh):
            for j in range(kw):
                y += np.einsum("nhwc,oc->nhwo", x[:, i:i + sh * (Ho - 1) + 1:sh, j:j + sw * (Wo - 1) + 1:sw, :], w[:, i, j, :]).astype(np.float32)
        if "bias" in self.__dict__ or hasattr(self, "bias"):
            y = y + np.asarray(self.bias)
        return mx.array(y.astype(np.float32))


nn.Conv2d = Conv2d


def load_reference():
    M.import_reference()
    for pkg, path in (("mlx_audio.stt", "stt"), ("mlx_audio.stt.models", "stt/models"), ("mlx_audio.stt.models.fireredasr2", "stt/models/fireredasr2")):
        if pkg not in sys.modules:
            M._pkg(pkg, f"{M.REF}/{path}")
    if "mlx_audio.stt.utils" not in sys.modules:
        mod = types.ModuleType("mlx_audio.stt.utils")
        mod.load_audio = None
        sys.modules["mlx_audio.stt.utils"] = mod
    M._load("mlx_audio.stt.models.base", f"{M.REF}/stt/models/base.py")
    cfg = M._load("mlx_audio.stt.models.fireredasr2.config", f"{M.REF}/stt/models/fireredasr2/config.py")
    fr = M._load("mlx_audio.stt.models.fireredasr2.fireredasr2", f"{M.REF}/stt/models/fireredasr2/fireredasr2.py")
    return cfg, fr


def sub(a):
    """At most 24 rows of a [T, C] stage (all of a short one), with their indices."""
    T = a.shape[0]
    rows = np.arange(T) if T <= 24 else np.unique(np.r_[0:T:-(-T // 23), T - 1])
    return a[rows].astype(np.float32), rows.astype(np.int32)


def run_encoder(model, audio):
    feats = model._extract_fbank(mx.array(audio))
    if model._cmvn is not None:
        feats = (feats - model._cmvn[0]) * model._cmvn[1]
    f = _np(feats).astype(np.float32)
    enc = model.encoder
    x = mx.array(f)[None]
    x = mx.concatenate([x, mx.zeros((1, enc.input_preprocessor.context - 1, x.shape[2]))], axis=1)
    x = enc.input_preprocessor(x)
    st = dict(sub=_np(x)[0].copy())
    pos = enc.positional_encoding(x)
    layers = []
    for i, layer in enumerate(enc.layer_stack):
        if i == 0:
            h = 0.5 * x + 0.5 * layer.ffn1(x)
            h = layer.mhsa(h, h, h, pos)
            st["attn0"] = _np(h)[0].copy()
            st["conv0"] = _np(layer.conv(h))[0].copy()
        x = layer(x, pos)
        layers.append(_np(x)[0].copy())
    whole = _np(enc(mx.array(f)[None]))
    assert np.array_equal(_np(x), whole), "the stepped encoder is not the module's own call"
    st["enc"] = _np(x)[0].copy()
    out = dict(feats=f)
    for k, v in st.items():
        out[k], out[k + "_rows"] = sub(v)
    for i, l in enumerate(layers):
        out[f"layer{i}"], _ = sub(l)
    return out


def run_generate(model, c, audio, B, **kw):
    """``generate`` with the decoder's ``_topk`` recorded: call 2 s is the per-beam top-B of step s (x = t_scores [B, V]), call 2 s + 1 the top-B of
    the B x B sums."""
    dec = model.decoder
    calls = []
    orig = type(dec)._topk

    def spy(x, k):
        v, i = orig(dec, x, k)
        calls.append((_np(x).astype(np.float64).copy(), _np(v).copy(), _np(i).copy()))
        return v, i

    dec._topk = spy
    try:
        res = model.generate(np.asarray(audio), beam_size=B, **kw)
    finally:
        del dec._topk
    assert len(calls) % 2 == 0
    fin = np.zeros(B, dtype=bool)
    steps = dict(beam_idx=[], tokens=[], scores=[], margin=[])
    for s in range(len(calls) // 2):
        t, _, idx1 = calls[2 * s]
        allsc, best, bidx = calls[2 * s + 1]
        margin = 1e10
        srt = -np.sort(-t, axis=-1)
        for i in range(B):
            if not fin[i]:
                margin = min(margin, float((srt[i, :B] - srt[i, 1:B + 1]).min()))
        s2 = -np.sort(-allsc.reshape(-1))[:B + 1]
        if s2.size > 1:
            margin = min(margin, float((s2[:-1] - s2[1:]).min()))
        ys = np.where(fin[:, None], c.eos_id, idx1)
        bidx = bidx.reshape(-1)
        tok = ys.reshape(-1)[bidx]
        steps["beam_idx"].append((bidx // B).astype(np.int32))
        steps["tokens"].append(tok.astype(np.int32))
        steps["scores"].append(best.reshape(-1).astype(np.float32))
        steps["margin"].append(margin)
        fin = tok == c.eos_id
    arrays = {k: np.asarray(v) for k, v in steps.items()}
    return arrays, dict(text=res.text, confidence=res.segments[0]["confidence"], generation_tokens=res.generation_tokens, steps=len(steps["margin"]),
                        all_finished=bool(fin.all()))


def main():
    from mlx_audio_amd.stt.models.fireredasr2 import expected_shapes, make_fireredasr2_weights

    C, S = load_reference()
    out, meta = {}, dict(configs={})
    margins, runs = [], []
    for tag, cc in R.CONFIGS.items():
        config = C.ModelConfig.from_dict(dict(cc["cfg"]))
        mine = R.make_config(cc["cfg"])
        base = make_fireredasr2_weights(mine, cc["seed_w"], logit_gain=cc["logit_gain"], eos_gain=cc["eos_gain"])
        assert {k: tuple(v.shape) for k, v in base.items()} == expected_shapes(mine)
        models = {}
        with tempfile.TemporaryDirectory() as d:
            with open(os.path.join(d, "dict.txt"), "w", encoding="utf8") as f:
                f.write("".join(f"{wd} {i}\n" for i, wd in enumerate(R.make_dict(mine.odim))))
            if cc["cmvn"]:
                mean, istd = R.cmvn_for(tag)
                with open(os.path.join(d, "cmvn.json"), "w") as f:
                    json.dump(dict(means=mean.tolist(), istd=istd.tolist()), f)
            for ending in R.ENDINGS:
                model = S.FireRedASR2(config)
                w = R.eos_variant(base, mine, ending)
                model.load_weights([(k, mx.array(v.numpy())) for k, v in w.items()], strict=True)
                missing, unexpected, mism = model._load_report
                assert not unexpected and not mism and all(m.endswith("positional_encoding.pe") for m in missing), (missing, unexpected, mism)
                model.eval()
                models[ending] = S.FireRedASR2.post_load_hook(model, d)
                assert models[ending]._tokenizer is not None and (models[ending]._cmvn is not None) == cc["cmvn"]
        meta["configs"][tag] = dict(cfg=cc["cfg"], names=sorted(base), runs=[])
        for i, (n, seed) in enumerate(cc["clips"]):
            audio = R.synth_audio(seed, n)
            out[f"{tag}{i}_audiosum"] = np.array([audio.astype(np.float64).sum(), (audio.astype(np.float64) ** 2).sum()])
            enc = run_encoder(models["late"], audio)
            for k, v in enc.items():
                out[f"{tag}{i}_{k}"] = np.asarray(v)
            for ending in (R.ENDINGS if i == 2 else ("late",)):
                for B in cc["beams"]:
                    arrays, info = run_generate(models[ending], config, audio, B)
                    key = f"{tag}{i}_{ending}_b{B}"
                    for k, v in arrays.items():
                        out[f"{key}_{k}"] = v
                    info.update(clip=i, ending=ending, beam=B, key=key)
                    meta["configs"][tag]["runs"].append(info)
                    margins += list(arrays["margin"])
                    runs.append(info)
                    print(key, "rows", enc["enc"].shape, "steps", info["steps"], "tokens", info["generation_tokens"], "fin" if info["all_finished"] else "limit",
                          "min margin %.5f" % min(arrays["margin"]), repr(info["text"][:24]), info["confidence"])
        # the reference's own test intent (stt/tests/test_fireredasr2.py): beam_size = 1, max_len = 10
        arrays, info = run_generate(models["late"], config, R.synth_audio(cc["clips"][2][1], cc["clips"][2][0]), 1, max_len=10)
        assert info["steps"] <= 10
        for k, v in arrays.items():
            out[f"{tag}2_maxlen10_b1_{k}"] = v
        info.update(clip=2, ending="late", beam=1, key=f"{tag}2_maxlen10_b1", max_len=10)
        meta["configs"][tag]["runs"].append(info)
        margins += list(arrays["margin"])
    low = sum(1 for m in margins if m < _margin.THR)
    print(f"{low} of {len(margins)} steps have a margin below {_margin.THR}")
    assert low <= 0.05 * len(margins), (low, len(margins))
    assert any(r["all_finished"] and r["generation_tokens"] >= 3 for r in runs), "no run ends by EOS after three or more tokens"
    assert any(r["ending"] == "first" and r["generation_tokens"] == 0 and r["all_finished"] for r in runs), "no run ends at the first step"
    assert any(r["ending"] == "limit" and not r["all_finished"] for r in runs), "no run reaches the step limit"
    path = os.path.join(HERE, "ref_fireredasr2.npz")
    np.savez_compressed(path, **out)
    with open(os.path.join(HERE, "ref_fireredasr2.json"), "w") as f:
        json.dump(meta, f, ensure_ascii=False, indent=1)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= 1_000_000


if __name__ == "__main__":
    main()
