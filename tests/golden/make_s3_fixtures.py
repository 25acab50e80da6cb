#!/usr/bin/env python
"""Runs the reference's OWN ``codec/models/s3/model_v2.py`` and ``utils.py`` (unmodified, imported from where they lie) over the numpy stand-in for MLX
(``mlx_shim.py``, left as it is) on seeded checkpoints and stores what they compute in ``tests/golden/ref_s3_v2.npz``.

The stand-in lacks ``mx.outer`` and ``mx.logical_not`` (model_v2.py / utils.py use both) and ``Module.parameters()`` (only ``sanitize`` uses it): added
here at run time.  ``mlx_audio.utils`` gets ``hanning`` / ``mel_filters`` / ``stft`` from ``mlx_audio.dsp`` before ``s3/utils.py`` is loaded.

The reference's v2 model runs ONE un-padded sequence per call (its attention mask [B, 1, T] against scores [B, H, T, T]): every clip and every 30 s
segment goes through it alone, at B == 1.

  * ``tiny``: 128 wide, 2 heads, 2 layers, 128 mels, ``make_s3_weights(cfg, SEED_W)``; clips of 1001, 163 and 37 mel frames (251, 41, 10 codes): the
    eight FSQ pre-activations ``h`` per frame, codes, ``code_len``; for the two short ones the hidden state behind the stem and every block and the
    FSMN term of block 0 (``forward_fsmn``'s return);
  * ``long``: the same model on a 7 500-frame mel: the reference per segment (3000 / 3000 / 2300 frames from 0 / 2600 / 5200) and its own
    ``merge_tokenized_segments(overlap=4, token_rate=25)`` over the three code lists;
  * the utils helpers on scripted inputs, ``sanitize`` on a scripted dict of torch-style keys;
  * the FSQ margin of every decision is recomputed from ``h`` by the tests: min_d | |h_d| - atanh(0.5 / 0.9990000128746033) |.
The mels are NOT stored: they are regenerated from their seeds (``tests/_s3_ref.synth_mel``); the file holds each one's float64 sum and sum of squares.

Only runs where the reference lies: ``python tests/golden/make_s3_fixtures.py``."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_reference_fixtures as M  # noqa: E402  (installs the stand-in)
import _s3_ref as R  # noqa: E402

mx, nn, _np = M.mx, M.nn, M._np

if not hasattr(mx, "outer"):
    mx.outer = lambda a, b, stream=None: mx.array(np.outer(np.asarray(a), np.asarray(b)))
if not hasattr(mx, "logical_not"):
    mx.logical_not = lambda a, stream=None: mx.array(np.logical_not(np.asarray(a)))


def _parameters(self):
    """Nested dict of the module's parameter arrays (``mlx.nn.Module.parameters``)."""
    return {name: self_get(self, name) for name in self.parameter_names()}


def self_get(obj, dotted):
    for p in dotted.split("."):
        obj = obj[int(p)] if isinstance(obj, (list, tuple)) else getattr(obj, p)
    return obj


if not hasattr(nn.Module, "parameters"):
    nn.Module.parameters = _parameters

SEED_W = 71
TINY = dict(n_mels=128, n_audio_ctx=1500, n_audio_state=128, n_audio_head=2, n_audio_layer=2)
CLIPS = ((1001, 201), (163, 202), (37, 203))   # (mel frames, mel seed)
LONG = (7500, 204)


def load_reference():
    M.import_reference()
    dsp, utils = sys.modules["mlx_audio.dsp"], sys.modules["mlx_audio.utils"]
    for name in ("hanning", "mel_filters", "stft"):
        setattr(utils, name, getattr(dsp, name))
    for pkg, path in (("mlx_audio.codec", "codec"), ("mlx_audio.codec.models", "codec/models"), ("mlx_audio.codec.models.s3", "codec/models/s3")):
        if pkg not in sys.modules:
            M._pkg(pkg, f"{M.REF}/{path}")
    if "huggingface_hub" not in sys.modules:
        import types

        hub = types.ModuleType("huggingface_hub")
        hub.snapshot_download = None
        sys.modules["huggingface_hub"] = hub
    import mlx.utils as mu

    mu.tree_flatten = lambda tree: list(tree.items())   # _parameters above is already flat
    U = M._load("mlx_audio.codec.models.s3.utils", f"{M.REF}/codec/models/s3/utils.py")
    M._load("mlx_audio.codec.models.s3.model", f"{M.REF}/codec/models/s3/model.py")
    V2 = M._load("mlx_audio.codec.models.s3.model_v2", f"{M.REF}/codec/models/s3/model_v2.py")
    return U, V2


def run_one(V2, U, model, mel, stages):
    """The reference on ONE un-padded mel [n_mels, T]: AudioEncoderV2.__call__ (model_v2.py:290-322) stepped through its own modules so that the
    intermediate tensors can be kept, checked against the module's own call."""
    enc = model.encoder
    x = mx.array(mel[None])
    n = mx.array(np.array([mel.shape[1]], dtype=np.int32))
    hidden, code_len = enc(x, n)
    h = model.quantizer.fsq_codebook.project_down(hidden.reshape(-1, hidden.shape[-1]))
    codes = model.quantizer.encode(hidden)
    out = dict(h=_np(h), codes=np.asarray(codes).astype(np.int32)[0], code_len=int(np.asarray(code_len)[0]))
    if stages:
        mask = mx.expand_dims(U.make_non_pad_mask(n), axis=1)
        y = nn.gelu(enc.conv1(x.transpose(0, 2, 1) * mask.transpose(0, 2, 1)))
        n1 = (n + 2 - 1 * (3 - 1) - 1) // enc.stride + 1
        y = nn.gelu(enc.conv2(y * mx.expand_dims(U.make_non_pad_mask(n1), axis=-1)))
        n2 = (n1 + 2 - 1 * (3 - 1) - 1) // 2 + 1
        m = U.make_non_pad_mask(n2)
        mask_pad = mx.expand_dims(m, axis=-1)
        bias = mx.expand_dims(U.mask_to_bias(m, y.dtype), axis=1)
        layers = [_np(y)[0]]
        for i, blk in enumerate(enc.blocks):
            if i == 0:
                hx = blk.attn_ln(y)
                v = blk.attn.value(hx)
                out["fsmn0"] = _np(blk.attn.forward_fsmn(v.reshape(1, v.shape[1], blk.attn.n_head, -1), mask_pad))[0]
            y = blk(y, bias, mask_pad, enc._freqs_cis)
            layers.append(_np(y)[0])
        assert np.array_equal(_np(y), _np(hidden)), "the stepped encoder is not the module's own call"
        out["layers"] = np.stack(layers)
    return out


def main():
    from mlx_audio_amd.codec.models.s3.model_v2 import MAX_FRAMES, WINDOW_STRIDE, ModelConfig, S3TokenizerV2, make_s3_weights

    U, V2 = load_reference()
    cfg = ModelConfig(**TINY)
    w = make_s3_weights(cfg, SEED_W)
    model = V2.S3TokenizerV2("speech_tokenizer_v2_25hz", V2.ModelConfig(**TINY))
    model.load_weights([(k, mx.array(v.numpy())) for k, v in w.items()], strict=True)
    missing, unexpected, mism = model._load_report
    assert not missing and not unexpected and not mism, (missing, unexpected, mism)
    out = dict(config=json.dumps(TINY), seed_w=SEED_W, clips=np.array(CLIPS), long=np.array(LONG))
    all_h = []
    for i, (frames, seed) in enumerate(CLIPS):
        mel = R.synth_mel(seed, TINY["n_mels"], frames)
        out[f"clip{i}_melsum"] = np.array([mel.astype(np.float64).sum(), (mel.astype(np.float64) ** 2).sum()])
        r = run_one(V2, U, model, mel, stages=i > 0)
        # the model's public call gives the same codes
        c2, l2 = model(mx.array(mel[None]), mx.array(np.array([frames], dtype=np.int32)))
        assert np.array_equal(np.asarray(c2)[0], r["codes"]) and int(np.asarray(l2)[0]) == r["code_len"] == len(r["codes"])
        assert np.array_equal(R.fsq_codes(r["h"]), r["codes"]), "the restated FSQ decision is not the reference's"
        for k, v in r.items():
            out[f"clip{i}_{k}"] = np.asarray(v)
        all_h.append(r["h"])
    # long audio: the reference per segment (alone) + its own merge
    frames, seed = LONG
    mel = R.synth_mel(seed, TINY["n_mels"], frames)
    out["long_melsum"] = np.array([mel.astype(np.float64).sum(), (mel.astype(np.float64) ** 2).sum()])
    segs, start = [], 0
    while start < frames:
        segs.append((start, min(start + MAX_FRAMES, frames)))
        start += WINDOW_STRIDE
    out["long_segments"] = np.array(segs)
    lists = []
    for j, (s, e) in enumerate(segs):
        r = run_one(V2, U, model, mel[:, s:e], stages=False)
        out[f"long_seg{j}_h"], out[f"long_seg{j}_codes"] = r["h"], r["codes"]
        lists.append(r["codes"].tolist())
        all_h.append(r["h"])
    out["long_merged"] = np.array(U.merge_tokenized_segments(lists, overlap=4, token_rate=25), dtype=np.int32)
    # utils helpers on scripted inputs
    lens = np.array([5, 3, 2, 7], dtype=np.int32)
    m0 = U.make_non_pad_mask(mx.array(lens))
    out["util_lens"] = lens
    out["util_mask"] = np.asarray(m0).astype(np.bool_)
    out["util_mask_max9"] = np.asarray(U.make_non_pad_mask(mx.array(lens), 9)).astype(np.bool_)
    out["util_bias"] = _np(U.mask_to_bias(m0, mx.float32))
    feats = [np.arange(3 * n, dtype=np.float32).reshape(3, n) + 1 for n in (4, 2, 6)]
    pf, pl = U.padding([mx.array(f) for f in feats])
    out["util_padded"], out["util_padded_lens"] = _np(pf), np.asarray(pl).astype(np.int32)
    merge_in = [list(range(0, 120)), list(range(1000, 1130)), list(range(2000, 2075))]
    out["util_merge_in"] = json.dumps(merge_in)
    out["util_merge_out"] = np.array(U.merge_tokenized_segments(merge_in, overlap=4, token_rate=25), dtype=np.int32)
    out["util_merge_one"] = np.array(U.merge_tokenized_segments([list(range(7))], overlap=4, token_rate=25), dtype=np.int32)
    # sanitize on torch-style keys (shapes only: the values are not touched apart from the swap)
    na, nm = TINY["n_audio_state"], TINY["n_mels"]
    g = np.random.default_rng(5)
    script = {"encoder.conv1.weight": (na, nm, 3), "encoder.conv2.weight": (na, 3, na), "encoder.blocks.0.attn.fsmn_block.weight": (na, 1, 31),
              "encoder.blocks.0.mlp.0.weight": (4 * na, na), "encoder.blocks.1.mlp.2.bias": (na,), "quantizer._codebook.project_down.weight": (8, na),
              "quantizer.codebook.project_down.bias": (8,), "onnx::MatMul_123": (4, 4), "encoder._freqs_cis": (2048, 64), "_mel_filters": (nm, 201),
              "encoder.blocks.1.attn.query.weight": (na, na)}
    sw = {k: g.standard_normal(s).astype(np.float32) for k, s in script.items()}
    res = model.sanitize({k: mx.array(v) for k, v in sw.items()})
    out["sanitize_in"] = json.dumps({k: list(s) for k, s in script.items()})
    out["sanitize_out"] = json.dumps({k: list(np.asarray(v).shape) for k, v in res.items()})
    out["sanitize_conv1"] = _np(res["encoder.conv1.weight"])
    out["sanitize_conv1_in"] = sw["encoder.conv1.weight"]
    # knife-edge share over the whole file
    mg = np.concatenate([R.margins(h) for h in all_h])
    share = float((mg < 3e-3).mean())
    out["margin_share_3e-3"] = np.array(share)
    assert share < 0.04, share
    hs = np.concatenate(all_h)
    print("frames", len(mg), "h std", float(hs.std()), "share < 1e-3 / 3e-3 / 1e-2:", float((mg < 1e-3).mean()), share, float((mg < 1e-2).mean()))
    path = os.path.join(HERE, "ref_s3_v2.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
