#!/usr/bin/env python
"""Runs the reference's OWN ``codec/models/encodec/encodec.py`` (unmodified, imported from where it lies) with ``norm_type = "time_group_norm"`` -- the
48 kHz model's GroupNorm behind every conv and transposed conv -- on seeded checkpoints and stores what it computes in
``tests/golden/ref_encodec_gn_stereo.npz``.

The numpy stand-in for MLX (``mlx_shim.py``, left as it is) has no ``GroupNorm``: one is added to its ``nn`` here at run time -- ``mlx.nn.GroupNorm(1, C,
pytorch_compatible=True)``: one group, statistics over all non-batch axes (float64 here), eps 1e-5, per-channel affine.

``stereo``: ``ENCODEC_ENC_STEREO`` of ``make_reference_fixtures.py`` with the norm switched on (2 channels, non-causal, reflect padding, loudness
    normalisation, rates 5 / 2 / 2, 0.05 s chunks with 20 % overlap), 2 600 samples -> 3 chunks; per chunk the normalised-input encoder embeddings, codes,
    scales and the reference's top-2 score gaps ((best - second) / 2 of its own ``dist``) for both bandwidths, the decoder's stage tensors of chunk 0,
    the decoded audio.
No fixture exists for ``pad_mode = "constant"``: the reference cannot run it -- ``EncodecConv1d._pad1d`` hands ``mx.pad`` ONE (left, right) pair, which
MLX applies to every axis (batch and channels too), and the conv that follows rejects the shape (encodec.py:219-222; the stand-in reproduces that).
Zero padding is held to the restated helper ``tests/_encodec_gn_ref.py`` instead (tests/test_encodec_gn_gpu.py).

Only runs where the reference lies: ``python tests/golden/make_encodec_gn_fixtures.py``.  The checkpoints are regenerated from their seeds by the tests."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_reference_fixtures as M  # noqa: E402  (installs the stand-in)

mx, nn, _np = M.mx, M.nn, M._np


class GroupNorm(nn.Module):
    def __init__(self, num_groups, dims, eps=1e-5, affine=True, pytorch_compatible=False):
        super().__init__()
        assert num_groups == 1 and affine and pytorch_compatible
        self.eps = eps
        self.weight = mx.ones((dims,))
        self.bias = mx.zeros((dims,))

    def __call__(self, x):
        x = np.asarray(x)
        d = x.astype(np.float64)
        ax = tuple(range(1, d.ndim))
        mean = d.mean(axis=ax, keepdims=True)
        var = d.var(axis=ax, keepdims=True)
        y = (d - mean) / np.sqrt(var + self.eps) * np.asarray(self.weight).astype(np.float64) + np.asarray(self.bias).astype(np.float64)
        return mx.array(y.astype(x.dtype))


nn.GroupNorm = GroupNorm


def load_model(cfg_dict, seed_w):
    if "mlx_audio" not in sys.modules:
        M.import_reference()
    if "mlx_audio.codec" not in sys.modules:
        M._pkg("mlx_audio.codec", f"{M.REF}/codec")
        M._pkg("mlx_audio.codec.models", f"{M.REF}/codec/models")
    M._pkg("mlx_audio.codec.models.encodec", f"{M.REF}/codec/models/encodec")
    E = M._load("mlx_audio.codec.models.encodec.encodec", f"{M.REF}/codec/models/encodec/encodec.py")
    from mlx_audio_amd.codec.models.encodec.encodec import make_encodec_encoder_weights, make_encodec_weights

    model = E.Encodec(E.EncodecConfig(**cfg_dict))
    w = make_encodec_weights(cfg_dict, seed=seed_w)
    w.update(make_encodec_encoder_weights(cfg_dict, seed=seed_w))
    assert any(k.endswith(".norm.bias") for k in w)
    model.load_weights([(k, mx.array(v.numpy())) for k, v in w.items()], strict=True)
    return E, model, w


def rvq_gaps(emb, w, n):
    """The reference's search (encodec.py:452-469, 516-533) in numpy float32: codes and the top-2 gap of ``dist`` / 2 per decision."""
    residual = np.asarray(emb, dtype=np.float32)
    codes, gaps = [], []
    for i in range(n):
        e = w[f"quantizer.layers.{i}.codebook.embed"].numpy()
        flat = residual.reshape(-1, residual.shape[-1])
        dist = -((flat ** 2).sum(1, keepdims=True) - 2 * flat @ e.T + (e.T ** 2).sum(0, keepdims=True))
        ind = dist.argmax(-1)
        top = np.sort(dist, axis=1)[:, -2:]
        gaps.append(((top[:, 1] - top[:, 0]) / 2).reshape(residual.shape[:-1]))
        codes.append(ind.reshape(residual.shape[:-1]))
        residual = residual - e[ind].reshape(residual.shape)
    return np.stack(codes, 1), np.stack(gaps, 1).astype(np.float32)


def run(seed_w, seed_audio, cfg_dict, n_samples, tag):
    from mlx_audio_amd.codec.models.encodec.encodec import decoder_layer_names

    E, model, w = load_model(cfg_dict, seed_w)
    g = np.random.default_rng(seed_audio)
    t = np.arange(n_samples) / cfg_dict["sampling_rate"]
    ch = cfg_dict["audio_channels"]
    raw = np.stack([0.5 * np.sin(2 * np.pi * (210 + 130 * c) * t) * (0.6 + 0.4 * np.sin(2 * np.pi * 9 * t)) + 0.15 * g.standard_normal(n_samples) for c in range(ch)], axis=1)
    raw = raw.astype(np.float32)
    inputs, masks = E.preprocess_audio(mx.array(raw if ch > 1 else raw[:, 0]), cfg_dict["sampling_rate"], model.chunk_length, model.chunk_stride)
    out = dict(seed_w=seed_w, seed_audio=seed_audio, config=json.dumps(cfg_dict), raw=raw, inputs=_np(inputs), masks=np.asarray(masks).astype(np.bool_))
    n = inputs.shape[1]
    chunk, stride = (n, n) if model.chunk_length is None else (model.chunk_length, model.chunk_stride)
    embs = []
    for off in range(0, n - (chunk - stride), stride):
        x = inputs[:, off:off + chunk]
        if cfg_dict["normalize"]:
            x = x * masks[:, off:off + chunk][..., None]
            mono = mx.sum(x, axis=2, keepdims=True) / x.shape[2]
            x = x / (mono.square().mean(axis=1, keepdims=True).sqrt() + 1e-8)
        embs.append(_np(model.encoder(x)))
    out["embeddings"] = np.stack(embs)                                     # [chunks, B, T, D]: the encoder on the (normalised) chunk
    for bw in cfg_dict["target_bandwidths"]:
        codes, scales = model.encode(inputs, masks, bandwidth=bw)
        codes = np.asarray(codes).astype(np.int32)
        out[f"codes_bw{bw}"] = codes
        out[f"scales_bw{bw}"] = np.stack([_np(sc) for sc in scales]) if scales[0] is not None else np.zeros(0, np.float32)
        gaps = []
        for ci in range(codes.shape[0]):
            c2, gp = rvq_gaps(embs[ci], w, codes.shape[2])
            assert np.array_equal(c2, codes[ci]), (tag, bw, ci)            # the restated search IS the reference's
            gaps.append(gp)
        out[f"gaps_bw{bw}"] = np.stack(gaps)
    audio = model.decode(mx.array(codes), scales, masks)
    out["decoded"] = _np(audio)
    # the decoder's stage tensors for chunk 0 (the names of Encodec._decoder(return_stages=True))
    names = decoder_layer_names(cfg_dict)
    idx = lambda s: int(s.rsplit(".", 1)[1])  # noqa: E731
    marks = {idx(names["conv_in"]): "conv_in", idx(names["lstm"]): "lstm", idx(names["conv_out"]): "out"}
    for bi, blk in enumerate(names["blocks"]):
        marks[idx(blk["res"][-1] if blk["res"] else blk["up"])] = f"block{bi}"
    h = model.quantizer.decode(mx.array(codes[0]))
    out["dec_z"] = _np(h)
    for i, layer in enumerate(model.decoder.layers):
        h = layer(h)
        if i in marks:
            out["dec_" + marks[i]] = _np(h)
    np.savez_compressed(os.path.join(HERE, f"ref_encodec_gn_{tag}.npz"), **out)
    return {a: (v.shape if hasattr(v, "shape") else v) for a, v in out.items() if a != "config"}


GN_STEREO = dict(M.ENCODEC_ENC_STEREO, norm_type="time_group_norm")

if __name__ == "__main__":
    print("encodec time_group_norm (stereo):", run(43, 5, GN_STEREO, 2600, "stereo"))
