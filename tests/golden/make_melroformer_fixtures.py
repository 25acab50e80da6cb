#!/usr/bin/env python
"""Runs the reference's OWN ``sts/models/mel_roformer/config.py`` and ``model.py``, unmodified and imported from where they lie, over the numpy
stand-in for MLX (``mlx_shim.py``, left as it is) on seeded checkpoints and stores what they compute in ``tests/golden/ref_melroformer.npz`` /
``ref_melroformer.json``.  Pieces the stand-in lacks are added here at run time.

  * config ``A``: dim 64, depth 2, 2 heads of 64, 8 bands, n_fft 64, hop 16, mask_estimator_depth 2;
  * config ``B``: dim 32, depth 1, 1 head of 64, 6 bands, n_fft 32, hop 8, mask_estimator_depth 1, ff_mult 2, mlp_expansion_factor 2.
Their band widths are asserted below (A: 8 8 8 12 20 28 48 80; B: 4 4 8 12 24 48), as is that both hold bins covered once and bins covered twice.
Clips come from seeds (``tests/_melroformer_ref.synth_clip``) and are NOT stored, only their float64 sum and sum of squares: the shortest length the
reference's reflect padding accepts (n_fft / 2 + 1), about 400 and about 1 000 samples, one whose first 128 samples are exactly zero, and one
``B = 2`` call.  Per call: the band-split output, the output of each transformer of level 0, the merged mask and the waveform; the three
activation tensors of calls with more than ``STRIDE_ABOVE`` frames are stored every ``STRIDE``-th frame (the file's size).

Asserted before writing: the stepped path reproduces ``MelRoFormer.__call__`` bit for bit; the waveform differs from the input by more than 10 % of
its peak and is not all zero; no mask is constant; the silent frames' split output equals the bias rows.

Only runs where the reference lies: ``python tests/golden/make_melroformer_fixtures.py``."""
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_reference_fixtures as M  # noqa: E402  (installs the stand-in)
import _melroformer_ref as R  # noqa: E402

mx, nn = M.mx, M.nn
SEED_W = 11
STRIDE_ABOVE, STRIDE = 20, 4
WIDTHS = {"A": [8, 8, 8, 12, 20, 28, 48, 80], "B": [4, 4, 8, 12, 24, 48]}

CONFIGS = {
    "A": dict(kw=dict(depth=2, dim=64, heads=2, dim_head=64, num_bands=8, n_fft=64, win_length=64, hop_length=16, mask_estimator_depth=2),
              calls=[[(31, 33, 0)], [(32, 400, 0)], [(33, 1000, 0)], [(34, 416, 128)], [(35, 400, 0), (36, 400, 0)]]),
    "B": dict(kw=dict(depth=1, dim=32, heads=1, dim_head=64, num_bands=6, n_fft=32, win_length=32, hop_length=8, mask_estimator_depth=1, ff_mult=2,
                      mlp_expansion_factor=2),
              calls=[[(41, 17, 0)], [(42, 403, 0)], [(43, 1001, 0)], [(44, 400, 128)], [(45, 200, 0), (46, 200, 0)]]),
}


def _children(self):
    """``Module._children`` through lists of any depth (the stand-in's stops at two levels; ``MaskEstimator.to_freqs`` has three)."""
    def walk(prefix, v):
        if isinstance(v, nn.Module):
            yield prefix, v
        elif isinstance(v, (list, tuple)):
            for i, e in enumerate(v):
                yield from walk(f"{prefix}.{i}", e)
    for k, v in self.__dict__.items():
        yield from walk(k, v)


def load_reference():
    if not hasattr(mx, "outer"):
        mx.outer = lambda a, b, stream=None: mx.array(np.outer(np.asarray(a), np.asarray(b)))
    nn.Module._children = _children
    M.import_reference()
    for pkg, path in (("mlx_audio.sts", "sts"), ("mlx_audio.sts.models", "sts/models"), ("mlx_audio.sts.models.mel_roformer", "sts/models/mel_roformer")):
        if pkg not in sys.modules:
            M._pkg(pkg, f"{M.REF}/{path}")
    u = sys.modules["mlx_audio.utils"]
    if not hasattr(u, "get_model_path"):
        u.get_model_path = lambda p, *a, **k: p
    base = f"{M.REF}/sts/models/mel_roformer"
    return {name: M._load(f"mlx_audio.sts.models.mel_roformer.{name}", f"{base}/{name}.py") for name in ("config", "model")}


def build(ref, tag):
    from mlx_audio_amd.sts.models import mel_roformer as mine

    kw = CONFIGS[tag]["kw"]
    cfg = ref["config"].MelRoFormerConfig.custom(**kw)
    my_cfg = mine.MelRoFormerConfig.custom(**kw)
    assert {f: getattr(cfg, f) for f in cfg.__dataclass_fields__} == {f: getattr(my_cfg, f) for f in my_cfg.__dataclass_fields__}
    w = mine.make_melroformer_weights(my_cfg, SEED_W)
    model = ref["model"].MelRoFormer(cfg)
    assert model.band_split.filterbank.band_dims == WIDTHS[tag], model.band_split.filterbank.band_dims
    names = set(model.parameter_names())
    assert names == set(w), sorted(names ^ set(w))[:6]                         # every name of the seeded checkpoint finds its parameter
    wt = mine.make_melroformer_weights(my_cfg, SEED_W, torch_names=True)       # through the reference's own sanitize, from the PyTorch names
    model.load_weights([(k, mx.array(v.numpy())) for k, v in model.sanitize(wt).items()], strict=True)
    assert model._load_report == ([], [], []), model._load_report
    for k, v in w.items():
        obj = model
        for p in k.split("."):
            obj = obj[int(p)] if isinstance(obj, (list, tuple)) else getattr(obj, p)
        assert np.array_equal(np.asarray(obj), v.numpy()), k
    return model, cfg, w


def stepped(model, cfg, audio):
    """MelRoFormer.__call__ (model.py:581-646) again, step by step, so that the stage tensors can be kept."""
    rm = sys.modules["mlx_audio.sts.models.mel_roformer.model"]
    window = mx.array(np.hanning(cfg.n_fft + 1)[:-1].astype(np.float32))
    re, im = rm.stft(audio, cfg.n_fft, cfg.hop_length, window)
    B, F, T = re.shape[0], re.shape[2], re.shape[3]
    rep = mx.stack([re.transpose(0, 2, 1, 3).reshape(B, F * 2, T), im.transpose(0, 2, 1, 3).reshape(B, F * 2, T)], axis=-1)
    x = model.band_split.split(rep)
    st = dict(split=np.asarray(x))
    Nb, D = x.shape[2], x.shape[3]
    for lv, (time_tf, freq_tf) in enumerate(model.layers):
        x = time_tf(x.transpose(0, 2, 1, 3).reshape(B * Nb, T, D)).reshape(B, Nb, T, D).transpose(0, 2, 1, 3)
        if lv == 0:
            st["tf0"] = np.asarray(x)
        x = freq_tf(x.reshape(B * T, Nb, D)).reshape(B, T, Nb, D)
        if lv == 0:
            st["tf1"] = np.asarray(x)
    mask = model.band_split.merge(model.mask_estimators[0](x), F * 2)
    st["mask"] = np.asarray(mask)
    o_re = rep[..., 0] * mask[..., 0] - rep[..., 1] * mask[..., 1]
    o_im = rep[..., 0] * mask[..., 1] + rep[..., 1] * mask[..., 0]
    y = rm.istft(o_re.reshape(B, F, 2, T).transpose(0, 2, 1, 3), o_im.reshape(B, F, 2, T).transpose(0, 2, 1, 3), cfg.n_fft, cfg.hop_length, window,
                 audio.shape[2])
    return np.asarray(y), st, T


def main():
    ref = load_reference()
    out, meta = {}, dict(seed_w=SEED_W, stride_above=STRIDE_ABOVE, stride=STRIDE, configs={})
    for tag, c in CONFIGS.items():
        model, cfg, w = build(ref, tag)
        idx = [np.asarray(ix) for ix in model.band_split.filterbank.freq_indices]
        cover = np.bincount(np.concatenate(idx), minlength=2 * cfg.freq_bins)
        assert cover.min() >= 1 and (cover == 1).any() and (cover == 2).any() and cover.max() == 2, cover
        out[f"{tag}_band_ptr"] = np.concatenate([[0], np.cumsum([len(ix) for ix in idx])]).astype(np.int32)
        out[f"{tag}_band_idx"] = np.concatenate(idx).astype(np.int32)
        out[f"{tag}_count"] = np.asarray(model.band_split.filterbank.num_bands_per_freq, dtype=np.float32)
        meta["configs"][tag] = dict(kw=c["kw"], widths=WIDTHS[tag], calls=[[list(cl) for cl in call] for call in c["calls"]], frames=[])
        bias = np.stack([w[f"band_split.to_features.{n}.1.bias"].numpy() for n in range(cfg.num_bands)])
        for i, call in enumerate(c["calls"]):
            x = np.stack([R.synth_clip(seed, n, zero) for seed, n, zero in call])                     # [B, 2, S]
            out[f"{tag}{i}_clipsum"] = np.array([x.astype(np.float64).sum(), (x.astype(np.float64) ** 2).sum()])
            wave = np.asarray(model(mx.array(x)), dtype=np.float32)
            y, st, T = stepped(model, cfg, mx.array(x))
            assert np.array_equal(y.astype(np.float32), wave), "the stepped path is not MelRoFormer.__call__"
            meta["configs"][tag]["frames"].append(T)
            peak = float(np.abs(wave).max())
            diff = float(np.abs(wave - x).max())
            print(tag, i, x.shape, "->", T, "frames; input peak", float(np.abs(x).max()), "output peak", peak, "max |out - in|", diff,
                  "mask in", float(st["mask"].min()), float(st["mask"].max()))
            assert peak > 0 and diff > 0.1 * peak, (peak, diff)
            assert float(st["mask"].max()) > float(st["mask"].min())
            for (seed, n, zero), b in zip(call, range(len(call))):
                if zero:
                    silent = [t for t in range(T) if t * cfg.hop_length + cfg.n_fft // 2 <= zero]       # frames wholly inside the zeros
                    assert len(silent) >= 2 and np.array_equal(st["split"][b, silent], np.broadcast_to(bias, (len(silent),) + bias.shape)), "silent frames"
                    meta["configs"][tag].setdefault("silent_frames", {})[str(i)] = silent
            out[f"{tag}{i}_wave"] = wave
            out[f"{tag}{i}_mask"] = st["mask"].astype(np.float32)
            for k in ("split", "tf0", "tf1"):
                v = st[k].astype(np.float32)
                assert float(v.max()) > float(v.min()), (tag, i, k)
                out[f"{tag}{i}_{k}"] = v[:, ::STRIDE] if T > STRIDE_ABOVE else v
    path = os.path.join(HERE, "ref_melroformer.npz")
    np.savez_compressed(path, **out)
    with open(os.path.join(HERE, "ref_melroformer.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= 870_000


if __name__ == "__main__":
    main()
