#!/usr/bin/env python
"""Runs the reference's OWN ``sts/models/mossformer2_se`` files and ``dsp.py``, unmodified and imported from where they lie, over the numpy stand-in
for MLX (``mlx_shim.py``, left as it is) on seeded checkpoints and stores what they compute in ``tests/golden/ref_mossformer2.npz`` / ``.json``.
Pieces the stand-in lacks are added here at run time: ``nn.GroupNorm`` (one group), ``nn.PReLU``, ``nn.ReLU``, ``nn.Conv2d``, ``Module.update``,
``mx.stop_gradient``, ``mx.contiguous(allow_col_major=)``, ``mx.core.fast.metal_kernel`` keyed by kernel name (``relu_squared``: max(x, 0)^2;
``custom_depthwise_conv1d``: the zero-padded correlation its source states) and stubs for ``huggingface_hub`` and ``sam_audio.processor.load_audio``.
Kaldi's dither stays ON: ``mx.random.normal`` is served from ``numpy.random.default_rng(seed)`` so that a test can redraw the same numbers.

  * config ``A``: ``MossFormer_MaskNet(180, 64, 961, num_blocks=2)`` installed on the reference's ``TestNet``, the real front end; clips of
    1, 2, 58, 256, 257 and 300 frames (1920 + (frames - 1) * 384 samples);
  * config ``B``: width 32, 1 block; 257 and 300 frames (weight seed 14: of the seeds 11 .. 16 tried, 12, 14 and 15 meet the conditions below and 14 leaves the most exact zeros).
Weights come from ``make_mossformer2_weights`` and clips from ``tests/_mossformer2_ref.synth_clip``; neither is stored (clips: their float64 sum and
sum of squares).  Per call: the assembled 180-column features, the output of layer 0's FLASH and of its Gated-FSMN block, the mask and the
waveform.  Features of more than ``FEAT_FULL`` frames and stage tensors of more than ``STRIDE_ABOVE`` frames keep every ``STRIDE``-th frame; the mask
of such calls also keeps every ``MASK_COL_STRIDE``-th column and their waveforms every ``WAVE_STRIDE``-th sample (the file's size).  Once, with decode
lengths scaled down (windows and chunks of 59 frames, whole-clip limit 1 s, a 2.3 s clip): ``enhance`` through the segmented path and through
``_decode_chunked``.  Also stored: the parameter names and shapes of the reference's full-size ``MossFormer2SE``.

Asserted before writing: the stepped path reproduces the reference's forward bit for bit; every stored stage is finite with standard deviation in
[1e-2, 1e2]; no mask column is constant over time (calls of more than 20 frames); the mask has exact zeros and positive entries; in layer 0 the quadratic and the linear term each
carry at least 10 % of A's energy; the waveform differs from the input by more than 10 % of its peak.

Only runs where the reference lies: ``python tests/golden/make_mossformer2_fixtures.py``."""
import importlib
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_reference_fixtures as M  # noqa: E402  (installs the stand-in)
import _mossformer2_ref as R  # noqa: E402

mx, nn = M.mx, M.nn
SEED_W = 11
STRIDE_ABOVE, STRIDE, FEAT_FULL, MASK_COL_STRIDE, WAVE_STRIDE = 20, 4, 64, 6, 16
WIN, HOP = 1920, 384
PKG = "mlx_audio.sts.models.mossformer2_se"

CONFIGS = {
    "A": dict(kw=dict(out_channels=64, num_blocks=2), seed_w=11, calls=[(101, 1), (102, 2), (103, 58), (104, 256), (105, 257), (106, 300)]),
    "B": dict(kw=dict(out_channels=32, num_blocks=1), seed_w=14, calls=[(111, 257), (112, 300)]),
}
LONG = dict(one_time_decode_length=1, decode_window=24192 / 48000, chunk_seconds=24192 / 48000, auto_chunk_threshold=2.0)
LONG_CLIP = (121, int(2.3 * 48000))
NOISE_SEED = 1000        # + the call's clip seed


def samples(frames):
    return WIN + (frames - 1) * HOP


# ------------------------------------------------------------------------------------------------ run-time additions to the stand-in
def _torch():
    import torch
    return torch


class GroupNorm(nn.Module):
    def __init__(self, num_groups, dims, eps=1e-5, affine=True, pytorch_compatible=False):
        super().__init__()
        assert num_groups == 1, "only GroupNorm(1, C) is on this path"
        self.eps, self.dims = eps, dims
        if affine:
            self.weight, self.bias = mx.ones((dims,)), mx.zeros((dims,))

    def __call__(self, x):
        a = np.asarray(x, dtype=np.float32)
        ax = tuple(range(1, a.ndim))
        mean = a.mean(axis=ax, keepdims=True)
        var = a.var(axis=ax, keepdims=True)
        y = (a - mean) * (1.0 / np.sqrt(var + np.float32(self.eps)))
        if "weight" in self.__dict__:
            y = y * np.asarray(self.weight) + np.asarray(self.bias)
        return mx.array(y.astype(np.float32))


class PReLU(nn.Module):
    def __init__(self, num_parameters=1, init=0.25):
        super().__init__()
        self.weight = mx.full((num_parameters,), init, dtype=np.float32)

    def __call__(self, x):
        return mx.maximum(0, x) + self.weight * mx.minimum(0, x)


class ReLU(nn.Module):
    def __call__(self, x):
        return mx.maximum(x, 0)


class Conv2d(nn.Module):
    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias=True):
        super().__init__()
        kh, kw = (kernel_size, kernel_size) if isinstance(kernel_size, int) else kernel_size
        self.weight = mx.zeros((out_channels, kh, kw, in_channels // groups))
        if bias:
            self.bias = mx.zeros((out_channels,))
        self.stride, self.padding, self.groups = stride, padding, groups

    def __call__(self, x):
        torch = _torch()
        xt = torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float32))).permute(0, 3, 1, 2)
        wt = torch.from_numpy(np.ascontiguousarray(np.asarray(self.weight, dtype=np.float32))).permute(0, 3, 1, 2)
        b = torch.from_numpy(np.asarray(self.bias, dtype=np.float32)) if "bias" in self.__dict__ else None
        y = torch.nn.functional.conv2d(xt, wt, b, stride=self.stride, padding=self.padding, groups=self.groups)
        return mx.array(y.permute(0, 2, 3, 1).contiguous().numpy())


def _metal_kernel(name, input_names, output_names, header="", source="", **kw):
    if name == "relu_squared":
        def call(inputs, output_shapes, output_dtypes, **k):
            v = np.maximum(np.asarray(inputs[0], dtype=np.float32), np.float32(0))
            return [mx.array(v * v)]
        return call
    if name == "custom_depthwise_conv1d":
        def call(inputs, output_shapes, output_dtypes, **k):
            x, w, params = (np.asarray(t) for t in inputs)
            B, L, C, K, pad, Lout = (int(v) for v in params)
            x, w = x.astype(np.float32).reshape(B, L, C), w.astype(np.float32).reshape(C, K)
            acc = np.zeros((B, Lout, C), dtype=np.float32)
            for k_ in range(K):   # acc += inp[time + k - pad] * weight[chan, k] where 0 <= time + k - pad < L, k ascending
                lo, hi = max(0, pad - k_), min(Lout, L + pad - k_)
                if hi > lo:
                    acc[:, lo:hi] += x[:, lo + k_ - pad:hi + k_ - pad] * w[:, k_]
            return [mx.array(acc)]
        return call

    def unused(*a, **k):   # the module defines more kernels than the model's path calls
        raise NotImplementedError(f"metal kernel {name!r} has no stand-in")
    return unused


class _Noise:
    """``mx.random`` for the run: normal draws from a numpy generator the tests can rebuild; everything else from the stand-in's."""

    def __init__(self, base):
        self.base, self.rng = base, np.random.default_rng(0)

    def reseed(self, seed):
        self.rng = np.random.default_rng(seed)

    def normal(self, shape=(), dtype=np.float32, loc=0.0, scale=1.0, key=None, stream=None):
        return mx.array((self.rng.standard_normal(tuple(shape)).astype(np.float32) * np.float32(scale) + np.float32(loc)).astype(np.float32))

    def __getattr__(self, k):
        return getattr(self.base, k)


def load_reference():
    for name, cls in (("GroupNorm", GroupNorm), ("PReLU", PReLU), ("ReLU", ReLU), ("Conv2d", Conv2d)):
        if not hasattr(nn, name):
            setattr(nn, name, cls)
    if not hasattr(nn.Module, "update"):
        nn.Module.update = lambda self, tree: self.load_weights(list(tree.items()))
    if not hasattr(mx, "stop_gradient"):
        mx.stop_gradient = lambda a, stream=None: a
    mx.contiguous = lambda a, allow_col_major=False, stream=None: mx.array(np.ascontiguousarray(np.asarray(a)))
    fast = types.ModuleType("mlx.core.fast")
    for k in dir(mx.fast):
        if not k.startswith("__"):
            setattr(fast, k, getattr(mx.fast, k))
    fast.metal_kernel = _metal_kernel
    sys.modules["mlx.core.fast"] = fast
    mx.random = _Noise(mx.random)
    hub = types.ModuleType("huggingface_hub")
    hub.hf_hub_download = lambda *a, **k: (_ for _ in ()).throw(RuntimeError("no hub here"))
    sys.modules.setdefault("huggingface_hub", hub)
    M.import_reference()
    for pkg, path in (("mlx_audio.sts", "sts"), ("mlx_audio.sts.models", "sts/models"), (PKG, "sts/models/mossformer2_se"),
                      ("mlx_audio.sts.models.sam_audio", "sts/models/sam_audio")):
        if pkg not in sys.modules:
            M._pkg(pkg, f"{M.REF}/{path}")
    proc = types.ModuleType("mlx_audio.sts.models.sam_audio.processor")
    proc.load_audio = lambda *a, **k: (_ for _ in ()).throw(RuntimeError("file input is not part of the fixtures"))
    sys.modules["mlx_audio.sts.models.sam_audio.processor"] = proc
    return importlib.import_module(PKG + ".model")


# ------------------------------------------------------------------------------------------------ the reference, built and stepped
def build(rm, kw, extra_cfg=None, seed_w=SEED_W):
    from mlx_audio_amd.sts.models import mossformer2_se as mine

    net_mod = importlib.import_module(PKG + ".mossformer_masknet")
    cfg = rm.MossFormer2SEConfig.from_dict({**kw, **(extra_cfg or {})})
    my_cfg = mine.MossFormer2SEConfig.from_dict({**kw, **(extra_cfg or {})})
    assert cfg.to_dict() == my_cfg.to_dict()
    model = rm.MossFormer2SEModel(cfg)
    model.model.model.mossformer = net_mod.MossFormer_MaskNet(cfg.in_channels, cfg.out_channels, cfg.out_channels_final, num_blocks=cfg.num_blocks)
    w = mine.make_mossformer2_weights(my_cfg, seed_w)
    names = set(model.model.parameter_names())
    assert names == set(w), sorted(names ^ set(w))[:8]
    model.load_weights([(k, mx.array(v.numpy())) for k, v in w.items()])          # the reference's own load_weights
    assert model.model._load_report == ([], [], []), model.model._load_report
    return model, cfg, w


def features(model, audio):
    """model.py:384-399 again (the reference's own dsp functions), so that the features can be kept."""
    rm = sys.modules[PKG + ".model"]
    c = model.config
    fb = rm.compute_fbank_kaldi(audio, sample_rate=c.sample_rate, win_len=c.win_len, win_inc=c.win_inc, num_mels=c.num_mels, win_type=c.win_type,
                                preemphasis=c.preemphasis)
    ft = mx.transpose(fb, [1, 0])
    d1 = rm.compute_deltas_kaldi(ft, win_length=5)
    d2 = rm.compute_deltas_kaldi(d1, win_length=5)
    return mx.expand_dims(mx.concatenate([fb, mx.transpose(d1, [1, 0]), mx.transpose(d2, [1, 0])], axis=1), axis=0)


def stepped(net, feats):
    """MossFormer_MaskNet.__call__ (mossformer_masknet.py:122-205) with Computation_Block, MossFormerM and MossFormerBlock_GFSMN unrolled, step by
    step over the reference's own sub-modules; -> (mask [B, T, F], stages)."""
    x = mx.transpose(feats, (0, 2, 1))
    x = net.norm(x)
    x = mx.transpose(net.conv1d_encoder(mx.transpose(x, (0, 2, 1))), (0, 2, 1))
    base = x
    xt = mx.transpose(x, (0, 2, 1))
    emb = net.pos_enc(xt)
    emb = mx.broadcast_to(mx.expand_dims(emb, axis=0), (xt.shape[0], emb.shape[0], emb.shape[1]))
    x = base + mx.transpose(emb, (0, 2, 1))
    blk = net.mdl
    intra = mx.transpose(x, (0, 2, 1))
    g = blk.intra_mdl.mossformerM
    st = {}
    for i in range(g.depth):
        if i == 0:   # the two attention terms of layer 0: quad_q = 0 leaves the linear term alone
            st["energy"] = _attention_terms(g.layers[0], intra)
        intra = g.layers[i](intra, mask=None)
        if i == 0:
            st["flash0"] = np.asarray(intra)
        intra = g.fsmn[i](intra)
        if i == 0:
            st["fsmn0"] = np.asarray(intra)
    intra = blk.intra_mdl.norm(intra)
    intra = blk.intra_norm(intra)
    x = mx.transpose(intra, (0, 2, 1)) + x
    x = net.prelu(x)
    x = mx.transpose(net.conv1d_out(mx.transpose(x, (0, 2, 1))), (0, 2, 1))
    B, _, S = x.shape
    x = mx.transpose(mx.reshape(x, (B * net.num_spks, -1, S)), (0, 2, 1))
    x = mx.tanh(net.output(x)) * mx.sigmoid(net.output_gate(x))
    x = mx.transpose(net.conv1_decoder(x), (0, 2, 1))
    _, N, L = x.shape
    x = net.activation(mx.reshape(x, (B, net.num_spks, N, L)))
    x = mx.transpose(x, (1, 0, 2, 3))
    return mx.transpose(x[0], (0, 2, 1)), st


def _attention_terms(layer, x):
    """flash_sharea_ffconvm.py:134-171 up to cal_attention, then cal_attention twice: as it is, and with quad_q = 0 (the linear term alone)."""
    x_shift, x_pass = mx.split(x, 2, axis=-1)
    if x_shift.shape[1] > 1:
        x_shift = mx.concatenate([mx.zeros((x_shift.shape[0], 1, x_shift.shape[2])), x_shift[:, :-1, :]], axis=1)
    else:
        x_shift = mx.zeros_like(x_shift)
    nx = mx.concatenate([x_shift, x_pass], axis=-1)
    v, u = mx.split(layer.to_hidden(nx), 2, axis=-1)
    quad_q, lin_q, quad_k, lin_k = layer.qk_offset_scale(layer.to_qk(nx))
    av, au = layer.cal_attention(x, quad_q, lin_q, quad_k, lin_k, v, u, None)
    lv, lu = layer.cal_attention(x, quad_q * 0, lin_q, quad_k, lin_k, v, u, None)
    A = np.concatenate([np.asarray(av), np.asarray(au)], -1).astype(np.float64)
    lin = np.concatenate([np.asarray(lv), np.asarray(lu)], -1).astype(np.float64)
    tot = float((A ** 2).sum())
    return dict(quad=float(((A - lin) ** 2).sum()) / tot, lin=float((lin ** 2).sum()) / tot)


def strided(v, T, axis=0):
    return np.take(v, np.arange(0, T, STRIDE), axis=axis) if T > STRIDE_ABOVE else v


def main():
    rm = load_reference()
    wrap = importlib.import_module(PKG + ".mossformer2_se_wrapper")
    full = wrap.MossFormer2SE()
    meta = dict(seed_w=SEED_W, stride_above=STRIDE_ABOVE, stride=STRIDE, feat_full=FEAT_FULL, mask_col_stride=MASK_COL_STRIDE, wave_stride=WAVE_STRIDE,
                noise_seed=NOISE_SEED, configs={}, parameters={k: list(_param(full, k).shape) for k in full.parameter_names()})
    del full
    out = {}
    for tag, c in CONFIGS.items():
        model, cfg, w = build(rm, c["kw"], None, c["seed_w"])
        net = model.model.model.mossformer
        meta["configs"][tag] = dict(kw=c["kw"], seed_w=c["seed_w"], calls=[list(cl) for cl in c["calls"]], energy=[])
        for i, (seed, frames) in enumerate(c["calls"]):
            clip = R.synth_clip(seed, samples(frames))
            out[f"{tag}{i}_clipsum"] = np.array([clip.astype(np.float64).sum(), (clip.astype(np.float64) ** 2).sum()])
            x = mx.array(clip * 32768.0)                                  # model.py:231 on a float32 clip
            window = rm.hamming(cfg.win_len, periodic=False)
            mx.random.reseed(NOISE_SEED + seed)
            wave = np.asarray(model._process_chunk(x, window, clip.shape[0]), dtype=np.float32)
            mx.random.reseed(NOISE_SEED + seed)
            feats = features(model, x)
            mask_ref = np.asarray(model.model(feats)[-1][0])
            mask, st = stepped(net, feats)
            mask = np.asarray(mask)[0]
            assert np.array_equal(mask, mask_ref), "the stepped path is not the reference's forward"
            T = feats.shape[1]
            assert T == frames and wave.shape == clip.shape
            wave = wave / np.float32(32768.0)
            e = st.pop("energy")
            meta["configs"][tag]["energy"].append(e)
            diff, peak = float(np.abs(wave - clip).max()), float(np.abs(wave).max())
            print(tag, i, frames, "frames; quad / lin share of A", round(e["quad"], 3), round(e["lin"], 3), "mask zeros", float((mask == 0).mean()),
                  "peak", peak, "max |out - in|", diff)
            stages = dict(feats=np.asarray(feats)[0], flash0=st["flash0"][0], fsmn0=st["fsmn0"][0], mask=mask)
            for k, v in stages.items():
                assert np.isfinite(v).all() and 1e-2 <= float(v.std()) <= 1e2, (tag, i, k, float(v.std()))
            if T > STRIDE_ABOVE:   # (one or two frames: a column the ReLU zeroes in both is constant)
                assert (mask.max(axis=0) > mask.min(axis=0)).all(), "a mask column is constant over time"
            assert (mask == 0).any() and (mask > 0).any()
            if T >= 58:
                assert e["quad"] >= 0.1 and e["lin"] >= 0.1, e
            assert diff > 0.1 * peak, (diff, peak)
            out[f"{tag}{i}_feats"] = stages["feats"] if T <= FEAT_FULL else strided(stages["feats"], T)
            out[f"{tag}{i}_flash0"], out[f"{tag}{i}_fsmn0"] = strided(stages["flash0"], T), strided(stages["fsmn0"], T)
            out[f"{tag}{i}_mask"] = strided(mask, T)[:, ::MASK_COL_STRIDE] if T > STRIDE_ABOVE else mask
            out[f"{tag}{i}_wave"] = wave[::WAVE_STRIDE] if T > STRIDE_ABOVE else wave
    # the two long-audio paths, decode lengths scaled down
    model, cfg, w = build(rm, CONFIGS["A"]["kw"], LONG)
    seed, n = LONG_CLIP
    clip = R.synth_clip(seed, n)
    out["long_clipsum"] = np.array([clip.astype(np.float64).sum(), (clip.astype(np.float64) ** 2).sum()])
    mx.random.reseed(NOISE_SEED + seed)
    seg = np.asarray(model.enhance(clip, chunked=False), dtype=np.float64)
    mx.random.reseed(NOISE_SEED + seed)
    chk = np.asarray(model.enhance(clip), dtype=np.float64)                  # 2.3 s >= auto_chunk_threshold: _decode_chunked
    assert seg.shape == chk.shape == clip.shape and np.isfinite(seg).all() and np.isfinite(chk).all()
    assert not np.array_equal(seg, chk) and np.abs(seg - clip).max() > 0.1 * np.abs(seg).max()
    out["long_segmented"], out["long_chunked"] = seg[::WAVE_STRIDE].astype(np.float32), chk[::WAVE_STRIDE].astype(np.float32)
    meta["long"] = dict(config=LONG, clip=list(LONG_CLIP))
    path = os.path.join(HERE, "ref_mossformer2.npz")
    np.savez_compressed(path, **out)
    with open(os.path.join(HERE, "ref_mossformer2.json"), "w") as f:
        json.dump(meta, f)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= 1_000_000


def _param(model, name):
    obj = model
    for p in name.split("."):
        obj = obj[int(p)] if isinstance(obj, (list, tuple)) else getattr(obj, p)
    return np.asarray(obj)


if __name__ == "__main__":
    main()
