#!/usr/bin/env python
"""Runs the reference's OWN ``sts/models/deepfilternet/config.py``, ``network.py``, ``weight_loader.py`` and ``model.py``, unmodified and imported from
where they lie, over the numpy stand-in for MLX (``mlx_shim.py``, left as it is) on seeded checkpoints and stores what they compute in
``tests/golden/ref_dfn.npz`` / ``ref_dfn.json``.

The stand-in lacks ``nn.GRU``, ``mx.conv2d``, ``mx.conv_transpose2d``, ``nn.ReLU``, ``nn.Sigmoid``, ``Module.parameters`` and a working
``mlx.utils.tree_flatten``: added here at run time (the convs through ``torch.nn.functional`` on the MLX layouts, the GRU as a float32 numpy loop with
MLX ``nn.GRU`` semantics).  ``model.py`` imports the hub client and the package's audio I/O at module level; neither is on the ``enhance_array`` path
and each gets an empty stand-in module.

Before anything is written the stand-in GRU is checked against two witnesses on the same weights: the reference's own ``PyTorchGRU`` (network.py:37-150,
full ``bias_hh``) against the folded-bias form its loader produces, and ``torch.nn.GRU``.

  * config ``A``: DeepFilterNet3 at the published sizes (fft 960 / hop 480, 32 ERB bands, 96 DF bins, order 5, 16 channels, hidden 256,
    ``conv_lookahead = df_lookahead = 2``, ``enc_concat = False``);
  * config ``B``: DeepFilterNet2-like and small (``enc_concat = True``, look-ahead 0, hidden 64, 16 bands, 48 bins, 8 channels, fft 480 / hop 240);
    its group counts divide, asserted below.
Clips come from seeds (``tests/_dfn_ref.synth_clip``: speech-band noise plus tones) and are NOT stored, only their float64 sum and sum of squares:
0.2 - 0.7 s, one with 10 frames of exact zeros inside, one of 700 samples (3 frames: one more than the look-ahead, a single frame survives the
shift) and one shorter than a hop (the reference's framing -- one hop of zeros in front, ``fft_size`` behind -- gives every clip at least 2 frames:
that one has 2, no more than the look-ahead, so the shift is skipped).
Per clip: ``feat_erb`` and ``feat_df`` as the network receives them behind the reference's own ``DfNet._apply_lookahead``, ``emb``, ``m``, ``lsnr``,
``df_coefs`` (every third frame for clips of more than 40 frames: the file's size) and the enhanced waveform of ``enhance_array``.

Asserted before writing: the stepped path (features -> ``DfNet`` -> inverse STFT) reproduces ``enhance_array`` bit for bit; every enhanced clip's
peak lies in [1e-3, 0.9], so the final clip never engages; no stored tensor is constant.

Only runs where the reference lies: ``python tests/golden/make_dfn_fixtures.py``."""
import json
import math
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_reference_fixtures as M  # noqa: E402  (installs the stand-in)
import _dfn_ref as R  # noqa: E402

mx, nn, _np = M.mx, M.nn, M._np
SEED_W = 7
COEF_STRIDE_ABOVE, COEF_STRIDE = 40, 3

CONFIGS = {
    "A": dict(cls="DeepFilterNet3Config", kw=dict(conv_lookahead=2, df_lookahead=2),
              clips=[(11, 9600, None), (12, 19200, (7200, 12000)), (13, 33600, None), (14, 700, None), (15, 200, None)]),
    "B": dict(cls="DeepFilterNet2Config", kw=dict(enc_concat=True, fft_size=480, hop_size=240, nb_erb=16, nb_df=48, conv_ch=8, emb_hidden_dim=64, df_hidden_dim=64,
                                                  linear_groups=8, enc_linear_groups=8),
              clips=[(21, 9600, None), (22, 16800, None)]),
}


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x), dtype=np.float32))


def conv2d(x, w, stride=1, padding=0, dilation=1, groups=1, stream=None):
    """``mx.conv2d``: input [N, H, W, C], weight [O, kh, kw, I / groups]."""
    y = torch.nn.functional.conv2d(_t(x).permute(0, 3, 1, 2), _t(w).permute(0, 3, 1, 2), None, stride=stride, padding=padding, dilation=dilation, groups=groups)
    return mx.array(y.permute(0, 2, 3, 1).contiguous().numpy())


def conv_transpose2d(x, w, stride=1, padding=0, dilation=1, output_padding=0, groups=1, stream=None):
    """``mx.conv_transpose2d``: input [N, H, W, C], weight [O, kh, kw, I] (groups = 1 only, like MLX)."""
    assert groups == 1
    y = torch.nn.functional.conv_transpose2d(_t(x).permute(0, 3, 1, 2), _t(w).permute(3, 0, 1, 2), None, stride=stride, padding=padding,
                                             output_padding=output_padding, dilation=dilation)
    return mx.array(y.permute(0, 2, 3, 1).contiguous().numpy())


def _sig(v):
    return 1.0 / (1.0 + np.exp(-v))


class GRU(nn.Module):
    """``mlx.nn.GRU``: batch-first [B, T, In] (or [T, In]) input, ``b`` [3H] on the input side, ``bhn`` [H] on the n gate's recurrent side only."""

    def __init__(self, input_size, hidden_size, bias=True):
        super().__init__()
        s = 1.0 / math.sqrt(hidden_size)
        self.hidden_size = hidden_size
        self.Wx = mx.random.uniform(-s, s, (3 * hidden_size, input_size))
        self.Wh = mx.random.uniform(-s, s, (3 * hidden_size, hidden_size))
        self.b = mx.random.uniform(-s, s, (3 * hidden_size,)) if bias else None
        self.bhn = mx.random.uniform(-s, s, (hidden_size,)) if bias else None

    def __call__(self, x, hidden=None):
        H = self.hidden_size
        x = np.asarray(x, dtype=np.float32)
        xp = x @ np.asarray(self.Wx, dtype=np.float32).T
        if self.b is not None:
            xp = xp + np.asarray(self.b, dtype=np.float32)
        wh = np.asarray(self.Wh, dtype=np.float32)
        bhn = np.asarray(self.bhn, dtype=np.float32) if self.bhn is not None else np.float32(0)
        h = None if hidden is None else np.asarray(hidden, dtype=np.float32)
        out = []
        for t in range(xp.shape[-2]):
            xt = xp[..., t, :]
            hp = np.zeros_like(xt) if h is None else h @ wh.T
            r, z = _sig(xt[..., :H] + hp[..., :H]), _sig(xt[..., H:2 * H] + hp[..., H:2 * H])
            n = np.tanh(xt[..., 2 * H:] + r * (hp[..., 2 * H:] + bhn))
            h = ((1 - z) * n + (z * h if h is not None else 0)).astype(np.float32)
            out.append(h)
        return mx.array(np.stack(out, axis=-2))


class ReLU(nn.Module):
    def __call__(self, x):
        return nn.relu(x)


class Sigmoid(nn.Module):
    def __call__(self, x):
        return mx.sigmoid(x)


def _parameters(self):
    """``Module.parameters()``: the nested dict of arrays, through Module, dict and list children."""
    def walk(v):
        if isinstance(v, nn.Module):
            d = {k: walk(c) for k, c in v.__dict__.items() if not k.startswith("_")}
            return {k: c for k, c in d.items() if c is not None}
        if isinstance(v, mx.array):
            return v
        if isinstance(v, dict):
            d = {k: walk(c) for k, c in v.items()}
            return {k: c for k, c in d.items() if c is not None} or None
        if isinstance(v, (list, tuple)):
            lst = [walk(c) for c in v]
            return lst if any(c is not None for c in lst) else None
        return None
    return walk(self)


def _tree_flatten(tree, prefix=""):
    out = []
    if isinstance(tree, dict):
        for k, v in tree.items():
            out += _tree_flatten(v, f"{prefix}{k}.")
    elif isinstance(tree, (list, tuple)):
        for i, v in enumerate(tree):
            out += _tree_flatten(v, f"{prefix}{i}.")
    elif tree is not None:
        out.append((prefix[:-1], tree))
    return out


def load_reference():
    for name, obj in (("GRU", GRU), ("ReLU", ReLU), ("Sigmoid", Sigmoid)):
        if not hasattr(nn, name):
            setattr(nn, name, obj)
    for name, obj in (("conv2d", conv2d), ("conv_transpose2d", conv_transpose2d)):
        if not hasattr(mx, name):
            setattr(mx, name, obj)
    if not hasattr(nn.Module, "parameters"):
        nn.Module.parameters = _parameters
    sys.modules["mlx.utils"].tree_flatten = _tree_flatten
    M.import_reference()
    for name, attrs in (("huggingface_hub", ("hf_hub_download", "snapshot_download")), ("mlx_audio.audio_io", ("read", "write"))):
        if name not in sys.modules:
            mod = types.ModuleType(name)
            for a in attrs:
                setattr(mod, a, None)
            sys.modules[name] = mod
    sys.modules["mlx_audio"].audio_io = sys.modules["mlx_audio.audio_io"]
    for pkg, path in (("mlx_audio.sts", "sts"), ("mlx_audio.sts.models", "sts/models"), ("mlx_audio.sts.models.deepfilternet", "sts/models/deepfilternet")):
        if pkg not in sys.modules:
            M._pkg(pkg, f"{M.REF}/{path}")
    base = f"{M.REF}/sts/models/deepfilternet"
    return {name: M._load(f"mlx_audio.sts.models.deepfilternet.{name}", f"{base}/{name}.py") for name in ("config", "network", "network_df1", "weight_loader", "model")}


def check_gru(ref):
    """The stand-in GRU against the reference's PyTorchGRU (full bias_hh) and torch.nn.GRU, same weights, the r / z parts of bias_hh folded into b."""
    for H, In, T in ((64, 48, 9), (256, 256, 6)):
        tg = torch.nn.GRU(In, H, batch_first=True)
        g = torch.Generator().manual_seed(H)
        x = torch.randn(2, T, In, generator=g)
        with torch.no_grad():
            want = tg(x, torch.zeros(1, 2, H))[0].numpy()
        wih, whh, bih, bhh = (p.detach().numpy() for p in (tg.weight_ih_l0, tg.weight_hh_l0, tg.bias_ih_l0, tg.bias_hh_l0))
        pt = ref["network"].PyTorchGRU(In, H)
        pt.Wx, pt.Wh, pt.b, pt.bhn = mx.array(wih), mx.array(whh), mx.array(bih), mx.array(bhh)
        full = np.asarray(pt(mx.array(x.numpy().transpose(1, 0, 2)))).transpose(1, 0, 2)
        mine = GRU(In, H)
        mine.Wx, mine.Wh = mx.array(wih), mx.array(whh)
        mine.b = mx.array(bih + np.concatenate([bhh[:2 * H], np.zeros(H, dtype=np.float32)]))
        mine.bhn = mx.array(bhh[2 * H:])
        got = np.asarray(mine(mx.array(x.numpy()), mx.zeros((2, H))))
        e1, e2 = float(np.abs(got - full).max()), float(np.abs(got - want).max())
        print(f"GRU stand-in H={H}: vs PyTorchGRU {e1:.2e}, vs torch.nn.GRU {e2:.2e}")
        assert e1 < 2e-6 and e2 < 2e-6, (e1, e2)


def build(ref, tag):
    from mlx_audio_amd.sts.models.deepfilternet import make_dfn_weights
    from mlx_audio_amd.sts.models.deepfilternet import config as my_config

    c = CONFIGS[tag]
    cfg = getattr(ref["config"], c["cls"])(**c["kw"])
    mine = getattr(my_config, c["cls"])(**c["kw"])
    assert cfg.to_dict() == mine.to_dict()
    p = cfg
    for n, g in ((p.conv_ch * p.nb_df // 2, p.enc_linear_groups), (p.conv_ch * p.nb_erb // 4, p.enc_linear_groups), (p.conv_ch * p.nb_erb // 4, p.linear_groups),
                 (p.emb_hidden_dim, p.linear_groups), (p.df_hidden_dim, 8), (p.nb_df * 2 * p.df_order, p.linear_groups), (p.nb_erb, 4), (p.nb_df, 2)):
        assert n % g == 0, (tag, n, g)
    w = make_dfn_weights(mine, SEED_W)
    net = ref["network"].DfNet(cfg)
    loaded = ref["weight_loader"].load_weights(net, {k: mx.array(v.numpy()) for k, v in w.items()})
    assert loaded == len(w), (loaded, len(w))   # every name of the seeded checkpoint found its parameter
    for gru in [g for m_ in (net.enc.emb_gru, net.erb_dec.emb_gru, net.df_dec.df_gru) for g in m_.gru_layers]:
        assert getattr(gru, "_pt_bhn_folded", False) and np.asarray(gru.bhn).shape == (gru.hidden_size,)
    assert np.array_equal(np.asarray(net.erb_fb), w["erb_fb"].numpy()) and np.array_equal(np.asarray(net.mask.erb_inv_fb), w["mask.erb_inv_fb"].numpy())
    return ref["model"].DeepFilterNetModel(cfg, model=net), cfg


def run_clip(ref, model, cfg, x):
    """The reference on ONE clip: ``enhance_array`` itself, then its own steps again (model.py:284-354) so that the stage tensors can be kept."""
    dsp = sys.modules["mlx_audio.dsp"]
    wave = np.asarray(model.enhance_array(x.copy()), dtype=np.float32)
    p = cfg
    xp = mx.pad(mx.array(x.astype(np.float32)), [(p.hop_size, p.fft_size)])
    spec = dsp.stft(xp, n_fft=p.fft_size, hop_length=p.hop_size, win_length=p.fft_size, window=model._vorbis, center=False) * model.wnorm
    alpha = model._norm_alpha()
    erb_db = 10.0 * mx.log10(model._erb(mx.real(spec) ** 2 + mx.imag(spec) ** 2) + 1e-10)
    feat_erb = model._band_mean_norm(erb_db, alpha, p.nb_erb)[None, None, :, :]
    df_re, df_im = model._band_unit_norm(spec[:, :p.nb_df], alpha, p.nb_df)
    feat_df = mx.stack([df_re, df_im], axis=-1)[None, None, :, :, :]
    spec_in = mx.stack([mx.real(spec), mx.imag(spec)], axis=-1)[None, None, :, :, :]
    net = model.model
    spec_e, m, lsnr, df_coefs = net(spec_in, feat_erb, feat_df)
    fe_l = net._apply_lookahead(feat_erb, net.conv_lookahead, time_axis=2)
    fs_l = net._apply_lookahead(mx.transpose(feat_df.squeeze(1), (0, 3, 1, 2)), net.conv_lookahead, time_axis=2)
    emb = net.enc(fe_l, fs_l)[4]
    enh = np.asarray(spec_e)[0, 0]
    y = dsp.istft(mx.transpose(mx.array((enh[..., 0] + 1j * enh[..., 1]).astype(np.complex64)) / model.wnorm, (1, 0)), hop_length=p.hop_size, win_length=p.fft_size,
                  window=model._vorbis, center=False, length=len(x) + p.hop_size + p.fft_size, normalized=True)
    d = p.fft_size - p.hop_size
    stepped = np.clip(np.array(y[d:len(x) + d], dtype=np.float32), -1.0, 1.0)
    assert np.array_equal(stepped, wave), "the stepped path is not enhance_array"
    T = np.asarray(spec).shape[0]
    coefs = np.asarray(df_coefs)[0].transpose(1, 2, 0, 3)                      # [T, D, order, 2]
    return dict(wave=wave, feat_erb=np.asarray(fe_l)[0, 0], feat_df=np.asarray(fs_l)[0].transpose(1, 2, 0), emb=np.asarray(emb)[0], m=np.asarray(m)[0, 0],
                lsnr=np.asarray(lsnr)[0, :, 0], df_coefs=coefs[::COEF_STRIDE] if T > COEF_STRIDE_ABOVE else coefs), T


def main():
    ref = load_reference()
    check_gru(ref)
    out, meta = {}, dict(seed_w=SEED_W, coef_stride_above=COEF_STRIDE_ABOVE, coef_stride=COEF_STRIDE, configs={})
    for tag, c in CONFIGS.items():
        model, cfg = build(ref, tag)
        meta["configs"][tag] = dict(cls=c["cls"], kw=c["kw"], clips=[[s, n, list(z) if z else None] for s, n, z in c["clips"]], frames=[])
        assert abs(model._norm_alpha() - 0.99) < 1e-12 if (cfg.hop_size, cfg.sample_rate) == (480, 48000) else True
        for i, (seed, n, zero) in enumerate(c["clips"]):
            x = R.synth_clip(seed, n, cfg.sample_rate, zero)
            if zero:
                assert (zero[1] - zero[0]) >= 10 * cfg.hop_size and not x[zero[0]:zero[1]].any()
            out[f"{tag}{i}_clipsum"] = np.array([x.astype(np.float64).sum(), (x.astype(np.float64) ** 2).sum()])
            r, T = run_clip(ref, model, cfg, x)
            meta["configs"][tag]["frames"].append(T)
            peak = float(np.abs(r["wave"]).max())
            print(tag, i, n, "samples ->", T, "frames; input peak", float(np.abs(x).max()), "enhanced peak", peak, "m in", float(r["m"].min()), float(r["m"].max()),
                  "lsnr", float(r["lsnr"].min()), float(r["lsnr"].max()))
            assert 1e-3 <= peak <= 0.9, peak
            for k, v in r.items():
                v = np.asarray(v, dtype=np.float32)
                assert v.size == 1 or float(v.max()) > float(v.min()), (tag, i, k)
                out[f"{tag}{i}_{k}"] = v
    path = os.path.join(HERE, "ref_dfn.npz")
    np.savez_compressed(path, **out)
    with open(os.path.join(HERE, "ref_dfn.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= 1_140_000


if __name__ == "__main__":
    main()
