"""TEST INFRASTRUCTURE: Mel-Band RoFormer restated in float64 numpy from the reference's ``sts/models/mel_roformer/model.py`` (line numbers below)
and ``dsp.py`` (stft 385-433, istft 436-513).  Independent of the engine's host schedule: it follows the reference's own tensor layouts
([B, 2 F, T, 2] CaC spectra, lists of per-band arrays, transposes between the two attention axes).  Weights come under the reference's parameter
names (``mel_roformer.expected_shapes``).  Not a fallback: nothing under ``mlx_audio_amd/`` imports it."""
import math

import numpy as np


def synth_clip(seed: int, n: int, zero_head: int = 0) -> np.ndarray:
    """A seeded stereo clip [2, n] in float32: band-limited noise plus two tones per channel, peak about 0.5; the first ``zero_head`` samples exact zeros."""
    r = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)
    x = np.zeros((2, n))
    for ch in range(2):
        noise = np.convolve(r.standard_normal(n + 8), np.hanning(9) / 4.0, mode="valid")
        f1, f2 = r.uniform(0.01, 0.08), r.uniform(0.1, 0.3)
        x[ch] = 0.15 * noise + 0.2 * np.sin(2 * np.pi * f1 * t + r.uniform(0, 6)) + 0.1 * np.sin(2 * np.pi * f2 * t + r.uniform(0, 6))
    x = 0.5 * x / np.abs(x).max()
    x[:, :zero_head] = 0.0
    return x.astype(np.float32)


def band_indices(cfg):
    """MelFilterbank (model.py:63-140) on the package's ``dsp.mel_filters``."""
    from mlx_audio_amd.dsp import mel_filters

    fb = mel_filters(sample_rate=cfg.sample_rate, n_fft=cfg.n_fft, n_mels=cfg.num_bands, mel_scale="slaney").numpy().astype(np.float32)
    fb[0, 0] = 1.0
    fb[-1, -1] = 1.0
    fb = fb > 0
    out = []
    for i in range(cfg.num_bands):
        bins = np.where(fb[i])[0]
        if len(bins) == 0:
            bins = np.array([i])
        cac = []
        for b in bins:
            cac.extend([b * 2, b * 2 + 1])
        out.append(np.array(cac, dtype=np.int64))
    return out


def window(cfg):
    return np.hanning(cfg.n_fft + 1)[:-1].astype(np.float32).astype(np.float64)   # model.py:585: a float32 window


def stft(x, n_fft, hop, w):
    """dsp.py:411-433, center=True, reflect."""
    p = n_fft // 2
    xp = np.concatenate([x[1:p + 1][::-1], x, x[-(p + 1):-1][::-1]])
    T = 1 + (len(xp) - n_fft) // hop
    idx = np.arange(T)[:, None] * hop + np.arange(n_fft)[None, :]
    return np.fft.rfft(xp[idx] * w, axis=-1)                                     # [T, F]


def istft(spec, n_fft, hop, w):
    """dsp.py:479-508 with center=True, length=None, normalized=True; spec [F, T]."""
    T = spec.shape[1]
    total = (T - 1) * hop + n_fft
    fr = np.fft.irfft(spec, n=n_fft, axis=0).T * w
    y, ws = np.zeros(total), np.zeros(total)
    for t in range(T):
        y[t * hop:t * hop + n_fft] += fr[t]
        ws[t * hop:t * hop + n_fft] += w * w
    y = np.where(ws > 1e-10, y / np.where(ws > 1e-10, ws, 1.0), y)
    return y[n_fft // 2:-(n_fft // 2)]


def rmsnorm(x, g):
    """model.py:40-42."""
    n = np.sqrt((x * x).sum(-1, keepdims=True))
    return x / np.maximum(n, 1e-12) * math.sqrt(x.shape[-1]) * g


def _sigmoid(v):
    return 1.0 / (1.0 + np.exp(-v))


def _gelu(v):
    import torch

    return 0.5 * v * (1.0 + torch.erf(torch.from_numpy(np.ascontiguousarray(v / math.sqrt(2.0)))).numpy())   # nn.gelu: the exact (erf) form


def rope(x, dh):
    """model.py:165-196: interleaved pairs, angles position * 10000^(-i / half) in float32 like the reference's tables."""
    L, half = x.shape[-2], dh // 2
    freqs = (1.0 / (10000.0 ** (np.arange(0, half, dtype=np.float32) / half))).astype(np.float32)
    ang = np.repeat((np.arange(L, dtype=np.float32)[:, None] * freqs[None, :]).astype(np.float32), 2, axis=-1)
    cos, sin = np.cos(ang).astype(np.float32).astype(np.float64), np.sin(ang).astype(np.float32).astype(np.float64)
    pairs = x.reshape(*x.shape[:-1], half, 2)
    rot = np.stack([-pairs[..., 1], pairs[..., 0]], axis=-1).reshape(x.shape)
    return x * cos + rot * sin


def attention(x, w, p, heads, dh):
    """RoFormerAttention (model.py:219-243); x [N, L, D]."""
    N, L, _ = x.shape
    h = rmsnorm(x, w[p + "norm.weight"])
    sp = lambda m: (h @ w[p + m + ".weight"].T).reshape(N, L, heads, dh).transpose(0, 2, 1, 3)
    q, k, v = rope(sp("to_q"), dh), rope(sp("to_k"), dh), sp("to_v")
    s = (q @ k.transpose(0, 1, 3, 2)) / math.sqrt(dh)
    s = np.exp(s - s.max(-1, keepdims=True))
    a = (s / s.sum(-1, keepdims=True)) @ v
    gates = _sigmoid(h @ w[p + "to_gates.weight"].T + w[p + "to_gates.bias"])    # [N, L, heads]
    a = a * gates.transpose(0, 2, 1)[..., None]
    return a.transpose(0, 2, 1, 3).reshape(N, L, heads * dh) @ w[p + "to_out.weight"].T


def ffn(x, w, p):
    """RoFormerFFN (model.py:267-272)."""
    h = rmsnorm(x, w[p + "0.weight"])
    h = _gelu(h @ w[p + "1.weight"].T + w[p + "1.bias"])
    return h @ w[p + "4.weight"].T + w[p + "4.bias"]


def transformer(x, w, p, heads, dh):
    """Transformer with depth 1 (model.py:289-293)."""
    x = attention(x, w, p + "layers.0.0.", heads, dh) + x
    x = ffn(x, w, p + "layers.0.1.net.") + x
    return rmsnorm(x, w[p + "norm.weight"])


def band_split(rep, idx, w):
    """BandSplit.split (model.py:310-336); rep [B, 2 F, T, 2] -> [B, T, Nb, D]."""
    B, _, T, _ = rep.shape
    bands = []
    for n, ix in enumerate(idx):
        u = rep[:, ix].transpose(0, 2, 1, 3).reshape(B, T, 2 * len(ix))
        p = f"band_split.to_features.{n}."
        bands.append(rmsnorm(u, w[p + "0.weight"]) @ w[p + "1.weight"].T + w[p + "1.bias"])
    return np.stack(bands, axis=2)


def mask_estimate(x, w, n_bands, depth):
    """MaskEstimator (model.py:400-425): per band tanh MLP, then GLU."""
    masks = []
    for n in range(n_bands):
        h = x[:, :, n]
        p = f"mask_estimators.0.to_freqs.{n}."
        for i in range(depth):
            h = np.tanh(h @ w[f"{p}{i}.0.weight"].T + w[f"{p}{i}.0.bias"])
        h = h @ w[f"{p}{depth}.0.weight"].T + w[f"{p}{depth}.0.bias"]
        half = h.shape[-1] // 2
        masks.append(h[..., :half] * _sigmoid(h[..., half:]))
    return masks


def band_merge(masks, idx, n_cac):
    """BandSplit.merge (model.py:338-368): scatter-add in band order, divided by max(count, 1)."""
    B, T = masks[0].shape[:2]
    out, cnt = np.zeros((B, n_cac, T, 2)), np.zeros(n_cac)
    for ix, m in zip(idx, masks):
        mr = m.reshape(B, T, len(ix), 2).transpose(0, 2, 1, 3)
        for j, i in enumerate(ix):
            out[:, i] += mr[:, j]
            cnt[i] += 1
    return out / np.maximum(cnt, 1.0)[None, :, None, None]


def forward(cfg, weights, audio, idx=None):
    """MelRoFormer.__call__ (model.py:572-646): audio [B, 2, S] -> (vocals [B, 2, S], stages)."""
    w = {k: np.asarray(v, dtype=np.float64) for k, v in weights.items()}
    audio = np.asarray(audio, dtype=np.float64)
    B, C, S = audio.shape
    idx = band_indices(cfg) if idx is None else idx
    win = window(cfg)
    spec = np.stack([np.stack([stft(audio[b, c], cfg.n_fft, cfg.hop_length, win).T for c in range(C)]) for b in range(B)])   # [B, 2, F, T]
    F, T = spec.shape[2], spec.shape[3]
    inter = spec.transpose(0, 2, 1, 3).reshape(B, 2 * F, T)                      # CaC interleave (model.py:593-598)
    rep = np.stack([inter.real, inter.imag], axis=-1)
    x = band_split(rep, idx, w)
    st = dict(split=x, tf=[])
    Nb, D = x.shape[2], x.shape[3]
    for lv in range(cfg.depth):
        tin = x.transpose(0, 2, 1, 3).reshape(B * Nb, T, D)
        x = transformer(tin, w, f"layers.{lv}.0.", cfg.heads, cfg.dim_head).reshape(B, Nb, T, D).transpose(0, 2, 1, 3)
        if lv == 0:
            st["tf"].append(x)
        x = transformer(x.reshape(B * T, Nb, D), w, f"layers.{lv}.1.", cfg.heads, cfg.dim_head).reshape(B, T, Nb, D)
        if lv == 0:
            st["tf"].append(x)
    mask = band_merge(mask_estimate(x, w, Nb, cfg.mask_estimator_depth), idx, 2 * F)
    st["mask"] = mask
    out_re = rep[..., 0] * mask[..., 0] - rep[..., 1] * mask[..., 1]
    out_im = rep[..., 0] * mask[..., 1] + rep[..., 1] * mask[..., 0]
    o = (out_re + 1j * out_im).reshape(B, F, 2, T).transpose(0, 2, 1, 3)         # de-interleave (model.py:632-634)
    y = np.zeros((B, C, S))
    for b in range(B):
        for c in range(C):
            r = istft(o[b, c], cfg.n_fft, cfg.hop_length, win)[:S]
            y[b, c, :len(r)] = r
    return y, st
