"""DeepFilterNet2 / 3 restated in float64 (numpy + torch.float64 convolutions), straight from the PyTorch-named checkpoint: TEST INFRASTRUCTURE for
batches and for sizes ``tests/golden/ref_dfn.npz`` does not hold.  It follows the reference file by file (model.py: framing, features; network.py:
Encoder, ErbDecoder, DfDecoder, DeepFilterOp, DfNet) in the reference's own NCHW layout, and is itself held to the reference's runs by
``tests/test_dfn_cpu.py``.  ``synth_clip`` is the seeded clip generator the fixtures were made with."""
import math

import numpy as np
import torch
import torch.nn.functional as Fn

import _gru_ref

F64 = torch.float64


def synth_clip(seed: int, n: int, sr: int = 48000, zero_span=None, amp: float = 0.12) -> np.ndarray:
    """Speech-band noise (a one-pole low-pass of white noise under a slow envelope) plus three tones, float32; ``zero_span`` = (start, stop) samples of
    exact zeros."""
    rng = np.random.default_rng(seed)
    white = rng.standard_normal(n)
    lp = np.empty(n)
    acc = 0.0
    for i in range(n):
        acc = 0.93 * acc + 0.07 * white[i]
        lp[i] = acc
    t = np.arange(n) / sr
    env = 0.6 + 0.4 * np.sin(2 * np.pi * 3.1 * t + rng.uniform(0, 6.28))
    tones = sum(a * np.sin(2 * np.pi * f * t + rng.uniform(0, 6.28)) for a, f in ((0.5, 220.0), (0.3, 1370.0), (0.15, 5200.0)))
    x = amp * (3.0 * lp * env + 0.4 * tones + 0.05 * white)
    if zero_span is not None:
        x[zero_span[0]:zero_span[1]] = 0.0
    return x.astype(np.float32)


def vorbis_window(size):
    n = np.arange(size, dtype=np.float32)
    inner = np.sin(0.5 * np.pi * (n + 0.5) / (size // 2))
    return np.sin(0.5 * np.pi * inner * inner).astype(np.float32).astype(np.float64)


def norm_alpha(hop, sr):
    a_raw, precision, a = math.exp(-hop / sr), 3, 1.0
    while a >= 1.0:
        a = round(a_raw, precision)
        precision += 1
    return a


def _t(w, name):
    return torch.as_tensor(np.asarray(w[name]), dtype=F64)


def _bn(w, prefix, x):
    g, b, m, v = (_t(w, f"{prefix}.{n}") for n in ("weight", "bias", "running_mean", "running_var"))
    sh = (1, -1, 1, 1)
    return (x - m.view(sh)) / torch.sqrt(v.view(sh) + 1e-5) * g.view(sh) + b.view(sh)


def _conv(w, name, x, groups, fstride=1):
    wt = _t(w, name + ".weight")
    kt, kf = wt.shape[2], wt.shape[3]
    return Fn.conv2d(Fn.pad(x, (kf // 2, kf // 2, kt - 1, 0)), wt, stride=(1, fstride), groups=groups)


def _convt(w, name, x, groups, fstride):
    wt = _t(w, name + ".weight")
    kt, kf = wt.shape[2], wt.shape[3]
    return Fn.conv_transpose2d(x, wt, stride=(1, fstride), padding=(kt - 1, kf // 2), output_padding=(0, kf // 2), groups=groups)


def _glin(w, name, x):
    wt = _t(w, name)                                   # [G, ws, hs]
    G, ws, _ = wt.shape
    return torch.einsum("btgi,gih->btgh", x.reshape(x.shape[0], x.shape[1], G, ws), wt).reshape(x.shape[0], x.shape[1], -1)


def _squeezed_gru(w, prefix, x, layers, has_out, round_wh):
    x = torch.relu(_glin(w, f"{prefix}.linear_in.0.weight", x))
    for l in range(layers):
        wih, whh = _t(w, f"{prefix}.gru.weight_ih_l{l}"), _t(w, f"{prefix}.gru.weight_hh_l{l}")
        bih, bhh = _t(w, f"{prefix}.gru.bias_ih_l{l}"), _t(w, f"{prefix}.gru.bias_hh_l{l}")
        H = whh.shape[1]
        if round_wh is not None:
            whh = round_wh(whh)
        b = bih + torch.cat([bhh[:2 * H], torch.zeros(H, dtype=F64)])
        out, _ = _gru_ref.gru_seq((x @ wih.T + b).numpy(), whh.numpy(), bhh[2 * H:].numpy())
        x = torch.from_numpy(out)
    if has_out:
        x = torch.relu(_glin(w, f"{prefix}.linear_out.0.weight", x))
    return x


def dfnet(cfg, w, spec, feat_erb, feat_df, round_wh=None):
    """``DfNet.__call__`` on ONE item: spec [T, F] complex (times wnorm), feat_erb [T, E], feat_df [T, D] complex -> dict of stage tensors (numpy)."""
    C, O = cfg.conv_ch, cfg.df_order
    T = spec.shape[0]

    def look(x):   # DfNet._apply_lookahead on the time axis 2
        la = cfg.conv_lookahead
        if la <= 0 or x.shape[2] <= la:
            return x
        return torch.cat([x[:, :, la:], torch.zeros_like(x[:, :, :la])], 2)

    fe = look(torch.as_tensor(feat_erb, dtype=F64)[None, None])                                          # [1, 1, T, E]
    fs = look(torch.stack([torch.as_tensor(feat_df.real, dtype=F64), torch.as_tensor(feat_df.imag, dtype=F64)])[None])   # [1, 2, T, D]

    def block(name, x, i_conv, groups, fstride=1, pw=True):
        y = _conv(w, f"{name}.{i_conv}", x, groups, fstride)
        if pw:
            y = Fn.conv2d(y, _t(w, f"{name}.{i_conv + 1}.weight"))
        return torch.relu(_bn(w, f"{name}.{i_conv + (2 if pw else 1)}", y))

    e0 = block("enc.erb_conv0", fe, 1, 1, pw=False)
    e1 = block("enc.erb_conv1", e0, 0, C, 2)
    e2 = block("enc.erb_conv2", e1, 0, C, 2)
    e3 = block("enc.erb_conv3", e2, 0, C, 1)
    c0 = block("enc.df_conv0", fs, 1, math.gcd(2, C))
    c1 = block("enc.df_conv1", c0, 0, C, 2)
    flat = lambda x: x.permute(0, 2, 3, 1).reshape(1, T, -1)
    cemb = torch.relu(_glin(w, "enc.df_fc_emb.0.weight", flat(c1)))
    emb = torch.cat([flat(e3), cemb], -1) if cfg.enc_concat else flat(e3) + cemb
    emb = _squeezed_gru(w, "enc.emb_gru", emb, 1, not cfg.enc_concat, round_wh)
    lsnr = torch.sigmoid(emb @ _t(w, "enc.lsnr_fc.0.weight").T + _t(w, "enc.lsnr_fc.0.bias")) * (cfg.lsnr_max - cfg.lsnr_min) + cfg.lsnr_min

    def pathway(i, x):
        return torch.relu(_bn(w, f"erb_dec.conv{i}p.1", _conv(w, f"erb_dec.conv{i}p.0", x, C)))

    def up(name, x, transposed):
        y = _convt(w, name + ".0", x, C, 2) if transposed else _conv(w, name + ".0", x, C)
        return torch.relu(_bn(w, name + ".2", Fn.conv2d(y, _t(w, name + ".1.weight"))))

    f8 = e3.shape[3]
    demb = _squeezed_gru(w, "erb_dec.emb_gru", emb, max(1, cfg.emb_num_layers - 1), True, round_wh).reshape(1, T, f8, -1).permute(0, 3, 1, 2)
    d3 = up("erb_dec.convt3", pathway(3, e3) + demb, False)
    d2 = up("erb_dec.convt2", pathway(2, e2) + d3, True)
    d1 = up("erb_dec.convt1", pathway(1, e1) + d2, True)
    m = torch.sigmoid(_bn(w, "erb_dec.conv0_out.1", _conv(w, "erb_dec.conv0_out.0", pathway(0, e0) + d1, 1)))[0, 0]      # [T, E]

    c = _squeezed_gru(w, "df_dec.df_gru", emb, cfg.df_num_layers, False, round_wh)
    if cfg.df_gru_skip == "groupedlinear":
        c = c + _glin(w, "df_dec.df_skip.weight", emb)
    c0p = _conv(w, "df_dec.df_convp.1", c0, math.gcd(C, 2 * O))
    c0p = torch.relu(_bn(w, "df_dec.df_convp.3", Fn.conv2d(c0p, _t(w, "df_dec.df_convp.2.weight")))).permute(0, 2, 3, 1)     # [1, T, D, 2 O]
    coef = (torch.tanh(_glin(w, "df_dec.df_out.0.weight", c)).reshape(1, T, cfg.nb_df, 2 * O) + c0p)[0].reshape(T, cfg.nb_df, O, 2)
    coef_c = torch.complex(coef[..., 0], coef[..., 1])                                                                      # [T, D, O]

    s = torch.as_tensor(spec, dtype=torch.complex128)
    masked = s * (m @ _t(w, "mask.erb_inv_fb"))
    src = (masked if cfg.enc_concat else s)[:, :cfg.nb_df]
    left = O - 1 - cfg.df_lookahead
    pad = torch.cat([torch.zeros(left, cfg.nb_df, dtype=src.dtype), src, torch.zeros(cfg.df_lookahead, cfg.nb_df, dtype=src.dtype)])
    df = sum(pad[k:k + T] * coef_c[:, :, k] for k in range(O))
    spec_e = torch.cat([df, masked[:, cfg.nb_df:]], 1)
    return dict(feat_erb=fe[0, 0].numpy(), feat_df=fs[0].permute(1, 2, 0).numpy(), e0=e0[0].permute(1, 2, 0).numpy(), c0=c0[0].permute(1, 2, 0).numpy(),
                emb=emb[0].numpy(), m=m.numpy(), lsnr=lsnr[0].numpy(), df_coefs=coef.numpy(), spec_e=spec_e.numpy())


def features(cfg, w, x):
    """model.py:284-323: framing, STFT, wnorm, ERB / DF features of ONE clip -> (spec [T, F] complex, feat_erb [T, E], feat_df [T, D] complex)."""
    n_fft, hop = cfg.fft_size, cfg.hop_size
    wnorm = 1.0 / (n_fft * n_fft / (2.0 * hop))
    xp = np.concatenate([np.zeros(hop), np.asarray(x, dtype=np.float64), np.zeros(n_fft)])
    T = 1 + (xp.shape[0] - n_fft) // hop
    idx = np.arange(T)[:, None] * hop + np.arange(n_fft)[None, :]
    spec = np.fft.rfft(xp[idx] * vorbis_window(n_fft), axis=-1) * wnorm
    mag2 = spec.real ** 2 + spec.imag ** 2
    if "erb_fb" in w:
        erb = mag2 @ np.asarray(w["erb_fb"], dtype=np.float64)
    else:
        st = np.concatenate([[0], np.cumsum(cfg.erb_widths)])
        erb = np.stack([mag2[:, st[i]:st[i + 1]].mean(1) for i in range(cfg.nb_erb)], 1)
    db = 10.0 * np.log10(erb + 1e-10)
    alpha = norm_alpha(hop, cfg.sample_rate)
    a, oma = float(np.float32(alpha)), float(np.float32(1.0 - alpha))
    se, sd = np.linspace(-60.0, -90.0, cfg.nb_erb), np.linspace(0.001, 0.0001, cfg.nb_df)
    fe, fd = np.empty_like(db), np.empty((T, cfg.nb_df), dtype=np.complex128)
    mag = np.abs(spec[:, :cfg.nb_df])
    for t in range(T):
        se = db[t] * oma + se * a
        fe[t] = (db[t] - se) / 40.0
        sd = mag[t] * oma + sd * a
        fd[t] = spec[t, :cfg.nb_df] / np.sqrt(sd)
    return spec, fe, fd


def enhance(cfg, w, x, round_wh=None):
    """``DeepFilterNetModel.enhance_array`` on one clip -> (waveform float64 [L], stages)."""
    n_fft, hop = cfg.fft_size, cfg.hop_size
    wnorm = 1.0 / (n_fft * n_fft / (2.0 * hop))
    spec, fe, fd = features(cfg, w, x)
    st = dfnet(cfg, w, spec, fe, fd, round_wh)
    T, L = spec.shape[0], len(x)
    win = vorbis_window(n_fft)
    frames = np.fft.irfft(st["spec_e"] / wnorm, n=n_fft, axis=-1) * win
    y, env = np.zeros((T - 1) * hop + n_fft), np.zeros((T - 1) * hop + n_fft)
    for t in range(T):
        y[t * hop:t * hop + n_fft] += frames[t]
        env[t * hop:t * hop + n_fft] += win * win
    y = np.where(env > 1e-10, y / np.where(env > 1e-10, env, 1.0), y)
    d = n_fft - hop
    return np.clip(y[d:d + L], -1.0, 1.0), st
