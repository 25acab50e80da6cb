"""TEST INFRASTRUCTURE: the mask estimator of MossFormer2 SE restated in float64 torch, one item at a time, straight from the reference's module tree
(sts/models/mossformer2_se of the reference; nothing here is shared with the engine's host schedule or with ``_ops_emu_mossformer2``):

  MossFormer_MaskNet.__call__    mossformer_masknet.py:122-205     GlobalLayerNorm           globallayernorm.py:55-74
  ScaledSinuEmbedding            scaledsinuembedding.py:58-83      Computation_Block         computation_block.py:71-100
  MossFormerM                    mossformerm.py:72-88              MossFormerBlock_GFSMN     mossformerblock_gfsmn.py:61-63,89-106
  FLASH_ShareA_FFConvM           flash_sharea_ffconvm.py:119-378   FFConvM / ConvModule      ffconvm.py:52-70, convmodule.py:49-69
  ScaleNorm / OffsetScale        scalenorm.py:25-41, offsetscale.py:30-59
  Gated_FSMN_Block / CLayerNorm  gated_fsmn_block.py:38-54,129-160 Gated_FSMN / UniDeepFsmn  gated_fsmn.py:85-116, unideepfsmn.py:73-123
"""
import numpy as np
import torch

P = "model.mossformer."
F64 = torch.float64


def synth_clip(seed: int, n: int) -> np.ndarray:
    """A seeded clip: three tones under a slow envelope plus noise, peak below 0.5."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 48000.0
    x = sum(a * np.sin(2 * np.pi * f * t + p) for a, f, p in zip((0.2, 0.1, 0.05), rng.uniform(100, 4000, 3), rng.uniform(0, 6.28, 3)))
    x = x * (0.6 + 0.4 * np.sin(2 * np.pi * 3.0 * t)) + 0.02 * rng.standard_normal(n)
    return x.astype(np.float32)


def _lin(x, w, name, bias=True):
    wt = w[name + ".weight"].to(F64)
    wt = wt.reshape(wt.shape[0], -1)
    y = x @ wt.T
    return y + w[name + ".bias"].to(F64) if bias else y


def _scalenorm(x, g, eps=1e-8):
    nrm = torch.sqrt((x * x).sum(-1, keepdim=True)) * x.shape[-1] ** -0.5
    return x * (g.to(F64) / torch.clamp(nrm, min=eps))


def _layernorm(x, wt, b, eps):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    y = (x - mu) / torch.sqrt(var + eps)
    return y if wt is None else y * wt.to(F64) + b.to(F64)


def _dw_same(x, wt):
    """Zero-padded depthwise correlation over time: out[t, c] = sum_k x[t + k - pad, c] * wt[c, k] (depthwise_conv1d_kernel.py:38-47)."""
    T, C = x.shape
    K = wt.shape[1]
    pad = (K - 1) // 2
    xp = torch.zeros(T + K - 1, C, dtype=F64)
    xp[pad:pad + T] = x
    out = torch.zeros(T, C, dtype=F64)
    for k in range(K):
        out += xp[k:k + T] * wt[:, k].to(F64)
    return out


def _ffconvm(x, w, p, norm):
    h = _scalenorm(x, w[p + "norm.g"]) if norm == "scale" else _layernorm(x, w[p + "norm.weight"], w[p + "norm.bias"], 1e-5)
    h = torch.nn.functional.silu(_lin(h, w, p + "linear"))
    return h + _dw_same(h, w[p + "conv_module.weight"].reshape(h.shape[1], -1))


def _rope(x):
    """nn.RoPE(dims=32, traditional=False, base=10000) on [T, 128]: the sequence axis is T, the pairs are (i, i + 16)."""
    T = x.shape[0]
    ang = torch.arange(T, dtype=F64)[:, None] * torch.pow(torch.tensor(10000.0, dtype=F64), -torch.arange(16, dtype=F64) / 16)
    c, s = torch.cos(ang), torch.sin(ang)
    a, b = x[:, :16], x[:, 16:32]
    return torch.cat([a * c - b * s, a * s + b * c, x[:, 32:]], dim=1)


def flash(x, w, p, parts=None):
    T, C = x.shape
    s = x.clone()
    s[1:, :C // 2] = x[:-1, :C // 2]
    s[0, :C // 2] = 0
    hidden = _ffconvm(s, w, p + "to_hidden.", "scale")
    v, u = hidden[:, :2 * C], hidden[:, 2 * C:]
    qk = _ffconvm(s, w, p + "to_qk.", "scale")
    heads = qk[:, None, :] * w[p + "qk_offset_scale.gamma"].to(F64) + w[p + "qk_offset_scale.beta"].to(F64)
    quad_q, lin_q, quad_k, lin_k = (_rope(heads[:, h]) for h in range(4))
    g = 256
    pad = (-T) % g
    z = lambda t: torch.cat([t, torch.zeros(pad, t.shape[1], dtype=F64)])
    qq, lq, qk_, lk, vp, up = (z(t).reshape(-1, g, t.shape[1]) for t in (quad_q, lin_q, quad_k, lin_k, v, u))
    attn = torch.clamp(qq @ qk_.transpose(1, 2) / g, min=0) ** 2
    kv, ku = (lk.reshape(-1, 128).T @ vp.reshape(-1, vp.shape[2])) / T, (lk.reshape(-1, 128).T @ up.reshape(-1, up.shape[2])) / T
    quad_v, quad_u = attn @ vp, attn @ up
    lin_v, lin_u = lq @ kv, lq @ ku
    if parts is not None:
        parts["quad"], parts["lin"] = float((quad_v ** 2).sum() + (quad_u ** 2).sum()), float((lin_v ** 2).sum() + (lin_u ** 2).sum())
    att_v = (quad_v + lin_v).reshape(-1, vp.shape[2])[:T]
    att_u = (quad_u + lin_u).reshape(-1, up.shape[2])[:T]
    out = (att_u * v) * torch.sigmoid(att_v * u)
    return x + _ffconvm(out, w, p + "to_out.", "scale")


def fsmn_block(x, w, p):
    prelu = lambda t, a: torch.clamp(t, min=0) + a.to(F64) * torch.clamp(t, max=0)
    h = prelu(_lin(x, w, p + "conv1"), w[p + "prelu.weight"])
    h = _layernorm(h, w[p + "norm1.weight"], w[p + "norm1.bias"], 1e-8)
    gp = p + "gated_fsmn."
    xu = _ffconvm(h, w, gp + "to_u.", "layer")
    xv = _ffconvm(h, w, gp + "to_v.", "layer")
    p1 = _lin(torch.clamp(_lin(xu, w, gp + "fsmn.linear"), min=0), w, gp + "fsmn.project", bias=False)
    mem = p1 + _dw_same(p1, w[gp + "fsmn.conv1.weight"].reshape(p1.shape[1], -1))     # padded by lorder - 1 on both sides: 'same' for 2 lorder - 1 taps
    h = xv * (xu + mem) + h
    h = _layernorm(h, w[p + "norm2.weight"], w[p + "norm2.bias"], 1e-8)
    return _lin(h, w, p + "conv2") + x


def masknet(feats, w, num_blocks, stages=None):
    """feats [T, in_channels] (any float dtype) -> mask [T, out_channels_final] float64."""
    x = feats.to(F64)
    T = x.shape[0]
    mu = x.mean()
    var = ((x - mu) ** 2).mean()
    x = w[P + "norm.weight"].reshape(-1).to(F64) * (x - mu) / torch.sqrt(var + 1e-8) + w[P + "norm.bias"].reshape(-1).to(F64)
    x = _lin(x, w, P + "conv1d_encoder", bias=False)
    C = x.shape[1]
    inv = w[P + "pos_enc.inv_freq"].to(F64)
    ang = torch.arange(T, dtype=F64)[:, None] * inv[None, :]
    x = x + torch.cat([torch.sin(ang), torch.cos(ang)], dim=1) * w[P + "pos_enc.scale"].to(F64)
    x0 = x
    m = P + "mdl.intra_mdl.mossformerM."
    for i in range(num_blocks):
        parts = {} if (stages is not None and i == 0) else None
        x = flash(x, w, f"{m}layers.{i}.", parts)
        if stages is not None and i == 0:
            stages["flash0"], stages["parts"] = x.clone(), parts
        x = fsmn_block(x, w, f"{m}fsmn.{i}.")
        if stages is not None and i == 0:
            stages["fsmn0"] = x.clone()
    x = _layernorm(x, w[P + "mdl.intra_mdl.norm.weight"], w[P + "mdl.intra_mdl.norm.bias"], 1e-8)
    mu = x.mean()
    var = ((x - mu) ** 2).mean()
    x = (x - mu) / torch.sqrt(var + 1e-8) * w[P + "mdl.intra_norm.weight"].to(F64) + w[P + "mdl.intra_norm.bias"].to(F64) + x0
    a = w[P + "prelu.weight"].to(F64)
    x = torch.clamp(x, min=0) + a * torch.clamp(x, max=0)
    x = _lin(x, w, P + "conv1d_out")[:, :C]                                            # speaker 0
    x = torch.tanh(_lin(x, w, P + "output")) * torch.sigmoid(_lin(x, w, P + "output_gate"))
    return torch.clamp(_lin(x, w, P + "conv1_decoder", bias=False), min=0)
