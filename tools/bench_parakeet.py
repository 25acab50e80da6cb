#!/usr/bin/env python
"""Parakeet CTC at the published 0.6 B encoder size (24 layers, 1024 wide, 8 heads, 128 mels, 256 conv channels, K 9, factor 8) on seeded weights, at
1 x 30 s and 16 x 30 s: the whole encoder + CTC head, each of the three kernels of csrc/conformer.hip alone at the shapes the model gives them, and the
rel-pos attention call composed from torch ops on the same device (matmuls, the pad / reshape shift, softmax) for comparison.  Medians over repeats of
event-timed windows behind a warm-up; one JSON line per batch size.  The layers are 24 copies of one seeded layer in separate device memory."""
import copy
import dataclasses
import json
import statistics
import sys

import torch

import _bench_util as U  # noqa: F401  (puts the repo root on sys.path)
from mlx_audio_amd import ops
from mlx_audio_amd.stt.models.parakeet import ParakeetCTC, make_parakeet_weights
from mlx_audio_amd.stt.models.parakeet.parakeet import ParakeetCTCArgs, _from_dict

ENC = dict(feat_in=128, n_layers=1, d_model=1024, n_heads=8, ff_expansion_factor=4, subsampling_factor=8, self_attention_model="rel_pos",
           subsampling="dw_striding", conv_kernel_size=9, subsampling_conv_channels=256, pos_emb_max_len=5000)
LAYERS = 24
FRAMES = 3001   # 30 s of 10 ms hops


def timed_us(fn, inner=5, repeats=7, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        e0, e1 = U.ev(), U.ev()
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1000.0 / inner)
    return statistics.median(out)


def _clone(v):
    if isinstance(v, torch.Tensor):
        return v.clone()
    if isinstance(v, tuple):
        return tuple(_clone(x) for x in v)
    if dataclasses.is_dataclass(v):
        return dataclasses.replace(v, **{f.name: _clone(getattr(v, f.name)) for f in dataclasses.fields(v) if isinstance(getattr(v, f.name), torch.Tensor)})
    return copy.copy(v)


def build():
    vocab = [f"t{i}" for i in range(1024)]
    cfg = dict(preprocessor=dict(sample_rate=16000, normalize="per_feature", window_size=0.025, window_stride=0.01, window="hann", features=128, n_fft=512, dither=0.0),
               encoder=ENC, decoder=dict(feat_in=1024, num_classes=1024, vocabulary=vocab), decoding=dict(greedy=None))
    args = _from_dict(ParakeetCTCArgs, cfg)
    eng = ParakeetCTC(args, make_parakeet_weights(args, 0))
    eng.encoder.layers = [eng.encoder.layers[0]] + [{k: _clone(v) for k, v in eng.encoder.layers[0].items()} for _ in range(LAYERS - 1)]
    return eng


def torch_relpos(q, k, v, p, u, vb, H, dh, scale):
    """The same call from torch ops: [B, H, T, 2T - 1] and [B, H, T, T] go through memory."""
    B, T, _ = q.shape
    q4 = q.reshape(B, T, H, dh)
    qu, qv = (q4 + u.reshape(H, dh)).transpose(1, 2), (q4 + vb.reshape(H, dh)).transpose(1, 2)
    k4, v4 = k.reshape(B, T, H, dh).transpose(1, 2), v.reshape(B, T, H, dh).transpose(1, 2)
    bd = qv @ p.reshape(1, -1, H, dh).transpose(1, 2).transpose(-2, -1)
    bd = torch.nn.functional.pad(bd, (1, 0)).reshape(B, H, 2 * T, T)[:, :, 1:].reshape(B, H, T, 2 * T - 1)[..., :T]
    w = torch.softmax((qu @ k4.transpose(-2, -1) + bd) * scale, -1)
    return (w @ v4).transpose(1, 2).reshape(B, T, H * dh)


def main():
    ops.require_gpu()
    dev = torch.device("cuda", 0)
    eng = build()
    enc = eng.encoder
    d, H, C, K = 1024, 8, 256, 9
    dh = d // H
    g = torch.Generator().manual_seed(1)
    for B in (1, 16):
        mel = torch.randn(B, FRAMES, 128, generator=g).to(dev)
        lens = [FRAMES] * B
        T = enc.out_lengths([FRAMES])[0]
        r = {"what": "parakeet_ctc_0.6b_encoder", "B": B, "seconds": 30, "frames": T, "layers": LAYERS}
        r["total_ms"] = timed_us(lambda: eng.decoder.frame_ids(enc(mel, lens)[0]), inner=2, repeats=5, warmup=2) / 1e3
        # the three kernels alone, at the model's shapes
        qkv = torch.randn(B, T, 3 * d, generator=g).to(dev)
        p = torch.randn(2 * T - 1, d, generator=g).to(dev)
        u, vb = torch.randn(d, generator=g).to(dev) * 0.2, torch.randn(d, generator=g).to(dev) * 0.2
        out = torch.empty(B, T, d, device=dev)
        q, k, v = qkv[:, :, :d], qkv[:, :, d:2 * d], qkv[:, :, 2 * d:]
        attn = lambda: ops.relpos_attention(q, k, v, p, u, vb, out, heads=H, dh=dh, center=T - 1)
        r["relpos_attention_us"] = timed_us(attn)
        want = torch_relpos(q, k, v, p, u, vb, H, dh, dh ** -0.5)
        attn()
        r["relpos_vs_torch_max_abs"] = float((out - want).abs().max())
        r["relpos_torch_composed_us"] = timed_us(lambda: torch_relpos(q, k, v, p, u, vb, H, dh, dh ** -0.5))
        r["relpos_attention_TFLOPs"] = 4 * 2.0 * B * H * T * T * dh / r["relpos_attention_us"] / 1e6   # q k, q p, p v at T x T, the band computed twice over
        pw = torch.randn(B, T, 2 * d, generator=g).to(dev)
        w9, b9 = torch.randn(d, K, generator=g).to(dev) / 3, torch.randn(d, generator=g).to(dev)
        r["glu_dwconv_silu_us"] = timed_us(lambda: ops.glu_dwconv_silu(pw, w9, b9, out))
        r["glu_dwconv_silu_GBps"] = 3 * out.numel() * 4 / r["glu_dwconv_silu_us"] / 1e3
        r["copy_same_bytes_us"] = timed_us(lambda: pw[:, :, :d].copy_(out))
        w3, b3 = torch.randn(C, 3, 3, generator=g).to(dev) / 3, torch.randn(C, generator=g).to(dev)
        x, st = mel, []
        for i in range(3):
            Tn, Fn = ops.stencil2d_out(x.shape[1]), ops.stencil2d_out(x.shape[2])
            y = torch.empty(B, Tn, Fn, C, device=dev)
            st.append(timed_us(lambda: ops.stencil2d_k3s2(x, w3, b3, y, relu=i == 0)))
            x = y
        r["stencil2d_k3s2_us"] = st
        r["new_kernels_share_of_total"] = (LAYERS * (r["relpos_attention_us"] + r["glu_dwconv_silu_us"]) + sum(st)) / (r["total_ms"] * 1e3)
        print(json.dumps(r))
        sys.stdout.flush()


if __name__ == "__main__":
    main()
