#!/usr/bin/env python
"""MossFormer2 SE 48K at the published size (180 -> 512, 24 layers, 961 mask columns) on seeded weights.

Each kernel of csrc/mossformer.hip at the 4 s chunk size (496 frames) and at 20 s (2496 frames), B = 1 and B = 16, against the same arithmetic
composed from ``torch.matmul`` and elementwise ops on the same machine and the same tensors (the composed form is the baseline, not code under
test; it materialises the [B, groups, 256, 256] score tensor as the reference does).  Then end to end, waveform to waveform: 1 x 4 s, 16 x 4 s as
one batch, 1 x 20 s.  Medians over repeats of event-timed windows behind a warm-up; nothing is fixed in advance.

    python tools/bench_mossformer2.py [--out-dir DIR] [--blocks N]     # DIR receives bench_mossformer2.jsonl
"""
import argparse
import json
import os
import statistics
import time

import numpy as np
import torch

import _bench_util as U  # noqa: F401  (puts the repo root on sys.path)
from mlx_audio_amd import ops
from mlx_audio_amd.sts.models.mossformer2_se import MossFormer2SEConfig, MossFormer2SEModel, make_mossformer2_weights

DEV = "cuda:0"
C, E, D, G = 512, 2048, 128, 256


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


def torch_heads(qk, gamma, beta, cos, sin):
    T = qk.shape[1]
    z = qk[:, :, None, :] * gamma + beta                                   # [B, T, 4, 128]
    a, b, c, s = z[..., :16], z[..., 16:32], cos[:T, None, :], sin[:T, None, :]
    return torch.cat([a * c - b * s, b * c + a * s, z[..., 32:]], dim=-1)


def torch_attention(qk, vu, gamma, beta, cos, sin):
    """cal_attention and the gate composed from tensor ops: heads, zero padding to whole groups, S for v and for u, the linear terms."""
    B, T, _ = qk.shape
    h = torch_heads(qk, gamma, beta, cos, sin)
    pad = (-T) % G
    z = lambda t: torch.nn.functional.pad(t, (0, 0, 0, pad)).reshape(B, -1, G, t.shape[-1])
    qq, lq, kk, lk = (z(h[:, :, i]) for i in range(4))
    v, u = z(vu[..., :E // 2]), z(vu[..., E // 2:])
    sim = torch.matmul(qq, kk.transpose(-1, -2)) / G
    attn = torch.relu(sim) ** 2
    qv, qu = torch.matmul(attn, v), torch.matmul(attn, u)
    lkf = lk.reshape(B, -1, D).transpose(1, 2)
    kv, ku = torch.matmul(lkf, v.reshape(B, -1, E // 2)) / T, torch.matmul(lkf, u.reshape(B, -1, E // 2)) / T
    lqf = lq.reshape(B, -1, D)
    av = (qv.reshape(B, -1, E // 2) + torch.matmul(lqf, kv))[:, :T]
    au = (qu.reshape(B, -1, E // 2) + torch.matmul(lqf, ku))[:, :T]
    return (au * vu[..., :E // 2]) * torch.sigmoid(av * vu[..., E // 2:])


def torch_shift_scalenorm(x, g):
    s = torch.cat([torch.nn.functional.pad(x[:, :-1, :C // 2], (0, 0, 1, 0)), x[:, :, C // 2:]], dim=-1)
    n = torch.sqrt((s * s).sum(-1, keepdim=True)) * C ** -0.5
    return s * (g / torch.clamp(n, min=1e-8))


def torch_gated_fsmn(p, xu, xv, res, w):
    K = w.shape[1]
    conv = torch.nn.functional.conv1d(p.transpose(1, 2), w[:, None, :], padding=(K - 1) // 2, groups=p.shape[2]).transpose(1, 2)
    return xv * (xu + p + conv) + res


def kernel_lines(B, T):
    g = torch.Generator().manual_seed(1)
    r = lambda *s: torch.randn(*s, generator=g).to(DEV)
    qk, vu, x = r(B, T, D) * 2, r(B, T, E), r(B, T, C)
    gamma, beta = (1 + 0.1 * r(4, D)), 0.1 * r(4, D)
    rope = ops.gau_rope_tables(T, DEV)
    kv, ws, out = torch.empty(B, D, E, device=DEV), torch.empty(ops.gau_kv_workspace_floats(B, T, E), device=DEV), torch.empty(B, T, E // 2, device=DEV)
    p, xu, xv, res, w = r(B, T, 256), r(B, T, 256), r(B, T, 256), r(B, T, 256), r(256, 39) / 6
    y, yf, gs = torch.empty(B, T, C, device=DEV), torch.empty(B, T, 256, device=DEV), torch.ones(1, device=DEV)
    lines = []

    def line(kernel, ours, composed, **extra):
        a, b = timed_us(ours), timed_us(composed)
        lines.append(dict(what="mossformer2_kernel", kernel=kernel, B=B, frames=T, kernel_us=a, torch_composed_us=b, speedup=b / a, **extra))

    def attn():
        ops.gau_kv(qk, vu, gamma, beta, rope, kv=kv, ws=ws)
        ops.gau_attention(qk, vu, kv, gamma, beta, rope, out)

    flop = 2.0 * B * T * (min(T, G) * D + min(T, G) * E + 2 * D * E)
    line("gau_kv + gau_attention", attn, lambda: torch_attention(qk, vu, gamma, beta, rope[0], rope[1]), approx_gflop=flop / 1e9)
    for cols in (64, 128):
        lines.append(dict(what="mossformer2_kernel", kernel=f"gau_attention alone, cols={cols}", B=B, frames=T,
                          kernel_us=timed_us(lambda: ops.gau_attention(qk, vu, kv, gamma, beta, rope, out, cols=cols))))
    lines.append(dict(what="mossformer2_kernel", kernel="gau_kv alone", B=B, frames=T, kernel_us=timed_us(lambda: ops.gau_kv(qk, vu, gamma, beta, rope, kv=kv, ws=ws))))
    line("shift_scalenorm", lambda: ops.shift_scalenorm(x, y, g=gs), lambda: torch_shift_scalenorm(x, gs))
    line("gated_fsmn", lambda: ops.gated_fsmn(p, xu, xv, res, w, yf), lambda: torch_gated_fsmn(p, xu, xv, res, w))
    return lines


def end_to_end(eng, B, seconds):
    rng = np.random.default_rng(0)
    clips = [(0.1 * rng.standard_normal(seconds * 48000)).astype(np.float32) for _ in range(B)]
    for _ in range(2):
        eng.enhance_batch(clips)
    ts = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.enhance_batch(clips)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    ms = statistics.median(ts) * 1e3
    return dict(what="mossformer2_se_published_size", B=B, seconds=seconds, frames=1 + (seconds * 48000 - 1920) // 384, blocks=eng.config.num_blocks,
                enhance_batch_ms=ms, audio_seconds_per_second=B * seconds / (ms / 1e3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=os.path.join(U.ROOT, "profiles"))
    ap.add_argument("--blocks", type=int, default=24)
    args = ap.parse_args()
    lines = []
    for B, T in ((1, 496), (16, 496), (1, 2496)):
        lines += kernel_lines(B, T)
    cfg = MossFormer2SEConfig(num_blocks=args.blocks)
    eng = MossFormer2SEModel(cfg, weights=make_mossformer2_weights(cfg, 0), device=DEV, dither=0.0)
    for B, s in ((1, 4), (16, 4), (1, 20)):
        lines.append(end_to_end(eng, B, s))
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "bench_mossformer2.jsonl"), "w") as f:
        for ln in lines:
            print(json.dumps(ln))
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
