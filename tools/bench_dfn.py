#!/usr/bin/env python
"""DeepFilterNet3 at the published sizes (fft 960 / hop 480, 32 ERB bands, 96 DF bins, order 5, 16 channels, five GRU layers of 256 units) on seeded
weights, waveform to waveform: 1 x 60 s, 16 x 60 s and 64 x 10 s of 48 kHz audio through ``enhance_batch`` (host framing, upload and download
included), with the share of the five ``gru_seq`` launches (event-timed around each launch in a run of their own); and ``mi355_gru_seq`` alone at
H = 256: microseconds per dependent step at 10 s and 60 s of frames for 1, 16 and 64 sequences, against the same recurrence composed per step from
``ops.gemv`` (the recurrent product, fp16 row-major image of the same weights) plus torch element-wise ops -- the only way to run a GRU with this
package before the kernel -- both taking turns window by window in one process.  Every time is the median of event-timed windows behind a warm-up;
the spread is the windows' own (min, max).  The composed loop is timed over ``--composed-steps`` steps (its cost per step does not depend on T).
One JSON line per configuration, printed and written to ``--out`` (default ``profiles/bench_dfn.jsonl``, rewritten per run)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

import _bench_util as U
from mlx_audio_amd import ops


def window_us(fn, inner):
    e0, e1 = U.ev(), U.ev()
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / inner


def stat(ws, unit="us"):
    return {f"median_{unit}": statistics.median(ws), f"min_{unit}": min(ws), f"max_{unit}": max(ws)}


def composed(xproj, rw, bhn, out, h, rec):
    """One ``ops.gemv`` and the gates from torch ops per step; ``h`` [B, H] is advanced in place."""
    H = h.shape[1]
    for t in range(xproj.shape[1]):
        ops.gemv(h, rw, rec)
        x = xproj[:, t]
        rz = torch.sigmoid(x[:, :2 * H] + rec[:, :2 * H])
        n = torch.tanh(torch.addcmul(x[:, 2 * H:], rz[:, :H], rec[:, 2 * H:] + bhn))
        h.copy_(torch.lerp(n, h, rz[:, H:]))   # (1 - z) n + z h
        out[:, t] = h


def bench_kernel(dev, g, B, T, H, composed_steps, repeats, warmup):
    s = H ** -0.5
    wh = ((torch.rand(3 * H, H, generator=g) * 2 - 1) * s).half().float()
    bhn = ((torch.rand(H, generator=g) * 2 - 1) * s).to(dev)
    xproj = torch.randn(B, T, 3 * H, generator=g).to(dev)
    img = ops.pack_gru_wh(wh, dev)
    rw = ops.pack_rowmajor16(wh, None, dev, f16=True)
    out = torch.empty(B, T, H, device=dev)
    Tc = min(T, composed_steps)
    out_c, h, rec = torch.empty(B, Tc, H, device=dev), torch.zeros(B, H, device=dev), torch.empty(B, 3 * H, device=dev)

    def run_composed():
        h.zero_()
        composed(xproj[:, :Tc], rw, bhn, out_c, h, rec)

    fns = {"gru_seq": (lambda: ops.gru_seq(xproj, img, bhn, out), 3, T), "composed": (run_composed, 1, Tc)}
    for fn, _, _ in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ws = {k: [] for k in fns}
    for _ in range(repeats):
        for k, (fn, inner, steps) in fns.items():
            ws[k].append(window_us(fn, inner) / steps)
    r = {"what": "gru_seq", "H": H, "B": B, "T": T, "composed_steps": Tc}
    for k, w in ws.items():
        r[k + "_per_step"] = stat(w)
    r["gru_seq_launch_ms"] = r["gru_seq_per_step"]["median_us"] * T / 1e3
    r["composed_over_gru_seq"] = r["composed_per_step"]["median_us"] / r["gru_seq_per_step"]["median_us"]
    # the medians differ by more than the run-to-run spread when the slowest kernel window is still faster than the fastest composed window
    r["gru_seq_max_below_composed_min"] = r["gru_seq_per_step"]["max_us"] < r["composed_per_step"]["min_us"]
    r["vs_composed_max_abs"] = float((out[:, :Tc] - out_c).abs().max())
    return r


def bench_model(eng, B, seconds, repeats, warmup):
    rng = np.random.default_rng(B)
    clips = [(0.1 * rng.standard_normal(int(seconds * 48000))).astype(np.float32) for _ in range(B)]
    run = lambda: eng.enhance_batch(clips)
    for _ in range(warmup):
        ys = run()
    assert len(ys) == B and all(y.shape == c.shape and np.isfinite(y).all() for y, c in zip(ys, clips))
    ws = [window_us(run, 1) / 1e3 for _ in range(repeats)]
    # the five GRU launches, event-timed one by one in a run of their own
    real, spans = ops.gru_seq, []

    def timed(*a, **k):
        e0, e1 = U.ev(), U.ev()
        e0.record()
        r = real(*a, **k)
        e1.record()
        spans.append((e0, e1))
        return r

    ops.gru_seq = timed
    try:
        total = window_us(run, 1) / 1e3
    finally:
        ops.gru_seq = real
    gru_ms = sum(e0.elapsed_time(e1) for e0, e1 in spans)
    r = {"what": "dfn3_enhance_batch", "B": B, "seconds": seconds, "frames": eng.n_frames(int(seconds * 48000)), **stat(ws, "ms")}
    r["x_real_time"] = B * seconds * 1e3 / r["median_ms"]
    r.update(gru_launches=len(spans), gru_ms=gru_ms, gru_us_per_step=gru_ms * 1e3 / (len(spans) * r["frames"]), gru_share=gru_ms / total)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(U.ROOT, "profiles", "bench_dfn.jsonl"))
    ap.add_argument("--kernel-only", action="store_true", help="skip the whole-model lines")
    ap.add_argument("--composed-steps", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    ops.require_gpu()
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(1)
    lines = []

    def emit(r):
        lines.append(r)
        print(json.dumps(r))
        sys.stdout.flush()

    for H, B, T in ((256, 1, 1000), (256, 1, 6000), (256, 16, 6000), (256, 64, 1000), (128, 1, 1000), (64, 1, 1000)):
        emit(bench_kernel(dev, g, B, T, H, a.composed_steps, a.repeats, a.warmup))
    if not a.kernel_only:
        from mlx_audio_amd.sts.models.deepfilternet import DeepFilterNet3Config, DeepFilterNetModel

        eng = DeepFilterNetModel(DeepFilterNet3Config(conv_lookahead=2, df_lookahead=2), device="cuda:0", seed=0)
        for B, seconds in ((1, 60), (16, 60), (64, 10)):
            emit(bench_model(eng, B, seconds, repeats=5, warmup=2))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for r in lines:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
