#!/usr/bin/env python
"""``ops.shortconv`` (shortconv.hip) against the five-step route the same ShortConv takes on the ops that existed before it, on the same weights:

  five steps   ``linear`` to [rows, 3H] (the GEMV kernels up to 8 rows, the MFMA image above) -> torch split and multiply -> ``ops.dwconv`` on a
               concatenated copy of the state -> torch multiply -> torch slice copy for the new state

at H = 1024 / 2048, L = 3, one item of 1 / 8 rows (step form) and 128 / 1024 rows (tile form).  Every timed call takes the NEXT of enough distinct
weight images that they exceed the 256 MB Infinity Cache, so a decode step's weights come from HBM.  Medians over five event-timed windows behind
a warm-up, the routes alternating in one process; the clock is whatever the device runs at under this load.

    python tools/bench_lfm2.py [--out-dir DIR]     # DIR receives bench_lfm2.jsonl
"""
import argparse
import json
import os
import statistics
import sys

import torch

import _bench_util as U  # noqa: F401  (puts the repo root on sys.path)
from mlx_audio_amd import ops
from mlx_audio_amd.lm.stack import linear, make_lin

L = 3


def timed_us(fn, inner, repeats=5, warmup=8):
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
    return statistics.median(out), (max(out) - min(out)) / statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=None)
    a = ap.parse_args()
    ops.require_gpu()
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    lines = []
    for H in (1024, 2048):
        n_img = -(-300_000_000 // (6 * H * H))
        lins = [make_lin(torch.randn(3 * H, H, generator=g) / H ** 0.5, None, dev) for _ in range(n_img)]
        taps, state = torch.randn(H, L, generator=g).to(dev), torch.randn(1, L - 1, H, generator=g).to(dev)
        for T in (1, 8, 128, 1024):
            x = torch.randn(1, T, H, generator=g).to(dev)
            y, y0, s_out, s0 = torch.empty(1, T, H, device=dev), torch.empty(1, T, H, device=dev), torch.empty_like(state), torch.empty_like(state)
            u, z = torch.empty(1, T, 3 * H, device=dev), torch.empty(1, T + L - 1, H, device=dev)
            turn = [0]

            def nxt():
                turn[0] += 1
                return lins[turn[0] % n_img]

            def fused():
                ops.shortconv(x, nxt().rm, taps, y, state_in=state, state_out=s_out)

            def five():
                linear(x, nxt(), u)
                z[:, :L - 1] = state
                torch.mul(u[..., :H], u[..., 2 * H:], out=z[:, L - 1:])
                ops.dwconv(z, taps, None, y0)
                y0.mul_(u[..., H:2 * H])
                s0.copy_(z[:, T:])

            turn[0] = -1
            fused()
            turn[0] = -1
            five()
            r = {"what": "shortconv_vs_five_steps", "H": H, "L": L, "rows": T, "images": n_img, "form": ops.shortconv_route(1, T, H, L)["form"],
                 "max_abs_diff_y": float((y - y0).abs().max()), "peak_abs_y": float(y0.abs().max()), "max_abs_diff_state": float((s_out - s0).abs().max())}
            inner = 200 if T <= 128 else 40
            r["shortconv_us"], r["shortconv_window_spread"] = timed_us(fused, inner)
            r["five_steps_us"], r["five_steps_window_spread"] = timed_us(five, inner)
            r["shortconv_vs_five_steps"] = r["shortconv_us"] / r["five_steps_us"]
            r["weight_bytes_per_s_share_of_8TBps"] = 6 * H * H / (r["shortconv_us"] * 1e-6) / 8.0e12
            lines.append(r)
            print(json.dumps(r), flush=True)
        del lins
        torch.cuda.empty_cache()
    if a.out_dir:
        os.makedirs(a.out_dir, exist_ok=True)
        with open(os.path.join(a.out_dir, "bench_lfm2.jsonl"), "w") as f:
            f.write("".join(json.dumps(x) + "\n" for x in lines))


if __name__ == "__main__":
    sys.exit(main())
