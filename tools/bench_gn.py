#!/usr/bin/env python
"""The one-group GroupNorm kernels (csrc/group_norm.hip) against a device copy of the same bytes, in one process: statistics (one read), coefficients,
apply (one read + one write; two-operand: two reads + one write).  Medians over repeats of event-timed windows; one JSON line per shape."""
import json
import statistics

import torch

import _bench_util as U  # noqa: F401  (puts the repo root on sys.path)
from mlx_audio_amd import ops


def timed_us(fn, inner=20, repeats=9, warmup=5):
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


def main():
    ops.require_gpu()
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    for B, L, C in ((1, 48000, 32), (31, 48000, 32), (31, 150, 512)):
        x = torch.randn(B, L, C, generator=g).to(dev)
        x2, y = torch.randn(B, L, C, generator=g).to(dev), torch.empty(B, L, C, device=dev)
        w, b = torch.rand(C, device=dev) + 0.5, torch.randn(C, device=dev)
        parts = ops.group_norm_stats(x)
        coef = ops.group_norm_coef(parts, L, C, w, b)
        mb = x.numel() * 4 / 1e6
        r = {"shape": [B, L, C], "MB": mb,
             "copy_us": timed_us(lambda: y.copy_(x)),
             "stats_us": timed_us(lambda: ops.group_norm_stats(x)),
             "coef_us": timed_us(lambda: ops.group_norm_coef(parts, L, C, w, b)),
             "apply_us": timed_us(lambda: ops.group_norm_apply(x, coef, y)),
             "apply2_us": timed_us(lambda: ops.group_norm_apply(x, coef, y, x2, coef)),
             "add_us": timed_us(lambda: torch.add(x, x2, out=y))}
        r["stats_GBps"] = mb / r["stats_us"] * 1e3 / 1e3
        r["apply_GBps"] = 2 * mb / r["apply_us"] * 1e3 / 1e3
        r["apply_vs_copy"] = r["apply_us"] / r["copy_us"]
        r["stats_vs_copy"] = r["stats_us"] / r["copy_us"]
        r["apply2_vs_add"] = r["apply2_us"] / r["add_us"]
        print(json.dumps(r))


if __name__ == "__main__":
    main()
