#!/usr/bin/env python
"""``ops.switch_glu`` (plan + grouped GLU + combine, moe.hip) against the torch routes a sparse-MoE checkpoint would take without it, on the same
device in float32 (TF32 off), at the Ling-lite expert shape D 2048, I 1408, E 64, k 6 for N = 1, 8, 64, 512, 4096 tokens:

  gather route   ``w[ids]`` (index_select of [N k, I, D] weights through HBM) + ``bmm`` per projection: the reference's gather_mm spelled in torch;
                 run while one gathered projection stays under 8 GiB
  sorted route   stable sort by expert, one ``mm`` per expert and projection over its rows, ``index_add`` back: the route for many tokens

Both share the router's ids / weights with the kernel.  Every timed call takes the NEXT of 8 routings (for one token: 8 x 6 experts, ~ 1.4 GB of
images, beyond the 256 MB Infinity Cache), so that a decode line is not a warm-cache figure.  The decode line also reports the kernel's bytes / time against the weight bytes of the k
touched experts (hi + lo bf16 images: 4 bytes per weight).  Medians over repeats of event-timed windows behind a warm-up.

    python tools/bench_moe.py [--out-dir DIR]     # DIR receives bench_moe.jsonl
"""
import argparse
import json
import os
import statistics
import sys

import torch

import _bench_util as U  # noqa: F401  (puts the repo root on sys.path)
from mlx_audio_amd import ops

D, I, E, K = 2048, 1408, 64, 6
SPREAD = []   # (max - min) / median of the five windows of every timing


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
    SPREAD.append((max(out) - min(out)) / statistics.median(out))
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=None)
    ap.add_argument("--tokens", type=int, nargs="*", default=[1, 8, 64, 512, 4096])
    a = ap.parse_args()
    ops.require_gpu()
    torch.backends.cuda.matmul.allow_tf32 = False
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    wg, wu = (torch.randn(E, I, D, device=dev, generator=g) / D ** 0.5 for _ in range(2))
    wd = torch.randn(E, D, I, device=dev, generator=g) / I ** 0.5
    experts = ops.PackedExperts.pack(wg, wu, wd, dev)
    lines = []
    for N in a.tokens:
        x = torch.randn(N, D, device=dev, generator=g)
        routes = [ops.moe_route(torch.randn(N, E, device=dev, generator=g), K, norm_topk_prob=True) for _ in range(8)]
        out = torch.empty(N, D, device=dev)
        ws = ops.MoeWorkspace(N, K, E, D, I, dev)
        turn = [0]

        def pick():
            turn[0] += 1
            ids, wts = routes[turn[0] % len(routes)]
            return ids, wts, ids.long()

        def gather_route():
            ids, wts, idl = pick()
            xs = x[:, None, None, :].expand(N, K, 1, D).reshape(N * K, 1, D)
            f = idl.flatten()
            h = torch.nn.functional.silu(torch.bmm(xs, wg[f].transpose(1, 2))) * torch.bmm(xs, wu[f].transpose(1, 2))
            return (torch.bmm(h, wd[f].transpose(1, 2)).view(N, K, D) * wts[..., None]).sum(1)

        def sorted_route(fixed=None):
            ids, wts, idl = fixed or pick()
            order = torch.sort(idl.flatten(), stable=True).indices
            counts = torch.bincount(idl.flatten(), minlength=E).tolist()   # the host needs the group sizes: one read-back per call
            xs, y, r0 = x[order // K], torch.zeros(N, D, device=dev), 0
            for e, c in enumerate(counts):
                if c:
                    rows = xs[r0:r0 + c]
                    h = torch.nn.functional.silu(rows @ wg[e].T) * (rows @ wu[e].T)
                    y.index_add_(0, order[r0:r0 + c] // K, (h @ wd[e].T) * wts.flatten()[order[r0:r0 + c], None])
                    r0 += c
            return y

        def ours(fixed=None):
            ids, wts, _ = fixed or pick()
            return ops.switch_glu(x, experts, ids, wts, out, ws=ws)

        ids, wts = routes[0]
        idl = ids.long()
        ours((ids, wts, idl))
        ref = sorted_route((ids, wts, idl))
        r = {"what": "switch_glu_vs_torch_routes", "N": N, "D": D, "I": I, "E": E, "k": K, "tile_rows": ops.MOE_TILE_ROWS, "col_tile": ops.MOE_COL_TILE,
             "max_abs_diff_vs_sorted_route": float((out - ref).abs().max()), "peak_abs": float(ref.abs().max())}
        inner = 400 if N <= 8 else (100 if N <= 64 else 16)   # windows of 30 - 60 ms
        r["switch_glu_us"] = timed_us(ours, inner)
        r["switch_glu_window_spread"] = SPREAD[-1]
        r["plan_only_us"] = timed_us(lambda: ops.moe_plan(ids, E, D, I, ws=ws), inner)
        r["torch_sorted_route_us"] = timed_us(sorted_route, max(inner // 8, 2))
        if N * K * I * D * 4 <= 8 << 30:
            r["torch_gather_route_us"] = timed_us(gather_route, max(inner // 8, 2))
        else:
            r["torch_gather_route_us"] = None   # one gathered projection alone would exceed 8 GiB
        best = min(v for v in (r["torch_sorted_route_us"], r["torch_gather_route_us"]) if v is not None)
        r["switch_glu_vs_best_torch_route"] = r["switch_glu_us"] / best
        touched = len(set(idl.flatten().tolist()))
        r["touched_experts"] = touched
        r["image_bytes_touched"] = touched * 3 * D * I * 4
        r["switch_glu_image_GBps"] = r["image_bytes_touched"] / r["switch_glu_us"] / 1e3
        r["switch_glu_tflops"] = 2.0 * N * K * 3 * D * I / r["switch_glu_us"] / 1e6   # algorithmic: one product per weight and pair
        lines.append(r)
        print(json.dumps(r), flush=True)
    if a.out_dir:
        os.makedirs(a.out_dir, exist_ok=True)
        with open(os.path.join(a.out_dir, "bench_moe.jsonl"), "w") as f:
            f.write("".join(json.dumps(x) + "\n" for x in lines))


if __name__ == "__main__":
    sys.exit(main())
