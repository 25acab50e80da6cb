#!/usr/bin/env python
"""``ops.qlinear`` on MLX mxfp4 / nvfp4 / mxfp8 images (qlinear_mx.hip) against the affine kernel of the same bits at group 32 (qlinear.hip) and
the fp16 GEMV route, at the whisper-large-v3-turbo decoder shapes (K, N) = (1280, 1280), (1280, 3840), (1280, 5120), (5120, 1280), (1280, 51866)
and M = 1, 8, 9, 64 rows (both forms, both sides of the 8 / 9 switch).

Every timed call takes the NEXT of enough distinct images that the packed ones alone exceed the 256 MB Infinity Cache, so one-row weights come
from HBM.  The three routes ALTERNATE window by window in one process; medians over five event-timed windows behind a warm-up, with the spread
(max - min) / median of each route's windows -- "not slower than affine" is read against the affine line's own spread.

    python tools/bench_qlinear_mx.py [--out-dir DIR] [--shapes I ...]     # DIR receives bench_qlinear_mx.jsonl
"""
import argparse
import json
import os
import statistics
import sys

import torch

import _bench_util as U  # noqa: F401  (puts the repo root on sys.path)
from mlx_audio_amd import ops

SHAPES = [(1280, 1280), (1280, 3840), (1280, 5120), (5120, 1280), (1280, 51866)]
ROWS = [1, 8, 9, 64]
HBM_PEAK = 8.0e12


def alternated_us(fns, inner, repeats=5, warmup=8):
    """{name: (median us, spread)} of the callables ``fns``, one window of each in turn per repeat."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            e0, e1 = U.ev(), U.ev()
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out[k].append(e0.elapsed_time(e1) * 1000.0 / inner)
    return {k: (statistics.median(v), (max(v) - min(v)) / statistics.median(v)) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=None)
    ap.add_argument("--shapes", type=int, nargs="*", default=list(range(len(SHAPES))))
    ap.add_argument("--modes", nargs="*", default=list(ops.QMODES))
    a = ap.parse_args()
    ops.require_gpu()
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    lines = []
    for K, N in (SHAPES[i] for i in a.shapes):
        for mode in a.modes:
            _, bits, g = ops.QMODES[mode]
            q_bytes = N * K * bits // 8 + N * (K // g)
            n_img = max(2, min(400, -(-600_000_000 // q_bytes)))
            mxs, afs, rms = [], [], []
            for _ in range(n_img):   # random codes and scales made on the device; the fp16 image holds the MX image's dequantised values
                words = torch.randint(-2 ** 31, 2 ** 31 - 1, (N, K * bits // 32), device=dev, generator=gen, dtype=torch.int64).to(torch.int32)
                if bits == 8:   # no E4M3 NaN codes: clear bit 0 of every byte
                    words &= ~0x01010101
                sb = torch.randint(40, 56, (N, K // g), device=dev, generator=gen) if mode == "nvfp4" else torch.randint(112, 120, (N, K // g), device=dev, generator=gen)
                mx = ops.QuantizedLinearMX(words, sb.to(torch.uint8), None, N, K, mode, bits, g)
                scale = (torch.rand(N, K // 32, device=dev, generator=gen) + 0.5) * (0.4 / (1 << bits) / K ** 0.5)
                afs.append(ops.QuantizedLinear(words, torch.stack([scale, -scale * (1 << (bits - 1))], -1).half().contiguous(), None, N, K, bits, 32))
                mxs.append(mx), rms.append(ops.RowMajor16(ops.dequantize_mx(mx).half().view(torch.int16), None, N, K, True))
            for M in ROWS:
                x = torch.randn(M, K, device=dev, generator=gen)
                y, y0 = torch.empty(M, N, device=dev), torch.empty(M, N, device=dev)
                turn = [0]

                def nxt(images):
                    turn[0] += 1
                    return images[turn[0] % n_img]

                ops.qlinear(x, mxs[0], y)
                ops.gemv(x, rms[0], y0)
                r = {"what": "qlinear_mx_vs_affine_g32_vs_fp16", "K": K, "N": N, "M": M, "mode": mode, "bits": bits, "group_size": g, "images": n_img,
                     "form": ops.qlinear_mx_route(M, N, K, mode)["form"], "max_abs_diff_vs_gemv": float((y - y0).abs().max()), "peak_abs": float(y0.abs().max())}
                inner = max(20, min(400, int(4e4 / (q_bytes / 4e6 + 5))))
                t = alternated_us({"mx": lambda: ops.qlinear(x, nxt(mxs), y), "affine": lambda: ops.qlinear(x, nxt(afs), y),
                                   "fp16": lambda: ops.gemv(x, nxt(rms), y0)}, inner)
                r["mx_us"], r["mx_window_spread"] = t["mx"]
                r["affine_g32_us"], r["affine_window_spread"] = t["affine"]
                r["gemv_fp16_us"], r["gemv_window_spread"] = t["fp16"]
                r["mx_vs_affine"] = r["mx_us"] / r["affine_g32_us"]
                r["mx_vs_fp16_gemv"] = r["mx_us"] / r["gemv_fp16_us"]
                r["mx_bytes"] = q_bytes + 4 * M * (K + N)
                r["mx_share_of_hbm_peak"] = r["mx_bytes"] / (r["mx_us"] * 1e-6) / HBM_PEAK
                lines.append(r)
                print(json.dumps(r), flush=True)
            del mxs, afs, rms
            torch.cuda.empty_cache()
    if a.out_dir:
        os.makedirs(a.out_dir, exist_ok=True)
        with open(os.path.join(a.out_dir, "bench_qlinear_mx.jsonl"), "w") as f:
            f.write("".join(json.dumps(x) + "\n" for x in lines))


if __name__ == "__main__":
    sys.exit(main())
