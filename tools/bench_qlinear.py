#!/usr/bin/env python
"""``ops.qlinear`` on MLX 4- / 8-bit group-64 images (qlinear.hip) against the routes the same dequantised weights take as an fp16 image, at the
whisper-large-v3-turbo decoder shapes (K, N) = (1280, 1280), (1280, 3840), (1280, 5120), (5120, 1280), (1280, 51866) and M = 1, 4, 8, 16, 64 rows:

  gemv route   ``ops.gemv`` on the row-major fp16 image of the dequantised weights (1..8 rows: FMA / matrix-pipe GEMV; 9..64: gemm_rows.hip)
  rows route   9..64 rows: the rows pipeline (``rows_finish`` float rows -> planes, ``rows_gemm`` on the tile image, ``rows_finish`` partials -> y)

Every timed call takes the NEXT of enough distinct images that the packed ones alone exceed the 256 MB Infinity Cache, so one-row weights come
from HBM.  Medians over five event-timed windows behind a warm-up, the routes alternating in one process.  Also reported: the bytes a call must
move (packed words, (scale, zero) pairs, x, y) over the kernel time, as a share of the 8 TB/s HBM peak.

    python tools/bench_qlinear.py [--out-dir DIR]     # DIR receives bench_qlinear.jsonl
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
ROWS = [1, 4, 8, 16, 64]
G = 64
HBM_PEAK = 8.0e12


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
    ap.add_argument("--shapes", type=int, nargs="*", default=list(range(len(SHAPES))))
    a = ap.parse_args()
    ops.require_gpu()
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    lines = []
    for K, N in (SHAPES[i] for i in a.shapes):
        for bits in (4, 8):
            q_bytes = N * K * bits // 8 + N * (K // G) * 4
            n_img = max(2, min(400, -(-600_000_000 // q_bytes)))
            qls, rms, tls = [], [], []
            for _ in range(n_img):   # random codes and pairs made on the device; the fp16 images hold the same dequantised values
                words = torch.randint(-2 ** 31, 2 ** 31 - 1, (N, K * bits // 32), device=dev, generator=gen, dtype=torch.int64).to(torch.int32)
                scale = (torch.rand(N, K // G, device=dev, generator=gen) + 0.5) * (0.4 / (1 << bits) / K ** 0.5)
                sz = torch.stack([scale, -scale * (1 << (bits - 1))], -1).half().contiguous()
                ql = ops.QuantizedLinear(words, sz, None, N, K, bits, G)
                rm = ops.RowMajor16(ops.dequantize_affine(ql).half().view(torch.int16), None, N, K, True)
                qls.append(ql), rms.append(rm), tls.append(ops.tiles16_from_rowmajor(rm))
            for M in ROWS:
                x = torch.randn(M, K, device=dev, generator=gen)
                y, y0 = torch.empty(M, N, device=dev), torch.empty(M, N, device=dev)
                turn = [0]

                def nxt(images):
                    turn[0] += 1
                    return images[turn[0] % n_img]

                ops.qlinear(x, qls[0], y)
                ops.gemv(x, rms[0], y0)
                r = {"what": "qlinear_vs_fp16_routes", "K": K, "N": N, "M": M, "bits": bits, "group_size": G, "images": n_img,
                     "form": ops.qlinear_route(M, N, K, bits, G)["form"], "max_abs_diff_vs_gemv": float((y - y0).abs().max()), "peak_abs": float(y0.abs().max())}
                inner = max(20, min(400, int(4e4 / (q_bytes / 4e6 + 5))))
                r["qlinear_us"], r["qlinear_window_spread"] = timed_us(lambda: ops.qlinear(x, nxt(qls), y), inner)
                r["gemv_fp16_us"], _ = timed_us(lambda: ops.gemv(x, nxt(rms), y0), inner)
                best = r["gemv_fp16_us"]
                if M >= 9:
                    R, kg = ops.rows_R(M), ops.rows_kgroups(N, K)
                    planes, part = ops.rows_planes(R, K, dev), torch.empty(kg, M, ops.round_up(N, 8), device=dev)

                    def rows_route():
                        ops.rows_finish(x, M, K, 1, planes=planes, R=R, f16=True)
                        ops.rows_gemm(planes, nxt(tls), part, M, R, kgroups=kg)
                        ops.rows_finish(part, M, N, kg, y=y0)

                    rows_route()
                    r["max_abs_diff_vs_rows"] = float((y - y0).abs().max()) if turn[0] % n_img == 0 else None
                    r["rows_pipeline_us"], _ = timed_us(rows_route, inner)
                    best = min(best, r["rows_pipeline_us"])
                r["qlinear_vs_best_fp16_route"] = r["qlinear_us"] / best
                r["qlinear_bytes"] = q_bytes + 4 * M * (K + N)
                r["qlinear_share_of_hbm_peak"] = r["qlinear_bytes"] / (r["qlinear_us"] * 1e-6) / HBM_PEAK
                r["fp16_bytes"] = 2 * N * K + 4 * M * (K + N)
                r["best_fp16_share_of_hbm_peak"] = r["fp16_bytes"] / (best * 1e-6) / HBM_PEAK
                lines.append(r)
                print(json.dumps(r), flush=True)
            del qls, rms, tls
            torch.cuda.empty_cache()
    if a.out_dir:
        os.makedirs(a.out_dir, exist_ok=True)
        with open(os.path.join(a.out_dir, "bench_qlinear.jsonl"), "w") as f:
            f.write("".join(json.dumps(x) + "\n" for x in lines))


if __name__ == "__main__":
    sys.exit(main())
