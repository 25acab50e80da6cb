#!/usr/bin/env python
"""``ops.switch_glu`` on MLX's packed 4 / 8-bit expert codes (moe_quant.hip) against ``ops.switch_glu`` on the float images of the SAME dequantised
weights (moe.hip: the path a quantised checkpoint had to take before), at the Ling-lite expert shape D 2048, I 1408, E 64, k 6, group 64, for
N = 1, 8, 64, 512, 4096 tokens.  The two alternate in one process; every timed call takes the NEXT of 8 routings, as tools/bench_moe.py does, so
that the weights of a decode line come from HBM.  Per line: the medians and the spread of the five windows, packed bytes touched over time, the
ratio quantised / float, and the largest output difference.  The last line is the weight footprint of the Ling-lite and Ling-mini expert shapes,
computed from the shapes.

    python tools/bench_moe_quant.py [--out-dir DIR]     # DIR receives bench_moe_quant.jsonl

``--mx`` measures instead ``ops.switch_glu`` on mxfp4 / nvfp4 / mxfp8 codes (moe_quant_mx.hip) against the affine 4-bit group-32 kernel
(moe_quant.hip) at the same shape, tokens and rotation, both quantised from the same float weights, alternating in one process; DIR receives
bench_moe_mx.jsonl.
"""
import argparse
import json
import os
import sys

import torch

import _bench_util as U  # noqa: F401  (puts the repo root on sys.path)
import bench_moe as M
from mlx_audio_amd import ops

D, I, E, K, G = M.D, M.I, M.E, M.K, 64


def footprint(name, layers, d, i, e, bits, g=G):
    """Bytes of the routed experts of ``layers`` sparse layers: float images (bf16 hi + lo: 4 bytes a weight) against codes + 16-bit pairs."""
    weights = layers * e * 3 * d * i
    return {"what": "expert_footprint", "model": name, "layers": layers, "D": d, "I": i, "E": e, "bits": bits, "group_size": g, "weights": weights,
            "float_image_GB": weights * 4 / 1e9, "packed_GB": weights * (bits / 8 + 4 / g) / 1e9, "bytes_per_weight": bits / 8 + 4 / g}


def main_mx(a, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    floats = [(torch.randn(E * n, k, device=dev, generator=g) / k ** 0.5).half() for n, k in ((I, D), (I, D), (D, I))]
    shape = lambda t, n: t.view(E, n, -1)
    aff = ops.PackedQuantizedExperts(*[ops.pack_quantized_switch_linear(*(shape(t, n) for t in ops.quantize_affine(w, 32, 4)), None, dev, group_size=32, bits=4)
                                       for w, n in zip(floats, (I, I, D))])
    mx = {m: ops.PackedQuantizedExpertsMX(*[ops.pack_quantized_switch_linear_mx(*(shape(t, n) for t in ops.quantize_mx(w, m)), None, dev, mode=m)
                                            for w, n in zip(floats, (I, I, D))]) for m in ops.QMODES}
    lines = []
    for N in a.tokens:
        x = torch.randn(N, D, device=dev, generator=g)
        routes = [ops.moe_route(torch.randn(N, E, device=dev, generator=g), K, norm_topk_prob=True) for _ in range(8)]
        out_a, out_m = torch.empty(N, D, device=dev), torch.empty(N, D, device=dev)
        ws = ops.MoeWorkspace(N, K, E, D, I, dev)
        turn = [0]

        def run(ex, out):
            turn[0] += 1
            ids, wts = routes[turn[0] % len(routes)]
            return ops.switch_glu(x, ex, ids, wts, out, ws=ws)

        ids, wts = routes[0]
        ops.switch_glu(x, aff, ids, wts, out_a, ws=ws)
        touched = len(set(ids.flatten().tolist()))
        inner = 400 if N <= 8 else (100 if N <= 64 else 16)
        for mode, (_, bits, gs) in ops.QMODES.items():
            ops.switch_glu(x, mx[mode], ids, wts, out_m, ws=ws)
            r = {"what": "switch_glu_mx_vs_affine_4bit_g32", "mode": mode, "N": N, "D": D, "I": I, "E": E, "k": K, "touched_experts": touched,
                 "max_abs_diff_to_affine": float((out_m - out_a).abs().max()), "peak_abs": float(out_a.abs().max())}   # two quantisers of one weight
            for rep in range(2):   # the two kernels alternate; the second pass is reported
                r["mx_us"] = M.timed_us(lambda: run(mx[mode], out_m), inner)
                r["mx_window_spread"] = M.SPREAD[-1]
                r["affine_us"] = M.timed_us(lambda: run(aff, out_a), inner)
                r["affine_window_spread"] = M.SPREAD[-1]
            r["mx_bytes_touched"] = int(touched * 3 * D * I * (bits + 8 / gs) / 8)
            r["affine_bytes_touched"] = int(touched * 3 * D * I * (4 + 32 / 32) / 8)
            r["mx_packed_GBps"] = r["mx_bytes_touched"] / r["mx_us"] / 1e3
            r["mx_over_affine"] = r["mx_us"] / r["affine_us"]
            lines.append(r)
            print(json.dumps(r), flush=True)
    if a.out_dir:
        os.makedirs(a.out_dir, exist_ok=True)
        with open(os.path.join(a.out_dir, "bench_moe_mx.jsonl"), "w") as f:
            f.write("".join(json.dumps(x) + "\n" for x in lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=None)
    ap.add_argument("--tokens", type=int, nargs="*", default=[1, 8, 64, 512, 4096])
    ap.add_argument("--mx", action="store_true", help="the three MX modes against the affine 4-bit group-32 kernel")
    a = ap.parse_args()
    ops.require_gpu()
    dev = torch.device("cuda", 0)
    if a.mx:
        return main_mx(a, dev)
    g = torch.Generator(device=dev).manual_seed(0)
    lines = []
    for bits in (4, 8):
        packed, deq = [], []
        for n, k in ((I, D), (I, D), (D, I)):
            wq, scale, zero = ops.quantize_affine((torch.randn(E * n, k, device=dev, generator=g) / k ** 0.5).half(), G, bits)
            deq.append((scale.float().repeat_interleave(G, 1) * ops.unpack_codes(wq, bits) + zero.float().repeat_interleave(G, 1)).view(E, n, k))
            packed.append(ops.pack_quantized_switch_linear(wq.view(torch.int32).view(E, n, -1), scale.view(E, n, -1), zero.view(E, n, -1), None, dev,
                                                           group_size=G, bits=bits))
        qex, fex = ops.PackedQuantizedExperts(*packed), ops.PackedExperts.pack(*deq, dev)
        del deq
        for N in a.tokens:
            x = torch.randn(N, D, device=dev, generator=g)
            routes = [ops.moe_route(torch.randn(N, E, device=dev, generator=g), K, norm_topk_prob=True) for _ in range(8)]
            out_q, out_f = torch.empty(N, D, device=dev), torch.empty(N, D, device=dev)
            ws = ops.MoeWorkspace(N, K, E, D, I, dev)
            turn = [0]

            def run(ex, out):
                turn[0] += 1
                ids, wts = routes[turn[0] % len(routes)]
                return ops.switch_glu(x, ex, ids, wts, out, ws=ws)

            ids, wts = routes[0]
            ops.switch_glu(x, qex, ids, wts, out_q, ws=ws)
            ops.switch_glu(x, fex, ids, wts, out_f, ws=ws)
            r = {"what": "switch_glu_quantised_vs_float_images", "bits": bits, "group_size": G, "N": N, "D": D, "I": I, "E": E, "k": K,
                 "max_abs_diff": float((out_q - out_f).abs().max()), "peak_abs": float(out_f.abs().max())}
            inner = 400 if N <= 8 else (100 if N <= 64 else 16)
            for rep in range(2):   # the two paths alternate; the second pass is reported
                r["quantised_us"] = M.timed_us(lambda: run(qex, out_q), inner)
                r["quantised_window_spread"] = M.SPREAD[-1]
                r["float_images_us"] = M.timed_us(lambda: run(fex, out_f), inner)
                r["float_images_window_spread"] = M.SPREAD[-1]
            touched = len(set(ids.flatten().tolist()))
            r["touched_experts"] = touched
            r["packed_bytes_touched"] = int(touched * 3 * D * I * (bits / 8 + 4 / G))
            r["quantised_packed_GBps"] = r["packed_bytes_touched"] / r["quantised_us"] / 1e3
            r["quantised_over_float"] = r["quantised_us"] / r["float_images_us"]
            lines.append(r)
            print(json.dumps(r), flush=True)
        del qex, fex
    # per sparse layer: Ling-lite has 64 experts of 2048 x 1408, Ling-mini 256 of 2048 x 512
    lines += [footprint("Ling-lite", 1, 2048, 1408, 64, b) for b in (4, 8)] + [footprint("Ling-mini", 1, 2048, 512, 256, b) for b in (4, 8)]
    for r in lines[-4:]:
        print(json.dumps(r), flush=True)
    if a.out_dir:
        os.makedirs(a.out_dir, exist_ok=True)
        with open(os.path.join(a.out_dir, "bench_moe_quant.jsonl"), "w") as f:
            f.write("".join(json.dumps(x) + "\n" for x in lines))


if __name__ == "__main__":
    sys.exit(main())
