#!/usr/bin/env python
"""Mel-Band RoFormer at the ``kim_vocal_2`` size (dim 384, depth 6, 60 bands, n_fft 2048 / hop 441) on seeded weights, waveform to waveform:
1 x 8 s and 4 x 8 s of 44.1 kHz stereo through ``MelRoFormer.__call__`` (upload included); and ``band_split`` / ``band_merge`` alone at the same
sizes against the composition of existing ops they replace, both taking turns window by window in one process:

  * split, composed: per band one gather (``index_select`` on the CaC-interleaved spectrum), one ``ops.rmsnorm`` and one ``ops.conv_gemm`` into the
    band's strided column of ``[B, T, Nb, D]`` -- 180 launches (plus the interleave) for one; ``rmsnorm`` has no clamp, so this form is also
    not safe on digital silence;
  * merge, composed: per band the GLU from element-wise ops and one ``index_add_`` into ``[B, 2 F, T, 2]`` (the reference does one scatter per
    index), then the division, the complex product and the de-interleave.

Every time is the median of event-timed windows behind a warm-up; the spread is the windows' own (min, max).  One JSON line per configuration,
printed and written to ``--out`` (default ``profiles/bench_melroformer.jsonl``, rewritten per run).

The share of a forward pass that is gaps between kernels comes from a ``rocprofv3 --kernel-trace --stats`` run of its own:

    rocprofv3 --kernel-trace --stats -d DIR -o NAME -- python tools/bench_melroformer.py --trace-pass 3
    python tools/bench_melroformer.py --gaps DIR/.../NAME_results.db [--append]

``--gaps`` reads the trace: a pass is the window from the start of its ``band_split_kernel`` to the end of its ``band_merge_kernel`` (everything but
the STFT and the inverse STFT), the gap share is 1 - (length of the union of the kernels' intervals inside the window) / (window length), the
median over the traced passes."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

import _bench_util as U
from mlx_audio_amd import ops


def window_ms(fn, inner=1):
    e0, e1 = U.ev(), U.ev()
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner


def stat(ws, unit="ms"):
    return {f"median_{unit}": statistics.median(ws), f"min_{unit}": min(ws), f"max_{unit}": max(ws)}


def take_turns(fns, repeats, warmup):
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ws = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            ws[k].append(window_ms(fn))
    return ws


def bench_kernels(eng, B, seconds, repeats, warmup):
    c, dev, tab = eng.config, eng.device, eng.tables
    S = int(seconds * c.sample_rate)
    T, F, Nb, D = eng.n_frames(S), c.freq_bins, c.num_bands, c.dim
    g = torch.Generator().manual_seed(B)
    audio = (0.1 * torch.randn(B * 2, S, generator=g)).to(dev)
    spec = ops.stft_frames(audio, c.n_fft, c.hop_length, eng._window_d, 1, T)
    idx_d = [torch.from_numpy(ix.astype(np.int64)).to(dev) for ix in eng.band_indices]
    ptr = tab.band_ptr
    # ---- split
    wts = [eng.split_wt[D * 2 * int(ptr[n]):D * 2 * int(ptr[n + 1])].view(-1, D).t().contiguous().cpu() for n in range(Nb)]
    packs = [ops.pack_conv(wts[n], eng.split_bias[n].cpu(), dev, f16=True) for n in range(Nb)]
    gammas = [eng.split_gamma[2 * int(ptr[n]):2 * int(ptr[n + 1])].contiguous() for n in range(Nb)]
    y_k = torch.empty(B, T, Nb, D, device=dev)
    y_c = torch.empty(B, T, Nb, D, device=dev)
    sr = torch.view_as_real(spec)

    def split_composed():
        rep = sr.view(B, 2, T, F, 2).permute(0, 2, 3, 1, 4).reshape(B * T, 2 * F, 2)           # CaC interleave, [B T, 2 F, 2]
        yv = y_c.view(1, B * T, Nb * D)
        for n in range(Nb):
            u = rep.index_select(1, idx_d[n]).reshape(1, B * T, -1)
            ops.rmsnorm(u, u, gammas[n], eps=1e-36)
            ops.conv_gemm(u, packs[n], yv[:, :, n * D:(n + 1) * D], precision=4)

    ws = take_turns({"band_split": lambda: ops.band_split(spec, tab, eng.split_wt, eng.split_gamma, eng.split_bias, y=y_k), "composed": split_composed},
                    repeats, warmup)
    r = {"what": "band_split", "B": B, "seconds": seconds, "frames": T, "bands": Nb, "composed_launches_per_call": 1 + 3 * Nb}
    r.update(band_split=stat(ws["band_split"]), composed=stat(ws["composed"]))
    r["composed_over_kernel"] = r["composed"]["median_ms"] / r["band_split"]["median_ms"]
    r["kernel_max_below_composed_min"] = r["band_split"]["max_ms"] < r["composed"]["min_ms"]
    r["vs_composed_rel_peak"] = float((y_k - y_c).abs().max() / y_k.abs().max())   # fp32 FMA against the fp16 hi + lo MFMA passes
    flops = 2.0 * B * T * D * sum(tab.band_dims)
    r["gflop"] = flops / 1e9
    r["band_split_tflops"] = flops / (r["band_split"]["median_ms"] * 1e-3) / 1e12
    yield r
    # ---- merge
    h = torch.randn(B, T, tab.h_cols, generator=g).to(dev)
    count = torch.from_numpy(np.maximum(np.bincount(tab.band_idx, minlength=2 * F), 1).astype(np.float32)).to(dev)
    out_k = torch.empty(B * 2, T, F, 2, device=dev)
    keep = {}

    def merge_kernel():
        ops.band_merge(h, tab, spec, out=out_k.permute(0, 2, 1, 3))

    def merge_composed():
        acc = torch.zeros(B, T, 2 * F, 2, device=dev)
        for n in range(Nb):
            c0, bd = 4 * int(ptr[n]), 2 * int(ptr[n + 1] - ptr[n])
            m = h[:, :, c0:c0 + bd] * torch.sigmoid(h[:, :, c0 + bd:c0 + 2 * bd])
            acc.index_add_(2, idx_d[n], m.view(B, T, bd // 2, 2))
        mask = torch.view_as_complex(acc / count[None, None, :, None])                          # [B, T, 2 F]
        rep = torch.view_as_complex(sr.view(B, 2, T, F, 2).permute(0, 2, 3, 1, 4).reshape(B, T, 2 * F, 2))
        keep["out"] = (rep * mask).view(B, T, F, 2).permute(0, 3, 1, 2).reshape(B * 2, T, F).contiguous()

    ws = take_turns({"band_merge": merge_kernel, "composed": merge_composed}, repeats, warmup)
    r = {"what": "band_merge", "B": B, "seconds": seconds, "frames": T, "bands": Nb, "composed_launches_per_call": "about 4 per band + 6"}
    r.update(band_merge=stat(ws["band_merge"]), composed=stat(ws["composed"]))
    r["composed_over_kernel"] = r["composed"]["median_ms"] / r["band_merge"]["median_ms"]
    r["kernel_max_below_composed_min"] = r["band_merge"]["max_ms"] < r["composed"]["min_ms"]
    r["vs_composed_rel_peak"] = float((torch.view_as_complex(out_k) - keep["out"]).abs().max() / keep["out"].abs().max())
    byts = 4.0 * (h.numel() + 2 * 2 * B * 2 * T * F)
    r["band_merge_gbytes_per_s"] = byts / (r["band_merge"]["median_ms"] * 1e-3) / 1e9
    yield r


def model_flops(c, B, T):
    """Multiply-adds x 2 of one forward pass, counted from the shapes (attention scores and values included, the STFTs not)."""
    Nb, D, I = c.num_bands, c.dim, c.dim_inner
    rows = B * T * Nb
    per_tf = 2.0 * rows * (D * (3 * I + c.heads) + I * D + 2 * D * c.ff_dim)
    attn_t = 4.0 * B * Nb * c.heads * T * T * c.dim_head
    attn_f = 4.0 * B * T * c.heads * Nb * Nb * c.dim_head
    from mlx_audio_amd.sts.models.mel_roformer import band_dims
    bd = band_dims(c)
    mlp = 2.0 * B * T * sum(D * c.mlp_hidden + (c.mask_estimator_depth - 1) * c.mlp_hidden ** 2 + c.mlp_hidden * 2 * b for b in bd)
    split = 2.0 * B * T * D * sum(bd)
    return c.depth * (2 * per_tf + attn_t + attn_f) + mlp + split


def bench_model(eng, B, seconds, repeats, warmup):
    c = eng.config
    S = int(seconds * c.sample_rate)
    rng = np.random.default_rng(B)
    audio = torch.from_numpy((0.1 * rng.standard_normal((B, 2, S))).astype(np.float32))
    out = {}

    def run():
        out["y"] = eng(audio)

    for _ in range(warmup):
        run()
    torch.cuda.synchronize()
    assert out["y"].shape == (B, 2, S) and bool(torch.isfinite(out["y"]).all())
    ws = [window_ms(run) for _ in range(repeats)]
    T = eng.n_frames(S)
    r = {"what": "melroformer_kim_vocal_2", "B": B, "seconds": seconds, "frames": T, "tokens": B * T * c.num_bands, **stat(ws)}
    r["x_real_time"] = B * seconds * 1e3 / r["median_ms"]
    r["tflop_per_pass"] = model_flops(c, B, T) / 1e12
    r["tflops"] = r["tflop_per_pass"] / (r["median_ms"] * 1e-3)
    r["launches_mask_mlp"] = c.num_bands * (c.mask_estimator_depth + 1)
    return r


def gaps(db_path):
    import sqlite3

    cur = sqlite3.connect(db_path).cursor()
    cols = [r[1] for r in cur.execute("pragma table_info(kernels)")]
    name_col = "name" if "name" in cols else [c for c in cols if "name" in c][0]
    rows = cur.execute(f"select {name_col}, start, end from kernels order by start").fetchall()
    starts = [s for n, s, e in rows if "band_split_kernel" in n]
    ends = [e for n, s, e in rows if "band_merge_kernel" in n]
    assert starts and len(starts) == len(ends), (len(starts), len(ends))
    shares, lens, counts = [], [], []
    for s0, e1 in zip(starts, ends):
        inside = [(s, e) for _, s, e in rows if s >= s0 and e <= e1]
        busy, edge = 0, s0
        for s, e in inside:                                                      # the union of the kernels' intervals (rows are in start order)
            busy += max(0, e - max(s, edge))
            edge = max(edge, e)
        shares.append(1.0 - busy / (e1 - s0))
        lens.append((e1 - s0) / 1e6)
        counts.append(len(inside))
    half = len(shares) // 2 if len(shares) > 1 else 0                           # the first passes are the warm-up
    return {"what": "melroformer_gap_share", "passes_traced": len(shares), "passes_used": len(shares) - half, "kernels_per_pass": counts[-1],
            "window_ms": statistics.median(lens[half:]), "gap_share": statistics.median(shares[half:]), "gap_share_min": min(shares[half:]),
            "gap_share_max": max(shares[half:]), "source": "rocprofv3 --kernel-trace --stats, window = band_split start .. band_merge end"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(U.ROOT, "profiles", "bench_melroformer.jsonl"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kernel-only", action="store_true", help="skip the whole-model lines")
    ap.add_argument("--trace-pass", type=int, default=0, help="run only this many 1 x 8 s forward passes twice over (warm-up, then traced): the body of the rocprofv3 run")
    ap.add_argument("--gaps", default=None, help="a rocprofv3 results database of a --trace-pass run: print the gap-share line")
    ap.add_argument("--append", action="store_true", help="with --gaps: append the line to --out")
    a = ap.parse_args()
    if a.gaps:
        r = gaps(a.gaps)
        print(json.dumps(r))
        if a.append:
            with open(a.out, "a") as f:
                f.write(json.dumps(r) + "\n")
        return
    from mlx_audio_amd.sts.models.mel_roformer import MelRoFormer, MelRoFormerConfig

    ops.require_gpu()
    eng = MelRoFormer(MelRoFormerConfig.kim_vocal_2(), device="cuda:0", seed=0)
    if a.trace_pass:
        audio = torch.from_numpy((0.1 * np.random.default_rng(1).standard_normal((1, 2, 8 * 44100))).astype(np.float32))
        for _ in range(2 * a.trace_pass):
            eng(audio)
            torch.cuda.synchronize()
        return
    lines = []

    def emit(r):
        lines.append(r)
        print(json.dumps(r))
        sys.stdout.flush()

    for B in (1, 4):
        for r in bench_kernels(eng, B, 8, a.repeats, a.warmup):
            emit(r)
    if not a.kernel_only:
        for B in (1, 4):
            emit(bench_model(eng, B, 8, a.repeats, a.warmup))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for r in lines:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
