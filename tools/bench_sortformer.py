#!/usr/bin/env python
"""Sortformer at the published sizes (FastConformer 18 x 512 wide / 8 heads of 64 / K 9 / 80 mels / 256 conv channels; Transformer 18 x 192 wide /
8 heads of 24 / FFN 768; 4 speakers) on seeded weights: the offline model at 1 x 90 s and 16 x 90 s (1125 frames), one streaming step at
188 + 188 + 63 frames (a full speaker cache, a full FIFO and a 5 s chunk), and ``narrow_attention`` alone at (T 1125, 8 x 24, B 1 and 16) and at
T 439, alternating in one process with the same call composed from torch ops on the same device (``matmul``, ``softmax``, ``matmul``); at T 439 also
``ops.attention`` (PL-BERT's kernel, T <= 512).  Every time is the median of event-timed windows behind a warm-up; the spread is the windows' own
(min, max).  The layers are 18 + 18 copies of one seeded layer each, in separate device memory.  One JSON line per configuration, printed and
appended to ``--out`` (default ``profiles/bench_sortformer.jsonl``, rewritten per run)."""
import argparse
import json
import os
import statistics
import sys

import torch

import _bench_util as U
from mlx_audio_amd import ops
from mlx_audio_amd.vad.models.sortformer import Model, ModelConfig, make_sortformer_weights

LAYERS = 18
MEL_1125 = 8 * 1125 - 7   # mel frames that subsample to 1125 diarization frames (90 s / 0.08 s)


def windows_us(fn, inner, repeats, warmup):
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
    return out


def alternating_us(fns, inner=20, repeats=11, warmup=3):
    """name -> window times, the candidates taking turns window by window (whatever else shares the machine hits all of them alike)."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            out[k] += windows_us(fn, inner, 1, 0)
    return out


def stat(ws):
    return dict(median_us=statistics.median(ws), min_us=min(ws), max_us=max(ws))


def build():
    cfg = ModelConfig.from_dict(dict(fc_encoder_config=dict(num_hidden_layers=1), tf_encoder_config=dict(encoder_layers=1)))
    eng = Model(cfg, make_sortformer_weights(cfg, 0, head_gain=6.0, head_bias=-3.0))
    fc, tf = eng.fc_encoder, eng.tf_encoder
    clone = lambda layer: {k: U._clone_obj(v) for k, v in layer.items()}   # fresh device memory for every tensor and weight image
    fc.layers = [fc.layers[0]] + [clone(fc.layers[0]) for _ in range(LAYERS - 1)]
    tf.layers = [tf.layers[0]] + [clone(tf.layers[0]) for _ in range(LAYERS - 1)]
    return eng


def torch_attention(q, k, v, H, dh, scale):
    """The same call from torch ops: the [B, H, T, T] scores and weights go through memory."""
    B, T, _ = q.shape
    q4, k4, v4 = (t.reshape(B, T, H, dh).transpose(1, 2) for t in (q, k, v))
    w = torch.softmax((q4 * scale) @ k4.transpose(-2, -1), -1)
    return (w @ v4).transpose(1, 2).reshape(B, T, H * dh)


def bench_kernel(dev, g, B, T, H=8, dh=24, with_attention=False):
    d = H * dh
    qkv = torch.randn(B, T, 3 * d, generator=g).to(dev)
    q, k, v = qkv[:, :, :d], qkv[:, :, d:2 * d], qkv[:, :, 2 * d:]
    out, out2 = torch.empty(B, T, d, device=dev), torch.empty(B, T, d, device=dev)
    fns = {"narrow_attention": lambda: ops.narrow_attention(q, k, v, out, heads=H, dh=dh),
           "torch_composed": lambda: torch_attention(q, k, v, H, dh, dh ** -0.5)}
    if with_attention:
        fns["ops_attention"] = lambda: ops.attention(qkv, H, dh, out2)
    ws = alternating_us(fns)
    r = {"what": "narrow_attention", "B": B, "T": T, "heads": H, "dh": dh}
    for name, w in ws.items():
        r[name] = stat(w)
    fns["narrow_attention"]()
    want = torch_attention(q, k, v, H, dh, dh ** -0.5)
    r["vs_torch_max_abs"] = float((out - want).abs().max())
    if with_attention:
        fns["ops_attention"]()
        r["ops_attention_vs_torch_max_abs"] = float((out2 - want).abs().max())
        r["ops_attention_over_narrow"] = r["ops_attention"]["median_us"] / r["narrow_attention"]["median_us"]
    r["torch_over_narrow"] = r["torch_composed"]["median_us"] / r["narrow_attention"]["median_us"]
    # the medians differ by more than the run-to-run spread when the slowest narrow window is still faster than the fastest torch window
    r["narrow_max_below_torch_min"] = r["narrow_attention"]["max_us"] < r["torch_composed"]["min_us"]
    r["narrow_attention_TFLOPs"] = 2 * 2.0 * B * H * T * T * dh / r["narrow_attention"]["median_us"] / 1e6
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(U.ROOT, "profiles", "bench_sortformer.jsonl"))
    ap.add_argument("--kernel-only", action="store_true", help="skip the whole-model lines")
    a = ap.parse_args()
    ops.require_gpu()
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(1)
    lines = []

    def emit(r):
        lines.append(r)
        print(json.dumps(r))
        sys.stdout.flush()

    for B, T, att in ((1, 1125, False), (16, 1125, False), (1, 439, True), (16, 439, True)):
        emit(bench_kernel(dev, g, B, T, with_attention=att))
    if not a.kernel_only:
        eng = build()
        for B in (1, 16):
            feats = torch.randn(B, 80, MEL_1125, generator=g).to(dev)
            lens = [MEL_1125] * B
            assert eng(feats, lens).shape == (B, 1125, 4)
            ws = windows_us(lambda: eng(feats, lens), inner=2, repeats=5, warmup=2)
            emit({"what": "sortformer_offline", "B": B, "seconds": 90, "frames": 1125, "layers": [LAYERS, LAYERS],
                  **{k.replace("_us", "_ms"): v / 1e3 for k, v in stat(ws).items()}})
        state = eng.init_streaming_state()
        state.spkcache = torch.randn(1, 188, 512, generator=g).to(dev) * 0.5
        state.spkcache_preds = torch.rand(1, 188, 4, generator=g).to(dev)
        state.fifo = torch.randn(1, 188, 512, generator=g).to(dev) * 0.5
        state.fifo_preds = torch.rand(1, 188, 4, generator=g).to(dev)
        chunk = torch.randn(1, 80, 8 * 63 - 7, generator=g).to(dev)
        p, _ = eng.streaming_step(chunk, [chunk.shape[2]], state)
        assert p.shape == (63, 4)
        ws = windows_us(lambda: eng.streaming_step(chunk, [chunk.shape[2]], state), inner=2, repeats=5, warmup=2)
        emit({"what": "sortformer_streaming_step", "frames": [188, 188, 63], "layers": [LAYERS, LAYERS],
              **{k.replace("_us", "_ms"): v / 1e3 for k, v in stat(ws).items()}})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for r in lines:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
