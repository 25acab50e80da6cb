#!/usr/bin/env python
"""Times of the word-timestamp kernels (csrc/align.hip) at whisper-small sizes: T = 224 tokens, F = 1500 frames, dh = 64, with 72 alignment heads (the
default: every head of the last 6 layers) and with 10 (a typical published head set).

Steps, each in a child process of its own under its own time limit; the driver stops at the first one that fails:
  kernels   per-kernel times (QK softmax over all layers' launches, statistics + matrix, DTW, probability rows), event-timed medians
  torch     the same pipeline assembled from torch ops on the device + the numpy DTW of tests/_whisper_timing_ref.py on the host
  engine    ``WhisperEngine.align`` on a synthetic whisper-small against ``WhisperEngine.decode`` of the same window (224 steps): the share of a window

    python tools/bench_whisper_align.py [--out profiles/whisper_align_kernels.jsonl]

One JSON line per (step, head count) goes to stdout and to ``--out``."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

T, F, DH, H, LAYERS = 224, 1500, 64, 12, 12
STEP_LIMIT_S = {"kernels": 240, "torch": 300, "engine": 420}


def _timed_us(fn, inner, repeats=7, warmup=3):
    import torch

    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1000.0 / inner)
    return statistics.median(out)


def _heads(n):
    """n (layer, head) pairs spread over the last half of the decoder, layer-major."""
    allh = [(l, h) for l in range(LAYERS // 2, LAYERS) for h in range(H)]
    return allh if n >= len(allh) else sorted(allh[i * len(allh) // n] for i in range(n))


def _inputs(A, kv_dtype):
    import torch

    g = torch.Generator().manual_seed(0)
    q = torch.randn(1, T, H * DH, generator=g).cuda()
    k = torch.randn(1, H, F, DH, generator=g).to(kv_dtype).cuda()
    heads = _heads(A)
    per_layer = {}
    for s, (l, h) in enumerate(heads):
        per_layer.setdefault(l, []).append([h, s])
    pairs = [torch.tensor(v, dtype=torch.int32, device="cuda") for v in per_layer.values()]
    return q, k, pairs, len(heads)


def step_kernels():
    import torch

    from mlx_audio_amd import ops

    ops.require_gpu()
    for A in (72, 10):
        q, k, pairs, A = _inputs(A, torch.float16)
        w = torch.empty(1, A, T, F, device="cuda")
        cost = torch.empty(1, T - 4, F, device="cuda")
        stats = torch.empty(A * F * 2, device="cuda")
        ws = torch.empty(ops.dtw_workspace_bytes(T - 4, F, 1), dtype=torch.uint8, device="cuda")
        lg = torch.randn(T, 51868, device="cuda")
        tk = torch.randint(0, 50257, (T,), dtype=torch.int32, device="cuda")

        def qk():
            for p in pairs:
                ops.align_qk_softmax(q, k, w, p, heads=H, dh=DH, head_major=True)

        def matrix():
            ops.align_matrix(w, cost, row_begin=3, row_trim=1, stats=stats)

        qk()
        matrix()
        r = dict(step="kernels", heads=A, T=T, F=F, dh=DH, kv="f16", qk_launches=len(pairs),
                 qk_softmax_us=_timed_us(qk, 10), matrix_us=_timed_us(matrix, 10), dtw_us=_timed_us(lambda: ops.dtw(cost, ws=ws), 3),
                 prob_rows_us=_timed_us(lambda: ops.softmax_prob_rows(lg, tk, V=50257), 10))
        r["w_MB"] = A * T * F * 4 / 1e6
        r["qk_GFLOP"] = 2 * A * T * F * DH / 1e9
        print(json.dumps(r), flush=True)


def step_torch():
    import numpy as np
    import torch

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import _whisper_timing_ref as R

    for A in (72, 10):
        q, k, pairs, A = _inputs(A, torch.float32)
        heads = _heads(A)
        hs = torch.tensor([h for _, h in heads], device="cuda")
        qh = q.view(T, H, DH).permute(1, 0, 2)

        def device_part():
            s = torch.matmul(qh[hs], k[0, hs].transpose(1, 2)) * DH ** -0.5
            w = torch.softmax(s, dim=-1)
            std, mean = torch.std_mean(w, dim=-2, keepdim=True, unbiased=False)
            z = (w - mean) / std
            zp = torch.nn.functional.pad(z, (3, 3), mode="reflect")
            med = zp.unfold(-1, 7, 1).median(dim=-1).values
            return -med.mean(dim=0)[3:-1]

        m = device_part()
        dev_us = _timed_us(device_part, 5)
        x = m.cpu().numpy()
        t0 = time.perf_counter()
        R.dtw(x)
        host_dtw_us = (time.perf_counter() - t0) * 1e6
        print(json.dumps(dict(step="torch", heads=A, T=T, F=F, torch_device_ops_us=dev_us, host_numpy_dtw_us=host_dtw_us,
                              note="numpy DTW vectorised along anti-diagonals; the reference's is a per-cell Python loop")), flush=True)


def step_engine():
    import torch

    from mlx_audio_amd.stt.models.whisper import synthetic as WS
    from mlx_audio_amd.stt.models.whisper.engine import WhisperEngine
    from mlx_audio_amd.stt.models.whisper.tokenizer import get_tokenizer

    dims = WS.WHISPER_SMALL
    eng = WhisperEngine(WS.make_whisper_weights(dims, seed=0), dims, device="cuda")
    tok = get_tokenizer(True, language="en", task="transcribe")
    mel = WS.make_mel(1, seed=1).cuda()
    xa = eng.encode(mel)
    g = torch.Generator().manual_seed(3)
    text = torch.randint(0, 50257, (T - 5,), generator=g).tolist()
    full = [*tok.sot_sequence, tok.no_timestamps, *text, tok.eot]
    decode_us = _timed_us(lambda: eng.decode(None, tok, audio_features=xa, sample_len=T - 4, fixed_steps=True), 1, repeats=3, warmup=1)
    for A in (72, 10):
        heads = _heads(A)
        align_us = _timed_us(lambda: eng.align(xa, [full], [3000], heads, sot_len=3, eot=tok.eot), 1, repeats=5, warmup=2)
        print(json.dumps(dict(step="engine", heads=len(heads), tokens=len(full), align_pass_us=align_us, decode_window_us=decode_us,
                              align_over_decode=align_us / decode_us)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", choices=sorted(STEP_LIMIT_S), default=None, help="run one step in this process (what the driver starts)")
    a = ap.parse_args()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    if a.step:
        {"kernels": step_kernels, "torch": step_torch, "engine": step_engine}[a.step]()
        return 0
    lines = []
    for step in ("kernels", "torch", "engine"):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step], stdout=subprocess.PIPE, text=True, timeout=STEP_LIMIT_S[step])
        except subprocess.TimeoutExpired:
            print(f"step {step}: time limit of {STEP_LIMIT_S[step]} s; stopping", file=sys.stderr)
            return 124
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        lines += [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        if r.returncode != 0:
            print(f"step {step}: exit status {r.returncode}; stopping", file=sys.stderr)
            return r.returncode
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
