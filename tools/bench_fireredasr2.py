#!/usr/bin/env python
"""The four kernels of csrc/firered.hip at FireRedASR2-AED's published shapes (encoder 1280 wide, 20 heads of 64, 33 depthwise taps over 2560 channels,
subsampler of 32 channels over 80 mel bins, vocabulary 8667, beam 3) for 1 / 8 / 64 clips of 10 s, each against the composition it replaces on the
same tensors:

  * ``subsample2d_k3s2`` x 2 against ``torch.nn.functional.conv2d`` + ReLU x 2 + the (N, T, C, D) transpose copy;
  * ``glu_dwconv_ln_swish`` against ``glu`` + depthwise ``conv1d`` + ``layer_norm`` + ``silu`` from torch ops, and against the library's own separate
    launches where they exist (none does at 33 taps / 2560 channels, which is why the kernel was written);
  * ``beam_step`` against the reference's step from tensor ops (log-softmax with smoothing, two top-k, the finished mask, the history gathers);
  * ``beam_attention`` against a physical ``index_select`` of the fp32 k / v caches of one layer by ``beam_idx`` followed by ``flash_attention``.

Interleaved rounds in one process (both arms alternate inside every round), event-timed windows of at least 25 ms of device time each behind a warm-up;
the line records the median and the minimum of the rounds, the calls per window, and how far the two routes' outputs are apart.  Then ``generate_batch`` from waveforms at the published size (``bench_end_to_end``).

    python tools/bench_fireredasr2.py [--out-dir DIR]     # DIR receives bench_fireredasr2.jsonl
"""
import argparse
import json
import math
import os
import statistics

import torch

import _bench_util as U  # noqa: F401  (puts the repo root on sys.path)
from mlx_audio_amd import ops

D_MODEL, HEADS, DH, TAPS, SUB_C, MELS, VOCAB, BEAM = 1280, 20, 64, 33, 32, 80, 8667, 3
FRAMES = 998 + 6      # 10 s of 10 ms frames (snip_edges) and the encoder's six zero frames
T_DEC = 50            # decoded tokens so far (the issue's example)
SECONDS = 10


WINDOW_MS = 25.0      # every timed window holds at least this much device time (its call count comes from a first, untimed estimate)


def ab_us(arms, inner=None, rounds=9, warmup=3):
    """{name: (median, min)} in microseconds per call; the arms alternate inside every round.  ``inner`` calls per window: by default as many as
    fill WINDOW_MS for that arm, so that a window of a 15 us kernel is ~ 1700 calls and not a handful."""
    for fn in arms.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()

    def window(fn, n):
        e0, e1 = U.ev(), U.ev()
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1000.0 / n

    calls = {k: inner or max(10, int(math.ceil(WINDOW_MS * 1000.0 / window(fn, 20)))) for k, fn in arms.items()}
    out = {k: [] for k in arms}
    for _ in range(rounds):
        for name, fn in arms.items():
            out[name].append(window(fn, calls[name]))
    ab_us.last_calls = calls
    return {k: (statistics.median(v), min(v)) for k, v in out.items()}


def line(kernel, shape, res, new="hip", **extra):
    rec = dict(kernel=kernel, shape=shape, **{f"{k}_us_median": round(v[0], 2) for k, v in res.items()}, **{f"{k}_us_min": round(v[1], 2) for k, v in res.items()})
    for k, v in res.items():
        if k != new:
            rec[f"{k}_over_{new}"] = round(v[0] / res[new][0], 3)
    rec["calls_per_window"] = dict(getattr(ab_us, "last_calls", {}))
    rec.update(extra)
    return rec


def bench_subsample(B, dev, g):
    x = torch.randn(B, FRAMES, MELS, generator=g).to(dev)
    w1, b1 = (0.3 * torch.randn(SUB_C, 3, 3, 1, generator=g)).to(dev), (0.1 * torch.randn(SUB_C, generator=g)).to(dev)
    w2, b2 = (0.1 * torch.randn(SUB_C, 3, 3, SUB_C, generator=g)).to(dev), (0.1 * torch.randn(SUB_C, generator=g)).to(dev)
    T1, F1 = ops.subsample2d_out(FRAMES), ops.subsample2d_out(MELS)
    T2, F2 = ops.subsample2d_out(T1), ops.subsample2d_out(F1)
    y1, y2 = torch.empty(B, T1, F1, SUB_C, device=dev), torch.empty(B, T2, SUB_C, F2, device=dev)
    tw1, tw2 = w1.permute(0, 3, 1, 2).contiguous(), w2.permute(0, 3, 1, 2).contiguous()

    def hip():
        ops.subsample2d_k3s2(x, w1, b1, y1)
        ops.subsample2d_k3s2(y1, w2, b2, y2, out_cf=True)

    def torch_ops():
        h = torch.relu(torch.nn.functional.conv2d(x[:, None], tw1, b1, stride=2))
        h = torch.relu(torch.nn.functional.conv2d(h, tw2, b2, stride=2))
        return h.transpose(1, 2).reshape(B, T2, SUB_C * F2)

    err = float((torch_ops() - (hip() or y2.reshape(B, T2, -1))).abs().max())
    return line("subsample2d_k3s2 x 2", f"B={B} T={FRAMES} F={MELS} C={SUB_C}", ab_us(dict(hip=hip, torch=torch_ops)), max_abs_diff=err)


def bench_glu(B, dev, g):
    C, L = 2 * D_MODEL, ops.subsample2d_out(ops.subsample2d_out(FRAMES))
    x = torch.randn(B, L, 2 * C, generator=g).to(dev)
    w = (torch.randn(C, TAPS, generator=g) / math.sqrt(TAPS)).to(dev)
    lw, lb = (1.0 + 0.1 * torch.randn(C, generator=g)).to(dev), (0.1 * torch.randn(C, generator=g)).to(dev)
    y = torch.empty(B, L, C, device=dev)
    tw = w[:, None, :].contiguous()

    def hip():
        ops.glu_dwconv_ln_swish(x, w, lw, lb, y)

    def torch_ops():
        h = torch.nn.functional.glu(x, dim=-1).transpose(1, 2)
        h = torch.nn.functional.conv1d(h, tw, padding=(TAPS - 1) // 2, groups=C).transpose(1, 2)
        return torch.nn.functional.silu(torch.nn.functional.layer_norm(h, (C,), lw, lb, 1e-5))

    hip()
    err = float((torch_ops() - y).abs().max())
    compulsory = B * L * 3 * C * 4      # 2 C floats in, C floats out per row
    res = ab_us(dict(hip=hip, torch=torch_ops))
    return line("glu_dwconv_ln_swish", f"B={B} L={L} C={C} K={TAPS}", res, max_abs_diff=err, compulsory_bytes=compulsory,
                hip_compulsory_gb_per_s=round(compulsory / res["hip"][0] / 1e3, 1))


def bench_beam_step(N, dev, g):
    B, V, Tmax = BEAM, VOCAB, 256
    logits = (3.0 * torch.randn(N * B, V, generator=g)).to(dev)
    st = ops.beam_state(N, B, Tmax, [Tmax] * N, sos_id=3, device=dev)
    scores0 = (-torch.rand(N, B, generator=g) * 5).to(dev)
    ys = torch.randint(0, V, (N, B, T_DEC), generator=g).to(dev)
    conf = torch.rand(N, B, T_DEC, generator=g).to(dev)
    fin = torch.zeros(N, B, 1, device=dev)
    mask = torch.tensor([0.0] + [-1e10] * (B - 1), device=dev).view(1, 1, B)
    eos = 4

    def hip():
        st.step.fill_(T_DEC)          # every timed call is the same step: three tiny resets ride along, in this arm only
        st.done.zero_()
        st.scores.copy_(scores0)
        ops.beam_step(logits, st, eos_id=eos)

    def torch_ops():
        t = torch.log(torch.softmax(logits / 1.25, -1) + 1e-10).view(N, B, V)
        top, idx = torch.topk(t, B, dim=-1)
        top = top * (1 - fin) + mask * fin
        idx = idx * (1 - fin.long()) + eos * fin.long()
        best, bidx = torch.topk((scores0[:, :, None] + top).view(N, B * B), B, dim=-1)
        beam = bidx // B
        new = torch.gather(idx.view(N, B * B), 1, bidx)
        nconf = torch.exp(torch.gather(top.view(N, B * B), 1, bidx))
        ys2 = torch.cat([torch.gather(ys, 1, beam[:, :, None].expand(N, B, T_DEC)), new[:, :, None]], -1)
        cf2 = torch.cat([torch.gather(conf, 1, beam[:, :, None].expand(N, B, T_DEC)), nconf[:, :, None]], -1)
        return best, beam, ys2, cf2, (new == eos)

    # the same step on both routes: decisions equal (random logits: no ties), values to float32 rounding
    hip()
    best, beam, ys2, cf2, _ = torch_ops()
    dst = st.cur
    same = bool(torch.equal(st.beam_idx.long(), beam) and torch.equal(st.tokens[dst][:, :, T_DEC].long(), ys2[:, :, T_DEC]))
    err = float((st.scores - best).abs().max())
    cerr = float((st.new_conf - cf2[:, :, T_DEC]).abs().max())
    return line("beam_step", f"N={N} B={B} V={V} step={T_DEC}", ab_us(dict(hip=hip, torch=torch_ops)), decisions_equal=same, max_abs_diff_scores=err,
                max_abs_diff_conf=cerr)


def bench_beam_attention(N, dev, g):
    B, C, Tcap = BEAM, HEADS * DH, 64
    q = torch.randn(N * B, C, generator=g).to(dev)
    k, v = torch.randn(N * B, Tcap, C, generator=g).to(dev), torch.randn(N * B, Tcap, C, generator=g).to(dev)
    ind = torch.randint(0, B, (N, B, Tcap), generator=g, dtype=torch.int32).to(dev)
    pos = torch.full((N,), T_DEC - 1, dtype=torch.int32, device=dev)
    lens = torch.full((N * B,), T_DEC, dtype=torch.int32, device=dev)
    src = (torch.randint(0, B, (N, B), generator=g) + B * torch.arange(N)[:, None]).reshape(-1).to(dev)
    out, out2 = torch.empty(N * B, C, device=dev), torch.empty(N * B, 1, C, device=dev)
    k2, v2 = torch.empty_like(k), torch.empty_like(v)

    def hip():
        ops.beam_attention(q, k, v, ind, pos, out, beams=B, heads=HEADS, dh=DH)

    def gather_then_flash():
        torch.index_select(k, 0, src, out=k2)      # one layer's fp32 caches, re-gathered by beam_idx as the reference does every step
        torch.index_select(v, 0, src, out=v2)
        ops.flash_attention(q[:, None], k2, v2, out2, heads=HEADS, dh=DH, lens_k=lens)

    def flash_only():
        ops.flash_attention(q[:, None], k, v, out2, heads=HEADS, dh=DH, lens_k=lens)

    # the same function on both routes: caches gathered position by position as `ind` says, then flash_attention
    rows = (ind.long() + B * torch.arange(N, device=dev)[:, None, None]).reshape(N * B, Tcap)
    kg = k[rows, torch.arange(Tcap, device=dev)[None, :]].contiguous()
    vg = v[rows, torch.arange(Tcap, device=dev)[None, :]].contiguous()
    hip()
    ops.flash_attention(q[:, None], kg, vg, out2, heads=HEADS, dh=DH, lens_k=lens)
    err = float((out - out2[:, 0]).abs().max())
    res = ab_us(dict(hip=hip, gather_flash=gather_then_flash, flash_only=flash_only))
    return line("beam_attention", f"N={N} B={B} heads={HEADS} dh={DH} keys={T_DEC} (cache rows {Tcap})", res,
                gathered_bytes_per_layer=2 * 2 * N * B * Tcap * C * 4, max_abs_diff=err)


def synth_clip(seed, n):
    import numpy as np

    rng = np.random.default_rng(seed)
    t = np.arange(n) / 16000.0
    x = 0.05 * rng.standard_normal(n)
    for _ in range(4):
        x += rng.uniform(0.05, 0.25) * np.sin(2 * np.pi * rng.uniform(80, 3000) * t + rng.uniform(0, 6.28))
    return np.clip(x, -1, 1).astype("float32")


def bench_end_to_end(batches, dev):
    """Waveform to text at the published size (16 + 16 layers, 1280 wide, 20 heads of 64, vocabulary 8667, beam 3) on seeded weights: the 16 layers of
    each side are copies of one seeded layer in separate device memory.  Random weights do not end by EOS, so every utterance decodes ``max_len`` = 50
    tokens (the issue's example); wall clock around synchronised calls, upload and fbank included."""
    import time

    from mlx_audio_amd.stt.models.fireredasr2 import ModelConfig, make_fireredasr2_weights
    from mlx_audio_amd.stt.models.fireredasr2.fireredasr2 import Model

    c = ModelConfig.from_dict(dict(encoder=dict(n_layers=1), decoder=dict(n_layers=1)))
    model = Model(c, make_fireredasr2_weights(c, 0, logit_gain=20.0), device=dev)
    clone = lambda blk: {k: U._clone_obj(v) for k, v in blk.items()}
    model.enc_layers = [model.enc_layers[0]] + [clone(model.enc_layers[0]) for _ in range(15)]
    model.dec_layers = [model.dec_layers[0]] + [clone(model.dec_layers[0]) for _ in range(15)]
    model._tokenizer = [f"w{i} " for i in range(c.odim)]
    out = []
    for N in batches:
        clips = [synth_clip(100 + i, SECONDS * 16000) for i in range(N)]
        model.generate_batch(clips, beam_size=BEAM, max_len=T_DEC)            # warm-up
        times, enc_times = [], []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = model.generate_batch(clips, beam_size=BEAM, max_len=T_DEC)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            model.encode(clips)
            torch.cuda.synchronize()
            enc_times.append(time.perf_counter() - t0)
        t, te = statistics.median(times), statistics.median(enc_times)
        out.append(dict(kernel="end to end (waveform to text)", shape=f"N={N} x {SECONDS} s, beam {BEAM}, {T_DEC} decoded tokens, 16 + 16 layers",
                        ms_median=round(t * 1e3, 2), ms_min=round(min(times) * 1e3, 2), audio_seconds_per_second=round(N * SECONDS / t, 1),
                        encode_ms_median=round(te * 1e3, 2), decode_ms_per_step=round((t - te) * 1e3 / T_DEC, 3), tokens=[r.generation_tokens for r in res][:4]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-model", action="store_true", help="kernels only")
    ap.add_argument("--out-dir", default=os.path.join(U.ROOT, "profiles"))
    ap.add_argument("--batches", default="1,8,64")
    args = ap.parse_args()
    ops.require_gpu()
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    os.makedirs(args.out_dir, exist_ok=True)
    path = os.path.join(args.out_dir, "bench_fireredasr2.jsonl")
    with open(path, "w") as f:
        for B in [int(b) for b in args.batches.split(",")]:
            for fn in (bench_subsample, bench_glu, bench_beam_step, bench_beam_attention):
                rec = fn(B, dev, g)
                print(json.dumps(rec), flush=True)
                f.write(json.dumps(rec) + "\n")
        if not args.no_model:
            for rec in bench_end_to_end([int(b) for b in args.batches.split(",")], dev):
                print(json.dumps(rec), flush=True)
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
