#!/usr/bin/env python
"""Granite Speech NAR on seeded weights.

(a) ``shaw_block_attention`` at the published encoder shape (8 heads of 128, context 200, 30 s = 1500 frames, B = 1 and 16) against the route the
    library had before it: a flipped, head-tiled copy of the Shaw table and two zero bias vectors (built once, outside the timed window), a
    zero-filled copy of the fused q | k | v buffer padded to a multiple of the context (inside the timed window: it is needed on every call), and
    ``relpos_attention`` over [B * blocks, ctx] with every key visible.  Both write the same numbers for full-length items (the difference is
    reported); the old route has no rule for a ragged batch.
(b) ``generate_batch`` from waveforms at the two test-sized configurations and at the published widths cut to one encoder / projector / editor layer
    and a vocabulary of 4096, with the share of the front end, the encoder with its BPE head, the projector and the editor.

Medians over repeats of event-timed (or, where the host takes part, synchronised wall-clock) windows behind a warm-up.

    python tools/bench_granite_nar.py [--out-dir DIR]     # DIR receives bench_granite_nar.jsonl
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

import _bench_util as U  # noqa: F401  (puts the repo root on sys.path)
from mlx_audio_amd import ops
from mlx_audio_amd.stt.models.granite_speech_nar import GraniteSpeechNar as Model, ModelConfig, add_insertion_slots, make_granite_nar_weights

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import _granite_nar_ref as R  # noqa: E402  (the test-sized and the published configurations, the synthetic clips)


def timed_us(fn, inner=5, repeats=7, warmup=3):
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


def wall_us(fn, inner=2, repeats=5, warmup=2):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e6 / inner)
    return statistics.median(out)


def attention_lines(dev):
    H, dh, ctx, max_pos, T = 8, 128, 200, 512, 1500
    hd = H * dh
    g = torch.Generator().manual_seed(0)
    table = (0.5 * torch.randn(2 * max_pos + 1, dh, generator=g)).to(dev)
    lines = []
    for B in (1, 16):
        qkv = torch.randn(B, T, 3 * hd, generator=g).to(dev)
        out = torch.empty(B, T, hd, device=dev)
        ours = lambda: ops.shaw_block_attention(qkv[..., :hd], qkv[..., hd:2 * hd], qkv[..., 2 * hd:], table, out, heads=H, dh=dh, ctx=ctx, max_pos=max_pos)
        # the previous route: relpos_attention reads row center - (i - j), so its table is the Shaw table flipped, cut to the 2 ctx - 1 distances of a
        # block and tiled over the heads; the biases are zero
        nb = -(-T // ctx)
        p = table[max_pos - (ctx - 1):max_pos + ctx].flip(0).repeat(1, H).contiguous()
        zero = torch.zeros(hd, device=dev)
        padded = torch.empty(B, nb * ctx, 3 * hd, device=dev)
        out2 = torch.empty(B * nb, ctx, hd, device=dev)

        def copies():
            padded[:, T:].zero_()
            padded[:, :T].copy_(qkv)

        def attn_only():
            v = padded.view(B * nb, ctx, 3 * hd)
            ops.relpos_attention(v[..., :hd], v[..., hd:2 * hd], v[..., 2 * hd:], p, zero, zero, out2, heads=H, dh=dh, center=ctx - 1)

        def route():
            copies()
            attn_only()

        ours()
        route()
        r = {"what": "shaw_block_attention_vs_relpos_route", "B": B, "T": T, "heads": H, "dh": dh, "ctx": ctx, "max_pos": max_pos,
             "max_abs_diff": float((out2.view(B, nb * ctx, hd)[:, :T] - out).abs().max())}
        r["shaw_block_attention_us"] = timed_us(ours)
        r["relpos_route_us"] = timed_us(route)
        r["relpos_route_attention_only_us"] = timed_us(attn_only)
        r["relpos_route_copies_us"] = timed_us(copies)
        r["shaw_vs_route"] = r["shaw_block_attention_us"] / r["relpos_route_us"]
        r["shaw_vs_route_attention_only"] = r["shaw_block_attention_us"] / r["relpos_route_attention_only_us"]
        # q k^T, q table^T over the band (two 64-row blocks per 32 keys) and p v: multiply-adds per (query, key) pair = dh (1 + 2 + 1), over padded blocks
        r["shaw_tflops"] = 2.0 * B * H * nb * ctx * ctx * dh * 4 / r["shaw_block_attention_us"] / 1e6
        lines.append(r)
        print(json.dumps(r), flush=True)
    return lines


def model_lines(dev):
    lines = []
    cases = [("test_config_A", R.config_dict("A"), R.WEIGHTS["A"]), ("test_config_B", R.config_dict("B"), R.WEIGHTS["B"]),
             ("published_widths_one_layer_each_vocab_4096", R.published_config_dict(), dict(seed=1, head_gain=6.0, bpe_blank_bias=3.0, embed_gain=0.02))]
    for name, d, wkw in cases:
        cfg = ModelConfig.from_dict(d)
        model = Model(cfg, make_granite_nar_weights(cfg, **wkw), device=dev)
        model._tokenizer = R.ListTokenizer()
        for B, seconds in ((1, 5), (16, 5)):
            clips = [R.synth_audio(seconds * R.FS, 100 + b) for b in range(B)]
            feats, lens = model._pad([model._compute_features(c) for c in clips])
            x = feats.to(torch.bfloat16).to(torch.float32)
            enc = model.encode(x, lens)
            audio, alens = model.project(enc["fused"], lens)
            text_ids = [add_insertion_slots(h, cfg.blank_token_id, cfg.min_edit_sequence_length) for h in enc["hyp"]]
            r = {"what": "granite_speech_nar_generate_batch", "config": name, "B": B, "seconds": seconds, "frames": lens[0],
                 "hypothesis_tokens_first_clip": len(enc["hyp"][0])}
            r["generate_batch_ms"] = wall_us(lambda: model.generate_batch(clips)) / 1e3
            stage = {"front_end": wall_us(lambda: [model._compute_features(c) for c in clips]), "encoder_and_bpe_head": wall_us(lambda: model.encode(x, lens)),
                     "projector": wall_us(lambda: model.project(enc["fused"], lens)), "editor": wall_us(lambda: model.edit(audio, alens, text_ids))}
            total = sum(stage.values())
            r["stage_ms"] = {k: v / 1e3 for k, v in stage.items()}
            r["stage_share"] = {k: v / total for k, v in stage.items()}
            r["audio_seconds_per_second"] = B * seconds / (r["generate_batch_ms"] / 1e3)
            lines.append(r)
            print(json.dumps(r), flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=None)
    ap.add_argument("--skip-model", action="store_true")
    a = ap.parse_args()
    ops.require_gpu()
    dev = torch.device("cuda", 0)
    lines = attention_lines(dev) + ([] if a.skip_model else model_lines(dev))
    if a.out_dir:
        os.makedirs(a.out_dir, exist_ok=True)
        with open(os.path.join(a.out_dir, "bench_granite_nar.jsonl"), "w") as f:
            f.write("".join(json.dumps(x) + "\n" for x in lines))


if __name__ == "__main__":
    sys.exit(main())
