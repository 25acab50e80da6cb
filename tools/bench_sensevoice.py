#!/usr/bin/env python
"""SenseVoice-Small at the published size (560 -> 512, 4 heads of 128, FFN 2048, K 11, 50 + 20 layers, vocabulary 25 055) on seeded weights, 10 s clips
at B = 1, 8, 64: ``generate_batch`` from waveforms (audio-seconds per second, entry-point calls per clip) and the pass behind the fbank; then each kernel
of csrc/sanm.hip against the torch composition it replaces, on the same tensors, at 171 rows (one clip) and 64 x 171 rows and the published vocabulary:
``ctc_rows`` + ``ctc_collapse`` + one copy against ``log_softmax`` + ``argmax`` + ``.tolist()`` + the host collapse loop, ``sanm_input`` against the
gathered / stacked assembly, and the CTC head (``ctc_lo`` GEMM + ``ctc_rows``) at every row-chunk size tried.  Medians over repeats of event-timed (or,
where the host takes part, synchronised wall-clock) windows behind a warm-up.  The 70 layers are copies of three seeded layers in separate device memory.

    python tools/bench_sensevoice.py [--out-dir DIR]     # DIR receives bench_sensevoice.jsonl and sanm_kernels_vs_torch.jsonl
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

import _bench_util as U  # noqa: F401  (puts the repo root on sys.path)
from mlx_audio_amd import _lib, ops
from mlx_audio_amd.stt.models.sensevoice import ModelConfig, SenseVoiceSmall, make_sensevoice_weights
from mlx_audio_amd.stt.models.sensevoice.sensevoice import CTC_CHUNK_ROWS, position_table

SECONDS, FS = 10, 16000
CHUNKS = (256, 512, 1024, 2048, 4096, 1 << 30)


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


def wall_us(fn, inner=3, repeats=7, warmup=2):
    """For work that ends on the host (a copy, a Python loop): wall clock around synchronised windows."""
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


def build(dev):
    cfg = ModelConfig.from_dict(dict(encoder_conf=dict(num_blocks=2, tp_blocks=1)))
    eng = SenseVoiceSmall(cfg, make_sensevoice_weights(cfg, 0, blank_bias=15.5), device=dev)
    clone = lambda blk: {k: U._clone_obj(v) for k, v in blk.items()}
    eng.layers = [eng.layers[0]] + [clone(eng.layers[1]) for _ in range(49)] + [clone(eng.layers[2]) for _ in range(20)]
    cfg.encoder_conf.num_blocks, cfg.encoder_conf.tp_blocks = 50, 20
    g = torch.Generator().manual_seed(3)
    eng.set_cmvn((-12.0 + torch.randn(560, generator=g)).tolist(), (0.25 + 0.05 * torch.rand(560, generator=g)).tolist())
    return eng


class CallCounter:
    """Counts the library's entry-point calls (one or, for a split GEMM, two launches each)."""

    def __enter__(self):
        self.n, self.saved = 0, _lib.call_struct

        def counted(*a, **k):
            self.n += 1
            return self.saved(*a, **k)

        _lib.call_struct = counted
        return self

    def __exit__(self, *a):
        _lib.call_struct = self.saved


def host_collapse(ids_rows, blank=0):
    """The reference's loop (``_greedy_ctc_decode``) on one clip's ``.tolist()``."""
    out, prev = [], None
    for t in ids_rows:
        if t != prev:
            if t != blank:
                out.append(t)
            prev = t
    return out


def torch_assembly(feats, lens, means, istd, embed, qids, pe, m, n, scale):
    """The stacked / gathered input assembly from torch ops, batched: an index table, a gather, CMVN, the query rows, scale, positions, the mask."""
    B, T, D = feats.shape
    R = -(-T // n)
    dev = feats.device
    idx = torch.arange(R, device=dev)[None, :, None] * n + torch.arange(m, device=dev)[None, None, :] - (m - 1) // 2
    idx = torch.minimum(idx.clamp_min(0), (lens[:, None, None] - 1).long())
    x = torch.gather(feats, 1, idx.reshape(B, R * m, 1).expand(B, R * m, D)).reshape(B, R, m * D)
    x = (x + means) * istd
    x = torch.cat([embed[qids.long()], x], dim=1) * scale + pe[:R + 4]
    valid = torch.arange(R + 4, device=dev)[None, :] < (4 + (lens + n - 1) // n)[:, None]
    return x * valid[:, :, None]


def model_lines(eng, dev):
    g = torch.Generator().manual_seed(1)
    lines = []
    for B in (1, 8, 64):
        t = torch.arange(SECONDS * FS, dtype=torch.float32) / FS
        audios = [(0.05 * torch.randn(SECONDS * FS, generator=g) + 0.2 * torch.sin(2 * math.pi * (200 + 13 * b) * t)) for b in range(B)]
        fbs = [eng._fbank(a) for a in audios]
        with CallCounter() as cc:
            outs = eng.generate_batch(audios, language="auto")
        r = {"what": "sensevoice_small_published_size", "B": B, "seconds": SECONDS, "fbank_frames": int(fbs[0].shape[0]), "rows_per_clip": ops.sanm_rows(fbs[0].shape[0], 6),
             "layers": "50 + 20", "ctc_chunk_rows": eng.ctc_chunk_rows, "entry_point_calls_per_clip": cc.n / B, "tokens_first_clip": len(outs[0].text.split())}
        r["generate_batch_ms"] = wall_us(lambda: eng.generate_batch(audios, language="auto"), inner=2, repeats=5, warmup=2) / 1e3
        r["behind_fbank_ms"] = wall_us(lambda: eng.transcribe_fbank(fbs, "auto", False), inner=2, repeats=5, warmup=2) / 1e3
        r["audio_seconds_per_second"] = B * SECONDS / (r["generate_batch_ms"] / 1e3)
        r["audio_seconds_per_second_behind_fbank"] = B * SECONDS / (r["behind_fbank_ms"] / 1e3)
        lines.append(r)
        print(json.dumps(r), flush=True)
    return lines


def kernel_lines(eng, dev):
    V, d, W = eng.config.vocab_size, eng.config.encoder_conf.output_size, eng.config.input_size
    g = torch.Generator().manual_seed(2)
    lines = []
    for B in (1, 64):
        R = 171
        rows = B * R
        r = {"what": "sanm_kernels_vs_torch", "B": B, "rows": rows, "V": V}
        hidden = torch.randn(B, R, d, generator=g).to(dev)
        logits = torch.empty(rows, ops.round_up(V, 64), device=dev)[:, :V]   # rows 16-byte aligned, as in the engine's workspace
        ops.conv_gemm(hidden.view(1, rows, d), eng.ctc_lo, logits[None], precision=eng.precision)
        lens = torch.full((B,), R, dtype=torch.int32, device=dev)
        # the head behind the GEMM: device time, then everything up to host token lists
        r["ctc_rows_us"] = timed_us(lambda: ops.ctc_rows(logits))
        r["ctc_rows_GBps"] = rows * V * 4 / r["ctc_rows_us"] / 1e3
        r["torch_log_softmax_argmax_us"] = timed_us(lambda: torch.argmax(torch.log_softmax(logits, dim=-1), dim=-1))
        r["ctc_rows_vs_torch"] = r["ctc_rows_us"] / r["torch_log_softmax_argmax_us"]
        ids = ops.ctc_rows(logits)[0]
        want = torch.argmax(torch.log_softmax(logits, dim=-1), dim=-1)
        r["ids_equal_torch"] = bool((ids.long() == want).all())
        r["ctc_collapse_us"] = timed_us(lambda: ops.ctc_collapse(ids.view(B, R), lens=lens, skip=4))

        def ours():
            i = ops.ctc_rows(logits)[0].view(B, R)
            tok, cnt = ops.ctc_collapse(i, lens=lens, skip=4)
            host = torch.cat([cnt[:, None], tok], dim=1).cpu()
            return [host[b, 1:1 + int(host[b, 0])].tolist() for b in range(B)]

        def theirs():
            lp = torch.log_softmax(logits, dim=-1).reshape(B, R, V)
            return [host_collapse(torch.argmax(lp[b, 4:], dim=-1).tolist()) for b in range(B)]

        r["tokens_equal_torch"] = ours() == theirs()
        r["head_to_host_tokens_us"] = wall_us(ours)
        r["torch_head_to_host_tokens_us"] = wall_us(theirs)
        r["head_to_host_vs_torch"] = r["head_to_host_tokens_us"] / r["torch_head_to_host_tokens_us"]
        # the GEMM + ctc_rows at every row-chunk size (a fixed workspace of that many rows)
        tried = {}
        for c in CHUNKS:
            if c != CHUNKS[-1] and c >= rows:
                continue
            eng.ctc_chunk_rows, eng._ctc_ws = c, None
            tried["all" if c == CHUNKS[-1] else str(c)] = timed_us(lambda: eng.head(hidden), inner=3, repeats=5, warmup=2)
        eng.ctc_chunk_rows, eng._ctc_ws = CTC_CHUNK_ROWS, None
        r["head_gemm_plus_ctc_rows_us_by_chunk_rows"] = tried
        r["chosen_chunk_rows"] = CTC_CHUNK_ROWS
        r["torch_head_full_matrix_us"] = timed_us(lambda: torch.argmax(torch.log_softmax(ops.conv_gemm(hidden.view(1, rows, d), eng.ctc_lo, logits[None], precision=eng.precision)[0], dim=-1), dim=-1),
                                                  inner=3, repeats=5, warmup=2)
        del logits
        # the input assembly
        T = 998
        feats = (12.0 + 4.0 * torch.randn(B, T, 80, generator=g)).to(dev)
        flens = torch.full((B,), T, dtype=torch.int32, device=dev)
        if B > 1:
            flens[1::2] = T - 37
        qids = torch.tensor([[0, 1, 2, 15]] * B, dtype=torch.int32, device=dev)
        pe = position_table(256, W).to(dev)
        scale = math.sqrt(d)
        x = torch.empty(B, ops.sanm_rows(T, 6), W, device=dev)
        run = lambda: ops.sanm_input(feats, eng.embed, qids, pe, lfr_m=7, lfr_n=6, scale=scale, lens=flens, means=eng._cmvn_means, istd=eng._cmvn_istd, x=x)
        comp = lambda: torch_assembly(feats, flens, eng._cmvn_means, eng._cmvn_istd, eng.embed, qids, pe, 7, 6, scale)
        run()
        r["sanm_input_vs_torch_max_abs"] = float((x - comp()).abs().max())
        r["sanm_input_us"] = timed_us(run)
        r["torch_assembly_us"] = timed_us(comp)
        r["sanm_input_vs_torch"] = r["sanm_input_us"] / r["torch_assembly_us"]
        r["sanm_input_GBps"] = (x.numel() + feats.numel()) * 4 / r["sanm_input_us"] / 1e3
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
    eng = build(dev)
    k = kernel_lines(eng, dev)
    m = [] if a.skip_model else model_lines(eng, dev)
    if a.out_dir:
        os.makedirs(a.out_dir, exist_ok=True)
        for name, lines in (("sanm_kernels_vs_torch.jsonl", k), ("bench_sensevoice.jsonl", m)):
            if lines:
                with open(os.path.join(a.out_dir, name), "w") as f:
                    f.write("".join(json.dumps(x) + "\n" for x in lines))


if __name__ == "__main__":
    sys.exit(main())
