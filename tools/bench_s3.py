#!/usr/bin/env python
"""The two kernels of csrc/s3.hip in one process, alternating with what they are measured against: ``fsmn_memory`` against (a) a device copy of the same
bytes and (b) the composition it replaces (``ops.dwconv`` over the zero-padded masked values + the elementwise adds and masks giving the same tensor);
``fsq_encode`` against a device copy of the hidden state.  Medians over repeats of event-timed windows; one JSON line per shape."""
import json
import statistics

import torch

import _bench_util as U  # noqa: F401  (puts the repo root on sys.path)
from mlx_audio_amd import ops


def timed_us(fn, inner=20, repeats=9, warmup=5):
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


def main():
    ops.require_gpu()
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    K = 31
    for B, L, C in ((64, 250, 1280), (1, 750, 1280)):
        qkv = torch.randn(B, L, 3 * C, generator=g).to(dev)
        v = qkv[:, :, 2 * C:]
        x, y = torch.randn(B, L, C, generator=g).to(dev), torch.empty(B, L, C, device=dev)
        w = (0.1 * torch.randn(C, K, generator=g)).to(dev)
        lens = torch.full((B,), L, dtype=torch.int32, device=dev)
        lens[B // 2:] = max(L - 37, 1)
        mask = (torch.arange(L, device=dev)[None, :] < lens[:, None])[:, :, None].to(torch.float32)
        vm, conv = torch.empty(B, L, C, device=dev), torch.empty(B, L, C, device=dev)

        def composed():
            torch.mul(v, mask, out=vm)                      # inputs * mask
            ops.dwconv(vm, w, None, conv, pad=(K - 1) // 2)  # the 31-tap depthwise conv, zero padded
            conv.add_(vm).mul_(mask)                         # + inputs, * mask
            return torch.add(x, conv, out=y)                 # the residual stream

        ops.fsmn_memory(v, w, y, add=x, lens=lens)
        got = y.clone()
        assert float((composed() - got).abs().max()) < 1e-4
        wq, bq = torch.randn(8, C, generator=g).to(dev) / C ** 0.5, torch.zeros(8, device=dev)
        mb = x.numel() * 4 / 1e6
        r = {"shape": [B, L, C], "MB": mb,
             "copy_us": timed_us(lambda: y.copy_(x)),
             "fsmn_us": timed_us(lambda: ops.fsmn_memory(v, w, y, add=x, lens=lens)),
             "dwconv_composition_us": timed_us(composed),
             "copy_again_us": timed_us(lambda: y.copy_(x)),
             "fsmn_again_us": timed_us(lambda: ops.fsmn_memory(v, w, y, add=x, lens=lens)),
             "fsq_us": timed_us(lambda: ops.fsq_encode(x, wq, bq, lens=lens)),
             "read_only_copy_us": timed_us(lambda: vm.copy_(x))}
        r["fsmn_GBps"] = 3 * mb / r["fsmn_us"] * 1e3 / 1e3   # read v, read add, write y
        r["fsmn_vs_copy"] = r["fsmn_us"] / r["copy_us"]
        r["fsmn_vs_composition"] = r["fsmn_us"] / r["dwconv_composition_us"]
        r["fsq_GBps"] = mb / r["fsq_us"] * 1e3 / 1e3
        r["fsq_vs_copy"] = r["fsq_us"] / r["copy_us"]
        print(json.dumps(r))


if __name__ == "__main__":
    main()
