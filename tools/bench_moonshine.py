#!/usr/bin/env python
"""Moonshine at the published widths (tiny: 288 wide, 8 heads of 36, 6 + 6 layers; base: 416 wide, 8 heads of 52, 8 + 8 layers; vocabulary 32768)
on seeded weights, and its attention kernel against the route the library offered before it.

  * the encoder (stem + layers) at 8 x 30 s, and the waveform upload in front of it;
  * one decode step (all decoder layers + logits + arg-max) at B = 1 and 8 over 30 s of encoder output with 32 tokens in the cache, and the
    entry-point calls one step makes (counted at ``_lib.call_struct`` and ``ops.swiglu``: a lower bound on its launches, the torch gather / copies
    around them are not counted);
  * ``mid_attention`` against ``flash_attention`` on the same heads zero-padded to 64 channels with ``scale = dh ** -0.5`` (the same function: the
    padded channels add 0 to every score and produce output columns nobody reads): the encoder shape (T = 1250, B = 8, 8 heads, q | k | v thirds
    of one fused buffer on both routes, with and without per-item lengths) and one-query decode steps over 200 and 1250 keys at B = 1 and 8;
  * ``partial_rope`` on the encoder's q | k (in place) at the same shape.

The candidates of a line take turns window by window in one process; every time is the median of event-timed windows behind a warm-up, with the
windows' own (min, max).  The clock is whatever the device runs at under this load (not pinned, not read).  One JSON line per configuration, printed
and written to ``--out`` (default ``profiles/bench_moonshine.jsonl``, rewritten per run)."""
import argparse
import json
import os
import statistics
import sys

import torch

import _bench_util as U
from mlx_audio_amd import ops


def alternating_us(fns, inner=20, repeats=11, warmup=3):
    """name -> window times, the candidates taking turns window by window (whatever else shares the machine hits all of them alike)."""
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
    return out


def stat(ws):
    return dict(median_us=statistics.median(ws), min_us=min(ws), max_us=max(ws))


def padded(x, H, dh):
    """[B, T, H dh] -> [B, T, H 64], every head's channels dh .. 63 zero."""
    B, T, _ = x.shape
    out = torch.zeros(B, T, H, 64, device=x.device)
    out[..., :dh] = x.reshape(B, T, H, dh)
    return out.reshape(B, T, H * 64)


def bench_attention(dev, g, what, B, Tq, Tk, H, dh, lens_k=None):
    d = H * dh
    if Tq == Tk:   # thirds of one fused projection buffer, on both routes
        buf = torch.randn(B, Tq, 3 * d, generator=g).to(dev)
        q, k, v = buf[:, :, :d], buf[:, :, d:2 * d], buf[:, :, 2 * d:]
        pbuf = torch.cat([padded(t, H, dh) for t in (q, k, v)], dim=2)
        qp, kp, vp = pbuf[:, :, :H * 64], pbuf[:, :, H * 64:2 * H * 64], pbuf[:, :, 2 * H * 64:]
    else:
        q = torch.randn(B, Tq, d, generator=g).to(dev)
        k, v = torch.randn(B, Tk, d, generator=g).to(dev), torch.randn(B, Tk, d, generator=g).to(dev)
        qp, kp, vp = padded(q, H, dh), padded(k, H, dh), padded(v, H, dh)
    lk = None if lens_k is None else torch.tensor(lens_k, dtype=torch.int32, device=dev)
    lq = lk if Tq == Tk else None
    out, outp = torch.empty(B, Tq, d, device=dev), torch.empty(B, Tq, H * 64, device=dev)
    fns = {"mid_attention": lambda: ops.mid_attention(q, k, v, out, heads=H, dh=dh, lens_q=lq, lens_k=lk, check_lens=False),
           "flash_padded_64": lambda: ops.flash_attention(qp, kp, vp, outp, heads=H, dh=64, scale=dh ** -0.5, lens_q=lq, lens_k=lk)}
    ws = alternating_us(fns)
    r = {"what": what, "B": B, "Tq": Tq, "Tk": Tk, "heads": H, "dh": dh, "lens_k": lens_k}
    for name, w in ws.items():
        r[name] = stat(w)
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    got, ref = out.reshape(B, Tq, H, dh), outp.reshape(B, Tq, H, 64)[..., :dh]
    if lens_k is not None and Tq == Tk:   # flash_attention leaves the rows beyond lens_q alone, mid_attention zeroes them
        keep = torch.arange(Tq, device=dev)[None, :] < lk[:, None]
        got, ref = got[keep], ref[keep]
    r["routes_max_abs_diff"] = float((got - ref).abs().max())
    r["flash_padded_over_mid"] = r["flash_padded_64"]["median_us"] / r["mid_attention"]["median_us"]
    # the medians differ by more than the run-to-run spread when the slower route's fastest window is still slower than the faster route's slowest
    r["spread_separates_them"] = (r["mid_attention"]["max_us"] < r["flash_padded_64"]["min_us"]) or (r["flash_padded_64"]["max_us"] < r["mid_attention"]["min_us"])
    r["mid_attention_TFLOPs"] = 2 * 2.0 * B * H * Tq * Tk * dh / r["mid_attention"]["median_us"] / 1e6
    return r


def bench_rope(dev, g, B, T, H, dh, rot):
    d = H * dh
    buf = torch.randn(B, T, 3 * d, generator=g).to(dev)
    q, k = buf[:, :, :d], buf[:, :, d:2 * d]
    cos, sin = ops.moonshine_rope_tables(rot, T, device=dev)
    ws = alternating_us({"partial_rope": lambda: ops.partial_rope(q, q, heads=H, dh=dh, rot=rot, cos=cos, sin=sin, second=(k, k, H))})
    r = {"what": "partial_rope_q_k_in_place", "B": B, "T": T, "heads": H, "dh": dh, "rot": rot, "partial_rope": stat(ws["partial_rope"])}
    r["GBps_read_plus_write"] = 2 * 4.0 * B * T * 2 * d / r["partial_rope"]["median_us"] / 1e3
    return r


def bench_model(dev, g, name, cfg_kw):
    from mlx_audio_amd import _lib
    from mlx_audio_amd.stt.models.moonshine.moonshine import Model, ModelConfig, make_moonshine_weights

    c = ModelConfig.from_dict(cfg_kw)
    model = Model(c, make_moonshine_weights(c, 0), device=dev)
    out = []
    clips = [torch.randn(480000, generator=g) * 0.1 for _ in range(8)]
    buf, ns = model._pad_audio(clips)
    enc_fn = lambda: model.encode_frames(*model.stem(buf, ns))
    ws = alternating_us({"encoder": enc_fn}, inner=2, repeats=7, warmup=2)["encoder"]
    x, frames = model.stem(buf, ns)
    enc = model.encode_frames(x, frames)
    out.append({"what": "moonshine_encoder", "model": name, "B": 8, "seconds": 30, "frames": frames[0], "layers": c.encoder_num_hidden_layers,
                **{k.replace("_us", "_ms"): v / 1e3 for k, v in stat(ws).items()}})
    for B in (1, 8):
        e = enc[:B].contiguous()
        cache = model.new_cache(e, frames[:B], capacity=64)
        tok = torch.ones((B, 1), dtype=torch.int32, device=dev)
        model(torch.ones((B, 32), dtype=torch.int32), e, cache)   # 32 positions in the cache
        ids, gap = torch.empty((B,), dtype=torch.int32, device=dev), torch.empty((B,), device=dev)

        def step():
            cache["pos"] = 32
            hidden, _ = model(tok, e, cache)
            ops.ctc_rows(model._get_logits(hidden[:, -1, :]), ids=ids, gap=gap)

        calls = [0]
        real_cs, real_sw = _lib.call_struct, ops.swiglu
        _lib.call_struct = lambda *a, **k: (calls.__setitem__(0, calls[0] + 1), real_cs(*a, **k))[1]
        ops.swiglu = lambda *a, **k: (calls.__setitem__(0, calls[0] + 1), real_sw(*a, **k))[1]
        try:
            step()
        finally:
            _lib.call_struct, ops.swiglu = real_cs, real_sw
        ws = alternating_us({"step": step}, inner=5, repeats=7, warmup=2)["step"]
        out.append({"what": "moonshine_decode_step", "model": name, "B": B, "encoder_frames": frames[0], "cache_positions": 32,
                    "layers": c.decoder_num_hidden_layers, "entry_point_calls_per_token": calls[0],
                    **{k.replace("_us", "_ms"): v / 1e3 for k, v in stat(ws).items()}})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(U.ROOT, "profiles", "bench_moonshine.jsonl"))
    a = ap.parse_args()
    ops.require_gpu()
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(1)
    lines = []

    def emit(r):
        lines.append(r)
        print(json.dumps(r))
        sys.stdout.flush()

    for name, kw in (("tiny", dict()), ("base", dict(hidden_size=416, intermediate_size=1664, encoder_num_hidden_layers=8, decoder_num_hidden_layers=8))):
        for r in bench_model(dev, g, name, kw):
            emit(r)
    ragged = [1250, 1100, 950, 800, 650, 500, 350, 200]
    for dh in (36, 52):
        emit(bench_attention(dev, g, "encoder_self_attention", 8, 1250, 1250, 8, dh))
        emit(bench_attention(dev, g, "encoder_self_attention", 8, 1250, 1250, 8, dh, lens_k=ragged))
    for dh in (36, 52):
        for B in (1, 8):
            emit(bench_attention(dev, g, "decode_step_self_attention", B, 1, 200, 8, dh))
            emit(bench_attention(dev, g, "decode_step_cross_attention", B, 1, 1250, 8, dh))
    for dh, rot in ((36, 32), (52, 46)):
        emit(bench_rope(dev, g, 8, 1250, 8, dh, rot))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for r in lines:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
