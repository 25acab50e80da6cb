#!/usr/bin/env python
"""Headline benchmark: audio samples/sec + real-time factor, Kokoro-82M TTS on MI355X.

Contract (driver): ``python bench.py --gpus N --steps K --warmup W`` (N>1 under
``python -m torch.distributed.run``, one rank per GPU, RCCL).  One "step" = one pass of the hot path
(tokens -> waveform, ``Model.__call__`` of the reference, kokoro.py:111-177) over one batch of
synthetic utterances per GPU: BASELINE.json config[1], "Kokoro-82M bf16 TTS on 1 MI355X".  Each
utterance is the canonical short sentence of BASELINE.md: 78 phonemes (T = 80 tokens), durations
forced to 264 frames -> 158 400 samples = 6.6 s at 24 kHz.  Weights: seeded random, bf16-valued, in
the exact Kokoro-82M shapes (no network => no checkpoint).  Per-utterance inputs (voice rows, forced durations,
SineGen noise) are resident in HBM before the timed region; the request block itself (int32 token ids, 131 KB for 64
utterances) travels inside the step because that IS the first message of the sharded step (mlx_audio_amd/shard.py: rank 0
owns the request queue; one broadcast).  ``--config whisper | qwen3 | csm`` run the secondary lines with the same schema.

A plain run sets up, warms up, times ``--steps`` steps and prints the line.  ``--full`` adds the legs that are not the headline figure: the
batch-vs-single check, the precision-2 leg, the roofline (instrumented step + in-run PMC passes), the one-utterance latency and the CPU baseline.
``--dump-outputs DIR`` writes the waveforms of the last timed step as .npy files (see ``dump_outputs``).

Rank 0 prints ONE JSON line; see DESIGN.md section "Measurement" for every field.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

SAMPLES_PER_UTT = 158400
T_TOKENS, F_FRAMES = 80, 264
MFMA_BF16_PEAK_TFLOPS = 2500.0   # /opt/skills/guides/MI355X_MICROARCH.md: dense bf16 MFMA
HBM_PEAK_GBS = 8000.0            # same guide: HBM3E spec peak


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64,
                    help="utterances per GPU per step (SURVEY 8d batch list: 1 / 8 / 64 / 512; 64 per GPU = 512 over the 8-GPU node; measured on one\n"
                         "MI355X: 122 M samples/s at 32, 140 M at 64, 146 M at 128, 150 M at 256 -- the front end's latency-bound LSTMs amortise)")
    ap.add_argument("--precision", type=int, default=None,
                    help="default: the mode load_model() / KokoroEngine pick for a bf16 checkpoint (KokoroEngine.default_precision = 6: vocoder convs of >= 7 taps\n"
                         "as fp16 hi pass + block-scaled FP4 lo pass; parity at the benchmarked batch: tests/test_kokoro_gpu.py::\n"
                         "test_kokoro_default_mode_batch64_canonical).  5 = the e4m3 lo pass of rounds 4 - 5 (7.9e-5 of the peak), 2 = bf16 hi+lo split MFMA\n"
                         "everywhere (3e-5), 3 = single fp16 pass in the vocoder (misses the 2e-3 bar), 1 = single bf16 pass.  A --full run also reports\n"
                         "mode 2 as value_precision2")
    ap.add_argument("--full", action="store_true",
                    help="also run the legs beyond the headline figure: batch_vs_single, value_precision2, roofline (with the in-run PMC passes), latency_b1,\n"
                         "cpu_baseline; the --no-* options drop single legs of a --full run")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="write the waveforms the last timed step returned to DIR/*.npy (float32, at most 64 MB: see dump_outputs)")
    ap.add_argument("--no-secondary-precision", action="store_true", help="skip the value_precision2 leg")
    ap.add_argument("--no-batch-check", action="store_true", help="skip the batch-vs-single leg (a kernel trace of the run then holds the step's launches only)")
    ap.add_argument("--config", choices=["kokoro", "whisper", "qwen3", "csm", "kitten", "dsp"], default="kokoro",
                    help="kokoro = the headline line (BASELINE config[1]); whisper / qwen3 / csm = the secondary lines of SURVEY 8d (BASELINE configs\n"
                         "[2] / [3] / [4]) with the same JSON schema (tools/bench_{whisper,qwen3,csm}.py run in-process); dsp = the STFT -> mel -> log front end\n"
                         "against the HBM roofline (tools/bench_dsp.py)")
    ap.add_argument("--dry-run-gloo", action="store_true",
                    help="CPU rehearsal of the multi-GPU launch: the self-launcher spawns --gpus N ranks over gloo, every rank runs the REAL sharded step\n"
                         "(mlx_audio_amd/shard.py: broadcast, all_reduce, all_to_all) around a stand-in engine, rank 0 prints the JSON line (value is not a measurement)")
    ap.add_argument("--ragged", action="store_true",
                    help="utterance lengths drawn from 20..510 tokens with +-35 %% frames-per-token spread instead of the uniform canonical sentence:\n"
                         "shows the load imbalance the frame-count re-balance (mlx_audio_amd/shard.py) is there for; not the headline configuration")
    ap.add_argument("--wire", choices=["fp32", "fp16"], default="fp32", help="waveform dtype on the wire of the multi-GPU gather")
    ap.add_argument("--gather", choices=["rank0", "none"], default="rank0",
                    help="--config whisper | qwen3 | csm on several GPUs: results (token / code sequences) back to rank 0, or kept on the rank that made them")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--no-latency", action="store_true", help="skip the one-utterance-per-call leg (latency_b1): a kernel trace of the run then holds the batch's launches only")
    ap.add_argument("--no-pmc", action="store_true", help="skip the two in-run rocprofv3 PMC passes (roofline.traffic is then null)")
    ap.add_argument("--pmc-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--cpu-baseline-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--shape-table", default="", help="write the per-shape conv_gemm timing table (roofline leg, needs --full) to this file")
    args = ap.parse_known_args()[0]
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.shape_table and not args.full:
        ap.error("--shape-table needs --full (it is written by the roofline leg)")
    if args.dump_outputs and args.config != "kokoro":
        ap.error("--dump-outputs is implemented for the Kokoro line only")
    if not args.full:   # a plain run: set-up, warm-up, the timed steps, the line
        args.no_batch_check = args.no_secondary_precision = args.no_roofline = args.no_latency = args.no_cpu_baseline = True
    return args


DUMP_BUDGET_BYTES = 63_000_000   # 64 MB in all, less headroom for the .npy headers


def dump_outputs(path, outs):
    """``--dump-outputs DIR``: what a caller of the timed path receives from its last step, the waveforms of every utterance, in float32.
    ``waveforms.npy`` is [utterances, samples] when all have one length (the canonical batch: 64 x 158 400 = 40.6 MB), else their concatenation
    in item order; ``lengths.npy`` holds the samples per utterance.  Above DUMP_BUDGET_BYTES a fixed seeded sample of the concatenation is written
    instead, its positions in ``waveforms_index.npy``."""
    os.makedirs(path, exist_ok=True)
    w = [o.detach().to("cpu", torch.float32).reshape(-1).numpy() for o in outs]
    lengths = np.array([a.size for a in w], dtype=np.float64)
    flat = np.concatenate(w)
    if flat.nbytes + lengths.nbytes > DUMP_BUDGET_BYTES:
        n = (DUMP_BUDGET_BYTES - lengths.nbytes) // 12   # float32 value + float64 position per sample
        idx = np.unique(np.random.default_rng(0).integers(0, flat.size, size=n))
        np.save(os.path.join(path, "waveforms_index.npy"), idx.astype(np.float64))
        arr = flat[idx]
    else:
        arr = flat.reshape(len(w), -1) if len(set(lengths.tolist())) == 1 else flat
    np.save(os.path.join(path, "waveforms.npy"), arr)
    np.save(os.path.join(path, "lengths.npy"), lengths)


def cpu_baseline_child():
    """``--cpu-baseline-child``: the oracle (restated reference, PyTorch-CPU fp32) timed in its own process (the parent enforces a wall-clock limit).
    BASELINE.md section 3's protocol -- intra-op threads = the cores this process may run on, 2 warm-ups, median of 10 -- bounded to ~30 s of CPU work
    and to 32 threads: on the 256-core GPU box the 256-thread run did not finish a single pass within 15 minutes (round-5 call 7: the leg was killed
    by the call's timeout; these conv sizes spend their time in the thread pool's barriers), so ``capped_at`` states the cap instead."""
    from mlx_audio_amd.tts.models.kokoro import synthetic as S
    from oracle.kokoro_ref import KokoroRef

    try:
        avail = len(os.sched_getaffinity(0))
    except AttributeError:
        avail = os.cpu_count() or 1
    cores = max(1, min(avail, 32))
    torch.set_num_threads(cores)
    ref = KokoroRef(S.make_kokoro_weights(), S.KOKORO_CONFIG)
    ids = S.make_phoneme_ids(T_TOKENS - 2, seed=0)
    ref_s = S.make_voice_pack()[T_TOKENS - 3]

    def run(frames):
        fd = S.forced_durations(T_TOKENS, frames, seed=0)
        t0 = time.perf_counter()
        ref.forward(ids, ref_s, pred_dur=fd)
        return time.perf_counter() - t0

    budget = 30.0
    run(T_TOKENS)           # warm-up 1 (F = 80: allocator, thread pool)
    probe = run(T_TOKENS)   # warm-up 2, and the probe that sizes the sample
    est = probe * F_FRAMES / T_TOKENS
    frames = F_FRAMES if est * 3 <= budget else 66
    est = probe * frames / T_TOKENS
    reps = int(max(1, min(10, budget // max(est, 1e-3))))
    times = sorted(run(frames) for _ in range(reps))
    med = times[len(times) // 2]
    samples = frames * 600
    out = {"value": samples / med, "unit": "samples/s", "cores": cores, "kind": "port",
           "sample": f"1 utterance (T=80, F={frames}, {samples} samples), 2 warm-ups (F=80) + median of {reps}; torch.set_num_threads({cores}); restated "
                     "reference (oracle/kokoro_ref.py, PyTorch-CPU fp32), not MLX",
           "x_realtime": samples / 24000.0 / med, "host_cores_available": avail, "reps": reps}
    caps = []
    if cores < avail:
        caps.append(f"{cores} of {avail} cores (more intra-op threads only add barrier time for these conv sizes; the 256-thread run never finished: see the docstring)")
    if reps < 10 or frames != F_FRAMES:
        caps.append(f"{budget:.0f} s of CPU work: {reps} repetition(s) of F={frames} instead of 10 of F={F_FRAMES}")
    if caps:
        out["capped_at"] = "; ".join(caps)
    print("CPU_BASELINE_JSON " + json.dumps(out))


def cpu_baseline(limit_s: float = 150.0):
    """Runs ``cpu_baseline_child`` in a subprocess under a wall-clock limit: the bench line must come out whatever the host's thread pool does."""
    import subprocess

    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--cpu-baseline-child"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True,
                           timeout=limit_s, env=dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES=""))
        for ln in r.stdout.splitlines():
            if ln.startswith("CPU_BASELINE_JSON "):
                return json.loads(ln[len("CPU_BASELINE_JSON "):])
        return {"value": None, "unit": "samples/s", "kind": "port", "error": f"child exited with {r.returncode}"}
    except subprocess.TimeoutExpired:
        return {"value": None, "unit": "samples/s", "kind": "port", "error": f"not finished within {limit_s:.0f} s (killed)"}


def _free_port():
    import socket

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def self_launch(args):
    """``python bench.py --gpus N`` with N > 1 and no launcher around it: re-exec this command line under ``torch.distributed.run`` (one rank per
    GPU, rendezvous on 127.0.0.1), exactly the command the driver would have typed; the ranks' rank 0 prints the JSON line on our stdout."""
    import subprocess

    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC: RCCL across processes needs it on this driver
    env.setdefault("OMP_NUM_THREADS", "8")
    sys.exit(subprocess.call(cmd, env=env))


def run_secondary(args):
    """``--config whisper | qwen3 | csm``: the secondary lines (tools/bench_*.py) behind the driver's flags, same JSON schema, one GPU."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import importlib

    mod = importlib.import_module(f"bench_{args.config}")
    # --gpus N: launched like the headline line (torch.distributed.run, one rank per GPU); the tools read RANK / WORLD_SIZE themselves and shard
    # their batch over the ranks through mlx_audio_amd.shard.ShardChannel (requests out in one broadcast, ragged integer results back)
    argv = ["--steps", str(args.steps), "--warmup", str(args.warmup)] + (["--no-cpu-baseline"] if args.no_cpu_baseline else [])
    if args.config not in ("kitten", "dsp"):
        argv += ["--gather", args.gather]
    mod.main(argv)


# sustained rates of the matrix pipe ALONE at this part's 1400 W cap (tools/src/mfma_peak.hip, 50 ms loops, random operands, two waves per SIMD:
# profiles/r6_mfma_peak_fp4_call2.jsonl): what "100 % MFMA" buys on this box -- the 2.5 PFLOP/s dense figure needs 2.4 GHz, the cap allows ~1.7
MFMA_SUSTAINED_TFLOPS = {"f16": 1777.0, "e4m3": 3886.0, "fp4": 6738.0}


def power_cap_view(prof, conv_ms):
    """The conv set against the matrix pipe's own sustained rates under the power cap: time the step's MFMA work would take with NOTHING else on the
    chip (per conv: one 16-bit pass, + the lo pass of its mode: a second 16-bit pass for the bf16 / fp16 splits, the padded tap pairs at the e4m3 / FP4
    rate for the MX convs = the >= 7-tap convs of >= 64 channels), and the share of the measured conv time that floor is."""
    from mlx_audio_amd import ops

    floor_ms, mode = 0.0, None
    for fl, by, a0, a1, shp in prof:
        cin, cout, k = shp[0], shp[1], shp[2]
        hi = fl / (MFMA_SUSTAINED_TFLOPS["f16"] * 1e12)
        if PRECISION_FOR_VIEW in (5, 6) and ops.mx_pays(cout, k, cin):
            lo = fl * (2.0 * ((k + 1) // 2) / k) / (MFMA_SUSTAINED_TFLOPS["fp4" if PRECISION_FOR_VIEW == 6 else "e4m3"] * 1e12)
        else:
            lo = hi
        floor_ms += (hi + lo) * 1e3
    return {"mfma_only_floor_ms": floor_ms, "share_of_conv_time": floor_ms / max(conv_ms, 1e-9),
            "sustained_tflops": MFMA_SUSTAINED_TFLOPS,
            "what": "the conv set's matrix work at the pipe's measured sustained rates under the 1400 W cap (profiles/r6_mfma_peak_fp4_call2.jsonl) / measured conv time; "
                    "the remainder is the energy of everything else -- weight fragments L2 -> registers, the producers' VALU work, HBM traffic, data toggling "
                    "(profiles/r6_conv_ws4_p5_ablation_b64_call1.txt, r6_conv_energy_probe_call3.txt: each removal buys its share, the chip stays at 1390 W)"}


PRECISION_FOR_VIEW = 2


def pmc_traffic(args):
    """HBM bytes per conv launch from the PMC counters, measured in THIS run: two child passes of this same command (one step each) under
    ``rocprofv3 --kernel-trace --pmc FETCH_SIZE`` and ``... --pmc WRITE_SIZE`` (separate passes: the TCC block has 4 slots, the two counters
    need 3 + 2), summed per dispatch over the counter instances, corrected as MI355X_MICROARCH.md prescribes for gfx950 (FETCH_SIZE counts
    half of a coalesced streaming read; both are in KB): bytes = (2 * FETCH_SIZE + WRITE_SIZE) * 1024.  Returns None when rocprofv3 is not
    usable here (then ``roofline.traffic`` is null rather than a number from another run)."""
    import glob
    import shutil
    import subprocess
    import tempfile

    if shutil.which("rocprofv3") is None or os.environ.get("ROCPROFILER_REGISTER_FORCE_LOAD") or os.environ.get("ROCP_TOOL_LIBRARIES"):
        return None
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from pmc_traffic import per_kernel

    tmp = tempfile.mkdtemp(prefix="mi355_pmc_")
    env = dict(os.environ, TMPDIR="/tmp")
    tot = {}
    try:
        # third pass: MFMA pipe occupancy of the same launches (SQ_VALU_MFMA_BUSY_CYCLES: cycles summed over the 1024 SIMDs; GRBM_GUI_ACTIVE: cycles
        # summed over the 8 XCDs, so GUI_ACTIVE / 8 is the launch's duration in shader clocks and also gives the clock the chip actually ran at)
        for ctrs in (("FETCH_SIZE",), ("WRITE_SIZE",), ("SQ_VALU_MFMA_BUSY_CYCLES", "GRBM_GUI_ACTIVE")):
            out = os.path.join(tmp, ctrs[0])
            cmd = ["rocprofv3", "--kernel-trace", "--pmc", *ctrs, "-d", out, "-o", "p", "--", sys.executable, os.path.abspath(__file__), "--pmc-child",
                   "--steps", "1", "--warmup", "1", "--batch", str(args.batch), "--precision", str(args.precision), "--no-roofline",
                   "--no-cpu-baseline"]
            r = subprocess.run(cmd, cwd="/tmp", env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240)
            dbs = glob.glob(os.path.join(out, "**", "*results.db"), recursive=True)
            if r.returncode != 0 or not dbs:
                return None
            for ctr in ctrs:
                per = per_kernel(dbs[0], ctr)
                vals = [v for k, vs in per.items() if "conv_ws4_kernel" in k or "conv_gemm_kernel" in k for v in vs]
                tot[ctr] = (sum(vals), len(vals))
                if ctr in ("SQ_VALU_MFMA_BUSY_CYCLES", "GRBM_GUI_ACTIVE"):   # ... and of the dominant instantiation alone
                    domk = "conv_ws4_kernel<%d, 2" % (args.precision if args.precision in (5, 6) else 2)   # the Snake resblock convs of the mode
                    dom = [v for k, vs in per.items() if domk in k for v in vs]
                    tot[ctr + "_dom"] = (sum(dom), len(dom))
                    if ctr == "GRBM_GUI_ACTIVE":   # wall time of the same dispatches: GUI_ACTIVE / 8 XCDs / duration = the clock the chip ran them at
                        import sqlite3

                        cur = sqlite3.connect(dbs[0]).cursor()
                        cols = [r[1] for r in cur.execute("pragma table_info(kernels)")]
                        ncol = "name" if "name" in cols else [c for c in cols if "name" in c][0]
                        tot["dom_ns"] = sum(r[1] - r[0] for r in cur.execute(f"select start, end, {ncol} from kernels") if domk in r[2])
        n = max(tot["FETCH_SIZE"][1], 1)
        res = {"bytes_per_launch": (2.0 * tot["FETCH_SIZE"][0] + tot["WRITE_SIZE"][0]) * 1024.0 / n, "launches_counted": n,
               "fetch_kb_total": tot["FETCH_SIZE"][0], "write_kb_total": tot["WRITE_SIZE"][0]}
        gui, busy = tot["GRBM_GUI_ACTIVE"][0], tot["SQ_VALU_MFMA_BUSY_CYCLES"][0]
        if gui > 0:
            res["mfma_busy_frac"] = busy / (gui / 8.0 * 1024.0)
        gd, bd = tot["GRBM_GUI_ACTIVE_dom"][0], tot["SQ_VALU_MFMA_BUSY_CYCLES_dom"][0]
        if gd > 0:
            res["mfma_busy_frac_dominant"] = bd / (gd / 8.0 * 1024.0)
            if tot.get("dom_ns", 0) > 0:
                res["clock_ghz_dominant"] = gd / 8.0 / tot["dom_ns"]
        # the child ran warm-up + timed step = 2 steps; every counter saw the same launches
        return res
    except Exception:
        return None
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


_T0 = time.perf_counter()


def _log(msg):
    """Phase marks on stderr (elapsed wall seconds): which leg a slow run is in."""
    print(f"[bench +{time.perf_counter() - _T0:6.1f}s] {msg}", file=sys.stderr, flush=True)


def main():
    args = parse()
    if args.cpu_baseline_child:
        return cpu_baseline_child()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.gpus > 1 and world == 1:
        return self_launch(args)   # never returns
    if args.config != "kokoro":
        return run_secondary(args)
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    dry = args.dry_run_gloo
    dist = None
    if world > 1:
        import torch.distributed as dist

        if dry:
            dist.init_process_group("gloo")
        else:
            torch.cuda.set_device(local)
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    dev = torch.device("cpu") if dry else torch.device("cuda", local)
    if not dry:
        torch.cuda.set_device(dev)

    def sync():
        if not dry:
            torch.cuda.synchronize()

    from mlx_audio_amd.tts.models.kokoro import synthetic as S

    from mlx_audio_amd import shard

    if dry:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        from _bench_util import RehearsalEngine

        ops = None
        eng = RehearsalEngine()
        args.no_roofline = args.no_latency = args.no_cpu_baseline = args.no_secondary_precision = True
    else:
        from mlx_audio_amd import ops
        from mlx_audio_amd.tts.models.kokoro.engine import KokoroEngine

        eng = KokoroEngine(S.make_kokoro_weights(), S.KOKORO_CONFIG, device=dev, precision=args.precision)
    args.precision = eng.precision   # None -> the engine's own default (KokoroEngine.default_precision): what load_model() users get
    global PRECISION_FOR_VIEW
    PRECISION_FOR_VIEW = args.precision
    B = args.batch
    n_total = B * world
    # requests (token ids) are owned by rank 0 and cross ranks inside the step (one broadcast); voice rows, forced durations and SineGen noise
    # are per-utterance inputs every rank derives locally from the seed, resident in HBM before the timed region
    if args.ragged:
        rng = np.random.default_rng(7)
        t_of = [int(v) for v in rng.integers(20, 511, size=n_total)]
        f_of = [max(t, int(round(t * 3.3 * (1.0 + 0.35 * (2.0 * rng.random() - 1.0))))) for t in t_of]
    else:
        t_of, f_of = [T_TOKENS] * n_total, [F_FRAMES] * n_total
    requests = [S.make_phoneme_ids(t_of[i] - 2, seed=i) for i in range(n_total)] if rank == 0 else None
    voice = S.make_voice_pack().to(dev)
    fds = [S.forced_durations(t_of[i], f_of[i], seed=i).to(dev) for i in range(n_total)]
    ch = shard.ShardChannel(dev, dist, max_items=max(n_total, 8), max_tokens=512)
    # SineGen's uniform initial phases and gaussian noise are drawn on the device INSIDE every step (engine default, like the reference's
    # mx.random calls inside its forward pass, istftnet.py:581,649): nothing of a step is precomputed except the inputs
    noise_kw = None
    wire = torch.float16 if args.wire == "fp16" else None

    class VoiceRows:  # style row of an utterance = voice pack row (n_phonemes - 1), kokoro.py:223-226; one device gather per step
        def __init__(self):
            self.cache = {}

        def __call__(self, i, t):
            return voice[t - 3]

        def rows(self, items, lens):
            key = tuple(items)
            if key not in self.cache:
                self.cache[key] = torch.tensor([lens[i] - 3 for i in items], dtype=torch.long, device=dev)
            return voice[self.cache[key], 0]

    voice_rows = VoiceRows()

    class ForcedRows:  # forced durations of a shard as one padded int32 block (resident; built once per plan)
        def __init__(self):
            self.cache = {}

        def __call__(self, i):
            return fds[i]

        def rows(self, items, lens):
            key = tuple(items)
            if key not in self.cache:
                self.cache[key] = torch.nn.utils.rnn.pad_sequence([fds[i].to(torch.int32) for i in items], batch_first=True).contiguous()
            return self.cache[key]

    forced_rows = ForcedRows()

    def step():
        # mlx_audio_amd/shard.py: broadcast of the request block, token-rate half on this rank's shard, all_reduce of the frame counts,
        # re-balance on the real frame counts (all_to_all, only when it pays), frame-rate half, exact-size all_to_all of the waveforms to
        # rank 0 -- over RCCL / xGMI when world > 1
        return shard.kokoro_step(ch, eng, requests, voice_rows, 600, forced_durations_of=forced_rows,
                                 wire_dtype=wire, back_kwargs=noise_kw)

    def timed(fn, warmup, steps):
        for _ in range(warmup):
            fn()
        sync()
        if world > 1:
            dist.barrier()
        sync()
        t0 = time.perf_counter()
        for _ in range(steps):
            outs = fn()
        sync()
        if world > 1:
            dist.barrier()
        sync()
        dt = time.perf_counter() - t0
        if world > 1:
            t = torch.tensor([dt], device=dev, dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dt = float(t.item())
        return outs, dt

    _log("engine ready; timed region")
    outs, dt = timed(step, args.warmup, args.steps)
    _log(f"timed region done: {1000.0 * dt / args.steps:.2f} ms per step")
    if rank == 0:
        assert len(outs) == n_total and all(o.numel() == f_of[i] * 600 for i, o in enumerate(outs))
        assert bool(torch.isfinite(torch.cat([o.reshape(-1) for o in outs])).all())   # one fused check, after the timed region
        if args.dump_outputs:   # before any other leg runs the engine again
            dump_outputs(args.dump_outputs, outs)

    # ---- after the timed region (N = 1): the benchmarked step against the SAME utterance run alone, SineGen inputs fixed on both sides
    batch_check = None
    if rank == 0 and world == 1 and not dry and not args.ragged and not args.pmc_child and not args.no_batch_check:   # (the PMC child passes count the step's own launches only)
        g = torch.Generator(device="cpu").manual_seed(4321)
        ri1 = torch.rand((1, 9), generator=g).to(dev)
        nz1 = torch.randn((1, 2 * F_FRAMES * 300, 9), generator=g).to(dev)
        # F0 / N of the lone run are injected into the batch step: the harmonic source INTEGRATES F0 into a phase, so the ~1e-6 relative
        # summation-order difference between the B = 64 and B = 1 kernel selections of the predictor would otherwise decorrelate the two waveforms
        # within a second (tests/test_kokoro_gpu.py module docstring); everything downstream of the curves is compared free-running
        o1, _, t1 = eng.forward([requests[0]], voice[T_TOKENS - 3], forced_durations=[fds[0]], rand_ini=ri1, noise=nz1, return_intermediates=True)
        f0_1, n_1 = t1["f0"][:1].clone(), t1["n"][:1].clone()
        del t1
        fixed = lambda items: dict(rand_ini=ri1.expand(len(items), -1).contiguous(), noise=nz1.expand(len(items), -1, -1).contiguous(),  # noqa: E731
                                   overrides=dict(f0=f0_1.expand(len(items), -1).contiguous(), n=n_1.expand(len(items), -1).contiguous()))
        ob = shard.kokoro_step(ch, eng, requests, voice_rows, 600, forced_durations_of=forced_rows, wire_dtype=wire, back_kwargs=fixed)
        sync()
        peak = float(o1[0].abs().max())
        diff = float((ob[0].to(torch.float32) - o1[0]).abs().max())
        # mode 5: the lone utterance leaves generator stage 0 on the 4-wave kernels (fp16 hi + fp16 lo on the same images) while the batch runs the
        # MX lo pass there, so the two differ by the lo pass's own error (~1e-4 of the peak); the other modes differ by summation order only
        bar = {5: 4e-4, 6: 5e-4}.get(args.precision, 5e-5)   # (mode 6: measured 1.7e-4 -- the FP4 lo pass's own error is ~3x the e4m3 one's; B = 1 and B = 64 take different kernels for generator stage 0)
        batch_check = {"max_abs_diff_over_peak": diff / peak, "bar": bar, "what": "utterance 0 of the benchmarked batch step vs the same utterance run alone (same SineGen inputs, the lone "
                       "run's F0 / N curves injected into the batch), max |diff| / peak"}
        batch_check["ok"] = bool(diff <= bar * peak)   # reported, not fatal: the line's own parity gate is tests/test_kokoro_gpu.py (B = 64, against the oracle)
        if not batch_check["ok"]:
            print("bench.py: WARNING batch_vs_single above its bar: %r" % (batch_check,), file=sys.stderr)
        del ob, o1, nz1

    _log("batch-vs-single check done")
    # ---- the other precision mode on the same workload (N = 1): bf16 hi + lo split everywhere (mode 2), reported as value_precision2
    p2 = None
    if rank == 0 and world == 1 and not args.no_secondary_precision and not args.pmc_child and not args.ragged and args.precision != 2:
        eng_main = eng
        eng = KokoroEngine(S.make_kokoro_weights(), S.KOKORO_CONFIG, device=dev, precision=2)   # `step` reads the name `eng`
        _, dt2 = timed(step, min(args.warmup, 2), args.steps)
        p2 = {"value": sum(f_of) * 600 * args.steps / dt2, "ms_per_step": 1000.0 * dt2 / args.steps}
        eng = eng_main
        torch.cuda.empty_cache()

    res = None
    if rank == 0:
        total_samples = sum(f_of) * 600 * args.steps
        value = total_samples / dt
        res = {
            "metric": "audio samples/sec + real-time factor, Kokoro-82M TTS", "value": value, "unit": "samples/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": 1000.0 * dt / args.steps,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": {0: "none (dry run: stand-in engine)", 2: "bf16 weights x fp32 activations (bf16 hi+lo split MFMA, fp32 accumulate)",
                      3: "fp16 activations x bf16-valued weights in fp16 (single MFMA pass, fp32 accumulate) in the vocoder; hi+lo front end",
                      1: "bf16", 4: "fp16-valued weights x fp32 activations (fp16 hi+lo split MFMA)",
                      5: "bf16 weights x fp32 activations: vocoder convs = fp16 hi pass (v_mfma_f32_32x32x16_f16) + block-scaled e4m3 lo pass "
                         "(v_mfma_scale_f32_32x32x64_f8f6f4, OCP MX: E8M0 scale per row x 32 channels / per output column), fp32 accumulate; "
                         "front end bf16 hi+lo split",
                      6: "bf16 weights x fp32 activations: vocoder convs = fp16 hi pass (v_mfma_f32_32x32x16_f16) + block-scaled FP4 (e2m1) lo pass "
                         "(v_mfma_scale_f32_32x32x64_f8f6f4 cbsz / blgp 4, OCP MX: E8M0 scale per row x 32 channels / per output column), fp32 accumulate; "
                         "front end bf16 hi+lo split"}[args.precision],
            "data": "synthetic",
            "config": {"workload": ("Kokoro-82M bf16 TTS, tokens->waveform, RAGGED utterances T in 20..510 tokens, frames/token 3.3 +-35 %"
                                     if args.ragged else
                                     "Kokoro-82M bf16 TTS, tokens->waveform, canonical short sentence T=80 F=264 (6.6 s @ 24 kHz)"),
                       "utterances_per_gpu": B, "global_batch": B * world,
                       "samples_per_utterance": (sum(f_of) * 600 / n_total) if args.ragged else SAMPLES_PER_UTT,
                       "parallelism": f"utterance-dp{world}", "precision_mode": args.precision, "wire": args.wire,
                       "shard_plan_makespan_frames": shard.makespan(f_of, ch.owned), "collectives_per_step": ch.collectives // max(1, args.steps + args.warmup)},
            "x_realtime": value / 24000.0, "rtf_reference_style": 24000.0 / value,
        }
        if batch_check:
            res["batch_vs_single"] = batch_check
        if p2:
            res["value_precision2"] = p2["value"]
            res["ms_per_step_precision2"] = p2["ms_per_step"]
        if dry:
            res["dry_run"] = "gloo rehearsal on CPU with a stand-in engine: the collectives are the real ones, the value is NOT a measurement"
    _log("secondary precision leg done")
    # ---- roofline leg (rank 0, N=1 only): one extra instrumented step, events around every conv_gemm launch
    if rank == 0 and world == 1 and not args.no_roofline:
        ops.PROFILE = []
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        step()
        e1.record()
        torch.cuda.synchronize()
        prof, ops.PROFILE = ops.profile_finalize(ops.PROFILE), None
        if args.shape_table:
            agg = {}
            for fl, by, a0, a1, shp in prof:
                e = agg.setdefault(shp[:4], [0, 0.0, 0.0, 0])
                e[0] += 1; e[1] += a0.elapsed_time(a1); e[2] += fl; e[3] = shp[4]
            with open(args.shape_table, "w") as f:
                f.write("cin cout k dil rows launches ms gflop tflops\n")
                for shp, e in sorted(agg.items(), key=lambda kv: -kv[1][1]):
                    f.write(f"{shp[0]} {shp[1]} {shp[2]} {shp[3]} {e[3]} {e[0]} {e[1]:.3f} {e[2] / 1e9:.2f} {e[2] / (e[1] * 1e-3) / 1e12:.1f}\n")
        flops = sum(p[0] for p in prof)
        byts = sum(p[1] for p in prof)
        # HBM bytes per conv launch from the PMC counters, measured by two child passes of this same command (pmc_traffic above)
        pmc = None if (args.no_pmc or args.ragged) else pmc_traffic(args)
        traffic = pmc["bytes_per_launch"] if pmc else None
        ms = sum(p[2].elapsed_time(p[3]) for p in prof)
        res["roofline"] = {
            "bound": "mfma", "kernel": ("conv_ws4_kernel<5, ...> (fp16 hi taps on v_mfma_f32_32x32x16_f16 + e4m3 lo tap pairs on v_mfma_scale_f32_32x32x64_f8f6f4) + "
                                        "conv_ws4_kernel<2 / 4, ...> + conv_gemm_kernel (implicit-GEMM conv1d/convT/linear)" if args.precision == 5 else
                                        "conv_ws4_kernel<6, ...> (fp16 hi taps on v_mfma_f32_32x32x16_f16 + FP4 lo tap pairs on v_mfma_scale_f32_32x32x64_f8f6f4) + "
                                        "conv_ws4_kernel<2 / 4, ...> + conv_gemm_kernel (implicit-GEMM conv1d/convT/linear)" if args.precision == 6 else
                                        "conv_ws4_kernel + conv_gemm_kernel (implicit-GEMM conv1d/convT/linear, v_mfma_f32_32x32x16_bf16)"),
            "achieved": flops / (ms * 1e-3) / 1e12, "peak": MFMA_BF16_PEAK_TFLOPS, "unit": "TFLOP/s",
            "frac": flops / (ms * 1e-3) / 1e12 / MFMA_BF16_PEAK_TFLOPS, "traffic": traffic,
            "mfma_busy_frac": pmc.get("mfma_busy_frac") if pmc else None,
            "mfma_busy_frac_dominant_kernel": pmc.get("mfma_busy_frac_dominant") if pmc else None,
            "clock_ghz_dominant_kernel": pmc.get("clock_ghz_dominant") if pmc else None,
            "mfma_busy_note": "SQ_VALU_MFMA_BUSY_CYCLES / (GRBM_GUI_ACTIVE / 8 XCDs x 1024 SIMDs) over the conv launches of a third in-run rocprofv3 pass: the share of "
                              "SIMD-cycles with the matrix pipe busy, at the clock the chip actually ran (DVFS: clock_ghz_dominant_kernel = GRBM_GUI_ACTIVE / 8 / "
                              "duration; the part sits at its 1400 W cap under these kernels, profiles/r6_smi_power_clock_during_conv_call1.txt); dominant = "
                              "conv_ws4_kernel<mode, 2, ...> (the Snake resblock convs).  An FP4 lo MFMA occupies the pipe half as long as the e4m3 one it replaced: "
                              "mode 6 LOWERS this fraction while it raises the rate",
            "power_cap_view": power_cap_view(prof, ms),
            "traffic_note": "avg HBM bytes per conv launch measured in this run: (2*FETCH_SIZE + WRITE_SIZE)*1024 over %s launches of two rocprofv3 PMC "
                            "child passes; algorithmic avg = %.3e B per launch (inputs + outputs + residual / accumulate reads + weights, each once)" % (
                                pmc["launches_counted"] if pmc else "no", byts / max(1, len(prof))),
            "algorithmic_bytes_per_launch": byts / max(1, len(prof)),
            "traffic_over_algorithmic": (traffic / (byts / max(1, len(prof)))) if traffic else None,
            "launches_per_step": len(prof), "algorithmic_gflop_per_step": flops / 1e9,
            "conv_gemm_ms_per_step": ms, "instrumented_step_ms": e0.elapsed_time(e1),
            "hbm_view": {"algorithmic_GB_per_step": byts / 1e9, "achieved_GBps": byts / (ms * 1e-3) / 1e9,
                         "peak_GBps": HBM_PEAK_GBS, "frac": byts / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                         # SURVEY section 8(d)'s own count beside it (bf16 activations, each conv's input + output once, 96.8 MB of weights once per step):
                         # 3 746 B per output sample and utterance -- the line's count above is 2.6x that: fp32 activations + the residual / running-sum reads
                         "survey_8d_GB_per_step": (3746.0 * sum(f_of) * 600 + 96.8e6) / 1e9,
                         "frac_on_survey_8d_bytes": (3746.0 * sum(f_of) * 600 + 96.8e6) / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                         "measured_GB_per_step": (traffic * len(prof) / 1e9) if traffic else None},
            "note": "intensity of the conv stack AS RUN (fp32 activations in HBM: flops / algorithmic bytes of this line = %.0f FLOP/B) is BELOW the bf16 ridge "
                    "(2500 TF/s / 8 TB/s = 312 FLOP/B): the k = 3 convs sit on the HBM side (2.8-4.0 TB/s of their bytes), the k >= 7 convs on the MFMA / issue "
                    "side; `frac` prices the whole set against MFMA, `hbm_view` against HBM (DESIGN.md section 6)" % (flops / max(byts, 1.0)),
        }
    _log("roofline leg done")
    # ---- latency leg (rank 0, N=1 only): ONE canonical utterance at a time, the reference's own configuration (config[0] / [1] synthesise a single
    # sentence); median wall time of the whole request: ids -> waveform on the device, SineGen noise drawn inside, synchronised
    if rank == 0 and world == 1 and not args.ragged and not args.no_latency and not args.pmc_child:
        ids1 = S.make_phoneme_ids(T_TOKENS - 2, seed=0)
        ref1 = voice[T_TOKENS - 3]
        fd1 = [fds[0]]
        for _ in range(3):
            eng.forward([ids1], ref1, forced_durations=fd1)
        torch.cuda.synchronize()
        lat = []
        for _ in range(15):
            t1 = time.perf_counter()
            o1, _ = eng.forward([ids1], ref1, forced_durations=fd1)
            torch.cuda.synchronize()
            lat.append(time.perf_counter() - t1)
        lat.sort()
        assert o1[0].numel() == SAMPLES_PER_UTT
        res["latency_b1"] = {"ms": 1000.0 * lat[len(lat) // 2], "ms_min": 1000.0 * lat[0], "x_realtime": SAMPLES_PER_UTT / 24000.0 / lat[len(lat) // 2],
                             "what": "one canonical utterance (T=80, F=264, 6.6 s of audio) per call, median of 15 synchronised calls after 3 warm-ups"}
    _log("latency leg done")
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        res["cpu_baseline"] = cpu_baseline()
        _log("cpu baseline leg done")
    if rank == 0:
        res["reference_note"] = ("parity oracle and cpu_baseline are the restated reference (oracle/kokoro_ref.py, PyTorch-CPU fp32) pinned to the reference's own "
                                 "Python run over an MLX stand-in (tests/golden/mlx_shim.py); MLX itself is not installable here and never executed")
    if rank == 0:
        print(json.dumps(res))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
