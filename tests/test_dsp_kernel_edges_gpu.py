"""Dispatch-branch parity of the transform kernels: csrc/fft.hip (the LDS Stockham STFT / iSTFT for any n_fft, mi355_logmel, mi355_kaldi_frames,
mi355_polar_spec), csrc/fft_fast.h (the register-resident kernels for n_fft 400 / 512 / 1024) and the two small-FFT heads of csrc/source.hip.

tests/test_kernels_gpu.py calls these at a handful of even sizes with contiguous, aligned operands; this file walks the branches of their launch
code those shapes do not reach: every radix of the Stockham plan, odd sizes, the LDS attribute branch, the scalar and the prefetching load paths
of the fast kernels, the mel slice and filterbank-capacity boundaries, the iSTFT's normalisation / clamp / trim / gap branches, the generic heads,
ragged lengths and strided views.  Statements, case tables and the restated launch arithmetic live in tests/_dsp_cases.py;
tests/test_dsp_refs_cpu.py holds them to known-good implementations.  Each statement is evaluated in float64 (the reference) and in float32 with
torch.fft on the CPU (its own rounding error, ``e32``).

Bars.  Exact (``torch.equal``) where only the loads or the wave schedule differ (load-path identity, prefetch against default), for sentinels
and for refusals.  Float outputs: ``4 * e32 + 1e-6 * peak`` of the float64 result ("float rule") -- except where tests/test_kernels_gpu.py already
sets a bar for the same kernel at the same input scale and a comparable size; that bar is kept there ("kept bar": spectrum 2e-6 x peak, iSTFT 5e-5,
phase 1e-3 modulo 2 pi at bins of magnitude >= 1e-4).  Each test says which rule it uses.
Every comparison prints ``EDGE <kernel> <case> err e32 peak bar`` before it asserts (``pytest -s`` shows the figures)."""
import math

import pytest
import torch

import _dsp_cases as S

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = S.SENTINEL
F64, F32 = torch.float64, torch.float32


@pytest.fixture(scope="module")
def ops():
    from mlx_audio_amd import ops as _ops

    _ops.require_gpu()
    return _ops


@pytest.fixture(scope="module")
def E():
    from mlx_audio_amd import _lib

    return _lib.Mi355Error


def check(name, case, got, ref64, ref32, existing=None):
    """``got`` (float32, cpu) against the float64 statement; bar = ``existing`` (an absolute figure) or 4 * e32 + 1e-6 * peak."""
    ref64 = ref64.double()
    err = float((got.double() - ref64).abs().max())
    e32 = float((ref32.double() - ref64).abs().max())
    peak = float(ref64.abs().max())
    bar = existing if existing is not None else 4.0 * e32 + 1e-6 * peak
    print(f"EDGE {name} {case} err={err:.3e} e32={e32:.3e} peak={peak:.3e} bar={bar:.3e}")
    assert math.isfinite(err) and err <= bar, (name, case, err, e32, bar)
    return err, e32


def ri(z):
    """complex [...] -> real [..., 2]."""
    return torch.view_as_real(z.contiguous())


def misaligned(t):
    """The values of ``t`` as a ``buf[1:1 + n]`` view of a fresh float32 device buffer: 4-byte but not 16-byte aligned."""
    buf = torch.empty(t.numel() + 1, dtype=torch.float32, device=DEV)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def widened(t, extra, fill=SENTINEL):
    """The values of a [B, L] (or [B, R, C]) tensor as the leading columns of a device buffer ``extra`` columns wider."""
    shape = list(t.shape)
    shape[-1] += extra
    buf = torch.full(shape, fill, dtype=torch.float32, device=DEV)
    buf[..., :t.shape[-1]] = t.to(DEV)
    return buf, buf[..., :t.shape[-1]]


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


# ================================================================================================================= A. generic Stockham forward
# measured on an MI355X: worst case by err / bar: n_fft 122 (radix 61): err 8.7e-6, e32 8.8e-6, peak 48, bar 8.3e-5 (0.10 of the bar); every case is below 0.11 of its bar
@pytest.mark.parametrize("c", S.STOCKHAM_CASES, ids=S.stockham_id)
def test_stockham_forward_edges(ops, monkeypatch, c):
    """mi355_stft on the LDS Stockham kernel (MI355_FFT_FAST=0) at every radix of make_plan (4, 2, 3, 5 and the generic branch at 7, 11, 13, 61), odd
    n_fft (no Nyquist bin), n_fft = 2 / 3, pairs = 1 (2048), dynamic LDS above 64 KB (4096), odd frame counts and n_frames = 1 (the partner frame
    of the last pair is absent), the shortest reflect-admissible signal, and x as a [:, :L] view of a wider buffer.  Float rule."""
    monkeypatch.setenv("MI355_FFT_FAST", "0")
    n, hop, L, pad, B = c["n_fft"], c["hop"], c["L"], c["pad"], c["B"]
    nfr = S.stockham_frames(c)
    x, w = S.ramp_noise(B, L, n), S.hamming(n)
    xd = widened(x, c["ld"] - L)[1] if "ld" in c else x.to(DEV)
    assert xd.stride(0) == c.get("ld", L)
    got = ops.stft_frames(xd, n, hop, w.to(DEV), pad, nfr)
    torch.cuda.synchronize()
    assert tuple(got.shape) == (B, nfr, n // 2 + 1)
    check("stft", S.stockham_id(c), ri(got.cpu()), ri(S.stft_stmt(x, w, n, hop, pad, nfr, F64)), ri(S.stft_stmt(x, w, n, hop, pad, nfr, F32)))


def raw_stft(ops, x, n_fft, hop, w, pad_mode, nfr, out):
    from mlx_audio_amd import _lib

    _lib.call_struct("mi355_stft", "mi355_stft_args", ops._stream(), x=x.data_ptr(), ldx=x.stride(0), L=x.shape[1], B=x.shape[0], n_fft=n_fft, hop=hop,
                     window=w.data_ptr(), pad_mode=pad_mode, n_frames=nfr, out=out.data_ptr())


def test_stockham_refusals(ops, monkeypatch, E):
    """Status and mi355_last_error text, nothing launched (the output keeps its sentinel): a prime factor above 61; LDS above 160 KB; reflect padding
    of a signal of n_fft / 2 samples; pad_mode 3.  Exact."""
    monkeypatch.setenv("MI355_FFT_FAST", "0")
    x = torch.zeros(1, 16384, device=DEV)
    w = torch.ones(16384, device=DEV)
    out = torch.full((1, 4, 8193, 2), SENTINEL, device=DEV)
    with pytest.raises(E, match="prime factor > 61"):
        raw_stft(ops, x, 134, 67, w, 0, 4, out)
    with pytest.raises(E, match="too large for LDS"):
        raw_stft(ops, x, 16384, 4096, w, 0, 1, out)
    with pytest.raises(E, match="too short for reflect"):
        raw_stft(ops, x[:, :48], 96, 24, w, 1, 1, out)
    with pytest.raises(E, match="pad_mode must be"):
        raw_stft(ops, x, 96, 24, w, 3, 4, out)
    monkeypatch.setenv("MI355_FFT_FAST", "1")
    with pytest.raises(E, match="too short for reflect"):   # the same check in front of the fast kernels
        raw_stft(ops, x[:, :200], 400, 160, w, 1, 1, out)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


# ================================================================================================================= B. mi355_logmel, generic path
def mel_refs(x, w, n, hop, pad, nfr, fb, mode, guard=0.0, fixed_max=None, finish=True):
    out = []
    for dt in (F64, F32):
        y = S.logmel_stmt(x, w, n, hop, pad, nfr, fb, mode, dt, log_guard=guard)
        out.append(S.whisper_finish_stmt(y, fixed_max) if (mode == 0 and finish) else y)
    return out


# measured on an MI355X: worst: (n_fft 96, 13 mels, mode 1) err 1.6e-6, e32 3.2e-7, peak 11.5, bar 1.3e-5 (0.12 of the bar)
@pytest.mark.parametrize("mode", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("c", S.LOGMEL_GENERIC, ids=lambda c: f"n{c['n_fft']}-m{c['n_mels']}")
def test_logmel_generic_modes(ops, monkeypatch, c, mode):
    """stft_kernel<1> (sizes without a fast kernel): the five modes at nb = 49 and nb = 126 (one and two trips of the 64-lane dot product, each with
    a tail), a bank with two all-zero rows (their value is the clamp floor's / the guard's logarithm), mode 4 with log_guard = 2^-24, mode 0 with
    its per-item maximum and the (y + 4) / 4 finish.  Every value is compared.  Float rule."""
    monkeypatch.setenv("MI355_FFT_FAST", "0")
    n, hop, L, n_mels = c["n_fft"], c["hop"], c["L"], c["n_mels"]
    nfr = S.n_frames_of(L, n, hop, 1)
    x, w = S.ramp_noise(2, L, n + mode), S.hamming(n)
    fb = S.random_sparse_bank(n_mels, n // 2 + 1, n, zero_rows=(2, n_mels - 1))
    guard = 2.0 ** -24 if mode == 4 else 0.0
    got = ops.logmel(x.to(DEV), n, hop, w.to(DEV), 1, nfr, fb.to(DEV), mode, log_guard=guard)
    torch.cuda.synchronize()
    r64, r32 = mel_refs(x, w, n, hop, 1, nfr, fb, mode, guard)
    check("logmel", (n, n_mels, mode), got.cpu(), r64, r32)


# measured on an MI355X: silent item: err 2.5e-7, e32 1.1e-7, peak 1.6, bar 2.0e-6 (0.12 of the bar)
def test_logmel_generic_whisper_maximum(ops, monkeypatch):
    """Mode 0 on the generic path at B = 3 with an all-zero item: its maximum is the clamp floor (-10), its rows all finish at (-10 + 4) / 4, and
    the other items keep their own maxima; then ``fixed_max``.  Float rule."""
    monkeypatch.setenv("MI355_FFT_FAST", "0")
    n, hop, L, n_mels = 250, 50, 1000, 40
    nfr = S.n_frames_of(L, n, hop, 1)
    x, w = S.ramp_noise(3, L, 77), S.hamming(n)
    x[1] = 0.0
    x[2] *= 1e-3
    fb = S.random_sparse_bank(n_mels, n // 2 + 1, 3)
    got = ops.logmel(x.to(DEV), n, hop, w.to(DEV), 1, nfr, fb.to(DEV), 0)
    torch.cuda.synchronize()
    r64, r32 = mel_refs(x, w, n, hop, 1, nfr, fb, 0)
    check("logmel", "gmax, one silent item", got.cpu(), r64, r32)
    silent = got[1].cpu()   # one value throughout: (log10f(1e-10f) + 4) / 4, -1.5 to a rounding of the logarithm
    assert bool((silent == silent[0, 0]).all()) and abs(float(silent[0, 0]) + 1.5) <= 2.0 ** -21
    fixed = float(r64[2].max()) * 4.0 - 4.0 + 1.0   # one decade above item 2's own maximum, far below item 0's
    got = ops.logmel(x.to(DEV), n, hop, w.to(DEV), 1, nfr, fb.to(DEV), 0, fixed_max=fixed)
    torch.cuda.synchronize()
    r64, r32 = mel_refs(x, w, n, hop, 1, nfr, fb, 0, fixed_max=fixed)
    check("logmel", "fixed_max", got.cpu(), r64, r32)


# ================================================================================================================= C. fast kernels
FAST_BANK = {400: (16000, 80), 512: (16000, 60), 1024: (24000, 100)}


def fast_bank(n_fft):
    sr, n_mels = FAST_BANK[n_fft]
    return S.slaney_bank(sr, n_fft, n_mels)


def run_fast(ops, xd, n, hop, wd, pad, nfr, fbd, mode):
    """(spectrum as floats, log-mel) of the fast kernels; the caller has set the environment."""
    spec = ops.stft_frames(xd, n, hop, wd, pad, nfr)
    mel = ops.logmel(xd, n, hop, wd, pad, nfr, fbd, mode, log_guard=2.0 ** -24 if mode == 4 else 0.0)
    return torch.view_as_real(spec), mel


# measured on an MI355X: every identity: bit-equal.  Against float64: spectrum (512, hop 130) err 1.6e-5, e32 1.9e-5, peak 104, bar 2.1e-4; log-mel (1024) err 1.2e-6,
# e32 1.2e-6, peak 6.8, bar 1.2e-5 (at most 0.10 of the bar)
@pytest.mark.parametrize("n_fft", [400, 512, 1024])
def test_fast_load_paths_are_bit_identical(ops, monkeypatch, n_fft):
    """stft_fast_kernel, ``inner && vec4`` against ``inner && !vec4`` on interior tiles (tests/test_dsp_refs_cpu.py asserts every case has at least two
    per item): the aligned contiguous launch against (i) x as a buf[1:1 + n] view (pointer % 16 == 4), (ii) L % 4 != 0 at B = 2 (ldx % 4 != 0: the
    same samples as a [:, :L] view of a buffer with ldx % 4 == 0 take the float4 path); (iii) a hop that is no multiple of 4 -- scalar either way, so
    the aligned buffer is compared with the misaligned one.  MODE 0 and MODE 1 (mode 2: no finish in between).  Exact: the arithmetic is identical,
    only the loads differ.  The aligned launch of (i) is also held to float64: kept bars (spectrum 2e-6 x peak) and the float rule (log-mel)."""
    monkeypatch.setenv("MI355_FFT_FAST", "1")
    monkeypatch.delenv("MI355_FFT_PREFETCH", raising=False)
    wd, fbd = S.hamming(n_fft).to(DEV), fast_bank(n_fft).to(DEV)
    hop = S.FAST_HOPS[n_fft]
    L0, L1 = S.load_path_lengths(n_fft, hop)
    x = S.ramp_noise(2, L0, n_fft)
    nfr = S.n_frames_of(L0, n_fft, hop, 1)
    xd = x.to(DEV)
    assert xd.data_ptr() % 16 == 0 and xd.stride(0) % 4 == 0
    s0, m0 = run_fast(ops, xd, n_fft, hop, wd, 1, nfr, fbd, 2)
    s1, m1 = run_fast(ops, misaligned(xd), n_fft, hop, wd, 1, nfr, fbd, 2)
    torch.cuda.synchronize()
    assert torch.equal(s0, s1) and torch.equal(m0, m1), "misaligned pointer"
    w = S.hamming(n_fft)
    r64 = S.stft_stmt(x, w, n_fft, hop, 1, nfr, F64)
    check("stft_fast", (n_fft, "aligned"), s0.cpu(), ri(r64), ri(S.stft_stmt(x, w, n_fft, hop, 1, nfr, F32)), existing=2e-6 * float(ri(r64).abs().max()))
    check("logmel_fast", (n_fft, "aligned"), m0.cpu(), *mel_refs(x, w, n_fft, hop, 1, nfr, fast_bank(n_fft), 2))
    # (ii)
    x1 = S.ramp_noise(2, L1, n_fft + 1)
    nfr1 = S.n_frames_of(L1, n_fft, hop, 1)
    wide = widened(x1, 3)[1]
    assert wide.stride(0) % 4 == 0 and wide.data_ptr() % 16 == 0 and L1 % 4 != 0
    s0, m0 = run_fast(ops, wide, n_fft, hop, wd, 1, nfr1, fbd, 2)
    s1, m1 = run_fast(ops, x1.to(DEV), n_fft, hop, wd, 1, nfr1, fbd, 2)
    torch.cuda.synchronize()
    assert torch.equal(s0, s1) and torch.equal(m0, m1), "ldx % 4 != 0"
    # (iii)
    hop3 = S.FAST_ODD_HOPS[n_fft]
    L3 = S.load_path_lengths(n_fft, hop3)[0]
    x3 = S.ramp_noise(2, L3, n_fft + 2).to(DEV)
    nfr3 = S.n_frames_of(L3, n_fft, hop3, 1)
    s0, m0 = run_fast(ops, x3, n_fft, hop3, wd, 1, nfr3, fbd, 2)
    s1, m1 = run_fast(ops, misaligned(x3), n_fft, hop3, wd, 1, nfr3, fbd, 2)
    torch.cuda.synchronize()
    assert torch.equal(s0, s1) and torch.equal(m0, m1), "hop % 4 != 0"
    r64 = S.stft_stmt(x3.cpu(), w, n_fft, hop3, 1, nfr3, F64)
    check("stft_fast", (n_fft, "hop", hop3), s0.cpu(), ri(r64), ri(S.stft_stmt(x3.cpu(), w, n_fft, hop3, 1, nfr3, F32)),
          existing=2e-6 * float(ri(r64).abs().max()))


# measured on an MI355X: all 12 outputs per size: bit-equal.  Alternating case against float64 (1024): err 2.7e-5, e32 2.0e-5, peak 179, bar 3.6e-4
@pytest.mark.parametrize("n_fft", [400, 512, 1024])
def test_fast_prefetch_configuration_is_bit_identical(ops, monkeypatch, n_fft):
    """MI355_FFT_PREFETCH=1 (four waves, the next tile's samples prefetched into registers by ``load_regs``) against the default configuration (six
    waves, no prefetch): MODE 0 and every mel mode.  A wave gets a second tile only when the launch has more tiles than are resident at once
    (``FastGeom.resident_tiles``, from the device's CU count), so the shapes are sized from that: (a) B = 3 with hop = 4 and a ragged last tile per
    item, total tiles = resident + 633, so the prefetch of a wave's next tile crosses into another item (another row of x); (b) many short items
    of three tiles each -- edge, interior, edge under reflect padding -- so edge and interior tiles alternate for a wave: an interior tile
    followed by an edge tile (no prefetch issued) and an edge tile followed by an interior one (``have`` is false: ``load_regs`` runs directly).  The
    hand-over of prefetched registers from one interior tile to the next is case (a)'s.  Compared on the device.  Exact: the arithmetic per tile is identical."""
    g = S.fast_geom_of(n_fft)
    T = 2 * g.PW
    wd, fb = S.hamming(n_fft).to(DEV), fast_bank(n_fft)
    fbd = fb.to(DEV)
    resident = max(g.resident_tiles(mel, True, cus()) for mel in (False, True))
    # (a)
    per_item = resident // 3 + 211
    nfr = per_item * T - 1
    hop, L = 4, (per_item * T - 2) * 4
    assert S.n_frames_of(L, n_fft, hop, 1) == nfr and 3 * per_item > resident and per_item < resident
    xa = S.ramp_noise(3, L, n_fft + 5).to(DEV)
    # (b)
    hop_b, Lb = S.alternating_case(n_fft)
    Bb = resident // 3 + 50
    nfr_b = S.n_frames_of(Lb, n_fft, hop_b, 1)
    assert S.tile_kinds(n_fft, hop_b, Lb, 1, nfr_b) == [False, True, False] and 3 * Bb > resident
    xb = S.ramp_noise(Bb, Lb, n_fft + 6).to(DEV)
    outs = {}
    for pref in ("0", "1"):
        monkeypatch.setenv("MI355_FFT_FAST", "1")
        monkeypatch.setenv("MI355_FFT_PREFETCH", pref)
        o = [ops.stft_frames(xa, n_fft, hop, wd, 1, nfr), ops.stft_frames(xb, n_fft, hop_b, wd, 1, nfr_b)]
        for mode in range(5):
            guard = 2.0 ** -24 if mode == 4 else 0.0
            o.append(ops.logmel(xa, n_fft, hop, wd, 1, nfr, fbd, mode, log_guard=guard))
            o.append(ops.logmel(xb, n_fft, hop_b, wd, 1, nfr_b, fbd, mode, log_guard=guard))
        torch.cuda.synchronize()
        outs[pref] = o
    for i, (a, b) in enumerate(zip(outs["0"], outs["1"])):
        assert bool(torch.isfinite(torch.view_as_real(a) if a.is_complex() else a).all()), i
        assert torch.equal(torch.view_as_real(a) if a.is_complex() else a, torch.view_as_real(b) if b.is_complex() else b), i
    # the alternating case also against float64 on a few items (MODE 0, kept bar 2e-6 x peak): bit-equal configurations could still share a mistake
    x4, w = xb[:4].cpu(), S.hamming(n_fft)
    r64 = S.stft_stmt(x4, w, n_fft, hop_b, 1, nfr_b, F64)
    check("stft_fast", (n_fft, "prefetch, alternating tiles"), ri(outs["1"][1][:4].cpu()), ri(r64), ri(S.stft_stmt(x4, w, n_fft, hop_b, 1, nfr_b, F32)),
          existing=2e-6 * float(ri(r64).abs().max()))


# measured on an MI355X: worst: spectrum (400, n_frames 1) err 3.5e-6, e32 3.0e-6, peak 25, bar 5.1e-5; log-mel (400, n_frames 6) err 2.3e-7, e32 1.3e-7, bar 2.0e-6
@pytest.mark.parametrize("which", S.SHORT_LAUNCHES)
@pytest.mark.parametrize("n_fft", [400, 512, 1024])
def test_fast_short_launches(ops, monkeypatch, n_fft, which):
    """n_frames = 1, 2 PW - 1, 2 PW, 2 PW + 1 (PW frame pairs per wave tile): fewer frames than one tile, exactly one, one and a single frame -- and
    at n_frames = 1, B = 1 fewer tiles than the waves of one workgroup.  Constant padding, so that one frame is admissible.  MODE 0: kept bar
    2e-6 x peak; MODE 1 (mode 0 with its maximum): float rule."""
    monkeypatch.setenv("MI355_FFT_FAST", "1")
    monkeypatch.delenv("MI355_FFT_PREFETCH", raising=False)
    hop, L, nfr, B = S.short_launch_case(n_fft, which)
    assert S.n_frames_of(L, n_fft, hop, 2) == nfr
    x, w, fb = S.ramp_noise(B, L, n_fft + nfr), S.hamming(n_fft), fast_bank(n_fft)
    spec, mel = run_fast(ops, x.to(DEV), n_fft, hop, w.to(DEV), 2, nfr, fb.to(DEV), 0)
    torch.cuda.synchronize()
    r64 = S.stft_stmt(x, w, n_fft, hop, 2, nfr, F64)
    check("stft_fast", (n_fft, "n_frames", nfr), spec.cpu(), ri(r64), ri(S.stft_stmt(x, w, n_fft, hop, 2, nfr, F32)), existing=2e-6 * float(ri(r64).abs().max()))
    check("logmel_fast", (n_fft, "n_frames", nfr), mel.cpu(), *mel_refs(x, w, n_fft, hop, 2, nfr, fb, 0))


MEL_BOUNDARY = [
    # n_fft, bank (sr, n_mels), mode, on the fast kernel?
    (400, (16000, 235), 0, True),     # fills a wave's slice exactly (FastGeom<20, 20>: 4824 + 5640 = 10464 B)
    (400, (16000, 236), 0, False),    # one more row: mel_fits fails, the LDS Stockham kernel takes it
    (400, (16000, 160), 4, True),     # Slaney banks with all-zero rows (span_len = 0): 4, 34 and 24 of them
    (400, (16000, 234), 1, True),
    (512, (16000, 256), 3, True),     # kMaxMels
    (1024, (24000, 256), 2, True),
    (512, (16000, 257), 2, False),    # past kMaxMels
]


# measured on an MI355X: worst on the fast kernel: (1024, 256 mels, mode 2) err 2.1e-5, e32 1.5e-5, peak 10, bar 7.1e-5 (0.29); on the Stockham fallback: (512, 257 mels, mode 2)
# err 4.0e-5, e32 1.1e-5, peak 18, bar 6.4e-5 (0.63); (400, 235, mode 0) err 3.6e-6 of bar 2.3e-5; (400, 236, mode 0) err 4.9e-6 of bar 1.1e-5
@pytest.mark.parametrize("n_fft,bank,mode,fast", MEL_BOUNDARY, ids=lambda v: str(v).replace(" ", ""))
def test_fast_mel_slice_boundaries(ops, monkeypatch, n_fft, bank, mode, fast):
    """MODE 1 at the edges of ``mel_fits`` and ``kMaxMels``, B = 2 with at least 12 tiles so that all six wave slices of a workgroup are live at once
    (an off-by-one in the slice arithmetic writes into the next wave's slice), and Slaney banks with empty rows.  ``fast`` is what
    FastGeom.mel_fits / kMaxMels say the launcher does; either way the result is held to float64.  Float rule."""
    monkeypatch.setenv("MI355_FFT_FAST", "1")
    monkeypatch.delenv("MI355_FFT_PREFETCH", raising=False)
    g = S.fast_geom_of(n_fft)
    n_mels = bank[1]
    assert fast == (g.mel_fits(n_mels) and n_mels <= S.K_MAX_MELS)
    hop = S.FAST_HOPS[n_fft]
    nfr = 6 * 2 * g.PW + 1
    L = (nfr - 1) * hop
    assert 2 * ((nfr + 2 * g.PW - 1) // (2 * g.PW)) >= 12 and S.n_frames_of(L, n_fft, hop, 1) == nfr
    x, w, fb = S.ramp_noise(2, L, n_fft + n_mels), S.hamming(n_fft), S.slaney_bank(bank[0], n_fft, n_mels)
    guard = 2.0 ** -24 if mode == 4 else 0.0
    got = ops.logmel(x.to(DEV), n_fft, hop, w.to(DEV), 1, nfr, fb.to(DEV), mode, log_guard=guard)
    torch.cuda.synchronize()
    check("logmel_fast" if fast else "logmel", (n_fft, n_mels, mode), got.cpu(), *mel_refs(x, w, n_fft, hop, 1, nfr, fb, mode, guard))


# measured on an MI355X: 1536 (LDS): err 1.0e-6; 1537 (L2): err 1.3e-6; e32 4.0e-7, peak 7.6, bar 9.2e-6; LDS against L2 on the shared rows: 9.5e-7 (not zero)
def test_fast_filterbank_capacity(ops, monkeypatch):
    """kFbCap: two banks at n_fft 512 whose span totals are exactly 1536 (the compacted rows are resident in LDS) and 1537 (they are read from L2),
    one row with zeros inside its span.  Both against float64, and against each other on the rows they share: the resident path keeps two running
    sums (even / odd terms), the L2 path sums ascending, so that bar is the float rule's as well, not equality.  Float rule."""
    monkeypatch.setenv("MI355_FFT_FAST", "1")
    monkeypatch.delenv("MI355_FFT_PREFETCH", raising=False)
    a, b = S.cap_banks()
    n_fft, hop, L = 512, 128, 128 * 24
    nfr = S.n_frames_of(L, n_fft, hop, 1)
    x, w = S.ramp_noise(2, L, 1536), S.hamming(n_fft)
    ga = ops.logmel(x.to(DEV), n_fft, hop, w.to(DEV), 1, nfr, a.to(DEV), 2).cpu()
    gb = ops.logmel(x.to(DEV), n_fft, hop, w.to(DEV), 1, nfr, b.to(DEV), 2).cpu()
    torch.cuda.synchronize()
    ra64, ra32 = mel_refs(x, w, n_fft, hop, 1, nfr, a, 2)
    rb64, rb32 = mel_refs(x, w, n_fft, hop, 1, nfr, b, 2)
    check("logmel_fast", "span total 1536 (LDS)", ga, ra64, ra32)
    check("logmel_fast", "span total 1537 (L2)", gb, rb64, rb32)
    shared = a.shape[0] - 1
    e32 = float((ra32[..., :shared].double() - ra64[..., :shared]).abs().max())
    bar = 4.0 * e32 + 1e-6 * float(ra64[..., :shared].abs().max())
    err = float((ga[..., :shared] - gb[..., :shared]).abs().max())
    print(f"EDGE logmel_fast LDS-vs-L2 err={err:.3e} e32={e32:.3e} bar={bar:.3e}")
    assert err <= bar
    # ... and not equality either: 350 sums of 192 terms in two different orders do not all round alike, so bit-equal shared rows mean that both
    # banks took the same path (kFbCap compared with < instead of <=, or a capacity that is not 1536)
    assert err > 0.0, "both banks took the same path"


# measured on an MI355X: err 2.7e-7, e32 2.3e-7, peak 3.5, bar 4.4e-6
def test_fast_whisper_maximum_across_items(ops, monkeypatch):
    """Mode 0 ``gmax`` on the fast kernel at B = 3 with more tiles than are resident, so a wave walks from item 0 into a later item within one launch
    and must flush item 0's running maximum when the item changes; the maximum of item 0 lies in its LAST tile (a burst 30 000 times louder than the
    body, which therefore clamps to max - 8 nearly everywhere: a lost maximum changes most of the item).  Float rule."""
    monkeypatch.setenv("MI355_FFT_FAST", "1")
    monkeypatch.delenv("MI355_FFT_PREFETCH", raising=False)
    n_fft, hop = 400, 4
    g = S.fast_geom_of(n_fft)
    T = 2 * g.PW
    resident = g.resident_tiles(True, False, cus())
    per_item = resident // 2 + 64
    nfr = per_item * T
    L = (nfr - 1) * hop
    assert S.n_frames_of(L, n_fft, hop, 1) == nfr and resident // 2 < per_item < resident
    x, w = S.ramp_noise(3, L, 4321), S.hamming(n_fft)
    x[0, L - 8:] *= 3e4
    fb = S.slaney_bank(16000, n_fft, 20)
    got = ops.logmel(x.to(DEV), n_fft, hop, w.to(DEV), 1, nfr, fb.to(DEV), 0)
    torch.cuda.synchronize()
    r64, r32 = mel_refs(x, w, n_fft, hop, 1, nfr, fb, 0)
    raw = S.logmel_stmt(x[:1], w, n_fft, hop, 1, nfr, fb, 0, F64)[0]
    assert int(raw.amax(dim=1).argmax()) >= nfr - T                    # the maximum is in the last tile
    assert float((raw < raw.max() - 8.0).double().mean()) > 0.5        # and most of the item clamps to it
    check("logmel_fast", "gmax across items", got.cpu(), r64, r32)


# ================================================================================================================= D. mi355_istft
# measured on an MI355X, worst by err / bar: clamp launch (1024, hop 256, 1 frame) err 2.7e-6, e32 1.7e-6, peak 1.0, bar 7.9e-6 (0.35 of the bar); norm_mode 1
# and norm_mode 0 launches (960, hop 960, 8 frames) err 2.9e-6, e32 2.8e-6, peak 3.9, bar 1.5e-5 (0.19); gaps under norm_mode 1: exact zeros
@pytest.mark.parametrize("n_fft,hop,nfr", S.ISTFT_CASES)
def test_istft_edges(ops, n_fft, hop, nfr):
    """mi355_istft at n_fft 2 ... 1024 (radix 61 and DeepFilterNet's 960 among them), odd and even frame counts and a single frame (the ``nf_even``
    partner row of the last pair), hop = n_fft / 4, hop = n_fft, hop = n_fft + 3 (gaps: empty f_lo .. f_hi ranges; the samples there are exactly 0 under
    norm_mode 1) and hop = 1; spectra from the float64 STFT of unit noise, with junk in the imaginary parts irfft ignores.  Three launches per case:
    norm_mode 1 with the centre trim; norm_mode 0 with trim = 0 and the full length (DeepFilterNet, ISTFTCache); clamp = 1 on the spectrum times
    ISTFT_CLAMP_GAIN (5 % .. 50 % of the samples exceed this window, asserted for this spectrum and window in tests/test_dsp_refs_cpu.py) with the output cut short.
    Kept bar 5e-5 on the norm_mode 1 / centre-trim launch at n_fft 20 / 96 / 1024 with hop = n_fft / 4 (the launch and sizes of
    test_dsp_stft_istft_roundtrip_and_oracle, unit noise); float rule on every other launch."""
    spec, w = S.istft_inputs(n_fft, hop, nfr)
    total = (nfr - 1) * hop + n_fft
    kept = 5e-5 if (n_fft in (20, 96, 1024) and hop == n_fft // 4) else None
    junk = spec.clone()
    junk.imag[..., 0] = 0.25
    junk.imag[..., -1] = -0.5
    sd, wd = junk.to(DEV), w.to(DEV)
    env1 = S.ola_envelope(w, nfr, hop, squared=True)
    env0 = S.ola_envelope(w, nfr, hop, squared=True, floor=1e-10)
    runs = []
    trim = n_fft // 2 if total - n_fft > 0 else 0
    runs.append(("norm1-trim", sd, spec, env1, 1, False, trim, total - 2 * trim))
    runs.append(("norm0-full", sd, spec, env0, 0, False, 0, total))
    g = S.ISTFT_CLAMP_GAIN
    cut = max(1, total - n_fft // 2 - 3)
    runs.append(("clamp-cut", (spec * g).to(DEV), spec * g, env0, 0, True, n_fft // 2, cut))
    for name, s_dev, s_ref, env, norm_mode, clamp, tr, out_len in runs:
        got = ops.istft_frames(s_dev, n_fft, hop, wd, env.to(DEV), norm_mode, clamp, tr, out_len)
        torch.cuda.synchronize()
        r64 = S.istft_stmt(s_ref, w, n_fft, hop, env, norm_mode, clamp, tr, out_len, F64)
        r32 = S.istft_stmt(s_ref, w, n_fft, hop, env, norm_mode, clamp, tr, out_len, F32)
        check("istft", (n_fft, hop, nfr, name), got.cpu(), r64, r32, existing=kept if name == "norm1-trim" else None)
        if hop > n_fft and norm_mode == 1:
            gap = (env[tr:tr + out_len] == 0)
            assert int(gap.sum()) > 0 and bool((got.cpu()[:, gap] == 0).all())


# measured on an MI355X: dsp.istft (length = 100): err 1.4e-6, e32 1.5e-6, peak 3.6, bar 9.5e-6; ISTFTCache: err 1.2e-7, e32 1.3e-7, bar 1.5e-6
def test_istft_refusals_and_wrappers(ops, E):
    """Refusals (trim + out_len past the overlap-add range; odd n_fft), then the two public wrappers once each: dsp.istft with ``length``, with
    center = False, normalized True / False, and ISTFTCache.istft with ``audio_length`` and constrain_value_range = True.  Float rule."""
    from mlx_audio_amd import dsp

    n_fft, hop, nfr = 96, 24, 7
    spec, w = S.istft_inputs(n_fft, hop, nfr)
    total = (nfr - 1) * hop + n_fft
    env = S.ola_envelope(w, nfr, hop, squared=True)
    with pytest.raises(E, match="outside the overlap-add range"):
        ops.istft_frames(spec.to(DEV), n_fft, hop, w.to(DEV), env.to(DEV), 1, False, n_fft // 2, total - n_fft // 2 + 1)
    with pytest.raises(E, match="bad shape"):
        ops.istft_frames(spec[..., :8].to(DEV), 15, 5, w[:15].to(DEV), env.to(DEV), 1, False, 0, 10)
    xs = spec.transpose(1, 2)   # [B, bins, frames]
    for kw, (squared, trim, out_len) in [
        (dict(length=100, normalized=True), (True, 0, 100)),
        (dict(center=False, normalized=False), (False, 0, total)),
        (dict(center=True, normalized=True), (True, n_fft // 2, total - n_fft)),
    ]:
        got = dsp.istft(xs.to(DEV), hop_length=hop, win_length=n_fft, window=w, **kw)
        torch.cuda.synchronize()
        e = S.ola_envelope(w, nfr, hop, squared=squared)
        check("dsp.istft", tuple(kw.items()), got.cpu(), S.istft_stmt(spec, w, n_fft, hop, e, 1, False, trim, out_len, F64),
              S.istft_stmt(spec, w, n_fft, hop, e, 1, False, trim, out_len, F32))
    e0 = S.ola_envelope(w, nfr, hop, squared=True, floor=1e-10)
    sg = spec * S.ISTFT_CLAMP_GAIN
    got = dsp.ISTFTCache().istft(sg.real.transpose(1, 2).to(DEV), sg.imag.transpose(1, 2).to(DEV), n_fft, hop, n_fft, w, center=True, audio_length=111,
                                 constrain_value_range=True)
    torch.cuda.synchronize()
    check("ISTFTCache.istft", "audio_length, clamp", got.cpu(), S.istft_stmt(sg, w, n_fft, hop, e0, 0, True, n_fft // 2, 111, F64),
          S.istft_stmt(sg, w, n_fft, hop, e0, 0, True, n_fft // 2, 111, F32))


# ================================================================================================================= E. small-FFT heads
def check_magphase(name, case, got, r64, r32, nb):
    """Magnitude: float rule.  Phase: kept bar 1e-3 modulo 2 pi at the bins whose float64 magnitude is >= 1e-4.  Sentinel rows: exact."""
    live = r64[..., :1] != SENTINEL
    assert torch.equal(got[~live.expand_as(got)], torch.full_like(got[~live.expand_as(got)], SENTINEL)), (name, case, "rows past the length were written")
    z = torch.zeros_like(r64)
    g64, g32, gg = torch.where(live, r64, z), torch.where(live, r32.double(), z), torch.where(live, got.double(), z)
    check(name, (case, "mag"), gg[..., :nb].float(), g64[..., :nb], g32[..., :nb])
    d = (gg[..., nb:] - g64[..., nb:]).abs()
    d = torch.minimum(d, 2 * math.pi - d)
    big = live.expand_as(d) & (g64[..., :nb] >= 1e-4)
    perr = float(d[big].max())
    print(f"EDGE {name} {case} phase err={perr:.3e} bins={int(big.sum())} of {int(live.expand_as(d).sum())} bar=1.000e-03")
    assert perr <= 1e-3


def run_magphase(ops, x, n_fft, hop, w, lens):
    """x as a [:, :L] view of a wider buffer, y as the leading 2 nb columns of a buffer three columns wider, pre-filled with the sentinel."""
    B, L = x.shape
    nb = n_fft // 2 + 1
    rows = S.magphase_frames(L, hop)
    xd = widened(x, 5)[1]
    ybuf = torch.full((B, rows, 2 * nb + 3), SENTINEL, device=DEV)
    ld = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
    ops.stft_magphase(xd, n_fft, hop, w.to(DEV), ybuf[..., :2 * nb], lens=ld)
    torch.cuda.synchronize()
    assert bool((ybuf[..., 2 * nb:] == SENTINEL).all())
    return ybuf[..., :2 * nb].cpu()


# measured on an MI355X: worst magnitude: (64, hop 1) err 1.5e-6, e32 1.9e-6, peak 12.4, bar 2.0e-5; worst phase: (15, hop 5) 5.7e-6 of 1e-3
@pytest.mark.parametrize("n_fft,hop", S.HEAD_GENERIC)
def test_stft_magphase_generic_edges(ops, n_fft, hop):
    """stft_magphase_kernel (every (n_fft, hop) but (20, 5)): 16 / 4; odd n_fft 15 / 5; n_fft = 64 = kMaxSmallFft at hop 16 and hop 1; 20 / 4, the
    generic kernel next to the fast size.  Full lengths, then ragged ``lens`` with the shortest item at n_fft / 2 + 1 samples; strided x and y."""
    L, lens = S.magphase_generic_case(n_fft, hop)
    x, w = S.magphase_input(3, L, n_fft * hop), S.hann_periodic(n_fft)
    for ln in (None, lens):
        got = run_magphase(ops, x, n_fft, hop, w, ln)
        check_magphase("stft_magphase", (n_fft, hop, "lens" if ln else "full"), got, S.magphase_stmt(x, w, n_fft, hop, F64, lens=ln),
                       S.magphase_stmt(x, w, n_fft, hop, F32, lens=ln), n_fft // 2 + 1)


# measured on an MI355X: worst magnitude: (L 1272) err 7.7e-7, e32 1.1e-6, peak 7.4, bar 1.2e-5; worst phase 1.4e-6 of 1e-3
def test_stft_magphase_fast_edges(ops):
    """stft_magphase_fast_kernel<20, 5> at 3 (the fewest frames L > n_fft / 2 allows), 255, 256, 257 and 600 frames (256 frames per workgroup), then
    ragged ``lens`` [700, 11, 403]; strided x and y."""
    w = S.hann_periodic(20)
    for L in S.MAGPHASE_FAST_LENGTHS:
        x = S.magphase_input(2, L, L)
        got = run_magphase(ops, x, 20, 5, w, None)
        check_magphase("stft_magphase_fast", (L, "full"), got, S.magphase_stmt(x, w, 20, 5, F64), S.magphase_stmt(x, w, 20, 5, F32), 11)
    x, lens = S.magphase_input(3, 700, 9), [700, 11, 403]
    got = run_magphase(ops, x, 20, 5, w, lens)
    check_magphase("stft_magphase_fast", "lens", got, S.magphase_stmt(x, w, 20, 5, F64, lens=lens), S.magphase_stmt(x, w, 20, 5, F32, lens=lens), 11)


def run_head(ops, x, n_fft, hop, w, lens):
    """x as the leading 2 nb columns of a buffer five columns wider; audio with ld_audio seven samples larger than the length, sentinel-filled."""
    B, Fr, _ = x.shape
    nb = n_fft // 2 + 1
    xd = widened(x, 5)[1]
    abuf = torch.full((B, (Fr - 1) * hop + 7), SENTINEL, device=DEV)
    ld = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
    ops.istft_head(xd, n_fft, hop, w.to(DEV), abuf, lens=ld)
    torch.cuda.synchronize()
    assert bool((abuf[:, (Fr - 1) * hop:] == SENTINEL).all())
    return abuf[:, :(Fr - 1) * hop].cpu()


def check_head(name, case, got, r64, r32, existing=None):
    live = r64 != SENTINEL
    assert bool((got[~live] == SENTINEL).all()), (name, case, "samples past the length were written")
    z = torch.zeros_like(r64)
    check(name, case, torch.where(live, got.double(), z).float(), torch.where(live, r64, z), torch.where(live, r32.double(), z), existing=existing)


# measured on an MI355X: worst: (64, hop 1, lens) err 9.8e-9, e32 9.5e-9, peak 2.4e-2, bar 6.2e-8 (0.16 of the bar)
@pytest.mark.parametrize("n_fft,hop", S.HEAD_GENERIC)
def test_istft_head_generic_edges(ops, n_fft, hop):
    """istft_head_kernel at the sizes above (odd n_fft: no Nyquist term; hop = 1 at n_fft = 64: a halo of 64 frames staged per block), Fr = 101 (several
    blocks of 48 frames), then ragged ``lens`` [101, 2, 67]; strided x, ld_audio larger than the length.  Float rule."""
    nb = n_fft // 2 + 1
    x, w = S.head_input(3, 101, nb, n_fft + hop), S.hann_periodic(n_fft)
    for ln in (None, [101, 2, 67]):
        got = run_head(ops, x, n_fft, hop, w, ln)
        check_head("istft_head", (n_fft, hop, "lens" if ln else "full"), got, S.head_stmt(x, w, n_fft, hop, F64, lens=ln),
                   S.head_stmt(x, w, n_fft, hop, F32, lens=ln))


# measured on an MI355X: worst: Fr 252: err 3.8e-8, e32 3.9e-8, peak 0.23, bar 3.8e-7 (0.10 of the bar)
def test_istft_head_fast_edges(ops):
    """istft_head_fast_kernel<20, 5> at Fr = 2, 252, 253, 260 (FO = 252 output frames per workgroup) and ragged ``lens`` with a two-frame item.
    Float rule (it is tighter here than test_istft_head's 2e-6: the audio peaks at 0.23)."""
    w = S.hann_periodic(20)
    for Fr in S.HEAD_FAST_FRAMES:
        x = S.head_input(2, Fr, 11, Fr)
        got = run_head(ops, x, 20, 5, w, None)
        check_head("istft_head_fast", Fr, got, S.head_stmt(x, w, 20, 5, F64), S.head_stmt(x, w, 20, 5, F32))
    x, lens = S.head_input(3, 300, 11, 5), [300, 2, 253]
    got = run_head(ops, x, 20, 5, w, lens)
    check_head("istft_head_fast", "lens", got, S.head_stmt(x, w, 20, 5, F64, lens=lens), S.head_stmt(x, w, 20, 5, F32, lens=lens))


# ================================================================================================================= F. kaldi_frames, polar_spec
# measured on an MI355X: worst: (win 1920, noise, preemph 0) err 6.4e-7, e32 6.4e-7, peak 6.8, bar 9.3e-6 (0.07 of the bar)
@pytest.mark.parametrize("noise,preemph", [(False, 0.0), (True, 0.97), (False, 0.97), (True, 0.0)])
@pytest.mark.parametrize("c", S.KALDI_CASES, ids=lambda c: f"win{c['win']}")
def test_kaldi_frames_edges(ops, c, noise, preemph):
    """mi355_kaldi_frames at win < 64 (25 into n_fft 32), win = 400 < n_fft = 512 with pad = 120 at the exact admissible limit, win = 1920 (several
    trips of the 256-lane loop), win = n_fft = 300 with pad = 100 at the limit; with and without dither noise, preemph 0 and 0.97.  Float rule."""
    win, n_fft, shift, pad, nfr, L = c["win"], c["n_fft"], c["shift"], c["pad"], c["n_frames"], c["L"]
    x, w = S.ramp_noise(1, L, win)[0], S.hamming(win)
    nz = S.unit_noise((nfr, win), win + 1) if noise else None
    got = ops.kaldi_frames(x.to(DEV), win, shift, pad, n_fft, nfr, w.to(DEV), preemph, noise=None if nz is None else nz.to(DEV), dither=0.5 if noise else 0.0)
    torch.cuda.synchronize()
    dither = 0.5 if noise else 0.0
    check("kaldi_frames", (win, n_fft, shift, pad, nfr, noise, preemph), got.cpu(), S.kaldi_stmt(x, win, shift, pad, n_fft, nfr, w, preemph, nz, dither, F64),
          S.kaldi_stmt(x, win, shift, pad, n_fft, nfr, w, preemph, nz, dither, F32))


def test_kaldi_frames_refusals(ops, E):
    """One frame past the admissible limit, and pad = L.  Exact (status and text; nothing is launched)."""
    for c in S.KALDI_CASES:
        if c["limit"]:
            with pytest.raises(E, match="run past the reflected edges"):
                ops.kaldi_frames(torch.zeros(c["L"], device=DEV), c["win"], c["shift"], c["pad"], c["n_fft"], c["n_frames"] + 1,
                                 torch.ones(c["win"], device=DEV), 0.0)
    with pytest.raises(E, match="run past the reflected edges"):
        ops.kaldi_frames(torch.zeros(50, device=DEV), 25, 10, 50, 32, 2, torch.ones(25, device=DEV), 0.0)


# measured on an MI355X: worst: (2, 3, 513, 1030) err 9.1e-6, e32 9.4e-6, peak 100, bar 1.4e-4 (0.07 of the bar)
@pytest.mark.parametrize("i", range(len(S.POLAR_CASES)))
def test_polar_spec_edges(ops, i):
    """mi355_polar_spec at a single bin, at nb = 513 with ldx = 1030 > 2 nb, and with a batch stride larger than Fr * ldx; the log-magnitudes straddle
    ln(clip) (tests/test_dsp_refs_cpu.py), and where they exceed it the magnitude is the clip.  Float rule."""
    B, Fr, nb, ldx, bs = S.POLAR_CASES[i]
    bs = bs or Fr * ldx
    x = S.polar_input(B, Fr, nb, i)
    buf = torch.full((B * bs,), SENTINEL, device=DEV)
    xd = buf.as_strided((B, Fr, 2 * nb), (bs, ldx, 1))
    xd.copy_(x)
    got = ops.polar_spec(xd, nb, S.POLAR_CLIP)
    torch.cuda.synchronize()
    g = torch.view_as_real(got).cpu()
    check("polar_spec", S.POLAR_CASES[i], g, S.polar_stmt(x, nb, S.POLAR_CLIP, F64), S.polar_stmt(x, nb, S.POLAR_CLIP, F32))
    clipped = x[..., :nb] > math.log(S.POLAR_CLIP) + 1e-3
    mag = torch.sqrt(g[..., 0].double() ** 2 + g[..., 1].double() ** 2)
    assert float((mag[clipped] - S.POLAR_CLIP).abs().max() if clipped.any() else 0.0) <= 1e-4 * S.POLAR_CLIP
    assert float(mag.max()) <= S.POLAR_CLIP * (1 + 1e-6)
