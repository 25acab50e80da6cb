"""The reference statements of tests/test_dsp_kernel_edges_gpu.py held to known-good implementations, and the preconditions of its case tables, on
the CPU: a failure of the GPU file then cannot be the reference's or the inputs' fault, and a case that claims to reach a branch it does not reach
fails here, before any GPU run.  Statements, tables and the restated host arithmetic live in tests/_dsp_cases.py, which both files import.

Agreement bars.  Against an implementation that works in float64 throughout (numpy's FFT on explicitly padded frames, oracle/dsp_ref.py's
``whisper_log_mel_f64``): 1e-12 relative to the peak.  oracle/dsp_ref.py's ``stft`` / ``istft`` / ``ISTFTCache`` / ``compute_fbank_kaldi`` round
their frames, products and results to float32 as the reference does, so a float64 statement cannot agree with them to 1e-12; those are held to a few
float32 roundings of the peak (3e-7 relative; 2e-5 absolute on the Kaldi log-mel), which still catches every mistake of layout, padding, ordering
or normalisation."""
import math

import numpy as np
import pytest
import torch

import _dsp_cases as S
from oracle import dsp_ref

F64 = torch.float64


def rel(a, b):
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


# ----------------------------------------------------------------------------------------------------------------- statements
@pytest.mark.parametrize("c", S.STOCKHAM_CASES, ids=S.stockham_id)
def test_stft_statement_is_numpy_rfft_of_padded_frames(c):
    """stft_stmt in float64 against np.pad (reflect / constant) + np.fft.rfft: 1e-12; and against oracle/dsp_ref.py's stft on each item (float32
    products and a complex64 result there: 3e-7) wherever the case's frame count is dsp.stft's own."""
    n, hop, L, pad = c["n_fft"], c["hop"], c["L"], c["pad"]
    nfr = S.stockham_frames(c)
    x, w = S.ramp_noise(c["B"], L, n), S.hamming(n)
    got = S.stft_stmt(x, w, n, hop, pad, nfr, F64)
    xp = x.numpy().astype(np.float64)
    if pad:
        xp = np.pad(xp, [(0, 0), (n // 2, n // 2)], mode="reflect" if pad == 1 else "constant")
    idx = np.arange(nfr)[:, None] * hop + np.arange(n)[None, :]
    want = np.fft.rfft(xp[:, idx] * w.numpy().astype(np.float64), axis=-1)
    assert got.shape == (c["B"], nfr, n // 2 + 1)
    assert rel(got, torch.from_numpy(want)) <= 1e-12
    if nfr == S.n_frames_of(L, n, hop, pad):
        kw = dict(center=False) if pad == 0 else dict(pad_mode="reflect" if pad == 1 else "constant")
        o = np.stack([dsp_ref.stft(r, n_fft=n, hop_length=hop, window=w.numpy(), **kw) for r in x.numpy()])
        assert o.shape == tuple(got.shape) and rel(got, torch.from_numpy(o).to(torch.complex128)) <= 3e-7


def test_whisper_statement_is_the_float64_oracle():
    """logmel_stmt mode 0 + whisper_finish_stmt in float64 against oracle/dsp_ref.py whisper_log_mel_f64 (float64 throughout): 1e-12.  The oracle
    drops the last frame and uses the symmetric Hann window in float64 and the float32 Slaney bank."""
    x = S.ramp_noise(1, 4000, 7)
    want = dsp_ref.whisper_log_mel_f64(x[0].numpy(), n_mels=80)
    k = np.arange(400, dtype=np.float64)
    w64 = torch.from_numpy(0.5 * (1.0 - np.cos(2.0 * np.pi * k / 399)))
    fb = torch.from_numpy(dsp_ref.mel_filters(16000, 400, 80, norm="slaney", mel_scale=None))
    nfr = S.n_frames_of(4000, 400, 160, 1) - 1
    raw = S.logmel_stmt(x, w64, 400, 160, 1, nfr, fb, 0, F64)
    y = S.whisper_finish_stmt(raw)
    assert y.shape[1:] == want.shape and rel(y[0], torch.from_numpy(want)) <= 1e-12
    # a fixed maximum replaces the item's own
    assert torch.equal(S.whisper_finish_stmt(raw, fixed_max=1.5), (torch.maximum(raw, torch.tensor(1.5 - 8.0, dtype=F64)) + 4.0) / 4.0)
    # the maximum is per item: a silent item sits on the clamp floor and does not pull the other item up or down
    x2 = torch.cat([x, torch.zeros_like(x)])
    y2 = S.whisper_finish_stmt(S.logmel_stmt(x2, w64, 400, 160, 1, nfr, fb, 0, F64))
    assert torch.equal(y2[0], y[0]) and torch.equal(y2[1], torch.full_like(y2[1], (-10.0 + 4.0) / 4.0))


@pytest.mark.parametrize("mode", [1, 2, 3, 4])
def test_logmel_modes_are_the_header_formulas(mode):
    """Modes 1 - 4 spelled out once more with numpy on the float64 spectrum (mode 1 is qwen3_mel_spectrogram's chain, mode 2 compute_fbank_kaldi's,
    mode 3 Vocos's, mode 4 NeMo's)."""
    x, w = S.ramp_noise(2, 1000, 3), S.hamming(250)
    fb = S.random_sparse_bank(40, 126, 1, zero_rows=(0, 17))
    nfr = S.n_frames_of(1000, 250, 50, 1)
    X = S.stft_stmt(x, w, 250, 50, 1, nfr, F64).numpy()
    p = np.abs(X) ** 2
    if mode == 1:
        p = np.sqrt(p + 1e-9)
    if mode == 3:
        p = np.sqrt(p)
    mel = p @ fb.numpy().astype(np.float64).T
    want = np.log(mel + 2.0 ** -24) if mode == 4 else np.log(np.maximum(mel, {1: 1e-5, 2: 1e-8, 3: 1e-5}[mode]))
    got = S.logmel_stmt(x, w, 250, 50, 1, nfr, fb, mode, F64, log_guard=2.0 ** -24)
    assert rel(got, torch.from_numpy(want)) <= 1e-12


@pytest.mark.parametrize("n_fft,hop,nfr", [c for c in S.ISTFT_CASES if c[2] > 1 and c[0] <= 122])
def test_istft_statement_is_the_oracle(n_fft, hop, nfr):
    """istft_stmt (norm_mode 1, plain and squared window envelope, centre trim and ``length``) against oracle/dsp_ref.py's istft, and (norm_mode 0,
    with and without the clamp) against its ISTFTCache.  Both oracles hold float32 frames and sums: 3e-7 of the peak, compared where the envelope is
    a sound divisor (the periodic Hann starts at 0, and a float32 sum over a near-zero float32 envelope is not a yardstick for anything)."""
    total = (nfr - 1) * hop + n_fft
    x, w = S.unit_noise((2, total), n_fft + hop), S.hann_periodic(n_fft)
    spec = S.stft_stmt(x, S.hamming(n_fft), n_fft, hop, 0, nfr, F64)

    def close(got, want, env):
        assert want.shape == tuple(got.shape)
        ok = (env > 1e-3)[None].expand_as(got)
        assert float((got - torch.from_numpy(want).double())[ok].abs().max()) <= 3e-7 * float(got[ok].abs().max())

    for normalized in (False, True):
        env = S.ola_envelope(w, nfr, hop, squared=normalized)
        for length in (None, total - 3):
            trim = n_fft // 2 if length is None else 0
            out_len = total - 2 * trim if length is None else length
            got = S.istft_stmt(spec, w, n_fft, hop, env, 1, False, trim, out_len, F64)
            want = np.stack([dsp_ref.istft(s.numpy().T, hop_length=hop, win_length=n_fft, window=w.numpy(), length=length, normalized=normalized)
                             for s in spec])
            close(got, want, env[trim:trim + out_len])
    env0 = S.ola_envelope(w, nfr, hop, squared=True, floor=1e-10)
    for clamp in (False, True):
        got = S.istft_stmt(spec * 0.05, w, n_fft, hop, env0, 0, clamp, n_fft // 2, total - n_fft // 2, F64)
        want = dsp_ref.ISTFTCache().istft((spec.real * 0.05).transpose(1, 2).numpy(), (spec.imag * 0.05).transpose(1, 2).numpy(), n_fft, hop, n_fft,
                                           w.numpy(), constrain_value_range=clamp)
        close(got, want, env0[n_fft // 2:])


def test_istft_statement_ignores_the_imaginary_parts_irfft_ignores():
    spec = S.stft_stmt(S.unit_noise((1, 200), 1), S.hamming(20), 20, 5, 0, 37, F64)
    w = S.hann_periodic(20)
    env = S.ola_envelope(w, 37, 5, squared=True)
    a = S.istft_stmt(spec, w, 20, 5, env, 1, False, 10, 180, F64)
    junk = spec.clone()
    junk.imag[..., 0] = 0.25
    junk.imag[..., -1] = -0.5
    assert torch.equal(a, S.istft_stmt(junk, w, 20, 5, env, 1, False, 10, 180, F64))
    want = np.fft.irfft(junk[0].numpy(), n=20, axis=-1)   # numpy ignores them too
    assert np.abs(want - np.fft.irfft(spec[0].numpy(), n=20, axis=-1)).max() <= 1e-14


@pytest.mark.parametrize("c", S.KALDI_CASES, ids=lambda c: f"win{c['win']}")
def test_kaldi_statement_through_the_mel_stage_is_the_oracle(c):
    """kaldi_raw_frames against oracle/dsp_ref.py get_strided_kaldi (exact: both only select samples), and kaldi_stmt -> |rfft|^2 -> Kaldi mel bank
    -> ln(max(., 1e-8)) against compute_fbank_kaldi (float32 frames there: 2e-5 on the log-mel).  Every case's pad and frame count are Kaldi's own
    for its (win, shift, L), so the oracle accepts all four; it pads each frame to the next power of two, and so does the statement here."""
    win, shift, pad, nfr, L = c["win"], c["shift"], c["pad"], c["n_frames"], c["L"]
    snip = pad == 0
    assert pad == (0 if snip else win // 2 - shift // 2) and nfr == (1 + (L - win) // shift if snip else (L + shift // 2) // shift)
    P = 2 ** (win - 1).bit_length()
    x = S.ramp_noise(1, L, win)[0] * 100.0
    w, noise = S.hamming(win), S.unit_noise((nfr, win), 5)
    raw = dsp_ref.get_strided_kaldi(x.numpy(), win, shift, snip)
    assert raw.shape == (nfr, win) and np.array_equal(raw.astype(np.float64), S.kaldi_raw_frames(x, win, shift, pad, nfr, F64).numpy())
    sr = 16000
    assert int(sr * (shift / sr * 1000) * 0.001) == shift and int(sr * (win / sr * 1000) * 0.001) == win   # the oracle's own unit round trip
    for pre, dither in ((0.97, 1.0), (0.0, 0.0)):
        want = dsp_ref.compute_fbank_kaldi(x.numpy(), sample_rate=sr, win_len=win, win_inc=shift, num_mels=23, win_type="hamming", preemphasis=pre,
                                           dither=dither, snip_edges=snip, noise=noise.numpy())
        fr = S.kaldi_stmt(x, win, shift, pad, P, nfr, w, pre, noise if dither else None, dither, F64)
        bins, _ = dsp_ref.get_mel_banks_kaldi(23, P, float(sr), 20.0, 0.0)
        bins = np.pad(bins, [(0, 0), (0, 1)]).astype(np.float64)
        mel = np.log(np.maximum((np.abs(np.fft.rfft(fr.numpy(), axis=1)) ** 2) @ bins.T, 1e-8))
        assert want.shape == mel.shape and np.abs(mel - want).max() <= 2e-5
    # zero padding to the case's own n_fft, and the first sample keeps no pre-emphasis
    fr = S.kaldi_stmt(x, win, shift, pad, c["n_fft"], nfr, torch.ones(win), 0.97, None, 0.0, F64)
    r = raw.astype(np.float64)
    r = r - r.mean(axis=1, keepdims=True)
    assert fr.shape == (nfr, c["n_fft"]) and torch.equal(fr[:, win:], torch.zeros(nfr, c["n_fft"] - win, dtype=F64))
    assert np.abs(fr[:, 0].numpy() - r[:, 0]).max() <= 1e-12 * np.abs(r).max()
    assert np.abs(fr[:, 1:win].numpy() - (r[:, 1:] - float(np.float32(0.97)) * r[:, :-1])).max() <= 1e-12 * np.abs(r).max()


def test_heads_statements_are_the_kokoro_oracle():
    """magphase_stmt and head_stmt against oracle/kokoro_ref.py at the even sizes it takes (its irfft has no length argument): magnitude and audio to
    a few float32 roundings (the oracle returns float32), phase modulo 2 pi at bins above 1e-4."""
    from oracle import kokoro_ref

    for n_fft, hop in [(20, 5), (16, 4), (64, 16)]:
        nb = n_fft // 2 + 1
        x = S.magphase_input(2, 40 * hop + 3, n_fft)
        w = S.hann_periodic(n_fft)
        got = S.magphase_stmt(x, w, n_fft, hop, F64)
        want = torch.from_numpy(kokoro_ref.stft_mag_phase(x.numpy(), n_fft, hop).transpose(0, 2, 1)).double()
        assert want.shape == got.shape
        assert float((got[..., :nb] - want[..., :nb]).abs().max()) <= 3e-7 * float(got[..., :nb].max())
        d = (got[..., nb:] - want[..., nb:]).abs()
        d = torch.minimum(d, 2 * math.pi - d)
        assert float(d[got[..., :nb] >= 1e-4].max()) <= 1e-5
        xh = S.head_input(2, 37, nb, n_fft)
        a = S.head_stmt(xh, w, n_fft, hop, F64)
        wa = kokoro_ref.istft_head(xh.transpose(1, 2), n_fft, hop)[:, 0].double()
        assert wa.shape == a.shape and float((a - wa).abs().max()) <= 1e-6 * max(1.0, float(a.abs().max()))


def test_polar_statement():
    x = S.polar_input(2, 3, 7, 1)
    got = S.polar_stmt(x, 7, S.POLAR_CLIP, F64)
    z = np.minimum(np.exp(x[..., :7].numpy().astype(np.float64)), 100.0) * np.exp(1j * x[..., 7:].numpy().astype(np.float64))
    assert rel(torch.view_as_complex(got.contiguous()), torch.from_numpy(z)) <= 1e-12


# ----------------------------------------------------------------------------------------------------------------- the Stockham plan
def test_plans_are_what_the_cases_claim():
    """make_plan restated: every table size gets the radix list its case names; the table reaches every radix the issue lists; 134 = 2 x 67 and
    536 = 4 x 2 x 67 are refused; the restated schedule is a DFT at every table size that is cheap to walk in Python."""
    seen = set()
    for c in S.STOCKHAM_CASES:
        assert S.make_plan(c["n_fft"]) == c["rad"], c
        assert math.prod(c["rad"]) == c["n_fft"]
        seen |= set(c["rad"])
    assert seen >= S.PLAN_RADICES, S.PLAN_RADICES - seen
    for n in S.STOCKHAM_REFUSED:
        assert S.make_plan(n) is None
    assert S.make_plan(61 * 4) == [4, 61] and S.make_plan(67) is None
    rng = np.random.default_rng(0)
    for n in sorted({c["n_fft"] for c in S.STOCKHAM_CASES if c["n_fft"] <= 250} | {n for n, _, _ in S.ISTFT_CASES if n <= 250}):
        v = rng.standard_normal(n) + 1j * rng.standard_normal(n)
        assert np.abs(S.fft_lds_numpy(v, S.make_plan(n)) - np.fft.fft(v)).max() <= 1e-12 * n
        assert np.abs(S.fft_lds_numpy(v, S.make_plan(n), inverse=True) - np.fft.ifft(v) * n).max() <= 1e-12 * n


def test_stockham_launch_arithmetic():
    """pairs = 1 at 2048 and 4096; dynamic LDS above 64 KB (the hipFuncSetAttribute branch) at 4096 only; above 160 KB (refused) at 16384; every
    mi355_istft size of the table is even and has a plan."""
    by_n = {c["n_fft"]: S.stockham_lds(c["n_fft"]) for c in S.STOCKHAM_CASES}
    assert by_n[2048][1] == 1 and by_n[4096][1] == 1 and by_n[960][1] > 1
    assert by_n[4096][0] == 96 * 1024 and all(lds <= 64 * 1024 for n, (lds, _) in by_n.items() if n != 4096)
    assert S.stockham_lds(16384)[0] > 160 * 1024 and S.make_plan(16384) is not None
    for n, hop, nfr in S.ISTFT_CASES:
        assert n % 2 == 0 and S.make_plan(n) is not None and S.stockham_lds(n)[0] <= 64 * 1024
    for c in S.LOGMEL_GENERIC:
        assert S.stockham_lds(c["n_fft"], mel=True)[0] <= 64 * 1024
    assert [c["n_fft"] // 2 + 1 for c in S.LOGMEL_GENERIC] == [49, 126]   # one and two trips of the 64-lane dot product, each with a tail


# ----------------------------------------------------------------------------------------------------------------- preconditions
@pytest.mark.parametrize("c", S.STOCKHAM_CASES, ids=S.stockham_id)
def test_every_stored_frame_stays_inside_the_signal(c):
    lo, hi = S.reflect_index_range(c["n_fft"], c["hop"], c["L"], c["pad"], S.stockham_frames(c))
    assert 0 <= lo and hi < c["L"], (lo, hi)
    if c["pad"] == 1:
        assert c["L"] > c["n_fft"] // 2
    assert S.stockham_frames(c) >= 1 and S.stockham_frames(c) <= S.n_frames_of(c["L"], c["n_fft"], c["hop"], c["pad"])


@pytest.mark.parametrize("g", S.derived_forward_geometries(), ids=lambda g: "-".join(map(str, g)))
def test_derived_forward_cases_stay_inside_the_signal(g):
    """The same for the log-mel and fast-kernel cases whose shapes do not depend on the device; the short launches have the frame counts they name."""
    n_fft, hop, L, pad, nfr = g
    lo, hi = S.reflect_index_range(n_fft, hop, L, pad, nfr)
    assert 0 <= lo and hi < L and 1 <= nfr <= S.n_frames_of(L, n_fft, hop, pad) and (pad != 1 or L > n_fft // 2)


def test_short_launches_have_the_named_frame_counts():
    for n in S.FAST_SPLIT:
        T = 2 * S.fast_geom_of(n).PW
        got = [S.short_launch_case(n, w) for w in S.SHORT_LAUNCHES]
        assert [nfr for _, _, nfr, _ in got] == [1, T - 1, T, T + 1] and got[0][3] == 1
        assert all(S.n_frames_of(L, n, hop, 2) == nfr for hop, L, nfr, _ in got)


def test_stockham_table_has_the_named_shapes():
    t = S.STOCKHAM_CASES
    assert any(S.stockham_frames(c) == 1 for c in t)
    assert any(c["pad"] == 1 and c["L"] == c["n_fft"] // 2 + 1 for c in t)
    assert any(c.get("ld", c["L"]) != c["L"] for c in t)
    assert any(c["n_fft"] == 960 and S.stockham_frames(c) == 11 for c in t) and any(c["n_fft"] == 960 and S.stockham_frames(c) == 10 for c in t)
    assert any(S.stockham_frames(c) % 2 == 1 for c in t) and any(c["n_fft"] % 2 == 1 for c in t)


@pytest.mark.parametrize("c", S.KALDI_CASES, ids=lambda c: f"win{c['win']}")
def test_kaldi_cases_are_admissible(c):
    need = (c["n_frames"] - 1) * c["shift"] + c["win"] - c["pad"]
    assert need <= c["L"] + c["pad"] and c["pad"] < c["L"] and c["n_fft"] >= c["win"]
    assert (need == c["L"] + c["pad"]) == c["limit"]
    if c["limit"]:
        assert need + c["shift"] > c["L"] + c["pad"]   # one more frame is refused


def test_kaldi_table_has_the_named_windows():
    wins = [c["win"] for c in S.KALDI_CASES]
    assert any(w < 64 for w in wins) and any(w > 256 for w in wins) and any(w & (w - 1) and w < c["n_fft"] for w, c in zip(wins, S.KALDI_CASES))
    assert sum(c["limit"] for c in S.KALDI_CASES) == 2


def test_polar_inputs_straddle_the_clip():
    """Between 10 % and 90 % of the log-magnitudes lie above ln(clip) in every case with more than one value, and over the whole table (the
    (1, 1, 1, 2) case has a single magnitude)."""
    above = total = 0
    for i, (B, Fr, nb, ldx, bs) in enumerate(S.POLAR_CASES):
        m = S.polar_input(B, Fr, nb, i)[..., :nb]
        share = float((m > math.log(S.POLAR_CLIP)).double().mean())
        above, total = above + int((m > math.log(S.POLAR_CLIP)).sum()), total + m.numel()
        assert ldx >= 2 * nb and (bs == 0 or bs > Fr * ldx)
        if m.numel() > 1:
            assert 0.1 <= share <= 0.9, share
    assert 0.1 <= above / total <= 0.9


@pytest.mark.parametrize("n_fft,hop,nfr", S.ISTFT_CASES)
def test_istft_clamp_case_clips_a_known_share(n_fft, hop, nfr):
    """The clamp launches of the GPU file (test_istft_edges and the ISTFTCache wrapper case) take their spectrum, window and gain from
    istft_inputs / ISTFT_CLAMP_GAIN: between 5 % and 50 % of the irfft samples exceed that window."""
    share = S.istft_clamp_share(n_fft, hop, nfr)
    assert 0.05 <= share <= 0.5, share


def test_istft_table_has_the_named_geometries():
    t = S.ISTFT_CASES
    assert {n for n, _, _ in t} == {2, 20, 96, 122, 960, 1024} and {f for _, _, f in t} == {1, 2, 7, 8}
    for n in (20, 96, 122, 960, 1024):
        assert any(a == n and h == n // 4 for a, h, _ in t)
    assert any(h == n for n, h, _ in t) and any(h == n + 3 for n, h, _ in t) and (20, 1, 8) in t


# ----------------------------------------------------------------------------------------------------------------- filterbanks, fast geometry
def test_cap_banks_sit_on_either_side_of_the_lds_capacity():
    a, b = S.cap_banks()
    assert S.span_total(a) == S.K_FB_CAP == 1536 and S.span_total(b) == 1537
    assert torch.equal(a[:-1], b[:-1]) and a.shape == b.shape and a.shape[1] == 257
    lo, n = S.spans(a)[3]
    assert int((a[3, lo:lo + n] == 0).sum()) > 10 and a[3, lo] != 0 and a[3, lo + n - 1] != 0   # zeros INSIDE the span
    g = S.fast_geom_of(512)
    assert g.mel_fits(a.shape[0])
    dense = torch.ones(S.K_MAX_MELS, 257)
    assert S.span_total(dense) > S.K_FB_CAP


def test_slaney_banks_have_empty_rows():
    counts = {}
    for sr, n_fft, n_mels in S.SLANEY_EMPTY_ROW_BANKS:
        fb = S.slaney_bank(sr, n_fft, n_mels)
        counts[(sr, n_fft, n_mels)] = sum(1 for _, n in S.spans(fb) if n == 0)
        assert counts[(sr, n_fft, n_mels)] >= 1 and S.fast_geom_of(n_fft).mel_fits(n_mels) and S.span_total(fb) <= S.K_FB_CAP
    assert counts == {(16000, 400, 160): 4, (16000, 400, 234): 34, (16000, 512, 256): 24}


def test_fast_geometry_boundaries():
    """FastGeom<20, 20>: 4824 B of power rows + 5640 B of staged output = zbytes = 10464 B at 235 mels, nothing to spare; 236 does not fit.
    256 (kMaxMels) fits at 512 and 1024."""
    g = S.fast_geom(20, 20)
    assert (g.PW, g.PITCH, g.NBP, g.zbytes, g.pw_floats * 4) == (3, 436, 201, 10464, 4824)
    assert g.mel_bytes(235) == 4824 + 5640 == g.zbytes and g.mel_fits(235) and not g.mel_fits(236)
    assert not g.mel_fits(237) and g.mel_fits(234)   # 236 | 1 == 237: the odd pitch is what overflows
    for n in (512, 1024):
        gg = S.fast_geom_of(n)
        assert gg.PW == 2 and gg.mel_fits(256) and gg.mel_fits(257)   # 257 is refused by kMaxMels, not by the slice
    assert S.K_MAX_MELS == 256


@pytest.mark.parametrize("n_fft", [400, 512, 1024])
def test_load_path_cases_have_interior_tiles(n_fft):
    """Every load-path identity case of the GPU file has at least two interior tiles per item, one edge tile at either end (reflect padding), and
    the prefetch case with alternating tiles has an interior tile between two edge tiles."""
    for hop in (S.FAST_HOPS[n_fft], S.FAST_ODD_HOPS[n_fft]):
        for L in S.load_path_lengths(n_fft, hop):
            k = S.tile_kinds(n_fft, hop, L, 1, S.n_frames_of(L, n_fft, hop, 1))
            assert sum(k) >= 2 and not k[0] and not k[-1], (hop, L, k)
    assert S.FAST_ODD_HOPS[n_fft] % 4 != 0 and S.FAST_HOPS[n_fft] % 4 == 0
    hop, L = S.alternating_case(n_fft)
    assert L % 4 == 0 and hop % 4 == 0
    assert S.tile_kinds(n_fft, hop, L, 1, S.n_frames_of(L, n_fft, hop, 1)) == [False, True, False]


# ----------------------------------------------------------------------------------------------------------------- the heads' inputs
@pytest.mark.parametrize("n_fft,hop", S.HEAD_GENERIC + [(20, 5)])
def test_phase_is_compared_on_all_but_one_percent_of_the_bins(n_fft, hop):
    """For every stft_magphase case the float64 reference has at most 1 % of its bins below 1e-4 (where the phase is not compared); the ragged
    lengths respect lens[b] > n_fft / 2 with the shortest at n_fft / 2 + 1; an odd n_fft never meets a length that hop divides."""
    w = S.hann_periodic(n_fft)
    nb = n_fft // 2 + 1
    if (n_fft, hop) == (20, 5):
        inputs = [(S.magphase_input(2, L, L), None) for L in S.MAGPHASE_FAST_LENGTHS] + [(S.magphase_input(3, 700, 9), [700, 11, 403])]
        assert [S.magphase_frames(L, 5) for L in S.MAGPHASE_FAST_LENGTHS] == [3, 255, 256, 257, 600]
    else:
        L, lens = S.magphase_generic_case(n_fft, hop)
        inputs = [(S.magphase_input(3, L, n_fft * hop), None), (S.magphase_input(3, L, n_fft * hop), lens)]
        assert min(lens) == n_fft // 2 + 1 and max(lens) == L
    for x, lens in inputs:
        for n in ([x.shape[1]] if lens is None else lens):
            assert n > n_fft // 2 and (n_fft % 2 == 0 or n % hop != 0)
        y = S.magphase_stmt(x, w, n_fft, hop, F64, lens=lens)
        mag = y[..., :nb]
        live = mag != S.SENTINEL
        assert float((mag[live] < 1e-4).double().mean()) <= 0.01
