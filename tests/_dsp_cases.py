"""TEST INFRASTRUCTURE shared by tests/test_dsp_kernel_edges_gpu.py and tests/test_dsp_refs_cpu.py: the reference statements of the transform kernels
(csrc/fft.hip, csrc/fft_fast.h and the two small-FFT heads of csrc/source.hip), each written from the formulas of include/mi355audio.h and of
oracle/dsp_ref.py and evaluated in whatever dtype the caller asks for (float64: the reference; float32 with torch.fft on the CPU: its own rounding
error, ``e32``); the case tables; the synthetic filterbanks; and the launch arithmetic of the host code restated in Python (``make_plan``,
``choose_pairs``, ``fast_geom``), so that the boundary cases are derived and not typed in.  The CPU file holds all of this to known-good
implementations and asserts the preconditions of every case.  CPU only: nothing here touches ``mlx_audio_amd.ops``."""
import math

import numpy as np
import torch

SENTINEL = -777.25   # exactly representable; no kernel here produces it
CDT = {torch.float64: torch.complex128, torch.float32: torch.complex64}


# ----------------------------------------------------------------------------------------------------------------- inputs
def ramp_noise(B, L, seed):
    """Seeded unit noise with a gain ramp 0.2 ... 3.0 over the signal (tests/test_kernels_gpu.py's fast-kernel input), float32 [B, L]."""
    rng = np.random.default_rng(seed)
    return torch.from_numpy((rng.standard_normal((B, L)) * np.linspace(0.2, 3.0, L)[None]).astype(np.float32))


def unit_noise(shape, seed):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal(shape).astype(np.float32))


def hamming(n):
    """Symmetric Hamming window, float32 [n]: no zero at either end, so n = 2 and n = 3 are not the zero transform (a symmetric Hann is)."""
    k = np.arange(n, dtype=np.float64)
    return torch.from_numpy((0.54 - 0.46 * np.cos(2.0 * np.pi * k / max(n - 1, 1))).astype(np.float32))


def hann_periodic(n):
    """hanning(n + 1)[:-1]: the synthesis window of dsp.istft and of the Kokoro heads."""
    k = np.arange(n, dtype=np.float64)
    return torch.from_numpy((0.5 * (1.0 - np.cos(2.0 * np.pi * k / n))).astype(np.float32))


# ----------------------------------------------------------------------------------------------------------------- statements: forward
PAD_NONE, PAD_REFLECT, PAD_CONSTANT = 0, 1, 2


def n_frames_of(L, n_fft, hop, pad_mode):
    """dsp.stft's frame count: 1 + (padded length - n_fft) // hop with n_fft // 2 samples of padding on either side when centred."""
    return 1 + (L + (2 * (n_fft // 2) if pad_mode else 0) - n_fft) // hop


def padded_signal(x, n_fft, pad_mode, dtype):
    """dsp.stft's centre padding (oracle/dsp_ref.py: stft): reflect = x[1 : p + 1] reversed | x | x[-(p + 1) : -1] reversed, constant = zeros."""
    x = x.to(dtype)
    p = n_fft // 2
    if pad_mode == PAD_NONE:
        return x
    if pad_mode == PAD_CONSTANT:
        z = torch.zeros(x.shape[0], p, dtype=dtype)
        return torch.cat([z, x, z], dim=1)
    assert pad_mode == PAD_REFLECT and x.shape[1] > p
    return torch.cat([x[:, 1:p + 1].flip(1), x, x[:, x.shape[1] - (p + 1):x.shape[1] - 1].flip(1)], dim=1)


def frames_stmt(x, n_fft, hop, pad_mode, n_frames, dtype):
    """[B, L] -> [B, n_frames, n_fft]: frame f is padded[f * hop : f * hop + n_fft]."""
    xp = padded_signal(x, n_fft, pad_mode, dtype)
    fr = xp.unfold(1, n_fft, hop)
    assert fr.shape[1] >= n_frames, (fr.shape, n_frames)
    return fr[:, :n_frames]


def stft_stmt(x, window, n_fft, hop, pad_mode, n_frames, dtype):
    """dsp.stft: rfft(frames * window) -> complex [B, n_frames, n_fft // 2 + 1] (Hermitian half, bin k at index k)."""
    return torch.fft.rfft(frames_stmt(x, n_fft, hop, pad_mode, n_frames, dtype) * window.to(dtype), dim=-1)


def logmel_stmt(x, window, n_fft, hop, pad_mode, n_frames, fb, mode, dtype, log_guard=0.0):
    """mi355_logmel before the Whisper finish, the five modes of the header: 0 log10(max(mel(|X|^2), 1e-10)); 1 ln(max(mel(sqrt(|X|^2 + 1e-9)), 1e-5));
    2 ln(max(mel(|X|^2), 1e-8)); 3 ln(max(mel(|X|), 1e-5)); 4 ln(mel(|X|^2) + guard).  mel(p) = p @ fb^T."""
    X = stft_stmt(x, window, n_fft, hop, pad_mode, n_frames, dtype)
    p = X.real * X.real + X.imag * X.imag
    if mode == 1:
        p = torch.sqrt(p + 1e-9)
    elif mode == 3:
        p = torch.sqrt(p)
    mel = p @ fb.to(dtype).transpose(0, 1)
    if mode == 0:
        return torch.log10(mel.clamp(min=1e-10))
    if mode in (1, 3):
        return torch.log(mel.clamp(min=1e-5))
    if mode == 2:
        return torch.log(mel.clamp(min=1e-8))
    assert mode == 4 and log_guard > 0
    return torch.log(mel + log_guard)


def whisper_finish_stmt(y, fixed_max=None):
    """whisper/audio.py: max(y, max - 8) with the maximum of each ITEM (or a fixed one: Voxtral Realtime), then (y + 4) / 4."""
    m = y.amax(dim=(1, 2), keepdim=True) if fixed_max is None else torch.full((y.shape[0], 1, 1), fixed_max, dtype=y.dtype)
    return (torch.maximum(y, m - 8.0) + 4.0) / 4.0


# ----------------------------------------------------------------------------------------------------------------- statements: inverse
def ola_envelope(window, n_frames, hop, squared, floor=None):
    """The normaliser the caller hands mi355_istft: the window (or its square) overlap-added in frame order with float32 accumulation, as
    dsp.istft's scatter-add and ISTFTCache.get_norm_buffer (which also floors it at 1e-10) produce it.  float32 [ola]: it is INPUT DATA."""
    w = window.numpy().astype(np.float32)
    wn = (w * w).astype(np.float32) if squared else w
    env = np.zeros((n_frames - 1) * hop + w.shape[0], np.float32)
    for f in range(n_frames):
        env[f * hop:f * hop + w.shape[0]] += wn
    if floor is not None:
        env = np.maximum(env, np.float32(floor))
    return torch.from_numpy(env)


def overlap_add(frames, hop):
    B, nf, N = frames.shape
    out = torch.zeros(B, (nf - 1) * hop + N, dtype=frames.dtype)
    for f in range(nf):
        out[:, f * hop:f * hop + N] += frames[:, f]
    return out


def istft_stmt(spec, window, n_fft, hop, norm, norm_mode, clamp, trim, out_len, dtype):
    """mi355_istft: frames = irfft(spec, n_fft) (the imaginary parts of bin 0 and of the Nyquist bin are ignored), clamped to +-window when asked
    (constrain_value_range), times the window, overlap-added, divided by ``norm`` (norm_mode 0: always; 1: only where norm > 1e-10),
    out = ola[trim : trim + out_len].  spec complex [B, n_frames, n_fft // 2 + 1]."""
    s = spec.to(CDT[dtype]).clone()
    s.imag[..., 0] = 0
    if n_fft % 2 == 0:
        s.imag[..., -1] = 0
    w = window.to(dtype)
    fr = torch.fft.irfft(s, n=n_fft, dim=-1)
    if clamp:
        fr = torch.minimum(torch.maximum(fr, -w), w)
    ola = overlap_add(fr * w, hop)
    nv = norm.to(dtype)[None, :]
    o = ola / nv if norm_mode == 0 else torch.where(nv > 1e-10, ola / torch.where(nv > 1e-10, nv, torch.ones_like(nv)), ola)
    assert trim + out_len <= o.shape[1]
    return o[:, trim:trim + out_len]


# ----------------------------------------------------------------------------------------------------------------- statements: small-FFT heads
def magphase_frames(L, hop):
    return L // hop + 1


def magphase_stmt(x, window, n_fft, hop, dtype, lens=None):
    """mi355_stft_magphase: the reflect-centred STFT of each item's first lens[b] samples; y[b, f, :nb] = |X|, y[b, f, nb:] = atan2(Im X, Re X) with
    Im X = 0 at bin 0 and at the Nyquist bin; rows f in [0, lens[b] // hop]; rows past that hold SENTINEL.  (For odd n_fft the padded signal has
    1 + (len - 1) // hop frames: one fewer than the kernel's count when hop divides len; the cases avoid that.)"""
    B, L = x.shape
    nb = n_fft // 2 + 1
    rows = magphase_frames(L, hop)
    y = torch.full((B, rows, 2 * nb), SENTINEL, dtype=dtype)
    for b in range(B):
        n = L if lens is None else int(lens[b])
        nf = magphase_frames(n, hop)
        X = stft_stmt(x[b:b + 1, :n], window, n_fft, hop, PAD_REFLECT, nf, dtype)[0]
        im = X.imag.clone()
        im[:, 0] = 0
        if n_fft % 2 == 0:
            im[:, -1] = 0
        y[b, :nf, :nb] = torch.sqrt(X.real * X.real + im * im)
        y[b, :nf, nb:] = torch.atan2(im, X.real)
    return y


def head_stmt(x, window, n_fft, hop, dtype, lens=None):
    """mi355_istft_head: mag = exp(x[..., :nb]), phase = sin(x[..., nb:]), spec = mag * (cos phase + i sin phase), irfft(n_fft), times the window,
    overlap-add normalised by the overlap-added squared window where that exceeds 1e-10, n_fft // 2 trimmed off either end:
    audio [B, (Fr - 1) * hop]; an item with lens[b] frames fills its first (lens[b] - 1) * hop samples, the rest holds SENTINEL."""
    B, Fr, _ = x.shape
    nb = n_fft // 2 + 1
    w = window.to(dtype)
    audio = torch.full((B, (Fr - 1) * hop), SENTINEL, dtype=dtype)
    for b in range(B):
        nf = Fr if lens is None else int(lens[b])
        xb = x[b, :nf].to(dtype)
        mag, ph = torch.exp(xb[:, :nb]), torch.sin(xb[:, nb:2 * nb])
        fr = torch.fft.irfft(torch.complex(mag * torch.cos(ph), mag * torch.sin(ph)), n=n_fft, dim=-1) * w
        rec = overlap_add(fr[None], hop)[0]
        env = overlap_add((w * w)[None, None].expand(1, nf, n_fft).contiguous(), hop)[0]
        o = torch.where(env > 1e-10, rec / torch.where(env > 1e-10, env, torch.ones_like(env)), rec)
        audio[b, :(nf - 1) * hop] = o[n_fft // 2:n_fft // 2 + (nf - 1) * hop]
    return audio


# ----------------------------------------------------------------------------------------------------------------- statements: kaldi, polar
def kaldi_raw_frames(x, win, shift, pad, n_frames, dtype):
    """get_strided_kaldi: x[1 : pad + 1] reversed | x | x[L - 1], x[L - 2], ... (pad of them), frame f = padded[f * shift : f * shift + win]."""
    x = x.to(dtype)
    xp = torch.cat([x[1:pad + 1].flip(0), x, x.flip(0)[:pad]]) if pad > 0 else x
    assert (n_frames - 1) * shift + win <= xp.shape[0]
    return xp.unfold(0, win, shift)[:n_frames]


def kaldi_stmt(x, win, shift, pad, n_fft, n_frames, window, preemph, noise, dither, dtype):
    """mi355_kaldi_frames (oracle/dsp_ref.py: get_strided_kaldi + compute_fbank_kaldi up to the window): the signal with ``pad`` reflected samples
    at either end (x[1 : pad + 1] reversed | x | x[L - 1], x[L - 2], ...), frame f = padded[f * shift : f * shift + win], + dither * noise, minus the
    frame mean, pre-emphasis inside the frame (the first sample kept), times the window, zero-padded to n_fft.  x [L] -> [n_frames, n_fft]."""
    fr = kaldi_raw_frames(x, win, shift, pad, n_frames, dtype)
    if noise is not None:
        fr = fr + noise.to(dtype) * torch.tensor(dither, dtype=torch.float32).to(dtype)
    fr = fr - fr.mean(dim=1, keepdim=True)
    if preemph != 0.0:
        pe = torch.tensor(preemph, dtype=torch.float32).to(dtype)   # the kernel receives a float
        fr = torch.cat([fr[:, :1], fr[:, 1:] - pe * fr[:, :-1]], dim=1)
    fr = fr * window.to(dtype)
    return torch.cat([fr, torch.zeros(n_frames, n_fft - win, dtype=dtype)], dim=1)


def polar_stmt(x, nb, clip, dtype):
    """mi355_polar_spec (Vocos ISTFTHead): min(exp(m), clip) * (cos p, sin p) with m = x[..., :nb], p = x[..., nb : 2 nb] -> [B, Fr, nb, 2]."""
    m = torch.exp(x[..., :nb].to(dtype)).clamp(max=clip)
    p = x[..., nb:2 * nb].to(dtype)
    return torch.stack([m * torch.cos(p), m * torch.sin(p)], dim=-1)


# ----------------------------------------------------------------------------------------------------------------- host arithmetic restated
def make_plan(N):
    """csrc/fft.hip make_plan: radices 4, 2, 3, 5 while they divide, then the odd factors from 7 upwards; None when a factor exceeds 61 (or more
    than 24 stages)."""
    rad, n = [], N
    for r in (4, 2, 3, 5):
        while n % r == 0:
            rad.append(r)
            n //= r
    q = 7
    while n > 1:
        while n % q == 0:
            if q > 61:
                return None
            rad.append(q)
            n //= q
        q += 2
    return rad if len(rad) <= 24 else None


def fft_lds_numpy(v, rad, inverse=False):
    """The Stockham schedule of csrc/fft.hip fft_lds, index by index, in complex128: what the device code computes if its indexing is right."""
    N = v.shape[0]
    tw = np.exp((2j if inverse else -2j) * np.pi * np.arange(N) / N)
    src, Ns = v.astype(np.complex128), 1
    for R in rad:
        NR, stride = N // R, N // (Ns * R)
        dst = np.zeros(N, np.complex128)
        for j in range(NR):
            k = j % Ns
            t = np.arange(R)
            vv = src[j + t * NR] * tw[(k * stride * t) % N]
            base = (j // Ns) * Ns * R + k
            for q in range(R):
                dst[base + q * Ns] = np.sum(vv * tw[(NR * t * q) % N])
        src, Ns = dst, Ns * R
    return src


def choose_pairs(N, extra_per_frame_bytes=0):
    pairs = 8
    while pairs > 1 and N * 8 + pairs * (2 * N * 8 + 2 * extra_per_frame_bytes) > 60 * 1024:
        pairs >>= 1
    return pairs


def stockham_lds(N, mel=False):
    """Dynamic LDS of stft_kernel / istft_frames_kernel: twiddles + two buffers of ``pairs`` transforms (+ the power rows of the mel kernel)."""
    nb = N // 2 + 1
    pairs = choose_pairs(N, nb * 4 if mel else 0)
    return N * 8 * (1 + 2 * pairs) + (2 * pairs * nb * 4 if mel else 0), pairs


K_FB_CAP, K_MAX_MELS = 1536, 256
FAST_SPLIT = {400: (20, 20), 512: (16, 32), 1024: (32, 32)}


class FastGeom:
    """csrc/fft_fast.h FastGeom<N1, N2>."""

    def __init__(self, N1, N2):
        self.N1, self.N2 = N1, N2
        self.N, self.NB = N1 * N2, N1 * N2 // 2 + 1
        self.PR = N2 + 1
        self.BASE = N1 * self.PR
        self.PITCH = self.BASE + ((N2 % 32) - (self.BASE % 32) + 32) % 32 if N2 < 32 else self.BASE
        self.PW = 64 // max(N1, N2)
        self.NBP = self.NB | 1
        self.zbytes = self.PW * self.PITCH * 8
        self.pw_floats = 2 * self.PW * self.NBP

    def mel_bytes(self, n_mels):
        """Power rows + staged output, the bytes a wave's slice must hold in MODE 1."""
        return self.pw_floats * 4 + 2 * self.PW * (n_mels | 1) * 4

    def mel_fits(self, n_mels):
        return self.mel_bytes(n_mels) <= self.zbytes

    def lds_bytes(self, mel, waves):
        return self.N * 8 + self.N * 4 + ((K_FB_CAP * 4 + K_MAX_MELS * 12 + 16) if mel else 0) + waves * self.zbytes

    def resident_tiles(self, mel, prefetch, cus):
        """Tiles in flight in one launch (launch_fast_cfg): waves x workgroups resident; a wave gets a second tile only beyond this."""
        waves = 4 if prefetch else 6
        by_lds = max(1, (160 * 1024) // self.lds_bytes(mel, waves))
        by_regs = max(1, ((2 if prefetch else 3) * 4) // waves)
        return waves * cus * min(by_lds, by_regs)


def fast_geom(N1, N2):
    return FastGeom(N1, N2)


def fast_geom_of(n_fft):
    return FastGeom(*FAST_SPLIT[n_fft])


def tile_kinds(n_fft, hop, L, pad_mode, n_frames):
    """Per tile of one item: True where stft_fast_kernel's ``inner`` holds (every sample of the tile's 2 PW frames lies inside the signal)."""
    g = fast_geom_of(n_fft)
    off = n_fft // 2 if pad_mode else 0
    T = 2 * g.PW
    kinds = []
    for f0 in range(0, n_frames, T):
        kinds.append(f0 * hop - off >= 0 and (f0 + T - 1) * hop - off + n_fft <= L and f0 + T <= n_frames)
    return kinds


def reflect_index_range(n_fft, hop, L, pad_mode, n_frames):
    """(min, max) over every stored frame of the kernels' padded index f * hop + n - off after ONE reflection (reflect) or as it is (none); for
    constant padding the range of the indices that are read (those inside the signal)."""
    off = n_fft // 2 if pad_mode else 0
    idx = (np.arange(n_frames)[:, None] * hop + np.arange(n_fft)[None, :] - off).astype(np.int64)
    if pad_mode == PAD_REFLECT:
        idx = np.where(idx < 0, -idx, idx)
        idx = np.where(idx >= L, 2 * (L - 1) - idx, idx)
    elif pad_mode == PAD_CONSTANT:
        idx = idx[(idx >= 0) & (idx < L)]
    return int(idx.min()), int(idx.max())


# ----------------------------------------------------------------------------------------------------------------- filterbanks
def slaney_bank(sr, n_fft, n_mels):
    from oracle import dsp_ref

    return torch.from_numpy(np.ascontiguousarray(dsp_ref.mel_filters(sr, n_fft, n_mels, norm="slaney", mel_scale="slaney")))


SLANEY_EMPTY_ROW_BANKS = [(16000, 400, 160), (16000, 400, 234), (16000, 512, 256)]


def spans(fb):
    """(lo, len) per row as the fast kernel finds them: first to last non-zero column."""
    out = []
    for row in fb.numpy():
        nz = np.nonzero(row)[0]
        out.append((int(nz[0]), int(nz[-1] - nz[0] + 1)) if nz.size else (0, 0))
    return out


def span_total(fb):
    return sum(n for _, n in spans(fb))


def cap_banks(n_fft=512, rows=8, seed=5):
    """Two banks [rows, n_fft / 2 + 1] whose span totals are exactly kFbCap (the compacted rows sit in LDS) and kFbCap + 1 (they are read from
    L2): ``rows`` spans of kFbCap / rows columns at staggered offsets; the second bank has one more non-zero column at the end of its last row.
    Row 3 has zeros INSIDE its span (every third column), which the span covers.  Rows 0 .. rows - 2 are shared."""
    nb = n_fft // 2 + 1
    width = K_FB_CAP // rows
    assert width * rows == K_FB_CAP and width + 1 + (rows - 1) * 8 <= nb
    rng = np.random.default_rng(seed)
    a = np.zeros((rows, nb), np.float32)
    for m in range(rows):
        a[m, m * 8:m * 8 + width] = (rng.random(width) * 1e-2 + 1e-4).astype(np.float32)
    a[3, 3 * 8 + 1:3 * 8 + width - 1:3] = 0.0
    b = a.copy()
    b[rows - 1, (rows - 1) * 8 + width] = np.float32(3e-3)
    return torch.from_numpy(a), torch.from_numpy(b)


def random_sparse_bank(n_mels, nb, seed, zero_rows=()):
    """Triangles of random width and height; the rows in ``zero_rows`` are all zero."""
    rng = np.random.default_rng(seed)
    fb = np.zeros((n_mels, nb), np.float32)
    for m in range(n_mels):
        if m in zero_rows:
            continue
        c = (m + 0.5) * nb / n_mels
        half = max(1.5, 1.5 * nb / n_mels)
        k = np.arange(nb)
        fb[m] = np.maximum(0.0, 1.0 - np.abs(k - c) / half) * (0.5 + rng.random()) * 2e-2
    return torch.from_numpy(fb)


# ----------------------------------------------------------------------------------------------------------------- case tables
# A. generic Stockham forward (MI355_FFT_FAST=0): n_fft, hop, L, pad_mode, B, the radix list make_plan must give, what the case reaches
STOCKHAM_CASES = [
    dict(n_fft=2, hop=1, L=9, pad=1, B=2, rad=[2], why="single radix-2 stage, 2k == N at k = 1"),
    dict(n_fft=3, hop=1, L=11, pad=1, B=2, rad=[3], why="smallest odd size, generic radix R = 3"),
    dict(n_fft=15, hop=4, L=101, pad=1, B=2, rad=[3, 5], why="odd N (no Nyquist bin)"),
    dict(n_fft=63, hop=16, L=300, pad=2, B=2, rad=[3, 3, 7], why="constant padding"),
    dict(n_fft=122, hop=61, L=700, pad=1, B=2, rad=[2, 61], why="R = 61, the full v[61] array"),
    dict(n_fft=143, hop=32, L=700, pad=0, B=2, rad=[11, 13], why="no padding"),
    dict(n_fft=250, hop=50, L=1000, pad=1, B=2, rad=[2, 5, 5, 5], why="2 5 5 5"),
    dict(n_fft=960, hop=480, L=5280, pad=0, B=2, rad=[4, 4, 4, 3, 5], why="DeepFilterNet's geometry"),
    dict(n_fft=960, hop=480, L=5760, pad=0, B=2, rad=[4, 4, 4, 3, 5], why="DeepFilterNet's geometry, odd n_frames (11)"),
    dict(n_fft=2048, hop=512, L=6000, pad=1, B=2, rad=[4, 4, 4, 4, 4, 2], why="pairs = 1"),
    dict(n_fft=4096, hop=1024, L=9000, pad=1, B=1, rad=[4, 4, 4, 4, 4, 4], why="LDS 96 KB: the hipFuncSetAttribute branch"),
    dict(n_fft=96, hop=24, L=40, pad=2, B=2, rad=[4, 4, 2, 3], n_frames=1, why="n_frames = 1: the odd partner frame is absent"),
    dict(n_fft=56, hop=14, L=29, pad=1, B=2, rad=[4, 2, 7], why="L = n_fft / 2 + 1, the shortest reflect-admissible signal"),
    dict(n_fft=45, hop=9, L=200, pad=1, B=2, rad=[3, 3, 5], ld=217, why="x a [:, :L] view of a wider buffer: ldx != L"),
]
STOCKHAM_REFUSED = [134, 2 * 67 * 4]
PLAN_RADICES = {2, 3, 4, 5, 7, 11, 13, 61}


def stockham_id(c):
    return f"n{c['n_fft']}-h{c['hop']}-L{c['L']}-p{c['pad']}"


def stockham_frames(c):
    return c.get("n_frames", n_frames_of(c["L"], c["n_fft"], c["hop"], c["pad"]))


# B. mi355_logmel on the generic path
LOGMEL_GENERIC = [dict(n_fft=96, hop=24, L=500, n_mels=13), dict(n_fft=250, hop=50, L=1000, n_mels=40)]

# C. fast kernels: (n_fft, hop not a multiple of 4)
FAST_ODD_HOPS = {400: 150, 512: 130, 1024: 250}
FAST_HOPS = {400: 160, 512: 128, 1024: 256}

# D. mi355_istft: n_fft, hop, n_frames (B = 2)
ISTFT_CASES = [
    (2, 1, 7), (2, 2, 8), (20, 5, 1), (20, 5, 2), (20, 1, 8), (20, 20, 7), (20, 23, 8), (96, 24, 7), (96, 96, 2), (96, 99, 7),
    (122, 30, 7), (122, 125, 2), (960, 480, 7), (960, 240, 1), (960, 960, 8), (1024, 256, 8), (1024, 256, 7), (1024, 1027, 2), (1024, 256, 1),
]

# E. small-FFT heads: (n_fft, hop) of the generic kernels; the signal length of each is no multiple of hop for the odd size
HEAD_GENERIC = [(16, 4), (15, 5), (64, 16), (64, 1), (20, 4)]
MAGPHASE_FAST_LENGTHS = [11, 254 * 5 + 2, 255 * 5 + 3, 256 * 5, 599 * 5 + 4]   # frames 3 (the fewest L > n_fft / 2 allows), 255, 256, 257, 600
HEAD_FAST_FRAMES = [2, 252, 253, 260]


def magphase_input(B, L, seed):
    """Unit-variance noise: keeps the share of near-zero bins (|X| < 1e-4, where the phase is not compared) far below 1 %."""
    return unit_noise((B, L), seed)


def magphase_generic_case(n_fft, hop):
    L = 37 * hop + (hop // 2 if hop > 1 else 0) + n_fft    # no multiple of hop unless hop == 1
    if n_fft % 2 == 1 and L % hop == 0:
        L += 1
    lens = [L, n_fft // 2 + 1 + (1 if (n_fft % 2 == 1 and (n_fft // 2 + 1) % hop == 0) else 0), (L * 2) // 3]
    if n_fft % 2 == 1 and lens[2] % hop == 0:
        lens[2] += 1
    return L, lens


def head_input(B, Fr, nb, seed):
    """conv_post-like rows: log-magnitudes around -1 (std 0.5), phases of unit variance (tests/test_kernels_gpu.py test_istft_head)."""
    x = unit_noise((B, Fr, 2 * nb), seed)
    x[:, :, :nb] = x[:, :, :nb] * 0.5 - 1.0
    return x


# F. kaldi_frames: win, n_fft, shift, pad, n_frames, L ("limit": (n_frames - 1) shift + win - pad == L + pad)
KALDI_CASES = [
    dict(win=25, n_fft=32, shift=10, pad=0, n_frames=5, L=70, limit=False),
    dict(win=400, n_fft=512, shift=160, pad=120, n_frames=4, L=640, limit=True),
    dict(win=1920, n_fft=2048, shift=384, pad=0, n_frames=3, L=2700, limit=False),
    dict(win=300, n_fft=300, shift=100, pad=100, n_frames=5, L=500, limit=True),
]
# polar_spec: B, Fr, nb, ldx, batch stride (0: Fr * ldx)
POLAR_CASES = [(1, 1, 1, 2, 0), (2, 3, 513, 1030, 0), (3, 5, 7, 16, 5 * 16 + 24)]
POLAR_CLIP = 1e2


def polar_input(B, Fr, nb, seed):
    """Log-magnitudes N(ln(clip), 1.5): about half above the clip; phases N(0, 2)."""
    x = unit_noise((B, Fr, 2 * nb), seed)
    x[..., :nb] = x[..., :nb] * 1.5 + math.log(POLAR_CLIP)
    x[..., nb:] = x[..., nb:] * 2.0
    return x


# ----------------------------------------------------------------------------------------------------------------- derived inputs
# the spectra below are the Hamming-windowed frames of unit noise and the clamp is to +-(the same Hamming window), so a sample is clipped where
# gain * |x| > 1: at gain 0.75 that is P(|N(0, 1)| > 4 / 3) = 18 %, well inside the 5 % .. 50 % the clamp case asks for on either side -- the
# n_fft = 2 cases have only 28 and 32 samples, whose realised share strays far from the expectation (asserted per case on the CPU)
ISTFT_CLAMP_GAIN = 0.75


def istft_inputs(n_fft, hop, n_frames, B=2):
    """(spec complex64 [B, n_frames, nb], synthesis window) of every mi355_istft case: the float64 STFT (Hamming analysis window, no padding) of unit
    noise, rounded to the complex64 the kernel receives; the synthesis window is the same symmetric Hamming window, which has no zero, so that
    the trim = 0 launches do not divide by a vanishing envelope."""
    x = unit_noise((B, (n_frames - 1) * hop + n_fft), 1000 * n_fft + 10 * hop + n_frames)
    spec = stft_stmt(x, hamming(n_fft), n_fft, hop, PAD_NONE, n_frames, torch.float64).to(torch.complex64)
    return spec, hamming(n_fft)


def istft_clamp_share(n_fft, hop, n_frames):
    """Share of the irfft samples of the clamp launch (spectrum times ISTFT_CLAMP_GAIN) that exceed its window, in float64."""
    spec, w = istft_inputs(n_fft, hop, n_frames)
    fr = torch.fft.irfft(spec.to(torch.complex128) * ISTFT_CLAMP_GAIN, n=n_fft, dim=-1)
    return float((fr.abs() > w.double()).double().mean())


def load_path_lengths(n_fft, hop):
    """(L with L % 4 == 0, L with L % 4 != 0) for the load-path identity cases: five tiles' worth of frames past one window."""
    T = 2 * fast_geom_of(n_fft).PW
    L0 = (n_fft + 5 * T * hop + 3) // 4 * 4
    return L0, L0 + 1


ALTERNATING = {400: (40, 680), 512: (64, 704), 1024: (128, 1408)}


def alternating_case(n_fft):
    """(hop, L) of an item of three tiles under reflect padding: edge, interior, edge."""
    return ALTERNATING[n_fft]


SHORT_LAUNCHES = ["one", "T-1", "T", "T+1"]


def short_launch_case(n_fft, which):
    """(hop, L, n_frames, B) with n_frames = 1, 2 PW - 1, 2 PW, 2 PW + 1 under constant padding (reflect padding cannot have one frame: it needs
    L > n_fft / 2 >= hop); B = 1 at one frame, so the launch has fewer tiles than a workgroup has waves."""
    T = 2 * fast_geom_of(n_fft).PW
    nfr = {"one": 1, "T-1": T - 1, "T": T, "T+1": T + 1}[which]
    hop = FAST_HOPS[n_fft]
    return hop, (nfr - 1) * hop + hop // 2, nfr, 1 if nfr == 1 else 2


def derived_forward_geometries():
    """(n_fft, hop, L, pad_mode, n_frames) of every forward case outside STOCKHAM_CASES whose shape does not depend on the device."""
    out = [(c["n_fft"], c["hop"], c["L"], 1, n_frames_of(c["L"], c["n_fft"], c["hop"], 1)) for c in LOGMEL_GENERIC]
    for n in FAST_SPLIT:
        for hop in (FAST_HOPS[n], FAST_ODD_HOPS[n]):
            out += [(n, hop, L, 1, n_frames_of(L, n, hop, 1)) for L in load_path_lengths(n, hop)]
        hop, L = alternating_case(n)
        out.append((n, hop, L, 1, n_frames_of(L, n, hop, 1)))
        for which in SHORT_LAUNCHES:
            hop, L, nfr, _ = short_launch_case(n, which)
            out.append((n, hop, L, 2, nfr))
    return out
