"""The generator tail in one launch (``ops.conv_post_istft`` -> ``mi355_conv_post_istft``): LeakyReLU -> conv_post (128 -> 22, k = 7) -> exp / sin ->
iSTFT (n_fft 20, hop 5), against a float64 numpy statement written here and against the two launches it replaces (``ops.conv_gemm`` at precision 2
+ ``ops.istft_head``), which are the reference kernels of this file, not the code under test.

Shapes: frame blocks of the kernel own 252 frames (256 staged), so lens = [509, 253, 252, 9] puts items on two blocks + a remainder, on either side
of a block seam and below two halos; B = 2, L = 300 is the uniform case.  Weights are bf16-valued with std 0.02 (conv output std ~0.4: exp finite).

Parity rule: max |fused - f64| / peak <= 1.5 x max |two-launch - f64| / peak, both measured in the same test (the paths differ at most in fp32
summation order).  Measured on MI355X: see docs/PARITY.md (conv_post + iSTFT head)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
CIN, COUT, K, NFFT, HOP = 128, 22, 7, 20, 5
SLOPE = 0.01
SENTINEL = -777.0
RAGGED = [509, 253, 252, 9]


@pytest.fixture(scope="module")
def ops():
    from mlx_audio_amd import ops as _ops

    _ops.require_gpu()
    return _ops


def _bf16_valued(t):
    return t.to(torch.bfloat16).to(torch.float32)


def _hann(n):
    return (0.5 * (1.0 - np.cos(2.0 * np.pi * np.arange(n) / n))).astype(np.float32)   # periodic Hann, as the engine builds it


def _weights(seed, cout=COUT, k=K, cin=CIN):
    g = torch.Generator().manual_seed(seed)
    w = _bf16_valued(torch.randn(cout, k, cin, generator=g) * 0.02)
    b = torch.randn(cout, generator=g) * 0.1
    return w, b


def head_f64(post, win, n_fft, hop):
    """The iSTFT of tests/test_kernels_gpu.py::test_istft_head, restated in float64: post [n, n_fft + 2] -> audio [(n - 1) * hop]."""
    n, nb = post.shape[0], n_fft // 2 + 1
    mag, ph = np.exp(post[:, :nb]), np.sin(post[:, nb:2 * nb])
    fr = np.fft.irfft(mag * np.cos(ph) + 1j * mag * np.sin(ph), n=n_fft, axis=-1) * win[None, :]
    total = (n - 1) * hop + n_fft
    rec, env = np.zeros(total), np.zeros(total)
    for f in range(n):
        rec[f * hop:f * hop + n_fft] += fr[f]
        env[f * hop:f * hop + n_fft] += win * win
    out = np.where(env > 1e-10, rec / np.where(env > 1e-10, env, 1.0), rec)
    return out[n_fft // 2:n_fft // 2 + (n - 1) * hop]


def tail_f64(x, w, b, win, lens, n_fft=NFFT, hop=HOP, slope=SLOPE):
    """LeakyReLU -> zero-padded conv (pad = (k - 1) / 2) with the given weights + bias -> head_f64; one array per item."""
    x, w, b, win = x.double().numpy(), w.double().numpy(), b.double().numpy(), win.astype(np.float64)
    k = w.shape[1]
    outs = []
    for i, n in enumerate(lens):
        xa = x[i, :n]
        xa = np.where(xa > 0, xa, xa * slope)
        xp = np.concatenate([np.zeros((k // 2, xa.shape[1])), xa, np.zeros((k // 2, xa.shape[1]))])
        post = np.broadcast_to(b, (n, w.shape[0])).copy()
        for t in range(k):
            post += xp[t:t + n] @ w[:, t, :].T
        outs.append(head_f64(post, win, n_fft, hop))
    return outs


def two_launch(ops, x, pc, win, audio, lens, n_fft=NFFT, hop=HOP, pre_fq=None):
    """Today's path: conv_post as a conv_gemm launch into `post`, then the head on it."""
    B, L, _ = x.shape
    post = torch.zeros(B, L, ops.round_up(pc.cout, 4), device=DEV)[:, :, :pc.cout]
    ops.conv_gemm(x, pc, post, pad=3, lens_in=lens, lens_out=lens, pre_act=ops.ACT_LEAKY, pre_slope=SLOPE, precision=2, pre_fq=pre_fq)
    ops.istft_head(post, n_fft, hop, win, audio, lens=lens)
    return audio


class Case:
    """One input batch, its float64 statement and both device results (computed once per module)."""

    def __init__(self, ops, seed, B, L, lens):
        g = torch.Generator().manual_seed(seed)
        self.w, self.b = _weights(seed + 100)
        self.pc = ops.pack_conv(self.w, self.b, DEV)
        self.x = torch.randn(B, L, CIN, generator=g)
        self.xd = self.x.to(DEV)
        self.lens = lens
        self.ld = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
        self.win = _hann(NFFT)
        self.wd = torch.from_numpy(self.win).to(DEV)
        self.ref = tail_f64(self.x, self.w, self.b, self.win, lens if lens is not None else [L] * B)
        assert ops.conv_post_istft_eligible(self.pc, NFFT, HOP)
        self.fused = ops.conv_post_istft(self.xd, self.pc, NFFT, HOP, self.wd, self.new_audio(), lens=self.ld, pre_slope=SLOPE).cpu()
        self.two = two_launch(ops, self.xd, self.pc, self.wd, self.new_audio(), self.ld).cpu()
        torch.cuda.synchronize()

    def new_audio(self):
        B, L, _ = self.x.shape
        return torch.full((B, (L - 1) * HOP), SENTINEL, device=DEV)

    def errors(self):
        peak = max(float(np.abs(r).max()) for r in self.ref)
        ef = max(float(np.abs(self.fused[i, :len(r)].double().numpy() - r).max()) for i, r in enumerate(self.ref) if len(r))
        et = max(float(np.abs(self.two[i, :len(r)].double().numpy() - r).max()) for i, r in enumerate(self.ref) if len(r))
        return ef / peak, et / peak, peak


@pytest.fixture(scope="module")
def ragged(ops):
    return Case(ops, 1, len(RAGGED), max(RAGGED), RAGGED)


@pytest.fixture(scope="module")
def uniform(ops):
    return Case(ops, 2, 2, 300, None)


@pytest.mark.parametrize("which", ["ragged", "uniform"])
def test_parity_against_float64_and_the_two_launches(which, request):
    c = request.getfixturevalue(which)
    ef, et, peak = c.errors()
    same = all(torch.equal(c.fused[i, :len(r)], c.two[i, :len(r)]) for i, r in enumerate(c.ref))
    print(f"conv_post_istft {which}: fused {ef:.3e}  two-launch {et:.3e}  of peak {peak:.3f}  bit-equal to the two launches: {same}")
    assert np.isfinite(ef) and peak > 0.01
    assert ef <= 1.5 * et, (ef, et)


def test_identical_rows_and_repeat(ops, ragged):
    c = ragged
    x3 = c.xd[:1].expand(3, -1, -1).contiguous()
    a1 = ops.conv_post_istft(x3, c.pc, NFFT, HOP, c.wd, torch.full((3, (x3.shape[1] - 1) * HOP), SENTINEL, device=DEV), pre_slope=SLOPE).cpu()
    a2 = ops.conv_post_istft(x3, c.pc, NFFT, HOP, c.wd, torch.full((3, (x3.shape[1] - 1) * HOP), SENTINEL, device=DEV), pre_slope=SLOPE).cpu()
    assert torch.equal(a1[0], a1[1]) and torch.equal(a1[0], a1[2])
    assert torch.equal(a1, a2)
    assert not bool((a1 == SENTINEL).any())


def test_batch_invariance(ops, ragged):
    c = ragged
    n = (RAGGED[0] - 1) * HOP
    alone = ops.conv_post_istft(c.xd[:1].contiguous(), c.pc, NFFT, HOP, c.wd, torch.full((1, n), SENTINEL, device=DEV),
                                lens=torch.tensor(RAGGED[:1], dtype=torch.int32, device=DEV), pre_slope=SLOPE).cpu()
    assert torch.equal(alone[0], c.fused[0, :n])


def test_untouched_tails(ragged):
    c = ragged
    for i, n in enumerate(RAGGED):
        valid = (n - 1) * HOP   # the head writes (lens - 1) * hop samples: everything from there on -- lens * hop and beyond included -- keeps the sentinel
        assert bool((c.fused[i, valid:] == SENTINEL).all()), i
        assert not bool((c.fused[i, :valid] == SENTINEL).any()), i


def test_fallback_is_the_two_launches(ops, ragged):
    c = ragged
    # a quantising prologue: not the fused kernel's
    mm = ops.fake_quant_extrema(c.xd, lens=c.ld, pre_act=ops.ACT_LEAKY, pre_slope=SLOPE)
    assert not ops.conv_post_istft_eligible(c.pc, NFFT, HOP, pre_fq=mm)
    got = ops.conv_post_istft(c.xd, c.pc, NFFT, HOP, c.wd, c.new_audio(), lens=c.ld, pre_slope=SLOPE, pre_fq=mm).cpu()
    want = two_launch(ops, c.xd, c.pc, c.wd, c.new_audio(), c.ld, pre_fq=mm).cpu()
    assert torch.equal(got, want)
    # n_fft 16, hop 4 (18 columns): the generic head
    w, b = _weights(7, cout=18)
    pc = ops.pack_conv(w, b, DEV)
    wd = torch.from_numpy(_hann(16)).to(DEV)
    assert not ops.conv_post_istft_eligible(pc, 16, 4)
    new = lambda: torch.full((c.xd.shape[0], (c.xd.shape[1] - 1) * 4), SENTINEL, device=DEV)
    got = ops.conv_post_istft(c.xd, pc, 16, 4, wd, new(), lens=c.ld, pre_slope=SLOPE).cpu()
    want = two_launch(ops, c.xd, pc, wd, new(), c.ld, n_fft=16, hop=4).cpu()
    assert torch.equal(got, want)
