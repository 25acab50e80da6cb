"""``csrc/align.hip`` kernel by kernel: the DTW path bit for bit against ``tests/_whisper_timing_ref.py`` (and the reference's stored outputs), the median
filter as an exact selection, the matrix and QK-softmax kernels against float64 with the bar "4 x the float32 restatement's own error on the same
inputs" (the margin covers another summation order and square-root / division path), ``softmax_prob_rows`` against float64, and the refusals."""
import json
import os

import numpy as np
import pytest
import torch

import _whisper_timing_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLD, "ref_whisper_timing.npz")), json.load(open(os.path.join(GOLD, "ref_whisper_timing.json")))


def _matrix(kind, N, M, seed):
    g = np.random.default_rng(seed)
    if kind == "random":
        return g.standard_normal((N, M)).astype(np.float32)
    if kind == "integer":
        return g.integers(-2, 3, size=(N, M)).astype(np.float32)
    return np.zeros((N, M), np.float32)


def _dev_dtw(x):
    from mlx_audio_amd.stt.models.whisper.timing import dtw

    return dtw(x)


def test_helper_dtw_antidiagonal_equals_cell_by_cell():
    for kind in ("random", "integer", "zero"):
        for N, M in ((1, 1), (1, 9), (7, 1), (13, 29)):
            x = _matrix(kind, N, M, 3)
            np.testing.assert_array_equal(R.dtw(x), R.dtw_scalar(x))


@pytest.mark.parametrize("kind", ["random", "integer", "zero"])
@pytest.mark.parametrize("shape", [(1, 1), (1, 9), (7, 1), (40, 13), (65, 130)])
def test_dtw_path_is_bit_exact(kind, shape):
    x = _matrix(kind, *shape, seed=11)
    got = _dev_dtw(x)
    want = R.dtw(x)
    assert got.shape == want.shape, (got.shape, want.shape)
    np.testing.assert_array_equal(got, want)


def test_dtw_largest_window_once():
    x = _matrix("random", 448, 1500, seed=5)
    np.testing.assert_array_equal(_dev_dtw(x), R.dtw(x))


def test_dtw_equals_the_reference_outputs(fx):
    npz, meta = fx
    for name in meta["matrices"]:
        x = npz[f"mat_{name}"]
        np.testing.assert_array_equal(_dev_dtw(x), npz[f"mat_{name}_path"], err_msg=name)
        np.testing.assert_array_equal(R.dtw(x), npz[f"mat_{name}_path"], err_msg=name)


def test_dtw_ragged_batch_ignores_poisoned_padding():
    from mlx_audio_amd import ops

    sizes = [(40, 13), (7, 130), (65, 77)]
    N, M = 65, 130
    cost = np.full((3, N, M + 3), np.nan, np.float32)     # padding (and 3 spare columns per row) is NaN
    mats = []
    for b, (n, m) in enumerate(sizes):
        x = _matrix("integer" if b == 1 else "random", n, m, seed=20 + b)
        cost[b, :n, :m] = x
        mats.append(x)
    c = torch.from_numpy(cost).to(DEV)[:, :, :M]
    ln = torch.tensor([s[0] for s in sizes], dtype=torch.int32, device=DEV)
    lm = torch.tensor([s[1] for s in sizes], dtype=torch.int32, device=DEV)
    text, time, plen = ops.dtw(c, lens_n=ln, lens_m=lm)
    text, time, plen = text.cpu().numpy(), time.cpu().numpy(), plen.cpu().numpy()
    for b, x in enumerate(mats):
        want = R.dtw(x)
        L = int(plen[b])
        assert L == want.shape[1]
        np.testing.assert_array_equal(text[b, :L], want[0])
        np.testing.assert_array_equal(time[b, :L], want[1])


@pytest.mark.parametrize("F", [1, 3, 4, 7, 85, 750])
def test_median_filter_is_an_exact_selection(F):
    from mlx_audio_amd.stt.models.whisper.timing import median_filter

    g = np.random.default_rng(F)
    x = g.standard_normal((2, 3, F)).astype(np.float32)
    x[0, 1] = np.round(x[0, 1])                     # ties
    got = median_filter(torch.from_numpy(x).to(DEV), 7)
    assert got.shape == x.shape and got.is_cuda
    np.testing.assert_array_equal(got.cpu().numpy(), R.median_filter(x, 7))
    got2 = median_filter(x[0], 5)                   # array in -> array out, another width
    assert isinstance(got2, np.ndarray)
    np.testing.assert_array_equal(got2, R.median_filter(x[0], 5))


def test_median_filter_equals_the_reference_outputs(fx):
    from mlx_audio_amd.stt.models.whisper.timing import median_filter

    npz, meta = fx
    for name in meta["matrices"]:
        x = npz[f"mat_{name}"]
        np.testing.assert_array_equal(median_filter(x, 7), npz[f"mat_{name}_medfilt"], err_msg=name)


def _probs(A, T, F, seed):
    g = np.random.default_rng(seed)
    s = 2.0 * g.standard_normal((A, T, F))
    e = np.exp(s - s.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True)).astype(np.float32)


@pytest.mark.parametrize("A", [1, 8])
@pytest.mark.parametrize("T", [2, 6, 70])
@pytest.mark.parametrize("F", [4, 85, 750])
def test_align_matrix_against_float64(A, T, F):
    from mlx_audio_amd import ops

    w = _probs(A, T, F, seed=A * 1000 + T * 10 + F)
    row_begin = 1 if T > 2 else 0
    want64 = R.align_matrix(w.astype(np.float64), 7, row_begin, 1, np.float64)
    want32 = R.align_matrix(w, 7, row_begin, 1, np.float32)
    # one padded batch of two items: item 1 is item 0's data inside a larger, poisoned buffer
    buf = torch.full((2, A, T + 2, F + 5), float("nan"), device=DEV)
    buf[:, :, :T, :F] = torch.from_numpy(w).to(DEV)
    lens_t = torch.tensor([T, T], dtype=torch.int32, device=DEV)
    lens_f = torch.tensor([F, F], dtype=torch.int32, device=DEV)
    out = torch.full((2, T + 1, F + 5), float("nan"), device=DEV)
    ops.align_matrix(buf, out, T=T + 2, F=F + 5, lens_t=lens_t, lens_f=lens_f, medfilt_width=7, row_begin=row_begin, row_trim=1)
    got = out.cpu().numpy()
    N = T - 1 - row_begin
    assert np.isnan(got[:, N:]).all() and np.isnan(got[:, :, F:]).all()          # nothing written beyond the item's own lengths
    e_dev = float(np.abs(got[:, :N, :F].astype(np.float64) - want64).max())
    e_f32 = float(np.abs(want32.astype(np.float64) - want64).max())
    print(f"align_matrix A={A} T={T} F={F}: device error {e_dev:.3e}, float32 restatement error {e_f32:.3e}")
    assert e_dev <= 4 * e_f32


@pytest.mark.parametrize("dh", [64, 128])
@pytest.mark.parametrize("kv", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("head_major", [False, True])
@pytest.mark.parametrize("TF", [(1, 85), (6, 750), (70, 1500)])
def test_align_qk_softmax_against_float64(dh, kv, head_major, TF):
    from mlx_audio_amd import ops

    T, F = TF
    H, B = 5, 2
    dt = dict(f32=torch.float32, f16=torch.float16, bf16=torch.bfloat16)[kv]
    g = torch.Generator().manual_seed(dh + T + F)
    q = torch.randn(B, T, H * dh, generator=g)
    k = torch.randn(B, F + 3, H * dh, generator=g).to(dt)        # rounded to the cache type before either side sees it
    pairs = [(4, 0), (0, 2), (2, 1)]                              # skips heads 1 and 3, permutes the slots
    lens_t = [T, max(T - 1, 1)]
    lens_f = [F, F - 2]
    scale, qk_scale = dh ** -0.5, 1.5
    kd = k.to(DEV)
    if head_major:
        kd = kd.view(B, F + 3, H, dh).permute(0, 2, 1, 3).contiguous()
    w = torch.full((B, 4, T + 1, F + 4), float("nan"), device=DEV)
    ops.align_qk_softmax(q.to(DEV), kd, w, torch.tensor(pairs, dtype=torch.int32, device=DEV), heads=H, dh=dh, scale=scale, qk_scale=qk_scale,
                         lens_t=torch.tensor(lens_t, dtype=torch.int32, device=DEV), lens_f=torch.tensor(lens_f, dtype=torch.int32, device=DEV),
                         head_major=head_major, F=F)
    got = w.cpu().numpy()
    assert np.isnan(got[:, 3]).all()                              # the slot no pair names stays untouched
    kf = k.float().numpy()
    e_dev = e_f32 = 0.0
    for b in range(B):
        tb, fb = lens_t[b], lens_f[b]
        assert np.isnan(got[b, :3, tb:]).all() and np.isnan(got[b, :3, :, fb:]).all()
        for head, slot in pairs:
            qq = q[b, :tb, head * dh:(head + 1) * dh].numpy()
            kk = kf[b, :fb, head * dh:(head + 1) * dh]
            w64 = R.qk_softmax(qq, kk, scale, qk_scale, np.float64)
            w32 = R.qk_softmax(qq, kk, scale, qk_scale, np.float32)
            gw = got[b, slot, :tb, :fb]
            e_dev = max(e_dev, float(np.abs(gw.astype(np.float64) - w64).max()))
            e_f32 = max(e_f32, float(np.abs(w32.astype(np.float64) - w64).max()))
            rows = gw.astype(np.float64).sum(-1)
            assert np.abs(rows - 1.0).max() <= fb * 2.0 ** -24, rows   # each of the fb terms rounded once, relative to a sum of 1
    print(f"align_qk_softmax dh={dh} {kv} head_major={head_major} T={T} F={F}: device error {e_dev:.3e}, float32 restatement error {e_f32:.3e}")
    assert e_dev <= 4 * e_f32


def test_softmax_prob_rows_against_float64():
    from mlx_audio_amd import ops

    V, R_, ld = 50257, 9, 51868
    g = torch.Generator().manual_seed(2)
    lg = 3.0 * torch.randn(R_, ld, generator=g)
    tok = torch.tensor([0, 50256, 17, 31000, 4, 50000, 123, 9999, 25000], dtype=torch.int32)
    got = ops.softmax_prob_rows(lg.to(DEV), tok.to(DEV), V=V).cpu().numpy().astype(np.float64)
    want = R.softmax_prob_rows(lg.numpy(), tok.numpy(), V)
    # V terms of at most 1 summed in float32 (tree of depth ~ 16 + serial 50 per lane) and two exp evaluations: a few 1e-6 relative at the outside
    np.testing.assert_allclose(got, want, rtol=2e-5, atol=0)


def test_refusals_launch_nothing():
    from mlx_audio_amd import _lib, ops

    lib = _lib.load()

    def err():
        return lib.mi355_last_error().decode()

    assert lib.mi355_align_qk_softmax(None, None) == -1 and "null" in err()
    assert lib.mi355_align_matrix(None, None) == -1 and "null" in err()
    assert lib.mi355_dtw(None, None) == -1 and "null" in err()
    assert lib.mi355_softmax_prob_rows(None, 0, 0, 0, None, None, None) == -1 and "null" in err()
    x = torch.zeros(1, 1025, 4, device=DEV)
    with pytest.raises(_lib.Mi355Error, match="1024"):
        ops.dtw(x)
    w = torch.zeros(1, 1, 4, 16, device=DEV)
    o = torch.zeros(1, 4, 16, device=DEV)
    with pytest.raises(_lib.Mi355Error, match="odd"):
        ops.align_matrix(w, o, medfilt_width=6)
    q = torch.zeros(1, 2, 2 * 96, device=DEV)
    k = torch.zeros(1, 8, 2 * 96, device=DEV)
    ww = torch.full((1, 1, 2, 8), 7.0, device=DEV)
    with pytest.raises(_lib.Mi355Error, match="dh"):
        ops.align_qk_softmax(q, k, ww, torch.zeros(1, 2, dtype=torch.int32, device=DEV), heads=2, dh=96)
    torch.cuda.synchronize()
    assert float(ww.min()) == 7.0 and float(o.abs().max()) == 0.0
    assert lib.mi355_dtw_ws_bytes(448, 1500, 1) >= 448 * (448 + 1500 - 1)


def test_median_filter_propagates_nan_like_np_median():
    from mlx_audio_amd.stt.models.whisper.timing import median_filter

    x = np.random.default_rng(0).standard_normal((3, 40)).astype(np.float32)
    x[1, 17] = np.nan
    xp = np.pad(x, ((0, 0), (3, 3)), mode="reflect")
    want = np.median(np.lib.stride_tricks.sliding_window_view(xp, 7, axis=-1), axis=-1)
    got = median_filter(x, 7)
    np.testing.assert_array_equal(got, want)          # NaN in the seven windows that touch column 17 of row 1, exact selection elsewhere
    assert np.isnan(got).sum() == 7
