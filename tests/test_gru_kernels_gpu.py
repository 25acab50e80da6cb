"""``csrc/gru.hip`` (``mi355_gru_seq``) against float64 on the host over the same 16-bit-rounded recurrent weights (``tests/_gru_ref.py``)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _gru_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
BAR = 5e-5   # the LSTM test's bar on outputs bounded by 1 (test_kernels_gpu.py::test_lstm_vs_oracle)
B = 3


def _views(xproj, H, T, strided):
    """(xproj view, out view, the whole out buffer): ``strided`` puts both behind a column offset inside wider rows."""
    if not strided:
        return torch.from_numpy(xproj).to(DEV), (o := torch.full((B, T, H), 7.0, device=DEV)), o
    xbuf = torch.full((B, T, 3 * H + 40), 3.0, device=DEV)
    xbuf[:, :, 8:8 + 3 * H] = torch.from_numpy(xproj).to(DEV)
    obuf = torch.full((B, T, H + 24), 7.0, device=DEV)
    return xbuf[:, :, 8:8 + 3 * H], obuf[:, :, 16:16 + H], obuf


@pytest.mark.parametrize("strided", [True, False])
@pytest.mark.parametrize("with_h0", [False, True])
@pytest.mark.parametrize("with_lens", [True, False])
@pytest.mark.parametrize("T", [1, 2, 37])
@pytest.mark.parametrize("H", [64, 128, 256])
def test_gru_seq_vs_float64(H, T, with_lens, with_h0, strided):
    """Outputs are bounded by 1 (h is a convex mix of tanh values and h0 in (-1, 1)); bar 5e-5 absolute.  Both sides hold the same weights, so what is
    left is float32 rounding of the 3 H-term sums and the two activations, damped by z at every step.
    Measured on MI355X over all 72 cases: the largest |out - float64| is 2.6e-7 (H = 256, T = 37, no lens, no h0), 0.005 of the bar.
    Rows beyond ``lens`` are exactly zero, bytes outside the views are untouched, ``hT`` is the last valid row, and a second run gives the same bits."""
    from mlx_audio_amd import ops

    xproj, wh, bhn, h0 = R.make_case(H, T, B, seed=1000 * H + 10 * T + 2 * with_lens + with_h0)
    lens = [T, 1, max(1, T // 2)] if with_lens else None
    wr, k = ops.round_gru_wh(torch.from_numpy(wh))
    assert float((wr - torch.from_numpy(wh)).abs().max()) <= 2.0 ** -11 * float(np.abs(wh).max())   # half's 11 significant bits
    ref, ref_hT = R.gru_seq(xproj, wr.numpy(), bhn, h0 if with_h0 else None, lens)
    img = ops.pack_gru_wh(torch.from_numpy(wh), DEV)
    assert img.scale == 2.0 ** -k and img.h == H
    bhn_d = torch.from_numpy(bhn).to(DEV)
    h0_d = torch.from_numpy(h0).to(DEV) if with_h0 else None
    lens_d = torch.tensor(lens, dtype=torch.int32, device=DEV) if with_lens else None
    runs = []
    for _ in range(2):
        xv, ov, obuf = _views(xproj, H, T, strided)
        _, hT = ops.gru_seq(xv, img, bhn_d, ov, h0=h0_d, lens=lens_d, return_state=True)
        torch.cuda.synchronize()
        runs.append((ov.cpu().clone(), hT.cpu(), obuf.cpu()))
    out, hT, obuf = runs[0]
    err = float(np.abs(out.double().numpy() - ref).max())
    err_h = float(np.abs(hT.double().numpy() - ref_hT).max())
    print(f"gru_seq H={H} T={T} lens={with_lens} h0={with_h0} strided={strided}: max|out - f64| = {err:.3e}, max|hT - f64| = {err_h:.3e}, bar {BAR:.0e}")
    assert err < BAR and err_h < BAR
    assert float(np.abs(ref).max()) < 1.0
    for b in range(B):
        n = T if lens is None else lens[b]
        assert n == T or float(out[b, n:].abs().max()) == 0.0
        assert torch.equal(hT[b], out[b, n - 1])
    if strided:
        assert torch.equal(obuf[:, :, :16], torch.full_like(obuf[:, :, :16], 7.0)) and torch.equal(obuf[:, :, 16 + H:], torch.full_like(obuf[:, :, 16 + H:], 7.0))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


def test_gru_seq_chained_state_and_empty_item():
    """A sequence run in two halves through ``hT`` -> ``h0`` gives the bits of the whole run (same sums in the same order), and an item with
    ``lens`` 0 writes only zeros and hands ``h0`` back."""
    from mlx_audio_amd import ops

    H, T = 128, 10
    xproj, wh, bhn, h0 = R.make_case(H, T, B, seed=5)
    img = ops.pack_gru_wh(torch.from_numpy(wh), DEV)
    x, bhn_d, h0_d = torch.from_numpy(xproj).to(DEV), torch.from_numpy(bhn).to(DEV), torch.from_numpy(h0).to(DEV)
    whole = torch.empty(B, T, H, device=DEV)
    ops.gru_seq(x, img, bhn_d, whole, h0=h0_d)
    parts = torch.empty(B, T, H, device=DEV)
    _, mid = ops.gru_seq(x[:, :4], img, bhn_d, parts[:, :4], h0=h0_d, return_state=True)
    ops.gru_seq(x[:, 4:], img, bhn_d, parts[:, 4:], h0=mid)
    out0 = torch.full((B, T, H), 7.0, device=DEV)
    _, hT = ops.gru_seq(x, img, bhn_d, out0, h0=h0_d, lens=torch.tensor([0, T, 0], dtype=torch.int32, device=DEV), return_state=True)
    torch.cuda.synchronize()
    assert torch.equal(whole, parts)
    assert float(out0[0].abs().max()) == 0.0 and float(out0[2].abs().max()) == 0.0 and torch.equal(out0[1], whole[1])
    assert torch.equal(hT[0], h0_d[0]) and torch.equal(hT[2], h0_d[2]) and torch.equal(hT[1], whole[1, -1])


def test_gru_seq_unsupported_hidden_size():
    from mlx_audio_amd import _lib, ops

    H, T = 96, 3
    xproj, wh, bhn, _ = R.make_case(H, T, B, seed=1)
    img = ops.pack_gru_wh(torch.from_numpy(wh), DEV)
    out = torch.full((B, T, H), 7.0, device=DEV)
    with pytest.raises(_lib.Mi355Error, match=r"\(-3\).*unsupported hidden size 96"):
        ops.gru_seq(torch.from_numpy(xproj).to(DEV), img, torch.from_numpy(bhn).to(DEV), out)
    torch.cuda.synchronize()
    assert float((out - 7.0).abs().max()) == 0.0   # refused without a launch
