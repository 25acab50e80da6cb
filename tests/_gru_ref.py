"""The contract of ``mi355_gru_seq`` (include/mi355audio.h) restated in float64 numpy: test infrastructure, shared by the CPU and the GPU tests.

MLX nn.GRU semantics: ``xproj`` [B, T, 3H] = x Wx^T + b with gate blocks r | z | n (PyTorch's bias_hh r / z parts folded into b), and per step
    r = sigmoid(x_r + (Wh h)_r),  z = sigmoid(x_z + (Wh h)_z),  n = tanh(x_n + r * ((Wh h)_n + bhn)),  h' = (1 - z) n + z h.
Rows at and beyond ``lens[b]`` are zeros; the returned state is the one after step ``lens[b]``."""
import numpy as np


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def gru_seq(xproj, wh, bhn, h0=None, lens=None):
    """(out [B, T, H], hT [B, H]) in float64."""
    xproj, wh, bhn = np.asarray(xproj, np.float64), np.asarray(wh, np.float64), np.asarray(bhn, np.float64)
    B, T, H3 = xproj.shape
    H = H3 // 3
    assert wh.shape == (3 * H, H) and bhn.shape == (H,)
    out = np.zeros((B, T, H))
    hT = np.zeros((B, H))
    for b in range(B):
        h = np.zeros(H) if h0 is None else np.asarray(h0[b], np.float64).copy()
        n_valid = T if lens is None else min(max(int(lens[b]), 0), T)
        for t in range(n_valid):
            rec = wh @ h
            x = xproj[b, t]
            r = sigmoid(x[:H] + rec[:H])
            z = sigmoid(x[H:2 * H] + rec[H:2 * H])
            n = np.tanh(x[2 * H:] + r * (rec[2 * H:] + bhn))
            h = (1.0 - z) * n + z * h
            out[b, t] = h
        hT[b] = h
    return out, hT


def make_case(H, T, B, seed):
    """Seeded float32 inputs of one recurrence: (xproj [B, T, 3H], Wh [3H, H] uniform in +-1/sqrt(H) like a PyTorch GRU, bhn [H], h0 [B, H] in (-1, 1))."""
    rng = np.random.default_rng(seed)
    s = 1.0 / np.sqrt(H)
    xproj = rng.standard_normal((B, T, 3 * H)).astype(np.float32)
    wh = rng.uniform(-s, s, (3 * H, H)).astype(np.float32)
    bhn = rng.uniform(-s, s, (H,)).astype(np.float32)
    h0 = rng.uniform(-0.9, 0.9, (B, H)).astype(np.float32)
    return xproj, wh, bhn, h0
