"""TEST INFRASTRUCTURE: a float64 numpy restatement of the S3 tokenizer v2 forward (codec/models/s3/model_v2.py) for right-padded BATCHES with lengths.

The reference's own model runs one un-padded sequence per call (its attention mask [B, 1, T] only broadcasts against [B, H, T, T] for B == 1 or B == H);
this helper states the module's meaning for a batch -- padded positions zeroed before each conv, masked as keys, zeroed into and out of the FSMN conv --
and ``tests/test_s3_cpu.py`` pins it to the reference's B == 1 runs stored in ``tests/golden/ref_s3_v2.npz``.  It is the source of truth at the published
size, where the reference's run is not stored.  Nothing under ``mlx_audio_amd/`` imports it."""
import math

import numpy as np

FSQ_SCALE = np.float32(0.9990000128746033)
EDGE = math.atanh(0.5 / float(FSQ_SCALE))   # |h_d| at which a digit changes


def synth_mel(seed: int, n_mels: int, frames: int) -> np.ndarray:
    """The synthetic log-mel-like input of the fixtures: 0.6 N(0, 1) + 0.3 sin(t / 7) per frame t, float32 [n_mels, frames], from the torch generator the
    seeded checkpoints use."""
    import torch

    g = torch.Generator().manual_seed(seed)
    x = 0.6 * torch.randn(n_mels, frames, generator=g) + 0.3 * torch.sin(torch.arange(frames, dtype=torch.float32) / 7.0)[None, :]
    return x.to(torch.float32).numpy()


def conv_len(n):
    return (n - 1) // 2 + 1


def _erf(x):
    import torch

    return torch.special.erf(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))).numpy()


def gelu(x):
    return 0.5 * x * (1.0 + _erf(x / math.sqrt(2.0)))


def _ln(x, w, b, eps):
    mu = x.mean(-1, keepdims=True)
    var = x.var(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * w + b


def _conv_s2(x, w, b):
    """x [B, T, Cin], w [Cout, 3, Cin], stride 2, pad 1 -> [B, conv_len(T), Cout]."""
    B, T, _ = x.shape
    To = conv_len(T)
    xp = np.zeros((B, 2 * To + 2, x.shape[2]))
    xp[:, 1:T + 1] = x
    y = np.zeros((B, To, w.shape[0]))
    for k in range(3):
        y += xp[:, k:k + 2 * To:2] @ w[:, k, :].T
    return y + b


def rope_tables(dim=64, end=2048, theta=10000.0):
    """precompute_freqs_cis in float32, as the reference builds them (the engine's tables are built the same way)."""
    freqs = (1.0 / (np.float32(theta) ** (np.arange(0, dim, 2)[: dim // 2].astype(np.float32) / np.float32(dim)))).astype(np.float32)
    f = np.outer(np.arange(end).astype(np.float32), freqs).astype(np.float32)
    return np.cos(f).astype(np.float32), np.sin(f).astype(np.float32)


def fsmn(v, taps, mask):
    """forward_fsmn: v [B, T, C], taps [C, K], mask [B, T] (1 = valid) -> [B, T, C]."""
    K = taps.shape[1]
    left = (K - 1) // 2
    vm = v * mask[:, :, None]
    T = v.shape[1]
    xp = np.zeros((v.shape[0], T + K - 1, v.shape[2]))
    xp[:, left:left + T] = vm
    y = np.zeros_like(vm)
    for j in range(K):
        y += xp[:, j:j + T] * taps[:, j]
    return (y + vm) * mask[:, :, None]


def fsq_codes(h):
    """h [..., 8] (any float type) -> int codes, the reference's float32 decision: round half to even of tanh(h) * 0.999 in float32."""
    t = (np.tanh(h.astype(np.float32)).astype(np.float32) * FSQ_SCALE).astype(np.float32)
    d = np.rint(t).astype(np.int64) + 1
    return (d * (3 ** np.arange(8))).sum(-1).astype(np.int32)


def margins(h):
    """min_d | |h_d| - EDGE | per frame."""
    return np.abs(np.abs(h.astype(np.float64)) - EDGE).min(-1)


def forward(w, n_state, n_head, n_layer, mel, mel_len):
    """w: name -> array (the reference's names, MLX layouts); mel [B, n_mels, T]; mel_len [B].  Returns dict(layers = [stem, block 0, ...] each
    [B, T', n_state], fsmn0 [B, T', n_state], h [B, T', 8], codes int32 [B, T'] (zero beyond code_len), code_len [B])."""
    W = {k: np.asarray(v, dtype=np.float64) for k, v in w.items()}
    mel = np.asarray(mel, dtype=np.float64)
    lens = np.asarray(mel_len, dtype=np.int64).reshape(-1)
    B, _, T = mel.shape
    m = (np.arange(T)[None, :] < lens[:, None]).astype(np.float64)
    x = gelu(_conv_s2(mel.transpose(0, 2, 1) * m[:, :, None], W["encoder.conv1.weight"], W["encoder.conv1.bias"]))
    lens = conv_len(lens)
    m = (np.arange(x.shape[1])[None, :] < lens[:, None]).astype(np.float64)
    x = gelu(_conv_s2(x * m[:, :, None], W["encoder.conv2.weight"], W["encoder.conv2.bias"]))
    lens = conv_len(lens)
    T2 = x.shape[1]
    m = (np.arange(T2)[None, :] < lens[:, None]).astype(np.float64)
    cos, sin = rope_tables()
    cos, sin = cos[:T2].astype(np.float64), sin[:T2].astype(np.float64)
    cosf, sinf = np.concatenate([cos, cos], -1)[None, :, None, :], np.concatenate([sin, sin], -1)[None, :, None, :]
    dh = n_state // n_head
    layers, fsmn0 = [x.copy()], None

    def rot(t):
        return np.concatenate([-t[..., dh // 2:], t[..., :dh // 2]], -1)

    for i in range(n_layer):
        p = f"encoder.blocks.{i}."
        hx = _ln(x, W[p + "attn_ln.weight"], W[p + "attn_ln.bias"], 1e-6)
        q = hx @ W[p + "attn.query.weight"].T + W[p + "attn.query.bias"]
        k = hx @ W[p + "attn.key.weight"].T
        v = hx @ W[p + "attn.value.weight"].T + W[p + "attn.value.bias"]
        q4, k4, v4 = (t.reshape(B, T2, n_head, dh) for t in (q, k, v))
        q4, k4 = q4 * cosf + rot(q4) * sinf, k4 * cosf + rot(k4) * sinf
        mem = fsmn(v, W[p + "attn.fsmn_block.weight"][:, :, 0], m)
        if i == 0:
            fsmn0 = mem.copy()
        sc = np.einsum("bqhd,bkhd->bhqk", q4, k4) * dh ** -0.5
        sc = np.where(m[:, None, None, :] > 0, sc, -np.inf)
        e = np.exp(sc - sc.max(-1, keepdims=True))
        att = np.einsum("bhqk,bkhd->bqhd", e / e.sum(-1, keepdims=True), v4).reshape(B, T2, n_state)
        x = x + att @ W[p + "attn.out.weight"].T + W[p + "attn.out.bias"] + mem
        hx = _ln(x, W[p + "mlp_ln.weight"], W[p + "mlp_ln.bias"], 1e-5)
        x = x + gelu(hx @ W[p + "mlp.layers.0.weight"].T + W[p + "mlp.layers.0.bias"]) @ W[p + "mlp.layers.2.weight"].T + W[p + "mlp.layers.2.bias"]
        layers.append(x.copy())
    h = x @ W["quantizer.fsq_codebook.project_down.weight"].T + W["quantizer.fsq_codebook.project_down.bias"]
    codes = fsq_codes(h) * (m > 0)
    return dict(layers=layers, fsmn0=fsmn0, h=h, codes=codes.astype(np.int32), code_len=lens.astype(np.int32))
