"""TEST INFRASTRUCTURE: a float64 restatement of the SenseVoice-Small forward (stt/models/sensevoice/sensevoice.py) for ONE un-padded clip, the two
fixture configs and the seeded inputs.  ``tests/test_sensevoice_cpu.py`` pins it to the reference's own runs stored in
``tests/golden/ref_sensevoice.npz``; it is the source of truth at the published widths, where the reference's run is not stored.  The fbank comes
from ``oracle/dsp_ref.compute_fbank_kaldi`` (float32, pinned to the reference elsewhere); everything behind it is float64.  Nothing under
``mlx_audio_amd/`` imports it."""
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CFG_A = dict(vocab_size=100, input_size=560, frontend_conf=dict(n_mels=80, lfr_m=7, lfr_n=6),
             encoder_conf=dict(output_size=128, attention_heads=2, linear_units=256, num_blocks=3, tp_blocks=2, kernel_size=5))
CFG_B = dict(vocab_size=300, input_size=200, frontend_conf=dict(n_mels=40, lfr_m=5, lfr_n=3),
             encoder_conf=dict(output_size=256, attention_heads=2, linear_units=512, num_blocks=2, tp_blocks=1, kernel_size=11, sanm_shfit=2))
CFG_WIDE = dict(vocab_size=25055, input_size=560, frontend_conf=dict(n_mels=80, lfr_m=7, lfr_n=6),   # the published widths, depth cut to 2 + 1
                encoder_conf=dict(output_size=512, attention_heads=4, linear_units=2048, num_blocks=2, tp_blocks=1, kernel_size=11))
FRAMES = (1, 5, 6, 7, 13, 300)   # fbank frames per clip: one frame is exactly 400 samples, every further one 160 more
CONFIGS = {"A": dict(cfg=CFG_A, seed_w=121, blank_bias=9.0, cmvn_seed=None, clips=tuple((n, 500 + i) for i, n in enumerate(FRAMES))),
           "B": dict(cfg=CFG_B, seed_w=122, blank_bias=11.0, cmvn_seed=77, clips=tuple((n, 520 + i) for i, n in enumerate(FRAMES)))}
HEAD_GAIN = 4.0
LANGUAGE, USE_ITN = "en", True


def make_config(cfg: dict):
    from mlx_audio_amd.stt.models.sensevoice import ModelConfig

    return ModelConfig.from_dict(dict(cfg, encoder_conf=dict(cfg["encoder_conf"]), frontend_conf=dict(cfg.get("frontend_conf", {}))))


def n_samples(frames: int) -> int:
    return 400 + 160 * (frames - 1)


def synth_audio(seed: int, frames: int) -> np.ndarray:
    """A waveform in [-1, 1] giving exactly ``frames`` fbank frames: 0.05 N(0, 1) + two drifting tones, float32."""
    g = torch.Generator().manual_seed(seed)
    n = n_samples(frames)
    t = torch.arange(n, dtype=torch.float64) / 16000.0
    f1, f2 = 180.0 + 40.0 * (seed % 7), 900.0 + 130.0 * (seed % 5)
    x = 0.05 * torch.randn(n, generator=g, dtype=torch.float64) + 0.2 * torch.sin(2 * math.pi * f1 * t * (1 + 0.3 * t)) + 0.1 * torch.sin(2 * math.pi * f2 * t)
    return x.to(torch.float32).numpy()


def make_cmvn(seed: int, width: int):
    """(means, istd) as an ``am.mvn`` holds them: the AddShift row (negative means, around -12) and the Rescale row (around 0.25), rounded to the six
    decimals the file is written with."""
    g = np.random.default_rng(seed)
    return [round(float(v), 6) for v in -12.0 + g.standard_normal(width)], [round(float(v), 6) for v in 0.25 * (1 + 0.2 * g.random(width))]


def am_mvn_text(means, istd) -> str:
    """A Kaldi-nnet ``am.mvn`` file in the layout FunASR ships."""
    n = len(means)
    row = lambda v: " ".join(f"{x:.6f}" for x in v)
    return (f"<Nnet> \n<Splice> {n} {n}\n[ 0 ]\n<AddShift> {n} {n} \n<LearnRateCoef> 0 [ {row(means)} ]\n<Rescale> {n} {n}\n"
            f"<LearnRateCoef> 0 [ {row(istd)} ]\n</Nnet> \n")


def token_list(vocab: int):
    """A ``tokens.json`` list: a blank, word pieces with and without the sentencepiece space marker."""
    return ["<blank>"] + [("▁" if i % 3 == 0 else "") + "".join(chr(97 + (i * k) % 26) for k in (1, 3))[: 1 + i % 2] for i in range(1, vocab)]


def fbank(audio: np.ndarray, cfg) -> np.ndarray:
    """``_compute_fbank`` (sensevoice.py:17-44): samples * 2^15, 25 ms hamming window every 10 ms, pre-emphasis 0.97, no dither, snip_edges."""
    from oracle import dsp_ref

    fc = cfg.frontend_conf
    return dsp_ref.compute_fbank_kaldi(np.asarray(audio, dtype=np.float32) * np.float32(1 << 15), sample_rate=fc.fs, win_len=int(fc.fs * fc.frame_length / 1000),
                                       win_inc=int(fc.fs * fc.frame_shift / 1000), num_mels=fc.n_mels, win_type=fc.window, preemphasis=0.97, dither=0.0,
                                       snip_edges=True, low_freq=20.0, high_freq=0.0)


def apply_lfr(feats: np.ndarray, m: int, n: int) -> np.ndarray:
    """``_apply_lfr`` (sensevoice.py:47-72) as an index table: output frame i, block j reads frame clamp(i n + j - (m - 1) / 2, 0, T - 1)."""
    T = feats.shape[0]
    idx = np.clip(np.arange(math.ceil(T / n))[:, None] * n + np.arange(m)[None, :] - (m - 1) // 2, 0, T - 1)
    return feats[idx].reshape(idx.shape[0], -1)


def positions(rows: int, width: int) -> np.ndarray:
    """``SinusoidalPositionEncoder`` (sensevoice.py:106-122) in float64: positions from 1, sines then cosines."""
    half = width // 2
    inv = np.exp(np.arange(half, dtype=np.float64) * -(math.log(10000) / (half - 1)))
    t = np.arange(1, rows + 1, dtype=np.float64)[:, None] * inv[None, :]
    return np.concatenate([np.sin(t), np.cos(t)], axis=1)


def qids(language: str, use_itn: bool):
    """sensevoice.py:397-433: rows [language, event (1), emotion (2), textnorm]."""
    lid = {"auto": 0, "zh": 3, "en": 4, "yue": 7, "ja": 11, "ko": 12, "nospeech": 13}.get(language, 0)
    return [lid, 1, 2, 14 if use_itn else 15]


def assemble(cfg, W, fb: np.ndarray, cmvn, language=LANGUAGE, use_itn=USE_ITN) -> np.ndarray:
    """fbank [T, n_mels] -> the encoder's input after the scale and the position term (sensevoice.py:390-395,426-433,322-324), float64."""
    fc = cfg.frontend_conf
    x = apply_lfr(np.asarray(fb, dtype=np.float64), fc.lfr_m, fc.lfr_n)
    if cmvn is not None:
        x = (x + np.asarray(cmvn[0], dtype=np.float32).astype(np.float64)) * np.asarray(cmvn[1], dtype=np.float32).astype(np.float64)
    return assemble_stacked(cfg, W, x, language, use_itn)


def assemble_stacked(cfg, W, feats: np.ndarray, language=LANGUAGE, use_itn=USE_ITN) -> np.ndarray:
    """Stacked, normalised features [T, input_size] -> the encoder's input: the query rows in front, * sqrt(d), + positions."""
    x = np.concatenate([torch.as_tensor(W["embed.weight"]).double().numpy()[qids(language, use_itn)], np.asarray(feats, dtype=np.float64)], axis=0)
    return x * math.sqrt(cfg.encoder_conf.output_size) + positions(x.shape[0], x.shape[1])


def _ln(x, w, b, eps=1e-5):
    mu = x.mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(x.var(-1, unbiased=False, keepdim=True) + eps) * w + b


def fsmn(v: torch.Tensor, taps: torch.Tensor, shift: int) -> torch.Tensor:
    """``_forward_fsmn`` (sensevoice.py:164-177), literally: pad (left, right) = ((K - 1) / 2 + shift, K - 1 - left), depthwise conv, + v.  v [T, C]."""
    K = taps.shape[1]
    left = (K - 1) // 2 + shift
    xp = torch.nn.functional.pad(v.t()[None], (left, K - 1 - left))
    return torch.nn.functional.conv1d(xp, taps[:, None, :], groups=taps.shape[0])[0].t() + v


def encode(cfg, weights, x) -> dict:
    """The encoder and the head on one assembled input [R, input_size] (sensevoice.py:135-237,322-338,436-437), float64: dict(layers [n, R, d],
    attn0, hidden, logits, logp, ids, gap)."""
    from mlx_audio_amd.stt.models.sensevoice.sensevoice import layer_names

    enc = cfg.encoder_conf
    W = {k: torch.as_tensor(v).double() for k, v in weights.items()}
    lin = lambda x, n: x @ W[n + ".weight"].t() + W[n + ".bias"]
    d, H = enc.output_size, enc.attention_heads
    dh = d // H
    x = torch.as_tensor(x).double()
    R = x.shape[0]
    out = dict(layers=[])
    for i, (p, din) in enumerate(layer_names(cfg)):
        if i == enc.num_blocks:
            x = _ln(x, W["encoder.after_norm.weight"], W["encoder.after_norm.bias"])
        h = _ln(x, W[p + "norm1.weight"], W[p + "norm1.bias"])
        q, k, v = lin(h, p + "self_attn.linear_q_k_v").split(d, dim=-1)
        mem = fsmn(v, W[p + "self_attn.fsmn_block.weight"][:, :, 0], enc.sanm_shift)
        qh, kh, vh = (t.reshape(R, H, dh).transpose(0, 1) for t in (q, k, v))
        att = torch.softmax((qh * dh ** -0.5) @ kh.transpose(1, 2), -1) @ vh
        att = lin(att.transpose(0, 1).reshape(R, d), p + "self_attn.linear_out") + mem
        if i == 0:
            out["attn0"] = att
        x = x + att if din == d else att
        x = x + lin(torch.relu(lin(_ln(x, W[p + "norm2.weight"], W[p + "norm2.bias"]), p + "feed_forward.w_1")), p + "feed_forward.w_2")
        out["layers"].append(x.clone())
    if enc.tp_blocks == 0:
        x = _ln(x, W["encoder.after_norm.weight"], W["encoder.after_norm.bias"])
    x = _ln(x, W["encoder.tp_norm.weight"], W["encoder.tp_norm.bias"])
    logits = lin(x, "ctc_lo")
    logp = torch.log_softmax(logits, -1)
    top = torch.topk(logp, 2, dim=-1).values
    out.update(layers=torch.stack(out["layers"]), hidden=x, logits=logits, logp=logp, ids=logp.argmax(-1), gap=top[:, 0] - top[:, 1])
    return out


def collapse(ids, blank: int = 0, return_frames: bool = False):
    """``_greedy_ctc_decode`` (sensevoice.py:450-463): drop repeats of the previous id, then blanks."""
    toks, frames, prev = [], [], None
    for t, i in enumerate(int(v) for v in ids):
        if i != prev:
            if i != blank:
                toks.append(i)
                frames.append(t)
            prev = i
    return (toks, frames) if return_frames else toks


def forward(cfg, weights, audio, cmvn=None, language=LANGUAGE, use_itn=USE_ITN) -> dict:
    W = {k: torch.as_tensor(v) for k, v in weights.items()}
    x = assemble(cfg, W, fbank(audio, cfg), cmvn, language, use_itn)
    out = encode(cfg, weights, x)
    out.update(x=x, tokens=collapse(out["ids"][4:].tolist()))
    return out


def load_models(meta) -> dict:
    """tag -> (config, weights, [audio], cmvn or None) of the fixture's configs, regenerated from their seeds."""
    from mlx_audio_amd.stt.models.sensevoice import make_sensevoice_weights

    out = {}
    for tag, c in meta["configs"].items():
        want = CONFIGS[tag]
        assert c["cfg"] == want["cfg"] and [tuple(x) for x in c["clips"]] == list(want["clips"]) and c["seed_w"] == want["seed_w"]
        cfg = make_config(c["cfg"])
        w = make_sensevoice_weights(cfg, c["seed_w"], head_gain=HEAD_GAIN, blank_bias=c["blank_bias"])
        cmvn = None if want["cmvn_seed"] is None else make_cmvn(want["cmvn_seed"], cfg.input_size)
        out[tag] = (cfg, w, [synth_audio(seed, frames) for frames, seed in c["clips"]], cmvn)
    return out
