"""TEST INFRASTRUCTURE: the Moonshine test configurations, the seeded clips, and a float64 restatement of the reference's forward pass
(stt/models/moonshine/moonshine.py) in torch on the CPU, written from the module's lines (valid strided convs, GroupNorm(1, d), weight-only
LayerNorm, interleaved partial rotary embedding from the float32 tables, additive causal mask with a cache prefix, the split / silu decoder MLP).
Nothing under ``mlx_audio_amd/`` imports it."""
import math

import numpy as np
import torch

from mlx_audio_amd import ops
from mlx_audio_amd.stt.models.moonshine import ModelConfig

F64 = torch.float64
MAX_TOKENS = 24
CONFIGS = {
    "A": dict(cfg=dict(vocab_size=100, hidden_size=144, intermediate_size=288, encoder_num_hidden_layers=2, decoder_num_hidden_layers=2,
                       encoder_num_attention_heads=4, decoder_num_attention_heads=4), seed_w=11, logit_gain=6.0, eos_gain=1.6,
              clips=[(895, 101), (4800, 102), (16000, 103), (48000, 104)]),
    "B": dict(cfg=dict(vocab_size=97, hidden_size=208, intermediate_size=256, encoder_num_hidden_layers=2, decoder_num_hidden_layers=2,
                       encoder_num_attention_heads=4, decoder_num_attention_heads=4, encoder_num_key_value_heads=2, tie_word_embeddings=False),
              seed_w=12, logit_gain=6.0, eos_gain=1.6, clips=[(895, 201), (5000, 202), (16000, 203), (48000, 204)]),
}
FORCED = [1, 17, 5, 40, 9]   # the teacher-forced decoder call: T = 3, then T = 2 over the cache


def make_config(d: dict) -> ModelConfig:
    return ModelConfig.from_dict(d)


def synth_audio(seed: int, n: int) -> np.ndarray:
    """A few drifting tones plus noise in [-1, 1], float32."""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64) / 16000.0
    x = 0.05 * rng.standard_normal(n)
    for _ in range(4):
        f, a, ph = rng.uniform(80, 3000), rng.uniform(0.05, 0.25), rng.uniform(0, 2 * np.pi)
        x += a * np.sin(2 * np.pi * f * t + ph + 3.0 * np.sin(2 * np.pi * rng.uniform(0.5, 3.0) * t))
    return np.clip(x, -1, 1).astype(np.float32)


def _ln(x, w):
    m, v = x.mean(-1, keepdim=True), x.var(-1, unbiased=False, keepdim=True)
    return (x - m) / torch.sqrt(v + 1e-5) * w


def _lin(w, name, x):
    y = x @ w[name + ".weight"].T
    return y + w[name + ".bias"] if name + ".bias" in w else y


def _rope(x, pos0, rot, theta):
    """x [H, T, dh]: interleaved pairs on the first rot channels, angles from the float32 tables."""
    T = x.shape[1]
    cos, sin = (t.double().repeat_interleave(2, dim=1)[None] for t in ops.moonshine_rope_tables(rot, T, base=theta, pos0=pos0))
    xr = x[..., :rot]
    rh = torch.stack([-xr[..., 1::2], xr[..., 0::2]], dim=-1).reshape(xr.shape)
    return torch.cat([xr * cos + rh * sin, x[..., rot:]], dim=-1)


def _attn(w, p, x, src, H, KH, c, *, rope_pos=None, causal=False):
    """x [T, d] queries, src [S, d] keys / values (x itself for self-attention) -> (o_proj output [T, d])."""
    T, d = x.shape
    S, dh = src.shape[0], d // H
    q = _lin(w, p + ".q_proj", x).reshape(T, H, dh).transpose(0, 1)
    k = _lin(w, p + ".k_proj", src).reshape(S, KH, dh).transpose(0, 1)
    v = _lin(w, p + ".v_proj", src).reshape(S, KH, dh).transpose(0, 1)
    if rope_pos is not None:
        r = int(dh * c.partial_rotary_factor)
        r -= r % 2
        q, k = _rope(q, rope_pos, r, c.rope_theta), _rope(k, rope_pos, r, c.rope_theta)
    k, v = k.repeat_interleave(H // KH, 0), v.repeat_interleave(H // KH, 0)
    s = (q * dh ** -0.5) @ k.transpose(1, 2)
    if causal:
        s = s + torch.triu(torch.full((T, S), -1e9, dtype=F64), diagonal=1 + S - T)
    o = (torch.softmax(s, -1) @ v).transpose(0, 1).reshape(T, H * dh)
    return o @ w[p + ".o_proj.weight"].T


def _conv_valid(x, wt, b, stride):
    """x [T, C], wt [C_out, K, C] (MLX layout) -> [T', C_out]."""
    y = torch.nn.functional.conv1d(x.T[None], wt.permute(0, 2, 1), b, stride=stride)
    return y[0].T


def encoder64(w, c, audio, stages=None):
    x = torch.as_tensor(audio, dtype=F64)[:, None]
    x = torch.tanh(_conv_valid(x, w["encoder.conv1.weight"], None, 64))
    if stages is not None:
        stages["tanh"] = x
    x = (x - x.mean()) / torch.sqrt(x.var(unbiased=False) + 1e-5) * w["encoder.groupnorm.weight"] + w["encoder.groupnorm.bias"]
    if stages is not None:
        stages["gn"] = x
    x = torch.nn.functional.gelu(_conv_valid(x, w["encoder.conv2.weight"], w["encoder.conv2.bias"], 3))
    if stages is not None:
        stages["conv2"] = x
    x = torch.nn.functional.gelu(_conv_valid(x, w["encoder.conv3.weight"], w["encoder.conv3.bias"], 2))
    if stages is not None:
        stages["conv3"], stages["layers"] = x, []
    H, KH = c.encoder_num_attention_heads, c.encoder_num_key_value_heads
    for i in range(c.encoder_num_hidden_layers):
        p = f"encoder.layers.{i}"
        h = _ln(x, w[p + ".input_layernorm.weight"])
        a = _attn(w, p + ".self_attn", h, h, H, KH, c, rope_pos=0)
        if stages is not None and i == 0:
            stages["attn0"] = a
        x = x + a
        h = _ln(x, w[p + ".post_attention_layernorm.weight"])
        x = x + _lin(w, p + ".mlp.fc2", torch.nn.functional.gelu(_lin(w, p + ".mlp.fc1", h)))
        if stages is not None:
            stages["layers"].append(x)
    return _ln(x, w["encoder.layer_norm.weight"])


def decoder64(w, c, tokens, enc):
    """All positions of ``tokens`` at once under the causal mask (what the cached calls compute position by position) -> hidden [T, d]."""
    H, KH = c.decoder_num_attention_heads, c.decoder_num_key_value_heads
    x = w["decoder.embed_tokens.weight"][torch.as_tensor(tokens).long()]
    for i in range(c.decoder_num_hidden_layers):
        p = f"decoder.layers.{i}"
        h = _ln(x, w[p + ".input_layernorm.weight"])
        x = x + _attn(w, p + ".self_attn", h, h, H, KH, c, rope_pos=0, causal=True)
        x = x + _attn(w, p + ".encoder_attn", _ln(x, w[p + ".post_attention_layernorm.weight"]), enc, H, KH, c)
        y = _lin(w, p + ".mlp.fc1", _ln(x, w[p + ".final_layernorm.weight"]))
        u, gate = y.chunk(2, dim=-1)
        x = x + _lin(w, p + ".mlp.fc2", torch.nn.functional.silu(gate) * u)
    return _ln(x, w["decoder.norm.weight"])


def logits64(w, c, hidden):
    return hidden @ (w["decoder.embed_tokens.weight"] if c.tie_word_embeddings else w["proj_out.weight"]).T


def greedy64(w, c, enc, max_tokens=MAX_TOKENS):
    """(tokens, per-step logits rows, per-step top-2 gaps), the reference's loop: a step that picks EOS ends it without appending."""
    toks, rows, gaps = [c.decoder_start_token_id], [], []
    for _ in range(max_tokens):
        lg = logits64(w, c, decoder64(w, c, toks, enc)[-1])
        top = torch.sort(lg).values
        rows.append(lg)
        gaps.append(float(top[-1] - top[-2]))
        nxt = int(lg.argmax())
        if nxt == c.eos_token_id:
            break
        toks.append(nxt)
    return toks[1:], torch.stack(rows), gaps


def to64(weights):
    return {k: torch.as_tensor(v).double() for k, v in weights.items()}


# ---------------------------------------------------------------------------------------------------- shared by the CPU and GPU test files
def load_fixtures():
    import json
    import os

    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    with open(os.path.join(here, "ref_moonshine.json")) as f:
        return np.load(os.path.join(here, "ref_moonshine.npz")), json.load(f)


def clip_audio(z, tag, i):
    n, seed = CONFIGS[tag]["clips"][i]
    audio = synth_audio(seed, n)
    s = z[f"{tag}{i}_audiosum"]
    assert audio.astype(np.float64).sum() == s[0] and (audio.astype(np.float64) ** 2).sum() == s[1], "the regenerated clip is not the stored one"
    return audio


def check_clip(model, z, meta, tag, i, bar, family, report=None):
    """One stored clip through ``model``: every stage, the greedy decisions with their logits rows, the T = 3 then T = 2 decoder call, text and
    counters.  Errors are max |got - want| / max |want| per tensor, asserted below ``bar``; returns name -> error."""
    import _margin

    c = model.config
    audio = clip_audio(z, tag, i)
    out, frames, st = model.encode(audio, return_stages=True)
    errs = {}

    def cmp(name, got, rows_key):
        want = torch.from_numpy(z[f"{tag}{i}_{name}"]).double()
        g = got.detach().double().cpu()[torch.from_numpy(z[f"{tag}{i}_{rows_key}_rows"]).long()]
        assert g.shape == want.shape, (name, g.shape, want.shape)
        errs[name] = float((g - want).abs().max() / want.abs().max())
        assert errs[name] < bar, (tag, i, name, errs[name])

    for name in ("tanh", "gn", "conv2", "conv3", "attn0"):
        cmp(name, st[name][0], name)
    for l, x in enumerate(st["layers"]):
        cmp(f"layer{l}", x[0], "enc")
    cmp("enc", out[0], "enc")
    dec = meta["configs"][tag]["decode"][i]
    toks, trace = model.decode_greedy(out, frames, max_tokens=meta["max_tokens"], return_trace=True)
    exp = dec["tokens"] + ([c.eos_token_id] if dec["eos"] else [])
    want_rows, gaps = z[f"{tag}{i}_logits"], z[f"{tag}{i}_gap"]
    got_ids = [int(r[0].argmax()) for r in trace["logits"]]
    assert len(got_ids) == len(exp) == len(gaps), (len(got_ids), len(exp))
    assert _margin.walk(family, got_ids, exp, gaps, where=(tag, i)) == len(exp)
    e = max(float((r[0].double() - torch.from_numpy(w_).double()).abs().max() / np.abs(w_).max()) for r, w_ in zip(trace["logits"], want_rows))
    g = max(abs(float(a[0]) - float(b)) for a, b in zip(trace["gap"], gaps))
    errs["logits"], errs["gap_abs"] = e, g
    assert e < bar, (tag, i, "logits", e)
    assert toks[0] == dec["tokens"] and (len(toks[0]) == meta["max_tokens"]) == (not dec["eos"])
    forced = meta["forced"]
    h1, cache = model(torch.tensor([forced[:3]]), out, None, frames=frames)
    h2, _ = model(torch.tensor([forced[3:]]), out, cache)
    want = torch.from_numpy(z[f"{tag}{i}_forced"]).double()
    errs["forced"] = float((torch.cat([h1[0], h2[0]]).double().cpu() - want).abs().max() / want.abs().max())
    assert errs["forced"] < bar, (tag, i, "forced", errs["forced"])
    res = model.generate(audio, max_tokens=meta["max_tokens"], language="en", generation_stream=None)
    assert res.text == dec["text"] and res.segments == dec["segments"]
    assert (res.prompt_tokens, res.generation_tokens, res.total_tokens) == (dec["prompt_tokens"], dec["generation_tokens"], dec["total_tokens"])
    if report is not None:
        report(f"moonshine {tag}{i} ({len(audio)} samples, {frames[0]} frames): " + ", ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    return errs
