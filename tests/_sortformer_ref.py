"""TEST INFRASTRUCTURE: a float64 torch restatement of the Sortformer forward (vad/models/sortformer/sortformer.py) for ONE un-padded clip, under the
reference's own parameter names, plus the fixture configs and the seeded inputs.  ``tests/test_sortformer_cpu.py`` pins it to the reference's own
runs stored in ``tests/golden/ref_sortformer.npz``; it is the source of truth at the published widths, where the reference's run is not stored.  The
attention restates the module's order (scale q, scores, additive -1e4 mask, softmax, @ v), the position term goes through the literal pad / reshape
``rel_shift``.  Nothing under ``mlx_audio_amd/`` imports it."""
import math

import numpy as np
import torch

from _parakeet_ref import rel_shift_literal, synth_mel  # noqa: F401

FC_A = dict(num_mel_bins=16, hidden_size=128, num_attention_heads=2, num_key_value_heads=2, num_hidden_layers=2, intermediate_size=512, conv_kernel_size=9,
            subsampling_conv_channels=32)
TF_A = dict(d_model=48, encoder_attention_heads=2, encoder_layers=2, encoder_ffn_dim=96, max_source_positions=256)
CONFIGS = {
    "A": dict(fc=FC_A, tf=TF_A, seed_w=91, head_gain=6.0, head_bias=-3.0, clips=((1601, 401), (203, 402), (41, 403), (9, 404))),   # (mel frames, mel seed)
    "B": dict(fc=dict(FC_A, attention_bias=False), tf=dict(TF_A, d_model=64, encoder_attention_heads=8, k_proj_bias=True), seed_w=92, head_gain=6.0,
              head_bias=-3.0, clips=((203, 411), (64, 412))),
}
# the published widths (diar_sortformer_4spk-v1), two layers each
FC_WIDE = dict(num_mel_bins=80, hidden_size=512, num_attention_heads=8, num_key_value_heads=8, num_hidden_layers=2, intermediate_size=2048, conv_kernel_size=9,
               subsampling_conv_channels=256)
TF_WIDE = dict(d_model=192, encoder_attention_heads=8, encoder_layers=2, encoder_ffn_dim=768, max_source_positions=1500)
SEGMENT_SETTINGS = ((0.5, 0.0, 0.0), (0.4, 0.2, 0.17))   # (threshold, min_duration, merge_gap)
STREAM = dict(seed=431, chunks=8, chunk_samples=10240, spkcache_max=16, fifo_max=16)   # 8 chunks of 0.64 s: 65 mel frames, 9 diarization frames each
GENERATE = dict(seed=432, seconds=6.0)


def config_dict(fc: dict, tf: dict, n_spk: int = 4) -> dict:
    """A ``config.json`` for ``ModelConfig.from_dict``."""
    return dict(model_type="sortformer", num_speakers=n_spk, fc_encoder_config=dict(fc), tf_encoder_config=dict(tf),
                modules_config=dict(num_speakers=n_spk, fc_d_model=fc["hidden_size"], tf_d_model=tf["d_model"]),
                processor_config=dict(feature_size=fc["num_mel_bins"]))


def make_config(fc: dict, tf: dict, n_spk: int = 4):
    from mlx_audio_amd.vad.models.sortformer import ModelConfig

    return ModelConfig.from_dict(config_dict(fc, tf, n_spk))


def synth_wave(seed: int, n: int, sr: int = 16000) -> np.ndarray:
    """A seeded waveform with speech-like level changes: three tones under slow envelopes plus noise, float32 [n]."""
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(n, dtype=torch.float64) / sr
    x = 0.02 * torch.randn(n, generator=g, dtype=torch.float64)
    for f, rate, ph in ((180.0, 0.9, 0.0), (410.0, 1.7, 1.3), (1250.0, 0.6, 2.1)):
        x = x + 0.3 * torch.sin(2 * math.pi * f * t) * torch.clamp(torch.sin(2 * math.pi * rate * t + ph), min=0.0)
    return x.to(torch.float32).numpy()


def _ln(x, w, b, eps=1e-5):
    mu = x.mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(x.var(-1, unbiased=False, keepdim=True) + eps) * w + b


def pre_encode(config, W, feats):
    """ConvSubsampling (sortformer.py:176-203) on features [n_mels, T] -> UNSCALED embeddings [T', hidden], float64."""
    fc = config.fc_encoder_config
    C = fc.subsampling_conv_channels
    p = "fc_encoder.subsampling."
    conv2 = lambda x, n, **k: torch.nn.functional.conv2d(x, W[p + n + ".weight"].permute(0, 3, 1, 2), W[p + n + ".bias"], **k)
    y = torch.relu(conv2(feats.t()[None, None], "layers_0", stride=2, padding=1))
    y = torch.relu(conv2(conv2(y, "layers_2", stride=2, padding=1, groups=C), "layers_3"))
    y = torch.relu(conv2(conv2(y, "layers_5", stride=2, padding=1, groups=C), "layers_6"))
    y = y[0].permute(1, 0, 2).reshape(y.shape[2], -1)   # [T', C * F'], column c * F' + f
    return y @ W[p + "linear.weight"].t() + W[p + "linear.bias"]


def encode(config, W, embs) -> dict:
    """``FastConformerEncoder.encode`` + the rest of ``Model.__call__`` on UNSCALED embeddings [T, hidden] of one clip, float64:
    dict(fc_layers, encoder_proj, tf_layers, logits, preds)."""
    from mlx_audio_amd.stt.models.parakeet.conformer import rel_positions

    fc, tf = config.fc_encoder_config, config.tf_encoder_config
    g = lambda n: W.get(n)
    lin = lambda x, n: x @ W[n + ".weight"].reshape(W[n + ".weight"].shape[0], -1).t() + (g(n + ".bias") if g(n + ".bias") is not None else 0.0)
    x = embs * (fc.hidden_size ** 0.5) if fc.scale_input else embs
    T, d, H = x.shape[0], fc.hidden_size, fc.num_attention_heads
    dh = d // H
    pos = rel_positions(T, d).double()
    out = dict(fc_layers=[])
    for i in range(fc.num_hidden_layers):
        p = f"fc_encoder.layers.{i}."
        ln = lambda x, n: _ln(x, W[p + n + ".weight"], W[p + n + ".bias"])
        ff = lambda x, n: lin(torch.nn.functional.silu(lin(x, p + n + ".linear1")), p + n + ".linear2")
        x = x + 0.5 * ff(ln(x, "norm_feed_forward1"), "feed_forward1")
        h = ln(x, "norm_self_att")
        q, k, v = (lin(h, p + f"self_attn.{n}_proj").reshape(T, H, dh).transpose(0, 1) for n in "qkv")
        pp = lin(pos, p + "self_attn.relative_k_proj").reshape(2 * T - 1, H, dh).transpose(0, 1)
        ac = (q + W[p + "self_attn.bias_u"][:, None, :]) @ k.transpose(1, 2)
        bd = rel_shift_literal((q + W[p + "self_attn.bias_v"][:, None, :]) @ pp.transpose(1, 2))[:, :, :T]
        x = x + lin((torch.softmax((ac + bd) / math.sqrt(dh), -1) @ v).transpose(0, 1).reshape(T, d), p + "self_attn.o_proj")
        h = lin(ln(x, "norm_conv"), p + "conv.pointwise_conv1")
        h = h[:, :d] * torch.sigmoid(h[:, d:])
        K = fc.conv_kernel_size
        h = torch.nn.functional.conv1d(h.t()[None], W[p + "conv.depthwise_conv.weight"].permute(0, 2, 1), W[p + "conv.depthwise_conv.bias"],
                                       padding=(K - 1) // 2, groups=d)[0].t()
        bn = lambda n: W[p + "conv.norm." + n]
        h = (h - bn("running_mean")) / torch.sqrt(bn("running_var") + 1e-5) * bn("weight") + bn("bias")
        x = x + lin(torch.nn.functional.silu(h), p + "conv.pointwise_conv2")
        x = x + 0.5 * ff(ln(x, "norm_feed_forward2"), "feed_forward2")
        x = ln(x, "norm_out")
        out["fc_layers"].append(x.clone())
    out["fc_layers"] = torch.stack(out["fc_layers"])
    # ---- Model.__call__ behind the FastConformer encoder (797-809), one un-padded clip: the mask is all valid
    x = lin(x, "sortformer_modules.encoder_proj")
    out["encoder_proj"] = x.clone()
    d, H = tf.d_model, tf.encoder_attention_heads
    dh = d // H
    x = x + W["tf_encoder.embed_positions.weight"][:T]
    mask = torch.zeros(T, dtype=torch.float64) * -1e4
    out["tf_layers"] = []
    for i in range(tf.encoder_layers):
        p = f"tf_encoder.layers.{i}."
        q, k, v = (lin(x, p + f"self_attn.{n}_proj").reshape(T, H, dh).transpose(0, 1) for n in "qkv")
        scores = (q * dh ** -0.5) @ k.transpose(1, 2) + mask
        a = lin((torch.softmax(scores, -1) @ v).transpose(0, 1).reshape(T, d), p + "self_attn.out_proj")
        x = _ln(x + a, W[p + "self_attn_layer_norm.weight"], W[p + "self_attn_layer_norm.bias"], tf.layer_norm_eps)
        h = lin(torch.relu(lin(x, p + "fc1")), p + "fc2")
        x = _ln(x + h, W[p + "final_layer_norm.weight"], W[p + "final_layer_norm.bias"], tf.layer_norm_eps)
        out["tf_layers"].append(x.clone())
    out["tf_layers"] = torch.stack(out["tf_layers"])
    h = torch.relu(lin(torch.relu(x), "sortformer_modules.first_hidden_to_hidden"))
    out["logits"] = lin(h, "sortformer_modules.single_hidden_to_spks")
    out["preds"] = torch.sigmoid(out["logits"])
    return out


def forward(config, weights, feats) -> dict:
    """One clip alone: features [n_mels, T] -> ``encode``'s dict plus ``pre_encode`` (the unscaled embeddings)."""
    W = {k: torch.as_tensor(v).double() for k, v in weights.items()}
    embs = pre_encode(config, W, torch.as_tensor(feats).double())
    out = encode(config, W, embs)
    out["pre_encode"] = embs
    return out


def segments_list(segments) -> list:
    """``DiarizationSegment``s (the reference's or this package's) as plain data."""
    return [[float(s.start), float(s.end), int(s.speaker)] for s in segments]


def same_segments(got: list, want: list) -> bool:
    return len(got) == len(want) and all(g[2] == w[2] and abs(g[0] - w[0]) < 1e-9 and abs(g[1] - w[1]) < 1e-9 for g, w in zip(got, want))


def load_models(meta) -> dict:
    """tag -> (config, weights, [features [n_mels, T]]) of the fixture's configs, regenerated from their seeds."""
    from mlx_audio_amd.vad.models.sortformer import make_sortformer_weights

    out = {}
    for tag, c in meta["configs"].items():
        k = CONFIGS[tag]
        assert c["fc"] == k["fc"] and c["tf"] == k["tf"] and [tuple(x) for x in c["clips"]] == list(k["clips"])
        cfg = make_config(c["fc"], c["tf"])
        w = make_sortformer_weights(cfg, c["seed_w"], head_gain=c["head_gain"], head_bias=c["head_bias"])
        out[tag] = (cfg, w, [np.ascontiguousarray(synth_mel(seed, c["fc"]["num_mel_bins"], frames).T) for frames, seed in c["clips"]])
    return out


def pad_batch(feats):
    """Right-padded [B, n_mels, T] batch and the items' lengths."""
    T = max(f.shape[1] for f in feats)
    batch = torch.zeros(len(feats), feats[0].shape[0], T)
    for i, f in enumerate(feats):
        batch[i, :, :f.shape[1]] = torch.from_numpy(f)
    return batch, [f.shape[1] for f in feats]
