"""TEST INFRASTRUCTURE: a float64 torch restatement of the Parakeet CTC forward (stt/models/parakeet/conformer.py, attention.py, ctc.py) for ONE un-padded
clip, the two fixture configs and the seeded inputs.  ``tests/test_parakeet_cpu.py`` pins it to the reference's own runs stored in
``tests/golden/ref_parakeet_ctc.npz``; it is the source of truth at the published widths, where the reference's run is not stored.  The position term goes
through the literal pad / reshape ``rel_shift``, not the index formula the kernel uses.  Nothing under ``mlx_audio_amd/`` imports it."""
import math

import numpy as np
import torch

ENC_A = dict(feat_in=16, n_layers=2, d_model=128, n_heads=2, ff_expansion_factor=4, subsampling_factor=8, self_attention_model="rel_pos",
             subsampling="dw_striding", conv_kernel_size=9, subsampling_conv_channels=32, pos_emb_max_len=5000)
ENC_B = dict(feat_in=80, n_layers=1, d_model=256, n_heads=2, ff_expansion_factor=4, subsampling_factor=8, self_attention_model="rel_pos",
             subsampling="dw_striding", conv_kernel_size=31, subsampling_conv_channels=32, pos_emb_max_len=5000, xscaling=True, use_bias=False)
ENC_WIDE = dict(feat_in=128, n_layers=2, d_model=1024, n_heads=8, ff_expansion_factor=4, subsampling_factor=8, self_attention_model="rel_pos",
                subsampling="dw_striding", conv_kernel_size=9, subsampling_conv_channels=256, pos_emb_max_len=5000)   # the published 0.6 B widths, two layers
VOCAB = ["<unk>", "▁the", "▁a", "s", ".", "▁cat", "▁dog", "ing", "?", "▁on", "e", "▁mat", "!", "t", "▁sat", "<|endoftext|>", "▁it", "r", "▁is", "n", "'", "▁so", "ed", "▁we"]
CONFIGS = {"A": dict(enc=ENC_A, seed_w=81, blank_bias=5.5, clips=((1601, 301), (203, 302), (41, 303), (9, 304), (1, 305))),   # (mel frames, mel seed)
           "B": dict(enc=ENC_B, seed_w=82, blank_bias=4.0, clips=((203, 311), (64, 312)))}
HEAD_GAIN = 4.0


def config_dict(enc: dict) -> dict:
    """A NeMo-style ``config.json`` for ``ParakeetCTC.from_config``."""
    return dict(target="nemo.collections.asr.models.ctc_bpe_models.EncDecCTCModelBPE",
                preprocessor=dict(sample_rate=16000, normalize="per_feature", window_size=0.025, window_stride=0.01, window="hann", features=enc["feat_in"],
                                  n_fft=512, dither=0.0),
                encoder=dict(enc), decoder=dict(feat_in=enc["d_model"], num_classes=len(VOCAB), vocabulary=list(VOCAB)), decoding=dict(greedy=None))


def make_args(enc: dict):
    from mlx_audio_amd.stt.models.parakeet.parakeet import ParakeetCTCArgs, _from_dict

    return _from_dict(ParakeetCTCArgs, config_dict(enc))


def synth_mel(seed: int, feat: int, frames: int) -> np.ndarray:
    """The synthetic normalised-log-mel-like input of the fixtures: 0.8 N(0, 1) + 0.5 sin(t / 9 + f / 5), float32 [frames, feat]."""
    g = torch.Generator().manual_seed(seed)
    t, f = torch.arange(frames, dtype=torch.float32)[:, None], torch.arange(feat, dtype=torch.float32)[None, :]
    return (0.8 * torch.randn(frames, feat, generator=g) + 0.5 * torch.sin(t / 9.0 + f / 5.0)).to(torch.float32).numpy()


def rel_shift_literal(x):
    """attention.py:82-91: pad one column on the left, reshape, drop a row, reshape.  [H, Tq, pos_len]."""
    H, Tq, pos_len = x.shape
    x = torch.nn.functional.pad(x, (1, 0)).reshape(H, pos_len + 1, Tq)[:, 1:, :]
    return x.reshape(H, Tq, pos_len)


def _ln(x, w, b, eps=1e-5):
    mu = x.mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(x.var(-1, unbiased=False, keepdim=True) + eps) * w + b


def forward(args, weights, mel) -> dict:
    """One clip alone, float64: dict(pre_encode [T', d], layers [n, T', d], attn0, conv0 (layer 0's module outputs), logp [T', V + 1], ids, gap, out_len)."""
    from mlx_audio_amd.stt.models.parakeet.conformer import n_stages, rel_positions

    a = args.encoder
    W = {k: torch.as_tensor(v).double() for k, v in weights.items()}
    g = lambda n: W.get(n)
    lin = lambda x, n: x @ W[n + ".weight"].reshape(W[n + ".weight"].shape[0], -1).t() + (g(n + ".bias") if g(n + ".bias") is not None else 0.0)
    x = torch.as_tensor(mel).double()
    if a.subsampling_factor > 1:
        conv2 = lambda x, n, **k: torch.nn.functional.conv2d(x, W[n + ".weight"].permute(0, 3, 1, 2), W[n + ".bias"], **k)
        C = a.subsampling_conv_channels
        y = torch.relu(conv2(x[None, None], "encoder.pre_encode.conv.0", stride=2, padding=1))
        for i in range(n_stages(a) - 1):
            y = conv2(y, f"encoder.pre_encode.conv.{2 + 3 * i}", stride=2, padding=1, groups=C)
            y = torch.relu(conv2(y, f"encoder.pre_encode.conv.{3 + 3 * i}"))
        y = y[0].permute(1, 0, 2).reshape(y.shape[2], -1)   # [T', C * F'], column c * F' + f
        x = lin(y, "encoder.pre_encode.out")
    else:
        x = lin(x, "encoder.pre_encode")
    x = x * (math.sqrt(a.d_model) if a.xscaling else 1.0)
    T, d, H = x.shape[0], a.d_model, a.n_heads
    dh = d // H
    pos = rel_positions(T, d).double()
    out = dict(pre_encode=x.clone(), layers=[], out_len=T)
    for i in range(a.n_layers):
        p = f"encoder.layers.{i}."
        ln = lambda x, n: _ln(x, W[p + n + ".weight"], W[p + n + ".bias"])
        ff = lambda x, n: lin(torch.nn.functional.silu(lin(x, p + n + ".linear1")), p + n + ".linear2")
        x = x + 0.5 * ff(ln(x, "norm_feed_forward1"), "feed_forward1")
        h = ln(x, "norm_self_att")
        q, k, v = (lin(h, p + "self_attn.linear_" + n).reshape(T, H, dh).transpose(0, 1) for n in "qkv")
        pp = lin(pos, p + "self_attn.linear_pos").reshape(2 * T - 1, H, dh).transpose(0, 1)
        ac = (q + W[p + "self_attn.pos_bias_u"][:, None, :]) @ k.transpose(1, 2)
        bd = rel_shift_literal((q + W[p + "self_attn.pos_bias_v"][:, None, :]) @ pp.transpose(1, 2))[:, :, :T]
        att = lin((torch.softmax((ac + bd) * dh ** -0.5, -1) @ v).transpose(0, 1).reshape(T, d), p + "self_attn.linear_out")
        x = x + att
        h = lin(ln(x, "norm_conv"), p + "conv.pointwise_conv1")
        h = h[:, :d] * torch.sigmoid(h[:, d:])
        K = a.conv_kernel_size
        h = torch.nn.functional.conv1d(h.t()[None], W[p + "conv.depthwise_conv.weight"].permute(0, 2, 1), g(p + "conv.depthwise_conv.bias"), padding=(K - 1) // 2, groups=d)[0].t()
        bn = lambda n: W[p + "conv.batch_norm." + n]
        h = (h - bn("running_mean")) / torch.sqrt(bn("running_var") + 1e-5) * bn("weight") + bn("bias")
        cv = lin(torch.nn.functional.silu(h), p + "conv.pointwise_conv2")
        x = x + cv
        x = x + 0.5 * ff(ln(x, "norm_feed_forward2"), "feed_forward2")
        x = ln(x, "norm_out")
        if i == 0:
            out["attn0"], out["conv0"] = att, cv
        out["layers"].append(x.clone())
    out["layers"] = torch.stack(out["layers"])
    logp = torch.log_softmax(lin(x, "decoder.decoder_layers.0"), -1)
    top = torch.topk(logp, 2, dim=-1).values
    out.update(logp=logp, ids=logp.argmax(-1), gap=(top[:, 0] - top[:, 1]))
    return out


def result_dict(result) -> dict:
    """An ``AlignedResult`` (the reference's or this package's) as plain data."""
    toks = [t for s in result.sentences for t in s.tokens]
    return dict(text=result.text, sentences=[s.text for s in result.sentences], ids=[int(t.id) for t in toks], start=[float(t.start) for t in toks],
                duration=[float(t.duration) for t in toks], token_text=[t.text for t in toks])


def load_models(meta) -> dict:
    """tag -> (args, weights, [mel]) of the fixture's configs, regenerated from their seeds."""
    from mlx_audio_amd.stt.models.parakeet import make_parakeet_weights

    out = {}
    for tag, c in meta["configs"].items():
        assert c["enc"] == CONFIGS[tag]["enc"] and [tuple(x) for x in c["clips"]] == list(CONFIGS[tag]["clips"]) and meta["vocab"] == VOCAB
        args = make_args(c["enc"])
        w = make_parakeet_weights(args, c["seed_w"], head_gain=HEAD_GAIN, blank_bias=c["blank_bias"])
        out[tag] = (args, w, [synth_mel(seed, c["enc"]["feat_in"], frames) for frames, seed in c["clips"]])
    return out


def pad_batch(mels):
    """Right-padded [B, T, feat] batch and the items' lengths."""
    T = max(m.shape[0] for m in mels)
    batch = torch.zeros(len(mels), T, mels[0].shape[1])
    for i, m in enumerate(mels):
        batch[i, :m.shape[0]] = torch.from_numpy(m)
    return batch, [m.shape[0] for m in mels]


def same_decode(got: dict, want: dict) -> bool:
    """Two ``result_dict``s: ids, texts and sentence texts equal, ``start`` / ``duration`` within 1e-9."""
    return ((got["ids"], got["text"], got["sentences"], got["token_text"]) == (want["ids"], want["text"], want["sentences"], want["token_text"])
            and np.allclose(got["start"], want["start"], rtol=0, atol=1e-9) and np.allclose(got["duration"], want["duration"], rtol=0, atol=1e-9))
