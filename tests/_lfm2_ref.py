"""The two test configurations of LFM2, their seeded checkpoints, and a float64 restatement of ``lm/models/lfm2.py`` (``forward``) that
``tests/test_lfm2_cpu.py`` holds to the reference's own stored runs (``tests/golden/ref_lfm2.npz``)."""
import os

import torch

_BASE = dict(model_type="lfm2", vocab_size=96, max_position_embeddings=64, norm_eps=1e-5, num_attention_heads=2, block_multiple_of=64,
             block_ffn_dim_multiplier=1.0)
CONFIGS = {
    # heads of 64, one kv head, conv, conv, attention, conv; no conv biases; the ff width adjusted 256 -> 170 -> 192
    "A": dict(_BASE, hidden_size=128, block_dim=128, num_hidden_layers=4, num_key_value_heads=1, conv_bias=False, conv_L_cache=3, block_ff_dim=256,
              block_auto_adjust_ff_dim=True, layer_types=["conv", "conv", "full_attention", "conv"]),
    # heads of 128, an attention layer first, conv biases, four taps, theta from rope_parameters, the ff width as given
    "B": dict(_BASE, hidden_size=256, block_dim=256, num_hidden_layers=3, num_key_value_heads=2, conv_bias=True, conv_L_cache=4, block_ff_dim=320,
              block_auto_adjust_ff_dim=False, full_attn_idxs=[0], rope_parameters={"rope_theta": 10000.0}),
}
SEEDS = {"A": 21, "B": 22}
TOKENS, PREFILL = 17, 15   # one 17-token pass; 15 tokens and then two one-row steps through the caches
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_lfm2.npz")


def setup(name):
    """(ModelArgs, bfloat16-valued float32 checkpoint, token ids [TOKENS])."""
    from mlx_audio_amd.lm import lfm2

    args = lfm2.ModelArgs.from_dict(CONFIGS[name])
    w = {k: v.to(torch.bfloat16).float() for k, v in lfm2.make_lfm2_weights(args, SEEDS[name]).items()}
    ids = torch.randint(0, args.vocab_size, (TOKENS,), generator=torch.Generator().manual_seed(SEEDS[name]))
    return args, w, ids


def forward(a, w, ids):
    """Token ids [L] -> dict(layer{i}, logits) in float64, one causal pass without a cache."""
    d = {k: v.double() for k, v in w.items()}
    H, G, L, Lc = a.num_attention_heads, a.num_key_value_heads, ids.numel(), a.conv_L_cache
    dh = a.hidden_size // H
    rms = lambda x, wt: x * torch.rsqrt((x * x).mean(-1, keepdim=True) + a.norm_eps) * wt
    lin = lambda x, n: x @ d[n + ".weight"].T + (d[n + ".bias"] if n + ".bias" in d else 0.0)
    ang = torch.arange(L, dtype=torch.float64)[:, None] * a.rope_theta ** (-torch.arange(0, dh // 2, dtype=torch.float64) * 2.0 / dh)

    def rope(x):   # [heads, L, dh]: pairs (i, i + dh / 2)
        x1, x2 = x[..., :dh // 2], x[..., dh // 2:]
        return torch.cat([x1 * ang.cos() - x2 * ang.sin(), x1 * ang.sin() + x2 * ang.cos()], -1)

    out, x = {}, d["model.embed_tokens.weight"][ids]
    for i in range(a.num_hidden_layers):
        p = f"model.layers.{i}."
        h = rms(x, d[p + "operator_norm.weight"])
        if i in a.full_attn_idxs:
            q, k, v = (lin(h, f"{p}self_attn.{n}_proj").view(L, -1, dh).transpose(0, 1) for n in "qkv")
            q, k = rope(rms(q, d[p + "self_attn.q_layernorm.weight"])), rope(rms(k, d[p + "self_attn.k_layernorm.weight"])).repeat_interleave(H // G, 0)
            s = (q @ k.transpose(1, 2)) * dh ** -0.5 + torch.full((L, L), float("-inf"), dtype=torch.float64).triu(1)
            x = x + lin((torch.softmax(s, -1) @ v.repeat_interleave(H // G, 0)).transpose(0, 1).reshape(L, H * dh), p + "self_attn.out_proj")
        else:
            B, C, xx = lin(h, p + "conv.in_proj").chunk(3, -1)
            z = torch.cat([torch.zeros(Lc - 1, a.hidden_size, dtype=torch.float64), B * xx])
            conv = sum(d[p + "conv.conv.weight"][:, j, 0] * z[j:j + L] for j in range(Lc)) + (d[p + "conv.conv.bias"] if a.conv_bias else 0.0)
            x = x + lin(C * conv, p + "conv.out_proj")
        h = rms(x, d[p + "ffn_norm.weight"])
        x = x + lin(torch.nn.functional.silu(lin(h, p + "feed_forward.w1")) * lin(h, p + "feed_forward.w3"), p + "feed_forward.w2")
        out[f"layer{i}"] = x
    out["logits"] = rms(x, d["model.embedding_norm.weight"]) @ d["model.embed_tokens.weight"].T
    return out
