"""The two test configurations of the Bailing MoE model, their seeded checkpoints, and a float64 restatement of ``lm/models/bailing_moe.py``
(``forward``) that ``tests/test_bailing_moe_cpu.py`` holds to the reference's own stored runs (``tests/golden/ref_bailing_moe.npz``)."""
import os

import numpy as np
import torch

_BASE = dict(model_type="bailing_moe", max_position_embeddings=64, norm_topk_prob=True, num_attention_heads=2, num_hidden_layers=2, rms_norm_eps=1e-6,
             rope_theta=10000.0, vocab_size=96, first_k_dense_replace=1)
CONFIGS = {
    # softmax, 4 experts, top-2, no groups, one shared expert; heads of 64, full rotary
    "A": dict(_BASE, hidden_size=128, intermediate_size=192, moe_intermediate_size=64, num_experts=4, num_experts_per_tok=2, num_shared_experts=1,
              num_key_value_heads=2),
    # sigmoid + bias, 16 experts in 4 groups, top-4; heads of 128 (one kv head), rotary on half of them, q / k norm, biases, tied head
    "B": dict(_BASE, hidden_size=256, intermediate_size=320, moe_intermediate_size=48, num_experts=16, num_experts_per_tok=4, num_shared_experts=0,
              num_key_value_heads=1, score_function="sigmoid", moe_router_enable_expert_bias=True, n_group=4, topk_group=2, routed_scaling_factor=2.5,
              use_bias=True, use_qkv_bias=True, use_qk_norm=True, partial_rotary_factor=0.5, tie_word_embeddings=True),
}
SEEDS = {"A": 11, "B": 12}
TOKENS = 17   # B: 17 x 4 pairs >= 64, the reference sorts by expert; A: 34 pairs, it does not
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_bailing_moe.npz")


def setup(name):
    """(ModelArgs, bfloat16-valued float32 checkpoint, token ids [TOKENS])."""
    from mlx_audio_amd.lm import moe

    args = moe.ModelArgs.from_dict(CONFIGS[name])
    w = {k: v.to(torch.bfloat16).float() for k, v in moe.make_moe_weights(args, SEEDS[name]).items()}
    ids = torch.randint(0, args.vocab_size, (TOKENS,), generator=torch.Generator().manual_seed(SEEDS[name]))
    return args, w, ids


def _select(logits, bias, a):
    """group_expert_select up to the selection scores: (scores, selection scores) float64 [N, E]."""
    sc = torch.sigmoid(logits) if a.score_function == "sigmoid" else torch.softmax(logits, -1)
    sel = sc if bias is None else sc + bias
    if a.n_group > 1:
        g = sel.view(sel.shape[0], a.n_group, -1)
        gs = g.topk(2, -1).values.sum(-1)
        drop = torch.argsort(gs, dim=-1)[:, :a.n_group - a.topk_group]
        mask = torch.zeros_like(gs, dtype=torch.bool).scatter_(1, drop, True)
        sel = torch.where(mask[:, :, None], torch.zeros((), dtype=sel.dtype), g).reshape(sc.shape)
    return sc, sel


def selection_gap(logits, gate, a):
    """Per token: the k-th / (k + 1)-th selection gap of the float64 restatement on the reference's router logits (numpy [N, E])."""
    bias = None if getattr(gate, "expert_bias", None) is None else torch.from_numpy(np.asarray(gate.expert_bias, dtype=np.float64))
    s = torch.sort(_select(torch.from_numpy(logits), bias, a)[1], dim=-1, descending=True).values
    return (s[:, a.num_experts_per_tok - 1] - s[:, a.num_experts_per_tok]).numpy()


def forward(a, w, ids):
    """Token ids [L] -> dict(layer{i}, router{i}.ids (sorted), router{i}.wsum, logits) in float64, one causal pass."""
    d = {k: v.double() for k, v in w.items()}
    H, G = a.num_attention_heads, a.num_key_value_heads
    dh = a.hidden_size // H
    rot = a.rotary_dim if a.rotary_dim is not None else int(dh * a.partial_rotary_factor)
    L = ids.numel()
    rms = lambda x, wt: x * torch.rsqrt((x * x).mean(-1, keepdim=True) + a.rms_norm_eps) * wt
    lin = lambda x, n: x @ d[n + ".weight"].T + (d[n + ".bias"] if n + ".bias" in d else 0.0)
    mlp = lambda x, p: lin(torch.nn.functional.silu(lin(x, p + "gate_proj")) * lin(x, p + "up_proj"), p + "down_proj")
    ang = torch.arange(L, dtype=torch.float64)[:, None] * a.rope_theta ** (-torch.arange(0, rot // 2, dtype=torch.float64) * 2.0 / rot)

    def rope(x):   # [heads, L, dh]: pairs (i, i + rot / 2)
        x1, x2 = x[..., :rot // 2], x[..., rot // 2:rot]
        return torch.cat([x1 * ang.cos() - x2 * ang.sin(), x1 * ang.sin() + x2 * ang.cos(), x[..., rot:]], -1)

    out, x = {}, d["model.word_embeddings.weight"][ids]
    for i in range(a.num_hidden_layers):
        p = f"model.layers.{i}."
        qkv = lin(rms(x, d[p + "input_layernorm.weight"]), p + "attention.query_key_value")
        q, k, v = (t.view(L, -1, dh).transpose(0, 1) for t in qkv.split([H * dh, G * dh, G * dh], -1))
        if a.use_qk_norm:
            q, k = rms(q, d[p + "attention.query_layernorm.weight"]), rms(k, d[p + "attention.key_layernorm.weight"])
        q, k = rope(q), rope(k).repeat_interleave(H // G, 0)
        s = (q @ k.transpose(1, 2)) * dh ** -0.5 + torch.full((L, L), float("-inf"), dtype=torch.float64).triu(1)
        att = (torch.softmax(s, -1) @ v.repeat_interleave(H // G, 0)).transpose(0, 1).reshape(L, H * dh)
        x = x + lin(att, p + "attention.dense")
        h = rms(x, d[p + "post_attention_layernorm.weight"])
        if i < a.first_k_dense_replace:
            x = x + mlp(h, p + "mlp.")
            out[f"layer{i}"] = x
            continue
        sc, sel = _select(lin(h, p + "mlp.gate.gate_proj"), d.get(p + "mlp.gate.expert_bias") if a.moe_router_enable_expert_bias else None, a)
        top = torch.argsort(sel, dim=-1, descending=True, stable=True)[:, :a.num_experts_per_tok]
        wt = sc.gather(1, top)
        if a.num_experts_per_tok > 1 and a.norm_topk_prob:
            wt = wt / (wt.sum(-1, keepdim=True) + 1e-20)
        wt = wt * a.routed_scaling_factor
        y = torch.zeros_like(x)
        for t in range(L):
            for s_ in range(a.num_experts_per_tok):
                e = int(top[t, s_])
                ex = {n: (d[f"{p}mlp.switch_mlp.{n}.weight"][e], d[f"{p}mlp.switch_mlp.{n}.bias"][e] if a.use_bias else 0.0) for n in ("gate_proj", "up_proj", "down_proj")}
                f = lambda v_, n: v_ @ ex[n][0].T + ex[n][1]
                y[t] += wt[t, s_] * f(torch.nn.functional.silu(f(h[t], "gate_proj")) * f(h[t], "up_proj"), "down_proj")
        if a.num_shared_experts > 0 and a.moe_router_enable_shared_expert:
            y = y + mlp(h, p + "mlp.shared_experts.")
        x = x + y
        out[f"layer{i}"], out[f"router{i}.ids"], out[f"router{i}.wsum"] = x, top.sort(-1).values, wt.sum(-1)
    head = d["model.word_embeddings.weight"] if a.tie_word_embeddings else d["lm_head.weight"]
    out["logits"] = rms(x, d["model.norm.weight"]) @ head.T
    return out
