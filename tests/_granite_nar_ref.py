"""Shared by the Granite Speech NAR tests and the fixture maker: the two test-sized configurations, the seeded checkpoints' recipe and the clips.
The audio is regenerated from its seeds, never stored."""
import numpy as np

FS = 16000
# clip lengths in samples: 400 samples, 1 s, 1.3 s, 3 s, 5 s -> 1, 50, 65, 150, 250 encoder frames (the 1.3 s clip leaves an odd mel frame to trim)
CLIPS = ((400, 11), (16000, 12), (20800, 13), (48000, 14), (80000, 15))
VOCAB = 120
BLANK = VOCAB - 1


def config_dict(tag):
    """Config A: encoder 128 = 2 x 64, ctx 50, max_pos 64, 3 layers, self-conditioning at 2, editor 128 = 2 x 64.  Config B: encoder 128 = 1 x 128,
    ctx 200, max_pos 512, 2 layers, self-conditioning at 1, editor 256 = 2 x 128.  Both: conv kernel 15, projector block 15 / rate 5 with 2 heads of
    64, 1 editor kv head, 2 editor layers, vocabulary 120."""
    a = tag == "A"
    layers = 3 if a else 2
    enc = dict(num_layers=layers, hidden_dim=128, num_heads=2 if a else 1, dim_head=64 if a else 128, input_dim=160, output_dim=48, bpe_output_dim=VOCAB,
               bpe_pooling_window=4, conv_kernel_size=15, conv_expansion_factor=2, feedforward_mult=2, max_pos_emb=64 if a else 512,
               context_size=50 if a else 200, self_conditioning_layer=2 if a else 1, blank_token_id=BLANK, dropout=0.0, pred_dropout=0.0,
               initializer_range=0.02)
    ht = 128 if a else 256
    proj = dict(num_layers=2, num_encoder_layers=3, hidden_size=128, num_heads=2, block_size=15, downsample_rate=5, encoder_dim=128, llm_dim=ht,
                mlp_ratio=2, mlp_bias=True, attn_bias=True, dropout_prob=0.0, layernorm_eps=1e-6)
    text = dict(hidden_size=ht, intermediate_size=2 * ht, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1, vocab_size=VOCAB,
                max_position_embeddings=4096, rms_norm_eps=1e-5, rope_parameters=dict(rope_theta=10000.0), tie_word_embeddings=True,
                attention_multiplier=1.0 / (64 if a else 128), embedding_multiplier=12.0, logits_scaling=8.0, residual_multiplier=0.22, bos_token_id=0,
                eos_token_id=0, pad_token_id=0)
    return dict(encoder_config=enc, projector_config=proj, text_config=text, encoder_layer_indices=[1, 2, -1] if a else [0, 1, -1],
                blank_token_id=BLANK, scale_projected_embeddings=True, min_edit_sequence_length=8, tie_word_embeddings=True)


# the checkpoints' seeds and head biases (chosen by the fixture maker's own checks: margins, an empty hypothesis, a long one, collapsing repeats)
WEIGHTS = dict(A=dict(seed=12, head_gain=6.0, blank_bias=1.0, bpe_blank_bias=3.0, embed_gain=0.02),
               B=dict(seed=4, head_gain=6.0, blank_bias=1.0, bpe_blank_bias=3.0, embed_gain=0.01))


def synth_audio(n, seed):
    """A few seeded partials under a slow envelope plus noise, float32 in [-1, 1]."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / FS
    x = 0.02 * rng.standard_normal(n)
    for _ in range(4):
        f, ph, am = rng.uniform(120, 3000), rng.uniform(0, 2 * np.pi), rng.uniform(0.05, 0.2)
        x += am * np.sin(2 * np.pi * f * t + ph) * (0.6 + 0.4 * np.sin(2 * np.pi * rng.uniform(1, 6) * t))
    return np.clip(x, -1, 1).astype(np.float32)


class ListTokenizer:
    """The smallest object ``generate`` works with: ``decode(ids, skip_special_tokens=True)``."""

    def decode(self, ids, skip_special_tokens=True):
        return " ".join(f"t{int(i)}" for i in ids)


# ---------------------------------------------------------------------------------------------------- the stored runs (tests/golden/ref_granite_nar.*)
def load_fixture():
    import json
    import os

    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    with open(os.path.join(here, "ref_granite_nar.json")) as f:
        meta = json.load(f)
    return np.load(os.path.join(here, "ref_granite_nar.npz")), meta


def stored_features(fx, i):
    """Clip ``i``'s features as the reference's encoder saw them: the bfloat16 values, widened to float32."""
    import torch

    return torch.from_numpy(fx[f"feat{i}_bf16"].copy()).view(torch.bfloat16).to(torch.float32)


def build_model(tag, device):
    from mlx_audio_amd.stt.models.granite_speech_nar import GraniteSpeechNar as Model, ModelConfig, make_granite_nar_weights

    cfg = ModelConfig.from_dict(config_dict(tag))
    model = Model(cfg, make_granite_nar_weights(cfg, **WEIGHTS[tag]), device=device)
    model._tokenizer = ListTokenizer()
    return model


def compare_clip(st, fx, tag, i, b=0):
    """One item ``b`` of ``transcribe_batch(..., return_stages=True)``'s stages against clip ``i``'s stored run of config ``tag``: every decision is
    asserted equal; returns stage -> max |error| / the stored stage's peak."""
    key = lambda k: fx[f"{tag}{i}_{k}"]
    n_ = lambda t: t.detach().cpu().double().numpy()
    rows, wins, erows = key("rows"), key("windows"), key("editor_rows")
    W, N = len(key("bpe_ids")), len(key("text_ids"))
    assert st["bpe_lens"][b] == W and st["text_lens"][b] == N
    assert np.array_equal(st["bpe_ids"][b, :W].cpu().numpy(), key("bpe_ids")), (tag, i, "a BPE frame decision differs")
    assert st["hyp"][b] == key("hyp").tolist() and st["text_ids"][b] == key("text_ids").tolist()
    assert np.array_equal(st["edit_ids"][b, :N].cpu().numpy(), key("edit_ids")), (tag, i, "an edited-position decision differs")
    assert st["final"][b] == key("final").tolist()
    B = st["hidden"].shape[0]
    nbmax = st["proj_queries"].shape[0] // B
    nq, llm = st["proj_queries"].shape[1], st["audio"].shape[-1]
    t0 = sum(st["text_lens"][:b])
    got = dict(input_linear=n_(st["input_linear"][b])[rows], probs=n_(st["probs"][b])[rows], pooled=n_(st["pooled"][b, :W]),
               proj_queries=n_(st["proj_queries"][b * nbmax:(b + 1) * nbmax])[wins], proj_kv=n_(st["proj_kv"][b * nbmax:(b + 1) * nbmax])[wins],
               audio=n_(st["audio"][b]).reshape(-1, nq, llm)[wins], editor_in=n_(st["editor_in"][b])[erows], tail_logits=n_(st["tail_logits"][t0:t0 + N]))
    for k in st:
        if k.startswith("attn") or k.startswith("block"):
            got[k] = n_(st[k][b])[rows]
        elif k.startswith("editor") and k != "editor_in":
            got[k] = n_(st[k][b])[erows]
    out = {}
    for k, g in got.items():
        want = key(k).astype(np.float64)
        assert g.shape == want.shape, (k, g.shape, want.shape)
        out[k] = float(np.abs(g - want).max() / np.abs(want).max())
    return out


# ---------------------------------------------------------------------------------------------------- float64 restatement of the reference's modules
def published_config_dict(vocab=4096):
    """The published widths as the reference's docstrings give them (encoder 1024 = 8 x 128 at context 200, four fused layers to 4096; projector
    2048 = 32 x 64, block 15, rate 5; editor 2048 with 16 heads of 128 over 4 kv heads, multipliers 1 / 128, 12, 8, 0.22), cut to ONE encoder, projector
    and editor layer and a vocabulary of ``vocab``.  Every other value (max_pos 512, the FFN / conv / MLP ratios, the character head of 348, the editor's
    intermediate width, eps) is a parameter of the test, not a published fact."""
    enc = dict(num_layers=1, hidden_dim=1024, num_heads=8, dim_head=128, input_dim=160, output_dim=348, bpe_output_dim=vocab, bpe_pooling_window=4,
               conv_kernel_size=15, conv_expansion_factor=2, feedforward_mult=4, max_pos_emb=512, context_size=200, self_conditioning_layer=1,
               blank_token_id=vocab - 1, dropout=0.0, pred_dropout=0.0, initializer_range=0.02)
    proj = dict(num_layers=1, num_encoder_layers=4, hidden_size=2048, num_heads=32, block_size=15, downsample_rate=5, encoder_dim=1024, llm_dim=2048,
                mlp_ratio=2, mlp_bias=True, attn_bias=True, dropout_prob=0.0, layernorm_eps=1e-6)
    text = dict(hidden_size=2048, intermediate_size=4096, num_hidden_layers=1, num_attention_heads=16, num_key_value_heads=4, vocab_size=vocab,
                max_position_embeddings=4096, rms_norm_eps=1e-5, rope_parameters=dict(rope_theta=10000.0), tie_word_embeddings=True,
                attention_multiplier=1.0 / 128, embedding_multiplier=12.0, logits_scaling=8.0, residual_multiplier=0.22, bos_token_id=0, eos_token_id=0,
                pad_token_id=0)
    return dict(encoder_config=enc, projector_config=proj, text_config=text, encoder_layer_indices=[0, 1, 1, -1], blank_token_id=vocab - 1,
                scale_projected_embeddings=True, min_edit_sequence_length=8, tie_word_embeddings=True)


def reference_forward(cfg, w, feats):
    """The reference's ``_transcribe_tokens`` behind the bfloat16 cast, restated module by module in float64 torch for ONE clip: ``cfg`` a
    ``ModelConfig``, ``w`` the checkpoint, ``feats`` [T, 160] (bfloat16 values).  Returns the stages the published-width test compares."""
    import torch
    import torch.nn.functional as F

    e, p, t = cfg.encoder, cfg.projector, cfg.text
    W = {k: v.double() for k, v in w.items()}
    lin = lambda n, x: x @ W[n + ".weight"].reshape(W[n + ".weight"].shape[0], -1).T + (W[n + ".bias"] if n + ".bias" in W else 0.0)
    ln = lambda n, x, eps=1e-5: F.layer_norm(x, x.shape[-1:], W[n + ".weight"], W[n + ".bias"], eps)
    rms = lambda n, x: x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + t.rms_norm_eps) * W[n + ".weight"]
    x = torch.as_tensor(feats).double()
    T = x.shape[0]
    h = lin("encoder.input_linear", x)
    states = [h]
    H, dh, ctx, mp = e.num_heads, e.dim_head, e.context_size, e.max_pos_emb
    for i in range(1, e.num_layers + 1):
        q = f"encoder.layers.{i - 1}."
        ffn = lambda f, z: lin(q + f + ".down_proj", F.silu(lin(q + f + ".up_proj", ln(q + f + ".pre_norm", z))))
        h = 0.5 * ffn("ff1", h) + h
        a = ln(q + "attn.pre_norm", h)                                           # encoder.py:84-126
        pad = (ctx - T % ctx) % ctx
        a = torch.cat([a, torch.zeros(pad, a.shape[1], dtype=torch.float64)])
        nb = (T + pad) // ctx
        blocks = lambda z: z.reshape(nb, ctx, H, dh).permute(0, 2, 1, 3)
        qq = blocks(lin(q + "attn.to_q", a))
        kk, vv = (blocks(z) for z in lin(q + "attn.to_kv", a).chunk(2, dim=-1))
        idx = torch.arange(ctx)
        rel = W[q + "attn.rel_pos_emb.weight"][(idx[:, None] - idx[None, :]).clamp(-ctx, ctx) + mp]
        logits = (qq @ kk.transpose(-1, -2) + torch.einsum("mhcd,crd->mhcr", qq, rel)) * dh ** -0.5
        att = (torch.softmax(logits, -1) @ vv).permute(0, 2, 1, 3).reshape(nb * ctx, H * dh)[:T]
        h = lin(q + "attn.to_out", att) + h
        c = lin(q + "conv.up_conv", ln(q + "conv.norm", h))                      # encoder.py:185-195
        c = c[:, :c.shape[1] // 2] * torch.sigmoid(c[:, c.shape[1] // 2:])
        c = F.conv1d(c.T[None], W[q + "conv.depth_conv.weight"].permute(0, 2, 1), padding=e.conv_kernel_size // 2, groups=c.shape[1])[0].T
        c = (c - W[q + "conv.bn.running_mean"]) * torch.rsqrt(W[q + "conv.bn.running_var"] + 1e-5) * W[q + "conv.bn.weight"] + W[q + "conv.bn.bias"]
        h = lin(q + "conv.down_conv", F.silu(c)) + h
        h = 0.5 * ffn("ff2", h) + h
        h = ln(q + "post_norm", h)
        if i == e.self_conditioning_layer:
            probs = torch.softmax(lin("encoder.out", h), -1)
            h = h + lin("encoder.out_mid", probs)
        states.append(h)
    win = e.bpe_pooling_window                                                   # encoder.py:302-334
    padw = (win - T % win) % win
    imp = torch.cat([1.0 - probs[:, 0], torch.zeros(padw, dtype=torch.float64)]).reshape(-1, win)
    hw = torch.cat([h, torch.zeros(padw, h.shape[1], dtype=torch.float64)]).reshape(-1, win, h.shape[1])
    pooled = (hw * (imp / imp.sum(-1, keepdim=True).clamp_min(1e-6))[..., None]).sum(1)
    bpe_logits = lin("encoder.out_bpe", pooled)
    bpe_ids = bpe_logits.argmax(-1).tolist()
    hyp = [tk for j, tk in enumerate(bpe_ids) if (j == 0 or tk != bpe_ids[j - 1]) and tk != cfg.blank_token_id]
    d = e.hidden_dim                                                             # projector.py:183-226
    fused = torch.cat([ln(f"projector.layer_norms.{s}", states[idx], p.layernorm_eps) for s, idx in enumerate(cfg.encoder_layer_indices)], -1)
    g = F.gelu(lin("projector.layer_projector", fused))
    block, rate = p.block_size, p.downsample_rate
    padb = (block - T % block) % block
    g = torch.cat([g, torch.zeros(padb, g.shape[1], dtype=torch.float64)]).reshape(-1, block, p.hidden_size)
    query = W["projector.query"] + g.reshape(g.shape[0], block // rate, rate, -1).mean(-2)
    kv = g + W["projector.window_positions"]
    hp, dp = p.num_heads, p.hidden_size // p.num_heads
    for i in range(p.num_layers):
        q = f"projector.qformer.layers.{i}."
        heads = lambda z: z.reshape(z.shape[0], z.shape[1], hp, dp).transpose(1, 2)
        qn = ln(q + "attn_norm", query, p.layernorm_eps)
        qh, kh, vh = heads(lin(q + "cross_attention.q_proj", qn)), heads(lin(q + "cross_attention.k_proj", kv)), heads(lin(q + "cross_attention.v_proj", kv))
        att = (torch.softmax(qh @ kh.transpose(-1, -2) * dp ** -0.5, -1) @ vh).transpose(1, 2).reshape(query.shape)
        query = query + lin(q + "cross_attention.o_proj", att)
        query = query + lin(q + "mlp.fc2", F.silu(lin(q + "mlp.fc1", ln(q + "mlp_norm", query, p.layernorm_eps))))
    audio = lin("projector.out_linear", ln("projector.out_norm", query, p.layernorm_eps)).reshape(-1, p.llm_dim)
    from mlx_audio_amd.stt.models.granite_speech_nar import add_insertion_slots

    text_ids = add_insertion_slots(hyp, cfg.blank_token_id, cfg.min_edit_sequence_length)
    z = torch.cat([audio / t.embedding_multiplier, W["editor.embed_tokens.weight"][text_ids]]) * t.embedding_multiplier      # editor.py:232-262
    S, A = z.shape[0], audio.shape[0]
    Hq, Hkv = t.num_attention_heads, t.num_key_value_heads
    dt = t.hidden_size // Hq
    ang = torch.arange(S, dtype=torch.float64)[:, None] * (t.rope_theta ** (-torch.arange(0, dt, 2, dtype=torch.float64) / dt))[None]
    cos, sin = torch.cos(ang)[:, None, :], torch.sin(ang)[:, None, :]

    def rope(v):                                                                  # half rotation (traditional=False)
        a, b = v[..., :dt // 2], v[..., dt // 2:]
        return torch.cat([a * cos - b * sin, b * cos + a * sin], -1)

    for i in range(t.num_hidden_layers):
        q = f"editor.layers.{i}."
        n = rms(q + "input_layernorm", z)
        qh = rope(lin(q + "self_attn.q_proj", n).reshape(S, Hq, dt)).transpose(0, 1)
        kh = rope(lin(q + "self_attn.k_proj", n).reshape(S, Hkv, dt)).transpose(0, 1).repeat_interleave(Hq // Hkv, 0)
        vh = lin(q + "self_attn.v_proj", n).reshape(S, Hkv, dt).transpose(0, 1).repeat_interleave(Hq // Hkv, 0)
        att = (torch.softmax(qh @ kh.transpose(-1, -2) * t.attention_multiplier, -1) @ vh).transpose(0, 1).reshape(S, Hq * dt)
        z = z + lin(q + "self_attn.o_proj", att) * t.residual_multiplier
        n = rms(q + "post_attention_layernorm", z)
        z = z + lin(q + "mlp.down_proj", F.silu(lin(q + "mlp.gate_proj", n)) * lin(q + "mlp.up_proj", n)) * t.residual_multiplier
    tail = (rms("editor.norm", z)[A:] @ W["editor.embed_tokens.weight"].T) / t.logits_scaling
    edit_ids = tail.argmax(-1).tolist()
    final = [tk for j, tk in enumerate(edit_ids) if (j == 0 or tk != edit_ids[j - 1]) and tk != cfg.blank_token_id]
    gap = lambda lg: (lambda s: (s[:, -1] - s[:, -2]))(lg.sort(-1).values)
    return dict(hidden=h, probs=probs, pooled=pooled, bpe_ids=bpe_ids, bpe_gap=gap(bpe_logits), hyp=hyp, audio=audio, editor_out=z, tail_logits=tail,
                edit_ids=edit_ids, edit_gap=gap(tail), final=final)
