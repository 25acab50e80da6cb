"""LFM2 (lm/models/lfm2.py of the reference; the backbone of LFM2-Audio and of its detokenizer) on the device.  Most layers are ``ShortConv`` layers:
``in_proj -> (B, C, x) -> B * x -> causal depthwise conv over L_cache rows with a carried state -> C * conv``, one launch of csrc/shortconv.hip
(``ops.shortconv``) between the existing ``rmsnorm`` and the ``out_proj`` ``linear``; the attention layers are per-head q / k RMSNorm + half-rotation
rotary (``head_norm_rope``), ``flash_attention`` over a ``KVCache`` and ``linear``; the MLP is ``linear`` + ``swiglu``.

Parameter names and ``ModelArgs`` fields are the reference's.  ``Lfm2Model`` / ``Model`` are a host schedule: token ids (or ``input_embeddings``) ->
logits for prefill, one-row steps and right-padded batches (``lengths``: each item's valid rows, so that its carried conv state is that of the item
alone).  NOT built (each raises by name): hub download, quantised and 16-bit checkpoints, head widths other than 64 / 128, decode steps after a
ragged prefill (the KV cache holds one offset), the ``lfm_audio`` speech-to-speech wrapper."""
from __future__ import annotations

from dataclasses import dataclass, fields
from typing import Dict, List, Optional

import torch

from .. import ops
from .cache import ConvState
from .stack import KVCache, linear, make_lin


@dataclass
class ModelArgs:
    model_type: str
    vocab_size: int
    hidden_size: int
    num_hidden_layers: int
    num_attention_heads: int
    num_key_value_heads: int
    max_position_embeddings: int
    norm_eps: float
    conv_bias: bool
    conv_L_cache: int
    block_dim: int
    block_ff_dim: int
    block_multiple_of: int
    block_ffn_dim_multiplier: float
    block_auto_adjust_ff_dim: bool
    rope_theta: float = 1000000.0
    rope_parameters: Optional[dict] = None
    full_attn_idxs: Optional[List[int]] = None
    layer_types: Optional[List[str]] = None

    def __post_init__(self):
        if self.rope_parameters is not None and "rope_theta" in self.rope_parameters:
            self.rope_theta = self.rope_parameters["rope_theta"]
        if self.num_key_value_heads is None:
            self.num_key_value_heads = self.num_attention_heads
        if self.full_attn_idxs is None:
            self.full_attn_idxs = [i for i, t in enumerate(self.layer_types) if t == "full_attention"]

    @classmethod
    def from_dict(cls, d: dict) -> "ModelArgs":
        names = {f.name for f in fields(cls)}
        a = cls(**{k: v for k, v in d.items() if k in names})
        if a.hidden_size // a.num_attention_heads not in (64, 128):
            raise NotImplementedError(f"lfm2: head width {a.hidden_size // a.num_attention_heads} is not built (64 or 128)")
        return a

    @property
    def ff_dim(self) -> int:
        """``MLP.__init__`` of the reference: two thirds, the multiplier, rounded up to ``block_multiple_of``."""
        ff = self.block_ff_dim
        if self.block_auto_adjust_ff_dim:
            ff = int(2 * ff / 3)
            if self.block_ffn_dim_multiplier is not None:
                ff = int(self.block_ffn_dim_multiplier * ff)
            ff = self.block_multiple_of * ((ff + self.block_multiple_of - 1) // self.block_multiple_of)
        return ff


def from_pretrained(*_, **__):
    raise NotImplementedError("lfm2: hub download is not built; load a local checkpoint and pass its tensors")


def lfm_audio(*_, **__):
    raise NotImplementedError("lfm2: the lfm_audio speech-to-speech wrapper is not built (the LFM2 backbone is)")


def sanitize(weights: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """``Model.sanitize`` of the reference: a ``conv.weight`` stored [H, 1, L] becomes [H, L, 1]."""
    out = {}
    for name, p in weights.items():
        if "conv.weight" in name and p.shape[-1] > p.shape[1]:
            p = p.permute(0, 2, 1)
        out[name] = p
    return out


def _check_checkpoint(weights):
    for k, v in weights.items():
        if k.endswith((".scales", ".biases")):
            raise NotImplementedError(f"lfm2: quantised checkpoints are not built ({k})")
        if v.dtype in (torch.bfloat16, torch.float16):
            raise NotImplementedError(f"lfm2: 16-bit checkpoints are not built ({k} is {v.dtype}); pass float32 tensors")


class ShortConv:
    def __init__(self, args: ModelArgs, weights, prefix: str, device):
        f32 = lambda n: weights[prefix + n].to(device=device, dtype=torch.float32).contiguous() if prefix + n in weights else None
        self.w_in = ops.pack_rowmajor16(weights[prefix + "in_proj.weight"], None, device)
        self.in_bias, self.conv_bias = f32("in_proj.bias"), f32("conv.bias")
        self.taps = f32("conv.weight")[:, :, 0].contiguous()   # [H, L]: conv[t] = sum_j taps[:, j] * z[t + j]
        self.out_proj = make_lin(weights[prefix + "out_proj.weight"], weights.get(prefix + "out_proj.bias"), device)

    def __call__(self, h: torch.Tensor, x: torch.Tensor, st: ConvState):
        """x += out_proj(C * conv(state | B * x)) with h the normed input; the layer's state moves on by the rows of this call."""
        y = torch.empty_like(h)
        ops.shortconv(h, self.w_in, self.taps, y, state_in=st.state, state_out=st.next_state(h.shape[0]), lens=st.lengths, in_bias=self.in_bias,
                      conv_bias=self.conv_bias)
        st.swap(h.shape[1])
        return linear(y, self.out_proj, x, res=x)


class Attention:
    def __init__(self, args: ModelArgs, weights, prefix: str, device):
        H, G = args.num_attention_heads, args.num_key_value_heads
        self.H, self.G, self.dh, self.eps = H, G, args.hidden_size // H, args.norm_eps
        w = lambda n: weights[f"{prefix}{n}.weight"]
        self.wq = make_lin(w("q_proj"), None, device)
        self.wkv = make_lin(torch.cat([w("k_proj"), w("v_proj")]), None, device)
        self.out_proj = make_lin(w("out_proj"), None, device)
        self.qn, self.kn = (w(n).to(device=device, dtype=torch.float32).contiguous() for n in ("q_layernorm", "k_layernorm"))
        self.cos, self.sin = ops.moonshine_rope_tables(self.dh, args.max_position_embeddings, base=args.rope_theta, device=device)

    def __call__(self, h: torch.Tensor, x: torch.Tensor, kvc: KVCache):
        B, L, _ = h.shape
        H, G, dh = self.H, self.G, self.dh
        off = kvc.offset
        if off + L > self.cos.shape[0]:
            raise ValueError(f"lfm2: position {off + L - 1} is past max_position_embeddings = {self.cos.shape[0]}")
        slot = kvc.reserve(B, L)
        q, att = torch.empty(B, L, H * dh, device=h.device), torch.empty(B, L, H * dh, device=h.device)
        linear(h, self.wq, q)
        linear(h, self.wkv, slot)
        ks = slot[:, :, :G * dh]
        ops.head_norm_rope(q, q, heads=H, dh=dh, norm_weight=self.qn, eps=self.eps, cos=self.cos, sin=self.sin, pos0=off, second=(ks, ks, G, self.kn))
        ops.flash_attention(q, kvc.keys, kvc.values, att, heads=H, kv_heads=G, dh=dh, causal=True)
        return linear(att, self.out_proj, x, res=x)


class MLP:
    """w2(swiglu(w1(x), w3(x))): w1 and w3 rows interleaved into one image for ``ops.swiglu``."""

    def __init__(self, weights, prefix: str, device):
        w1, w3 = weights[prefix + "w1.weight"], weights[prefix + "w3.weight"]
        self.inter = w1.shape[0]
        self.gate_up = make_lin(torch.stack([w1, w3], 1).reshape(2 * self.inter, -1), None, device)
        self.down = make_lin(weights[prefix + "w2.weight"], None, device)

    def __call__(self, h: torch.Tensor, x: torch.Tensor):
        B, L, _ = h.shape
        gu, a = torch.empty(B, L, 2 * self.inter, device=h.device), torch.empty(B, L, self.inter, device=h.device)
        linear(h, self.gate_up, gu)
        ops.swiglu(gu, a)
        return linear(a, self.down, x, res=x)


class Lfm2Model:
    def __init__(self, args: ModelArgs, weights, device="cuda:0", prefix: str = "model."):
        ops.require_gpu()
        _check_checkpoint(weights)
        self.args, self.device = args, torch.device(device)
        vec = lambda n: weights[prefix + n].to(device=self.device, dtype=torch.float32).contiguous()
        self.embed_tokens = vec("embed_tokens.weight")
        self.layers = []
        for i in range(args.num_hidden_layers):
            p = f"{prefix}layers.{i}."
            op = Attention(args, weights, p + "self_attn.", self.device) if i in args.full_attn_idxs else ShortConv(args, weights, p + "conv.", self.device)
            self.layers.append((vec(f"layers.{i}.operator_norm.weight"), op, vec(f"layers.{i}.ffn_norm.weight"), MLP(weights, p + "feed_forward.", self.device)))
        self.embedding_norm = vec("embedding_norm.weight")

    def make_cache(self) -> list:
        a = self.args
        return [KVCache(a.num_key_value_heads, a.hidden_size // a.num_attention_heads, self.device) if isinstance(op, Attention)
                else ConvState(a.conv_L_cache - 1, a.hidden_size, self.device) for _, op, _, _ in self.layers]

    def __call__(self, inputs: Optional[torch.Tensor], cache: Optional[list] = None, input_embeddings: Optional[torch.Tensor] = None, *,
                 lengths=None, trace: Optional[dict] = None) -> torch.Tensor:
        """inputs [B, L] token ids (or ``input_embeddings`` [B, L, D]) -> the final-normed hidden states [B, L, D]; ``cache`` (``make_cache``) moves on
        by L rows.  ``lengths``: the valid rows of each item of a right-padded batch."""
        eps = self.args.norm_eps
        cache = self.make_cache() if cache is None else cache
        if input_embeddings is not None:
            x = input_embeddings.to(device=self.device, dtype=torch.float32).clone()
        else:
            x = torch.empty(*inputs.shape, self.args.hidden_size, device=self.device)
            ops.embed_sum(self.embed_tokens, inputs.to(device=self.device, dtype=torch.int32).reshape(*inputs.shape, 1), x)
        if lengths is not None:
            lens = torch.as_tensor(lengths, dtype=torch.int32).to(self.device)
        elif any(isinstance(c, KVCache) and getattr(c, "ragged", False) for c in cache):
            raise NotImplementedError("lfm2: decode steps after a ragged prefill are not built (the KV cache holds one offset)")
        h = torch.empty_like(x)
        for i, ((n1, op, n2, mlp), c) in enumerate(zip(self.layers, cache)):
            if lengths is not None:
                if isinstance(c, ConvState):
                    c.lengths = lens
                else:
                    c.ragged = True
            op(ops.rmsnorm(x, h, n1, eps=eps), x, c)
            mlp(ops.rmsnorm(x, h, n2, eps=eps), x)
            if trace is not None:
                trace[f"layer{i}"] = x.clone()
        return ops.rmsnorm(x, h, self.embedding_norm, eps=eps)


class Model:
    """Token ids -> logits; the head is the tied embedding.  ``weights``: a sanitized float32 checkpoint under the reference's names."""

    def __init__(self, args: ModelArgs, weights, device="cuda:0"):
        self.args, self.model_type = args, args.model_type
        self.model = Lfm2Model(args, weights, device)
        self.head = make_lin(weights["model.embed_tokens.weight"], None, self.model.device)

    @property
    def layers(self):
        return self.model.layers

    def make_cache(self):
        return self.model.make_cache()

    def __call__(self, inputs, cache=None, input_embeddings=None, *, lengths=None, trace: Optional[dict] = None) -> torch.Tensor:
        h = self.model(inputs, cache, input_embeddings, lengths=lengths, trace=trace)
        return linear(h, self.head, torch.empty(*h.shape[:2], self.args.vocab_size, device=h.device))


def make_lfm2_weights(args: ModelArgs, seed: int = 0) -> Dict[str, torch.Tensor]:
    """A seeded float32 checkpoint under the reference's parameter names (``conv.conv.weight`` as MLX holds it, [H, L, 1])."""
    g = torch.Generator().manual_seed(seed)
    D, H, G, F = args.hidden_size, args.num_attention_heads, args.num_key_value_heads, args.ff_dim
    dh = D // H
    r = lambda *s, fan: torch.randn(*s, generator=g) / fan ** 0.5
    ln = lambda n: 1.0 + 0.1 * torch.randn(n, generator=g)
    w = {"model.embed_tokens.weight": torch.randn(args.vocab_size, D, generator=g), "model.embedding_norm.weight": ln(D)}
    for i in range(args.num_hidden_layers):
        p = f"model.layers.{i}."
        w[p + "operator_norm.weight"], w[p + "ffn_norm.weight"] = ln(D), ln(D)
        w[p + "feed_forward.w1.weight"], w[p + "feed_forward.w3.weight"], w[p + "feed_forward.w2.weight"] = r(F, D, fan=D), r(F, D, fan=D), r(D, F, fan=F)
        if i in args.full_attn_idxs:
            a = p + "self_attn."
            w[a + "q_proj.weight"], w[a + "k_proj.weight"], w[a + "v_proj.weight"] = r(H * dh, D, fan=D), r(G * dh, D, fan=D), r(G * dh, D, fan=D)
            w[a + "out_proj.weight"], w[a + "q_layernorm.weight"], w[a + "k_layernorm.weight"] = r(D, H * dh, fan=D), ln(dh), ln(dh)
        else:
            c = p + "conv."
            w[c + "conv.weight"], w[c + "in_proj.weight"], w[c + "out_proj.weight"] = r(D, args.conv_L_cache, 1, fan=args.conv_L_cache), r(3 * D, D, fan=D), r(D, D, fan=D)
            if args.conv_bias:
                w[c + "conv.bias"], w[c + "in_proj.bias"], w[c + "out_proj.bias"] = (0.1 * torch.randn(n, generator=g) for n in (D, 3 * D, D))
    return w
