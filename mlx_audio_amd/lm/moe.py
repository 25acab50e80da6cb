"""The sparse mixture-of-experts FFN of the Ling / Ming language models (lm/models/bailing_moe.py, switch_layers.py of the reference) on the
device: the router's ``gate_proj`` and the shared experts run on the existing ``linear`` + ``swiglu``; routing, the sort by expert, the routed
``SwitchGLU`` and the weighted combine are the kernels of csrc/moe.hip (``ops.moe_route`` / ``ops.switch_glu``).

Quantised checkpoints (MLX's affine `-4bit` / `-8bit`, group 32 / 64 / 128) load as they are: ``sanitize`` stacks the per-expert ``weight`` /
``scales`` / ``biases``, the routed experts run on the packed codes (csrc/moe_quant.hip: ``ops.PackedQuantizedExperts``), and every dense parameter
that carries ``.scales`` -- attention, shared experts, dense MLPs, the router's ``gate_proj`` (8 bits in real checkpoints), ``lm_head`` and the
embedding -- runs on ``ops.qlinear`` / ``ops.dequantize_packed``.  Bits and group size come from the config's ``quantization`` dict (with
per-path overrides) or, without one, from the shapes.

So do the `-mxfp4` / `-nvfp4` / `-mxfp8` checkpoints.  A parameter whose ``.scales`` is uint8 with no ``.biases`` beside it is an MX parameter and its
shapes name the mode (``ops.infer_quantization_mx``); a ``mode`` in the config (global or per path) must agree.  The routed experts run on
csrc/moe_quant_mx.hip (``ops.PackedQuantizedExpertsMX``), the dense parameters on ``ops.QuantizedLinearMX``.  Each parameter is decided on its own,
so a checkpoint may mix the kinds (a router kept at affine 8 bits).

Parameter names and ``ModelArgs`` fields are the reference's.  ``BailingMoeModel`` / ``Model`` are a host schedule on existing kernels (``rmsnorm``,
``linear``, ``head_norm_rope`` / ``partial_rope``, ``flash_attention`` over a ``KVCache``, ``embed_sum``): token ids -> logits for prefill and
one-row decode steps.  NOT built (each raises by name): quantised experts at bits 2 / 3 / 5 / 6 or in MLX's non-affine modes (``.scales`` without
``.biases`` whose ``.scales`` is not uint8), hub download, head widths other than 64 / 128, ``rope_scaling``."""
from __future__ import annotations

from dataclasses import dataclass, fields
from typing import Dict, List, Optional, Union

import torch

from .. import ops
from .stack import KVCache, linear, make_lin


@dataclass
class ModelArgs:
    model_type: str
    hidden_size: int
    intermediate_size: int
    max_position_embeddings: int
    moe_intermediate_size: int
    num_experts: int
    num_shared_experts: int
    norm_topk_prob: bool
    num_attention_heads: int
    num_experts_per_tok: int
    num_hidden_layers: int
    num_key_value_heads: int
    rms_norm_eps: float
    rope_theta: float
    vocab_size: int
    first_k_dense_replace: int
    rope_scaling: Optional[Dict[str, Union[float, str]]] = None
    use_bias: bool = False
    use_qkv_bias: bool = False
    norm_head: bool = False
    norm_softmax: bool = False
    use_qk_norm: bool = False
    tie_word_embeddings: bool = False
    partial_rotary_factor: float = 1.0
    rotary_dim: Optional[int] = None
    moe_router_enable_expert_bias: bool = False
    moe_router_enable_routed_scaling: bool = True
    routed_scaling_factor: float = 1.0
    score_function: str = "softmax"
    n_group: int = 1
    topk_group: int = 4
    moe_shared_expert_intermediate_size: Optional[int] = None
    moe_router_enable_shared_expert: bool = True
    quantization: Optional[dict] = None   # the config's ``quantization`` (or ``quantization_config``): group_size, bits, {path: {...}} overrides

    @classmethod
    def from_dict(cls, d: dict) -> "ModelArgs":
        names = {f.name for f in fields(cls)}
        a = cls(**{k: v for k, v in d.items() if k in names})
        if a.quantization is None:
            a.quantization = d.get("quantization_config")
        if a.rope_scaling is not None:
            raise NotImplementedError("bailing_moe: rope_scaling is not built")
        if a.hidden_size // a.num_attention_heads not in (64, 128):
            raise NotImplementedError(f"bailing_moe: head width {a.hidden_size // a.num_attention_heads} is not built (64 or 128)")
        if a.score_function not in ops.MOE_SCORE_FN:
            raise ValueError(f"bailing_moe: unknown score_function {a.score_function!r}")
        return a


def from_pretrained(*_, **__):
    raise NotImplementedError("bailing_moe: hub download is not built; load a local checkpoint and pass its tensors")


QUANT_BITS, QUANT_GROUPS = (4, 8), (32, 64, 128)   # what csrc/qlinear.hip and csrc/moe_quant.hip are built for


def resolve_quantization(quantization: Optional[dict], path: str, words: int, groups: int):
    """(bits, group_size) of the parameter at ``path`` (no ``.weight``) whose packed rows hold ``words`` words beside ``groups`` scales: the entry of
    ``quantization`` for that path, else its global ``bits`` / ``group_size``, else what the shapes say (``ops.infer_quantization``)."""
    q = quantization or {}
    own = q.get(path) or q.get("model." + path)
    src = own if isinstance(own, dict) else q
    if src.get("mode") in ops.QMODES:   # the entry speaks of the MX parameters; an affine one beside them is read from its shapes
        src = {}
    return ops.infer_quantization(words, groups, group_size=src.get("group_size"), bits=src.get("bits"))


def _is_mx(t, prefix: str = "") -> bool:
    """An MX parameter: uint8 ``.scales`` with no ``.biases`` beside it."""
    sc = t.get(f"{prefix}scales")
    return sc is not None and sc.dtype == torch.uint8 and t.get(f"{prefix}biases") is None


def resolve_quantization_mx(quantization: Optional[dict], path: str, words: int, groups: int) -> str:
    """The mode of the MX parameter at ``path``: what the shapes name; ``quantization``'s ``mode`` for that path, else its global one, must agree
    (``ops.infer_quantization_mx`` raises ValueError, here with the parameter's name)."""
    q = quantization or {}
    own = q.get(path) or q.get("model." + path)
    src = own if isinstance(own, dict) else q
    try:
        return ops.infer_quantization_mx(words, groups, mode=src.get("mode"))[0]
    except ValueError as err:
        raise ValueError(f"bailing_moe: {path}: {err}") from None


def _check_quantized_experts(w, prefix: str, quantization):
    """What is still not built for ``{prefix}.{weight,scales,biases}``, refused by name."""
    not_built = "bailing_moe: quantised experts (QuantizedSwitchLinear) "
    if _is_mx(w, f"{prefix}."):
        wt = w.get(f"{prefix}.weight")
        if wt is None or wt.dtype not in (torch.uint32, torch.int32):
            raise NotImplementedError(not_built + f"need packed uint32 codes ({prefix}.weight is {None if wt is None else wt.dtype})")
        resolve_quantization_mx(quantization, prefix, wt.shape[-1], w[f"{prefix}.scales"].shape[-1])
        return
    if f"{prefix}.biases" not in w:
        raise NotImplementedError(not_built + f"in a non-affine mode are not built ({prefix}.scales has no .biases beside it)")
    wt = w.get(f"{prefix}.weight")
    if wt is None or wt.dtype not in (torch.uint32, torch.int32):
        raise NotImplementedError(not_built + f"need packed uint32 codes ({prefix}.weight is {None if wt is None else wt.dtype})")
    try:
        bits, group = resolve_quantization(quantization, prefix, wt.shape[-1], w[f"{prefix}.scales"].shape[-1])
    except (ValueError, AssertionError) as err:
        raise NotImplementedError(not_built + f"at {prefix}: {err}") from None
    if bits not in QUANT_BITS or group not in QUANT_GROUPS:
        raise NotImplementedError(not_built + f"with bits = {bits}, group_size = {group} are not built (bits {QUANT_BITS}, groups {QUANT_GROUPS} are)")


def sanitize(weights: Dict[str, torch.Tensor], args: ModelArgs) -> Dict[str, torch.Tensor]:
    """``Model.sanitize`` of the reference: per-expert tensors (``weight`` / ``scales`` / ``biases`` / ``bias``) stacked into ``switch_mlp.*``, the
    router renamed to ``gate.gate_proj.*``, the tied head dropped, ``norm_head`` applied.  Quantised experts outside what is built are refused by name."""
    w = dict(weights)
    if args.tie_word_embeddings:
        w.pop("lm_head.weight", None)
    if args.norm_head and "lm_head.weight" in w:
        h = w["lm_head.weight"].float()
        w["lm_head.weight"] = h / (torch.linalg.norm(h, dim=0, keepdim=True) + 1e-7)
    for l in range(args.first_k_dense_replace, args.num_hidden_layers):
        p = f"model.layers.{l}.mlp"
        for m in ("gate_proj", "down_proj", "up_proj"):
            for k in ("weight", "scales", "biases", "bias"):
                if f"{p}.experts.0.{m}.{k}" in w:
                    w[f"{p}.switch_mlp.{m}.{k}"] = torch.stack([w.pop(f"{p}.experts.{e}.{m}.{k}") for e in range(args.num_experts)])
            if f"{p}.switch_mlp.{m}.scales" in w:
                _check_quantized_experts(w, f"{p}.switch_mlp.{m}", args.quantization)
        for k in ("weight", "scales", "biases", "bias"):
            if f"{p}.gate.{k}" in w:
                w[f"{p}.gate.gate_proj.{k}"] = w.pop(f"{p}.gate.{k}")
    return w


def _rows_of(weights, name: str, pick=None) -> Dict[str, torch.Tensor]:
    """The row tensors of parameter ``name`` (``weight``, ``bias`` and, when quantised, ``scales`` / ``biases``), each with the row operation ``pick``
    applied: a row pick, split or interleave acts on the packed words and on the pair rows as it does on float rows."""
    t = {k: weights[f"{name}.{k}"] for k in ("weight", "scales", "biases", "bias") if weights.get(f"{name}.{k}") is not None}
    return t if pick is None else {k: pick(v) for k, v in t.items()}


def _make_lin(t: Dict[str, torch.Tensor], device, quantization, path: str):
    """A dense Linear from its row tensors: float -> ``make_lin``; with ``scales`` -> the packed codes for ``ops.qlinear``, affine or MX."""
    if "scales" not in t:
        return make_lin(t["weight"], t.get("bias"), device)
    if _is_mx(t):
        mode = resolve_quantization_mx(quantization, path, t["weight"].shape[-1], t["scales"].shape[-1])
        return ops.pack_quantized_mx(t["weight"], t["scales"], t.get("bias"), device, mode=mode)
    if "biases" not in t:
        raise NotImplementedError(f"bailing_moe: {path} in a non-affine mode is not built ({path}.scales is {t['scales'].dtype} with no .biases beside it)")
    bits, group = resolve_quantization(quantization, path, t["weight"].shape[-1], t["scales"].shape[-1])
    return ops.pack_quantized(t["weight"], t["scales"], t["biases"], t.get("bias"), device, group_size=group, bits=bits)


def _linear(x: torch.Tensor, l, y: torch.Tensor, *, res: Optional[torch.Tensor] = None):
    """``linear`` on [B, L, C] views for either kind of image."""
    if not isinstance(l, (ops.QuantizedLinear, ops.QuantizedLinearMX)):
        return linear(x, l, y, res=res)
    for b in range(x.shape[0]):
        ops.qlinear(x[b], l, y[b], res=None if res is None else res[b])
    return y


class SwitchGLU:
    """``switch_mlp.{gate,up,down}_proj``: the packed expert images (float) or the packed codes (a quantised checkpoint).  ``__call__`` is the routed
    FFN with its combine (``ops.switch_glu``)."""

    def __init__(self, weights, prefix: str, device, quantization: Optional[dict] = None):
        g = lambda n: weights.get(f"{prefix}{n}")
        if _is_mx(weights, f"{prefix}gate_proj."):
            for m in ("gate_proj", "up_proj", "down_proj"):   # the config's mode, where it names one, must agree with every projection
                resolve_quantization_mx(quantization, f"{prefix}{m}", g(f"{m}.weight").shape[-1], g(f"{m}.scales").shape[-1])
            gud = [(g(f"{m}.weight"), g(f"{m}.scales")) for m in ("gate_proj", "up_proj", "down_proj")]
            self.experts = ops.pack_quantized_experts_mx(*gud, device, gate_b=g("gate_proj.bias"), up_b=g("up_proj.bias"), down_b=g("down_proj.bias"))
            return
        if g("gate_proj.scales") is not None:
            packed = []
            for m in ("gate_proj", "up_proj", "down_proj"):
                bits, group = resolve_quantization(quantization, f"{prefix}{m}", g(f"{m}.weight").shape[-1], g(f"{m}.scales").shape[-1])
                packed.append(ops.pack_quantized_switch_linear(g(f"{m}.weight"), g(f"{m}.scales"), g(f"{m}.biases"), g(f"{m}.bias"), device,
                                                               group_size=group, bits=bits))
            self.experts = ops.PackedQuantizedExperts(*packed)
            return
        self.experts = ops.PackedExperts.pack(g("gate_proj.weight"), g("up_proj.weight"), g("down_proj.weight"), device, gate_b=g("gate_proj.bias"),
                                              up_b=g("up_proj.bias"), down_b=g("down_proj.bias"))

    def __call__(self, x, ids, weights, out, *, shared=None, res=None):
        return ops.switch_glu(x, self.experts, ids, weights, out, shared=shared, res=res)


class BailingMoeGate:
    def __init__(self, args: ModelArgs, weights, prefix: str, device):
        self.args = args
        self.lin = _make_lin(_rows_of(weights, f"{prefix}gate_proj"), device, args.quantization, f"{prefix}gate_proj")
        b = weights.get(f"{prefix}expert_bias") if args.moe_router_enable_expert_bias else None
        self.expert_bias = None if b is None else b.to(device=device, dtype=torch.float32).contiguous()

    def __call__(self, x: torch.Tensor, trace: Optional[dict] = None):
        """x [B, L, D] -> (ids [B L, k] int32, weights [B L, k]); ``trace`` receives the router ``logits`` [B L, E]."""
        a = self.args
        B, L, _ = x.shape
        logits = torch.empty(B, L, a.num_experts, device=x.device)
        _linear(x, self.lin, logits)
        if trace is not None:
            trace["logits"] = logits.view(B * L, a.num_experts)
        return ops.moe_route(logits.view(B * L, a.num_experts), a.num_experts_per_tok, expert_bias=self.expert_bias, score_function=a.score_function,
                             n_group=a.n_group, topk_group=a.topk_group, norm_topk_prob=a.norm_topk_prob, routed_scaling_factor=a.routed_scaling_factor)


class BailingMoeMLP:
    """down(swiglu(gate(x), up(x))) on the dense kernels: gate and up rows interleaved into one image for ``ops.swiglu``."""

    def __init__(self, weights, prefix: str, device, quantization: Optional[dict] = None):
        tg, tu = _rows_of(weights, f"{prefix}gate_proj"), _rows_of(weights, f"{prefix}up_proj")
        assert tg.keys() == tu.keys(), f"bailing_moe: {prefix}gate_proj and up_proj differ in kind ({sorted(tg)} / {sorted(tu)})"
        self.inter = tg["weight"].shape[0]
        inter = lambda a, b: torch.stack([a, b], 1).reshape(2 * a.shape[0], *a.shape[1:])
        self.gate_up = _make_lin({k: inter(tg[k], tu[k]) for k in tg}, device, quantization, f"{prefix}gate_proj")
        self.down = _make_lin(_rows_of(weights, f"{prefix}down_proj"), device, quantization, f"{prefix}down_proj")

    def __call__(self, x: torch.Tensor, out: torch.Tensor, *, res: Optional[torch.Tensor] = None):
        B, L, _ = x.shape
        gu = torch.empty(B, L, 2 * self.inter, device=x.device)
        h = torch.empty(B, L, self.inter, device=x.device)
        _linear(x, self.gate_up, gu)
        ops.swiglu(gu, h)
        return _linear(h, self.down, out, res=res)


class BailingMoeSparseMoeBlock:
    def __init__(self, args: ModelArgs, weights, prefix: str, device):
        self.args = args
        self.switch_mlp = SwitchGLU(weights, f"{prefix}switch_mlp.", device, args.quantization)
        self.gate = BailingMoeGate(args, weights, f"{prefix}gate.", device)
        on = args.num_shared_experts > 0 and args.moe_router_enable_shared_expert
        self.shared_experts = BailingMoeMLP(weights, f"{prefix}shared_experts.", device, args.quantization) if on else None

    def __call__(self, x: torch.Tensor, out: torch.Tensor, *, res: Optional[torch.Tensor] = None, trace: Optional[dict] = None):
        """x / out / res [B, L, D]: out = sum_slot weight * expert(x) + shared_experts(x) + res."""
        B, L, D = x.shape
        ids, wts = self.gate(x, trace)
        shared = None
        if self.shared_experts is not None:
            shared = self.shared_experts(x, torch.empty(B, L, D, device=x.device)).view(B * L, D)
        if trace is not None:
            trace.update(ids=ids, weights=wts, shared=shared)
        self.switch_mlp(x.reshape(B * L, D), ids, wts, out.view(B * L, D), shared=shared, res=None if res is None else res.reshape(B * L, D))
        return out


class _Attention:
    """``BailingMoeAttention``: the fused ``query_key_value`` image split at load into q and k | v (the cache row's own layout).  nn.RoPE pairs
    channel i with i + rot / 2; on ``rot < head_dim`` the kernel at hand (``partial_rope``) pairs 2i with 2i + 1, so the q / k rows (and the q / k
    norm weights) are permuted inside every head at load: q . k does not change under one permutation of both."""

    def __init__(self, args: ModelArgs, weights, prefix: str, device):
        H, G = args.num_attention_heads, args.num_key_value_heads
        dh = args.hidden_size // H
        self.H, self.G, self.dh, self.eps = H, G, dh, args.rms_norm_eps
        self.rot = args.rotary_dim if args.rotary_dim is not None else int(dh * args.partial_rotary_factor)
        src = torch.arange(dh)
        if self.rot < dh:
            src[0:self.rot:2], src[1:self.rot:2] = torch.arange(self.rot // 2), torch.arange(self.rot // 2, self.rot)
        rows = lambda n: (torch.arange(n)[:, None] * dh + src[None, :]).reshape(-1)
        pick = torch.cat([rows(H), H * dh + rows(G), (H + G) * dh + torch.arange(G * dh)])
        qkv, quant = f"{prefix}query_key_value", args.quantization
        self.wq = _make_lin(_rows_of(weights, qkv, lambda t: t[pick][:H * dh]), device, quant, qkv)
        self.wkv = _make_lin(_rows_of(weights, qkv, lambda t: t[pick][H * dh:]), device, quant, qkv)
        self.dense = _make_lin(_rows_of(weights, f"{prefix}dense"), device, quant, f"{prefix}dense")
        nw = lambda n: weights[f"{prefix}{n}_layernorm.weight"][src].to(device=device, dtype=torch.float32).contiguous() if args.use_qk_norm else None
        self.qn, self.kn = nw("query"), nw("key")
        self.cos, self.sin = ops.moonshine_rope_tables(self.rot, args.max_position_embeddings, base=args.rope_theta, device=device)

    def __call__(self, h: torch.Tensor, x: torch.Tensor, kvc: KVCache):
        """x += dense(attention(h)) with h the normed input; appends L rows to ``kvc``."""
        B, L, _ = h.shape
        H, G, dh = self.H, self.G, self.dh
        off = kvc.offset
        if off + L > self.cos.shape[0]:
            raise ValueError(f"bailing_moe: position {off + L - 1} is past max_position_embeddings = {self.cos.shape[0]}")
        slot = kvc.reserve(B, L)
        q, att = torch.empty(B, L, H * dh, device=h.device), torch.empty(B, L, H * dh, device=h.device)
        _linear(h, self.wq, q)
        _linear(h, self.wkv, slot)
        ks = slot[:, :, :G * dh]
        if self.rot == dh:
            ops.head_norm_rope(q, q, heads=H, dh=dh, norm_weight=self.qn, eps=self.eps, cos=self.cos, sin=self.sin, pos0=off, second=(ks, ks, G, self.kn))
        else:
            if self.qn is not None:
                ops.head_norm_rope(q, q, heads=H, dh=dh, norm_weight=self.qn, eps=self.eps, second=(ks, ks, G, self.kn))
            ops.partial_rope(q, q, heads=H, dh=dh, rot=self.rot, cos=self.cos, sin=self.sin, pos0=off, second=(ks, ks, G))
        ops.flash_attention(q, kvc.keys, kvc.values, att, heads=H, kv_heads=G, dh=dh, causal=True)
        return _linear(att, self.dense, x, res=x)


class BailingMoeModel:
    def __init__(self, args: ModelArgs, weights, device="cuda:0", prefix: str = "model."):
        ops.require_gpu()
        self.args, self.device = args, torch.device(device)
        vec = lambda n: weights[prefix + n].to(device=self.device, dtype=torch.float32).contiguous()
        emb = _rows_of(weights, prefix + "word_embeddings")
        self.word_embeddings = _make_lin(emb, self.device, args.quantization, prefix + "word_embeddings") if "scales" in emb else vec("word_embeddings.weight")
        self.layers = []
        for i in range(args.num_hidden_layers):
            p = f"{prefix}layers.{i}."
            sparse = args.num_experts is not None and i >= args.first_k_dense_replace
            mlp = BailingMoeSparseMoeBlock(args, weights, p + "mlp.", self.device) if sparse else BailingMoeMLP(weights, p + "mlp.", self.device, args.quantization)
            self.layers.append((vec(f"layers.{i}.input_layernorm.weight"), _Attention(args, weights, p + "attention.", self.device),
                                vec(f"layers.{i}.post_attention_layernorm.weight"), mlp))
        self.norm = vec("norm.weight")

    def make_cache(self) -> List[KVCache]:
        a = self.args
        return [KVCache(a.num_key_value_heads, a.hidden_size // a.num_attention_heads, self.device) for _ in self.layers]

    def __call__(self, inputs: torch.Tensor, cache: Optional[List[KVCache]] = None, trace: Optional[dict] = None) -> torch.Tensor:
        """inputs [B, L] token ids -> the final-normed hidden states [B, L, D]; ``cache`` (``make_cache``) is extended by L positions."""
        B, L = inputs.shape
        eps = self.args.rms_norm_eps
        cache = self.make_cache() if cache is None else cache
        x = torch.empty(B, L, self.args.hidden_size, device=self.device)
        tokens = inputs.to(device=self.device, dtype=torch.int32)
        if isinstance(self.word_embeddings, (ops.QuantizedLinear, ops.QuantizedLinearMX)):   # the quantised table: a row gather that dequantises
            ops.dequantize_packed(self.word_embeddings, tokens, out=x.view(B * L, -1))
        else:
            ops.embed_sum(self.word_embeddings, tokens.reshape(B, L, 1), x)
        h = torch.empty_like(x)
        for i, ((ln1, attn, ln2, mlp), kvc) in enumerate(zip(self.layers, cache)):
            attn(ops.rmsnorm(x, h, ln1, eps=eps), x, kvc)
            ops.rmsnorm(x, h, ln2, eps=eps)
            if isinstance(mlp, BailingMoeSparseMoeBlock):
                t = {} if trace is not None else None
                mlp(h, x, res=x, trace=t)
                if trace is not None:
                    trace[f"ids{i}"], trace[f"weights{i}"], trace[f"router_logits{i}"] = t["ids"], t["weights"], t["logits"]
            else:
                mlp(h, x, res=x)
            if trace is not None:
                trace[f"layer{i}"] = x.clone()
        return ops.rmsnorm(x, h, self.norm, eps=eps)


class Model:
    """Token ids -> logits.  ``weights``: a sanitized checkpoint (``sanitize``) under the reference's names."""

    def __init__(self, args: ModelArgs, weights, device="cuda:0"):
        self.args = args
        self.model = BailingMoeModel(args, weights, device)
        if args.tie_word_embeddings and isinstance(self.model.word_embeddings, (ops.QuantizedLinear, ops.QuantizedLinearMX)):
            self.lm_head = self.model.word_embeddings   # the quantised table is also the head
        else:
            name = "model.word_embeddings" if args.tie_word_embeddings else "lm_head"
            head = {k: v for k, v in _rows_of(weights, name).items() if k != "bias"}
            self.lm_head = _make_lin(head, self.model.device, args.quantization, name)

    def make_cache(self):
        return self.model.make_cache()

    def __call__(self, inputs: torch.Tensor, cache=None, trace: Optional[dict] = None) -> torch.Tensor:
        h = self.model(inputs, cache, trace)
        return _linear(h, self.lm_head, torch.empty(*h.shape[:2], self.args.vocab_size, device=h.device))


def make_moe_weights(args: ModelArgs, seed: int = 0) -> Dict[str, torch.Tensor]:
    """A seeded float32 checkpoint under the reference's (sanitized) parameter names."""
    g = torch.Generator().manual_seed(seed)
    D, H, G, V = args.hidden_size, args.num_attention_heads, args.num_key_value_heads, args.vocab_size
    dh = D // H
    r = lambda *s, fan: torch.randn(*s, generator=g) / fan ** 0.5
    ln = lambda n: 1.0 + 0.1 * torch.randn(n, generator=g)
    w = {"model.word_embeddings.weight": torch.randn(V, D, generator=g), "model.norm.weight": ln(D)}
    if not args.tie_word_embeddings:
        w["lm_head.weight"] = r(V, D, fan=D)
    for i in range(args.num_hidden_layers):
        p = f"model.layers.{i}."
        w[p + "input_layernorm.weight"], w[p + "post_attention_layernorm.weight"] = ln(D), ln(D)
        w[p + "attention.query_key_value.weight"], w[p + "attention.dense.weight"] = r((H + 2 * G) * dh, D, fan=D), r(D, H * dh, fan=D)
        if args.use_qkv_bias:
            w[p + "attention.query_key_value.bias"] = 0.1 * torch.randn((H + 2 * G) * dh, generator=g)
        if args.use_bias:
            w[p + "attention.dense.bias"] = 0.1 * torch.randn(D, generator=g)
        if args.use_qk_norm:
            w[p + "attention.query_layernorm.weight"], w[p + "attention.key_layernorm.weight"] = ln(dh), ln(dh)
        if i >= args.first_k_dense_replace:
            w.update(_block_weights(args, g, p + "mlp."))
        else:
            F = args.intermediate_size
            for n, shape, fan in (("gate_proj", (F, D), D), ("up_proj", (F, D), D), ("down_proj", (D, F), F)):
                w[f"{p}mlp.{n}.weight"] = r(*shape, fan=fan)
                if args.use_bias:
                    w[f"{p}mlp.{n}.bias"] = 0.1 * torch.randn(shape[0], generator=g)
    return w


def quantize_checkpoint_mx(weights: Dict[str, torch.Tensor], args: ModelArgs, mode: str, *, everything: bool = False, affine8=()):
    """The float checkpoint ``weights`` (sanitized names) as a `-mxfp4` / `-nvfp4` / `-mxfp8` one in the layout of the files -- ``ops.quantize_mx`` on every
    expert matrix and, with ``everything``, on every other matrix (the embedding included), the paths in ``affine8`` at affine 8 bits, group 64, with a power-of-two scale instead (fp16-exact); per-expert ``experts.{e}.*``
    tensors and the router under ``gate.*``, so that ``sanitize`` has its work to do -- and the float checkpoint of the dequantised values beside it."""
    _, bits, g = ops.QMODES[mode]
    ck, deq = {}, {}
    for key, v in weights.items():
        stem, kind = key.rsplit(".", 1)
        parts, deq[key] = {kind: v}, v
        if stem in affine8 and kind == "weight":
            grp = v.float().reshape(v.shape[0], -1, 64)
            scale = torch.pow(2.0, torch.ceil(torch.log2(2 * grp.abs().amax(-1).clamp_min(2.0 ** -14) / 255)))
            codes = torch.round(grp / scale[..., None] + 128).clamp_(0, 255).to(torch.int64)
            deq[key] = (scale[..., None] * (codes - 128)).reshape(v.shape)
            parts = {"weight": ops.pack_codes(codes.reshape(v.shape), 8).view(torch.int32), "scales": scale.half(), "biases": (-128 * scale).half()}
        elif kind == "weight" and v.dim() >= 2 and (".switch_mlp." in key or everything):
            words, scales = ops.quantize_mx(v.reshape(-1, v.shape[-1]).float(), mode)
            deq[key] = (ops.mx_code_values(ops.unpack_codes(words, bits), mode) * ops.mx_scale_values(scales, mode).repeat_interleave(g, 1)).reshape(v.shape)
            parts = {"weight": words.view(torch.int32).reshape(*v.shape[:-1], -1), "scales": scales.reshape(*v.shape[:-1], -1)}
        stem = stem.replace("gate.gate_proj", "gate")
        for k, t in parts.items():
            if ".switch_mlp." in key:
                ck.update({f"{stem.replace('switch_mlp.', f'experts.{e}.')}.{k}": t[e] for e in range(args.num_experts)})
            else:
                ck[f"{stem}.{k}"] = t
    return ck, deq


def _block_weights(args: ModelArgs, g: torch.Generator, prefix: str) -> Dict[str, torch.Tensor]:
    D, I, E = args.hidden_size, args.moe_intermediate_size, args.num_experts
    r = lambda *s, fan: torch.randn(*s, generator=g) / fan ** 0.5
    w = {f"{prefix}gate.gate_proj.weight": r(E, D, fan=D) * 2.0}
    for n, shape, fan in (("gate_proj", (E, I, D), D), ("up_proj", (E, I, D), D), ("down_proj", (E, D, I), I)):
        w[f"{prefix}switch_mlp.{n}.weight"] = r(*shape, fan=fan)
        if args.use_bias:
            w[f"{prefix}switch_mlp.{n}.bias"] = 0.1 * torch.randn(E, shape[1], generator=g)
    if args.moe_router_enable_expert_bias:
        w[f"{prefix}gate.expert_bias"] = 0.02 * torch.randn(E, generator=g)
    if args.num_shared_experts > 0 and args.moe_router_enable_shared_expert:
        S = (args.moe_shared_expert_intermediate_size or I) * args.num_shared_experts
        for n, shape, fan in (("gate_proj", (S, D), D), ("up_proj", (S, D), D), ("down_proj", (D, S), S)):
            w[f"{prefix}shared_experts.{n}.weight"] = r(*shape, fan=fan)
            if args.use_bias:
                w[f"{prefix}shared_experts.{n}.bias"] = 0.1 * torch.randn(shape[0], generator=g)
    return w
