"""TEST INFRASTRUCTURE: the FireRedASR2 test configurations, the seeded clips, and a float64 restatement of the reference's forward pass
(stt/models/fireredasr2/fireredasr2.py) in torch on the CPU, written from the module's lines: Conv2dSubsampling (:17-39), RelPositionalEncoding
(:42-66), ConformerFeedForward (:69-82), ConformerConvolution (:85-118), RelPosMultiHeadAttention with ``_rel_shift`` (:121-191), ConformerBlock
(:194-209), ConformerEncoder with its six zero frames (:212-233), the decoder layer over the whole prefix (:252-329) and ``beam_search`` (:369-464)
with the reference's layer-output caches replaced by recomputation over the full prefix (the same function).  Nothing under ``mlx_audio_amd/``
imports it."""
import math

import numpy as np
import torch

from mlx_audio_amd.stt.models.fireredasr2 import ModelConfig
from mlx_audio_amd.stt.models.fireredasr2.fireredasr2 import abs_pe_table, rel_pe_table

F64 = torch.float64
INF = 1e10
CONFIGS = {
    "A": dict(cfg=dict(odim=200, encoder=dict(n_layers=2, n_head=2, d_model=128, kernel_size=33), decoder=dict(n_layers=2, n_head=2, d_model=128)),
              seed_w=21, logit_gain=20.0, eos_gain=1.0, beams=(3,), cmvn=False, clips=[(400, 301), (4800, 302), (16000, 303), (48000, 304)]),
    "B": dict(cfg=dict(odim=500, encoder=dict(n_layers=1, n_head=2, d_model=256, kernel_size=15), decoder=dict(n_layers=2, n_head=2, d_model=256)),
              seed_w=22, logit_gain=20.0, eos_gain=1.0, beams=(1, 5), cmvn=True, clips=[(400, 401), (4800, 402), (16000, 403), (48000, 404)]),
}
# endings: EOS after several tokens (eos_bias raises the EOS logit from that step on), EOS at the first step, the T_enc step limit (never EOS)
ENDINGS = ("late", "first", "limit")
LATE_EOS = {200: 9.5, 500: 13.5}
FIRST_EOS = {200: 18.0, 500: 18.0}   # per configuration (keyed by odim): tuned on the reference until a run ends by EOS after several tokens


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


def cmvn_for(name: str, idim: int = 80):
    rng = np.random.default_rng(7 if name == "B" else 8)
    return (10.0 + rng.standard_normal(idim)).astype(np.float32), (0.2 + 0.05 * rng.random(idim)).astype(np.float32)


def eos_variant(w: dict, c: ModelConfig, ending: str) -> dict:
    """The seeded checkpoint with its EOS row of ``tgt_word_prj`` changed so that decoding ends as ``ending`` says (fp16-representable values)."""
    w = dict(w)
    prj = w["decoder.tgt_word_prj.weight"].clone()
    if ending == "late":
        prj[c.eos_id] = 0.0
        w["decoder.layer_norm_out.weight"] = w["decoder.layer_norm_out.weight"].clone()
        w["decoder.layer_norm_out.bias"] = w["decoder.layer_norm_out.bias"].clone()
        prj[c.eos_id, 0] = LATE_EOS[c.odim]
        w["decoder.layer_norm_out.weight"][0] = 0.0
        w["decoder.layer_norm_out.bias"][0] = 4.0          # the EOS logit is the constant 4 LATE_EOS: about the level of a step's best other logit
    elif ending == "first":
        prj[c.eos_id] = 0.0
        w["decoder.layer_norm_out.bias"] = w["decoder.layer_norm_out.bias"].clone()
        prj[c.eos_id, 0] = FIRST_EOS[c.odim]
        w["decoder.layer_norm_out.weight"] = w["decoder.layer_norm_out.weight"].clone()
        w["decoder.layer_norm_out.weight"][0] = 0.0
        w["decoder.layer_norm_out.bias"][0] = 4.0          # channel 0 of the normalised state is the constant 4: the EOS logit is 4 FIRST_EOS at every step: above the others, which stay clear of the 1e-10 floor
    elif ending == "limit":
        prj[c.eos_id] = 0.0
        w["decoder.layer_norm_out.weight"] = w["decoder.layer_norm_out.weight"].clone()
        w["decoder.layer_norm_out.bias"] = w["decoder.layer_norm_out.bias"].clone()
        prj[c.eos_id, 0] = -64.0
        w["decoder.layer_norm_out.weight"][0] = 0.0
        w["decoder.layer_norm_out.bias"][0] = 4.0          # ... -256: EOS never enters a beam
    w["decoder.tgt_word_prj.weight"] = prj
    return w


def _ln(x, w, p):
    m, v = x.mean(-1, keepdim=True), x.var(-1, unbiased=False, keepdim=True)
    return (x - m) / torch.sqrt(v + 1e-5) * w[p + ".weight"] + w[p + ".bias"]


def _lin(w, p, x):
    y = x @ w[p + ".weight"].reshape(w[p + ".weight"].shape[0], -1).T
    return y + w[p + ".bias"] if p + ".bias" in w else y


def _swish(x):
    return x * torch.sigmoid(x)


def subsample(w, x):
    """x [T + 6, idim] (zero frames appended) -> [T', d] (:27-39)."""
    ip = "encoder.input_preprocessor"
    conv = lambda t, p: torch.relu(torch.nn.functional.conv2d(t, w[p + ".weight"].permute(0, 3, 1, 2), w[p + ".bias"], stride=2))
    h = conv(conv(x[None, None], ip + ".conv1"), ip + ".conv2")[0]       # [C, T', F']
    return _lin(w, ip + ".out", h.permute(1, 0, 2).reshape(h.shape[1], -1))


def _ffn(w, p, x):
    return _lin(w, p + ".net_4", _swish(_lin(w, p + ".net_1", _ln(x, w, p + ".net_0")))) + x


def _mhsa(w, p, x, pos_emb, H):
    T, d = x.shape
    dk = d // H
    q = _lin(w, p + ".w_qs", _ln(x, w, p + ".layer_norm_q")).reshape(T, H, dk)
    k = _lin(w, p + ".w_ks", _ln(x, w, p + ".layer_norm_k")).reshape(T, H, dk).transpose(0, 1)
    v = _lin(w, p + ".w_vs", _ln(x, w, p + ".layer_norm_v")).reshape(T, H, dk).transpose(0, 1)
    pp = _lin(w, p + ".linear_pos", pos_emb).reshape(-1, H, dk).transpose(0, 1)          # [H, 2T - 1, dk]
    ac = (q + w[p + ".pos_bias_u"]).transpose(0, 1) @ k.transpose(1, 2)
    bd = (q + w[p + ".pos_bias_v"]).transpose(0, 1) @ pp.transpose(1, 2)                  # [H, T, 2T - 1]
    T2 = bd.shape[-1]
    pad = torch.cat([torch.zeros((H, T, 1), dtype=F64), bd], -1).reshape(H, T2 + 1, T)   # _rel_shift (:142-149)
    bd = pad[:, 1:, :].reshape(H, T, T2)[:, :, :T2 // 2 + 1]
    att = torch.softmax((ac + bd) * (1.0 / dk ** 0.5), -1) @ v
    return _lin(w, p + ".fc", att.transpose(0, 1).reshape(T, d)) + x


def _conv(w, p, x, K):
    out = _lin(w, p + ".pointwise_conv1", _ln(x, w, p + ".pre_layer_norm"))
    a, b = out.chunk(2, -1)
    g = (a * torch.sigmoid(b)).T[None]
    out = torch.nn.functional.conv1d(g, w[p + ".depthwise_conv.weight"].permute(0, 2, 1), padding=(K - 1) // 2, groups=g.shape[1])[0].T
    out = _swish(_ln(out, w, p + ".batch_norm"))
    return _lin(w, p + ".pointwise_conv2", out) + x


def encode(w: dict, c: ModelConfig, feats) -> dict:
    """feats [T, idim] (after CMVN) -> dict(sub, attn0, conv0, layers, out), float64."""
    w = {k: v.to(F64) for k, v in w.items()}
    x = torch.cat([torch.as_tensor(feats).to(F64), torch.zeros((6, c.idim), dtype=F64)], 0)
    x = subsample(w, x)
    T, d = x.shape
    pos_emb = rel_pe_table(T, d).to(F64)
    st = dict(sub=x, layers=[])
    for i in range(c.encoder.n_layers):
        p = f"encoder.layer_stack.{i}"
        x = 0.5 * x + 0.5 * _ffn(w, p + ".ffn1", x)
        x = _mhsa(w, p + ".mhsa", x, pos_emb, c.encoder.n_head)
        if i == 0:
            st["attn0"] = x
        x = _conv(w, p + ".conv", x, c.encoder.kernel_size)
        if i == 0:
            st["conv0"] = x
        x = 0.5 * x + 0.5 * _ffn(w, p + ".ffn2", x)
        x = _ln(x, w, p + ".layer_norm")
        st["layers"].append(x)
    st["out"] = x
    return st


def _dec_attn(w, p, q_in, kv_in, H, mask=None):
    Tq, d = q_in.shape[-2:]
    dk = d // H
    sp = lambda t: t.reshape(*t.shape[:-1], H, dk).transpose(-2, -3)
    q, k, v = sp(_lin(w, p + ".w_qs", q_in)), sp(_lin(w, p + ".w_ks", kv_in)), sp(_lin(w, p + ".w_vs", kv_in))
    att = (q @ k.transpose(-1, -2)) * (1.0 / dk ** 0.5)
    if mask is not None:
        att = torch.where(mask, att, torch.tensor(-1e9, dtype=F64))
    att = torch.softmax(att, -1)
    out = (att @ v).transpose(-2, -3).reshape(*q_in.shape[:-1], d)
    return _lin(w, p + ".fc", out)


def decoder_logits(w, c: ModelConfig, ys, enc):
    """ys int [B, L], enc [T, d] -> logits of the last position [B, V] (the whole prefix recomputed: :391-405 without the caches)."""
    dc = c.decoder
    B, L = ys.shape
    x = w["decoder.tgt_word_emb.weight"][ys] * (dc.d_model ** 0.5) + abs_pe_table(L, dc.d_model).to(F64)
    mask = torch.tril(torch.ones((L, L), dtype=torch.bool))
    e = enc[None].expand(B, -1, -1)
    for i in range(dc.n_layers):
        p = f"decoder.layer_stack.{i}"
        xn = _ln(x, w, p + ".self_attn_norm")
        x = x + _dec_attn(w, p + ".self_attn", xn, xn, dc.n_head, mask)
        x = x + _dec_attn(w, p + ".cross_attn", _ln(x, w, p + ".cross_attn_norm"), e, dc.n_head)
        x = x + _lin(w, p + ".mlp.w_2", torch.nn.functional.gelu(_lin(w, p + ".mlp.w_1", _ln(x, w, p + ".mlp_norm"))))
    return _lin(w, "decoder.tgt_word_prj", _ln(x, w, "decoder.layer_norm_out")[:, -1])


def _topk(x, k):
    """Descending, ties to the lower index (the reference's argpartition leaves ties open; the engine's rule)."""
    idx = torch.argsort(-x, dim=-1, stable=True)[..., :k]
    return torch.gather(x, -1, idx), idx


def beam_search(w: dict, c: ModelConfig, enc, beam_size=3, max_len=0, softmax_smoothing=1.25, length_penalty=0.6, eos_penalty=1.0) -> dict:
    """:369-464 for one utterance in float64; per step the chosen ``beam_idx``, tokens, scores and the step's decision margin (the smallest gap
    between neighbours in the sorted top B + 1 of the B x B candidates and of each live beam's t)."""
    w = {k: v.to(F64) for k, v in w.items()}
    enc = torch.as_tensor(enc).to(F64)
    B = beam_size
    max_decode = max_len if max_len > 0 else enc.shape[0]
    ys = torch.full((B, 1), c.sos_id, dtype=torch.long)
    scores = torch.tensor([0.0] + [-INF] * (B - 1), dtype=F64).reshape(B, 1)
    fin = torch.zeros((B, 1), dtype=F64)
    conf = torch.zeros((B, 1), dtype=F64)
    steps = []
    for _ in range(max_decode):
        logits = decoder_logits(w, c, ys, enc)
        t = torch.log(torch.softmax(logits / float(np.float32(softmax_smoothing)), -1) + 1e-10)
        if eos_penalty != 1.0:
            t[:, c.eos_id] = t[:, c.eos_id] * float(np.float32(eos_penalty))
        top, idx = _topk(t, B)
        margin = INF
        srt = torch.sort(t, -1, descending=True).values
        for i in range(B):
            if not fin[i, 0] and srt.shape[1] > B:
                margin = min(margin, float((srt[i, :B] - srt[i, 1:B + 1]).min()))
        mask = torch.tensor([0.0] + [-INF] * (B - 1), dtype=F64).reshape(1, B).repeat(B, 1)
        top = top * (1 - fin) + mask * fin
        idx = idx * (1 - fin.long()) + c.eos_id * fin.long()
        allsc = (scores + top).reshape(B * B)
        best, bidx = _topk(allsc, B)
        s2 = torch.sort(allsc, descending=True).values
        live = s2[:B + 1][s2[:B + 1] > -1e9]
        if live.numel() > 1:
            margin = min(margin, float((live[:-1] - live[1:]).min()))
        scores = best.reshape(B, 1)
        beam = bidx // B
        new = idx.reshape(B * B)[bidx].reshape(B, 1)
        ys = torch.cat([ys[beam], new], 1)
        conf = torch.cat([conf[beam], torch.exp(top.reshape(B * B)[bidx]).reshape(B, 1)], 1)
        fin = (new == c.eos_id).to(F64)
        steps.append(dict(beam_idx=beam.tolist(), tokens=new[:, 0].tolist(), scores=scores[:, 0].tolist(), margin=margin))
        if fin.sum() == B:
            break
    ys_len = (ys != c.eos_id).sum(-1, keepdim=True).to(F64)
    final = scores / torch.pow((5.0 + ys_len) / 6.0, length_penalty) if length_penalty > 0.0 else scores
    best = int(torch.argmax(final.reshape(-1)))
    seq, cf = ys[best, 1:].tolist(), conf[best, 1:].tolist()
    if c.eos_id in seq:
        seq = seq[:seq.index(c.eos_id)]
    confidence = float(np.mean(cf[:len(seq)])) if seq else 0.0
    return dict(steps=steps, seq=seq, conf=cf, confidence=confidence, best=best,
                final_margin=float(torch.sort(final.reshape(-1), descending=True).values[:2].diff().abs().min()) if B > 1 else INF)


def detokenize(id2word, ids) -> str:
    import re

    text = "".join(id2word[int(i)] for i in ids if 0 <= int(i) < len(id2word)).replace("▁", " ").strip()
    return re.sub(r"(<blank>)|(<sil>)", "", text).lower()


def make_dict(odim: int):
    words = ["<blank>", "<unk>", "<pad>", "<sos>", "<eos>", "<space>", "<sil>"]
    return words + [("▁" if i % 3 == 0 else "") + "".join(chr(97 + (i * 7 + j) % 26).upper() for j in range(1 + i % 3)) for i in range(len(words), odim)]


# ------------------------------------------------------------------ fixtures of the reference's own runs and the checks both suites share
def load_fixtures():
    import json
    import os

    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    with open(os.path.join(here, "ref_fireredasr2.json")) as f:
        meta = json.load(f)
    return np.load(os.path.join(here, "ref_fireredasr2.npz")), meta


def write_side_files(tag: str, path: str, c: ModelConfig):
    """``dict.txt`` (both configurations) and ``cmvn.json`` (B) as the maker wrote them for the reference's ``post_load_hook``."""
    import json
    import os

    with open(os.path.join(path, "dict.txt"), "w", encoding="utf8") as f:
        f.write("".join(f"{wd} {i}\n" for i, wd in enumerate(make_dict(c.odim))))
    if CONFIGS[tag]["cmvn"]:
        mean, istd = cmvn_for(tag)
        with open(os.path.join(path, "cmvn.json"), "w") as f:
            json.dump(dict(means=mean.tolist(), istd=istd.tolist()), f)


def rel_err(got, want) -> float:
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.abs(got - want).max() / np.abs(want).max())


def check_encoder(model, z, tag, i, bar, *, feats=None, report=print):
    """The model's stages for clip i against the stored ones; ``feats`` None: the stored features (the CPU suite; the GPU suite passes its own)."""
    f = torch.from_numpy(z[f"{tag}{i}_feats"]) if feats is None else feats
    buf = torch.zeros((1, f.shape[0] + 6, f.shape[1]), dtype=torch.float32, device=model.device)
    buf[0, :f.shape[0]] = f.to(model.device)
    out, rows, st = model.encode_features(buf, [f.shape[0]], return_stages=True)
    worst = {}
    for key, got in (("sub", st["sub"]), ("attn0", st["attn0"]), ("conv0", st["conv0"]), ("enc", out)):
        r = z[f"{tag}{i}_{key}_rows"]
        worst[key] = rel_err(got[0, :rows[0]].cpu().numpy()[r], z[f"{tag}{i}_{key}"])
    r = z[f"{tag}{i}_enc_rows"]
    for l, got in enumerate(st["layers"]):
        worst[f"layer{l}"] = rel_err(got[0, :rows[0]].cpu().numpy()[r], z[f"{tag}{i}_layer{l}"])
    report(f"fireredasr2 {tag}{i}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert max(worst.values()) < bar, worst
    return out, rows


def check_run(model, z, run, enc, rows, family, *, report=print):
    """One stored ``generate`` run against the model's beam search on ``enc``: every decision before the first knife edge equal (``_margin.walk``),
    and, when no knife edge was met, the text, the token count and the confidence."""
    import _margin

    key, B = run["key"], run["beam"]
    hyps, trace = model.beam_search(enc, rows, beam_size=B, max_len=run.get("max_len", 0), return_trace=True)
    want_bi, want_tok, margins = z[f"{key}_beam_idx"], z[f"{key}_tokens"], z[f"{key}_margin"]
    live = [t for t in trace if not int(t["done_before"][0])]
    got, exp, mar = [], [], []
    for s in range(min(len(live), len(margins))):
        got += live[s]["beam_idx"][0].tolist() + live[s]["tokens"][0].tolist()
        exp += want_bi[s].tolist() + want_tok[s].tolist()
        mar += [float(margins[s])] * (2 * B)
    n = _margin.walk(family, got, exp, mar, where=key)
    if n == len(mar):
        assert len(live) == len(margins), (key, len(live), len(margins))
        sc = rel_err(live[-1]["scores"][0].numpy(), z[f"{key}_scores"][-1]) if len(live) else 0.0
        seq, conf = hyps[0]
        c = model.config
        if c.eos_id in seq:
            seq = seq[:seq.index(c.eos_id)]
        text = model._detokenize(seq)
        confidence = float(np.mean(np.asarray(conf[:len(seq)], dtype=np.float32))) if seq else 0.0
        assert text == run["text"] and len(seq) == run["generation_tokens"], (key, text, run["text"])
        assert abs(confidence - run["confidence"]) <= 2e-3 and sc < 1e-3, (key, confidence, run["confidence"], sc)
    report(f"fireredasr2 {key}: {n}/{len(mar)} decisions compared")
    return n, len(mar)


def to_torch_checkpoint(w: dict, tied: bool = True) -> dict:
    """The reference-named parameters back under the PyTorch checkpoint's names and layouts (what ``sanitize`` undoes); ``tied``: the output
    projection left out."""
    out = {}
    for k, v in w.items():
        if tied and k == "decoder.tgt_word_prj.weight":
            continue
        nk = k.replace("input_preprocessor.conv1.", "input_preprocessor.conv.0.").replace("input_preprocessor.conv2.", "input_preprocessor.conv.2.")
        nk = nk.replace(".net_", ".net.")
        if "pointwise_conv" in k or "depthwise_conv" in k:
            v = v.permute(0, 2, 1)
        elif "input_preprocessor.conv" in k and v.dim() == 4:
            v = v.permute(0, 3, 1, 2)
        out[nk] = v.contiguous()
    return out
