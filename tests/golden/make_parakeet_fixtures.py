#!/usr/bin/env python
"""Runs the reference's OWN ``stt/models/parakeet/attention.py``, ``conformer.py``, ``ctc.py``, ``tokenizer.py``, ``stt/models/nemo/alignment.py`` and
``ParakeetCTC.decode`` (``parakeet.py``), unmodified and imported from where they lie, over the numpy stand-in for MLX (``mlx_shim.py``, left as it is) on
seeded checkpoints and stores what they compute in ``tests/golden/ref_parakeet_ctc.npz``.

The stand-in lacks ``nn.Conv2d``, ``nn.BatchNorm``, ``nn.glu``, ``nn.SiLU`` and ``nn.ReLU``: added here at run time (Conv2d through
``torch.nn.functional.conv2d`` on the MLX [O, kh, kw, I] layout, BatchNorm on its running statistics).  ``parakeet.py`` imports the hub client, tqdm
and the package's loaders at module level; none of them is on the ``decode`` path and each gets an empty stand-in module.

The reference runs ONE un-padded sequence per call (attention.py:119 reshapes the batch-1 position projection to the batch size): every clip goes
through it alone.

  * config ``A``: feat_in 16, d_model 128, 2 heads (dh 64), 2 layers, K 9, 32 conv channels, factor 8; mels of 1601, 203, 41, 9 and 1 frames;
  * config ``B``: feat_in 80, d_model 256, 2 heads (dh 128), 1 layer, K 31, 32 conv channels, factor 8, ``xscaling``, ``use_bias=False``; 203 and 64 frames;
  * for every clip except the 1601-frame one: the subsampler's output, every layer's output, layer 0's attention-module and convolution-module outputs;
  * for every clip: the frame arg-max ids, the float32 top-2 gap of the log-probabilities per frame, ``out_lengths`` and the decode result (token ids,
    ``start``, ``duration``, text, sentence texts -- ``ref_parakeet_ctc.json``);
  * scripted inputs for the tokenizer, the alignment helpers and the CTC collapse (``a, blank, a``; all blank; a trailing special token; one frame).
The mels are NOT stored: they are regenerated from their seeds (``tests/_parakeet_ref.synth_mel``); the file holds each one's float64 sum and sum of squares.

Asserted before anything is written: at most 2 % of all frames have a top-2 gap below ``tests/_margin.THR``; between 20 % and 80 % of the frames are
blank; the ids hold a repeat and an ``a, blank ..., a`` pattern; a literal pad / reshape ``rel_shift`` equals ``bd[i, T - 1 - i + j]``.

Only runs where the reference lies: ``python tests/golden/make_parakeet_fixtures.py``."""
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_reference_fixtures as M  # noqa: E402  (installs the stand-in)
import _margin  # noqa: E402
import _parakeet_ref as R  # noqa: E402

mx, nn, _np = M.mx, M.nn, M._np


class Conv2d(nn.Module):
    """``mlx.nn.Conv2d``: channels-last input [N, H, W, C], weight [O, kh, kw, I / groups]."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias=True):
        super().__init__()
        k = (kernel_size, kernel_size) if isinstance(kernel_size, int) else tuple(kernel_size)
        s = (1.0 / (in_channels * k[0] * k[1])) ** 0.5
        self.weight = mx.random.uniform(-s, s, (out_channels, k[0], k[1], in_channels // groups))
        if bias:
            self.bias = mx.zeros((out_channels,))
        self.stride, self.padding, self.dilation, self.groups = stride, padding, dilation, groups

    def __call__(self, x):
        xt = torch.from_numpy(np.ascontiguousarray(np.asarray(x), dtype=np.float32)).permute(0, 3, 1, 2)
        wt = torch.from_numpy(np.ascontiguousarray(np.asarray(self.weight), dtype=np.float32)).permute(0, 3, 1, 2)
        bt = torch.from_numpy(np.asarray(self.bias, dtype=np.float32)) if "bias" in self.__dict__ else None
        y = torch.nn.functional.conv2d(xt, wt, bt, stride=self.stride, padding=self.padding, dilation=self.dilation, groups=self.groups)
        return mx.array(y.permute(0, 2, 3, 1).contiguous().numpy())


class BatchNorm(nn.Module):
    """``mlx.nn.BatchNorm`` in inference (``Model.from_config`` calls ``model.eval()``): the running statistics."""

    def __init__(self, num_features, eps=1e-5, momentum=0.1, affine=True, track_running_stats=True):
        super().__init__()
        self.eps = eps
        self.weight, self.bias = mx.ones((num_features,)), mx.zeros((num_features,))
        self.running_mean, self.running_var = mx.zeros((num_features,)), mx.ones((num_features,))

    def __call__(self, x):
        assert not self.training, "the fixtures run the model in eval()"
        x = np.asarray(x)
        y = (x - np.asarray(self.running_mean)) * (1.0 / np.sqrt(np.asarray(self.running_var) + np.float32(self.eps)))
        return mx.array((y * np.asarray(self.weight) + np.asarray(self.bias)).astype(np.float32))


def _glu(x, axis=-1):
    a, b = np.split(np.asarray(x), 2, axis=axis)
    return mx.array((a * (1.0 / (1.0 + np.exp(-b)))).astype(np.float32))


class SiLU(nn.Module):
    def __call__(self, x):
        return nn.silu(x)


class ReLU(nn.Module):
    def __call__(self, x):
        return nn.relu(x)


for _name, _obj in (("Conv2d", Conv2d), ("BatchNorm", BatchNorm), ("glu", _glu), ("SiLU", SiLU), ("ReLU", ReLU)):
    if not hasattr(nn, _name):
        setattr(nn, _name, _obj)


def load_reference():
    M.import_reference()
    utils = sys.modules["mlx_audio.utils"]
    for name in ("STR_TO_WINDOW_FN", "bartlett", "blackman", "hamming", "hanning", "mel_filters", "stft", "from_dict", "base_load_model", "get_model_path", "load_config"):
        if not hasattr(utils, name):
            setattr(utils, name, getattr(sys.modules["mlx_audio.dsp"], name, None))
    for pkg, path in (("mlx_audio.stt", "stt"), ("mlx_audio.stt.models", "stt/models"), ("mlx_audio.stt.models.nemo", "stt/models/nemo"),
                      ("mlx_audio.stt.models.parakeet", "stt/models/parakeet")):
        if pkg not in sys.modules:
            M._pkg(pkg, f"{M.REF}/{path}")
    for name, attrs in (("huggingface_hub", ("hf_hub_download", "snapshot_download")), ("tqdm", ("tqdm",)), ("mlx_audio.stt.utils", ("load_audio",))):
        if name not in sys.modules:
            mod = types.ModuleType(name)
            for a in attrs:
                setattr(mod, a, None)
            sys.modules[name] = mod
    base = f"{M.REF}/stt/models"
    out = dict(alignment=M._load("mlx_audio.stt.models.nemo.alignment", f"{base}/nemo/alignment.py"))
    for name in ("tokenizer", "audio", "attention", "conformer", "ctc", "rnnt", "parakeet"):
        out[name] = M._load(f"mlx_audio.stt.models.parakeet.{name}", f"{base}/parakeet/{name}.py")
    return out


def check_rel_shift(ref):
    """The reference's own ``rel_shift`` (pad / reshape) against the index formula the kernel uses."""
    att = ref["attention"].RelPositionMultiHeadAttention(2, 128)
    g = np.random.default_rng(3)
    for T in (1, 2, 5, 33):
        bd = g.standard_normal((1, 2, T, 2 * T - 1)).astype(np.float32)
        got = np.asarray(att.rel_shift(mx.array(bd)))[:, :, :, :T]
        i, j = np.arange(T)[:, None], np.arange(T)[None, :]
        assert np.array_equal(got, bd[:, :, i, T - 1 - i + j]), T


def build(ref, enc, seed_w, blank_bias):
    from mlx_audio_amd.stt.models.parakeet.parakeet import make_parakeet_weights

    P = ref["parakeet"]
    cfg = R.config_dict(enc)
    args = P.ParakeetCTCArgs(preprocessor=ref["audio"].PreprocessArgs(**cfg["preprocessor"]), encoder=ref["conformer"].ConformerArgs(**cfg["encoder"]),
                             decoder=ref["ctc"].ConvASRDecoderArgs(**cfg["decoder"]), decoding=P.CTCDecodingArgs(**cfg["decoding"]))
    model = P.ParakeetCTC(args)
    w = make_parakeet_weights(R.make_args(enc), seed_w, head_gain=R.HEAD_GAIN, blank_bias=blank_bias)
    model.load_weights([(k, mx.array(v.numpy())) for k, v in w.items()], strict=True)
    missing, unexpected, mism = model._load_report
    assert not missing and not unexpected and not mism, (missing, unexpected, mism)
    model.eval()
    return model, w


def run_clip(ref, model, mel, stages):
    """The reference on ONE un-padded mel [T, feat]: ``Conformer.__call__`` stepped through its own modules so that intermediate tensors can be kept,
    checked against the module's own call; then ``ParakeetCTC.decode``."""
    enc = model.encoder
    x = mx.array(mel[None])
    hidden, lengths = enc(mx.array(mel[None].copy()))
    hidden = _np(hidden).copy()
    logp = _np(model.decoder(mx.array(hidden))).astype(np.float32)[0]
    top = np.sort(logp, axis=-1)
    out = dict(ids=logp.argmax(-1).astype(np.int32), gap=(top[:, -1] - top[:, -2]).astype(np.float32), out_len=int(np.asarray(lengths)[0]))
    assert out["out_len"] == hidden.shape[1] == len(out["ids"])
    if stages:
        y, _ = enc.pre_encode(x, mx.array(np.array([mel.shape[0]], dtype=np.float32)))
        y, pos_emb = enc.pos_enc(y, offset=0)
        out["pre_encode"] = _np(y).copy()[0]
        layers = []
        for i, layer in enumerate(enc.layers):
            if i == 0:
                y0 = mx.array(_np(y).copy())
                y0 = y0 + 0.5 * layer.feed_forward1(layer.norm_feed_forward1(y0))
                xn = layer.norm_self_att(y0)
                att = layer.self_attn(xn, xn, xn, pos_emb=pos_emb)
                out["attn0"] = _np(att).copy()[0]
                y0 = y0 + att
                out["conv0"] = _np(layer.conv(layer.norm_conv(y0))).copy()[0]
            y = layer(mx.array(_np(y).copy()), pos_emb=pos_emb)
            layers.append(_np(y).copy()[0])
        assert np.array_equal(layers[-1], hidden[0]), "the stepped encoder is not the module's own call"
        out["layers"] = np.stack(layers)
    res = model.decode(mx.array(mel[None].copy()))
    assert len(res) == 1
    return out, R.result_dict(res[0])


def scripted(ref, model):
    """Tokenizer, alignment helpers and the collapse of ``ParakeetCTC.decode`` on scripted frame ids (the encoder and head replaced by a table look-up)."""
    tok, al = ref["tokenizer"], ref["alignment"]
    V = len(R.VOCAB)
    out = dict(special=[bool(tok.is_special_token(i, R.VOCAB)) for i in range(-1, V + 2)],
               decode_all=tok.decode(list(range(-1, V + 2)), R.VOCAB), decode_some=tok.decode([1, 5, 3, 4, 0, 15, 2, 6], R.VOCAB))
    toks = [al.AlignedToken(i, tok.decode([i], R.VOCAB), 0.08 * n, 0.08) for n, i in enumerate([1, 5, 14, 9, 1, 11, 4, 16, 18, 21, 12, 2, 6, 8, 1, 4, 3, 4, 10])]
    out["sentences"] = R.result_dict(al.sentences_to_result(al.tokens_to_sentences(toks)))
    out["sentences_in"] = [int(t.id) for t in toks]
    out["sentences_empty"] = R.result_dict(al.sentences_to_result(al.tokens_to_sentences([])))
    rows = dict(a_blank_a=[5, V, 5, V, 6, 6, V, 5], all_blank=[V, V, V, V], trailing_special=[1, 1, V, 5, 15, 15, V], single=[7], single_blank=[V],
                special_first=[0, 0, 5, V, 5, 4, V, V], mixed=[1, V, V, 5, 5, 14, V, 4, 1, 6, 8, V, V])
    enc, dec = model.encoder, model.decoder
    out["collapse"] = {}
    for name, ids in rows.items():
        n = len(ids)
        model.encoder = lambda mel, n=n: (mx.array(np.zeros((1, n, 1), dtype=np.float32)), mx.array(np.array([n], dtype=np.int32)))
        model.decoder = lambda feats, ids=ids: mx.array(np.eye(V + 1, dtype=np.float32)[np.array(ids)][None])
        out["collapse"][name] = dict(frames=ids, result=R.result_dict(model.decode(mx.array(np.zeros((1, 8 * n, 1), dtype=np.float32)))[0]))
    model.encoder, model.decoder = enc, dec
    return out


def main():
    ref = load_reference()
    check_rel_shift(ref)
    out, meta = {}, dict(vocab=R.VOCAB, configs={})
    all_ids, all_gap = [], []
    first_model = None
    for tag, c in R.CONFIGS.items():
        model, _ = build(ref, c["enc"], c["seed_w"], c["blank_bias"])
        first_model = first_model or model
        meta["configs"][tag] = dict(enc=c["enc"], seed_w=c["seed_w"], blank_bias=c["blank_bias"], clips=[list(x) for x in c["clips"]], decode=[])
        for i, (frames, seed) in enumerate(c["clips"]):
            mel = R.synth_mel(seed, c["enc"]["feat_in"], frames)
            out[f"{tag}{i}_melsum"] = np.array([mel.astype(np.float64).sum(), (mel.astype(np.float64) ** 2).sum()])
            r, dec = run_clip(ref, model, mel, stages=frames <= 1000)
            for k, v in r.items():
                out[f"{tag}{i}_{k}"] = np.asarray(v)
            meta["configs"][tag]["decode"].append(dec)
            all_ids.append(r["ids"])
            all_gap.append(r["gap"])
            print(tag, i, frames, "->", r["out_len"], "frames;", repr(dec["text"][:60]))
    meta["scripted"] = scripted(ref, first_model)
    ids, gap, blank = np.concatenate(all_ids), np.concatenate(all_gap), len(R.VOCAB)
    share, blank_share = float((gap < _margin.THR).mean()), float((ids == blank).mean())
    repeat = any(bool((s[1:] == s[:-1]).any() and (s[1:][s[1:] == s[:-1]] != blank).any()) for s in all_ids if len(s) > 1)

    def aba(s):
        last = None
        seen_blank = False
        for t in s.tolist():
            if t == blank:
                seen_blank = last is not None
                continue
            if seen_blank and t == last:
                return True
            last, seen_blank = t, False
        return False

    print("frames", len(ids), "gap <", _margin.THR, ":", share, " < 1e-2:", float((gap < 1e-2).mean()), " blank share:", blank_share, " repeat:", repeat,
          " a-blank-a:", any(aba(s) for s in all_ids))
    assert share <= 0.02, share
    assert 0.2 <= blank_share <= 0.8, blank_share
    assert repeat and any(aba(s) for s in all_ids)
    path = os.path.join(HERE, "ref_parakeet_ctc.npz")
    np.savez_compressed(path, **out)
    with open(os.path.join(HERE, "ref_parakeet_ctc.json"), "w") as f:
        json.dump(meta, f, ensure_ascii=False, indent=1)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= 1_140_000


if __name__ == "__main__":
    main()
