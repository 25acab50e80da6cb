"""DeepFilterNet2 / DeepFilterNet3 (``DfNet``, ``mlx_audio/sts/models/deepfilternet/network.py``) as a host schedule over HIP kernels.

Every tensor is channels-last ``[B, T, F, C]`` (the reference transposes to that layout around each conv and back); a right-padded batch carries
``lens`` and item ``b`` equals that item run alone: the convs read frames at and beyond ``lens[b]`` as zero, the GRUs stop there.

  * conv blocks (conv, optional pointwise conv, BatchNorm folded to scale / shift, ReLU / sigmoid, skip sum): ``ops.dfn_conv2d``, one launch per block;
  * grouped linears (block-diagonal dense images), GRU input projections, ``lsnr_fc``, ``df_out``: ``ops.conv_gemm`` with fp16 weight images;
  * the five GRU layers: ``ops.gru_seq``, one launch per layer for the whole batch;
  * mask, deep filter, assembly and the division by ``wnorm``: ``ops.dfn_apply``.

Checkpoints use the PyTorch names the reference's loader accepts (``weight_loader.py``): ``enc.emb_gru.gru.weight_ih_l0`` ..., ``erb_fb``,
``mask.erb_inv_fb``; ``num_batches_tracked`` and ``.h0`` entries are ignored.  ``df_dec.df_fc_a`` is loaded by the reference and never used by
``DfNet.__call__`` (``alpha`` is None): it is accepted and not computed."""
from __future__ import annotations

import math
from typing import Dict, Optional, Tuple

import torch

from .... import ops
from .config import DeepFilterNetConfig

BN_EPS = 1e-5


# ---------------------------------------------------------------------------------------------------------------- checkpoint layout
def _conv_groups(cin: int, cout: int, kernel, separable: bool) -> Tuple[int, bool]:
    """(groups, has pointwise) of ``Encoder._make_conv`` (network.py:249-279)."""
    groups = math.gcd(cin, cout) if separable else 1
    return groups, groups > 1


def _blocks(p: DeepFilterNetConfig) -> Dict[str, dict]:
    """Every conv block: checkpoint prefixes of its conv / pointwise / BatchNorm and its geometry."""
    C, O2 = p.conv_ch, 2 * p.df_order
    kin, kc, kt_ = tuple(p.conv_kernel_inp), tuple(p.conv_kernel), tuple(p.convt_kernel)
    out = {}

    def enc(name, cin, kernel, separable, fstride, idx0):   # idx0: checkpoint index of the conv (stride convs have no pad module in front)
        g, pw = _conv_groups(cin, C, kernel, separable)
        out[name] = dict(conv=f"{name}.{idx0}", pw=f"{name}.{idx0 + 1}" if pw else None, bn=f"{name}.{idx0 + (2 if pw else 1)}", cin=cin, cmid=C, cout=C,
                         groups=g, kernel=kernel, fstride=fstride, act=ops.DFN_ACT_RELU)

    enc("enc.erb_conv0", 1, kin, False, 1, 1)
    for i, fs in ((1, 2), (2, 2), (3, 1)):
        enc(f"enc.erb_conv{i}", C, kc, True, fs, 0)
    enc("enc.df_conv0", 2, kin, True, 1, 1)
    enc("enc.df_conv1", C, kc, True, 2, 0)
    for i in range(4):   # pathway convs: 1 x 1 depthwise + BatchNorm + ReLU (network.py:357-360,403-406)
        out[f"erb_dec.conv{i}p"] = dict(conv=f"erb_dec.conv{i}p.0", pw=None, bn=f"erb_dec.conv{i}p.1", cin=C, cmid=C, cout=C, groups=C, kernel=(1, 1),
                                        fstride=1, act=ops.DFN_ACT_RELU)
    out["erb_dec.convt3"] = dict(conv="erb_dec.convt3.0", pw="erb_dec.convt3.1", bn="erb_dec.convt3.2", cin=C, cmid=C, cout=C, groups=C, kernel=kt_,
                                 fstride=1, act=ops.DFN_ACT_RELU)
    for i in (2, 1):
        out[f"erb_dec.convt{i}"] = dict(conv=f"erb_dec.convt{i}.0", pw=f"erb_dec.convt{i}.1", bn=f"erb_dec.convt{i}.2", cin=C, cmid=C, cout=C, groups=C,
                                        kernel=kt_, fstride=2, transposed=True, act=ops.DFN_ACT_RELU)
    out["erb_dec.conv0_out"] = dict(conv="erb_dec.conv0_out.0", pw=None, bn="erb_dec.conv0_out.1", cin=C, cmid=1, cout=1, groups=1, kernel=kt_, fstride=1,
                                    act=ops.DFN_ACT_SIGMOID)
    out["df_dec.df_convp"] = dict(conv="df_dec.df_convp.1", pw="df_dec.df_convp.2", bn="df_dec.df_convp.3", cin=C, cmid=O2, cout=O2, groups=math.gcd(C, O2),
                                  kernel=(p.df_pathway_kernel_size_t, 1), fstride=1, act=ops.DFN_ACT_RELU)
    return out


def _dims(p: DeepFilterNetConfig) -> dict:
    conv_emb = p.conv_ch * p.nb_erb // 4
    return dict(conv_emb=conv_emb, emb_out=p.emb_hidden_dim if p.enc_concat else conv_emb, gru_in=2 * conv_emb if p.enc_concat else conv_emb,
                dec_in=p.emb_hidden_dim if p.enc_concat else conv_emb, erb_layers=max(1, p.emb_num_layers - 1))


def expected_shapes(p: DeepFilterNetConfig, with_erb_fb: bool = True) -> Dict[str, Tuple[int, ...]]:
    """Checkpoint name -> shape (PyTorch layouts)."""
    d, C, H, Hd = _dims(p), p.conv_ch, p.emb_hidden_dim, p.df_hidden_dim
    s: Dict[str, Tuple[int, ...]] = {}
    for b in _blocks(p).values():
        kt, kf = b["kernel"]
        if b.get("transposed"):
            s[b["conv"] + ".weight"] = (b["cin"], b["cmid"] // b["groups"], kt, kf)
        else:
            s[b["conv"] + ".weight"] = (b["cmid"], b["cin"] // b["groups"], kt, kf)
        if b["pw"]:
            s[b["pw"] + ".weight"] = (b["cout"], b["cmid"], 1, 1)
        for n in ("weight", "bias", "running_mean", "running_var"):
            s[f"{b['bn']}.{n}"] = (b["cout"],)

    def glin(name, n_in, n_out, groups):
        s[name] = (groups, n_in // groups, n_out // groups)

    def gru(prefix, n_in, hidden, layers, n_out, lin_groups):
        glin(f"{prefix}.linear_in.0.weight", n_in, hidden, lin_groups)
        for l in range(layers):
            s[f"{prefix}.gru.weight_ih_l{l}"] = s[f"{prefix}.gru.weight_hh_l{l}"] = (3 * hidden, hidden)
            s[f"{prefix}.gru.bias_ih_l{l}"] = s[f"{prefix}.gru.bias_hh_l{l}"] = (3 * hidden,)
        if n_out:
            glin(f"{prefix}.linear_out.0.weight", hidden, n_out, lin_groups)

    glin("enc.df_fc_emb.0.weight", C * p.nb_df // 2, d["conv_emb"], p.enc_linear_groups)
    gru("enc.emb_gru", d["gru_in"], H, 1, None if p.enc_concat else d["emb_out"], p.linear_groups)
    s["enc.lsnr_fc.0.weight"], s["enc.lsnr_fc.0.bias"] = (1, d["emb_out"]), (1,)
    gru("erb_dec.emb_gru", d["dec_in"], H, d["erb_layers"], d["conv_emb"], p.linear_groups)
    gru("df_dec.df_gru", d["dec_in"], Hd, p.df_num_layers, None, 8)
    if p.df_gru_skip == "groupedlinear":
        glin("df_dec.df_skip.weight", d["dec_in"], Hd, p.linear_groups)
    glin("df_dec.df_out.0.weight", Hd, p.nb_df * 2 * p.df_order, p.linear_groups)
    s["df_dec.df_fc_a.0.weight"], s["df_dec.df_fc_a.0.bias"] = (1, Hd), (1,)
    if with_erb_fb:
        s["erb_fb"] = (p.freq_bins, p.nb_erb)
    s["mask.erb_inv_fb"] = (p.nb_erb, p.freq_bins)
    return s


def check_config(p: DeepFilterNetConfig):
    """What this build runs; everything else is refused with the reason."""
    if p.model_version == "DeepFilterNet":
        raise NotImplementedError("DeepFilterNet (model_version 'DeepFilterNet', the reference's DfNetV1 in network_df1.py) is not built: DeepFilterNet2 and "
                                  "DeepFilterNet3 (DfNet) are")
    for name, h in (("emb_hidden_dim", p.emb_hidden_dim), ("df_hidden_dim", p.df_hidden_dim)):
        if h not in ops.GRU_SEQ_HIDDEN:
            raise NotImplementedError(f"DeepFilterNet: {name} = {h}: the GRU kernel holds hidden sizes {ops.GRU_SEQ_HIDDEN}")
    if p.nb_erb % 4 or p.nb_df % 2:
        raise ValueError(f"DeepFilterNet: nb_erb ({p.nb_erb}) must be a multiple of 4 and nb_df ({p.nb_df}) even (two frequency-stride-2 convs / one)")
    if tuple(p.conv_kernel)[1] != 3 or tuple(p.convt_kernel)[1] != 3 or tuple(p.conv_kernel_inp)[1] != 3:
        raise NotImplementedError("DeepFilterNet: the stride-2 / transposed geometry is built for frequency kernels of 3")
    if max(p.nb_erb, p.nb_df) > ops.DFN_MAX_BANDS or max(p.conv_ch, 2 * p.df_order) > ops.DFN_MAX_CH or p.nb_df > p.freq_bins:
        raise ValueError(f"DeepFilterNet: at most {ops.DFN_MAX_BANDS} bands / bins and {ops.DFN_MAX_CH} channels")
    if not 0 <= p.df_lookahead < p.df_order or p.conv_lookahead < 0:
        raise ValueError("DeepFilterNet: df_lookahead must lie in [0, df_order) and conv_lookahead be >= 0")


# ---------------------------------------------------------------------------------------------------------------- the schedule
def _dense_grouped(w: torch.Tensor) -> torch.Tensor:
    """GroupedLinearEinsum weight [G, ws, hs] (network.py:20-34) -> the block-diagonal nn.Linear image [G hs, G ws]."""
    G, ws, hs = w.shape
    out = torch.zeros(G * hs, G * ws, dtype=torch.float32)
    for g in range(G):
        out[g * hs:(g + 1) * hs, g * ws:(g + 1) * ws] = w[g].t()
    return out


class SqueezedGRU:
    """``SqueezedGRU`` (network.py:153-192): grouped linear + ReLU, GRU layers from a zero state, optional grouped linear + ReLU."""

    def __init__(self, w: Dict[str, torch.Tensor], prefix: str, layers: int, has_out: bool, device):
        lin = lambda name: ops.pack_conv(_dense_grouped(w[name]), None, device, f16=True)
        self.lin_in = lin(f"{prefix}.linear_in.0.weight")
        self.lin_out = lin(f"{prefix}.linear_out.0.weight") if has_out else None
        self.layers = []
        for l in range(layers):
            wih, whh = w[f"{prefix}.gru.weight_ih_l{l}"], w[f"{prefix}.gru.weight_hh_l{l}"]
            bih, bhh = w[f"{prefix}.gru.bias_ih_l{l}"], w[f"{prefix}.gru.bias_hh_l{l}"]
            H = whh.shape[1]
            b = bih + torch.cat([bhh[:2 * H], torch.zeros(H)])   # PyTorch's bias_hh r / z parts fold into b (weight_loader.py:174-196)
            self.layers.append((ops.pack_conv(wih, b, device, f16=True), ops.pack_gru_wh(whh, device), bhh[2 * H:].contiguous().to(device)))
        self.hidden = self.layers[0][1].h

    def __call__(self, x: torch.Tensor, lens_d: Optional[torch.Tensor]) -> torch.Tensor:
        B, T, _ = x.shape
        new = lambda n: torch.zeros((B, T, n), dtype=torch.float32, device=x.device)
        h = ops.conv_gemm(x, self.lin_in, new(self.hidden), post_act=ops.ACT_LEAKY, post_slope=0.0, precision=4, lens_in=lens_d, lens_out=lens_d)
        for wx, wh, bhn in self.layers:
            xp = ops.conv_gemm(h, wx, new(3 * self.hidden), precision=4, lens_in=lens_d, lens_out=lens_d)
            h = ops.gru_seq(xp, wh, bhn, new(self.hidden), lens=lens_d)
        if self.lin_out is not None:
            h = ops.conv_gemm(h, self.lin_out, new(self.lin_out.cout), post_act=ops.ACT_LEAKY, post_slope=0.0, precision=4, lens_in=lens_d, lens_out=lens_d)
        return h


def _conv_table(p: DeepFilterNetConfig, w: Dict[str, torch.Tensor], device, prefix: str) -> Dict[str, "ops.DfnConv"]:
    """The conv blocks whose checkpoint names start with ``prefix``, BatchNorm folded to scale / shift, on the device."""
    dev = lambda t: t.to(torch.float32).contiguous().to(device)
    out = {}
    for name, b in _blocks(p).items():
        if not name.startswith(prefix):
            continue
        bn = {n: w[f"{b['bn']}.{n}"] for n in ("weight", "bias", "running_mean", "running_var")}
        scale = bn["weight"] / torch.sqrt(bn["running_var"] + BN_EPS)
        shift = bn["bias"] - bn["running_mean"] * scale
        out[name[len(prefix):]] = ops.DfnConv(w=dev(w[b["conv"] + ".weight"]), cin=b["cin"], cmid=b["cmid"], cout=b["cout"], groups=b["groups"], kt=b["kernel"][0],
                                              kf=b["kernel"][1], fstride=b["fstride"], transposed=bool(b.get("transposed")),
                                              pw=dev(w[b["pw"] + ".weight"].reshape(b["cout"], b["cmid"])) if b["pw"] else None, scale=dev(scale), shift=dev(shift),
                                              act=b["act"])
    return out


def _zeros(x: torch.Tensor, n: int) -> torch.Tensor:
    return torch.zeros((x.shape[0], x.shape[1], n), dtype=torch.float32, device=x.device)


def _gemm(x, pc, y, lens_d, **kw):
    return ops.conv_gemm(x, pc, y, precision=4, lens_in=lens_d, lens_out=lens_d, **kw)


class Encoder:
    """``Encoder`` (network.py:195-319): the ERB and DF conv stacks, ``df_fc_emb``, the embedding GRU and ``lsnr_fc``."""

    def __init__(self, p: DeepFilterNetConfig, w: Dict[str, torch.Tensor], device):
        self.p, self.n = p, _dims(p)["conv_emb"]
        self.convs = _conv_table(p, w, device, "enc.")
        self.df_fc_emb = ops.pack_conv(_dense_grouped(w["enc.df_fc_emb.0.weight"]), None, device, f16=True)
        self.emb_gru = SqueezedGRU(w, "enc.emb_gru", 1, not p.enc_concat, device)
        self.lsnr_fc = ops.pack_conv(w["enc.lsnr_fc.0.weight"], w["enc.lsnr_fc.0.bias"], device, f16=True)

    def __call__(self, feat_erb: torch.Tensor, feat_df: torch.Tensor, lens_d: Optional[torch.Tensor]):
        """feat_erb [B, T, E, 1], feat_df [B, T, D, 2] -> (e0, e1, e2, e3, emb, c0, lsnr), the reference's order; c1 rides along last."""
        p, n = self.p, self.n
        B, T = feat_erb.shape[:2]
        conv = lambda name, x: ops.dfn_conv2d(x, self.convs[name], lens=lens_d)
        e0 = conv("erb_conv0", feat_erb)
        e1 = conv("erb_conv1", e0)
        e2 = conv("erb_conv2", e1)
        e3 = conv("erb_conv3", e2)
        c0 = conv("df_conv0", feat_df)
        c1 = conv("df_conv1", c0)
        e3f, c1f = e3.reshape(B, T, -1), c1.reshape(B, T, -1)
        if p.enc_concat:
            emb_in = _zeros(e3f, 2 * n)
            emb_in[:, :, :n] = e3f
            _gemm(c1f, self.df_fc_emb, emb_in[:, :, n:], lens_d, post_act=ops.ACT_LEAKY, post_slope=0.0)
        else:
            emb_in = _gemm(c1f, self.df_fc_emb, _zeros(e3f, n), lens_d, post_act=ops.ACT_LEAKY, post_slope=0.0, res=e3f)
        emb = self.emb_gru(emb_in, lens_d)
        lsnr = torch.sigmoid(_gemm(emb, self.lsnr_fc, _zeros(emb, 1), lens_d)) * float(p.lsnr_max - p.lsnr_min) + float(p.lsnr_min)
        return e0, e1, e2, e3, emb, c0, lsnr, c1


class ErbDecoder:
    """``ErbDecoder`` (network.py:322-417): every pathway block adds the tensor coming up AFTER its ReLU."""

    def __init__(self, p: DeepFilterNetConfig, w: Dict[str, torch.Tensor], device):
        self.f8 = p.nb_erb // 4
        self.convs = _conv_table(p, w, device, "erb_dec.")
        self.emb_gru = SqueezedGRU(w, "erb_dec.emb_gru", _dims(p)["erb_layers"], True, device)

    def __call__(self, emb, e3, e2, e1, e0, lens_d: Optional[torch.Tensor]) -> torch.Tensor:
        B, T = emb.shape[:2]
        conv = lambda name, x, add=None: ops.dfn_conv2d(x, self.convs[name], add=add, lens=lens_d)
        d3 = conv("convt3", conv("conv3p", e3, self.emb_gru(emb, lens_d).reshape(B, T, self.f8, -1)))
        d2 = conv("convt2", conv("conv2p", e2, d3))
        d1 = conv("convt1", conv("conv1p", e1, d2))
        return conv("conv0_out", conv("conv0p", e0, d1))                          # m [B, T, E, 1]


class DfDecoder:
    """``DfDecoder`` (network.py:420-482): the DF GRUs, the pathway conv on c0, ``df_out`` with the pathway tensor added behind its tanh."""

    def __init__(self, p: DeepFilterNetConfig, w: Dict[str, torch.Tensor], device):
        self.p = p
        self.convs = _conv_table(p, w, device, "df_dec.")
        self.df_gru = SqueezedGRU(w, "df_dec.df_gru", p.df_num_layers, False, device)
        lin = lambda name: ops.pack_conv(_dense_grouped(w[name]), None, device, f16=True)
        self.df_skip = lin("df_dec.df_skip.weight") if p.df_gru_skip == "groupedlinear" else None
        self.df_out = lin("df_dec.df_out.0.weight")

    def __call__(self, emb: torch.Tensor, c0: torch.Tensor, lens_d: Optional[torch.Tensor]) -> torch.Tensor:
        p = self.p
        B, T = emb.shape[:2]
        c = self.df_gru(emb, lens_d)
        if self.df_skip is not None:
            _gemm(emb, self.df_skip, c, lens_d, accumulate=True)
        c0p = ops.dfn_conv2d(c0, self.convs["df_convp"], lens=lens_d)             # [B, T, D, 2 order]
        coef = _gemm(c, self.df_out, _zeros(c, p.nb_df * 2 * p.df_order), lens_d, post_act=ops.ACT_TANH, res=c0p.reshape(B, T, -1))
        return coef.reshape(B, T, p.nb_df, p.df_order, 2)


class DfNet:
    """``DfNet`` (network.py:739-806).  ``weights``: a validated checkpoint (float32 CPU tensors under the PyTorch names)."""

    def __init__(self, config: DeepFilterNetConfig, weights: Dict[str, torch.Tensor], device):
        check_config(config)
        self.config, self.device = config, torch.device(device)
        self.enc = Encoder(config, weights, self.device)
        self.erb_dec = ErbDecoder(config, weights, self.device)
        self.df_dec = DfDecoder(config, weights, self.device)
        self.erb_inv_fb = weights["mask.erb_inv_fb"].to(torch.float32).contiguous().to(self.device)

    def __call__(self, spec: torch.Tensor, feat_erb: torch.Tensor, feat_df: torch.Tensor, lens_d: Optional[torch.Tensor] = None, *, wnorm: float = 1.0,
                 return_stages: bool = False):
        """spec [B, T, F, 2] (re, im; already times ``wnorm``), feat_erb [B, T, E, 1], feat_df [B, T, D, 2] (both behind the look-ahead shift) ->
        (spec_e, m, lsnr, df_coefs) like the reference: spec_e complex64 [B, T, F] = the enhanced spectrum / ``wnorm``, m [B, 1, T, E],
        lsnr [B, T, 1] (returned, not used), df_coefs [B, order, T, D, 2].  ``return_stages``: also a dict of the stage tensors (``emb`` [B, T, emb_out], ...)."""
        p = self.config
        B, T = spec.shape[:2]
        e0, e1, e2, e3, emb, c0, lsnr, c1 = self.enc(feat_erb, feat_df, lens_d)
        m = self.erb_dec(emb, e3, e2, e1, e0, lens_d)
        coef = self.df_dec(emb, c0, lens_d)
        spec_e = ops.dfn_apply(spec, m.reshape(B, T, p.nb_erb), self.erb_inv_fb, coef, order=p.df_order, df_lookahead=p.df_lookahead,
                               mask_first=p.enc_concat, wnorm=wnorm, lens=lens_d)
        out = (spec_e, m.permute(0, 3, 1, 2), lsnr, coef.permute(0, 3, 1, 2, 4))
        if return_stages:
            return out, dict(e0=e0, e1=e1, e2=e2, e3=e3, c0=c0, c1=c1, emb=emb, m=m, lsnr=lsnr, df_coefs=coef)
        return out
