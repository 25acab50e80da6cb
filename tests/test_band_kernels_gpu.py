"""``csrc/bandsplit.hip`` against float64 on the host (``tests/_ops_emu_melroformer.py``): ``band_split``, ``band_merge`` and ``head_gate``.  Every element
is compared; the bars are float32 rounding bounds (u = 2^-24) times the sum of the absolute terms behind the element, derived in the docstrings
and not tuned; the measured maxima are written next to them."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _ops_emu_melroformer as E  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RATIOS = {}
T_CASES = [1, 2, 16, 17, 63, 64, 65]   # 16 frames per workgroup: one frame, a partial tile, a full one, one more, and the same around four tiles


def _note(name, ratio):
    RATIOS[name] = max(RATIOS.get(name, 0.0), ratio)
    print(f"{name}: error / bar = {ratio:.3f} (largest so far {RATIOS[name]:.3f})")


def _tables(kind):
    """(list of CaC index lists, F).  ``hand``: a band of one bin (bd 4), a band of 130 bins (bd 520), non-contiguous and unsorted indices, bin 70 in
    three bands, bin 140 in none, one channel of a bin without the other."""
    if kind in ("A", "B"):
        npz = np.load(os.path.join(GOLD, "ref_melroformer.npz"))
        with open(os.path.join(GOLD, "ref_melroformer.json")) as f:
            kw = json.load(f)["configs"][kind]["kw"]
        ptr, idx = npz[f"{kind}_band_ptr"], npz[f"{kind}_band_idx"]
        return [idx[ptr[n]:ptr[n + 1]].tolist() for n in range(len(ptr) - 1)], kw["n_fft"] // 2 + 1
    pair = lambda bins: [j for b in bins for j in (2 * b, 2 * b + 1)]
    bands = [pair([0]), pair(range(1, 131)), pair([70, 135, 3, 137, 131]), pair([139, 70, 141, 142]) + [2 * 143], pair(range(132, 135)) + [2 * 143 + 1, 2 * 136]]
    return bands, 144


def _weights(bands, D, g):
    from mlx_audio_amd import ops

    ws = [torch.randn(D, 2 * len(ix), generator=g) / (2 * len(ix)) ** 0.5 for ix in bands]
    gs = [1 + 0.1 * torch.randn(2 * len(ix), generator=g) for ix in bands]
    bs = [torch.randn(D, generator=g) for _ in bands]
    return ops.pack_band_split(ws, gs, bs, "cpu")


def _strided_spec(spec, misalign):
    """The same values behind a larger channel stride and frame stride, the base pointer ``misalign`` floats off a 16-byte boundary."""
    B2, T, F, _ = spec.shape
    ts, cs = 2 * F + 6, T * (2 * F + 6) + 10
    buf = torch.full((B2 * cs + 8,), float("nan"), device=DEV)
    v = buf[misalign:].as_strided((B2, T, F, 2), (cs, ts, 2, 1))
    v.copy_(spec)
    return v


# ---------------------------------------------------------------------------------------------------------------- band_split
@pytest.mark.parametrize("T", T_CASES)
@pytest.mark.parametrize("kind", ["A", "B", "hand"])
def test_band_split(kind, T):
    """Bar per element: (1.5 bd_n + 8) u (sum_k |W[d, k] v[k]| + |bias[d]|).  ||u||^2 is a sum of bd_n squares, relative error at most (bd_n + 1) u,
    halved by the square root; the root, the division, sqrt(bd_n) and the two products add 5 u: v[k] carries (bd_n / 2 + 6) u.  The dot product
    is a sequential chain of bd_n FMAs, bd_n u of the absolute sum, and the bias add and the float32 store 2 u more.
    Measured on MI355X over all cases: largest error / bar 0.26.
    B = 1 and 2, D = 8 and 300 (more than one pass of the 256 threads, no multiple of 64), frames of exact zeros, strided and misaligned views."""
    from mlx_audio_amd import ops

    bands, F = _tables(kind)
    g = torch.Generator().manual_seed(100 * T + len(bands))
    for B, D, strided in ((1, 300, False), (2, 8, True)):
        tab = ops.band_tables(bands, F, DEV)
        tab_h = ops.band_tables(bands, F, "cpu")
        wt, gamma, bias = _weights(bands, D, g)
        spec = torch.randn(B * 2, T, F, 2, generator=g) * (torch.rand(B * 2, T, 1, 1, generator=g) * 3 + 0.01)
        zero_t = [t for t in (0, T // 2) if T > 1 or t == 0][:1 if T == 1 else 2]
        spec[:, zero_t] = 0.0                                                   # digital silence: whole frames of zeros on every channel
        ref, mag = E.band_split64(spec, tab_h, wt, gamma, bias)
        sd = _strided_spec(spec, 1) if strided else spec.to(DEV)
        outs = [ops.band_split(sd, tab, wt.to(DEV), gamma.to(DEV), bias.to(DEV)) for _ in range(2)]
        torch.cuda.synchronize()
        assert torch.equal(outs[0], outs[1])                                    # two calls, the same bits
        y = outs[0].cpu()
        assert y.shape == (B, T, len(bands), D) and torch.isfinite(y).all()
        assert torch.equal(y[:, zero_t], bias.expand(B, len(zero_t), -1, -1))   # exactly the bias rows, not NaN
        bd = torch.tensor(tab_h.band_dims, dtype=torch.float64)[None, None, :, None]
        bar = (1.5 * bd + 8) * U * mag
        err = (y.double() - ref).abs()
        _note(f"band_split[{kind}]", float((err / bar).max()))
        assert torch.all(err <= bar)


def test_band_split_refuses_without_a_launch():
    from mlx_audio_amd import _lib, ops

    F, T, D = 260, 3, 8
    bands = [[j for b in range(241) for j in (2 * b, 2 * b + 1)], [4, 5]]       # bd 964 > 960
    tab = ops.band_tables(bands, F, DEV)
    g = torch.Generator().manual_seed(0)
    wt, gamma, bias = (t.to(DEV) for t in _weights(bands, D, g))
    spec = torch.randn(2, T, F, 2, generator=g).to(DEV)
    y = torch.full((1, T, 2, D), 7.0, device=DEV)
    with pytest.raises(_lib.Mi355Error, match="at most 960"):
        ops.band_split(spec, tab, wt, gamma, bias, y=y)
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())                                               # nothing ran
    ok = ops.band_tables([[0, 1]], F, DEV)
    with pytest.raises(_lib.Mi355Error, match="bad spectrum strides"):
        _lib.call_struct("mi355_band_split", "mi355_band_split_args", 0, spec=spec.data_ptr(), spec_cstride=10, spec_tstride=2 * F, band_ptr=ok.ptr_d.data_ptr(),
                         band_idx=ok.idx_d.data_ptr(), n_idx=2, max_band_dim=4, wt=wt.data_ptr(), gamma=gamma.data_ptr(), bias=bias.data_ptr(), B=1, T=T, F=F,
                         Nb=1, D=D, y=y.data_ptr(), y_bstride=T * D)
    with pytest.raises(_lib.Mi355Error, match="null tensor"):
        _lib.call_struct("mi355_band_split", "mi355_band_split_args", 0, spec=spec.data_ptr(), B=1, T=T, F=F, Nb=1, D=D)
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())


# ---------------------------------------------------------------------------------------------------------------- band_merge
@pytest.mark.parametrize("T", T_CASES)
@pytest.mark.parametrize("kind", ["A", "B", "hand"])
def test_band_merge(kind, T):
    """Bar per element (re and im alike): 12 u (|x_re| + |x_im|) (sum_c |t_c,re| + |t_c,im|) / max(count, 1), t_c = h * sigmoid(gate) of contributor c.
    sigmoid is expf (2 u), one sum and one division: 5 u; the product with h 1 u, the sum over at most three contributors 2 u, the division by the
    count 1 u: the mask carries 9 u of its absolute sum; the complex product adds two roundings of products and one of their sum.
    Measured on MI355X over all cases: largest error / bar 0.27.
    B = 1 and 2, both output orders, h behind a wider row and a misaligned base, frames of exact zeros (exact zeros out), an uncovered index (zeros)."""
    from mlx_audio_amd import ops

    bands, F = _tables(kind)
    g = torch.Generator().manual_seed(200 * T + len(bands))
    for B, strided in ((1, False), (2, True)):
        tab, tab_h = ops.band_tables(bands, F, DEV), ops.band_tables(bands, F, "cpu")
        spec = torch.randn(B * 2, T, F, 2, generator=g) * (torch.rand(B * 2, T, 1, 1, generator=g) * 3 + 0.01)
        spec[:, 0] = 0.0
        h = torch.randn(B, T, tab_h.h_cols, generator=g) * 3
        ref, mag = E.band_merge64(h, tab_h, spec)
        if strided:
            sd = _strided_spec(spec, 3)
            hb = torch.full((B * T * (tab_h.h_cols + 5) + 4,), float("nan"), device=DEV)
            hd = hb[1:].as_strided((B, T, tab_h.h_cols), (T * (tab_h.h_cols + 5), tab_h.h_cols + 5, 1))
            hd.copy_(h)
            store = torch.full((B * 2, T, F, 2), float("nan"), device=DEV)      # frame-major storage behind the [B * 2, F, T] view
            outs = [ops.band_merge(hd, tab, sd, out=store.permute(0, 2, 1, 3)).clone(), ops.band_merge(hd, tab, sd)]
        else:
            outs = [ops.band_merge(h.to(DEV), tab, spec.to(DEV)) for _ in range(2)]
        torch.cuda.synchronize()
        assert torch.equal(torch.view_as_real(outs[0]), torch.view_as_real(outs[1]))   # two calls (and both output orders): the same bits
        o = outs[0].cpu()
        assert o.shape == (B * 2, F, T) and o.dtype == torch.complex64
        assert not torch.view_as_real(o[:, :, 0]).any()                         # a silent frame: exact zeros
        covered = np.zeros(2 * F, dtype=bool)
        covered[[j for ix in bands for j in ix if 0 <= j < 2 * F]] = True
        for j in np.where(~covered)[0]:
            assert not torch.view_as_real(o[int(j) % 2::2, int(j) // 2]).any()  # an index no band covers: mask 0
        bar = 12 * U * mag + 1e-300
        for part, r in ((o.real, ref.real), (o.imag, ref.imag)):
            err = (part.double() - r).abs()
            _note(f"band_merge[{kind}]", float((err / bar).max()))
            assert torch.all(err <= bar)


def test_band_merge_refuses_without_a_launch():
    from mlx_audio_amd import _lib, ops

    bands, F = _tables("B")
    tab = ops.band_tables(bands, F, DEV)
    T = 4
    spec = torch.randn(2, T, F, 2).to(DEV)
    h = torch.randn(1, T, tab.h_cols).to(DEV)
    out = torch.full((2, F, T, 2), 7.0, device=DEV)
    kw = dict(h=h.data_ptr(), h_bstride=h.stride(0), ldh=h.stride(1), h_cols=tab.h_cols, inv_ptr=tab.inv_ptr_d.data_ptr(), inv_col=tab.inv_col_d.data_ptr(),
              inv_bd=tab.inv_bd_d.data_ptr(), n_inv=tab.n_inv, spec=spec.data_ptr(), spec_cstride=spec.stride(0), spec_tstride=spec.stride(1), B=1, T=T, F=F,
              out=out.data_ptr(), out_cstride=out.stride(0), out_fstride=out.stride(1), out_tstride=out.stride(2))
    for bad, msg in ((dict(out_fstride=2, out_tstride=2), "output strides"), (dict(ldh=tab.h_cols - 1), "bad strides of h"), (dict(T=0), "bad shape"),
                     (dict(inv_ptr=None), "null tensor")):
        with pytest.raises(_lib.Mi355Error, match=msg):
            _lib.call_struct("mi355_band_merge", "mi355_band_merge_args", 0, **dict(kw, **bad))
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    _lib.call_struct("mi355_band_merge", "mi355_band_merge_args", torch.cuda.current_stream().cuda_stream, **kw)   # the unmodified arguments do run
    torch.cuda.synchronize()
    assert not bool((out == 7.0).any())


# ---------------------------------------------------------------------------------------------------------------- head_gate
@pytest.mark.parametrize("heads", [1, 8])
@pytest.mark.parametrize("aligned", [True, False])
def test_head_gate(heads, aligned):
    """Bar per element: 8 u |x sigmoid(g)| (sigmoid 5 u as above, one product, the float32 store).  Measured on MI355X: largest error / bar 0.33.
    Heads 1 and 8 of 64, ``ld`` larger than heads * dh on both operands (the gates are columns of the same buffer as q | k | v), a batch stride, the
    16-byte path and, from a base pointer one float off, the scalar path; the columns beside the heads stay as they were."""
    from mlx_audio_amd import ops

    dh, B, L = 64, 2, 37
    g = torch.Generator().manual_seed(heads)
    ld = 3 * heads * dh + (heads + 3) // 4 * 4 + 4
    off = 0 if aligned else 1
    raw = torch.randn(B * L * ld + 8, generator=g) * 3
    buf = raw.to(DEV)
    qkv = buf[off:off + B * L * ld].view(B, L, ld)
    x, gates = qkv[:, :, heads * dh:2 * heads * dh], qkv[:, :, 3 * heads * dh:3 * heads * dh + heads]
    host = raw[off:off + B * L * ld].view(B, L, ld)
    ref = E.head_gate64(host[:, :, heads * dh:2 * heads * dh], host[:, :, 3 * heads * dh:], heads, dh)
    ops.head_gate(x, gates, heads=heads, dh=dh)
    again = raw.to(DEV)
    ops.head_gate(again[off:off + B * L * ld].view(B, L, ld)[:, :, heads * dh:2 * heads * dh], again[off:off + B * L * ld].view(B, L, ld)[:, :, 3 * heads * dh:3 * heads * dh + heads],
                  heads=heads, dh=dh)
    torch.cuda.synchronize()
    assert torch.equal(buf, again)
    got = buf.cpu()
    view = got[off:off + B * L * ld].view(B, L, ld)
    err = (view[:, :, heads * dh:2 * heads * dh].double() - ref).abs()
    bar = 8 * U * ref.abs() + 1e-300
    _note("head_gate", float((err / bar).max()))
    assert torch.all(err <= bar)
    keep = torch.ones(ld, dtype=torch.bool)
    keep[heads * dh:2 * heads * dh] = False
    assert torch.equal(view[:, :, keep], host[:, :, keep]) and torch.equal(got[:off], raw[:off]) and torch.equal(got[off + B * L * ld:], raw[off + B * L * ld:])


def test_head_gate_refuses_without_a_launch():
    from mlx_audio_amd import _lib, ops

    x = torch.full((1, 5, 128), 7.0, device=DEV)
    gate = torch.zeros((1, 5, 2), device=DEV)
    with pytest.raises(_lib.Mi355Error, match="do not fit"):
        ops.head_gate(x, gate, heads=3, dh=64)
    kw = dict(x=x.data_ptr(), x_bstride=x.stride(0), ldx=128, g=gate.data_ptr(), g_bstride=gate.stride(0), ldg=2, heads=2, dh=64, L=5, B=1)
    for bad, msg in ((dict(ldx=127), "bad strides"), (dict(ldg=1), "bad strides"), (dict(heads=0), "bad shape"), (dict(g=None), "null tensor")):
        with pytest.raises(_lib.Mi355Error, match=msg):
            _lib.call_struct("mi355_head_gate", "mi355_head_gate_args", 0, **dict(kw, **bad))
    torch.cuda.synchronize()
    assert bool((x == 7.0).all())
