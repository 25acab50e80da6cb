"""Dispatch-branch parity of the row kernels of csrc/norm.hip, the Kokoro half of csrc/glue.hip and csrc/attention.hip.

tests/test_kernels_gpu.py calls each of these kernels at one shape; this file walks the branches of their launch code that shape does not reach
(template instantiations, operand alignment, ragged lengths, strided views, chunk and workgroup tails).  Every test states the operation in torch
from the formulas of include/mi355audio.h and of the reference's call sites, evaluates it in float64 (the reference) and in float32 (its own
rounding error, ``e32``) on the CPU, and compares the kernel with the float64 result.

Bars.  Exact (``torch.equal``) where the kernel only moves data or performs the reference's float32 operations in the reference's order: gather,
broadcast, the integer outputs of the duration head, untouched regions, reuse against fresh, VEC against non-VEC, split words against floats.
Float outputs: ``4 * e32 + 1e-6 * peak`` of the float64 result -- the factor covers a different summation tree (wave butterfly against torch's
pairwise sums), the second term a few float32 roundings of the largest value -- except where tests/test_kernels_gpu.py already sets a bar for the
same kernel at the same input scale and a shape of comparable size; that bar is kept there (each test says which shapes those are).
Every comparison prints ``EDGE <kernel> <case> err e32 bar`` before it asserts (``pytest -s`` shows the figures).
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from mlx_audio_amd import ops as _ops

    _ops.require_gpu()
    return _ops


DEV = "cuda"
SENTINEL = -777.25   # exactly representable; no kernel here produces it


def check(name, case, got, ref64, ref32, existing=None):
    """``got`` (float32, cpu) against the float64 statement; bar = ``existing`` (an absolute figure) or 4 * e32 + 1e-6 * peak."""
    ref64 = ref64.double()
    err = float((got.double() - ref64).abs().max())
    e32 = float((ref32.double() - ref64).abs().max())
    peak = float(ref64.abs().max())
    bar = existing if existing is not None else 4.0 * e32 + 1e-6 * peak
    print(f"EDGE {name} {case} err={err:.3e} e32={e32:.3e} peak={peak:.3e} bar={bar:.3e}")
    assert math.isfinite(err) and err <= bar, (name, case, err, e32, bar)
    return err, e32


def misaligned(t):
    """The values of ``t`` as a ``buf[1:1 + n]`` view of a fresh float32 device buffer: 4-byte but not 16-byte aligned."""
    buf = torch.empty(t.numel() + 1, dtype=torch.float32, device=DEV)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 != 0
    return v


def words(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


# ----------------------------------------------------------------------------------------------------------------- LayerNorm
def ln_ref(x, res, w, b, gb, leaky, eps, dtype):
    """nn.LayerNorm / AdaLayerNorm as the header states them: xhat = (t - mean) / sqrt(var + eps) with the biased variance over the channel axis of
    t = x + res; then weight * xhat + bias, then (1 + gamma) * xhat + beta, then LeakyReLU(0.2)."""
    t = x.to(dtype)
    if res is not None:
        t = t + res.to(dtype)
    C = t.shape[-1]
    mean = t.mean(-1, keepdim=True)
    var = ((t - mean) ** 2).mean(-1, keepdim=True)
    o = (t - mean) / torch.sqrt(var + torch.tensor(eps, dtype=dtype))
    if w is not None:
        o = o * w.to(dtype)
        if b is not None:
            o = o + b.to(dtype)
    if gb is not None:
        o = (1 + gb[:, None, :C].to(dtype)) * o + gb[:, None, C:2 * C].to(dtype)
    if leaky:
        o = torch.where(o > 0, o, o * torch.tensor(0.2, dtype=dtype))
    return o


LN_SHAPES = [(1, 1, 4), (2, 5, 1024), (2, 5, 1028), (3, 7, 1280), (1, 3, 2048), (2, 37, 768)]
LN_MODES = ["wb", "w", "none", "ada", "ada_leaky", "wb_res"]
LN_CASES = [(B, L, C, m, 0) for (B, L, C) in LN_SHAPES for m in LN_MODES]
LN_CASES += [(B, L, C, "ada_leaky", s) for (B, L, C) in [(2, 5, 512), (3, 7, 1280)] for s in (2, 4)]


# measured on an MI355X, worst over the cases (absolute): C = 768 / 1024 (bar 2e-5): kernel 1.5e-6, e32 1.6e-6; the other widths: kernel 1.4e-6,
# e32 2.0e-6, at most 0.13 of the bar (the smallest bar, at C = 4, is 1.2e-6).  VEC against non-VEC and split words against floats: bit-equal.
@pytest.mark.parametrize("B,L,C,mode,split", LN_CASES)
def test_layernorm_edges(ops, B, L, C, mode, split):
    """mi355_layernorm, layernorm_kernel<VEC, NCH>:
    - NCH = 8 (C in 1025..2048): (2, 5, 1028) -- the first width past the switch, one live lane in chunk 4 --, (3, 7, 1280) and (1, 3, 2048), which
      fills every lane of the last chunk; NCH = 4 up to the switch: (2, 5, 1024); one live lane in all: (1, 1, 4);
    - VEC = false: weight / bias / ada_gb as ``buf[1:1 + n]`` views (pointer % 16 == 4), and ada_gb as the first 2C columns of a [B, 2C + 1] buffer
      (ada_ld % 4 == 1): both bit-identical to the aligned launch -- the arithmetic is the same, only the loads differ;
    - lens = [L, max(1, L // 2), 1][:B]: rows at or past the length keep the sentinel (Kokoro normalises in place and relies on it);
    - B * L = 1, 10, 21, 3, 74: never a multiple of 4, so the last workgroup has dead waves (``row >= B * L``);
    - x and y are [:, :, :C] slices of buffers 32 columns wider (the columns outside stay as they were), res a slice of a buffer 8 columns wider (its
      own row stride);
    - split = 2 / 4 with ada_gb + leaky at C = 512 (NCH 4) and C = 1280 (NCH 8): the words are oracle/mx_ref.py's split words of the float output of
      the same launch without ``split``.
    Bar: 2e-5 abs (test_layernorm_variants: C = 768 / 512, the same input scale) at C = 768 and C = 1024, the widths of that instantiation at that
    size; 4 * e32 + 1e-6 * peak elsewhere."""
    from oracle import mx_ref

    g = torch.Generator().manual_seed(1000 * C + 10 * LN_MODES.index(mode) + split)
    x = torch.randn(B, L, C, generator=g) * 2 + 1
    r = torch.randn(B, L, C, generator=g)
    w, b = torch.randn(C, generator=g), torch.randn(C, generator=g)
    gb = torch.randn(B, 2 * C, generator=g)
    eps = 1e-5
    kw, ref_kw = {}, dict(res=None, w=None, b=None, gb=None, leaky=False)
    if mode in ("wb", "w", "wb_res"):
        kw["weight"], ref_kw["w"] = w.to(DEV), w
    if mode in ("wb", "wb_res"):
        kw["bias"], ref_kw["b"] = b.to(DEV), b
    if mode in ("ada", "ada_leaky"):
        kw["ada_gb"], ref_kw["gb"] = gb.to(DEV), gb
    if mode == "ada_leaky":
        kw.update(post_act=ops.ACT_LEAKY, post_slope=0.2)
        ref_kw["leaky"] = True
    for k in ("weight", "bias", "ada_gb"):
        assert k not in kw or kw[k].data_ptr() % 16 == 0

    if split:
        xd = x.to(DEV)
        y = ops.layernorm(xd, torch.empty_like(xd), eps=eps, **kw)
        ys = ops.layernorm(xd, torch.empty_like(xd), eps=eps, split=split, **kw)
        torch.cuda.synchronize()
        assert np.array_equal(words(ys), mx_ref.split16_words(y.cpu().numpy(), split))
        ref = ln_ref(x, **ref_kw, eps=eps, dtype=torch.float64)
        check("layernorm", (B, L, C, mode, "float launch of the split case"), y.cpu(), ref, ln_ref(x, **ref_kw, eps=eps, dtype=torch.float32))
        return

    lens = torch.tensor([L, max(1, L // 2), 1][:B], dtype=torch.int32)
    lens_d = lens.to(DEV)
    xbuf0 = torch.randn(B, L, C + 32, generator=g)
    xbuf0[:, :, :C] = x
    xbuf = xbuf0.to(DEV)
    if mode == "wb_res":
        rbuf = torch.zeros(B, L, C + 8, device=DEV)
        rbuf[:, :, :C] = r.to(DEV)
        kw["res"], ref_kw["res"] = rbuf[:, :, :C], r

    def run(**over):
        ybuf = torch.full((B, L, C + 32), SENTINEL, device=DEV)
        ops.layernorm(xbuf[:, :, :C], ybuf[:, :, :C], eps=eps, lens=lens_d, **{**kw, **over})
        torch.cuda.synchronize()
        return ybuf.cpu()

    y1 = run()
    assert torch.equal(xbuf.cpu(), xbuf0)
    assert torch.equal(y1[:, :, C:], torch.full((B, L, 32), SENTINEL))
    ref64 = ln_ref(x, **ref_kw, eps=eps, dtype=torch.float64)
    ref32 = ln_ref(x, **ref_kw, eps=eps, dtype=torch.float32)
    existing = 2e-5 if C in (768, 1024) else None
    for i in range(B):
        n = int(lens[i])
        check("layernorm", (B, L, C, mode, i), y1[i, :n, :C], ref64[i, :n], ref32[i, :n], existing)
        assert torch.equal(y1[i, n:], torch.full((L - n, C + 32), SENTINEL))
    # VEC = false on the same values
    mis = {k: misaligned(kw[k]) for k in ("weight", "bias", "ada_gb") if k in kw}
    if mis:
        assert torch.equal(run(**mis), y1)
    if "ada_gb" in kw:
        wide = torch.zeros(B, 2 * C + 1, device=DEV)
        wide[:, :2 * C] = kw["ada_gb"]
        odd = wide[:, :2 * C]
        assert odd.stride(0) % 4 == 1 and odd.data_ptr() % 16 == 0
        assert torch.equal(run(ada_gb=odd), y1)


# ----------------------------------------------------------------------------------------------------------------- AdaIN coefficients
def adain_ref(v, gb, C, eps, dtype):
    """InstanceNorm1d + AdaIN1d as the header states them: per channel mean / biased variance over the rows of v [n, C], then
    scale = (1 + gamma) / sqrt(var + eps), shift = beta - mean * scale."""
    v = v.to(dtype)
    mean = v.mean(0)
    var = ((v - mean) ** 2).mean(0)
    gamma = gb[:C].to(dtype) if gb is not None else torch.zeros(C, dtype=dtype)
    beta = gb[C:2 * C].to(dtype) if gb is not None else torch.zeros(C, dtype=dtype)
    scale = (1 + gamma) / torch.sqrt(var + torch.tensor(eps, dtype=dtype))
    return scale, beta - mean * scale


# measured on an MI355X, worst over the cases, relative to the peak of the float64 result: (3, 1000, 514) (bar 2e-5): scale 1.6e-7, shift 1.7e-7
# (e32 1.6e-7 / 2.3e-7); the other shapes: scale 1.7e-7, shift 2.4e-7 (e32 1.8e-7 / 2.7e-7), at most 0.15 of the bar.  In absolute terms the largest
# figures belong to L = 1, where scale ~ 1e3 and shift ~ 5e4: scale 1.3e-4 (e32 7.3e-5), shift 1.0e-2 (e32 5.0e-3).
@pytest.mark.parametrize("B,L,C,lens", [
    (1, 1, 32, None),
    (2, 63, 36, [63, 17]),
    (3, 1000, 514, [1000, 40, 1]),
    (40, 130, 900, [130 - (7 * b) % 129 for b in range(40)]),
])
def test_adain_coef_edges(ops, B, L, C, lens):
    """mi355_adain_coef (instnorm_partial_kernel + adain_finalize_kernel):
    - (1, 1, 32): L = 1, variance exactly 0, rstd = 1 / sqrt(eps); no lens (the ``a.L`` path); nsplit clamps to 1;
    - (2, 63, 36): L < 64 -> max_split = 1, so nsplit (256 before the clamp) becomes 1; C = 36 leaves 28 dead channels in the second column block;
    - (3, 1000, 514) with lens = [1000, 40, 1]: nsplit = 16 splits of 63 rows; lens[1] = 40 and lens[2] = 1 lie inside the first split, so splits
      1..15 of those utterances have r0 >= len and must add nothing;
    - (40, 130, 900): B * cblocks = 40 * 29 = 1160 >= 1024 -> nsplit = 1 although L > 64;
    each with gb and with gb = None, and with ``reuse_sums``: a second gb on the kept sums equals a fresh call with that gb bit for bit.  The padding
    columns C..round_up(C, 32) of scale and shift are exactly 0.  Input: mean 50, std 3 (the cancellation-prone scale of test_adain_coef).
    Bar: 2e-5 of the peak (test_adain_coef) at (3, 1000, 514), that test's shape; 4 * e32 + 1e-6 * peak at the others."""
    g = torch.Generator().manual_seed(100 * B + C)
    ld = ops.round_up(C, 32)
    x = torch.randn(B, L, ld, generator=g) * 3 + 50.0
    gb1 = torch.randn(B, 2 * C + 8, generator=g)
    gb2 = torch.randn(B, 2 * C + 8, generator=g)
    xd = x.to(DEV)[:, :, :C]
    lens_d = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
    eps = 1e-5
    sums = torch.empty(B * C * 2, dtype=torch.float64, device=DEV)
    sc1, sh1 = ops.adain_coef(xd, gb1.to(DEV), lens=lens_d, eps=eps, sums=sums)
    sc2, sh2 = ops.adain_coef(xd, gb2.to(DEV), lens=lens_d, eps=eps, sums=sums, reuse=True)
    sc2f, sh2f = ops.adain_coef(xd, gb2.to(DEV), lens=lens_d, eps=eps)
    sc0, sh0 = ops.adain_coef(xd, None, lens=lens_d, eps=eps)
    torch.cuda.synchronize()
    assert torch.equal(sc2, sc2f) and torch.equal(sh2, sh2f)
    for t in (sc1, sh1, sc2, sh2, sc0, sh0):
        assert tuple(t.shape) == (B, ld)
        assert int(torch.count_nonzero(t[:, C:])) == 0
    same_shape = (B, L, C) == (3, 1000, 514)
    for tag, gb, sc, sh in (("gb", gb1, sc1, sh1), ("gb2-reused", gb2, sc2, sh2), ("none", None, sc0, sh0)):
        for b in range(B):
            n = L if lens is None else lens[b]
            gbb = None if gb is None else gb[b]
            s64, h64 = adain_ref(x[b, :n, :C], gbb, C, eps, torch.float64)
            s32, h32 = adain_ref(x[b, :n, :C], gbb, C, eps, torch.float32)
            check("adain_coef.scale", (B, L, C, tag, b), sc[b, :C].cpu(), s64, s32, 2e-5 * float(s64.abs().max()) if same_shape else None)
            check("adain_coef.shift", (B, L, C, tag, b), sh[b, :C].cpu(), h64, h32, 2e-5 * float(h64.abs().max()) if same_shape else None)
    if L == 1:   # variance exactly 0: scale is (1 + gamma) / sqrt(eps) to float32 rounding
        want = (1 + gb1[:, :C].double()) / math.sqrt(eps)
        assert float(((sc1[:, :C].cpu().double() - want) / want).abs().max()) < 1e-6


# ----------------------------------------------------------------------------------------------------------------- AdaIN from partials
LONG = 64 * 512


# measured on an MI355X, worst over the cases, relative to the peak: len >= 64 (bar 2e-6): scale 1.3e-7, shift 1.8e-7 (e32 1.3e-7 / 2.6e-7); len = 1:
# scale 1.1e-7, shift 1.4e-7 (e32 8.9e-8 / 1.1e-7), at most 0.10 of the bar; absolute there (scale ~ 5e2, shift ~ 4e3): 5.9e-5 and 5.8e-4 (e32 5.0e-5, 4.4e-4).
@pytest.mark.parametrize("B,C,lens", [
    (2, 6, [65, 1]), (2, 70, [65, 1]), (2, 128, [65, 1]),
    (2, 6, None), (2, 70, None), (2, 128, None),          # no lens: every utterance is L = 64 rows, exactly one full block
    (8, 6, [65, 64, 1, 65, 64, 1, 65, 64]), (8, 70, [65, 64, 1, 65, 64, 1, 65, 64]), (8, 128, [65, 64, 1, 65, 64, 1, 65, 64]),
    (8, 6, [LONG + 1, LONG, 65, 64, 1, LONG, LONG + 1, 1]),
])
def test_adain_from_partials_edges(ops, B, C, lens):
    """mi355_adain_from_partials, adain_from_partials_kernel<CPW>: B = 2 takes CPW = 4, B = 8 takes CPW = 16 (the register-keeping sweep).
    - C = 6 and C = 70 are multiples of neither CPW: dead channel lanes (``c >= C``) in a workgroup that also has live ones; C = 128 divides both;
    - len = 1 (one block of one row: M2 = 0, variance 0), len = 64 (exactly one full block), len = 65 (a second block with cnt = 1, the
      ``sv.x / cnt`` branch of the block mean), and lens = None (the ``a.L`` path, L = 64);
    - the CPW = 16 ``keep`` boundary: len = 64 * 512 -> nblk = 512 = kAdainKeep * 16 blocks, kept in registers; len = 64 * 512 + 1 -> 513 blocks, the
      re-reading fallback, with a last block of one row.  ``keep`` is per utterance, so one launch holds both (C = 6 keeps the host loop small);
    each with gb and with gb = None; blocks past an utterance's length hold NaN and must not be read into a result.
    Bar: 2e-6 of the peak (test_adain_from_partials_batch_kernel, the same input scale) for utterances of at least one full block, that test's range of
    lengths; 4 * e32 + 1e-6 * peak for len = 1."""
    g = torch.Generator().manual_seed(B * 1000 + C + (0 if lens is None else max(lens)))
    L = 64 if lens is None else max(lens)
    ll = [L] * B if lens is None else lens
    y = torch.randn(B, L, C, generator=g) * 2.0 + 5.0
    gb = torch.randn(B, 2 * C, generator=g) * 0.3
    nblk = (L + 63) // 64
    st = torch.full((B, nblk, C, 2), float("nan"))
    for b in range(B):
        n = ll[b]
        for e in range((n + 63) // 64):
            blk = y[b, e * 64:min(n, (e + 1) * 64)].double()
            st[b, e, :, 0] = blk.sum(0).float()
            st[b, e, :, 1] = ((blk - blk.mean(0)) ** 2).sum(0).float()
    lens_d = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
    std = st.to(DEV)
    sc1, sh1 = ops.adain_from_partials(std, L, gb.to(DEV), lens_d)
    sc0, sh0 = ops.adain_from_partials(std, L, None, lens_d)
    torch.cuda.synchronize()
    cp = ops.round_up(C, 32)
    for tag, gbt, sc, sh in (("gb", gb, sc1, sh1), ("none", None, sc0, sh0)):
        assert tuple(sc.shape) == (B, cp) and int(torch.count_nonzero(sc[:, C:])) == 0 and int(torch.count_nonzero(sh[:, C:])) == 0
        for b in range(B):
            n = ll[b]
            gbb = None if gbt is None else gbt[b]
            s64, h64 = adain_ref(y[b, :n], gbb, C, 1e-5, torch.float64)
            s32, h32 = adain_ref(y[b, :n], gbb, C, 1e-5, torch.float32)
            full = n >= 64
            check("adain_partials.scale", (B, C, n, tag), sc[b, :C].cpu(), s64, s32, 2e-6 * float(s64.abs().max()) if full else None)
            check("adain_partials.shift", (B, C, n, tag), sh[b, :C].cpu(), h64, h32, 2e-6 * float(h64.abs().max()) if full else None)


# ----------------------------------------------------------------------------------------------------------------- attention
def attn_ref(qkv, n, heads, dh, dtype):
    """AlbertSelfAttention on the first n rows: softmax(q k^T / sqrt(dh)) v per head (keys past n carry the reference's -10000 mask: weight 0)."""
    D = heads * dh
    q, k, v = [t.reshape(n, heads, dh).transpose(0, 1).to(dtype) for t in qkv[:n].split(D, dim=-1)]
    s = q @ k.transpose(-1, -2) / math.sqrt(dh)
    return (torch.softmax(s, -1) @ v).transpose(0, 1).reshape(n, D)


# measured on an MI355X: the unit-variance cases (bar 2e-5): kernel 6.9e-7, e32 6.8e-7; q, k x 30: kernel 2.28e-4, e32 2.28e-4 (bar 9.2e-4) -- the
# softmax is nearly one-hot there and both float32 evaluations round the same scores of ~2e3.
@pytest.mark.parametrize("B,T,heads,dh,lens,qk_scale", [
    (1, 1, 2, 64, None, 1.0),
    (2, 64, 3, 32, None, 1.0),
    (2, 65, 2, 4, None, 1.0),
    (3, 83, 12, 64, [83, 1, 40], 1.0),
    (2, 512, 2, 64, [512, 449], 1.0),
    (1, 130, 4, 32, None, 30.0),
])
def test_attention_edges(ops, B, T, heads, dh, lens, qk_scale):
    """mi355_attention (one wave per query, lanes own keys, then head channels):
    - T = 1 (one key: the output is v), T = 64 (score chunk 0 full, chunk 1 empty), T = 65 (one key in chunk 1; 65 and 83 are no multiples of 4, so
      the last workgroup has waves with ``q >= len``), T = 512 (all eight score chunks; 449 = 7 * 64 + 1 keys in the second utterance);
    - dh = 32 and dh = 4 (``lane < dh`` in the q load and in the PV phase);
    - lens = [83, 1, 40]: an utterance of one key inside a longer batch;
    - q and k scaled by 30 (scores of several hundred: without the max subtraction expf overflows);
    - qkv is a [:, :, :3D] slice of a buffer 8 columns wider, out a [:, :, :D] slice of a sentinel-filled buffer 12 columns wider: rows >= len and the
      columns outside the slice keep the sentinel.
    Bar: 2e-5 abs (test_attention, unit-variance qkv) for the unit-variance cases; 4 * e32 + 1e-6 * peak for the scaled one."""
    g = torch.Generator().manual_seed(T * 100 + dh)
    D = heads * dh
    qkv = torch.randn(B, T, 3 * D, generator=g)
    qkv[:, :, :2 * D] *= qk_scale
    buf = torch.randn(B, T, 3 * D + 8, generator=g)
    buf[:, :, :3 * D] = qkv
    bufd = buf.to(DEV)
    obuf = torch.full((B, T, D + 12), SENTINEL, device=DEV)
    lens_d = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
    ops.attention(bufd[:, :, :3 * D], heads, dh, obuf[:, :, :D], lens=lens_d)
    torch.cuda.synchronize()
    out = obuf.cpu()
    assert torch.equal(out[:, :, D:], torch.full((B, T, 12), SENTINEL))
    for b in range(B):
        n = T if lens is None else lens[b]
        assert torch.equal(out[b, n:], torch.full((T - n, D + 12), SENTINEL))
        check("attention", (B, T, heads, dh, b), out[b, :n, :D], attn_ref(qkv[b], n, heads, dh, torch.float64),
              attn_ref(qkv[b], n, heads, dh, torch.float32), 2e-5 if qk_scale == 1.0 else None)
    if T == 1:
        assert float((out[0, 0, :D] - qkv[0, 0, 2 * D:]).abs().max()) == 0.0   # softmax over one key is exactly 1


# ----------------------------------------------------------------------------------------------------------------- duration / alignment
def dur_ref(logits, bins, speed, max_frames, dtype):
    """kokoro.py:140-147: sum of sigmoids / speed, nan -> 1, +inf -> 100, -inf -> 1, round half to even, at least 1, at most the cap
    (max_frames 0: 100; N: N; < 0: none).  Returns (pre-round value, int32 durations)."""
    lg = logits[..., :bins].to(dtype)
    r = (1.0 / (1.0 + torch.exp(-lg))).sum(-1) / torch.tensor(speed, dtype=dtype)
    v = torch.nan_to_num(r, nan=1.0, posinf=100.0, neginf=1.0)
    v = torch.clamp(torch.round(v), min=1.0)   # torch.round is half-to-even like mx.round
    if max_frames >= 0:
        v = torch.clamp(v, max=float(max_frames) if max_frames else 100.0)
    return r, v.to(torch.int32)


def dur_logits(seed, B, T, ld, bins, speed, lens):
    """Random logits whose float64 pre-round durations all lie more than 1e-3 from a rounding tie on the valid rows: drawn from ``seed``, redrawn
    from the next seeds otherwise (the seeds used below pass at the first draw; test_duration_random asserts it)."""
    for s in range(seed, seed + 64):
        logits = torch.randn(B, T, ld, generator=torch.Generator().manual_seed(s)) * 2
        r, _ = dur_ref(logits, bins, speed, 0, torch.float64)
        frac = (r - torch.floor(r) - 0.5).abs()
        valid = torch.arange(T)[None, :] < torch.tensor(lens if lens is not None else [T] * B)[:, None]
        if float(frac[valid].min()) > 1e-3:
            return logits, s
    raise AssertionError("no seed with a clear rounding margin")


def check_alignment(dur, frames, idx, lens, T, idx_cap):
    d = dur.cpu()
    for b in range(d.shape[0]):
        n = T if lens is None else lens[b]
        assert int(d[b, n:].abs().sum()) == 0                      # durations past the length are 0
        want = torch.repeat_interleave(torch.arange(T), d[b].long())
        assert int(frames[b]) == want.numel()                      # the total, also when it exceeds the index row
        m = min(want.numel(), idx_cap)
        assert torch.equal(idx[b, :m].cpu().long(), want[:m])
        assert int(idx[b, m:].abs().sum()) == 0                    # entries past the total stay as the wrapper zeroed them


@pytest.mark.parametrize("max_frames,want", [(0, 100), (7, 7), (-1, 200)])
def test_duration_saturation(ops, max_frames, want):
    """mi355_duration_align, the three ``max_frames`` modes and the replacements.  All logits +40, bins = 50, speed = 0.25: every sigmoid is exactly 1
    in float32, the pre-round value exactly 200 -> 100 (max_frames = 0: the cap of 100), 7 (max_frames = 7), 200 (max_frames < 0: no cap).  All logits
    -40: pre-round value ~ 1e-15 -> the floor of 1.  A row of NaN logits: pre-round NaN, duration 1.  speed = 1.2e-38 (a normal float32): 50 / speed
    overflows to +inf, replaced by 100 before the cap (so 100 without a cap, 7 under max_frames = 7).  The -inf replacement cannot be reached: a sum
    of sigmoids is >= 0 and speed > 0."""
    B, T, cap = 2, 3, 1024
    hi = torch.full((B, T, 64), 40.0)
    hi[1, 1] = float("nan")
    dur, raw, frames, idx = ops.duration_align(hi.to(DEV)[:, :, :50], T, B, 0.25, cap, DEV, max_frames=max_frames)
    torch.cuda.synchronize()
    exp = torch.full((B, T), want, dtype=torch.int32)
    exp[1, 1] = 1
    assert torch.equal(dur.cpu(), exp)
    r = raw.cpu()
    assert math.isnan(float(r[1, 1])) and float(r[0].min()) == 200.0 and float(r[0].max()) == 200.0
    _, refd = dur_ref(hi, 50, 0.25, max_frames, torch.float32)
    assert torch.equal(refd, exp)
    check_alignment(dur, frames, idx, None, T, cap)
    lo = torch.full((B, T, 64), -40.0)
    dur, raw, frames, idx = ops.duration_align(lo.to(DEV)[:, :, :50], T, B, 0.25, cap, DEV, max_frames=max_frames)
    torch.cuda.synchronize()
    assert torch.equal(dur.cpu(), torch.ones((B, T), dtype=torch.int32)) and 0.0 <= float(raw.min()) and float(raw.max()) < 1e-12
    assert [int(f) for f in frames] == [T, T]
    dur, raw, frames, idx = ops.duration_align(hi.to(DEV)[:, :, :50], T, B, 1.2e-38, cap, DEV, max_frames=max_frames)
    torch.cuda.synchronize()
    assert float(raw[0, 0]) == float("inf")
    exp = torch.full((B, T), 7 if max_frames == 7 else 100, dtype=torch.int32)
    exp[1, 1] = 1
    assert torch.equal(dur.cpu(), exp)
    check_alignment(dur, frames, idx, None, T, cap)


@pytest.mark.parametrize("bins,raw_want,want", [(5, 2.5, 2), (7, 3.5, 4), (1, 0.5, 1)])
def test_duration_ties(ops, bins, raw_want, want):
    """Round half to even, and ``bins != 50``: logits all 0 give sigmoid = 0.5 exactly (expf(-0) = 1), speed = 1: 2.5 -> 2, 3.5 -> 4, and 0.5 -> 0 -> the
    floor of 1.  (round-half-away would give 3, 4, 1.)"""
    B, T = 2, 4
    z = torch.zeros(B, T, 8, device=DEV)
    dur, raw, frames, idx = ops.duration_align(z[:, :, :bins], T, B, 1.0, 64, DEV, bins=bins)
    torch.cuda.synchronize()
    assert torch.equal(raw.cpu(), torch.full((B, T), raw_want))
    assert torch.equal(dur.cpu(), torch.full((B, T), want, dtype=torch.int32))
    check_alignment(dur, frames, idx, None, T, 64)


# measured on an MI355X: pre-round value: kernel 1.2e-5, e32 6.1e-6 at a peak of 33 (0.20 of the bar); every integer output equal.
@pytest.mark.parametrize("B,T,ld,bins,lens,seed", [
    (2, 20, 64, 50, [20, 11], 3),
    (1, 1, 40, 37, None, 0),
    (2, 512, 52, 50, [512, 300], 5),
])
def test_duration_random(ops, B, T, ld, bins, lens, seed):
    """Random logits away from every rounding tie (a condition on the float64 reference, asserted here: the first draw of each seed passes, so the
    integer comparison always runs): T = 1 (bins = 37, one thread with work), T = 512 with lens = [512, 300] (every thread of the block, the whole
    ``sstart`` scan) and the shape of test_glue_kernels.  Durations, totals and the frame -> token index are exact; the pre-round value has
    4 * e32 + 1e-6 * peak."""
    speed = 0.9
    logits, used = dur_logits(seed, B, T, ld, bins, speed, lens)
    assert used == seed
    cap = 32 * T
    lens_d = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
    dur, raw, frames, idx = ops.duration_align(logits.to(DEV)[:, :, :bins], T, B, speed, cap, DEV, lens=lens_d, bins=bins)
    torch.cuda.synchronize()
    r64, refd = dur_ref(logits, bins, speed, 0, torch.float64)
    r32, _ = dur_ref(logits, bins, speed, 0, torch.float32)
    for b in range(B):
        n = T if lens is None else lens[b]
        check("duration.raw", (B, T, bins, b), raw[b, :n].cpu(), r64[b, :n], r32[b, :n])
        assert torch.equal(dur[b, :n].cpu(), refd[b, :n])
    check_alignment(dur, frames, idx, lens, T, cap)


def test_duration_index_overflow(ops):
    """Total frames (8 tokens x 5 forced frames = 40) greater than ``idx_cap`` = 16: writes stop at the row end -- idx[b, :16] is the repeat-interleave
    prefix for BOTH utterances, so utterance 0 did not run into utterance 1's row -- while frames[b] still reports the total; with lens = [8, 5] the
    durations past the length are 0 and the total counts the valid tokens only."""
    B, T, cap = 2, 8, 16
    forced = torch.full((B, T), 5, dtype=torch.int32, device=DEV)
    prefix = torch.repeat_interleave(torch.arange(T), 5)[:cap]
    dur, _, frames, idx = ops.duration_align(None, T, B, 1.0, cap, DEV, forced=forced)
    torch.cuda.synchronize()
    assert [int(f) for f in frames] == [40, 40]
    assert torch.equal(dur.cpu(), forced.cpu())
    for b in range(B):
        assert torch.equal(idx[b].cpu().long(), prefix)
    lens = torch.tensor([8, 5], dtype=torch.int32, device=DEV)
    dur, _, frames, idx = ops.duration_align(None, T, B, 1.0, cap, DEV, forced=forced, lens=lens)
    torch.cuda.synchronize()
    assert [int(f) for f in frames] == [40, 25]
    assert int(dur[1, 5:].abs().sum()) == 0 and int(dur[1, :5].min()) == 5
    for b in range(B):
        assert torch.equal(idx[b].cpu().long(), prefix)


# ----------------------------------------------------------------------------------------------------------------- pool-up2
# measured on an MI355X: kernel 1.25e-6, e32 1.25e-6 (peak 11).
def test_adain_pool_up2_ragged(ops):
    """mi355_adain_pool_up2 with lens: B = 3, L = 9, C = 300 (the thread-stride loop: C > 256), lens = [9, 1, 4].  Per utterance the oracle's depthwise
    transposed conv on the first ``len`` rows only: the even outputs' ``t < len`` tap at the ragged tail (output 2 len - 1 takes x[len - 1] alone, not
    the row behind it, which holds other data), len = 1 (two outputs), and rows >= 2 len of a sentinel-filled y untouched.
    Bar: 1e-5 abs (test_adain_pool_up2, the same input scale)."""
    from oracle import kokoro_ref

    g = torch.Generator().manual_seed(17)
    B, L, C = 3, 9, 300
    lens = [9, 1, 4]
    x = torch.randn(B, L, C, generator=g)
    sc, sh = torch.rand(B, C, generator=g) + 0.5, torch.randn(B, C, generator=g)
    w = torch.randn(C, 3, generator=g)
    bias = torch.randn(C, generator=g)
    y = torch.full((B, 2 * L, C), SENTINEL, device=DEV)
    ops.adain_pool_up2(x.to(DEV), sc.to(DEV), sh.to(DEV), 0.2, w.to(DEV), bias.to(DEV), y, lens=torch.tensor(lens, dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    got = y.cpu()

    def ref(b, n, dtype):
        a = F.leaky_relu(x[b:b + 1, :n].to(dtype) * sc[b].to(dtype) + sh[b].to(dtype), 0.2).transpose(1, 2)
        r = kokoro_ref.conv_transpose1d_mlx(a, w[:, :, None].to(dtype), bias.to(dtype), stride=2, padding=0, groups=C)[:, :, 1:]
        assert r.shape[2] == 2 * n
        return r[0].transpose(0, 1)

    for b in range(B):
        n = lens[b]
        check("pool_up2", (b, n), got[b, :2 * n], ref(b, n, torch.float64), ref(b, n, torch.float32), 1e-5)
        assert torch.equal(got[b, 2 * n:], torch.full((2 * L - 2 * n, C), SENTINEL))


# ----------------------------------------------------------------------------------------------------------------- conv1d_c1_k3s2
# measured on an MI355X: kernel 2.6e-7, e32 2.3e-7 (peak 2.4).
@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("Lin", [1, 2, 40, 41])
def test_conv1d_c1_k3s2_edges(ops, Lin, ragged):
    """mi355_conv1d_c1_k3s2 (k3, stride 2, pad 1; output l reads x[2 l - 1 .. 2 l + 1]): Lin = 1 (one output, the centre tap alone), 2 (one output,
    two taps), 40 (even: the last output reads x[37 .. 39], all three taps live) and 41 (odd: the third tap of the last output is the right pad),
    without lens_in and with lens_in = [Lin, max(1, Lin - 3), 0] (the ``i < len`` taps inside a longer row whose tail holds other data; the
    utterance of length 0 has no output row and writes nothing).  Per utterance F.conv1d on its first ``len`` samples; rows past the utterance's
    output length and the other columns of y keep the sentinel.
    Bar: 1e-6 abs (test_glue_kernels, the same input scale and weights)."""
    g = torch.Generator().manual_seed(Lin)
    B, col, ncol = 3, 5, 8
    w3, bias = [0.3, -1.2, 0.7], 0.05
    x = torch.randn(B, Lin, generator=g)
    lens = [Lin, max(1, Lin - 3), 0] if ragged else None
    Lout = (Lin - 1) // 2 + 1
    y = torch.full((B, Lout, ncol), SENTINEL, device=DEV)
    ops.conv1d_c1_k3s2(x.to(DEV), w3, bias, y, col, lens_in=None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    got = y.cpu()
    keep = [c for c in range(ncol) if c != col]
    assert torch.equal(got[:, :, keep], torch.full((B, Lout, ncol - 1), SENTINEL))
    for b in range(B):
        n = Lin if lens is None else lens[b]
        if n == 0:
            assert torch.equal(got[b, :, col], torch.full((Lout,), SENTINEL))
            continue

        def ref(dtype):
            return F.conv1d(x[b, :n].to(dtype)[None, None], torch.tensor([[w3]], dtype=dtype), torch.tensor([bias], dtype=dtype), stride=2, padding=1)[0, 0]

        r64 = ref(torch.float64)
        lo = r64.numel()
        assert lo == (n - 1) // 2 + 1
        check("conv1d_c1_k3s2", (Lin, ragged, b), got[b, :lo, col], r64, ref(torch.float32), 1e-6)
        assert torch.equal(got[b, lo:, col], torch.full((Lout - lo,), SENTINEL))


# ----------------------------------------------------------------------------------------------------------------- gather / broadcast
@pytest.mark.parametrize("per_batch", [False, True])
def test_gather_rows_wide_and_per_batch(ops, per_batch):
    """mi355_gather_rows with C = 700 (three trips of the 256-thread stride loop, the last with 188 live threads), y a [:, :, :C] slice of a buffer
    20 columns wider, a table whose rows are 4 floats longer than C, position table + added row, lens = [13, 6, 1]; ``per_batch=True`` takes a
    [B, rows, ld] table (``table_bstride != 0``: the alignment gather of kokoro.py:161-169).  Exact: the kernel adds in the reference's order
    (words + position + token type); rows >= len are zeroed inside the slice, and the columns outside it are untouched."""
    g = torch.Generator().manual_seed(23 + per_batch)
    B, T, C, rows = 3, 13, 700, 31
    lens = [13, 6, 1]
    table = torch.randn((B, rows, C + 4) if per_batch else (rows, C + 4), generator=g)
    pos = torch.randn(T, C, generator=g)
    row = torch.randn(C, generator=g)
    idx = torch.randint(0, rows, (B, T), generator=g, dtype=torch.int32)
    ybuf = torch.full((B, T, C + 20), SENTINEL, device=DEV)
    td = table.to(DEV)
    ops.gather_rows(td[..., :C], idx.to(DEV), ybuf[:, :, :C], per_batch=per_batch, pos_table=pos.to(DEV), add_row=row.to(DEV),
                    lens=torch.tensor(lens, dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    got = ybuf.cpu()
    src = torch.stack([table[b, idx[b].long(), :C] for b in range(B)]) if per_batch else table[idx.long(), :C]
    ref = src + pos[None] + row
    for b in range(B):
        ref[b, lens[b]:] = 0
    assert torch.equal(got[:, :, :C], ref)
    assert torch.equal(got[:, :, C:], torch.full((B, T, 20), SENTINEL))
    # the plain gather (no position table, no added row, no lens) moves bits
    ops.gather_rows(td[..., :C], idx.to(DEV), ybuf[:, :, :C], per_batch=per_batch)
    torch.cuda.synchronize()
    assert torch.equal(ybuf[:, :, :C].cpu(), src)


def test_broadcast_rows_wide(ops):
    """mi355_broadcast_rows with C = 700 (the thread-stride loop), v a slice of a wider buffer (its own row stride), y a slice at a column offset,
    lens = [13, 6, 1]: rows < len receive v[b] bit for bit, rows >= len zeros, the columns outside the slice are untouched."""
    g = torch.Generator().manual_seed(29)
    B, T, C = 3, 13, 700
    lens = [13, 6, 1]
    v = torch.randn(B, C + 4, generator=g)
    ybuf = torch.full((B, T, C + 20), SENTINEL, device=DEV)
    ops.broadcast_rows(v.to(DEV)[:, :C], ybuf[:, :, 8:8 + C], lens=torch.tensor(lens, dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    got = ybuf.cpu()
    ref = v[:, None, :C].expand(B, T, C).clone()
    for b in range(B):
        ref[b, lens[b]:] = 0
    assert torch.equal(got[:, :, 8:8 + C], ref)
    assert torch.equal(got[:, :, :8], torch.full((B, T, 8), SENTINEL)) and torch.equal(got[:, :, 8 + C:], torch.full((B, T, 12), SENTINEL))
