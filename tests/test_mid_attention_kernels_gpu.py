"""``csrc/mid_attn.hip`` against float64 on the host.  The attention reference restates the module's own order (moonshine.py, MoonshineAttention: scale,
ADDITIVE mask, softmax over all Tk keys, @ v), not the kernel's formulation (hidden keys, log2 domain, online softmax).  The rotary reference is
apply_rotary_pos_emb in float64 on the float32 tables, under a per-element float32 rounding bound."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"

BAR = 2e-6   # the project's bar for this arithmetic (tests/test_narrow_attention_kernels_gpu.py, the f32 flash kernel): one dh-long contraction, fp32, online softmax
NEG = -1e9   # the additive mask: exp(-1e9 - max) is exactly 0 in float64


def module_ref(q, k, v, H, KH, dh, lens_q=None, lens_k=None, causal=False):
    """[B, Tq, H dh] float64.  Every query sees all Tk keys, the invisible ones behind an additive -1e9; ``vis[b, i, j]`` comes back with it."""
    B, Tq, _ = q.shape
    Tk = k.shape[1]
    q4 = q.double().reshape(B, Tq, H, dh).permute(0, 2, 1, 3)
    k4, v4 = (t.double().reshape(B, Tk, KH, dh).permute(0, 2, 1, 3).repeat_interleave(H // KH, dim=1) for t in (k, v))
    nq = torch.tensor([Tq] * B if lens_q is None else lens_q)
    nk = torch.tensor([Tk] * B if lens_k is None else lens_k)
    j = torch.arange(Tk)[None, None, :]
    i = torch.arange(Tq)[None, :, None]
    vis = (j < nk[:, None, None]).expand(B, Tq, Tk)
    if causal:
        vis = vis & (j <= i + (nk - nq)[:, None, None])
    scores = (q4 * dh ** -0.5) @ k4.transpose(2, 3) + (~vis)[:, None].double() * NEG
    return (torch.softmax(scores, dim=-1) @ v4).permute(0, 2, 1, 3).reshape(B, Tq, H * dh), vis


def run_case(tag, q, k, v, H, KH, dh, lens_q=None, lens_k=None, causal=False):
    """One call checked four ways: two calls bit-equal, NaN-initialised output fully written, rows beyond ``lens_q`` (and rows that see no key) exact
    zeros, the rest within the bar of the float64 module.  Returns max|err| / max|want|."""
    from mlx_audio_amd import ops

    B, Tq = q.shape[:2]
    lq = None if lens_q is None else torch.tensor(lens_q, dtype=torch.int32, device=DEV)
    lk = None if lens_k is None else torch.tensor(lens_k, dtype=torch.int32, device=DEV)
    outs = []
    for _ in range(2):
        out = torch.full((B, Tq, H * dh), float("nan"), device=DEV)
        ops.mid_attention(q, k, v, out, heads=H, kv_heads=KH, dh=dh, causal=causal, lens_q=lq, lens_k=lk)
        outs.append(out)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1]), f"{tag}: two calls on the same bytes differ"
    got = outs[0].double().cpu()
    want, vis = module_ref(q.cpu(), k.cpu(), v.cpu(), H, KH, dh, lens_q, lens_k, causal)
    live = vis.any(dim=2)   # [B, Tq]: the query sees a key ...
    for b in range(B):
        live[b, (Tq if lens_q is None else lens_q[b]):] = False   # ... and is a valid row
    assert not got[~live].any(), f"{tag}: rows beyond lens_q (or without a visible key) are not exactly zero"
    assert bool(live.any())
    err, peak = float((got[live] - want[live]).abs().max()), float(want[live].abs().max())
    print(f"mid_attention {tag}: max|err| / max|want| = {err / peak:.2e}")
    assert err / peak < BAR, (tag, err / peak)
    return err / peak


def operands(g, B, Tq, Tk, H, KH, dh, fused):
    """q / k / v as slices of one fused buffer (self-attention shapes) or of separate, wider-than-needed buffers."""
    hd, kd = H * dh, KH * dh
    if fused and Tq == Tk:
        buf = torch.randn(B, Tq, hd + 2 * kd, generator=g).to(DEV)
        return buf[:, :, :hd], buf[:, :, hd:hd + kd], buf[:, :, hd + kd:]
    return torch.randn(B, Tq, hd, generator=g).to(DEV), torch.randn(B, Tk, kd, generator=g).to(DEV), torch.randn(B, Tk, kd, generator=g).to(DEV)


TILE_CASES = [(dh, T) for dh in (36, 52) for T in (5, 31, 32, 33, 127, 128, 129, 300, 1250)] + [(dh, T) for dh in (40, 44, 48, 56, 60) for T in (33, 129)]


@pytest.mark.parametrize("dh,T", TILE_CASES)
def test_mid_attention_tile(dh, T):
    """Self-attention, 128-query tiles: 32-key stage edges, 32-query wave edges, the 128-query block edge, 1250 = 30 s of audio.
    Measured on MI355X: the largest ratio over the 32 shapes is 1.66e-6 (dh = 36, T = 1250, fused buffer, no lens); 1.32e-6 at dh = 52, T = 1250; below
    8.4e-7 everywhere else."""
    H, B = 2, 3
    g = torch.Generator().manual_seed(1000 * dh + T)
    worst = 0.0
    for fused in (True, False):
        q, k, v = operands(g, B, T, T, H, H, dh, fused)
        for lens in ([T, max(T // 2, 1), 1], None):
            worst = max(worst, run_case(f"dh={dh} T={T} fused={fused} lens={lens}", q, k, v, H, H, dh, lens, lens))
    print(f"mid_attention tile dh={dh} T={T}: worst max|err| / max|want| = {worst:.2e}")


@pytest.mark.parametrize("dh", [36, 52])
@pytest.mark.parametrize("Tq,Tk", [(5, 40), (33, 129), (130, 31)])
def test_mid_attention_cross(dh, Tq, Tk):
    """Tq != Tk with independent ragged lengths on both sides, and 2 query heads on 1 kv head."""
    B = 3
    g = torch.Generator().manual_seed(7000 + 100 * dh + Tq)
    for H, KH in ((2, 2), (2, 1)):
        q, k, v = operands(g, B, Tq, Tk, H, KH, dh, False)
        run_case(f"cross dh={dh} {Tq}x{Tk} H={H}/{KH} no lens", q, k, v, H, KH, dh)
        run_case(f"cross dh={dh} {Tq}x{Tk} H={H}/{KH} ragged", q, k, v, H, KH, dh, [Tq, max(Tq // 3, 1), 2], [max(Tk // 2, 1), Tk, 1])
        run_case(f"cross dh={dh} {Tq}x{Tk} H={H}/{KH} lens_k only", q, k, v, H, KH, dh, None, [Tk, 1, max(Tk - 1, 1)])


@pytest.mark.parametrize("dh", [36, 52])
@pytest.mark.parametrize("Tq,Tk", [(5, 5), (33, 33), (129, 129), (5, 40), (33, 129)])
def test_mid_attention_causal(dh, Tq, Tk):
    """The causal form: the queries are the last len_q positions of the len_k keys (a prefix of Tk - Tq cached keys when Tq < Tk)."""
    B, H = 3, 2
    g = torch.Generator().manual_seed(9000 + 100 * dh + Tq + Tk)
    q, k, v = operands(g, B, Tq, Tk, H, H, dh, Tq == Tk)
    run_case(f"causal dh={dh} {Tq}x{Tk}", q, k, v, H, H, dh, causal=True)
    lq = [Tq, max(Tq // 2, 1), 1]
    run_case(f"causal dh={dh} {Tq}x{Tk} ragged", q, k, v, H, H, dh, lq, [Tk, lq[1] + min(3, Tk - Tq), 1], causal=True)
    q1, k1, v1 = operands(g, B, Tq, Tk, H, 1, dh, False)
    run_case(f"causal dh={dh} {Tq}x{Tk} H=2/1", q1, k1, v1, H, 1, dh, causal=True)
    # fewer keys than queries: the first len_q - len_k queries see nothing and come back as zero rows
    run_case(f"causal dh={dh} {Tq}x{Tk} short keys", q, k, v, H, H, dh, [Tq, Tq, 2], [max(Tq - 2, 1), 1, 1], causal=True)


@pytest.mark.parametrize("dh", [36, 52])
@pytest.mark.parametrize("Tk", [1, 63, 64, 65, 200, 1250])
def test_mid_attention_one_query(dh, Tk):
    """The few-query form at Tq = 1: 64-key chunk edges and many chunks (no 512 cap)."""
    B, H = 3, 2
    g = torch.Generator().manual_seed(11000 + 100 * dh + Tk)
    for KH in (2, 1):
        q, k, v = operands(g, B, 1, Tk, H, KH, dh, False)
        run_case(f"few dh={dh} 1x{Tk} H={H}/{KH}", q, k, v, H, KH, dh)
        run_case(f"few dh={dh} 1x{Tk} H={H}/{KH} lens_k", q, k, v, H, KH, dh, None, [Tk, max(Tk // 2, 1), 1])
        run_case(f"few dh={dh} 1x{Tk} H={H}/{KH} causal", q, k, v, H, KH, dh, causal=True)


@pytest.mark.parametrize("dh", [36, 40, 44, 48, 52, 56, 60])
@pytest.mark.parametrize("Tk", [4, 70])
def test_mid_attention_four_queries_causal(dh, Tk):
    """Tq = 4 causal over Tk keys (a T > 1 decoder call over a cache), and k / v as a strided slice of a preallocated cache."""
    B, H, KH, Tq = 3, 2, 1, 4
    g = torch.Generator().manual_seed(13000 + 100 * dh + Tk)
    q = torch.randn(B, Tq, H * dh, generator=g).to(DEV)
    cache = torch.randn(B, Tk + 9, 2 * KH * dh, generator=g).to(DEV)   # k | v side by side, more rows than the call sees
    cache[:, Tk:] = float("nan")                                     # rows behind the slice are never read
    k, v = cache[:, :Tk, :KH * dh], cache[:, :Tk, KH * dh:]
    run_case(f"few dh={dh} 4x{Tk} causal cache", q, k, v, H, KH, dh, causal=True)
    run_case(f"few dh={dh} 4x{Tk} causal cache ragged", q, k, v, H, KH, dh, [4, 2, 1], [Tk, Tk - 1, 1], causal=True)
    run_case(f"few dh={dh} 4x{Tk} cache", q, k, v, H, KH, dh)
    # fewer keys than queries: the first len_q - len_k queries see nothing and come back as zero rows
    run_case(f"few dh={dh} 4x{Tk} causal short keys", q, k, v, H, KH, dh, [4, 4, 2], [2, 1, 1], causal=True)


@pytest.mark.parametrize("dh", [36, 52])
def test_mid_attention_dispatch_boundary(dh):
    """Tq = 4 (one wavefront per query) and Tq = 5 (the tile) on the same data: each within the bar of float64, and of each other."""
    from mlx_audio_amd import ops

    B, H, Tk = 2, 2, 70
    g = torch.Generator().manual_seed(15000 + dh)
    q5, k, v = operands(g, B, 5, Tk, H, H, dh, False)
    q4 = q5[:, :4]
    run_case(f"boundary dh={dh} Tq=4", q4, k, v, H, H, dh)
    run_case(f"boundary dh={dh} Tq=5", q5, k, v, H, H, dh)
    o4 = torch.full((B, 4, H * dh), float("nan"), device=DEV)
    o5 = torch.full((B, 5, H * dh), float("nan"), device=DEV)
    ops.mid_attention(q4, k, v, o4, heads=H, dh=dh)
    ops.mid_attention(q5, k, v, o5, heads=H, dh=dh)
    torch.cuda.synchronize()
    gap = float((o4 - o5[:, :4]).abs().max() / o5.abs().max())
    print(f"mid_attention boundary dh={dh}: few vs tile max|diff| / max = {gap:.2e}")
    assert gap < BAR, gap


def test_mid_attention_refusals():
    from mlx_audio_amd import _lib, ops

    T = 40

    def refused(match, q, k, v, out, **kw):
        with pytest.raises(_lib.Mi355Error, match=match):
            ops.mid_attention(q, k, v, out, **kw)
        torch.cuda.synchronize()
        assert bool((out == 7.0).all()), "a refused call wrote its output"

    for dh in (32, 64, 38):
        q = torch.randn(1, T, 2 * dh + 2, device=DEV)[:, :, :2 * dh] if dh == 38 else torch.randn(1, T, 2 * dh, device=DEV)
        refused("dh must be", q, q, q, torch.full_like(q, 7.0), heads=2, dh=dh)
    buf = torch.randn(1, T, 2 * 36 + 4, device=DEV)
    q = buf[:, :, :72]
    refused("16-byte aligned", buf[:, :, 1:73], q, q, torch.full_like(q, 7.0), heads=2, dh=36)       # a pointer 4 bytes off
    odd = torch.randn(1, T, 74, device=DEV)[:, :, :72]
    refused("16-byte aligned", q, odd, q, torch.full_like(q, 7.0), heads=2, dh=36)                    # a row stride of 74 floats
    q3 = torch.randn(1, T, 3 * 36, device=DEV)
    refused("multiple of kv_heads", q3, q, q, torch.full_like(q3, 7.0), heads=3, kv_heads=2, dh=36)
    q3 = torch.randn(3, T, 72, device=DEV)
    refused("lens_k", q3, q3, q3, torch.full_like(q3, 7.0), heads=2, dh=36, lens_k=torch.tensor([T, 0, 3], dtype=torch.int32, device=DEV))
    out = torch.full_like(q3, 7.0)
    ops.mid_attention(q3, q3, q3, out, heads=2, dh=36, lens_k=torch.tensor([T, 1, 3], dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and not bool((out == 7.0).any())


# ---------------------------------------------------------------------------------------------------- partial_rope
U = 2.0 ** -24   # unit roundoff of float32


def rope_ref(x, heads, dh, rot, cos, sin, pos0):
    """apply_rotary_pos_emb in float64 on the float32 tables: (want, bound) [B, L, heads dh].  The kernel rounds x c, x' s and their sum once each:
    |err| <= U (|x c| + |x' s| + |r|) (1 + O(U)); pass-through channels have bound 0."""
    B, L, _ = x.shape
    x4 = x.double().reshape(B, L, heads, dh)
    c = cos.double()[pos0:pos0 + L].repeat_interleave(2, dim=1)[None, :, None, :]
    s = sin.double()[pos0:pos0 + L].repeat_interleave(2, dim=1)[None, :, None, :]
    xr = x4[..., :rot]
    rh = torch.stack([-xr[..., 1::2], xr[..., 0::2]], dim=-1).reshape(xr.shape)
    r = xr * c + rh * s
    want = torch.cat([r, x4[..., rot:]], dim=-1)
    bound = torch.cat([U * ((xr * c).abs() + (rh * s).abs() + r.abs()) * 1.001, torch.zeros_like(x4[..., rot:])], dim=-1)
    return want.reshape(B, L, heads * dh), bound.reshape(B, L, heads * dh)


@pytest.mark.parametrize("dh,rot", [(36, 32), (52, 46), (40, 40), (36, 2)])
@pytest.mark.parametrize("L", [1, 5, 300])
@pytest.mark.parametrize("pos0", [0, 7])
def test_partial_rope(dh, rot, L, pos0):
    from mlx_audio_amd import ops

    B, H, H2 = 3, 4, 2
    g = torch.Generator().manual_seed(17000 + 100 * dh + 10 * rot + L + pos0)
    cos, sin = ops.moonshine_rope_tables(rot, pos0 + L, device=DEV)
    lens = [L, max(L // 2, 1), 1]
    ld = torch.tensor(lens, dtype=torch.int32, device=DEV)
    # (a) in place on the q | k thirds of a fused buffer, ragged: rows beyond lens and the v third keep their bits
    buf0 = torch.randn(B, L, (H + 2 * H2) * dh, generator=g).to(DEV)
    buf = buf0.clone()
    xq, xk = buf[:, :, :H * dh], buf[:, :, H * dh:(H + H2) * dh]
    ops.partial_rope(xq, xq, heads=H, dh=dh, rot=rot, cos=cos, sin=sin, pos0=pos0, lens=ld, second=(xk, xk, H2))
    # (b) out of place, the second operand into a strided cache row range at pos0, no lens
    yq = torch.full((B, L, H * dh), float("nan"), device=DEV)
    cache0 = torch.randn(B, pos0 + L + 3, 2 * H2 * dh, generator=g).to(DEV)
    cache = cache0.clone()
    ops.partial_rope(buf0[:, :, :H * dh], yq, heads=H, dh=dh, rot=rot, cos=cos, sin=sin, pos0=pos0,
                     second=(buf0[:, :, H * dh:(H + H2) * dh], cache[:, pos0:pos0 + L, :H2 * dh], H2))
    torch.cuda.synchronize()
    wq, bq = rope_ref(buf0[:, :, :H * dh].cpu(), H, dh, rot, cos.cpu(), sin.cpu(), pos0)
    wk, bk = rope_ref(buf0[:, :, H * dh:(H + H2) * dh].cpu(), H2, dh, rot, cos.cpu(), sin.cpu(), pos0)
    passq = (torch.arange(H * dh) % dh) >= rot
    passk = (torch.arange(H2 * dh) % dh) >= rot
    worst = 0.0
    for name, got, src, want, bound, pas, ragged in (("q in place", xq, buf0[:, :, :H * dh], wq, bq, passq, True),
                                                    ("k in place", xk, buf0[:, :, H * dh:(H + H2) * dh], wk, bk, passk, True),
                                                    ("q out of place", yq, buf0[:, :, :H * dh], wq, bq, passq, False),
                                                    ("k into the cache", cache[:, pos0:pos0 + L, :H2 * dh], buf0[:, :, H * dh:(H + H2) * dh], wk, bk, passk, False)):
        got, src = got.cpu(), src.cpu()
        for b in range(B):
            n = lens[b] if ragged else L
            assert torch.equal(got[b, n:], src[b, n:]), f"{name}: rows beyond lens changed"
            assert torch.equal(got[b, :n][:, pas], src[b, :n][:, pas]), f"{name}: pass-through channels are not bit-equal to the input"
            err = (got[b, :n].double() - want[b, :n]).abs()
            assert bool((err <= bound[b, :n]).all()), (name, b, float((err - bound[b, :n]).max()))
            rot_cols = ~pas
            worst = max(worst, float((err[:, rot_cols] / bound[b, :n][:, rot_cols].clamp_min(1e-300)).max()))
    print(f"partial_rope dh={dh} rot={rot} L={L} pos0={pos0}: worst |err| / bound = {worst:.3f}")
    assert torch.equal(buf[:, :, (H + H2) * dh:], buf0[:, :, (H + H2) * dh:]), "the v third changed"
    untouched = torch.ones(cache.shape[1], dtype=torch.bool)
    untouched[pos0:pos0 + L] = False
    assert torch.equal(cache[:, untouched], cache0[:, untouched]) and torch.equal(cache[:, :, H2 * dh:], cache0[:, :, H2 * dh:]), "cache rows outside the slot changed"


@pytest.mark.parametrize("dh,rot", [(36, 32), (52, 46)])
def test_partial_rope_against_reference_run(dh, rot):
    """The reference's own apply_rotary_pos_emb (tests/golden/make_moonshine_rope_fixtures.py: float32 numpy, every product and the sum rounded once)
    on q (4 heads) and k (2 heads) at positions 7 .. 12: the kernel rounds the same three operations, so the bits are equal."""
    import os

    import numpy as np

    from mlx_audio_amd import ops

    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_moonshine_rope.npz"))
    q, k = torch.from_numpy(z[f"q{dh}"])[None].to(DEV), torch.from_numpy(z[f"k{dh}"])[None].to(DEV)
    L = q.shape[1]
    cos, sin = ops.moonshine_rope_tables(rot, 7 + L, device=DEV)
    yq, yk = torch.full_like(q, float("nan")), torch.full_like(k, float("nan"))
    ops.partial_rope(q, yq, heads=4, dh=dh, rot=rot, cos=cos, sin=sin, pos0=7, second=(k, yk, 2))
    torch.cuda.synchronize()
    assert torch.equal(yq[0].cpu(), torch.from_numpy(z[f"qe{dh}"])) and torch.equal(yk[0].cpu(), torch.from_numpy(z[f"ke{dh}"]))


def test_partial_rope_refusals():
    from mlx_audio_amd import _lib, ops

    cos, sin = ops.moonshine_rope_tables(32, 10, device=DEV)
    x = torch.randn(2, 5, 4 * 36, device=DEV)
    for kw, match in ((dict(pos0=6), "past the 10-row"), (dict(pos0=0, rot=30), None), (dict(pos0=-1), "past the 10-row")):
        y = torch.full_like(x, 7.0)
        if match is None:   # the tables do not fit the rot asked for: the front end's own check
            with pytest.raises(AssertionError):
                ops.partial_rope(x, y, heads=4, dh=36, cos=cos, sin=sin, **kw)
        else:
            with pytest.raises(_lib.Mi355Error, match=match):
                ops.partial_rope(x, y, heads=4, dh=36, rot=32, cos=cos, sin=sin, **kw)
        torch.cuda.synchronize()
        assert bool((y == 7.0).all()), "a refused call wrote its output"
    c3, s3 = ops.moonshine_rope_tables(38, 10, device=DEV)
    y = torch.full_like(x, 7.0)
    with pytest.raises(_lib.Mi355Error, match="rot must be"):
        ops.partial_rope(x, y, heads=4, dh=36, rot=38, cos=c3, sin=s3)
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())
    ops.partial_rope(x, y, heads=4, dh=36, rot=32, cos=cos, sin=sin, pos0=5)   # the last five rows of the tables: accepted
    torch.cuda.synchronize()
    assert bool(torch.isfinite(y).all()) and not bool((y == 7.0).any())
