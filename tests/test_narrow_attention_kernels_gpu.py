"""``csrc/narrow_attn.hip`` against float64 on the host.  The reference restates the module's own order (sortformer.py:557-563 under the mask of
621-631: scale q, scores, ADDITIVE -1e4 on padded keys, softmax over all T keys, @ v), not the kernel's formulation (hidden keys, log2 domain)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"

NARROW_T = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257, 513, 1125]   # tile edges (32 keys, 32 queries per wave, 128 per block), 513 = one past
                                                                           # mi355_attention's cap, 1125 = 90 s of audio
BAR = 2e-6   # the f32 flash kernel's bar (tests/test_lm_kernels_gpu.py): the same arithmetic, one dh-long contraction, fp32 MFMA, online softmax


def module_ref(q, k, v, lens, H, dh):
    """[B, T, H dh] float64 through TransformerAttention's lines: every item sees all T keys, the padded ones behind -1e4."""
    B, T, _ = q.shape
    scale = dh ** -0.5
    q4, k4, v4 = (t.double().reshape(B, T, H, dh).permute(0, 2, 1, 3) for t in (q, k, v))
    scores = (q4 * scale) @ k4.transpose(2, 3)
    if lens is not None:
        valid = torch.arange(T)[None, :] < torch.tensor(lens)[:, None]
        scores = scores + (~valid)[:, None, None, :].double() * -1e4
    attn = torch.softmax(scores, dim=-1)
    return (attn @ v4).permute(0, 2, 1, 3).reshape(B, T, H * dh)


@pytest.mark.parametrize("dh", [8, 16, 24, 32])
@pytest.mark.parametrize("T", NARROW_T)
def test_narrow_attention(dh, T):
    """max |got - want| / max |want| < 2e-6 per call over the valid rows; rows at and beyond ``lens`` exactly zero; two calls bitwise equal; the
    outputs start as NaN.
    Measured on MI355X: the largest ratio over the 56 cases is 1.39e-6 (dh = 16, T = 1125, separate buffers, no lens); 1.2e-6 at dh = 32, T = 1125."""
    from mlx_audio_amd import ops

    H, B = 2, 3
    hd = H * dh
    g = torch.Generator().manual_seed(1000 * dh + T)
    worst = 0.0
    for fused in (True, False):
        if fused:
            buf = torch.randn(B, T, 3 * hd, generator=g).to(DEV)
            q, k, v = buf[:, :, :hd], buf[:, :, hd:2 * hd], buf[:, :, 2 * hd:]
        else:
            q, k, v = (torch.randn(B, T, hd, generator=g).to(DEV) for _ in range(3))
        for lens in ([T, max(T // 2, 1), 1], None):
            ld = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
            out = torch.full((B, T, hd), float("nan"), device=DEV)
            ops.narrow_attention(q, k, v, out, heads=H, dh=dh, lens=ld)
            out2 = torch.full((B, T, hd), float("nan"), device=DEV)
            ops.narrow_attention(q, k, v, out2, heads=H, dh=dh, lens=ld)
            torch.cuda.synchronize()
            assert torch.equal(out, out2), "two calls on the same bytes differ"
            got = out.double().cpu()
            want = module_ref(q.cpu(), k.cpu(), v.cpu(), lens, H, dh)
            err = peak = 0.0
            for b in range(B):
                n = T if lens is None else lens[b]
                err = max(err, float((got[b, :n] - want[b, :n]).abs().max()))
                peak = max(peak, float(want[b, :n].abs().max()))
                assert not got[b, n:].any(), "rows beyond lens are not exactly zero"
            worst = max(worst, err / peak)
            print(f"narrow_attention dh={dh} T={T} fused={fused} lens={lens}: max|err| / max|want| = {err / peak:.2e}")
            assert err / peak < BAR, (fused, lens, err / peak)
    print(f"narrow_attention dh={dh} T={T}: worst max|err| / max|want| = {worst:.2e}")


def test_narrow_attention_refusals():
    from mlx_audio_amd import _lib, ops

    T = 40
    for dh in (12, 40, 64):
        q = torch.randn(1, T, 2 * dh, device=DEV)
        out = torch.full_like(q, 7.0)
        with pytest.raises(_lib.Mi355Error, match="dh"):
            ops.narrow_attention(q, q, q, out, heads=2, dh=dh)
        torch.cuda.synchronize()
        assert bool((out == 7.0).all()), "a refused call wrote its output"
    q = torch.randn(3, T, 48, device=DEV)
    out = torch.full_like(q, 7.0)
    with pytest.raises(_lib.Mi355Error, match="lens"):
        ops.narrow_attention(q, q, q, out, heads=2, dh=24, lens=torch.tensor([T, 0, 3], dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()), "a refused call wrote its output"
    ops.narrow_attention(q, q, q, out, heads=2, dh=24, lens=torch.tensor([T, 1, 3], dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and not bool((out == 7.0).all())
