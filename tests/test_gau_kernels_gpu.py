"""``mi355_gau_kv`` and ``mi355_gau_attention`` against their float64 contracts (``tests/_ops_emu_mossformer2.py``) on the same float32 inputs.

The bound is per element and derived there, not tuned: every contraction of ``n`` terms is held to ``n * 2^-24 * sum |terms|`` and propagated in
float64 through S -> S^2 -> A -> gate, with the stated ulp allowances for the rope's products and the sigmoid.  Each test prints the largest
error / bound ratio it saw (docs/COVERAGE.md records them)."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import _ops_emu_mossformer2 as E64  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [(T, E) for T in (1, 2, 255, 256, 257, 513) for E in (64, 256)]


def _inputs(B, T, E, seed, ldqk=128, ldvu=None):
    g = torch.Generator().manual_seed(seed)
    ldvu = ldvu or E
    qk_buf = torch.randn(B, T, ldqk, generator=g) * 2.0
    vu_buf = torch.randn(B, T, ldvu, generator=g)
    gamma = 1.0 + 0.1 * torch.randn(4, 128, generator=g)
    beta = 0.1 * torch.randn(4, 128, generator=g)
    return qk_buf, vu_buf, gamma, beta


_CACHE = {}


def _case(T, E):
    """One B = 1 case: inputs, float32 tables, the float64 kv and attention with their bounds -- computed once, shared, never written to."""
    if (T, E) not in _CACHE:
        from mlx_audio_amd import ops

        qk, vu, gamma, beta = _inputs(1, T, E, seed=1000 * T + E)
        cos, sin = ops.gau_rope_tables(T)
        kv64, kvb = E64.gau_kv64(qk, vu, gamma, beta, cos, sin)
        kv32 = kv64.float()
        out64, ob, quad, lin = E64.gau_attention64(qk, vu, kv32, gamma, beta, cos, sin, parts=True)
        _CACHE[(T, E)] = dict(qk=qk, vu=vu, gamma=gamma, beta=beta, cos=cos, sin=sin, kv64=kv64, kvb=kvb, kv32=kv32, out64=out64, ob=ob, quad=quad, lin=lin)
    return _CACHE[(T, E)]


def _ratio(got, want, bound):
    err = (got.double().cpu() - want).abs()
    assert torch.isfinite(err).all()
    assert bool((err <= bound).all()), f"largest error {float(err.max()):.3e}, largest error / bound {float((err / bound.clamp(min=1e-300)).max()):.3f}"
    return float((err / bound.clamp(min=1e-300)).max())


def _dev(c, *names):
    return [c[n].to(DEV) for n in names]


@pytest.mark.parametrize("T,E", SIZES)
def test_kv_against_float64(T, E):
    from mlx_audio_amd import ops

    c = _case(T, E)
    qk, vu, gamma, beta, cos, sin = _dev(c, "qk", "vu", "gamma", "beta", "cos", "sin")
    kv = ops.gau_kv(qk, vu, gamma, beta, (cos, sin))
    r = _ratio(kv, c["kv64"], c["kvb"])
    print(f"gau_kv T={T} E={E}: largest error / bound {r:.3f}")


@pytest.mark.parametrize("T,E", SIZES)
def test_attention_against_float64(T, E):
    from mlx_audio_amd import ops

    c = _case(T, E)
    if T >= 255:   # both terms carry weight in what is compared
        q2, l2 = float((c["quad"] ** 2).sum()), float((c["lin"] ** 2).sum())
        assert min(q2, l2) > 0.05 * (q2 + l2), (q2, l2)
    qk, vu, gamma, beta, cos, sin, kv = _dev(c, "qk", "vu", "gamma", "beta", "cos", "sin", "kv32")
    out = torch.full((1, T, E // 2), float("nan"), device=DEV)
    ops.gau_attention(qk, vu, kv, gamma, beta, (cos, sin), out)
    r = _ratio(out, c["out64"], c["ob"])
    print(f"gau_attention T={T} E={E}: largest error / bound {r:.3f}")
    again = torch.empty_like(out)
    ops.gau_attention(qk, vu, kv, gamma, beta, (cos, sin), again)
    assert torch.equal(out, again)


@pytest.fixture(scope="module")
def ragged():
    """B = 3, lens = [513, 256, 1]; qk rows of 160 floats, vu a strided view (columns 64 .. 64 + E of rows of E + 96 floats)."""
    from mlx_audio_amd import ops

    B, T, E = 3, 513, 256
    lens = [513, 256, 1]
    qk_buf, vu_buf, gamma, beta = _inputs(B, T, E, seed=77, ldqk=160, ldvu=E + 96)
    qk, vu = qk_buf[:, :, :128], vu_buf[:, :, 64:64 + E]
    cos, sin = ops.gau_rope_tables(T + 3)
    kv64, kvb = E64.gau_kv64(qk, vu, gamma, beta, cos, sin, lens)
    kv32 = kv64.float()
    out64, ob = E64.gau_attention64(qk, vu, kv32, gamma, beta, cos, sin, lens)
    d = dict(B=B, T=T, E=E, lens=lens, kv64=kv64, kvb=kvb, out64=out64, ob=ob)
    d["qk"], d["vu"] = qk_buf.to(DEV)[:, :, :128], vu_buf.to(DEV)[:, :, 64:64 + E]
    d["gamma"], d["beta"], d["rope"] = gamma.to(DEV), beta.to(DEV), (cos.to(DEV), sin.to(DEV))
    d["lens_dev"] = torch.tensor(lens, dtype=torch.int32, device=DEV)
    d["kv"] = ops.gau_kv(d["qk"], d["vu"], d["gamma"], d["beta"], d["rope"], lens=d["lens_dev"])
    obuf = torch.full((B, T, E // 2 + 32), float("nan"), device=DEV)
    d["out_buf"] = obuf
    d["out"] = ops.gau_attention(d["qk"], d["vu"], kv32.to(DEV), d["gamma"], d["beta"], d["rope"], obuf[:, :, :E // 2], lens=d["lens_dev"])
    return d


def test_ragged_batch_against_float64_and_zero_rows(ragged):
    d = ragged
    r = _ratio(d["kv"], d["kv64"], d["kvb"])
    print(f"gau_kv ragged: largest error / bound {r:.3f}")
    r = _ratio(d["out"], d["out64"], d["ob"])
    print(f"gau_attention ragged: largest error / bound {r:.3f}")
    for b, n in enumerate(d["lens"]):
        assert not d["out"][b, n:].any()
    assert torch.isnan(d["out_buf"][:, :, d["E"] // 2:]).all()   # nothing written beyond the width


def test_ragged_items_are_bit_equal_to_the_items_alone_and_calls_repeat(ragged):
    from mlx_audio_amd import ops

    d = ragged
    E = d["E"]
    kv2 = ops.gau_kv(d["qk"], d["vu"], d["gamma"], d["beta"], d["rope"], lens=d["lens_dev"])
    assert torch.equal(kv2, d["kv"])
    kv_in = d["kv64"].float().to(DEV)
    for b, n in enumerate(d["lens"]):
        qk1, vu1 = d["qk"][b:b + 1, :n].contiguous(), d["vu"][b:b + 1, :n].contiguous()
        kv1 = ops.gau_kv(qk1, vu1, d["gamma"], d["beta"], d["rope"])
        assert torch.equal(kv1[0], d["kv"][b]), b
        out1 = torch.empty((1, n, E // 2), device=DEV)
        ops.gau_attention(qk1, vu1, kv_in[b:b + 1].contiguous(), d["gamma"], d["beta"], d["rope"], out1)
        assert torch.equal(out1[0], d["out"][b, :n]), b


@pytest.mark.parametrize("cols", [32, 64, 128])
def test_columns_per_workgroup_never_change_a_bit(ragged, cols):
    from mlx_audio_amd import ops

    d = ragged
    out = torch.empty((d["B"], d["T"], d["E"] // 2), device=DEV)
    ops.gau_attention(d["qk"], d["vu"], d["kv64"].float().to(DEV), d["gamma"], d["beta"], d["rope"], out, lens=d["lens_dev"], cols=cols)
    assert torch.equal(out, d["out"])


def test_all_negative_scores_give_a_quadratic_part_of_exactly_zero():
    """quad_q > 0 and quad_k < 0 in every column that does not rotate, zeros in those that do: every score is negative, relu^2 is 0.  With kv = 0
    the whole of A is then exactly zero and so is the output."""
    from mlx_audio_amd import ops

    T, E = 300, 64
    g = torch.Generator().manual_seed(5)
    qk = torch.rand(1, T, 128, generator=g) + 0.5
    qk[:, :, :32] = 0
    vu = torch.randn(1, T, E, generator=g)
    gamma = torch.ones(4, 128)
    gamma[2] = -1.0
    beta = torch.zeros(4, 128)
    cos, sin = ops.gau_rope_tables(T)
    out = torch.full((1, T, E // 2), float("nan"), device=DEV)
    ops.gau_attention(qk.to(DEV), vu.to(DEV), torch.zeros(1, 128, E, device=DEV), gamma.to(DEV), beta.to(DEV), (cos.to(DEV), sin.to(DEV)), out)
    assert not out.any() and not torch.isnan(out).any()


def test_refusals():
    from mlx_audio_amd import _lib, ops

    T = 8

    def run(E=64, rope_rows=T, **kw):
        qk, vu, gamma, beta = _inputs(1, T, E, seed=3)
        cos, sin = ops.gau_rope_tables(rope_rows, DEV)
        out = torch.empty((1, T, E // 2), device=DEV)
        return ops.gau_attention(qk.to(DEV), vu.to(DEV), torch.zeros(1, 128, E, device=DEV), gamma.to(DEV), beta.to(DEV), (cos, sin), out, **kw)

    run()
    for kw, word in ((dict(causal=True), "causal"), (dict(qk_dim=64), "qk_dim"), (dict(group=128), "group"), (dict(E=96), "multiple of 64"),
                     (dict(E=4096), "multiple of 64"), (dict(rope_rows=T - 1), "rope"), (dict(cols=48), "cols"), (dict(cols=64), "cols")):
        with pytest.raises(_lib.Mi355Error, match=word):
            run(**kw)
    qk, vu, gamma, beta = _inputs(1, T, 96, seed=3)
    with pytest.raises(_lib.Mi355Error, match="multiple of 64"):
        ops.gau_kv(qk.to(DEV), vu.to(DEV), gamma.to(DEV), beta.to(DEV), ops.gau_rope_tables(T, DEV))
    qk, vu, gamma, beta = _inputs(1, T, 64, seed=3)
    with pytest.raises(_lib.Mi355Error, match="workspace"):
        ops.gau_kv(qk.to(DEV), vu.to(DEV), gamma.to(DEV), beta.to(DEV), ops.gau_rope_tables(T, DEV), ws=torch.empty(16, device=DEV))
