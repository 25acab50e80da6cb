"""The reference statements of tests/test_lm_row_kernel_edges_gpu.py held to known-good implementations, and the input preconditions of its sampler
cases, on the CPU: a failure of the GPU file then cannot be the reference's fault, and a sampler case that sits on a knife edge fails here, before
any GPU run.  Statements and case tables live in tests/_lm_row_cases.py, which both files import."""
import pytest
import torch
import torch.nn.functional as F

import _lm_row_cases as S
import _ops_emu


@pytest.mark.parametrize("c", S.comb_cases() + S.generic_cases(), ids=S.dwconv_id)
def test_dwconv_statement_is_conv1d(c):
    """dwconv_stmt (plain, dilated, Snake, ragged) against F.conv1d with groups = C on each item's first lens_in[b] rows, Snake applied to the input in
    float64 by its own formula, explicit zero padding (left ``pad``; right whatever the Lout outputs read)."""
    x, w, bias, alpha, inv = S.dwconv_inputs(c)
    got = S.dwconv_stmt(x, w, bias, pad=c["pad"], dil=c["dil"], Lout=c["Lout"], lens_in=c["lens"], alpha=alpha, inv=inv, dtype=torch.float64)
    dil, K, C = max(c["dil"], 1), c["K"], c["C"]
    for b in range(c["B"]):
        n = c["Lin"] if c["lens"] is None else c["lens"][b]
        v = x[b, :n].double()
        if alpha is not None:
            v = v + inv.double() * torch.sin(alpha.double() * v) ** 2
        right = max(0, c["Lout"] + (K - 1) * dil - c["pad"] - n)
        want = F.conv1d(F.pad(v.transpose(0, 1)[None], (c["pad"], right)), w.double()[:, None, :], None if bias is None else bias.double(), dilation=dil,
                        groups=C)[0, :, :c["Lout"]].transpose(0, 1)
        assert want.shape == got[b].shape
        assert float((got[b] - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))


@pytest.mark.parametrize("c", S.transposed_cases(), ids=S.dwconv_id)
def test_dwconv_transposed_statement_is_conv_transpose1d(c):
    """The header's sum over t * stride + k - pad == n against F.conv_transpose1d (groups = C), trimmed / padded to Lout."""
    x, w, bias, _, _ = S.dwconv_inputs(c)
    kw = dict(stride=c["stride"], pad=c["pad"], Lout=c["Lout"], lens_in=c["lens"], dtype=torch.float64)
    got, want = S.dwconv_t_stmt(x, w, bias, **kw), S.dwconv_t_ref(x, w, bias, **kw)
    assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))


def test_dwconv_emulation_has_no_stride():
    """tests/_ops_emu.py::dwconv refuses a strided plain conv like mi355_dwconv does, and agrees with the statement otherwise."""
    c = dict(K=7, dil=3, snake=True, pad=9, Lin=25, Lout=25, C=40, B=2, lens=None, bias=True)
    x, w, bias, alpha, inv = S.dwconv_inputs(c)
    y = torch.empty(2, 25, 40, dtype=torch.float64)
    _ops_emu.dwconv(x, w, bias, y, pad=9, dil=3, pre_alpha=alpha, pre_inv=inv)
    assert float((y - S.dwconv_stmt(x, w, bias, pad=9, dil=3, Lout=25, alpha=alpha, inv=inv)).abs().max()) <= 1e-12
    with pytest.raises(AssertionError, match="no stride"):
        _ops_emu.dwconv(x, w, bias, y, pad=9, stride=2)
    yt = torch.empty(2, 50, 40, dtype=torch.float64)
    _ops_emu.dwconv(x, w[:, :4].contiguous(), None, yt, stride=2, transpose=True)   # the transposed conv keeps its stride
    assert float((yt - S.dwconv_t_ref(x, w[:, :4], None, stride=2, pad=0, Lout=50)).abs().max()) <= 1e-12


@pytest.mark.parametrize("Q,C,so,add,scale", [(1, 64, False, False, 1.0), (9, 4, True, True, 0.5), (17, 64, True, False, 0.0), (33, 1028, False, True, 1.0)])
def test_embed_sum_statement_is_the_emulation(Q, C, so, add, scale):
    """embed_sum_stmt in float64 against tests/_ops_emu.py::embed_sum (a different formulation: masked slots add a zero row), with masks in the first,
    the last and all slots of a row."""
    g = torch.Generator().manual_seed(Q * 10000 + C)
    B, L, rows = 2, 3, 11
    table = torch.randn(rows * Q, C, generator=g)
    ids = torch.randint(0, rows, (B, L, Q), generator=g, dtype=torch.int32)
    ids[0, 0, 0] = ids[0, 1, Q - 1] = -1
    ids[1, 2, :] = -1
    offs = torch.arange(Q, dtype=torch.int32) * rows if so else None
    a = torch.randn(B, L, C, generator=g) if add else None
    got = S.embed_sum_stmt(table, ids, offs, a, scale, torch.float64)
    want = _ops_emu.embed_sum(table, ids, torch.empty(B, L, C, dtype=torch.float64), slot_offset=offs, add=a, scale=1.0 if scale == 0 else scale)
    assert float((got - want).abs().max()) <= 1e-12
    if not add:
        assert float(got[1, 2].abs().max()) == 0.0   # every slot masked, nothing added: zeros


@pytest.mark.parametrize("interleaved", [False, True])
@pytest.mark.parametrize("dh", [64, 128])
def test_rope_statement_is_apply_rope(dh, interleaved):
    """rope_stmt (the header's pairs, index by index) against oracle.lm_ref.apply_rope, which the reference's own modules pin; and the position rule:
    pos - pos_sub clamped to rows 0 and rope_rows - 1."""
    from oracle.lm_ref import StackConfig, apply_rope, rope_tables

    cfg = StackConfig(d_model=64, n_layers=1, n_heads=2, n_kv_heads=2, head_dim=dh, d_ff=64, rope_theta=10000.0, max_pos=16)
    cos, sin = rope_tables(cfg)
    g = torch.Generator().manual_seed(dh)
    B, L, H = 2, 5, 3
    x = torch.randn(B, L, H, dh, generator=g, dtype=torch.float64)
    pos = torch.tensor([[3, 9, 0, 15, 1, 99], [14, 15, 16, 17, 2, 99]], dtype=torch.int32)
    p = S.rope_positions(B, L, 16, pos=pos, pos_sub=torch.tensor([2, 0], dtype=torch.int32))
    assert p.tolist() == [[1, 7, 0, 13, 0], [14, 15, 15, 15, 2]]
    assert S.rope_positions(2, 3, 16, pos0=4).tolist() == [[4, 5, 6]] * 2
    got = S.rope_stmt(x, cos[p].double(), sin[p].double(), interleaved)
    for b in range(B):
        assert torch.equal(got[b:b + 1], apply_rope(x[b:b + 1], cos[p[b]].double(), sin[p[b]].double(), interleaved))
    ref = S.head_norm_rope_ref(x.reshape(B, L, H * dh), H, dh, None, 1e-6, cos, sin, p, interleaved, torch.float64)
    assert torch.equal(ref, got.reshape(B, L, H * dh))


SPECS = S.sampler_specs()


def test_sampler_case_table_covers_the_issue():
    names = [s["name"] for s in SPECS]
    assert len(set(names)) == len(names)
    assert sorted({s["V"] for s in SPECS if s["name"].endswith("-defaults")}) == S.SAMPLER_V
    assert all(s["B"] <= 4 for s in SPECS)


@pytest.mark.parametrize("spec", SPECS, ids=lambda s: s["name"])
def test_sampler_case_preconditions(spec):
    """Every sampler case of the GPU file, before any GPU run: float32 / float64 survivors equal, every cumulative probability and log-probability
    P_MARGIN from its threshold, top-2 gap of the draw at least THR, at least ``min_alive`` survivors per row -- so that no entry of any case is
    excluded from the device comparison.  Also what a case knows without the oracle (which ties survive)."""
    case = S.build_case(spec)
    margins = S.sampler_preconditions(case)
    print("SAMPLER-PRE", spec["name"], margins)
    f, _ = S.oracle_run(case)
    for key, want in (("alive", True), ("dead", False)):
        if case[key] is not None:
            assert bool((torch.isfinite(f[:, case[key]]) == want).all()), (spec["name"], key)
    if spec["kind"] in ("few_finite", "minp1"):
        assert int(torch.isfinite(f).sum()) == spec["B"] * 3
    if spec["kind"] == "ties":
        assert int(torch.isfinite(f).sum()) == spec["B"] * spec["kw"]["top_k"]
