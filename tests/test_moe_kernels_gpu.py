"""``csrc/moe.hip`` against plain torch float64 / int64 statements written here: the grouped GEMM (``ops.switch_linear``: ONE launch of the tile
kernel on its own -- the choice made for the exact cases, since SiLU cannot be integer-exact; ``switch_glu`` runs the same kernel twice), the full
``ops.switch_glu`` with combine / shared / res, the router ``ops.moe_route``, the counting sort ``ops.moe_plan``, and the refusals.  Outputs start
as NaN inside sentinel guards; a repeat is bit-equal; a token inside a batch is bit-equal to that token routed alone.  Every rounding test prints
its largest error / bound (``pytest -s``; docs/COVERAGE.md records them)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = -777.25
TILE = 32


@pytest.fixture(scope="module")
def ops():
    from mlx_audio_amd import ops

    ops.require_gpu()
    assert ops.MOE_TILE_ROWS == TILE
    return ops


def _ids(N, E, k, g, kind="rand"):
    """[N, k] int32, distinct per token.  ``one``: every pair on expert E - 2; ``hole``: expert 1 gets no token."""
    if kind == "one":
        return torch.full((N, k), E - 2, dtype=torch.int32)
    pool = [e for e in range(E) if not (kind == "hole" and e == 1)]
    return torch.stack([torch.tensor(pool)[torch.randperm(len(pool), generator=g)[:k]] for _ in range(N)]).to(torch.int32)


def _guarded(N, k, C):
    buf = torch.full((N + 2, k, C + 4), SENT, device=DEV)
    buf[1:-1, :, :C] = float("nan")
    return buf, buf[1:-1, :, :C]


def _guards_intact(buf, C):
    return bool((buf[0] == SENT).all() and (buf[-1] == SENT).all() and (buf[1:-1, :, C:] == SENT).all())


# ------------------------------------------------------------------ grouped GEMM, exact
# (D, I, E, k, N, ids kind).  D 136: a K-step tail and a second K chunk; I 48 / 160: a dead wave / a column-tile tail; N k around one tile
# (30 / 36, 30 / 34), on both sides of 64 (62 / 66), 65 rows on one expert (three tiles, the last of one row), an expert without a token.
EXACT_CASES = [(16, 32, 1, 1, 1, "rand"), (64, 48, 4, 2, 2, "rand"), (136, 160, 64, 6, 1, "rand"), (136, 160, 64, 6, 5, "rand"),
               (136, 48, 64, 6, 6, "rand"), (64, 160, 4, 2, 15, "hole"), (64, 160, 4, 2, 17, "hole"), (16, 48, 4, 2, 31, "rand"),
               (16, 48, 4, 2, 33, "rand"), (136, 32, 4, 1, 65, "one"), (64, 160, 64, 6, 65, "rand")]


@pytest.mark.parametrize("D,I,E,k,N,kind", EXACT_CASES)
def test_switch_linear_exact(ops, D, I, E, k, N, kind):
    g = torch.Generator().manual_seed(1000 * D + 10 * I + N)
    e2 = torch.tensor([(-6, 6, 0, -3, 3, 1, -1, 5)[t % 8] for t in range(N)])
    xi = torch.randint(-4, 5, (N, D), generator=g)
    w = torch.randint(-7, 8, (E, I, D), generator=g)
    b = torch.randint(-8, 9, (E, I), generator=g)
    ids = _ids(N, E, k, g, kind)
    scale = torch.pow(2.0, e2.double())
    granule = torch.pow(2.0, e2.clamp(max=0).double())
    budget = (4 * 7 * D * scale + 8) / granule
    assert float(budget.max()) < 2 ** 24      # every partial sum is an integer multiple of the row's granule below 2^24
    want = torch.stack([torch.stack([(xi[t] @ w[int(e)].T).double() * scale[t] + b[int(e)].double() for e in ids[t]]) for t in range(N)])
    lin = ops.pack_switch_linear(w.float(), b.float(), DEV)
    x = (xi.double() * scale[:, None]).float().to(DEV)
    buf, out = _guarded(N, k, I)
    ops.switch_linear(x, lin, ids.to(DEV), out)
    got = out.cpu()
    assert _guards_intact(buf, I) and not torch.isnan(got).any()
    assert torch.equal(got.double(), want)
    buf2, out2 = _guarded(N, k, I)
    ops.switch_linear(x, lin, ids.to(DEV), out2)
    assert torch.equal(out2.cpu(), got)
    for t in {0, N // 2, N - 1}:
        alone = ops.switch_linear(x[t:t + 1], lin, ids[t:t + 1].to(DEV))
        assert torch.equal(alone.cpu()[0], got[t]), t


@pytest.mark.parametrize("D,I,E,k,N", [(136, 160, 4, 2, 17), (264, 48, 8, 6, 6)])
def test_switch_linear_against_the_emulated_split(ops, D, I, E, k, N):
    """Float operands with non-zero lo images against the bit-level emulation of the split (hi = bf16(v), lo = bf16(v - hi); hi.hi + hi.lo + lo.hi in
    float64): what remains is the accumulation alone, (3 K16 + 10) * 2^-24 of |x| @ |w|^T (+ 1 ulp) -- about 70 times tighter than the split
    residual at these depths, so a lo fragment in the wrong lane or K step (2^-9 of a product) cannot hide."""
    g = torch.Generator().manual_seed(D + N)
    x, w, b = torch.randn(N, D, generator=g) * 1.5 + 0.2, torch.randn(E, I, D, generator=g), torch.randn(E, I, generator=g)
    ids = _ids(N, E, k, g)
    hi = lambda v: v.to(torch.bfloat16).float()
    xh, wh = hi(x), hi(w)
    xl, wl = hi(x - xh).double(), hi(w - wh).double()
    xh, wh = xh.double(), wh.double()
    got = ops.switch_linear(x.to(DEV), ops.pack_switch_linear(w, b, DEV), ids.to(DEV)).cpu().double()
    for t in range(N):
        for s, e in enumerate(ids[t].tolist()):
            want = wh[e] @ xh[t] + wl[e] @ xh[t] + wh[e] @ xl[t] + b[e].double()
            bound = (3 * ((D + 15) // 16 * 16) + 10) * 2.0 ** -24 * (w[e].double().abs() @ x[t].double().abs() + b[e].double().abs()) + _ulp(want)
            assert bool(((got[t, s] - want).abs() <= bound).all()), (t, s, float(((got[t, s] - want).abs() / bound).max()))


# ------------------------------------------------------------------ switch_glu with combine, shared, res
# The bound, per element, from the kernel's arithmetic (float64 quantities of the same float32 inputs):
#   one tile GEMM of depth K:  |err| <= g(K) * (|a| @ |W|^T + |bias|) + ulp,   g(K) = 3 * 2^-16 + (3 K16 + 10) * 2^-24, K16 = K rounded up to 16
#     3 * 2^-16: the rows pipeline's 2^-8 * 2^-8 per dropped term (tests/_linear_cases.py::split_gamma), three terms here: the residual of the x
#     split, of the w split, and the lo.lo product that is never formed.  (3 K16 + 10) * 2^-24: three matrix instructions per K step, each at worst
#     a sequential chain over its 16 products, plus the K-group join, the bias add and the store.
#   S = silu(G):  |dS| <= 1.1 |dG| + 8 * 2^-24 |S|      (|silu'| <= 1.1; expf, the add, the divide and the multiply)
#   h = S * U:    |dh| <= |dS| (|U| + |dU|) + |S| |dU| + 2^-24 |h|
#   y = h @ Wd^T + bd:  |dy| <= |dh| @ |Wd|^T + g(I) (|h| @ |Wd|^T + |bd|) + ulp
#   out = sum_s w_s y_s + shared + res:  |dout| <= sum_s |w_s| |dy_s| + (k + 2) 2^-24 (sum_s |w_s y_s| + |shared| + |res|) + ulp
def _g(K):
    return 3 * 2.0 ** -16 + (3 * ((K + 15) // 16 * 16) + 10) * 2.0 ** -24


def _ulp(v):
    return torch.pow(2.0, torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -126))) - 23)


GLU_CASES = [(64, 48, 4, 2, 17, True), (136, 160, 64, 6, 5, False), (256, 96, 8, 2, 65, True), (136, 160, 64, 6, 1, True)]


@pytest.mark.parametrize("D,I,E,k,N,bias", GLU_CASES)
def test_switch_glu_against_float64(ops, D, I, E, k, N, bias):
    g = torch.Generator().manual_seed(7 * D + I + N)
    x = torch.randn(N, D, generator=g) * 1.5 + 0.2
    wg, wu = torch.randn(E, I, D, generator=g) / D ** 0.5, torch.randn(E, I, D, generator=g) / D ** 0.5
    wd = torch.randn(E, D, I, generator=g) / I ** 0.5
    bg, bu, bd = (torch.randn(E, n, generator=g) * 0.1 if bias else None for n in (I, I, D))
    ids = _ids(N, E, k, g)
    wts = torch.rand(N, k, generator=g) + 0.1
    shared, res = torch.randn(N, D, generator=g), torch.randn(N, D, generator=g)
    z = lambda t, n: torch.zeros(E, n, dtype=torch.float64) if t is None else t.double()
    want, bound = torch.zeros(N, D, dtype=torch.float64), torch.zeros(N, D, dtype=torch.float64)
    mag = shared.double().abs() + res.double().abs()
    for t in range(N):
        for s in range(k):
            e = int(ids[t, s])
            xa = x[t].double().abs()
            G, U = wg[e].double() @ x[t].double() + z(bg, I)[e], wu[e].double() @ x[t].double() + z(bu, I)[e]
            dG = _g(D) * (wg[e].double().abs() @ xa + z(bg, I)[e].abs()) + _ulp(G)
            dU = _g(D) * (wu[e].double().abs() @ xa + z(bu, I)[e].abs()) + _ulp(U)
            S = G * torch.sigmoid(G)
            dS = 1.1 * dG + 8 * 2.0 ** -24 * S.abs()
            h = S * U
            dh = dS * (U.abs() + dU) + S.abs() * dU + 2.0 ** -24 * h.abs()
            y = wd[e].double() @ h + z(bd, D)[e]
            dy = wd[e].double().abs() @ dh + _g(I) * (wd[e].double().abs() @ h.abs() + z(bd, D)[e].abs()) + _ulp(y)
            want[t] += wts[t, s].double() * y
            bound[t] += wts[t, s].double() * dy
            mag[t] += (wts[t, s].double() * y).abs()
    want = want + shared.double() + res.double()
    bound = bound + (k + 2) * 2.0 ** -24 * mag + _ulp(want)
    ex = ops.PackedExperts.pack(wg, wu, wd, DEV, gate_b=bg, up_b=bu, down_b=bd)
    buf, out = _guarded(N, 1, D)
    args = (x.to(DEV), ex, ids.to(DEV), wts.to(DEV))
    ops.switch_glu(*args, out[:, 0], shared=shared.to(DEV), res=res.to(DEV))
    got = out[:, 0].cpu()
    assert _guards_intact(buf, D) and not torch.isnan(got).any()
    ratio = float(((got.double() - want).abs() / bound).max())
    print(f"MOE switch_glu D={D} I={I} E={E} k={k} N={N} bias={bias} ratio={ratio:.3f}")
    assert ratio <= 1.0
    again = torch.full((N, D), float("nan"), device=DEV)
    ops.switch_glu(*args, again, shared=shared.to(DEV), res=res.to(DEV))
    assert torch.equal(again.cpu(), got)
    for t in {0, N - 1}:
        alone = torch.full((1, D), float("nan"), device=DEV)
        ops.switch_glu(x[t:t + 1].to(DEV), ex, ids[t:t + 1].to(DEV), wts[t:t + 1].to(DEV), alone, shared=shared[t:t + 1].to(DEV), res=res[t:t + 1].to(DEV))
        assert torch.equal(alone.cpu()[0], got[t]), t
    # without shared / res: the plain weighted sum
    plain = torch.full((N, D), float("nan"), device=DEV)
    ops.switch_glu(*args, plain)
    assert float(((plain.cpu().double() - (want - shared.double() - res.double())).abs() / bound).max()) <= 1.0


# ------------------------------------------------------------------ router
def _route_ref(logits, k, fn, bias, n_group, topk_group, norm, rsf):
    """group_expert_select in float64 with this library's tie rule (the lower index wins).  -> ids, weights, selection gap (k-th / (k+1)-th), smallest
    gap between consecutive selected scores, group-cut gap."""
    x = logits.double()
    N, E = x.shape
    sc = torch.sigmoid(x) if fn == "sigmoid" else torch.softmax(x, -1)
    sel = sc if bias is None else sc + bias.double()
    gap_g = float("inf")
    nz = n_group - topk_group
    if n_group > 1 and nz > 0:
        grp = sel.view(N, n_group, -1)
        gs = grp.topk(2, -1).values.sum(-1)
        order = n_group - 1 - torch.argsort(gs.flip(-1), dim=-1, stable=True)   # ascending score; of equals the higher index first
        sgs = gs.gather(1, order)
        gap_g = float((sgs[:, nz] - sgs[:, nz - 1]).min())
        mask = torch.zeros(N, n_group, dtype=torch.bool).scatter_(1, order[:, :nz], True)
        sel = torch.where(mask[:, :, None], torch.zeros((), dtype=torch.float64), grp).reshape(N, E)
    order = torch.argsort(sel, dim=-1, descending=True, stable=True)
    ssel = sel.gather(1, order)
    gap = float((ssel[:, k - 1] - ssel[:, k]).min()) if k < E else float("inf")
    gap_in = float((ssel[:, :k - 1] - ssel[:, 1:k]).min()) if k > 1 else float("inf")
    ids = order[:, :k]
    w = sc.gather(1, ids)
    if k > 1 and norm:
        w = w / (w.sum(-1, keepdim=True) + 1e-20)
    return ids, w * rsf, gap, gap_in, gap_g


def _route_inputs(E, fn, bias, seed, N=5):
    """A permuted ladder of logits 0.25 apart (plus jitter), so that the leading scores stay well apart up to E = 512; bias in +-0.02."""
    g = torch.Generator().manual_seed(seed)
    rank = torch.stack([torch.randperm(E, generator=g) for _ in range(N)]).float()
    logits = (3.0 if fn == "sigmoid" else 0.0) - 0.25 * rank + 0.05 * torch.randn(N, E, generator=g)
    return logits, (torch.randn(E, generator=g) * 0.02 if bias else None)


# (E, k, score function, bias, n_group, topk_group, norm_topk_prob, routed_scaling_factor, seed): the seeds were picked on the CPU so that the
# float64 reference's gaps are >= 1e-3 (asserted below; nothing is skipped)
ROUTE_CASES = [
    (4, 1, "softmax", False, 1, 1, False, 1.0, 0), (4, 2, "softmax", True, 1, 1, True, 2.5, 0), (4, 2, "sigmoid", False, 1, 1, True, 1.0, 0),
    (64, 6, "softmax", False, 1, 1, True, 1.0, 0), (64, 6, "sigmoid", True, 4, 2, True, 2.5, 0), (64, 2, "softmax", True, 8, 4, False, 1.0, 0),
    (64, 16, "sigmoid", False, 8, 4, True, 1.0, 1), (64, 1, "sigmoid", True, 4, 1, True, 2.5, 0), (256, 6, "softmax", True, 8, 4, True, 2.5, 0),
    (256, 16, "sigmoid", True, 4, 2, False, 1.0, 2), (256, 2, "sigmoid", False, 1, 1, False, 2.5, 0), (512, 16, "softmax", False, 1, 1, True, 1.0, 14),
    (512, 6, "sigmoid", True, 8, 4, True, 2.5, 0), (512, 1, "softmax", True, 4, 2, False, 1.0, 0), (512, 2, "sigmoid", False, 4, 3, True, 1.0, 0),
    (16, 4, "sigmoid", True, 4, 2, True, 1.0, 0),
]
# weights: float32 against float64.  The exponent's argument (x - max, or -x) is rounded at up to half an ulp of 128 = 2^-17 absolute, which is the
# relative error of the exponential; expf, the sum of E terms in 8 + 6 steps, the divide, the normalising sum and divide and the scale add
# under 40 * 2^-24 more; the normalised weight carries the error of numerator and denominator: 2 * (2^-17 + 40 * 2^-24) < 2^-15.
ROUTE_REL = 2.0 ** -15


def _check_route(ops, logits, bias, k, fn, n_group, topk_group, norm, rsf, want_ids, want_w):
    N = logits.shape[0]
    ids = torch.full((N, k), -7, dtype=torch.int32, device=DEV)
    w = torch.full((N, k), float("nan"), device=DEV)
    kw = dict(expert_bias=None if bias is None else bias.to(DEV), score_function=fn, n_group=n_group, topk_group=topk_group, norm_topk_prob=norm,
              routed_scaling_factor=rsf)
    ops.moe_route(logits.to(DEV), k, ids=ids, weights=w, **kw)
    assert torch.equal(ids.cpu().long(), want_ids)                      # as sets and in order
    err = (w.cpu().double() - want_w).abs() / (ROUTE_REL * want_w.abs() + 2.0 ** -126)
    ids2, w2 = ops.moe_route(logits.to(DEV), k, **kw)
    assert torch.equal(ids2, ids) and torch.equal(w2, w)
    return float(err.max())


@pytest.mark.parametrize("E,k,fn,bias,n_group,topk_group,norm,rsf,seed", ROUTE_CASES)
def test_moe_route(ops, E, k, fn, bias, n_group, topk_group, norm, rsf, seed):
    logits, b = _route_inputs(E, fn, bias, seed)
    want_ids, want_w, gap, gap_in, gap_g = _route_ref(logits, k, fn, b, n_group, topk_group, norm, rsf)
    assert gap >= 1e-3 and gap_g >= 1e-3 and gap_in >= 1e-5, (gap, gap_g, gap_in)
    ratio = _check_route(ops, logits, b, k, fn, n_group, topk_group, norm, rsf, want_ids, want_w)
    print(f"MOE route E={E} k={k} {fn} bias={bias} groups={n_group}/{topk_group} ratio={ratio:.3f}")
    assert ratio <= 1.0


def test_moe_route_exact_ties(ops):
    """Equal scores go to the lower index -- among experts, among groups, and among the experts of zeroed groups whose 0.0 beats a negative biased
    score (the reference zeroes with 0.0, not -inf)."""
    flat = torch.zeros(3, 8)
    ids, w, *_ = _route_ref(flat, 3, "softmax", None, 1, 1, True, 1.0)
    assert ids.tolist() == [[0, 1, 2]] * 3
    assert _check_route(ops, flat, None, 3, "softmax", 1, 1, True, 1.0, ids, w) <= 1.0
    # four equal groups of two, two kept: groups 2 and 3 are zeroed; with bias -2 the kept experts score below the zeroed ones' 0.0
    bias = torch.full((8,), -2.0)
    ids, w, *_ = _route_ref(flat, 3, "sigmoid", bias, 4, 2, False, 1.0)
    assert ids.tolist() == [[4, 5, 6]] * 3
    assert _check_route(ops, flat, bias, 3, "sigmoid", 4, 2, False, 1.0, ids, w) <= 1.0
    # ... and with k = 6 the kept experts follow the four zeroed ones, again in index order
    ids, w, *_ = _route_ref(flat, 6, "sigmoid", bias, 4, 2, True, 2.5)
    assert ids.tolist() == [[4, 5, 6, 7, 0, 1]] * 3
    assert _check_route(ops, flat, bias, 6, "sigmoid", 4, 2, True, 2.5, ids, w) <= 1.0
    # a tie between two experts that are 64 and 65 apart in a 512-wide row
    x = torch.full((2, 512), -4.0)
    x[:, [300, 365, 364]] = 1.0
    ids, w, *_ = _route_ref(x, 2, "sigmoid", None, 1, 1, False, 1.0)
    assert ids.tolist() == [[300, 364]] * 2
    assert _check_route(ops, x, None, 2, "sigmoid", 1, 1, False, 1.0, ids, w) <= 1.0


# ------------------------------------------------------------------ plan
@pytest.mark.parametrize("N,k,E,kind", [(1, 6, 64, "rand"), (65, 6, 64, "rand"), (3, 1, 512, "rand"), (33, 2, 4, "hole"), (70, 1, 4, "one"), (64, 1, 1, "rand")])
def test_moe_plan(ops, N, k, E, kind):
    ids = _ids(N, E, k, torch.Generator().manual_seed(N + E), kind)
    ws = ops.moe_plan(ids.to(DEV), E, 16, 32)
    flat = ids.flatten().long()
    counts = torch.bincount(flat, minlength=E)
    offsets = torch.cat([torch.zeros(1, dtype=torch.long), counts.cumsum(0)])
    perm = torch.sort(flat, stable=True).indices
    tiles = [[e, int(offsets[e]) + j, min(TILE, int(counts[e]) - j), 0] for e in range(E) for j in range(0, int(counts[e]), TILE)]
    assert ws.max_tiles == (N * k + TILE - 1) // TILE + E and len(tiles) <= ws.max_tiles
    assert torch.equal(ws.counts.cpu().long(), counts) and torch.equal(ws.offsets.cpu().long(), offsets)
    assert torch.equal(ws.perm.cpu().long(), perm)
    got = ws.tiles.cpu()
    assert got[:len(tiles)].tolist() == tiles and bool((got[len(tiles):, 2] == 0).all())


# ------------------------------------------------------------------ refusals
def test_moe_refusals(ops):
    from mlx_audio_amd._lib import Mi355Error

    def refused(status, text, fn, *outs):
        before = [o.clone() for o in outs]
        with pytest.raises(Mi355Error, match=rf"\({status}\).*{text}"):
            fn()
        torch.cuda.synchronize()
        assert all(torch.equal(o, b) for o, b in zip(outs, before))

    def route(E, k, **kw):
        ids, w = torch.full((2, k), -7, dtype=torch.int32, device=DEV), torch.full((2, k), SENT, device=DEV)
        refused(kw.pop("status"), kw.pop("text"), lambda: ops.moe_route(torch.zeros(2, E, device=DEV), k, ids=ids, weights=w, **kw), ids, w)

    route(513, 2, status=-3, text="MI355_MOE_MAX_EXPERTS")
    route(4, 5, status=-3, text="k = 5")
    route(64, 17, status=-3, text="MI355_MOE_MAX_TOPK")
    route(64, 2, n_group=6, topk_group=2, status=-1, text="n_group = 6 must divide")
    N, k, E, D, I = 3, 2, 4, 16, 32
    g = torch.Generator().manual_seed(0)
    ex = ops.PackedExperts.pack(torch.randn(E, I, D, generator=g), torch.randn(E, I, D, generator=g), torch.randn(E, D, I, generator=g), DEV)
    ids, wts = _ids(N, E, k, g).to(DEV), torch.ones(N, k, device=DEV)
    out = torch.full((N, D), SENT, device=DEV)
    wide = torch.zeros(N, D + 3, device=DEV)
    refused(-1, "misaligned rows", lambda: ops.switch_glu(wide[:, :D], ex, ids, wts, out), out)          # a row stride of D + 3 floats
    refused(-1, "misaligned rows", lambda: ops.switch_glu(wide[:, 1:D + 1], ex, ids, wts, out), out)     # ... and a base 4 bytes off
    short = ops.MoeWorkspace(N, k, E, D, I, DEV, nbytes=ops.MoeWorkspace(N, k, E, D, I, DEV).nbytes - 16)
    short.buf.fill_(17)
    refused(-1, "workspace of", lambda: ops.moe_plan(ids, E, D, I, ws=short), short.buf)
    refused(-1, "workspace of", lambda: ops.switch_glu(torch.zeros(N, D, device=DEV), ex, ids, wts, out, ws=short), out, short.buf)
