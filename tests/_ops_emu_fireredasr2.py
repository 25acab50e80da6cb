"""float64 statements of the four contracts of ``csrc/firered.hip`` (``include/mi355audio.h``, section FireRedASR2-AED), each with the per-element
float32 rounding bound of the kernel's operation order (U = 2^-24; first order, padded by a few per cent for the second).  Inputs are the float32
arrays the kernel reads.  The second half states the same contracts as stand-ins for ``mlx_audio_amd.ops`` (``patched``), for the CPU suite of the
model's host schedule; the package is imported only there."""
import math

import numpy as np

U = 2.0 ** -24
NEG = -1e10


def sub_out(n):
    return (n - 3) // 2 + 1


# ------------------------------------------------------------------ subsample2d_k3s2
def subsample2d(x, w, bias, lens_in=None, lens_out=None, relu=True, out_cf=False):
    """x [B, T, F] or [B, T, F, Cin], w [Cout, 3, 3, Cin] -> (y, bound).  The kernel: bias, then one fmaf per (kh, kw, ci): at most 9 Cin roundings,
    each at most U times a partial sum that sum |w x| + |bias| dominates."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 3:
        x = x[..., None]
    w = np.asarray(w, dtype=np.float64)
    B, T, F, Cin = x.shape
    Cout = w.shape[0]
    To, Fo = sub_out(T), sub_out(F)
    x = x.copy()
    for b in range(B):
        if lens_in is not None:
            x[b, max(0, min(int(lens_in[b]), T)):] = 0.0
    y = np.zeros((B, To, Fo, Cout))
    mag = np.zeros((B, To, Fo, Cout))
    for kh in range(3):
        for kw in range(3):
            xs = x[:, kh:kh + 2 * To - 1:2, kw:kw + 2 * Fo - 1:2, :]
            y += np.einsum("btfi,oi->btfo", xs, w[:, kh, kw, :])
            mag += np.einsum("btfi,oi->btfo", np.abs(xs), np.abs(w[:, kh, kw, :]))
    if bias is not None:
        y += np.asarray(bias, dtype=np.float64)
        mag += np.abs(np.asarray(bias, dtype=np.float64))
    if relu:
        y = np.maximum(y, 0.0)
    bound = U * (9 * Cin + 1) * mag * 1.01
    for b in range(B):
        if lens_out is not None:
            n = max(0, min(int(lens_out[b]), To))
            y[b, n:] = 0.0
            bound[b, n:] = 0.0
    if out_cf:
        y, bound = y.transpose(0, 1, 3, 2), bound.transpose(0, 1, 3, 2)
    return np.ascontiguousarray(y), np.ascontiguousarray(bound)


# ------------------------------------------------------------------ glu_dwconv_ln_swish
def _sigmoid(v):
    return 1.0 / (1.0 + np.exp(-v))


def glu_dwconv_ln_swish(x, w, ln_w, ln_b, eps, lens=None):
    """x [B, L, 2 C], w [C, K] -> (y, bound) [B, L, C].

    Rounding, in the kernel's order.  g = a / (1 + expf(-b)): expf 2 U, the add, the division and the product one U each: 5 U |g|, taken as 6.
    z: K fmaf in a chain: (6 + K) U sum |w g| =: ez.  The row sums: a thread adds its channels (ceil(C / 256) of them up to 1024 channels,
    ceil(C / 512) above), the DPP wave sum 6 more levels, the join 2 (four waves) or 8 (eight): ns roundings of partial sums below sum |z|.  mean: em = mean(ez) + (ns + 1) U mean |z|.  d = z - mean:
    ed = ez + em + U |d|.  var = mean(d^2) by fmaf: ev = mean(2 |d| ed) + (ns + 2) U var.  r = 1 / sqrt(var + eps): relative
    er = ev / (2 (var + eps)) + 3 U.  n = fma(d r, lw, lb): en = |lw| r (ed + |d| (er + U)) + U |n|.  y = n / (1 + expf(-n)): |dy / dn| <= 1.1,
    plus 6 U |y|."""
    x = np.asarray(x, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    lw, lb = np.asarray(ln_w, dtype=np.float64), np.asarray(ln_b, dtype=np.float64)
    B, L, C2 = x.shape
    C, K = w.shape
    assert C2 == 2 * C
    half = (K - 1) // 2
    y, bound = np.zeros((B, L, C)), np.zeros((B, L, C))
    ns = math.ceil(C / 256) + 8 if C <= 1024 else math.ceil(C / 512) + 14
    for b in range(B):
        n = L if lens is None else max(0, min(int(lens[b]), L))
        if n == 0:
            continue
        g = np.zeros((L + 2 * half, C))
        g[half:half + n] = x[b, :n, :C] * _sigmoid(x[b, :n, C:])
        z, mag = np.zeros((n, C)), np.zeros((n, C))
        for k in range(K):
            z += w[:, k] * g[k:k + n]
            mag += np.abs(w[:, k] * g[k:k + n])
        ez = (6 + K) * U * mag
        mean = z.mean(-1, keepdims=True)
        em = ez.mean(-1, keepdims=True) + (ns + 1) * U * np.abs(z).mean(-1, keepdims=True)
        d = z - mean
        ed = ez + em + U * np.abs(d)
        var = (d * d).mean(-1, keepdims=True)
        ev = (2 * np.abs(d) * ed).mean(-1, keepdims=True) + (ns + 2) * U * var
        r = 1.0 / np.sqrt(var + eps)
        er = ev / (2 * (var + eps)) + 3 * U
        nn = d * r * lw + lb
        en = np.abs(lw) * r * (ed + np.abs(d) * (er + U)) + U * np.abs(nn)
        yy = nn * _sigmoid(nn)
        y[b, :n] = yy
        bound[b, :n] = (1.1 * en + 6 * U * np.abs(yy)) * 1.05
    return y, bound


# ------------------------------------------------------------------ beam_step
def beam_t(logits_row, smoothing, eos_id, eos_penalty):
    """(t [V] float64, bound [V]) of one row.  u = x / s (U |u|), u - M (U |u - M|), expf (2 U): a term's relative error is at most
    U (|u| + |M| + |u - M| + 2) <= U (2 A + D + 2), A = max |u|, D = max - min.  The sum adds ceil(V / 256) terms per thread and 8 joins.  p = e / S one
    more, p + 1e-10 one more, logf 2 U |t|, the eos product one U |t|."""
    u = np.asarray(logits_row, dtype=np.float64) / float(np.float32(smoothing))
    M = u.max()
    e = np.exp(u - M)
    S = e.sum()
    t = np.log(e / S + 1e-10)
    A, D, n = np.abs(u).max(), M - u.min(), math.ceil(len(u) / 256)
    rel = U * ((2 * A + D + 2) * 2 + n + 8 + 2)
    bound = rel + 2 * U * np.abs(t)
    pen = float(np.float32(eos_penalty))
    t[eos_id] *= pen
    bound[eos_id] = bound[eos_id] * abs(pen) + U * abs(t[eos_id])
    return t, bound * 1.01


def _order_key(v, beam, tok, rank):
    return (-v, beam, tok, rank)


def beam_step(logits, scores, finished, step, max_steps, done, tokens, ind, conf, *, eos_id, smoothing, eos_penalty):
    """The contract of ``mi355_beam_step`` on numpy arrays; returns a dict of the new state (copies; the histories are the *_out buffers with the
    untouched entries left as NaN / -7) plus ``margin`` [N]: the smallest relative gap that any decision of the step rested on (ties that are exact
    by construction -- equal inputs, or sums that the float32 rounding of -1e10 + t makes equal -- are resolved by the documented rule and do not
    count).  Decisions are taken on float32-rounded sums, as the kernel's are."""
    logits = np.asarray(logits, dtype=np.float32)
    N, B = scores.shape
    V = logits.shape[1]
    Tmax = tokens.shape[2]
    out = dict(scores=scores.astype(np.float64).copy(), finished=finished.copy(), step=step.copy(), done=done.copy(),
               beam_idx=np.full((N, B), -7, dtype=np.int32), new_tokens=np.full((N, B), -7, dtype=np.int32), new_conf=np.full((N, B), np.nan),
               tokens=np.full((N, B, Tmax), -7, dtype=np.int32), ind=np.full((N, B, Tmax), -7, dtype=np.int32), conf=np.full((N, B, Tmax), np.nan),
               score_bound=np.zeros((N, B)), conf_bound=np.zeros((N, B)), margin=np.full((N,), np.inf))
    for n in range(N):
        if done[n]:
            continue
        st = int(step[n])
        if st < 1 or st >= Tmax:
            out["done"][n] = 1
            continue
        cands = []   # (sum32, beam, token, rank, t, t_bound, sum64)
        margin = np.inf
        for i in range(B):
            if finished[n, i]:
                for r in range(B):
                    t = 0.0 if r == 0 else NEG
                    cands.append((np.float32(np.float32(scores[n, i]) + np.float32(t)), i, eos_id, r, t, 0.0))
                continue
            row = logits[n * B + i]
            t, tb = beam_t(row, smoothing, eos_id, eos_penalty)
            # the kernel's candidates: the B largest logits other than eos (equal logits: the lower id), eos inserted by its t
            ids = [c for c in np.lexsort((np.arange(V), -row.astype(np.float64))) if c != eos_id][:B]
            lst = [(t[c], int(c)) for c in ids]
            pe = next((r for r, (tv, c) in enumerate(lst) if t[eos_id] > tv or (t[eos_id] == tv and eos_id < c)), B)
            lst.insert(pe, (t[eos_id], eos_id))
            for r in range(B):   # t decides only where eos goes (the other entries are ordered by their logits, exactly)
                if pe not in (r, r + 1):
                    continue
                other = lst[r + 1][1] if pe == r else lst[r][1]
                if row[other] == row[eos_id] and float(np.float32(eos_penalty)) == 1.0:
                    continue   # the same logit gives the same t bit for bit: the lower token id, by the rule
                margin = min(margin, (lst[r][0] - lst[r + 1][0]) / (tb[lst[r][1]] + tb[lst[r + 1][1]] + 1e-300))
            for r, (tv, c) in enumerate(lst[:B]):
                cands.append((np.float32(np.float32(scores[n, i]) + np.float32(tv)), i, c, r, tv, tb[c]))
        cands.sort(key=lambda q: _order_key(float(q[0]), q[1], q[2], q[3]))
        for a, b in zip(cands[:B], cands[1:B + 1]):
            s64a, s64b = float(scores[n, a[1]]) + a[4], float(scores[n, b[1]]) + b[4]
            exact = (scores[n, a[1]] == scores[n, b[1]] and a[4] == b[4]) or (a[0] == b[0] and abs(float(a[0])) >= 1e9)
            if not exact:
                margin = min(margin, (s64a - s64b) / (a[5] + b[5] + 2 * U * max(abs(s64a), abs(s64b)) + 1e-300))
        out["margin"][n] = margin
        nfin = 0
        for j, (s32, i, c, r, tv, tb) in enumerate(cands[:B]):
            s64 = float(scores[n, i]) + tv
            out["scores"][n, j] = s64
            out["score_bound"][n, j] = (tb + U * abs(s64)) * 1.01
            out["finished"][n, j] = int(c == eos_id)
            out["beam_idx"][n, j] = i
            out["new_tokens"][n, j] = c
            out["new_conf"][n, j] = math.exp(tv)
            out["conf_bound"][n, j] = math.exp(tv) * (tb + 2 * U) * 1.01 + 1e-45
            out["tokens"][n, j, :st] = tokens[n, i, :st]
            out["tokens"][n, j, st] = c
            out["ind"][n, j, :st] = ind[n, i, :st]
            out["ind"][n, j, st] = j
            out["conf"][n, j, :st] = conf[n, i, :st]
            out["conf"][n, j, st] = math.exp(tv)
            nfin += int(c == eos_id)
        if nfin == B or st + 1 == int(max_steps[n]):
            out["done"][n] = 1
        out["step"][n] = st + 1
    return out


# ------------------------------------------------------------------ beam_attention
def beam_attention(q, k, v, ind, pos, *, beams, heads, dh, scale, Tk=None):
    """q [N B, H dh], k / v [N B, Tcap, H dh], ind [N, B, Tmax], pos [N] -> (out, bound).

    A score is an fmaf chain of dh terms and one product: es = (dh + 1) U scale sum |q k|.  exp(s - m): the argument carries es + em + U |s - m|
    (em: the maximum's own error, at most max es), expf 2 U.  The sum: ceil(nk / 64) terms per lane and 6 butterfly levels.  p = e / S one more.
    out = chain of nk fmaf: nk U sum |p v|."""
    q, k, v = (np.asarray(t, dtype=np.float64) for t in (q, k, v))
    NB, Tcap, _ = k.shape
    Tk = Tcap if Tk is None else Tk
    sc = float(np.float32(scale))
    out, bound = np.zeros_like(q), np.zeros_like(q)
    for nb in range(NB):
        n, j = divmod(nb, beams)
        p = int(pos[n])
        if p < 0:
            continue
        nk = min(p, Tk - 1) + 1
        slots = np.clip(ind[n, j, :nk], 0, beams - 1) + n * beams
        kk, vv = k[slots, np.arange(nk)], v[slots, np.arange(nk)]     # [nk, H dh]
        for h in range(heads):
            sl = slice(h * dh, (h + 1) * dh)
            s = (kk[:, sl] @ q[nb, sl]) * sc
            es = (dh + 1) * U * sc * (np.abs(kk[:, sl]) @ np.abs(q[nb, sl]))
            m = s.max()
            e = np.exp(s - m)
            pr = e / e.sum()
            rel = es + es.max() + U * (np.abs(s - m) + 2)
            rel_p = rel + (rel * pr).sum() + U * (math.ceil(nk / 64) + 6 + 1)
            out[nb, sl] = pr @ vv[:, sl]
            bound[nb, sl] = ((pr * rel_p) @ np.abs(vv[:, sl]) + nk * U * (pr @ np.abs(vv[:, sl]))) * 1.05
    return out, bound


# ------------------------------------------------------------------ the same contracts as stand-ins for ``mlx_audio_amd.ops`` (torch in, torch out)
# What the FireRedASR2 host schedule uses beyond these four comes from the existing emulation modules, imported unchanged and only when ``patched``
# is entered: conv_gemm and the packers (``_ops_emu``), layernorm (``_ops_emu_sortformer``), relpos_attention (``_ops_emu_parakeet``), the
# decoder's gemv (``_ops_emu_moonshine``).  ``flash_attention`` is stated here as the decoder's cross-attention uses it.
def _t_subsample2d_k3s2(x, w, bias, y, *, relu=True, out_cf=False, lens_in=None, lens_out=None):
    li = None if lens_in is None else lens_in.tolist()
    lo = None if lens_out is None else lens_out.tolist()
    val, _ = subsample2d(x.double().numpy(), w.numpy(), None if bias is None else bias.numpy(), li, lo, relu=relu, out_cf=out_cf)
    import torch

    y.copy_(torch.from_numpy(val).to(y.dtype))
    return y


def _t_glu_dwconv_ln_swish(x, w, ln_w, ln_b, y, *, eps=1e-5, lens=None):
    import torch

    val, _ = glu_dwconv_ln_swish(x.double().numpy(), w.numpy(), ln_w.numpy(), ln_b.numpy(), eps, None if lens is None else lens.tolist())
    y.copy_(torch.from_numpy(val).to(y.dtype))
    return y


def _t_beam_step(logits, st, *, eos_id, softmax_smoothing=1.25, eos_penalty=1.0):
    import torch

    n_ = lambda t: t.numpy().copy()
    src, dst = st.cur, 1 - st.cur
    o = beam_step(n_(logits), n_(st.scores), n_(st.finished), n_(st.step), n_(st.max_steps), n_(st.done), n_(st.tokens[src]), n_(st.ind[src]),
                  n_(st.conf[src]).astype(np.float64), eos_id=eos_id, smoothing=softmax_smoothing, eos_penalty=eos_penalty)
    live = torch.from_numpy((n_(st.done) == 0) & (n_(st.step) >= 1) & (n_(st.step) < st.tokens[0].shape[2]))
    for n in torch.nonzero(live).flatten().tolist():
        s = int(st.step[n])
        st.tokens[dst][n, :, :s + 1] = torch.from_numpy(o["tokens"][n, :, :s + 1])
        st.ind[dst][n, :, :s + 1] = torch.from_numpy(o["ind"][n, :, :s + 1])
        st.conf[dst][n, :, :s + 1] = torch.from_numpy(o["conf"][n, :, :s + 1]).float()
        st.scores[n] = torch.from_numpy(o["scores"][n]).float()
        st.beam_idx[n], st.new_tokens[n] = torch.from_numpy(o["beam_idx"][n]), torch.from_numpy(o["new_tokens"][n])
        st.new_conf[n] = torch.from_numpy(o["new_conf"][n]).float()
        st.finished[n] = torch.from_numpy(o["finished"][n])
    st.step.copy_(torch.from_numpy(o["step"]))
    st.done.copy_(torch.from_numpy(o["done"]))
    st.cur = dst
    return st


def _t_beam_attention(q, k, v, ind, pos, out, *, beams, heads, dh, scale=None, Tk=None):
    import torch

    val, _ = beam_attention(q.double().numpy(), k.double().numpy(), v.double().numpy(), ind.numpy(), pos.tolist(), beams=beams, heads=heads, dh=dh,
                            scale=dh ** -0.5 if scale is None else scale, Tk=Tk)
    out.copy_(torch.from_numpy(val).to(out.dtype))
    return out


def _t_flash_attention(q, k, v, out, *, heads, dh, scale=None, lens_k=None, **kw):
    import torch

    assert not kw, kw
    N, Tq, Tk = q.shape[0], q.shape[1], k.shape[1]
    scale = dh ** -0.5 if scale is None else scale
    for b in range(N):
        nk = Tk if lens_k is None else min(max(int(lens_k[b]), 0), Tk)
        q4 = q[b, :, :heads * dh].double().reshape(Tq, heads, dh).transpose(0, 1)
        k4, v4 = (t[b, :nk, :heads * dh].double().reshape(nk, heads, dh).transpose(0, 1) for t in (k, v))
        p = torch.softmax(q4 @ k4.transpose(1, 2) * scale, -1)
        out[b, :, :heads * dh] = (p @ v4).transpose(0, 1).reshape(Tq, heads * dh).to(out.dtype)
    return out


def patched():
    import contextlib

    import _ops_emu_moonshine
    import _ops_emu_sensevoice
    from mlx_audio_amd import ops

    @contextlib.contextmanager
    def cm():
        names = dict(subsample2d_k3s2=_t_subsample2d_k3s2, glu_dwconv_ln_swish=_t_glu_dwconv_ln_swish, beam_step=_t_beam_step,
                     beam_attention=_t_beam_attention, flash_attention=_t_flash_attention, gemv=_ops_emu_moonshine.gemv)
        saved = {k: getattr(ops, k) for k in names}
        with _ops_emu_sensevoice.patched():
            try:
                for k, v in names.items():
                    setattr(ops, k, v)
                yield
            finally:
                for k, v in saved.items():
                    setattr(ops, k, v)

    return cm()
