"""Float64 statements of the four MossFormer2 entry points (include/mi355audio.h: mi355_shift_scalenorm, mi355_gau_kv, mi355_gau_attention,
mi355_gated_fsmn), computed on the same float32 inputs the kernels read.  Each ``*64`` function returns the value and, next to it, a per-element
error bound for a float32 kernel, derived from the arithmetic and not from any kernel's output:

* a contraction of ``n`` terms run as one ``fmaf`` chain (what ``v_mfma_f32_32x32x2_f32`` is along k) is within ``n * U * sum |terms|`` of the
  exact sum, ``U = 2^-24``; errors of its operands propagate by the product rule (first order plus the second-order term where it is kept);
* a head element ``rope(qk * gamma + beta)`` is one fmaf, two (rope columns) rounded products and one rounded sum: ``HEAD_ULPS = 4`` units of
  ``U * (|z| |cos| + |z'| |sin|)`` cover them with the table entries' own half-ulp rounding being part of the INPUT (the tables are shared);
* ``sigmoid`` is expf, one add and one divide: ``SIGMOID_ULPS = 4`` units of ``U * sigmoid``, and its slope is at most 1 / 4.

Restated from sts/models/mossformer2_se of the reference: flash_sharea_ffconvm.py:134-156 (token shift), scalenorm.py:35-41, offsetscale.py:40-57,
mossformerblock_gfsmn.py:61-63 (nn.RoPE(dims=32, traditional=False, base=10000)), flash_sharea_ffconvm.py:244-378 with
flash_attention_kernels.py:107-132 (the two attention terms), flash_sharea_ffconvm.py:170-188 (the gate), gated_fsmn.py:105-116 and
unideepfsmn.py:96-123 (the gated memory)."""
import torch

U = 2.0 ** -24
HEAD_ULPS = 4
SIGMOID_ULPS = 4
D = 128
GROUP = 256
ROPE = 32


def _lens(lens, B, T):
    return [T] * B if lens is None else [min(max(int(n), 0), T) for n in lens]


def rope_tables64(rows):
    """What ops.gau_rope_tables rounds to float32."""
    t = torch.arange(rows, dtype=torch.float64)[:, None]
    inv = torch.pow(torch.tensor(10000.0, dtype=torch.float64), -torch.arange(ROPE // 2, dtype=torch.float64) / (ROPE // 2))
    return torch.cos(t * inv), torch.sin(t * inv)


def head64(qk, gamma, beta, cos, sin, h):
    """-> (head h of qk [T, 128] float64, its error bound).  cos / sin: the float32 tables' values, [>= T, 16]."""
    T = qk.shape[0]
    z = qk.double() * gamma[h].double() + beta[h].double()
    c, s = cos[:T].double(), sin[:T].double()
    y = z.clone()
    a, b = z[:, :16], z[:, 16:32]
    y[:, :16] = a * c - b * s
    y[:, 16:32] = b * c + a * s
    mag = z.abs()
    mag[:, :16] = a.abs() * c.abs() + b.abs() * s.abs()
    mag[:, 16:32] = b.abs() * c.abs() + a.abs() * s.abs()
    return y, HEAD_ULPS * U * mag


def shift_scalenorm64(x, g=None, eps=1e-8, shift=True, lens=None):
    """-> (y [B, T, C] float64, bound).  ss is C / 64 fmaf terms per lane (4 per 256 columns) and six butterfly adds of positive numbers:
    relative error (4 ceil(C / 256) + 6) U; the square root halves it; sqrt, * C^-1/2 (itself rounded), the clamp's divide and the last multiply
    add 5 U."""
    B, T, C = x.shape
    xd = x.double()
    s = xd.clone()
    if shift:
        s[:, 1:, :C // 2] = xd[:, :-1, :C // 2]
        s[:, 0, :C // 2] = 0
    for b, n in enumerate(_lens(lens, B, T)):
        s[b, n:] = 0
    gv = 1.0 if g is None else float(g)
    nrm = torch.sqrt((s * s).sum(-1, keepdim=True)) * (C ** -0.5)
    y = s * (gv / torch.clamp(nrm, min=eps))
    rel = (0.5 * (4 * ((C + 255) // 256) + 6) + 5) * U
    return y, rel * y.abs()


def gated_fsmn64(p, xu, xv, res, w, lens=None):
    """-> (y, bound).  The tap chain: K U sum |w p|; (xu + p), + chain: one U each of the partial sums' magnitudes; the closing fmaf: U |y|."""
    B, T, C = p.shape
    K = w.shape[1]
    left = (K - 1) // 2
    pd = p.double().clone()
    ls = _lens(lens, B, T)
    for b, n in enumerate(ls):
        pd[b, n:] = 0
    pad = torch.zeros(B, T + K - 1, C, dtype=torch.float64)
    pad[:, left:left + T] = pd
    wd = w.double()
    acc = torch.zeros(B, T, C, dtype=torch.float64)
    mag = torch.zeros_like(acc)
    for j in range(K):
        term = pad[:, j:j + T] * wd[:, j]
        acc += term
        mag += term.abs()
    m = xu.double() + pd + acc
    y = xv.double() * m + res.double()
    em = U * (K * mag + (xu.double().abs() + pd.abs()) + (xu.double().abs() + pd.abs() + mag))
    bound = xv.double().abs() * em + U * ((xv.double() * m).abs() + res.double().abs())
    for b, n in enumerate(ls):
        y[b, n:] = 0
        bound[b, n:] = 0
    return y, bound


def gau_kv64(qk, vu, gamma, beta, cos, sin, lens=None):
    """-> (kv [B, 128, E], bound): a chain of at most 256 rows per group, the groups added in order, one divide: (n + G + 1) U sum |terms| / n with
    n = lens[b] covers them; the heads' own error rides on |vu|."""
    B, T, E = vu.shape
    kv = torch.zeros(B, D, E, dtype=torch.float64)
    bound = torch.zeros_like(kv)
    for b, n in enumerate(_lens(lens, B, T)):
        if n == 0:
            continue
        lk, elk = head64(qk[b, :n], gamma, beta, cos, sin, 3)
        v = vu[b, :n].double()
        G = (n + GROUP - 1) // GROUP
        kv[b] = lk.T @ v / n
        bound[b] = ((n + G + 1) * U * (lk.abs().T @ v.abs()) + elk.T @ v.abs()) / n
    return kv, bound


def gau_attention64(qk, vu, kv, gamma, beta, cos, sin, lens=None, parts=False):
    """-> (out [B, T, E / 2], bound); kv [B, 128, E] is an INPUT (float32 values).  ``parts=True`` also returns the quadratic and the linear part of A."""
    B, T, E = vu.shape
    H = E // 2
    out = torch.zeros(B, T, H, dtype=torch.float64)
    bound = torch.zeros_like(out)
    quad_all = torch.zeros(B, T, E, dtype=torch.float64)
    lin_all = torch.zeros_like(quad_all)
    for b, n in enumerate(_lens(lens, B, T)):
        if n == 0:
            continue
        q, eq = head64(qk[b, :n], gamma, beta, cos, sin, 0)
        lq, elq = head64(qk[b, :n], gamma, beta, cos, sin, 1)
        k, ek = head64(qk[b, :n], gamma, beta, cos, sin, 2)
        v = vu[b, :n].double()
        kvb = kv[b].double()
        lin = lq @ kvb
        lin_mag = lq.abs() @ kvb.abs()
        e_lin_in = elq @ kvb.abs()
        for g0 in range(0, n, GROUP):
            g1 = min(g0 + GROUP, n)
            nk = g1 - g0
            s = q[g0:g1] @ k[g0:g1].T / GROUP
            es = (D * U * (q[g0:g1].abs() @ k[g0:g1].abs().T) + eq[g0:g1] @ k[g0:g1].abs().T + q[g0:g1].abs() @ ek[g0:g1].T + eq[g0:g1] @ ek[g0:g1].T) / GROUP
            sp = torch.clamp(s, min=0)
            S = sp * sp
            eS = 2 * sp * es + es * es + U * (sp + es) ** 2
            quad = S @ v[g0:g1]
            quad_mag = S @ v[g0:g1].abs()
            A = lin[g0:g1] + quad
            eA = (D + nk) * U * (lin_mag[g0:g1] + quad_mag) + e_lin_in[g0:g1] + eS @ v[g0:g1].abs()
            quad_all[b, g0:g1], lin_all[b, g0:g1] = quad, lin[g0:g1]
            Av, Au, eAv, eAu = A[:, :H], A[:, H:], eA[:, :H], eA[:, H:]
            vv, uu = v[g0:g1, :H], v[g0:g1, H:]
            x = Av * uu
            sg = torch.sigmoid(x)
            e_sg = 0.25 * (eAv * uu.abs() + U * x.abs()) + SIGMOID_ULPS * U * sg
            y1 = Au * vv
            e_y1 = eAu * vv.abs() + U * y1.abs()
            o = y1 * sg
            out[b, g0:g1] = o
            bound[b, g0:g1] = e_y1 * sg + y1.abs() * e_sg + e_y1 * e_sg + U * o.abs()
    if parts:
        return out, bound, quad_all, lin_all
    return out, bound


# ---- float32-valued stand-ins with the signatures of mlx_audio_amd.ops, for host schedules run without a device
def shift_scalenorm(x, y, *, g=None, eps=1e-8, shift=True, lens=None):
    y.copy_(shift_scalenorm64(x, g, eps, shift, lens)[0].float())
    return y


def gated_fsmn(p, xu, xv, res, w, y, *, lens=None):
    y.copy_(gated_fsmn64(p, xu, xv, res, w, lens)[0].float())
    return y


def gau_kv(qk, vu, gamma, beta, rope, *, lens=None, kv=None, ws=None):
    r = gau_kv64(qk, vu, gamma, beta, rope[0], rope[1], lens)[0].float()
    if kv is None:
        return r
    kv.copy_(r)
    return kv


def gau_attention(qk, vu, kv, gamma, beta, rope, out, *, lens=None, causal=False, qk_dim=D, group=GROUP, cols=0):
    assert not causal and qk_dim == D and group == GROUP
    out.copy_(gau_attention64(qk, vu, kv, gamma, beta, rope[0], rope[1], lens)[0].float())
    return out


def gau_rope_tables(rows, device=None):
    c, s = rope_tables64(rows)
    return c.float(), s.float()


def layernorm(x, y, *, weight=None, bias=None, ada_gb=None, res=None, eps=1e-5, lens=None, post_act=0, post_slope=0.0, split=0):
    """mi355_layernorm's plain form: per row, biased variance, optional affine."""
    assert ada_gb is None and res is None and post_act == 0 and split == 0, "not emulated"
    xd = x.double()
    mu = xd.mean(-1, keepdim=True)
    v = (xd - mu) / torch.sqrt(((xd - mu) ** 2).mean(-1, keepdim=True) + eps)
    if weight is not None:
        v = v * weight.double()
    if bias is not None:
        v = v + bias.double()
    y.copy_(v.to(y.dtype))
    return y


def dwconv(x, w, bias, y, *, pad=0, stride=1, transpose=False, lens_in=None, dil=1, pre_alpha=None, pre_inv=None):
    """mi355_dwconv with lens_in: input rows at and beyond lens_in[b] read as zero."""
    import _ops_emu

    if lens_in is not None:
        x = x.clone()
        for b in range(x.shape[0]):
            x[b, int(lens_in[b]):] = 0
    return _ops_emu.dwconv(x, w, bias, y, pad=pad, stride=stride, transpose=transpose, dil=dil, pre_alpha=pre_alpha, pre_inv=pre_inv)


import contextlib  # noqa: E402


@contextlib.contextmanager
def patched():
    """The entry points the MossFormer2 host schedule calls, swapped for their float64 statements (on top of ``_ops_emu`` / ``_ops_emu_gn``)."""
    import _ops_emu_gn
    import _ops_emu_melroformer
    from mlx_audio_amd import ops

    names = dict(shift_scalenorm=shift_scalenorm, gated_fsmn=gated_fsmn, gau_kv=gau_kv, gau_attention=gau_attention, gau_rope_tables=gau_rope_tables,
                 layernorm=layernorm, dwconv=dwconv, head_gate=_ops_emu_melroformer.head_gate)
    saved = {k: getattr(ops, k) for k in names}
    with _ops_emu_gn.patched():
        try:
            for k, v in names.items():
                setattr(ops, k, v)
            yield
        finally:
            for k, v in saved.items():
                setattr(ops, k, v)
