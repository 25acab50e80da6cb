"""numpy restatement of Whisper's word-timing arithmetic, written from the algorithm (reference ``stt/models/whisper/timing.py``), for the tests.

``dtype`` selects the arithmetic: ``np.float32`` is the reference's, ``np.float64`` the yardstick the float32 results are measured against.
The DTW is always float32 (one add per cell, the reference's comparison chain); it is vectorised along anti-diagonals, which changes no
cell's operands: a cell on diagonal s depends on diagonals s - 1 and s - 2 only.
"""
import string

import numpy as np

TOKENS_PER_SECOND = 50


def qk_softmax(q, k, scale, qk_scale=1.0, dtype=np.float32):
    """q [T, dh], k [F, dh] -> softmax over F of qk_scale * scale * q k^T."""
    q, k = np.asarray(q, dtype), np.asarray(k, dtype)
    s = (q @ k.T) * dtype(scale) * dtype(qk_scale)
    s = s - s.max(axis=-1, keepdims=True)
    e = np.exp(s)
    return (e / e.sum(axis=-1, keepdims=True)).astype(dtype)


def standardise(w, dtype=np.float32):
    """w [A, T, F]: (w - mean) / std over the tokens (population standard deviation)."""
    w = np.asarray(w, dtype)
    mean = w.mean(axis=-2, keepdims=True, dtype=dtype)
    std = np.sqrt(((w - mean) ** 2).mean(axis=-2, keepdims=True, dtype=dtype))
    return ((w - mean) / std).astype(dtype)


def median_filter(x, width):
    """Median of odd ``width`` along the last axis with reflect padding; rows no longer than width // 2 pass unchanged.  Exact selection: dtype kept."""
    x = np.asarray(x)
    pad = width // 2
    if x.shape[-1] <= pad:
        return x
    assert width > 0 and width % 2 == 1
    xp = np.pad(x, [(0, 0)] * (x.ndim - 1) + [(pad, pad)], mode="reflect")
    win = np.lib.stride_tricks.sliding_window_view(xp, width, axis=-1)
    return np.sort(win, axis=-1)[..., pad].astype(x.dtype)


def align_matrix(w, width=7, row_begin=0, row_trim=1, dtype=np.float32, negate=True):
    """w [A, T, F] probabilities -> the (negated) [N, F] matrix handed to dtw: standardise, median filter, mean over heads, rows kept."""
    z = median_filter(standardise(w, dtype), width)
    m = z.mean(axis=0, dtype=dtype)
    m = m[row_begin:m.shape[0] - row_trim]
    return (-m if negate else m).astype(dtype)


def dtw(x):
    """x [N, M] float32 -> int array [2, L]: the warping path, forward order."""
    x = np.asarray(x, np.float32)
    N, M = x.shape
    cost = np.full((N + 1, M + 1), np.inf, np.float32)
    trace = np.full((N + 1, M + 1), -1, np.int8)
    cost[0, 0] = 0
    for s in range(N + M - 1):     # cells (i, j), 1-based, with (i - 1) + (j - 1) = s
        i = np.arange(max(1, s + 2 - M), min(N, s + 1) + 1)
        j = s + 2 - i
        c0, c1, c2 = cost[i - 1, j - 1], cost[i - 1, j], cost[i, j - 1]
        t = np.where((c0 < c1) & (c0 < c2), 0, np.where((c1 < c0) & (c1 < c2), 1, 2)).astype(np.int8)
        c = np.where(t == 0, c0, np.where(t == 1, c1, c2))
        cost[i, j] = x[i - 1, j - 1] + c
        trace[i, j] = t
    trace[0, :] = 2
    trace[:, 0] = 1
    i, j = N, M
    path = []
    while i > 0 or j > 0:
        path.append((i - 1, j - 1))
        t = trace[i, j]
        if t == 0:
            i, j = i - 1, j - 1
        elif t == 1:
            i -= 1
        else:
            j -= 1
    return np.array(path[::-1], dtype=np.int64).T.reshape(2, -1)


def dtw_scalar(x):
    """The same DP cell by cell in the reference's loop order (columns outside, rows inside); pins the anti-diagonal version on small inputs."""
    x = np.asarray(x, np.float32)
    N, M = x.shape
    cost = np.full((N + 1, M + 1), np.inf, np.float32)
    trace = np.full((N + 1, M + 1), -1, np.int8)
    cost[0, 0] = 0
    for j in range(1, M + 1):
        for i in range(1, N + 1):
            c0, c1, c2 = cost[i - 1, j - 1], cost[i - 1, j], cost[i, j - 1]
            if c0 < c1 and c0 < c2:
                c, t = c0, 0
            elif c1 < c0 and c1 < c2:
                c, t = c1, 1
            else:
                c, t = c2, 2
            cost[i, j] = x[i - 1, j - 1] + c
            trace[i, j] = t
    trace[0, :] = 2
    trace[:, 0] = 1
    i, j = N, M
    path = []
    while i > 0 or j > 0:
        path.append((i - 1, j - 1))
        if trace[i, j] == 0:
            i, j = i - 1, j - 1
        elif trace[i, j] == 1:
            i -= 1
        else:
            j -= 1
    return np.array(path[::-1], dtype=np.int64).T.reshape(2, -1)


def path_cost(x, path):
    """Sum of x along a path, float64."""
    return float(np.asarray(x, np.float64)[path[0], path[1]].sum())


def softmax_prob_rows(logits, tokens, V, dtype=np.float64):
    lg = np.asarray(logits, dtype)[:, :V]
    e = np.exp(lg - lg.max(axis=-1, keepdims=True))
    p = e / e.sum(axis=-1, keepdims=True)
    return p[np.arange(len(tokens)), np.asarray(tokens)]


# ------------------------------------------------------------------------------------------------ host word logic
def split_on_unicode(decode, tokens):
    full = decode(tokens)
    words, groups, cur, off = [], [], [], 0
    for t in tokens:
        cur.append(t)
        d = decode(cur)
        if "\ufffd" not in d or full[off + d.index("\ufffd")] == "\ufffd":
            words.append(d)
            groups.append(cur)
            cur = []
            off += len(d)
    return words, groups


def split_on_spaces(decode, tokens, eot):
    sub, subt = split_on_unicode(decode, tokens)
    words, groups = [], []
    for s, g in zip(sub, subt):
        if g[0] >= eot or s.startswith(" ") or s.strip() in string.punctuation or not words:
            words.append(s)
            groups.append(list(g))
        else:
            words[-1] += s
            groups[-1].extend(g)
    return words, groups


def words_from_path(words, groups, path, probs):
    """(word, tokens, start, end, probability) per word but the trailing eot group; [] when the eot group is the only one."""
    if len(groups) <= 1:
        return []
    bounds = np.concatenate([[0], np.cumsum([len(g) for g in groups[:-1]])]).astype(int)
    text_idx, time_idx = path
    jumps = np.concatenate([[1], np.diff(text_idx)]).astype(bool)
    jt = time_idx[jumps] / TOKENS_PER_SECOND
    return [(w, list(g), float(jt[a]), float(jt[b]), float(np.mean(probs[a:b])))
            for w, g, a, b in zip(words, groups, bounds[:-1], bounds[1:])]


# ------------------------------------------------------------------------------------------------ toy vocabulary and scripted alignment
class ToyCodec:
    """A scripted vocabulary over the fixture's table {id: bytes as hex}: ``decode`` joins the pieces' bytes and decodes them as UTF-8 with replacement
    characters (so a multi-byte character split over two ids behaves like a byte-level BPE's); ids from the end-of-text id up render as ``<|id|>``."""

    def __init__(self, table, eot=50257):
        self.table = {int(k): bytes.fromhex(v) for k, v in table.items()}
        self.eot = eot

    def decode(self, tokens, skip_special_tokens=False):
        out, run = [], b""
        for t in tokens:
            t = int(t)
            if t >= self.eot:
                out.append(run.decode("utf-8", errors="replace"))
                run = b""
                if not skip_special_tokens:
                    out.append(f"<|{t}|>")
            else:
                run += self.table.get(t) or (" t%d" % t).encode()   # ids outside the table (a free-running decode): a word of their own
        out.append(run.decode("utf-8", errors="replace"))
        return "".join(out)

    def encode(self, text, add_special_tokens=False):
        data, ids = text.encode("utf-8"), []
        by_len = sorted(self.table.items(), key=lambda kv: -len(kv[1]))
        while data:
            t, b = next((t, b) for t, b in by_len if data.startswith(b))
            ids.append(t)
            data = data[len(b):]
        return ids


def toy_table():
    """ids for " wNN" words, word-internal pieces, punctuation, and the two halves of one three-byte character."""
    t = {300 + i: (" w%02d" % i).encode() for i in range(24)}
    t.update({400: b"ab", 401: b"ing", 402: b"s", 403: b"cd"})
    t.update({500: b",", 501: b".", 502: b" (", 503: b")", 504: b"?", 505: b" -", 506: b'"', 507: b" \""})
    full = "\u8a9e".encode("utf-8")
    t.update({600: full[:2], 601: full[2:], 602: b" " + "\u65e5".encode("utf-8")})
    return {str(k): v.hex() for k, v in t.items()}


def scripted_alignment(tokenizer, text_tokens, spec, make):
    """The stand-in for find_alignment in the host-logic fixtures: the tokenizer's own word split of ``text_tokens`` with the (start, end, probability)
    triples of ``spec`` attached in order; ``make(word, tokens, start, end, probability)`` builds the record."""
    if len(text_tokens) == 0:
        return []
    words, groups = tokenizer.split_to_word_tokens(list(text_tokens) + [tokenizer.eot])
    assert len(words) - 1 == len(spec), (words, spec)
    return [make(w, list(g), float(s), float(e), float(p)) for w, g, (s, e, p) in zip(words[:-1], groups[:-1], spec)]
