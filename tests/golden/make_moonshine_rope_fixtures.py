#!/usr/bin/env python
"""Runs the reference's OWN ``MoonshineRotaryEmbedding`` and ``apply_rotary_pos_emb`` (``stt/models/moonshine/moonshine.py``, unmodified and imported
from where it lies) over the numpy stand-in for MLX (``mlx_shim.py``, left as it is) and stores what they compute in
``tests/golden/ref_moonshine_rope.npz``:

  * the float32 cos / sin tables at ``rotary_ndims`` 32 (heads of 36) and 46 (heads of 52) for the positions ``ROWS`` (0 .. 8, the last position of
    ``max_position_embeddings`` = 512 and the first past it, and 1249 = the last frame of 30 s of audio) -- the first ``rot / 2`` columns, which is all
    ``apply_rotary_pos_emb`` reads of them;
  * ``apply_rotary_pos_emb`` on seeded q [1, 4, 6, dh] / k [1, 2, 6, dh] at positions 7 .. 12, for (dh, rot) = (36, 32) and (52, 46).

``moonshine.py`` imports ``mlx_audio.stt.utils`` lazily only; the empty stand-in module of the other STT makers is installed all the same.
Only runs where the reference lies: ``python tests/golden/make_moonshine_rope_fixtures.py``."""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_reference_fixtures as M  # noqa: E402  (installs the stand-in)

mx, _np = M.mx, M._np

ROWS = [0, 1, 2, 3, 4, 5, 6, 7, 8, 511, 512, 1249]
CASES = [(36, 32), (52, 46)]
POS0, L, HQ, HK = 7, 6, 4, 2


def load_reference():
    M.import_reference()
    for pkg, path in (("mlx_audio.stt", "stt"), ("mlx_audio.stt.models", "stt/models"), ("mlx_audio.stt.models.moonshine", "stt/models/moonshine")):
        if pkg not in sys.modules:
            M._pkg(pkg, f"{M.REF}/{path}")
    if "mlx_audio.stt.utils" not in sys.modules:
        mod = types.ModuleType("mlx_audio.stt.utils")
        mod.load_audio = None
        sys.modules["mlx_audio.stt.utils"] = mod
    M._load("mlx_audio.stt.models.base", f"{M.REF}/stt/models/base.py")
    M._load("mlx_audio.stt.models.moonshine.config", f"{M.REF}/stt/models/moonshine/config.py")
    return M._load("mlx_audio.stt.models.moonshine.moonshine", f"{M.REF}/stt/models/moonshine/moonshine.py")


def main():
    S = load_reference()
    out = dict(rows=np.array(ROWS, dtype=np.int32))
    for dh, rot in CASES:
        assert rot == int(dh * 0.9) - int(dh * 0.9) % 2   # MoonshineAttention's rotary_ndims at partial_rotary_factor 0.9
        emb = S.MoonshineRotaryEmbedding(rot, max_position_embeddings=512, base=10000.0)
        cos, sin = emb(None, mx.array(np.array([ROWS], dtype=np.int32)))
        cos, sin = _np(cos)[0], _np(sin)[0]
        assert cos.dtype == np.float32 and cos.shape == (len(ROWS), rot) and np.array_equal(cos[:, :rot // 2], cos[:, rot // 2:])
        out[f"cos{rot}"], out[f"sin{rot}"] = cos[:, :rot // 2].copy(), sin[:, :rot // 2].copy()
        rng = np.random.default_rng(100 * dh + rot)
        q = rng.standard_normal((1, HQ, L, dh)).astype(np.float32)
        k = rng.standard_normal((1, HK, L, dh)).astype(np.float32)
        c, s = emb(None, mx.array(np.arange(POS0, POS0 + L, dtype=np.int32)[None, :]))
        qe, ke = S.apply_rotary_pos_emb(mx.array(q), mx.array(k), c, s)
        qe, ke = _np(qe), _np(ke)
        assert qe.dtype == np.float32 and qe.shape == q.shape and ke.shape == k.shape
        assert np.array_equal(qe[..., rot:], q[..., rot:]) and not np.array_equal(qe[..., :rot], q[..., :rot])
        # channels-last [L, heads * dh], the layout the kernel takes
        out[f"q{dh}"], out[f"k{dh}"] = q[0].transpose(1, 0, 2).reshape(L, HQ * dh), k[0].transpose(1, 0, 2).reshape(L, HK * dh)
        out[f"qe{dh}"], out[f"ke{dh}"] = qe[0].transpose(1, 0, 2).reshape(L, HQ * dh), ke[0].transpose(1, 0, 2).reshape(L, HK * dh)
    path = os.path.join(HERE, "ref_moonshine_rope.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= 100_000


if __name__ == "__main__":
    main()
