"""The host side of ``csrc/mid_attn.hip``: the two entry points are declared, exported and refuse by name without a launch (every refusal is decided
before the launch, so none of them needs a device), the ctypes structs have the C layout, the ABI is still 37, and the rotary tables are the bits the
reference's own ``MoonshineRotaryEmbedding`` computes (``tests/golden/make_moonshine_rope_fixtures.py``)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mi355audio.h")
FUNCS = ["mi355_mid_attention", "mi355_partial_rope"]
STRUCTS = ["mi355_mid_attention_args", "mi355_partial_rope_args"]
P = 4096   # a non-null, 16-byte aligned "pointer": a refused call never reads it


def test_entry_points_declared_exported_and_refuse_null():
    from mlx_audio_amd import _lib

    lib = _lib.load()
    assert lib.mi355_abi_version() == 37 == _lib.ABI_VERSION   # two additive entry points: no layout changed, no bump
    for f, s in zip(FUNCS, STRUCTS):
        assert f in _lib.declared_functions() and hasattr(lib, f), f
        st = _lib.STRUCTS[s]()
        assert getattr(lib, f)(ctypes.byref(st), None) == -1 and b"null tensor" in lib.mi355_last_error(), f
        assert getattr(lib, f)(None, None) == -1


def test_struct_layouts_match_c(tmp_path):
    from mlx_audio_amd import _lib

    src = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){"]
    for name in STRUCTS:
        src.append(f'printf("{name} %zu\\n", sizeof({name}));')
        for f, _ in _lib._STRUCT_DECLS[name]:
            src.append(f'printf("{name}.{f} %zu\\n", offsetof({name}, {f}));')
    src.append("return 0;}")
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", str(c), "-o", str(exe)], check=True)
    want = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.strip().splitlines())
    for name in STRUCTS:
        st = _lib.STRUCTS[name]
        assert ctypes.sizeof(st) == int(want[name]), name
        for f, _ in _lib._STRUCT_DECLS[name]:
            assert getattr(st, f).offset == int(want[f"{name}.{f}"]), (name, f)


def _refused(fn, struct, match, **kw):
    from mlx_audio_amd import _lib

    lib = _lib.load()
    st = _lib.STRUCTS[struct](**kw)
    assert getattr(lib, fn)(ctypes.byref(st), None) == -1, (match, kw)
    msg = lib.mi355_last_error().decode()
    assert match in msg, (match, msg)


def test_mid_attention_refusals_by_name():
    ok = dict(q=P, k=P, v=P, out=P, q_bstride=7200, k_bstride=7200, v_bstride=7200, out_bstride=7200, ldq=72, ldk=72, ldv=72, ldo=72, B=1, Tq=100, Tk=100,
              heads=2, kv_heads=2, dh=36, scale=1.0)
    call = lambda match, **kw: _refused("mi355_mid_attention", "mi355_mid_attention_args", match, **{**ok, **kw})
    for dh in (0, 8, 24, 32, 38, 62, 64, 128):   # narrow_attention's and flash_attention's widths stay theirs
        call(f"dh must be 36, 40, 44, 48, 52, 56 or 60 (got dh = {dh})", dh=dh)
    call("Tq and Tk must be at least 1", Tq=0)
    call("Tq and Tk must be at least 1", Tk=0)
    call("bad shape", B=0)
    call("bad shape", kv_heads=0)
    call("heads (3) must be a multiple of kv_heads (2)", heads=3, ldq=108, ldo=108)
    call("a row stride is smaller than heads * dh", ldq=68)
    call("a row stride is smaller than heads * dh", ldo=68)
    call("a row stride is smaller than heads * dh", ldk=68)
    call("a row stride is smaller than heads * dh", kv_heads=1, ldv=32)
    call("rows must be 16-byte aligned", ldk=74)
    call("rows must be 16-byte aligned", out_bstride=7202)
    call("rows must be 16-byte aligned", q=P + 4)
    call("rows must be 16-byte aligned", v=P + 8)
    for name in ("q", "k", "v", "out"):
        call("null tensor", **{name: None})


def test_partial_rope_refusals_by_name():
    ok = dict(x=P, y=P, cos_table=P, sin_table=P, x_bstride=720, y_bstride=720, ldx=144, ldy=144, heads=4, dh=36, rot=32, B=2, L=5, pos0=0, rope_rows=5)
    call = lambda match, **kw: _refused("mi355_partial_rope", "mi355_partial_rope_args", match, **{**ok, **kw})
    call("dh must be a positive multiple of 4 (got dh = 38)", dh=38)
    call("dh must be a positive multiple of 4 (got dh = 0)", dh=0)
    for rot in (0, 1, 31, 38):
        call(f"rot must be even and in [2, dh = 36] (got rot = {rot})", rot=rot)
    call("positions 1..5 run past the 5-row rotary tables", pos0=1)
    call("positions 0..5 run past the 5-row rotary tables", L=6)
    call("positions -1..3 run past the 5-row rotary tables", pos0=-1)
    call("bad shape", L=0)
    call("a row stride is smaller than heads * dh", ldy=140)
    call("rows must be 8-byte aligned", ldx=145)
    call("rows must be 8-byte aligned", y=P + 4)
    call("the second operand needs y2 and heads2", x2=P, ldx2=72, heads2=2)
    call("a row stride is smaller than heads2 * dh", x2=P, y2=P, ldx2=72, ldy2=68, heads2=2)
    call("rows must be 8-byte aligned", x2=P + 4, y2=P, ldx2=72, ldy2=72, heads2=2)
    for name in ("x", "y", "cos_table", "sin_table"):
        call("null tensor", **{name: None})


def test_widths_are_disjoint_from_the_other_attention_kernels():
    from mlx_audio_amd import ops

    assert ops.MID_ATTENTION_WIDTHS == (36, 40, 44, 48, 52, 56, 60) and ops.MID_ATTENTION_FEW_TQ == 4
    assert not set(ops.MID_ATTENTION_WIDTHS) & (set(ops.NARROW_ATTENTION_WIDTHS) | {64, 128})
    assert "mid_attn.hip" in __import__("mlx_audio_amd.build", fromlist=["SOURCES"]).SOURCES


def test_rope_tables_are_the_reference_bits():
    """``ops.moonshine_rope_tables`` against the tables the reference's MoonshineRotaryEmbedding computed (float32: inv_freq, position * inv_freq,
    cos / sin), bit for bit, past ``max_position_embeddings`` too; a table that starts at ``pos0`` is the slice of the one that starts at 0."""
    from mlx_audio_amd import ops

    z = np.load(os.path.join(ROOT, "tests", "golden", "ref_moonshine_rope.npz"))
    rows = z["rows"]
    assert rows.max() == 1249 and 512 in rows
    for rot in (32, 46):
        cos, sin = ops.moonshine_rope_tables(rot, 1250)
        assert cos.dtype == sin.dtype == torch.float32 and cos.shape == sin.shape == (1250, rot // 2) and cos.is_contiguous()
        assert np.array_equal(cos.numpy()[rows], z[f"cos{rot}"]) and np.array_equal(sin.numpy()[rows], z[f"sin{rot}"])
        c7, s7 = ops.moonshine_rope_tables(rot, 6, pos0=7)
        assert torch.equal(c7, cos[7:13]) and torch.equal(s7, sin[7:13])
    with pytest.raises(AssertionError):
        ops.moonshine_rope_tables(31, 4)


def test_reference_rotation_is_the_interleaved_pair_formula():
    """The stored run of the reference's apply_rotary_pos_emb equals the pair formula the kernel is written from, op for op in float32:
    (x[2i] c_i - x[2i+1] s_i, x[2i+1] c_i + x[2i] s_i) on the first rot channels of every head, the rest copied."""
    from mlx_audio_amd import ops

    z = np.load(os.path.join(ROOT, "tests", "golden", "ref_moonshine_rope.npz"))
    for dh, rot in ((36, 32), (52, 46)):
        for name, heads in (("q", 4), ("k", 2)):
            x, want = z[f"{name}{dh}"], z[f"{name}e{dh}"]
            L = x.shape[0]
            cos, sin = (t.numpy() for t in ops.moonshine_rope_tables(rot, L, pos0=7))
            x4 = x.reshape(L, heads, dh)
            got = x4.copy()
            c, s = cos[:, None, :], sin[:, None, :]
            x0, x1 = x4[..., 0:rot:2], x4[..., 1:rot:2]
            got[..., 0:rot:2] = x0 * c - x1 * s
            got[..., 1:rot:2] = x1 * c + x0 * s
            assert got.dtype == np.float32 and np.array_equal(got.reshape(L, heads * dh), want), (dh, name)
