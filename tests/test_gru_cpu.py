"""``mi355_gru_seq`` without a GPU: the float64 restatement ``tests/_gru_ref.py`` held to two witnesses (``torch.nn.GRU`` with its full ``bias_hh``
against the folded-bias form), the 16-bit weight image of ``ops.pack_gru_wh``, and the new C entry point: declared, exported, refusing nulls and bad
arguments before any launch, its args struct laid out as gcc lays it out."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
HEADER = os.path.join(os.path.dirname(HERE), "include", "mi355audio.h")

import _gru_ref as R  # noqa: E402

FUNC, STRUCT = "mi355_gru_seq", "mi355_gru_seq_args"


@pytest.mark.parametrize("H,In,T", [(64, 48, 9), (256, 64, 5)])
def test_ref_matches_torch_gru_with_folded_bias(H, In, T):
    """torch.nn.GRU adds bias_hh to all three gates; the contract keeps only its n part as ``bhn`` and takes the r / z parts inside ``xproj``'s bias,
    as the reference's loader folds them (sts/models/deepfilternet/weight_loader.py:174-196).  Same function, to float64 rounding."""
    torch.manual_seed(H)
    gru = torch.nn.GRU(In, H, batch_first=True).double()
    x = torch.randn(3, T, In, dtype=torch.float64)
    h0 = torch.rand(1, 3, H, dtype=torch.float64) - 0.5
    with torch.no_grad():
        want, want_h = gru(x, h0)
        b = gru.bias_ih_l0 + torch.cat([gru.bias_hh_l0[:2 * H], torch.zeros(H, dtype=torch.float64)])
        xproj = x @ gru.weight_ih_l0.T + b
    got, got_h = R.gru_seq(xproj.numpy(), gru.weight_hh_l0.detach().numpy(), gru.bias_hh_l0[2 * H:].detach().numpy(), h0[0].numpy())
    assert np.abs(got - want.numpy()).max() < 1e-13 and np.abs(got_h - want_h[0].numpy()).max() < 1e-13
    lens = [T, 1, 0]
    got, got_h = R.gru_seq(xproj.numpy(), gru.weight_hh_l0.detach().numpy(), gru.bias_hh_l0[2 * H:].detach().numpy(), h0[0].numpy(), lens)
    assert np.array_equal(got[0], R.gru_seq(xproj.numpy(), gru.weight_hh_l0.detach().numpy(), gru.bias_hh_l0[2 * H:].detach().numpy(), h0[0].numpy())[0][0])
    assert np.abs(got[1, 0] - want.numpy()[1, 0]).max() < 1e-13 and not got[1, 1:].any() and not got[2].any()
    assert np.array_equal(got_h[1], got[1, 0]) and np.array_equal(got_h[2], h0[0, 2].numpy())


def test_weight_image_layout_scale_and_rounding():
    from mlx_audio_amd import ops

    H = 64
    _, wh, _, _ = R.make_case(H, 1, 1, seed=3)
    wr, k = ops.round_gru_wh(torch.from_numpy(wh))
    amax = float(np.abs(wh).max())
    assert 16384.0 < amax * 2.0 ** k <= 32768.0
    assert float((wr - torch.from_numpy(wh)).abs().max()) <= 2.0 ** -11 * amax and not torch.equal(wr, torch.from_numpy(wh))
    img = ops.pack_gru_wh(torch.from_numpy(wh), "cpu")
    assert img.h == H and img.scale == 2.0 ** -k and img.w.dtype == torch.int16 and img.w.shape == (3 * H * H,)
    vals = img.w.view(torch.float16).float().view(H // 8, 3 * H, 8) * img.scale   # group (kg, row) = Wh[row, 8 kg .. 8 kg + 8)
    assert torch.equal(vals.permute(1, 0, 2).reshape(3 * H, H), wr)
    # fp16-representable checkpoints (what the seeded checkpoints of this package hold) and bf16 ones are held exactly
    w16 = torch.from_numpy(wh).half().float()
    assert torch.equal(ops.round_gru_wh(w16)[0], w16)
    wb = torch.from_numpy(wh).bfloat16().float()
    wb = torch.where(wb.abs() < amax * 2.0 ** -14, torch.zeros_like(wb), wb)
    assert torch.equal(ops.round_gru_wh(wb)[0], wb)
    assert ops.round_gru_wh(torch.zeros(3 * H, H))[1] == 0 and ops.pack_gru_wh(torch.zeros(3 * H, H), "cpu").scale == 1.0
    with pytest.raises(ValueError, match="non-finite"):
        ops.round_gru_wh(torch.full((3 * H, H), math.inf))
    assert ops.GRU_SEQ_HIDDEN == (64, 128, 256)


def test_entry_point_declared_exported_and_refuses_bad_arguments():
    from mlx_audio_amd import _lib

    lib = _lib.load()
    assert lib.mi355_abi_version() == 37 == _lib.ABI_VERSION   # an additive entry point: no layout changed, no bump
    assert FUNC in _lib.declared_functions() and hasattr(lib, FUNC)
    fn = getattr(lib, FUNC)
    assert fn(None, None) == -1
    assert fn(ctypes.byref(_lib.STRUCTS[STRUCT]()), None) == -1 and b"null tensor" in lib.mi355_last_error()
    buf = (ctypes.c_float * 64)()   # host memory: every case below must be refused before a launch could touch it
    p = ctypes.addressof(buf)

    def args(**kw):
        base = dict(xproj=p, xproj_bstride=3 * 64, ld_xproj=3 * 64, wh=p, wh_scale=1.0, bhn=p, B=1, T=1, H=64, out=p, out_bstride=64, ld_out=64)
        base.update(kw)
        return ctypes.byref(_lib.STRUCTS[STRUCT](**base))

    for H in (96, 32, 512, 8):
        assert fn(args(H=H, ld_xproj=3 * H, xproj_bstride=3 * H, ld_out=H, out_bstride=H), None) == -3, H
        assert f"unsupported hidden size {H}".encode() in lib.mi355_last_error()
    assert fn(args(ld_xproj=3 * 64 - 1), None) == -1 and b"strides" in lib.mi355_last_error()
    assert fn(args(ld_out=63), None) == -1 and b"strides" in lib.mi355_last_error()
    assert fn(args(T=2), None) == -1 and b"strides" in lib.mi355_last_error()
    assert fn(args(B=0), None) == -1 and b"bad shape" in lib.mi355_last_error()
    assert fn(args(T=0), None) == -1 and b"bad shape" in lib.mi355_last_error()
    assert fn(args(wh=p + 2), None) == -1 and b"aligned" in lib.mi355_last_error()
    assert fn(args(wh_scale=-1.0), None) == -1 and b"wh_scale" in lib.mi355_last_error()


def test_struct_layout_matches_c(tmp_path):
    from mlx_audio_amd import _lib

    src = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){", f'printf("{STRUCT} %zu\\n", sizeof({STRUCT}));']
    for f, _ in _lib._STRUCT_DECLS[STRUCT]:
        src.append(f'printf("{STRUCT}.{f} %zu\\n", offsetof({STRUCT}, {f}));')
    src.append("return 0;}")
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", str(c), "-o", str(exe)], check=True)
    want = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.strip().splitlines())
    st = _lib.STRUCTS[STRUCT]
    assert ctypes.sizeof(st) == int(want[STRUCT])
    for f, _ in _lib._STRUCT_DECLS[STRUCT]:
        assert getattr(st, f).offset == int(want[f"{STRUCT}.{f}"]), f
    assert [f for f, _ in _lib._STRUCT_DECLS[STRUCT]] == ["xproj", "xproj_bstride", "ld_xproj", "wh", "wh_scale", "bhn", "h0", "lens", "B", "T", "H",
                                                         "out", "out_bstride", "ld_out", "hT"]


def test_wrapper_checks_shapes_before_the_call():
    from mlx_audio_amd import ops

    H = 64
    img = ops.pack_gru_wh(torch.zeros(3 * H, H), "cpu")
    with pytest.raises(AssertionError):
        ops.gru_seq(torch.zeros(1, 2, 3 * H + 1), img, torch.zeros(H), torch.zeros(1, 2, H))
    with pytest.raises(AssertionError):
        ops.gru_seq(torch.zeros(1, 2, 3 * H), img, torch.zeros(H + 1), torch.zeros(1, 2, H))
    with pytest.raises(AssertionError):
        ops.gru_seq(torch.zeros(1, 2, 3 * H), img, torch.zeros(H), torch.zeros(1, 2, H), h0=torch.zeros(2, H))
