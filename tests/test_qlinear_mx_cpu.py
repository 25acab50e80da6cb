"""MLX mxfp4 / nvfp4 / mxfp8 without a device: ``ops.quantize_mx`` and the value tables, ``ops.infer_quantization_mx``, and the route and refusals
of ``mi355_qlinear_mx_route`` on made-up aligned addresses that are never read."""
import pytest
import torch

from mlx_audio_amd import _lib, ops

MODES = tuple(ops.QMODES)


def test_value_tables():
    assert ops.mx_code_values(torch.arange(16), "nvfp4").tolist() == [0, 0.5, 1, 1.5, 2, 3, 4, 6, -0.0, -0.5, -1, -1.5, -2, -3, -4, -6]
    assert ops.mx_code_values(torch.tensor([0x01, 0x08, 0x38, 0x7E, 0xB8]), "mxfp8").tolist() == [2.0 ** -9, 2.0 ** -6, 1.0, 448.0, -1.0]
    assert ops.mx_scale_values(torch.tensor([0, 124, 127, 130], dtype=torch.uint8), "mxfp4").tolist() == [2.0 ** -127, 0.125, 1.0, 8.0]
    assert ops.mx_scale_values(torch.tensor([0x38, 0x3C, 0x7E], dtype=torch.uint8), "nvfp4").tolist() == [1.0, 1.5, 448.0]


@pytest.mark.parametrize("mode", MODES)
def test_quantize_mx_is_within_half_an_element_step(mode):
    _, bits, g = ops.QMODES[mode]
    w = torch.randn(6, 4 * g, generator=torch.Generator().manual_seed(bits + g)) * torch.tensor([1e-3, 0.1, 1.0, 1.0, 30.0, 0.0])[:, None]
    w[2, :g] = torch.tensor([6.0, -0.25, 0.75, 1.25, 5.0, -2.5] + [0.0] * (g - 6))   # fp4 ties at scale 1: to the even code, 0, 1, 1, 4, -2
    wq, s = ops.quantize_mx(w, mode)
    assert wq.dtype == torch.uint32 and tuple(wq.shape) == (6, 4 * g * bits // 32) and s.dtype == torch.uint8 and tuple(s.shape) == (6, 4)
    assert ops.infer_quantization_mx(wq.shape[1], s.shape[1]) == (mode, bits, g) == ops.infer_quantization_mx(wq.shape[1], s.shape[1], mode=mode)
    sd = ops.mx_scale_values(s, mode).double().repeat_interleave(g, 1)
    deq = ops.mx_code_values(ops.unpack_codes(wq, bits), mode).double() * sd
    a = (w.double().abs() / sd.clamp_min(2.0 ** -140)).clamp_min(2.0 ** -30)   # the element grid's spacing at |w| / scale
    step = torch.where(a < 2, 0.5, torch.where(a < 4, 1.0, 2.0)) if bits == 4 else torch.pow(2.0, torch.floor(torch.log2(a)).clamp_min(-6) - 3)
    assert bool(((deq - w.double()).abs() <= 0.5 * step * sd * (1 + 1e-6)).all())
    if mode == "mxfp4":
        assert deq[2, :6].tolist() == [6.0, -0.0, 1.0, 1.0, 4.0, -2.0]
    with pytest.raises(ValueError, match="contradicts the shapes"):
        ops.infer_quantization_mx(wq.shape[1], s.shape[1], mode="mxfp8" if mode != "mxfp8" else "nvfp4")


REFUSALS = [(dict(group_size=64), -3, "group_size = 64"), (dict(bits=8), -3, "bits = 8"),
            (dict(K=48, ldx=48), -3, "K = 48 is not a multiple of 32"), (dict(scales=0), -1, "null pointer"), (dict(M=0), -1, "M = 0"),
            (dict(x=0x10000004), -1, "16-byte aligned"), (dict(ldy=32), -1, "shorter than N"),
            (dict(norm=1), -3, "norm"), (dict(glu=1), -3, "glu"), (dict(rope_cos=0x50000000), -3, "rope"), (dict(x_ids=0x50000000), -3, "x_ids")]


@pytest.mark.parametrize("fields,rc,fragment", REFUSALS, ids=lambda v: "-".join(f"{k}{x}" for k, x in v.items()) if isinstance(v, dict) else None)
def test_refusals_come_before_any_device_work(fields, rc, fragment):
    with pytest.raises(_lib.Mi355Error, match=rf"\({rc}\).*{fragment}"):
        sizes = {**dict(M=4, N=33, K=128), **{k: v for k, v in fields.items() if k in ("M", "K")}}
        ops.qlinear_mx_route(**sizes, mode="mxfp4", **{k: v for k, v in fields.items() if k not in sizes})


@pytest.mark.parametrize("mode", MODES)
def test_route_switches_form_between_8_and_9_rows(mode):
    rows = {M: ops.qlinear_mx_route(M, 1280, 1280, mode) for M in (1, 2, 3, 5, 8, 9, 16, 17, 65)}
    assert [rows[M]["form"] for M in (1, 2, 3, 5, 8)] == [ops.QLINEAR_STREAM] * 5 and [rows[M]["rows"] for M in (1, 2, 3, 5, 8)] == [1, 2, 4, 8, 8]
    assert [rows[M]["form"] for M in (9, 16, 17, 65)] == [ops.QLINEAR_TILE] * 4 and [rows[M]["rows"] for M in (9, 16, 17, 65)] == [16, 16, 32, 32]
    assert (rows[8]["grid_x"], rows[8]["grid_y"]) == (160, 1) and (rows[65]["grid_x"], rows[65]["grid_y"]) == (80, 3)
    assert rows[8]["chunk_k"] == 1280 and ops.qlinear_mx_route(8, 16, 5120, mode)["chunk_k"] < 5120 and rows[8]["mode"] == ops.QMODES[mode][0]
    assert all(r["lds_bytes"] <= 80 * 1024 for r in rows.values())
    assert ops.qlinear_mx_route(9, 8, 48, "nvfp4")["chunk_k"] == 128   # K % 16 == 0 is enough at nvfp4
