"""MLX affine group quantisation without a device: the bit layout of the packed words, ``ops.quantize_affine``, the refusals of ``mi355_qlinear``
(checked before any device work, on made-up aligned addresses that are never read) and the form switch of ``mi355_qlinear_route``."""
import ctypes

import pytest
import torch

from mlx_audio_amd import _lib, ops


def test_bit_layout():
    assert ops.pack_codes(torch.arange(8)[None], 4).view(torch.int32).tolist() == [[0x76543210]]
    assert ops.pack_codes(torch.tensor([[0x10, 0x32, 0x54, 0x76, 0xFF, 0, 0, 0x80]]), 8).view(torch.int32).tolist() == [[0x76543210, 0x800000FF - (1 << 32)]]
    for bits in (4, 8):
        codes = torch.randint(0, 1 << bits, (3, 64), generator=torch.Generator().manual_seed(bits))
        assert torch.equal(ops.unpack_codes(ops.pack_codes(codes, bits), bits), codes)


@pytest.mark.parametrize("bits,g", [(4, 32), (4, 64), (8, 64), (8, 128)])
def test_quantize_affine_is_within_half_a_step(bits, g):
    w = torch.randn(5, 3 * g, generator=torch.Generator().manual_seed(g + bits))
    w[1, :g] = 0.25   # a constant group: codes 0, the value in the zero
    wq, s, z = ops.quantize_affine(w, g, bits)
    assert wq.dtype == torch.uint32 and tuple(wq.shape) == (5, 3 * g * bits // 32) and tuple(s.shape) == tuple(z.shape) == (5, 3)
    assert ops.infer_quantization(wq.shape[1], s.shape[1], group_size=g) == (bits, g) == ops.infer_quantization(wq.shape[1], s.shape[1], bits=bits)
    sd = s.double().repeat_interleave(g, 1)
    deq = sd * ops.unpack_codes(wq, bits) + z.double().repeat_interleave(g, 1)
    assert bool(((deq - w.double()).abs() <= 0.5 * sd * (1 + 1e-6)).all())
    assert torch.equal(deq[1, :g], w[1, :g].double())


REFUSALS = [(dict(bits=b), -3, f"bits = {b} ") for b in (2, 3, 5, 6)] + [(dict(group_size=g), -3, f"group_size = {g} ") for g in (16, 48, 256)] + [
    (dict(K=96, ldx=96), -3, "K = 96 is not a multiple of group_size = 64"), (dict(K=160, ldx=160, group_size=128), -3, "K = 160 is not a multiple"),
    (dict(x=0), -1, "null pointer"), (dict(q=0), -1, "null pointer"), (dict(sz=0), -1, "null pointer"), (dict(y=0), -1, "null pointer"),
    (dict(M=0), -1, "M = 0"), (dict(x=0x10000004), -1, "16-byte aligned"), (dict(ldx=130), -1, "16-byte aligned"), (dict(ldy=32), -1, "shorter than N"),
    (dict(norm=1), -3, "norm"), (dict(glu=1), -3, "glu"), (dict(rope_cos=0x50000000), -3, "rope"), (dict(x_ids=0x50000000), -3, "x_ids")]


@pytest.mark.parametrize("fields,rc,fragment", REFUSALS, ids=lambda v: "-".join(f"{k}{x}" for k, x in v.items()) if isinstance(v, dict) else None)
def test_refusals_come_before_any_device_work(fields, rc, fragment):
    with pytest.raises(_lib.Mi355Error, match=rf"\({rc}\).*{fragment}"):
        sizes = {**dict(M=4, N=33, K=128, bits=4, group_size=64), **{k: v for k, v in fields.items() if k in ("M", "K", "bits", "group_size")}}
        ops.qlinear_route(**sizes, **{k: v for k, v in fields.items() if k not in sizes})
    kw = dict(x=0x10000000, ldx=128, M=4, K=128, N=33, q=0x20000000, sz=0x30000000, bits=4, group_size=64, sz_dtype=2, y=0x40000000, ldy=33)
    kw.update(fields)
    st = _lib.STRUCTS["mi355_qlinear_args"](**kw)
    assert _lib.load().mi355_qlinear(ctypes.byref(st), None) == rc and fragment in _lib.load().mi355_last_error().decode()


def test_route_switches_form_between_8_and_9_rows():
    rows = {M: ops.qlinear_route(M, 1280, 1280, 4, 64) for M in (1, 2, 3, 5, 8, 9, 16, 17, 65)}
    assert [rows[M]["form"] for M in (1, 2, 3, 5, 8)] == [ops.QLINEAR_STREAM] * 5 and [rows[M]["rows"] for M in (1, 2, 3, 5, 8)] == [1, 2, 4, 8, 8]
    assert [rows[M]["form"] for M in (9, 16, 17, 65)] == [ops.QLINEAR_TILE] * 4 and [rows[M]["rows"] for M in (9, 16, 17, 65)] == [16, 16, 32, 32]
    assert (rows[8]["grid_x"], rows[8]["grid_y"]) == (160, 1) and (rows[65]["grid_x"], rows[65]["grid_y"]) == (80, 3)
    assert rows[8]["chunk_k"] == 1280 and ops.qlinear_route(8, 16, 5120, 8, 32)["chunk_k"] < 5120   # K = 5120 at 8 rows is staged in chunks
    assert all(r["lds_bytes"] <= 80 * 1024 for r in rows.values())
