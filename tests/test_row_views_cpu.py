"""The strided row movers take torch views (ops._rows, ops.pack_parts): the addresses, strides and shapes they hand to the C interface,
against numbers written out here, on CPU tensors (no device, no library call)."""
import pytest
import torch

from kai0_amd import ops

BF16 = torch.bfloat16


def x3():
    return torch.zeros((2, 8, 24), dtype=BF16)


def geometry(view, base):
    ptr, *rest = ops._rows(view)
    return (ptr - base.data_ptr(), *rest)  # (byte offset, batch stride, row stride, B, rows, cols)


def test_row_and_column_slices_of_a_3d_tensor():
    x = x3()
    assert geometry(x[:, 2:5], x) == (2 * 24 * 2, 192, 24, 2, 3, 24)
    assert geometry(x[:, :, 8:16], x) == (8 * 2, 192, 24, 2, 8, 8)
    assert geometry(x[:, 2:5, 8:16], x) == ((2 * 24 + 8) * 2, 192, 24, 2, 3, 8)
    assert ops._row0(x[:, 2:5], 192, 24) == 2 and ops._row0(x[:, 2:5, 8:16], 192, 24) == 2 and ops._row0(x[:, :, 8:16], 192, 24) == 0


def test_column_slice_of_a_fused_buffer_unflattened():
    B, L, H, HD = 2, 3, 3, 8
    W3 = (H + 2) * HD  # 40: dq | dk | dv
    buf = torch.zeros((B * L, W3), dtype=BF16)
    dk = buf[:, H * HD : (H + 1) * HD]
    assert geometry(dk.unflatten(0, (B, L)), buf) == (24 * 2, 120, 40, 2, 3, 8)
    assert ops._row0(dk.unflatten(0, (B, L)), 120, 40) == 0


def test_2d_view_is_one_batch_entry():
    y = torch.zeros((6, 16), dtype=BF16)
    assert geometry(y[1:5, 8:16], y) == ((16 + 8) * 2, 4 * 16, 16, 1, 4, 8)
    assert ops._row0(y[1:5, 8:16], 64, 16) == 0


def test_slab_of_a_stacked_buffer():
    B, S, HD = 2, 5, 8
    dkv = torch.zeros((2, B, S, HD), dtype=BF16)
    assert geometry(dkv[1], dkv) == (B * S * HD * 2, 40, 8, 2, 5, 8)
    assert geometry(dkv[1][:, 3:5], dkv) == ((B * S * HD + 3 * HD) * 2, 40, 8, 2, 2, 8)
    assert ops._row0(dkv[1], 40, 8) == 0 and ops._row0(dkv[1][:, 3:5], 40, 8) == 3


def test_pack_parts_fields():
    x, y = x3(), torch.zeros((2, 3, 8), dtype=BF16)
    (arr,) = ops.pack_parts([ops.Move(x[:, 2:5, 8:16], y, ops.ROPE_INV, 7), ops.Move(y, x[:, 5:8, 16:24], ops.COPY),
                             ops.Move(None, x[:, 5:], ops.ZERO)])
    assert len(arr) == 3
    a = arr[0]
    assert (a.src - x.data_ptr(), a.dst - y.data_ptr()) == ((2 * 24 + 8) * 2, 0)
    assert (a.src_bs, a.src_ld, a.dst_bs, a.dst_ld, a.B, a.rows, a.cols, a.mode, a.pos_off) == (192, 24, 24, 8, 2, 3, 8, 2, 7)
    a = arr[1]
    assert (a.src - y.data_ptr(), a.dst - x.data_ptr()) == (0, (5 * 24 + 16) * 2)
    assert (a.src_bs, a.src_ld, a.dst_bs, a.dst_ld, a.B, a.rows, a.cols, a.mode, a.pos_off) == (24, 8, 192, 24, 2, 3, 8, 0, 0)
    a = arr[2]  # ZERO: no source
    assert a.src is None and a.dst - x.data_ptr() == 5 * 24 * 2
    assert (a.src_bs, a.src_ld, a.dst_bs, a.dst_ld, a.B, a.rows, a.cols, a.mode, a.pos_off) == (0, 0, 192, 24, 2, 3, 24, 3, 0)
    assert (ops.COPY, ops.ROPE, ops.ROPE_INV, ops.ZERO) == (0, 1, 2, 3)


def test_13_moves_are_two_launches():
    x = x3()
    chunks = ops.pack_parts([ops.Move(None, x[:, i % 8 : i % 8 + 1], ops.ZERO) for i in range(13)])
    assert [len(c) for c in chunks] == [12, 1]
    assert chunks[1][0].dst - x.data_ptr() == (12 % 8) * 24 * 2


@pytest.mark.parametrize("bad,word", [
    (lambda: x3()[:, :, ::2], "last stride"),
    (lambda: torch.zeros((2, 2, 8, 24), dtype=BF16), "view"),
    (lambda: torch.zeros((2, 8, 24), dtype=torch.float32), "float32"),
    (lambda: x3()[:, 3:3], "empty"),
])  # fmt: skip
def test_rows_rejects(bad, word):
    with pytest.raises(ValueError, match=word) as e:
        ops._rows(bad(), "mover: src")
    assert "mover: src" in str(e.value)


def test_movers_reject_before_any_launch():
    x, y = x3(), torch.zeros((2, 3, 8), dtype=BF16)
    with pytest.raises(ValueError, match="differ in shape"):
        ops.copy_rows(x[:, 2:6, 8:16], y)
    with pytest.raises(ValueError, match="move 1.*differ in shape"):
        ops.pack_parts([ops.Move(None, y, ops.ZERO), ops.Move(x[:, 2:6, 8:16], y, ops.COPY)])
    with pytest.raises(ValueError, match="unknown kind"):
        ops.pack_parts([ops.Move(y, y, 7)])
    with pytest.raises(ValueError, match="ZERO takes src=None"):
        ops.pack_parts([ops.Move(y, y, ops.ZERO)])
    pos, inv = torch.zeros((2, 8), dtype=torch.int32), torch.ones(4)
    with pytest.raises(ValueError, match="rope_: x.*do not fit the in-place entry point"):
        ops.rope_(x[:, :, 8:16], pos, inv, 8)  # rows not dense: a column slice
    with pytest.raises(ValueError, match="positions"):
        ops.rope_(x[:, 2:5], pos, inv, 8)  # 3 rows, 8 positions
    with pytest.raises(ValueError, match="not the same rows"):
        ops.rope2_(x[:, 2:5], x3()[:, 1:4], pos[:, :3].contiguous(), inv, 8)
