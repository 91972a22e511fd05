"""The guarded-buffer helpers of tests/helpers.py (carve, carve_like, guards_intact) on CPU tensors:
what test_gpu_buffers.py and test_gpu_stage_img.py rely on to notice a kernel that writes one byte
outside a buffer it was handed.  The helpers' sensitivity is shown with torch index assignments only."""
import numpy as np
import pytest

from helpers import GUARD, carve, carve_like, guards_intact

torch = pytest.importorskip("torch")

CASES = [((3, 5, 7), torch.float32), ((2, 9), torch.bfloat16), ((13,), torch.uint8), ((4, 6), torch.int32), (11, torch.uint8)]


@pytest.mark.parametrize("shape,dtype", CASES)
@pytest.mark.parametrize("fill,guard_fill", [(0x00, 0x00), (0xFF, 0xFF), (0xA5, 0xA5), (0x00, 0xFF)])
def test_carve_view_and_fills(shape, dtype, fill, guard_fill):
    buf, view = carve(shape, dtype, "cpu", fill, guard_fill)
    want_shape = (shape,) if isinstance(shape, int) else shape
    nbytes = int(np.prod(want_shape)) * torch.empty(0, dtype=dtype).element_size()
    assert view.dtype == dtype and tuple(view.shape) == want_shape and view.is_contiguous()
    assert view.numel() * view.element_size() == nbytes
    assert buf.dtype == torch.uint8 and buf.numel() == GUARD + nbytes + GUARD
    assert view.data_ptr() == buf.data_ptr() + GUARD  # the allocation's 256-byte alignment is kept
    assert GUARD % 256 == 0
    b = buf.numpy()
    assert (b[:GUARD] == guard_fill).all() and (b[GUARD + nbytes:] == guard_fill).all()
    assert (b[GUARD:GUARD + nbytes] == fill).all()
    guards_intact(buf, nbytes, "clean", guard_fill)
    # the view aliases the interior: writing all of it leaves the guards alone
    view.view(torch.uint8).fill_(fill ^ 0x5A)
    assert (b[GUARD:GUARD + nbytes] == fill ^ 0x5A).all()
    guards_intact(buf, nbytes, "interior written", guard_fill)


def test_ff_prefill_is_nan_and_all_ones():
    _, f = carve((4,), torch.float32, "cpu", 0xFF, 0xFF)
    _, h = carve((4,), torch.bfloat16, "cpu", 0xFF, 0xFF)
    _, i = carve((4,), torch.int32, "cpu", 0xFF, 0xFF)
    assert torch.isnan(f).all() and torch.isnan(h.float()).all() and (i == -1).all()


@pytest.mark.parametrize("guard_fill", [0x00, 0xFF, 0xA5])
def test_one_byte_before_is_noticed(guard_fill):
    buf, view = carve((5, 3), torch.float32, "cpu", 0x00, guard_fill)
    nbytes = 60
    buf[GUARD - 1] = guard_fill ^ 0x01
    with pytest.raises(AssertionError, match="dx: bytes before the buffer overwritten"):
        guards_intact(buf, nbytes, "dx", guard_fill)


@pytest.mark.parametrize("guard_fill", [0x00, 0xFF, 0xA5])
def test_one_byte_after_is_noticed(guard_fill):
    buf, view = carve((5, 3), torch.float32, "cpu", 0x00, guard_fill)
    nbytes = 60
    buf[GUARD + nbytes] = guard_fill ^ 0x80
    with pytest.raises(AssertionError, match="mask: bytes after the buffer overwritten"):
        guards_intact(buf, nbytes, "mask", guard_fill)


def test_far_ends_of_the_guards_are_noticed():
    for at, side in ((0, "before"), (2 * GUARD + 60 - 1, "after")):
        buf, _ = carve((15,), torch.float32, "cpu", 0x00, 0xFF)
        buf[at] = 0
        with pytest.raises(AssertionError, match=f"bytes {side} the buffer"):
            guards_intact(buf, 60, "ws", 0xFF)


def test_wrong_size_is_refused():
    buf, _ = carve((15,), torch.float32, "cpu", 0x00, 0xFF)
    with pytest.raises(AssertionError, match="not a carved buffer"):
        guards_intact(buf, 64, "ws", 0xFF)


def test_carve_like_copies_bits():
    t = torch.arange(24, dtype=torch.float32).reshape(2, 3, 4).transpose(0, 2)  # not contiguous
    buf, view = carve_like(t, 0xFF)
    assert view.is_contiguous() and view.dtype == t.dtype and tuple(view.shape) == tuple(t.shape)
    assert torch.equal(view, t)
    guards_intact(buf, 96, "x", 0xFF)
    assert torch.isnan(buf[:GUARD].view(torch.float32)).all() and torch.isnan(buf[GUARD + 96:].view(torch.float32)).all()
