"""CPU (not gpu): shape_based_matching_amd.torch_frames.plane_addresses -- the table of plane addresses of planar PyTorch frames
for Context.match_batch_device_planes, as arithmetic on data_ptr() and stride().  On CPU tensors the addresses can be read back:
every entry must be the first byte of the plane it names."""
import ctypes

import numpy as np
import pytest
import torch

from shape_based_matching_amd.torch_frames import plane_addresses, plane_table


def byte_at(addr):
    return ctypes.c_uint8.from_address(addr).value


def batch(b=4, h=6, w=8, seed=3):
    return torch.from_numpy(np.random.RandomState(seed).randint(0, 256, (b, 3, h, w)).astype(np.uint8))


def check(addresses, stride, frames, order=(0, 1, 2)):
    """entry 3 f + c is plane order[c] of frame f: its first byte, and (through the stride) its last row's last byte"""
    assert len(addresses) == 3 * len(frames)
    for f, t in enumerate(frames):
        h, w = t.shape[1:]
        for c in range(3):
            a = addresses[3 * f + c]
            assert byte_at(a) == int(t[order[c], 0, 0]), (f, c)
            assert byte_at(a + (h - 1) * stride + w - 1) == int(t[order[c], h - 1, w - 1]), (f, c)


def test_contiguous_batch():
    x = batch()
    addresses, stride = plane_addresses(x)
    assert stride == 8
    base = x.data_ptr()
    assert addresses == [base + (3 * f + c) * 48 for f in range(4) for c in range(3)]
    check(addresses, stride, list(x))
    # one frame [3, H, W] is a batch of one
    a1, s1 = plane_addresses(x[2])
    assert a1 == addresses[6:9] and s1 == stride


def test_list_of_separately_allocated_frames():
    frames = [batch(1, seed=s)[0].clone() for s in (1, 2, 3)]
    frames = [frames[2], frames[0], frames[2], frames[1]]  # any order, one listed twice
    addresses, stride = plane_addresses(frames)
    assert stride == 8 and addresses[0:3] == addresses[6:9]
    check(addresses, stride, frames)


def test_reversed_order_is_the_channel_swap():
    x = batch()
    straight, _ = plane_addresses(x)
    rev, stride = plane_addresses(x, order=(2, 1, 0))
    for f in range(4):
        assert rev[3 * f:3 * f + 3] == straight[3 * f:3 * f + 3][::-1]
    check(rev, stride, list(x), order=(2, 1, 0))
    # a plane may be listed more than once
    same, _ = plane_addresses(x, order=(1, 1, 1))
    assert all(same[3 * f + c] == straight[3 * f + 1] for f in range(4) for c in range(3))


def test_sliced_window_keeps_the_canvas_stride():
    canvas = batch(2, 20, 32)
    win = canvas[:, :, 5:17, 7:27]  # 12 x 20 at (5, 7): an odd byte offset
    assert not win.is_contiguous()
    addresses, stride = plane_addresses(win)
    assert stride == 32
    assert addresses[0] == canvas.data_ptr() + 5 * 32 + 7 and addresses[0] % 2 == 1
    check(addresses, stride, list(win))
    # windows at another place in each canvas, as a list
    wins = [canvas[0][:, 0:12, 1:21], canvas[1][:, 8:20, 12:32]]
    a2, s2 = plane_addresses(wins, order=(2, 1, 0))
    assert s2 == 32
    check(a2, s2, wins, order=(2, 1, 0))


def test_value_errors():
    x = batch()
    with pytest.raises(ValueError):  # the W stride is not 1: every second column, and an NHWC tensor seen as NCHW
        plane_addresses(x[:, :, :, ::2])
    with pytest.raises(ValueError):
        plane_addresses(x.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2))
    with pytest.raises(ValueError):  # row strides that differ between the frames of a list
        plane_addresses([batch(1, 6, 8)[0], batch(1, 6, 16)[0][:, :, :8]])
    with pytest.raises(ValueError):  # not uint8
        plane_addresses(x.to(torch.float32))
    with pytest.raises(ValueError):
        plane_addresses(x.to(torch.int8))
    # and what else cannot be a table: other shapes, frames of two sizes, an order that is no channel list, nothing at all
    for bad in (x[:, :2], x[0][0], [x[0], x[1][:, :4]], []):
        with pytest.raises(ValueError):
            plane_addresses(bad)
    for order in ((0, 1), (0, 1, 3), (-1, 0, 1)):
        with pytest.raises(ValueError):
            plane_addresses(x, order=order)
    with pytest.raises(ValueError):  # the table itself is device memory
        plane_table(x)
