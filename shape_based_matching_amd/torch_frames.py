"""Planar PyTorch frames for Context.match_batch_device_planes: the table of plane addresses of a [B, 3, H, W] uint8 batch, or of a
list of [3, H, W] tensors (what torchvision's GPU JPEG decoder returns), with no copy of the pixels.

plane_addresses is arithmetic on data_ptr() and stride() and works on CPU tensors as well; views and windows -- slices along H and
W -- are taken where they lie, their row stride being the stride of the tensor they were cut from.  `order` lists, for each channel
the matcher sees (the reference's B, G, R), the tensor channel it is read from: (2, 1, 0) presents an RGB tensor as the BGR frame."""
from typing import List, Sequence, Tuple


def _frames(frames) -> list:
    if hasattr(frames, "dim"):  # one tensor: a batch [B, 3, H, W] or a single frame [3, H, W]
        if frames.dim() == 4:
            return [frames[b] for b in range(frames.shape[0])]
        return [frames]
    return list(frames)


def plane_addresses(frames, order: Sequence[int] = (0, 1, 2)) -> Tuple[List[int], int]:
    """(addresses, stride): addresses[3 f + c] is the first byte of plane order[c] of frame f, stride the bytes per row that all
    planes share.  ValueError: not uint8, not [3, H, W] frames of one size, a W stride other than 1, row strides that differ."""
    import torch

    fr = _frames(frames)
    if not fr:
        raise ValueError("no frames")
    order = tuple(int(o) for o in order)
    if len(order) != 3 or any(o < 0 or o > 2 for o in order):
        raise ValueError("order names three channels out of 0, 1, 2")
    addresses, stride, shape = [], None, None
    for f, t in enumerate(fr):
        if t.dtype != torch.uint8:
            raise ValueError("frame %d is %s, not uint8" % (f, t.dtype))
        if t.dim() != 3 or t.shape[0] != 3:
            raise ValueError("frame %d has shape %s, not [3, H, W]" % (f, tuple(t.shape)))
        if shape is None:
            shape = tuple(t.shape)
        if tuple(t.shape) != shape:
            raise ValueError("frame %d has shape %s, frame 0 %s" % (f, tuple(t.shape), shape))
        sc, sh, sw = t.stride()
        if sw != 1 and t.shape[2] > 1:
            raise ValueError("frame %d: the W stride is %d, the pixels of a row must be adjacent" % (f, sw))
        if t.shape[1] == 1:
            sh = stride if stride is not None else t.shape[2]  # one row: its stride is never read
        if stride is None:
            stride = sh
        if sh != stride:
            raise ValueError("frame %d: row stride %d, frame 0 has %d; the planes of a call share one" % (f, sh, stride))
        if stride < t.shape[2]:
            raise ValueError("frame %d: row stride %d below the width %d" % (f, stride, t.shape[2]))
        base = t.data_ptr()  # uint8: element strides are byte strides
        addresses.extend(base + o * sc for o in order)
    return addresses, int(stride)


def plane_table(frames, order: Sequence[int] = (0, 1, 2), out=None, stream=None):
    """(table, stride): the addresses of plane_addresses in an int64 DEVICE tensor -- `out` (at least 3 * frames entries, on the
    frames' device; the rest is left alone) or a new one -- written on `stream` (default: the current one) from pinned memory, so
    that the copy is ordered before the kernels of a match call enqueued on that stream afterwards.  Rewriting `out` between the
    replays of one captured graph is how one graph serves frames that move."""
    import torch

    fr = _frames(frames)
    addresses, stride = plane_addresses(fr, order)
    device = fr[0].device
    if device.type != "cuda":
        raise ValueError("plane_table needs frames in device memory (plane_addresses works on any tensor)")
    n = len(addresses)
    if out is None:
        out = torch.empty(n, dtype=torch.int64, device=device)
    elif out.dtype != torch.int64 or out.dim() != 1 or out.numel() < n or not out.is_contiguous() or out.device != device:
        raise ValueError("out must be a contiguous int64 tensor of at least %d entries on %s" % (n, device))
    host = torch.tensor(addresses, dtype=torch.int64).pin_memory()
    st = stream if stream is not None else torch.cuda.current_stream(device)
    with torch.cuda.stream(st):
        out[:n].copy_(host, non_blocking=True)
    st.synchronize()  # (the pinned source may go)
    return out, stride
