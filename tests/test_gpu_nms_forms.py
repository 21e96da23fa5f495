"""-m gpu: k_nms_frames (sbm_nms_batch_device) at the edges of its gather, sort, compaction and walk -- the cases of
tests/nms_form_cases.py written into device buffers.  Every frame's kept list (as rows), count and flags word must equal the
case's expectation exactly: epilogue() then py_nms, which tests/test_reference_nms.py pins to the reference's nms.hpp.  Every
launch runs a second time with its frames in reverse order (a frame's result must not depend on its block index); d_out is
prefilled with a sentinel byte and the counts with -1, so that a record written beyond min(kept, out_cap) or a pair left
unwritten shows.  No fault is provoked and nothing is timed."""
import numpy as np
import pytest

import nms_form_cases as NC
from shape_based_matching_amd.templates import MATCH_DTYPE

pytestmark = pytest.mark.gpu
REC = NC.REC
GUARD = 4096  # sentinel bytes behind the last frame's records


@pytest.fixture()
def ctx(ctx_factory, case1):
    c = ctx_factory()
    ts = NC.label_table(case1["templates"])
    assert NC.sizes_of(ts) == NC.SIZES
    c.upload_templates(ts)
    return c


def run_launch(ctx, launch, order=None, stream=0):
    """one sbm_nms_batch_device call over the launch's frames in the given order: (the bytes of d_out, the count pairs)"""
    import torch

    order = list(range(len(launch.cases))) if order is None else list(order)
    buf, hdr, stride = launch.buffer(order)
    nf = len(order)
    d = torch.from_numpy(buf).to("cuda:0")
    d_out = torch.full((nf * launch.out_cap * REC + GUARD,), NC.SENTINEL_BYTE, dtype=torch.uint8, device="cuda:0")
    d_oc = torch.full((nf * 2,), -1, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    p = launch.params
    ctx.nms_batch_device(d.data_ptr() + hdr, d.data_ptr(), launch.cap, nf, d_out.data_ptr(), launch.out_cap, d_oc.data_ptr(), p.score, p.thr,
                         p.eta, p.top_k, n_parts=launch.n_parts, part_stride=stride, stream=stream)
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), d_oc.cpu().numpy().reshape(-1, 2)


def check_launch(ctx, launch, order=None, stream=0):
    order = list(range(len(launch.cases))) if order is None else list(order)
    out, oc = run_launch(ctx, launch, order, stream)
    frame = launch.out_cap * REC
    for k, ci in enumerate(order):
        c = launch.cases[ci]
        want = NC.want(c)
        where = (launch.name, c.name, k)
        assert oc[k, 0] == len(want), where
        assert oc[k, 1] == c.flags, where
        stored = min(len(want), launch.out_cap)
        mine = out[k * frame: (k + 1) * frame]
        assert NC.rows_of(mine[: stored * REC].view(MATCH_DTYPE)) == NC.rows_of(want[:stored]), where
        assert (mine[stored * REC:] == NC.SENTINEL_BYTE).all(), where  # nothing beyond min(kept, out_cap) records
    assert (out[len(order) * frame:] == NC.SENTINEL_BYTE).all(), launch.name


def check_group(ctx, group):
    for launch in NC.launches(group):
        check_launch(ctx, launch)
        check_launch(ctx, launch, reversed(range(len(launch.cases))))


def test_record_counts(ctx):
    """n = 0 .. 4097 around the chunk, the tile, the sort paddings and NMS_LDS_MAX, LDS and scratch frames in one launch; and the
    host's N > NMS_LDS_MAX against the kernel's n <= NMS_LDS_MAX"""
    check_group(ctx, "counts")


def test_candidate_counts(ctx):
    """m = 0 .. 1025 candidates cut out of 1100 records by the score threshold, between two similarities and equal to one"""
    check_group(ctx, "candidates")


def test_top_k(ctx):
    """top_k on the chunk, tile and list boundaries; an unknown label just inside and just outside the cut"""
    check_group(ctx, "top_k")


def test_unique_step(ctx):
    """runs across the wave and tile boundaries, at position 0 and at n - 1; equal records that are not adjacent; exact duplicates
    told apart by raw alone -- the index tie-break of the sort -- in one part, across parts, and under sentinel padding"""
    check_group(ctx, "unique")


def test_sort_keys(ctx):
    check_group(ctx, "sort_keys")


def test_walk_order(ctx):
    check_group(ctx, "walk")


def test_overlap_equal_to_the_threshold(ctx):
    check_group(ctx, "equal_overlap")


def test_adaptive_threshold(ctx):
    check_group(ctx, "adaptive")


def test_kept_list_and_outputs(ctx):
    """2049 kept boxes against out_cap 2049, 2048, 5 and 0: the count is always the full one, flag 2 says what was cut"""
    check_group(ctx, "outputs")


def test_parts(ctx):
    check_group(ctx, "parts")


def test_seventy_frames(ctx):
    check_group(ctx, "launches")


def test_scratch_growth_between_calls(ctx):
    """a call with scratch frames, a call whose n_parts * cap makes the scratch grow, then the first call again on the context's
    stream and on a caller's stream"""
    import torch

    first, second = NC.scratch_growth()
    assert second.n_parts * second.cap > first.n_parts * first.cap > NC.NMS_LDS_MAX
    check_launch(ctx, first)
    check_launch(ctx, second)
    check_launch(ctx, first)
    s = torch.cuda.Stream()
    check_launch(ctx, first, stream=s.cuda_stream)
    check_launch(ctx, second, reversed(range(len(second.cases))), stream=s.cuda_stream)
