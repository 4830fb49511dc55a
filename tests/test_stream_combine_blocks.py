"""CPU tests of the pair stream's combine by row blocks (spmm_stream_combine_kernel in csrc/spmm_stream.hip): a workgroup takes
``PAIR_STREAM_COMBINE_ROWS`` consecutive stream rows, stages their range of ``row_seg`` through an LDS tile of ``PAIR_STREAM_COMBINE_CAP``
entries — in entry order, thread ``t`` the entries ``t, t + 256, ...`` of a tile, ``tile[j] = partial[row_seg[base + j]]`` — and thread
``i`` adds its row's floats from the tile in ``row_seg`` order, keeping its sum and its next entry from one tile to the next.

``tile_walk`` restates that walk in numpy, thread by thread and tile by tile, from the sentence above.  On plans of
``wide_plans.pair_stream_plan`` (through ``HopGraph.pair_stream_plan``; the families of tests/test_stream_queue_order.py) it must give, for
every row, the bits of the chain ((p_0 + p_1) + p_2) + ... over ``partial[row_seg[s]]`` in ``row_seg`` order from 0.f — the thread-per-row
kernel's chain — with random floats of mixed magnitude as partials, so that another order or a lost carry is another number.  Every tile
place is written exactly once and read exactly once.  The walk runs with the kernel's own (rows, cap) and with small ones, at which the
small plans show every shape: a full block, a short last block (a range that is no multiple of the block), a single-row last block, a
block of several tiles, a row that straddles a tile edge, a row that alone spans three tiles.  Two planted errors — the sum not carried
over a tile edge, a tile staged one place off — are seen.  The module constants the GPU tests read are held against the source."""
import os
import re

import numpy as np
import pytest

import gnan_amd  # noqa: F401
from gnan_amd import aggregate

from test_stream_queue_order import _family

f32 = np.float32
THREADS = 256


def block_shapes(ptr, rb, cap):
    """What a plan's ``row_slot_ptr`` makes the tile walk meet: per block (rows, entries, tiles), and the rows that straddle a tile edge."""
    ptr = np.asarray(ptr, dtype=np.int64)
    n_rows = len(ptr) - 1
    blocks, straddle = [], []
    for r0 in range(0, n_rows, rb):
        rows = min(rb, n_rows - r0)
        e0, e1 = int(ptr[r0]), int(ptr[r0 + rows])
        blocks.append((rows, e1 - e0, -(-(e1 - e0) // cap)))
        for r in range(r0, r0 + rows):
            if (int(ptr[r]) - e0) // cap != (int(ptr[r + 1]) - 1 - e0) // cap:
                straddle.append(r)
    return blocks, straddle


def tile_walk(row_seg, ptr, partial, rb, cap, carry_sum=True, stage_shift=0):
    """The kernel's walk: (y of every row, reads per entry).  ``carry_sum`` False and ``stage_shift`` 1 are the planted errors: a row's
    sum starts again behind a tile edge; place j of a tile holds the float of the tile's entry j + 1."""
    n_rows = len(ptr) - 1
    y = np.zeros(n_rows, dtype=f32)
    reads = np.zeros(len(row_seg), dtype=np.int64)
    for r0 in range(0, n_rows, rb):
        rows = min(rb, n_rows - r0)
        s = [int(ptr[r0 + i]) for i in range(rows)]                     # a thread's next entry
        s1 = [int(ptr[r0 + i + 1]) for i in range(rows)]
        e0, e1 = int(ptr[r0]), int(ptr[r0 + rows])
        for base in range(e0, e1, cap):
            m = min(cap, e1 - base)
            tile, writes = np.full(cap, np.nan, dtype=f32), np.zeros(cap, dtype=np.int64)
            for t in range(min(THREADS, m)):                            # staging, entry order: thread t the places t, t + 256, ...
                j = np.arange(t, m, THREADS)
                tile[j] = partial[row_seg[base + (j + stage_shift) % m]]
                writes[j] += 1
            assert (writes[:m] == 1).all() and not writes[m:].any(), "every place of a tile is staged exactly once"
            # (barrier) thread i: its row's entries that lie in this tile
            for i in range(rows):
                hi = min(s1[i], base + m)
                if not carry_sum and int(ptr[r0 + i]) < base and s[i] < hi:
                    y[r0 + i] = f32(0)
                while s[i] < hi:
                    assert 0 <= s[i] - base < m
                    y[r0 + i] = f32(y[r0 + i] + tile[s[i] - base])
                    reads[s[i]] += 1
                    s[i] += 1
            # (barrier)
        assert s == s1, "every row of the block is through its entries when the block's tiles are"
    return y, reads


def chain(row_seg, ptr, partial):
    """The thread-per-row kernel: y = 0.f; for s in row order: y += partial[row_seg[s]]."""
    y = np.zeros(len(ptr) - 1, dtype=f32)
    for r in range(len(y)):
        for s in range(int(ptr[r]), int(ptr[r + 1])):
            y[r] = f32(y[r] + partial[row_seg[s]])
    return y


def _partials(rng, n_seg):
    return (rng.standard_normal(n_seg) * 2.0 ** rng.integers(-6, 7, n_seg)).astype(f32)


def _plan_arrays(n, block_rows, n_blocks, min_pairs, chunk):
    plan = _family(n, block_rows, n_blocks, min_pairs, chunk)[-1]
    row_seg, ptr = plan.row_seg.long().numpy(), plan.row_slot_ptr.long().numpy()
    assert sorted(row_seg.tolist()) == list(range(plan.n_seg)) and ptr[0] == 0 and ptr[-1] == plan.n_seg
    return row_seg, ptr


SHIPPED = (aggregate.PAIR_STREAM_COMBINE_ROWS, aggregate.PAIR_STREAM_COMBINE_CAP)
# (n, block_rows, n_blocks, min_pairs, chunk) of tests/test_stream_queue_order.py's families x (rows per block, tile entries)
PLANS = [(300, 4, 1, 5, 16), (400, 16, 4, 9, 16), (350, 4, 4, 17, 32)]
WALKS = [SHIPPED, (128, 2048), (64, 256), (16, 64), (97, 16), (1, 32)]     # (195 stream rows = 2 x 97 + 1; rows of 49 .. 60 entries)


@pytest.mark.parametrize("n,block_rows,n_blocks,min_pairs,chunk", PLANS)
@pytest.mark.parametrize("rb,cap", WALKS)
def test_the_tile_walk_gives_every_row_the_chain_of_row_seg_order(n, block_rows, n_blocks, min_pairs, chunk, rb, cap):
    row_seg, ptr = _plan_arrays(n, block_rows, n_blocks, min_pairs, chunk)
    partial = _partials(np.random.default_rng(n + rb + cap), len(row_seg))
    y, reads = tile_walk(row_seg, ptr, partial, rb, cap)
    want = chain(row_seg, ptr, partial)
    assert np.array_equal(y.view(np.int32), want.view(np.int32))
    assert (reads == 1).all(), "every entry is added exactly once"
    # (the chain is not indifferent to the order: the partials sorted within a row give other bits somewhere)
    by_size = np.concatenate([np.sort(row_seg[ptr[r]:ptr[r + 1]])[np.argsort(-np.abs(partial[np.sort(row_seg[ptr[r]:ptr[r + 1]])]), kind="stable")]
                              for r in range(len(ptr) - 1)])
    assert not np.array_equal(chain(by_size, ptr, partial).view(np.int32), want.view(np.int32))


def test_the_small_walks_meet_every_shape():
    seen = set()
    for plan in PLANS:
        row_seg, ptr = _plan_arrays(*plan)
        n_rows = len(ptr) - 1
        for rb, cap in WALKS:
            blocks, straddle = block_shapes(ptr, rb, cap)
            assert sum(b[0] for b in blocks) == n_rows and sum(b[1] for b in blocks) == len(row_seg)
            if blocks[0][0] == rb and len(blocks) > 1:
                seen.add("a full block")
            if n_rows % rb:
                seen.add("a range that is no multiple of the block")
            if blocks[-1][0] == 1 and rb > 1:
                seen.add("a last block of one row")
            if max(b[2] for b in blocks) >= 2:
                seen.add("a block of several tiles")
            if straddle:
                seen.add("a row over a tile edge")
            if (np.diff(ptr) > 2 * cap).any():
                seen.add("a row over three tiles")
            if any(b[1] % cap == 0 for b in blocks) or any(b[1] < cap for b in blocks):
                seen.add("a last tile that is short or exactly full")
    assert seen == {"a full block", "a range that is no multiple of the block", "a last block of one row", "a block of several tiles",
                    "a row over a tile edge", "a row over three tiles", "a last tile that is short or exactly full"}, seen


def test_a_last_block_of_one_row_and_a_range_that_ends_on_a_block():
    row_seg, ptr = _plan_arrays(*PLANS[0])
    n_rows = len(ptr) - 1
    partial = _partials(np.random.default_rng(2), len(row_seg))
    want = chain(row_seg, ptr, partial)
    for rb in (n_rows - 1, n_rows, n_rows + 1, (n_rows - 1) // 2):
        blocks, _ = block_shapes(ptr, rb, 64)
        assert blocks[-1][0] == (n_rows - 1) % rb + 1
        y, reads = tile_walk(row_seg, ptr, partial, rb, 64)
        assert np.array_equal(y.view(np.int32), want.view(np.int32)) and (reads == 1).all()
    assert block_shapes(ptr, n_rows - 1, 64)[0][-1][0] == 1 and block_shapes(ptr, (n_rows - 1) // 2, 64)[0][-1][0] in (1, 2)


def test_two_planted_errors_are_seen():
    row_seg, ptr = _plan_arrays(*PLANS[1])
    partial = _partials(np.random.default_rng(5), len(row_seg))
    want = chain(row_seg, ptr, partial)
    rb, cap = 16, 64
    _, straddle = block_shapes(ptr, rb, cap)
    assert straddle
    y, _ = tile_walk(row_seg, ptr, partial, rb, cap, carry_sum=False)
    differ = np.nonzero(y.view(np.int32) != want.view(np.int32))[0]
    assert len(differ) and set(differ.tolist()) <= set(straddle)          # only rows over a tile edge can lose their sum
    y, reads = tile_walk(row_seg, ptr, partial, rb, cap, stage_shift=1)
    assert (reads == 1).all() and int((y.view(np.int32) != want.view(np.int32)).sum()) > len(want) // 2


def test_the_module_constants_are_the_kernels():
    src = os.path.join(os.path.dirname(os.path.abspath(aggregate.__file__)), "csrc", "spmm_stream.hip")
    with open(src) as f:
        text = f.read()
    rows = re.search(r"constexpr int kCombineRows = (\d+);", text)
    cap = re.search(r"constexpr int kCombineCap = (\d+);", text)
    assert rows and cap
    assert (int(rows.group(1)), int(cap.group(1))) == SHIPPED
    assert 1 <= SHIPPED[0] <= THREADS and SHIPPED[1] % THREADS == 0 and SHIPPED[1] * 4 <= 64 * 1024
