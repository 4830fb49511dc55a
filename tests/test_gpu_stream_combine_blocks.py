"""The pair stream's combine by row blocks on the GPU (spmm_stream_combine_kernel in csrc/spmm_stream.hip: a workgroup per
``PAIR_STREAM_COMBINE_ROWS`` consecutive stream rows, their range of ``row_seg`` staged through an LDS tile of ``PAIR_STREAM_COMBINE_CAP``
entries, a thread per row adding from the tile).  Through the real route, the gates lowered as tests/test_gpu_pair_stream.py lowers them.

A graph of its own, 2 400 nodes and about 70 000 pairs, so that two row blocks and a third of one row come about: 513 stream rows
(= 1 mod 256 and mod 128) — one of exactly ``min_pairs`` = 5 pairs, 210 of 5 .. 9, 300 of 180 .. 220, one of 511 and, last of the sorted
copy's stream rows, one of exactly 512 whose pairs all fall in class 5 — beside tiled rows of 0 .. 4 pairs and two hub rows (513, 700).
The long rows draw half their pairs from 128 often listed columns (16 per class: with 4 ranked blocks of 4 operand rows every (class,
block) cell is met) and list no column of class 7, so a long row has about 35 segments and the second block's 256 rows well over two
tiles' worth.  Asserted from the plan each case takes, before the launch: a block of full ``ROWS`` rows, a last block of a single row, a
block of more than ``CAP`` entries (two tiles or more), a row whose entries straddle a tile edge, rows of exactly 512 and exactly
``min_pairs`` pairs, a block in which some class has no segment while the block before it has one.

Exact inputs (tests/test_stream_queue_order.py: exact in ANY association): S[j, f] = ((31 j + 7 f) mod 17) - 8, the look-up table
(4, -2, 1), no count normalisation.  The expected rows are computed in int64 and compared BIT FOR BIT on every row; every case runs
twice (same bits) and once with ``PAIR_STREAM = False`` (the same expected bits)."""
import numpy as np
import pytest
import torch

import rowwise
from test_gpu_kernels import _graph
from test_gpu_pair_stream import _check_describe, _launch, _lower, _parts, _stream_plan
from test_self_free_plan import self_graph
from test_stream_combine_blocks import block_shapes
from test_stream_queue_order import EXACT_LUT, exact_expected, exact_operand

pytestmark = pytest.mark.gpu
DEV = "cuda"
N = 2400
MIN_PAIRS = 5
N_BLOCKS = 4                    # ranked blocks (of test_gpu_pair_stream.BLOCK_ROWS = 4 operand rows)
N_LONG, N_SHORT = 300, 210
ALL_CLASS5 = 512                # the row of this many pairs lists class 5 only

_CSR = {}


def _csr():
    if not _CSR:
        rng = np.random.default_rng(27)
        lengths = np.concatenate([[MIN_PAIRS], rng.integers(5, 10, N_SHORT), rng.integers(180, 221, N_LONG), [511, 512, 513, 700]])
        lengths = np.concatenate([lengths, rng.integers(0, 5, N - len(lengths))])
        lengths = lengths[rng.permutation(N)]
        pool = np.concatenate([np.tile(np.arange(8, 136), 20), np.arange(N)])
        rowptr, col, code = self_graph(rng, N, N, "middle", lengths, 3, listed_cols=pool)
        row = np.repeat(np.arange(N), np.diff(rowptr))
        twin = col != row
        stream = (lengths >= MIN_PAIRS) & (lengths <= 512)
        move = twin & stream[row] & ((col & 7) == 7)          # no stream row lists a column of class 7 ...
        col[move] -= 1
        col[move & (col == row)] -= 8
        one = twin & (lengths[row] == ALL_CLASS5)             # ... and the 512-pair row lists class 5 alone
        col[one] = (col[one] & ~7) | 5
        col[one & (col == row)] += 8
        assert col.min() >= 0 and col.max() < N and (np.bincount(row[col == row], minlength=N) == 1).all()
        assert np.array_equal(np.bincount(row[col != row], minlength=N), lengths) and len(col) <= 100_000
        _CSR["csr"] = (rowptr, col, code, lengths)
    return _CSR["csr"]


def _check_shapes(plan, lengths, chunk):
    """Every shape of the tile walk, read from the plan the launch takes and the kernel's own constants."""
    from gnan_amd import aggregate
    rb, cap = aggregate.PAIR_STREAM_COMBINE_ROWS, aggregate.PAIR_STREAM_COMBINE_CAP
    ptr, row_seg = plan.row_slot_ptr.cpu().numpy().astype(np.int64), plan.row_seg.cpu().numpy().astype(np.int64)
    n_rows = plan.q_hi - plan.q_lo
    assert n_rows == int(((lengths >= MIN_PAIRS) & (lengths <= 512)).sum()) == 2 + N_SHORT + N_LONG + 1 and n_rows % rb == 1 and n_rows > rb
    assert len(ptr) == n_rows + 1 and ptr[-1] == plan.n_seg == len(row_seg) and sorted(row_seg.tolist()) == list(range(plan.n_seg))
    blocks, straddle = block_shapes(ptr, rb, cap)
    assert blocks[0][0] == rb, "a block of full rows"
    assert blocks[-1][0] == 1 and len(blocks) >= 2, "a last block of a single row"
    assert max(b[1] for b in blocks) > cap and max(b[2] for b in blocks) >= 2, "a block of more entries than a tile holds"
    assert straddle, "a row whose entries straddle a tile edge"
    # the sorted copy's stream rows are shortest first: the first has min_pairs pairs, the last 512
    srt = np.sort(lengths[(lengths >= MIN_PAIRS) & (lengths <= 512)])
    assert srt[0] == MIN_PAIRS and srt[-1] == 512 and srt[-2] == 511
    pairs = np.zeros(n_rows, dtype=np.int64)                  # pairs per stream row, counted from the plan's own index
    idx = plan.index.cpu().long().numpy() & 0xFFFFFFFF
    pp, cp = plan.cls_pair_ptr.cpu().numpy(), plan.cls_chunk_ptr.cpu().numpy()
    first = np.concatenate([plan.chunk_first_seg.cpu().numpy(), [plan.n_seg]])
    seg_row = np.empty(plan.n_seg, dtype=np.int64)
    seg_row[row_seg] = np.repeat(np.arange(n_rows), np.diff(ptr))
    seg_cls = np.repeat(np.arange(8), [int(first[cp[c + 1]] - first[cp[c]]) for c in range(8)])
    seg_of_entry = np.concatenate([[0], np.cumsum((idx & (1 << 31)) != 0)[:-1]])
    np.add.at(pairs, seg_row[seg_of_entry], 1)
    assert np.array_equal(pairs, srt), "rows of exactly min_pairs and exactly 512 pairs, every row's pairs in the stream"
    # a block in which some class has no segment: the last block (the class-5 row) against the block before it
    block_of_seg = seg_row // rb
    cls_in = [set(seg_cls[block_of_seg == b].tolist()) for b in range(len(blocks))]
    assert cls_in[-1] == {5} and {0, 1, 2, 3, 4, 5, 6} <= cls_in[-2] and all(7 not in s for s in cls_in)
    assert plan.chunk_pairs == chunk and plan.n_blocks == N_BLOCKS


# (W, parts, chunk)
CASES = [(64, 1, 16), (64, 2, 32), (256, 2, 16), (256, 1, 32)]


@pytest.mark.parametrize("W,parts,chunk", CASES)
def test_every_row_of_every_block_is_bitwise_the_integer_result(W, parts, chunk, monkeypatch):
    from gnan_amd import functional as Fn
    _lower(monkeypatch, W, MIN_PAIRS, N_BLOCKS, chunk)
    D = 3
    rowptr, col, code, lengths = _csr()
    g = _graph(rowptr, col, code, N, D)
    plan = _stream_plan(g, MIN_PAIRS, N_BLOCKS, chunk)
    assert plan is not None
    _check_shapes(plan, lengths, chunk)
    Sn = exact_operand(N, W)
    S = torch.from_numpy(Sn)
    lut = torch.tensor(EXACT_LUT).view(D, 1).to(DEV)
    Sd = S.to(DEV)
    s_total = Fn.column_sums(Sd)
    assert np.array_equal(s_total.cpu().numpy().astype(np.float64), Sn.astype(np.float64).sum(0))
    t, a = exact_expected(rowptr, col, code, Sn, s_total.cpu().numpy())
    assert int(a.max()) < 2 ** 24
    want = t.double().float()
    assert torch.equal(want.double(), t.double())
    self_sum = _parts(S, parts).to(DEV)
    d_on, d_off = [], []
    y = _launch(monkeypatch, g, Sd, lut, False, s_total, self_sum, True, d_on)
    again = _launch(monkeypatch, g, Sd, lut, False, s_total, self_sum, True)
    off = _launch(monkeypatch, g, Sd, lut, False, s_total, self_sum, False, d_off)
    torch.cuda.synchronize()
    _check_describe(d_on[0], d_off[0], plan, W)
    assert d_on[0]["lpr"] == rowwise.lanes_per_row(W)
    y, again, off = y.cpu(), again.cpu(), off.cpu()
    wrong = torch.nonzero((y != want).flatten()).flatten().tolist()
    assert not wrong, f"rows {wrong[:8]} of {len(wrong)}: got {y.flatten()[wrong[:8]].tolist()}, want {want.flatten()[wrong[:8]].tolist()}"
    assert torch.equal(y.view(torch.int32), want.view(torch.int32))
    assert torch.equal(again.view(torch.int32), y.view(torch.int32))
    assert torch.equal(off.view(torch.int32), want.view(torch.int32))
