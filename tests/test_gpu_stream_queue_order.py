"""The pair stream's partials in QUEUE order on the GPU (``gnan_spmm_args.stream_row_seg``; spmm_stream_kernel keeps the float of a round's
``kr``-th finished segment in lane ``kr`` and stores a round's floats with one instruction at ``partial[seg0 + k + sub]``;
spmm_stream_combine_kernel reads a row's floats through ``row_seg``).  Through the real route, the gates lowered as
tests/test_gpu_pair_stream.py lowers them, on that file's graph of 2 504 nodes, blocks of 4 operand rows.

Exact inputs (tests/test_stream_queue_order.py asserts on the CPU that they are exact in ANY association): S[j, f] =
((31 j + 7 f) mod 17) - 8, the look-up table (4, -2, 1), no count normalisation.  The expected output is computed in int64 and compared
BIT FOR BIT on every row — stream rows, hub rows, tiled rows and walked rows: a misplaced, dropped or doubled partial is a wrong
number, not a rounding.  Every case runs twice (same bits) and once with ``PAIR_STREAM = False`` (the same expected bits).

The shapes the store rule must meet are asserted from the plan each case takes: a round in which all 16 entries end a segment, a
row whose run is cut by a chunk edge, a class whose queue is empty, a class whose last chunk is short, the last segment of the last
class ending the index, rows of exactly ``min_pairs`` and of exactly 512 pairs beside a 513-pair hub row and a 4-pair tiled row; chunks
of 16, 32 and 64 entries are one, two and four rounds; W = 48 leaves column lanes idle, W = 64 / 128 / 256 are 16 / 32 / 64 lanes."""
import numpy as np
import pytest
import torch

import rowwise
from test_gpu_kernels import _graph
from test_gpu_pair_stream import LENGTHS, N, _check_describe, _csr, _kinds, _launch, _lower, _parts, _stream_plan
from test_stream_queue_order import EXACT_LUT, IW, exact_expected, exact_operand

pytestmark = pytest.mark.gpu
DEV = "cuda"
LAST = 1 << 31


def _check_shapes(plan, rowptr, min_pairs, chunk):
    idx = plan.index.cpu().long().numpy() & 0xFFFFFFFF
    flag = (idx & LAST) != 0
    pp, cp = plan.cls_pair_ptr.cpu().numpy(), plan.cls_chunk_ptr.cpu().numpy()
    first = np.concatenate([plan.chunk_first_seg.cpu().numpy(), [plan.n_seg]])
    row_seg, ptr = plan.row_seg.cpu().numpy(), plan.row_slot_ptr.cpu().numpy()
    assert sorted(row_seg.tolist()) == list(range(plan.n_seg))
    seg_row = np.empty(plan.n_seg, dtype=np.int64)
    seg_row[row_seg] = np.repeat(np.arange(plan.q_hi - plan.q_lo), np.diff(ptr))           # (queue order)
    n_cls = np.diff(pp)
    full_round = cut = short_last = False
    for c in range(8):
        for g in range(cp[c + 1] - cp[c]):
            lo = pp[c] + g * chunk
            n = min(chunk, pp[c + 1] - lo)
            short_last |= n < chunk
            for base in range(0, n - IW + 1, IW):
                full_round |= bool(flag[lo + base:lo + base + IW].all())
            t = cp[c] + g
            if g + 1 < cp[c + 1] - cp[c] and seg_row[first[t + 1] - 1] == seg_row[first[t + 1]]:
                cut = True
    assert full_round, "a round in which all 16 entries end a segment"
    assert cut, "a row whose run is cut by a chunk edge"
    assert (n_cls == 0).any() and short_last, "a class whose queue is empty, a class whose last chunk is short"
    assert flag[-1] and int(first[-1]) == plan.n_seg and int(flag.sum()) == plan.n_seg      # the last segment of the last class
    assert np.diff(first).max() > IW or chunk == IW                                         # more segments in a chunk than one round stores
    twin = np.diff(rowptr) - 1
    _, stream = _kinds(rowptr, min_pairs)
    assert stream[[r for r in LENGTHS if LENGTHS[r] in (min_pairs, 512)]].all() and (twin[stream] == min_pairs).any()
    assert (twin == 513).any() and (twin == 4).any() and not stream[twin == 513].any() and not stream[twin == 4].any()
    assert plan.q_hi - plan.q_lo == int(stream.sum())


# (W, parts, min_pairs, ranked blocks, chunk): every W with every lane count, every chunk size, 1 / 2 / 4 blocks
CASES = [(48, 1, 5, 1, 16), (48, 1, 9, 2, 64), (64, 2, 5, 2, 32), (64, 1, 5, 4, 16), (64, 1, 9, 1, 64), (128, 1, 5, 4, 32),
         (128, 2, 9, 2, 16), (256, 2, 5, 2, 64), (256, 1, 9, 1, 32), (256, 1, 5, 4, 16)]


@pytest.mark.parametrize("W,parts,min_pairs,n_blocks,chunk", CASES)
def test_every_row_is_bitwise_the_integer_result(W, parts, min_pairs, n_blocks, chunk, monkeypatch):
    from gnan_amd import functional as Fn
    _lower(monkeypatch, W, min_pairs, n_blocks, chunk)
    D = 3
    rowptr, col, code = _csr(D)
    g = _graph(rowptr, col, code, N, D)
    plan = _stream_plan(g, min_pairs, n_blocks, chunk)
    assert plan is not None and plan.chunk_pairs == chunk and plan.n_blocks == n_blocks
    _check_shapes(plan, rowptr, min_pairs, chunk)
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
    assert d_on[0]["lpr"] == rowwise.lanes_per_row(W) == {48: 16, 64: 16, 128: 32, 256: 64}[W]
    y, again, off = y.cpu(), again.cpu(), off.cpu()
    wrong = torch.nonzero((y != want).flatten()).flatten().tolist()
    assert not wrong, f"rows {wrong[:8]} of {len(wrong)}: got {y.flatten()[wrong[:8]].tolist()}, want {want.flatten()[wrong[:8]].tolist()}"
    assert torch.equal(y.view(torch.int32), want.view(torch.int32))
    assert torch.equal(again.view(torch.int32), y.view(torch.int32))
    assert torch.equal(off.view(torch.int32), want.view(torch.int32))
