"""CPU tests of the pair stream's partials in QUEUE order (``PairStreamPlan.row_seg``, ``gnan_spmm_args.stream_row_seg``;
spmm_stream_kernel and spmm_stream_combine_kernel in csrc/spmm_stream.hip).

Segment ``s`` of the plan's queue-order enumeration — class-major, inside a class by block, then by row, the enumeration
``chunk_first_seg`` counts in — stores its float at ``partial[s]``.  ``row_seg[row_slot_ptr[r] .. row_slot_ptr[r + 1])`` are the numbers of
row ``r``'s segments, ascending; it is the inverse of ``seg_slot``.  Checked here:

* ``row_seg`` against a restatement written from that sentence and the header's description of the queue, not from the builder: the
  queue is rebuilt pair by pair from the CSR, cut into chunks, its runs numbered, and every row's numbers collected.  Plan families of
  tests/test_pair_stream_plan.py (rows of 5, 16, 17, 31, 32, 33, 100, 511, 512 pairs beside shorter rows and hubs), chunks of 16 and 32
  entries, 1, 2 and 4 ranked blocks, packed and plain index.
* the kernel's store rule, lane by lane in numpy: within a 16-entry round lane ``kr`` of the lane group keeps the float of the round's
  ``kr``-th finished segment, and at the end of the round lanes ``sub < kr`` store ``partial[seg0 + k + sub]``.  Every ``partial[s]`` is
  written exactly once and holds the float the row-major layout held at ``seg_slot[s]``; the combine's chain over ``row_seg`` then gives
  the bits of tests/test_pair_stream_plan.py's emulation of the row-major layout.
* two planted errors — two ``row_seg`` entries of different rows swapped; ``k`` one short after a round — are both seen.
* the inputs of tests/test_gpu_stream_queue_order.py (defined here: ``exact_operand``, ``EXACT_LUT``) make its bit-for-bit comparison
  legitimate for ANY association: operand entries are integers of -8 .. 8, the weights the combine forms (4 - 1, -2 - 1, 1) are
  integers, so every product and every partial sum of any evaluation order is an integer whose magnitude the triangle inequality
  bounds by A_i = sum_f (|w_0| |S[i, f]| + |w_1| sum_j |S[j, f]| + |w_2| (sum_j |S[j, f]| + |S[i, f]| + |tot_f|)); A_i < 2^24 is asserted,
  and so is the float64 -> float32 -> float64 round trip of the result."""
import numpy as np
import pytest
import torch

import gnan_amd  # noqa: F401

import rowwise
from test_blocked_hub_plan import _blocks
from test_pair_stream_plan import LAST, PACK, _arrays, _graph, _sorted_csr, _weights, _with_self_pairs, emulate

f32 = np.float32
IW = 16                                         # index entries per round (spmm_stream_kernel)
EXACT_LUT = (4.0, -2.0, 1.0)                    # powers of two; the combine's folded weights 3, -3, 1 are integers


def exact_operand(n, W):
    """S[j, f] = ((31 j + 7 f) mod 17) - 8: integers of -8 .. 8 that differ along rows and columns."""
    j, f = np.arange(n, dtype=np.int64)[:, None], np.arange(W, dtype=np.int64)[None, :]
    return (((31 * j + 7 * f) % 17) - 8).astype(f32)


def exact_expected(rowptr, col, code, S, s_total):
    """(the row's fused read-out in int64, its magnitude A_i): ``rowwise.exact_scaled`` at scale 1 — integer weights."""
    t, a = rowwise.exact_scaled(rowptr, col, code, torch.from_numpy(S), torch.tensor(EXACT_LUT).view(3, 1), torch.from_numpy(s_total), 1,
                                None, 1)
    return t, a


# ------------------------------------------------------------------------------------------------- row_seg, restated
def _queue_segments(rowptr, col, block, n_blocks, min_pairs, chunk, max_pairs=512):
    """The queue as the header describes it, from the CSR alone: [(row, [columns])] of every segment, in queue order."""
    deg = np.diff(rowptr)
    rows = [q for q in range(len(deg)) if min_pairs <= deg[q] <= max_pairs]
    segs = []
    for c in range(8):
        queue = [(q, int(col[e])) for b in range(n_blocks + 1) for q in rows for e in range(rowptr[q], rowptr[q + 1])
                 if (col[e] & 7) == c and block[col[e]] == b]
        for j0 in range(0, len(queue), chunk):
            at = None
            for q, cc in queue[j0:j0 + chunk]:
                if q != at:                                                  # a maximal run of one row inside one chunk
                    segs.append((q, []))
                    at = q
                segs[-1][1].append(cc)
    return rows[0], rows[-1] + 1, segs


def _restated_row_seg(q_lo, q_hi, segs):
    """For row r, its segments' queue-order numbers, in queue order; the rows one after the other."""
    mine = {q: [] for q in range(q_lo, q_hi)}
    for s, (q, _) in enumerate(segs):
        mine[q].append(s)
    ptr = np.concatenate([[0], np.cumsum([len(mine[q]) for q in range(q_lo, q_hi)])])
    return np.array([s for q in range(q_lo, q_hi) for s in mine[q]], dtype=np.int64), ptr


def _plan_segments(a, chunk):
    """The columns of every segment as the plan's index lists them: entries up to and including a flagged one, chunk by chunk."""
    idx = a["index"] & 0xFFFFFFFF
    out = []
    for c in range(8):
        lo, hi = int(a["cls_pair_ptr"][c]), int(a["cls_pair_ptr"][c + 1])
        for g in range(int(a["cls_chunk_ptr"][c + 1] - a["cls_chunk_ptr"][c])):
            assert int(a["chunk_first_seg"][int(a["cls_chunk_ptr"][c]) + g]) == len(out), "chunk_first_seg counts in queue order"
            cur = []
            for e in idx[lo + g * chunk:min(hi, lo + (g + 1) * chunk)]:
                cur.append(int(e) & PACK)
                if int(e) & LAST:
                    out.append(cur)
                    cur = []
            assert not cur, "a chunk's last entry is flagged"
    return out


def _verify_row_seg(row_seg, a, segs, q_lo, q_hi, chunk):
    n_seg = len(segs)
    assert sorted(row_seg.tolist()) == list(range(n_seg)), "row_seg is a permutation"
    assert np.array_equal(a["seg_slot"][row_seg], np.arange(n_seg)) and np.array_equal(row_seg[a["seg_slot"]], np.arange(n_seg)), \
        "row_seg is the inverse of seg_slot"
    ptr = a["row_slot_ptr"]
    assert ptr[0] == 0 and ptr[-1] == n_seg and len(ptr) == q_hi - q_lo + 1
    listed = _plan_segments(a, chunk)
    assert len(listed) == n_seg and [cols for _, cols in segs] == listed
    for r in range(q_hi - q_lo):
        mine = row_seg[ptr[r]:ptr[r + 1]]
        assert (np.diff(mine) > 0).all(), "a row's entries ascend"
        assert mine.tolist() == [s for s in range(n_seg) if segs[s][0] == q_lo + r], "a row names exactly its segments"


FAMILIES = [(300, 4, 1, 5, 16), (300, 4, 2, 5, 32), (400, 16, 4, 9, 16), (350, 4, 4, 17, 32), (320, 16, 2, 33, 32)]


def _family(n, block_rows, n_blocks, min_pairs, chunk, packed=True, idx_dtype=torch.int64):
    rng = np.random.default_rng(n + chunk + n_blocks)
    deg, rowptr, col, code = _sorted_csr(rng, n)
    assert {5, 16, 17, 31, 32, 33, 100, 511, 512} <= set(deg.tolist())
    plan = _graph(rowptr, col, code, n, idx_dtype, packed).pair_stream_plan(min_pairs, block_rows, n_blocks, chunk)
    return deg, rowptr, col, code, _blocks(col, n, block_rows, n_blocks), plan


@pytest.mark.parametrize("n,block_rows,n_blocks,min_pairs,chunk", FAMILIES)
@pytest.mark.parametrize("packed,idx_dtype", [(True, torch.int64), (False, torch.int32)])
def test_row_seg_equals_the_restatement_and_inverts_seg_slot(n, block_rows, n_blocks, min_pairs, chunk, packed, idx_dtype):
    deg, rowptr, col, code, block, plan = _family(n, block_rows, n_blocks, min_pairs, chunk, packed, idx_dtype)
    assert plan.row_seg.dtype == torch.int32 and plan.seg_slot.dtype == torch.int32 and plan.row_seg.numel() == plan.n_seg
    q_lo, q_hi, segs = _queue_segments(rowptr, col, block, n_blocks, min_pairs, chunk)
    want, ptr = _restated_row_seg(q_lo, q_hi, segs)
    a = _arrays(plan)
    row_seg = plan.row_seg.long().numpy()
    assert (plan.q_lo, plan.q_hi, plan.n_seg) == (q_lo, q_hi, len(segs))
    assert np.array_equal(row_seg, want) and np.array_equal(a["row_slot_ptr"], ptr)
    _verify_row_seg(row_seg, a, segs, q_lo, q_hi, chunk)
    per_row = np.diff(ptr)
    assert per_row.min() >= 1 and per_row.max() > 8                     # (a row of 512 pairs spans many classes, blocks and chunks)


# ------------------------------------------------------------------------------------------------- the store rule, lane by lane
def _segment_floats(a, chunk, S, W):
    """The float of every segment in queue order: spmm_stream_kernel's arithmetic as tests/test_pair_stream_plan.py's emulation has it."""
    lpr = rowwise.lanes_per_row(W)
    Sp = np.zeros((S.shape[0], lpr * 4), dtype=f32)
    Sp[:, :W] = S
    out = []
    for cols in _plan_segments(a, chunk):
        acc = np.zeros((lpr, 4), dtype=f32)
        for cc in cols:
            acc = acc + Sp[cc].reshape(lpr, 4)
        r = (acc[:, 0] + acc[:, 1]) + (acc[:, 2] + acc[:, 3])
        off = 1
        while off < lpr:
            r = r + r[np.arange(lpr) ^ off]
            off *= 2
        assert (r == r[0]).all()                                         # the butterfly leaves the sum in every lane
        out.append(r[0])
    return np.array(out, dtype=f32)


def store_rule(a, chunk, value, k_short_after_round=False):
    """Lane groups over their chunks, 16 entries per round: (partial in queue order, writes per element).  ``value[s]`` is what the
    reduction of segment ``s`` leaves in every lane.  ``k_short_after_round``: the planted error, k advanced by one too few."""
    n_seg = len(value)
    partial, writes = np.full(n_seg, np.nan, dtype=f32), np.zeros(n_seg, dtype=np.int64)
    idx = a["index"] & 0xFFFFFFFF
    for c in range(8):
        lo, hi = int(a["cls_pair_ptr"][c]), int(a["cls_pair_ptr"][c + 1])
        t0 = int(a["cls_chunk_ptr"][c])
        for g in range(int(a["cls_chunk_ptr"][c + 1]) - t0):
            seg0 = int(a["chunk_first_seg"][t0 + g])
            n = min(chunk, hi - lo - g * chunk)
            k, done = 0, 0                                               # done: segments of the chunk finished (the truth; k: the kernel's)
            for base in range(0, n, IW):
                keep, kr = np.zeros(IW, dtype=f32), 0
                for j in range(base, min(n, base + IW)):
                    if int(idx[lo + g * chunk + j]) & LAST:
                        r = value[seg0 + done]
                        keep = np.where(np.arange(IW) == kr, r, keep)    # keep = (sub == kr) ? r : keep
                        kr += 1
                        done += 1
                for sub in range(IW):
                    if sub < kr and seg0 + k + sub < n_seg:
                        partial[seg0 + k + sub] = keep[sub]
                        writes[seg0 + k + sub] += 1
                k += kr - 1 if (k_short_after_round and kr > 0) else kr
    return partial, writes


def combine(a, row_seg, partial, weights, s_total, self_term):
    """spmm_stream_combine_kernel: a row's floats through row_seg in index order, then the weight, the rest and the self term."""
    T = f32(np.asarray(s_total, dtype=np.float64).sum())
    out = np.empty(a["q_hi"] - a["q_lo"], dtype=f32)
    for r in range(len(out)):
        y = f32(0)
        for s in range(int(a["row_slot_ptr"][r]), int(a["row_slot_ptr"][r + 1])):
            y = f32(y + partial[row_seg[s]])
        y = f32(weights[r, 0] * y)
        y = f32(np.float64(weights[r, 1]) * np.float64(T) + np.float64(y))
        out[r] = f32(np.float64(weights[r, 2]) * np.float64(self_term[r]) + np.float64(y))
    return out


def _operands(rng, n, W):
    S = rng.standard_normal((n, W)).astype(f32) * f32(2.0) ** rng.integers(-3, 4, (n, 1)).astype(f32)
    return S, rng.standard_normal((3, 1)).astype(f32), rng.integers(1, 9, (n, 3)).astype(np.int32)


@pytest.mark.parametrize("W,n_blocks,min_pairs,chunk", [(48, 2, 5, 16), (64, 4, 5, 32), (128, 1, 9, 64), (256, 2, 17, 32)])
def test_the_store_rule_fills_every_partial_once_with_the_row_major_layouts_float(W, n_blocks, min_pairs, chunk):
    n = 300
    deg, rowptr, col, code, block, plan = _family(n, 4, n_blocks, min_pairs, chunk)
    a, row_seg = _arrays(plan), plan.row_seg.long().numpy()
    rng = np.random.default_rng(W + chunk)
    S, lut, cnt = _operands(rng, n, W)
    value = _segment_floats(a, chunk, S, W)
    row_major = np.empty_like(value)
    row_major[a["seg_slot"]] = value                                     # the parent's layout: segment s at seg_slot[s]
    partial, writes = store_rule(a, chunk, value)
    assert (writes == 1).all(), "every partial[s] is written exactly once"
    assert np.array_equal(partial.view(np.int32), row_major[a["seg_slot"]].view(np.int32))
    # the shapes the rule must meet: a round that ends 16 segments (chunk 16: min_pairs 5), a chunk of more than one round with segment
    # ends in several of them, a segment that runs over a round's end
    first = np.concatenate([a["chunk_first_seg"], [plan.n_seg]])
    assert np.diff(first).max() >= (16 if min_pairs <= 5 and chunk <= 32 else 2)
    rows = np.arange(plan.q_lo, plan.q_hi)
    weights = _weights(lut, cnt, rows, plan.code)
    s_total = S.astype(np.float64).sum(0).astype(f32)
    self_term = S.astype(np.float64).sum(1).astype(f32)[rows]
    new = combine(a, row_seg, partial, weights, s_total, self_term)
    old = emulate(a, chunk, S, W, weights, s_total, self_term)          # the row-major layout's emulation, unchanged
    assert np.array_equal(new.view(np.int32), old.view(np.int32))


def test_two_planted_errors_are_seen():
    n, W, chunk, n_blocks, min_pairs = 300, 64, 32, 2, 5
    deg, rowptr, col, code, block, plan = _family(n, 4, n_blocks, min_pairs, chunk)
    a, row_seg = _arrays(plan), plan.row_seg.long().numpy()
    q_lo, q_hi, segs = _queue_segments(rowptr, col, block, n_blocks, min_pairs, chunk)
    _verify_row_seg(row_seg, a, segs, q_lo, q_hi, chunk)
    rng = np.random.default_rng(11)
    S, lut, cnt = _operands(rng, n, W)
    value = _segment_floats(a, chunk, S, W)
    rows = np.arange(plan.q_lo, plan.q_hi)
    weights = _weights(lut, cnt, rows, plan.code)
    s_total = S.astype(np.float64).sum(0).astype(f32)
    self_term = S.astype(np.float64).sum(1).astype(f32)[rows]
    old = emulate(a, chunk, S, W, weights, s_total, self_term)
    partial, writes = store_rule(a, chunk, value)
    assert np.array_equal(combine(a, row_seg, partial, weights, s_total, self_term).view(np.int32), old.view(np.int32))
    # 1: two entries of different rows swapped — the plan check sees it, and so do the two rows' sums
    ptr = a["row_slot_ptr"]
    i, j = int(ptr[3]), int(ptr[40])
    assert value[row_seg[i]] != value[row_seg[j]]
    bad = row_seg.copy()
    bad[i], bad[j] = row_seg[j], row_seg[i]
    with pytest.raises(AssertionError):
        _verify_row_seg(bad, a, segs, q_lo, q_hi, chunk)
    swapped = combine(a, bad, partial, weights, s_total, self_term)
    differ = np.nonzero(swapped.view(np.int32) != old.view(np.int32))[0]
    assert set(differ.tolist()) == {3, 40}
    # 2: k one short after a round that ended segments — in a chunk of two rounds the second round then overwrites the first's last
    # float and the chunk's last partial stays unwritten
    partial2, writes2 = store_rule(a, chunk, value, k_short_after_round=True)
    assert (writes2 == 0).any() and (writes2 > 1).any()
    assert not np.array_equal(partial2.view(np.int32), partial.view(np.int32))
    got = combine(a, row_seg, partial2, weights, s_total, self_term)
    assert not np.array_equal(got.view(np.int32), old.view(np.int32))


# ------------------------------------------------------------------------------------------------- the exact inputs of the GPU file
def exact_case_graph():
    """tests/test_gpu_pair_stream.py's graph of 2 504 nodes, one listed hop code (D = 3): (rowptr, col, code, N)."""
    import test_gpu_pair_stream as P
    return (*P._csr(3), P.N)


@pytest.mark.parametrize("W", [48, 64, 128, 256])
def test_the_exact_inputs_are_exact_in_any_association(W):
    rowptr, col, code, n = exact_case_graph()
    assert 2000 <= n <= 4000
    S = exact_operand(n, W)
    assert S.min() == -8 and S.max() == 8 and (S == np.round(S)).all()
    assert S[1, 0] == ((31 * 1 + 7 * 0) % 17) - 8 and S[5, 3] == ((31 * 5 + 7 * 3) % 17) - 8
    lut = np.array(EXACT_LUT, dtype=np.float64)
    assert all(float(np.log2(abs(v))).is_integer() for v in lut)                          # powers of two
    folded = np.array([lut[1] - lut[2], lut[2], lut[0] - lut[2]])                         # what the combine multiplies by
    assert (folded == np.round(folded)).all()
    s_total = S.astype(np.float64).sum(0)
    assert np.array_equal(s_total.astype(f32).astype(np.float64), s_total)               # (the column sums the GPU forms are exact too)
    t, a = exact_expected(rowptr, col, code, S, s_total.astype(f32))
    assert t.shape == (n, 1) and int(a.max()) < 2 ** 24, "every intermediate of any association is an integer below 2^24"
    # the folded form's own magnitude, term by term: |w_1 - w_2| sum |S_j| + |w_2| |T| + |w_0 - w_2| |self|
    row = np.repeat(np.arange(n), np.diff(rowptr))
    twin = col != row
    listed = np.zeros(n)
    np.add.at(listed, row[twin], np.abs(S).sum(1)[col[twin]])
    mag = abs(folded[0]) * listed + abs(folded[1]) * np.abs(s_total).sum() + abs(folded[2]) * np.abs(S).sum(1)
    assert mag.max() < 2 ** 24
    want = t.double()
    assert torch.equal(want.float().double(), want), "the float64 result survives the round trip through float32"
    assert int((t != 0).sum()) > n // 2 and len(np.unique(t.numpy())) > 64                 # (not a degenerate answer)
