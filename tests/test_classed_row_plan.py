"""CPU tests of the classed row plan (HopGraph.classed_row_plan, gnan_spmm_args.seg_*): the framework route against a plain numpy
restatement, array by array, and the gate of aggregate.spmm_launch.  The plan is taken on a degree-sorted copy (rows shortest first),
so the graphs here are built sorted."""
import numpy as np
import pytest
import torch

import gnan_amd  # noqa: F401
from gnan_amd import HopGraph
from gnan_amd import graph as G

N_COLS = 4096


def _sorted_csr(rng, min_pairs, extra=()):
    """Rows shortest first: empty rows, rows of 1 .. 40 pairs, of exactly min_pairs - 1 and min_pairs, 512 and 513 pairs, hub rows; a
    row whose pairs all fall in class 5, one with exactly one pair in every class, one that lists column 77 three times."""
    deg = np.concatenate([np.zeros(7, dtype=np.int64), rng.integers(1, 41, 300), [min_pairs - 1] * 3, [min_pairs] * 3, [8, 8, 8],
                          [512, 512, 513, 700, 2100], np.asarray(extra, dtype=np.int64)])
    deg = np.sort(deg, kind="stable")
    rowptr = np.zeros(len(deg) + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(deg)
    col = rng.integers(0, N_COLS, int(rowptr[-1])).astype(np.int32)
    code = rng.integers(0, 4, int(rowptr[-1])).astype(np.uint8)           # code 3 in the top bits: a negative int32 entry
    eights = np.nonzero(deg == 8)[0]
    special = {}
    if len(eights) >= 3:
        a, b, c = (int(v) for v in eights[:3])
        col[rowptr[a]:rowptr[a + 1]] = (col[rowptr[a]:rowptr[a + 1]] & ~7) | 5                         # one class
        col[rowptr[b]:rowptr[b + 1]] = (col[rowptr[b]:rowptr[b + 1]] & ~7) | rng.permutation(8)        # a pair in every class
        col[rowptr[c] + np.array([1, 4, 6])] = 77                                                     # one column three times
        special = {"one": a, "each": b, "thrice": c}
    return deg, rowptr, col, code, special


def _restated(rowptr, col, code, min_pairs, max_pairs=512):
    """The plan as gnan_hip.h states it: class by class, row by row, pair by pair."""
    deg = np.diff(rowptr)
    rows = [q for q in range(len(deg)) if min_pairs <= deg[q] <= max_pairs]
    if not rows:
        return None
    q_lo, q_hi = rows[0], rows[-1] + 1
    assert rows == list(range(q_lo, q_hi))
    index, start, seg_row, ptr = [], [], [], [0]
    mask = np.zeros(q_hi - q_lo, dtype=np.int64)
    for c in range(8):
        for q in rows:
            e = [k for k in range(rowptr[q], rowptr[q + 1]) if (col[k] & 7) == c]
            if e:
                start.append(len(index))
                seg_row.append(q)
                mask[q - q_lo] |= 1 << c
                index.extend(int(col[k]) | (int(code[k]) << 29) for k in e)
        ptr.append(len(seg_row))
    start.append(len(index))
    index = np.array(index, dtype=np.int64)
    index = np.where(index >= 1 << 31, index - (1 << 32), index)
    return q_lo, q_hi, index, np.array(start), np.array(seg_row), np.array(ptr), mask


def _graph(rowptr, col, code, idx_dtype=torch.int64, packed=True):
    g = HopGraph.from_csr(torch.from_numpy(rowptr).to(idx_dtype), torch.from_numpy(col), torch.from_numpy(code), n_cols=N_COLS, n_codes=4)
    if packed:
        g.colp = g._packed_index()
    return g


@pytest.mark.parametrize("idx_dtype", [torch.int64, torch.int32])
@pytest.mark.parametrize("packed", [True, False])
@pytest.mark.parametrize("min_pairs", [5, 17])
def test_classed_row_plan_equals_the_restatement(min_pairs, packed, idx_dtype):
    rng = np.random.default_rng(min_pairs + 2 * packed)
    deg, rowptr, col, code, special = _sorted_csr(rng, min_pairs)
    plan = _graph(rowptr, col, code, idx_dtype, packed).classed_row_plan(min_pairs)
    q_lo, q_hi, index, start, seg_row, ptr, mask = _restated(rowptr, col, code, min_pairs)
    assert isinstance(plan, G.ClassedRowPlan) and (plan.q_lo, plan.q_hi, plan.min_pairs) == (q_lo, q_hi, min_pairs)
    # the range: from the first row of min_pairs pairs (the rows of min_pairs - 1 stay out) through the last of 512 (513 stays out)
    assert deg[q_lo] == min_pairs and deg[q_lo - 1] == min_pairs - 1 and deg[q_hi - 1] == 512 and deg[q_hi] == 513
    assert plan.index.dtype == torch.int32 and np.array_equal(plan.index.long().numpy(), index)
    assert plan.seg_start.dtype == torch.int64 and np.array_equal(plan.seg_start.numpy(), start)
    assert plan.seg_row.dtype == torch.int32 and np.array_equal(plan.seg_row.long().numpy(), seg_row)
    assert plan.cls_seg_ptr.dtype == torch.int32 and np.array_equal(plan.cls_seg_ptr.long().numpy(), ptr)
    assert plan.mask.dtype == torch.uint8 and np.array_equal(plan.mask.long().numpy(), mask)
    assert plan.n_seg == len(seg_row) and plan.max_per_class == int(np.diff(ptr).max())
    # every pair of every classed row exactly once, in its class, in the row's order, under its row
    cols, codes = index & ((1 << 29) - 1), (index >> 29) & 7
    seen = {}
    for s in range(plan.n_seg):
        c = int(np.searchsorted(ptr, s, side="right")) - 1
        assert start[s + 1] > start[s] and ((cols[start[s]:start[s + 1]] & 7) == c).all()
        seen.setdefault(int(seg_row[s]), {})[c] = (cols[start[s]:start[s + 1]], codes[start[s]:start[s + 1]])
    assert sorted(seen) == list(range(q_lo, q_hi))
    for q in range(q_lo, q_hi):
        rc, rd = col[rowptr[q]:rowptr[q + 1]], code[rowptr[q]:rowptr[q + 1]]
        assert sum(len(v[0]) for v in seen[q].values()) == len(rc)
        for c, (pc, pd) in seen[q].items():
            assert np.array_equal(pc, rc[(rc & 7) == c]) and np.array_equal(pd, rd[(rc & 7) == c])
        assert int(mask[q - q_lo]) == sum(1 << c for c in seen[q])
    if min_pairs <= 8:
        assert int(mask[special["one"] - q_lo]) == 1 << 5 and int(mask[special["each"] - q_lo]) == 255
        q = special["thrice"]
        s = [k for k in range(plan.n_seg) if seg_row[k] == q and ptr[77 & 7] <= k < ptr[(77 & 7) + 1]][0]
        assert int((cols[start[s]:start[s + 1]] == 77).sum()) == 3


def test_no_classed_row_no_plan_and_the_plan_is_cached():
    rng = np.random.default_rng(1)
    deg = np.sort(np.concatenate([np.zeros(5, dtype=np.int64), rng.integers(1, 5, 200), [513, 600]]), kind="stable")
    rowptr = np.zeros(len(deg) + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(deg)
    col = rng.integers(0, N_COLS, int(rowptr[-1])).astype(np.int32)
    code = rng.integers(0, 3, int(rowptr[-1])).astype(np.uint8)
    g = _graph(rowptr, col, code)
    assert _restated(rowptr, col, code, 5) is None and g.classed_row_plan(5) is None and g.classed_row_plan(17) is None
    assert g.classed_row_plan(4) is not None and g.classed_row_plan(4) is g.classed_row_plan(4)
    # rows that are not sorted by length: refused, the plan's ranges would be wrong
    bad = np.zeros(4, dtype=np.int64)
    bad[1:] = np.cumsum([6, 2, 7])
    gb = _graph(bad, col[:15], code[:15])
    with pytest.raises(ValueError):
        gb.classed_row_plan(5)


def test_only_the_self_term_route_of_large_graphs_takes_the_plan(monkeypatch):
    """The gate of aggregate.spmm_launch, read from the arguments it hands the library (a recording stand-in of gnan_spmm_fwd)."""
    from gnan_amd import _lib, aggregate
    rng = np.random.default_rng(5)
    _, rowptr, col, code, _ = _sorted_csr(rng, 5)
    n = len(rowptr) - 1
    col = np.minimum(col, n - 1)
    g = HopGraph.from_csr(torch.from_numpy(rowptr), torch.from_numpy(col), torch.from_numpy(code), n_cols=n, n_codes=4)
    seen = []

    class Lib:
        def gnan_spmm_fwd_workspace_bytes(self, a):
            return 0

        def gnan_spmm_fwd(self, a, st):
            seen.append((a.seg_index is not None, a.n_seg, a.seg_q_lo, a.seg_q_hi, a.seg_max_per_class))
            return 0

    monkeypatch.setattr(_lib, "lib", lambda: Lib())
    monkeypatch.setattr(_lib, "require_device", lambda *t: None)
    monkeypatch.setattr(_lib, "stream_of", lambda t: 0)
    monkeypatch.setattr(aggregate, "DEGREE_SORTED_COPY_MIN_ROWS", 1)
    monkeypatch.setattr(G, "SORTED_COPY_IN_HIP", False)
    monkeypatch.setattr(aggregate, "CLASSED_MIN_NNZ", 1)                       # (the hub plan's gate is not this route's)
    lut = torch.tensor([[0.5], [0.25], [0.1], [0.05]])
    S, tot, self_sum = torch.zeros(n, 64), torch.zeros(64), torch.zeros(2, n)
    aggregate.spmm_launch(g, S, lut, True, True, s_total=tot, reduce_cr=1, self_sum=self_sum)      # below CLASSED_ROWS_MIN_NNZ
    monkeypatch.setattr(aggregate, "CLASSED_ROWS_MIN_NNZ", 1)
    aggregate.spmm_launch(g, S, lut, True, True, s_total=tot, reduce_cr=1, self_sum=self_sum)      # the route
    aggregate.spmm_launch(g, S, lut, True, True, s_total=tot, reduce_cr=1)                         # no self term: generic forward
    aggregate.spmm_launch(g, S, lut, True, True, s_total=tot)                                      # all columns stored
    monkeypatch.setattr(aggregate, "CLASSED_ROWS", False)
    aggregate.spmm_launch(g, S, lut, True, True, s_total=tot, reduce_cr=1, self_sum=self_sum)      # switched off
    assert [s[0] for s in seen] == [False, True, False, False, False]
    copy = g.degree_sorted_copy()[0]
    plan = copy.classed_row_plan(aggregate.CLASSED_ROWS_MIN_PAIRS)
    assert seen[1][1:] == (plan.n_seg, plan.q_lo, plan.q_hi, plan.max_per_class) and plan.q_lo > 0
