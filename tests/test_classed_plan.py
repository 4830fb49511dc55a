"""CPU tests of the classed hub plan (HopGraph.classed_hub_plan, gnan_spmm_args.cls_*): the framework route — the reference the
GPU suite holds the library kernels to (tests/test_gpu_classed_hubs.py) — against a plain numpy restatement, array by array."""
import numpy as np
import pytest
import torch

import gnan_amd  # noqa: F401
from gnan_amd import HopGraph
from gnan_amd import graph as G


def _csr(n, rng, hubs, one_class=(), few_classes=()):
    deg = rng.poisson(4, n)
    for r, d in hubs:
        deg[r] = d
    rowptr = np.zeros(n + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(deg)
    col = rng.integers(0, n, int(rowptr[-1])).astype(np.int32)
    for r in one_class:                                     # every pair of the row in class 5
        seg = col[rowptr[r]:rowptr[r + 1]]
        col[rowptr[r]:rowptr[r + 1]] = (seg & ~7) | 5
    for r in few_classes:                                   # classes 0 and 3 only: six empty classes
        seg = col[rowptr[r]:rowptr[r + 1]]
        col[rowptr[r]:rowptr[r + 1]] = (seg & ~7) | np.where(seg & 1, 3, 0)
    col = np.minimum(col, n - 1)
    code = rng.integers(0, 3, int(rowptr[-1])).astype(np.uint8)
    return rowptr, col, code


def _restated(rowptr, col, code, rows, row_ids, se):
    """The plan as gnan_hip.h states it, one (slot, class) at a time."""
    index, starts, slice_row, slice_ptr, queues = [], [], [], [0], [[] for _ in range(8)]
    for r, q in enumerate(rows):
        i = row_ids[q] if row_ids is not None else q
        seg = np.arange(rowptr[i], rowptr[i + 1])
        for g in range(8):
            e = seg[(col[seg] & 7) == g]                     # CSR order within the class
            for j in range(0, len(e), se):
                queues[g].append(len(starts))
                starts.append(len(index) + j)
                slice_row.append(r)
            index.extend(int(col[k]) | (int(code[k]) << 29) for k in e)
        slice_ptr.append(len(starts))
    starts.append(len(index))
    longest = max(len(qu) for qu in queues)
    slot = np.full(8 * longest, -1, dtype=np.int64)
    for g in range(8):
        for e, s in enumerate(queues[g]):
            slot[8 * e + g] = s
    index = np.array(index, dtype=np.int64)
    index = np.where(index >= 1 << 31, index - (1 << 32), index)
    return index, np.array(starts), np.array(slice_row), np.array(slice_ptr), slot


@pytest.mark.parametrize("idx_dtype", [torch.int64, torch.int32])
@pytest.mark.parametrize("order", [False, True])
@pytest.mark.parametrize("se", [64, 2048])
def test_classed_plan_equals_the_restatement(idx_dtype, order, se):
    rng = np.random.default_rng(se + (idx_dtype == torch.int32) + 2 * order)
    n = 3000
    # a row of > 100 slices at se = 64, one of a single class, one with six empty classes, one just over the threshold
    hubs = [(7, 9000), (100, 700), (2000, 1300), (2999, 513), (1500, 512)]
    rowptr, col, code = _csr(n, rng, hubs, one_class=[100], few_classes=[2000])
    g = HopGraph.from_csr(torch.from_numpy(rowptr).to(idx_dtype), torch.from_numpy(col), torch.from_numpy(code), n_cols=n, n_codes=3)
    row_ids = torch.from_numpy(rng.permutation(n).astype(np.int32)) if order else None
    plan = g.classed_hub_plan(row_ids, 512, se)
    assert isinstance(plan, G.ClassedHubPlan) and plan.threshold == 512 and plan.slice_edges == se
    base = g.long_row_plan(row_ids, 512)
    assert torch.equal(plan.rows, base.rows) and plan.n_long == 4                 # the same hub slots (512 pairs is not a hub row)
    rows = plan.rows.long().numpy()
    index, starts, slice_row, slice_ptr, slot = _restated(rowptr, col, code, rows, row_ids.numpy() if order else None, se)
    assert plan.index.dtype == torch.int32 and np.array_equal(plan.index.long().numpy(), index)
    assert plan.slice_start.dtype == torch.int64 and np.array_equal(plan.slice_start.numpy(), starts)
    assert np.array_equal(plan.slice_row.long().numpy(), slice_row) and np.array_equal(plan.slice_ptr.long().numpy(), slice_ptr)
    assert plan.n_slices == len(slice_row) and plan.n_slots == len(slot) and np.array_equal(plan.slot_slice.long().numpy(), slot)
    assert plan.n_slots % 8 == 0 and (slot == -1).any() == (plan.n_slots > plan.n_slices)        # padding where queues differ
    if se == 64:
        r7 = int(np.nonzero(rows == (int(np.nonzero(row_ids.numpy() == 7)[0][0]) if order else 7))[0][0])
        assert slice_ptr[r7 + 1] - slice_ptr[r7] > 100
    # every slice holds one class, and slot b & 7 is that class
    cls = (plan.index.long() & 7).numpy()
    for b, s in enumerate(slot):
        if s >= 0:
            assert (cls[starts[s]:starts[s + 1]] == b % 8).all() and starts[s + 1] > starts[s]


def test_classed_plan_is_cached_and_declines_what_the_entries_cannot_hold():
    rng = np.random.default_rng(3)
    rowptr, col, code = _csr(1000, rng, [(4, 600)])
    g = HopGraph.from_csr(torch.from_numpy(rowptr), torch.from_numpy(col), torch.from_numpy(code), n_cols=1000, n_codes=3)
    assert g.classed_hub_plan() is g.classed_hub_plan() and g.classed_hub_plan(None, 256) is not g.classed_hub_plan()
    plain = g.classed_hub_plan(None, 5000)                                   # no hub rows: the plain (empty) plan
    assert plain.n_long == 0 and not isinstance(plain, G.ClassedHubPlan)
    wide = HopGraph.from_csr(torch.from_numpy(rowptr), torch.from_numpy(col), torch.from_numpy(code), n_cols=1000, n_codes=9)
    assert wide.classed_hub_plan() is None


def test_only_wide_forward_calls_of_large_graphs_take_the_classed_plan(monkeypatch):
    """The gate of aggregate.spmm_launch, read from the arguments it hands the library (a recording stand-in of gnan_spmm_fwd)."""
    from gnan_amd import _lib, aggregate
    rng = np.random.default_rng(5)
    n = 2000
    rowptr, col, code = _csr(n, rng, [(4, 900), (9, 1500)])
    g = HopGraph.from_csr(torch.from_numpy(rowptr), torch.from_numpy(col), torch.from_numpy(code), n_cols=n, n_codes=3)
    seen = []

    class Lib:
        def gnan_spmm_fwd_workspace_bytes(self, a):
            return 0

        def gnan_spmm_fwd(self, a, st):
            seen.append((a.cls_index is not None, a.cls_n_slots, a.n_long))
            return 0

    monkeypatch.setattr(_lib, "lib", lambda: Lib())
    monkeypatch.setattr(_lib, "require_device", lambda *t: None)
    monkeypatch.setattr(_lib, "stream_of", lambda t: 0)
    monkeypatch.setattr(aggregate, "CLASSED_MIN_NNZ", 1)
    monkeypatch.setattr(aggregate, "DEGREE_SORTED_COPY_MIN_ROWS", 1 << 30)        # (the CPU route of the sorted copy is not the point)
    lut = torch.tensor([[0.5], [0.25], [0.1]])
    for W, dtype in ((32, torch.float32), (16, torch.float32), (64, torch.bfloat16), (32, torch.bfloat16)):
        aggregate.spmm_launch(g, torch.zeros(n, W, dtype=dtype), lut, True, True, s_total=torch.zeros(W))
    aggregate.spmm_launch(g, torch.zeros(n, 64), lut, True, False, weight_by_col=True)
    monkeypatch.setattr(aggregate, "XCD_CLASSED_HUBS", False)
    aggregate.spmm_launch(g, torch.zeros(n, 64), lut, True, True, s_total=torch.zeros(64))
    assert [s[0] for s in seen] == [True, False, True, False, False, False]
    assert all(s[2] == 2 for s in seen) and seen[0][1] > 0 and seen[0][1] % 8 == 0
