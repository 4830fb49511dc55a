"""CPU tests of the blocked hub plan (HopGraph.blocked_hub_plan / column_blocks, gnan_spmm_args.hub_*): the framework route against a
plain numpy restatement, array by array; the plan's properties one named case each (``_verify``), with planted errors that must fail
the case they are named after; the gate of aggregate.spmm_launch.  The plan is taken on a degree-sorted copy (rows shortest first), so
the graphs here are built sorted.  Graphs of 300 .. 3000 nodes, blocks of 4 and 16 columns, 2 and 3 ranked blocks, pieces of 8 pairs."""
import numpy as np
import pytest
import torch

import gnan_amd  # noqa: F401
from gnan_amd import HopGraph
from gnan_amd import graph as G

CAP = 8
X_COL, Y_COL = 8 * 9 + 5, 8 * 11 + 6          # listed CAP and CAP + 1 times by the two rows that list nothing else of class 5 / class 6


def _sorted_csr(rng, n_cols, hubs=(513, 514, 700, 2100)):
    """Rows shortest first: empty rows, short rows, rows of 512 pairs (no hubs), then the hub rows.  The first hub row lists X_COL CAP
    times and no other column of class 5, the second Y_COL CAP + 1 times and no other column of class 6."""
    deg = np.sort(np.concatenate([np.zeros(3, dtype=np.int64), rng.integers(1, 41, n_cols - 5 - len(hubs)), [512, 512],
                                  np.asarray(hubs, dtype=np.int64)]), kind="stable")
    rowptr = np.zeros(len(deg) + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(deg)
    # a skewed column draw, so that the listing counts differ AND tie
    col = np.minimum((n_cols * rng.random(int(rowptr[-1])) ** 3).astype(np.int64), n_cols - 1).astype(np.int32)
    code = rng.integers(0, 4, int(rowptr[-1])).astype(np.uint8)           # code 3 in the top bits: a negative int32 entry
    first = [int(q) for q in np.nonzero(deg > 512)[0][:2]]
    for q, c, times in zip(first, (X_COL, Y_COL), (CAP, CAP + 1)):
        e = np.arange(rowptr[q], rowptr[q + 1])
        same = e[(col[e] & 7) == (c & 7)]
        col[same] ^= 1                                                    # (into the neighbouring class)
        col[e[3:3 + 2 * times:2]] = c
    return deg, rowptr, col, code, first


def _graph(rowptr, col, code, n_cols, idx_dtype=torch.int64, packed=True):
    g = HopGraph.from_csr(torch.from_numpy(rowptr).to(idx_dtype), torch.from_numpy(col), torch.from_numpy(code), n_cols=n_cols, n_codes=4)
    if packed:
        g.colp = g._packed_index()
    return g


def _blocks(col, n_cols, block_rows, n_blocks):
    """gnan_hip.h's ranking: inside class col & 7 by listing count, most listed first, ties by column id."""
    listed = np.bincount(col, minlength=n_cols)
    block = np.zeros(n_cols, dtype=np.int64)
    for c in range(8):
        ids = sorted(range(c, n_cols, 8), key=lambda j: (-listed[j], j))
        for rank, j in enumerate(ids):
            block[j] = min(rank // block_rows, n_blocks)
    return block


def _restated(rowptr, col, code, block, n_blocks, cap, threshold=512):
    """The plan as gnan_hip.h states it: class by class, block by block, row by row, piece by piece, pair by pair."""
    deg = np.diff(rowptr)
    rows = [q for q in range(len(deg)) if deg[q] > threshold]
    if not rows:
        return None
    q_lo = rows[0]
    assert rows == list(range(q_lo, len(deg)))
    index, start, seg_row, seg_key, ptr = [], [], [], [], [0]
    for c in range(8):
        for b in range(n_blocks + 1):
            for q in rows:
                e = [k for k in range(rowptr[q], rowptr[q + 1]) if (col[k] & 7) == c and block[col[k]] == b]
                for piece, k0 in enumerate(range(0, len(e), cap)):
                    start.append(len(index))
                    seg_row.append(q)
                    seg_key.append((q, c, b, piece))
                    index.extend(int(col[k]) | (int(code[k]) << 29) for k in e[k0:k0 + cap])
        ptr.append(len(seg_row))
    start.append(len(index))
    index = np.array(index, dtype=np.int64)
    index = np.where(index >= 1 << 31, index - (1 << 32), index)
    by_row = sorted(range(len(seg_key)), key=lambda s: seg_key[s])          # the row-major enumeration (row, class, block, piece)
    slot = np.empty(len(seg_key), dtype=np.int64)
    slot[by_row] = np.arange(len(seg_key))
    row_slot_ptr = np.concatenate([[0], np.cumsum(np.bincount(np.array(seg_row) - q_lo, minlength=len(rows)))])
    return dict(q_lo=q_lo, index=index, seg_start=np.array(start), seg_row=np.array(seg_row), seg_slot=slot, row_slot_ptr=row_slot_ptr,
                cls_seg_ptr=np.array(ptr))


def _arrays(plan):
    return dict(q_lo=plan.q_lo, index=plan.index.long().numpy().copy(), seg_start=plan.seg_start.numpy().copy(),
                seg_row=plan.seg_row.long().numpy().copy(), seg_slot=plan.seg_slot.long().numpy().copy(),
                row_slot_ptr=plan.row_slot_ptr.long().numpy().copy(), cls_seg_ptr=plan.cls_seg_ptr.long().numpy().copy())


def _segments(a):
    cols, codes = a["index"] & ((1 << 29) - 1), (a["index"] >> 29) & 7
    for s in range(len(a["seg_row"])):
        lo, hi = int(a["seg_start"][s]), int(a["seg_start"][s + 1])
        yield s, int(np.searchsorted(a["cls_seg_ptr"], s, side="right")) - 1, int(a["seg_row"][s]), cols[lo:hi], codes[lo:hi]


def _verify(a, rowptr, col, code, block, cap, S=None, w=None):
    """The properties of the plan, a named case each: the first that fails raises AssertionError(name)."""
    n_rows, q_lo = len(rowptr) - 1, a["q_lo"]
    n_seg = len(a["seg_row"])
    seen, last = {}, {}
    for s, c, q, cols, codes in _segments(a):
        assert len(cols) > 0 and q_lo <= q < n_rows and ((cols & 7) == c).all(), "a segment's pairs share row and class"
        assert len(set(block[cols].tolist())) == 1, "a segment's pairs share one block"
        assert len(cols) <= cap, "no segment exceeds the cap"
        b = int(block[cols[0]])
        assert last.get(c, (0, 0))[0] <= b, "queues are block-major"
        assert (b, q) >= last.get(c, (0, 0)), "queues are block-major, then by row"
        last[c] = (b, q)
        seen.setdefault(q, {}).setdefault((c, b), []).append((s, cols, codes))
    for q in range(q_lo, n_rows):
        rc, rd = col[rowptr[q]:rowptr[q + 1]], code[rowptr[q]:rowptr[q + 1]]
        got = seen.get(q, {})
        assert sum(len(p[1]) for run in got.values() for p in run) == len(rc), "every hub pair appears in exactly one segment"
        for (c, b), run in got.items():
            m = ((rc & 7) == c) & (block[rc] == b)
            assert np.array_equal(np.concatenate([p[1] for p in run]), rc[m]), "every hub pair appears in exactly one segment"
            assert np.array_equal(np.concatenate([p[2] for p in run]), rd[m]), "every hub pair appears in exactly one segment"
            assert [len(p[1]) for p in run] == [cap] * (int(m.sum()) // cap) + [int(m.sum()) % cap] * (int(m.sum()) % cap > 0), \
                "a run is cut into full pieces and one remainder"
    assert sorted(a["seg_slot"].tolist()) == list(range(n_seg)), "seg_slot is a permutation"
    ptr = a["row_slot_ptr"]
    assert ptr[0] == 0 and ptr[-1] == n_seg and len(ptr) == n_rows - q_lo + 1, "row ranges match row_slot_ptr"
    key = {}
    for s, c, q, cols, _ in _segments(a):
        assert ptr[q - q_lo] <= a["seg_slot"][s] < ptr[q - q_lo + 1], "row ranges match row_slot_ptr"
        key[int(a["seg_slot"][s])] = (q, c, int(block[cols[0]]), s)
    assert [key[t] for t in range(n_seg)] == sorted(key.values()), "slots are the row-major enumeration"
    if S is not None:
        # the aggregation in int64 through the plan — a partial per slot, a row's slots added — against the CSR's
        partial = np.zeros(n_seg, dtype=np.int64)
        for s, _, _, cols, codes in _segments(a):
            partial[a["seg_slot"][s]] = int((w[codes][:, None] * S[cols]).sum())
        for q in range(q_lo, n_rows):
            rc, rd = col[rowptr[q]:rowptr[q + 1]], code[rowptr[q]:rowptr[q + 1]]
            assert int(partial[ptr[q - q_lo]:ptr[q - q_lo + 1]].sum()) == int((w[rd][:, None] * S[rc]).sum()), \
                "the aggregation through the plan equals the CSR's"


CASES = [(300, 4, 2), (400, 16, 2), (1000, 4, 3), (3000, 16, 3)]


@pytest.mark.parametrize("n_cols,block_rows,n_blocks", CASES)
@pytest.mark.parametrize("packed,idx_dtype", [(True, torch.int64), (False, torch.int32)])
def test_blocked_hub_plan_equals_the_restatement(n_cols, block_rows, n_blocks, packed, idx_dtype):
    rng = np.random.default_rng(n_cols + block_rows)
    deg, rowptr, col, code, first = _sorted_csr(rng, n_cols)
    g = _graph(rowptr, col, code, n_cols, idx_dtype, packed)
    block = _blocks(col, n_cols, block_rows, n_blocks)
    assert np.array_equal(g.column_blocks(block_rows, n_blocks).numpy(), block)          # ties by column id
    listed = np.bincount(col, minlength=n_cols)[block < n_blocks]
    assert len(set(listed.tolist())) < len(listed)                                         # (there ARE ties among the ranked columns)
    plan = g.blocked_hub_plan(block_rows, n_blocks, CAP)
    want = _restated(rowptr, col, code, block, n_blocks, CAP)
    assert isinstance(plan, G.BlockedHubPlan) and plan.q_lo == want["q_lo"] and plan.n_hub == len(deg) - plan.q_lo == 4
    assert deg[plan.q_lo] == 513 and deg[plan.q_lo - 1] == 512
    assert (plan.index.dtype, plan.seg_start.dtype, plan.seg_row.dtype, plan.seg_slot.dtype, plan.row_slot_ptr.dtype,
            plan.cls_seg_ptr.dtype) == (torch.int32, torch.int64, torch.int32, torch.int32, torch.int32, torch.int32)
    got = _arrays(plan)
    for name, v in want.items():
        assert np.array_equal(got[name], v), name
    assert plan.n_seg == len(want["seg_row"]) and plan.max_per_class == int(np.diff(want["cls_seg_ptr"]).max())
    assert sum(plan.block_pairs) == len(want["index"]) == int(deg[plan.q_lo:].sum()) and sum(plan.block_segs) == plan.n_seg
    assert len(plan.block_pairs) == n_blocks + 1 and plan.block_pairs[0] > 0 and plan.block_pairs[n_blocks] > 0
    # the same plan twice (a fresh graph: nothing cached), and the cache on one graph
    again = _arrays(_graph(rowptr, col, code, n_cols, idx_dtype, packed).blocked_hub_plan(block_rows, n_blocks, CAP))
    assert all(np.array_equal(got[k], again[k]) for k in got)
    assert g.blocked_hub_plan(block_rows, n_blocks, CAP) is plan and g.blocked_hub_plan(block_rows, n_blocks, CAP + 1) is not plan
    # runs of CAP and CAP + 1 pairs: one piece, two pieces
    for q, c, pieces in ((first[0], X_COL, [CAP]), (first[1], Y_COL, [CAP, 1])):
        mine = [len(cols) for _, cl, row, cols, _ in _segments(got) if row == q and cl == (c & 7)]
        assert mine == pieces
    S = rng.integers(-4, 5, (n_cols, 3))
    _verify(got, rowptr, col, code, block, CAP, S, np.array([4, -2, 1, 3]))


def _planted(name):
    rng = np.random.default_rng(11)
    n_cols, block_rows, n_blocks = 600, 4, 3
    _, rowptr, col, code, _ = _sorted_csr(rng, n_cols)
    block = _blocks(col, n_cols, block_rows, n_blocks)
    a = _arrays(_graph(rowptr, col, code, n_cols).blocked_hub_plan(block_rows, n_blocks, CAP))
    S, w = rng.integers(-4, 5, (n_cols, 3)), np.array([4, -2, 1, 3])
    _verify(a, rowptr, col, code, block, CAP, S, w)                       # (sound before the error is planted)
    if name == "block key off by one":
        # the ranking cut one rank late: the first column of every block but the first belongs to the block before
        listed = np.bincount(col, minlength=n_cols)
        wrong = np.zeros(n_cols, dtype=np.int64)
        for c in range(8):
            ids = sorted(range(c, n_cols, 8), key=lambda j: (-listed[j], j))
            for rank, j in enumerate(ids):
                wrong[j] = min(max(rank - 1, 0) // block_rows, n_blocks)
        assert (wrong != block).any()
        a = _arrays(_restated_plan(rowptr, col, code, wrong, n_blocks))
    elif name == "a dropped last piece":
        # the pieces of a run counted with floor instead of ceil: the remainder of the last run is gone
        a["seg_start"], a["seg_row"], a["seg_slot"] = a["seg_start"][:-1].copy(), a["seg_row"][:-1], a["seg_slot"][:-1]
        a["cls_seg_ptr"] = np.minimum(a["cls_seg_ptr"], len(a["seg_row"]))
        a["seg_slot"] = np.argsort(np.argsort(a["seg_slot"]))
        a["row_slot_ptr"] = np.concatenate([[0], np.cumsum(np.bincount(a["seg_row"] - a["q_lo"], minlength=len(rowptr) - 1 - a["q_lo"]))])
    elif name == "slots in queue order":
        a["seg_slot"] = np.arange(len(a["seg_row"]))
    return a, rowptr, col, code, block, S, w


class _Plain:
    def __init__(self, d):
        self.q_lo = d["q_lo"]
        for k, v in d.items():
            if k != "q_lo":
                setattr(self, k, torch.from_numpy(np.asarray(v)))


def _restated_plan(rowptr, col, code, block, n_blocks):
    return _Plain(_restated(rowptr, col, code, block, n_blocks, CAP))


@pytest.mark.parametrize("name,case", [("block key off by one", "a segment's pairs share one block"),
                                       ("a dropped last piece", "every hub pair appears in exactly one segment"),
                                       ("slots in queue order", "row ranges match row_slot_ptr")])
def test_a_planted_error_fails_its_named_case(name, case):
    a, rowptr, col, code, block, S, w = _planted(name)
    with pytest.raises(AssertionError) as err:
        _verify(a, rowptr, col, code, block, CAP, S, w)
    assert str(err.value).startswith(case)


def test_no_hub_row_no_plan_and_unsorted_rows_are_refused():
    rng = np.random.default_rng(1)
    deg = np.sort(np.concatenate([np.zeros(5, dtype=np.int64), rng.integers(1, 5, 300), [511, 512]]), kind="stable")
    rowptr = np.zeros(len(deg) + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(deg)
    col = rng.integers(0, 307, int(rowptr[-1])).astype(np.int32)
    code = rng.integers(0, 3, int(rowptr[-1])).astype(np.uint8)
    g = _graph(rowptr, col, code, 307)
    assert g.blocked_hub_plan(4, 2, CAP) is None and g.blocked_hub_plan(4, 2, CAP) is None
    assert g.blocked_hub_plan(4, 2, CAP, threshold=511) is not None                      # (its own hub threshold: the row of 512)
    bad = np.zeros(4, dtype=np.int64)
    bad[1:] = np.cumsum([6, 2, 7])
    with pytest.raises(ValueError):
        _graph(bad, col[:15], code[:15], 307).blocked_hub_plan(4, 2, CAP, threshold=5)


def test_only_the_self_term_route_of_large_graphs_takes_the_plan(monkeypatch):
    """The gate of aggregate.spmm_launch, read from the arguments it hands the library (a recording stand-in of gnan_spmm_fwd)."""
    from gnan_amd import _lib, aggregate
    rng = np.random.default_rng(5)
    n = 700
    _, rowptr, col, code, _ = _sorted_csr(rng, n)
    g = HopGraph.from_csr(torch.from_numpy(rowptr), torch.from_numpy(col), torch.from_numpy(code), n_cols=n, n_codes=4)
    seen = []

    class Lib:
        def gnan_spmm_fwd_workspace_bytes(self, a):
            return 0

        def gnan_spmm_fwd(self, a, st):
            seen.append((a.hub_index is not None, a.n_long, a.n_slices, a.cls_index is not None, a.long_threshold, a.hub_q_lo, a.n_hub,
                         a.n_hub_seg, a.hub_seg_max_per_class, a.seg_index is not None))
            return 0

    monkeypatch.setattr(_lib, "lib", lambda: Lib())
    monkeypatch.setattr(_lib, "require_device", lambda *t: None)
    monkeypatch.setattr(_lib, "stream_of", lambda t: 0)
    monkeypatch.setattr(aggregate, "DEGREE_SORTED_COPY_MIN_ROWS", 1)
    monkeypatch.setattr(G, "SORTED_COPY_IN_HIP", False)
    monkeypatch.setattr(aggregate, "CLASSED_MIN_NNZ", 1)                       # (the older gates are not this route's)
    monkeypatch.setattr(aggregate, "CLASSED_ROWS_MIN_NNZ", 1)
    lut = torch.tensor([[0.5], [0.25], [0.1], [0.05]])
    S, tot, self_sum = torch.zeros(n, 64), torch.zeros(64), torch.zeros(2, n)
    aggregate.spmm_launch(g, S, lut, True, True, s_total=tot, reduce_cr=1, self_sum=self_sum)      # below BLOCKED_HUBS_MIN_NNZ
    monkeypatch.setattr(aggregate, "BLOCKED_HUBS_MIN_NNZ", 1)
    aggregate.spmm_launch(g, S, lut, True, True, s_total=tot, reduce_cr=1, self_sum=self_sum)      # the route
    aggregate.spmm_launch(g, S, lut, True, True, s_total=tot, reduce_cr=1)                         # no self term: generic forward
    aggregate.spmm_launch(g, S, lut, True, True, s_total=tot)                                      # all columns stored
    aggregate.spmm_launch(g, S.bfloat16(), lut, True, True, s_total=tot, reduce_cr=1, self_sum=self_sum)     # bf16 rows
    monkeypatch.setattr(aggregate, "BLOCKED_HUBS", False)
    aggregate.spmm_launch(g, S, lut, True, True, s_total=tot, reduce_cr=1, self_sum=self_sum)      # switched off
    assert [s[0] for s in seen] == [False, True, False, False, False, False]
    assert all(s[1] == 4 and s[2] > 0 and s[3] for k, s in enumerate(seen) if k != 1)              # the classed hub plan everywhere else
    copy = g.degree_sorted_copy()[0]
    plan = copy.blocked_hub_plan(aggregate.BLOCKED_HUB_BLOCK_BYTES // 256, aggregate.BLOCKED_HUB_BLOCKS, aggregate.BLOCKED_HUB_SEG_PAIRS)
    assert seen[1][1:] == (0, 0, False, 512, plan.q_lo, 4, plan.n_seg, plan.max_per_class, True) and plan.q_lo == n - 4
