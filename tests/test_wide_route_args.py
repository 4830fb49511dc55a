"""CPU tests of what aggregate.spmm_launch hands the library on the reference-order inference route, read from a
recording stand-in of gnan_spmm_fwd (as tests/test_pair_stream_plan.py's): which gnan_spmm_args field every plan array lands in, the
truth table of the route's gate, what the blocked hubs leave of the slice plan, and that a second call builds nothing.  The tables
below are written out by hand: FIELDS from include/gnan_hip.h, GATE from the behaviour recorded before the plans bound themselves
(profiles/r20_wide_plans_args.txt).  Degree-sorted graphs of 700 rows, one hop code, W = 64 unless a case says otherwise."""
import ctypes

import numpy as np
import pytest
import torch

import gnan_amd  # noqa: F401
from gnan_amd import HopGraph, _lib, aggregate, wide_plans
from gnan_amd import graph as G

N = 700
LENGTHS = (5, 5, 6, 16, 17, 31, 32, 33, 100, 511, 512, 512, 513, 700)


def _sorted_csr(rng, n, lengths=LENGTHS):
    """Rows shortest first: empty and short rows, rows of 5 .. 40 pairs, the named lengths; a skewed column draw, hop code 1."""
    deg = np.sort(np.concatenate([np.zeros(3, dtype=np.int64), rng.integers(1, 5, n // 3), rng.integers(5, 41, n - 3 - n // 3 - len(lengths)),
                                  np.asarray(lengths, dtype=np.int64)]), kind="stable")
    rowptr = np.zeros(n + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(deg)
    col = np.minimum((n * rng.random(int(rowptr[-1])) ** 3).astype(np.int64), n - 1).astype(np.int32)
    return deg, rowptr, col, np.ones(int(rowptr[-1]), dtype=np.uint8)


def _graph(rowptr, col, code):
    return HopGraph.from_csr(torch.from_numpy(rowptr), torch.from_numpy(col), torch.from_numpy(code), n_cols=N, n_codes=3)


MIN_NNZ = ("CLASSED_MIN_NNZ", "CLASSED_ROWS_MIN_NNZ", "BLOCKED_HUBS_MIN_NNZ", "PAIR_STREAM_MIN_NNZ")

# gnan_spmm_args field -> attribute of the plan that owns it
FIELDS = {
    "stream": {"stream_index": "index", "stream_cls_pair_ptr": "cls_pair_ptr", "stream_cls_chunk_ptr": "cls_chunk_ptr",
               "stream_chunk_first_seg": "chunk_first_seg", "stream_row_seg": "row_seg", "stream_row_slot_ptr": "row_slot_ptr",
               "stream_q_lo": "q_lo", "stream_q_hi": "q_hi", "stream_chunk": "chunk_pairs", "stream_code": "code", "n_stream_seg": "n_seg",
               "stream_max_chunks_per_class": "max_chunks_per_class"},
    "rows": {"seg_index": "index", "seg_start": "seg_start", "seg_row": "seg_row", "cls_seg_ptr": "cls_seg_ptr", "seg_mask": "mask",
             "seg_q_lo": "q_lo", "seg_q_hi": "q_hi", "n_seg": "n_seg", "seg_max_per_class": "max_per_class"},
    "hubs": {"hub_index": "index", "hub_seg_start": "seg_start", "hub_seg_row": "seg_row", "hub_seg_slot": "seg_slot",
             "hub_row_slot_ptr": "row_slot_ptr", "hub_cls_seg_ptr": "cls_seg_ptr", "hub_q_lo": "q_lo", "n_hub": "n_hub", "n_hub_seg": "n_seg",
             "hub_seg_max_per_class": "max_per_class"},
    "slices": {"cls_index": "index", "cls_slice_start": "slice_start", "cls_slice_row": "slice_row", "cls_slot_slice": "slot_slice",
               "cls_n_slots": "n_slots", "long_rows": "rows", "long_slice_ptr": "slice_ptr", "n_long": "n_long", "n_slices": "n_slices",
               "slice_edges": "slice_edges", "long_threshold": "threshold"},
}
FIRST = {"stream": "stream_index", "rows": "seg_index", "hubs": "hub_index", "slices": "cls_index"}


class Recorder:
    """gnan_spmm_fwd's stand-in: keeps every field of the argument struct of every call."""

    def __init__(self):
        self.calls = []

    def gnan_spmm_fwd_workspace_bytes(self, a):
        return 0

    def gnan_spmm_fwd(self, a, st):
        self.calls.append({name: getattr(a, name) for name, _ in a._fields_})
        return 0

    def bound(self, k=-1):
        """(stream, classed rows, hubs, classed hub slices) of call ``k``."""
        return tuple(self.calls[k][FIRST[f]] is not None for f in ("stream", "rows", "hubs", "slices"))


@pytest.fixture
def route(monkeypatch):
    """The recording library, every size gate lowered, and one graph's launch with the route's arguments as defaults."""
    rec = Recorder()
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    monkeypatch.setattr(_lib, "require_device", lambda *t: None)
    monkeypatch.setattr(_lib, "stream_of", lambda t: 0)
    monkeypatch.setattr(aggregate, "DEGREE_SORTED_COPY_MIN_ROWS", 1)
    monkeypatch.setattr(G, "SORTED_COPY_IN_HIP", False)
    for name in MIN_NNZ:
        monkeypatch.setattr(aggregate, name, 1)
    deg, rowptr, col, code = _sorted_csr(np.random.default_rng(5), N)
    lut = torch.tensor([[0.5], [0.25], [0.1]])

    def launch(g=None, W=64, dtype=torch.float32, with_rest=True, **kw):
        kw = {"reduce_cr": 1, "self_sum": torch.zeros(2, N), **kw}
        aggregate.spmm_launch(rec.g if g is None else g, torch.zeros(N, W, dtype=dtype), lut, True, with_rest,
                              s_total=torch.zeros(W) if with_rest else None, **kw)
        return rec.calls[-1]

    rec.g, rec.launch, rec.csr = _graph(rowptr, col, code), launch, (deg, rowptr, col, code)
    return rec


def _plans(g, W=64):
    """The four plans of the route as the graph's sorted copy caches them: the calls spmm_launch makes, argument for argument."""
    copy = g.degree_sorted_copy()[0]
    block_rows = max(1, aggregate.BLOCKED_HUB_BLOCK_BYTES // (W * 4))
    first_row = aggregate.SHORT_ROW_LMAX + 1
    return {"stream": copy.pair_stream_plan(max(aggregate.PAIR_STREAM_MIN_PAIRS, first_row), block_rows, aggregate.PAIR_STREAM_BLOCKS,
                                            aggregate.PAIR_STREAM_CHUNK_PAIRS),
            "rows": copy.classed_row_plan(max(aggregate.CLASSED_ROWS_MIN_PAIRS, first_row)),
            "hubs": copy.blocked_hub_plan(block_rows, aggregate.BLOCKED_HUB_BLOCKS, aggregate.BLOCKED_HUB_SEG_PAIRS),
            "slices": copy.classed_hub_plan(None)}


def test_the_table_names_every_field_of_the_four_plan_families():
    declared = {name for name, _ in _lib.SpmmArgs._fields_
                if name.startswith(("cls_", "seg_", "hub_", "stream_")) or name in ("n_seg", "n_hub", "n_hub_seg", "n_stream_seg")}
    named = {f for fam in FIELDS.values() for f in fam}
    assert declared - named == {"stream_seg_slot"} and len(named) == sum(len(fam) for fam in FIELDS.values())


def test_every_plan_array_lands_in_its_field(route, monkeypatch):
    first = route.launch()                                                   # the stream and the hubs
    monkeypatch.setattr(aggregate, "PAIR_STREAM", False)
    monkeypatch.setattr(aggregate, "BLOCKED_HUBS", False)
    second = route.launch()                                                  # the classed rows and the classed hub slices
    assert route.bound(0) == (True, False, True, False) and route.bound(1) == (False, True, False, True)
    plans = _plans(route.g)
    assert isinstance(plans["stream"], G.PairStreamPlan) and isinstance(plans["rows"], G.ClassedRowPlan)
    assert isinstance(plans["hubs"], G.BlockedHubPlan) and isinstance(plans["slices"], G.ClassedHubPlan)
    types = dict(_lib.SpmmArgs._fields_)
    for family, call in (("stream", first), ("hubs", first), ("rows", second), ("slices", second)):
        for fld, attr in FIELDS[family].items():
            want = getattr(plans[family], attr)
            if types[fld] is ctypes.c_void_p:
                assert isinstance(want, torch.Tensor) and want.numel() > 0 and call[fld] == _lib.ptr(want), (family, fld)
            else:
                assert isinstance(want, int) and call[fld] == want, (family, fld)
    assert first["stream_seg_slot"] is None and second["stream_seg_slot"] is None


# (stream, classed rows, hubs, classed hub slices) with ONE condition of the route flipped
ROUTE = (True, False, True, False)
GATE = [
    ("no self_sum", dict(self_sum=None), {}, (False, False, False, True)),
    ("reduce_cr = 0", dict(reduce_cr=0), {}, (False, False, False, True)),
    ("bf16 rows", dict(dtype=torch.bfloat16), {}, (False, False, False, True)),
    ("W = 32", dict(W=32), {}, (False, True, True, False)),
    ("W = 512", dict(W=512), {}, (False, True, True, False)),
    ("s_total absent", dict(with_rest=False), {}, (False, False, False, True)),
    ("two hop codes in the range", dict(g="two"), {}, (False, True, True, False)),
    ("no hub row", dict(g="no hub"), {}, (True, False, False, False)),
    ("PAIR_STREAM off", {}, dict(PAIR_STREAM=False), (False, True, True, False)),
    ("CLASSED_ROWS off", {}, dict(CLASSED_ROWS=False), (True, False, True, False)),
    ("BLOCKED_HUBS off", {}, dict(BLOCKED_HUBS=False), (True, False, False, True)),
    ("XCD_CLASSED_HUBS off", {}, dict(XCD_CLASSED_HUBS=False), (True, False, True, False)),
    ("PAIR_STREAM_MIN_NNZ above the graph", {}, dict(PAIR_STREAM_MIN_NNZ=1 << 24), (False, True, True, False)),
    ("CLASSED_ROWS_MIN_NNZ above the graph", {}, dict(CLASSED_ROWS_MIN_NNZ=1 << 24), (True, False, True, False)),
    ("BLOCKED_HUBS_MIN_NNZ above the graph", {}, dict(BLOCKED_HUBS_MIN_NNZ=1 << 24), (True, False, False, True)),
    ("CLASSED_MIN_NNZ above the graph", {}, dict(CLASSED_MIN_NNZ=1 << 24), (True, False, True, False)),
]


@pytest.mark.parametrize("label,call,switches,want", GATE, ids=[c[0] for c in GATE])
def test_one_condition_flipped(route, monkeypatch, label, call, switches, want):
    deg, rowptr, col, code = route.csr
    if call.get("g") == "two":
        two = code.copy()
        two[rowptr[int(np.nonzero(deg >= 5)[0][0])]] = 0                      # one pair of the range under another code
        call = dict(call, g=_graph(rowptr, col, two))
    elif call.get("g") == "no hub":
        d2, rp2, c2, k2 = _sorted_csr(np.random.default_rng(6), N, lengths=(5, 5, 6, 16, 17, 31, 32, 33, 100, 300, 400, 511, 512, 512))
        assert d2.max() == 512
        call = dict(call, g=_graph(rp2, c2, k2))
    route.launch()
    assert route.bound() == ROUTE, "the route binds the stream and the hubs"
    for name, value in switches.items():
        monkeypatch.setattr(aggregate, name, value)
    route.launch(**call)
    assert route.bound() == want, label


def test_the_bound_hubs_leave_no_slice_plan(route):
    a = route.launch()
    assert route.bound() == ROUTE
    assert a["n_long"] == a["n_slices"] == a["cls_n_slots"] == 0
    assert all(a[f] is None for f in ("long_rows", "long_slice_ptr", "cls_index", "cls_slice_start", "cls_slice_row", "cls_slot_slice"))
    assert a["long_threshold"] == G.LONG_ROW_THRESHOLD == 512
    assert _plans(route.g)["slices"].n_long == a["n_hub"] == 2                # (the slice plan exists: the launch took the hubs out of it)


def test_a_second_call_builds_nothing(route, monkeypatch):
    built = []
    for name in ("long_row_plan", "classed_hub_plan", "classed_row_plan", "blocked_hub_plan", "pair_stream_plan"):
        real = getattr(wide_plans, name)
        monkeypatch.setattr(wide_plans, name, lambda *a, _real=real, _name=name, **kw: (built.append(_name), _real(*a, **kw))[1])
    a = route.launch()
    assert {"pair_stream_plan", "blocked_hub_plan"} <= set(built)
    before = _plans(route.g)
    del built[:]
    b = route.launch()
    assert built == []
    after = _plans(route.g)
    assert all(after[k] is before[k] for k in before)
    plan_fields = [f for fam in FIELDS.values() for f in fam]
    assert all(a[f] == b[f] for f in plan_fields)
