"""The lone rows' part of the launch query (``gnan_spmm_args.lone_rows``, the ``lone`` fields of ``gnan_spmm_fwd_describe``), host only:
what spmm_lone_kernel takes is reported beside an unchanged tile partition on the self_sum route, is zero everywhere else, and the flag
is refused without ``self_sum``.  The query reads no device memory and starts no GPU work, so every pointer here is host memory."""
import numpy as np
import pytest
import torch

import rowwise
from test_rowwise_bound import _cpu_graph

ZERO = {"n_lone_rows": 0, "n_lone_blocks": 0, "n_tile_blocks_skipped": 0}


def _args(g, S, lut, lone, self_parts=1, lmax=4, reduce_cr=1):
    """aggregate.spmm_launch's record for a wide call over the degree-sorted copy (tests/test_rowwise_bound.py's _describe), with the
    self term and the flag as spmm_launch sets them.  Returns the record and what it points to."""
    from gnan_amd import _lib, aggregate
    copy, order, plan = g.degree_sorted_copy()
    out = torch.empty((g.n_rows, reduce_cr or S.shape[1]), dtype=torch.float32)
    s_total = S.float().sum(0)
    a = aggregate._spmm_args(copy, S, lut, True, s_total, out, order, False, plan=plan, reduce_cr=reduce_cr, scatter_out=2, packed=True)
    runs = copy.short_row_runs(lmax)
    if a.packed_index:
        a.short_lmax, a.short_row, a.short_pair = runs.lmax, runs.row_ptr, runs.pair_ptr
    self_sum = torch.zeros((max(self_parts, 1), g.n_rows))
    if self_parts:
        a.self_sum, a.self_parts = _lib.ptr(self_sum), self_parts
    a.lone_rows = int(lone)
    return a, (copy, order, plan, out, s_total, runs, self_sum)


def _query(a):
    from gnan_amd import _lib
    info = _lib.SpmmLaunchInfo()
    rc = _lib.lib().gnan_spmm_fwd_describe(a, info)
    return rc, info.as_dict()


def _graph(n=6000, D=3, seed=1):
    rng = np.random.default_rng(seed)
    rowptr, col, code = rowwise.short_csr(n, rng, D, self_share=0.0)
    return _cpu_graph(rowptr, col, code, n, D), np.diff(rowptr)


@pytest.mark.parametrize("W", [40, 64, 128, 256])
def test_on_the_route_the_old_fields_stay_and_the_new_ones_count_run_0(W):
    g, deg = _graph()
    S, lut = torch.zeros((g.n_rows, W)), torch.ones((3, 1))
    a_on, keep_on = _args(g, S, lut, True)
    a_off, keep_off = _args(g, S, lut, False)
    (rc_on, on), (rc_off, off) = _query(a_on), _query(a_off)
    assert rc_on == rc_off == 0
    assert on == off                                                        # n_tiles, n_tile_blocks, row_q0, short_tile[], the variant ...
    lpr = rowwise.lanes_per_row(W)
    n_tiles, q0, first = rowwise.tile_partition(deg, lpr, 4)
    assert (on["n_tiles"], on["row_q0"], on["short_tile"][:5], on["n_tile_blocks"]) == (n_tiles, q0, first, -(-n_tiles // 4))
    n_lone = int((deg == 0).sum())
    assert n_lone > 256 and first[1] == -(-n_lone // (8 * (64 // lpr)))
    assert off.lone == ZERO
    assert on.lone == {"n_lone_rows": n_lone, "n_lone_blocks": -(-n_lone // 256),
                       "n_tile_blocks_skipped": on["n_tile_blocks"] - -(-(n_tiles - first[1]) // 4)}
    assert on.lone["n_tile_blocks_skipped"] >= first[1] // 4 > 0


def test_a_graph_without_a_lone_row_reports_none():
    rng = np.random.default_rng(2)
    n = 2000
    rowptr, col, code = rowwise.csr_of_degrees(rng.integers(1, 8, n), n, rng, 3)
    g = _cpu_graph(rowptr, col, code, n, 3)
    a, keep = _args(g, torch.zeros((n, 64)), torch.ones((3, 1)), True)
    rc, info = _query(a)
    assert rc == 0 and info["n_tiles"] > 0 and info["short_tile"][1] == 0 and info.lone == ZERO


def test_off_the_route_the_new_fields_are_zero():
    from gnan_amd import _lib
    g, deg = _graph()
    n = g.n_rows
    lut = torch.ones((3, 1))
    # no self_sum (spmm_launch sets no flag then), fp32 rows of 64 floats: tiles, no lone kernel
    a, keep = _args(g, torch.zeros((n, 64)), lut, False, self_parts=0)
    rc, info = _query(a)
    assert rc == 0 and info["n_tiles"] > 0 and info.lone == ZERO
    # bf16 rows and W = 32 take no tiles at all, hence no lone rows either; with self_sum both are refused before any partition
    for S in (torch.zeros((n, 64), dtype=torch.bfloat16), torch.zeros((n, 32))):
        a, keep = _args(g, S, lut, False, self_parts=0)
        rc, info = _query(a)
        assert rc == 0 and info["n_tiles"] == 0 and info.lone == ZERO
        a, keep = _args(g, S, lut, True)
        assert _query(a)[0] == _lib.ERR_UNSUPPORTED
    # all W columns stored (no fused read-out): the self term has no route
    a, keep = _args(g, torch.zeros((n, 64)), lut, True, reduce_cr=0)
    assert _query(a)[0] == _lib.ERR_UNSUPPORTED
    # a dense graph: row blocks alone
    code = torch.ones((40, 40), dtype=torch.uint8)
    S, out, tot, ones = torch.zeros((40, 64)), torch.empty((40, 1)), torch.zeros(64), torch.ones((3, 1))
    d = _lib.SpmmArgs(n_rows=40, n_cols=40, code=_lib.ptr(code), S=_lib.ptr(S), W=64, s_stride=64, lut=_lib.ptr(ones), D=3, Cw=1,
                      s_total=_lib.ptr(tot), reduce_cr=1, Y=_lib.ptr(out), y_stride=1)
    rc, info = _query(d)
    assert rc == 0 and info["dense"] == 1 and info["n_tiles"] == 0 and info.lone == ZERO


def test_the_flag_is_refused_without_self_sum():
    from gnan_amd import _lib
    g, deg = _graph()
    a, keep = _args(g, torch.zeros((g.n_rows, 64)), torch.ones((3, 1)), True, self_parts=0)
    rc, info = _query(a)
    assert rc == _lib.ERR_BAD_ARG and b"lone_rows" in _lib.lib().gnan_last_error()
    assert _lib.lib().gnan_spmm_fwd(a, None) == _lib.ERR_BAD_ARG             # (validated on the host, before any HIP call)


def test_spmm_launch_sets_the_flag_on_the_route_only(monkeypatch):
    """aggregate.spmm_launch: the flag where self_sum is given, the runs are declared and LONE_ROWS is on (the launch itself needs a GPU:
    the record is caught at the query, which a stand-in answers)."""
    from gnan_amd import _lib, aggregate
    seen = []

    class Caught(Exception):
        pass

    class Lib:
        def __getattr__(self, name):
            return getattr(real, name)

        def gnan_spmm_fwd_describe(self, a, info):
            seen.append((a.lone_rows, a.short_lmax, bool(a.self_sum)))
            raise Caught

    real = _lib.lib()
    g, deg = _graph()
    n = g.n_rows
    monkeypatch.setattr(aggregate, "DEGREE_SORTED_COPY_MIN_ROWS", 1)
    monkeypatch.setattr(_lib, "require_device", lambda *t: None)
    monkeypatch.setattr(_lib, "lib", lambda: Lib())
    S, lut, tot = torch.zeros((n, 64)), torch.ones((3, 1)), torch.zeros(64)
    for lone, tiles, self_sum, want in ((True, True, torch.zeros((1, n)), (1, 4, True)), (False, True, torch.zeros((1, n)), (0, 4, True)),
                                        (True, False, torch.zeros((1, n)), (0, 0, True)), (True, True, None, (0, 4, False))):
        monkeypatch.setattr(aggregate, "LONE_ROWS", lone)
        monkeypatch.setattr(aggregate, "SHORT_ROW_TILES", tiles)
        with pytest.raises(Caught):
            aggregate.spmm_launch(g, S, lut, True, True, s_total=tot, reduce_cr=1, self_sum=self_sum, describe=[])
        assert seen[-1] == want
