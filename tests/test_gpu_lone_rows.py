"""The lone rows a thread each (``aggregate.LONE_ROWS``, ``gnan_spmm_args.lone_rows``; spmm_lone_kernel in csrc/spmm_lone.hip) and the
tiles' row epilogue on the self_sum route (``short_tile<.., SELF>`` in csrc/spmm_fwd_body.hpp): the rows of a degree-sorted twin that list
no pair leave the short-row tiles for a kernel of their own, and the tiles keep one channel sum, read ``s_total`` once and their self terms
ahead of the row loop.  Both must leave every row the bits of the plain row walk (``SHORT_ROW_TILES = False``: ``rows_body``).

Graphs of 3 000 to 6 000 rows without a self pair, called through ``aggregate.spmm_launch(..., reduce_cr=1, s_total=..., self_sum=...)``
with the degree-sorted copy's size gate at 1.  W in {40, 64, 128, 256} (lanes past W; 16, 32 and 64 lanes per row), D in {1, 2, 3, 4},
counts on and off, with and without the rest total, ``self_sum`` of one and of two parts, lone runs of 0, 1, 255, 256, 257 and a few
thousand rows (the workgroup's edge; no launch), and one graph whose rows with a pair are all stream or hub rows (the lone kernel beside
an empty tile range).  Exact-integer cases assert their own 2^24 bound."""
import numpy as np
import pytest
import torch

import rowwise
from test_gpu_kernels import _graph

pytestmark = pytest.mark.gpu
DEV = "cuda"
LONE_BLOCK = 256                        # rows per workgroup of spmm_lone_kernel (kLoneBlock)
_GRAPHS = {}


def _csr(n_lone, D, kind="mixed"):
    """``n_lone`` rows without a pair at random row ids; the others list 1 .. 9 or 30 pairs and two hubs 600 and 513 ('mixed'), or 5 .. 30
    pairs under the one code 1 and two hubs ('stream': no row of 1 .. 4 pairs).  No row lists itself; codes 0 .. D - 2."""
    key = (n_lone, D, kind)
    if key not in _GRAPHS:
        rng = np.random.default_rng(35 + 7 * n_lone + D)
        n = 3000 + n_lone
        if kind == "mixed":
            deg = rng.choice([1, 2, 3, 4, 5, 7, 9, 30], size=n, p=[.4, .15, .1, .1, .08, .07, .05, .05])
        else:
            deg = rng.integers(5, 31, n)
        lone = rng.permutation(n)[:n_lone]
        deg[lone] = 0
        hubs = np.setdiff1d(np.arange(n), lone)[[11, 1500]]
        deg[hubs] = 600, 513
        rowptr, col, code = rowwise.csr_of_degrees(deg, n, rng, D)
        if kind == "stream":
            code[:] = 1
        row = np.repeat(np.arange(n), deg)
        col[col == row] = (col[col == row] + 1) % n
        _GRAPHS[key] = (rowptr, col, code, n)
    return _GRAPHS[key]


def _self_sum(rng, n, parts, integer=False):
    a = rng.integers(-8, 9, (parts, n)).astype(np.float32) if integer else rng.standard_normal((parts, n)).astype(np.float32)
    return torch.from_numpy(a)


def _launch_one_code(g, S, lut, use_cnt, s_total, self_sum, describe):
    """D = 1 — the rest bucket alone, which ``HopGraph`` (two codes at least) and hence ``aggregate.spmm_launch`` cannot state: the record
    spmm_launch builds for the two-code graph ``g`` (every pair under code 0) with ``D`` set to 1 and a one-row table, handed to the library
    directly; the switches are read as spmm_launch reads them.  Every pair's code is then clamped to the rest code 0."""
    from gnan_amd import _lib, aggregate
    copy, order, plan = g.degree_sorted_copy()
    out = torch.empty((g.n_rows, 1), dtype=torch.float32, device=S.device)
    lut2 = torch.cat([lut, torch.full_like(lut, float("nan"))])                  # (row 1 is never read)
    a = aggregate._spmm_args(copy, S, lut2, use_cnt, s_total, out, order, False, plan=plan, reduce_cr=1, scatter_out=2, packed=True)
    a.D = 1
    runs = copy.short_row_runs(aggregate.SHORT_ROW_LMAX)
    if aggregate.SHORT_ROW_TILES and a.packed_index:
        a.short_lmax, a.short_row, a.short_pair = runs.lmax, runs.row_ptr, runs.pair_ptr
    a.self_sum, a.self_parts = _lib.ptr(self_sum), int(self_sum.shape[0])
    a.lone_rows = int(aggregate.LONE_ROWS and a.short_lmax > 0)
    need = _lib.lib().gnan_spmm_fwd_workspace_bytes(a)
    ws = torch.empty(max(need // 4, 1), dtype=torch.float32, device=S.device)
    a.workspace, a.workspace_bytes = _lib.ptr(ws), need
    info = _lib.SpmmLaunchInfo()
    _lib.check(_lib.lib().gnan_spmm_fwd_describe(a, info), "gnan_spmm_fwd_describe")
    describe.append(info.as_dict())
    _lib.check(_lib.lib().gnan_spmm_fwd(a, _lib.stream_of(S)), "gnan_spmm_fwd")
    torch.cuda.synchronize()                                                     # (ws, lut2 and runs live until the kernels are done)
    return out


def _three_launches(monkeypatch, g, S, lut, use_cnt, with_rest, s_total, self_sum, one_code=False):
    """(lone kernel on, lone kernel off, plain row walk) with the first two calls' launch queries."""
    from gnan_amd import aggregate
    out, info = {}, {}
    for name, lone, tiles in (("on", True, True), ("off", False, True), ("walk", False, False)):
        monkeypatch.setattr(aggregate, "LONE_ROWS", lone)
        monkeypatch.setattr(aggregate, "SHORT_ROW_TILES", tiles)
        d = []
        if one_code:
            out[name] = _launch_one_code(g, S, lut, use_cnt, s_total, self_sum, d)
        else:
            out[name] = aggregate.spmm_launch(g, S, lut, use_cnt, with_rest, s_total=s_total, reduce_cr=1, self_sum=self_sum, describe=d)
        info[name] = d[0]
    torch.cuda.synchronize()
    return out, info


def _check_describe(info, n_lone, W):
    on, off, walk = info["on"], info["off"], info["walk"]
    assert on == off and on["n_tiles"] > 0 and on["lpr"] == rowwise.lanes_per_row(W)           # n_tiles, n_tile_blocks, row_q0, short_tile[] ...
    assert walk["n_tiles"] == 0
    assert off.lone == walk.lone == {"n_lone_rows": 0, "n_lone_blocks": 0, "n_tile_blocks_skipped": 0}
    tiles0 = on["short_tile"][1]                                    # run 0's tiles: ceil(n_lone / (8 rows x 64 / lpr groups))
    assert tiles0 == -(-n_lone // (8 * (64 // on["lpr"])))
    launched = -(-(on["n_tiles"] - tiles0) // 4)
    assert on.lone == {"n_lone_rows": n_lone, "n_lone_blocks": -(-n_lone // LONE_BLOCK),
                       "n_tile_blocks_skipped": on["n_tile_blocks"] - launched if n_lone else 0}
    assert all(bool(v) == (n_lone > 0) for k, v in on.lone.items() if k != "n_tile_blocks_skipped")


# (W, D, counts, rest total, parts, lone rows): every value of every parameter, the three lane groups with every D and both totals
CASES = [(40, 1, True, True, 1, 255), (40, 2, False, True, 2, 256), (40, 3, True, False, 2, 257), (40, 4, False, True, 1, 3001),
         (64, 1, False, False, 2, 3001), (64, 2, True, True, 1, 257), (64, 3, True, True, 2, 3001), (64, 3, False, True, 1, 0),
         (64, 4, True, True, 2, 1), (64, 4, False, False, 1, 256), (128, 1, False, True, 2, 257), (128, 2, True, False, 1, 3001),
         (128, 3, False, True, 1, 1), (128, 4, True, True, 2, 255), (256, 1, True, True, 1, 3001), (256, 2, False, True, 2, 1),
         (256, 3, True, True, 1, 256), (256, 4, False, False, 2, 257), (256, 4, True, True, 1, 0)]


@pytest.mark.parametrize("W,D,use_cnt,with_rest,parts,n_lone", CASES)
def test_every_row_keeps_the_row_walks_bits(W, D, use_cnt, with_rest, parts, n_lone, monkeypatch):
    from gnan_amd import aggregate
    from gnan_amd import functional as Fn
    monkeypatch.setattr(aggregate, "DEGREE_SORTED_COPY_MIN_ROWS", 1)
    rowptr, col, code, n = _csr(n_lone, D)
    g = _graph(rowptr, col, code, n, max(D, 2))                       # (D = 1: _launch_one_code)
    rng = np.random.default_rng(W + D + n_lone)
    S = torch.from_numpy(rng.standard_normal((n, W)).astype(np.float32)).to(DEV)
    lut = torch.from_numpy(rng.standard_normal((D, 1)).astype(np.float32)).to(DEV)
    s_total = Fn.column_sums(S) if with_rest else None
    out, info = _three_launches(monkeypatch, g, S, lut, use_cnt, with_rest, s_total, _self_sum(rng, n, parts).to(DEV), one_code=D == 1)
    _check_describe(info, n_lone, W)
    assert int((np.diff(rowptr) == 0).sum()) == n_lone and bool(torch.isfinite(out["walk"]).all())
    bits = {k: v.view(torch.int32) for k, v in out.items()}
    assert torch.equal(bits["on"], bits["walk"])                    # the lone kernel and the tiles' new epilogue against rows_body
    assert torch.equal(bits["off"], bits["walk"])                   # the tiles' new epilogue alone


@pytest.mark.parametrize("W,parts,n_lone", [(40, 2, 257), (64, 1, 3001), (128, 2, 256), (256, 1, 255)])
def test_exact_integer_cases(W, parts, n_lone, monkeypatch):
    """S integers in [-4, 4], weights 2, -1, 1/2, -1/4, integer self terms: every product and partial sum is a multiple of 1/4 below
    2^24 / 4 (asserted), so float32 is exact in any order and the output equals the int64 restatement."""
    from gnan_amd import aggregate
    from gnan_amd import functional as Fn
    monkeypatch.setattr(aggregate, "DEGREE_SORTED_COPY_MIN_ROWS", 1)
    D = 4
    rowptr, col, code, n = _csr(n_lone, D)
    g = _graph(rowptr, col, code, n, D)
    rng = np.random.default_rng(W)
    S = torch.from_numpy(rng.integers(-4, 5, (n, W)).astype(np.float32))
    lut = torch.tensor([2.0, -1.0, 0.5, -0.25]).view(D, 1)
    self_sum = _self_sum(rng, n, parts, integer=True)
    Sd = S.to(DEV)
    s_total = Fn.column_sums(Sd)
    t4, a4 = rowwise.exact_quarters(rowptr, col, code, S, lut, s_total.cpu(), 1)
    a = self_sum.double().sum(0).long().view(n, 1)                   # the self term: (w_0 - w_rest) a_i = 9/4 a_i
    t4, a4 = t4 + 9 * a, a4 + 9 * self_sum.double().abs().sum(0).long().view(n, 1)
    assert int(a4.max()) < 2 ** 24
    want = (t4.double() / 4).float()
    out, info = _three_launches(monkeypatch, g, Sd, lut.to(DEV), False, True, s_total, self_sum.to(DEV))
    _check_describe(info, n_lone, W)
    for name in ("on", "off", "walk"):
        assert torch.equal(out[name].cpu(), want), name


def test_the_lone_kernel_runs_beside_an_empty_tile_range(monkeypatch):
    """Every row with a pair is a stream row or a hub row (the size gates at 1, as tests/test_gpu_hub_stream.py lowers them): run 0 is the
    only tiled run, so with the lone kernel on spmm_kernel has no workgroup left.  The stream's and the hubs' rows have their own
    summation order, so the plain row walk is the reference for the lone rows only; with the switch on and off every row agrees."""
    from gnan_amd import aggregate
    from gnan_amd import functional as Fn
    W, D, n_lone = 64, 3, 1000
    for name, v in (("DEGREE_SORTED_COPY_MIN_ROWS", 1), ("CLASSED_MIN_NNZ", 1), ("CLASSED_ROWS_MIN_NNZ", 1), ("BLOCKED_HUBS_MIN_NNZ", 1),
                    ("PAIR_STREAM_MIN_NNZ", 1), ("HUB_STREAM_MIN_NNZ", 1), ("BLOCKED_HUB_BLOCK_BYTES", 4 * W * 4)):
        monkeypatch.setattr(aggregate, name, v)
    rowptr, col, code, n = _csr(n_lone, D, "stream")
    g = _graph(rowptr, col, code, n, D)
    rng = np.random.default_rng(5)
    S = torch.from_numpy(rng.standard_normal((n, W)).astype(np.float32)).to(DEV)
    lut = torch.from_numpy(rng.standard_normal((D, 1)).astype(np.float32)).to(DEV)
    out, info = _three_launches(monkeypatch, g, S, lut, True, True, Fn.column_sums(S), _self_sum(rng, n, 2).to(DEV))
    on = info["on"]
    assert on == info["off"] and on["n_stream_blocks"] > 0 and on["n_slice_blocks"] == on["n_hub_seg_blocks"] == 0
    assert on["n_tiles"] == on["short_tile"][1] > 0 and on["row_q0"] == n_lone          # run 0 alone is tiled, no row is walked
    assert on.lone == {"n_lone_rows": n_lone, "n_lone_blocks": -(-n_lone // LONE_BLOCK), "n_tile_blocks_skipped": on["n_tile_blocks"]}
    assert not any(info["off"].lone.values())
    bits = {k: v.view(torch.int32) for k, v in out.items()}
    assert torch.equal(bits["on"], bits["off"])
    lone = torch.from_numpy(np.diff(rowptr) == 0).to(DEV)
    assert int(lone.sum()) == n_lone and torch.equal(bits["on"][lone], bits["walk"][lone])
    assert bool(torch.isfinite(out["on"]).all())
