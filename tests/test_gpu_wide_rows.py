"""The wide aggregation kernel (spmm_kernel: short-row tiles, row blocks, hub slices) against tests/rowwise.py: every case asserts
(a) the ROUTE — the launch query's tile partition equals a restatement from the sorted row lengths, so a case that is meant to run
the tiles cannot silently compare the row walk with itself; (b) the derived per-row float64 bound on EVERY element; (c) the same
bits as the same call with the tiles switched off; (d) the same bits from a second call.  Then: the shapes the tiles decline (the
list a change of the gate has to edit), crafted run edges, exact integer cases with no tolerance at all, and locality under
non-finite operand rows."""
import numpy as np
import pytest
import torch

import rowwise
from helpers import assert_rule
from oracle import gnan_oracle as O
from test_gpu_kernels import _graph, _rho_state, _stack_rho

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _count_table(D):
    """A per-row weight table as a fixed smooth function of the shell counts (elementwise: the same bits in any row order)."""
    base = torch.tensor([0.9, -0.6, 0.45, 0.3, -0.2, 0.7][:D], device=DEV).view(1, D, 1)
    return lambda cnt: base * (0.5 + 1.0 / (1.0 + cnt.float().unsqueeze(-1)))


def _check(monkeypatch, csr, n_cols, D, W, use_cnt, with_rest, reduce_cr=0, lmax=4, i64=True, table="shared", dtype=torch.float32,
           Cw=1, row_ids=None, expect="tiles", seed=0, cnt=None, classed=False, sorted_copy=True, S=None, what=""):
    """One case through (a) - (d); returns ``(worst |err| / bound, launch info, output)``.  ``expect``: 'tiles' (the restated partition,
    and it is not empty), 'restated' (the restated partition, whatever it holds) or 'declined' (no tiles)."""
    from gnan_amd import HopGraph, aggregate
    from gnan_amd import functional as Fn
    monkeypatch.setattr(aggregate, "DEGREE_SORTED_COPY_MIN_ROWS", 1)
    monkeypatch.setattr(aggregate, "DEGREE_SORTED_COPY", sorted_copy)
    monkeypatch.setattr(aggregate, "SHORT_ROW_LMAX", lmax)
    if classed:
        monkeypatch.setattr(aggregate, "CLASSED_MIN_NNZ", 1)
    rowptr, col, code = csr
    n = len(rowptr) - 1
    rng = np.random.default_rng(1000 + seed)
    idx = torch.int64 if i64 else torch.int32
    if cnt is None:
        g = _graph(rowptr, col, code, n_cols, D, idx)
    else:
        g = HopGraph.from_csr(torch.from_numpy(rowptr).to(idx).to(DEV), torch.from_numpy(col).to(DEV), torch.from_numpy(code).to(DEV),
                              n_cols=n_cols, n_codes=D, cnt=torch.from_numpy(cnt).to(DEV))
    if S is None:
        S = torch.from_numpy(rng.standard_normal((n_cols, W)).astype(np.float32))
    S = S.to(DEV).to(dtype)
    s_total = Fn.column_sums(S) if with_rest else None
    if table == "shared":
        lut = torch.from_numpy(rng.standard_normal((D, Cw)).astype(np.float32)).to(DEV)
        lut_nat, kw = lut, {}
    else:
        lut, f = None, _count_table(D)
        lut_nat, kw = f(g.cnt), {"lut_of_counts": f}
    ids = None if row_ids is None else torch.from_numpy(np.asarray(row_ids, dtype=np.int32)).to(DEV)

    def call(tiles):
        monkeypatch.setattr(aggregate, "SHORT_ROW_TILES", tiles)
        d = []
        y = aggregate.spmm_launch(g, S, lut, use_cnt, with_rest, row_ids=ids, s_total=s_total, reduce_cr=reduce_cr, describe=d, **kw)
        assert len(d) == 1
        return y, d[0]

    y, info = call(True)
    again, info2 = call(True)
    plain, info0 = call(False)
    torch.cuda.synchronize()
    # (a) the route
    assert info == info2 and info0["n_tiles"] == 0 and info0["row_q0"] == 0
    assert info["kernel"] == 1 and info["classed"] == int(classed)
    deg = np.sort(np.diff(rowptr))
    if expect == "declined":
        assert (info["n_tiles"], info["n_tile_blocks"], info["row_q0"]) == (0, 0, 0), info
    else:
        assert (info["vec"], info["lpr"], info["smalld"], info["dense"]) == (4, rowwise.lanes_per_row(W), 1, 0), info
        n_tiles, q0, first = rowwise.tile_partition(deg, info["lpr"], lmax)
        assert (info["n_tiles"], info["row_q0"], info["short_tile"][:lmax + 1]) == (n_tiles, q0, first), info
        assert info["n_tile_blocks"] == -(-n_tiles // 4)
        if expect == "tiles":
            assert n_tiles > 0
    # (b) every element within its own row's bound
    truth, bound = rowwise.reference(rowptr, col, code, S.float().cpu(), lut_nat.cpu(), g.cnt.cpu() if use_cnt else None,
                                     None if s_total is None else s_total.cpu(), reduce_cr=reduce_cr, rows=row_ids)
    ratio = rowwise.assert_within(y.cpu(), truth, bound, what)
    # (c) the row walk's bits, (d) the same bits twice
    assert torch.equal(y, plain)
    assert torch.equal(y, again)
    print(f"ROW-BOUND worst |err|/bound {ratio:.3f} tiles {info['n_tiles']} :: {what}")
    return ratio, info, y


# ---- served shapes --------------------------------------------------------------------------------------------------------------
# (W, D, use_cnt, with_rest, reduce_cr, SHORT_ROW_LMAX, int64 rowptr, weight table)
SERVED = [
    (36, 2, True, True, 0, 4, True, "shared"), (40, 3, False, True, 1, 4, False, "shared"), (64, 4, True, False, 2, 8, True, "counts"),
    (36, 2, False, False, 4, 1, False, "counts"), (40, 4, True, True, 0, 8, True, "counts"), (64, 3, True, True, 1, 4, True, "shared"),
    (64, 2, False, True, 0, 4, False, "counts"), (40, 2, True, False, 1, 1, True, "shared"), (36, 3, True, True, 2, 4, False, "shared"),
    (36, 4, False, True, 1, 8, True, "shared"), (64, 4, False, False, 4, 4, False, "shared"), (40, 3, True, True, 4, 8, True, "counts"),
    (64, 3, False, False, 0, 1, True, "shared"), (40, 4, False, True, 2, 4, True, "counts"),
    (100, 2, True, True, 0, 4, True, "shared"), (128, 3, False, True, 1, 4, False, "counts"), (100, 4, True, False, 2, 8, False, "shared"),
    (128, 2, False, False, 4, 1, True, "shared"), (128, 4, True, True, 0, 4, True, "counts"), (100, 3, True, True, 4, 4, True, "shared"),
    (128, 3, True, False, 0, 8, False, "shared"), (100, 2, False, True, 1, 8, True, "counts"), (128, 4, False, True, 1, 1, False, "shared"),
    (100, 3, False, False, 2, 4, True, "counts"), (128, 2, True, True, 2, 4, True, "counts"), (100, 4, False, True, 0, 4, False, "shared"),
    (200, 2, True, True, 0, 4, True, "shared"), (256, 3, False, True, 1, 4, False, "shared"), (200, 4, True, False, 2, 8, True, "counts"),
    (256, 2, False, False, 4, 1, False, "counts"), (256, 4, True, True, 0, 4, True, "shared"), (200, 3, True, True, 4, 8, False, "shared"),
    (256, 3, True, False, 0, 1, True, "counts"), (200, 2, False, True, 1, 4, True, "shared"), (256, 4, False, True, 1, 8, True, "counts"),
    (200, 3, False, False, 2, 4, False, "shared"), (256, 2, True, True, 2, 4, False, "shared"), (200, 4, False, True, 4, 4, True, "counts"),
    (256, 3, True, True, 4, 4, True, "counts"), (256, 4, False, False, 0, 8, False, "shared"),
]


def _lane_class(W):
    return rowwise.lanes_per_row(W)


def test_the_served_list_covers_what_it_claims():
    """Every value of every dimension, and every pair of (lane-group class of W, D), (class, reduce_cr), (table kind, use_cnt)."""
    cols = list(zip(*SERVED))
    assert set(cols[0]) == {36, 40, 64, 100, 128, 200, 256} and set(cols[1]) == {2, 3, 4}
    assert set(cols[2]) == set(cols[3]) == set(cols[6]) == {True, False}
    assert set(cols[4]) == {0, 1, 2, 4} and set(cols[5]) == {1, 4, 8} and set(cols[7]) == {"shared", "counts"}
    assert {(_lane_class(c[0]), c[1]) for c in SERVED} == {(k, D) for k in (16, 32, 64) for D in (2, 3, 4)}
    assert {(_lane_class(c[0]), c[4]) for c in SERVED} == {(k, cr) for k in (16, 32, 64) for cr in (0, 1, 2, 4)}
    assert {(c[7], c[2]) for c in SERVED} == {(t, u) for t in ("shared", "counts") for u in (True, False)}


@pytest.mark.parametrize("W,D,use_cnt,with_rest,reduce_cr,lmax,i64,table", SERVED)
def test_served_shapes_take_the_tiles_and_meet_the_row_bound(W, D, use_cnt, with_rest, reduce_cr, lmax, i64, table, monkeypatch):
    seed = W + 7 * D + 3 * reduce_cr + lmax
    n = 4000
    csr = rowwise.short_csr(n, np.random.default_rng(seed), D)
    _check(monkeypatch, csr, n, D, W, use_cnt, with_rest, reduce_cr, lmax, i64, table, seed=seed,
           what=f"W={W} D={D} cnt={use_cnt} rest={with_rest} cr={reduce_cr} lmax={lmax} i64={i64} {table}")


@pytest.mark.parametrize("W,with_rest", [(64, True), (128, False), (256, True)])
def test_pre_rho_route_takes_the_tiles_with_a_per_row_table(W, with_rest, monkeypatch):
    """pre_rho_aggregate end to end: the route decides on the tiles BEFORE the table of the walked copy exists, so short_tile reads a
    per-row table.  Judged twice: the aggregation, given the table the library looked up, by the per-row bound; the whole, against
    the float64 oracle's pre-rho weights, by the project's global rule (the table's own error is the shape functions', not the sum's)."""
    from gnan_amd import _lib, aggregate
    from gnan_amd import functional as Fn
    from gnan_amd.graph import hop_inputs
    monkeypatch.setattr(aggregate, "DEGREE_SORTED_COPY_MIN_ROWS", 1)
    monkeypatch.setattr(Fn, "FMLP_ALGO", _lib.FMLP_PWL)                   # rho's table route at this size
    n, D = 4000, 3
    rng = np.random.default_rng(W)
    rowptr, col, code = rowwise.short_csr(n, rng, D)
    g = _graph(rowptr, col, code, n, D)
    sd = _rho_state(3, 16, 1, True, seed=4, zero_bias=False)
    p = _stack_rho(sd, 3, 16, 1, True)
    u = hop_inputs(D, DEV)
    S = torch.from_numpy(rng.standard_normal((n, W)).astype(np.float32)).to(DEV)
    s_total = Fn.column_sums(S) if with_rest else None
    out = {}
    with torch.no_grad():
        for tiles in (True, True, False):
            monkeypatch.setattr(aggregate, "SHORT_ROW_TILES", tiles)
            d = []
            y = aggregate.pre_rho_aggregate(g, S, p, u, with_rest=with_rest, s_total=s_total, describe=d)
            out.setdefault(tiles, []).append((y, d[0]))
        lut_nat = Fn.rho_row_lut(g.cnt, u, p)
    (y, info), (again, _), (plain, info0) = out[True][0], out[True][1], out[False][0]
    n_tiles, q0, first = rowwise.tile_partition(np.sort(np.diff(rowptr)), info["lpr"], 4)
    assert n_tiles > 0 and (info["n_tiles"], info["row_q0"], info["short_tile"][:5]) == (n_tiles, q0, first)
    assert info0["n_tiles"] == 0
    tot = None if s_total is None else s_total.cpu()
    truth, bound = rowwise.reference(rowptr, col, code, S.cpu(), lut_nat.cpu(), None, tot)
    ratio = rowwise.assert_within(y.cpu(), truth, bound, "pre-rho")
    print(f"ROW-BOUND worst |err|/bound {ratio:.3f} tiles {n_tiles} :: pre-rho W={W} rest={with_rest}")
    assert torch.equal(y, plain) and torch.equal(y, again)
    lut64 = O.row_lut_pre_rho({k: v.double() for k, v in sd.items()}, g.cnt.cpu().numpy(), torch.float64)
    truth64, _ = rowwise.reference(rowptr, col, code, S.cpu(), lut64, None, tot)
    assert_rule(y.cpu(), truth64, None, what="pre-rho against the oracle's weights")


# ---- declined shapes: the list a change of the gate has to edit --------------------------------------------------------------------
@pytest.mark.parametrize("name", ["W=32", "W=50", "W=320", "bf16", "D=6", "Cw=2", "row_ids", "no sorted copy"])
def test_declined_shapes_report_no_tiles_and_meet_the_row_bound(name, monkeypatch):
    n = 4000
    rng = np.random.default_rng(len(name))
    kw = dict(W=64, D=3, use_cnt=True, with_rest=True)
    if name.startswith("W="):
        kw["W"] = int(name[2:])
    elif name == "bf16":
        kw["dtype"] = torch.bfloat16                    # (the truth is taken from the operand as stored: rounded to bf16)
    elif name == "D=6":
        kw["D"] = 6                                     # the copy has no packed index beyond four codes
    elif name == "Cw=2":
        kw["Cw"] = 2
    elif name == "row_ids":
        kw["row_ids"] = np.concatenate([rng.integers(0, n, 700), [7, 1234, n - 1, 7]])
    else:
        kw["sorted_copy"] = False
    csr = rowwise.short_csr(n, rng, kw["D"])
    _, info, _ = _check(monkeypatch, csr, n, expect="declined", seed=len(name), what=f"declined: {name}", **kw)
    if name == "W=50":
        assert info["vec"] == 1
    if name == "bf16":
        assert info["vec"] == 8


# ---- run edges ------------------------------------------------------------------------------------------------------------------------
def _edge(name, W, rng):
    """(degrees, D, keywords of _check) of a crafted degree sequence."""
    G = 64 // rowwise.lanes_per_row(W)
    kw = dict(use_cnt=True, with_rest=True)
    D = 3
    if name == "all empty":
        deg = np.zeros(300, dtype=np.int64)
        kw["expect"] = "declined"                      # nnz == 0: the gate declines, the output is the rest term alone
    elif name == "L in {0, 4}":
        deg = rng.permutation(np.repeat([0, 4], [50, 70]))
    elif name.startswith("run of"):
        c1, c3 = {"run of 1": (1, 1), "run of G R": (8 * G, 2 * G), "run of G R + 1": (8 * G + 1, 2 * G + 1)}[name]
        deg = rng.permutation(np.repeat([1, 3, 2, 6], [c1, c3, 5, 3]))
    elif name == "all short":
        deg = rng.integers(0, 5, 500)
    elif name == "none short":
        deg = rng.integers(5, 13, 300)
        kw["expect"] = "restated"                      # served, and every run is empty
    elif name == "empty shells":
        deg, D = rng.integers(0, 4, 400), 4             # rows of at most 3 pairs over 3 listed codes: most counts are zero
    else:
        raise ValueError(name)
    return deg, D, kw


@pytest.mark.parametrize("W", [64, 256])
@pytest.mark.parametrize("name", ["all empty", "L in {0, 4}", "run of 1", "run of G R", "run of G R + 1", "all short", "none short",
                                  "empty shells"])
def test_run_edges(name, W, monkeypatch):
    rng = np.random.default_rng(W + len(name))
    deg, D, kw = _edge(name, W, rng)
    n = len(deg)
    csr = rowwise.csr_of_degrees(deg, n, rng, D)
    _, info, y = _check(monkeypatch, csr, n, D, W, seed=W, what=f"edge: {name} W={W}", **kw)
    if name == "all empty":
        assert csr[1].size == 0 and bool((y == y[0:1]).all())          # one shell count for every row: one rest term
    if name == "all short":
        assert info["row_q0"] == n                                      # no row blocks at all
    if name == "none short":
        assert info["n_tiles"] == 0 and info["row_q0"] == 0
    if name == "L in {0, 4}":
        t = info["short_tile"]
        assert t[1] == t[2] == t[3] == t[4] > 0                        # the runs between are empty
    if name == "empty shells":
        cnt = rowwise._idx(np.stack([np.bincount(csr[2][csr[0][i]:csr[0][i + 1]], minlength=D)[:D - 1] for i in range(n)]))
        assert bool((cnt == 0).any())


@pytest.mark.parametrize("W,use_cnt", [(64, True), (256, False)])
@pytest.mark.parametrize("with_rest", [True, False])
def test_listed_pairs_carrying_the_rest_code_are_clipped(W, use_cnt, with_rest, monkeypatch):
    rng = np.random.default_rng(W + with_rest)
    n, D = 1500, 3
    rowptr, col, code = rowwise.short_csr(n, rng, D, hubs=((7, 600),))
    high = rng.random(code.size) < 0.3
    code[high] = rng.integers(D - 1, 4, int(high.sum())).astype(np.uint8)      # the rest code, and one above it
    clipped = np.minimum(code, D - 1)
    cnt = np.zeros((n, D), dtype=np.int32)
    np.add.at(cnt, (np.repeat(np.arange(n), np.diff(rowptr)), clipped), 1)
    cnt[:, D - 1] = n - np.diff(rowptr)
    _check(monkeypatch, (rowptr, col, code), n, D, W, use_cnt, with_rest, cnt=cnt, seed=W, what=f"rest-coded pairs W={W} rest={with_rest}")


def _own_counts(n, D, rng, powers_of_two=False):
    """Shell counts handed in by the caller (HopGraph.from_csr(cnt=...)), different from row to row WITHIN a run of equal row lengths
    — the counts the graph derives give the rows of one run one rest count, and a tile that read another row's would go unnoticed."""
    if powers_of_two:
        return (1 << rng.integers(0, 3, (n, D))).astype(np.int32)
    cnt = rng.integers(0, 6, (n, D)).astype(np.int32)               # zeros: empty shells
    cnt[:, D - 1] = rng.integers(1, 60, n)
    return cnt


@pytest.mark.parametrize("W,D,reduce_cr,table", [(64, 3, 0, "shared"), (256, 4, 0, "counts"), (40, 2, 1, "counts"), (128, 4, 4, "shared"),
                                                 (64, 4, 0, "counts"), (256, 3, 2, "shared")])
@pytest.mark.parametrize("with_rest", [True, False])
def test_rows_of_one_group_keep_their_own_counts(W, D, reduce_cr, table, with_rest, monkeypatch):
    rng = np.random.default_rng(W + D + with_rest)
    n = 3000
    csr = rowwise.short_csr(n, rng, D, hubs=((7, 600),))
    _check(monkeypatch, csr, n, D, W, True, with_rest, reduce_cr, table=table, cnt=_own_counts(n, D, rng), seed=W + D,
           what=f"own counts W={W} D={D} cr={reduce_cr} {table} rest={with_rest}")


@pytest.mark.parametrize("W,reduce_cr", [(64, 0), (256, 0), (64, 1), (128, 4)])
def test_slice_tile_and_row_blocks_in_one_launch(W, reduce_cr, monkeypatch):
    """The classed hub plan on a small graph: hubs of 513, 2500 and 40 000 pairs ahead of the tiles and the row blocks."""
    rng = np.random.default_rng(W)
    n, D = 4000, 4
    csr = rowwise.short_csr(n, rng, D, hubs=((5, 513), (17, 2500), (400, 40_000)))
    _, info, _ = _check(monkeypatch, csr, n, D, W, True, True, reduce_cr, classed=True, seed=W, what=f"classed W={W} cr={reduce_cr}")
    assert info["classed"] == 1 and info["n_slice_blocks"] > 0 and info["n_tiles"] > 0 and info["row_q0"] < n


# ---- exact cases: no tolerance ---------------------------------------------------------------------------------------------------------
EXACT_LUT = [2.0, -1.0, 0.5, -0.25]


def _exact_inputs(n, D, W, rng, hubs, unique_cols=False):
    rowptr, col, code = rowwise.short_csr(n, rng, D, hubs=hubs)
    if unique_cols:                                    # (the dense layout holds one code per pair of nodes)
        for i in range(n):
            lo, hi = rowptr[i], rowptr[i + 1]
            keep_self = hi > lo and col[lo] == i and code[lo] == 0
            others = rng.permutation(n - 1)[:hi - lo]
            others[others >= i] += 1
            col[lo:hi] = others
            if keep_self:
                col[lo] = i
    S = torch.from_numpy(rng.integers(-4, 5, (n, W)).astype(np.float32))
    lut = torch.tensor(EXACT_LUT[:D]).view(D, 1)
    return (rowptr, col, code), S, lut


EXACT = [  # (route, W, D, with_rest, reduce_cr)
    ("tiles", 40, 4, True, 0), ("tiles", 64, 4, True, 0), ("tiles", 256, 4, True, 0), ("tiles", 64, 3, True, 1), ("tiles", 40, 2, True, 4),
    ("tiles", 256, 4, True, 1), ("tiles", 256, 3, False, 4), ("tiles", 64, 4, False, 0), ("tiles", 40, 4, True, 1),
    ("rows", 64, 4, True, 0), ("rows", 256, 4, True, 1), ("rows", 40, 3, False, 4),
    ("classed", 64, 4, True, 0), ("classed", 40, 4, True, 4), ("classed", 256, 4, False, 0),
    ("hubs", 64, 4, True, 0), ("hubs", 40, 4, True, 4), ("hubs", 256, 3, True, 0),
    ("bf16", 64, 4, True, 0), ("bf16", 64, 4, False, 1),
    # beyond the list above: shell counts 1, 2, 4 of the caller's own, different within a run (weights in sixteenths): a weight
    # or a rest weight taken from another row of the lane group changes an integer
    ("tiles+cnt", 64, 4, True, 0), ("tiles+cnt", 256, 4, True, 0), ("tiles+cnt", 40, 3, True, 1), ("tiles+cnt", 128, 4, False, 0),
]


@pytest.mark.parametrize("route,W,D,with_rest,reduce_cr", EXACT)
def test_exact_integer_cases(route, W, D, with_rest, reduce_cr, monkeypatch):
    """S integer-valued in [-4, 4], weights 2, -1, 1/2, -1/4, no counts: every product and every partial sum is a multiple of 1/4 of
    less than 2^24 quarters (asserted from the magnitudes), so float32 is exact in any order and the output equals the int64
    restatement — a pair read from the wrong row, a weight from the wrong code or a lost slice changes an integer."""
    from gnan_amd import aggregate
    from gnan_amd import functional as Fn
    monkeypatch.setattr(aggregate, "DEGREE_SORTED_COPY_MIN_ROWS", 1)
    monkeypatch.setattr(aggregate, "SHORT_ROW_TILES", route != "rows")
    big = route in ("classed", "hubs")
    if big:
        monkeypatch.setattr(aggregate, "CLASSED_MIN_NNZ", 1)
        monkeypatch.setattr(aggregate, "XCD_CLASSED_HUBS", route == "classed")
    rng = np.random.default_rng(W + D + reduce_cr)
    n = 3000
    hubs = ((5, 513), (17, 2500), (400, 40_000)) if big else ((7, 600), (1234, 1200), (-1, 513))
    (rowptr, col, code), S, lut = _exact_inputs(n, D, W, rng, hubs)
    own = route == "tiles+cnt"
    cnt = _own_counts(n, D, rng, powers_of_two=True) if own else None
    scale = 16 if own else 4
    if own:
        from gnan_amd import HopGraph
        g = HopGraph.from_csr(torch.from_numpy(rowptr).to(DEV), torch.from_numpy(col).to(DEV), torch.from_numpy(code).to(DEV),
                              n_cols=n, n_codes=D, cnt=torch.from_numpy(cnt).to(DEV))
    else:
        g = _graph(rowptr, col, code, n, D)
    Sd = S.to(DEV).to(torch.bfloat16 if route == "bf16" else torch.float32)
    assert torch.equal(Sd.float().cpu(), S)                       # small integers are exact in bf16
    s_total = Fn.column_sums(Sd) if with_rest else None
    t4, a4 = rowwise.exact_scaled(rowptr, col, code, S, lut, None if s_total is None else s_total.cpu(), reduce_cr, cnt, scale)
    assert int(a4.max()) < 2 ** 24
    d = []
    y = aggregate.spmm_launch(g, Sd, lut.to(DEV), own, with_rest, s_total=s_total, reduce_cr=reduce_cr, describe=d)
    info = d[0]
    assert (info["n_tiles"] > 0) == (route in ("tiles", "tiles+cnt", "classed", "hubs")) and info["classed"] == int(route == "classed")
    assert info["n_slice_blocks"] > 0
    want = (t4.double() / scale).float()
    assert bool((want.double() * scale == t4.double()).all())
    bad = torch.nonzero(y.cpu() != want)
    assert bad.numel() == 0, (f"{bad.shape[0]} elements differ; first at {bad[0].tolist()}: got {float(y.cpu()[tuple(bad[0])])}, "
                              f"exact {float(want[tuple(bad[0])])}")


@pytest.mark.parametrize("with_rest", [True, False])
def test_exact_integer_case_dense_layout_equals_the_tiled_csr(with_rest, monkeypatch):
    """The same graph in the dense layout (every pair of nodes coded, unlisted ones with the rest code): the same integers."""
    from gnan_amd import HopGraph, aggregate
    from gnan_amd import functional as Fn
    monkeypatch.setattr(aggregate, "DEGREE_SORTED_COPY_MIN_ROWS", 1)
    rng = np.random.default_rng(3)
    n, D, W = 1500, 4, 64
    (rowptr, col, code), S, lut = _exact_inputs(n, D, W, rng, ((7, 600), (-1, 513)), unique_cols=True)
    g = _graph(rowptr, col, code, n, D)
    dense_code = torch.full((n, n), D - 1, dtype=torch.uint8)
    dense_code[torch.from_numpy(np.repeat(np.arange(n), np.diff(rowptr))), torch.from_numpy(col).long()] = torch.from_numpy(code)
    gd = HopGraph(n_rows=n, n_cols=n, n_codes=D, code=dense_code.to(DEV), cnt=g.cnt)
    Sd = S.to(DEV)
    s_total = Fn.column_sums(Sd)
    if not with_rest:                                  # listed pairs only: the dense layout's unlisted pairs get weight zero
        lut = lut.clone()
        lut[D - 1] = 0.0
    t4, a4 = rowwise.exact_quarters(rowptr, col, code, S, lut, s_total.cpu() if with_rest else None)
    assert int(a4.max()) < 2 ** 24
    want = (t4.double() / 4.0).float()
    d, dd = [], []
    y = aggregate.spmm_launch(g, Sd, lut.to(DEV), False, with_rest, s_total=s_total if with_rest else None, describe=d)
    yd = aggregate.spmm_launch(gd, Sd, lut.to(DEV), False, False, describe=dd)
    assert d[0]["n_tiles"] > 0 and dd[0]["dense"] == 1 and dd[0]["n_tiles"] == 0
    assert torch.equal(y.cpu(), want)
    assert torch.equal(yd.cpu(), want)


# ---- locality ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,reduce_cr", [(64, 0), (256, 0), (64, 1), (128, 2)])
def test_non_finite_operand_rows_stay_in_the_rows_that_list_them(W, reduce_cr, monkeypatch):
    """Ordinary float values, no fault: S[j] = NaN for a few j, +Inf for a few others, no rest term.  The rows that list such a j are
    non-finite; every other row — the other rows of the same tile group included — keeps the bits of the clean run."""
    from gnan_amd import aggregate
    monkeypatch.setattr(aggregate, "DEGREE_SORTED_COPY_MIN_ROWS", 1)
    rng = np.random.default_rng(W + reduce_cr)
    n, D = 2000, 3
    rowptr, col, code = rowwise.short_csr(n, rng, D)
    deg = np.diff(rowptr)
    poison = rng.choice(n, 6, replace=False)
    for L in (1, 2, 3, 4):                                           # a few rows of every tiled length list a poisoned neighbour
        for i in rng.choice(np.nonzero(deg == L)[0], 5, replace=False):
            col[rowptr[i] + rng.integers(0, L)] = poison[rng.integers(0, 6)]
    lists = np.zeros(n, dtype=bool)
    lists[np.repeat(np.arange(n), deg)[np.isin(col, poison)]] = True
    # a clean row and a poisoned row share a lane group, for every tiled length: the copy's order is (length, row id), a group R_L rows
    order = np.argsort(deg, kind="stable")
    for L in (1, 2, 3, 4):
        run = order[deg[order] == L]
        R = max(1, 8 // L)
        grp = [lists[run[k:k + R]] for k in range(0, len(run), R)]
        assert any(x.any() and not x.all() for x in grp), L
    g = _graph(rowptr, col, code, n, D)
    S = torch.from_numpy(rng.standard_normal((n, W)).astype(np.float32))
    lut = torch.tensor([[0.9], [0.35], [-0.2]], device=DEV)
    bad = S.clone()
    bad[poison[:3]] = float("nan")
    bad[poison[3:]] = float("inf")
    d = []
    clean = aggregate.spmm_launch(g, S.to(DEV), lut, True, False, reduce_cr=reduce_cr, describe=d)
    dirty = aggregate.spmm_launch(g, bad.to(DEV), lut, True, False, reduce_cr=reduce_cr)
    assert d[0]["n_tiles"] > 0
    clean, dirty = clean.cpu(), dirty.cpu()
    assert bool(torch.isfinite(clean).all())
    assert not bool(torch.isfinite(dirty[torch.from_numpy(lists)]).any())
    keep = torch.from_numpy(~lists)
    assert torch.equal(dirty[keep], clean[keep])
