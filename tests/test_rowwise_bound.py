"""tests/rowwise.py pinned without a GPU: the float64 stand-in of the aggregation and two float32 passes (the oracle's, and the wide
kernel's own order — folded weights, an fma chain over the row's pairs, one fma for the rest term) sit inside the derived per-row
bound; planted errors of the size ``helpers.rule`` lets through do not.  And the host-only launch query (gnan_spmm_fwd_describe)
against a restatement of the tile partition, over the operand widths on both sides of the gate."""
import numpy as np
import pytest
import torch

import cpu_kernels
import rowwise
from helpers import rule
from oracle import gnan_oracle as O


def _cpu_graph(rowptr, col, code, n, D, idx_dtype=torch.int64):
    from gnan_amd import HopGraph
    return HopGraph.from_csr(torch.from_numpy(rowptr).to(idx_dtype), torch.from_numpy(col), torch.from_numpy(code), n_cols=n, n_codes=D)


def _fma32(a, b, c):
    """fmaf on float32 arrays: the product of two float32 is exact in float64; the sum is rounded once more on the way to float64
    (2^-53 relative, far below the float32 rounding that follows)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _kernel_order_f32(rowptr, col, code, S, lut, cnt, s_total, reduce_cr=0):
    """The small-D rows' arithmetic of csrc/spmm_fwd_body.hpp (rows_body / short_tile) in float32, rows of any length walked as one chain."""
    n, D = len(rowptr) - 1, lut.shape[0]
    rest = D - 1
    w = np.broadcast_to(lut.reshape(1, D).astype(np.float32), (n, D)).copy()
    if cnt is not None:
        w = (w / np.maximum(cnt, 1).astype(np.float32)).astype(np.float32)
    wr = w[:, rest].copy()
    if s_total is not None:
        w = (w - wr[:, None]).astype(np.float32)
        w[:, rest] = 0.0
    acc = np.zeros((n, S.shape[1]), dtype=np.float32)
    deg = np.diff(rowptr)
    for l in range(int(deg.max())):
        rows = np.nonzero(deg > l)[0]
        e = rowptr[rows] + l
        d = np.minimum(code[e], rest)
        acc[rows] = _fma32(w[rows, d][:, None], S[col[e]], acc[rows])
    if s_total is not None:
        acc = _fma32(wr[:, None], s_total[None, :].astype(np.float32), acc)
    if reduce_cr:
        acc = acc.reshape(n, -1, reduce_cr).sum(1, dtype=np.float32)
    return acc


@pytest.mark.parametrize("W,D", [(40, 2), (64, 3), (40, 4), (64, 4)])
@pytest.mark.parametrize("use_cnt", [True, False])
@pytest.mark.parametrize("with_rest", [True, False])
def test_float64_stand_in_and_float32_passes_sit_inside_the_row_bound(W, D, use_cnt, with_rest):
    rng = np.random.default_rng(W + D + 2 * use_cnt + with_rest)
    n = 4000
    rowptr, col, code = rowwise.short_csr(n, rng, D)
    g = _cpu_graph(rowptr, col, code, n, D)
    S = torch.from_numpy(rng.standard_normal((n, W)).astype(np.float32))
    lut = torch.from_numpy(rng.standard_normal((D, 1)).astype(np.float32))
    cnt = g.cnt.numpy() if use_cnt else None
    s_total = S.sum(0) if with_rest else None                    # float32, as a launch would be handed it
    for cr in (0, 1, 4):
        truth, bound = rowwise.reference(rowptr, col, code, S, lut, cnt, s_total, reduce_cr=cr)
        assert truth.shape == bound.shape == (n, cr or W)
        y64 = cpu_kernels.spmm_launch(g, S, lut, use_cnt, with_rest, s_total=s_total, reduce_cr=cr)
        r64 = rowwise.assert_within(y64, truth, bound, "float64 stand-in")
        assert r64 <= 0.25                                       # one rounding of the result against k >= 5 of them
        yk = _kernel_order_f32(rowptr, col, code, S.numpy(), lut.numpy(), cnt, None if s_total is None else s_total.numpy(), cr)
        rk = rowwise.assert_within(yk, truth, bound, "float32, the kernel's order")
        assert 0.0 < rk < 1.0
    if with_rest:                                                # the oracle's own float32 pass (it sums the operand itself)
        S32 = S.clone()
        y32 = O.spmm_csr_vectorised(rowptr, col, code, S32, lut, cnt)
        truth, bound = rowwise.reference(rowptr, col, code, S, lut, cnt, S32.sum(dim=0))
        short = np.diff(rowptr) <= 30                            # (its hub rows are one index_add chain each: not the kernel's slices)
        rowwise.assert_within(y32.numpy()[short], truth[short], bound[short], "float32 oracle")


def test_the_row_bound_catches_what_the_global_rule_lets_through():
    rng = np.random.default_rng(5)
    n, W, D = 4000, 64, 3
    rowptr, col, code = rowwise.short_csr(n, rng, D)
    g = _cpu_graph(rowptr, col, code, n, D)
    S = torch.from_numpy(rng.standard_normal((n, W)).astype(np.float32))
    lut = torch.tensor([[0.9], [0.35], [-0.2]])
    s_total = S.sum(0)
    truth, bound = rowwise.reference(rowptr, col, code, S, lut, g.cnt.numpy(), s_total)
    good = cpu_kernels.spmm_launch(g, S, lut, True, True, s_total=s_total)
    rowwise.assert_within(good, truth, bound)
    deg = np.diff(rowptr)
    i = int(np.nonzero(deg == 2)[0][3])
    scale = float(np.abs(truth).max())
    # (i) one element of a short row off by 5e-6 of the largest entry of the result
    bad = good.clone()
    bad[i, 17] += 5e-6 * scale
    assert rule(bad, truth)[0]
    with pytest.raises(AssertionError, match=f"row {i}, column 17"):
        rowwise.assert_within(bad, truth, bound)
    assert rowwise.worst_ratio(bad, truth, bound) == float("inf")
    # (ii) the row's second pair weighted with its neighbour row's pair's code: the wrong hop weight
    lo = int(rowptr[i])
    code2 = code.copy()
    code2[lo + 1] = 1 if code[lo + 1] != 1 else 0
    wrong = cpu_kernels.spmm_launch(_cpu_graph(rowptr, col, code2, n, D), S, lut, True, True, s_total=s_total)
    wrong_row = good.clone()
    wrong_row[i] = wrong[i]
    with pytest.raises(AssertionError, match=f"row {i},"):
        rowwise.assert_within(wrong_row, truth, bound)
    # (iii) a zero bound asks for an exact zero: an empty row without the rest term
    truth0, bound0 = rowwise.reference(rowptr, col, code, S, lut, g.cnt.numpy(), None)
    e = int(np.nonzero(deg == 0)[0][0])
    assert not bound0[e].any() and not truth0[e].any()
    y0 = cpu_kernels.spmm_launch(g, S, lut, True, False)
    rowwise.assert_within(y0, truth0, bound0)
    y0[e, 3] = 1e-30
    with pytest.raises(AssertionError, match=f"row {e}, column 3"):
        rowwise.assert_within(y0, truth0, bound0)
    y0[e, 3] = float("nan")
    with pytest.raises(AssertionError):
        rowwise.assert_within(y0, truth0, bound0)


def test_the_bound_counts_hub_rows_from_the_library_threshold():
    """rowwise.py stays free of the package; the row length from which it counts k = 2 L roundings is the one the plans slice from."""
    from gnan_amd import graph as G
    assert rowwise.HUB_THRESHOLD == G.LONG_ROW_THRESHOLD == G.CLASSED_HUB_THRESHOLD


def test_row_bound_subsets_per_row_tables_and_clipped_codes():
    rng = np.random.default_rng(9)
    n, W, D = 500, 8, 3
    rowptr, col, code = rowwise.short_csr(n, rng, D, hubs=((7, 600),))
    code[rng.random(code.size) < 0.2] = D - 1                    # listed pairs that carry the rest code
    g = _cpu_graph(rowptr, col, np.minimum(code, D - 2), n, D)   # (the stand-in indexes its table by the code: give it the clipped ones ...
    S = torch.from_numpy(rng.standard_normal((n, W)).astype(np.float32))
    lut = torch.from_numpy(rng.standard_normal((n, D, 2)).astype(np.float32))
    s_total = S.sum(0)
    truth, bound = rowwise.reference(rowptr, col, code, S, lut, None, s_total)
    # ... for which a listed pair of the rest code counts as unlisted: w_rest S - w_rest S)
    keep = code < D - 1
    rp2 = np.zeros(n + 1, dtype=np.int64)
    rp2[1:] = np.cumsum(np.add.reduceat(keep.astype(np.int64), rowptr[:-1]) * (np.diff(rowptr) > 0))
    g2 = _cpu_graph(rp2, col[keep], code[keep], n, D)
    y = cpu_kernels.spmm_launch(g2, S, lut, False, True, s_total=s_total)
    rowwise.assert_within(y, truth, bound, "clipped codes")
    rows = np.array([7, 0, 499, 7, 33])
    t_sub, b_sub = rowwise.reference(rowptr, col, code, S, lut, None, s_total, rows=rows)
    assert np.array_equal(t_sub, truth[rows]) and np.array_equal(b_sub, bound[rows])
    del g


def test_exact_quarters_is_the_float64_truth():
    rng = np.random.default_rng(2)
    n, W, D = 300, 8, 4
    rowptr, col, code = rowwise.short_csr(n, rng, D, hubs=((7, 600),))
    S = torch.from_numpy(rng.integers(-4, 5, (n, W)).astype(np.float32))
    lut = torch.tensor([2.0, -1.0, 0.5, -0.25]).view(D, 1)
    for tot in (S.sum(0), None):
        for cr in (0, 4):
            t4, a4 = rowwise.exact_quarters(rowptr, col, code, S, lut, tot, cr)
            truth, _ = rowwise.reference(rowptr, col, code, S, lut, None, tot, reduce_cr=cr)
            assert int(a4.max()) < 2 ** 24 and np.array_equal(t4.numpy() / 4.0, truth)


# ---- the launch query, host only ---------------------------------------------------------------------------------------------------
def _describe(g, S, lut, use_cnt, with_rest, lmax=4, reduce_cr=0):
    """What aggregate.spmm_launch hands the library for a wide call over the degree-sorted copy, on host memory (the query reads no
    device memory and starts no GPU work)."""
    from gnan_amd import _lib, aggregate
    copy, order, plan = g.degree_sorted_copy()
    out = torch.empty((g.n_rows, reduce_cr or S.shape[1]), dtype=torch.float32)
    s_total = S.float().sum(0) if with_rest else None
    a = aggregate._spmm_args(copy, S, lut, use_cnt, s_total, out, order, lut.dim() == 3, plan=plan, reduce_cr=reduce_cr,
                             scatter_out=2, packed=True)
    runs = copy.short_row_runs(lmax)
    if a.packed_index:
        a.short_lmax, a.short_row, a.short_pair = runs.lmax, runs.row_ptr, runs.pair_ptr
    info = _lib.SpmmLaunchInfo()
    _lib.check(_lib.lib().gnan_spmm_fwd_describe(a, info), "gnan_spmm_fwd_describe")
    return info.as_dict(), np.diff(copy.rowptr.numpy())


@pytest.mark.parametrize("W", [32, 36, 40, 50, 60, 64, 100, 128, 200, 256, 320])
@pytest.mark.parametrize("lmax", [1, 4, 8])
def test_launch_query_reports_the_tile_partition(W, lmax):
    from gnan_amd import _lib
    rng = np.random.default_rng(W + lmax)
    n, D = 3000, 3
    g = _cpu_graph(*rowwise.short_csr(n, rng, D), n, D, torch.int32 if W % 8 else torch.int64)
    S = torch.zeros((n, W))
    lut = torch.ones((D, 1))
    info, deg = _describe(g, S, lut, True, True, lmax)
    vec = 4 if W % 4 == 0 else 1
    lpr = rowwise.lanes_per_row(W, vec)
    assert (info["vec"], info["lpr"], info["smalld"], info["dense"], info["kernel"]) == (vec, lpr, 1, 0, _lib.SPMM_KERNEL_ROWS)
    assert info["classed"] == 0 and info["n_slice_blocks"] == 3           # the rows of 513, 600 and 2000 pairs: one slice of at most 2048 pairs each
    served = vec == 4 and 32 < W <= 256
    if served:
        n_tiles, q0, first = rowwise.tile_partition(deg, lpr, lmax)
        assert n_tiles > 0
        assert (info["n_tiles"], info["row_q0"], info["short_tile"][:lmax + 1]) == (n_tiles, q0, first)
        assert info["n_tile_blocks"] == -(-n_tiles // 4)
    else:
        assert (info["n_tiles"], info["n_tile_blocks"], info["row_q0"]) == (0, 0, 0) and not any(info["short_tile"])


def test_launch_query_declines_what_the_tiles_do_not_serve_and_validates():
    from gnan_amd import _lib
    rng = np.random.default_rng(1)
    n = 2000
    csr = rowwise.short_csr(n, rng, 3)
    g = _cpu_graph(*csr, n, 3)
    assert _describe(g, torch.zeros((n, 64)), torch.ones((3, 1)), True, True)[0]["n_tiles"] > 0
    bf = _describe(g, torch.zeros((n, 64), dtype=torch.bfloat16), torch.ones((3, 1)), True, True)[0]
    assert (bf["vec"], bf["lpr"], bf["n_tiles"], bf["row_q0"]) == (8, 8, 0, 0)                # bf16 rows are declined
    assert _describe(g, torch.zeros((n, 64)), torch.ones((3, 2)), True, True)[0]["n_tiles"] == 0          # two weight channels
    g6 = _cpu_graph(*rowwise.short_csr(n, rng, 6), n, 6)
    d6 = _describe(g6, torch.zeros((n, 64)), torch.ones((6, 1)), True, True)[0]
    assert (d6["smalld"], d6["n_tiles"]) == (0, 0)                                              # no packed index beyond four codes
    lib = _lib.lib()
    info = _lib.SpmmLaunchInfo()
    assert lib.gnan_spmm_fwd_describe(_lib.SpmmArgs(n_rows=4, n_cols=4, W=0, D=2, Cw=1), info) == -1
    assert b"W must be" in lib.gnan_last_error()
    assert lib.gnan_spmm_fwd_describe(_lib.SpmmArgs(n_rows=0, n_cols=4, W=8, D=2, Cw=1), info) == 0
    assert info.kernel == _lib.SPMM_KERNEL_NONE and info.n_tiles == 0


def test_a_stand_in_launch_is_named_the_query_only_when_it_is_asked_for():
    """rho_aggregate and pre_rho_aggregate hand ``describe=`` on only when the caller gave one: a stand-in of spmm_launch written
    before the keyword (tests/cpu_kernels.py as it stood before the query existed) keeps serving every call that asks for no
    query, forward and backward.  The real launch is back in place afterwards, which is asserted."""
    from gnan_amd import aggregate
    real = aggregate.spmm_launch
    rng = np.random.default_rng(4)
    n, W, D = 300, 8, 3
    rowptr, col, code = rowwise.short_csr(n, rng, D, hubs=((7, 600),))
    g = _cpu_graph(rowptr, col, code, n, D)
    undo = cpu_kernels.install()
    try:
        def old_launch(g, S, lut, use_cnt, with_rest, row_ids=None, weight_by_col=False, minus_rest=False, s_total=None,
                       reduce_cr=0, s_by_code=False, lut_of_counts=None, lut_channels=1, room=None, keep_shell=None):
            return cpu_kernels.spmm_launch(g, S, lut, use_cnt, with_rest, row_ids, weight_by_col, minus_rest, s_total, reduce_cr,
                                           s_by_code, lut_of_counts, lut_channels, room, keep_shell)
        aggregate.spmm_launch = old_launch                        # (undo() below puts back what install() found: the real one)
        S = torch.from_numpy(rng.standard_normal((n, W)).astype(np.float32)).requires_grad_()
        lut = torch.from_numpy(rng.standard_normal((D, 1)).astype(np.float32)).requires_grad_()
        tot = S.detach().sum(0)                                   # handed in, so that its own rounding is an input of the bound
        y = aggregate.rho_aggregate(g, S, lut, True, True, s_total=tot)
        truth, bound = rowwise.reference(rowptr, col, code, S.detach(), lut.detach(), g.cnt.numpy(), tot)
        rowwise.assert_within(y.detach(), truth, bound, "rho_aggregate over the stand-in")
        y.sum().backward()
        assert S.grad is not None and lut.grad is not None
        with pytest.raises(TypeError, match="describe"):         # asked for, the query is not dropped silently
            aggregate.rho_aggregate(g, S.detach(), lut.detach(), True, True, describe=[])
    finally:
        undo()
    assert aggregate.spmm_launch is real and real is not cpu_kernels.spmm_launch
