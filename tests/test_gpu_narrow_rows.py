"""The narrow aggregation (W in {1, 2, 4}) row by row, forward and backward, against tests/rowwise.py.

Forward: ``gnan_spmm_pb_fwd`` (pb_expand_kernel + pb_reduce_kernel) inside ``rowwise.pb_reference``'s bound on EVERY element, its kept
shell sums equal to ``rowwise.pb_shell_exact`` BIT FOR BIT (no tolerance: pins to_fixed, the shift, the absmax pass, the slot sums of
hub rows and the coverage of tiles, bins and column blocks), scale equivariance by 2^+-100 bit for bit, exact integer cases; the
row-parallel narrow routes (natural order, the sorted copy, spmm_hot_kernel, s_by_code) on the same graphs and operands inside
``rowwise.reference(hub_threshold=64)``, the route asserted through the launch query.  Backward through ``rho_aggregate`` and autograd:
``gnan_spmm_pb_pack1`` + the PB phases over the transposed graph, ``gnan_spmm_pb_bwd``, ``gnan_spmm_bwd_narrow`` /
``spmm_bwd_hot_kernel`` inside ``rowwise.narrow_bwd_reference``, the route asserted by which launch ran.

Operand families (``rowwise.narrow_operand``): unit, range (rows over 2^-40 .. 2^10), outlier (2^60 in a row no pair lists: absmax is
taken over the whole operand and the small rows may lose every digit — the contract), same-sign (every entry the float below 2: row
sums of L max |S|, the most the headroom must hold; it CANNOT see a headroom one bit short, because the sums are scaled to 2^62 and an
int64 has one more bit), zeros, integers, and unit scaled by 2^+-100."""
import numpy as np
import pytest
import torch

import rowwise
from gnan_amd import aggregate

pytestmark = pytest.mark.gpu
DEV = "cuda"
FWD_FAMILIES = ("unit", "range", "outlier", "same-sign", "same-sign-neg", "zeros", "integers")


def _dev_graph(rowptr, col, code, n_cols, D, cnt=None):
    from gnan_amd import HopGraph
    return HopGraph.from_csr(torch.from_numpy(rowptr).to(DEV), torch.from_numpy(col).to(DEV), torch.from_numpy(code).to(DEV),
                             n_cols=n_cols, n_codes=D, cnt=None if cnt is None else torch.from_numpy(cnt).to(DEV))


def _small_lds(monkeypatch, W):
    from gnan_amd import graph as G
    monkeypatch.setattr(G, "PB_LDS_BYTES", 1024 * W)          # 128 accumulators per bin, 256 operand rows per column block
    monkeypatch.setattr(G, "PB_SLOT_PAIRS", 8)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _pb_forward(g, plan, csr, S, lut, use_cnt, with_rest, what, ratios):
    """One operand through gnan_spmm_pb_fwd: the bound on every element, the same bits twice, the exact shell sums, the routed call."""
    from gnan_amd import functional as Fn
    from gnan_amd.aggregate import pb_launch, spmm_launch
    rowptr, col, code = csr
    Sd = torch.from_numpy(S).to(DEV)
    tot = Fn.column_sums(Sd) if with_rest else None
    lutd = torch.from_numpy(lut).to(DEV)
    got = pb_launch(g, plan, Sd, lutd, use_cnt, tot)
    again = pb_launch(g, plan, Sd, lutd, use_cnt, tot)
    assert torch.equal(_bits(got), _bits(again)), what
    truth, bound = rowwise.pb_reference(rowptr, col, code, S, lut, g.cnt.cpu() if use_cnt else None, None if tot is None else tot.cpu(),
                                        plan.headroom_bits, plan.code_base)
    ratio = rowwise.assert_within(got.cpu(), truth, bound, what)
    ratios[what] = ratio
    if S.shape[1] == 1 and plan.n_acc == 1:
        shell = torch.full((g.n_rows,), float("nan"), device=DEV)
        kept = pb_launch(g, plan, Sd, lutd, use_cnt, tot, shell_out=shell)
        assert torch.equal(_bits(kept), _bits(got)), what
        want = rowwise.pb_shell_exact(rowptr, col, code, S, plan.headroom_bits, plan.code_base)
        diff = np.nonzero(shell.cpu().numpy().view(np.uint32) != want.view(np.uint32))[0]
        assert diff.size == 0, f"{what}: shell_out differs from the exact fixed-point sum in {diff.size} rows, first {int(diff[0])}: " \
                               f"{shell.cpu().numpy()[diff[0]]!r} != {want[diff[0]]!r}"
    routed = spmm_launch(g, Sd, lutd, use_cnt, with_rest, s_total=tot)               # (PB_MIN_NNZ = 0: the route takes the buckets)
    assert torch.equal(_bits(routed), _bits(got)), what
    return got, tot


@pytest.mark.parametrize("D,W,layout,use_cnt,with_rest,top,shape", rowwise.NARROW_CASES)
def test_pb_forward_row_bound_exact_shell_sums_and_scale(D, W, layout, use_cnt, with_rest, top, shape, monkeypatch):
    from gnan_amd.aggregate import pb_launch
    _small_lds(monkeypatch, W)
    monkeypatch.setattr(aggregate, "PB_MIN_NNZ", 0)
    rng = np.random.default_rng(D * 100 + W * 10 + top)
    n_rows, n_cols = shape
    csr = rowwise.narrow_csr(rng, n_rows, n_cols, D, layout, top)
    g = _dev_graph(*csr, n_cols, D)
    plan = g.pb_plan(W)
    assert plan is not None and plan.n_bins > 3 and plan.n_cblocks > 3
    if D > 2 and layout == "self":
        assert plan.code_base == 1 and plan.self_is_row == (n_rows <= n_cols)
    if D == 2 or layout == "double":
        assert plan.code_base == 0 and plan.self_col is None
    if D > 2 and layout == "none":
        assert plan.code_base == 1 and int(plan.self_col.max()) == -1
    lut = rng.standard_normal((D, 1)).astype(np.float32)
    ratios = {}
    for fam in FWD_FAMILIES:
        S = rowwise.narrow_operand(rng, fam, n_cols, W)
        got, tot = _pb_forward(g, plan, csr, S, lut, use_cnt, with_rest, fam, ratios)
        if fam == "zeros":
            assert not bool(got.any())
        if fam == "unit":                                      # scale equivariance: a power of two moves the exponents and nothing else
            for k in (100, -100):
                f = float(2.0 ** k)
                scaled = pb_launch(g, plan, torch.from_numpy(S).to(DEV) * f, torch.from_numpy(lut).to(DEV), use_cnt,
                                   None if tot is None else tot * f)
                assert torch.equal(_bits(scaled), _bits(got * f)), f"unit * 2^{k}"
    print("NARROW-PB", (D, W, layout, top, shape), {k: round(v, 3) for k, v in ratios.items()})


@pytest.mark.parametrize("W", [1, 2, 4])
def test_pb_forward_at_the_real_lds_size(W, monkeypatch):
    """64 KB of LDS: 20 000 x 40 000 with a hub row of 3 000 pairs: several bins, several column blocks, multi-slot rows of 512."""
    monkeypatch.setattr(aggregate, "PB_MIN_NNZ", 0)
    D, n_rows, n_cols = 3, 20_000, 40_000
    rng = np.random.default_rng(50 + W)
    csr = rowwise.narrow_csr(rng, n_rows, n_cols, D, "self", 3000, hubs=rowwise.NARROW_HUBS + ((1234, 513), (19_999, 3000)))
    g = _dev_graph(*csr, n_cols, D)
    plan = g.pb_plan(W)
    assert plan is not None and plan.n_bins >= 2 and plan.n_cblocks >= 3 and plan.headroom_bits == 12
    assert int((plan.slot_ptr[1:] - plan.slot_ptr[:-1]).max()) == 6
    lut = rng.standard_normal((D, 1)).astype(np.float32)
    ratios = {}
    for fam in ("unit", "range", "outlier", "same-sign"):
        _pb_forward(g, plan, csr, rowwise.narrow_operand(rng, fam, n_cols, W), lut, True, True, fam, ratios)
    print("NARROW-PB 64KB", W, {k: round(v, 3) for k, v in ratios.items()})


EXACT = [(3, 1, "self", True, 150), (4, 2, "none", True, 129), (2, 4, "self", False, 65), (4, 1, "double", True, 128), (3, 4, "moved", True, 64),
         (3, 2, "some", False, 150)]


def _row_routes(monkeypatch):
    """The row-parallel narrow routes as ``(name, settings, kernel the launch query must report)``."""
    from gnan_amd import _lib, graph as G
    monkeypatch.setattr(aggregate, "PB_NARROW", False)
    monkeypatch.setattr(G, "HOT_COLUMNS", 64)
    monkeypatch.setattr(G, "HOT_COLUMNS_MIN", 32)              # (fewer than 1024 neighbour nodes: the copy holds the 32 most listed)
    monkeypatch.setattr(G, "HOT_COLUMNS_MIN_NNZ", 0)
    monkeypatch.setattr(aggregate, "DEGREE_SORTED_COPY_MIN_ROWS", 1)
    monkeypatch.setattr(aggregate, "NARROW_SORTED_MIN_NNZ", 0)
    return [("natural", (False, False), _lib.SPMM_KERNEL_ROWS), ("sorted", (True, False), _lib.SPMM_KERNEL_ROWS),
            ("hot", (True, True), _lib.SPMM_KERNEL_HOT)]


def _run_route(monkeypatch, g, settings, Sd, lutd, use_cnt, with_rest, tot, **kw):
    monkeypatch.setattr(aggregate, "NARROW_SORTED_WALK", settings[0])
    monkeypatch.setattr(aggregate, "HOT_COLUMN_ROWS", settings[1])
    d = []
    y = aggregate.spmm_launch(g, Sd, lutd, use_cnt, with_rest, s_total=tot, describe=d, **kw)
    assert len(d) == 1
    return y, d[0]


ROW_CASES = [c for c in rowwise.NARROW_CASES if c[5] in (150, 129) or c[0] == 2]


@pytest.mark.parametrize("D,W,layout,use_cnt,with_rest,top,shape", ROW_CASES)
def test_row_parallel_narrow_routes_meet_the_row_bound(D, W, layout, use_cnt, with_rest, top, shape, monkeypatch):
    """PB_NARROW off: the W <= 4 row walks (rows of more than 64 pairs in slices for one or two lanes per row) in natural order, over
    the sorted copy, through spmm_hot_kernel (HOT_COLUMNS = 64, the hot rows in LDS) and with one operand row per (node, hop code).
    A float chain has no absolute term: gamma_k A row by row on the outlier and range families too."""
    from gnan_amd import functional as Fn
    rng = np.random.default_rng(D * 100 + W * 10 + top + 1)
    n_rows, n_cols = shape
    csr = rowwise.narrow_csr(rng, n_rows, n_cols, D, layout, top)
    rowptr, col, code = csr
    g = _dev_graph(*csr, n_cols, D)
    routes = _row_routes(monkeypatch)
    lut = rng.standard_normal((D, 1)).astype(np.float32)
    lutd = torch.from_numpy(lut).to(DEV)
    ratios = {}
    for fam in ("unit", "range", "outlier", "zeros"):
        S = rowwise.narrow_operand(rng, fam, n_cols, W)
        Sd = torch.from_numpy(S).to(DEV)
        tot = Fn.column_sums(Sd) if with_rest else None
        truth, bound = rowwise.reference(rowptr, col, code, S, lut, g.cnt.cpu() if use_cnt else None, None if tot is None else tot.cpu(),
                                         hub_threshold=64)
        for name, settings, kernel in routes:
            y, info = _run_route(monkeypatch, g, settings, Sd, lutd, use_cnt, with_rest, tot)
            assert info["kernel"] == kernel, (name, info)
            again, _ = _run_route(monkeypatch, g, settings, Sd, lutd, use_cnt, with_rest, tot)
            assert torch.equal(_bits(y), _bits(again)), (name, fam)
            ratios[name, fam] = rowwise.assert_within(y.cpu(), truth, bound, f"{name} {fam}")
        # one operand row per (node, hop code): the pair (c, d) reads row c D + d — no counts, no rest bucket
        Sb = rowwise.narrow_operand(rng, fam, n_cols * D, W)
        tb, bb = rowwise.reference(rowptr, col.astype(np.int64) * D + code, code, Sb, lut, None, None, hub_threshold=64)
        yb, info = _run_route(monkeypatch, g, (True, True), torch.from_numpy(Sb).to(DEV), lutd, False, False, None, s_by_code=True)
        assert info["kernel"] == routes[0][2]
        ratios["s_by_code", fam] = rowwise.assert_within(yb.cpu(), tb, bb, f"s_by_code {fam}")
    assert g._sorted_copy_hot is not None and g._sorted_copy_hot.n_cols == n_cols + 32
    print("NARROW-ROWS", (D, W, layout, top, shape), {f"{a}/{b}": round(v, 3) for (a, b), v in ratios.items()})


@pytest.mark.parametrize("D,W,layout,with_rest,top", EXACT)
@pytest.mark.parametrize("weights", ["quarters", "sixteenths"])
def test_integer_cases_are_exact_on_every_forward_route(D, W, layout, with_rest, top, weights, monkeypatch):
    """Integer operand, weights in quarters — in sixteenths through counts of 1, 2 and 4: no tolerance on any route."""
    from gnan_amd.aggregate import pb_launch
    _small_lds(monkeypatch, W)
    rng = np.random.default_rng(D + W + top)
    n_rows, n_cols = 700, 900
    csr = rowwise.narrow_csr(rng, n_rows, n_cols, D, layout, top)
    rowptr, col, code = csr
    cnt = (2 ** rng.integers(0, 3, (n_rows, D))).astype(np.int32) if weights == "sixteenths" else None
    g = _dev_graph(*csr, n_cols, D, cnt=cnt)
    S = rowwise.narrow_operand(rng, "integers", n_cols, W)
    lut = (rng.integers(-8, 9, (D, 1)) / 4.0).astype(np.float32)
    Sd, lutd = torch.from_numpy(S).to(DEV), torch.from_numpy(lut).to(DEV)
    tot = torch.from_numpy(S.sum(0)).to(DEV) if with_rest else None
    scale = 4 if cnt is None else 16
    t, a = rowwise.exact_scaled(rowptr, col, code, S, lut, None if tot is None else tot.cpu(), 0, cnt, scale)
    assert int(a.max()) < 2 ** 24
    want = t.double() / scale
    y = pb_launch(g, g.pb_plan(W), Sd, lutd, cnt is not None, tot)
    assert torch.equal(y.cpu().double(), want), "gnan_spmm_pb_fwd"
    for name, settings, kernel in _row_routes(monkeypatch):
        y, info = _run_route(monkeypatch, g, settings, Sd, lutd, cnt is not None, with_rest, tot)
        assert info["kernel"] == kernel, (name, info)
        assert torch.equal(y.cpu().double(), want), name
    Sb = rowwise.narrow_operand(rng, "integers", n_cols * D, W)
    tb, _ = rowwise.exact_scaled(rowptr, col.astype(np.int64) * D + code, code, Sb, lut, None, 0, None, 4)
    yb, _ = _run_route(monkeypatch, g, (True, True), torch.from_numpy(Sb).to(DEV), lutd, False, False, None, s_by_code=True)
    assert torch.equal(yb.cpu().double(), tb.double() / 4), "s_by_code"


# =====================================================================================================================================
# backward, through rho_aggregate and autograd
# =====================================================================================================================================
BWD_HUBS = rowwise.NARROW_HUBS + tuple((40 * k + 3, 100) for k in range(1, 21))        # the transposed graph's most listed nodes
# (D, W, layout, use_cnt, with_rest, PB_NARROW, PB_BACKWARD_ONE_COLUMN, hot packed rows, the launch that must run)
BWD_CASES = [
    (3, 1, "self", True, True, True, True, False, "pb1"), (3, 1, "self", False, False, True, True, False, "pb1"),
    # (a graph without code-0 pairs still has code_base 1 in both plans — self_col is all -1 — and keeps its shell sums: pack1)
    (3, 1, "some", True, True, True, True, False, "pb1"), (3, 1, "none", True, True, True, True, False, "pb1"),
    (3, 1, "self", True, True, True, False, False, "pb2"), (2, 1, "self", True, True, True, True, False, "pb2"),
    # without the rest bucket M[j] has no term shared by every row: only there can a row of small dY see the buckets' quantum
    (3, 1, "self", True, False, True, False, False, "pb2"), (3, 1, "self", False, False, True, False, False, "pb2"),
    (2, 1, "self", False, False, True, True, False, "pb2"), (3, 1, "none", True, False, True, False, False, "pb2"),
    # (moved self pairs: some transposed row lists two code-0 pairs, its plan buckets code 0, two accumulated codes: the row walk)
    (3, 1, "moved", True, False, True, False, False, "rows"), (4, 1, "self", True, True, True, True, False, "rows"),
    (3, 1, "self", True, True, False, True, False, "rows"), (3, 1, "self", True, True, False, True, True, "rows"),
    (4, 2, "some", True, True, False, True, False, "rows"), (3, 2, "self", False, True, False, True, True, "rows"),
    (4, 4, "none", True, False, False, True, False, "rows"), (2, 4, "self", True, True, False, True, True, "rows"),
]


def _upstream(rng, family, n, W):
    dY = rng.standard_normal((n, W)).astype(np.float32)
    if family == "masked":
        dY[rng.random(n) < 0.7] = 0.0
    elif family == "range":
        dY = (dY * np.exp2(rng.integers(-40, 11, (n, 1)).astype(np.float64))).astype(np.float32)
    elif family == "integers":
        dY = rng.integers(-4, 5, (n, W)).astype(np.float32)
    return dY


def _backward_setup(monkeypatch, D, W, layout, pb_narrow, one_column, hot, n, cnt_pow2=False, seed=0, cnt_agree=False):
    from gnan_amd import graph as G
    _small_lds(monkeypatch, 2)                                 # (2048 bytes, as the existing backward test: plans of W = 1 and W = 2)
    monkeypatch.setattr(aggregate, "PB_MIN_NNZ", 0)
    monkeypatch.setattr(aggregate, "PB_NARROW", pb_narrow)
    monkeypatch.setattr(aggregate, "PB_BACKWARD_ONE_COLUMN", one_column)
    if hot:
        monkeypatch.setattr(G, "HOT_COLUMNS", 64)
        monkeypatch.setattr(G, "HOT_COLUMNS_MIN", 32)
        monkeypatch.setattr(G, "HOT_COLUMNS_MIN_NNZ", 0)
        monkeypatch.setattr(aggregate, "NARROW_SORTED_MIN_NNZ", 0)
        monkeypatch.setattr(aggregate, "DEGREE_SORTED_COPY_MIN_ROWS", 1)
    ran = []
    for name, tag in (("pb_bwd1_launch", "pb1"), ("pb_bwd_launch", "pb2"), ("bwd_narrow_launch", "rows"), ("rows_bwd1_launch", "rows1")):
        real = getattr(aggregate, name)
        monkeypatch.setattr(aggregate, name, lambda *a, _r=real, _t=tag, **k: ran.append(_t) or _r(*a, **k))
    rng = np.random.default_rng(seed)
    csr = rowwise.narrow_csr(rng, n, n, D, layout, 150, hub_share=0.25, hubs=BWD_HUBS, reserve=False)
    cnt = (2 ** rng.integers(0, 3, (n, D))).astype(np.int32) if cnt_pow2 else None
    if cnt_agree:                                              # count columns 0 and 1 agree in all but 2 % of the rows
        cnt = rng.integers(1, 9, (n, D)).astype(np.int32)
        cnt[:, 1] = cnt[:, 0]
        differ = rng.random(n) < 0.02
        cnt[differ, 1] += rng.integers(1, 5, int(differ.sum())).astype(np.int32)
    g = _dev_graph(*csr, n, D, cnt=cnt)
    return rng, csr, g, ran


def _grads(g, S0, lut0, up, use_cnt, with_rest, tot):
    S, lut = S0.clone().requires_grad_(True), lut0.clone().requires_grad_(True)
    return torch.autograd.grad(aggregate.rho_aggregate(g, S, lut, use_cnt, with_rest=with_rest, s_total=tot), [S, lut], up)


def _plan_bits(g, route):
    """(headroom of the transposed plan, its code base, headroom of the forward plan) for the PB routes."""
    if route == "pb1":
        f, t = g.pb_plan(1), g.transposed().pb_plan(1)
        return t.headroom_bits, t.code_base, f.headroom_bits
    if route == "pb2":
        t = g.transposed().pb_plan(2)
        return t.headroom_bits, t.code_base, 0
    return 0, 0, 0


@pytest.mark.parametrize("D,W,layout,use_cnt,with_rest,pb_narrow,one_column,hot,expect", BWD_CASES)
def test_narrow_backward_meets_the_row_bound_on_every_route(D, W, layout, use_cnt, with_rest, pb_narrow, one_column, hot, expect, monkeypatch):
    from gnan_amd import functional as Fn
    n = 900
    rng, csr, g, ran = _backward_setup(monkeypatch, D, W, layout, pb_narrow, one_column, hot, n, seed=D * 100 + W * 10 + len(layout) + hot)
    rowptr, col, code = csr
    assert int(np.bincount(col, minlength=n).max()) > 64                      # hub rows of the transposed graph
    S = rowwise.narrow_operand(rng, "unit", n, W)
    lut = rng.standard_normal((D, 1)).astype(np.float32)
    S0, lut0 = torch.from_numpy(S).to(DEV), torch.from_numpy(lut).to(DEV)
    tot = Fn.column_sums(S0) if with_rest else None
    cnt = g.cnt.cpu() if use_cnt else None
    ratios = {}
    for fam in ("unit", "masked", "range"):
        dY = _upstream(rng, fam, n, W)
        up = torch.from_numpy(dY).to(DEV)
        del ran[:]
        got = _grads(g, S0, lut0, up, use_cnt, with_rest, tot)
        route = ran[-1] if ran else None
        assert ran == [expect], (ran, expect)
        again = _grads(g, S0, lut0, up, use_cnt, with_rest, tot)
        assert torch.equal(_bits(got[0]), _bits(again[0])) and torch.equal(_bits(got[1]), _bits(again[1])), fam
        ht, base, hf = _plan_bits(g, route)
        dS, dSb, dl, dlb = rowwise.narrow_bwd_reference(rowptr, col, code, S, lut, cnt, dY, None if tot is None else tot.cpu(), route,
                                                        ht, base, hf)
        ratios[fam, "dS"] = rowwise.assert_within(got[0].cpu(), dS, dSb, f"dS {route} {fam}")
        ratios[fam, "dlut"] = rowwise.assert_within(got[1].cpu().reshape(-1, 1), dl.reshape(-1, 1), dlb.reshape(-1, 1), f"dlut {route} {fam}")
        if fam == "masked" and not with_rest:
            listers = np.zeros(n)
            np.add.at(listers, col, np.abs(dY[np.repeat(np.arange(n), np.diff(rowptr))]).sum(1))
            dead = listers == 0
            assert dead.any() and not bool(got[0].cpu()[torch.from_numpy(dead)].any()), "a row whose listers are all masked must be exactly 0"
    if hot:
        gt = g.transposed()
        assert gt._sorted_copy_hot is not None and gt._sorted_copy_hot.n_cols == n + 32
    print("NARROW-BWD", (D, W, layout, pb_narrow, one_column, hot), route, {f"{a}/{b}": round(v, 3) for (a, b), v in ratios.items()})


@pytest.mark.parametrize("D,W,layout,use_cnt,with_rest,pb_narrow,one_column,hot,expect", BWD_CASES)
def test_narrow_backward_integer_cases_are_exact(D, W, layout, use_cnt, with_rest, pb_narrow, one_column, hot, expect, monkeypatch):
    """Integer operand and upstream gradient, weights in quarters (sixteenths through counts of 1, 2, 4): dS and dlut with no tolerance."""
    n = 900
    rng, csr, g, ran = _backward_setup(monkeypatch, D, W, layout, pb_narrow, one_column, hot, n, cnt_pow2=use_cnt, seed=7 + D + W)
    rowptr, col, code = csr
    S = rowwise.narrow_operand(rng, "integers", n, W)
    dY = _upstream(rng, "integers", n, W)
    lut = (rng.integers(-8, 9, (D, 1)) / 4.0).astype(np.float32)
    tot = torch.from_numpy(S.sum(0)).to(DEV) if with_rest else None
    got = _grads(g, torch.from_numpy(S).to(DEV), torch.from_numpy(lut).to(DEV), torch.from_numpy(dY).to(DEV), use_cnt, with_rest, tot)
    assert ran == [expect], (ran, expect)
    mags = []
    dS, _, dl, _ = rowwise.narrow_bwd_reference(rowptr, col, code, S, lut, g.cnt.cpu() if use_cnt else None, dY,
                                                None if tot is None else tot.cpu(), "rows", magnitudes=mags)
    assert float(mags[0].max()) * 16 < 2 ** 24 and float(mags[1].max()) * 16 < 2 ** 24      # the sums of |terms|: exact in any order
    assert np.array_equal(got[0].cpu().double().numpy(), dS), ran
    assert np.array_equal(got[1].cpu().double().numpy().reshape(-1), dl), ran


@pytest.mark.parametrize("one_column", [True, False])
def test_one_column_backward_reads_each_codes_own_count(one_column, monkeypatch):
    """The self pair's gradient is dY_i / cnt(i, 0), the accumulated code's dY_i / cnt(i, 1).  Count columns that agree in all but 2 % of
    the rows confine a mix-up of the two to those rows: the largest entry of the result does not move, the rows' own bounds do."""
    from gnan_amd import functional as Fn
    n, D = 900, 3
    rng, csr, g, ran = _backward_setup(monkeypatch, D, 1, "self", True, one_column, False, n, seed=31, cnt_agree=True)
    rowptr, col, code = csr
    S = rowwise.narrow_operand(rng, "unit", n, 1)
    dY = _upstream(rng, "unit", n, 1)
    lut = rng.standard_normal((D, 1)).astype(np.float32)
    S0 = torch.from_numpy(S).to(DEV)
    tot = Fn.column_sums(S0)
    got = _grads(g, S0, torch.from_numpy(lut).to(DEV), torch.from_numpy(dY).to(DEV), True, True, tot)
    route = "pb1" if one_column else "pb2"
    assert ran == [route]
    ht, base, hf = _plan_bits(g, route)
    dS, dSb, dl, dlb = rowwise.narrow_bwd_reference(rowptr, col, code, S, lut, g.cnt.cpu(), dY, tot.cpu(), route, ht, base, hf)
    rowwise.assert_within(got[0].cpu(), dS, dSb, f"dS {route}")
    rowwise.assert_within(got[1].cpu().reshape(-1, 1), dl.reshape(-1, 1), dlb.reshape(-1, 1), f"dlut {route}")
