"""The reference-order inference route (``aggregate.reference_order_inference``): the look-up's row sums and kept rows
(``gnan_fpwl_args.row_sum / row_keep``), the aggregation's self term (``gnan_spmm_args.self_sum``) over the self-free twin, and the
module.  About 3 000 rows; the gates that keep small graphs off the route are lowered as tests/test_gpu_wide_rows.py lowers them.

Per-row bound of the aggregation (derived in tests/test_self_free_plan.py, which holds a float32 emulation of the same chain to
it): a term of the truth meets at most

    k_i = max( L_i + 15,  6 + log2(TPN) + parts )        L_i the row's pairs in the ORIGINAL graph, its self pair included

roundings — a gathered term: 2 divisions and the fold (3), the fmaf chain over the twin's L_i - 1 pairs, fmaf(w_rest, tot) (1),
at most 4 in-lane adds and 6 butterfly steps of the read-out (10), the self fmaf (1); a self term: 3 in-lane adds and log2(TPN)
butterfly steps of the look-up's sum, parts - 1 adds of the parts (rows_body / short_tile / the fix-up: ``self_term``), the folded
weight (3), the self fmaf (1).  Hub rows of the twin (more than 512 pairs): 2 (L_i - 1) + 11 for the gathered terms.  Truth and
magnitude are ``rowwise.reference``'s for the ORIGINAL graph: |y - t| <= gamma_k A, a zero bound demands an exact zero, no row is
left out."""
import numpy as np
import pytest
import torch

import rowwise
from test_gpu_kernels import _graph, _mlp_state, _stack
from test_self_free_plan import lookup_row_sums, self_graph, self_row_bound

pytestmark = pytest.mark.gpu
DEV = "cuda"
N = 3001                                     # not a multiple of the look-up's node block (256) nor of a tile's rows
TWIN_LENGTHS = [0, 1, 2, 3, 4, 5, 9, 40]
HUB = (77, 600)                              # (row, pairs in the twin): over the slice threshold of 512


def _lower(monkeypatch, classed=False):
    from gnan_amd import _lib, aggregate
    from gnan_amd import functional as Fn
    monkeypatch.setattr(aggregate, "DEGREE_SORTED_COPY_MIN_ROWS", 1)
    monkeypatch.setattr(aggregate, "SELF_FROM_LOOKUP_MIN_ROWS", 0)
    monkeypatch.setattr(aggregate, "CLASSED_MIN_NNZ", 1 if classed else 1 << 40)
    monkeypatch.setattr(Fn, "FMLP_ALGO", _lib.FMLP_PWL)
    monkeypatch.setattr(Fn, "INDEX_MIN_NODES", 0)
    Fn._RANGE_CHURN.clear()


_CSR = {}


def _csr(D=3):
    """Every row: its self pair (code 0, in the middle) and 0, 1, 2, 3, 4, 5, 9 or 40 others, one hub row; a third of the nodes (ids
    = 0 mod 3, the last node among them) are listed by no other row."""
    if D not in _CSR:
        rng = np.random.default_rng(D)
        lengths = rng.choice(TWIN_LENGTHS, N)
        lengths[HUB[0]] = HUB[1]
        pool = np.arange(N)[np.arange(N) % 3 != 0]
        _CSR[D] = self_graph(rng, N, N, "middle", lengths, D, listed_cols=pool)
    return _CSR[D]


def _plan(g):
    plan = g.self_free_plan(strict=False)
    assert plan is not None and plan.strict
    return plan


def _listed(plan):
    return torch.from_numpy(np.unpackbits(plan.listed.cpu().numpy().view(np.uint8), bitorder="little")[:N].astype(bool))


# ---- the look-up ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,parts", [(32, 1), (48, 3), (64, 2)])
def test_lookup_stores_listed_rows_only_and_hands_out_every_rows_sum(F, parts, monkeypatch):
    from gnan_amd import _lib
    from gnan_amd import functional as Fn
    _lower(monkeypatch)
    rowptr, col, code = _csr()
    plan = _plan(_graph(rowptr, col, code, N, 3))
    listed = _listed(plan)
    assert 0 < int(listed.sum()) < N and not bool(listed[N - 1])
    st = _stack(_mlp_state(F, 3, 16, 1, True, seed=F), F, 3, 16, 1, True)
    x = torch.randn(N, F, generator=torch.Generator().manual_seed(F)).to(DEV)
    with torch.no_grad():
        fx0, tables, tot0 = Fn._fmlp_forward(x, st, False, True)
        buf = torch.full((N, F), float("nan"), device=DEV)
        req = Fn.LookupRequest(out=buf, keep=plan.listed, skip_stores=True)
        fx1, _, tot1 = Fn._fmlp_forward(x, st, False, True, request=req)
    torch.cuda.synchronize()
    assert fx1 is buf and tables is not None and tot0 is not None
    assert req.row_sum is not None and tuple(req.row_sum.shape) == (parts, N)
    fx0c, fx1c = fx0.cpu(), fx1.cpu()
    assert torch.equal(fx1c[listed].view(torch.int32), fx0c[listed].view(torch.int32))        # listed rows: the plain call's bits
    assert bool(torch.isnan(fx1c[~listed]).all())                                               # unlisted rows: never written
    assert torch.equal(tot1.view(torch.int32), tot0.view(torch.int32))
    want = lookup_row_sums(fx0c.numpy(), F // parts)
    assert np.array_equal(req.row_sum.cpu().numpy().view(np.uint32), want.view(np.uint32))
    # modes that do not serve the fields refuse before their first launch: the output buffer stays as it was
    t = tables
    xr = Fn._rows(x)
    for mode in ("sum", "bf16", "search"):
        out = torch.full((N, 1 if mode == "sum" else F), float("nan"), device=DEV,
                         dtype=torch.bfloat16 if mode == "bf16" else torch.float32)
        a = Fn._fpwl_args(xr, t, mode == "sum", out)
        keep = Fn._fpwl_index(a, xr, t, Fn._feature_range(x)) if mode != "search" else None
        assert mode == "search" or keep is not None
        if mode == "bf16":
            a.out_dtype = _lib.GNAN_BF16
        a.row_keep = _lib.ptr(plan.listed)
        rc = _lib.lib().gnan_fpwl_fwd(a, _lib.stream_of(x))
        torch.cuda.synchronize()
        assert rc == _lib.ERR_UNSUPPORTED, (mode, rc)
        assert bool(torch.isnan(out.float()).all()), mode
        assert _lib.lib().gnan_fpwl_row_sum_parts(a) == 0


def test_one_request_reports_the_launch_that_received_it_last(monkeypatch):
    """One request handed to two look-ups in a row: the first has the feature range and is served by the direct index (row sums,
    listed rows only), the second has none and is not — its outcome is "no row sums, complete rows", not the first launch's buffer."""
    from gnan_amd import functional as Fn
    _lower(monkeypatch)
    F = 32
    rowptr, col, code = _csr()
    plan = _plan(_graph(rowptr, col, code, N, 3))
    st = _stack(_mlp_state(F, 3, 16, 1, True, seed=F), F, 3, 16, 1, True)
    x = torch.randn(N, F, generator=torch.Generator().manual_seed(F)).to(DEV)
    with torch.no_grad():
        _, tables, _ = Fn._fmlp_forward(x, st, False, True)
        plain = Fn._fpwl_launch(x, tables, False)
        buf = torch.full((N, F), float("nan"), device=DEV)
        req = Fn.LookupRequest(out=buf, keep=plan.listed, skip_stores=True)
        first = Fn._fpwl_launch(x, tables, False, x_range=Fn._feature_range(x), request=req)
        served = req.row_sum
        holes = bool(torch.isnan(buf).any())
        second = Fn._fpwl_launch(x, tables, False, x_range=None, request=req)
    torch.cuda.synchronize()
    assert first is buf and served is not None and tuple(served.shape) == (1, N) and holes
    assert req.row_sum is None and req.room is None
    assert second is buf and torch.equal(second.view(torch.int32), plain.view(torch.int32))


def test_out_rows_of_the_wrong_shape_are_left_alone(monkeypatch):
    """``feature_mlps(out=buf)``: rows that do not fit the result are not written and a fresh tensor comes back; rows that fit ARE
    the result; the next plain call allocates its own rows — nothing of the request outlives its call."""
    from gnan_amd import _lib
    from gnan_amd import functional as Fn
    monkeypatch.setattr(Fn, "FMLP_ALGO", _lib.FMLP_PWL)
    n, F = 300, 16
    st = _stack(_mlp_state(F, 3, 16, 1, True, seed=3), F, 3, 16, 1, True)
    x = torch.randn(n, F, generator=torch.Generator().manual_seed(3)).to(DEV)
    with torch.no_grad():
        want = Fn.feature_mlps(x, st, False)
        wrong = torch.full((n + 1, F), float("nan"), device=DEV)
        got = Fn.feature_mlps(x, st, False, out=wrong)
        fits = torch.full((n, F), float("nan"), device=DEV)
        into = Fn.feature_mlps(x, st, False, out=fits)
        after = Fn.feature_mlps(x, st, False)
    torch.cuda.synchronize()
    assert got.data_ptr() != wrong.data_ptr() and bool(torch.isnan(wrong).all())
    assert into.data_ptr() == fits.data_ptr() and after.data_ptr() not in (wrong.data_ptr(), fits.data_ptr())
    for rows in (got, fits, after):
        assert torch.equal(rows.view(torch.int32), want.view(torch.int32))


# ---- the aggregation ----------------------------------------------------------------------------------------------------------------
def _host_parts(S, parts):
    """Row sums of ``S`` per block of ``W / parts`` columns, in the look-up's association."""
    return torch.from_numpy(lookup_row_sums(np.ascontiguousarray(S.numpy()), S.shape[1] // parts))


@pytest.mark.parametrize("W,parts", [(48, 3), (64, 2), (256, 8)])
@pytest.mark.parametrize("classed", [False, True])
def test_exact_integer_cases_equal_the_original_graph(W, parts, classed, monkeypatch):
    """Weights in quarters, S integers in [-4, 4] (the operands of tests/test_gpu_wide_rows.py's exact cases): float32 is exact in any
    order, so the twin with the self term equals the original graph and the int64 restatement, through tiles, row walk and hub slices."""
    from gnan_amd import _lib, aggregate
    from gnan_amd import functional as Fn
    _lower(monkeypatch, classed)
    D = 3
    rowptr, col, code = _csr()
    g = _graph(rowptr, col, code, N, D)
    plan = _plan(g)
    rng = np.random.default_rng(W)
    S = torch.from_numpy(rng.integers(-4, 5, (N, W)).astype(np.float32))
    lut = torch.tensor([2.0, -1.0, 0.5]).view(D, 1)
    Sd = S.to(DEV)
    s_total = Fn.column_sums(Sd)
    t4, a4 = rowwise.exact_quarters(rowptr, col, code, S, lut, s_total.cpu(), 1)
    assert int(a4.max()) < 2 ** 24
    want = (t4.double() / 4).float()
    self_sum = _host_parts(S, parts).to(DEV)
    d0, d1, d2 = [], [], []
    y0 = aggregate.spmm_launch(g, Sd, lut.to(DEV), False, True, s_total=s_total, reduce_cr=1, describe=d0)
    y1 = aggregate.spmm_launch(plan.twin, Sd, lut.to(DEV), False, True, s_total=s_total, reduce_cr=1, describe=d1, self_sum=self_sum)
    y2 = aggregate.spmm_launch(plan.twin, Sd, lut.to(DEV), False, True, s_total=s_total, reduce_cr=1, self_sum=self_sum)
    aggregate.spmm_launch(plan.twin, Sd, lut.to(DEV), False, True, s_total=s_total, reduce_cr=1, describe=d2)
    torch.cuda.synchronize()
    info = d1[0]
    assert info == d2[0]                                             # the partition does not depend on self_sum
    assert info["n_tiles"] > 0 and info["n_slice_blocks"] > 0 and info["row_q0"] < N and info["classed"] == int(classed)
    assert info["short_tile"][1] > 0                                 # a run of EMPTY rows (L = 0) ahead of the others
    assert torch.equal(y0.cpu(), want) and torch.equal(y1.cpu(), want) and torch.equal(y1, y2)
    # refused off its route, before a launch: all W columns stored, no sorted copy
    out = torch.full((N, W), float("nan"), device=DEV)
    a = aggregate._spmm_args(plan.twin, Sd, lut.to(DEV), False, s_total, out, None, False)
    a.self_sum, a.self_parts = _lib.ptr(self_sum), parts
    assert _lib.lib().gnan_spmm_fwd(a, _lib.stream_of(Sd)) == _lib.ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


@pytest.mark.parametrize("family", ["unit", "range", "outlier"])
@pytest.mark.parametrize("W,parts,use_cnt", [(48, 3, True), (64, 2, True), (64, 4, False), (128, 4, True)])
def test_per_row_bound_against_the_original_graph(family, W, parts, use_cnt, monkeypatch):
    from gnan_amd import aggregate
    from gnan_amd import functional as Fn
    _lower(monkeypatch, classed=W == 128)
    D = 3
    rowptr, col, code = _csr()
    g = _graph(rowptr, col, code, N, D)
    plan = _plan(g)
    rng = np.random.default_rng(W + parts + len(family))
    S = torch.from_numpy(rowwise.narrow_operand(rng, family, N, W))           # 'outlier': 2^60 in the last row, which no other row lists
    lut = torch.from_numpy(rng.standard_normal((D, 1)).astype(np.float32))
    Sd = S.to(DEV)
    s_total = Fn.column_sums(Sd)
    fg = W // parts
    self_sum = _host_parts(S, parts).to(DEV)
    d = []
    y = aggregate.spmm_launch(plan.twin, Sd, lut.to(DEV), use_cnt, True, s_total=s_total, reduce_cr=1, describe=d, self_sum=self_sum)
    again = aggregate.spmm_launch(plan.twin, Sd, lut.to(DEV), use_cnt, True, s_total=s_total, reduce_cr=1, self_sum=self_sum)
    torch.cuda.synchronize()
    assert d[0]["n_tiles"] > 0 and d[0]["n_slice_blocks"] > 0 and d[0]["row_q0"] < N
    truth, bound = self_row_bound(rowptr, col, code, S, lut, g.cnt.cpu() if use_cnt else None, s_total.cpu(), parts, fg // 4)
    ratio = rowwise.assert_within(y.cpu(), truth, bound, f"{family} W={W} parts={parts}")
    print(f"ROW-BOUND worst |err|/bound {ratio:.3f} :: self term {family} W={W} parts={parts} cnt={use_cnt}")
    assert torch.equal(y, again)


# ---- the route ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [48, 64])
def test_route_never_gathers_an_unlisted_row(F, monkeypatch):
    """The operand buffer NaN-filled before the look-up: every output finite, within the per-row bound of the complete operand, and
    the same bits with the stores of unlisted rows switched back on."""
    from gnan_amd import aggregate
    from gnan_amd import functional as Fn
    _lower(monkeypatch)
    D = 3
    rowptr, col, code = _csr()
    g = _graph(rowptr, col, code, N, D)
    plan = _plan(g)
    st = _stack(_mlp_state(F, 3, 16, 1, True, seed=F + 1), F, 3, 16, 1, True)
    x = torch.randn(N, F, generator=torch.Generator().manual_seed(F + 1)).to(DEV)
    lut = torch.tensor([[0.9], [-0.6], [0.45]], device=DEV)
    assert aggregate.reference_order_inference_applies(x, st, lut, g)
    with torch.no_grad():
        fx, _, tot = Fn._fmlp_forward(x, st, False, True)
        buf = torch.full((N, F), float("nan"), device=DEV)             # the route's operand buffer: NaN where nothing is stored
        marks = []
        y = aggregate.reference_order_inference(g, x, st, lut, True, mark=lambda: marks.append(1), operand=buf)
        monkeypatch.setattr(aggregate, "SELF_FROM_LOOKUP_SKIP_STORES", False)
        full = aggregate.reference_order_inference(g, x, st, lut, True)
    torch.cuda.synchronize()
    assert marks == [1] and tuple(y.shape) == (N, 1)
    assert bool(torch.isnan(buf.cpu()[~_listed(plan)]).all()) and bool(torch.isnan(buf).any())
    assert bool(torch.isfinite(y).all())
    assert torch.equal(y, full)
    parts = 2 if F == 64 else 3
    truth, bound = self_row_bound(rowptr, col, code, fx.cpu(), lut.cpu(), g.cnt.cpu(), tot.cpu(), parts, (F // parts) // 4)
    ratio = rowwise.assert_within(y.cpu(), truth, bound, f"route F={F}")
    print(f"ROW-BOUND worst |err|/bound {ratio:.3f} :: route F={F}")


# ---- the module -----------------------------------------------------------------------------------------------------------------------
class Bag:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def test_module_takes_the_route_above_the_default_gate(monkeypatch):
    """TensorGNAN, reference order, no_grad, 70 000 nodes of a preferential-attachment graph, F = 64: above the route's row gate,
    no gate lowered.  The shape functions are pinned to the table path (``FMLP_ALGO``, as the kernel tests pin it): left to itself
    the strategy choice tabulates from 2^24 look-ups on, which F = 64 reaches at 262 144 nodes, and the route exists only where
    the look-up runs."""
    import gnan_amd  # noqa: F401
    from gnan_amd import _lib, aggregate, models, replay
    from gnan_amd import functional as Fn
    from gnan_amd import synthetic as syn
    from helpers import assert_rule
    monkeypatch.setattr(Fn, "FMLP_ALGO", _lib.FMLP_PWL)
    n, E, F = 70_000, 400_000, 64
    src, dst = syn.preferential_attachment_edges(n, E, seed=0, device=DEV)
    loops = int((src == dst).sum())
    g = syn.hop1_csr(src, dst, n)
    assert g.self_free_plan(strict=False) is not None and (g.self_free_plan() is None) == (loops > 0)
    x = syn.block_features(n, F, 0, n, seed=1, device=DEV)
    torch.manual_seed(0)
    mod = models.TensorGNAN(F, 1, 3, hidden_channels=16, device=DEV)
    gen = torch.Generator().manual_seed(7)
    with torch.no_grad():
        for _, p in mod.named_parameters():
            p.copy_(torch.randn(p.shape, generator=gen) * (0.5 if p.dim() == 1 else (2.0 / sum(p.shape)) ** 0.5))
    mod = mod.to(DEV).eval()
    mod.aggregation_order = "reference"
    data = Bag(x=x, edge_index=None, gnan_graph=g)
    took = []
    real = aggregate.reference_order_inference
    monkeypatch.setattr(aggregate, "reference_order_inference", lambda *a, **k: took.append(1) or real(*a, **k))

    def forward(d=data, grad=False):
        replay.release(mod)
        with torch.enable_grad() if grad else torch.no_grad():
            return mod.forward(d).detach()

    monkeypatch.setattr(aggregate, "SELF_FROM_LOOKUP", False)
    off = forward()
    assert not took
    monkeypatch.setattr(aggregate, "SELF_FROM_LOOKUP", True)
    marks = []
    mod.stage_hook = marks.append
    y = forward()
    mod.stage_hook = None
    assert took == [1] and marks == ["start", "lut", "fmlp", "spmm"]
    # per-row bound and the project's rule, from the operand the module itself aggregates
    with torch.no_grad():
        fx, total = mod._operand(x, "fs", mod.fs, False, True, pad_ok=True)
        lut = mod._lut_global(g)
    rowptr, col, code = g.rowptr.cpu(), g.col.cpu(), g.code.cpu()
    truth, bound = self_row_bound(rowptr, col, code, fx.cpu(), lut.cpu(), g.cnt.cpu(), total.cpu(), 2, 8)
    ratio = rowwise.assert_within(y.cpu(), truth, bound, "module")
    print(f"ROW-BOUND worst |err|/bound {ratio:.3f} :: module, 70 000 nodes ({loops} self-loop edges)")
    assert_rule(y.cpu(), truth, off.cpu(), what="module: new route against the switched-off one")
    # declined: grad mode with parameters that require grad, a graph with one self pair missing, a bf16 operand
    took.clear()
    g_on = forward(grad=True)
    monkeypatch.setattr(aggregate, "SELF_FROM_LOOKUP", False)
    assert torch.equal(forward(grad=True), g_on) and not took
    monkeypatch.setattr(aggregate, "SELF_FROM_LOOKUP", True)
    first = int(g.rowptr[5])
    at = first + int(torch.nonzero(g.col[first:int(g.rowptr[6])] == 5)[0])
    col2 = g.col.clone()
    col2[at] = 6
    g2 = type(g).from_csr(g.rowptr, col2, g.code, n_cols=n, n_codes=3)
    d2 = Bag(x=x, edge_index=None, gnan_graph=g2)
    y2 = forward(d2)
    monkeypatch.setattr(aggregate, "SELF_FROM_LOOKUP", False)
    assert torch.equal(forward(d2), y2) and not took
    mod.operand_dtype = torch.bfloat16
    b_off = forward()
    monkeypatch.setattr(aggregate, "SELF_FROM_LOOKUP", True)
    assert torch.equal(forward(), b_off) and not took
    mod.operand_dtype = torch.float32
    # three forwards on the same inputs: two eager ones, then the replayed capture — the same bits
    replay.release(mod)
    with torch.no_grad():
        outs = [mod.forward(data).clone() for _ in range(3)]
    assert len(took) >= 3 and mod.__dict__["_replays"].get(*replay._key(mod, data, False))["plan"] is not None
    assert torch.equal(outs[0], y) and torch.equal(outs[1], y) and torch.equal(outs[2], y)
    replay.release(mod)
