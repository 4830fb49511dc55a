"""The classed row segments of the reference-order inference route (``gnan_spmm_args.seg_*``, ``HopGraph.classed_row_plan``, seg_body in
csrc/spmm_fwd_body.hpp, spmm_seg_combine_kernel in csrc/spmm.hip): rows of the twin's degree-sorted copy with ``CLASSED_ROWS_MIN_PAIRS``
.. 512 pairs are taken a lane group per (row, column class) and combined in a second pass.  About 2 500 rows; the gates that keep small
graphs off the route are lowered as tests/test_gpu_self_from_lookup.py lowers them, plus ``CLASSED_ROWS_MIN_NNZ``; the kernel tests set
``CLASSED_ROWS_MIN_PAIRS`` to 5 (every row the tiles leave: segments of one or two pairs, the one-class row, the row with a pair per
class) or leave the shipped value (33: rows of 32 pairs stay with the row walk), the module test leaves it.

Per-row bound, truth and magnitude ``rowwise._truth_mag``'s for the ORIGINAL graph (L_i its pairs, the self pair included):

    classed rows      k = L_i + 24      counted from the kernels as built: a gathered term meets 2 divisions and the fold (3: it inherits
                      two roundings and adds one), the fmaf chain over the twin's L_i - 1 pairs, at most 4 adds within the lane, log2(LPR)
                      <= 6 butterfly steps (4 at W = 64, 5 at W = 128), 3 adds of the class tree (it has depth 3: <= 7), the fmaf of the
                      rest term, the self fmaf: L_i + 17 at most.  The rest term: one division, the float64 total's cast, two fmaf.  The
                      self term: as tests/test_gpu_self_from_lookup.py counts it (below L_i + 15).  All of them stay below L_i + 24.
    every other row   ``rowwise.reference``'s k (tiles, rows below the plan's minimum, hub rows): unchanged code, unchanged bits.

A zero bound demands an exact zero; no element is left out."""
import numpy as np
import pytest
import torch

import rowwise
from test_gpu_kernels import _graph
from test_self_free_plan import self_graph

pytestmark = pytest.mark.gpu
DEV = "cuda"
N = 2504                                     # (N - 1) & 7 == 7; node N - 1 is listed by no other row (the 'outlier' operand's large row)
MIX = ([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 30], [.05, .35, .12, .1, .08, .06, .05, .05, .05, .05, .04])      # rowwise.short_csr's degree mix
LENGTHS = {40: 5, 41: 8, 42: 9, 43: 16, 44: 17, 45: 64, 46: 511, 47: 512, 48: 513, 49: 600, 50: 4, 51: 5, 52: 32, 53: 33, 54: 33,
           55: 100, 56: 257}                 # (row, pairs in the twin)
ONE_CLASS, EACH_CLASS = 60, 61               # rows of 8 pairs in the twin: all in class 5 / one in every class


def _lower(monkeypatch, min_pairs=None):
    from gnan_amd import _lib, aggregate
    from gnan_amd import functional as Fn
    monkeypatch.setattr(aggregate, "DEGREE_SORTED_COPY_MIN_ROWS", 1)
    monkeypatch.setattr(aggregate, "SELF_FROM_LOOKUP_MIN_ROWS", 0)
    monkeypatch.setattr(aggregate, "CLASSED_MIN_NNZ", 1)
    monkeypatch.setattr(aggregate, "CLASSED_ROWS_MIN_NNZ", 1)
    if min_pairs is not None:
        monkeypatch.setattr(aggregate, "CLASSED_ROWS_MIN_PAIRS", min_pairs)
    monkeypatch.setattr(Fn, "FMLP_ALGO", _lib.FMLP_PWL)
    monkeypatch.setattr(Fn, "INDEX_MIN_NODES", 0)
    Fn._RANGE_CHURN.clear()


_CSR = {}


def _csr(D):
    """Every row: its self pair (code 0, in the middle) and the twin's pairs: the short rows' mix, the lengths around every threshold,
    a one-class row and a row with one pair per class."""
    if D not in _CSR:
        rng = np.random.default_rng(D)
        lengths = rng.choice(MIX[0], N, p=MIX[1])
        for r, d in LENGTHS.items():
            lengths[r] = d
        lengths[ONE_CLASS] = lengths[EACH_CLASS] = 8
        rowptr, col, code = self_graph(rng, N, N, "middle", lengths, D, listed_cols=np.arange(N - 1))
        for r, classes in ((ONE_CLASS, np.full(8, 5)), (EACH_CLASS, rng.permutation(8))):
            e = np.arange(rowptr[r], rowptr[r + 1])
            e = e[col[e] != r]
            col[e] = rng.integers(16, 300, 8).astype(np.int32) * 8 + classes          # (never the row itself, never node N - 1)
        _CSR[D] = (rowptr, col, code)
    return _CSR[D]


def _classed(rowptr):
    from gnan_amd import aggregate
    twin = np.diff(rowptr) - 1
    return (twin >= aggregate.CLASSED_ROWS_MIN_PAIRS) & (twin <= 512)


def _parts(S, parts):
    """``self_sum [parts, N]``: the rows' sums over blocks of W / parts columns, float64 rounded once."""
    n, W = S.shape
    return torch.from_numpy(np.ascontiguousarray(S.numpy().astype(np.float64).reshape(n, parts, W // parts).sum(2).T.astype(np.float32)))


def _bound(rowptr, col, code, S, lut, cnt, tot):
    truth, mag, deg = rowwise._truth_mag(rowptr, col, code, S, lut, cnt, tot)
    k = np.where(deg > rowwise.HUB_THRESHOLD, 2 * deg, deg + 5).astype(np.float64) + 10          # rowwise.reference, fused read-out
    k = np.where(_classed(rowptr), deg + 24.0, k)
    return truth.sum(1, keepdims=True), rowwise.gamma(k)[:, None] * mag.sum(1, keepdims=True)


def _launch(monkeypatch, g, Sd, lut, use_cnt, s_total, self_sum, on, describe=None):
    from gnan_amd import aggregate
    monkeypatch.setattr(aggregate, "CLASSED_ROWS", on)
    plan = g.self_free_plan(strict=False)
    assert plan is not None
    return aggregate.spmm_launch(plan.twin, Sd, lut, use_cnt, True, s_total=s_total, reduce_cr=1, self_sum=self_sum, describe=describe)


def _check_describe(info, rowptr, W):
    from gnan_amd import aggregate
    twin = np.sort(np.diff(rowptr) - 1)
    assert info["n_seg_blocks"] > 0 and info["n_seg_blocks"] % 8 == 0 and info["n_segs"] > 0
    assert info["n_tiles"] > 0 and info["n_slice_blocks"] > 0 and info["classed"] == 1
    assert info["row_q0"] == int((twin <= aggregate.SHORT_ROW_LMAX).sum()) and info["lpr"] == rowwise.lanes_per_row(W)


@pytest.mark.parametrize("W", [48, 64, 128])
@pytest.mark.parametrize("D", [3, 4])
@pytest.mark.parametrize("parts,min_pairs", [(1, 5), (2, 5), (2, None)])
def test_integer_operands_are_exact_with_the_route_on_and_off(W, D, parts, min_pairs, monkeypatch):
    from gnan_amd import functional as Fn
    _lower(monkeypatch, min_pairs)
    rowptr, col, code = _csr(D)
    g = _graph(rowptr, col, code, N, D)
    rng = np.random.default_rng(W + D + parts)
    S = torch.from_numpy(rng.integers(-4, 5, (N, W)).astype(np.float32))
    lut = torch.tensor([2.0, -1.0, 0.5, 0.25][:D]).view(D, 1)
    Sd = S.to(DEV)
    s_total = Fn.column_sums(Sd)
    t4, a4 = rowwise.exact_quarters(rowptr, col, code, S, lut, s_total.cpu(), 1)
    assert int(a4.max()) < 2 ** 24
    want = (t4.double() / 4).float()
    self_sum = _parts(S, parts).to(DEV)
    d_on, d_off = [], []
    y_on = _launch(monkeypatch, g, Sd, lut.to(DEV), False, s_total, self_sum, True, d_on)
    y_off = _launch(monkeypatch, g, Sd, lut.to(DEV), False, s_total, self_sum, False, d_off)
    torch.cuda.synchronize()
    _check_describe(d_on[0], rowptr, W)
    assert d_off[0]["n_seg_blocks"] == 0 and d_off[0]["n_segs"] == 0 and d_off[0]["n_tiles"] == d_on[0]["n_tiles"]
    assert torch.equal(y_on.cpu(), want) and torch.equal(y_off.cpu(), want)


# (W, D, parts, counts, CLASSED_ROWS_MIN_PAIRS or None for the shipped value)
CASES = [(48, 3, 1, True, 5), (48, 4, 2, False, 5), (64, 3, 2, True, 5), (64, 4, 1, False, 5), (128, 3, 1, False, 5), (128, 4, 2, True, 5),
         (64, 3, 2, True, None), (128, 4, 1, True, 17)]


@pytest.mark.parametrize("family", ["unit", "range", "outlier"])
@pytest.mark.parametrize("W,D,parts,use_cnt,min_pairs", CASES)
def test_per_row_bound_reproducible_and_other_rows_keep_their_bits(family, W, D, parts, use_cnt, min_pairs, monkeypatch):
    from gnan_amd import functional as Fn
    _lower(monkeypatch, min_pairs)
    rowptr, col, code = _csr(D)
    g = _graph(rowptr, col, code, N, D)
    rng = np.random.default_rng(W + D + parts + len(family))
    S = torch.from_numpy(rowwise.narrow_operand(rng, family, N, W))           # 'outlier': 2^60 in the last row, which no other row lists
    lut = torch.from_numpy(rng.standard_normal((D, 1)).astype(np.float32))
    Sd = S.to(DEV)
    s_total = Fn.column_sums(Sd)
    self_sum = _parts(S, parts).to(DEV)
    d = []
    y = _launch(monkeypatch, g, Sd, lut.to(DEV), use_cnt, s_total, self_sum, True, d)
    again = _launch(monkeypatch, g, Sd, lut.to(DEV), use_cnt, s_total, self_sum, True)
    off = _launch(monkeypatch, g, Sd, lut.to(DEV), use_cnt, s_total, self_sum, False)
    torch.cuda.synchronize()
    _check_describe(d[0], rowptr, W)
    truth, bound = _bound(rowptr, col, code, S, lut, g.cnt.cpu() if use_cnt else None, s_total.cpu())
    ratio = rowwise.assert_within(y.cpu(), truth, bound, f"{family} W={W} D={D} parts={parts}")
    print(f"ROW-BOUND worst |err|/bound {ratio:.3f} :: classed rows {family} W={W} D={D} parts={parts} cnt={use_cnt}")
    assert torch.equal(y, again)
    other = torch.from_numpy(~_classed(rowptr))
    assert 0 < int(other.sum()) < N and not bool(other[45]) and bool(other[50]) and bool(other[48])    # 64 pairs: classed; 4, 513: not
    assert torch.equal(y.cpu()[other].view(torch.int32), off.cpu()[other].view(torch.int32))


class Bag:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def test_module_takes_the_segments_on_the_inference_route(monkeypatch):
    """TensorGNAN, reference order, no_grad, F = 64: ``reference_order_inference`` hands the twin's launch the plan."""
    import gnan_amd  # noqa: F401
    from gnan_amd import aggregate, models, replay
    from gnan_amd import synthetic as syn
    _lower(monkeypatch)
    D, F = 3, 64
    rowptr, col, code = _csr(D)
    g = _graph(rowptr, col, code, N, D)
    x = syn.block_features(N, F, 0, N, seed=1, device=DEV)
    torch.manual_seed(0)
    mod = models.TensorGNAN(F, 1, 3, hidden_channels=16, device=DEV)
    gen = torch.Generator().manual_seed(7)
    with torch.no_grad():
        for _, p in mod.named_parameters():
            p.copy_(torch.randn(p.shape, generator=gen) * (0.5 if p.dim() == 1 else (2.0 / sum(p.shape)) ** 0.5))
    mod = mod.to(DEV).eval()
    mod.aggregation_order = "reference"
    data = Bag(x=x, edge_index=None, gnan_graph=g)
    took, infos = [], []
    route, launch = aggregate.reference_order_inference, aggregate.spmm_launch
    monkeypatch.setattr(aggregate, "reference_order_inference", lambda *a, **k: took.append(1) or route(*a, **k))
    monkeypatch.setattr(aggregate, "spmm_launch", lambda *a, **k: launch(*a, **{**k, "describe": infos}))

    def forward(on):
        monkeypatch.setattr(aggregate, "CLASSED_ROWS", on)
        replay.release(mod)
        with torch.no_grad():
            return mod.forward(data).detach().clone()

    y, again, off = forward(True), forward(True), forward(False)
    torch.cuda.synchronize()
    assert len(took) == 3 and len(infos) == 3
    assert infos[0]["n_seg_blocks"] > 0 and infos[0] == infos[1] and infos[2]["n_seg_blocks"] == 0
    assert aggregate.CLASSED_ROWS_MIN_PAIRS > 30 and int(_classed(rowptr).sum()) >= 7      # the shipped minimum: rows of 33 .. 512 pairs
    with torch.no_grad():
        fx, total = mod._operand(x, "fs", mod.fs, False, True, pad_ok=True)
        lut = mod._lut_global(g)
    truth, bound = _bound(rowptr, col, code, fx.cpu(), lut.cpu(), g.cnt.cpu(), total.cpu())
    ratio = rowwise.assert_within(y.cpu(), truth, bound, "module")
    print(f"ROW-BOUND worst |err|/bound {ratio:.3f} :: module, classed rows")
    assert torch.equal(y, again)
    other = torch.from_numpy(~_classed(rowptr))
    assert torch.equal(y.cpu()[other].view(torch.int32), off.cpu()[other].view(torch.int32))
    replay.release(mod)
