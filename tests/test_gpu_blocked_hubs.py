"""The blocked hub segments of the reference-order inference route (``gnan_spmm_args.hub_*``, ``HopGraph.blocked_hub_plan``, seg_body<.., HUB> in
csrc/spmm_fwd_body.hpp, spmm_hub_combine_kernel in csrc/spmm.hip): the twin's rows of more than 512 pairs are taken a lane group per (row,
column class, popularity block) piece and combined in a second pass, with no slice blocks and no fix-up launch.  About 2 500 rows; the
gates that keep small graphs off the route are lowered as tests/test_gpu_classed_rows.py lowers them, plus ``BLOCKED_HUBS_MIN_NNZ``, and
the blocks are 4 operand rows (2 or 3 ranked blocks and the cold one) so that a graph of this size has them all.  Hub rows: 513 and 514
pairs in the twin, one whose pairs all fall in class 5, one with a pair in every (class, block), one listing only cold columns, one of
1 500 pairs; beside them rows of 511 and 512 pairs and the shorter ones, so that the r11 segments, the tiles and the row walk are in the
same launch.

Per-row bound, truth and magnitude ``rowwise._truth_mag``'s for the ORIGINAL graph (L_i its pairs, the self pair included):

    hub rows          k = min(cap, L_i - 1) + ceil((L_i - 1) / 64) + 24     counted from the kernels as built: a gathered term meets 2
                      divisions and the fold (3), the fmaf chain over the segment's pairs — at most the cap (BLOCKED_HUB_SEG_PAIRS), at
                      most the twin's L_i - 1 pairs —, at most 4 adds within the lane, log2(LPR) <= 6 butterfly steps, the combine's chain
                      of a lane over the row's slots l, l + 64, ... (a row has no more slots than pairs: ceil((L_i - 1) / 64) adds), its 6
                      butterfly steps, the fmaf of the rest term, the self fmaf: chain + slots + 21.  The rest term (one division, the
                      float64 total's cast, two fmaf) and the self term (as tests/test_gpu_self_from_lookup.py counts it) stay below that.
                      It never exceeds the 2 (L_i - 1) + 11 the full-size tests grant hub rows (asserted below for every hub row).
    classed rows      k = L_i + 24     (tests/test_gpu_classed_rows.py: unchanged code, unchanged bits)
    every other row   ``rowwise.reference``'s k: unchanged code, unchanged bits.

A zero bound demands an exact zero; no element is left out.  Worst |err| / bound over the hub rows as measured on an MI355X: 0.026 in
the kernel cases ('outlier', W = 48, cap 8), 0.042 in the module case (profiles/r12_blocked_hubs_ab.txt)."""
import numpy as np
import pytest
import torch

import rowwise
from test_blocked_hub_plan import _blocks
from test_gpu_kernels import _graph
from test_self_free_plan import self_graph

pytestmark = pytest.mark.gpu
DEV = "cuda"
N = 2504                                     # (N - 1) & 7 == 7; node N - 1 is listed by no other row (the 'outlier' operand's large row)
MIX = ([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 30], [.05, .35, .12, .1, .08, .06, .05, .05, .05, .05, .04])      # rowwise.short_csr's degree mix
ONE_CLASS, EACH, COLD = 49, 50, 51           # hub rows: all pairs in class 5 / a pair in every (class, block) / cold columns only
LENGTHS = {40: 5, 41: 32, 42: 33, 43: 100, 44: 257, 45: 511, 46: 512, 47: 513, 48: 514, ONE_CLASS: 600, EACH: 700, COLD: 600, 52: 1500}
HUBS = [r for r, d in LENGTHS.items() if d > 512]
BLOCK_ROWS = 4


def _lower(monkeypatch, n_blocks, cap):
    from gnan_amd import _lib, aggregate
    from gnan_amd import functional as Fn
    monkeypatch.setattr(aggregate, "DEGREE_SORTED_COPY_MIN_ROWS", 1)
    monkeypatch.setattr(aggregate, "SELF_FROM_LOOKUP_MIN_ROWS", 0)
    monkeypatch.setattr(aggregate, "CLASSED_MIN_NNZ", 1)
    monkeypatch.setattr(aggregate, "CLASSED_ROWS_MIN_NNZ", 1)
    monkeypatch.setattr(aggregate, "BLOCKED_HUBS_MIN_NNZ", 1)
    monkeypatch.setattr(aggregate, "BLOCKED_HUB_BLOCKS", n_blocks)
    monkeypatch.setattr(aggregate, "BLOCKED_HUB_SEG_PAIRS", cap)
    monkeypatch.setattr(Fn, "FMLP_ALGO", _lib.FMLP_PWL)
    monkeypatch.setattr(Fn, "INDEX_MIN_NODES", 0)
    Fn._RANGE_CHURN.clear()


def _block_bytes(monkeypatch, W):
    from gnan_amd import aggregate
    monkeypatch.setattr(aggregate, "BLOCKED_HUB_BLOCK_BYTES", BLOCK_ROWS * W * 4)


_CSR = {}


def _twin_blocks(rowptr, col, n_blocks):
    """Popularity block of every column, from the pairs the twin keeps (every pair but a row's own)."""
    row = np.repeat(np.arange(N), np.diff(rowptr))
    return _blocks(col[col != row], N, BLOCK_ROWS, n_blocks)


def _csr(D):
    """Every row: its self pair (code 0, in the middle) and the twin's pairs, drawn from a pool that holds 128 columns twenty times (the
    often listed ones) and every column but the last once."""
    if D not in _CSR:
        rng = np.random.default_rng(D)
        lengths = rng.choice(MIX[0], N, p=MIX[1])
        for r, d in LENGTHS.items():
            lengths[r] = d
        pool = np.concatenate([np.tile(np.arange(8, 136), 20), np.arange(N - 1)])
        rowptr, col, code = self_graph(rng, N, N, "middle", lengths, D, listed_cols=pool)

        def twin(r):
            e = np.arange(rowptr[r], rowptr[r + 1])
            return e[col[e] != r]

        col[twin(ONE_CLASS)] = (col[twin(ONE_CLASS)] & ~7) | 5                              # (never the row itself, never node N - 1)
        col[twin(COLD)] = rng.integers(1000, 2400, len(twin(COLD))).astype(np.int32)
        block = _twin_blocks(rowptr, col, 3)
        e, k = twin(EACH), 0
        for c in range(8):
            for b in range(4):
                col[e[k]] = np.nonzero((np.arange(N) & 7 == c) & (block == b) & (np.arange(N) > 7) & (np.arange(N) < N - 8))[0][0]
                k += 1
        for n_blocks in (2, 3):                                                             # the rows are what their names say
            block = _twin_blocks(rowptr, col, n_blocks)
            assert len({(int(c) & 7, int(block[c])) for c in col[twin(EACH)]}) == 8 * (n_blocks + 1)
            assert (block[col[twin(COLD)]] == n_blocks).all() and ((col[twin(ONE_CLASS)] & 7) == 5).all()
            assert len(set(block[col[twin(ONE_CLASS)]].tolist())) == n_blocks + 1
        _CSR[D] = (rowptr, col, code)
    return _CSR[D]


def _kinds(rowptr):
    from gnan_amd import aggregate
    twin = np.diff(rowptr) - 1
    return twin > 512, (twin >= aggregate.CLASSED_ROWS_MIN_PAIRS) & (twin <= 512)


def _parts(S, parts):
    """``self_sum [parts, N]``: the rows' sums over blocks of W / parts columns, float64 rounded once."""
    n, W = S.shape
    return torch.from_numpy(np.ascontiguousarray(S.numpy().astype(np.float64).reshape(n, parts, W // parts).sum(2).T.astype(np.float32)))


def _bound(rowptr, col, code, S, lut, cnt, tot, cap):
    truth, mag, deg = rowwise._truth_mag(rowptr, col, code, S, lut, cnt, tot)
    hub, classed = _kinds(rowptr)
    k = deg + 15.0                                                                        # rowwise.reference, fused read-out
    k = np.where(classed, deg + 24.0, k)
    k_hub = np.minimum(cap, deg - 1) + np.ceil((deg - 1) / 64.0) + 24.0
    assert (k_hub[hub] <= 2.0 * (deg[hub] - 1) + 11).all()                                 # what the full-size tests grant hub rows
    k = np.where(hub, k_hub, k)
    return truth.sum(1, keepdims=True), rowwise.gamma(k)[:, None] * mag.sum(1, keepdims=True)


def _launch(monkeypatch, g, Sd, lut, use_cnt, s_total, self_sum, on, describe=None):
    from gnan_amd import aggregate
    monkeypatch.setattr(aggregate, "BLOCKED_HUBS", on)
    plan = g.self_free_plan(strict=False)
    assert plan is not None
    return aggregate.spmm_launch(plan.twin, Sd, lut, use_cnt, True, s_total=s_total, reduce_cr=1, self_sum=self_sum, describe=describe)


def _check_describe(on, off, g, W, n_blocks, cap):
    from gnan_amd import aggregate
    plan = g.self_free_plan(strict=False).twin.degree_sorted_copy()[0].blocked_hub_plan(BLOCK_ROWS, n_blocks, cap)
    assert plan is not None and plan.n_hub == len(HUBS) and min(plan.block_pairs) > 0
    assert on["n_hub_seg_blocks"] > 0 and on["n_hub_seg_blocks"] % 8 == 0 and on["n_hub_segs"] == plan.n_seg
    assert on["n_slice_blocks"] == 0 and on["classed"] == 0
    assert off["n_hub_seg_blocks"] == 0 and off["n_hub_segs"] == 0 and off["n_slice_blocks"] > 0 and off["classed"] == 1
    for k in ("n_seg_blocks", "n_segs", "n_tiles", "n_tile_blocks", "row_q0", "lpr", "vec"):
        assert on[k] == off[k]
    assert on["n_seg_blocks"] > 0 and on["n_tiles"] > 0 and on["lpr"] == rowwise.lanes_per_row(W)
    assert aggregate.CLASSED_ROWS_MIN_PAIRS == 33


# (W, D, parts, ranked blocks, cap)
EXACT = [(48, 3, 1, 2, 8), (64, 4, 2, 3, 16), (64, 2, 1, 2, 256), (128, 4, 1, 3, 64), (128, 3, 2, 2, 256)]


@pytest.mark.parametrize("W,D,parts,n_blocks,cap", EXACT)
def test_integer_operands_are_exact_with_the_route_on_and_off(W, D, parts, n_blocks, cap, monkeypatch):
    from gnan_amd import functional as Fn
    _lower(monkeypatch, n_blocks, cap)
    _block_bytes(monkeypatch, W)
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
    _check_describe(d_on[0], d_off[0], g, W, n_blocks, cap)
    assert torch.equal(y_on.cpu(), want) and torch.equal(y_off.cpu(), want)


# (W, D, parts, counts, ranked blocks, cap)
CASES = [(48, 3, 1, True, 2, 8), (48, 4, 2, False, 3, 256), (64, 2, 1, True, 3, 16), (64, 3, 2, True, 2, 256), (64, 4, 1, False, 3, 64),
         (128, 3, 1, False, 2, 256), (128, 4, 2, True, 3, 8)]


@pytest.mark.parametrize("family", ["unit", "range", "outlier"])
@pytest.mark.parametrize("W,D,parts,use_cnt,n_blocks,cap", CASES)
def test_per_row_bound_reproducible_unlisted_rows_and_other_rows_keep_their_bits(family, W, D, parts, use_cnt, n_blocks, cap, monkeypatch):
    from gnan_amd import functional as Fn
    _lower(monkeypatch, n_blocks, cap)
    _block_bytes(monkeypatch, W)
    rowptr, col, code = _csr(D)
    g = _graph(rowptr, col, code, N, D)
    rng = np.random.default_rng(W + D + parts + len(family))
    S = torch.from_numpy(rowwise.narrow_operand(rng, family, N, W))           # 'outlier': 2^60 in the last row, which no other row lists
    lut = torch.from_numpy(rng.standard_normal((D, 1)).astype(np.float32))
    Sd = S.to(DEV)
    s_total = Fn.column_sums(Sd)
    self_sum = _parts(S, parts).to(DEV)
    # the operand as the look-up leaves it: NaN behind every row no pair of the twin lists
    row = np.repeat(np.arange(N), np.diff(rowptr))
    unlisted = torch.from_numpy(np.bincount(col[col != row], minlength=N) == 0)
    assert 50 < int(unlisted.sum()) < N // 2
    Sn = Sd.clone()
    Sn[unlisted.to(DEV)] = float("nan")
    d, d_off = [], []
    y = _launch(monkeypatch, g, Sn, lut.to(DEV), use_cnt, s_total, self_sum, True, d)
    again = _launch(monkeypatch, g, Sn, lut.to(DEV), use_cnt, s_total, self_sum, True)
    off = _launch(monkeypatch, g, Sn, lut.to(DEV), use_cnt, s_total, self_sum, False, d_off)
    torch.cuda.synchronize()
    _check_describe(d[0], d_off[0], g, W, n_blocks, cap)
    assert bool(torch.isfinite(y).all())
    truth, bound = _bound(rowptr, col, code, S, lut, g.cnt.cpu() if use_cnt else None, s_total.cpu(), cap)
    rowwise.assert_within(y.cpu(), truth, bound, f"{family} W={W} D={D} parts={parts}")
    hub, _ = _kinds(rowptr)
    assert sorted(np.nonzero(hub)[0].tolist()) == sorted(HUBS)
    ratio = rowwise.worst_ratio(y.cpu()[torch.from_numpy(hub)], truth[hub], bound[hub])
    print(f"ROW-BOUND worst |err|/bound {ratio:.3f} :: blocked hub rows {family} W={W} D={D} parts={parts} cnt={use_cnt} "
          f"blocks={n_blocks} cap={cap}")
    assert torch.equal(y, again)
    other = torch.from_numpy(~hub)
    assert torch.equal(y.cpu()[other].view(torch.int32), off.cpu()[other].view(torch.int32))       # BLOCKED_HUBS = False: the parent's route


class Bag:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def test_module_takes_the_hub_segments_on_the_inference_route(monkeypatch):
    """TensorGNAN, reference order, no_grad, F = 64: ``reference_order_inference`` hands the twin's launch the plan."""
    import gnan_amd  # noqa: F401
    from gnan_amd import aggregate, models, replay
    from gnan_amd import synthetic as syn
    _lower(monkeypatch, 3, 64)
    D, F = 3, 64
    _block_bytes(monkeypatch, F)
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
        monkeypatch.setattr(aggregate, "BLOCKED_HUBS", on)
        replay.release(mod)
        with torch.no_grad():
            return mod.forward(data).detach().clone()

    y, again, off = forward(True), forward(True), forward(False)
    torch.cuda.synchronize()
    assert len(took) == 3 and len(infos) == 3
    _check_describe(infos[0], infos[2], g, F, 3, 64)
    assert infos[0] == infos[1]
    with torch.no_grad():
        fx, total = mod._operand(x, "fs", mod.fs, False, True, pad_ok=True)
        lut = mod._lut_global(g)
    truth, bound = _bound(rowptr, col, code, fx.cpu(), lut.cpu(), g.cnt.cpu(), total.cpu(), 64)
    ratio = rowwise.assert_within(y.cpu(), truth, bound, "module")
    print(f"ROW-BOUND worst |err|/bound {ratio:.3f} :: module, blocked hub rows")
    assert torch.equal(y, again)
    other = torch.from_numpy(~_kinds(rowptr)[0])
    assert torch.equal(y.cpu()[other].view(torch.int32), off.cpu()[other].view(torch.int32))
    replay.release(mod)
