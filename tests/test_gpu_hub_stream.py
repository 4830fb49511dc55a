"""The hub rows through the pair stream (``aggregate.HUB_STREAM``, ``gnan_spmm_args.q_hub``, ``HopGraph.pair_stream_plan(..., None, hub_blocks)``;
spmm_stream_kernel, spmm_stream_combine_kernel and spmm_stream_hub_combine_kernel in csrc/spmm_stream.hip): on the reference-order inference
route the twin's rows of more than 512 pairs leave the blocked hub segments for the end of every class's queue of the pair stream, and
spmm_kernel keeps the tiles alone.  About 2 500 rows; the size gates lowered as tests/test_gpu_pair_stream.py lowers them, plus
``HUB_STREAM_MIN_NNZ``; blocks of 4 operand rows, chunks of 16 and 32 entries.  Rows of 5, 31, 32, 33, 511 and 512 twin pairs beside hub rows
of 513, 700, 3 000 and 20 000, tiled rows and, with ``min_pairs`` 9, walked rows that the row blocks must still reach.  The hub combine takes
64 x 8 = 512 segments of a row per trip of its loop and requests the next trip's ``row_seg`` entries inside the loop: the 3 000-pair row
(more than 64 segments, fewer than 512) ends in the first trip, a lane taking several entries of the one batch; the 20 000-pair row owns
more than 512 segments at chunk 32 and more than 1 024 at chunk 16 (asserted from the plan), so its wave takes a second and a third trip on
the entries requested in the loop, the last one partial — in every case here, the integer-exact ones included.  One more graph has no row
of 4 pairs or fewer: no tile, no walked row, ``spmm_kernel`` has nothing to launch.

Per-row bound, truth and magnitude ``rowwise._truth_mag``'s for the ORIGINAL graph (L_i its pairs, the self pair included):

    hub rows, m segments   k = chunk + 18 + ceil(m / 64)    counted from the kernels (tests/test_hub_stream_plan.py derives it): chunk - 1
                           adds in a segment's accumulators, 2 within the lane, <= 6 butterfly steps, ceil(m / 64) - 1 adds of a combine
                           lane, 6 butterfly steps, the multiply, 3 for the folded weight, two fmaf.  m is read from the plan.  Never above
                           the min(256, L_i - 1) + ceil((L_i - 1) / 64) + 24 of tests/test_gpu_blocked_hubs.py (asserted).
    stream rows            k = L_i + 13    tests/test_gpu_pair_stream.py's: unchanged segments, unchanged bits.
    every other row        ``rowwise.reference``'s k (fused read-out): unchanged code, unchanged bits.

With ``HUB_STREAM = False`` the launch is the parent's: every row outside the hubs has the same bits either way (the hub rows' pairs follow
the other rows' in a class's queue, so no chunk cut of theirs moves), the hub rows meet the blocked hubs' bound.  A zero bound demands an
exact zero; no element is left out.  Worst |err| / bound over the hub rows as measured on an MI355X: 0.002 in the
kernel cases ('range', W = 64, counts, blocks 2 + 4, chunk 32), 0.048 over all rows of the module case (profiles/r34_hub_stream_ab.txt)."""
import numpy as np
import pytest
import torch

import rowwise
from test_gpu_kernels import _graph
from test_gpu_pair_stream import MIX, _parts
from test_self_free_plan import self_graph

pytestmark = pytest.mark.gpu
DEV = "cuda"
N = 2504                                     # node N - 1 is listed by no row (the 'outlier' operand's large row)
LENGTHS = {38: 4, 39: 5, 40: 8, 41: 9, 42: 31, 43: 32, 44: 33, 45: 511, 46: 512, 47: 513, 48: 700, 49: 3000, 50: 20000}
TRIP = 64 * 8                                 # segments per trip of the hub combine's loop (kWave x kHubFly, csrc/spmm_stream.hip)
BLOCK_ROWS = 4
HUB_CAP = 256


def _lower(monkeypatch, W, min_pairs, n_blocks, hub_blocks, chunk):
    from gnan_amd import _lib, aggregate
    from gnan_amd import functional as Fn
    for name, v in (("DEGREE_SORTED_COPY_MIN_ROWS", 1), ("SELF_FROM_LOOKUP_MIN_ROWS", 0), ("CLASSED_MIN_NNZ", 1), ("CLASSED_ROWS_MIN_NNZ", 1),
                    ("BLOCKED_HUBS_MIN_NNZ", 1), ("PAIR_STREAM_MIN_NNZ", 1), ("HUB_STREAM_MIN_NNZ", 1), ("BLOCKED_HUB_BLOCKS", hub_blocks),
                    ("BLOCKED_HUB_SEG_PAIRS", HUB_CAP), ("BLOCKED_HUB_BLOCK_BYTES", BLOCK_ROWS * W * 4), ("PAIR_STREAM_MIN_PAIRS", min_pairs),
                    ("PAIR_STREAM_BLOCKS", n_blocks), ("PAIR_STREAM_CHUNK_PAIRS", chunk), ("HUB_STREAM_BLOCKS", hub_blocks),
                    ("HUB_STREAM_CHUNK_PAIRS", chunk)):
        monkeypatch.setattr(aggregate, name, v)
    monkeypatch.setattr(Fn, "FMLP_ALGO", _lib.FMLP_PWL)
    monkeypatch.setattr(Fn, "INDEX_MIN_NODES", 0)
    Fn._RANGE_CHURN.clear()


_CSR = {}


def _csr(D=3):
    """Every row: its self pair (code 0, in the middle) and the twin's pairs under code 1, drawn from a pool that holds 128 columns twenty
    times (the often listed ones) and every column but the last once."""
    if D not in _CSR:
        rng = np.random.default_rng(340 + D)
        lengths = rng.choice(MIX[0], N, p=MIX[1])
        for r, d in LENGTHS.items():
            lengths[r] = d
        pool = np.concatenate([np.tile(np.arange(8, 136), 20), np.arange(N - 1)])
        _CSR[D] = self_graph(rng, N, N, "middle", lengths, D, listed_cols=pool)
    return _CSR[D]


def _plan(g, min_pairs, n_blocks, hub_blocks, chunk):
    copy, order = g.self_free_plan(strict=False).twin.degree_sorted_copy()[:2]
    return copy.pair_stream_plan(min_pairs, BLOCK_ROWS, n_blocks, chunk, None, hub_blocks), order


def _bounds(g, rowptr, col, code, S, lut, cnt, tot, min_pairs, n_blocks, hub_blocks, chunk):
    """(truth, bound with the route on, bound with it off, hub mask, stream mask)."""
    truth, mag, deg = rowwise._truth_mag(rowptr, col, code, S, lut, cnt, tot)
    twin = deg - 1
    hub, stream = twin > 512, (twin >= min_pairs) & (twin <= 512)
    plan, order = _plan(g, min_pairs, n_blocks, hub_blocks, chunk)
    assert plan is not None and plan.q_hi == N and N - plan.q_hub == int(hub.sum()) == 4 and plan.max_hub_segs > (2 * TRIP if chunk == 16 else TRIP)
    segs = np.zeros(N)
    segs[order.cpu().numpy()[plan.q_lo:]] = np.diff(plan.row_slot_ptr.cpu().numpy())
    k_blocked = np.minimum(HUB_CAP, deg - 1) + np.ceil((deg - 1) / 64.0) + 24.0
    k_hub = chunk + 18.0 + np.ceil(segs / 64.0)
    assert (k_hub[hub] <= k_blocked[hub]).all() and (segs[hub] <= twin[hub]).all() and (segs[hub] > 0).all()
    k = np.where(stream, deg + 13.0, deg + 15.0)
    m = mag.sum(1, keepdims=True)
    return (truth.sum(1, keepdims=True), rowwise.gamma(np.where(hub, k_hub, k))[:, None] * m,
            rowwise.gamma(np.where(hub, k_blocked, k))[:, None] * m, hub, stream)


def _launch(monkeypatch, g, Sd, lut, use_cnt, s_total, self_sum, on, describe=None):
    from gnan_amd import aggregate
    monkeypatch.setattr(aggregate, "HUB_STREAM", on)
    plan = g.self_free_plan(strict=False)
    assert plan is not None
    return aggregate.spmm_launch(plan.twin, Sd, lut, use_cnt, True, s_total=s_total, reduce_cr=1, self_sum=self_sum, describe=describe)


def _check_describe(on, off, plan, W):
    assert on["n_stream_blocks"] > 0 and on["n_stream_blocks"] % 8 == 0 and on["n_stream_segs"] == plan.n_seg
    assert on["n_hub_seg_blocks"] == on["n_hub_segs"] == on["n_slice_blocks"] == on["n_seg_blocks"] == 0      # spmm_kernel: tiles (and walked rows)
    assert off["n_hub_seg_blocks"] > 0 and 0 < off["n_stream_segs"] < plan.n_seg
    for k in ("n_tiles", "n_tile_blocks", "row_q0", "lpr", "vec"):
        assert on[k] == off[k]
    assert on["n_tiles"] > 0 and on["lpr"] == rowwise.lanes_per_row(W)


# (W, parts, min_pairs, ranked blocks, the hub rows' ranked blocks, chunk)
EXACT = [(48, 1, 5, 2, 3, 16), (64, 2, 9, 3, 1, 32), (128, 1, 5, 1, 3, 32)]


@pytest.mark.parametrize("W,parts,min_pairs,n_blocks,hub_blocks,chunk", EXACT)
def test_integer_operands_are_exact_with_the_route_on_and_off(W, parts, min_pairs, n_blocks, hub_blocks, chunk, monkeypatch):
    from gnan_amd import functional as Fn
    _lower(monkeypatch, W, min_pairs, n_blocks, hub_blocks, chunk)
    D = 3
    rowptr, col, code = _csr(D)
    g = _graph(rowptr, col, code, N, D)
    rng = np.random.default_rng(W + parts)
    amp = 4 if W <= 48 else (2 if W <= 64 else 1)       # (the 20 000-pair row's magnitude, summed over W columns, stays below 2^24 quarters)
    S = torch.from_numpy(rng.integers(-amp, amp + 1, (N, W)).astype(np.float32))
    lut = torch.tensor([2.0, -1.0, 0.5]).view(D, 1)
    Sd = S.to(DEV)
    s_total = Fn.column_sums(Sd)
    t4, a4 = rowwise.exact_quarters(rowptr, col, code, S, lut, s_total.cpu(), 1)
    assert int(a4.max()) < 2 ** 24
    segs = _plan(g, min_pairs, n_blocks, hub_blocks, chunk)[0].max_hub_segs
    assert segs > (2 * TRIP if chunk == 16 else TRIP) and segs % TRIP % 64 != 0      # three trips (two at chunk 32), the last one partial
    want = (t4.double() / 4).float()
    self_sum = _parts(S, parts).to(DEV)
    d_on, d_off = [], []
    y_on = _launch(monkeypatch, g, Sd, lut.to(DEV), False, s_total, self_sum, True, d_on)
    y_off = _launch(monkeypatch, g, Sd, lut.to(DEV), False, s_total, self_sum, False, d_off)
    torch.cuda.synchronize()
    _check_describe(d_on[0], d_off[0], _plan(g, min_pairs, n_blocks, hub_blocks, chunk)[0], W)
    assert torch.equal(y_on.cpu(), want) and torch.equal(y_off.cpu(), want)


# (W, parts, counts, min_pairs, ranked blocks, the hub rows' ranked blocks, chunk)
CASES = [(48, 1, True, 5, 2, 3, 16), (64, 2, False, 9, 3, 1, 32), (64, 1, True, 5, 2, 4, 32), (128, 2, True, 9, 1, 3, 16)]


@pytest.mark.parametrize("family", ["unit", "range"])
@pytest.mark.parametrize("W,parts,use_cnt,min_pairs,n_blocks,hub_blocks,chunk", CASES)
def test_per_row_bound_same_bits_twice_and_rows_outside_the_hubs_keep_their_bits(family, W, parts, use_cnt, min_pairs, n_blocks, hub_blocks,
                                                                                 chunk, monkeypatch):
    from gnan_amd import functional as Fn
    _lower(monkeypatch, W, min_pairs, n_blocks, hub_blocks, chunk)
    D = 3
    rowptr, col, code = _csr(D)
    g = _graph(rowptr, col, code, N, D)
    rng = np.random.default_rng(W + parts + len(family))
    S = torch.from_numpy(rowwise.narrow_operand(rng, family, N, W))
    lut = torch.from_numpy(rng.standard_normal((D, 1)).astype(np.float32))
    Sd = S.to(DEV)
    s_total = Fn.column_sums(Sd)
    self_sum = _parts(S, parts).to(DEV)
    d, d_off = [], []
    y = _launch(monkeypatch, g, Sd, lut.to(DEV), use_cnt, s_total, self_sum, True, d)
    again = _launch(monkeypatch, g, Sd, lut.to(DEV), use_cnt, s_total, self_sum, True)
    off = _launch(monkeypatch, g, Sd, lut.to(DEV), use_cnt, s_total, self_sum, False, d_off)
    torch.cuda.synchronize()
    _check_describe(d[0], d_off[0], _plan(g, min_pairs, n_blocks, hub_blocks, chunk)[0], W)
    assert bool(torch.isfinite(y).all())
    truth, bound, bound_off, hub, stream = _bounds(g, rowptr, col, code, S, lut, g.cnt.cpu() if use_cnt else None, s_total.cpu(), min_pairs,
                                                   n_blocks, hub_blocks, chunk)
    assert all(stream[r] == (min_pairs <= LENGTHS[r] <= 512) and hub[r] == (LENGTHS[r] > 512) for r in LENGTHS)
    rowwise.assert_within(y.cpu(), truth, bound, f"{family} W={W} parts={parts}")
    ratio = rowwise.worst_ratio(y.cpu()[torch.from_numpy(hub)], truth[hub], bound[hub])
    print(f"ROW-BOUND worst |err|/bound {ratio:.3f} :: hub rows in the pair stream {family} W={W} parts={parts} cnt={use_cnt} "
          f"min_pairs={min_pairs} blocks={n_blocks}+{hub_blocks} chunk={chunk}")
    assert torch.equal(y.view(torch.int32), again.view(torch.int32))
    other = torch.from_numpy(~hub)
    assert torch.equal(y.cpu()[other].view(torch.int32), off.cpu()[other].view(torch.int32))       # HUB_STREAM = False: the parent's route
    rowwise.assert_within(off.cpu(), truth, bound_off, f"off {family} W={W}")


def test_a_graph_without_a_short_row_leaves_spmm_kernel_nothing_to_launch(monkeypatch):
    """Every row lists 5 pairs or more: no tile, no walked row — with the hub rows in the stream spmm_kernel's grid is empty and is not
    launched; exact for integer operands, route on and off."""
    from gnan_amd import functional as Fn
    W, D, n, min_pairs, n_blocks, hub_blocks, chunk = 64, 3, 600, 5, 2, 3, 16
    _lower(monkeypatch, W, min_pairs, n_blocks, hub_blocks, chunk)
    rng = np.random.default_rng(77)
    lengths = rng.integers(5, 31, n)
    lengths[[7, 300]] = 513, 900
    rowptr, col, code = self_graph(rng, n, n, "middle", lengths, D)
    g = _graph(rowptr, col, code, n, D)
    S = torch.from_numpy(rng.integers(-4, 5, (n, W)).astype(np.float32))
    lut = torch.tensor([2.0, -1.0, 0.5]).view(D, 1)
    Sd = S.to(DEV)
    s_total = Fn.column_sums(Sd)
    t4, a4 = rowwise.exact_quarters(rowptr, col, code, S, lut, s_total.cpu(), 1)
    assert int(a4.max()) < 2 ** 24
    self_sum = _parts(S, 1).to(DEV)
    d_on, d_off = [], []
    y_on = _launch(monkeypatch, g, Sd, lut.to(DEV), False, s_total, self_sum, True, d_on)
    y_off = _launch(monkeypatch, g, Sd, lut.to(DEV), False, s_total, self_sum, False, d_off)
    torch.cuda.synchronize()
    on, off = d_on[0], d_off[0]
    assert on["n_stream_blocks"] > 0 and on["n_tiles"] == on["n_tile_blocks"] == on["n_hub_seg_blocks"] == on["n_slice_blocks"] == 0
    assert on["row_q0"] == 0 and off["n_hub_seg_blocks"] > 0 and off["n_tiles"] == 0
    want = (t4.double() / 4).float()
    assert torch.equal(y_on.cpu(), want) and torch.equal(y_off.cpu(), want)


class Bag:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def test_module_takes_the_route_on_a_graph_of_70000_nodes(monkeypatch):
    """TensorGNAN, reference order, no_grad, F = 64, a graph large enough for the degree-sorted copy without lowering its gate:
    ``reference_order_inference`` hands the twin's launch the plan; twice the same bits; the rows outside the hubs as with the switch off."""
    import gnan_amd  # noqa: F401
    from gnan_amd import aggregate, models, replay
    from gnan_amd import synthetic as syn
    n, D, F = 70_001, 3, 64
    _lower(monkeypatch, F, 5, 2, 4, 32)
    monkeypatch.setattr(aggregate, "DEGREE_SORTED_COPY_MIN_ROWS", 1 << 16)        # (its shipped value: the graph is large enough)
    monkeypatch.setattr(aggregate, "BLOCKED_HUB_BLOCK_BYTES", 64 * F * 4)
    rng = np.random.default_rng(34)
    lengths = rng.choice(MIX[0], n, p=MIX[1])
    hubs = {100: 513, 2000: 700, 30_000: 1500, 69_000: 40_000}
    for r, d in hubs.items():
        lengths[r] = d
    # (vectorised self_graph: the self pair first under code 0, then the others under code 1, never the row itself)
    rowptr = np.zeros(n + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(lengths + 1)
    row = np.repeat(np.arange(n), lengths + 1)
    col = np.minimum((n * rng.random(len(row)) ** 3).astype(np.int64), n - 2).astype(np.int32)
    col[col == row] += 1
    code = np.ones(len(row), dtype=np.uint8)
    col[rowptr[:-1]], code[rowptr[:-1]] = np.arange(n), 0
    g = _graph(rowptr, col, code, n, D)
    x = syn.block_features(n, F, 0, n, seed=1, device=DEV)
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
        monkeypatch.setattr(aggregate, "HUB_STREAM", on)
        replay.release(mod)
        with torch.no_grad():
            return mod.forward(data).detach().clone()

    y, again, off = forward(True), forward(True), forward(False)
    torch.cuda.synchronize()
    assert len(took) == 3 and len(infos) == 3 and infos[0] == infos[1]
    assert infos[0]["n_stream_blocks"] > 0 and infos[0]["n_hub_seg_blocks"] == 0 and infos[2]["n_hub_seg_blocks"] > 0
    assert infos[0]["n_stream_segs"] > infos[2]["n_stream_segs"] > 0
    plan = g.self_free_plan(strict=False).twin.degree_sorted_copy()[0].pair_stream_plan(5, 64, 2, 32, None, 4)     # (the launch's: cached)
    assert plan.n_seg == infos[0]["n_stream_segs"] and plan.max_hub_segs > 2 * TRIP       # the 40 000-pair row: three trips and more
    with torch.no_grad():
        fx, total = mod._operand(x, "fs", mod.fs, False, True, pad_ok=True)
        lut = mod._lut_global(g)
    truth, mag, deg = rowwise._truth_mag(rowptr, col, code, fx.cpu(), lut.cpu(), g.cnt.cpu(), total.cpu())
    hub = (deg - 1) > 512
    assert int(hub.sum()) == len(hubs)
    # a hub row's k with m <= L_i - 1 segments (the kernel cases read m from the plan)
    k_hub = aggregate.HUB_STREAM_CHUNK_PAIRS + 18.0 + np.ceil((deg - 1) / 64.0)
    assert (k_hub[hub] <= np.minimum(HUB_CAP, deg[hub] - 1) + np.ceil((deg[hub] - 1) / 64.0) + 24.0).all()
    k = np.where(hub, k_hub, np.where(deg - 1 >= 5, deg + 13.0, deg + 15.0))
    bound = rowwise.gamma(k)[:, None] * mag.sum(1, keepdims=True)
    ratio = rowwise.assert_within(y.cpu(), truth.sum(1, keepdims=True), bound, "module")
    print(f"ROW-BOUND worst |err|/bound {ratio:.3f} :: module, hub rows in the pair stream")
    assert torch.equal(y.view(torch.int32), again.view(torch.int32))
    other = torch.from_numpy(~hub)
    assert torch.equal(y.cpu()[other].view(torch.int32), off.cpu()[other].view(torch.int32))
    replay.release(mod)
