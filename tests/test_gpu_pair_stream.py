"""The pair stream of the reference-order inference route (``gnan_spmm_args.stream_*``, ``HopGraph.pair_stream_plan``, spmm_stream_kernel and
spmm_stream_combine_kernel in csrc/spmm_stream.hip): the twin's rows of ``PAIR_STREAM_MIN_PAIRS`` .. 512 pairs leave the row walk and the
classed row segments for one queue of pairs per column class, a chunk of it per lane group.  About 2 500 rows; the gates that keep small
graphs off the route are lowered as tests/test_gpu_blocked_hubs.py lowers them, plus ``PAIR_STREAM_MIN_NNZ``; blocks of 4 operand rows,
chunks of 16 and 32 entries.  Rows of ``min_pairs - 1``, ``min_pairs``, 32, 33, 511 and 512 twin pairs beside hub rows (513, 700), tiled
rows and — with ``min_pairs`` 9 — walked rows of 5 .. 8 pairs, all in one launch; a row whose pairs all fall in class 5 (it spans three
chunks and more), one listing only cold columns; no stream row lists a column of class 7 (a class with no pairs) and only one lists one
of class 3, five times (a class shorter than one chunk, every block of it but one empty).  The plan's shapes the kernel must meet — a
segment that ends exactly on a chunk end, a chunk of sixteen one-pair segments and more (more flushes than one index round holds slots
for when the chunk is 32), a partial last chunk — are asserted from the plan itself.

Per-row bound, truth and magnitude ``rowwise._truth_mag``'s for the ORIGINAL graph (L_i its pairs, the self pair included):

    stream rows       k = L_i + 13     counted from the kernels as built (tests/test_pair_stream_plan.py derives it): segment chain and
                      slot chain together at most the twin's L_i - 1 adds, 2 adds within the lane, log2(LPR) <= 6 butterfly steps, one
                      multiply by the folded weight (2 divisions and the fold: 3), the fmaf of the rest term, the self fmaf.  Never
                      above the L_i + 24 the classed rows have (asserted).
    hub rows          tests/test_gpu_blocked_hubs.py's k: unchanged code, unchanged bits.
    every other row   ``rowwise.reference``'s k (fused read-out): unchanged code, unchanged bits.

A zero bound demands an exact zero; no element is left out.  Worst |err| / bound over the stream rows as measured on an MI355X: 0.036
('range', W = 48, counts, min_pairs 5, chunk 16; profiles/r17_pair_stream_ab.txt)."""
import numpy as np
import pytest
import torch

import rowwise
from test_blocked_hub_plan import _blocks
from test_gpu_kernels import _graph
from test_self_free_plan import self_graph

pytestmark = pytest.mark.gpu
DEV = "cuda"
N = 2504                                     # node N - 1 is listed by no row (the 'outlier' operand's large row)
MIX = ([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 30], [.05, .35, .12, .1, .08, .06, .05, .05, .05, .05, .04])      # rowwise.short_csr's degree mix
PLANTED, ONE_CLASS, COLD = 46, 49, 50        # lists a class-3 column five times / all pairs in class 5 / cold columns only
LENGTHS = {38: 4, 39: 5, 40: 8, 41: 9, 42: 16, 43: 17, 44: 32, 45: 33, PLANTED: 100, 47: 511, 48: 512, ONE_CLASS: 300, COLD: 200,
           51: 513, 52: 700}
CLASS3_COL = 8 * 20 + 3
BLOCK_ROWS = 4
HUB_CAP = 256


def _lower(monkeypatch, W, min_pairs, n_blocks, chunk):
    from gnan_amd import _lib, aggregate
    from gnan_amd import functional as Fn
    for name, v in (("DEGREE_SORTED_COPY_MIN_ROWS", 1), ("SELF_FROM_LOOKUP_MIN_ROWS", 0), ("CLASSED_MIN_NNZ", 1), ("CLASSED_ROWS_MIN_NNZ", 1),
                    ("BLOCKED_HUBS_MIN_NNZ", 1), ("PAIR_STREAM_MIN_NNZ", 1), ("BLOCKED_HUB_BLOCKS", n_blocks), ("BLOCKED_HUB_SEG_PAIRS", HUB_CAP),
                    ("BLOCKED_HUB_BLOCK_BYTES", BLOCK_ROWS * W * 4), ("PAIR_STREAM_MIN_PAIRS", min_pairs), ("PAIR_STREAM_BLOCKS", n_blocks),
                    ("PAIR_STREAM_CHUNK_PAIRS", chunk)):
        monkeypatch.setattr(aggregate, name, v)
    monkeypatch.setattr(Fn, "FMLP_ALGO", _lib.FMLP_PWL)
    monkeypatch.setattr(Fn, "INDEX_MIN_NODES", 0)
    Fn._RANGE_CHURN.clear()


_CSR = {}


def _csr(D):
    """Every row: its self pair (code 0, in the middle) and the twin's pairs, drawn from a pool that holds 128 columns twenty times (the
    often listed ones) and every column but the last once.  D = 3: one listed code (a stream); D = 4: two (no stream)."""
    if D not in _CSR:
        rng = np.random.default_rng(100 + D)
        lengths = rng.choice(MIX[0], N, p=MIX[1])
        for r, d in LENGTHS.items():
            lengths[r] = d
        pool = np.concatenate([np.tile(np.arange(8, 136), 20), np.arange(N - 1)])
        rowptr, col, code = self_graph(rng, N, N, "middle", lengths, D, listed_cols=pool)

        def twin(r):
            e = np.arange(rowptr[r], rowptr[r + 1])
            return e[col[e] != r]

        col[twin(ONE_CLASS)] = (col[twin(ONE_CLASS)] & ~7) | 5
        col[twin(COLD)] = rng.integers(1000, 2400, len(twin(COLD))).astype(np.int32)
        for r in np.nonzero((lengths >= 5) & (lengths <= 512))[0]:       # the rows a stream can take list no column of class 7 or 3
            e = twin(r)
            move = e[np.isin(col[e] & 7, (3, 7))]
            col[move] -= 1
            col[move[col[move] == r]] += 8
        col[twin(PLANTED)[10:20:2]] = CLASS3_COL
        # the shortest rows a stream takes (5 pairs, 9 pairs) list column 8 — the most listed of class 0 — once and no other column of
        # class 0: class 0's queue starts with a run of one-pair segments, a row each
        for r in np.nonzero(((lengths == 5) | (lengths == 9)) & (np.arange(N) > 16))[0]:
            e = twin(r)
            other = e[(col[e] & 7) == 0]
            col[other] += 1
            col[other[col[other] == r]] += 8
            col[e[0]] = 8
        row = np.repeat(np.arange(N), np.diff(rowptr))
        assert all((col[twin(r)] != r).all() and len(twin(r)) == lengths[r] for r in LENGTHS) and col[col != row].max() < N - 1
        assert (np.bincount(row[col == row], minlength=N) == 1).all()                         # every row still lists itself once
        _CSR[D] = (rowptr, col, code)
    return _CSR[D]


def _kinds(rowptr, min_pairs):
    twin = np.diff(rowptr) - 1
    return twin > 512, (twin >= min_pairs) & (twin <= 512)


def _parts(S, parts):
    n, W = S.shape
    return torch.from_numpy(np.ascontiguousarray(S.numpy().astype(np.float64).reshape(n, parts, W // parts).sum(2).T.astype(np.float32)))


def _bound(rowptr, col, code, S, lut, cnt, tot, min_pairs):
    truth, mag, deg = rowwise._truth_mag(rowptr, col, code, S, lut, cnt, tot)
    hub, stream = _kinds(rowptr, min_pairs)
    k = deg + 15.0                                                                        # rowwise.reference, fused read-out
    k = np.where(stream, deg + 13.0, k)
    assert (k[stream] <= deg[stream] + 24.0).all()                                        # the classed rows' k is the ceiling
    k = np.where(hub, np.minimum(HUB_CAP, deg - 1) + np.ceil((deg - 1) / 64.0) + 24.0, k)
    return truth.sum(1, keepdims=True), rowwise.gamma(k)[:, None] * mag.sum(1, keepdims=True)


def _launch(monkeypatch, g, Sd, lut, use_cnt, s_total, self_sum, on, describe=None):
    from gnan_amd import aggregate
    monkeypatch.setattr(aggregate, "PAIR_STREAM", on)
    plan = g.self_free_plan(strict=False)
    assert plan is not None
    return aggregate.spmm_launch(plan.twin, Sd, lut, use_cnt, True, s_total=s_total, reduce_cr=1, self_sum=self_sum, describe=describe)


def _stream_plan(g, min_pairs, n_blocks, chunk):
    return g.self_free_plan(strict=False).twin.degree_sorted_copy()[0].pair_stream_plan(min_pairs, BLOCK_ROWS, n_blocks, chunk)


def _check_plan_shapes(g, rowptr, col, min_pairs, n_blocks, chunk):
    """What the header promises of the graph, read from the plan the launch takes."""
    plan = _stream_plan(g, min_pairs, n_blocks, chunk)
    assert plan is not None and plan.code == 1
    _, stream = _kinds(rowptr, min_pairs)
    assert plan.q_hi - plan.q_lo == int(stream.sum())
    idx = plan.index.cpu().long().numpy() & 0xFFFFFFFF
    pp, cp = plan.cls_pair_ptr.cpu().numpy(), plan.cls_chunk_ptr.cpu().numpy()
    first = np.concatenate([plan.chunk_first_seg.cpu().numpy(), [plan.n_seg]])
    n_cls = np.diff(pp)
    assert n_cls[7] == 0 and 0 < n_cls[3] < chunk and cp[8] == plan.n_chunks                 # an empty class, one shorter than a chunk
    assert any(n % chunk for n in n_cls)                                                     # a partial last chunk
    assert np.diff(first).max() >= (17 if chunk > 16 else 16)                                # more flushes than one index round
    ones = (idx >> 31).astype(bool)
    row_of_slot = np.repeat(np.arange(plan.q_hi - plan.q_lo), np.diff(plan.row_slot_ptr.cpu().numpy()))
    seg_row = row_of_slot[plan.seg_slot.cpu().numpy()]                                       # (queue order)
    run, best, on_end = 1, 1, False
    for s in range(1, plan.n_seg):
        run = run + 1 if seg_row[s] == seg_row[s - 1] else 1
        best = max(best, run)
    assert best >= 3                                                                         # a row over three chunks and more
    for c in range(8):
        for t in range(cp[c], cp[c + 1] - 1):
            if seg_row[first[t + 1] - 1] != seg_row[first[t + 1]]:
                on_end = True                                                                # a segment that ends exactly on a chunk end
    assert on_end and ones[pp[1:][n_cls > 0] - 1].all()
    twin_row = np.repeat(np.arange(N), np.diff(rowptr))
    block = _blocks(col[col != twin_row], N, BLOCK_ROWS, n_blocks)
    e = np.arange(rowptr[COLD], rowptr[COLD + 1])
    assert (block[col[e[col[e] != COLD]]] == n_blocks).all()                                 # a row listing only cold columns
    assert len({int(block[c]) for c in idx[pp[3]:pp[4]] & ((1 << 29) - 1)}) == 1             # class 3: every block but one is empty
    return plan


def _check_describe(on, off, plan, W):
    assert on["n_stream_blocks"] > 0 and on["n_stream_blocks"] % 8 == 0 and on["n_stream_segs"] == plan.n_seg
    assert off["n_stream_blocks"] == 0 and off["n_stream_segs"] == 0
    assert on["n_seg_blocks"] == 0 and off["n_seg_blocks"] > 0                             # the stream replaces the classed rows
    for k in ("n_hub_seg_blocks", "n_hub_segs", "n_slice_blocks", "n_tiles", "n_tile_blocks", "row_q0", "lpr", "vec"):
        assert on[k] == off[k]
    assert on["n_hub_seg_blocks"] > 0 and on["n_tiles"] > 0 and on["lpr"] == rowwise.lanes_per_row(W)


# (W, parts, min_pairs, ranked blocks, chunk)
EXACT = [(48, 1, 5, 2, 16), (64, 2, 9, 3, 32), (128, 1, 5, 3, 16), (256, 2, 9, 2, 32)]


@pytest.mark.parametrize("W,parts,min_pairs,n_blocks,chunk", EXACT)
def test_integer_operands_are_exact_with_the_route_on_and_off(W, parts, min_pairs, n_blocks, chunk, monkeypatch):
    from gnan_amd import functional as Fn
    _lower(monkeypatch, W, min_pairs, n_blocks, chunk)
    D = 3
    rowptr, col, code = _csr(D)
    g = _graph(rowptr, col, code, N, D)
    rng = np.random.default_rng(W + parts)
    S = torch.from_numpy(rng.integers(-4, 5, (N, W)).astype(np.float32))
    lut = torch.tensor([2.0, -1.0, 0.5]).view(D, 1)
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
    _check_describe(d_on[0], d_off[0], _stream_plan(g, min_pairs, n_blocks, chunk), W)
    assert torch.equal(y_on.cpu(), want) and torch.equal(y_off.cpu(), want)


# (W, parts, counts, min_pairs, ranked blocks, chunk)
CASES = [(48, 1, True, 5, 2, 16), (64, 2, False, 9, 3, 32), (64, 1, True, 5, 3, 16), (128, 2, True, 9, 2, 16), (256, 1, False, 5, 3, 32)]


@pytest.mark.parametrize("family", ["unit", "range", "outlier"])
@pytest.mark.parametrize("W,parts,use_cnt,min_pairs,n_blocks,chunk", CASES)
def test_per_row_bound_reproducible_and_rows_outside_the_stream_keep_their_bits(family, W, parts, use_cnt, min_pairs, n_blocks, chunk,
                                                                               monkeypatch):
    from gnan_amd import functional as Fn
    _lower(monkeypatch, W, min_pairs, n_blocks, chunk)
    D = 3
    rowptr, col, code = _csr(D)
    g = _graph(rowptr, col, code, N, D)
    plan = _check_plan_shapes(g, rowptr, col, min_pairs, n_blocks, chunk)
    rng = np.random.default_rng(W + parts + len(family))
    S = torch.from_numpy(rowwise.narrow_operand(rng, family, N, W))           # 'outlier': 2^60 in the last row, which no row lists
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
    _check_describe(d[0], d_off[0], plan, W)
    assert bool(torch.isfinite(y).all())
    truth, bound = _bound(rowptr, col, code, S, lut, g.cnt.cpu() if use_cnt else None, s_total.cpu(), min_pairs)
    rowwise.assert_within(y.cpu(), truth, bound, f"{family} W={W} parts={parts}")
    _, stream = _kinds(rowptr, min_pairs)
    assert all(stream[r] == (LENGTHS[r] >= min_pairs) for r in LENGTHS if LENGTHS[r] <= 512)
    ratio = rowwise.worst_ratio(y.cpu()[torch.from_numpy(stream)], truth[stream], bound[stream])
    print(f"ROW-BOUND worst |err|/bound {ratio:.3f} :: pair stream rows {family} W={W} parts={parts} cnt={use_cnt} min_pairs={min_pairs} "
          f"blocks={n_blocks} chunk={chunk}")
    assert torch.equal(y, again)
    other = torch.from_numpy(~stream)
    assert torch.equal(y.cpu()[other].view(torch.int32), off.cpu()[other].view(torch.int32))       # PAIR_STREAM = False: the parent's route
    off_truth, off_bound = truth, _bound_off(rowptr, col, code, S, lut, g.cnt.cpu() if use_cnt else None, s_total.cpu())
    rowwise.assert_within(off.cpu(), off_truth, off_bound, f"off {family} W={W}")


def _bound_off(rowptr, col, code, S, lut, cnt, tot):
    """The route with the stream switched off: tests/test_gpu_blocked_hubs.py's bound."""
    from gnan_amd import aggregate
    truth, mag, deg = rowwise._truth_mag(rowptr, col, code, S, lut, cnt, tot)
    twin = deg - 1
    k = np.where((twin >= aggregate.CLASSED_ROWS_MIN_PAIRS) & (twin <= 512), deg + 24.0, deg + 15.0)
    k = np.where(twin > 512, np.minimum(HUB_CAP, deg - 1) + np.ceil((deg - 1) / 64.0) + 24.0, k)
    return rowwise.gamma(k)[:, None] * mag.sum(1, keepdims=True)


@pytest.mark.parametrize("W,chunk", [(64, 16), (128, 32)])
def test_an_inf_stays_out_of_every_row_that_does_not_list_it(W, chunk, monkeypatch):
    """The operand row behind the LAST entry of a class whose last chunk is partial — the row the slots past the chunk's end read
    again — holds an inf: the rows that list it become non-finite, every other row keeps its bits."""
    from gnan_amd import functional as Fn
    min_pairs, n_blocks, D = 5, 2, 3
    _lower(monkeypatch, W, min_pairs, n_blocks, chunk)
    rowptr, col, code = _csr(D)
    g = _graph(rowptr, col, code, N, D)
    plan = _stream_plan(g, min_pairs, n_blocks, chunk)
    pp = plan.cls_pair_ptr.cpu().numpy()
    c = next(c for c in range(8) if (pp[c + 1] - pp[c]) % chunk)
    j = int(plan.index.cpu().long().numpy()[pp[c + 1] - 1] & ((1 << 29) - 1))
    rng = np.random.default_rng(W)
    S = torch.from_numpy(rowwise.narrow_operand(rng, "unit", N, W))
    lut = torch.from_numpy(rng.standard_normal((D, 1)).astype(np.float32)).to(DEV)
    Sd = S.to(DEV)
    s_total = Fn.column_sums(Sd)
    self_sum = _parts(S, 1).to(DEV)
    Si = Sd.clone()
    Si[j] = float("inf")
    clean = _launch(monkeypatch, g, Sd, lut, True, s_total, self_sum, True)
    y = _launch(monkeypatch, g, Si, lut, True, s_total, self_sum, True)
    torch.cuda.synchronize()
    row = np.repeat(np.arange(N), np.diff(rowptr))
    lists = torch.from_numpy(np.bincount(row[(col == j) & (row != j)], minlength=N) > 0)
    assert 0 < int(lists.sum()) < N // 2 and bool(torch.isfinite(clean).all())
    assert not bool(torch.isfinite(y.cpu()[lists]).any())
    assert torch.equal(y.cpu()[~lists].view(torch.int32), clean.cpu()[~lists].view(torch.int32))


def test_a_two_code_graph_takes_the_classed_rows_with_unchanged_bits(monkeypatch):
    from gnan_amd import functional as Fn
    W, D = 64, 4
    _lower(monkeypatch, W, 5, 2, 16)
    rowptr, col, code = _csr(D)
    g = _graph(rowptr, col, code, N, D)
    assert _stream_plan(g, 5, 2, 16) is None
    rng = np.random.default_rng(9)
    S = torch.from_numpy(rowwise.narrow_operand(rng, "unit", N, W))
    lut = torch.from_numpy(rng.standard_normal((D, 1)).astype(np.float32)).to(DEV)
    Sd = S.to(DEV)
    s_total = Fn.column_sums(Sd)
    self_sum = _parts(S, 2).to(DEV)
    d_on, d_off = [], []
    on = _launch(monkeypatch, g, Sd, lut, True, s_total, self_sum, True, d_on)
    off = _launch(monkeypatch, g, Sd, lut, True, s_total, self_sum, False, d_off)
    torch.cuda.synchronize()
    assert d_on[0] == d_off[0] and d_on[0]["n_stream_blocks"] == 0 and d_on[0]["n_seg_blocks"] > 0
    assert torch.equal(on.view(torch.int32), off.view(torch.int32))
    truth, _ = _bound(rowptr, col, code, S, lut.cpu(), g.cnt.cpu(), s_total.cpu(), 5)
    rowwise.assert_within(off.cpu(), truth, _bound_off(rowptr, col, code, S, lut.cpu(), g.cnt.cpu(), s_total.cpu()), "two codes")
