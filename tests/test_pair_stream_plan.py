"""CPU tests of the pair stream plan (HopGraph.pair_stream_plan, gnan_spmm_args.stream_*): the framework route against a plain numpy
restatement, array by array; the plan's properties one assertion each; the cases without a plan; and a numpy emulation of
spmm_stream_kernel's and spmm_stream_combine_kernel's association (csrc/spmm_stream.hip) held against ``rowwise``'s float64 truth.
The plan is taken on a degree-sorted copy (rows shortest first), so the graphs here are built sorted, one hop code throughout.
Graphs of 300 .. 900 nodes, blocks of 4 and 16 columns, 1 .. 3 ranked blocks, chunks of 16, 32 and 64 entries.

Per-row bound of a stream row (L_i its pairs in the ORIGINAL graph, the self pair included; the twin lists L_i - 1):

    k = L_i + 13     counted from the kernels as built: a gathered term meets the add chain of its segment (c adds for a segment of c
                     pairs), 2 adds within the lane, log2(LPR) <= 6 butterfly steps, the combine's chain over the row's m slots (m
                     adds) — and c + m <= L_i - 1, because m slots leave the longest segment at most L_i - 1 - (m - 1) pairs and the
                     first add of either chain is to an exact 0 —, then one multiply by the folded weight (two divisions and the
                     fold's subtraction: 3) and the two fmaf of the rest and self terms: (L_i - 1) + 2 + 6 + 1 + 3 + 2.  The rest term
                     (one division, the float64 total's cast, two fmaf) and the self term stay below that.  It never exceeds the
                     L_i + 24 the classed rows have.

A zero bound demands an exact zero; no element is left out.  Worst |err| / bound of the emulation here: 0.015 (W = 128, chunk 16)."""
import numpy as np
import pytest
import torch

import gnan_amd  # noqa: F401
from gnan_amd import HopGraph
from gnan_amd import graph as G

import rowwise
from test_blocked_hub_plan import _blocks

PACK = (1 << 29) - 1
LAST = 1 << 31


def _sorted_csr(rng, n, code=1, lengths=(5, 5, 6, 16, 17, 31, 32, 33, 100, 511, 512, 512, 513, 700)):
    """Rows shortest first: empty and short rows, rows of 5 .. 40 pairs, the named lengths.  A skewed column draw; one hop code."""
    deg = np.sort(np.concatenate([np.zeros(3, dtype=np.int64), rng.integers(1, 5, n // 3), rng.integers(5, 41, n - 3 - n // 3 - len(lengths)),
                                  np.asarray(lengths, dtype=np.int64)]), kind="stable")
    assert len(deg) == n
    rowptr = np.zeros(n + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(deg)
    col = np.minimum((n * rng.random(int(rowptr[-1])) ** 3).astype(np.int64), n - 1).astype(np.int32)
    return deg, rowptr, col, np.full(int(rowptr[-1]), code, dtype=np.uint8)


def _graph(rowptr, col, code, n, idx_dtype=torch.int64, packed=True, D=3):
    g = HopGraph.from_csr(torch.from_numpy(rowptr).to(idx_dtype), torch.from_numpy(col), torch.from_numpy(code), n_cols=n, n_codes=D)
    if packed:
        g.colp = g._packed_index()
    return g


def _restated(rowptr, col, code, block, n_blocks, min_pairs, chunk, max_pairs=512):
    """The plan as gnan_hip.h states it: class by class, block by block, row by row, pair by pair, a chunk at a time."""
    deg = np.diff(rowptr)
    rows = [q for q in range(len(deg)) if min_pairs <= deg[q] <= max_pairs]
    if not rows:
        return None
    assert rows == list(range(rows[0], rows[-1] + 1))
    index, seg_row, first_seg, pair_ptr, chunk_ptr = [], [], [], [0], [0]
    for c in range(8):
        queue = [(q, k) for b in range(n_blocks + 1) for q in rows for k in range(rowptr[q], rowptr[q + 1])
                 if (col[k] & 7) == c and block[col[k]] == b]
        for j0 in range(0, len(queue), chunk):
            first_seg.append(len(seg_row))
            piece = queue[j0:j0 + chunk]
            for j, (q, k) in enumerate(piece):
                if j == 0 or piece[j - 1][0] != q:
                    seg_row.append(q)
                last = j == len(piece) - 1 or piece[j + 1][0] != q
                index.append(int(col[k]) | (int(code[k]) << 29) | (LAST if last else 0))
        pair_ptr.append(len(index))
        chunk_ptr.append(len(first_seg))
    index = np.array(index, dtype=np.int64)
    index = np.where(index >= 1 << 31, index - (1 << 32), index)
    by_row = sorted(range(len(seg_row)), key=lambda s: (seg_row[s], s))       # the row-major enumeration: a row's segments in queue order
    slot = np.empty(len(seg_row), dtype=np.int64)
    slot[by_row] = np.arange(len(seg_row))
    row_slot_ptr = np.concatenate([[0], np.cumsum(np.bincount(np.array(seg_row) - rows[0], minlength=len(rows)))])
    return dict(q_lo=rows[0], q_hi=rows[-1] + 1, index=index, cls_pair_ptr=np.array(pair_ptr), cls_chunk_ptr=np.array(chunk_ptr),
                chunk_first_seg=np.array(first_seg), seg_slot=slot, row_slot_ptr=row_slot_ptr)


def _arrays(plan):
    return dict(q_lo=plan.q_lo, q_hi=plan.q_hi, index=plan.index.long().numpy().copy(), cls_pair_ptr=plan.cls_pair_ptr.long().numpy().copy(),
                cls_chunk_ptr=plan.cls_chunk_ptr.long().numpy().copy(), chunk_first_seg=plan.chunk_first_seg.long().numpy().copy(),
                seg_slot=plan.seg_slot.long().numpy().copy(), row_slot_ptr=plan.row_slot_ptr.long().numpy().copy())


def _walk(a, chunk):
    """Every entry of the plan as the kernel meets it: (class, chunk, position in the chunk, column, last flag, segment in queue order)."""
    idx = a["index"] & 0xFFFFFFFF
    for c in range(8):
        lo, hi = int(a["cls_pair_ptr"][c]), int(a["cls_pair_ptr"][c + 1])
        assert int(a["cls_chunk_ptr"][c + 1] - a["cls_chunk_ptr"][c]) == -(-(hi - lo) // chunk), "a class's chunks cover its pairs"
        for g in range(int(a["cls_chunk_ptr"][c + 1] - a["cls_chunk_ptr"][c])):
            t = int(a["cls_chunk_ptr"][c]) + g
            k = 0
            for j in range(min(chunk, hi - lo - g * chunk)):
                e = int(idx[lo + g * chunk + j])
                yield c, t, j, e & PACK, bool(e & LAST), int(a["chunk_first_seg"][t]) + k
                k += bool(e & LAST)


def _verify(a, rowptr, col, block, chunk, min_pairs):
    q_lo, q_hi = a["q_lo"], a["q_hi"]
    deg = np.diff(rowptr)
    assert (deg[q_lo:q_hi] >= min_pairs).all() and (deg[q_lo:q_hi] <= 512).all() and (q_lo == 0 or deg[q_lo - 1] < min_pairs)
    assert q_hi == len(deg) or deg[q_hi] > 512
    n_seg = len(a["seg_slot"])
    assert sorted(a["seg_slot"].tolist()) == list(range(n_seg)), "seg_slot is a permutation"
    ptr = a["row_slot_ptr"]
    assert ptr[0] == 0 and ptr[-1] == n_seg and len(ptr) == q_hi - q_lo + 1 and (np.diff(ptr) > 0).all()
    row_of_slot = np.repeat(np.arange(q_lo, q_hi), np.diff(ptr))
    per_row = {q: [] for q in range(q_lo, q_hi)}
    seen_segs, prev, order = set(), None, {}
    for c, t, j, cc, last, s in _walk(a, chunk):
        assert (cc & 7) == c, "a class's queue holds its class's columns"
        q = int(row_of_slot[a["seg_slot"][s]])
        key = (c, int(block[cc]), q)
        assert order.get(c, key) <= key, "the order is class-major, block-major, then by row"
        order[c] = key
        per_row[q].append(cc)
        if prev is not None and prev[0] == (c, t):
            assert prev[1] == (prev[2] != q), "flags sit exactly at row changes"
            assert s == prev[3] + prev[1], "a chunk's segments are consecutive from chunk_first_seg"
        elif prev is not None:
            assert prev[1], "a chunk's last entry ends a segment"
            assert s == prev[3] + 1, "chunk_first_seg continues the queue order"
        else:
            assert s == 0
        prev = ((c, t), last, q, s)
        seen_segs.add(s)
    assert prev[1] and seen_segs == set(range(n_seg))
    for q in range(q_lo, q_hi):       # every pair of the range exactly once, a row's pairs of one (class, block) in their own order
        rc = col[rowptr[q]:rowptr[q + 1]]
        assert sorted(per_row[q]) == sorted(rc.tolist()), "every pair of the range appears exactly once"
        want = [int(v) for c in range(8) for b in range(int(block.max()) + 1) for v in rc[((rc & 7) == c) & (block[rc] == b)]]
        assert per_row[q] == want
    # a row's slots follow the queue order of its segments
    slot_of_seg = a["seg_slot"]
    for q in range(q_lo, q_hi):
        mine = [s for s in range(n_seg) if row_of_slot[slot_of_seg[s]] == q] if n_seg < 4000 else None
        if mine is not None:
            assert [int(slot_of_seg[s]) for s in mine] == list(range(int(ptr[q - q_lo]), int(ptr[q - q_lo + 1])))


CASES = [(300, 4, 2, 5, 16), (400, 16, 1, 9, 32), (600, 4, 3, 17, 16), (900, 16, 3, 5, 64), (500, 4, 2, 33, 32)]


@pytest.mark.parametrize("n,block_rows,n_blocks,min_pairs,chunk", CASES)
@pytest.mark.parametrize("packed,idx_dtype", [(True, torch.int64), (False, torch.int32)])
def test_pair_stream_plan_equals_the_restatement(n, block_rows, n_blocks, min_pairs, chunk, packed, idx_dtype):
    rng = np.random.default_rng(n + chunk)
    deg, rowptr, col, code = _sorted_csr(rng, n)
    g = _graph(rowptr, col, code, n, idx_dtype, packed)
    block = _blocks(col, n, block_rows, n_blocks)
    plan = g.pair_stream_plan(min_pairs, block_rows, n_blocks, chunk)
    want = _restated(rowptr, col, code, block, n_blocks, min_pairs, chunk)
    assert isinstance(plan, G.PairStreamPlan) and plan.code == 1 and plan.chunk_pairs == chunk and plan.min_pairs == min_pairs
    assert all(t.dtype == torch.int32 for t in (plan.index, plan.cls_pair_ptr, plan.cls_chunk_ptr, plan.chunk_first_seg, plan.seg_slot,
                                                plan.row_slot_ptr))
    got = _arrays(plan)
    for name, v in want.items():
        assert np.array_equal(got[name], v), name
    assert plan.n_seg == len(want["seg_slot"]) and plan.n_chunks == len(want["chunk_first_seg"])
    assert plan.max_chunks_per_class == int(np.diff(want["cls_chunk_ptr"]).max())
    assert sum(plan.block_pairs) == len(want["index"]) == int(deg[plan.q_lo:plan.q_hi].sum()) and len(plan.block_pairs) == n_blocks + 1
    assert deg[plan.q_hi - 1] == 512 and deg[plan.q_hi] == 513
    assert plan.nbytes == 4 * sum(len(got[k]) for k in got if k not in ("q_lo", "q_hi"))
    again = _arrays(_graph(rowptr, col, code, n, idx_dtype, packed).pair_stream_plan(min_pairs, block_rows, n_blocks, chunk))
    assert all(np.array_equal(got[k], again[k]) for k in got)
    assert g.pair_stream_plan(min_pairs, block_rows, n_blocks, chunk) is plan
    assert g.pair_stream_plan(min_pairs, block_rows, n_blocks, chunk + 16) is not plan
    _verify(got, rowptr, col, block, chunk, min_pairs)
    # the shapes the kernel must meet are all here: a row over three chunks or more, a chunk of sixteen or more segments, a partial last chunk
    per_chunk = np.diff(np.concatenate([got["chunk_first_seg"], [plan.n_seg]]))
    assert per_chunk.max() >= 16 or chunk > 32 or min_pairs > 9
    assert any((got["cls_pair_ptr"][c + 1] - got["cls_pair_ptr"][c]) % chunk for c in range(8))


def test_a_planted_error_is_seen():
    rng = np.random.default_rng(3)
    deg, rowptr, col, code = _sorted_csr(rng, 300)
    block = _blocks(col, 300, 4, 2)
    a = _arrays(_graph(rowptr, col, code, 300).pair_stream_plan(5, 4, 2, 16))
    _verify(a, rowptr, col, block, 16, 5)
    b = dict(a, index=a["index"].copy())
    e = int(np.nonzero((b["index"] & LAST) == 0)[0][0])
    b["index"][e] = (int(b["index"][e]) | LAST) - (1 << 32)                      # a flag inside a segment
    with pytest.raises(AssertionError):
        _verify(b, rowptr, col, block, 16, 5)
    b = dict(a, seg_slot=np.arange(len(a["seg_slot"])))                          # slots in queue order
    with pytest.raises(AssertionError):
        _verify(b, rowptr, col, block, 16, 5)
    b = dict(a, chunk_first_seg=a["chunk_first_seg"] + (np.arange(len(a["chunk_first_seg"])) == 3))
    with pytest.raises(AssertionError):
        _verify(b, rowptr, col, block, 16, 5)


def test_no_plan_for_two_codes_an_empty_range_a_bad_chunk_or_unsorted_rows():
    rng = np.random.default_rng(1)
    deg, rowptr, col, code = _sorted_csr(rng, 300)
    assert _graph(rowptr, col, code, 300).pair_stream_plan(5, 4, 2, 16) is not None
    for chunk in (0, 8, 24, 40):
        assert _graph(rowptr, col, code, 300).pair_stream_plan(5, 4, 2, chunk) is None
    two = code.copy()
    q = int(np.nonzero(deg >= 5)[0][0])
    two[rowptr[q] + 2] = 0                                                      # one pair of the range under another code
    g = _graph(rowptr, col, two, 300)
    assert g.pair_stream_plan(5, 4, 2, 16) is None and g.pair_stream_plan(5, 4, 2, 16) is None
    outside = code.copy()
    outside[0] = 0                                                              # (a pair of a shorter row: not the stream's)
    assert deg[np.searchsorted(rowptr, 0, side="right") - 1] < 5
    assert _graph(rowptr, col, outside, 300).pair_stream_plan(5, 4, 2, 16) is not None
    assert _graph(rowptr, col, code, 300, D=5).pair_stream_plan(5, 4, 2, 16) is None          # bit 31 is the flag: codes stay below 4
    short = np.sort(np.concatenate([rng.integers(0, 5, 100), [600, 700]]))
    rp = np.zeros(103, dtype=np.int64)
    rp[1:] = np.cumsum(short)
    cs = rng.integers(0, 102, int(rp[-1])).astype(np.int32)
    assert _graph(rp, cs, np.ones(len(cs), dtype=np.uint8), 102).pair_stream_plan(5, 4, 2, 16) is None     # no row of 5 .. 512 pairs
    bad = np.zeros(4, dtype=np.int64)
    bad[1:] = np.cumsum([6, 2, 7])
    with pytest.raises(ValueError):
        _graph(bad, col[:15], code[:15], 300).pair_stream_plan(5, 4, 2, 16)


# ------------------------------------------------------------------------------------------------- the kernels' association in numpy
f32 = np.float32


def _fmaf(a, b, c):
    return f32(np.float64(a) * np.float64(b) + np.float64(c))     # (the product is exact in float64)


def emulate(a, chunk, S, W, weights, s_total, self_term):
    """spmm_stream_kernel and spmm_stream_combine_kernel in float32, add by add: ``weights [rows, 3]`` = (w_code - w_rest, w_rest,
    w_0 - w_rest) of the stream's rows as the combine forms them."""
    lpr = rowwise.lanes_per_row(W)
    Sp = np.zeros((S.shape[0], lpr * 4), dtype=f32)
    Sp[:, :W] = S
    partial = np.full(len(a["seg_slot"]), np.nan, dtype=f32)
    acc, at = np.zeros((lpr, 4), dtype=f32), None
    for c, t, j, cc, last, s in _walk(a, chunk):
        if at != t:
            assert not acc.any()
            at = t
        acc = acc + Sp[cc].reshape(lpr, 4)
        if last:
            r = (acc[:, 0] + acc[:, 1]) + (acc[:, 2] + acc[:, 3])
            off = 1
            while off < lpr:                                      # (the mirrors of the DPP steps pair lanes that hold one value)
                r = r + r[np.arange(lpr) ^ off]
                off *= 2
            partial[a["seg_slot"][s]] = r[0]
            acc = np.zeros((lpr, 4), dtype=f32)
    T = f32(np.asarray(s_total, dtype=np.float64).sum())
    out = np.empty(a["q_hi"] - a["q_lo"], dtype=f32)
    for r in range(len(out)):
        y = f32(0)
        for s in range(int(a["row_slot_ptr"][r]), int(a["row_slot_ptr"][r + 1])):
            y = f32(y + partial[s])
        y = f32(weights[r, 0] * y)
        y = _fmaf(weights[r, 1], T, y)
        out[r] = _fmaf(weights[r, 2], self_term[r], y)
    return out


def _with_self_pairs(rowptr, col, code):
    """The original graph of a twin: every row lists itself under code 0 behind its pairs."""
    n = len(rowptr) - 1
    rp = rowptr + np.arange(n + 1)
    c2, d2 = np.empty(int(rp[-1]), dtype=np.int32), np.empty(int(rp[-1]), dtype=np.uint8)
    for q in range(n):
        c2[rp[q]:rp[q + 1] - 1], d2[rp[q]:rp[q + 1] - 1] = col[rowptr[q]:rowptr[q + 1]], code[rowptr[q]:rowptr[q + 1]]
        c2[rp[q + 1] - 1], d2[rp[q + 1] - 1] = q, 0
    return rp, c2, d2


def _weights(lut, cnt, rows, code):
    lut = np.asarray(lut, dtype=f32).reshape(-1)
    rest = len(lut) - 1
    w = np.tile(lut, (len(rows), 1))
    if cnt is not None:
        w = (w / np.maximum(cnt[rows], 1).astype(f32)).astype(f32)
    listed = (w[:, code] - w[:, rest]).astype(f32) if code < rest else np.zeros(len(rows), dtype=f32)
    return np.stack([listed, w[:, rest], (w[:, 0] - w[:, rest]).astype(f32) if rest > 0 else np.zeros(len(rows), dtype=f32)], 1)


@pytest.mark.parametrize("W,chunk,min_pairs,use_cnt", [(48, 16, 5, True), (64, 32, 9, False), (128, 16, 5, True), (256, 64, 17, True)])
def test_the_emulated_association_holds_the_per_row_bound(W, chunk, min_pairs, use_cnt):
    n = 300
    rng = np.random.default_rng(W + chunk)
    deg, rowptr, col, code = _sorted_csr(rng, n)
    plan = _graph(rowptr, col, code, n).pair_stream_plan(min_pairs, 4, 2, chunk)
    a = _arrays(plan)
    rows = np.arange(plan.q_lo, plan.q_hi)
    S = rng.standard_normal((n, W)).astype(f32) * f32(2.0) ** rng.integers(-3, 4, (n, 1)).astype(f32)
    lut = rng.standard_normal((3, 1)).astype(f32)
    cnt = rng.integers(1, 9, (n, 3)).astype(np.int32) if use_cnt else None
    s_total = S.astype(np.float64).sum(0).astype(f32)
    self_term = S.astype(np.float64).sum(1).astype(f32)
    y = emulate(a, chunk, S, W, _weights(lut, cnt, rows, plan.code), s_total, self_term[rows])
    rp, c2, d2 = _with_self_pairs(rowptr, col, code)
    truth, mag, L = rowwise._truth_mag(rp, c2, d2, S, lut, cnt, s_total, rows=rows)
    assert (L == deg[rows] + 1).all()
    k = L + 13.0
    assert (k <= L + 24.0).all()
    bound = rowwise.gamma(k)[:, None] * mag.sum(1, keepdims=True)
    ratio = rowwise.assert_within(torch.from_numpy(y), truth.sum(1, keepdims=True), bound, f"emulation W={W}")
    print(f"ROW-BOUND worst |err|/bound {ratio:.3f} :: pair stream emulation W={W} chunk={chunk}")


@pytest.mark.parametrize("W,chunk", [(48, 16), (64, 64)])
def test_the_emulation_is_exact_for_integer_operands_and_power_of_two_weights(W, chunk):
    n = 300
    rng = np.random.default_rng(W)
    deg, rowptr, col, code = _sorted_csr(rng, n)
    plan = _graph(rowptr, col, code, n).pair_stream_plan(5, 4, 2, chunk)
    rows = np.arange(plan.q_lo, plan.q_hi)
    S = rng.integers(-4, 5, (n, W)).astype(f32)
    lut = np.array([[2.0], [-1.0], [0.5]], dtype=f32)
    s_total = S.sum(0)
    y = emulate(_arrays(plan), chunk, S, W, _weights(lut, None, rows, plan.code), s_total, S.sum(1)[rows])
    rp, c2, d2 = _with_self_pairs(rowptr, col, code)
    t4, a4 = rowwise.exact_quarters(rp, c2, d2, torch.from_numpy(S), torch.from_numpy(lut), torch.from_numpy(s_total), 1)
    assert int(a4.max()) < 2 ** 24
    assert np.array_equal(y, (t4.double() / 4).float().numpy().reshape(-1)[rows])


def test_only_the_self_term_route_of_large_one_code_graphs_takes_the_stream(monkeypatch):
    """The gate of aggregate.spmm_launch, read from the arguments it hands the library (a recording stand-in of gnan_spmm_fwd)."""
    from gnan_amd import _lib, aggregate
    rng = np.random.default_rng(5)
    n = 700
    deg, rowptr, col, code = _sorted_csr(rng, n)
    seen = []

    class Lib:
        def gnan_spmm_fwd_workspace_bytes(self, a):
            return 0

        def gnan_spmm_fwd(self, a, st):
            seen.append((a.stream_index is not None, a.seg_index is not None, a.hub_index is not None, a.stream_q_lo, a.stream_q_hi,
                         a.stream_chunk, a.stream_code, a.n_stream_seg, a.stream_max_chunks_per_class))
            return 0

    monkeypatch.setattr(_lib, "lib", lambda: Lib())
    monkeypatch.setattr(_lib, "require_device", lambda *t: None)
    monkeypatch.setattr(_lib, "stream_of", lambda t: 0)
    monkeypatch.setattr(aggregate, "DEGREE_SORTED_COPY_MIN_ROWS", 1)
    monkeypatch.setattr(G, "SORTED_COPY_IN_HIP", False)
    for name in ("CLASSED_MIN_NNZ", "CLASSED_ROWS_MIN_NNZ", "BLOCKED_HUBS_MIN_NNZ"):      # (the older gates are not this route's)
        monkeypatch.setattr(aggregate, name, 1)
    lut = torch.tensor([[0.5], [0.25], [0.1]])
    S, tot, self_sum = torch.zeros(n, 64), torch.zeros(64), torch.zeros(2, n)

    def launch(g, S=S, **kw):
        aggregate.spmm_launch(g, S, lut, True, True, s_total=tot, **kw)

    g = _graph(rowptr, col, code, n, packed=False)
    launch(g, reduce_cr=1, self_sum=self_sum)                                    # below PAIR_STREAM_MIN_NNZ
    monkeypatch.setattr(aggregate, "PAIR_STREAM_MIN_NNZ", 1)
    launch(g, reduce_cr=1, self_sum=self_sum)                                    # the route
    launch(g, reduce_cr=1)                                                       # no self term: generic forward
    launch(g)                                                                    # all columns stored
    launch(g, S.bfloat16(), reduce_cr=1, self_sum=self_sum)                      # bf16 rows
    two = code.copy()
    two[rowptr[int(np.nonzero(deg >= 5)[0][0])]] = 0
    launch(_graph(rowptr, col, two, n, packed=False), reduce_cr=1, self_sum=self_sum)       # two codes: the classed rows
    monkeypatch.setattr(aggregate, "PAIR_STREAM", False)
    launch(g, reduce_cr=1, self_sum=self_sum)                                    # switched off
    assert [s[0] for s in seen] == [False, True, False, False, False, False, False]
    assert [s[1] for s in seen] == [True, False, False, False, False, True, True]          # the stream replaces the classed row plan
    assert seen[1][2] and seen[0][2]                                                        # ... and leaves the blocked hubs alone
    copy = g.degree_sorted_copy()[0]
    plan = copy.pair_stream_plan(aggregate.PAIR_STREAM_MIN_PAIRS, aggregate.BLOCKED_HUB_BLOCK_BYTES // 256, aggregate.PAIR_STREAM_BLOCKS,
                                 aggregate.PAIR_STREAM_CHUNK_PAIRS)
    assert seen[1][3:] == (plan.q_lo, plan.q_hi, aggregate.PAIR_STREAM_CHUNK_PAIRS, 1, plan.n_seg, plan.max_chunks_per_class)
    assert aggregate.PAIR_STREAM_CHUNK_PAIRS % 16 == 0 and aggregate.PAIR_STREAM_MIN_PAIRS > aggregate.SHORT_ROW_LMAX
