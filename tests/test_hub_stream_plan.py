"""CPU tests of the pair stream that ends with the hub rows (``HopGraph.pair_stream_plan(..., max_pairs=None, hub_blocks=...)``,
``gnan_spmm_args.q_hub``, ``aggregate.HUB_STREAM``): the plan against a plain restatement, its properties one assertion each, a float32
emulation of spmm_stream_kernel, spmm_stream_combine_kernel and spmm_stream_hub_combine_kernel (csrc/spmm_stream.hip) against float64,
and what aggregate.spmm_launch hands the library (the recording stand-in of tests/test_wide_route_args.py).  Degree-sorted graphs of 700
rows with rows of 5, 31, 32, 33, 511, 512, 513, 700, 3 000 and 20 000 pairs, blocks of 4 operand rows, 1 and 3 ranked blocks, chunks of 16
and 32 entries.  spmm_stream_hub_combine_kernel takes 64 x 8 = 512 segments of a row per trip of its loop (a lane the entries l, l + 64, ...,
l + 448 of the batch) and requests the next trip's ``row_seg`` entries inside the loop: the 3 000-pair row (121 .. 205 segments) ends in
the first trip with some lanes idle in its last turn, the 20 000-pair row owns more than 512 segments at either chunk (more than 1 024 at
chunk 16): its wave takes a second and a third trip on the entries requested in the loop, the last one partial.  The emulation walks
the same batches through the same clamped indices.

Per-row bound (L_i the row's pairs in the ORIGINAL graph, the self pair included; the twin lists L_i - 1):

    rows in front of the hubs   k = L_i + 13                     tests/test_pair_stream_plan.py's: the same segments, the same combine.
    hub rows, m segments        k = chunk + 18 + ceil(m / 64)     counted from the kernels: chunk - 1 adds in the accumulators of a segment
                                (a segment holds at most a chunk), 2 within the lane, log2(LPR) <= 6 butterfly steps, ceil(m / 64) - 1
                                adds of a combine lane over its slots l, l + 64, ..., its 6 butterfly steps, the multiply by the folded
                                weight (two divisions and the fold: 3), the two fmaf of the rest and self terms:
                                (chunk - 1) + 2 + 6 + (ceil(m / 64) - 1) + 6 + 1 + 3 + 2.
                                m <= L_i - 1 and chunk <= 64, so k never exceeds the min(256, L_i - 1) + ceil((L_i - 1) / 64) + 24 that
                                tests/test_gpu_blocked_hubs.py grants hub rows (asserted for every hub row).

A zero bound demands an exact zero; no element is left out.  Worst |err| / bound of the emulation over the hub rows here: 0.003 (W = 48, chunk 16)."""
import ctypes

import numpy as np
import pytest
import torch

import gnan_amd  # noqa: F401
from gnan_amd import _lib, aggregate, wide_plans
from gnan_amd import graph as G

import rowwise
from test_blocked_hub_plan import _blocks
from test_pair_stream_plan import LAST, PACK, _arrays, _fmaf, _graph, _restated, _sorted_csr, _walk, _weights, _with_self_pairs, f32
from test_wide_route_args import FIELDS, route  # noqa: F401  (the fixture)

N = 700
LENGTHS = (5, 31, 32, 33, 511, 512, 513, 700, 3000, 20000)
HUBS = 4
TRIP = 64 * 8                                  # segments per trip of the hub combine's loop (kWave x kHubFly, csrc/spmm_stream.hip)
BLOCK_ROWS = 4


def _case(seed):
    deg, rowptr, col, code = _sorted_csr(np.random.default_rng(seed), N, lengths=LENGTHS)
    assert deg[-HUBS:].tolist() == [513, 700, 3000, 20000] and deg[-HUBS - 1] == 512
    return deg, rowptr, col, code


def _restated_hubs(rowptr, col, code, n_blocks, hub_blocks, min_pairs, chunk):
    """The plan as gnan_hip.h and PairStreamPlan state it: a class's queue lists the rows of min_pairs .. 512 pairs by (block, row), then
    the hub rows by (block of their own, row); chunks, flags and segments over the whole queue."""
    deg = np.diff(rowptr)
    n = len(deg)
    rows = [q for q in range(n) if deg[q] >= min_pairs]
    q_hub = next(q for q in rows if deg[q] > 512)
    blocks = (_blocks(col, n, BLOCK_ROWS, n_blocks), _blocks(col, n, BLOCK_ROWS, hub_blocks))
    index, seg_row, first_seg, pair_ptr, chunk_ptr = [], [], [], [0], [0]
    for c in range(8):
        queue = []
        for part, nb in ((0, n_blocks), (1, hub_blocks)):
            mine = [q for q in rows if (q >= q_hub) == bool(part)]
            queue += [(q, k) for b in range(nb + 1) for q in mine for k in range(rowptr[q], rowptr[q + 1])
                      if (col[k] & 7) == c and blocks[part][col[k]] == b]
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
    seg_row = np.array(seg_row)
    row_seg = np.argsort(seg_row, kind="stable")
    slot = np.empty(len(seg_row), dtype=np.int64)
    slot[row_seg] = np.arange(len(seg_row))
    row_slot_ptr = np.concatenate([[0], np.cumsum(np.bincount(seg_row - rows[0], minlength=len(rows)))])
    return dict(q_lo=rows[0], q_hi=n, index=index, cls_pair_ptr=np.array(pair_ptr), cls_chunk_ptr=np.array(chunk_ptr),
                chunk_first_seg=np.array(first_seg), seg_slot=slot, row_slot_ptr=row_slot_ptr), q_hub, seg_row


PLANS = [(1, 1, 16), (3, 3, 32), (1, 3, 32), (3, 1, 16)]


@pytest.mark.parametrize("n_blocks,hub_blocks,chunk", PLANS)
def test_the_plan_equals_the_restatement_and_the_four_argument_plan_is_the_cached_one(n_blocks, hub_blocks, chunk):
    deg, rowptr, col, code = _case(n_blocks + chunk)
    g = _graph(rowptr, col, code, N)
    before = g.pair_stream_plan(5, BLOCK_ROWS, n_blocks, chunk)
    plan = g.pair_stream_plan(5, BLOCK_ROWS, n_blocks, chunk, None, hub_blocks)
    want, q_hub, seg_row = _restated_hubs(rowptr, col, code, n_blocks, hub_blocks, 5, chunk)
    assert isinstance(plan, G.PairStreamPlan) and plan.code == 1 and plan.chunk_pairs == chunk
    got = _arrays(plan)
    for name, v in want.items():
        assert np.array_equal(got[name], v), name
    assert plan.q_hub == q_hub == N - HUBS and plan.q_hi == N and deg[plan.q_hub - 1] == 512
    per_row = np.diff(want["row_slot_ptr"])
    assert plan.max_hub_segs == int(per_row[q_hub - plan.q_lo:].max()) > (2 * TRIP if chunk == 16 else TRIP)    # a second (and third) trip
    assert plan.max_hub_segs % TRIP % 64 != 0 and 64 < per_row[-2] < TRIP             # ... the last one partial; the 3 000-pair row: one trip
    assert plan.n_seg == len(seg_row) < 2 ** 31 and int(want["cls_pair_ptr"][-1]) == int(deg[plan.q_lo:].sum())
    assert len(plan.block_pairs) == n_blocks + hub_blocks + 2 and sum(plan.block_pairs[:n_blocks + 1]) == int(deg[plan.q_lo:q_hub].sum())
    # every pair of the range exactly once, flags at segment ends and at chunk ends
    seen = {q: [] for q in range(plan.q_lo, N)}
    prev = None
    for c, t, j, cc, last, s in _walk(got, chunk):
        q = int(seg_row[s])
        seen[q].append(cc)
        if prev is not None and prev[0] == t:
            assert prev[1] == (prev[2] != q) and s == prev[3] + prev[1], "flags sit exactly at row changes inside a chunk"
        elif prev is not None:
            assert prev[1] and s == prev[3] + 1, "a chunk's last entry ends a segment"
        prev = (t, last, q, s)
    assert prev[1]
    for q in range(plan.q_lo, N):
        assert sorted(seen[q]) == sorted(col[rowptr[q]:rowptr[q + 1]].tolist()), "every pair of the range appears exactly once"
    # row_seg: a permutation, row by row, a row's segments in queue order
    row_seg = plan.row_seg.long().numpy()
    assert sorted(row_seg.tolist()) == list(range(plan.n_seg))
    for r in range(N - plan.q_lo):
        mine = row_seg[want["row_slot_ptr"][r]:want["row_slot_ptr"][r + 1]]
        assert (seg_row[mine] == plan.q_lo + r).all() and (np.diff(mine) > 0).all() and len(mine) > 0
    # the rows in front of the hubs keep their segments: the plan to 512 pairs is a prefix of every class's queue
    old = _arrays(before)
    for c in range(8):
        lo, n_old = int(got["cls_pair_ptr"][c]), int(old["cls_pair_ptr"][c + 1] - old["cls_pair_ptr"][c])
        assert np.array_equal(got["index"][lo:lo + n_old], old["index"][old["cls_pair_ptr"][c]:old["cls_pair_ptr"][c + 1]])
    # existing callers: the identical cached object, today's arrays, no hub row named
    assert g.pair_stream_plan(5, BLOCK_ROWS, n_blocks, chunk) is before and g.pair_stream_plan(5, BLOCK_ROWS, n_blocks, chunk, 512) is before
    assert before is not plan and before.q_hub == before.q_hi == q_hub and before.max_hub_segs == 0
    today = _restated(rowptr, col, code, _blocks(col, N, BLOCK_ROWS, n_blocks), n_blocks, 5, chunk)
    assert all(np.array_equal(old[k], v) for k, v in today.items())
    assert g.pair_stream_plan(5, BLOCK_ROWS, n_blocks, chunk, None, hub_blocks) is plan


def test_no_plan_for_two_codes_or_without_a_row_in_front_of_the_hubs():
    deg, rowptr, col, code = _case(2)
    two = code.copy()
    two[rowptr[N - 1] + 7] = 0                                                     # one pair of a hub row under another code
    g = _graph(rowptr, col, two, N)
    assert g.pair_stream_plan(5, BLOCK_ROWS, 2, 32, None, 4) is None and g.pair_stream_plan(5, BLOCK_ROWS, 2, 32) is not None
    assert _graph(rowptr, col, code, N).pair_stream_plan(513, BLOCK_ROWS, 2, 32, None, 4) is None      # hub rows alone
    assert _graph(rowptr, col, code, N).pair_stream_plan(5, BLOCK_ROWS, 2, 32, None, 0) is None
    d2, rp2, c2, k2 = _sorted_csr(np.random.default_rng(6), N, lengths=(5, 31, 32, 33, 511, 512))
    plan = _graph(rp2, c2, k2, N).pair_stream_plan(5, BLOCK_ROWS, 2, 32, None, 4)                     # no hub row: today's arrays
    assert plan is not None and plan.q_hub == plan.q_hi == N and plan.max_hub_segs == 0


def emulate(a, row_seg, q_hub, chunk, S, W, weights, s_total, self_term):
    """spmm_stream_kernel and the two combines in float32, add by add (partials in queue order; ``weights`` as test_pair_stream_plan's)."""
    lpr = rowwise.lanes_per_row(W)
    Sp = np.zeros((S.shape[0], lpr * 4), dtype=f32)
    Sp[:, :W] = S
    partial = np.full(len(row_seg), np.nan, dtype=f32)
    acc = np.zeros((lpr, 4), dtype=f32)
    for c, t, j, cc, last, s in _walk(a, chunk):
        acc = acc + Sp[cc].reshape(lpr, 4)
        if last:
            r = (acc[:, 0] + acc[:, 1]) + (acc[:, 2] + acc[:, 3])
            off = 1
            while off < lpr:
                r = r + r[np.arange(lpr) ^ off]
                off *= 2
            partial[s] = r[0]
            acc = np.zeros((lpr, 4), dtype=f32)
    T = f32(np.asarray(s_total, dtype=np.float64).sum())
    out = np.empty(a["q_hi"] - a["q_lo"], dtype=f32)
    ptr = a["row_slot_ptr"]
    for r in range(len(out)):
        mine = partial[row_seg[ptr[r]:ptr[r + 1]]]
        if a["q_lo"] + r < q_hub:                                   # a thread per row: one chain
            y = f32(0)
            for v in mine:
                y = f32(y + v)
        else:        # a wave per row, as the kernel walks it: trips of 8 entries per lane, the next trip's entries requested inside the loop
            s0, s1 = int(ptr[r]), int(ptr[r + 1])
            lanes = np.zeros(64, dtype=f32)
            for l in range(64):
                sg = [row_seg[min(s0 + l + 64 * u, s1 - 1)] for u in range(8)]
                s = s0 + l
                while s < s1:
                    v = [partial[g] for g in sg]
                    sg = [row_seg[min(s + 64 * (8 + u), s1 - 1)] for u in range(8)]
                    for u in range(8):
                        if s + 64 * u < s1:                          # (a select: the entry read again is dropped)
                            lanes[l] = f32(lanes[l] + v[u])
                    s += 64 * 8
            off = 32
            while off >= 1:
                lanes = lanes + lanes[np.arange(64) ^ off]
                off //= 2
            y = lanes[0]
        y = f32(weights[r, 0] * y)
        y = _fmaf(weights[r, 1], T, y)
        out[r] = _fmaf(weights[r, 2], self_term[r], y)
    return out


def hub_k(chunk, segs):
    return chunk + 18.0 + np.ceil(segs / 64.0)


@pytest.mark.parametrize("W,n_blocks,hub_blocks,chunk,use_cnt", [(48, 1, 3, 16, True), (64, 3, 1, 32, False), (128, 1, 1, 16, True)])
def test_the_emulated_association_holds_the_per_row_bound(W, n_blocks, hub_blocks, chunk, use_cnt):
    deg, rowptr, col, code = _case(W + chunk)
    plan = _graph(rowptr, col, code, N).pair_stream_plan(5, BLOCK_ROWS, n_blocks, chunk, None, hub_blocks)
    a = _arrays(plan)
    rows = np.arange(plan.q_lo, N)
    rng = np.random.default_rng(W)
    S = rng.standard_normal((N, W)).astype(f32) * f32(2.0) ** rng.integers(-3, 4, (N, 1)).astype(f32)
    lut = rng.standard_normal((3, 1)).astype(f32)
    cnt = rng.integers(1, 9, (N, 3)).astype(np.int32) if use_cnt else None
    s_total = S.astype(np.float64).sum(0).astype(f32)
    self_term = S.astype(np.float64).sum(1).astype(f32)
    y = emulate(a, plan.row_seg.long().numpy(), plan.q_hub, chunk, S, W, _weights(lut, cnt, rows, plan.code), s_total, self_term[rows])
    rp, c2, d2 = _with_self_pairs(rowptr, col, code)
    truth, mag, L = rowwise._truth_mag(rp, c2, d2, S, lut, cnt, s_total, rows=rows)
    hub = rows >= plan.q_hub
    segs = np.diff(a["row_slot_ptr"])
    k = np.where(hub, hub_k(chunk, segs), L + 13.0)
    assert (segs[hub] <= L[hub] - 1).all() and (k[hub] <= np.minimum(256, L[hub] - 1) + np.ceil((L[hub] - 1) / 64.0) + 24.0).all()
    bound = rowwise.gamma(k)[:, None] * mag.sum(1, keepdims=True)
    assert segs[-1] > TRIP and 64 < segs[-2] < TRIP                  # more than one trip of the combine's loop / one, partly idle
    y, t = torch.from_numpy(y), truth.sum(1, keepdims=True)
    rowwise.assert_within(y, t, bound, f"emulation W={W}")
    print(f"ROW-BOUND worst |err|/bound {rowwise.worst_ratio(y[hub], t[hub], bound[hub]):.3f} :: hub stream emulation, hub rows W={W} chunk={chunk}")
    # the rows in front of the hubs: the bits of the plan to 512 pairs
    from test_pair_stream_plan import emulate as emulate_today
    before = _graph(rowptr, col, code, N).pair_stream_plan(5, BLOCK_ROWS, n_blocks, chunk)
    r0 = np.arange(before.q_lo, before.q_hi)
    y0 = emulate_today(_arrays(before), chunk, S, W, _weights(lut, cnt, r0, before.code), s_total, self_term[r0])
    assert np.array_equal(y0.view(np.int32), y.numpy()[:len(r0)].view(np.int32))


# ------------------------------------------------------------------------------------------------- what spmm_launch hands the library
ON = (True, False, False, False)              # (stream, classed rows, blocked hubs, classed hub slices): the stream alone


@pytest.fixture
def hub_route(route, monkeypatch):  # noqa: F811
    monkeypatch.setattr(aggregate, "HUB_STREAM_MIN_NNZ", 1)
    return route


def _plan(g, W=64):
    copy = g.degree_sorted_copy()[0]
    return copy.pair_stream_plan(max(aggregate.PAIR_STREAM_MIN_PAIRS, aggregate.SHORT_ROW_LMAX + 1), max(1, aggregate.BLOCKED_HUB_BLOCK_BYTES // (W * 4)),
                                 aggregate.PAIR_STREAM_BLOCKS, aggregate.HUB_STREAM_CHUNK_PAIRS, None, aggregate.HUB_STREAM_BLOCKS)


def test_the_route_binds_the_stream_alone_and_names_the_first_hub_row(hub_route):
    a = hub_route.launch()
    assert hub_route.bound() == ON
    plan = _plan(hub_route.g)
    types = dict(_lib.SpmmArgs._fields_)
    for fld, attr in FIELDS["stream"].items():
        want = getattr(plan, attr)
        assert a[fld] == (_lib.ptr(want) if types[fld] is ctypes.c_void_p else want), fld
    assert a["q_hub"] == plan.q_hub == N - 2 and a["stream_q_hi"] == N and plan.q_hub < plan.q_hi
    for family in ("hubs", "rows", "slices"):                     # no blocked hub segments, no classed rows, nothing of the slice plan
        for fld in FIELDS[family]:
            if fld not in ("long_threshold", "slice_edges"):
                assert a[fld] in (None, 0), fld
    assert a["long_threshold"] == G.LONG_ROW_THRESHOLD == 512


TODAY = [
    ("a second hop code in a hub row", dict(g="two hub"), {}, (True, False, True, False)),     # the stream to 512 pairs and the blocked hubs
    ("a second hop code in a shorter row", dict(g="two"), {}, (False, True, True, False)),
    ("W = 32", dict(W=32), {}, (False, True, True, False)),
    ("bf16 rows", dict(dtype=torch.bfloat16), {}, (False, False, False, True)),
    ("HUB_STREAM off", {}, dict(HUB_STREAM=False), (True, False, True, False)),
    ("HUB_STREAM_MIN_NNZ above the graph", {}, dict(HUB_STREAM_MIN_NNZ=1 << 24), (True, False, True, False)),
    ("no hub row", dict(g="no hub"), {}, (True, False, False, False)),
    ("PAIR_STREAM off", {}, dict(PAIR_STREAM=False), (False, True, True, False)),            # the hub route is the pair stream, extended
    ("another chunk than the pair stream's", {}, dict(HUB_STREAM_CHUNK_PAIRS=64), (True, False, True, False)),
]


@pytest.mark.parametrize("label,call,switches,want", TODAY, ids=[c[0] for c in TODAY])
def test_each_of_these_binds_todays_route(hub_route, monkeypatch, label, call, switches, want):
    deg, rowptr, col, code = hub_route.csr
    from test_wide_route_args import _graph as route_graph, _sorted_csr as route_csr
    if call.get("g") in ("two", "two hub"):
        two = code.copy()
        two[rowptr[N - 1 if call["g"] == "two hub" else int(np.nonzero(deg >= 5)[0][0])]] = 0      # one pair under another code
        call = dict(call, g=route_graph(rowptr, col, two))
    elif call.get("g") == "no hub":
        d2, rp2, c2, k2 = route_csr(np.random.default_rng(6), N, lengths=(5, 5, 6, 16, 17, 31, 32, 33, 100, 300, 400, 511, 512, 512))
        call = dict(call, g=route_graph(rp2, c2, k2))
    hub_route.launch()
    assert hub_route.bound() == ON
    for name, value in switches.items():
        monkeypatch.setattr(aggregate, name, value)
    a = hub_route.launch(**call)
    assert hub_route.bound() == want, label
    if want[0]:                                                                 # today's stream: to the last row of 512 pairs, no hub row named
        assert a["q_hub"] in (0, a["stream_q_hi"]) and (label == "no hub row" or a["stream_q_hi"] < N)


def test_a_second_call_builds_nothing(hub_route, monkeypatch):
    built = []
    for name in ("long_row_plan", "classed_hub_plan", "classed_row_plan", "blocked_hub_plan", "pair_stream_plan"):
        real = getattr(wide_plans, name)
        monkeypatch.setattr(wide_plans, name, lambda *a, _real=real, _name=name, **kw: (built.append(_name), _real(*a, **kw))[1])
    a = hub_route.launch()
    assert "pair_stream_plan" in built and "blocked_hub_plan" not in built and "classed_row_plan" not in built
    before = _plan(hub_route.g)
    del built[:]
    b = hub_route.launch()
    assert built == [] and _plan(hub_route.g) is before
    assert all(a[f] == b[f] for fam in FIELDS.values() for f in fam) and a["q_hub"] == b["q_hub"]
