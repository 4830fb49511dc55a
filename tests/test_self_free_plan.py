"""``HopGraph.self_free_plan`` against a numpy restatement, bit for bit, and the reference-order inference route's row formula
emulated in float32 in the kernels' own order, held to the per-row bound the GPU file (tests/test_gpu_self_from_lookup.py) uses.

The route (``aggregate.reference_order_inference``) evaluates, for output row i of L_i listed pairs (its self pair included),

    acc_c   = fma chain over the L_i - 1 pairs of the self-free twin, weights (w_d - w_rest), then fmaf(w_rest, tot_c, acc_c)
    red     = ((0 + acc_0) + acc_1 + acc_2) + acc_3 per lane of 4 columns, butterfly over the row's lanes
    a_i     = per feature group ((y_0 + y_1) + y_2) + y_3 per lane, butterfly over the group's TPN lanes; groups added in order
    Y_i     = fmaf(w_0 - w_rest, a_i, red)

``self_row_k`` counts the roundings one TERM of the truth can meet on its way into ``Y_i`` (a bound gamma_k A needs the largest
count over the terms, not their sum):

    a gathered term   2 divisions + the fold (3), the chain's L_i - 1 fmaf, fmaf(w_rest, tot) (1) — "L + 5" of tests/rowwise.py with
                      L_i - 1 pairs, one division counted for the rest weight's own term — then at most 4 in-lane adds and 6
                      butterfly steps (10), then the self fmaf (1):                 (L_i - 1) + 5 + 10 + 1 = L_i + 15
                      hub rows (more than the threshold's pairs in the TWIN): 2 (L_i - 1) + 10 + 1
    a self term       3 in-lane adds, log2(TPN) butterfly steps, parts - 1 adds of the groups, the weight's 2 divisions and fold (3),
                      the self fmaf (1):                                            6 + log2(TPN) + parts
"""
import numpy as np
import pytest
import torch

import rowwise
from gnan_amd import HopGraph

U32 = np.uint32


# ---- the plan ---------------------------------------------------------------------------------------------------------------------
def restate_plan(rowptr, col, code, n_cols, strict=True):
    """``None`` or ``(rowptr, col, code, listed words)`` of the self-free twin, in plain loops.  ``strict=False``: a row may list
    itself again under another code; those pairs stay."""
    n = len(rowptr) - 1
    keep = np.ones(len(col), dtype=bool)
    for i in range(n):
        own = [e for e in range(rowptr[i], rowptr[i + 1]) if col[e] == i]
        at = [e for e in own if code[e] == 0]
        if len(at) != 1 or (strict and len(own) != 1):
            return None
        keep[at[0]] = False
    words = np.zeros((n_cols + 31) // 32, dtype=np.uint64)
    for j in set(col[keep].tolist()):
        words[j >> 5] |= np.uint64(1) << np.uint64(j & 31)
    return np.asarray(rowptr) - np.arange(n + 1), col[keep], code[keep], words.astype(U32)


def graph_of(rowptr, col, code, n_cols, D=3, idx=torch.int64):
    return HopGraph.from_csr(torch.from_numpy(np.asarray(rowptr)).to(idx), torch.from_numpy(np.asarray(col, dtype=np.int32)),
                             torch.from_numpy(np.asarray(code, dtype=np.uint8)), n_cols=n_cols, n_codes=D)


def self_graph(rng, n, n_cols, where="first", lengths=None, D=3, listed_cols=None):
    """Every row lists itself once under code 0 — ``where`` among its pairs — and ``lengths[i]`` other nodes (never itself) under the
    codes 1 .. D - 2, drawn from ``listed_cols`` (default: all)."""
    lengths = rng.integers(0, 6, n) if lengths is None else np.asarray(lengths)
    pool = np.arange(n_cols) if listed_cols is None else np.asarray(listed_cols)
    rowptr, col, code = [0], [], []
    for i in range(n):
        others = rng.choice(pool[pool != i], int(lengths[i]), replace=True) if lengths[i] else np.zeros(0, dtype=np.int64)
        at = {"first": 0, "last": len(others), "middle": len(others) // 2}[where]
        col += list(others[:at]) + [i] + list(others[at:])
        code += list(rng.integers(1, max(D - 1, 2), at)) + [0] + list(rng.integers(1, max(D - 1, 2), len(others) - at))
        rowptr.append(len(col))
    return np.asarray(rowptr, dtype=np.int64), np.asarray(col, dtype=np.int32), np.asarray(code, dtype=np.uint8)


def check_plan(rowptr, col, code, n_cols, D=3, idx=torch.int64, strict=True):
    g = graph_of(rowptr, col, code, n_cols, D, idx)
    plan, want = g.self_free_plan(strict=strict), restate_plan(rowptr, col, code, n_cols, strict)
    if want is None:
        assert plan is None
        return None
    assert plan is not None and g.self_free_plan(strict=strict) is plan  # cached on the graph
    assert strict or (g.self_free_plan() is plan) == (restate_plan(rowptr, col, code, n_cols) is not None)
    t = plan.twin
    assert (t.n_rows, t.n_cols, t.n_codes) == (g.n_rows, g.n_cols, g.n_codes) and t.cnt is g.cnt
    assert t.rowptr.dtype == g.rowptr.dtype and t.col.dtype == torch.int32 and t.code.dtype == torch.uint8
    assert np.array_equal(t.rowptr.numpy(), want[0]) and np.array_equal(t.col.numpy(), want[1]) and np.array_equal(t.code.numpy(), want[2])
    assert plan.listed.dtype == torch.int32 and np.array_equal(plan.listed.numpy().view(U32), want[3])
    return plan


@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("idx", [torch.int32, torch.int64])
def test_self_pair_anywhere_in_the_row(where, idx):
    rng = np.random.default_rng(len(where))
    plan = check_plan(*self_graph(rng, 97, 97, where), 97, idx=idx)
    assert plan is not None and plan.twin.nnz > 0


def test_rows_without_or_with_a_wrong_self_pair_give_no_plan():
    rng = np.random.default_rng(1)
    rowptr, col, code = self_graph(rng, 40, 40, "middle", lengths=rng.integers(1, 5, 40))
    assert check_plan(rowptr, col, code, 40) is not None
    e = int(np.nonzero(col[rowptr[7]:rowptr[8]] == 7)[0][0]) + rowptr[7]
    c2 = col.copy()
    c2[e] = 8                                                            # row 7 without a self pair
    assert check_plan(rowptr, c2, code, 40) is None
    k2 = code.copy()
    k2[e] = 1                                                            # row 7 lists itself under code 1
    assert check_plan(rowptr, col, k2, 40) is None
    other = rowptr[7] if e != rowptr[7] else rowptr[7] + 1                # a second (7, 7, 0) pair
    c3, k3 = col.copy(), code.copy()
    c3[other], k3[other] = 7, 0
    assert check_plan(rowptr, c3, k3, 40) is None
    k4 = code.copy()                                                     # ... and a second self pair under another code
    k4[other] = 1
    assert check_plan(rowptr, c3, k4, 40) is None
    assert graph_of(rowptr[:-1], col[:rowptr[-2]], code[:rowptr[-2]], 38).self_free_plan() is None      # more rows than columns
    # what the inference route asks (strict=False): a second listing under ANOTHER code stays in the twin as an ordinary pair — an
    # edge list with self loops gives such rows — and node 7 is then listed; every other case above still has no plan
    plan = check_plan(rowptr, c3, k4, 40, strict=False)
    assert plan is not None and not plan.strict and plan.listed.numpy().view(U32)[0] >> 7 & 1
    assert 7 in plan.twin.col[plan.twin.rowptr[7]:plan.twin.rowptr[8]].tolist()
    assert check_plan(rowptr, c2, code, 40, strict=False) is None and check_plan(rowptr, c3, k3, 40, strict=False) is None
    assert check_plan(rowptr, col, k2, 40, strict=False) is None        # (its only self listing has code 1: no code-0 self pair)
    assert check_plan(rowptr, col, code, 40, strict=False).strict


def test_rows_listing_only_themselves_and_nodes_listed_by_nobody_one_or_themselves():
    n = 70
    rng = np.random.default_rng(2)
    lengths = np.zeros(n, dtype=np.int64)
    lengths[[3, 9, 40]] = [1, 4, 2]
    rowptr, col, code = self_graph(rng, n, n, "first", lengths, listed_cols=[5, 33, 64])
    col[rowptr[3] + 1] = 12                                              # node 12: listed by exactly one row
    plan = check_plan(rowptr, col, code, n)
    bits = np.unpackbits(plan.listed.numpy().view(np.uint8), bitorder="little")[:n]
    assert set(np.nonzero(bits)[0]) <= {5, 12, 33, 64} and bits[12] == 1 and bits[3] == 0 and bits[0] == 0
    assert np.array_equal(np.diff(plan.twin.rowptr.numpy()), lengths)
    only_self = self_graph(rng, n, n, "first", np.zeros(n, dtype=np.int64))
    plan = check_plan(*only_self, n)
    assert plan.twin.nnz == 0 and not plan.listed.any()


@pytest.mark.parametrize("n_cols", [31, 32, 33, 64 * 3 + 1])
def test_bit_words_at_the_word_edges(n_cols):
    rng = np.random.default_rng(n_cols)
    n = n_cols
    rowptr, col, code = self_graph(rng, n, n_cols, "last", rng.integers(0, 3, n))
    col[rowptr[0]] = n_cols - 1 if rowptr[1] - rowptr[0] > 1 else col[rowptr[0]]
    plan = check_plan(rowptr, col, code, n_cols)
    assert plan.listed.numel() == (n_cols + 31) // 32
    full = self_graph(rng, n, n_cols, "first", np.full(n, n_cols - 1), listed_cols=None)      # every node listed: all bits of the last word's live part
    rp, c, k = full
    for i in range(n):
        c[rp[i] + 1:rp[i + 1]] = np.delete(np.arange(n_cols), i)
    plan = check_plan(rp, c, k, n_cols)
    bits = np.unpackbits(plan.listed.numpy().view(np.uint8), bitorder="little")
    assert bits[:n_cols].all() and not bits[n_cols:].any()


def test_more_columns_than_rows_as_in_a_halo_graph():
    rng = np.random.default_rng(5)
    n, n_cols = 50, 83
    rowptr, col, code = self_graph(rng, n, n_cols, "middle", rng.integers(0, 7, n))
    plan = check_plan(rowptr, col, code, n_cols)
    assert plan.twin.n_cols == n_cols and plan.listed.numel() == 3


# ---- the row formula in float32, the kernels' order ---------------------------------------------------------------------------------
def f32(v):
    return np.asarray(v, dtype=np.float32)


def fma32(a, b, c):
    """fmaf on float32 arrays: the product of two float32 is exact in float64; the sum is rounded to float64 first, which can differ from
    the fused result in the last place once in ~2^29 cases — the emulation is held to a bound, not to the GPU's bits."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def butterfly(v, lanes):
    """``v [rows, lanes]``: every step adds the partner's value (offsets 1, 2, 4, ...); lane 0's result."""
    v = v.copy()
    off = 1
    while off < lanes:
        v = (v + v[:, np.arange(lanes) ^ off]).astype(np.float32)
        off *= 2
    return v[:, 0]


def lookup_row_sums(S, fg):
    """``row_sum [F / fg, n]`` of the look-up: per lane ((y0 + y1) + y2) + y3, butterfly over the fg / 4 lanes of the node."""
    n, F = S.shape
    out = np.empty((F // fg, n), dtype=np.float32)
    for g in range(F // fg):
        y = S[:, g * fg:(g + 1) * fg].reshape(n, fg // 4, 4)
        lane = ((y[:, :, 0] + y[:, :, 1]).astype(np.float32) + y[:, :, 2]).astype(np.float32)
        out[g] = butterfly((lane + y[:, :, 3]).astype(np.float32), fg // 4)
    return out


def emulate_route(rowptr, col, code, S, lut, cnt, tot, fg):
    """``Y [n]`` of the inference route in float32: the twin's chain, the read-out, the self fmaf over the part-ordered ``a_i``."""
    plan = restate_plan(rowptr, col, code, S.shape[0])
    rp, tc, tk, _ = plan
    n, W = len(rp) - 1, S.shape[1]
    D = len(lut)
    w = np.broadcast_to(f32(lut).reshape(1, D), (n, D)).copy()
    if cnt is not None:
        w = (w / np.maximum(cnt, 1).astype(np.float32)).astype(np.float32)
    w_rest = w[:, D - 1].copy() if tot is not None else np.zeros(n, dtype=np.float32)
    wf = (w - w_rest[:, None]).astype(np.float32) if tot is not None else w
    if tot is not None:
        wf[:, D - 1] = 0.0
    acc = np.zeros((n, W), dtype=np.float32)
    deg = np.diff(rp)
    for l in range(int(deg.max()) if n else 0):
        on = np.nonzero(deg > l)[0]
        e = rp[on] + l
        d = np.minimum(tk[e], D - 1)
        acc[on] = fma32(wf[on, d][:, None], S[tc[e]], acc[on])
    if tot is not None:
        acc = fma32(w_rest[:, None], f32(tot)[None, :], acc)
    lpr = rowwise.lanes_per_row(W)
    lanes = np.zeros((n, lpr, 4), dtype=np.float32)
    lanes.reshape(n, -1)[:, :W] = acc
    red = np.zeros((n, lpr), dtype=np.float32)
    for v in range(4):
        red = (red + lanes[:, :, v]).astype(np.float32)
    red = butterfly(red, lpr)
    parts = lookup_row_sums(S, fg)
    a = parts[0].copy()
    for g in range(1, parts.shape[0]):
        a = (a + parts[g]).astype(np.float32)
    return fma32(wf[:, 0], a, red), parts.shape[0]


def self_row_k(deg, parts, tpn, hub_threshold=rowwise.HUB_THRESHOLD):
    """The rounding count of the module docstring for rows of ``deg`` listed pairs (self pair included)."""
    deg = np.asarray(deg, dtype=np.float64)
    gathered = np.where(deg - 1 > hub_threshold, 2 * (deg - 1) + 11, deg + 15)
    return np.maximum(gathered, 6 + int(np.log2(tpn)) + parts)


def self_row_bound(rowptr, col, code, S, lut, cnt, tot, parts, tpn):
    """``(truth [n, 1], bound [n, 1])`` of the ORIGINAL graph with the route's own rounding count."""
    truth, bound = rowwise.reference(rowptr, col, code, S, lut, cnt, tot, reduce_cr=1)
    deg = np.diff(np.asarray(rowptr))
    k_ref = np.where(deg > rowwise.HUB_THRESHOLD, 2 * deg, deg + 5) + 10
    mag = bound / rowwise.gamma(k_ref)[:, None]
    return truth, rowwise.gamma(self_row_k(deg, parts, tpn))[:, None] * mag


@pytest.mark.parametrize("family", ["unit", "range", "outlier"])
@pytest.mark.parametrize("F,fg", [(64, 32), (48, 16), (64, 16)])
@pytest.mark.parametrize("use_cnt", [True, False])
def test_row_formula_in_float32_meets_the_per_row_bound(family, F, fg, use_cnt):
    rng = np.random.default_rng(F + fg + len(family))
    n, D = 300, 3
    lengths = rng.choice([0, 1, 2, 3, 4, 5, 9, 40], n)
    lengths[11] = 600                                                    # a hub row of the twin (its slices' order is not emulated:
    rowptr, col, code = self_graph(rng, n, n, "middle", lengths, D, listed_cols=np.arange(n - 1))    # the count covers any order)
    S = rowwise.narrow_operand(rng, family, n, F)
    lut = f32([0.9, -0.6, 0.45])
    g = graph_of(rowptr, col, code, n, D)
    cnt = g.cnt.numpy() if use_cnt else None
    tot = S.astype(np.float64).sum(0).astype(np.float32)
    y, parts = emulate_route(rowptr, col, code, S, lut, cnt, tot, fg)
    assert parts == F // fg
    truth, bound = self_row_bound(rowptr, col, code, S, lut.reshape(D, 1), cnt, tot, parts, fg // 4)
    ratio = rowwise.assert_within(y, truth, bound, f"{family} F={F} fg={fg}")
    print(f"ROW-BOUND worst |err|/bound {ratio:.3f} :: emulated self-term route {family} F={F} fg={fg} cnt={use_cnt}")
    assert np.isfinite(y).all()


def test_zero_operand_gives_exact_zeros():
    rng = np.random.default_rng(9)
    n, D, F = 60, 3, 64
    rowptr, col, code = self_graph(rng, n, n, "first", rng.integers(0, 5, n), D)
    S = np.zeros((n, F), dtype=np.float32)
    y, parts = emulate_route(rowptr, col, code, S, f32([0.9, -0.6, 0.45]), None, np.zeros(F, dtype=np.float32), 32)
    truth, bound = self_row_bound(rowptr, col, code, S, f32([0.9, -0.6, 0.45]).reshape(D, 1), None, np.zeros(F), parts, 8)
    assert not bound.any() and not y.any() and rowwise.assert_within(y, truth, bound) == 0.0
