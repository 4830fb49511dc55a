"""``gnan_attr_reduce`` (csrc/attr_reduce.hip) through ``attribution.prepare_reduced``, every element of ``M [G, 3, D + 1, W]`` against
tests/attr_reduce_ref.py: both adjacency layouts, both rowptr widths, row_ids absent / permuted / repeating / one below, at and above
the block length with a group boundary inside a block, empty groups, counts (with zeros) or none, shared and per-row tables, one weight
channel or one per output channel, with and without s_total, listed codes past the cover — at the operand widths, shell counts and row
lengths where the kernels change path (``chunk`` and the block length come from ``gnan_attr_reduce_describe``).  Exact integer cases,
``gnan_attr_rows`` reduced on the host, planted errors the checker must reject, bit reproducibility, groups alone and among others,
and the split over several launches."""
import functools
import types

import numpy as np
import pytest
import torch

import attr_reduce_ref as ref
from gnan_amd import _lib, attribution

pytestmark = pytest.mark.gpu
DEV = "cuda"


def plan(D):
    """``(chunk_pairs, block_rows)`` of the library for ``D`` shells."""
    info = _lib.AttrReduceInfo()
    a = _lib.AttrReduceArgs(n_rows=1, n_cols=1, W=1, s_stride=1, D=D, Cw=1)
    assert _lib.lib().gnan_attr_reduce_describe(a, info) == 0
    return info.chunk_pairs, info.block_rows


# layout, rowptr dtype, W, D, Cw, cnt, per-row lut, s_total, row_ids ("none" / "perm" / "repeat" / "block-1" / "block" / "block+1"),
# n_cols, top listed code, groups ("one": group_ptr absent / "split": five groups, one empty, a boundary inside a block)
CASES = [
    ("csr", np.int64, 130, 3, 1, True, False, True, "block+1", 311, 255, "split"),     # three column tiles, the last ragged; two blocks
    ("csr", np.int32, 3, 2, 3, False, True, False, "repeat", 257, 1, "one"),           # 16 pair slots per wave; D = 2; per-row table
    ("csr", np.int32, 63, 64, 1, False, False, True, "perm", 300, 62, "split"),        # eight full passes
    ("csr", np.int64, 64, 65, 4, True, False, False, "none", 300, 64, "one"),          # one full tile; nine passes, the last of one shell
    ("csr", np.int32, 1, 256, 1, True, True, True, "block", 301, 254, "split"),        # 64 slots; 32 passes; exactly one multi-pass block
    ("csr", np.int32, 15, 3, 15, True, False, True, "block-1", 300, 254, "split"),     # Cw = C; codes past the cover beside s_total
    ("csr", np.int64, 65, 8, 5, True, False, True, "block", 300, 7, "one"),            # D = the pass length; one full block, one group
    ("dense", None, 65, 65, 5, True, False, False, "none", 301, 64, "one"),            # two tiles, one column in the second
    ("dense", None, 8, 256, 1, False, True, False, "block+1", 61, 255, "split"),       # dense rows of one chunk, per-row table, two blocks
    ("dense", None, 3, 5, 1, True, False, True, "perm", None, 4, "split"),             # dense rows of chunk + 3 pairs: chunk partials
]


def row_lengths(D):
    c = plan(D)[0]
    return [0, 1, c - 1, c, c + 1, 2 * c + 3, 5]


@functools.lru_cache(maxsize=None)
def inputs(idx, exact=False):
    """Host inputs of a case (numpy) and the float64 reference, computed once and shared."""
    layout, ptr_t, W, D, Cw, use_cnt, per_row, with_total, ids, n_cols, top, groups = CASES[idx]
    rng = np.random.default_rng(200 + idx)
    chunk, br = plan(D)
    if n_cols is None:
        n_cols = chunk + 3
    if layout == "csr":
        lens = np.array(row_lengths(D))
        n_adj = len(lens)
        rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(ptr_t)
        nnz = int(rowptr[-1])
        col = rng.integers(0, n_cols, nnz).astype(np.int32)
        code = rng.integers(0, min(top, D - 2) + 1, nnz).astype(np.uint8)
        if top > D - 2:                                             # out-of-contract codes: the rest shell, never past it
            code[rng.random(nnz) < 0.1] = top
            code[rng.random(nnz) < 0.05] = top - 1
    else:
        n_adj = 6
        rowptr = col = None
        code = rng.integers(0, D, (n_adj, n_cols)).astype(np.uint8)
        code[rng.random((n_adj, n_cols)) < 0.1] = top
        code[2] = 0                                                 # a row with one shell only: every other shell all-zero
    if exact:
        S = rng.integers(-4, 5, (n_cols, W)).astype(np.float32)
        lut = (2.0 ** rng.integers(-3, 4, (n_adj, D, Cw) if per_row else (D, Cw)) * rng.choice([-1.0, 1.0], (D, Cw))).astype(np.float32)
        cnt = (2 ** rng.integers(0, 4, (n_adj, D))).astype(np.int32) if use_cnt else None
    else:
        S = rng.standard_normal((n_cols, W)).astype(np.float32)
        lut = rng.standard_normal((n_adj, D, Cw) if per_row else (D, Cw)).astype(np.float32)
        cnt = rng.integers(0, 40, (n_adj, D)).astype(np.int32) if use_cnt else None            # 0: the max(cnt, 1) guard
    tot = S.astype(np.float64).sum(0).astype(np.float32) if with_total else None             # (exact: integer sums, exact in fp32)
    if ids in ("block-1", "block", "block+1"):
        R = br + {"block-1": -1, "block": 0, "block+1": 1}[ids]
        rows = rng.integers(0, n_adj, R).astype(np.int32)
        rows[-1] = rows[0] = n_adj - 2                              # the longest row in the first block and in the last
    else:
        rows = {"none": None, "perm": rng.permutation(n_adj).astype(np.int32),
                "repeat": np.array([n_adj - 1, 0, 2, n_adj - 1, 1, 2], dtype=np.int32)}[ids]
    R = n_adj if rows is None else len(rows)
    gp = None if groups == "one" else np.array([0, 1, 1, R // 2, R - 1, R], dtype=np.int64)
    host = dict(rowptr=rowptr, col=col, code=code, S=S, lut=lut, cnt=cnt, tot=tot, rows=rows, n_cols=n_cols, D=D, W=W, Cw=Cw,
                n_adj=n_adj, gp=gp, R=R)
    T, B = ref.row_terms(code, S, lut, rowptr, col, cnt, tot, rows)
    truth, bound = ref.moments(T, B, gp)
    return host, truth, bound, T, B


def graph_of(h):
    """What ``prepare_reduced`` reads of a ``HopGraph``, with the case's own counts (zeros included)."""
    t = lambda v: None if v is None else torch.from_numpy(np.ascontiguousarray(v)).to(DEV)      # noqa: E731
    return types.SimpleNamespace(n_codes=h["D"], n_cols=h["n_cols"], n_rows=h["n_adj"], code=t(h["code"]), device=torch.device(DEV, 0),
                                 is_dense=h["rowptr"] is None, rowptr=t(h["rowptr"]), col=t(h["col"]), cnt=t(h["cnt"]),
                                 nnz=0 if h["col"] is None else len(h["col"]))


def prepared(h, rows="same", gp="same"):
    t = lambda v: None if v is None else torch.from_numpy(np.ascontiguousarray(v)).to(DEV)      # noqa: E731
    rows = h["rows"] if isinstance(rows, str) else rows
    gp = h["gp"] if isinstance(gp, str) else gp
    return attribution.prepare_reduced(graph_of(h), t(h["S"]), t(h["lut"]), h["cnt"] is not None, t(rows),
                                       None if gp is None else torch.from_numpy(gp), t(h["tot"]))


def launch(h, rows="same", gp="same"):
    M = prepared(h, rows, gp).run()
    torch.cuda.synchronize()
    return M.cpu()


def bits(t):
    return t.contiguous().view(torch.int64)


@pytest.mark.parametrize("idx", range(len(CASES)))
def test_every_element_within_its_derived_bound_and_two_runs_give_equal_bits(idx):
    h, truth, bound, T, B = inputs(idx)
    got = launch(h)
    assert got.dtype == torch.float64 and tuple(got.shape) == truth.shape
    ref.check(got, truth, bound, f"case {idx} {CASES[idx][:5]}")
    assert torch.equal(bits(got), bits(launch(h)))
    zero = bound == 0
    assert (got.numpy()[zero] == truth[zero]).all()                 # an all-zero shell, an empty group: exactly zero
    if h["gp"] is not None:
        assert zero[1].all() and (got[1] == 0).all()                # the empty group


@pytest.mark.parametrize("idx", range(len(CASES)))
def test_exact_integer_cases_match_bit_for_bit(idx):
    h, truth, bound, T, B = inputs(idx, True)
    got = launch(h).numpy()
    assert np.array_equal(got, truth), f"case {idx}: {int((got != truth).sum())} elements differ from the exact result"
    assert (truth[:, 1] > 0).any() and (truth[:, 2, h["D"]] > 0).any()


@pytest.mark.parametrize("idx", [0, 2, 5, 9])
def test_agrees_with_attr_rows_reduced_on_the_host(idx):
    """``gnan_attr_rows`` on the same rows, its float32 terms reduced in float64 numpy: both routes lie within the per-term bound of
    the truth, so the moments differ by at most twice the derived bound."""
    from test_gpu_attr_rows import launch as rows_launch
    h, truth, bound, T, B = inputs(idx)
    A = rows_launch(h).double().numpy()                             # [R, D, W]
    tot = np.zeros_like(A[:, 0])
    for d in range(h["D"]):
        tot = tot + A[:, d]
    composed, _ = ref.moments(np.concatenate([A, tot[:, None]], 1), np.zeros((A.shape[0], h["D"] + 1, h["W"])), h["gp"])
    got = launch(h).numpy()
    assert (np.abs(got - composed) <= 2 * bound).all()
    ref.check(composed, truth, bound, "attr_rows reduced on the host")


@pytest.mark.parametrize("idx", [0, 4, 9])
def test_the_checker_rejects_planted_errors(idx):
    h, truth, bound, T, B = inputs(idx)
    got = launch(h).numpy()
    assert len(ref.violations(got, truth, bound)) == 0
    gp, D = h["gp"], h["D"]
    # one element off by twice its bound: a per-shell moment, the all-distances slot, the one-row group
    g_big = int(np.argmax(np.diff(gp)))
    for spot in ((g_big, 0, 0, 0), (g_big, 1, D, h["W"] - 1), (g_big, 2, D - 1, 0), (0, 1, D, 0)):
        assert bound[spot] > 0
        bad = got.copy()
        bad[spot] += 2 * bound[spot] * (1.0 if got[spot] >= truth[spot] else -1.0)
        v = ref.violations(bad, truth, bound)
        assert len(v) == 1 and tuple(v[0]) == spot, (spot, v)
        with pytest.raises(AssertionError, match="outside their bound"):
            ref.check(bad, truth, bound)
    # a dropped row: the moments of the group's rows but one
    q = int(gp[g_big]) + 1
    keep = np.ones(len(T), dtype=bool)
    keep[q] = False
    gp_less = gp.copy()
    gp_less[g_big + 1:] -= 1
    dropped, _ = ref.moments(T[keep], B[keep], gp_less)
    assert len(ref.violations(dropped, truth, bound)) > 0
    # the abs slot replaced by |sum|
    bad = got.copy()
    bad[:, 1] = np.abs(got[:, 0])
    assert len(ref.violations(bad, truth, bound)) > 0
    # a group boundary shifted by one row
    gp_shift = gp.copy()
    gp_shift[g_big + 1] -= 1
    shifted, _ = ref.moments(T, B, gp_shift)
    assert len(ref.violations(shifted, truth, bound)) > 0


@pytest.mark.parametrize("idx", [0, 4, 8, 9])
def test_a_group_has_the_same_bits_alone_as_among_the_others(idx):
    h, truth, bound, T, B = inputs(idx)
    gp = h["gp"]
    rows = np.arange(h["n_adj"], dtype=np.int32) if h["rows"] is None else h["rows"]
    everything = launch(h)
    for g in range(len(gp) - 1):
        mine = np.ascontiguousarray(rows[gp[g]:gp[g + 1]])
        alone = launch(h, rows=mine, gp=None)
        assert torch.equal(bits(alone[0]), bits(everything[g])), f"group {g}"
    # all rows as ONE group among none: what group_ptr = [0, R] gives
    assert torch.equal(bits(launch(h, gp=None)), bits(launch(h, gp=np.array([0, h["R"]], dtype=np.int64))))


@pytest.mark.parametrize("idx", [0, 5, 9])
def test_several_launches_give_the_bits_of_one(idx, monkeypatch):
    h, truth, bound, T, B = inputs(idx)
    one = prepared(h)
    assert len(one.calls) == 1
    want = one.run().cpu()
    monkeypatch.setattr(attribution, "ATTR_REDUCE_MAX_WORKSPACE", 1)
    split = prepared(h)
    assert len(split.calls) >= 2 and [c.combine for c in split.calls] == [0] * (len(split.calls) - 1) + [1]
    assert sum(c.block_count for c in split.calls) == one.calls[0].n_blocks
    got = split.run().cpu()
    assert torch.equal(bits(got), bits(want))
    ref.check(got, truth, bound, f"case {idx} in {len(split.calls)} launches")


def test_no_rows_and_groups_without_rows_give_exact_zeros():
    h, truth, bound, T, B = inputs(1)
    none = np.zeros(0, dtype=np.int32)
    M = launch(h, rows=none, gp=None)
    assert tuple(M.shape) == (1, 3, h["D"] + 1, h["W"]) and (M == 0).all()
    M = launch(h, rows=none, gp=np.array([0, 0, 0], dtype=np.int64))
    assert tuple(M.shape) == (2, 3, h["D"] + 1, h["W"]) and (M == 0).all()
    assert tuple(launch(h, rows=none, gp=np.array([0], dtype=np.int64)).shape) == (0, 3, h["D"] + 1, h["W"])
    with pytest.raises(ValueError, match="group_ptr must rise from 0"):
        prepared(h, gp=np.array([0, 4, 3, 6], dtype=np.int64))
    with pytest.raises(ValueError, match="group_ptr must rise from 0"):
        prepared(h, gp=np.array([0, 5], dtype=np.int64))
    with pytest.raises(_lib.GnanHipError, match="CPU tensor"):
        attribution.reduced_attributions(graph_of(h), torch.from_numpy(h["S"]), torch.from_numpy(h["lut"]).to(DEV), False)
