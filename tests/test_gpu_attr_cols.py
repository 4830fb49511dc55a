"""``gnan_attr_cols`` (csrc/attr_cols.hip) through the C ABI, element by element against tests/attr_cols_ref.py: both layouts of
the transposed adjacency, both rowptr widths, col_ids absent / permuted / repeating, row_ids absent / a subset / with repeats /
empty, counts (holding 0) or none, shared and per-row tables, one weight channel or one per output channel, with and without
rest_from_total, listed codes past the cover — at the operand widths, shell counts and column lengths where the kernel changes
path (``chunk`` comes from ``gnan_attr_cols_describe``).  Exact integer cases (bit equality with the truth, with
``gnan_attr_rows`` summed over the rows and with ``gnan_spmm_fwd`` summed over the rows), planted errors the checker must reject,
bit reproducibility."""
import functools

import numpy as np
import pytest
import torch

import attr_cols_ref
import attr_ref
import test_gpu_attr_rows as rows_side
from gnan_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"


def chunk_pairs():
    info = _lib.AttrColsInfo()
    a = _lib.AttrColsArgs(n_cols=1, n_src=1, n_rows=1, n_row_ids=-1, W=1, s_stride=1, D=2, Cw=1, b_stride=2)
    assert _lib.lib().gnan_attr_cols_describe(a, info) == 0
    return info.chunk_pairs


# layout, rowptr dtype, W, D, Cw, cnt, per-row lut, rest_from_total, row_ids ("none" / "subset" / "repeat" / "empty"),
# col_ids ("none" / "perm" / "repeat"), forward rows, top listed code
CASES = [
    ("csr", np.int64, 130, 17, 1, True, False, True, "none", "none", 311, 255),      # every row; codes 254 / 255 beside the rest bucket
    ("csr", np.int32, 3, 2, 3, False, True, False, "repeat", "repeat", 257, 1),      # D = 2; Cw = C; per-row table; repeats on both sides
    ("csr", np.int32, 63, 64, 1, False, False, True, "subset", "perm", 300, 62),     # one pass of exactly 64 bins; V = T - sum on a listed column
    ("csr", np.int64, 64, 65, 4, True, False, False, "none", "none", 300, 64),       # 260 bins: five passes, the last of four
    ("csr", np.int32, 1, 256, 1, True, True, True, "repeat", "perm", 301, 254),      # W = 1; four passes; per-row table with counts
    ("csr", np.int32, 8, 17, 8, True, False, True, "empty", "repeat", 300, 254),     # no row requested: all of B is zero
    ("csr", np.int32, 8, 17, 8, True, False, True, "subset", "repeat", 300, 254),    # Cw = C beside the rest bucket; codes past the cover
    ("dense", None, 65, 65, 5, True, False, False, "none", "none", 300, 64),         # 6 x 300 entries; two column tiles' worth of W
    ("dense", None, 8, 256, 1, False, True, False, "repeat", "repeat", 203, 255),    # dense, per-row table, repeating ids
    ("dense", None, 3, 5, 1, True, False, True, "subset", "perm", None, 4),          # dense columns of chunk + 3 entries: partials in the workspace
]
N_DENSE = 6


def col_lengths():
    c = chunk_pairs()
    return [0, 1, c - 1, c, c + 1, 2 * c + 3, 5]


@functools.lru_cache(maxsize=None)
def inputs(idx, exact=False, in_cover=False):
    """Host inputs of a case (numpy) and the float64 reference, computed once and shared.  ``in_cover``: no listed code past the
    cover (what ``gnan_spmm_fwd``'s contract asks for)."""
    layout, ptr_t, W, D, Cw, use_cnt, per_row, rft, row_mode, col_mode, n_rows, top = CASES[idx]
    rng = np.random.default_rng(300 + idx)
    if n_rows is None:
        n_rows = chunk_pairs() + 3
    pool = rng.choice(n_rows, 12, replace=False)
    rows = {"none": None, "subset": np.sort(pool[:5]).astype(np.int32), "repeat": pool[[0, 1, 0, 2, 0, 3]].astype(np.int32),
            "empty": np.zeros(0, dtype=np.int32)}[row_mode]
    if layout == "csr":
        lens = np.array(col_lengths())
        n_src = len(lens)
        rowptr_t = np.concatenate([[0], np.cumsum(lens)]).astype(ptr_t)
        nnz = int(rowptr_t[-1])
        # with few rows requested the pairs come from a small pool of forward rows, so that most of them count (and repeat)
        row = (rng.integers(0, n_rows, nnz) if row_mode in ("none", "empty") else pool[rng.integers(0, len(pool), nnz)]).astype(np.int32)
        code = rng.integers(0, min(top, D - 2) + 1, nnz).astype(np.uint8)
        if top > D - 2:                                             # out-of-contract codes: the rest shell, never past it
            code[rng.random(nnz) < 0.1] = top
            code[rng.random(nnz) < 0.05] = top - 1
        if row_mode == "subset":                                    # the last column: listed by EVERY requested row below D - 1
            row[-5:] = rows
            code[-5:] = rng.integers(0, D - 1, 5)
    else:
        n_src = N_DENSE
        rowptr_t = row = None
        code = rng.integers(0, D, (n_src, n_rows)).astype(np.uint8)
        code[rng.random((n_src, n_rows)) < 0.1] = top
        code[2] = 0                                                 # a source every row sees at hop 0: every other shell all-zero
    if in_cover:
        code = np.minimum(code, D - 2 if layout == "csr" else D - 1).astype(np.uint8)
    shape = (n_rows, D, Cw) if per_row else (D, Cw)
    if exact:
        S = rng.integers(-4, 5, (n_src, W)).astype(np.float32)
        lut = (2.0 ** rng.integers(-3, 4, shape) * rng.choice([-1.0, 1.0], shape)).astype(np.float32)
        cnt = (2 ** rng.integers(0, 4, (n_rows, D))).astype(np.int32) if use_cnt else None
    else:
        S = rng.standard_normal((n_src, W)).astype(np.float32)
        lut = rng.standard_normal(shape).astype(np.float32)
        cnt = rng.integers(0, 40, (n_rows, D)).astype(np.int32) if use_cnt else None            # 0: the max(cnt, 1) guard
    cols = {"none": None, "perm": rng.permutation(n_src).astype(np.int32),
            "repeat": np.array([n_src - 1, 0, 2, n_src - 1, 1, 2], dtype=np.int32)}[col_mode]
    host = dict(rowptr_t=rowptr_t, row=row, code=code, S=S, lut=lut, cnt=cnt, rows=rows, cols=cols, rft=rft, n_rows=n_rows,
                n_src=n_src, D=D, W=W, Cw=Cw)
    truth, bound, mag = attr_cols_ref.reference(code, S, lut, rowptr_t, row, cnt, rows, cols, rft, n_rows)
    return host, truth, bound, mag


def launch(h, rows="same", cols="same", s_pad=0, item_ptr=True):
    """One call of gnan_attr_cols on the host inputs ``h``; ``rows`` / ``cols``: other id arrays (or None) than the case's."""
    t = lambda v: None if v is None else torch.from_numpy(np.ascontiguousarray(v)).to(DEV)      # noqa: E731
    rows = h["rows"] if isinstance(rows, str) else rows
    cols = h["cols"] if isinstance(cols, str) else cols
    S = t(h["S"])
    if s_pad:                                                        # an operand with a row stride, NaN behind every row
        S = torch.cat([S, torch.full((S.shape[0], s_pad), float("nan"), device=DEV)], 1)[:, : h["W"]]
    dev = dict(rowptr_t=t(h["rowptr_t"]), row=t(h["row"]), code=t(h["code"]), S=S, lut=t(h["lut"]), cnt=t(h["cnt"]),
               rows=t(rows), cols=t(cols))
    P = h["n_src"] if cols is None else len(cols)
    D, W = h["D"], h["W"]
    B = torch.full((P, D, W), float("nan"), device=DEV)
    a = _lib.AttrColsArgs(n_cols=P, n_src=h["n_src"], n_rows=h["n_rows"], code=_lib.ptr(dev["code"]), col_ids=_lib.ptr(dev["cols"]),
                          row_ids=_lib.ptr(dev["rows"]), n_row_ids=-1 if rows is None else len(rows), S=_lib.ptr(S), W=W,
                          s_stride=S.stride(0), lut=_lib.ptr(dev["lut"]), lut_row_stride=D * h["Cw"] if h["lut"].ndim == 3 else 0,
                          D=D, Cw=h["Cw"], rest_from_total=int(h["rft"]), B=_lib.ptr(B), b_stride=D * W)
    if h["cnt"] is not None:
        a.cnt, a.cnt_stride = _lib.ptr(dev["cnt"]), D
    if h["rowptr_t"] is not None:
        a.rowptr_t, a.rowptr_is64, a.row = _lib.ptr(dev["rowptr_t"]), int(h["rowptr_t"].dtype == np.int64), _lib.ptr(dev["row"])
        a.nnz = len(h["row"])
        lens = np.diff(h["rowptr_t"].astype(np.int64))
        lens = lens if cols is None else lens[np.asarray(cols)]
        a.max_col_pairs = int(lens.max())
        if item_ptr:                                                 # the per-source chunk list; without: the longest column's for all
            c = chunk_pairs()
            ptr = np.concatenate([[0], np.cumsum(np.maximum(1, -(-lens // c)))]).astype(np.int32)
            dev["item_ptr"] = t(ptr)
            a.item_ptr, a.n_items = _lib.ptr(dev["item_ptr"]), int(ptr[-1])
    need = _lib.lib().gnan_attr_cols_workspace_bytes(a)
    ws = torch.full(((need + 3) // 4,), float("nan"), device=DEV) if need else None
    a.workspace, a.workspace_bytes = _lib.ptr(ws), need
    _lib.check(_lib.lib().gnan_attr_cols(a, torch.cuda.current_stream().cuda_stream), "gnan_attr_cols")
    torch.cuda.synchronize()
    return B.cpu()


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("idx", range(len(CASES)))
def test_every_element_within_its_derived_bound(idx):
    h, truth, bound, mag = inputs(idx)
    got = launch(h)
    attr_ref.check(got, truth, bound, f"case {idx} {CASES[idx][:5]}")
    again = launch(h, s_pad=3)                                       # a second launch, the operand behind a row stride: equal bits
    assert torch.equal(bits(got), bits(again))
    if h["rowptr_t"] is not None:                                    # the uniform chunk list: equal bits again
        assert torch.equal(bits(got), bits(launch(h, item_ptr=False)))
    zero = bound == 0
    assert zero.any() and (got.numpy()[zero] == 0).all()            # a shell no requested row sees the source in: exactly zero
    if h["rows"] is not None and len(h["rows"]) == 0:
        assert zero.all()
    elif h["rft"]:                                                   # the rest shell carries T even for a source nobody lists
        assert (mag[:, h["D"] - 1] > 0).any(axis=1).all()


@pytest.mark.parametrize("idx", range(len(CASES)))
def test_exact_integer_cases_match_bit_for_bit(idx):
    h, truth, bound, mag = inputs(idx, True)
    got = launch(h).double().numpy()
    assert np.array_equal(got, truth), f"case {idx}: {int((got != truth).sum())} elements differ from the exact result"
    assert (got[mag == 0] == 0).all() and ((mag > 0).any() or len(h["rows"]) == 0)
    if h["rft"] and h["rowptr_t"] is not None and h["rows"] is not None and len(h["rows"]):
        cols = np.arange(h["n_src"]) if h["cols"] is None else h["cols"]
        unlisted = int(np.nonzero(cols == 0)[0][0])                  # column 0 has no pair: V = T, exactly
        lut, D = h["lut"].astype(np.float64), h["D"]
        wt = (lut[:, D - 1] if lut.ndim == 3 else np.broadcast_to(lut[D - 1], (h["n_rows"], h["Cw"]))).copy()
        if h["cnt"] is not None:
            wt = wt / np.maximum(h["cnt"][:, D - 1], 1)[:, None]
        T = wt[h["rows"]].sum(0)
        want = T[np.arange(h["W"]) % h["Cw"]] * h["S"][0].astype(np.float64)
        assert np.array_equal(got[unlisted, D - 1], want)


def forward_side(h):
    """The forward adjacency of the same pairs, in the keys tests/test_gpu_attr_rows.py's ``launch`` takes."""
    tot = h["S"].astype(np.float64).sum(0).astype(np.float32) if h["rft"] else None          # integer sums: exact in float32
    base = dict(S=h["S"], lut=h["lut"], cnt=h["cnt"], tot=tot, rows=h["rows"], n_cols=h["n_src"], D=h["D"], W=h["W"], Cw=h["Cw"],
                n_adj=h["n_rows"])
    if h["rowptr_t"] is None:
        return dict(base, rowptr=None, col=None, code=np.ascontiguousarray(h["code"].T))
    src = np.repeat(np.arange(h["n_src"]), np.diff(h["rowptr_t"].astype(np.int64)))
    order = np.argsort(h["row"], kind="stable")
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(h["row"], minlength=h["n_rows"]))]).astype(np.int64)
    return dict(base, rowptr=rowptr, col=src[order].astype(np.int32), code=h["code"][order])


@pytest.mark.parametrize("idx", [i for i in range(len(CASES)) if CASES[i][8] != "empty"])
def test_exact_cases_sum_to_the_row_side_and_to_the_forward(idx):
    """Summed over ALL sources: ``B.sum(0)`` is ``gnan_attr_rows``'s ``A.sum(0)`` on the same inputs, and ``B.sum((0, 1))`` the sum
    over the requested rows of ``gnan_spmm_fwd``'s rows — bit for bit, every sum being exact in float32.  (The forward takes the
    case without listed codes past the cover: its contract has none.)"""
    from gnan_amd import HopGraph
    from gnan_amd.aggregate import rho_aggregate
    h, truth, _, _ = inputs(idx, True)
    B = launch(h, cols=None)
    A = rows_side.launch(forward_side(h))
    assert torch.equal(bits(B.sum(0) + 0.0), bits(A.sum(0) + 0.0))  # (+ 0.0: a -0 and a +0 are the same exact value)
    h, truth, _, _ = inputs(idx, True, True)
    f = forward_side(h)
    t = lambda v: None if v is None else torch.from_numpy(np.ascontiguousarray(v)).to(DEV)      # noqa: E731
    cnt = t(h["cnt"]) if h["cnt"] is not None else torch.ones((h["n_rows"], h["D"]), dtype=torch.int32, device=DEV)
    if f["rowptr"] is None:
        g = HopGraph(n_rows=h["n_rows"], n_cols=h["n_src"], n_codes=h["D"], code=t(f["code"]), cnt=cnt)
    else:
        g = HopGraph.from_csr(t(f["rowptr"]), t(f["col"]), t(f["code"]), n_cols=h["n_src"], n_codes=h["D"], cnt=cnt)
    Y = rho_aggregate(g, t(h["S"]), t(h["lut"]), use_cnt=h["cnt"] is not None, with_rest=bool(h["rft"]), row_ids=t(h["rows"]),
                      s_total=t(f["tot"])).float().cpu()
    B = launch(h, cols=None)
    assert torch.equal(bits(B.sum((0, 1)) + 0.0), bits(Y.sum(0) + 0.0))


@pytest.mark.parametrize("idx", [0, 2, 9])
def test_the_checker_rejects_planted_errors(idx):
    """On a correct result: 2 gamma_k M added (away from the truth) to ONE element — in a one-pair column, in the rest column
    and in the longest column; two shells of a source swapped; a non-zero where the bound is 0."""
    h, truth, bound, mag = inputs(idx)
    got = launch(h).double().numpy()
    assert len(attr_ref.violations(got, truth, bound)) == 0
    cols = np.arange(h["n_src"]) if h["cols"] is None else h["cols"]
    short = int(np.nonzero(cols == 1)[0][0])                        # source 1: one pair (CSR cases)
    hub = int(np.argmax(mag.reshape(len(cols), -1).sum(1)))

    def largest(p, d=None):                                          # the element of source p (in shell d) with the widest bound
        sub = mag[p] if d is None else mag[p, d:d + 1]
        dd, w = np.unravel_index(np.argmax(sub), sub.shape)
        return (p, int(dd) if d is None else d, int(w))
    spots = [largest(short), largest(short, h["D"] - 1), largest(hub)]
    planted = 0
    for spot in spots:
        if bound[spot] == 0:
            continue
        bad = got.copy()
        bad[spot] += 2 * bound[spot] * (1.0 if got[spot] >= truth[spot] else -1.0)
        v = attr_ref.violations(bad, truth, bound)
        assert len(v) == 1 and tuple(v[0]) == spot, (spot, v)
        with pytest.raises(AssertionError, match="outside their bound"):
            attr_ref.check(bad, truth, bound)
        planted += 1
    assert planted >= 2 and bound[spots[-1]] > 0
    # two shells of the hub swapped
    d1, d2 = np.argsort(mag[hub].sum(1))[-2:]
    bad = got.copy()
    bad[hub, [d1, d2]] = bad[hub, [d2, d1]]
    v = attr_ref.violations(bad, truth, bound)
    assert len(v) and {tuple(x[:2]) for x in v} <= {(hub, d1), (hub, d2)}
    # a non-zero where nothing may be
    zp, zd, zw = np.argwhere(bound == 0)[0]
    bad = got.copy()
    bad[zp, zd, zw] = 1e-30
    v = attr_ref.violations(bad, truth, bound)
    assert len(v) == 1 and tuple(v[0]) == (zp, zd, zw)


@pytest.mark.parametrize("idx", [0, 2, 4, 8, 9])
def test_a_source_has_the_same_bits_alone_among_others_and_reversed(idx):
    h, truth, bound, mag = inputs(idx)
    n = h["n_src"]
    everything = launch(h, cols=None)
    assert torch.equal(bits(everything), bits(launch(h, cols=None)))
    rev = np.arange(n - 1, -1, -1).astype(np.int32)
    assert torch.equal(bits(launch(h, cols=rev)), bits(everything.flip(0)))
    for j in range(n):
        alone = launch(h, cols=np.array([j], dtype=np.int32))
        assert torch.equal(bits(alone[0]), bits(everything[j])), f"source {j}"
    if h["rows"] is not None and len(h["rows"]):                     # the SET of requested rows decides, not their order
        assert torch.equal(bits(launch(h, rows=h["rows"][::-1].copy(), cols=None)), bits(everything))
