"""``gnan_attr_rows`` (csrc/attr_rows.hip) through the C ABI, element by element against tests/attr_ref.py: both adjacency
layouts, both rowptr widths, row_ids absent / permuted / repeating, counts or none, shared and per-row tables, one weight channel
or one per output channel, with and without s_total, listed codes past the cover — at the operand widths, shell counts and row
lengths where the kernel changes path (``chunk`` comes from ``gnan_attr_rows_describe``).  Exact integer cases, planted errors
the checker must reject, bit reproducibility, and the shell sum against ``gnan_spmm_fwd``."""
import functools

import numpy as np
import pytest
import torch

import attr_ref
import rowwise
from gnan_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"


def chunk_pairs():
    info = _lib.AttrInfo()
    a = _lib.AttrArgs(n_rows=1, n_cols=1, W=1, s_stride=1, D=2, Cw=1, a_stride=2)
    assert _lib.lib().gnan_attr_rows_describe(a, info) == 0
    return info.chunk_pairs


# layout, rowptr dtype, W, D, Cw, cnt, per-row lut, s_total, row_ids ("none" / "perm" / "repeat"), n_cols, top listed code
CASES = [
    ("csr", np.int64, 130, 17, 1, True, False, True, "none", 311, 255),      # three column tiles, the last ragged; codes 254 / 255 clipped
    ("csr", np.int32, 3, 2, 3, False, True, False, "repeat", 257, 1),        # 16 pair slots per wave; D = 2; per-row table
    ("csr", np.int32, 63, 64, 1, False, False, True, "perm", 300, 62),       # one pass of exactly 64 shells
    ("csr", np.int64, 64, 65, 4, True, False, False, "none", 300, 64),       # one full tile; two passes, the second of one shell
    ("csr", np.int32, 1, 256, 1, True, True, True, "perm", 301, 254),        # 64 slots; four passes
    ("csr", np.int32, 8, 17, 8, True, False, True, "repeat", 300, 254),      # Cw = C; codes past the cover beside s_total
    ("dense", None, 65, 65, 5, True, False, False, "none", 301, 64),         # width no multiple of 4; two tiles, one column in the second
    ("dense", None, 8, 256, 1, False, True, False, "repeat", 203, 255),      # dense, per-row table, repeating row_ids
    ("dense", None, 3, 5, 1, True, False, True, "perm", None, 4),            # dense rows of chunk + 3 pairs: partials in the workspace
]


def row_lengths():
    c = chunk_pairs()
    return [0, 1, c - 1, c, c + 1, 2 * c + 3, 5]


@functools.lru_cache(maxsize=None)
def inputs(idx, exact=False):
    """Host inputs of a case (numpy) and the float64 reference, computed once and shared."""
    layout, ptr_t, W, D, Cw, use_cnt, per_row, with_total, ids, n_cols, top = CASES[idx]
    rng = np.random.default_rng(100 + idx)
    if n_cols is None:
        n_cols = chunk_pairs() + 3
    if layout == "csr":
        lens = np.array(row_lengths())
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
        lut = (2.0 ** rng.integers(-3, 4, (n_adj, D, Cw) if per_row else (D, Cw)) * rng.choice([-1.0, 1.0])).astype(np.float32)
        cnt = (2 ** rng.integers(0, 4, (n_adj, D))).astype(np.int32) if use_cnt else None
    else:
        S = rng.standard_normal((n_cols, W)).astype(np.float32)
        lut = rng.standard_normal((n_adj, D, Cw) if per_row else (D, Cw)).astype(np.float32)
        cnt = rng.integers(0, 40, (n_adj, D)).astype(np.int32) if use_cnt else None            # 0: the max(cnt, 1) guard
    tot = S.astype(np.float64).sum(0).astype(np.float32) if with_total else None             # (exact: integer sums, exact in fp32)
    rows = {"none": None, "perm": rng.permutation(n_adj).astype(np.int32),
            "repeat": np.array([n_adj - 1, 0, 2, n_adj - 1, 1, 2], dtype=np.int32)}[ids]
    host = dict(rowptr=rowptr, col=col, code=code, S=S, lut=lut, cnt=cnt, tot=tot, rows=rows, n_cols=n_cols, D=D, W=W, Cw=Cw,
                n_adj=n_adj)
    truth, bound, mag = attr_ref.reference(code, S, lut, rowptr, col, cnt, tot, rows)
    return host, truth, bound, mag


def launch(h, rows="same", s_pad=0, item_ptr=True):
    """One call of gnan_attr_rows on the host inputs ``h``; ``rows``: another row_ids array (or None) than the case's."""
    t = lambda v: None if v is None else torch.from_numpy(np.ascontiguousarray(v)).to(DEV)      # noqa: E731
    rows = h["rows"] if isinstance(rows, str) else rows
    S = t(h["S"])
    if s_pad:                                                        # an operand with a row stride
        S = torch.cat([S, torch.full((S.shape[0], s_pad), float("nan"), device=DEV)], 1)[:, : h["W"]]
    dev = dict(rowptr=t(h["rowptr"]), col=t(h["col"]), code=t(h["code"]), S=S, lut=t(h["lut"]), cnt=t(h["cnt"]), tot=t(h["tot"]),
               rows=t(rows))
    R = h["n_adj"] if rows is None else len(rows)
    D, W = h["D"], h["W"]
    A = torch.full((R, D, W), float("nan"), device=DEV)
    a = _lib.AttrArgs(n_rows=R, n_cols=h["n_cols"], code=_lib.ptr(dev["code"]), row_ids=_lib.ptr(dev["rows"]), S=_lib.ptr(S), W=W,
                      s_stride=S.stride(0), lut=_lib.ptr(dev["lut"]), lut_row_stride=D * h["Cw"] if h["lut"].ndim == 3 else 0,
                      D=D, Cw=h["Cw"], s_total=_lib.ptr(dev["tot"]), A=_lib.ptr(A), a_stride=D * W)
    if h["cnt"] is not None:
        a.cnt, a.cnt_stride = _lib.ptr(dev["cnt"]), D
    if h["rowptr"] is not None:
        a.rowptr, a.rowptr_is64, a.col = _lib.ptr(dev["rowptr"]), int(h["rowptr"].dtype == np.int64), _lib.ptr(dev["col"])
        a.nnz = len(h["col"])
        lens = np.diff(h["rowptr"].astype(np.int64))
        lens = lens if rows is None else lens[np.asarray(rows)]
        a.max_row_pairs = int(lens.max())
        if item_ptr:                                                 # the per-row chunk list; without: the longest row's for all
            c = chunk_pairs()
            ptr = np.concatenate([[0], np.cumsum(np.maximum(1, -(-lens // c)))]).astype(np.int32)
            dev["item_ptr"] = t(ptr)
            a.item_ptr, a.n_items = _lib.ptr(dev["item_ptr"]), int(ptr[-1])
    need = _lib.lib().gnan_attr_rows_workspace_bytes(a)
    ws = torch.full(((need + 3) // 4,), float("nan"), device=DEV) if need else None
    a.workspace, a.workspace_bytes = _lib.ptr(ws), need
    _lib.check(_lib.lib().gnan_attr_rows(a, torch.cuda.current_stream().cuda_stream), "gnan_attr_rows")
    torch.cuda.synchronize()
    return A.cpu()


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("idx", range(len(CASES)))
def test_every_element_within_its_derived_bound(idx):
    h, truth, bound, mag = inputs(idx)
    got = launch(h)
    attr_ref.check(got, truth, bound, f"case {idx} {CASES[idx][:5]}")
    again = launch(h, s_pad=3)                                       # a second launch, the operand behind a row stride: equal bits
    assert torch.equal(bits(got), bits(again))
    if h["rowptr"] is not None:                                      # the uniform chunk list: equal bits again
        assert torch.equal(bits(got), bits(launch(h, item_ptr=False)))
    zero = bound == 0
    assert zero.any() and (got.numpy()[zero] == 0).all()            # an all-zero shell is exactly zero


@pytest.mark.parametrize("idx", range(len(CASES)))
def test_exact_integer_cases_match_bit_for_bit(idx):
    h, truth, bound, mag = inputs(idx, True)
    got = launch(h).double().numpy()
    assert np.array_equal(got, truth), f"case {idx}: {int((got != truth).sum())} elements differ from the exact result"
    assert (mag > 0).any() and (got[mag == 0] == 0).all()


@pytest.mark.parametrize("idx", [0, 4, 8])
def test_the_checker_rejects_a_planted_error(idx):
    """2 gamma_k M added (away from the truth) to ONE element of a correct result — among them one in a one-pair row beside the
    row of 2 chunk + 3 pairs, and one in the rest column."""
    h, truth, bound, mag = inputs(idx)
    got = launch(h).double().numpy()
    assert len(attr_ref.violations(got, truth, bound)) == 0
    rows = np.arange(h["n_adj"]) if h["rows"] is None else h["rows"]
    short = int(np.nonzero(rows == 1)[0][0])                        # adjacency row 1: one pair (CSR cases)
    hub = int(np.argmax(mag.reshape(len(rows), -1).sum(1)))          # the row with the most weight: the longest

    def largest(q, d=None):                                          # the element of row q (in shell d) with the widest bound
        sub = mag[q] if d is None else mag[q, d:d + 1]
        dd, w = np.unravel_index(np.argmax(sub), sub.shape)
        return (q, int(dd) if d is None else d, int(w))
    spots = [largest(short), largest(short, h["D"] - 1), largest(hub)]
    assert hub != short
    for spot in spots:
        if bound[spot] == 0:                                         # (a rest column without pairs and without s_total)
            continue
        bad = got.copy()
        bad[spot] += 2 * bound[spot] * (1.0 if got[spot] >= truth[spot] else -1.0)
        v = attr_ref.violations(bad, truth, bound)
        assert len(v) == 1 and tuple(v[0]) == spot, (spot, v)
        with pytest.raises(AssertionError, match="outside their bound"):
            attr_ref.check(bad, truth, bound)
    assert bound[spots[0]] > 0 and bound[spots[-1]] > 0


@pytest.mark.parametrize("idx", [0, 2, 7, 8])
def test_a_row_has_the_same_bits_alone_among_others_and_reversed(idx):
    h, truth, bound, mag = inputs(idx)
    n = h["n_adj"]
    everything = launch(h, rows=None)
    assert torch.equal(bits(everything), bits(launch(h, rows=None)))
    rev = np.arange(n - 1, -1, -1).astype(np.int32)
    assert torch.equal(bits(launch(h, rows=rev)), bits(everything.flip(0)))
    for i in range(n):
        alone = launch(h, rows=np.array([i], dtype=np.int32))
        assert torch.equal(bits(alone[0]), bits(everything[i])), f"row {i}"


def test_shell_sum_agrees_with_spmm_fwd():
    """sum_d A against ``gnan_spmm_fwd`` (``rho_aggregate``) on the same graph, operand, table, counts and s_total: within the sum
    of the two derived bounds (attr_ref's summed over the shells, rowwise's for the forward)."""
    from gnan_amd import HopGraph
    from gnan_amd.aggregate import rho_aggregate
    from gnan_amd.attribution import shell_attributions
    from gnan_amd.functional import column_sums
    rng = np.random.default_rng(7)
    c = chunk_pairs()
    n_cols, D, W = 300, 5, 8
    lens = np.array([0, 1, 7, c + 1, 40, 600])
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    col = rng.integers(0, n_cols, int(rowptr[-1])).astype(np.int32)
    code = rng.integers(0, D - 1, int(rowptr[-1])).astype(np.uint8)
    g = HopGraph.from_csr(torch.from_numpy(rowptr).to(DEV), torch.from_numpy(col).to(DEV), torch.from_numpy(code).to(DEV),
                          n_cols=n_cols, n_codes=D)
    S = torch.from_numpy(rng.standard_normal((n_cols, W)).astype(np.float32)).to(DEV)
    lut = torch.from_numpy(rng.standard_normal((D, 1)).astype(np.float32)).to(DEV)
    tot = column_sums(S)
    rows = torch.tensor([5, 0, 3, 1, 2, 4, 3], dtype=torch.int32, device=DEV)
    A = shell_attributions(g, S, lut, True, rows, tot).cpu()
    Y = rho_aggregate(g, S, lut, use_cnt=True, row_ids=rows, s_total=tot).cpu()
    truth, bound, _ = attr_ref.reference(code, S, lut, rowptr, col, g.cnt, tot, rows)
    attr_ref.check(A, truth, bound, "shell_attributions")
    t_fwd, b_fwd = rowwise.reference(rowptr, col, code, S.cpu(), lut.cpu(), g.cnt.cpu(), tot.cpu(), rows=rows.cpu())
    assert np.abs(truth.sum(1) - t_fwd).max() <= 1e-12 * np.abs(t_fwd).max()                  # one function, two restatements
    diff = np.abs(A.double().numpy().sum(1) - Y.double().numpy())
    assert (diff <= bound.sum(1) + b_fwd).all(), float((diff / (bound.sum(1) + b_fwd + 1e-300)).max())
