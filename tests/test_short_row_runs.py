"""HopGraph.short_row_runs (the run boundaries behind gnan_spmm_args.short_*) against a plain restatement, on the CPU."""
import numpy as np
import pytest
import torch


def _copy(deg, idx_dtype):
    from gnan_amd import HopGraph
    rowptr = np.zeros(len(deg) + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(deg)
    rng = np.random.default_rng(len(deg))
    col = rng.integers(0, len(deg), int(rowptr[-1])).astype(np.int32)
    code = rng.integers(0, 3, int(rowptr[-1])).astype(np.uint8)
    g = HopGraph.from_csr(torch.from_numpy(rowptr).to(idx_dtype), torch.from_numpy(col), torch.from_numpy(code),
                          n_cols=len(deg), n_codes=4)
    return g.degree_sorted_copy()[0]


@pytest.mark.parametrize("idx_dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("lmax", [1, 4, 8])
@pytest.mark.parametrize("deg", [[3, 0, 1, 1, 5, 2, 9, 1, 0, 4, 700, 2], [1, 1, 1], [6, 7, 9], [0, 0, 2, 5]])
def test_short_row_runs_match_a_restatement(deg, lmax, idx_dtype):
    copy = _copy(np.array(deg), idx_dtype)
    runs = copy.short_row_runs(lmax)
    d = sorted(deg)                                     # the copy's rows, shortest first
    rows = [sum(1 for x in d if x < L) for L in range(lmax + 2)]
    pairs = [sum(d[: rows[L]]) for L in range(lmax + 1)]
    assert (runs.lmax, runs.rows, runs.pairs) == (lmax, rows, pairs)
    rp = copy.rowptr.tolist()
    for L in range(lmax + 1):                           # what the kernel relies on: row q of run L starts at pairs[L] + (q - rows[L]) L
        for q in range(rows[L], rows[L + 1]):
            assert rp[q] == runs.pairs[L] + (q - rows[L]) * L and rp[q + 1] - rp[q] == L
    assert copy.short_row_runs(lmax) is runs            # cached
