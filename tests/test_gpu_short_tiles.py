"""Short-row tiles (aggregate.SHORT_ROW_TILES, gnan_spmm_args.short_*): the wide forward over a degree-sorted copy with the rows
of at most SHORT_ROW_LMAX pairs taken in tiles gives the same bits as the plain row walk — self-only rows, rows without a self
pair, empty rows, a run of every length up to the longest tiled one, hub rows behind them.  The launch query says which shapes
take the tiles at all: fp32 rows of W = 64 and 128 do; W = 32 and bf16 rows are declined and compare the row walk with itself here
(tests/test_gpu_wide_rows.py holds the per-row bounds and the list of declined shapes)."""
import numpy as np
import pytest
import torch

from test_gpu_kernels import _graph

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _short_csr(n, rng):
    """Rows of 0 .. 9 pairs and a few hubs; most rows with 1 .. 4 pairs list themselves first (code 0), some do not."""
    deg = rng.choice([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 30], size=n, p=[.05, .35, .12, .1, .08, .06, .05, .05, .05, .05, .04])
    deg[[7, 1234, n - 1]] = [600, 2000, 513]
    rowptr = np.zeros(n + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(deg)
    col = rng.integers(0, n, int(rowptr[-1])).astype(np.int32)
    code = rng.integers(1, 3, int(rowptr[-1])).astype(np.uint8)
    for i in np.nonzero((deg > 0) & (deg <= 4) & (rng.random(n) < 0.8))[0]:
        col[rowptr[i]], code[rowptr[i]] = i, 0
    return rowptr, col, code


@pytest.mark.parametrize("lmax", [4, 8])
@pytest.mark.parametrize("dtype,W", [(torch.float32, 64), (torch.float32, 32), (torch.float32, 128), (torch.bfloat16, 64)])
@pytest.mark.parametrize("with_rest", [True, False])
@pytest.mark.parametrize("reduce_cr", [0, 1])
def test_short_tiles_give_the_row_walks_bits(lmax, dtype, W, with_rest, reduce_cr, monkeypatch):
    from gnan_amd import aggregate
    monkeypatch.setattr(aggregate, "DEGREE_SORTED_COPY_MIN_ROWS", 1)      # the test graph is small: walk its degree-sorted copy
    monkeypatch.setattr(aggregate, "SHORT_ROW_LMAX", lmax)
    rng = np.random.default_rng(W + 7 * lmax + int(with_rest) + 3 * reduce_cr)
    n = 20_000
    rowptr, col, code = _short_csr(n, rng)
    g = _graph(rowptr, col, code, n, 4)
    S = torch.from_numpy(rng.standard_normal((n, W)).astype(np.float32)).to(DEV).to(dtype)
    lut = torch.from_numpy(rng.standard_normal((4, 1)).astype(np.float32)).to(DEV)
    out, info = {}, {}
    for tiles in (True, False):
        monkeypatch.setattr(aggregate, "SHORT_ROW_TILES", tiles)
        d = []
        out[tiles] = aggregate.spmm_launch(g, S, lut, True, with_rest, reduce_cr=reduce_cr, describe=d)
        info[tiles] = d[0]
    torch.cuda.synchronize()
    if dtype == torch.float32 and W in (64, 128):
        assert info[True]["n_tiles"] > 0 and info[True]["row_q0"] > 0
    else:
        assert info[True]["n_tiles"] == 0
    assert info[False]["n_tiles"] == 0
    copy = g.degree_sorted_copy()[0]
    runs = copy.short_row_runs(lmax)
    assert all(runs.rows[L + 1] > runs.rows[L] for L in range(lmax + 1))        # every run is there
    assert torch.equal(out[True], out[False])
    assert torch.isfinite(out[True]).all()
