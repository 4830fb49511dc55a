"""``interpret.importance`` on the CPU route (``cpu_route.reduced_attributions``: plain torch, no kernels) — no GPU needed: the nine
module classes of tests/test_gpu_explain.py on a dense graph and a K-hop CSR, a NAM, row subsets with groups, the refusals, and
``cpu_route.reduced_attributions`` itself against the float64 reference of tests/attr_reduce_ref.py."""
import types

import numpy as np
import pytest
import torch

import attr_reduce_ref as ref
import importance_cases as cases
from test_gpu_explain import MODULES

from gnan_amd import cpu_route


@pytest.mark.parametrize("which", ["dense", "csr"])
@pytest.mark.parametrize("name", list(MODULES))
def test_importance_matches_restatement_and_explain(name, which):
    cases.check_module(name, which, "cpu", 1e-12)


def test_rows_subset_with_groups():
    cases.check_rows_subset("cpu", 1e-12)


def test_nam_has_one_distance():
    cases.check_nam("cpu", 1e-12)


def test_refusals():
    cases.check_refusals("cpu")


@pytest.mark.parametrize("dense", [False, True])
def test_reduced_attributions_is_the_definition(dense, monkeypatch):
    """The plain-torch twin against the float64 truth, in row batches of three (the batch must not show)."""
    rng = np.random.default_rng(3)
    n, D, W, cw = 9, 4, 6, 2
    S = torch.from_numpy(rng.standard_normal((n, W)).astype(np.float32))
    wt = torch.from_numpy(rng.standard_normal((n, D, cw)).astype(np.float32))
    if dense:
        code = torch.from_numpy(rng.integers(0, D + 2, (n, n)).astype(np.uint8))
        g = types.SimpleNamespace(n_codes=D, n_rows=n, n_cols=n, is_dense=True, code=code)
        rowptr = col = tot = None
    else:
        lens = rng.integers(0, 6, n)
        rowptr = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64))
        col = torch.from_numpy(rng.integers(0, n, int(rowptr[-1])).astype(np.int32))
        code = torch.from_numpy(rng.integers(0, D + 1, int(rowptr[-1])).astype(np.uint8))
        g = types.SimpleNamespace(n_codes=D, n_rows=n, n_cols=n, is_dense=False, rowptr=rowptr, col=col, code=code)
        tot = S.sum(0)
    rows = torch.tensor([8, 0, 3, 3, 5, 1, 7, 2])
    gp = torch.tensor([0, 2, 2, 7, 8])
    monkeypatch.setattr(cpu_route, "REDUCE_BATCH_BYTES", 3 * D * W * 8)
    M = cpu_route.reduced_attributions(g, S, wt, rows, gp)
    assert M.dtype == torch.float64 and tuple(M.shape) == (4, 3, D + 1, W) and bool((M[1] == 0).all())
    truth, _ = ref.reference(code, S, wt, rowptr, col, None, tot, rows, gp.numpy())
    scale = np.abs(truth).max()
    assert np.abs(M.numpy() - truth).max() <= 1e-5 * scale           # float32 terms against the float64 truth
    monkeypatch.setattr(cpu_route, "REDUCE_BATCH_BYTES", 1 << 26)
    assert torch.allclose(cpu_route.reduced_attributions(g, S, wt, rows, gp), M, rtol=1e-13, atol=0)
    assert torch.equal(cpu_route.reduced_attributions(g, S, wt, rows[2:7])[0], cpu_route.reduced_attributions(g, S, wt, rows, gp)[2])
    with pytest.raises(ValueError, match="group_ptr must rise"):
        cpu_route.reduced_attributions(g, S, wt, rows, torch.tensor([0, 5, 4, 8]))
