"""``interpret.explain`` on the CPU route (``cpu_route.shell_attributions``: plain torch, no kernels) — no GPU needed.

Completeness against the REFERENCE's recorded output: the attributions of every golden model case sum to the fixture's
``out64`` by the rule of SURVEY.md 8c (``out32`` as the float32 reference, 1e-5 floor).  Every element of
``by_feature_distance`` against a dense float64 restatement that forms no hop code (tests/attr_ref.py)."""
import numpy as np
import pytest
import torch

import attr_ref
import gpu_util
from conftest import Golden
from helpers import assert_rule
from oracle import gnan_oracle as O
from test_cpu_route import MODEL_CASES

from gnan_amd import HopGraph, interpret


def kind_of(variant):
    return "standalone_tensor" if variant.startswith("standalone_tensor") else "post"


@pytest.mark.parametrize("name", MODEL_CASES)
def test_attributions_sum_to_the_reference_output_and_match_the_dense_restatement(name):
    g = Golden(name)
    v = g.meta["variant"]
    mod = gpu_util.build_module(g, "cpu")
    data = gpu_util.device_inputs(g, "cpu")
    node_ids = g.meta.get("node_ids") if v.endswith("gnan") else None
    ex = interpret.explain(mod, data.x if v == "models_nam" else data, node_ids=node_ids)
    F = data.x.shape[1]
    assert ex.by_feature_distance.shape[:2] == (len(node_ids) if node_ids is not None else data.x.shape[0], F)
    assert torch.equal(ex.output, ex.by_feature_distance.sum(dim=2).sum(dim=1))
    # --- completeness: the terms add up to what the reference computed
    if v == "models_nam":
        total = ex.output
    elif g.meta.get("readout_n_layers", 0) > 0 and v.endswith("graph"):
        assert ex.hidden.shape == (F,) and ex.readout_by_feature.shape == (F, g.meta["C"])
        total = ex.readout_by_feature.sum(0).view(-1, 1)
    elif v.endswith("graph"):
        assert ex.graph_by_feature_distance.shape == ex.by_feature_distance.shape[1:]
        total = ex.output.sum(0).view(-1, 1)
    else:
        total = ex.output
    assert tuple(total.shape) == g.out64.shape
    assert_rule(total, g.out64, g.out32, what=f"{name}: sum of the attributions")
    if v == "models_nam":
        fx = O.feature_mlps(data.x.double(), {k: torch.from_numpy(np.array(a)).double() for k, a in g.sd.items()})
        assert_rule(ex.by_feature_distance[:, :, 0], fx, what=f"{name}: per-feature terms")
        return
    # --- every element against the dense restatement (no hop codes)
    D = ex.hops.numel()
    assert ex.hops[-1] == float("inf") and ex.hops[:-1].tolist() == list(range(D - 1))
    params = {k: torch.from_numpy(np.array(a)) for k, a in g.sd.items()}
    truth = attr_ref.explain_restatement(kind_of(v), data.x, data.node_distances, data.normalization_matrix, params,
                                         g.meta["normalize_rho"], D, node_ids)
    assert truth.shape == ex.by_feature_distance.shape
    assert_rule(ex.by_feature_distance, truth, what=f"{name}: by_feature_distance")
    # nothing lies outside the distances listed: the restatement's shells cover every pair
    if g.meta.get("readout_n_layers", 0) == 0:
        whole = truth.sum(dim=(0, 1, 2)).view(-1, 1) if v.endswith("graph") else truth.sum(dim=(1, 2))
        assert_rule(whole, g.out64, g.out32, what=f"{name}: the restatement itself")
    if ex.graph_by_feature_distance is not None:
        assert_rule(ex.graph_by_feature_distance, truth.sum(0), what=f"{name}: graph_by_feature_distance")
    if ex.hidden is not None:
        assert_rule(ex.hidden, truth.sum(0).sum(1).view(-1), what=f"{name}: hidden")


def khop_case(K=1, n=60, f_raw=4, seed=0):
    rng = np.random.default_rng(seed)
    ei = np.stack([rng.integers(0, n - 5, 150), rng.integers(0, n - 5, 150)])
    ei = np.concatenate([ei, ei[::-1]], axis=1)
    nd, _ = O.pre_process_dense(ei, n)
    x = torch.cat([torch.from_numpy(rng.random((n, f_raw), dtype=np.float32)), torch.ones(n, 1)], 1)
    hops = O.hop_codes_from_dense(nd)
    ndK, normK = O.truncate_dense(nd, K)
    rowptr, col, code = O.csr_from_hops(hops, K)
    return x, ndK, normK, (torch.from_numpy(rowptr), torch.from_numpy(col), torch.from_numpy(code)), K + 2


def redraw(m, seed=1, scale=0.4):
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for _, p in m.named_parameters():
            p.copy_(torch.randn(p.shape, generator=gen) * scale)      # biases too: rho(0) != 0, the rest column is not zero


@pytest.mark.parametrize("K", [1, 2])
def test_khop_truncated_csr_with_a_biased_rho(K):
    from gnan_amd.models import GNAN, TensorGNAN
    x, ndK, normK, (rowptr, col, code), D = khop_case(K)
    g = HopGraph.from_csr(rowptr, col, code, n_cols=x.shape[0], n_codes=D)
    for mod, rows in ((GNAN(x.shape[1], 2, num_layers=3, hidden_channels=16), [1, 5, 7, 5]),
                      (TensorGNAN(x.shape[1], 3, 2, hidden_channels=8, rho_per_feature=True), None)):
        redraw(mod)
        mod.eval()
        data = gpu_util.Bag(x=x, edge_index=None, gnan_graph=g)
        ex = interpret.explain(mod, data, rows=rows)
        params = {k: v.detach() for k, v in mod.state_dict().items()}
        truth = attr_ref.explain_restatement("post", x, ndK, normK, params, True, D, rows)
        assert float(truth[:, :, D - 1].abs().max()) > 1e-3 * float(truth.abs().max())      # the rest column carries weight
        assert_rule(ex.by_feature_distance, truth, what="K-hop CSR by_feature_distance")
        y = mod(data, rows) if rows is not None else mod(data)
        assert_rule(ex.output, y.detach().double(), what="K-hop CSR output against forward", floor=2e-5)


def test_explain_wants_eval_mode_and_one_device():
    from gnan_amd import _lib
    from gnan_amd.models import TensorGNAN
    m = TensorGNAN(3, 2, 2, hidden_channels=4)
    x, ndK, normK, _, _ = khop_case(1, n=12, f_raw=2)
    data = gpu_util.Bag(x=x, node_distances=ndK, normalization_matrix=normK)
    with pytest.raises(_lib.GnanHipError, match="eval"):
        interpret.explain(m.train(), data)
    with pytest.raises(_lib.GnanHipError, match="ONE device"):
        interpret.explain(m.eval(), gpu_util.Bag(x=torch.empty(12, 3, device="meta")))
