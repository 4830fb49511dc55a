"""``interpret.explain`` on the HIP path (``gnan_attr_rows``): every module class on a ~30-node dense graph and a ~200-node K-hop
CSR with a biased rho (a non-zero rest column), element by element against the dense float64 restatement of tests/attr_ref.py,
against the module's own forward, and against the CPU route on a CPU twin of the module."""
import functools

import numpy as np
import pytest
import torch

import attr_ref
import gpu_util
from helpers import TWO_FLOORS, assert_rule
from oracle import gnan_oracle as O

from gnan_amd import GNAN as standalone
from gnan_amd import HopGraph, _lib, interpret, models

pytestmark = pytest.mark.gpu
DEV = "cuda"
F_RAW = 4

# name: (constructor, kind of the restatement, node_ids)
MODULES = {
    "standalone_tensor_node_pre_rho": (lambda F: standalone.TensorGNAN(F, 3, 3, hidden_channels=8), "standalone_tensor", None),
    "standalone_tensor_node_no_norm": (lambda F: standalone.TensorGNAN(F, 2, 2, hidden_channels=8, normalize_rho=False),
                                       "standalone_tensor", None),
    "standalone_tensor_graph_pre_rho": (lambda F: standalone.TensorGNAN(F, 2, 3, hidden_channels=8, is_graph_task=True),
                                        "standalone_tensor", None),
    "models_tensor_node": (lambda F: models.TensorGNAN(F, 3, 3, hidden_channels=8), "post", None),
    "models_tensor_node_rho_per_feature": (lambda F: models.TensorGNAN(F, 3, 2, hidden_channels=8, rho_per_feature=True), "post", None),
    "models_tensor_graph": (lambda F: models.TensorGNAN(F, 2, 3, hidden_channels=8, is_graph_task=True, readout_n_layers=0), "post", None),
    "models_tensor_graph_readout": (lambda F: models.TensorGNAN(F, 3, 3, hidden_channels=8, is_graph_task=True, readout_n_layers=2),
                                    "post", None),
    "models_gnan_node_ids": (lambda F: models.GNAN(F, 2, num_layers=3, hidden_channels=8), "post", [3, 0, 11, 3]),
    "standalone_gnan_node_ids": (lambda F: standalone.GNAN(F, 3, 2, hidden_channels=8, rho_per_feature=True), "post", [7, 2]),
}


@functools.lru_cache(maxsize=None)
def graph_case(which):
    """``(x, nd, norm, csr or None, D)`` on the host: "dense" — ~30 nodes as the reference's dense inputs; "csr" — ~200 nodes,
    K = 2 truncated (the restatement's inputs are ``O.truncate_dense``'s)."""
    n, e, K = (30, 45, None) if which == "dense" else (200, 260, 2)
    rng = np.random.default_rng(n)
    ei = np.stack([rng.integers(0, n - 3, e), rng.integers(0, n - 3, e)])
    ei = np.concatenate([ei, ei[::-1]], axis=1)
    nd, norm = O.pre_process_dense(ei, n)
    x = torch.cat([torch.from_numpy(rng.random((n, F_RAW), dtype=np.float32)), torch.ones(n, 1)], 1)
    if K is None:
        return x, nd, norm, None, int(O.hop_codes_from_dense(nd).max()) + 2
    hops = O.hop_codes_from_dense(nd)
    ndK, normK = O.truncate_dense(nd, K)
    rowptr, col, code = O.csr_from_hops(hops, K)
    return x, ndK, normK, (torch.from_numpy(rowptr), torch.from_numpy(col), torch.from_numpy(code)), K + 2


def build(name, dev):
    m = MODULES[name][0](F_RAW + 1)
    gen = torch.Generator().manual_seed(sum(map(ord, name)))
    with torch.no_grad():
        for _, p in m.named_parameters():
            p.copy_(torch.randn(p.shape, generator=gen) * 0.4)       # biases too: rho(0) != 0 where rho has a bias
    return m.to(dev).eval()


def inputs_on(which, dev):
    x, nd, norm, csr, D = graph_case(which)
    if csr is None:
        return gpu_util.Bag(x=x.to(dev), edge_index=None, node_distances=nd.to(dev), normalization_matrix=norm.to(dev))
    g = HopGraph.from_csr(csr[0].to(dev), csr[1].to(dev), csr[2].to(dev), n_cols=x.shape[0], n_codes=D)
    return gpu_util.Bag(x=x.to(dev), edge_index=None, gnan_graph=g)


def forward(m, data, node_ids):
    with torch.no_grad():
        return m(data, node_ids) if node_ids is not None else m(data)


@pytest.mark.parametrize("which", ["dense", "csr"])
@pytest.mark.parametrize("name", list(MODULES))
def test_explain_matches_restatement_forward_and_cpu_twin(name, which):
    _, kind, node_ids = MODULES[name]
    x, nd, norm, csr, D = graph_case(which)
    m = build(name, DEV)
    data = inputs_on(which, DEV)
    ex = interpret.explain(m, data, node_ids=node_ids)
    R = x.shape[0] if node_ids is None else len(node_ids)
    C = ex.by_feature_distance.shape[-1]
    assert ex.by_feature_distance.is_cuda and tuple(ex.by_feature_distance.shape) == (R, F_RAW + 1, D, C)
    assert ex.hops.tolist() == [float(d) for d in range(D - 1)] + [float("inf")]
    assert ex.rows.tolist() == (list(range(R)) if node_ids is None else node_ids)
    params = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    truth = attr_ref.explain_restatement(kind, x, nd, norm, params, bool(m.normalize_rho), D, node_ids)
    assert_rule(ex.by_feature_distance, truth, what=f"{name}/{which}: by_feature_distance")
    if which == "csr" and any(k.startswith("rho.") and k.endswith("bias") for k in params):
        assert float(truth[:, :, D - 1].abs().max()) > 0            # a biased rho: rho(0) != 0, the rest column carries weight
    assert torch.equal(ex.output, ex.by_feature_distance.sum(dim=2).sum(dim=1))
    # the module's own forward: two routes of the build
    y = forward(m, data, node_ids).double().cpu()
    graph_task = bool(getattr(m, "is_graph_task", False))
    with_readout = graph_task and getattr(m, "readout_n_layers", 0) > 0 and isinstance(m, models.TensorGNAN)
    if with_readout:
        assert_rule(ex.hidden, truth.sum(0).sum(1).view(-1), what=f"{name}/{which}: hidden")
        assert tuple(ex.readout_by_feature.shape) == (F_RAW + 1, m.out_channels)
        assert_rule(ex.readout_by_feature.sum(0).view(-1, 1), y, what=f"{name}/{which}: read-out sum against forward", floor=TWO_FLOORS)
    elif graph_task:
        assert_rule(ex.output.sum(0).view(-1, 1), y, what=f"{name}/{which}: output against forward", floor=TWO_FLOORS)
    else:
        assert_rule(ex.output, y, what=f"{name}/{which}: output against forward", floor=TWO_FLOORS)
    if graph_task:
        assert_rule(ex.graph_by_feature_distance, truth.sum(0), what=f"{name}/{which}: graph_by_feature_distance")
    else:
        assert ex.graph_by_feature_distance is None and ex.hidden is None and ex.readout_by_feature is None
    # the CPU route on a CPU twin
    twin = build(name, "cpu")
    ex_cpu = interpret.explain(twin, inputs_on(which, "cpu"), node_ids=node_ids)
    assert not ex_cpu.by_feature_distance.is_cuda
    assert_rule(ex.by_feature_distance, ex_cpu.by_feature_distance.double(), what=f"{name}/{which}: CPU twin", floor=TWO_FLOORS)
    if with_readout:
        assert_rule(ex.readout_by_feature, ex_cpu.readout_by_feature.double(), what=f"{name}/{which}: CPU twin read-out", floor=TWO_FLOORS)


def test_rows_in_any_order_give_the_rows_of_the_full_explanation():
    m = build("models_tensor_node", DEV)
    data = inputs_on("csr", DEV)
    full = interpret.explain(m, data)
    some = interpret.explain(m, data, rows=[190, 3, 3, 0])
    assert torch.equal(some.by_feature_distance, full.by_feature_distance[[190, 3, 3, 0]])


def test_cpu_tensors_on_a_cuda_module_raise_and_the_byte_budget_advises_batches(monkeypatch):
    from gnan_amd import attribution
    m = build("models_tensor_node", DEV)
    with pytest.raises(_lib.GnanHipError, match="ONE device"):
        interpret.explain(m, inputs_on("dense", "cpu"))
    data = inputs_on("dense", DEV)
    g = m.hop_graph(data)
    S = torch.rand(g.n_cols, 4, device=DEV)
    with pytest.raises(_lib.GnanHipError, match="CPU tensor"):
        attribution.shell_attributions(g, S.cpu(), torch.rand(g.n_codes, 1, device=DEV), True)
    monkeypatch.setattr(attribution, "ATTR_MAX_BYTES", 4 * g.n_rows * g.n_codes * 4 - 1)
    with pytest.raises(_lib.GnanHipError, match=r"\[30, \d+, 4\] float32 takes \d+ bytes.*pass `rows` in batches"):
        attribution.shell_attributions(g, S, torch.rand(g.n_codes, 1, device=DEV), True)
    part = attribution.shell_attributions(g, S, torch.rand(g.n_codes, 1, device=DEV), True, rows=torch.arange(15, device=DEV))
    assert tuple(part.shape) == (15, g.n_codes, 4)
