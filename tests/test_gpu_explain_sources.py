"""``interpret.explain_sources`` on the HIP path (``gnan_attr_cols``): every module class on a ~30-node dense graph and a ~200-node
K-hop CSR with a biased rho (a non-zero rest column), element by element against the dense float64 restatement by source node of
tests/attr_cols_ref.py, against the module's own forward, and against the CPU route on a CPU twin of the module."""
import pytest
import torch

import attr_cols_ref
from helpers import TWO_FLOORS, assert_rule
from test_gpu_explain import F_RAW, MODULES, build, forward, graph_case, inputs_on

from gnan_amd import _lib, interpret, models

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("which", ["dense", "csr"])
@pytest.mark.parametrize("name", list(MODULES))
def test_explain_sources_matches_restatement_forward_and_cpu_twin(name, which):
    _, kind, node_ids = MODULES[name]
    x, nd, norm, csr, D = graph_case(which)
    m = build(name, DEV)
    data = inputs_on(which, DEV)
    sx = interpret.explain_sources(m, data, node_ids=node_ids)
    n = x.shape[0]
    C = sx.by_feature_distance.shape[-1]
    assert sx.by_feature_distance.is_cuda and tuple(sx.by_feature_distance.shape) == (n, F_RAW + 1, D, C)
    assert sx.hops.tolist() == [float(d) for d in range(D - 1)] + [float("inf")]
    assert sx.sources.tolist() == list(range(n)) and sx.rows.tolist() == (list(range(n)) if node_ids is None else node_ids)
    params = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    truth = attr_cols_ref.explain_sources_restatement(kind, x, nd, norm, params, bool(m.normalize_rho), D, node_ids)
    assert_rule(sx.by_feature_distance, truth, what=f"{name}/{which}: by_feature_distance")
    if which == "csr" and any(k.startswith("rho.") and k.endswith("bias") for k in params):
        assert float(truth[:, :, D - 1].abs().max()) > 0            # a biased rho: rho(0) != 0, the rest column carries weight
    assert torch.equal(sx.by_node, sx.by_feature_distance.sum(dim=2).sum(dim=1))
    # the module's own forward: two routes of the build
    y = forward(m, data, node_ids).double().cpu()
    graph_task = bool(getattr(m, "is_graph_task", False))
    with_readout = graph_task and getattr(m, "readout_n_layers", 0) > 0 and isinstance(m, models.TensorGNAN)
    if with_readout:
        ex = interpret.explain(m, data)
        assert tuple(sx.hidden_by_node.shape) == (n, F_RAW + 1)
        assert_rule(sx.hidden_by_node, truth.sum(2).view(n, -1), what=f"{name}/{which}: hidden_by_node")
        assert_rule(sx.hidden_by_node.sum(0), ex.hidden.double().cpu(), what=f"{name}/{which}: hidden_by_node against explain", floor=TWO_FLOORS)
    else:
        assert sx.hidden_by_node is None
        total = sx.by_node.sum(0)
        assert_rule(total.view(-1, 1) if graph_task else total, y if graph_task else y.sum(0), what=f"{name}/{which}: by_node against forward",
                    floor=TWO_FLOORS)
    # the CPU route on a CPU twin
    twin = build(name, "cpu")
    sx_cpu = interpret.explain_sources(twin, inputs_on(which, "cpu"), node_ids=node_ids)
    assert not sx_cpu.by_feature_distance.is_cuda
    assert_rule(sx.by_feature_distance, sx_cpu.by_feature_distance.double(), what=f"{name}/{which}: CPU twin", floor=TWO_FLOORS)


def test_sources_in_any_order_give_the_rows_of_the_full_explanation():
    m = build("models_tensor_node", DEV)
    data = inputs_on("csr", DEV)
    full = interpret.explain_sources(m, data)
    some = interpret.explain_sources(m, data, sources=[190, 3, 3, 0])
    assert some.sources.tolist() == [190, 3, 3, 0]
    assert torch.equal(some.by_feature_distance, full.by_feature_distance[[190, 3, 3, 0]])
    assert torch.equal(some.by_node, full.by_node[[190, 3, 3, 0]])


@pytest.mark.parametrize("which", ["dense", "csr"])
def test_one_row_puts_each_source_at_exactly_one_distance(which):
    m = build("models_tensor_node", DEV)
    data = inputs_on(which, DEV)
    sources = [17, 0, 5, 29, 5]
    sx = interpret.explain_sources(m, data, rows=[17], sources=sources)
    per_distance = sx.by_feature_distance.abs().sum(dim=(1, 3))      # [P, D]
    assert ((per_distance > 0).sum(1) == 1).all(), per_distance
    assert per_distance[0, 0] > 0                                    # a node sees itself at hop 0
    ex = interpret.explain(m, data, rows=[17])
    everything = interpret.explain_sources(m, data, rows=[17])
    assert_rule(everything.by_feature_distance.sum(0), ex.by_feature_distance[0].double().cpu(), what="one row against explain",
                floor=TWO_FLOORS)


def test_training_mode_cpu_tensors_and_the_byte_budget(monkeypatch):
    from gnan_amd import attribution
    m = build("models_tensor_node", DEV)
    data = inputs_on("dense", DEV)
    with pytest.raises(_lib.GnanHipError, match="eval"):
        interpret.explain_sources(m.train(), data)
    m.eval()
    with pytest.raises(_lib.GnanHipError, match="ONE device"):
        interpret.explain_sources(m, inputs_on("dense", "cpu"))
    g = m.hop_graph(data)
    S = torch.rand(g.n_cols, 4, device=DEV)
    lut = torch.rand(g.n_codes, 1, device=DEV)
    with pytest.raises(_lib.GnanHipError, match="CPU tensor"):
        attribution.source_attributions(g, S.cpu(), lut, True)
    monkeypatch.setattr(attribution, "ATTR_MAX_BYTES", 4 * g.n_cols * g.n_codes * 4 - 1)
    with pytest.raises(_lib.GnanHipError, match=r"\[30, \d+, 4\] float32 takes \d+ bytes.*pass `cols` in batches"):
        attribution.source_attributions(g, S, lut, True)
    part = attribution.source_attributions(g, S, lut, True, cols=torch.arange(15, device=DEV))
    assert tuple(part.shape) == (15, g.n_codes, 4)
    monkeypatch.undo()
    assert torch.equal(part, attribution.source_attributions(g, S, lut, True)[:15])
