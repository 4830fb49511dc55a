"""``interpret.explain_graphs`` / ``importance_graphs`` on the HIP path (``gnan_attr_blocks``): a batch of graphs of 1, 7, 30, 64, 65
and 140 nodes through every graph-level module class — per graph against the dense float64 restatements, the single-graph
``explain`` / ``explain_sources``, the module's own forward and the CPU twin; ``batched.TensorGNAN`` against its forward and a float64
restatement of the batched script's maths; ``GraphBatch`` against ``HopGraph.batch_from_edge_index``."""
import functools

import numpy as np
import pytest
import torch

import attr_cols_ref
import attr_ref
import graph_batch_cases as cases
from helpers import TWO_FLOORS, assert_rule
from oracle import gnan_oracle as O

from gnan_amd import HopGraph, _lib, attribution, batched, interpret, models
from gnan_amd.graph import cat_edges
from gnan_amd.small_graph import SlotGraph

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = cases.F_RAW + 1


@functools.lru_cache(maxsize=None)
def device_batch():
    datas = cases.datas(DEV)
    return datas, interpret.GraphBatch.from_datas(datas)


def close(a, b, what):
    assert_rule(a, b.double(), what=what, floor=TWO_FLOORS)


def test_graph_batch_field_by_field_against_batch_from_edge_index():
    datas, b = device_batch()
    D = max(g[4] for g in cases.graphs())
    assert b.sizes == cases.SIZES and b.n_codes == D and b.x.is_cuda and torch.equal(b.x, torch.cat([d.x for d in datas]))
    assert b.blocks.node_off.tolist() == np.cumsum([0] + cases.SIZES).tolist()
    assert b.blocks.code_off.tolist() == np.cumsum([0] + [s * s for s in cases.SIZES]).tolist()
    ei, graph_of = cat_edges([d.edge_index for d in datas], cases.SIZES, DEV)
    singles = HopGraph.batch_from_edge_index(ei, graph_of, len(cases.SIZES), sizes=cases.SIZES)
    slot = SlotGraph(F, "cpu", n_codes=D)
    n0 = c0 = 0
    for g, n in zip(singles, cases.SIZES):
        assert torch.equal(b.blocks.code[c0: c0 + n * n].view(n, n), g.code)
        cpu = HopGraph(n_rows=n, n_cols=n, n_codes=g.n_codes, code=g.code.cpu(), cnt=g.cnt.cpu())
        want = slot._cnt_layout(cpu)
        # the slot layout leaves the hops no pair has at 1, the batch's bincount at 0: every reader takes max(cnt, 1)
        assert torch.equal(b.cnt[n0: n0 + n].cpu().clamp_min(1), want.clamp_min(1))
        assert not bool(b.cnt[n0: n0 + n, g.n_codes - 1: D - 1].any())
        n0, c0 = n0 + n, c0 + n * n
    again = interpret.GraphBatch.from_edge_index(b.x, ei, graph_of, len(cases.SIZES))
    assert torch.equal(again.blocks.code, b.blocks.code) and torch.equal(again.cnt, b.cnt) and again.sizes == b.sizes


@pytest.mark.parametrize("name", list(cases.MODULES))
def test_explain_graphs_per_graph(name):
    _, kind, _ = cases.MODULES[name]
    m = cases.build(name, DEV)
    datas, batch = device_batch()
    ex = interpret.explain_graphs(m, batch)
    G, N, D = len(cases.SIZES), sum(cases.SIZES), batch.n_codes
    C = ex.by_graph.shape[-1]
    assert ex.by_graph.is_cuda and tuple(ex.by_graph.shape) == (G, F, D, C) and tuple(ex.by_node_feature_distance.shape) == (N, F, D, C)
    assert ex.hops.tolist() == [float(d) for d in range(D - 1)] + [float("inf")]
    assert ex.node_off.tolist() == np.cumsum([0] + cases.SIZES).tolist()
    assert ex.graph_of.tolist() == np.repeat(np.arange(G), cases.SIZES).tolist()
    assert torch.equal(ex.output, ex.by_graph.sum(dim=2).sum(dim=1))
    params = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    readout = isinstance(m, models.TensorGNAN) and m.readout_n_layers > 0
    twin = interpret.explain_graphs(cases.build(name, "cpu"), interpret.GraphBatch.from_datas(cases.datas("cpu")))
    n0 = 0
    for g, (d, n) in enumerate(zip(datas, cases.SIZES)):
        x, _, nd, norm, Dg = cases.graphs()[g]
        what = f"{name}: graph {g}"
        rows = attr_ref.explain_restatement(kind, x, nd, norm, params, bool(m.normalize_rho), D)
        assert_rule(ex.by_graph[g], rows.sum(0), what=what + " by_graph against the restatement")
        by_src = attr_cols_ref.explain_sources_restatement(kind, x, nd, norm, params, bool(m.normalize_rho), D)
        assert_rule(ex.by_node_feature_distance[n0: n0 + n], by_src, what=what + " by node against the restatement")
        one, src = interpret.explain(m, d), interpret.explain_sources(m, d)
        cases.compare_with_single(ex.by_graph[g], one.graph_by_feature_distance, D, Dg, what + " by_graph", close)
        cases.compare_with_single(ex.by_node_feature_distance[n0: n0 + n], src.by_feature_distance, D, Dg, what + " by node", close)
        with torch.no_grad():
            y = m(d).double().view(-1)
        if readout:
            close(ex.readout_by_feature[g].sum(0), y, what + " read-out sum against forward")
            close(ex.hidden[g], one.hidden, what + " hidden")
            close(ex.hidden_by_node[n0: n0 + n], src.hidden_by_node, what + " hidden_by_node")
        else:
            close(ex.output[g], y, what + " output against forward")
        close(ex.by_graph[g], twin.by_graph[g], what + " CPU twin")
        close(ex.by_node_feature_distance[n0: n0 + n], twin.by_node_feature_distance[n0: n0 + n], what + " CPU twin by node")
        n0 += n
    if readout:
        assert tuple(ex.readout_by_feature.shape) == (G, F, m.out_channels)
        close(ex.readout_by_feature, twin.readout_by_feature, f"{name}: CPU twin read-out")
    lean = interpret.explain_graphs(m, batch, by_node=False)
    assert lean.by_node_feature_distance is None and torch.equal(lean.by_graph, ex.by_graph)


def test_batched_tensor_gnan_against_its_forward_and_the_scripts_maths():
    m = cases.redraw(batched.TensorGNAN(F, 2, 2, hidden_channels=8), "batched").to(DEV).eval()
    _, batch = device_batch()
    blocks, bv = batch.blocks, batch.blocks.batch_vector()
    G, N, D = len(cases.SIZES), sum(cases.SIZES), batch.n_codes
    ex = interpret.explain_graphs(m, (batch.x, blocks, bv))
    same = interpret.explain_graphs(m, batch)
    assert torch.equal(ex.by_graph, same.by_graph) and torch.equal(ex.by_node_feature_distance, same.by_node_feature_distance)
    with torch.no_grad():
        close(ex.output, m(batch.x, blocks, bv), "output against the forward")
    # float64: rho on the raw hop counts, the unreachable pairs weigh nothing (batched_pyg_main.py:151-159)
    p64 = {k: v.detach().cpu().double() for k, v in m.state_dict().items()}
    rho = O.mlp_apply(O.mlp_layers(p64, "rho"), torch.arange(D - 1, dtype=torch.float64).view(-1, 1))      # [D - 1, C]
    dist = torch.full((N, N), -1.0, dtype=torch.float64)
    n0 = 0
    for g, n in enumerate(cases.SIZES):
        x, _, nd, _, _ = cases.graphs()[g]
        hops = torch.from_numpy(O.hop_codes_from_dense(nd).astype(np.int64))                               # -1: unreachable
        dist[n0: n0 + n, n0: n0 + n] = hops.double()
        fx = O.feature_mlps(x.double(), p64)                                                               # [n, F, C]
        truth = torch.zeros((n, F, D, 2), dtype=torch.float64)
        for d in range(D - 1):
            seen = (hops == d).double().sum(0)                                                             # rows that see node j at hop d
            truth[:, :, d] = seen.view(-1, 1, 1) * rho[d].view(1, 1, -1) * fx
        assert_rule(ex.by_node_feature_distance[n0: n0 + n], truth, what=f"graph {g} by node")
        assert_rule(ex.by_graph[g], truth.sum(0), what=f"graph {g} by_graph")
        assert not bool(ex.by_graph[g, :, D - 1].any())
        n0 += n
    out64 = O.batched_tensor_gnan_forward(torch.cat([g[0] for g in cases.graphs()]).double(), dist, bv.cpu(), p64)
    assert_rule(ex.output, out64, what="output against the oracle", floor=TWO_FLOORS)
    imp = interpret.importance_graphs(m, (batch.x, blocks, bv), groups=cases.LABELS)
    assert tuple(imp.mean.shape) == (2, F, D, 2)
    with pytest.raises(_lib.GnanHipError, match="explain / explain_sources"):
        interpret.explain_graphs(cases.redraw(batched.TensorGNAN(F, 2, 2, hidden_channels=8, is_graph_task=False), "b").to(DEV).eval(), batch)


@pytest.mark.parametrize("name", ["standalone_tensor_graph_pre_rho", "models_tensor_graph", "models_tensor_graph_readout"])
def test_importance_graphs(name):
    m = cases.build(name, DEV)
    datas, batch = device_batch()
    ex = interpret.explain_graphs(m, batch, by_node=False)
    imp = interpret.importance_graphs(m, batch, groups=cases.LABELS)
    assert imp.group_labels.tolist() == [0, 1] and imp.count.tolist() == [3.0, 3.0] and imp.mean.dtype == torch.float64 and imp.mean.is_cuda
    a, lab = ex.by_graph.double(), torch.tensor(cases.LABELS, device=DEV)
    readout = isinstance(m, models.TensorGNAN) and m.readout_n_layers > 0
    for r in (0, 1):
        part = a[lab == r]
        for got, want in ((imp.mean[r], part.mean(0)), (imp.mean_abs[r], part.abs().mean(0)), (imp.rms[r], (part * part).mean(0).sqrt()),
                          (imp.feature_mean[r], part.sum(2).mean(0)), (imp.feature_mean_abs[r], part.sum(2).abs().mean(0)),
                          (imp.feature_rms[r], (part.sum(2) ** 2).mean(0).sqrt())):
            assert torch.allclose(got, want, rtol=1e-12, atol=1e-300)
        if not readout:
            with torch.no_grad():
                ys = torch.stack([m(d).double().view(-1) for d, l in zip(datas, cases.LABELS) if l == r]).sum(0)
            close((imp.mean[r] * imp.count[r]).sum(dim=(0, 1)), ys, f"{name}: mean * count against the summed forwards, label {r}")
    three = interpret.importance_graphs(m, batch, groups=cases.LABELS, max_nodes_per_pass=140)      # three passes: 1+7+30+64 | 65 | 140
    for f in ("mean", "mean_abs", "rms", "feature_mean", "feature_mean_abs", "feature_rms"):
        close(getattr(three, f), getattr(imp, f), f"{name}: three passes, {f}")


def test_refusals():
    datas, batch = device_batch()
    m = cases.build("models_tensor_graph", DEV)
    with pytest.raises(_lib.GnanHipError, match=r"eval\(\) mode"):
        interpret.explain_graphs(m.train(), batch)
    m.eval()
    node_task = cases.redraw(models.TensorGNAN(F, 3, 3, hidden_channels=8), "n").to(DEV).eval()
    with pytest.raises(_lib.GnanHipError, match="explain / explain_sources"):
        interpret.explain_graphs(node_task, batch)
    with pytest.raises(_lib.GnanHipError, match="ONE device"):
        interpret.explain_graphs(m, interpret.GraphBatch.from_datas(cases.datas("cpu")))


def test_the_byte_budget_advises_batches(monkeypatch):
    _, batch = device_batch()
    m = cases.build("models_tensor_graph", DEV)
    N, D = sum(cases.SIZES), batch.n_codes
    monkeypatch.setattr(attribution, "ATTR_MAX_BYTES", N * D * F * 2 * 4 - 1)
    with pytest.raises(_lib.GnanHipError, match=r"\[%d, %d, %d\] float32 takes \d+ bytes.*pass the graphs in batches" % (N, D, F * 2)):
        interpret.explain_graphs(m, batch)
    assert interpret.explain_graphs(m, batch, by_node=False).by_node is None
    part = interpret.explain_graphs(m, batch.graphs(0, 4))
    assert tuple(part.by_node.shape) == (sum(cases.SIZES[:4]), 2)
