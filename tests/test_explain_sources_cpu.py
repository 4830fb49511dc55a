"""``interpret.explain_sources`` on the CPU route (``cpu_route.source_attributions``: plain torch, no kernels) — no GPU needed.

Every element of ``by_feature_distance`` against the dense float64 restatement by source node (tests/attr_cols_ref.py, no hop
code formed) for the module table of tests/test_gpu_explain.py; the identities that tie it to ``interpret.explain`` (summed over
the sources it is ``explain``'s result summed over the rows) and to the module's forward; and ``cpu_route.source_attributions``
itself against the per-element bound of ``attr_cols_ref.reference``."""
import numpy as np
import pytest
import torch

import attr_cols_ref
import attr_ref
import gpu_util
from helpers import TWO_FLOORS, assert_rule
from test_gpu_explain import F_RAW, MODULES, build, forward, graph_case, inputs_on

from gnan_amd import HopGraph, _lib, cpu_route, interpret, models


@pytest.mark.parametrize("which", ["dense", "csr"])
@pytest.mark.parametrize("name", list(MODULES))
def test_cpu_route_matches_the_restatement_explain_and_the_forward(name, which):
    _, kind, node_ids = MODULES[name]
    x, nd, norm, csr, D = graph_case(which)
    m = build(name, "cpu")
    data = inputs_on(which, "cpu")
    sx = interpret.explain_sources(m, data, node_ids=node_ids)
    n = x.shape[0]
    C = sx.by_feature_distance.shape[-1]
    assert tuple(sx.by_feature_distance.shape) == (n, F_RAW + 1, D, C) and not sx.by_feature_distance.is_cuda
    assert sx.hops.tolist() == [float(d) for d in range(D - 1)] + [float("inf")]
    assert sx.sources.tolist() == list(range(n)) and sx.rows.tolist() == (list(range(n)) if node_ids is None else node_ids)
    params = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    truth = attr_cols_ref.explain_sources_restatement(kind, x, nd, norm, params, bool(m.normalize_rho), D, node_ids)
    assert_rule(sx.by_feature_distance, truth, what=f"{name}/{which}: by_feature_distance")
    if which == "csr" and any(k.startswith("rho.") and k.endswith("bias") for k in params):
        assert float(truth[:, :, D - 1].abs().max()) > 0            # a biased rho: the rest column carries weight
    assert torch.equal(sx.by_node, sx.by_feature_distance.sum(dim=2).sum(dim=1))
    # summed over the sources: explain's result summed over the rows (two routes of the build)
    ex = interpret.explain(m, data, node_ids=node_ids)
    assert_rule(sx.by_feature_distance.sum(0), ex.by_feature_distance.double().sum(0), what=f"{name}/{which}: against explain",
                floor=TWO_FLOORS)
    rows_truth = attr_ref.explain_restatement(kind, x, nd, norm, params, bool(m.normalize_rho), D, node_ids)
    assert float((truth.sum(0) - rows_truth.sum(0)).abs().max()) <= 1e-12 * float(rows_truth.sum(0).abs().max())
    # by_node against the module's own forward
    y = forward(m, data, node_ids).double()
    graph_task = bool(getattr(m, "is_graph_task", False))
    with_readout = graph_task and getattr(m, "readout_n_layers", 0) > 0 and isinstance(m, models.TensorGNAN)
    if with_readout:
        assert tuple(sx.hidden_by_node.shape) == (n, F_RAW + 1)
        assert_rule(sx.hidden_by_node.sum(0), ex.hidden.double(), what=f"{name}/{which}: hidden_by_node", floor=TWO_FLOORS)
        assert_rule(sx.hidden_by_node, truth.sum(2).view(n, -1), what=f"{name}/{which}: hidden_by_node against the restatement")
    else:
        assert sx.hidden_by_node is None
        total = sx.by_node.sum(0)
        assert_rule(total.view(-1, 1) if graph_task else total, y if graph_task else y.sum(0), what=f"{name}/{which}: by_node against forward",
                    floor=TWO_FLOORS)
    # sources in any order, with repeats: the rows of the full result
    some = interpret.explain_sources(m, data, node_ids=node_ids, sources=[n - 1, 3, 3, 0])
    assert some.sources.tolist() == [n - 1, 3, 3, 0]
    assert torch.equal(some.by_feature_distance, sx.by_feature_distance[[n - 1, 3, 3, 0]])


def test_one_row_puts_each_source_at_exactly_one_distance():
    m = build("models_tensor_node", "cpu")
    data = inputs_on("csr", "cpu")
    sx = interpret.explain_sources(m, data, rows=[17])
    per_distance = sx.by_feature_distance.abs().sum(dim=(1, 3))      # [P, D]
    assert ((per_distance > 0).sum(1) == 1).all()                    # one row sees a node at one hop — or not at all: the rest
    full = interpret.explain(m, data, rows=[17])
    assert_rule(sx.by_feature_distance.sum(0), full.by_feature_distance[0].double(), what="one row", floor=TWO_FLOORS)


def test_nam_a_node_is_its_own_only_source():
    m = models.NAM(F_RAW + 1, 3, 3, hidden_channels=8).eval()
    x = graph_case("dense")[0]
    sx = interpret.explain_sources(m, x, rows=[4, 2, 4], sources=[2, 4, 5])
    ex = interpret.explain(m, x)
    assert sx.hops.tolist() == [0.0] and tuple(sx.by_feature_distance.shape) == (3, F_RAW + 1, 1, 3)
    want = torch.stack([ex.by_feature_distance[2], 2 * ex.by_feature_distance[4], 0 * ex.by_feature_distance[5]])
    assert torch.equal(sx.by_feature_distance, want)


def test_explain_sources_wants_eval_mode_and_one_device():
    m = build("models_tensor_node", "cpu")
    data = inputs_on("dense", "cpu")
    with pytest.raises(_lib.GnanHipError, match="eval"):
        interpret.explain_sources(m.train(), data)
    with pytest.raises(_lib.GnanHipError, match="ONE device"):
        interpret.explain_sources(m.eval(), gpu_util.Bag(x=torch.empty(30, F_RAW + 1, device="meta")))


@pytest.mark.parametrize("with_rest", [False, True])
@pytest.mark.parametrize("layout", ["csr", "dense"])
def test_cpu_source_attributions_within_the_derived_bound(layout, with_rest):
    """The plain-torch twin against the float64 truth of the kernel's definition: repeating rows, repeating sources, duplicate
    pairs, counts holding 0, a per-row table with two weight channels."""
    rng = np.random.default_rng(5)
    n_rows, n_src, D, Cw, W = 40, 23, 5, 2, 6
    cnt = torch.from_numpy(rng.integers(0, 9, (n_rows, D)).astype(np.int32))
    if layout == "csr":
        lens = rng.integers(0, 9, n_rows)
        lens[3] = 0
        rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        col = rng.integers(0, n_src, int(rowptr[-1])).astype(np.int32)         # duplicates of a pair happen
        code = rng.integers(0, D - 1, int(rowptr[-1])).astype(np.uint8)
        g = HopGraph.from_csr(torch.from_numpy(rowptr), torch.from_numpy(col), torch.from_numpy(code), n_cols=n_src, n_codes=D, cnt=cnt)
    else:
        code = torch.from_numpy(rng.integers(0, D + 2, (n_rows, n_src)).astype(np.uint8))      # codes past the cover: the rest shell
        g = HopGraph(n_rows=n_rows, n_cols=n_src, n_codes=D, code=code, cnt=cnt)
    S = torch.from_numpy(rng.standard_normal((n_src, W)).astype(np.float32))
    lut = torch.from_numpy(rng.standard_normal((n_rows, D, Cw)).astype(np.float32))
    wt = lut / cnt.clamp_min(1).float().unsqueeze(-1)
    rows = torch.tensor([7, 1, 7, 30, 3, 12, 7])
    cols = torch.tensor([22, 0, 5, 5, 9])
    got = cpu_route.source_attributions(g, S, wt, rows, cols, with_rest=with_rest)
    t = g.transposed()
    truth, bound, mag = attr_cols_ref.reference(t.code, S, lut, t.rowptr if layout == "csr" else None, t.col if layout == "csr" else None,
                                                cnt, rows, cols, with_rest, n_rows)
    attr_ref.check(got, truth, bound, f"{layout} with_rest={with_rest}")
    assert (got.numpy()[bound == 0] == 0).all() and (bound > 0).any()
    # summed over all sources: the row side summed over the rows
    everything = cpu_route.source_attributions(g, S, wt, rows, None, with_rest=with_rest)
    by_rows = cpu_route.shell_attributions(g, S, wt, rows, with_rest=with_rest)
    assert_rule(everything.sum(0), by_rows.double().sum(0), what="sum over sources against sum over rows", floor=TWO_FLOORS)
