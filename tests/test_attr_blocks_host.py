"""Host side of ``gnan_attr_blocks`` (csrc/attr_blocks.hip) and of the batch fronts above it, all without a GPU: the ABI additions are
declared, exported and bound under ABI 51; every refusal happens before a HIP call; ``describe``'s arithmetic; the CPU route
against the float64 reference; ``GraphBatch`` on the CPU field by field; ``explain_graphs`` / ``importance_graphs`` on CPU modules
against the per-graph ``explain`` / ``explain_sources``; and the reference catches a planted error of twice the bound."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import attr_blocks_ref
import graph_batch_cases as cases
from attr_ref import check, violations
from conftest import ROOT
from helpers import TWO_FLOORS, assert_rule

import gnan_amd  # noqa: F401
from gnan_amd import _lib, batched, cpu_route, interpret, models
from gnan_amd.batched import HopBlocks

FUNCS = ("gnan_attr_blocks", "gnan_attr_blocks_workspace_bytes", "gnan_attr_blocks_describe")
P = 0x1000                      # a non-null pointer value: nothing is dereferenced before the refusals (or by describe)


def header():
    return open(os.path.join(ROOT, "include", "gnan_hip.h")).read()


def args(**kw):
    base = dict(code=P, node_off=P, code_off=P, n_graphs=3, total_nodes=100, max_nodes=65, S=P, W=8, s_stride=8, lut=P, D=5, Cw=1,
                B=P, b_stride=40, T=P)
    base.update(kw)
    return _lib.AttrBlocksArgs(**base)


def refused(a, code, text):
    lib = _lib.lib()
    assert lib.gnan_attr_blocks(a, None) == code
    msg = lib.gnan_last_error().decode()
    assert text in msg, msg
    return msg


def describe(a):
    info = _lib.AttrBlocksInfo()
    assert _lib.lib().gnan_attr_blocks_describe(a, info) == 0, _lib.lib().gnan_last_error()
    return info.as_dict()


def test_declared_exported_and_bound_under_abi_51():
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for f in FUNCS:
        assert re.search(r"\b%s\s*\(" % f, text), f
        assert hasattr(handle, f) and f in _lib.SYMBOLS, f
    for s in ("gnan_attr_blocks_args", "gnan_attr_blocks_info"):
        assert re.search(r"typedef struct %s \{" % s, text), s
    assert "#define GNAN_ABI_VERSION 51" in header()
    assert _lib.ABI_VERSION == 51 and _lib.lib().gnan_abi_version() == 51


def test_ctypes_field_order_matches_the_header():
    text = header()
    for struct, cls in (("gnan_attr_blocks_args", _lib.AttrBlocksArgs), ("gnan_attr_blocks_info", _lib.AttrBlocksInfo)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = [decl.strip().split()[-1].lstrip("*") for decl in body.split(";") if decl.strip()]
        assert fields == [f[0] for f in cls._fields_], struct


def test_refusals_come_before_any_hip_call():
    lib = _lib.lib()
    assert lib.gnan_attr_blocks(None, None) == _lib.ERR_BAD_ARG and b"null args" in lib.gnan_last_error()
    for name in ("code", "S", "lut", "node_off", "code_off"):
        refused(args(**{name: None}), _lib.ERR_BAD_ARG, "null")
    refused(args(B=None, T=None), _lib.ERR_BAD_ARG, "both outputs are NULL")
    assert "D=1" in refused(args(D=1, b_stride=8), _lib.ERR_UNSUPPORTED, "2 <= D <= 256")
    assert "D=257" in refused(args(D=257, b_stride=257 * 8), _lib.ERR_UNSUPPORTED, "2 <= D <= 256")
    assert "W must be >= 1 (got 0)" in refused(args(W=0), _lib.ERR_BAD_ARG, "W must be")
    assert "Cw=3, W=8" in refused(args(Cw=3), _lib.ERR_BAD_ARG, "Cw must divide W")
    refused(args(s_stride=7), _lib.ERR_BAD_ARG, "operand row stride")
    refused(args(b_stride=39), _lib.ERR_BAD_ARG, "output row stride")
    refused(args(cnt=P, cnt_stride=4), _lib.ERR_BAD_ARG, "cnt row stride")
    refused(args(lut_row_stride=4), _lib.ERR_BAD_ARG, "lut_row_stride")
    refused(args(n_graphs=-1), _lib.ERR_BAD_ARG, "negative size")
    refused(args(max_nodes=0), _lib.ERR_BAD_ARG, "max_nodes=0")
    refused(args(max_nodes=101), _lib.ERR_BAD_ARG, "above total_nodes")
    refused(args(n_graphs=1 << 31), _lib.ERR_UNSUPPORTED, "pass the graphs in batches")
    refused(args(n_graphs=1 << 30, total_nodes=1 << 30, max_nodes=129), _lib.ERR_UNSUPPORTED, "column tiles exceed one launch")
    info = _lib.AttrBlocksInfo()
    assert lib.gnan_attr_blocks_describe(args(), None) == _lib.ERR_BAD_ARG
    assert lib.gnan_attr_blocks_describe(args(D=257, b_stride=257 * 8), info) == _lib.ERR_UNSUPPORTED
    # nothing to do: no graph — accepted without a workspace and without a launch
    assert lib.gnan_attr_blocks(args(n_graphs=0, total_nodes=0, max_nodes=0), None) == 0
    # an output stride is not looked at where B is not asked for
    refused(args(B=None, b_stride=0), _lib.ERR_WORKSPACE, "workspace")


def test_short_workspace_is_refused_with_both_sizes():
    a = args()
    need = _lib.lib().gnan_attr_blocks_workspace_bytes(a)
    assert need == 100 * 5 * 1 * 4                                         # nodes x D x Cw floats: V alone
    assert str(need) in refused(a, _lib.ERR_WORKSPACE, "workspace")
    a.workspace, a.workspace_bytes = P, need - 4
    assert str(need - 4) in refused(a, _lib.ERR_WORKSPACE, str(need))


@pytest.mark.parametrize("Cw", [1, 3])
@pytest.mark.parametrize("D", [2, 64, 65, 256])
def test_describe_arithmetic(D, Cw):
    W, bins = 2 * Cw, D * Cw
    for per_row, with_cnt in ((False, False), (True, False), (False, True)):
        kw = dict(W=W, s_stride=W, D=D, Cw=Cw, b_stride=D * W, lut_row_stride=bins if per_row else 0)
        if with_cnt:
            kw.update(cnt=P, cnt_stride=D)
        d = describe(args(**kw))
        assert d["tile_cols"] == 64 and d["col_tiles"] == 2 and d["n_tiles"] == 3 * 2          # a graph of 65 nodes: two tiles each
        assert d["bin_passes"] == -(-bins // 64) and d["block_size"] == 64 * d["row_slices"] == 256
        staged = d["row_chunk"] if (per_row or with_cnt) else 1
        assert d["lds_bytes"] == (d["row_slices"] * 64 + staged) * min(bins, 64) * 4 <= 160 * 1024
        assert d["workspace_bytes"] == d["v_bytes"] == 100 * bins * 4 == _lib.lib().gnan_attr_blocks_workspace_bytes(args(**kw))
        assert d["launches"] == 3
        assert describe(args(T=None, **kw))["launches"] == 2 and describe(args(B=None, **kw))["launches"] == 2
    assert describe(args(max_nodes=64))["col_tiles"] == 1 and describe(args(max_nodes=1))["col_tiles"] == 1
    assert describe(args(n_graphs=0, total_nodes=0, max_nodes=0))["launches"] == 0
    assert describe(args(n_graphs=4, total_nodes=0, max_nodes=0, B=None))["launches"] == 1     # empty graphs only: their zero rows of T


# ---------------------------------------------------------------------------------------------
# the CPU route and the reference
# ---------------------------------------------------------------------------------------------
def cpu_case(D=6, W=6, Cw=3, sizes=(1, 2, 9, 0, 70, 5)):
    gen = torch.Generator().manual_seed(D)
    N, Pn = sum(sizes), sum(s * s for s in sizes)
    code = torch.randint(0, D + 2, (Pn,), generator=gen).to(torch.uint8)
    code[torch.rand(Pn, generator=gen) < 0.2] = 255
    node_off, code_off = HopBlocks._offsets(sizes, "cpu")
    blocks = HopBlocks(code, node_off, code_off, sizes, D - 2)
    return blocks, torch.randn((N, W), generator=gen), torch.randn((N, D, Cw), generator=gen)


def test_cpu_route_block_attributions_against_the_reference():
    blocks, S, wt = cpu_case()
    B, T = cpu_route.block_attributions(blocks, S, wt)
    tB, bB, tT, bT = attr_blocks_ref.reference(blocks.code, blocks.sizes, S, wt)
    check(B, tB, bB, "cpu_route B")
    check(T, tT, bT, "cpu_route T")
    assert not bool(T[3].any())
    only_T = cpu_route.block_attributions(blocks, S, wt, want_nodes=False)
    assert only_T[0] is None and torch.equal(only_T[1], T)


def test_a_planted_error_of_twice_the_bound_is_caught():
    blocks, S, wt = cpu_case()
    tB, bB, tT, bT = attr_blocks_ref.reference(blocks.code, blocks.sizes, S, wt)
    for truth, bound in ((tB, bB), (tT, bT)):
        assert len(violations(truth.copy(), truth, bound)) == 0
        at = tuple(np.argwhere(bound > 0)[len(np.argwhere(bound > 0)) // 2])
        bad = truth.copy()
        bad[at] += 2.0 * bound[at]
        assert [tuple(v) for v in violations(bad, truth, bound)] == [at]
        zero = tuple(np.argwhere(bound == 0)[0])                              # where the bound is 0 the value must be exactly 0
        bad = truth.copy()
        bad[zero] = 1e-30
        assert [tuple(v) for v in violations(bad, truth, bound)] == [zero]


# ---------------------------------------------------------------------------------------------
# the batch and the model-level fronts on the CPU
# ---------------------------------------------------------------------------------------------
def test_graph_batch_on_the_cpu_field_by_field():
    datas = cases.datas("cpu")
    b = interpret.GraphBatch.from_datas(datas)
    D = max(g[4] for g in cases.graphs())
    assert b.sizes == cases.SIZES and b.n_graphs == len(cases.SIZES) and b.total_nodes == sum(cases.SIZES) and b.n_codes == D
    assert b.blocks.node_off.dtype == torch.int32 and b.blocks.code_off.dtype == torch.int64 and b.blocks.code.dtype == torch.uint8
    assert b.blocks.node_off.tolist() == np.cumsum([0] + cases.SIZES).tolist()
    assert b.blocks.code_off.tolist() == np.cumsum([0] + [s * s for s in cases.SIZES]).tolist()
    assert torch.equal(b.x, torch.cat([d.x for d in datas]))
    assert b.cnt.dtype == torch.int32 and tuple(b.cnt.shape) == (b.total_nodes, D)
    n0 = c0 = 0
    for d, n in zip(datas, cases.SIZES):
        g = cpu_route.graph_from_dense(d.node_distances, d.normalization_matrix)
        assert torch.equal(b.blocks.code[c0: c0 + n * n].view(n, n), g.code)
        Dg = g.n_codes
        mine = b.cnt[n0: n0 + n]
        assert torch.equal(mine[:, : Dg - 1], g.cnt[:, : Dg - 1]) and torch.equal(mine[:, D - 1], g.cnt[:, Dg - 1])
        assert not bool(mine[:, Dg - 1: D - 1].any())                         # hops no pair of the graph has
        assert bool((mine.sum(1) == n).all())
        n0, c0 = n0 + n, c0 + n * n
    part = b.graphs(2, 5)
    assert part.sizes == cases.SIZES[2:5] and part.blocks.node_off.tolist() == [0, 30, 94, 159] and part.n_codes == D
    assert torch.equal(part.x, b.x[8: 8 + 159]) and torch.equal(part.cnt, b.cnt[8: 8 + 159])
    with pytest.raises(_lib.GnanHipError, match="CPU tensor"):
        interpret.GraphBatch.from_edge_index(b.x, datas[1].edge_index, torch.zeros(7, dtype=torch.int64))


def close(a, b, what):
    assert_rule(a, b.double(), what=what, floor=TWO_FLOORS)


@pytest.mark.parametrize("name", list(cases.MODULES))
def test_explain_graphs_on_a_cpu_module_against_the_single_graph_calls(name):
    m = cases.build(name, "cpu")
    datas = cases.datas("cpu")
    batch = interpret.GraphBatch.from_datas(datas)
    ex = interpret.explain_graphs(m, batch)
    G, N, D, F = len(cases.SIZES), sum(cases.SIZES), batch.n_codes, cases.F_RAW + 1
    C = ex.by_graph.shape[-1]
    assert tuple(ex.by_graph.shape) == (G, F, D, C) and tuple(ex.by_node_feature_distance.shape) == (N, F, D, C)
    assert ex.hops.tolist() == [float(d) for d in range(D - 1)] + [float("inf")]
    assert ex.node_off.tolist() == np.cumsum([0] + cases.SIZES).tolist()
    assert ex.graph_of.tolist() == np.repeat(np.arange(G), cases.SIZES).tolist()
    assert torch.equal(ex.output, ex.by_graph.sum(dim=2).sum(dim=1)) and torch.equal(ex.by_node, ex.by_node_feature_distance.sum(dim=2).sum(dim=1))
    readout = isinstance(m, models.TensorGNAN) and m.readout_n_layers > 0
    n0 = 0
    for g, (d, n) in enumerate(zip(datas, cases.SIZES)):
        Dg = cases.graphs()[g][4]
        one = interpret.explain(m, d)
        src = interpret.explain_sources(m, d)
        cases.compare_with_single(ex.by_graph[g], one.graph_by_feature_distance, D, Dg, f"{name}: graph {g} by_graph", close)
        cases.compare_with_single(ex.by_node_feature_distance[n0: n0 + n], src.by_feature_distance, D, Dg, f"{name}: graph {g} by node", close)
        y = m(d).detach().double().view(-1)
        if readout:
            close(ex.hidden[g], one.hidden, f"{name}: graph {g} hidden")
            close(ex.hidden_by_node[n0: n0 + n], src.hidden_by_node, f"{name}: graph {g} hidden_by_node")
            close(ex.readout_by_feature[g], one.readout_by_feature, f"{name}: graph {g} read-out")
            close(ex.readout_by_feature[g].sum(0), y, f"{name}: graph {g} read-out sum against forward")
        else:
            close(ex.output[g], y, f"{name}: graph {g} output against forward")
        n0 += n
    if not readout:
        assert ex.hidden is None and ex.hidden_by_node is None and ex.readout_by_feature is None
    lean = interpret.explain_graphs(m, batch, by_node=False)
    assert lean.by_node_feature_distance is None and lean.by_node is None and lean.hidden_by_node is None
    assert torch.equal(lean.by_graph, ex.by_graph)


@pytest.mark.parametrize("name", ["standalone_tensor_graph_pre_rho", "models_tensor_graph_readout", "models_tensor_graph_rho_per_feature"])
def test_importance_graphs_on_a_cpu_module(name):
    m = cases.build(name, "cpu")
    batch = interpret.GraphBatch.from_datas(cases.datas("cpu"))
    ex = interpret.explain_graphs(m, batch, by_node=False)
    imp = interpret.importance_graphs(m, batch, groups=cases.LABELS)
    assert imp.group_labels.tolist() == [0, 1] and imp.count.tolist() == [3.0, 3.0]
    a = ex.by_graph.double()
    lab = torch.tensor(cases.LABELS)
    for r, label in enumerate((0, 1)):
        part = a[lab == label]
        assert torch.allclose(imp.mean[r], part.mean(0), rtol=1e-12, atol=0) and torch.allclose(imp.mean_abs[r], part.abs().mean(0), rtol=1e-12, atol=0)
        assert torch.allclose(imp.rms[r], (part * part).mean(0).sqrt(), rtol=1e-12, atol=0)
        tot = part.sum(2)
        assert torch.allclose(imp.feature_mean[r], tot.mean(0), rtol=1e-12, atol=1e-300)
        assert torch.allclose(imp.feature_mean_abs[r], tot.abs().mean(0), rtol=1e-12, atol=0)
        assert torch.allclose(imp.feature_rms[r], (tot * tot).mean(0).sqrt(), rtol=1e-12, atol=0)
    for dt in (imp.mean, imp.rms, imp.feature_mean, imp.count, imp.hops):
        assert dt.dtype == torch.float64
    three = interpret.importance_graphs(m, batch, groups=cases.LABELS, max_nodes_per_pass=140)      # three passes: 1+7+30+64 | 65 | 140
    assert torch.equal(three.mean, imp.mean) and torch.equal(three.feature_rms, imp.feature_rms)
    whole = interpret.importance_graphs(m, batch)
    assert whole.group_labels.tolist() == [0] and whole.count.tolist() == [6.0]
    with pytest.raises(ValueError, match="one label per graph"):
        interpret.importance_graphs(m, batch, groups=[0, 1])


def test_refusals_name_the_single_graph_fronts():
    batch = interpret.GraphBatch.from_datas(cases.datas("cpu"))
    node_task = cases.redraw(models.TensorGNAN(cases.F_RAW + 1, 3, 3, hidden_channels=8), "n").eval()
    for m in (node_task, models.GNAN(cases.F_RAW + 1, 2, num_layers=3, hidden_channels=8).eval(),
              models.NAM(cases.F_RAW + 1, 2, 2, hidden_channels=8).eval(),
              batched.TensorGNAN(cases.F_RAW + 1, 2, 2, hidden_channels=8, is_graph_task=False).eval()):
        for front in (interpret.explain_graphs, interpret.importance_graphs):
            with pytest.raises(_lib.GnanHipError, match="explain / explain_sources"):
                front(m, batch)
    m = cases.build("models_tensor_graph", "cpu").train()
    with pytest.raises(_lib.GnanHipError, match=r"eval\(\) mode"):
        interpret.explain_graphs(m, batch)
    with pytest.raises(_lib.GnanHipError, match="no CPU route"):
        interpret.explain_graphs(batched.TensorGNAN(cases.F_RAW + 1, 2, 2, hidden_channels=8).eval(), batch)
    with pytest.raises(_lib.GnanHipError, match="batched.TensorGNAN evaluates many graphs"):
        interpret.explain(batched.TensorGNAN(cases.F_RAW + 1, 2, 2, hidden_channels=8).eval(), cases.datas("cpu")[1])
