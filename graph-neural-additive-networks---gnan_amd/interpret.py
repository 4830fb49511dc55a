"""What the reference's notebook plots (mutagenicity_visualizations.ipynb cells 4-9): the distance
function rho on the hop grid, every shape function f_k on a value grid, and their product.

Everything here is read off the tables the fast path evaluates the model with: ``gnan_pwl_build`` tabulates each f_k and
rho EXACTLY (they are ReLU MLPs of a scalar, hence piecewise linear: breakpoints, values, slopes), and the curves are
``gnan_fpwl_fwd`` look-ups of a grid in those tables — the same kernels, the same numbers the forward pass uses.
:func:`shape_function_tables` / :func:`rho_table` hand out the tables themselves: the breakpoints are where a plot of f_k
bends, which a value grid can only approximate.  Device tensors in, device tensors out; no CPU path.

:func:`explain` goes from the global curves to one prediction: every term ``(feature k, distance d)`` of the sum that IS the
model's output for a node of a graph (``gnan_attr_rows`` on the HIP path, ``cpu_route.shell_attributions`` for a module that
lives on the CPU).  :func:`explain_sources` turns the same sum by SOURCE node: what every node of the graph adds to the outputs asked
for (``gnan_attr_cols`` / ``cpu_route.source_attributions``).  :func:`importance` is the global chart: the mean, mean magnitude and rms of
those terms over all nodes, a mask or the nodes of each class (``gnan_attr_reduce`` / ``cpu_route.reduced_attributions``), formed without
storing a term per row.  :func:`explain_graphs` / :func:`importance_graphs` ask the same of a whole :class:`GraphBatch` of graphs in one
pass (``gnan_attr_blocks`` / ``cpu_route.block_attributions``): graph-level models, per graph and per node."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch

from . import _lib
from .functional import StackedMLP, _c, _fpwl_launch, feature_mlps, stack_mlps
from .graph import hop_inputs


def _stacked(model, what: str) -> StackedMLP:
    p = model._stacked(what, model.fs if what == "fs" else [model.rho]) if hasattr(model, "_stacked") \
        else stack_mlps(model.fs if what == "fs" else [model.rho])
    _lib.require_device(p.w_last)
    return StackedMLP(*[_c(t) for t in p[:6]], *p[6:])


def _tables(p: StackedMLP):
    from .pwl import build_tables
    return build_tables(p)


@torch.no_grad()
def shape_function_tables(model):
    """The exact piecewise-linear tables of all shape functions (:class:`gnan_amd.pwl.PwlTables`): feature ``k`` owns pieces
    ``off[k] .. off[k+1]-1``; on piece ``i``, ``f_k(x) = val[i] + slope[i] * (x - anchor[i])``.  None if some f_k needs
    more pieces than the tables hold."""
    return _tables(_stacked(model, "fs"))


@torch.no_grad()
def rho_table(model):
    """The exact piecewise-linear table of the distance function rho (one 'feature')."""
    return _tables(_stacked(model, "rho"))


def _curve(p: StackedMLP, x: torch.Tensor) -> torch.Tensor:
    """``[n, F * C]``: every function of ``p`` at its column of ``x [n, F]`` — table look-up, or the shape-function
    kernels when the functions do not fit the tables."""
    t = _tables(p)
    if t is None:
        return feature_mlps(x, p, False)
    return _fpwl_launch(x, t, False)


@torch.no_grad()
def rho_curve(model, max_hop: int) -> torch.Tensor:
    """``rho(1/(1+d))`` for ``d = 0..max_hop`` followed by ``rho(0)`` (unreachable): ``[max_hop + 2, C_rho]``."""
    p = _stacked(model, "rho")
    u = hop_inputs(max_hop + 2, p.w_last.device)
    return _curve(p, u.view(-1, 1).contiguous())


@torch.no_grad()
def shape_functions(model, grid: torch.Tensor, features: Optional[list] = None) -> torch.Tensor:
    """``f_k(v)`` for every grid value ``v``: ``[len(features), len(grid), C]`` (the notebook evaluates ``f_k(1)``)."""
    p = _stacked(model, "fs")
    g = grid.to(p.w_last.device).float().reshape(-1)
    y = _curve(p, g.view(-1, 1).expand(-1, p.F).contiguous()).view(g.numel(), p.F, p.C).permute(1, 0, 2)
    return y.contiguous() if features is None else y[list(features)].contiguous()


@torch.no_grad()
def contribution_heatmap(model, max_hop: int, value: float = 1.0) -> torch.Tensor:
    """``f_k(value) * rho(1/(1+d))`` — the notebook's feature-by-distance heat map: ``[F, max_hop + 1, C]``."""
    f = shape_functions(model, torch.tensor([value]))[:, 0]          # [F, C]
    r = rho_curve(model, max_hop)[: max_hop + 1]                     # [D, C_rho]
    return f.unsqueeze(1) * r.unsqueeze(0)


# =============================================================================
# the shared preamble of explain / explain_sources / importance: operand, graph, weight table
# =============================================================================
@dataclass
class _Terms:
    """What the three attribution fronts start from: ``fx [N, F * C]`` (the shape functions of every node, the operand), and — but
    for a NAM, which has no graph — the hop graph, the weight table (``lut`` on the HIP path, per-row ``wt`` on the CPU route) and
    whether the shell sizes divide it."""
    x: torch.Tensor
    cpu: bool
    fx: torch.Tensor
    F: int
    C: int
    nam: bool
    g: object = None
    table: Optional[torch.Tensor] = None
    use_cnt: bool = False


def _terms(model, data, who: str) -> _Terms:
    from . import batched, cpu_route
    from .modules import NAM, StandaloneTensorGNAN, _GNANCore
    if isinstance(model, batched.TensorGNAN):
        raise _lib.GnanHipError(f"{who}() covers the single-graph modules; batched.TensorGNAN evaluates many graphs per call")
    if model.training:
        raise _lib.GnanHipError(f"{who}() describes the model in eval() mode (training-mode Dropout has no fixed decomposition)")
    x = data if torch.is_tensor(data) else data.x
    cpu = cpu_route.applies(model, x)
    if not cpu:
        _lib.require_device(x)
    f = model._stacked("fs", model.fs)
    fx = cpu_route.shape_functions(x, f, False) if cpu else feature_mlps(x, f, sum_features=False)      # [N, F * C]
    t = _Terms(x, cpu, fx, x.shape[1], fx.shape[1] // x.shape[1], isinstance(model, NAM))
    if t.nam:
        return t
    pre = isinstance(model, StandaloneTensorGNAN) and bool(model.normalize_rho)
    t.use_cnt = (not isinstance(model, StandaloneTensorGNAN)) and bool(model.normalize_rho)
    if cpu:
        want = True if isinstance(model, _GNANCore) else bool(model.normalize_rho)
        t.g = cpu_route.graph_of(model, data, want_norm=want)
        t.table = cpu_route._pre_rho_weights(model, t.g) if pre else cpu_route.shell_weights(t.g, cpu_route._rho_lut(model, t.g), t.use_cnt)
    else:
        t.g = model.hop_graph(data)
        t.table = model._lut_pre_rho(t.g) if pre else model._lut_global(t.g)
    return t


def _hops(D: int, dev) -> torch.Tensor:
    hops = torch.arange(D, dtype=torch.float32, device=dev)
    hops[D - 1] = float("inf")
    return hops


# =============================================================================
# per-prediction explanations: the (feature, distance) terms of rows
# =============================================================================
@dataclass
class Explanation:
    """The exact decomposition of the outputs of ``rows``: ``by_feature_distance[q, k, d, c]`` is what feature ``k`` of the nodes
    at hop ``hops[d]`` from node ``rows[q]`` adds to its channel ``c`` (``hops[-1] = inf``: every node beyond the listed hops).
    ``output[q] = by_feature_distance[q].sum((0, 1))`` — the model's output for the node.  Graph tasks (all rows requested) also
    carry the sum over the nodes, ``graph_by_feature_distance [F, D, C]``; a NAM read-out on top of it has ``hidden [F]`` (that sum
    over the distances) and ``readout_by_feature[k] = g_k(hidden[k])``, whose sum over ``k`` is the model's output."""
    rows: torch.Tensor
    by_feature_distance: torch.Tensor
    hops: torch.Tensor
    output: torch.Tensor
    graph_by_feature_distance: Optional[torch.Tensor] = None
    hidden: Optional[torch.Tensor] = None
    readout_by_feature: Optional[torch.Tensor] = None


@torch.no_grad()
def explain(model, data, rows=None, node_ids=None) -> Explanation:
    """Attributions of ``model``'s outputs for ``rows`` (``node_ids``: the same, under ``GNAN.forward``'s name; default: every
    node) on ``data`` — the model in ``eval()`` mode.  A module on the GPU runs ``gnan_attr_rows`` (device inputs only, as the
    forward); a module that lives on the CPU, called with CPU inputs, runs the plain-torch restatement of ``cpu_route``.
    The result's bytes grow as ``R * F * D * C``: ``attribution.ATTR_MAX_BYTES`` bounds them, pass ``rows`` in batches beyond."""
    from . import attribution, cpu_route
    from .functional import column_sums
    from .modules import TensorGNAN
    t = _terms(model, data, "explain")
    if rows is None:
        rows = node_ids
    x, cpu, fx, F, C, g = t.x, t.cpu, t.fx, t.F, t.C, t.g
    dev = x.device
    if rows is not None:
        rows = torch.as_tensor(list(rows) if not torch.is_tensor(rows) else rows).to(device=dev, dtype=torch.int64).view(-1)
    ids = torch.arange(x.shape[0], device=dev) if rows is None else rows
    if t.nam:                                                                 # no graph: one "distance", the node itself
        bfd = fx.float()[ids].view(-1, F, 1, C).contiguous()
        return Explanation(ids, bfd, torch.zeros(1, device=dev), bfd.sum(dim=2).sum(dim=1))
    if cpu:
        A = cpu_route.shell_attributions(g, fx, t.table, rows)
    else:
        A = attribution.shell_attributions(g, fx, t.table, t.use_cnt, rows, None if g.is_dense else column_sums(fx))
    D = g.n_codes
    bfd = A.view(-1, D, F, C).permute(0, 2, 1, 3).contiguous()                # [R, F, D, C]
    hops = _hops(D, dev)
    out = Explanation(ids, bfd, hops, bfd.sum(dim=2).sum(dim=1))
    if getattr(model, "is_graph_task", False) and rows is None:
        out.graph_by_feature_distance = bfd.sum(dim=0)                        # [F, D, C]  (framework arithmetic: DESIGN.md section 6)
        if isinstance(model, TensorGNAN) and model.readout_n_layers > 0:
            nam = model.readout_nam
            out.hidden = out.graph_by_feature_distance.sum(dim=1).view(-1)    # [F]  models.py:379
            h = out.hidden.view(1, -1)
            gk = cpu_route.shape_functions(h, nam._stacked("fs", nam.fs), False) if cpu \
                else feature_mlps(h.contiguous(), nam._stacked("fs", nam.fs), sum_features=False)
            out.readout_by_feature = gk.view(F, -1)                           # [F, out_channels]  models.py:380-381
    return out


# =============================================================================
# per-prediction explanations by source node: "which nodes does the prediction come from"
# =============================================================================
@dataclass
class SourceExplanation:
    """The outputs of ``rows``, summed, decomposed by SOURCE node: ``by_feature_distance[p, k, d, c]`` is what feature ``k`` of node
    ``sources[p]`` adds to channel ``c`` of those outputs from hop ``hops[d]`` (the hop at which the row sees the node;
    ``hops[-1] = inf``: the rows that do not list it).  A row that repeats in ``rows`` counts as often as it occurs.
    ``by_node[p] = by_feature_distance[p].sum((0, 1))``; over all sources it sums to the sum of the rows' outputs — a graph task's
    output before a read-out.  ``hidden_by_node [P, F]`` (graph task with a NAM read-out, all rows requested): each node's share of
    ``Explanation.hidden``."""
    sources: torch.Tensor
    rows: torch.Tensor
    hops: torch.Tensor
    by_feature_distance: torch.Tensor
    by_node: torch.Tensor
    hidden_by_node: Optional[torch.Tensor] = None


@torch.no_grad()
def explain_sources(model, data, rows=None, node_ids=None, sources=None) -> SourceExplanation:
    """Attributions of ``model``'s outputs for ``rows`` (``node_ids``: the same; default: every node) to the nodes ``sources``
    (default: every node; any order, repeats allowed) — the model in ``eval()`` mode, the same model cover as :func:`explain`.
    A module on the GPU runs ``gnan_attr_cols`` (device inputs only); a module that lives on the CPU, called with CPU inputs, runs
    ``cpu_route.source_attributions``.  The result's bytes grow as ``P * F * D * C``: ``attribution.ATTR_MAX_BYTES`` bounds them,
    pass ``sources`` in batches beyond."""
    from . import attribution, cpu_route
    from .modules import TensorGNAN
    t = _terms(model, data, "explain_sources")
    if rows is None:
        rows = node_ids
    x, cpu, fx, F, C, g = t.x, t.cpu, t.fx, t.F, t.C, t.g
    dev = x.device

    def ids_of(v):
        return torch.as_tensor(list(v) if not torch.is_tensor(v) else v).to(device=dev, dtype=torch.int64).view(-1)
    everything = torch.arange(x.shape[0], device=dev)
    row_ids = everything if rows is None else ids_of(rows)
    src_ids = everything if sources is None else ids_of(sources)
    if t.nam:                                                                 # no graph: a node is its own only source, at distance 0
        mult = torch.bincount(row_ids, minlength=x.shape[0]).to(torch.float32)
        bfd = (fx.float() * mult.unsqueeze(1))[src_ids].view(-1, F, 1, C).contiguous()
        return SourceExplanation(src_ids, row_ids, torch.zeros(1, device=dev), bfd, bfd.sum(dim=2).sum(dim=1))
    if cpu:
        B = cpu_route.source_attributions(g, fx, t.table, None if rows is None else row_ids, None if sources is None else src_ids)
    else:
        B = attribution.source_attributions(g, fx, t.table, t.use_cnt, None if rows is None else row_ids,
                                            None if sources is None else src_ids)
    D = g.n_codes
    bfd = B.view(-1, D, F, C).permute(0, 2, 1, 3).contiguous()                # [P, F, D, C]
    hops = _hops(D, dev)
    out = SourceExplanation(src_ids, row_ids, hops, bfd, bfd.sum(dim=2).sum(dim=1))
    if getattr(model, "is_graph_task", False) and rows is None and isinstance(model, TensorGNAN) and model.readout_n_layers > 0:
        out.hidden_by_node = bfd.sum(dim=2).view(-1, F)                       # [P, F]  (f is one wide; models.py:379 before the node sum)
    return out


# =============================================================================
# global importance: the attributions' moments over groups of rows
# =============================================================================
@dataclass
class Importance:
    """How much feature ``k`` at distance ``hops[d]`` contributes to channel ``c`` over the rows of group ``g`` — the moments of
    :class:`Explanation`'s ``by_feature_distance`` over each group, formed without it: ``mean``, ``mean_abs`` (the global importance
    chart) and ``rms``, each ``[G, F, D, C]``; ``feature_mean``, ``feature_mean_abs`` and ``feature_rms`` ``[G, F, C]`` are the same
    moments of a feature's TOTAL over the distances (``mean |sum_d A|``, which the per-distance moments cannot give).  ``rows``: the
    requested rows in the order the groups take them (sorted stably by label); ``group_labels [G]`` the distinct labels, ascending;
    ``count [G]`` the rows of each group.  Statistics, ``count`` and ``hops`` are float64.  ``mean * count`` summed over ``(k, d)`` is
    the sum of the model's outputs over the group."""
    rows: torch.Tensor
    group_labels: torch.Tensor
    count: torch.Tensor
    hops: torch.Tensor
    mean: torch.Tensor
    mean_abs: torch.Tensor
    rms: torch.Tensor
    feature_mean: torch.Tensor
    feature_mean_abs: torch.Tensor
    feature_rms: torch.Tensor


@torch.no_grad()
def importance(model, data, rows=None, node_ids=None, groups=None) -> Importance:
    """Global importance of ``model`` on ``data`` over ``rows`` (``node_ids``: the same; default: every node), optionally apart by
    ``groups`` — one integer label per requested row, the class for example.  The model cover and refusals are :func:`explain`'s.  A
    module on the GPU runs ``gnan_attr_reduce`` (the ``[R, F, D, C]`` terms are never stored, so no ``ATTR_MAX_BYTES`` applies);
    a module that lives on the CPU, called with CPU inputs, runs ``cpu_route.reduced_attributions``."""
    from . import attribution, cpu_route
    from .functional import column_sums
    t = _terms(model, data, "importance")
    if rows is None:
        rows = node_ids
    x, fx, F, C, g = t.x, t.fx, t.F, t.C, t.g
    dev = x.device

    def ints(v):
        return torch.as_tensor(list(v) if not torch.is_tensor(v) else v).to(device=dev, dtype=torch.int64).view(-1)
    ids = torch.arange(x.shape[0], device=dev) if rows is None else ints(rows)
    R = ids.numel()
    gp = None
    labels, count = torch.zeros(1, dtype=torch.int64, device=dev), torch.full((1,), R, dtype=torch.int64, device=dev)
    if groups is not None:
        lab = ints(groups)
        if lab.numel() != R:
            raise ValueError(f"groups must hold one label per requested row ({R}), got {lab.numel()}")
        order = torch.sort(lab, stable=True).indices
        ids = ids[order]
        labels, count = torch.unique_consecutive(lab[order], return_counts=True)
        gp = torch.zeros(labels.numel() + 1, dtype=torch.int64, device=dev)
        torch.cumsum(count, 0, out=gp[1:])
    G = labels.numel()
    if t.nam:                                                                 # no graph: one "distance"; framework arithmetic on [R, F * C]
        a = fx.double()[ids]
        who = torch.repeat_interleave(torch.arange(G, device=dev), count)
        M = torch.zeros((G, 3, 2, F * C), dtype=torch.float64, device=dev)
        for j, v in enumerate((a, a.abs(), a * a)):
            M[:, j, 0].index_add_(0, who, v)
        M[:, :, 1] = M[:, :, 0]
        D = 1
        hops = torch.zeros(1, dtype=torch.float64, device=dev)
    else:
        D = g.n_codes
        hops = _hops(D, dev).double()
        if t.cpu:
            M = cpu_route.reduced_attributions(g, fx, t.table, ids, gp)
        else:
            M = attribution.reduced_attributions(g, fx, t.table, t.use_cnt, None if rows is None and groups is None else ids, gp,
                                                 None if g.is_dense else column_sums(fx))
    M = M.view(G, 3, D + 1, F, C).permute(0, 1, 3, 2, 4)                      # [G, 3, F, D + 1, C]
    n = count.double().clamp_min(1.0).view(G, 1, 1, 1)
    mean, mean_abs, rms = M[:, 0] / n, M[:, 1] / n, (M[:, 2] / n).sqrt()
    return Importance(ids, labels, count.double(), hops, mean[:, :, :D].contiguous(), mean_abs[:, :, :D].contiguous(),
                      rms[:, :, :D].contiguous(), mean[:, :, D].contiguous(), mean_abs[:, :, D].contiguous(), rms[:, :, D].contiguous())


# =============================================================================
# a batch of graphs in one pass: per-graph and per-node terms (gnan_attr_blocks / cpu_route.block_attributions)
# =============================================================================
IMPORTANCE_NODES_PER_PASS = 1 << 18     # nodes of the graphs importance_graphs() hands to one gnan_attr_blocks call


@dataclass
class GraphBatch:
    """Many graphs for :func:`explain_graphs` / :func:`importance_graphs`: the node features ``x [N, F]`` of all graphs, node after
    node, their hop codes as :class:`gnan_amd.batched.HopBlocks` (``D = blocks.n_codes``: the batch's largest hop + 2) and the shell
    sizes ``cnt [N, D]`` int32 in the slot layout — column ``d < D - 1``: the pairs of the row coded ``d``; the last column: its
    unreachable pairs; a hop no pair of the row has: 0 (every reader takes ``max(cnt, 1)``).  ``sizes``: the graphs' node counts,
    on the host."""
    x: torch.Tensor
    blocks: object
    cnt: Optional[torch.Tensor]
    sizes: list

    @property
    def n_graphs(self) -> int:
        return len(self.sizes)

    @property
    def total_nodes(self) -> int:
        return sum(self.sizes)

    @property
    def n_codes(self) -> int:
        return self.blocks.n_codes

    @staticmethod
    def shell_counts(blocks) -> torch.Tensor:
        """``cnt [N, D]`` of ``blocks`` in the slot layout: one ``bincount`` over the ``sum n_g^2`` codes (integer, exact)."""
        dev = blocks.code.device
        G, N, D = blocks.n_graphs, blocks.total_nodes, blocks.n_codes
        if blocks.code.numel() == 0:
            return torch.zeros((N, D), dtype=torch.int32, device=dev)
        sizes = torch.tensor(blocks.sizes, dtype=torch.int64, device=dev)
        graph_of = torch.repeat_interleave(torch.arange(G, device=dev), sizes * sizes)
        local = torch.arange(blocks.code.numel(), device=dev) - blocks.code_off.long()[graph_of]
        row = blocks.node_off.long()[graph_of] + local // sizes[graph_of]
        shell = blocks.code.long().clamp_(max=D - 1)                          # 255 (unreachable inside the block) -> the last column
        return torch.bincount(row * D + shell, minlength=N * D).view(N, D).to(torch.int32)

    @staticmethod
    def _of(x, blocks) -> "GraphBatch":
        return GraphBatch(x, blocks, GraphBatch.shell_counts(blocks), list(blocks.sizes))

    @staticmethod
    def from_datas(datas) -> "GraphBatch":
        """From objects with ``x [n_g, F]`` and ``edge_index [2, E_g]`` (the graph's own node ids), as ``attach_hop_graphs`` takes them:
        the codes of all graphs by ``HopBlocks.from_edge_index`` (one ``gnan_bfs_blocks`` launch).  Objects that live on the CPU
        carry the reference's dense ``node_distances`` (or a ``gnan_graph``) instead; their codes are read off it."""
        from .batched import HopBlocks
        from .graph import cat_edges
        datas = list(datas)
        if not datas:
            raise ValueError("GraphBatch.from_datas: no graph")
        sizes = [int(d.x.shape[0]) for d in datas]
        x = torch.cat([d.x for d in datas], dim=0)
        if x.is_cuda:
            _lib.require_device(*[d.edge_index for d in datas])
            ei, graph_of = cat_edges([d.edge_index for d in datas], sizes, x.device)
            return GraphBatch._of(x, HopBlocks.from_edge_index(ei, graph_of, len(sizes), sizes=sizes))
        from . import cpu_route
        gs = [getattr(d, "gnan_graph", None) or cpu_route.graph_from_dense(d.node_distances, None) for d in datas]
        if any(not g.is_dense for g in gs):
            raise _lib.GnanHipError("GraphBatch holds dense hop blocks: a graph held as CSR goes through explain / explain_sources")
        code = torch.cat([g.code.reshape(-1) for g in gs])
        node_off, code_off = HopBlocks._offsets(sizes, "cpu")
        return GraphBatch._of(x, HopBlocks(code, node_off, code_off, sizes, max(g.n_codes for g in gs) - 2))

    @staticmethod
    def from_edge_index(x: torch.Tensor, edge_index: torch.Tensor, batch: torch.Tensor, num_graphs: Optional[int] = None) -> "GraphBatch":
        """From a PyG-style batch on the device: ``x [N, F]``, ``edge_index [2, E]`` with global node ids, the sorted ``batch [N]``."""
        from .batched import HopBlocks
        _lib.require_device(x, edge_index, batch)
        return GraphBatch._of(x, HopBlocks.from_edge_index(edge_index, batch, num_graphs))

    def graphs(self, g0: int, g1: int) -> "GraphBatch":
        """The graphs ``g0 .. g1 - 1`` as a batch of their own (views of this one's tensors, fresh offsets)."""
        from .batched import HopBlocks
        b = self.blocks
        sizes = self.sizes[g0:g1]
        n0, c0 = sum(self.sizes[:g0]), sum(s * s for s in self.sizes[:g0])
        n1, c1 = n0 + sum(sizes), c0 + sum(s * s for s in sizes)
        node_off, code_off = HopBlocks._offsets(sizes, b.code.device)
        return GraphBatch(self.x[n0:n1], HopBlocks(b.code[c0:c1], node_off, code_off, sizes, b.n_codes - 2),
                          None if self.cnt is None else self.cnt[n0:n1], sizes)


@dataclass
class _GraphTerms:
    """The preamble of the batch fronts: operand rows, weight table (``lut`` for the kernel; per-row ``wt`` on the CPU route), and
    the counts the kernel divides by (None: none, or already inside the table)."""
    batch: GraphBatch
    cpu: bool
    fx: torch.Tensor
    F: int
    C: int
    table: torch.Tensor
    cnt: Optional[torch.Tensor]


def _graph_terms(model, batch, who: str) -> _GraphTerms:
    from . import batched, cpu_route
    from .modules import StandaloneTensorGNAN, TensorGNAN
    covered = isinstance(model, (batched.TensorGNAN, StandaloneTensorGNAN, TensorGNAN)) and bool(getattr(model, "is_graph_task", False))
    if not covered:
        raise _lib.GnanHipError(f"{who}() covers graph-level models (TensorGNAN with is_graph_task, batched.TensorGNAN with "
                                f"is_graph_task); {type(model).__name__} here predicts per node or has no graph: use explain / "
                                "explain_sources on one graph")
    if model.training:
        raise _lib.GnanHipError(f"{who}() describes the model in eval() mode (training-mode Dropout has no fixed decomposition)")
    raw = isinstance(model, batched.TensorGNAN)
    if raw and not isinstance(batch, GraphBatch):
        x_batch, dist, bv = batch                                             # what its forward takes
        _lib.require_device(x_batch)
        blocks = model._blocks(dist, bv)
        if blocks is None:
            raise _lib.GnanHipError(f"{who}(): dist_batch is not block-diagonal over a sorted batch_vector")
        batch = GraphBatch(x_batch, blocks, None, list(blocks.sizes))
    if not isinstance(batch, GraphBatch):
        raise ValueError(f"{who}() takes a GraphBatch (GraphBatch.from_datas / from_edge_index)")
    if getattr(batch.blocks, "slots", False):
        raise _lib.GnanHipError(f"{who}(): these blocks are the slots of a captured step: their sizes live on the device only")
    x = batch.x
    cpu = cpu_route.applies(model, x, batch.blocks.code)
    if cpu and raw:
        raise _lib.GnanHipError("batched.TensorGNAN has no CPU route: move the module and the batch to the GPU")
    if not cpu:
        _lib.require_device(x, batch.blocks.code, batch.cnt)
    D, N = batch.n_codes, batch.total_nodes
    f, rho = model._stacked("fs", model.fs), model._stacked("rho", [model.rho])
    fx = cpu_route.shape_functions(x, f, False) if cpu else feature_mlps(x, f, sum_features=False)      # [N, F * C]: ONE call
    F = x.shape[1]
    t = _GraphTerms(batch, cpu, fx, F, fx.shape[1] // F, None, None)
    norm = (not raw) and bool(model.normalize_rho)
    if norm and batch.cnt is None:
        raise ValueError(f"{who}(): the model normalises by the shell sizes, the batch carries no cnt")
    pre = norm and isinstance(model, StandaloneTensorGNAN)
    dev = x.device
    if cpu:
        u = hop_inputs(D, "cpu")
        den = batch.cnt.clamp_min(1).float() if norm else None
        if pre:
            t.table = cpu_route._rho(model, u.unsqueeze(0) / den).view(N, D, -1)
        else:
            lut = cpu_route._rho(model, u)
            t.table = lut.unsqueeze(0) / den.unsqueeze(-1) if norm else lut.unsqueeze(0).expand(N, -1, -1)
    elif raw:
        hops = torch.arange(D - 1, dtype=torch.float32, device=dev).view(-1, 1)                 # rho on the raw hop counts
        t.table = torch.cat([feature_mlps(hops, rho, sum_features=False), torch.zeros(1, rho.C, device=dev)], dim=0)
    elif pre:
        from .functional import rho_row_lut
        t.table = rho_row_lut(batch.cnt, hop_inputs(D, dev), rho)                               # [N, D, C]
    else:
        t.table = feature_mlps(hop_inputs(D, dev).view(-1, 1), rho, sum_features=False)         # [D, C_rho]: ONE call
        t.cnt = batch.cnt if norm else None
    return t


def _block_terms(t: _GraphTerms, batch: GraphBatch, n0: int, want_nodes: bool, want_graphs: bool):
    """``(B, T)`` of ``batch`` — the whole batch of ``t`` or a run of its graphs whose first node is ``n0``."""
    from . import attribution, cpu_route
    n1 = n0 + batch.total_nodes
    table = t.table if t.table.dim() == 2 else t.table[n0:n1]
    if t.cpu:
        return cpu_route.block_attributions(batch.blocks, t.fx[n0:n1], table, want_nodes, want_graphs)
    return attribution.block_attributions(batch.blocks, t.fx[n0:n1], table, None if t.cnt is None else t.cnt[n0:n1], want_nodes, want_graphs)


@dataclass
class GraphExplanations:
    """The outputs of the ``G`` graphs of a batch, decomposed: ``by_graph[g, k, d, c]`` is what feature ``k`` at hop ``hops[d]``
    (``hops[-1] = inf``: the unreachable pairs) adds to channel ``c`` of graph ``g``'s output before a read-out — graph ``g``'s
    ``Explanation.graph_by_feature_distance``; ``output[g] = by_graph[g].sum((0, 1))``.  ``by_node_feature_distance[j, k, d, c]`` /
    ``by_node[j]``: the share of node ``j`` (``graph_of[j]`` names its graph, ``node_off`` the graphs' first nodes) in ITS graph's
    output; None under ``by_node=False``.  With a NAM read-out (``models.TensorGNAN``): ``hidden [G, F]``, ``hidden_by_node [N, F]``
    and ``readout_by_feature[g, k] = g_k(hidden[g, k])``, whose sum over ``k`` is the model's output for graph ``g``."""
    node_off: torch.Tensor
    graph_of: torch.Tensor
    hops: torch.Tensor
    by_graph: torch.Tensor
    output: torch.Tensor
    by_node_feature_distance: Optional[torch.Tensor] = None
    by_node: Optional[torch.Tensor] = None
    hidden: Optional[torch.Tensor] = None
    hidden_by_node: Optional[torch.Tensor] = None
    readout_by_feature: Optional[torch.Tensor] = None


@torch.no_grad()
def explain_graphs(model, batch, by_node: bool = True) -> GraphExplanations:
    """Every graph of ``batch`` (:class:`GraphBatch`; for ``batched.TensorGNAN`` also what its forward takes: ``(x_batch, HopBlocks
    or dense dist_batch, batch_vector)``) explained in one pass — the model in ``eval()`` mode.  A module on the GPU runs
    ``gnan_attr_blocks``: the launches do not grow with the number of graphs; a module that lives on the CPU, with a CPU batch,
    runs ``cpu_route.block_attributions``.  Covers graph-level ``TensorGNAN`` modules and ``batched.TensorGNAN``.  The per-node
    result's bytes grow as ``N * F * D * C``: ``attribution.ATTR_MAX_BYTES`` bounds them, pass the graphs in batches beyond
    (:meth:`GraphBatch.graphs`) or ask for ``by_node=False``."""
    from . import cpu_route
    from .modules import TensorGNAN
    t = _graph_terms(model, batch, "explain_graphs")
    batch = t.batch
    G, N, D, F, C = batch.n_graphs, batch.total_nodes, batch.n_codes, t.F, t.C
    dev = batch.x.device
    B, T = _block_terms(t, batch, 0, by_node, True)
    by_graph = T.view(G, D, F, C).permute(0, 2, 1, 3).contiguous()            # [G, F, D, C]
    sizes = torch.tensor(batch.sizes, dtype=torch.int64)
    node_off = torch.zeros(G + 1, dtype=torch.int64)
    torch.cumsum(sizes, 0, out=node_off[1:])
    graph_of = torch.repeat_interleave(torch.arange(G), sizes).to(dev)
    out = GraphExplanations(node_off.to(dev), graph_of, _hops(D, dev), by_graph, by_graph.sum(dim=2).sum(dim=1))
    if by_node:
        out.by_node_feature_distance = B.view(N, D, F, C).permute(0, 2, 1, 3).contiguous()          # [N, F, D, C]
        out.by_node = out.by_node_feature_distance.sum(dim=2).sum(dim=1)
    if isinstance(model, TensorGNAN) and model.readout_n_layers > 0:
        nam = model.readout_nam
        out.hidden = by_graph.sum(dim=2).view(G, F)                           # models.py:379, every graph's row
        if by_node:
            out.hidden_by_node = out.by_node_feature_distance.sum(dim=2).view(N, F)
        stacked = nam._stacked("fs", nam.fs)
        gk = cpu_route.shape_functions(out.hidden, stacked, False) if t.cpu \
            else feature_mlps(out.hidden.contiguous(), stacked, sum_features=False)             # ONE call on [G, F]
        out.readout_by_feature = gk.view(G, F, -1)
    return out


@dataclass
class GraphImportance:
    """The moments of :class:`GraphExplanations`' ``by_graph`` over the GRAPHS of each group: ``mean``, ``mean_abs`` and ``rms``
    ``[Gr, F, D, C]``; ``feature_mean``, ``feature_mean_abs``, ``feature_rms`` ``[Gr, F, C]`` the same of a feature's total over the
    distances.  ``group_labels [Gr]``: the distinct labels, ascending; ``count [Gr]``: the graphs of each.  All float64.
    ``mean * count`` summed over ``(k, d)`` is the sum of the group's outputs before a read-out."""
    group_labels: torch.Tensor
    count: torch.Tensor
    hops: torch.Tensor
    mean: torch.Tensor
    mean_abs: torch.Tensor
    rms: torch.Tensor
    feature_mean: torch.Tensor
    feature_mean_abs: torch.Tensor
    feature_rms: torch.Tensor


@torch.no_grad()
def importance_graphs(model, batch, groups=None, max_nodes_per_pass: int = IMPORTANCE_NODES_PER_PASS) -> GraphImportance:
    """Which feature at which distance matters over the graphs of ``batch``, optionally apart by ``groups`` — one integer label per
    graph, the class for example.  The per-node terms are never stored: ``gnan_attr_blocks`` gives the per-graph sums alone, over
    runs of consecutive graphs of at most ``max_nodes_per_pass`` nodes (a larger graph is a run of its own; a graph's bits do not
    depend on the run it falls into); the moments are formed in float64 on the ``G * F * D * C`` numbers.  Model cover and refusals
    as :func:`explain_graphs`."""
    t = _graph_terms(model, batch, "importance_graphs")
    batch = t.batch
    G, D, F, C = batch.n_graphs, batch.n_codes, t.F, t.C
    dev = batch.x.device
    lab = torch.zeros(G, dtype=torch.int64, device=dev) if groups is None else \
        torch.as_tensor(list(groups) if not torch.is_tensor(groups) else groups).to(device=dev, dtype=torch.int64).view(-1)
    if lab.numel() != G:
        raise ValueError(f"groups must hold one label per graph ({G}), got {lab.numel()}")
    parts, g0, n0 = [], 0, 0
    while g0 < G:
        g1, nodes = g0, 0
        while g1 < G and (g1 == g0 or nodes + batch.sizes[g1] <= max_nodes_per_pass):
            nodes += batch.sizes[g1]
            g1 += 1
        run = batch if (g0, g1) == (0, G) else batch.graphs(g0, g1)
        parts.append(_block_terms(t, run, n0, False, True)[1])
        g0, n0 = g1, n0 + nodes
    T = torch.cat(parts, dim=0) if len(parts) > 1 else parts[0]
    a = T.view(G, D, F, C).permute(0, 2, 1, 3).double()                       # [G, F, D, C]
    a = torch.cat([a, a.sum(dim=2, keepdim=True)], dim=2)                     # slot D: a feature's total over the distances
    labels, who, count = torch.unique(lab, sorted=True, return_inverse=True, return_counts=True)
    M = torch.zeros((labels.numel(), 3, F, D + 1, C), dtype=torch.float64, device=dev)
    for j, v in enumerate((a, a.abs(), a * a)):
        M[:, j].index_add_(0, who, v)
    n = count.double().clamp_min(1.0).view(-1, 1, 1, 1)
    mean, mean_abs, rms = M[:, 0] / n, M[:, 1] / n, (M[:, 2] / n).sqrt()
    return GraphImportance(labels, count.double(), _hops(D, dev).double(), mean[:, :, :D].contiguous(), mean_abs[:, :, :D].contiguous(),
                           rms[:, :, :D].contiguous(), mean[:, :, D].contiguous(), mean_abs[:, :, D].contiguous(), rms[:, :, D].contiguous())
