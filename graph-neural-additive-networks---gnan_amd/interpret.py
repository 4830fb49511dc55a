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
storing a term per row."""
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
