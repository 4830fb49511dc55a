"""One-launch forward and backward of SMALL dense-coded graphs (``csrc/small_graph.hip``, ``csrc/small_graph_nam.hip``,
``csrc/mid_graph.hip``, ``csrc/mid_graph_nam.hip``) — what a graph-level task feeds per step (trainer.py:23-86 with
``batch_size = 1``; SURVEY.md section 8d C2: 30 nodes on average).

* :func:`small_graph_forward` — features summed per node, rho on the distinct distances (or, ``use_cnt="pre"``, on the n x D
  normalised distances of GNAN.py:65-67), the normalised aggregation and the graph read-out: GNAN.py:55-79 / 146-172,
  models.py:358-384 with ``readout_n_layers == 0``;
* :func:`mid_graph_forward` — the same for graphs of 129 to 448 nodes, over tiles of 64 rows (pre-rho: behind ``MID_GRAPH_PRE_RHO``);
* :func:`small_graph_nam_forward` — the NAM read-out over the per-feature aggregates (models.py:379-381) on graphs of up to 128 nodes;
* :func:`mid_graph_nam_forward` — the same read-out for graphs of 129 to 448 nodes: one launch forward, two backward, over tiles of
  64 rows, no workgroup waiting for another (behind ``MID_GRAPH_NAM``).

All are autograd nodes whose backward pass is one launch as well (the first two are ONE node, :class:`_OneLaunch`, told its route;
the last one's backward is two launches in stream order).
The general kernels (``functional``) take everything these do not cover; the ``*_applies`` predicates say which is which: each
is the shared test of the graph (:func:`_graph_ok`) and of the MLP stacks (:func:`_stack_ok`) with the route's limits, which stand
next to it.  The library's copy of the same limits: the ``RouteLimits`` next to each route's entry points.
"""
from __future__ import annotations

from typing import NamedTuple

import torch

from . import _lib
from . import aggregate
from . import functional as Fn
from .functional import StackedMLP
from .graph import HopGraph, hop_inputs

SMALL_GRAPH_FORWARD = True
SMALL_GRAPH_MAX_NODES = 128   # gnan_small_graph_fwd / _bwd: one block of 64 nodes (static LDS) or two (64 KB of tables)
SMALL_GRAPH_BACKWARD = True   # ... and its backward pass (gnan_small_graph_bwd)
SMALL_GRAPH_DROPOUT = True    # training-mode Dropout of the shape functions stays on these routes (gnan_*_graph_fwd_drop / _bwd_drop);
                              # off: such a forward takes the general kernels (functional.feature_mlps_dropout), as before
_SMALL_WS = {}               # (device index, stream) -> workspace whose counter word the kernel leaves zero
_MAX_HIDDEN, _MAX_CHANNELS = 64, 8     # every route's MLP kernels: hidden width, output channels
_FORWARD_CODES = 256         # hop codes gnan_small_graph_fwd / gnan_small_batch_fwd take ...
_ONE_LAUNCH_CODES = 64       # ... and the one-launch backward passes, pre-rho, the NAM and the mid route: a lane per shell


def _graph_ok(x, g, lo: int, hi: int, max_codes: int) -> bool:
    """A dense-coded graph of ``lo`` to ``hi`` nodes and at most ``max_codes`` codes; its features float32 on the device, their
    gradient not wanted."""
    return bool(g.is_dense and x.is_cuda and x.dtype == torch.float32 and not x.requires_grad and lo <= x.shape[0] <= hi
                and g.n_rows == g.n_cols == x.shape[0] and g.n_codes <= max_codes)


def _stack_ok(m: StackedMLP, max_c: int = _MAX_CHANNELS, depths=(2, 3)) -> bool:
    """These stacked MLPs are float32 with L, H, C inside the kernels' cover (``L == 1``: a Linear(1, C), no hidden width)."""
    return bool(m.L in depths and (m.L == 1 or 1 <= m.H <= _MAX_HIDDEN) and 1 <= m.C <= max_c
                and all(t is None or t.dtype == torch.float32 for t in m[:6]))


def small_graph_applies(x: torch.Tensor, g: HopGraph, f: StackedMLP, rho: StackedMLP, pre_rho: bool = False) -> bool:
    """Can ``gnan_small_graph_fwd`` take this forward (features summed per node; post-rho normalisation, or — ``pre_rho`` — the
    stand-alone file's rho(distance / shell size), GNAN.py:65-67, with a one-channel rho and at most 64 shells)?"""
    if pre_rho and not (g.cnt is not None and rho.C == 1 and g.n_codes <= _ONE_LAUNCH_CODES and SMALL_GRAPH_BACKWARD):
        return False
    return bool(SMALL_GRAPH_FORWARD and _graph_ok(x, g, 1, SMALL_GRAPH_MAX_NODES, _FORWARD_CODES) and x.shape[1] == f.F
                and rho.F == 1 and _stack_ok(f) and _stack_ok(rho) and rho.C in (1, f.C))


def _small_mlp(keep, L, H, C) -> "_lib.SmallMlp":
    w_mid = None if keep[2] is None else keep[2][0]
    b_mid = None if keep[3] is None else keep[3][0]
    return _lib.SmallMlp(L=L, H=H, C=C, w_first=_lib.ptr(keep[0]), b_first=_lib.ptr(keep[1]), w_mid=_lib.ptr(w_mid),
                         b_mid=_lib.ptr(b_mid), w_last=_lib.ptr(keep[4]), b_last=_lib.ptr(keep[5]))


def _mlp_grads(o, L: int = 2) -> "_lib.SmallMlpGrads":
    """Where the gradients of one stack go (``Fn._grad_outputs``); ``L == 1``: the NAM read-out's Linear(1, C) has a last layer only."""
    if L == 1:
        return _lib.SmallMlpGrads(w_first=None, b_first=None, w_mid=None, b_mid=None, w_last=_lib.ptr(o[4]), b_last=_lib.ptr(o[5]))
    return _lib.SmallMlpGrads(w_first=_lib.ptr(o[0]), b_first=_lib.ptr(o[1]), w_mid=None if o[2] is None else _lib.ptr(o[2][0]),
                              b_mid=None if o[3] is None else _lib.ptr(o[3][0]), w_last=_lib.ptr(o[4]), b_last=_lib.ptr(o[5]))


def _kept(tensors) -> list:
    """Detached contiguous copies (None stays None): what the kernels read."""
    return [None if t is None else Fn._c(t.detach()) for t in tensors]


def _cnt_pair(cnt) -> dict:
    """The ``cnt`` / ``cnt_stride`` fields of every argument struct."""
    return dict(cnt=_lib.ptr(cnt), cnt_stride=0 if cnt is None else cnt.stride(0))


def _save(ctx, lead, params) -> None:
    """Save ``lead`` and the parameters that exist; remember which do and where their gradients go."""
    ctx.present = [t is not None for t in params]
    ctx.dests = Fn._grad_dests_of(params)
    ctx.save_for_backward(*lead, *[t for t in params if t is not None])


def _saved(ctx, n_lead: int):
    """``(lead, params)`` as :func:`_save` took them: the absent parameters are None again."""
    saved = list(ctx.saved_tensors)
    rest = saved[n_lead:]
    return saved[:n_lead], [rest.pop(0) if pr else None for pr in ctx.present]


def _workspace(dev, need: int) -> torch.Tensor:
    """The kernels' counter + scratch: zero-filled, left zero by every launch, one per (device, stream) — or the captured step's."""
    if torch.cuda.is_current_stream_capturing():
        # a captured step owns its workspace: zeroed eagerly BEFORE the capture (graphed.GraphedCallable) — every capture
        # runs on the framework's one capture stream, so a buffer keyed by stream would be shared by all captured steps,
        # and one allocated inside a capture would have its zero fill recorded, never run
        ws = Fn.CAPTURE_SCRATCH
        if ws is None or (ws.numel() - Fn.ARRIVE_SLOTS) * 4 < need:      # (its last words are arrival counters)
            ws = torch.zeros(need // 4 + 1, dtype=torch.int32, device=dev)     # (recorded fill: runs at every replay)
        return ws
    key = (dev.index, torch.cuda.current_stream(dev).cuda_stream)
    ws = _SMALL_WS.get(key)
    if ws is None or ws.numel() * 4 < need:
        ws = _SMALL_WS[key] = torch.zeros(max(need // 4 + 1, 1 << 16), dtype=torch.int32, device=dev)
    return ws


class _Route(NamedTuple):
    """What tells the two one-launch routes of :class:`_OneLaunch` apart."""
    name: str            # the library's entry points ``<name>_fwd`` / ``_bwd`` and ``<name>_workspace_bytes`` / ``_bwd_workspace_bytes``
    args: type           # ... and their argument structs
    bwd_args: type
    flag: str            # the struct field that says pre-rho (the mid route's ``reserved``: 1 = ``GNAN_MID_PRE_RHO``)
    bwd_borrows: bool    # the backward always takes a workspace (else only under pre-rho)
    pre_bwd_ws: str      # the query of the backward's workspace under pre-rho (rho's partial gradients in slots)


_SMALL = _Route("gnan_small_graph", _lib.SmallGraphArgs, _lib.SmallGraphBwdArgs, "pre_rho", False,
                "gnan_small_graph_bwd_workspace_bytes")
_MID = _Route("gnan_mid_graph", _lib.MidGraphArgs, _lib.MidGraphBwdArgs, "reserved", True,
              "gnan_mid_graph_pre_bwd_workspace_bytes")


class _OneLaunch(torch.autograd.Function):
    """``Y`` (``[n, C]``) or its sum over the nodes (``[C, 1]``, ``graph_sum``) by ONE launch of ``route``'s forward; backward: one
    launch too (``gnan_small_graph_bwd`` / ``gnan_mid_graph_bwd``: one rho channel, <= 64 shells, the gradients of both f and rho
    wanted — or pre-rho), else the general path's kernels on the saved node sums and rho table — transposed aggregation, table
    gradient, the two small-batch MLP backward launches (their gradients land in the flat gradient buffers directly).
    ``use_cnt``: False / True (post-rho shell normalisation) / ``"pre"`` (GNAN.py:65-67: the rows' table ``[n, D]`` is saved, and the
    backward is the one launch or an error).
    ``dropout``: None, or ``(p, seed)`` — training-mode Dropout behind every hidden ReLU of f (never of rho), masks hashed from
    the seed (csrc/dropout.hpp; node = row of ``x``, feature = its column): both launches go through the ``_drop`` entry points
    with the same record, and so does ``gnan_fmlp_bwd`` where the general backward runs.  ``seed`` an int: by value, the eager
    path.  A one-element device tensor: the seed's cell, read by the ``_drop_dev`` entry points (captured steps) — then the backward
    is the one launch or an error, never the general backward."""

    @staticmethod
    def forward(ctx, route, x, g, use_cnt, graph_sum, fm, rm, dropout, *params):
        Lf, Hf, Cf, F = fm
        Lr, Hr, Cr = rm
        xk = Fn._rows(x.detach())
        n, D = xk.shape[0], g.n_codes
        dev = xk.device
        keep = _kept(params)
        pre_rho = use_cnt == "pre"
        S = torch.empty((n, Cf), dtype=torch.float32, device=dev)
        lut = torch.empty((n * D if pre_rho else D, Cr), dtype=torch.float32, device=dev)
        Y = None if graph_sum else torch.empty((n, Cf), dtype=torch.float32, device=dev)
        Ysum = torch.empty(Cf, dtype=torch.float32, device=dev) if graph_sum else None
        ws = _workspace(dev, getattr(_lib.lib(), route.name + "_workspace_bytes")(n, F, Cf))
        a = route.args(x=_lib.ptr(xk), x_stride=xk.stride(0), n=n, F=F, f=_small_mlp(keep[:6], Lf, Hf, Cf),
                       rho=_small_mlp(keep[6:], Lr, Hr, Cr), code=_lib.ptr(g.code), D=D, **{route.flag: int(pre_rho)},
                       **_cnt_pair(g.cnt if use_cnt else None), S=_lib.ptr(S), lut=_lib.ptr(lut), Y=_lib.ptr(Y), Ysum=_lib.ptr(Ysum),
                       workspace=_lib.ptr(ws), workspace_bytes=ws.numel() * 4)
        _launch(route.name + "_fwd", a, dropout, xk)
        ctx.route, ctx.g, ctx.use_cnt, ctx.graph_sum, ctx.fm, ctx.rm, ctx.dropout = route, g, use_cnt, graph_sum, fm, rm, dropout
        _save(ctx, (xk, S, lut), params)
        return Ysum.view(-1, 1) if graph_sum else Y

    @staticmethod
    def backward(ctx, d_out):
        (x, S, lut), params = _saved(ctx, 3)
        route = ctx.route
        Lf, Hf, Cf, F = ctx.fm
        Lr, Hr, Cr = ctx.rm
        n, D = x.shape[0], ctx.g.n_codes
        need_f, need_r = any(ctx.needs_input_grad[8:14]), any(ctx.needs_input_grad[14:])      # (eight arguments, then f's six, rho's six)
        pre_rho = ctx.use_cnt == "pre"          # (the ``*_applies`` predicates admitted it only where the one launch below covers it)
        if not ((SMALL_GRAPH_BACKWARD and Cr == 1 and D <= _ONE_LAUNCH_CODES and d_out.dtype == torch.float32
                 and all(t is None or t.dtype == torch.float32 for t in params)) and ((need_f and need_r) or pre_rho)):
            if pre_rho:
                raise RuntimeError("the one-launch graph forward with pre-rho normalisation was taken where its backward "
                                   "does not apply (float32 parameters and output gradient expected)")
            if ctx.dropout is not None and torch.is_tensor(ctx.dropout[1]):
                raise RuntimeError("a one-launch forward under Dropout with its seed in a device cell was taken where the one-launch "
                                   "backward does not apply (the gradients of both f and rho, one rho channel, at most 64 shells, "
                                   "float32): the general backward takes its seed by value")
            return (None, *_general_backward(ctx, x, S, lut, params, d_out, need_f, need_r))
        # one launch: every workgroup forms the operand (or table) gradient it needs itself, then the small-batch MLP backward
        keep = _kept(params)
        outs_f, outs_r = Fn._grad_outputs(keep[:6], ctx.dests[:6]), Fn._grad_outputs(keep[6:], ctx.dests[6:])
        g_out = d_out.detach().contiguous()
        ws = None
        if route.bwd_borrows or pre_rho:
            query = route.pre_bwd_ws if pre_rho else route.name + "_bwd_workspace_bytes"
            ws = _workspace(x.device, getattr(_lib.lib(), query)(n, D))
        a = route.bwd_args(x=_lib.ptr(x), x_stride=x.stride(0), n=n, F=F, f=_small_mlp(keep[:6], Lf, Hf, Cf),
                           rho=_small_mlp(keep[6:], Lr, Hr, Cr), code=_lib.ptr(ctx.g.code), D=D, **{route.flag: int(pre_rho)},
                           **_cnt_pair(ctx.g.cnt if ctx.use_cnt else None), S=_lib.ptr(S), lut=_lib.ptr(lut),
                           dY=None if ctx.graph_sum else _lib.ptr(g_out), dYsum=_lib.ptr(g_out) if ctx.graph_sum else None,
                           df=_mlp_grads(outs_f), drho=_mlp_grads(outs_r), workspace=_lib.ptr(ws),
                           workspace_bytes=0 if ws is None else ws.numel() * 4)
        _launch(route.name + "_bwd", a, ctx.dropout, x)
        if not need_f:
            outs_f = [None] * 6
        if not need_r:
            outs_r = [None] * 6
        return (None, None, None, None, None, None, None, None, *outs_f, *outs_r)


def _launch(entry: str, a, dropout, on: torch.Tensor) -> None:
    """``entry(a, stream)``, or — ``dropout = (p, seed)`` — ``entry_drop(a, record, stream)`` for a seed by value (an int: the eager
    path) and ``entry_drop_dev`` for a seed cell (a one-element device tensor: what a capture may record)."""
    if dropout is None:
        _lib.check(getattr(_lib.lib(), entry)(a, _lib.stream_of(on)), entry)
        return
    if torch.is_tensor(dropout[1]):
        d = _lib.SmallDropoutDev(p=float(dropout[0]), reserved=0, seed=_lib.ptr(dropout[1]))
        _lib.check(getattr(_lib.lib(), entry + "_drop_dev")(a, d, _lib.stream_of(on)), entry + "_drop_dev")
        return
    d = _lib.SmallDropout(p=float(dropout[0]), reserved=0, seed=int(dropout[1]))
    _lib.check(getattr(_lib.lib(), entry + "_drop")(a, d, _lib.stream_of(on)), entry + "_drop")


def seed_cell(device) -> torch.Tensor:
    """A Dropout seed's device cell (one ``int64`` word, 0 until :func:`seed_cell_set` writes it)."""
    return torch.zeros(1, dtype=torch.int64, device=device)


def seed_cell_set(cell: torch.Tensor, seed: int) -> None:
    """Store ``seed`` (its 64 bits) in ``cell`` — one tiny launch (``gnan_dropout_seed_set``) on the current stream."""
    _lib.check(_lib.lib().gnan_dropout_seed_set(_lib.ptr(cell), int(seed) & ((1 << 64) - 1), _lib.stream_of(cell)),
               "gnan_dropout_seed_set")


def _general_backward(ctx, x, S, lut, params, d_out, need_f, need_r):
    """The backward of a one-launch forward by the general path's kernels on the node sums and the rho table it saved.  A forward
    under Dropout: f's gradients by ``gnan_fmlp_bwd`` with the forward's ``(p, seed)`` — the same masks — never a Dropout-free
    formula."""
    fp, rp = params[:6], params[6:]
    Lf, Hf, Cf, F = ctx.fm
    Lr, Hr, Cr = ctx.rm
    n = x.shape[0]
    dY = d_out.reshape(1, Cf).expand(n, Cf).contiguous() if ctx.graph_sum else d_out.contiguous()
    call = aggregate.AggregateCall(ctx.g, ctx.use_cnt, with_rest=False)
    dS, dlut = aggregate._aggregate_backward(call, S, lut, dY, need_f, need_r)
    pg_f = pg_r = [None] * 6
    if need_f and ctx.dropout is not None and ctx.dropout[0] > 0:
        pg_f = Fn._fmlp_backward_launch(x, fp, dS, True, Lf, Hf, Cf, F, dropout=ctx.dropout, dests=ctx.dests[:6])
    elif need_f:
        _, pg_f = Fn._shape_function_grads(x, fp, ctx.present[:6], None, dS, True, Lf, Hf, Cf, F, dests=ctx.dests[:6])
    if need_r:
        u = hop_inputs(ctx.g.n_codes, x.device).view(-1, 1)
        _, pg_r = Fn._shape_function_grads(u, rp, ctx.present[6:], None, dlut.reshape(-1, Cr), False, Lr, Hr, Cr, 1,
                                        dests=ctx.dests[6:])
    return (None, None, None, None, None, None, None, *pg_f, *pg_r)


def _dropout_record(dropout):
    """``None`` or ``(p, seed)`` as :class:`_OneLaunch` takes it: p in [0, 1), and the seed's 64 bits — or its cell, a
    one-element ``int64`` / ``uint64`` device tensor (the ``_dev`` entry points)."""
    if dropout is None:
        return None
    p, seed = float(dropout[0]), dropout[1]
    if not 0.0 <= p < 1.0:
        raise ValueError("dropout p must be in [0, 1)")
    if torch.is_tensor(seed):
        if not (seed.is_cuda and seed.numel() == 1 and seed.dtype in (torch.int64, torch.uint64) and seed.is_contiguous()):
            raise ValueError("a dropout seed cell is a one-element int64 / uint64 device tensor")
        return (p, seed)
    return (p, int(seed) & ((1 << 64) - 1))


def small_graph_forward(x: torch.Tensor, g: HopGraph, f: StackedMLP, rho: StackedMLP, use_cnt, graph_sum: bool, dropout=None):
    """The forward of GNAN.py:146-172 / models.py:358-384 (post-rho; ``use_cnt="pre"``: GNAN.py:55-79, pre-rho) on a small
    dense-coded graph by ``gnan_small_graph_fwd``: ``[n, C]`` node outputs, or ``[C, 1]`` with ``graph_sum`` (GNAN.py:75-79).
    ``dropout = (p, seed)``: training-mode Dropout of f (``gnan_small_graph_fwd_drop``; ``functional.draw_dropout_seed``)."""
    _lib.require_device(x, f.w_last, rho.w_last, g.code)
    return _OneLaunch.apply(_SMALL, x, g, "pre" if use_cnt == "pre" else bool(use_cnt), bool(graph_sum), (f.L, f.H, f.C, f.F),
                            (rho.L, rho.H, rho.C), _dropout_record(dropout), *f[:6], *rho[:6])


# =============================================================================
# 129 to 448 nodes: the same forward and backward, one launch each, over tiles of 64 rows (csrc/mid_graph.hip)
# =============================================================================
MID_GRAPH = True
MID_GRAPH_MIN_NODES = SMALL_GRAPH_MAX_NODES + 1
MID_GRAPH_MAX_NODES = 448     # gnan_mid_graph_fwd / _bwd: seven row tiles (the largest Mutagenicity graph has 417 nodes, datasets.py:123-129)


def mid_graph_applies(x: torch.Tensor, g: HopGraph, f: StackedMLP, rho: StackedMLP, use_cnt=True) -> bool:
    """Can ``gnan_mid_graph_fwd`` take this forward: a dense-coded graph of 129 to 448 nodes, features summed per node, post-rho
    shell normalisation or none (not ``use_cnt="pre"``), a one-channel rho, at most 64 shells?"""
    if use_cnt == "pre" or (use_cnt and g.cnt is None):
        return False
    return bool(MID_GRAPH and SMALL_GRAPH_FORWARD and _graph_ok(x, g, MID_GRAPH_MIN_NODES, MID_GRAPH_MAX_NODES, _ONE_LAUNCH_CODES)
                and x.shape[1] == f.F and rho.F == 1 and _stack_ok(f) and _stack_ok(rho, max_c=1))


MID_GRAPH_PRE_RHO = True      # pre-rho normalisation (GNAN.py:65-67, the stand-alone class's default) on this route: ``reserved =
                              # GNAN_MID_PRE_RHO``.  On by the measured rule of DESIGN.md section 5: the replayed one-launch step beats the
                              # general route's at 130, 200 and 417 nodes by far more than the latter's spread (5 kernels against 25)


def mid_graph_pre_rho_applies(x: torch.Tensor, g: HopGraph, f: StackedMLP, rho: StackedMLP) -> bool:
    """Can ``gnan_mid_graph_fwd`` / ``_bwd`` with ``reserved = GNAN_MID_PRE_RHO`` take this forward AND its backward: what
    :func:`mid_graph_applies` asks of graph and stacks, the shell sizes, a one-channel rho, the one-launch backward (a pre-rho forward
    has no other) and the route's switch?"""
    return bool(MID_GRAPH_PRE_RHO and MID_GRAPH and SMALL_GRAPH_FORWARD and SMALL_GRAPH_BACKWARD and g.cnt is not None
                and _graph_ok(x, g, MID_GRAPH_MIN_NODES, MID_GRAPH_MAX_NODES, _ONE_LAUNCH_CODES) and x.shape[1] == f.F and rho.F == 1
                and rho.C == 1 and _stack_ok(f) and _stack_ok(rho, max_c=1))


def mid_graph_forward(x: torch.Tensor, g: HopGraph, f: StackedMLP, rho: StackedMLP, use_cnt, graph_sum: bool, dropout=None):
    """:func:`small_graph_forward` for a dense-coded graph of 129 to 448 nodes (``gnan_mid_graph_fwd`` / ``_fwd_drop``): ``[n, C]``
    node outputs, or ``[C, 1]`` with ``graph_sum``.  ``use_cnt="pre"``: GNAN.py:65-67 (:func:`mid_graph_pre_rho_applies`)."""
    _lib.require_device(x, f.w_last, rho.w_last, g.code)
    return _OneLaunch.apply(_MID, x, g, "pre" if use_cnt == "pre" else bool(use_cnt), bool(graph_sum), (f.L, f.H, f.C, f.F),
                            (rho.L, rho.H, rho.C), _dropout_record(dropout), *f[:6], *rho[:6])


# =============================================================================
# ... with a NAM read-out over the per-feature aggregates (csrc/small_graph_nam.hip)
# =============================================================================
def _nam_mlp(keep, L, H, C) -> "_lib.SmallMlp":
    if L == 1:                                       # Linear(1, C) per feature: w_last [F, C]
        return _lib.SmallMlp(L=1, H=0, C=C, w_first=None, b_first=None, w_mid=None, b_mid=None, w_last=_lib.ptr(keep[4]),
                             b_last=_lib.ptr(keep[5]))
    return _small_mlp(keep, L, H, C)


SMALL_GRAPH_NAM_MAX_FEATURES = 127   # the backward's workgroups (one per feature + rho's) must be resident together (csrc/small_graph_nam.hip)


def small_graph_nam_applies(x: torch.Tensor, g: HopGraph, f: StackedMLP, rho: StackedMLP, nam: StackedMLP) -> bool:
    """Can ``gnan_small_graph_nam_fwd`` / ``_bwd`` take this graph-level forward with a NAM read-out?"""
    return bool(_graph_ok(x, g, 1, SMALL_GRAPH_MAX_NODES, _ONE_LAUNCH_CODES) and x.shape[1] == f.F == nam.F
                and f.F <= SMALL_GRAPH_NAM_MAX_FEATURES and rho.F == 1 and _stack_ok(f, max_c=1) and _stack_ok(rho, max_c=1)
                and _stack_ok(nam, depths=(1, 2, 3)))


class _SmallGraphNam(torch.autograd.Function):
    """``out [C, 1] = sum_k nam_k(sum_ij w_ij f_k(x_jk))`` by ONE launch; backward: one launch as well."""

    @staticmethod
    def forward(ctx, x, g, use_cnt, fm, rm, nm, *params):
        Lf, Hf, F = fm
        Lr, Hr = rm
        Ln, Hn, Cn = nm
        xk = Fn._rows(x.detach())
        n, D, dev = xk.shape[0], g.n_codes, xk.device
        keep = _kept(params)
        fx = torch.empty((F, n), dtype=torch.float32, device=dev)
        lut = torch.empty(D, dtype=torch.float32, device=dev)
        hidden = torch.empty(F, dtype=torch.float32, device=dev)
        out = torch.empty(Cn, dtype=torch.float32, device=dev)
        ws = _workspace(dev, _lib.lib().gnan_small_graph_nam_workspace_bytes(F, Cn))
        a = _lib.SmallGraphNamArgs(x=_lib.ptr(xk), x_stride=xk.stride(0), n=n, F=F, f=_small_mlp(keep[:6], Lf, Hf, 1),
                                   rho=_small_mlp(keep[6:12], Lr, Hr, 1), nam=_nam_mlp(keep[12:], Ln, Hn, Cn),
                                   code=_lib.ptr(g.code), D=D, reserved=0, **_cnt_pair(g.cnt if use_cnt else None), fx=_lib.ptr(fx),
                                   lut=_lib.ptr(lut), hidden=_lib.ptr(hidden), out=_lib.ptr(out), workspace=_lib.ptr(ws),
                                   workspace_bytes=ws.numel() * 4)
        _lib.check(_lib.lib().gnan_small_graph_nam_fwd(a, _lib.stream_of(xk)), "gnan_small_graph_nam_fwd")
        ctx.g, ctx.use_cnt, ctx.fm, ctx.rm, ctx.nm = g, use_cnt, fm, rm, nm
        _save(ctx, (xk, fx, lut, hidden), params)
        return out.view(-1, 1)

    @staticmethod
    def backward(ctx, d_out):
        (x, fx, lut, hidden), params = _saved(ctx, 4)
        Lf, Hf, F = ctx.fm
        Lr, Hr = ctx.rm
        Ln, Hn, Cn = ctx.nm
        n, dev = x.shape[0], x.device
        keep = _kept(params)
        outs = [Fn._grad_outputs(keep[i:i + 6], ctx.dests[i:i + 6]) for i in (0, 6, 12)]
        g_out = d_out.detach().to(torch.float32).contiguous().view(-1)
        ws = _workspace(dev, _lib.lib().gnan_small_graph_nam_workspace_bytes(F, Cn))
        a = _lib.SmallGraphNamBwdArgs(x=_lib.ptr(x), x_stride=x.stride(0), n=n, F=F, f=_small_mlp(keep[:6], Lf, Hf, 1),
                                      rho=_small_mlp(keep[6:12], Lr, Hr, 1), nam=_nam_mlp(keep[12:], Ln, Hn, Cn),
                                      code=_lib.ptr(ctx.g.code), D=ctx.g.n_codes, reserved=0,
                                      **_cnt_pair(ctx.g.cnt if ctx.use_cnt else None), fx=_lib.ptr(fx), lut=_lib.ptr(lut),
                                      hidden=_lib.ptr(hidden), d_out=_lib.ptr(g_out), df=_mlp_grads(outs[0], Lf),
                                      drho=_mlp_grads(outs[1], Lr), dnam=_mlp_grads(outs[2], Ln), workspace=_lib.ptr(ws),
                                      workspace_bytes=ws.numel() * 4)
        _lib.check(_lib.lib().gnan_small_graph_nam_bwd(a, _lib.stream_of(x)), "gnan_small_graph_nam_bwd")
        flat = []
        for i, o in zip((0, 6, 12), outs):
            need = ctx.needs_input_grad[6 + i:12 + i]
            flat += [v if nd else None for v, nd in zip(o, need)]
        return (None, None, None, None, None, None, *flat)


def small_graph_nam_forward(x: torch.Tensor, g: HopGraph, f: StackedMLP, rho: StackedMLP, nam: StackedMLP, use_cnt: bool):
    """models.py:358-384 with ``is_graph_task`` and ``readout_n_layers > 0`` on a small dense-coded graph: ``[C, 1]``."""
    _lib.require_device(x, f.w_last, rho.w_last, nam.w_last, g.code)
    return _SmallGraphNam.apply(x, g, bool(use_cnt), (f.L, f.H, f.F), (rho.L, rho.H), (nam.L, nam.H, nam.C),
                                *f[:6], *rho[:6], *nam[:6])


# =============================================================================
# ... for graphs of 129 to 448 nodes: one launch forward, two backward, over tiles of 64 rows (csrc/mid_graph_nam.hip)
# =============================================================================
MID_GRAPH_NAM = True          # the route's switch, read at every call.  Off: such a forward takes the general kernels (table, operand,
                              # rho_aggregate, gnan_colsum, the read-out's MLPs), as before.  On by the measured rule of DESIGN.md section
                              # 5 (tools/mid_graph_nam_time.py): the replayed step beats the general route's at 130, 200 and 417 nodes by
                              # 35 to 155 times the latter's spread (6 kernels against 28 with a one-layer read-out, 39 with two layers)


def mid_graph_nam_applies(x: torch.Tensor, g: HopGraph, f: StackedMLP, rho: StackedMLP, nam: StackedMLP, use_cnt=True) -> bool:
    """Can ``gnan_mid_graph_nam_fwd`` / ``_bwd`` take this graph-level forward with a NAM read-out: a dense-coded graph of 129 to 448
    nodes and at most 64 shells, one-wide f and rho, the read-out by the rules of :func:`small_graph_nam_applies` — and any number of
    features: no workgroup of these kernels waits for another.  ``use_cnt`` without the graph's shell sizes does not apply."""
    if use_cnt and g.cnt is None:
        return False
    return bool(MID_GRAPH_NAM and _graph_ok(x, g, MID_GRAPH_MIN_NODES, MID_GRAPH_MAX_NODES, _ONE_LAUNCH_CODES)
                and x.shape[1] == f.F == nam.F and rho.F == 1 and _stack_ok(f, max_c=1) and _stack_ok(rho, max_c=1)
                and _stack_ok(nam, depths=(1, 2, 3)))


class _MidGraphNam(torch.autograd.Function):
    """:class:`_SmallGraphNam` by ``gnan_mid_graph_nam_fwd`` (one launch) and ``gnan_mid_graph_nam_bwd`` (two launches, stream-ordered):
    the forward also leaves ``colw [n]``, the column sums the backward reads."""

    @staticmethod
    def forward(ctx, x, g, use_cnt, fm, rm, nm, *params):
        Lf, Hf, F = fm
        Lr, Hr = rm
        Ln, Hn, Cn = nm
        xk = Fn._rows(x.detach())
        n, D, dev = xk.shape[0], g.n_codes, xk.device
        keep = _kept(params)
        fx = torch.empty((F, n), dtype=torch.float32, device=dev)
        lut = torch.empty(D, dtype=torch.float32, device=dev)
        hidden = torch.empty(F, dtype=torch.float32, device=dev)
        colw = torch.empty(n, dtype=torch.float32, device=dev)
        out = torch.empty(Cn, dtype=torch.float32, device=dev)
        ws = _workspace(dev, _lib.lib().gnan_mid_graph_nam_workspace_bytes(n, F, D, Cn))
        a = _lib.MidGraphNamArgs(x=_lib.ptr(xk), x_stride=xk.stride(0), n=n, F=F, f=_small_mlp(keep[:6], Lf, Hf, 1),
                                 rho=_small_mlp(keep[6:12], Lr, Hr, 1), nam=_nam_mlp(keep[12:], Ln, Hn, Cn),
                                 code=_lib.ptr(g.code), D=D, reserved=0, **_cnt_pair(g.cnt if use_cnt else None), fx=_lib.ptr(fx),
                                 lut=_lib.ptr(lut), hidden=_lib.ptr(hidden), out=_lib.ptr(out), workspace=_lib.ptr(ws),
                                 workspace_bytes=ws.numel() * 4, colw=_lib.ptr(colw))
        _lib.check(_lib.lib().gnan_mid_graph_nam_fwd(a, _lib.stream_of(xk)), "gnan_mid_graph_nam_fwd")
        ctx.g, ctx.use_cnt, ctx.fm, ctx.rm, ctx.nm = g, use_cnt, fm, rm, nm
        _save(ctx, (xk, fx, lut, hidden, colw), params)
        return out.view(-1, 1)

    @staticmethod
    def backward(ctx, d_out):
        (x, fx, lut, hidden, colw), params = _saved(ctx, 5)
        Lf, Hf, F = ctx.fm
        Lr, Hr = ctx.rm
        Ln, Hn, Cn = ctx.nm
        n, D, dev = x.shape[0], ctx.g.n_codes, x.device
        keep = _kept(params)
        outs = [Fn._grad_outputs(keep[i:i + 6], ctx.dests[i:i + 6]) for i in (0, 6, 12)]
        g_out = d_out.detach().to(torch.float32).contiguous().view(-1)
        ws = _workspace(dev, _lib.lib().gnan_mid_graph_nam_workspace_bytes(n, F, D, Cn))
        a = _lib.MidGraphNamBwdArgs(x=_lib.ptr(x), x_stride=x.stride(0), n=n, F=F, f=_small_mlp(keep[:6], Lf, Hf, 1),
                                    rho=_small_mlp(keep[6:12], Lr, Hr, 1), nam=_nam_mlp(keep[12:], Ln, Hn, Cn),
                                    code=_lib.ptr(ctx.g.code), D=D, reserved=0, **_cnt_pair(ctx.g.cnt if ctx.use_cnt else None),
                                    fx=_lib.ptr(fx), lut=_lib.ptr(lut), hidden=_lib.ptr(hidden), d_out=_lib.ptr(g_out),
                                    df=_mlp_grads(outs[0], Lf), drho=_mlp_grads(outs[1], Lr), dnam=_mlp_grads(outs[2], Ln),
                                    workspace=_lib.ptr(ws), workspace_bytes=ws.numel() * 4, colw=_lib.ptr(colw))
        _lib.check(_lib.lib().gnan_mid_graph_nam_bwd(a, _lib.stream_of(x)), "gnan_mid_graph_nam_bwd")
        flat = []
        for i, o in zip((0, 6, 12), outs):
            need = ctx.needs_input_grad[6 + i:12 + i]      # (six arguments, then f's six, rho's six, the read-out's six)
            flat += [v if nd else None for v, nd in zip(o, need)]
        return (None, None, None, None, None, None, *flat)


def mid_graph_nam_forward(x: torch.Tensor, g: HopGraph, f: StackedMLP, rho: StackedMLP, nam: StackedMLP, use_cnt: bool):
    """:func:`small_graph_nam_forward` for a dense-coded graph of 129 to 448 nodes (:func:`mid_graph_nam_applies`): ``[C, 1]``."""
    if use_cnt and g.cnt is None:
        raise _lib.GnanHipError("shell normalisation was asked for on a graph without shell sizes")
    _lib.require_device(x, f.w_last, rho.w_last, nam.w_last, g.code)
    return _MidGraphNam.apply(x, g, bool(use_cnt), (f.L, f.H, f.F), (rho.L, rho.H), (nam.L, nam.H, nam.C),
                              *f[:6], *rho[:6], *nam[:6])


# =============================================================================
# one graph in slots: a batch-size-1 loop through ONE captured step
# =============================================================================
SLOT_MAX_NODES = 128
SLOT_CODES = 64              # most hop codes slots are laid out for (hops 0 .. 62 + the rest code); what gnan_small_batch_bwd covers
SLOT_CODE_TIERS = (16, 32, 64)   # ... and the capacities a loop picks from: the kernels' work on tables and bins grows with the capacity
_SLOT_CNT = None             # TensorKeyedCache: a graph's shell sizes (object identity + version) -> their [n, SLOT_CODES] layout


class SlotGraph:
    """ONE small dense-coded graph held in device slots whose SIZE only the device knows (``node_off = [0, n]``,
    ``code_off = [0, n * n]``): what a captured step of a graph-level task reads (trainer.py:23-86 feeds one graph of another
    size per step).  The batched kernels (``gnan_small_batch_fwd`` / ``_bwd``: blockIdx.y = graph, sizes from the offset
    arrays) run it as a batch of one, with the shell sizes (``cnt``, ABI 42) and the reference's rho arguments — so ONE capture
    serves every graph of up to 128 nodes and 63 hops, instead of one capture per (nodes, features, shells) shape.
    ``cnt`` is laid out for the slots' ``n_codes`` codes whatever the graph's own largest hop: its listed hops keep their columns, its
    rest bucket (unreachable pairs, code 255) moves to the last column, the columns between are hops no pair has."""
    is_dense = True

    def __init__(self, n_features: int, device, use_cnt: bool = True, max_nodes: int = SLOT_MAX_NODES, n_codes: int = SLOT_CODES):
        """``max_nodes``: 64 or 128 — the kernels come in a one-block (64 nodes, static LDS) and a two-block build; 97 % of
        Mutagenicity-shaped graphs fit the first, which is the faster one."""
        from .batched import HopBlocks
        if max_nodes not in (64, 128) or not 2 <= n_codes <= SLOT_CODES:
            raise ValueError("graph slots hold 64 or 128 nodes and 2 to 64 hop codes")
        self.F, self.device, self.n_codes, self.max_nodes = int(n_features), torch.device(device), int(n_codes), int(max_nodes)
        self.x = torch.zeros((max_nodes, self.F), dtype=torch.float32, device=device)
        self.code = torch.full((max_nodes * max_nodes,), 255, dtype=torch.uint8, device=device)
        self.cnt = torch.ones((max_nodes, self.n_codes), dtype=torch.int32, device=device) if use_cnt else None
        self.node_off = torch.zeros(2, dtype=torch.int32, device=device)
        self.code_off = torch.zeros(2, dtype=torch.int64, device=device)
        self.blocks = HopBlocks(self.code, self.node_off, self.code_off, [0], self.n_codes - 2)
        self.blocks.total_nodes, self.blocks.max_nodes, self.blocks.min_nodes, self.blocks.slots = max_nodes, max_nodes, 1, True
        self._offs = {}

    def fits(self, graph: HopGraph, x: torch.Tensor) -> bool:
        return bool(graph.is_dense and 1 <= graph.n_rows == graph.n_cols <= self.max_nodes and graph.n_codes <= self.n_codes
                    and x.is_cuda and x.dtype == torch.float32 and tuple(x.shape) == (graph.n_rows, self.F)
                    and (self.cnt is None or graph.cnt is not None))

    def _cnt_layout(self, graph: HopGraph) -> torch.Tensor:
        global _SLOT_CNT
        if _SLOT_CNT is None:
            from ._cache import TensorKeyedCache
            _SLOT_CNT = TensorKeyedCache(1 << 16)
        hit = _SLOT_CNT.get((graph.cnt,), self.n_codes)
        if hit is None:
            D = graph.n_codes
            wide = torch.ones((graph.n_rows, self.n_codes), dtype=torch.int32, device=graph.cnt.device)
            wide[:, : D - 1] = graph.cnt[:, : D - 1]
            wide[:, self.n_codes - 1] = graph.cnt[:, D - 1]
            hit = _SLOT_CNT.put((graph.cnt,), self.n_codes, wide)
        return hit

    def load(self, graph: HopGraph, x: torch.Tensor, extra=()) -> None:
        """Copy a graph (that :meth:`fits`) into the slots — one launch (``gnan_multi_copy``); ``extra``: further (dst, src) pairs."""
        n = graph.n_rows
        offs = self._offs.get(n)
        if offs is None:
            offs = self._offs[n] = (torch.tensor([0, n], dtype=torch.int32, device=self.device),
                                    torch.tensor([0, n * n], dtype=torch.int64, device=self.device))
        pairs = [(self.x[:n], x), (self.code[: n * n], graph.code.reshape(-1)), (self.node_off, offs[0]), (self.code_off, offs[1])]
        if self.cnt is not None:
            pairs.append((self.cnt[:n], self._cnt_layout(graph)))
        pairs += list(extra)
        if all(sr.is_contiguous() and sr.dtype == d.dtype and sr.shape == d.shape and sr.is_cuda for d, sr in pairs) and len(pairs) <= 8:
            _lib.multi_copy(pairs)
            return
        for d, sr in pairs:
            d.copy_(sr)


SLOT_PRE_RHO = True          # on: the stand-alone class with its default pre-rho normalisation (GNAN.py:65-67) runs graph-level tasks through
                             # graph slots too (gnan_small_batch_pre_fwd / _bwd).  Off: such a model takes a captured step per graph shape,
                             # as before.  On by the measured rule of DESIGN.md section 5: the 4337-graph epoch's first two epochs are 20
                             # times shorter than the parent's, 4 captured steps instead of 451, 0.12 GB reserved instead of 2.06


SLOT_NAM_READOUT = False     # on: ``models.TensorGNAN`` with a NAM read-out (the class's default for graph tasks) runs graph-level tasks through
                             # graph slots too (gnan_small_slot_nam_fwd / _bwd).  Off: such a model takes a captured step per graph shape,
                             # as before.  Ships off by the measured rule of DESIGN.md section 5: the 4337-graph epoch's first two epochs
                             # are 16 to 35 times shorter than the parent's, 4 captured steps instead of 451, 0.11 GB reserved instead of
                             # 2.06 — but an existing test pins ``slot_mode(...) is None`` for this class, and the rule asks the whole
                             # existing suite to pass unchanged with the switch on


class SlotNamMode:
    """:func:`slot_mode`'s answer for a model that ends in a NAM read-out.  It is TRUE exactly where the shell sizes are used
    (``normalize_rho``): ``SlotGraph(use_cnt=mode)`` and ``harness`` read a mode's truth as "lay out ``cnt``"."""
    __slots__ = ("use_cnt",)

    def __init__(self, use_cnt: bool):
        self.use_cnt = bool(use_cnt)

    def __bool__(self) -> bool:
        return self.use_cnt

    def __eq__(self, other) -> bool:
        return isinstance(other, SlotNamMode) and other.use_cnt == self.use_cnt

    def __hash__(self) -> int:
        return hash(("nam", self.use_cnt))

    def __repr__(self) -> str:
        return f"SlotNamMode(use_cnt={self.use_cnt})"


def slot_mode(model):
    """``use_cnt`` (True / False / ``"pre"`` / a :class:`SlotNamMode`) of the slot forward this model can run, or None: the read-out
    of a graph-level task, a one-channel rho, features summed per node — ``models.TensorGNAN`` without a NAM read-out in its default
    order (post-rho normalisation or none), the stand-alone class without normalisation, — ``"pre"``, behind ``SLOT_PRE_RHO`` and
    with the one-launch backward on (a pre-rho forward has no other) — the stand-alone class with it, and — a ``SlotNamMode``, behind
    ``SLOT_NAM_READOUT`` and the one-launch backward — ``models.TensorGNAN`` WITH a NAM read-out (``readout_n_layers > 0``) in its
    default order, its f and rho one-wide and its read-out inside the cover of :func:`small_graph_nam_applies`.  The model's side is
    decided once per model; the switches (and the read-out model's order) are read at every call.
    Dropout: the read-out kernels draw no masks.  Under training-mode Dropout of f or of the read-out NAM nothing changes:
    :func:`dropout_capture_applies` refuses such a model whatever this function says, so its forwards run eagerly as before."""
    mode = model.__dict__.get("_slot_mode", "?")
    if mode == "?":
        import types
        from . import modules
        mode = None
        pre = isinstance(model, modules.StandaloneTensorGNAN) and bool(model.normalize_rho)
        nam = isinstance(model, modules.TensorGNAN) and bool(model.is_graph_task) and model.readout_n_layers > 0
        if (pre and not (SLOT_PRE_RHO and SMALL_GRAPH_BACKWARD)) or (nam and not (SLOT_NAM_READOUT and SMALL_GRAPH_BACKWARD)):
            return None                                  # (nothing decided, nothing touched: as before the switch)
        if nam:
            with torch.no_grad():
                f, rho = model._stacked("fs", model.fs), model._stacked("rho", [model.rho])
                readout = model.readout_nam._stacked("fs", model.readout_nam.fs)
            if slot_nam_applies(types.SimpleNamespace(F=f.F), f, rho, readout):
                mode = SlotNamMode(bool(model.normalize_rho))
        elif (isinstance(model, (modules.TensorGNAN, modules.StandaloneTensorGNAN)) and model.is_graph_task
                and not (isinstance(model, modules.TensorGNAN) and model.aggregation_order == "reference")):
            with torch.no_grad():
                f, rho = model._stacked("fs", model.fs), model._stacked("rho", [model.rho])
            if slot_graph_applies(types.SimpleNamespace(F=f.F), f, rho):
                mode = "pre" if pre else bool(model.normalize_rho)
        object.__setattr__(model, "_slot_mode", mode)
    if mode == "pre" and not (SLOT_PRE_RHO and SMALL_GRAPH_BACKWARD):
        return None
    if isinstance(mode, SlotNamMode) and not (SLOT_NAM_READOUT and SMALL_GRAPH_BACKWARD and model.aggregation_order == "sum_first"):
        return None
    return mode


def slot_tier(graph: HopGraph):
    """(node tier, hop-code tier) of the slots a dense-coded graph fits, or None."""
    if not graph.is_dense or graph.n_rows > SLOT_MAX_NODES or graph.n_codes > SLOT_CODES or graph.n_rows < 1:
        return None
    return (64 if graph.n_rows <= 64 else 128, next(c for c in SLOT_CODE_TIERS if graph.n_codes <= c))


def slot_graph_applies(slot: SlotGraph, f: StackedMLP, rho: StackedMLP) -> bool:
    """The stacks' side of ``gnan_small_batch_fwd`` / ``_bwd`` with shell sizes (the graph's side: :meth:`SlotGraph.fits`)."""
    return bool(f.F == slot.F and rho.F == 1 and _stack_ok(f) and _stack_ok(rho, max_c=1))


CAPTURE_DROPOUT = False      # on: forwards under training-mode Dropout may be captured (replay.py, graphed.py): their kernels read the
                             # seed from a device cell the host rewrites before every replay.  Off (the default): such forwards stay
                             # eager, as before.  Ships off by the measured rule of DESIGN.md section 5: harness.train_epoch's captured
                             # step is 1.7 to 7.6 times faster than the eager step, but the modules' own replay inside the unchanged
                             # loop is not faster at 130 and 417 nodes in two of three processes, and one switch governs both


def dropout_capture_applies(model, x: torch.Tensor, g, node_ids=None) -> bool:
    """May this forward of ``model`` under active Dropout be captured into a hipGraph?  Only where every kernel that draws a mask
    reads its seed from a device cell — the one-launch routes: a graph in slots (``gnan_small_batch_*_drop_dev``) or a dense graph
    of up to 448 nodes (``gnan_small_graph_*_drop_dev`` / ``gnan_mid_graph_*_drop_dev``) — and where the backward is one of theirs
    too (the gradients of all of f's and rho's parameters, or of none: the general backward takes its seed by value).  Everything
    else under Dropout stays eager as far as THIS predicate goes: the general route (CSR graphs, larger graphs: it has a predicate
    and a switch of its own, ``functional.dropout_direct_capture_applies``), the NAM read-out, ``batched.TensorGNAN``, ``node_ids``."""
    route = getattr(model, "_small_route", None)
    if not (CAPTURE_DROPOUT and SMALL_GRAPH_DROPOUT and route is not None) or node_ids is not None or x.requires_grad:
        return False
    args = route(node_ids)
    if args is None:
        return False
    use_cnt = args[0]
    f, rho = model._stacked("fs", model.fs), model._stacked("rho", [model.rho])
    wanted = [t.requires_grad for t in (*f[:6], *rho[:6]) if t is not None]
    if any(wanted) and not all(wanted):
        return False
    if isinstance(g, SlotGraph):
        return slot_mode(model) is not None and slot_graph_applies(g, f, rho)
    if not (g.is_dense and SMALL_GRAPH_BACKWARD):
        return False
    if x.shape[0] > SMALL_GRAPH_MAX_NODES:                      # (one rho channel, at most 64 shells: its backward's cover too)
        return mid_graph_pre_rho_applies(x, g, f, rho) if use_cnt == "pre" else mid_graph_applies(x, g, f, rho, use_cnt)
    # (... which the small route's forward exceeds: a device-seed backward is the one launch or nothing)
    return small_graph_applies(x, g, f, rho, pre_rho=use_cnt == "pre") and rho.C == 1 and g.n_codes <= _ONE_LAUNCH_CODES


def slot_graph_forward(slot: SlotGraph, f: StackedMLP, rho: StackedMLP, use_cnt, dropout=None) -> torch.Tensor:
    """The graph read-out ``[C, 1]`` (GNAN.py:75-79 / models.py:383-384) of the graph in the slots: one launch forward, two
    backward (``gnan_small_batch_bwd`` + the slab reduction).  ``use_cnt="pre"``: pre-rho normalisation (GNAN.py:65-67;
    ``gnan_small_batch_pre_fwd`` / ``_bwd``).  ``dropout = (p, seed cell)``: training-mode Dropout of f
    (``gnan_small_batch_fwd_drop_dev``; a slot's graph sits at row 0: the masks of ``gnan_small_graph_fwd_drop``)."""
    from .batched import _BatchedGraphs, _BatchedGraphsPre
    if use_cnt and slot.cnt is None:
        raise _lib.GnanHipError("these slots were laid out without shell sizes")
    fm, rm = (f.L, f.H, f.C, f.F), (rho.L, rho.H, rho.C)
    if use_cnt == "pre":
        out = _BatchedGraphsPre.apply(slot.x, slot.blocks, True, fm, rm, slot.cnt, _dropout_record(dropout), *f[:6], *rho[:6])
        return out.reshape(-1, 1)
    out = _BatchedGraphs.apply(slot.x, slot.blocks, True, fm, rm, slot.cnt if use_cnt else None, False, _dropout_record(dropout),
                               *f[:6], *rho[:6])   # [1, C]
    return out.reshape(-1, 1)


# ---- ... with a NAM read-out (gnan_small_slot_nam_fwd / _bwd) ----------------------------------------------------------------------
def slot_nam_applies(slot: SlotGraph, f: StackedMLP, rho: StackedMLP, nam: StackedMLP) -> bool:
    """The stacks' side of ``gnan_small_slot_nam_fwd`` / ``_bwd`` (the graph's side: :meth:`SlotGraph.fits`): one-wide f and rho, the
    read-out by the rules of :func:`small_graph_nam_applies` — without its limit on the feature count, which was the waiting
    workgroup's."""
    return bool(f.F == nam.F == slot.F and rho.F == 1 and _stack_ok(f, max_c=1) and _stack_ok(rho, max_c=1)
                and _stack_ok(nam, depths=(1, 2, 3)))


class _SlotGraphNam(torch.autograd.Function):
    """:class:`_SmallGraphNam` for the graph in the slots: one launch forward, one backward, sizes read from the device."""

    @staticmethod
    def forward(ctx, slot, use_cnt, fm, rm, nm, *params):
        Lf, Hf, F = fm
        Lr, Hr = rm
        Ln, Hn, Cn = nm
        dev, D = slot.x.device, slot.n_codes
        keep = _kept(params)
        fx = torch.empty((F, slot.max_nodes), dtype=torch.float32, device=dev)
        lut = torch.empty(D, dtype=torch.float32, device=dev)
        hidden = torch.empty(F, dtype=torch.float32, device=dev)
        out = torch.empty(Cn, dtype=torch.float32, device=dev)
        ws = _workspace(dev, _lib.lib().gnan_small_slot_nam_workspace_bytes(F, Cn))
        a = _lib.SmallSlotNamArgs(x=_lib.ptr(slot.x), x_stride=slot.x.stride(0), max_nodes=slot.max_nodes, F=F,
                                  f=_small_mlp(keep[:6], Lf, Hf, 1), rho=_small_mlp(keep[6:12], Lr, Hr, 1),
                                  nam=_nam_mlp(keep[12:], Ln, Hn, Cn), code=_lib.ptr(slot.code), D=D, reserved=0,
                                  **_cnt_pair(slot.cnt if use_cnt else None), node_off=_lib.ptr(slot.node_off), fx=_lib.ptr(fx),
                                  fx_stride=fx.stride(0), lut=_lib.ptr(lut), hidden=_lib.ptr(hidden), out=_lib.ptr(out),
                                  workspace=_lib.ptr(ws), workspace_bytes=ws.numel() * 4)
        _lib.check(_lib.lib().gnan_small_slot_nam_fwd(a, _lib.stream_of(slot.x)), "gnan_small_slot_nam_fwd")
        ctx.slot, ctx.use_cnt, ctx.fm, ctx.rm, ctx.nm = slot, use_cnt, fm, rm, nm
        _save(ctx, (fx, lut, hidden), params)
        return out.view(-1, 1)

    @staticmethod
    def backward(ctx, d_out):
        (fx, lut, hidden), params = _saved(ctx, 3)
        slot = ctx.slot
        Lf, Hf, F = ctx.fm
        Lr, Hr = ctx.rm
        Ln, Hn, Cn = ctx.nm
        dev = slot.x.device
        keep = _kept(params)
        outs = [Fn._grad_outputs(keep[i:i + 6], ctx.dests[i:i + 6]) for i in (0, 6, 12)]
        g_out = d_out.detach().to(torch.float32).contiguous().view(-1)
        ws = _workspace(dev, _lib.lib().gnan_small_slot_nam_workspace_bytes(F, Cn))
        a = _lib.SmallSlotNamBwdArgs(x=_lib.ptr(slot.x), x_stride=slot.x.stride(0), max_nodes=slot.max_nodes, F=F,
                                     f=_small_mlp(keep[:6], Lf, Hf, 1), rho=_small_mlp(keep[6:12], Lr, Hr, 1),
                                     nam=_nam_mlp(keep[12:], Ln, Hn, Cn), code=_lib.ptr(slot.code), D=slot.n_codes, reserved=0,
                                     **_cnt_pair(slot.cnt if ctx.use_cnt else None), node_off=_lib.ptr(slot.node_off),
                                     fx=_lib.ptr(fx), fx_stride=fx.stride(0), lut=_lib.ptr(lut), hidden=_lib.ptr(hidden),
                                     d_out=_lib.ptr(g_out), df=_mlp_grads(outs[0], Lf), drho=_mlp_grads(outs[1], Lr),
                                     dnam=_mlp_grads(outs[2], Ln), workspace=_lib.ptr(ws), workspace_bytes=ws.numel() * 4)
        _lib.check(_lib.lib().gnan_small_slot_nam_bwd(a, _lib.stream_of(slot.x)), "gnan_small_slot_nam_bwd")
        flat = []
        for i, o in zip((0, 6, 12), outs):
            need = ctx.needs_input_grad[5 + i:11 + i]      # (five arguments, then f's six, rho's six, the read-out's six)
            flat += [v if nd else None for v, nd in zip(o, need)]
        return (None, None, None, None, None, *flat)


def slot_graph_nam_forward(slot: SlotGraph, f: StackedMLP, rho: StackedMLP, nam: StackedMLP, use_cnt) -> torch.Tensor:
    """models.py:358-384 with ``is_graph_task`` and ``readout_n_layers > 0`` on the graph in the slots: ``[C, 1]``, one launch forward
    (``gnan_small_slot_nam_fwd``) and one backward.  ``use_cnt``: post-rho shell normalisation (its truth: a :class:`SlotNamMode`
    will do)."""
    if use_cnt and slot.cnt is None:
        raise _lib.GnanHipError("these slots were laid out without shell sizes")
    if not slot_nam_applies(slot, f, rho, nam):
        raise _lib.GnanHipError("graph slots with a NAM read-out take one-wide f and rho (2 or 3 layers, hidden width <= 64) and a "
                                "read-out of 1 to 3 layers and at most 8 output channels over the slots' features")
    _lib.require_device(slot.x, f.w_last, rho.w_last, nam.w_last, slot.code)
    return _SlotGraphNam.apply(slot, bool(use_cnt), (f.L, f.H, f.F), (rho.L, rho.H), (nam.L, nam.H, nam.C),
                               *f[:6], *rho[:6], *nam[:6])
