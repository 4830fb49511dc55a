"""Per-row attributions on the HIP path (``gnan_attr_rows``, csrc/attr_rows.hip): the terms of the aggregation by
(shell, operand column) for the requested rows — what ``rho_aggregate`` sums away.

``A[q, d, w] = wt(i_q, d, w % Cw) * sum of S[j, w] over the nodes j in shell d of row i_q`` and ``A.sum(1)`` is
``rho_aggregate``'s row.  Device tensors only; no autograd.  :func:`gnan_amd.interpret.explain`
is the model-level front.

By source node (``gnan_attr_cols``, csrc/attr_cols.hip): ``B[p, d, w] = S[j_p, w] * sum over the requested rows i that see node
j_p at hop d of wt(i, d, w % Cw)`` — :func:`source_attributions`, with :func:`gnan_amd.interpret.explain_sources` in front.

Reduced over groups of rows (``gnan_attr_reduce``, csrc/attr_reduce.hip): the float64 moments ``sum A``, ``sum |A|``, ``sum A^2`` of the
terms over groups of requested rows, and of a row's total over the shells, without ``A`` itself — :func:`reduced_attributions`, with
:func:`gnan_amd.interpret.importance` in front.

A batch of graphs (``gnan_attr_blocks``, csrc/attr_blocks.hip): the by-source-node terms of EVERY graph of a ``HopBlocks`` batch and their
sums per graph, in at most three launches whatever the number of graphs — :func:`block_attributions`, with
:func:`gnan_amd.interpret.explain_graphs` / ``importance_graphs`` in front."""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib
from .functional import _rows
from .graph import HopGraph

ATTR_MAX_BYTES = 1 << 30        # largest result [R, D, W] a call allocates; pass ``rows`` in batches beyond


def _args(g: HopGraph, S: torch.Tensor, lut: torch.Tensor, use_cnt: bool, rows: Optional[torch.Tensor],
          s_total: Optional[torch.Tensor], n_out: int) -> _lib.AttrArgs:
    D = g.n_codes
    W = S.shape[1]
    per_row = lut.dim() == 3
    a = _lib.AttrArgs(n_rows=n_out, n_cols=g.n_cols, code=_lib.ptr(g.code), row_ids=_lib.ptr(rows),
                      S=_lib.ptr(S), W=W, s_stride=S.stride(0), lut=_lib.ptr(lut), lut_row_stride=D * lut.shape[-1] if per_row else 0,
                      D=D, Cw=lut.shape[-1], s_total=_lib.ptr(s_total), a_stride=D * W)
    if use_cnt:
        a.cnt, a.cnt_stride = _lib.ptr(g.cnt), g.cnt.stride(0)
    if not g.is_dense:
        a.rowptr, a.rowptr_is64 = _lib.ptr(g.rowptr), int(g.rowptr.dtype == torch.int64)
        a.col, a.nnz = _lib.ptr(g.col), g.nnz
    return a


def describe(a: _lib.AttrArgs) -> dict:
    """``gnan_attr_rows_describe``: column tiles, shell passes, chunk length, chunks of the longest row, launches, LDS bytes
    (host-only)."""
    info = _lib.AttrInfo()
    _lib.check(_lib.lib().gnan_attr_rows_describe(a, info), "gnan_attr_rows_describe")
    return info.as_dict()


class Launch:
    """One prepared call of ``gnan_attr_rows``: the argument record, the result it writes and the tensors it points into.
    ``pairs``: listed pairs of the requested rows (what the first launch walks per column tile and shell pass)."""

    def __init__(self, args: _lib.AttrArgs, A: torch.Tensor, keep: tuple, pairs: int):
        self.args, self.A, self.keep, self.pairs = args, A, keep, pairs

    def run(self) -> torch.Tensor:
        if self.A.shape[0]:
            _lib.check(_lib.lib().gnan_attr_rows(self.args, _lib.stream_of(self.A)), "gnan_attr_rows")
        return self.A


@torch.no_grad()
def shell_attributions(g: HopGraph, S: torch.Tensor, lut: torch.Tensor, use_cnt: bool, rows: Optional[torch.Tensor] = None,
                       s_total: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``A [R, D, W]`` float32 for the rows ``rows`` of ``g`` (all of them by default; any order, repeats allowed).

    ``S [n_cols, W]`` float32 operand rows; ``lut [D, Cw]`` (one table) or ``[n_rows, D, Cw]`` (pre-rho: per row);
    ``use_cnt`` divides by the shell sizes ``g.cnt``; ``s_total [W]`` (a CSR's rest bucket): the rest shell is
    ``s_total`` minus the listed pairs' rows instead of the pairs coded ``D - 1``."""
    return prepare(g, S, lut, use_cnt, rows, s_total).run()


@torch.no_grad()
def prepare(g: HopGraph, S: torch.Tensor, lut: torch.Tensor, use_cnt: bool, rows: Optional[torch.Tensor] = None,
            s_total: Optional[torch.Tensor] = None) -> Launch:
    """Everything of :func:`shell_attributions` but the launches (tools/explain_time.py times ``Launch.run`` alone)."""
    _lib.require_device(S, lut, g.code, s_total, rows if torch.is_tensor(rows) else None)
    if S.dim() != 2 or S.shape[0] != g.n_cols:
        raise ValueError(f"S must be [n_cols={g.n_cols}, W], got {tuple(S.shape)}")
    S = _rows(S.detach().float())
    lut = lut.detach().float().contiguous()
    if lut.dim() not in (2, 3) or lut.shape[-2] != g.n_codes or (lut.dim() == 3 and lut.shape[0] != g.n_rows):
        raise ValueError(f"lut must be [D={g.n_codes}, Cw] or [n_rows={g.n_rows}, D, Cw], got {tuple(lut.shape)}")
    if s_total is not None:
        s_total = s_total.detach().float().contiguous()
    if rows is not None:
        rows = torch.as_tensor(rows, device=g.device).to(torch.int32).contiguous().view(-1)
    R = g.n_rows if rows is None else rows.numel()
    D, W = g.n_codes, S.shape[1]
    nbytes = R * D * W * 4
    if nbytes > ATTR_MAX_BYTES:
        raise _lib.GnanHipError(f"shell_attributions: the result [{R}, {D}, {W}] float32 takes {nbytes} bytes, above ATTR_MAX_BYTES = "
                                f"{ATTR_MAX_BYTES}: pass `rows` in batches")
    A = torch.empty((R, D, W), dtype=torch.float32, device=g.device)
    a = _args(g, S, lut, use_cnt, rows, s_total, R)
    a.A = _lib.ptr(A)
    if R == 0:
        return Launch(a, A, (), 0)
    keep, pairs = None, R * g.n_cols
    if not g.is_dense:
        # framework arithmetic on R integers: chunks per requested row, their prefix sum, the longest row
        chunk = describe(a)["chunk_pairs"]
        deg = (g.rowptr[1:] - g.rowptr[:-1]).long()
        if rows is not None:
            deg = deg[rows.long()]
        ptr = torch.zeros(R + 1, dtype=torch.int64, device=g.device)
        torch.cumsum(((deg + (chunk - 1)) // chunk).clamp_(min=1), 0, out=ptr[1:])
        n_items, longest, pairs = torch.stack([ptr[-1], deg.max(), deg.sum()]).tolist()
        a.max_row_pairs = longest
        if n_items > R:
            if n_items > 0x7fffffff:
                raise _lib.GnanHipError(f"shell_attributions: {n_items} work items exceed one launch: pass `rows` in batches")
            keep = ptr.to(torch.int32)
            a.item_ptr, a.n_items = _lib.ptr(keep), n_items
    need = _lib.lib().gnan_attr_rows_workspace_bytes(a)
    ws = torch.empty((need + 3) // 4, dtype=torch.float32, device=g.device) if need else None
    a.workspace, a.workspace_bytes = _lib.ptr(ws), need
    return Launch(a, A, (g, S, lut, rows, s_total, keep, ws), pairs)


# =============================================================================
# by source node: gnan_attr_cols (csrc/attr_cols.hip)
# =============================================================================
def describe_sources(a: _lib.AttrColsArgs) -> dict:
    """``gnan_attr_cols_describe``: chunk length, bin passes, launches, LDS bytes, blocks of the T sum (host-only)."""
    info = _lib.AttrColsInfo()
    _lib.check(_lib.lib().gnan_attr_cols_describe(a, info), "gnan_attr_cols_describe")
    return info.as_dict()


class SourceLaunch(Launch):
    """One prepared call of ``gnan_attr_cols``; ``pairs``: listed pairs of the requested sources (walked once)."""

    def run(self) -> torch.Tensor:
        if self.A.shape[0]:
            _lib.check(_lib.lib().gnan_attr_cols(self.args, _lib.stream_of(self.A)), "gnan_attr_cols")
        return self.A


@torch.no_grad()
def source_attributions(g: HopGraph, S: torch.Tensor, lut: torch.Tensor, use_cnt: bool, rows: Optional[torch.Tensor] = None,
                        cols: Optional[torch.Tensor] = None, rest_from_total: Optional[bool] = None) -> torch.Tensor:
    """``B [P, D, W]`` float32: what source node ``cols[p]`` (every node by default) adds, at hop ``d``, to column ``w`` of the SUM
    of the outputs of ``rows`` (every row by default; any order, a row that repeats counts as often as it occurs) —
    ``B[p, d, w] = S[j_p, w] * sum over the requested rows i that see j_p at hop d of wt(i, d, w % Cw)``.

    ``g`` is the forward graph (its cached transpose is walked); ``S``, ``lut``, ``use_cnt`` as in :func:`shell_attributions`.
    ``rest_from_total`` (default: ``g`` is a CSR): the rest shell counts every pair NOT listed below ``D - 1`` — the sum of the
    requested rows' rest weights minus the listed ones.  ``B.sum(0)`` equals ``shell_attributions(...).sum(0)`` for the same rows."""
    return prepare_sources(g, S, lut, use_cnt, rows, cols, rest_from_total).run()


@torch.no_grad()
def prepare_sources(g: HopGraph, S: torch.Tensor, lut: torch.Tensor, use_cnt: bool, rows: Optional[torch.Tensor] = None,
                    cols: Optional[torch.Tensor] = None, rest_from_total: Optional[bool] = None) -> SourceLaunch:
    """Everything of :func:`source_attributions` but the launches (tools/explain_sources_time.py times ``run`` alone)."""
    _lib.require_device(S, lut, g.code, rows if torch.is_tensor(rows) else None, cols if torch.is_tensor(cols) else None)
    if S.dim() != 2 or S.shape[0] != g.n_cols:
        raise ValueError(f"S must be [n_cols={g.n_cols}, W], got {tuple(S.shape)}")
    S = _rows(S.detach().float())
    lut = lut.detach().float().contiguous()
    if lut.dim() not in (2, 3) or lut.shape[-2] != g.n_codes or (lut.dim() == 3 and lut.shape[0] != g.n_rows):
        raise ValueError(f"lut must be [D={g.n_codes}, Cw] or [n_rows={g.n_rows}, D, Cw], got {tuple(lut.shape)}")
    if rest_from_total is None:
        rest_from_total = not g.is_dense
    ids = lambda v: torch.as_tensor(v, device=g.device).to(torch.int32).contiguous().view(-1)      # noqa: E731
    rows = None if rows is None else ids(rows)
    cols = None if cols is None else ids(cols)
    P = g.n_cols if cols is None else cols.numel()
    D, W = g.n_codes, S.shape[1]
    nbytes = P * D * W * 4
    if nbytes > ATTR_MAX_BYTES:
        raise _lib.GnanHipError(f"source_attributions: the result [{P}, {D}, {W}] float32 takes {nbytes} bytes, above ATTR_MAX_BYTES = "
                                f"{ATTR_MAX_BYTES}: pass `cols` in batches")
    B = torch.empty((P, D, W), dtype=torch.float32, device=g.device)
    t = g.transposed()
    per_row = lut.dim() == 3
    a = _lib.AttrColsArgs(n_cols=P, n_src=g.n_cols, n_rows=g.n_rows, code=_lib.ptr(t.code), col_ids=_lib.ptr(cols),
                          row_ids=_lib.ptr(rows), n_row_ids=-1 if rows is None else rows.numel(), S=_lib.ptr(S), W=W,
                          s_stride=S.stride(0), lut=_lib.ptr(lut), lut_row_stride=D * lut.shape[-1] if per_row else 0, D=D,
                          Cw=lut.shape[-1], rest_from_total=int(bool(rest_from_total)), B=_lib.ptr(B), b_stride=D * W)
    if use_cnt:
        a.cnt, a.cnt_stride = _lib.ptr(g.cnt), g.cnt.stride(0)
    if not g.is_dense:
        a.rowptr_t, a.rowptr_is64 = _lib.ptr(t.rowptr), int(t.rowptr.dtype == torch.int64)
        a.row, a.nnz = _lib.ptr(t.col), g.nnz
    if P == 0:
        return SourceLaunch(a, B, (), 0)
    keep, pairs = None, P * g.n_rows
    if not g.is_dense:
        # framework arithmetic on P integers: chunks per requested source, their prefix sum, the longest column
        chunk = describe_sources(a)["chunk_pairs"]
        deg = (t.rowptr[1:] - t.rowptr[:-1]).long()
        if cols is not None:
            deg = deg[cols.long()]
        ptr = torch.zeros(P + 1, dtype=torch.int64, device=g.device)
        torch.cumsum(((deg + (chunk - 1)) // chunk).clamp_(min=1), 0, out=ptr[1:])
        n_items, longest, pairs = torch.stack([ptr[-1], deg.max(), deg.sum()]).tolist()
        a.max_col_pairs = longest
        if n_items > P:
            if n_items > 0x7fffffff:
                raise _lib.GnanHipError(f"source_attributions: {n_items} work items exceed one launch: pass `cols` in batches")
            keep = ptr.to(torch.int32)
            a.item_ptr, a.n_items = _lib.ptr(keep), n_items
    need = _lib.lib().gnan_attr_cols_workspace_bytes(a)
    ws = torch.empty((need + 3) // 4, dtype=torch.float32, device=g.device) if need else None
    a.workspace, a.workspace_bytes = _lib.ptr(ws), need
    return SourceLaunch(a, B, (g, t, S, lut, rows, cols, keep, ws), pairs)


# =============================================================================
# reduced over groups of rows: gnan_attr_reduce (csrc/attr_reduce.hip)
# =============================================================================
ATTR_REDUCE_MAX_WORKSPACE = 1 << 30     # chunk partials of long rows one launch may hold; beyond, several launches cut at block boundaries


def describe_reduced(a: _lib.AttrReduceArgs) -> dict:
    """``gnan_attr_reduce_describe``: chunk length, rows per block, shell passes, launches, LDS bytes and the workspace split into
    chunk partials, block partials and the plan's integers (host-only)."""
    info = _lib.AttrReduceInfo()
    _lib.check(_lib.lib().gnan_attr_reduce_describe(a, info), "gnan_attr_reduce_describe")
    return info.as_dict()


class ReducedLaunch(Launch):
    """The prepared calls of ``gnan_attr_reduce`` for one result ``A = M [G, 3, D + 1, W]``: one call per range of blocks, the last
    one adds the groups' block partials.  ``pairs``: listed pairs of the requested rows."""

    def __init__(self, calls: list, M: torch.Tensor, keep: tuple, pairs: int):
        super().__init__(calls[-1], M, keep, pairs)
        self.calls = calls

    def run(self) -> torch.Tensor:
        if self.A.numel():
            st = _lib.stream_of(self.A)
            for a in self.calls:
                _lib.check(_lib.lib().gnan_attr_reduce(a, st), "gnan_attr_reduce")
        return self.A


@torch.no_grad()
def reduced_attributions(g: HopGraph, S: torch.Tensor, lut: torch.Tensor, use_cnt: bool, rows: Optional[torch.Tensor] = None,
                         group_ptr: Optional[torch.Tensor] = None, s_total: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``M [G, 3, D + 1, W]`` float64: over the requested rows ``group_ptr[g] .. group_ptr[g + 1] - 1`` of group ``g`` (positions in
    ``rows``; default: one group of all requested rows), ``M[g, 0] = sum a``, ``M[g, 1] = sum |a|``, ``M[g, 2] = sum a^2`` of the
    float32 terms ``a = shell_attributions(...)[q, d, w]`` for ``d < D``; slot ``d = D`` holds the same moments of a row's total over
    the shells.  The ``[R, D, W]`` array is never formed; inputs as :func:`shell_attributions`.  An empty group gives zeros."""
    return prepare_reduced(g, S, lut, use_cnt, rows, group_ptr, s_total).run()


@torch.no_grad()
def prepare_reduced(g: HopGraph, S: torch.Tensor, lut: torch.Tensor, use_cnt: bool, rows: Optional[torch.Tensor] = None,
                    group_ptr: Optional[torch.Tensor] = None, s_total: Optional[torch.Tensor] = None) -> ReducedLaunch:
    """Everything of :func:`reduced_attributions` but the launches (tools/importance_time.py times ``run`` alone)."""
    _lib.require_device(S, lut, g.code, s_total, rows if torch.is_tensor(rows) else None)
    if S.dim() != 2 or S.shape[0] != g.n_cols:
        raise ValueError(f"S must be [n_cols={g.n_cols}, W], got {tuple(S.shape)}")
    S = _rows(S.detach().float())
    lut = lut.detach().float().contiguous()
    if lut.dim() not in (2, 3) or lut.shape[-2] != g.n_codes or (lut.dim() == 3 and lut.shape[0] != g.n_rows):
        raise ValueError(f"lut must be [D={g.n_codes}, Cw] or [n_rows={g.n_rows}, D, Cw], got {tuple(lut.shape)}")
    if s_total is not None:
        s_total = s_total.detach().float().contiguous()
    if rows is not None:
        rows = torch.as_tensor(rows, device=g.device).to(torch.int32).contiguous().view(-1)
    R = g.n_rows if rows is None else rows.numel()
    D, W = g.n_codes, S.shape[1]
    dev = g.device
    gp = gp_host = None
    G = 1
    if group_ptr is not None:
        # the device copy is checked here; the library checks the host copy again
        gp = torch.as_tensor(group_ptr).to(device=dev, dtype=torch.int64).contiguous().view(-1)
        if gp.numel() < 1:
            raise ValueError("group_ptr must hold at least one entry")
        gp_host = gp.cpu()
        if int(gp_host[0]) != 0 or int(gp_host[-1]) != R or bool((gp_host[1:] < gp_host[:-1]).any()):
            raise ValueError(f"group_ptr must rise from 0 to the number of requested rows ({R}) without a step down")
        G = gp.numel() - 1
    per_row = lut.dim() == 3
    a = _lib.AttrReduceArgs(n_rows=R, n_cols=g.n_cols, code=_lib.ptr(g.code), row_ids=_lib.ptr(rows), S=_lib.ptr(S), W=W,
                            s_stride=S.stride(0), lut=_lib.ptr(lut), lut_row_stride=D * lut.shape[-1] if per_row else 0, D=D,
                            Cw=lut.shape[-1], s_total=_lib.ptr(s_total), group_ptr=_lib.ptr(gp_host), n_groups=G)
    if use_cnt:
        a.cnt, a.cnt_stride = _lib.ptr(g.cnt), g.cnt.stride(0)
    if not g.is_dense:
        a.rowptr, a.rowptr_is64 = _lib.ptr(g.rowptr), int(g.rowptr.dtype == torch.int64)
        a.col = _lib.ptr(g.col)
    info = describe_reduced(a)
    chunk, br = info["chunk_pairs"], info["block_rows"]
    M = torch.empty((G, 3, D + 1, W), dtype=torch.float64, device=dev)
    # framework arithmetic on integers: the blocks of every group, the chunk items of the long rows
    if gp is None:
        n_blocks = -(-R // br)
        block_ptr = gbp = None
        starts = torch.arange(n_blocks + 1, dtype=torch.int64).mul_(br).clamp_(max=R)            # host
    else:
        nb_g = (gp_host[1:] - gp_host[:-1] + (br - 1)) // br
        gbp_host = torch.zeros(G + 1, dtype=torch.int64)
        torch.cumsum(nb_g, 0, out=gbp_host[1:])
        n_blocks = int(gbp_host[-1])
        gid = torch.repeat_interleave(torch.arange(G), nb_g)
        starts = torch.full((n_blocks + 1,), R, dtype=torch.int64)
        starts[:-1] = gp_host[gid] + (torch.arange(n_blocks) - gbp_host[gid]) * br
        block_ptr, gbp = starts.to(dev), gbp_host.to(dev)
    a.block_ptr, a.group_block_ptr, a.n_blocks = _lib.ptr(block_ptr), _lib.ptr(gbp), n_blocks
    partials = torch.empty(n_blocks * 3 * (D + 1) * W, dtype=torch.float64, device=dev)
    a.partials, a.partials_bytes, a.M = _lib.ptr(partials), partials.numel() * 8, _lib.ptr(M)
    item_ptr, pairs = None, R * g.n_cols
    if g.is_dense:
        uc = -(-g.n_cols // chunk) if g.n_cols > chunk else 0
        item_at = starts * uc                                                                  # chunk items before each block
    else:
        deg = (g.rowptr[1:] - g.rowptr[:-1]).long()
        if rows is not None:
            deg = deg[rows.long()]
        ptr = torch.zeros(R + 1, dtype=torch.int64, device=dev)
        n_items = longest = pairs = 0
        if R:
            nch = (deg + (chunk - 1)) // chunk
            torch.cumsum(torch.where(nch > 1, nch, torch.zeros_like(nch)), 0, out=ptr[1:])
            n_items, longest, pairs = torch.stack([ptr[-1], deg.max(), deg.sum()]).tolist()
        if n_items > 0x7fffffff:
            raise _lib.GnanHipError(f"reduced_attributions: {n_items} chunk items exceed an int32 plan: pass `rows` in batches")
        item_ptr = ptr.to(torch.int32)
        a.item_ptr, a.max_row_pairs = _lib.ptr(item_ptr), longest
        item_at = ptr[starts.to(dev)].cpu() if n_items else torch.zeros(n_blocks + 1, dtype=torch.int64)
    # launches: cut at block boundaries where the chunk partials of one launch would exceed ATTR_REDUCE_MAX_WORKSPACE
    item_bytes = D * W * 4
    cuts = [0]
    if int(item_at[-1]) * item_bytes > ATTR_REDUCE_MAX_WORKSPACE:
        at = item_at.tolist()
        for b in range(1, n_blocks):
            if (at[b + 1] - at[cuts[-1]]) * item_bytes > ATTR_REDUCE_MAX_WORKSPACE and b > cuts[-1]:
                cuts.append(b)
    cuts.append(n_blocks)
    calls, need = [], 0
    for b0, b1 in zip(cuts[:-1], cuts[1:]):
        c = _lib.AttrReduceArgs.from_buffer_copy(a)
        c.block_first, c.block_count = b0, b1 - b0
        c.item_first, c.item_count = int(item_at[b0]), int(item_at[b1] - item_at[b0])
        c.combine = int(b1 == n_blocks)
        need = max(need, _lib.lib().gnan_attr_reduce_workspace_bytes(c))
        calls.append(c)
    ws = torch.empty((need + 3) // 4, dtype=torch.float32, device=dev) if need else None
    for c in calls:
        c.workspace, c.workspace_bytes = _lib.ptr(ws), need
    return ReducedLaunch(calls, M, (g, S, lut, rows, s_total, gp_host, block_ptr, gbp, item_ptr, partials, ws), pairs)


# =============================================================================
# a batch of graphs, by source node and by graph: gnan_attr_blocks (csrc/attr_blocks.hip)
# =============================================================================
def describe_blocks(a: _lib.AttrBlocksArgs) -> dict:
    """``gnan_attr_blocks_describe``: column tiles, bin passes, row-chunk length, launches, LDS bytes, the workspace (host-only)."""
    info = _lib.AttrBlocksInfo()
    _lib.check(_lib.lib().gnan_attr_blocks_describe(a, info), "gnan_attr_blocks_describe")
    return info.as_dict()


class BlocksLaunch(Launch):
    """One prepared call of ``gnan_attr_blocks``: ``B`` (or None) and ``T`` (or None) are what :meth:`run` returns; ``pairs``: the
    ``sum n_g^2`` codes of the batch (walked once per bin pass)."""

    def __init__(self, args: _lib.AttrBlocksArgs, B, T, keep: tuple, pairs: int):
        super().__init__(args, B, keep, pairs)
        self.B, self.T = B, T

    def run(self):
        out = self.B if self.B is not None else self.T
        if self.args.n_graphs:
            _lib.check(_lib.lib().gnan_attr_blocks(self.args, _lib.stream_of(out)), "gnan_attr_blocks")
        return self.B, self.T


@torch.no_grad()
def block_attributions(blocks, S: torch.Tensor, lut: torch.Tensor, cnt: Optional[torch.Tensor] = None, want_nodes: bool = True,
                       want_graphs: bool = True):
    """``(B, T)`` for ALL graphs of ``blocks`` (:class:`gnan_amd.batched.HopBlocks`) in one call: ``B [N, D, W]`` float32 — what node
    ``j`` adds, at hop ``d``, to column ``w`` of the summed output of ITS graph, :func:`source_attributions` of every graph alone —
    and ``T [G, D, W]``, its sum over the nodes of each graph in node order (an empty graph: zeros).  ``want_nodes`` / ``want_graphs``:
    which of the two is formed (the other is None; each has the bits it has alone).

    ``S [N, W]`` float32 operand rows; ``lut [D, Cw]`` or ``[N, D, Cw]`` (pre-rho: per forward row), ``D = blocks.n_codes``; ``cnt
    [N, D]`` int32 divides by the shell sizes (the slot layout: hops below ``D - 1`` in their columns, the unreachable pairs in the
    last).  A code of 255 and every listed code ``>= D - 1`` count for the rest shell."""
    return prepare_blocks(blocks, S, lut, cnt, want_nodes, want_graphs).run()


@torch.no_grad()
def prepare_blocks(blocks, S: torch.Tensor, lut: torch.Tensor, cnt: Optional[torch.Tensor] = None, want_nodes: bool = True,
                   want_graphs: bool = True) -> BlocksLaunch:
    """Everything of :func:`block_attributions` but the launches (tools/explain_graphs_time.py times ``run`` alone)."""
    if getattr(blocks, "slots", False):
        raise _lib.GnanHipError("block_attributions: these blocks are the slots of a captured step: their sizes live on the device only")
    if not (want_nodes or want_graphs):
        raise ValueError("block_attributions: one of want_nodes / want_graphs must be set")
    _lib.require_device(S, lut, blocks.code, cnt)
    G, N, D = blocks.n_graphs, blocks.total_nodes, blocks.n_codes
    if S.dim() != 2 or S.shape[0] != N:
        raise ValueError(f"S must be [total_nodes={N}, W], got {tuple(S.shape)}")
    S = _rows(S.detach().float())
    lut = lut.detach().float().contiguous()
    if lut.dim() not in (2, 3) or lut.shape[-2] != D or (lut.dim() == 3 and lut.shape[0] != N):
        raise ValueError(f"lut must be [D={D}, Cw] or [total_nodes={N}, D, Cw], got {tuple(lut.shape)}")
    if cnt is not None:
        if cnt.dim() != 2 or cnt.shape[0] != N or cnt.shape[1] < D or cnt.dtype != torch.int32:
            raise ValueError(f"cnt must be int32 [total_nodes={N}, >= D={D}], got {cnt.dtype} {tuple(cnt.shape)}")
        cnt = cnt if cnt.stride(1) == 1 else cnt.contiguous()
    W = S.shape[1]
    dev = S.device
    B = T = None
    if want_nodes:
        nbytes = N * D * W * 4
        if nbytes > ATTR_MAX_BYTES:
            raise _lib.GnanHipError(f"block_attributions: the result [{N}, {D}, {W}] float32 takes {nbytes} bytes, above ATTR_MAX_BYTES = "
                                    f"{ATTR_MAX_BYTES}: pass the graphs in batches")
        B = torch.empty((N, D, W), dtype=torch.float32, device=dev)
    if want_graphs:
        T = torch.empty((G, D, W), dtype=torch.float32, device=dev)
    a = _lib.AttrBlocksArgs(code=_lib.ptr(blocks.code), node_off=_lib.ptr(blocks.node_off), code_off=_lib.ptr(blocks.code_off),
                            n_graphs=G, total_nodes=N, max_nodes=blocks.max_nodes, S=_lib.ptr(S), W=W, s_stride=S.stride(0),
                            lut=_lib.ptr(lut), lut_row_stride=D * lut.shape[-1] if lut.dim() == 3 else 0, D=D, Cw=lut.shape[-1],
                            B=_lib.ptr(B), b_stride=D * W, T=_lib.ptr(T))
    if cnt is not None:
        a.cnt, a.cnt_stride = _lib.ptr(cnt), cnt.stride(0)
    need = _lib.lib().gnan_attr_blocks_workspace_bytes(a)
    ws = torch.empty((need + 3) // 4, dtype=torch.float32, device=dev) if need else None
    a.workspace, a.workspace_bytes = _lib.ptr(ws), need
    return BlocksLaunch(a, B, T, (blocks, S, lut, cnt, ws), int(blocks.code.numel()))
