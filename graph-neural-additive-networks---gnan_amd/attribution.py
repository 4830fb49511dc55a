"""Per-row attributions on the HIP path (``gnan_attr_rows``, csrc/attr_rows.hip): the terms of the aggregation by
(shell, operand column) for the requested rows — what ``rho_aggregate`` sums away.

``A[q, d, w] = wt(i_q, d, w % Cw) * sum of S[j, w] over the nodes j in shell d of row i_q`` and ``A.sum(1)`` is
``rho_aggregate``'s row.  Device tensors only; no autograd.  :func:`gnan_amd.interpret.explain`
is the model-level front."""
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
