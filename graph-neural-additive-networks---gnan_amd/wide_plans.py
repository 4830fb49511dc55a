"""Plans of the wide aggregation: the records ``gnan_spmm_args`` points into (each writes its own fields of the struct:
``bind``), their framework-route builders and the steps those share, each written once; :class:`gnan_amd.graph.HopGraph` gates, caches
and delegates here.  Index work wherever the graph's tensors live; pair-sized temporaries are few and short-lived: C4 holds 110M pairs."""
from dataclasses import dataclass
from typing import Optional

import torch

from . import _lib

LONG_ROW_THRESHOLD = 512   # rows with more listed pairs than this go through the slice kernel
SLICE_EDGES = 2048         # pairs per slice of a hub row
PACK_SHIFT = 29            # packed index entries: column id in the low 29 bits, hop code above (gnan_spmm_args.packed_index)
HUB_CLASSES = 8                 # classed hub plan (HopGraph.classed_hub_plan): column class col & 7, one per XCD of the MI355X
CLASSED_HUB_THRESHOLD = 512     # ... its hub rows: more listed pairs than this
CLASSED_SLICE_EDGES = 2048      # ... pairs per slice of one (hub row, class)
STREAM_LAST = 1 << 31             # PairStreamPlan.index: "last pair of its segment" (the packed entry's top bit; codes stay below 4)


def _tensor_bytes(plan) -> int:                 # (``nbytes`` of the plans that report it: their tensor fields)
    return sum(t.numel() * t.element_size() for t in vars(plan).values() if isinstance(t, torch.Tensor))


@dataclass
class LongRowPlan:
    """Hub rows of a CSR graph, cut into fixed-size slices (deterministic reduction order)."""
    rows: Optional[torch.Tensor]        # int32 [n_long] output-row indices
    slice_ptr: Optional[torch.Tensor]   # int32 [n_long + 1]
    n_long: int = 0
    n_slices: int = 0
    threshold: int = LONG_ROW_THRESHOLD
    slice_edges: int = SLICE_EDGES

    def bind(self, a) -> None:            # write this plan's fields of ``a`` (``_lib.SpmmArgs``); every plan has one
        a.long_threshold, a.slice_edges, a.n_long, a.n_slices = self.threshold, self.slice_edges, self.n_long, self.n_slices
        a.long_rows, a.long_slice_ptr = _lib.ptr(self.rows), _lib.ptr(self.slice_ptr)


@dataclass
class ClassedHubPlan(LongRowPlan):
    """A hub-row plan whose slices each hold the pairs of ONE column class ``col & 7``, a class per XCD (``gnan_spmm_args.cls_*`` in
    include/gnan_hip.h states the layout): ``rows`` are the hub slots, ``slice_ptr`` a slot's slices, class-major."""
    index: Optional[torch.Tensor] = None         # int32 [pairs of the hub slots]
    slice_start: Optional[torch.Tensor] = None   # int64 [n_slices + 1]
    slice_row: Optional[torch.Tensor] = None     # int32 [n_slices]
    slot_slice: Optional[torch.Tensor] = None    # int32 [n_slots]
    n_slots: int = 0

    def bind(self, a) -> None:
        super().bind(a)
        if self.index is not None and self.n_long > 0:
            a.cls_index, a.cls_slice_start = _lib.ptr(self.index), _lib.ptr(self.slice_start)
            a.cls_slice_row, a.cls_slot_slice, a.cls_n_slots = _lib.ptr(self.slice_row), _lib.ptr(self.slot_slice), self.n_slots


@dataclass
class ClassedRowPlan:
    """:meth:`HopGraph.classed_row_plan`: the pairs of rows ``[q_lo, q_hi)`` of a degree-sorted copy as SEGMENTS, one per (row, column
    class ``col & 7``) that holds a pair; class-major, then by row (``gnan_spmm_args.seg_*`` in include/gnan_hip.h states the layout)."""
    q_lo: int
    q_hi: int
    min_pairs: int
    n_seg: int
    max_per_class: int            # segments of the largest class (sizes the launch)
    index: torch.Tensor           # int32 [pairs of the classed rows]
    seg_start: torch.Tensor       # int64 [n_seg + 1]
    seg_row: torch.Tensor         # int32 [n_seg]
    cls_seg_ptr: torch.Tensor     # int32 [9]
    mask: torch.Tensor            # uint8 [q_hi - q_lo]

    def bind(self, a) -> None:
        a.seg_index, a.seg_start, a.seg_row = _lib.ptr(self.index), _lib.ptr(self.seg_start), _lib.ptr(self.seg_row)
        a.cls_seg_ptr, a.seg_mask = _lib.ptr(self.cls_seg_ptr), _lib.ptr(self.mask)
        a.seg_q_lo, a.seg_q_hi, a.n_seg, a.seg_max_per_class = self.q_lo, self.q_hi, self.n_seg, self.max_per_class


def drop_slice_plan(a) -> None:
    """The hub rows leave the slice plan (no slice blocks, no fix-up launch); long_threshold stays: the row blocks leave them out by it."""
    a.long_rows = a.long_slice_ptr = a.cls_index = a.cls_slice_start = a.cls_slice_row = a.cls_slot_slice = None
    a.n_long = a.n_slices = a.cls_n_slots = 0


@dataclass
class BlockedHubPlan:
    """:meth:`HopGraph.blocked_hub_plan`: the pairs of the hub rows ``[q_lo, n_rows)`` of a degree-sorted copy as SEGMENTS of at most
    ``seg_pairs`` pairs of one (row, column class ``col & 7``, popularity block) each, in QUEUE order: class-major, block-major, then by
    row, then by piece; ``seg_slot`` is a segment's place in the ROW-major enumeration (``gnan_spmm_args.hub_*`` in include/gnan_hip.h)."""
    q_lo: int
    n_hub: int
    block_rows: int
    n_blocks: int                 # ranked blocks; block ``n_blocks`` is the cold remainder
    seg_pairs: int
    n_seg: int
    max_per_class: int            # segments of the largest class (sizes the launch)
    index: torch.Tensor           # int32 [pairs of the hub rows]
    seg_start: torch.Tensor       # int64 [n_seg + 1]
    seg_row: torch.Tensor         # int32 [n_seg]
    seg_slot: torch.Tensor        # int32 [n_seg]
    row_slot_ptr: torch.Tensor    # int32 [n_hub + 1]
    cls_seg_ptr: torch.Tensor     # int32 [9]
    block_pairs: list             # pairs per block, 0 .. n_blocks (for the record)
    block_segs: list              # segments per block

    nbytes = property(_tensor_bytes)

    def bind(self, a) -> None:
        drop_slice_plan(a)
        a.hub_index, a.hub_seg_start, a.hub_seg_row = _lib.ptr(self.index), _lib.ptr(self.seg_start), _lib.ptr(self.seg_row)
        a.hub_seg_slot, a.hub_row_slot_ptr = _lib.ptr(self.seg_slot), _lib.ptr(self.row_slot_ptr)
        a.hub_cls_seg_ptr, a.hub_q_lo, a.n_hub = _lib.ptr(self.cls_seg_ptr), self.q_lo, self.n_hub
        a.n_hub_seg, a.hub_seg_max_per_class = self.n_seg, self.max_per_class


@dataclass
class PairStreamPlan:
    """:meth:`HopGraph.pair_stream_plan`: the pairs of rows ``[q_lo, q_hi)`` of a degree-sorted copy, all of hop code ``code``, as one
    STREAM per column class ``col & 7``: by popularity block, then by row, cut into chunks of ``chunk_pairs`` entries; a SEGMENT is a
    maximal run of one row inside a chunk and its last entry carries :data:`STREAM_LAST` (``gnan_spmm_args.stream_*`` in
    include/gnan_hip.h states the layout).  ``seg_slot``, the inverse of ``row_seg``, is computed on demand: the library does not read it.
    A range without an upper limit ends with the hub rows ``[q_hub, q_hi)`` (more than :data:`LONG_ROW_THRESHOLD` pairs; ``q_hub == q_hi``
    without one): the same stream and a combine of their own (``gnan_spmm_args.q_hub``).  A class's queue then lists the rows in front of
    the hub rows first, pair for pair as the plan to :data:`LONG_ROW_THRESHOLD` does — those rows keep their segments — and the hub rows'
    pairs behind them, by ``hub_blocks`` ranked blocks of their own, then by row (``block_pairs``: the first part's blocks, then theirs)."""
    q_lo: int
    q_hi: int
    min_pairs: int
    block_rows: int
    n_blocks: int                 # ranked blocks; block ``n_blocks`` is the cold remainder
    chunk_pairs: int
    code: int
    n_seg: int
    n_chunks: int
    max_chunks_per_class: int     # chunks of the largest class (sizes the launch)
    index: torch.Tensor           # int32 [pairs of the stream rows]
    cls_pair_ptr: torch.Tensor    # int32 [9]
    cls_chunk_ptr: torch.Tensor   # int32 [9]
    chunk_first_seg: torch.Tensor  # int32 [n_chunks]
    row_seg: torch.Tensor         # int32 [n_seg] a permutation
    row_slot_ptr: torch.Tensor    # int32 [q_hi - q_lo + 1]
    block_pairs: list             # pairs per block, 0 .. n_blocks (for the record)
    q_hub: int = 0                # first hub row of the range (0 or q_hi: none)
    max_hub_segs: int = 0         # segments of the hub row that lists the most (for the record and the tests: the library does not
                                  # read it — a wave per hub row whatever its length; one device read-back at build time)

    @property
    def seg_slot(self) -> torch.Tensor:
        """int32 [n_seg]: the inverse of ``row_seg`` (the library does not read it; built per call)."""
        slot = torch.empty_like(self.row_seg)
        slot[self.row_seg.long()] = torch.arange(self.n_seg, dtype=torch.int32, device=self.row_seg.device)
        return slot

    nbytes = property(_tensor_bytes)

    def bind(self, a) -> None:
        a.stream_index, a.stream_cls_pair_ptr = _lib.ptr(self.index), _lib.ptr(self.cls_pair_ptr)
        a.stream_cls_chunk_ptr, a.stream_chunk_first_seg = _lib.ptr(self.cls_chunk_ptr), _lib.ptr(self.chunk_first_seg)
        a.stream_row_seg, a.stream_row_slot_ptr = _lib.ptr(self.row_seg), _lib.ptr(self.row_slot_ptr)      # (stream_seg_slot: not read)
        a.stream_q_lo, a.stream_q_hi, a.stream_chunk, a.stream_code = self.q_lo, self.q_hi, self.chunk_pairs, self.code
        a.n_stream_seg, a.stream_max_chunks_per_class = self.n_seg, self.max_chunks_per_class
        a.q_hub = self.q_hub
        if 0 < self.q_hub < self.q_hi:     # (the library's own reading of q_hub) the hub rows ride the stream: they leave the slice plan as BlockedHubPlan.bind takes them out
            drop_slice_plan(a)


def holds_packed(g, max_codes: int = 8, int32_pairs: bool = True) -> bool:
    """Can packed entries ``col | code << 29`` hold this graph (``max_codes``: 8, or 4 where bit 31 is a flag), its pairs numbered in int32?"""
    return not g.is_dense and g.n_cols <= (1 << PACK_SHIFT) and g.n_codes <= max_codes and (not int32_pairs or g.nnz < 2 ** 31)


def signed32(v: torch.Tensor) -> torch.Tensor:
    """int64 values in ``[0, 2^32)`` wrapped to the values of the int32 words of the same bits (still int64: the caller narrows)."""
    return torch.where(v >= (1 << 31), v - (1 << 32), v)


def sorted_range(g, method: str, lo_pairs: int, hi_pairs: Optional[int] = None):
    """The rows of ``lo_pairs .. hi_pairs`` pairs (no ``hi_pairs``: to the last row) of a degree-sorted copy — any other row order
    raises: ``(pairs per row, q_lo, q_hi, R, e0, e1)``, the ``R`` rows ``[q_lo, q_hi)`` holding the pairs ``[e0, e1)``; None without one."""
    rp = g.rowptr.long()
    deg = rp[1:] - rp[:-1]
    if bool((deg[1:] < deg[:-1]).any()):
        raise ValueError(f"{method} needs a degree-sorted copy (rows shortest first)")
    q = torch.searchsorted(deg, torch.tensor([lo_pairs] if hi_pairs is None else [lo_pairs, hi_pairs + 1], device=deg.device)).tolist()
    q_lo, q_hi = q[0], (g.n_rows if hi_pairs is None else q[1])
    return None if q_hi <= q_lo else (deg, q_lo, q_hi, q_hi - q_lo, int(rp[q_lo]), int(rp[q_hi]))


def packed_entries(g, e0: int, e1: int, c: Optional[torch.Tensor] = None) -> torch.Tensor:
    """int32 ``col | code << 29`` of the pairs ``[e0, e1)``, from the graph's own packed stream where it carries one (``c``: their int64 ids)."""
    if g.colp is not None:
        return g.colp[e0:e1]
    return signed32((g.col[e0:e1].long() if c is None else c) | (g.code[e0:e1].long() << PACK_SHIFT)).to(torch.int32)


def rows_of_pairs(deg: torch.Tensor, q_lo: int, q_hi: int) -> torch.Tensor:      # the row, from q_lo, of every pair of [q_lo, q_hi)
    return torch.repeat_interleave(torch.arange(q_hi - q_lo, device=deg.device), deg[q_lo:q_hi])


def queue_key(col: torch.Tensor, row: torch.Tensor, R: int, blk: Optional[torch.Tensor] = None, NB: int = 1) -> torch.Tensor:
    """``((class * NB) + block) * R + row`` of the pairs with column ids ``col`` (no blocks: ``class * R + row``), each in ONE expression."""
    K = HUB_CLASSES
    return (col.long() & (K - 1)) * R + row if blk is None else ((col.long() & (K - 1)) * NB + blk) * R + row


def ptr_from_counts(counts: torch.Tensor) -> torch.Tensor:       # int64 [n + 1]: 0, then the running totals
    ptr = torch.zeros(int(counts.numel()) + 1, dtype=torch.int64, device=counts.device)
    ptr[1:] = torch.cumsum(counts, 0)
    return ptr


def cut_runs(counts: torch.Tensor, cap: int):
    """Runs of ``counts`` consecutive pairs, each cut into pieces of at most ``cap``: ``(run of every piece, its number within the run,
    start, first piece of every run)`` — ``start [n_pieces + 1]`` a piece's first pair, the total behind the last."""
    pieces = (counts + cap - 1) // cap
    pair_off, piece_off = torch.cumsum(counts, 0) - counts, torch.cumsum(pieces, 0) - pieces
    t = torch.repeat_interleave(torch.arange(int(counts.numel()), device=counts.device), pieces)
    j = torch.arange(int(pieces.sum()), device=counts.device) - piece_off[t]
    return t, j, torch.cat([pair_off[t] + j * cap, counts.sum().view(1)]), piece_off


def long_row_plan(g, row_ids, threshold: int) -> LongRowPlan:
    deg = (g.rowptr[1:] - g.rowptr[:-1])
    if row_ids is not None:
        deg = deg[row_ids.long()]
    long_rows = torch.nonzero(deg > threshold).flatten()
    if long_rows.numel() == 0:
        return LongRowPlan(None, None, threshold=threshold)
    ptr = ptr_from_counts((deg[long_rows] + SLICE_EDGES - 1) // SLICE_EDGES)
    return LongRowPlan(long_rows.to(torch.int32), ptr.to(torch.int32), int(long_rows.numel()), int(ptr[-1]), threshold=threshold)


def classed_hub_plan(g, base: LongRowPlan, row_ids, slice_edges: int) -> ClassedHubPlan:
    dev, K, SE = g.device, HUB_CLASSES, int(slice_edges)
    q = base.rows.long()
    i = row_ids.long()[q] if row_ids is not None else q
    rp = g.rowptr.long()
    lo, deg = rp[i], rp[i + 1] - rp[i]
    R = int(q.numel())
    slot = rows_of_pairs(deg, 0, R)
    first = torch.cumsum(deg, 0) - deg
    e = lo[slot] + torch.arange(int(slot.numel()), device=dev) - first[slot]
    c = g.col[e].long()
    v = c | (g.code[e].long() << PACK_SHIFT)
    key = slot * K + (c & (K - 1))
    index = signed32(v)[torch.argsort(key, stable=True)].to(torch.int32)
    t, _, slice_start, slice_off = cut_runs(torch.bincount(key, minlength=R * K), SE)     # t: the (slot, class) of every slice
    n_slices = int(t.numel())
    g8 = t % K
    pos = torch.empty(n_slices, dtype=torch.int64, device=dev)                    # place in its class's queue (slice order)
    longest = 0
    for k in range(K):
        m = torch.nonzero(g8 == k).flatten()
        pos[m] = torch.arange(int(m.numel()), device=dev)
        longest = max(longest, int(m.numel()))
    slot_slice = torch.full((K * longest,), -1, dtype=torch.int32, device=dev)
    slot_slice[pos * K + g8] = torch.arange(n_slices, dtype=torch.int32, device=dev)
    slice_ptr = torch.cat([slice_off.view(R, K)[:, 0], torch.tensor([n_slices], device=dev)]).to(torch.int32)
    return ClassedHubPlan(base.rows, slice_ptr, R, n_slices, threshold=base.threshold, slice_edges=SE, index=index,
                          slice_start=slice_start, slice_row=(t // K).to(torch.int32), slot_slice=slot_slice,
                          n_slots=K * longest)


def classed_row_plan(g, min_pairs: int, max_pairs: int) -> Optional[ClassedRowPlan]:
    dev, K = g.device, HUB_CLASSES
    rng = sorted_range(g, "classed_row_plan", min_pairs, max_pairs)
    if rng is None:
        return None
    deg, q_lo, q_hi, R, e0, e1 = rng
    v = packed_entries(g, e0, e1)
    row = rows_of_pairs(deg, q_lo, q_hi)
    key = queue_key(g.col[e0:e1], row, R)                # class-major, then row; the sort keeps a row's order
    index = v[torch.argsort(key, stable=True)].contiguous()
    cnt = torch.bincount(key, minlength=K * R)
    del key, row
    seg = torch.nonzero(cnt).flatten()                                   # (class, row) of every segment, in plan order
    n_seg = int(seg.numel())
    seg_start = ptr_from_counts(cnt[seg])
    cls_ptr = torch.searchsorted(seg, torch.arange(K + 1, device=dev) * R)
    has = (cnt.view(K, R) > 0).long()
    mask = (has << torch.arange(K, device=dev).view(K, 1)).sum(0).to(torch.uint8)
    return ClassedRowPlan(q_lo, q_hi, int(min_pairs), n_seg, int((cls_ptr[1:] - cls_ptr[:-1]).max()), index, seg_start,
                          (seg % R + q_lo).to(torch.int32), cls_ptr.to(torch.int32), mask.contiguous())


def column_blocks(g, block_rows: int, n_blocks: int) -> torch.Tensor:
    """Popularity block of every column (int64 ``[n_cols]``): the columns of one class ``col & 7`` ranked by how often the graph's pairs
    list them (ties by column id), ``block_rows`` to a block; ranks from ``block_rows * n_blocks`` on share the cold block ``n_blocks``."""
    dev, K = g.device, HUB_CLASSES
    listed = torch.bincount(g.col.long(), minlength=g.n_cols)
    by_count = torch.argsort(listed, descending=True, stable=True)              # ties keep the ascending column id
    order = by_count[torch.argsort(by_count & (K - 1), stable=True)]             # class-major, a class's columns by rank
    cls_first = torch.cumsum(torch.bincount(order & (K - 1), minlength=K), 0)
    cls_first = torch.cat([cls_first.new_zeros(1), cls_first[:-1]])
    rank = torch.empty(g.n_cols, dtype=torch.int64, device=dev)
    rank[order] = torch.arange(g.n_cols, device=dev) - cls_first[order & (K - 1)]
    return torch.clamp(rank // int(block_rows), max=int(n_blocks))


def blocked_hub_plan(g, block_rows: int, n_blocks: int, cap: int, threshold: int) -> Optional[BlockedHubPlan]:
    dev, K, NB = g.device, HUB_CLASSES, n_blocks + 1
    rng = sorted_range(g, "blocked_hub_plan", threshold + 1)
    if rng is None:
        return None
    deg, q_lo, q_hi, R, e0, e1 = rng
    c = g.col[e0:].long()
    v = packed_entries(g, e0, e1, c)
    blk = g.column_blocks(block_rows, n_blocks)[c]
    row = rows_of_pairs(deg, q_lo, q_hi)
    key = queue_key(c, row, R, blk, NB)                      # class, block, row; the sort keeps a row's pair order
    block_pairs = torch.bincount(blk, minlength=NB).tolist()
    del c, blk, row
    index = v[torch.argsort(key, stable=True)].contiguous()
    cnt = torch.bincount(key, minlength=K * NB * R)
    del key
    run = torch.nonzero(cnt).flatten()                                 # (class, block, row) of every run, in queue order
    t, _, seg_start, _ = cut_runs(cnt[run], cap)                        # the run of every segment
    n_seg = int(t.numel())
    seg_key = run[t]
    seg_r, seg_cb = seg_key % R, seg_key // R
    cls_ptr = torch.searchsorted(seg_key, torch.arange(K + 1, device=dev) * (NB * R))
    # the row-major enumeration (row, class, block, piece): a stable sort of the queue order by (row, class, block) keeps the pieces
    by_row = torch.argsort(seg_r * (K * NB) + seg_cb, stable=True)
    seg_slot = torch.empty(n_seg, dtype=torch.int64, device=dev)
    seg_slot[by_row] = torch.arange(n_seg, device=dev)
    row_slot_ptr = ptr_from_counts(torch.bincount(seg_r, minlength=R))
    return BlockedHubPlan(q_lo, R, int(block_rows), int(n_blocks), int(cap), n_seg, int((cls_ptr[1:] - cls_ptr[:-1]).max()), index,
                          seg_start, (seg_r + q_lo).to(torch.int32), seg_slot.to(torch.int32), row_slot_ptr.to(torch.int32),
                          cls_ptr.to(torch.int32), block_pairs, torch.bincount(seg_cb % NB, minlength=NB).tolist())


def pair_stream_plan(g, min_pairs: int, block_rows: int, n_blocks: int, chunk: int, max_pairs: Optional[int],
                     hub_blocks: Optional[int] = None) -> Optional[PairStreamPlan]:
    dev, K, NB = g.device, HUB_CLASSES, n_blocks + 1
    rng = sorted_range(g, "pair_stream_plan", min_pairs, max_pairs)
    if rng is None:
        return None
    deg, q_lo, q_hi, R, e0, e1 = rng
    if e1 - e0 >= 2 ** 31:                                              # (int32 pair, chunk and segment pointers)
        return None
    q_hub = q_hi                                                         # (a range with an upper limit names no hub rows)
    if max_pairs is None:
        q_hub = min(max(int(torch.searchsorted(deg, torch.tensor([LONG_ROW_THRESHOLD + 1], device=deg.device))), q_lo), q_hi)
        if q_hub == q_lo:                                                # (hub rows alone: no row for the first combine)
            return None
    codes = g.code[e0:e1]
    code = int(codes[0])
    if bool((codes != code).any()):
        return None
    c = g.col[e0:e1].long()
    blk = g.column_blocks(block_rows, n_blocks)[c]
    row = rows_of_pairs(deg, q_lo, q_hi)
    if q_hub < q_hi:
        # a class's queue: the rows in front of the hub rows FIRST, exactly as the plan to LONG_ROW_THRESHOLD lists them (the same chunk
        # cuts, hence the same segments and the same bits for those rows), then the hub rows by their own ``hub_blocks`` ranked blocks —
        # numbered behind the others', so that the one key orders both parts
        HB = (n_blocks if hub_blocks is None else int(hub_blocks)) + 1
        blk = torch.where(row >= q_hub - q_lo, NB + g.column_blocks(block_rows, HB - 1)[c], blk)
        NB += HB
    key = queue_key(c, row, R, blk, NB)                      # class, block, row; the sort keeps a row's pair order
    block_pairs = torch.bincount(blk, minlength=NB).tolist()
    order = torch.argsort(key, stable=True)
    key, v = key[order], (c | (code << PACK_SHIFT))[order]
    del c, blk, row, order
    P = int(key.numel())
    cls, row = key // (NB * R), key % R
    cls_pair_ptr = torch.searchsorted(key, torch.arange(K + 1, device=dev) * (NB * R))
    n_chunk_cls = (cls_pair_ptr[1:] - cls_pair_ptr[:-1] + chunk - 1) // chunk
    cls_chunk_ptr = torch.cat([n_chunk_cls.new_zeros(1), torch.cumsum(n_chunk_cls, 0)])
    pos = torch.arange(P, device=dev) - cls_pair_ptr[cls]               # place in its class's queue
    first = pos % chunk == 0                                            # (a class starts a chunk)
    first[1:] |= row[1:] != row[:-1]
    last = torch.ones(P, dtype=torch.bool, device=dev)
    last[:-1] = first[1:]
    seg_of_pair = torch.cumsum(first, 0) - 1
    n_seg = int(seg_of_pair[-1]) + 1
    n_chunks = int(cls_chunk_ptr[-1])
    t_cls = torch.repeat_interleave(torch.arange(K, device=dev), n_chunk_cls)
    chunk_pair = cls_pair_ptr[t_cls] + (torch.arange(n_chunks, device=dev) - cls_chunk_ptr[t_cls]) * chunk
    chunk_first_seg = seg_of_pair[chunk_pair]
    seg_row = row[first]
    row_seg = torch.argsort(seg_row, stable=True)                      # row by row, a row's segments in queue order
    row_slot_ptr = ptr_from_counts(torch.bincount(seg_row, minlength=R))
    max_hub_segs = int((row_slot_ptr[q_hub - q_lo + 1:] - row_slot_ptr[q_hub - q_lo:-1]).max()) if q_hub < q_hi else 0
    v = v | (last.long() << 31)
    index = signed32(v).to(torch.int32).contiguous()
    return PairStreamPlan(q_lo, q_hi, int(min_pairs), int(block_rows), int(n_blocks), int(chunk), code, n_seg, n_chunks,
                          int(n_chunk_cls.max()), index, cls_pair_ptr.to(torch.int32), cls_chunk_ptr.to(torch.int32),
                          chunk_first_seg.to(torch.int32), row_seg.to(torch.int32), row_slot_ptr.to(torch.int32), block_pairs,
                          q_hub, max_hub_segs)
