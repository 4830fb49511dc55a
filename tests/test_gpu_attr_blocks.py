"""``gnan_attr_blocks`` on the GPU (csrc/attr_blocks.hip): every element of ``B`` and ``T`` within the derived bound of
tests/attr_blocks_ref.py over tile edges, a multi-tile graph, an empty graph, clamped codes, every bin-pass count, shared and
per-row tables, counts on and off; exact cases; the same bits alone, together, twice and wherever the graph stands in the batch;
70 001 graphs in one call; and the one-graph route ``gnan_attr_cols`` on every graph alone."""
import functools

import numpy as np
import pytest
import torch

import attr_blocks_ref
import attr_cols_ref
from attr_ref import check

from gnan_amd import HopGraph, _lib, attribution
from gnan_amd.batched import HopBlocks

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZES = [1, 2, 63, 64, 65, 0, 130, 5]


def blocks_of(code, sizes, D):
    node_off, code_off = HopBlocks._offsets(sizes, DEV)
    return HopBlocks(code.to(DEV), node_off, code_off, sizes, D - 2)


@functools.lru_cache(maxsize=None)
def case(D, W, Cw, per_row, with_cnt, sizes=tuple(SIZES)):
    """Host tensors: codes 0 .. D + 1 (the listed codes >= D - 1 are clamped) and 255, S in a row stride of W + 3."""
    gen = torch.Generator().manual_seed(1000 * D + 10 * W + Cw + 2 * per_row + with_cnt)
    N, P = sum(sizes), sum(s * s for s in sizes)
    code = torch.randint(0, min(D + 2, 255), (P,), generator=gen).to(torch.uint8)
    code[torch.rand(P, generator=gen) < 0.2] = 255
    S = torch.randn((N, W + 3), generator=gen)[:, :W]
    lut = torch.randn((N, D, Cw) if per_row else (D, Cw), generator=gen)
    cnt = torch.randint(0, 9, (N, D), generator=gen).to(torch.int32) if with_cnt else None
    return code, S, lut, cnt


def run(D, sizes, code, S, lut, cnt, want_nodes=True, want_graphs=True):
    dev = lambda t: None if t is None else t.to(DEV)      # noqa: E731
    Sd = torch.empty((S.shape[0], S.shape[1] + 3), device=DEV)[:, : S.shape[1]]
    Sd.copy_(S)
    assert Sd.stride(0) > Sd.shape[1]
    return attribution.block_attributions(blocks_of(code, list(sizes), D), Sd, dev(lut), dev(cnt), want_nodes, want_graphs)


@pytest.mark.parametrize("with_cnt", [False, True])
@pytest.mark.parametrize("per_row", [False, True])
@pytest.mark.parametrize("W,Cw", [(1, 1), (5, 1), (6, 3), (67, 1)])
@pytest.mark.parametrize("D", [2, 3, 17, 65, 256])
def test_every_element_within_its_bound(D, W, Cw, per_row, with_cnt):
    code, S, lut, cnt = case(D, W, Cw, per_row, with_cnt)
    assert int((code == 255).sum()) > 0 and (D >= 254 or int(((code >= D - 1) & (code < 255)).sum()) > 0)
    B, T = run(D, SIZES, code, S, lut, cnt)
    tB, bB, tT, bT = attr_blocks_ref.reference(code, SIZES, S, lut, cnt)
    assert tuple(B.shape) == (sum(SIZES), D, W) and tuple(T.shape) == (len(SIZES), D, W)
    check(B, tB, bB, f"B D={D} W={W} Cw={Cw} per_row={per_row} cnt={with_cnt}")
    check(T, tT, bT, f"T D={D} W={W} Cw={Cw} per_row={per_row} cnt={with_cnt}")
    assert not bool(T[SIZES.index(0)].any())                        # the empty graph in the middle: a row of zeros


@pytest.mark.parametrize("D,W,Cw,per_row", [(2, 1, 1, False), (17, 6, 3, True), (65, 5, 1, False), (256, 67, 1, True)])
def test_exact_cases_equal_an_int64_restatement(D, W, Cw, per_row):
    gen = torch.Generator().manual_seed(D)
    N, P = sum(SIZES), sum(s * s for s in SIZES)
    code = torch.randint(0, min(D + 2, 255), (P,), generator=gen).to(torch.uint8)
    code[torch.rand(P, generator=gen) < 0.2] = 255
    S = torch.randint(-4, 5, (N, W), generator=gen)
    lut = torch.randint(-3, 4, (N, D, Cw) if per_row else (D, Cw), generator=gen)
    B, T = run(D, SIZES, code, S.float(), lut.float(), None)
    wt = lut if per_row else lut.unsqueeze(0).expand(N, -1, -1)
    wantB, wantT = torch.zeros((N, D, W), dtype=torch.int64), torch.zeros((len(SIZES), D, W), dtype=torch.int64)
    ch = torch.arange(W) % Cw
    n0 = c0 = 0
    for g, n in enumerate(SIZES):
        if n:
            d = code[c0: c0 + n * n].long().clamp_max(D - 1)
            i, j = torch.arange(n).repeat_interleave(n), torch.arange(n).repeat(n)
            V = torch.zeros((n * D, Cw), dtype=torch.int64).index_add_(0, j * D + d, wt[n0 + i, d]).view(n, D, Cw)
            wantB[n0: n0 + n] = V[:, :, ch] * S[n0: n0 + n].unsqueeze(1)
            wantT[g] = wantB[n0: n0 + n].sum(0)
        n0, c0 = n0 + n, c0 + n * n
    assert torch.equal(B.cpu().long(), wantB) and torch.equal(B.cpu(), wantB.float())
    assert torch.equal(T.cpu().long(), wantT) and torch.equal(T.cpu(), wantT.float())


@pytest.mark.parametrize("D,W,Cw,per_row,with_cnt", [(17, 6, 3, True, True), (65, 5, 1, False, True), (3, 67, 1, False, False)])
def test_alone_together_and_twice_give_the_same_bits(D, W, Cw, per_row, with_cnt):
    c = case(D, W, Cw, per_row, with_cnt)
    B, T = run(D, SIZES, *c)
    B1, none = run(D, SIZES, *c, want_graphs=False)
    none2, T1 = run(D, SIZES, *c, want_nodes=False)
    B2, T2 = run(D, SIZES, *c)
    assert none is None and none2 is None
    assert torch.equal(B, B1) and torch.equal(B, B2) and torch.equal(T, T1) and torch.equal(T, T2)


@pytest.mark.parametrize("D,W,Cw,per_row,with_cnt", [(17, 6, 3, True, True), (65, 5, 1, False, False)])
def test_a_graphs_bits_do_not_depend_on_the_batch(D, W, Cw, per_row, with_cnt):
    code, S, lut, cnt = case(D, W, Cw, per_row, with_cnt)
    gi = SIZES.index(130)
    n0, c0 = sum(SIZES[:gi]), sum(s * s for s in SIZES[:gi])
    n, nn = 130, 130 * 130
    rows = lambda t, order: None if t is None else torch.cat([t[a:b] for a, b in order])          # noqa: E731
    B, T = run(D, SIZES, code, S, lut, cnt)
    wantB, wantT = B[n0: n0 + n], T[gi]
    N, P = sum(SIZES), code.numel()
    for name, sizes, node_order, code_order, at, g_at in (
            ("alone", [130], [(n0, n0 + n)], [(c0, c0 + nn)], 0, 0),
            ("first", [130] + SIZES[:gi] + SIZES[gi + 1:], [(n0, n0 + n), (0, n0), (n0 + n, N)], [(c0, c0 + nn), (0, c0), (c0 + nn, P)], 0, 0),
            ("last", SIZES[:gi] + SIZES[gi + 1:] + [130], [(0, n0), (n0 + n, N), (n0, n0 + n)], [(0, c0), (c0 + nn, P), (c0, c0 + nn)],
             N - n, len(SIZES) - 1)):
        B2, T2 = run(D, sizes, rows(code, code_order), rows(S, node_order), lut if lut.dim() == 2 else rows(lut, node_order),
                     rows(cnt, node_order))
        assert torch.equal(B2[at: at + n], wantB) and torch.equal(T2[g_at], wantT), name


def test_seventy_thousand_graphs_in_one_call():
    G1, D, W = 70_000, 5, 4
    sizes = [1] * G1 + [65]
    gen = torch.Generator().manual_seed(7)
    code = torch.randint(0, 7, (G1 + 65 * 65,), generator=gen).to(torch.uint8)
    S = torch.randn((G1 + 65, W), generator=gen)
    lut = torch.randn((D, 1), generator=gen)
    cnt = torch.randint(0, 4, (G1 + 65, D), generator=gen).to(torch.int32)
    none, T = run(D, sizes, code, S, lut, cnt, want_nodes=False)
    assert none is None and tuple(T.shape) == (G1 + 1, D, W)
    for g in (0, G1 // 2, G1 - 1):
        _, _, tT, bT = attr_blocks_ref.reference(code[g: g + 1], [1], S[g: g + 1], lut, cnt[g: g + 1])
        check(T[g: g + 1], tT, bT, f"graph {g}")
    _, _, tT, bT = attr_blocks_ref.reference(code[G1:], [65], S[G1:], lut, cnt[G1:])
    check(T[G1:], tT, bT, "the last graph")


@pytest.mark.parametrize("D,W,Cw,per_row,with_cnt", [(17, 6, 3, True, False), (65, 5, 1, False, True), (3, 1, 1, False, True)])
def test_against_the_one_graph_route_on_every_graph(D, W, Cw, per_row, with_cnt):
    code, S, lut, cnt = case(D, W, Cw, per_row, with_cnt)
    B, _ = run(D, SIZES, code, S, lut, cnt, want_graphs=False)
    _, bB, _, _ = attr_blocks_ref.reference(code, SIZES, S, lut, cnt)
    n0 = c0 = 0
    for n in SIZES:
        if n:
            cg = code[c0: c0 + n * n].view(n, n)
            lg = lut[n0: n0 + n] if per_row else lut
            ng = None if cnt is None else cnt[n0: n0 + n]
            g = HopGraph(n_rows=n, n_cols=n, n_codes=D, code=cg.to(DEV), cnt=None if ng is None else ng.to(DEV))
            one = attribution.source_attributions(g, S[n0: n0 + n].to(DEV), lg.to(DEV), with_cnt)
            _, b_cols, _ = attr_cols_ref.reference(cg.T.contiguous(), S[n0: n0 + n], lg, cnt=ng)
            diff = (one.double().cpu().numpy() - B[n0: n0 + n].double().cpu().numpy())
            assert np.all(np.abs(diff) <= b_cols + bB[n0: n0 + n]), f"graph of {n} nodes: {np.abs(diff).max():.3e}"
        n0, c0 = n0 + n, c0 + n * n


def test_refusals_and_the_byte_budget(monkeypatch):
    code, S, lut, cnt = case(3, 5, 1, False, True)
    b = blocks_of(code, SIZES, 3)
    with pytest.raises(_lib.GnanHipError, match="CPU tensor"):
        attribution.block_attributions(b, S, lut.to(DEV))
    b.slots = True
    with pytest.raises(_lib.GnanHipError, match="slots of a captured step"):
        attribution.block_attributions(b, S.to(DEV), lut.to(DEV))
    b.slots = False
    N = sum(SIZES)
    monkeypatch.setattr(attribution, "ATTR_MAX_BYTES", N * 3 * 5 * 4 - 1)
    with pytest.raises(_lib.GnanHipError, match=r"\[%d, 3, 5\] float32 takes \d+ bytes.*pass the graphs in batches" % N):
        attribution.block_attributions(b, S.to(DEV), lut.to(DEV))
    none, T = attribution.block_attributions(b, S.to(DEV), lut.to(DEV), want_nodes=False)      # T alone stores no B: no budget
    assert none is None and tuple(T.shape) == (len(SIZES), 3, 5)
