"""Batched preprocessing on the GPU (csrc/bfs_blocks.hip): hop codes and shell sizes of many graphs from ONE edge_index.
Every output is an integer: every comparison here is bit-exact (golden fixtures, an independent numpy BFS, the one-graph route
``HopGraph.from_edge_index`` and the dense-input route ``HopGraph.from_dense``)."""
import numpy as np
import pytest
import torch

from conftest import Golden, golden_names
from oracle import gnan_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda"
MODEL_CASES = [n for n in golden_names() if not any(t in n for t in ("pre_process", "batched", "trainer", "run_exp"))]
GOLDEN = golden_names("pre_process") + [MODEL_CASES[5], MODEL_CASES[11], MODEL_CASES[0]]     # test_gpu_preprocessing_bit_exact's


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")


def np_hops(ei, n):
    """All-pairs directed hop counts, -1 where unreachable: level by level on boolean matrices (nothing of the kernels' scheme)."""
    adj = np.zeros((n, n), dtype=np.float32)
    adj[ei[0], ei[1]] = 1.0
    hops = np.full((n, n), -1, dtype=np.int32)
    np.fill_diagonal(hops, 0)
    frontier, d = np.eye(n, dtype=np.float32), 0
    while frontier.any():
        d += 1
        frontier = ((frontier @ adj > 0) & (hops < 0)).astype(np.float32)
        hops[frontier > 0] = d
    return hops


def batch_of(edge_lists, sizes, seed):
    """One PyG-style batch: node ids offset, the edge order shuffled by a seeded permutation."""
    off = np.cumsum([0] + list(sizes))
    ei = np.concatenate([np.asarray(e, dtype=np.int64).reshape(2, -1) + off[g] for g, e in enumerate(edge_lists)], axis=1)
    ei = ei[:, np.random.default_rng(seed).permutation(ei.shape[1])]
    batch = np.repeat(np.arange(len(sizes)), sizes)
    return torch.from_numpy(ei).to(DEV), torch.from_numpy(batch).to(DEV)


def check_graph(g, hops, max_hops=None, what=""):
    """A HopGraph against a hop matrix, truncated as test_gpu_preprocessing_bit_exact truncates its expectation."""
    if max_hops is not None:
        hops = np.where(hops > max_hops, -1, hops)
    n = hops.shape[0]
    D = (int(hops.max()) if n else 0) + 2
    assert g.is_dense and g.n_rows == g.n_cols == n, what
    assert g.n_codes == D, (what, g.n_codes, D)
    assert tuple(g.code.shape) == (n, n) and tuple(g.cnt.shape) == (n, D), what
    assert g.code.dtype == torch.uint8 and g.cnt.dtype == torch.int32
    assert np.array_equal(g.code.cpu().numpy(), np.where(hops < 0, 255, hops).astype(np.uint8)), what
    assert np.array_equal(g.cnt.cpu().numpy(), O.shell_counts(hops, D)), what


# ---------------------------------------------------------------------------------------------- 1. golden fixtures
@pytest.fixture(scope="module")
def golden_batch():
    cases = [Golden(name) for name in GOLDEN]
    sizes = [int(c.inputs["node_distances"].shape[0]) for c in cases]
    hops = [O.hop_codes_from_dense(torch.from_numpy(np.array(c.inputs["node_distances"]))) for c in cases]
    ei, batch = batch_of([np.array(c.inputs["edge_index"]) for c in cases], sizes, seed=11)
    return ei, batch, hops


@pytest.mark.parametrize("max_hops", [None, 2, 3])
def test_golden_fixtures_in_one_batch(golden_batch, max_hops):
    from gnan_amd import HopGraph
    ei, batch, hops = golden_batch
    assert {7, 40, 300} <= {h.shape[0] for h in hops}
    graphs = HopGraph.batch_from_edge_index(ei, batch, max_hops=max_hops)
    assert len(graphs) == len(hops)
    for name, g, h in zip(GOLDEN, graphs, hops):
        check_graph(g, h, max_hops, name)


# ---------------------------------------------------------------------------------------------- 2. size edges
def _random_directed(rng, n):
    """About 1.5 n directed edges among the first 7/8 of the nodes (the rest stay isolated), a tenth of them duplicated, self loops."""
    m = int(1.5 * n)
    ei = rng.integers(0, max(1, n - n // 8), (2, m))
    ei[:, : m // 10] = ei[:, m // 10: 2 * (m // 10)]
    ei[1, m - 1] = ei[0, m - 1]
    if m > 4:
        ei[1, 3] = ei[0, 3]
    return ei.astype(np.int64)


@pytest.fixture(scope="module")
def edge_graphs():
    """Seeded random directed graphs at every size where the kernels change path — one block of 64 nodes or several, the one-launch
    routes' limits, the bound and one past it — plus a graph without edges and a graph id without nodes; their numpy hop matrices."""
    from gnan_amd import _lib
    bound = _lib.BFS_BLOCKS_MAX_NODES
    sizes = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 448, bound, 5, 0, bound + 1]
    rng = np.random.default_rng(5)
    edges = [_random_directed(rng, n) if n else np.zeros((2, 0), np.int64) for n in sizes]
    edges[sizes.index(5)] = np.zeros((2, 0), np.int64)
    hops = [np_hops(e, n) for e, n in zip(edges, sizes)]
    assert max(int(h.max()) for h in hops if h.size) <= 254
    return sizes, edges, hops


def _counted(monkeypatch):
    from gnan_amd import _lib
    calls = []
    for name in ("gnan_bfs_blocks", "gnan_shell_counts_blocks", "gnan_bfs_dense"):
        real = getattr(_lib.lib(), name)
        monkeypatch.setattr(_lib.lib(), name, lambda a, st, name=name, real=real: calls.append(name) or real(a, st))
    return calls


@pytest.mark.parametrize("with_oversize", [False, True])
def test_size_edges(edge_graphs, with_oversize, monkeypatch):
    from gnan_amd import HopGraph, _lib
    sizes, edges, hops = edge_graphs
    k = len(sizes) if with_oversize else len(sizes) - 1
    ei, batch = batch_of(edges[:k], sizes[:k], seed=7)
    calls = _counted(monkeypatch)
    graphs = HopGraph.batch_from_edge_index(ei, batch, num_graphs=k)
    if with_oversize:
        assert sizes[-1] == _lib.BFS_BLOCKS_MAX_NODES + 1
        assert calls == ["gnan_bfs_blocks", "gnan_shell_counts_blocks", "gnan_bfs_dense"]
    else:                              # the empty graph id is the batch's last: num_graphs names it
        assert sizes[k - 1] == 0
        assert calls == ["gnan_bfs_blocks", "gnan_shell_counts_blocks"]
    assert len(graphs) == k
    for g, n, e, h in zip(graphs, sizes, edges, hops):
        check_graph(g, h, None, f"n={n}")
        if e.shape[1] or not n:        # (gnan_bfs_dense refuses the null edge array of a graph with nodes and no edge)
            one = HopGraph.from_edge_index(torch.from_numpy(e).to(DEV), n)
            assert one.n_codes == g.n_codes and torch.equal(one.code, g.code) and torch.equal(one.cnt, g.cnt), n
        if n:
            ht = torch.from_numpy(h).to(DEV)
            nd = torch.where(ht < 0, torch.zeros((), device=DEV), 1.0 / (1.0 + ht.float()))
            dense = HopGraph.from_dense(nd)
            assert dense.n_codes == g.n_codes and torch.equal(dense.code, g.code) and torch.equal(dense.cnt, g.cnt), n


@pytest.mark.parametrize("max_hops", [2, 5])
def test_size_edges_truncated(edge_graphs, max_hops):
    from gnan_amd import HopGraph
    sizes, edges, hops = edge_graphs
    ei, batch = batch_of(edges[:-1], sizes[:-1], seed=8)
    for g, n, h in zip(HopGraph.batch_from_edge_index(ei, batch, len(sizes) - 1, max_hops), sizes, hops):
        check_graph(g, h, max_hops, f"n={n} K={max_hops}")


# ---------------------------------------------------------------------------------------------- 3. limits and errors
def _path(n):
    return torch.stack([torch.arange(n - 1), torch.arange(1, n)]).to(DEV)


def test_limits_and_errors():
    """All host exceptions raised from a status word: nothing here faults the device."""
    from gnan_amd import HopGraph, _lib
    zeros = lambda n: torch.zeros(n, dtype=torch.long, device=DEV)      # noqa: E731
    g, = HopGraph.batch_from_edge_index(_path(255), zeros(255))
    assert g.n_codes == 256 and int(g.code[0, 254]) == 254 and int(g.code[254, 0]) == 255
    assert g.cnt[0].tolist() == [1] * 255 + [0] and g.cnt[254].tolist() == [1] + [0] * 254 + [254]
    with pytest.raises(_lib.GnanHipError, match="longer than 254 hops"):
        HopGraph.batch_from_edge_index(_path(256), zeros(256))
    g, = HopGraph.batch_from_edge_index(_path(256), zeros(256), max_hops=254)          # truncation is not an overflow
    assert g.n_codes == 256 and int(g.code[0, 255]) == 255
    batch = torch.tensor([0, 0, 0, 1, 1], device=DEV)
    ok = torch.tensor([[0, 1, 3], [1, 2, 4]], device=DEV)
    assert [h.n_rows for h in HopGraph.batch_from_edge_index(ok, batch)] == [3, 2]
    with pytest.raises(_lib.GnanHipError, match="two different graphs"):
        HopGraph.batch_from_edge_index(torch.tensor([[0, 2], [1, 3]], device=DEV), batch)
    for bad in (5, -1, 1 << 40):
        with pytest.raises(_lib.GnanHipError, match="outside"):
            HopGraph.batch_from_edge_index(torch.tensor([[0, 1], [1, bad]], device=DEV), batch)
    with pytest.raises(_lib.GnanHipError, match="sorted"):
        HopGraph.batch_from_edge_index(ok, torch.tensor([0, 1, 0, 1, 1], device=DEV))
    with pytest.raises(ValueError, match="num_graphs"):
        HopGraph.batch_from_edge_index(ok, batch, num_graphs=1)
    from gnan_amd.batched import HopBlocks
    with pytest.raises(_lib.GnanHipError, match="two different graphs"):
        HopBlocks.from_edge_index(torch.tensor([[0, 2], [1, 3]], device=DEV), batch)


# ---------------------------------------------------------------------------------------------- 4. views and reproducibility
def test_views_of_two_packed_buffers_and_reproducibility(edge_graphs):
    from gnan_amd import HopGraph, graph
    sizes, edges, _ = edge_graphs
    sizes, edges = sizes[:-1], edges[:-1]
    ei, batch = batch_of(edges, sizes, seed=9)
    first = HopGraph.batch_from_edge_index(ei, batch, len(sizes))
    code_off = graph.packed_offsets([n * n for n in sizes], graph.BFS_BLOCKS_ALIGN)
    cnt_off = graph.packed_offsets([n * g.n_codes for n, g in zip(sizes, first)])
    live = [g for g in first if g.n_rows]
    code_buf, cnt_buf = live[0].code._base, live[0].cnt._base
    assert code_buf.dim() == 1 and code_buf.numel() == code_off[-1] and cnt_buf.dim() == 1 and cnt_buf.numel() == cnt_off[-1]
    for i, g in enumerate(first):
        assert g.code.is_contiguous() and g.cnt.is_contiguous()
        if g.n_rows:
            assert g.code._base.data_ptr() == code_buf.data_ptr() and g.cnt._base.data_ptr() == cnt_buf.data_ptr()
            assert g.code.data_ptr() == code_buf.data_ptr() + code_off[i]
            assert g.cnt.data_ptr() == cnt_buf.data_ptr() + 4 * cnt_off[i]
            assert g.code.data_ptr() % 4 == 0                  # what gnan_mid_graph_fwd asks of a code pointer
    second = HopGraph.batch_from_edge_index(ei, batch, len(sizes))
    again = [g for g in second if g.n_rows]
    assert torch.equal(again[0].code._base, code_buf) and torch.equal(again[0].cnt._base, cnt_buf)


# ---------------------------------------------------------------------------------------------- 5. blocks
def _undirected(rng, n, extra):
    tree = np.stack([np.arange(1, n), rng.integers(0, np.arange(1, n))]) if n > 1 else np.zeros((2, 0), np.int64)
    more = np.stack([rng.integers(0, n, extra), rng.integers(0, n, extra)])
    ei = np.concatenate([tree, more], axis=1)
    return np.concatenate([ei, ei[::-1]], axis=1).astype(np.int64)


def test_blocks_equal_from_blocks(edge_graphs):
    from gnan_amd.batched import HopBlocks
    sizes, edges, hops = edge_graphs                       # (the oversize graph included: its block is copied in)
    ei, batch = batch_of(edges, sizes, seed=10)
    got = HopBlocks.from_edge_index(ei, batch)
    want = HopBlocks.from_blocks([torch.from_numpy(h).float().to(DEV) for h in hops])
    assert got.sizes == want.sizes and got.n_codes == want.n_codes and got.n_graphs == want.n_graphs
    assert (got.total_nodes, got.max_nodes, got.min_nodes) == (want.total_nodes, want.max_nodes, want.min_nodes)
    for name in ("code", "node_off", "code_off"):
        a, b = getattr(got, name), getattr(want, name)
        assert a.dtype == b.dtype and a.is_contiguous() and torch.equal(a, b), name
    assert torch.equal(got.batch_vector(), want.batch_vector())


def test_batched_model_on_collate_edges():
    """batched.TensorGNAN forward and parameter gradients: collate_edges(...) against collate(...) of the same graphs — the same
    kernels with the same bytes in, so equal to the bit."""
    from gnan_amd.batched import TensorGNAN, collate, collate_edges
    rng = np.random.default_rng(21)
    sizes, F = [5, 12, 30, 64, 9, 40], 4
    edges = [_undirected(rng, n, n // 6 + 1) for n in sizes]
    xs = [torch.from_numpy(rng.random((n, F), dtype=np.float32)).to(DEV) for n in sizes]
    ys = [torch.tensor([float(i % 2)], device=DEV) for i in range(len(sizes))]
    with_hops = [(x, torch.from_numpy(np_hops(e, n)).float().to(DEV), y) for x, e, n, y in zip(xs, edges, sizes, ys)]
    with_edges = [(x, torch.from_numpy(e).to(DEV), y) for x, e, y in zip(xs, edges, ys)]
    torch.manual_seed(0)
    m = TensorGNAN(F, 2, 2, hidden_channels=16, device=DEV).to(DEV).eval()

    def run(batch):
        x, blocks, y, bv = batch
        m.zero_grad(set_to_none=True)
        out = m(x, blocks, bv)
        out.pow(2).sum().backward()
        return out.detach().clone(), y, bv, {k: p.grad.detach().clone() for k, p in m.named_parameters()}
    want, want_y, want_bv, want_g = run(collate(with_hops))
    got, got_y, got_bv, got_g = run(collate_edges(with_edges))
    assert got.shape == (len(sizes), 2) and torch.equal(got, want) and torch.equal(got_y, want_y) and torch.equal(got_bv, want_bv)
    assert got_g.keys() == want_g.keys()
    for k in want_g:
        assert torch.equal(got_g[k], want_g[k]), k


# ---------------------------------------------------------------------------------------------- 6. modules
class Bag:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _module(kind, F):
    from gnan_amd import GNAN as standalone
    from gnan_amd import models
    torch.manual_seed(3)
    if kind == "models.TensorGNAN":
        m = models.TensorGNAN(F, 1, 3, hidden_channels=16, is_graph_task=True, readout_n_layers=0, device=DEV)
    elif kind == "GNAN.TensorGNAN":
        m = standalone.TensorGNAN(F, 1, 3, hidden_channels=16, is_graph_task=True, device=DEV)
    else:
        m = models.GNAN(F, 2, num_layers=3, hidden_channels=16, device=DEV)
    return m.to(DEV).eval()


@pytest.fixture(scope="module")
def task_graphs():
    """5, 70 and 200 nodes: the small, the 65-128 and the mid one-launch routes."""
    rng = np.random.default_rng(31)
    sizes, F = [5, 70, 200], 6
    out = []
    for n in sizes:
        x = torch.zeros(n, F)
        x[torch.arange(n), torch.from_numpy(rng.integers(0, F - 1, n))] = 1.0
        x[:, -1] = 1.0
        out.append((x.to(DEV), torch.from_numpy(_undirected(rng, n, n // 10 + 1)).to(DEV), torch.tensor([[1.0]], device=DEV)))
    return out


@pytest.mark.parametrize("kind", ["models.TensorGNAN", "GNAN.TensorGNAN", "models.GNAN"])
def test_modules_on_attached_graphs(task_graphs, kind):
    import gnan_amd
    from gnan_amd import HopGraph
    fresh = lambda: [Bag(x=x, edge_index=ei, y=y) for x, ei, y in task_graphs]      # noqa: E731
    attached = gnan_amd.attach_hop_graphs(fresh())
    chunked = gnan_amd.attach_hop_graphs(fresh(), pair_budget=25)                     # 5^2 at most: three chunks
    single = fresh()
    for d in single:
        d.gnan_graph = HopGraph.from_edge_index(d.edge_index, d.x.shape[0])
    for a, c, s in zip(attached, chunked, single):
        assert isinstance(a.gnan_graph, HopGraph) and a.gnan_graph.n_codes == c.gnan_graph.n_codes == s.gnan_graph.n_codes
        for t in ("code", "cnt"):
            assert torch.equal(getattr(a.gnan_graph, t), getattr(s.gnan_graph, t)), t
            assert torch.equal(getattr(c.gnan_graph, t), getattr(s.gnan_graph, t)), t
    m = _module(kind, task_graphs[0][0].shape[1])

    def run(d):
        m.zero_grad(set_to_none=True)
        out = m.forward(d)
        out.pow(2).sum().backward()
        return out.detach().clone(), {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}
    for a, s in zip(attached, single):
        want, want_g = run(s)
        got, got_g = run(a)
        assert torch.isfinite(want).all() and torch.equal(got, want), (kind, a.x.shape[0])
        assert got_g.keys() == want_g.keys() and len(want_g) > 0
        for k in want_g:
            assert torch.equal(got_g[k], want_g[k]), (kind, a.x.shape[0], k)
