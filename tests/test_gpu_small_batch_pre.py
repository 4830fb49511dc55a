"""Pre-rho normalisation (GNAN.py:65-67: the weight of pair (i, j) is rho(u_d / |shell_i(d)|)) on the batched / slot kernels
(csrc/small_graph.hip: gnan_small_batch_pre_fwd / _bwd and their ``_drop_dev`` twins; batched._BatchedGraphsPre,
small_graph.slot_graph_forward(..., "pre")): batches against the float64 chain graph by graph, a batch of one against the one-graph
kernel's bits, offsets, graph slots, the Dropout twins, and the stand-alone module class through ``harness.train_epoch`` and the
modules' own replay.

Tolerances: the project's rule (helpers.assert_rule / assert_grads_rule: the float32 chain's own error beyond the 1e-5 floor) against
the float64 chain; TWO_FLOORS between two routes of the build (each lies within the floor of the same truth)."""
import copy
import functools
import types
import warnings

import numpy as np
import pytest
import torch

import test_gpu_dropout_capture as cap_tests
from helpers import TWO_FLOORS, assert_grads_rule, assert_rule
from test_gpu_graphed import DEV, _graph_task, _need_gpu
from test_gpu_mid_graph import _mlps
from test_gpu_mid_graph_pre import _Case
from test_gpu_small_graph_dropout import P, SEED

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def switch_on(monkeypatch):
    """The route's switch follows a measured rule: the tests do not depend on how it ships."""
    from gnan_amd import small_graph
    monkeypatch.setattr(small_graph, "SLOT_PRE_RHO", True)


def _hops(rng, n, D, top=False):
    """Hop counts of one graph over at most D codes (-1 = unreachable).  D == 64: every row lists eight of the 63 hops (and the rest):
    most of its shells are empty.  ``top``: hop D - 2 is listed (the graph has D codes of its own)."""
    if D == 64 and n > 1:
        own = np.stack([rng.choice(D - 1, 8, replace=False) for _ in range(n)])
        pick = rng.integers(-1, 8, (n, n))
        hops = np.where(pick >= 0, np.take_along_axis(own, np.maximum(pick, 0), axis=1), -1).astype(np.int32)
    else:
        hops = rng.integers(-1, D - 1, (n, n)).astype(np.int32)
    hops[np.arange(n), np.arange(n)] = 0
    if top and n > 1:
        hops[0, 1] = D - 2
    return hops


def _cnt_of(hops, D):
    codes = np.where(hops >= 0, hops, D - 1)
    return np.stack([(codes == d).sum(1) for d in range(D)], axis=1).astype(np.int32)


class _Batch:
    """Graphs of a batch with ONE pair of stacks: on the device through ``_BatchedGraphsPre``, on the CPU as one chain per graph
    (test_gpu_mid_graph_pre._Case.chain over the BATCH's D codes and shell sizes) whose gradients add up."""

    def __init__(self, sizes, F, D, C, L, H, bias_f, bias_r, seed=0):
        from gnan_amd.batched import HopBlocks
        self.sizes, self.F, self.D, self.C, self.L, self.H = list(sizes), F, D, C, L, H
        rng = np.random.default_rng(1000 * sum(sizes) + 10 * D + seed)
        self.fp, self.rp = _mlps(rng, F, C, L, H, bias_f, bias_r)
        big = int(np.argmax(sizes))
        self.hops = [_hops(rng, n, D, top=g == big) for g, n in enumerate(sizes)]
        self.blocks = HopBlocks.from_blocks([torch.from_numpy(h).float().to(DEV) for h in self.hops])
        assert self.blocks.n_codes == D or max(sizes) == 1, (self.blocks.n_codes, D)
        self.D = D = self.blocks.n_codes
        self.N, self.G = sum(sizes), len(sizes)
        self.xs = [torch.from_numpy(rng.standard_normal((n, F)).astype(np.float32)) for n in sizes]
        self.x = torch.cat(self.xs)
        self.cnts = [_cnt_of(h, D) for h in self.hops]
        self.cnt = torch.from_numpy(np.concatenate(self.cnts)).to(DEV)
        self.up = {True: torch.from_numpy(rng.standard_normal((self.G, C))), False: torch.from_numpy(rng.standard_normal((self.N, C)))}
        self.off = np.concatenate([[0], np.cumsum(sizes)])

    def sub(self, g, graph_sum):
        """Graph g as a case of the one-graph tests, on the batch's D codes and its own rows of the shell sizes."""
        s = _Case.__new__(_Case)
        s.hops, s.x, s.fp, s.rp, s.L, s.H, s.C, s.graph_sum = self.hops[g], self.xs[g], self.fp, self.rp, self.L, self.H, self.C, graph_sum
        s.n, s.F, s.D = self.sizes[g], self.F, self.D
        s.g = types.SimpleNamespace(cnt=torch.from_numpy(self.cnts[g]))
        s.up = self.up[True][g].view(-1, 1) if graph_sum else self.up[False][self.off[g]:self.off[g + 1]]
        return s

    def leaves(self):
        fl = [None if t is None else t.to(DEV).requires_grad_(True) for t in self.fp]
        rl = [None if t is None else t.to(DEV).requires_grad_(True) for t in self.rp]
        return fl, rl

    def device(self, graph_sum, dropout=None, only=None):
        """-> (outputs, gradients, (S, lut [N * D, 1])); ``only``: graph g sent alone."""
        from gnan_amd.batched import HopBlocks, _BatchedGraphsPre
        fl, rl = self.leaves()
        x, blocks, cnt, up = self.x, self.blocks, self.cnt, self.up[graph_sum]
        if only is not None:
            g, lo, hi = only, self.off[only], self.off[only + 1]
            blocks = HopBlocks.from_blocks([torch.from_numpy(self.hops[g]).float().to(DEV)])
            if blocks.n_codes != self.D:                   # (the batch's codes: the graph's own largest hop may be smaller)
                blocks = HopBlocks(blocks.code, blocks.node_off, blocks.code_off, [self.sizes[g]], self.D - 2)
            x, cnt, up = self.xs[g], self.cnt[lo:hi].contiguous(), (up[g:g + 1] if graph_sum else up[lo:hi])
        out = _BatchedGraphsPre.apply(x.to(DEV), blocks, graph_sum, (self.L, self.H, self.C, self.F), (self.L, self.H, 1), cnt, dropout,
                                      *fl, *rl)
        saved = out.grad_fn.saved_tensors
        left = (saved[1].detach().clone(), saved[2].detach().clone())
        grads = torch.autograd.grad(out, [t for t in fl + rl if t is not None], up.to(DEV, torch.float32))
        return out.detach(), grads, left

    def chain(self, dtype, graph_sum):
        outs, Ss, luts, total = [], [], [], None
        for g in range(self.G):
            out, grads, (S, lut) = self.sub(g, graph_sum).chain(dtype)
            outs.append(out.view(1, -1) if graph_sum else out)
            Ss.append(S)
            luts.append(lut)
            total = list(grads) if total is None else [a + b for a, b in zip(total, grads)]
        return torch.cat(outs), total, (torch.cat(Ss), torch.cat(luts))


BUILDS = {"NB1": [1, 5, 33, 64], "NB2": [1, 2, 63, 64, 65, 128, 30]}
#          D, C, L, H, bias_f, bias_rho, F
STACKS = [(2, 1, 3, 64, True, False, 7), (7, 3, 2, 30, True, False, 4), (64, 8, 3, 48, False, True, 3)]
CASES = [(b, s, gs) for b in BUILDS for s in range(len(STACKS)) for gs in (False, True)]
IDS = ["%s-D%d-C%d-L%d-H%d-%s" % (b, *STACKS[s][:4], "sum" if gs else "nodes") for b, s, gs in CASES]


@functools.lru_cache(maxsize=None)
def _batch(build, s):
    _need_gpu()
    D, C, L, H, bias_f, bias_r, F = STACKS[s]
    return _Batch(BUILDS[build], F, D, C, L, H, bias_f, bias_r)


@functools.lru_cache(maxsize=None)
def _truth(build, s, graph_sum, dtype=torch.float64):
    """The chain of a batch: computed once, shared, never changed."""
    return _batch(build, s).chain(dtype, graph_sum)


@functools.lru_cache(maxsize=None)
def _got(build, s, graph_sum):
    return _batch(build, s).device(graph_sum)


@pytest.mark.parametrize("build,s,graph_sum", CASES, ids=IDS)
def test_batches_against_the_chain_graph_by_graph(build, s, graph_sum):
    b = _batch(build, s)
    assert b.D == STACKS[s][0] and b.blocks.max_nodes == max(BUILDS[build])
    got, got_g, (S, lut) = _got(build, s, graph_sum)
    want, want_g, (want_S, want_lut) = _truth(build, s, graph_sum)
    lazy = lambda: _truth(build, s, graph_sum, torch.float32)          # noqa: E731
    assert got.shape == want.shape == ((b.G, b.C) if graph_sum else (b.N, b.C)) and lut.shape == (b.N * b.D, 1)
    assert_rule(got, want, lambda: lazy()[0], "forward")
    assert_rule(S, want_S, lambda: lazy()[2][0], "S")
    for g in range(b.G):                                               # the rows' table of every graph, on its own scale
        lo, hi = b.off[g] * b.D, b.off[g + 1] * b.D
        assert_rule(lut[lo:hi], want_lut[lo:hi], lambda: lazy()[2][1][lo:hi], "lut of graph %d" % g)
    assert_grads_rule(list(got_g), list(want_g), lambda: list(lazy()[1]), "gradients")
    again, again_g, (again_S, again_lut) = b.device(graph_sum)
    assert torch.equal(got, again) and all(torch.equal(a, c) for a, c in zip(got_g, again_g))
    assert torch.equal(S, again_S) and torch.equal(lut, again_lut)
    if b.D == 64:                                                      # most (row, shell) arguments are shells no pair lies in
        empty = sum(int((c == 0).sum()) for c in b.cnts)
        assert empty > b.N * b.D // 2


@pytest.mark.parametrize("D", [2, 11, 64])
@pytest.mark.parametrize("n", [1, 30, 64, 65, 128])
def test_a_batch_of_one_has_the_one_graph_kernels_bits(n, D):
    """node_off = [0, n]: outputs, S, lut and every gradient are torch.equal to gnan_small_graph_fwd / _bwd with pre_rho = 1 (which
    lends its backward a workspace)."""
    _need_gpu()
    from gnan_amd.batched import HopBlocks, _BatchedGraphsPre
    F, C, L, H = 5, 2, 3, 32
    rng = np.random.default_rng(100 * n + D)
    hops = _hops(rng, n, D, top=True)
    fp, rp = _mlps(rng, F, C, L, H, True, True)
    x = torch.from_numpy(rng.standard_normal((n, F)).astype(np.float32))
    for graph_sum in (False, True):
        case = _Case(hops, x, fp, rp, L, H, C, graph_sum)
        assert case.D == (D if n > 1 else 2)
        want, want_g, (want_S, want_lut) = case.device("small")
        blocks = HopBlocks.from_blocks([torch.from_numpy(hops).float().to(DEV)])
        assert blocks.n_codes == case.D and blocks.max_nodes == n
        fl, rl = case.leaves(torch.float32, DEV)
        out = _BatchedGraphsPre.apply(x.to(DEV), blocks, graph_sum, (L, H, C, F), (L, H, 1), case.g.cnt, None, *fl, *rl)
        saved = out.grad_fn.saved_tensors
        grads = torch.autograd.grad(out, [t for t in fl + rl if t is not None], case.up.to(DEV, torch.float32).reshape(out.shape))
        assert torch.equal(out.detach().reshape(want.shape), want), (n, D, graph_sum)
        assert torch.equal(saved[1], want_S) and torch.equal(saved[2], want_lut) and saved[2].shape == (n * case.D, 1)
        assert len(grads) == len(want_g) and all(torch.equal(a, w) for a, w in zip(grads, want_g)), (n, D, graph_sum)


def test_offsets_a_graph_of_the_batch_has_the_bits_of_the_graph_alone():
    b = _batch("NB2", 1)
    for graph_sum in (False, True):
        got, _, (S, lut) = _got("NB2", 1, graph_sum)
        for g in range(b.G):
            lo, hi = b.off[g], b.off[g + 1]
            alone, _, (alone_S, alone_lut) = b.device(graph_sum, only=g)
            assert torch.equal(got[g:g + 1] if graph_sum else got[lo:hi], alone), (g, graph_sum)
            assert torch.equal(S[lo:hi], alone_S) and torch.equal(lut[lo * b.D:hi * b.D], alone_lut), (g, graph_sum)


def test_slots_hold_graphs_of_their_own_codes_and_sizes():
    """SlotGraph(n_codes=16) loaded in turn with graphs of D = 16, 3, 9 codes and 64 and 4 nodes — each smaller graph after a larger
    one: the read-out and the gradients meet the chain on the graph's OWN D, so stale rows and codes past n are never read."""
    _need_gpu()
    from gnan_amd.functional import StackedMLP
    from gnan_amd.small_graph import SlotGraph, slot_graph_applies, slot_graph_forward
    F, C, L, H = 6, 2, 3, 32
    rng = np.random.default_rng(16)
    fp, rp = _mlps(rng, F, C, L, H, True, True)
    slot = SlotGraph(F, DEV, use_cnt=True, max_nodes=64, n_codes=16)
    for n, D in ((64, 16), (4, 3), (64, 9), (4, 16), (64, 3), (4, 9)):
        hops = _hops(rng, n, D, top=True)
        x = torch.from_numpy(rng.standard_normal((n, F)).astype(np.float32))
        case = _Case(hops, x, fp, rp, L, H, C, True)
        assert case.D == D and slot.fits(case.g, x.to(DEV))
        slot.load(case.g, x.to(DEV))
        fl, rl = case.leaves(torch.float32, DEV)
        f, r = StackedMLP(*fl, L, H, C, F), StackedMLP(*rl, L, H, 1, 1)
        assert slot_graph_applies(slot, f, r)
        out = slot_graph_forward(slot, f, r, "pre")
        grads = torch.autograd.grad(out, [t for t in fl + rl if t is not None], case.up.to(DEV, torch.float32))
        want, want_g, _ = case.chain(torch.float64)
        lazy = functools.lru_cache(maxsize=None)(lambda case=case: case.chain(torch.float32))
        assert out.shape == want.shape == (C, 1)
        assert_rule(out.detach(), want, lambda: lazy()[0], "read-out n=%d D=%d" % (n, D))
        assert_grads_rule(list(grads), list(want_g), lambda: list(lazy()[1]), "gradients n=%d D=%d" % (n, D))


# ---- the Dropout twins ------------------------------------------------------------------------------------------------------------
_cell = cap_tests._cell


def test_dropout_p_zero_is_the_plain_kernel_bit_for_bit():
    b = _batch("NB2", 1)
    for graph_sum in (False, True):
        plain, plain_g, (plain_S, plain_lut) = _got("NB2", 1, graph_sum)
        zero, zero_g, (zero_S, zero_lut) = b.device(graph_sum, dropout=(0.0, _cell(SEED)))
        assert torch.equal(plain, zero) and all(torch.equal(a, c) for a, c in zip(plain_g, zero_g))
        assert torch.equal(plain_S, zero_S) and torch.equal(plain_lut, zero_lut)


@pytest.mark.parametrize("n", [30, 128])
def test_a_seed_cell_on_a_batch_of_one_gives_the_one_graph_dropout_bits(n):
    _need_gpu()
    from gnan_amd.batched import HopBlocks, _BatchedGraphsPre
    from gnan_amd.functional import StackedMLP
    from gnan_amd.small_graph import small_graph_forward
    F, C, L, H, D = 5, 2, 3, 32, 11
    rng = np.random.default_rng(n)
    hops = _hops(rng, n, D, top=True)
    fp, rp = _mlps(rng, F, C, L, H, True, True)
    x = torch.from_numpy(rng.standard_normal((n, F)).astype(np.float32)).to(DEV)
    case = _Case(hops, x.cpu(), fp, rp, L, H, C, True)
    up = case.up.to(DEV, torch.float32)

    def run(fn):
        fl, rl = case.leaves(torch.float32, DEV)
        out = fn(fl, rl)
        saved = out.grad_fn.saved_tensors
        return out.detach().reshape(-1), torch.autograd.grad(out, [t for t in fl + rl if t is not None], up.reshape(out.shape)), saved[2]
    want, want_g, want_lut = run(lambda fl, rl: small_graph_forward(x, case.g, StackedMLP(*fl, L, H, C, F), StackedMLP(*rl, L, H, 1, 1),
                                                                    "pre", True, dropout=(P, SEED)))
    blocks = HopBlocks.from_blocks([torch.from_numpy(hops).float().to(DEV)])
    batch = lambda drop: run(lambda fl, rl: _BatchedGraphsPre.apply(x, blocks, True, (L, H, C, F), (L, H, 1), case.g.cnt, drop,
                                                                    *fl, *rl))          # noqa: E731
    got, got_g, got_lut = batch((P, _cell(SEED)))
    assert torch.equal(got, want) and all(torch.equal(a, w) for a, w in zip(got_g, want_g)) and torch.equal(got_lut, want_lut)
    other, _, other_lut = batch((P, _cell(SEED + 1)))
    plain, _, plain_lut = batch(None)
    assert not torch.equal(other, got) and not torch.equal(plain, got)                    # the masks matter, and follow the cell
    assert torch.equal(other_lut, got_lut) and torch.equal(plain_lut, got_lut)            # ... and rho is never masked


class _DropBatch(cap_tests._Batch):
    """test_gpu_dropout_capture's batch (its chain: the oracle's pieces under ``gnan_dropout_mask(seed, p, total_nodes, ...)``, one
    graph after the other) with pre-rho normalisation: O.row_lut_pre_rho on the CPU, ``_BatchedGraphsPre`` on the device."""

    def __init__(self, sizes, F, stack):
        super().__init__(sizes, F, stack)
        for sub in self.subs:
            sub.use_cnt = "pre"

    def fused(self, dropout, graph_sum):
        from gnan_amd.batched import _BatchedGraphsPre
        fl, rl = self.subs[0].leaves(torch.float32, DEV)
        fm, rm = (self.L, self.H, self.C, self.F), (self.L, self.H, 1)
        out = _BatchedGraphsPre.apply(self.x.to(DEV), self.blocks, graph_sum, fm, rm, self.cnt, dropout, *fl, *rl)
        live = [(i, t) for i, t in enumerate(fl + rl) if t is not None]
        grads = torch.autograd.grad(out, [t for _, t in live], self.up[graph_sum].to(DEV, torch.float32))
        return out.detach(), {i: g for (i, _), g in zip(live, grads)}


@functools.lru_cache(maxsize=None)
def _drop_batch():
    _need_gpu()
    return _DropBatch((30, 65, 7), 5, cap_tests.A)


@pytest.mark.parametrize("graph_sum", [True, False], ids=["Ysum", "Y"])
def test_a_three_graph_batch_under_dropout_against_the_chain(graph_sum):
    b = _drop_batch()
    got, got_g = b.fused((P, _cell(SEED)), graph_sum)
    want, want_g = b.chain(torch.float64, graph_sum)
    lazy = functools.lru_cache(maxsize=None)(lambda: b.chain(torch.float32, graph_sum))
    assert got.shape == want.shape == ((3, b.C) if graph_sum else (b.N, b.C)) and sorted(got_g) == sorted(want_g)
    assert_rule(got, want, lambda: lazy()[0], "forward")
    assert_grads_rule(got_g, want_g, lambda: lazy()[1], "gradients")
    plain, _ = b.fused(None, graph_sum)
    assert float((plain.cpu().double() - want).abs().max()) > 1e-3 * float(want.abs().max())          # the masks matter
    again, again_g = b.fused((P, _cell(SEED)), graph_sum)
    assert torch.equal(got, again) and all(torch.equal(got_g[k], again_g[k]) for k in got_g)


# ---- the modules -----------------------------------------------------------------------------------------------------------------
SIZES = [12, 23, 30, 41, 64, 70, 128, 130]


@functools.lru_cache(maxsize=None)
def _graphs():
    _need_gpu()
    return _graph_task(14, 15, sizes=SIZES, seed=24)


def _model(dropout=0.0, seed=0):
    from gnan_amd import GNAN as standalone
    torch.manual_seed(seed)
    m = standalone.TensorGNAN(15, 1, 3, hidden_channels=32, is_graph_task=True, dropout=dropout, device=DEV)
    assert m.normalize_rho is True                                    # the class's default
    with torch.no_grad():
        for _, p in m.named_parameters():
            p.copy_(torch.randn(p.shape) * 0.3)
    return m.to(DEV).train() if dropout else m.to(DEV).eval()


def _epochs(m, opt, graphs, n):
    from gnan_amd import harness
    loss_fn = torch.nn.BCEWithLogitsLoss()
    return [harness.train_epoch(m, graphs, loss_fn, opt, DEV, classify=True, is_graph_task=True)[:2] for _ in range(n)]


def test_harness_epochs_run_from_slot_steps(monkeypatch):
    """Four epochs of harness.train_epoch over 14 graphs of 12 to 130 nodes: every graph of <= 128 nodes replays from a slot step
    (at most six, no per-shape capture), the 130-node graph keeps its route; losses and parameters track an eager twin."""
    from gnan_amd import harness, small_graph
    graphs = _graphs()
    runs = {}
    for on in (False, True):
        monkeypatch.setattr(harness, "GRAPHED_STEPS", on)
        m = _model()
        assert small_graph.slot_mode(m) == "pre"
        opt = torch.optim.Adam(m.parameters(), lr=1e-3)
        runs[on] = (_epochs(m, opt, graphs, 4), {k: v.detach().clone() for k, v in m.state_dict().items()}, m)
    for a, b in zip(runs[False][0], runs[True][0]):
        assert abs(a[0] - b[0]) <= 1e-5 * max(1.0, abs(a[0])) and a[1] == b[1], (a, b)
    scale = max(float(v.abs().max()) for v in runs[False][1].values())
    for k, v in runs[False][1].items():
        assert float((v - runs[True][1][k]).abs().max()) <= 1e-5 * scale, k
    steps = harness._steps_of(runs[True][2]).graph
    n_fit = sum(d.x.shape[0] <= 128 for d in graphs)
    assert 2 <= len(steps.slots) <= 6 and {t[0] for t in steps.slots} == {64, 128}
    replays = sum(s.step.graph.replays for s in steps.slots.values())
    print("slot steps", len(steps.slots), "replays", replays, "kernel nodes", [s.step.graph.kernel_nodes for s in steps.slots.values()])
    assert replays >= 4 * n_fit - 3, (replays, n_fit)                  # from the third step of the first epoch on
    assert all(s.step.graph.kernel_nodes <= 7 for s in steps.slots.values())
    assert all(key[0] > 128 for key, rec in steps.buckets.items() if rec["step"] is not None)
    assert any(key[0] == 130 for key in steps.buckets)                 # the 130-node graph: its own per-shape route, as before
    harness.release_steps(runs[True][2])


def test_the_switch_off_is_the_route_as_before(monkeypatch):
    from gnan_amd import harness, small_graph
    monkeypatch.setattr(small_graph, "SLOT_PRE_RHO", False)
    graphs = _graphs()[:4]
    m = _model()
    assert small_graph.slot_mode(m) is None
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    _epochs(m, opt, graphs, 3)
    steps = harness._steps_of(m).graph
    assert not steps.slots and any(rec["step"] is not None for rec in steps.buckets.values())      # a captured step per shape
    with torch.no_grad():
        for _ in range(4):
            for d in graphs:
                m.forward(d)
    assert "_replay_slots" not in m.__dict__                           # the modules' own replay: no slot plan either
    harness.release_steps(m)


def test_a_plain_loop_replays_from_slot_plans():
    """The caller's own unchanged loop (another graph object every step) through replay.run: forward and backward replay from the
    slot plans and give the eager twin's outputs and gradients."""
    from gnan_amd import replay
    graphs = [d for d in _graphs() if d.x.shape[0] <= 128][:6]

    def loop(m, passes=3):
        outs = []
        for _ in range(passes):
            for d in graphs:
                m.zero_grad(set_to_none=True)
                out = m.forward(d)
                out.pow(2).sum().backward()
                outs.append((out.detach().clone(), {k: p.grad.detach().clone() for k, p in m.named_parameters()}))
        return outs
    on_model, off_model = _model(), _model()
    on = loop(on_model)
    old = replay.REPLAY_FORWARD
    replay.REPLAY_FORWARD = False
    try:
        off = loop(off_model)
    finally:
        replay.REPLAY_FORWARD = old
    for s, ((a, a_g), (b, b_g)) in enumerate(zip(on, off)):
        assert float((a - b).abs().max()) <= TWO_FLOORS * float(b.abs().max()), s
        scale = max(float(v.abs().max()) for v in b_g.values())
        for k in b_g:
            assert float((a_g[k] - b_g[k]).abs().max()) <= TWO_FLOORS * scale, (s, k)
    plans = [rec["plan"] for rec in on_model.__dict__["_replay_slots"].plans.values() if rec["plan"] is not None]
    assert plans and sum(p.fwd.replays for p in plans) >= len(on) - 3 and all(p.bwd.replays == p.fwd.replays for p in plans)
    assert "_replay_slots" not in off_model.__dict__
    replay.release(on_model)


def test_the_slot_step_is_captured_under_dropout(monkeypatch):
    """CAPTURE_DROPOUT and dropout = 0.6: the slot step is captured over the ``_drop_dev`` twins; an epoch replayed under one
    manual_seed matches the eager twin from the same state under the same seed (test_gpu_dropout_capture's comparison)."""
    from gnan_amd import harness, small_graph
    monkeypatch.setattr(small_graph, "CAPTURE_DROPOUT", True)
    graphs = _graph_task(8, 15, sizes=[20, 33, 27, 40, 24, 38, 31, 22], seed=5)
    loss_fn = torch.nn.BCEWithLogitsLoss()
    m = _model(dropout=P)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                # (the one-time note of _check_dropout)
        harness.train_epoch(m, graphs, loss_fn, opt, DEV, classify=True, is_graph_task=True)      # two eager steps, then the capture
        steps = harness._graph_task_steps(m, opt, loss_fn, True, DEV)
        assert steps.captured >= 1 and steps.slot is not None and steps.slot.step.cell is not None
        twin = copy.deepcopy(m)
        twin_opt = torch.optim.Adam(twin.parameters(), lr=1e-3)
        twin_opt.load_state_dict(copy.deepcopy(opt.state_dict()))
        replays = lambda: sum(s.step.graph.replays for s in steps.slots.values())      # noqa: E731
        for seed in (17, 18):                                          # two replayed epochs, each against the eager twin's under its seed
            before = replays()
            torch.manual_seed(seed)
            got = harness.train_epoch(m, graphs, loss_fn, opt, DEV, classify=True, is_graph_task=True)
            assert replays() == before + len(graphs)
            with monkeypatch.context() as mp:
                mp.setattr(harness, "GRAPHED_STEPS", False)
                torch.manual_seed(seed)
                want = harness.train_epoch(twin, graphs, loss_fn, twin_opt, DEV, classify=True, is_graph_task=True)
            assert abs(got[0] - want[0]) <= TWO_FLOORS * max(abs(want[0]), 1e-30), (seed, got, want)
    assert all(bool(torch.isfinite(p).all()) for p in m.parameters())
    harness.release_steps(m)
