"""Training-mode Dropout in captured steps: the seed in a device cell (gnan_dropout_seed_set, the *_drop_dev entry points), Dropout
on the batched / slot kernels (gnan_small_batch_fwd_drop_dev / _bwd_drop_dev), the modules' own replay and ``harness.train_epoch``
under ``dropout = 0.6`` in ``train()`` mode, and the gates that stay shut.

Tolerances: the project's rule (helpers.assert_rule / assert_grads_rule: the float32 oracle chain's own error beyond the floor)
against the float64 oracle chain, TWO_FLOORS between two routes of the build."""
import copy
import functools
import warnings

import numpy as np
import pytest
import torch

from helpers import TWO_FLOORS, assert_grads_rule, assert_rule
from test_gpu_graphed import DEV, _graph_task, _need_gpu, _node_task
from test_gpu_small_graph_dropout import CASES, P, SEED, _Case, _case, _graph_cached, _model

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def capture_dropout_on(monkeypatch):
    """``small_graph.CAPTURE_DROPOUT`` ships off: everything here runs with it on — the gates that stay shut
    stay shut WITH the switch on — and one case switches it off again."""
    from gnan_amd import small_graph
    monkeypatch.setattr(small_graph, "CAPTURE_DROPOUT", True)


def _cell(seed):
    from gnan_amd.small_graph import seed_cell, seed_cell_set
    c = seed_cell(DEV)
    seed_cell_set(c, seed)
    return c


# ---- a cell that holds SEED == the by-value call with SEED -------------------------------------------------------------------------
# n = 1, 64, 65, 128: the small route's one and two node blocks; 129, 200, 448: the mid route's tile edge, padded stride, seven tiles
DEV_SEED_CASES = [next(i for i, c in enumerate(CASES) if c[0] == n and c[1] == F and c[3] != "pre")
                  for n, F in ((1, 1), (64, 15), (65, 15), (128, 15), (129, 15), (200, 15), (448, 15))]


@pytest.mark.parametrize("i", DEV_SEED_CASES, ids=["n%d" % CASES[i][0] for i in DEV_SEED_CASES])
def test_a_seed_cell_gives_the_bits_of_the_by_value_seed(i):
    from gnan_amd.small_graph import seed_cell_set
    case = _case(i)
    want, want_g = case.fused((P, SEED))
    cell = _cell(SEED)
    assert int(cell.item()) & ((1 << 64) - 1) == SEED
    got, got_g = case.fused((P, cell))
    assert torch.equal(got, want) and sorted(got_g) == sorted(want_g)
    assert all(torch.equal(got_g[k], want_g[k]) for k in want_g)
    # rewriting the cell — nothing else — changes the masks: to those of the by-value call with the new seed
    seed_cell_set(cell, SEED + 1)
    other, other_g = case.fused((P, cell))
    nxt, nxt_g = case.fused((P, SEED + 1))
    assert not torch.equal(other, want)
    assert torch.equal(other, nxt) and all(torch.equal(other_g[k], nxt_g[k]) for k in nxt_g)
    # p == 0: the plain kernels, and the cell is never read (any address will do as long as it is not NULL)
    plain, plain_g = case.fused(None)
    zero, zero_g = case.fused((0.0, cell))
    assert torch.equal(plain, zero) and all(torch.equal(plain_g[k], zero_g[k]) for k in plain_g)


def test_a_device_seed_backward_is_one_launch_or_nothing():
    """Only f's gradients wanted: the general backward would run — it takes its seed by value, so a cell is refused loudly."""
    case = _case(DEV_SEED_CASES[1])
    with pytest.raises(RuntimeError, match="seed in a device cell"):
        case.fused((P, _cell(SEED)), r_grad=False)


# ---- Dropout on the batched kernels against the oracle chain -------------------------------------------------------------------------
A, C8 = (3, 64, 1, True), (2, 8, 8, True)
BATCHES = {"NB1": ((1, 30, 64), 5, A), "NB2": ((65, 128, 7), 3, C8), "twins": ((30, 30), 5, A)}


class _Batch:
    """Graphs of a batch with ONE pair of stacks: on the device through ``_BatchedGraphs`` with the slots' semantics (``cnt``,
    ``raw_hops=False``), on the CPU as one oracle chain per graph (``_Case.chain``) whose gradients add up."""

    def __init__(self, sizes, F, stack, same_x=False):
        from gnan_amd.batched import HopBlocks
        self.sizes, self.F, (self.L, self.H, self.C, bias) = sizes, F, stack
        rng = np.random.default_rng(sum(sizes) + F)
        base = _Case(sizes[0], F, stack, True, True)           # (its parameter tensors; its graph is not used)
        self.fp, self.rp = base.fp, base.rp
        hops = []
        for g, n in enumerate(sizes):
            h = hops[0] if (same_x and g) else rng.integers(-1, 6, (n, n)).astype(np.int32)
            h[np.arange(n), np.arange(n)] = 0
            hops.append(h)
        self.blocks = HopBlocks.from_blocks([torch.from_numpy(h).float().to(DEV) for h in hops])
        self.D = D = self.blocks.n_codes
        self.N = sum(sizes)
        xs = [torch.from_numpy(rng.standard_normal((n, F)).astype(np.float32)) for n in sizes]
        if same_x:
            xs = [xs[0]] * len(sizes)
        self.x = torch.cat(xs)
        self.subs = []
        for h, x in zip(hops, xs):
            sub = _Case.__new__(_Case)
            sub.n, sub.F, sub.L, sub.H, sub.C, sub.use_cnt, sub.D = h.shape[0], F, self.L, self.H, self.C, True, D
            sub.codes = torch.from_numpy(np.where(h >= 0, h, D - 1)).long()
            sub.cnt = np.stack([(sub.codes.numpy() == d).sum(1) for d in range(D)], axis=1).astype(np.int32)
            sub.fp, sub.rp, sub.x = self.fp, self.rp, x
            self.subs.append(sub)
        self.cnt = torch.from_numpy(np.concatenate([s.cnt for s in self.subs])).to(DEV)
        self.up = {True: torch.from_numpy(rng.standard_normal((len(sizes), self.C))),
                   False: torch.from_numpy(rng.standard_normal((self.N, self.C)))}

    def fused(self, dropout, graph_sum):
        from gnan_amd.batched import _BatchedGraphs
        fl, rl = self.subs[0].leaves(torch.float32, DEV)
        fm, rm = (self.L, self.H, self.C, self.F), (self.L, self.H, 1)
        out = _BatchedGraphs.apply(self.x.to(DEV), self.blocks, graph_sum, fm, rm, self.cnt, False, dropout, *fl, *rl)
        live = [(i, t) for i, t in enumerate(fl + rl) if t is not None]
        grads = torch.autograd.grad(out, [t for _, t in live], self.up[graph_sum].to(DEV, torch.float32))
        return out.detach(), {i: g for (i, _), g in zip(live, grads)}

    def masks(self, seed=SEED):
        from gnan_amd.functional import dropout_masks
        return dropout_masks(seed, P, self.N, self.F, self.L - 1, self.H, DEV).cpu()         # the BATCH's mask tensor

    def chain(self, dtype, graph_sum):
        keep, outs, total, lo = self.masks(), [], {}, 0
        for g, sub in enumerate(self.subs):
            sub.graph_sum = graph_sum
            sub.up = self.up[True][g].view(-1, 1) if graph_sum else self.up[False][lo:lo + sub.n]
            out, grads = sub.chain(dtype, keep[lo:lo + sub.n])                                 # node = the row of the packed x
            outs.append(out.view(1, -1) if graph_sum else out)
            for k, v in grads.items():
                total[k] = v if k not in total else total[k] + v
            lo += sub.n
        return torch.cat(outs), total


@functools.lru_cache(maxsize=None)
def _batch(name):
    _need_gpu()
    sizes, F, stack = BATCHES[name]
    return _Batch(sizes, F, stack, same_x=name == "twins")


@functools.lru_cache(maxsize=None)
def _batch_truth(name, graph_sum, dtype):
    return _batch(name).chain(dtype, graph_sum)


@pytest.mark.parametrize("graph_sum", [True, False], ids=["Ysum", "Y"])
@pytest.mark.parametrize("name", ["NB1", "NB2"])
def test_batch_kernels_against_the_oracle_chain(name, graph_sum):
    b = _batch(name)
    got, got_g = b.fused((P, _cell(SEED)), graph_sum)
    want, want_g = _batch_truth(name, graph_sum, torch.float64)
    assert got.shape == want.shape == ((len(b.sizes), b.C) if graph_sum else (b.N, b.C))
    assert sorted(got_g) == sorted(want_g)
    lazy = lambda: _batch_truth(name, graph_sum, torch.float32)             # noqa: E731
    assert_rule(got, want, lambda: lazy()[0], "forward")
    assert_grads_rule(got_g, want_g, lambda: lazy()[1], "gradients")


@pytest.mark.parametrize("name", ["NB1", "NB2"])
def test_graph_0_of_a_batch_and_a_slot_draw_the_one_graph_routes_masks(name):
    """Graph 0 sits at row 0 of the packed x, and so does a slot's graph: the masks of gnan_small_graph_fwd_drop for the seed."""
    from gnan_amd import HopGraph
    from gnan_amd.functional import StackedMLP
    from gnan_amd.small_graph import SlotGraph, slot_graph_forward, small_graph_forward
    b = _batch(name)
    sub = b.subs[0]
    n = sub.n
    hops = np.where(sub.codes.numpy() == b.D - 1, -1, sub.codes.numpy())
    nd = torch.zeros(n, n)
    nd[torch.from_numpy(hops >= 0)] = 1.0 / (torch.from_numpy(hops[hops >= 0]).float() + 1.0)
    g = HopGraph.from_dense(nd.to(DEV))
    x = sub.x.to(DEV)
    up = b.up[True][0].view(-1, 1).to(DEV, torch.float32)

    def run(fn):
        fl, rl = sub.leaves(torch.float32, DEV)
        f, r = StackedMLP(*fl, b.L, b.H, b.C, b.F), StackedMLP(*rl, b.L, b.H, 1, 1)
        out = fn(f, r)
        live = [t for t in fl + rl if t is not None]
        return out.detach(), torch.autograd.grad(out, live, up)
    want, want_g = run(lambda f, r: small_graph_forward(x, g, f, r, True, True, dropout=(P, SEED)))
    slot = SlotGraph(b.F, DEV, use_cnt=True, max_nodes=64 if n <= 64 else 128)
    assert slot.fits(g, x)
    slot.load(g, x)
    in_slot, slot_g = run(lambda f, r: slot_graph_forward(slot, f, r, True, dropout=(P, _cell(SEED))))
    batch_out, _ = b.fused((P, _cell(SEED)), True)
    scale = float(want.abs().max())
    assert float((in_slot - want).abs().max()) <= TWO_FLOORS * scale
    assert float((batch_out[0].view(-1, 1) - want).abs().max()) <= TWO_FLOORS * scale
    gscale = max(float(v.abs().max()) for v in want_g)
    for a, w in zip(slot_g, want_g):
        assert float((a - w).abs().max()) <= TWO_FLOORS * gscale


def test_two_graphs_with_identical_x_in_one_batch_get_different_masks():
    b = _batch("twins")
    out, _ = b.fused((P, _cell(SEED)), True)
    assert not torch.equal(out[0], out[1])                      # (the node coordinate is the row of the packed x)
    plain, _ = b.fused(None, True)
    assert torch.equal(plain[0], plain[1])                      # ... and without Dropout the twins agree


def test_the_batched_scripts_semantics_are_refused():
    from gnan_amd import _lib
    from gnan_amd.batched import _BatchedGraphs
    b = _batch("twins")
    fl, rl = b.subs[0].leaves(torch.float32, DEV)
    with pytest.raises(_lib.GnanHipError):
        _BatchedGraphs.apply(b.x.to(DEV), b.blocks, True, (b.L, b.H, b.C, b.F), (b.L, b.H, 1), None, True, (P, _cell(SEED)), *fl, *rl)
    with pytest.raises(_lib.GnanHipError):                     # a by-value seed: these kernels have no such entry point
        _BatchedGraphs.apply(b.x.to(DEV), b.blocks, True, (b.L, b.H, b.C, b.F), (b.L, b.H, 1), b.cnt, False, (P, SEED), *fl, *rl)


# ---- the modules replay ----------------------------------------------------------------------------------------------------------
class _Spy:
    """``_lib.lib()`` with the calls of the device-seed entry points (and of the seed store) noted."""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        fn = getattr(self.real, name)
        if not (name.endswith("_drop_dev") or name == "gnan_dropout_seed_set"):
            return fn

        def counted(*args):
            self.calls.append(name)
            return fn(*args)
        return counted


@pytest.fixture
def spy(monkeypatch):
    from gnan_amd import _lib
    s = _Spy(_lib.lib())
    monkeypatch.setattr(_lib, "lib", lambda: s)
    return s


@functools.lru_cache(maxsize=None)
def _small_graphs():
    _need_gpu()
    return _graph_task(4, 15, sizes=[20, 33, 27, 40], seed=11)


def _loop(m, graphs, steps=8, seed=21):
    """The reference's loop shape without its optimizer: ``steps`` forwards and backwards under ONE manual_seed."""
    torch.manual_seed(seed)
    outs = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                # (the one-time note of _check_dropout)
        for s in range(steps):
            m.zero_grad(set_to_none=True)
            out = m.forward(graphs[s % len(graphs)])
            out.pow(2).sum().backward()
            outs.append((out.detach().clone(), {k: p.grad.detach().clone() for k, p in m.named_parameters()}))
    return outs


def _plans(m):
    """Every replay plan ``m`` holds: the slot tiers' and the per-object ones."""
    found = [rec["plan"] for rec in getattr(m.__dict__.get("_replay_slots"), "plans", {}).values()]
    cache = m.__dict__.get("_replays")
    found += [e.value["plan"] for e in cache.entries.values()] if cache is not None else []
    return [p for p in found if p is not None]


@pytest.mark.parametrize("kind,route", [("models_tensor", "slots"), ("models_tensor", "per-object"), ("models_gnan", "slots"),
                                        ("models_gnan", "per-object")])
def test_a_replayed_loop_is_the_eager_loops_twin(kind, route, spy, monkeypatch):
    from gnan_amd import replay
    graphs = _small_graphs() if route == "slots" else [_graph_cached(130)]
    on_model, off_model = _model(kind), _model(kind)
    assert on_model.training and on_model._dropout_active()
    on = _loop(on_model, graphs)
    seen = list(spy.calls)
    del spy.calls[:]
    with monkeypatch.context() as mp:
        mp.setattr(replay, "REPLAY_FORWARD", False)
        off = _loop(off_model, graphs)
    assert spy.calls == []                                             # the eager path: the by-value entry points only
    for s, ((a, a_g), (b, b_g)) in enumerate(zip(on, off)):
        assert float((a - b).abs().max()) <= TWO_FLOORS * float(b.abs().max()), s
        scale = max(float(v.abs().max()) for v in b_g.values())
        assert sorted(a_g) == sorted(b_g)
        for k in b_g:
            assert float((a_g[k] - b_g[k]).abs().max()) <= TWO_FLOORS * scale, (s, k)
    if kind == "models_gnan" and route == "slots":
        assert not _plans(on_model) and seen == []                     # node outputs of a small graph: no slot route, eager as ever
        return
    plans = _plans(on_model)
    assert len(plans) == 1 and plans[0].gen >= 3 and plans[0].cell is not None
    assert seen.count("gnan_dropout_seed_set") == plans[0].gen         # one seed store (one draw) per replayed forward
    # two consecutive replays on the same graph differ: the masks are not frozen
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gen = plans[0].gen
        one = on_model.forward(graphs[0]).detach().clone()
        two = on_model.forward(graphs[0]).detach().clone()
        assert plans[0].gen == gen + 2 and not torch.equal(one, two)
        # the same manual_seed twice: equal bits
        torch.manual_seed(5)
        three = on_model.forward(graphs[0]).detach().clone()
        torch.manual_seed(5)
        four = on_model.forward(graphs[0]).detach().clone()
        assert torch.equal(three, four) and not torch.equal(three, one)
        # eval(): the Dropout-free forward, bit for bit — a twin that never had Dropout, on the same route (a copied model starts
        # without plans: two eager forwards put it where the replayed model is)
        twin = copy.deepcopy(on_model)
        twin.dropout = 0.0
        twin.train()
        on_model.eval()
        with torch.no_grad():
            for _ in range(2):
                twin.forward(graphs[0])
            for _ in range(4):
                got = on_model.forward(graphs[0])
                assert torch.equal(got, twin.forward(graphs[0])) and got.shape == one.shape and not torch.equal(got, one)
        replay.release(twin)
    replay.release(on_model)


@pytest.mark.parametrize("gate", ["readout", "node_ids", "449 nodes", "only f's gradients", "batched", "harness node task",
                                  "CAPTURE_DROPOUT off"])
def test_the_gates_stay_shut_under_dropout(gate, spy, monkeypatch):
    """What the device-seed routes do not cover runs eagerly exactly as before: no ``_dev`` call, no seed store, no new warning —
    the same bits as with replay switched off under the same manual_seed."""
    from gnan_amd import batched, harness, models, replay, small_graph
    data, kw, steps = _graph_cached(30), {}, 5
    make = lambda: _model("models_tensor")                             # noqa: E731
    if gate == "readout":
        def make():
            torch.manual_seed(0)
            return models.TensorGNAN(15, 1, 3, hidden_channels=32, dropout=P, is_graph_task=True, readout_n_layers=1,
                                     device=DEV).to(DEV).train()
    elif gate == "node_ids":
        make, kw, data = (lambda: _model("models_gnan")), {"node_ids": [0, 3, 129]}, _graph_cached(130)
    elif gate == "449 nodes":
        data = _graph_cached(449)
    elif gate == "only f's gradients":
        def make():
            m = _model("models_tensor")
            for p in m.rho.parameters():
                p.requires_grad_(False)
            return m
        data = _graph_cached(130)
    elif gate == "CAPTURE_DROPOUT off":
        monkeypatch.setattr(small_graph, "CAPTURE_DROPOUT", False)

    def run(m):
        torch.manual_seed(3)
        outs = []
        for _ in range(steps):
            m.zero_grad(set_to_none=True)
            if gate == "batched":
                out = m.forward(*data)
            elif gate == "harness node task":
                outs.append(harness.train_epoch(m, [data], torch.nn.CrossEntropyLoss(), opt[id(m)], DEV, classify=True,
                                                is_graph_task=False)[0])
                continue
            else:
                out = m.forward(data, **kw)
            out.pow(2).sum().backward()
            outs.append(out.detach().clone())
        return outs
    opt = {}
    if gate == "batched":
        g = _small_graphs()
        blocks = batched.HopBlocks.from_blocks([torch.round(1.0 / d.node_distances.clamp_min(1e-9) - 1.0).masked_fill(
            d.node_distances <= 0, -1.0) for d in g[:2]])
        bv = torch.cat([torch.full((d.x.shape[0],), i, dtype=torch.long) for i, d in enumerate(g[:2])]).to(DEV)
        data = (torch.cat([d.x for d in g[:2]]), blocks, bv)

        def make():
            torch.manual_seed(0)
            return batched.TensorGNAN(15, 1, 2, hidden_channels=16, dropout=P, device=DEV).to(DEV).train()
    elif gate == "harness node task":
        data = _node_task(600, 9, 4, False)                            # (a CSR graph: what a full-batch node task trains on)

        def make():
            torch.manual_seed(0)
            m = models.TensorGNAN(9, 4, 3, hidden_channels=16, dropout=P, device=DEV).to(DEV).train()
            opt[id(m)] = torch.optim.Adam(m.parameters(), lr=1e-3)
            return m
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        got = run(make())
    assert spy.calls == []
    assert not [w for w in seen if "Dropout" not in str(w.message) and "gnan_amd" in str(w.message)], [str(w.message) for w in seen]
    with monkeypatch.context() as mp, warnings.catch_warnings():
        warnings.simplefilter("ignore")
        mp.setattr(replay, "REPLAY_FORWARD", False)
        mp.setattr(harness, "GRAPHED_STEPS", False)
        want = run(make())
    if gate == "batched":
        return                                                         # (its rho draws torch's own masks and sums with atomics: no bits to compare)
    for a, b in zip(got, want):
        assert torch.equal(a, b) if torch.is_tensor(a) else abs(a - b) <= 1e-6 * max(1.0, abs(b))


# ---- harness.train_epoch ---------------------------------------------------------------------------------------------------------
def test_harness_epochs_replay_the_slot_step_under_dropout(monkeypatch):
    from gnan_amd import harness, models
    _need_gpu()
    graphs = _graph_task(8, 15, sizes=[20, 33, 27, 40, 24, 38, 31, 22], seed=5)
    loss_fn = torch.nn.BCEWithLogitsLoss()
    torch.manual_seed(0)
    m = models.TensorGNAN(15, 1, 3, hidden_channels=32, dropout=P, is_graph_task=True, readout_n_layers=0, device=DEV)
    with torch.no_grad():
        for _, p in m.named_parameters():
            p.copy_(torch.randn(p.shape) * 0.3)
    m = m.to(DEV).train()
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                # (the one-time note of _check_dropout)
        harness.train_epoch(m, graphs, loss_fn, opt, DEV, classify=True, is_graph_task=True)      # two eager steps, then the capture
        steps = harness._graph_task_steps(m, opt, loss_fn, True, DEV)
        assert steps.captured >= 1 and steps.slot is not None and steps.slot.step.cell is not None
        # the first epoch that is replayed from its first step on, against an eager twin from the same state under the same seed
        twin = copy.deepcopy(m)
        twin_opt = torch.optim.Adam(twin.parameters(), lr=1e-3)
        twin_opt.load_state_dict(copy.deepcopy(opt.state_dict()))
        replays = lambda: sum(s.step.graph.replays for s in steps.slots.values())      # noqa: E731  (a step per hop-code tier)
        before = replays()
        torch.manual_seed(17)
        got = harness.train_epoch(m, graphs, loss_fn, opt, DEV, classify=True, is_graph_task=True)
        assert replays() == before + len(graphs)
        with monkeypatch.context() as mp:
            mp.setattr(harness, "GRAPHED_STEPS", False)
            torch.manual_seed(17)
            want = harness.train_epoch(twin, graphs, loss_fn, twin_opt, DEV, classify=True, is_graph_task=True)
        assert abs(got[0] - want[0]) <= TWO_FLOORS * max(abs(want[0]), 1e-30), (got, want)
        for _ in range(2):
            harness.train_epoch(m, graphs, loss_fn, opt, DEV, classify=True, is_graph_task=True)
    assert all(bool(torch.isfinite(p).all()) for p in m.parameters())
    harness.release_steps(m)
