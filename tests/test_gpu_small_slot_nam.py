"""The NAM read-out on graph slots (csrc/small_graph_nam.hip: gnan_small_slot_nam_fwd / _bwd; small_graph.slot_graph_nam_forward):
the slot kernels against the one-graph kernels' bits, against the float64 chain, stale slots, ``harness.train_epoch`` /
``test_epoch`` and the modules' own replay through slot steps, the switch off, and Dropout.

Tolerances: bits (torch.equal) between the slot and the one-graph kernels; the project's rule (helpers.assert_rule /
assert_grads_rule: the float32 chain's own error beyond the 1e-5 floor) against the float64 chain; the bounds of
test_gpu_small_batch_pre.test_harness_epochs_run_from_slot_steps for its twin here."""
import functools
import warnings

import numpy as np
import pytest
import torch

from helpers import TWO_FLOORS, assert_grads_rule, assert_rule
from test_gpu_graphed import DEV, Bag, _graph_task, _need_gpu

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def switch_on(monkeypatch):
    """The route's switch follows a measured rule: the tests do not depend on how it ships."""
    from gnan_amd import small_graph
    monkeypatch.setattr(small_graph, "SLOT_NAM_READOUT", True)


def _model(F, C, Ln, bias=True, normalize=True, dropout=0.0, scale=0.4, seed=0):
    from gnan_amd import models
    torch.manual_seed(seed)
    m = models.TensorGNAN(F, C, 3, hidden_channels=32, bias=bias, is_graph_task=True, readout_n_layers=Ln, normalize_rho=normalize,
                          dropout=dropout, device=DEV)
    with torch.no_grad():
        for _, p in m.named_parameters():
            p.copy_(torch.randn(p.shape) * scale)
    return m.to(DEV).train() if dropout else m.to(DEV).eval()


def _stacks(m):
    return m._stacked("fs", m.fs), m._stacked("rho", [m.rho]), m.readout_nam._stacked("fs", m.readout_nam.fs)


def _hop_graph(rng, n, D, rest=True):
    """A dense-coded graph of exactly D codes (hops 0 .. D - 2, hop D - 2 listed) with (``rest``) or without unreachable pairs."""
    from gnan_amd import HopGraph
    hops = rng.integers(-1 if rest else 0, D - 1, (n, n)).astype(np.int32)
    hops[np.arange(n), np.arange(n)] = 0
    if n > 1:
        hops[0, 1] = D - 2
        if rest:
            hops[1, 0] = -1
    nd = torch.zeros(n, n)
    nd[torch.from_numpy(hops >= 0)] = 1.0 / (torch.from_numpy(hops[hops >= 0]).float() + 1.0)
    g = HopGraph.from_dense(nd.to(DEV))
    assert g.n_codes == (D if n > 1 else 2) and g.is_dense
    assert bool((g.code == 255).any()) == (rest and n > 1)
    return g


def _run(m, forward, up):
    """One forward + backward: (out, what the forward left, every parameter gradient)."""
    m.zero_grad(set_to_none=True)
    out = forward()
    left = out.grad_fn.saved_tensors
    (out * up).sum().backward()
    return out.detach().clone(), left, {k: p.grad.detach().clone() for k, p in m.named_parameters()}


#        n, cap, tier,  D,  F, Ln, C, bias, shell sizes, unreachable pairs
KERNEL_CASES = [
    (1, 64, 16, 2, 1, 1, 1, True, True, False),
    (2, 64, 16, 3, 15, 2, 3, False, False, True),
    (63, 64, 16, 16, 15, 3, 8, True, True, True),          # D equal to the tier; n * n = 1 mod 4
    (64, 64, 16, 9, 70, 1, 3, True, True, True),           # more than 64 features: the chunk loop of T
    (64, 64, 32, 20, 15, 2, 1, True, True, True),          # (the waves that bin: four for the graph's 20 shells, two for the tier's 32)
    (65, 128, 16, 16, 15, 2, 1, False, True, True),        # n * n = 1 mod 4, two node blocks
    (127, 128, 32, 20, 15, 3, 3, True, False, True),
    (128, 128, 64, 64, 70, 1, 8, True, True, True),        # both limits
    (128, 128, 16, 5, 1, 2, 8, True, True, False),
    (30, 128, 64, 12, 15, 3, 1, True, True, True),         # a small graph in the largest slots
]


@pytest.mark.parametrize("n,cap,tier,D,F,Ln,C,bias,use_cnt,rest", KERNEL_CASES,
                         ids=["n%d-cap%d-tier%d-D%d-F%d-L%d-C%d" % c[:7] for c in KERNEL_CASES])
def test_the_slot_kernels_give_the_one_graph_kernels_bits(n, cap, tier, D, F, Ln, C, bias, use_cnt, rest):
    """out, hidden, fx[:, :n], lut's listed hops and every gradient of f, rho and the read-out: torch.equal; two runs of the slot
    backward: equal bits."""
    _need_gpu()
    from gnan_amd import small_graph
    from gnan_amd.small_graph import (SlotGraph, slot_graph_nam_forward, slot_nam_applies, slot_tier, small_graph_nam_applies,
                                      small_graph_nam_forward)
    rng = np.random.default_rng(1000 * n + 10 * D + F)
    g = _hop_graph(rng, n, D, rest)
    Dg = g.n_codes
    x = torch.from_numpy(rng.standard_normal((n, F)).astype(np.float32)).to(DEV)
    m = _model(F, C, Ln, bias=bias, normalize=use_cnt)
    up = torch.from_numpy(rng.standard_normal((C, 1)).astype(np.float32)).to(DEV)
    f, rho, nam = _stacks(m)
    assert small_graph_nam_applies(x, g, f, rho, nam) and nam.L == Ln and nam.C == C and (f.b_first is not None) == bias
    want, (_, want_fx, want_lut, want_hidden, *_), want_g = _run(m, lambda: small_graph_nam_forward(x, g, *_stacks(m), use_cnt), up)
    slot = SlotGraph(F, DEV, use_cnt=use_cnt, max_nodes=cap, n_codes=tier)
    assert slot.fits(g, x) and slot_nam_applies(slot, f, rho, nam) and slot_tier(g)[1] <= tier
    slot.load(g, x)
    got, (fx, lut, hidden, *_), got_g = _run(m, lambda: slot_graph_nam_forward(slot, *_stacks(m), use_cnt), up)
    assert got.shape == want.shape == (C, 1) and fx.shape == (F, cap) and lut.shape == (tier,)
    assert torch.equal(got, want) and torch.equal(hidden, want_hidden) and torch.equal(fx[:, :n], want_fx)
    assert torch.equal(lut[: Dg - 1], want_lut[: Dg - 1]) and torch.equal(lut[tier - 1], want_lut[Dg - 1])
    assert sorted(got_g) == sorted(want_g) and len(got_g) >= 5
    for k in want_g:
        assert torch.equal(got_g[k], want_g[k]), k
    again, _, again_g = _run(m, lambda: slot_graph_nam_forward(slot, *_stacks(m), use_cnt), up)
    assert torch.equal(again, got) and all(torch.equal(again_g[k], got_g[k]) for k in got_g)
    ws = [w for w in small_graph._SMALL_WS.values() if w.device == x.device]
    assert ws and all(int(w[:4].abs().sum()) == 0 for w in ws)                 # the counter line is left zero


@functools.lru_cache(maxsize=None)
def _truth_graphs():
    _need_gpu()
    return _graph_task(2, 15, sizes=[30, 128], seed=7)


@pytest.mark.parametrize("Ln,C,normalize", [(1, 1, True), (2, 3, True), (3, 8, False)])
@pytest.mark.parametrize("which", [0, 1], ids=["n30", "n128"])
def test_slots_against_the_float64_chain(which, Ln, C, normalize):
    from gnan_amd.small_graph import SlotGraph, slot_graph_nam_forward, slot_tier
    from oracle import gnan_oracle as O
    d = _truth_graphs()[which]
    n, F = d.x.shape
    assert n == (30, 128)[which]
    m = _model(F, C, Ln, normalize=normalize, seed=Ln)
    g = m.hop_graph(d)
    tier = slot_tier(g)
    slot = SlotGraph(F, DEV, use_cnt=normalize, max_nodes=tier[0], n_codes=tier[1])
    assert slot.fits(g, d.x)
    slot.load(g, d.x)
    up = torch.from_numpy(np.random.default_rng(5).standard_normal((C, 1)))
    got, _, got_g = _run(m, lambda: slot_graph_nam_forward(slot, *_stacks(m), normalize), up.to(DEV, torch.float32))
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}

    @functools.lru_cache(maxsize=None)
    def chain(dtype):
        p = {k: v.to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
        out = O.tensor_gnan_forward_models(d.x.cpu().to(dtype), d.node_distances.cpu().to(dtype), d.normalization_matrix.cpu().to(dtype),
                                           p, normalize, True, Ln)
        (out * up.to(dtype)).sum().backward()
        return out.detach(), {k: v.grad for k, v in p.items()}
    want, want_g = chain(torch.float64)
    assert got.shape == want.shape == (C, 1) and sorted(got_g) == sorted(want_g)
    assert_rule(got, want, lambda: chain(torch.float32)[0], "read-out")
    assert_grads_rule(got_g, want_g, lambda: chain(torch.float32)[1], "gradients")


def test_stale_slots_are_never_read():
    """A 128-node graph, then a 5-node graph in the same slots — and the other way round: the bits of fresh slots."""
    _need_gpu()
    from gnan_amd.small_graph import SlotGraph, slot_graph_nam_forward
    F, C = 15, 3
    rng = np.random.default_rng(3)
    m = _model(F, C, 2)
    up = torch.from_numpy(rng.standard_normal((C, 1)).astype(np.float32)).to(DEV)
    big, small = _hop_graph(rng, 128, 16), _hop_graph(rng, 5, 4)
    xs = {128: torch.from_numpy(rng.standard_normal((128, F)).astype(np.float32)).to(DEV),
          5: torch.from_numpy(rng.standard_normal((5, F)).astype(np.float32)).to(DEV)}

    def on(slot, g):
        slot.load(g, xs[g.n_rows])
        out, _, grads = _run(m, lambda: slot_graph_nam_forward(slot, *_stacks(m), True), up)
        return out, grads

    def fresh():
        return SlotGraph(F, DEV, use_cnt=True, max_nodes=128, n_codes=16)
    want = {g.n_rows: on(fresh(), g) for g in (big, small)}
    used = fresh()
    for g in (big, small, big, small):
        out, grads = on(used, g)
        assert torch.equal(out, want[g.n_rows][0]), g.n_rows
        assert all(torch.equal(grads[k], want[g.n_rows][1][k]) for k in grads), g.n_rows
    assert not torch.equal(want[128][0], want[5][0])


# ---- the modules -----------------------------------------------------------------------------------------------------------------
SIZES = [12, 23, 30, 41, 64, 70, 128, 130]


@functools.lru_cache(maxsize=None)
def _graphs():
    _need_gpu()
    return _graph_task(14, 15, sizes=SIZES, seed=24)


def _epochs(m, opt, graphs, n):
    from gnan_amd import harness
    loss_fn = torch.nn.BCEWithLogitsLoss()
    return [harness.train_epoch(m, graphs, loss_fn, opt, DEV, classify=True, is_graph_task=True)[:2] for _ in range(n)]


def test_harness_epochs_run_from_slot_steps(monkeypatch):
    """Four epochs of harness.train_epoch over 14 graphs of 12 to 130 nodes: every graph of <= 128 nodes replays from a slot step
    (at most six, no per-shape capture), the 130-node graph keeps its route; losses and parameters track an eager twin; one
    evaluation pass replays from slots as well."""
    from gnan_amd import harness, small_graph
    graphs = _graphs()
    loss_fn = torch.nn.BCEWithLogitsLoss()
    runs = {}
    for on in (False, True):
        monkeypatch.setattr(harness, "GRAPHED_STEPS", on)
        m = _model(15, 1, 1, scale=0.3)
        assert small_graph.slot_mode(m) == small_graph.SlotNamMode(True)
        opt = torch.optim.Adam(m.parameters(), lr=1e-3)
        hist = _epochs(m, opt, graphs, 4)
        evals = [harness.test_epoch(m, graphs, loss_fn, DEV, classify=True, val_mask=True, is_graph_task=True)[:2] for _ in range(2)]
        runs[on] = (hist, {k: v.detach().clone() for k, v in m.state_dict().items()}, m, evals)
    for a, b in zip(runs[False][0] + runs[False][3], runs[True][0] + runs[True][3]):
        print("eager", a, "slots", b)
        assert abs(a[0] - b[0]) <= 1e-5 * max(1.0, abs(a[0])) and a[1] == b[1], (a, b)
    scale = max(float(v.abs().max()) for v in runs[False][1].values())
    for k, v in runs[False][1].items():
        assert float((v - runs[True][1][k]).abs().max()) <= 1e-5 * scale, k
    store = harness._steps_of(runs[True][2])
    steps = store.graph
    n_fit = sum(d.x.shape[0] <= 128 for d in graphs)
    assert 2 <= len(steps.slots) <= 6 and {t[0] for t in steps.slots} == {64, 128}
    replays = sum(s.step.graph.replays for s in steps.slots.values())
    print("slot steps", len(steps.slots), "replays", replays, "kernel nodes", [s.step.graph.kernel_nodes for s in steps.slots.values()])
    assert replays >= 4 * n_fit - 3, (replays, n_fit)                  # from the third step of the first epoch on
    assert all(s.step.graph.kernel_nodes <= 7 for s in steps.slots.values())
    assert all(key[0] > 128 for key, rec in steps.buckets.items() if rec["step"] is not None)
    assert any(key[0] == 130 for key in steps.buckets)                 # the 130-node graph: its own per-shape route, as before
    ev = store.graph_eval                                              # the evaluation passes: slots as well
    assert 2 <= len(ev.slots) <= 6 and sum(s.step.graph.replays for s in ev.slots.values()) >= 2 * n_fit - 3
    assert all(key[0] > 128 for key, rec in ev.buckets.items() if rec["step"] is not None)
    harness.release_steps(runs[True][2])


def test_a_plain_no_grad_loop_replays_from_slot_plans():
    """The modules' own replay: four passes of m.forward(d) over graphs of different sizes leave a slot plan and return the eager
    outputs."""
    from gnan_amd import replay
    graphs = [d for d in _graphs() if d.x.shape[0] <= 128][:6]
    assert len({d.x.shape[0] for d in graphs}) >= 4
    m = _model(15, 3, 2, scale=0.3)
    with torch.no_grad():
        got = [m.forward(d).detach().clone() for _ in range(4) for d in graphs]
        old = replay.REPLAY_FORWARD
        replay.REPLAY_FORWARD = False
        try:
            want = [m.forward(d).detach().clone() for _ in range(4) for d in graphs]
        finally:
            replay.REPLAY_FORWARD = old
    for s, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape == (3, 1)
        assert float((a - b).abs().max()) <= TWO_FLOORS * float(b.abs().max()), s
    plans = [rec["plan"] for rec in m.__dict__["_replay_slots"].plans.values() if rec["plan"] is not None]
    assert plans and sum(p.fwd.replays for p in plans) >= len(got) - 3
    replay.release(m)


def test_the_switch_off_is_the_route_as_before(monkeypatch):
    from gnan_amd import harness, small_graph
    monkeypatch.setattr(small_graph, "SLOT_NAM_READOUT", False)
    graphs = _graphs()[:4]
    m = _model(15, 1, 1, scale=0.3)
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


@pytest.mark.parametrize("capture_dropout", [False, True])
def test_dropout_takes_no_slot_step(capture_dropout, monkeypatch):
    """train() with dropout = 0.5: the read-out kernels draw no masks, so nothing is captured over slots — eager steps, finite
    gradients — whether or not other routes' forwards under Dropout may be captured (``CAPTURE_DROPOUT``)."""
    from gnan_amd import harness, small_graph
    monkeypatch.setattr(small_graph, "CAPTURE_DROPOUT", capture_dropout)
    graphs = _graphs()[:6]
    m = _model(15, 1, 1, dropout=0.5, scale=0.3)
    assert isinstance(small_graph.slot_mode(m), small_graph.SlotNamMode) and m._dropout_active()
    assert not small_graph.dropout_capture_applies(m, graphs[0].x, m.hop_graph(graphs[0]))
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                # (the one-time note of _check_dropout)
        hist = _epochs(m, opt, graphs, 2)
    steps = harness._steps_of(m).graph                                 # (None: the harness did not even ask for captured steps)
    assert steps is None or (not steps.slots and steps.captured == 0)
    assert all(np.isfinite(h[0]) for h in hist)
    assert all(bool(torch.isfinite(p).all()) for p in m.parameters())
    d = graphs[0]
    m.zero_grad(set_to_none=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m.forward(d).sum().backward()                                  # the caller's own loop: eager as well
    assert "_replay_slots" not in m.__dict__ or not any(r["plan"] is not None for r in m.__dict__["_replay_slots"].plans.values())
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.parameters())
    slot = small_graph.SlotGraph(15, DEV, use_cnt=True, max_nodes=64, n_codes=16)
    slot.load(m.hop_graph(d), d.x)
    with pytest.raises(Exception, match="Dropout"):                    # a slot never serves such a forward
        m._forward(Bag(x=slot.x, edge_index=None, gnan_graph=slot))
    harness.release_steps(m)
