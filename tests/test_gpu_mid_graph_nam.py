"""The NAM read-out of dense-coded graphs of 129 to 448 nodes in one launch forward and two backward (csrc/mid_graph_nam.hip,
small_graph.mid_graph_nam_forward): the kernels against the float64 chain at the sizes where a tiled walk goes wrong, a tile-edge probe
on the kernel's own leftovers, the small route's kernels as a second implementation, the modules' routing, and the route inside
captured and replayed training steps."""
import copy

import numpy as np
import pytest
import torch

import reference_loop
from helpers import TWO_FLOORS, assert_grads_rule, assert_rule
from oracle import gnan_oracle as O
from test_gpu_graphed import DEV, Bag, _need_gpu

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _route_on(monkeypatch):
    """The tests do not depend on how the switch ships."""
    from gnan_amd import small_graph
    monkeypatch.setattr(small_graph, "MID_GRAPH_NAM", True)


def _graph_of(hops):
    from gnan_amd import HopGraph
    nd = torch.zeros(hops.shape)
    nd[torch.from_numpy(hops >= 0)] = 1.0 / (torch.from_numpy(hops[hops >= 0]).float() + 1.0)
    return HopGraph.from_dense(nd.to(DEV))


def _mlp(rng, Fk, Ck, Lk, Hk, b):
    t = lambda *s: torch.from_numpy((rng.standard_normal(s) * 0.5).astype(np.float32))      # noqa: E731
    if Lk == 1:
        return [None, None, None, None, t(Fk, Ck), t(Fk, Ck) if b else None]
    return [t(Fk, Hk), t(Fk, Hk) if b else None, t(1, Fk, Hk, Hk) if Lk == 3 else None, t(1, Fk, Hk) if (Lk == 3 and b) else None,
            t(Fk, Ck, Hk), t(Fk, Ck) if b else None]


def _net(v, p, k, Lk):                                             # v [m] -> [m, C]
    if Lk == 1:
        return v[:, None] * p[4][k][None, :] + (0 if p[5] is None else p[5][k])
    h = torch.relu(v[:, None] * p[0][k] + (0 if p[1] is None else p[1][k]))
    if Lk == 3:
        h = torch.relu(h @ p[2][0, k].T + (0 if p[3] is None else p[3][0, k]))
    return h @ p[4][k].T + (0 if p[5] is None else p[5][k])


class _Case:
    """One graph, the three stacks, one upstream gradient: a fused route on the device, the chain written out on the CPU."""

    def __init__(self, hops, x, fp, rp, npar, L, H, Ln, Hn, Cn, use_cnt):
        self.hops, self.x, self.fp, self.rp, self.npar = hops, x, fp, rp, npar
        self.L, self.H, self.Ln, self.Hn, self.Cn, self.use_cnt = L, H, Ln, Hn, Cn, use_cnt
        self.n, self.F = x.shape
        self.g = _graph_of(hops)
        self.D = self.g.n_codes

    def run(self, dtype, dev, route):
        """``route``: "mid" / "small" (the device kernels) or None (the chain) -> (out, gradients, (fx [F, n], lut, hidden, colw))"""
        from gnan_amd.functional import StackedMLP
        from gnan_amd import small_graph as sg
        L, H, Ln, Hn, Cn, F, n, D = self.L, self.H, self.Ln, self.Hn, self.Cn, self.F, self.n, self.D
        fl, rl, nl = ([None if t is None else t.to(dev, dtype).requires_grad_(True) for t in q] for q in (self.fp, self.rp, self.npar))
        xs = self.x.to(dev, dtype)
        if route is not None:
            f, r, nm = StackedMLP(*fl, L, H, 1, F), StackedMLP(*rl, L, H, 1, 1), StackedMLP(*nl, Ln, Hn if Ln > 1 else 0, Cn, F)
            if route == "mid":
                assert sg.mid_graph_nam_applies(xs, self.g, f, r, nm, self.use_cnt) == (n >= 129)
                out = sg.mid_graph_nam_forward(xs, self.g, f, r, nm, self.use_cnt)      # (no predicate inside: straight to the library)
                left = tuple(t.detach().clone() for t in out.grad_fn.saved_tensors[1:5])
            else:
                assert sg.small_graph_nam_applies(xs, self.g, f, r, nm)
                out = sg.small_graph_nam_forward(xs, self.g, f, r, nm, self.use_cnt)
                left = None
        else:
            fx = torch.cat([_net(xs[:, k], fl, k, L) for k in range(F)], 1)            # [n, F]
            u = torch.zeros(D, dtype=dtype)
            u[: D - 1] = (1.0 / (torch.arange(D - 1, dtype=torch.float32) + 1.0)).to(dtype)
            lut = _net(u, rl, 0, L)[:, 0]
            codes = torch.from_numpy(np.where(self.hops >= 0, self.hops, D - 1)).long()
            w = lut[codes]
            if self.use_cnt:
                cnt = self.g.cnt.cpu().clamp_min(1).to(dtype)
                w = w / cnt[torch.arange(n)[:, None], codes]
            hidden = (w @ fx).sum(0)                                                  # [F]   models.py:373-379
            out = sum(_net(hidden[k:k + 1], nl, k, Ln) for k in range(F)).T            # [C, 1]
            left = (fx.detach().T, lut.detach(), hidden.detach(), w.detach().sum(0))
        up = torch.from_numpy(np.random.default_rng(5).standard_normal(tuple(out.shape))).to(dev, dtype)
        live = [t for t in fl + rl + nl if t is not None]
        return out.detach(), torch.autograd.grad(out, live, up), left


def _random_case(n, F, L, H, Ln, Hn, Cn, D_hops, use_cnt, bias):
    """The inputs of test_gpu_kernels.test_small_graph_nam_readout_in_one_launch: its seed, its draws in its order, a rho without bias
    whose last layer is non-negative (the instance stays well conditioned: see the note there)."""
    rng = np.random.default_rng(n * 13 + F + 4)
    hops = rng.integers(-1, D_hops, (n, n)).astype(np.int32)
    hops[np.arange(n), np.arange(n)] = 0
    fp, rp, npar = _mlp(rng, F, 1, L, H, bias), _mlp(rng, 1, 1, L, H, False), _mlp(rng, F, Cn, Ln, Hn, bias)
    rp[4] = rp[4].abs()
    x = torch.from_numpy(rng.standard_normal((n, F)).astype(np.float32))
    return _Case(hops, x, fp, rp, npar, L, H, Ln, Hn, Cn, use_cnt)


def _counter_lines_are_zero(device):
    from gnan_amd import small_graph
    ws = [w for w in small_graph._SMALL_WS.values() if w.device == device]
    assert ws and all(int(w[:4].abs().sum()) == 0 for w in ws)                 # the counter line is left zero


LEFT = ("fx", "lut", "hidden", "colw")


@pytest.mark.parametrize("n,F,L,H,Ln,Hn,Cn,D_hops,use_cnt,bias", [
    (129, 15, 3, 64, 1, 0, 1, 9, True, True),        # one row into the third tile; n * n odd: the 4-byte code loads have a tail
    (192, 7, 3, 64, 2, 64, 3, 20, True, True),       # exactly a tile edge
    (193, 7, 2, 32, 3, 48, 3, 20, True, False),      # one row past it; two-layer f and rho
    (200, 70, 2, 16, 1, 0, 4, 30, False, False),     # more than 64 features: T's chunk loop
    (256, 4, 3, 30, 2, 30, 8, 63, False, True),      # 64 shells, H no multiple of 4, 8 classes
    (300, 130, 3, 16, 2, 16, 2, 2, True, True),      # F > 127: no residency limit
    (417, 15, 3, 64, 2, 64, 1, 12, True, True),      # the data set's largest graph
    (448, 3, 3, 48, 3, 64, 8, 5, True, True)])       # the cap
def test_mid_graph_nam_readout_one_launch_forward_two_backward(n, F, L, H, Ln, Hn, Cn, D_hops, use_cnt, bias):
    """gnan_mid_graph_nam_fwd / _bwd == the float64 chain (the floor of 1e-5, the float32 chain's own error beyond it):
    the output, every parameter gradient of f, rho and the read-out, and the leftovers fx, lut, hidden, colw; a second run gives the
    same bits; the workspace's counter line is zero afterwards.  (The float32 chain on the CPU for exactly these seeds: forward
    <= 3.8e-7, gradients <= 6.3e-6 of the largest entry — the floor decides.)"""
    _need_gpu()
    case = _random_case(n, F, L, H, Ln, Hn, Cn, D_hops, use_cnt, bias)
    assert case.D == D_hops + 1 <= 64
    got, got_g, got_left = case.run(torch.float32, DEV, "mid")
    want, want_g, want_left = case.run(torch.float64, "cpu", None)
    ref32 = {}

    def ref(i):                                                       # the float32 chain: evaluated once, and only if needed
        if not ref32:
            ref32["v"] = case.run(torch.float32, "cpu", None)
        return ref32["v"][i]
    assert got.shape == (Cn, 1)
    err = lambda a, b: float((a.detach().cpu().double().reshape(b.shape) - b).abs().max()) / max(float(b.abs().max()), 1e-300)   # noqa: E731
    scale_g = max(float(w.abs().max()) for w in want_g)
    print("forward %.3e  gradients %.3e  leftovers %s" % (
        err(got, want), max(float((a.cpu().double() - b).abs().max()) for a, b in zip(got_g, want_g)) / scale_g,
        " ".join("%s %.3e" % (nm, err(a, b)) for nm, a, b in zip(LEFT, got_left, want_left))))
    assert_rule(got, want, lambda: ref(0), "forward")
    assert_grads_rule(list(got_g), list(want_g), lambda: list(ref(1)), "gradients")
    for i, name in enumerate(LEFT):
        assert got_left[i].shape == want_left[i].shape, name
        assert_rule(got_left[i], want_left[i], lambda i=i: ref(2)[i], name)
    again, again_g, again_left = case.run(torch.float32, DEV, "mid")
    assert torch.equal(got, again) and all(torch.equal(a, b) for a, b in zip(got_g, again_g))
    assert all(torch.equal(a, b) for a, b in zip(got_left, again_left))
    _counter_lines_are_zero(got.device)


def test_one_pair_across_a_tile_edge():
    """193 nodes, every pair unreachable but the diagonal (hop 0) and the single pair (192, 0) at hop 1: D = 3, rho has no bias so
    lut[2] = rho(0) is exactly 0, and every shell size on the path is 1.  The kernel's own leftovers, bit for bit: colw[j] = lut[0]
    for j != 0 and colw[0] = lut[0] + lut[1] as a float32 sum — every other addend is an exact zero, and row 192 is the fourth
    tile's only row."""
    _need_gpu()
    n, F, H = 193, 5, 16
    rng = np.random.default_rng(193)
    hops = np.full((n, n), -1, dtype=np.int32)
    hops[np.arange(n), np.arange(n)] = 0
    hops[192, 0] = 1
    fp, rp, npar = _mlp(rng, F, 1, 3, H, True), _mlp(rng, 1, 1, 3, H, False), _mlp(rng, F, 2, 2, H, True)
    x = torch.from_numpy(rng.standard_normal((n, F)).astype(np.float32))
    case = _Case(hops, x, fp, rp, npar, 3, H, 2, H, 2, True)
    assert case.D == 3
    got, got_g, (fx, lut, hidden, colw) = case.run(torch.float32, DEV, "mid")
    want, want_g, _ = case.run(torch.float64, "cpu", None)
    ref32 = lambda: case.run(torch.float32, "cpu", None)             # noqa: E731
    fx, lut, hidden, colw = fx.cpu(), lut.cpu(), hidden.cpu(), colw.cpu()
    assert float(lut[2]) == 0.0
    assert torch.equal(colw[1:], lut[0].expand(n - 1))
    assert torch.equal(colw[0], lut[0] + lut[1])                      # (a float32 sum)
    expect = lut[0].double() * fx.double().sum(1) + lut[1].double() * fx[:, 0].double()
    assert float((hidden.double() - expect).abs().max()) <= 1e-6 * float(hidden.abs().max())
    assert_rule(got, want, lambda: ref32()[0], "forward")
    assert_grads_rule(list(got_g), list(want_g), lambda: list(ref32()[1]), "gradients")


@pytest.mark.parametrize("n", [64, 128])
def test_two_independent_implementations(n):
    """Below the predicate's lower bound the library's entry points take the graphs the small route's kernels take: the tiled kernels
    and small_graph_nam_forward's agree on the output and on every gradient within two floors of the largest float64 entry."""
    _need_gpu()
    case = _random_case(n, 15, 3, 64, 2, 64, 3, 11, True, True)
    mid, mid_g, _ = case.run(torch.float32, DEV, "mid")
    small, small_g, _ = case.run(torch.float32, DEV, "small")
    want, want_g, _ = case.run(torch.float64, "cpu", None)
    assert float((mid - small).abs().max()) <= TWO_FLOORS * float(want.abs().max())
    scale = max(float(w.abs().max()) for w in want_g)
    for a, b in zip(mid_g, small_g):
        assert float((a - b).abs().max()) <= TWO_FLOORS * scale


def _graphs(sizes, F, seed=3):
    """Random trees with a few extra edges (connected, diameters far below 63 hops), one-hot features: test_gpu_mid_graph._graphs."""
    rng = np.random.default_rng(seed)
    data = []
    for n in sizes:
        tree = np.stack([np.arange(1, n), rng.integers(0, np.arange(1, n))])
        extra = np.stack([rng.integers(0, n, n // 4 + 1), rng.integers(0, n, n // 4 + 1)])
        ei = np.concatenate([tree, extra], axis=1)
        nd, norm = O.pre_process_dense(np.concatenate([ei, ei[::-1]], axis=1), n)
        x = torch.zeros(n, F)
        x[torch.arange(n), torch.from_numpy(rng.integers(0, F - 1, n))] = 1.0
        x[:, -1] = 1.0
        y = torch.tensor([[1.0 if rng.random() < 0.5 else -1.0]])
        data.append(Bag(x=x.to(DEV), y=y.to(DEV), edge_index=None, node_distances=nd.to(DEV), normalization_matrix=norm.to(DEV)))
    return data


def _readout_model(Ln, C=1, normalize=True, hidden=32, scale=0.4, dropout=0.0):
    from gnan_amd.models import TensorGNAN
    m = TensorGNAN(15, C, 3, hidden_channels=hidden, is_graph_task=True, readout_n_layers=Ln, normalize_rho=normalize, dropout=dropout,
                   device=DEV)
    torch.manual_seed(Ln)
    with torch.no_grad():
        for _, p in m.named_parameters():
            p.copy_(torch.randn(p.shape) * scale)
    return m.to(DEV).eval()


@pytest.fixture(scope="module")
def graphs():
    _need_gpu()
    return _graphs([130, 200, 417], 15)


def _spy(monkeypatch):
    from gnan_amd import _lib
    calls = []
    real = _lib.lib().gnan_mid_graph_nam_fwd

    def counted(a, stream):
        calls.append(a.n)
        return real(a, stream)
    monkeypatch.setattr(_lib.lib(), "gnan_mid_graph_nam_fwd", counted)
    return calls


@pytest.mark.parametrize("Ln,C,normalize", [(1, 1, True), (2, 3, True), (3, 8, False)])
@pytest.mark.parametrize("which", [0, 1, 2])
def test_the_modules_take_the_route(which, Ln, C, normalize, graphs, monkeypatch):
    """models.TensorGNAN with a NAM read-out on dense graphs of 130, 200 and 417 nodes: the entry point is called, the stages are the
    one-launch routes'; forward and every parameter gradient == the float64 oracle; with MID_GRAPH_NAM off (the general route) the
    entry point is not called and the results agree within two floors."""
    from gnan_amd import replay, small_graph
    monkeypatch.setattr(replay, "REPLAY_FORWARD", False)
    data = graphs[which]
    m = _readout_model(Ln, C, normalize)
    calls = _spy(monkeypatch)
    stages = []
    m.stage_hook = stages.append

    def run():
        m.zero_grad(set_to_none=True)
        out = m.forward(data)
        out.sum().backward()
        return out.detach().clone(), {k: p.grad.detach().clone() for k, p in m.named_parameters()}
    got, got_g = run()
    assert calls == [data.x.shape[0]] and stages == ["start", "fmlp", "spmm"]
    monkeypatch.setattr(small_graph, "MID_GRAPH_NAM", False)
    general, general_g = run()
    assert len(calls) == 1                                            # (not taken with the switch off)
    monkeypatch.setattr(small_graph, "MID_GRAPH_NAM", True)

    def oracle(dtype):
        p = {k: v.detach().cpu().to(dtype).clone().requires_grad_(True) for k, v in m.state_dict().items()}
        out = O.tensor_gnan_forward_models(data.x.cpu().to(dtype), data.node_distances.cpu().to(dtype),
                                           data.normalization_matrix.cpu().to(dtype), p, normalize, True, Ln)
        out.sum().backward()
        return out.detach(), {k: v.grad for k, v in p.items()}
    want, want_g = oracle(torch.float64)
    assert got.shape == want.shape == (C, 1)
    assert_rule(got, want, lambda: oracle(torch.float32)[0], "forward")
    assert_grads_rule(got_g, want_g, lambda: oracle(torch.float32)[1], "gradients")
    assert float((got - general).abs().max()) <= TWO_FLOORS * float(want.abs().max())
    scale = max(float(v.abs().max()) for v in want_g.values())
    for k in got_g:
        assert float((got_g[k] - general_g[k]).abs().max()) <= TWO_FLOORS * scale, k


def test_dropout_and_input_gradients_keep_the_general_route(graphs, monkeypatch):
    """Training-mode Dropout (of f and of the read-out NAM) and a wanted gradient of x are outside this route."""
    import warnings
    from gnan_amd import replay
    monkeypatch.setattr(replay, "REPLAY_FORWARD", False)
    calls = _spy(monkeypatch)
    data = graphs[0]
    m = _readout_model(2, 1, True, dropout=0.3).train()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m.forward(data).sum().backward()
    assert calls == []
    m = _readout_model(2, 1, True)
    x = data.x.clone().requires_grad_(True)
    out = m.forward(Bag(x=x, y=data.y, edge_index=None, node_distances=data.node_distances,
                        normalization_matrix=data.normalization_matrix))
    assert calls == [] and out.shape == (1, 1)
    m.forward(data).sum().backward()                                  # (the spy does see the route where it applies)
    assert calls == [130]


def test_the_route_inside_a_replayed_training_step(graphs, monkeypatch):
    """Six training steps on ONE 200-node graph object: the replay plan (forward + backward, gnan_amd.replay) is captured with
    the three launches in it and replayed; parameters == a twin with the replay switched off."""
    from gnan_amd import replay
    data = graphs[1]
    loss_fn = torch.nn.BCEWithLogitsLoss()
    calls = _spy(monkeypatch)
    a = _readout_model(1, scale=0.3)
    b = copy.deepcopy(a)
    oa, ob = torch.optim.Adam(a.parameters(), lr=1e-3), torch.optim.Adam(b.parameters(), lr=1e-3)
    for e in range(6):
        monkeypatch.setattr(replay, "REPLAY_FORWARD", False)
        ta = reference_loop.train_epoch(a, [data], loss_fn, oa, DEV, classify=True, is_graph_task=True)
        monkeypatch.setattr(replay, "REPLAY_FORWARD", True)
        tb = reference_loop.train_epoch(b, [data], loss_fn, ob, DEV, classify=True, is_graph_task=True)
        assert abs(ta[0] - tb[0]) <= 1e-5 * max(1.0, abs(ta[0])) and ta[1] == tb[1], (e, ta, tb)
        scale = max(float(v.abs().max()) for v in a.state_dict().values())
        for (k, va), (_, vb) in zip(a.state_dict().items(), b.state_dict().items()):
            assert float((va - vb).abs().max()) <= 1e-5 * scale, (e, k)
    assert calls and set(calls) == {200}                              # (the route was taken, eagerly and under capture)
    cache = b.__dict__.get("_replays")
    plans = [] if cache is None else [r.value["plan"] for r in cache.entries.values() if r.value["plan"] is not None]
    train = [p for p in plans if p.grad]
    assert train and all(p.fwd.replays >= 1 and p.bwd.replays == p.fwd.replays for p in train)
    replay.release(b)


def test_graph_task_steps_replayed_per_shape_match_eager_steps(monkeypatch):
    """harness.train_epoch over graphs of 130, 130, 150, 130, 150 nodes, two epochs: one captured step per graph shape, two copies of
    the model in lock-step — one eagerly, one through the replayer — compared and reset after EVERY step
    (test_gpu_graphed.test_graph_task_steps_replayed_per_shape_match_eager_steps's comparison); at least one step was replayed."""
    _need_gpu()
    from gnan_amd import harness
    from gnan_amd.models import TensorGNAN
    monkeypatch.setattr(harness, "SLOT_STEPS", False)
    F = 15
    loader = _graphs([130, 130, 150, 130, 150], F, seed=0)
    loss_fn = torch.nn.BCEWithLogitsLoss()
    calls = _spy(monkeypatch)

    def make():
        torch.manual_seed(0)
        m = TensorGNAN(F, 1, 3, hidden_channels=32, is_graph_task=True, readout_n_layers=2, device=DEV)
        with torch.no_grad():
            for _, p in m.named_parameters():
                p.copy_(torch.randn(p.shape) * 0.5)
        m = m.to(DEV).eval()
        return m, torch.optim.Adam(m.parameters(), lr=2e-3, capturable=True, fused=True)
    (ma, oa), (mb_, ob) = make(), make()
    worst = 0
    for epoch in range(2):
        for g in loader:
            monkeypatch.setattr(harness, "GRAPHED_STEPS", False)
            ra = harness.train_epoch(ma, [g], loss_fn, oa, DEV, classify=True, is_graph_task=True)
            monkeypatch.setattr(harness, "GRAPHED_STEPS", True)
            rb = harness.train_epoch(mb_, [g], loss_fn, ob, DEV, classify=True, is_graph_task=True)
            assert abs(ra[0] - rb[0]) <= 1e-5 * max(1.0, abs(ra[0])) and ra[1] == rb[1], (epoch, ra, rb)
            with torch.no_grad():
                for pa, pb in zip(ma.parameters(), mb_.parameters()):
                    scale = float(pa.abs().max()) + 1e-12
                    worst = max(worst, float((pa - pb).abs().max()) / scale)
                    pb.copy_(pa)
                    for key in ("exp_avg", "exp_avg_sq", "step"):
                        ob.state[pb][key].copy_(oa.state[pa][key])
            assert worst <= 1e-5, (epoch, worst)
    assert calls and set(calls) <= {130, 150}
    steps = harness._steps_of(mb_).graph
    replayed = sum(r["step"].step.graph.replays for r in steps.buckets.values() if r["step"] is not None)
    assert replayed >= 1, replayed
