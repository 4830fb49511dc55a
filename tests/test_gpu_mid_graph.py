"""The one-launch forward and backward of dense-coded graphs of 129 to 448 nodes (csrc/mid_graph.hip, small_graph.mid_graph_forward):
the kernels against the float64 chain at the sizes where a tiled walk goes wrong, a tile-edge probe, the modules' routing, and
the route inside a captured and replayed training step."""
import copy

import numpy as np
import pytest
import torch

import reference_loop
from helpers import TWO_FLOORS, assert_grads_rule, assert_rule
from oracle import gnan_oracle as O
from test_gpu_graphed import DEV, Bag, _need_gpu

pytestmark = pytest.mark.gpu


def _graph_of(hops):
    from gnan_amd import HopGraph
    nd = torch.zeros(hops.shape)
    nd[torch.from_numpy(hops >= 0)] = 1.0 / (torch.from_numpy(hops[hops >= 0]).float() + 1.0)
    return HopGraph.from_dense(nd.to(DEV))


def _mlps(rng, F, C, L, H, bias_f, bias_r):
    def mlp(Fk, Ck, bias):
        t = lambda *s: torch.from_numpy((rng.standard_normal(s) * 0.5).astype(np.float32))      # noqa: E731
        return [t(Fk, H), t(Fk, H) if bias else None, t(1, Fk, H, H) if L == 3 else None, t(1, Fk, H) if (L == 3 and bias) else None,
                t(Fk, Ck, H), t(Fk, Ck) if bias else None]
    return mlp(F, C, bias_f), mlp(1, 1, bias_r)


class _Case:
    """One graph, one pair of MLPs, one upstream gradient: the fused route on the device, the chain written out on the CPU."""

    def __init__(self, hops, x, fp, rp, L, H, C, use_cnt, graph_sum, up=None):
        self.hops, self.x, self.fp, self.rp, self.L, self.H, self.C = hops, x, fp, rp, L, H, C
        self.use_cnt, self.graph_sum, self.up = use_cnt, graph_sum, up
        self.n, self.F = x.shape
        self.g = _graph_of(hops)
        self.D = self.g.n_codes

    def run(self, dtype, dev, fused):
        """-> (output, gradients of every parameter, (S, lut))"""
        from gnan_amd.functional import StackedMLP
        from gnan_amd.small_graph import mid_graph_applies, mid_graph_forward
        L, H, C, F, n, D = self.L, self.H, self.C, self.F, self.n, self.D
        fl = [None if t is None else t.to(dev, dtype).requires_grad_(True) for t in self.fp]
        rl = [None if t is None else t.to(dev, dtype).requires_grad_(True) for t in self.rp]
        xs = self.x.to(dev, dtype)
        if fused:
            f, r = StackedMLP(*fl, L, H, C, F), StackedMLP(*rl, L, H, 1, 1)
            assert mid_graph_applies(xs, self.g, f, r, self.use_cnt)
            out = mid_graph_forward(xs, self.g, f, r, self.use_cnt, self.graph_sum)
            saved = out.grad_fn.saved_tensors
            left = (saved[1].detach().clone(), saved[2].detach().clone())
        else:                                                         # the chain, written out
            def net(v, p, k):                                         # v [m] -> [m, C]
                h = torch.relu(v[:, None] * p[0][k] + (0 if p[1] is None else p[1][k]))
                if L == 3:
                    h = torch.relu(h @ p[2][0, k].T + (0 if p[3] is None else p[3][0, k]))
                return h @ p[4][k].T + (0 if p[5] is None else p[5][k])
            S = sum(net(xs[:, k], fl, k) for k in range(F))
            u = torch.zeros(D, dtype=dtype)
            u[: D - 1] = (1.0 / (torch.arange(D - 1, dtype=torch.float32) + 1.0)).to(dtype)
            lut = net(u, rl, 0)                                       # [D, 1]
            codes = torch.from_numpy(np.where(self.hops >= 0, self.hops, D - 1)).long()
            w = lut[codes]                                            # [n, n, 1]
            if self.use_cnt:
                cnt = self.g.cnt.cpu().clamp_min(1).to(dtype)
                w = w / cnt[torch.arange(n)[:, None], codes][..., None]
            out = (w * S[None, :, :]).sum(1)
            out = out.sum(0).view(-1, 1) if self.graph_sum else out
            left = (S.detach(), lut.detach())
        up = self.up if self.up is not None else torch.from_numpy(np.random.default_rng(5).standard_normal(tuple(out.shape)))
        live = [t for t in fl + rl if t is not None]
        return out.detach(), torch.autograd.grad(out, live, up.to(dev, dtype)), left


def _random_case(n, F, C, L, H, D_hops, use_cnt, graph_sum, bias_f=True, bias_r=False):
    rng = np.random.default_rng(n * 7 + F)
    hops = rng.integers(-1, D_hops, (n, n)).astype(np.int32)           # -1 = unreachable
    hops[np.arange(n), np.arange(n)] = 0
    fp, rp = _mlps(rng, F, C, L, H, bias_f, bias_r)
    x = torch.from_numpy(rng.standard_normal((n, F)).astype(np.float32))
    return _Case(hops, x, fp, rp, L, H, C, use_cnt, graph_sum)


@pytest.mark.parametrize("n,F,C,L,H,D_hops,use_cnt,graph_sum,bias_f,bias_r", [
    (129, 15, 1, 3, 64, 9, True, True, True, False),       # one row into the third tile; n * n odd: the 4-byte code loads have a tail
    (192, 7, 2, 3, 64, 20, True, False, True, False),      # exactly a tile edge
    (193, 7, 2, 3, 64, 20, True, False, True, False),      # one row past it
    (200, 15, 1, 3, 64, 30, True, True, True, False),
    (256, 4, 8, 2, 30, 63, False, True, True, False),      # 8 channels, two-layer MLPs, H no multiple of 4, 64 shells
    (417, 15, 1, 3, 64, 12, True, True, True, False),      # the dataset's largest graph
    (448, 3, 3, 3, 48, 5, True, False, True, False),       # the cap
    (300, 64, 1, 3, 64, 2, False, True, True, False),      # many features, two shells
    (200, 7, 2, 3, 32, 10, True, False, False, True)])     # no bias on f, biases on rho
def test_mid_graph_forward_and_backward_in_one_launch_each(n, F, C, L, H, D_hops, use_cnt, graph_sum, bias_f, bias_r):
    """gnan_mid_graph_fwd / _bwd == the float64 chain (the float32 chain's own error is the bound beyond the floor),
    forward, every parameter gradient, and the node sums and rho table the forward leaves behind; two runs give the same bits;
    the general kernels on the saved S and lut give the same gradients within two floors."""
    _need_gpu()
    from gnan_amd import small_graph
    case = _random_case(n, F, C, L, H, D_hops, use_cnt, graph_sum, bias_f, bias_r)
    assert case.D == D_hops + 1 <= 64
    got, got_g, got_left = case.run(torch.float32, DEV, True)
    want, want_g, want_left = case.run(torch.float64, "cpu", False)
    ref32 = {}

    def ref(i):                                                       # the float32 chain: evaluated once, and only if needed
        if not ref32:
            ref32["v"] = case.run(torch.float32, "cpu", False)
        return ref32["v"][i]
    assert got.shape == ((C, 1) if graph_sum else (n, C))
    assert_rule(got, want, lambda: ref(0), "forward")
    assert_grads_rule(list(got_g), list(want_g), lambda: list(ref(1)), "gradients")
    assert_rule(got_left[0], want_left[0], lambda: ref(2)[0], "S")
    assert_rule(got_left[1], want_left[1], lambda: ref(2)[1], "lut")
    again, again_g, again_left = case.run(torch.float32, DEV, True)
    assert torch.equal(got, again) and all(torch.equal(a, b) for a, b in zip(got_g, again_g))
    assert torch.equal(got_left[0], again_left[0]) and torch.equal(got_left[1], again_left[1])
    old = small_graph.SMALL_GRAPH_BACKWARD
    small_graph.SMALL_GRAPH_BACKWARD = False                          # the general kernels on the saved S and lut
    try:
        _, general_g, _ = case.run(torch.float32, DEV, True)
    finally:
        small_graph.SMALL_GRAPH_BACKWARD = old
    scale = max(float(w.abs().max()) for w in want_g)
    for a, b in zip(got_g, general_g):
        assert float((a - b).abs().max()) <= TWO_FLOORS * scale


def test_one_pair_across_a_tile_edge():
    """193 nodes, every pair unreachable but the diagonal and the single pair (192, 0) at hop 1: rho has no bias, so the rest
    shell weighs rho(0) = 0 and the pair's weight is all that links two rows — Y[192] = lut[0] S[192] + lut[1] S[0] from the
    fourth tile's only row, and in the backward dS[0] and dS[192] alone receive it (upstream gradient on row 192 only)."""
    _need_gpu()
    n, F, C, L, H = 193, 5, 2, 3, 16
    rng = np.random.default_rng(193)
    hops = np.full((n, n), -1, dtype=np.int32)
    hops[np.arange(n), np.arange(n)] = 0
    hops[192, 0] = 1
    fp, rp = _mlps(rng, F, C, L, H, True, False)
    x = torch.from_numpy(rng.standard_normal((n, F)).astype(np.float32))
    up = torch.zeros(n, C, dtype=torch.float64)
    up[192] = torch.tensor([1.0, -2.0], dtype=torch.float64)
    case = _Case(hops, x, fp, rp, L, H, C, True, False, up=up)
    assert case.D == 3
    got, got_g, (S, lut) = case.run(torch.float32, DEV, True)
    want, want_g, _ = case.run(torch.float64, "cpu", False)
    ref32 = lambda: case.run(torch.float32, "cpu", False)             # noqa: E731
    assert_rule(got, want, lambda: ref32()[0], "Y")
    # the two rows the pair touches, from the node sums and the table the kernel itself left (float32 products of its own values)
    S, lut, Y = S.cpu().double(), lut.cpu().double().view(-1), got.cpu().double()
    assert float(lut[2]) == 0.0
    assert float((Y[192] - (lut[0] * S[192] + lut[1] * S[0])).abs().max()) <= 1e-6 * float(Y.abs().max())
    assert float((Y[0] - lut[0] * S[0]).abs().max()) <= 1e-6 * float(Y.abs().max())
    assert float((Y[:192] - lut[0] * S[:192]).abs().max()) <= 1e-6 * float(Y.abs().max())
    assert_grads_rule(list(got_g), list(want_g), lambda: list(ref32()[1]), "gradients")


def _graphs(sizes, F, seed=3):
    """Random trees with a few extra edges (connected, diameters far below 63 hops), one-hot features: test_gpu_graphed._graph_task's."""
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


def _graph_model(F, hidden=32, seed=0):
    from gnan_amd.models import TensorGNAN
    torch.manual_seed(seed)
    m = TensorGNAN(F, 1, 3, hidden_channels=hidden, is_graph_task=True, readout_n_layers=0, device=DEV)
    with torch.no_grad():
        for _, p in m.named_parameters():
            p.copy_(torch.randn(p.shape) * 0.3)
    return m.to(DEV).eval()


@pytest.fixture(scope="module")
def graphs():
    _need_gpu()
    return _graphs([130, 200, 417], 15)


@pytest.mark.parametrize("which", [0, 1, 2])
def test_the_modules_take_the_route(which, graphs, monkeypatch):
    """models.TensorGNAN on dense graphs of 130, 200 and 417 nodes: forward and every parameter gradient == the float64 oracle;
    with MID_GRAPH off (the general route) the same within two floors; the entry point is called with the flag on, not with it off."""
    from gnan_amd import _lib, replay, small_graph
    monkeypatch.setattr(replay, "REPLAY_FORWARD", False)
    data = graphs[which]
    m = _graph_model(15)
    calls = []
    real = _lib.lib().gnan_mid_graph_fwd

    def counted(a, stream):
        calls.append(a.n)
        return real(a, stream)
    monkeypatch.setattr(_lib.lib(), "gnan_mid_graph_fwd", counted)
    stages = []
    m.stage_hook = stages.append

    def run():
        m.zero_grad(set_to_none=True)
        out = m.forward(data)
        out.sum().backward()
        return out.detach().clone(), {k: p.grad.detach().clone() for k, p in m.named_parameters()}
    got, got_g = run()
    assert calls == [data.x.shape[0]] and stages == ["start", "lut", "fmlp", "spmm"]
    monkeypatch.setattr(small_graph, "MID_GRAPH", False)
    general, general_g = run()
    assert len(calls) == 1                                            # (not taken with the flag off)
    monkeypatch.setattr(small_graph, "MID_GRAPH", True)

    def oracle(dtype):
        p = {k: v.detach().cpu().to(dtype).clone().requires_grad_(True) for k, v in m.state_dict().items()}
        out = O.tensor_gnan_forward_models(data.x.cpu().to(dtype), data.node_distances.cpu().to(dtype),
                                           data.normalization_matrix.cpu().to(dtype), p, True, True, 0)
        out.sum().backward()
        return out.detach(), {k: v.grad for k, v in p.items()}
    want, want_g = oracle(torch.float64)
    assert got.shape == want.shape == (1, 1)
    assert_rule(got, want, lambda: oracle(torch.float32)[0], "forward")
    assert_grads_rule(got_g, want_g, lambda: oracle(torch.float32)[1], "gradients")
    assert float((got - general).abs().max()) <= TWO_FLOORS * float(want.abs().max())
    scale = max(float(v.abs().max()) for v in want_g.values())
    for k in got_g:
        assert float((got_g[k] - general_g[k]).abs().max()) <= TWO_FLOORS * scale, k


def test_the_route_inside_a_replayed_training_step(graphs, monkeypatch):
    """Six training steps on ONE 200-node graph object: the replay plan (forward + backward, gnan_amd.replay) is captured with
    the new kernels in it and replayed; parameters == a twin with the replay switched off."""
    from gnan_amd import replay
    data = graphs[1]
    loss_fn = torch.nn.BCEWithLogitsLoss()
    a = _graph_model(15)
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
    cache = b.__dict__.get("_replays")
    plans = [] if cache is None else [r.value["plan"] for r in cache.entries.values() if r.value["plan"] is not None]
    train = [p for p in plans if p.grad]
    assert train and all(p.fwd.replays >= 1 and p.bwd.replays == p.fwd.replays for p in train)
    replay.release(b)
