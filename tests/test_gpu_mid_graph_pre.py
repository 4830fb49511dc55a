"""Pre-rho normalisation (GNAN.py:65-67: the weight of pair (i, j) is rho(u_d / |shell_i(d)|)) on the one-launch route of dense-coded
graphs of 129 to 448 nodes (csrc/mid_graph.hip with ``reserved = GNAN_MID_PRE_RHO``; small_graph.mid_graph_forward(..., "pre", ...)):
the kernels against the float64 chain written out on the CPU, a tile-edge probe, the small route's bits where both cover, the general
route, the stand-alone module class, a replayed training step and training-mode Dropout.

Tolerances: the project's rule (helpers.assert_rule / assert_grads_rule: the float32 chain's own error beyond the 1e-5 floor) against
the truth; between the one-launch and the general route twice that bound (each lies within it of the same truth)."""
import copy
import functools
import warnings

import numpy as np
import pytest
import torch

import reference_loop
import test_gpu_small_graph_dropout as drop_tests
from helpers import assert_grads_rule, assert_rule, grad_rule, rule
from oracle import gnan_oracle as O
from test_gpu_graphed import DEV, _need_gpu
from test_gpu_mid_graph import _graph_of, _graphs, _mlps

pytestmark = pytest.mark.gpu

PRE = 1                       # GNAN_MID_PRE_RHO


@pytest.fixture(autouse=True)
def switch_on(monkeypatch):
    """The route's switch follows a measured rule: the tests do not depend on how it ships."""
    from gnan_amd import small_graph
    monkeypatch.setattr(small_graph, "MID_GRAPH_PRE_RHO", True)


class _Case:
    """One graph, one pair of MLPs, one upstream gradient: a route of the build on the device, the chain written out on the CPU."""

    def __init__(self, hops, x, fp, rp, L, H, C, graph_sum, up=None):
        self.hops, self.x, self.fp, self.rp, self.L, self.H, self.C, self.graph_sum = hops, x, fp, rp, L, H, C, graph_sum
        self.n, self.F = x.shape
        self.g = _graph_of(hops)
        self.D = self.g.n_codes
        shape = (C, 1) if graph_sum else (self.n, C)
        self.up = up if up is not None else torch.from_numpy(np.random.default_rng(5).standard_normal(shape))

    def leaves(self, dtype, dev):
        fl = [None if t is None else t.to(dev, dtype).requires_grad_(True) for t in self.fp]
        rl = [None if t is None else t.to(dev, dtype).requires_grad_(True) for t in self.rp]
        return fl, rl

    def _finish(self, out, fl, rl, dev, dtype, left):
        live = [t for t in fl + rl if t is not None]
        return out.detach(), torch.autograd.grad(out, live, self.up.to(dev, dtype)), left

    def device(self, route, dropout=None):
        """-> (output, gradients of every parameter, (S, lut [n * D, 1])) by ``route``: "mid" / "small" (the one-launch routes,
        called directly) or "general" (what the modules run with the switch off: shape functions, rho's row table and
        ``pre_rho_aggregate``, the read-out sum)."""
        from gnan_amd import aggregate, functional, small_graph
        from gnan_amd.functional import StackedMLP
        from gnan_amd.graph import hop_inputs
        fl, rl = self.leaves(torch.float32, DEV)
        xs = self.x.to(DEV)
        f, r = StackedMLP(*fl, self.L, self.H, self.C, self.F), StackedMLP(*rl, self.L, self.H, 1, 1)
        if route == "general":
            S = functional.feature_mlps(xs, f, sum_features=True)
            out = aggregate.pre_rho_aggregate(self.g, S, r, hop_inputs(self.D, DEV))
            out = functional.graph_readout(out) if self.graph_sum else out
            return self._finish(out, fl, rl, DEV, torch.float32, None)
        if route == "mid" and self.n > 128:
            assert small_graph.mid_graph_pre_rho_applies(xs, self.g, f, r)
        forward = small_graph.mid_graph_forward if route == "mid" else small_graph.small_graph_forward
        out = forward(xs, self.g, f, r, "pre", self.graph_sum, **({} if dropout is None else {"dropout": dropout}))
        saved = out.grad_fn.saved_tensors
        return self._finish(out, fl, rl, DEV, torch.float32, (saved[1].detach().clone(), saved[2].detach().clone()))

    def chain(self, dtype):
        """The chain written out in ``dtype`` on the CPU: weights rho(u_d / max(cnt[i, d], 1)) gathered by hop code."""
        L, n, D = self.L, self.n, self.D
        fl, rl = self.leaves(dtype, "cpu")
        xs = self.x.to(dtype)

        def net(v, p, k):                                         # v [m] -> [m, C]
            h = torch.relu(v[:, None] * p[0][k] + (0 if p[1] is None else p[1][k]))
            if L == 3:
                h = torch.relu(h @ p[2][0, k].T + (0 if p[3] is None else p[3][0, k]))
            return h @ p[4][k].T + (0 if p[5] is None else p[5][k])
        S = sum(net(xs[:, k], fl, k) for k in range(self.F))
        u = torch.zeros(D, dtype=torch.float32)
        u[: D - 1] = 1.0 / (torch.arange(D - 1, dtype=torch.float32) + 1.0)
        arg = u.to(dtype)[None, :] / self.g.cnt.cpu().clamp_min(1).to(dtype)          # [n, D]
        lut = net(arg.reshape(-1), rl, 0)                                             # [n * D, 1]
        codes = torch.from_numpy(np.where(self.hops >= 0, self.hops, D - 1)).long()
        w = lut.view(n, D)[torch.arange(n)[:, None], codes][..., None]               # [n, n, 1]
        out = (w * S[None, :, :]).sum(1)
        out = out.sum(0).view(-1, 1) if self.graph_sum else out
        return self._finish(out, fl, rl, "cpu", dtype, (S.detach(), lut.detach()))


SHAPES = [
    # n, F, C, L, H, D, bias_f, bias_r
    (129, 15, 1, 3, 64, 3, True, False),       # one row in the third tile; 387 arguments of rho: a run with a tail
    (192, 7, 2, 3, 64, 21, True, False),       # the tile edge ...
    (193, 7, 2, 3, 64, 21, True, False),       # ... and one row past it
    (256, 4, 8, 2, 30, 64, True, False),       # eight channels, L = 2, H no multiple of 4, 64 shells, many of them empty
    (448, 3, 1, 3, 48, 64, True, False),       # the cap: 64 forward rho workgroups, 14 backward groups, two binning waves
    (200, 7, 2, 3, 32, 11, False, True),       # biases on rho and none on f
]
CASES = [s + (gs,) for s in SHAPES for gs in (False, True)]
IDS = ["n%d-F%d-C%d-L%d-H%d-D%d-%s" % (*c[:6], "sum" if c[8] else "nodes") for c in CASES]


@functools.lru_cache(maxsize=None)
def _case(i):
    _need_gpu()
    n, F, C, L, H, D, bias_f, bias_r, graph_sum = CASES[i]
    rng = np.random.default_rng(n * 7 + F)
    if n == 256:
        # every row lists eight of the 63 hops (and the rest): most of its 64 shells are empty
        own = np.stack([rng.choice(D - 1, 8, replace=False) for _ in range(n)])
        pick = rng.integers(-1, 8, (n, n))
        hops = np.where(pick >= 0, np.take_along_axis(own, np.maximum(pick, 0), axis=1), -1).astype(np.int32)
        hops[0, 1] = D - 2                                                # (the last listed hop exists: D codes)
    else:
        hops = rng.integers(-1, D - 1, (n, n)).astype(np.int32)          # -1 = unreachable
    hops[np.arange(n), np.arange(n)] = 0
    fp, rp = _mlps(rng, F, C, L, H, bias_f, bias_r)
    x = torch.from_numpy(rng.standard_normal((n, F)).astype(np.float32))
    case = _Case(hops, x, fp, rp, L, H, C, graph_sum)
    assert case.D == D
    return case


@functools.lru_cache(maxsize=None)
def _truth(i):
    """The float64 chain of case i: computed once, shared, never changed."""
    return _case(i).chain(torch.float64)


@functools.lru_cache(maxsize=None)
def _lazy32(i):
    return _case(i).chain(torch.float32)


@functools.lru_cache(maxsize=None)
def _mid(i):
    return _case(i).device("mid")


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_the_kernels_against_the_chain(i):
    """gnan_mid_graph_fwd / _bwd with reserved = 1 == the float64 chain: forward, every parameter gradient, and the node sums and
    rows' table [n, D] the forward leaves behind; two runs give the same bits."""
    case = _case(i)
    got, got_g, (S, lut) = _mid(i)
    want, want_g, (want_S, want_lut) = _truth(i)
    assert got.shape == ((case.C, 1) if case.graph_sum else (case.n, case.C)) and lut.shape == (case.n * case.D, 1)
    assert_rule(got, want, lambda: _lazy32(i)[0], "forward")
    assert_grads_rule(list(got_g), list(want_g), lambda: list(_lazy32(i)[1]), "gradients")
    assert_rule(S, want_S, lambda: _lazy32(i)[2][0], "S")
    assert_rule(lut, want_lut, lambda: _lazy32(i)[2][1], "lut")
    again, again_g, (again_S, again_lut) = case.device("mid")
    assert torch.equal(got, again) and all(torch.equal(a, b) for a, b in zip(got_g, again_g))
    assert torch.equal(S, again_S) and torch.equal(lut, again_lut)
    if case.n == 256:
        # most (row, shell) arguments are shells no pair of the row lies in: they weigh nothing and hand rho no gradient — the chain
        # above evaluates rho's gradient through the gathered (non-empty) entries only, and rho's gradients follow it by the rule
        cnt = case.g.cnt.cpu()
        listed = torch.zeros(case.n, case.D, dtype=torch.bool)
        codes = torch.from_numpy(np.where(case.hops >= 0, case.hops, case.D - 1)).long()
        listed[torch.arange(case.n)[:, None], codes] = True
        assert int((~listed).sum()) > case.n * case.D // 2 and bool((cnt[~listed] == 0).all())
        n_f = sum(t is not None for t in case.fp)
        assert_grads_rule(list(got_g[n_f:]), list(want_g[n_f:]), lambda: list(_lazy32(i)[1][n_f:]), "rho's gradients")


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_against_the_general_route(i):
    """The same case through the general kernels: the two routes differ by at most 2 max(1e-5, the float32 chain's own error)
    relative to the float64 scale, forward and gradients — each lies within that bound of the truth by the rule."""
    case = _case(i)
    got, got_g, _ = _mid(i)
    gen, gen_g, _ = case.device("general")
    want, want_g, _ = _truth(i)
    assert_rule(gen, want, lambda: _lazy32(i)[0], "general forward")
    assert_grads_rule(list(gen_g), list(want_g), lambda: list(_lazy32(i)[1]), "general gradients")
    e32 = rule(_lazy32(i)[0], want)[1]                                # (rule(x, truth): x's own error relative to the truth's scale)
    print("forward: float32 chain", e32, "routes apart", float((got - gen).abs().max()) / float(want.abs().max()))
    assert float((got - gen).abs().max()) <= 2 * max(1e-5, e32) * float(want.abs().max())
    as_dict = lambda v: dict(enumerate(v))                            # noqa: E731
    g32 = grad_rule(as_dict(_lazy32(i)[1]), as_dict(want_g))[1]
    scale = max(float(w.abs().max()) for w in want_g)
    apart = max(float((a - b).abs().max()) for a, b in zip(got_g, gen_g)) / scale
    print("gradients: float32 chain", g32, "routes apart", apart)
    assert apart <= 2 * max(1e-5, g32)


def test_one_pair_across_a_tile_edge():
    """193 nodes, every pair unreachable but the diagonal and the single pair (192, 0) at hop 1: rho has no bias, so the rest shell
    weighs rho(0 / cnt) = 0 and the pair's weight is all that links two rows — Y[192] = lut[192, 0] S[192] + lut[192, 1] S[0] from
    the fourth tile's only row, out of the kernel's own S and rows' table; upstream gradient on row 192 only."""
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
    case = _Case(hops, x, fp, rp, L, H, C, False, up=up)
    assert case.D == 3
    got, got_g, (S, lut) = case.device("mid")
    want, want_g, _ = case.chain(torch.float64)
    ref32 = functools.lru_cache(maxsize=None)(lambda: case.chain(torch.float32))
    assert_rule(got, want, lambda: ref32()[0], "Y")
    S, lut, Y = S.cpu().double(), lut.cpu().double().view(n, 3), got.cpu().double()
    assert float(lut[:, 2].abs().max()) == 0.0
    top = float(Y.abs().max())
    assert float((Y[192] - (lut[192, 0] * S[192] + lut[192, 1] * S[0])).abs().max()) <= 1e-6 * top
    assert float((Y[0] - lut[0, 0] * S[0]).abs().max()) <= 1e-6 * top
    assert float((Y[:192] - lut[:192, :1] * S[:192]).abs().max()) <= 1e-6 * top
    assert_grads_rule(list(got_g), list(want_g), lambda: list(ref32()[1]), "gradients")


@pytest.mark.parametrize("n", [100, 128])
@pytest.mark.parametrize("graph_sum", [False, True])
def test_the_small_routes_bits_where_both_cover(n, graph_sum):
    """gnan_mid_graph_fwd takes every n <= 448: at 100 and 128 nodes its pre-rho forward returns gnan_small_graph_fwd's bits —
    outputs, node sums and rows' table (the same arithmetic in the same orders)."""
    _need_gpu()
    F, C, L, H, D = 7, 2, 3, 32, 11
    rng = np.random.default_rng(n)
    hops = rng.integers(-1, D - 1, (n, n)).astype(np.int32)
    hops[np.arange(n), np.arange(n)] = 0
    fp, rp = _mlps(rng, F, C, L, H, True, True)
    case = _Case(hops, torch.from_numpy(rng.standard_normal((n, F)).astype(np.float32)), fp, rp, L, H, C, graph_sum)
    mid, _, (mid_S, mid_lut) = case.device("mid")
    small, _, (small_S, small_lut) = case.device("small")
    assert torch.equal(mid, small) and torch.equal(mid_S, small_S) and torch.equal(mid_lut, small_lut)
    assert mid_lut.shape == (n * case.D, 1)


# ---- the modules -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def graphs():
    _need_gpu()
    return _graphs([130, 200, 417], 15)


def _model(graph_task, out_channels=1, seed=0):
    from gnan_amd import GNAN as standalone
    torch.manual_seed(seed)
    m = standalone.TensorGNAN(15, out_channels, 3, hidden_channels=32, is_graph_task=graph_task, device=DEV)
    assert m.normalize_rho is True                                    # the class's default
    with torch.no_grad():
        for _, p in m.named_parameters():
            p.copy_(torch.randn(p.shape) * 0.3)
    return m.to(DEV).eval()


class _Counted:
    """``gnan_mid_graph_fwd`` with the ``reserved`` word of every call noted."""

    def __init__(self, monkeypatch):
        from gnan_amd import _lib
        self.flags = []
        real = _lib.lib().gnan_mid_graph_fwd

        def counted(a, stream):
            self.flags.append(a.reserved)
            return real(a, stream)
        monkeypatch.setattr(_lib.lib(), "gnan_mid_graph_fwd", counted)


def _oracle(m, data, dtype, graph_task):
    p = {k: v.detach().cpu().to(dtype).clone().requires_grad_(True) for k, v in m.state_dict().items()}
    out = O.tensor_gnan_forward_standalone(data.x.cpu().to(dtype), data.node_distances.cpu().to(dtype),
                                           data.normalization_matrix.cpu().to(dtype), p, True, graph_task)
    out.sum().backward()
    return out.detach(), {k: v.grad for k, v in p.items()}


def _run(m, data):
    m.zero_grad(set_to_none=True)
    out = m.forward(data)
    out.sum().backward()
    return out.detach().clone(), {k: p.grad.detach().clone() for k, p in m.named_parameters()}


@pytest.mark.parametrize("which", [0, 1, 2])
@pytest.mark.parametrize("graph_task", [True, False], ids=["graph", "node"])
def test_the_stand_alone_class_takes_the_route(which, graph_task, graphs, monkeypatch):
    """GNAN.TensorGNAN with its default normalize_rho on dense graphs of 130, 200 and 417 nodes, as a graph task and as a node task
    (rho has a bias): forward and every parameter gradient == the float64 oracle by the rule; gnan_mid_graph_fwd is called once,
    with reserved == 1 — and not at all with the switch off, which is right by the rule too."""
    from gnan_amd import replay, small_graph
    monkeypatch.setattr(replay, "REPLAY_FORWARD", False)
    data = graphs[which]
    m = _model(graph_task)
    assert (m.rho[0].bias is not None) == (not graph_task)
    calls = _Counted(monkeypatch)
    stages = []
    m.stage_hook = stages.append
    got, got_g = _run(m, data)
    assert calls.flags == [PRE] and stages == ["start", "lut", "fmlp", "spmm"]
    monkeypatch.setattr(small_graph, "MID_GRAPH_PRE_RHO", False)
    general, general_g = _run(m, data)
    assert calls.flags == [PRE]                                       # (not taken with the switch off)
    monkeypatch.setattr(small_graph, "MID_GRAPH_PRE_RHO", True)
    want, want_g = _oracle(m, data, torch.float64, graph_task)
    lazy = functools.lru_cache(maxsize=None)(lambda: _oracle(m, data, torch.float32, graph_task))
    assert got.shape == want.shape == ((1, 1) if graph_task else (data.x.shape[0], 1))
    assert_rule(got, want, lambda: lazy()[0], "forward")
    assert_grads_rule(got_g, want_g, lambda: lazy()[1], "gradients")
    assert_rule(general, want, lambda: lazy()[0], "general forward")
    assert_grads_rule(general_g, want_g, lambda: lazy()[1], "general gradients")


def test_a_rho_of_two_channels_keeps_the_general_route(graphs, monkeypatch):
    from gnan_amd import replay
    monkeypatch.setattr(replay, "REPLAY_FORWARD", False)
    data = graphs[0]
    m = _model(True, out_channels=2)
    calls = _Counted(monkeypatch)
    got, got_g = _run(m, data)
    assert calls.flags == []
    want, want_g = _oracle(m, data, torch.float64, True)
    lazy = functools.lru_cache(maxsize=None)(lambda: _oracle(m, data, torch.float32, True))
    assert got.shape == want.shape == (2, 1)
    assert_rule(got, want, lambda: lazy()[0], "forward")
    assert_grads_rule(got_g, want_g, lambda: lazy()[1], "gradients")


def test_the_route_inside_a_replayed_training_step(graphs, monkeypatch):
    """Six training steps on ONE 200-node graph object: the replay plan (forward + backward, gnan_amd.replay) is captured with the
    pre-rho kernels in it and replayed; parameters == a twin with the replay switched off (test_gpu_mid_graph's bound)."""
    from gnan_amd import replay
    data = graphs[1]
    loss_fn = torch.nn.BCEWithLogitsLoss()
    a = _model(True)
    b = copy.deepcopy(a)
    oa, ob = torch.optim.Adam(a.parameters(), lr=1e-3), torch.optim.Adam(b.parameters(), lr=1e-3)
    calls = _Counted(monkeypatch)
    for e in range(6):
        monkeypatch.setattr(replay, "REPLAY_FORWARD", False)
        ta = reference_loop.train_epoch(a, [data], loss_fn, oa, DEV, classify=True, is_graph_task=True)
        monkeypatch.setattr(replay, "REPLAY_FORWARD", True)
        tb = reference_loop.train_epoch(b, [data], loss_fn, ob, DEV, classify=True, is_graph_task=True)
        assert abs(ta[0] - tb[0]) <= 1e-5 * max(1.0, abs(ta[0])) and ta[1] == tb[1], (e, ta, tb)
        scale = max(float(v.abs().max()) for v in a.state_dict().values())
        for (k, va), (_, vb) in zip(a.state_dict().items(), b.state_dict().items()):
            assert float((va - vb).abs().max()) <= 1e-5 * scale, (e, k)
    assert calls.flags and set(calls.flags) == {PRE}
    cache = b.__dict__.get("_replays")
    plans = [] if cache is None else [r.value["plan"] for r in cache.entries.values() if r.value["plan"] is not None]
    train = [p for p in plans if p.grad]
    assert train and all(p.fwd.replays >= 1 and p.bwd.replays == p.fwd.replays for p in train)
    replay.release(b)


# ---- training-mode Dropout ---------------------------------------------------------------------------------------------------------
P, SEED = drop_tests.P, drop_tests.SEED


class _DropCase(drop_tests._Case):
    """The existing Dropout test's case (its chain: O.feature_mlps under the kernels' masks, O.row_lut_pre_rho) on the mid route
    under pre-rho."""

    def fused(self, dropout, r_grad=True):
        from gnan_amd.functional import StackedMLP
        from gnan_amd.small_graph import mid_graph_forward, mid_graph_pre_rho_applies
        fl, rl = self.leaves(torch.float32, DEV, True, r_grad)
        xs = self.x.to(DEV)
        f, r = StackedMLP(*fl, self.L, self.H, self.C, self.F), StackedMLP(*rl, self.L, self.H, 1, 1)
        assert self.use_cnt == "pre" and mid_graph_pre_rho_applies(xs, self.g, f, r)
        out = mid_graph_forward(xs, self.g, f, r, "pre", self.graph_sum, dropout=dropout)
        live = [(i, t) for i, t in enumerate(fl + rl) if t is not None and t.requires_grad]
        grads = torch.autograd.grad(out, [t for _, t in live], self.up.to(DEV, torch.float32))
        return out.detach(), {i: g for (i, _), g in zip(live, grads)}


DROP_CASES = [(129, 15, drop_tests.A, "pre", True), (129, 1, drop_tests.B, "pre", False), (448, 3, drop_tests.B, "pre", True),
              (448, 1, drop_tests.C8, "pre", False)]
DROP_IDS = ["n%d-F%d-L%dH%dC%d-%s" % (n, F, s[0], s[1], s[2], "sum" if gs else "nodes") for n, F, s, _, gs in DROP_CASES]


@functools.lru_cache(maxsize=None)
def _drop_case(i):
    _need_gpu()
    return _DropCase(*DROP_CASES[i])


@pytest.mark.parametrize("i", range(len(DROP_CASES)), ids=DROP_IDS)
def test_dropout_against_the_chain_under_the_kernels_masks(i):
    """gnan_mid_graph_fwd_drop / _bwd_drop with reserved = 1 at 129 and 448 nodes == the float64 chain under
    functional.dropout_masks(seed, p, ...); a seed fixes the bits, the next seed changes them; p = 0 is the plain entry point bit
    for bit; a seed cell (``_drop_dev``) gives the bits of the same seed by value."""
    from gnan_amd import small_graph
    case = _drop_case(i)
    masks = case.masks()
    got, got_g = case.fused((P, SEED))
    want, want_g = case.chain(torch.float64, masks)
    lazy = functools.lru_cache(maxsize=None)(lambda: case.chain(torch.float32, masks))
    assert got.shape == want.shape and sorted(got_g) == sorted(want_g)
    assert_rule(got, want, lambda: lazy()[0], "forward")
    assert_grads_rule(got_g, want_g, lambda: lazy()[1], "gradients")
    plain64, _ = case.chain(torch.float64, None)
    assert float((plain64 - want).abs().max()) > 1e-3 * float(want.abs().max())          # the masks matter
    again, again_g = case.fused((P, SEED))
    assert torch.equal(got, again) and all(torch.equal(got_g[k], again_g[k]) for k in got_g)
    other, _ = case.fused((P, SEED + 1))
    assert not torch.equal(got, other)
    # p = 0 through the _drop entry points: the plain kernels' bits
    plain, plain_g = case.fused(None)
    zero, zero_g = case.fused((0.0, SEED))
    assert torch.equal(plain, zero) and all(torch.equal(plain_g[k], zero_g[k]) for k in plain_g)
    # the seed in a device cell
    cell = small_graph.seed_cell(DEV)
    small_graph.seed_cell_set(cell, SEED)
    dev, dev_g = case.fused((P, cell))
    assert torch.equal(got, dev) and all(torch.equal(got_g[k], dev_g[k]) for k in got_g)


def test_the_stand_alone_class_keeps_the_route_in_training_mode(graphs, monkeypatch):
    """GNAN.TensorGNAN(dropout = 0.6).train() on the 130-node graph: the ``_drop`` entry points with reserved == 1, one seed draw
    per forward; with the switch off the general Dropout route gives the same masks (the same manual_seed)."""
    from gnan_amd import GNAN as standalone
    from gnan_amd import _lib, replay, small_graph
    from helpers import TWO_FLOORS
    monkeypatch.setattr(replay, "REPLAY_FORWARD", False)
    torch.manual_seed(0)
    m = standalone.TensorGNAN(15, 1, 3, hidden_channels=32, dropout=P, is_graph_task=True, device=DEV)
    with torch.no_grad():
        for _, p in m.named_parameters():
            p.copy_(torch.randn(p.shape) * 0.3)
    m = m.to(DEV).train()
    flags = []
    real = _lib.lib().gnan_mid_graph_fwd_drop

    def counted(a, d, stream):
        flags.append(a.reserved)
        return real(a, d, stream)
    monkeypatch.setattr(_lib.lib(), "gnan_mid_graph_fwd_drop", counted)

    def step(seed=7):
        m.zero_grad(set_to_none=True)
        torch.manual_seed(seed)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            out = m.forward(graphs[0])
        out.pow(2).sum().backward()
        return out.detach().clone(), {k: p.grad.detach().clone() for k, p in m.named_parameters()}
    one, one_g = step()
    assert flags == [PRE]
    two, _ = step()
    assert torch.equal(one, two) and not torch.equal(one, step(8)[0])
    del flags[:]
    monkeypatch.setattr(small_graph, "MID_GRAPH_PRE_RHO", False)
    gen, gen_g = step()
    assert flags == []
    assert float((one - gen).abs().max()) <= TWO_FLOORS * float(gen.abs().max())
    scale = max(float(v.abs().max()) for v in gen_g.values())
    for k in gen_g:
        assert float((one_g[k] - gen_g[k]).abs().max()) <= TWO_FLOORS * scale, k
