"""Training-mode Dropout on the one-launch graph routes (gnan_small_graph_fwd_drop / _bwd_drop, gnan_mid_graph_fwd_drop / _bwd_drop;
small_graph.small_graph_forward / mid_graph_forward with ``dropout=(p, seed)``): the kernels against the float64 oracle chain fed
with the kernels' own keep-masks (``functional.dropout_masks``), at the node-block and tile edges of both routes; the general
backward behind a masked forward; seeds; the Dropout-free calls bit for bit; the three module classes; the gates that stay shut.

Tolerances: the project's rule (helpers.assert_rule / assert_grads_rule: the float32 oracle chain's own error beyond the floor)
against the truth, TWO_FLOORS between two routes of the build."""
import copy
import functools
import warnings

import numpy as np
import pytest
import torch

from helpers import TWO_FLOORS, assert_grads_rule, assert_rule
from oracle import gnan_oracle as O
from test_gpu_graphed import DEV, Bag, _need_gpu

pytestmark = pytest.mark.gpu

P = 0.6
SEED = 0xC2B2AE3D27D4EB4F                      # 64 bits, the upper half (and the top bit) set

A, B, C8 = (3, 64, 1, True), (3, 48, 3, False), (2, 8, 8, True)      # (L, H, C, bias of f)
CASES = [
    # n, F, stack, use_cnt, graph_sum                 small route: one node block (n <= 64) or two
    (1, 1, A, False, True),
    (30, 15, A, True, True),
    (30, 15, B, "pre", False),
    (64, 1, B, "pre", True),
    (64, 15, C8, False, False),
    (65, 15, B, True, False),
    (65, 1, C8, "pre", True),
    (128, 15, C8, False, True),
    (128, 1, A, "pre", False),
    # mid route: 129 = one row into the third tile; 200 = 0 mod 4: the padded code stride; 448: seven full tiles
    (129, 15, A, True, True),
    (129, 1, B, False, False),
    (200, 1, C8, True, True),
    (200, 15, B, True, False),
    (448, 15, A, True, True),
    (448, 1, C8, False, False),
]
IDS = ["n%d-F%d-L%dH%dC%d-%s-%s" % (n, F, s[0], s[1], s[2], {False: "nocnt", True: "cnt", "pre": "pre"}[u], "sum" if gs else "nodes")
       for n, F, s, u, gs in CASES]


class _Case:
    """One graph, one pair of stacks, one upstream gradient; the fused route on the device and the oracle chain on the CPU."""

    def __init__(self, n, F, stack, use_cnt, graph_sum):
        from gnan_amd import HopGraph
        self.n, self.F, (self.L, self.H, self.C, bias), self.use_cnt, self.graph_sum = n, F, stack, use_cnt, graph_sum
        L, H, C = self.L, self.H, self.C
        rng = np.random.default_rng(1000 * n + F)
        hops = rng.integers(-1, 6, (n, n)).astype(np.int32)               # -1 = unreachable
        hops[np.arange(n), np.arange(n)] = 0
        nd = torch.zeros(n, n)
        nd[torch.from_numpy(hops >= 0)] = 1.0 / (torch.from_numpy(hops[hops >= 0]).float() + 1.0)
        self.g = HopGraph.from_dense(nd.to(DEV))
        self.D = self.g.n_codes
        self.codes = torch.from_numpy(np.where(hops >= 0, hops, self.D - 1)).long()
        self.cnt = self.g.cnt.cpu().numpy()
        t = lambda *s: torch.from_numpy((rng.standard_normal(s) * 0.5).astype(np.float32))      # noqa: E731

        def mlp(Fk, Ck, b):
            return [t(Fk, H), t(Fk, H) if b else None, t(1, Fk, H, H) if L == 3 else None, t(1, Fk, H) if (L == 3 and b) else None,
                    t(Fk, Ck, H), t(Fk, Ck) if b else None]
        self.fp, self.rp = mlp(F, C, bias), mlp(1, 1, not bias)
        self.x = torch.from_numpy(rng.standard_normal((n, F)).astype(np.float32))
        self.up = torch.from_numpy(rng.standard_normal((C, 1) if graph_sum else (n, C)))

    def leaves(self, dtype, dev, f_grad=True, r_grad=True):
        fl = [None if t is None else t.to(dev, dtype).requires_grad_(f_grad) for t in self.fp]
        rl = [None if t is None else t.to(dev, dtype).requires_grad_(r_grad) for t in self.rp]
        return fl, rl

    def fused(self, dropout, r_grad=True):
        """-> (output, {index: gradient} over f's six and rho's six stacked tensors that exist and want one)"""
        from gnan_amd.functional import StackedMLP
        from gnan_amd.small_graph import mid_graph_applies, mid_graph_forward, small_graph_applies, small_graph_forward
        fl, rl = self.leaves(torch.float32, DEV, True, r_grad)
        xs = self.x.to(DEV)
        f, r = StackedMLP(*fl, self.L, self.H, self.C, self.F), StackedMLP(*rl, self.L, self.H, 1, 1)
        if self.n > 128:
            assert mid_graph_applies(xs, self.g, f, r, self.use_cnt)
            out = mid_graph_forward(xs, self.g, f, r, self.use_cnt, self.graph_sum, dropout=dropout)
        else:
            assert small_graph_applies(xs, self.g, f, r, pre_rho=self.use_cnt == "pre")
            out = small_graph_forward(xs, self.g, f, r, self.use_cnt, self.graph_sum, dropout=dropout)
        live = [(i, t) for i, t in enumerate(fl + rl) if t is not None and t.requires_grad]
        grads = torch.autograd.grad(out, [t for _, t in live], self.up.to(DEV, torch.float32))
        return out.detach(), {i: g for (i, _), g in zip(live, grads)}

    def masks(self, seed=SEED, p=P):
        from gnan_amd.functional import dropout_masks
        return dropout_masks(seed, p, self.n, self.F, self.L - 1, self.H, DEV).cpu()

    def chain(self, dtype, keep):
        """The oracle's pieces in ``dtype``: shape functions under the given keep-masks summed over the features, rho's table
        (O.rho_lut, or per row O.row_lut_pre_rho), the normalised weight table (O.weight_table), the dense sum over hop codes."""
        fl, rl = self.leaves(dtype, "cpu")
        L, n, D = self.L, self.n, self.D
        params = {}
        for k in range(self.F):
            params["fs.%d.0.weight" % k] = fl[0][k].unsqueeze(1)
            params["fs.%d.3.weight" % k] = fl[2][0, k] if L == 3 else fl[4][k]
            if L == 3:
                params["fs.%d.6.weight" % k] = fl[4][k]
            if fl[1] is not None:
                params["fs.%d.0.bias" % k] = fl[1][k]
                params["fs.%d.3.bias" % k] = fl[3][0, k] if L == 3 else fl[5][k]
                if L == 3:
                    params["fs.%d.6.bias" % k] = fl[5][k]
        params["rho.0.weight"] = rl[0][0].unsqueeze(1)
        params["rho.2.weight"] = rl[2][0, 0] if L == 3 else rl[4][0]
        if L == 3:
            params["rho.4.weight"] = rl[4][0]
        if rl[1] is not None:
            params["rho.0.bias"] = rl[1][0]
            params["rho.2.bias"] = rl[3][0, 0] if L == 3 else rl[5][0]
            if L == 3:
                params["rho.4.bias"] = rl[5][0]
        S = O.feature_mlps(self.x.to(dtype), params, "fs", keep=keep, drop_p=P).sum(1)                 # [n, C]
        if self.use_cnt == "pre":
            wtab = O.row_lut_pre_rho(params, self.cnt, dtype)                                          # [n, D, 1]
        else:
            wtab = O.weight_table(O.rho_lut(params, D, dtype), self.cnt if self.use_cnt else None)     # [n or 1, D, 1]
        w = wtab.expand(n, D, 1)[torch.arange(n)[:, None], self.codes]                                 # [n, n, 1]
        out = (w * S[None, :, :]).sum(1)
        out = out.sum(0).view(-1, 1) if self.graph_sum else out
        live = [(i, t) for i, t in enumerate(fl + rl) if t is not None]
        grads = torch.autograd.grad(out, [t for _, t in live], self.up.to(dtype))
        return out.detach(), {i: g for (i, _), g in zip(live, grads)}


@functools.lru_cache(maxsize=None)
def _case(i):
    _need_gpu()
    return _Case(*CASES[i])


@functools.lru_cache(maxsize=None)
def _truth(i):
    """The float64 chain of case i under the kernels' masks for (P, SEED): computed once, shared, never changed."""
    case = _case(i)
    return case.chain(torch.float64, case.masks())


@functools.lru_cache(maxsize=None)
def _lazy32(i):
    case = _case(i)
    return case.chain(torch.float32, case.masks())


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_forward_and_one_launch_backward_against_the_oracle_chain(i):
    """Both gradients wanted: one launch each way.  The forward and the gradient of EVERY parameter of f and rho."""
    case = _case(i)
    got, got_g = case.fused((P, SEED))
    want, want_g = _truth(i)
    assert got.shape == want.shape == ((case.C, 1) if case.graph_sum else (case.n, case.C))
    assert sorted(got_g) == sorted(want_g)
    assert_rule(got, want, lambda: _lazy32(i)[0], "forward")
    assert_grads_rule(got_g, want_g, lambda: _lazy32(i)[1], "gradients")
    # ... and the masks matter: the Dropout-free chain is somewhere else entirely
    plain, _ = case.chain(torch.float64, None)
    assert float((plain - want).abs().max()) > 1e-3 * float(want.abs().max())


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_general_backward_behind_a_masked_forward(i):
    """Only f's parameters want a gradient: the general backward runs (pre-rho: the one launch, whatever is wanted) — f's
    gradients come from gnan_fmlp_bwd under the forward's (p, seed), and still match the oracle's."""
    case = _case(i)
    got, got_g = case.fused((P, SEED), r_grad=False)
    want, want_g = _truth(i)
    assert sorted(got_g) == [k for k in sorted(want_g) if k < 6]
    assert_rule(got, want, lambda: _lazy32(i)[0], "forward")
    f_only = lambda g: {k: v for k, v in g.items() if k < 6}             # noqa: E731
    assert_grads_rule(got_g, f_only(want_g), lambda: f_only(_lazy32(i)[1]), "f's gradients")


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_a_seed_fixes_the_bits_and_the_next_seed_changes_them(i):
    case = _case(i)
    a, a_g = case.fused((P, SEED))
    b, b_g = case.fused((P, SEED))
    assert torch.equal(a, b) and all(torch.equal(a_g[k], b_g[k]) for k in a_g)
    c, _ = case.fused((P, SEED + 1))
    assert not torch.equal(a, c)


class _Spy:
    """``_lib.lib()`` with the calls of the ``_drop`` entry points noted."""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        fn = getattr(self.real, name)
        if not name.endswith("_drop"):
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


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_no_dropout_is_the_plain_call_bit_for_bit(i, spy):
    """``dropout=None`` goes through the plain entry points; p = 0 through the ``_drop`` entry points launches the plain entry
    points' kernels: the same bits, forward and gradients (and the node sums and table the forward leaves)."""
    case = _case(i)
    plain, plain_g = case.fused(None)
    assert spy.calls == []
    route = "gnan_mid_graph" if case.n > 128 else "gnan_small_graph"
    zero, zero_g = case.fused((0.0, SEED))
    assert spy.calls == [route + "_fwd_drop", route + "_bwd_drop"]
    assert torch.equal(plain, zero) and sorted(plain_g) == sorted(zero_g)
    assert all(torch.equal(plain_g[k], zero_g[k]) for k in plain_g)
    want, want_g = case.chain(torch.float64, None)
    lazy = functools.lru_cache(maxsize=None)(lambda: case.chain(torch.float32, None))
    assert_rule(plain, want, lambda: lazy()[0], "Dropout-free forward")
    assert_grads_rule(plain_g, want_g, lambda: lazy()[1], "Dropout-free gradients")


# ---- the modules -----------------------------------------------------------------------------------------------------------------
def _graph(n, F, seed=3):
    """A random tree with a few extra edges, one-hot features (test_gpu_mid_graph._graphs)."""
    rng = np.random.default_rng(seed + n)
    ei = np.stack([np.arange(1, n), rng.integers(0, np.arange(1, n))]) if n > 1 else np.zeros((2, 0), dtype=np.int64)
    extra = np.stack([rng.integers(0, n, n // 4 + 1), rng.integers(0, n, n // 4 + 1)])
    ei = np.concatenate([ei, extra], axis=1)
    nd, norm = O.pre_process_dense(np.concatenate([ei, ei[::-1]], axis=1), n)
    x = torch.zeros(n, F)
    x[torch.arange(n), torch.from_numpy(rng.integers(0, F - 1, n))] = 1.0
    x[:, -1] = 1.0
    return Bag(x=x.to(DEV), y=None, edge_index=None, node_distances=nd.to(DEV), normalization_matrix=norm.to(DEV))


@functools.lru_cache(maxsize=None)
def _graph_cached(n):
    _need_gpu()
    return _graph(n, 15)


def _model(kind, F=15, hidden=32):
    from gnan_amd import GNAN as standalone
    from gnan_amd import models
    torch.manual_seed(0)
    if kind == "models_tensor":
        m = models.TensorGNAN(F, 1, 3, hidden_channels=hidden, dropout=P, is_graph_task=True, readout_n_layers=0, device=DEV)
    elif kind == "models_gnan":
        m = models.GNAN(F, 2, num_layers=3, hidden_channels=hidden, dropout=P, device=DEV)
    elif kind == "standalone_tensor":
        m = standalone.TensorGNAN(F, 1, 3, hidden_channels=hidden, dropout=P, is_graph_task=True, device=DEV)
    else:
        raise ValueError(kind)
    with torch.no_grad():
        for _, p in m.named_parameters():
            p.copy_(torch.randn(p.shape) * 0.3)
    return m.to(DEV).train()


def _step(m, data, seed=7, **kw):
    m.zero_grad(set_to_none=True)
    torch.manual_seed(seed)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                # (the one-time note of _check_dropout)
        out = m.forward(data, **kw)
    out.pow(2).sum().backward()
    return out.detach().clone(), {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("kind,n", [("models_tensor", 30), ("models_tensor", 130), ("models_gnan", 30), ("models_gnan", 130),
                                    ("standalone_tensor", 30)])
def test_the_modules_keep_their_one_launch_route_in_training_mode(kind, n, spy, monkeypatch):
    from gnan_amd import functional, replay, small_graph
    monkeypatch.setattr(replay, "REPLAY_FORWARD", False)
    data = _graph_cached(n)
    m = _model(kind)
    assert m.training and m._dropout_active()
    route = "gnan_mid_graph" if n > 128 else "gnan_small_graph"

    def refuse(*a, **k):
        raise AssertionError("the general Dropout route was taken")
    with monkeypatch.context() as mp:                                  # the general Dropout route is out of reach: forward and
        mp.setattr(functional, "feature_mlps_dropout", refuse)         # backward succeed all the same
        one, one_g = _step(m, data)
        assert spy.calls == [route + "_fwd_drop", route + "_bwd_drop"]
        two, _ = _step(m, data)
        assert torch.equal(one, two)                                   # torch.manual_seed fixes the masks
        other, _ = _step(m, data, seed=8)
        assert not torch.equal(one, other)
    assert all(torch.isfinite(v).all() for v in one_g.values()) and len(one_g) == len(list(m.named_parameters()))
    # the general route under the same manual_seed: the same seed draw, the same masks
    del spy.calls[:]
    monkeypatch.setattr(small_graph, "SMALL_GRAPH_DROPOUT", False)
    gen, gen_g = _step(m, data)
    monkeypatch.setattr(small_graph, "SMALL_GRAPH_DROPOUT", True)
    assert spy.calls == []
    assert float((one - gen).abs().max()) <= TWO_FLOORS * float(gen.abs().max())
    scale = max(float(v.abs().max()) for v in gen_g.values())
    assert sorted(one_g) == sorted(gen_g)
    for k in gen_g:
        assert float((one_g[k] - gen_g[k]).abs().max()) <= TWO_FLOORS * scale, k
    # eval(): the Dropout-free forward, bit for bit (a twin that never had Dropout)
    twin = copy.deepcopy(m)
    twin.dropout = 0.0
    with torch.no_grad():
        want = twin.train().forward(data)
        assert torch.equal(m.eval().forward(data), want)
    assert spy.calls == [] and not torch.equal(want, one)


@pytest.mark.parametrize("gate", ["node_ids", "readout", "449 nodes", "x.requires_grad"])
def test_the_gates_stay_shut_under_dropout(gate, spy, monkeypatch):
    """What the one-launch routes do not cover takes the general Dropout route as before: no ``_drop`` entry point is called,
    ``functional.feature_mlps_dropout`` is."""
    from gnan_amd import functional, models, replay, small_graph
    monkeypatch.setattr(replay, "REPLAY_FORWARD", False)
    taken = []
    real = functional.feature_mlps_dropout

    def counted(*a, **k):
        taken.append(1)
        return real(*a, **k)
    monkeypatch.setattr(functional, "feature_mlps_dropout", counted)
    data, kw = _graph_cached(30), {}
    if gate == "node_ids":
        m, kw = _model("models_gnan"), {"node_ids": [0, 3, 29]}
    elif gate == "readout":
        torch.manual_seed(0)
        m = models.TensorGNAN(15, 1, 3, hidden_channels=32, dropout=P, is_graph_task=True, readout_n_layers=1, device=DEV).to(DEV).train()
    elif gate == "449 nodes":
        m, data = _model("models_tensor"), _graph_cached(449)
    else:
        m = _model("models_tensor")
        data = Bag(**{**data.__dict__, "x": data.x.clone().requires_grad_(True)})
    out, grads = _step(m, data, **kw)
    assert spy.calls == [] and taken
    assert torch.isfinite(out).all() and grads
    # one seed draw per forward whichever way the gates sent it: with the switch off the same manual_seed gives the same bits
    with monkeypatch.context() as mp:
        mp.setattr(small_graph, "SMALL_GRAPH_DROPOUT", False)
        off, _ = _step(m, data, **kw)
    assert torch.equal(out, off)
    # ... and the same model on a plain covered call does take the route (the spy sees it)
    if gate in ("node_ids", "449 nodes", "x.requires_grad"):
        _step(m, _graph_cached(30))
        assert spy.calls == ["gnan_small_graph_fwd_drop", "gnan_small_graph_bwd_drop"]
