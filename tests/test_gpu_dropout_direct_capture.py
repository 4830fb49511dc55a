"""The Dropout seed cell of the DIRECT kernels (gnan_fmlp_fwd_dev, gnan_fmlp_bwd_dev, gnan_fmlp_bwd_mfma_dev, gnan_fmlp_mc_fwd_dev,
gnan_fmlp_mc_bwd_dev) and the captured steps they allow behind ``functional.CAPTURE_DROPOUT_DIRECT``: a cell gives the bits of the
by-value seed in every kernel family, one case per family against the oracle's float64 chain fed with gnan_dropout_mask's masks
(the project's rule), a captured full-batch node-task step, the modules' own replay on a 449-node dense graph and on a CSR graph,
and the gates that stay shut.  The kernel routes are forced with ``_fmlp_launch(algo=/mc=)`` / ``_fmlp_backward_launch(mfma=/mc=)``."""
import copy
import functools
import itertools
import warnings

import pytest
import torch

from helpers import TWO_FLOORS, assert_grads_rule, assert_rule
from test_gpu_dropout_mc import NAMES, _inputs, _masks, _mlp_state, _oracle, _stack, _want_l3
from test_gpu_graphed import DEV, _need_gpu, _node_task
from test_gpu_small_graph_dropout import _graph_cached

pytestmark = pytest.mark.gpu
P, SEED = 0.6, 0xC2B2AE3D27D4EB4F & ((1 << 63) - 1)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    _need_gpu()


def _cell(seed):
    from gnan_amd.small_graph import seed_cell, seed_cell_set
    c = seed_cell(DEV)
    seed_cell_set(c, seed)
    return c


def _random_stack(F, L, H, C, seed):
    """Stacked float32 weights of F shape functions (biases present), L in {2, 3, 4}."""
    from gnan_amd.functional import StackedMLP
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: (torch.randn(*s, generator=g) * 0.5).to(DEV)          # noqa: E731
    mid = L - 2
    return StackedMLP(r(F, H), r(F, H), r(mid, F, H, H) * 0.3 if mid else None, r(mid, F, H) if mid else None, r(F, C, H), r(F, C),
                      L, H, C, F)


FAMILIES = {   # name -> (forward keywords of _fmlp_launch, backward keywords of _fmlp_backward_launch or None)
    "lane": (lambda lib: dict(algo=lib.FMLP_LANE), dict()),
    "mfma": (lambda lib: dict(algo=lib.FMLP_MFMA), dict(mfma=True)),
    "mc": (lambda lib: dict(mc=True), dict(mc=True)),
}


def _both(family, x, st, gup, sum_features, dropout, backward=True):
    """Output and (L <= 3) parameter gradients of one kernel family under ``dropout = (p, seed or cell)`` or None."""
    from gnan_amd import _lib
    from gnan_amd import functional as Fn
    fwd_kw, bwd_kw = FAMILIES[family]
    y = Fn._fmlp_launch(x, st, sum_features, dropout=dropout, **fwd_kw(_lib))
    if not backward:
        return y, []
    g = Fn._fmlp_backward_launch(x, list(st[:6]), gup, sum_features, st.L, st.H, st.C, st.F, dropout=dropout, **bwd_kw)
    return y, [t for t in g if t is not None]


def _same(a, b):
    return torch.equal(a[0], b[0]) and len(a[1]) == len(b[1]) and all(torch.equal(s, t) for s, t in zip(a[1], b[1]))


def _cell_is_the_seed(family, n, F, L, H, C, sum_features, backward=True):
    st = _random_stack(F, L, H, C, seed=n + 7 * L + H + C)
    x, gup = (t.to(DEV) for t in _inputs(n, F, C, sum_features, seed=n))
    run = lambda d: _both(family, x, st, gup, sum_features, d, backward)   # noqa: E731
    what = (family, n, F, L, H, C, sum_features)
    cell = _cell(SEED)
    want, got = run((P, SEED)), run((P, cell))
    assert _same(got, want), what
    from gnan_amd.small_graph import seed_cell_set
    seed_cell_set(cell, SEED + 1)                                          # nothing but the cell changes
    other, nxt = run((P, cell)), run((P, SEED + 1))
    assert _same(other, nxt), what
    assert n * F * H < 64 or not torch.equal(other[0], want[0]), what
    plain = run(None)
    assert _same(run((0.0, cell)), plain) and _same(run((0.0, 0)), plain), what     # p == 0: the plain bits, the cell is not read
    assert not torch.equal(plain[0], want[0]) or n * F * H < 64


# ---- a cell gives the bits of the by-value seed -----------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [2, 3])
@pytest.mark.parametrize("n", [1, 64, 65])
def test_lane_forward_and_fmlp_bwd(n, L):
    """fmlp_lane_kernel and fmlp_bwd_kernel: one lane, a full wave, a second wave."""
    for H, C, sum_features in itertools.product((8, 64), (1, 8), (False, True)):
        _cell_is_the_seed("lane", n, 3, L, H, C, sum_features)


@pytest.mark.parametrize("n", [31, 32, 33, 129])
def test_matrix_core_forward_and_fmlp_bwd_mfma(n):
    """The DROP instances of fmlp_mfma_kernel and fmlp_bwd_mfma_kernel: 32-node tiles, four waves (129: a second round); the
    forward at L = 4 as well (two mid layers; no backward kernel there)."""
    for H, C, sum_features in itertools.product((32, 64), (1, 8), (False, True)):
        _cell_is_the_seed("mfma", n, 3, 3, H, C, sum_features)
        _cell_is_the_seed("mfma", n, 3, 4, H, C, sum_features, backward=False)


@pytest.mark.parametrize("C", [9, 32, 33, 40, 64])
def test_many_channel_forward_and_backward(C):
    """fmlp_mc_fwd_kernel / fmlp_mc_bwd_kernel: one and two channel tiles, H = 32 / 64 (two tiles and one tile per wave)."""
    for H, n, sum_features in itertools.product((32, 64), (33, 65), (False, True)):
        _cell_is_the_seed("mc", n, 3, 3, H, C, sum_features)
    _cell_is_the_seed("mc", 33, 3, 4, 64, C, True, backward=False)


def test_the_record_keeps_no_seed_beside_the_cell():
    """The Python launchers leave the record's by-value seed at 0 under a cell (anything else is refused on the host), and a cell
    that is no one-element int64 / uint64 device tensor is refused."""
    from gnan_amd import functional as Fn
    st = _random_stack(3, 3, 8, 1, seed=1)
    x = torch.rand(5, 3, device=DEV)
    for bad in (torch.zeros(2, dtype=torch.int64, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV),
                torch.zeros(1, dtype=torch.int64)):
        with pytest.raises(ValueError, match="seed cell"):
            Fn._fmlp_launch(x, st, True, dropout=(P, bad))


# ---- one case per family against the float64 oracle chain ---------------------------------------------------------------------------
@pytest.mark.parametrize("family,n,F,H,C,sum_features", [("lane", 65, 3, 33, 3, True), ("mfma", 129, 3, 64, 8, False),
                                                         ("mc", 65, 3, 64, 40, True)])
def test_a_cell_against_the_oracle_chain(family, n, F, H, C, sum_features):
    """Forward and gradients under a CELL == the oracle's chain with the masks gnan_dropout_mask writes for the seed it holds."""
    L = 3
    sd = _mlp_state(F, L, H, C, True, seed=F + H + C)
    st = _stack(sd, F, L, H, C, True)
    x, gup = _inputs(n, F, C, sum_features)
    y, grads = _both(family, x.to(DEV), st, gup.to(DEV), sum_features, (P, _cell(SEED)))
    ref, want = _oracle(x, sd, _masks(n, F, L, H, seed=SEED), P, sum_features, gup)
    assert_rule(y, ref, None, (family, "forward"))
    want = _want_l3(want, True)
    assert_grads_rule({k: g.reshape(want[k].shape) for k, g in zip(NAMES, grads)}, want, None, (family, "gradients"))


# ---- captured steps ------------------------------------------------------------------------------------------------------------------
class _Spy:
    """``_lib.lib()`` with the calls of the direct kernels' entry points (by value and ``_dev``) and of the seed store noted."""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        fn = getattr(self.real, name)
        if not ((name.startswith("gnan_fmlp") and "workspace" not in name) or name == "gnan_dropout_seed_set"):
            return fn

        def counted(*args):
            self.calls.append(name)
            return fn(*args)
        return counted

    def dev(self):
        return [c for c in self.calls if c.endswith("_dev")]

    def stores(self):
        return self.calls.count("gnan_dropout_seed_set")


@pytest.fixture
def spy(monkeypatch):
    from gnan_amd import _lib
    s = _Spy(_lib.lib())
    monkeypatch.setattr(_lib, "lib", lambda: s)
    return s


@pytest.fixture
def direct_on(monkeypatch):
    from gnan_amd import functional as Fn
    monkeypatch.setattr(Fn, "CAPTURE_DROPOUT_DIRECT", True)


@functools.lru_cache(maxsize=None)
def _task():
    _need_gpu()
    return _node_task(600, 9, 4, False)                  # (a CSR graph: what a full-batch node task trains on)


def _node_model(hidden=16, n_layers=3, C=4, F=9, **kw):
    from gnan_amd import models
    torch.manual_seed(0)
    m = models.TensorGNAN(F, C, n_layers, hidden_channels=hidden, dropout=P, device=DEV, **kw)
    with torch.no_grad():
        for _, p in m.named_parameters():
            p.copy_(torch.randn(p.shape) * 0.3)
    return m.to(DEV).train()


LOSS = torch.nn.CrossEntropyLoss()                   # (ONE object: the harness keys its captured steps by the loss, too)


def _epochs(m, opt, data, epochs, seed):
    from gnan_amd import harness
    torch.manual_seed(seed)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                # (the one-time note of _check_dropout)
        return [harness.train_epoch(m, [data], LOSS, opt, DEV, classify=True, is_graph_task=False)[0] for _ in range(epochs)]


def _node_steps(m):
    from gnan_amd import harness
    return [r.value["step"] for r in harness._steps_of(m).node.entries.values() if r.value["step"] is not None]


def test_a_captured_node_task_step(spy, direct_on, monkeypatch):
    """harness.train_epoch on a full-batch node task under Dropout: replays from its third epoch, one seed store per replay, fresh
    masks per replay, the same manual_seed the same bits, and an eager twin's losses and parameters (1e-5, the slot tests' bound)."""
    from gnan_amd import harness, replay
    data = _task()
    m = _node_model()
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    twin = copy.deepcopy(m)
    twin_opt = torch.optim.Adam(twin.parameters(), lr=1e-3)
    got = _epochs(m, opt, data, 8, seed=3)
    steps = _node_steps(m)
    assert len(steps) == 1 and steps[0].cell is not None and steps[0].graph.replays == 6, "not replayed from the third epoch on"
    assert spy.stores() == 6                                                 # one seed store (one draw) per replay
    assert {"gnan_fmlp_fwd_dev", "gnan_fmlp_bwd_dev"} <= set(spy.dev())     # recorded once, at the capture
    with monkeypatch.context() as mp:
        mp.setattr(harness, "GRAPHED_STEPS", False)
        mp.setattr(replay, "REPLAY_FORWARD", False)
        del spy.calls[:]
        want = _epochs(twin, twin_opt, data, 8, seed=3)
        assert spy.dev() == [] and spy.stores() == 0
    for e, (a, b) in enumerate(zip(got, want)):
        print(f"epoch {e}: captured {a:.9g} eager {b:.9g}")
        assert abs(a - b) <= 1e-5 * max(1.0, abs(b)), (e, a, b)
    top = max(float(p.abs().max()) for p in twin.parameters())
    for (k, p), q in zip(m.named_parameters(), twin.parameters()):
        assert float((p - q).abs().max()) <= 1e-5 * top, k
    # two consecutive replays differ (the masks are not frozen); the same manual_seed twice gives equal bits.  The learning rate
    # is 0 from here on: the parameters stand still, so nothing but the masks can move the loss
    for group in opt.param_groups:
        group["lr"] = 0.0
    one, two, other = _epochs(m, opt, data, 2, seed=11), _epochs(m, opt, data, 2, seed=11), _epochs(m, opt, data, 2, seed=12)
    assert one == two and one[0] != one[1] and other[0] != one[0]
    assert _node_steps(m) == steps and steps[0].graph.replays == 12 and spy.stores() == 6
    # eval(): the Dropout-free bits
    plain = copy.deepcopy(m)
    plain.dropout = 0.0
    m.eval(), plain.eval()
    with torch.no_grad(), monkeypatch.context() as mp:
        mp.setattr(replay, "REPLAY_FORWARD", False)
        assert torch.equal(m.forward(data), plain.forward(data))
    harness.release_steps(m)


def _loop(m, data, steps=8, seed=21):
    torch.manual_seed(seed)
    outs = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for _ in range(steps):
            m.zero_grad(set_to_none=True)
            out = m.forward(data)
            out.pow(2).sum().backward()
            outs.append((out.detach().clone(), {k: p.grad.detach().clone() for k, p in m.named_parameters()}))
    return outs


def _plans(m):
    cache = m.__dict__.get("_replays")
    return [e.value["plan"] for e in cache.entries.values() if e.value["plan"] is not None] if cache is not None else []


def _graph_model():
    from test_gpu_small_graph_dropout import _model
    return _model("models_tensor")


@pytest.mark.parametrize("graph", ["dense449", "csr"])
def test_the_modules_own_replay_is_the_eager_loops_twin(graph, spy, direct_on, monkeypatch):
    from gnan_amd import replay
    data, make = (_graph_cached(449), _graph_model) if graph == "dense449" else (_task(), _node_model)
    on_model, off_model = make(), make()
    on = _loop(on_model, data)
    plans = _plans(on_model)
    assert len(plans) == 1 and plans[0].cell is not None and plans[0].gen >= 3
    assert spy.stores() == plans[0].gen and spy.dev()
    del spy.calls[:]
    with monkeypatch.context() as mp:
        mp.setattr(replay, "REPLAY_FORWARD", False)
        off = _loop(off_model, data)
    assert spy.dev() == [] and spy.stores() == 0
    for s, ((a, a_g), (b, b_g)) in enumerate(zip(on, off)):
        assert float((a - b).abs().max()) <= TWO_FLOORS * float(b.abs().max()), s
        scale = max(float(v.abs().max()) for v in b_g.values())
        for k in b_g:
            assert float((a_g[k] - b_g[k]).abs().max()) <= TWO_FLOORS * scale, (s, k)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        one, two = on_model.forward(data).detach().clone(), on_model.forward(data).detach().clone()
        assert not torch.equal(one, two)
    replay.release(on_model)


# ---- gates -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gate", ["x.requires_grad", "L = 4", "H = 128", "C = 40 at small n", "readout", "batched", "node_ids"])
def test_the_gates_stay_shut_with_the_switch_on(gate, spy, monkeypatch):
    """Out of scope: nothing is captured under Dropout, no ``_dev`` call, no seed store, and the bits of the switch-off run."""
    from gnan_amd import batched, functional as Fn, harness, models
    data, kw, harnessed = _task(), {}, gate in ("L = 4", "H = 128", "C = 40 at small n")
    make = _node_model
    if gate == "x.requires_grad":
        data = copy.copy(data)
        data.x = data.x.clone().requires_grad_(True)
    elif gate == "L = 4":
        make = lambda: _node_model(n_layers=4)                                     # noqa: E731
    elif gate == "H = 128":
        make = lambda: _node_model(hidden=128)                                     # noqa: E731
    elif gate == "C = 40 at small n":
        make = lambda: _node_model(C=40)                                           # noqa: E731
        data = copy.copy(data)
        data.y = data.y * 9
    elif gate == "readout":
        data = _graph_cached(449)

        def make():
            torch.manual_seed(0)
            return models.TensorGNAN(15, 1, 3, hidden_channels=32, dropout=P, is_graph_task=True, readout_n_layers=1,
                                     device=DEV).to(DEV).train()
    elif gate == "node_ids":
        from test_gpu_small_graph_dropout import _model
        make, kw, data = (lambda: _model("models_gnan")), {"node_ids": [0, 3, 129]}, _graph_cached(449)
    elif gate == "batched":
        from test_gpu_dropout_capture import _small_graphs
        g = _small_graphs()
        blocks = batched.HopBlocks.from_blocks([torch.round(1.0 / d.node_distances.clamp_min(1e-9) - 1.0).masked_fill(
            d.node_distances <= 0, -1.0) for d in g[:2]])
        bv = torch.cat([torch.full((d.x.shape[0],), i, dtype=torch.long) for i, d in enumerate(g[:2])]).to(DEV)
        data = (torch.cat([d.x for d in g[:2]]), blocks, bv)

        def make():
            torch.manual_seed(0)
            return batched.TensorGNAN(15, 1, 2, hidden_channels=16, dropout=P, device=DEV).to(DEV).train()

    def run(m):
        torch.manual_seed(3)
        if harnessed:
            opt = torch.optim.Adam(m.parameters(), lr=1e-3)
            out = _epochs(m, opt, data, 5, seed=3)
            assert not _node_steps(m)
            return out
        outs = []
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for _ in range(5):
                m.zero_grad(set_to_none=True)
                out = m.forward(*data) if gate == "batched" else m.forward(data, **kw)
                out.pow(2).sum().backward()
                outs.append(out.detach().clone())
        assert not _plans(m)
        return outs
    with monkeypatch.context() as mp:
        mp.setattr(Fn, "CAPTURE_DROPOUT_DIRECT", True)
        got = run(make())
    assert spy.dev() == [] and spy.stores() == 0
    want = run(make())
    if gate == "batched":
        return                                           # (its rho draws torch's own masks and sums with atomics: no bits to compare)
    for a, b in zip(got, want):
        assert torch.equal(a, b) if torch.is_tensor(a) else abs(a - b) <= 1e-6 * max(1.0, abs(b))


def test_a_cell_handed_to_a_restatement_backward_raises():
    """L = 4, H = 128, C = 40 at small n, x.grad: the batched restatement would run — its masks are by value, so a cell is refused."""
    from gnan_amd import functional as Fn
    for L, H, C, x_grad in ((4, 16, 2, False), (3, 128, 2, False), (3, 32, 40, False), (3, 16, 2, True)):
        st = _random_stack(3, L, H, C, seed=5)
        st = st._replace(**{k: getattr(st, k).requires_grad_(True) for k in NAMES if getattr(st, k) is not None})
        x = torch.rand(20, 3, device=DEV).requires_grad_(x_grad)
        out = Fn.feature_mlps_dropout(x, st, True, P, seed=_cell(SEED))
        want = Fn.feature_mlps_dropout(x.detach(), st, True, P, seed=SEED)
        assert torch.equal(out, want)                      # (the forward kernels take the cell)
        with pytest.raises(RuntimeError, match="seed in a device cell"):
            out.sum().backward()


@pytest.mark.parametrize("case", ["node task", "dense449", "csr"])
def test_with_the_switch_off_nothing_new_is_reached(case, spy):
    from gnan_amd import functional as Fn
    assert Fn.CAPTURE_DROPOUT_DIRECT is False
    if case == "node task":
        m = _node_model()
        _epochs(m, torch.optim.Adam(m.parameters(), lr=1e-3), _task(), 5, seed=3)
        assert not _node_steps(m)
    else:
        m = _graph_model() if case == "dense449" else _node_model()
        _loop(m, _graph_cached(449) if case == "dense449" else _task(), steps=5)
        assert not _plans(m)
    assert spy.dev() == [] and spy.stores() == 0
    assert [c for c in spy.calls if c in ("gnan_fmlp_fwd", "gnan_fmlp_bwd")]      # the by-value entry points, as before
