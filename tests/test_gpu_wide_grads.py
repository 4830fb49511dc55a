"""``gnan_fpwl_param_grads`` for three-layer nets of 65-128 hidden units (csrc/fpwl_grad.hip: ``fpwl_grad3_kernel<128, 1, CQ>``):
every element of all six gradient tensors against the exact reference of tests/grads_ref.py, inside
``u32 |t| + (1 + u32) gamma64_k Mag + 2^-149`` with ``k = k_piece(3, H, w, nl, NG = 1)`` (the count and the instances:
tests/wide_grads_cases.py), exact zeros where the bound is zero, the same bits twice, an integer family bit for bit; then the
real chain (tables of ``gnan_pwl_build``, raw moments of ``_fpwl_moments``), the modules end to end against autograd through the
float64 oracle with the probe-point route made to raise, a captured training step, and the switch."""
import math

import numpy as np
import pytest
import torch

import grads_ref as G
import wide_grads_cases as W
from helpers import TWO_FLOORS, assert_rule, grad_rule, module_grads, oracle_grads, tolerance_ok
from test_gpu_deep_tables import Bag, _oracle_chain, _redraw

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")


@pytest.fixture(autouse=True)
def _switch_on(monkeypatch):
    from gnan_amd import functional
    monkeypatch.setattr(functional, "WIDE_TABLE_GRADS", True)


def _to(p, dev):
    return type(p)(*[None if q is None else q.to(dev) for q in p[:6]], *p[6:])


def _launch(case):
    """Two launches through ``functional._fpwl_param_grads_launch`` with the case's moments handed in."""
    from gnan_amd import functional, pwl
    p = _to(case.p, DEV)
    T = int(case.off[-1])
    t = pwl.PwlTables(torch.from_numpy(case.off).to(DEV), torch.from_numpy(np.concatenate(case.anchors)).to(DEV),
                      torch.zeros(T, p.C, device=DEV), torch.zeros(T, p.C, device=DEV), int(case.max_pieces), 1,
                      int(case.max_pieces))
    if case.exps is None:
        moments = torch.from_numpy(np.ascontiguousarray(case.M, dtype=np.float32)).to(DEV)
    else:
        scales = torch.tensor([2.0 ** case.exps[0], 2.0 ** case.exps[1]], dtype=torch.float64, device=DEV)
        moments = (torch.from_numpy(np.ascontiguousarray(case.M, dtype=np.int64)).to(DEV), scales)
    runs = []
    for _ in range(2):
        got = functional._fpwl_param_grads_launch(list(p[:6]), t, moments, p.L, p.H, p.C, p.F)
        torch.cuda.synchronize()
        runs.append([None if g is None else g.cpu() for g in got])
    return runs


def _hold(case):
    first, second = _launch(case)
    for a, b in zip(first, second):
        assert (a is None and b is None) or torch.equal(a, b), "the same bits twice"
    ref = W.reference(case)
    assert sum(ex.undecided for ex in ref) == 0
    got = G.split(case, first)
    ratio, where, zero_bounds = W.hold(case, got)
    print(f"WIDE-GRAD-ELEMENTS {case.name} NG={W.WIDE_NG} nl={[ex.nl for ex in ref]} ratio={ratio:.4f} at={where} "
          f"zero_bounds={zero_bounds}")
    assert ratio <= 1.0, (case.name, ratio, where)
    return got


@pytest.mark.parametrize("name", list(W.RANDOM))
def test_every_element_is_inside_its_bound(name):
    case = W.case(name)
    got = _hold(case)
    if name == "H128-C1-one-feature-empty":
        assert W.reference(case)[1].nl == 0
        assert all(not np.asarray(a).any() for a in got[1].values()), "a feature with no live piece returns exact zeros"


def _kernel_tables(p):
    from gnan_amd import pwl
    pd = _to(p, DEV)
    assert pwl.hip_build_applies(pd)
    return pwl.build_tables(pd)


@pytest.mark.parametrize("name", ["H65-C1", "H128-C40"])
def test_every_element_on_the_kernel_builders_tables(name):
    case = W.case(name, tables=_kernel_tables)
    _hold(case._replace(name=name + "@gnan_pwl_build"))


def test_the_largest_lds_corner_runs_and_is_inside_the_bound():
    """H = 128, C = 64 and a tables record of ``max_pieces = 8192``: 139 296 bytes of dynamic LDS, the most the entry point asks
    for."""
    case = W.case(W.LDS_CORNER)
    assert case.max_pieces == 8192 and case.p.H == 128 and case.p.C == 64
    _hold(case)


def test_the_integer_family_returns_the_truths_own_bits():
    case = W.case(W.INTEGER)
    ok, name = W.truth_bits(case, W.emulate(case))           # the kernel's order is exact on it ...
    assert ok, name
    ok, name = W.truth_bits(case, _hold(case))               # ... so the kernel is
    assert ok, name


def test_real_chain_tables_and_raw_moments():
    """Tables from ``gnan_pwl_build`` at (L, H, C) = (3, 128, 2), raw int64 moments from ``_fpwl_moments(raw=True)`` (n = 2000,
    F = 3): those very integers go to the kernel and to the reference."""
    import tables_ref as R
    from gnan_amd import functional, pwl
    L, H, C, F, n, seed = 3, 128, 2, 3, 2000, 73
    p = R.random_state(F, L, H, C, True, seed)
    pd = _to(p, DEV)
    assert pwl.hip_build_applies(pd)
    t = pwl.build_tables(pd)
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(n, F, generator=g) * 4 - 2).to(DEV)
    grad = torch.randn(n, F * C, generator=g).to(DEV)
    Mi, scales = functional._fpwl_moments(x, t, grad, False, raw=True)
    exps = tuple(int(round(math.log2(float(s)))) for s in scales.cpu())
    assert all(2.0 ** e == float(s) for e, s in zip(exps, scales.cpu())), "power-of-two scales"
    off = t.off.cpu().tolist()
    anchor = t.anchor.cpu().numpy()
    anchors = [anchor[off[k]:off[k + 1]].copy() for k in range(F)]
    case = G.Case("real-chain-L3-H128", p, anchors, Mi.cpu().numpy()[:off[F]], exps, int(t.max_pieces), G.features_of(p, kinks=False))
    _hold(case)


# ---- end to end ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def graph600():
    """600 nodes, one hop (self, neighbour, rest), 5 features; unique directed edges without self loops."""
    from gnan_amd import synthetic as syn
    rng = np.random.default_rng(0)
    n, F = 600, 5
    e = rng.integers(0, n, (2, 2400))
    e = np.unique(e[:, e[0] != e[1]], axis=1)
    src, dst = torch.from_numpy(e[0]).to(DEV), torch.from_numpy(e[1]).to(DEV)
    g = syn.hop1_csr(src, dst, n)
    x = torch.rand(n, F, generator=torch.Generator().manual_seed(1)) * 4 - 2
    csr = (g.rowptr.cpu().long().numpy(), g.col.cpu().numpy(), g.code.cpu().numpy(), g.cnt.cpu().long().numpy())
    return g, x, csr


def _module(kind, F, C, hidden, normalize):
    from gnan_amd import GNAN as standalone
    from gnan_amd import models
    torch.manual_seed(0)
    if kind == "tensor":
        mod = models.TensorGNAN(F, C, 3, hidden_channels=hidden, normalize_rho=normalize, device=DEV)
    elif kind == "gnan":
        mod = models.GNAN(F, C, num_layers=3, hidden_channels=hidden, normalize_rho=normalize, device=DEV)
    else:
        mod = standalone.TensorGNAN(F, C, 3, hidden_channels=hidden, normalize_rho=normalize, device=DEV)
    _redraw(mod, 7)
    return mod


@pytest.mark.parametrize("hidden", [96, 128])
@pytest.mark.parametrize("kind,normalize", [("tensor", True), ("tensor", False), ("gnan", True), ("standalone", True)])
def test_wide_models_end_to_end(kind, normalize, hidden, graph600, monkeypatch):
    """n_layers = 3 with 96 / 128 hidden units through the modules on the table path: forward and every parameter gradient
    against autograd through the float64 oracle, with the probe-point route made to raise.  ``standalone`` (the stand-alone file's
    TensorGNAN, pre-rho normalisation) sends a wide rho through ``_rho_param_grads``.  (``_fmlp_eager`` stays: rho's table on the
    hop values is a direct evaluation.)"""
    from gnan_amd import _lib, functional, pwl
    g, x, csr = graph600
    n, F = x.shape
    C = 3
    monkeypatch.setattr(functional, "FMLP_ALGO", _lib.FMLP_PWL)
    mod = _module(kind, F, C, hidden, normalize)
    sd = {k: v.detach().cpu().clone() for k, v in mod.state_dict().items()}
    mod = mod.to(DEV).eval()
    target = torch.randn(n, C, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    data = Bag(x=x.to(DEV), edge_index=None, gnan_graph=g)

    def refuse(*a, **k):
        raise AssertionError("a wide three-layer step reached the probe-point route")
    monkeypatch.setattr(pwl, "parameter_grads_from_moments", refuse)
    launches = []
    launch = functional._fpwl_param_grads_launch
    monkeypatch.setattr(functional, "_fpwl_param_grads_launch", lambda *a, **k: (launches.append(a[3:6]), launch(*a, **k))[1])
    y = mod.forward(data)
    ((y - target.to(DEV).float()) ** 2).mean().backward()
    torch.cuda.synchronize()
    print(f"WIDE-MODULES {kind} hidden={hidden} normalize={normalize} gnan_fpwl_param_grads (L, H, C)={launches}")
    assert (3, hidden, C) in launches, launches

    chain = _oracle_chain(kind, x, csr, normalize)
    with torch.no_grad():
        truth = chain({k: v.double() for k, v in sd.items()}, torch.float64)
    assert_rule(y.detach().cpu(), truth, lambda: chain(sd, torch.float32), (kind, hidden, normalize))
    g64 = oracle_grads(lambda p: ((chain(p, torch.float64) - target) ** 2).mean(), sd, torch.float64)
    g32 = lambda: oracle_grads(lambda p: ((chain(p, torch.float32) - target.float()) ** 2).mean(), sd, torch.float32)   # noqa: E731
    ok, e_build, e_ref, where = grad_rule(module_grads(mod), g64, g32)
    assert ok, f"{where}: build {e_build:.3e} vs fp32 oracle {e_ref:.3e}"


def test_wide_training_step_is_captured_and_replayed(graph600, monkeypatch):
    """harness.train_epoch at hidden = 96: after the eager warm-up epochs the whole step is one replayed hipGraph, and the loss
    trajectory is the eager loop's."""
    from gnan_amd import _lib, functional, harness, models
    g, x, _ = graph600
    n, F = x.shape
    C = 3
    monkeypatch.setattr(functional, "FMLP_ALGO", _lib.FMLP_PWL)
    rng = np.random.default_rng(3)
    data = Bag(x=x.to(DEV), edge_index=None, gnan_graph=g, y=torch.from_numpy(rng.integers(0, C, n)).to(DEV),
               train_mask=torch.from_numpy(rng.random(n) < 0.6).to(DEV))
    losses = {}
    for graphed in (False, True):
        monkeypatch.setattr(harness, "GRAPHED_STEPS", graphed)
        torch.manual_seed(0)
        model = models.TensorGNAN(F, C, 3, hidden_channels=96, device=DEV)
        _redraw(model, 11)                          # (seeded: the same weights in both runs)
        model = model.to(DEV).train()
        opt = torch.optim.Adam(model.parameters(), lr=0.01)
        loss_fn = torch.nn.CrossEntropyLoss()
        losses[graphed] = [harness.train_epoch(model, [data], loss_fn, opt, DEV, classify=True, compute_auc=False,
                                               is_graph_task=False)[0] for _ in range(6)]
        if graphed:
            store = harness._steps_of(model)
            replays = sum(r.value["step"].graph.replays for r in store.node.entries.values() if r.value["step"] is not None)
            assert replays >= 3, "the captured step was never replayed"
            harness.release_steps(model)
    ok, e, _ = tolerance_ok(np.array(losses[True]), np.array(losses[False]), np.array(losses[False]), floor=TWO_FLOORS)   # two routes
    assert ok, (e, losses)


def test_switch_off_takes_the_probe_point_route(graph600, monkeypatch):
    from gnan_amd import _lib, functional, pwl
    g, x, _ = graph600
    n, F = x.shape
    C = 3
    monkeypatch.setattr(functional, "FMLP_ALGO", _lib.FMLP_PWL)
    calls = []
    probe = pwl.parameter_grads_from_moments
    monkeypatch.setattr(pwl, "parameter_grads_from_moments", lambda *a, **k: (calls.append(1), probe(*a, **k))[1])
    data = Bag(x=x.to(DEV), edge_index=None, gnan_graph=g)
    for on, want in ((True, 0), (False, 1)):
        monkeypatch.setattr(functional, "WIDE_TABLE_GRADS", on)
        mod = _module("tensor", F, C, 96, True).to(DEV).eval()
        del calls[:]
        mod.forward(data).pow(2).mean().backward()
        torch.cuda.synchronize()
        assert (len(calls) >= 1) == bool(want), (on, len(calls))
        assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in mod.parameters())
