"""``x.grad`` through the table path, end to end on the MI355X: ``feature_mlps`` in both modes and the modules (``models.TensorGNAN``
in the sum-first and the ``"reference"`` order, the stand-alone file's ``TensorGNAN``) with ``x`` a leaf and with ``x = Linear(raw)``,
on a 300-node random graph under ``FMLP_ALGO = FMLP_PWL``.  ``x.grad`` (or ``raw.grad`` and the encoder's gradients) and every
parameter gradient follow the project's rule against autograd through the float64 oracle (helpers.rule / grad_rule; the float32
oracle is evaluated only where the floor does not decide) — with the batched-GEMM restatement ``_fmlp_eager`` made to raise, so the
backward pass is the tables'.  The one-hot zero-bias goldens 400-405 are run the same way.  Parameter gradients do not depend on
whether ``x`` needs a gradient, bit for bit, and without one the route is the hand-composed moments route, bit for bit."""
import numpy as np
import pytest
import torch

from conftest import Golden
from helpers import assert_grads_rule, assert_rule, inputs_from, params_from
from oracle import gnan_oracle as O
from test_gpu_deep_tables import Bag, _mlp_state, _oracle_chain, _redraw, _stack

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(7, 1, 3), (16, 3, 3), (7, 3, 4), (16, 1, 4)]          # (F, C, L): F = 7, 16; C = 1, 3; L = 3, 4
H = 16
R_RAW = 5


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")


@pytest.fixture(autouse=True)
def _tables_only(monkeypatch):
    """The table path, and no way back to the restatement: a backward pass that reaches ``_fmlp_eager`` fails the test."""
    from gnan_amd import _lib, functional

    def refuse(*a, **k):
        raise AssertionError("the backward pass reached the batched-GEMM restatement")
    monkeypatch.setattr(functional, "FMLP_ALGO", _lib.FMLP_PWL)
    monkeypatch.setattr(functional, "_fmlp_eager", refuse)


_GRAPHS = {}


def graph300():
    """300 nodes, one hop (self, neighbour, rest); unique directed edges without self loops."""
    if not _GRAPHS:
        from gnan_amd import synthetic as syn
        rng = np.random.default_rng(0)
        n = 300
        e = rng.integers(0, n, (2, 1500))
        e = np.unique(e[:, e[0] != e[1]], axis=1)
        g = syn.hop1_csr(torch.from_numpy(e[0]).to(DEV), torch.from_numpy(e[1]).to(DEV), n)
        _GRAPHS["g"] = (g, (g.rowptr.cpu().long().numpy(), g.col.cpu().numpy(), g.code.cpu().numpy(), g.cnt.cpu().long().numpy()))
    return _GRAPHS["g"]


def draw_inputs(F, seed, kinks=False):
    gen = torch.Generator().manual_seed(seed)
    x = torch.rand(300, F, generator=gen) * 4 - 2
    if kinks:
        x = torch.randint(0, 2, (300, F), generator=gen).float()
    raw = torch.rand(300, R_RAW, generator=gen) * 2 - 1
    enc = {"weight": torch.randn(F, R_RAW, generator=gen) * 0.7, "bias": torch.randn(F, generator=gen) * 0.3}
    return x, raw, enc


def oracle_input_side(mode, x, raw, enc, dtype):
    """Leaves and the feature matrix of the oracle's graph: ``(x, {name: leaf})``."""
    if mode == "leaf":
        xl = x.to(dtype).clone().requires_grad_(True)
        return xl, {"x": xl}
    leaves = {"raw": raw.to(dtype).clone().requires_grad_(True), "enc.weight": enc["weight"].to(dtype).clone().requires_grad_(True),
              "enc.bias": enc["bias"].to(dtype).clone().requires_grad_(True)}
    return leaves["raw"] @ leaves["enc.weight"].t() + leaves["enc.bias"], leaves


def device_input_side(mode, x, raw, enc):
    if mode == "leaf":
        xl = x.to(DEV).requires_grad_(True)
        return xl, {"x": xl}
    lin = torch.nn.Linear(R_RAW, x.shape[1]).to(DEV)
    with torch.no_grad():
        lin.weight.copy_(enc["weight"])
        lin.bias.copy_(enc["bias"])
    rl = raw.to(DEV).requires_grad_(True)
    return lin(rl), {"raw": rl, "enc.weight": lin.weight, "enc.bias": lin.bias}


def oracle_all_grads(loss_of, sd, mode, x, raw, enc, dtype):
    """Gradients of ``loss_of(params, x)`` w.r.t. the parameters and the input side, in ``dtype``: ``{name: grad}``."""
    p = {k: v.to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    xo, leaves = oracle_input_side(mode, x, raw, enc, dtype)
    loss_of(p, xo, dtype).backward()
    out = {k: v.grad for k, v in p.items()}
    out.update({"in." + k: v.grad for k, v in leaves.items()})
    return out


def stacked_names(F, L):
    """state-dict keys of the stacked tensors, in StackedMLP order."""
    return {"w_first": [f"fs.{k}.0.weight" for k in range(F)], "b_first": [f"fs.{k}.0.bias" for k in range(F)],
            "w_mid": [[f"fs.{k}.{3 * li}.weight" for k in range(F)] for li in range(1, L - 1)],
            "b_mid": [[f"fs.{k}.{3 * li}.bias" for k in range(F)] for li in range(1, L - 1)],
            "w_last": [f"fs.{k}.{3 * (L - 1)}.weight" for k in range(F)], "b_last": [f"fs.{k}.{3 * (L - 1)}.bias" for k in range(F)]}


def restack(grads, F, L):
    nm = stacked_names(F, L)
    return {"w_first": torch.stack([grads[k][:, 0] for k in nm["w_first"]]), "b_first": torch.stack([grads[k] for k in nm["b_first"]]),
            "w_mid": torch.stack([torch.stack([grads[k] for k in row]) for row in nm["w_mid"]]),
            "b_mid": torch.stack([torch.stack([grads[k] for k in row]) for row in nm["b_mid"]]),
            "w_last": torch.stack([grads[k] for k in nm["w_last"]]), "b_last": torch.stack([grads[k] for k in nm["b_last"]])}


@pytest.mark.parametrize("mode", ["leaf", "linear"])
@pytest.mark.parametrize("sum_features", [True, False], ids=["sum", "per-feature"])
@pytest.mark.parametrize("F,C,L", SHAPES)
def test_feature_mlps_input_gradient(F, C, L, sum_features, mode):
    from gnan_amd import functional
    from gnan_amd.functional import StackedMLP
    sd = _mlp_state(F, L, H, C, True, seed=F * 7 + L)
    x, raw, enc = draw_inputs(F, 11 * F + C)
    wgt = torch.randn(300, C if sum_features else F * C, generator=torch.Generator().manual_seed(3), dtype=torch.float64)

    def loss_of(p, xo, dtype):
        y = O.feature_mlps(xo, p)
        y = y.sum(1) if sum_features else y.reshape(300, -1)
        return (y * wgt.to(dtype)).sum()

    def run(with_x_grad):
        st = _stack(sd, F, L, H, C, True)
        leaves = [q.clone().requires_grad_(True) for q in st[:6]]
        if with_x_grad:
            xd, inputs = device_input_side(mode, x, raw, enc)
        else:
            xd, inputs = x.to(DEV), {}
        y = functional.feature_mlps(xd, StackedMLP(*leaves, *st[6:]), sum_features)
        (y * wgt.to(DEV).float()).sum().backward()
        torch.cuda.synchronize()
        return y.detach(), dict(zip(("w_first", "b_first", "w_mid", "b_mid", "w_last", "b_last"), [q.grad for q in leaves])), inputs

    y, pg, inputs = run(True)
    got = dict(pg)
    got.update({"in." + k: v.grad for k, v in inputs.items()})
    assert all(v is not None for v in got.values())

    def truth(dtype):
        g = oracle_all_grads(loss_of, sd, mode, x, raw, enc, dtype)
        out = restack(g, F, L)
        out.update({k: v for k, v in g.items() if k.startswith("in.")})
        return out
    t64 = truth(torch.float64)
    assert_grads_rule(got, t64, lambda: truth(torch.float32), (F, C, L, sum_features, mode))
    # the input side on its own scale as well (next to large parameter gradients a wrong x.grad could hide under the floor)
    for k in inputs:
        assert_rule(got["in." + k], t64["in." + k], lambda k=k: truth(torch.float32)["in." + k], ("in." + k, F, C, L))
    if mode == "leaf":
        # the parameter gradients do not depend on whether x needs a gradient: the same launches on the same inputs
        y0, pg0, _ = run(False)
        assert torch.equal(y0, y)
        for k in pg:
            assert torch.equal(pg[k], pg0[k]), k


@pytest.mark.parametrize("F,C,L", SHAPES)
def test_without_x_grad_the_route_is_the_moments_route(F, C, L, monkeypatch):
    """``x`` without a gradient: outputs and gradients are those of the look-up, the per-piece moments over the kept pieces and
    ``gnan_fpwl_param_grads`` composed by hand, bit for bit, and the moments launch is the one the describe query names for the
    same arguments — with and without ``x.requires_grad``."""
    from gnan_amd import functional
    from gnan_amd.functional import StackedMLP
    sd = _mlp_state(F, L, H, C, True, seed=F * 7 + L)
    x, _, _ = draw_inputs(F, 11 * F + C)
    xd = x.to(DEV)
    wgt = torch.randn(300, C, generator=torch.Generator().manual_seed(3)).to(DEV)
    st = _stack(sd, F, L, H, C, True)
    routes = []
    real = functional._fpwl_moments

    def spy(*a, **k):
        d = []
        out = real(*a, describe=d, **k)
        routes.append(d[0])
        return out
    monkeypatch.setattr(functional, "_fpwl_moments", spy)
    results = []
    for with_x_grad in (False, True):
        leaves = [q.clone().requires_grad_(True) for q in st[:6]]
        xin = xd.clone().requires_grad_(True) if with_x_grad else xd
        y = functional.feature_mlps(xin, StackedMLP(*leaves, *st[6:]), True)
        (y * wgt).sum().backward()
        results.append((y.detach(), [q.grad for q in leaves]))
    monkeypatch.setattr(functional, "_fpwl_moments", real)
    located = []
    out, tables, _ = functional._fmlp_forward(xd, st, True, False, True, located=located)
    d = []
    M = functional._fpwl_moments(xd, tables, wgt, True, functional._abs_max_cached(xd), raw=True, located=located, describe=d)
    want = functional._fpwl_param_grads_launch(list(st[:6]), tables, M, L, H, C, F)
    torch.cuda.synchronize()
    assert len(routes) == 2 and routes[0] == routes[1] == d[0] and d[0]["kernel"] != 0
    for y, grads in results:
        assert torch.equal(y, out)
        for a, b in zip(grads, want):
            assert torch.equal(a, b)


def test_frozen_parameters_run_the_two_launches_alone(monkeypatch):
    """Saliency on an eval model: parameters without a gradient, ``x`` with one — no moments, no parameter-gradient kernel."""
    from gnan_amd import functional
    F, C, L = 7, 3, 3
    sd = _mlp_state(F, L, H, C, True, seed=5)
    st = _stack(sd, F, L, H, C, True)
    x, _, _ = draw_inputs(F, 2)

    def refuse(*a, **k):
        raise AssertionError("frozen parameters: no parameter-gradient launch expected")
    monkeypatch.setattr(functional, "_fpwl_moments", refuse)
    monkeypatch.setattr(functional, "_fpwl_param_grads_launch", refuse)
    xd = x.to(DEV).requires_grad_(True)
    functional.feature_mlps(xd, st, False).sum().backward()
    xo = x.double().requires_grad_(True)
    O.feature_mlps(xo, {k: v.double() for k, v in sd.items()}).sum().backward()
    assert_rule(xd.grad, xo.grad, None, "saliency")


def _module(kind, F, C, L):
    from gnan_amd import GNAN as standalone
    from gnan_amd import models
    torch.manual_seed(0)
    if kind == "standalone":
        mod = standalone.TensorGNAN(F, C, L, hidden_channels=H, normalize_rho=True, device=DEV)
    else:
        mod = models.TensorGNAN(F, C, L, hidden_channels=H, normalize_rho=True, device=DEV)
        mod.aggregation_order = "reference" if kind == "tensor-reference" else "sum_first"
    _redraw(mod, 7)
    sd = {k: v.detach().cpu().clone() for k, v in mod.state_dict().items()}
    return mod.to(DEV).eval(), sd


@pytest.mark.parametrize("mode", ["leaf", "linear"])
@pytest.mark.parametrize("kind", ["tensor-sum-first", "tensor-reference", "standalone"])
@pytest.mark.parametrize("F,C,L", SHAPES)
def test_modules_input_gradient(F, C, L, kind, mode, monkeypatch):
    from gnan_amd import aggregate
    g, csr = graph300()
    x, raw, enc = draw_inputs(F, 13 * F + L)
    mod, sd = _module(kind, F, C, L)
    target = torch.randn(300, C, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    taken = []
    real = aggregate.reference_order_forward
    monkeypatch.setattr(aggregate, "reference_order_forward", lambda *a, **k: (taken.append(1), real(*a, **k))[1])
    xd, inputs = device_input_side(mode, x, raw, enc)
    y = mod.forward(Bag(x=xd, edge_index=None, gnan_graph=g))
    ((y - target.to(DEV).float()) ** 2).mean().backward()
    torch.cuda.synchronize()
    # the one-node reference order serves the read-out widths the aggregation fuses, with x.requires_grad as without
    assert bool(taken) == (kind == "tensor-reference" and C in aggregate.FUSABLE_READOUT)
    got = {k: p.grad for k, p in mod.named_parameters()}
    got.update({"in." + k: v.grad for k, v in inputs.items()})
    assert all(v is not None for v in got.values())

    def loss_of(p, xo, dtype):
        chain = _oracle_chain("standalone" if kind == "standalone" else "tensor", xo, csr, True)
        return ((chain(p, dtype) - target.to(dtype)) ** 2).mean()
    t64 = oracle_all_grads(loss_of, sd, mode, x, raw, enc, torch.float64)
    t32 = lambda: oracle_all_grads(loss_of, sd, mode, x, raw, enc, torch.float32)   # noqa: E731
    assert_grads_rule(got, t64, t32, (kind, F, C, L, mode))
    for k in inputs:
        assert_rule(got["in." + k], t64["in." + k], lambda k=k: t32()["in." + k], ("in." + k, kind, F, C, L))


def _golden_oracle(gold, dtype, p, x):
    m, i = gold.meta, inputs_from(gold, dtype)
    v = m["variant"]
    if v.startswith("standalone_tensor"):
        return O.tensor_gnan_forward_standalone(x, i["node_distances"], i["normalization_matrix"], p, m["normalize_rho"], v.endswith("graph"))
    if v.startswith("models_tensor"):
        return O.tensor_gnan_forward_models(x, i["node_distances"], i["normalization_matrix"], p, m["normalize_rho"],
                                            v.endswith("graph"), m.get("readout_n_layers", 0))
    return O.gnan_forward(x, i["node_distances"], i["normalization_matrix"], p, m["normalize_rho"], m.get("node_ids"))


@pytest.mark.parametrize("name", ["case_400_kink_models_tensor_node", "case_401_kink_standalone_tensor_node", "case_402_kink_models_gnan",
                                  "case_403_kink_models_tensor_node", "case_404_kink_models_tensor_graph",
                                  "case_405_kink_models_tensor_node"])
def test_kink_goldens_input_gradient(name):
    """One-hot features on zero-bias kinks (or on exactly representable ones): most look-ups land on a point piece, where the
    input derivative is the one AT the kink — ``tables.slope`` would be off by the size of the gradient itself."""
    import gpu_util
    gold = Golden(name)
    mod = gpu_util.build_module(gold)
    data = gpu_util.device_inputs(gold)
    data.x = data.x.float().requires_grad_(True)
    y = gpu_util.call(mod, gold, data)
    y.pow(2).sum().backward()
    torch.cuda.synchronize()
    assert data.x.grad is not None

    def truth(dtype):
        p = {k: v.clone().requires_grad_(True) for k, v in params_from(gold, dtype).items()}
        x = inputs_from(gold, dtype)["x"].clone().requires_grad_(True)
        _golden_oracle(gold, dtype, p, x).pow(2).sum().backward()
        out = {k: v.grad for k, v in p.items()}
        out["in.x"] = x.grad
        return out
    t64 = truth(torch.float64)
    got = {k: q.grad for k, q in mod.named_parameters()}
    got["in.x"] = data.x.grad
    assert_grads_rule(got, t64, lambda: truth(torch.float32), name)
    assert_rule(got["in.x"], t64["in.x"], lambda: truth(torch.float32)["in.x"], name + " x.grad")
