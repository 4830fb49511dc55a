"""Four-layer shape functions on the HIP table path (L == 4, H <= 64): gnan_pwl_build against the torch restatement of the
same procedure and the float64 oracle, gnan_fpwl_param_grads against the probe-point route in float64, the refusals outside
the range, and models with n_layers = 4 end to end — eager, and as a captured training step.  Tolerances are the project's
rule (helpers.rule / grad_rule: 1e-5 of the largest float64 entry, or the float32 reference's own error)."""
import numpy as np
import pytest
import torch

from conftest import Golden
from helpers import TWO_FLOORS, assert_grads_rule, assert_rule, grad_rule, module_grads, oracle_grads, tolerance_ok
from oracle import gnan_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"

CASES = [(5, 4, 8, 1, True), (9, 4, 32, 5, False), (64, 4, 64, 1, True), (6, 4, 33, 2, True), (3, 4, 20, 40, True),
         (2, 4, 64, 64, True)]
# Seeds F * 7 + H (as tests/test_gpu_kernels.py draws them).  Checked on the CPU with the torch builder: the closest two
# float64 kinks of any feature lie 2.2e3 (5-8), 4.5e1 (64-64), 1.8e3 (6-33), 9.3e3 (3-20), 6.2e2 (2-64-64) and 6.0e4 (the rho
# shape 1-16) float32 spacings apart: no seed had to be replaced, equal piece counts are a fair demand.  9-32 has no biases:
# every kink of every layer coincides at 0 by construction (one anchor and its point piece in either builder).
RHO_SHAPE = (1, 4, 16, 1, True)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")


class Bag:
    def __init__(self, **kw):
        self.__dict__.update(kw)

    def to(self, device):
        return self


def _mlp_state(F, L, H, C, bias, seed):
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k in range(F):
        dims = [1] + [H] * (L - 1) + [C]
        for li in range(L):
            sd[f"fs.{k}.{3 * li}.weight"] = torch.randn(dims[li + 1], dims[li], generator=g) * (2.0 / (dims[li] + dims[li + 1])) ** 0.5
            if bias:
                sd[f"fs.{k}.{3 * li}.bias"] = torch.randn(dims[li + 1], generator=g) * 0.5
    return sd


def _stack(sd, F, L, H, C, bias, dev=DEV):
    from gnan_amd.functional import StackedMLP

    def cat(li, what):
        return torch.stack([sd[f"fs.{k}.{3 * li}.{what}"] for k in range(F)], 0).to(dev)

    w_mid = torch.stack([cat(li, "weight") for li in range(1, L - 1)], 0)
    b_mid = torch.stack([cat(li, "bias") for li in range(1, L - 1)], 0) if bias else None
    return StackedMLP(cat(0, "weight")[..., 0], cat(0, "bias") if bias else None, w_mid, b_mid,
                      cat(L - 1, "weight"), cat(L - 1, "bias") if bias else None, L, H, C, F)


_BUILT = {}


def _built(case):
    """(state dict, stacked weights on the device, torch builder's tables, kernel's tables, cache keys before / after the kernel
    build) of a case — built once, shared by the build and the gradient tests."""
    if case not in _BUILT:
        from gnan_amd import pwl
        F, L, H, C, bias = case
        sd = _mlp_state(F, L, H, C, bias, seed=F * 7 + H)
        st = _stack(sd, F, L, H, C, bias)
        backend = pwl.BUILD_BACKEND
        try:
            pwl.BUILD_BACKEND = "torch"
            t_ref = pwl.build_tables(st, use_graph=False)
            pwl.BUILD_BACKEND = "auto"
            applies = pwl.hip_build_applies(st)
            before = set(pwl._GraphedBuild._cache)
            t_hip = pwl.build_tables(st)
            after = set(pwl._GraphedBuild._cache)
        finally:
            pwl.BUILD_BACKEND = backend
        _BUILT[case] = (sd, st, t_ref, t_hip, applies, before, after)
    return _BUILT[case]


def _check_tables(sd, F, t_ref, t_hip, n=5000, spread=6.0):
    from gnan_amd import pwl
    assert t_ref is not None and t_hip is not None
    assert torch.equal(t_ref.off, t_hip.off), "same number of pieces per feature"
    assert float((t_ref.anchor - t_hip.anchor).abs().max()) <= 1e-6 * max(1.0, float(t_ref.anchor.abs().max()))
    assert torch.isfinite(t_hip.val).all() and torch.isfinite(t_hip.slope).all() and torch.isfinite(t_hip.anchor).all()
    x = (torch.rand(n, F, generator=torch.Generator().manual_seed(2)) * spread - spread / 2)
    x[:4] = torch.tensor([0.0, 1.0, -50.0, 50.0]).unsqueeze(1)
    truth = O.feature_mlps(x.double(), {k: v.double() for k, v in sd.items()}).reshape(n, -1)
    tc = pwl.PwlTables(*[q.cpu() if torch.is_tensor(q) else q for q in t_hip])
    assert_rule(pwl.evaluate_reference(x, tc, False), truth, lambda: O.feature_mlps(x, sd).reshape(n, -1), "tables vs oracle")


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_four_layer_build_kernel_matches_torch_builder(case):
    """gnan_pwl_build at L == 4 vs the torch restatement (same piece counts, anchors to 1e-6) and vs the float64 oracle on 5000
    points that include 0, 1 and +-50; the route was the kernel (no graph of the torch builder was made)."""
    sd, st, t_ref, t_hip, applies, before, after = _built(case)
    assert applies and before == after
    _check_tables(sd, case[0], t_ref, t_hip)


def test_four_layer_build_kernel_degenerate_weights():
    """Zero first-layer biases (kinks coincide at 0), zero biases in layers 1 and 2, alternate first-layer weights zero, a
    feature whose second hidden layer is dead (W2 = 0, b2 < 0) and an all-zero feature."""
    from gnan_amd import pwl
    F, L, H, C = 5, 4, 16, 2
    sd = _mlp_state(F, L, H, C, True, seed=3)
    sd["fs.0.0.bias"].zero_()
    sd["fs.1.0.bias"].zero_()
    sd["fs.1.3.bias"].zero_()
    sd["fs.2.0.weight"][::2] = 0.0
    sd["fs.3.3.weight"].zero_()
    sd["fs.3.3.bias"].fill_(-0.25)
    for li in range(L):
        sd[f"fs.4.{3 * li}.weight"].zero_()
        sd[f"fs.4.{3 * li}.bias"].zero_()
    st = _stack(sd, F, L, H, C, True)
    t_ref = pwl.build_tables(type(st)(*[None if q is None else q.cpu() for q in st[:6]], *st[6:]))     # CPU tensors: the torch builder
    assert pwl.hip_build_applies(st)
    t_hip = pwl.build_tables(st)
    t_hip_c = pwl.PwlTables(*[q.cpu() if torch.is_tensor(q) else q for q in t_hip])
    _check_tables(sd, F, t_ref, t_hip_c, n=3000, spread=4.0)


def test_refusals_before_a_launch():
    from gnan_amd import _lib
    lib = _lib.lib()

    def args(F, L, H, C, with_mid=True):
        cap = min(1024, max(64, 4 * H) * (L - 1))
        keep = [torch.zeros(F, H, device=DEV), torch.zeros(max(L - 2, 1), F, H, H, device=DEV), torch.zeros(F, C, H, device=DEV),
                torch.empty(F * (cap + 1), device=DEV), torch.empty(F * (cap + 1), C, device=DEV),
                torch.empty(F * (cap + 1), C, device=DEV), torch.empty(F + 2, dtype=torch.int32, device=DEV),
                torch.empty(lib.gnan_pwl_build_scratch_bytes(F, C, cap) // 8 + 1, dtype=torch.float64, device=DEV)]
        a = _lib.PwlBuildArgs(w_first=_lib.ptr(keep[0]), b_first=None, w_mid=_lib.ptr(keep[1]) if with_mid else None, b_mid=None,
                              w_last=_lib.ptr(keep[2]), b_last=None, F=F, L=L, H=H, C=C, cap=cap, anchor=_lib.ptr(keep[3]),
                              val=_lib.ptr(keep[4]), slope=_lib.ptr(keep[5]), off=_lib.ptr(keep[6]),
                              overflow=keep[6][F + 1:].data_ptr(), scratch=_lib.ptr(keep[7]), scratch_bytes=keep[7].numel() * 8)
        return a, keep

    stream = torch.cuda.current_stream().cuda_stream
    a, keep = args(2, 4, 65, 1)
    assert lib.gnan_pwl_build(a, stream) == _lib.ERR_UNSUPPORTED and b"L == 4" in lib.gnan_last_error()
    a, keep = args(2, 5, 16, 1)
    assert lib.gnan_pwl_build(a, stream) == _lib.ERR_UNSUPPORTED and b"{2, 3, 4}" in lib.gnan_last_error()
    a, keep = args(2, 4, 8, 1, with_mid=False)
    assert lib.gnan_pwl_build(a, stream) == _lib.ERR_BAD_ARG and b"w_mid" in lib.gnan_last_error()

    def grad_args(F, L, H, C, with_mid=True, with_d_mid=True):
        mids = max(L - 2, 1)
        keep = [torch.zeros(F + 1, dtype=torch.int32, device=DEV), torch.zeros(4, device=DEV), torch.zeros(4, 2, C, device=DEV),
                torch.zeros(F, H, device=DEV), torch.zeros(mids, F, H, H, device=DEV), torch.zeros(F, C, H, device=DEV),
                torch.zeros(F, H, device=DEV), torch.zeros(mids, F, H, H, device=DEV), torch.zeros(F, C, H, device=DEV)]
        a = _lib.FpwlGradArgs(off=_lib.ptr(keep[0]), anchor=_lib.ptr(keep[1]), moments=_lib.ptr(keep[2]), moments_fixed=None,
                              scales=None, w_first=_lib.ptr(keep[3]), b_first=None, w_mid=_lib.ptr(keep[4]) if with_mid else None,
                              b_mid=None, w_last=_lib.ptr(keep[5]), b_last=None, F=F, L=L, H=H, C=C, max_pieces=4,
                              d_w_first=_lib.ptr(keep[6]), d_b_first=None, d_w_mid=_lib.ptr(keep[7]) if with_d_mid else None,
                              d_b_mid=None, d_w_last=_lib.ptr(keep[8]), d_b_last=None)
        return a, keep

    a, keep = grad_args(2, 4, 65, 1)
    assert lib.gnan_fpwl_param_grads(a, stream) == _lib.ERR_UNSUPPORTED and b"H <= 64" in lib.gnan_last_error()
    a, keep = grad_args(2, 5, 16, 1)
    assert lib.gnan_fpwl_param_grads(a, stream) == _lib.ERR_UNSUPPORTED and b"{2, 3, 4}" in lib.gnan_last_error()
    a, keep = grad_args(2, 4, 8, 65)
    assert lib.gnan_fpwl_param_grads(a, stream) == _lib.ERR_UNSUPPORTED and b"C <= 64" in lib.gnan_last_error()
    a, keep = grad_args(2, 4, 8, 1, with_mid=False)
    assert lib.gnan_fpwl_param_grads(a, stream) == _lib.ERR_BAD_ARG and b"w_mid" in lib.gnan_last_error()
    a, keep = grad_args(2, 4, 8, 1, with_d_mid=False)
    assert lib.gnan_fpwl_param_grads(a, stream) == _lib.ERR_BAD_ARG and b"d_w_mid" in lib.gnan_last_error()
    torch.cuda.synchronize()


def _probe_route(st, t, M64):
    from gnan_amd import pwl
    from gnan_amd.functional import StackedMLP, _fmlp_eager
    leaves = [None if q is None else q.clone().requires_grad_(True) for q in st[:6]]
    return pwl.parameter_grads_from_moments(
        StackedMLP(*leaves, *st[6:]), t, M64,
        lambda U, q: _fmlp_eager(U, StackedMLP(*[None if a is None else a.double() for a in q[:6]], *q[6:]), False))


def _moments64(M):
    return M[0].double() / M[1].view(1, 2, 1) if isinstance(M, tuple) else M.double()


@pytest.mark.parametrize("fixed", [True, False], ids=["fixed", "float"])
@pytest.mark.parametrize("case", CASES + [RHO_SHAPE], ids=lambda c: "-".join(map(str, c)))
def test_four_layer_gradient_kernel_matches_probe_points(case, fixed, monkeypatch):
    """gnan_fpwl_param_grads at L == 4 on the moments gnan_fpwl_moments made (both formats) vs two probe points per piece
    through the batched MLP in float64 on the same tables and moments; two runs give the same bits."""
    from gnan_amd import functional
    F, L, H, C, bias = case
    sd, st, _, t, _, _, _ = _built(case)
    monkeypatch.setattr(functional, "MOMENTS_FIXED_POINT", fixed)
    n = 2000
    x = (torch.rand(n, F, generator=torch.Generator().manual_seed(3)) * 4 - 2).to(DEV)
    g = torch.randn(n, F * C, generator=torch.Generator().manual_seed(4)).to(DEV)
    M = functional._fpwl_moments(x, t, g, False, raw=True)
    assert fixed or not isinstance(M, tuple)          # (64 channels: the 64-bit bins do not fit LDS, float moments either way)
    got = functional._fpwl_param_grads_launch(list(st[:6]), t, M, L, H, C, F)
    again = functional._fpwl_param_grads_launch(list(st[:6]), t, M, L, H, C, F)
    for a, b, q in zip(got, again, st[:6]):
        assert (a is None) == (q is None)
        if a is not None:
            assert a.shape == q.shape and torch.equal(a, b)
    want = _probe_route(st, t, _moments64(M))
    assert_grads_rule([a for a in got if a is not None], list(want), None, case)


def test_four_layer_gradients_on_kinks_take_relu_prime_zero():
    """One-hot inputs with zero hidden biases (the golden cases 400-405 at four layers): most look-ups sit exactly on the anchor
    0 where every hidden pre-activation is 0.  Their point piece takes its masks AT the anchor, strictly: the bias gradients
    equal the probe-point route's and autograd's through the float64 oracle (relu'(0) = 0)."""
    from gnan_amd import functional, pwl
    F, L, H, C = 6, 4, 16, 2
    sd = _mlp_state(F, L, H, C, True, seed=41)
    for k in range(F):
        for li in range(L - 1):
            sd[f"fs.{k}.{3 * li}.bias"].zero_()
    st = _stack(sd, F, L, H, C, True)
    t = pwl.build_tables(st)
    n = 1500
    hot = torch.randint(0, F, (n,), generator=torch.Generator().manual_seed(5))
    x = torch.zeros(n, F)
    x[torch.arange(n), hot] = 1.0
    g = torch.randn(n, F * C, generator=torch.Generator().manual_seed(6))
    M = functional._fpwl_moments(x.to(DEV), t, g.to(DEV), False, raw=True)
    got = functional._fpwl_param_grads_launch(list(st[:6]), t, M, L, H, C, F)
    want = _probe_route(st, t, _moments64(M))
    assert_grads_rule(got, list(want), None, "kernel vs probe points")
    sd64 = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    O.feature_mlps(x.double(), sd64).reshape(n, -1).backward(g.double())
    truth = {"b_first": torch.stack([sd64[f"fs.{k}.0.bias"].grad for k in range(F)]),
             "b_mid": torch.stack([torch.stack([sd64[f"fs.{k}.{3 * li}.bias"].grad for k in range(F)]) for li in (1, 2)]),
             "w_first": torch.stack([sd64[f"fs.{k}.0.weight"].grad[:, 0] for k in range(F)]),
             "w_mid": torch.stack([torch.stack([sd64[f"fs.{k}.{3 * li}.weight"].grad for k in range(F)]) for li in (1, 2)]),
             "w_last": torch.stack([sd64[f"fs.{k}.9.weight"].grad for k in range(F)]),
             "b_last": torch.stack([sd64[f"fs.{k}.9.bias"].grad for k in range(F)])}
    by_name = dict(zip(("w_first", "b_first", "w_mid", "b_mid", "w_last", "b_last"), got))
    assert_grads_rule(by_name, truth, None, "kernel vs oracle autograd")


# ---- end to end ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def graph3000():
    """3000 nodes, one hop (self, neighbour, rest), 16 features; unique directed edges without self loops."""
    from gnan_amd import synthetic as syn
    rng = np.random.default_rng(0)
    n, F = 3000, 16
    e = rng.integers(0, n, (2, 12000))
    e = np.unique(e[:, e[0] != e[1]], axis=1)
    src, dst = torch.from_numpy(e[0]).to(DEV), torch.from_numpy(e[1]).to(DEV)
    g = syn.hop1_csr(src, dst, n)
    x = torch.rand(n, F, generator=torch.Generator().manual_seed(1)) * 4 - 2
    csr = (g.rowptr.cpu().long().numpy(), g.col.cpu().numpy(), g.code.cpu().numpy(), g.cnt.cpu().long().numpy())
    return g, x, csr


def _redraw(mod, seed):
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for _, p in mod.named_parameters():
            p.copy_(torch.randn(p.shape, generator=gen) * (0.5 if p.dim() == 1 else (2.0 / sum(p.shape)) ** 0.5))


def _oracle_chain(kind, x, csr, normalize):
    rowptr, col, code, cnt = csr

    def forward(p, dtype):
        S = O.feature_mlps(x.to(dtype), p).sum(1)
        if kind == "standalone":                     # pre-rho normalisation (GNAN.py:65-67), shell form
            wtab = O.row_lut_pre_rho(p, cnt, dtype)                                      # [n, 3, C]
            rp = torch.from_numpy(rowptr)
            row_of = torch.repeat_interleave(torch.arange(len(rowptr) - 1), rp[1:] - rp[:-1])
            w_e = wtab[row_of, torch.from_numpy(code.astype(np.int64))]
            w_rest = wtab[:, -1]
            out = torch.zeros(len(rowptr) - 1, S.shape[1], dtype=dtype).index_add(
                0, row_of, (w_e - w_rest[row_of]) * S[torch.from_numpy(col.astype(np.int64))])
            return out + w_rest * S.sum(0, keepdim=True)
        return O.spmm_csr_vectorised(rowptr, col, code, S, O.rho_lut(p, 3, dtype), cnt if normalize else None)
    return forward


@pytest.mark.parametrize("kind,hidden,normalize", [("tensor", 16, True), ("tensor", 16, False), ("tensor", 64, True),
                                                   ("tensor", 64, False), ("gnan", 16, True), ("gnan", 16, False),
                                                   ("gnan", 64, True), ("gnan", 64, False), ("standalone", 16, True)])
def test_four_layer_models_end_to_end(kind, hidden, normalize, graph3000, monkeypatch):
    """n_layers = 4 through the modules on the table path: forward and every parameter gradient against autograd through the
    float64 oracle — with the torch table builder and the batched-GEMM restatement made to raise, so neither is reached.
    ``standalone`` (the stand-alone file's TensorGNAN, pre-rho normalisation) sends a four-layer rho through
    ``_rho_param_grads``; the ``models`` classes tabulate rho on the three hop values."""
    from gnan_amd import GNAN as standalone
    from gnan_amd import _lib, functional, models, pwl
    g, x, csr = graph3000
    n, F = x.shape
    C = 3
    monkeypatch.setattr(functional, "FMLP_ALGO", _lib.FMLP_PWL)
    torch.manual_seed(0)
    if kind == "tensor":
        mod = models.TensorGNAN(F, C, 4, hidden_channels=hidden, normalize_rho=normalize, device=DEV)
    elif kind == "gnan":
        mod = models.GNAN(F, C, num_layers=4, hidden_channels=hidden, normalize_rho=normalize, device=DEV)
    else:
        mod = standalone.TensorGNAN(F, C, 4, hidden_channels=hidden, normalize_rho=normalize, device=DEV)
    _redraw(mod, 7)
    sd = {k: v.detach().cpu().clone() for k, v in mod.state_dict().items()}
    mod = mod.to(DEV).eval()
    target = torch.randn(n, C, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    data = Bag(x=x.to(DEV), edge_index=None, gnan_graph=g)

    def refuse(*a, **k):
        raise AssertionError("a four-layer step reached the torch route")
    monkeypatch.setattr(functional, "_fmlp_eager", refuse)
    monkeypatch.setattr(pwl, "_build_padded", refuse)
    y = mod.forward(data)
    ((y - target.to(DEV).float()) ** 2).mean().backward()
    torch.cuda.synchronize()

    chain = _oracle_chain(kind, x, csr, normalize)
    with torch.no_grad():
        truth = chain({k: v.double() for k, v in sd.items()}, torch.float64)
    assert_rule(y.detach().cpu(), truth, lambda: chain(sd, torch.float32), (kind, hidden, normalize))
    g64 = oracle_grads(lambda p: ((chain(p, torch.float64) - target) ** 2).mean(), sd, torch.float64)
    g32 = lambda: oracle_grads(lambda p: ((chain(p, torch.float32) - target.float()) ** 2).mean(), sd, torch.float32)   # noqa: E731
    ok, e_build, e_ref, where = grad_rule(module_grads(mod), g64, g32)
    assert ok, f"{where}: build {e_build:.3e} vs fp32 oracle {e_ref:.3e}"


def test_four_layer_training_step_is_captured_and_replayed(graph3000, monkeypatch):
    """harness.train_epoch on a four-layer model: after the eager warm-up epochs the whole step is one replayed hipGraph (the
    table build inside it needs no read-back), and the loss trajectory is the eager loop's."""
    from gnan_amd import _lib, functional, harness, models
    g, x, _ = graph3000
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
        model = models.TensorGNAN(F, C, 4, hidden_channels=16, device=DEV)
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


# ---- goldens captured from the reference at four layers (tests/golden/make_golden_deep.py) ---------------------------------
@pytest.mark.parametrize("algo", ["auto", "pwl"])
@pytest.mark.parametrize("name", ["case_500_models_tensor_node", "case_501_models_tensor_node", "case_502_models_gnan"])
def test_four_layer_goldens_through_the_modules(name, algo, monkeypatch):
    import gpu_util
    from gnan_amd import _lib, functional
    monkeypatch.setattr(functional, "FMLP_ALGO", _lib.FMLP_AUTO if algo == "auto" else _lib.FMLP_PWL)
    gold = Golden(name)
    mod = gpu_util.build_module(gold)
    y = gpu_util.call(mod, gold, gpu_util.device_inputs(gold))
    ok, e_build, e_ref = tolerance_ok(y.detach().cpu(), gold.out32, gold.out64, floor=1e-5)
    assert ok, f"build err {e_build:.3e} vs fp32-reference err {e_ref:.3e}"
    y.pow(2).sum().backward()
    named = dict(mod.named_parameters())
    ok, e_build, e_ref, where = grad_rule({k: named[k].grad for k in gold.g64}, gold.g64, gold.g32)
    assert ok, f"{where}: build {e_build:.3e} vs fp32-reference {e_ref:.3e}"
