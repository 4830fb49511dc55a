"""Four-layer shape functions on the table path, host side (no GPU): the gates, the ABI version and the derivation that
csrc/fpwl_grad.hip:fpwl_grad4_kernel implements — restated here per piece in float64 and compared with the probe-point
route (pwl.parameter_grads_from_moments), which stays the reference the kernel is tested against on the GPU."""
import os
import re

import pytest
import torch

import gnan_amd  # noqa: F401
from gnan_amd import _lib, functional, pwl
from gnan_amd.functional import StackedMLP, _fmlp_eager
from helpers import assert_grads_rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def mlp_state(F, L, H, C, bias, seed):
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k in range(F):
        dims = [1] + [H] * (L - 1) + [C]
        for li in range(L):
            sd[f"fs.{k}.{3 * li}.weight"] = torch.randn(dims[li + 1], dims[li], generator=g) * (2.0 / (dims[li] + dims[li + 1])) ** 0.5
            if bias:
                sd[f"fs.{k}.{3 * li}.bias"] = torch.randn(dims[li + 1], generator=g) * 0.5
    return sd


def stack(sd, F, L, H, C, bias):
    def cat(li, what):
        return torch.stack([sd[f"fs.{k}.{3 * li}.{what}"] for k in range(F)], 0)
    w_mid = torch.stack([cat(li, "weight") for li in range(1, L - 1)], 0)
    b_mid = torch.stack([cat(li, "bias") for li in range(1, L - 1)], 0) if bias else None
    return StackedMLP(cat(0, "weight")[..., 0], cat(0, "bias") if bias else None, w_mid, b_mid,
                      cat(L - 1, "weight"), cat(L - 1, "bias") if bias else None, L, H, C, F)


def test_gradient_gate_covers_four_layers_up_to_64_units():
    g = functional._table_grads_applies
    assert g(4, 64, 1) and g(4, 8, 40)
    assert not g(4, 65, 1) and not g(5, 16, 1)
    # unchanged: L in {2, 3}
    assert g(3, 64, 1) and not g(3, 65, 1) and g(2, 128, 1) and not g(2, 129, 1) and g(3, 16, 4096) and not g(3, 16, 4097)


def test_build_gate_needs_a_device_tensor():
    st = stack(mlp_state(2, 4, 8, 1, True, 0), 2, 4, 8, 1, True)
    assert not pwl.hip_build_applies(st)              # CPU tensors: the torch restatement, at every depth


def test_abi_version_is_51():
    assert _lib.ABI_VERSION == 51
    with open(os.path.join(ROOT, "include", "gnan_hip.h")) as f:
        assert re.search(r"^#define GNAN_ABI_VERSION 51$", f.read(), re.M)


def grads_by_the_derivation(st, t, M):
    """d/dtheta of  sum over pieces ( <M0, f(anchor)> + <M1, slope> )  for a four-layer network, float64, piece by piece: the
    masks D1, D2, D3 at the piece's inner point (pwl.piece_probe_points; a point piece: AT the anchor, strictly z > 0), then
        h1a = D1 (w1 a + b1)    h2a = D2 (W2 h1a + b2)    h3a = D3 (W3 h2a + b3)         value at the anchor
        h1' = D1 w1             h2' = D2 W2 h1'          h3' = D3 W3 h2'                x-derivative
        dW4 = M0 (x) h3a + M1 (x) h3'    db4 = M0    e0 = D3 W4^T M0    e1 = D3 W4^T M1
        dW3 = e0 (x) h2a + e1 (x) h2'    db3 = e0    r0 = D2 W3^T e0    r1 = D2 W3^T e1
        dW2 = r0 (x) h1a + r1 (x) h1'    db2 = r0    q0 = D1 W2^T r0    q1 = D1 W2^T r1
        dw1 = q0 a + q1                  db1 = q0
    Returns the gradients in the order of the non-None stacked tensors."""
    f64 = torch.float64
    F, H, C = st.F, st.H, st.C
    w1 = st.w_first.to(f64)
    b1 = torch.zeros(F, H, dtype=f64) if st.b_first is None else st.b_first.to(f64)
    W2, W3 = st.w_mid[0].to(f64), st.w_mid[1].to(f64)
    b2 = torch.zeros(F, H, dtype=f64) if st.b_mid is None else st.b_mid[0].to(f64)
    b3 = torch.zeros(F, H, dtype=f64) if st.b_mid is None else st.b_mid[1].to(f64)
    W4 = st.w_last.to(f64)
    d_w1, d_b1 = torch.zeros_like(w1), torch.zeros_like(b1)
    d_W2, d_W3, d_b2, d_b3 = torch.zeros_like(W2), torch.zeros_like(W3), torch.zeros_like(b2), torch.zeros_like(b3)
    d_W4, d_b4 = torch.zeros_like(W4), torch.zeros(F, C, dtype=f64)
    u1, _, _ = pwl.piece_probe_points(t)
    off = t.off.tolist()
    M = M.double()
    for k in range(F):
        for i in range(off[k], off[k + 1]):
            M0, M1 = M[i, 0], M[i, 1]
            if not bool((M0 != 0).any() or (M1 != 0).any()):
                continue
            a, xi = t.anchor[i].double(), u1[i]
            D1 = (w1[k] * xi + b1[k] > 0).to(f64)
            h1i = D1 * (w1[k] * xi + b1[k])
            D2 = (W2[k] @ h1i + b2[k] > 0).to(f64)
            h2i = D2 * (W2[k] @ h1i + b2[k])
            D3 = (W3[k] @ h2i + b3[k] > 0).to(f64)
            h1a, h1p = D1 * (w1[k] * a + b1[k]), D1 * w1[k]
            h2a, h2p = D2 * (W2[k] @ h1a + b2[k]), D2 * (W2[k] @ h1p)
            h3a, h3p = D3 * (W3[k] @ h2a + b3[k]), D3 * (W3[k] @ h2p)
            d_W4[k] += torch.outer(M0, h3a) + torch.outer(M1, h3p)
            d_b4[k] += M0
            e0, e1 = D3 * (W4[k].t() @ M0), D3 * (W4[k].t() @ M1)
            d_W3[k] += torch.outer(e0, h2a) + torch.outer(e1, h2p)
            d_b3[k] += e0
            r0, r1 = D2 * (W3[k].t() @ e0), D2 * (W3[k].t() @ e1)
            d_W2[k] += torch.outer(r0, h1a) + torch.outer(r1, h1p)
            d_b2[k] += r0
            q0, q1 = D1 * (W2[k].t() @ r0), D1 * (W2[k].t() @ r1)
            d_w1[k] += q0 * a + q1
            d_b1[k] += q0
    bias = st.b_first is not None
    out = [d_w1] + ([d_b1] if bias else []) + [torch.stack([d_W2, d_W3])] + ([torch.stack([d_b2, d_b3])] if bias else []) + [d_W4]
    return out + ([d_b4] if st.b_last is not None else [])


def probe_route(st, t, M):
    leaves = [None if q is None else q.clone().requires_grad_(True) for q in st[:6]]
    return pwl.parameter_grads_from_moments(
        StackedMLP(*leaves, *st[6:]), t, M,
        lambda U, q: _fmlp_eager(U, StackedMLP(*[None if a is None else a.double() for a in q[:6]], *q[6:]), False))


@pytest.mark.parametrize("F,L,H,C,bias,zero_bias", [(3, 4, 8, 2, True, False), (4, 4, 8, 2, False, False), (3, 4, 8, 2, True, True)])
@pytest.mark.parametrize("sum_features", [False, True])
def test_four_layer_derivation_equals_the_probe_point_route(F, L, H, C, bias, zero_bias, sum_features):
    """The per-piece formulas of fpwl_grad4_kernel in float64 == two probe points per piece through the batched MLP, by the
    rule (truth: the probe-point route in float64; no float32 reference, so the bound is the floor).  Zero biases put every
    kink of every layer at 0 and a fifth of the inputs are exact zeros: the point piece behind that anchor takes its masks AT
    the anchor, as torch's relu'(0) = 0 does."""
    sd = mlp_state(F, L, H, C, bias, seed=11 * F + H + C)
    if zero_bias:
        for k, v in sd.items():
            if k.endswith("bias") and not k.endswith(f".{3 * (L - 1)}.bias"):
                v.zero_()
    st = stack(sd, F, L, H, C, bias)
    t = pwl.build_tables(st)
    assert t is not None
    n = 600
    x = torch.rand(n, F, generator=torch.Generator().manual_seed(5)) * 4 - 2
    x[::5] = 0.0
    g = torch.randn(n, C if sum_features else F * C, generator=torch.Generator().manual_seed(6))
    M = pwl.moments_reference(x, g, t, sum_features)
    want = probe_route(st, t, M)
    got = grads_by_the_derivation(st, t, M)
    assert len(got) == len(want)
    assert_grads_rule(got, [w.double() for w in want], None, "derivation vs probe points")


# ---- the four-layer goldens (tests/golden/make_golden_deep.py; not in manifest.json, which parametrises the older tests) ----
DEEP_GOLDENS = ["case_500_models_tensor_node", "case_501_models_tensor_node", "case_502_models_gnan"]


@pytest.mark.parametrize("name", DEEP_GOLDENS)
def test_oracle_replays_the_four_layer_goldens(name):
    """As tests/test_oracle_golden.py does for the manifest's cases: float32 to the last ulps, float64 and its gradients."""
    import numpy as np
    from conftest import Golden
    from helpers import oracle_forward, params_from
    from oracle import gnan_oracle as O
    g = Golden(name)
    assert g.meta["L"] == 4
    assert O.rel_err(oracle_forward(g, torch.float32), torch.from_numpy(g.out32)) <= 2e-6
    assert O.rel_err(oracle_forward(g, torch.float64), torch.from_numpy(g.out64)) <= 1e-12
    p = {k: v.clone().requires_grad_(True) for k, v in params_from(g, torch.float64).items()}
    oracle_forward(g, torch.float64, p).pow(2).sum().backward()
    for k, ref in g.g64.items():
        got = p[k].grad if p[k].grad is not None else torch.zeros_like(p[k])
        assert float((got - torch.from_numpy(ref)).abs().max()) <= 1e-10 * max(1.0, float(np.abs(ref).max())), k


@pytest.mark.parametrize("name", DEEP_GOLDENS)
def test_cpu_route_matches_the_four_layer_goldens(name):
    import gpu_util
    from conftest import Golden
    from helpers import grad_rule, tolerance_ok
    g = Golden(name)
    mod = gpu_util.build_module(g, "cpu")
    y = gpu_util.call(mod, g, gpu_util.device_inputs(g, "cpu"))
    ok, e_build, e_ref = tolerance_ok(y.detach(), g.out32, g.out64, floor=1e-5)
    assert ok, f"build err {e_build:.3e} vs fp32-reference err {e_ref:.3e}"
    y.pow(2).sum().backward()
    named = dict(mod.named_parameters())
    ok, e_build, e_ref, where = grad_rule({k: named[k].grad for k in g.g64}, g.g64, g.g32)
    assert ok, f"{where}: build {e_build:.3e} vs fp32-reference {e_ref:.3e}"
