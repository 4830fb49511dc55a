"""Input gradients of the table path, CPU side: the per-piece derivative table (``pwl.piece_derivatives_reference``, the
restatement of ``gnan_pwl_piece_dfdx``) and the look-up (``pwl.input_grad_reference``, of ``gnan_fpwl_input_grad``) against
float64 autograd through the oracle's ``feature_mlps``; and the host side of the two entry points (ABI, symbols, struct
layout, refusals before a launch).  The kernels themselves: tests/test_gpu_input_grad.py."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import gnan_amd  # noqa: F401
from gnan_amd import _lib, pwl
from conftest import ROOT
from helpers import rule
from oracle import gnan_oracle as O
from test_pwl_tables import _on_kink_state, mlp_state, probe_points, stack


def oracle_input_grad(x, g, sd, dtype):
    """``d/dx sum <g, feature_mlps(x)>`` by autograd through the oracle in ``dtype``; ``g [n, F*C]`` (per-feature layout)."""
    xx = x.to(dtype).clone().requires_grad_(True)
    y = O.feature_mlps(xx, {k: v.to(dtype) for k, v in sd.items()}).reshape(x.shape[0], -1)
    (y * g.to(dtype)).sum().backward()
    return xx.grad


def table_input_grad(x, g, st, t, sum_features, table=None):
    """The product's arithmetic restated: the float32 derivative table (one rounding), then the look-up."""
    dfdx = pwl.piece_derivatives_reference(st, t).float() if table is None else table
    return pwl.input_grad_reference(x, g, t, dfdx, sum_features)


def check_against_autograd(sd, F, L, H, C, bias, x, seed=5):
    st = stack(sd, F, L, H, C, bias)
    t = pwl.build_tables(st)
    assert t is not None
    n = x.shape[0]
    g = torch.randn(n, F * C, generator=torch.Generator().manual_seed(seed))
    truth = oracle_input_grad(x, g, sd, torch.float64)
    ok, e, e32 = rule(table_input_grad(x, g, st, t, False), truth, lambda: oracle_input_grad(x, g, sd, torch.float32))
    assert ok, f"per-feature layout: {e:.3e} vs fp32 oracle {e32:.3e}"
    # feature-sum layout: every feature's rows carry the same gradient gs [n, C]
    gs = g[:, :C].contiguous()
    gw = gs.repeat(1, F)
    truth_s = oracle_input_grad(x, gw, sd, torch.float64)
    ok, e, e32 = rule(table_input_grad(x, gs, st, t, True), truth_s, lambda: oracle_input_grad(x, gw, sd, torch.float32))
    assert ok, f"feature-sum layout: {e:.3e} vs fp32 oracle {e32:.3e}"
    return st, t


@pytest.mark.parametrize("F,L,H,C,bias", [
    (3, 1, 0, 2, True), (4, 2, 8, 3, True), (5, 3, 8, 1, True), (9, 3, 32, 5, False), (15, 3, 64, 1, True),
    (7, 4, 16, 7, True), (3, 3, 20, 40, True), (2, 5, 16, 3, True), (6, 3, 33, 2, False),
])
def test_derivative_table_reproduces_autograd(F, L, H, C, bias):
    sd = mlp_state(F, L, max(H, 1), C, bias, seed=F * 100 + L)
    check_against_autograd(sd, F, L, H, C, bias, probe_points(1500, F, 1))


def one_hot_rows(n, F, seed):
    x = torch.randint(0, 2, (n, F), generator=torch.Generator().manual_seed(seed)).float()
    x[:, -1] = 1.0
    return x


ZERO_BIAS_CASES = [(5, 3, 16, 2, 1.0), (5, 3, 64, 1, 0.01)]          # the second: the reference's initialisation (GNAN.py:49-53)


@pytest.mark.parametrize("F,L,H,C,w_scale", ZERO_BIAS_CASES)
def test_zero_bias_one_hot_inputs(F, L, H, C, w_scale):
    """Every kink at 0 and most inputs ON it: the look-up lands on the point piece, whose derivative is taken at the kink."""
    sd = mlp_state(F, L, H, C, True, seed=5, w_scale=w_scale, b_scale=0.0)
    check_against_autograd(sd, F, L, H, C, True, one_hot_rows(3000, F, 7))


def test_reference_initialisation_scale():
    F, L, H, C = 6, 3, 64, 1
    sd = mlp_state(F, L, H, C, True, seed=5, w_scale=0.01, b_scale=0.0)
    check_against_autograd(sd, F, L, H, C, True, torch.rand(1500, F, generator=torch.Generator().manual_seed(2)))


def test_dead_units():
    F, L, H, C = 4, 3, 16, 2
    sd = mlp_state(F, L, H, C, True, seed=3, b_scale=0.0)
    sd["fs.1.0.weight"][::2] = 0.0
    sd["fs.2.0.bias"] += 0.3
    check_against_autograd(sd, F, L, H, C, True, probe_points(1500, F, 2))


@pytest.mark.parametrize("F,L,H,C,mode", [(6, 3, 16, 2, "exact"), (5, 2, 8, 1, "exact"), (3, 4, 8, 1, "exact"), (6, 3, 16, 3, "zero")])
def test_x_on_every_anchor(F, L, H, C, mode):
    """Every anchor of every feature is an input (and the float32 numbers next to it).  Where an anchor is the float32 number
    above a kink that no float32 number hits, autograd and the tables agree that the node lies right of the kink."""
    sd = _on_kink_state(F, L, H, C, mode, seed=3 * F + L)
    st = stack(sd, F, L, H, C, True)
    t = pwl.build_tables(st)
    off = t.off.tolist()
    rows = max(b - a for a, b in zip(off, off[1:]))
    x = torch.zeros(3 * rows, F)
    inf = torch.tensor(float("inf"))
    for k in range(F):
        a = t.anchor[off[k]:off[k + 1]]
        col = torch.cat([a, torch.nextafter(a, inf), torch.nextafter(a, -inf)])
        x[:, k] = col[torch.arange(3 * rows) % col.numel()]
    check_against_autograd(sd, F, L, H, C, True, x)


@pytest.mark.parametrize("F,L,H,C,w_scale", ZERO_BIAS_CASES)
def test_the_slope_is_not_the_derivative_at_a_kink(F, L, H, C, w_scale):
    """The trap: on the point piece behind a kink ``tables.slope`` is the divided difference to the kink's right, autograd takes
    relu'(0) = 0 AT the kink.  On zero-bias one-hot rows the slope route misses by more than a tenth of the largest entry;
    the derivative table stays under the floor."""
    sd = mlp_state(F, L, H, C, True, seed=5, w_scale=w_scale, b_scale=0.0)
    st = stack(sd, F, L, H, C, True)
    t = pwl.build_tables(st)
    x = one_hot_rows(3000, F, 7)
    g = torch.randn(3000, F * C, generator=torch.Generator().manual_seed(5))
    truth = oracle_input_grad(x, g, sd, torch.float64)
    _, e_slope, _ = rule(table_input_grad(x, g, st, t, False, table=t.slope), truth)
    _, e_table, _ = rule(table_input_grad(x, g, st, t, False), truth)
    assert e_slope > 0.1, f"slope route: {e_slope:.3e}"
    assert e_table <= 1e-5, f"derivative table: {e_table:.3e}"


@pytest.mark.parametrize("F,L,H,C,bias", [(4, 2, 8, 3, True), (5, 3, 8, 1, True), (7, 4, 16, 7, True), (3, 3, 20, 40, True)])
def test_derivative_equals_slope_inside_ordinary_pieces(F, L, H, C, bias):
    """On an interior piece [a, a') that is not a point piece the slope is the divided difference (v' - v) / w of float64 network
    values, w = a' - a, rounded to float32; the function is affine on [a, kink') where the true kink' lies within one float32
    step below its rounded-up anchor a'.  Hence, with d the piece's derivative and d+ the derivative right of kink'
    (of the next piece, or of the one behind it when the next is a point piece):

        |dfdx - slope| <= 2^-24 (|dfdx| + |slope|)          the two float32 roundings
                          + |d+ - d| ulp32(a') / w          the stretch [kink', a'] of the divided difference
                          + 2^-44 max(|v|, |v'|, |d| w) / w   float64 evaluation of v, v' (<= 2^8 roundings each) and of d."""
    sd = mlp_state(F, L, H, C, bias, seed=F * 100 + L)
    st = stack(sd, F, L, H, C, bias)
    t = pwl.build_tables(st)
    d64 = pwl.piece_derivatives_reference(st, t)
    d32 = d64.float().double()
    off = t.off.tolist()
    inf = torch.tensor(float("inf"))
    checked = 0
    for k in range(F):
        a = t.anchor[off[k]:off[k + 1]]
        P = a.numel()
        v, s, d = t.val[off[k]:off[k + 1]].double(), t.slope[off[k]:off[k + 1]].double(), d32[off[k]:off[k + 1]]
        dk = d64[off[k]:off[k + 1]]
        for i in range(1, P - 1):
            if not a[i + 1] > torch.nextafter(a[i], inf):
                continue
            w = float(a[i + 1].double() - a[i].double())
            ulp = float(torch.nextafter(a[i + 1], inf).double() - a[i + 1].double())
            jump = (dk[i + 1] - dk[i]).abs()
            if i + 2 < P:
                jump = torch.maximum(jump, (dk[i + 2] - dk[i]).abs())
            bound = (2.0 ** -24 * (d[i].abs() + s[i].abs()) + jump * ulp / w
                     + 2.0 ** -44 * torch.maximum(torch.maximum(v[i].abs(), v[i + 1].abs()), dk[i].abs() * w) / w)
            assert bool(((d[i] - s[i]).abs() <= bound).all()), (k, i, float(((d[i] - s[i]).abs() - bound).max()))
            checked += 1
    assert checked >= F


def test_rows_behind_the_tables_are_zero_and_points_match_the_probes():
    """Capacity-sized tables: rows behind ``off[F]`` get zeros.  The derivative points are the parameter gradients' probe
    points on every piece that can hold a node."""
    F, L, H, C = 3, 3, 8, 2
    st = stack(mlp_state(F, L, H, C, True, seed=1, b_scale=0.0), F, L, H, C, True)
    t = pwl.build_tables(st)
    T = t.anchor.numel()
    big = pwl.PwlTables(t.off, torch.cat([t.anchor, torch.full((7,), 3.0)]), torch.cat([t.val, torch.ones(7, C)]),
                        torch.cat([t.slope, torch.ones(7, C)]), t.max_pieces, t.features_per_group, t.max_group_pieces)
    d = pwl.piece_derivatives_reference(st, big)
    assert d.shape == (T + 7, C) and bool((d[T:] == 0).all())
    assert torch.equal(d[:T], pwl.piece_derivatives_reference(st, t))
    xi = pwl.piece_derivative_points(t)
    u1, u2, _ = pwl.piece_probe_points(t)
    nxt = torch.cat([t.anchor[1:], t.anchor[-1:]])
    up = torch.nextafter(t.anchor, torch.full_like(t.anchor, float("inf")))
    first = torch.zeros(T, dtype=torch.bool)
    last = torch.zeros(T, dtype=torch.bool)
    first[t.off[:-1].long()] = True
    last[t.off[1:].long() - 1] = True
    point = (nxt > t.anchor) & (nxt <= up) & ~first & ~last
    assert bool(point.any())
    assert torch.equal(xi[point], u1[point]) and torch.equal(xi[point], t.anchor.double()[point])
    assert torch.equal(xi[first], t.anchor.double()[first] - 1.0) and torch.equal(xi[last & ~first], t.anchor.double()[last & ~first] + 1.0)
    inner = ~point & ~first & ~last & (nxt > t.anchor)
    assert bool(((xi[inner] > torch.minimum(u1, u2)[inner]) & (xi[inner] < torch.maximum(u1, u2)[inner])).all())


# ---- host side of the entry points ----------------------------------------------------------------------------------------
NEW_SYMBOLS = ("gnan_pwl_piece_dfdx", "gnan_fpwl_input_grad", "gnan_fpwl_input_grad_describe")
NEW_STRUCTS = (("gnan_pwl_dfdx_args", "PwlDfdxArgs"), ("gnan_fpwl_input_grad_args", "FpwlInputGradArgs"),
               ("gnan_fpwl_input_grad_info", "FpwlInputGradInfo"))


def test_abi_number_did_not_move():
    with open(os.path.join(ROOT, "include", "gnan_hip.h")) as f:
        assert re.search(r"^#define GNAN_ABI_VERSION 51$", f.read(), re.M)
    assert _lib.ABI_VERSION == 51 and _lib.lib().gnan_abi_version() == 51


def test_new_symbols_are_exported_and_bound():
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(handle, name), f"{name} not exported"
        assert name in _lib.SYMBOLS, f"{name} not bound"
        assert getattr(_lib.lib(), name).argtypes == _lib.SYMBOLS[name][1]


def test_new_struct_layouts_match_the_header():
    text = open(os.path.join(ROOT, "include", "gnan_hip.h")).read()
    for struct, name in NEW_STRUCTS:
        cls = getattr(_lib, name)
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = []
        for decl in body.split(";"):
            decl = decl.strip()
            if not decl:
                continue
            names = decl.split(None, 1)[1] if not decl.startswith("const") else decl.split(None, 2)[2]
            for n in names.split(","):
                fields.append(n.strip().lstrip("*").strip())
        assert fields == [f[0] for f in cls._fields_], struct


def test_unsupported_shapes_are_refused_before_a_launch():
    """Host-side validation: no pointer is needed to be told that a shape is not served (nothing can have been launched)."""
    lib = _lib.lib()
    for L, H, C in ((1, 8, 1), (5, 16, 1), (3, 65, 1), (4, 65, 2), (2, 129, 1), (3, 16, 4097)):
        a = _lib.PwlDfdxArgs(F=2, L=L, H=H, C=C, T=10)
        assert lib.gnan_pwl_piece_dfdx(a, None) == _lib.ERR_UNSUPPORTED, (L, H, C)
    for L, H, C in ((2, 128, 1), (3, 64, 40), (4, 64, 4096)):                 # served shapes get as far as the pointer check
        assert lib.gnan_pwl_piece_dfdx(_lib.PwlDfdxArgs(F=2, L=L, H=H, C=C, T=10), None) == _lib.ERR_BAD_ARG
    assert lib.gnan_pwl_piece_dfdx(None, None) == _lib.ERR_BAD_ARG
    # the look-up: oversize tables (pwl.oversize) are refused, by the launch and by the query alike
    info = _lib.FpwlInputGradInfo()
    big = _lib.FpwlInputGradArgs(n=5, x_stride=8, F=8, C=172, max_pieces=148, features_per_group=1, max_group_pieces=148,
                                 grad_stride=172 * 8, gx_stride=8)
    t = pwl.PwlTables(None, None, torch.zeros(8 * 148, 172), None, 148, 1, 148)
    assert pwl.oversize(t)
    assert lib.gnan_fpwl_input_grad(big, None) == _lib.ERR_UNSUPPORTED and b"exceed" in lib.gnan_last_error()
    assert lib.gnan_fpwl_input_grad_describe(big, info) == _lib.ERR_UNSUPPORTED
    ok = _lib.FpwlInputGradArgs(n=5, x_stride=8, F=8, C=40, max_pieces=148, features_per_group=1, max_group_pieces=148,
                                grad_stride=40, gx_stride=8)
    assert not pwl.oversize(pwl.PwlTables(None, None, torch.zeros(8 * 148, 40), None, 148, 1, 148))
    assert lib.gnan_fpwl_input_grad(ok, None) == _lib.ERR_BAD_ARG                # null pointers: validated, nothing launched
    assert lib.gnan_fpwl_input_grad(_lib.FpwlInputGradArgs(n=5, F=8, C=1, max_pieces=4, features_per_group=3, max_group_pieces=4),
                                    None) == _lib.ERR_BAD_ARG
    assert lib.gnan_fpwl_input_grad_describe(ok, None) == _lib.ERR_BAD_ARG


def test_describe_reports_the_plan_without_a_device():
    lib = _lib.lib()
    info = _lib.FpwlInputGradInfo()
    assert lib.gnan_fpwl_input_grad_describe(_lib.FpwlInputGradArgs(n=0, F=3, C=2), info) == 0
    assert all(v == 0 for v in info.as_dict().values())
    assert lib.gnan_fpwl_input_grad(_lib.FpwlInputGradArgs(n=0, F=3, C=2), None) == 0          # n = 0: a no-op
    buf = np.zeros(64, dtype=np.float32)               # addresses only: the query reads no memory
    p = buf.ctypes.data
    p16 = p + (-p) % 16
    for F, C, fg, mgp, n, xs, want_bs, want_vec in ((32, 1, 16, 2100, 1000, 32, 512, 1), (33, 1, 16, 2100, 1000, 33, 512, 0),
                                                    (20, 3, 4, 500, 300000, 20, 256, 1), (7, 40, 1, 130, 257, 7, 256, 0),
                                                    (16, 2, 8, 900, 5000, 20, 512, 1)):
        a = _lib.FpwlInputGradArgs(x=p16, n=n, x_stride=xs, F=F, C=C, off=p16, anchor=p16, dfdx=p16, max_pieces=256,
                                   features_per_group=fg, max_group_pieces=mgp, sum_features=1, grad=p16, grad_stride=C,
                                   gx=p16, gx_stride=xs)
        assert lib.gnan_fpwl_input_grad_describe(a, info) == 0
        npb = min(4096, max(256, (n // 1024 + 255) // 256 * 256))
        assert info.as_dict() == dict(block_size=want_bs, nodes_per_block=npb, features_per_group=fg,
                                      lds_bytes=mgp * (1 + pwl.table_stride(C)) * 4, vec=want_vec, n_groups=-(-F // fg),
                                      n_blocks=-(-n // npb)), (F, C, fg)
        a.x = p16 + 4                                   # rows that are not 16-byte aligned: scalar requests
        assert lib.gnan_fpwl_input_grad_describe(a, info) == 0 and info.vec == 0
