"""Training-mode Dropout on the matrix cores: gnan_fmlp_fwd(algo = MFMA, dropout_p > 0), gnan_fmlp_bwd_mfma,
gnan_dropout_mask_window and their routing in functional._DropoutMLPs — against the oracle's Linear / ReLU / Dropout chain fed
with the masks gnan_dropout_mask writes out (the chain of test_gpu_kernels.test_training_mode_dropout_in_the_kernels), by the
project's rule: rel_err <= 1e-5 on outputs, helpers.assert_grads_rule on gradients.

tests/golden/dropout_mfma_parent_bits.npz holds what the commit BEFORE this feature computed on an MI355X for three calls
(inputs included): the matrix-core forward without Dropout, feature_mlps_dropout on its lane route, and the restatement's
backward of a C = 9 model — the bits those calls must still give."""
import os

import numpy as np
import pytest
import torch

from oracle import gnan_oracle as O
from helpers import TWO_FLOORS, assert_grads_rule
from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAMES = ("w_first", "b_first", "w_mid", "b_mid", "w_last", "b_last")
P, SEED = 0.6, 123456789012345


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")


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


def _stack(sd, F, L, H, C, bias):
    from gnan_amd.functional import StackedMLP

    def cat(li, what):
        return torch.stack([sd[f"fs.{k}.{3 * li}.{what}"] for k in range(F)], 0).to(DEV)

    w_mid = torch.stack([cat(li, "weight") for li in range(1, L - 1)], 0)
    b_mid = torch.stack([cat(li, "bias") for li in range(1, L - 1)], 0) if bias else None
    return StackedMLP(cat(0, "weight")[..., 0], cat(0, "bias") if bias else None, w_mid, b_mid,
                      cat(L - 1, "weight"), cat(L - 1, "bias") if bias else None, L, H, C, F)


def _inputs(n, F, C, sum_features, seed=1):
    gen = torch.Generator().manual_seed(seed)
    x = torch.rand(n, F, generator=gen) * 2 - 0.5
    gup = torch.randn(n, C if sum_features else F * C, generator=gen)
    return x, gup


def _oracle(x, sd, keep, p, sum_features, gup=None):
    """float64 forward (and, with ``gup``, the stacked parameter gradients) of the reference chain with the masks ``keep``."""
    n, F = x.shape
    sd64 = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    ref = O.feature_mlps(x.double(), sd64, keep=keep, drop_p=p if keep is not None else 0.0)
    ref = ref.sum(1) if sum_features else ref.reshape(n, -1)
    if gup is None:
        return ref.detach(), None
    ref.backward(gup.double())
    L = 1 + max(int(k.split(".")[2]) for k in sd) // 3
    last = 3 * (L - 1)
    bias = f"fs.0.{last}.bias" in sd
    want = {"w_last": torch.stack([sd64[f"fs.{k}.{last}.weight"].grad for k in range(F)]),
            "w_first": torch.stack([sd64[f"fs.{k}.0.weight"].grad[:, 0] for k in range(F)]),
            "w_mid": torch.stack([torch.stack([sd64[f"fs.{k}.{3 * li}.weight"].grad for k in range(F)]) for li in range(1, L - 1)])}
    if bias:
        want["b_last"] = torch.stack([sd64[f"fs.{k}.{last}.bias"].grad for k in range(F)])
        want["b_first"] = torch.stack([sd64[f"fs.{k}.0.bias"].grad for k in range(F)])
        want["b_mid"] = torch.stack([torch.stack([sd64[f"fs.{k}.{3 * li}.bias"].grad for k in range(F)]) for li in range(1, L - 1)])
    return ref.detach(), want


def _masks(n, F, L, H, p=P, seed=SEED):
    from gnan_amd.functional import dropout_masks
    return dropout_masks(seed, p, n, F, L - 1, H, DEV).cpu()


def _forward(x, st, sum_features, algo, p=P, seed=SEED, x_pad=0, out_pad=0):
    """gnan_fmlp_fwd called directly: ``x_pad`` / ``out_pad`` extra floats per row of x / out (strides beyond the widths)."""
    from gnan_amd import _lib
    n, F = x.shape
    xb = torch.full((n, F + x_pad), 7.0, device=DEV)
    xb[:, :F] = x.to(DEV)
    width = st.C if sum_features else st.F * st.C
    out = torch.full((n, width + out_pad), -77.0, device=DEV)
    keep = [None if t is None else t.detach().float().contiguous() for t in st[:6]]
    a = _lib.FmlpArgs(x=_lib.ptr(xb), n=n, x_stride=xb.stride(0), F=st.F, L=st.L, H=st.H, C=st.C, w_first=_lib.ptr(keep[0]),
                      b_first=_lib.ptr(keep[1]), w_mid=_lib.ptr(keep[2]), b_mid=_lib.ptr(keep[3]), w_last=_lib.ptr(keep[4]),
                      b_last=_lib.ptr(keep[5]), sum_features=int(sum_features), out=_lib.ptr(out), out_stride=out.stride(0),
                      algo=algo, dropout_p=p, dropout_seed=seed)
    need = _lib.lib().gnan_fmlp_fwd_workspace_bytes(a)
    ws = torch.empty(max(need, 4) // 4, dtype=torch.float32, device=DEV)
    a.workspace, a.workspace_bytes = _lib.ptr(ws), need
    _lib.check(_lib.lib().gnan_fmlp_fwd(a, _lib.stream_of(xb)), "gnan_fmlp_fwd")
    torch.cuda.synchronize()
    if out_pad:
        assert bool((out[:, width:] == -77.0).all())                  # nothing is written past the output's width
    return out[:, :width].contiguous()


FORWARD_CASES = [
    # n: one lane / a second tile / a second workgroup / ragged; F: odd counts re-fetch the last double-buffer slot, F = 5 at
    # n = 33 also cuts feature chunks; (L, H): HT 1 / 2, padded units, two mid layers
    (1, 1, 3, 8, 1, True, False), (33, 5, 3, 33, 3, True, True), (33, 5, 4, 64, 8, False, False), (257, 2, 3, 64, 1, True, True),
    (257, 5, 4, 32, 3, True, False), (700, 1, 3, 64, 8, True, True), (700, 2, 3, 8, 3, False, True), (700, 5, 3, 33, 1, True, False),
    (700, 2, 4, 64, 1, False, True), (1, 5, 4, 32, 8, True, True), (33, 1, 3, 64, 3, False, False), (257, 1, 4, 64, 8, True, True),
    (33, 2, 3, 64, 1, True, False), (257, 5, 3, 8, 8, False, True), (700, 1, 4, 32, 3, True, False),
]


@pytest.mark.parametrize("n,F,L,H,C,bias,sum_features", FORWARD_CASES)
def test_forward_on_the_matrix_cores_under_dropout_vs_oracle(n, F, L, H, C, bias, sum_features):
    """gnan_fmlp_fwd(algo = MFMA, p = 0.6) == the oracle with gnan_dropout_mask's masks: a wrong unit, layer or node coordinate
    in the kernel's hash is an O(1) error.  (Before this feature the call was refused: GNAN_ERR_UNSUPPORTED.)"""
    from gnan_amd import _lib
    sd = _mlp_state(F, L, H, C, bias, seed=F + L + H)
    st = _stack(sd, F, L, H, C, bias)
    x, _ = _inputs(n, F, C, sum_features)
    y = _forward(x, st, sum_features, _lib.FMLP_MFMA)
    ref, _ = _oracle(x, sd, _masks(n, F, L, H), P, sum_features)
    err = O.rel_err(y.cpu(), ref)
    print(f"forward ({n}, {F}, {L}, {H}, {C}): rel_err {err:.3e}")
    assert err <= 1e-5
    # the lane kernel, same masks: the two agree to rounding
    assert O.rel_err(_forward(x, st, sum_features, _lib.FMLP_LANE).cpu(), ref) <= 1e-5


@pytest.mark.parametrize("x_pad,out_pad", [(3, 0), (0, 5)])
def test_forward_row_strides_beyond_the_widths(x_pad, out_pad):
    from gnan_amd import _lib
    n, F, L, H, C = 257, 5, 3, 33, 3
    sd = _mlp_state(F, L, H, C, True, seed=3)
    st = _stack(sd, F, L, H, C, True)
    x, _ = _inputs(n, F, C, False)
    y = _forward(x, st, False, _lib.FMLP_MFMA, x_pad=x_pad, out_pad=out_pad)
    assert torch.equal(y, _forward(x, st, False, _lib.FMLP_MFMA))
    ref, _ = _oracle(x, sd, _masks(n, F, L, H), P, False)
    assert O.rel_err(y.cpu(), ref) <= 1e-5


@pytest.mark.parametrize("L", [3, 4])
def test_every_units_keep_bit_is_gnan_dropout_masks(L):
    """Weights that expose ONE keep bit per output, H = 64 (both 32-unit tiles, every accumulator quarter, both lane halves),
    feature k probing unit k, 700 nodes.  b1 = 1, w1 = 0: h1 = keep_0 / (1 - p).
      last hidden layer, unit j: the layer before it has W = 0, b = 1, w_last = e_j           -> out = keep_last[j] / (1 - p)
      hidden layer l < last, unit j: the next layer reads unit j into every unit (column j of ones), later layers sum
      everything (ones), w_last = ones                  -> out != 0 iff keep_l[j] and some unit of every later layer is kept
    compared bit by bit with gnan_dropout_mask, whose kept fraction is therefore the kernel's."""
    from gnan_amd import _lib
    from gnan_amd.functional import StackedMLP
    n, F, H = 700, 64, 64
    keep = _masks(n, F, L, H).bool()                                     # [n, F, L - 1, H]
    x = torch.zeros(n, F)
    scale = 1.0 / (1.0 - P)
    assert abs(float(keep.float().mean()) - (1 - P)) < 0.005
    eye = torch.eye(H)
    for layer in range(L - 1):
        w_mid = torch.zeros(L - 2, F, H, H)
        b_mid = torch.zeros(L - 2, F, H)
        if layer >= 1:
            b_mid[layer - 1] = 1.0                                       # z = 1 in every unit of the probed layer (W = 0 before it)
        if layer == L - 2:
            w_last = eye.clone().reshape(F, 1, H)                        # feature k reads unit k
        else:
            w_mid[layer] = eye.reshape(F, 1, H).expand(F, H, H)          # feature k: every unit of the next layer reads unit k
            w_mid[layer + 1:] = 1.0
            w_last = torch.ones(F, 1, H)
        st = StackedMLP(torch.zeros(F, H).to(DEV), torch.ones(F, H).to(DEV), w_mid.to(DEV), b_mid.to(DEV), w_last.to(DEV), None,
                        L, H, 1, F)
        y = _forward(x, st, False, _lib.FMLP_MFMA).cpu()                 # [n, F]
        bit = keep[:, :, layer].diagonal(dim1=1, dim2=2)                 # [n, F]: unit k of feature k
        if layer == L - 2:
            assert torch.equal(y != 0, bit), layer
            assert float((y[bit] - scale).abs().max()) <= 1e-6 * scale
        else:
            later = torch.ones(n, F, dtype=torch.bool)
            for l2 in range(layer + 1, L - 1):
                later &= keep[:, :, l2].any(-1)
            assert torch.equal(y != 0, bit & later), layer
        frac = float((y != 0).float().mean())
        assert abs(frac - (1 - P)) < 0.02, (layer, frac)
        for quarter in range(8):                                         # both tiles x four quarters: units of both lane halves
            cols = slice(8 * quarter, 8 * quarter + 8)
            assert 0 < int((y[:, cols] != 0).sum()) < y[:, cols].numel()


def test_forward_bits_without_dropout_same_seed_other_seed():
    from gnan_amd import _lib
    z = np.load(os.path.join(GOLDEN_DIR, "dropout_mfma_parent_bits.npz"))
    st, x = _golden_model(z, "mfma0"), torch.from_numpy(z["mfma0/x"])
    for sum_features in (False, True):
        want = torch.from_numpy(z[f"mfma0/out{int(sum_features)}"])
        # p = 0 launches the instance without Dropout, whatever the seed: the bits of the commit before this feature
        assert torch.equal(_forward(x, st, sum_features, _lib.FMLP_MFMA, p=0.0, seed=0).cpu(), want)
        assert torch.equal(_forward(x, st, sum_features, _lib.FMLP_MFMA, p=0.0, seed=SEED).cpu(), want)
        a = _forward(x, st, sum_features, _lib.FMLP_MFMA)
        assert torch.equal(a, _forward(x, st, sum_features, _lib.FMLP_MFMA))
        assert not torch.equal(a, _forward(x, st, sum_features, _lib.FMLP_MFMA, seed=SEED + 1))
        assert not torch.equal(a.cpu(), want)


def _golden_model(z, tag):
    from gnan_amd.functional import StackedMLP
    L, H, C, F = (int(v) for v in z[f"{tag}/shape"])
    ts = [torch.from_numpy(z[f"{tag}/{nm}"]).to(DEV) if f"{tag}/{nm}" in z.files else None for nm in NAMES]
    return StackedMLP(*ts, L, H, C, F)


def _backward(x, st, gup, sum_features, p, seed=SEED, mfma=True):
    """gnan_fmlp_bwd_mfma (or gnan_fmlp_bwd) called directly; the six outputs are cut from ONE buffer with guard floats
    between them, which must come back untouched."""
    from gnan_amd import _lib
    F, H, C = st.F, st.H, st.C
    xd, g = x.to(DEV).contiguous(), gup.to(DEV).contiguous()
    keep = [None if t is None else t.detach().float().contiguous() for t in st[:6]]
    w_mid, b_mid = keep[2][0], None if keep[3] is None else keep[3][0]
    sizes = [F * H, F * H, F * H * H, F * H, F * C * H, F * C]
    guard = 16
    buf = torch.full((sum(sizes) + guard * 7,), -77.0, device=DEV)
    outs, pos = [], guard
    for t, sz in zip(keep, sizes):
        outs.append(None if t is None else buf[pos:pos + sz])
        pos += sz + guard
    a = _lib.FmlpBwdArgs(x=_lib.ptr(xd), n=xd.shape[0], x_stride=xd.stride(0), F=F, L=3, H=H, C=C, w_first=_lib.ptr(keep[0]),
                         b_first=_lib.ptr(keep[1]), w_mid=_lib.ptr(w_mid), b_mid=_lib.ptr(b_mid), w_last=_lib.ptr(keep[4]),
                         b_last=_lib.ptr(keep[5]), sum_features=int(sum_features), grad=_lib.ptr(g), grad_stride=g.stride(0),
                         d_w_first=_lib.ptr(outs[0]), d_b_first=_lib.ptr(outs[1]), d_w_mid=_lib.ptr(outs[2]),
                         d_b_mid=_lib.ptr(outs[3]), d_w_last=_lib.ptr(outs[4]), d_b_last=_lib.ptr(outs[5]), dropout_p=p,
                         dropout_seed=seed)
    lib = _lib.lib()
    need = lib.gnan_fmlp_bwd_mfma_workspace_bytes(a) if mfma else lib.gnan_fmlp_bwd_workspace_bytes(a)
    ws = torch.full((max(need, 4) // 4,), float("nan"), device=DEV)
    a.workspace, a.workspace_bytes = _lib.ptr(ws), need
    if mfma:
        _lib.check(lib.gnan_fmlp_bwd_mfma(a, _lib.stream_of(xd)), "gnan_fmlp_bwd_mfma")
    else:
        _lib.check(lib.gnan_fmlp_bwd(a, _lib.stream_of(xd)), "gnan_fmlp_bwd")
    torch.cuda.synchronize()
    written = torch.zeros_like(buf, dtype=torch.bool)
    for o in outs:
        if o is not None:
            written[o.storage_offset():o.storage_offset() + o.numel()] = True
    assert bool((buf[~written] == -77.0).all())            # guards, and the slots of absent biases: untouched
    return {nm: o.clone() for nm, o in zip(NAMES, outs) if o is not None}, need


BACKWARD_CASES = [
    # n = 700 with F = 1: several node ranges, hence the reduce kernel
    (1, 1, 8, 1, True, False, 0.6), (31, 3, 33, 3, True, True, 0.6), (32, 3, 64, 8, False, False, 0.6), (65, 1, 64, 1, True, True, 0.0),
    (65, 3, 8, 8, True, False, 0.6), (700, 1, 64, 3, True, True, 0.6), (700, 3, 33, 1, False, True, 0.0), (700, 1, 8, 8, False, False, 0.6),
    (32, 1, 33, 1, True, True, 0.0), (31, 1, 64, 8, True, False, 0.6), (65, 3, 64, 3, False, True, 0.6), (700, 3, 64, 1, True, False, 0.6),
]


@pytest.mark.parametrize("n,F,H,C,bias,sum_features,p", BACKWARD_CASES)
def test_backward_on_the_matrix_cores_vs_oracle_autograd(n, F, H, C, bias, sum_features, p):
    """gnan_fmlp_bwd_mfma == oracle autograd with the same masks (assert_grads_rule), agrees with gnan_fmlp_bwd under the same
    rule (another order of summation: not bit for bit), gives the same bits twice, and writes nothing but its outputs."""
    sd = _mlp_state(F, 3, H, C, bias, seed=F + H + C)
    st = _stack(sd, F, 3, H, C, bias)
    x, gup = _inputs(n, F, C, sum_features)
    got, need = _backward(x, st, gup, sum_features, p)
    assert (need > 0) == (n > 128)                         # node ranges of at least 128 nodes: 700 nodes are six of them
    _, want = _oracle(x, sd, _masks(n, F, 3, H) if p > 0 else None, p, sum_features, gup)
    want["w_mid"] = want["w_mid"][0]
    if bias:
        want["b_mid"] = want["b_mid"][0]
    shaped = {k: v.reshape(want[k].shape) for k, v in got.items()}
    assert set(shaped) == set(want)
    assert_grads_rule(shaped, want, None, ("mfma", n, F, H, C))
    lane, _ = _backward(x, st, gup, sum_features, p, mfma=False)
    assert_grads_rule(lane, {k: v.reshape(-1) for k, v in want.items()}, None, ("lane", n, F, H, C))
    assert_grads_rule(got, {k: v.double() for k, v in lane.items()}, None, ("mfma vs lane", n, F, H, C), floor=TWO_FLOORS)
    again, _ = _backward(x, st, gup, sum_features, p)
    assert all(torch.equal(again[k], got[k]) for k in got)
    if p > 0:
        other, _ = _backward(x, st, gup, sum_features, p, seed=SEED + 1)
        assert n * F * H < 64 or any(not torch.equal(other[k], got[k]) for k in got)


class _Spy:
    """Stands in for the loaded library: records (entry point, algo of its record if it has one) of every call."""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        fn = getattr(self.real, name)

        def call(*args):
            self.calls.append((name, getattr(args[0], "algo", None) if args else None))
            return fn(*args)
        return call

    def names(self):
        return [c[0] for c in self.calls]


def _spy(monkeypatch):
    from gnan_amd import _lib
    spy = _Spy(_lib.lib())
    monkeypatch.setattr(_lib, "lib", lambda: spy)
    return spy


def _module_call(st, x, gup, sum_features, x_grad=False):
    from gnan_amd.functional import feature_mlps_dropout
    leaves = [t for t in st[:6] if t is not None]
    for t in leaves:
        t.requires_grad_(True)
    xs = x.to(DEV).requires_grad_(x_grad)
    y = feature_mlps_dropout(xs, st, sum_features, P, seed=SEED)
    got = torch.autograd.grad(y, leaves + ([xs] if x_grad else []), gup.to(DEV))
    names = [nm for nm, t in zip(NAMES, st[:6]) if t is not None]
    return y.detach(), dict(zip(names, got[:len(names)]))


@pytest.mark.parametrize("sum_features", [False, True])
def test_module_level_routes_to_the_matrix_cores_when_switched_on(sum_features, monkeypatch):
    from gnan_amd import _lib, functional
    n, F, L, H, C = 300, 4, 3, 16, 2
    monkeypatch.setattr(functional, "DROPOUT_MFMA", True)
    monkeypatch.setattr(functional, "DROPOUT_MFMA_BACKWARD", True)
    monkeypatch.setattr(functional, "DROPOUT_MFMA_MIN_WORK", 1)
    sd = _mlp_state(F, L, H, C, True, seed=11)
    st = _stack(sd, F, L, H, C, True)
    x, gup = _inputs(n, F, C, sum_features)
    spy = _spy(monkeypatch)
    y, got = _module_call(st, x, gup, sum_features)
    assert ("gnan_fmlp_fwd", _lib.FMLP_MFMA) in spy.calls and "gnan_fmlp_bwd_mfma" in spy.names()
    assert "gnan_fmlp_bwd" not in spy.names() and ("gnan_fmlp_fwd", _lib.FMLP_LANE) not in spy.calls
    ref, want = _oracle(x, sd, _masks(n, F, L, H), P, sum_features, gup)
    assert O.rel_err(y.cpu(), ref) <= 1e-5
    assert_grads_rule(got, want, None, "module")


def test_module_level_as_shipped_keeps_the_lane_route_and_its_bits(monkeypatch):
    """(300, 4, 3, 16, 2) is far below DROPOUT_MFMA_MIN_WORK whatever the switches say: lane forward, gnan_fmlp_bwd, and the
    bits the commit before this feature gave (tests/golden/dropout_mfma_parent_bits.npz)."""
    from gnan_amd import _lib, functional
    monkeypatch.setattr(functional, "DROPOUT_MFMA", True)
    monkeypatch.setattr(functional, "DROPOUT_MFMA_BACKWARD", True)
    z = np.load(os.path.join(GOLDEN_DIR, "dropout_mfma_parent_bits.npz"))
    st = _golden_model(z, "lane")
    spy = _spy(monkeypatch)
    y, got = _module_call(st, torch.from_numpy(z["lane/x"]), torch.from_numpy(z["lane/gup"]), False)
    assert ("gnan_fmlp_fwd", _lib.FMLP_LANE) in spy.calls and "gnan_fmlp_bwd" in spy.names()
    assert "gnan_fmlp_bwd_mfma" not in spy.names() and ("gnan_fmlp_fwd", _lib.FMLP_MFMA) not in spy.calls
    assert torch.equal(y.cpu(), torch.from_numpy(z["lane/out"]))
    for nm, g in got.items():
        assert torch.equal(g.cpu(), torch.from_numpy(z[f"lane/d_{nm}"])), nm


@pytest.mark.parametrize("L,C,x_grad", [(3, 2, True), (3, 9, False), (4, 2, False)])
def test_module_level_backward_stays_where_it_was_outside_its_cover(L, C, x_grad, monkeypatch):
    from gnan_amd import _lib, functional
    n, F, H = 300, 4, 16
    monkeypatch.setattr(functional, "DROPOUT_MFMA", True)
    monkeypatch.setattr(functional, "DROPOUT_MFMA_BACKWARD", True)
    monkeypatch.setattr(functional, "DROPOUT_MFMA_MIN_WORK", 1)
    sd = _mlp_state(F, L, H, C, True, seed=5)
    st = _stack(sd, F, L, H, C, True)
    x, gup = _inputs(n, F, C, True)
    spy = _spy(monkeypatch)
    y, got = _module_call(st, x, gup, True, x_grad=x_grad)
    assert "gnan_fmlp_bwd_mfma" not in spy.names() and "gnan_fmlp_bwd" not in spy.names()      # the restatement, as before
    assert ("gnan_fmlp_fwd", _lib.FMLP_MFMA if C <= 8 else _lib.FMLP_LANE) in spy.calls
    ref, want = _oracle(x, sd, _masks(n, F, L, H), P, True, gup)
    assert O.rel_err(y.cpu(), ref) <= 1e-5
    assert_grads_rule(got, want, None, (L, C, x_grad))


def test_mask_window_is_a_row_range_of_the_mask():
    from gnan_amd.functional import dropout_mask_window
    F, LH, H = 3, 2, 16
    full = _masks(100, F, LH + 1, H)
    win = dropout_mask_window(SEED, P, 37, 50, F, LH, H, DEV).cpu()
    assert win.shape == (50, F, LH, H) and torch.equal(win, full[37:87])
    assert torch.equal(dropout_mask_window(SEED, P, 0, 100, F, LH, H, DEV).cpu(), full)
    assert dropout_mask_window(SEED, P, 37, 0, F, LH, H, DEV).numel() == 0


def test_restatement_backward_in_mask_windows_gives_the_unchunked_bits(monkeypatch):
    """C = 9 back-propagates through the batched restatement.  With the whole mask inside DROPOUT_MASK_MAX_ELEMS: the bits of the
    commit before this feature (golden).  With the budget lowered until the masks come in >= 4 windows: the same bits — and
    no refusal is left, however small the budget."""
    from gnan_amd import _lib, functional
    z = np.load(os.path.join(GOLDEN_DIR, "dropout_mfma_parent_bits.npz"))
    st = _golden_model(z, "wide")
    n, F, L, H = 500, st.F, st.L, st.H
    assert (n, F, L, H, st.C) == (500, 3, 3, 16, 9)
    x, gup = torch.from_numpy(z["wide/x"]), torch.from_numpy(z["wide/gup"])
    real = _lib.lib()
    y, whole = _module_call(st, x, gup, True)
    assert torch.equal(y.cpu(), torch.from_numpy(z["wide/out"]))
    for nm, g in whole.items():
        assert torch.equal(g.cpu(), torch.from_numpy(z[f"wide/d_{nm}"])), nm
    per_node = F * (L - 1) * H
    for budget in (n * per_node // 4, per_node, 1):
        monkeypatch.setattr(functional, "DROPOUT_MASK_MAX_ELEMS", budget)
        spy = _Spy(real)
        monkeypatch.setattr(_lib, "lib", lambda spy=spy: spy)
        _, cut = _module_call(st, x, gup, True)
        windows = spy.names().count("gnan_dropout_mask_window")
        assert windows >= 4 * 2 * (L - 1) and "gnan_dropout_mask" not in spy.names(), (budget, windows)   # per layer, forward + backward
        for nm, g in cut.items():
            assert torch.equal(g, whole[nm]), (budget, nm)
