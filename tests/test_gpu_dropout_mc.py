"""Many output channels (9 <= C <= 64) on the matrix cores: gnan_fmlp_mc_fwd, gnan_fmlp_mc_bwd (csrc/fmlp_mc.hip) and their
routing in functional._DropoutMLPs — against the oracle's float64 Linear / ReLU / Dropout chain fed with the masks
gnan_dropout_mask writes out (the scheme of tests/test_gpu_dropout_mfma.py), by the project's rule: rel_err <= 1e-5 on outputs,
helpers.assert_grads_rule on gradients; plus exact small-integer cases that pin the channel and unit mapping bit for bit."""
import pytest
import torch

from oracle import gnan_oracle as O
from helpers import TWO_FLOORS, assert_grads_rule

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


def _forward(x, st, sum_features, p=P, seed=SEED, x_pad=0, out_pad=0, entry="mc"):
    """gnan_fmlp_mc_fwd (``entry="mfma"``: gnan_fmlp_fwd with GNAN_FMLP_MFMA) called directly: ``x_pad`` / ``out_pad`` extra
    floats per row of x / out (strides beyond the widths); the sentinel past the output's width must come back intact."""
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
                      algo=_lib.FMLP_MFMA, dropout_p=p, dropout_seed=seed)
    lib = _lib.lib()
    need = lib.gnan_fmlp_mc_fwd_workspace_bytes(a) if entry == "mc" else lib.gnan_fmlp_fwd_workspace_bytes(a)
    ws = torch.full((max(need, 4) // 4,), float("nan"), device=DEV)
    a.workspace, a.workspace_bytes = _lib.ptr(ws), need
    if entry == "mc":
        _lib.check(lib.gnan_fmlp_mc_fwd(a, _lib.stream_of(xb)), "gnan_fmlp_mc_fwd")
    else:
        _lib.check(lib.gnan_fmlp_fwd(a, _lib.stream_of(xb)), "gnan_fmlp_fwd")
    torch.cuda.synchronize()
    if out_pad:
        assert bool((out[:, width:] == -77.0).all())                  # nothing is written past the output's width
    return out[:, :width].contiguous()


FORWARD_CASES = [
    # (n, F, L, H, C, bias, sum_features, p).  C: one padded tile / a full tile / one channel in the second tile / the real
    # model / two full tiles.  n: one lane / a second tile / a second workgroup / ragged; n = 33, F = 5 also cuts feature chunks.
    (1, 1, 3, 8, 9, True, False, 0.6), (33, 5, 3, 33, 40, True, True, 0.6), (33, 5, 4, 64, 64, False, False, 0.6),
    (257, 2, 3, 64, 40, True, True, 0.6), (257, 5, 4, 33, 33, True, False, 0.0), (700, 1, 3, 64, 64, True, True, 0.6),
    (700, 2, 3, 8, 32, False, True, 0.6), (700, 5, 3, 33, 9, True, False, 0.6), (700, 2, 4, 64, 40, False, True, 0.0),
    (1, 5, 4, 8, 64, True, True, 0.6), (33, 1, 3, 64, 33, False, False, 0.6), (257, 1, 4, 64, 32, True, True, 0.6),
    (33, 2, 3, 64, 9, True, False, 0.0), (257, 5, 3, 8, 64, False, True, 0.6), (700, 1, 4, 33, 40, True, False, 0.6),
    (700, 5, 3, 64, 40, True, True, 0.6), (33, 5, 3, 64, 33, True, True, 0.0), (257, 2, 4, 64, 64, True, True, 0.6),
    (1, 2, 3, 33, 32, False, False, 0.6), (700, 2, 3, 64, 9, True, False, 0.6),
]


@pytest.mark.parametrize("n,F,L,H,C,bias,sum_features,p", FORWARD_CASES)
def test_forward_with_many_channels_vs_oracle(n, F, L, H, C, bias, sum_features, p):
    """gnan_fmlp_mc_fwd == the oracle with gnan_dropout_mask's masks (rel_err <= 1e-5): a wrong channel tile, K order or hash
    coordinate is an O(1) error."""
    sd = _mlp_state(F, L, H, C, bias, seed=F + L + H + C)
    st = _stack(sd, F, L, H, C, bias)
    x, _ = _inputs(n, F, C, sum_features)
    y = _forward(x, st, sum_features, p=p)
    ref, _ = _oracle(x, sd, _masks(n, F, L, H) if p > 0 else None, p, sum_features)
    err = O.rel_err(y.cpu(), ref)
    print(f"forward ({n}, {F}, {L}, {H}, {C}, p={p}): rel_err {err:.3e}")
    assert err <= 1e-5
    assert torch.equal(y, _forward(x, st, sum_features, p=p))                     # the same bits twice
    if p > 0:
        assert n * F * H < 64 or not torch.equal(y, _forward(x, st, sum_features, p=p, seed=SEED + 1))


@pytest.mark.parametrize("L,H,sum_features", [(3, 64, False), (4, 33, True)])
def test_forward_at_eight_channels_agrees_with_the_lane_dot_product_kernel(L, H, sum_features):
    n, F, C = 257, 5, 8
    sd = _mlp_state(F, L, H, C, True, seed=21)
    st = _stack(sd, F, L, H, C, True)
    x, _ = _inputs(n, F, C, sum_features)
    ref, _ = _oracle(x, sd, _masks(n, F, L, H), P, sum_features)
    mc, mfma = _forward(x, st, sum_features), _forward(x, st, sum_features, entry="mfma")
    assert O.rel_err(mc.cpu(), ref) <= 1e-5 and O.rel_err(mfma.cpu(), ref) <= 1e-5
    assert O.rel_err(mc.cpu(), mfma.double().cpu()) <= TWO_FLOORS


@pytest.mark.parametrize("x_pad,out_pad,C,sum_features", [(3, 0, 40, False), (0, 5, 40, False), (0, 4, 40, True), (2, 3, 33, True),
                                                          (0, 8, 64, False)])
def test_forward_row_strides_beyond_the_widths(x_pad, out_pad, C, sum_features):
    """Strides beyond the widths give the same bits (16-byte stores where C, stride and base allow, dwords otherwise), and the
    sentinel past the output's width is intact."""
    n, F, L, H = 257, 5, 3, 33
    sd = _mlp_state(F, L, H, C, True, seed=3)
    st = _stack(sd, F, L, H, C, True)
    x, _ = _inputs(n, F, C, sum_features)
    y = _forward(x, st, sum_features, x_pad=x_pad, out_pad=out_pad)
    assert torch.equal(y, _forward(x, st, sum_features))
    ref, _ = _oracle(x, sd, _masks(n, F, L, H), P, sum_features)
    assert O.rel_err(y.cpu(), ref) <= 1e-5


def _backward(x, st, gup, sum_features, p, seed=SEED, entry="mc", grad_pad=0):
    """gnan_fmlp_mc_bwd (``entry="mfma"``: gnan_fmlp_bwd_mfma) called directly; the six outputs are cut from ONE buffer with
    guard floats between them, which must come back untouched.  ``grad_pad``: extra floats per row of grad."""
    from gnan_amd import _lib
    F, H, C = st.F, st.H, st.C
    xd = x.to(DEV).contiguous()
    g = torch.full((gup.shape[0], gup.shape[1] + grad_pad), 1e30, device=DEV)
    g[:, :gup.shape[1]] = gup.to(DEV)
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
    need = lib.gnan_fmlp_mc_bwd_workspace_bytes(a) if entry == "mc" else lib.gnan_fmlp_bwd_mfma_workspace_bytes(a)
    ws = torch.full((max(need, 4) // 4,), float("nan"), device=DEV)
    a.workspace, a.workspace_bytes = _lib.ptr(ws), need
    if entry == "mc":
        _lib.check(lib.gnan_fmlp_mc_bwd(a, _lib.stream_of(xd)), "gnan_fmlp_mc_bwd")
    else:
        _lib.check(lib.gnan_fmlp_bwd_mfma(a, _lib.stream_of(xd)), "gnan_fmlp_bwd_mfma")
    torch.cuda.synchronize()
    written = torch.zeros_like(buf, dtype=torch.bool)
    for o in outs:
        if o is not None:
            written[o.storage_offset():o.storage_offset() + o.numel()] = True
    assert bool((buf[~written] == -77.0).all())            # guards, and the slots of absent biases: untouched
    return {nm: o.clone() for nm, o in zip(NAMES, outs) if o is not None}, need


def _want_l3(want, bias):
    want = dict(want)
    want["w_mid"] = want["w_mid"][0]
    if bias:
        want["b_mid"] = want["b_mid"][0]
    return want


BACKWARD_CASES = [
    # (n, F, H, C, bias, sum_features, p); n = 257 with F = 1: three node ranges, hence the reduce kernel
    (1, 1, 8, 9, True, False, 0.6), (33, 3, 33, 40, True, True, 0.6), (33, 3, 64, 64, False, False, 0.6),
    (257, 1, 64, 40, True, True, 0.6), (257, 1, 8, 33, True, False, 0.0), (700, 1, 64, 64, True, True, 0.6),
    (700, 3, 33, 32, False, True, 0.6), (700, 1, 8, 9, False, False, 0.6), (33, 1, 33, 9, True, True, 0.0),
    (1, 3, 64, 33, True, False, 0.6), (257, 3, 64, 32, False, True, 0.0), (700, 3, 64, 40, True, False, 0.6),
    (257, 1, 64, 9, True, False, 0.6), (700, 1, 33, 64, True, True, 0.0),
]


@pytest.mark.parametrize("n,F,H,C,bias,sum_features,p", BACKWARD_CASES)
def test_backward_with_many_channels_vs_oracle_autograd(n, F, H, C, bias, sum_features, p):
    """gnan_fmlp_mc_bwd == oracle autograd with the same masks (assert_grads_rule), gives the same bits twice (with several
    node ranges too), and writes nothing but its outputs."""
    sd = _mlp_state(F, 3, H, C, bias, seed=F + H + C)
    st = _stack(sd, F, 3, H, C, bias)
    x, gup = _inputs(n, F, C, sum_features)
    got, need = _backward(x, st, gup, sum_features, p)
    assert (need > 0) == (n > 128)                         # node ranges of at least 128 nodes
    _, want = _oracle(x, sd, _masks(n, F, 3, H) if p > 0 else None, p, sum_features, gup)
    want = _want_l3(want, bias)
    shaped = {k: v.reshape(want[k].shape) for k, v in got.items()}
    assert set(shaped) == set(want)
    assert_grads_rule(shaped, want, None, ("mc", n, F, H, C))
    again, _ = _backward(x, st, gup, sum_features, p)
    assert all(torch.equal(again[k], got[k]) for k in got)
    if p > 0:
        other, _ = _backward(x, st, gup, sum_features, p, seed=SEED + 1)
        assert n * F * H < 64 or any(not torch.equal(other[k], got[k]) for k in got)


@pytest.mark.parametrize("H,sum_features,p", [(64, False, 0.6), (33, True, 0.6), (64, True, 0.0)])
def test_backward_at_eight_channels_agrees_with_the_lane_dot_product_kernel(H, sum_features, p):
    n, F, C = 700, 3, 8
    sd = _mlp_state(F, 3, H, C, True, seed=31)
    st = _stack(sd, F, 3, H, C, True)
    x, gup = _inputs(n, F, C, sum_features)
    _, want = _oracle(x, sd, _masks(n, F, 3, H) if p > 0 else None, p, sum_features, gup)
    want = {k: v.reshape(-1) for k, v in _want_l3(want, True).items()}
    mc, _ = _backward(x, st, gup, sum_features, p)
    mfma, _ = _backward(x, st, gup, sum_features, p, entry="mfma")
    assert_grads_rule(mc, want, None, "mc")
    assert_grads_rule(mfma, want, None, "mfma")
    assert_grads_rule(mc, {k: v.double() for k, v in mfma.items()}, None, "mc vs mfma", floor=TWO_FLOORS)


@pytest.mark.parametrize("C,sum_features", [(40, False), (33, True)])
def test_backward_grad_stride_beyond_the_width(C, sum_features):
    n, F, H = 257, 2, 33
    sd = _mlp_state(F, 3, H, C, True, seed=7)
    st = _stack(sd, F, 3, H, C, True)
    x, gup = _inputs(n, F, C, sum_features)
    a, _ = _backward(x, st, gup, sum_features, P)
    b, _ = _backward(x, st, gup, sum_features, P, grad_pad=5)
    assert all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("H,C", [(64, 64), (33, 40)])
@pytest.mark.parametrize("sum_features", [False, True])
def test_channel_and_unit_mapping_exact(H, C, sum_features):
    """p = 0 and small integers, so that every product and sum is exact in float32: x in {0, 1, 2}, w1 = 1, b1 = 0, W2 = I,
    W3[c, j] = (c + 1) [j == c mod H], integer grad.  Then h1 = h2 = x in every unit, out[n, k, c] = (c + 1) x[n, k], and with
    G[k, c] = sum_n g[n, k, c], GX[k, c] = sum_n g[n, k, c] x[n, k]:
      d_w_last[k, c, j] = GX[k, c] for every j (all units carry x), d_b_last[k, c] = G[k, c],
      dh2[n, j] = sum over c with c mod H == j of (c + 1) g[n, k, c], masked by x > 0, and d_w_mid[k, j, i] = sum_n dh2[n, j] x[n, k].
    Compared bit for bit with int64 arithmetic: a swapped channel tile, a wrong drow or K order, or a padded channel leaking in
    is an O(1) error."""
    from gnan_amd.functional import StackedMLP
    n, F = 257, 2
    gen = torch.Generator().manual_seed(5)
    x = torch.randint(0, 3, (n, F), generator=gen)
    g = torch.randint(-2, 3, (n, C if sum_features else F * C), generator=gen)
    w3 = torch.zeros(C, H, dtype=torch.int64)
    w3[torch.arange(C), torch.arange(C) % H] = torch.arange(C) + 1
    st = StackedMLP(torch.ones(F, H, device=DEV), torch.zeros(F, H, device=DEV),
                    torch.eye(H).expand(1, F, H, H).contiguous().to(DEV), torch.zeros(1, F, H, device=DEV),
                    w3.float().expand(F, C, H).contiguous().to(DEV), torch.zeros(F, C, device=DEV), 3, H, C, F)
    chan = torch.arange(C) + 1
    fx = x[:, :, None] * chan                                                   # [n, F, C]
    want_out = fx.sum(1) if sum_features else fx.reshape(n, F * C)
    y = _forward(x.float(), st, sum_features, p=0.0)
    assert torch.equal(y.cpu().double(), want_out.double())
    g3 = g[:, None, :].expand(n, F, C) if sum_features else g.reshape(n, F, C)   # [n, F, C]
    got, _ = _backward(x.float(), st, g.float(), sum_features, 0.0)
    G = g3.sum(0)
    GX = (g3 * x[:, :, None]).sum(0)                                            # [F, C]
    assert torch.equal(got["b_last"].cpu().double().reshape(F, C), G.double())
    assert torch.equal(got["w_last"].cpu().double().reshape(F, C, H), GX[:, :, None].expand(F, C, H).double())
    dh2 = torch.einsum("nkc,cj->nkj", g3, w3) * (x > 0)[:, :, None]              # [n, F, H]
    want_mid = torch.einsum("nkj,nk->kj", dh2, x)[:, :, None].expand(F, H, H)   # every input unit i carries x
    assert torch.equal(got["w_mid"].cpu().double().reshape(F, H, H), want_mid.double())
    assert torch.equal(got["b_mid"].cpu().double().reshape(F, H), dh2.sum(0).double())


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


def _switch_on(monkeypatch, min_work=None):
    from gnan_amd import functional
    monkeypatch.setattr(functional, "DROPOUT_MC", True)
    monkeypatch.setattr(functional, "DROPOUT_MC_BACKWARD", True)
    if min_work is not None:
        monkeypatch.setattr(functional, "DROPOUT_MC_MIN_WORK", min_work)


@pytest.mark.parametrize("n,F,L,H,C", [(300, 4, 3, 16, 9), (257, 2, 3, 64, 40)])
@pytest.mark.parametrize("sum_features", [False, True])
def test_module_level_routes_to_the_many_channel_kernels_when_switched_on(n, F, L, H, C, sum_features, monkeypatch):
    _switch_on(monkeypatch, 1)
    sd = _mlp_state(F, L, H, C, True, seed=11)
    st = _stack(sd, F, L, H, C, True)
    x, gup = _inputs(n, F, C, sum_features)
    spy = _spy(monkeypatch)
    y, got = _module_call(st, x, gup, sum_features)
    assert "gnan_fmlp_mc_fwd" in spy.names() and "gnan_fmlp_mc_bwd" in spy.names()
    assert "gnan_fmlp_fwd" not in spy.names() and "gnan_fmlp_bwd" not in spy.names() and "gnan_fmlp_bwd_mfma" not in spy.names()
    assert not any(nm.startswith("gnan_dropout_mask") for nm in spy.names())        # no mask tensor is drawn
    ref, want = _oracle(x, sd, _masks(n, F, L, H), P, sum_features, gup)
    assert O.rel_err(y.cpu(), ref) <= 1e-5
    assert_grads_rule(got, want, None, "module")


@pytest.mark.parametrize("L,x_grad", [(3, True), (4, False)])
def test_module_level_backward_stays_the_restatement_outside_its_cover(L, x_grad, monkeypatch):
    from gnan_amd import _lib
    n, F, H, C = 300, 4, 16, 9
    _switch_on(monkeypatch, 1)
    sd = _mlp_state(F, L, H, C, True, seed=5)
    st = _stack(sd, F, L, H, C, True)
    x, gup = _inputs(n, F, C, True)
    spy = _spy(monkeypatch)
    y, got = _module_call(st, x, gup, True, x_grad=x_grad)
    assert "gnan_fmlp_mc_fwd" in spy.names()                                       # the forward's cover holds both
    assert not any(nm in spy.names() for nm in ("gnan_fmlp_mc_bwd", "gnan_fmlp_bwd_mfma", "gnan_fmlp_bwd"))
    assert any(nm.startswith("gnan_dropout_mask") for nm in spy.names())           # the restatement draws its masks, as before
    ref, want = _oracle(x, sd, _masks(n, F, L, H), P, True, gup)
    assert O.rel_err(y.cpu(), ref) <= 1e-5
    assert_grads_rule(got, want, None, (L, x_grad))


def test_module_level_as_shipped_keeps_todays_calls_below_the_threshold(monkeypatch):
    """(300, 4, 3, 16, 9) is far below DROPOUT_MC_MIN_WORK whatever the switches say: lane forward and the restatement."""
    from gnan_amd import _lib
    _switch_on(monkeypatch)
    n, F, L, H, C = 300, 4, 3, 16, 9
    sd = _mlp_state(F, L, H, C, True, seed=11)
    st = _stack(sd, F, L, H, C, True)
    x, gup = _inputs(n, F, C, True)
    spy = _spy(monkeypatch)
    y, got = _module_call(st, x, gup, True)
    assert ("gnan_fmlp_fwd", _lib.FMLP_LANE) in spy.calls and "gnan_dropout_mask" in spy.names()
    assert not any(nm.startswith("gnan_fmlp_mc") for nm in spy.names())
    ref, want = _oracle(x, sd, _masks(n, F, L, H), P, True, gup)
    assert O.rel_err(y.cpu(), ref) <= 1e-5
    assert_grads_rule(got, want, None, "as shipped")


def test_module_level_at_the_shipped_threshold_takes_the_new_route(monkeypatch):
    """n * F == DROPOUT_MC_MIN_WORK as the module holds it (F = 128, H = 16, C = 9), only the switches forced on: the new
    entry points, within the rule."""
    from gnan_amd import functional
    _switch_on(monkeypatch)
    F, L, H, C = 128, 3, 16, 9
    n = functional.DROPOUT_MC_MIN_WORK // F
    assert n * F == functional.DROPOUT_MC_MIN_WORK >= 1 << 16
    sd = _mlp_state(F, L, H, C, True, seed=13)
    st = _stack(sd, F, L, H, C, True)
    x, gup = _inputs(n, F, C, True)
    spy = _spy(monkeypatch)
    y, got = _module_call(st, x, gup, True)
    assert "gnan_fmlp_mc_fwd" in spy.names() and "gnan_fmlp_mc_bwd" in spy.names()
    assert "gnan_fmlp_fwd" not in spy.names() and not any(nm.startswith("gnan_dropout_mask") for nm in spy.names())
    ref, want = _oracle(x, sd, _masks(n, F, L, H), P, True, gup)
    assert O.rel_err(y.cpu(), ref) <= 1e-5
    assert_grads_rule(got, want, None, "at the threshold")
