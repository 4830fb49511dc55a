"""The DIRECT shape-function kernels element by element against the float64 reference of tests/mlp_ref.py, on the case matrix of
tests/mlp_cases.py: ``fmlp_lane_kernel``, ``fmlp_point_kernel``, ``fmlp_mfma_kernel`` (csrc/fmlp.hip), ``fmlp_mc_fwd_kernel`` /
``fmlp_mc_bwd_kernel`` (csrc/fmlp_mc.hip), ``fmlp_bwd_kernel`` (csrc/fmlp_bwd.hip) and ``fmlp_bwd_mfma_kernel``
(csrc/fmlp_bwd_mfma.hip).  Every element of the outputs and of all six gradient tensors inside its own bound with the route's
counted ``k``, exact zeros where the bound is zero, the sentinel padding of strided rows untouched, the same bits twice, the
exact family bit for bit on every route (the matrix cores included), powers of two moving the exponent only, and clean
``GNAN_ERR_UNSUPPORTED`` refusals that write nothing outside the covers.

The routes are called by name: ``functional._fmlp_launch`` with ``algo = FMLP_LANE`` / ``FMLP_MFMA``, the AUTO point route at
``n F <= 64``, ``mc=True`` for ``gnan_fmlp_mc_fwd``; ``functional._fmlp_backward_launch`` plain, ``mfma=True`` and ``mc=True``; the
strided cases and the refusals build the records directly (the pattern of test_gpu_dropout_mfma._forward).  The Dropout mask is
``functional.dropout_masks``' (asserted equal to the cases' restatement of the hash) and goes to the reference as an input."""
import numpy as np
import pytest
import torch

import mlp_cases as MC
import mlp_ref as M

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -77.0
WORST = {}            # (direction, route, dropout) -> (ratio, case)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")


@pytest.fixture(scope="module", autouse=True)
def _worst_ratios():
    """The worst ``|err| / bound`` per direction, route and Dropout of whatever ran, printed once at the end (DESIGN.md section 8 records
    them; tests/test_mlp_bound.py asserts that the case list exercises every route both ways)."""
    yield
    for key in sorted(WORST):
        print(f"MLP-ELEMENTS worst {key[0]} route={key[1]} dropout={key[2]} ratio={WORST[key][0]:.4f} case={WORST[key][1]}")


def _note(direction, route, drop, ratio, name):
    key = (direction, route, bool(drop))
    if key not in WORST or ratio > WORST[key][0]:
        WORST[key] = (ratio, name)


def _stacked(c):
    from gnan_amd.functional import StackedMLP
    return StackedMLP(*[None if t is None else t.to(DEV) for t in c.params[:6]], *c.params[6:])


def _keep(c):
    """The library's keep-mask of the case (None without Dropout), asserted equal to the restated hash."""
    if not c.spec.p:
        return None
    from gnan_amd.functional import dropout_masks
    s = c.spec
    m = dropout_masks(MC.DROP_SEED, s.p, s.n, s.F, s.L - 1, s.H, DEV).cpu().numpy()
    assert np.array_equal(m, c.keep), "mlp_cases.keep_mask restates gnan_dropout_mask"
    return m


def _algo(route):
    from gnan_amd import _lib
    return {"lane": _lib.FMLP_LANE, "point": _lib.FMLP_AUTO, "mfma": _lib.FMLP_MFMA, "mc": _lib.FMLP_AUTO}[route]


def _padded(a: np.ndarray, pad: int, fill: float):
    t = torch.full((a.shape[0], a.shape[1] + pad), fill, device=DEV)
    t[:, :a.shape[1]] = torch.from_numpy(a).to(DEV)
    return t


def _forward_record(c, route, pads=(0, 0, 0)):
    """``gnan_fmlp_fwd`` / ``gnan_fmlp_mc_fwd`` through a record built here: ``(rc, out with its padding, x with its padding)``."""
    from gnan_amd import _lib
    s = c.spec
    st = _stacked(c)
    xb = _padded(c.x, pads[0], 7.0)
    width = s.C if s.sum_features else s.F * s.C
    out = torch.full((s.n, width + pads[1]), SENTINEL, device=DEV)
    a = _lib.FmlpArgs(x=_lib.ptr(xb), n=s.n, x_stride=xb.stride(0), F=s.F, L=s.L, H=s.H, C=s.C, w_first=_lib.ptr(st.w_first),
                      b_first=_lib.ptr(st.b_first), w_mid=_lib.ptr(st.w_mid), b_mid=_lib.ptr(st.b_mid), w_last=_lib.ptr(st.w_last),
                      b_last=_lib.ptr(st.b_last), sum_features=int(s.sum_features), out=_lib.ptr(out), out_stride=out.stride(0),
                      algo=_algo(route), dropout_p=s.p, dropout_seed=MC.DROP_SEED if s.p else 0)
    lib = _lib.lib()
    entry = "gnan_fmlp_mc_fwd" if route == "mc" else "gnan_fmlp_fwd"
    need = getattr(lib, entry + "_workspace_bytes")(a)
    ws = torch.empty(max(need, 16) // 4, dtype=torch.float32, device=DEV)
    a.workspace, a.workspace_bytes = _lib.ptr(ws), need
    rc = getattr(lib, entry)(a, _lib.stream_of(xb))
    torch.cuda.synchronize()
    return rc, out.cpu().numpy(), xb.cpu().numpy()


def _forward(c, route):
    """The route's output as float32 numpy ``[n, width]``: twice, the same bits; strided rows keep their sentinels."""
    from gnan_amd import functional
    s = c.spec
    width = s.C if s.sum_features else s.F * s.C
    runs = []
    for _ in range(2):
        if any(s.pads):
            rc, out, xb = _forward_record(c, route, s.pads)
            assert rc == 0, (c.name, route, rc)
            assert (out[:, width:] == SENTINEL).all() and (xb[:, s.F:] == 7.0).all(), "the padding is untouched"
            runs.append(out[:, :width].copy())
        else:
            y = functional._fmlp_launch(torch.from_numpy(c.x).to(DEV), _stacked(c), s.sum_features, _algo(route),
                                        (s.p, MC.DROP_SEED) if s.p else None, mc=route == "mc")
            torch.cuda.synchronize()
            runs.append(y.cpu().numpy())
    assert np.array_equal(runs[0].view(np.uint32), runs[1].view(np.uint32)), (c.name, route, "the same bits twice")
    return runs[0]


def _guarded(t):
    """A zero-size-safe output tensor of ``t``'s shape inside a sentinel buffer: ``(view, buffer)``."""
    buf = torch.full((t.numel() + 16,), SENTINEL, device=DEV)
    return buf[:t.numel()].view(t.shape), buf


def _backward_record(c, route, pads=(0, 0, 0)):
    """``gnan_fmlp_bwd`` / ``gnan_fmlp_bwd_mfma`` / ``gnan_fmlp_mc_bwd`` through a record built here, every output inside a sentinel
    buffer: ``(rc, outputs (None where absent), buffers, x and grad with their padding)``."""
    from gnan_amd import _lib
    s = c.spec
    st = _stacked(c)
    xb, gb = _padded(c.x, pads[0], 7.0), _padded(c.g, pads[2], 9.0)
    six = [st.w_first, st.b_first, None if st.w_mid is None else st.w_mid[0], None if st.b_mid is None else st.b_mid[0], st.w_last, st.b_last]
    outs, bufs = [], []
    for t in six:
        v, b = (None, None) if t is None else _guarded(t)
        outs.append(v)
        bufs.append(b)
    a = _lib.FmlpBwdArgs(x=_lib.ptr(xb), n=s.n, x_stride=xb.stride(0), F=s.F, L=s.L, H=s.H, C=s.C, w_first=_lib.ptr(six[0]),
                         b_first=_lib.ptr(six[1]), w_mid=_lib.ptr(six[2]), b_mid=_lib.ptr(six[3]), w_last=_lib.ptr(six[4]),
                         b_last=_lib.ptr(six[5]), sum_features=int(s.sum_features), grad=_lib.ptr(gb), grad_stride=gb.stride(0),
                         d_w_first=_lib.ptr(outs[0]), d_b_first=_lib.ptr(outs[1]), d_w_mid=_lib.ptr(outs[2]), d_b_mid=_lib.ptr(outs[3]),
                         d_w_last=_lib.ptr(outs[4]), d_b_last=_lib.ptr(outs[5]), dropout_p=s.p, dropout_seed=MC.DROP_SEED if s.p else 0)
    lib = _lib.lib()
    entry = {"lane": "gnan_fmlp_bwd", "mfma": "gnan_fmlp_bwd_mfma", "mc": "gnan_fmlp_mc_bwd"}[route]
    need = getattr(lib, entry + "_workspace_bytes")(a)
    ws = torch.empty(max(need, 16) // 4, dtype=torch.float32, device=DEV)
    a.workspace, a.workspace_bytes = _lib.ptr(ws), need
    rc = getattr(lib, entry)(a, _lib.stream_of(xb))
    torch.cuda.synchronize()
    return rc, outs, bufs, xb.cpu().numpy(), gb.cpu().numpy()


def _backward(c, route):
    """The route's six gradients by name (float32 numpy in the stacked tensors' shapes): twice, the same bits."""
    from gnan_amd import functional
    s = c.spec
    runs = []
    for _ in range(2):
        if any(s.pads):
            rc, outs, bufs, xb, gb = _backward_record(c, route, s.pads)
            assert rc == 0, (c.name, route, rc)
            assert (xb[:, s.F:] == 7.0).all() and (gb[:, c.g.shape[1]:] == 9.0).all(), "the padding is untouched"
            for v, b in zip(outs, bufs):
                assert b is None or bool((b[v.numel():] == SENTINEL).all()), "nothing is written behind a gradient tensor"
            got = M.grads_dict(outs)
            for nm in ("w_mid", "b_mid"):
                if nm in got:
                    got[nm] = got[nm][None]
        else:
            st = _stacked(c)
            outs = functional._fmlp_backward_launch(torch.from_numpy(c.x).to(DEV), list(st[:6]), torch.from_numpy(c.g).to(DEV), s.sum_features,
                                                    s.L, s.H, s.C, s.F, dropout=(s.p, MC.DROP_SEED) if s.p else None,
                                                    mfma=route == "mfma", mc=route == "mc")
            torch.cuda.synchronize()
            got = M.grads_dict(outs)
        runs.append(got)
    for nm in runs[0]:
        assert np.array_equal(runs[0][nm].view(np.uint32), runs[1][nm].view(np.uint32)), (c.name, route, nm, "the same bits twice")
    return runs[0]


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MC.ALL)
def test_every_output_element_is_inside_its_bound_on_every_forward_route(name):
    c = MC.case(name)
    s = c.spec
    routes = MC.fwd_routes(s)
    assert routes
    keep = _keep(c)
    for route in routes:
        got = _forward(c, route)
        ref = M.forward(c.net, c.x, s.sum_features, M.fwd_counts(route, s.n, s.F, s.L, s.H, s.C, s.sum_features), keep, s.p)
        ratio = M.assert_within(got, ref.truth, ref.bound, f"{name} forward {route}")
        print(f"MLP-ELEMENTS forward {name} route={route} ratio={ratio:.4f} zero_bounds={int((ref.bound == 0).sum())}")
        assert ratio <= 1.0, (name, route, ratio)
        _note("forward", route, s.p, ratio, name)
        if name in MC.EXACT:
            want = M.exact(c.net, c.x, s.sum_features, None, keep, s.p, MC.QW, MC.QX).out
            assert np.array_equal(got.astype(np.float64), want), (name, route, "bit for bit")


@pytest.mark.parametrize("name", MC.BACKWARD)
def test_every_gradient_element_is_inside_its_bound_on_every_backward_route(name):
    c = MC.case(name)
    s = c.spec
    routes = MC.bwd_routes(s)
    assert routes
    keep = _keep(c)
    if not s.family.startswith("exact"):
        assert M.forward(c.net, c.x, s.sum_features, M.DECIDE, keep, s.p).undecided == 0
    for route in routes:
        got = _backward(c, route)
        ref = M.backward(c.net, c.x, c.g, s.sum_features, M.bwd_counts(route, s.n, s.F, s.L, s.H, s.C, bool(s.p)), keep, s.p)
        ratio, where = M.hold_grads(got, ref, f"{name} backward {route}")
        zeros = sum(int((b == 0).sum()) for b in ref.bound.values())
        print(f"MLP-ELEMENTS backward {name} route={route} ratio={ratio:.4f} in={where} zero_bounds={zeros}")
        assert ratio <= 1.0, (name, route, ratio, where)
        _note("backward", route, s.p, ratio, name)
        if name in MC.EXACT:
            want = M.exact(c.net, c.x, s.sum_features, c.g, keep, s.p, MC.QW, MC.QX).grads
            for nm, a in got.items():
                assert np.array_equal(a.astype(np.float64), want[nm]), (name, route, nm, "bit for bit")


@pytest.mark.parametrize("name", MC.MOVED)
def test_power_of_two_scales_move_the_exponent_only(name):
    """The last layer times ``2^e`` and ``g`` times ``2^-e``: outputs times ``2^e``, ``d w_last`` / ``d b_last`` times ``2^-e``, the
    other four gradients bit for bit — on every route, inside the normal range."""
    c, unit = MC.case(name), MC.case(MC.base_of(name))
    e = c.spec.e
    for route in MC.fwd_routes(c.spec):
        assert np.array_equal(np.ldexp(_forward(unit, route), e), _forward(c, route)), (name, route)
    for route in MC.bwd_routes(c.spec):
        a, b = _backward(unit, route), _backward(c, route)
        for nm in a:
            assert np.array_equal(np.ldexp(a[nm], -e if nm in ("w_last", "b_last") else 0), b[nm]), (name, route, nm)
            nz = np.abs(b[nm][b[nm] != 0])
            assert nz.size == 0 or nz.min() >= 2.0 ** -126


FWD_REFUSED = [("random-n33-F2-L3-H32-C9-nobias-sum", "mfma"), ("random-n65-F6-L2-H64-C7", "mfma"), ("random-n65-F6-L2-H64-C7", "mc"),
               ("random-n65-F3-L5-H8-C2", "mfma"), ("random-n65-F3-L5-H8-C2", "mc"), ("random-n1-F1-L1-H0-C3", "mc"),
               ("random-n65-F2-L3-H64-C40-p0.6", "mfma")]
BWD_REFUSED = [("random-n65-F3-L3-H64-C40", "lane"), ("random-n65-F3-L3-H64-C40", "mfma"), ("random-n65-F6-L2-H64-C7", "mfma"),
               ("random-n65-F6-L2-H64-C7", "mc"), ("random-n33-F2-L3-H32-C9-nobias-sum", "lane")]


def test_routes_outside_their_cover_refuse_cleanly_and_write_nothing():
    from gnan_amd import _lib
    for name, route in FWD_REFUSED:
        c = MC.case(name)
        s = c.spec
        assert route not in MC.fwd_routes(s)
        rc, out, _ = _forward_record(c, route, (0, 2, 0))
        assert rc == _lib.ERR_UNSUPPORTED, (name, route, rc)
        assert (out == SENTINEL).all(), (name, route, "nothing is written")
    for name, route in BWD_REFUSED:
        c = MC.case(name)
        assert route not in MC.bwd_routes(c.spec)
        rc, outs, bufs, _, _ = _backward_record(c, route)
        assert rc == _lib.ERR_UNSUPPORTED, (name, route, rc)
        assert all(b is None or bool((b == SENTINEL).all()) for b in bufs), (name, route, "nothing is written")
