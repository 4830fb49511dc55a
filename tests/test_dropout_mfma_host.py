"""Host side of training-mode Dropout on the matrix cores: gnan_fmlp_bwd_mfma, its workspace query and
gnan_dropout_mask_window — declared, exported and bound under ABI 51; the refusals, which all happen on the host before any
HIP call; the workspace sizes; and functional's routing predicate.  None of this needs a GPU."""
import ctypes
import os
import re

import pytest

from gnan_amd import _lib, functional
from conftest import ROOT

PTR = 0x1000          # a non-NULL "device" address: no refusal under test ever follows it


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gnan_hip.h")).read(), flags=re.S)


def _bwd(n=1000, F=3, L=3, H=16, C=2, p=0.6, bias=True, **more):
    b = PTR if bias else None
    kw = dict(x=PTR, n=n, x_stride=F, F=F, L=L, H=H, C=C, w_first=PTR, b_first=b, w_mid=PTR, b_mid=b, w_last=PTR, b_last=b,
              sum_features=0, grad=PTR, grad_stride=F * C, d_w_first=PTR, d_b_first=b, d_w_mid=PTR, d_b_mid=b, d_w_last=PTR,
              d_b_last=b, dropout_p=p, dropout_seed=7)
    kw.update(more)
    return _lib.FmlpBwdArgs(**kw)


def _fwd(n=1000, F=3, L=3, H=16, C=2, p=0.6, algo=_lib.FMLP_MFMA, sum_features=0):
    return _lib.FmlpArgs(x=PTR, n=n, x_stride=F, F=F, L=L, H=H, C=C, w_first=PTR, b_first=PTR, w_mid=PTR, b_mid=PTR, w_last=PTR,
                         b_last=PTR, sum_features=sum_features, out=PTR, out_stride=C if sum_features else F * C, algo=algo,
                         dropout_p=p, dropout_seed=7)


def test_the_three_entry_points_are_declared_exported_and_bound_under_abi_51():
    text = _header()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    assert _lib.ABI_VERSION == 51 and handle.gnan_abi_version() == 51
    assert re.search(r"\bint gnan_fmlp_bwd_mfma\(const gnan_fmlp_bwd_args\* a, gnan_stream_t stream\);", text)
    assert re.search(r"\bsize_t gnan_fmlp_bwd_mfma_workspace_bytes\(const gnan_fmlp_bwd_args\* a\);", text)
    assert re.search(r"\bint gnan_dropout_mask_window\(uint64_t seed, float p, int64_t node_lo, int64_t n_nodes, int32_t F, "
                     r"int32_t n_hidden_layers,\s+int32_t H, uint8_t\* mask, gnan_stream_t stream\);", text)
    want = {
        "gnan_fmlp_bwd_mfma": (ctypes.c_int, [ctypes.POINTER(_lib.FmlpBwdArgs), ctypes.c_void_p]),
        "gnan_fmlp_bwd_mfma_workspace_bytes": (ctypes.c_size_t, [ctypes.POINTER(_lib.FmlpBwdArgs)]),
        "gnan_dropout_mask_window": (ctypes.c_int, [ctypes.c_uint64, ctypes.c_float, ctypes.c_int64, ctypes.c_int64, ctypes.c_int32,
                                                    ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]),
    }
    for name, (res, argtypes) in want.items():
        assert hasattr(handle, name), name
        assert _lib.SYMBOLS[name] == (res, argtypes), name
        fn = getattr(_lib.lib(), name)
        assert fn.restype is res and fn.argtypes == argtypes, name
    # the record both backward kernels take did not change
    assert _lib.SYMBOLS["gnan_fmlp_bwd"][1] == _lib.SYMBOLS["gnan_fmlp_bwd_mfma"][1]


def test_the_backward_refuses_in_the_order_of_gnan_fmlp_bwd_before_any_hip_call():
    lib = _lib.lib()
    fn = lib.gnan_fmlp_bwd_mfma
    said = lambda: lib.gnan_last_error()                       # noqa: E731
    assert fn(None, None) == _lib.ERR_BAD_ARG and said() == b"fmlp_bwd_mfma: null args"
    # bad sizes come before the cover, the cover before every pointer
    assert fn(_bwd(n=-1, L=2), None) == _lib.ERR_BAD_ARG and said() == b"fmlp_bwd_mfma: bad sizes"
    assert fn(_bwd(F=0, H=65), None) == _lib.ERR_BAD_ARG and said() == b"fmlp_bwd_mfma: bad sizes"
    for kw in (dict(L=2), dict(L=4), dict(H=65), dict(C=9), dict(H=0), dict(C=0)):
        a = _bwd(w_first=None, d_b_first=None, dropout_p=1.0, **kw)         # (later refusals' causes are there too: the cover wins)
        assert fn(a, None) == _lib.ERR_UNSUPPORTED, kw
        assert said() == b"fmlp_bwd_mfma: covers L == 3, H <= 64, C <= 8 (got L=%d H=%d C=%d)" % (a.L, a.H, a.C), kw
    for kw in (dict(w_first=None), dict(w_last=None), dict(d_w_first=None), dict(d_w_last=None)):
        assert fn(_bwd(w_mid=None, **kw), None) == _lib.ERR_BAD_ARG and said() == b"fmlp_bwd_mfma: null weight / gradient pointer", kw
    for kw in (dict(w_mid=None), dict(d_w_mid=None)):
        assert fn(_bwd(d_b_last=None, **kw), None) == _lib.ERR_BAD_ARG and said() == b"fmlp_bwd_mfma: L == 3 needs w_mid and d_w_mid", kw
    # a bias gradient without its bias, a bias without its gradient
    for kw in (dict(b_first=None), dict(d_b_first=None), dict(b_mid=None), dict(d_b_mid=None), dict(b_last=None), dict(d_b_last=None)):
        assert fn(_bwd(x=None, **kw), None) == _lib.ERR_BAD_ARG, kw
        assert said() == b"fmlp_bwd_mfma: a bias gradient is wanted exactly where there is a bias", kw
    for kw in (dict(x=None), dict(grad=None), dict(x_stride=2), dict(grad_stride=5)):
        assert fn(_bwd(dropout_p=1.0, **kw), None) == _lib.ERR_BAD_ARG and said() == b"fmlp_bwd_mfma: bad x / grad", kw
    for p in (1.0, 1.5, -0.25, float("nan")):
        assert fn(_bwd(p=p), None) == _lib.ERR_BAD_ARG and said() == b"fmlp_bwd_mfma: dropout_p must be in [0, 1)", p
    # everything in order but the workspace of a batch that is cut into node ranges: the last refusal, still no launch
    a = _bwd()
    assert lib.gnan_fmlp_bwd_mfma_workspace_bytes(a) > 0
    assert fn(a, None) == _lib.ERR_WORKSPACE and said().startswith(b"fmlp_bwd_mfma: workspace 0 B < required ")


def test_the_forward_under_dropout_keeps_auto_and_lane_and_opens_mfma_inside_its_cover():
    lib = _lib.lib()
    for sum_features in (0, 1):
        for algo in (_lib.FMLP_AUTO, _lib.FMLP_LANE):
            assert lib.gnan_fmlp_fwd_workspace_bytes(_fwd(algo=algo, sum_features=sum_features)) == 0
        need = lib.gnan_fmlp_fwd_workspace_bytes(_fwd(sum_features=sum_features))
        assert need > 0
        # the packed weights (plus chunk partials): what the same shape needs without Dropout
        assert need == lib.gnan_fmlp_fwd_workspace_bytes(_fwd(p=0.0, sum_features=sum_features))
        assert need == lib.gnan_fmlp_fwd_workspace_bytes(_fwd(p=0.0, algo=_lib.FMLP_AUTO, sum_features=sum_features))
    assert lib.gnan_fmlp_fwd_workspace_bytes(_fwd(L=4, H=64, C=8)) > 0
    for kw in (dict(L=2), dict(L=5), dict(H=65), dict(C=9)):
        a = _fwd(**kw)
        assert lib.gnan_fmlp_fwd_workspace_bytes(a) == 0, kw
        assert lib.gnan_fmlp_fwd(a, None) == _lib.ERR_UNSUPPORTED, kw
        assert lib.gnan_last_error() == b"fmlp: MFMA path covers 3 <= L <= 4, H <= 64, C <= 8 (got L=%d H=%d C=%d)" % (a.L, a.H, a.C)
    # inside the cover the call now goes on to its workspace check (it used to be refused: "runs on the lane kernel")
    assert lib.gnan_fmlp_fwd(_fwd(), None) == _lib.ERR_WORKSPACE
    assert lib.gnan_last_error().startswith(b"fmlp: workspace 0 B < required ")
    assert lib.gnan_fmlp_fwd(_fwd(p=1.0), None) == _lib.ERR_BAD_ARG and b"dropout_p must be in [0, 1)" in lib.gnan_last_error()


def test_the_backward_workspace_grows_with_the_split_count_and_is_zero_for_no_nodes():
    lib = _lib.lib()
    q = lib.gnan_fmlp_bwd_mfma_workspace_bytes
    assert q(None) == 0 and q(_bwd(n=0)) == 0
    F, H, C = 3, 16, 2
    block = 4 * (2 * F * H + F * H * H + F * H + F * C * H + F * C)       # one node range's gradients, bytes
    sizes = [q(_bwd(n=n, F=F, H=H, C=C)) for n in (1, 128, 129, 256, 257, 700, 5000, 1 << 20, 1 << 24)]
    assert sizes[0] == sizes[1] == 0                                      # one range: straight into the outputs
    assert sizes == sorted(sizes)
    assert all(s % block == 0 for s in sizes)
    assert [s // block for s in sizes[2:6]] == [2, 2, 3, 6]              # ranges of at least 128 nodes (a tile per wave)
    assert sizes[-1] == sizes[-2] == block * ((512 + F - 1) // F)        # capped: enough workgroups to fill the chip
    assert q(_bwd(n=1 << 20, F=1000, H=H, C=C)) == 0                      # many features: one range each
    assert q(_bwd(L=2)) == 0 and q(_bwd(H=0)) == 0


def test_the_mask_window_refuses_bad_arguments_on_the_host():
    lib = _lib.lib()
    fn = lib.gnan_dropout_mask_window
    for args in ((1, 1.0, 0, 4, 2, 2, 8), (1, 0.5, -1, 4, 2, 2, 8), (1, 0.5, 0, -4, 2, 2, 8), (1, 0.5, 0, 4, 0, 2, 8),
                 (1, 0.5, 0, 4, 2, 0, 8), (1, 0.5, 0, 4, 2, 2, 0)):
        assert fn(*args, PTR, None) == _lib.ERR_BAD_ARG and lib.gnan_last_error() == b"dropout_mask_window: bad arguments", args
    assert fn(1, 0.5, 37, 0, 2, 2, 8, None, None) == 0               # no rows: nothing to write
    assert fn(1, 0.5, 37, 4, 2, 2, 8, None, None) == _lib.ERR_BAD_ARG and lib.gnan_last_error() == b"dropout_mask_window: null output"
    assert lib.gnan_dropout_mask(1, 1.0, 4, 2, 2, 8, PTR, None) == _lib.ERR_BAD_ARG
    assert lib.gnan_last_error() == b"dropout_mask: bad arguments"


def test_the_routing_predicate_over_the_covers_edges_and_the_clamp():
    route = functional.dropout_mfma_routes
    on = dict(forward_on=True, backward_on=True, min_work=1 << 16)
    n, F = 1 << 14, 4                                                       # n * F == the threshold
    assert route(n, F, 3, 64, 8, **on) == (True, True)
    assert route(n, F, 3, 1, 1, **on) == (True, True)
    assert route(n - 1, F, 3, 64, 8, **on) == (False, False)                # one node short of the threshold: lane route
    assert route(n, F, 4, 64, 8, **on) == (True, False)                     # L = 4: the forward's cover only
    assert route(n, F, 2, 64, 8, **on) == (False, False)
    assert route(n, F, 5, 64, 8, **on) == (False, False)
    assert route(n, F, 3, 65, 8, **on) == (False, False)
    assert route(n, F, 3, 64, 9, **on) == (False, False)
    assert route(n, F, 3, 64, 8, x_grad=True, **on) == (True, False)        # x.grad: the backward stays where it was
    assert route(n, F, 3, 64, 8, forward_on=False, backward_on=True, min_work=1) == (False, True)
    assert route(n, F, 3, 64, 8, forward_on=True, backward_on=False, min_work=1) == (True, False)
    assert route(1, 1, 3, 64, 8, forward_on=True, backward_on=True, min_work=1) == (True, True)
    # as shipped: the threshold never lies below the clamp, so no batch below 2^16 node-features leaves the lane route
    assert functional.DROPOUT_MFMA_CLAMP == 1 << 16
    assert functional.DROPOUT_MFMA_MIN_WORK >= functional.DROPOUT_MFMA_CLAMP
    assert route(700, 6, 3, 64, 7, forward_on=True, backward_on=True) == (False, False)
    assert route((1 << 16) - 1, 1, 3, 64, 1, forward_on=True, backward_on=True) == (False, False)
    assert isinstance(functional.DROPOUT_MFMA, bool) and isinstance(functional.DROPOUT_MFMA_BACKWARD, bool)
    assert route(1 << 20, 64, 3, 64, 1) == (functional.DROPOUT_MFMA, functional.DROPOUT_MFMA_BACKWARD)
    assert functional.DROPOUT_MASK_MAX_ELEMS == 1 << 31
