"""Host side of the many-channel matrix-core shape functions (9 <= C <= 64): gnan_fmlp_mc_fwd, gnan_fmlp_mc_bwd and their
workspace queries — declared, exported and bound under ABI 51; the refusals, which all happen on the host before any HIP
call, and their order; the workspace sizes; and functional's routing predicate.  None of this needs a GPU."""
import ctypes
import os
import re

from gnan_amd import _lib, functional
from conftest import ROOT

PTR = 0x1000          # a non-NULL "device" address: no refusal under test ever follows it
WS = 0x2000           # a 16-byte aligned "workspace"


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gnan_hip.h")).read(), flags=re.S)


def _bwd(n=1000, F=3, L=3, H=16, C=40, p=0.6, bias=True, **more):
    b = PTR if bias else None
    kw = dict(x=PTR, n=n, x_stride=F, F=F, L=L, H=H, C=C, w_first=PTR, b_first=b, w_mid=PTR, b_mid=b, w_last=PTR, b_last=b,
              sum_features=0, grad=PTR, grad_stride=F * C, d_w_first=PTR, d_b_first=b, d_w_mid=PTR, d_b_mid=b, d_w_last=PTR,
              d_b_last=b, dropout_p=p, dropout_seed=7)
    kw.update(more)
    return _lib.FmlpBwdArgs(**kw)


def _fwd(n=1000, F=3, L=3, H=16, C=40, p=0.6, sum_features=0, **more):
    kw = dict(x=PTR, n=n, x_stride=F, F=F, L=L, H=H, C=C, w_first=PTR, b_first=PTR, w_mid=PTR, b_mid=PTR, w_last=PTR,
              b_last=PTR, sum_features=sum_features, out=PTR, out_stride=C if sum_features else F * C, dropout_p=p, dropout_seed=7)
    kw.update(more)
    return _lib.FmlpArgs(**kw)


def test_the_four_entry_points_are_declared_exported_and_bound_under_abi_51():
    text = _header()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    assert _lib.ABI_VERSION == 51 and handle.gnan_abi_version() == 51
    assert re.search(r"\bint gnan_fmlp_mc_fwd\(const gnan_fmlp_args\* a, gnan_stream_t stream\);", text)
    assert re.search(r"\bsize_t gnan_fmlp_mc_fwd_workspace_bytes\(const gnan_fmlp_args\* a\);", text)
    assert re.search(r"\bint gnan_fmlp_mc_bwd\(const gnan_fmlp_bwd_args\* a, gnan_stream_t stream\);", text)
    assert re.search(r"\bsize_t gnan_fmlp_mc_bwd_workspace_bytes\(const gnan_fmlp_bwd_args\* a\);", text)
    want = {
        "gnan_fmlp_mc_fwd": (ctypes.c_int, [ctypes.POINTER(_lib.FmlpArgs), ctypes.c_void_p]),
        "gnan_fmlp_mc_fwd_workspace_bytes": (ctypes.c_size_t, [ctypes.POINTER(_lib.FmlpArgs)]),
        "gnan_fmlp_mc_bwd": (ctypes.c_int, [ctypes.POINTER(_lib.FmlpBwdArgs), ctypes.c_void_p]),
        "gnan_fmlp_mc_bwd_workspace_bytes": (ctypes.c_size_t, [ctypes.POINTER(_lib.FmlpBwdArgs)]),
    }
    for name, (res, argtypes) in want.items():
        assert hasattr(handle, name), name
        assert _lib.SYMBOLS[name] == (res, argtypes), name
        fn = getattr(_lib.lib(), name)
        assert fn.restype is res and fn.argtypes == argtypes, name
    # the records did not change: the new entry points take the existing ones
    assert _lib.SYMBOLS["gnan_fmlp_fwd"][1] == _lib.SYMBOLS["gnan_fmlp_mc_fwd"][1]
    assert _lib.SYMBOLS["gnan_fmlp_bwd_mfma"][1] == _lib.SYMBOLS["gnan_fmlp_mc_bwd"][1]


def test_the_forward_refuses_in_order_before_any_hip_call():
    lib = _lib.lib()
    fn = lib.gnan_fmlp_mc_fwd
    said = lambda: lib.gnan_last_error()                       # noqa: E731
    assert fn(None, None) == _lib.ERR_BAD_ARG and said() == b"fmlp_mc_fwd: null args"
    # bad sizes come before the cover, the cover before every pointer
    assert fn(_fwd(n=-1, L=2), None) == _lib.ERR_BAD_ARG and said() == b"fmlp_mc_fwd: bad sizes"
    assert fn(_fwd(F=0, H=65), None) == _lib.ERR_BAD_ARG and said() == b"fmlp_mc_fwd: bad sizes"
    for kw in (dict(L=2), dict(L=5), dict(H=65), dict(H=0), dict(C=0), dict(C=65)):
        a = _fwd(x=None, w_last=None, x_stride=1, p=1.0, **kw)     # (later refusals' causes are there too: the cover wins)
        assert fn(a, None) == _lib.ERR_UNSUPPORTED, kw
        assert said() == b"fmlp_mc_fwd: covers 3 <= L <= 4, H <= 64, C <= 64 (got L=%d H=%d C=%d)" % (a.L, a.H, a.C), kw
    assert fn(_fwd(n=0, x=None, out=None), None) == 0          # no rows: nothing to do
    for kw in (dict(x=None), dict(out=None), dict(w_first=None), dict(w_mid=None), dict(w_last=None)):
        assert fn(_fwd(x_stride=1, p=1.0, **kw), None) == _lib.ERR_BAD_ARG and said() == b"fmlp_mc_fwd: null x / out / weight pointer", kw
    assert fn(_fwd(x_stride=2, out_stride=1), None) == _lib.ERR_BAD_ARG and said() == b"fmlp_mc_fwd: x row stride smaller than F"
    assert fn(_fwd(out_stride=3 * 40 - 1, p=1.0), None) == _lib.ERR_BAD_ARG
    assert said() == b"fmlp_mc_fwd: out row stride smaller than the output width"
    assert fn(_fwd(sum_features=1, out_stride=39), None) == _lib.ERR_BAD_ARG
    for p in (1.0, 1.5, -0.25, float("nan")):
        assert fn(_fwd(p=p), None) == _lib.ERR_BAD_ARG and said() == b"fmlp_mc_fwd: dropout_p must be in [0, 1)", p
    # everything in order but the workspace: the last refusal, with both byte counts, still no launch
    a = _fwd()
    need = lib.gnan_fmlp_mc_fwd_workspace_bytes(a)
    assert need > 0
    assert fn(a, None) == _lib.ERR_WORKSPACE and said() == b"fmlp_mc_fwd: workspace 0 B < required %d B" % need
    a.workspace, a.workspace_bytes = WS, need - 1
    assert fn(a, None) == _lib.ERR_WORKSPACE and said() == b"fmlp_mc_fwd: workspace %d B < required %d B" % (need - 1, need)
    a.workspace, a.workspace_bytes = WS + 4, need
    assert fn(a, None) == _lib.ERR_BAD_ARG and said() == b"fmlp_mc_fwd: workspace must be 16-byte aligned"


def test_the_backward_refuses_in_the_order_of_gnan_fmlp_bwd_mfma_before_any_hip_call():
    lib = _lib.lib()
    fn = lib.gnan_fmlp_mc_bwd
    said = lambda: lib.gnan_last_error()                       # noqa: E731
    assert fn(None, None) == _lib.ERR_BAD_ARG and said() == b"fmlp_mc_bwd: null args"
    assert fn(_bwd(n=-1, L=2), None) == _lib.ERR_BAD_ARG and said() == b"fmlp_mc_bwd: bad sizes"
    assert fn(_bwd(F=0, H=65), None) == _lib.ERR_BAD_ARG and said() == b"fmlp_mc_bwd: bad sizes"
    for kw in (dict(L=2), dict(L=4), dict(H=65), dict(H=0), dict(C=0), dict(C=65)):
        a = _bwd(w_first=None, d_b_first=None, dropout_p=1.0, **kw)
        assert fn(a, None) == _lib.ERR_UNSUPPORTED, kw
        assert said() == b"fmlp_mc_bwd: covers L == 3, H <= 64, C <= 64 (got L=%d H=%d C=%d)" % (a.L, a.H, a.C), kw
    for kw in (dict(w_first=None), dict(w_last=None), dict(d_w_first=None), dict(d_w_last=None)):
        assert fn(_bwd(w_mid=None, **kw), None) == _lib.ERR_BAD_ARG and said() == b"fmlp_mc_bwd: null weight / gradient pointer", kw
    for kw in (dict(w_mid=None), dict(d_w_mid=None)):
        assert fn(_bwd(d_b_last=None, **kw), None) == _lib.ERR_BAD_ARG and said() == b"fmlp_mc_bwd: L == 3 needs w_mid and d_w_mid", kw
    for kw in (dict(b_first=None), dict(d_b_first=None), dict(b_mid=None), dict(d_b_mid=None), dict(b_last=None), dict(d_b_last=None)):
        assert fn(_bwd(x=None, **kw), None) == _lib.ERR_BAD_ARG, kw
        assert said() == b"fmlp_mc_bwd: a bias gradient is wanted exactly where there is a bias", kw
    for kw in (dict(x=None), dict(grad=None), dict(x_stride=2), dict(grad_stride=3 * 40 - 1)):
        assert fn(_bwd(dropout_p=1.0, **kw), None) == _lib.ERR_BAD_ARG and said() == b"fmlp_mc_bwd: bad x / grad", kw
    for p in (1.0, 1.5, -0.25, float("nan")):
        assert fn(_bwd(p=p), None) == _lib.ERR_BAD_ARG and said() == b"fmlp_mc_bwd: dropout_p must be in [0, 1)", p
    a = _bwd()
    need = lib.gnan_fmlp_mc_bwd_workspace_bytes(a)
    assert need > 0
    assert fn(a, None) == _lib.ERR_WORKSPACE and said() == b"fmlp_mc_bwd: workspace 0 B < required %d B" % need
    a.workspace, a.workspace_bytes = WS, need - 4
    assert fn(a, None) == _lib.ERR_WORKSPACE and said() == b"fmlp_mc_bwd: workspace %d B < required %d B" % (need - 4, need)


def test_the_forward_workspace_is_the_packed_weights_plus_the_chunk_partials():
    lib = _lib.lib()
    q = lib.gnan_fmlp_mc_fwd_workspace_bytes
    assert q(None) == 0
    for kw in (dict(L=2), dict(L=5), dict(H=65), dict(H=0), dict(C=0), dict(C=65), dict(n=-1), dict(F=0)):
        assert q(_fwd(**kw)) == 0, kw

    def stream(H, L, C):        # floats per feature: mid layers | W3 | {w1, b1} | b_mid | b_last, in whole KiB pieces per wave
        HP, CP, M = (32 if H <= 32 else 64), (32 if C <= 32 else 64), L - 2
        return (M * HP * HP + CP * HP + 2 * HP + M * HP + CP + 1023) // 1024 * 1024

    for H, L, C in ((16, 3, 9), (16, 3, 33), (64, 3, 40), (64, 4, 64), (33, 4, 8), (32, 3, 32)):
        assert q(_fwd(F=5, H=H, L=L, C=C)) == 4 * 5 * stream(H, L, C), (H, L, C)
        assert q(_fwd(F=5, H=H, L=L, C=C, p=0.0)) == 4 * 5 * stream(H, L, C)       # Dropout does not move it
    # the existing entry point still answers 0 at C = 9, and still refuses the matrix cores there
    assert lib.gnan_fmlp_fwd_workspace_bytes(_fwd(C=9, algo=_lib.FMLP_MFMA)) == 0
    assert lib.gnan_fmlp_fwd(_fwd(C=9, algo=_lib.FMLP_MFMA), None) == _lib.ERR_UNSUPPORTED
    # sum_features: one feature chunk -> nothing more; chunks > 1 (few nodes, several features) -> chunks * n * C floats more
    packed = 4 * 5 * stream(16, 3, 40)
    assert q(_fwd(F=1, sum_features=1)) == 4 * stream(16, 3, 40)
    assert q(_fwd(F=2, sum_features=1)) == 4 * 2 * stream(16, 3, 40)
    n = 33
    assert q(_fwd(n=n, F=5, sum_features=1)) == packed + 3 * n * 40 * 4               # ceil(5 / 2) = 3 chunks of two features
    assert q(_fwd(n=n, F=5, sum_features=0)) == packed
    assert q(_fwd(n=1 << 20, F=5, sum_features=1)) == packed                          # enough node blocks: one chunk
    assert q(_fwd(n=0, F=5, sum_features=1)) == packed


def test_the_backward_workspace_grows_with_the_split_count_and_is_zero_for_no_nodes():
    lib = _lib.lib()
    q = lib.gnan_fmlp_mc_bwd_workspace_bytes
    assert q(None) == 0 and q(_bwd(n=0)) == 0
    F, H, C = 3, 16, 40
    block = 4 * (2 * F * H + F * H * H + F * H + F * C * H + F * C)       # one node range's gradients, bytes
    sizes = [q(_bwd(n=n, F=F, H=H, C=C)) for n in (1, 128, 129, 256, 257, 700, 5000, 1 << 20, 1 << 24)]
    assert sizes[0] == sizes[1] == 0                                      # one range: straight into the outputs
    assert sizes == sorted(sizes)
    assert all(s % block == 0 for s in sizes)
    assert [s // block for s in sizes[2:6]] == [2, 2, 3, 6]              # ranges of at least 128 nodes (a tile per wave)
    assert sizes[-1] == sizes[-2] == block * ((512 + F - 1) // F)        # capped: enough workgroups to fill the chip
    assert q(_bwd(n=1 << 20, F=1000, H=H, C=C)) == 0                      # many features: one range each
    for kw in (dict(L=2), dict(L=4), dict(H=0), dict(H=65), dict(C=0), dict(C=65)):
        assert q(_bwd(**kw)) == 0, kw
    # the C <= 8 entry point still refuses C = 9
    assert lib.gnan_fmlp_bwd_mfma(_bwd(C=9), None) == _lib.ERR_UNSUPPORTED


def test_the_routing_predicate_over_the_covers_edges_the_switches_and_the_clamp():
    route = functional.dropout_mc_routes
    on = dict(forward_on=True, backward_on=True, min_work=1 << 16)
    n, F = 1 << 14, 4                                                       # n * F == the threshold
    assert route(n, F, 3, 64, 9, **on) == (True, True)
    assert route(n, F, 3, 64, 64, **on) == (True, True)
    assert route(n, F, 3, 1, 40, **on) == (True, True)
    assert route(n - 1, F, 3, 64, 40, **on) == (False, False)               # one node short of the threshold
    assert route(n, F, 4, 64, 40, **on) == (True, False)                    # L = 4: the forward's cover only
    assert route(n, F, 2, 64, 40, **on) == (False, False)
    assert route(n, F, 5, 64, 40, **on) == (False, False)
    assert route(n, F, 3, 65, 40, **on) == (False, False)
    assert route(n, F, 3, 0, 40, **on) == (False, False)
    assert route(n, F, 3, 64, 8, **on) == (False, False)                    # C <= 8 belongs to dropout_mfma_routes
    assert route(n, F, 3, 64, 65, **on) == (False, False)
    assert route(n, F, 3, 64, 40, x_grad=True, **on) == (True, False)       # x.grad: the backward stays where it was
    assert route(n, F, 3, 64, 40, forward_on=False, backward_on=True, min_work=1) == (False, True)
    assert route(n, F, 3, 64, 40, forward_on=True, backward_on=False, min_work=1) == (True, False)
    assert route(1, 1, 3, 64, 40, forward_on=True, backward_on=True, min_work=1) == (True, True)
    # as shipped: the threshold is its own name and never lies below the clamp, so no batch below 2^16 node-features leaves
    # the lane forward and the restatement's backward, whatever was measured
    assert functional.DROPOUT_MFMA_CLAMP == 1 << 16
    assert functional.DROPOUT_MC_MIN_WORK == max(functional.DROPOUT_MC_MEASURED_MIN_WORK, functional.DROPOUT_MFMA_CLAMP)
    assert functional.DROPOUT_MC_MIN_WORK >= 1 << 16
    assert route(300, 4, 3, 16, 9, forward_on=True, backward_on=True) == (False, False)
    assert route((1 << 16) - 1, 1, 3, 64, 40, forward_on=True, backward_on=True) == (False, False)
    assert isinstance(functional.DROPOUT_MC, bool) and isinstance(functional.DROPOUT_MC_BACKWARD, bool)
    assert route(1 << 20, 64, 3, 64, 40) == (functional.DROPOUT_MC, functional.DROPOUT_MC_BACKWARD)
    # the C <= 8 predicate and its threshold are what they were
    assert functional.dropout_mfma_routes(n, F, 3, 64, 9, **on) == (False, False)
    assert functional.dropout_mfma_routes(1 << 20, 64, 3, 64, 9) == (False, False)
    assert functional.DROPOUT_MFMA_MIN_WORK == max(1 << 18, functional.DROPOUT_MFMA_CLAMP)


def _documented_routes(n, F, L, H, C, x_grad, mfma_fwd, mfma_bwd, mc_fwd, mc_bwd):
    """The truth table of a Dropout call's kernels, written out from the covers the kernels document: ``gnan_fmlp_fwd`` on the matrix
    cores 3 <= L <= 4, H <= 64, C <= 8; ``gnan_fmlp_mc_fwd`` the same with 9 <= C <= 64; ``gnan_fmlp_bwd`` L in {2, 3}, H <= 64,
    C <= 8; ``gnan_fmlp_bwd_mfma`` L = 3 inside that; ``gnan_fmlp_mc_bwd`` L = 3, H <= 64, 9 <= C <= 64; no backward kernel hands out
    x.grad; the matrix-core kernels start at their thresholds."""
    work, narrow, wide = n * F, 1 <= C <= 8, 9 <= C <= 64
    forward = "lane"
    if L in (3, 4) and 1 <= H <= 64:
        if narrow and mfma_fwd and work >= functional.DROPOUT_MFMA_MIN_WORK:
            forward = "mfma"
        if wide and mc_fwd and work >= functional.DROPOUT_MC_MIN_WORK:
            forward = "mc"
    backward = None
    if not x_grad and 1 <= H <= 64:
        if narrow and L == 2:
            backward = "lane"
        if narrow and L == 3:
            backward = "mfma" if mfma_bwd and work >= functional.DROPOUT_MFMA_MIN_WORK else "lane"
        if wide and L == 3 and mc_bwd and work >= functional.DROPOUT_MC_MIN_WORK:
            backward = "mc"
    return forward, backward


def test_the_combined_route_function_agrees_with_the_documented_truth_table(monkeypatch):
    F = 4
    assert functional.DROPOUT_MC_MIN_WORK < functional.DROPOUT_MFMA_MIN_WORK and functional.DROPOUT_MC_MIN_WORK % F == 0
    sizes = [functional.DROPOUT_MC_MIN_WORK // F - 1, functional.DROPOUT_MC_MIN_WORK // F,
             functional.DROPOUT_MFMA_MIN_WORK // F - 1, functional.DROPOUT_MFMA_MIN_WORK // F]
    seen = set()
    for bits in range(16):
        switches = [bool(bits >> k & 1) for k in range(4)]
        for name, on in zip(("DROPOUT_MFMA", "DROPOUT_MFMA_BACKWARD", "DROPOUT_MC", "DROPOUT_MC_BACKWARD"), switches):
            monkeypatch.setattr(functional, name, on)
        for L in (1, 2, 3, 4, 5):
            for H in (1, 64, 65):
                for C in (1, 8, 9, 64, 65):
                    for n in sizes:
                        for x_grad in (False, True):
                            want = _documented_routes(n, F, L, H, C, x_grad, *switches)
                            assert functional.dropout_routes(n, F, L, H, C, x_grad) == want, (switches, n, L, H, C, x_grad)
                            seen.add(want)
    # the grid reaches every pair the covers allow (C <= 8 and C >= 9 never share a call)
    assert seen == {("lane", None), ("lane", "lane"), ("lane", "mfma"), ("lane", "mc"), ("mfma", None), ("mfma", "lane"),
                    ("mfma", "mfma"), ("mc", None), ("mc", "mc")}
