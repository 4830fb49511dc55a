"""Host side of Dropout in captured steps: the seed cell (gnan_dropout_seed_set), the device-seed record and the six *_drop_dev
entry points — declared, exported and bound under ABI 51, the record's layout, and the refusals: all of them happen on the host
before any HIP call, so none of this needs a GPU."""
import ctypes
import os
import re

import pytest

from gnan_amd import _lib
from conftest import ROOT

ENTRY_POINTS = {
    "gnan_small_graph_fwd_drop_dev": (_lib.SmallGraphArgs, "small_graph"),
    "gnan_small_graph_bwd_drop_dev": (_lib.SmallGraphBwdArgs, "small_graph_bwd"),
    "gnan_mid_graph_fwd_drop_dev": (_lib.MidGraphArgs, "mid_graph"),
    "gnan_mid_graph_bwd_drop_dev": (_lib.MidGraphBwdArgs, "mid_graph_bwd"),
    "gnan_small_batch_fwd_drop_dev": (_lib.SmallBatchArgs, "small_batch"),
    "gnan_small_batch_bwd_drop_dev": (_lib.SmallBatchBwdArgs, "small_batch_bwd"),
}
CELL = 0x1000          # a non-NULL "device" address: no refusal under test ever follows it


def _header():
    return open(os.path.join(ROOT, "include", "gnan_hip.h")).read()


def _args(cls, n=30, F=3, D=4, L=3, H=8, C=1, rho_c=1, **more):
    """A record of sizes the routes cover — no pointers: every refusal under test comes before the first pointer is looked at."""
    mlp = lambda c: _lib.SmallMlp(L=L, H=H, C=c)                  # noqa: E731
    if cls is _lib.SmallBatchBwdArgs:           # (this backward looks at its gradient pointers before its sizes: give it some)
        full = _lib.SmallMlpGrads(w_first=CELL, w_mid=CELL, w_last=CELL)
        more = dict(df=full, drho=full, **more)
    if cls in (_lib.SmallBatchArgs, _lib.SmallBatchBwdArgs):
        return cls(total_nodes=n, n_graphs=1, max_nodes=n, F=F, D=D, x_stride=F, cnt_stride=D, f=mlp(C), rho=mlp(rho_c), **more)
    return cls(n=n, F=F, D=D, x_stride=F, cnt_stride=D, f=mlp(C), rho=mlp(rho_c))


def _record(p=0.6, reserved=0, seed=CELL):
    return _lib.SmallDropoutDev(p=p, reserved=reserved, seed=seed)


def test_the_seven_entry_points_are_declared_exported_and_bound_under_abi_51():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    handle = ctypes.CDLL(_lib.LIB_PATH)
    assert _lib.ABI_VERSION == 51 and handle.gnan_abi_version() == 51
    assert re.search(r"#define GNAN_ABI_VERSION 51\b", _header())
    for name, (cls, _) in ENTRY_POINTS.items():
        assert not name.endswith("_drop")                        # (the eager path's spy counts names with that ending)
        assert re.search(r"\bint %s\(const \w+\* a, const gnan_small_dropout_dev\* d, gnan_stream_t stream\);" % name, text), name
        assert hasattr(handle, name), name
        res, argtypes = _lib.SYMBOLS[name]
        assert res is ctypes.c_int
        assert argtypes == [ctypes.POINTER(cls), ctypes.POINTER(_lib.SmallDropoutDev), ctypes.c_void_p], name
        assert getattr(_lib.lib(), name).argtypes == argtypes
    assert re.search(r"\bint gnan_dropout_seed_set\(uint64_t\* cell, uint64_t seed, gnan_stream_t stream\);", text)
    assert hasattr(handle, "gnan_dropout_seed_set")
    assert _lib.SYMBOLS["gnan_dropout_seed_set"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p])


def test_the_record_is_the_headers():
    body = re.search(r"typedef struct gnan_small_dropout_dev \{(.*?)\} gnan_small_dropout_dev;", _header(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decls = [d.strip() for d in body.split(";") if d.strip()]
    assert [d.split()[-1] for d in decls] == [f[0] for f in _lib.SmallDropoutDev._fields_] == ["p", "reserved", "seed"]
    assert decls == ["float p", "int32_t reserved", "const uint64_t* seed"]
    assert [f[1] for f in _lib.SmallDropoutDev._fields_] == [ctypes.c_float, ctypes.c_int32, ctypes.c_void_p]
    assert ctypes.sizeof(_lib.SmallDropoutDev) == 16 and _lib.SmallDropoutDev.seed.offset == 8
    # the by-value record did not move
    assert ctypes.sizeof(_lib.SmallDropout) == 16 and [f[0] for f in _lib.SmallDropout._fields_] == ["p", "reserved", "seed"]


def test_a_null_cell_is_refused_before_any_hip_call():
    lib = _lib.lib()
    assert lib.gnan_dropout_seed_set(None, 5, None) == _lib.ERR_BAD_ARG
    assert b"dropout_seed_set: null cell" in lib.gnan_last_error()


@pytest.mark.parametrize("name", sorted(ENTRY_POINTS))
def test_a_bad_record_is_refused_before_anything_else_in_the_order_of_drop_ok(name):
    cls, who = ENTRY_POINTS[name]
    lib = _lib.lib()
    fn = getattr(lib, name)
    a = _args(cls, n=200 if "mid" in name else 30)
    assert fn(a, None, None) == _lib.ERR_BAD_ARG and b"null dropout record" in lib.gnan_last_error()
    for p in (1.0, 1.5, -0.25, float("nan"), float("inf")):
        # (a bad p wins over a bad reserved word and a NULL cell: the order of drop_ok)
        assert fn(a, _record(p=p, reserved=7, seed=None), None) == _lib.ERR_BAD_ARG, p
        assert b"p must be in [0, 1)" in lib.gnan_last_error(), p
    assert fn(a, _record(reserved=7, seed=None), None) == _lib.ERR_BAD_ARG
    assert b"reserved must be 0" in lib.gnan_last_error() and b"reserved=7" in lib.gnan_last_error()
    for p in (0.0, 0.6):
        assert fn(a, _record(p=p, seed=None), None) == _lib.ERR_BAD_ARG
        assert lib.gnan_last_error().startswith(who.encode() + b":") and b"null dropout seed cell" in lib.gnan_last_error()
    assert fn(None, _record(), None) == _lib.ERR_BAD_ARG
    assert b"null args" in lib.gnan_last_error()
    # a good record: the call goes on to the plain entry point's own checks — these sizes are covered, the pointers are missing
    for p in (0.0, 0.6):
        assert fn(a, _record(p=p), None) == _lib.ERR_BAD_ARG
        assert b"null" in lib.gnan_last_error() and b"dropout" not in lib.gnan_last_error()


@pytest.mark.parametrize("name", sorted(ENTRY_POINTS))
def test_shapes_outside_the_cover_stay_unsupported(name):
    """... with the messages of the plain entry points (shape_ok): the limit and the value."""
    cls, who = ENTRY_POINTS[name]
    lib = _lib.lib()
    fn, plain = getattr(lib, name), getattr(lib, name[: -len("_drop_dev")])
    top = 448 if "mid" in name else 128
    for kw, said in ((dict(n=top + 1), b"covers n <= %d nodes (got n=%d)" % (top, top + 1)),
                     (dict(H=65), b"covers 1 <= H <= 64 (got H=65 for f)"),
                     (dict(C=9), b"covers 1 <= C <= 8 output channels (got C=9)"),
                     (dict(L=4), b"covers L in {2, 3} (got L=4 for f)")):
        a = _args(cls, **kw)
        assert fn(a, _record(), None) == _lib.ERR_UNSUPPORTED, kw
        mine = lib.gnan_last_error()
        assert mine.startswith(who.encode() + b":") and said in mine, (kw, mine)
        assert plain(a, None) == _lib.ERR_UNSUPPORTED and lib.gnan_last_error() == mine


@pytest.mark.parametrize("name", ["gnan_small_batch_fwd_drop_dev", "gnan_small_batch_bwd_drop_dev"])
def test_the_batch_kernels_cover_the_slots_semantics_only(name):
    """rho_raw_hops == 0, rest_zero == 0 and a one-channel rho: anything else is GNAN_ERR_UNSUPPORTED naming limit and value —
    shapes the plain batch entry points take (they go on to their pointer checks)."""
    cls, who = ENTRY_POINTS[name]
    lib = _lib.lib()
    fn, plain = getattr(lib, name), getattr(lib, name[: -len("_drop_dev")])
    for kw, said in ((dict(rho_raw_hops=1), b"covers rho_raw_hops == 0 (got rho_raw_hops=1)"),
                     (dict(rest_zero=1), b"covers rest_zero == 0 (got rest_zero=1)"),
                     (dict(C=4, rho_c=4), b"covers a one-channel rho (got rho.C=4)")):
        a = _args(cls, **kw)
        assert fn(a, _record(), None) == _lib.ERR_UNSUPPORTED, kw
        mine = lib.gnan_last_error()
        assert mine.startswith(who.encode() + b":") and said in mine, (kw, mine)
        assert plain(a, None) == _lib.ERR_BAD_ARG and b"null" in lib.gnan_last_error()     # the plain route's cover holds it
    a = _args(cls)
    assert fn(a, _record(), None) == _lib.ERR_BAD_ARG and b"null" in lib.gnan_last_error()
