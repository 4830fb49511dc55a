"""Host side of the one-launch graph routes under training-mode Dropout (gnan_small_graph_fwd_drop / _bwd_drop,
gnan_mid_graph_fwd_drop / _bwd_drop): declared, exported and bound under ABI 51, the record's layout, and the refusals — all of
them happen on the host before any HIP call, so none of this needs a GPU."""
import ctypes
import os
import re

import pytest

from gnan_amd import _lib
from conftest import ROOT

ENTRY_POINTS = {
    "gnan_small_graph_fwd_drop": (_lib.SmallGraphArgs, "small_graph"),
    "gnan_small_graph_bwd_drop": (_lib.SmallGraphBwdArgs, "small_graph_bwd"),
    "gnan_mid_graph_fwd_drop": (_lib.MidGraphArgs, "mid_graph"),
    "gnan_mid_graph_bwd_drop": (_lib.MidGraphBwdArgs, "mid_graph_bwd"),
}


def _header():
    return open(os.path.join(ROOT, "include", "gnan_hip.h")).read()


def _args(cls, n=30, F=3, D=4, L=3, H=8, C=1):
    """A record of sizes the routes cover (n: 30 for the small route; the mid route takes it too) — no pointers: every refusal
    under test comes before the first pointer is looked at."""
    mlp = lambda c: _lib.SmallMlp(L=L, H=H, C=c)                  # noqa: E731
    return cls(n=n, F=F, D=D, x_stride=F, cnt_stride=D, f=mlp(C), rho=mlp(1))


def test_the_four_entry_points_are_declared_exported_and_bound_under_abi_51():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    handle = ctypes.CDLL(_lib.LIB_PATH)
    assert _lib.ABI_VERSION == 51 and handle.gnan_abi_version() == 51
    assert re.search(r"#define GNAN_ABI_VERSION 51\b", _header())
    for name, (cls, _) in ENTRY_POINTS.items():
        assert re.search(r"\bint %s\(const \w+\* a, const gnan_small_dropout\* d, gnan_stream_t stream\);" % name, text), name
        assert hasattr(handle, name), name
        res, argtypes = _lib.SYMBOLS[name]
        assert res is ctypes.c_int
        assert argtypes == [ctypes.POINTER(cls), ctypes.POINTER(_lib.SmallDropout), ctypes.c_void_p], name
        assert getattr(_lib.lib(), name).argtypes == argtypes


def test_the_record_is_the_headers():
    body = re.search(r"typedef struct gnan_small_dropout \{(.*?)\} gnan_small_dropout;", _header(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [d.split()[-1] for d in body.split(";") if d.strip()]
    types = [d.split()[0] for d in body.split(";") if d.strip()]
    assert fields == [f[0] for f in _lib.SmallDropout._fields_] == ["p", "reserved", "seed"]
    assert types == ["float", "int32_t", "uint64_t"]
    assert [f[1] for f in _lib.SmallDropout._fields_] == [ctypes.c_float, ctypes.c_int32, ctypes.c_uint64]
    assert ctypes.sizeof(_lib.SmallDropout) == 16 and _lib.SmallDropout.seed.offset == 8


@pytest.mark.parametrize("name", sorted(ENTRY_POINTS))
def test_a_bad_record_is_refused_before_anything_else(name):
    cls, _ = ENTRY_POINTS[name]
    lib = _lib.lib()
    fn = getattr(lib, name)
    a = _args(cls, n=200 if "mid" in name else 30)
    assert fn(a, None, None) == _lib.ERR_BAD_ARG and b"null dropout" in lib.gnan_last_error()
    for p in (1.0, 1.5, -0.25, float("nan"), float("inf")):
        assert fn(a, _lib.SmallDropout(p=p, reserved=0, seed=1), None) == _lib.ERR_BAD_ARG, p
        assert b"p must be in [0, 1)" in lib.gnan_last_error(), p
    assert fn(a, _lib.SmallDropout(p=0.5, reserved=7, seed=1), None) == _lib.ERR_BAD_ARG
    assert b"reserved must be 0" in lib.gnan_last_error() and b"reserved=7" in lib.gnan_last_error()
    assert fn(None, _lib.SmallDropout(p=0.5, reserved=0, seed=1), None) == _lib.ERR_BAD_ARG
    assert b"null args" in lib.gnan_last_error()
    # a good record: the call goes on to the plain entry point's own checks — these sizes are covered, the pointers are missing
    for p in (0.0, 0.6):
        assert fn(a, _lib.SmallDropout(p=p, reserved=0, seed=(1 << 63) + 5), None) == _lib.ERR_BAD_ARG
        assert b"null" in lib.gnan_last_error() and b"dropout" not in lib.gnan_last_error()


@pytest.mark.parametrize("name", sorted(ENTRY_POINTS))
def test_shapes_outside_the_cover_stay_unsupported(name):
    """... with the messages of the plain entry points (shape_ok): the limit and the value."""
    cls, who = ENTRY_POINTS[name]
    lib = _lib.lib()
    fn, plain = getattr(lib, name), getattr(lib, name[: -len("_drop")])
    good = _lib.SmallDropout(p=0.6, reserved=0, seed=3)
    top = 448 if "mid" in name else 128
    for kw, said in ((dict(n=top + 1), b"covers n <= %d nodes (got n=%d)" % (top, top + 1)),
                     (dict(H=65), b"covers 1 <= H <= 64 (got H=65 for f)"),
                     (dict(C=9), b"covers 1 <= C <= 8 output channels (got C=9)"),
                     (dict(L=4), b"covers L in {2, 3} (got L=4 for f)")):
        a = _args(cls, **kw)
        assert fn(a, good, None) == _lib.ERR_UNSUPPORTED, kw
        mine = lib.gnan_last_error()
        assert mine.startswith(who.encode() + b":") and said in mine, (kw, mine)
        assert plain(a, None) == _lib.ERR_UNSUPPORTED and lib.gnan_last_error() == mine
