"""Host side of ``gnan_attr_rows`` (csrc/attr_rows.hip): the ABI additions are declared, exported and bound under ABI 51, every
refusal happens before a HIP call (so all of this runs without a GPU), and ``describe`` agrees with ``workspace_bytes``."""
import ctypes
import os
import re

import pytest

import gnan_amd  # noqa: F401
from gnan_amd import _lib
from conftest import ROOT

FUNCS = ("gnan_attr_rows", "gnan_attr_rows_workspace_bytes", "gnan_attr_rows_describe")
P = 0x1000                      # a non-null pointer value: nothing is dereferenced before the refusals (or by describe)


def header():
    return open(os.path.join(ROOT, "include", "gnan_hip.h")).read()


def args(**kw):
    base = dict(n_rows=4, n_cols=300, rowptr=P, col=P, code=P, S=P, W=8, s_stride=8, lut=P, D=5, Cw=1, A=P, a_stride=40,
                max_row_pairs=10)
    base.update(kw)
    return _lib.AttrArgs(**base)


def refused(a, code, text):
    lib = _lib.lib()
    assert lib.gnan_attr_rows(a, None) == code
    msg = lib.gnan_last_error().decode()
    assert text in msg, msg
    return msg


def test_declared_exported_and_bound_under_abi_51():
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for f in FUNCS:
        assert re.search(r"\b%s\s*\(" % f, text), f
        assert hasattr(handle, f) and f in _lib.SYMBOLS, f
    for s in ("gnan_attr_args", "gnan_attr_info"):
        assert re.search(r"typedef struct %s \{" % s, text), s
    assert "#define GNAN_ABI_VERSION 51" in header()
    assert _lib.ABI_VERSION == 51 and _lib.lib().gnan_abi_version() == 51


def test_ctypes_field_order_matches_the_header():
    text = header()
    for struct, cls in (("gnan_attr_args", _lib.AttrArgs), ("gnan_attr_info", _lib.AttrInfo)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                fields.append(decl.split()[-1].lstrip("*"))
        assert fields == [f[0] for f in cls._fields_], struct


def test_refusals_come_before_any_hip_call():
    lib = _lib.lib()
    assert lib.gnan_attr_rows(None, None) == _lib.ERR_BAD_ARG and b"null args" in lib.gnan_last_error()
    for name in ("code", "S", "lut", "A"):
        refused(args(**{name: None}), _lib.ERR_BAD_ARG, "null")
    assert "D=1" in refused(args(D=1, a_stride=8), _lib.ERR_UNSUPPORTED, "2 <= D <= 256")
    assert "D=257" in refused(args(D=257, a_stride=257 * 8), _lib.ERR_UNSUPPORTED, "2 <= D <= 256")
    assert "W must be >= 1 (got 0)" in refused(args(W=0), _lib.ERR_BAD_ARG, "W must be")
    assert "Cw=3, W=8" in refused(args(Cw=3), _lib.ERR_BAD_ARG, "Cw must divide W")
    refused(args(col=None), _lib.ERR_BAD_ARG, "rowptr and col must both be set (CSR) or both NULL (dense)")
    refused(args(rowptr=None), _lib.ERR_BAD_ARG, "rowptr and col")
    refused(args(s_stride=7), _lib.ERR_BAD_ARG, "operand row stride")
    refused(args(a_stride=39), _lib.ERR_BAD_ARG, "output row stride")
    refused(args(cnt=P, cnt_stride=4), _lib.ERR_BAD_ARG, "cnt row stride")
    refused(args(lut_row_stride=4), _lib.ERR_BAD_ARG, "lut_row_stride")
    refused(args(item_ptr=P, n_items=3), _lib.ERR_BAD_ARG, "at least one work item per row")
    info = _lib.AttrInfo()
    assert lib.gnan_attr_rows_describe(args(), None) == _lib.ERR_BAD_ARG
    assert lib.gnan_attr_rows_describe(args(D=257, a_stride=257 * 8), info) == _lib.ERR_UNSUPPORTED


def test_short_workspace_is_refused_with_both_sizes():
    chunk = describe(args())["chunk_pairs"]
    a = args(max_row_pairs=2 * chunk + 3)
    need = _lib.lib().gnan_attr_rows_workspace_bytes(a)
    assert need == 4 * 3 * 5 * 8 * 4                                       # rows x chunks x D x W floats
    msg = refused(a, _lib.ERR_WORKSPACE, "workspace")
    assert str(need) in msg
    a.workspace, a.workspace_bytes = P, need - 4
    assert str(need - 4) in refused(a, _lib.ERR_WORKSPACE, str(need))


def describe(a):
    info = _lib.AttrInfo()
    assert _lib.lib().gnan_attr_rows_describe(a, info) == 0, _lib.lib().gnan_last_error()
    return info.as_dict()


@pytest.mark.parametrize("W,D", [(1, 2), (3, 17), (8, 64), (63, 65), (64, 256), (65, 5), (130, 256)])
def test_describe_is_consistent_with_workspace_bytes(W, D):
    lib = _lib.lib()
    base = describe(args(W=W, s_stride=W, D=D, a_stride=D * W))
    chunk = base["chunk_pairs"]
    assert base["col_tiles"] == -(-W // 64) and base["shell_passes"] == -(-D // 64) and base["launches"] == 2
    assert base["lds_bytes"] == 4 * min(D, 64) * 64 * 4 <= 64 * 1024
    wp = 1
    while wp < W:
        wp *= 2                                                              # the next power of two >= W
    assert base["pair_slots"] == (64 // wp if W < 64 else 1)
    for pairs, chunks in ((0, 1), (1, 1), (chunk - 1, 1), (chunk, 1), (chunk + 1, 2), (2 * chunk + 3, 3)):
        a = args(W=W, s_stride=W, D=D, a_stride=D * W, max_row_pairs=pairs)
        d = describe(a)
        assert d["max_row_chunks"] == chunks and d["n_items"] == 4 * chunks
        want = 0 if chunks == 1 else 4 * chunks * D * W * 4
        assert d["workspace_bytes"] == want == lib.gnan_attr_rows_workspace_bytes(a)
    # a per-row chunk list replaces the uniform one; the dense layout is as long as it is wide
    a = args(W=W, s_stride=W, D=D, a_stride=D * W, item_ptr=P, n_items=7)
    assert describe(a)["n_items"] == 7 and lib.gnan_attr_rows_workspace_bytes(a) == 7 * D * W * 4
    a = args(W=W, s_stride=W, D=D, a_stride=D * W, rowptr=None, col=None, n_cols=chunk + 1, max_row_pairs=0)
    assert describe(a)["max_row_chunks"] == 2
    assert describe(args(W=W, s_stride=W, D=D, a_stride=D * W, n_rows=0))["launches"] == 0
