"""Host side of ``gnan_attr_cols`` (csrc/attr_cols.hip): the ABI additions are declared, exported and bound under ABI 51, every
refusal happens before a HIP call (so all of this runs without a GPU), and ``describe`` agrees with ``workspace_bytes``."""
import ctypes
import os
import re

import pytest

import gnan_amd  # noqa: F401
from gnan_amd import _lib
from conftest import ROOT

FUNCS = ("gnan_attr_cols", "gnan_attr_cols_workspace_bytes", "gnan_attr_cols_describe")
P = 0x1000                      # a non-null pointer value: nothing is dereferenced before the refusals (or by describe)


def header():
    return open(os.path.join(ROOT, "include", "gnan_hip.h")).read()


def args(**kw):
    base = dict(n_cols=4, n_src=300, n_rows=200, rowptr_t=P, row=P, code=P, n_row_ids=-1, S=P, W=8, s_stride=8, lut=P, D=5, Cw=1,
                B=P, b_stride=40, max_col_pairs=10)
    base.update(kw)
    return _lib.AttrColsArgs(**base)


def refused(a, code, text):
    lib = _lib.lib()
    assert lib.gnan_attr_cols(a, None) == code
    msg = lib.gnan_last_error().decode()
    assert text in msg, msg
    return msg


def describe(a):
    info = _lib.AttrColsInfo()
    assert _lib.lib().gnan_attr_cols_describe(a, info) == 0, _lib.lib().gnan_last_error()
    return info.as_dict()


def test_declared_exported_and_bound_under_abi_51():
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for f in FUNCS:
        assert re.search(r"\b%s\s*\(" % f, text), f
        assert hasattr(handle, f) and f in _lib.SYMBOLS, f
    for s in ("gnan_attr_cols_args", "gnan_attr_cols_info"):
        assert re.search(r"typedef struct %s \{" % s, text), s
    assert "#define GNAN_ABI_VERSION 51" in header()
    assert _lib.ABI_VERSION == 51 and _lib.lib().gnan_abi_version() == 51


def test_ctypes_field_order_matches_the_header():
    text = header()
    for struct, cls in (("gnan_attr_cols_args", _lib.AttrColsArgs), ("gnan_attr_cols_info", _lib.AttrColsInfo)):
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
    assert lib.gnan_attr_cols(None, None) == _lib.ERR_BAD_ARG and b"null args" in lib.gnan_last_error()
    for name in ("code", "S", "lut", "B"):
        refused(args(**{name: None}), _lib.ERR_BAD_ARG, "null")
    assert "D=1" in refused(args(D=1, b_stride=8), _lib.ERR_UNSUPPORTED, "2 <= D <= 256")
    assert "D=257" in refused(args(D=257, b_stride=257 * 8), _lib.ERR_UNSUPPORTED, "2 <= D <= 256")
    assert "W must be >= 1 (got 0)" in refused(args(W=0), _lib.ERR_BAD_ARG, "W must be")
    assert "Cw=3, W=8" in refused(args(Cw=3), _lib.ERR_BAD_ARG, "Cw must divide W")
    refused(args(row=None), _lib.ERR_BAD_ARG, "rowptr_t and row must both be set (CSR) or both NULL (dense)")
    refused(args(rowptr_t=None), _lib.ERR_BAD_ARG, "rowptr_t and row")
    refused(args(s_stride=7), _lib.ERR_BAD_ARG, "operand row stride")
    refused(args(b_stride=39), _lib.ERR_BAD_ARG, "output row stride")
    refused(args(cnt=P, cnt_stride=4), _lib.ERR_BAD_ARG, "cnt row stride")
    refused(args(lut_row_stride=4), _lib.ERR_BAD_ARG, "lut_row_stride")
    assert "n_row_ids=3" in refused(args(n_row_ids=3), _lib.ERR_BAD_ARG, "null row_ids")
    refused(args(item_ptr=P, n_items=3), _lib.ERR_BAD_ARG, "at least one work item per source")
    refused(args(n_rows=-1), _lib.ERR_BAD_ARG, "negative size")
    info = _lib.AttrColsInfo()
    assert lib.gnan_attr_cols_describe(args(), None) == _lib.ERR_BAD_ARG
    assert lib.gnan_attr_cols_describe(args(D=257, b_stride=257 * 8), info) == _lib.ERR_UNSUPPORTED
    # nothing to do: no source requested — accepted without a workspace and without a launch
    assert lib.gnan_attr_cols(args(n_cols=0), None) == 0


def test_short_workspace_is_refused_with_both_sizes():
    a = args()
    need = _lib.lib().gnan_attr_cols_workspace_bytes(a)
    assert need == 4 * 5 * 1 * 4                                           # sources x D x Cw floats: V alone
    msg = refused(a, _lib.ERR_WORKSPACE, "workspace")
    assert str(need) in msg
    a.workspace, a.workspace_bytes = P, need - 4
    assert str(need - 4) in refused(a, _lib.ERR_WORKSPACE, str(need))


@pytest.mark.parametrize("W,D,Cw", [(1, 2, 1), (3, 17, 3), (8, 64, 1), (63, 65, 1), (64, 256, 4), (65, 5, 5), (130, 256, 1)])
def test_describe_is_consistent_with_workspace_bytes(W, D, Cw):
    lib = _lib.lib()
    kw = dict(W=W, s_stride=W, D=D, Cw=Cw, b_stride=D * W)
    base = describe(args(**kw))
    chunk, bins = base["chunk_pairs"], D * Cw
    assert base["bin_passes"] == -(-bins // 64) and base["block_size"] == 64 * base["items_per_block"]
    assert base["lds_bytes"] == base["items_per_block"] * min(bins, 64) * 64 * 4 <= 64 * 1024
    assert base["launches"] == 2 and base["t_blocks"] == 0
    for pairs, chunks in ((0, 1), (1, 1), (chunk - 1, 1), (chunk, 1), (chunk + 1, 2), (2 * chunk + 3, 3)):
        a = args(max_col_pairs=pairs, **kw)
        d = describe(a)
        assert d["max_col_chunks"] == chunks and d["n_items"] == 4 * chunks
        want = 4 * bins * 4 + (0 if chunks == 1 else 4 * chunks * bins * 4)  # V, and the partials of columns of several chunks
        assert d["workspace_bytes"] == want == lib.gnan_attr_cols_workspace_bytes(a)
        assert d["launches"] == (2 if chunks == 1 else 3)
    # the multiplicities of row_ids, the blocks of T and T itself join the workspace
    rows = 2 * base["t_block_rows"] + 1
    a = args(n_rows=rows, row_ids=P, n_row_ids=7, rest_from_total=1, **kw)
    d = describe(a)
    assert d["t_blocks"] == 3 and d["launches"] == 7
    assert d["workspace_bytes"] == (rows + 3 * Cw + Cw + 4 * bins) * 4 == lib.gnan_attr_cols_workspace_bytes(a)
    assert describe(args(n_row_ids=0, **kw))["launches"] == 3                # an empty request: the fill, the walk, the product
    # a per-source chunk list replaces the uniform one; the dense layout is as long as the forward graph has rows
    a = args(item_ptr=P, n_items=7, **kw)
    assert describe(a)["n_items"] == 7 and lib.gnan_attr_cols_workspace_bytes(a) == (4 + 7) * bins * 4
    a = args(rowptr_t=None, row=None, n_rows=chunk + 1, max_col_pairs=0, **kw)
    assert describe(a)["max_col_chunks"] == 2
    assert describe(args(n_cols=0, **kw))["launches"] == 0
