"""Host side of ``gnan_attr_reduce`` (csrc/attr_reduce.hip): the ABI additions are declared, exported and bound under ABI 51, every
refusal happens before a HIP call (so all of this runs without a GPU), ``describe`` agrees with ``workspace_bytes``, and for rows of
at most one chunk the workspace holds nothing that grows as R * D * W."""
import ctypes
import os
import re

import pytest
import torch

import gnan_amd  # noqa: F401
from gnan_amd import _lib
from conftest import ROOT

FUNCS = ("gnan_attr_reduce", "gnan_attr_reduce_workspace_bytes", "gnan_attr_reduce_describe")
P = 0x1000                      # a non-null pointer value: nothing DEVICE-side is dereferenced before the refusals (or by describe)


def header():
    return open(os.path.join(ROOT, "include", "gnan_hip.h")).read()


def args(**kw):
    base = dict(n_rows=4, n_cols=300, rowptr=P, col=P, code=P, S=P, W=8, s_stride=8, lut=P, D=5, Cw=1, max_row_pairs=10,
                n_blocks=1, block_count=1, combine=1, partials=P, partials_bytes=1 << 40, M=P)
    base.update(kw)
    return _lib.AttrReduceArgs(**base)


def describe(a):
    info = _lib.AttrReduceInfo()
    assert _lib.lib().gnan_attr_reduce_describe(a, info) == 0, _lib.lib().gnan_last_error()
    return info.as_dict()


def refused(a, code, text):
    lib = _lib.lib()
    assert lib.gnan_attr_reduce(a, None) == code, lib.gnan_last_error()
    msg = lib.gnan_last_error().decode()
    assert text in msg, msg
    return msg


def host_ptr(values):
    t = torch.tensor(values, dtype=torch.int64)
    return t, t.data_ptr()


def test_declared_exported_and_bound_under_abi_51():
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for f in FUNCS:
        assert re.search(r"\b%s\s*\(" % f, text), f
        assert hasattr(handle, f) and f in _lib.SYMBOLS, f
    for s in ("gnan_attr_reduce_args", "gnan_attr_reduce_info"):
        assert re.search(r"typedef struct %s \{" % s, text), s
    assert "#define GNAN_ABI_VERSION 51" in header()
    assert _lib.ABI_VERSION == 51 and _lib.lib().gnan_abi_version() == 51


def test_ctypes_field_order_matches_the_header():
    text = header()
    for struct, cls in (("gnan_attr_reduce_args", _lib.AttrReduceArgs), ("gnan_attr_reduce_info", _lib.AttrReduceInfo)):
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
    assert lib.gnan_attr_reduce(None, None) == _lib.ERR_BAD_ARG and b"null args" in lib.gnan_last_error()
    for name in ("code", "S", "lut", "partials", "M"):
        refused(args(**{name: None}), _lib.ERR_BAD_ARG, "null")
    assert "D=1" in refused(args(D=1), _lib.ERR_UNSUPPORTED, "2 <= D <= 256")
    assert "D=257" in refused(args(D=257), _lib.ERR_UNSUPPORTED, "2 <= D <= 256")
    assert "W must be >= 1 (got 0)" in refused(args(W=0), _lib.ERR_BAD_ARG, "W must be")
    assert "Cw=3, W=8" in refused(args(Cw=3), _lib.ERR_BAD_ARG, "Cw must divide W")
    refused(args(col=None), _lib.ERR_BAD_ARG, "rowptr and col must both be set (CSR) or both NULL (dense)")
    refused(args(rowptr=None), _lib.ERR_BAD_ARG, "rowptr and col")
    refused(args(s_stride=7), _lib.ERR_BAD_ARG, "operand row stride")
    refused(args(cnt=P, cnt_stride=4), _lib.ERR_BAD_ARG, "cnt row stride")
    refused(args(lut_row_stride=4), _lib.ERR_BAD_ARG, "lut_row_stride")
    # the plan: block count, block range, partials
    assert "1 blocks" in refused(args(n_blocks=2), _lib.ERR_BAD_ARG, "the plan must hold")
    refused(args(block_first=1), _lib.ERR_BAD_ARG, "outside the plan")
    refused(args(block_count=-1), _lib.ERR_BAD_ARG, "outside the plan")
    refused(args(item_ptr=P, item_count=-1), _lib.ERR_BAD_ARG, "negative item range")
    need = 3 * 6 * 8 * 8
    assert str(need) in refused(args(partials_bytes=need - 8), _lib.ERR_BAD_ARG, "partials")
    # group_ptr, where the host can see it
    for bad, text in (([0, 3, 2, 4], "not monotone at group 1"), ([1, 2, 4], "must start at 0"), ([0, 2, 3], "must end at the number"),
                      ([0, 2, 5], "must end at the number")):
        keep, ptr = host_ptr(bad)
        refused(args(group_ptr=ptr, n_groups=len(bad) - 1, block_ptr=P, group_block_ptr=P, n_blocks=len(bad) - 1), _lib.ERR_BAD_ARG, text)
        info = _lib.AttrReduceInfo()
        assert lib.gnan_attr_reduce_describe(args(group_ptr=ptr, n_groups=len(bad) - 1), info) == _lib.ERR_BAD_ARG
        assert lib.gnan_attr_reduce_workspace_bytes(args(group_ptr=ptr, n_groups=len(bad) - 1)) == 0
    keep, ptr = host_ptr([0, 1, 1, 4])
    refused(args(group_ptr=ptr, n_groups=3, n_blocks=2), _lib.ERR_BAD_ARG, "group_ptr needs block_ptr and group_block_ptr")
    assert "2 blocks" in refused(args(group_ptr=ptr, n_groups=3, n_blocks=3, block_ptr=P, group_block_ptr=P), _lib.ERR_BAD_ARG,
                                 "the plan must hold")
    info = _lib.AttrReduceInfo()
    assert lib.gnan_attr_reduce_describe(args(), None) == _lib.ERR_BAD_ARG
    assert lib.gnan_attr_reduce_describe(args(D=257), info) == _lib.ERR_UNSUPPORTED


def test_short_workspace_is_refused_with_both_sizes():
    chunk = describe(args())["chunk_pairs"]
    a = args(max_row_pairs=2 * chunk + 3)
    need = _lib.lib().gnan_attr_reduce_workspace_bytes(a)
    assert need == 4 * 3 * 5 * 8 * 4                                       # rows x chunks x D x W floats
    msg = refused(a, _lib.ERR_WORKSPACE, "workspace")
    assert str(need) in msg
    a.workspace, a.workspace_bytes = P, need - 4
    assert str(need - 4) in refused(a, _lib.ERR_WORKSPACE, str(need))


@pytest.mark.parametrize("W,D", [(1, 2), (3, 3), (15, 8), (63, 9), (64, 64), (65, 65), (130, 256)])
def test_describe_is_consistent_with_workspace_bytes(W, D):
    lib = _lib.lib()
    base = describe(args(W=W, s_stride=W, D=D))
    chunk, br, ps = base["chunk_pairs"], base["block_rows"], base["pass_shells"]
    assert base["col_tiles"] == -(-W // 64) and base["shell_passes"] == -(-D // ps) and base["block_size"] == 256
    assert base["launches"] == 2 and base["n_blocks"] == 1 and base["n_long_items"] == 0 and base["long_items_bytes"] == 0
    assert base["partials_bytes"] == 3 * (D + 1) * W * 8 and base["plan_int_bytes"] == 0
    assert base["lds_bytes"] <= 64 * 1024 and br % 4 == 0
    for pairs, chunks in ((0, 0), (1, 0), (chunk - 1, 0), (chunk, 0), (chunk + 1, 2), (2 * chunk + 3, 3)):
        d = describe(args(W=W, s_stride=W, D=D, max_row_pairs=pairs))
        assert d["n_long_items"] == 4 * chunks and d["launches"] == 2 + (chunks > 0)
        assert d["long_items_bytes"] == 4 * chunks * D * W * 4 == lib.gnan_attr_reduce_workspace_bytes(
            args(W=W, s_stride=W, D=D, max_row_pairs=pairs))
    # a list of the long rows' chunk items replaces the uniform one: this call's range sizes the workspace
    a = args(W=W, s_stride=W, D=D, max_row_pairs=10 * chunk, item_ptr=P, item_first=3, item_count=7)
    d = describe(a)
    assert d["n_long_items"] == 7 and d["long_items_bytes"] == lib.gnan_attr_reduce_workspace_bytes(a) == 7 * D * W * 4
    assert d["plan_int_bytes"] == 5 * 4
    # the dense layout is as long as it is wide; a range of blocks sizes the uniform chunk list by its rows
    a = args(W=W, s_stride=W, D=D, rowptr=None, col=None, n_cols=chunk + 1, max_row_pairs=0, n_rows=2 * br + 1, n_blocks=3,
             block_first=1, block_count=2)
    assert describe(a)["n_long_items"] == (br + 1) * 2 and describe(a)["n_blocks"] == 3
    # groups: blocks never straddle a boundary, an empty group has none
    keep, ptr = host_ptr([0, 1, 1, br + 2, 2 * br + 2])
    d = describe(args(W=W, s_stride=W, D=D, n_rows=2 * br + 2, group_ptr=ptr, n_groups=4, block_ptr=P, group_block_ptr=P))
    assert d["n_blocks"] == 1 + 0 + 2 + 1 and d["plan_int_bytes"] == 5 * 8 + 5 * 8
    assert describe(args(W=W, s_stride=W, D=D, n_rows=0, n_blocks=0, block_count=0))["launches"] == 1         # M is zeroed
    assert describe(args(W=W, s_stride=W, D=D, n_rows=0, n_blocks=0, block_count=0, combine=0))["launches"] == 0


@pytest.mark.parametrize("D", [4, 65])
def test_nothing_in_the_workspace_grows_as_r_d_w_for_rows_of_one_chunk(D):
    """Doubling R at a fixed block count changes the O(R) integer part only; more blocks add block partials, never row terms."""
    W = 129
    br = describe(args(W=W, s_stride=W, D=D))["block_rows"]
    chunk = describe(args(W=W, s_stride=W, D=D))["chunk_pairs"]
    one = describe(args(W=W, s_stride=W, D=D, n_rows=br // 2, max_row_pairs=chunk, item_ptr=P))
    two = describe(args(W=W, s_stride=W, D=D, n_rows=br, max_row_pairs=chunk, item_ptr=P))
    assert one["n_blocks"] == two["n_blocks"] == 1
    assert one["long_items_bytes"] == two["long_items_bytes"] == 0 and one["partials_bytes"] == two["partials_bytes"]
    assert two["plan_int_bytes"] - one["plan_int_bytes"] == 4 * (br - br // 2)
    many = describe(args(W=W, s_stride=W, D=D, n_rows=1000 * br, max_row_pairs=chunk, item_ptr=P))
    assert many["long_items_bytes"] == 0 and many["partials_bytes"] == 1000 * 3 * (D + 1) * W * 8
    assert many["partials_bytes"] < (1000 * br * D * W * 4) // 4                  # under a quarter of the R * D * W floats it replaces
