"""Host side of pre-rho normalisation (GNAN.py:65-67) on the one-launch route for dense-coded graphs of 129 to 448 nodes
(csrc/mid_graph.hip with ``reserved = GNAN_MID_PRE_RHO``): the two new queries are exported, declared and bound; the route query's
grids, LDS and workspaces over the WHOLE admitted domain; the refusals before any HIP call; the Python predicate's edges.  No GPU."""
import ctypes
import re
import types

import pytest
import torch

from gnan_amd import _lib
from gnan_amd import small_graph as sg
from gnan_amd.functional import StackedMLP
from test_mid_graph_host import _bwd_args, _FakeCuda, _fwd_args, _mlp, header

SYMBOLS = ("gnan_mid_graph_pre_bwd_workspace_bytes", "gnan_mid_graph_pre_describe")
PRE = 1                       # GNAN_MID_PRE_RHO
RHO_SLOT = 64 * 64 + 5 * 64   # floats of one rho group's partial gradients: W2, then five vectors of 64


def test_symbols_are_exported_declared_and_bound():
    handle = ctypes.CDLL(_lib.LIB_PATH)
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    for name in SYMBOLS:
        assert hasattr(handle, name), f"{name} not exported"
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} not declared"
        assert name in _lib.SYMBOLS, f"{name} not bound"
        assert getattr(_lib.lib(), name).argtypes == _lib.SYMBOLS[name][1]
    assert re.search(r"^#define GNAN_MID_PRE_RHO %d\b" % PRE, header(), re.M)
    # entry points and a flag value were ADDED: no struct changed, the number did not move
    assert _lib.lib().gnan_abi_version() == _lib.ABI_VERSION == 51
    for struct in ("gnan_mid_graph_args", "gnan_mid_graph_bwd_args"):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header(), flags=re.S).group(1)
        assert re.search(r"int32_t D;\s*int32_t reserved;", body), struct


def test_grids_lds_and_workspaces_over_the_whole_domain():
    """Every admitted (n, D, C): F + R forward workgroups with R = ceil(ceil(n D / 64) / ceil(n / 64)) — no rho workgroup runs more
    MLP passes than a feature workgroup —, F + ceil(n / 32) backward workgroups, both kernels within 96 KB of LDS (two workgroups
    per compute unit, the route's aim), and the workspace sizes the queries return."""
    lib = _lib.lib()
    info, plain = _lib.MidGraphInfo(), _lib.MidGraphInfo()
    F = 15
    most_rho = 0
    for n in range(129, 449):
        tiles, groups = -(-n // 64), -(-n // 32)
        for D in (2, 17, 64):
            passes = -(-n * D // 64)
            R = -(-passes // tiles)
            assert R * tiles >= passes and (R - 1) * tiles < passes
            for C in (1, 8):
                assert lib.gnan_mid_graph_pre_describe(n, F, D, C, info) == 0, (n, D, C, lib.gnan_last_error())
                assert info.row_tiles == tiles and info.rho_groups == groups, (n, info.as_dict())
                assert info.fwd_grid == F + R and info.bwd_grid == F + groups, (n, D, info.as_dict())
                assert 0 < info.fwd_lds_bytes <= 96 * 1024 and 0 < info.bwd_lds_bytes <= 96 * 1024, (n, D, C, info.as_dict())
                assert info.fwd_workspace_bytes == lib.gnan_mid_graph_workspace_bytes(n, F, C)
                assert info.bwd_workspace_bytes == lib.gnan_mid_graph_pre_bwd_workspace_bytes(n, D) == 16 + groups * RHO_SLOT * 4
                assert lib.gnan_mid_graph_describe(n, F, D, C, plain) == 0
                assert plain.fwd_grid == F + 1 and plain.bwd_workspace_bytes == lib.gnan_mid_graph_bwd_workspace_bytes(n, D)
                most_rho = max(most_rho, R)
    assert most_rho == 64                                        # 448 nodes x 64 shells
    assert lib.gnan_mid_graph_pre_bwd_workspace_bytes(448, 64) == 247312
    for n, D, C, named in ((449, 12, 1, b"n=449"), (200, 65, 1, b"D=65"), (200, 12, 9, b"C=9")):
        assert lib.gnan_mid_graph_pre_describe(n, F, D, C, info) == _lib.ERR_UNSUPPORTED and named in lib.gnan_last_error()


def _calls():
    lib = _lib.lib()
    drop = _lib.SmallDropout(p=0.5, reserved=0, seed=7)
    dev = _lib.SmallDropoutDev(p=0.5, reserved=0, seed=0x800000)
    return [("fwd", lambda a: lib.gnan_mid_graph_fwd(a, None)), ("bwd", lambda a: lib.gnan_mid_graph_bwd(a, None)),
            ("fwd", lambda a: lib.gnan_mid_graph_fwd_drop(a, drop, None)), ("bwd", lambda a: lib.gnan_mid_graph_bwd_drop(a, drop, None)),
            ("fwd", lambda a: lib.gnan_mid_graph_fwd_drop_dev(a, dev, None)),
            ("bwd", lambda a: lib.gnan_mid_graph_bwd_drop_dev(a, dev, None))]


def _pre_bwd_args(n=200, D=12, **over):
    kw = dict(reserved=PRE, workspace_bytes=_lib.lib().gnan_mid_graph_pre_bwd_workspace_bytes(n, D))
    kw.update(over)
    return _bwd_args(n=n, D=D, **kw)


def _args(which, **over):
    return _fwd_args(**{"reserved": PRE, **over}) if which == "fwd" else _pre_bwd_args(**over)


def test_the_flag_and_the_pre_rho_refusals_come_before_any_hip_call():
    """A null stream and made-up addresses on a machine without a GPU: every refusal is the host-side validator's, on all six entry
    points."""
    lib = _lib.lib()
    for which, call in _calls():
        assert call(_args(which, reserved=2)) == _lib.ERR_BAD_ARG, which
        assert b"reserved=2" in lib.gnan_last_error()
        assert call(_args(which, reserved=-1)) == _lib.ERR_BAD_ARG and b"reserved=-1" in lib.gnan_last_error()
        # without the shell sizes: refused as gnan_small_graph_fwd refuses it
        assert call(_args(which, cnt=None, cnt_stride=0)) == _lib.ERR_UNSUPPORTED, which
        assert b"shell sizes" in lib.gnan_last_error()
        for kw, named in ((dict(rho=_mlp(C=2, bias=False, base=0x2000)), b"rho.C=2"), (dict(D=65), b"D=65"), (dict(n=449), b"n=449")):
            assert call(_args(which, **kw)) == _lib.ERR_UNSUPPORTED, (which, named)
            assert named in lib.gnan_last_error(), (which, lib.gnan_last_error())
    small = _lib.SmallGraphArgs(x=0x100000, x_stride=15, n=100, F=15, f=_mlp(), rho=_mlp(bias=False, base=0x2000), code=0x200000, D=12,
                                pre_rho=1, cnt=None, cnt_stride=0, S=0x400000, lut=0x500000, Y=None, Ysum=0x600000,
                                workspace=0x700000, workspace_bytes=1 << 20)
    assert lib.gnan_small_graph_fwd(small, None) == _lib.ERR_UNSUPPORTED          # (... which is this)


def test_the_backward_workspace_under_pre_rho():
    lib = _lib.lib()
    need, plain = lib.gnan_mid_graph_pre_bwd_workspace_bytes(200, 12), lib.gnan_mid_graph_bwd_workspace_bytes(200, 12)
    assert need == 16 + 7 * RHO_SLOT * 4 > plain
    assert lib.gnan_mid_graph_bwd(_pre_bwd_args(workspace_bytes=need - 1), None) == _lib.ERR_WORKSPACE
    assert str(need).encode() in lib.gnan_last_error() and str(need - 1).encode() in lib.gnan_last_error()
    assert lib.gnan_mid_graph_bwd(_pre_bwd_args(workspace_bytes=plain), None) == _lib.ERR_WORKSPACE
    assert lib.gnan_mid_graph_bwd(_pre_bwd_args(workspace=0x700004), None) == _lib.ERR_BAD_ARG and b"aligned" in lib.gnan_last_error()
    # reserved = 0 still takes today's smaller workspace: with exactly that size the next check behind it (alignment) speaks
    assert lib.gnan_mid_graph_bwd(_bwd_args(workspace_bytes=plain - 1), None) == _lib.ERR_WORKSPACE
    assert lib.gnan_mid_graph_bwd(_bwd_args(workspace_bytes=plain, workspace=0x700004), None) == _lib.ERR_BAD_ARG
    assert b"aligned" in lib.gnan_last_error()                    # (the check BEHIND the workspace's size: the size was accepted)
    assert lib.gnan_mid_graph_bwd(_pre_bwd_args(workspace_bytes=need, workspace=0x700004), None) == _lib.ERR_BAD_ARG
    assert b"aligned" in lib.gnan_last_error()
    # the forward's workspace is the plain one
    fneed = lib.gnan_mid_graph_workspace_bytes(200, 15, 1)
    assert lib.gnan_mid_graph_fwd(_fwd_args(reserved=PRE, workspace_bytes=fneed - 1), None) == _lib.ERR_WORKSPACE


@pytest.fixture
def switch_on(monkeypatch):
    monkeypatch.setattr(sg, "MID_GRAPH_PRE_RHO", True)


def test_the_predicate(switch_on, monkeypatch):
    F = 5
    t = lambda *s: torch.zeros(*s)        # noqa: E731
    f = StackedMLP(t(F, 8), t(F, 8), t(1, F, 8, 8), t(1, F, 8), t(F, 1, 8), t(F, 1), 3, 8, 1, F)
    rho = StackedMLP(t(1, 8), t(1, 8), t(1, 1, 8, 8), t(1, 1, 8), t(1, 1, 8), t(1, 1), 3, 8, 1, 1)
    rho2 = StackedMLP(t(1, 8), None, t(1, 1, 8, 8), None, t(1, 2, 8), None, 3, 8, 2, 1)
    f2 = StackedMLP(t(F, 8), t(F, 8), t(1, F, 8, 8), t(1, F, 8), t(F, 2, 8), t(F, 2), 3, 8, 2, F)

    def dense(n, codes=2, cnt=True):
        return types.SimpleNamespace(is_dense=True, n_rows=n, n_cols=n, n_codes=codes,
                                     cnt=torch.ones(n, codes, dtype=torch.int32) if cnt else None)
    assert isinstance(sg.MID_GRAPH_PRE_RHO, bool)
    assert sg.mid_graph_pre_rho_applies(_FakeCuda(129, F), dense(129), f, rho)
    assert sg.mid_graph_pre_rho_applies(_FakeCuda(448, F), dense(448, 64), f, rho)
    assert sg.mid_graph_pre_rho_applies(_FakeCuda(200, F), dense(200), f2, rho)              # two channels of f, one of rho
    assert not sg.mid_graph_pre_rho_applies(torch.zeros(129, F), dense(129), f, rho)         # CPU tensors
    assert not sg.mid_graph_pre_rho_applies(_FakeCuda(128, F), dense(128), f, rho)           # the small route's
    assert not sg.mid_graph_pre_rho_applies(_FakeCuda(449, F), dense(449), f, rho)
    assert not sg.mid_graph_pre_rho_applies(_FakeCuda(129, F), dense(129, cnt=False), f, rho)
    assert not sg.mid_graph_pre_rho_applies(_FakeCuda(129, F), dense(129), f2, rho2)         # a rho channel per output channel
    assert not sg.mid_graph_pre_rho_applies(_FakeCuda(129, F), dense(129, 65), f, rho)
    assert not sg.mid_graph_pre_rho_applies(_FakeCuda(129, F, requires_grad=True), dense(129), f, rho)
    assert not sg.mid_graph_pre_rho_applies(_FakeCuda(129, F + 1), dense(129), f, rho)
    # mid_graph_applies is what it was: it keeps refusing "pre", whatever the new switch says
    assert not sg.mid_graph_applies(_FakeCuda(129, F), dense(129), f, rho, use_cnt="pre")
    assert sg.mid_graph_applies(_FakeCuda(129, F), dense(129), f, rho)
    for name in ("MID_GRAPH_PRE_RHO", "MID_GRAPH", "SMALL_GRAPH_BACKWARD", "SMALL_GRAPH_FORWARD"):
        with monkeypatch.context() as mp:
            mp.setattr(sg, name, False)
            assert not sg.mid_graph_pre_rho_applies(_FakeCuda(129, F), dense(129), f, rho), name
        assert sg.mid_graph_pre_rho_applies(_FakeCuda(129, F), dense(129), f, rho)
