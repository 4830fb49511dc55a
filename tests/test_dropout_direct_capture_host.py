"""Host side of the Dropout seed cell of the DIRECT kernels: the five ``_dev`` entry points — declared, exported and bound under
ABI 51 — their refusals (all on the host before any HIP call), the switch's default and the truth table of
``functional.dropout_direct_capture_applies`` on fake tensors.  None of this needs a GPU."""
import ctypes
import os
import re
import types

import pytest
import torch

from gnan_amd import _lib
from gnan_amd import functional as Fn
from conftest import ROOT

ENTRY_POINTS = {
    "gnan_fmlp_fwd_dev": (_lib.FmlpArgs, "gnan_fmlp_args", "fmlp_fwd_dev", "gnan_fmlp_fwd"),
    "gnan_fmlp_bwd_dev": (_lib.FmlpBwdArgs, "gnan_fmlp_bwd_args", "fmlp_bwd_dev", "gnan_fmlp_bwd"),
    "gnan_fmlp_bwd_mfma_dev": (_lib.FmlpBwdArgs, "gnan_fmlp_bwd_args", "fmlp_bwd_mfma_dev", "gnan_fmlp_bwd_mfma"),
    "gnan_fmlp_mc_fwd_dev": (_lib.FmlpArgs, "gnan_fmlp_args", "fmlp_mc_fwd_dev", "gnan_fmlp_mc_fwd"),
    "gnan_fmlp_mc_bwd_dev": (_lib.FmlpBwdArgs, "gnan_fmlp_bwd_args", "fmlp_mc_bwd_dev", "gnan_fmlp_mc_bwd"),
}
CELL = 0x1000          # a non-NULL "device" address: no refusal under test ever follows it


def _header():
    return open(os.path.join(ROOT, "include", "gnan_hip.h")).read()


def _args(cls, **more):
    """A record of sizes every one of the five covers (n > 0, no pointers: the by-value entry point's pointer checks refuse it)."""
    kw = dict(n=40, x_stride=3, F=3, L=3, H=32, C=1 if "mc" not in more.pop("name", "") else 16)
    kw.update(more)
    return cls(**kw)


def test_the_five_entry_points_are_declared_exported_and_bound_under_abi_51():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    handle = ctypes.CDLL(_lib.LIB_PATH)
    assert _lib.ABI_VERSION == 51 and handle.gnan_abi_version() == 51
    assert re.search(r"#define GNAN_ABI_VERSION 51\b", _header())
    for name, (cls, ctype, _, plain) in ENTRY_POINTS.items():
        assert re.search(r"\bint %s\(const %s\* a, const uint64_t\* seed_cell, gnan_stream_t stream\);" % (name, ctype), text), name
        assert hasattr(handle, name), name
        assert _lib.SYMBOLS[name] == (ctypes.c_int, [ctypes.POINTER(cls), ctypes.c_void_p, ctypes.c_void_p]), name
        assert getattr(_lib.lib(), name).argtypes == _lib.SYMBOLS[name][1]
        # the by-value entry point and its record did not move
        assert _lib.SYMBOLS[plain] == (ctypes.c_int, [ctypes.POINTER(cls), ctypes.c_void_p])
    assert [f[0] for f in _lib.FmlpArgs._fields_][-2:] == ["dropout_p", "dropout_seed"]
    assert [f[0] for f in _lib.FmlpBwdArgs._fields_][-2:] == ["dropout_p", "dropout_seed"]


@pytest.mark.parametrize("name", sorted(ENTRY_POINTS))
def test_a_bad_seed_is_refused_before_any_hip_call(name):
    cls, _, who, plain = ENTRY_POINTS[name]
    lib = _lib.lib()
    fn = getattr(lib, name)
    assert fn(None, CELL, None) == _lib.ERR_BAD_ARG and b"null args" in lib.gnan_last_error()
    for p in (1.0, 1.5, -0.25, float("nan"), float("inf")):
        # (a bad p wins over a by-value seed and a NULL cell)
        assert fn(_args(cls, name=name, dropout_p=p, dropout_seed=7), None, None) == _lib.ERR_BAD_ARG, p
        said = lib.gnan_last_error()
        assert said.startswith(who.encode() + b":") and b"dropout_p must be in [0, 1)" in said, (p, said)
    for p in (0.0, 0.6):
        # a seed by value in the record: the cell is the seed (it wins over a NULL cell)
        assert fn(_args(cls, name=name, dropout_p=p, dropout_seed=7), None, None) == _lib.ERR_BAD_ARG
        said = lib.gnan_last_error()
        assert said.startswith(who.encode() + b":") and b"dropout_seed must be 0" in said and b"dropout_seed=7" in said, said
    assert fn(_args(cls, name=name, dropout_p=0.6), None, None) == _lib.ERR_BAD_ARG
    said = lib.gnan_last_error()
    assert said.startswith(who.encode() + b":") and b"null dropout seed cell" in said, said
    # a good seed — and p == 0 with a NULL cell, which is never read — goes on to the by-value entry point's own checks, with its
    # messages: these sizes are covered, the pointers are missing
    for p, cell in ((0.6, CELL), (0.0, CELL), (0.0, None)):
        a = _args(cls, name=name, dropout_p=p)
        assert fn(a, cell, None) == _lib.ERR_BAD_ARG
        mine = lib.gnan_last_error()
        assert b"null" in mine and b"dropout" not in mine, mine
        assert getattr(lib, plain)(a, None) == _lib.ERR_BAD_ARG and lib.gnan_last_error() == mine


@pytest.mark.parametrize("name", sorted(ENTRY_POINTS))
def test_shapes_outside_the_cover_stay_unsupported(name):
    """... with the by-value entry point's message; the lane forward covers every shape, so it has none."""
    cls, _, who, plain = ENTRY_POINTS[name]
    lib = _lib.lib()
    if name == "gnan_fmlp_fwd_dev":
        a = _args(cls, name=name, dropout_p=0.6, algo=_lib.FMLP_MFMA, C=9, x=CELL, out=CELL, w_last=CELL, w_first=CELL, w_mid=CELL,
                  out_stride=27)
    else:
        a = _args(cls, name=name, dropout_p=0.6, H=65)
    assert getattr(lib, name)(a, CELL, None) == _lib.ERR_UNSUPPORTED
    mine = lib.gnan_last_error()
    assert b"covers" in mine, mine
    assert getattr(lib, plain)(a, None) == _lib.ERR_UNSUPPORTED and lib.gnan_last_error() == mine


def test_the_workspace_queries_are_the_by_value_ones():
    """No query of their own: the five take the by-value entry points' workspaces."""
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert not re.search(r"gnan_fmlp\w*_dev_workspace_bytes|gnan_fmlp\w*_workspace_bytes_dev", text)
    assert not [s for s in _lib.SYMBOLS if "fmlp" in s and "_dev" in s and "workspace" in s]


def test_the_switch_ships_off():
    assert Fn.CAPTURE_DROPOUT_DIRECT is False


# ---- the predicate ---------------------------------------------------------------------------------------------------------------
def _x(n, F, dtype=torch.float32, requires_grad=False):
    return types.SimpleNamespace(shape=(n, F), dtype=dtype, requires_grad=requires_grad, is_cuda=True)


def _g(n, dense=False, n_codes=5):
    return types.SimpleNamespace(is_dense=dense, n_rows=n, n_cols=n, n_codes=n_codes, cnt=object())


def _model(kind="tensor", F=4, C=3, L=3, H=16, **kw):
    from gnan_amd import batched, modules
    if kind == "tensor":
        m = modules.TensorGNAN(F, C, L, hidden_channels=H, dropout=0.6, **kw)
    elif kind == "standalone":
        m = modules.StandaloneTensorGNAN(F, C, L, hidden_channels=H, dropout=0.6, **kw)
    elif kind == "gnan":
        m = modules.GNAN(F, C, L, hidden_channels=H, dropout=0.6, **kw)
    else:
        m = batched.TensorGNAN(F, C, 2, hidden_channels=H, dropout=0.6, **kw)
    return m.train()


@pytest.fixture()
def switch_on(monkeypatch):
    monkeypatch.setattr(Fn, "CAPTURE_DROPOUT_DIRECT", True)


def test_the_predicate_is_false_with_the_switch_off():
    assert not Fn.dropout_direct_capture_applies(_model(), _x(600, 4), _g(600))


@pytest.mark.parametrize("kind", ["tensor", "standalone", "gnan"])
@pytest.mark.parametrize("L,H,C", [(2, 8, 1), (3, 64, 8), (3, 16, 3)])
def test_the_general_route_inside_a_kernel_backwards_cover(switch_on, kind, L, H, C):
    m = _model(kind, L=L, H=H, C=C)
    assert Fn.dropout_direct_capture_applies(m, _x(600, 4), _g(600)) is True             # a CSR-coded graph
    assert Fn.dropout_direct_capture_applies(m, _x(449, 4), _g(449, dense=True)) is True  # dense, past the one-launch routes
    assert Fn.dropout_direct_capture_applies(m, _x(11758, 4), _g(11758)) is True


def test_many_channels_from_the_measured_size_on(switch_on):
    m = _model(F=4, C=40, L=3, H=64)
    big = -(-Fn.DROPOUT_MC_MIN_WORK // 4)
    assert Fn.dropout_direct_capture_applies(m, _x(big, 4), _g(big)) is True
    assert Fn.dropout_direct_capture_applies(m, _x(big - 1, 4), _g(big - 1)) is False      # C = 40 at small n: the restatement
    assert Fn.dropout_direct_capture_applies(_model(F=4, C=65, L=3, H=64), _x(big, 4), _g(big)) is False
    assert Fn.dropout_direct_capture_applies(_model(F=4, C=40, L=2, H=64), _x(big, 4), _g(big)) is False


def test_everything_out_of_scope_stays_eager(switch_on):
    m = _model()
    assert Fn.dropout_direct_capture_applies(m, _x(600, 4), _g(600), node_ids=[1, 2]) is False
    assert Fn.dropout_direct_capture_applies(m, _x(600, 4, requires_grad=True), _g(600)) is False
    assert Fn.dropout_direct_capture_applies(m, _x(600, 4, dtype=torch.float64), _g(600)) is False
    assert Fn.dropout_direct_capture_applies(m, _x(600, 4, dtype=torch.bfloat16), _g(600)) is False
    assert Fn.dropout_direct_capture_applies(_model(L=4), _x(600, 4), _g(600)) is False
    assert Fn.dropout_direct_capture_applies(_model(H=128), _x(600, 4), _g(600)) is False
    assert Fn.dropout_direct_capture_applies(_model(H=65), _x(600, 4), _g(600)) is False
    assert Fn.dropout_direct_capture_applies(_model(C=9), _x(600, 4), _g(600)) is False
    nam = _model(C=2, is_graph_task=True, readout_n_layers=2)
    assert Fn.dropout_direct_capture_applies(nam, _x(600, 4), _g(600)) is False
    assert Fn.dropout_direct_capture_applies(_model(C=2, is_graph_task=True, readout_n_layers=0), _x(600, 4), _g(600)) is True
    assert Fn.dropout_direct_capture_applies(_model("batched", C=1), _x(600, 4), _g(600)) is False
    assert Fn.dropout_direct_capture_applies(torch.nn.Linear(2, 2), _x(600, 4), _g(600)) is False


def test_a_forward_the_one_launch_routes_take_is_theirs(switch_on):
    """A dense graph of up to 448 nodes that a one-launch route takes eagerly is not the general route's: the other predicate's."""
    from gnan_amd import small_graph as sg
    m = _model(C=1)
    for n in (30, 200, 448):
        assert Fn.dropout_direct_capture_applies(m, _x(n, 4), _g(n, dense=True)) is False, n
    assert Fn.dropout_direct_capture_applies(m, _x(200, 4), _g(200)) is True                  # the same sizes, CSR-coded
    assert Fn.dropout_direct_capture_applies(m, _x(200, 4), _g(200, dense=True, n_codes=65)) is True    # more shells than they hold
    assert Fn.dropout_direct_capture_applies(m, _x(30, 4), sg.SlotGraph.__new__(sg.SlotGraph)) is False  # a graph in slots


def test_the_other_predicate_keeps_its_answers(switch_on, monkeypatch):
    from gnan_amd import small_graph as sg
    monkeypatch.setattr(sg, "CAPTURE_DROPOUT", True)
    m = _model(C=1)
    assert sg.dropout_capture_applies(m, _x(600, 4), _g(600)) is False
    assert sg.dropout_capture_applies(m, _x(449, 4), _g(449, dense=True)) is False
