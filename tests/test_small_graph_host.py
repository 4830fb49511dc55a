"""Host side of the one-launch routes for dense-coded graphs of up to 128 nodes (csrc/small_graph.hip, csrc/small_graph_nam.hip):
what the six launching entry points refuse, with which status and — for shapes outside the cover — naming the offending value;
the four Python predicates at every limit and one past it.  Made-up addresses and a null stream: every refusal comes from the host
checks, before any HIP call.  No GPU.  (csrc/mid_graph.hip's two entry points: tests/test_mid_graph_host.py.)"""
import types

import pytest
import torch

from gnan_amd import _lib
from gnan_amd import small_graph as sg
from gnan_amd.functional import StackedMLP
from test_mid_graph_host import _FakeCuda, _grads, _mlp
from test_mid_graph_host import _bwd_args as _mid_bwd
from test_mid_graph_host import _fwd_args as _mid_fwd

BAD_ARG, UNSUPPORTED, WORKSPACE = _lib.ERR_BAD_ARG, _lib.ERR_UNSUPPORTED, _lib.ERR_WORKSPACE


def _rho(**kw):
    return _mlp(**{"bias": False, "base": 0x2000, **kw})


def _nam(**kw):
    return _mlp(**{"C": 2, "base": 0x3000, **kw})


def _linear_nam(C=2):
    """The one-layer read-out (Linear(1, C) per feature): only the last layer exists."""
    return _lib.SmallMlp(L=1, H=0, C=C, w_first=None, b_first=None, w_mid=None, b_mid=None, w_last=0x3400, b_last=0x3500)


def _grads_of(m, base=0x9000):
    """Gradient pointers that match ``m``'s pointers whatever its depth (a depth outside the cover is the cover's to refuse)."""
    g = _grads(m, base)
    if m.L != 2:
        g.w_mid = base + 0x200
    return g


def _linear_grads(m):
    return _lib.SmallMlpGrads(w_first=None, b_first=None, w_mid=None, b_mid=None, w_last=0xB400, b_last=0xB500 if m.b_last else None)


def _graph_args(cls, workspace_bytes, short=0, **over):
    """One graph: the fields gnan_small_graph_args, _bwd_args, _nam_args and _nam_bwd_args share."""
    kw = dict(x=0x100000, x_stride=15, n=100, F=15, f=_mlp(), rho=_rho(), code=0x200000, D=12, cnt=0x300000, cnt_stride=12,
              lut=0x500000, workspace=0x700000)
    kw.update(over)
    kw.setdefault("workspace_bytes", workspace_bytes(kw) - short)
    return cls(**kw)


def _small_fwd(**over):
    return _graph_args(_lib.SmallGraphArgs, lambda kw: _lib.lib().gnan_small_graph_workspace_bytes(kw["n"], kw["F"], kw["f"].C),
                       **{"pre_rho": 0, "S": 0x400000, "Y": None, "Ysum": 0x600000, **over})


def _small_bwd(**over):
    kw = {"pre_rho": 0, "S": 0x400000, "dY": None, "dYsum": 0x600000, **over}
    kw.setdefault("df", _grads_of(kw.get("f") or _mlp()))
    kw.setdefault("drho", _grads_of(kw.get("rho") or _rho(), 0xA000))
    return _graph_args(_lib.SmallGraphBwdArgs, lambda kw: _lib.lib().gnan_small_graph_bwd_workspace_bytes(kw["n"], kw["D"]), **kw)


def _nam_bytes(kw):
    return _lib.lib().gnan_small_graph_nam_workspace_bytes(kw["F"], kw["nam"].C)


def _nam_fwd(**over):
    return _graph_args(_lib.SmallGraphNamArgs, _nam_bytes,
                       **{"nam": _nam(), "reserved": 0, "fx": 0x400000, "hidden": 0x600000, "out": 0x800000, **over})


def _nam_bwd(**over):
    kw = {"nam": _nam(), "reserved": 0, "fx": 0x400000, "hidden": 0x600000, "d_out": 0x800000, **over}
    kw.setdefault("df", _grads_of(kw.get("f") or _mlp()))
    kw.setdefault("drho", _grads_of(kw.get("rho") or _rho(), 0xA000))
    kw.setdefault("dnam", _linear_grads(kw["nam"]) if kw["nam"].L == 1 else _grads_of(kw["nam"], 0xB000))
    return _graph_args(_lib.SmallGraphNamBwdArgs, _nam_bytes, **kw)


def _batch_kw(over):
    kw = dict(x=0x100000, x_stride=15, total_nodes=150, F=15, n_graphs=2, max_nodes=100, f=_mlp(), rho=_rho(), code=0x200000,
              node_off=0x210000, code_off=0x220000, D=12, rho_raw_hops=1, rest_zero=1, S=0x400000, lut=0x500000, workspace=0x700000,
              cnt=None, cnt_stride=0)
    kw.update(over)
    if "n" in kw:                                        # (the cases below name the node count as the one-graph structs do)
        kw["max_nodes"] = kw.pop("n")
    return kw


def _batch_fwd(short=0, **over):
    kw = _batch_kw({"Y": None, "Ysum": 0x600000, **over})
    kw.setdefault("workspace_bytes",
                  _lib.lib().gnan_small_batch_workspace_bytes(kw["n_graphs"], kw["total_nodes"], kw["F"], kw["f"].C) - short)
    return _lib.SmallBatchArgs(**kw)


def _batch_bwd(short=0, **over):
    kw = _batch_kw({"dY": None, "dYsum": 0x600000, **over})
    kw.setdefault("df", _grads_of(kw["f"]))
    kw.setdefault("drho", _grads_of(kw["rho"], 0xA000))
    if "workspace_bytes" not in kw:
        kw["workspace_bytes"] = 0
        kw["workspace_bytes"] = _lib.lib().gnan_small_batch_bwd_workspace_bytes(_lib.SmallBatchBwdArgs(**kw)) - short
    return _lib.SmallBatchBwdArgs(**kw)


ENTRIES = {"small_fwd": ("gnan_small_graph_fwd", _small_fwd), "small_bwd": ("gnan_small_graph_bwd", _small_bwd),
           "nam_fwd": ("gnan_small_graph_nam_fwd", _nam_fwd), "nam_bwd": ("gnan_small_graph_nam_bwd", _nam_bwd),
           "batch_fwd": ("gnan_small_batch_fwd", _batch_fwd), "batch_bwd": ("gnan_small_batch_bwd", _batch_bwd),
           "mid_fwd": ("gnan_mid_graph_fwd", _mid_fwd), "mid_bwd": ("gnan_mid_graph_bwd", _mid_bwd)}
SMALL, NAM, BATCH = ("small_fwd", "small_bwd"), ("nam_fwd", "nam_bwd"), ("batch_fwd", "batch_bwd")
FWD_256 = ("small_fwd", "batch_fwd")                     # the two forwards that take up to 256 shells
BWD = ("small_bwd", "nam_bwd", "batch_bwd")


def _refused(entry, kw):
    lib = _lib.lib()
    symbol, make = ENTRIES[entry]
    return getattr(lib, symbol)(make(**kw), None), lib.gnan_last_error()


# one fault per case: (entry points, the fault, what the refusal names)
OUTSIDE_THE_COVER = [
    (SMALL + NAM + BATCH, dict(n=129), b"(got n=129)"),
    (FWD_256, dict(D=257, cnt=None), b"(got D=257)"),
    (("small_bwd", "batch_bwd") + NAM, dict(D=65, cnt_stride=65), b"(got D=65)"),
    (SMALL + BATCH, dict(f=_mlp(C=9)), b"(got C=9)"),
    (NAM, dict(nam=_nam(C=9)), b"(got C=9"),
    (NAM, dict(f=_mlp(C=2)), b"(got C=2)"),
    (SMALL + NAM + BATCH, dict(f=_mlp(H=65)), b"(got H=65 for f)"),
    (SMALL + NAM + BATCH, dict(rho=_rho(H=65)), b"(got H=65 for rho)"),
    (NAM, dict(nam=_nam(H=65)), b"(got H=65"),
    (SMALL + NAM + BATCH, dict(f=_mlp(L=4)), b"(got L=4 for f)"),
    (SMALL + NAM + BATCH, dict(rho=_rho(L=1)), b"(got L=1 for rho)"),
    (NAM, dict(nam=_nam(L=4)), b"(got L=4"),
    (("small_fwd",) + BATCH, dict(f=_mlp(C=3), rho=_rho(C=2)), b"(got rho.C=2)"),
    (("small_bwd",) + NAM, dict(rho=_rho(C=2)), b"(got rho.C=2)"),
    # the extra rules of single entry points
    (("small_fwd",), dict(pre_rho=1, cnt=None, cnt_stride=0), b"pre-rho"),
    (("small_fwd",), dict(pre_rho=1, D=65, cnt_stride=65), b"D=65"),
    (("small_fwd",), dict(pre_rho=1, f=_mlp(C=2), rho=_rho(C=2)), b"rho.C=2"),
    (("nam_bwd",), dict(F=128, x_stride=128), b"F=128"),
    (BATCH, dict(cnt=0x300000, cnt_stride=12, f=_mlp(C=2), rho=_rho(C=2)), b"rho.C=2"),
    (("batch_fwd",), dict(cnt=0x300000, cnt_stride=65, D=65), b"D=65"),
    (BATCH, dict(n=0), b"max_nodes=0"),
]
BAD_ARGUMENTS = [
    (SMALL + NAM, dict(n=0), b"n=0"), (BATCH, dict(F=0), b"bad sizes"), (BATCH, dict(total_nodes=-1), b"bad sizes"),
    (SMALL + NAM + BATCH, dict(x=None), b"null"), (SMALL + NAM + BATCH, dict(code=None), b"null"),
    (SMALL + NAM + BATCH, dict(lut=None), b"null"), (SMALL + BATCH, dict(S=None), b"null"),
    (FWD_256, dict(Ysum=None), b"null"), (("small_bwd", "batch_bwd"), dict(dYsum=None), b"null"),
    (NAM, dict(fx=None), b"null"), (NAM, dict(hidden=None), b"null"), (("nam_fwd",), dict(out=None), b"null"),
    (("nam_bwd",), dict(d_out=None), b"null"), (BATCH, dict(node_off=None), b"null"), (BATCH, dict(code_off=None), b"null"),
    (SMALL + NAM + BATCH, dict(x_stride=14), b"stride"), (SMALL + NAM, dict(cnt_stride=11), b"stride"),
    (BATCH, dict(cnt=0x300000, cnt_stride=11), b"stride"), (BATCH, dict(n_graphs=65536), b"65535"),
    (("small_bwd",), dict(pre_rho=1, cnt=None, cnt_stride=0), b"pre-rho"),
]


def _spread(table):
    return [pytest.param(e, kw, named, id=f"{e}-{'-'.join(kw)}-{i}") for i, (entries, kw, named) in enumerate(table) for e in entries]


@pytest.mark.parametrize("entry,kw,named", _spread(OUTSIDE_THE_COVER))
def test_shapes_outside_the_cover_are_refused_by_name(entry, kw, named):
    rc, said = _refused(entry, kw)
    assert rc == UNSUPPORTED, (entry, kw, said)
    assert named in said, (entry, kw, said)


@pytest.mark.parametrize("entry,kw,named", _spread(BAD_ARGUMENTS))
def test_bad_arguments_are_refused_before_any_hip_call(entry, kw, named):
    rc, said = _refused(entry, kw)
    assert rc == BAD_ARG, (entry, kw, said)
    assert named in said, (entry, kw, said)


@pytest.mark.parametrize("entry", BWD)
def test_a_bias_gradient_exactly_where_there_is_a_bias(entry):
    missing = _grads(_mlp())
    missing.b_first = None
    surplus = _grads(_rho(), 0xA000)
    surplus.b_last = 0xA500
    for kw in (dict(df=missing), dict(drho=surplus)):
        rc, said = _refused(entry, kw)
        assert rc == BAD_ARG and b"bias" in said, (entry, kw, said)
    if entry == "nam_bwd":
        linear = _linear_nam()
        no_bias = _linear_grads(linear)
        no_bias.b_last = None
        rc, said = _refused(entry, dict(nam=linear, dnam=no_bias))
        assert rc == BAD_ARG and b"read-out" in said, said


@pytest.mark.parametrize("entry", ("small_fwd", "nam_fwd", "nam_bwd", "batch_fwd", "batch_bwd"))
def test_a_workspace_one_byte_short(entry):
    """... is the LAST refusal: everything else about these arguments was accepted (gnan_small_graph_bwd only borrows a workspace)."""
    full = ENTRIES[entry][1]().workspace_bytes
    assert full > 16
    for kw in (dict(short=1),) + ((dict(short=1, nam=_linear_nam()),) if entry in NAM else ()):
        rc, said = _refused(entry, kw)
        assert rc == WORKSPACE, (entry, said)
        assert str(full).encode() in said and str(full - 1).encode() in said, (entry, said)
    assert _refused(entry, dict(workspace=None))[0] == WORKSPACE


# written last: the ONE answer the shared validator changed.  A null weight pointer was UNSUPPORTED at the six entry points above
# (their shape test looked at the pointers too) and BAD_ARG at the two of csrc/mid_graph.hip; it is a bad argument everywhere.
@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_a_null_weight_is_a_bad_argument_at_every_entry_point(entry):
    for which in ("f", "rho"):
        for field in ("w_first", "w_mid", "w_last"):
            m = _mlp() if which == "f" else _rho()
            setattr(m, field, None)
            rc, said = _refused(entry, {which: m})
            assert rc == BAD_ARG and b"null weights" in said, (entry, which, field, said)
    if entry in NAM:
        linear = _linear_nam()
        linear.w_last = None
        rc, said = _refused(entry, dict(nam=linear))
        assert rc == BAD_ARG and b"null weights" in said, said


# ---------------------------------------------------------------------------------------------------------------------------------
# the four predicates
# ---------------------------------------------------------------------------------------------------------------------------------
F = 5


def _stack(L=3, H=8, C=1, n_features=F, dtype=torch.float32, odd=None):
    """What a predicate reads of a StackedMLP; ``odd``: the index of ONE parameter held in float64."""
    t = [torch.zeros(1, dtype=dtype) for _ in range(6)]
    if odd is not None:
        t[odd] = t[odd].double()
    return StackedMLP(*t, L, H, C, n_features)


def _dense(n, n_codes=2, cnt=True):
    return types.SimpleNamespace(is_dense=True, n_rows=n, n_cols=n, n_codes=n_codes,
                                 cnt=torch.ones(1, dtype=torch.int32) if cnt else None)


def _small(n=100, x=None, g=None, f=None, rho=None, **kw):
    return sg.small_graph_applies(_FakeCuda(n, F) if x is None else x, g or _dense(n), f or _stack(), rho or _stack(n_features=1), **kw)


def _mid(n=200, x=None, g=None, f=None, rho=None, **kw):
    return sg.mid_graph_applies(_FakeCuda(n, F) if x is None else x, g or _dense(n), f or _stack(), rho or _stack(n_features=1), **kw)


def _nam_applies(n=100, x=None, g=None, f=None, rho=None, nam=None):
    return sg.small_graph_nam_applies(_FakeCuda(n, F) if x is None else x, g or _dense(n), f or _stack(), rho or _stack(n_features=1),
                                      nam or _stack(C=2))


def _slot(f=None, rho=None, n_features=F):
    return sg.slot_graph_applies(types.SimpleNamespace(F=n_features), f or _stack(), rho or _stack(n_features=1))


PREDICATES = [
    # node counts
    (_small, dict(n=0), False), (_small, dict(n=1), True), (_small, dict(n=128), True), (_small, dict(n=129), False),
    (_mid, dict(n=128), False), (_mid, dict(n=129), True), (_mid, dict(n=448), True), (_mid, dict(n=449), False),
    (_nam_applies, dict(n=0), False), (_nam_applies, dict(n=1), True), (_nam_applies, dict(n=128), True),
    (_nam_applies, dict(n=129), False),
    (_small, dict(g=_dense(99)), False), (_mid, dict(g=_dense(199)), False), (_nam_applies, dict(g=_dense(99)), False),
    # hop codes
    (_small, dict(g=_dense(100, 64)), True), (_small, dict(g=_dense(100, 65)), True), (_small, dict(g=_dense(100, 256)), True),
    (_small, dict(g=_dense(100, 257)), False),
    (_small, dict(g=_dense(100, 64), pre_rho=True), True), (_small, dict(g=_dense(100, 65), pre_rho=True), False),
    (_mid, dict(g=_dense(200, 64)), True), (_mid, dict(g=_dense(200, 65)), False),
    (_nam_applies, dict(g=_dense(100, 64)), True), (_nam_applies, dict(g=_dense(100, 65)), False),
    # hidden width
    (_small, dict(f=_stack(H=64)), True), (_small, dict(f=_stack(H=65)), False), (_small, dict(f=_stack(H=0)), False),
    (_small, dict(rho=_stack(H=64, n_features=1)), True), (_small, dict(rho=_stack(H=65, n_features=1)), False),
    (_mid, dict(f=_stack(H=64)), True), (_mid, dict(f=_stack(H=65)), False), (_mid, dict(rho=_stack(H=65, n_features=1)), False),
    (_nam_applies, dict(f=_stack(H=64)), True), (_nam_applies, dict(f=_stack(H=65)), False),
    (_nam_applies, dict(nam=_stack(H=64, C=2)), True), (_nam_applies, dict(nam=_stack(H=65, C=2)), False),
    (_nam_applies, dict(nam=_stack(L=1, H=0, C=2)), True), (_nam_applies, dict(nam=_stack(L=2, H=0, C=2)), False),
    (_slot, dict(f=_stack(H=64)), True), (_slot, dict(f=_stack(H=65)), False), (_slot, dict(rho=_stack(H=65, n_features=1)), False),
    # output channels, rho's channels
    (_small, dict(f=_stack(C=8)), True), (_small, dict(f=_stack(C=9)), False),
    (_small, dict(f=_stack(C=8), rho=_stack(C=8, n_features=1)), True), (_small, dict(f=_stack(C=8), rho=_stack(C=2, n_features=1)), False),
    (_small, dict(f=_stack(C=2), rho=_stack(C=2, n_features=1), pre_rho=True), False),
    (_mid, dict(f=_stack(C=8)), True), (_mid, dict(f=_stack(C=9)), False), (_mid, dict(f=_stack(C=0)), False),
    (_mid, dict(f=_stack(C=8), rho=_stack(C=8, n_features=1)), False), (_mid, dict(f=_stack(C=8), rho=_stack(C=2, n_features=1)), False),
    (_nam_applies, dict(f=_stack(C=2)), False), (_nam_applies, dict(rho=_stack(C=2, n_features=1)), False),
    (_nam_applies, dict(nam=_stack(C=8)), True), (_nam_applies, dict(nam=_stack(C=9)), False), (_nam_applies, dict(nam=_stack(C=0)), False),
    (_slot, dict(f=_stack(C=8)), True), (_slot, dict(f=_stack(C=9)), False),
    (_slot, dict(f=_stack(C=8), rho=_stack(C=8, n_features=1)), False), (_slot, dict(f=_stack(C=8), rho=_stack(C=2, n_features=1)), False),
    # feature counts
    (_small, dict(f=_stack(n_features=F + 1)), False), (_small, dict(rho=_stack(n_features=2)), False),
    (_mid, dict(f=_stack(n_features=F + 1)), False), (_mid, dict(rho=_stack(n_features=2)), False),
    (_nam_applies, dict(nam=_stack(C=2, n_features=F + 1)), False), (_nam_applies, dict(rho=_stack(n_features=2)), False),
    (_nam_applies, dict(x=_FakeCuda(100, 127), f=_stack(n_features=127), nam=_stack(C=2, n_features=127)), True),
    (_nam_applies, dict(x=_FakeCuda(100, 128), f=_stack(n_features=128), nam=_stack(C=2, n_features=128)), False),
    (_slot, dict(n_features=F + 1), False), (_slot, dict(rho=_stack(n_features=2)), False),
    # the input: on the host, another dtype, wanting a gradient, a graph in CSR form
    (_small, dict(x=torch.zeros(100, F)), False), (_mid, dict(x=torch.zeros(200, F)), False),
    (_nam_applies, dict(x=torch.zeros(100, F)), False),
    (_small, dict(x=_FakeCuda(100, F, requires_grad=True)), False), (_mid, dict(x=_FakeCuda(200, F, requires_grad=True)), False),
    (_nam_applies, dict(x=_FakeCuda(100, F, requires_grad=True)), False),
    (_small, dict(g=types.SimpleNamespace(**{**vars(_dense(100)), "is_dense": False})), False),
    (_mid, dict(g=types.SimpleNamespace(**{**vars(_dense(200)), "is_dense": False})), False),
    (_nam_applies, dict(g=types.SimpleNamespace(**{**vars(_dense(100)), "is_dense": False})), False),
    # shell sizes
    (_small, dict(g=_dense(100, cnt=False)), True), (_small, dict(g=_dense(100, cnt=False), pre_rho=True), False),
    (_small, dict(pre_rho=True), True),
    (_mid, dict(use_cnt=True), True), (_mid, dict(use_cnt=False), True), (_mid, dict(use_cnt="pre"), False),
    (_mid, dict(g=_dense(200, cnt=False), use_cnt=True), False), (_mid, dict(g=_dense(200, cnt=False), use_cnt=False), True),
]
# depths 1 to 4 of every stack, and each parameter in turn in another dtype
for _L in (1, 2, 3, 4):
    _ok = _L in (2, 3)
    PREDICATES += [(_small, dict(f=_stack(L=_L)), _ok), (_small, dict(rho=_stack(L=_L, n_features=1)), _ok),
                   (_mid, dict(f=_stack(L=_L)), _ok), (_mid, dict(rho=_stack(L=_L, n_features=1)), _ok),
                   (_nam_applies, dict(f=_stack(L=_L)), _ok), (_nam_applies, dict(rho=_stack(L=_L, n_features=1)), _ok),
                   (_nam_applies, dict(nam=_stack(L=_L, C=2)), _L in (1, 2, 3)),
                   (_slot, dict(f=_stack(L=_L)), _ok), (_slot, dict(rho=_stack(L=_L, n_features=1)), _ok)]
for _i in range(6):
    PREDICATES += [(_small, dict(f=_stack(odd=_i)), False), (_small, dict(rho=_stack(odd=_i, n_features=1)), False),
                   (_mid, dict(f=_stack(odd=_i)), False), (_mid, dict(rho=_stack(odd=_i, n_features=1)), False),
                   (_nam_applies, dict(f=_stack(odd=_i)), False), (_nam_applies, dict(nam=_stack(odd=_i, C=2)), False),
                   (_slot, dict(f=_stack(odd=_i)), False), (_slot, dict(rho=_stack(odd=_i, n_features=1)), False)]


def test_the_predicates_at_every_limit():
    for i, (predicate, kw, expected) in enumerate(PREDICATES):
        got = predicate(**kw)
        assert got is expected, (i, predicate.__name__, kw, got)
    # a stack whose absent parameters are None (no bias, two layers) is float32 throughout
    bare = StackedMLP(torch.zeros(1), None, None, None, torch.zeros(1), None, 2, 8, 1, F)
    assert _small(f=bare) and _mid(f=bare) and _nam_applies(f=bare) and _slot(f=bare)


# each switch, and what it turns off: (switch, (predicate, arguments) it governs, (predicate, arguments) it leaves alone)
SWITCHES = [
    ("SMALL_GRAPH_FORWARD", [(_small, {}), (_mid, {})], [(_nam_applies, {}), (_slot, {})]),
    ("MID_GRAPH", [(_mid, {})], [(_small, {}), (_nam_applies, {}), (_slot, {})]),
    ("SMALL_GRAPH_BACKWARD", [(_small, dict(pre_rho=True))], [(_small, {}), (_mid, {}), (_nam_applies, {}), (_slot, {})]),
]


@pytest.mark.parametrize("switch,governed,others", SWITCHES)
def test_each_switch_off(switch, governed, others):
    assert all(p(**kw) is True for p, kw in governed + others)
    old = getattr(sg, switch)
    setattr(sg, switch, False)
    try:
        assert all(p(**kw) is False for p, kw in governed), switch
        assert all(p(**kw) is True for p, kw in others), switch
    finally:
        setattr(sg, switch, old)
    assert (sg.SMALL_GRAPH_MAX_NODES, sg.MID_GRAPH_MIN_NODES, sg.MID_GRAPH_MAX_NODES) == (128, 129, 448)
    assert (sg.SMALL_GRAPH_NAM_MAX_FEATURES, sg.SLOT_MAX_NODES, sg.SLOT_CODES) == (127, 128, 64)
