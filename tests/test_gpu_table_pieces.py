"""The tables of gnan_pwl_build (pwl_build_kernel<false> for L = 2 and 3, pwl_build_kernel<true> for L = 4) piece by piece, and
the look-up kernels on them, against the exact reference of tests/tables_ref.py — the same anchor, point-piece, no-kink and
per-element value assertions tests/test_tables_bound.py holds the torch builder to, on the kernel's OWN tables (not only against
the torch builder's; the piece counts of the two builders stay equal, which pins the duplicates of coinciding kinks).

Every (probe, feature, channel) of ``functional._fpwl_launch`` is held to its bound with k = 3 float32 roundings on the longer
path (the slope as stored, ``x - a``, the look-up's fma); summed over the features, the per-feature bounds add up and F float32
additions are counted on top.  Each look-up runs twice for the same bits.  Shapes: the smallest that reach every instance and
route of the build kernel (L = 2 / 3 by dot products, the affine route, the deep instance; 64- and 32-node passes with roots
around the pass boundary; odd H; narrow, LDS-staged and global last layers) and of the look-up (ragged feature groups, the
two-phase kernels at C = 130)."""
import pytest
import torch

import tables_ref as R
from test_tables_bound import CASES as CPU_CASES

pytestmark = pytest.mark.gpu
DEV = "cuda"
K32 = 3


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")


# name -> (stack, route of the build kernel it must take)
GPU_CASES = {
    # L = 2: dot products
    "random-L2-H8": "dot", "random-L2-H128-C40": "dot", "dead-L2": "dot", "no-bias-L2": "dot",
    # L = 3, H <= 64: the interval forms
    "ladder-L3-H2-issue": "affine", "ladder-L3-edges": "affine", "thirds-L3": "affine", "random-L3-H8": "affine",
    "random-L3-H16-C5": "affine", "random-L3-H33": "affine", "random-L3-H64": "affine", "no-bias-L3": "affine",
    "zero-biases-L3": "affine", "range-L3": "affine", "wide-L3": "affine", "dead-L3": "affine",
    # L = 3, H = 128: dot products in 32-node passes
    "random-L3-H128": "dot", "pass-32-L3-P28": "dot", "pass-32-L3-P29": "dot", "pass-32-L3-P30": "dot",
    # L = 4: the deep instance, 64-node passes
    "ladder-L4-edges": "deep", "thirds-L4": "deep", "random-L4-H8": "deep", "random-L4-H16": "deep", "random-L4-H33": "deep",
    "no-bias-L4": "deep", "zero-biases-L4": "deep", "range-L4": "deep", "wide-L4": "deep", "dead-L4": "deep",
    "pass-64-L4-P60": "deep", "pass-64-L4-P61": "deep", "pass-64-L4-P62": "deep",
}
EXTRA = {
    "random-L3-H8-C1": (lambda: R.random_state(3, 3, 8, 1, True, 21), "affine"),
    "random-L3-H8-C4-F20": (lambda: R.random_state(20, 3, 8, 4, True, 22), "affine"),              # ragged feature groups
    "random-L3-H64-C40": (lambda: R.random_state(1, 3, 64, 40, True, 23), "affine"),               # last layer staged in LDS
    "random-L4-H64-C1": (lambda: R.random_state(1, 4, 64, 1, True, 24), "deep"),
    "random-L4-H8-C65": (lambda: R.random_state(2, 4, 8, 65, True, 25), "deep"),                   # above 64: from global memory
    "random-L3-H8-C130": (lambda: R.random_state(3, 3, 8, 130, True, 26), "affine"),
    "random-L4-H64-C130-rows": (lambda: R.random_state(1, 4, 64, 130, True, 26), "deep"),          # no LDS image: gnan_fpwl_rows_fwd
    "ladder-L4-H8-edges": (lambda: R.stack_of(R.ladder_edges(4, 8, 2)[1], 4, 8, 2), "deep"),
    "pass-64-L4-H33-P29": (lambda: R.stack_of([R.ladder_pass_boundary(4, 33, 1, 29)], 4, 33, 1), "deep"),   # odd H: scalar dense_layer
}
ALL = list(GPU_CASES) + list(EXTRA)
_SHARED = {}


def _case(name):
    if name not in _SHARED:
        p = (CPU_CASES[name] if name in CPU_CASES else EXTRA[name][0])()
        route = GPU_CASES.get(name) or (EXTRA[name][1] if name in EXTRA else "deep" if p.L == 4 else None)
        _SHARED[name] = (p, R.features_of(p), route)
    return _SHARED[name]


def _to(p, dev):
    return type(p)(*[None if q is None else q.to(dev) for q in p[:6]], *p[6:])


def _piece_by_piece(name, equal_counts=True):
    from gnan_amd import functional, pwl
    p, exs, route = _case(name)
    assert pwl.BUILD_BACKEND == "auto"
    pd = _to(p, DEV)
    assert pwl.hip_build_applies(pd)
    assert route == ("deep" if p.L == 4 else "affine" if (p.L == 3 and p.H <= 64) else "dot")
    t = pwl.build_tables(pd)
    t_ref = pwl.build_tables(p)                                        # CPU tensors: the torch builder
    assert t is not None and t_ref is not None
    tc = R.cpu_tables(t)
    if equal_counts:
        assert torch.equal(tc.off, t_ref.off), "the two builders count the same pieces per feature"
    else:
        for k in range(p.F):
            a, b = R.feature_table(tc, k)[0], R.feature_table(t_ref, k)[0]
            assert bool((R.distinct_breakpoints(a) == R.distinct_breakpoints(b)).all()), "the two builders' distinct anchors"
    assert bool(torch.isfinite(tc.anchor).all() and torch.isfinite(tc.val).all() and torch.isfinite(tc.slope).all())
    runs = []

    def look_up(x, sum_features=False):
        xd = x.to(DEV)
        a = functional._fpwl_launch(xd, t, sum_features).cpu()
        b = functional._fpwl_launch(xd, t, sum_features).cpu()
        runs.append(bool((a.view(torch.int32) == b.view(torch.int32)).all()))
        return a

    rep, x, _ = R.check_tables(p, tc, look_up, K32, exs)
    if name.endswith("rows"):
        assert pwl.oversize(t) and functional._fpwl_rows_applies(x.shape[0], p.C, t, bins=False)
    summed = R.check_sum(rep, look_up(torch.from_numpy(x), True).numpy())
    print(f"{name}: route {route}, {tc.anchor.numel()} pieces, {x.shape[0]} probes per feature, {rep['point_pieces']} point pieces, "
          f"worst |err| / bound = {rep['worst']:.3f} per feature, {summed:.3f} summed")
    assert rep["anchors"] == [], rep["anchors"][:4]
    assert rep["kinks"] == [], rep["kinks"][:4]
    assert rep["worst"] <= 1.0, f"|err| / bound = {rep['worst']:.3g} at {rep['where']}"
    assert summed <= 1.0
    assert all(runs), "the look-up gave other bits the second time"


@pytest.mark.parametrize("name", ALL)
def test_kernel_tables_piece_by_piece(name):
    _piece_by_piece(name)


def test_roots_on_inexact_breakpoints_differ_in_duplicates_at_most():
    """A third-layer root that is, in exact arithmetic, ON a second-layer root which no float64 holds: beside such a breakpoint
    the pre-activation is a rounding residue, and whether a builder sees a sign change there — and lists the kink a second time
    — is decided by its order of operations.  The kernel and the torch builder may then differ in the number of COINCIDING
    anchors (zero-width pieces no value falls in); the distinct anchors, the point pieces and every value are held as ever."""
    _piece_by_piece("thirds-L4-coincident", equal_counts=False)


def test_kernel_and_torch_builder_anchor_for_anchor():
    """Beyond the piece counts: on the ladder cases (every kink a small dyadic, both builders exact) the two builders' anchors
    are the same float32 values, piece for piece."""
    from gnan_amd import pwl
    for name in ("ladder-L3-edges", "ladder-L4-edges", "pass-64-L4-P61", "pass-32-L3-P29"):
        p, _, _ = _case(name)
        t, t_ref = pwl.build_tables(_to(p, DEV)), pwl.build_tables(p)
        assert torch.equal(t.off.cpu(), t_ref.off) and bool((t.anchor.cpu() == t_ref.anchor).all()), name
