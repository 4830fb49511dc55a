"""The per-piece moments of the table path on the MI355X, piece by piece: every moment kernel against the exact integer restatement
and the float64 truth of tests/moments_ref.py (bounds and their counted constants: that file's header).

Every case asserts  (1) its ROUTE through ``gnan_fpwl_moments_describe`` / ``gnan_fpwl_rows_moments_describe`` — the launcher's own
routing functions, stopped short of the launch —, the tree depth and the node blocks where the case is about them;  (2) the two
scales against their restatement from the arrays as passed;  (3) the same bits from a second run;  (4) the raw int64 bins against
the restatement BIT FOR BIT — on the kept route M0 bit for bit and M1 inside K_t quanta of the exactly formed rational
M1x - a M0 2^(e1 - e0);  (5) every element against the float64 truth within its own piece's bound, empty pieces exact zeros.
The float-bin route has no bit-exact claim: gamma_k with k counted from the kernel.  Kept pieces come from a real forward
(``_fpwl_launch(..., located=[])``) and are themselves compared with the ownership rule #{anchors[1:] <= x}.

The cases (tests/moments_ref.py ``CASES``; the reference alone passes each in tests/test_moments_bound.py):
  fam-*        every gradient family x {uniform, levels, offset} on the c1 search and c1 kept routes
  tail-*       last node blocks of 1, NODES - 1, NODES, NODES + 1, 2 NODES nodes with 256-node blocks, a single node, rays; blocks of
               three rounds (from 16 384 nodes) with last blocks of 2 NODES + 1 and 3 NODES - 1 nodes: the kept loop's third round
  headroom-*   all nodes in one piece per feature, every gradient the float below 2 (and negated), n = 4096 and 4097
  edge-*       64 | 65, 128 | 129, 256 pieces (tree depth), 257 (the kept byte is abandoned although a piece buffer is attached),
               1023 | 1024 (deepest tree), 1025 (general kernel)
  perfeature-* per-feature gradient: kept piece-major (16-byte readable rows), kept with staged anchors (column-offset view), searched
  ragged-*     F = 20, 33 with column-offset x, F = 3;  narrow-groups-3: two features per group (general kernel)
  general-flag MOMENTS_GENERAL (fast kernel; ragged: general kernel);  fast-C{2,3,8,9};  rows-C{12,40,64,65,130} x {sum, per}
               with (piece, dx) kept by the forward (sum) or located again (per);  float-*: MOMENTS_FIXED_POINT = False
"""
import numpy as np
import pytest
import torch

import moments_ref as R
from gpu_util import DEV

pytestmark = pytest.mark.gpu

BY_NAME = {c.name: c for c in R.CASES}
RESULTS = {}          # case name -> (raw bins, scales, route): a case is launched once, the scaled families read their sibling's
WORST = {}            # (route, gradient family) -> worst |err| / bound of (M0, M1, kept flush)


def _check_kept_pieces(case, located):
    """The forward's kept pieces against the ownership rule (they were found by other searches than the moments' own)."""
    b = R.build_case(case)
    ht, own = b["ht"], R.owners(b["x"], b["ht"])
    if case.route.startswith("rows"):
        piece, dx = (v.cpu().numpy() for v in located)
        assert np.array_equal(piece, own)
        assert np.array_equal(dx, (b["x"] - ht.anchor[own]).astype(np.float32))
    else:
        fg = located[0].shape[2]
        got = located[0].cpu().numpy()
        for k in range(ht.F):
            assert np.array_equal(got[k // fg, :, k % fg], own[:, k] - ht.off[k]), k


def launch(case, monkeypatch):
    from gnan_amd import functional
    if case.name in RESULTS:
        return RESULTS[case.name]
    monkeypatch.setattr(functional, "MOMENTS_GENERAL", case.general)
    monkeypatch.setattr(functional, "MOMENTS_FIXED_POINT", case.fixed)
    if case.rows_min:
        monkeypatch.setattr(functional, "FPWL_ROWS_MIN_NODES", case.rows_min)
    t, xd, gd = R.launch_inputs(case, DEV)
    rows = case.route.startswith("rows")
    assert functional._fpwl_rows_applies(case.n, case.C, t) == rows
    located = None
    if case.kept:
        located = []
        functional._fpwl_launch(xd, t, case.sum_features if rows else True, located=located)
        assert len(located) == (2 if rows else 1), "the forward kept no pieces"
        _check_kept_pieces(case, located)
    elif case.stale_pieces:
        fg = t.features_per_group
        located = [torch.zeros(((xd.shape[1] + fg - 1) // fg, case.n, fg), dtype=torch.uint8, device=DEV)]
    d = []
    if case.fixed:
        M, scales = functional._fpwl_moments(xd, t, gd, case.sum_features, raw=True, located=located, describe=d)
        M2, scales2 = functional._fpwl_moments(xd, t, gd, case.sum_features, raw=True, located=located)
        assert torch.equal(M, M2) and torch.equal(scales, scales2), "two runs, two results"
        out = (M.cpu().numpy(), scales.cpu().numpy(), d[0])
    else:
        M = functional._fpwl_moments(xd, t, gd, case.sum_features, located=located, describe=d)
        out = (M.cpu().numpy(), None, d[0])
    R.assert_route(case, d[0])
    RESULTS[case.name] = out
    return out


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for (route, gfam), r in sorted(WORST.items()):
        print(f"worst |err|/bound  {route:14s} {gfam:14s} M0 {r[0]:.3g}  M1 {r[1]:.3g}  flush {r[2]:.3g}")


@pytest.mark.parametrize("name", [c.name for c in R.CASES if c.fixed])
def test_fixed_point_moments(name, monkeypatch):
    case = BY_NAME[name]
    M, scales, info = launch(case, monkeypatch)
    r = R.check_fixed(case, M, scales, info["nodes_per_block"], name)
    key = (case.route, case.gfam)
    WORST[key] = tuple(max(p, q) for p, q in zip(WORST.get(key, (0.0, 0.0, 0.0)), r))
    sib, shift = R.sibling(case)
    if sib is not None:
        # unit 2^+-100: the same bins bit for bit, the scales' exponents shifted — wherever no float32 product left the normal range
        b, bs = R.build_case(case), R.build_case(sib)
        Ms, ss, _ = launch(sib, monkeypatch)
        assert (b["e0"], b["e1"]) == (bs["e0"] + shift, bs["e1"] + shift)
        assert np.array_equal(M[:, 0, :], Ms[:, 0, :])
        if b["ref"]["normal"] and bs["ref"]["normal"]:
            assert np.array_equal(M, Ms), "scaled gradient, other bins"


@pytest.mark.parametrize("name", [c.name for c in R.CASES if not c.fixed])
def test_float_bin_moments(name, monkeypatch):
    case = BY_NAME[name]
    M, _, info = launch(case, monkeypatch)
    tr = R.build_case(case)["truth"]
    b0, b1 = R.float_bounds(tr)
    r = (R.assert_within(M[:, 0, :], tr["T0"], b0, name + " M0"), R.assert_within(M[:, 1, :], tr["T1"], b1, name + " M1"), 0.0)
    if case.gfam == "integers":
        assert np.array_equal(M[:, 0, :], tr["T0"]) and np.array_equal(M[:, 1, :], tr["T1"])
    key = (case.route, case.gfam)
    WORST[key] = tuple(max(p, q) for p, q in zip(WORST.get(key, (0.0, 0.0, 0.0)), r))
