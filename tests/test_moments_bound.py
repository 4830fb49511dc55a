"""The per-piece moments of the table path, CPU side: the reference of tests/moments_ref.py against an emulation of the kernels'
own arithmetic, over EVERY case of tests/test_gpu_moment_pieces.py, before a GPU is involved — and planted errors that each
must fail a named case.  The route of every case is asked of the library's host-only query (``gnan_fpwl_moments_describe`` /
``gnan_fpwl_rows_moments_describe``: no device memory is read), so the case table cannot drift from the launcher.

Worst |err| / bound per gradient family: on the fixed-point routes the emulation's bins ARE the restatement's, which are the
kernels' (asserted bit for bit on both sides), so its figures are by construction the ones measured on the MI355X and recorded in
DESIGN section 8 ("The table path's moments, piece by piece"); on the kept route the emulation rounds at the same places as the
kernel and gave the same flush figures.  ``test_reference_passes_every_case`` prints them with ``-s``.
"""
import numpy as np
import pytest
import torch

import moments_ref as R

BY_NAME = {c.name: c for c in R.CASES}
FIXED = [c for c in R.CASES if c.fixed]


def host_route(case):
    """The route query for a case, on host memory, with the arguments ``functional._fpwl_moments`` would pass."""
    from gnan_amd import _lib, functional
    t, x, g = R.launch_inputs(case, "cpu")
    n, F = x.shape
    a = _lib.FpwlArgs(x=_lib.ptr(x), n=n, x_stride=x.stride(0), F=F, C=case.C, off=_lib.ptr(t.off), anchor=_lib.ptr(t.anchor),
                      val=_lib.ptr(t.val), slope=_lib.ptr(t.slope), max_pieces=t.max_pieces, features_per_group=t.features_per_group,
                      max_group_pieces=t.max_group_pieces, sum_features=int(case.sum_features), out=None, out_stride=0,
                      flags=_lib.FPWL_MOMENTS_GENERAL if case.general else 0)
    pieces = torch.zeros(4 * n * (F + 16), dtype=torch.uint8)
    if (case.kept or case.stale_pieces) and not case.route.startswith("rows"):
        a.piece_in = _lib.ptr(pieces)
    info = _lib.FpwlMomentsInfo()
    if case.route.startswith("rows"):
        assert functional.FPWL_ROWS and case.C >= functional.FPWL_ROWS_MIN_CHANNELS and n >= case.rows_min > 0
        _lib.check(_lib.lib().gnan_fpwl_rows_moments_describe(a, g.stride(0), info), "describe")
    else:
        assert not functional._fpwl_rows_applies(n, case.C, t)
        _lib.check(_lib.lib().gnan_fpwl_moments_describe(a, _lib.ptr(g), g.stride(0), int(case.fixed), info), "describe")
    return info.as_dict()


def emulate_float(case):
    """Float bins: float32 additions in node order (ONE of the orders the atomics may take; the bound covers all of them)."""
    b = R.build_case(case)
    ht, x, g = b["ht"], b["x"], b["g"]
    T, C = int(ht.off[-1]), case.C
    M = np.zeros((T, 2, C), dtype=np.float32)
    t = R.owners(x, ht)
    cols = np.arange(C)[None, :]
    for k in range(ht.F):
        gk = np.ascontiguousarray(R._g_of(g, k, C, case.sum_features))
        d = (x[:, k] - ht.anchor[t[:, k]]).astype(np.float32)
        idx = (np.broadcast_to(t[:, k][:, None], gk.shape), np.broadcast_to(cols, gk.shape))
        np.add.at(M[:, 0, :], idx, gk)
        np.add.at(M[:, 1, :], idx, (gk * d[:, None]).astype(np.float32))
    return M


WORST = {}


@pytest.mark.parametrize("name", [c.name for c in R.CASES])
def test_reference_passes_every_case(name):
    """The emulation in the kernels' arithmetic (magic-number conversion, the power-of-two search, the kept route block by block
    with the query's nodes_per_block) equals the exact restatement and stays inside the truth bound, element by element."""
    case = BY_NAME[name]
    info = host_route(case)
    R.assert_route(case, info)
    b = R.build_case(case)
    if not case.fixed:
        M = emulate_float(case)
        b0, b1 = R.float_bounds(b["truth"])
        r = (R.assert_within(M[:, 0, :], b["truth"]["T0"], b0, name + " M0"), R.assert_within(M[:, 1, :], b["truth"]["T1"], b1, name + " M1"))
    else:
        kept = case.route == "c1_kept"
        M, (e0, e1) = R.emulate(b["x"], b["g"], b["ht"], case.C, case.sum_features, "kept" if kept else "search", info["nodes_per_block"])
        r = R.check_fixed(case, M, (2.0 ** e0, 2.0 ** e1), info["nodes_per_block"], name)
    key = (case.route, case.gfam)
    WORST[key] = tuple(max(p, q) for p, q in zip(WORST.get(key, (0.0,) * len(r)), r))
    print(name, " ".join(f"{v:.3g}" for v in r))


def test_case_table_reaches_what_it_claims():
    """Properties of the inputs the cases rely on, from the reference alone."""
    b = R.build_case(BY_NAME["tail-c1_search-1"])
    cnt = b["truth"]["cnt"]
    off = b["ht"].off
    for k, P in enumerate(R.MIX32):
        if P >= 4:
            assert cnt[off[k] + 2] == 0 and cnt[off[k] + 3] == 1          # an empty piece and a piece with a single node
    assert np.all(b["truth"]["T0"][cnt == 0] == 0)
    full = R.build_case(BY_NAME["tail-c1_search-256"])["truth"]["cnt"]
    assert np.all(np.delete(full, [o + i for o, P in zip(off[:-1], R.MIX32) if P >= 4 for i in (2, 3)]) > 0)   # every other piece and both rays
    lev = R.build_case(BY_NAME["fam-c1_search-unit-levels"])
    d = lev["x"] - lev["ht"].anchor[R.owners(lev["x"], lev["ht"])]
    assert not d.any()                                              # ON the anchors: every d is zero, ownership by <=
    rays = R.build_case(BY_NAME["tail-c1_search-rays"])
    assert np.abs(rays["x"] - rays["ht"].anchor[R.owners(rays["x"], rays["ht"])]).max() >= 1.0e4
    one = R.build_case(BY_NAME["headroom-c1_search-4097-same-sign"])
    assert np.count_nonzero(one["truth"]["cnt"]) == 16 and R.restate_bits(4097) == 48 and R.restate_bits(4096) == 49
    assert int(np.abs(one["ref"]["M0"]).max()) > 2 ** 59           # the largest sum the headroom must hold (below 2^62)
    down = R.build_case(BY_NAME["fam-c1_search-unit-down-levels"])
    assert down["ref"]["normal"] and (down["e0"], down["e1"]) == tuple(v + 100 for v in (lev["e0"], lev["e1"]))
    assert np.array_equal(down["ref"]["M0"], lev["ref"]["M0"]) and np.array_equal(down["ref"]["M1"], lev["ref"]["M1"])


# ---- planted errors: each must fail the case it names ---------------------------------------------------------------------------
def _planted(name, plant, route="search", npb=R.BLOCK_SMALL):
    case = BY_NAME[name]
    b = R.build_case(case)
    M, (e0, e1) = R.emulate(b["x"], b["g"], b["ht"], case.C, case.sum_features, route, npb, plant=plant)
    return case, b, M, e0, e1


def test_planted_coarser_fixed_point_fails_the_m0_bound_of_the_range_family():
    case, b, M, e0, e1 = _planted("fam-c1_search-range-uniform", "coarse")
    b0, _ = R.fixed_bounds(b["truth"], b["e0"], b["e1"])
    assert R.worst_ratio(np.ldexp(M[:, 0, :].astype(np.float64), -e0), b["truth"]["T0"], b0) > 1.0
    with pytest.raises(AssertionError, match="scales"):
        R.check_fixed(case, M, (2.0 ** e0, 2.0 ** e1), R.BLOCK_SMALL)
    # the unit family cannot see it in M0 (g 2^e0 stays an integer 2^8 coarser): what the range family is for
    _, bu, Mu, u0, _ = _planted("fam-c1_search-unit-uniform", "coarse")
    assert np.array_equal(np.ldexp(Mu[:, 0, :].astype(np.float64), -u0), np.ldexp(bu["ref"]["M0"].astype(np.float64), -bu["e0"]))


def test_planted_truncation_fails_the_exact_restatement():
    case, b, M, e0, e1 = _planted("fam-c1_search-range-uniform", "trunc")
    assert (e0, e1) == (b["e0"], b["e1"])
    with pytest.raises(AssertionError, match="M0 differs"):
        R.check_fixed(case, M, (2.0 ** e0, 2.0 ** e1), R.BLOCK_SMALL)
    assert not np.array_equal(M[:, 1, :], b["ref"]["M1"])
    # (the unit family cannot see it: N(0, 1) gradients and their float32 products times 2^e are integers already)


def test_planted_maximum_over_half_the_rows_fails_the_scale_assertion():
    case, b, M, e0, e1 = _planted("fam-c1_search-outlier-uniform", "half-max")
    assert e0 > b["e0"]
    with pytest.raises(AssertionError, match="scales"):
        R.check_fixed(case, M, (2.0 ** e0, 2.0 ** e1), R.BLOCK_SMALL)
    # the range family, its rows ordered so that the largest gradient sits in the second half
    br = R.build_case(BY_NAME["fam-c1_search-range-uniform"])
    g = br["g"] if np.abs(br["g"][br["g"].shape[0] // 2:]).max() == np.abs(br["g"]).max() else br["g"][::-1].copy()
    _, (h0, h1) = R.emulate(br["x"], g, br["ht"], 1, True, plant="half-max")
    assert (h0, h1) != R.restate_scales(g.shape[0], g, br["x"], br["ht"].anchor)
    # the outlier sits in the last row: its term, converted with the half maximum's scale, is not the integer it should be
    assert not np.array_equal(M[:, 0, :], b["ref"]["M0"])
    # equal entries have the same maximum over any rows: the same-sign family cannot see this error and does not claim to
    case, b, M, e0, e1 = _planted("headroom-c1_search-4097-same-sign", "half-max")
    assert (e0, e1) == (b["e0"], b["e1"])


def test_planted_strict_comparison_fails_on_the_anchors():
    for name in ("fam-c1_search-unit-levels", "fam-c1_search-integers-levels"):
        case, b, M, e0, e1 = _planted(name, "strict")
        with pytest.raises(AssertionError, match="M0 differs"):
            R.check_fixed(case, M, (2.0 ** e0, 2.0 ** e1), R.BLOCK_SMALL)


def test_planted_neighbouring_anchor_fails_the_offset_family():
    case, b, M, e0, e1 = _planted("fam-c1_search-unit-offset", "neighbour")
    with pytest.raises(AssertionError, match="M1 differs"):
        R.check_fixed(case, M, (2.0 ** e0, 2.0 ** e1), R.BLOCK_SMALL)
    _, b1 = R.fixed_bounds(b["truth"], e0, e1)
    assert R.worst_ratio(np.ldexp(M[:, 1, :].astype(np.float64), -e1), b["truth"]["T1"], b1) > 1.0
    case, b, M, e0, e1 = _planted("fam-c1_kept-unit-offset", "neighbour", "kept")
    with pytest.raises(AssertionError, match="kept flush"):
        R.check_fixed(case, M, (2.0 ** e0, 2.0 ** e1), R.BLOCK_SMALL)


def test_planted_dropped_tail_node_fails_the_restatement():
    for name, route in (("tail-c1_search-1", "search"), ("tail-c1_kept-129", "kept")):
        case, b, M, e0, e1 = _planted(name, "tail", route)
        with pytest.raises(AssertionError, match="M0 differs"):
            R.check_fixed(case, M, (2.0 ** e0, 2.0 ** e1), R.BLOCK_SMALL)


def test_planted_inverted_ratio_fails_the_kept_flush():
    case, b, M, e0, e1 = _planted("fam-c1_kept-unit-offset", "ratio", "kept")
    assert e0 != e1
    with pytest.raises(AssertionError, match="kept flush"):
        R.check_fixed(case, M, (2.0 ** e0, 2.0 ** e1), R.BLOCK_SMALL)


def test_old_rule_lets_a_coarse_fixed_point_through():
    """What the per-piece bound is for: 2^16 and 2^20 coarser quanta stay below ``1e-6 max|want|`` over the whole table."""
    case = BY_NAME["fam-c1_search-unit-uniform"]
    b = R.build_case(case)
    for bitsless in (16, 20):
        M = R.restate(b["x"], b["g"], b["ht"], 1, True, b["e0"] - bitsless, b["e1"] - bitsless)
        got1 = np.ldexp(M["M1"].astype(np.float64), -(b["e1"] - bitsless))
        assert np.abs(got1 - b["truth"]["T1"]).max() <= 1e-6 * np.abs(b["truth"]["T1"]).max()
        _, b1 = R.fixed_bounds(b["truth"], b["e0"], b["e1"])
        assert R.worst_ratio(got1, b["truth"]["T1"], b1) > 10.0


# ---- the route query, host only ---------------------------------------------------------------------------------------------------
def test_route_query_edges():
    from gnan_amd import _lib
    lib = _lib.lib()
    info = _lib.FpwlMomentsInfo()
    assert lib.gnan_fpwl_moments_describe(_lib.FpwlArgs(n=5, F=1, C=1), None, 1, 1, None) == -1
    assert lib.gnan_fpwl_rows_moments_describe(_lib.FpwlArgs(n=5, F=1, C=1), 1, None) == -1
    assert lib.gnan_fpwl_moments_describe(_lib.FpwlArgs(n=0, F=1, C=1), None, 1, 1, info) == 0 and info.kernel == _lib.MOMENTS_NONE
    assert lib.gnan_fpwl_rows_moments_describe(_lib.FpwlArgs(n=0, F=1, C=1), 1, info) == 0 and info.kernel == _lib.MOMENTS_NONE
    assert lib.gnan_fpwl_moments_describe(_lib.FpwlArgs(n=5, F=1, C=1), None, 1, 1, info) == -1        # validated as the launch is
    # rows: the channel chunk and the lanes per node
    for C, want in ((8, ("rows", 8, 1, 8)), (12, ("rows", 12, 1, 16)), (32, ("rows", 32, 1, 32)), (33, ("rows_pairs", 33, 1, 0)),
                    (40, ("rows_pairs", 40, 1, 0)), (42, ("rows_pairs", 42, 1, 0)), (43, ("rows", 43, 1, 64)), (64, ("rows", 64, 1, 64)),
                    (65, ("rows_pairs", 33, 2, 0)), (130, ("rows", 44, 3, 64))):
        a = _lib.FpwlArgs(n=2000, F=3, C=C, max_pieces=9, max_group_pieces=16, sum_features=1)
        assert lib.gnan_fpwl_rows_moments_describe(a, C, info) == 0
        assert (R.KERNELS[info.kernel], info.channel_chunk, info.n_chunks, info.cp2) == want, C
        assert (info.nodes_per_block, info.nodes_per_round, info.block_size, info.n_blocks) == (1024, 1024, 1024, 2)
