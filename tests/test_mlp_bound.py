"""tests/mlp_ref.py and tests/mlp_cases.py on the CPU: the conditions on the committed cases (no undecided hidden unit, the exact
family's ``< 2^24`` quanta), the float32 emulations of the lane forward and of ``feature_grads`` inside the bounds (held to
``2 k``: numpy has no fma), the planted errors the per-element check must catch — and the assertion that the project's
global-norm rule (``helpers.rule`` / ``helpers.grad_rule``) passes the graded-scale plants, which is why this module exists —
and the restated launch arithmetic against what the library's workspace queries report.  None of this needs a GPU."""
import numpy as np
import pytest

import helpers
import mlp_cases as MC
import mlp_ref as M

PTR = 0x1000          # a non-NULL "device" address: the workspace queries never follow it


def _lane_forward(c, plant=None):
    s = c.spec
    counts = M.fwd_counts("lane", s.n, s.F, s.L, s.H, s.C, s.sum_features)
    ref = M.forward(c.net, c.x, s.sum_features, counts, c.keep, s.p, scale=2)
    return ref, M.emulate_lane(c.net, c.x, s.sum_features, c.keep, s.p, plant=plant)


def _lane_backward(c, plant=None):
    s = c.spec
    counts = M.bwd_counts("lane", s.n, s.F, s.L, s.H, s.C, bool(s.p))
    ref = M.backward(c.net, c.x, c.g, s.sum_features, counts, c.keep, s.p, scale=2)
    got = M.stack_features([M.emulate_bwd(c.net, c.x, c.g, s.sum_features, k, c.keep, s.p, plant=plant) for k in range(s.F)], c.net)
    return ref, got


def _exact(c, with_g=True):
    s = c.spec
    return M.exact(c.net, c.x, s.sum_features, c.g if with_g and s.bwd else None, c.keep, s.p, MC.QW, MC.QX)


# ---------------------------------------------------------------------------------------------------------------------------
# conditions on the cases
# ---------------------------------------------------------------------------------------------------------------------------
def test_the_case_list_covers_every_route_in_both_directions():
    assert all(s.n <= 600 and s.F <= 6 and s.H <= 64 for s in MC.SPECS.values())
    for route in M.FWD_ROUTES:
        for drop in (False, True) if route != "point" else (False,):
            assert sum(route in MC.fwd_routes(s) and bool(s.p) == drop for s in MC.SPECS.values()) >= 4, (route, drop)
    for route in M.BWD_ROUTES:
        for drop in (False, True):
            assert sum(route in MC.bwd_routes(s) and bool(s.p) == drop for s in MC.SPECS.values()) >= 3, (route, drop)
    assert 40 <= len(MC.ALL) <= 75 and 40 <= len(MC.BACKWARD) <= 60


@pytest.mark.parametrize("name", [nm for nm in MC.BACKWARD if not MC.SPECS[nm].family.startswith("exact")])
def test_no_committed_backward_case_has_an_undecided_unit(name):
    und, judged = MC.undecided(MC.case(name))
    assert und == 0, (name, und, judged)
    assert judged > 0 or MC.SPECS[name].L == 2


@pytest.mark.parametrize("name", MC.EXACT)
def test_every_exact_case_stays_below_2_to_the_24_quanta(name):
    ex = _exact(MC.case(name))                       # (asserts the condition on every magnitude)
    assert ex.worst_bits < 24
    assert (ex.grads is not None) == MC.SPECS[name].bwd


def test_the_exact_zero_case_holds_exact_zeros_with_a_gradient_waiting_behind_them():
    c = MC.case("exact-zero-n65-F2-L3-H8-C3")
    z2 = np.einsum("fnj,fij->fni", np.maximum(c.x.T[:, :, None] * c.net.w_first[:, None, :] + c.net.b_first[:, None, :], 0), c.net.w_mid[0]) \
        + c.net.b_mid[0][:, None, :]
    assert (z2[:, :, -1] == 0).all()
    strict = M.backward(c.net, c.x, c.g, False, M.bwd_counts("lane", 65, 2, 3, 8, 3, False))
    loose = M.backward(c.net, c.x, c.g, False, M.bwd_counts("lane", 65, 2, 3, 8, 3, False), ge=True)
    assert (strict.truth["b_mid"][0, :, -1] == 0).all() and (strict.bound["b_mid"][0, :, -1] == 0).all()
    assert (loose.truth["b_mid"][0, :, -1] != 0).all()


def test_the_hash_restatement_draws_about_p_and_depends_on_every_coordinate():
    m = MC.keep_mask(MC.DROP_SEED, 0.6, 300, 3, 2, 33)
    assert m.shape == (300, 3, 2, 33) and abs(float(m.mean()) - 0.4) < 0.01
    assert not np.array_equal(m[0], m[1]) and not np.array_equal(m[:, 0], m[:, 1]) and not np.array_equal(m[:, :, 0], m[:, :, 1])
    assert not np.array_equal(m, MC.keep_mask(MC.DROP_SEED + (1 << 32), 0.6, 300, 3, 2, 33))


# ---------------------------------------------------------------------------------------------------------------------------
# the emulations lie inside the bounds
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MC.ALL)
def test_the_lane_emulation_lies_inside_the_forward_bound(name):
    c = MC.case(name)
    ref, got = _lane_forward(c)
    ratio = M.assert_within(got, ref.truth, ref.bound, name)
    assert ratio <= 1.0
    if name in MC.EXACT:
        assert np.array_equal(got.astype(np.float64), _exact(c, with_g=False).out), "bit for bit"


@pytest.mark.parametrize("name", MC.BACKWARD)
def test_the_feature_grads_emulation_lies_inside_the_backward_bound(name):
    c = MC.case(name)
    ref, got = _lane_backward(c)
    ratio, _ = M.hold_grads(got, ref, name)
    assert ratio <= 1.0
    if name in MC.EXACT:
        ex = _exact(c)
        for nm, a in got.items():
            assert np.array_equal(a.astype(np.float64), ex.grads[nm]), (name, nm)


@pytest.mark.parametrize("name", MC.MOVED)
def test_a_power_of_two_moves_the_exponent_only_in_the_reference_and_the_emulations(name):
    c, unit = MC.case(name), MC.case(MC.base_of(name))
    e = c.spec.e
    assert np.array_equal(np.ldexp(_lane_forward(unit)[1], e), _lane_forward(c)[1])
    a, b = _lane_backward(unit)[1], _lane_backward(c)[1]
    for nm in a:
        assert np.array_equal(np.ldexp(a[nm], -e if nm in ("w_last", "b_last") else 0), b[nm]), nm
        nz = np.abs(b[nm][b[nm] != 0])
        assert nz.size == 0 or (nz.min() >= 2.0 ** -126 and nz.max() < 2.0 ** 127), "inside the normal range"


# ---------------------------------------------------------------------------------------------------------------------------
# planted errors
# ---------------------------------------------------------------------------------------------------------------------------
def _live_unit(c, k):
    """A first-layer unit of feature ``k`` that is alive at most nodes."""
    a1 = c.x[:, k:k + 1].astype(np.float64) * c.net.w_first[k][None, :] + (0 if c.net.b_first is None else c.net.b_first[k][None, :])
    return int(np.argmax((a1 > 0).sum(0)))


def test_plant_one_column_of_w2_skipped_for_one_feature():
    c = MC.case("random-n65-F3-L3-H33-C5-nobias")
    ref, got = _lane_forward(c, plant=("skip_w2_col", 1, _live_unit(c, 1)))
    assert not M.within(got, ref.truth, ref.bound)
    with pytest.raises(AssertionError, match="elements outside their bound; first at"):
        M.assert_within(got, ref.truth, ref.bound, "plant")
    blocks = np.abs(got - ref.truth).reshape(65, 3, 5) > ref.bound.reshape(65, 3, 5)
    assert blocks[:, 1].any() and not blocks[:, 0].any() and not blocks[:, 2].any(), "only the planted feature is off"


def test_plant_the_last_node_of_a_ragged_tile_evaluated_at_zero():
    c = MC.case("random-n33-F5-L3-H33-C3-sum")
    ref, got = _lane_forward(c, plant=("x0", 32))
    off = (np.abs(got - ref.truth) > ref.bound).any(1)
    assert off[32] and not off[:32].any()


def test_plant_one_mask_flipped_at_a_decided_unit():
    c = MC.case("random-n65-F3-L3-H33-C5-nobias")
    ref, clean = _lane_backward(c)
    assert M.grads_within(clean, ref)
    for layer in (0, 1):
        got = M.stack_features([M.emulate_bwd(c.net, c.x, c.g, False, k, plant=("flip", 7, layer, _live_unit(c, k)) if k == 2 else None)
                                for k in range(3)], c.net)
        assert not M.grads_within(got, ref), layer


def test_plant_greater_or_equal_for_greater_on_the_exact_zero_case():
    c = MC.case("exact-zero-n65-F2-L3-H8-C3")
    ref, clean = _lane_backward(c)
    ex = _exact(c)
    assert all(np.array_equal(clean[nm].astype(np.float64), ex.grads[nm]) for nm in clean)
    _, got = _lane_backward(c, plant=("ge",))
    assert not M.within(got["b_mid"], ref.truth["b_mid"], ref.bound["b_mid"])
    assert (got["b_mid"][0, :, -1] != 0).all() and not np.array_equal(got["b_mid"].astype(np.float64), ex.grads["b_mid"])
    with pytest.raises(AssertionError):
        M.hold_grads(got, ref, "plant")


def test_plant_one_splits_block_left_out():
    c = MC.case("random-n65-F3-L3-H33-C5-nobias")
    assert M.node_splits(65, 3, "lane")[0] == 3
    ref, _ = _lane_backward(c)
    _, got = _lane_backward(c, plant=("drop_split", 1))
    assert not M.grads_within(got, ref)


@pytest.mark.parametrize("name", [nm for nm in MC.GRADED if MC.SPECS[nm].L == 3 and not MC.SPECS[nm].sum_features])
def test_plant_d_b_mid_of_the_smallest_graded_feature_zeroed_passes_the_global_rule_and_fails_here(name):
    """THE reason for this module: the smallest feature's whole ``d b_mid`` gone, and ``helpers.grad_rule`` — the rule every
    direct-path gradient test used until now — says yes."""
    c = MC.case(name)
    ref, got = _lane_backward(c)
    assert M.grads_within(got, ref)
    last = c.spec.F - 1
    assert np.abs(got["b_mid"][0, last]).max() > 0
    got["b_mid"] = got["b_mid"].copy()
    got["b_mid"][0, last] = 0.0
    ok, e_build, _, _ = helpers.grad_rule(got, ref.truth)
    assert ok and e_build <= 1e-5, "the global-norm rule is blind to this plant"
    assert not M.grads_within(got, ref)
    assert not M.within(got["b_mid"][0, last], ref.truth["b_mid"][0, last], ref.bound["b_mid"][0, last])


@pytest.mark.parametrize("name", [nm for nm in MC.GRADED if MC.SPECS[nm].L == 3])
def test_plant_a_skipped_column_in_the_smallest_graded_feature_passes_the_global_rule_and_fails_here(name):
    c = MC.case(name)
    last = c.spec.F - 1
    ref, got = _lane_forward(c, plant=("skip_w2_col", last, _live_unit(c, last)))
    ok, e_build, _ = helpers.rule(got, ref.truth)
    assert ok and e_build <= 1e-5, "the global-norm rule is blind to this plant"
    if c.spec.sum_features:
        # under the feature sum the smallest feature drowns in the sum's own rounding: the per-FEATURE truth still shows it
        clean = M.emulate_lane(c.net, c.x, True, c.keep, c.spec.p)
        assert np.abs(got - clean).max() > 0
    else:
        assert not M.within(got, ref.truth, ref.bound)


# ---------------------------------------------------------------------------------------------------------------------------
# the restated launch arithmetic
# ---------------------------------------------------------------------------------------------------------------------------
GRID = [(n, F, H) for n in (1, 31, 32, 33, 64, 65, 127, 128, 129, 255, 256, 257, 300, 512, 600, 5000, 300000) for F in (1, 2, 3, 4, 5, 6, 100, 600)
        for H in (8, 32, 33, 64)]


def test_node_splits_equal_what_the_workspace_queries_report():
    from gnan_amd import _lib
    lib = _lib.lib()
    for n, F, H in GRID:
        for route, fn, Ls in (("lane", lib.gnan_fmlp_bwd_workspace_bytes, (2, 3)), ("mfma", lib.gnan_fmlp_bwd_mfma_workspace_bytes, (3,)),
                              ("mc", lib.gnan_fmlp_mc_bwd_workspace_bytes, (3,))):
            for L in Ls:
                C = 3
                a = _lib.FmlpBwdArgs(x=PTR, n=n, x_stride=F, F=F, L=L, H=H, C=C, w_first=PTR, b_first=PTR, w_mid=PTR, b_mid=PTR, w_last=PTR,
                                     b_last=PTR, sum_features=0, grad=PTR, grad_stride=F * C, d_w_first=PTR, d_b_first=PTR, d_w_mid=PTR,
                                     d_b_mid=PTR, d_w_last=PTR, d_b_last=PTR)
                blk = 2 * F * H + (F * H * H + F * H if L == 3 else 0) + F * C * H + F * C
                splits, nps = M.node_splits(n, F, route)
                assert fn(a) == (splits * blk * 4 if splits > 1 else 0), (route, n, F, H, L)
                assert splits * nps >= n and nps % (4 if route == "lane" and splits > 1 else 1 if route == "lane" else 128) == 0


def test_feature_chunks_equal_what_the_workspace_queries_report():
    from gnan_amd import _lib
    lib = _lib.lib()
    for n, F, H in GRID:
        for mc, fn in ((False, lib.gnan_fmlp_fwd_workspace_bytes), (True, lib.gnan_fmlp_mc_fwd_workspace_bytes)):
            C = 3
            sizes = []
            for sum_features in (0, 1):
                a = _lib.FmlpArgs(x=PTR, n=n, x_stride=F, F=F, L=3, H=H, C=C, w_first=PTR, b_first=PTR, w_mid=PTR, b_mid=PTR, w_last=PTR,
                                  b_last=PTR, sum_features=sum_features, out=PTR, out_stride=F * C, algo=_lib.FMLP_MFMA)
                sizes.append(fn(a))
            real, fc, asked = M.feature_chunks(n, F, H, mc)
            assert sizes[1] - sizes[0] == (asked * n * C * 4 if asked > 1 else 0), (mc, n, F, H)
            assert fc % 2 == 0 and real <= asked and (real - 1) * fc < F <= real * fc


def test_the_covers_equal_the_librarys_refusals_on_the_host():
    """The cover predicates of mlp_ref against the entry points themselves: outside the cover the call is refused with
    GNAN_ERR_UNSUPPORTED on the host, before any HIP call (no GPU here: nothing could have been launched)."""
    from gnan_amd import _lib
    lib = _lib.lib()
    for L, H, C in [(2, 8, 3), (5, 8, 3), (3, 65, 3), (3, 8, 9), (3, 8, 65), (1, 8, 3)]:
        a = _lib.FmlpBwdArgs(x=PTR, n=10, x_stride=2, F=2, L=L, H=H, C=C, w_first=PTR, w_mid=PTR, w_last=PTR, sum_features=0, grad=PTR,
                             grad_stride=2 * C, d_w_first=PTR, d_w_mid=PTR, d_w_last=PTR)
        for route, fn in (("lane", lib.gnan_fmlp_bwd), ("mfma", lib.gnan_fmlp_bwd_mfma), ("mc", lib.gnan_fmlp_mc_bwd)):
            if not M.bwd_covers(route, L, H, C):
                assert fn(a, None) == _lib.ERR_UNSUPPORTED, (route, L, H, C)
        f = _lib.FmlpArgs(x=PTR, n=10, x_stride=2, F=2, L=L, H=H, C=C, w_first=PTR, w_mid=PTR, w_last=PTR, sum_features=0, out=PTR,
                          out_stride=2 * C, algo=_lib.FMLP_MFMA)
        if not M.fwd_covers("mfma", 10, 2, L, H, C, False, False):
            assert lib.gnan_fmlp_fwd(f, None) == _lib.ERR_UNSUPPORTED, (L, H, C)
        if not M.fwd_covers("mc", 10, 2, L, H, C, False, False):
            assert lib.gnan_fmlp_mc_fwd(f, None) == _lib.ERR_UNSUPPORTED, (L, H, C)
