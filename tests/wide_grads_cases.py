"""Cases of the wide instance of ``gnan_fpwl_param_grads`` (csrc/fpwl_grad.hip: ``fpwl_grad3_kernel<128, 1, CQ>``, L == 3 with
64 < H <= 128) and the bound they are held to — TEST INFRASTRUCTURE ONLY, shared by tests/test_wide_grads_host.py (the numpy
emulation, no GPU) and tests/test_gpu_wide_grads.py (the kernel).

``grads_ref.route_of`` and ``Case.route`` know nothing of H (they would name the sweep for C <= 4), so nothing here asks them:
the truth is ``grads_ref.exact_grads(ex, A, M, exps, "grad3")`` and the bound ``grads_ref.check(got, exact, k, chunks)`` with

    k = grads_ref.k_piece(3, H, w, nl, NG)        w: channel width of the chunk, NG: groups of the launched instance

The wide instance keeps the quad split (four adjacent lanes take consecutive blocks of ``q = ceil(H / 4)`` units, then the fixed
two-step butterfly) and the in-order group add of ``fpwl_grad3_kernel``, so ``k_piece`` counts its roundings unchanged and
``grads_ref.emulate_piece`` is its order.  What it launches, next to the kernel's own comment:

    channels of the launch   instance                       NG   threads   k at H = 128, nl = 3
    1 .. 4                   fpwl_grad3_kernel<128, 1, 1>    1    512       1 + 36 + (1 + 2 + 34) + (6 + 1) = 81
    5 .. 8                   fpwl_grad3_kernel<128, 1, 2>    1    512       82
    9 .. 16                  fpwl_grad3_kernel<128, 1, 4>    1    512       83 .. 84
    17 .. 64                 fpwl_grad3_kernel<128, 1, 16>   1    512       85 .. 96

(two groups spill registers at every channel count: DESIGN section 4.5), C > 64 in chunks of 64 through the Python wrapper.
"""
import numpy as np

import grads_cases as GC
import grads_ref as G

WIDE_NG = 1            # groups of every wide instance gnan_fpwl_param_grads launches

# name -> (F, H, C, n_live, keywords of grads_ref.random_case); seed 11, the default (torch, CPU) builder unless ``tables`` is given
RANDOM = {
    "H65-C1": (2, 65, 1, 5, {}),
    "H96-C5": (2, 96, 5, 7, {}),
    "H127-C2-no-bias": (2, 127, 2, 5, dict(bias=False)),
    "H128-C1-one-feature-empty": (2, 128, 1, 0, dict(live=[9, 0])),
    "H128-C40": (1, 128, 40, 3, {}),
    "H128-C65-wrapper": (1, 128, 65, 3, {}),
    "H128-C4-float-moments": (2, 128, 4, 6, dict(fixed=False)),
}
LDS_CORNER = "H128-C64-max-pieces-8192"      # the largest shape served: 139 296 bytes of dynamic LDS
INTEGER = "integer-H96"

_BUILT = {}
_REF = {}


def _integer_case(name, H=96, C=2, seed=953):
    """``grads_cases._integer_case`` at H = 96: weights in {-2 .. 2}, first-layer kinks at the half integers 0.5 .. H - 0.5, integer
    anchors right of all of them, integer moments with a slope moment of 2^30 + 1 cancelled by -2^30 in the piece next to it."""
    f = GC._integer_net(3, H, C, seed)
    first = float(H + 24)
    extra = [first + i for i in range(8)]
    picked = (first, first + 1.0, first + 3.0, first + 5.0)

    def live(A):
        return [t for t in range(1, len(A)) if float(A[t]) in picked]

    def edit(k, A, M):
        rng = np.random.default_rng(951)
        lv = [t for t in range(len(M)) if M[t].any()]
        for t in lv:
            M[t] = rng.integers(-4, 5, size=M[t].shape)
            M[t, 0, 0] = 1
        M[lv[0], 1, 0] = (1 << 30) + 1
        M[lv[1], 1, 0] = -(1 << 30)
        return M
    return G.hand_case(name, [f], 3, H, C, [extra], [live], np.random.default_rng(952), exps=(0, 0), moments=edit, exact=True)


def case(name, tables=None):
    """The built case (cached; with ``tables`` — another table builder, ``tables(p) -> PwlTables`` — built afresh)."""
    if tables is None and name in _BUILT:
        return _BUILT[name]
    if name == INTEGER:
        c = _integer_case(name)
    elif name == LDS_CORNER:
        c = G.random_case(name, 1, 3, 128, 64, 11, 3, max_pieces=8192, tables=tables)
    else:
        F, H, C, n_live, kw = RANDOM[name]
        c = G.random_case(name, F, 3, H, C, 11, n_live, tables=tables, **kw)
    if tables is None:
        _BUILT[name] = c
    return c


def reference(case):
    """Exact truth and magnitudes of every feature (cached on the case name): the per-piece contract, whatever C."""
    if case.name not in _REF:
        _REF[case.name] = [G.exact_grads(ex, A, case.feature_moments(k), case.exps, "grad3")
                           for k, (ex, A) in enumerate(zip(case.exs, case.anchors))]
    return _REF[case.name]


def hold(case, per_feature, NG=WIDE_NG, k_scale=1):
    """Worst ratio of a whole result (list of per-feature dicts) to the bound; asserts nothing.  ``k_scale = 2``: the numpy
    emulation (no fma: a multiply-add rounds twice).  Chunks of 64 channels as the wrapper cuts them."""
    C, H = case.p.C, case.p.H
    chunks = -(-C // 64)
    widths = {min(64, C - c0) for c0 in range(0, C, 64)}
    worst, where, zb = 0.0, None, 0
    for f, (got, ex) in enumerate(zip(per_feature, reference(case))):
        k = k_scale * max(G.k_piece(3, H, w, ex.nl, NG) for w in widths)
        r, name, z = G.check(got, ex, k, chunks)
        zb += z
        if r > worst:
            worst, where = r, (f, name)
    return worst, where, zb


def emulate(case, NG=WIDE_NG, plant=None, edit=None):
    """``grads_ref.emulate_piece`` per feature, stored as float32 (the one rounding at the store).  C > 64: chunk by chunk as the
    wrapper does, the hidden layers' gradients added in float32.  ``edit(w) -> w`` changes the weights the emulation sees."""
    C = case.p.C
    out = []
    for f in range(case.p.F):
        w, A, M = G.weights_f64(case.p, f), case.anchors[f], case.feature_moments(f)
        if edit is not None:
            w = edit(w)
        total = None
        for c0 in range(0, C, 64):
            c1 = min(C, c0 + 64)
            g = G.emulate_piece((w[0], w[1], w[2], w[3][c0:c1]), A, M[:, :, c0:c1], case.exps, NG, plant)
            with np.errstate(over="ignore"):
                g = {n: v.astype(np.float32) for n, v in g.items()}
            if total is None:
                total = g
            else:
                for n in ("w_first", "b_first", "w_mid", "b_mid"):
                    total[n] = total[n] + g[n]
                total["w_last"] = np.concatenate([total["w_last"], g["w_last"]], 0)
                total["b_last"] = np.concatenate([total["b_last"], g["b_last"]], 0)
        out.append(total)
    return out


def sixteen_accumulators(w):
    """A kernel that kept the 16 accumulators of H <= 64: ``W2[:, 64:]`` never read."""
    w1, b1, ((W2, b2),), wl = w
    W2 = W2.copy()
    W2[:, 64:] = 0.0
    return w1, b1, [(W2, b2)], wl


def truth_bits(case, per_feature):
    """Whether every element equals the truth exactly (the integer family)."""
    for got, ex in zip(per_feature, reference(case)):
        for name, a in got.items():
            want = np.array([float(t) for t in ex.grads[name].reshape(-1)], dtype=np.float64)
            if not np.array_equal(np.asarray(a).reshape(-1).astype(np.float64), want):
                return False, name
    return True, None
