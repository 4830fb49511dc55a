"""Exact reference of the shape-function tables (no GPU, no product code): kinks, values, slopes and slope jumps of a ReLU
MLP of a scalar whose weights are float32, in integer arithmetic, and the per-element bound a built table is held to.

**Truth.**  A float32 is a dyadic rational, so every weight times ``2^S`` (one ``S`` for the whole feature) is a Python
integer.  On an interval on which no hidden unit changes its activation, the pre-activations of hidden layer ``l`` are
``(A_l x + B_l) / 2^(S (l + 1))`` with integer vectors ``A_l``, ``B_l`` that depend on the activation pattern only (masked
products of the weight matrices), and ``f = (A_out x + B_out) / 2^(S L)``.  The kinks are found layer by layer: layer 1 is
``-b / w``; inside each open interval between consecutive distinct kinks found so far, and on both rays, the pattern of the
layers below is read at ONE interior rational point, the next layer's forms follow, and a unit's root ``-B / A`` is a kink where
it lies strictly inside the interval (a root on an end of the interval is a kink already).  No sample nodes, no floating point:
the roots are ``fractions.Fraction``.  :meth:`ExactFeature.preacts_direct` evaluates the hidden layers at a float32 point by
plain integer dot products, without the intervals — the brute-force check of the interval argument.

**Bound** of a table entry at probe ``x`` in piece ``p`` (anchor ``a``, right anchor ``a'``, exact slope ``s`` inside the piece) of
feature ``k``, channel ``c`` (:func:`check_values`)::

    |T(x) - f(x)| <= gamma32_k (|f(a)| + |s| |x - a|)                               the look-up's float32 roundings
                     + (1 + gamma32_k) ulp32(a') sum_{r in (pred(a'), a']} |J_r| max(1, |x - a| / w)   the secant slope
                     + gamma64_m (mag(a) + (mag(a) + mag(a')) max(1, |x - a| / w))   the builder's float64 evaluation
                     + 2^-53 |f(x)| + the float32 underflow steps

``k`` counts the float32 roundings on the longer path — ``slope`` stored, ``x - a``, the look-up's fma: 3; the torch
restatement ``val + slope * (x - a)`` multiplies and adds separately: 4 —; ``J_r`` is the slope jump at kink ``r`` (the slope
of a piece is the secant between anchors that are rounded UP, so it carries ``J (a' - r) / w`` of the next piece's slope;
``w = a' - a``, and ``w = 1`` on the left ray, whose secant runs from ``a - 1`` to ``a``: there ``|x - a| / w`` is unbounded);
``mag`` is the network with every weight, bias and input replaced by its magnitude (the sum of the |terms| of the float64
evaluation) and ``m = L (H + 2) + 4`` its float64 roundings on one path (an fma per term, the bias, the secant's subtraction
and division).  The magnitudes are those of the feature's own channel at that piece.  A bound of zero demands an exact zero.
"""
import bisect
from fractions import Fraction

import numpy as np

U32 = 2.0 ** -24
U64 = 2.0 ** -53
F32_MAX = float(np.finfo(np.float32).max)
CLAMP = 3.0e38                                  # the builders clamp a kink to +-3e38 before rounding it up


def gamma(k, u):
    return k * u / (1.0 - k * u)


def _as_ratio(v):
    n, d = float(v).as_integer_ratio()
    return n, d.bit_length() - 1                # v = n / 2^e


def _scaled(arr, S):
    """float array -> object array of the integers ``v * 2^S``."""
    flat = []
    for v in np.asarray(arr, dtype=np.float64).reshape(-1):
        n, e = _as_ratio(v)
        flat.append(n << (S - e))
    out = np.empty(len(flat), dtype=object)
    out[:] = flat
    return out.reshape(np.shape(arr))


def frac(x):
    return Fraction(*float(x).as_integer_ratio())


def round_up_f32(r):
    """Smallest float32 not below the rational ``r`` (clamped to +-3e38 first, as the builders do), decided exactly."""
    r = min(max(r, Fraction(-CLAMP)), Fraction(CLAMP))
    f = np.float32(float(r))
    if frac(f) < r:
        f = np.nextafter(f, np.float32(np.inf))
    return np.float32(f)


def round_nearest_f32(r):
    return np.float32(float(min(max(r, Fraction(-CLAMP)), Fraction(CLAMP))))


def up(a):
    return np.nextafter(np.float32(a), np.float32(np.inf))


def down(a):
    return np.nextafter(np.float32(a), np.float32(-np.inf))


class ExactFeature:
    """One feature's network ``R -> R^C`` in exact arithmetic.  ``w1 [H]``, ``b1 [H]``, ``mids = [(W [H, H], b [H]), ...]``,
    ``wl [C, H]``, ``bl [C]`` as float arrays (biases may be None)."""

    def __init__(self, w1, b1, mids, wl, bl):
        H, C = len(w1), len(wl)
        zeros = np.zeros(H)
        b1 = zeros if b1 is None else b1
        mids = [(W, zeros if b is None else b) for W, b in mids]
        bl = np.zeros(C) if bl is None else bl
        every = [w1, b1, wl, bl] + [q for Wb in mids for q in Wb]
        S = 0
        for a in every:
            for v in np.unique(np.asarray(a, dtype=np.float64)):
                S = max(S, _as_ratio(v)[1])
        self.S, self.H, self.C, self.L = S, H, C, len(mids) + 2
        self.w1, self.b1 = _scaled(w1, S), _scaled(b1, S)
        self.mids = [(_scaled(W, S), _scaled(b, S)) for W, b in mids]
        self.wl, self.bl = _scaled(wl, S), _scaled(bl, S)
        self.f64 = dict(w1=np.abs(np.asarray(w1, np.float64)), b1=np.abs(np.asarray(b1, np.float64)),
                        mids=[(np.abs(np.asarray(W, np.float64)), np.abs(np.asarray(b, np.float64))) for W, b in mids],
                        wl=np.abs(np.asarray(wl, np.float64)), bl=np.abs(np.asarray(bl, np.float64)))
        self._find_kinks()

    # ---- forms on an interval --------------------------------------------------------------------
    def _forms(self, x, depth):
        """Forms ``[(A_0, B_0), ..., (A_depth, B_depth)]`` of the hidden layers (``depth = L - 1``: the output's last) on the
        interval whose activation pattern is the one at the rational ``x`` (an interior point)."""
        p, q = x.numerator, x.denominator
        S = self.S
        A, B = self.w1, self.b1
        out = [(A, B)]
        for l in range(1, depth + 1):
            on = (A * p + B * q) > 0
            Am, Bm = np.where(on, A, 0), np.where(on, B, 0)
            if l <= self.L - 2:
                W, b = self.mids[l - 1]
            else:
                W, b = self.wl, self.bl
            A, B = W.dot(Am), W.dot(Bm) + b * (1 << (S * l))
            out.append((A, B))
        return out

    def _interior(self, D, i):
        if not D:
            return Fraction(0)
        if i == 0:
            return D[0] - 1
        if i == len(D):
            return D[-1] + 1
        return (D[i - 1] + D[i]) / 2

    def _find_kinks(self):
        kinks = {Fraction(-int(b), int(a)) for a, b in zip(self.w1, self.b1) if a != 0}
        for depth in range(1, self.L - 1):
            D = sorted(kinks)
            for i in range(len(D) + 1):
                A, B = self._forms(self._interior(D, i), depth)[depth]
                lo = D[i - 1] if i > 0 else None
                hi = D[i] if i < len(D) else None
                for a, b in zip(A, B):
                    if a != 0:
                        r = Fraction(-int(b), int(a))
                        if (lo is None or r > lo) and (hi is None or r < hi):
                            kinks.add(r)
        self.kinks = sorted(kinks)
        self.forms = [self._forms(self._interior(self.kinks, i), self.L - 1) for i in range(len(self.kinks) + 1)]
        den = 1 << (self.S * self.L)
        self.slopes = np.array([[int(a) / den for a in fm[-1][0]] for fm in self.forms], dtype=np.float64)       # [I, C]
        # slope jump at kink i (between intervals i and i + 1), correctly rounded from the exact difference
        self.jumps = np.array([[abs(int(a1) - int(a0)) / den for a0, a1 in zip(self.forms[i][-1][0], self.forms[i + 1][-1][0])]
                               for i in range(len(self.kinks))], dtype=np.float64).reshape(len(self.kinks), self.C)

    # ---- evaluation -----------------------------------------------------------------------------
    def interval(self, x):
        """Index of the interval ``[kink i-1, kink i)`` that holds the rational ``x``."""
        return bisect.bisect_right(self.kinks, x)

    def f(self, x):
        """``f(x) [C]`` at the float ``x``, each channel the correctly rounded float64 of the exact value."""
        xr = frac(x)
        A, B = self.forms[self.interval(xr)][-1]
        p, q = xr.numerator, xr.denominator
        den = q << (self.S * self.L)
        return np.array([int(a * p + b * q) / den for a, b in zip(A, B)], dtype=np.float64)

    def f_many(self, xs):
        return np.stack([self.f(x) for x in xs]) if len(xs) else np.zeros((0, self.C))

    def preact_zero(self, x):
        """Is some hidden unit's exact pre-activation zero at the float ``x``?  (First-layer units with ``w = 0`` excluded.)"""
        xr = frac(x)
        p, q = xr.numerator, xr.denominator
        for l, (A, B) in enumerate(self.forms[self.interval(xr)][:-1]):
            z = A * p + B * q
            hit = (z == 0) & (self.w1 != 0) if l == 0 else z == 0
            if bool(hit.any()):
                return True
        return False

    def preacts_direct(self, x):
        """Hidden pre-activations at the float ``x`` by plain integer dot products (no intervals): ``[z_0, z_1, ...]``, layer
        ``l`` scaled by ``q 2^(S (l + 1))``, and the output scaled likewise as the last entry."""
        xr = frac(x)
        p, q = xr.numerator, xr.denominator
        z = self.w1 * p + self.b1 * q
        out = [z]
        for l, (W, b) in enumerate(self.mids + [(self.wl, self.bl)], start=1):
            z = W.dot(np.where(z > 0, z, 0)) + b * (q << (self.S * l))
            out.append(z)
        return out

    def mag(self, xs):
        """The network of magnitudes at ``xs [n]`` -> ``[n, C]`` float64: the sum of the |terms| of a float64 evaluation."""
        m = np.abs(np.asarray(xs, np.float64))[:, None] * self.f64["w1"][None, :] + self.f64["b1"][None, :]
        for W, b in self.f64["mids"]:
            m = m @ W.T + b[None, :]
        return m @ self.f64["wl"].T + self.f64["bl"][None, :]

    # ---- what a table of this feature must hold ------------------------------------------------------
    def expected_anchors(self):
        """Sorted distinct float32 anchors: every kink rounded up, and ``nextafter(a)`` behind each anchor ``a`` at which a
        hidden pre-activation is exactly zero.  Returns ``(anchors, point)`` with ``point`` the successors that were added."""
        base = sorted({float(round_up_f32(r)) for r in self.kinks})
        have = set(base)
        point = []
        for a in base:
            if self.preact_zero(a):
                n = float(up(a))
                if n not in have:
                    point.append(n)
        return np.array(sorted(have | set(point)), dtype=np.float32), np.array(sorted(point), dtype=np.float32)


def features_of(p):
    """``StackedMLP`` (CPU tensors, L >= 2) -> one :class:`ExactFeature` per feature."""
    out = []
    for k in range(p.F):
        mids = []
        for l in range(p.L - 2):
            mids.append((p.w_mid[l][k].numpy(), None if p.b_mid is None else p.b_mid[l][k].numpy()))
        out.append(ExactFeature(p.w_first[k].numpy(), None if p.b_first is None else p.b_first[k].numpy(), mids,
                                p.w_last[k].numpy(), None if p.b_last is None else p.b_last[k].numpy()))
    return out


# =============================================================================
# a built table against the truth
# =============================================================================
def feature_table(t, k):
    """``(anchor [P + 1], val [P + 1, C], slope [P + 1, C])`` of feature ``k`` as numpy arrays (tables on the CPU)."""
    off = t.off.tolist()
    s = slice(off[k], off[k + 1])
    return t.anchor[s].numpy(), t.val[s].numpy(), t.slope[s].numpy()


def distinct_breakpoints(anchor):
    return np.unique(anchor[1:]) if len(anchor) > 1 else np.zeros(0, np.float32)


def check_anchors(ex, anchor):
    """The distinct anchors against :meth:`ExactFeature.expected_anchors`, value for value (no tolerance; -0.0 == 0.0).
    Returns a list of complaints."""
    want, _ = ex.expected_anchors()
    got = distinct_breakpoints(anchor)
    if len(anchor) > 1 and float(anchor[0]) != float(anchor[1]):
        return [f"piece 0 is anchored at {anchor[0]!r}, not at the first breakpoint {anchor[1]!r}"]
    if len(want) == len(got) and bool((want == got).all()):
        return []
    missing = sorted(set(want.tolist()) - set(got.tolist()))
    extra = sorted(set(got.tolist()) - set(want.tolist()))
    return [f"anchors differ: missing {missing[:6]} ({len(missing)}), unexpected {extra[:6]} ({len(extra)})"]


def check_no_kink_inside(ex, anchor, direct=True):
    """No piece holds a kink: between a piece's first float32 value and its last there is no exact kink (the kink that ends the
    piece lies above the last value, its anchor being rounded up); with ``direct`` also by the activation patterns of every
    hidden unit at those two values, from plain integer dot products — equal patterns at both ends make every layer affine
    between them, by induction over the layers.  Returns a list of complaints."""
    bad = []
    bps = distinct_breakpoints(anchor)
    D = [min(max(r, Fraction(-CLAMP)), Fraction(CLAMP)) for r in ex.kinks]      # (the builders' clamp: no float32 lies beyond)
    n = len(bps)
    for i in range(n + 1):
        first = None if i == 0 else bps[i - 1]
        last = None if i == n else down(bps[i])
        lo = 0 if first is None else bisect.bisect_right(D, frac(first))
        hi = len(D) if last is None else bisect.bisect_right(D, frac(last))
        if hi != lo:
            bad.append(f"piece [{first}, {last}] holds {hi - lo} kink(s), the first at {float(D[lo])!r}")
        if direct and first is not None and last is not None and last > first:
            za, zb = ex.preacts_direct(first)[:-1], ex.preacts_direct(last)[:-1]
            for l, (u, v) in enumerate(zip(za, zb)):
                diff = np.nonzero((u > 0) != (v > 0))[0]
                if len(diff):
                    bad.append(f"piece [{first}, {last}]: unit {int(diff[0])} of hidden layer {l + 1} switches inside")
    return bad


def probes_of(anchor):
    """The probes of one feature's table, float32: every distinct anchor with its predecessor and successor, per bounded
    piece the midpoint and a point one tenth from each end, 1, 1e2 and 1e4 beyond the outer anchors, and 0, -0.0, 1, the
    smallest denormal and +-3e38."""
    bps = distinct_breakpoints(anchor).astype(np.float32)
    xs = [np.float32(0.0), np.float32(-0.0), np.float32(1.0), np.float32(1.4e-45), np.float32(3e38), np.float32(-3e38)]
    for b in bps:
        xs += [b, down(b), up(b)]
    for a, b in zip(bps[:-1], bps[1:]):
        w = np.float64(b) - np.float64(a)
        xs += [np.float32(np.float64(a) + 0.5 * w), np.float32(np.float64(a) + 0.1 * w), np.float32(np.float64(b) - 0.1 * w)]
    if len(bps):
        for d in (1.0, 1e2, 1e4):
            xs += [np.float32(np.float64(bps[0]) - d), np.float32(np.float64(bps[-1]) + d)]
    else:
        xs += [np.float32(s * d) for d in (1.0, 1e2, 1e4) for s in (-1.0, 1.0)]
    return np.array(xs, dtype=np.float32)


def probe_matrix(anchors):
    """One column of probes per feature, padded to the longest with a point inside the feature's right ray."""
    cols = [probes_of(a) for a in anchors]
    n = max(len(c) for c in cols)
    out = np.zeros((n, len(cols)), dtype=np.float32)
    for k, (c, a) in enumerate(zip(cols, anchors)):
        out[:, k] = np.float32(np.float64(a[-1]) + 0.5) if len(a) > 1 else np.float32(0.5)
        out[:len(c), k] = c
    return out


def value_bounds(ex, anchor, xs, k32):
    """``(f [n, C], bound [n, C])`` at the float32 probes ``xs [n]`` for a table with these anchors (module docstring)."""
    C = ex.C
    bps = anchor[1:]
    P = len(bps)
    piece = np.searchsorted(bps, xs, side="right")                       # #{breakpoints <= x}: the look-up's piece
    f = ex.f_many(xs)
    g32, g64 = gamma(k32, U32), gamma(ex.L * (ex.H + 2) + 4, U64)
    cache = {}
    bound = np.zeros((len(xs), C))
    for n, (x, i) in enumerate(zip(xs, piece)):
        i = int(i)
        if i not in cache:
            a = np.float32(anchor[i])
            nxt = None if i == P else np.float32(bps[i])                  # right anchor (piece 0: the first breakpoint itself)
            if P == 0:
                s = ex.slopes[0]
            elif i == 0:
                s = ex.slopes[ex.interval(frac(down(a)))]
            else:
                s = ex.slopes[ex.interval(frac(a))]
            J = np.zeros(C)
            if nxt is not None:
                lo, hi = bisect.bisect_right(ex.kinks, frac(down(nxt))), bisect.bisect_right(ex.kinks, frac(nxt))
                if hi > lo:
                    J = ex.jumps[lo:hi].sum(axis=0)
            w = 1.0 if (i == 0 or nxt is None) else float(np.float64(nxt) - np.float64(a))
            ulp = 0.0 if nxt is None else float(np.float64(nxt) - np.float64(down(nxt)))
            m_a = ex.mag([a])[0]
            m_n = ex.mag([nxt if (nxt is not None and i > 0) else np.float64(a) + (1.0 if nxt is None else -1.0)])[0]
            cache[i] = (a, np.abs(ex.f(a)), np.abs(s), J, w, ulp, m_a, m_n)
        a, fa, s, J, w, ulp, m_a, m_n = cache[i]
        d = abs(float(np.float64(x) - np.float64(a)))
        far = max(1.0, d / w) if w > 0 else 1.0
        base = fa + s * d
        b = g32 * base + (1.0 + g32) * ulp * J * far + g64 * (m_a + (m_a + m_n) * far) + U64 * np.abs(f[n])
        # float32 underflow: a subnormal val, slope or result is rounded to a multiple of 2^-149
        b = b + np.where((fa > 0) & (fa < 2.0 ** -125), 2.0 ** -150, 0.0) + np.where((s > 0) & (s < 2.0 ** -125), 2.0 ** -150 * d, 0.0) \
            + np.where((base > 0) & (base < 2.0 ** -120), 2.0 ** -150, 0.0)
        bound[n] = b
    return f, bound


def ratios(T, f, bound):
    """``|T - f| / bound`` per element; a zero bound demands ``T == f``: 0 where it holds, inf where not.  Where the exact
    value leaves the float32 range (the +-3e38 probes), an infinity of the right sign is the correct look-up."""
    T = np.asarray(T, dtype=np.float64)
    err = np.abs(T - f)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    over = np.isinf(T) & (np.abs(f) + bound >= F32_MAX) & (np.sign(T) == np.sign(f))
    r = np.where(over, 0.0, r)
    return np.where(np.isnan(r), np.inf, r)


def check_values(ex, anchor, xs, T, k32):
    """Worst ``|T - f| / bound`` over the probes ``xs [n]`` and channels, ``T [n, C]`` the table's float32 results there, and the
    place of the worst element."""
    f, bound = value_bounds(ex, anchor, xs, k32)
    r = ratios(T, f, bound)
    if r.size == 0:
        return 0.0, None
    n, c = np.unravel_index(int(np.argmax(r)), r.shape)
    return float(r[n, c]), dict(x=float(xs[n]), channel=int(c), got=float(np.asarray(T)[n, c]), want=float(f[n, c]),
                                bound=float(bound[n, c]))


# =============================================================================
# network families (CPU float32 StackedMLP; the container is the only thing taken from the package)
# =============================================================================
def stack_of(feats, L, H, C, bias=True, dtype=None):
    """``feats``: per feature ``dict(w1 [H], b1 [H], mids [(W [H, H], b [H])] * (L - 2), wl [C, H], bl [C])`` of arrays."""
    import torch
    from gnan_amd.functional import StackedMLP
    dtype = dtype or torch.float32

    def T(rows):
        return torch.tensor(np.stack(rows), dtype=torch.float64).to(dtype)
    w_mid = b_mid = None
    if L > 2:
        w_mid = torch.stack([T([f["mids"][l][0] for f in feats]) for l in range(L - 2)], 0)
        b_mid = torch.stack([T([f["mids"][l][1] for f in feats]) for l in range(L - 2)], 0) if bias else None
    return StackedMLP(T([f["w1"] for f in feats]), T([f["b1"] for f in feats]) if bias else None, w_mid, b_mid,
                      T([f["wl"] for f in feats]), T([f["bl"] for f in feats]) if bias else None, L, H, len(feats[0]["wl"]), len(feats))


def _out_layer(H, C, used, scale=1.0):
    """Small dyadic last-layer rows over the ``used`` last-hidden units (the others feed nothing), dyadic biases."""
    wl = np.zeros((C, H))
    for c in range(C):
        for j in range(used):
            wl[c, j] = (((7 * j + 3 * c) % 5) - 2) / 4.0 * scale
    return wl, np.array([(c + 1) / 8.0 * scale for c in range(C)])


def ladder(L, H, C, n_kinks, roots2, roots3=(), w=1.0, step=1.0, offset=0.0, scale=1.0):
    """*Ladder*: first-layer units ``m = 0 .. n_kinks - 1`` are ``relu(w x - (step m + offset))`` (kinks at the integers by
    default; ``w = step = 3, offset = 1``: at ``m + 1/3``, the *thirds*), unit ``H - 1`` is ``relu(-w x - offset)`` (the only
    unit alive left of the first kink).  ``roots2``: one second-layer unit per ``(src, c)``: ``relu(h_src - c)`` with ``src`` a
    first-layer unit or ``"neg"`` — its root is where ``h_src = c``: ``(step m + offset + c) / w`` resp. ``-(offset + c) / w``.  ``roots3`` (L = 4): per ``(src, c)`` a second-layer unit
    ``h_src + 1`` (alive everywhere: no kink of its own) and a third-layer unit ``relu(that - 1 - c)``.  Every number is a small dyadic: exact in both
    builders and in float32."""
    assert n_kinks < H and len(roots2) + len(roots3) <= H and (L == 4 or not roots3) and L in (3, 4)
    w1, b1 = np.zeros(H), -np.ones(H)                          # unused units of every layer are constant -1: dead, never zero
    w1[:n_kinks] = w
    b1[:n_kinks] = -(np.arange(n_kinks, dtype=np.float64) * step + offset)
    w1[H - 1], b1[H - 1] = -w, -offset
    unit = lambda src: H - 1 if src == "neg" else int(src)      # noqa: E731
    W2, b2 = np.zeros((H, H)), -np.ones(H)
    for j, (src, c) in enumerate(roots2):
        W2[j, unit(src)] = 1.0
        b2[j] = -c
    mids = [(W2, b2)]
    used = len(roots2)
    if L == 4:
        W3, b3 = np.zeros((H, H)), -np.ones(H)
        for j, (src, c) in enumerate(roots3):
            W2[len(roots2) + j, unit(src)] = 1.0                # h_src + 1 > 0: passed on without a kink or a zero of its own
            b2[len(roots2) + j] = 1.0
            W3[j, len(roots2) + j] = 1.0
            b3[j] = -(c + 1.0)
        # the second-layer units that carry a root of their own reach the output through units of the third layer (+ 1: alive)
        for j in range(len(roots2)):
            if len(roots3) + j < H:
                W3[len(roots3) + j, j] = 1.0
                b3[len(roots3) + j] = 1.0
        mids.append((W3, b3))
        used = min(H, len(roots3) + len(roots2))
    wl, bl = _out_layer(H, C, max(used, 1), scale)
    return dict(w1=w1, b1=b1, mids=mids, wl=wl, bl=bl)


def ladder_edges(L, H, C, P=4):
    """The edge cases of the issue as features of one ladder stack with ``P`` first-layer kinks at ``0 .. P - 1`` (so
    ``t_first = 0``, ``t_last = P - 1``; the added sample nodes of layer 2 are -2, -1, P, P + 1).  Returns ``(names, feats)``."""
    last = P - 1
    e = {
        "node t_last+1": [(0, last + 1.0)],
        "node t_last+2": [(0, last + 2.0)],
        "node t_first-1": [("neg", 1.0)],
        "node t_first-2": [("neg", 2.0)],
        "all four nodes": [(0, last + 1.0), (0, last + 2.0), ("neg", 1.0), ("neg", 2.0)],
        "far out on both rays": [(0, 1000.0), ("neg", 4096.0), (1, 3.0e6)],
        "root on a breakpoint": [(0, 2.0), (1, 1.0)],
        "two units, one root": [(1, 0.5), (1, 0.5), (0, 1.5)],
        "one step from a kink": [(1, 2.0 ** -23), (2, 2.0 ** -22)],
        "halves and quarters": [(0, 0.5), (1, 0.25), (2, 0.75), (last, 0.5), (last, 1.5), ("neg", 0.5), ("neg", 1.5)],
    }
    names, feats = [], []
    for name, r2 in e.items():
        if L == 3:
            names.append(name)
            feats.append(ladder(3, H, C, P, r2))
        else:
            # L = 4: the same roots carried by the third layer — the merged breakpoints are then those of layer 1 (the
            # second-layer units that pass h_src on have no root), so the third layer's added nodes are the same
            # -2, -1, P, P + 1 — and once with a second-layer root beyond both ends, which moves the third layer's nodes out
            names.append(name + " (layer 3)")
            feats.append(ladder(4, H, C, P, [], r2))
            if name.startswith("node") or name.startswith("all four"):
                names.append(name + " (layer 3, merged ends)")
                out2 = [(0, last + 0.5), ("neg", 0.5)]                    # second-layer roots at P - 1/2 and -1/2
                shift = [(s, c + 0.5) for s, c in r2]                      # t_last' = P - 1/2, t_first' = -1/2
                feats.append(ladder(4, H, C, P, out2, shift))
            names.append(name + " (layer 2)")
            feats.append(ladder(4, H, C, P, r2, []))
    return names, feats


def ladder_pass_boundary(L, H, C, P):
    """``P`` first-layer kinks at ``0 .. P - 1`` (``P + 4`` sample nodes) and roots of the last searched layer in the intervals
    around the kernel's pass boundary (node 63 of 64-node passes, node 31 of 32-node passes: kinks ``P - 4 .. P - 1``), on the
    two right nodes and between them."""
    r = [(P - 4, 0.5), (P - 3, 0.5), (P - 2, 0.5), (P - 1, 0.5), (P - 1, 1.0), (P - 1, 1.5), (P - 1, 2.0), (28 if P > 40 else 0, 0.25),
         ("neg", 1.0), ("neg", 0.5), (P - 3, 0.25), (P - 3, 0.75), (P - 2, 0.25), (P - 2, 0.75), (P - 1, 0.25)]
    if P >= 34:
        r += [(29, 0.5), (30, 0.5), (31, 0.5)]                            # around node 31 .. 33 as well
    # L = 4: the second layer's own roots sit in the last two intervals and on the node t_last + 1; the third layer's follow on
    # the merged breakpoints
    return ladder(L, H, C, P, r) if L == 3 else ladder(4, H, C, P, [(P - 2, 0.5), (P - 1, 0.5), (P - 1, 1.0)], r)


def random_state(F, L, H, C, bias, seed, w_scale=1.0, b_scale=0.5):
    """The suite's random shape functions (tests/test_pwl_tables.py:mlp_state) as a stack."""
    from test_pwl_tables import mlp_state, stack
    return stack(mlp_state(F, L, H, C, bias, seed, w_scale, b_scale), F, L, H, C, bias)


def range_family(F, L, H, C, seed):
    """*Range*: random networks whose last layers are scaled by ``2^k``, ``k`` spread over [-40, 10]: small features beside
    large ones."""
    import torch
    p = random_state(F, L, H, C, True, seed)
    ks = np.linspace(-40, 10, F).round().astype(int)
    s = torch.tensor([2.0 ** int(k) for k in ks], dtype=torch.float32)
    return p._replace(w_last=p.w_last * s.view(F, 1, 1), b_last=p.b_last * s.view(F, 1)), ks


def wide_family(L, H, C, seed):
    """*Wide*: kinks at 1e4 and at 1e-30 and a unit whose ``-b / w`` lies beyond 3e38, among random units; one feature."""
    p = random_state(2, L, H, C, True, seed)
    w, b = p.w_first.clone(), p.b_first.clone()
    w[0, 0], b[0, 0] = 1.0, -1.0e4
    w[0, 1], b[0, 1] = 1.0, -1.0e-30
    w[0, 2], b[0, 2] = 1.0e-39, -1.0                       # kink at 1e39: clamped to 3e38
    w[1, 0], b[1, 0] = -1.0e-39, -2.0                      # kink at -2e39
    w[1, 1], b[1, 1] = 2.0, 2.0e4
    return p._replace(w_first=w, b_first=b)


def dead_family(L, H, C, seed):
    """*Dead*: constant units (``w1 = 0``) with ``b > 0`` and ``b < 0``, a dead second layer (``W2 = 0``, ``b2 < 0``) and an
    all-zero feature, among random ones; three features."""
    p = random_state(3, L, H, C, True, seed)
    w, b = p.w_first.clone(), p.b_first.clone()
    w[0, ::2] = 0.0
    b[0, 0], b[0, 2] = 0.75, -0.75
    out = p._replace(w_first=w, b_first=b)
    if L >= 3:
        wm, bm = p.w_mid.clone(), p.b_mid.clone()
        wm[0, 1] = 0.0
        bm[0, 1] = -0.25
        wm[:, 2] = 0.0
        bm[:, 2] = 0.0
        out = out._replace(w_mid=wm, b_mid=bm)
    w, b = out.w_first.clone(), out.b_first.clone()
    w[2], b[2] = 0.0, 0.0
    return out._replace(w_first=w, b_first=b, w_last=_zero_row(p.w_last, 2), b_last=_zero_row(p.b_last, 2))


def _zero_row(t, k):
    t = t.clone()
    t[k] = 0.0
    return t


# =============================================================================
# the whole check of one stack's tables
# =============================================================================
def cpu_tables(t):
    import torch
    return type(t)(*[q.cpu() if torch.is_tensor(q) else q for q in t])


def check_tables(p, t, evaluate, k32, exs=None, direct=None):
    """Hold the tables ``t`` (CPU) of the stack ``p`` (CPU) to the anchor, no-kink and value assertions.  ``evaluate(x [n, F]
    float32 tensor) -> [n, F * C]`` evaluates the tables.  Returns a report ``dict(anchors=[...], kinks=[...], worst=ratio,
    where=..., per_feature=[ratio ...], point_pieces=count)``; the caller asserts on it."""
    import torch
    exs = exs or features_of(p)
    direct = (p.H <= 33) if direct is None else direct
    tabs = [feature_table(t, k) for k in range(p.F)]
    x = probe_matrix([a for a, _, _ in tabs])
    T = evaluate(torch.from_numpy(x)).detach().cpu().numpy().reshape(x.shape[0], p.F, -1)
    rep = dict(anchors=[], kinks=[], worst=0.0, where=None, per_feature=[], point_pieces=0)
    fs, bounds = [], []
    for k, (ex, (a, _, _)) in enumerate(zip(exs, tabs)):
        rep["anchors"] += [f"feature {k}: {m}" for m in check_anchors(ex, a)]
        rep["kinks"] += [f"feature {k}: {m}" for m in check_no_kink_inside(ex, a, direct)]
        rep["point_pieces"] += len(ex.expected_anchors()[1])
        f, bound = value_bounds(ex, a, x[:, k], k32)
        fs.append(f)
        bounds.append(bound)
        r = ratios(T[:, k], f, bound)
        n, c = np.unravel_index(int(np.argmax(r)), r.shape)
        rep["per_feature"].append(float(r[n, c]))
        if r[n, c] >= rep["worst"]:
            rep["worst"] = float(r[n, c])
            rep["where"] = dict(feature=k, x=float(x[n, k]), channel=int(c), got=float(T[n, k, c]), want=float(f[n, c]),
                                bound=float(bound[n, c]))
    rep["f"], rep["bound"] = np.stack(fs, 1), np.stack(bounds, 1)                  # [n, F, C]
    return rep, x, exs


def check_sum(rep, Tsum):
    """The look-up summed over the features, ``Tsum [n, C]`` float32, against the sum of the per-feature truths: the
    per-feature bounds add up, and the F - 1 float32 additions (counted as F) each round a partial sum that is at most
    ``sum_k (|f_k| + bound_k)``.  Where that sum of magnitudes leaves the float32 range (the +-3e38 probes: partial sums may
    overflow, infinities of both signs may meet) nothing is asked of the sum — each term was held on its own.  Returns the
    worst ratio."""
    f, b = rep["f"], rep["bound"]
    F = f.shape[1]
    total = np.abs(f).sum(1) + b.sum(1)
    bound = b.sum(1) + gamma(F, U32) * total + F * U64 * total
    r = ratios(Tsum, f.sum(1), bound)
    return float(np.where(total >= F32_MAX / 2, 0.0, r).max())
