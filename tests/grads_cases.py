"""The case matrix of the table path's parameter gradients (tests/test_grads_bound.py runs the emulations on it, on the CPU;
tests/test_gpu_grad_elements.py the kernels): name -> builder of a :class:`grads_ref.Case`.  Moments are handed in directly — no
nodes —, the tables record's ``max_pieces`` picks the kernel (1025 sends an L = 3, C <= 4 case to ``fpwl_grad3_kernel<4, 1>``
instead of the sweep).  Sizes are the smallest that reach each edge; the reference's cost (live pieces x H^2) sets them."""
import numpy as np

import grads_ref as G
import tables_ref as R

CASES = {}
_BUILT = {}


def case(name, tables=None):
    """The built case (cached; ``tables``: another table builder for the families that take one — not cached)."""
    if tables is not None:
        return CASES[name](tables)
    if name not in _BUILT:
        _BUILT[name] = CASES[name](None)
    return _BUILT[name]


def _random(name, F, L, H, C, seed, n_live, **kw):
    CASES[name] = lambda tables, kw=kw: G.random_case(name, F, L, H, C, seed, n_live, tables=tables, **kw)


# ---- routes and channel / quarter instances ------------------------------------------------------------------------------------
for H, C in ((1, 1), (5, 4), (33, 5), (127, 64), (128, 1)):
    _random(f"L2-H{H}-C{C}", 2, 2, H, C, 100 + H + C, 5)
for H, C in ((1, 1), (2, 3), (3, 4), (5, 1), (33, 3), (63, 4), (64, 1)):
    _random(f"L3-sweep-H{H}-C{C}", 2, 3, H, C, 200 + H + C, 6)
for H, C in ((5, 1), (33, 4)):
    _random(f"L3-piece4-H{H}-C{C}", 2, 3, H, C, 300 + H + C, 6, max_pieces=1025)
for H, C in ((64, 5), (8, 8), (3, 9), (8, 16), (33, 17), (8, 64)):
    _random(f"L3-piece2-H{H}-C{C}", 2, 3, H, C, 400 + H + C, 6)
for H, C in ((3, 1), (33, 4), (64, 5), (8, 8), (8, 9), (3, 16), (8, 17), (8, 64)):
    _random(f"L4-H{H}-C{C}", 2, 4, H, C, 500 + H + C, 6)
_random("L2-wrapper-C65", 2, 2, 8, 65, 601, 4)
_random("L3-wrapper-C65", 2, 3, 8, 65, 602, 4)
_random("L4-wrapper-C130", 2, 4, 5, 130, 603, 4)
_random("L3-F1-rho", 1, 3, 8, 1, 611, 6)
_random("L3-F3-one-feature-empty", 3, 3, 8, 2, 612, 4, live=[4, 0, 4])
_random("L4-F3-one-feature-empty", 3, 4, 8, 2, 613, 4, live=[4, 0, 4])
_random("L2-F3-one-feature-empty", 3, 2, 8, 2, 614, 4, live=[0, 4, 4])
_random("L3-no-bias", 2, 3, 8, 2, 615, 5, bias=False)
_random("L4-no-bias", 2, 4, 8, 5, 616, 5, bias=False)
_random("L2-no-bias", 2, 2, 8, 5, 617, 5, bias=False)
_random("L3-mid-bias-only", 2, 3, 8, 2, 618, 5, tweak=lambda p: p._replace(b_first=None, b_last=None))
_random("L4-mid-bias-only", 2, 4, 8, 2, 619, 5, tweak=lambda p: p._replace(b_first=None, b_last=None))
# round tails: nl = 0 .. 5 on the grouped kernels
_random("L3-piece2-tails", 6, 3, 5, 5, 621, 0, live=[0, 1, 2, 3, 4, 5])
_random("L3-piece4-tails", 6, 3, 5, 1, 622, 0, live=[0, 1, 2, 3, 4, 5], max_pieces=1025)
_random("L4-tails", 6, 4, 5, 1, 623, 0, live=[0, 1, 2, 3, 4, 5])
_random("L3-sweep-tails", 6, 3, 5, 1, 624, 0, live=[0, 1, 2, 3, 4, 5])
# float moments on three shapes
_random("L2-float-moments", 2, 2, 8, 5, 631, 5, fixed=False)
_random("L3-sweep-float-moments", 2, 3, 8, 2, 632, 5, fixed=False)
_random("L4-float-moments", 2, 4, 8, 2, 633, 5, fixed=False)
# magnitude families
_random("L3-range", 6, 3, 8, 1, 641, 4, family="range")
_random("L3-range-piece", 6, 3, 8, 5, 642, 4, family="range")
_random("L4-range", 6, 4, 8, 2, 643, 4, family="range")
_random("L2-range", 6, 2, 8, 2, 644, 4, family="range")
_random("L3-thirds", 1, 3, 8, 2, 645, 6, family="thirds")
_random("L3-thirds-piece", 1, 3, 8, 5, 646, 6, family="thirds")
_random("L4-thirds", 1, 4, 8, 2, 647, 6, family="thirds")
_random("L3-dead", 3, 3, 8, 2, 651, 5, family="dead")
_random("L3-dead-piece", 3, 3, 8, 2, 651, 5, family="dead", max_pieces=1025)
_random("L4-dead", 3, 4, 8, 2, 652, 5, family="dead")
_random("L2-dead", 3, 2, 8, 2, 653, 5, family="dead")


# ---- hand-made tables: switch nets and ladders -----------------------------------------------------------------------------------
def _pad(ex, target, start=100.0, step=0.25):
    """Superfluous anchors beyond the kinks that bring the table to exactly ``target`` pieces."""
    have = len(G.table_anchors(ex))
    assert have <= target, (have, target)
    return [start + step * i for i in range(target - have)]


def _small_net(L, H, C, seed):
    """Small dyadic network: the L = 3 switch net, for L = 4 with a second dyadic mid layer, for L = 2 without."""
    rng = np.random.default_rng(seed)
    kinks = [((1.0 if i % 2 == 0 else -1.0), float(i) + 0.125) for i in range(H)]
    f = G.switch_net(H, C, kinks, rng)
    if L == 2:
        f["mids"] = []
    if L == 4:
        f["mids"].append((G._dy(rng, (H, H)), G._dy(rng, H, 16)))
    return f


def _edges(name, L, C, target, live, max_pieces=None, H=4):
    def build(tables):
        f = _small_net(L, H, C, 700 + target + C + L)
        p = R.stack_of([f], L, H, C)
        ex = R.features_of(p)[0]
        return G.hand_case(name, [f], L, H, C, [_pad(ex, target)], [live], np.random.default_rng(target), max_pieces=max_pieces)
    CASES[name] = build


for L, C in ((2, 2), (3, 1), (3, 5), (4, 1)):
    _edges(f"edges-P257-L{L}-C{C}", L, C, 257, [0, 255, 256])
    _edges(f"edges-P513-L{L}-C{C}", L, C, 513, [0, 255, 256, 511, 512])
_edges("edges-P1024-sweep", 3, 2, 1024, [0, 255, 256, 511, 512, 1023])
_edges("edges-P1025-piece4", 3, 2, 1025, [0, 511, 512, 1023, 1024], max_pieces=1025)
_edges("edges-P1025-piece2", 3, 5, 1025, [0, 1023, 1024])
_edges("edges-P1025-L2", 2, 2, 1025, [0, 1023, 1024])
_edges("edges-P1025-L4", 4, 2, 1025, [0, 1023, 1024])
for n in (127, 128, 129):
    _edges(f"sweep-nl{n}", 3, 2, 257, list(range(60, 60 + n)), H=4)

GRID = [0.25 * i for i in range(140)]


def _switches(name, max_pieces=None, C=2):
    """Twelve first-layer units: a switch before live piece 0 (0), at live piece 128 (1), behind the last live piece (2: on
    everywhere, 3: off everywhere), four at one piece (4 .. 7), w1 = 0 with b1 > 0 (8), with b1 = 0 and b1 < 0 (9, 10), and a
    dominant unit (|W2 w1| 2^20 times the rest) that switches off mid-table (11).  140 live pieces on a quarter grid."""
    def build(tables):
        rng = np.random.default_rng(811)
        kinks = [(1.0, -5.125), (1.0, 31.875), (-1.0, 1000.125), (1.0, 1000.375), (2.0, 10.125), (-1.0, 10.125), (0.5, 10.125),
                 (-4.0, 10.125), (0.0, 0.0), (0.0, 0.0), (0.0, 0.0), (-1.0, 20.125)]
        f = G.switch_net(12, C, kinks, rng, dominant=11, const_on=(8,), const_off=(9, 10))
        grid = set(np.float32(GRID).tolist())

        def live(A):
            return [t for t in range(1, len(A)) if float(A[t]) in grid]
        return G.hand_case(name, [f], 3, 12, C, [GRID], [live], rng, max_pieces=max_pieces)
    CASES[name] = build


_switches("switches-sweep")
_switches("switches-piece4", max_pieces=1025)


def _moment_case(name, L, C, edit, max_pieces=None, exps=(30, 36)):
    def build(tables):
        f = _small_net(L, 4, C, 900 + L + C)
        return G.hand_case(name, [f], L, 4, C, [[50.0 + i for i in range(6)]], [lambda A: list(range(0, len(A), 2))],
                           np.random.default_rng(901), max_pieces=max_pieces, exps=exps, moments=edit)
    CASES[name] = build


def _m0_zero(k, A, M):
    """One live piece with M0 = 0 and M1 != 0 (bins of +g, -g), one with M1 = 0."""
    lv = [t for t in range(len(M)) if M[t].any() and t not in G.point_pieces(A)]
    M[lv[1], 0] = 0
    M[lv[2], 1] = 0
    return M


def _last_channel(k, A, M):
    M[:, :, :-1] = 0
    return M


def _huge(k, A, M):
    lv = [t for t in range(len(M)) if M[t].any() and t not in G.point_pieces(A)]
    M[lv[0], 0, 0] = (1 << 62) - 12345
    M[lv[1], 1, -1] = -(1 << 62) + 7
    M[lv[2]] = 0
    M[lv[2], 0, 0] = 1
    return M


for L, C, mp, tag in ((2, 2, None, "L2"), (3, 2, None, "sweep"), (3, 2, 1025, "piece4"), (3, 5, None, "piece2"), (4, 2, None, "L4")):
    _moment_case(f"m0-zero-{tag}", L, C, _m0_zero, mp)
    _moment_case(f"last-channel-{tag}", L, max(C, 3), _last_channel, mp)
    _moment_case(f"huge-and-one-{tag}", L, C, _huge, mp)


# ---- the integer family: exact on every route -------------------------------------------------------------------------------------
def _integer_net(L, H, C, seed):
    """Weights in {-2 .. 2}, first-layer kinks at the half integers, biases integers or halves."""
    rng = np.random.default_rng(seed)
    w1 = np.array([1.0 if i % 2 == 0 else -1.0 for i in range(H)])
    b1 = -w1 * (np.arange(H) + 0.5)
    mids = []
    for _ in range(L - 2):
        W = rng.integers(-2, 3, size=(H, H)).astype(np.float64)
        mids.append((W, rng.integers(-3, 4, size=H).astype(np.float64) / 2))
    return dict(w1=w1, b1=b1, mids=mids, wl=rng.integers(-2, 3, size=(C, H)).astype(np.float64),
                bl=rng.integers(-2, 3, size=C).astype(np.float64))


SEEDS = {(4, 2): 950}          # (a seed whose network is alive right of the kinks: the cancelled slope moment reaches the result)


def _integer_case(name, L, C, e, max_pieces=None):
    """Integer moments; a slope moment of 2^30 + 1 cancelled by -2^30 in the piece next to it, which a superfluous anchor splits off
    (same masks, same slope: the sum is 1).  ``e``: both scales are ``2^e``."""
    def build(tables):
        f = _integer_net(L, 4, C, SEEDS.get((L, C), 950 + L + C))
        extra = [20.0 + i for i in range(8)]                       # integer anchors right of every first-layer kink

        def live(A):
            return [t for t in range(1, len(A)) if float(A[t]) in (20.0, 21.0, 23.0, 25.0)]

        def edit(k, A, M):
            rng = np.random.default_rng(951)
            lv = [t for t in range(len(M)) if M[t].any()]
            for t in lv:
                M[t] = rng.integers(-4, 5, size=M[t].shape)
                M[t, 0, 0] = 1
            M[lv[0], 1, 0] = (1 << 30) + 1
            M[lv[1], 1, 0] = -(1 << 30)
            return M
        return G.hand_case(name, [f], L, 4, C, [extra], [live], np.random.default_rng(952), exps=(e, e), moments=edit,
                           max_pieces=max_pieces, exact=True)
    CASES[name] = build


for L, C, mp, tag in ((2, 2, None, "L2"), (3, 2, None, "sweep"), (3, 2, 1025, "piece4"), (3, 5, None, "piece2"), (4, 2, None, "L4")):
    for e in (0, 100, -100):
        _integer_case(f"integer-{tag}-e{e}", L, C, e, mp)


# ---- point pieces: an exact zero of a layer-2 (layer-3) unit on an anchor, the piece to its right live as well ---------------
def _ladder_case(name, L, max_pieces=None, C=2):
    def build(tables):
        roots = [(0, 2.0), (1, 1.0), (1, 0.5)]
        f = R.ladder(L, 8, C, 4, roots) if L == 3 else R.ladder(4, 8, C, 4, [(0, 1.0)], roots)
        return G.hand_case(name, [f], L, 8, C, None, [lambda A: list(range(len(A)))], np.random.default_rng(971),
                           max_pieces=max_pieces)
    CASES[name] = build


_ladder_case("point-sweep", 3)
_ladder_case("point-piece4", 3, max_pieces=1025)
_ladder_case("point-piece2", 3, C=5)
_ladder_case("point-L4", 4)


# ---- a wrong gradient confined to a small feature: last layers of 2^-40 beside 1 ---------------------------------------------------
def _small_feature(name, L, max_pieces=None):
    def build(tables):
        fs = [_small_net(L, 4, 2, 980 + k) for k in range(3)]
        fs[1]["wl"] = fs[1]["wl"] * 2.0 ** -40
        fs[1]["bl"] = fs[1]["bl"] * 2.0 ** -40
        return G.hand_case(name, fs, L, 4, 2, None, [lambda A: list(range(0, len(A), 2))] * 3, np.random.default_rng(981),
                           max_pieces=max_pieces)
    CASES[name] = build


_small_feature("small-feature-sweep", 3)
_small_feature("small-feature-L4", 4)
_small_feature("small-feature-L2", 2)

ALL = list(CASES)
