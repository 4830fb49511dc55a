"""Float64 reference of the DIRECT shape-function kernels and the bound every element of their results is held to — TEST
INFRASTRUCTURE ONLY (numpy float64 and Python / numpy integers; no GPU, no product code).

The kernels: ``fmlp_lane_kernel``, ``fmlp_point_kernel``, ``fmlp_mfma_kernel`` (csrc/fmlp.hip), ``fmlp_mc_fwd_kernel`` /
``fmlp_mc_bwd_kernel`` (csrc/fmlp_mc.hip), ``fmlp_bwd_kernel`` (csrc/fmlp_bwd.hip, body ``gnan_bwd::feature_grads`` in
csrc/fmlp_bwd_body.hpp) and ``fmlp_bwd_mfma_kernel`` (csrc/fmlp_bwd_mfma.hip).

**Contract.**  ``x [n, F]``, the six stacked tensors as ``functional.StackedMLP`` holds them (:class:`Net`: the same fields as
float64 numpy), ``sum_features``, and optionally Dropout as a keep-mask ``[n, F, L - 1, H]`` (an INPUT: ``functional.dropout_masks``
writes it, ``test_every_units_keep_bit_is_gnan_dropout_masks`` owns it) with ``p``.  Feature ``k``::

    h_0 = x[:, k];   z_l = b_l + W_l h_(l-1);   h_l = keep_l relu(z_l) / (1 - p)   (l < L);   f_k = z_L

and ``out = f_k`` side by side, or ``sum_k f_k``.  ``p`` is the float32 the record carries, ``1 / (1 - p)`` taken in float64.

**Forward bound**, per element, layer by layer (:func:`forward`), ``u = 2^-24``, ``gamma32(k) = k u / (1 - k u)``::

    mag_l = |b_l| + |W_l| (|h_(l-1)| + E_(l-1))          E_l = |W_l| E_(l-1) + gamma32(k_l) mag_l,   E_0 = 0

ReLU is 1-Lipschitz: ``E`` passes through it, whatever the sign.  Dropout: ``E <- keep s (E + gamma32(3) (|h| + E))`` — the kernels
form ``drop_scale = 1.f / (1.f - p)`` in float32 (two roundings: the difference, the quotient; make_params, csrc/fmlp.hip:515) and
multiply (one).  Side by side the output's bound is ``E_L``.  With ``sum_features``: ``sum_k E_k + gamma32(adds) sum_k (A_k + E_k)``
with ``A_k = |f_k|`` where a feature's value is finished before it is added (lane kernel) and ``A_k = mag_L`` of the feature where
the features' partial sums are added first (matrix cores: every product then passes the chain's and the adds' roundings).  No
kernel rounds at the store (the values are float32 already), so no ``u |t|`` is added in the forward.

``k_l`` per route (:func:`fwd_counts`), from the code:

    lane   (fmlp_lane_kernel)      layer 1: 1, fmaf(xv, w, b) (fmlp.hip:114; L == 1: :106)
                                   further layers: n_in = H fmas onto the bias (dense_layer, :63-70)
                                   sum: sacc += v, F - 1 adds behind the exact 0 + v (:98)
    point  (fmlp_point_kernel)     layer 1: 1 (:150); layer 2: the H-long fma chain onto the bias (:155-164)
                                   last: one product, six butterfly adds, the bias add = 8 (:169-172); sum only at F == 1: no add
    mfma   (fmlp_mfma_kernel)      layer 1: 1 (:317); a mid layer: the f32 MFMA is an fma chain over K with one rounding per step,
                                   K = the padded 32 HT units onto the bias (:335-344)
                                   last: 16 HT lane fmas from 0 (:358-372), the cross-half add, the bias add = 16 HT + 2 (:380)
                                   sum: partials over the chunk's features (feat_chunk - 1 adds, :375), cross-half add, the summed
                                   bias (:403; itself feat_chunk - 1 adds, :388), then fmlp_chunk_sum_kernel's chunks - 1 adds (:421):
                                   adds = (feat_chunk - 1) + 2 + (chunks - 1) on top of the chain's 16 HT
    mc     (fmlp_mc_fwd_kernel)    layer 1 and mid layers as mfma (fmlp_mc.hip:199, :216-225)
                                   last: a third matrix product over the 32 HT units from 0, then the bias add = 32 HT + 1 (:244-264)
                                   sum: the accumulators CARRY OVER the chunk's features (:236): the earliest product passes
                                   feat_chunk 32 HT chain steps, then the summed bias (:294) and chunks - 1 adds (:308):
                                   chain 32 HT, adds = (feat_chunk - 1) 32 HT + 1 + chunks - 1

Padded units enter the chains as exact zeros; they are counted all the same (the larger count).  ``feature_chunks`` /
``feat_chunk`` are restated in :func:`feature_chunks` (fmlp.hip:440-446, :493-495; fmlp_mc.hip:318-325, :817-819);
tests/test_mlp_bound.py holds them equal to what ``gnan_fmlp_fwd_workspace_bytes`` / ``gnan_fmlp_mc_fwd_workspace_bytes`` report.

**Backward truth** (:func:`backward`): ``d{w_first, b_first, w_mid, b_mid, w_last, b_last}`` for an upstream ``g``, by the reverse
pass at the head of csrc/fmlp_bwd.hip, L = 2 and L = 3, masks ``[z > 0]`` strict (fmlp_bwd_body.hpp:105, :110, :119, :128), the
Dropout factors on both passes.

**Backward bound** per element::

    |got - t| <= u32 |t| + gamma32(k) Mag

``Mag`` is the same reverse pass with every weight, bias, input and upstream gradient replaced by its magnitude (the masks stay:
they are decided, below), summed over the nodes.  With the masks fixed the pass is a straight-line program of sums and products;
``k`` counts the roundings on the longest path of one term (:func:`bwd_counts`), ``u32 |t|`` is kept on top as the issue states it:

    d_h1   = 1 (+ 3 under Dropout)                    the recomputed first layer (fmlp_bwd_body.hpp:104)
    d_h2   = d_h1 + HP (+ 3)                          z2's chain onto b2: HP = kH = 64 in the lane body, which unrolls all 64
                                                      lanes (:109), 32 HT on the matrix cores (fmlp_bwd_mfma.hip:169-179)
    d_dz2  = CH (+ 3)                                 the chain of dh2 over the channels: CH = C in the lane body (:114-115),
                                                      CT (C padded to 1, 2, 4, 8) in fmlp_bwd_mfma (:228-232), 32 CT32 as an MFMA
                                                      in fmlp_mc_bwd (fmlp_mc.hip:588-599);  L == 2: this is d_dz1
    d_dz1  = d_dz2 + HP (+ 3)                         dh1 = W2^T dz2 (:124-127; fmlp_bwd_mfma.hip:284-293)
    acc    lane:  ceil(nodes_per_split / 4) fmas of the nodes a wave owns (:92), the four waves' adds (3), the splits' adds
                  in fmlp_split_reduce_kernel (splits - 1)
           mfma, mc:  dW2 / dW3 are MFMA chains with K = node, 32 steps per tile, ceil(nodes_per_split / 128) tiles per wave;
                  the lane sums take one add per tile and a five-step butterfly (fmlp_bwd_mfma.hip:299-320), fmlp_mc_bwd's
                  d_b_mid / d_b_last twelve roundings per tile (fmlp_mc.hip:564, :632) — all below 32 per tile, so ONE count is
                  taken for all six tensors (the larger): 32 tiles + 5, the waves' 3, splits - 1
    k      w_last: d_h(last hidden) + acc;  b_last: acc;  w_mid: d_dz2 + d_h1 + acc;  b_mid: d_dz2 + acc;
           w_first, b_first: d_dz1 + acc

``node_splits`` and ``nodes_per_split`` are restated in :func:`node_splits` (fmlp_bwd.hip:68-76, :138; fmlp_bwd_mfma.hip:367-373,
:436-444; fmlp_mc.hip:736-742, :879-888); tests/test_mlp_bound.py holds the split counts equal to what the three
``*_bwd*_workspace_bytes`` report.  A zero bound demands an exact zero, forward and backward; no element is left out.

**Decided masks** (a condition on the CASE, not a tolerance): parameter gradients jump when a hidden pre-activation changes sign.
:func:`forward` counts as *undecided* every kept hidden unit of a layer >= 2 whose float64 ``|z|`` does not exceed its ``E``; for
the backward cases ``E`` is taken with the largest mid-layer count of any route (64, :data:`DECIDE`).  The first layer is one
fma: its sign is exact.  An exact zero of the exact family is decided by construction (every order gives the zero).  Committed
backward cases have no undecided unit (tests/test_mlp_bound.py).

**Exact family** (:func:`exact`): weights, biases, ``x`` and ``g`` dyadic with few bits, Dropout scale 2.  The passes run in
int64 on the scaled integers; ``assert`` on the MAGNITUDES (all masks on): every forward value below ``2^24`` quanta of its own
quantum, every gradient sum likewise.  Every product and partial sum of the float32 evaluation is then exact in any order, and
outputs and gradients must equal the reference bit for bit.

**Emulations** in numpy float32: :func:`emulate_lane` (the lane kernel's forward in its own order) and :func:`emulate_bwd`
(``feature_grads``' order for one feature, splits included), with ``plant=`` for deliberate errors.  numpy has no fma: a
multiply-add rounds twice, so they are held to ``2 k`` (``scale=2`` of :func:`forward` / :func:`backward`).
"""
from typing import NamedTuple, Optional

import numpy as np

U = 2.0 ** -24
NAMES = ("w_first", "b_first", "w_mid", "b_mid", "w_last", "b_last")
DROP_K = 3
FWD_ROUTES = ("lane", "point", "mfma", "mc")
BWD_ROUTES = ("lane", "mfma", "mc")


def gamma(k):
    k = np.asarray(k, dtype=np.float64)
    return k * U / (1.0 - k * U)


class Net(NamedTuple):
    """``functional.StackedMLP``'s fields as float64 numpy (None where absent)."""
    w_first: Optional[np.ndarray]   # [F, H]
    b_first: Optional[np.ndarray]   # [F, H]
    w_mid: Optional[np.ndarray]     # [L-2, F, H, H]
    b_mid: Optional[np.ndarray]     # [L-2, F, H]
    w_last: np.ndarray              # [F, C, H]  ([F, C] when L == 1)
    b_last: Optional[np.ndarray]    # [F, C]
    L: int
    H: int
    C: int
    F: int


def net_of(p) -> Net:
    """A StackedMLP of torch tensors (or anything with its fields) as a :class:`Net`."""
    def a(t):
        if t is None:
            return None
        t = t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)
        return np.ascontiguousarray(t, dtype=np.float64)
    return Net(*[a(t) for t in p[:6]], *[int(v) for v in p[6:10]])


def scale_of(p: float) -> float:
    """``1 / (1 - p)`` in float64 for the float32 ``p`` the record carries."""
    return 1.0 / (1.0 - float(np.float32(p)))


# ---------------------------------------------------------------------------------------------------------------------------
# the project's launch arithmetic, restated
# ---------------------------------------------------------------------------------------------------------------------------
def ht_of(H: int) -> int:
    return 1 if H <= 32 else 2


def feature_chunks(n: int, F: int, H: int, mc: bool):
    """``(real_chunks, feat_chunk, chunks asked)`` of run_mfma (csrc/fmlp.hip:440-446, :491-495) and fmlp_mc_fwd
    (csrc/fmlp_mc.hip:318-325, :816-819): 256 nodes per workgroup, 128 in the mc kernel at H > 32."""
    per_block = 256 if (not mc or H <= 32) else 128
    node_blocks = -(-n // per_block)
    chunks = -(-1024 // node_blocks)
    chunks = max(1, min(chunks, (F + 1) // 2))
    fc = -(-F // chunks)
    fc += fc & 1
    return -(-F // fc), fc, chunks


def node_splits(n: int, F: int, route: str):
    """``(splits, nodes_per_split)`` of gnan_fmlp_bwd (csrc/fmlp_bwd.hip:68-76, :128, :138) and of gnan_fmlp_bwd_mfma /
    gnan_fmlp_mc_bwd (csrc/fmlp_bwd_mfma.hip:367-373, :436-444; csrc/fmlp_mc.hip:736-742, :879-888)."""
    unit, grain = (32, 4) if route == "lane" else (128, 128)
    want = min(-(-512 // F), -(-n // unit), 1024)
    splits = max(want, 1)
    if splits == 1:
        return 1, (n if route == "lane" else max(-(-n // 128) * 128, 128))
    return splits, -(-(-(-n // splits)) // grain) * grain


def mc_channel_tiles(H: int, C: int, drop: bool) -> int:
    """bwd_channel_tiles of csrc/fmlp_mc.hip:396."""
    return 2 if (C > 32 or (H > 32 and drop)) else 1


def fwd_covers(route: str, n: int, F: int, L: int, H: int, C: int, sum_features: bool, drop: bool) -> bool:
    """The documented cover of a forward route: lane anything; point under AUTO at n F <= 64 (point_route, csrc/fmlp.hip:524-527);
    mfma_shape (:431-437); fwd_cover (csrc/fmlp_mc.hip:315)."""
    if route == "lane":
        return True
    if route == "point":
        return n * F <= 64 and L in (2, 3) and 1 <= H <= 64 and not drop and (not sum_features or F == 1)
    return 3 <= L <= 4 and 1 <= H <= 64 and C <= (8 if route == "mfma" else 64)


def bwd_covers(route: str, L: int, H: int, C: int) -> bool:
    """csrc/fmlp_bwd.hip:99, csrc/fmlp_bwd_mfma.hip:410, csrc/fmlp_mc.hip:732."""
    if route == "lane":
        return L in (2, 3) and 1 <= H <= 64 and 1 <= C <= 8
    return L == 3 and 1 <= H <= 64 and 1 <= C <= (8 if route == "mfma" else 64)


# ---------------------------------------------------------------------------------------------------------------------------
# counts
# ---------------------------------------------------------------------------------------------------------------------------
class FwdCounts(NamedTuple):
    first: int
    mid: int
    last: int
    adds: int
    interleaved: bool     # the features' partial sums are added before a feature's value is finished (A_k = mag, not |f_k|)


DECIDE = FwdCounts(1, 64, 64, 0, False)      # the largest mid-layer count of any route: decides the backward cases' masks


def fwd_counts(route: str, n: int, F: int, L: int, H: int, C: int, sum_features: bool) -> FwdCounts:
    """``k_l`` of the header for a forward route."""
    hp = 32 * ht_of(H)
    if route == "lane":
        return FwdCounts(1, H, H if L >= 2 else 1, F - 1 if sum_features else 0, False)
    if route == "point":
        return FwdCounts(1, H, 8, 0, False)
    chunks, fc, _ = feature_chunks(n, F, H, route == "mc")
    fc = min(fc, F)
    if route == "mfma":
        return FwdCounts(1, hp, hp // 2 + 2 if not sum_features else hp // 2, fc + chunks if sum_features else 0, True)
    if route == "mc":
        return FwdCounts(1, hp, hp + 1 if not sum_features else hp, (fc - 1) * hp + 1 + chunks - 1 if sum_features else 0, True)
    raise ValueError(route)


def bwd_counts(route: str, n: int, F: int, L: int, H: int, C: int, drop: bool) -> dict:
    """``k`` of the header per gradient tensor for a backward route."""
    dk = DROP_K if drop else 0
    splits, nps = node_splits(n, F, route)
    if route == "lane":
        hp, ch = 64, C
        acc = -(-nps // 4) + 3 + splits - 1
    else:
        hp = 32 * ht_of(H)
        ch = (1 if C <= 1 else 2 if C <= 2 else 4 if C <= 4 else 8) if route == "mfma" else 32 * mc_channel_tiles(H, C, drop)
        acc = 32 * -(-nps // 128) + 5 + 3 + splits - 1
    d_h1 = 1 + dk
    if L == 2:
        d_dz1 = ch + dk
        return {"w_first": d_dz1 + acc, "b_first": d_dz1 + acc, "w_last": d_h1 + acc, "b_last": acc}
    d_h2 = d_h1 + hp + dk
    d_dz2 = ch + dk
    d_dz1 = d_dz2 + hp + dk
    return {"w_first": d_dz1 + acc, "b_first": d_dz1 + acc, "w_mid": d_dz2 + d_h1 + acc, "b_mid": d_dz2 + acc,
            "w_last": d_h2 + acc, "b_last": acc}


# ---------------------------------------------------------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------------------------------------------------------
def _z(v):
    return 0.0 if v is None else v


def _factors(keep, p, n, F, n_hidden, H):
    """Dropout factors ``[F, n_hidden, n, H]`` (0 or 1 / (1 - p)); ones without Dropout."""
    if keep is None or not p:
        return np.ones((F, n_hidden, n, H)), False
    k = np.asarray(keep.detach().cpu().numpy() if hasattr(keep, "detach") else keep)
    assert k.shape == (n, F, n_hidden, H), (k.shape, (n, F, n_hidden, H))
    return np.transpose(k.astype(np.float64), (1, 2, 0, 3)) * scale_of(p), True


class Forward(NamedTuple):
    truth: np.ndarray        # [n, F C] or [n, C]
    bound: np.ndarray
    undecided: int           # kept hidden units of layers >= 2 with |z| <= E
    judged: int
    per_feature: np.ndarray  # [F, n, C] truth of every feature


def forward(net: Net, x, sum_features: bool, counts: FwdCounts, keep=None, p: float = 0.0, scale: int = 1) -> Forward:
    """Truth and bound of the header for the counts of one route (``scale``: 2 for the fma-less emulations)."""
    x = np.asarray(x, dtype=np.float64)
    n, F = x.shape
    L, H, C = net.L, net.H, net.C
    assert F == net.F
    g = lambda k: gamma(scale * k)   # noqa: E731
    xk = x.T[:, :, None]                                              # [F, n, 1]
    if L == 1:
        w = net.w_last[:, None, :]                                    # [F, 1, C]
        f = xk * w + _z(None if net.b_last is None else net.b_last[:, None, :])
        mag = np.abs(xk) * np.abs(w) + _z(None if net.b_last is None else np.abs(net.b_last)[:, None, :])
        E = g(counts.last) * mag
        undecided = judged = 0
    else:
        fac, drop = _factors(keep, p, n, F, L - 1, H)
        z = xk * net.w_first[:, None, :] + _z(None if net.b_first is None else net.b_first[:, None, :])
        mag = np.abs(xk) * np.abs(net.w_first)[:, None, :] + _z(None if net.b_first is None else np.abs(net.b_first)[:, None, :])
        E = g(counts.first) * mag
        undecided = judged = 0

        def behind(z, E, l):
            h = np.maximum(z, 0.0)
            if drop:
                s = fac[:, l]
                E = s * (E + g(DROP_K) * (h + E))
                h = h * s
            return h, E
        h, E = behind(z, E, 0)
        for l in range(L - 2):
            W = net.w_mid[l]                                          # [F, H, H]
            b = None if net.b_mid is None else net.b_mid[l][:, None, :]
            z = np.einsum("fnj,fij->fni", h, W) + _z(b)
            mag = np.einsum("fnj,fij->fni", h + E, np.abs(W)) + _z(None if b is None else np.abs(b))
            E = np.einsum("fnj,fij->fni", E, np.abs(W)) + g(counts.mid) * mag
            live = fac[:, l + 1] != 0
            undecided += int((live & (np.abs(z) <= E) & ~((z == 0) & (E == 0))).sum())
            judged += int(live.sum())
            h, E = behind(z, E, l + 1)
        b = None if net.b_last is None else net.b_last[:, None, :]
        f = np.einsum("fnj,fcj->fnc", h, net.w_last) + _z(b)
        mag = np.einsum("fnj,fcj->fnc", h + E, np.abs(net.w_last)) + _z(None if b is None else np.abs(b))
        E = np.einsum("fnj,fcj->fnc", E, np.abs(net.w_last)) + g(counts.last) * mag
    if sum_features:
        A = mag if counts.interleaved else np.abs(f)
        truth = f.sum(0)
        bound = E.sum(0) + g(counts.adds) * (A + E).sum(0)
    else:
        truth = np.transpose(f, (1, 0, 2)).reshape(n, F * C)
        bound = np.transpose(E, (1, 0, 2)).reshape(n, F * C)
    return Forward(truth, bound, undecided, judged, f)


# ---------------------------------------------------------------------------------------------------------------------------
# backward
# ---------------------------------------------------------------------------------------------------------------------------
def _reverse(net, x, g, fac, masks=None, ge=False):
    """The reverse pass at the head of csrc/fmlp_bwd.hip for all features at once on arrays of any dtype (float64, or int64 for the
    exact family, where ``net`` holds scaled integers and the biases are lifted by the caller).  ``x [F, n]``, ``g [F, n, C]``,
    ``fac [F, L - 1, n, H]``.  ``masks``: take these ``[z > 0]`` instead of the pass's own (the magnitude pass).  Returns the six
    gradients by name, the masks, and the hidden pre-activations."""
    L = net.L
    xk = x[:, :, None]
    pos = (lambda z: z >= 0) if ge else (lambda z: z > 0)
    a1 = xk * net.w_first[:, None, :] + _z(None if net.b_first is None else net.b_first[:, None, :])
    r1 = pos(a1) if masks is None else masks[0]
    h1 = r1 * a1 * fac[:, 0]
    out = {}
    if L == 3:
        W2 = net.w_mid[0]
        z2 = np.einsum("fnj,fij->fni", h1, W2) + _z(None if net.b_mid is None else net.b_mid[0][:, None, :])
        r2 = pos(z2) if masks is None else masks[1]
        h2 = r2 * z2 * fac[:, 1]
        hl = h2
    else:
        z2, r2, hl = None, None, h1
    out["w_last"] = np.einsum("fnc,fnj->fcj", g, hl)
    if net.b_last is not None:
        out["b_last"] = g.sum(1)
    dh = np.einsum("fnc,fcj->fnj", g, net.w_last)
    if L == 3:
        dz2 = r2 * dh * fac[:, 1]
        if net.b_mid is not None:
            out["b_mid"] = dz2.sum(1)[None]
        out["w_mid"] = np.einsum("fni,fnj->fij", dz2, h1)[None]
        dh = np.einsum("fni,fij->fnj", dz2, W2)
    dz1 = r1 * dh * fac[:, 0]
    out["w_first"] = (dz1 * xk).sum(1)
    if net.b_first is not None:
        out["b_first"] = dz1.sum(1)
    return out, (r1, r2), (a1, z2)


def _abs_net(net: Net) -> Net:
    return Net(*[None if t is None else np.abs(t) for t in net[:6]], *net[6:])


def _g_of(g, F, C, sum_features):
    g = np.asarray(g)
    n = g.shape[0]
    if sum_features:
        return np.broadcast_to(g.reshape(1, n, C), (F, n, C))
    return np.transpose(g.reshape(n, F, C), (1, 0, 2))


class Backward(NamedTuple):
    truth: dict      # name -> float64 array in the stacked tensor's shape
    bound: dict
    mag: dict


def backward(net: Net, x, g, sum_features: bool, counts: dict, keep=None, p: float = 0.0, scale: int = 1, ge: bool = False) -> Backward:
    """Truth, bound and magnitude of the header for the counts of one route (L = 2, 3)."""
    assert net.L in (2, 3)
    x = np.asarray(x, dtype=np.float64)
    n, F = x.shape
    fac, _ = _factors(keep, p, n, F, net.L - 1, net.H)
    g3 = _g_of(np.asarray(g, dtype=np.float64), F, net.C, sum_features)
    truth, masks, _ = _reverse(net, x.T, g3, fac, ge=ge)
    mag, _, _ = _reverse(_abs_net(net), np.abs(x.T), np.abs(g3), fac, masks=masks)
    bound = {nm: U * np.abs(t) + gamma(scale * counts[nm]) * mag[nm] for nm, t in truth.items()}
    return Backward(truth, bound, mag)


# ---------------------------------------------------------------------------------------------------------------------------
# the per-element check
# ---------------------------------------------------------------------------------------------------------------------------
def worst_ratio(got, truth, bound):
    """``(ratio, flat index)``: the largest ``|got - t| / bound`` over the elements with a positive bound; inf at the first element that
    is not finite or misses a zero bound (which demands an exact zero)."""
    got = np.asarray(got, dtype=np.float64).reshape(truth.shape)
    err = np.abs(got - truth)
    bad = ~np.isfinite(got) | ((bound == 0) & (err != 0))
    if bad.any():
        return float("inf"), int(np.flatnonzero(bad.reshape(-1))[0])
    pos = bound > 0
    if not pos.any():
        return 0.0, 0
    r = np.where(pos, err / np.where(pos, bound, 1.0), 0.0)
    i = int(np.argmax(r))
    return float(r.reshape(-1)[i]), i


def assert_within(got, truth, bound, what=""):
    """Every element within its bound (a zero bound: an exact zero); returns the worst ratio."""
    got = np.asarray(got, dtype=np.float64).reshape(truth.shape)
    err = np.abs(got - truth)
    bad = ~(err <= bound)
    if bad.any():
        i = np.unravel_index(int(np.flatnonzero(bad.reshape(-1))[0]), truth.shape)
        raise AssertionError(f"{what}: {int(bad.sum())} of {truth.size} elements outside their bound; first at {tuple(int(v) for v in i)}: "
                             f"got {got[i]!r} truth {truth[i]!r} error {err[i]:.3e} bound {bound[i]:.3e}")
    return worst_ratio(got, truth, bound)[0]


def within(got, truth, bound) -> bool:
    got = np.asarray(got, dtype=np.float64).reshape(truth.shape)
    return bool((np.abs(got - truth) <= bound).all())


def grads_dict(outs) -> dict:
    """The six outputs of a backward launch (None where absent) by name, as numpy."""
    d = {}
    for nm, t in zip(NAMES, outs):
        if t is not None:
            d[nm] = t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)
    return d


def hold_grads(got: dict, ref: Backward, what=""):
    """Every element of every gradient tensor within its bound; the worst ratio and the tensor it is in."""
    assert set(got) == set(ref.truth), (what, sorted(got), sorted(ref.truth))
    worst, where = 0.0, None
    for nm in NAMES:
        if nm in got:
            r = assert_within(got[nm], ref.truth[nm], ref.bound[nm], f"{what} d {nm}")
            if r >= worst:
                worst, where = r, nm
    return worst, where


def grads_within(got: dict, ref: Backward) -> bool:
    return all(within(got[nm], ref.truth[nm], ref.bound[nm]) for nm in ref.truth)


# ---------------------------------------------------------------------------------------------------------------------------
# exact family
# ---------------------------------------------------------------------------------------------------------------------------
LIMIT = 1 << 24


def _ints(a, q):
    """``a 2^q`` as int64, asserted integral."""
    if a is None:
        return None
    v = np.asarray(a, dtype=np.float64) * 2.0 ** q
    assert np.array_equal(v, np.round(v)) and np.abs(v).max(initial=0) < 2 ** 40, "not a multiple of the quantum"
    return v.astype(np.int64)


class Exact(NamedTuple):
    out: np.ndarray      # float64, exactly what every route must store
    grads: Optional[dict]
    worst_bits: float    # log2 of the largest magnitude in quanta (< 24)


def exact(net: Net, x, sum_features: bool, g=None, keep=None, p: float = 0.0, qw: int = 4, qx: int = 3) -> Exact:
    """The forward (any L >= 2) and, with ``g`` (integers; L = 2, 3), the six gradients in int64.  Weights and biases are multiples of
    ``2^-qw``, ``x`` of ``2^-qx``, Dropout is off or ``p = 0.5`` (scale 2).  Hidden layer ``l`` lives on the quantum
    ``2^-(qx + l qw)``; the biases are lifted to their layer's quantum.  The ``< 2^24`` condition is asserted on the magnitudes of
    every intermediate and every result (all masks on, kept units only)."""
    x = np.asarray(x, dtype=np.float64)
    n, F = x.shape
    L, H, C = net.L, net.H, net.C
    assert L >= 2 and (not p or p == 0.5)
    W = Net(*[_ints(t, qw) for t in net[:6]], *net[6:])
    A = _abs_net(W)
    X = _ints(x.T, qx)
    fac, _ = _factors(keep, p, n, F, L - 1, H)
    fac = fac.astype(np.int64)
    worst = [0]

    def see(m):
        worst[0] = max(worst[0], int(np.abs(m).max(initial=0)))
        assert worst[0] < LIMIT, f"magnitude {worst[0]} >= 2^24 quanta"

    def lift(b, l):                                   # a bias of layer l (1-based) onto the quantum 2^-(qx + l qw)
        return 0 if b is None else b * (1 << (qx + (l - 1) * qw))

    def chain(Wn, Xn, masked):
        zs = []
        z = Xn[:, :, None] * Wn.w_first[:, None, :] + lift(None if Wn.b_first is None else Wn.b_first[:, None, :], 1)
        zs.append(z)
        h = (np.maximum(z, 0) if masked else z) * fac[:, 0]
        for l in range(L - 2):
            z = np.einsum("fnj,fij->fni", h, Wn.w_mid[l]) + lift(None if Wn.b_mid is None else Wn.b_mid[l][:, None, :], l + 2)
            zs.append(z)
            h = (np.maximum(z, 0) if masked else z) * fac[:, l + 1]
        f = np.einsum("fnj,fcj->fnc", h, Wn.w_last) + lift(None if Wn.b_last is None else Wn.b_last[:, None, :], L)
        return zs, h, f
    zs_m, h_m, f_m = chain(A, np.abs(X), False)
    for m in zs_m + [h_m, f_m]:
        see(m)
    zs, h, f = chain(W, X, True)
    qo = qx + L * qw
    if sum_features:
        see(f_m.sum(0))
        out = f.sum(0).astype(np.float64) * 2.0 ** -qo
    else:
        out = np.transpose(f, (1, 0, 2)).reshape(n, F * C).astype(np.float64) * 2.0 ** -qo
    grads = None
    if g is not None:
        assert L in (2, 3)
        G = _ints(_g_of(g, F, C, sum_features), 0)
        # the reverse pass on integers: the biases never enter it, the forward values come from the lifted chain above
        Wl = Net(W.w_first, None if W.b_first is None else lift(W.b_first, 1), W.w_mid,
                 None if W.b_mid is None else lift(W.b_mid, 2), W.w_last, W.b_last, L, H, C, F)
        Al = _abs_net(Wl)
        got, masks, _ = _reverse(Wl, X, G, fac)
        ones = tuple(None if m is None else np.ones_like(m) for m in masks)
        mags, _, _ = _reverse(Al, np.abs(X), np.abs(G), fac, masks=ones)
        q1 = qx + qw
        quanta = {"w_last": q1 + (L - 2) * qw, "b_last": 0, "w_mid": qw + q1, "b_mid": qw, "w_first": (L - 1) * qw + qx,
                  "b_first": (L - 1) * qw}
        grads = {}
        for nm, v in got.items():
            see(mags[nm])
            grads[nm] = v.astype(np.float64) * 2.0 ** -quanta[nm]
    return Exact(out, grads, float(np.log2(max(worst[0], 1))))


# ---------------------------------------------------------------------------------------------------------------------------
# emulations (numpy float32, the kernels' own order)
# ---------------------------------------------------------------------------------------------------------------------------
F32 = np.float32


def _f32(a):
    return None if a is None else np.asarray(a, dtype=F32)


def _scale32(p):
    return F32(1.0) / (F32(1.0) - F32(p)) if p else F32(1.0)


def emulate_lane(net: Net, x, sum_features: bool, keep=None, p: float = 0.0, plant=None):
    """fmlp_lane_kernel's forward in float32, its own order: per feature the first layer's multiply-add, ``dense_layer``'s chain over
    ``j`` onto the bias, ``sacc += v`` over the features.  ``plant``: ``("skip_w2_col", k, j)`` leaves hidden unit ``j`` out of the
    first mid layer's chain of feature ``k``; ``("x0", node)`` evaluates that node at x = 0."""
    x = np.array(x, dtype=F32)
    n, F = x.shape
    L, H, C = net.L, net.H, net.C
    if plant is not None and plant[0] == "x0":
        x[plant[1], :] = 0
    s = _scale32(p)
    km = None if keep is None or not p else np.asarray(keep.detach().cpu().numpy() if hasattr(keep, "detach") else keep).astype(bool)
    out = np.zeros((n, C if sum_features else F * C), dtype=F32)

    def dense(Wm, b, h, skip=None):
        acc = np.zeros((n, Wm.shape[0]), dtype=F32) if b is None else np.broadcast_to(_f32(b), (n, Wm.shape[0])).copy()
        Wm = _f32(Wm)
        for j in range(Wm.shape[1]):
            if j == skip:
                continue
            acc = (Wm[None, :, j] * h[:, j:j + 1]).astype(F32) + acc
        return acc
    for k in range(F):
        xv = x[:, k:k + 1]
        if L == 1:
            v = (xv * _f32(net.w_last[k])[None, :]).astype(F32) + (F32(0) if net.b_last is None else _f32(net.b_last[k])[None, :])
        else:
            h = (xv * _f32(net.w_first[k])[None, :]).astype(F32) + (F32(0) if net.b_first is None else _f32(net.b_first[k])[None, :])
            h = np.maximum(h, F32(0))
            if km is not None:
                h = np.where(km[:, k, 0], h * s, F32(0)).astype(F32)
            for l in range(L - 2):
                skip = plant[2] if plant is not None and plant[0] == "skip_w2_col" and plant[1] == k and l == 0 else None
                h = np.maximum(dense(net.w_mid[l][k], None if net.b_mid is None else net.b_mid[l][k], h, skip), F32(0))
                if km is not None:
                    h = np.where(km[:, k, l + 1], h * s, F32(0)).astype(F32)
            v = dense(net.w_last[k], None if net.b_last is None else net.b_last[k], h)
        if sum_features:
            out = out + v
        else:
            out[:, k * C:(k + 1) * C] = v
    return out


def emulate_bwd(net: Net, x, g, sum_features: bool, k: int, keep=None, p: float = 0.0, plant=None):
    """``gnan_bwd::feature_grads``' order in float32 for feature ``k`` (L = 2, 3), with gnan_fmlp_bwd's splits: a wave owns every
    fourth node of its split, the chains run over ``t`` / ``c`` in order, the four waves meet in wave order and the splits in split
    order.  Returns ``{name: the feature's slice}``.  ``plant``: ``("flip", node, layer, unit)`` flips one mask; ``("ge",)`` takes
    ``>=`` for ``>``; ``("drop_split", s)`` leaves split ``s`` out of the last sum."""
    x = np.asarray(x, dtype=F32)
    n, F = x.shape
    L, H, C = net.L, net.H, net.C
    xv = x[:, k]
    gk = np.asarray(g, dtype=F32).reshape(n, -1)
    gk = gk[:, :C] if sum_features else gk[:, k * C:(k + 1) * C]
    s = _scale32(p)
    if keep is None or not p:
        m = np.ones((n, L - 1, H), dtype=F32)
    else:
        km = np.asarray(keep.detach().cpu().numpy() if hasattr(keep, "detach") else keep)[:, k]
        m = np.where(km != 0, s, F32(0)).astype(F32)
    ge = plant is not None and plant[0] == "ge"
    pos = (lambda z: z >= 0) if ge else (lambda z: z > 0)
    w1, b1 = _f32(net.w_first[k]), (np.zeros(H, F32) if net.b_first is None else _f32(net.b_first[k]))
    W3 = _f32(net.w_last[k])                                         # [C, H]
    a1 = (w1[None, :] * xv[:, None]).astype(F32) + b1[None, :]
    r1 = pos(a1)
    if plant is not None and plant[0] == "flip" and plant[2] == 0:
        r1[plant[1], plant[3]] ^= True
    h1 = np.where(r1, a1 * m[:, 0], F32(0)).astype(F32)
    if L == 3:
        W2 = _f32(net.w_mid[0][k])
        z2 = np.broadcast_to(np.zeros(H, F32) if net.b_mid is None else _f32(net.b_mid[0][k]), (n, H)).copy()
        for t in range(H):
            z2 = (W2[None, :, t] * h1[:, t:t + 1]).astype(F32) + z2
        r2 = pos(z2)
        if plant is not None and plant[0] == "flip" and plant[2] == 1:
            r2[plant[1], plant[3]] ^= True
        h2 = np.where(r2, z2 * m[:, 1], F32(0)).astype(F32)
        hl = h2
    else:
        hl = h1
    dh = np.zeros((n, H), F32)
    for c in range(C):
        dh = (gk[:, c:c + 1] * W3[None, c, :]).astype(F32) + dh
    if L == 3:
        dz2 = np.where(r2, dh * m[:, 1], F32(0)).astype(F32)
        dh = np.zeros((n, H), F32)
        for t in range(H):
            dh = (W2[None, t, :] * dz2[:, t:t + 1]).astype(F32) + dh
    dz1 = np.where(r1, dh * m[:, 0], F32(0)).astype(F32)
    splits, nps = node_splits(n, F, "lane")
    names = ["w_first", "b_first", "w_last", "b_last"] + (["w_mid", "b_mid"] if L == 3 else [])
    shapes = {"w_first": (H,), "b_first": (H,), "w_mid": (H, H), "b_mid": (H,), "w_last": (C, H), "b_last": (C,)}
    total = None
    for sp in range(splits):
        lo, hi = sp * nps, min((sp + 1) * nps, n)
        waves = []
        for wv in range(4):
            acc = {nm: np.zeros(shapes[nm], F32) for nm in names}
            for node in range(lo + wv, hi, 4):
                acc["w_last"] = (gk[node][:, None] * hl[node][None, :]).astype(F32) + acc["w_last"]
                acc["b_last"] = acc["b_last"] + gk[node]
                if L == 3:
                    acc["b_mid"] = acc["b_mid"] + dz2[node]
                    acc["w_mid"] = (dz2[node][:, None] * h1[node][None, :]).astype(F32) + acc["w_mid"]
                acc["w_first"] = (dz1[node] * xv[node]).astype(F32) + acc["w_first"]
                acc["b_first"] = acc["b_first"] + dz1[node]
            waves.append(acc)
        block = {nm: ((waves[0][nm] + waves[1][nm]) + waves[2][nm]) + waves[3][nm] for nm in names}
        if plant is not None and plant[0] == "drop_split" and plant[1] == sp:
            continue
        total = block if total is None else {nm: total[nm] + block[nm] for nm in names}
    present = {"w_first": True, "b_first": net.b_first is not None, "w_mid": L == 3, "b_mid": L == 3 and net.b_mid is not None,
               "w_last": True, "b_last": net.b_last is not None}
    return {nm: total[nm] for nm in names if present[nm]}


def stack_features(per_feature: list, net: Net) -> dict:
    """:func:`emulate_bwd`'s per-feature slices stacked into the six tensors' shapes."""
    out = {}
    for nm in per_feature[0]:
        a = np.stack([d[nm] for d in per_feature], 0)
        out[nm] = a[None] if nm in ("w_mid", "b_mid") else a
    return out
