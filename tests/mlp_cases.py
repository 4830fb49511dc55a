"""The named cases of the direct shape-function kernels, shared by tests/test_mlp_bound.py (CPU) and
tests/test_gpu_mlp_elements.py (GPU) — TEST INFRASTRUCTURE ONLY.  References and bounds: tests/mlp_ref.py.

Every case has ``n <= 600``, ``F <= 6``, ``H <= 64``.  What the axes are there for:

    n     lane forward: 64 nodes per wave, 1 .. 4 waves per workgroup (1, 63, 65, 257); matrix-core tiles of 32 nodes, two per wave,
          256 per workgroup (1, 31, 33, 255, 257); backward: four nodes in flight, splits from n = 33 (1, 3, 5, 33, 65, 600; the
          matrix-core backwards split from n = 129)
    H     1, 8, 31, 32, 33, 64: the HT 1 / 2 boundary, padded units, JB = 8 remainders, the point kernel's scalar path (H % 4 != 0)
    C     1 .. 8 (CT padding, launch_bwd<C>); 9, 12, 31, 32, 33, 40, 64 (the mc kernels, CT32 1 / 2, 16-byte stores or not)
    L     1 .. 5 on the lane kernel, 2 / 3 on the point kernel, 3 / 4 on the matrix-core forwards, 2 / 3 on gnan_fmlp_bwd, 3 on the
          matrix-core backwards
    F     1, 2, odd counts, and F >= 4 at small n: feature_chunks cuts chunks and the even feat_chunk leaves a short last chunk
    bias on / off, sum_features on / off, Dropout off / p = 0.6 (the exact family: p = 0.5), row strides beyond the widths

Families: ``random`` (``_mlp_state``-style weights of tests/test_gpu_dropout_mfma.py, ``x = 2 rand - 0.5``, ``g = randn``);
``graded`` (the same, feature ``k``'s last layer and upstream gradient scaled by ``2^(-4 k)``: its elements are 2^-12 and smaller
against feature 0 — the family the global-norm rule cannot see); ``exact`` (weights and biases multiples of 1/2 in [-1, 1], ``x``
multiples of 1/4 in [-1, 1], ``g`` integers in [-2, 2]; bit for bit); ``exact-zero`` (the exact family with a second-layer unit
whose bias is 0 and whose two weights cancel on equal first-layer units: its pre-activation is an exact zero at every node, and
the strict ``>`` sends no gradient through it); ``e`` = +-100: the last layer times ``2^e`` and ``g`` times ``2^-e`` — the outputs
move by ``2^e``, ``d w_last`` / ``d b_last`` by ``2^-e``, the other four gradients keep their bits.

The seed of every case with a backward is chosen so that the case has NO undecided hidden unit (tests/mlp_ref.py, "Decided
masks"; tests/test_mlp_bound.py asserts it): the first seed from 0 that gives none.

The Dropout keep-mask is ``functional.dropout_masks``' (an input of the reference, owned by
test_every_units_keep_bit_is_gnan_dropout_masks); :func:`keep_mask` restates csrc/dropout.hpp's hash so that the CPU tests see
the very mask the kernels draw — the GPU tests assert the two equal and hand the library's to the reference.
"""
from functools import lru_cache
from typing import NamedTuple, Optional

import numpy as np
import torch

import mlp_ref as M

DROP_SEED = 123456789012345
QW, QX = 1, 2            # the exact family's quanta: weights 2^-1, x 2^-2


class Spec(NamedTuple):
    name: str
    n: int
    F: int
    L: int
    H: int
    C: int
    bias: bool = True
    sum_features: bool = False
    p: float = 0.0
    family: str = "random"
    pads: tuple = (0, 0, 0)      # extra floats per row of x, out, grad
    bwd: bool = False
    e: int = 0


def _s(n, F, L, H, C, bias=True, sum_features=False, p=0.0, family="random", pads=(0, 0, 0), bwd=False, e=0):
    name = f"{family}-n{n}-F{F}-L{L}-H{H}-C{C}" + ("" if bias else "-nobias") + ("-sum" if sum_features else "") + \
        (f"-p{p}" if p else "") + ("-strided" if any(pads) else "") + (f"-e{e}" if e else "")
    return Spec(name, n, F, L, H, C, bias, sum_features, p, family, pads, bwd, e)


# forward only: the layer counts and shapes no backward kernel covers, and the widest forward shapes
_FORWARD_ONLY = [
    _s(1, 1, 1, 0, 3), _s(63, 3, 1, 0, 2, bias=False, sum_features=True),
    _s(255, 3, 4, 64, 8), _s(257, 2, 4, 32, 4, sum_features=True), _s(33, 2, 4, 1, 1), _s(5, 6, 4, 33, 2, bias=False),
    _s(65, 3, 5, 8, 2), _s(257, 1, 5, 33, 5, bias=False, sum_features=True),
    _s(257, 2, 4, 33, 32), _s(1, 6, 4, 31, 64, bias=False), _s(63, 4, 4, 8, 9, sum_features=True, p=0.6),
    _s(257, 3, 4, 64, 8, bias=False, p=0.6), _s(31, 5, 4, 32, 3, sum_features=True, p=0.6),
    _s(63, 2, 4, 31, 2, family="exact"), _s(33, 3, 4, 32, 12, sum_features=True, family="exact"),
]
# both directions (L = 2, 3): seeds by the decided-mask search
_BOTH = [
    _s(1, 1, 2, 1, 1), _s(3, 2, 2, 8, 2, bias=False, sum_features=True), _s(5, 5, 3, 31, 3), _s(1, 2, 3, 8, 4),
    _s(33, 1, 3, 32, 4, sum_features=True), _s(63, 1, 3, 33, 7, sum_features=True), _s(64, 1, 3, 64, 8),
    _s(5, 6, 3, 32, 2), _s(31, 2, 3, 8, 3, bias=False), _s(33, 5, 3, 33, 3, sum_features=True),
    _s(65, 3, 3, 33, 5, bias=False), _s(600, 2, 3, 64, 1, sum_features=True), _s(257, 5, 3, 64, 3),
    _s(300, 4, 3, 33, 8, sum_features=True), _s(65, 6, 2, 64, 7), _s(33, 3, 3, 1, 6), _s(129, 1, 3, 8, 2, bias=False),
    _s(255, 2, 2, 33, 8, sum_features=True), _s(1, 4, 3, 64, 5, sum_features=True), _s(257, 4, 3, 31, 1, bias=False, sum_features=True),
    # many channels (the mc kernels)
    _s(65, 3, 3, 64, 40), _s(33, 2, 3, 32, 9, bias=False, sum_features=True), _s(129, 2, 3, 33, 33), _s(5, 4, 3, 8, 64, sum_features=True),
    _s(257, 1, 3, 31, 32), _s(600, 2, 3, 64, 31, bias=False), _s(129, 4, 3, 64, 64, sum_features=True),
    # Dropout
    _s(65, 3, 3, 33, 5, p=0.6), _s(33, 2, 2, 8, 3, sum_features=True, p=0.6), _s(257, 2, 3, 64, 8, sum_features=True, p=0.6),
    _s(129, 3, 3, 32, 1, bias=False, p=0.6), _s(65, 2, 3, 64, 40, p=0.6), _s(300, 2, 3, 8, 12, sum_features=True, p=0.6),
    _s(600, 1, 3, 64, 3, p=0.6), _s(33, 5, 3, 33, 3, sum_features=True, p=0.6),
    # row strides beyond the widths
    _s(65, 3, 3, 32, 3, pads=(2, 3, 3)), _s(33, 2, 3, 64, 12, sum_features=True, pads=(1, 1, 2)),
    _s(129, 2, 2, 31, 4, p=0.6, pads=(3, 4, 1)), _s(5, 3, 3, 8, 2, pads=(1, 2, 5)), _s(257, 2, 3, 8, 8, p=0.6, pads=(3, 4, 4)),
    # graded scales
    _s(65, 6, 3, 32, 3, family="graded"), _s(129, 5, 3, 64, 12, family="graded"), _s(257, 5, 2, 31, 2, family="graded"),
    _s(65, 4, 3, 33, 4, sum_features=True, family="graded"),
    # exact
    _s(65, 3, 3, 32, 3, family="exact"), _s(33, 2, 3, 64, 8, sum_features=True, family="exact"), _s(5, 4, 2, 8, 4, family="exact"),
    _s(65, 3, 3, 33, 5, p=0.5, family="exact"), _s(33, 2, 3, 32, 40, family="exact"), _s(129, 2, 3, 33, 2, bias=False, family="exact"),
    _s(65, 2, 3, 8, 3, family="exact-zero"), _s(33, 2, 3, 32, 40, p=0.5, family="exact"),
    _s(65, 3, 3, 32, 3, family="exact", e=100), _s(65, 3, 3, 32, 3, family="exact", e=-100),
    _s(33, 2, 3, 32, 40, family="exact", e=100), _s(33, 2, 3, 32, 40, family="exact", e=-100),
]
# name -> the first seed from 0 without an undecided unit, where that is not 0 (every committed case: seed 0 has none)
SEEDS = {}

SPECS = {s.name: s for s in _FORWARD_ONLY + [s._replace(bwd=True) for s in _BOTH]}
assert len(SPECS) == len(_FORWARD_ONLY) + len(_BOTH), "case names are unique"
ALL = tuple(SPECS)
BACKWARD = tuple(nm for nm, s in SPECS.items() if s.bwd)
EXACT = tuple(nm for nm, s in SPECS.items() if s.family.startswith("exact") and not s.e)
MOVED = tuple(nm for nm, s in SPECS.items() if s.e)
GRADED = tuple(nm for nm, s in SPECS.items() if s.family == "graded")


def base_of(name: str) -> str:
    """The unit-exponent case of an ``e`` variant."""
    return name[:name.rindex("-e")]


class Case(NamedTuple):
    spec: Spec
    params: tuple                    # the six stacked float32 torch tensors (None where absent), then L, H, C, F
    net: M.Net
    x: np.ndarray                    # float32 [n, F]
    g: Optional[np.ndarray]          # float32 [n, C] or [n, F C]
    keep: Optional[np.ndarray]       # uint8 [n, F, L - 1, H] under Dropout

    @property
    def name(self):
        return self.spec.name


# ---------------------------------------------------------------------------------------------------------------------------
# csrc/dropout.hpp, restated on uint32 arrays
# ---------------------------------------------------------------------------------------------------------------------------
def _mix32(h):
    h = h.astype(np.uint32)
    h = h ^ (h >> np.uint32(16))
    h = h * np.uint32(0x85ebca6b)
    h = h ^ (h >> np.uint32(13))
    h = h * np.uint32(0xc2b2ae35)
    return h ^ (h >> np.uint32(16))


def drop_threshold(p: float) -> int:
    t = float(np.float32(p)) * 4294967296.0
    return 0 if t <= 0 else min(int(t), 4294967295)


def keep_mask(seed: int, p: float, n: int, F: int, n_hidden: int, H: int) -> np.ndarray:
    """``gnan_dropout_mask`` (csrc/fmlp.hip:606-616; drop_base / drop_keep of csrc/dropout.hpp:23-31): uint8 ``[n, F, n_hidden, H]``."""
    node = np.arange(n, dtype=np.uint64)
    lo, hi = np.uint32(seed & 0xffffffff), np.uint32((seed >> 32) & 0xffffffff)
    a = _mix32(lo ^ node.astype(np.uint32))
    feat = np.arange(F, dtype=np.uint32) * np.uint32(0x85ebca77)
    node_hi = (node >> np.uint64(32)).astype(np.uint32) * np.uint32(0x9e3779b1)
    base = _mix32((a ^ hi ^ node_hi)[:, None] ^ feat[None, :])                                   # [n, F]
    layer = np.arange(n_hidden, dtype=np.uint32)[:, None] * np.uint32(4096)
    unit = np.arange(H, dtype=np.uint32)[None, :] + np.uint32(1)
    salt = (layer + unit) * np.uint32(0xc2b2ae3d)                                                # [n_hidden, H]
    return (_mix32(base[:, :, None, None] ^ salt[None, None]) >= np.uint32(drop_threshold(p))).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------------------
# building a case
# ---------------------------------------------------------------------------------------------------------------------------
def _random_params(s: Spec, seed: int):
    g = torch.Generator().manual_seed(seed)
    dims = [1] + [s.H] * (s.L - 1) + [s.C]
    w = [[None] * s.L for _ in range(s.F)]
    b = [[None] * s.L for _ in range(s.F)]
    for k in range(s.F):
        for li in range(s.L):
            w[k][li] = torch.randn(dims[li + 1], dims[li], generator=g) * (2.0 / (dims[li] + dims[li + 1])) ** 0.5
            b[k][li] = torch.randn(dims[li + 1], generator=g) * 0.5
    return w, b


def _exact_params(s: Spec, seed: int):
    rng = np.random.default_rng(1000 + seed)
    dims = [1] + [s.H] * (s.L - 1) + [s.C]
    half = lambda shape: torch.from_numpy(rng.integers(-2, 3, size=shape).astype(np.float32) / 2)   # noqa: E731
    w = [[half((dims[li + 1], dims[li])) for li in range(s.L)] for _ in range(s.F)]
    b = [[half((dims[li + 1],)) for li in range(s.L)] for _ in range(s.F)]
    if s.family == "exact-zero":
        assert s.L == 3 and s.H >= 3
        for k in range(s.F):
            w[k][0][0, 0] = w[k][0][1, 0] = 1.0          # first-layer units 0 and 1 are equal, and alive for x > -1/2
            b[k][0][0] = b[k][0][1] = 0.5
            j0 = s.H - 1
            w[k][1][j0, :] = 0.0
            w[k][1][j0, 0], w[k][1][j0, 1] = 1.0, -1.0   # z2[j0] = h1[0] - h1[1] + 0: an exact zero at every node
            b[k][1][j0] = 0.0
            w[k][2][:, j0] = 1.0                         # ... with a gradient waiting behind it
    return w, b


def _stack(s: Spec, w, b):
    F, L = s.F, s.L
    st = lambda t, li: torch.stack([t[k][li] for k in range(F)], 0).contiguous()   # noqa: E731
    if L == 1:
        return (None, None, None, None, st(w, 0)[..., 0].contiguous(), st(b, 0) if s.bias else None, 1, 0, s.C, F)
    w_mid = b_mid = None
    if L > 2:
        w_mid = torch.stack([st(w, li) for li in range(1, L - 1)], 0).contiguous()
        b_mid = torch.stack([st(b, li) for li in range(1, L - 1)], 0).contiguous() if s.bias else None
    return (st(w, 0)[..., 0].contiguous(), st(b, 0) if s.bias else None, w_mid, b_mid, st(w, L - 1), st(b, L - 1) if s.bias else None,
            L, s.H, s.C, F)


def build(s: Spec, seed: int) -> Case:
    width = s.C if s.sum_features else s.F * s.C
    if s.family.startswith("exact"):
        w, b = _exact_params(s, seed)
        rng = np.random.default_rng(2000 + seed)
        x = rng.integers(-4, 5, size=(s.n, s.F)).astype(np.float32) / 4
        g = rng.integers(-2, 3, size=(s.n, width)).astype(np.float32)
    else:
        w, b = _random_params(s, seed)
        gen = torch.Generator().manual_seed(seed + 1)
        x = (torch.rand(s.n, s.F, generator=gen) * 2 - 0.5).numpy()
        g = torch.randn(s.n, width, generator=gen).numpy()
    params = list(_stack(s, w, b))
    if s.family == "graded":
        sc = torch.tensor([2.0 ** (-4 * k) for k in range(s.F)])
        params[4] = params[4] * sc[:, None, None]
        if params[5] is not None:
            params[5] = params[5] * sc[:, None]
        if not s.sum_features:
            g = (g.reshape(s.n, s.F, s.C) * sc.numpy()[None, :, None]).reshape(s.n, width).astype(np.float32)
    if s.e:
        params[4] = torch.ldexp(params[4], torch.tensor(s.e))
        if params[5] is not None:
            params[5] = torch.ldexp(params[5], torch.tensor(s.e))
        g = np.ldexp(g, -s.e).astype(np.float32)
    keep = keep_mask(DROP_SEED, s.p, s.n, s.F, s.L - 1, s.H) if s.p else None
    params = tuple(params)
    return Case(s, params, M.net_of(params), np.ascontiguousarray(x, dtype=np.float32), g, keep)


@lru_cache(maxsize=None)
def case(name: str) -> Case:
    """The committed case (built once: the tests share it and leave it unchanged)."""
    s = SPECS[name]
    return build(s, SEEDS.get(base_of(name) if s.e else name, 0))


def undecided(c: Case):
    """``(undecided, judged)`` hidden units of the case under the largest count of any route (mlp_ref.DECIDE)."""
    if c.spec.L < 3:
        return 0, 0
    f = M.forward(c.net, c.x, c.spec.sum_features, M.DECIDE, c.keep, c.spec.p)
    return f.undecided, f.judged


def fwd_routes(s: Spec):
    return [r for r in M.FWD_ROUTES if M.fwd_covers(r, s.n, s.F, s.L, s.H, s.C, s.sum_features, bool(s.p))]


def bwd_routes(s: Spec):
    return [r for r in M.BWD_ROUTES if s.bwd and M.bwd_covers(r, s.L, s.H, s.C)]
