#!/usr/bin/env python3
"""Golden vectors of FOUR-layer models, captured by importing the upstream reference (build container only).

Run from the repo root:  ``python tests/golden/make_golden_deep.py``

Same conventions as ``make_golden.py`` (whose helpers it uses): seeded inputs through the reference's own pre-processing,
weights re-drawn at O(1) scale, float32 and float64 outputs and the gradients of ``out.pow(2).sum()``, data only.  The
cases are NOT listed in ``manifest.json`` — that list parametrises the existing tests — but named here;
``tests/test_deep_tables_host.py`` replays them against the oracle and the CPU route, ``tests/test_gpu_deep_tables.py``
through the modules on the GPU.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402

# (n_layers, hidden) in {(4, 16), (4, 64)} for models.TensorGNAN, (4, 16) for models.GNAN.  The 64-wide case has two
# features and 30 nodes: a four-layer MLP of that width is 8.6k parameters, stored three times over (state, g32, g64)
DEEP_CASES = [
    dict(id=500, variant="models_tensor_node", seed=0, n=40, f_raw=3, H=16, C=3, L=4, bias=True, normalize_rho=True,
         directed=False, n_isolated=2, rho_per_feature=False),
    dict(id=501, variant="models_tensor_node", seed=1, n=30, f_raw=1, H=64, C=3, L=4, bias=True, normalize_rho=True,
         directed=False, n_isolated=2, rho_per_feature=True),
    dict(id=502, variant="models_gnan", seed=2, n=40, f_raw=3, H=16, C=3, L=4, bias=True, normalize_rho=True,
         directed=False, n_isolated=2, rho_per_feature=False),
]
DEEP_NAMES = [f"case_{c['id']:03d}_{c['variant']}" for c in DEEP_CASES]


def main():
    for c, name in zip(DEEP_CASES, DEEP_NAMES):
        rng = np.random.default_rng(1000 + c["id"])
        ei = mg.random_graph(rng, c["n"], c["directed"], c["n_isolated"])
        n = c["n"]
        perm = np.arange(n)                      # (isolated nodes in the middle of the id range: see make_golden.main)
        top = int(ei.max())
        perm[[top, n - 1]] = perm[[n - 1, top]]
        ei = perm[ei]
        data = mg.run_pre_process(ei, n, c["f_raw"], rng, False)
        build, call = mg.build_and_call(c, data.x.shape[1])
        arrays = mg.capture(build, call, data, c["seed"])
        size = mg.save(name, c, data, arrays)
        print(f"{name}: out {arrays['out32'].shape} {size / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
