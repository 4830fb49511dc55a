"""``interpret.importance`` on the HIP path (``gnan_attr_reduce``): the nine module classes of tests/test_gpu_explain.py on a ~30-node
dense graph and a ~200-node K-hop CSR with a biased rho, every field against moments formed in float64 from the dense restatement of
tests/attr_ref.py and from ``interpret.explain`` on the GPU; groups by class, row subsets, a NAM, the identities and the refusals
(tests/importance_cases.py holds the checks, shared with the CPU route's file)."""
import pytest
import torch

import importance_cases as cases
from test_gpu_explain import MODULES, build, inputs_on

from gnan_amd import interpret

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("which", ["dense", "csr"])
@pytest.mark.parametrize("name", list(MODULES))
def test_importance_matches_restatement_and_explain(name, which):
    cases.check_module(name, which, DEV, 1e-5)


def test_rows_subset_with_groups():
    cases.check_rows_subset(DEV, 1e-5)


def test_nam_has_one_distance():
    cases.check_nam(DEV, 1e-5)


def test_refusals():
    cases.check_refusals(DEV)


def test_gpu_and_cpu_twin_agree_and_two_calls_give_equal_bits():
    labels = torch.arange(200) % 4
    a = interpret.importance(build("standalone_gnan_node_ids", DEV), inputs_on("csr", DEV), groups=labels)
    b = interpret.importance(build("standalone_gnan_node_ids", DEV), inputs_on("csr", DEV), groups=labels)
    twin = interpret.importance(build("standalone_gnan_node_ids", "cpu"), inputs_on("csr", "cpu"), groups=labels)
    for name in cases.FIELDS:
        assert torch.equal(getattr(a, name), getattr(b, name)), name
        cases.assert_rule(getattr(a, name), getattr(twin, name), what=f"CPU twin: {name}", floor=cases.TWO_FLOORS)
