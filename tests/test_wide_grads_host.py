"""Table-path parameter gradients of three-layer nets of 65-128 hidden units, host side (no GPU): the C entry point's range
checks, the Python gates, and the bound of tests/grads_ref.py at these widths — the numpy emulation of the kernel's order inside
it, two planted errors outside.  The kernel itself: tests/test_gpu_wide_grads.py; cases and the count of roundings:
tests/wide_grads_cases.py."""
import pytest

import gnan_amd  # noqa: F401
from gnan_amd import _lib, functional

import wide_grads_cases as W


def _null_args(L, H, C):
    return _lib.FpwlGradArgs(off=None, anchor=None, moments=None, moments_fixed=None, scales=None, w_first=None, b_first=None,
                             w_mid=None, b_mid=None, w_last=None, b_last=None, F=2, L=L, H=H, C=C, max_pieces=4, d_w_first=None,
                             d_b_first=None, d_w_mid=None, d_b_mid=None, d_w_last=None, d_b_last=None)


@pytest.mark.parametrize("H,C", [(65, 1), (128, 64)])
def test_wide_shapes_pass_the_range_check(H, C):
    """With null pointers the call gets as far as the pointer check (before this width was served: GNAN_ERR_UNSUPPORTED)."""
    lib = _lib.lib()
    assert lib.gnan_fpwl_param_grads(_null_args(3, H, C), None) == _lib.ERR_BAD_ARG
    assert b"null pointer" in lib.gnan_last_error()


def test_refusals_name_the_width_served():
    lib = _lib.lib()
    assert lib.gnan_fpwl_param_grads(_null_args(3, 129, 1), None) == _lib.ERR_UNSUPPORTED and b"H <= 128" in lib.gnan_last_error()
    assert lib.gnan_fpwl_param_grads(_null_args(4, 65, 1), None) == _lib.ERR_UNSUPPORTED and b"H <= 64" in lib.gnan_last_error()
    assert lib.gnan_fpwl_param_grads(_null_args(2, 129, 1), None) == _lib.ERR_UNSUPPORTED and b"H <= 128" in lib.gnan_last_error()
    assert lib.gnan_fpwl_param_grads(_null_args(3, 128, 65), None) == _lib.ERR_UNSUPPORTED and b"C <= 64" in lib.gnan_last_error()


def test_the_pinned_gate_is_unchanged(monkeypatch):
    """``_table_grads_applies`` also decides ``x.grad`` (``_input_grad_applies``, ``aggregate.reference_order_applies``), which
    stays out at these widths: the answers tests/test_deep_tables_host.py lists, whatever the new switch says."""
    for on in (True, False):
        monkeypatch.setattr(functional, "WIDE_TABLE_GRADS", on)
        g = functional._table_grads_applies
        assert g(4, 64, 1) and g(4, 8, 40)
        assert not g(4, 65, 1) and not g(5, 16, 1)
        assert g(3, 64, 1) and not g(3, 65, 1) and g(2, 128, 1) and not g(2, 129, 1) and g(3, 16, 4096) and not g(3, 16, 4097)
        assert not g(3, 128, 1)


def test_the_wide_gate(monkeypatch):
    monkeypatch.setattr(functional, "WIDE_TABLE_GRADS", True)
    g = functional._wide_table_grads_applies
    assert g(3, 65, 1) and g(3, 128, 4096) and g(3, 96, 40)
    assert not g(3, 64, 1) and not g(3, 129, 1) and not g(4, 96, 1) and not g(2, 96, 1) and not g(3, 128, 4097)
    monkeypatch.setattr(functional, "WIDE_TABLE_GRADS", False)
    for shape in [(3, 65, 1), (3, 128, 4096), (3, 96, 40), (3, 64, 1), (3, 129, 1), (4, 96, 1), (2, 96, 1)]:
        assert not g(*shape), shape
    monkeypatch.setattr(functional, "WIDE_TABLE_GRADS", True)
    monkeypatch.setattr(functional, "HIP_TABLE_GRADS", False)
    assert not g(3, 65, 1)


@pytest.mark.parametrize("name", ["H65-C1", "H127-C2-no-bias", "H128-C1-one-feature-empty", "H128-C65-wrapper"])
def test_the_emulation_is_inside_the_bound_and_planted_errors_are_not(name):
    """``emulate_piece`` at H in {65, 127, 128}, one and two groups, inside ``2 k`` (numpy has no fma); a kernel that kept the 16
    accumulators of H <= 64 (``W2[:, 64:]`` never read) and one that drops the last group's sums are outside."""
    case = W.case(name)
    assert sum(ex.undecided for ex in W.reference(case)) == 0
    for NG in (1, 2):
        ratio, where, _ = W.hold(case, W.emulate(case, NG), NG, k_scale=2)
        print(f"WIDE-EMULATION {name} NG={NG} ratio={ratio:.4f} at={where}")
        assert ratio <= 1.0, (name, NG, ratio, where)
    ratio, where, _ = W.hold(case, W.emulate(case, 1, edit=W.sixteen_accumulators), 1, k_scale=2)
    print(f"WIDE-EMULATION {name} sixteen accumulators ratio={ratio:.3g}")
    assert ratio > 1e6, (name, ratio)
    ratio, where, _ = W.hold(case, W.emulate(case, 2, plant="skip_last_group"), 2, k_scale=2)
    print(f"WIDE-EMULATION {name} skip_last_group ratio={ratio:.3g}")
    assert ratio > 1e3, (name, ratio)


def test_the_integer_family_is_exact_in_the_kernels_order():
    """H = 96, weights in {-2 .. 2}, integer moments: every partial sum is an integer or a half below 2^53, so the kernel's order
    must return the truth's own bits — checked here on the emulation before the kernel is held to it on the GPU."""
    case = W.case(W.INTEGER)
    ref = W.reference(case)
    assert sum(ex.undecided for ex in ref) == 0
    assert any(t != 0 for t in ref[0].grads["w_first"].reshape(-1)), "the network is alive right of the kinks"
    for NG in (1, 2):
        ok, name = W.truth_bits(case, W.emulate(case, NG))
        assert ok, (NG, name)
