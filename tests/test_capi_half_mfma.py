"""CPU: the ``bwd_half_mfma`` tuning knob (the matrix-core backward for 16-bit features on graphs of 9..16
nodes): accepted values, range check, ``"reset"``, the header's knob list, and the unchanged ABI — all
decided on the host, so no GPU is needed.  Before the knob existed ``mrp_tuning_set`` rejected its name."""
import os

import mrp_gnn_amd as m

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_INVALID_VALUE = 1
ACCEPTED = (0, 1)  # 0: film_bwd_dx + the Gram pass, 1: film_bwd_mfma on 64-pixel groups (the default)


def test_bwd_half_mfma_knob_values_and_range():
    lib = m.load_library()
    try:
        for v in ACCEPTED:
            assert lib.mrp_tuning_set(b"bwd_half_mfma", v) == 0, v
        assert lib.mrp_tuning_set(b"bwd_half_mfma", ACCEPTED[-1] + 1) == HIP_INVALID_VALUE
        assert lib.mrp_tuning_set(b"bwd_half_mfma", -1) == HIP_INVALID_VALUE
    finally:
        assert lib.mrp_tuning_set(b"reset", 0) == 0


def test_bwd_half_mfma_knob_is_documented_in_the_header():
    header = open(os.path.join(ROOT, "include", "mrp_gnn.h"), "rb").read()
    assert b'"bwd_half_mfma"' in header


def test_reset_restores_the_default_and_the_abi_is_unchanged():
    """``mrp_tuning_set`` has no getter; the default (1) is pinned on the GPU by
    ``test_gpu_half_mfma.test_default_is_the_matrix_core_kernel``.  Here: ``"reset"`` after a change succeeds
    and leaves the knob settable, and no export or ABI bump came with the knob."""
    lib = m.load_library()
    assert lib.mrp_tuning_set(b"bwd_half_mfma", 0) == 0
    assert lib.mrp_tuning_set(b"reset", 0) == 0
    assert lib.mrp_tuning_set(b"bwd_half_mfma", 1) == 0
    assert lib.mrp_tuning_set(b"reset", 0) == 0
    assert lib.mrp_abi_version() == 22
