"""The plain one-sequence GEMV at K > 2048 on the GPU against float64, per element (csrc/k_gemv.hip gemv1_body, the XH form: x is
fetched once per workgroup and handed to the four waves through LDS): the cases of tests/gemv_plain_handover_ref.py, one launch each
through q3a_selftest_gemv_launch in the precise arithmetic, against the input-derived bound of tests/decode_kernels_ref.py
(tests/test_gemv_plain_handover_host.py shows that a broken hand-over leaves it by a factor of at least 100).  The launch puts x into an
allocation that goes on past K with NaN, and the output between guard zones that it checks byte by byte: a read past K that is not
voided comes back as NaN, a store past N as a refusal.  Rows inside N that were never stored keep the sentinel.  Each test prints its
figure before it asserts."""
import ctypes as C

import numpy as np
import pytest

import decode_kernels_ref as R
import gemv_plain_handover_ref as H

pytestmark = pytest.mark.gpu


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _launch(lib, d, mode):
    """One launch_gemv call; a refusal fails the test, a HIP error ends the session (nothing more runs on a device that has faulted)."""
    N, K = d["W"].shape
    out = np.full(N, R.SENTINEL, np.float32)
    w = np.ascontiguousarray(R.bf16_bits(d["W"]))
    x, bias, resid = (None if d[k] is None else np.ascontiguousarray(d[k], np.float32) for k in ("x", "bias", "resid"))
    rc = lib.q3a_selftest_gemv_launch(0, 0, _ptr(w), N, K, _ptr(x), None, 0.0, _ptr(bias), mode, _ptr(resid), None, None, None, 0, 0,
                                      _ptr(out), None)
    if rc != 0:
        msg = (lib.q3a_last_error(None) or b"").decode()
        if "HIP error" in msg:
            pytest.exit(f"stopping: {msg}", returncode=3)
        pytest.fail(msg)
    return out


@pytest.mark.parametrize("c", H.CASES, ids=H.IDS)
def test_plain_gemv_hands_x_over_through_lds(lib, c):
    d, ref, bound = H.case_data(c)
    out = _launch(lib, d, c["mode"])
    w = R.excess(out, ref, bound)
    print(f"{c['name']}: at {w:.4f} of the bound")
    assert w <= 1.0
