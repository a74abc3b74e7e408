"""tests/gemv_plain_handover_ref.py on the CPU: for every case tests/test_gpu_gemv_plain_handover.py runs, (a) the same computation in
numpy float32 with another summation order stays inside the bound of tests/decode_kernels_ref.py, and (b) a broken hand-over of x --
slice 0 read 8 columns on, or the lanes beyond K left un-voided -- leaves it by a factor of at least 100: the GPU test would see it."""
import pytest

import decode_kernels_ref as R
import gemv_plain_handover_ref as H


@pytest.mark.parametrize("c", H.CASES, ids=H.IDS)
def test_bound_accepts_fp32_and_rejects_a_broken_handover(c):
    d, ref, bound = H.case_data(c)
    honest = R.excess(R.gemv_f32(c, d), ref, bound)
    print(f"{c['name']}: honest fp32 at {honest:.3f} of the bound")
    assert honest <= 1.0
    for m in H.MUTANTS:
        if not H.mutant_applies(c, m):
            continue
        w = R.excess(H.mutant(c, d, ref, m), ref, bound)
        print(f"{c['name']}: {m} at {w:.0f} x the bound")
        assert w >= 100.0, m


def test_every_mutant_is_exercised_at_both_slice_counts():
    for m in H.MUTANTS:
        assert {H.slices(c["K"]) for c in H.CASES if H.mutant_applies(c, m)} == {6, 12}, m
