"""tests/decode_kernels_ref.py on the CPU: for every case of the one-sequence decode kernels, (a) the same computation in numpy float32
with another summation order stays inside the derived bound, and (b) every single-argument mutation that applies to the case leaves it
by a factor of at least 100 -- the proof that the inputs make every argument matter, so that tests/test_gpu_decode_kernels.py would see
a mis-marshalled kernel argument."""
import numpy as np
import pytest

import decode_kernels_ref as R


@pytest.mark.parametrize("c", R.GEMV_CASES, ids=[c["name"] for c in R.GEMV_CASES])
def test_gemv_bound_accepts_fp32_and_rejects_mutants(c):
    d = R.gemv_inputs(c)
    ref, bound = R.gemv_reference(c, d)
    honest = R.excess(R.gemv_f32(c, d), ref, bound)
    print(f"{c['name']}: honest fp32 at {honest:.3f} of the bound")
    assert honest <= 1.0
    ran = 0
    for m in R.GEMV_MUTATIONS:
        if not R.gemv_mutation_applies(c, m):
            continue
        w = R.excess(R.gemv_f32(c, d, m), ref, bound)
        print(f"{c['name']}: {m} at {w:.0f} x the bound")
        assert w >= 100.0, m
        ran += 1
    assert ran >= 1


def test_every_gemv_mutation_is_exercised_by_some_case():
    for m in R.GEMV_MUTATIONS:
        assert any(R.gemv_mutation_applies(c, m) for c in R.GEMV_CASES), m


@pytest.mark.parametrize("c", R.ATTN_GEMV_CASES, ids=[c["name"] for c in R.ATTN_GEMV_CASES])
def test_attn_gemv_bound_accepts_fp32_and_rejects_mutants(c):
    d = R.attn_gemv_inputs(c)
    ref, bound = R.gemv_reference(c, d)
    honest = R.excess(R.attn_gemv_f32(c, d), ref, bound)
    print(f"{c['name']}: honest fp32 at {honest:.3f} of the bound")
    assert honest <= 1.0
    for m in R.ATTN_GEMV_MUTATIONS:
        if not R.attn_gemv_mutation_applies(c, m):
            continue
        w = R.excess(R.attn_gemv_f32(c, d, m), ref, bound)
        print(f"{c['name']}: {m} at {w:.0f} x the bound")
        assert w >= 100.0, m


@pytest.mark.parametrize("c", R.LM_HEAD_CASES, ids=[c["name"] for c in R.LM_HEAD_CASES])
def test_lm_head_winner_stands_clear_of_the_bound(c):
    """The planted row wins in float64 by more than twice the largest logit bound: any evaluation inside the bound picks it."""
    d, winner = R.lm_head_inputs(c)
    ref, bound = R.gemv_reference(dict(mode=0), d)
    top = np.argsort(ref)[::-1][:2]
    assert top[0] == winner and ref[top[0]] - ref[top[1]] > 2 * bound.max()
    assert int(np.argmax(R.gemv_f32(dict(mode=0), d))) == winner


@pytest.mark.parametrize("c", R.DATTN_CASES, ids=[c["name"] for c in R.DATTN_CASES])
def test_decode_attention_bound_accepts_fp32_and_rejects_mutants(c):
    d = R.dattn_inputs(c)
    honest = R.dattn_excess(c, d, *R.dattn_f32(c, d))
    print(f"{c['name']}: honest fp32 at {honest:.3f} of the bound")
    assert honest <= 1.0
    for m in R.DATTN_MUTATIONS:
        if m == "pos-1" and d["pos"] == 0:
            continue
        w = R.dattn_excess(c, d, *R.dattn_f32(c, d, m))
        print(f"{c['name']}: {m} at {w:.0f} x the bound")
        assert w >= 100.0, m
