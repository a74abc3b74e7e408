"""CPU side of the op-level veneer's fp64 checks (tests/ops_ref.py): for every case tests/test_gpu_ops_shapes.py runs on the
GPU, (a) torch's own float32 CPU op lies inside the bound -- the bound is wide enough for an honest fp32 implementation, and
is validated against the reference, not against the code under test -- and (b) every mutant the case lists lies outside it
(or differs where equality is asserted) -- the GPU check can fail.  A case no mutant fails is a defect of the case list."""
import numpy as np
import pytest
import torch

import ops_ref as R

CASES = [(f, c["name"]) for f, make in R.FAMILIES.items() for c in make()]
_cache = {}


def case(family, name):
    if family not in _cache:
        _cache[family] = {c["name"]: c for c in R.FAMILIES[family]()}
    return _cache[family][name]


@pytest.mark.parametrize("family,name", CASES, ids=[f"{f}-{n}" for f, n in CASES])
def test_bound_accepts_torch_fp32_and_rejects_every_mutant(family, name):
    c = case(family, name)
    exp = R.expected(c)
    got = R.honest(c)
    if exp[1] is not None:
        e = R.excess(got, exp[0], exp[1])
        print(f"{family}-{name}: torch fp32 at {float(e.max()) if e.size else 0.0:.3f} of the bound")
    assert R.accepts(c, got, exp), "torch's float32 op is outside the bound"
    assert c["mutants"], "no mutant listed"
    for m in c["mutants"]:
        wrong = R.MUTANTS[m](c)
        assert not R.accepts(c, wrong, exp), f"mutant {m} passes"
        if exp[1] is not None:
            print(f"  {m}: breaks {100 * R.broken_fraction(wrong, exp[0], exp[1]):.1f} % of the elements")


def test_matmul_bound_table():
    """The figures of the bound's derivation: torch fp32 well inside (K + 2) u cond, the drop-one-term mutant outside on nearly
    every element at short K and on a good share of them at K = 4321."""
    for (M, N, K), honest_max, broken_min in [((65, 129, 33), 0.5, 0.99), ((37, 45, 70), 0.5, 0.99), ((130, 70, 4321), 0.1, 0.2)]:
        g = R.rng(K)
        c = dict(family="matmul", name="t", a=R.f32(g.standard_normal((M, K))), pa=[], b=R.f32(g.standard_normal((K, N))), pb=[], mutants=[])
        ref, bound = R.expected(c)
        assert R.excess(R.honest(c), ref, bound).max() <= honest_max
        assert R.broken_fraction(R.MUTANTS["drop_last_k"](c), ref, bound) >= broken_min


@pytest.mark.parametrize("name", sorted(R.UNARY_REF))
def test_unary_gate_accepts_torch_fp32_and_rejects_half_precision(name):
    x = R.unary_sweep(name)
    ref = R.unary_ref(name, x)
    assert np.isfinite(ref).all() and (np.abs(ref) >= 2.0 ** -126).all() | (name in ("sin", "gelu", "silu")), "the sweep leaves the normal range"
    assert R.ULP_GATE[name] is not None and R.ULP_GATE[name] == 2.0 * R.ULP_MEASURED[name]
    bound = R.unary_bound(name, x, ref)
    got = R.UNARY_TORCH[name](torch.from_numpy(x)).numpy()
    print(f"{name}: torch fp32 worst {np.where(R.gate_domain(name, x), R.ulp_error(got, ref), 0.0).max():.2f} ULP, gate {R.ULP_GATE[name]}")
    assert R.inside(got, ref, bound)
    for m in ("f16_math",) + (("gelu_tanh",) if name == "gelu" else ()):
        assert not R.inside(R.UNARY_MUTANTS[m](name, x), ref, bound), m


@pytest.mark.parametrize("dtype", [R.BF16, R.F16])
def test_conversion_cases_tell_rounding_from_truncation(dtype):
    x = R.conversion_inputs()
    assert not R.bits_equal(R.convert_truncating(x, dtype), R.convert_ref(x, dtype))
    # and the reference is round-to-nearest-even: the two neighbours of a tie go to the even one
    tie = np.array([0x3F808000, 0x3F818000], np.uint32).view(np.float32)
    assert R.convert_ref(tie, R.BF16).view(np.uint32).tolist() == [0x3F800000, 0x3F820000]
    assert R.convert_ref(np.float32([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 65520.0, 65519.996]), R.F16).tolist() == [1.0, 1.0 + 2.0 ** -9, np.inf, 65504.0]


def test_big_array_cases_reach_past_the_grid():
    x = R.big_array()
    refs, _, _ = R.big_refs(x)
    for name, ref in refs.items():
        assert ref.size > R.GRID_THREADS and not R.bits_equal(R.grid_stride_dropped(ref), ref), name
