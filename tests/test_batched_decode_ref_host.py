"""tests/batched_decode_ref.py on the CPU: for every case of the batched decode step's kernels, (a) the same computation in numpy float32
with another summation order stays inside the derived bound, and (b) every mutant that applies to the case -- one plausible mistake of
the kernel or its launcher, restated on the buffers the launch is given -- leaves it by a factor of at least 100 (at least 10 under the
wide bound of the attention form whose scores come from bf16(q)).  Every mutant applies to some case, and the case table reaches every
skinny_kernel family listed in the reference module: the proof that tests/test_gpu_batched_decode_kernels.py would see such a mistake."""
import os
import re

import numpy as np
import pytest

import batched_decode_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("c", R.SKINNY_CASES, ids=[c["name"] for c in R.SKINNY_CASES])
def test_skinny_bound_accepts_fp32_and_rejects_mutants(c):
    d = R.skinny_inputs(c)
    honest = R.skinny_excess(c, d, R.skinny_sim(c, d, honest=True))
    print(f"{c['name']}: honest fp32 at {honest:.3f} of the bound")
    assert honest <= 1.0
    for m in R.SKINNY_MUTANTS:
        if not R.skinny_applies(c, m):
            continue
        w = R.skinny_excess(c, d, R.skinny_sim(c, d, mut=m))
        print(f"{c['name']}: {m} at {w:.0f} x the bound")
        assert w >= 100.0, m


def test_every_mutant_is_exercised_by_some_case():
    for m in R.SKINNY_MUTANTS:
        assert any(R.skinny_applies(c, m) for c in R.SKINNY_CASES), m
    for m in R.ATTN_MUTANTS:
        assert any(R.attn_applies(c, m, form) for c in R.ATTN_CASES for form in R.OUT_FORMS), m


def test_case_table_reaches_every_family_and_states_a_consistent_form():
    reached = {R.family(c) for c in R.SKINNY_CASES}
    assert reached == set(R.FAMILIES), (sorted(set(R.FAMILIES) - reached), sorted(reached - set(R.FAMILIES)))
    assert len({c["name"] for c in R.SKINNY_CASES}) == len(R.SKINNY_CASES)
    for c in R.SKINNY_CASES:
        f = c["form"]
        per = (c["K"] // 32 + R.WAVES - 1) // R.WAVES
        if f["wlds"]:   # whole passes over a wave's K slice, and the LDS image the form states
            assert per % f["unr"] == 0 and (c["K"] // 32) % per == 0, c["name"]
            pieces = 1 if f["qs"] else 2
            assert f["dyn_lds"] == R.WAVES * f["tiles"] * (f["unr"] // 2) * pieces * 1024, c["name"]
        assert f["sh"] == (1 if c["S"] <= 16 or f["qs"] else 2) and f["split"] == int(c["split"]), c["name"]
        assert f["xmode"] == {"f32": 0, "f32norm": 1, "x16": 2, "x16frag": 2, "pre": 3}[c["x"]], c["name"]


def test_family_list_names_what_skinny_init_registers():
    """The twelve large-LDS families of FAMILIES are the instantiations skinny_init() sets the attribute for: LDS-staged x {1, 2} tiles x
    {1, 2} halves for each XMODE, the half-pair form and the two-pass pair form for XMODE 2 / 3 at both sequence-half counts."""
    src = open(os.path.join(ROOT, "qwen3_asr_rs_amd", "csrc", "k_skinny.hip")).read()
    init = src[src.index("const char* skinny_init()"):]
    init = init[:init.index("\n}\n")]
    xmodes = {int(m) for m in re.findall(r"allow_big_lds_shapes<(\d), \d+>", init)}
    assert xmodes == {0, 1, 2, 3}
    assert set(re.findall(r"allow_glu_hp3<(\d)>", init)) == {"1", "2"}
    assert {(int(a), int(b)) for a, b in re.findall(r"allow_glu_2pass<(\d), (\d), \d+>", init)} == {(1, 2), (2, 2), (1, 3), (2, 3)}
    body = src[src.index("hipError_t allow_big_lds_shapes()"):]
    assert re.findall(r"allow_big_lds<(\d), (\d), XMODE, UNR>", body[:body.index("\n}\n")]) == [("1", "1"), ("1", "2"), ("2", "1"), ("2", "2")]
    big = [f for f in R.FAMILIES if f[0] in ("wlds", "hp", "palias")]
    assert len(big) == 12


@pytest.mark.parametrize("kv_f32", [False, True], ids=["bf16-cache", "fp32-cache"])
@pytest.mark.parametrize("c", R.ATTN_CASES, ids=[c["name"] for c in R.ATTN_CASES])
def test_batched_attention_bound_accepts_fp32_and_rejects_mutants(c, kv_f32):
    d = R.attn_inputs(c, kv_f32)
    bf16_q = not kv_f32
    factor = 10.0 if bf16_q else 100.0
    for form in R.OUT_FORMS:
        honest = R.attn_excess(c, d, *R.attn_sim(c, d, form, bf16_q), form, bf16_q)
        print(f"{c['name']} {form}: honest fp32 at {honest:.3f} of the bound")
        assert honest <= 1.0
        for m in R.ATTN_MUTANTS:
            if not R.attn_applies(c, m, form):
                continue
            w = R.attn_excess(c, d, *R.attn_sim(c, d, form, bf16_q, mut=m), form, bf16_q)
            print(f"{c['name']} {form}: {m} at {w:.0f} x the bound")
            assert w >= factor, m


def test_split_path_bound_accepts_fp32_and_rejects_mutants():
    """The split kernel's partials in honest float32, merged as attn_combine merges them: inside the merge bound of the float64 merge
    and inside the context bound of the float64 attention; loud stale rows (not NaN), so a reader one row too far shows as a number."""
    c = R.SPLIT_CASE
    d = R.attn_inputs(c, False, stale_nan=False)
    pm, pl, po = R.split_partials_f32(c, d)
    R.check_empty_splits(c, d, pm, pl, po)
    ref, bound = R.combine_reference(pm, pl, po)
    got = R.combine_f32(pm, pl, po)
    w = float((np.abs(got - ref) / bound).max())
    print(f"combine: honest fp32 at {w:.3f} of the merge bound")
    assert w <= 1.0
    w = float((np.abs(R.combine_f32(pm, pl, po, "combine-drops-last-split") - ref) / bound).max())
    print(f"combine: last split dropped at {w:.0f} x the merge bound")
    assert w >= 100.0
    _, k, v = R.attn_new_rows(c, d, np.float32)
    ctx_ref, ctx_bound = R.attn_context(c, d, R.bf16_round(k), R.bf16_round(v))
    w = float((np.abs(got - ctx_ref) / ctx_bound).max())
    print(f"split path: honest fp32 context at {w:.3f} of the attention bound")
    assert w <= 1.0
    for m in ("pos-1", "pos+1", "caches-swapped", "new-row-not-patched"):
        bad, _ = R.attn_context(c, d, R.bf16_round(k), R.bf16_round(v), np.float32, mut=m)
        w = float((np.abs(bad - ctx_ref) / ctx_bound).max())
        print(f"split path: {m} at {w:.0f} x the attention bound")
        assert w >= 100.0, m
