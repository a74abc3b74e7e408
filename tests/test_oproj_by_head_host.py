"""tests/oproj_by_head_ref.py on the CPU: for every case of the chain with o_proj per pair of kv heads, (a) the same computation in numpy float32
in the chain's order -- one dot product per 512-column slice, then the residual and the partial vectors added ascending -- stays inside
the derived bounds, and (b) every single-argument mutant that applies leaves them by a factor of at least 100: a slice merged from the
neighbouring q heads' partials, a partial vector dropped or added twice, the residual dropped, pm and pl swapped, one split too few.
So tests/test_gpu_oproj_by_head.py would see any of them.  Also: the engine's split-size table, and the margin of the end-to-end
fixture."""
import numpy as np
import pytest

import decode_kernels_ref as R
import oproj_by_head_ref as Q


@pytest.mark.parametrize("c", Q.OPROJ_CASES, ids=[c["name"] for c in Q.OPROJ_CASES])
def test_oproj_bounds_accept_fp32_and_reject_mutants(c):
    d = Q.oproj_inputs(c)
    honest = Q.oproj_excess(c, d, *Q.oproj_f32(c, d))
    print(f"{c['name']}: honest fp32 at {honest:.3f} of the bound")
    assert honest <= 1.0
    for m in Q.OPROJ_MUTATIONS:
        if not Q.oproj_mutation_applies(c, m):
            continue
        w = Q.oproj_excess(c, d, *Q.oproj_f32(c, d, m))
        print(f"{c['name']}: {m} at {w:.0f} x the bound")
        assert w >= 100.0, m


def test_every_oproj_mutation_is_exercised_by_some_case():
    for m in Q.OPROJ_MUTATIONS:
        assert any(Q.oproj_mutation_applies(c, m) for c in Q.OPROJ_CASES), m


@pytest.mark.parametrize("c", Q.PARTS_CASES, ids=[c["name"] for c in Q.PARTS_CASES])
def test_parts_bounds_accept_fp32_and_reject_mutants(c):
    d = Q.parts_inputs(c)
    x_ref, x_b = Q.parts_sum_reference(d)

    def worst(xs, out):
        # the sum against float64 (where a wrong sum shows); the GLU against the reference formed from the sum that was stored, as
        # the GPU test does
        g_ref, g_b = Q.parts_glu_reference(c, d, xs)
        return max(R.excess(xs, x_ref, x_b), R.excess(out, g_ref, g_b))

    honest = worst(*Q.parts_f32(c, d))
    print(f"{c['name']}: honest fp32 at {honest:.3f} of the bound")
    assert honest <= 1.0
    for m in Q.PARTS_MUTATIONS:
        if not Q.parts_mutation_applies(c, m):
            continue
        w = worst(*Q.parts_f32(c, d, m))
        print(f"{c['name']}: {m} at {w:.0f} x the bound")
        assert w >= 100.0, m


def test_split_cases_cover_both_sizes_and_the_regime_change():
    sizes = {c["kps"] for c in Q.DATTN_SPLIT_CASES}
    assert sizes == {32, 64}
    for k in sizes:
        pos = {c["pos"] for c in Q.DATTN_SPLIT_CASES if c["kps"] == k}
        assert {0, 31, 32, 33, 63, 64, 65, 511, 512} <= pos
    for c in Q.DATTN_SPLIT_CASES:
        ns = Q.dattn_nsplit(c)
        assert c["pos"] < ns * c["kps"] and (ns - 1) * c["kps"] < c["max_ctx"]


@pytest.mark.parametrize("c", [c for c in Q.DATTN_SPLIT_CASES if c["max_ctx"] == 96], ids=lambda c: c["name"])
def test_split_case_inputs_reject_attention_mutants(c):
    """The inputs of the split-size cases are decode_kernels_ref's: honest fp32 inside the bound, its mutants 100 x outside."""
    d = R.dattn_inputs(c)
    assert R.dattn_excess(c, d, *R.dattn_f32(c, d)) <= 1.0
    for m in R.DATTN_MUTATIONS:
        if m == "pos-1" and d["pos"] == 0:
            continue
        assert R.dattn_excess(c, d, *R.dattn_f32(c, d, m)) >= 100.0, m


def test_regime_table_keeps_sixteen_splits_or_fewer():
    """The engine's table (csrc/kernels.h dattn_fine_keys_per_split), restated: the smallest of 32 / 64 / 128 keys per split that keeps
    the live splits of a context at 16 or fewer; the kernel cases and the fixture straddle its first change."""
    table = lambda keys: 32 if keys <= 512 else 64 if keys <= 1024 else 128 if keys <= 2048 else 0
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "qwen3_asr_rs_amd", "csrc", "kernels.h")).read()
    m = re.search(r"inline int dattn_fine_keys_per_split\(int keys\) \{ return keys <= (\d+) \? (\d+) : keys <= (\d+) \? (\d+) : keys <= (\d+) \? (\d+) : 0; \}", src)
    assert m and [int(v) for v in m.groups()] == [512, 32, 1024, 64, 2048, 128]
    for keys in range(1, 2049):
        k = table(keys)
        assert (keys + k - 1) // k <= Q.MAX_SPLITS and (k == 32 or (keys + k // 2 - 1) // (k // 2) > Q.MAX_SPLITS)
    assert table(2049) == 0


def test_fixture_margin_in_the_oracle(tiny_oracle):
    """The end-to-end fixture of tests/test_gpu_oproj_by_head.py: over the whole run the fp32 oracle's top two logits stand further apart
    than 1e-3, orders of magnitude more than two fp32 summation orders differ by, and the context crosses 512 keys."""
    import torch
    from qwen3_asr_rs_amd import synthetic
    r = tiny_oracle.transcribe_ids(synthetic.synthetic_clip(Q.E2E_CLIP_SEED, Q.E2E_CLIP_SECONDS), fixed_new_tokens=Q.E2E_STEPS)
    margin = min(float(t[0] - t[1]) for t in (torch.topk(l, 2).values for l in r.step_logits))
    print(f"prompt {r.prompt_len}, {Q.E2E_STEPS} steps, smallest top-1 / top-2 margin {margin:.3e}")
    assert r.prompt_len <= 512 - 32 and r.prompt_len + Q.E2E_STEPS - 1 >= 512 + 8
    assert margin > Q.E2E_MIN_MARGIN
