"""tests/seg_attn_ref.py on the CPU: for every case of the segment attention (a) the same computation in numpy float32, tile by tile in
the kernel's order with P rounded to bf16 for the MFMA forms, stays inside the derived bound, and (b) every mutant that applies to the
case -- one plausible mistake of a kernel or its launcher -- leaves it by a factor of at least 10.  Every mutant applies to some case,
the case table reaches every instantiation the launchers can pick, and the fattn_block remap, restated in numpy, is a bijection on every
grid up to 6 x 8 x 12: the proof that tests/test_gpu_seg_attn.py would see such a mistake."""
import numpy as np
import pytest

import seg_attn_ref as R

ALL = R.CASES + R.grid_cases()
BF16_OUT_TOO = {"enc-dma", "enc-staged-f32", "pre-dma-g1", "pre-dma-g2", "pre-dma-g4", "pre-ksplit"}   # one of each MFMA kernel and layout


@pytest.mark.parametrize("c", ALL, ids=[c["name"] for c in ALL])
def test_bound_accepts_fp32_and_rejects_mutants(c):
    d = R.inputs(c)
    for out16 in ((False, True) if c["name"] in BF16_OUT_TOO else (False,)):
        honest = R.excess(c, d, R.sim(c, d, honest=True, out16=out16), out16)
        print(f"{c['name']}{' bf16 out' if out16 else ''}: honest fp32 at {honest:.3f} of the bound")
        assert honest <= 1.0
        for m in R.MUTANTS:
            if not R.applies(c, m, out16):
                continue
            w = R.excess(c, d, R.sim(c, d, mut=m, out16=out16), out16)
            print(f"{c['name']}{' bf16 out' if out16 else ''}: {m} at {w:.0f} x the bound")
            assert w >= 10.0, m


def test_every_mutant_is_exercised_by_some_case():
    for m in R.MUTANTS:
        assert any(R.applies(c, m, out16) for c in ALL for out16 in (False, True) if R.mfma(c) or not out16), m


def test_case_table_reaches_every_instantiation():
    """attn_kernel HD 64 and HD 128 x groups x both cache types; fattn_kernel x {fp32, bf16 K/V} x groups x KSPLIT 2; fattn_dma_kernel x
    HD 64 / 128 x groups (NS 4 and the bf16 staged encoder form come from the knob children of the GPU test, on these same cases)."""
    key = lambda f: (f["mfma"], f["dma"], f["hd"], f["group"], f["kv_f32"], f["ksplit"], f["qpw"])
    reached = {key(c["form"]) for c in ALL}
    want = {(0, 0, 64, 1, 1, 1, 8)} | {(0, 0, 128, g, kv, 1, 2 if g == 4 else 4) for g in (1, 2, 4) for kv in (0, 1)}
    want |= {(1, 0, 64, 1, 1, 1, 0), (1, 0, 128, 2, 0, 2, 0)} | {(1, 0, 128, g, 0, 1, 0) for g in (1, 2, 4)}
    want |= {(1, 1, 64, 1, 0, 1, 0)} | {(1, 1, 128, g, 0, 1, 0) for g in (1, 2, 4)}
    assert reached == want, (sorted(want - reached), sorted(reached - want))
    assert len({c["name"] for c in ALL}) == len(ALL)
    for c in R.CASES:   # the launcher's KSPLIT rule, restated: ceil(max_len / 64) n_kv n_segs < 128 at group 2
        if c["launcher"] == 3 and c["group"] == 2:
            wgs64 = (c.get("max_len", max(c["lens"])) + 63) // 64 * c["n_kv"] * len(c["lens"])
            assert (wgs64 < 128) == (c["form"]["ksplit"] == 2), c["name"]
    for (segs, n_kv, grid), c in zip(R.GRIDS, R.grid_cases()):
        assert grid == ((max(R.lens_of(c)) + 31) // 32, n_kv, len(segs)) and all((L + 31) // 32 == grid[0] or len(segs) > 1 for L in R.lens_of(c))
    assert sorted(g[0] * g[1] * g[2] for _, _, g in R.GRIDS) == [1, 7, 8, 9, 27]


def test_fattn_block_is_a_bijection_on_every_grid():
    for gx in range(1, 7):
        for gy in range(1, 9):
            for gz in range(1, 13):
                t = R.fattn_block(gx, gy, gz)
                assert t.min() >= 0 and (t.max(axis=0) < (gx, gy, gz)).all(), (gx, gy, gz)
                assert len({tuple(x) for x in t.tolist()}) == gx * gy * gz, (gx, gy, gz)


def test_loud_keys_are_loud():
    """A planted key scores about 4.5 above a typical one for the queries that see it."""
    c = R.BY_NAME["pre-dma-g2"]
    d = R.inputs(c)
    s, L = 6, c["lens"][6]
    q, k = d["q"][s][:, 0].astype(np.float64), d["k"][s][0].astype(np.float64)
    sc = q @ k.T / R.scale_of(c)
    loud = R.loud_keys(L)
    quiet = np.setdiff1d(np.arange(L), loud)
    gap = sc[:, loud].mean() - sc[:, quiet].mean()
    print(f"planted keys score {gap:.2f} above the others (std of the others {sc[:, quiet].std():.2f})")
    assert 3.5 <= gap <= 5.5
