"""Cases, inputs and mutants of the plain one-sequence GEMV at K > 2048 (csrc/k_gemv.hip gemv1_body, the XH form: the down projection),
where each thread fetches its 16-byte pieces of x once, the workgroup hands them over through LDS and every wave reads its 512-column
slices back.  References and bounds are those of tests/decode_kernels_ref.py.

Shapes: the smallest at which the hand-over can go wrong.
  K = 3072, 6144   every slice whole (KI = 6 and 12);
  K = 2560, 5640   the last slice wholly (2560 = 5 x 512) or all but 8 columns (5640 = 11 x 512 + 8) outside K: the pieces fetched for it
                   are clamped and the lanes that own its columns voided;
  K = 2056         the first K on this path, 8 columns into the third pair of slices;
  N = 5, 1021      one row per wave: a last workgroup with one wave at work and one with one wave idle -- clamped rows are never stored;
  N = 4098         two rows per wave (the forms launch_gemv picks from 4096 rows on), a last workgroup with one row at work.
Modes 0 and 1 (residual), each with and without a bias.

What a broken hand-over looks like, and why the inputs carry a plant.  The bound is 4 (K + 16) u times the sum of the terms' magnitudes,
about 4 gamma |y| with every column of ordinary inputs contributing alike.  An error confined to ONE of KI slices of such inputs is of
the order |y| / KI, i.e. 1 / (4 gamma KI) ~ 55 bounds at K = 6144: real, but short of the factor 100 asked of a mutant.  So the first
eight columns of x -- the piece thread 0 hands over, and the columns every voided lane is clamped to -- are scaled by PLANT = 1024 (a
power of two: exact).  They then hold about half of sum |terms|, and both mutants move a share of exactly that half:
  shifted slice    slice 0 read 8 columns on (x[k + 8] for x[k], k < 512): the planted columns are lost;
  un-voided        the lanes beyond K keep their products: each adds W[n][0..7] . x[0..7], the clamped address, once.
"""
import functools

import numpy as np

import decode_kernels_ref as R

PLANT = 1024.0


def _case(K, N, mode, bias):
    return dict(name=f"k{K}-n{N}-mode{mode}-{'bias' if bias else 'nobias'}", K=K, N=N, mode=mode, rms=False, bias=bias)


CASES = [_case(K, N, mode, bias) for K in (3072, 6144, 2560, 5640, 2056) for N in (5, 1021) for mode in (0, 1) for bias in (False, True)]
CASES += [_case(3072, 4098, 1, True), _case(5640, 4098, 0, False)]  # two rows per wave, KI = 6 and 12
IDS = [c["name"] for c in CASES]


def slices(K):
    """KI of the form launch_gemv picks: 512-column slices per wave."""
    assert 2048 < K <= 6144
    return 6 if K <= 3072 else 12


@functools.lru_cache(maxsize=2)  # (the tests of a case run back to back; a weight matrix is up to 92 MB)
def _case_data(name):
    c = next(c for c in CASES if c["name"] == name)
    d = R.gemv_inputs(c)
    d["x"][:8] *= np.float32(PLANT)
    ref, bound = R.gemv_reference(c, d)
    for v in list(d.values()) + [ref, bound]:
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d, ref, bound


def case_data(c):
    """(inputs, float64 reference, bound) of a case: computed once for the tests that share it, read-only."""
    return _case_data(c["name"])


MUTANTS = ["shifted slice", "un-voided"]


def mutant_applies(c, m):
    return m != "un-voided" or slices(c["K"]) * 512 > c["K"]


def mutant(c, d, ref, m):
    """What the kernel would return with the hand-over broken in way m (float64: the mutation alone, no rounding)."""
    W, x = d["W"].astype(np.float64), d["x"].astype(np.float64)
    if m == "shifted slice":
        return ref + W[:, :512] @ (x[8:520] - x[:512])
    void_lanes = (slices(c["K"]) * 512 - c["K"]) // 8
    return ref + void_lanes * (W[:, :8] @ x[:8])
