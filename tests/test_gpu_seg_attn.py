"""Segment attention (encoder windows, causal prefill) on the GPU against float64, per element: csrc/k_attn.hip and the three kernels of
csrc/k_fattn.hip in every instantiation their launchers pick (the case table of tests/seg_attn_ref.py: one launch per case through
q3a_selftest_seg_attn_launch, the reported instantiation compared with the form the case states).  Output buffers go in filled with a
sentinel and come back whole; K/V rows behind a segment and q rows of no segment hold NaN.  Next to the float64 checks stand the relations
that must hold bit for bit: the bf16 output against the fp32 output, a segment alone against the ragged batch and under every grid, q16
against fp32 q, bf16 against fp32 K/V, a ring of four stages against three.  The knob forms (Q3A_FATTN_NS=4, Q3A_FATTN_DMA=0) run in
fresh child processes (tests/seg_attn_child.py).  Each test prints its figure before it asserts.  tests/test_seg_attn_ref_host.py shows
on the CPU what these checks would catch.

Worst excess (|got - ref| / bound, <= 1 passes) on an MI355X (also in tests/seg_attn_ref.py and DESIGN.md section 5):
    family                                               fp32 out                bf16 out
    fattn_dma_kernel HD 64 (encoder), NS 3 and 4         0.733                   0.757
    fattn_dma_kernel HD 128, GROUP 1 / 2 / 4             0.804 / 0.906 / 0.822   0.746 / 0.792 / 0.856
    fattn_dma_kernel GROUP 4, grids of 1 .. 27           0.496 .. 0.834          -
    fattn_kernel with q16 (Q3A_FATTN_DMA=0)              0.733; 0.804 / 0.906 / 0.822 (the DMA kernel's cases)
    fattn_kernel KSPLIT 2, q16 / fp32 q                  0.705 / 0.109           0.824 / -
    fattn_kernel behind fp32 q, GROUP 1 / 2 / 4          0.100 / 0.133 / 0.150   0.111 / 0.150 / 0.161   (the bound carries the rounding of q)
    fattn_kernel fp32 K/V, fp32 q (encoder)              0.065                   0.109
    attn_kernel HD 64                                    0.018                   -
    attn_kernel HD 128, GROUP 1 / 2 / 4, either cache    0.012 / 0.017 / 0.015   -
The P term is a half-ulp bound: the MFMA kernels with exact operands sit near it by construction (the honest float32 restatement reaches
0.906 on the same case).  Every case reported the form its table entry states, NS = 4 reproduced the NS = 3 bits, every bit-identity held.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import seg_attn_ref as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GRID_CASES = R.grid_cases()
ALL = R.CASES + GRID_CASES
MFMA_FORMS = ["enc-dma", "enc-staged-f32", "pre-dma-g1", "pre-dma-g2", "pre-dma-g4", "pre-ksplit", "pre-staged-g1", "pre-staged-g2", "pre-staged-g4"]
DMA_CASES = ["enc-dma", "pre-dma-g1", "pre-dma-g2", "pre-dma-g4"] + [c["name"] for c in GRID_CASES]
_runs = {}


def _launch(lib, c, out16=False):
    """The case's launch, once per session: (raw output buffer, form)."""
    key = (c["name"], out16)
    if key not in _runs:
        raw, form = R.launch(lib, c, R.inputs(c), out16)
        if raw is None:
            if "HIP error" in form:
                pytest.exit(f"stopping: {form}", returncode=3)
            pytest.fail(form)
        _runs[key] = (raw, form)
    return _runs[key]


def _checked(lib, c, out16=False, form_of=None):
    """Launch, compare the reported form and every element of the output buffer with float64, print, assert; the raw buffer."""
    raw, form = _launch(lib, c, out16)
    got = R.decode(raw, out16)
    by_seg = R.excess_by_segment(c, R.inputs(c), got, out16)
    w = R.excess(c, R.inputs(c), got, out16)
    print(f"{c['name']}{' bf16 out' if out16 else ''}: at {w:.4f} of the bound (per segment " + " ".join(f"{x:.3f}" for x in by_seg) + f"), form {form}")
    want = (form_of or c)["form"]
    assert {k: form[k] for k in want} == want
    assert w <= 1.0
    return raw


def _rows(c, raw, seg, kv_heads=None):
    """The output rows of segment `seg` (an index into c["lens"]) in a launch of c, the columns of the first kv_heads K/V heads."""
    ids, lens = list(R.seg_ids(c)), R.lens_of(c)
    i = ids.index(seg)
    r0 = int(np.sum(lens[:i]))
    cols = (kv_heads or R.n_kv_of(c)) * c["group"] * c["hd"]
    return raw[r0:r0 + lens[i], :cols]


@pytest.mark.parametrize("c", ALL, ids=[c["name"] for c in ALL])
def test_every_form_against_float64(lib, c):
    _checked(lib, c)


def test_grids_report_their_size(lib):
    """n_segs x n_kv x tiles = 1, 7, 8, 9, 27 workgroups through fattn_block: every triple is computed (a lost one leaves sentinels),
    and a segment's rows are the same bits under every grid."""
    raws = {}
    for (segs, n_kv, grid), c in zip(R.GRIDS, GRID_CASES):
        raws[c["name"]] = (c, _checked(lib, c))
        form = _launch(lib, c)[1]
        assert (form["grid_x"], form["grid_y"], form["grid_z"]) == grid
    (c1, r1), (c9, r9), (c27, r27) = (raws[GRID_CASES[i]["name"]] for i in (0, 3, 4))
    assert np.array_equal(_rows(c1, r1, 0), _rows(c27, r27, 0, kv_heads=1))
    assert np.array_equal(_rows(c9, r9, 1), _rows(c27, r27, 1))


@pytest.mark.parametrize("name", MFMA_FORMS)
def test_bf16_output_is_the_rounded_fp32_output(lib, name):
    c = R.BY_NAME[name]
    f32 = _checked(lib, c)
    b16 = _checked(lib, c, out16=True)
    written = f32 != R.SENT32
    want = np.where(written, R.bits16(R.bf16_round(np.where(written, f32, np.uint32(0)).view(np.float32))), R.SENT16)
    assert np.array_equal(b16, want)


@pytest.mark.parametrize("name,seg", [("enc-dma", 6), ("enc-staged-f32", 9), ("enc-valu", 8), ("pre-dma-g1", 6), ("pre-dma-g4", 3), ("pre-ksplit", 5),
                                      ("pre-staged-g1", 3), ("pre-staged-g4", 2), ("pre-valu-g2-bf16", 4), ("pre-valu-g4-f32", 1)])
def test_a_segment_alone_equals_the_segment_in_the_batch(lib, name, seg):
    """Another q_row0, another kv_off, another grid: the same bits."""
    c = R.BY_NAME[name]
    batch = _checked(lib, c)
    alone_c = R.sub_case(c, (seg,))
    alone = _checked(lib, alone_c)
    assert np.array_equal(_rows(c, batch, seg), _rows(alone_c, alone, seg))


@pytest.mark.parametrize("name", ["pre-dma-g2", "pre-staged-g2"])
def test_a_batch_in_another_order_gives_the_same_rows(lib, name):
    """Group 2 alone in a launch would be served by the KSPLIT kernel (few workgroups); the whole batch reversed keeps the form and
    moves every q_row0 and kv_off."""
    c = R.BY_NAME[name]
    batch = _checked(lib, c)
    rev_c = R.sub_case(c, tuple(reversed(range(len(c["lens"])))))
    rev = _checked(lib, rev_c)
    for s in range(len(c["lens"])):
        assert np.array_equal(_rows(c, batch, s), _rows(rev_c, rev, s)), s


@pytest.mark.parametrize("g", [1, 2, 4])
def test_valu_bf16_cache_equals_fp32_cache_holding_the_same_values(lib, g):
    a, b = _checked(lib, R.BY_NAME[f"pre-valu-g{g}-f32"]), _checked(lib, R.BY_NAME[f"pre-valu-g{g}-bf16"])
    assert np.array_equal(a, b)


def test_ksplit_q16_equals_fp32_q_holding_the_same_values(lib):
    c = R.BY_NAME["pre-ksplit"]
    assert np.array_equal(_checked(lib, c), _checked(lib, R.variant(c, q="f32x")))


# ---- the launchers' refusals -------------------------------------------------------------------------------------------------------
def _refused(lib, c, pk, out16=False):
    raw, msg = R.launch(lib, c, R.inputs(c), out16, pk=pk)
    assert raw is None, "the launch was served"
    assert "HIP error" not in msg, msg
    return msg


def _widened(pk, key, stride_key, by):
    a = pk[key]
    wide = np.full((a.shape[0], a.shape[1] + by), np.nan, a.dtype) if a.dtype.kind == "f" else np.full((a.shape[0], a.shape[1] + by), a.flat[0], a.dtype)
    wide[:, :a.shape[1]] = a
    return dict(pk, **{key: wide, stride_key: a.shape[1] + by})


def test_every_refusal_of_the_launchers_comes_back_as_an_error(lib):
    pre = R.sub_case(R.BY_NAME["pre-staged-g1"], (1,))                       # fp32 q
    pre16 = R.sub_case(R.BY_NAME["pre-dma-g1"], (2,))                        # bf16 q
    enc32 = R.sub_case(R.BY_NAME["enc-staged-f32"], (0,))
    enc16 = R.sub_case(R.BY_NAME["enc-dma"], (0,))
    d = R.inputs
    assert "fattn: row strides must be multiples of 4" in _refused(lib, pre, _widened(R.pack(pre, d(pre)), "out", "o_rs", 2))
    assert "fattn: row strides must be multiples of 4" in _refused(lib, pre, _widened(R.pack(pre, d(pre)), "q", "q_rs", 2))
    assert "fattn: bf16 q row stride must be a multiple of 8" in _refused(lib, pre16, _widened(R.pack(pre16, d(pre16)), "q", "q_rs", 4))
    assert "fattn: row strides must be multiples of 4" in _refused(lib, enc32, _widened(R.pack(enc32, d(enc32)), "out", "o_rs", 2))
    pk = R.pack(enc16, d(enc16))
    wide = _widened(pk, "q", "q_rs", 4)   # the one interleaved buffer: q, K and V rows get the same stride, kv_off of its one segment is 0
    assert "fattn: bf16 row strides must be multiples of 8" in _refused(lib, enc16, dict(wide, k=wide["q"], v=wide["q"], kv_rs=wide["q_rs"]))
    for c, msg in ((dict(pre, group=3, n_kv=1, sub_kv=None), "fattn: GQA group must be 1, 2 or 4"),
                   (dict(R.sub_case(R.BY_NAME["pre-valu-g1-bf16"], (1,)), group=3, n_kv=1, sub_kv=None), "attn: GQA group must be 1, 2 or 4")):
        pk = R.pack(dict(c, group=1, n_kv=2), d(c))   # two heads' room; three are named and refused before the bounds matter
        pk = _widened(_widened(pk, "q", "q_rs", 128), "out", "o_rs", 128)
        assert msg in _refused(lib, c, dict(pk, n_kv=1))


# ---- the knob forms: one fresh process each ----------------------------------------------------------------------------------------
_children = {}


def _child(tmp_path_factory, knob, value, names):
    """The DMA cases in a fresh interpreter with the knob set: name -> (raw output, form).  A child that ends on a signal or at its
    time limit ends the session: nothing more is started on a device that may have faulted."""
    if knob not in _children:
        out = str(tmp_path_factory.mktemp("seg_attn_" + knob) / "out.npz")
        env = {k: v for k, v in os.environ.items() if not k.startswith("Q3A_FATTN_")}
        env[knob] = value
        try:
            r = subprocess.run([sys.executable, os.path.join(HERE, "seg_attn_child.py"), out] + names, env=env, timeout=240, capture_output=True, text=True)
        except subprocess.TimeoutExpired:
            pytest.exit(f"stopping: the {knob}={value} child did not end within its time limit", returncode=3)
        if r.returncode < 0 or "HIP error" in r.stderr:
            pytest.exit(f"stopping: the {knob}={value} child ended with {r.returncode}: {r.stderr[-2000:]}", returncode=3)
        assert r.returncode == 0, r.stderr[-2000:]
        z = np.load(out)
        _children[knob] = {n: (z[n + "|out"], dict(zip(R.FORM_FIELDS, z[n + "|form"].tolist()))) for n in names}
    return _children[knob]


def test_a_ring_of_four_stages_gives_the_bits_of_three(lib, tmp_path_factory):
    """By reading, the ring depth changes no arithmetic: tile t lands in stage t % NS either way and is consumed in the same order."""
    res = _child(tmp_path_factory, "Q3A_FATTN_NS", "4", DMA_CASES)
    by_name = {c["name"]: c for c in ALL}
    for n in DMA_CASES:
        raw, form = res[n]
        want = dict(by_name[n]["form"], ns=4)
        assert {k: form[k] for k in want} == want, n
        mine, mform = _launch(lib, by_name[n])
        assert mform["ns"] == 3
        same = np.array_equal(raw, mine)
        print(f"{n}: NS = 4 " + ("reproduces the NS = 3 bits" if same else "differs from NS = 3"))
        assert same, n


def test_without_dma_the_staged_kernel_serves_q16(lib, tmp_path_factory):
    """Q3A_FATTN_DMA=0: the register-staged kernel with bf16 q (and, in the encoder, bf16 K/V) inside the float64 bounds -- and bit for
    bit what it computes from fp32 q (fp32 K/V) holding the same values in this process."""
    names = ["enc-dma", "pre-dma-g1", "pre-dma-g2", "pre-dma-g4"]
    res = _child(tmp_path_factory, "Q3A_FATTN_DMA", "0", names)
    for n in names:
        c = R.BY_NAME[n]
        raw, form = res[n]
        want = dict(c["form"], dma=0, ns=0)
        assert {k: form[k] for k in want} == want, n
        w = R.excess(c, R.inputs(c), R.decode(raw, False))
        print(f"{n} on the staged kernel with q16: at {w:.4f} of the bound")
        assert w <= 1.0, n
        twin = R.variant(c, q="f32x", kv="f32", form=dict(want, kv_f32=1)) if c["layout"] == "enc" else R.variant(c, q="f32x", form=want)
        assert np.array_equal(raw, _checked(lib, twin)), n
