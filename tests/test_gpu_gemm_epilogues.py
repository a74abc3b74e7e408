"""The GEMM family on the GPU against float64, per element: every epilogue form of csrc/k_gemm.hip, k_gemm16.hip and k_gemm256.hip on every
tile form its launcher picks, the three implicit-GEMM convolution loaders, gemm256's wave-quantisation split, and QK-norm + RoPE + KV-cache
append fused and separate -- the cases, references and derived bounds of tests/gemm_ref.py, one launch each through
q3a_selftest_gemm_launch / q3a_selftest_qkrope_launch.  Every element of every output buffer is compared: inside the bound where the
launch must write, bit for bit the initial content (a sentinel, or the residual) everywhere else.  tests/test_gemm_ref_host.py shows on
the CPU that each case accepts an honest fp32 evaluation and rejects the listed mutants.  Each test prints its figure before it asserts;
the last one prints the worst excess per family."""
import ctypes as C

import numpy as np
import pytest

import gemm_ref as G

pytestmark = pytest.mark.gpu

DEFAULT_KNOBS = dict(gemm256_min_tiles=128, gemm256_persist=1, gemm256_group_m=0)
LAUNCHER = {"gemm": 0, "gemm16": 1, "gemm16_small": 2, "conv": 3, "conv16": 4}
WORST = {}


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _knobs(lib, **kw):
    for k, v in kw.items():
        assert lib.q3a_debug_set(k.encode(), int(v)) == 0, k


def _ok(lib, rc):
    """A refusal fails the test; a HIP error ends the session -- nothing more is launched on a device that has faulted."""
    if rc != 0:
        msg = (lib.q3a_last_error(None) or b"").decode()
        if "HIP error" in msg:
            pytest.exit(f"stopping: {msg}", returncode=3)
        pytest.fail(msg)


def _check(tag, name, raw, init, exp, out16):
    ref, written, bound = exp
    full = G.decode(raw, out16)
    w = G.worst_excess(full, exp)
    print(f"{name}: at {w:.3f} of the bound")
    tag = f"{tag}, {'bf16' if out16 else 'fp32'} out"   # (a bf16 result sits within half an ulp by construction: its figure is near 1)
    WORST[tag] = max(WORST.get(tag, 0.0), w)
    assert np.array_equal(raw[~written], init[~written]), f"{name}: an element outside the rows and columns the epilogue names was written"
    assert G.accepts(full, exp), f"{name} outside its bound"


def _cases(family, pred):
    return [c for c in G.FAMILIES[family]() if pred(c)]


def _ids(cases):
    return [c["name"] for c in cases]


def run_gemm_case(lib, tag, c):
    d = G.materialize(c)
    exp = G.evaluate(c, d)
    conv = c["family"] == "conv"
    x = d["x"] if conv else d["x_strided"]
    x = np.ascontiguousarray(x if c["launcher"] in ("gemm", "conv") else G.bf16_bits(x))
    w = np.ascontiguousarray(G.bf16_bits(d["w"]))
    inplace = c["resid"] == "inplace"
    flags = int(c["split"]) | (2 if c["glu"] else 0) | (4 if c["out16"] else 0) | (8 if inplace else 0)
    raw = d["init"].copy()
    resid = None if inplace else d["resid"]
    geo = (c["imgs"], c["H"], c["W"], c["C"]) if conv else (0, 0, 0, 0)
    try:
        _knobs(lib, **c["knobs"])
        rc = lib.q3a_selftest_gemm_launch(0, LAUNCHER[c["launcher"]], flags, _ptr(x), _ptr(w), c["M"], c["N"], c["K"], c["lda"], c["ldo"], *geo,
                                          _ptr(d["bias"]), _ptr(d["addend"]), max(c["addend"], 1), _ptr(resid), _ptr(d["rowmap"]), c["act"],
                                          _ptr(raw), d["rows"])
    finally:
        _knobs(lib, **DEFAULT_KNOBS)
    _ok(lib, rc)
    _check(tag, c["name"], raw, d["init"], exp, c["out16"])


GEMM = _cases("dense", lambda c: c["launcher"] == "gemm")
GEMM16 = _cases("dense", lambda c: c["group"].startswith("gemm16-"))
GEMM256 = _cases("dense", lambda c: c["form"] == "gemm256")
SPLIT_TAIL = _cases("dense", lambda c: c["form"] == "gemm256+tail")
CONV = _cases("conv", lambda c: c["launcher"] == "conv")
CONV16 = _cases("conv", lambda c: c["group"] == "conv16-tiles")
CONV256 = _cases("conv", lambda c: c["group"].startswith("conv256"))
QK = G.qk_cases()
QK_FUSED = [c for c in QK if c["fused"] and not c["split_rows"]]
QK_SEPARATE = [c for c in QK if not c["fused"]]
QK_SPLIT = [c for c in QK if c["split_rows"]]
assert len(GEMM) + len(GEMM16) + len(GEMM256) + len(SPLIT_TAIL) == len(G.dense_cases()) and len(CONV) + len(CONV16) + len(CONV256) == len(G.conv_cases())
assert len(QK_FUSED) + len(QK_SEPARATE) + len(QK_SPLIT) == len(QK)


@pytest.mark.parametrize("c", GEMM, ids=_ids(GEMM))
def test_launch_gemm(lib, c):
    run_gemm_case(lib, "dense: launch_gemm (fp32 x, split 0 / 1)", c)


@pytest.mark.parametrize("c", GEMM16, ids=_ids(GEMM16))
def test_gemm16_small_tiles(lib, c):
    run_gemm_case(lib, "dense: launch_gemm16_small, every tile form", c)


@pytest.mark.parametrize("c", GEMM256, ids=_ids(GEMM256))
def test_gemm256(lib, c):
    run_gemm_case(lib, "dense: launch_gemm256, persist 0 / 1 / 2", c)


@pytest.mark.parametrize("c", SPLIT_TAIL, ids=_ids(SPLIT_TAIL))
def test_gemm256_split_tail(lib, c):
    assert lib.q3a_gemm256_split_rows(c["M"], c["N"]) == c["split_rows"] == 65536
    run_gemm_case(lib, "dense: launch_gemm256 + split tail", c)


@pytest.mark.parametrize("c", CONV, ids=_ids(CONV))
def test_conv_gemm(lib, c):
    run_gemm_case(lib, "conv: launch_conv3x3s2_gemm (ConvA, split 0 / 1)", c)


@pytest.mark.parametrize("c", CONV16, ids=_ids(CONV16))
def test_conv_gemm16_tiles(lib, c):
    run_gemm_case(lib, "conv: launch_conv3x3s2_gemm16 small tiles (ConvA16)", c)


@pytest.mark.parametrize("c", CONV256, ids=_ids(CONV256))
def test_conv_gemm256(lib, c):
    run_gemm_case(lib, "conv: launch_conv3x3s2_gemm256 (ConvA256)", c)


def run_qk_case(lib, tag, c):
    d = G.qk_materialize(c)
    exp = G.qk_evaluate(c, d)
    M, N, S, n_kv, max_ctx = c["M"], c["N"], c["n_seq"], c["n_kv"], d["max_ctx"]
    kv16 = not c["kv_f32"]
    bufs, inits = {}, {}
    inits["kcache"] = np.full((S, n_kv, max_ctx, 128), G.SENT16 if kv16 else G.SENT32, np.uint16 if kv16 else np.uint32)
    inits["vcache"] = inits["kcache"].copy()
    if c["q16"]: inits["q16"] = np.full((M, c["n_q"] * 128), G.SENT16, np.uint16)
    if not c["fused"]: inits["qkv"] = np.ascontiguousarray(d["qkv"]).view(np.uint32).copy()
    elif c["scratch"]: inits["qkv"] = np.full((M, N), G.SENT32, np.uint32)
    bufs = {k: v.copy() for k, v in inits.items()}
    x = w = None
    if c["fused"]:
        x, w = np.ascontiguousarray(G.bf16_bits(d["x"])), np.ascontiguousarray(G.bf16_bits(d["w"]))
    try:
        _knobs(lib, **c["knobs"])
        rc = lib.q3a_selftest_qkrope_launch(0, int(c["fused"]), int(c["kv_f32"]), _ptr(x), c["K"], _ptr(w), M, c["K"], _ptr(d.get("bias")),
                                            _ptr(bufs.get("qkv")), _ptr(d["row_seq"]), _ptr(d["row_pos"]), _ptr(d["q_norm"]), _ptr(d["k_norm"]),
                                            G.QK_EPS, _ptr(d["cos"]), _ptr(d["sin"]), max_ctx, c["n_q"], n_kv, S, max_ctx, _ptr(bufs.get("q16")),
                                            _ptr(bufs["kcache"]), _ptr(bufs["vcache"]))
    finally:
        _knobs(lib, **DEFAULT_KNOBS)
    _ok(lib, rc)
    assert set(exp) == set(bufs)
    for k in sorted(exp):
        _check(tag, f"{c['name']}[{k}]", bufs[k], inits[k], exp[k], bufs[k].dtype == np.uint16)


@pytest.mark.parametrize("c", QK_FUSED, ids=_ids(QK_FUSED))
def test_qkrope_fused(lib, c):
    run_qk_case(lib, "qk: launch_gemm256_qkrope", c)


@pytest.mark.parametrize("c", QK_SEPARATE, ids=_ids(QK_SEPARATE))
def test_qkrope_separate(lib, c):
    run_qk_case(lib, "qk: launch_qknorm_rope_kv", c)


@pytest.mark.parametrize("c", QK_SPLIT, ids=_ids(QK_SPLIT))
def test_qkrope_fused_split(lib, c):
    assert lib.q3a_gemm256_split_rows(c["M"], c["N"]) == c["split_rows"] == 32768
    run_qk_case(lib, "qk: launch_gemm256_qkrope + split tail", c)


def test_fast_activations_alone(lib):
    """gelu_fast and silu_fast at inputs known exactly: X has the bf16 value x_m in column 0 and 1 in column 1, W picks one of them, so the
    accumulator is x_m (or 1) without a rounding and the epilogue's fl(x_m + bias_n) is the fp32 sum numpy forms too.  What is left is the
    activation's own error: GELU against its gate, SiLU (through the GLU pair, up = 1) against its derived bound."""
    g = G.rng_of("activation sweep")
    M, N, K = 512, 256, 32
    X = np.zeros((M, K), np.float32)
    X[:, 0], X[:, 1] = G.bf16_round(np.linspace(-12.0, 12.0, M)), 1.0
    x16 = np.ascontiguousarray(G.bf16_bits(X))
    for name, glu in (("gelu_fast", 0), ("silu_fast", 1)):
        Wm = np.zeros((N, K), np.float32)
        bias = G.f32(g.uniform(-0.05, 0.05, N))
        gate = np.ones(N, bool)
        if glu:
            gate = (np.arange(N) % 32) < 16
            bias[~gate] = 0.0
        Wm[gate, 0], Wm[~gate, 1] = 1.0, 1.0
        ncols = N // 2 if glu else N
        raw = np.full((M, ncols), G.SENT32, np.uint32)
        w16 = np.ascontiguousarray(G.bf16_bits(Wm))
        _ok(lib, lib.q3a_selftest_gemm_launch(0, LAUNCHER["gemm16_small"], 2 if glu else 0, _ptr(x16), _ptr(w16), M, N, K, K, ncols, 0, 0, 0, 0,
                                              _ptr(bias), None, 1, None, None, 0 if glu else 1, _ptr(raw), M))
        v = (X[:, :1] + bias[None, gate]).astype(np.float64)   # fp32 sum, exactly the kernel's
        got = raw.view(np.float32).astype(np.float64)
        assert np.isfinite(got).all()
        if glu:
            ref, b = G.silu_step(v, 0.0, True)
            rel = np.abs(got - ref) / np.maximum(np.abs(ref), 2.0 ** -126) / G.U
            print(f"silu_fast on the device: worst relative error {rel.max():.2f} u at x = {v.reshape(-1)[rel.argmax()]:.4f}; {(np.abs(got - ref) / b).max():.3f} of the bound")
        else:
            ref, b = G.gelu_step(v, 0.0, True)
            rel = np.abs(got - ref) / np.maximum(1.0, np.abs(v))
            print(f"gelu_fast on the device: worst error {rel.max():.3e} max(1, |x|) at x = {v.reshape(-1)[rel.argmax()]:.4f}; gate {2 * G.GELU_FAST_WORST:.2e}")
        e = np.abs(got - ref) / b
        WORST[f"{name} alone (device, exact inputs)"] = float(e.max())
        assert (e <= 1.0).all(), f"{name} outside its bound: {e.max():.3f}"


def test_worst_excess_per_family():
    """The figures of tests/gemm_ref.py's header table (the families that ran in this session)."""
    for tag in sorted(WORST):
        print(f"{tag:60s} {WORST[tag]:.3f}")
    assert all(v <= 1.0 for v in WORST.values())
