"""Op-level veneer on the GPU at the shapes where its loops wrap: every kernel of csrc/k_ops.hip (and the engine's LayerNorm
behind q3a_op_layer_norm) against the float64 references and derived bounds of tests/ops_ref.py -- more than one tile and more
than one wave per row, K and row tails, the grid-stride step, both LayerNorm kernels around their boundary, NaN / inf / empty
inputs -- plus bit-identity between the forms that must agree exactly.  tests/test_ops_ref_host.py shows on the CPU that each
case accepts an honest fp32 implementation and rejects the listed mutants.  One test per kernel family; each prints its
figures before it asserts."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ops_ref as R
from qwen3_asr_rs_amd import tensor as T
from qwen3_asr_rs_amd.tensor import Tensor

pytestmark = pytest.mark.gpu


def dev(x):
    x = np.asarray(x)
    return Tensor.from_numpy(x.astype(np.float32) if x.dtype == np.float64 else x, 0)


def apply_dev(t, prog):
    for op in prog:
        k = op[0]
        if k == "tr": t = t.tr()
        elif k == "transpose": t = t.transpose(op[1], op[2])
        elif k == "permute": t = t.permute(list(op[1]))
        elif k == "narrow": t = t.narrow(op[1], op[2], op[3])
        elif k == "unsqueeze": t = t.unsqueeze(op[1])
        elif k == "expand": t = t.expand(list(op[1]))
        elif k == "select": t = t.select(op[1], op[2])
        elif k == "bf16": t = t.to_dtype(T.BF16)
        else: raise KeyError(k)
    return t


def indices(t):
    """An I64 index array as numpy int64 (through F32: exact below 2^24)."""
    return t.to_dtype(T.F32).numpy().astype(np.int64)


def check(c, got, exp=None):
    ref, bound = exp if exp is not None else R.expected(c)
    got = np.asarray(got)
    assert got.shape == ref.shape, (c["name"], got.shape, ref.shape)
    if bound is not None:
        e = R.excess(got, ref, bound)
        print(f"{c['family']}-{c['name']}: at {float(e.max()) if e.size else 0.0:.3f} of the bound")
    assert R.accepts(c, got, (ref, bound)), f"{c['family']}-{c['name']} outside its bound"


def same_bits(a: Tensor, b: Tensor):
    x, y = a.numpy(), b.numpy()
    return x.shape == y.shape and np.array_equal(x.view(np.uint32), y.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------
def test_matmul():
    for c in R.matmul_cases():
        got = apply_dev(dev(c["a"]), c["pa"]).matmul(apply_dev(dev(c["b"]), c["pb"])).numpy()
        check(c, got)
        if c["name"] == "5x3x0":
            assert got.shape == (5, 3) and not got.any()
    g = R.rng(21)
    r = lambda *s: R.f32(g.standard_normal(s))
    # the in-place [N][K] reader against the [K][N] reader: the same k-ordered fma chain, so the same bits
    for M, N, K in [(65, 63, 33), (129, 130, 70), (5, 130, 4321)]:
        x, w = dev(r(M, K)), dev(r(N, K))
        assert same_bits(x.matmul(w.tr()), x.matmul(w.tr().contiguous())), (M, N, K)
    # the same A row at row 0 and at row 67 of a taller A (another tile, another wave, another lane)
    row, b = r(1, 70), r(70, 45)
    tall = r(131, 70)
    tall[67] = row[0]
    B = dev(b)
    assert np.array_equal(dev(row).matmul(B).numpy()[0], dev(tall).matmul(B).numpy()[67])
    # K padded with zero columns up to the next multiple of 32: the tail tile's zero fill is the same as stored zeros
    a, b = r(66, 70), r(70, 67)
    ap, bp = np.zeros((66, 96), np.float32), np.zeros((96, 67), np.float32)
    ap[:, :70], bp[:70] = a, b
    assert same_bits(dev(a).matmul(dev(b)), dev(ap).matmul(dev(bp)))
    # a batched call against its per-batch 2-D calls
    a3, b3 = r(3, 66, 70), r(3, 70, 67)
    full = dev(a3).matmul(dev(b3)).numpy()
    for i in range(3):
        assert np.array_equal(full[i], dev(a3[i]).matmul(dev(b3[i])).numpy()), i


def test_conv2d():
    for c in R.conv_cases():
        x, w = dev(c["x"]), dev(c["w"])
        st, pd, dl = list(c["stride"]), list(c["padding"]), list(c["dilation"])
        got = x.conv2d(w, None if c["bias"] is None else dev(c["bias"]), st, pd, dl, 1).numpy()
        check(c, got)
        # without bias: bit-identical to the matmul of the host-built im2col matrix with weight.reshape(Co, -1).tr()
        plain = x.conv2d(w, None, st, pd, dl, 1).numpy()
        Co = c["w"].shape[0]
        mm = dev(R.im2col(c["x"], c["w"].shape, c["stride"], c["padding"], c["dilation"])).matmul(w.reshape([Co, -1]).tr()).numpy()
        N, _, OH, OW = plain.shape
        assert np.array_equal(plain, mm.reshape(N, OH, OW, Co).transpose(0, 3, 1, 2)), c["name"]
        if c["bias"] is not None:   # and the bias is one fp32 addition on top of that
            assert np.array_equal(got, plain + c["bias"][None, :, None, None]), c["name"]


def test_softmax():
    for c in R.softmax_cases():
        got = apply_dev(dev(c["x"]), c["px"]).softmax(c["dim"]).numpy()
        check(c, got)
        D = got.shape[c["dim"]]
        s = got.astype(np.float64).sum(c["dim"])
        ok = ~np.isnan(s)
        assert ok.any() and np.abs(s[ok] - 1.0).max() <= D * R.U, (c["name"], np.abs(s[ok] - 1.0).max() / R.U)
        if c["name"] == "all_masked_row":
            assert np.isnan(got[1]).all() and not np.isnan(got[[0, 2]]).any()


def test_mean_dim():
    for c in R.mean_cases():
        check(c, apply_dev(dev(c["x"]), c["px"]).mean_dim(list(c["dims"]), c["keepdim"]).numpy())


def test_layer_norm():
    for c in R.layer_norm_cases():
        D = c["x"].shape[-1]
        got = dev(c["x"]).layer_norm([D], None if c["w"] is None else dev(c["w"]), None if c["b"] is None else dev(c["b"]), R.LN_EPS).numpy()
        check(c, got)
    # D = 2048 through both kernels: the engine's (weight and bias given) and the generic one (no bias; the bias added afterwards --
    # the same final fp32 addition).  Each is within the bound of the reference, so they agree within the sum of their bounds.
    for c in R.layer_norm_cases():
        if c["name"] in ("5x2048_both", "9x2048_both", "5x2048_both_offset100"):
            x, w, b = dev(c["x"]), dev(c["w"]), dev(c["b"])
            eng = x.layer_norm([2048], w, b, R.LN_EPS).numpy()
            gen = (x.layer_norm([2048], w, None, R.LN_EPS) + b).numpy()
            ref, bound = R.expected(c)
            check(c, gen, (ref, bound))
            e = R.excess(eng, gen, 2.0 * bound)
            print(f"layer_norm-{c['name']}: engine vs generic kernel at {e.max():.3f} of the summed bounds")
            assert e.max() <= 1.0


def test_argmax_and_max():
    for c in R.argmax_cases():
        x = dev(c["x"])
        got = indices(x.argmax(c["dim"], c["keepdim"]))
        ref, _ = R.expected(c)
        bad = np.argwhere(got != ref)[:5].tolist() if got.shape == ref.shape else "shape"
        assert got.shape == ref.shape and np.array_equal(got, ref), (c["name"], bad, [c["tags"][i[0]] for i in bad] if c["tags"] and bad != "shape" else None)
        if c["tags"]:   # max of each row as its own array: the same kernel over one row of D
            for i, tag in enumerate(c["tags"]):
                v, want = x.get(i).max().f64_value([]), R.max_ref(c["x"][i])
                assert (np.isnan(v) and np.isnan(want)) or v == float(want), (c["name"], tag, v, want)
    lg = R.argmax_cases()[-3]
    assert lg["name"] == "logits_151936" and dev(lg["x"]).max().f64_value([]) == 9.0     # a global max over 303 872 elements: one row, 1187 strides


def test_stft_and_reflection_pad():
    for c in R.stft_cases():
        x, win = dev(c["x"]), dev(c["win"])
        ref, bound = R.expected(c)
        real = x.stft(c["n_fft"], c["hop"], c["n_fft"], win, c["normalized"], c["onesided"], False)
        assert real.kind() == T.F32
        check(c, real.numpy(), (ref, bound))
        cplx = x.stft(c["n_fft"], c["hop"], c["n_fft"], win, c["normalized"], c["onesided"], True)
        assert cplx.kind() == T.C64 and cplx.size() == list(ref.shape[:2])
        mag = cplx.abs().numpy()     # the complex form holds the same numbers: |z| = hypot(re, im) of them
        want = np.hypot(real.numpy()[..., 0].astype(np.float64), real.numpy()[..., 1].astype(np.float64))
        assert np.abs(mag - want).max() <= 4 * R.U * max(want.max(), 1e-30)
    # a frame that does not fit one workgroup's LDS is refused on the host: no table is built, nothing is launched
    n = 1 << 20
    with pytest.raises(T.OpsError, match="LDS"):
        Tensor.zeros([n]).stft(n, n, n, Tensor.ones([n]), False, True, True)
    for c in R.reflect_pad_cases():
        check(c, dev(c["x"]).reflection_pad1d(list(c["pad"])).numpy())


def test_elementwise_views_dtypes():
    # ---- one array with more elements than a launch has threads: the grid-stride step of every kernel that has one
    x = R.big_array()
    refs, row, col = R.big_refs(x)
    X = dev(x)
    got = {"neg": X.neg(), "add_row": X + dev(row), "add_col": X + dev(col), "transpose_contiguous": X.transpose(0, 1).contiguous(),
           "triu1": X.triu(1), "bf16_round_trip": X.to_dtype(T.BF16).to_dtype(T.F32), "cat_self": Tensor.cat([X, X], 0)}
    Z = Tensor.zeros(list(R.BIG_SHAPE))
    Z.fill_(1.25)
    got["fill"] = Z
    for name, ref in refs.items():
        assert R.bits_equal(got[name].numpy(), ref), name
    emb = R.f32(R.rng(31).standard_normal((50, 1024)))
    idx = R.rng(32).integers(0, 50, (3, 1400)).astype(np.int64)        # 4 300 800 output elements
    idx[0, 0], idx[-1, -1] = 49, 0
    assert R.bits_equal(Tensor.embedding(dev(emb), dev(idx)).numpy(), emb[idx])
    assert R.bits_equal(Tensor.stack([dev(row), dev(row * 2)], 1).numpy(), np.stack([row, row * 2], 1))
    # ---- an 8-D permuted and expanded view through contiguous
    b8 = R.f32(R.rng(33).standard_normal((2, 1, 3, 1, 2, 3, 1, 2)))
    perm = (7, 2, 0, 5, 1, 4, 3, 6)
    v = dev(b8).expand([2, 3, 3, 2, 2, 3, 1, 2]).permute(list(perm))
    assert R.bits_equal(v.contiguous().numpy(), np.ascontiguousarray(np.broadcast_to(b8, (2, 3, 3, 2, 2, 3, 1, 2)).transpose(perm)))
    # ---- slice_scatter: step 3, negative start / end, a src of another dtype
    a = R.f32(R.rng(34).standard_normal((4, 20)))
    src = R.rng(35).integers(-9, 9, (4, 5)).astype(np.int64)
    want = a.copy()
    want[:, 3:18:3] = src
    assert R.bits_equal(dev(a).slice_scatter(dev(src), 1, -17, -2, 3).numpy(), want)
    want = a.copy()
    want[1:4:2] = a[:2] * 2
    assert R.bits_equal(dev(a).slice_scatter(dev(a[:2] * 2), 0, 1, 20, 2).numpy(), want)
    # ---- I64 values near 2^62 through cat / narrow / select, read back exactly
    big = (2 ** 62 + np.arange(12, dtype=np.int64).reshape(3, 4) * 3 + 1) * np.array([[1], [-1], [1]], np.int64)
    B = dev(big)
    cat = Tensor.cat([B, B.narrow(0, 1, 2)], 0)
    wantc = np.concatenate([big, big[1:3]], 0)
    assert cat.kind() == T.I64 and cat.size() == [5, 4]
    for i in range(5):
        for j in range(4):
            assert cat.int64_value([i, j]) == int(wantc[i, j]), (i, j)
    assert cat.select(1, 3).narrow(0, 3, 2).int64_value([1]) == int(wantc[4, 3]) and cat.transpose(0, 1).contiguous().int64_value([2, 4]) == int(wantc[4, 2])
    # ---- conversions at special values: equal to torch's
    cx = R.conversion_inputs()
    CX = dev(cx)
    for dt in (R.BF16, R.F16, R.BOOL):
        back = CX.to_dtype(dt).to_dtype(T.F32).numpy()
        assert R.bits_equal(back, R.convert_ref(cx, dt)), (dt, cx[back.view(np.uint32) != R.convert_ref(cx, dt).view(np.uint32)][:8])
    for dt in (R.I64, R.I32):
        ok = R.convertible(cx, dt)
        sub = cx[ok]
        conv = dev(sub).to_dtype(dt)
        assert conv.kind() == dt
        want = R.convert_ref(sub, dt)
        assert np.array_equal(conv.to_dtype(T.F32).numpy().astype(np.float64), want.astype(np.float64)), dt
        for i in (int(np.argmax(sub == np.float32(-0.75))), int(np.argmax(sub == np.float32(-2.5))), int(np.argmax(sub == np.float32(0.999)))):
            assert conv.int64_value([i]) == int(want[i]) == int(np.trunc(sub[i]))


def _special(name, got, x, torch_out):
    """The NaN / +-inf / signed-zero pattern of torch's float32 op; its finite non-zero results within the function's ULP gate of
    the float64 reference."""
    want = torch_out.numpy()
    assert R.special_pattern_equal(got, want), (name, x.tolist(), got.tolist(), want.tolist())
    m = np.isfinite(want) & (want != 0)
    if name in R.UNARY_REF and m.any():
        ref = R.unary_ref(name, x[m])
        assert (R.ulp_error(got[m], ref) <= R.ULP_GATE[name]).all(), (name, x[m].tolist(), got[m].tolist(), ref.tolist())
    elif m.any():
        assert R.bits_equal(got[m], want[m]), (name, got.tolist(), want.tolist())      # one IEEE operation: equal


def test_unary_ulp_and_special_values():
    worst = {}
    for name in sorted(R.UNARY_REF):
        x = R.unary_sweep(name)
        X = dev(x)
        got = (X.pow_scalar(R.POW_E) if name == "pow" else getattr(X, name)()).numpy()
        ref = R.unary_ref(name, x)
        e = np.where(R.gate_domain(name, x), R.ulp_error(got, ref), 0.0)
        worst[name] = (float(e.max()), float(x[e.argmax()]), float(e[np.abs(x) > 4.0].max()))
        print(f"ULP {name}: worst {worst[name][0]:.3f} at x = {worst[name][1]!r}; beyond |x| = 4: {worst[name][2]:.3f}; gate {R.ULP_GATE[name]}")
    for name in sorted(R.UNARY_REF):
        assert R.ULP_GATE[name] is not None, f"{name}: no gate measured yet"
        x = R.unary_sweep(name)
        X = dev(x)
        got = (X.pow_scalar(R.POW_E) if name == "pow" else getattr(X, name)()).numpy()
        ref = R.unary_ref(name, x)
        assert R.inside(got, ref, R.unary_bound(name, x, ref)), (name, worst[name])
    nan, inf = np.nan, np.inf
    t = lambda a: torch.from_numpy(R.f32(a))
    for name, vals in [("rsqrt", [0.0, 4.0, 1e-30, inf, -1.0]), ("log10", [0.0, 1.0, 1e-30, inf, -1.0]), ("sqrt", [-1.0, 0.0, -0.0, 4.0, inf]),
                       ("exp", [89.0, -89.0, -104.0, 0.0, -inf, nan]), ("silu", [-100.0, 100.0, 0.0, -0.0, -20.0]), ("gelu", [10.0, -10.0, 0.0, -0.0, 3.0]),
                       ("sin", [0.0, -0.0, inf, 1.0]), ("cos", [0.0, inf, nan, 1.0])]:
        x = R.f32(vals)
        got = getattr(dev(x), name)().numpy()
        print(f"special {name}: {x.tolist()} -> {got.tolist()} (torch {R.UNARY_TORCH[name](t(x)).tolist()})")
        _special(name, got, x, R.UNARY_TORCH[name](t(x)))
    base = R.f32([-2.0, -0.5, -0.0, 0.0, 2.0, -inf])
    for e in (2.0, 3.0, 0.5, -0.5, -1.0, -2.0, 0.0, 1.5, -1.5):   # (the first six are not pow() in ATen: x * x, sqrt, reciprocal ...)
        got = dev(base).pow_scalar(e).numpy()
        want = t(base).pow(e)
        assert R.special_pattern_equal(got, want.numpy()), (e, got.tolist(), want.tolist())
        m = np.isfinite(want.numpy()) & (want.numpy() != 0)
        ref = np.power(base[m].astype(np.float64), e)
        assert (R.ulp_error(got[m], ref) <= R.ULP_GATE["pow"]).all(), (e, got.tolist(), want.tolist())
    x = R.f32([nan, 1.0, -1.0, inf, -inf, 0.25])
    _special("clamp_min", dev(x).clamp_min(0.5).numpy(), x, t(x).clamp_min(0.5))
    _special("clamp_min_nan", dev(x).clamp_min(nan).numpy(), x, t(x).clamp_min(nan))
    a, b = R.f32([nan, 1.0, nan, -inf, 2.0, -3.0]), R.f32([1.0, nan, nan, inf, -2.0, -1.0])
    _special("maximum", dev(a).maximum(dev(b)).numpy(), a, torch.maximum(t(a), t(b)))
    a, b = R.f32([1.0, -1.0, 0.0, nan, 5.0, -5.0, 6.0]), R.f32([0.0, 0.0, 0.0, 1.0, -0.0, -0.0, 3.0])
    _special("div", (dev(a) / dev(b)).numpy(), a, t(a) / t(b))
    _special("div_scalar", (dev(a) / 0.0).numpy(), a, t(a) / 0.0)


def test_zero_element_arrays():
    """The right shape and no error from every family."""
    E = Tensor.zeros([0, 5])
    assert E.exp().size() == [0, 5] and E.neg().size() == [0, 5] and (E + Tensor.ones([5])).size() == [0, 5] and (E * 2.0).size() == [0, 5]
    assert E.maximum(E).size() == [0, 5] and E.clamp_min(0.0).size() == [0, 5]
    assert E.matmul(Tensor.ones([5, 3])).size() == [0, 3] and Tensor.ones([3, 5]).matmul(Tensor.zeros([5, 0])).size() == [3, 0]
    z = Tensor.ones([3, 0]).matmul(Tensor.ones([0, 4]))
    assert z.size() == [3, 4] and not z.numpy().any()
    assert E.softmax(-1).size() == [0, 5] and E.softmax(0).size() == [0, 5] and Tensor.zeros([3, 0]).softmax(-1).size() == [3, 0]
    assert E.mean_dim([-1], False).size() == [0] and E.mean_dim([-1], True).size() == [0, 1]
    m = Tensor.zeros([3, 0]).mean_dim([-1], False)           # the mean of nothing: NaN, as torch
    assert m.size() == [3] and np.isnan(m.numpy()).all()
    assert E.layer_norm([5], Tensor.ones([5]), Tensor.ones([5]), 1e-5).size() == [0, 5] and E.layer_norm([5], None, None, 1e-5).size() == [0, 5]
    assert E.argmax(-1, False).size() == [0] and E.argmax(-1, True).size() == [0, 1]
    assert Tensor.zeros([0, 3, 3]).triu(1).size() == [0, 3, 3]
    assert Tensor.cat([E, Tensor.ones([2, 5])], 0).numpy().tolist() == [[1.0] * 5] * 2 and Tensor.stack([E, E], 0).size() == [2, 0, 5]
    assert E.transpose(0, 1).contiguous().size() == [5, 0] and E.to_dtype(T.BF16).to_dtype(T.F32).size() == [0, 5]
    assert Tensor.ones([4, 5]).slice_scatter(Tensor.zeros([0, 5]), 0, 2, 2, 1).numpy().tolist() == [[1.0] * 5] * 4
    assert Tensor.zeros([0, 10]).reflection_pad1d([2, 3]).size() == [0, 15]
    assert Tensor.zeros([0, 3, 5, 5]).conv2d(Tensor.ones([4, 3, 3, 3]), Tensor.ones([4]), [1, 1], [1, 1], [1, 1], 1).size() == [0, 4, 5, 5]
    assert Tensor.embedding(Tensor.ones([7, 4]), Tensor.zeros([0, 2], T.I64)).size() == [0, 2, 4]
    E.fill_(1.0)
    assert E.numpy().shape == (0, 5) and Tensor.arange(3, 3).size() == [0]
