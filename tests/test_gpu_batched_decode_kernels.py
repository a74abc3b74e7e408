"""The batched decode step's kernels on the GPU against float64, per element: launch_skinny in every form its launcher picks (the case
table of tests/batched_decode_ref.py: one launch per case through q3a_selftest_skinny_launch, the reported instantiation compared with
the form the case states), launch_decode_attn_batched at the tile edges, and launch_decode_attn at S > 1 with launch_attn_combine behind
it (q3a_selftest_batched_attn_launch).  Next to the float64 checks stand the relations that must hold bit for bit: half-pair against
pair tiles, quarter against full workgroups, row-major against fragment-order activations, a sequence's row whatever S is and wherever
it sits.  Output buffers go in filled with a sentinel and come back whole; every input slot of a sequence >= S holds NaN.  Each test
prints its figure before it asserts.  tests/test_batched_decode_ref_host.py shows on the CPU what these checks would catch."""
import numpy as np
import pytest

import batched_decode_ref as R
from test_gpu_decode_kernels import _ok, _ptr

pytestmark = pytest.mark.gpu

FORM_FIELDS = ("split", "tiles", "sh", "xmode", "unr", "wlds", "qs", "palias", "hp", "grid", "dyn_lds")


def _launch(lib, c, d):
    """One launch of the case on data d: (the packed buffers with the outputs written, the reported form)."""
    pk = {k: np.ascontiguousarray(v) for k, v in R.pack(c, d).items()}
    w = np.ascontiguousarray(R.bf16_bits(d["W"]))
    form = np.full(11, -1, np.int32)
    flags = 1 * c["split"] | 2 * c["fast"] | 4 * c["qsplit"] | 8 * c["inplace"]
    g = lambda k: _ptr(pk.get(k))
    _ok(lib, lib.q3a_selftest_skinny_launch(0, _ptr(w), c["N"], c["K"], c["S"], g("x"), R.ldx_of(c), g("rms_w"), g("x16"), int(c["x"] == "x16frag"),
                                            g("xw16f"), g("ss_parts"), c["ss_nparts"] if c["x"] == "pre" else 0, R.EPS, g("bias"), c["mode"], g("resid"),
                                            g("out"), g("out16"), int(c["out"] == "bf16frag"), R.ldo_of(c), g("next_w"), g("next_xw16f"), g("next_ss"),
                                            flags, c["glu_hp3"], c["n_cu"], _ptr(form)))
    return pk, dict(zip(FORM_FIELDS, form.tolist()))


def _checked(lib, c, d):
    """Launch, compare every output buffer with float64, print, assert; returns the packed buffers."""
    pk, form = _launch(lib, c, d)
    by = R.skinny_excess_by_buffer(c, d, R.decode_outputs(c, pk))
    print(f"{c['name']}: at " + ", ".join(f"{k} {v:.4f}" for k, v in by.items()) + f" of the bound, form {form}")
    assert max(by.values()) <= 1.0
    return pk, form


def _variant(c, **kw):
    return dict(c, name=c["name"] + "/" + ",".join(f"{k}={v}" for k, v in kw.items()), **kw)


@pytest.mark.parametrize("c", R.SKINNY_CASES, ids=[c["name"] for c in R.SKINNY_CASES])
def test_skinny_forms(lib, c):
    _, form = _checked(lib, c, R.skinny_inputs(c))
    want = {k: v for k, v in c["form"].items() if k != "kind"}
    assert {k: form[k] for k in want} == want


@pytest.mark.parametrize("name", ["12-hp3-one-pass-s21", "12-hp3-one-pass-s9", "12-hp3-bias-f32-out", "13-hp3-two-passes-s9", "13-hp3-two-passes-s21",
                                  "14-hp3-balances-ncu5"])
def test_half_pair_tiles_equal_pair_tiles_bit_for_bit(lib, name):
    """Same K slices, same reduction order per output element (k_skinny.hip): the half-pair form against whichever pair form serves the
    shape with glu_hp3 = 0, on the same data."""
    c = R.SKINNY_BY_NAME[name]
    d = R.skinny_inputs(c)
    hp, form = _checked(lib, c, d)
    pair, pform = _checked(lib, _variant(c, glu_hp3=0), d)
    assert form["hp"] == 1 and pform["hp"] == 0 and pform["tiles"] == 2
    key = "out" if c["out"] == "f32" else "out16"
    assert np.array_equal(hp[key], pair[key])


@pytest.mark.parametrize("c", [c for c in R.SKINNY_CASES if c["qsplit"]], ids=[c["name"] for c in R.SKINNY_CASES if c["qsplit"]])
def test_quarter_workgroups_equal_full_workgroups_bit_for_bit(lib, c):
    d = R.skinny_inputs(c)
    qs, form = _checked(lib, c, d)
    full_c = _variant(c, qsplit=False)
    full, fform = _checked(lib, full_c, d)
    assert form["qs"] == 1 and fform["qs"] == 0
    assert np.array_equal(qs["out"], full["out"]) and np.array_equal(qs["next_xw16f"], full["next_xw16f"])
    # N / 8 partial rows against N / 16: the two sums per sequence agree within their bounds
    out = R.decode_outputs(c, qs)["out"]
    S = c["S"]
    (rq, bq), (rf, bf) = R.next_reference(c, d, out)["next_ss"], R.next_reference(full_c, d, out)["next_ss"]
    sq, sf = R.decode(qs["next_ss"], False)[:, :S].sum(axis=0), R.decode(full["next_ss"], False)[:, :S].sum(axis=0)
    gap = np.abs(sq - sf) / (bq[:, :S].sum(axis=0) + bf[:, :S].sum(axis=0))
    print(f"{c['name']}: sums of squares {gap.max():.4f} of their joint bound apart")
    assert gap.max() <= 1.0


def test_row_major_and_fragment_order_x_give_the_same_bits(lib):
    a, b = R.SKINNY_BY_NAME["07-direct-unr8-x16-rowmajor"], R.SKINNY_BY_NAME["07-direct-unr8-x16-frag"]
    d = R.skinny_inputs(a)
    assert np.array_equal(_checked(lib, a, d)[0]["out"], _checked(lib, b, d)[0]["out"])


@pytest.mark.parametrize("name", ["01-wlds-norm-bias-s5", "17-pre-nparts64-s9"])
def test_a_sequence_does_not_depend_on_s_or_its_neighbours(lib, name):
    """Row 3 of an S = 5 call, of the S = 21 call on the same data, and the same row placed at s = 19 (the other sequence half, the same
    lanes): the same bits."""
    c = R.SKINNY_BY_NAME[name]
    d = R.skinny_inputs(c)
    c5, c21 = _variant(c, S=5), _variant(c, S=21)
    moved = dict(d, x=d["x"].copy())
    moved["x"][19] = d["x"][3]
    r5, r21, r19 = (_checked(lib, cc, dd)[0]["out"] for cc, dd in ((c5, d), (c21, d), (c21, moved)))
    assert np.array_equal(r5[3], r21[3]) and np.array_equal(r5[3], r19[19])
    assert np.array_equal(r5[:5], r21[:5])


@pytest.mark.parametrize("qsplit", [False, True], ids=["full-workgroups", "quarter-workgroups"])
def test_hand_over_chain(lib, qsplit):
    """A mode-1 launch with next_w writes (out, next_xw16f, next_ss); those buffers go unchanged into a mode-0 pre-normalised launch,
    whose output is compared with the float64 RMSNorm + GEMM of `out` -- and with the fp32-x + rms_w launch on `out`: the same operand,
    another order of the sum of squares, so the two agree within the sum of their bounds."""
    S, H = 21, 512
    prod = R._c("chain-producer", 512, H, S, 1, "x16frag", None, qsplit=qsplit, bias=True, next=True, inplace=True)
    d = R.skinny_inputs(prod)
    pk, form = _checked(lib, prod, d)
    assert form["qs"] == int(qsplit)
    out = R.decode_outputs(prod, pk)["out"]
    rows = R.ss_rows_of(prod)
    cons = R._c("chain-consumer", H, 70, S, 0, "pre", None, ss_nparts=rows)
    d2 = R.skinny_inputs(cons)
    d2["x"] = np.zeros((32, H), np.float32)
    d2["x"][:S] = out[:S, :H].astype(np.float32)
    d2["g"] = d["next_w"]
    mine = R.pack(cons, d2)
    live = R.frag_index(np.arange(S)[:, None], np.arange(H)[None, :])
    assert np.array_equal(mine["xw16f"][live], pk["next_xw16f"][live])   # one IEEE multiply, one rounding: the producer's bits
    w = np.ascontiguousarray(R.bf16_bits(d2["W"]))
    form_c, o = np.zeros(11, np.int32), np.ascontiguousarray(mine["out"])
    xw, ss = np.ascontiguousarray(pk["next_xw16f"]), np.ascontiguousarray(pk["next_ss"].view(np.float32))
    _ok(lib, lib.q3a_selftest_skinny_launch(0, _ptr(w), 70, H, S, None, 0, None, None, 0, _ptr(xw), _ptr(ss), rows, R.EPS, None, 0, None, _ptr(o), None, 0,
                                            R.ldo_of(cons), None, None, None, 2, 1, 0, _ptr(form_c)))
    (ref, bound), = R.skinny_reference(cons, d2).values()
    got = R.decode(o, False)
    wc = R.buffer_excess(got, ref, bound)
    print(f"consumer on the producer's buffers ({rows} partial rows): at {wc:.4f} of the bound, XMODE {form_c[3]}")
    assert wc <= 1.0 and form_c[3] == 3
    fused = R._c("chain-fused-norm", H, 70, S, 0, "f32norm", None)
    pf, _ = _checked(lib, fused, d2)
    (_, bound_f), = R.skinny_reference(fused, d2).values()
    gap = np.abs(got[:S, :70] - R.decode(pf["out"], False)[:S, :70]) / (bound[:S, :70] + bound_f[:S, :70])
    print(f"pre-normalised against fused-norm launch: {gap.max():.4f} of their joint bound apart")
    assert gap.max() <= 1.0


# ---- attention ---------------------------------------------------------------------------------------------------------------------
def _attn(lib, c, d, form, split=False):
    """One q3a_selftest_batched_attn_launch: (kc_out, vc_out as fp32 values, the output buffer decoded, the raw partials or None)."""
    S, n_q, n_kv = len(c["pos"]), c["n_q"], c["n_kv"]
    conv = (lambda a: np.ascontiguousarray(a, np.float32).copy()) if d["kv_f32"] else (lambda a: np.ascontiguousarray(R.bf16_bits(a)))
    kc, vc = conv(d["kc"]), conv(d["vc"])
    out = np.ascontiguousarray(R.attn_out_init(c, form))
    qkv, qn, kn, rope, pos = (np.ascontiguousarray(d[k]) for k in ("qkv", "q_norm", "k_norm", "rope", "pos"))
    parts = None
    if split:   # NaN bytes, what the poison_attn_partials knob leaves in the engine's partial buffers
        ns = c["nsplit"]
        parts = [np.full(shape, np.nan, np.float32) for shape in ((S, n_q, ns), (S, n_q, ns), (S, n_q, ns, 128))]
    rc = lib.q3a_selftest_batched_attn_launch(0, int(d["kv_f32"]), int(split), S, _ptr(qkv), _ptr(pos), _ptr(qn), _ptr(kn), R.ATTN_EPS, _ptr(rope), _ptr(kc),
                                              _ptr(vc), n_q, n_kv, c["max_ctx"], R.SCALE, c.get("trim", 0), c.get("nsplit", 0), c.get("keys", 0),
                                              R.OUT_FORMS.index(form), _ptr(out), *(map(_ptr, parts) if split else (None, None, None)))
    if rc != 0:
        return rc
    val = (lambda a: a) if d["kv_f32"] else R.bf16_value
    return val(kc), val(vc), R.decode(out, form != "f32"), parts


@pytest.mark.parametrize("form", R.OUT_FORMS)
@pytest.mark.parametrize("kv_f32", [False, True], ids=["bf16-cache", "fp32-cache"])
@pytest.mark.parametrize("c", R.ATTN_CASES, ids=[c["name"] for c in R.ATTN_CASES])
def test_batched_attention(lib, c, kv_f32, form):
    d = R.attn_inputs(c, kv_f32)
    res = _attn(lib, c, d, form)
    _ok(lib, res if isinstance(res, int) else 0)
    kc, vc, out, _ = res
    rows, ctx = R.attn_excess_parts(c, d, kc, vc, out, form, bf16_q=not kv_f32)
    print(f"{c['name']} {'fp32' if kv_f32 else 'bf16'} cache, {form} out: new rows at {rows:.4f}, context at {ctx:.4f} of the bound")
    assert max(rows, ctx) <= 1.0


def test_fragment_order_holds_32_sequences(lib):
    """33 sequences: fragment order is refused before anything runs, on either path; row-major is served."""
    c = dict(name="s33", n_q=4, n_kv=2, pos=tuple(s % 5 for s in range(33)), max_ctx=128, trim=1, nsplit=1, keys=128)
    d = R.attn_inputs(c, False)
    for split in (False, True):
        rc = _attn(lib, c, d, "bf16frag", split=split)
        msg = (lib.q3a_last_error(None) or b"").decode()
        assert isinstance(rc, int) and rc != 0 and "fragment order holds at most 32 sequences" in msg, msg
    res = _attn(lib, c, d, "bf16")
    _ok(lib, res if isinstance(res, int) else 0)
    w = R.attn_excess(c, d, res[0], res[1], res[2], "bf16", bf16_q=True)
    print(f"33 sequences, row-major bf16: at {w:.4f} of the bound")
    assert w <= 1.0


def test_split_path_and_combine(lib):
    """launch_decode_attn on six ragged sequences with five 128-key splits, then launch_attn_combine in its three output forms: empty
    splits are (-inf, 0, 0), each output form against the float64 merge of the partials the launch wrote, the bf16 forms within half a
    bf16 ulp of the fp32 form, and the combined context -- like the batched kernel's on the same data -- inside its own bound of the
    float64 attention on the appended rows."""
    c = R.SPLIT_CASE
    d = R.attn_inputs(c, False, stale_nan=False)
    by_form = {}
    for form in R.OUT_FORMS:
        res = _attn(lib, c, d, form, split=True)
        _ok(lib, res if isinstance(res, int) else 0)
        kc, vc, out, (pm, pl, po) = res
        R.check_empty_splits(c, d, pm, pl, po)
        ref, bound = R.combine_reference(pm, pl, po)
        if form == "f32":
            w = R.buffer_excess(out, R.attn_place(c, ref, form), R.attn_place(c, bound, form))
        else:   # half a bf16 ulp of the fp32 form's value
            f32_form = by_form["f32"].reshape(ref.shape)
            w = R.buffer_excess(out, R.attn_place(c, f32_form, form), np.nan_to_num(R.attn_place(c, R.half_ulp_bf16(f32_form), form), nan=1.0))
        wa = R.attn_excess_parts(c, d, kc, vc, out, form, bf16_q=False)[1]
        print(f"combine {form}: at {w:.4f} of the merge bound, {wa:.4f} of the attention bound")
        assert w <= 1.0 and wa <= 1.0
        by_form[form] = out
    res = _attn(lib, dict(c, trim=0), d, "f32")
    _ok(lib, res if isinstance(res, int) else 0)
    rows, wb = R.attn_excess_parts(c, d, res[0], res[1], res[2], "f32", bf16_q=True)
    print(f"batched kernel on the same data: new rows at {rows:.4f}, context at {wb:.4f} of its bound")
    assert max(rows, wb) <= 1.0
