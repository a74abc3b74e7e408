"""The one-sequence chain with o_proj per pair of kv heads on the GPU against float64, per element, with the cases, references and derived
bounds of tests/oproj_by_head_ref.py (tests/test_oproj_by_head_host.py shows what those bounds let through and what they catch):
oproj_head_kernel, the gate / up form that adds its partial vectors, decode attention at 32 and 64 keys per split -- one launch each
through the selftest entry points -- and the engine end to end across the table's change from 32- to 64-key splits.  Output buffers go in
filled with a sentinel and come back whole.  Each test prints its figure before it asserts."""
import ctypes as C

import numpy as np
import pytest

import decode_kernels_ref as R
import oproj_by_head_ref as Q

pytestmark = pytest.mark.gpu


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _f32(a):
    return None if a is None else np.ascontiguousarray(a, np.float32)


def _ok(lib, rc):
    """A refusal fails the test; a HIP error ends the session -- nothing more is launched on a device that has faulted."""
    if rc != 0:
        msg = (lib.q3a_last_error(None) or b"").decode()
        if "HIP error" in msg:
            pytest.exit(f"stopping: {msg}", returncode=3)
        pytest.fail(msg)


def _oproj(lib, c, d, nsplit=None, pm=None, pl=None, po=None):
    W = d["W"]
    N, K = W.shape
    w, bias = np.ascontiguousarray(R.bf16_bits(W)), _f32(d["bias"])
    pm, pl, po = _f32(d["pm"] if pm is None else pm), _f32(d["pl"] if pl is None else pl), _f32(d["po"] if po is None else po)
    y = np.full((c["n_parts"], N), R.SENTINEL, np.float32)
    rc = lib.q3a_selftest_oproj_head_launch(0, _ptr(w), N, K, _ptr(bias), _ptr(pm), _ptr(pl), _ptr(po), c["nsplit"] if nsplit is None else nsplit,
                                            c["heads"], c["n_parts"], _ptr(y))
    return rc, y


@pytest.mark.parametrize("c", Q.OPROJ_CASES, ids=[c["name"] for c in Q.OPROJ_CASES])
def test_oproj_head_kernel(lib, c):
    d = Q.oproj_inputs(c)
    rc, y = _oproj(lib, c, d)
    _ok(lib, rc)
    assert not np.any(y == R.SENTINEL), "a partial vector entry was not written"
    w = Q.oproj_excess(c, d, y)
    print(f"{c['name']}: at {w:.4f} of the bound")
    assert w <= 1.0


def test_oproj_head_refuses_seventeen_splits(lib):
    c = dict(Q.OPROJ_CASES[0], nsplit=17, name="oproj-17-splits")
    d = Q.oproj_inputs(c)
    rc, y = _oproj(lib, c, d)
    msg = (lib.q3a_last_error(None) or b"").decode()
    print(f"rc {rc}: {msg}")
    assert rc != 0 and "oproj_head" in msg and "HIP error" not in msg
    assert np.all(y == R.SENTINEL), "a refused launch wrote"


@pytest.mark.parametrize("c", Q.PARTS_CASES, ids=[c["name"] for c in Q.PARTS_CASES])
def test_gate_up_adds_the_partial_vectors(lib, c):
    d = Q.parts_inputs(c)
    N, K = d["W"].shape
    w = np.ascontiguousarray(R.bf16_bits(d["W"]))
    x, g, bias, parts = _f32(d["resid_x"]), _f32(d["g"]), _f32(d["bias"]), _f32(d["parts"])
    out, xs = np.full(N // 2, R.SENTINEL, np.float32), np.full(K, R.SENTINEL, np.float32)
    _ok(lib, lib.q3a_selftest_gemv_parts_launch(0, _ptr(w), N, K, _ptr(x), _ptr(g), d["eps"], _ptr(bias), _ptr(parts), c["n_parts"], _ptr(out), _ptr(xs)))
    x_ref, x_b = Q.parts_sum_reference(d)
    wx = R.excess(xs, x_ref, x_b)
    g_ref, g_b = Q.parts_glu_reference(c, d, xs)
    wo = R.excess(out, g_ref, g_b)
    print(f"{c['name']}: summed x at {wx:.4f} of the bound, GLU at {wo:.4f}")
    assert wx <= 1.0 and wo <= 1.0


@pytest.mark.parametrize("c", Q.DATTN_SPLIT_CASES, ids=[c["name"] for c in Q.DATTN_SPLIT_CASES])
def test_decode_attention_split_sizes(lib, c):
    d = R.dattn_inputs(c)
    ns = Q.dattn_nsplit(c)
    kc, vc = np.ascontiguousarray(R.bf16_bits(d["kc"])), np.ascontiguousarray(R.bf16_bits(d["vc"]))
    pm, pl = np.full((R.N_Q, ns), R.SENTINEL, np.float32), np.full((R.N_Q, ns), R.SENTINEL, np.float32)
    po = np.full((R.N_Q, ns, 128), R.SENTINEL, np.float32)
    qkv, qn, kn, rope = (_f32(d[k]) for k in ("qkv", "q_norm", "k_norm", "rope"))
    _ok(lib, lib.q3a_selftest_decode_attn_split_launch(0, 0, c["kps"], _ptr(qkv), d["pos"], _ptr(qn), _ptr(kn), d["eps"], _ptr(rope), _ptr(kc),
                                                       _ptr(vc), R.N_Q, R.N_KV, c["max_ctx"], ns, R.SCALE, _ptr(pm), _ptr(pl), _ptr(po)))
    w = Q.dattn_check(c, d, R.bf16_value(kc), R.bf16_value(vc), pm, pl, po)
    print(f"{c['name']}: {ns} splits, at {w:.4f} of the bound")
    assert w <= 1.0


def _knob(lib, v):
    assert lib.q3a_debug_set(b"oproj_by_head", v) == 0


def test_ids_equal_the_merging_chain_across_the_split_size_change(lib, tiny_dir):
    """Tiny preset, the fixture clip of oproj_by_head_ref (a 275-token prompt), generated until the context has passed 512 keys: the
    chain with o_proj per pair of kv heads -- 32-key splits, 9 to 16 of them, then 64-key splits -- graph-replayed and eager (one decode_step per
    token), against the chain with the merging o_proj and 128-key splits (knob oproj_by_head = 0).  The ids must be equal: the fixture's
    smallest top-1 / top-2 margin in the fp32 oracle is asserted in tests/test_oproj_by_head_host.py, so a difference is a bug, not a
    near-tie.  (Contexts with fewer splits: the kernel cases above, and every other tiny-preset test, which now runs this chain.)"""
    from qwen3_asr_rs_amd import synthetic
    from qwen3_asr_rs_amd.engine import HipEngine
    clip, steps = synthetic.synthetic_clip(Q.E2E_CLIP_SEED, Q.E2E_CLIP_SECONDS), Q.E2E_STEPS

    def graph_run():
        eng = HipEngine(tiny_dir, 0, use_graph=True, max_new_tokens=steps + 8)
        ids = eng.transcribe_batch([clip], None, max_new=steps, fixed_new_tokens=steps)[0]
        eng.close()
        return ids

    try:
        _knob(lib, 0)
        base = graph_run()
        _knob(lib, 1)
        new = graph_run()
        eng = HipEngine(tiny_dir, 0, use_graph=False, max_new_tokens=steps + 8)
        eng.mel([clip])
        eng.encode()
        P = len(HipEngine.build_prompt(eng.num_audio_tokens(len(clip))))
        _, nxt = eng.prefill([HipEngine.build_prompt(eng.num_audio_tokens(len(clip)))])
        eager = [int(nxt[0])]
        for _ in range(steps - 1):
            _, nxt, _ = eng.decode_step()
            eager.append(int(nxt[0]))
        eng.close()
    finally:
        _knob(lib, 1)
    first = next((i for i, (a, b) in enumerate(zip(base, new)) if a != b), None)
    print(f"prompt {P}, {steps} steps: context reaches {P + steps - 1} keys; first difference graph {first}, "
          f"eager {next((i for i, (a, b) in enumerate(zip(base, eager)) if a != b), None)}")
    assert P <= 512 - 32 and P + steps - 1 >= 512 + 8
    assert len(base) == steps and new == base and eager == base
