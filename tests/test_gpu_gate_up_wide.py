"""The gate / up GEMV of the one-sequence chain with twelve waves per workgroup (csrc/k_gemv.hip gemv1_xp_body) on the GPU, one launch
each through q3a_selftest_gemv_parts_launch, against the float64 reference and the derived bounds of tests/oproj_by_head_ref.py -- no
tolerance of its own.  The shapes are those at which the grouping of waves into workgroups can go wrong:
  N   32 (16 outputs: the second workgroup has four live waves and eight voided ones), 96 (48 outputs: whole workgroups), 224 (112
      outputs: nine workgroups and four rows);
  K   8 (every lane but the first void), 520 (crosses the first 512-column round by one lane), 1024;
  n   1, 3, 4 partial vectors (three, one and none of the hand-over's four requests clamped and not added).
Per case: the GLU output within its bound; the stored sum x_out bit-equal to the float32 sum formed in ascending order in numpy; a
second launch into buffers poisoned with another pattern returns the same bits.  At the engine level, on the tiny checkpoint, the ids
of the chain equal those of the chain with the merging o_proj (whose gate / up is the plain norm-fused form), graph-replayed and eager,
over a run whose context crosses the change from 32- to 64-key attention splits.  Each test prints its figure before it asserts."""
import ctypes as C

import numpy as np
import pytest

import decode_kernels_ref as R
import oproj_by_head_ref as Q

pytestmark = pytest.mark.gpu

CASES = [dict(name=f"wide-n{N}-k{K}-{P}-vectors", K=K, N=N, n_parts=P, mode=2, rms=True, bias=True)
         for N in (32, 96, 224) for K in (8, 520, 1024) for P in (1, 3, 4)]


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _ok(lib, rc):
    """A refusal fails the test; a HIP error ends the session -- nothing more is launched on a device that has faulted."""
    if rc != 0:
        msg = (lib.q3a_last_error(None) or b"").decode()
        if "HIP error" in msg:
            pytest.exit(f"stopping: {msg}", returncode=3)
        pytest.fail(msg)


def _launch(lib, c, d, poison):
    N, K = d["W"].shape
    w = np.ascontiguousarray(R.bf16_bits(d["W"]))
    x, g, bias, parts = (np.ascontiguousarray(d[k], np.float32) for k in ("resid_x", "g", "bias", "parts"))
    out, xs = np.full(N // 2, poison, np.float32), np.full(K, poison, np.float32)
    _ok(lib, lib.q3a_selftest_gemv_parts_launch(0, _ptr(w), N, K, _ptr(x), _ptr(g), d["eps"], _ptr(bias), _ptr(parts), c["n_parts"], _ptr(out), _ptr(xs)))
    return out, xs


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_wide_gate_up(lib, c):
    d = Q.parts_inputs(c)
    out, xs = _launch(lib, c, d, R.SENTINEL)
    assert not np.any(out == R.SENTINEL) and not np.any(xs == R.SENTINEL), "an output was not written"
    want = d["resid_x"].copy()
    for h in range(c["n_parts"]):
        want = (want + d["parts"][h]).astype(np.float32)
    x_ref, x_b = Q.parts_sum_reference(d)
    g_ref, g_b = Q.parts_glu_reference(c, d, xs)
    wx, wo = R.excess(xs, x_ref, x_b), R.excess(out, g_ref, g_b)
    differ = int((xs.view(np.uint32) != want.view(np.uint32)).sum())
    out2, xs2 = _launch(lib, c, d, np.float32(-7.25e11))
    again = int((out2.view(np.uint32) != out.view(np.uint32)).sum() + (xs2.view(np.uint32) != xs.view(np.uint32)).sum())
    print(f"{c['name']}: summed x at {wx:.4f} of the bound, {differ} of {len(xs)} entries differ from the ascending float32 sum; "
          f"GLU at {wo:.4f} of the bound; second launch: {again} entries differ")
    assert wx <= 1.0 and wo <= 1.0
    assert differ == 0
    assert again == 0


def test_ids_equal_the_merging_chain_graph_and_eager(lib, tiny_dir):
    """The tiny preset on the fixture clip of oproj_by_head_ref (a 275-token prompt, 260 steps: the context goes from 276 to 535 keys,
    32-key splits up to 512 keys, then 64-key splits; the fixture's smallest top-1 / top-2 margin is asserted in
    tests/test_oproj_by_head_host.py, so a difference is a bug, not a near-tie)."""
    from qwen3_asr_rs_amd import synthetic
    from qwen3_asr_rs_amd.engine import HipEngine
    clip, steps = synthetic.synthetic_clip(Q.E2E_CLIP_SEED, Q.E2E_CLIP_SECONDS), Q.E2E_STEPS

    def graph_run():
        eng = HipEngine(tiny_dir, 0, use_graph=True, max_new_tokens=steps + 8)
        ids = eng.transcribe_batch([clip], None, max_new=steps, fixed_new_tokens=steps)[0]
        eng.close()
        return ids

    try:
        assert lib.q3a_debug_set(b"oproj_by_head", 0) == 0
        base = graph_run()
        assert lib.q3a_debug_set(b"oproj_by_head", 1) == 0
        new = graph_run()
        eng = HipEngine(tiny_dir, 0, use_graph=False, max_new_tokens=steps + 8)
        eng.mel([clip])
        eng.encode()
        prompt = HipEngine.build_prompt(eng.num_audio_tokens(len(clip)))
        _, nxt = eng.prefill([prompt])
        eager = [int(nxt[0])]
        for _ in range(steps - 1):
            _, nxt, _ = eng.decode_step()
            eager.append(int(nxt[0]))
        eng.close()
    finally:
        assert lib.q3a_debug_set(b"oproj_by_head", 1) == 0
    P = len(prompt)
    first = lambda got: next((i for i, (a, b) in enumerate(zip(base, got)) if a != b), None)  # noqa: E731
    print(f"prompt {P}, {steps} steps: context reaches {P + steps - 1} keys; first difference graph {first(new)}, eager {first(eager)}")
    assert P <= 512 - 32 and P + steps - 1 >= 512 + 8
    assert len(base) == steps and new == base and eager == base
