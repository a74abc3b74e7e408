"""The one-sequence decode kernels on the GPU against float64, per element: every form launch_gemv picks at one sequence (norm-fused
through LDS and through registers, GLU, residual, the long-K forms), the o_proj forms that merge flash-decoding partials on the fly,
the lm_head (unpruned, and the int8 pre-pass + rescore pair) with argmax_finalize behind it, and launch_decode_attn at the positions
where its split logic can go wrong -- the cases, references and derived bounds of tests/decode_kernels_ref.py, one launch each through
q3a_selftest_gemv_launch / q3a_selftest_decode_attn_launch in the precise arithmetic.  Every kernel of the chain takes a flat, preloaded
argument head and a tail struct: a mis-marshalled argument lands far outside these bounds (tests/test_decode_kernels_ref_host.py shows
by how much).  Output buffers go in filled with a sentinel and come back whole.  Each test prints its figure before it asserts."""
import ctypes as C

import numpy as np
import pytest

import decode_kernels_ref as R

pytestmark = pytest.mark.gpu


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _ok(lib, rc):
    """A refusal fails the test; a HIP error ends the session -- nothing more is launched on a device that has faulted."""
    if rc != 0:
        msg = (lib.q3a_last_error(None) or b"").decode()
        if "HIP error" in msg:
            pytest.exit(f"stopping: {msg}", returncode=3)
        pytest.fail(msg)


def _gemv(lib, d, mode, pruned=0, want_out=True, heads=0, nsplit=0):
    W = d["W"]
    N, K = W.shape
    out = np.full(N // 2 if mode == 2 else N, R.SENTINEL, np.float32) if want_out else None
    state = np.full(4, -99, np.int32)
    keep = [np.ascontiguousarray(R.bf16_bits(W))] + [None if d.get(k) is None else np.ascontiguousarray(d[k], np.float32)
                                                      for k in ("x", "g", "bias", "resid", "pm", "pl", "po")]
    w, x, g, bias, resid, pm, pl, po = keep
    _ok(lib, lib.q3a_selftest_gemv_launch(0, pruned, _ptr(w), N, K, _ptr(x), _ptr(g), d.get("eps", 0.0), _ptr(bias), mode, _ptr(resid),
                                          _ptr(pm), _ptr(pl), _ptr(po), nsplit, heads, _ptr(out), _ptr(state)))
    return out, state


@pytest.mark.parametrize("c", R.GEMV_CASES, ids=[c["name"] for c in R.GEMV_CASES])
def test_gemv_forms(lib, c):
    d = R.gemv_inputs(c)
    ref, bound = R.gemv_reference(c, d)
    out, _ = _gemv(lib, d, c["mode"])
    w = R.excess(out, ref, bound)
    print(f"{c['name']}: at {w:.4f} of the bound")
    assert w <= 1.0


@pytest.mark.parametrize("c", R.ATTN_GEMV_CASES, ids=[c["name"] for c in R.ATTN_GEMV_CASES])
def test_gemv_merges_attention_partials(lib, c):
    d = R.attn_gemv_inputs(c)
    ref, bound = R.gemv_reference(c, d)
    out, _ = _gemv(lib, d, 1, heads=c["heads"], nsplit=c["nsplit"])
    w = R.excess(out, ref, bound)
    print(f"{c['name']}: at {w:.4f} of the bound")
    assert w <= 1.0


@pytest.mark.parametrize("c", R.LM_HEAD_CASES, ids=[c["name"] for c in R.LM_HEAD_CASES])
def test_lm_head_forms_and_finalize(lib, c):
    """The unpruned launch (logits against float64, then the id) and, where it exists, the pruned pair: the same id, the float64 argmax,
    on logits whose top two stand further apart than twice the bound; argmax_finalize leaves the id in next_tok and in out_ids at
    the step it found, and advances the step count and the position by one."""
    d, winner = R.lm_head_inputs(c)
    ref, bound = R.gemv_reference(dict(mode=0), d)
    top = np.argsort(ref)[::-1][:2]
    gap = ref[top[0]] - ref[top[1]]
    print(f"{c['name']}: top-two gap {gap:.4f}, largest logit bound {bound.max():.6f}")
    assert top[0] == winner and gap > 2 * bound.max()
    logits, state = _gemv(lib, d, 3)
    w = R.excess(logits, ref, bound)
    print(f"{c['name']}: logits at {w:.4f} of the bound, state {state.tolist()}")
    assert w <= 1.0
    assert state.tolist() == [winner, winner, 3, 6]
    _, state = _gemv(lib, d, 3, want_out=False)  # the launch as the decode step makes it: no logits stored
    assert state.tolist() == [winner, winner, 3, 6]
    if c["pruned"]:
        _, state = _gemv(lib, d, 3, pruned=1, want_out=False)
        print(f"{c['name']}: pruned pair state {state.tolist()}")
        assert state.tolist() == [winner, winner, 3, 6]


@pytest.mark.parametrize("c", R.DATTN_CASES, ids=[c["name"] for c in R.DATTN_CASES])
def test_decode_attention_positions(lib, c):
    d = R.dattn_inputs(c)
    ns = c["nsplit"]
    kc, vc = np.ascontiguousarray(R.bf16_bits(d["kc"])), np.ascontiguousarray(R.bf16_bits(d["vc"]))
    pm, pl = np.full((R.N_Q, ns), R.SENTINEL, np.float32), np.full((R.N_Q, ns), R.SENTINEL, np.float32)
    po = np.full((R.N_Q, ns, 128), R.SENTINEL, np.float32)
    qkv, qn, kn, rope = (np.ascontiguousarray(d[k], np.float32) for k in ("qkv", "q_norm", "k_norm", "rope"))
    _ok(lib, lib.q3a_selftest_decode_attn_launch(0, 0, _ptr(qkv), d["pos"], _ptr(qn), _ptr(kn), d["eps"], _ptr(rope), _ptr(kc), _ptr(vc),
                                                 R.N_Q, R.N_KV, c["max_ctx"], ns, R.SCALE, _ptr(pm), _ptr(pl), _ptr(po)))
    w = R.dattn_check(c, d, R.bf16_value(kc), R.bf16_value(vc), pm, pl, po)
    print(f"{c['name']}: at {w:.4f} of the bound")
    assert w <= 1.0


def test_graph_replayed_ids_equal_the_eager_stage_api(tiny_dir):
    """End to end on the tiny preset, one clip, 20 tokens: the captured decode chain and the eager stage API (prefill, then one
    decode_step per token) give the same ids."""
    from qwen3_asr_rs_amd import synthetic
    from qwen3_asr_rs_amd.engine import HipEngine
    clip, steps = synthetic.synthetic_clip(4, 3.0), 20
    eng = HipEngine(tiny_dir, 0, use_graph=True, max_new_tokens=32)
    graph_ids = eng.transcribe_batch([clip], None, max_new=steps, fixed_new_tokens=steps)[0]
    eng.close()
    eng = HipEngine(tiny_dir, 0, use_graph=False, max_new_tokens=32)
    eng.mel([clip])
    eng.encode()
    _, nxt = eng.prefill([HipEngine.build_prompt(eng.num_audio_tokens(len(clip)))])
    eager_ids = [int(nxt[0])]
    for _ in range(steps - 1):
        _, nxt, _ = eng.decode_step()
        eager_ids.append(int(nxt[0]))
    eng.close()
    print(f"graph {graph_ids}\neager {eager_ids}")
    assert len(graph_ids) == steps and graph_ids == eager_ids
