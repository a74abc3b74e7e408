#!/usr/bin/env python
"""Cost of scoring a given transcript (q3a_score_batch_ptrs) and of its head (k_align.hip launch_score_head) against the prefill of the
same call, next to the only way to the same rows without it: q3a_prefill + one (q3a_set_next_tokens, q3a_decode_step) per token on
an engine with token_logprobs = 1.

On a synthetic checkpoint (preset 0.6b), B clips of S seconds with N targets each.  Both variants run alternately in one process,
the warm-up round is excluded, times are the engine's device events (q3a_stage_timings, q3a_debug_read "score_head_ms") plus the
wall time of the call.  Reports medians: whole-call ms and audio seconds scored per second, the prefill with and without the head,
the head in ms, its achieved FLOP/s (2 M vocab hidden), its share of the prefill next to its share of the prefill's FLOPs.

    python tools/score_cost.py --batch 1 --rounds 7
    python tools/score_cost.py --batch 32 --rounds 7
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def prefill_flops(dims, rows, seq_lens):
    """Matrix FLOPs of the decoder prefill over `rows` prompt rows (projections + causal attention); the head is not included."""
    H, I, L = dims.hidden_size, dims.intermediate_size, dims.dec_layers
    qd, kvd = dims.num_q_heads * dims.head_dim, dims.num_kv_heads * dims.head_dim
    proj = 2.0 * rows * (H * (qd + 2 * kvd) + qd * H + 3 * H * I)
    attn = sum(2.0 * 2.0 * dims.num_q_heads * dims.head_dim * n * (n + 1) / 2 for n in seq_lens)
    return L * (proj + attn)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="0.6b")
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--targets", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--precise", action="store_true")
    ap.add_argument("--no-decode-loop", action="store_true", help="skip the stage-API comparison")
    args = ap.parse_args()
    from qwen3_asr_rs_amd import synthetic
    from qwen3_asr_rs_amd.engine import HipEngine
    model_dir = f"/tmp/q3a_ckpt_{args.preset.replace('.', 'p')}_peaked"
    synthetic.write_checkpoint(model_dir, args.preset, seed=0, embed_scale=synthetic.PEAKED_EMBED_SCALE)
    B, N = args.batch, args.targets
    clips = [synthetic.synthetic_clip(i, args.seconds) for i in range(B)]
    eng = HipEngine(model_dir, 0, precise=args.precise, max_new_tokens=N, token_logprobs=True)
    V, H = eng.dims.vocab_size, eng.dims.hidden_size
    # targets: the model's own ids with every seventh replaced (both the "agrees" and the "disagrees" rows are exercised)
    ids = eng.transcribe_batch(clips, None, max_new=N, fixed_new_tokens=N)
    targets = [[(t * 48271 + 12345) % V if s % 7 == 3 else t for s, t in enumerate(u)] for u in ids]
    targets = [[t + 1 if t == 151676 else t for t in u] for u in targets]
    M = B * N

    def score_round():
        t0 = time.perf_counter()
        eng.score_batch(clips, targets)
        wall = (time.perf_counter() - t0) * 1e3
        t = eng.timings()
        return wall, t, float(eng.debug_read("score_head_ms")[0])

    def loop_round():
        """The same rows through the stage API: device time is not separable per call here, so wall time of prefill + N - 1 forced
        steps (mel and encoder excluded: they are the same in both variants)."""
        eng.mel(clips)
        eng.encode()
        prompts = [HipEngine.build_prompt(t) for t in eng._T]
        t0 = time.perf_counter()
        eng.prefill(prompts, want_logits=False)
        for s in range(N - 1):
            eng.set_next_tokens([u[s] for u in targets])
            eng.decode_step(want_logits=False)
        wall = (time.perf_counter() - t0) * 1e3
        eng.fetch_logprobs()
        return wall

    score_round()
    if not args.no_decode_loop:
        loop_round()
    walls, totals, pre, head, loops = [], [], [], [], []
    t = None
    for r in range(args.rounds):
        w, t, h = score_round()
        walls.append(w); totals.append(t["total_ms"]); pre.append(t["prefill_ms"]); head.append(h)
        line = f"round {r}: score wall {w:.2f} ms  total {t['total_ms']:.3f}  prefill {t['prefill_ms']:.3f}  head {h:.3f} ms"
        if not args.no_decode_loop:
            loops.append(loop_round())
            line += f"  | prefill + {N - 1} forced decode steps: wall {loops[-1]:.2f} ms"
        print(line)
    w, tot, p, h = (statistics.median(x) for x in (walls, totals, pre, head))
    rows = t["total_prompt_tokens"]
    seq_lens = [rows // B] * B
    head_flops = 2.0 * M * V * H
    pf = prefill_flops(eng.dims, rows, seq_lens)
    print(f"preset {args.preset} batch {B} x {args.seconds:.0f} s, {N} targets / clip, {M} scored rows, {rows} prefilled rows, "
          f"{'precise' if args.precise else 'default'} mode")
    print(f"whole call {tot:.2f} ms on the device (median wall {w:.2f} ms): {B * args.seconds / (w / 1e3):.1f} audio-s/s")
    print(f"prefill {p:.3f} ms with the head, {p - h:.3f} ms without; head {h:.3f} ms = {head_flops / (h * 1e-3) / 1e12:.1f} TFLOP/s "
          f"({head_flops / 1e9:.1f} GFLOP)")
    print(f"head share of the prefill (head included) {100.0 * h / p:.1f} %; share of its FLOPs {100.0 * head_flops / (head_flops + pf):.1f} %")
    if loops:
        lw = statistics.median(loops)
        print(f"same rows through q3a_prefill + {N - 1} x (q3a_set_next_tokens, q3a_decode_step): median wall {lw:.2f} ms "
              f"against {p:.2f} ms of prefill + head here ({lw / p:.1f} x)")
    eng.close()


if __name__ == "__main__":
    main()
