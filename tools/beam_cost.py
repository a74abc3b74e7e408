#!/usr/bin/env python
"""Cost of a beam search (q3a_beam_search_batch_ptrs) next to the greedy loop of the same engine at the same number of sequences.

On a synthetic checkpoint (preset 0.6b), U clips of S seconds, width W, N rounds.  Both variants run alternately in one process, the
warm-up round is excluded, times are the engine's device events (q3a_stage_timings).  Reports medians: per-step time of the beam
step (decode_ms / decode_steps) against the greedy step at U * W sequences, KV rows copied per round (q3a_debug_read "beam_stats"),
and the share of the call spent on the W-fold front end (mel + encoder + prefill of U * W sequences against the same for U).

    python tools/beam_cost.py --utterances 1 --width 4
    python tools/beam_cost.py --utterances 8 --width 4

The split of the per-step difference into its launches (stored logits, top-W, advance, reorder) comes from a kernel trace in a run
of its own:

    rocprofv3 --kernel-trace --stats -- python tools/beam_cost.py --utterances 8 --width 4 --rounds 1 --beam-only
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="0.6b")
    ap.add_argument("--utterances", type=int, default=1)
    ap.add_argument("--width", type=int, default=4)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--steps", type=int, default=100, help="rounds of the search = tokens of the greedy run")
    ap.add_argument("--rounds", type=int, default=7, help="repetitions (medians)")
    ap.add_argument("--precise", action="store_true")
    ap.add_argument("--beam-only", action="store_true", help="no greedy runs (kernel traces)")
    args = ap.parse_args()
    from qwen3_asr_rs_amd import synthetic
    from qwen3_asr_rs_amd.engine import HipEngine
    model_dir = f"/tmp/q3a_ckpt_{args.preset.replace('.', 'p')}_peaked"
    synthetic.write_checkpoint(model_dir, args.preset, seed=0, embed_scale=synthetic.PEAKED_EMBED_SCALE)
    U, W, N = args.utterances, args.width, args.steps
    clips = [synthetic.synthetic_clip(i, args.seconds) for i in range(U)]
    wide = [c for c in clips for _ in range(W)]  # the greedy batch of the same size: each clip W times
    eng = HipEngine(model_dir, 0, precise=args.precise, max_new_tokens=N)

    def beam_round():
        eng.beam_search_batch(clips, W, max_new=N)
        return eng.timings(), eng.beam_debug()["stats"].tolist()

    def greedy_round(batch):
        eng.transcribe_batch(batch, None, max_new=N, fixed_new_tokens=N)
        return eng.timings()

    beam_round()
    if not args.beam_only:
        greedy_round(wide)
        greedy_round(clips)
    bs, gs, g1, stats = [], [], [], None
    for r in range(args.rounds):
        t, stats = beam_round()
        bs.append(t)
        line = f"round {r}: beam total {t['total_ms']:.2f} ms  decode {t['decode_ms']:.2f} ms / {t['decode_steps']} steps"
        if not args.beam_only:
            gs.append(greedy_round(wide))
            g1.append(greedy_round(clips))
            line += f"  | greedy x{U * W}: decode {gs[-1]['decode_ms']:.2f} ms / {gs[-1]['decode_steps']} steps  | greedy x{U}: total {g1[-1]['total_ms']:.2f} ms"
        print(line)
    med = lambda ts, f: statistics.median(f(t) for t in ts)  # noqa: E731
    b_step = med(bs, lambda t: t["decode_ms"] / max(t["decode_steps"], 1)) * 1e3
    b_total = med(bs, lambda t: t["total_ms"])
    front_w = med(bs, lambda t: t["mel_ms"] + t["encoder_ms"] + t["prefill_ms"])
    print(f"preset {args.preset}, {U} x {args.seconds:.0f} s clips, width {W} ({U * W} sequences), {N} rounds, {'precise' if args.precise else 'default'} mode")
    print(f"beam step {b_step:.1f} us (decode {med(bs, lambda t: t['decode_ms']):.2f} ms of a {b_total:.2f} ms call)")
    rounds, copies, rows, fin = stats
    print(f"history: {copies} survivors left their parent's slot in {rounds} rounds, {rows} KV rows copied = {rows / max(rounds, 1):.1f} per round "
          f"(x layers x 2 x kv heads x 128 elements each); {fin} hypotheses finished")
    if not args.beam_only:
        g_step = med(gs, lambda t: t["decode_ms"] / max(t["decode_steps"], 1)) * 1e3
        front_1 = med(g1, lambda t: t["mel_ms"] + t["encoder_ms"] + t["prefill_ms"])
        print(f"greedy step at {U * W} sequences {g_step:.1f} us: the beam step costs {b_step - g_step:+.1f} us ({100.0 * (b_step / g_step - 1):+.1f} %)")
        print(f"front end (mel + encoder + prefill): {front_w:.2f} ms for {U * W} sequences = {100.0 * front_w / b_total:.1f} % of the call; "
              f"{front_1:.2f} ms for the {U} clip(s) once: the W-fold redundancy is {front_w - front_1:.2f} ms = {100.0 * (front_w - front_1) / b_total:.1f} % of the call")
    eng.close()


if __name__ == "__main__":
    main()
