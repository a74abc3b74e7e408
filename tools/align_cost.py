#!/usr/bin/env python
"""Forced-aligner throughput and the cost of its head (k_align.hip) against the prefill of the same call.

On a synthetic aligner checkpoint (presets 0.6b_aligner / tiny_aligner), B clips of S seconds with about 2.5 words per second of
audio (two markers each), whole path q3a_align_batch_ptrs (host PCM in, classes out).  Per round: wall time of the call, the
prefill (layers + head) and the head's three launches (q3a_debug_read "align_head_ms", HIP events around them).  Reports medians:
audio seconds aligned per second of wall time, the head in us and as a share of the prefill.

    python tools/align_cost.py --batch 1 --rounds 7
    python tools/align_cost.py --batch 32 --rounds 7
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="0.6b_aligner")
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--words-per-second", type=float, default=2.5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--precise", action="store_true")
    args = ap.parse_args()
    from align_ref import word_ids
    from qwen3_asr_rs_amd import synthetic
    from qwen3_asr_rs_amd.engine import HipEngine
    model_dir = f"/tmp/q3a_ckpt_{args.preset.replace('.', 'p')}"
    synthetic.write_checkpoint(model_dir, args.preset, seed=4, embed_scale=synthetic.PEAKED_EMBED_SCALE)
    clips = [synthetic.synthetic_clip(i, args.seconds) for i in range(args.batch)]
    n_words = max(1, int(round(args.seconds * args.words_per_second)))
    texts = [word_ids(n_words, 100 + i) for i in range(args.batch)]
    eng = HipEngine(model_dir, 0, precise=args.precise, max_new_tokens=1)
    eng.align_batch(clips, texts)  # warm-up: buffers, code objects
    walls, pre, head = [], [], []
    for r in range(args.rounds):
        t0 = time.perf_counter()
        cls = eng.align_batch(clips, texts)
        walls.append((time.perf_counter() - t0) * 1e3)
        t = eng.timings()
        pre.append(t["prefill_ms"])
        head.append(float(eng.debug_read("align_head_ms")[0]))
        print(f"round {r}: wall {walls[-1]:.2f} ms  prefill {pre[-1]:.3f} ms  head {head[-1] * 1e3:.1f} us  "
              f"mel {t['mel_ms']:.3f} enc {t['encoder_ms']:.3f}  prompt rows {t['total_prompt_tokens']}")
    markers = sum(len(c) for c in cls)
    w, p, h = statistics.median(walls), statistics.median(pre), statistics.median(head)
    print(f"preset {args.preset} batch {args.batch} x {args.seconds:.0f} s, {n_words} words / clip, {markers} markers, "
          f"{'precise' if args.precise else 'default'} mode")
    print(f"throughput {args.batch * args.seconds / (w / 1e3):.1f} audio-s/s (median wall {w:.2f} ms)")
    print(f"head {h * 1e3:.1f} us = {100.0 * h / p:.2f} % of the prefill ({p:.3f} ms, head included)")
    eng.close()


if __name__ == "__main__":
    main()
