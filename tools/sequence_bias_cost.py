#!/usr/bin/env python
"""Cost of the sequence bias (q3a_set_sequence_bias) on the decode step: an interleaved A/B on ONE engine, PCM resident,
graph-replayed fixed-length decode (q3a_run_resident with fixed_new_tokens); decode ms per step from q3a_stage_timings (device
events).  Arms, their order rotated round by round:
    off     the setting off (the launches of an engine that never had it; at one sequence the pruned lm_head argmax)
    e16     a list of 16 entries (two to four ids each) on 16 targets
    e4096   a list of 4096 entries on 4096 targets: 16 target groups per thread of the kernel

    python tools/sequence_bias_cost.py --preset 0.6b --batch 1 --rounds 7
    python tools/sequence_bias_cost.py --preset 0.6b --batch 32 --rounds 7

The entries' leading ids are drawn at random, so almost none fires: what is timed is the stored row, the kernel's walk over the
tables and the fresh argmax partials, not a changed transcript.  Prints one line per round and a summary: median us per step of each
arm, the difference to `off` in percent and in us, pruned passes per arm at one sequence, and that `off` generated the same ids
before and after the other arms ran."""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_list(n, vocab, seed=0):
    rng = np.random.default_rng(seed)
    targets = rng.choice(vocab - 1000, n, replace=False)
    return [(tuple(int(x) for x in rng.integers(0, vocab - 1000, 1 + i % 3)) + (int(t),), 0.5) for i, t in enumerate(targets)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="0.6b")
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--new-tokens", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--arms", default="off,e16,e4096")
    args = ap.parse_args()
    from qwen3_asr_rs_amd import synthetic
    from qwen3_asr_rs_amd.engine import HipEngine
    model_dir = f"/tmp/q3a_ckpt_{args.preset.replace('.', 'p')}"
    synthetic.write_checkpoint(model_dir, args.preset, seed=0, shards=2 if args.preset == "1.7b" else 1, embed_scale=synthetic.PEAKED_EMBED_SCALE)
    N = args.new_tokens
    clips = [synthetic.synthetic_clip(i, args.seconds) for i in range(args.batch)]
    eng = HipEngine(model_dir, 0, max_new_tokens=max(N, 16))
    eng.upload_pcm(clips)
    lists = {"e16": make_list(16, eng.dims.vocab_size), "e4096": make_list(4096, eng.dims.vocab_size)}
    names = [a for a in args.arms.split(",") if a]
    state = {"set": False}

    def stats():
        return eng.debug_read_raw("lm_head_prune_stats").view(np.int32).astype(np.int64)

    def run(arm):
        if arm != "off":
            eng.set_sequence_bias(lists[arm])
            state["set"] = True
        elif state["set"]:
            eng.set_sequence_bias(None)
            state["set"] = False
        s0 = stats()
        eng.run_resident(None, N, N)
        t = eng.timings()
        return t["decode_ms"] / max(1, t["decode_steps"]), eng.fetch_ids(N), int((stats() - s0)[1])

    _, ids0, _ = run("off")
    for arm in names:  # warm-up: graph capture, caches
        run(arm)
    per, passes, ids = {a: [] for a in names}, {a: [] for a in names}, {}
    for r in range(args.rounds):
        order = names[r % len(names):] + names[:r % len(names)]
        got = {}
        for arm in order:
            ms, ids[arm], np_ = run(arm)
            per[arm].append(ms)
            passes[arm].append(np_)
            got[arm] = ms
        print(f"round {r}: " + ", ".join(f"{a} {1e3 * got[a]:.1f}" for a in names) + " us/step", flush=True)
    med = {a: statistics.median(v) for a, v in per.items()}
    base = med.get("off")
    line = f"{args.preset} x {args.batch} clips of {args.seconds:g} s, {N} tokens, {args.rounds} rounds, median us/step: "
    line += ", ".join(f"{a} {1e3 * med[a]:.1f}" + (f" ({100.0 * (med[a] / base - 1.0):+.2f} %, {1e3 * (med[a] - base):+.1f} us)" if base and a != "off" else "")
                      for a in names)
    if args.batch == 1:
        line += "; pruned lm_head passes per run: " + ", ".join(f"{a} {statistics.median(passes[a]):.0f}" for a in names)
    if "off" in ids:
        line += f"; off ids unchanged: {ids['off'] == ids0}"
    print(line)
    eng.close()


if __name__ == "__main__":
    main()
