#!/usr/bin/env python
"""Cost of a logit bias (q3a_set_logit_bias) on the decode step: an interleaved A/B on ONE engine, PCM resident, graph-replayed
fixed-length decode (q3a_run_resident with fixed_new_tokens); decode ms per step from q3a_stage_timings (device events).  Arms,
their order rotated round by round:
    none      no bias set (the launches of an engine that never had one)
    suppress  every id the unbiased run emitted plus a 6144-id range around its first id at -inf (bias kind (a) of the tests)
    allow     an allow-list of 1000 seeded ids plus both EOS ids, everything else -inf (bias kind (c))
At one sequence the pruned lm_head argmax runs in every arm; its candidate 16-row blocks per pass are printed per arm.

    python tools/logit_bias_cost.py --preset 0.6b --batch 1 --rounds 7
    python tools/logit_bias_cost.py --preset 0.6b --batch 32 --rounds 7
    python tools/logit_bias_cost.py --rounds 1 --arms none        # no bias call at all: the run a kernel trace compares launches on

Prints one line per round and a summary: median us per step of each arm, the difference to `none` in percent, candidate blocks
per pruned pass, and that `none` generated the same ids before and after the biased arms ran."""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def bias_kinds(vocab, emitted, top):
    lo = max(0, (int(top) // 2048) * 2048 - 2048)
    suppress = {t: -np.inf for t in set(int(t) for t in emitted) | set(range(lo, min(vocab, lo + 6144)))}
    rng = np.random.default_rng(11)
    allow = {int(t): 0.0 for t in set(rng.choice(vocab, 1000, replace=False).tolist()) | {151643, 151645}}
    return {"suppress": (suppress, 0.0), "allow": (allow, -np.inf)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="0.6b")
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--new-tokens", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--arms", default="none,suppress,allow")
    args = ap.parse_args()
    from qwen3_asr_rs_amd import synthetic
    from qwen3_asr_rs_amd.engine import HipEngine
    model_dir = f"/tmp/q3a_ckpt_{args.preset.replace('.', 'p')}"
    synthetic.write_checkpoint(model_dir, args.preset, seed=0, shards=2 if args.preset == "1.7b" else 1, embed_scale=synthetic.PEAKED_EMBED_SCALE)
    N = args.new_tokens
    clips = [synthetic.synthetic_clip(i, args.seconds) for i in range(args.batch)]
    eng = HipEngine(model_dir, 0, max_new_tokens=max(N, 16))
    eng.upload_pcm(clips)
    names = [a for a in args.arms.split(",") if a]
    state = {"set": False}

    def stats():
        return eng.debug_read_raw("lm_head_prune_stats").view(np.int32).astype(np.int64)

    def run(arm, kinds):
        if arm != "none":
            eng.set_logit_bias(*kinds[arm])
            state["set"] = True
        elif state["set"]:  # (never called when only `none` runs: the same tool then drives a library without the call)
            eng.set_logit_bias(None)
            state["set"] = False
        s0 = stats()
        eng.run_resident(None, N, N)
        t = eng.timings()
        ds = stats() - s0
        return t["decode_ms"] / max(1, t["decode_steps"]), eng.fetch_ids(N), (float(ds[0]) / float(ds[1]) if ds[1] else float("nan"))

    _, ids0, _ = run("none", None)  # warm-up of `none`; its ids define the biases
    kinds = bias_kinds(eng.dims.vocab_size, [t for x in ids0 for t in x], ids0[0][0])
    for arm in names:  # warm-up: graph capture, caches
        run(arm, kinds)
    per, blocks, ids = {a: [] for a in names}, {a: [] for a in names}, {}
    for r in range(args.rounds):
        order = names[r % len(names):] + names[:r % len(names)]
        got = {}
        for arm in order:
            ms, ids[arm], blk = run(arm, kinds)
            per[arm].append(ms)
            blocks[arm].append(blk)
            got[arm] = ms
        print(f"round {r}: " + ", ".join(f"{a} {1e3 * got[a]:.1f}" for a in names) + " us/step", flush=True)
    med = {a: statistics.median(v) for a, v in per.items()}
    base = med.get("none")
    line = f"{args.preset} x {args.batch} clips of {args.seconds:g} s, {N} tokens, {args.rounds} rounds, median us/step: "
    line += ", ".join(f"{a} {1e3 * med[a]:.1f}" + (f" ({100.0 * (med[a] / base - 1.0):+.2f} %)" if base and a != "none" else "") for a in names)
    if args.batch == 1:
        line += "; candidate blocks per pruned pass: " + ", ".join(f"{a} {statistics.median(blocks[a]):.2f}" for a in names)
    if "none" in ids:
        line += f"; none ids unchanged: {ids['none'] == ids0}"
    for a in names:
        if a != "none":
            b, _ = kinds[a]
            line += f"; {a}: {sum(1 for v in b.values() if v == -np.inf) if a == 'suppress' else len(b)} ids {'suppressed' if a == 'suppress' else 'allowed'}, ids differ from none: {ids[a] != ids0}"
    print(line)
    eng.close()


if __name__ == "__main__":
    main()
