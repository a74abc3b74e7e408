#!/usr/bin/env python
"""Cost of temperature sampling (q3a_set_sampling) on the decode step: an interleaved A/B on ONE engine, PCM resident,
graph-replayed fixed-length decode (q3a_run_resident with fixed_new_tokens); decode ms per step from q3a_stage_timings (device
events).  Arms, their order rotated round by round:
    off     sampling off (the launches of an engine that never sampled; at one sequence the pruned lm_head argmax)
    t1      temperature 1, min_p 0: every finite logit gets its Philox word and its two logs
    t1minp  temperature 1, min_p 0.05: only the kept set does
    t1k50 / t1p09 / t1k50p09  temperature 1 under q3a_set_sampling_filter: top_k 50, top_p 0.9, both (the threshold stage's two launches)
    rows    a row table (q3a_set_row_options) whose rows all carry the t1 record: the same launches reading a record per row
    top5 / top20  greedy under q3a_set_top_logprobs with n = 5 / 20: two more launches per step and the stored logits (at one sequence
            the full lm_head GEMV in the place of the pruned argmax)

    python tools/sampling_cost.py --preset 0.6b --batch 1 --rounds 7
    python tools/sampling_cost.py --preset 0.6b --batch 32 --rounds 7
    python tools/sampling_cost.py --batch 1 --arms off,t1,t1k50,t1p09,t1k50p09     # the filter's arms against the sampler's
    python tools/sampling_cost.py --rounds 1 --arms off        # no sampling call at all: the run a kernel trace compares launches on
    python tools/sampling_cost.py --batch 32 --arms t1,rows    # per-row records against the one record (Q3A_LIB: another build's t1)
    python tools/sampling_cost.py --batch 1 --arms off,top5,top20   # top log-probabilities against the greedy step

Prints one line per round and a summary: median us per step of each arm, the difference to `off` in percent and in us, pruned
passes per arm at one sequence, and that `off` generated the same ids before and after the sampled arms ran."""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ARMS = {"t1": (1.0, 0.0), "t1minp": (1.0, 0.05)}          # temperature, min_p
FILTERS = {"t1k50": (50, 1.0), "t1p09": (0, 0.9), "t1k50p09": (50, 0.9)}   # top_k, top_p at temperature 1, min_p 0
TOPS = {"top5": 5, "top20": 20}                            # n of q3a_set_top_logprobs, greedy


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="0.6b")
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--new-tokens", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--arms", default="off,t1,t1minp")
    args = ap.parse_args()
    unknown = [a for a in args.arms.split(",") if a and a not in ("off", "rows") and a not in ARMS and a not in FILTERS and a not in TOPS]
    if unknown:
        ap.error(f"unknown arm(s) {unknown}: choose from off, rows, {', '.join(list(ARMS) + list(FILTERS) + list(TOPS))}")
    from qwen3_asr_rs_amd import synthetic
    from qwen3_asr_rs_amd.engine import HipEngine, RowOptions
    model_dir = f"/tmp/q3a_ckpt_{args.preset.replace('.', 'p')}"
    synthetic.write_checkpoint(model_dir, args.preset, seed=0, shards=2 if args.preset == "1.7b" else 1, embed_scale=synthetic.PEAKED_EMBED_SCALE)
    N = args.new_tokens
    clips = [synthetic.synthetic_clip(i, args.seconds) for i in range(args.batch)]
    eng = HipEngine(model_dir, 0, max_new_tokens=max(N, 16))
    eng.upload_pcm(clips)
    names = [a for a in args.arms.split(",") if a]
    state = {"set": False, "filter": False, "rows": False, "top": False}

    def stats():
        return eng.debug_read_raw("lm_head_prune_stats").view(np.int32).astype(np.int64)

    def run(arm):
        if arm == "rows":
            eng.set_row_options([RowOptions(temperature=ARMS["t1"][0], min_p=ARMS["t1"][1], seed=17)] * args.batch)
            state["rows"] = True
        elif state["rows"]:  # (never called unless the rows arm ran: the other arms drive a library without the call)
            eng.set_row_options(None)
            state["rows"] = False
        if arm in TOPS:
            eng.set_top_logprobs(TOPS[arm])
            state["top"] = True
        elif state["top"]:  # (never called unless a top arm ran: the other arms drive a library without the call)
            eng.set_top_logprobs(0)
            state["top"] = False
        if arm in FILTERS:
            eng.set_sampling_filter(*FILTERS[arm])
            state["filter"] = True
        elif state["filter"]:  # (never called unless a filter arm ran: the other arms drive a library without the call)
            eng.set_sampling_filter(0, 1.0)
            state["filter"] = False
        if arm == "rows":
            pass  # (the uniform setting stays what it was: remembered, not read)
        elif arm != "off" and arm not in TOPS:
            eng.set_sampling(*(ARMS[arm] if arm in ARMS else (1.0, 0.0)), 17)  # (a filter arm: temperature 1, min_p 0)
            state["set"] = True
        elif state["set"]:  # (never called when only `off` runs: the same tool then drives a library without the call)
            eng.set_sampling(0.0)
            state["set"] = False
        s0 = stats()
        eng.run_resident(None, N, N)
        t = eng.timings()
        return t["decode_ms"] / max(1, t["decode_steps"]), eng.fetch_ids(N), int((stats() - s0)[1])

    _, ids0, _ = run("off")  # (`off` before any setter ran calls none of them)
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
    for a in names:
        if a != "off":
            line += f"; {a}: ids differ from off: {ids[a] != ids0}"  # (a top arm is greedy: its ids must NOT differ)
    print(line)
    eng.close()


if __name__ == "__main__":
    main()
