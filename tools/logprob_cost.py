#!/usr/bin/env python
"""Cost of token log-probabilities (q3a_opts.token_logprobs) on the decode step: an interleaved A/B in ONE process of two engines on
the same checkpoint, PCM resident, graph-replayed fixed-length decode (q3a_run_resident with fixed_new_tokens); decode ms per step
from q3a_stage_timings.  Three arms, their order rotated round by round:
    off       the option off (the default: at one clip the int8-pruned lm_head argmax)
    off_full  the option off with knob lm_head_prune=0 (the full bf16 lm_head GEMV the option needs at one clip)
    on        the option on
on - off is the cost of the option; off_full - off is the part of it that is the lost prune, on - off_full the log-sum channel.

    python tools/logprob_cost.py --preset 0.6b --batch 1 --rounds 7
    python tools/logprob_cost.py --preset 0.6b --batch 32 --rounds 7

Prints one line per round, a summary (median us per step of each arm, differences in percent, whether every arm generated the same
ids -- it must: the option adds a reduction channel and never changes an id) and, per arm, the lm_head and argmax kernel classes of
one eager decode step bracketed by HIP events (q3a_profile_decode_step)."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="0.6b")
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--new-tokens", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    from qwen3_asr_rs_amd import _lib, synthetic
    from qwen3_asr_rs_amd.engine import HipEngine
    lib = _lib.load()
    model_dir = f"/tmp/q3a_ckpt_{args.preset.replace('.', 'p')}"
    synthetic.write_checkpoint(model_dir, args.preset, seed=0, shards=2 if args.preset == "1.7b" else 1, embed_scale=synthetic.PEAKED_EMBED_SCALE)
    N = args.new_tokens
    clips = [synthetic.synthetic_clip(i, args.seconds) for i in range(args.batch)]
    engines = {}
    for arm, on in (("off", False), ("on", True)):
        e = HipEngine(model_dir, 0, max_new_tokens=max(N, 16), token_logprobs=on)
        e.upload_pcm(clips)
        engines[arm] = e

    arms = {"off": ("off", 1), "off_full": ("off", 0), "on": ("on", 1)}  # arm -> (engine, knob lm_head_prune, latched at the batch set-up)

    def with_knob(prune, fn):
        assert lib.q3a_debug_set(b"lm_head_prune", prune) == 0
        try:
            return fn()
        finally:
            lib.q3a_debug_set(b"lm_head_prune", 1)

    def run(arm):
        eng, prune = arms[arm]
        e = engines[eng]

        def go():
            e.run_resident(None, N, N)
            t = e.timings()
            return t["decode_ms"] / max(1, t["decode_steps"]), e.fetch_ids(N)
        return with_knob(prune, go)

    def profile(arm):  # one eager step on the batch the arm just ran (its knob latched by that run)
        eng, prune = arms[arm]
        e = engines[eng]

        def go():
            e.run_resident(None, N, N)
            return e.profile_decode_step()
        return with_knob(prune, go)

    names = list(arms)
    for arm in names:  # warm-up: graph capture, caches
        run(arm)
    per = {a: [] for a in names}
    ids = {}
    for r in range(args.rounds):
        order = names[r % 3:] + names[:r % 3]
        got = {}
        for arm in order:
            ms, ids[arm] = run(arm)
            per[arm].append(ms)
            got[arm] = ms
        print(f"round {r}: " + ", ".join(f"{a} {1e3 * got[a]:.1f}" for a in names) + " us/step "
              f"(on vs off {100.0 * (got['on'] / got['off'] - 1.0):+.2f} %)", flush=True)
    lp = engines["on"].fetch_logprobs()
    med = {a: statistics.median(v) for a, v in per.items()}
    pct = lambda a, b: 100.0 * (med[a] / med[b] - 1.0)  # noqa: E731
    print(f"{args.preset} x {args.batch} clips of {args.seconds:g} s, {N} tokens, {args.rounds} rounds, median us/step: "
          + ", ".join(f"{a} {1e3 * med[a]:.1f}" for a in names)
          + f"; on vs off {pct('on', 'off'):+.2f} % (off_full vs off {pct('off_full', 'off'):+.2f} %, on vs off_full {pct('on', 'off_full'):+.2f} %)"
          + f"; ids equal: {all(ids[a] == ids['off'] for a in names)}; mean token lp {sum(float(x.mean()) for x in lp) / len(lp):.4f}")
    # kernel classes (q3asr.h Q3A_KC_*): gemv_lm_head = the one-sequence lm_head GEMV or the int8 pre-pass, gemm = every GEMM of the
    # step (the batched lm_head among them), argmax = partials, pruned rescore and finalize
    for arm in names:
        p = profile(arm)
        print(f"profile {arm} (one eager step, HIP events around each launch): "
              + ", ".join(f"{k} {p[k]['total_us']:.1f} us ({p[k]['launches']})" for k in ("gemv_lm_head", "gemm", "argmax")))
    for e in engines.values():
        e.close()


if __name__ == "__main__":
    main()
