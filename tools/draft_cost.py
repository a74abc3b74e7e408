#!/usr/bin/env python
"""Cost of draft-verified decoding (q3a_transcribe_draft_batch_ptrs) next to the plain call (q3a_transcribe_batch_ptrs) on the same
engine, by how much of the draft is accepted.

On a synthetic checkpoint (preset 0.6b), B clips of S seconds, max_new = N.  The plain call's ids are the "right" transcript; a draft
accepted to x % is that transcript with the id at position x N / 100 replaced (100 %: unchanged, 0 %: the first id is wrong -- the
useless draft: one longer prefill and every decode step).  On a random-init checkpoint some steps of a 100-token run sit inside the
default mode's rounding noise, where the verify head (prefill kernels) and the decode step (GEMV kernels) may pick different ids; so
the "right" transcript is settled first: a draft call's result is fed back as the next draft until it comes back unchanged.  The rounds rows use a draft with three substitutions, once with one
verification round and once with up to three (min_tail 1).  All variants run alternately in one process, the warm-up round is
excluded; times are the engine's device events (q3a_stage_timings), medians over the rounds.  Columns: the whole call (mel through the
last decode step), the prefill (every round, head and accept included), the decode steps actually run and their time.

    python tools/draft_cost.py --batch 1 --rounds 7
    python tools/draft_cost.py --batch 32 --rounds 7
"""
import argparse
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BAD = (151643, 151645, 151676)   # ids a draft may not hold


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="0.6b")
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--tokens", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    from qwen3_asr_rs_amd import synthetic
    from qwen3_asr_rs_amd.engine import HipEngine
    model_dir = f"/tmp/q3a_ckpt_{args.preset.replace('.', 'p')}_peaked"
    synthetic.write_checkpoint(model_dir, args.preset, seed=0, embed_scale=synthetic.PEAKED_EMBED_SCALE)
    B, N = args.batch, args.tokens
    clips = [synthetic.synthetic_clip(i, args.seconds) for i in range(B)]
    eng = HipEngine(model_dir, 0, max_new_tokens=N)
    V = eng.dims.vocab_size
    right = eng.transcribe_batch(clips, None, max_new=N)
    assert all(len(r) == N and not set(r) & set(BAD) for r in right), "the synthetic checkpoint stopped early or wrote a special id"
    first = None
    for passes in range(1, 61):   # settle: every pass gets past one under-margin step per clip
        got, acc = eng.transcribe_draft_batch(clips, right, None, max_new=N)
        first = list(acc) if first is None else first
        if got == right:
            break
        right = got
    assert got == right and all(len(r) == N and not set(r) & set(BAD) for r in right), "the transcript did not settle"
    print(f"the plain call's ids were accepted to {min(first)} .. {max(first)} of {N}; settled after {passes} passes")

    def wrong(t):
        w = (t * 48271 + 12345) % V
        return w if w != t and w not in BAD else (t + 1) % V

    def with_errors(positions):
        return [[wrong(t) if i in positions else t for i, t in enumerate(r)] for r in right]

    variants = [("plain call", None, 1)]
    for pct in (0, 50, 90, 100):
        variants.append((f"draft accepted to {pct:3d} %", with_errors({pct * N // 100} if pct < 100 else set()), 1))
    subs = {N // 4, N // 2, 3 * N // 4}
    variants.append(("3 substitutions, max_rounds 1", with_errors(subs), 1))
    variants.append(("3 substitutions, max_rounds 3", with_errors(subs), 3))

    def run(drafts, rounds):
        if drafts is None:
            got, acc = eng.transcribe_batch(clips, None, max_new=N), None
        else:
            got, acc = eng.transcribe_draft_batch(clips, drafts, None, max_new=N, max_rounds=rounds, min_tail=1)
        if acc is not None and rounds == 1:   # (behind a rejected id the decode step continues: those ids may differ inside the noise)
            assert all(g[:k + 1] == r[:k + 1] for g, r, k in zip(got, right, acc)), "the verified prefix differs from the settled transcript"
        return eng.timings(), acc, (eng.draft_stats() if drafts is not None else None)

    for _, drafts, rounds in variants:   # warm-up: code objects, graphs, buffers
        run(drafts, rounds)
    rec = {name: [] for name, _, _ in variants}
    last = {}
    for _ in range(args.rounds):
        for name, drafts, rounds in variants:
            t, acc, st = run(drafts, rounds)
            rec[name].append(t)
            last[name] = (acc, st)
    med = lambda name, key: statistics.median(t[key] for t in rec[name])
    print(f"preset {args.preset}, {B} x {args.seconds:.0f} s clips, max_new {N}, default mode, medians of {args.rounds} rounds (device events, ms)")
    print(f"{'variant':34s} {'whole call':>11s} {'prefill':>9s} {'decode':>9s} {'steps':>6s} {'accepted':>9s} {'rounds':>7s}  vs plain")
    plain_total = med("plain call", "total_ms")
    for name, drafts, _ in variants:
        acc, st = last[name]
        print(f"{name:34s} {med(name, 'total_ms'):11.3f} {med(name, 'prefill_ms'):9.3f} {med(name, 'decode_ms'):9.3f} "
              f"{int(med(name, 'decode_steps')):6d} {('-' if acc is None else str(min(acc))):>9s} {('-' if st is None else str(st['rounds'])):>7s}  "
              f"{med(name, 'total_ms') / plain_total:6.3f} x")
    step_ms = med("plain call", "decode_ms") / max(med("plain call", "decode_steps"), 1)
    full = "draft accepted to 100 %"
    useless = "draft accepted to   0 %"
    print(f"one decode step of the plain call: {step_ms * 1e3:.1f} us; prefill + head + accept over prompt + {N} draft ids: {med(full, 'prefill_ms'):.3f} ms "
          f"(the plain call's prefill: {med('plain call', 'prefill_ms'):.3f} ms)")
    print(f"break-even tail = prefill / step = {med(full, 'prefill_ms') / step_ms:.2f} ids -> DRAFT_MIN_TAIL = {math.ceil(med(full, 'prefill_ms') / step_ms)} at this batch")
    print(f"a useless draft costs {med(useless, 'total_ms') - plain_total:+.3f} ms on the whole call ({100.0 * (med(useless, 'total_ms') / plain_total - 1.0):+.2f} %)")
    eng.close()


if __name__ == "__main__":
    main()
