"""Reference side of the beam-search tests (include/q3asr.h "beam search"): one round restated in numpy with float32 arithmetic and
the header's ordering and slot rules, the top-W selection of a row of logits, and a CPU beam search over the fp32 oracle."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import q3asr_oracle as O

EOS_IDS = (151643, 151645)
NONE = -1  # "no token": the candidate a finished hypothesis contributes


def topk_ref(logits, W):
    """Rows of fp32 logits [S][V] -> (ids int32 [S][W] by larger logit then smaller id, lp float64 [S][W] = log_softmax in float64)."""
    x = np.asarray(logits, dtype=np.float32)
    S, V = x.shape
    ids = np.zeros((S, W), np.int32)
    lp = np.zeros((S, W), np.float64)
    for s in range(S):
        xd = x[s].astype(np.float64)
        cand = np.flatnonzero(xd >= np.partition(xd, V - W)[V - W])  # everything that ties with or beats the W-th largest value
        order = cand[np.lexsort((cand, -xd[cand]))][:W]  # last key first: larger logit, then smaller id (-inf last)
        ids[s] = order
        m = xd.max()
        lp[s] = (xd[order] - m) - np.log(np.exp(xd - m).sum())
    return ids, lp


def _candidates(topk_ids, topk_lp, score, finished, u, W):
    """(score float32, parent slot, token, lp float32) of utterance u's candidates, unordered."""
    out = []
    for s in range(W):
        q = u * W + s
        if finished[q]:
            out.append((np.float32(score[q]), s, NONE, np.float32(0)))
        elif score[q] != -np.inf:  # live; an empty slot produces no candidates
            for k in range(W):
                lp = np.float32(topk_lp[q, k])
                out.append((np.float32(np.float32(score[q]) + lp), s, int(topk_ids[q, k]), lp))
    return out


def rank_key(c):
    """Larger score, then smaller parent slot, then smaller token id ("none" first)."""
    return (-float(c[0]), c[1], c[2])


def assign_slots(parents, W):
    """Survivors in rank order (their parent slots) -> the slot each takes: its parent's if still free, the rest the free slots ascending."""
    slot = [None] * len(parents)
    taken = set()
    for r, p in enumerate(parents):
        if p not in taken:
            slot[r] = p
            taken.add(p)
    for r in range(len(parents)):
        if slot[r] is None:
            slot[r] = min(j for j in range(W) if j not in taken)
            taken.add(slot[r])
    return slot


def beam_round(topk_ids, topk_lp, score, finished, W, cands=None):
    """One round of U x W slots.  topk_ids / topk_lp [S][W], score float32 [S], finished uint8 [S] -> dict of parent (sequence
    index), token (-1: none), score, finished, lp per sequence, and copies = survivors that left their parent's slot.
    cands: per utterance an explicit candidate list instead of the tables' (the brute-force check)."""
    topk_ids, topk_lp = np.asarray(topk_ids), np.asarray(topk_lp, dtype=np.float32)
    score, finished = np.asarray(score, dtype=np.float32), np.asarray(finished, dtype=np.uint8)
    S = len(score)
    U = S // W
    out = {"parent": np.arange(S, dtype=np.int32), "token": np.full(S, NONE, np.int32), "score": np.full(S, -np.inf, np.float32),
           "finished": np.zeros(S, np.uint8), "lp": np.zeros(S, np.float32), "copies": 0, "min_gap": np.inf}
    for u in range(U):
        c = sorted(cands[u] if cands is not None else _candidates(topk_ids, topk_lp, score, finished, u, W), key=rank_key)
        for a, b in zip(c[:W], c[1:W + 1]):  # gaps between neighbouring candidates down to rank W + 1
            out["min_gap"] = min(out["min_gap"], float(a[0]) - float(b[0]))
        surv = c[:W]
        for r, j in enumerate(assign_slots([x[1] for x in surv], W)):
            sc, p, tok, lp = surv[r]
            q = u * W + j
            out["parent"][q] = u * W + p
            out["token"][q] = tok
            out["score"][q] = sc
            out["lp"][q] = lp
            out["finished"][q] = 1 if (tok == NONE or tok in EOS_IDS) else 0
            out["copies"] += int(p != j)
    return out


def brute_round(lp_full, score, finished, W):
    """The same round from ALL live-slot x vocabulary candidates (lp_full float32 [S][V]): an independent sort, no top-W tables."""
    lp_full = np.asarray(lp_full, dtype=np.float32)
    S, V = lp_full.shape
    cands = []
    for u in range(S // W):
        c = []
        for s in range(W):
            q = u * W + s
            if finished[q]:
                c.append((np.float32(score[q]), s, NONE, np.float32(0)))
            elif score[q] != -np.inf:
                c += [(np.float32(np.float32(score[q]) + lp_full[q, v]), s, v, lp_full[q, v]) for v in range(V)]
        cands.append(c)
    return beam_round(None, None, score, finished, W, cands=cands)


def initial_state(U, W):
    """Before round 0: only slot 0 of every utterance is live (score 0), the others are empty (score -inf)."""
    score = np.full(U * W, -np.inf, np.float32)
    score[::W] = 0.0
    return score, np.zeros(U * W, np.uint8)


class _Clip:
    """One clip's prompt with the audio rows injected: last-row logits of prompt ++ ids in one causal forward."""

    def __init__(self, orc, clip, prefix=None):
        self.orc, self.tc = orc, orc.cfg.text
        audio = orc.encode(clip)
        self.T = audio.shape[0]
        self.ids, apos = O.build_prompt(self.T, prefix)
        self.audio, self.a0 = audio, apos[0]
        self.embed = O._w(orc.weights, "thinker.model", "embed_tokens.weight")

    @torch.no_grad()
    def logits(self, gen, normed_out=None):
        ids = self.ids + [int(t) for t in gen]
        hidden = F.embedding(torch.tensor(ids, dtype=torch.int64), self.embed)[None].clone()
        hidden[0, self.a0:self.a0 + self.T] = self.audio
        tc = self.tc
        cos, sin = O.compute_mrope_cos_sin(O.build_position_ids(ids), tc.head_dim, tc.rope_theta, tc.mrope_section, tc.mrope_interleaved)
        out = O.text_decoder_forward(self.orc.weights, tc, hidden, cos, sin, O.KvCache(tc.num_hidden_layers), O.create_causal_mask(len(ids), 0),
                                     last_only=True, normed_out=normed_out)
        return out[0, -1].numpy().astype(np.float32)


def oracle_beam_search(orc, clip, W, max_new, prefix=None, states=None):
    """CPU beam search of one utterance over the fp32 oracle: one causal forward per live hypothesis and round; the round itself is
    beam_round on float64 log_softmax tables rounded to float32.  Returns (hyps best first: dicts of ids / score / finished / lps,
    history copies, smallest candidate gap down to rank W + 1 over all rounds).  states (a list): receives per round the final-normed
    last rows (the lm_head's input) of the slots that were live in it."""
    ctx = _Clip(orc, clip, prefix)
    score, finished = initial_state(1, W)
    hist = [[] for _ in range(W)]  # (token, lp) per slot, EOS included
    copies, min_gap = 0, np.inf
    for rnd in range(max_new):
        ids = np.zeros((W, W), np.int32)
        lp = np.zeros((W, W), np.float32)
        for s in range(W):
            if not finished[s] and score[s] != -np.inf:
                normed = [] if states is not None else None
                i, l = topk_ref(ctx.logits([t for t, _ in hist[s]], normed)[None], W)
                if states is not None:
                    states.append((rnd, normed[0].numpy()))
                ids[s], lp[s] = i[0], l[0].astype(np.float32)
        r = beam_round(ids, lp, score, finished, W)
        hist = [hist[int(r["parent"][j])] + ([(int(r["token"][j]), float(r["lp"][j]))] if r["token"][j] != NONE else []) for j in range(W)]
        score, finished = r["score"], r["finished"]
        copies += r["copies"]
        min_gap = min(min_gap, r["min_gap"])
        if finished.all():
            break
    hyps = []
    for j in sorted(range(W), key=lambda j: (-float(score[j]), j)):
        toks = [t for t, _ in hist[j]]
        hyps.append({"ids": toks[:-1] if finished[j] and toks else toks, "score": float(score[j]), "finished": int(finished[j]),
                     "lps": [l for _, l in hist[j]]})
    return hyps, copies, float(min_gap)


def plant_beam_stops(model_dir, clips, W, stop_rounds, max_new, hi=30.0, lo=-10.0):
    """Rewrite the <|endoftext|> row of model_dir's output embedding so that in a width-W search EVERY live hypothesis of clip u has
    EOS as its (overwhelming) best token in round stop_rounds[u] and nowhere before: the states come from the oracle's search on the
    checkpoint as it is (EOS row zero: never selected), which the planted search equals up to that round.  Returns the worst planted
    logits (fire, quiet)."""
    from qwen3_asr_rs_amd import synthetic
    orc = O.AsrOracle(model_dir)
    H, t = [], []
    for clip, stop in zip(clips, stop_rounds):
        st = []
        oracle_beam_search(orc, clip, W, min(stop + 1, max_new), states=st)
        for rnd, h in st:
            H.append(h)
            t.append(hi if rnd == stop else lo)
    H, t = np.stack(H).astype(np.float64), np.asarray(t)
    w, *_ = np.linalg.lstsq(H, t, rcond=1e-4)
    stored = synthetic.overwrite_row(model_dir, synthetic.output_embedding_key(model_dir), synthetic.ENDOFTEXT_ID, w.astype(np.float32))
    got = H @ stored.astype(np.float64)
    return float(got[t == hi].min()), float(got[t == lo].max())
