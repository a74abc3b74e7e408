"""Reference side of the scoring tests (q3a_score*): the fp32 oracle teacher-forced on a given transcript, reduced in float64."""
import numpy as np
import torch

V = 151936
EOS = 151645
AUDIO_PAD = 151676


def reduce_logits(logits, targets):
    """Rows of fp32 logits [n][V] and the n target ids -> float64 lp, int top_id, float64 top_lp, float64 top-1 / top-2 margin."""
    t = np.asarray(targets, dtype=np.int64)
    if len(t) == 0:
        z = np.zeros(0)
        return z, np.zeros(0, np.int64), z.copy(), z.copy()
    x = np.asarray(logits, dtype=np.float64).reshape(len(t), -1)
    m = x.max(axis=1)
    lse = m + np.log(np.exp(x - m[:, None]).sum(axis=1))
    top = x.argmax(axis=1)  # numpy returns the first index of the maximum: the library's tie rule
    part = np.partition(x, -2, axis=1)
    return x[np.arange(len(t)), t] - lse, top, m - lse, part[:, -1] - part[:, -2]


def oracle_score(orc, clip, targets, prefix=None):
    """(lp, top_id, top_lp, margin, logits) of `targets` for `clip`: step i of the oracle's greedy loop fed targets[:i] instead of
    its own argmax.  lp / top_lp / margin float64 [n], logits fp32 [n][V]."""
    targets = [int(t) for t in targets]
    n = len(targets)
    if n == 0:
        lp, top, top_lp, margin = reduce_logits(np.zeros((0, V), np.float32), [])
        return lp, top, top_lp, margin, np.zeros((0, V), np.float32)
    res = orc.transcribe_ids(clip, prefix, forced_ids=targets[:-1], last_only=True)
    assert len(res.step_logits) == n
    logits = torch.stack(res.step_logits).numpy().astype(np.float32)
    lp, top, top_lp, margin = reduce_logits(logits, targets)
    return lp, top, top_lp, margin, logits


def ragged_lens(B):
    """The issue's ragged target lengths: 3, 8, 13, 4, ... (0 at i = 5, 1 at i = 8; 210 rows at B = 32)."""
    return [(5 * i + 3) % 14 for i in range(B)]


def perturb(t):
    return (int(t) * 48271 + 12345) % V
