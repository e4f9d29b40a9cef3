"""TEST YARDSTICK: a float64 numpy restatement of the talker's codebook-0 chain with HF generate's remaining sampling controls
(transformers 4.57.3 `_get_logits_processor` order and generation/logits_process.py formulas):

    RepetitionPenalty -> NoRepeatNGram -> MinNewTokensLength -> SuppressTokens ->
    [Temperature -> TopK -> TopP -> MinP -> Typical -> EpsilonCutoff -> EtaCutoff] -> argmax | softmax + draw

One row at a time: `scores` is a 1-d array (-inf = removed), `hist` the row's own generated tokens.  Every softmax is over the scores as
they stand; `min_tokens_to_keep` is 1 everywhere.  Each warper also says how close its decision came to its threshold, so that a test
can leave out the draws no two precisions can agree on (`Chain.borderline`), and how many surviving tokens it removed (`Chain.removed`).
tests/test_warpers_ref.py pins this file against transformers' own classes, the committed tests/golden/warpers_cases.npz and hand cases."""
from dataclasses import dataclass, field

import numpy as np

NEG = -np.inf
REL_BAND = 1e-4        # a probability within this relative distance of a min_p / epsilon / eta threshold is undecidable in fp32
MASS_BAND = 1e-5       # ... and so is a tie group's cumulative mass this close to typical_p / top_p


def softmax(s):
    s = np.asarray(s, np.float64)
    live = np.isfinite(s)
    if not live.any():
        return np.zeros_like(s)
    e = np.where(live, np.exp(np.where(live, s, 0.0) - s[live].max()), 0.0)
    return e / e.sum()


def entropy(s):
    """-sum p log p over the finite entries."""
    p = softmax(s)
    live = p > 0
    lp = np.where(live, np.log(np.where(live, p, 1.0)), 0.0)
    return float(-(p * lp).sum())


def banned_ngram_tokens(hist, n):
    """NoRepeatNGramLogitsProcessor: with c = len(hist), nothing while c < n; else every hist[i + n - 1], 0 <= i <= c - n, whose n - 1
    predecessors equal the last n - 1 tokens.  n = 1 bans every token generated so far."""
    h = [int(x) for x in hist]
    c = len(h)
    if n <= 0 or c < n:
        return []
    suffix = h[c - n + 1:]
    return sorted({h[i + n - 1] for i in range(c - n + 1) if h[i:i + n - 1] == suffix})


def repetition_penalty(s, hist, rep):
    s = np.array(s, np.float64)
    if rep != 1.0 and len(hist):
        idx = np.unique(np.asarray(hist, np.int64))
        s[idx] = np.where(s[idx] < 0, s[idx] * rep, s[idx] / rep)
    return s


def top_k_cut(s, k):
    s = np.array(s, np.float64)
    if k and 0 < k < len(s):
        thr = np.sort(s)[-k]
        s[s < thr] = NEG
    return s


def top_p_cut(s, top_p):
    """TopPLogitsWarper: ascending cumulative softmax <= 1 - top_p is removed; the top token always stays.  Returns (scores, distance of the
    nearest cumulative mass to the cut)."""
    s = np.array(s, np.float64)
    order = np.argsort(s, kind="stable")
    cum = np.cumsum(softmax(s)[order])
    rm = cum <= 1.0 - top_p
    rm[-1] = False
    near = float(np.abs(cum[:-1] - (1.0 - top_p)).min()) if len(s) > 1 else 1.0
    s[order[rm]] = NEG
    return s, near


def _below(s, p, thr):
    """remove p < thr except scores equal to the maximum; (scores, relative distance of the nearest live probability to thr)"""
    s = np.array(s, np.float64)
    live = np.isfinite(s)
    rm = live & (p < thr) & (s < s[live].max())
    near = float(np.abs(p[live] / thr - 1.0).min()) if thr > 0 and live.any() else 1.0
    s[rm] = NEG
    return s, near


def min_p_cut(s, min_p):
    p = softmax(s)
    return _below(s, p, min_p * p.max())


def epsilon_cut(s, eps):
    return _below(s, softmax(s), eps)


def eta_cut(s, eps):
    return _below(s, softmax(s), min(eps, np.sqrt(eps) * np.exp(-entropy(s))))


def typical_cut(s, mass):
    """TypicalLogitsWarper in threshold form: d = |-log p - H|; keep d <= t*, the smallest value of d whose group {d <= t*} has mass >=
    `mass` (never reached: keep all).  Returns (scores, distance of the nearest group mass to `mass`)."""
    s = np.array(s, np.float64)
    live = np.isfinite(s)
    p = softmax(s)
    lp = np.where(live, s - s[live].max() - np.log(np.exp(s[live] - s[live].max()).sum()), NEG)
    H = float(-(p[live] * lp[live]).sum())
    d = np.where(live, np.abs(-np.where(live, lp, 0.0) - H), np.inf)
    vals = np.unique(d[live])
    group = np.array([p[live & (d <= v)].sum() for v in vals])
    reached = np.nonzero(group >= mass)[0]
    near = float(np.abs(group - mass).min())
    if len(reached):
        s[live & (d > vals[reached[0]])] = NEG
    return s, near


@dataclass
class Chain:
    scores: np.ndarray                   # the processed scores (float64, -inf = removed)
    borderline: bool = False             # some keep / remove decision lies inside REL_BAND / MASS_BAND of its threshold
    removed: dict = field(default_factory=dict)     # warper name -> surviving tokens it removed

    @property
    def probs(self):
        return softmax(self.scores)

    @property
    def token(self):
        return int(np.argmax(self.scores))     # greedy: first maximum, like torch.argmax


def chain(raw, hist, *, do_sample=True, temperature=1.0, top_k=0, top_p=1.0, repetition_penalty_=1.0, eos_id=None, min_new_tokens=0,
          suppress=(), min_p=0.0, typical_p=0.0, epsilon_cutoff=0.0, eta_cutoff=0.0, no_repeat_ngram_size=0):
    """The whole chain on one row's raw logits.  Knobs as the kernel takes them: 0 = off for the five new ones."""
    s = repetition_penalty(np.asarray(raw, np.float64), hist, float(repetition_penalty_))
    out = Chain(s)
    n_live = lambda a: int(np.isfinite(a).sum())

    def step(name, new, near=None, band=None):
        out.removed[name] = n_live(out.scores) - n_live(new)
        if near is not None and near < band:
            out.borderline = True
        out.scores = new

    if no_repeat_ngram_size and no_repeat_ngram_size > 0:
        t = np.array(out.scores)
        t[banned_ngram_tokens(hist, int(no_repeat_ngram_size))] = NEG
        step("no_repeat_ngram_size", t)
    t = np.array(out.scores)
    if eos_id is not None and len(hist) < min_new_tokens:
        t[eos_id] = NEG
    if len(suppress):
        t[np.asarray(suppress, np.int64)] = NEG
    out.scores = t
    if not do_sample:
        return out
    if temperature != 1.0:
        out.scores = out.scores / float(np.float32(temperature))
    if top_k:
        step("top_k", top_k_cut(out.scores, int(top_k)))
    if top_p < 1.0:
        step("top_p", *top_p_cut(out.scores, float(np.float32(top_p))), MASS_BAND)
    if min_p > 0.0:
        step("min_p", *min_p_cut(out.scores, float(np.float32(min_p))), REL_BAND)
    if 0.0 < typical_p < 1.0:
        step("typical_p", *typical_cut(out.scores, float(np.float32(typical_p))), MASS_BAND)
    if 0.0 < epsilon_cutoff < 1.0:
        step("epsilon_cutoff", *epsilon_cut(out.scores, float(np.float32(epsilon_cutoff))), REL_BAND)
    if 0.0 < eta_cutoff < 1.0:
        step("eta_cutoff", *eta_cut(out.scores, float(np.float32(eta_cutoff))), REL_BAND)
    return out
