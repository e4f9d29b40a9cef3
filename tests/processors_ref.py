"""TEST YARDSTICK: a float64 numpy restatement of HF generate's remaining logits processors on the talker's codebook-0 chain, composed
with tests/warpers_ref.py in transformers' `_get_logits_processor` order (read from the installed 5.x source; 4.57.3 has the same):

    SequenceBias -> RepetitionPenalty -> NoRepeatNGram -> NoBadWords -> MinLength -> MinNewTokensLength -> ForcedEOS
     -> ExponentialDecayLengthPenalty -> SuppressTokens -> SuppressTokensAtBegin
     -> [Temperature -> TopK -> TopP -> MinP -> Typical -> EpsilonCutoff -> EtaCutoff] -> argmax | softmax + draw

One row at a time, like warpers_ref: `scores` is a 1-d array (-inf = removed), `hist` the row's own generated tokens, cur_len =
len(hist) (the prompt is embeds-only).  tests/test_processors_ref.py pins this file against transformers' own classes and hand cases."""
import numpy as np

import warpers_ref
from warpers_ref import NEG, Chain


def as_bias_dict(sequence_bias):
    """HF's two forms -> {tuple: float}, in listed order (a repeated key keeps its first place and its last value, as a dict does)."""
    if sequence_bias is None:
        return {}
    if isinstance(sequence_bias, dict):
        return {tuple(int(t) for t in k): float(v) for k, v in sequence_bias.items()}
    return {tuple(int(t) for t in s[0]): float(s[1]) for s in sequence_bias}


def sequence_matches(hist, ids):
    """SequenceBiasLogitsProcessor's rule for one sequence: a single token always; a longer one when the history holds at least
    len(ids) tokens and ends in ids[:-1]."""
    n = len(ids)
    if n == 1:
        return True
    if n > len(hist):
        return False
    return [int(x) for x in hist[len(hist) - (n - 1):]] == [int(x) for x in ids[:-1]]


def sequence_bias(s, hist, bias):
    """scores + bias, where bias[last token] sums -- single-token sequences first, then the others in listed order -- the values of the
    sequences that match.  The values are fp32 (torch.tensor(float)), the sums float64 here."""
    s = np.array(s, np.float64)
    add = np.zeros_like(s)
    d = as_bias_dict(bias)
    for single in (True, False):
        for ids, v in d.items():
            if (len(ids) == 1) == single and sequence_matches(hist, ids):
                add[ids[-1]] += float(np.float32(v))
    return s + add


def bad_words(s, hist, words, eos_id):
    """NoBadWordsLogitsProcessor: SequenceBias with -inf, single-token entries equal to eos dropped."""
    s = np.array(s, np.float64)
    for ids in words:
        ids = [int(t) for t in ids]
        if ids == [eos_id]:
            continue
        if sequence_matches(hist, ids):
            s[ids[-1]] = NEG
    return s


def forced_eos(s, cur_len, limit, eos_id):
    s = np.array(s, np.float64)
    if cur_len == limit - 1:
        s[:] = NEG
        s[eos_id] = 0.0
    return s


def exponential_decay(s, cur_len, start, factor, eos_id):
    """Once cur_len > start: x[eos] += |x[eos]| * (factor ** (cur_len - start) - 1), the power as Python evaluates it."""
    s = np.array(s, np.float64)
    if cur_len > start and np.isfinite(s[eos_id]):
        s[eos_id] = s[eos_id] + abs(s[eos_id]) * (pow(float(factor), cur_len - start) - 1.0)
    return s


def begin_suppress(s, cur_len, tokens):
    s = np.array(s, np.float64)
    if cur_len == 0 and len(tokens):
        s[np.asarray(tokens, np.int64)] = NEG
    return s


def chain(raw, hist, *, limit=None, eos_id=None, min_new_tokens=0, min_length=0, suppress=(), repetition_penalty_=1.0,
          no_repeat_ngram_size=0, sequence_bias_=None, bad_words_ids=None, forced_eos_token_id=None,
          exponential_decay_length_penalty=None, begin_suppress_tokens=None, **sampling) -> Chain:
    """The whole chain on one row's raw logits.  `sampling`: warpers_ref.chain's do_sample / temperature / top_k / top_p / min_p /
    typical_p / epsilon_cutoff / eta_cutoff.  `Chain.removed` gains, per processor that is on, the surviving tokens it removed;
    `Chain.eos_moved` says whether a bias or the decay changed the EOS score."""
    hist = [int(x) for x in hist]
    cur = len(hist)
    removed = {}
    live = lambda a: int(np.isfinite(a).sum())
    s = np.asarray(raw, np.float64)
    eos_before = None
    if sequence_bias_ is not None:
        t = sequence_bias(s, hist, sequence_bias_)
        removed["sequence_bias"] = int((t != s).sum())          # (a bias moves scores: the tokens it moved)
        s = t
    s = warpers_ref.repetition_penalty(s, hist, float(repetition_penalty_))
    if no_repeat_ngram_size and no_repeat_ngram_size > 0:
        t = np.array(s)
        t[warpers_ref.banned_ngram_tokens(hist, int(no_repeat_ngram_size))] = NEG
        removed["no_repeat_ngram_size"] = live(s) - live(t)
        s = t
    if bad_words_ids is not None:
        t = bad_words(s, hist, bad_words_ids, eos_id)
        removed["bad_words_ids"] = live(s) - live(t)
        s = t
    s = np.array(s)
    if eos_id is not None and cur < max(int(min_new_tokens or 0), int(min_length or 0)):
        s[eos_id] = NEG
    if forced_eos_token_id is not None:
        t = forced_eos(s, cur, limit, int(forced_eos_token_id))
        removed["forced_eos_token_id"] = live(s) - live(t)
        s = t
    eos_moved = False
    if exponential_decay_length_penalty is not None:
        t = exponential_decay(s, cur, int(exponential_decay_length_penalty[0]), exponential_decay_length_penalty[1], eos_id)
        eos_moved = bool(t[eos_id] != s[eos_id])
        s = t
    if len(suppress):
        s[np.asarray(suppress, np.int64)] = NEG
    if begin_suppress_tokens is not None:
        t = begin_suppress(s, cur, begin_suppress_tokens)
        removed["begin_suppress_tokens"] = live(s) - live(t)
        s = t
    # the bracket: warpers_ref's chain on the processed scores, with everything in front of it off
    out = warpers_ref.chain(s, [], **sampling)
    out.removed = {**removed, **out.removed}
    out.eos_moved = eos_moved
    return out
