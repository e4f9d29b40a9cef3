"""CPU: tests/processors_ref.py -- the float64 restatement the processor tests measure the kernel with -- pinned (a) against
transformers' own classes, instantiated in `_get_logits_processor` order, on random scores and histories at V = 1280, (b) against
`_get_logits_processor`'s own list for one configuration, so that the order itself is pinned, (c) by hand cases."""
import numpy as np
import pytest

import processors_ref as pr

V, EOS = 1280, 1279


def _rows(seed, R=48):
    """R rows of Gaussian scores (scales 1 and 3; every token live, so that a bias always moves a score), histories of up to 24 tokens
    over six tokens so that suffixes repeat."""
    g = np.random.default_rng(seed)
    raw = (g.standard_normal((R, V)) * np.where(np.arange(R) % 2 == 0, 1.0, 3.0)[:, None]).astype(np.float32).astype(np.float64)
    pool = [g.choice(V - 1, 6, replace=False) for _ in range(R)]
    # (every sixth row has no history yet: the step at which the begin suppression acts)
    hists = [[int(x) for x in pool[r][g.integers(0, 6, 0 if r % 6 == 0 else g.integers(1, 24))]] for r in range(R)]
    return g, raw, pool, hists


def _config(g, pool, hist):
    """One row's controls: sequences over the row's few history tokens (so that they fire), in both of HF's forms."""
    p = [int(x) for x in pool]
    seqs = {(p[0],): 2.5, (p[1], p[2]): -3.0, (p[2], p[2]): 1.25, (p[0], p[1], p[2]): 4.0, (p[3], p[2]): 0.75}
    if len(hist) >= 2:       # two sequences ending in one token that both match the history's end
        seqs[(hist[-1], p[5])] = 1.5
        seqs[(hist[-2], hist[-1], p[5])] = -0.5
    bias = seqs if g.integers(0, 2) else [[list(k), v] for k, v in seqs.items() if all(t > 0 for t in k)]
    bad = [[p[4]], [EOS], [p[1], p[3]], [p[0], p[0], p[1]]] + ([[hist[-1], p[2]]] if hist else [])
    return dict(sequence_bias_=bias, bad_words_ids=bad, begin_suppress_tokens=[p[0], p[5], 7],
                exponential_decay_length_penalty=(int(g.integers(0, 12)), float(g.choice([1.05, 1.5, 0.8]))),
                min_length=int(g.integers(0, 16)), forced_eos_token_id=EOS)


def _hf_chain(lp, torch, cfg, hist, raw, limit, rep, ngram, min_new, suppress):
    ids = torch.tensor([hist], dtype=torch.long)
    procs = [lp.SequenceBiasLogitsProcessor(sequence_bias=cfg["sequence_bias_"]), lp.RepetitionPenaltyLogitsProcessor(penalty=rep),
             lp.NoRepeatNGramLogitsProcessor(ngram), lp.NoBadWordsLogitsProcessor(cfg["bad_words_ids"], torch.tensor([EOS]))]
    if cfg["min_length"] > 0:
        procs.append(lp.MinLengthLogitsProcessor(cfg["min_length"], torch.tensor([EOS])))
    procs += [lp.MinNewTokensLengthLogitsProcessor(0, min_new, torch.tensor([EOS])), lp.ForcedEOSTokenLogitsProcessor(limit, EOS),
              lp.ExponentialDecayLengthPenalty(cfg["exponential_decay_length_penalty"], torch.tensor([EOS]), 0),
              lp.SuppressTokensLogitsProcessor(suppress), lp.SuppressTokensAtBeginLogitsProcessor(cfg["begin_suppress_tokens"], 0)]
    s = torch.from_numpy(raw[None].copy())
    for p in procs:
        s = p(ids, s)
    return s[0].numpy()


def test_restatement_matches_transformers_classes():
    torch = pytest.importorskip("torch")
    lp = pytest.importorskip("transformers.generation.logits_process")
    g, raw, pool, hists = _rows(11)
    suppress = list(range(V - 64, V - 1))
    fired = {k: 0 for k in ("sequence_bias", "bad_words_ids", "forced_eos_token_id", "begin_suppress_tokens", "decay")}
    for r in range(raw.shape[0]):
        cfg = _config(g, pool[r], hists[r])
        limit = len(hists[r]) + int(g.integers(1, 4))          # (limit - 1 == cur_len in a third of the rows)
        kw = dict(limit=limit, eos_id=EOS, min_new_tokens=2, suppress=suppress, repetition_penalty_=1.05, no_repeat_ngram_size=2)
        ch = pr.chain(raw[r], hists[r], do_sample=False, **kw, **cfg)
        want = _hf_chain(lp, torch, cfg, hists[r], raw[r], limit, 1.05, 2, 2, suppress)
        assert np.array_equal(np.isfinite(ch.scores), np.isfinite(want)), r
        keep = np.isfinite(want)
        assert np.allclose(ch.scores[keep], want[keep], rtol=1e-12, atol=1e-12), (r, np.abs(ch.scores[keep] - want[keep]).max())
        for k in fired:
            fired[k] += bool(ch.eos_moved) if k == "decay" else ch.removed.get(k, 0) >= 1
    print(f"processors_ref vs transformers: fired {fired} of {raw.shape[0]} rows")
    assert all(v >= 4 for v in fired.values()), fired


def test_the_order_is_get_logits_processors_own():
    """The list transformers' `_get_logits_processor` builds for a configuration that names everything, class by class."""
    torch = pytest.importorskip("torch")
    transformers = pytest.importorskip("transformers")
    from transformers.generation.utils import GenerationMixin

    class Host(GenerationMixin):
        class config:
            is_encoder_decoder = False

    gc = transformers.GenerationConfig(
        sequence_bias={(3, 4): 1.0}, repetition_penalty=1.05, no_repeat_ngram_size=2, bad_words_ids=[[5, 6]], min_length=3,
        min_new_tokens=2, forced_eos_token_id=EOS, exponential_decay_length_penalty=(4, 1.5), suppress_tokens=[9],
        begin_suppress_tokens=[10], eos_token_id=EOS, max_length=20, do_sample=True, temperature=0.9, top_k=50, top_p=0.9, min_p=0.1,
        typical_p=0.9, epsilon_cutoff=3e-3, eta_cutoff=3e-3)
    gc._eos_token_tensor = torch.tensor([EOS])
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        procs = Host()._get_logits_processor(generation_config=gc, input_ids_seq_length=0, encoder_input_ids=None,
                                             prefix_allowed_tokens_fn=None, logits_processor=[], device="cpu")
    names = [type(p).__name__ for p in procs]
    assert names == ["SequenceBiasLogitsProcessor", "RepetitionPenaltyLogitsProcessor", "NoRepeatNGramLogitsProcessor",
                     "NoBadWordsLogitsProcessor", "MinLengthLogitsProcessor", "MinNewTokensLengthLogitsProcessor",
                     "ForcedEOSTokenLogitsProcessor", "ExponentialDecayLengthPenalty", "SuppressTokensLogitsProcessor",
                     "SuppressTokensAtBeginLogitsProcessor", "TemperatureLogitsWarper", "TopKLogitsWarper", "TopPLogitsWarper",
                     "MinPLogitsWarper", "TypicalLogitsWarper", "EpsilonLogitsWarper", "EtaLogitsWarper"], names
    # ... and that list, run on a row, is the restatement with the same settings (greedy part: the processors in front of the bracket)
    g, raw, pool, hists = _rows(12, R=4)
    hist = [3, 4, 5, 3]
    ids = torch.tensor([hist], dtype=torch.long)
    s = torch.from_numpy(raw[:1].copy())
    for p in procs[:10]:
        s = p(ids, s)
    ch = pr.chain(raw[0], hist, do_sample=False, limit=20, eos_id=EOS, min_new_tokens=2, min_length=3, suppress=[9], repetition_penalty_=1.05,
                  no_repeat_ngram_size=2, sequence_bias_={(3, 4): 1.0}, bad_words_ids=[[5, 6]], forced_eos_token_id=EOS,
                  exponential_decay_length_penalty=(4, 1.5), begin_suppress_tokens=[10])
    want = s[0].numpy()
    keep = np.isfinite(want)
    assert np.array_equal(np.isfinite(ch.scores), keep) and np.allclose(ch.scores[keep], want[keep], rtol=1e-12, atol=1e-12)


# ============================================================================================ hand cases
def _flat(n=16, v=0.0):
    return np.full(n, v, np.float64)


def test_a_bias_in_front_of_the_repetition_penalty_changes_which_way_it_acts():
    """SequenceBias -> RepetitionPenalty: a slightly negative score of a token in the history is biased positive first, so the penalty
    DIVIDES where it would have multiplied."""
    s = _flat()
    s[3] = -0.5
    ch = pr.chain(s, [3], do_sample=False, repetition_penalty_=2.0, sequence_bias_={(3,): 1.5})
    assert ch.scores[3] == (-0.5 + 1.5) / 2.0
    assert pr.chain(s, [3], do_sample=False, repetition_penalty_=2.0).scores[3] == -0.5 * 2.0
    # the other order would give -0.5 * 2 + 1.5 = 0.5 as well -- so a second value tells the two apart
    s[3] = -0.25
    assert pr.chain(s, [3], do_sample=False, repetition_penalty_=2.0, sequence_bias_={(3,): 1.5}).scores[3] == 0.625 != -0.25 * 2.0 + 1.5


def test_two_sequences_ending_in_one_token_both_match_and_add_up():
    s = _flat()
    bias = {(1, 2, 9): 1.0, (2, 9): 0.25, (9,): -2.0, (7, 9): 100.0}
    ch = pr.chain(s, [5, 1, 2], do_sample=False, sequence_bias_=bias)
    assert ch.scores[9] == -2.0 + 1.0 + 0.25 and ch.removed["sequence_bias"] == 1
    assert pr.chain(s, [5, 1, 2], do_sample=False, sequence_bias_=[[list(k), v] for k, v in bias.items()]).scores[9] == -0.75


def test_a_sequence_longer_than_the_history_is_ignored():
    s = _flat()
    # HF compares len(sequence) with cur_len: a 3-token sequence needs 3 generated tokens, although only 2 are compared
    assert pr.chain(s, [1, 2], do_sample=False, sequence_bias_={(1, 2, 9): 1.0}).scores[9] == 0.0
    assert pr.chain(s, [0, 1, 2], do_sample=False, sequence_bias_={(1, 2, 9): 1.0}).scores[9] == 1.0
    assert np.isfinite(pr.chain(s, [1, 2], do_sample=False, bad_words_ids=[[1, 2, 9]]).scores[9])
    assert pr.chain(s, [0, 1, 2], do_sample=False, bad_words_ids=[[1, 2, 9]]).scores[9] == -np.inf
    assert pr.chain(s, [], do_sample=False, bad_words_ids=[[9]]).scores[9] == -np.inf          # a single token: at every step


def test_eos_among_the_bad_words_is_dropped():
    s = _flat()
    ch = pr.chain(s, [], do_sample=False, eos_id=15, bad_words_ids=[[15], [4]])
    assert ch.scores[15] == 0.0 and ch.scores[4] == -np.inf
    assert pr.chain(s, [0, 3], do_sample=False, eos_id=15, bad_words_ids=[[3, 15]]).scores[15] == -np.inf      # only the single-token entry


def test_forced_eos_wins_over_an_eos_floor_above_the_limit():
    s = _flat()
    s[2] = 5.0
    kw = dict(do_sample=False, eos_id=15, limit=4, min_new_tokens=10, forced_eos_token_id=15)
    assert pr.chain(s, [1, 1], **kw).token == 2 and pr.chain(s, [1, 1], **kw).scores[15] == -np.inf
    ch = pr.chain(s, [1, 1, 1], **kw)
    assert ch.token == 15 and ch.scores[15] == 0.0 and np.isfinite(ch.scores).sum() == 1
    assert pr.chain(s, [1, 1, 1], **{**kw, "forced_eos_token_id": None}).token == 2
    # the suppress list and the begin suppression come later and still act
    assert np.isfinite(pr.chain(s, [], **{**kw, "limit": 1}, begin_suppress_tokens=[15]).scores).sum() == 0


def test_decay_on_a_negative_eos_score_moves_it_up():
    s = _flat()
    s[15] = -4.0
    kw = dict(do_sample=False, eos_id=15, exponential_decay_length_penalty=(2, 1.5))
    assert pr.chain(s, [1, 1], **kw).scores[15] == -4.0                       # cur_len == start: not yet
    assert pr.chain(s, [1, 1, 1], **kw).scores[15] == -4.0 + 4.0 * 0.5
    assert pr.chain(s, [1] * 5, **kw).scores[15] == -4.0 + 4.0 * (1.5 ** 3 - 1.0) > 0
    s[15] = 2.0
    assert pr.chain(s, [1] * 4, **kw).scores[15] == 2.0 * 1.5 ** 2
    assert pr.chain(s, [1] * 4, **{**kw, "exponential_decay_length_penalty": (2, 0.5)}).scores[15] == 2.0 * 0.25


def test_begin_suppression_acts_at_step_zero_only():
    s = _flat()
    assert pr.chain(s, [], do_sample=False, begin_suppress_tokens=[3, 4]).removed["begin_suppress_tokens"] == 2
    assert pr.chain(s, [7], do_sample=False, begin_suppress_tokens=[3, 4]).removed["begin_suppress_tokens"] == 0
