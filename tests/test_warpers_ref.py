"""CPU: tests/warpers_ref.py -- the float64 restatement the warper tests measure the kernel with -- pinned three ways: (a) against
transformers' own classes where transformers is importable, (b) against the committed tests/golden/warpers_cases.npz (what those
classes produced when tools/gen_golden_warpers.py ran), (c) by hand cases.  A decision inside the borderline band of its threshold
(`Chain.borderline`) is left out of (a) and (b); at most 2 % of the rows may be."""
import os

import numpy as np
import pytest

import warpers_ref as wr


def _cases(golden_dir):
    g = np.load(os.path.join(golden_dir, "warpers_cases.npz"))
    R = g["raw"].shape[0]
    full = np.full((R, 1280), -np.inf)
    np.put_along_axis(full, g["live"].astype(np.int64), g["raw"].astype(np.float64), 1)
    hists = [g["hist"][r, :g["hist_len"][r]] for r in range(R)]
    vals = {k: float(g["value_" + k]) for k in ("min_p", "typical_p", "epsilon_cutoff", "eta_cutoff", "top_p")}
    return g, full, hists, vals, dict(temperature=float(g["temperature"]), top_k=int(g["top_k"]))


def _restated(full, hists, r, base, **kw):
    ch = wr.chain(full[r], hists[r], **base, **kw)
    return ch


def test_restatement_matches_the_committed_transformers_results(golden_dir):
    g, full, hists, vals, base = _cases(golden_dir)
    R = full.shape[0]
    live = g["live"].astype(np.int64)
    for name in ("min_p", "typical_p", "epsilon_cutoff", "eta_cutoff", "chain", "ngram"):
        left_out, bites = 0, 0
        for r in range(R):
            if name == "chain":
                ch = _restated(full, hists, r, base, **vals, no_repeat_ngram_size=int(g["value_no_repeat_ngram_size"]))
            elif name == "ngram":
                ch = wr.chain(full[r], hists[r], do_sample=False, no_repeat_ngram_size=2)
            else:
                ch = _restated(full, hists, r, base, **{name: vals[name]})
            if ch.borderline:
                left_out += 1
                continue
            got = ch.scores[live[r]]
            assert np.array_equal(np.isfinite(got), g[name + "_keep"][r]), (name, r)
            keep = g[name + "_keep"][r]
            # (the restatement divides by the temperature as the kernel holds it, 0.9f: 2.6e-8 from the classes' 0.9)
            assert np.allclose(got[keep], g[name + "_scores"][r][keep], rtol=1e-7, atol=1e-7), (name, r)
            bites += ch.removed.get(name if name not in ("chain", "ngram") else "no_repeat_ngram_size", 0) >= 1
        assert left_out <= 0.02 * R, (name, left_out)
        assert bites >= 0.25 * R, (name, bites)     # a fixture in which a warper removes nothing pins nothing


def test_restatement_matches_transformers_classes(golden_dir):
    torch = pytest.importorskip("torch")
    lp = pytest.importorskip("transformers.generation.logits_process")
    _, full, hists, vals, base = _cases(golden_dir)
    make = dict(min_p=lambda v: lp.MinPLogitsWarper(v), typical_p=lambda v: lp.TypicalLogitsWarper(mass=v),
                epsilon_cutoff=lambda v: lp.EpsilonLogitsWarper(v), eta_cutoff=lambda v: lp.EtaLogitsWarper(v))
    g = np.random.default_rng(7)
    for name in make:
        for v in (vals[name], {"min_p": 0.3, "typical_p": 0.5, "epsilon_cutoff": 0.02, "eta_cutoff": 0.05}[name]):
            left_out = 0
            for r in range(full.shape[0]):
                s = full[r] * g.uniform(0.5, 2.0)
                ch = wr.chain(s, hists[r], **base, **{name: v})
                if ch.borderline:
                    left_out += 1
                    continue
                ids = torch.from_numpy(np.asarray(hists[r], np.int64))[None]
                x = torch.from_numpy(s.copy())[None]
                x = lp.TopKLogitsWarper(base["top_k"])(ids, lp.TemperatureLogitsWarper(base["temperature"])(ids, x))
                ref = make[name](v)(ids, x)[0].numpy()
                assert np.array_equal(np.isfinite(ref), np.isfinite(ch.scores)), (name, v, r)
            assert left_out <= 0.02 * full.shape[0], (name, v, left_out)
    for n in (1, 2, 3):
        for r in range(full.shape[0]):
            ids = torch.from_numpy(np.asarray(hists[r], np.int64))[None]
            ref = lp.NoRepeatNGramLogitsProcessor(n)(ids, torch.from_numpy(full[r].copy())[None])[0].numpy()
            got = wr.chain(full[r], hists[r], do_sample=False, no_repeat_ngram_size=n).scores
            assert np.array_equal(np.isfinite(ref), np.isfinite(got)), (n, r)


def test_hand_cases():
    inf = np.inf
    # ties at the maximum: epsilon / eta / min_p keep every score equal to it
    s = np.log(np.array([0.3, 0.3, 0.2, 0.1, 0.1]))
    assert np.isfinite(wr.epsilon_cut(s, 0.5)[0]).tolist() == [True, True, False, False, False]
    assert np.isfinite(wr.min_p_cut(s, 1.0)[0]).tolist() == [True, True, False, False, False]
    assert np.isfinite(wr.min_p_cut(s, 0.5)[0]).tolist() == [True, True, True, False, False]      # 0.2 >= 0.5 * 0.3
    H = wr.entropy(s)
    eta = min(0.25, np.sqrt(0.25) * np.exp(-H))
    assert np.isfinite(wr.eta_cut(s, 0.25)[0]).tolist() == [bool(p >= eta) for p in (0.3, 0.3, 0.2, 0.1, 0.1)]
    # typical: d = |-log p - H|; p = (0.5, 0.25, 0.125, 0.125): H = 1.75 bits; d in bits = (0.75, 0.25, 1.25, 1.25)
    s = np.log(np.array([0.5, 0.25, 0.125, 0.125]))
    assert np.isfinite(wr.typical_cut(s, 0.2)[0]).tolist() == [False, True, False, False]          # the smallest d alone holds 0.25 >= 0.2
    assert np.isfinite(wr.typical_cut(s, 0.3)[0]).tolist() == [True, True, False, False]           # the top token is NOT always kept at 0.2
    assert np.isfinite(wr.typical_cut(s, 0.8)[0]).tolist() == [True, True, True, True]             # the tie group enters together
    # typical_p never reached (removed tokens carry no mass; rounding keeps the total below the target): keep all
    assert np.isfinite(wr.typical_cut(np.array([0.0, -inf, 0.0]), 1.0 + 1e-9)[0]).tolist() == [True, False, True]
    # n-gram bans: n = 1 bans every generated token; c = n - 1 bans nothing; c = n bans on a match of the last n - 1
    assert wr.banned_ngram_tokens([4, 7, 4], 1) == [4, 7]
    assert wr.banned_ngram_tokens([], 1) == [] and wr.banned_ngram_tokens([4, 7], 3) == []
    assert wr.banned_ngram_tokens([4, 7, 4], 3) == [] and wr.banned_ngram_tokens([4, 4, 4], 3) == [4]
    assert wr.banned_ngram_tokens([1, 2, 3, 1, 2], 3) == [3] and wr.banned_ngram_tokens([1, 2, 9, 1], 2) == [2]
    # greedy rows ignore the probability warpers and keep the ban
    ch = wr.chain(np.array([3.0, 2.0, 1.0]), [0], do_sample=False, min_p=0.9, no_repeat_ngram_size=1)
    assert ch.token == 1 and "min_p" not in ch.removed
