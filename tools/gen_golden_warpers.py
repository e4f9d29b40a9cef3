"""TEST INFRASTRUCTURE ONLY -- never imported by the product path.

Fixtures for the talker's remaining HF sampling controls (min_p, typical_p, epsilon_cutoff, eta_cutoff, no_repeat_ngram_size:
tests/test_warpers_*.py).  Needs the reference tree and transformers, like oracle/gen_golden.py; the files it writes are committed.

    python tools/gen_golden_warpers.py                               # writes both files from the seeds recorded in CASES
    python tools/gen_golden_warpers.py --search b START STOP [STEP]  # the seeds of a range that keep case b's rules

tests/golden/talker_tiny_ngram.npz -- the REFERENCE's own talker (oracle/gen_golden.py: `ref_talker`) at `synth.talker_tiny()`, greedy
with repetition penalty 1.05 and EOS blocked.  The sampling loop is this file's (oracle/gen_golden.py's `restated_sample_loop` with one
more processor): transformers' own `NoRepeatNGramLogitsProcessor` runs at its place in the chain -- after the repetition penalty, before
the EOS floor and the suppress list -- on each row with that row's n.
  case A: 4 requests, n = [0, 1, 2, 3], 13 token steps;   case B: 2 requests, n = 3, 270 token steps (a history past 256 entries).
Per case: the inputs, codes, tokens, cb-0 top-2 margins after the processors, and the tokens of the same requests WITHOUT the ban.
The generator refuses a seed with a cb-0 margin below 1e-3 (MARGIN_EXEMPT: the comparison rule stops at such a flip and could hide a
failure) and a seed for which some n > 0 request's tokens equal its run without the ban (a ban that never bites proves nothing).

tests/golden/warpers_cases.npz -- 64 logit rows (V = 1280, 257 live, Gaussian, scales 1 and 3) with token histories, and what
transformers' classes make of them in float64: the keep mask and the processed scores of each warper alone (after temperature 0.9
and top-k 50) and of the full chain with top_p 0.9.  Records the transformers version.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, ROOT)
import synth  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
REP, MARGIN_EXEMPT, N_TRAIL = 1.05, 1e-3, 3
# `seed`: the prompt seed of the case, found with --search (most seeds of the 270-step case have a cb-0 decision with a margin below
# MARGIN_EXEMPT among their 540).  `plain_margin`: the tests compare the run WITHOUT the ban token for token too.
CASES = {"a": dict(ngram=[0, 1, 2, 3], lens=[9, 12, 5, 7], steps=13, seed=300, plain_margin=True),
         "b": dict(ngram=[3, 3], lens=[6, 8], steps=270, seed=418, plain_margin=False)}
# the values of the per-warper cases: each removes tokens at temperature 0.9 / top-k 50 on these rows
VALUES = dict(min_p=0.1, typical_p=0.9, epsilon_cutoff=3e-3, eta_cutoff=3e-3)
CHAIN = dict(VALUES, top_p=0.9, no_repeat_ngram_size=2)
TEMPERATURE, TOP_K = 0.9, 50


def ngram_loop(talker, t, embeds, mask, trailing, tts_pad, steps, ngram):
    """Greedy HF `_sample` around the reference talker.forward with the processors RepetitionPenalty -> NoRepeatNGram (transformers'
    class, row b under ngram[b]) -> MinNewTokensLength (EOS blocked throughout) -> SuppressTokens."""
    import torch
    from transformers.generation.logits_process import NoRepeatNGramLogitsProcessor
    eos = t.codec_eos_token_id
    suppress = [i for i in range(t.vocab_size - 1024, t.vocab_size) if i != eos]
    procs = {n: NoRepeatNGramLogitsProcessor(n) for n in set(ngram) if n > 0}
    B, T, _ = embeds.shape
    talker.rope_deltas = None
    o = talker(inputs_embeds=embeds, attention_mask=mask, use_cache=True, output_hidden_states=True, trailing_text_hidden=trailing,
               tts_pad_embed=tts_pad)
    generated = torch.zeros(B, 0, dtype=torch.long)
    frames, margins = [], []
    for step in range(steps):
        s = o.logits[:, -1].float().clone()
        if generated.shape[1] > 0:
            sc = torch.gather(s, 1, generated)
            sc = torch.where(sc < 0, sc * REP, sc / REP)
            s = s.scatter(1, generated, sc)
        for b, n in enumerate(ngram):
            if n > 0:
                s[b:b + 1] = procs[n](generated[b:b + 1], s[b:b + 1])
        s[:, eos] = float("-inf")
        s[:, suppress] = float("-inf")
        top2 = torch.topk(s, 2, dim=-1)[0]
        margins.append((top2[:, 0] - top2[:, 1]).clone())
        tok = torch.argmax(s, dim=-1)
        generated = torch.cat((generated, tok[:, None]), dim=1)
        if step == steps - 1:
            break
        mask = torch.cat([mask, mask.new_ones(B, 1)], 1)
        o = talker(input_ids=tok[:, None], attention_mask=mask, past_key_values=o.past_key_values, use_cache=True,
                   cache_position=torch.tensor([T + step]), past_hidden=o.past_hidden, generation_step=o.generation_step,
                   trailing_text_hidden=trailing, tts_pad_embed=tts_pad, output_hidden_states=True, subtalker_dosample=False,
                   subtalker_top_k=None, subtalker_top_p=None, subtalker_temperature=None)
        frames.append(o.hidden_states[1])
    return torch.stack(frames, dim=1), generated, torch.stack(margins, 1)


def try_seed(talker, t, name, case, seed):
    """One case at one seed: the fixture's entries, or None when the seed breaks a rule (a cb-0 margin below MARGIN_EXEMPT in the run
    with the ban -- and in the run without it where the tests compare that run token for token, `plain_margin` --, or a ban that
    never bites)."""
    import torch
    emb, mask, trailing, pad = synth.rand_prompt(np.random.default_rng(seed), t, case["lens"], N_TRAIL, scale=0.5)
    with torch.no_grad():
        codes, toks, margin = ngram_loop(talker, t, emb, mask, trailing, pad, case["steps"], case["ngram"])
        if float(margin.min()) < MARGIN_EXEMPT:
            print(f"case {name} seed {seed}: smallest cb-0 margin {float(margin.min()):.2e}: refused", flush=True)
            return None
        _, plain, pm = ngram_loop(talker, t, emb, mask, trailing, pad, case["steps"], [0] * len(case["ngram"]))
    bites = [not torch.equal(toks[b], plain[b]) for b, n in enumerate(case["ngram"]) if n > 0]
    print(f"case {name} seed {seed}: smallest cb-0 margin {float(margin.min()):.2e} (plain {float(pm.min()):.2e}), the ban bites: {bites}", flush=True)
    if (case["plain_margin"] and float(pm.min()) < MARGIN_EXEMPT) or not all(bites):
        return None
    for b, n in enumerate(case["ngram"]):
        assert n == 0 or not torch.equal(toks[b], plain[b]), (name, b)
        assert n != 0 or torch.equal(toks[b], plain[b]), (name, b)
    return {f"{name}_embeds": emb.numpy(), f"{name}_mask": mask.numpy(), f"{name}_trailing": trailing.numpy(),
            f"{name}_tts_pad": pad.numpy(), f"{name}_ngram": np.array(case["ngram"], np.int32), f"{name}_seed": seed,
            f"{name}_codes": codes.numpy(), f"{name}_tokens": toks.numpy(), f"{name}_margin": margin.numpy(),
            f"{name}_tokens_plain": plain.numpy(), f"{name}_margin_plain": pm.numpy()}


def _talker():
    from gen_golden import ref_talker
    t = synth.talker_tiny()
    w = synth.talker_weights(t)
    return t, w, ref_talker(t, w)


def gen_ngram():
    t, w, talker = _talker()
    out = {"weights_checksum": synth.weights_checksum(w)}
    for name, case in CASES.items():
        entries = try_seed(talker, t, name, case, case["seed"])
        assert entries is not None, f"case {name}: seed {case['seed']} breaks a rule: find another with --search {name} START STOP"
        out.update(entries)
    path = os.path.join(GOLDEN, "talker_tiny_ngram.npz")
    np.savez_compressed(path, **out)
    print(f"-> {path}: {os.path.getsize(path)} bytes")


def search(name, start, stop, step=1):
    """The seeds start, start + step, ... below stop that keep the rules of case `name` (several processes can share a range)."""
    t, _, talker = _talker()
    for seed in range(start, stop, step):
        if try_seed(talker, t, name, CASES[name], seed) is not None:
            print(f"case {name}: seed {seed} passes", flush=True)


def gen_cases():
    import torch
    import transformers
    from transformers.generation import logits_process as lp
    g = np.random.default_rng(2024)
    R, V, LIVE = 64, 1280, 257
    live = np.stack([np.sort(g.choice(V, LIVE, replace=False)) for _ in range(R)])
    raw = (g.standard_normal((R, LIVE)) * np.where(np.arange(R) % 2 == 0, 1.0, 3.0)[:, None]).astype(np.float32)
    hist_len = g.integers(0, 24, R)
    hist = np.full((R, 24), -1, np.int64)
    for r in range(R):                    # histories over a few live tokens, so that 2-grams repeat
        hist[r, :hist_len[r]] = live[r][g.integers(0, 6, hist_len[r])]
    full = np.full((R, V), -np.inf)
    np.put_along_axis(full, live, raw.astype(np.float64), 1)
    out = dict(live=live.astype(np.int32), raw=raw, hist=hist, hist_len=hist_len.astype(np.int32),
               transformers_version=transformers.__version__, temperature=TEMPERATURE, top_k=TOP_K,
               **{"value_" + k: v for k, v in CHAIN.items()})
    make = dict(min_p=lambda v: lp.MinPLogitsWarper(v), typical_p=lambda v: lp.TypicalLogitsWarper(mass=v),
                epsilon_cutoff=lambda v: lp.EpsilonLogitsWarper(v), eta_cutoff=lambda v: lp.EtaLogitsWarper(v))

    def base(r, ngram=0):
        s = torch.from_numpy(full[r:r + 1].copy())
        ids = torch.from_numpy(hist[r:r + 1, :hist_len[r]])
        if ngram:
            s = lp.NoRepeatNGramLogitsProcessor(ngram)(ids, s)
        s = lp.TemperatureLogitsWarper(TEMPERATURE)(ids, s)
        return ids, lp.TopKLogitsWarper(TOP_K)(ids, s)

    def store(name, rows):
        sc = np.stack([np.take_along_axis(x.numpy(), live[r:r + 1], 1)[0] for r, x in enumerate(rows)])
        out[name + "_keep"] = np.isfinite(sc)
        out[name + "_scores"] = np.where(np.isfinite(sc), sc, -np.inf)

    for k, v in VALUES.items():
        rows = []
        for r in range(R):
            ids, s = base(r)
            rows.append(make[k](v)(ids, s))
        store(k, rows)
    rows = []
    for r in range(R):
        ids, s = base(r, CHAIN["no_repeat_ngram_size"])
        s = lp.TopPLogitsWarper(CHAIN["top_p"])(ids, s)
        for k in ("min_p", "typical_p", "epsilon_cutoff", "eta_cutoff"):
            s = make[k](CHAIN[k])(ids, s)
        rows.append(s)
    store("chain", rows)
    store("ngram", [lp.NoRepeatNGramLogitsProcessor(2)(torch.from_numpy(hist[r:r + 1, :hist_len[r]]), torch.from_numpy(full[r:r + 1].copy()))
                    for r in range(R)])
    path = os.path.join(GOLDEN, "warpers_cases.npz")
    np.savez_compressed(path, **out)
    print(f"-> {path}: {os.path.getsize(path)} bytes, transformers {transformers.__version__}; kept per case: " +
          ", ".join(f"{k[:-5]} {out[k].sum(1).mean():.1f}" for k in out if k.endswith("_keep")))


if __name__ == "__main__":
    if "--search" in sys.argv:
        i = sys.argv.index("--search")
        search(sys.argv[i + 1], *[int(x) for x in sys.argv[i + 2:i + 5]])
    else:
        gen_cases()
        gen_ngram()
