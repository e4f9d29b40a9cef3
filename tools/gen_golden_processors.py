"""TEST INFRASTRUCTURE ONLY -- never imported by the product path.

The fixture of the talker's remaining HF logits processors (sequence_bias, bad_words_ids, min_length, forced_eos_token_id,
exponential_decay_length_penalty, begin_suppress_tokens: tests/test_processors_*.py).  Needs the reference tree and transformers, like
tools/gen_golden_warpers.py; the file it writes is committed.

    python tools/gen_golden_processors.py                          # writes the file from the seeds recorded in CASES
    python tools/gen_golden_processors.py --search a START STOP    # the prompt seeds of a range that keep case a's rules

tests/golden/talker_tiny_processors.npz -- the REFERENCE's own talker (oracle/gen_golden.py: `ref_talker`) at `synth.talker_tiny()`,
fp32, greedy, ONE REQUEST PER RUN (HF has no per-row values), each run with the request's own generate() keywords; the runs of a case
are stacked into 4 rows.  The processors of a run are the list transformers' own `GenerationMixin._get_logits_processor` builds from a
`GenerationConfig` holding those keywords -- its classes, its order, its gating -- with max_length = the request's limit and an
embeds-only prompt (input_ids_seq_length 0).  The loop around `talker.forward` is this file's, the greedy `_sample` restated as in
tools/gen_golden_warpers.py: HF 5.x's own `_sample` does not drive the reference talker, which was written against 4.57.3 (its decode
step fails on the attention mask's length), so generate() itself cannot be the driver here.

Per case: the inputs, every request's keywords (JSON), limits and EOS floors, tokens (eos behind a request's end), codes, the cb-0
top-2 margins after the processors, and the tokens and margins of the same requests WITHOUT the controls.  Rules, asserted here and
again in the tests: every cb-0 decision has a margin >= 1e-3; every request with a control on differs from its plain run in at least
one token; a decay request ends on EOS earlier than its plain run; a forced-EOS request's last token is EOS at limit - 1, and the
limits of a case differ; a bad-word and a bias sequence of length 3 fire; a begin-suppressed token is the plain run's first token."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, ROOT)
import synth  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
REP, MARGIN_EXEMPT, N_TRAIL = 1.05, 1e-3, 3
# Controls are written in terms of the request's PLAIN run (p[i]: its token i), so that they fire: `make(p, eos)` -> generate() keywords.
# `floor`: min_new_tokens of the request (HF's MinNewTokensLength; above the limit: EOS blocked throughout, as in the other goldens).
CASES = {
    "a": dict(seed=302, lens=[9, 12, 5, 7], limits=[13, 13, 13, 13], floors=[14, 14, 2, 14], make=[
        lambda p, eos: dict(sequence_bias={(p[1], p[2], p[3]): -30.0, (p[2], p[3]): 2.0, (p[6],): -1.5}),
        lambda p, eos: dict(bad_words_ids=[[p[1], p[2], p[3]], [eos], [p[7]]]),
        lambda p, eos: dict(begin_suppress_tokens=[p[0], 7], exponential_decay_length_penalty=(1, 3.0)),
        lambda p, eos: dict()]),
    "b": dict(seed=301, lens=[6, 8, 11, 7], limits=[9, 12, 7, 11], floors=[2, 2, 8, 12], make=[
        lambda p, eos: dict(forced_eos_token_id=eos, min_length=12),
        lambda p, eos: dict(exponential_decay_length_penalty=(2, 2.5)),
        lambda p, eos: dict(begin_suppress_tokens=[p[0]]),
        lambda p, eos: dict(sequence_bias=[[[p[2]], -25.0], [[p[0], p[1]], 3.0]], bad_words_ids=[[p[4], p[5]]], forced_eos_token_id=eos)]),
}


def processors_of(t, limit, floor, kw):
    """transformers' own processor list for one request's generate() keywords."""
    import warnings
    import torch
    import transformers
    from transformers.generation.utils import GenerationMixin

    class Host(GenerationMixin):
        class config:
            is_encoder_decoder = False

    eos = t.codec_eos_token_id
    suppress = [i for i in range(t.vocab_size - 1024, t.vocab_size) if i != eos]
    gc = transformers.GenerationConfig(do_sample=False, max_length=limit, min_new_tokens=floor, eos_token_id=eos, repetition_penalty=REP,
                                       suppress_tokens=suppress, **kw)
    gc._eos_token_tensor = torch.tensor([eos])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return Host()._get_logits_processor(generation_config=gc, input_ids_seq_length=0, encoder_input_ids=None,
                                            prefix_allowed_tokens_fn=None, logits_processor=[], device="cpu")


def run_one(talker, t, embeds, mask, trailing, tts_pad, limit, floor, kw):
    """Greedy `_sample` around the reference talker.forward for ONE request: `limit` tokens at most, stopping at EOS.  Returns (codes of
    the frames in front of the last token, tokens, cb-0 top-2 margins after the processors)."""
    import torch
    procs = processors_of(t, limit, floor, kw)
    eos = t.codec_eos_token_id
    T = embeds.shape[1]
    talker.rope_deltas = None
    o = talker(inputs_embeds=embeds, attention_mask=mask, use_cache=True, output_hidden_states=True, trailing_text_hidden=trailing,
               tts_pad_embed=tts_pad)
    generated = torch.zeros(1, 0, dtype=torch.long)
    frames, margins = [], []
    for step in range(limit):
        s = procs(generated, o.logits[:, -1].float().clone())
        top2 = torch.topk(s, 2, dim=-1)[0]
        margins.append(float(top2[0, 0] - top2[0, 1]))
        tok = torch.argmax(s, dim=-1)
        generated = torch.cat((generated, tok[:, None]), dim=1)
        if step == limit - 1 or int(tok) == eos:
            break
        mask = torch.cat([mask, mask.new_ones(1, 1)], 1)
        o = talker(input_ids=tok[:, None], attention_mask=mask, past_key_values=o.past_key_values, use_cache=True,
                   cache_position=torch.tensor([T + step]), past_hidden=o.past_hidden, generation_step=o.generation_step,
                   trailing_text_hidden=trailing, tts_pad_embed=tts_pad, output_hidden_states=True, subtalker_dosample=False,
                   subtalker_top_k=None, subtalker_top_p=None, subtalker_temperature=None)
        frames.append(o.hidden_states[1][0])
    codes = torch.stack(frames).numpy() if frames else np.zeros((0, t.num_code_groups), np.int64)
    return codes, generated[0].numpy(), np.array(margins)


def jsonable(kw):
    """generate() keywords as JSON: a sequence_bias dict becomes HF's list form (same order)."""
    out = {}
    for k, v in kw.items():
        if k == "sequence_bias" and isinstance(v, dict):
            v = [[[int(t) for t in ids], float(b)] for ids, b in v.items()]
        out[k] = v
    return json.loads(json.dumps(out, default=lambda x: int(x) if isinstance(x, (np.integer,)) else list(x)))


def fired_len3(kw, key, tokens):
    """whether a length-3 sequence of `key` matched the history of some step of the run (its first two tokens generated, back to back,
    with at least three tokens generated when the next one is chosen)"""
    seqs = kw.get(key) or []
    seqs = [list(k) for k in seqs] if isinstance(seqs, dict) else [list(s[0]) if key == "sequence_bias" else list(s) for s in seqs]
    h = [int(x) for x in tokens]
    return any(len(s) == 3 and any(h[c - 2:c] == s[:2] for c in range(3, len(h))) for s in seqs)


def try_seed(talker, t, name, case, seed):
    import torch
    eos = t.codec_eos_token_id
    B, L = len(case["lens"]), max(case["limits"])
    emb, mask, trailing, pad = synth.rand_prompt(np.random.default_rng(seed), t, case["lens"], N_TRAIL, scale=0.5)
    T = emb.shape[1]
    tokens, plain = np.full((B, L), eos, np.int64), np.full((B, L), eos, np.int64)
    margin, pmargin = np.full((B, L), np.inf), np.full((B, L), np.inf)
    codes = np.zeros((B, L - 1, t.num_code_groups), np.int64)
    n_tok, controls = [], []
    with torch.no_grad():
        for b in range(B):
            drop = T - case["lens"][b]
            a = (emb[b:b + 1, drop:], mask[b:b + 1, drop:], trailing[b:b + 1], pad)
            _, pt, pm = run_one(talker, t, *a, case["limits"][b], case["floors"][b], {})
            if len(pt) < case["limits"][b]:
                print(f"case {name} seed {seed} row {b}: the plain run ends on EOS at {len(pt) - 1}: refused", flush=True)
                return None
            kw = case["make"][b]([int(x) for x in pt], eos)
            c, tk, m = run_one(talker, t, *a, case["limits"][b], case["floors"][b], kw)
            tokens[b, :len(tk)], margin[b, :len(m)], codes[b, :len(c)] = tk, m, c
            plain[b, :len(pt)], pmargin[b, :len(pm)] = pt, pm
            n_tok.append(len(tk))
            controls.append(jsonable(kw))
    lo = min(float(margin.min()), float(pmargin.min()))
    print(f"case {name} seed {seed}: smallest cb-0 margin {float(margin.min()):.2e} (plain {float(pmargin.min()):.2e}), tokens {n_tok}", flush=True)
    if lo < MARGIN_EXEMPT:
        return None
    ok = check_rules(dict(tokens=tokens, tokens_plain=plain, limits=case["limits"], controls=controls), eos, name)
    if not ok:
        return None
    return {f"{name}_embeds": emb.numpy(), f"{name}_mask": mask.numpy(), f"{name}_trailing": trailing.numpy(), f"{name}_tts_pad": pad.numpy(),
            f"{name}_seed": seed, f"{name}_limits": np.array(case["limits"], np.int32), f"{name}_floors": np.array(case["floors"], np.int32),
            f"{name}_controls": json.dumps(controls), f"{name}_codes": codes, f"{name}_tokens": tokens, f"{name}_n_tokens": np.array(n_tok, np.int32),
            f"{name}_margin": margin, f"{name}_tokens_plain": plain, f"{name}_margin_plain": pmargin}


def check_rules(c, eos, name, say=print):
    """The fixture's rules on one case (tokens, tokens_plain, limits, controls); the tests assert them again on the committed file."""
    bad = []
    for b, kw in enumerate(c["controls"]):
        tk, pt, lim = c["tokens"][b], c["tokens_plain"][b], int(c["limits"][b])
        if kw and np.array_equal(tk[:lim], pt[:lim]):
            bad.append(f"row {b}: the controls never change a token")
        if not kw and not np.array_equal(tk, pt):
            bad.append(f"row {b}: no control, but the tokens differ")
        if "exponential_decay_length_penalty" in kw and "forced_eos_token_id" not in kw:
            end = int(np.argmax(tk == eos)) if (tk[:lim] == eos).any() else lim
            if not (end < lim - 1 and eos not in pt[:lim - 1]):
                bad.append(f"row {b}: the decay does not end the request before its plain run")
        if "forced_eos_token_id" in kw and not (tk[lim - 1] == eos and eos not in tk[:lim - 1] and pt[lim - 1] != eos):
            bad.append(f"row {b}: forced EOS is not what ends the request at limit - 1")
        if "begin_suppress_tokens" in kw and int(pt[0]) not in kw["begin_suppress_tokens"]:
            bad.append(f"row {b}: the plain run's first token is not begin-suppressed")
    for b in bad:
        say(f"case {name}: {b}")
    return not bad


def check_file_rules(g, eos):
    """The rules over the whole file: per case as above; a forced-EOS case has differing limits; over all cases a bad-word and a bias
    sequence of length 3 fire (against the PLAIN run's history, which the controlled run shares up to that step)."""
    fired = {"sequence_bias": False, "bad_words_ids": False}
    for name in CASES:
        c = dict(tokens=g[f"{name}_tokens"], tokens_plain=g[f"{name}_tokens_plain"], limits=g[f"{name}_limits"],
                 controls=json.loads(str(g[f"{name}_controls"])))
        assert float(g[f"{name}_margin"].min()) >= MARGIN_EXEMPT and float(g[f"{name}_margin_plain"].min()) >= MARGIN_EXEMPT, name
        assert check_rules(c, eos, name), name
        if any("forced_eos_token_id" in kw for kw in c["controls"]):
            assert len(set(int(x) for x in c["limits"])) > 1, name
        for b, kw in enumerate(c["controls"]):
            for key in fired:
                fired[key] = fired[key] or fired_len3(kw, key, c["tokens_plain"][b])
    assert all(fired.values()), fired


def _talker():
    from gen_golden import ref_talker
    t = synth.talker_tiny()
    w = synth.talker_weights(t)
    return t, w, ref_talker(t, w)


def generate():
    t, w, talker = _talker()
    out = {"weights_checksum": synth.weights_checksum(w)}
    import transformers
    out["transformers_version"] = transformers.__version__
    for name, case in CASES.items():
        entries = try_seed(talker, t, name, case, case["seed"])
        assert entries is not None, f"case {name}: seed {case['seed']} breaks a rule: find another with --search {name} START STOP"
        out.update(entries)
    check_file_rules(out, t.codec_eos_token_id)
    path = os.path.join(GOLDEN, "talker_tiny_processors.npz")
    np.savez_compressed(path, **out)
    print(f"-> {path}: {os.path.getsize(path)} bytes")


def search(name, start, stop, step=1):
    t, _, talker = _talker()
    for seed in range(start, stop, step):
        if try_seed(talker, t, name, CASES[name], seed) is not None:
            print(f"case {name}: seed {seed} passes", flush=True)


if __name__ == "__main__":
    if "--search" in sys.argv:
        i = sys.argv.index("--search")
        search(sys.argv[i + 1], *[int(x) for x in sys.argv[i + 2:i + 5]])
    else:
        generate()
