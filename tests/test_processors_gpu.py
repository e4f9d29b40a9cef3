"""HF generate's remaining logits processors on the talker's codebook-0 sampler, per request: sequence_bias, bad_words_ids, min_length,
forced_eos_token_id, exponential_decay_length_penalty and begin_suppress_tokens (include/qtts.h: qtts_row_processors,
qtts_talker_set_row_processors; csrc/sampling.hip: sample_warp_kernel; `TalkerEngine.generate(..., bad_words_ids=[...], ...)`).

The yardsticks are tests/processors_ref.py (a float64 restatement, pinned by tests/test_processors_ref.py against transformers' own
classes and `_get_logits_processor`'s own order) and the fixture tools/gen_golden_processors.py wrote.  The test BODIES (`body_*`) take
the device; tests/test_processors_hostemu.py runs the same bodies on the host-emulation build."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import synth
import processors_ref as pr
import test_row_sampling_gpu as rs
from test_gpu_parity import _philox4x32_10, _sampler_slot_order, _suppress, _td, _u_gap, dev  # noqa: F401  (`dev` is a fixture)

pytestmark = pytest.mark.gpu

TOL = rs.TOL
PROC = ("sequence_bias", "bad_words_ids", "min_length", "forced_eos_token_id", "exponential_decay_length_penalty", "begin_suppress_tokens")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _np(x):
    return rs._np(x)


def _tool():
    spec = importlib.util.spec_from_file_location("gen_golden_processors", os.path.join(ROOT, "tools", "gen_golden_processors.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


# ============================================================================================ 1. the reference run
def _case(golden_dir, name):
    g = np.load(os.path.join(golden_dir, "talker_tiny_processors.npz"))
    args = [torch.from_numpy(g[f"{name}_{k}"]) for k in ("embeds", "mask", "trailing", "tts_pad")]
    rows = json.loads(str(g[f"{name}_controls"]))
    ctl = {k: [r.get(k) for r in rows] for k in PROC if any(k in r for r in rows)}
    return g, args, rows, ctl


def _greedy_kw(t, g, name):
    return dict(max_new_tokens=[int(x) for x in g[f"{name}_limits"]], min_new_tokens=[int(x) for x in g[f"{name}_floors"]], do_sample=False,
                subtalker_dosample=False, repetition_penalty=1.05, suppress_tokens=_suppress(t))


def _check_rows(g, name, codes, tokens, eos, rows=None, what=""):
    """Request i of the case against the fixture: every frame in front of its last token and every token but the one at its limit,
    where a table run shows eos whatever was chosen (include/qtts.h); a request that ended on EOS shows it."""
    for i in (range(codes.shape[0]) if rows is None else rows):
        n = int(g[f"{name}_n_tokens"][i])
        ref_t, ref_c = g[f"{name}_tokens"][i], g[f"{name}_codes"][i]
        assert np.array_equal(tokens[i, :n - 1], ref_t[:n - 1]), (what, name, i, tokens[i, :n], ref_t[:n])
        assert np.array_equal(codes[i, :n - 1], ref_c[:n - 1]), (what, name, i)
        if tokens.shape[1] >= n:
            assert tokens[i, n - 1] == eos, (what, name, i)


def body_reference(dev, golden_dir, graph, name):
    """Greedy, fp32, one table call with other controls on every row: codes and tokens are the reference talker's under transformers'
    own processor list for each request's keywords (tests/golden/talker_tiny_processors.npz, whose rules are asserted again here); the
    sampler class is (3, 2); the row without a control equals the plain call, every other row differs from it."""
    t, w = rs._tiny()
    eos = t.codec_eos_token_id
    g, args, rows, ctl = _case(golden_dir, name)
    _tool().check_file_rules(g, eos)
    eng = rs._engine(t, w, dev, torch.float32, graph, 4)
    kw = _greedy_kw(t, g, name)
    out = eng.generate(*args, **kw, **ctl)
    assert eng.sampler_class() == (3, 2) and eng.stats()["row_table_last"] == 1
    codes, tokens = _np(out.codes), _np(out.tokens)
    _check_rows(g, name, codes, tokens, eos)
    plain = eng.generate(*args, **kw)
    assert eng.sampler_class() == (2, 2)
    pc, pt = _np(plain.codes), _np(plain.tokens)
    for i, r in enumerate(rows):
        n = int(g[f"{name}_n_tokens"][i])
        lim = int(g[f"{name}_limits"][i])
        assert np.array_equal(pt[i, :lim - 1], g[f"{name}_tokens_plain"][i, :lim - 1]), i
        # (a table run shows eos at a row's limit whatever was chosen: a request whose ONLY difference is its forced last token -- fixture
        # row b0 -- cannot differ here; every other request with a control does, and the request without one does not)
        same = np.array_equal(tokens[i, :lim - 1], pt[i, :lim - 1]) and np.array_equal(codes[i, :n - 1], pc[i, :n - 1])
        want = np.array_equal(g[f"{name}_tokens"][i, :lim - 1], g[f"{name}_tokens_plain"][i, :lim - 1])
        assert same == want and (want or r), (i, r)
        assert not want or set(r) <= {"forced_eos_token_id", "min_length"}, (i, r)


@pytest.mark.parametrize("name", ["a", "b"])
@pytest.mark.parametrize("graph", [False, True])
def test_processors_are_the_reference_run(dev, golden_dir, graph, name):
    body_reference(dev, golden_dir, graph, name)


def body_streams(dev, golden_dir):
    """The same controls through `generate_stream` packets (case b on 4 rows), and 12 requests -- case b three times over (one call
    has one tts_pad) -- on 4 rows through `schedule="continuous"`: eight requests are admitted into rows whose neighbours are
    mid-utterance, among them two whose begin suppression must land on THEIR step 0 and four whose forced EOS must land at THEIR
    limit - 1 (the limits are 9, 12, 7 and 11)."""
    t, w = rs._tiny()
    eos = t.codec_eos_token_id
    g, args, rows, ctl = _case(golden_dir, "b")
    eng = rs._engine(t, w, dev, torch.float32, True, 4)
    parts = [_np(p) for p in eng.generate_stream(*args, packet_frames=4, **_greedy_kw(t, g, "b"), **ctl)]
    assert eng.sampler_class()[0] == 3
    codes = np.concatenate(parts, axis=1)
    _check_rows(g, "b", codes, np.concatenate([codes[:, :, 0], np.full((4, 1), eos)], 1), eos, what="packets")
    # 12 requests: the prompts of both cases padded to one length
    names = ["b", "b", "b"]
    cases = {n: _case(golden_dir, n) for n in "b"}
    T = max(c[1][0].shape[1] for c in cases.values())
    emb, mask, trail, kws, ctls = [], [], [], [], {k: [] for k in PROC}
    for n in names:
        _, a, rws, _ = cases[n]
        d = T - a[0].shape[1]
        emb.append(torch.nn.functional.pad(a[0], (0, 0, d, 0)))
        mask.append(torch.nn.functional.pad(a[1], (d, 0)))
        trail.append(a[2])
        for k in PROC:
            ctls[k] += [r.get(k) for r in rws]
    lim = [int(x) for n in names for x in cases[n][0][f"{n}_limits"]]
    flo = [int(x) for n in names for x in cases[n][0][f"{n}_floors"]]
    out = eng.generate(torch.cat(emb), torch.cat(mask), torch.cat(trail), args[3], schedule="continuous", packet_frames=2, max_new_tokens=lim,
                       min_new_tokens=flo, do_sample=False, subtalker_dosample=False, repetition_penalty=1.05, suppress_tokens=_suppress(t),
                       **ctls)
    st = eng.last_refill
    assert eng.sampler_class()[0] == 3 and st["streams"] == 1 and st["admitted_rows"] == 8, st
    oc = _np(out.codes)
    toks = np.concatenate([oc[:, :, 0], np.full((12, 1), eos)], 1)
    for j, n in enumerate(names):
        sl = slice(4 * j, 4 * j + 4)
        _check_rows(cases[n][0], n, oc[sl], toks[sl], eos, what=f"continuous {j}")


def test_processors_through_stream_packets_and_the_continuous_schedule(dev, golden_dir):
    body_streams(dev, golden_dir)


# ============================================================================================ 2. per-draw check
KINDS = ("bias", "bad", "decay", "begin", "all", "none")
DECAY = 40.0          # on the tiny talker's EOS score (negative, outside the top 50) one step of this factor lifts EOS into the support


def _sampling_table(B, shift):
    return dict(do_sample=[True] * B, top_k=[50] * B, top_p=[1.0] * B, temperature=[[0.9, 1.1, 0.8][(b + shift) % 3] for b in range(B)],
                repetition_penalty=[1.05] * B, subtalker_dosample=[True] * B, subtalker_top_k=[50] * B, subtalker_top_p=[1.0] * B,
                subtalker_temperature=[0.9] * B, seed=[7000 * (shift + 1) + 37 * b for b in range(B)])


def _chain(raw, hist, s, c, t, sup, floor, limit):
    return pr.chain(raw.double().numpy(), [int(x) for x in hist], limit=limit, eos_id=t.codec_eos_token_id, min_new_tokens=floor,
                    suppress=sup, repetition_penalty_=s["repetition_penalty"], do_sample=True, temperature=s["temperature"],
                    top_k=s["top_k"], top_p=s["top_p"], sequence_bias_=c.get("sequence_bias"), bad_words_ids=c.get("bad_words_ids"),
                    exponential_decay_length_penalty=c.get("exponential_decay_length_penalty"),
                    begin_suppress_tokens=c.get("begin_suppress_tokens"))


def _pgap(raw, hist, tok, step, s, c, t, sup, floor, limit):
    """tests/test_warpers_gpu.py::_wgap with processors_ref's chain: (how far u = Philox(seed; step, 0, 0) lies outside the interval of
    `tok` in the inverse CDF of the chain under the settings `s` and the controls `c`, scanned in the kernel's order -- <= 0: inside,
    1: outside the support --, the chain)"""
    ch = _chain(raw, hist, s, c, t, sup, floor, limit)
    p = ch.probs[None]
    V = p.shape[1]
    if p[0, tok] <= 0:
        return 1.0, ch
    so = _sampler_slot_order(V) if 0 < s["top_k"] <= 256 and s["top_k"] < V else np.arange(V)
    seed = s["seed"]
    c0 = _philox4x32_10(np.array([step]), 0, 0, 0, seed & 0xFFFFFFFF, seed >> 32)[0]
    u = (c0 >> np.uint64(8)).astype(np.float64) / 16777216.0
    return float(_u_gap(p, so, np.argsort(so), np.array([0]), np.array([tok]), u)[0]), ch


def _ranked(raw, sup):
    s = raw.double().numpy().copy()
    s[sup] = -np.inf
    return [int(x) for x in np.argsort(-s, kind="stable")]


def _fresh_suffixes(hist):
    """The shortest suffix of the history that does not occur in front of its end as well, and the suffix one token longer: sequences
    over them can match at the checked step only (a match in front of it would change the history the check relies on)."""
    h = [int(x) for x in hist]
    if len(h) < 2:
        return [], []
    for k in range(1, len(h)):
        if not any(h[i:i + k] == h[-k:] for i in range(len(h) - k)):
            return h[-k - 1:], h[-k:]
    raise AssertionError("the history repeats itself")


def _controls_at(kind, rank, hist, step0):
    """One row's controls for a check at one step, written against that step's own raw ranking so that each of them acts there: a
    bias that removes the top token and one that lifts token 60 into the top 50 (both on one token twice: the sums count), a ban of
    ranks 1 and 2, begin suppression of ranks 3..6 (step 0 only), a decay that starts at this step."""
    c = {}
    pre2, pre1 = _fresh_suffixes(hist)
    if kind in ("bias", "all"):
        # (step 0: four single-token records, of which a repeated key keeps its last value; later: only sequences over the row's last
        # tokens -- a single-token record would act at every step in front of the checked one as well)
        c["sequence_bias"] = {tuple(pre1 + [rank[0]]): -20.0, tuple(pre1 + [rank[60]]): 18.0, tuple(pre2 + [rank[60]]): 12.0,
                              tuple(pre2 + [rank[0]]): -10.0}
    if kind in ("bad", "all"):
        c["bad_words_ids"] = [pre2 + [rank[1]], pre1 + [rank[2]]]
    if kind in ("decay", "all") and not step0:
        c["exponential_decay_length_penalty"] = (len(hist) - 1, DECAY)
    if kind in ("begin", "all") and step0:
        c["begin_suppress_tokens"] = rank[3:7]
    return c


def _columns(B, rows):
    return {k: [r.get(k) for r in rows] for k in PROC if any(k in r for r in rows)}


def body_draws(dev, t, w, dtype, graph, B, M=6, shifts=(0, 1), max_seq=64, long_prompt=False):
    """Every row draws under ITS OWN controls.  Two checked steps per call pair: step 0 (hist empty: the begin suppression and the
    single-token records) and step M - 1 (sequences of length 2 and 3 over the row's own last tokens, and the decay).  The controls of
    a step are written against the raw logits a first run WITHOUT them leaves at that step, so that each acts; with them only that
    step's choice changes (asserted: the history in front of it is the first run's).  Every drawn token then lies in its row's
    inverse-CDF interval for u = Philox(seed_b; step, 0, 0) under processors_ref's chain on the engine's own raw logits, within TOL;
    under the neighbouring row's controls and seed most draws miss.  Each control changed the support or the EOS probability in at
    least a quarter of the draws it is compared on."""
    eng = rs._engine(t, w, dev, dtype, graph, B, max_seq)
    args, _ = rs._prompt(t, B)
    sup = _suppress(t)
    eos = t.codec_eos_token_id
    used, bit = {}, {}
    n_cmp, n_own, n_miss, worst = 0, 0, 0, -1.0
    for shift in shifts:
        tab = _sampling_table(B, shift)
        kinds = [KINDS[(b + shift) % len(KINDS)] for b in range(B)]
        for m in (1, M):                                        # the token step m - 1 is the checked one
            floor = m + 1 if m == 1 else [m - 1] * B          # (EOS may be drawn at the checked step of a decay row, not before)
            base = dict(min_new_tokens=floor, suppress_tokens=sup, **tab)
            first = eng.generate(*args, max_new_tokens=[m] * B, **base)
            raw = eng.debug_logits()[:B].cpu()
            hist0 = _np(first.tokens)[:, :m - 1]
            rows = [_controls_at(kinds[b], _ranked(raw[b], sup), hist0[b], m == 1) for b in range(B)]
            ctl = _columns(B, rows)
            eng.generate(*args, max_new_tokens=[m] * B, **base, **ctl)
            assert eng.sampler_class()[0] == (3 if ctl else 1)
            raw2 = eng.debug_logits()[:B].cpu()
            lt = _np(eng.generate(*args, max_new_tokens=[m + 1] * B, **base, **ctl).tokens)
            assert np.array_equal(lt[:, :m - 1], hist0) and torch.equal(raw, raw2)
            for b in range(B):
                s, fl = rs._row(tab, b), (floor if m == 1 else floor[b])
                gap, ch = _pgap(raw[b], hist0[b], int(lt[b, m - 1]), m - 1, s, rows[b], t, sup, fl, m + 1)
                n_cmp += 1
                if ch.borderline:
                    continue
                worst = max(worst, gap)
                for k in rows[b]:
                    less = {q: v for q, v in rows[b].items() if q != k}
                    p0, p1 = _chain(raw[b], hist0[b], s, less, t, sup, fl, m + 1).probs, ch.probs
                    used[k] = used.get(k, 0) + 1
                    bit[k] = bit.get(k, 0) + bool(((p0 > 0) != (p1 > 0)).any() or p0[eos] != p1[eos])
                o = (b + 1) % B
                if rows[b] or rows[o]:
                    n_own += 1
                    n_miss += _pgap(raw[b], hist0[b], int(lt[b, m - 1]), m - 1, rs._row(tab, o), rows[o], t, sup, fl, m + 1)[0] > 1e-3
                print(f"  shift {shift} step {m - 1} row {b} ({kinds[b]}): gap {gap:.2e} removed {ch.removed}")
    print(f"processors: {n_cmp} draws, worst gap {worst:.2e}; {n_miss} of {n_own} miss under the neighbour's settings; acted {bit} of {used}")
    assert worst <= TOL, worst
    assert n_miss >= 0.5 * n_own, (n_miss, n_own)
    for k in ("sequence_bias", "bad_words_ids", "exponential_decay_length_penalty", "begin_suppress_tokens"):
        assert used.get(k, 0) >= 1 and bit.get(k, 0) >= 0.25 * used[k], (k, bit, used)


@pytest.mark.parametrize("dtype,graph", [(torch.bfloat16, True), (torch.float32, False)])
@pytest.mark.parametrize("B", [4, 8])
def test_every_row_draws_under_its_own_processors(dev, dtype, graph, B):
    body_draws(dev, *rs._tiny(), dtype, graph, B)


def test_every_row_draws_under_its_own_processors_at_the_real_vocabulary(dev):
    """V = 3072: the talker's real vocabulary and sample_warp_kernel<12> (0.6B dims, 2 talker layers, bf16, graph)."""
    t = synth.talker_06b()
    t.num_hidden_layers = 2
    assert t.vocab_size == 3072
    body_draws(dev, t, _td(synth.talker_weights(t, with_text=False)), torch.bfloat16, True, 8, shifts=(0,))


def body_long_history(dev, steps=262):
    """Sequences whose first tokens lie past the 256 history entries the kernel prefetches: 2 greedy requests run `steps` tokens; a bad
    word and a bias of length 3 are then written over each request's tokens 257..259 and the run repeated -- token 259 changes, nothing
    in front of it does, and the new token is the restatement's choice on the engine's raw logits."""
    t, w = rs._tiny()
    eng = rs._engine(t, w, dev, torch.float32, True, 2, 320)
    args, _ = rs._prompt(t, 2)
    sup = _suppress(t)
    kw = dict(min_new_tokens=steps + 1, do_sample=False, subtalker_dosample=False, repetition_penalty=1.05, suppress_tokens=sup,
              no_repeat_ngram_size=[3, 3])
    plain = _np(eng.generate(*args, max_new_tokens=[steps] * 2, **kw).tokens)

    def fresh(row):          # the first step >= 259 whose trigram has not occurred before it (an earlier match would change the history)
        for c in range(259, steps - 1):
            tri = list(row[c - 2:c + 1])
            if not any(list(row[i:i + 3]) == tri for i in range(c - 2)):
                return c
        raise AssertionError("every late trigram of the plain run is a repeat")
    cs = [fresh(plain[b]) for b in range(2)]
    ctl = dict(bad_words_ids=[[[int(x) for x in plain[0, cs[0] - 2:cs[0] + 1]]], None],
               sequence_bias=[None, {tuple(int(x) for x in plain[1, cs[1] - 2:cs[1] + 1]): -40.0}])
    raws = []
    for b in range(2):       # (one call per row: the logits a call leaves behind are its last step's)
        eng.generate(*args, max_new_tokens=[cs[b] + 1] * 2, **kw, **ctl)
        raws.append(eng.debug_logits()[b].cpu())
    out = _np(eng.generate(*args, max_new_tokens=[steps] * 2, **kw, **ctl).tokens)
    assert eng.sampler_class()[0] == 3
    for b in range(2):
        c, raw = cs[b], {b: raws[b]}
        assert np.array_equal(out[b, :c], plain[b, :c]) and out[b, c] != plain[b, c], b
        ch = pr.chain(raw[b].double().numpy(), out[b, :c], limit=steps, eos_id=t.codec_eos_token_id, min_new_tokens=steps + 1, suppress=sup,
                      repetition_penalty_=1.05, no_repeat_ngram_size=3, do_sample=False,
                      sequence_bias_=ctl["sequence_bias"][b], bad_words_ids=ctl["bad_words_ids"][b])
        assert ch.token == out[b, c], (b, ch.token, out[b, c])


def test_sequences_past_the_prefetched_history(dev):
    body_long_history(dev)


# ============================================================================================ 3. hand-driven: every step against the restatement
def body_hand(dev, graph=False, M=8):
    """Greedy rows under hand-written controls, every token step checked: the engine's token is the restatement's choice on the engine's
    own raw logits of that step (one call per step: the logits a call leaves behind are its last step's).  Row 0: biases, two of which
    land on one token; row 1: bad words; row 2: begin suppression, a decay and an open EOS; row 3: forced EOS under a floor above its
    limit.  Returns the tokens (the emulator runs this under several scheduling orders)."""
    t, w = rs._tiny()
    B, eos = 4, t.codec_eos_token_id
    eng = rs._engine(t, w, dev, torch.float32, graph, B)
    args, _ = rs._prompt(t, B)
    sup = _suppress(t)
    kw = dict(do_sample=False, subtalker_dosample=False, repetition_penalty=1.05, suppress_tokens=sup)
    lim, flo = [M, M, M, M - 2], [M + 1, M + 1, 2, M + 1]
    pt = _np(eng.generate(*args, max_new_tokens=lim, min_new_tokens=flo, **kw).tokens)
    i = lambda b, k: int(pt[b, k])
    ctl = dict(sequence_bias=[{(i(0, 1),): -20.0, (i(0, 0), i(0, 3)): -9.5, (i(0, 3),): 4.25, (i(0, 0), i(0, 1), i(0, 3)): 2.125}, None, None, None],
               bad_words_ids=[None, [[i(1, 2)], [i(1, 0), i(1, 1), i(1, 3)], [eos]], None, None],
               begin_suppress_tokens=[None, None, [i(2, 0), 3], None],
               exponential_decay_length_penalty=[None, None, (1, 3.0), None],
               forced_eos_token_id=[None, None, None, eos], min_length=[None, None, None, M + 3])
    full = _np(eng.generate(*args, max_new_tokens=lim, min_new_tokens=flo, **kw, **ctl).tokens)
    assert eng.sampler_class() == (3, 2)
    assert all(not np.array_equal(full[b, :lim[b] - 1], pt[b, :lim[b] - 1]) for b in range(3)) and full[3, lim[3] - 1] == eos
    assert eos in full[2, :M - 1], "the decay never ends row 2"
    for m in range(1, M):
        eng.generate(*args, max_new_tokens=[min(m, x) for x in lim], min_new_tokens=flo, **kw, **ctl)
        raw = eng.debug_logits()[:B].cpu().double().numpy()
        for b in range(B):
            hist = full[b, :m - 1]
            if eos in hist or m > lim[b]:
                continue
            ch = pr.chain(raw[b], hist, do_sample=False, limit=lim[b], eos_id=eos, min_new_tokens=flo[b], suppress=sup, repetition_penalty_=1.05,
                          **{("sequence_bias_" if k == "sequence_bias" else k): v[b] for k, v in ctl.items()})
            if m < lim[b] or ctl["forced_eos_token_id"][b] is not None:      # (a table run shows eos at a row's limit whatever was chosen)
                assert ch.token == full[b, m - 1], (m, b, ch.token, full[b, m - 1])
    return full


def test_every_step_of_hand_written_controls_is_the_restatements_choice(dev):
    body_hand(dev, graph=True)


# ============================================================================================ 4. place and neighbours
def body_place(dev, M=7):
    """A request's codes do not depend on its row index or on its neighbours' records: request 2 of a sampled batch of 4 -- whose row 0
    carries 64 sequences of 8 tokens, the capacity the engine must take at least -- alone, and in row 0 of a pair, has its codes of
    the batch; request 0 has the same codes with and without its never-matching records."""
    t, w = rs._tiny()
    eng = rs._engine(t, w, dev, torch.float32, False, 4)
    args, _ = rs._prompt(t, 4)
    sup = _suppress(t)
    kw = dict(min_new_tokens=M + 1, suppress_tokens=sup, temperature=0.9, top_k=50)
    seeds = [41, 42, 43, 44]
    pt = _np(eng.generate(*args, max_new_tokens=[M] * 4, seed=seeds, **kw).tokens)
    mine = dict(bad_words_ids=[[int(pt[2, 1])], [int(pt[2, 0]), int(pt[2, 1]), int(pt[2, 2])]], sequence_bias={(int(pt[2, 3]),): -15.0},
                begin_suppress_tokens=[int(pt[2, 0])])
    many = {tuple(int(x) for x in np.random.default_rng(5).integers(1, 200, 8)): -1.0 for _ in range(64)}
    col = lambda k, rows: [rows.get(b, {}).get(k) for b in range(4)]
    full = eng.generate(*args, max_new_tokens=[M] * 4, seed=seeds, **kw,
                        **{k: col(k, {2: mine, 0: dict(sequence_bias=many), 3: dict(begin_suppress_tokens=[int(pt[3, 0])])}) for k in mine})
    assert eng.sampler_class()[0] == 3
    fc, ft = _np(full.codes), _np(full.tokens)
    assert not np.array_equal(ft[2], pt[2]) and not np.array_equal(ft[3], pt[3])
    sel = lambda idx: [a[idx] for a in args[:3]] + [args[3]]           # (row 2 has the longest prompt: it keeps its left padding alone)
    alone = eng.generate(*sel([2]), max_new_tokens=[M], seed=[seeds[2]], **kw, **{k: [v] for k, v in mine.items()})
    assert np.array_equal(_np(alone.codes)[0], fc[2]) and np.array_equal(_np(alone.tokens)[0], ft[2])
    pair = eng.generate(*sel([2, 0]), max_new_tokens=[M] * 2, seed=[seeds[2], seeds[0]], **kw,
                        **{k: [v, None] for k, v in mine.items()})
    # request 0 carried 64 sequences of 8 tokens that never match in the batch of 4 and none here: the same codes
    assert eng.sampler_class()[0] == 3
    assert np.array_equal(_np(pair.codes)[0], fc[2]) and np.array_equal(_np(pair.codes)[1], fc[0])


def test_a_rows_codes_do_not_depend_on_place_or_neighbours(dev):
    body_place(dev)


# ============================================================================================ 5. streams
def _single(eng1, args, i, kw, ctl, sup, floor):
    a = [x[i:i + 1] for x in args[:3]] + [args[3]]
    drop = int((1 - a[1]).sum())
    a[0], a[1] = a[0][:, drop:], a[1][:, drop:]
    return eng1.generate(*a, **{k: [v[i]] for k, v in kw.items()}, min_new_tokens=floor, suppress_tokens=sup, **{k: [v[i]] for k, v in ctl.items()})


def body_admitted(dev):
    """`schedule="continuous"` on 2 rows, packets of one frame, 5 requests of which only the last TWO of the queue have records: the
    stream opens and admits its first queued request without any; `graph_captures` advances once when the first request with records
    is admitted and not again on the next -- 2 captures in all --, and every request's codes equal the request alone."""
    t, w = rs._tiny()
    N, M = 5, 6
    args, lens = rs._prompt(t, N, seed=61)
    sup = _suppress(t)
    order = sorted(range(N), key=lambda i: (-lens[i], i))
    limits = [0] * N
    for pos, i in enumerate(order):
        limits[i] = M - (pos % 2)
    kw = dict(max_new_tokens=limits, seed=[900 + i for i in range(N)], temperature=[0.9] * N)
    eng = rs._engine(t, w, dev, torch.float32, True, 2)
    plain = _np(eng.generate(*args, schedule="continuous", packet_frames=1, min_new_tokens=M + 2, suppress_tokens=sup, **kw).codes)
    ctl = {k: [None] * N for k in ("bad_words_ids", "begin_suppress_tokens", "sequence_bias")}
    ctl["begin_suppress_tokens"][order[-1]] = [int(plain[order[-1], 0, 0])]
    ctl["bad_words_ids"][order[-1]] = [[int(plain[order[-1], 1, 0])]]
    ctl["sequence_bias"][order[-2]] = {(int(plain[order[-2], 0, 0]),): -25.0}
    eng = rs._engine(t, w, dev, torch.float32, True, 2)
    out = eng.generate(*args, schedule="continuous", packet_frames=1, min_new_tokens=M + 2, suppress_tokens=sup, **kw, **ctl)
    st = eng.last_refill
    assert eng.sampler_class()[0] == 3 and st["streams"] == 1
    assert st["admit_calls"] == 3 and st["admitted_rows"] == 3, st
    assert st["graph_captures"] == 2, st
    one = rs._engine(t, w, dev, torch.float32, False, 1)
    oc = _np(out.codes)
    for i in range(N):
        ref = _single(one, args, i, kw, ctl, sup, M + 2)
        n = ref.codes.shape[1]
        assert np.array_equal(oc[i, :n], _np(ref.codes)[0]), i
        if i in order[-2:]:                                       # the two requests really ran under their records
            assert not np.array_equal(oc[i, :n], plain[i, :n]), i


def test_a_request_with_records_admitted_into_a_stream_that_ran_without_any(dev):
    body_admitted(dev)


def body_pooled_restart(dev):
    """A pooled engine small enough to preempt (5 pages): the restarted request has records and yields the codes of the unpreempted run."""
    from qwen3_tts_amd.talker import TalkerEngine
    t, w = rs._tiny()
    N, M = 4, 40
    args, lens = rs._prompt(t, N, seed=61)
    sup = _suppress(t)
    kw = dict(max_new_tokens=[M] * N, min_new_tokens=M + 2, suppress_tokens=sup, seed=[700 + i for i in range(N)], schedule="continuous")
    big = TalkerEngine(t, w, weight_dtype=torch.float32, device=dev, max_batch=N, max_seq=64, use_graph=False)
    plain = _np(big.generate(*args, **kw).codes)
    ctl = dict(bad_words_ids=[[[int(plain[i, 1, 0])], [int(plain[i, 2, 0]), int(plain[i, 3, 0])]] for i in range(N)],
               sequence_bias=[{(int(plain[i, 5, 0]),): -12.0} if i % 2 else None for i in range(N)],
               begin_suppress_tokens=[[int(plain[i, 0, 0])] for i in range(N)])
    ref = big.generate(*args, **kw, **ctl)
    assert big.sampler_class()[0] == 3
    small = TalkerEngine(t, w, weight_dtype=torch.float32, device=dev, max_batch=N, max_seq=64, use_graph=False, kv_pages=5)
    out = small.generate(*args, **kw, **ctl)
    assert small.last_refill["preemptions"] >= 1 and small.sampler_class()[0] == 3, small.last_refill
    assert np.array_equal(_np(out.codes), _np(ref.codes))
    for i in range(N):
        assert not np.array_equal(_np(out.codes)[i], plain[i]), i


def test_a_preempted_request_with_records_restarts_to_the_same_codes(dev):
    body_pooled_restart(dev)


# ============================================================================================ 6. wrapper
def body_wrapper(dev):
    """`Qwen3TTSModel.generate_custom_voice(..., bad_words_ids=..., exponential_decay_length_penalty=[(2, 1.5), None])` reaches the
    engine (class 3) and changes the codes of exactly the requests that name a control."""
    from qwen3_tts_amd.codec import Qwen3TTSTokenizer
    from qwen3_tts_amd.model import Qwen3TTSForConditionalGeneration, Qwen3TTSModel
    t = synth.talker_tiny()
    c = synth.codec_tiny()
    c.codebook_size = t.cp_vocab_size
    cfgd = dict(synth.cfg_dict(t), tts_model_type="custom_voice", tts_model_size="1b7", tokenizer_type="12hz")
    model = Qwen3TTSForConditionalGeneration(cfgd, _td(synth.talker_weights(t)), device=dev, dtype=torch.float32, max_batch=4, max_seq=128)
    model.load_speech_tokenizer(Qwen3TTSTokenizer.from_state_dict(synth.cfg_dict(c), _td(synth.codec_weights(c)), device=dev,
                                                                  max_batch=4, max_frames=64))

    class FakeProcessor:
        def __call__(self, text=None, return_tensors="pt", padding=True):
            body = [(ord(ch) * 7) % 490 for ch in text if ch not in "<|>_\\n"][:40]
            a, n = 77, 198
            if text.startswith("<|im_start|>user"):
                ids = [t.im_start_token_id] + body + [t.im_end_token_id, n]
            else:
                ids = [t.im_start_token_id, a, n] + body + [t.im_end_token_id, n, t.im_start_token_id, a, n]
            return {"input_ids": torch.tensor([ids])}
    tts = Qwen3TTSModel(model, FakeProcessor(), generate_defaults={})
    texts, spk, langs = ["hello world", "a rather longer sentence to speak", "third"], ["vivian", "ryan", "vivian"], ["english", "chinese", "english"]
    kw = dict(language=langs, max_new_tokens=24, seed=[11, 12, 13])
    calls = []
    inner = model.talker.generate

    def spy(*a, **k):
        out = inner(*a, **k)
        calls.append((k, _np(out.codes)))
        return out
    model.talker.generate = spy
    try:
        tts.generate_custom_voice(texts, spk, **kw)
        assert model.talker.sampler_class()[0] == 1
        first = int(calls[0][1][1, 0, 0])
        tts.generate_custom_voice(texts, spk, bad_words_ids=[None, [[first]], None], exponential_decay_length_penalty=[(2, 1.5), None, None], **kw)
        assert model.talker.sampler_class()[0] == 3
        tts.generate_custom_voice(texts, spk, bad_words_ids=[[first]], **kw)           # HF's own form: one value for the call
        assert model.talker.sampler_class()[0] == 3
    finally:
        model.talker.generate = inner
    assert len(calls) == 3
    assert calls[1][0]["bad_words_ids"] == [None, [[first]], None]
    assert calls[1][0]["exponential_decay_length_penalty"] == [(2, 1.5), None, None]
    plain, both, shared = calls[0][1], calls[1][1], calls[2][1]
    assert both[1, 0, 0] != first and shared[1, 0, 0] != first
    # exactly the requests that name a control change: request 1 (its first token is banned), request 0 (the decay ends it earlier)
    # -- and request 2, which names none, does not
    eos = t.codec_eos_token_id
    end = lambda x: int(np.argmax(x[:, 0] == eos)) if (x[:, 0] == eos).any() else x.shape[0]
    print(f"wrapper: request 0 ends at {end(both[0])} under the decay, at {end(plain[0])} without")
    assert end(both[0]) < end(plain[0])
    n2 = min(end(plain[2]), end(both[2]))
    assert end(plain[2]) == end(both[2]) and np.array_equal(both[2][:n2], plain[2][:n2])


def test_wrapper_passes_the_processors_to_the_engine(dev):
    body_wrapper(dev)
