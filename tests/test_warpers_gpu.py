"""HF generate's remaining sampling controls on the talker's codebook-0 sampler, per request: min_p, typical_p, epsilon_cutoff,
eta_cutoff and no_repeat_ngram_size (include/qtts.h: qtts_row_warpers, qtts_talker_set_row_warpers, qtts_talker_sampler_class;
csrc/sampling.hip: sample_warp_kernel; `TalkerEngine.generate(..., min_p=[...], no_repeat_ngram_size=3)`).

The yardsticks are tests/warpers_ref.py (a float64 restatement, pinned by tests/test_warpers_ref.py against transformers' own classes)
and the fixtures tools/gen_golden_warpers.py wrote.  The test BODIES (`body_*`) take the device; tests/test_warpers_hostemu.py runs the
same bodies on the host-emulation build."""
import os

import numpy as np
import pytest
import torch

import synth
import warpers_ref
import test_row_sampling_gpu as rs
from test_gpu_parity import _compare_greedy, _philox4x32_10, _sampler_slot_order, _suppress, _td, _u_gap, dev  # noqa: F401  (`dev` is a fixture)

pytestmark = pytest.mark.gpu

TOL = rs.TOL
WARP = ("min_p", "typical_p", "epsilon_cutoff", "eta_cutoff", "no_repeat_ngram_size")
KINDS = ("min_p", "typical_p", "epsilon_cutoff", "eta_cutoff", "all", "none")
# The values of the three calls of a per-draw test, per config: chosen on the emulator so that every warper removes at least one
# surviving token in at least a quarter of the draws it is compared on (asserted: a warper that removes nothing proves nothing).
# (the tiny talker's top-50 distribution is flat -- entropy near ln 50 -- so eta = sqrt(eps) * exp(-H) needs a large eps to reach any token)
VALUES_TINY = [dict(min_p=0.2, typical_p=0.6, epsilon_cutoff=0.02, eta_cutoff=0.3),
               dict(min_p=0.35, typical_p=0.4, epsilon_cutoff=0.03, eta_cutoff=0.45),
               dict(min_p=0.5, typical_p=0.5, epsilon_cutoff=0.025, eta_cutoff=0.6)]
VALUES_06B = VALUES_TINY


def _np(x):
    return rs._np(x)


def _warp_table(B, shift, vals):
    """B requests cycling through: min_p only, typical_p only, epsilon only, eta only, all four with top_p 0.9 and n = 2, none."""
    tab = dict(do_sample=[True] * B, top_k=[50] * B, top_p=[1.0] * B, temperature=[[0.9, 1.1, 0.8][(b + shift) % 3] for b in range(B)],
               repetition_penalty=[1.05] * B, subtalker_dosample=[True] * B, subtalker_top_k=[50] * B, subtalker_top_p=[1.0] * B,
               subtalker_temperature=[0.9] * B, seed=[5000 * (shift + 1) + 31 * b for b in range(B)])
    for k in WARP:
        tab[k] = [None] * B             # (None = off; a typical_p of 0 is an error in HF)
    for b in range(B):
        kind = KINDS[(b + shift) % len(KINDS)]
        for k in vals:
            if kind in (k, "all"):
                tab[k][b] = vals[k]
        if kind == "all":
            tab["top_p"][b], tab["no_repeat_ngram_size"][b] = 0.9, 2
    return tab


def _chain(raw, hist, s, t, sup, floor):
    return warpers_ref.chain(raw.double().numpy(), [int(x) for x in hist], do_sample=bool(s["do_sample"]), temperature=s["temperature"],
                             top_k=s["top_k"], top_p=s["top_p"], repetition_penalty_=s["repetition_penalty"], eos_id=t.codec_eos_token_id,
                             min_new_tokens=floor, suppress=sup, **{k: s.get(k, 0) or 0 for k in WARP})


def _wgap(raw, hist, tok, step, s, t, sup, floor):
    """(how far u = Philox(seed; step, 0, 0) lies outside the interval of `tok` in the inverse CDF of warpers_ref's chain under the
    settings `s`, scanned in the kernel's order -- <= 0: inside, 1: outside the support --, the distance of u to the nearest edge of
    that interval when inside, the chain)"""
    ch = _chain(raw, hist, s, t, sup, floor)
    p = ch.probs[None]
    V = p.shape[1]
    if p[0, tok] <= 0:
        return 1.0, 0.0, ch
    so = _sampler_slot_order(V) if 0 < s["top_k"] <= 256 and s["top_k"] < V else np.arange(V)
    seed = s["seed"]
    c0 = _philox4x32_10(np.array([step]), 0, 0, 0, seed & 0xFFFFFFFF, seed >> 32)[0]
    u = (c0 >> np.uint64(8)).astype(np.float64) / 16777216.0
    gap = float(_u_gap(p, so, np.argsort(so), np.array([0]), np.array([tok]), u)[0])
    return gap, -gap, ch


# ============================================================================================ 1. greedy n-gram bans
def _ngram_case(golden_dir, name):
    g = np.load(os.path.join(golden_dir, "talker_tiny_ngram.npz"))
    args = [torch.from_numpy(g[f"{name}_{k}"]) for k in ("embeds", "mask", "trailing", "tts_pad")]
    return g, args, [int(x) for x in g[f"{name}_ngram"]]


def _greedy_kw(t, steps):
    return dict(max_new_tokens=steps, min_new_tokens=steps + 1, do_sample=False, subtalker_dosample=False, repetition_penalty=1.05,
                suppress_tokens=_suppress(t))


def _check_ngram_run(g, name, codes, tokens, t):
    """codes / tokens of a table run against the fixture: every frame compared; the table shows eos at a row's last token index."""
    n = g[f"{name}_codes"].shape[1]
    gt = g[f"{name}_tokens"].copy()
    gt[:, n] = t.codec_eos_token_id
    assert codes.shape == g[f"{name}_codes"].shape and tokens.shape[1] == n + 1
    assert _compare_greedy(codes, tokens, g[f"{name}_codes"], gt, g[f"{name}_margin"]) == n


def body_greedy_ngram(dev, golden_dir, graph, name="a", max_seq=64):
    """Greedy, fp32, one table call with a ban size per row: codes and tokens are the reference talker's under transformers' own
    NoRepeatNGramLogitsProcessor (tests/golden/talker_tiny_ngram.npz), the sampler class is 3, and the n = 0 row equals the plain run."""
    t, w = rs._tiny()
    g, args, ngram = _ngram_case(golden_dir, name)
    assert float(g[f"{name}_margin"].min()) >= 1e-3
    steps = g[f"{name}_tokens"].shape[1]
    eng = rs._engine(t, w, dev, torch.float32, graph, len(ngram), max_seq)
    out = eng.generate(*args, no_repeat_ngram_size=ngram, **_greedy_kw(t, steps))
    assert eng.sampler_class() == (3, 2) and eng.stats()["row_table_last"] == 1
    codes, tokens = _np(out.codes), _np(out.tokens)
    _check_ngram_run(g, name, codes, tokens, t)
    plain = eng.generate(*args, **_greedy_kw(t, steps))
    assert eng.sampler_class() == (0, 0)
    pt = _np(plain.tokens)
    if float(g[f"{name}_margin_plain"].min()) >= 1e-3:       # (the run without the ban is pinned too where ITS margins are clear)
        assert np.array_equal(pt, g[f"{name}_tokens_plain"])
    for b, n in enumerate(ngram):
        assert np.array_equal(tokens[b, :-1], pt[b, :-1]) == (n == 0), (b, n)
        if n == 0:
            assert np.array_equal(codes[b], _np(plain.codes)[b])


@pytest.mark.parametrize("graph", [False, True])
def test_greedy_ngram_bans_are_the_reference_run(dev, golden_dir, graph):
    body_greedy_ngram(dev, golden_dir, graph)


def _late_bans(tokens, n, prefetched=256):
    """Token steps of a request at which the banned set depends on history entries at or behind `prefetched`: the n-gram scan's strides
    i >= 256, which read every token from global memory."""
    late = []
    for c in range(prefetched + 1, len(tokens)):
        h = [int(x) for x in tokens[:c]]
        early = {h[i + n - 1] for i in range(min(c - n + 1, prefetched - n + 1)) if h[i:i + n - 1] == h[c - n + 1:]}
        if set(warpers_ref.banned_ngram_tokens(h, n)) != early:
            late.append(c)
    return late


def body_greedy_ngram_long(dev, golden_dir):
    """Case B: 2 requests, n = 3, 270 token steps, fp32, graph, max_seq 320 -- bit-exact against the reference talker under transformers'
    NoRepeatNGramLogitsProcessor, every frame compared; in the fixture, bans that only history entries behind the 256 prefetched ones
    produce are in force at some steps (asserted: otherwise the strides i >= 256 of the scan would not be exercised)."""
    g = np.load(os.path.join(golden_dir, "talker_tiny_ngram.npz"))
    for b in range(2):
        late = _late_bans(g["b_tokens"][b], 3)
        print(f"case B row {b}: {len(late)} token steps whose banned set depends on history entries >= 256")
        assert len(late) >= 1, b
    body_greedy_ngram(dev, golden_dir, True, "b", 320)


def test_greedy_ngram_bans_past_the_prefetched_history(dev, golden_dir):
    body_greedy_ngram_long(dev, golden_dir)


def body_long_history_property(dev, steps=270, n=3):
    """The ban's own guarantee on a history past the 256 entries the kernel prefetches, without a fixture: 2 greedy requests, n = 3, 270
    token steps -- no 3-gram occurs twice in a request's tokens, while the same requests without the ban DO repeat 3-grams behind
    token 256 (so a scan that missed entries there would show)."""
    t, w = rs._tiny()
    eng = rs._engine(t, w, dev, torch.float32, True, 2, 320)
    args, _ = rs._prompt(t, 2)
    grams = lambda row: [tuple(row[i:i + n]) for i in range(len(row) - n + 1)]
    plain = _np(eng.generate(*args, **_greedy_kw(t, steps)).tokens)
    out = eng.generate(*args, no_repeat_ngram_size=[n, n], **_greedy_kw(t, steps))
    assert eng.sampler_class()[0] == 3
    toks = _np(out.tokens)[:, :-1]                       # (a table run shows eos at the last index)
    assert toks.shape[1] == steps - 1 > 256 + n
    for b in range(2):
        seen = set(grams(plain[b, :256]))
        assert any(g in seen for g in grams(plain[b, 256 - n + 1:])), "the plain run repeats no 3-gram behind token 256: nothing to ban there"
        g = grams(toks[b])
        assert len(set(g)) == len(g), f"row {b}: a 3-gram occurs twice under no_repeat_ngram_size = 3"


def test_no_ngram_repeats_past_the_prefetched_history(dev):
    body_long_history_property(dev)


def body_ngram_streams(dev, golden_dir):
    """Case A through `generate_stream` packets, and its 4 requests on 2 rows through `schedule="continuous"`."""
    t, w = rs._tiny()
    g, args, ngram = _ngram_case(golden_dir, "a")
    steps = g["a_tokens"].shape[1]
    eng = rs._engine(t, w, dev, torch.float32, True, 4)
    parts = [_np(p) for p in eng.generate_stream(*args, packet_frames=4, no_repeat_ngram_size=ngram, **_greedy_kw(t, steps))]
    assert eng.sampler_class()[0] == 3
    assert np.array_equal(np.concatenate(parts, axis=1), g["a_codes"])
    eng2 = rs._engine(t, w, dev, torch.float32, True, 2)
    out = eng2.generate(*args, schedule="continuous", no_repeat_ngram_size=ngram, **_greedy_kw(t, steps))
    assert eng2.sampler_class()[0] == 3
    assert np.array_equal(_np(out.codes), g["a_codes"])


def test_ngram_bans_through_stream_packets_and_the_continuous_schedule(dev, golden_dir):
    body_ngram_streams(dev, golden_dir)


# ============================================================================================ 2. / 3. per-draw check
def body_draws(dev, t, w, dtype, graph, B, values, M=6):
    """Every row draws under ITS OWN warpers: three calls on one engine with other values each; for the last talker step every drawn
    token lies in its row's inverse-CDF interval for u = Philox(seed_b; step, 0, 0) under warpers_ref's chain on the engine's own raw
    logits, within TOL; under the neighbouring row's knobs and seed the draws miss by more than 1e-3; the sub-code draws of the same
    frame pass the row-sampling test's check; on a graph engine the calls after the first capture nothing."""
    eng = rs._engine(t, w, dev, dtype, graph, B)
    args, _ = rs._prompt(t, B)
    sup = _suppress(t)
    later, caps, blocks = [], [], []
    for i, vals in enumerate(values):
        tab = _warp_table(B, i, vals)
        own, other, res, _ = rs._draw_check(eng, t, args, tab, M)
        assert eng.sampler_class() == (3, 1)
        caps.append(eng.stats()["graph_captures"])
        blocks.append(res[3])
        print(f"warpers, call {i}: sub-code draws worst gap {own:.2e} (neighbour's settings: {other:.2e}), captures {caps[-1]}")
        assert own <= TOL, (i, own)
        raw = eng.debug_logits()[:B].cpu()
        later.append((tab, raw, res[1]))
        if graph and i and blocks[i] == blocks[i - 1]:
            assert caps[i] == caps[i - 1], caps
    if graph and dev != "cpu":
        assert all(b == blocks[0] for b in blocks) and caps[-1] == caps[0], (caps, blocks)
    n_cmp, n_border, worst, worst_other, n_own, n_miss = 0, 0, -1.0, -1.0, 0, 0
    used, bit = {}, {}
    for i, (tab, raw, toks) in enumerate(later):
        lng = eng.generate(*args, max_new_tokens=[M + 1] * B, min_new_tokens=M + 1, suppress_tokens=sup, **tab)
        lt = _np(lng.tokens)
        assert np.array_equal(lt[:, :M - 1], toks[:, :M - 1])
        for b in range(B):
            s, o = rs._row(tab, b), rs._row(tab, (b + 1) % B)
            hist = lt[b, :M - 1]
            gap, _, ch = _wgap(raw[b], hist, int(lt[b, M - 1]), M - 1, s, t, sup, M + 1)
            n_cmp += 1
            if ch.borderline:
                n_border += 1
                continue
            for k in WARP:
                if s[k]:
                    used[k] = used.get(k, 0) + 1
                    bit[k] = bit.get(k, 0) + (ch.removed.get(k, 0) >= 1)
            print(f"  call {i} row {b}: gap {gap:.2e} removed {ch.removed}")
            worst = max(worst, gap)
            og = _wgap(raw[b], hist, int(lt[b, M - 1]), M - 1, o, t, sup, M + 1)[0]
            worst_other = max(worst_other, og)
            n_own += 1
            n_miss += og > 1e-3
    print(f"warpers: {n_cmp} talker draws, {n_border} borderline, worst gap {worst:.2e} (neighbour's settings: {worst_other:.2e}); bites {bit} of {used}")
    assert n_border <= 0.02 * n_cmp, (n_border, n_cmp)
    assert worst <= TOL and worst_other > 1e-3, (worst, worst_other)
    # Under the neighbour's knobs and seed u is an unrelated uniform: it falls into the drawn token's interval with that token's
    # probability, at most ~0.4 after these cuts and far less on average -- so most draws must miss, not just one of them.
    print(f"warpers: {n_miss} of {n_own} draws miss under the neighbour's settings")
    assert n_miss >= 0.5 * n_own, (n_miss, n_own)
    for k in WARP[:4]:       # (the four probability warpers; that the n-gram ban bites is the greedy fixture's business)
        assert used.get(k, 0) >= 1 and bit.get(k, 0) >= 0.25 * used[k], (k, bit, used)


@pytest.mark.parametrize("dtype,graph", [(torch.bfloat16, True), (torch.float32, False)])
@pytest.mark.parametrize("B", [4, 8])
def test_every_row_draws_under_its_own_warpers(dev, dtype, graph, B):
    body_draws(dev, *rs._tiny(), dtype, graph, B, VALUES_TINY)


def test_every_row_draws_under_its_own_warpers_at_the_real_vocabulary(dev):
    """V = 3072: the talker's real vocabulary and sample_warp_kernel<12>'s real loop counts (0.6B dims, 2 talker layers, bf16, graph)."""
    t = synth.talker_06b()
    t.num_hidden_layers = 2
    assert t.vocab_size == 3072
    body_draws(dev, t, _td(synth.talker_weights(t, with_text=False)), torch.bfloat16, True, 8, VALUES_06B)


# ============================================================================================ 4. place and neighbours
def _edge_distance(eng, t, args, tab, b, M):
    """The smallest distance of a talker draw's u to an edge of its interval over the M tokens of request b, from the engine's own
    logits (one call per step: the logits a call leaves behind are its last step's)."""
    sup = _suppress(t)
    B = args[0].shape[0]
    dist = 1.0
    for m in range(1, M + 1):
        eng.generate(*args, max_new_tokens=[m] * B, min_new_tokens=M + 2, suppress_tokens=sup, **tab)
        raw = eng.debug_logits()[:B].cpu()
        lt = _np(eng.generate(*args, max_new_tokens=[m + 1] * B, min_new_tokens=M + 2, suppress_tokens=sup, **tab).tokens)
        gap, inside, _ = _wgap(raw[b], lt[b, :m - 1], int(lt[b, m - 1]), m - 1, rs._row(tab, b), t, sup, M + 2)
        assert gap <= TOL, (m, gap)
        dist = min(dist, inside)
    return dist


def body_place(dev, dtype=torch.float32, M=5):
    """A warper request's codes alone equal its codes in row 3 of a batch of 4 with other knobs around it; a plain request beside warper
    rows (class 3) equals the same request alone (class 1) token for token -- for a seed whose every u lies at least 1e-4 from an
    interval edge (computed and asserted: the two kernels round their scans differently)."""
    t, w = rs._tiny()
    eng = rs._engine(t, w, dev, dtype, False, 4)
    args, _ = rs._prompt(t, 4)
    sup = _suppress(t)
    tab = _warp_table(4, 1, VALUES_TINY[0])           # rows: typical_p, epsilon, eta, all
    for k in WARP:                                    # row 2 (the longest prompt: keeps its left padding alone) is the plain request
        tab[k][2] = None
    kw = dict(max_new_tokens=[M] * 4, min_new_tokens=M + 2, suppress_tokens=sup)
    full = eng.generate(*args, **kw, **tab)
    assert eng.sampler_class()[0] == 3
    assert _edge_distance(eng, t, args, tab, 2, M - 1) >= 1e-4
    sel = lambda idx: ([a[idx] for a in args[:3]] + [args[3]], {k: [v[i] for i in idx] for k, v in tab.items()})
    a, tb = sel([2])
    alone = eng.generate(*a, max_new_tokens=[M], min_new_tokens=M + 2, suppress_tokens=sup, **tb)
    assert eng.sampler_class()[0] == 1
    assert np.array_equal(_np(alone.tokens)[0], _np(full.tokens)[2]) and np.array_equal(_np(alone.codes)[0], _np(full.codes)[2])
    a, tb = sel([2, 3])                               # the warper request of row 3, in row 1 of a batch of 2
    pair = eng.generate(*a, max_new_tokens=[M] * 2, min_new_tokens=M + 2, suppress_tokens=sup, **tb)
    assert eng.sampler_class()[0] == 3
    assert np.array_equal(_np(pair.codes)[1], _np(full.codes)[3]) and np.array_equal(_np(pair.tokens)[1], _np(full.tokens)[3])


def test_a_warper_rows_codes_do_not_depend_on_place_or_neighbours(dev):
    body_place(dev)


# ============================================================================================ 5. streams
def body_admitted_warper(dev):
    """`schedule="continuous"` on 2 rows, packets of one frame, 5 requests of which only the last TWO of the queue have warpers: the
    stream opens and admits its first queued request without any; the three admissions are three `stream_admit` calls (asserted);
    `graph_captures` advances once when the first warper request is admitted and not again on the next admission -- 2 captures in
    all, the stream's one bucket graph (max_seq 64) twice --, and every request's codes equal the request alone."""
    t, w = rs._tiny()
    N, M = 5, 6
    args, lens = rs._prompt(t, N, seed=61)
    sup = _suppress(t)
    order = sorted(range(N), key=lambda i: (-lens[i], i))        # the schedule's queue: longest prompt first
    warp = {k: [None] * N for k in WARP}
    warp["min_p"][order[-1]], warp["no_repeat_ngram_size"][order[-1]] = 0.3, 2
    warp["typical_p"][order[-2]] = 0.5
    limits = [0] * N
    for pos, i in enumerate(order):                               # the two opening rows finish at different steps: one admission at a time
        limits[i] = M - (pos % 2)
    kw = dict(max_new_tokens=limits, min_new_tokens=M + 2, suppress_tokens=sup, seed=[900 + i for i in range(N)], temperature=[0.9] * N)
    eng = rs._engine(t, w, dev, torch.float32, True, 2)
    out = eng.generate(*args, schedule="continuous", packet_frames=1, **kw, **warp)
    st = eng.last_refill
    assert eng.sampler_class()[0] == 3 and st["streams"] == 1
    assert st["admit_calls"] == 3 and st["admitted_rows"] == 3, st
    assert st["graph_captures"] == 2, st
    one = rs._engine(t, w, dev, torch.float32, False, 1)
    for i in range(N):
        a = [x[i:i + 1] for x in args[:3]] + [args[3]]
        drop = int((1 - a[1]).sum())
        a[0], a[1] = a[0][:, drop:], a[1][:, drop:]
        ref = one.generate(*a, **{k: [v[i]] for k, v in kw.items() if k != "suppress_tokens" and k != "min_new_tokens"}, min_new_tokens=M + 2,
                           suppress_tokens=sup, **{k: [v[i]] for k, v in warp.items()})
        n = ref.codes.shape[1]
        assert np.array_equal(_np(out.codes)[i, :n], _np(ref.codes)[0]), i
    return eng.last_refill


def test_a_warper_request_admitted_into_a_stream_that_ran_without_any(dev):
    body_admitted_warper(dev)


def body_pooled_restart(dev):
    """A pooled engine small enough to preempt: the restarted request has warpers and n = 2 and yields the codes of the unpreempted run."""
    from qwen3_tts_amd.talker import TalkerEngine
    t, w = rs._tiny()
    N, M = 4, 40
    args, lens = rs._prompt(t, N, seed=61)
    sup = _suppress(t)
    kw = dict(max_new_tokens=[M] * N, min_new_tokens=M + 2, suppress_tokens=sup, seed=[700 + i for i in range(N)], schedule="continuous",
              min_p=[0.2] * N, typical_p=[0.6, None, 0.6, None], no_repeat_ngram_size=[2] * N)
    big = TalkerEngine(t, w, weight_dtype=torch.float32, device=dev, max_batch=N, max_seq=64, use_graph=False)
    ref = big.generate(*args, **kw)
    assert big.sampler_class()[0] == 3
    small = TalkerEngine(t, w, weight_dtype=torch.float32, device=dev, max_batch=N, max_seq=64, use_graph=False, kv_pages=9)
    out = small.generate(*args, **kw)
    assert small.last_refill["preemptions"] >= 1 and small.sampler_class()[0] == 3, small.last_refill
    assert np.array_equal(_np(out.codes), _np(ref.codes))
    plain = small.generate(*args, **{k: v for k, v in kw.items() if k not in WARP})
    assert small.sampler_class()[0] == 1
    for i in range(N):                                            # every request really ran under its warpers
        assert not np.array_equal(_np(out.codes)[i], _np(plain.codes)[i]), i


def test_a_preempted_warper_request_restarts_to_the_same_codes(dev):
    body_pooled_restart(dev)


# ============================================================================================ 6. wrapper
def body_wrapper(dev):
    """`Qwen3TTSModel.generate_custom_voice(..., min_p=[...], no_repeat_ngram_size=2, seed=[...])`: the engine receives that table (the
    sampler class is 3), the engine-level call with the same arguments gives the same codes, and the waveforms differ from the call
    without the two arguments."""
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
    kw = dict(language=langs, max_new_tokens=10, seed=[11, 12, 13])
    calls = []
    inner = model.talker.generate

    def spy(*a, **k):
        out = inner(*a, **k)
        calls.append((a, k, _np(out.codes)))
        return out
    model.talker.generate = spy
    try:
        a, sr = tts.generate_custom_voice(texts, spk, min_p=[0.3, None, 0.5], no_repeat_ngram_size=2, **kw)
    finally:
        model.talker.generate = inner
    assert model.talker.sampler_class()[0] == 3
    assert len(calls) == 1 and calls[0][1]["min_p"] == [0.3, None, 0.5] and calls[0][1]["no_repeat_ngram_size"] == 2
    again = inner(*calls[0][0], **calls[0][1])
    assert np.array_equal(_np(again.codes), calls[0][2])
    direct = inner(*calls[0][0], **{**calls[0][1], "min_p": [0.3, 0.0, 0.5], "no_repeat_ngram_size": [2, 2, 2]})
    assert np.array_equal(_np(direct.codes), calls[0][2])
    b, _ = tts.generate_custom_voice(texts, spk, **kw)
    assert model.talker.sampler_class()[0] == 1
    assert len(a) == len(b) == 3 and any(x.shape != y.shape or not np.array_equal(x, y) for x, y in zip(a, b))
    # values that are off under HF's gating leave a scalar call on the scalar path, with the plain call's waveforms
    kw1 = dict(kw, seed=7)
    p1, _ = tts.generate_custom_voice(texts, spk, **kw1)
    assert model.talker.sampler_class() == (0, 0)
    p2, _ = tts.generate_custom_voice(texts, spk, min_p=0, typical_p=1.0, epsilon_cutoff=0.0, no_repeat_ngram_size=0, **kw1)
    assert model.talker.sampler_class() == (0, 0)
    assert all(np.array_equal(x, y) for x, y in zip(p1, p2))


def test_wrapper_passes_the_warpers_to_the_engine(dev):
    body_wrapper(dev)
