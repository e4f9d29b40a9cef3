"""Per-request sampling settings and seeds within one talker batch (include/qtts.h: qtts_row_sampling, qtts_talker_generate_rows,
qtts_talker_stream_begin_rows; `TalkerEngine.generate(..., temperature=[...], seed=[...])`): the samplers read every knob of a row
from a device table, so requests with different settings share a wave, a request's draws are a function of its own seed, and a change
of the values replays the captured frame graph.

The test BODIES (`body_*`) take the device; tests/test_row_sampling_hostemu.py runs the same bodies on the host-emulation build."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import synth
import talker_ref
from qwen3_tts_amd import _lib as _qlib
from test_gpu_parity import _philox4x32_10, _sampler_slot_order, _suppress, _td, _u_gap, dev  # noqa: F401  (`dev` is a fixture)

pytestmark = pytest.mark.gpu

TOL = 2e-5            # tests/test_gpu_parity.py::_sampled_path_body_1: fp32 softmax + scan against the float64 restatement; u has 24 bits
KNOBS = ("do_sample", "top_k", "top_p", "temperature", "repetition_penalty", "subtalker_dosample", "subtalker_top_k", "subtalker_top_p",
         "subtalker_temperature")


def _tiny():
    t = synth.talker_tiny()
    return t, _td(synth.talker_weights(t))


def _engine(t, w, dev, dtype, graph, B, max_seq=64):
    from qwen3_tts_amd.talker import TalkerEngine
    return TalkerEngine(t, w, weight_dtype=dtype, device=dev, max_batch=B, max_seq=max_seq, use_graph=graph)


def _prompt(t, B, seed=78):
    lens = [int(x) for x in np.random.default_rng(seed - 1).integers(5, 12, B)]
    lens[B // 2] = 12                                            # one longest row, so that subsets can keep the left padding
    return synth.rand_prompt(np.random.default_rng(seed), t, lens, 3, scale=0.5), lens


def _np(x):
    return x.cpu().numpy().copy()          # (a copy: a view would keep the engine's output block alive, and the next call off it)


def _ptrs(out):
    """The output blocks of a call: part of the frame graph's key (a call that gets other blocks from the allocator re-captures)."""
    return (out.codes.data_ptr(), out.hidden.data_ptr(), out.tokens.data_ptr())


# ============================================================================================ 1. greedy through the table
def body_greedy_table(dev, golden_dir, graph):
    """Every row greedy, fp32: the table run is the reference's run (tests/golden/talker_tiny.npz) and the scalar greedy call, bit for
    bit -- codes, hidden states and every token but the last, which a table run replaces by eos (include/qtts.h: a row that reached its
    own limit m receives eos from token index m - 1 on; a scalar run keeps the sampled token there)."""
    from test_gpu_parity import _compare_greedy
    t, w = _tiny()
    g = np.load(os.path.join(golden_dir, "talker_tiny.npz"))
    args = [torch.from_numpy(g[k]) for k in ("embeds", "mask", "trailing", "tts_pad")]
    B = args[0].shape[0]
    eng = _engine(t, w, dev, torch.float32, graph, 4, 128)
    kw = dict(min_new_tokens=2, subtalker_dosample=False, repetition_penalty=1.05, suppress_tokens=_suppress(t))
    ref = eng.generate(*args, max_new_tokens=14, do_sample=False, **kw)
    assert eng.stats()["row_table_last"] == 0
    out = eng.generate(*args, max_new_tokens=[14] * B, do_sample=[False] * B, **kw)
    assert eng.stats()["row_table_last"] == 1
    codes, tokens = _np(out.codes), _np(out.tokens)
    n = g["codes"].shape[1]
    assert codes.shape == g["codes"].shape and tokens.shape[1] == n + 1
    assert (tokens[:, n] == t.codec_eos_token_id).all()
    gt = g["tokens"].copy()
    gt[:, n] = t.codec_eos_token_id
    assert _compare_greedy(codes, tokens, g["codes"], gt, g["margin"]) == n
    assert np.array_equal(codes, _np(ref.codes)) and np.array_equal(tokens[:, :n], _np(ref.tokens)[:, :n])
    assert np.array_equal(_np(out.hidden), _np(ref.hidden))
    again = eng.generate(*args, max_new_tokens=14, do_sample=False, **kw)          # the scalar path after a table call
    assert eng.stats()["row_table_last"] == 0 and np.array_equal(_np(again.tokens), _np(ref.tokens))


@pytest.mark.parametrize("graph", [False, True])
def test_greedy_rows_through_the_table_are_the_reference_run(dev, golden_dir, graph):
    body_greedy_table(dev, golden_dir, graph)


# ============================================================================================ 2. / 3. per-draw check
def _gap(raw, hist, tok, step, stream, s, sub, t, sup, floor):
    """How far u = Philox(seed_b; step, 0, stream) lies outside the interval of `tok` in the inverse CDF of the processed softmax of `raw`
    (one row's raw logits) under the settings `s` of one row, scanned in the kernel's order (<= 0: inside; 1: outside the support)."""
    pre = "subtalker_" if sub else ""
    top_k, top_p, temp = s[pre + "top_k"], s[pre + "top_p"], s[pre + "temperature"]
    kw = dict(do_sample=True, temperature=temp, top_k=top_k, top_p=top_p)
    if not sub:
        kw.update(repetition_penalty=s["repetition_penalty"], eos_id=t.codec_eos_token_id, min_new_tokens=floor, suppress=sup)
    p = torch.softmax(talker_ref.process_logits(raw[None], hist[None], **kw).double(), -1).numpy()
    V = p.shape[1]
    if p[0, tok] <= 0:
        return 1.0
    # candidates of a top-k <= 256 are scanned in slot order (wave, slice, lane) by both kernels; without that bound sample_kernel scans
    # the vocabulary in index order
    so = _sampler_slot_order(V) if 0 < top_k <= 256 and top_k < V else np.arange(V)
    seed = s["seed"]
    c0 = _philox4x32_10(np.array([step]), 0, stream, 0, seed & 0xFFFFFFFF, seed >> 32)[0]
    u = (c0 >> np.uint64(8)).astype(np.float64) / 16777216.0
    return float(_u_gap(p, so, np.argsort(so), np.array([0]), np.array([tok]), u)[0])


def _row(table, b):
    return {k: v[b] for k, v in table.items()}


def _draw_check(eng, t, args, table, M):
    """One table call of M tokens with EOS blocked throughout, then the per-draw check on its LAST frame's 15 sub-codes (frame M - 2,
    drawn under step counter M - 1) from the engine's own raw logits.  The talker token of step M - 1 is checked too, against the raw
    logits this call leaves behind -- but a table run shows eos at a row's last index, so the drawn token is read from a second call
    with limit M + 1 (same seeds: same history, asserted).  Returns (worst gap with the rows' own settings, worst gap with the settings
    and seed of row (b + 1) % B, the short call's (codes, tokens, hidden, output block addresses), a closure that runs the second call);
    the call's output tensors are released before it returns, so that the allocator can hand the same blocks to the next call."""
    B = args[0].shape[0]
    sup = _suppress(t)
    out = eng.generate(*args, max_new_tokens=[M] * B, min_new_tokens=M + 1, suppress_tokens=sup, **table)
    assert eng.stats()["row_table_last"] == 1
    toks, codes, res = _np(out.tokens), _np(out.codes), (_np(out.codes), _np(out.tokens), _np(out.hidden), _ptrs(out))
    del out
    assert toks.shape == (B, M) and codes.shape[1] == M - 1
    raw, cp_raw = eng.debug_logits()[:B].cpu(), eng.debug_cp_logits()[:, :B].cpu()
    empty = torch.zeros(0, dtype=torch.long)
    own, other = -1.0, -1.0
    for b in range(B):
        s, o = _row(table, b), _row(table, (b + 1) % B)
        if not s["subtalker_dosample"]:
            continue
        for j in range(t.num_code_groups - 1):
            tk = int(codes[b, M - 2, 1 + j])
            own = max(own, _gap(cp_raw[j, b], empty, tk, M - 1, 1 + j, s, True, t, sup, 0))
            other = max(other, _gap(cp_raw[j, b], empty, tk, M - 1, 1 + j, o, True, t, sup, 0))

    def talker_step():
        lng = eng.generate(*args, max_new_tokens=[M + 1] * B, min_new_tokens=M + 1, suppress_tokens=sup, **table)
        lt = _np(lng.tokens)
        assert np.array_equal(lt[:, :M - 1], toks[:, :M - 1]) and np.array_equal(_np(lng.codes)[:, :M - 1], codes)
        a, c = -1.0, -1.0
        for b in range(B):
            s, o = _row(table, b), _row(table, (b + 1) % B)
            if not s["do_sample"]:
                continue
            hist = torch.from_numpy(lt[b, :M - 1])
            a = max(a, _gap(raw[b], hist, int(lt[b, M - 1]), M - 1, 0, s, False, t, sup, M + 1))
            c = max(c, _gap(raw[b], hist, int(lt[b, M - 1]), M - 1, 0, o, False, t, sup, M + 1))
        return a, c
    return own, other, res, talker_step


def _fast_table(B, shift):
    pick = lambda vals, k: [vals[(b * k + shift) % len(vals)] for b in range(B)]
    return dict(do_sample=[True] * B, top_k=pick([5, 20, 50, 64], 1), top_p=[1.0] * B, temperature=pick([0.6, 0.9, 1.3], 1),
                repetition_penalty=pick([1.0, 1.05, 1.5], 2), subtalker_dosample=[True] * B, subtalker_top_k=pick([50, 5, 64, 20], 1),
                subtalker_top_p=[1.0] * B, subtalker_temperature=pick([0.9, 1.3, 0.6], 1), seed=[1000 * (shift + 1) + 17 * b for b in range(B)])


def body_fast_class(dev, t, w, dtype, graph, B, calls=3, M=5):
    """Every row samples with its own temperature, top-k, repetition penalty and seed (all inside sample_kernel_v2's class); the values
    change between consecutive calls on one engine.  Each draw of the last frame and the last talker step lies in ITS ROW's inverse-CDF
    interval for u = Philox(seed_b; step, 0, stream) within TOL; evaluated with the neighbouring row's settings and seed the same draws
    miss by more than 1e-3 (the check can tell rows apart).  On a graph engine no call after the first captures: nothing is baked in."""
    eng = _engine(t, w, dev, dtype, graph, B)
    args, _ = _prompt(t, B)
    later, caps, blocks, replays = [], [], [], 0
    for i in range(calls):
        own, other, res, talker_step = _draw_check(eng, t, args, _fast_table(B, i), M)
        caps.append(eng.stats()["graph_captures"])
        blocks.append(res[3])
        print(f"row table, fast class, call {i}: sub-code draws worst gap {own:.2e} (neighbour's settings: {other:.2e}), captures {caps[-1]}")
        assert own <= TOL, (i, own)
        assert other > 1e-3, (i, other)
        later.append(talker_step)
        # the frame graph's key holds the output blocks and no sampling value: same blocks, other values -> no capture
        if graph and i and blocks[i] == blocks[i - 1]:
            assert caps[i] == caps[i - 1], caps
            replays += 1
    if graph:
        assert caps[0] >= 1 and eng.stats()["graph_nodes"] > 0
        if dev != "cpu":              # (torch's caching allocator hands a freed block of the same size back; malloc need not)
            assert replays == calls - 1, (caps, blocks)
    else:
        assert caps[-1] == 0
    for i, step in enumerate(later):
        own, other = step()
        print(f"row table, fast class, call {i}: talker draw worst gap {own:.2e} (neighbour's settings: {other:.2e})")
        assert own <= TOL and other > 1e-3, (i, own, other)


@pytest.mark.parametrize("dtype,graph", [(torch.bfloat16, True), (torch.float32, False)])
@pytest.mark.parametrize("B", [4, 8])
def test_every_row_draws_under_its_own_settings_fast_class(dev, dtype, graph, B):
    body_fast_class(dev, *_tiny(), dtype, graph, B)


def test_every_row_draws_under_its_own_settings_at_the_benchmarked_vocabularies(dev):
    """V = 3072 / 2048: sample_kernel_v2<12> and <8>, the instantiations the headline runs (0.6B dims, 2 talker layers, bf16, graph)."""
    t = synth.talker_06b()
    t.num_hidden_layers = 2
    assert t.vocab_size == 3072 and t.cp_vocab_size == 2048
    body_fast_class(dev, t, _td(synth.talker_weights(t, with_text=False)), torch.bfloat16, True, 8, calls=2)


def _general_table(B):
    base = [dict(do_sample=False, top_k=50, top_p=1.0, subtalker_dosample=False, subtalker_top_k=50, subtalker_top_p=1.0),   # greedy
            dict(do_sample=True, top_k=0, top_p=0.9, subtalker_dosample=True, subtalker_top_k=0, subtalker_top_p=0.9),     # top-p only
            dict(do_sample=True, top_k=300, top_p=1.0, subtalker_dosample=True, subtalker_top_k=300, subtalker_top_p=1.0),
            dict(do_sample=True, top_k=50, top_p=1.0, subtalker_dosample=True, subtalker_top_k=50, subtalker_top_p=1.0)]
    tab = {k: [base[b % 4][k] for b in range(B)] for k in base[0]}
    tab.update(temperature=[[0.9, 1.3, 0.6][b % 3] for b in range(B)], subtalker_temperature=[[1.3, 0.6, 0.9][b % 3] for b in range(B)],
               repetition_penalty=[[1.05, 1.5, 1.0][b % 3] for b in range(B)], seed=[77 + 5 * b for b in range(B)])
    return tab


def body_general_class(dev, dtype, graph, B=4, M=5):
    """One batch with a greedy row, a top-p-only row, a top-k 300 row and a top-k 50 row: the general kernel serves all of them.  The
    sampling rows pass the per-draw check; the greedy rows equal the same rows of the scalar greedy call.  On a graph engine the class
    switch (this table after an all-fast one) re-captures the one frame graph of a short sequence, and a second general table replays."""
    t, w = _tiny()
    eng = _engine(t, w, dev, dtype, graph, B)
    args, _ = _prompt(t, B)
    sup = _suppress(t)
    b0 = _draw_check(eng, t, args, _fast_table(B, 0), M)[2][3]
    c0 = eng.stats()["graph_captures"]
    tab = _general_table(B)
    own, other, out, talker_step = _draw_check(eng, t, args, tab, M)
    c1 = eng.stats()["graph_captures"]
    tab2 = dict(tab, seed=[s + 1 for s in tab["seed"]], temperature=tab["temperature"][::-1])
    own2, _, out2, _ = _draw_check(eng, t, args, tab2, M)
    c2 = eng.stats()["graph_captures"]
    print(f"row table, general class: sub-code draws worst gap {own:.2e} / {own2:.2e} (neighbour's settings: {other:.2e}); captures {c0} -> {c1} -> {c2}")
    assert own <= TOL and own2 <= TOL and other > 1e-3
    if not graph:
        assert (c1, c2) == (0, 0)
    else:
        assert c1 == c0 + 1                                       # the class switch: the one frame graph of a short sequence again
        if out2[3] == out[3]:
            assert c2 == c1                                       # same class, same blocks, other values: replayed
        if dev != "cpu":
            assert b0 == out[3] == out2[3], "the allocator did not hand the output blocks back: nothing was shown about replay"
    a, c = talker_step()
    assert a <= TOL and c > 1e-3, (a, c)
    ref = eng.generate(*args, max_new_tokens=M, min_new_tokens=M + 1, do_sample=False, subtalker_dosample=False, repetition_penalty=1.05,
                       suppress_tokens=sup)
    for b in range(0, B, 4):
        assert np.array_equal(out[0][b], _np(ref.codes)[b]) and np.array_equal(out[2][b], _np(ref.hidden)[b])
        assert np.array_equal(out[1][b, :M - 1], _np(ref.tokens)[b, :M - 1])


@pytest.mark.parametrize("dtype,graph", [(torch.bfloat16, True), (torch.float32, False)])
def test_greedy_top_p_only_and_large_top_k_rows_share_a_batch(dev, dtype, graph):
    body_general_class(dev, dtype, graph)


# ============================================================================================ 4. position independence
def body_position_independence(dev, dtype, graph=True, B=8, M=5):
    """Ragged prompts, sampling: the rows permuted together with their table entries give the same permutation of codes, tokens and
    hidden states, bit for bit; so do the 4 rows that include the longest prompt (same left padding) called on their own."""
    t, w = _tiny()
    eng = _engine(t, w, dev, dtype, graph, B)
    args, lens = _prompt(t, B)
    tab = _fast_table(B, 1)
    kw = dict(min_new_tokens=2, suppress_tokens=_suppress(t))
    full = eng.generate(*args, max_new_tokens=[M] * B, **kw, **tab)
    assert full.codes.shape[1] >= 1
    perm = [int(x) for x in np.random.default_rng(5).permutation(B)]
    sel = lambda idx: ([a[idx] for a in args[:3]] + [args[3]], {k: [v[i] for i in idx] for k, v in tab.items()})
    for idx in (perm, sorted({B // 2, 0, 1, B - 1})):
        a, tb = sel(idx)
        part = eng.generate(*a, max_new_tokens=[M] * len(idx), **kw, **tb)
        # (a subset may stop earlier or later than the whole batch: compare the steps both ran)
        n = min(part.codes.shape[1], full.codes.shape[1])
        assert n >= 1
        assert np.array_equal(_np(part.codes)[:, :n], _np(full.codes)[idx, :n]), idx
        assert np.array_equal(_np(part.tokens)[:, :n], _np(full.tokens)[idx, :n]), idx
        assert np.array_equal(_np(part.hidden)[:, :n], _np(full.hidden)[idx, :n]), idx
        if len(idx) == B:
            assert part.codes.shape == full.codes.shape and np.array_equal(_np(part.tokens), _np(full.tokens)[idx])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_a_rows_output_does_not_depend_on_its_place_in_the_batch(dev, dtype):
    body_position_independence(dev, dtype)


def _fake_ids(t, text):
    body = [(ord(ch) * 7) % 490 for ch in text][:40]
    a, n = 77, 198
    return torch.tensor([[t.im_start_token_id, a, n] + body + [t.im_end_token_id, n, t.im_start_token_id, a, n]])


def body_model_waves(dev):
    """`Qwen3TTSForConditionalGeneration.generate`, 8 equal-length requests in waves of 4 with a seed per request: the same requests in
    reversed order (other wave, other row) get the same codes."""
    from qwen3_tts_amd.model import Qwen3TTSForConditionalGeneration
    t = synth.talker_tiny()
    cfgd = dict(synth.cfg_dict(t), tts_model_type="custom_voice", tts_model_size="tiny", tokenizer_type="12hz")
    model = Qwen3TTSForConditionalGeneration(cfgd, _td(synth.talker_weights(t)), device=dev, dtype=torch.float32, max_batch=4, max_seq=128)
    ids = [_fake_ids(t, "request %d!" % i) for i in range(8)]
    assert len({x.shape[1] for x in ids}) == 1
    kw = dict(languages=["english"] * 8, speakers=["vivian", "ryan"] * 4, max_new_tokens=6)
    seeds = [300 + i for i in range(8)]
    temps = [0.6 + 0.1 * i for i in range(8)]
    fwd, _ = model.generate(input_ids=ids, seed=seeds, temperature=temps, **kw)
    rev, _ = model.generate(input_ids=ids[::-1], seed=seeds[::-1], temperature=temps[::-1], **dict(kw, speakers=kw["speakers"][::-1]))
    assert len(fwd) == len(rev) == 8
    for i in range(8):
        assert np.array_equal(_np(fwd[i]), _np(rev[7 - i])), i
    assert len({_np(c).tobytes() for c in fwd}) > 1
    with pytest.raises(ValueError, match="entries for 8 requests"):
        model.generate(input_ids=ids, seed=seeds[:3], **kw)


def test_a_request_keeps_its_codes_whatever_wave_it_lands_in(dev):
    body_model_waves(dev)


def body_requests_without_own_seeds(dev):
    """Per-request knobs but no seed list: 8 IDENTICAL requests (same text, speaker and temperature) in waves of 4 must not repeat each
    other -- the table's Philox counter has no row term, so one seed for all rows would give every request the same draws.  With no
    seed every request draws its own; with ONE integer s, request i samples with s + i (the same codes as the list [s, s + 1, ...],
    repeatable).  The same at the engine: identical rows under one integer seed differ, row b's seed is s + b."""
    from qwen3_tts_amd.model import Qwen3TTSForConditionalGeneration
    t = synth.talker_tiny()
    w = _td(synth.talker_weights(t))
    cfgd = dict(synth.cfg_dict(t), tts_model_type="custom_voice", tts_model_size="tiny", tokenizer_type="12hz")
    model = Qwen3TTSForConditionalGeneration(cfgd, w, device=dev, dtype=torch.float32, max_batch=4, max_seq=128)
    ids = [_fake_ids(t, "the same request")] * 8
    kw = dict(input_ids=ids, languages=["english"] * 8, speakers=["vivian"] * 8, max_new_tokens=6, temperature=[1.2] * 8)
    distinct = lambda codes: len({_np(c).tobytes() for c in codes})
    torch.manual_seed(1234)
    free, _ = model.generate(**kw)
    assert len(free) == 8 and distinct(free) == 8, "identical requests without seeds repeated each other's draws"
    one, _ = model.generate(seed=40, **kw)
    again, _ = model.generate(seed=40, **kw)
    listed, _ = model.generate(seed=[40 + i for i in range(8)], **kw)
    assert distinct(one) == 8
    for i in range(8):
        assert np.array_equal(_np(one[i]), _np(again[i])) and np.array_equal(_np(one[i]), _np(listed[i])), i
    # the engine itself, rows 0..3 all the longest prompt of `_prompt`
    eng = _engine(t, w, dev, torch.float32, False, 4)
    (emb, mask, trail, pad), _ = _prompt(t, 4)
    args = [x[[2] * 4] for x in (emb, mask, trail)] + [pad]
    ekw = dict(max_new_tokens=5, min_new_tokens=2, temperature=[1.2] * 4, suppress_tokens=_suppress(t))
    a, b = _np(eng.generate(*args, seed=7, **ekw).codes), _np(eng.generate(*args, seed=[7, 8, 9, 10], **ekw).codes)
    assert np.array_equal(a, b) and len({r.tobytes() for r in a}) == 4
    torch.manual_seed(99)
    assert len({r.tobytes() for r in _np(eng.generate(*args, **ekw).codes)}) == 4


def test_identical_requests_without_own_seeds_do_not_share_draws(dev):
    body_requests_without_own_seeds(dev)


# ============================================================================================ 5. per-row limits
def body_row_limits(dev, graph):
    """Greedy, limits [3, 6, 4, 6]: row b's frames are the first m_b - 1 frames of the unlimited run, its tokens are eos from index
    m_b - 1 on, the call has 5 frames; limits [3, 3, 4, 3] end the call at 3 frames.  A row's own min_new_tokens blocks its EOS."""
    t, w = _tiny()
    eng = _engine(t, w, dev, torch.float32, graph, 4)
    args, _ = _prompt(t, 4, seed=91)
    sup = _suppress(t)
    eos = t.codec_eos_token_id
    kw = dict(do_sample=False, subtalker_dosample=False, repetition_penalty=1.05, suppress_tokens=sup)
    ref = eng.generate(*args, max_new_tokens=6, min_new_tokens=2, **kw)
    rc, rt = _np(ref.codes), _np(ref.tokens)
    assert rc.shape[1] == 5 and not (rt == eos).any(), "the unlimited run must not meet a real EOS for this comparison"
    for limits, frames in (([3, 6, 4, 6], 5), ([3, 3, 4, 3], 3)):
        out = eng.generate(*args, max_new_tokens=limits, min_new_tokens=[2] * 4, **kw)
        codes, toks = _np(out.codes), _np(out.tokens)
        assert out.n_frames == frames and codes.shape[1] == frames and toks.shape[1] == frames + 1
        st = eng.stats()
        assert st["frames_run"] == frames and st["row_table_last"] == 1
        for b, m in enumerate(limits):
            assert np.array_equal(codes[b, :m - 1], rc[b, :m - 1]) and np.array_equal(toks[b, :m - 1], rt[b, :m - 1]), (limits, b)
            assert (toks[b, m - 1:] == eos).all(), (limits, b, toks[b])
            assert (codes[b, m - 1:, 0] == eos).all()              # the trimming rule (M:2283-2289) cuts the row at m - 1 frames
            assert np.array_equal(_np(out.hidden)[b, :m - 1], _np(ref.hidden)[b, :m - 1])
    # per-row floor: with eos' := the token row 0 emits at index 1 (the original eos joins the suppress list, so the scores of the
    # first two steps are those of the run above), a floor of 1 lets row 0 stop there and a floor of 4 does not
    eos2 = int(rt[0, 1])
    assert rt[0, 0] != eos2
    sup2 = sup + [eos]
    for floors in ([1, 4, 1, 4], [4, 1, 4, 1]):
        out = eng.generate(*args, max_new_tokens=[6] * 4, min_new_tokens=floors, eos_token_id=eos2, **dict(kw, suppress_tokens=sup2))
        toks = _np(out.tokens)
        for b, fl in enumerate(floors):
            hit = np.nonzero(toks[b] == eos2)[0]
            assert len(hit) == 0 or hit[0] >= fl, (floors, b, toks[b])
        if floors[0] == 1:
            assert toks[0, 0] == rt[0, 0] and (toks[0, 1:] == eos2).all(), toks[0]
        else:
            assert not (toks[0, :4] == eos2).any(), toks[0]


@pytest.mark.parametrize("graph", [False, True])
def test_rows_stop_at_their_own_limits_and_floors(dev, graph):
    body_row_limits(dev, graph)


# ============================================================================================ 6. streaming
def body_stream(dev, graph):
    """`generate_stream` with a table: the packets concatenate to the codes of `generate` with the same table."""
    t, w = _tiny()
    eng = _engine(t, w, dev, torch.float32, graph, 4)
    args, _ = _prompt(t, 4)
    tab = _fast_table(4, 2)
    kw = dict(max_new_tokens=[5, 7, 7, 4], min_new_tokens=2, suppress_tokens=_suppress(t))
    ref = _np(eng.generate(*args, **kw, **tab).codes)
    for packet in (1, 4):
        parts = [_np(p) for p in eng.generate_stream(*args, packet_frames=packet, **kw, **tab)]
        assert eng.stats()["row_table_last"] == 1
        assert all(0 < p.shape[1] <= packet for p in parts)
        assert np.array_equal(np.concatenate(parts, axis=1), ref), packet


@pytest.mark.parametrize("graph", [False, True])
def test_stream_packets_with_a_table_equal_generate(dev, graph):
    body_stream(dev, graph)


# ============================================================================================ 7. wrapper
def body_wrapper(dev):
    """`Qwen3TTSModel.generate_custom_voice` with per-request temperature, seed and max_new_tokens: one waveform per text, repeatable,
    and a change of request 0's seed alone leaves the other requests' waveforms bit-identical."""
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
    assert tts._merge_generate_kwargs(temperature=[None, 0.5])["temperature"] == [0.9, 0.5]
    texts, spk, langs = ["hello world", "a rather longer sentence to speak", "third"], ["vivian", "ryan", "vivian"], ["english", "chinese", "english"]
    kw = dict(language=langs, temperature=[0.7, None, 1.2], max_new_tokens=[6, 9, 7])
    a, sr = tts.generate_custom_voice(texts, spk, seed=[11, 12, 13], **kw)
    b, _ = tts.generate_custom_voice(texts, spk, seed=[11, 12, 13], **kw)
    d, _ = tts.generate_custom_voice(texts, spk, seed=[99, 12, 13], **kw)
    assert len(a) == len(b) == len(d) == 3 and sr > 0
    for i in range(3):
        assert a[i].size > 0 and np.array_equal(a[i], b[i]), i
        assert a[i].shape[0] <= (kw["max_new_tokens"][i] - 1) * c.total_upsample
    assert np.array_equal(a[1], d[1]) and np.array_equal(a[2], d[2])
    assert a[0].shape != d[0].shape or not np.array_equal(a[0], d[0])


def test_wrapper_takes_per_request_settings(dev):
    body_wrapper(dev)
