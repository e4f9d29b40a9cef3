"""Shared KV page pool for the talker cache (include/qtts.h: qtts_talker_set_kv_pool, qtts_talker_stream_kv, qtts_talker_stream_evict;
`TalkerEngine(kv_pages=...)`, `stream_kv()`, `stream_evict()`, the optimistic `generate(schedule="continuous")`): the cache is
`kv_pages` pages of 16 keys that the rows take as they grow, instead of max_batch x max_seq keys reserved per row; a continuous stream
that runs out of pages preempts by restart.

Every request's result is pinned to what the REFERENCE produced for it (tests/golden/talker_tiny_admit.npz, as in
tests/test_row_positions_gpu.py: 24 ragged requests, prompts of 3..15 rows, limits 3..13, greedy, every margin >= 1e-3).  Geometry: 4 rows,
max_seq 32 = two pages per row; a 15-row prompt takes its second page with the step that appends slot 16.  A test that needs longer
prompts left-pads the group (`Tg`): a pad consumes cache slots without changing the reference's codes.

Page counts are kept here from the rule alone: a row admitted at T holds ceil(T / 16) pages; before a step of n frames a running row of
length len under the limit L that has run k steps holds ceil((len + min(n, L - 1 - k)) / 16); a finished row holds none once a
`stream_step` / `stream_rows` return has observed it.

The test BODIES (`body_*`) take the device; tests/test_kv_pool_hostemu.py runs the same bodies on the host-emulation build."""
import os

import numpy as np
import pytest
import torch

from qwen3_tts_amd import _lib as _qlib
from test_gpu_parity import _suppress, dev  # noqa: F401  (`dev` is a fixture)
from test_row_sampling_gpu import _np
import test_refill_gpu as rg
import test_row_positions_gpu as rp

pytestmark = pytest.mark.gpu
gga, LENS = rg.gga, rg.LENS
QTTS_ERR_ARG, QTTS_ERR_STATE, QTTS_ERR_LIMIT = -1, -3, -6
MAX_SEQ = 32


def _engine(t, w, dev, dtype, graph, B=4, max_seq=MAX_SEQ, kv_pages=None):
    from qwen3_tts_amd.talker import TalkerEngine
    return TalkerEngine(t, w, weight_dtype=dtype, device=dev, max_batch=B, max_seq=max_seq, use_graph=graph, kv_pages=kv_pages)


def _pages(n_keys):
    return -(-n_keys // 16)


class PoolStream(rp.RowStream):
    """`RowStream` that also keeps the host's own page count: `held[b]` as the rule in the module docstring gives it."""

    def __init__(self, eng, *a, **k):
        super().__init__(eng, *a, **k)
        self.pool = eng.kv_pages
        self.held = [_pages(x) for x in self.base]
        self.gone = set()             # rows whose occupant was evicted: frozen where they were
        self.frozen = {}

    def lens_now(self):
        return [self.frozen.get(b, x) for b, x in enumerate(self.expected_lens())]

    def check_kv(self):
        got = self.eng.stream_kv()
        assert got == (self.held, self.pool - sum(self.held), self.pool), (got, self.held)
        return got

    def running(self, b):
        return b not in self.gone and self.age[b] < self.limit[b] - 1

    def want(self, n):
        lens = self.lens_now()
        return [max(self.held[b], _pages(lens[b] + min(n, self.limit[b] - 1 - self.age[b]))) if self.running(b) else 0 for b in range(len(self.held))]

    def step(self, n):
        want = self.want(n)
        out = super().step(n)            # (a refused step raises before the count moves)
        self.held = [w if self.running(b) else 0 for b, w in enumerate(want)]
        return out

    def rows(self):
        out = super().rows()
        self.held = [h if self.running(b) else 0 for b, h in enumerate(self.held)]
        return out

    def evict(self, rows_):
        lens = self.lens_now()
        self.eng.stream_evict(rows_)
        for b in rows_:
            self.gone.add(b)
            self.frozen[b], self.held[b], self.slot[b] = lens[b], 0, None

    def admit(self, pairs, Tg=None):
        super().admit(pairs, Tg)
        for b, _ in pairs:
            self.gone.discard(b)
            self.frozen.pop(b, None)
            self.held[b] = _pages(self.base[b])

    def check_lens(self):
        got = self.eng.stream_row_lens()
        assert got == self.lens_now(), (got, self.lens_now())
        return got


# ============================================================================================ 3. a pool of the static size
def body_static_size(dev, golden_dir, graph):
    """24 requests on 4 rows, max_seq 32, kv_pages = 8 (what the static layout reserves), `schedule="continuous"`, fp32: codes and hidden
    states are bit-identical to the static engine's and the codes equal the fixture's; nothing is preempted; a grant captures no graph."""
    g, t, w, args = rg._fixture(golden_dir)
    kw = rp._continuous_kw(t)
    ref_eng = _engine(t, w, dev, torch.float32, graph)
    ref = ref_eng.generate(*args, schedule="continuous", **kw)
    ref_st = dict(ref_eng.last_refill)
    assert ref_st["pool_pages"] == 0 and ref_st["preemptions"] == 0
    eng = _engine(t, w, dev, torch.float32, graph, kv_pages=8)
    out = eng.generate(*args, schedule="continuous", **kw)
    st = eng.last_refill
    rp._check_all(g, t, out)
    assert np.array_equal(_np(out.codes), _np(ref.codes)) and np.array_equal(_np(out.hidden), _np(ref.hidden))
    assert st["preemptions"] == 0 and st["pool_pages"] == 8 and 4 <= st["peak_pages"] <= 8, st
    assert st["graph_captures"] == ref_st["graph_captures"] <= (1 if graph else 0), (st, ref_st)
    assert st["streams"] == 1 and eng.stats()["row_positions"] == 1


@pytest.mark.parametrize("graph", [False, True])
def test_a_pool_of_the_static_size_is_the_static_engine(dev, golden_dir, graph):
    body_static_size(dev, golden_dir, graph)


# ============================================================================================ 4. hand-driven exhaustion
def body_exhaustion(dev, golden_dir, graph):
    """4 rows, max_seq 32, 6 pages.  Four limit-13 requests left-padded to T = 15 hold one page each, two are free.  Step 1 appends slot
    15.  Step 2 would append slot 16 in all four rows: refused with QTTS_ERR_LIMIT naming 4 needed and 2 free, and `stream_rows`,
    `stream_row_lens` and `stream_kv` are what they were.  Rows 2 and 3 are evicted: the step passes.  The survivors run to their end and
    their pages are back after `stream_rows`; the two evicted requests are admitted again; all four requests' codes equal the fixture's.
    After every call `stream_kv` equals the host's count."""
    g, t, w, args = rg._fixture(golden_dir)
    reqs = [11, 1, 4, 6]
    limits = {r: 13 for r in reqs}
    eng = _engine(t, w, dev, torch.float32, graph, kv_pages=6)
    s = PoolStream(eng, t, args, reqs, rg._greedy_settings(limits), Tg=15)
    assert s.check_kv() == ([1, 1, 1, 1], 2, 6) and s.check_lens() == [15] * 4
    assert s.step(1) == (1, False)
    s.check_kv()
    before = (s.rows(), s.check_lens(), s.check_kv())
    caps = eng.stats()["graph_captures"]
    with pytest.raises(_qlib.QttsError, match=r"4 pages needed, 2 free") as ei:
        s.step(1)
    assert ei.value.code == QTTS_ERR_LIMIT
    assert (s.rows(), s.check_lens(), s.check_kv()) == before and before[1] == [16] * 4
    s.evict([2, 3])
    assert s.check_kv() == ([1, 1, 0, 0], 4, 6) and s.check_lens() == [16] * 4
    assert s.rows()[0] == [1, 1, 0, 0]
    assert s.step(1) == (2, False)
    assert s.check_kv() == ([2, 2, 0, 0], 2, 6) and s.check_lens() == [17, 17, 16, 16]
    fin = False
    while not fin:
        _, fin = s.step(1)
        s.check_kv()
        s.check_lens()
    assert s.retire() == [0, 1, 2, 3] and s.check_kv() == ([0] * 4, 6, 6)
    assert eng.stats()["graph_captures"] - caps <= (1 if graph else 0)
    s.admit([(0, 4), (1, 6)], Tg=15)
    assert s.check_kv() == ([1, 1, 0, 0], 4, 6) and s.check_lens() == [15, 15, 16, 16]
    fin = False
    while not fin:
        _, fin = s.step(1)
        s.check_kv()
    s.finish()
    assert sorted(s.out) == sorted(reqs)
    for r, codes in s.out.items():
        rg._check_request(g, t, codes, r, 13)


@pytest.mark.parametrize("graph", [False, True])
def test_a_step_the_pool_cannot_cover_is_refused_and_eviction_frees_it(dev, golden_dir, graph):
    body_exhaustion(dev, golden_dir, graph)


# ============================================================================================ 5. released pages and the sink
def body_sink(dev, golden_dir, dtype):
    """A stream of 2 rows on a pool of 3 pages.  Request 11 (limit 4, T = 15) finishes at length 17 holding two of the three pages (the
    spare row beside it, limit 1, gave its page back at the first step).  Request 1, then request 4 (limit 13 each, T = 15) take the other
    row: each grows to 26 keys, so its two pages include at least one the finished row held -- while that row idles for 24 further steps
    and appends at its frozen length every step.  Those appends must land in the sink: both neighbours' codes are the fixture's, and the
    frozen length stays 17."""
    g, t, w, args = rg._fixture(golden_dir)
    limits = {11: 4, 0: 1, 1: 13, 4: 13}
    eng = _engine(t, w, dev, dtype, True, kv_pages=3)
    s = PoolStream(eng, t, args, [11, 0], rg._greedy_settings(limits), Tg=15)
    assert s.check_kv() == ([1, 1], 1, 3)
    for k in (1, 2, 3):
        assert s.step(1) == (k, k == 3)
        s.check_kv()
    assert s.retire() == [0, 1] and s.check_lens()[0] == 17 and s.check_kv() == ([0, 0], 3, 3)
    idle = 0
    for r in (1, 4):
        s.admit([(1, r)], Tg=15)
        fin = False
        while not fin:
            _, fin = s.step(1)
            idle += 1
            assert s.check_lens()[0] == 17
            assert s.check_kv()[0][0] == 0
        assert s.retire() == [0, 1]
    assert idle > 16
    s.finish()
    rg._judge(g, t, dtype, {r: c for r, c in s.out.items() if r != 0}, limits)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_a_finished_row_idles_into_the_sink_while_a_neighbour_takes_its_pages(dev, golden_dir, dtype):
    body_sink(dev, golden_dir, dtype)


# ============================================================================================ 6. split-KV on a scattered table
def body_split_kv(dev, golden_dir, dtype, gq=False):
    """`test_row_positions_gpu.body_split_kv` on a pool of 20 pages (max_seq 192: 12 per row).  Rows 0 and 1 finish after two steps and
    release their pages one row after the other, so the 150-key prompt admitted next receives them last-released-first: its ten page ids
    are not monotonic.  It sits beside 46-key rows; the span goes 128 -> 256 -> 128 -> short.  fp32: the fixture's codes; bf16
    (transposed V pages): the project's bf16 bound.  `gq`: the general attention family serves every launch."""
    g, t, w, args = rg._fixture(golden_dir)
    limits = {0: 3, 13: 3, 7: 5, 2: 13, 15: 13, 10: 13}
    settings = rg._greedy_settings(limits)
    with _qlib.options(QTTS_ATTN_NSPLIT="2", QTTS_ATTN_SPLIT_FROM="20", QTTS_ATTN_SPLIT_KEYS="64", **({"QTTS_ATTN_GQ": "1"} if gq else {})):
        eng = _engine(t, w, dev, dtype, True, 4, 192, kv_pages=20)
    s = PoolStream(eng, t, args, [0, 13, 2, 15], settings, Tg=40)
    spans = []

    def run(n):
        for _ in range(n):
            s.step(1)
            s.check_lens()
            s.check_kv()
            spans.append(eng.stats()["attn_span_last"])
    assert s.check_kv() == ([3] * 4, 8, 20)
    run(2)
    assert spans == [128, 128] and s.retire() == [0, 1] and s.check_kv() == ([0, 0, 3, 3], 14, 20)
    s.admit([(0, 7)], Tg=150)
    assert s.check_lens() == [150, 41, 42, 42] and s.check_kv() == ([10, 0, 3, 3], 4, 20)
    # the device table itself: the long row holds ten distinct pages that are NOT in ascending order, none of them a neighbour's; every
    # entry behind them, and the whole table of the retired row, names the sink
    tab = [eng.debug_kv_table(b) for b in range(4)]
    ids = tab[0][:10]
    assert len(set(ids)) == 10 and all(0 <= x < 20 for x in ids) and any(x > y for x, y in zip(ids, ids[1:])), ids
    assert tab[0][10:] == [20] * 2 and tab[1] == [20] * 12 and all(tab[b][3:] == [20] * 9 for b in (2, 3)), tab
    assert len(set(ids) | set(tab[2][:3]) | set(tab[3][:3])) == 16, tab
    run(4)
    assert spans[2:] == [256] * 4 and eng.stats()["attn_nsplit_last"] == 2
    assert s.retire() == [0, 1] and s.check_lens() == [153, 41, 46, 46] and s.check_kv() == ([0, 0, 3, 3], 14, 20)
    run(1)
    assert spans[-1] == 128
    s.admit([(0, 10)])
    fin = False
    while not fin:
        _, fin = s.step(1)
        s.check_lens()
        s.check_kv()
        spans.append(eng.stats()["attn_span_last"])
    assert spans[7:] == [128] * 5 + [0] * 7, spans
    s.finish()
    assert (eng.stats()["attn_gq_per_step"] > 0) == gq
    assert sorted(s.out) == sorted(limits)
    rg._judge(g, t, dtype, s.out, limits)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_split_kv_reads_a_scattered_table(dev, golden_dir, dtype):
    body_split_kv(dev, golden_dir, dtype)


def test_the_general_attention_family_reads_a_scattered_table(dev, golden_dir):
    body_split_kv(dev, golden_dir, torch.float32, gq=True)


GQ_SHAPE = "gq4_hd64"     # talker 8 / 2 / 64, code predictor 8 / 1 / 64: neither the group nor the head_dim of the released shape


def body_gq_head_shape(dev, golden_dir, dtype, n_new):
    """One `talker_tiny_gq*` head shape (tools/gen_golden_gq.py; the REFERENCE's greedy run of 5 ragged rows) on a pool whose table has
    seen releases: the page-table forms of the general family (attn_gq.h) at a group and a head_dim other than the released ones.  The
    prompts are left-padded to T = 30 on max_seq 96 (6 entries per row).  A first `generate` of three tokens takes three pages per row (two
    for the prompt, then one more each); the next call's prefill releases them all and grants two per row again, last released first, so
    the rows' pages of the `n_new`-token call are scattered -- read back from the device table: distinct, some rows not ascending, every other entry the sink.  The result is the
    static engine's bit for bit (codes and hidden states: the same kernels on the same keys, only the addresses differ), in fp32 the
    reference's codes, in bf16 within the bar tests/test_attn_gq_gpu.py sets for this fixture (first two frames agree at >= 0.7)."""
    import test_attn_gq_gpu as gq
    g, t, w, args = gq._fixture(golden_dir, GQ_SHAPE)
    emb, mask = args[0], args[1]
    B, T, Tp = emb.shape[0], emb.shape[1], 30
    assert T < Tp
    args = [torch.cat([emb.new_zeros(B, Tp - T, emb.shape[2]), emb], 1), torch.cat([mask.new_zeros(B, Tp - T), mask], 1), args[2], args[3]]
    kw = dict(do_sample=False, subtalker_dosample=False, repetition_penalty=1.05, suppress_tokens=_suppress(t))
    want, pool = _pages(Tp + n_new), 32
    assert _pages(Tp) == 2 and _pages(Tp + 3) == 3 <= want <= 6
    ref = _engine(t, w, dev, dtype, True, 5, 96).generate(*args, max_new_tokens=n_new, min_new_tokens=n_new, **kw)
    eng = _engine(t, w, dev, dtype, True, 5, 96, kv_pages=pool)
    eng.generate(*args, max_new_tokens=3, min_new_tokens=3, **kw)
    assert eng.stream_kv() == ([3] * B, pool - 3 * B, pool)
    out = eng.generate(*args, max_new_tokens=n_new, min_new_tokens=n_new, **kw)
    assert eng.stream_kv() == ([want] * B, pool - want * B, pool)
    tab = [eng.debug_kv_table(b) for b in range(B)]
    held = [x for row in tab for x in row[:want]]
    assert len(set(held)) == B * want and all(0 <= x < pool for x in held) and all(row[want:] == [pool] * (6 - want) for row in tab), tab
    scattered = [b for b in range(B) if any(x > y for x, y in zip(tab[b], tab[b][1:want]))]
    assert scattered, tab
    assert eng.stats()["attn_gq_per_step"] == gq._per_step(t)
    codes, tokens = _np(out.codes), _np(out.tokens)
    assert codes.shape[1] == n_new - 1
    assert np.array_equal(codes, _np(ref.codes)) and np.array_equal(_np(out.hidden), _np(ref.hidden))
    if dtype == torch.float32:
        n = n_new - 1
        assert gq._compare_greedy(codes, tokens, g["codes"][:, :n], g["tokens"][:, :n + 1], g["margin"]) == n
    else:
        agree = float((codes[:, :2] == g["codes"][:, :2]).mean())
        print(f"{GQ_SHAPE} bf16, pooled, vs the fp32 golden, first 2 frames: {agree:.2f}")
        assert agree >= 0.7


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_another_head_shape_reads_a_scattered_table(dev, golden_dir, dtype):
    body_gq_head_shape(dev, golden_dir, dtype, 40)


# ============================================================================================ 7. the scheduler under a tight pool
TIGHT = 5


def _host_schedule_preempts(limits, pool, rows=4, packet=2, lens=None, max_seq=MAX_SEQ):
    """The optimistic schedule of `TalkerEngine._refill_stream` replayed on page counts alone (no engine): the number of evictions.  Every
    prompt of the fixture has at most 15 rows: one page, and every admission is one group.  A row admitted at T that has run k steps
    holds ceil((T + k) / 16) pages."""
    from qwen3_tts_amd.talker import TalkerEngine
    LENS = lens or rg.LENS
    queue = sorted(range(len(limits)), key=lambda i: (-LENS[i], i))
    first = TalkerEngine._widest_opener(queue, LENS, limits, max_seq, rows)
    assert len(first) == rows
    queue = [i for i in queue if i not in first]
    slot, age, T = list(first), [0] * rows, [max(LENS[i] for i in first)] * rows
    evictions = 0
    while any(r is not None for r in slot):
        while True:
            run = [b for b, r in enumerate(slot) if r is not None]
            if sum(_pages(T[b] + age[b] + min(packet, limits[slot[b]] - 1 - age[b])) for b in run) <= pool or len(run) <= 1:
                break
            v = min(run, key=lambda b: (age[b], -slot[b]))
            queue.insert(0, slot[v])
            slot[v] = None
            evictions += 1
        for b in range(rows):
            if slot[b] is not None:
                age[b] = min(age[b] + packet, limits[slot[b]] - 1)
                if age[b] == limits[slot[b]] - 1:
                    slot[b] = None
        free_rows = [b for b in range(rows) if slot[b] is None]
        free = pool - sum(_pages(T[b] + age[b]) for b in range(rows) if slot[b] is not None)
        running, take = rows - len(free_rows), []
        for i in queue[:len(free_rows)]:
            n = len(take) + 1
            if n + (running + n if running or take else 0) > free:
                break
            take.append(i)
        for b, i in zip(free_rows, take):
            slot[b], age[b], T[b] = i, 0, max(LENS[j] for j in take)
        queue = queue[len(take):]
    return evictions


def body_scheduler(dev, golden_dir, graph):
    """`generate(schedule="continuous")`, all 24 requests on 4 rows over 5 pages: a host-side page count says the schedule must preempt;
    every request's codes equal the fixture's, `preemptions >= 1`, `peak_pages <= pool_pages`.  `generate_stream` on the same input: per
    request the packets from its last `restart` on concatenate to the fixture, and what a restarted request had delivered before is a
    prefix of it."""
    g, t, w, args = rg._fixture(golden_dir)
    assert _host_schedule_preempts(list(gga.LIMITS), TIGHT) >= 1
    eng = _engine(t, w, dev, torch.float32, graph, kv_pages=TIGHT)
    kw = rp._continuous_kw(t)
    out = eng.generate(*args, schedule="continuous", **kw)
    st = dict(eng.last_refill)
    print(f"pool {TIGHT}: {st}")
    rp._check_all(g, t, out)
    assert st["preemptions"] >= 1 and st["pool_pages"] == TIGHT and 4 <= st["peak_pages"] <= TIGHT, st
    assert st["graph_captures"] <= (1 if graph else 0), st
    parts, earlier, restarts, last = {i: [] for i in range(gga.N_REQ)}, {i: [] for i in range(gga.N_REQ)}, 0, set()
    for packet in eng.generate_stream(*args, schedule="continuous", **kw):
        for e in packet.rows:
            assert e.request not in last and (not e.restart or e.first)
            if e.restart:
                restarts += 1
                if parts[e.request]:
                    earlier[e.request].append(np.concatenate(parts[e.request]))
                parts[e.request] = []
            parts[e.request].append(_np(e.codes))
            if e.last:
                last.add(e.request)
    assert 1 <= restarts <= eng.last_refill["preemptions"] and last == set(range(gga.N_REQ))
    for i, L in enumerate(gga.LIMITS):
        cat = np.concatenate(parts[i])
        rg._check_request(g, t, cat, i, L)
        for old in earlier[i]:
            assert np.array_equal(old, cat[:old.shape[0]]), i


@pytest.mark.parametrize("graph", [False, True])
def test_the_continuous_schedule_preempts_by_restart_under_a_tight_pool(dev, golden_dir, graph):
    body_scheduler(dev, golden_dir, graph)


# ============================================================================================ 8. audio
def _tts_pooled(dev, kv_pages, max_seq):
    """`test_stream_slots_gpu._tts` (tiny talker of 2 rows + tiny codec of 2 slots, a deterministic stand-in tokenizer) on a pooled talker"""
    import synth
    import test_stream_slots_gpu as ss
    from test_gpu_parity import _td
    from qwen3_tts_amd.codec import Qwen3TTSTokenizer
    from qwen3_tts_amd.model import Qwen3TTSForConditionalGeneration
    tts, c = ss._tts(dev, 2)
    t = synth.talker_tiny()
    cfgd = dict(synth.cfg_dict(t), tts_model_type="custom_voice", tts_model_size="1b7", tokenizer_type="12hz")
    model = Qwen3TTSForConditionalGeneration(cfgd, _td(synth.talker_weights(t)), device=dev, dtype=torch.float32, max_batch=2, max_seq=max_seq,
                                             kv_pages=kv_pages)
    model.load_speech_tokenizer(tts.model.speech_tokenizer)
    return type(tts)(model, tts.processor, generate_defaults={}), c


def body_audio(dev):
    """`stream_custom_voice(schedule="continuous")` on a pooled model: 6 texts (prompts of 10 rows, limits 20..36: a row grows by two
    pages) on 2 rows over 4 pages of max_seq 64 -- the host-side count says the schedule preempts, and it does.  Per request the streamed
    PCM has exactly the sample count of the one-shot audio (no sample is delivered twice, none is missing) and is within 1e-5 RMS of it,
    the bar of tests/test_stream_slots_gpu.py for the same comparison."""
    from test_gpu_parity import _rms
    limits = [20, 30, 24, 28, 36, 26]
    assert _host_schedule_preempts(limits, 4, rows=2, packet=3, lens=[10] * 6, max_seq=64) >= 1
    tts, c = _tts_pooled(dev, 4, 64)
    texts = ["hello world", "a rather longer sentence to speak", "hi", "one more request in the queue", "and another", "the sixth text"]
    spk, langs = ["vivian", "ryan"] * 3, ["english", "chinese"] * 3
    kw = dict(language=langs, non_streaming_mode=False, max_new_tokens=limits, seed=[500 + i for i in range(6)])
    whole, sr = tts.generate_custom_voice(texts, spk, schedule="continuous", **kw)
    up = c.total_upsample
    got = [[] for _ in texts]
    for packet, sr2 in tts.stream_custom_voice(texts, spk, packet_frames=3, schedule="continuous", **kw):
        assert sr2 == sr and len(packet) == len(texts)
        for i, p in enumerate(packet):
            if p.shape[0]:
                got[i].append(p)
    st = tts.model.talker.last_refill
    print(f"pooled wrapper: {st}")
    assert st["preemptions"] >= 1 and st["peak_pages"] <= st["pool_pages"] == 4, st
    for i in range(len(texts)):
        cat = np.concatenate(got[i])
        d = _rms(cat, whole[i]) if cat.shape == whole[i].shape else float("nan")
        print(f"request {i}: {cat.shape[0] // up} frames, rms against the one-shot audio {d:.2e}")
        assert cat.shape == whole[i].shape and whole[i].shape[0] >= up and d <= 1e-5, (i, cat.shape, whole[i].shape, d)


def test_streamed_audio_survives_a_restart_without_a_repeated_sample(dev):
    body_audio(dev)


# ============================================================================================ 9. scalar paths and refusals
def body_scalar_and_refusals(dev, golden_dir):
    """`generate` (waves, scalar settings) on a pooled tiny engine gives the codes of tests/golden/talker_tiny.npz and, bit for bit, the
    static engine's hidden states.  Refused, with the engine left usable: a call whose worst case exceeds the pool (QTTS_ERR_LIMIT),
    `set_kv_pool` after finalize (QTTS_ERR_STATE), a pool smaller than one request of max_seq keys (QTTS_ERR_LIMIT), `stream_kv` on an
    engine without a pool (QTTS_ERR_STATE), `stream_evict` of a row listed twice or out of range (QTTS_ERR_ARG); the ABI version is
    still 15 and every new symbol is declared in the header and bound."""
    import ctypes as C
    from test_gpu_parity import _compare_greedy
    from test_row_sampling_gpu import _tiny
    t, w = _tiny()
    g = np.load(os.path.join(golden_dir, "talker_tiny.npz"))
    args = [torch.from_numpy(g[k]) for k in ("embeds", "mask", "trailing", "tts_pad")]
    B, T = args[0].shape[:2]
    kw = dict(min_new_tokens=2, do_sample=False, subtalker_dosample=False, repetition_penalty=1.05, suppress_tokens=_suppress(t))
    ref = _engine(t, w, dev, torch.float32, True, 4, 128).generate(*args, max_new_tokens=14, **kw)
    need = B * _pages(T + 14)
    eng = _engine(t, w, dev, torch.float32, True, 4, 128, kv_pages=max(8, need))
    assert eng.kv_page_bytes == t.num_hidden_layers * 2 * t.num_key_value_heads * 16 * t.head_dim * 4
    out = eng.generate(*args, max_new_tokens=14, **kw)
    n = g["codes"].shape[1]
    assert _compare_greedy(_np(out.codes), _np(out.tokens), g["codes"], g["tokens"], g["margin"]) == n
    assert np.array_equal(_np(out.codes), _np(ref.codes)) and np.array_equal(_np(out.hidden), _np(ref.hidden))
    assert eng.stream_kv() == ([_pages(T + 14)] * B, eng.kv_pages - need, eng.kv_pages)
    # a call whose worst case exceeds the pool: 8 pages hold one request of 128 keys, not B requests of T + 100
    small = _engine(t, w, dev, torch.float32, True, 4, 128, kv_pages=8)
    assert B * _pages(T + 100) > 8 >= B * _pages(T)
    with pytest.raises(_qlib.QttsError, match=r"worst case") as ei:
        small.generate(*args, max_new_tokens=100, **kw)
    assert ei.value.code == QTTS_ERR_LIMIT
    one = [a[:1] for a in args[:3]] + [args[3]]
    again = small.generate(*one, max_new_tokens=14, **kw)          # the engine is usable: one request fits
    assert _np(again.codes).shape[1] >= 1
    lib, h = small._lib, small._h
    assert lib.qtts_talker_set_kv_pool(h, 16) == QTTS_ERR_STATE
    with pytest.raises(_qlib.QttsError, match="do not hold one request") as ei:
        _engine(t, w, dev, torch.float32, True, 4, 128, kv_pages=7)
    assert ei.value.code == QTTS_ERR_LIMIT
    static = _engine(t, w, dev, torch.float32, True, 4, MAX_SEQ)
    with pytest.raises(_qlib.QttsError, match="no KV page pool") as ei:
        static.stream_kv()
    assert ei.value.code == QTTS_ERR_STATE
    # stream_evict: bad row lists change nothing; on a static engine it cancels a request and frees nothing
    g2, t2, w2, args2 = rg._fixture(golden_dir)
    limits = {11: 13, 1: 13, 4: 13, 6: 13}
    for e in (static, _engine(t2, w2, dev, torch.float32, True, kv_pages=8)):
        s = rp.RowStream(e, t2, args2, [11, 1, 4, 6], rg._greedy_settings(limits))
        s.step(1)
        before = (s.rows(), s.check_lens())
        for bad in ([1, 1], [4], [-1]):
            with pytest.raises(_qlib.QttsError) as ei:
                e.stream_evict(bad)
            assert ei.value.code == QTTS_ERR_ARG
        assert (s.rows(), s.check_lens()) == before
        e.stream_evict([2])
        assert s.rows()[0] == [1, 1, 0, 1] and e.stream_row_lens() == before[1]
        if e.kv_pages:
            assert e.stream_kv() == ([1, 1, 0, 1], 5, 8)
        s.slot[2] = None
        s.finish()
        for r in (11, 1, 6):
            rg._check_request(g2, t2, s.out[r], r, 13)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "qtts.h")).read()
    for sym in ("qtts_talker_set_kv_pool", "qtts_talker_stream_kv", "qtts_talker_stream_evict"):
        assert sym in _qlib.SYMBOLS and f"int {sym}(" in hdr and getattr(lib, sym).restype is C.c_int
    assert _qlib.ABI_VERSION == 15 == lib.qtts_abi_version()


def test_scalar_paths_reserve_their_worst_case_and_bad_calls_are_refused(dev, golden_dir):
    body_scalar_and_refusals(dev, golden_dir)
