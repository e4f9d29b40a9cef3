"""Per-row KV positions (include/qtts.h: qtts_talker_stream_begin_admitting_rows, qtts_talker_stream_row_lens;
`TalkerEngine.stream_open(..., row_positions=True)`, `generate(..., schedule="continuous")`): every row of an admitting stream carries its
own KV length.  An admitted prompt goes to slots [0, T) of its row, the row's length restarts at T and grows by one per frame while the
occupant runs; a finished row's length is frozen.  The stream never drains and a row's attention walks its own keys only.

As in tests/test_refill_gpu.py every request's result is pinned to what the REFERENCE produced for it (tests/golden/talker_tiny_admit.npz:
24 ragged requests, prompts of 3..15 rows, limits 3..13, greedy with penalty 1.05, two trailing rows, every cb-0 margin >= 1e-3: no
comparison stops early).  The geometry is the smallest that crosses everything: 4 rows, max_seq 32 = two 16-key pages per row; a 15-row
prompt crosses the page inside its generation; 15 + 13 = 28 <= 32, so no request is ever refused by the schedule.

A row's expected length is counted here from the limits alone: admitted at T under the limit L it samples token 0 at admission and one
token per step; the step that samples token L - 1 finishes it and does not advance it, so after k steps of its own its length is
T + min(k, L - 2) -- and stays there while it idles.

The test BODIES (`body_*`) take the device; tests/test_row_positions_hostemu.py runs the same bodies on the host-emulation build."""
import numpy as np
import pytest
import torch

import synth
from qwen3_tts_amd import _lib as _qlib
from test_gpu_parity import _rms, _suppress, _td, dev  # noqa: F401  (`dev` is a fixture)
from test_row_sampling_gpu import TOL, _gap, _np
import test_refill_gpu as rg

pytestmark = pytest.mark.gpu
gga, LENS = rg.gga, rg.LENS
QTTS_ERR_LIMIT = -6
MAX_SEQ = 32


class RowStream(rg.Stream):
    """`test_refill_gpu.Stream` on a stream with per-row positions (or, `row_positions=False`, the shared-position stream through the
    same calls), which also keeps the host's own count of every row's length.  `Tg`: the padded length of a group, at least its longest
    prompt (more: every member is left-padded further -- how a test reaches lengths the fixture's prompts do not have)."""

    def __init__(self, eng, t, args, first, settings, max_row=gga.MAX_NEW, hidden=False, row_positions=True, Tg=None):
        self.eng, self.t, self.args, self.settings = eng, t, args, settings
        self.emb, self.mask, self.trail, self.pad = args
        self.T = self.emb.shape[1]
        self.out, self.out_hidden = {}, {}
        e, npd, tr, tab = self._group(first, Tg)
        self.codes, self.hidden = eng.stream_open(e, npd, tr, self.pad, tab, max_row, t.codec_eos_token_id, _suppress(t), hidden, row_positions)
        self.slot, self.max_row = list(first), max_row
        self.base = [int(e.shape[1])] * len(first)       # the length each row's occupant started at ...
        self.age = [0] * len(first)                      # ... the stream steps since then ...
        self.limit = [settings[r]["max_new_tokens"] for r in first]      # ... and its limit
        self.total = 0

    def _group(self, reqs, Tg=None):
        Tg = Tg or max(LENS[i] for i in reqs)
        e = self.emb[reqs]
        e = e[:, self.T - Tg:] if Tg <= self.T else torch.cat([torch.zeros(len(reqs), Tg - self.T, e.shape[2], dtype=e.dtype), e], 1)
        return e, [Tg - LENS[i] for i in reqs], self.trail[reqs], rg._table([self.settings[i] for i in reqs])

    def step(self, n):
        total, fin = self.eng.stream_step(n)
        self.age = [a + total - self.total for a in self.age]          # (launches behind the stop latch run nothing)
        self.total = total
        return total, fin

    def admit(self, pairs, Tg=None):
        rows_, reqs = [p[0] for p in pairs], [p[1] for p in pairs]
        e, npd, tr, tab = self._group(reqs, Tg)
        self.eng.stream_admit(rows_, e, npd, tr, tab)
        for b, r in pairs:
            self.slot[b], self.base[b], self.age[b], self.limit[b] = r, int(e.shape[1]), 0, self.settings[r]["max_new_tokens"]

    def expected_lens(self):
        return [T + min(k, L - 2) for T, k, L in zip(self.base, self.age, self.limit)]

    def check_lens(self):
        got = self.eng.stream_row_lens()
        assert got == self.expected_lens(), (got, self.expected_lens(), self.slot, self.age)
        return got


def _continuous_kw(t):
    return dict(max_new_tokens=gga.LIMITS, min_new_tokens=gga.MAX_NEW, do_sample=False, subtalker_dosample=False, repetition_penalty=gga.REP,
                suppress_tokens=_suppress(t), packet_frames=2)


def _check_all(g, t, out):
    """every request of a `generate` result against the reference: all 16 codebooks of every frame, eos behind the last"""
    codes, compared = _np(out.codes), 0
    for i, L in enumerate(gga.LIMITS):
        compared += rg._check_request(g, t, codes[i, :L - 1], i, L)
        assert (codes[i, L - 1:, 0] == t.codec_eos_token_id).all(), i
        assert np.array_equal(_np(out.tokens)[i, :L - 1], g["tokens"][i, :L - 1])
    assert compared == sum(L - 1 for L in gga.LIMITS) == 163


# ============================================================================================ 1. / 5. one stream, recycled positions
def body_continuous_reference(dev, golden_dir, graph, gq=False):
    """fp32, 4 rows, max_seq 32, the 24 requests through `generate(schedule="continuous", packet_frames=2)`: every request's codes equal
    the fixture's on all 16 codebooks, every frame; ONE stream; it runs more frame steps than max_seq has positions (163 frames on 4 rows
    need at least 41), so positions were re-used; no row ever grew beyond 28; at most one frame graph.  At the same max_seq the
    shared-position schedule begins several streams.  `gq`: the same under QTTS_ATTN_GQ=1 -- attn_gqv_kernel serves the default shape."""
    g, t, w, args = rg._fixture(golden_dir)
    with _qlib.options(**({"QTTS_ATTN_GQ": "1"} if gq else {})):
        eng = rg._engine(t, w, dev, torch.float32, graph, 4, MAX_SEQ)
    out = eng.generate(*args, schedule="continuous", **_continuous_kw(t))
    st, stats = eng.last_refill, eng.stats()
    _check_all(g, t, out)
    assert st["streams"] == 1 and st["admitted_rows"] == gga.N_REQ - 4, st
    assert st["frames_run"] > MAX_SEQ, st
    assert 15 <= st["max_row_len"] <= 28, st
    assert st["graph_captures"] <= (1 if graph else 0), st
    assert stats["row_positions"] == 1 and stats["row_table_last"] == 1
    assert (stats["attn_gq_per_step"] > 0) == gq, stats
    if not gq:
        ref = eng.generate(*args, schedule="refill", **_continuous_kw(t))
        _check_all(g, t, ref)
        assert eng.last_refill["streams"] >= 2 and eng.stats()["row_positions"] == 0, eng.last_refill
        print(f"max_seq {MAX_SEQ}, graph {graph}: occupancy continuous {st['occupancy']:.3f} ({st['frames_run']} steps, 1 stream), "
              f"refill {eng.last_refill['occupancy']:.3f} ({eng.last_refill['frames_run']} steps, {eng.last_refill['streams']} streams)")


@pytest.mark.parametrize("graph", [False, True])
def test_one_stream_serves_every_request_on_recycled_positions(dev, golden_dir, graph):
    body_continuous_reference(dev, golden_dir, graph)


@pytest.mark.parametrize("graph", [False, True])
def test_the_general_attention_family_reads_per_row_lengths(dev, golden_dir, graph):
    body_continuous_reference(dev, golden_dir, graph, gq=True)


def body_clamped_limits(dev, golden_dir, graph):
    """Eight requests with eight different prompt lengths ask for 8192 tokens each at max_seq 32: every limit is clamped to the room its
    own prompt leaves (17..29), so each fits only behind its own length and the widest opening group has ONE member.  The stream still
    runs at full width -- the other three rows open as spare rows and the first admission fills them -- as one stream; the 12 frames
    the fixture has of every request (EOS blocked that long) equal it, and no row passes max_seq - 2."""
    import warnings
    g, t, w, args = rg._fixture(golden_dir)
    reqs = [11, 9, 7, 5, 3, 1, 0, 2]
    assert len({LENS[i] for i in reqs}) == len(reqs)
    sub = [a[reqs] for a in args[:3]] + [args[3]]
    eng = rg._engine(t, w, dev, torch.float32, graph, 4, MAX_SEQ)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = eng.generate(*sub, schedule="continuous", **dict(_continuous_kw(t), max_new_tokens=8192))
    st, codes = eng.last_refill, _np(out.codes)
    assert st["streams"] == 1 and st["admitted_rows"] == len(reqs) - 1 and eng._live_batch == 4, st
    assert st["max_row_len"] == MAX_SEQ - 2 and st["occupancy"] > 0.5, st
    for k, r in enumerate(reqs):
        assert np.array_equal(codes[k, :gga.MAX_NEW - 1], g["codes"][r]), r


@pytest.mark.parametrize("graph", [False, True])
def test_clamped_limits_still_open_a_full_width_stream(dev, golden_dir, graph):
    body_clamped_limits(dev, golden_dir, graph)


# ============================================================================================ 2. a long prompt into a young stream
def body_long_prompt(dev, golden_dir, graph):
    """The four shortest prompts open the stream (3, 3, 4, 4 rows); after the first retirement (2 steps: position 6) the 15-row prompt
    asks for the row.  The shared-position stream refuses exactly this with QTTS_ERR_LIMIT; with per-row positions it is accepted, its
    codes and its three neighbours' are the fixture's, and `stream_row_lens` equals the host's count after every step."""
    g, t, w, args = rg._fixture(golden_dir)
    limits = {0: 3, 13: 8, 2: 13, 15: 7, 11: 13}
    settings = rg._greedy_settings(limits)
    eng = rg._engine(t, w, dev, torch.float32, graph, 4, MAX_SEQ)
    s = RowStream(eng, t, args, [0, 13, 2, 15], settings, row_positions=False)
    assert s.step(2) == (2, False) and s.retire() == [0] and s.rows()[2] == 6
    with pytest.raises(_qlib.QttsError, match="longer than the stream's position") as ei:
        s.admit([(0, 11)])
    assert ei.value.code == QTTS_ERR_LIMIT
    with pytest.raises(_qlib.QttsError, match="no stream with per-row positions"):
        eng.stream_row_lens()
    s.slot[0] = None
    s.finish()

    s = RowStream(eng, t, args, [0, 13, 2, 15], settings)
    assert s.check_lens() == [4, 4, 4, 4] and eng.stats()["row_positions"] == 1
    for k in (1, 2):
        assert s.step(1) == (k, False)
        s.check_lens()
    assert s.retire() == [0] and s.rows() == ([0, 1, 1, 1], [2, 2, 2, 2], 6)
    s.admit([(0, 11)])
    assert s.check_lens() == [15, 6, 6, 6] and s.rows() == ([1, 1, 1, 1], [0, 2, 2, 2], 15)
    fin, seen = False, []
    while not fin:
        _, fin = s.step(1)
        seen.append(s.check_lens())
    assert max(x[0] for x in seen) == 15 + 13 - 2 and seen[-1] == [26, 4 + 8 - 2, 4 + 13 - 2, 4 + 7 - 2]
    s.finish()
    assert sorted(s.out) == [0, 2, 11, 13, 15]
    for r, codes in s.out.items():
        rg._check_request(g, t, codes, r, limits[r])


@pytest.mark.parametrize("graph", [False, True])
def test_a_long_prompt_enters_a_young_stream(dev, golden_dir, graph):
    body_long_prompt(dev, golden_dir, graph)


# ============================================================================================ 3. edges
def body_edges(dev, golden_dir, dtype, graph=True):
    """One stream, 4 rows, max_seq 32, stepped one frame at a time with `stream_row_lens` checked against the host's count every step:
      * rows 0..2 stop after 2 steps and a ragged group of three (12, 7 and 11 prompt rows: local pads 0, 5, 1) is admitted at once --
        each second occupant LONGER than the first;
      * request 11 (15 rows) is padded to T = 19 with the limit 13: T + L == 32, its last key goes to slot 30 of 32;
      * the same group at T = 20 (T + L == 33) is refused with QTTS_ERR_LIMIT naming the row; `stream_rows` / `stream_row_lens` are
        unchanged and every neighbour's later codes are the fixture's;
      * row 0 retires early and idles for more than max_seq steps while the others cycle through requests; its length stays frozen;
        then request 13 (3 rows) is admitted into it: SHORTER than both earlier occupants, stale keys above its length;
    every request's codes equal the fixture's (bf16: the project's bf16 bound, `test_refill_gpu._judge`)."""
    g, t, w, args = rg._fixture(golden_dir)
    limits = {0: 3, 2: 3, 14: 3, 9: 11, 5: 4, 8: 9, 3: 6, 11: 13, 12: 8, 1: 13, 4: 12, 6: 11, 13: 13, 15: 12, 17: 11, 19: 10, 21: 9}
    settings = rg._greedy_settings(limits)
    eng = rg._engine(t, w, dev, dtype, graph, 4, MAX_SEQ)
    s = RowStream(eng, t, args, [0, 2, 14, 9], settings)
    steps = peak = 0

    def run(n):
        nonlocal steps, peak
        for _ in range(n):
            steps += 1
            assert s.step(1) == (steps, False)
            peak = max(peak, max(s.check_lens()))
    run(2)
    assert s.retire() == [0, 1, 2]
    s.admit([(0, 5), (1, 8), (2, 3)])                          # T = 12: local pads 0, 5, 1
    assert s.check_lens() == [12, 12, 12, 14 + 2]
    run(3)                                                     # request 5 (limit 4) is done
    assert s.retire() == [0]
    frozen = s.check_lens()[0]
    assert frozen == 12 + 4 - 2
    idle_from = steps
    run(2)                                                     # request 3 (limit 6) is done
    assert s.retire() == [0, 2]
    before = (s.rows(), s.check_lens())
    with pytest.raises(_qlib.QttsError, match=r"row 2: the group's padded length T \(20\) \+ max_new_tokens \(13\) exceeds max_seq") as ei:
        s.admit([(2, 11)], Tg=20)                              # T + L == 33
    assert ei.value.code == QTTS_ERR_LIMIT and eng.stats()["admit_calls"] == 1
    assert (s.rows(), s.check_lens()) == before
    s.admit([(2, 11)], Tg=19)                                  # T + L == 32
    assert s.check_lens()[2] == 19
    queue = [1, 4, 6, 12, 15, 17, 19, 21]                      # rows 1..3 cycle through these; row 0 idles
    while steps - idle_from <= MAX_SEQ + 1:
        run(1)
        free = [b for b in s.retire() if b != 0]
        if free and queue:
            take = queue[:len(free)]
            queue = queue[len(take):]
            s.admit(list(zip(free, take)))
        assert s.check_lens()[0] == frozen
    assert steps - idle_from > MAX_SEQ and s.slot[0] is None
    assert peak == 19 + 13 - 2 == MAX_SEQ - 2                 # request 11 wrote its last key to slot 30: inside the row's second page
    s.admit([(0, 13)])                                         # 3 rows into the row that held 12 and, before that, 3 rows
    assert s.check_lens()[0] == 3
    fin = False
    while not fin:
        _, fin = s.step(1)
        s.check_lens()
    s.finish()
    assert sorted(s.out) == sorted(limits) and not queue
    rg._judge(g, t, dtype, s.out, limits)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_row_position_edges_at_the_abi(dev, golden_dir, dtype):
    body_edges(dev, golden_dir, dtype)


# ============================================================================================ 4. split-KV, rows of very different lengths
def body_split_kv(dev, golden_dir, dtype):
    """Split-KV from 20 keys on, two workgroups per (row, kv head); max_seq 192 spans the buckets 128 and 256.  The four shortest
    prompts open the stream left-padded to T = 40: span 128.  Request 7 is admitted left-padded to T = 150: the span rises to 256,
    where the short rows (<= 46 keys) have no valid key in the second split and the long row (keys 137..) none in the first -- the
    merge must give each exactly its non-empty split.  When the long row retires the span falls to 128 again, its frozen 153 keys keep
    nothing alive, and request 10 (8 rows) takes the row: stale keys above its length; when it is the last one running, below 20 keys,
    the stream is back in the short mode.  Codes equal the fixture's; graphs captured <= distinct spans visited."""
    g, t, w, args = rg._fixture(golden_dir)
    limits = {0: 3, 7: 5, 13: 13, 2: 13, 15: 13, 10: 13}
    settings = rg._greedy_settings(limits)
    with _qlib.options(QTTS_ATTN_NSPLIT="2", QTTS_ATTN_SPLIT_FROM="20", QTTS_ATTN_SPLIT_KEYS="64"):
        eng = rg._engine(t, w, dev, dtype, True, 4, 192)
    caps0 = eng.stats()["graph_captures"]
    s = RowStream(eng, t, args, [0, 13, 2, 15], settings, Tg=40)
    spans = []

    def run(n):
        for _ in range(n):
            s.step(1)
            s.check_lens()
            spans.append(eng.stats()["attn_span_last"])
    run(2)
    assert spans == [128, 128] and s.retire() == [0]
    s.admit([(0, 7)], Tg=150)                                  # 13 prompt rows at slots 137..149
    assert s.check_lens() == [150, 42, 42, 42] and s.rows()[2] == 150
    run(4)                                                     # its 5 tokens: done after 4 steps
    assert spans[2:] == [256] * 4 and eng.stats()["attn_nsplit_last"] == 2
    assert s.retire() == [0] and s.check_lens() == [150 + 5 - 2, 46, 46, 46]
    run(1)
    assert spans[-1] == 128                                    # the long row is frozen at 153 keys and keeps no bucket alive
    s.admit([(0, 10)])                                         # 8 rows: shorter than the first occupant's 150, stale keys above
    fin = False
    while not fin:
        _, fin = s.step(1)
        s.check_lens()
        spans.append(eng.stats()["attn_span_last"])
    # the 40-row prompts run until step 12 (span 128); request 10 then runs on alone with fewer than 20 keys: the short mode
    assert spans[7:] == [128] * 5 + [0] * 7, spans
    s.finish()
    st = eng.stats()
    assert st["graph_captures"] - caps0 <= len(set(spans)) == 3 and st["long_graphs"] == 2, (st, spans)
    assert sorted(s.out) == sorted(limits)
    rg._judge(g, t, dtype, s.out, limits)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_split_kv_with_rows_of_very_different_lengths(dev, golden_dir, dtype):
    body_split_kv(dev, golden_dir, dtype)


# ============================================================================================ 6. bf16
def body_bf16(dev, golden_dir, gq=False):
    """The 24 requests, bf16, graph (attn_tk16_kernel on transposed V pages; attn_gq16_kernel under QTTS_ATTN_GQ=1), judged by the
    measure and bound of `test_refill_gpu._judge`; two runs are bit-identical."""
    g, t, w, args = rg._fixture(golden_dir)
    with _qlib.options(**({"QTTS_ATTN_GQ": "1"} if gq else {})):
        eng = rg._engine(t, w, dev, torch.bfloat16, True, 4, MAX_SEQ)
    a = eng.generate(*args, schedule="continuous", **_continuous_kw(t))
    st = dict(eng.last_refill)
    b = eng.generate(*args, schedule="continuous", **_continuous_kw(t))
    assert st["streams"] == 1 and st["frames_run"] > MAX_SEQ and st["max_row_len"] <= 28 and (eng.stats()["attn_gq_per_step"] > 0) == gq, st
    assert np.array_equal(_np(a.codes), _np(b.codes)) and np.array_equal(_np(a.hidden), _np(b.hidden))
    codes = _np(a.codes)
    rg._judge(g, t, torch.bfloat16, {i: codes[i, :L - 1] for i, L in enumerate(gga.LIMITS)}, dict(enumerate(gga.LIMITS)))


@pytest.mark.parametrize("gq", [False, True])
def test_bf16_continuous_stream(dev, golden_dir, gq):
    body_bf16(dev, golden_dir, gq)


# ============================================================================================ 7. sampled rows
def body_sampling(dev, golden_dir, dtype, graph):
    """Mixed per-request settings and seeds on a stream with per-row positions.  Requests 5 and 8 enter rows 1 and 2 at stream step 2;
    after 3 steps of its own every sub-code draw of request 5's last frame and its last talker draw lie in the row's inverse-CDF
    interval for u = Philox(seed; OWN step 3, 0, codebook) within TOL -- with the stream's counter (5) they miss by more than 1e-3; row 0,
    which began with the stream, passes with the stream's counter.  Then the same group enters the OTHER rows two steps later: both
    requests draw exactly the same codes."""
    _, t, w, args = rg._fixture(golden_dir)
    sup = _suppress(t)
    knobs = lambda i: dict(do_sample=1, top_k=[50, 20, 64][i % 3], top_p=1.0, temperature=[0.9, 1.3, 0.7][i % 3], repetition_penalty=[1.05, 1.5][i % 2],
                           subtalker_dosample=1, subtalker_top_k=[50, 5, 64][i % 3], subtalker_top_p=1.0, subtalker_temperature=[0.9, 0.6, 1.3][i % 3],
                           min_new_tokens=40, seed=4000 + 13 * i, max_new_tokens={0: 3, 2: 3}.get(i, 11))
    settings = [knobs(i) for i in range(gga.N_REQ)]
    eng = rg._engine(t, w, dev, dtype, graph, 4, MAX_SEQ)
    s = RowStream(eng, t, args, [1, 0, 2, 7], settings)
    s.step(2)
    assert s.retire() == [1, 2]
    s.admit([(1, 5), (2, 8)])
    assert s.step(3) == (5, False)
    assert s.check_lens() == [13 + 5, 12 + 3, 12 + 3, 13 + 5]
    raw, cp_raw = eng.debug_logits()[:4].cpu(), eng.debug_cp_logits()[:, :4].cpu()
    codes = _np(s.codes)
    tok = torch.full((4, gga.MAX_NEW), -7, dtype=torch.int64, device=s.codes.device)
    eng.stream_close(tok)
    tok = _np(tok)
    empty = torch.zeros(0, dtype=torch.long)

    def gaps(b, req, frame, step):
        st, worst = settings[req], -1.0
        for j in range(t.num_code_groups - 1):
            worst = max(worst, _gap(cp_raw[j, b], empty, int(codes[b, frame, 1 + j]), step, 1 + j, st, True, t, sup, 0))
        hist = torch.from_numpy(tok[b, :frame + 1])
        return max(worst, _gap(raw[b], hist, int(tok[b, frame + 1]), step, 0, st, False, t, sup, 40))
    own, stream_ctr, neighbour = gaps(1, 5, 2, 3), gaps(1, 5, 2, 5), gaps(3, 7, 4, 5)
    print(f"admitted row, draws of its last frame: worst gap {own:.2e} with its own step, {stream_ctr:.2e} with the stream's; row 3: {neighbour:.2e}")
    assert own <= TOL and neighbour <= TOL, (own, neighbour)
    assert stream_ctr > 1e-3, stream_ctr

    def placed(rows_, after):
        s = RowStream(eng, t, args, [1, 0, 2, 7] if after == 2 else [0, 1, 4, 2], settings)
        s.step(after)
        assert sorted(s.retire()) == sorted(rows_)
        s.admit(list(zip(rows_, (5, 8))))
        s.finish()
        return s.out
    a, b = placed([1, 2], 2), placed([3, 0], 4)          # rows 1, 2 at step 2; rows 3, 0 at step 4 (requests 0, 2 stop at 2; 1, 4 run beside)
    for r in (5, 8):
        assert a[r].shape == (10, t.num_code_groups) and np.array_equal(a[r], b[r]), r


@pytest.mark.parametrize("dtype,graph", [(torch.bfloat16, True), (torch.float32, False)])
def test_sampled_rows_draw_with_their_own_step_wherever_they_are_admitted(dev, golden_dir, dtype, graph):
    body_sampling(dev, golden_dir, dtype, graph)


# ============================================================================================ 8. streaming and wrapper
def body_stream_packets(dev, golden_dir, graph):
    """`generate_stream(schedule="continuous")`: each request's packets concatenate to the reference's codes and to what
    `generate(schedule="continuous")` returns; every request is flagged `first` once and `last` once; no row has two occupants."""
    g, t, w, args = rg._fixture(golden_dir)
    eng = rg._engine(t, w, dev, torch.float32, graph, 4, MAX_SEQ)
    kw = dict(_continuous_kw(t), packet_frames=3)
    parts, first, last, occupant = {i: [] for i in range(gga.N_REQ)}, {}, {}, {}
    for n, packet in enumerate(eng.generate_stream(*args, schedule="continuous", **kw)):
        for e in packet.rows:
            assert e.codes.shape[0] <= 3 and e.request not in last and (e.request not in first) == e.first, e.request
            if e.first:
                first[e.request] = n
                assert occupant.get(e.row) is None, (e.row, e.request)
                occupant[e.row] = e.request
            assert occupant[e.row] == e.request
            parts[e.request].append(_np(e.codes))
            if e.last:
                last[e.request], occupant[e.row] = n, None
    assert sorted(first) == sorted(last) == list(range(gga.N_REQ)) and eng.last_refill["streams"] == 1
    whole = _np(eng.generate(*args, schedule="continuous", **kw).codes)
    for i, L in enumerate(gga.LIMITS):
        cat = np.concatenate(parts[i])
        rg._check_request(g, t, cat, i, L)
        assert np.array_equal(cat, whole[i, :L - 1]), i
    with pytest.raises(ValueError, match="schedule"):
        eng.generate(*args, schedule="eager", **kw)


@pytest.mark.parametrize("graph", [False, True])
def test_continuous_stream_packets_concatenate_to_the_reference_codes(dev, golden_dir, graph):
    body_stream_packets(dev, golden_dir, graph)


def body_wrapper(dev):
    """`stream_custom_voice(schedule="continuous")`: 6 texts on a talker of 2 rows, sampling with a seed per request: per request the
    streamed audio has the sample count of `generate_custom_voice(schedule="continuous")` and is within 1e-5 RMS of it (the bar of
    tests/test_stream_slots_gpu.py for the refill wrapper); the one-shot audio of the continuous schedule has the sample count of the
    refill schedule's for the same seeds and is within the same bar of it (fp32: a request's codes do not depend on the schedule)."""
    import test_stream_slots_gpu as ss
    tts, c = ss._tts(dev, 2)
    texts = ["hello world", "a rather longer sentence to speak", "hi", "one more request in the queue", "and another", "the sixth text"]
    spk, langs = ["vivian", "ryan"] * 3, ["english", "chinese"] * 3
    kw = dict(language=langs, non_streaming_mode=False, max_new_tokens=[6, 11, 4, 9, 13, 7], seed=[500 + i for i in range(6)])
    whole, sr = tts.generate_custom_voice(texts, spk, schedule="continuous", **kw)
    assert tts.model.talker.last_refill["streams"] == 1 and tts.model.talker.stats()["row_positions"] == 1
    refill, _ = tts.generate_custom_voice(texts, spk, schedule="refill", **kw)
    assert tts.model.talker.stats()["row_positions"] == 0
    for i in range(len(texts)):
        assert refill[i].shape == whole[i].shape and _rms(whole[i], refill[i]) <= 1e-5, (i, refill[i].shape, whole[i].shape)
    up = c.total_upsample
    got = [[] for _ in texts]
    for packet, sr2 in tts.stream_custom_voice(texts, spk, packet_frames=3, schedule="continuous", **kw):
        assert sr2 == sr and len(packet) == len(texts)
        for i, p in enumerate(packet):
            if p.shape[0]:
                got[i].append(p)
    assert tts.model.talker.last_refill["streams"] == 1 and tts.model.talker.last_refill["admitted_rows"] == 4
    for i in range(len(texts)):
        cat = np.concatenate(got[i])
        d = _rms(cat, whole[i]) if cat.shape == whole[i].shape else float("nan")
        print(f"request {i}: {cat.shape[0] // up} frames, rms against the one-shot audio {d:.2e}")
        assert cat.shape == whole[i].shape and whole[i].shape[0] >= up and d <= 1e-5, (i, cat.shape, whole[i].shape, d)


def test_stream_custom_voice_takes_the_continuous_schedule(dev):
    body_wrapper(dev)
