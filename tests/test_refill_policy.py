"""CPU, no library: the scheduling policy of the refill schedules (`qwen3_tts_amd.refill.RefillPolicy`) driven the way
`TalkerEngine._refill_stream` drives it, against a counting stand-in for the engine.

The stand-in (`Stand`): a request is (prompt length, frames until it is finished), its limit frames + 1.  A row admitted in a group
padded to T that has run k frames is T + k long and holds ceil((T + k) / 16) pages -- the count `_host_schedule_preempts` of
tests/test_kv_pool_gpu.py uses.  On top of it, as include/qtts.h states for the pooled engine: a finished row's pages go back when a
`stream_step` / `stream_rows` observes it finished (so a spare row, finished from the start, holds its prompt's pages until the first
step), an evicted row's at once.  A shared-position stream stands at its opening length + the frame steps run.

Every expected value below is worked out by hand from the rules `TalkerEngine._refill_stream` documents."""
from qwen3_tts_amd.refill import RefillPolicy, Report, pages_of, widest_opener


class Stand:
    def __init__(self, frames, pool=0):
        self.frames, self.pool = frames, pool
        self.T, self.k, self.req, self.held, self.pos, self.steps = [], [], [], [], 0, 0

    def open(self, lens, first, spare):
        n, T = len(first) + spare, max(lens[i] for i in first)
        self.T, self.k, self.req, self.pos, self.steps = [T] * n, [0] * n, list(first) + [None] * spare, T, 0
        self.held = [pages_of(T) if self.pool else 0] * n

    def running(self, b):
        return self.req[b] is not None and self.k[b] < self.frames[self.req[b]]

    def kv(self):
        return list(self.held), self.pool - sum(self.held)

    def row_lens(self):
        return [T + k for T, k in zip(self.T, self.k)]

    def evict(self, b):
        assert self.running(b)
        self.req[b], self.held[b] = None, 0

    def step(self, n):
        run = [b for b in range(len(self.req)) if self.running(b)]
        assert run
        ran = min(n, max(self.frames[self.req[b]] - self.k[b] for b in run))
        self.pos, self.steps = self.pos + ran, self.steps + ran
        for b in range(len(self.req)):
            if b in run:
                self.k[b] = min(self.k[b] + n, self.frames[self.req[b]])
            if self.pool:
                self.held[b] = pages_of(self.T[b] + self.k[b]) if b in run else 0
        assert not self.pool or sum(self.held) <= self.pool, (self.held, self.pool)      # (the engine would refuse the step)

    def rows(self):
        for b in range(len(self.req)):
            if not self.running(b):
                self.held[b] = 0
        return [int(self.running(b)) for b in range(len(self.req))], list(self.k), self.pos

    def admit(self, lens, row_ids, reqs):
        Tg = max(lens[i] for i in reqs)
        for b, r in zip(row_ids, reqs):
            assert not self.running(b)
            self.T[b], self.k[b], self.req[b], self.held[b] = Tg, 0, r, pages_of(Tg) if self.pool else 0
        assert not self.pool or sum(self.held) <= self.pool, (self.held, self.pool)


def drive(reqs, max_batch, max_seq, packet, row_positions=False, kv_pages=None):
    """The loop of `TalkerEngine._refill_stream` on the stand-in.  Returns (policy, the log of its decisions)."""
    lens, frames = [r[0] for r in reqs], [r[1] for r in reqs]
    pol = RefillPolicy(lens, [f + 1 for f in frames], max_batch, max_seq, packet, row_positions, kv_pages)
    s, log = Stand(frames, kv_pages or 0), []
    while pol.queue:
        first, spare = pol.open_stream()
        s.open(lens, first, spare)
        log.append(("open", first, spare))
        while pol.active:
            while pol.pooled and (victim := pol.victim(*s.kv(), s.row_lens())) is not None:
                log.append(("evict", victim, s.req[victim]))
                s.evict(victim)
            s.step(packet)
            unfinished, k, kv_len = s.rows()
            log.append(("packet", [tuple(r) for r in pol.reports(unfinished, k)]))
            for row_ids, grp in pol.admissions(kv_len, s.kv()[1] if pol.tight else None):
                s.admit(lens, row_ids, grp)
                log.append(("admit", row_ids, grp))
        pol.stream_closed(dict(admit_calls=0, admitted_rows=0, max_row_len=0), s.steps)
    return pol, log


def only(log, kind):
    return [e[1:] for e in log if e[0] == kind]


def test_shared_position():
    """2 rows, max_seq 16, packets of 2.  Prompts 6 4 4 3 9, limits 8 3 5 4 4.  The queue is 4 0 1 2 3 (longest first).  Stream 1 opens at
    T = 9 with request 4 and the longest of the rest whose limit fits behind 9 (<= 7): request 1, not request 0.  After packet 1 the
    position is 11, request 1 is done (2 frames) and request 2 fits (11 + 5 = 16): row 1.  After packets 2 and 3 (positions 13, 15)
    neither request 0 (limit 8) nor request 3 (limit 4) fits, every row has finished: stream 2 opens at T = 6 with both."""
    pol, log = drive([(6, 7), (4, 2), (4, 4), (3, 3), (9, 3)], 2, 16, 2)
    assert only(log, "open") == [([4, 1], 0), ([0, 3], 0)]
    assert only(log, "admit") == [([1], [2])]
    assert only(log, "packet")[:3] == [([(4, 0, 0, 2, True, False, False), (1, 1, 0, 2, True, True, False)],),
                                       ([(4, 0, 2, 3, False, True, False), (2, 1, 0, 2, True, False, False)],),
                                       ([(2, 1, 2, 4, False, True, False)],)]
    assert only(log, "packet")[3:] == [([(0, 0, 0, 2, True, False, False), (3, 1, 0, 2, True, False, False)],),
                                       ([(0, 0, 2, 4, False, False, False), (3, 1, 2, 3, False, True, False)],),
                                       ([(0, 0, 4, 6, False, False, False)],), ([(0, 0, 6, 7, False, True, False)],)]
    st = pol.finish(0)
    assert st["streams"] == 2 and st["row_frames"] == 3 + 2 + 4 + 7 + 3 and st["frames_run"] == 6 + 7 and st["preemptions"] == 0
    assert st["occupancy"] == 19 / (13 * 2)


def test_shared_position_fit_test():
    """The two halves of the fit test on contrived positions: a prompt longer than the position waits, a limit that passes max_seq waits."""
    pol = RefillPolicy([9, 5, 5], [3, 3, 8], 1, 16, 2)
    assert pol.open_stream() == ([0], 0) and pol.queue == [1, 2]
    assert pol.reports([0], [2]) == [Report(0, 0, 0, 2, True, True, False)]
    assert pol.admissions(4) == [] and pol.queue == [1, 2]            # prompts of 5 > position 4
    assert pol.admissions(14) == [] and pol.queue == [1, 2]           # 14 + 3 > 16
    assert pol.admissions(9) == [([0], [1])] and pol.queue == [2] and pol.slot == [1]       # request 2: 9 + 8 > 16


def test_continuous():
    """4 rows, max_seq 16, packets of 2.  Prompts 5 5 3 2 1 1 with limits 11 11 13 14 15 15: every limit fits only behind its own prompt
    length, so the candidate groups are {0, 1} at T = 5, {2} at 3, {3} at 2 and {4, 5} at 1; the tie goes to the longer T.  The stream
    opens with 0 and 1 and two spare rows.  The first admission fills them in queue order, 2 then 3 -- as two calls, because padded to 3
    request 3 would end at 3 + 14 = 17.  Requests 0 and 1 finish with packet 5 (10 frames); 4 and 5 take their rows as one group."""
    lens, limits = [5, 5, 3, 2, 1, 1], [11, 11, 13, 14, 15, 15]
    assert widest_opener([0, 1, 2, 3, 4, 5], lens, limits, 16, 4) == [0, 1]
    pol, log = drive([(n, m - 1) for n, m in zip(lens, limits)], 4, 16, 2, row_positions=True)
    assert only(log, "open") == [([0, 1], 2)] and len(pol.slot) == 4
    assert only(log, "admit") == [([2], [2]), ([3], [3]), ([0, 1], [4, 5])]
    at = [i for i, e in enumerate(log) if e[0] == "admit"]
    assert [sum(e[0] == "packet" for e in log[:i]) for i in at] == [1, 1, 5]
    assert only(log, "packet")[0] == ([(0, 0, 0, 2, True, False, False), (1, 1, 0, 2, True, False, False)],)      # (no spare row reports)
    st = pol.finish(0)
    assert st["streams"] == 1 and st["row_frames"] == 10 + 10 + 12 + 13 + 14 + 14 and not pol.pooled and not pol.tight


TIGHT = [(14, 8), (14, 6), (14, 6), (14, 3), (14, 3)]


def test_pooled_tight_victim_watermark_and_restart():
    """3 rows, max_seq 48 (3 pages a row), 4 pages, packets of 4; five prompts of 14 (one page) with 8 6 6 3 3 frames.
    Open 0 1 2: three pages held, one free.  Packet 1 takes every row to 18 keys: 3 more pages needed.  Nobody has a frame, the tie
    goes to the highest request, 2 (row 2): queue 2 3 4.  The count is read again: 2 needed, 2 free.  After the packet 4 pages are held:
    no admission (1 prompt page + 3 rows then running > 0 free).  Packet 2 finishes 0 and 1; 4 pages free, nothing running: request 2
    (1 page), then 3 (2 prompt pages + 2 rows then running = 4), but not 4 (3 + 3 > 4).  Request 2's first packet is a restart, its
    second is not.  Request 3 finishes in packet 3; request 4 waits (1 + 2 > 2 free) until request 2 has finished."""
    pol, log = drive(TIGHT, 3, 48, 4, row_positions=True, kv_pages=4)
    assert pol.pooled and pol.tight
    assert only(log, "open") == [([0, 1, 2], 0)]
    assert only(log, "evict") == [(2, 2)]
    assert only(log, "admit") == [([0, 1], [2, 3]), ([0], [4])]
    assert only(log, "packet") == [([(0, 0, 0, 4, True, False, False), (1, 1, 0, 4, True, False, False)],),
                                   ([(0, 0, 4, 8, False, True, False), (1, 1, 4, 6, False, True, False)],),
                                   ([(2, 0, 0, 4, True, False, True), (3, 1, 0, 3, True, True, False)],),
                                   ([(2, 0, 4, 6, False, True, False)],),
                                   ([(4, 0, 0, 3, True, True, False)],)]
    st = pol.finish(0)
    assert st["preemptions"] == 1 and st["pool_pages"] == 4 and st["peak_pages"] == 4 and st["streams"] == 1


def test_pooled_victim_has_the_fewest_frames_and_returns_to_the_front():
    """3 rows, max_seq 48, 6 pages, packets of 4.  Prompts 11 12 12 12, frames 24 24 4 24: the queue is 1 2 3 0.  Request 2 finishes in
    packet 1; request 0 takes row 1 (1 page + 3 rows then running = 4 free) and stays 4 frames behind.  Before packet 6 rows 0 and 2
    stand at 32 keys and need a third page each while all 6 are held: the victim is request 0 -- 16 frames against 20, although it has
    the lowest index.  It is alone in the queue, is admitted again when 1 and 3 have finished, and starts over."""
    pol, log = drive([(11, 24), (12, 24), (12, 4), (12, 24)], 3, 48, 4, row_positions=True, kv_pages=6)
    assert only(log, "open") == [([1, 2, 3], 0)]
    assert only(log, "evict") == [(1, 0)]
    assert only(log, "admit") == [([1], [0]), ([0], [0])]
    packets = only(log, "packet")
    assert log.index(("evict", 1, 0)) == [i for i, e in enumerate(log) if e[0] == "packet"][4] + 1          # before packet 6
    assert packets[1] == ([(1, 0, 4, 8, False, False, False), (0, 1, 0, 4, True, False, False), (3, 2, 4, 8, False, False, False)],)
    assert packets[5] == ([(1, 0, 20, 24, False, True, False), (3, 2, 20, 24, False, True, False)],)
    assert packets[6] == ([(0, 0, 0, 4, True, False, True)],) and packets[7] == ([(0, 0, 4, 8, False, False, False)],)
    assert len(packets) == 6 + 6
    st = pol.finish(0)
    assert st["preemptions"] == 1 and st["peak_pages"] == 6 and st["row_frames"] == 24 * 3 + 4


def test_the_sole_running_row_is_never_evicted_and_the_victim_goes_to_the_front():
    """On contrived counts: two rows of 16 keys, one page each, nothing free, the next packet needs a page more for each.  The victim is
    request 1 (tie: the highest index) and goes in front of the two queued requests; asked again with one row running and still no
    page free, the policy names nobody."""
    pol = RefillPolicy([12] * 4, [30] * 4, 2, 48, 4, True, 3)
    assert pol.open_stream() == ([0, 1], 0) and pol.queue == [2, 3]
    assert len(pol.reports([1, 1], [4, 4])) == 2
    assert pol.victim([1, 1], 0, [16, 16]) == 1 and pol.queue == [1, 2, 3] and pol.slot == [0, None] and pol.stats["preemptions"] == 1
    assert pol.victim([1, 0], 0, [16, 16]) is None and pol.slot == [0, None] and pol.stats["preemptions"] == 1


def test_a_pool_of_the_static_size_admits_like_the_static_engine():
    """9 pages = 3 rows x ceil(48 / 16): not tight.  The decisions are those of the engine without a pool, nothing is evicted."""
    static, log0 = drive(TIGHT, 3, 48, 4, row_positions=True)
    pol, log = drive(TIGHT, 3, 48, 4, row_positions=True, kv_pages=9)
    assert pol.pooled and not pol.tight and log == log0 and not only(log, "evict")
    assert only(log, "admit") == [([0, 1], [3, 4])]                    # after packet 2, which finishes all three openers
    st = pol.finish(0)
    assert st["preemptions"] == 0 and st["pool_pages"] == 9 and 3 <= st["peak_pages"] <= 9
    assert {k: v for k, v in static.finish(0).items() if k not in ("pool_pages", "peak_pages")} == \
        {k: v for k, v in st.items() if k not in ("pool_pages", "peak_pages")}


def test_pooled_opening_width():
    """max_batch 4, max_seq 64.  Prompts 40 40 10 10 with limits 24 24 54 54: the opener is {0, 1} (tie with {2, 3}: the longer T) and two
    spare rows.  Its longest prompt takes 3 pages, so 10 pages open 10 // 3 = 3 rows (one spare), 8 pages 2 (no spare), 5 pages 1."""
    for pages, want in ((None, ([0, 1], 2)), (12, ([0, 1], 2)), (10, ([0, 1], 1)), (8, ([0, 1], 0)), (5, ([0], 0))):
        pol = RefillPolicy([40, 40, 10, 10], [24, 24, 54, 54], 4, 64, 4, True, pages)
        assert pol.open_stream() == want, pages
        assert pol.slot == want[0] + [None] * want[1] and pol.queue == [i for i in range(4) if i not in want[0]]


def test_agrees_with_the_independent_count():
    """The two inputs tests/test_kv_pool_gpu.py checks with its own replay of the schedule (`_host_schedule_preempts`): the policy on
    the stand-in preempts too, the same number of times."""
    import test_kv_pool_gpu as kp
    limits = list(kp.gga.LIMITS)
    pol, _ = drive([(kp.LENS[i], limits[i] - 1) for i in range(len(limits))], 4, kp.MAX_SEQ, 2, row_positions=True, kv_pages=kp.TIGHT)
    want = kp._host_schedule_preempts(limits, kp.TIGHT)
    print(f"fixture of 24 on 4 rows over {kp.TIGHT} pages: policy {pol.stats['preemptions']} evictions, independent count {want}")
    assert want >= 1 and pol.stats["preemptions"] == want and pol.stats["peak_pages"] <= kp.TIGHT
    limits = [20, 30, 24, 28, 36, 26]
    pol, _ = drive([(10, m - 1) for m in limits], 2, 64, 3, row_positions=True, kv_pages=4)
    want = kp._host_schedule_preempts(limits, 4, rows=2, packet=3, lens=[10] * 6, max_seq=64)
    print(f"six requests on 2 rows over 4 pages: policy {pol.stats['preemptions']} evictions, independent count {want}")
    assert want >= 1 and pol.stats["preemptions"] == want and pol.stats["peak_pages"] <= 4
