"""The scheduling policy of the refill schedules (`TalkerEngine.generate / generate_stream(..., schedule="refill" | "continuous")`):
which requests open a stream, which row is preempted, which rows report into a packet, which queued requests are admitted.

Pure bookkeeping on integers: `RefillPolicy` holds no engine and no tensor.  `TalkerEngine._refill_stream` drives the engine and hands
the policy what it observed there (`stream_kv`, `stream_row_lens`, `stream_rows`); tests/test_refill_policy.py drives it with a counting
stand-in.  The schedule itself is described at `TalkerEngine._refill_stream`."""
from collections import namedtuple
from dataclasses import dataclass
from typing import Any, List, Optional, Tuple


@dataclass
class RefillRow:
    """One row's share of a `RefillPacket`."""
    request: int               # index of the request in the list given to `generate_stream`
    row: int                   # the row (= codec slot) the request occupies
    codes: Any                 # (k, G) int64 tensor: the frames the request gained in this packet (a copy; k may be 0 when `last`)
    first: bool                # the request started with this packet: whatever the row held before belongs to another request
    last: bool                 # the request finished: its frames end here (first eos in codebook 0, or its own limit)
    hidden: Optional[Any] = None                 # (k, H) float32 tensor, `past_hidden` of these frames, when asked for
    restart: bool = False      # (pooled engines) the request was preempted and starts again at frame 0 with this packet: set together with
                               # `first`; drop what was collected for it -- the replayed frames equal the dropped ones


@dataclass
class RefillPacket:
    """What `generate_stream(..., schedule="refill")` yields after every packet of the running stream: one entry per row whose occupant
    gained frames or finished in it."""
    rows: List[RefillRow]


# a row that reports into the packet just run: frames k0..k1 of its occupant are new (`RefillRow` without the tensors)
Report = namedtuple("Report", "request row k0 k1 first last restart")


def pages_of(n_keys: int) -> int:
    """16-key pages that hold n_keys keys"""
    return -(-int(n_keys) // 16)


def widest_opener(queue, lens, limits, max_seq, max_batch):
    """The opening group of a stream with per-row positions: among the groups {requests no longer than T whose limit fits behind T}
    for every prompt length T, the one with the most members (at most max_batch, longest prompts first; ties go to the longer T).
    `queue` is sorted longest first.  Limits clamped to the room their own prompt leaves fit only behind their own length, so the group
    can be narrow: the scheduler fills the stream's other rows with spare rows."""
    best = []
    for T in sorted({lens[i] for i in queue}, reverse=True):
        cand = [i for i in queue if lens[i] <= T and T + limits[i] <= max_seq][:max_batch]
        if len(cand) > len(best):
            best = cand
    return best


class RefillPolicy:
    """`lens[i]`, `limits[i]`: request i's prompt length and its `max_new_tokens` (clamped to the room its own prompt leaves).
    `row_positions`: the continuous schedule; with `kv_pages` on top, the optimistic pooled one.  State: `queue` (requests waiting, in
    admission order), `slot[b]` (the request in row b, None: the row is free), `seen[b]` (frames of it already reported), `fresh` (requests
    whose next report is their first), `restarted` (of those, the preempted ones), `stats` (what becomes `TalkerEngine.last_refill`)."""

    def __init__(self, lens, limits, max_batch, max_seq, packet_frames, row_positions=False, kv_pages=None):
        self.lens, self.limits = [int(x) for x in lens], [int(x) for x in limits]
        self.max_batch, self.max_seq, self.packet_frames = int(max_batch), int(max_seq), int(packet_frames)
        self.row_positions, self.kv_pages = bool(row_positions), int(kv_pages or 0)
        self.pooled = bool(self.row_positions and self.kv_pages)
        # (a pool that holds max_seq keys for every row can never run dry: nothing is preempted, so admission is not held back either)
        self.tight = self.pooled and self.kv_pages < self.max_batch * pages_of(self.max_seq)
        self.queue = sorted(range(len(self.lens)), key=lambda i: (-self.lens[i], i))
        self.slot, self.seen, self.fresh, self.restarted = [], [], set(), set()
        self.stats = dict(streams=0, admit_calls=0, admitted_rows=0, frames_run=0, row_frames=0, graph_captures=0, max_row_len=0,
                          pool_pages=self.kv_pages, peak_pages=0, preemptions=0)

    @property
    def active(self) -> bool:
        """the open stream still has an occupied row"""
        return any(r is not None for r in self.slot)

    def open_stream(self) -> Tuple[List[int], int]:
        """A fresh stream: (the requests of its opening group, spare rows behind them).  Shared position: the longest prompt first, then
        the longest of the rest whose limits fit behind it.  Per-row positions: the ONE stream's width is its opening group's (an
        admission takes a row of the stream), so it opens with the widest group that fits and is brought to full width with spare rows
        -- copies of the first prompt under the limit 1, finished with their token 0 -- that the first admission fills.  Pooled: the
        opening prompts (the spare rows' copies included) must fit the pool."""
        q, lens, limits, mb = self.queue, self.lens, self.limits, self.max_batch
        if self.row_positions:
            first = widest_opener(q, lens, limits, self.max_seq, mb)
            spare = min(mb, len(lens)) - len(first)
            if self.pooled:
                width = max(1, self.kv_pages // pages_of(max(lens[i] for i in first)))
                first = first[:width]
                spare = min(spare, width - len(first))
        else:
            first, spare = [i for i in q if lens[q[0]] + limits[i] <= self.max_seq][:mb], 0
        self.queue = [i for i in q if i not in first]
        self.slot, self.seen, self.fresh = list(first) + [None] * spare, [0] * (len(first) + spare), set(first)
        self.stats["streams"] += 1
        return first, spare

    def victim(self, held, free, row_len) -> Optional[int]:
        """Pooled, before a packet: the row to evict so that the pool can cover the packet, or None when it can (or one row is left:
        the only running row is never evicted).  `held[b]`, `free`: `stream_kv()`; `row_len[b]`: `stream_row_lens()`, both read again
        after every eviction.  The page count is the engine's own rule (include/qtts.h, stream_step on a pooled engine): a running row
        needs the pages of its length after the packet, a finished row gives its pages back.  The victim is the running request with the
        fewest frames (ties: the highest request index); it returns to the FRONT of the queue and will start again at frame 0."""
        need, avail, used = 0, free, 0
        for b, r in enumerate(self.slot):
            if r is None:
                avail += held[b]
                continue
            want = pages_of(row_len[b] + min(self.packet_frames, max(0, self.limits[r] - 1 - self.seen[b])))
            need += max(0, want - held[b])
            used += max(want, held[b])
        running = [b for b, r in enumerate(self.slot) if r is not None]
        if need <= avail or len(running) <= 1:
            self.stats["peak_pages"] = max(self.stats["peak_pages"], used)
            return None
        b = min(running, key=lambda b: (self.seen[b], -self.slot[b]))
        r, self.slot[b] = self.slot[b], None
        self.queue.insert(0, r)
        self.restarted.add(r)
        self.fresh.discard(r)
        self.stats["preemptions"] += 1
        return b

    def reports(self, unfinished, frames) -> List[Report]:
        """After a packet (`stream_rows()`): every row whose occupant gained frames or finished.  A finished row is retired."""
        out = []
        for b, r in enumerate(self.slot):
            if r is None:
                continue
            done, k0, k1 = not unfinished[b], self.seen[b], frames[b]
            if k1 > k0 or done:
                out.append(Report(r, b, k0, k1, r in self.fresh, done, r in self.fresh and r in self.restarted))
                self.fresh.discard(r)
                self.restarted.discard(r)
                self.seen[b] = k1
            if done:
                self.stats["row_frames"] += k1
                self.slot[b] = None
        return out

    def admissions(self, kv_len, free_pages=None) -> List[Tuple[List[int], List[int]]]:
        """After a packet: the `stream_admit` calls to make, as (rows, requests) groups; the requests take their rows here.
        Shared position (`kv_len`: the stream's, from `stream_rows()`): every queued request that fits -- prompt no longer than the
        position, position + its limit inside max_seq -- longest prompt first, as one group.  Per-row positions: the head of the queue,
        one request per free row, split by `_admission_groups`; on a tight pool (`free_pages`: `stream_kv()` after the packet) only as
        far as `_admissible` allows."""
        free = [b for b, r in enumerate(self.slot) if r is None]
        if self.row_positions:
            take = self._admissible(len(free), len(self.slot) - len(free), free_pages)
            groups = self._admission_groups(take)
        else:
            take = [i for i in self.queue if self.lens[i] <= kv_len and kv_len + self.limits[i] <= self.max_seq][:len(free)]
            groups = [take] if take else []
        out, at = [], 0
        for grp in groups:
            out.append((free[at:at + len(grp)], grp))
            at += len(grp)
        for b, r in zip(free, take):
            self.slot[b], self.seen[b] = r, 0
            self.fresh.add(r)
        self.queue = [i for i in self.queue if i not in take]
        return out

    def _admissible(self, n_free, running, free_pages):
        """The head of the queue that is admitted into n_free rows.  Tight pool: only while the prompt pages of its admission groups +
        one page per row then running <= free (the watermark keeps a preempted request from being admitted straight into the next
        preemption; nothing running and nothing taken yet: the prompt alone must fit)."""
        if not self.tight:
            return self.queue[:n_free]
        take = []
        for i in self.queue[:n_free]:
            cand = take + [i]
            prompt_pages = sum(len(grp) * pages_of(max(self.lens[j] for j in grp)) for grp in self._admission_groups(cand))
            if prompt_pages + (running + len(cand) if running or take else 0) > free_pages:
                break
            take = cand
        return take

    def _admission_groups(self, idx):
        """per-row positions: `idx` in queue order, cut into groups in each of which the padded length + every limit fits max_seq"""
        groups = []
        for i in idx:
            cand = (groups[-1] if groups else []) + [i]
            Tg = max(self.lens[j] for j in cand)
            if groups and all(Tg + self.limits[j] <= self.max_seq for j in cand):
                groups[-1] = cand
            else:
                groups.append([i])
        return groups

    def stream_closed(self, engine_stats, frames_run):
        """fold a closed stream's counters (`TalkerEngine.stats()` before `stream_close()`, and what that returned) into `stats`"""
        st = self.stats
        st["admit_calls"] += engine_stats["admit_calls"]
        st["admitted_rows"] += engine_stats["admitted_rows"]
        st["max_row_len"] = max(st["max_row_len"], engine_stats["max_row_len"]) if self.row_positions else 0
        st["frames_run"] += frames_run

    def finish(self, graph_captures) -> dict:
        """the call's `last_refill`"""
        self.stats["graph_captures"] = graph_captures
        self.stats["occupancy"] = self.stats["row_frames"] / max(1, self.stats["frames_run"] * self.max_batch)
        return self.stats
