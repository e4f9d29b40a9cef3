"""Queued requests admitted into finished rows of a running talker stream (include/qtts.h, ABI v15: qtts_talker_stream_begin_admitting,
qtts_talker_stream_admit, qtts_talker_stream_rows; `TalkerEngine.generate(..., schedule="refill")`): a new request's prompt is prefilled
into the slots below the stream's position of a finished row while the other rows keep running, and everything that counts per request
-- history, floor, limit, trailing text, frame index, Philox step -- counts from the row's own origin.

The reference has no counterpart (it hands one static batch to HF generate): every request's result is pinned to what the REFERENCE
produced for that request in tests/golden/talker_tiny_admit.npz (tools/gen_golden_admit.py: 24 ragged requests, 2 trailing rows, greedy
with repetition penalty 1.05, 12 frames, EOS blocked, every cb-0 margin >= 1e-3 so that no comparison can stop early).  Request i under
its own limit L yields `codes[i, :L - 1]` by the row-limit rule.  The trailing rows and the penalty make a stream-relative index show up
as wrong codes.

The test BODIES (`body_*`) take the device; tests/test_refill_hostemu.py runs the same bodies on the host-emulation build."""
import ctypes as C
import dataclasses
import os
import sys

import numpy as np
import pytest
import torch

import synth
from qwen3_tts_amd import _lib as _qlib
from test_gpu_parity import _suppress, _td, dev  # noqa: F401  (`dev` is a fixture)
from test_row_sampling_gpu import TOL, _fake_ids, _gap, _np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import gen_golden_admit as gga  # noqa: E402  (the fixture's prompts and limits; its reference imports are inside generate())

pytestmark = pytest.mark.gpu
MARGIN_EXEMPT = 1e-3
LENS = gga.lens()
_CACHE = {}


def _fixture(golden_dir):
    """(fixture arrays, tiny config, weights, the 24 prompts): computed once and shared, never modified."""
    if "fx" not in _CACHE:
        g = np.load(os.path.join(golden_dir, "talker_tiny_admit.npz"))
        t = synth.talker_tiny()
        wn = synth.talker_weights(t)
        assert abs(float(g["weights_checksum"]) - synth.weights_checksum(wn)) < 1e-6, "synth weights changed: regenerate (tools/gen_golden_admit.py)"
        assert g["codes"].shape == (gga.N_REQ, gga.MAX_NEW - 1, t.num_code_groups) and float(g["margin"].min()) >= MARGIN_EXEMPT
        _CACHE["fx"] = (g, t, _td(wn), list(gga.prompt()))
    return _CACHE["fx"]


def _engine(t, w, dev, dtype, graph, B=4, max_seq=64):
    from qwen3_tts_amd.talker import TalkerEngine
    return TalkerEngine(t, w, weight_dtype=dtype, device=dev, max_batch=B, max_seq=max_seq, use_graph=graph)


GREEDY = dict(do_sample=0, top_k=50, top_p=1.0, temperature=0.9, repetition_penalty=gga.REP, subtalker_dosample=0, subtalker_top_k=50,
              subtalker_top_p=1.0, subtalker_temperature=0.9, min_new_tokens=gga.MAX_NEW, seed=0)


def _table(settings):
    rows = (_qlib.RowSamplingC * len(settings))()
    for r, s in zip(rows, settings):
        for k, v in s.items():
            setattr(r, k, v)
    return rows


class Stream:
    """An admitting stream driven call by call through `TalkerEngine.stream_open / stream_step / stream_rows / stream_admit / stream_close`.
    A request is (index into the fixture's prompts, its settings).  `out[req]` receives the frames of a retired request."""

    def __init__(self, eng, t, args, first, settings, max_row=gga.MAX_NEW, hidden=False):
        self.eng, self.t, self.args, self.settings = eng, t, args, settings
        self.emb, self.mask, self.trail, self.pad = args
        self.T = self.emb.shape[1]
        self.out, self.out_hidden = {}, {}
        e, npd, tr, tab = self._group(first)
        self.codes, self.hidden = eng.stream_open(e, npd, tr, self.pad, tab, max_row, t.codec_eos_token_id, _suppress(t), hidden)
        self.slot = list(first)
        self.max_row = max_row

    def _group(self, reqs):
        Tg = max(LENS[i] for i in reqs)
        return (self.emb[reqs][:, self.T - Tg:], [Tg - LENS[i] for i in reqs], self.trail[reqs], _table([self.settings[i] for i in reqs]))

    def step(self, n):
        return self.eng.stream_step(n)

    def rows(self):
        return self.eng.stream_rows()

    def retire(self):
        """Copy out every finished row that still holds a request; returns the rows that are free now."""
        unfinished, frames, _ = self.rows()
        for b, r in enumerate(self.slot):
            if r is not None and not unfinished[b]:
                self.out[r] = _np(self.codes[b, :frames[b]])
                if self.hidden is not None:
                    self.out_hidden[r] = _np(self.hidden[b, :frames[b]])
                self.slot[b] = None
        return [b for b, r in enumerate(self.slot) if r is None]

    def admit(self, pairs):
        """pairs: [(row, request)]"""
        rows_, reqs = [p[0] for p in pairs], [p[1] for p in pairs]
        e, npd, tr, tab = self._group(reqs)
        self.eng.stream_admit(rows_, e, npd, tr, tab)
        for b, r in pairs:
            self.slot[b] = r

    def finish(self, tokens=False):
        fin = False
        while not fin:
            _, fin = self.step(4)
        self.retire()
        assert all(r is None for r in self.slot)
        tok = torch.full((len(self.slot), self.max_row), -7, dtype=torch.int64, device=self.codes.device) if tokens else None
        self.eng.stream_close(tok)
        return _np(tok) if tokens else None


def _check_request(g, t, codes, req, L):
    """A request that ran under the limit L against the reference: all 16 codebooks of its L - 1 frames."""
    assert codes.shape == (L - 1, t.num_code_groups), (req, L, codes.shape)
    assert np.array_equal(codes, g["codes"][req, :L - 1]), (req, L)
    return L - 1


# ============================================================================================ 1. / 2. refill equals the reference
def body_refill_reference(dev, golden_dir, graph, max_seq):
    """fp32, max_batch 4, the 24 requests of the fixture through `generate(schedule="refill")`: every request gets its fixture codes on
    all 16 codebooks, every frame compared (no margin of the fixture lets the rule stop early).  max_seq 128: at least 16 rows are
    admitted and fewer streams are begun than the 6 waves the static schedule needs; max_seq 40: the shared position runs out, at least
    two streams are begun, same results.  An admission captures nothing: at most one frame graph per stream begun."""
    g, t, w, args = _fixture(golden_dir)
    eng = _engine(t, w, dev, torch.float32, graph, 4, max_seq)
    out = eng.generate(*args, schedule="refill", max_new_tokens=gga.LIMITS, min_new_tokens=gga.MAX_NEW, do_sample=False,
                       subtalker_dosample=False, repetition_penalty=gga.REP, suppress_tokens=_suppress(t), packet_frames=2)
    codes, st = _np(out.codes), eng.last_refill
    print(f"refill, max_seq {max_seq}, graph {graph}: {st}")
    compared = 0
    for i, L in enumerate(gga.LIMITS):
        compared += _check_request(g, t, codes[i, :L - 1], i, L)
        assert (codes[i, L - 1:, 0] == t.codec_eos_token_id).all(), i
        assert np.array_equal(_np(out.tokens)[i, :L - 1], g["tokens"][i, :L - 1])
    assert compared == sum(L - 1 for L in gga.LIMITS)
    assert st["admit_calls"] >= 1 and st["admitted_rows"] + 4 * st["streams"] == gga.N_REQ
    if max_seq >= 128:
        assert st["admitted_rows"] >= 16 and st["streams"] < 6, st
        assert eng.stats()["admitted_rows"] == st["admitted_rows"] or st["streams"] > 1
    else:
        assert st["streams"] >= 2, st
    assert st["graph_captures"] <= (st["streams"] if graph else 0), st
    assert eng.stats()["row_table_last"] == 1


@pytest.mark.parametrize("graph", [False, True])
def test_refill_gives_every_request_its_reference_codes(dev, golden_dir, graph):
    body_refill_reference(dev, golden_dir, graph, 128)


@pytest.mark.parametrize("graph", [False, True])
def test_refill_restarts_when_the_shared_position_runs_out(dev, golden_dir, graph):
    body_refill_reference(dev, golden_dir, graph, 40)


# ============================================================================================ 3. edges at the ABI
def _greedy_settings(limits):
    """settings of all 24 requests: greedy, EOS blocked, limit 13 unless `limits` says otherwise"""
    return [dict(GREEDY, max_new_tokens=limits.get(i, gga.MAX_NEW)) for i in range(gga.N_REQ)]


def _judge(g, t, dtype, out, limits):
    """fp32: the reference's codes, every frame.  bf16: the frame structure, and the project's bf16 bound against the fp32 fixture --
    the first two frames agree in at least 0.7 of the positions (tests/test_batch64_gpu.py, test_talker_large_batch_paths)."""
    agree = []
    for r, codes in out.items():
        L = limits.get(r, gga.MAX_NEW)
        assert codes.shape == (L - 1, t.num_code_groups), (r, codes.shape)
        if dtype == torch.float32:
            _check_request(g, t, codes, r, L)
        else:
            agree.append((codes[:2] == g["codes"][r, :min(2, L - 1)]).mean())
    if agree:
        print(f"bf16 agreement with the fp32 reference, first two frames, per request: {[round(float(a), 3) for a in agree]}")
        assert float(np.mean(agree)) >= 0.7


def body_edges(dev, golden_dir, dtype, case):
    g, t, w, args = _fixture(golden_dir)
    if case == "pads_pages":
        # rows: requests 1 (10 prompt rows), 0, 2, 4; rows 1 and 2 stop after 2 steps.  At position 12 request 5 (12 rows: n_pad 0, base 0)
        # and request 8 (7 rows: n_pad 5) enter in ONE call; request 8 stops after 8 steps of its own, and at position 20 request 3
        # (11 rows) enters alone: base 9, no multiple of 16, slots 9..19 cross the 16-key page.
        limits = {0: 3, 2: 3, 8: 9, 3: 6}
        eng = _engine(t, w, dev, dtype, True)
        s = Stream(eng, t, args, [1, 0, 2, 4], _greedy_settings(limits))
        assert s.step(2) == (2, False)
        assert s.rows() == ([1, 0, 0, 1], [2, 2, 2, 2], 12)
        assert s.retire() == [1, 2]
        caps = eng.stats()["graph_captures"]
        s.admit([(1, 5), (2, 8)])
        assert s.rows() == ([1, 1, 1, 1], [2, 0, 0, 2], 12)           # token 0 sampled, the stream's counters did not move
        assert s.step(8) == (10, False)
        assert s.rows() == ([1, 1, 0, 1], [10, 8, 8, 10], 20)
        assert s.retire() == [2]
        s.admit([(2, 3)])
        s.finish()
        st = eng.stats()
        assert (st["admit_calls"], st["admitted_rows"]) == (2, 3) and st["graph_captures"] == caps, st
    elif case == "latched":
        # all four rows stop in the same step: the stop condition latches; launches behind it do nothing; an admission lifts it
        limits = {0: 3, 1: 3, 2: 3, 4: 3, 9: 5, 10: 4}
        eng = _engine(t, w, dev, dtype, True)
        s = Stream(eng, t, args, [1, 0, 2, 4], _greedy_settings(limits))
        assert s.step(6) == (2, True)
        assert s.step(3) == (2, True)
        assert s.rows() == ([0, 0, 0, 0], [2, 2, 2, 2], 12)
        assert s.retire() == [0, 1, 2, 3]
        s.admit([(3, 5), (0, 12)])          # 12 and 9 prompt rows at position 12
        assert s.rows()[0] == [1, 0, 0, 1]
        assert s.step(1) == (3, False)
        s.finish()
        assert eng.stats()["admitted_rows"] == 2
    else:
        # split-KV mode from 20 keys on: the stream is in it when requests 7 (13 rows) and 10 (8 rows) enter at position 21 (base 8)
        limits = {0: 7, 2: 7, 7: 5, 10: 5}
        with _qlib.options(QTTS_ATTN_NSPLIT="2", QTTS_ATTN_SPLIT_FROM="20", QTTS_ATTN_SPLIT_KEYS="64"):
            eng = _engine(t, w, dev, dtype, True)
        s = Stream(eng, t, args, [11, 9, 0, 2], _greedy_settings(limits))
        assert s.step(6) == (6, False)
        assert s.rows() == ([1, 1, 0, 0], [6, 6, 6, 6], 21)
        assert eng.stats()["attn_nsplit_last"] == 2
        assert s.retire() == [2, 3]
        s.admit([(2, 7), (3, 10)])
        s.finish()
        st = eng.stats()
        assert st["attn_nsplit_last"] == 2 and st["long_graphs"] >= 1 and st["admitted_rows"] == 2, st
    assert len(s.out) == {"pads_pages": 7, "latched": 6, "split_kv": 6}[case]
    _judge(g, t, dtype, s.out, limits)


@pytest.mark.parametrize("case", ["pads_pages", "latched", "split_kv"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_admission_edges_at_the_abi(dev, golden_dir, dtype, case):
    body_edges(dev, golden_dir, dtype, case)


# ============================================================================================ 4. neighbours undisturbed
def _neighbour_run(eng, t, args, settings, admit):
    s = Stream(eng, t, args, [1, 0, 2, 4], settings, hidden=True)
    s.step(2)
    free = s.retire()
    assert free == [1, 2]
    if admit:
        s.admit([(1, 5), (2, 8)])
    tok = s.finish(tokens=True)
    return s.out, s.out_hidden, tok[[0, 3], :11]          # (behind its 11 tokens an idle row shows eos for as long as the stream runs on)


def body_neighbours(dev, golden_dir, dtype, t=None, w=None, args=None, want_layer=False):
    """The rows that keep running across an admission (rows 0 and 3) give bit-identical codes, tokens and hidden states to the same
    stream without the admission; sampling rows, so that a disturbed Philox counter would show too."""
    if t is None:
        _, t, w, args = _fixture(golden_dir)
    settings = [dict(GREEDY, do_sample=1, subtalker_dosample=1, seed=900 + i, max_new_tokens={0: 3, 2: 3}.get(i, 11)) for i in range(gga.N_REQ)]
    eng = _engine(t, w, dev, dtype, True)
    with_adm = _neighbour_run(eng, t, args, settings, True)
    assert eng.stats()["admitted_rows"] == 2
    if want_layer:
        assert eng.stats()["cp_layer_per_step"] > 0, "the fused layer launch did not run: nothing was shown about the launches around an admission"
    without = _neighbour_run(eng, t, args, settings, False)
    assert eng.stats()["admitted_rows"] == 0
    for r in (1, 4):
        assert with_adm[0][r].shape[0] == 10
        assert np.array_equal(with_adm[0][r], without[0][r]) and np.array_equal(with_adm[1][r], without[1][r]), r
    assert np.array_equal(with_adm[2], without[2]) and (with_adm[2][:, :10] >= 0).all() and (with_adm[2][:, 10] == t.codec_eos_token_id).all()
    again = _neighbour_run(eng, t, args, settings, True)
    for r in with_adm[0]:
        assert np.array_equal(with_adm[0][r], again[0][r]) and np.array_equal(with_adm[1][r], again[1][r]), r


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_running_rows_are_not_disturbed_by_an_admission(dev, golden_dir, dtype):
    body_neighbours(dev, golden_dir, dtype)


def body_refill_repeatable(dev, golden_dir, dtype):
    """Two identical sampling refill runs are bit-identical."""
    _, t, w, args = _fixture(golden_dir)
    eng = _engine(t, w, dev, dtype, True)
    kw = dict(schedule="refill", max_new_tokens=gga.LIMITS, min_new_tokens=2, seed=31, temperature=1.1, suppress_tokens=_suppress(t))
    a, b = eng.generate(*args, **kw), eng.generate(*args, **kw)
    assert eng.last_refill["admitted_rows"] >= 1
    assert np.array_equal(_np(a.codes), _np(b.codes)) and np.array_equal(_np(a.hidden), _np(b.hidden))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_two_identical_refill_runs_are_bit_identical(dev, golden_dir, dtype):
    body_refill_repeatable(dev, golden_dir, dtype)


def body_neighbours_released_cp(dev):
    """Tiny talker dims with the released code predictor's dims, bf16, 4 rows: the fused launches (cp_layer.hip) run around an admission."""
    t6 = synth.talker_06b()
    t = dataclasses.replace(synth.talker_tiny(), **{f.name: getattr(t6, f.name) for f in dataclasses.fields(t6) if f.name.startswith("cp_")})
    w = _td(synth.talker_weights(t, with_text=False))
    args = list(synth.rand_prompt(np.random.default_rng(7), t, LENS, gga.N_TRAIL, scale=0.5))
    body_neighbours(dev, None, torch.bfloat16, t, w, args, want_layer=True)


def test_running_rows_are_not_disturbed_at_the_released_code_predictor_dims(dev):
    body_neighbours_released_cp(dev)


# ============================================================================================ 5. sampling
def body_sampling(dev, golden_dir, dtype, graph):
    """Request 5 enters row 1 at stream step 2 and runs 3 steps of its own.  Every sub-code draw of its last frame and its last talker
    draw lie in the row's inverse-CDF interval for u = Philox(seed; OWN step 3, 0, codebook) within TOL; evaluated with the stream's
    step counter (5) the same draws miss by more than 1e-3.  Row 0, which began with the stream, passes with the stream's counter."""
    _, t, w, args = _fixture(golden_dir)
    sup = _suppress(t)
    knobs = lambda i: dict(do_sample=1, top_k=[50, 20, 64][i % 3], top_p=1.0, temperature=[0.9, 1.3, 0.7][i % 3], repetition_penalty=[1.05, 1.5][i % 2],
                           subtalker_dosample=1, subtalker_top_k=[50, 5, 64][i % 3], subtalker_top_p=1.0, subtalker_temperature=[0.9, 0.6, 1.3][i % 3],
                           min_new_tokens=40, seed=4000 + 13 * i, max_new_tokens={0: 3, 2: 3}.get(i, 11))
    settings = [knobs(i) for i in range(gga.N_REQ)]
    eng = _engine(t, w, dev, dtype, graph)
    s = Stream(eng, t, args, [1, 0, 2, 4], settings)
    s.step(2)
    assert s.retire() == [1, 2]
    s.admit([(1, 5), (2, 8)])
    assert s.step(3) == (5, False)
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
    assert (tok[1, :4] >= 0).all() and (tok[1, 4:] == -1).all() and (tok[0, :6] >= 0).all() and (tok[0, 6:] == -1).all()
    own, stream_ctr, neighbour = gaps(1, 5, 2, 3), gaps(1, 5, 2, 5), gaps(0, 1, 4, 5)
    print(f"admitted row, draws of its last frame: worst gap {own:.2e} with its own step, {stream_ctr:.2e} with the stream's; row 0: {neighbour:.2e}")
    assert own <= TOL and neighbour <= TOL, (own, neighbour)
    assert stream_ctr > 1e-3, stream_ctr


@pytest.mark.parametrize("dtype,graph", [(torch.bfloat16, True), (torch.float32, False)])
def test_an_admitted_row_draws_with_its_own_step_counter(dev, golden_dir, dtype, graph):
    body_sampling(dev, golden_dir, dtype, graph)


# ============================================================================================ 6. bf16 closeness
def _rel_rms(a, ref):
    return float(np.sqrt(((a - ref) ** 2).mean()) / np.sqrt((ref ** 2).mean()))


def _plain_prefill_logits(eng, args, req):
    """the raw first-step logits of request `req` prefilled alone (qtts_talker_prefill: existing code)"""
    emb, _, trail, pad = args
    dev = eng.device
    e = emb[req:req + 1, emb.shape[1] - LENS[req]:].to(dev, torch.float32).contiguous()
    tr, pd = trail[req:req + 1].to(dev, torch.float32).contiguous(), pad.to(dev, torch.float32).reshape(-1).contiguous()
    npad = (C.c_int32 * 1)(0)
    eng._stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.device(dev), torch.cuda.stream(eng._stream):
        _qlib.check(eng._lib.qtts_talker_prefill(eng._h, C.c_void_p(e.data_ptr()), 1, LENS[req], npad, C.c_void_p(tr.data_ptr()), tr.shape[1],
                                                 C.c_void_p(pd.data_ptr()), eng._s()))
    return _np(eng.debug_logits()[0])


def body_bf16_closeness(dev, golden_dir):
    """Request 3 (11 prompt rows) admitted at position 20 (base 9) into a bf16 stream: its first-step raw logits against the fp32
    engine's logits for that prompt have a relative RMS of at most 1.25 x what the same bf16 engine's plain prefill of the prompt alone
    shows against the same fp32 logits (the margin: another summation chunking at another absolute position).
    Measured: see profiles/refill.md."""
    _, t, w, args = _fixture(golden_dir)
    ref = _plain_prefill_logits(_engine(t, w, dev, torch.float32, True), args, 3)
    eng = _engine(t, w, dev, torch.bfloat16, True)
    plain = _rel_rms(_plain_prefill_logits(eng, args, 3), ref)
    s = Stream(eng, t, args, [1, 0, 2, 4], _greedy_settings({0: 3}))
    assert s.step(10) == (10, False) and s.rows()[2] == 20
    assert s.retire() == [1]
    s.admit([(1, 3)])
    admitted = _rel_rms(_np(eng.debug_logits()[1]), ref)
    s.finish()
    print(f"bf16 first-step logits against fp32, relative RMS: admitted at position 20 {admitted:.4e}, plain prefill {plain:.4e}, ratio {admitted / plain:.3f}")
    assert plain > 0 and admitted <= 1.25 * plain, (admitted, plain)


def test_bf16_admitted_prefill_is_as_close_to_fp32_as_the_plain_prefill(dev, golden_dir):
    body_bf16_closeness(dev, golden_dir)


# ============================================================================================ 8. wrapper
def body_wrapper(dev):
    """`Qwen3TTSForConditionalGeneration.generate(schedule="refill")`: 10 requests of different lengths on 4 rows, fp32 greedy, fixed
    per-request seeds and limits -- the same per-request codes as the default schedule; without `schedule` the wave path runs."""
    from qwen3_tts_amd.model import Qwen3TTSForConditionalGeneration
    t = synth.talker_tiny()
    cfgd = dict(synth.cfg_dict(t), tts_model_type="custom_voice", tts_model_size="tiny", tokenizer_type="12hz")
    model = Qwen3TTSForConditionalGeneration(cfgd, _td(synth.talker_weights(t)), device=dev, dtype=torch.float32, max_batch=4, max_seq=128)
    n = 10
    ids = [_fake_ids(t, "request number %d " % i + "x" * (3 * i % 7)) for i in range(n)]
    assert len({x.shape[1] for x in ids}) > 2
    kw = dict(input_ids=ids, languages=["english"] * n, speakers=["vivian", "ryan"] * (n // 2), do_sample=False, subtalker_dosample=False,
              max_new_tokens=[4 + (5 * i) % 9 for i in range(n)], seed=[70 + i for i in range(n)])
    waves, _ = model.generate(**kw)
    st = model.talker.stats()
    assert st["admit_calls"] == 0 and st["admitted_rows"] == 0
    refill, hid = model.generate(schedule="refill", **kw)
    st = model.talker.stats()
    assert st["admit_calls"] >= 1 and model.talker.last_refill["admitted_rows"] >= n - 4 - 4 * (model.talker.last_refill["streams"] - 1)
    assert len(waves) == len(refill) == len(hid) == n
    for i in range(n):
        assert refill[i].shape[0] >= 1 and np.array_equal(_np(waves[i]), _np(refill[i])), i
    with pytest.raises(ValueError, match="schedule"):
        model.generate(schedule="eager", **kw)


def test_wrapper_takes_the_refill_schedule(dev):
    body_wrapper(dev)
