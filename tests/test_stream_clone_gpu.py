"""Streaming voice clone and voice design: codec slots primed from reference codes (include/qtts.h qtts_codec_stream_prime_rows /
qtts_codec_stream_prime_tail), `Qwen3TTSModel.stream_voice_clone` and `Qwen3TTSModel.stream_voice_design`.

The reference decodes a cloned voice as `cat([ref_code, codes])` and cuts the reference's share off the waveform
(qwen3_tts_model.py:612-631).  The decoder is causal, so a codec slot must stand where "the reference has just been decoded" before the
first generated frame is pushed.  `stream_prime_rows` puts it there for rows of different reference lengths in one set of launches, and
sends only the last `prime_tail_frames` frames of a reference through the upsampling stack.  Whatever is pushed next must come out as
`forward(cat(ref, gen))[..., ref * up:]`.

The bars are those of tests/test_stream_slots_gpu.py: 1e-5 RMS against the engine's whole-sequence `forward`, RMS_BAR against
`codec_ref.decoder_forward`.  The test BODIES (`body_*`) take the device; tests/test_stream_clone_hostemu.py runs them on the
host-emulation build with reduced plans."""
import numpy as np
import pytest
import torch

import codec_ref
import synth
from test_gpu_parity import RMS_BAR, _rms, _td, dev  # noqa: F401  (`dev` is a fixture)
import test_stream_slots_gpu as ss

pytestmark = pytest.mark.gpu
PACKETS = ss.PACKETS            # (1, 4, 2, 7), cycled
# tiny codec: window 8 (W1 = 7), prime tail 10.  Reference lengths: shorter than the tail, the tail, one more, longer than tail + window.
# (slot, reference frames), listed in this order: the slots are out of order
RAGGED = ((2, 3), (0, 10), (3, 11), (1, 40))
RAGGED_REDUCED = ((2, 3), (0, 10), (1, 11), (3, 18))
_CACHE = {}
QTTS_ERR_ARG, QTTS_ERR_STATE, QTTS_ERR_LIMIT = -1, -3, -6


def derive_tail(c):
    """The backward walk over the stack behind the transformer: trailing input rows of each layer that must be exact so that the last
    rows of every stateful layer's input -- its carry -- are.  Independent of the engine's own derivation (csrc/codec_engine.hip)."""
    need = 6                                        # final conv, k = 7
    for r in reversed(list(c.upsample_rates)):
        need += 6 * 9 + 6 * 3 + 6 * 1               # three residual units, conv k = 7 with dilations 9, 3, 1
        need = -(-need // r) + 1                    # transposed conv k = 2r
    need += 6                                       # decoder.0, k = 7
    for f in reversed(list(c.upsampling_ratios)):
        need += 6                                   # ConvNeXt dwconv, k = 7
        need = -(-need // f)                        # transposed conv k = s = f
    return need


def _seq(c, seed, T):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, c.codebook_size, (1, c.num_quantizers, T)))


def _block(c, refs, n_max, dev):
    """(M, Q, n_max): every reference right-aligned; the columns in front hold an index past the codebook -- reading one is an error"""
    block = torch.full((len(refs), c.num_quantizers, n_max), c.codebook_size + 3, dtype=torch.long)
    for m, r in enumerate(refs):
        block[m, :, n_max - r.shape[-1]:] = r[0]
    return block.to(dev)


def push_all(eng, c, ids, gens, dev, packets=PACKETS):
    """Push every sequence of `gens` ({slot: (1, Q, T)}, equal T) through its slot in packets cycled over `packets`, the slots listed as
    `ids`; the last packet is padded with code 0 and its surplus samples dropped.  Returns {slot: PCM (T * up,)}."""
    up = c.total_upsample
    T = next(iter(gens.values())).shape[-1]
    out = {s: [] for s in ids}
    pos, p = 0, 0
    while pos < T:
        n = packets[p % len(packets)]
        k = min(n, T - pos)
        batch = torch.zeros(len(ids), c.num_quantizers, n, dtype=torch.long)
        for m, s in enumerate(ids):
            batch[m, :, :k] = gens[s][0, :, pos:pos + k]
        wav = eng.stream_push_rows(list(ids), batch.to(dev))[:, 0].cpu().numpy()
        assert wav.shape == (len(ids), n * up)
        for m, s in enumerate(ids):
            out[s].append(wav[m, :k * up].copy())
        pos += k
        p += 1
    return {s: np.concatenate(v) for s, v in out.items()}


def _expected(eng, c, w, plan, refs, gens, dev, key):
    """per slot: (forward(cat(ref, gen)) behind the reference's samples, the oracle's) -- computed once per plan"""
    if key not in _CACHE:
        exp = {}
        for s, r in plan:
            full = torch.cat([refs[s], gens[s]], dim=-1)
            with torch.no_grad():
                o = codec_ref.decoder_forward(w, c, full).numpy()[0, 0]
            exp[s] = (eng.forward(full.to(dev)).cpu().numpy()[0, 0][r * c.total_upsample:], o[r * c.total_upsample:])
        _CACHE[key] = exp
    return _CACHE[key]


# ============================================================================================ 1. ragged prime, tiny codec
def body_ragged_prime(dev, plan, n_gen):
    from qwen3_tts_amd import _lib
    c, w, eng = ss._tiny(dev)
    up = c.total_upsample
    assert c.sliding_window == 8 and eng.prime_tail_frames == 10
    ids = [s for s, _ in plan]
    assert ids != sorted(ids)
    refs = {s: _seq(c, 100 + s, r) for s, r in plan}
    gens = {s: _seq(c, 200 + s, n_gen) for s, _ in plan}
    exp = _expected(eng, c, w, plan, refs, gens, dev, ("ragged", tuple(plan), n_gen))
    longest = max(r for _, r in plan)
    results = {}
    for n_max in (longest, longest + 5):            # the longest row unpadded; every row padded
        for tail in (True, False):
            _lib.set_option("QTTS_CODEC_PRIME_TAIL", None if tail else 0, lib=eng._lib)
            try:
                eng.stream_begin(4)
                eng.stream_prime_rows(ids, _block(c, [refs[s] for s in ids], n_max, dev), [r for _, r in plan])
            finally:
                _lib.set_option("QTTS_CODEC_PRIME_TAIL", None, lib=eng._lib)
            results[n_max, tail] = push_all(eng, c, ids, gens, dev)
    for (n_max, tail), got in results.items():
        for s, r in plan:
            assert got[s].shape == (n_gen * up,), (s, got[s].shape)
            d_fwd, d_ref = _rms(got[s], exp[s][0]), _rms(got[s], exp[s][1])
            d_tail = _rms(got[s], results[n_max, True][s])
            print(f"n_max {n_max}, tail {'on' if tail else 'off'}, slot {s} behind {r} reference frames: rms against forward {d_fwd:.2e}, "
                  f"against the oracle {d_ref:.2e}, against the tail's {d_tail:.2e}")
            assert d_fwd <= 1e-5 and d_ref <= RMS_BAR, (n_max, tail, s, d_fwd, d_ref)
            assert d_tail <= 1e-5, (n_max, s, d_tail)
    # the comparison bites: a slot that is only reset is far from the reference
    eng.stream_begin(4)
    eng.stream_reset_rows(ids)
    bare = push_all(eng, c, ids, gens, dev)
    for s, r in plan:
        d = _rms(bare[s], exp[s][1])
        print(f"slot {s}: reset only, not primed with its {r} reference frames: rms against the oracle {d:.2e}")
        assert d >= 100 * RMS_BAR, (s, d)


def test_ragged_prime_equals_forward_behind_the_reference(dev):
    body_ragged_prime(dev, RAGGED, 12)


# ============================================================================================ 2. neighbours
def body_neighbours(dev, at=(5, 19), ref_lens=(4, 13), n_gen=9):
    """Slots 3 and 0 are mid-stream at frames at[0] and at[1] when slots 1 and 2 are primed.  The running slots' PCM is bit-identical to
    the run without the prime; the primed slots' PCM is bit-identical whatever the neighbours' codes are, and whether the slot was fresh or
    had been in use."""
    c, w, eng = ss._tiny(dev)
    run_ids, new_ids = (3, 0), (2, 1)
    refs = [_seq(c, 300 + i, r) for i, r in enumerate(ref_lens)]
    gens = {s: _seq(c, 310 + s, n_gen) for s in new_ids}

    def run(seed, prime, used):
        heads = {s: _seq(c, seed + s, t) for s, t in zip(run_ids, at)}
        tails = {s: _seq(c, seed + 10 + s, n_gen) for s in run_ids}
        eng.stream_begin(4)
        if used:                                                     # the slots to prime have decoded something else before
            eng.stream_push_rows(list(new_ids), torch.cat([_seq(c, 390 + s, 6) for s in new_ids]).to(dev))
        for s in run_ids:
            eng.stream_push_rows([s], heads[s].to(dev))
        if prime:
            eng.stream_prime_rows(list(new_ids), _block(c, refs, max(ref_lens) + 2, dev), list(ref_lens))
        else:                                                        # (the same pushes, so the same launch shapes, behind a plain reset)
            eng.stream_reset_rows(list(new_ids))
        both = push_all(eng, c, run_ids + new_ids, {**tails, **gens}, dev)
        return {s: both[s] for s in run_ids}, {s: both[s] for s in new_ids}

    running, primed = run(320, True, False)
    alone, bare = run(320, False, False)
    assert all(not np.array_equal(primed[s], bare[s]) for s in new_ids)
    for s in run_ids:
        assert np.array_equal(running[s], alone[s]), f"slot {s}: disturbed by the prime of its neighbours"
    _, other = run(340, True, False)
    _, reused = run(320, True, True)
    for s in new_ids:
        assert np.array_equal(primed[s], other[s]), f"slot {s}: its PCM depends on its neighbours' codes"
        assert np.array_equal(primed[s], reused[s]), f"slot {s}: priming a used slot differs from priming a fresh one"


def test_prime_leaves_neighbours_alone_and_implies_the_reset(dev):
    body_neighbours(dev)


# ============================================================================================ 3. the tail, refusals
def body_tail_frames(dev):
    c, w, eng = ss._tiny(dev)
    assert derive_tail(c) == 10 and eng.prime_tail_frames == derive_tail(c)


def test_prime_tail_frames_follow_the_config(dev):
    body_tail_frames(dev)
    c, eng = ss._real(dev, torch.float32)
    assert derive_tail(c) == 10 and eng.prime_tail_frames == derive_tail(c)


def body_refusals(dev):
    """Every refusal names what it refuses and changes nothing: a refused prime followed by pushes equals the pushes without it."""
    from qwen3_tts_amd import _lib
    from qwen3_tts_amd.codec import CodecDecoderEngine
    c, w, eng = ss._tiny(dev)
    fresh = CodecDecoderEngine(c, w, compute_dtype=torch.float32, device=dev, max_batch=4, max_frames=64)
    ref = _seq(c, 400, 6)
    with pytest.raises(_lib.QttsError, match=r"stream_begin\(\) first") as e:
        fresh.stream_prime_rows([0], ref.to(dev), [6])
    assert e.value.code == QTTS_ERR_STATE
    seqs = {s: _seq(c, 410 + s, 8) for s in (2, 0)}
    eng.stream_begin(4)
    clean = push_all(eng, c, (2, 0), seqs, dev, packets=(1,))
    two = torch.cat([ref, ref]).to(dev)
    # (behind the transformer a prime holds only its tail, so it is the transformer's rows that outgrow the workspace: 4 x 12288 frames
    # of its widest activation against the 4 x 64 frames of the widest activation of the stack)
    big = torch.zeros(4, c.num_quantizers, 12288, dtype=torch.long, device=dev)
    cases = ((QTTS_ERR_ARG, "stream_prime_rows: row 4 is not a row", lambda: eng.stream_prime_rows([2, 4], two, [6, 6])),
             (QTTS_ERR_ARG, "stream_prime_rows: row -1 is not a row", lambda: eng.stream_prime_rows([-1], ref.to(dev), [6])),
             (QTTS_ERR_ARG, "stream_prime_rows: row 2: listed twice", lambda: eng.stream_prime_rows([2, 2], two, [6, 6])),
             (QTTS_ERR_ARG, "stream_prime_rows: row 0: n_frames 0 is not in [1, n_max = 6]", lambda: eng.stream_prime_rows([2, 0], two, [6, 0])),
             (QTTS_ERR_ARG, "stream_prime_rows: row 2: n_frames 7 is not in [1, n_max = 6]", lambda: eng.stream_prime_rows([2, 0], two, [7, 6])),
             (QTTS_ERR_LIMIT, "exceed the workspace", lambda: eng.stream_prime_rows([3, 2, 1, 0], big, [12288, 1, 64, 64])))
    eng.stream_begin(4)
    got = {s: [] for s in seqs}
    for t in range(8):
        if t < len(cases):
            code, frag, call = cases[t]
            with pytest.raises(_lib.QttsError) as e:
                call()
            assert e.value.code == code and frag in str(e.value), (frag, str(e.value))
        wav = eng.stream_push_rows([2, 0], torch.cat([seqs[2][..., t:t + 1], seqs[0][..., t:t + 1]]).to(dev))[:, 0].cpu().numpy()
        got[2].append(wav[0])
        got[0].append(wav[1])
    for s in seqs:
        assert np.array_equal(np.concatenate(got[s]), clean[s]), f"slot {s}: a refused prime changed it"


def test_refused_primes_name_the_row_and_change_nothing(dev):
    body_refusals(dev)


# ============================================================================================ 4. real dims, once
def test_prime_at_real_dims_fp32(dev):
    """Released codec dims (window 72), fp32: references of 37 and 125 frames in one call, 8 generated frames in packets of 4."""
    from qwen3_tts_amd.codec import CodecDecoderEngine
    c, w = ss._real(dev, torch.float32)[0], ss._CACHE["real_w"][1]
    eng = CodecDecoderEngine(c, w, compute_dtype=torch.float32, device=dev, max_batch=2, max_frames=200)
    plan = ((1, 37), (0, 125))
    refs = {s: _seq(c, 500 + s, r) for s, r in plan}
    gens = {s: _seq(c, 510 + s, 8) for s, _ in plan}
    eng.stream_begin(2)
    eng.stream_prime_rows([1, 0], _block(c, [refs[1], refs[0]], 125, dev), [37, 125])
    got = push_all(eng, c, (1, 0), gens, dev, packets=(4,))
    for s, r in plan:
        whole = eng.forward(torch.cat([refs[s], gens[s]], dim=-1).to(dev)).cpu().numpy()[0, 0][r * c.total_upsample:]
        d = _rms(got[s], whole)
        print(f"real dims fp32, slot {s} behind {r} reference frames: rms against forward {d:.2e}")
        assert got[s].shape == whole.shape and d <= 1e-5 <= RMS_BAR, (s, d)


# ============================================================================================ 5. wrappers
TEXTS = ["hello world", "a rather longer sentence to speak", "hi", "one more request in the queue", "and another"]
REF_FRAMES = (4, 12, None, 23, 12)          # reference frames per request: one below the prime tail, None = x-vector only


def _tts(dev, kind, codec_batch=2, kv_pages=None, max_seq=128):
    """A tiny model of type `kind` ("base" | "voice_design"): talker of 2 rows, tiny codec, the stand-in tokenizer of
    tests/test_stream_slots_gpu.py"""
    from qwen3_tts_amd.model import Qwen3TTSForConditionalGeneration
    key = ("tts", kind, codec_batch)
    if key not in _CACHE:
        _CACHE[key] = ss._tts(dev, codec_batch)
    tts, c = _CACHE[key]
    t = synth.talker_tiny()
    cfgd = dict(synth.cfg_dict(t), tts_model_type=kind, tts_model_size="tiny", tokenizer_type="12hz")
    model = Qwen3TTSForConditionalGeneration(cfgd, _td(synth.talker_weights(t)), device=dev, dtype=torch.float32, max_batch=2, max_seq=max_seq,
                                             kv_pages=kv_pages)
    model.load_speech_tokenizer(tts.model.speech_tokenizer)
    return type(tts)(model, tts.processor, generate_defaults={}), c, t


def _prompts(t, ref_frames=REF_FRAMES):
    from qwen3_tts_amd.model import VoiceClonePromptItem
    g = np.random.default_rng(61)
    items = []
    for i, n in enumerate(ref_frames):
        emb = torch.from_numpy(g.standard_normal(t.hidden_size).astype(np.float32) * 0.1)
        code = None if n is None else torch.from_numpy(g.integers(0, t.cp_vocab_size, (n, t.num_code_groups)))
        items.append(VoiceClonePromptItem(ref_code=code, ref_spk_embedding=emb, x_vector_only_mode=n is None, icl_mode=n is not None,
                                          ref_text=None if n is None else f"reference text number {i}"))
    return items


def _collect(stream, n_req, up, sr, packet_frames):
    """per request: the streamed packets, and the indices of the packets that carried samples for it"""
    got, spans, n = [[] for _ in range(n_req)], [[] for _ in range(n_req)], -1
    for n, (packet, sr2) in enumerate(stream):
        assert sr2 == sr and len(packet) == n_req
        for i, p in enumerate(packet):
            assert p.dtype == np.float32 and p.ndim == 1 and p.shape[0] % up == 0 and p.shape[0] // up <= packet_frames
            if p.shape[0]:
                got[i].append(p)
                spans[i].append(n)
    return got, spans, n + 1


def _same_audio(tag, got, spans, whole, up):
    for i in range(len(whole)):
        cat = np.concatenate(got[i])
        d = _rms(cat, whole[i]) if cat.shape == whole[i].shape else float("nan")
        print(f"{tag}, request {i}: {cat.shape[0] // up} frames in packets {spans[i][0]}..{spans[i][-1]}, rms against the one-shot audio {d:.2e}")
        assert cat.shape == whole[i].shape and whole[i].shape[0] >= up, (tag, i, cat.shape, whole[i].shape)
        assert d <= 1e-5, (tag, i, d)


def body_stream_voice_clone(dev, schedules=(None, "refill", "continuous")):
    """`stream_voice_clone` on a tiny Base model of 2 rows: five texts, ICL prompts with references of 4, 12 and 23 frames and one
    x-vector-only request, a seed per request, packets of 3 frames.  Under every schedule a request's concatenated PCM has the length of
    `generate_voice_clone`'s for the same seeds and is within 1e-5 RMS of it; its array is empty while it is queued and after it has
    finished."""
    tts, c, t = _tts(dev, "base")
    up = c.total_upsample
    assert min(n for n in REF_FRAMES if n) < tts.model.speech_tokenizer.model.decoder.prime_tail_frames and len({n for n in REF_FRAMES if n}) >= 3
    kw = dict(language=["english", "chinese", "english", "chinese", "english"], voice_clone_prompt=_prompts(t), non_streaming_mode=False,
              max_new_tokens=[6, 11, 4, 9, 13], seed=[700 + i for i in range(5)])
    whole, sr = tts.generate_voice_clone(TEXTS, **kw)
    assert sr == 24000
    for schedule in schedules:
        got, spans, n_packets = _collect(tts.stream_voice_clone(TEXTS, packet_frames=3, schedule=schedule, **kw), len(TEXTS), up, sr, 3)
        _same_audio(f"schedule {schedule}", got, spans, whole, up)
        for i, s in enumerate(spans):
            assert s == list(range(s[0], s[-1] + 1)), (schedule, i, s)                   # empty before its start and after its end only
        assert sum(1 for s in spans if s[0] > 0) >= 3 and sum(1 for s in spans if s[-1] < n_packets - 1) >= 1, (schedule, spans)


def test_stream_voice_clone_equals_generate_voice_clone(dev):
    body_stream_voice_clone(dev)


def body_stream_voice_clone_pooled(dev, limits=(20, 30, 24, 28, 36), kv_pages=6, max_seq=96):
    """The same on a talker with a KV page pool small enough to preempt: a restarted request's slot is primed again before its frames
    are replayed, every request's PCM still equals the one-shot audio and has its sample count -- no sample is delivered twice."""
    tts, c, t = _tts(dev, "base", kv_pages=kv_pages, max_seq=max_seq)
    up = c.total_upsample
    kw = dict(language=["english"] * 5, voice_clone_prompt=_prompts(t), non_streaming_mode=False, max_new_tokens=list(limits),
              seed=[800 + i for i in range(5)])
    whole, sr = tts.generate_voice_clone(TEXTS, schedule="continuous", **kw)
    got, spans, _ = _collect(tts.stream_voice_clone(TEXTS, packet_frames=3, schedule="continuous", **kw), len(TEXTS), up, sr, 3)
    st = tts.model.talker.last_refill
    print(f"pooled voice clone: {st}")
    assert st["preemptions"] >= 1, st
    _same_audio("pooled", got, spans, whole, up)


def test_stream_voice_clone_survives_a_restart(dev):
    body_stream_voice_clone_pooled(dev)


def body_stream_voice_design(dev, schedule="refill"):
    """`stream_voice_design` against `generate_voice_design`, five texts on 2 rows under one schedule."""
    tts, c, t = _tts(dev, "voice_design")
    up = c.total_upsample
    kw = dict(language=["english", "chinese", "english", "chinese", "english"], non_streaming_mode=True, max_new_tokens=[6, 11, 4, 9, 13],
              seed=[900 + i for i in range(5)])
    instruct = ["a calm low voice", "bright and quick", "a calm low voice", "whispering", "bright and quick"]
    whole, sr = tts.generate_voice_design(TEXTS, instruct, schedule=schedule, **kw)
    got, spans, _ = _collect(tts.stream_voice_design(TEXTS, instruct, packet_frames=3, schedule=schedule, **kw), len(TEXTS), up, sr, 3)
    _same_audio(f"voice design, schedule {schedule}", got, spans, whole, up)


def test_stream_voice_design_equals_generate_voice_design(dev):
    body_stream_voice_design(dev)
