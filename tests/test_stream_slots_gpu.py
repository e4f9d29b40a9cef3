"""Audio streamed per request from the refill schedule: per-slot state of the codec's state-carrying decoder (include/qtts.h
qtts_codec_stream_reset_rows / qtts_codec_stream_push_rows), `TalkerEngine.generate_stream(..., schedule="refill")` and
`Qwen3TTSModel.stream_custom_voice(..., schedule="refill")`.

After `stream_begin(B)` the codec handle owns B slots, each with its own carries and its own position; a push decodes a packet for
any subset of them.  Every sequence that ever occupied a slot must come out as the whole-sequence `forward` of that sequence alone,
whatever ran next to it, whatever ran in its slot before it, and wherever its neighbours stood in their own streams.

The test BODIES (`body_*`) take the device; tests/test_stream_slots_hostemu.py runs the same bodies on the host-emulation build."""
import numpy as np
import pytest
import torch

import codec_ref
import synth
from test_gpu_parity import RMS_BAR, _rms, _suppress, _td, dev  # noqa: F401  (`dev` is a fixture)
from test_row_sampling_gpu import _np
import test_refill_gpu as rg

pytestmark = pytest.mark.gpu
gga = rg.gga
PACKETS = (1, 4, 2, 7)          # cycled: a single frame, and n >= W1 = 7 of the tiny codec
# (name, slot, frames, first push): the full schedule on 4 slots.  A and B run from the first push, E ends in the second, C enters at the
# third, B ends in the fourth and D takes its slot -- reset -- at the seventh; pushes 12 and 13 carry D alone (M = 1).  A passes frame 7
# in the fourth push, when C is at frame 2; D starts when A is at frame 19.
FULL = (("A", 2, 40, 0), ("B", 0, 9, 0), ("E", 1, 3, 0), ("C", 3, 17, 2), ("D", 0, 26, 6))
# the emulator's schedule, 3 slots: Z ends in the second push; Y takes its slot -- reset -- at the fourth, the push in which X passes
# frame 7, and runs on alone
REDUCED = (("X", 2, 12, 0), ("Z", 0, 2, 0), ("Y", 0, 9, 3))
ORDER = (3, 2, 0, 1)            # rows are listed in this order: [2, 0, 1], [3, 2, 0], ...
_CACHE = {}


def _tiny(dev):
    """(config, weights, fp32 engine with max_batch 4 and max_frames 64): built once and shared"""
    if "tiny" not in _CACHE:
        from qwen3_tts_amd.codec import CodecDecoderEngine
        c = synth.codec_tiny()
        w = _td(synth.codec_weights(c))
        _CACHE["tiny"] = (c, w, CodecDecoderEngine(c, w, compute_dtype=torch.float32, device=dev, max_batch=4, max_frames=64))
    return _CACHE["tiny"]


def _codes(c, plan, seed):
    rng = np.random.default_rng(seed)
    return {name: torch.from_numpy(rng.integers(0, c.codebook_size, (1, c.num_quantizers, T))) for name, _, T, _ in plan}


def run_schedule(eng, c, plan, codes, n_slots, dev, packets=PACKETS, order=ORDER):
    """Drive `stream_begin / stream_reset_rows / stream_push_rows` through `plan`; returns ({name: PCM (samples,)}, [ids of each push]).
    A sequence whose remainder is shorter than the packet is padded with code 0 and its surplus samples are dropped."""
    up = c.total_upsample
    eng.stream_begin(n_slots)
    pos = {name: 0 for name, *_ in plan}
    out = {name: [] for name, *_ in plan}
    pushes, p = [], 0
    while any(pos[name] < T for name, _, T, _ in plan):
        n = packets[p % len(packets)]
        live = {slot: (name, T) for name, slot, T, start in plan if start <= p and pos[name] < T}
        assert len(live) == sum(1 for name, slot, T, start in plan if start <= p and pos[name] < T), "two sequences in one slot"
        starting = [slot for slot, (name, _) in live.items() if pos[name] == 0]
        if starting:
            eng.stream_reset_rows(starting)
        ids = [s for s in order if s in live]
        batch = torch.zeros(len(ids), c.num_quantizers, n, dtype=torch.long)
        for m, s in enumerate(ids):
            name, T = live[s]
            k = min(n, T - pos[name])
            batch[m, :, :k] = codes[name][0, :, pos[name]:pos[name] + k]
        wav = eng.stream_push_rows(ids, batch.to(dev))[:, 0].cpu().numpy()
        assert wav.shape == (len(ids), n * up)
        for m, s in enumerate(ids):
            name, T = live[s]
            k = min(n, T - pos[name])
            out[name].append(wav[m, :k * up].copy())
            pos[name] += k
        pushes.append(ids)
        p += 1
    return {name: np.concatenate(parts) for name, parts in out.items()}, pushes


# ============================================================================================ 1. codec at the ABI, tiny dims
def body_codec_slots(dev, plan, n_slots, keep):
    """Every sequence of the schedule: exact sample count, the engine's whole-sequence forward of that sequence alone within 1e-5 RMS
    and the oracle within RMS_BAR (the bars of test_codec_incremental_stream_equals_forward).  Then the same schedule with every
    sequence not in `keep` replaced by other codes -- the neighbours, and the earlier occupant of the re-used slot: the kept
    sequences' PCM is bit-identical (same launch shapes: only cross-talk or a missed reset can differ).  Two identical runs are
    bit-identical."""
    c, w, eng = _tiny(dev)
    codes = _codes(c, plan, 21)
    got, pushes = run_schedule(eng, c, plan, codes, n_slots, dev)
    assert any(ids != sorted(ids) for ids in pushes) and len(pushes[-1]) == 1, pushes
    for name, _, T, _ in plan:
        assert got[name].shape == (T * c.total_upsample,), name
        alone = eng.forward(codes[name].to(dev)).cpu().numpy()[0, 0]
        with torch.no_grad():
            ref = codec_ref.decoder_forward(w, c, codes[name]).numpy()[0, 0]
        d_fwd, d_ref = _rms(got[name], alone), _rms(got[name], ref)
        print(f"sequence {name} ({T} frames): rms against forward {d_fwd:.2e}, against the oracle {d_ref:.2e}")
        assert d_fwd <= 1e-5 and d_ref <= RMS_BAR, (name, d_fwd, d_ref)
    other = dict(_codes(c, plan, 22), **{k: codes[k] for k in keep})
    assert all(not torch.equal(other[name], codes[name]) for name, *_ in plan if name not in keep)
    swapped, _ = run_schedule(eng, c, plan, other, n_slots, dev)
    for k in keep:
        assert np.array_equal(swapped[k], got[k]), f"{k}: disturbed by its neighbours or by the earlier occupant of its slot"
    again, _ = run_schedule(eng, c, plan, codes, n_slots, dev)
    for name in got:
        assert np.array_equal(again[name], got[name]), name


def test_slots_decode_side_by_side_and_equal_forward(dev):
    body_codec_slots(dev, FULL, 4, ("A", "D"))


def body_lockstep_equals_stream_push(dev, B=2, T=10):
    """All slots reset together and pushed as [0..B): the bits of `stream_push` (which is that push)."""
    c, w, eng = _tiny(dev)
    codes = torch.from_numpy(np.random.default_rng(23).integers(0, c.codebook_size, (B, c.num_quantizers, T)))
    cuts = [0, 1, 5, 7, T]
    eng.stream_begin(B)
    a = [eng.stream_push(codes[..., i:j].to(dev)).cpu().numpy() for i, j in zip(cuts[:-1], cuts[1:])]
    eng.stream_begin(B)
    eng.stream_push_rows(list(range(B)), codes[..., :3].to(dev))             # something to reset
    eng.stream_reset_rows(list(range(B)))
    b = [eng.stream_push_rows(list(range(B)), codes[..., i:j].to(dev)).cpu().numpy() for i, j in zip(cuts[:-1], cuts[1:])]
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def test_lockstep_rows_equal_stream_push(dev):
    body_lockstep_equals_stream_push(dev)


# ============================================================================================ 2. codec at real dims
REAL = (("P", 2, 90, 0), ("Q", 0, 20, 0), ("R", 0, 75, 5))          # packets of 4: Q ends in push 4, R takes its slot -- reset -- at push 5


def _real(dev, dtype):
    from qwen3_tts_amd.codec import CodecDecoderEngine
    if "real_w" not in _CACHE:
        c = synth.codec_real()
        _CACHE["real_w"] = (c, _td(synth.codec_weights(c)))
    c, w = _CACHE["real_w"]
    return c, CodecDecoderEngine(c, w, compute_dtype=dtype, device=dev, max_batch=4, max_frames=64)


def test_slots_at_real_dims_fp32(dev):
    """Released codec dims (window 72: W1 = 71), fp32: P passes frame 71 while R, admitted into Q's reset slot, is inside its first 71.
    Per sequence against the engine's whole-sequence forward, <= RMS_BAR."""
    c, eng = _real(dev, torch.float32)
    codes = _codes(c, REAL, 31)
    got, pushes = run_schedule(eng, c, REAL, codes, 3, dev, packets=(4,), order=(2, 0, 1))
    assert len(pushes[-1]) == 1
    for name, _, T, _ in REAL:
        d = _rms(got[name], eng.forward(codes[name].to(dev)).cpu().numpy()[0, 0])
        print(f"real dims fp32, sequence {name} ({T} frames): rms against forward {d:.2e}")
        assert got[name].shape == (T * c.total_upsample,) and d <= RMS_BAR, (name, d)


def test_slots_at_real_dims_bf16(dev):
    """bf16: no absolute bar is known, so the yardstick is measured here: the distance between the lockstep `stream_push` of each
    sequence alone (B = 1, same packets) and the bf16 `forward`.  The slot path must be within 1.5 x of it -- the margin covers tile
    choices that differ with M; a state error (wrong position, wrong padding, a missed reset) is orders of magnitude larger.
    Measured on an MI355X: both distances 6.2e-03 ... 6.3e-03 per sequence, ratio 1.000 (profiles/stream_refill.md)."""
    c, eng = _real(dev, torch.bfloat16)
    codes = _codes(c, REAL, 31)
    got, _ = run_schedule(eng, c, REAL, codes, 3, dev, packets=(4,), order=(2, 0, 1))
    for name, _, T, _ in REAL:
        whole = eng.forward(codes[name].to(dev)).cpu().numpy()[0, 0]
        eng.stream_begin(1)
        alone = np.concatenate([eng.stream_push(codes[name][..., i:i + 4].to(dev)).cpu().numpy()[0, 0] for i in range(0, T, 4)])
        d_lock, d_slot = _rms(alone, whole), _rms(got[name], whole)
        print(f"real dims bf16, sequence {name} ({T} frames): rms against forward: lockstep alone {d_lock:.3e}, slot path {d_slot:.3e}, "
              f"ratio {d_slot / d_lock:.3f}")
        assert got[name].shape == whole.shape and d_lock > 0 and d_slot <= 1.5 * d_lock, (name, d_slot, d_lock)


# ============================================================================================ 3. talker: generate_stream(schedule="refill")
def body_talker_refill_stream(dev, golden_dir, graph):
    """The 24 requests of tests/golden/talker_tiny_admit.npz on 4 rows, greedy, packets of 3 frames: each request's packets concatenate
    to exactly the reference's codes for it, and to what `generate(schedule="refill")` returns; `first` and `last` occur once per
    request, no request has two rows and no row two occupants at a time.  Closing the generator after the second packet leaves the
    engine usable."""
    g, t, w, args = rg._fixture(golden_dir)
    eng = rg._engine(t, w, dev, torch.float32, graph, 4, 128)
    kw = dict(max_new_tokens=gga.LIMITS, min_new_tokens=gga.MAX_NEW, do_sample=False, subtalker_dosample=False, repetition_penalty=gga.REP,
              suppress_tokens=_suppress(t))
    parts = {i: [] for i in range(gga.N_REQ)}
    first, last, row_of, occupant, n_packets = {}, {}, {}, {}, 0
    for packet in eng.generate_stream(*args, schedule="refill", packet_frames=3, **kw):
        n_packets += 1
        for e in packet.rows:
            assert e.codes.shape[0] <= 3 and e.codes.shape[1] == t.num_code_groups and e.request not in last
            assert (e.request not in first) == e.first, e.request
            if e.first:
                first[e.request] = n_packets
                assert occupant.get(e.row) is None, (e.row, occupant.get(e.row), e.request)
                occupant[e.row] = e.request
            assert row_of.setdefault(e.request, e.row) == e.row and occupant[e.row] == e.request
            assert e.codes.shape[0] > 0 or e.last
            parts[e.request].append(_np(e.codes))
            if e.last:
                last[e.request] = n_packets
                occupant[e.row] = None
    streamed_stats = dict(eng.last_refill)
    assert sorted(first) == sorted(last) == list(range(gga.N_REQ)) and max(first.values()) > 1
    assert streamed_stats["admitted_rows"] >= 1 and streamed_stats["admitted_rows"] + 4 * streamed_stats["streams"] == gga.N_REQ, streamed_stats
    whole = _np(eng.generate(*args, schedule="refill", packet_frames=3, **kw).codes)
    for i, L in enumerate(gga.LIMITS):
        cat = np.concatenate(parts[i])
        rg._check_request(g, t, cat, i, L)
        assert np.array_equal(cat, whole[i, :L - 1]) and (whole[i, L - 1:, 0] == t.codec_eos_token_id).all(), i
    gen = eng.generate_stream(*args, schedule="refill", packet_frames=3, **kw)
    next(gen), next(gen)
    gen.close()
    assert eng.last_refill["streams"] == 1 and eng.last_refill["frames_run"] >= 1
    fresh = eng.generate(*[a[:4] for a in args[:3]], args[3], max_new_tokens=[3] * 4, min_new_tokens=gga.MAX_NEW, do_sample=False,
                         subtalker_dosample=False, repetition_penalty=gga.REP, suppress_tokens=_suppress(t))
    assert np.array_equal(_np(fresh.codes)[:, :2], g["codes"][:4, :2])


@pytest.mark.parametrize("graph", [False, True])
def test_refill_stream_packets_concatenate_to_the_reference_codes(dev, golden_dir, graph):
    body_talker_refill_stream(dev, golden_dir, graph)


# ============================================================================================ 4. wrapper
def _tts(dev, codec_batch):
    from qwen3_tts_amd.codec import Qwen3TTSTokenizer
    from qwen3_tts_amd.model import Qwen3TTSForConditionalGeneration, Qwen3TTSModel
    t = synth.talker_tiny()
    c = synth.codec_tiny()
    c.codebook_size = t.cp_vocab_size                 # codec codebooks must cover the talker's code range
    cfgd = dict(synth.cfg_dict(t), tts_model_type="custom_voice", tts_model_size="1b7", tokenizer_type="12hz")
    model = Qwen3TTSForConditionalGeneration(cfgd, _td(synth.talker_weights(t)), device=dev, dtype=torch.float32, max_batch=2, max_seq=128)
    model.load_speech_tokenizer(Qwen3TTSTokenizer.from_state_dict(synth.cfg_dict(c), _td(synth.codec_weights(c)), device=dev,
                                                                  max_batch=codec_batch, max_frames=64))

    class FakeProcessor:                               # deterministic stand-in for the HF text tokenizer
        def __call__(self, text=None, return_tensors="pt", padding=True):
            body = [(ord(ch) * 7) % 490 for ch in text if ch not in "<|>_\\n"][:40]
            a, n = 77, 198
            if text.startswith("<|im_start|>user"):
                ids = [t.im_start_token_id] + body + [t.im_end_token_id, n]
            else:
                ids = [t.im_start_token_id, a, n] + body + [t.im_end_token_id, n, t.im_start_token_id, a, n]
            return {"input_ids": torch.tensor([ids])}
    return Qwen3TTSModel(model, FakeProcessor(), generate_defaults={}), c


def body_wrapper_refill_stream(dev):
    """`stream_custom_voice(schedule="refill")`: 6 texts on a talker of 2 rows, sampling with a seed per request.  Per request the
    streamed audio has the sample count of `generate_custom_voice(schedule="refill", seed=...)` and is within 1e-5 RMS of it (the bar
    of the ABI check: streamed == whole-sequence forward); a request's array is empty before its start and after its end.  Without
    `schedule` 6 > 2 requests are refused as before; a codec with fewer slots than the talker has rows is refused."""
    tts, c = _tts(dev, 2)
    texts = ["hello world", "a rather longer sentence to speak", "hi", "one more request in the queue", "and another", "the sixth text"]
    spk, langs = ["vivian", "ryan"] * 3, ["english", "chinese"] * 3
    kw = dict(language=langs, non_streaming_mode=False, max_new_tokens=[6, 11, 4, 9, 13, 7], seed=[500 + i for i in range(6)])
    whole, sr = tts.generate_custom_voice(texts, spk, schedule="refill", **kw)
    up = c.total_upsample
    got, spans = [[] for _ in texts], [[] for _ in texts]
    for n, (packet, sr2) in enumerate(tts.stream_custom_voice(texts, spk, packet_frames=3, schedule="refill", **kw)):
        assert sr2 == sr == 24000 and len(packet) == len(texts)
        for i, p in enumerate(packet):
            assert p.dtype == np.float32 and p.ndim == 1 and p.shape[0] % up == 0 and p.shape[0] // up <= 3
            if p.shape[0]:
                got[i].append(p)
                spans[i].append(n)
    n_packets = n + 1
    for i in range(len(texts)):
        cat = np.concatenate(got[i])
        d = _rms(cat, whole[i]) if cat.shape == whole[i].shape else float("nan")
        print(f"request {i}: {cat.shape[0] // up} frames in packets {spans[i][0]}..{spans[i][-1]} of {n_packets}, rms against the one-shot audio {d:.2e}")
        assert cat.shape == whole[i].shape and whole[i].shape[0] >= up, (i, cat.shape, whole[i].shape)
        assert d <= 1e-5, (i, d)
        assert spans[i] == list(range(spans[i][0], spans[i][-1] + 1)), (i, spans[i])           # empty before its start and after its end only
    assert sum(1 for s in spans if s[0] > 0) >= 4 and sum(1 for s in spans if s[-1] < n_packets - 1) >= 1, spans
    assert tts.model.talker.last_refill["admitted_rows"] >= 1
    with pytest.raises(ValueError, match="exceed max_batch 2"):
        list(tts.stream_custom_voice(texts, spk, packet_frames=3, **kw))
    small, _ = _tts(dev, 1)
    with pytest.raises(ValueError, match=r"max_batch \(1\) is smaller than the talker's \(2\)"):
        list(small.stream_custom_voice(texts, spk, packet_frames=3, schedule="refill", **kw))


def test_stream_custom_voice_takes_the_refill_schedule(dev):
    body_wrapper_refill_stream(dev)
