"""GPU: `qtts_speaker_embed_ragged` -- reference clips of DIFFERENT lengths through the log-mel front end and the ECAPA-TDNN in one
launch sequence, packed row after row -- and the Python above it (`SpeakerEncoderEngine.embed_ragged / embed_many`, the voice-clone
wrappers).  The target is the reference's clip-by-clip loop: every clip's x-vector is what that clip gives alone.

The `body_*` functions take the device; tests/test_speaker_ragged_hostemu.py runs them on the host-emulation build.  All bars are the ones
this encoder already has: mels 2e-4 and embedding 1e-4 x max(1, largest component) against oracle/speaker_ref.py
(tests/test_hostemu.py::test_speaker_orchestration_embedding_vs_oracle), 1e-4 between a batched row and the clip alone and 2e-4 x max(1,
largest component) at the released dims (tests/test_gpu_parity.py::test_speaker_encoder_released_dims_vs_reference_golden), cosine 0.999
for the bf16 engine."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import synth
from test_gpu_parity import _td, dev  # noqa: F401  (`dev` is a fixture)

pytestmark = pytest.mark.gpu
# shortest legal clip | either side of a hop boundary | odd packed offsets | an equal pair | the longest
LENS = (1280, 1535, 1536, 6001, 4096, 4096, 8192)
MAX_BATCH, MAX_SAMPLES = 8, 8192
MARKER = -7.25
ARG, LIMIT = -1, -6          # include/qtts.h QTTS_ERR_ARG, QTTS_ERR_LIMIT
_CACHE = {}


def _clips(seed=9, lens=LENS):
    g = np.random.default_rng(seed)
    return [(g.standard_normal(n) * 0.2).clip(-1, 1).astype(np.float32) for n in lens]


def _engine(dev, dtype=torch.float32):
    key = ("eng", str(dev), dtype)
    if key not in _CACHE:
        from qwen3_tts_amd.speaker import SpeakerEncoderEngine
        c = synth.speaker_small()
        _CACHE[key] = SpeakerEncoderEngine(synth.cfg_dict(c), _td(synth.speaker_weights(c)), compute_dtype=dtype, device=dev,
                                           max_batch=MAX_BATCH, max_samples=MAX_SAMPLES)
    return _CACHE[key]


def _oracle():
    """per clip of `_clips()`: (log-mel (T_b, mel_dim), embedding (enc_dim,)) of oracle/speaker_ref.py, the clip alone; computed once"""
    if "oracle" not in _CACHE:
        import speaker_ref
        c = synth.speaker_small()
        w = _td(synth.speaker_weights(c))
        out = []
        with torch.no_grad():
            for clip in _clips():
                mel = speaker_ref.mel_spectrogram(torch.from_numpy(clip[None])).transpose(1, 2)
                out.append((mel[0].numpy(), speaker_ref.speaker_encoder_forward(w, c, mel)[0].numpy()))
        _CACHE["oracle"] = out
    return _CACHE["oracle"]


def _frames(eng, n):
    fr = C.c_int64()
    assert eng._lib.qtts_speaker_mel_frames(eng._h, n, C.byref(fr)) == 0
    return int(fr.value)


def _raw(eng, clips, lens=None, want_mels=True, emb=None):
    """The C entry point itself: (return code, embeddings (B, enc_dim), packed mels or None).  `lens` overrides the lengths passed (refusals)."""
    lens = [int(c.shape[0]) for c in clips] if lens is None else list(lens)
    B = len(lens)
    x = torch.from_numpy(np.concatenate(clips)).to(eng.device)
    n = (C.c_int32 * B)(*lens)
    if emb is None:
        emb = torch.full((B, eng.config.enc_dim), float("nan"), dtype=torch.float32, device=eng.device)
    mels = None
    if want_mels:
        mels = torch.full((sum(_frames(eng, k) for k in lens), eng.config.mel_dim), float("nan"), dtype=torch.float32, device=eng.device)
    with torch.cuda.device(eng.device):
        rc = eng._lib.qtts_speaker_embed_ragged(eng._h, C.c_void_p(x.data_ptr()), B, n, C.c_void_p(emb.data_ptr()),
                                                C.c_void_p(mels.data_ptr()) if want_mels else None,
                                                C.c_void_p(torch.cuda.current_stream(eng.device).cuda_stream))
    torch.cuda.synchronize()
    return rc, emb.cpu().numpy(), None if mels is None else mels.cpu().numpy()


def _solo(eng, clips):
    key = ("solo", id(eng))
    if key not in _CACHE:
        _CACHE[key] = [eng.embed(torch.from_numpy(c[None])).cpu().numpy()[0] for c in clips]
    return _CACHE[key]


# ============================================================================================ 1. against the oracle, clip by clip
def body_vs_oracle(dev):
    eng, clips, ref = _engine(dev), _clips(), _oracle()
    rc, emb, mels = _raw(eng, clips)
    assert rc == 0, eng._lib.qtts_last_error()
    assert np.isfinite(emb).all() and np.isfinite(mels).all()
    solo = _solo(eng, clips)
    t0 = 0
    for b, (mel_ref, emb_ref) in enumerate(ref):
        T = _frames(eng, LENS[b])
        assert T == mel_ref.shape[0], (b, T, mel_ref.shape)
        e_mel = float(np.abs(mels[t0:t0 + T] - mel_ref).max())
        e_emb = float(np.abs(emb[b] - emb_ref).max())
        e_solo = float(np.abs(emb[b] - solo[b]).max())
        print(f"clip {b} ({LENS[b]} samples, {T} frames): mels {e_mel:.2e}, embedding vs oracle {e_emb:.2e} "
              f"(largest component {float(np.abs(emb_ref).max()):.2f}), vs the clip alone {e_solo:.2e}")
        assert e_mel <= 2e-4, (b, e_mel)
        assert e_emb <= 1e-4 * max(1.0, float(np.abs(emb_ref).max())), (b, e_emb)
        assert e_solo <= 1e-4, (b, e_solo)
        t0 += T
    assert t0 == mels.shape[0]


def test_ragged_batch_equals_the_oracle_clip_by_clip(dev):
    body_vs_oracle(dev)


# ============================================================================================ 2. neighbours
def body_neighbours(dev):
    eng, clips = _engine(dev), _clips()
    rc, emb, _ = _raw(eng, clips, want_mels=False)
    assert rc == 0
    other = _clips(seed=123)
    for keep in (0, 3, 6):                                   # the shortest, the odd one, the longest (= last: nothing behind it)
        mixed = [clips[i] if i == keep else other[i] for i in range(len(clips))]
        rc, e2, _ = _raw(eng, mixed, want_mels=False)
        assert rc == 0 and np.array_equal(e2[keep], emb[keep]), keep
    solo = _solo(eng, clips)
    rc, rev, _ = _raw(eng, clips[::-1], want_mels=False)
    assert rc == 0 and np.isfinite(rev).all()
    for b in range(len(clips)):
        d = float(np.abs(rev[len(clips) - 1 - b] - solo[b]).max())
        assert d <= 1e-4, (b, d)
    for b in (0, 3):
        rc, one, _ = _raw(eng, [clips[b]], want_mels=False)
        assert rc == 0 and float(np.abs(one[0] - solo[b]).max()) <= 1e-4, b
    via_py = eng.embed_ragged(clips).cpu().numpy()
    assert np.array_equal(via_py, emb)


def test_a_clip_does_not_see_its_neighbours(dev):
    body_neighbours(dev)


# ============================================================================================ 3. bf16 engine
def body_bf16(dev):
    eng, clips, ref = _engine(dev, torch.bfloat16), _clips(), _oracle()
    rc, emb, mels = _raw(eng, clips)
    assert rc == 0 and np.isfinite(emb).all() and np.isfinite(mels).all()
    t0 = 0
    for b, (mel_ref, emb_ref) in enumerate(ref):
        T = mel_ref.shape[0]
        assert float(np.abs(mels[t0:t0 + T] - mel_ref).max()) <= 2e-4, b            # the mel front end stays fp32
        cos = float(np.dot(emb[b], emb_ref) / np.linalg.norm(emb[b]) / np.linalg.norm(emb_ref))
        print(f"bf16 clip {b}: cosine against the oracle {cos:.5f}")
        assert cos >= 0.999, (b, cos)
        t0 += T


def test_ragged_batch_bf16_engine(dev):
    body_bf16(dev)


# ============================================================================================ 4. refusals
def body_refusals(dev):
    eng, clips = _engine(dev), _clips()
    lib = eng._lib

    def refused(cl, lens, code, *words):
        emb = torch.full((len(lens), eng.config.enc_dim), MARKER, dtype=torch.float32, device=eng.device)
        rc, out, _ = _raw(eng, cl, lens=lens, want_mels=False, emb=emb)
        msg = (lib.qtts_last_error() or b"").decode()
        assert rc == code, (rc, msg)
        assert all(w in msg for w in words), msg
        assert (out == MARKER).all()

    short = [clips[0], clips[3], clips[4][:1279], clips[6]]                       # 1279 samples = 4 frames: the reference raises there too
    refused(short, [c.shape[0] for c in short], ARG, "clip 2", "1279")
    # a length above max_samples, in row 1 (the buffer really holds that many samples: nothing may be read anyway)
    long_ = [clips[0], np.zeros(MAX_SAMPLES + 1, np.float32), clips[2]]
    refused(long_, [c.shape[0] for c in long_], LIMIT, "clip 1", str(MAX_SAMPLES + 1))
    refused([clips[0], clips[1]], [1280, 0], LIMIT, "clip 1")
    nine = [clips[0]] * (MAX_BATCH + 1)
    refused(nine, [1280] * (MAX_BATCH + 1), LIMIT, str(MAX_BATCH + 1))
    with pytest.raises(ValueError):
        eng.embed_ragged([])
    rc, emb, _ = _raw(eng, clips, want_mels=False)                                # the engine is untouched by the refusals
    assert rc == 0 and float(np.abs(emb[3] - _solo(eng, clips)[3]).max()) <= 1e-4


def test_refused_batches_name_the_clip_and_change_nothing(dev):
    body_refusals(dev)


# ============================================================================================ 5. released dims, the reference's fixture
def test_released_dims_against_the_reference_fixture(dev, golden_dir):
    """The three clips of tests/golden/speaker_ragged.npz (tools/gen_golden_speaker_ragged.py: the reference's own Qwen3TTSSpeakerEncoder +
    mel_spectrogram, clip by clip) in ONE call at the released dims, fp32."""
    from qwen3_tts_amd.speaker import SpeakerEncoderEngine
    g = np.load(os.path.join(golden_dir, "speaker_ragged.npz"))
    c = synth.speaker_real()
    w = synth.speaker_weights(c)
    assert abs(synth.weights_checksum(w) - float(g["weights_checksum"])) < 1e-6
    lens = [int(n) for n in g["samples"]]
    clips = [synth.rand_audio(int(g["seed"]) + i, 1, n)[0] for i, n in enumerate(lens)]
    eng = SpeakerEncoderEngine(synth.cfg_dict(c), _td(w), compute_dtype=torch.float32, device=dev, max_batch=4, max_samples=max(lens))
    assert [_frames(eng, n) for n in lens] == [int(t) for t in g["frames"]]
    before = eng.embed_calls
    emb = eng.embed_ragged(clips).cpu().numpy()
    assert eng.embed_calls == before + 1 and emb.shape == g["embedding"].shape
    for b, n in enumerate(lens):
        ref = g["embedding"][b]
        err = float(np.abs(emb[b] - ref).max())
        print(f"released dims, clip {b} ({n} samples): max error {err:.3e} (largest component {float(np.abs(ref).max()):.2f})")
        assert err <= 2e-4 * max(1.0, float(np.abs(ref).max())), (b, err)


# ============================================================================================ 6. path and wrapper
def body_embed_many_paths(dev):
    eng, clips = _engine(dev), _clips()
    ten = clips + [clips[1], clips[5], clips[0]]                                  # ten clips of seven lengths
    n0 = eng.embed_calls
    many = [e.cpu().numpy() for e in eng.embed_many(ten)]
    assert eng.embed_calls == n0 + 2                                              # ceil(10 / 8) ragged calls, not seven buckets
    solo = _solo(eng, clips)
    for i, j in enumerate(list(range(7)) + [1, 5, 0]):
        assert float(np.abs(many[i] - solo[j]).max()) <= 1e-4, i
    same = [c[:4096] for c in _clips(seed=5, lens=(4096,) * 9)]
    n0 = eng.embed_calls
    got = eng.embed_many(same)
    assert eng.embed_calls == n0 + 2                                              # 8 + 1 rows through `embed`, as before
    a = eng.embed(torch.from_numpy(np.stack(same[:8]))).cpu().numpy()
    b = eng.embed(torch.from_numpy(np.stack(same[8:]))).cpu().numpy()
    assert np.array_equal(np.stack([e.cpu().numpy() for e in got]), np.concatenate([a, b]))


def test_embed_many_takes_the_ragged_path(dev):
    body_embed_many_paths(dev)


def _base_tts(dev):
    """the tiny Base-type model of tests/test_gpu_parity.py::test_wrapper_voice_clone_from_waveform_end_to_end: talker, speaker encoder, codec
    with its encoder (16 samples per code frame)"""
    import dataclasses
    from qwen3_tts_amd.codec import Qwen3TTSTokenizer
    from qwen3_tts_amd.model import Qwen3TTSForConditionalGeneration, Qwen3TTSModel
    t = synth.talker_tiny()
    G = t.num_code_groups
    c = synth.codec_tiny()
    c.codebook_size = t.cp_vocab_size
    enc = dataclasses.replace(synth.mimi_enc_small(), num_quantizers=G, encoder_valid_num_quantizers=G)
    spk = dataclasses.replace(synth.speaker_small(), enc_dim=t.hidden_size)
    sd = dict(synth.talker_weights(t))
    sd.update({"speaker_encoder." + k: v for k, v in synth.speaker_weights(spk).items()})
    tok_sd = dict(synth.codec_weights(c))
    tok_sd.update({"encoder." + k: v for k, v in synth.mimi_enc_weights(enc).items()})
    cfgd = dict(synth.cfg_dict(t), tts_model_type="base", tts_model_size="1b7", tokenizer_type="12hz", speaker_encoder_config=synth.cfg_dict(spk))
    tok_cfg = dict(synth.cfg_dict(c), encoder_config=synth.cfg_dict(enc), encoder_valid_num_quantizers=G,
                   encode_downsample_rate=enc.encode_downsample_rate, input_sample_rate=24000)
    model = Qwen3TTSForConditionalGeneration(cfgd, _td(sd), device=dev, dtype=torch.float32, max_batch=2, max_seq=128)
    model.load_speech_tokenizer(Qwen3TTSTokenizer.from_state_dict(tok_cfg, _td(tok_sd), device=dev, max_batch=3, max_frames=320))
    return Qwen3TTSModel(model, None, generate_defaults={}), model, t


def body_voice_clone_prompt(dev):
    tts, model, t = _base_tts(dev)
    g = np.random.default_rng(4)
    wavs = [(g.standard_normal(n) * 0.2).clip(-1, 1).astype(np.float32) for n in (2048, 1280, 1536)]
    model.extract_speaker_embedding(audio=wavs[0], sr=24000)                      # (builds the engine)
    n0 = model.speaker_encoder.embed_calls
    items = tts.create_voice_clone_prompt(ref_audio=[(w, 24000) for w in wavs], x_vector_only_mode=True)
    assert model.speaker_encoder.embed_calls == n0 + 1 and len(items) == 3        # three lengths, one speaker call
    for it, w in zip(items, wavs):
        own = model.extract_speaker_embedding(audio=w, sr=24000)
        assert it.ref_spk_embedding.shape == (t.hidden_size,)
        assert float((it.ref_spk_embedding.cpu() - own.cpu()).abs().max()) <= 1e-4


def test_create_voice_clone_prompt_embeds_ragged_clips_in_one_call(dev):
    body_voice_clone_prompt(dev)


# ============================================================================================ 7. binding
def body_binding():
    from qwen3_tts_amd import _lib
    lib = _lib.load_library()
    assert "qtts_speaker_embed_ragged" in _lib.SYMBOLS
    assert lib.qtts_speaker_embed_ragged.restype is C.c_int and len(lib.qtts_speaker_embed_ragged.argtypes) == 7
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "int qtts_speaker_embed_ragged(" in open(os.path.join(root, "include", "qtts.h")).read()


def test_the_entry_point_is_bound(dev):
    body_binding()
