"""Opt-in FP8 (e4m3) weights for the talker's decode GEMMs on the MI355X: the hardware's code conversion against the table, the fp8
kernels bitwise against the bf16 kernels on d (the cases of tests/test_fp8_weights_hostemu.py), and the engine identity through the
Python classes -- `weight_format="fp8"` on W is, bit for bit, the bf16 engine on `fp8.effective_state_dict(W)`: greedy, sampled under
the continuous schedule with a KV page pool, at 1.7B dims, and through `from_pretrained`."""
import dataclasses

import numpy as np
import pytest
import torch

import fp8_cases
import synth
from test_gpu_parity import _suppress, _td, dev  # noqa: F401  (`dev` is a fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib(dev):
    from qwen3_tts_amd import load_library
    return fp8_cases.prototypes(load_library())


# ============================================================================================ the kernels
@pytest.mark.parametrize("case", fp8_cases.SKINNY2 + fp8_cases.SKINNY8, ids=lambda c: "x".join(map(str, c[:4])) + f"a{c[5]}")
def test_fp8_kernels_are_bitwise_the_bf16_kernels_on_d(lib, case):
    fp8_cases.check_case(lib, case, seed=sum(case))


def test_every_finite_code_through_each_conversion_path(lib):
    fp8_cases.all_codes_skinny2(lib)
    fp8_cases.all_codes_skinny8(lib, 16)
    fp8_cases.all_codes_skinny8(lib, 8)


# ============================================================================================ the engine
def _mid():
    return dataclasses.replace(synth.talker_tiny(), hidden_size=1024, intermediate_size=1024, num_attention_heads=8, num_key_value_heads=4)


_CFG = {"tiny": synth.talker_tiny, "mid": _mid}
_W = {}


def _weights(name):
    """(config, W, W_eff): built once per configuration, never modified."""
    if name not in _W:
        from qwen3_tts_amd import fp8
        t = _CFG[name]()
        w = _td(synth.talker_weights(t))
        _W[name] = (t, w, fp8.effective_state_dict(synth.cfg_dict(t), w))
    return _W[name]


def _pair(name, dev, **kw):
    from qwen3_tts_amd.talker import TalkerEngine
    t, w, weff = _weights(name)
    return (t, TalkerEngine(t, w, weight_dtype=torch.bfloat16, device=dev, weight_format="fp8", **kw),
            TalkerEngine(t, weff, weight_dtype=torch.bfloat16, device=dev, **kw))


def _same(a, b):
    for f in ("codes", "tokens", "hidden"):
        assert getattr(a, f) is not None and torch.equal(getattr(a, f), getattr(b, f)), f
    assert a.n_frames == b.n_frames


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("name,frames", [("tiny", 8), ("mid", 3)])
def test_fp8_engine_is_the_bf16_engine_of_the_effective_checkpoint_greedy(dev, name, frames, graph):
    t, e8, eb = _pair(name, dev, max_batch=4, max_seq=48, use_graph=graph)
    prompt = synth.rand_prompt(np.random.default_rng(31), t, [7, 4], 2, scale=0.5 if name == "tiny" else 0.05)
    kw = dict(max_new_tokens=frames + 1, min_new_tokens=frames + 1, suppress_tokens=_suppress(t), repetition_penalty=1.05,
              do_sample=False, subtalker_dosample=False, output_hidden_states=True)
    a, b = e8.generate(*prompt, **kw), eb.generate(*prompt, **kw)
    assert a.n_frames == frames
    _same(a, b)
    assert torch.equal(e8.debug_logits()[:2], eb.debug_logits()[:2])
    assert e8.packed_weight_bytes < eb.packed_weight_bytes and e8.weight_format == "fp8" and eb.weight_format is None


def test_fp8_engine_sampled_continuous_schedule_with_a_page_pool(dev):
    """Six sampled requests with their own seeds on four rows, `schedule="continuous"`, a KV page pool: bitwise equal as well."""
    t, e8, eb = _pair("tiny", dev, max_batch=4, max_seq=32, use_graph=True, kv_pages=8)
    lens, limits = [7, 4, 9, 5, 3, 8], [6, 9, 4, 8, 7, 5]
    prompt = synth.rand_prompt(np.random.default_rng(32), t, lens, 2, scale=0.5)
    kw = dict(max_new_tokens=limits, min_new_tokens=9, suppress_tokens=_suppress(t), repetition_penalty=1.05, do_sample=True, top_k=50,
              top_p=1.0, temperature=0.9, subtalker_dosample=True, subtalker_top_k=50, subtalker_top_p=1.0, subtalker_temperature=0.9,
              seed=[700 + i for i in range(6)], packet_frames=2, output_hidden_states=True)
    a, b = e8.generate(*prompt, schedule="continuous", **kw), eb.generate(*prompt, schedule="continuous", **kw)
    _same(a, b)
    assert e8.last_refill["pool_pages"] == 8 and e8.stats()["row_positions"] == 1


def _fake_ids(t, text):
    body = [(ord(ch) * 7) % 490 for ch in text][:40]
    a, n = 77, 198
    return torch.tensor([[t.im_start_token_id, a, n] + body + [t.im_end_token_id, n, t.im_start_token_id, a, n]])


@pytest.mark.parametrize("name", ["tiny", "mid"])
def test_fp8_model_class_generate_is_the_bf16_models_on_the_effective_checkpoint(dev, name):
    """`Qwen3TTSForConditionalGeneration(W, weight_format="fp8").generate` against the same class on `fp8.effective_state_dict(W)`: the
    codes and hidden rows of every request, bitwise -- greedy, sampled with a seed per request, and sampled under the continuous schedule
    (three requests on two rows).  On `mid` every talker GEMM of the frame step is skinny8_fp8_kernel, ACT_SWIGLU8 included."""
    from qwen3_tts_amd.model import Qwen3TTSForConditionalGeneration
    t, w, weff = _weights(name)
    cfgd = dict(synth.cfg_dict(t), tts_model_type="custom_voice", tts_model_size="tiny", tokenizer_type="12hz")
    kw = dict(device=dev, dtype=torch.bfloat16, max_batch=2, max_seq=96)
    m8 = Qwen3TTSForConditionalGeneration(cfgd, w, weight_format="fp8", **kw)
    mb = Qwen3TTSForConditionalGeneration(cfgd, weff, **kw)
    assert m8.talker.weight_format == "fp8" and mb.talker.weight_format is None
    ids = [_fake_ids(t, x) for x in ("hello world", "a rather longer request", "hi")]
    base = dict(input_ids=ids, languages=["english", "chinese", "english"], speakers=["vivian", "ryan", "vivian"], max_new_tokens=7)
    calls = [dict(do_sample=False, subtalker_dosample=False),
             dict(seed=[51, 52, 53]),
             dict(seed=[61, 62, 63], schedule="continuous")]
    frames = 0
    for extra in calls:
        (c8, h8), (cb, hb) = m8.generate(**base, **extra), mb.generate(**base, **extra)
        assert len(c8) == len(cb) == 3, extra
        for i in range(3):
            assert torch.equal(c8[i], cb[i]), (name, extra, i)
            assert (h8[i] is None) == (hb[i] is None) and (h8[i] is None or torch.equal(h8[i], hb[i])), (name, extra, i)
            frames += int(c8[i].shape[0])
    assert frames >= 9, frames


def test_fp8_engine_at_the_real_models_dims(dev):
    """1.7B dims (two layers' worth of the stack): the K = 2048 / 6144 instantiations inside the engine and its captured graph, batch 8."""
    from qwen3_tts_amd import fp8
    from qwen3_tts_amd.talker import TalkerEngine
    t = dataclasses.replace(synth.talker_17b(), num_hidden_layers=2, cp_num_hidden_layers=2)
    w = _td(synth.talker_weights(t, with_text=False))
    weff = fp8.effective_state_dict(synth.cfg_dict(t), w)
    prompt = synth.rand_prompt(np.random.default_rng(33), t, [6, 4, 7, 3, 5, 6, 2, 7], 1)
    kw = dict(max_new_tokens=5, min_new_tokens=5, suppress_tokens=_suppress(t), repetition_penalty=1.05, do_sample=False,
              subtalker_dosample=False, output_hidden_states=True)
    out = []
    for sd, fmt in ((w, "fp8"), (weff, None)):
        eng = TalkerEngine(t, sd, weight_dtype=torch.bfloat16, device=dev, max_batch=8, max_seq=32, use_graph=True, weight_format=fmt)
        out.append(eng.generate(*prompt, **kw))
        assert eng.stats()["graph_nodes"] > 0
        del eng
    assert out[0].n_frames == 4
    _same(*out)


def test_from_pretrained_with_fp8_weights_builds_and_generates(dev, golden_dir, tmp_path):
    """`Qwen3TTSModel.from_pretrained(dir, weight_format="fp8")` on tests/golden/ckpt_tiny with synth weights; the audio is that of the
    same directory holding the effective checkpoint (sampled, fixed seeds, through Qwen3TTSForConditionalGeneration.generate)."""
    from ckpt_util import make_tiny_checkpoint
    from qwen3_tts_amd import Qwen3TTSModel, fp8
    t = synth.talker_tiny()
    wn = synth.talker_weights(t)
    c = synth.codec_tiny()
    c.codebook_size = t.cp_vocab_size
    cw = synth.codec_weights(c)
    weff = fp8.effective_state_dict(synth.cfg_dict(t), _td(wn))
    kw = dict(device_map=dev, dtype=torch.bfloat16, max_batch=2, max_seq=96)
    tts8 = Qwen3TTSModel.from_pretrained(make_tiny_checkpoint(str(tmp_path / "w"), golden_dir, t, wn, c, cw), weight_format="fp8", **kw)
    ttsb = Qwen3TTSModel.from_pretrained(make_tiny_checkpoint(str(tmp_path / "weff"), golden_dir, t, weff, c, cw), **kw)
    assert tts8.model.talker.weight_format == "fp8" and ttsb.model.talker.weight_format is None
    gk = dict(text=["hello world", "a longer sentence"], speaker=["Vivian", "ryan"], language=["English", "Chinese"], max_new_tokens=8,
              seed=[41, 42])
    (w8, sr8), (wb, srb) = tts8.generate_custom_voice(**gk), ttsb.generate_custom_voice(**gk)
    assert sr8 == srb and len(w8) == 2
    for x, y in zip(w8, wb):
        assert x.shape[0] > 0 and np.array_equal(np.asarray(x), np.asarray(y))
    with pytest.raises(ValueError, match="bf16 engine"):
        Qwen3TTSModel.from_pretrained(str(tmp_path / "w"), weight_format="fp8", **dict(kw, dtype=torch.float32))
