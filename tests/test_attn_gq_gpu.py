"""The talker engine at head shapes beyond the released checkpoints' on the MI355X: GQA groups up to 8 and head_dim 64 through the
general decode attention (csrc/attn_gq.h), against fixtures the REFERENCE produced (tools/gen_golden_gq.py ->
tests/golden/talker_tiny_gq*.npz) and against the oracle at run time.  Same comparison rule as tests/test_gpu_parity.py: greedy codes bit
for bit, a cb-0 mismatch exempt only behind a reference margin below MARGIN_EXEMPT."""
import dataclasses
import os
import sys

import numpy as np
import pytest
import torch

import synth
import talker_ref
from qwen3_tts_amd import _lib as _qlib

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import gen_golden_gq  # noqa: E402  (the fixtures' configs; its reference imports are inside generate())

pytestmark = pytest.mark.gpu

MARGIN_EXEMPT = 1e-3
FIXTURES = sorted(gen_golden_gq.SHAPES)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from qwen3_tts_amd import load_library
    load_library()
    return "cuda:0"


def _td(w):
    return {k: torch.from_numpy(v) for k, v in w.items()}


def _suppress(t):
    return [i for i in range(t.vocab_size - 1024, t.vocab_size) if i != t.codec_eos_token_id]


def _compare_greedy(codes, tokens, g_codes, g_tokens, margin):
    n = min(codes.shape[1], g_codes.shape[1])
    for f in range(n + 1):
        if f < tokens.shape[1] and not np.array_equal(tokens[:, f], g_tokens[:, f]):
            bad = np.nonzero(tokens[:, f] != g_tokens[:, f])[0]
            assert (margin[bad, f] < MARGIN_EXEMPT).all(), f"token mismatch at step {f}, rows {bad.tolist()}, margins {margin[bad, f]}"
            print(f"low-margin flip at step {f}: comparison stops (exempt)")
            return f
        if f < n:
            assert np.array_equal(codes[:, f], g_codes[:, f]), f"sub-codebook mismatch in frame {f}"
    assert codes.shape[1] == g_codes.shape[1]
    return n


def _oracle(w, t, emb, mask, tr, pad, n, forced):
    sp = talker_ref.SamplingParams(do_sample=False, subtalker_dosample=False)
    trace = {}
    nthr = torch.get_num_threads()
    torch.set_num_threads(1)             # tiny tensors: the thread pool's hand-offs cost more than the arithmetic
    try:
        with torch.no_grad():
            r = talker_ref.talker_generate(w, t, emb, mask, tr, pad, max_new_tokens=n, min_new_tokens=n if forced else 2, sp=sp, trace=trace)
    finally:
        torch.set_num_threads(nthr)
    top2 = torch.topk(torch.stack(trace["scores"], 1), 2, dim=-1)[0]
    return r["codes"].numpy(), r["tokens"].numpy(), (top2[..., 0] - top2[..., 1]).numpy()


_FIX = {}


def _fixture(golden_dir, name):
    """One load / weight build per fixture for the whole module; nothing in it is modified."""
    if name not in _FIX:
        g = np.load(os.path.join(golden_dir, f"talker_tiny_{name}.npz"))
        t = gen_golden_gq.cfg(name)
        _FIX[name] = (g, t, _td(synth.talker_weights(t)), [torch.from_numpy(g[k]) for k in ("embeds", "mask", "trailing", "tts_pad")])
    return _FIX[name]


def _per_step(t):
    return t.num_hidden_layers + (t.num_code_groups - 1) * t.cp_num_hidden_layers


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("name", FIXTURES)
def test_other_head_shapes_fp32_vs_reference_golden(dev, golden_dir, name, graph):
    """The three fixtures in full (5 ragged rows x 39 frames x 16 codebooks), fp32, eager and captured: the reference's greedy codes."""
    from qwen3_tts_amd.talker import TalkerEngine
    g, t, w, args = _fixture(golden_dir, name)
    eng = TalkerEngine(t, w, weight_dtype=torch.float32, device=dev, max_batch=5, max_seq=64, use_graph=graph)
    out = eng.generate(*args, max_new_tokens=40, min_new_tokens=40, do_sample=False, subtalker_dosample=False, repetition_penalty=1.05,
                       suppress_tokens=_suppress(t))
    assert _compare_greedy(out.codes.cpu().numpy(), out.tokens.cpu().numpy(), g["codes"], g["tokens"], g["margin"]) == 39
    assert eng.stats()["attn_gq_per_step"] == _per_step(t)


def test_default_head_shape_through_the_general_family(dev, golden_dir):
    """QTTS_ATTN_GQ=1: every decode-attention launch of the default tiny config (4 / 2 / 128) runs attn_gq.h's kernels -- the codes are
    still those of tests/golden/talker_tiny.npz; without the option none does."""
    from qwen3_tts_amd.talker import TalkerEngine
    t = synth.talker_tiny()
    w = _td(synth.talker_weights(t))
    g = np.load(os.path.join(golden_dir, "talker_tiny.npz"))
    args = [torch.from_numpy(g[k]) for k in ("embeds", "mask", "trailing", "tts_pad")]
    kw = dict(max_new_tokens=14, min_new_tokens=2, do_sample=False, subtalker_dosample=False, repetition_penalty=1.05, suppress_tokens=_suppress(t))
    with _qlib.options(QTTS_ATTN_GQ="1"):
        eng = TalkerEngine(t, w, weight_dtype=torch.float32, device=dev, max_batch=4, max_seq=128, use_graph=True)
    out = eng.generate(*args, **kw)
    assert _compare_greedy(out.codes.cpu().numpy(), out.tokens.cpu().numpy(), g["codes"], g["tokens"], g["margin"]) == 13
    assert np.abs(out.hidden.cpu().numpy() - g["hidden"]).max() <= 1e-4
    assert eng.stats()["attn_gq_per_step"] == _per_step(t)
    off = TalkerEngine(t, w, weight_dtype=torch.float32, device=dev, max_batch=4, max_seq=128, use_graph=True)
    off.generate(*args, **kw)
    assert off.stats()["attn_gq_per_step"] == 0


def test_group_of_8_long_generation_crosses_window_and_split_kv_buckets(dev, golden_dir):
    """gq8_hd128, 290 forced frames against the oracle at run time (as test_talker_long_generation_crosses_kv_chunks): the KV length
    passes the register window (256 keys) and, with split-KV brought into range (from 100 keys, 64 keys per workgroup, up to 4
    workgroups), the 128-, 256- and 512-key buckets with their merge kernel."""
    from qwen3_tts_amd.talker import TalkerEngine
    g, t, w, args = _fixture(golden_dir, "gq8_hd128")
    N = 291
    rc, rt, margin = _oracle(w, t, *args, n=N, forced=True)
    assert np.array_equal(rc[:, :39], g["codes"])          # the oracle run continues the committed fixture
    with _qlib.options(QTTS_ATTN_NSPLIT="4", QTTS_ATTN_SPLIT_FROM="100", QTTS_ATTN_SPLIT_KEYS="64"):
        eng = TalkerEngine(t, w, weight_dtype=torch.float32, device=dev, max_batch=5, max_seq=320, use_graph=True)
        out = eng.generate(*args, max_new_tokens=N, min_new_tokens=N, do_sample=False, subtalker_dosample=False, suppress_tokens=_suppress(t))
    assert out.n_frames == N - 1
    st = eng.stats()
    assert st["long_graphs"] >= 2 and (st["attn_nsplit_last"], st["attn_span_last"]) == (4, 512), st
    oc = out.codes.cpu().numpy()
    diff = np.nonzero((oc != rc).any(axis=(0, 2)))[0]
    n = int(diff[0]) if diff.size else N - 1
    print(f"group of 8, long generation: {n} of {N - 1} frames bit-exact vs the oracle; min cb-0 margin {float(margin.min()):.2e}")
    # (the bar of the existing long-generation test: a wrong key past the window or in a split shows long before frame 200; a last-ulp
    # argmax tie may legitimately end a 290 x 16 x 5 greedy chain late)
    assert n >= 200, f"first mismatch at frame {n}"


def test_group_of_8_batch_20_two_m_tiles(dev, golden_dir):
    """gq8_hd128 at batch 20 (two m-tiles in the GEMMs, 20 / 40 rows through the attention), 6 frames against the oracle."""
    from qwen3_tts_amd.talker import TalkerEngine
    _, t, w, _ = _fixture(golden_dir, "gq8_hd128")
    lens = [3 + (7 * i) % 13 for i in range(20)]
    emb, mask, tr, pad = synth.rand_prompt(np.random.default_rng(9), t, lens, 2, scale=0.5)
    rc, rt, margin = _oracle(w, t, emb, mask, tr, pad, n=7, forced=False)
    eng = TalkerEngine(t, w, weight_dtype=torch.float32, device=dev, max_batch=20, max_seq=64, use_graph=True)
    out = eng.generate(emb, mask, tr, pad, max_new_tokens=7, do_sample=False, subtalker_dosample=False, suppress_tokens=_suppress(t))
    assert _compare_greedy(out.codes.cpu().numpy(), out.tokens.cpu().numpy(), rc, rt, margin) == 6


@pytest.mark.parametrize("name", FIXTURES)
def test_other_head_shapes_bf16(dev, golden_dir, name):
    """bf16 engines (the talker's attention on the matrix pipe, transposed V pages): eager == captured graph bit for bit, two runs
    bit-identical, and the first two frames agree with the fp32 golden at >= 0.7 (the bar of test_talker_large_batch_paths)."""
    from qwen3_tts_amd.talker import TalkerEngine
    g, t, w, args = _fixture(golden_dir, name)
    kw = dict(max_new_tokens=12, min_new_tokens=12, do_sample=False, subtalker_dosample=False, suppress_tokens=_suppress(t))
    res = []
    for graph in (False, True):
        eng = TalkerEngine(t, w, weight_dtype=torch.bfloat16, device=dev, max_batch=5, max_seq=64, use_graph=graph)
        res.append(eng.generate(*args, **kw).codes.cpu().numpy())
        res.append(eng.generate(*args, **kw).codes.cpu().numpy())
        assert eng.stats()["attn_gq_per_step"] == _per_step(t)
        del eng
    assert all(np.array_equal(res[0], r) for r in res[1:]), "bf16 decode differs between eager / graph or between two runs"
    agree = float((res[0][:, :2] == g["codes"][:, :2]).mean())
    print(f"{name} bf16 vs the fp32 golden, first 2 frames: {agree:.2f}")
    assert agree >= 0.7


def test_real_code_predictor_keeps_its_fused_launches_when_the_talker_heads_change(dev):
    """0.6B dims with 2 talker layers and talker heads 16 / 2 / 128 (a group of 8); the code predictor stays 16 / 8 / 128.  bf16, batch 8,
    captured, 10 frames: the code predictor's fused launches are exactly those of the unmodified head shape, the talker's layers run
    the general attention, two runs are bit-identical; the fp32 engine matches the oracle."""
    from qwen3_tts_amd.talker import TalkerEngine
    base = dataclasses.replace(synth.talker_06b(), num_hidden_layers=2)
    t = dataclasses.replace(base, num_key_value_heads=2)
    kw = dict(max_new_tokens=11, min_new_tokens=11, do_sample=False, subtalker_dosample=False)
    lens = [20 + 3 * i for i in range(8)]
    counters = {}
    for tag, cfg in (("base", base), ("gq8", t)):
        w = _td(synth.talker_weights(cfg, with_text=False))
        emb, mask, tr, pad = synth.rand_prompt(np.random.default_rng(3), cfg, lens, 4, scale=0.05)
        eng = TalkerEngine(cfg, w, weight_dtype=torch.bfloat16, device=dev, max_batch=8, max_seq=128, use_graph=True)
        a = eng.generate(emb, mask, tr, pad, suppress_tokens=_suppress(cfg), **kw).codes.cpu().numpy()
        b = eng.generate(emb, mask, tr, pad, suppress_tokens=_suppress(cfg), **kw).codes.cpu().numpy()
        assert a.shape[1] == 10 and np.array_equal(a, b), tag
        counters[tag] = eng.stats()
        del eng
    for k in ("cp_fused_per_step", "cp_mlp_per_step", "cp_layer_per_step"):
        assert counters["gq8"][k] == counters["base"][k], (k, counters["gq8"][k], counters["base"][k])
    assert counters["base"]["cp_fused_per_step"] > 0
    assert counters["gq8"]["attn_gq_per_step"] == t.num_hidden_layers and counters["base"]["attn_gq_per_step"] == 0
    rc, rt, margin = _oracle(w, t, emb, mask, tr, pad, n=11, forced=True)
    e32 = TalkerEngine(t, w, weight_dtype=torch.float32, device=dev, max_batch=8, max_seq=128, use_graph=True)
    out = e32.generate(emb, mask, tr, pad, suppress_tokens=_suppress(t), **kw)
    assert _compare_greedy(out.codes.cpu().numpy(), out.tokens.cpu().numpy(), rc, rt, margin) == 10
