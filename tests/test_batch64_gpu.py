"""Talker batches of 33..64 rows on the MI355X: the engine at 40 and 64 rows against the fixtures the REFERENCE produced
(tools/gen_golden_b64.py), batch invariance, the 65..128-row decode GEMM against its two-launch fallback (QTTS_SKINNY_WIDE=0) at tiny
and at the released code predictor's dims, and the limits.  The same checks run on the CPU emulator in tests/test_batch64_hostemu.py."""
import dataclasses
import os
import sys

import numpy as np
import pytest
import torch

import synth
from qwen3_tts_amd import _lib as _qlib

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import gen_golden_b64  # noqa: E402  (the fixtures' prompt; its reference imports are inside generate())

pytestmark = pytest.mark.gpu
MARGIN_EXEMPT = 1e-3
PER_STEP = ("cp_fused_per_step", "cp_mlp_per_step", "cp_layer_per_step", "ks_split_per_step", "attn_gq_per_step", "graph_nodes")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from qwen3_tts_amd import load_library
    load_library()          # the product path must be the HIP library: fail loudly if it is missing
    return "cuda:0"


@pytest.fixture(scope="module")
def tiny():
    t = synth.talker_tiny()
    return t, {k: torch.from_numpy(v) for k, v in synth.talker_weights(t, with_text=False).items()}


def _suppress(t):
    return [i for i in range(t.vocab_size - 1024, t.vocab_size) if i != t.codec_eos_token_id]


def _engine(t, w, dev, dtype, max_batch, max_seq=64):
    from qwen3_tts_amd.talker import TalkerEngine
    return TalkerEngine(t, w, weight_dtype=dtype, device=dev, max_batch=max_batch, max_seq=max_seq, use_graph=True)


def _greedy(eng, t, args, n, **kw):
    out = eng.generate(*args, max_new_tokens=n, min_new_tokens=n, do_sample=False, subtalker_dosample=False, suppress_tokens=_suppress(t), **kw)
    return out.codes.cpu().numpy(), out.tokens.cpu().numpy(), out.hidden.cpu().numpy()


def _compare_greedy(codes, tokens, g_codes, g_tokens, margin):
    """The rule of tests/test_gpu_parity.py: bit-exact; a cb-0 mismatch is exempt only behind a reference margin below MARGIN_EXEMPT,
    and the comparison stops there.  Returns the number of compared frames."""
    n = min(codes.shape[1], g_codes.shape[1])
    for f in range(n + 1):
        if f < tokens.shape[1] and not np.array_equal(tokens[:, f], g_tokens[:, f]):
            bad = np.nonzero(tokens[:, f] != g_tokens[:, f])[0]
            assert (margin[bad, f] < MARGIN_EXEMPT).all(), f"token mismatch at step {f}, rows {bad.tolist()}, margins {margin[bad, f]}"
            return f
        if f < n:
            assert np.array_equal(codes[:, f], g_codes[:, f]), f"sub-codebook mismatch in frame {f}"
    return n


def _fixture(golden_dir, name):
    g = np.load(os.path.join(golden_dir, f"talker_tiny_{name}.npz"))
    assert float(g["margin"].min()) >= MARGIN_EXEMPT
    return g, list(gen_golden_b64.prompt(name))


@pytest.mark.parametrize("name", ["b64", "b40"])
def test_fp32_64_and_40_rows_vs_reference(tiny, dev, golden_dir, name):
    """fp32, captured frame graph, 64 and 40 ragged rows (pass 0 of the code predictor: 128 / 80 rows through the fp32 kernel's 8-tile
    form): all 9 frames of the REFERENCE's greedy run, bit for bit -- no margin of these fixtures lets the comparison stop early."""
    t, w = tiny
    g, args = _fixture(golden_dir, name)
    B = g["codes"].shape[0]
    eng = _engine(t, w, dev, torch.float32, B)
    codes, tokens, _ = _greedy(eng, t, args, 10)
    assert codes.shape == (B, 9, 16)
    assert _compare_greedy(codes, tokens, g["codes"], g["tokens"], g["margin"]) == 9
    assert eng.stats()["graph_nodes"] > 100


def test_bf16_64_rows_tracks_the_fp32_reference(tiny, dev, golden_dir):
    """bf16 at 64 rows against the fp32 fixture: the first two frames' codes agree in at least 0.7 of the positions (the bound
    test_talker_large_batch_paths uses at 20 rows)."""
    t, w = tiny
    g, args = _fixture(golden_dir, "b64")
    codes, _, _ = _greedy(_engine(t, w, dev, torch.bfloat16, 64), t, args, 4)
    agree = float((codes[:, :2] == g["codes"][:, :2]).mean())
    print(f"B=64 bf16 agreement (first 2 frames) {agree:.3f}")
    assert agree >= 0.7


@pytest.mark.parametrize("B", [40, 64])
def test_bf16_one_call_equals_two_half_calls(tiny, dev, B):
    """bf16, greedy, 6 tokens: B = 40 (64) rows in one call give exactly the codes of two calls of 20 (32) rows with the same left
    padding (the last row of each half is the longest prompt).  ks-split regroups fp32 sums at 17..32 rows: off."""
    t, w = tiny
    lens = ([3 + (5 * i) % 11 for i in range(B // 2 - 1)] + [15]) * 2
    e, m, tr, pad = synth.rand_prompt(np.random.default_rng(70 + B), t, lens, 2, scale=0.5)
    with _qlib.options(QTTS_SKINNY_KS="0"):
        eng = _engine(t, w, dev, torch.bfloat16, B)
    whole, wtok, _ = _greedy(eng, t, (e, m, tr, pad), 6)
    assert whole.shape == (B, 5, 16)
    for half in (slice(0, B // 2), slice(B // 2, B)):
        part, ptok, _ = _greedy(eng, t, (e[half], m[half], tr[half], pad), 6)
        assert np.array_equal(part, whole[half]) and np.array_equal(ptok, wtok[half])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_skinny_wide_option_changes_nodes_not_results(tiny, dev, golden_dir, dtype):
    """QTTS_SKINNY_WIDE on against off at 40 rows: codes and hidden states bit-identical; fewer graph nodes with the option on."""
    t, w = tiny
    _, args = _fixture(golden_dir, "b40")
    res = {}
    for flag in ("1", "0"):
        with _qlib.options(QTTS_SKINNY_WIDE=flag):
            eng = _engine(t, w, dev, dtype, 40)
            res[flag] = _greedy(eng, t, args, 4) + (eng.stats()["graph_nodes"],)
            del eng
    on, off = res["1"], res["0"]
    assert np.array_equal(on[0], off[0]) and np.array_equal(on[1], off[1]) and np.array_equal(on[2], off[2])
    assert 0 < on[3] < off[3], (on[3], off[3])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_engine_for_64_rows_called_with_20_makes_the_20_row_engines_launches(tiny, dev, dtype):
    """max_batch = 64 called with 20 rows: the codes, hidden states, per-step statistics and graph size of an engine with max_batch = 20."""
    t, w = tiny
    args = synth.rand_prompt(np.random.default_rng(81), t, [3 + (7 * i) % 13 for i in range(20)], 2, scale=0.5)
    res = []
    for mb in (64, 20):
        eng = _engine(t, w, dev, dtype, mb)
        st = None
        out = _greedy(eng, t, args, 4)
        st = eng.stats()
        res.append(out + ({k: st[k] for k in PER_STEP},))
        del eng
    big, small = res
    assert np.array_equal(big[0], small[0]) and np.array_equal(big[1], small[1]) and np.array_equal(big[2], small[2])
    assert big[3] == small[3], (big[3], small[3])


def test_released_code_predictor_dims_at_64_rows(dev):
    """The EXACT instantiations of skinny_wide_kernel (K = 1024 / 2048 / 3072) in the frame step: 0.6B dims with two talker layers, bf16,
    64 rows, 4 forced frames.  Two runs are bit-identical, and QTTS_SKINNY_WIDE on equals off bit for bit."""
    t = dataclasses.replace(synth.talker_06b(), num_hidden_layers=2)
    w = {k: torch.from_numpy(v) for k, v in synth.talker_weights(t, with_text=False).items()}
    args = synth.rand_prompt(np.random.default_rng(64), t, [3 + (7 * i) % 13 for i in range(64)], 2, scale=0.5)
    res = {}
    for flag in ("1", "0"):
        with _qlib.options(QTTS_SKINNY_WIDE=flag):
            eng = _engine(t, w, dev, torch.bfloat16, 64)
            res[flag] = _greedy(eng, t, args, 5)
            if flag == "1":
                again = _greedy(eng, t, args, 5)
                assert all(np.array_equal(a, b) for a, b in zip(res[flag], again)), "two runs differ"
            del eng
            torch.cuda.empty_cache()
    assert res["1"][0].shape == (64, 4, 16)
    assert all(np.array_equal(a, b) for a, b in zip(res["1"], res["0"])), "QTTS_SKINNY_WIDE=0 gives other bits"


def test_limits_and_debug_cp_logits(tiny, dev):
    """max_batch 65 and 0 are refused (QTTS_ERR_LIMIT, the message names 1..64); a 65-row call on a 64-row engine raises ValueError;
    debug_cp_logits at B < max_batch has the live batch's shape and its argmax is the engine's own greedy choice of every pass."""
    t, w = tiny
    for mb in (65, 0):
        with pytest.raises(_qlib.QttsError, match=r"max_batch must be 1\.\.64") as ei:
            _engine(t, w, dev, torch.float32, mb)
        assert ei.value.code == -6
    eng = _engine(t, w, dev, torch.float32, 64)
    e, m, tr, pad = synth.rand_prompt(np.random.default_rng(3), t, [4] * 65, 2, scale=0.5)
    with pytest.raises(ValueError, match="exceeds max_batch 64"):
        eng.generate(e, m, tr, pad, max_new_tokens=2)
    codes, _, _ = _greedy(eng, t, (e[:12], m[:12], tr[:12], pad), 3)
    lg = eng.debug_cp_logits().cpu().numpy()
    assert lg.shape == (t.num_code_groups - 1, 12, t.cp_vocab_size)
    assert np.array_equal(lg.argmax(-1).T, codes[:, -1, 1:])
