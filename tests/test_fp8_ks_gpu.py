"""FP8 weights at batch 17..32 on the MI355X: skinny2_ks_fp8_kernel bitwise against the bf16 split-K kernel on d (the cases of
tests/test_fp8_ks_hostemu.py), and the engine identity through the Python class where the o- and down-projections split -- at the
emulator test's dims with the K floor lowered, and at 1.7B dims, batch 32, default options (the shape BASELINE configs 4 and 5 run)."""
import dataclasses

import numpy as np
import pytest
import torch

import fp8_ks_cases as ks
import synth
from test_gpu_parity import _suppress, _td, dev  # noqa: F401  (`dev` is a fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib(dev):
    from qwen3_tts_amd import load_library
    return ks.prototypes(load_library())


# ============================================================================================ the kernel
@pytest.mark.parametrize("case", ks.CASES, ids=ks.IDS)
def test_fp8_split_k_is_bitwise_the_bf16_split_k_kernel_on_d(lib, case):
    ks.check_case(lib, case)


@pytest.mark.parametrize("shape", ks.ALL_CODES, ids=lambda s: "x".join(map(str, s)))
def test_every_finite_code_through_the_split_path(lib, shape):
    ks.all_codes(lib, *shape)


def test_shapes_outside_the_split_keep_the_unsplit_fp8_kernel(lib):
    ks.not_split(lib)


# ============================================================================================ the engine
def _same(a, b, what):
    for f in ("codes", "tokens", "hidden"):
        assert getattr(a, f) is not None and torch.equal(getattr(a, f), getattr(b, f)), (what, f)
    assert a.n_frames == b.n_frames, what


def _greedy(t, frames):
    return dict(max_new_tokens=frames + 1, min_new_tokens=frames + 1, suppress_tokens=_suppress(t), repetition_penalty=1.05, do_sample=False,
                subtalker_dosample=False, output_hidden_states=True)


def test_fp8_engine_is_the_bf16_engine_of_the_effective_checkpoint_where_k_splits(dev, lib):
    """The emulator test's configuration on the hardware: 18 rows, ragged prompt, 3 greedy frames, captured graph, K floor 2048; the control
    QTTS_SKINNY_KS_FP8=0 keeps skinny2_fp8_kernel for the fp8 engine's talker operators."""
    from qwen3_tts_amd import fp8
    from qwen3_tts_amd.talker import TalkerEngine
    t = ks.engine_config()
    w = _td(synth.talker_weights(t, with_text=False))
    weff = fp8.effective_state_dict(synth.cfg_dict(t), w)
    prompt = synth.rand_prompt(np.random.default_rng(21 + ks.ENGINE_ROWS), t, ks.ENGINE_LENS, 2, scale=0.05)
    kw = _greedy(t, ks.ENGINE_FRAMES)
    L = t.num_hidden_layers
    out, split = {}, {}
    for name, sd, fmt, fp8_split in (("fp8", w, "fp8", None), ("bf16", weff, None, None), ("fp8_unsplit", w, "fp8", "0")):
        with ks.options(lib, QTTS_SKINNY_KS_MINK=ks.MINK, QTTS_SKINNY_KS_FP8=fp8_split):
            eng = TalkerEngine(t, sd, weight_dtype=torch.bfloat16, device=dev, max_batch=ks.ENGINE_ROWS, max_seq=48, use_graph=True, weight_format=fmt)
            out[name] = eng.generate(*prompt, **kw)
            st = eng.stats()
            split[name] = st["ks_split_per_step"]
            assert st["graph_nodes"] > 0 and st["cp_fused_giveups"] == 0, st
            if name == "fp8":
                _same(eng.generate(*prompt, **kw), out[name], "second generation on the same handle")
                last = eng.debug_logits()[:ks.ENGINE_ROWS].clone()
            elif name == "bf16":
                assert torch.equal(eng.debug_logits()[:ks.ENGINE_ROWS], last), "last logits"
            del eng
    print("ks_split_per_step:", split)
    assert out["fp8"].n_frames == ks.ENGINE_FRAMES
    assert split["fp8"] == split["bf16"] and split["fp8"] >= 2 * L, split
    _same(out["fp8"], out["bf16"], "fp8 engine against the bf16 engine on the effective checkpoint")
    assert split["fp8_unsplit"] == split["fp8"] - 2 * L, split
    h1, h0 = out["fp8"].hidden.float().cpu().numpy(), out["fp8_unsplit"].hidden.float().cpu().numpy()
    assert not np.array_equal(h1, h0), "QTTS_SKINNY_KS_FP8=0 did not select another kernel"
    dh = float(np.abs(h1 - h0).max())
    print(f"|hidden split - unsplit|max {dh:.3e} (bound {3e-2 * max(1.0, float(np.abs(h0).max())):.3e})")
    assert dh <= 3e-2 * max(1.0, float(np.abs(h0).max())), dh


def test_fp8_engine_at_the_real_models_dims_batch_32(dev):
    """1.7B dims (two layers' worth of the talker and of the code predictor), batch 32, DEFAULT options, 4 greedy frames, captured graph: the
    down-projection (N 2048, K 6144) runs on skinny2_ks_fp8_kernel in the fp8 engine and on skinny2_ks_kernel in the bf16 engine on the
    effective checkpoint -- codes, tokens and hidden rows are identical, the split counters equal, three fp8 runs identical."""
    from qwen3_tts_amd import fp8
    from qwen3_tts_amd.talker import TalkerEngine
    t = dataclasses.replace(synth.talker_17b(), num_hidden_layers=2, cp_num_hidden_layers=2)
    w = _td(synth.talker_weights(t, with_text=False))
    weff = fp8.effective_state_dict(synth.cfg_dict(t), w)
    prompt = synth.rand_prompt(np.random.default_rng(34), t, [2 + (3 * i) % 6 for i in range(32)], 1)
    kw = _greedy(t, 4)
    out, split = [], []
    for sd, fmt in ((w, "fp8"), (weff, None)):
        eng = TalkerEngine(t, sd, weight_dtype=torch.bfloat16, device=dev, max_batch=32, max_seq=32, use_graph=True, weight_format=fmt)
        out.append(eng.generate(*prompt, **kw))
        if fmt == "fp8":
            for rep in (1, 2):
                _same(eng.generate(*prompt, **kw), out[0], f"fp8 run {rep} against run 0")
        st = eng.stats()
        assert st["graph_nodes"] > 0 and st["cp_fused_giveups"] == 0, st
        split.append(st["ks_split_per_step"])
        del eng
    print("ks_split_per_step (fp8, bf16 on W_eff):", split)
    assert out[0].n_frames == 4
    assert split[0] == split[1] and split[0] >= t.num_hidden_layers, split
    _same(out[0], out[1], "fp8 engine against the bf16 engine on the effective checkpoint")
