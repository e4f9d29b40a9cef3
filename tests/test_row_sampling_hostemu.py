"""CPU: per-request sampling settings (qtts_talker_generate_rows / qtts_talker_stream_begin_rows and the Python above them) on the
host-emulation build -- the engine's real C++ and sampling.hip's real kernels on the SIMT emulator, the product's Python unmodified
(tests/hostemu/pyshim.py, as tests/test_glue_on_emulator.py runs it).  The test bodies are those of tests/test_row_sampling_gpu.py;
the refusals and the host logic at the end need no GPU at all."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
QTTS_ERR_ARG, QTTS_ERR_LIMIT = -1, -6


@pytest.fixture(scope="module")
def rs():
    sys.path.insert(0, os.path.join(HERE, "hostemu"))
    import pyshim
    pyshim.install()
    try:
        import test_row_sampling_gpu as m
        yield m
    finally:
        pyshim.uninstall()


@pytest.mark.parametrize("graph", [False, True])
def test_greedy_rows_through_the_table_are_the_reference_run(rs, golden_dir, graph):
    rs.body_greedy_table("cpu", golden_dir, graph)


@pytest.mark.parametrize("dtype,graph,B", [(torch.bfloat16, True, 4), (torch.float32, False, 8)])
def test_every_row_draws_under_its_own_settings_fast_class(rs, dtype, graph, B):
    rs.body_fast_class("cpu", *rs._tiny(), dtype, graph, B, calls=2)


@pytest.mark.parametrize("dtype,graph", [(torch.bfloat16, True), (torch.float32, False)])
def test_greedy_top_p_only_and_large_top_k_rows_share_a_batch(rs, dtype, graph):
    rs.body_general_class("cpu", dtype, graph)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_a_rows_output_does_not_depend_on_its_place_in_the_batch(rs, dtype):
    rs.body_position_independence("cpu", dtype)


def test_a_request_keeps_its_codes_whatever_wave_it_lands_in(rs):
    rs.body_model_waves("cpu")


def test_identical_requests_without_own_seeds_do_not_share_draws(rs):
    rs.body_requests_without_own_seeds("cpu")


@pytest.mark.parametrize("graph", [False, True])
def test_rows_stop_at_their_own_limits_and_floors(rs, graph):
    rs.body_row_limits("cpu", graph)


@pytest.mark.parametrize("graph", [False, True])
def test_stream_packets_with_a_table_equal_generate(rs, graph):
    rs.body_stream("cpu", graph)


def test_wrapper_takes_per_request_settings(rs):
    rs.body_wrapper("cpu")


# ============================================================================================ 8. host logic and refusals
def _rows(B, **over):
    from qwen3_tts_amd import _lib
    rows = (_lib.RowSamplingC * B)()
    for b in range(B):
        r = rows[b]
        r.do_sample, r.top_k, r.top_p, r.temperature, r.repetition_penalty = 1, 50, 1.0, 0.9, 1.05
        r.subtalker_dosample, r.subtalker_top_k, r.subtalker_top_p, r.subtalker_temperature = 1, 50, 1.0, 0.9
        r.max_new_tokens, r.min_new_tokens, r.seed = 4, 2, 5 + b
    for k, (b, v) in over.items():
        setattr(rows[b], k, v)
    return rows


def test_refusals_name_the_row_and_leave_the_engine_usable(rs):
    """A sequence of the wrong length, a bad element (HF's wording), a table with teacher forcing: ValueError.  At the C ABI: n_rows != B,
    a top_p outside (0, 1] on a sampling row, temperature <= 0, max_new_tokens < 1 (QTTS_ERR_ARG, the message names the row), the
    largest limit beyond max_seq (QTTS_ERR_LIMIT), a table while teacher forcing is set (QTTS_ERR_ARG).  After each of them the same
    prefill still generates."""
    from qwen3_tts_amd import _lib
    t, w = rs._tiny()
    B = 4
    eng = rs._engine(t, w, "cpu", torch.float32, False, B, max_seq=32)
    args, _ = rs._prompt(t, B)
    sup = rs._suppress(t)
    kw = dict(max_new_tokens=4, min_new_tokens=2, suppress_tokens=sup)
    good = eng.generate(*args, seed=[1, 2, 3, 4], **kw)
    for bad, msg in ((dict(temperature=[0.9, 0.8]), r"`temperature` has 2 entries for a batch of 4"),
                     (dict(seed=[1, 2, 3, 4, 5]), r"`seed` has 5 entries"),
                     (dict(top_k=[50, -3, 50, 50]), r"`top_k` has to be a strictly positive integer, but is -3"),
                     (dict(top_p=[1.0, 1.0, 1.5, 1.0]), r"`top_p` has to be a float > 0 and < 1, but is 1.5"),
                     (dict(subtalker_temperature=[0.9, 0.9, 0.9, 0.0]), r"`subtalker_temperature` \(=0.0\) has to be a strictly positive float"),
                     (dict(max_new_tokens=[4, 0, 4, 4]), r"`max_new_tokens` of request 1"),
                     (dict(seed=[1, 2, 3, 4], teacher_codes=torch.zeros(B, 3, t.num_code_groups, dtype=torch.long)), r"teacher_codes takes scalar")):
        with pytest.raises(ValueError, match=msg):
            eng.generate(*args, **{**kw, **bad})
        if "teacher_codes" not in bad:                                 # (teacher forcing is a `generate` mode)
            with pytest.raises(ValueError, match=msg):
                list(eng.generate_stream(*args, **{**kw, **bad}))
    # a None seed draws a fresh one for that row only
    a = eng.generate(*args, seed=[1, None, 3, 4], **kw)
    assert np.array_equal(a.tokens[0].numpy(), good.tokens[0].numpy()) and np.array_equal(a.codes[2].numpy(), good.codes[2].numpy())
    # a per-row limit beyond the KV capacity is clamped per row, as the scalar is
    with pytest.warns(UserWarning, match="exceeds the KV capacity"):
        big = eng.generate(*args, seed=[1, 2, 3, 4], **dict(kw, max_new_tokens=[4, 1000, 4, 4], min_new_tokens=40))
    assert big.tokens.shape[1] == 32 - args[0].shape[1]

    # ---- the C ABI
    lib, h = eng._lib, eng._h
    emb, mask, trail, pad = args
    T = emb.shape[1]
    embc, trc, padc = emb.contiguous(), trail.contiguous(), pad.reshape(-1).contiguous()
    npad = (C.c_int32 * B)(*[int(x) for x in (1 - mask).sum(-1)])
    sup_c = (C.c_int32 * len(sup))(*sup)
    codes = torch.zeros(B, 3, t.num_code_groups, dtype=torch.int64)        # (B, largest limit - 1, G): the one call below that runs
    tokens = torch.zeros(B, 4, dtype=torch.int64)
    nf = C.c_int32(0)

    def prefill():
        _lib.check(lib.qtts_talker_prefill(h, C.c_void_p(embc.data_ptr()), B, T, npad, C.c_void_p(trc.data_ptr()), trc.shape[1],
                                           C.c_void_p(padc.data_ptr()), None))

    def call(rows, n):
        return lib.qtts_talker_generate_rows(h, rows, n, t.codec_eos_token_id, sup_c, len(sup), C.c_void_p(codes.data_ptr()), None,
                                             C.c_void_p(tokens.data_ptr()), C.byref(nf), None)

    def begin(rows, n):
        return lib.qtts_talker_stream_begin_rows(h, rows, n, t.codec_eos_token_id, sup_c, len(sup), C.c_void_p(codes.data_ptr()), None, None)

    err = lambda: (lib.qtts_last_error() or b"").decode()
    prefill()
    for fn in (call, begin):
        assert fn(_rows(B), B - 1) == QTTS_ERR_ARG and "n_rows (3) must equal the prefilled batch (4)" in err()
        assert fn(_rows(B, top_p=(2, 0.0)), B) == QTTS_ERR_ARG and "row 2: top_p" in err()
        assert fn(_rows(B, subtalker_top_p=(1, 1.5)), B) == QTTS_ERR_ARG and "row 1: subtalker_top_p" in err()
        assert fn(_rows(B, temperature=(3, 0.0)), B) == QTTS_ERR_ARG and "row 3: temperature" in err()
        assert fn(_rows(B, max_new_tokens=(0, 0)), B) == QTTS_ERR_ARG and "row 0: max_new_tokens" in err()
        assert fn(_rows(B, max_new_tokens=(1, 32 - T + 1)), B) == QTTS_ERR_LIMIT and "exceeds max_seq" in err()
        # a greedy row may carry any top_p: the knob is not read
        r = _rows(B, top_p=(2, 0.0))
        r[2].do_sample = 0
    tc = torch.zeros(B, 3, t.num_code_groups, dtype=torch.long)
    own = torch.zeros(B, 4, t.num_code_groups, dtype=torch.int32)
    _lib.check(lib.qtts_talker_set_teacher(h, C.c_void_p(tc.data_ptr()), 3, C.c_void_p(own.data_ptr()), None, None))
    try:
        assert call(_rows(B), B) == QTTS_ERR_ARG and "teacher forcing" in err()
    finally:
        _lib.check(lib.qtts_talker_set_teacher(h, None, 0, None, None, None))
    # every refusal above left the prefill in place: the call now runs, and equals the Python call with the same table
    assert call(r, B) == 0, err()
    n = nf.value
    again = eng.generate(*args, seed=[5, 6, 7, 8], do_sample=[True, True, False, True], **kw)
    assert again.n_frames == n >= 1 and np.array_equal(codes[:, :n].numpy(), again.codes.numpy())
    assert call(_rows(B), B) != 0 and "prefill() first" in err()      # ... and consumed it


def test_table_values_replay_the_captured_graph_at_the_c_abi(rs):
    """The frame graph's key holds the output buffers and, in table mode, no sampling value.  With the caller's buffers fixed (the C ABI,
    no allocator in between): a second table with other values adds no capture -- and gives other codes, so the values are read, not
    baked in --, a table of the general class adds one, another such table none, a scalar call one, the same scalar call none, and the
    first table again reproduces its codes bit for bit."""
    from qwen3_tts_amd import _lib
    t, w = rs._tiny()
    B, M = 4, 4
    eng = rs._engine(t, w, "cpu", torch.float32, True, B)
    (emb, mask, trail, pad), _ = rs._prompt(t, B)
    lib, h = eng._lib, eng._h
    embc, trc, padc = emb.contiguous(), trail.contiguous(), pad.reshape(-1).contiguous()
    npad = (C.c_int32 * B)(*[int(x) for x in (1 - mask).sum(-1)])
    sup = rs._suppress(t)
    sup_c = (C.c_int32 * len(sup))(*sup)
    codes = torch.zeros(B, M - 1, t.num_code_groups, dtype=torch.int64)
    nf = C.c_int32(0)

    def run(rows=None, temperature=0.9):
        _lib.check(lib.qtts_talker_prefill(h, C.c_void_p(embc.data_ptr()), B, emb.shape[1], npad, C.c_void_p(trc.data_ptr()), trc.shape[1],
                                           C.c_void_p(padc.data_ptr()), None))
        if rows is not None:
            _lib.check(lib.qtts_talker_generate_rows(h, rows, B, t.codec_eos_token_id, sup_c, len(sup), C.c_void_p(codes.data_ptr()), None,
                                                     None, C.byref(nf), None))
        else:
            sp = _lib.SamplingC(1, 50, 1.0, temperature, 1.05, 1, 50, 1.0, 0.9, 3)
            _lib.check(lib.qtts_talker_generate(h, C.byref(sp), M, M, t.codec_eos_token_id, sup_c, len(sup), C.c_void_p(codes.data_ptr()),
                                                None, None, C.byref(nf), None))
        st = eng.stats()
        assert nf.value == M - 1 and st["row_table_last"] == (rows is not None)
        return codes.numpy().copy(), st["graph_captures"]

    def table(temp, top_k):
        rows = _rows(B)
        for b in range(B):
            rows[b].max_new_tokens = rows[b].min_new_tokens = M
            rows[b].temperature, rows[b].top_k, rows[b].subtalker_top_k = temp + 0.1 * b, top_k, top_k
        return rows

    a, c = run(table(0.7, 20))
    assert c == 1
    b_, c = run(table(1.2, 64))
    assert c == 1 and not np.array_equal(a, b_)
    _, c = run(table(0.7, 300))
    assert c == 2
    _, c = run(table(1.1, 0))
    assert c == 2
    _, c = run(None, 0.9)
    assert c == 3
    _, c = run(None, 0.9)
    assert c == 3
    _, c = run(None, 0.8)                       # (the scalar path bakes its values in, as before)
    assert c == 4
    a2, c = run(table(0.7, 20))
    assert c == 5 and np.array_equal(a, a2)


def test_row_sampling_ctypes_layout_matches_the_header(tmp_path):
    """`_lib.RowSamplingC` against `qtts_row_sampling` of include/qtts.h as gcc lays it out (field order, offsets, size), and the two
    fields appended to `qtts_talker_stats` -- what tests/test_host_logic.py::test_ctypes_struct_layouts_match_the_header does for the
    structs it lists."""
    import re
    import subprocess
    from qwen3_tts_amd import _lib
    hdr_path = os.path.join(os.path.dirname(HERE), "include", "qtts.h")
    hdr = re.sub(r"/\*.*?\*/", "", open(hdr_path).read(), flags=re.S)
    body = re.search(r"typedef struct qtts_row_sampling\s*\{(.*?)\}\s*qtts_row_sampling\s*;", hdr, flags=re.S).group(1)
    names = [re.findall(r"([A-Za-z_][A-Za-z_0-9]*)\s*$", d.strip())[0] for d in body.split(";") if d.strip()]
    assert names == [f[0] for f in _lib.RowSamplingC._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{hdr_path}"', 'int main(void) {',
             'printf("size %zu\\n", sizeof(qtts_row_sampling));', 'printf("stats %zu\\n", sizeof(qtts_talker_stats));']
    lines += [f'printf("{f} %zu\\n", offsetof(qtts_row_sampling, {f}));' for f in names]
    lines += [f'printf("st_{f} %zu\\n", offsetof(qtts_talker_stats, {f}));' for f in ("row_table_last", "graph_captures")]
    lines += ['return 0; }']
    (tmp_path / "probe.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-o", str(tmp_path / "probe"), str(tmp_path / "probe.c")], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(tmp_path / "probe")], capture_output=True, text=True, check=True).stdout.splitlines())
    assert C.sizeof(_lib.RowSamplingC) == int(got["size"]) and C.sizeof(_lib.TalkerStatsC) == int(got["stats"])
    for f in names:
        assert getattr(_lib.RowSamplingC, f).offset == int(got[f]), f
    for f in ("row_table_last", "graph_captures"):
        assert getattr(_lib.TalkerStatsC, f).offset == int(got["st_" + f]), f
    assert [f[0] for f in _lib.TalkerStatsC._fields_][-2:] == ["row_table_last", "graph_captures"]


def test_merge_generate_kwargs_fills_none_elements_with_the_default():
    from qwen3_tts_amd.model import Qwen3TTSModel
    m = Qwen3TTSModel.__new__(Qwen3TTSModel)
    m.generate_defaults = {"top_k": 40}
    out = m._merge_generate_kwargs(temperature=[None, 0.5], top_k=[None, 7, None], max_new_tokens=[None, 12], seed=[1, 2])
    assert out["temperature"] == [0.9, 0.5] and out["top_k"] == [40, 7, 40] and out["max_new_tokens"] == [2048, 12]
    assert out["seed"] == [1, 2] and out["top_p"] == 1.0 and out["do_sample"] is True
