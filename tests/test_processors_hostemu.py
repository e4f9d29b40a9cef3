"""CPU: the talker's remaining HF logits processors (qtts_talker_set_row_processors, sample_warp_kernel's processor stages and the Python
above them) on the host-emulation build -- the engine's real C++ and sampling.hip's real kernels on the SIMT emulator, the product's
Python unmodified (tests/hostemu/pyshim.py).  The test bodies are those of tests/test_processors_gpu.py; the hand-driven ones run under
three fiber orders; the refusals, the layout and the host logic at the end need no GPU at all."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
QTTS_ERR_ARG, QTTS_ERR_LIMIT = -1, -6


@pytest.fixture(scope="module")
def pp():
    sys.path.insert(0, os.path.join(HERE, "hostemu"))
    import pyshim
    pyshim.install()
    try:
        import test_processors_gpu as m
        yield m
    finally:
        pyshim.uninstall()


@pytest.mark.parametrize("name,graph", [("a", False), ("b", True)])
def test_processors_are_the_reference_run(pp, golden_dir, name, graph):
    pp.body_reference("cpu", golden_dir, graph, name)


def test_processors_through_stream_packets_and_the_continuous_schedule(pp, golden_dir):
    pp.body_streams("cpu", golden_dir)


def test_every_row_draws_under_its_own_processors(pp):
    pp.body_draws("cpu", *pp.rs._tiny(), torch.float32, False, 6, M=4, shifts=(0,))


def test_hand_written_controls_under_three_fiber_orders(pp):
    """body_hand (every step against the restatement) and body_place (sampled rows, 64 records on a neighbour) with the emulator's
    fibers scheduled in three orders: the same tokens -- the bias sums and the bans do not depend on thread or wave scheduling."""
    from qwen3_tts_amd import _lib
    emu = _lib.load_library()
    runs = []
    for order in (0, 1, 2):
        emu.hostemu_set_fiber_order(order)
        try:
            runs.append(pp.body_hand("cpu", M=6))
            if order != 1:
                pp.body_place("cpu", M=5)
        finally:
            emu.hostemu_set_fiber_order(0)
    assert all(np.array_equal(r, runs[0]) for r in runs[1:])


def test_a_request_with_records_admitted_into_a_stream_that_ran_without_any(pp):
    pp.body_admitted("cpu")


def test_a_preempted_request_with_records_restarts_to_the_same_codes(pp):
    pp.body_pooled_restart("cpu")


def test_wrapper_passes_the_processors_to_the_engine(pp):
    pp.body_wrapper("cpu")


# ============================================================================================ refusals, layout, host logic
def test_python_refusals_use_hfs_wording(pp):
    t, w = pp.rs._tiny()
    B, V, eos = 4, t.vocab_size, t.codec_eos_token_id
    eng = pp.rs._engine(t, w, "cpu", torch.float32, False, B, max_seq=32)
    args, _ = pp.rs._prompt(t, B)
    kw = dict(max_new_tokens=4, min_new_tokens=2, suppress_tokens=pp._suppress(t), seed=3)
    cases = ((dict(sequence_bias={}), r"`sequence_bias` has to be a non-empty dictionary, or non-empty list of lists but is \{\}\."),
             (dict(sequence_bias=[]), r"`sequence_bias` has to be a non-empty dictionary, or non-empty list of lists but is \[\]\."),
             (dict(sequence_bias=5), r"`sequence_bias` has to be a non-empty dictionary, or non-empty list of lists but is 5\."),
             (dict(sequence_bias={"a": 1.0}), r"`sequence_bias` has to be a dict with tuples as keys"),
             (dict(sequence_bias={(1, -2): 1.0}), r"Each key in `sequence_bias` has to be a non-empty tuple of positive integers"),
             (dict(sequence_bias={(1, 2): 1}), r"`sequence_bias` has to be a dict with floats as values"),
             (dict(sequence_bias=[[[1, 2], 1]]), r"Each element in `sequence_bias` has to be a non-empty list of lists of positive integers and float"),
             (dict(sequence_bias={(1, V): 1.0}), rf"The model vocabulary size is {V}, but the following tokens were being biased: \[{V}\]"),
             (dict(bad_words_ids=[]), r"`bad_words_ids` has to be a non-empty list, but is \[\]\."),
             (dict(bad_words_ids=7), r"`bad_words_ids` has to be a non-empty list, but is 7\."),
             (dict(bad_words_ids=[[1, -1]]), r"Each list in `bad_words_ids` has to be a list of positive integers"),
             (dict(bad_words_ids=[[3, V + 1]]), rf"The model vocabulary size is {V}, but the following tokens were being biased: \[{V + 1}\]"),
             (dict(bad_words_ids=[None, [[1, -1]], None, None]), r"Each list in `bad_words_ids` has to be a list of positive integers"),
             (dict(min_length=-1), r"`min_length` has to be a non-negative integer, but is -1"),
             (dict(min_length=2.5), r"`min_length` has to be a non-negative integer, but is 2.5"),
             (dict(forced_eos_token_id=eos - 1), r"`forced_eos_token_id` can only force the call's own eos_token_id"),
             (dict(forced_eos_token_id=[eos, eos - 1, None, None]), r"`forced_eos_token_id` can only force the call's own eos_token_id"),
             (dict(forced_eos_token_id=[eos, eos]), r"`forced_eos_token_id` has 2 entries for a batch of 4"),
             (dict(forced_eos_token_id=[[eos], None, None, None]), r"`forced_eos_token_id` can only force the call's own eos_token_id"),
             (dict(exponential_decay_length_penalty=(2, -1.0)), r"`exponential_decay_length_penalty` has to be a \(start_index, decay_factor\) pair"),
             (dict(exponential_decay_length_penalty=[(2, 1.5), None]), r"`exponential_decay_length_penalty` has 2 entries for a batch of 4"),
             (dict(begin_suppress_tokens=[V]), r"`begin_suppress_tokens` has to be a list of token ids"),
             (dict(begin_suppress_tokens=[[1], [2]]), r"`begin_suppress_tokens` has 2 entries for a batch of 4"),
             (dict(sequence_bias={(i, i + 1): 1.0 for i in range(1, 99)}), r"request 0: 98 sequences with 196 tokens exceed the engine's capacity"),
             (dict(bad_words_ids=[[list(range(1, 200)), list(range(2, 201)), list(range(3, 202))], None, None, None]),
              r"request 0: 3 sequences with 597 tokens exceed the engine's capacity"),
             (dict(bad_words_ids=[[5]], teacher_codes=torch.zeros(B, 3, t.num_code_groups, dtype=torch.long)), r"teacher_codes takes scalar"))
    for bad, msg in cases:
        with pytest.raises(ValueError, match=msg):
            eng.generate(*args, **{**kw, **bad})
        if "teacher_codes" not in bad:
            with pytest.raises(ValueError, match=msg):
                list(eng.generate_stream(*args, **{**kw, **bad}))
            with pytest.raises(ValueError, match=msg):
                eng.generate(*args, schedule="continuous", **{**kw, **bad})
    # bad words that hold nothing but [eos]: HF drops the entry and then refuses the empty rest
    with pytest.raises(ValueError, match=r"`sequence_bias` has to be a non-empty dictionary"):
        eng.generate(*args, bad_words_ids=[[eos]], **kw)
    # gating: values that are off leave the call on the scalar path; min_length alone is a floor and no device control
    plain = eng.generate(*args, **kw)
    off = eng.generate(*args, sequence_bias=None, begin_suppress_tokens=[], min_length=0, forced_eos_token_id=[None] * B, **kw)
    assert eng.sampler_class() == (0, 0) and eng.stats()["row_table_last"] == 0
    assert np.array_equal(off.codes.numpy(), plain.codes.numpy())
    floor = eng.generate(*args, min_length=3, **kw)
    assert eng.sampler_class() == (0, 0) and (floor.tokens.numpy()[:, :3] != eos).all()
    on = eng.generate(*args, begin_suppress_tokens=[int(plain.tokens[0, 0])], **kw)
    assert eng.sampler_class() == (3, 1) and eng.stats()["row_table_last"] == 1
    listed = eng.generate(*args, begin_suppress_tokens=[[int(plain.tokens[0, 0])]] * B, **dict(kw, seed=[3, 4, 5, 6]))
    assert np.array_equal(on.codes.numpy(), listed.codes.numpy()) and int(on.tokens[0, 0]) != int(plain.tokens[0, 0])


def _records(n, **over):
    """n all-off `_lib.RowProcessorsC`; `over`: row -> (flags, decay_start, decay_factor, [(kind, ids, bias)])"""
    from qwen3_tts_amd import _lib
    ps = (_lib.RowProcessorsC * n)()
    for b, (flags, start, factor, recs) in over.items():
        words = []
        for kind, ids, bias in recs:
            words += [kind, len(ids), C.c_int32.from_buffer_copy(C.c_float(bias)).value] + list(ids)
        e = ps[int(b)]
        e.flags, e.decay_start, e.decay_factor, e.n_records, e.n_words = flags, start, factor, len(recs), len(words)
        e.records[:min(len(words), _lib.PROC_MAX_WORDS)] = words[:_lib.PROC_MAX_WORDS]
    return ps


def test_c_abi_refusals_leave_the_engine_usable(pp):
    """A bad value fails at set time and names the row -- capacity with QTTS_ERR_LIMIT, the rest with QTTS_ERR_ARG; a count mismatch at
    the consuming call, a scalar call with a pending table and a table together with teacher forcing fail too -- nothing changed: the
    same prefill then still generates."""
    from qwen3_tts_amd import _lib
    from test_row_sampling_hostemu import _rows
    t, w = pp.rs._tiny()
    B, V = 4, t.vocab_size
    eng = pp.rs._engine(t, w, "cpu", torch.float32, False, B, max_seq=32)
    (emb, mask, trail, pad), _ = pp.rs._prompt(t, B)
    lib, h = eng._lib, eng._h
    T = emb.shape[1]
    embc, trc, padc = emb.contiguous(), trail.contiguous(), pad.reshape(-1).contiguous()
    npad = (C.c_int32 * B)(*[int(x) for x in (1 - mask).sum(-1)])
    sup = pp._suppress(t)
    sup_c = (C.c_int32 * len(sup))(*sup)
    codes = torch.zeros(B, 3, t.num_code_groups, dtype=torch.int64)
    nf = C.c_int32(0)
    err = lambda: (lib.qtts_last_error() or b"").decode()

    def prefill():
        _lib.check(lib.qtts_talker_prefill(h, C.c_void_p(embc.data_ptr()), B, T, npad, C.c_void_p(trc.data_ptr()), trc.shape[1],
                                           C.c_void_p(padc.data_ptr()), None))

    def call(rows, n):
        return lib.qtts_talker_generate_rows(h, rows, n, t.codec_eos_token_id, sup_c, len(sup), C.c_void_p(codes.data_ptr()), None, None,
                                             C.byref(nf), None)
    prefill()
    BIAS, BAN, BEGIN = _lib.PROC_KIND_BIAS, _lib.PROC_KIND_BAN, _lib.PROC_KIND_BEGIN
    ok = {0: (0, 0, 0.0, [(BAN, [5], 0.0)])}
    for over, code, what in (({2: (0, 0, 0.0, [(BIAS, [1, V], 1.0)])}, QTTS_ERR_ARG, "row 2: record 0: token"),
                             ({1: (0, 0, 0.0, [(BAN, [3], 0.0), (BEGIN, [-1], 0.0)])}, QTTS_ERR_ARG, "row 1: record 1: token"),
                             ({3: (0, 0, 0.0, [(7, [3], 0.0)])}, QTTS_ERR_ARG, "row 3: record 0: unknown kind"),
                             ({0: (_lib.PROC_DECAY, 2, -1.0, [])}, QTTS_ERR_ARG, "row 0: decay_factor"),
                             ({0: (_lib.PROC_DECAY, 2, float("nan"), [])}, QTTS_ERR_ARG, "row 0: decay_factor"),
                             ({1: (4, 0, 0.0, [])}, QTTS_ERR_ARG, "row 1: unknown flag"),
                             ({2: (0, 0, 0.0, [(BAN, [1, 2, 3], 0.0)] * 3 + [(BAN, list(range(1, 200)), 0.0)] * 3)}, QTTS_ERR_LIMIT,
                              f"row 2: the records' tokens exceed the capacity of {_lib.PROC_MAX_TOKENS} per row")):
        assert lib.qtts_talker_set_row_processors(h, _records(B, **{str(k): v for k, v in over.items()}), B) == code and what in err(), (over, err())
    many = _records(B)
    many[1].n_records = _lib.PROC_MAX_RECORDS + 1
    assert lib.qtts_talker_set_row_processors(h, many, B) == QTTS_ERR_LIMIT and f"row 1: {_lib.PROC_MAX_RECORDS + 1} records exceed the capacity of {_lib.PROC_MAX_RECORDS}" in err()
    many = _records(B)
    many[3].n_words = _lib.PROC_MAX_WORDS + 1
    assert lib.qtts_talker_set_row_processors(h, many, B) == QTTS_ERR_LIMIT and "row 3" in err() and str(_lib.PROC_MAX_WORDS) in err()
    short = _records(B, **{"0": (0, 0, 0.0, [(BAN, [5, 6], 0.0)])})
    short[0].n_words = 4                                              # the record says 2 tokens, the row holds one
    assert lib.qtts_talker_set_row_processors(h, short, B) == QTTS_ERR_ARG and "overruns n_words" in err()
    assert lib.qtts_talker_set_row_processors(h, _records(B), B + 1) == QTTS_ERR_ARG
    # a count mismatch at the consuming call; the table is dropped, so the call after it runs without one
    assert lib.qtts_talker_set_row_processors(h, _records(B - 1, **{"0": ok[0]}), B - 1) == 0
    assert call(_rows(B), B) == QTTS_ERR_ARG and "pending processor table" in err()
    # a scalar call with a pending table
    sp = _lib.SamplingC(1, 50, 1.0, 0.9, 1.05, 1, 50, 1.0, 0.9, 3)
    assert lib.qtts_talker_set_row_processors(h, _records(B, **{"0": ok[0]}), B) == 0
    assert lib.qtts_talker_generate(h, C.byref(sp), 4, 2, t.codec_eos_token_id, sup_c, len(sup), C.c_void_p(codes.data_ptr()), None, None,
                                    C.byref(nf), None) == QTTS_ERR_ARG and "processor table is pending" in err()
    assert lib.qtts_talker_set_row_processors(h, _records(B, **{"0": ok[0]}), B) == 0
    assert lib.qtts_talker_stream_begin(h, C.byref(sp), 4, 2, t.codec_eos_token_id, sup_c, len(sup), C.c_void_p(codes.data_ptr()), None,
                                        None) == QTTS_ERR_ARG and "processor table is pending" in err()
    # NULL / 0 clears
    assert lib.qtts_talker_set_row_processors(h, _records(B - 1), B - 1) == 0 and lib.qtts_talker_set_row_processors(h, None, 0) == 0
    # teacher forcing refuses the table call
    tc = torch.zeros(B, 3, t.num_code_groups, dtype=torch.long)
    own = torch.zeros(B, 4, t.num_code_groups, dtype=torch.int32)
    _lib.check(lib.qtts_talker_set_teacher(h, C.c_void_p(tc.data_ptr()), 3, C.c_void_p(own.data_ptr()), None, None))
    try:
        assert lib.qtts_talker_set_row_processors(h, _records(B, **{"0": ok[0]}), B) == 0
        assert call(_rows(B), B) == QTTS_ERR_ARG and "teacher forcing" in err()
    finally:
        _lib.check(lib.qtts_talker_set_teacher(h, None, 0, None, None, None))
    # every refusal left the prefill in place and no table pending: the call runs in the plain class, and equals the Python call
    assert call(_rows(B), B) == 0, err()
    assert eng.sampler_class() == (1, 1)
    again = eng.generate(emb, mask, trail, pad, max_new_tokens=4, min_new_tokens=2, suppress_tokens=sup, seed=[5, 6, 7, 8])
    assert np.array_equal(codes[:, :nf.value].numpy(), again.codes.numpy())
    # a table with everything off is exactly the call without the table
    prefill()
    assert lib.qtts_talker_set_row_processors(h, _records(B), B) == 0 and call(_rows(B), B) == 0 and eng.sampler_class() == (1, 1)
    assert np.array_equal(codes[:, :nf.value].numpy(), again.codes.numpy())
    # ... and one with a record on is class 3, after which a call without a table finds the device entries cleared
    prefill()
    first = int(again.tokens[0, 0])
    assert lib.qtts_talker_set_row_processors(h, _records(B, **{"0": (0, 0, 0.0, [(BEGIN, [first], 0.0)])}), B) == 0
    assert call(_rows(B), B) == 0 and eng.sampler_class() == (3, 1) and int(codes[0, 0, 0]) != first
    assert np.array_equal(codes[1:, :nf.value].numpy(), again.codes.numpy()[1:])
    ws = (_lib.RowWarpersC * B)()
    ws[3].min_p = 1e-6                                                # (class 3 again, through a warper that removes nothing here)
    prefill()
    assert lib.qtts_talker_set_row_warpers(h, ws, B) == 0 and call(_rows(B), B) == 0 and eng.sampler_class() == (3, 1)
    assert int(codes[0, 0, 0]) == first


def test_row_processors_ctypes_layout_matches_the_header(tmp_path):
    """`_lib.RowProcessorsC` and the QTTS_PROC_* constants against include/qtts.h as gcc lays it out; the new symbol is declared and
    listed; the ABI version stays 15."""
    import re
    import subprocess
    from qwen3_tts_amd import _lib
    hdr_path = os.path.join(os.path.dirname(HERE), "include", "qtts.h")
    text = open(hdr_path).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    body = re.search(r"typedef struct qtts_row_processors\s*\{(.*?)\}\s*qtts_row_processors\s*;", hdr, flags=re.S).group(1)
    names = [re.findall(r"([A-Za-z_][A-Za-z_0-9]*)\s*(?:\[\w+\])?\s*$", d.strip())[0] for d in body.split(";") if d.strip()]
    assert names == [f[0] for f in _lib.RowProcessorsC._fields_]
    consts = dict(QTTS_PROC_MAX_RECORDS=_lib.PROC_MAX_RECORDS, QTTS_PROC_MAX_TOKENS=_lib.PROC_MAX_TOKENS, QTTS_PROC_MAX_WORDS=_lib.PROC_MAX_WORDS,
                  QTTS_PROC_KIND_BIAS=_lib.PROC_KIND_BIAS, QTTS_PROC_KIND_BAN=_lib.PROC_KIND_BAN, QTTS_PROC_KIND_BEGIN=_lib.PROC_KIND_BEGIN,
                  QTTS_PROC_DECAY=_lib.PROC_DECAY, QTTS_PROC_FORCED_EOS=_lib.PROC_FORCED_EOS)
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{hdr_path}"', 'int main(void) {',
             'printf("size %zu\\n", sizeof(qtts_row_processors));', 'printf("abi %d\\n", QTTS_ABI_VERSION);']
    lines += [f'printf("{f} %zu\\n", offsetof(qtts_row_processors, {f}));' for f in names]
    lines += [f'printf("{k} %d\\n", (int){k});' for k in consts]
    lines += ['return 0; }']
    (tmp_path / "probe.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-o", str(tmp_path / "probe"), str(tmp_path / "probe.c")], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(tmp_path / "probe")], capture_output=True, text=True, check=True).stdout.splitlines())
    assert C.sizeof(_lib.RowProcessorsC) == int(got["size"]) == 32 + 4 * _lib.PROC_MAX_WORDS
    for f in names:
        assert getattr(_lib.RowProcessorsC, f).offset == int(got[f]), f
    for k, v in consts.items():
        assert int(got[k]) == v, k
    assert _lib.PROC_MAX_RECORDS >= 64 + 1 and _lib.PROC_MAX_TOKENS >= 512       # 64 sequences (and a begin list) and 512 tokens per row
    assert int(got["abi"]) == _lib.ABI_VERSION == 15
    assert "qtts_talker_set_row_processors" in _lib.SYMBOLS and re.search(r"\bint qtts_talker_set_row_processors\(", hdr)


def test_merge_generate_kwargs_passes_the_processors_through():
    from qwen3_tts_amd.model import Qwen3TTSModel
    from qwen3_tts_amd.talker import _split_row_processors
    m = Qwen3TTSModel.__new__(Qwen3TTSModel)
    m.generate_defaults = {"bad_words_ids": [[7]], "min_length": 3}
    six = dict(sequence_bias={(1, 2): 0.5}, bad_words_ids=[None, [[3, 4]]], min_length=[2, None], forced_eos_token_id=[9, None],
               exponential_decay_length_penalty=(2, 1.5), begin_suppress_tokens=[5, 6])
    out = m._merge_generate_kwargs(seed=[1, 2], **six)
    assert all(out[k] == v for k, v in six.items())
    out = m._merge_generate_kwargs(top_k=5)
    assert out["bad_words_ids"] == [[7]] and out["min_length"] == 3 and "sequence_bias" not in out
    m.generate_defaults = {}
    assert not any(k in m._merge_generate_kwargs(top_k=5) for k in six)
    # the one rule for shared and per-request values
    sp = _split_row_processors(2, **six)
    assert sp["sequence_bias"] == [{(1, 2): 0.5}] * 2 and sp["bad_words_ids"] == [None, [[3, 4]]] and sp["min_length"] == [2, None]
    assert sp["forced_eos_token_id"] == [9, None] and sp["exponential_decay_length_penalty"] == [(2, 1.5)] * 2
    assert sp["begin_suppress_tokens"] == [[5, 6]] * 2
    assert _split_row_processors(2, begin_suppress_tokens=[[5], None])["begin_suppress_tokens"] == [[5], None]
    assert _split_row_processors(2, bad_words_ids=[[1, 2], [3]])["bad_words_ids"] == [[[1, 2], [3]]] * 2
    assert _split_row_processors(2, sequence_bias=[[[1, 2], 0.5], [[3], 1.0]])["sequence_bias"] == [[[[1, 2], 0.5], [[3], 1.0]]] * 2
    assert _split_row_processors(2, sequence_bias=[[[[1, 2], 0.5]], None])["sequence_bias"] == [[[[1, 2], 0.5]], None]
    with pytest.raises(ValueError, match=r"`bad_words_ids` has 3 entries for a batch of 2"):
        _split_row_processors(2, bad_words_ids=[None, [[1]], None])
