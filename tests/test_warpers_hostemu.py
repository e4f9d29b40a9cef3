"""CPU: the talker's remaining HF sampling controls (qtts_talker_set_row_warpers, sample_warp_kernel and the Python above them) on the
host-emulation build -- the engine's real C++ and sampling.hip's real kernels on the SIMT emulator, the product's Python unmodified
(tests/hostemu/pyshim.py).  The test bodies are those of tests/test_warpers_gpu.py; the refusals, the layout and the host logic at the
end need no GPU at all."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
QTTS_ERR_ARG = -1


@pytest.fixture(scope="module")
def wp():
    sys.path.insert(0, os.path.join(HERE, "hostemu"))
    import pyshim
    pyshim.install()
    try:
        import test_warpers_gpu as m
        yield m
    finally:
        pyshim.uninstall()


@pytest.mark.parametrize("graph", [False, True])
def test_greedy_ngram_bans_are_the_reference_run(wp, golden_dir, graph):
    wp.body_greedy_ngram("cpu", golden_dir, graph)


def test_ngram_bans_through_stream_packets_and_the_continuous_schedule(wp, golden_dir):
    wp.body_ngram_streams("cpu", golden_dir)


@pytest.mark.parametrize("dtype,graph,B", [(torch.bfloat16, True, 4), (torch.float32, False, 8)])
def test_every_row_draws_under_its_own_warpers(wp, dtype, graph, B):
    wp.body_draws("cpu", *wp.rs._tiny(), dtype, graph, B, wp.VALUES_TINY)


def test_a_warper_rows_codes_do_not_depend_on_place_or_neighbours(wp):
    wp.body_place("cpu")


def test_a_warper_request_admitted_into_a_stream_that_ran_without_any(wp):
    wp.body_admitted_warper("cpu")


def test_a_preempted_warper_request_restarts_to_the_same_codes(wp):
    wp.body_pooled_restart("cpu")


# ============================================================================================ refusals, layout, host logic
def test_python_refusals_use_hfs_wording(wp):
    t, w = wp.rs._tiny()
    B = 4
    eng = wp.rs._engine(t, w, "cpu", torch.float32, False, B, max_seq=32)
    args, _ = wp.rs._prompt(t, B)
    kw = dict(max_new_tokens=4, min_new_tokens=2, suppress_tokens=wp._suppress(t), seed=3)
    for bad, msg in ((dict(min_p=1.5), r"`min_p` has to be a float in the \[0, 1\] interval, but is 1.5"),
                     (dict(min_p=[0.1, -0.2, 0, 0]), r"`min_p` has to be a float in the \[0, 1\] interval, but is -0.2"),
                     (dict(typical_p=-0.5), r"`typical_p` has to be a float > 0 and < 1, but is -0.5"),
                     (dict(typical_p=[0.5, 0.0, 0.5, 0.5]), r"`typical_p` has to be a float > 0 and < 1, but is 0.0"),
                     (dict(no_repeat_ngram_size=2.5), r"`ngram_size` has to be a strictly positive integer, but is 2.5"),
                     (dict(epsilon_cutoff=[0.1, 0.1]), r"`epsilon_cutoff` has 2 entries for a batch of 4"),
                     (dict(min_p=0.1, teacher_codes=torch.zeros(B, 3, t.num_code_groups, dtype=torch.long)), r"teacher_codes takes scalar")):
        with pytest.raises(ValueError, match=msg):
            eng.generate(*args, **{**kw, **bad})
        if "teacher_codes" not in bad:
            with pytest.raises(ValueError, match=msg):
                list(eng.generate_stream(*args, **{**kw, **bad}))
            with pytest.raises(ValueError, match=msg):
                eng.generate(*args, schedule="continuous", **{**kw, **bad})
    # gating: values that are off leave the call on the scalar path; one that is on forces the table with seeds s + b
    off = eng.generate(*args, min_p=0, typical_p=1.0, epsilon_cutoff=1.5, eta_cutoff=0.0, no_repeat_ngram_size=0, **kw)
    assert eng.sampler_class() == (0, 0) and eng.stats()["row_table_last"] == 0
    plain = eng.generate(*args, **kw)
    assert np.array_equal(off.codes.numpy(), plain.codes.numpy())
    on = eng.generate(*args, min_p=0.3, **kw)
    assert eng.sampler_class() == (3, 1) and eng.stats()["row_table_last"] == 1
    listed = eng.generate(*args, min_p=[0.3] * B, **dict(kw, seed=[3, 4, 5, 6]))
    assert np.array_equal(on.codes.numpy(), listed.codes.numpy())


def test_c_abi_refusals_leave_the_engine_usable(wp):
    """A bad value fails at set time and names the row; a count mismatch at the consuming call, a scalar call with a pending table and a
    table together with teacher forcing fail -- QTTS_ERR_ARG each, nothing changed: the same prefill then still generates."""
    from qwen3_tts_amd import _lib
    from test_row_sampling_hostemu import _rows
    t, w = wp.rs._tiny()
    B = 4
    eng = wp.rs._engine(t, w, "cpu", torch.float32, False, B, max_seq=32)
    (emb, mask, trail, pad), _ = wp.rs._prompt(t, B)
    lib, h = eng._lib, eng._h
    T = emb.shape[1]
    embc, trc, padc = emb.contiguous(), trail.contiguous(), pad.reshape(-1).contiguous()
    npad = (C.c_int32 * B)(*[int(x) for x in (1 - mask).sum(-1)])
    sup = wp._suppress(t)
    sup_c = (C.c_int32 * len(sup))(*sup)
    codes = torch.zeros(B, 3, t.num_code_groups, dtype=torch.int64)
    nf = C.c_int32(0)
    err = lambda: (lib.qtts_last_error() or b"").decode()
    _lib.check(lib.qtts_talker_prefill(h, C.c_void_p(embc.data_ptr()), B, T, npad, C.c_void_p(trc.data_ptr()), trc.shape[1],
                                       C.c_void_p(padc.data_ptr()), None))

    def warpers(n, **over):
        ws = (_lib.RowWarpersC * n)()
        for k, (b, v) in over.items():
            setattr(ws[b], k, v)
        return ws

    def call(rows, n):
        return lib.qtts_talker_generate_rows(h, rows, n, t.codec_eos_token_id, sup_c, len(sup), C.c_void_p(codes.data_ptr()), None, None,
                                             C.byref(nf), None)

    for over, what in ((dict(min_p=(2, 1.5)), "row 2: min_p"), (dict(min_p=(0, -0.1)), "row 0: min_p"), (dict(typical_p=(1, 1.01)), "row 1: typical_p"),
                       (dict(epsilon_cutoff=(3, 1.0)), "row 3: epsilon_cutoff"), (dict(eta_cutoff=(0, -1e-3)), "row 0: eta_cutoff"),
                       (dict(no_repeat_ngram_size=(1, -1)), "row 1: no_repeat_ngram_size"), (dict(min_p=(1, float("nan"))), "row 1: min_p")):
        assert lib.qtts_talker_set_row_warpers(h, warpers(B, **over), B) == QTTS_ERR_ARG and what in err(), (over, err())
    assert lib.qtts_talker_set_row_warpers(h, warpers(B), B + 1) == QTTS_ERR_ARG
    # a count mismatch at the consuming call; the table is dropped, so the call after it runs without one
    assert lib.qtts_talker_set_row_warpers(h, warpers(B - 1, min_p=(0, 0.5)), B - 1) == 0
    assert call(_rows(B), B) == QTTS_ERR_ARG and "pending warper table" in err()
    # a scalar call with a pending table
    assert lib.qtts_talker_set_row_warpers(h, warpers(B, min_p=(0, 0.5)), B) == 0
    sp = _lib.SamplingC(1, 50, 1.0, 0.9, 1.05, 1, 50, 1.0, 0.9, 3)
    assert lib.qtts_talker_generate(h, C.byref(sp), 4, 2, t.codec_eos_token_id, sup_c, len(sup), C.c_void_p(codes.data_ptr()), None, None,
                                    C.byref(nf), None) == QTTS_ERR_ARG and "warper table is pending" in err()
    assert lib.qtts_talker_set_row_warpers(h, warpers(B, min_p=(0, 0.5)), B) == 0
    assert lib.qtts_talker_stream_begin(h, C.byref(sp), 4, 2, t.codec_eos_token_id, sup_c, len(sup), C.c_void_p(codes.data_ptr()), None,
                                        None) == QTTS_ERR_ARG and "warper table is pending" in err()
    # NULL / 0 clears
    assert lib.qtts_talker_set_row_warpers(h, warpers(B - 1), B - 1) == 0 and lib.qtts_talker_set_row_warpers(h, None, 0) == 0
    # teacher forcing refuses the table call
    tc = torch.zeros(B, 3, t.num_code_groups, dtype=torch.long)
    own = torch.zeros(B, 4, t.num_code_groups, dtype=torch.int32)
    _lib.check(lib.qtts_talker_set_teacher(h, C.c_void_p(tc.data_ptr()), 3, C.c_void_p(own.data_ptr()), None, None))
    try:
        assert lib.qtts_talker_set_row_warpers(h, warpers(B, min_p=(0, 0.5)), B) == 0
        assert call(_rows(B), B) == QTTS_ERR_ARG and "teacher forcing" in err()
    finally:
        _lib.check(lib.qtts_talker_set_teacher(h, None, 0, None, None, None))
    # every refusal left the prefill in place and no table pending: the call runs in the plain class, and equals the Python call
    assert call(_rows(B), B) == 0, err()
    assert eng.sampler_class() == (1, 1)
    again = eng.generate(emb, mask, trail, pad, max_new_tokens=4, min_new_tokens=2, suppress_tokens=sup, seed=[5, 6, 7, 8])
    assert np.array_equal(codes[:, :nf.value].numpy(), again.codes.numpy())
    # a table with every field off is exactly the call without the table
    _lib.check(lib.qtts_talker_prefill(h, C.c_void_p(embc.data_ptr()), B, T, npad, C.c_void_p(trc.data_ptr()), trc.shape[1],
                                       C.c_void_p(padc.data_ptr()), None))
    assert lib.qtts_talker_set_row_warpers(h, warpers(B), B) == 0 and call(_rows(B), B) == 0 and eng.sampler_class() == (1, 1)
    assert np.array_equal(codes[:, :nf.value].numpy(), again.codes.numpy())


def test_row_warpers_ctypes_layout_matches_the_header(tmp_path):
    """`_lib.RowWarpersC` against `qtts_row_warpers` of include/qtts.h as gcc lays it out; the two new symbols are declared and listed;
    the ABI version stays 15."""
    import re
    import subprocess
    from qwen3_tts_amd import _lib
    hdr_path = os.path.join(os.path.dirname(HERE), "include", "qtts.h")
    text = open(hdr_path).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    body = re.search(r"typedef struct qtts_row_warpers\s*\{(.*?)\}\s*qtts_row_warpers\s*;", hdr, flags=re.S).group(1)
    names = [re.findall(r"([A-Za-z_][A-Za-z_0-9]*)\s*(?:\[\d+\])?\s*$", d.strip())[0] for d in body.split(";") if d.strip()]
    assert names == [f[0] for f in _lib.RowWarpersC._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{hdr_path}"', 'int main(void) {',
             'printf("size %zu\\n", sizeof(qtts_row_warpers));', 'printf("abi %d\\n", QTTS_ABI_VERSION);']
    lines += [f'printf("{f} %zu\\n", offsetof(qtts_row_warpers, {f}));' for f in names]
    lines += ['return 0; }']
    (tmp_path / "probe.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-o", str(tmp_path / "probe"), str(tmp_path / "probe.c")], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(tmp_path / "probe")], capture_output=True, text=True, check=True).stdout.splitlines())
    assert C.sizeof(_lib.RowWarpersC) == int(got["size"]) == 32
    for f in names:
        assert getattr(_lib.RowWarpersC, f).offset == int(got[f]), f
    assert int(got["abi"]) == _lib.ABI_VERSION == 15
    for s in ("qtts_talker_set_row_warpers", "qtts_talker_sampler_class"):
        assert s in _lib.SYMBOLS and re.search(r"\bint " + s + r"\(", hdr)


def test_merge_generate_kwargs_passes_the_warpers_through():
    from qwen3_tts_amd.model import Qwen3TTSModel
    m = Qwen3TTSModel.__new__(Qwen3TTSModel)
    m.generate_defaults = {"min_p": 0.05}
    out = m._merge_generate_kwargs(min_p=[None, 0.2], typical_p=[0.9, None], no_repeat_ngram_size=3, seed=[1, 2])
    assert out["min_p"] == [0.05, 0.2] and out["typical_p"] == [0.9, None] and out["no_repeat_ngram_size"] == 3
    assert "epsilon_cutoff" not in out and "eta_cutoff" not in out
    assert m._merge_generate_kwargs()["min_p"] == 0.05
    m.generate_defaults = {}
    assert "min_p" not in m._merge_generate_kwargs(top_k=5)


def test_wrapper_passes_the_warpers_to_the_engine(wp):
    wp.body_wrapper("cpu")
