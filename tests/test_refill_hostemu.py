"""CPU: requests admitted into finished rows of a running talker stream (qtts_talker_stream_begin_admitting / stream_admit / stream_rows
and the refill schedule above them) on the host-emulation build -- the engine's real C++ and the real kernels on the SIMT emulator, the
product's Python unmodified (tests/hostemu/pyshim.py).  The test bodies are those of tests/test_refill_gpu.py; the refusals at the end
run here only."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
QTTS_ERR_ARG, QTTS_ERR_STATE, QTTS_ERR_LIMIT = -1, -3, -6


@pytest.fixture(scope="module")
def rf():
    sys.path.insert(0, os.path.join(HERE, "hostemu"))
    import pyshim
    pyshim.install()
    try:
        import test_refill_gpu as m
        yield m
    finally:
        pyshim.uninstall()


@pytest.mark.parametrize("graph", [False, True])
def test_refill_gives_every_request_its_reference_codes(rf, golden_dir, graph):
    rf.body_refill_reference("cpu", golden_dir, graph, 128)


@pytest.mark.parametrize("graph", [False, True])
def test_refill_restarts_when_the_shared_position_runs_out(rf, golden_dir, graph):
    rf.body_refill_reference("cpu", golden_dir, graph, 40)


@pytest.mark.parametrize("case", ["pads_pages", "latched", "split_kv"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_admission_edges_at_the_abi(rf, golden_dir, dtype, case):
    rf.body_edges("cpu", golden_dir, dtype, case)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_running_rows_are_not_disturbed_by_an_admission(rf, golden_dir, dtype):
    rf.body_neighbours("cpu", golden_dir, dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_two_identical_refill_runs_are_bit_identical(rf, golden_dir, dtype):
    rf.body_refill_repeatable("cpu", golden_dir, dtype)


@pytest.mark.parametrize("dtype,graph", [(torch.bfloat16, True), (torch.float32, False)])
def test_an_admitted_row_draws_with_its_own_step_counter(rf, golden_dir, dtype, graph):
    rf.body_sampling("cpu", golden_dir, dtype, graph)


def test_bf16_admitted_prefill_is_as_close_to_fp32_as_the_plain_prefill(rf, golden_dir):
    rf.body_bf16_closeness("cpu", golden_dir)


def test_wrapper_takes_the_refill_schedule(rf):
    rf.body_wrapper("cpu")


# ============================================================================================ 7. refusals
def test_refusals_name_the_row_and_change_nothing(rf, golden_dir):
    """Every refusal of qtts_talker_stream_admit returns its code and names the row; after each of them the stream continues, and in the
    end the running rows and a request admitted after all the refusals have the reference's codes, as in an undisturbed run."""
    g, t, w, args = rf._fixture(golden_dir)
    gga = rf.gga
    eng = rf._engine(t, w, "cpu", torch.float32, False, 4, 40)
    lib, h = eng._lib, eng._h
    err = lambda: (lib.qtts_last_error() or b"").decode()
    limits = {0: 3, 2: 3}
    settings = rf._greedy_settings(limits)
    emb, _, trail, _ = args
    T = emb.shape[1]

    def admit(rows_, reqs, Tg=None, trail_rows=None, **over):
        Tg = Tg or max(rf.LENS[i] for i in reqs)
        e = emb[reqs][:, T - Tg:].contiguous()
        tr = (trail[reqs] if trail_rows is None else trail[reqs].repeat(1, 2, 1)[:, :trail_rows]).contiguous()
        tab = rf._table([dict(settings[i], **over) for i in reqs])
        return lib.qtts_talker_stream_admit(h, len(reqs), (C.c_int32 * len(reqs))(*rows_), C.c_void_p(e.data_ptr()), Tg,
                                            (C.c_int32 * len(reqs))(*[Tg - rf.LENS[i] for i in reqs]), C.c_void_p(tr.data_ptr()), tr.shape[1], tab, None)

    # no admitting stream open: nothing at all, then a plain table stream
    assert admit([1], [8]) == QTTS_ERR_STATE and "no admitting stream" in err()
    s = rf.Stream(eng, t, args, [1, 0, 2, 4], settings)
    assert s.step(2) == (2, False) and s.retire() == [1, 2]
    assert s.rows()[2] == 12
    state = s.rows()
    for rc, frag, call in ((QTTS_ERR_ARG, "row 4 is not a row", lambda: admit([4], [8])),
                           (QTTS_ERR_ARG, "row 2: listed twice", lambda: admit([2, 2], [8, 6])),
                           (QTTS_ERR_ARG, "row 3: its occupant is still unfinished", lambda: admit([1, 3], [8, 6])),
                           (QTTS_ERR_LIMIT, "row 2: the prompt (13 rows", lambda: admit([1, 2], [8, 7])),
                           (QTTS_ERR_LIMIT, "row 1: the stream's position (12) + max_new_tokens (29) exceeds max_seq", lambda: admit([1], [8], max_new_tokens=29)),
                           (QTTS_ERR_LIMIT, "row 1: max_new_tokens (14) exceeds the stream's max_row_tokens (13)", lambda: admit([1], [8], max_new_tokens=14)),
                           (QTTS_ERR_LIMIT, "row 2: trailing rows (3) exceed", lambda: admit([2], [8], trail_rows=3)),
                           (QTTS_ERR_ARG, "row 1: temperature must be > 0", lambda: admit([1], [8], temperature=0.0)),
                           (QTTS_ERR_ARG, "row 2: top_p must be in (0, 1]", lambda: admit([2], [6], do_sample=1, top_p=0.0)),
                           (QTTS_ERR_ARG, "row 1: max_new_tokens >= 1", lambda: admit([1], [8], max_new_tokens=0))):
        assert call() == rc, (frag, err())
        assert frag in err(), (frag, err())
        assert s.rows() == state and eng.stats()["admit_calls"] == 0, frag
    assert s.step(1) == (3, False)
    assert admit([1], [8]) == 0, err()
    s.slot[1] = 8
    s.finish()
    assert eng.stats()["admit_calls"] == 1 and sorted(s.out) == [0, 1, 2, 4, 8]
    for r, codes in s.out.items():
        rf._check_request(g, t, codes, r, limits.get(r, gga.MAX_NEW))
    # a stream begun without admission refuses too
    out = list(eng.generate_stream(*[a[:4] for a in args[:3]], args[3], packet_frames=2, max_new_tokens=[3] * 4, min_new_tokens=2,
                                   do_sample=False, subtalker_dosample=False, suppress_tokens=rf._suppress(t)))
    assert len(out) >= 1
    assert admit([1], [8]) == QTTS_ERR_STATE


def test_stats_layout_carries_the_admission_counters(tmp_path):
    """`_lib.TalkerStatsC` against `qtts_talker_stats` of include/qtts.h as gcc lays it out, the two ABI v15 fields included."""
    import subprocess
    from qwen3_tts_amd import _lib
    hdr_path = os.path.join(os.path.dirname(HERE), "include", "qtts.h")
    names = [f[0] for f in _lib.TalkerStatsC._fields_]
    assert "admit_calls" in names and "admitted_rows" in names and _lib.ABI_VERSION == 15
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{hdr_path}"', 'int main(void) {', 'printf("size %zu\\n", sizeof(qtts_talker_stats));']
    lines += [f'printf("{f} %zu\\n", offsetof(qtts_talker_stats, {f}));' for f in names]
    lines += ['return 0; }']
    (tmp_path / "probe.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-o", str(tmp_path / "probe"), str(tmp_path / "probe.c")], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(tmp_path / "probe")], capture_output=True, text=True, check=True).stdout.splitlines())
    assert C.sizeof(_lib.TalkerStatsC) == int(got["size"])
    for f in names:
        assert getattr(_lib.TalkerStatsC, f).offset == int(got[f]), f
