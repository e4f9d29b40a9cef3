"""CPU: per-row KV positions (qtts_talker_stream_begin_admitting_rows / stream_row_lens and the continuous schedule above them) on the
host-emulation build -- the engine's real C++ and the real kernels on the SIMT emulator, the product's Python unmodified
(tests/hostemu/pyshim.py).  The test bodies are those of tests/test_row_positions_gpu.py.  The hand-driven cases -- a long prompt into a
young stream, the edges, split-KV with rows of very different lengths -- run under three wave scheduling orders of the emulator."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def rp():
    sys.path.insert(0, os.path.join(HERE, "hostemu"))
    import pyshim
    pyshim.install()
    try:
        import test_row_positions_gpu as m
        yield m
    finally:
        pyshim.uninstall()


@pytest.fixture
def order(request):
    """the emulator's fiber order for one test (0: as launched, 1 / 2: two other wave schedules)"""
    from qwen3_tts_amd import _lib
    emu = _lib.load_library()
    emu.hostemu_set_fiber_order.argtypes = [C.c_int32]
    emu.hostemu_set_fiber_order.restype = None
    emu.hostemu_set_fiber_order(request.param)
    try:
        yield request.param
    finally:
        emu.hostemu_set_fiber_order(0)


@pytest.mark.parametrize("graph", [False, True])
def test_one_stream_serves_every_request_on_recycled_positions(rp, golden_dir, graph):
    rp.body_continuous_reference("cpu", golden_dir, graph)


def test_clamped_limits_still_open_a_full_width_stream(rp, golden_dir):
    rp.body_clamped_limits("cpu", golden_dir, True)


def test_widest_opener():
    """`TalkerEngine._widest_opener` (no device): all fit behind the longest prompt -> the longest max_batch; limits clamped to their own
    room -> the most frequent length; a long prompt with a long limit does not keep the others out."""
    from qwen3_tts_amd.talker import TalkerEngine
    pick = TalkerEngine._widest_opener
    lens = [15, 14, 14, 13, 5, 5, 5, 3]
    q = list(range(8))
    assert pick(q, lens, [13] * 8, 32, 4) == [0, 1, 2, 3]
    assert pick(q, lens, [32 - x for x in lens], 32, 4) == [4, 5, 6]
    assert pick(q, lens, [17, 3, 3, 3, 3, 3, 3, 3], 32, 4) == [0, 1, 2, 3]
    assert pick(q, lens, [17, 18, 3, 3, 3, 3, 3, 3], 32, 4) == [0, 2, 3, 4]
    assert pick(q, lens, [17, 18, 18, 19, 3, 3, 3, 3], 32, 8) == [1, 2, 4, 5, 6, 7]


def test_the_general_attention_family_reads_per_row_lengths(rp, golden_dir):
    rp.body_continuous_reference("cpu", golden_dir, True, gq=True)


@pytest.mark.parametrize("order", [0, 1, 2], indirect=True)
def test_a_long_prompt_enters_a_young_stream(rp, golden_dir, order):
    rp.body_long_prompt("cpu", golden_dir, order != 1)


@pytest.mark.parametrize("order,dtype", [(0, torch.float32), (1, torch.bfloat16), (2, torch.float32)], indirect=["order"])
def test_row_position_edges_at_the_abi(rp, golden_dir, order, dtype):
    rp.body_edges("cpu", golden_dir, dtype, graph=order != 2)


@pytest.mark.parametrize("order,dtype", [(0, torch.float32), (1, torch.bfloat16), (2, torch.float32)], indirect=["order"])
def test_split_kv_with_rows_of_very_different_lengths(rp, golden_dir, order, dtype):
    rp.body_split_kv("cpu", golden_dir, dtype)


@pytest.mark.parametrize("gq", [False, True])
def test_bf16_continuous_stream(rp, golden_dir, gq):
    rp.body_bf16("cpu", golden_dir, gq)


@pytest.mark.parametrize("dtype,graph", [(torch.bfloat16, True), (torch.float32, False)])
def test_sampled_rows_draw_with_their_own_step_wherever_they_are_admitted(rp, golden_dir, dtype, graph):
    rp.body_sampling("cpu", golden_dir, dtype, graph)


def test_continuous_stream_packets_concatenate_to_the_reference_codes(rp, golden_dir):
    rp.body_stream_packets("cpu", golden_dir, True)


def test_stream_custom_voice_takes_the_continuous_schedule(rp):
    rp.body_wrapper("cpu")


def test_the_entry_points_are_declared_and_bound_and_the_stats_struct_keeps_its_layout(rp, tmp_path):
    """The header declares the three entry points and the binding names them; `qtts_talker_stats` is what it was under ABI 15 -- the
    same fields, `_lib.TalkerStatsC` as gcc lays the header's struct out -- and the mode's two figures come through `stats()` from
    qtts_talker_stream_mode."""
    from qwen3_tts_amd import _lib
    lib = _lib.load_library()
    hdr_path = os.path.join(os.path.dirname(HERE), "include", "qtts.h")
    hdr = open(hdr_path).read()
    for s in ("qtts_talker_stream_begin_admitting_rows", "qtts_talker_stream_row_lens", "qtts_talker_stream_mode"):
        assert s in _lib.SYMBOLS and f"int {s}(" in hdr and getattr(lib, s).restype is C.c_int
    names = [f[0] for f in _lib.TalkerStatsC._fields_]
    assert names[-4:] == ["admit_calls", "admitted_rows", "row_table_last", "graph_captures"] and _lib.ABI_VERSION == 15
    assert "row_positions" not in names and "max_row_len" not in names
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{hdr_path}"', 'int main(void) {', 'printf("size %zu\\n", sizeof(qtts_talker_stats));']
    lines += [f'printf("{f} %zu\\n", offsetof(qtts_talker_stats, {f}));' for f in names]
    lines += ['return 0; }']
    (tmp_path / "probe.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-o", str(tmp_path / "probe"), str(tmp_path / "probe.c")], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(tmp_path / "probe")], capture_output=True, text=True, check=True).stdout.splitlines())
    assert C.sizeof(_lib.TalkerStatsC) == int(got["size"])
    for f in names:
        assert getattr(_lib.TalkerStatsC, f).offset == int(got[f]), f
