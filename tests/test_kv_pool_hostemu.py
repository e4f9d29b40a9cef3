"""CPU: the shared KV page pool (qtts_talker_set_kv_pool / stream_kv / stream_evict and the optimistic continuous schedule above them) on
the host-emulation build -- the engine's real C++ and the real kernels on the SIMT emulator, the product's Python unmodified
(tests/hostemu/pyshim.py).  The test bodies are those of tests/test_kv_pool_gpu.py; the hand-driven ones run under three wave
scheduling orders of the emulator."""
import ctypes as C
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def kp():
    sys.path.insert(0, os.path.join(HERE, "hostemu"))
    import pyshim
    pyshim.install()
    try:
        import test_kv_pool_gpu as m
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
def test_a_pool_of_the_static_size_is_the_static_engine(kp, golden_dir, graph):
    kp.body_static_size("cpu", golden_dir, graph)


@pytest.mark.parametrize("order", [0, 1, 2], indirect=True)
def test_a_step_the_pool_cannot_cover_is_refused_and_eviction_frees_it(kp, golden_dir, order):
    kp.body_exhaustion("cpu", golden_dir, order != 1)


@pytest.mark.parametrize("order,dtype", [(0, torch.float32), (1, torch.bfloat16), (2, torch.float32)], indirect=["order"])
def test_a_finished_row_idles_into_the_sink_while_a_neighbour_takes_its_pages(kp, golden_dir, order, dtype):
    kp.body_sink("cpu", golden_dir, dtype)


@pytest.mark.parametrize("order,dtype", [(0, torch.float32), (1, torch.bfloat16), (2, torch.float32)], indirect=["order"])
def test_split_kv_reads_a_scattered_table(kp, golden_dir, order, dtype):
    kp.body_split_kv("cpu", golden_dir, dtype)


def test_the_general_attention_family_reads_a_scattered_table(kp, golden_dir):
    kp.body_split_kv("cpu", golden_dir, torch.float32, gq=True)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_another_head_shape_reads_a_scattered_table(kp, golden_dir, dtype):
    """(8 frames here, as tests/test_attn_gq_hostemu.py runs these fixtures on the emulator; the GPU test runs all 39)"""
    kp.body_gq_head_shape("cpu", golden_dir, dtype, 9)


@pytest.mark.parametrize("graph", [False, True])
def test_the_continuous_schedule_preempts_by_restart_under_a_tight_pool(kp, golden_dir, graph):
    kp.body_scheduler("cpu", golden_dir, graph)


def test_scalar_paths_reserve_their_worst_case_and_bad_calls_are_refused(kp, golden_dir):
    kp.body_scalar_and_refusals("cpu", golden_dir)


def test_streamed_audio_survives_a_restart_without_a_repeated_sample(kp):
    kp.body_audio("cpu")
