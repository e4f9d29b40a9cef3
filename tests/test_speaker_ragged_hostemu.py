"""CPU: `qtts_speaker_embed_ragged` and the Python above it on the host-emulation build -- the engine's real C++ and the real kernels on
the SIMT emulator, the product's Python unmodified (tests/hostemu/pyshim.py).  The test bodies are those of
tests/test_speaker_ragged_gpu.py; the kernel-level ones run with `hostemu_set_real_gemm(1)`, so gemm_tap.hip itself computes the packed
GEMMs (rows of several clips in one tile, taps that reach across a clip's first row).  The emulator fills fresh device memory with 0xFF
bytes: a read past a clip's end shows as a NaN, which the bodies look for.  The released dims (case 5) are GPU only: too slow here."""
import contextlib
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
FULL = os.environ.get("QTTS_HOSTEMU_FULL") == "1"


@pytest.fixture(scope="module")
def sr():
    sys.path.insert(0, os.path.join(HERE, "hostemu"))
    import pyshim
    pyshim.install()
    try:
        import test_speaker_ragged_gpu as m
        m._CACHE.clear()
        yield m
    finally:
        m._CACHE.clear()
        pyshim.uninstall()


@contextlib.contextmanager
def real_gemm():
    from qwen3_tts_amd import _lib
    lib = _lib.load_library()
    lib.hostemu_set_real_gemm(1)
    try:
        yield
    finally:
        lib.hostemu_set_real_gemm(1 if FULL else 0)


def test_ragged_batch_equals_the_oracle_clip_by_clip(sr):
    with real_gemm():
        sr.body_vs_oracle("cpu")


def test_a_clip_does_not_see_its_neighbours(sr):
    with real_gemm():
        sr.body_neighbours("cpu")


def test_ragged_batch_bf16_engine(sr):
    with real_gemm():
        sr.body_bf16("cpu")


def test_refused_batches_name_the_clip_and_change_nothing(sr):
    with real_gemm():
        sr.body_refusals("cpu")


def test_embed_many_takes_the_ragged_path(sr):
    sr.body_embed_many_paths("cpu")


def test_create_voice_clone_prompt_embeds_ragged_clips_in_one_call(sr):
    sr.body_voice_clone_prompt("cpu")


def test_the_entry_point_is_bound(sr):
    sr.body_binding()
