"""CPU: codec slots primed from reference codes, and the streaming voice-clone / voice-design wrappers above them, on the host-emulation
build -- the engine's real C++ and the real kernels on the SIMT emulator, the product's Python unmodified (tests/hostemu/pyshim.py).
The test bodies are those of tests/test_stream_clone_gpu.py with reduced plans."""
import ctypes as C
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def sc():
    sys.path.insert(0, os.path.join(HERE, "hostemu"))
    import pyshim
    pyshim.install()
    try:
        import test_stream_clone_gpu as m
        m._CACHE.clear()
        m.ss._CACHE.clear()
        yield m
    finally:
        m._CACHE.clear()
        m.ss._CACHE.clear()
        pyshim.uninstall()


def test_ragged_prime_equals_forward_behind_the_reference(sc):
    sc.body_ragged_prime("cpu", sc.RAGGED_REDUCED, 8)


def test_prime_leaves_neighbours_alone_and_implies_the_reset(sc):
    sc.body_neighbours("cpu", at=(2, 9), ref_lens=(4, 12), n_gen=5)


def test_prime_tail_frames_follow_the_config(sc):
    """The released dims are not built on the emulator: the walk itself is checked on their rates."""
    import synth
    sc.body_tail_frames("cpu")
    assert sc.derive_tail(synth.codec_real()) == 10


def test_refused_primes_name_the_row_and_change_nothing(sc):
    sc.body_refusals("cpu")


def test_the_two_entry_points_are_bound(sc):
    from qwen3_tts_amd import _lib
    lib = _lib.load_library()
    assert {"qtts_codec_stream_prime_rows", "qtts_codec_stream_prime_tail"} <= set(_lib.SYMBOLS)
    assert lib.qtts_codec_stream_prime_rows.argtypes is not None and lib.qtts_codec_stream_prime_tail.restype is C.c_int


def test_stream_voice_clone_equals_generate_voice_clone(sc):
    sc.body_stream_voice_clone("cpu", schedules=(None, "continuous"))       # ("refill" shares their loop; it runs on the GPU)


def test_stream_voice_clone_survives_a_restart(sc):
    sc.body_stream_voice_clone_pooled("cpu")


def test_stream_voice_design_equals_generate_voice_design(sc):
    sc.body_stream_voice_design("cpu")
