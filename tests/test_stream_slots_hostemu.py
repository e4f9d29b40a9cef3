"""CPU: per-slot state of the codec's state-carrying decoder, the refill schedule as a packet generator and the wrapper above them, on
the host-emulation build -- the engine's real C++ and the real kernels on the SIMT emulator, the product's Python unmodified
(tests/hostemu/pyshim.py).  The test bodies are those of tests/test_stream_slots_gpu.py (the codec schedule in its reduced form); the
refusals at the end run here only."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
QTTS_ERR_ARG, QTTS_ERR_STATE, QTTS_ERR_LIMIT = -1, -3, -6


@pytest.fixture(scope="module")
def ss():
    sys.path.insert(0, os.path.join(HERE, "hostemu"))
    import pyshim
    pyshim.install()
    try:
        import test_stream_slots_gpu as m
        m._CACHE.clear()
        yield m
    finally:
        m._CACHE.clear()
        pyshim.uninstall()


def test_slots_decode_side_by_side_and_equal_forward(ss):
    ss.body_codec_slots("cpu", ss.REDUCED, 3, ("X", "Y"))


def test_lockstep_rows_equal_stream_push(ss):
    ss.body_lockstep_equals_stream_push("cpu", B=2, T=8)


@pytest.mark.parametrize("graph", [False, True])
def test_refill_stream_packets_concatenate_to_the_reference_codes(ss, golden_dir, graph):
    ss.body_talker_refill_stream("cpu", golden_dir, graph)


def test_stream_custom_voice_takes_the_refill_schedule(ss):
    ss.body_wrapper_refill_stream("cpu")


def test_the_two_entry_points_are_bound(ss):
    from qwen3_tts_amd import _lib
    lib = _lib.load_library()
    assert {"qtts_codec_stream_reset_rows", "qtts_codec_stream_push_rows"} <= set(_lib.SYMBOLS)
    assert lib.qtts_codec_stream_push_rows.argtypes is not None and lib.qtts_codec_stream_reset_rows.restype is C.c_int


def test_refusals_name_the_row_and_change_no_slot(ss):
    """Every refusal of qtts_codec_stream_reset_rows / _push_rows returns its code and its message before anything is launched: after
    each of them the stream's next push gives the bits of an undisturbed run.  The workspace refusal is one that only the carried rows
    of the last decoder block trip -- a push that checked as it went would have refreshed every carry before it by then."""
    from qwen3_tts_amd.codec import CodecDecoderEngine
    c, w, _ = ss._tiny("cpu")
    up, Q = c.total_upsample, c.num_quantizers
    codes = np.random.default_rng(41).integers(0, c.codebook_size, (2, Q, 8))
    big = np.zeros((4, Q, 64), np.int64)

    def session():
        eng = CodecDecoderEngine(c, w, compute_dtype=torch.float32, device="cpu", max_batch=4, max_frames=64)
        lib, h = eng._lib, eng._h
        ids = lambda *r: (C.c_int32 * max(1, len(r)))(*r)
        state = {"t": 0}

        def push():                           # the next frame of slots 2 and 0
            t = state["t"]
            pk, o = np.ascontiguousarray(codes[:, :, t:t + 1]), np.zeros((2, up), np.float32)
            assert lib.qtts_codec_stream_push_rows(h, 2, ids(2, 0), C.c_void_p(pk.ctypes.data), 1, C.c_void_p(o.ctypes.data), None) == 0
            state["t"] = t + 1
            return o
        push_rows = lambda n_rows, row_ids, cd, n: lib.qtts_codec_stream_push_rows(
            h, n_rows, row_ids, C.c_void_p(cd.ctypes.data), n, C.c_void_p(np.zeros((max(1, n_rows), n * up), np.float32).ctypes.data), None)
        reset_rows = lambda n_rows, row_ids: lib.qtts_codec_stream_reset_rows(h, n_rows, row_ids, None)
        return eng, push, push_rows, reset_rows, lambda: (lib.qtts_last_error() or b"").decode()

    eng0, push0, *_ = session()
    eng0.stream_begin(4)
    clean = [push0() for _ in range(8)]

    eng, push, push_rows, reset_rows, err = session()
    one = np.ascontiguousarray(codes[:1, :, :1])
    assert push_rows(1, (C.c_int32 * 1)(0), one, 1) == QTTS_ERR_STATE and "stream_begin() first" in err()
    assert reset_rows(1, (C.c_int32 * 1)(0)) == QTTS_ERR_STATE and "stream_begin() first" in err()
    eng.stream_begin(4)
    got = [push()]
    I = lambda *r: (C.c_int32 * max(1, len(r)))(*r)
    for rc, frag, call in ((QTTS_ERR_ARG, "stream_push_rows: n_rows >= 1", lambda: push_rows(0, I(0), one, 1)),
                           (QTTS_ERR_ARG, "stream_reset_rows: n_rows >= 1", lambda: reset_rows(0, I(0))),
                           (QTTS_ERR_ARG, "stream_push_rows: row 4 is not a row", lambda: push_rows(2, I(2, 4), codes[:, :, :1].copy(), 1)),
                           (QTTS_ERR_ARG, "stream_reset_rows: row -1 is not a row", lambda: reset_rows(2, I(2, -1))),
                           (QTTS_ERR_ARG, "stream_push_rows: row 2: listed twice", lambda: push_rows(2, I(2, 2), codes[:, :, :1].copy(), 1)),
                           (QTTS_ERR_ARG, "stream_reset_rows: row 0: listed twice", lambda: reset_rows(3, I(0, 2, 0))),
                           (QTTS_ERR_LIMIT, "packet + carried rows exceed the workspace", lambda: push_rows(4, I(3, 2, 1, 0), big, 64))):
        assert call() == rc, (frag, err())
        assert frag in err(), (frag, err())
        got.append(push())
    assert len(got) == len(clean)
    for i, (a, b) in enumerate(zip(got, clean)):
        assert np.array_equal(a, b), f"push {i}: a refused call changed a slot"
