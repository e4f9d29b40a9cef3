"""CPU, no library: the host logic of `Qwen3TTSModel.stream_voice_clone` / `stream_voice_design` on stand-in model objects -- the errors of
`generate_voice_clone` / `generate_voice_design` (qwen3_tts_model.py:460-700), the slot rule of `stream_custom_voice`, and the packet
loop's priming: which rows are primed, which are reset, with what, and in how many calls."""
import types

import numpy as np
import pytest
import torch

from qwen3_tts_amd.model import Qwen3TTSModel, VoiceClonePromptItem
from qwen3_tts_amd.talker import RefillPacket, RefillRow

UP, Q = 4, 2


class _Decoder:
    """records what the packet loop asks of the codec; a pushed frame becomes UP samples of its first code"""
    def __init__(self, max_batch):
        self.max_batch = max_batch
        self.config = types.SimpleNamespace(codebook_size=64)
        self.calls = []

    def stream_begin(self, rows):
        self.calls.append(("begin", rows))

    def stream_reset_rows(self, ids):
        self.calls.append(("reset", list(ids)))

    def stream_prime_rows(self, ids, codes, n_frames):
        self.calls.append(("prime", list(ids), codes.clone(), list(n_frames)))

    def stream_push_rows(self, ids, codes):
        self.calls.append(("push", list(ids)))
        return codes[:, :1, :].float().repeat_interleave(UP, dim=-1)


class _Proc:
    def __call__(self, text=None, return_tensors="pt", padding=True):
        return {"input_ids": torch.tensor([[1, 2, 3, 4, 5, 6, 7, 8, 9, 10]])}


def _model(kind, records=None, talker_rows=2, codec_rows=2):
    dec = _Decoder(codec_rows)

    class M:
        device = torch.device("cpu")
        tts_model_type, tts_model_size, tokenizer_type = kind, "1b7", "12hz"
        talker = types.SimpleNamespace(max_batch=talker_rows)
        speech_tokenizer = types.SimpleNamespace(model=types.SimpleNamespace(decoder=dec, output_sample_rate=24000))
        seen = {}

        def get_supported_languages(self): return ["auto", "english"]
        def get_supported_speakers(self): return None

        def generate_stream(self, **kw):
            M.seen = kw
            yield from records
    return Qwen3TTSModel(M(), _Proc(), generate_defaults={}), dec, M


def _item(n):
    return VoiceClonePromptItem(ref_code=None if n is None else torch.arange(n * Q).reshape(n, Q) % 60, ref_spk_embedding=torch.zeros(8),
                                x_vector_only_mode=n is None, icl_mode=n is not None, ref_text=None if n is None else "ref")


def test_wrong_model_type_raises_the_reference_message():
    w, _, _ = _model("custom_voice")
    with pytest.raises(ValueError, match="does not support stream_voice_clone, Please check Model Card"):
        next(w.stream_voice_clone("hi", voice_clone_prompt=[_item(3)]))
    with pytest.raises(ValueError, match="does not support stream_voice_design, Please check Model Card"):
        next(w.stream_voice_design("hi", "a voice"))


def test_batch_size_mismatches_raise_the_messages_of_the_one_shot_calls():
    w, dec, _ = _model("base")
    with pytest.raises(ValueError, match=r"Batch size mismatch: text=2, language=3"):
        next(w.stream_voice_clone(["a", "b"], language=["english"] * 3, voice_clone_prompt=[_item(3)]))
    with pytest.raises(ValueError, match=r"Batch size mismatch: prompt=2, text=3"):
        next(w.stream_voice_clone(["a", "b", "c"], voice_clone_prompt=[_item(3), _item(None)]))
    with pytest.raises(ValueError, match="Either `voice_clone_prompt` or `ref_audio` must be provided."):
        next(w.stream_voice_clone("a"))
    with pytest.raises(ValueError, match="Unsupported languages"):
        next(w.stream_voice_clone("a", language="klingon", voice_clone_prompt=[_item(3)]))
    assert dec.calls == []                                      # refused before the codec is touched
    d, _, _ = _model("voice_design")
    with pytest.raises(ValueError, match=r"Batch size mismatch: text=3, language=3, instruct=2"):
        next(d.stream_voice_design(["a", "b", "c"], ["x", "y"]))


@pytest.mark.parametrize("schedule", [None, "refill", "continuous"])
def test_a_codec_with_fewer_slots_than_talker_rows_is_refused(schedule):
    w, dec, _ = _model("base", talker_rows=2, codec_rows=1)
    with pytest.raises(ValueError, match=r"stream_voice_clone\(schedule=.*\): the codec decoder's max_batch \(1\) is smaller than the talker's \(2\)"):
        next(w.stream_voice_clone("a", voice_clone_prompt=[_item(3)], schedule=schedule))
    d, _, _ = _model("voice_design", talker_rows=2, codec_rows=1)
    with pytest.raises(ValueError, match=r"stream_voice_design\(schedule=.*\): the codec decoder's max_batch \(1\) is smaller"):
        next(d.stream_voice_design("a", "x", schedule=schedule))
    assert dec.calls == []


def _row(request, row, frames, first=False, last=False, restart=False):
    return RefillRow(request=request, row=row, codes=torch.full((frames, Q), 10 + request), first=first, last=last, restart=restart)


def test_rows_that_start_together_are_primed_in_one_call_and_a_restart_is_primed_again():
    """Requests 0 (5 reference frames) and 1 (2) start in one packet: ONE prime call, right-aligned in a block of 5 columns; request 2 has no
    reference codes (x-vector only): its row is reset.  Request 0 is preempted after 4 frames and starts again: its slot is primed
    again, the 4 replayed frames are not delivered twice."""
    records = [RefillPacket([_row(0, 1, 2, first=True), _row(1, 0, 2, first=True)]),
               RefillPacket([_row(0, 1, 2), _row(1, 0, 1, last=True)]),
               RefillPacket([_row(2, 0, 2, first=True)]),
               RefillPacket([_row(0, 1, 2, first=True, restart=True), _row(2, 0, 2)]),
               RefillPacket([_row(0, 1, 2), _row(2, 0, 0, last=True)]),
               RefillPacket([_row(0, 1, 1, last=True)])]
    w, dec, M = _model("base", records)
    out = list(w.stream_voice_clone(["a", "b", "c"], voice_clone_prompt=[_item(5), _item(2), _item(None)], schedule="continuous", packet_frames=2))
    assert M.seen["schedule"] == "continuous" and M.seen["packet_frames"] == 2 and M.seen["voice_clone_prompt"]["ref_code"][2] is None
    kinds = [c[0] for c in dec.calls]
    assert kinds == ["begin", "prime", "push", "push", "reset", "push", "prime", "push", "push", "push"], kinds
    _, ids, block, lens = dec.calls[1]
    assert ids == [1, 0] and lens == [5, 2] and tuple(block.shape) == (2, Q, 5)
    assert torch.equal(block[0], _item(5).ref_code.T) and torch.equal(block[1, :, 3:], _item(2).ref_code.T)
    assert dec.calls[4] == ("reset", [0])
    _, ids, block, lens = dec.calls[6]
    assert ids == [1] and lens == [5] and torch.equal(block[0], _item(5).ref_code.T)
    assert all(sr == 24000 and len(p) == 3 for p, sr in out)
    total = [sum(p[i].shape[0] for p, _ in out) for i in range(3)]
    assert total == [5 * UP, 3 * UP, 4 * UP], total             # request 0: 4 frames, replayed (2 + 2 silent), then 1 more
    assert [p[0].shape[0] for p, _ in out] == [2 * UP, 2 * UP, 0, 0, 0, UP]
    assert all(a.dtype == np.float32 for p, _ in out for a in p)


def test_the_default_schedule_runs_waves_of_the_talkers_rows():
    """schedule=None: three requests on two rows are two waves; per-request sequences are sliced per wave, every request of a wave is
    primed with its own reference in that wave's first packet, and a later wave's requests are empty until their wave runs."""
    waves = []

    def records_for(kw):
        n = len(kw["input_ids"])
        waves.append(kw)
        yield [torch.full((2, Q), 20 + i) for i in range(n)]
        yield [torch.full((1 if i == 0 else 2, Q), 20 + i) for i in range(n)]      # request 0 of the wave hit eos inside the packet

    w, dec, M = _model("base")
    M.generate_stream = lambda self, **kw: records_for(kw)
    out = list(w.stream_voice_clone(["a", "b", "c"], voice_clone_prompt=[_item(5), _item(None), _item(3)], packet_frames=2,
                                    seed=[7, 8, 9], max_new_tokens=[4, 5, 6]))
    assert [len(k["input_ids"]) for k in waves] == [2, 1] and [k["seed"] for k in waves] == [[7, 8], [9]]
    assert [k["max_new_tokens"] for k in waves] == [[4, 5], [6]] and all("schedule" not in k for k in waves)
    assert waves[1]["voice_clone_prompt"]["ref_code"][0].shape[0] == 3 and waves[1]["languages"] == ["Auto"]
    kinds = [(c[0], c[1]) for c in dec.calls]
    assert kinds == [("begin", 2), ("reset", [1]), ("prime", [0]), ("push", [0, 1]), ("push", [0, 1]),
                     ("prime", [0]), ("push", [0]), ("push", [0])], kinds
    assert [[a.shape[0] // UP for a in p] for p, _ in out] == [[2, 2, 0], [1, 2, 0], [0, 0, 2], [0, 0, 1]]
