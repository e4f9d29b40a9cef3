#!/usr/bin/env python3
"""Audio streamed per request from the refill schedule: 1.7B talker dims and the released codec dims, bf16, captured frame graph,
sampling with EOS blocked, a ragged request list of 3 x `max_batch` requests on `max_batch` rows.

    python tools/bench_stream_refill.py                       # max_batch 8, packets of 4 frames
    python tools/bench_stream_refill.py --batch 4 --scale 0.25 --layers 4

Two legs, one JSON line each:

  * "stream_refill": `TalkerEngine.generate_stream(schedule="refill")` with every packet decoded by the codec's per-slot stream
    (`CodecDecoderEngine.stream_reset_rows / stream_push_rows`), as `Qwen3TTSModel.stream_custom_voice(schedule="refill")` does.  Per
    request the time from the start of the call to its first PCM on the host (requests admitted later wait for a row: their time to
    first audio is queueing + one packet), and the row occupancy the schedule achieved.
  * "codec_leg": the codec's share per packet for the first `max_batch` requests in lockstep -- `stream_push_rows` (only the new frames
    of the packet are decoded) against `CodecStreamDecoder` (which re-decodes up to 25 context frames through `forward` for every
    packet): the cost the slot path removes from the first-packet configuration.  Steady state: packets behind the 25-frame context.

The length list is fixed (no random source), as in tools/bench_refill.py.  Times are host wall clock around synchronised calls."""
import argparse
import dataclasses
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import synth  # noqa: E402
from bench_refill import LENGTHS  # noqa: E402
from bench_row_sampling import weights  # noqa: E402
from qwen3_tts_amd.codec import CodecDecoderEngine  # noqa: E402
from qwen3_tts_amd.talker import TalkerEngine  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--scale", type=float, default=0.5)
    ap.add_argument("--packet", type=int, default=4)
    ap.add_argument("--layers", type=int, default=28)
    ap.add_argument("--codec-packets", type=int, default=24, help="packets of the codec leg (the first 7 fill the 25-frame context)")
    a = ap.parse_args()
    dev = "cuda:0"
    t = synth.talker_17b() if a.layers == 28 else dataclasses.replace(synth.talker_17b(), num_hidden_layers=a.layers)
    c = synth.codec_real()
    B, k = a.batch, a.packet
    N = 3 * B
    limits = [max(3, int(a.scale * LENGTHS[i % 16])) for i in range(N)]
    lens = [24 + 4 * (i % 8) + 12 for i in range(N)]
    args = synth.rand_prompt(np.random.default_rng(1), t, lens, 1)
    max_seq = max(lens) + sum(sorted(limits)[-(N // B + 1):]) + 64
    talker = TalkerEngine(t, weights(t), weight_dtype=torch.bfloat16, device=dev, max_batch=B, max_seq=max_seq, use_graph=True)
    codec = CodecDecoderEngine(c, {n: torch.from_numpy(v) for n, v in synth.codec_weights(c).items()}, compute_dtype=torch.bfloat16,
                               device=dev, max_batch=B, max_frames=25 + k)
    sup = [i for i in range(t.vocab_size - 1024, t.vocab_size) if i != t.codec_eos_token_id]
    kw = dict(schedule="refill", packet_frames=k, max_new_tokens=limits, min_new_tokens=max(limits) + 1, suppress_tokens=sup,
              repetition_penalty=1.05, do_sample=True, top_k=50, top_p=1.0, temperature=0.9, seed=[1000 + i for i in range(N)])
    cb, up = c.codebook_size, c.total_upsample

    def run():
        first_audio, samples = [None] * N, [0] * N
        codec.stream_begin(B)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for record in talker.generate_stream(*args, **kw):
            started = [e.row for e in record.rows if e.first]
            if started:
                codec.stream_reset_rows(started)
            live = [e for e in record.rows if e.codes.shape[0] > 0]
            if not live:
                continue
            n = max(int(e.codes.shape[0]) for e in live)
            batch = torch.zeros(len(live), n, t.num_code_groups, dtype=torch.long, device=dev)
            for m, e in enumerate(live):
                batch[m, : e.codes.shape[0]] = e.codes.clamp(min=0, max=cb - 1)
            wav = codec.stream_push_rows([e.row for e in live], batch.transpose(1, 2))[:, 0].cpu()       # PCM on the host
            now = time.perf_counter() - t0
            for m, e in enumerate(live):
                samples[e.request] += int(e.codes.shape[0]) * up
                if first_audio[e.request] is None:
                    first_audio[e.request] = now
            del wav
        return time.perf_counter() - t0, first_audio, samples

    run()                                            # warm-up: graph captures, code objects, allocator
    wall, first_audio, samples = run()
    assert samples == [(m - 1) * up for m in limits], "a request's audio has the wrong length"
    st = talker.last_refill
    fa = np.array(first_audio)
    print(json.dumps({"bench": "stream_refill", "max_batch": B, "requests": N, "layers": a.layers, "packet_frames": k, "wall_s": round(wall, 4),
                      "audio_s": round(sum(samples) / 24000.0, 2), "occupancy": round(st["occupancy"], 4), "streams": st["streams"],
                      "admitted_rows": st["admitted_rows"],
                      "first_audio_ms_per_request": [round(1e3 * x, 2) for x in first_audio],
                      "first_audio_ms_first_rows": [round(1e3 * x, 2) for x in sorted(fa)[:B]],
                      "first_audio_ms_all": {"min": round(1e3 * fa.min(), 2), "median": round(1e3 * float(np.median(fa)), 2),
                                             "max": round(1e3 * fa.max(), 2)}}), flush=True)

    # ---- the codec leg per packet, B rows in lockstep
    P = a.codec_packets
    codes = torch.from_numpy(np.random.default_rng(2).integers(0, cb, (B, c.num_quantizers, P * k))).to(dev)
    ids = list(range(B))

    def leg(push):
        ms = []
        for p in range(P):
            pk = codes[..., p * k:(p + 1) * k].contiguous()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            push(pk)
            torch.cuda.synchronize()
            ms.append(1e3 * (time.perf_counter() - t0))
        return ms

    res = {}
    for name in ("push_rows", "context_redecode", "push_rows", "context_redecode"):          # first pass of each: warm-up
        if name == "push_rows":
            codec.stream_begin(B)
            codec.stream_reset_rows(ids)
            res[name] = leg(lambda pk: codec.stream_push_rows(ids, pk))
        else:
            sd = codec.stream(25)
            res[name] = leg(sd.push)
    steady = slice(-(-25 // k) + 1, None)              # packets whose context is full
    line = {"bench": "stream_refill_codec_leg", "rows": B, "packet_frames": k, "packets": P}
    for name, ms in res.items():
        line[name + "_ms_first_packet"] = round(ms[0], 3)
        line[name + "_ms_steady_median"] = round(float(np.median(ms[steady])), 3)
    line["steady_ratio"] = round(line["context_redecode_ms_steady_median"] / line["push_rows_ms_steady_median"], 3)
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
