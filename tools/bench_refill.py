#!/usr/bin/env python3
"""Static waves against the refill and the continuous schedule on a ragged request list: 1.7B dims, bf16, captured frame graph, sampling
with EOS blocked and a per-request `max_new_tokens`, 4 x `max_batch` requests, all schedules in ONE process on one engine per batch size.

    python tools/bench_refill.py                      # max_batch 8 and 32
    python tools/bench_refill.py --batch 8 --rounds 2 --scale 0.5

The length list is fixed (no random source): request i asks for `scale` x LENGTHS[i % 16] tokens, lengths an order of magnitude apart as
utterances are.  `waves` is `TalkerEngine.generate` on slices of `max_batch` requests in the order given (what
`Qwen3TTSForConditionalGeneration.generate` does), `refill` is `generate(schedule="refill")` on the whole list (one shared position per
stream), `continuous` is `generate(schedule="continuous")` (per-row positions: one stream, every row attends over its own occupant's
keys).  One JSON line per batch size: wall seconds of every round and the minimum per schedule, frame steps run, milliseconds per frame
step (prefills and admissions included) and the row occupancy each schedule achieved (useful row-frames / (frame steps x max_batch)).
Process-to-process variance on shared machines is a few per cent; the schedules of one line ran interleaved in the same process."""
import argparse
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
from bench_row_sampling import weights  # noqa: E402
from qwen3_tts_amd.talker import TalkerEngine  # noqa: E402

LENGTHS = [24, 220, 60, 36, 140, 30, 90, 260, 44, 28, 180, 70, 32, 110, 50, 300]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="*", default=[8, 32])
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--packet", type=int, default=8)
    ap.add_argument("--layers", type=int, default=28)
    a = ap.parse_args()
    t = synth.talker_17b() if a.layers == 28 else __import__("dataclasses").replace(synth.talker_17b(), num_hidden_layers=a.layers)
    w = weights(t)
    sup = [i for i in range(t.vocab_size - 1024, t.vocab_size) if i != t.codec_eos_token_id]
    for B in a.batch:
        N = 4 * B
        limits = [max(3, int(a.scale * LENGTHS[i % 16])) for i in range(N)]
        lens = [24 + 4 * (i % 8) + 12 for i in range(N)]
        args = synth.rand_prompt(np.random.default_rng(1), t, lens, 1)
        # positions: a refill stream carries its rows' requests one after the other on one shared position
        max_seq = max(lens) + sum(sorted(limits)[-(N // B + 1):]) + 64
        eng = TalkerEngine(t, w, weight_dtype=torch.bfloat16, max_batch=B, max_seq=max_seq, use_graph=True)
        kw = dict(suppress_tokens=sup, repetition_penalty=1.05, output_hidden_states=False, do_sample=True, top_k=50, top_p=1.0,
                  temperature=0.9, min_new_tokens=max(limits) + 1, seed=[1000 + i for i in range(N)])
        useful = sum(m - 1 for m in limits)

        def waves():
            steps = 0
            for b0 in range(0, N, B):
                sl = slice(b0, b0 + B)
                out = eng.generate(*[x[sl] for x in args[:3]], args[3], max_new_tokens=limits[sl], **dict(kw, seed=kw["seed"][sl]))
                steps += out.n_frames
            return steps

        def refill():
            eng.generate(*args, schedule="refill", max_new_tokens=limits, packet_frames=a.packet, **kw)
            return eng.last_refill["frames_run"]

        def continuous():
            eng.generate(*args, schedule="continuous", max_new_tokens=limits, packet_frames=a.packet, **kw)
            return eng.last_refill["frames_run"]

        names = ("waves", "refill", "continuous")
        fns = dict(waves=waves, refill=refill, continuous=continuous)
        res = {n: [] for n in names}
        steps, sched = {}, {}
        for n in names:                     # warm-up: captures, allocator
            fns[n]()
        for _ in range(a.rounds):
            for name, fn in fns.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                steps[name] = fn()
                torch.cuda.synchronize()
                res[name].append(round(time.perf_counter() - t0, 4))
                if name != "waves":
                    sched[name] = dict(eng.last_refill)
        line = {"bench": "refill", "max_batch": B, "requests": N, "layers": a.layers, "useful_row_frames": useful, "max_seq": max_seq,
                "packet_frames": a.packet}
        for name in names:
            line[name] = {"seconds": res[name], "min_seconds": min(res[name]), "frame_steps": steps[name],
                          "ms_per_frame": round(1e3 * min(res[name]) / steps[name], 4), "occupancy": round(useful / (steps[name] * B), 3)}
        for name in ("refill", "continuous"):
            line[name].update({k: sched[name][k] for k in ("streams", "admit_calls", "admitted_rows", "max_row_len", "graph_captures")})
        line["speedup"] = round(line["waves"]["min_seconds"] / line["refill"]["min_seconds"], 3)
        line["speedup_continuous"] = round(line["waves"]["min_seconds"] / line["continuous"]["min_seconds"], 3)
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
