#!/usr/bin/env python3
"""The continuous schedule on a shared KV page pool against the static cache: 1.7B dims, bf16, captured frame graph, `max_seq` 4096,
sampling with EOS blocked and a per-request `max_new_tokens` (the length spread of tools/bench_refill.py), 4 x `max_batch` requests.

    python tools/bench_kv_pool.py                      # max_batch 32 and 64
    python tools/bench_kv_pool.py --batch 32 --rounds 3 --scale 0.5

Three engines per batch size, all in ONE process, their rounds interleaved (process-to-process variance on shared machines is about 5 %):
  (a) `static`   the static engine (max_batch x max_seq keys reserved): the yardstick;
  (b) `pool`     a pool of the static size (max_batch x max_seq / 16 pages): the same schedule, every K / V request through the page
                 table -- isolates what the table costs;
  (c) `quarter`  a pool of a quarter of that: what the memory saving costs in admissions held back and preemptions.
`--pages N` replaces (c)'s size.  Engines that do not fit the device together are built and measured one after the other with
`--sequential` (then (a) and (b) are NOT interleaved and the comparison carries the process's drift).

One JSON line per batch size: per engine the wall seconds of every round, tokens/s (useful row-frames per second), ms per frame step,
the row occupancy, `peak_pages`, `preemptions` and the bytes the talker cache reserves; `static_spread` is (a)'s max / min over its own
rounds -- a difference between (a) and (b) below it is not resolved by this run."""
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
from bench_refill import LENGTHS  # noqa: E402
from bench_row_sampling import weights  # noqa: E402
from qwen3_tts_amd.talker import TalkerEngine  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="*", default=[32, 64])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--packet", type=int, default=8)
    ap.add_argument("--layers", type=int, default=28)
    ap.add_argument("--max-seq", type=int, default=4096)
    ap.add_argument("--pages", type=int, default=0)
    ap.add_argument("--sequential", action="store_true")
    a = ap.parse_args()
    t = synth.talker_17b() if a.layers == 28 else __import__("dataclasses").replace(synth.talker_17b(), num_hidden_layers=a.layers)
    w = weights(t)
    sup = [i for i in range(t.vocab_size - 1024, t.vocab_size) if i != t.codec_eos_token_id]
    for B in a.batch:
        N = 4 * B
        limits = [max(3, int(a.scale * LENGTHS[i % 16])) for i in range(N)]
        lens = [24 + 4 * (i % 8) + 12 for i in range(N)]
        args = synth.rand_prompt(np.random.default_rng(1), t, lens, 1)
        kw = dict(suppress_tokens=sup, repetition_penalty=1.05, output_hidden_states=False, do_sample=True, top_k=50, top_p=1.0,
                  temperature=0.9, min_new_tokens=max(limits) + 1, seed=[1000 + i for i in range(N)], max_new_tokens=limits,
                  packet_frames=a.packet, schedule="continuous")
        useful = sum(m - 1 for m in limits)
        static_pages = B * (-(-a.max_seq // 16))
        sizes = {"static": None, "pool": static_pages, "quarter": a.pages or max(-(-a.max_seq // 16), static_pages // 4)}
        build = lambda pages: TalkerEngine(t, w, weight_dtype=torch.bfloat16, max_batch=B, max_seq=a.max_seq, use_graph=True, kv_pages=pages)
        res, sched = {n: [] for n in sizes}, {}

        def run(eng, name):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.generate(*args, **kw)
            torch.cuda.synchronize()
            res[name].append(round(time.perf_counter() - t0, 4))
            sched[name] = dict(eng.last_refill)

        if a.sequential:
            for name, pages in sizes.items():
                eng = build(pages)
                eng.generate(*args, **kw)            # warm-up: captures, allocator
                for _ in range(a.rounds):
                    run(eng, name)
                page_bytes = eng.kv_page_bytes
                del eng
                torch.cuda.empty_cache()
        else:
            engines = {name: build(pages) for name, pages in sizes.items()}
            for eng in engines.values():
                eng.generate(*args, **kw)
            for _ in range(a.rounds):
                for name, eng in engines.items():
                    run(eng, name)
            page_bytes = engines["static"].kv_page_bytes
        line = {"bench": "kv_pool", "max_batch": B, "requests": N, "layers": a.layers, "max_seq": a.max_seq, "useful_row_frames": useful,
                "packet_frames": a.packet, "interleaved": not a.sequential, "kv_page_bytes": page_bytes}
        for name, pages in sizes.items():
            s, best = sched[name], min(res[name])
            line[name] = {"seconds": res[name], "min_seconds": best, "tokens_per_s": round(useful / best, 1), "frame_steps": s["frames_run"],
                          "ms_per_frame": round(1e3 * best / s["frames_run"], 4), "occupancy": round(s["occupancy"], 3),
                          "pool_pages": s["pool_pages"], "peak_pages": s["peak_pages"], "preemptions": s["preemptions"],
                          "kv_bytes_reserved": ((pages + 1) if pages else static_pages) * page_bytes}
        line["static_spread"] = round(max(res["static"]) / min(res["static"]), 4)
        line["pool_over_static_ms_per_frame"] = round(line["pool"]["ms_per_frame"] / line["static"]["ms_per_frame"], 4)
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
