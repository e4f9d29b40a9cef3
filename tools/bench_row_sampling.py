#!/usr/bin/env python3
"""What per-request sampling settings cost and save: 1.7B dims, bf16, captured frame graph, sampling, fixed frames, one engine per batch
size, scalar mode (`qtts_talker_generate`) against table mode (`qtts_talker_generate_rows`) INTERLEAVED in one process.

    python tools/bench_row_sampling.py                      # batch 8 and 32
    python tools/bench_row_sampling.py --batch 8 --frames 60 --rounds 5

Two comparisons per batch size, one JSON line each:
  * `frame_step`: ms per frame of a generation with the reference's defaults, scalar against a table whose entries all hold the same
    values (the table's cost: one 64-byte entry read per sampler launch).  `rounds` alternating pairs, the prefill-only call subtracted;
    min and all runs are printed.
  * `knob_change`: wall time per call when the temperature changes on EVERY call -- scalar mode destroys and re-captures the frame graph
    each time, table mode replays it (`graph_captures` of both legs are printed).
Process-to-process variance on shared machines is a few per cent; the two modes of one line ran interleaved in the same process."""
import argparse
import json
import os
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import synth  # noqa: E402
from qwen3_tts_amd.talker import TalkerEngine  # noqa: E402


def weights(t):
    base = np.random.default_rng(0).standard_normal(1 << 20, dtype=np.float32)
    w = {}
    for k, shp in synth.talker_param_shapes(t, with_text=False).items():      # cheap weights: timing does not care, logits must not be tied
        v = np.resize(base, int(np.prod(shp))).reshape(shp) * np.float32(0.02)
        if "norm" in k and k.endswith("weight"):
            v = v * 0 + 1
        if "head" in k:
            v = np.random.default_rng(zlib.crc32(k.encode())).standard_normal(shp, dtype=np.float32) * np.float32(0.08)
        w[k] = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32))
    return w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="*", default=[8, 32])
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--change-calls", type=int, default=6)
    ap.add_argument("--change-frames", type=int, default=16)
    ap.add_argument("--layers", type=int, default=28)
    a = ap.parse_args()
    t = synth.talker_17b() if a.layers == 28 else __import__("dataclasses").replace(synth.talker_17b(), num_hidden_layers=a.layers)
    w = weights(t)
    sup = [i for i in range(t.vocab_size - 1024, t.vocab_size) if i != t.codec_eos_token_id]
    for B in a.batch:
        F = a.frames
        lens = [24 + 4 * (i % 8) + 12 for i in range(B)]
        emb, mask, tr, pad = synth.rand_prompt(np.random.default_rng(1), t, lens, 1)
        eng = TalkerEngine(t, w, weight_dtype=torch.bfloat16, max_batch=B, max_seq=max(lens) + F + 8, use_graph=True)
        base = dict(suppress_tokens=sup, repetition_penalty=1.05, output_hidden_states=False, do_sample=True, top_k=50, top_p=1.0,
                    temperature=0.9, subtalker_dosample=True, subtalker_top_k=50, subtalker_top_p=1.0, subtalker_temperature=0.9)

        def run(table, frames, seed, temperature=0.9):
            kw = dict(base, max_new_tokens=frames + 1, min_new_tokens=frames + 1, temperature=temperature)
            kw.update(seed=seed)                 # (table mode: request b samples with seed + b)
            if table:
                kw.update(temperature=[temperature] * B)
            t1 = time.perf_counter()
            n = eng.generate(emb, mask, tr, pad, **kw).n_frames
            torch.cuda.synchronize()
            return time.perf_counter() - t1, n

        # ---- the frame step, scalar against table, alternating
        for table in (False, True):
            assert run(table, F, 0)[1] == F                            # warm-up: capture
        ts = {False: [], True: []}
        for r in range(a.rounds):
            for table in ((False, True) if r % 2 == 0 else (True, False)):
                ts[table].append(run(table, F, 1 + r)[0])
        tp = {table: min(run(table, 0, 0)[0] for _ in range(2)) for table in (False, True)}
        ms = {k: [round(1000 * (x - tp[k]) / F, 4) for x in v] for k, v in ts.items()}
        st = eng.stats()
        print(json.dumps({"what": "frame_step", "batch": B, "frames": F, "layers": a.layers, "scalar_ms_per_frame": min(ms[False]),
                          "table_ms_per_frame": min(ms[True]), "table_over_scalar": round(min(ms[True]) / min(ms[False]), 4),
                          "scalar_runs": ms[False], "table_runs": ms[True], "graph_nodes": st["graph_nodes"]}), flush=True)
        # ---- a knob that changes on every call
        Fc = a.change_frames
        res = {}
        for table in (False, True):
            run(table, Fc, 0, 0.9)
            c0 = eng.stats()["graph_captures"]
            t1 = time.perf_counter()
            for i in range(a.change_calls):
                run(table, Fc, 10 + i, 0.6 + 0.05 * i)
            res[table] = (1000 * (time.perf_counter() - t1) / a.change_calls, eng.stats()["graph_captures"] - c0)
        print(json.dumps({"what": "knob_change", "batch": B, "frames_per_call": Fc, "calls": a.change_calls, "layers": a.layers,
                          "scalar_ms_per_call": round(res[False][0], 2), "scalar_captures": res[False][1],
                          "table_ms_per_call": round(res[True][0], 2), "table_captures": res[True][1],
                          "saved_ms_per_call": round(res[False][0] - res[True][0], 2)}), flush=True)
        del eng
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
