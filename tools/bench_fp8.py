#!/usr/bin/env python3
"""FP8 (e4m3) weights against bf16 for the talker's decode GEMMs: the metric config's call (1.7B dims, 125 frames, default sampling,
captured frame graph) on ONE bf16 and ONE fp8 engine in ONE process, the timed calls interleaved (process-to-process variance on shared
machines is about 5 %: only numbers of one process compare).

    python tools/bench_fp8.py --batch 8
    python tools/bench_fp8.py --batch 32
    python tools/bench_fp8.py --batch 32 --ks-fp8 0      # A/B: the fp8 engine's split-K shapes on the unsplit fp8 kernel

Prints one JSON line per batch: frame-step ms of both engines (min of `--reps` timed generations each, the min of three prefill-only calls
subtracted; every run, the median and the max - min spread listed), `packed_weight_bytes` of both, and the per-class decode-GEMM profile of both (`set_profile(1)`: every launch of frames
1..6 of a real generation timed on its own, eager) for the talker stack's classes.  `ks_split_per_step` (of the timed graph) and
`ks_split_per_step_profile` (of the profiled call) say how many launches per frame step ran on the split-K kernel -- skinny2_ks_kernel in the
bf16 engine, skinny2_ks_fp8_kernel in the fp8 engine: the classes with K >= the floor and N = hidden (`split_k` in their rows).
`--ks-fp8` / `--ks-mink` set the engine-level switches QTTS_SKINNY_KS_FP8 / QTTS_SKINNY_KS_MINK for both engines of the process."""
import argparse
import gc
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
from qwen3_tts_amd import _lib  # noqa: E402
from qwen3_tts_amd.talker import TalkerEngine  # noqa: E402


def weights(t):
    """Cheap weights (timing does not care; logits must not be tied).  Rows differ in scale so that the row exponents do."""
    base = np.random.default_rng(0).standard_normal(1 << 20, dtype=np.float32)
    w = {}
    for k, shp in synth.talker_param_shapes(t, with_text=False).items():
        v = np.resize(base, int(np.prod(shp))).reshape(shp) * np.float32(0.02)
        if "norm" in k and k.endswith("weight"):
            v = v * 0 + 1
        if "head" in k:
            v = np.random.default_rng(zlib.crc32(k.encode())).standard_normal(shp, dtype=np.float32) * np.float32(0.08)
        w[k] = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32))
    return w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--frames", type=int, default=125)
    ap.add_argument("--layers", type=int, default=28)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--ks-fp8", type=int, choices=[0, 1], default=None, help="QTTS_SKINNY_KS_FP8: 0 keeps fp8 operators off the split-K kernel")
    ap.add_argument("--ks-mink", type=int, default=None, help="QTTS_SKINNY_KS_MINK: the smallest K that splits (default 6144)")
    a = ap.parse_args()
    switches = {k: v for k, v in (("QTTS_SKINNY_KS_FP8", a.ks_fp8), ("QTTS_SKINNY_KS_MINK", a.ks_mink)) if v is not None}
    for k, v in switches.items():                                  # for the whole process: engines copy them at creation, the launcher reads the floor at capture
        _lib.set_option(k, v)
    mink = a.ks_mink if a.ks_mink is not None else int(os.environ.get("QTTS_SKINNY_KS_MINK", 6144))
    t = synth.talker_17b() if a.layers == 28 else __import__("dataclasses").replace(synth.talker_17b(), num_hidden_layers=a.layers)
    w = weights(t)
    F = a.frames
    sup = [i for i in range(t.vocab_size - 1024, t.vocab_size) if i != t.codec_eos_token_id]
    kw = dict(max_new_tokens=F + 1, min_new_tokens=F + 1, suppress_tokens=sup, repetition_penalty=1.05, output_hidden_states=False,
              do_sample=True, top_k=50, top_p=1.0, temperature=0.9, subtalker_dosample=True, subtalker_top_k=50, subtalker_top_p=1.0,
              subtalker_temperature=0.9)
    for B in a.batch:
        lens = [24 + 4 * (i % 8) + 12 for i in range(B)]
        prompt = synth.rand_prompt(np.random.default_rng(1), t, lens, 1)
        engs = {}
        for name, fmt in (("bf16", None), ("fp8", "fp8")):
            t0 = time.perf_counter()
            engs[name] = TalkerEngine(t, w, weight_dtype=torch.bfloat16, max_batch=B, max_seq=max(lens) + F + 8, use_graph=True, weight_format=fmt)
            print(f"[bench_fp8] batch {B}: {name} engine built in {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)

        def run(e, seed, **over):
            n = e.generate(*prompt, seed=seed, **dict(kw, **over)).n_frames
            torch.cuda.synchronize()
            return n

        for e in engs.values():
            assert run(e, 0) == F                                  # warm-up: captures the graph
        ts = {k: [] for k in engs}
        for r in range(a.reps):                                    # interleaved: bf16, fp8, bf16, fp8, ...
            for k, e in engs.items():
                t1 = time.perf_counter()
                run(e, 1 + r)
                ts[k].append(time.perf_counter() - t1)
        tp = {k: [] for k in engs}
        for r in range(3):                                         # the prefill-only call that is subtracted: min of three, interleaved too
            for k, e in engs.items():
                t1 = time.perf_counter()
                run(e, 0, max_new_tokens=1, min_new_tokens=1)
                tp[k].append(time.perf_counter() - t1)
        tp = {k: min(v) for k, v in tp.items()}
        res = {"batch": B, "frames": F, "layers": a.layers, "switches": switches}
        for k, e in engs.items():
            res[k] = {"ms_per_frame": round(1000 * (min(ts[k]) - tp[k]) / F, 4), "ms_per_frame_runs": [round(1000 * (x - tp[k]) / F, 4) for x in ts[k]],
                      "ms_per_frame_median": round(1000 * (sorted(ts[k])[len(ts[k]) // 2] - tp[k]) / F, 4),
                      "ms_per_frame_spread": round(1000 * (max(ts[k]) - min(ts[k])) / F, 4), "prefill_ms": round(1000 * tp[k], 3),
                      "packed_weight_bytes": e.packed_weight_bytes, "weight_bytes_per_frame": e.stats()["weight_bytes_per_frame"],
                      "ks_split_per_step": e.stats()["ks_split_per_step"]}
        for k, e in engs.items():                                  # the per-launch profile: eager, frames 1..6 of a short call
            e.set_profile(1)
            run(e, 9, max_new_tokens=9, min_new_tokens=9)
            split = res[k]["ks_split_per_step_profile"] = e.stats()["ks_split_per_step"]
            res[k]["gemm_classes_talker"] = [
                {"N": c["N"], "K": c["K"], "launches": c["launches"], "avg_us": round(1000 * c["total_ms"] / max(1, c["launches"]), 3),
                 "min_us": round(c["min_us"], 3), "MB": round(c["bytes_per_launch"] / 1e6, 3),
                 "GBps": round(c["bytes_per_launch"] / (1e3 * c["total_ms"] / max(1, c["launches"])) / 1e3, 1),
                 "split_k": bool(split > 0 and c["N"] == t.hidden_size and c["K"] >= mink and not (k == "fp8" and a.ks_fp8 == 0))}
                for c in e.gemm_profile() if c["stack"] == 0]
            e.set_profile(0)
        res["fp8_over_bf16"] = round(res["fp8"]["ms_per_frame"] / res["bf16"]["ms_per_frame"], 4)
        print(json.dumps(res), flush=True)
        del engs, e, run                                           # (every reference: a live engine of this batch would keep its place in the device's
        gc.collect()                                               # account of fused code-predictor launches, and the next batch's second engine would run unfused)


if __name__ == "__main__":
    main()
