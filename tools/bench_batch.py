#!/usr/bin/env python3
"""Throughput of the talker's frame step by batch: 1.7B dims, bf16, captured frame graph, sampling, 125 fixed frames, `--batch` requests
run as `--waves` equal waves (one engine, created for the wave's rows; the waves one after the other, as model.py runs a request list
longer than max_batch).

    python tools/bench_batch.py --batch 64                  # one wave of 64
    python tools/bench_batch.py --batch 64 --waves 2        # the same 64 requests as two waves of 32

Prints one JSON line: ms per frame of the whole request list (min of 3 timed generations, the prefill-only calls subtracted; all three
in `ms_per_frame_runs`), speech tokens per second (requests x code groups x frames / decode time), graph_nodes and the fused / split
launches per step.  Options of the library (QTTS_*) come from the environment as usual.  Process-to-process variance on shared machines
is a few per cent: compare runs of one session."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--waves", type=int, default=1)
    ap.add_argument("--frames", type=int, default=125)
    ap.add_argument("--layers", type=int, default=28)
    ap.add_argument("--tag", default=None)
    a = ap.parse_args()
    if a.batch % a.waves:
        ap.error("--batch must be a multiple of --waves")
    t = synth.talker_17b() if a.layers == 28 else __import__("dataclasses").replace(synth.talker_17b(), num_hidden_layers=a.layers)
    base = np.random.default_rng(0).standard_normal(1 << 20, dtype=np.float32)
    w = {}
    for k, shp in synth.talker_param_shapes(t, with_text=False).items():      # cheap weights: timing does not care, logits must not be tied
        v = np.resize(base, int(np.prod(shp))).reshape(shp) * np.float32(0.02)
        if "norm" in k and k.endswith("weight"):
            v = v * 0 + 1
        if "head" in k:
            v = np.random.default_rng(zlib.crc32(k.encode())).standard_normal(shp, dtype=np.float32) * np.float32(0.08)
        w[k] = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32))
    B, F, W = a.batch, a.frames, a.batch // a.waves
    lens = [24 + 4 * (i % 8) + 12 for i in range(B)]
    emb, mask, tr, pad = synth.rand_prompt(np.random.default_rng(1), t, lens, 1)
    sup = [i for i in range(t.vocab_size - 1024, t.vocab_size) if i != t.codec_eos_token_id]
    kw = dict(max_new_tokens=F + 1, min_new_tokens=F + 1, suppress_tokens=sup, repetition_penalty=1.05, output_hidden_states=False,
              do_sample=True, top_k=50, top_p=1.0, temperature=0.9, subtalker_dosample=True, subtalker_top_k=50, subtalker_top_p=1.0,
              subtalker_temperature=0.9)
    eng = TalkerEngine(t, w, weight_dtype=torch.bfloat16, max_batch=W, max_seq=max(lens) + F + 8, use_graph=True)

    def run(seed, **over):
        n = 0
        for b0 in range(0, B, W):
            s = slice(b0, b0 + W)
            n = eng.generate(emb[s], mask[s], tr[s], pad, seed=seed, **dict(kw, **over)).n_frames
        torch.cuda.synchronize()
        return n

    assert run(0) == F
    ts = []
    for r in range(3):
        t1 = time.perf_counter()
        run(1 + r)
        ts.append(time.perf_counter() - t1)
    t1 = time.perf_counter()
    run(0, max_new_tokens=1, min_new_tokens=1)
    tp = time.perf_counter() - t1
    st = eng.stats()
    G = t.num_code_groups
    print(json.dumps({"tag": a.tag, "batch": B, "waves": a.waves, "rows_per_wave": W, "frames": F, "layers": a.layers,
                      "ms_per_frame": round(1000 * (min(ts) - tp) / F, 4), "ms_per_frame_runs": [round(1000 * (x - tp) / F, 4) for x in ts],
                      "tokens_per_s": round(B * G * F / (min(ts) - tp), 1), "tokens_per_s_runs": [round(B * G * F / (x - tp), 1) for x in ts],
                      "prefill_ms": round(1000 * tp, 2), "graph_nodes": st["graph_nodes"], "cp_fused_per_step": st["cp_fused_per_step"],
                      "cp_mlp_per_step": st.get("cp_mlp_per_step"), "ks_split_per_step": st.get("ks_split_per_step")}), flush=True)


if __name__ == "__main__":
    main()
