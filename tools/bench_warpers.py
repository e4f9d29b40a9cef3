#!/usr/bin/env python3
"""What the talker's remaining HF sampling controls cost per frame: 1.7B dims, batch 8, 125 frames, bf16, captured frame graph, three
per-row tables INTERLEAVED in one process (the manner of tools/ab_inproc.py):

  (a) `fast`    a row table inside the fast class (top_k 50: sample_kernel_v2);
  (b) `general` the same table with top_k = 300 (the general class: sample_kernel);
  (c) `warp`    table (a) plus min_p = 0.05, typical_p = 0.95 and no_repeat_ngram_size = 4 on every row (sample_warp_kernel).

    python tools/bench_warpers.py                         # one JSON line
    python tools/bench_warpers.py --frames 60 --rounds 5

Reports ms per frame of each case (the prefill-only call subtracted; min and all runs), the spread of (a) against itself, the sampler
classes each case ran, and (c) - (b), (c) - (a).  Runs on this tree's library only: (b) and (a) of another commit are that commit's
run of its own tools/bench_row_sampling.py / this file.  The talker sampler's per-launch time comes from a `rocprofv3 --kernel-trace
--stats` run of this tool (tools/rocpd_stats.py) or from the `tstamp` variant (tools/ts_frame.py): the kernel stamps the phases
1..5 = logits arrived | processors | cuts | drawn | rows gathered."""
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

CASES = {"fast": dict(top_k=50), "general": dict(top_k=300),
         "warp": dict(top_k=50, min_p=0.05, typical_p=0.95, no_repeat_ngram_size=4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--frames", type=int, default=125)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--layers", type=int, default=28)
    a = ap.parse_args()
    t = synth.talker_17b() if a.layers == 28 else __import__("dataclasses").replace(synth.talker_17b(), num_hidden_layers=a.layers)
    w = weights(t)
    sup = [i for i in range(t.vocab_size - 1024, t.vocab_size) if i != t.codec_eos_token_id]
    B, F = a.batch, a.frames
    lens = [24 + 4 * (i % 8) + 12 for i in range(B)]
    emb, mask, tr, pad = synth.rand_prompt(np.random.default_rng(1), t, lens, 1)
    eng = TalkerEngine(t, w, weight_dtype=torch.bfloat16, max_batch=B, max_seq=max(lens) + F + 8, use_graph=True)
    base = dict(suppress_tokens=sup, repetition_penalty=1.05, output_hidden_states=False, do_sample=True, top_p=1.0, temperature=[0.9] * B,
                subtalker_dosample=True, subtalker_top_k=50, subtalker_top_p=1.0, subtalker_temperature=0.9)
    classes = {}

    def run(case, frames, seed):
        kw = dict(base, max_new_tokens=frames + 1, min_new_tokens=frames + 1, seed=seed, **CASES[case])
        t1 = time.perf_counter()
        n = eng.generate(emb, mask, tr, pad, **kw).n_frames
        torch.cuda.synchronize()
        classes[case] = eng.sampler_class()
        return time.perf_counter() - t1, n

    names = list(CASES)
    for c in names:
        assert run(c, F, 0)[1] == F                                # warm-up: capture
    ts = {c: [] for c in names}
    for r in range(a.rounds):
        for c in (names if r % 2 == 0 else names[::-1]):
            ts[c].append(run(c, F, 1 + r)[0])
    tp = {c: min(run(c, 0, 0)[0] for _ in range(2)) for c in names}
    ms = {c: [round(1000 * (x - tp[c]) / F, 4) for x in v] for c, v in ts.items()}
    best = {c: min(v) for c, v in ms.items()}
    print(json.dumps({"what": "warpers", "batch": B, "frames": F, "layers": a.layers, "ms_per_frame": best, "runs": ms,
                      "fast_spread_ms": round(max(ms["fast"]) - min(ms["fast"]), 4), "sampler_class": classes,
                      "warp_minus_general_us": round(1000 * (best["warp"] - best["general"]), 2),
                      "warp_minus_fast_us": round(1000 * (best["warp"] - best["fast"]), 2),
                      "graph_nodes": eng.stats()["graph_nodes"]}), flush=True)


if __name__ == "__main__":
    main()
