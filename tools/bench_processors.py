#!/usr/bin/env python3
"""What the talker's remaining HF logits processors cost per frame: 1.7B dims, batch 8, 125 frames, bf16, captured frame graph, per-row
tables INTERLEAVED in one process (the manner of tools/bench_warpers.py, whose `warp` case is case (a) here, knob for knob):

  (a) `warp`    sample_warp_kernel with every processor off: top_k 50, min_p = 0.05, typical_p = 0.95, no_repeat_ngram_size = 4;
  (b) `few`     (a) plus, on every row, one bad word, one bias of length 3, a begin suppression and a decay;
  (c) `proc64`  (a) plus a 64-sequence table on every row: 32 biases and 32 bad words of 8 tokens each (512 tokens, the capacity).

    python tools/bench_processors.py                         # one JSON line
    python tools/bench_processors.py --frames 60 --rounds 5

Reports ms per frame of each case (the prefill-only call subtracted; min and all runs), the spread of (a) against itself, the sampler
classes each case ran, and (b) - (a), (c) - (a).  Runs on this tree's library only: (a) of another commit is that commit's run of its
own tools/bench_warpers.py.  The sampler's per-launch time comes from a `rocprofv3 --kernel-trace --stats` run of this tool
(tools/rocpd_stats.py)."""
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

WARP = dict(top_k=50, min_p=0.05, typical_p=0.95, no_repeat_ngram_size=4)


def cases(t):
    g = np.random.default_rng(3)
    live = t.vocab_size - 1024
    seq = lambda n: [int(x) for x in g.integers(1, live, n)]
    few = dict(bad_words_ids=[seq(1)], sequence_bias={tuple(seq(3)): -5.0}, begin_suppress_tokens=seq(4),
               exponential_decay_length_penalty=(100, 1.01))
    many = dict(sequence_bias={tuple(seq(8)): -2.0 for _ in range(32)}, bad_words_ids=[seq(8) for _ in range(32)])
    return {"warp": dict(WARP), "few": dict(WARP, **few), "proc64": dict(WARP, **many)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--frames", type=int, default=125)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--layers", type=int, default=28)
    ap.add_argument("--cases", default="warp,few,proc64", help="comma-separated subset (one case alone: for a kernel trace of that case)")
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
    CASES = {k: v for k, v in cases(t).items() if k in a.cases.split(",")}
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
    out = {"what": "processors", "batch": B, "frames": F, "layers": a.layers, "ms_per_frame": best, "runs": ms, "sampler_class": classes,
           "graph_nodes": eng.stats()["graph_nodes"]}
    if "warp" in best:
        out["warp_spread_ms"] = round(max(ms["warp"]) - min(ms["warp"]), 4)
        out.update({f"{c}_minus_warp_us": round(1000 * (best[c] - best["warp"]), 2) for c in best if c != "warp"})
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
