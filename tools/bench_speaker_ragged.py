#!/usr/bin/env python3
"""What the ragged speaker-encoder batch buys: released dims, fp32 and bf16 engines, 8 and 32 seeded clips of 3-10 s (all lengths
different, as real reference clips are), one `SpeakerEncoderEngine.embed_many` per measurement:

  `ragged`  this tree: the clips ordered by length, groups of `max_batch`, one `qtts_speaker_embed_ragged` launch sequence per group;
  `parent`  the parent commit's `embed_many` -- its loop restated below (bucket by exact length, `embed` per bucket): with no two clips
            alike that is one full launch sequence per clip.  `embed` itself is untouched by this tree, so the restated loop makes the
            C calls the parent made.

    python tools/bench_speaker_ragged.py                     # one JSON line
    python tools/bench_speaker_ragged.py --repeats 3 --iters 5

Per case: three repeats (each the mean of `iters` calls after a warm-up, the two arms interleaved in one process), their min / max, the
speed-up of the minima, the largest difference between the two arms' x-vectors, and the C calls each arm made."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import synth  # noqa: E402
from qwen3_tts_amd.speaker import SpeakerEncoderEngine  # noqa: E402


def clips(n, seed=17):
    g = np.random.default_rng(seed)
    lens = sorted({int(x) for x in g.integers(3 * 24000, 10 * 24000, 4 * n)})
    lens = [lens[i] for i in g.permutation(len(lens))[:n]]
    return [synth.rand_audio(seed + 1 + i, 1, k)[0] for i, k in enumerate(lens)]


def parent_embed_many(eng, audios):
    """`SpeakerEncoderEngine.embed_many` as it was before the ragged entry point: clips bucketed by exact length"""
    arrs = [np.asarray(a, dtype=np.float32).reshape(-1) for a in audios]
    groups = {}
    for i, a in enumerate(arrs):
        groups.setdefault(a.shape[0], []).append(i)
    out = [None] * len(arrs)
    for idx in groups.values():
        for k in range(0, len(idx), eng.max_batch):
            part = idx[k:k + eng.max_batch]
            emb = eng.embed(torch.from_numpy(np.stack([arrs[i] for i in part])))
            for r, i in enumerate(part):
                out[i] = emb[r]
    return out


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--batches", default="8,32")
    ap.add_argument("--dtypes", default="fp32,bf16")
    a = ap.parse_args()
    c = synth.speaker_real()
    w = {k: torch.from_numpy(v) for k, v in synth.speaker_weights(c).items()}
    runs = []
    for dt in a.dtypes.split(","):
        for n in (int(x) for x in a.batches.split(",")):
            cl = clips(n)
            eng = SpeakerEncoderEngine(synth.cfg_dict(c), w, compute_dtype=torch.float32 if dt == "fp32" else torch.bfloat16,
                                       max_batch=n, max_samples=10 * 24000)
            arms = {"ragged": lambda: eng.embed_many(cl), "parent": lambda: parent_embed_many(eng, cl)}
            calls, outs = {}, {}
            for name, fn in arms.items():                                      # warm-up, and what each arm computes
                n0 = eng.embed_calls
                outs[name] = torch.stack(fn()).cpu().numpy()
                calls[name] = eng.embed_calls - n0
            ms = {name: [] for name in arms}
            for _ in range(a.repeats):
                for name, fn in arms.items():
                    ms[name].append(timed(fn, a.iters))
            r = dict(dtype=dt, clips=n, seconds_of_audio=round(sum(x.shape[0] for x in cl) / 24000, 1), calls=calls,
                     max_diff=float(np.abs(outs["ragged"] - outs["parent"]).max()), largest_component=float(np.abs(outs["parent"]).max()))
            for name in arms:
                r[name + "_ms"] = [round(x, 3) for x in ms[name]]
            r["speedup_of_minima"] = round(min(ms["parent"]) / min(ms["ragged"]), 2)
            r["beats_parent_beyond_spread"] = max(ms["ragged"]) < min(ms["parent"])
            runs.append(r)
            del eng
    print(json.dumps(dict(tool="bench_speaker_ragged", device=torch.cuda.get_device_name(0), repeats=a.repeats, iters=a.iters, runs=runs)))


if __name__ == "__main__":
    main()
