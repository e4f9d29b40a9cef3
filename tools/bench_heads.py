#!/usr/bin/env python3
"""Frame time of the talker at a given head shape: the metric config's call (1.7B dims, batch 8, 125 fixed frames, sampling, bf16, captured
frame graph) with the talker's heads / kv heads / head_dim -- and optionally hidden / intermediate size -- taken from the command line.

    python tools/bench_heads.py --heads 16 --kv 2                       # a group of 8
    python tools/bench_heads.py --heads 32 --kv 8 --hidden 2560 --inter 9728      # the 4B backbone's shape

Prints one JSON line: ms per frame (min of 3 timed generations, the prefill-only call subtracted), graph_nodes, and which decode
attention ran (attn_gq_per_step: launches of the general family, csrc/attn_gq.h).  Options of the library (QTTS_*) come from the
environment as usual.  Process-to-process variance on shared machines is a few per cent: compare runs of one session."""
import argparse
import dataclasses
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
    ap.add_argument("--heads", type=int, default=16)
    ap.add_argument("--kv", type=int, default=8)
    ap.add_argument("--head-dim", type=int, default=128)
    ap.add_argument("--hidden", type=int, default=2048)
    ap.add_argument("--inter", type=int, default=6144)
    ap.add_argument("--layers", type=int, default=28)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--frames", type=int, default=125)
    ap.add_argument("--tag", default=None)
    a = ap.parse_args()
    t = dataclasses.replace(synth.talker_17b(), num_attention_heads=a.heads, num_key_value_heads=a.kv, head_dim=a.head_dim,
                            hidden_size=a.hidden, intermediate_size=a.inter, num_hidden_layers=a.layers)
    base = np.random.default_rng(0).standard_normal(1 << 20, dtype=np.float32)
    w = {}
    for k, shp in synth.talker_param_shapes(t, with_text=False).items():      # cheap weights: timing does not care, logits must not be tied
        v = np.resize(base, int(np.prod(shp))).reshape(shp) * np.float32(0.02)
        if "norm" in k and k.endswith("weight"):
            v = v * 0 + 1
        if "head" in k:
            v = np.random.default_rng(zlib.crc32(k.encode())).standard_normal(shp, dtype=np.float32) * np.float32(0.08)
        w[k] = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32))
    B, F = a.batch, a.frames
    lens = [24 + 4 * (i % 8) + 12 for i in range(B)]
    emb, mask, tr, pad = synth.rand_prompt(np.random.default_rng(1), t, lens, 1)
    sup = [i for i in range(t.vocab_size - 1024, t.vocab_size) if i != t.codec_eos_token_id]
    kw = dict(max_new_tokens=F + 1, min_new_tokens=F + 1, suppress_tokens=sup, repetition_penalty=1.05, output_hidden_states=False,
              do_sample=True, top_k=50, top_p=1.0, temperature=0.9, subtalker_dosample=True, subtalker_top_k=50, subtalker_top_p=1.0,
              subtalker_temperature=0.9)
    eng = TalkerEngine(t, w, weight_dtype=torch.bfloat16, max_batch=B, max_seq=max(lens) + F + 8, use_graph=True)
    out = eng.generate(emb, mask, tr, pad, seed=0, **kw)
    torch.cuda.synchronize()
    assert out.n_frames == F
    ts = []
    for r in range(3):
        t1 = time.perf_counter()
        eng.generate(emb, mask, tr, pad, seed=1 + r, **kw)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t1)
    t1 = time.perf_counter()
    eng.generate(emb, mask, tr, pad, seed=0, **dict(kw, max_new_tokens=1, min_new_tokens=1))
    torch.cuda.synchronize()
    tp = time.perf_counter() - t1
    st = eng.stats()
    print(json.dumps({"tag": a.tag, "heads": a.heads, "kv_heads": a.kv, "head_dim": a.head_dim, "hidden": a.hidden, "inter": a.inter,
                      "layers": a.layers, "batch": B, "frames": F, "ms_per_frame": round(1000 * (min(ts) - tp) / F, 4),
                      "ms_per_frame_runs": [round(1000 * (x - tp) / F, 4) for x in ts], "prefill_ms": round(1000 * tp, 2),
                      "graph_nodes": st["graph_nodes"], "attn_gq_per_step": st.get("attn_gq_per_step"),
                      "cp_fused_per_step": st["cp_fused_per_step"], "cp_layer_per_step": st.get("cp_layer_per_step")}), flush=True)


if __name__ == "__main__":
    main()
