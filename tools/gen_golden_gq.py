"""TEST INFRASTRUCTURE ONLY -- never imported by the product path.

Fixtures for the head shapes beyond the released checkpoints' (head_dim 64 | 128, GQA groups up to 8): the REFERENCE's own talker
(oracle/gen_golden.py: `ref_talker`, driven by `restated_sample_loop`) at tiny dims with three head shapes, greedy, on one ragged
left-padded batch.  Needs the reference tree, like oracle/gen_golden.py; the files it writes are committed.

    python tools/gen_golden_gq.py [--only gq8_hd128,gq4_hd64,gq5_hd128]

Each tests/golden/talker_tiny_<name>.npz: embeds, mask, trailing, tts_pad (the inputs), codes (5, 39, 16), tokens (5, 40), margin (cb-0 top-2
margins after the processors, every token step), logits (raw cb-0 logits of the first 8 token steps), weights_checksum.
"""
import argparse
import dataclasses
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, ROOT)
import synth  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
LENS, N_TRAIL, SEED, MAX_NEW = [3, 9, 14, 6, 11], 2, 9, 40
LOGIT_STEPS = 8         # raw cb-0 logits are kept for the first token steps only (the whole trace would be 1 MB per file)
# name -> (talker heads, kv heads, head_dim, code predictor heads, kv heads, head_dim)
SHAPES = {
    "gq8_hd128": (8, 1, 128, 4, 1, 128),
    "gq4_hd64": (8, 2, 64, 8, 1, 64),
    "gq5_hd128": (5, 1, 128, 3, 1, 128),
}


def cfg(name: str) -> synth.TalkerCfg:
    nh, nkv, hd, cnh, cnkv, chd = SHAPES[name]
    return dataclasses.replace(synth.talker_tiny(), num_attention_heads=nh, num_key_value_heads=nkv, head_dim=hd,
                               cp_num_attention_heads=cnh, cp_num_key_value_heads=cnkv, cp_head_dim=chd)


def prompt(t: synth.TalkerCfg):
    return synth.rand_prompt(np.random.default_rng(SEED), t, LENS, N_TRAIL, scale=0.5)


def generate(name: str):
    import torch
    from gen_golden import ref_talker, restated_sample_loop
    t = cfg(name)
    w = synth.talker_weights(t)
    talker = ref_talker(t, w)
    emb, mask, trailing, pad = prompt(t)
    tr = {}
    with torch.no_grad():
        codes, toks, _ = restated_sample_loop(talker, t, emb, mask, trailing, pad, max_new_tokens=MAX_NEW, min_new_tokens=MAX_NEW, trace=tr)
    margin = torch.stack(tr["margin"], 1).numpy()
    out = dict(weights_checksum=synth.weights_checksum(w), embeds=emb.numpy(), mask=mask.numpy(), trailing=trailing.numpy(),
               tts_pad=pad.numpy(), codes=codes.numpy(), tokens=toks.numpy(), logits=torch.stack(tr["logits"][:LOGIT_STEPS], 1).numpy(), margin=margin)
    path = os.path.join(GOLDEN, f"talker_tiny_{name}.npz")
    np.savez_compressed(path, **out)
    print(f"{name}: codes {tuple(codes.shape)} tokens {tuple(toks.shape)} min cb-0 margin {margin.min():.2e} -> {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=",".join(SHAPES))
    for n in ap.parse_args().only.split(","):
        generate(n)
