"""TEST INFRASTRUCTURE ONLY -- never imported by the product path.

Fixtures for talker batches above 32 rows: the REFERENCE's own talker (oracle/gen_golden.py: `ref_talker`, driven by
`restated_sample_loop`) at `synth.talker_tiny()`, greedy, 10 token steps (9 frames), on ragged left-padded batches of 64 and 40 rows.
Needs the reference tree, like oracle/gen_golden.py; the files it writes are committed.

    python tools/gen_golden_b64.py [--only b64,b40]

Each tests/golden/talker_tiny_<name>.npz holds only what the reference produced -- codes (B, 9, 16), tokens (B, 10), margin (cb-0 top-2
margins after the processors, every token step) -- and weights_checksum; the tests rebuild the inputs with `prompt(name)`.

The comparison rule of this project stops at the first cb-0 flip behind a reference margin below 1e-3 (MARGIN_EXEMPT), and such a stop
could hide a failure: the generator refuses a seed whose smallest cb-0 margin is below that, and the tests assert that all 9 frames
were compared.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, ROOT)
import synth  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
N_TRAIL, MAX_NEW, MARGIN_EXEMPT = 2, 10, 1e-3
# name -> (rows, seed).  Seeds 116 / 107 (B = 64) and 125 / 116 (B = 40) also keep every margin above MARGIN_EXEMPT.
CASES = {"b64": (64, 111), "b40": (40, 129)}


def lens(B: int):
    return [3 + (7 * i) % 13 for i in range(B)]


def prompt(name: str):
    B, seed = CASES[name]
    return synth.rand_prompt(np.random.default_rng(seed), synth.talker_tiny(), lens(B), N_TRAIL, scale=0.5)


def generate(name: str):
    import torch
    from gen_golden import ref_talker, restated_sample_loop
    t = synth.talker_tiny()
    w = synth.talker_weights(t)
    talker = ref_talker(t, w)
    emb, mask, trailing, pad = prompt(name)
    tr = {}
    with torch.no_grad():
        codes, toks, _ = restated_sample_loop(talker, t, emb, mask, trailing, pad, max_new_tokens=MAX_NEW, min_new_tokens=MAX_NEW, trace=tr)
    margin = torch.stack(tr["margin"], 1).numpy()
    assert float(margin.min()) >= MARGIN_EXEMPT, f"{name}: smallest cb-0 margin {margin.min():.2e} < {MARGIN_EXEMPT}: take the next seed"
    path = os.path.join(GOLDEN, f"talker_tiny_{name}.npz")
    np.savez_compressed(path, weights_checksum=synth.weights_checksum(w), codes=codes.numpy(), tokens=toks.numpy(), margin=margin)
    print(f"{name}: codes {tuple(codes.shape)} tokens {tuple(toks.shape)} min cb-0 margin {margin.min():.2e} -> {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=",".join(CASES))
    for n in ap.parse_args().only.split(","):
        generate(n)
