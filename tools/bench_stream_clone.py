#!/usr/bin/env python3
"""Streaming voice clone: what priming a codec slot from reference codes costs, and what the stream delivers.  Released codec dims and
1.7B talker dims, bf16, synthetic weights.

    python tools/bench_stream_clone.py                         # both legs
    python tools/bench_stream_clone.py --skip-stream           # the codec leg only

Two legs, one JSON line per configuration:

  * "prime_rows": `CodecDecoderEngine.stream_prime_rows` for 1 / 4 / 8 rows whose references are spread evenly over 3 .. 10 s (37 .. 125
    frames; one row: 10 s), three routes INTERLEAVED round by round in one process: the tail on (default), the tail off
    (QTTS_CODEC_PRIME_TAIL=0: the whole reference goes through the upsampling stack), and the only route there was before the entry point
    -- `stream_reset_rows` + one `stream_push_rows` per distinct length, PCM discarded.  Median of the rounds behind one warm-up round;
    host wall clock around synchronised calls.
  * "stream_clone": the packet loop of `Qwen3TTSModel.stream_voice_clone(schedule="continuous")` driven at the engine level (random
    prompt embeddings of the ICL prompt's length in place of the tokenizer and the prompt assembly, as tools/bench_configs.py builds
    BASELINE config 5): 38 reference frames per request, text of 16 .. 72 tokens, frames ~ 2.2 x text tokens, 2 x batch requests on
    `batch` rows.  Per request the time from the start of the call to its first PCM on the host; per packet the codec's share (prime +
    push, synchronised)."""
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
from qwen3_tts_amd import _lib  # noqa: E402
from qwen3_tts_amd.codec import CodecDecoderEngine  # noqa: E402

DEV = "cuda:0"


def _block(refs, n_max):
    block = torch.zeros(len(refs), refs[0].shape[0], n_max, dtype=torch.long, device=DEV)
    for m, r in enumerate(refs):
        block[m, :, n_max - r.shape[-1]:] = r
    return block


def prime_leg(codec, c, rounds):
    g = np.random.default_rng(3)
    for M in (1, 4, 8):
        lens = [125] if M == 1 else [int(round(x)) for x in np.linspace(37, 125, M)]
        refs = [torch.from_numpy(g.integers(0, c.codebook_size, (c.num_quantizers, n))).to(DEV) for n in lens]
        ids = list(range(M))
        block = _block(refs, max(lens))
        codec.stream_begin(M)

        def prime(tail):
            _lib.set_option("QTTS_CODEC_PRIME_TAIL", None if tail else 0, lib=codec._lib)
            try:
                codec.stream_prime_rows(ids, block, lens)
            finally:
                _lib.set_option("QTTS_CODEC_PRIME_TAIL", None, lib=codec._lib)

        def push_route():
            codec.stream_reset_rows(ids)
            for m, r in enumerate(refs):                   # distinct lengths: one call each, the PCM dropped
                codec.stream_push_rows([m], r[None])

        routes = {"tail_on": lambda: prime(True), "tail_off": lambda: prime(False), "reset_push": push_route}
        ms = {k: [] for k in routes}
        for r in range(rounds + 1):
            for name, fn in routes.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if r:                                      # round 0: warm-up
                    ms[name].append(1e3 * (time.perf_counter() - t0))
        med = {k: float(np.median(v)) for k, v in ms.items()}
        print(json.dumps({"bench": "prime_rows", "rows": M, "ref_frames": lens, "rounds": rounds,
                          **{k + "_ms": round(v, 3) for k, v in med.items()},
                          **{k + "_ms_min_max": [round(min(v), 3), round(max(v), 3)] for k, v in ms.items()},
                          "tail_off_over_tail_on": round(med["tail_off"] / med["tail_on"], 2),
                          "reset_push_over_tail_on": round(med["reset_push"] / med["tail_on"], 2)}), flush=True)


def stream_leg(c, cw, B, k, scale):
    from bench_row_sampling import weights
    from qwen3_tts_amd.talker import TalkerEngine
    t = synth.talker_17b()
    REF, N = 38, 2 * B
    rq = np.random.default_rng(5)
    text = rq.integers(16, 72, N).tolist()
    limits = [max(3, int(round(scale * 2.2 * x))) + 1 for x in text]
    lens = [12 + REF + 16 + (x % 7) for x in text]
    args = synth.rand_prompt(np.random.default_rng(1), t, lens, max(text), 0.05)
    talker = TalkerEngine(t, weights(t), weight_dtype=torch.bfloat16, device=DEV, max_batch=B, max_seq=max(lens) + max(limits) + 64, use_graph=True)
    codec = CodecDecoderEngine(c, cw, compute_dtype=torch.bfloat16, device=DEV, max_batch=B, max_frames=80 + REF)
    g = np.random.default_rng(7)
    refs = [torch.from_numpy(g.integers(0, c.codebook_size, (c.num_quantizers, REF))).to(DEV) for _ in range(N)]
    sup = [i for i in range(t.vocab_size - 1024, t.vocab_size) if i != t.codec_eos_token_id]
    kw = dict(schedule="continuous", packet_frames=k, max_new_tokens=limits, min_new_tokens=max(limits) + 1, suppress_tokens=sup,
              repetition_penalty=1.05, do_sample=True, top_k=50, top_p=1.0, temperature=0.9, seed=[1000 + i for i in range(N)])
    cb, up = c.codebook_size, c.total_upsample

    def run():
        first_audio, samples, codec_ms, prime_ms = [None] * N, [0] * N, [], []
        codec.stream_begin(B)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for record in talker.generate_stream(*args, **kw):
            started = [e for e in record.rows if e.first]
            torch.cuda.synchronize()
            c0 = time.perf_counter()
            if started:
                codec.stream_prime_rows([e.row for e in started], _block([refs[e.request] for e in started], REF), [REF] * len(started))
                torch.cuda.synchronize()
                prime_ms.append(1e3 * (time.perf_counter() - c0))
            live = [e for e in record.rows if e.codes.shape[0] > 0]
            if not live:
                continue
            n = max(int(e.codes.shape[0]) for e in live)
            batch = torch.zeros(len(live), n, t.num_code_groups, dtype=torch.long, device=DEV)
            for m, e in enumerate(live):
                batch[m, : e.codes.shape[0]] = e.codes.clamp(min=0, max=cb - 1)
            wav = codec.stream_push_rows([e.row for e in live], batch.transpose(1, 2))[:, 0].cpu()       # PCM on the host
            now = time.perf_counter()
            codec_ms.append(1e3 * (now - c0))
            for m, e in enumerate(live):
                samples[e.request] += int(e.codes.shape[0]) * up
                if first_audio[e.request] is None:
                    first_audio[e.request] = now - t0
            del wav
        return time.perf_counter() - t0, first_audio, samples, codec_ms, prime_ms

    run()                                            # warm-up: graph captures, code objects, allocator
    wall, first_audio, samples, codec_ms, prime_ms = run()
    assert samples == [(m - 1) * up for m in limits], "a request's audio has the wrong length"
    fa = np.array(first_audio)
    print(json.dumps({"bench": "stream_clone", "max_batch": B, "requests": N, "packet_frames": k, "ref_frames": REF, "wall_s": round(wall, 4),
                      "audio_s": round(sum(samples) / 24000.0, 2), "occupancy": round(talker.last_refill["occupancy"], 4),
                      "first_audio_ms_first_rows": {"min": round(1e3 * float(np.sort(fa)[:B].min()), 2),
                                                    "max": round(1e3 * float(np.sort(fa)[:B].max()), 2)},
                      "first_audio_ms_all": {"min": round(1e3 * fa.min(), 2), "median": round(1e3 * float(np.median(fa)), 2),
                                             "max": round(1e3 * fa.max(), 2)},
                      "codec_ms_per_packet": {"median": round(float(np.median(codec_ms)), 3), "max": round(max(codec_ms), 3),
                                              "packets": len(codec_ms)},
                      "prime_calls": len(prime_ms), "prime_ms": {"first": round(prime_ms[0], 3), "median": round(float(np.median(prime_ms)), 3)}}),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--packet", type=int, default=4)
    ap.add_argument("--scale", type=float, default=0.5, help="generated frames = scale x 2.2 x text tokens (the stream leg)")
    ap.add_argument("--batches", type=int, nargs="*", default=[8, 32])
    ap.add_argument("--skip-stream", action="store_true")
    ap.add_argument("--skip-prime", action="store_true")
    a = ap.parse_args()
    c = synth.codec_real()
    cw = {n: torch.from_numpy(v) for n, v in synth.codec_weights(c).items()}
    if not a.skip_prime:
        prime_leg(CodecDecoderEngine(c, cw, compute_dtype=torch.bfloat16, device=DEV, max_batch=8, max_frames=200), c, a.rounds)
    if not a.skip_stream:
        for B in a.batches:
            stream_leg(c, cw, B, a.packet, a.scale)


if __name__ == "__main__":
    main()
