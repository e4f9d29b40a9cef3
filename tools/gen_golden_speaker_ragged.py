"""TEST INFRASTRUCTURE ONLY -- never imported by the product path.

Fixture for the ragged speaker-encoder batch (`qtts_speaker_embed_ragged`): the REFERENCE's own Qwen3TTSSpeakerEncoder (M:95-393) and
mel_spectrogram (M:402-464, fed the restated Slaney filterbank as in oracle/gen_golden.py: `gen_speaker_real`) at the released dims, run
CLIP BY CLIP -- as the reference does (inference/qwen3_tts_model.py:440-455) -- on three clips of different lengths.  Needs the reference
tree, like oracle/gen_golden.py; the file it writes is committed.

    python tools/gen_golden_speaker_ragged.py

tests/golden/speaker_ragged.npz: embedding (3, 2048), frames (3,), samples (3,), seed, weights_checksum.  No audio is stored: clip i is
`synth.rand_audio(seed + i, 1, samples[i])[0]`.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, ROOT)
import synth  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
SEED, SAMPLES = 311, (24000, 56789, 72000)


def clips():
    return [synth.rand_audio(SEED + i, 1, n)[0] for i, n in enumerate(SAMPLES)]


def generate():
    import ref_shims
    ref_shims.install()
    import torch
    import speaker_ref
    from qwen_tts.core.models import modeling_qwen3_tts as M
    from qwen_tts.core.models.configuration_qwen3_tts import Qwen3TTSSpeakerEncoderConfig
    c = synth.speaker_real()
    w = synth.speaker_weights(c)
    cfg = Qwen3TTSSpeakerEncoderConfig(mel_dim=c.mel_dim, enc_dim=c.enc_dim, enc_channels=list(c.enc_channels),
                                       enc_kernel_sizes=list(c.enc_kernel_sizes), enc_dilations=list(c.enc_dilations),
                                       enc_attention_channels=c.enc_attention_channels, enc_res2net_scale=c.enc_res2net_scale,
                                       enc_se_channels=c.enc_se_channels)
    m = M.Qwen3TTSSpeakerEncoder(cfg).eval()
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == synth.speaker_param_shapes(c)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=True)
    fb = speaker_ref.mel_filterbank_slaney(24000, 1024, 128, 0, 12000)
    M.librosa_mel_fn = lambda sr, n_fft, n_mels, fmin, fmax: fb                 # the stubbed third-party call
    embs, frames = [], []
    with torch.no_grad():
        for clip in clips():
            mel = M.mel_spectrogram(torch.from_numpy(clip).unsqueeze(0), n_fft=1024, num_mels=128, sampling_rate=24000, hop_size=256,
                                    win_size=1024, fmin=0, fmax=12000)
            embs.append(m(mel.transpose(1, 2))[0].numpy())                     # M:1951: mels (1, frames, 128)
            frames.append(mel.shape[-1])
    path = os.path.join(GOLDEN, "speaker_ragged.npz")
    np.savez_compressed(path, weights_checksum=synth.weights_checksum(w), seed=SEED, samples=np.asarray(SAMPLES, np.int64),
                        frames=np.asarray(frames, np.int64), embedding=np.stack(embs))
    print(f"speaker_ragged: samples {SAMPLES} -> frames {frames}, |max| {float(np.abs(np.stack(embs)).max()):.3f} -> {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    generate()
