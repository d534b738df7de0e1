"""The log-mel front end off its default geometry: the cases of tests/golden/mel_geometry.npz
(written by gen_goldens.py:gen_mel_geometry from the real reference) and their seeded audio,
shared by the generator, tests/test_oracle.py and tests/test_mel_geometry.py.

Each row is (sample_rate, n_fft, hop_length, n_mels, samples), the smallest shape that still
reaches the branch named (kFPB = 6 frames per real-FFT workgroup, kMelChunk = 16 frames per
chunk of the chunked mel pass, which needs n_mels <= 85 and n_fft // 2 + 1 <= 256)."""

import zlib

import numpy as np

CASES = [
    (16000, 400, 160, 40, 2560),     # FFT path, chunked mel, n_mels != 80, F = 17
    (16000, 400, 160, 85, 1000),     # kMaxMels itself (12 stat phases x 85 threads), F = 7
    (16000, 400, 160, 86, 1000),     # first unchunked n_mels; the last 16-bin block has 6 valid bins
    (16000, 400, 160, 128, 2560),    # unchunked; 4 empty filters
    (16000, 512, 128, 80, 2100),     # GEMM STFT K = 512, 257 bins > 256 -> unchunked with 80 bins
    (16000, 256, 64, 80, 1100),      # GEMM STFT K = 256, chunked with 129 bins; 2 empty filters
    (8000, 256, 80, 40, 1300),       # another sample rate, hop != n_fft / 4
    (16000, 64, 16, 8, 300),         # smallest GEMM: K = 64, N = 128, 33 bins
    (22050, 1024, 256, 128, 4000),   # K = 1024, 1011 non-zeros, F = 16
    (16000, 400, 200, 80, 2000),     # n_fft 400 but hop != 160: must take the GEMM path
    (16000, 400, 400, 80, 300),      # F = 1
]


def name(sr, n_fft, hop, n_mels, S):
    return f"sr{sr}_fft{n_fft}_hop{hop}_mel{n_mels}_S{S}"


def audio(case_name, S, B=2):
    """0.1 * standard_normal (B, S) float32, seeded from the case name."""
    rng = np.random.default_rng(zlib.crc32(case_name.encode()))
    return (0.1 * rng.standard_normal((B, S))).astype(np.float32)


def frames(S, n_fft, hop):
    return (S + 2 * (n_fft // 2) - n_fft) // hop + 1
