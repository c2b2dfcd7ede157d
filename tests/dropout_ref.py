"""The training plans' dropout mask restated in Python integers (include/gigl_hip.h: gigl_sage_train_plan_set_dropout) —
an independent implementation for the tests, never read by the library.

Philox4x32-10 (Random123): ten rounds of
    hi0:lo0 = 0xD2511F53 * c0,  hi1:lo1 = 0xCD9E8D57 * c2
    (c0, c1, c2, c3) <- (hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0)
with the key moved on by (0x9E3779B9, 0xBB67AE85) between rounds.  Element (row, col) of the output of conv layer `layer`
of encode `encode` at step `step` takes word col & 3 of the block with key (seed low, seed high) and counter
(row, col >> 2, step, (encode << 8) | layer); it is kept iff that word >= T = floor(float32(p) * 2^32)."""
import math

import numpy as np

M32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    c0, c1, c2, c3 = (int(v) & M32 for v in counter)
    k0, k1 = (int(v) & M32 for v in key)
    for r in range(10):
        if r:
            k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
    return c0, c1, c2, c3


def threshold(p: float) -> int:
    """T: the float32 p the library is handed, widened to double, times 2^32, floored"""
    return int(math.floor(float(np.float32(p)) * 4294967296.0))


def scale(p: float) -> np.float32:
    """what a kept element is multiplied by: 1.0f / (1.0f - p) in float32"""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def keep_mask(seed: int, step: int, encode: int, layer: int, rows: int, cols: int, p: float) -> np.ndarray:
    """uint8 [rows, cols]: 1 where element (row, col) is kept"""
    key = (seed & M32, (seed >> 32) & M32)
    T = threshold(p)
    tag = (encode << 8) | layer
    keep = np.zeros((rows, cols), dtype=np.uint8)
    for r in range(rows):
        for g in range((cols + 3) // 4):
            words = philox4x32_10((r, g, step, tag), key)
            for k in range(min(4, cols - 4 * g)):
                keep[r, 4 * g + k] = 1 if words[k] >= T else 0
    return keep
