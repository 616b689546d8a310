"""numpy reference of the forecast kernel's noise stream (include/vsde_hip.h: vsde_forecast): Philox4x32-10 (Random123) and the
Box-Muller transform, vectorised over numpy arrays of counters.

The normal of path b, step t, dim i is number t % 4 of philox4x32_10(counter {t // 4, i, b, 0}, key).  u is formed in float32
exactly as the kernel forms it (``(w >> 8) + 0.5`` rounds to nearest even once w >> 8 needs all 24 bits); log, sqrt, sin and cos
are then taken in float64."""
import numpy as np

_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = 0xFFFFFFFF


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Four uint32 arrays (broadcast together) of the Philox4x32-10 output words for counter (c0..c3) and key (k0, k1)."""
    c = [np.asarray(v, dtype=np.uint64) & _MASK for v in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = np.uint64(k0 & _MASK), np.uint64(k1 & _MASK)
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c[0], np.uint64(_M1) * c[2]
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & np.uint64(_MASK), p1 >> np.uint64(32), p1 & np.uint64(_MASK)
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
        k0, k1 = (k0 + np.uint64(_W0)) & np.uint64(_MASK), (k1 + np.uint64(_W1)) & np.uint64(_MASK)
    return [v.astype(np.uint32) for v in c]


def _uniform(w):
    return ((w >> np.uint32(8)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)


def box_muller(wa, wb):
    """(z_a, z_b) float64 from two uint32 word arrays."""
    r = np.sqrt(-2.0 * np.log(_uniform(wa).astype(np.float64)))
    ang = 2.0 * np.pi * _uniform(wb).astype(np.float64)
    return r * np.cos(ang), r * np.sin(ang)


def forecast_noise(B, T, S, key):
    """The kernel's normals as a float64 array [B, T, S] for key = (key0, key1) (unsigned or signed 32-bit ints)."""
    k0, k1 = (int(v) & _MASK for v in key)
    nblk = (T + 3) // 4
    blk, i, b = np.meshgrid(np.arange(nblk), np.arange(S), np.arange(B), indexing="ij")
    w = philox4x32_10(blk, i, b, 0, k0, k1)
    z0, z1 = box_muller(w[0], w[1])
    z2, z3 = box_muller(w[2], w[3])
    z = np.stack([z0, z1, z2, z3], axis=1)          # [nblk, 4, S, B]
    z = z.reshape(nblk * 4, S, B)[:T]                # step t = 4 blk + j
    return np.ascontiguousarray(z.transpose(2, 0, 1))
