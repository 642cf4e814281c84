"""numpy restatement of the noise stream of the batch-assembly kernels (csrc/batch_rng.hip.h, docs/kernels/data.md):
Philox4x32-10 as published, in uint64 arithmetic, and the map from its words to standard normals, in float64."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57          # round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85          # key increments
MASK = np.uint64(0xFFFFFFFF)
TAG_NS, TAG_WB = 0x6E73, 0x7762          # counter word 3 of dlwp_ns_batch / dlwp_wb_batch
Z_MAX = float(np.sqrt(48 * np.log(2)))   # u1 >= 2^-24


def philox4x32_10(counter, key):
    """counter: four words (scalars or arrays of one shape), key: two words -> uint64 array [..., 4] of 32-bit words."""
    c = [np.asarray(w, dtype=np.uint64) & MASK for w in np.broadcast_arrays(*counter)]
    k = [np.uint64(int(key[0]) & 0xFFFFFFFF), np.uint64(int(key[1]) & 0xFFFFFFFF)]
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]          # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & MASK]
        k = [(k[0] + np.uint64(W0)) & MASK, (k[1] + np.uint64(W1)) & MASK]
    return np.stack(c, axis=-1)


def normals(seed, epoch, item, n, tag):
    """The standard normals of the elements 0 .. n-1 of dataset item `item` in epoch `epoch` under the 64-bit `seed`, float64."""
    seed = int(seed)
    groups = np.arange((n + 3) // 4, dtype=np.uint64)
    w = philox4x32_10((groups, item, epoch, tag), (seed & 0xFFFFFFFF, seed >> 32))
    z = np.empty((len(groups), 4))
    for q in (0, 1):
        u1 = ((w[:, 2 * q] >> np.uint64(8)).astype(np.float64) + 1.0) * 2.0 ** -24
        u2 = (w[:, 2 * q + 1] >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
        r = np.sqrt(-2.0 * np.log(u1))
        z[:, 2 * q] = r * np.cos(2.0 * np.pi * u2)
        z[:, 2 * q + 1] = r * np.sin(2.0 * np.pi * u2)
    return z.reshape(-1)[:n]
