"""numpy restatement of dsn_train_draws' rule (include/dsnerf.h): Philox4x32-10, the addressing (seed, step, ray id, quad, kind), the
jitter's 24-bit conversion and the noise's float64 Box-Muller.  Written from the rule, not from the kernel: integer arithmetic in
uint64 with explicit masks, the float64 part with numpy's log / cos / sin (the device library's may differ in the last float64 bits)."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
KIND_JITTER, KIND_NOISE = 0, 1
TWO_PI = 6.283185307179586
Z_MAX = float(np.sqrt(64.0 * np.log(2.0)))          # u1 = 2^-32: the largest |z| the rule can give (6.66)

KNOWN_ANSWERS = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def philox4x32(counter, key, rounds=10):
    """counter: four arrays (or ints) of 32-bit words, key: two; broadcast against each other -> uint32 [..., 4]"""
    c = [np.asarray(x, dtype=np.uint64) & MASK for x in counter]
    k = [np.asarray(x, dtype=np.uint64) & MASK for x in key]
    c = list(np.broadcast_arrays(*c, *k)[:4])
    for _ in range(rounds):
        p0 = np.uint64(M0) * c[0]           # < 2^64: no wrap
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & MASK]
        k = [(k[0] + np.uint64(W0)) & MASK, (k[1] + np.uint64(W1)) & MASK]
    return np.stack(c, axis=-1).astype(np.uint32)


def jitter_from_words(x):
    """u = (x >> 8) 2^-24: exact in float32"""
    return ((np.asarray(x, np.uint32) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)


def box_muller(a, b):
    """word pair -> (z0, z1, r): float64 throughout, z rounded to float32 once"""
    u1 = (np.asarray(a, np.uint32).astype(np.float64) + 1.0) * 2.0 ** -32
    u2 = np.asarray(b, np.uint32).astype(np.float64) * 2.0 ** -32
    r = np.sqrt(-2.0 * np.log(u1))
    t = TWO_PI * u2
    return (r * np.cos(t)).astype(np.float32), (r * np.sin(t)).astype(np.float32), r


def noise_from_words(x, noise_std=1.0):
    """x: uint32 [..., 4] -> float32 [..., 4]: the unit draws times noise_std in float32"""
    x = np.asarray(x, np.uint32)
    z0, z1, _ = box_muller(x[..., 0], x[..., 1])
    z2, z3, _ = box_muller(x[..., 2], x[..., 3])
    return (np.stack([z0, z1, z2, z3], axis=-1) * np.float32(noise_std)).astype(np.float32)


def ray_id_words(R, ray_base=0, ray_ids=None):
    if ray_ids is not None:
        ids = np.asarray(ray_ids).astype(np.int64)
        assert ids.shape == (R,)
        return (ids & 0xFFFFFFFF).astype(np.uint64)
    return ((np.arange(R, dtype=np.uint64) + np.uint64(int(ray_base) & 0xFFFFFFFF)) & MASK)


def words(R, S, seed, step, kind, ray_base=0, ray_ids=None):
    """the generator's words for every (ray, quad): uint32 [R, ceil(S / 4), 4]"""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    nq = (S + 3) // 4
    ids = ray_id_words(R, ray_base, ray_ids)[:, None]
    q = np.arange(nq, dtype=np.uint64)[None, :]
    return philox4x32((q, ids, int(step) & 0xFFFFFFFF, kind), (seed & 0xFFFFFFFF, seed >> 32)).reshape(R, nq, 4)


def draws(R, S, seed, step, ray_base=0, ray_ids=None, noise_std=1.0, want_jitter=True, want_noise=True):
    """(jitter, noise): float32 [R, S] each, None where not wanted - what dsn_train_draws writes"""
    jitter = noise = None
    if want_jitter:
        jitter = jitter_from_words(words(R, S, seed, step, KIND_JITTER, ray_base, ray_ids)).reshape(R, 4 * ((S + 3) // 4))[:, :S].copy()
    if want_noise:
        noise = noise_from_words(words(R, S, seed, step, KIND_NOISE, ray_base, ray_ids), noise_std).reshape(R, 4 * ((S + 3) // 4))[:, :S].copy()
    return jitter, noise


def ulp_distance(a, b):
    """distance in float32 units in the last place between two finite arrays (the sign-magnitude bits mapped to a line; +0 and -0
    coincide)"""
    def line(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(line(a) - line(b))
