"""The perturbed sequences of include/sfw_hip.h (sfw_sequences_perturb_stage) restated in numpy.

Pure numpy, no GPU.  For sample t, knot k and channel c (0 vx, 1 vy, 2 vtheta), with g = index_base + t:
  (w0, w1, w2, w3) = Philox4x32-10(counter = (g & 0xffffffff, g >> 32, k, c), key = (seed & 0xffffffff, seed >> 32));
  u1 = ((((w1 << 32) | w0) >> 11) + 1) * 2^-53 in (0, 1],  u2 = (((w3 << 32) | w2) >> 11) * 2^-53 in [0, 1);
  z = sqrt(-2 log u1) * cos(6.283185307179586 * u2);  z = 0 at g == 0 under KEEP_NOMINAL;
  knot = fmin(fmax(nominal[k][c] + sigma[c] * z, lo[c]), hi[c]), product and sum rounded on their own.
`reference` forms the knots with elementwise numpy operations (IEEE, one rounding each), so that with the device's own
normals handed in (`normals=`) the device's knots are reproduced bit for bit; with `normals=None` the only difference is
numpy's log and cos against the device library's.
"""
import numpy as np

KEEP_NOMINAL, NO_VY, KEEP_NORMALS = 1, 2, 4   # SFW_PERTURB_*
MAX_KNOTS = 64                                # SFW_SEQ_MAX_KNOTS
TWO_PI = 6.283185307179586
R_MAX = 8.58                                  # r <= sqrt(106 ln 2): u1 >= 2^-53

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LOW = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32(counter, key, rounds=10):
    """Random123's Philox4x32: counter = four and key = two arrays (or scalars) of 32-bit words, broadcast against each other.
    Returns the four output words as uint64 arrays holding 32-bit values."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & _LOW for c in counter)
    k0, k1 = (int(k) & 0xFFFFFFFF for k in key)
    for _ in range(rounds):
        p0, p1 = _M0 * c0, _M1 * c2      # 32 x 32 -> 64: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ np.uint64(k0), p1 & _LOW, (p0 >> _S32) ^ c3 ^ np.uint64(k1), p0 & _LOW
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def _words(seed, n, K, index_base):
    seed, index_base = int(seed), int(index_base)
    if not 0 <= seed < 1 << 64 or index_base < 0 or n < 1 or not 1 <= K <= MAX_KNOTS:
        raise ValueError("seed: 64 bits unsigned; index_base >= 0; n >= 1; 1 <= K <= 64")
    g = np.arange(n, dtype=np.uint64) + np.uint64(index_base)
    k = np.arange(K, dtype=np.uint64)[:, None, None]
    c = np.arange(3, dtype=np.uint64)[None, :, None]
    shape = (K, 3, n)
    return philox4x32((np.broadcast_to(g & _LOW, shape), np.broadcast_to(g >> _S32, shape), np.broadcast_to(k, shape),
                       np.broadcast_to(c, shape)), (seed & 0xFFFFFFFF, seed >> 32))


def uniforms(seed, n, K, index_base=0):
    """(u1, u2), each (K, 3, n): u1 in (0, 1], u2 in [0, 1), both exact multiples of 2^-53."""
    w0, w1, w2, w3 = _words(seed, n, K, index_base)
    m1 = ((w1 << _S32) | w0) >> np.uint64(11)
    m2 = ((w3 << _S32) | w2) >> np.uint64(11)
    return (m1 + np.uint64(1)).astype(np.float64) * 2.0 ** -53, m2.astype(np.float64) * 2.0 ** -53


def radius(seed, n, K, index_base=0):
    """r = sqrt(-2 log u1), (K, 3, n): the scale a normal's rounding error is measured in."""
    u1, _ = uniforms(seed, n, K, index_base)
    return np.sqrt(-2.0 * np.log(u1))


def normals(seed, n, K, index_base=0, flags=0):
    """z (K, 3, n), standard normal: Box-Muller's cosine branch over `uniforms`; 0.0 at global index 0 under KEEP_NOMINAL."""
    u1, u2 = uniforms(seed, n, K, index_base)
    z = np.sqrt(-2.0 * np.log(u1)) * np.cos(TWO_PI * u2)
    if flags & KEEP_NOMINAL and index_base == 0:
        z[:, :, 0] = 0.0
    return z


_draw = normals  # (reference's keyword `normals` shadows the function)


def reference(seed, nominal, sigma, lo, hi, n, index_base=0, flags=0, normals=None):
    """The knots (K, 3, n) of sfw_sequences_perturb_stage: nominal (K, 3), sigma / lo / hi (3,).  normals (K, 3, n) or None:
    they replace this module's z, e.g. the device's own (sfw_sequences_normals).  Under NO_VY channel 1 is 0.0."""
    nominal = np.asarray(nominal, dtype=np.float64)
    if nominal.ndim != 2 or nominal.shape[1] != 3:
        raise ValueError("nominal must be a (K, 3) array")
    K = nominal.shape[0]
    sigma, lo, hi = (np.asarray(a, dtype=np.float64).reshape(3) for a in (sigma, lo, hi))
    if not (np.all(np.isfinite(nominal)) and np.all(np.isfinite(sigma)) and np.all(np.isfinite(lo)) and np.all(np.isfinite(hi))):
        raise ValueError("non-finite nominal, sigma, lo or hi")
    if np.any(sigma < 0.0) or np.any(lo > hi):
        raise ValueError("sigma >= 0 and lo <= hi")
    if flags & NO_VY and (sigma[1] != 0.0 or np.any(nominal[:, 1] != 0.0)):
        raise ValueError("NO_VY: sigma[1] and every nominal vy must be 0")
    if normals is None:
        z = _draw(seed, n, K, index_base, flags)
    else:
        z = np.asarray(normals, dtype=np.float64).reshape(K, 3, n)
    step = sigma[None, :, None] * z                  # one rounding
    u = nominal[:, :, None] + step                   # one rounding
    u = np.fmin(np.fmax(u, lo[None, :, None]), hi[None, :, None])
    if flags & NO_VY:
        u[:, 1, :] = 0.0
    return u
