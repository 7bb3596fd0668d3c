"""
The NumPy model of csrc/neo_counter_rng.hpp: the counter-based jitter of the plan retries and of the fleet's
re-targeting.  Every function here does the header's operations in the header's order, each rounded on its own, so the
kernels (plan_jitter_kernel, fleet_jitter_kernel) reproduce these arrays bit for bit.

A value is a pure function of (seed, id, a, b, domain, index): Philox4x32-10 (Salmon et al., SC'11) with the key
(seed's low word, seed's high word) and the counter (id, a, b, domain << 24 | j); value e of a stream comes from block
j = e >> 1, output words (0, 1) when e is even and (2, 3) when it is odd; the two words make a 52-bit uniform strictly
inside (0, 1), and Wichura's AS241 PPND16 makes it a unit normal.

  domain 1   retry noise      a = attempt, b = 0        D * count values, e = d * count + k, scaled by 0.5
  domain 2   target jitter    a = tick,    b = target   2 values; target 0 draws nothing (zeros)
"""
import numpy as np

DOMAIN_RETRY, DOMAIN_TARGET = 1, 2
JITTERS = ("numpy", "counter")

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LOW = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """the block function: counter (..., 4) and key (..., 2) of 32-bit words (broadcast against each other) -> (..., 4) uint32"""
    counter = np.asarray(counter, dtype=np.uint64)
    key = np.asarray(key, dtype=np.uint64)
    shape = np.broadcast_shapes(counter.shape[:-1], key.shape[:-1])
    c0, c1, c2, c3 = (np.broadcast_to(counter[..., i], shape) for i in range(4))
    k0, k1 = (np.broadcast_to(key[..., i], shape) for i in range(2))
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2                       # (below 2^64: both factors are 32-bit words)
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _LOW, (p0 >> _S32) ^ c3 ^ k1, p0 & _LOW
        k0, k1 = (k0 + np.uint64(_W0)) & _LOW, (k1 + np.uint64(_W1)) & _LOW
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def uniform(wa, wb):
    """two 32-bit words -> u = (((wa >> 6) * 2^26 + (wb >> 6)) + 0.5) * 2^-52, exact, strictly inside (0, 1)"""
    wa = np.asarray(wa, dtype=np.uint64); wb = np.asarray(wb, dtype=np.uint64)
    k = ((wa >> np.uint64(6)) << np.uint64(26)) | (wb >> np.uint64(6))
    return (k.astype(np.float64) + 0.5) * 2.0 ** -52


_LN2_HI, _LN2_LO = 6.93147180369123816490e-01, 1.90821492927058770002e-10
_SQRT2_MANT = np.uint64(0x6A09E667F3BCD)


def log(x):
    """ln x for positive normal x, from the bits and + - * / only (the header's counter_log)"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    bits = x.view(np.uint64)
    mant = bits & np.uint64(0x000FFFFFFFFFFFFF)
    e = (bits >> np.uint64(52)).astype(np.int64) - 1023
    big = mant >= _SQRT2_MANT
    e = e + big
    ex = np.where(big, np.uint64(1022), np.uint64(1023))
    m = ((ex << np.uint64(52)) | mant).view(np.float64)
    s = (m - 1.0) / (m + 1.0)
    t = s * s
    p = np.full(x.shape, 1.0 / 23.0)
    for d in (21.0, 19.0, 17.0, 15.0, 13.0, 11.0, 9.0, 7.0, 5.0, 3.0):
        p = p * t + 1.0 / d
    p = p * t + 1.0
    de = e.astype(np.float64)
    lo = (2.0 * s) * p + de * _LN2_LO
    return de * _LN2_HI + lo


# AS241 PPND16: numerator and denominator coefficients, highest power first, as CPython's statistics.py writes them
_A = (2.5090809287301226727e+3, 3.3430575583588128105e+4, 6.7265770927008700853e+4, 4.5921953931549871457e+4,
      1.3731693765509461125e+4, 1.9715909503065514427e+3, 1.3314166789178437745e+2, 3.3871328727963666080e+0)
_B = (5.2264952788528545610e+3, 2.8729085735721942674e+4, 3.9307895800092710610e+4, 2.1213794301586595867e+4,
      5.3941960214247511077e+3, 6.8718700749205790830e+2, 4.2313330701600911252e+1, 1.0)
_C = (7.74545014278341407640e-4, 2.27238449892691845833e-2, 2.41780725177450611770e-1, 1.27045825245236838258e+0,
      3.64784832476320460504e+0, 5.76949722146069140550e+0, 4.63033784615654529590e+0, 1.42343711074968357734e+0)
_D = (1.05075007164441684324e-9, 5.47593808499534494600e-4, 1.51986665636164571966e-2, 1.48103976427480074590e-1,
      6.89767334985100004550e-1, 1.67638483018380384940e+0, 2.05319162663775882187e+0, 1.0)
_E = (2.01033439929228813265e-7, 2.71155556874348757815e-5, 1.24266094738807843860e-3, 2.65321895265761230930e-2,
      2.96560571828504891230e-1, 1.78482653991729133580e+0, 5.46378491116411436990e+0, 6.65790464350110377720e+0)
_F = (2.04426310338993978564e-15, 1.42151175831644588870e-7, 1.84631831751005468180e-5, 7.86869131145613259100e-4,
      1.48753612908506148525e-2, 1.36929880922735805310e-1, 5.99832206555887937690e-1, 1.0)


def _horner(coef, r):
    acc = coef[0] * r + coef[1]
    for c in coef[2:]:
        acc = acc * r + c
    return acc


def probit_branch(u):
    """which AS241 branch a uniform takes: 0 central (|u - 0.5| <= 0.425), 1 tail with sqrt(-ln) <= 5, 2 far tail"""
    u = np.asarray(u, dtype=np.float64)
    q = u - 0.5
    out = np.zeros(u.shape, dtype=np.int64)
    tail = np.abs(q) > 0.425
    if tail.any():
        rt = np.where(q[tail] <= 0.0, u[tail], 1.0 - u[tail])
        out[tail] = np.where(np.sqrt(-log(rt)) <= 5.0, 1, 2)
    return out


def probit(u):
    """Phi^-1(u), 0 < u < 1 (the header's counter_probit)"""
    u = np.asarray(u, dtype=np.float64)
    q = u - 0.5
    z = np.empty(u.shape, dtype=np.float64)
    central = np.abs(q) <= 0.425
    qc = q[central]
    r = 0.180625 - qc * qc
    z[central] = (_horner(_A, r) * qc) / _horner(_B, r)
    tail = ~central
    if tail.any():
        ut, qt = u[tail], q[tail]
        r = np.sqrt(-log(np.where(qt <= 0.0, ut, 1.0 - ut)))
        near = r <= 5.0
        r1, r2 = r - 1.6, r - 5.0
        x = np.where(near, _horner(_C, r1) / _horner(_D, r1), _horner(_E, r2) / _horner(_F, r2))
        z[tail] = np.where(qt < 0.0, -x, x)
    return z


def check_seed(seed, who):
    seed = int(seed)
    if not 0 <= seed < 2 ** 64:
        raise ValueError("%s: jitter='counter' needs a seed in 0 .. 2^64 - 1" % who)
    return seed


def check_ids(ids, who):
    """the stream ids as int64 (n,): each in 0 .. 2^31 - 1 (the resident id arrays are int32)"""
    ids = np.asarray(ids).reshape(-1)
    if ids.size and (ids.dtype.kind not in "iu" or int(ids.min()) < 0 or int(ids.max()) >= 2 ** 31):
        raise ValueError("%s: jitter='counter' needs integer ids in 0 .. 2^31 - 1" % who)
    return ids.astype(np.int64)


def check_word(v, name, who):
    v = int(v)
    if not 0 <= v < 2 ** 31:
        raise ValueError("%s: %s must be in 0 .. 2^31 - 1" % (who, name))
    return v


def check_jitter(jitter, who):
    if jitter not in JITTERS:
        raise ValueError("%s: jitter must be 'numpy' or 'counter'" % who)
    return jitter == "counter"


def stream_words(seed, ids, a, b, domain, nblocks):
    """blocks 0 .. nblocks - 1 of the streams (seed, id, a, b, domain), id over ids: (len(ids), nblocks, 4) uint32"""
    ids = np.asarray(ids, dtype=np.uint64).reshape(-1)
    if nblocks > 1 << 24:
        raise ValueError("counter_rng: a stream has at most 2^25 values")
    counter = np.empty((ids.shape[0], nblocks, 4), dtype=np.uint64)
    counter[..., 0] = ids[:, None]
    counter[..., 1] = int(a)
    counter[..., 2] = int(b)
    counter[..., 3] = (int(domain) << 24) | np.arange(nblocks, dtype=np.uint64)[None, :]
    seed = int(seed)
    return philox4x32_10(counter, np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint64))


def stream_uniforms(seed, ids, a, b, domain, nvalues):
    """values 0 .. nvalues - 1 of the streams as uniforms: (len(ids), nvalues)"""
    w = stream_words(seed, ids, a, b, domain, (int(nvalues) + 1) // 2)
    return uniform(w[..., 0::2], w[..., 1::2]).reshape(w.shape[0], 2 * w.shape[1])[:, :int(nvalues)]


def stream_normals(seed, ids, a, b, domain, nvalues):
    """values 0 .. nvalues - 1 of the streams as unit normals: (len(ids), nvalues)"""
    return probit(stream_uniforms(seed, ids, a, b, domain, nvalues))


def retry_noise(seed, stream_ids, attempt, D, count):
    """(len(stream_ids), D, count): 0.5 * the unit draws of domain 1 (the reference's N(0, 0.5), :94), e = d * count + k"""
    who = "retry_noise_counter"
    ids = check_ids(stream_ids, who)
    z = stream_normals(check_seed(seed, who), ids, check_word(attempt, "attempt", who), 0, DOMAIN_RETRY, int(D) * int(count))
    return 0.5 * z.reshape(ids.shape[0], int(D), int(count))


def target_jitter(seed, mission_ids, tick, target):
    """(len(mission_ids), 2): the unit draws of domain 2; target 0 gives zeros without drawing"""
    who = "target_jitter_counter"
    ids = check_ids(mission_ids, who)
    seed, tick, target = check_seed(seed, who), check_word(tick, "tick", who), check_word(target, "target", who)
    if target == 0:
        return np.zeros((ids.shape[0], 2))
    return stream_normals(seed, ids, tick, target, DOMAIN_TARGET, 2)
