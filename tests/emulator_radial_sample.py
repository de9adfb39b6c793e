"""The radius draw of usf_radial_sample_norm_f32 restated in numpy fp64 (include/usflows_hip_internal.h states the layout): Philox4x32-10
with 64-bit counters, the stream layout, the component choice and the five component kinds.  It takes the CONSTRAINED
parameters (softplus already applied) and imports nothing from the product; the device kernel is held to it row by row
(tests/test_radial_sample_gpu.py), and its own distribution is checked against scipy on the CPU (tests/test_radial_sample_cpu.py).
"""
import numpy as np

KINDS = ("lognormal", "gamma", "weibull", "halfnormal", "chi")
STREAM = 0x85EBCA6B                 # radius draws: Philox stream  offset ^ STREAM ^ (attempt << 32)
BOOST_ATTEMPT = 0xFFFF              # the "attempt" whose word 0 is the a < 1 boost's uniform
GAMMA_ATTEMPTS = 32
TINY32 = float(np.finfo(np.float32).tiny)

_M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(ctr, stream_id, seed):
    """ctr: uint64 array; stream_id, seed: Python ints (64 bit).  Returns the four uint32 words as uint64 arrays."""
    ctr = np.asarray(ctr, dtype=np.uint64)
    c0, c1 = ctr & _M32, ctr >> _S32
    c2 = np.full_like(ctr, np.uint64(stream_id & 0xFFFFFFFF))
    c3 = np.full_like(ctr, np.uint64((stream_id >> 32) & 0xFFFFFFFF))
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        n0 = (p1 >> _S32) ^ c1 ^ np.uint64(k0)
        n2 = (p0 >> _S32) ^ c3 ^ np.uint64(k1)
        c0, c1, c2, c3 = n0, p1 & _M32, n2, p0 & _M32
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0, c1, c2, c3


def u01(w):
    """(w + 1/2) 2^-32: exact in fp64, never 0 or 1"""
    return (w.astype(np.float64) + 0.5) * (1.0 / 4294967296.0)


def _normal(w1, w2):
    return np.sqrt(-2.0 * np.log(u01(w1))) * np.cos(6.28318530717958647692 * u01(w2))


def _ph(ctr, offset, seed, t):
    return philox4x32_10(ctr, (offset ^ STREAM ^ (t << 32)) & 0xFFFFFFFFFFFFFFFF, seed)


def component(w0, logits, K):
    """k = #{j : C_j <= u(w0) C_{K-1}} capped at K - 1, C the running sum of exp(l - max l) in index order"""
    if logits is None or K == 1:
        return np.zeros(w0.shape, dtype=np.int64)
    l = np.asarray(logits, dtype=np.float64)
    e = np.exp(l - l.max())
    C = np.empty(K)
    s = 0.0
    for j in range(K):
        s = s + e[j]
        C[j] = s
    t = u01(w0) * C[K - 1]
    k = (C[None, :] <= t[:, None]).sum(1)
    return np.minimum(k, K - 1)


def _gamma(shape, ctr, offset, seed, first, stats=None):
    """Gamma(shape, 1), Marsaglia-Tsang over the attempts' Philox blocks; shape: fp64 array per row"""
    a1 = np.where(shape < 1.0, shape + 1.0, shape)
    d = a1 - 1.0 / 3.0
    c = 1.0 / np.sqrt(9.0 * d)
    g = d.copy()
    pending = np.ones(shape.shape, dtype=bool)
    attempts = np.zeros(shape.shape, dtype=np.int64)
    for t in range(GAMMA_ATTEMPTS):
        idx = np.nonzero(pending)[0]
        if idx.size == 0:
            break
        w = [x[idx] for x in first] if t == 0 else _ph(ctr[idx], offset, seed, t)
        n = _normal(w[1], w[2])
        q = 1.0 + c[idx] * n
        v = q * q * q
        di = d[idx]
        with np.errstate(invalid="ignore", divide="ignore"):
            ok = (v > 0.0) & (np.log(u01(w[3])) < 0.5 * n * n + di - di * v + di * np.log(np.where(v > 0.0, v, 1.0)))
        g[idx[ok]] = di[ok] * v[ok]
        attempts[idx] += 1
        pending[idx[ok]] = False
    if stats is not None:
        stats["capped"] = int(pending.sum())
        stats["max_attempts"] = int(attempts.max()) if attempts.size else 0
    small = shape < 1.0
    if small.any():
        i = np.nonzero(small)[0]
        w0 = _ph(ctr[i], offset, seed, BOOST_ATTEMPT)[0]
        g[i] = g[i] * np.power(u01(w0), 1.0 / shape[i])
    return g


def radii(kind, a, b=None, logits=None, M=1, seed=0, offset=0, row_offset=0, stats=None):
    """fp32 radii [M] of rows row_offset .. row_offset + M - 1.  a, b: constrained parameters per component ([K] or scalars):
    lognormal (mu, sigma), gamma (concentration, rate), weibull (scale, concentration), halfnormal (sigma,), chi (df, scale)."""
    assert kind in KINDS
    a = np.atleast_1d(np.asarray(a, dtype=np.float64))
    K = a.size
    b = np.ones(K) if b is None else np.atleast_1d(np.asarray(b, dtype=np.float64))
    ctr = (np.arange(M, dtype=np.uint64) + np.uint64(row_offset))
    w = _ph(ctr, offset, seed, 0)
    k = component(w[0], logits, K)
    ak, bk = a[k], b[k]
    if kind == "lognormal":
        r = np.exp(ak + bk * _normal(w[1], w[2]))
    elif kind == "halfnormal":
        r = ak * np.abs(_normal(w[1], w[2]))
    elif kind == "weibull":
        r = ak * np.power(-np.log(u01(w[1])), 1.0 / bk)
    elif kind == "gamma":
        r = _gamma(ak, ctr, offset, seed, w, stats) / bk
    else:
        r = bk * np.sqrt(2.0 * _gamma(0.5 * ak, ctr, offset, seed, w, stats))
    return np.maximum(r, TINY32).astype(np.float32)
