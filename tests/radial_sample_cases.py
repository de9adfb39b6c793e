"""The fourteen norm distributions the seeded radial sampler is tested on (constrained parameter values), shared by
tests/test_radial_sample_cpu.py (the emulator's own distribution) and tests/test_radial_sample_gpu.py (the kernel against
the emulator)."""
import numpy as np

M_DRAW, SEED = 16384, 1234


def _rand(K, lo, span_a):
    """a in [lo, lo + span_a], b in [.2, 1.2], standard-normal logits (unequal weights: the component choice is part of what
    the cases test), in this order from default_rng(0)"""
    g = np.random.default_rng(0)
    a = lo + span_a * g.random(K)
    b = 0.2 + g.random(K)
    return a, b, g.standard_normal(K)


def cases():
    """name -> (kind, a [K], b [K] | None, logits [K] | None), fp32-representable fp64 values"""
    a20, b20, l20 = _rand(20, 1.0, 180.0)
    a64, b64, l64 = _rand(64, 0.6, 30.0)
    c = {
        "lognormal": ("lognormal", [6.0], [.35], None),
        "lognormal_x5": ("lognormal", np.linspace(-1, 3, 5), [.2, .5, 1, .3, .7], np.linspace(-1, 1, 5)),
        "gamma_0.5_2": ("gamma", [.5], [2.0], None),
        "gamma_1_0.7": ("gamma", [1.0], [.7], None),
        "gamma_392_0.5": ("gamma", [392.0], [.5], None),
        "gamma_x20": ("gamma", a20, b20, l20),
        "gamma_x64": ("gamma", a64, b64, l64),
        "weibull": ("weibull", [3.0], [.8], None),
        "weibull_x3": ("weibull", [1, 5, 20], [1.5, 4, 9], [.3, -.2, .1]),
        "halfnormal": ("halfnormal", [2.5], None, None),
        "halfnormal_x4": ("halfnormal", [.5, 1, 4, 9], None, [0, 1, -1, .5]),
        "chi_784_1.3": ("chi", [784.0], [1.3], None),
        "chi_1_1": ("chi", [1.0], [1.0], None),
        "chi_3_0.5": ("chi", [3.0], [.5], None),
    }
    f32 = lambda v: None if v is None else np.asarray(v, dtype=np.float32).astype(np.float64)
    return {n: (k, f32(a), f32(b), f32(l)) for n, (k, a, b, l) in c.items()}


CASE_NAMES = list(cases())


def mixture_cdf(kind, a, b, logits, x):
    """the analytic CDF of the (mixture) distribution at x, from scipy.stats"""
    from scipy import stats
    K = len(a)
    w = np.ones(1) if logits is None else np.exp(logits - logits.max()) / np.exp(logits - logits.max()).sum()
    out = np.zeros_like(x)
    for k in range(K):
        if kind == "lognormal":
            F = stats.lognorm.cdf(x, s=b[k], scale=np.exp(a[k]))
        elif kind == "gamma":
            F = stats.gamma.cdf(x, a[k], scale=1.0 / b[k])
        elif kind == "weibull":
            F = stats.weibull_min.cdf(x, b[k], scale=a[k])
        elif kind == "halfnormal":
            F = stats.halfnorm.cdf(x, scale=a[k])
        else:
            F = stats.chi.cdf(x, a[k], scale=b[k])
        out += w[k] * F
    return out


def ks_distance(kind, a, b, logits, r):
    x = np.sort(np.asarray(r, dtype=np.float64))
    n = x.size
    F = mixture_cdf(kind, a, b, logits, x)
    return max((np.arange(1, n + 1) / n - F).max(), (F - np.arange(0, n) / n).max())
