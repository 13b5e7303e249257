"""What the host and GPU tests of the batch-statistics BatchNorm backward (rtod_bn_grad, csrc/bn_grad.hip) share: the shapes and the
numpy float64 model of the three formulas

    S1 = sum du                      S2 = sum du (z - mean)
    dbeta  = S1                      dgamma = S2 r                          r = 1 / sqrt(var + 1e-5)
    dz_i   = gamma r ( du_i - S1 / N - (z_i - mean) r r S2 / N )            N = B H W

with, for every output, the sum of the absolute values of its terms (its "mass"): what a bound on the rounding of a float64 sum of
N terms multiplies."""
import numpy as np

F = np.float32
U = 2.0 ** -24
EPS = 1e-5

# (B, C, H, W): an odd plane at a misaligned start with C no multiple of 4; the 13 x 13 plane; more channels than a workgroup has
# threads on 16-pixel planes; several parts with a ragged tail
SHAPES = [(2, 3, 5, 5), (3, 32, 13, 13), (2, 260, 4, 4), (1, 8, 67, 61)]
PARTS_SHAPE = (1, 8, 67, 61)


def batch_stats(z):
    """Per-channel mean and biased variance of ``z`` [B,C,H,W] in float64 (what F.batch_norm(training=True) normalises with)."""
    z = z.astype(np.float64)
    return z.mean(axis=(0, 2, 3)), z.var(axis=(0, 2, 3))


def bn_grad_model(du, z, mean, var, gamma):
    """``(dz, dgamma, dbeta, mass_dz, mass_dgamma, mass_dbeta)`` in float64 from ``du``, ``z`` [B,C,H,W], ``mean``, ``var``, ``gamma`` [C]."""
    du, z = du.astype(np.float64), z.astype(np.float64)
    mean, var, gamma = (np.asarray(a, np.float64).reshape(1, -1, 1, 1) for a in (mean, var, gamma))
    N = du.shape[0] * du.shape[2] * du.shape[3]
    r = 1.0 / np.sqrt(var + EPS)
    d = z - mean
    ax = (0, 2, 3)
    S1, S2 = du.sum(axis=ax, keepdims=True), (du * d).sum(axis=ax, keepdims=True)
    A1, A2 = np.abs(du).sum(axis=ax, keepdims=True), np.abs(du * d).sum(axis=ax, keepdims=True)
    dz = gamma * r * (du - S1 / N - d * r * r * S2 / N)
    mass_dz = np.abs(gamma) * r * (np.abs(du) + A1 / N + np.abs(d) * r * r * A2 / N)
    return dz, (S2 * r).ravel(), S1.ravel(), mass_dz, (A2 * r).ravel(), A1.ravel()


def float_case(shape, seed=0):
    """Random float32 ``du``, ``z`` (a per-channel offset and spread, so mean and variance differ by channel) and ``gamma`` of ``shape``."""
    B, C_, H, W = shape
    rng = np.random.default_rng(1000 * seed + B * 131 + C_ * 17 + H * W)
    du = rng.standard_normal(shape).astype(F)
    z = (rng.standard_normal(shape) * rng.uniform(0.5, 2.0, (1, C_, 1, 1)) + rng.uniform(-1.0, 1.0, (1, C_, 1, 1))).astype(F)
    gamma = rng.uniform(0.5, 1.5, C_).astype(F) * rng.choice([-1.0, 1.0], C_).astype(F)
    return du, z, gamma


def integer_case(shape):
    """``du`` in -2..2 and ``z`` in {-1, +1}, as many of each per channel as N allows (an odd N leaves one over): with the mean 0 that
    the test hands to the kernel, S1 and S2 are small integers, exact in every order of summation."""
    B, C_, H, W = shape
    rng = np.random.default_rng(B * 7 + C_ * 3 + H * W)
    du = rng.integers(-2, 3, shape).astype(F)
    N = B * H * W
    z = np.empty((C_, N), F)
    for c in range(C_):
        z[c] = rng.permutation(np.where(np.arange(N) % 2 == 0, F(1), F(-1)))
    z = np.ascontiguousarray(z.reshape(C_, B, H, W).transpose(1, 0, 2, 3))
    return du, z


def fma32(a, b, c):
    """float32 ``fma(a, b, c)``, one rounding, on float32 arrays: the product of two float32 is exact in float64, TwoSum gives the
    rounding error of the float64 sum, and that error decides the one case in which rounding the float64 sum again would go wrong —
    the sum lying exactly half way between two float32 values.  (Results in the normal float32 range.)"""
    s = a.astype(np.float64) * b.astype(np.float64)
    c = np.broadcast_to(c.astype(np.float64), s.shape)
    t = s + c
    bb = t - s
    e = (s - (t - bb)) + (c - bb)
    half_way = (t.view(np.uint64) & np.uint64(0x1FFFFFFF)) == np.uint64(0x10000000)
    t = np.where(half_way & (e != 0), np.nextafter(t, np.where(e > 0, np.inf, -np.inf)), t)
    return t.astype(F)


def plan_stats(m, layer, channels):
    """The float64 mean and biased variance the model's plan normalised ``layer`` with in its last forward (rtod_plan_bn_batch_stats)."""
    import ctypes as C
    import torch
    from realtimeobjectdetection_amd import _ffi
    mean, var = np.zeros(channels, np.float64), np.zeros(channels, np.float64)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _ffi.check(_ffi.lib().rtod_plan_bn_batch_stats(m._plan, int(layer), mean.ctypes.data_as(C.c_void_p), var.ctypes.data_as(C.c_void_p), channels, stream))
    return mean, var


def normalise_model(z, mean, var, gamma, beta, leaky):
    """The forward's float expression on the raw sums ``z`` [B,C,H,W] (aux_kernels.hip bn_channel_constants / bn_normalise): w and b in
    double, rounded to float once each, u = fma(z, w, b), leaky: u > 0 ? u : u * 0.1f."""
    r = 1.0 / np.sqrt(np.asarray(var, np.float64) + EPS)
    w = (r * gamma.astype(np.float64)).astype(F)
    b = (beta.astype(np.float64) - np.asarray(mean, np.float64) * r * gamma.astype(np.float64)).astype(F)
    u = fma32(z, w.reshape(1, -1, 1, 1), b.reshape(1, -1, 1, 1))
    return np.where(u > 0, u, u * F(0.1)).astype(F) if leaky else u
