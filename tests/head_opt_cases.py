"""What tests/golden/make_golden_adam.py, tests/test_head_opt_host.py and tests/test_head_opt_gpu.py share: the inputs of the Adam
fixture regenerated from their seeds, torch's own ``optim.Adam`` on the CPU, a float64 restatement of it in numpy, the error
scales of the gate, and the adversarial head weights of the pack test.

The gate (tests/golden/adam_step.npz).  With u = 2^-24 and per element
    D_w = u (|w'| + |w' - w|)          the result and the step it took
    D_m = u (beta1 |m| + (1 - beta1) |g|)
    D_v = u v'
an implementation's w', m', v' are compared with float64 ``torch.optim.Adam`` as max and rms of |value - float64| / D over the elements
with D > 0; elements with D = 0 must be exact.  The fixture records, per case, what float32 ``torch.optim.Adam`` on the CPU gives in
those units (the float32 floor); the gate is 4 x that floor, the project's convention for a different but equally legitimate
arrangement of the same handful of roundings.

A committed file holds at most 1 MiB, and the float64 results of four 255 x 512 cases are 12 MiB.  So the fixture stores torch's
float64 result for the rows ``STORED_ROWS`` only, and the floors, which the generator measured over the whole arrays; the tests
recompute the float64 result everywhere with ``adam_ref64`` (numpy, float64, the textbook formula) and hold it to the stored rows
to 1e-12 of D / u — a millionth of the gate's unit — before they use it."""
import zlib

import numpy as np

F = np.float32
U = 2.0 ** -24
SHAPE = (255, 512)
STEPS = (1, 2, 10, 1000)
LR, BETAS, EPS = 1e-2, (0.9, 0.999), 1e-8         # the reference's optim.Adam(lr=1e-2), torch's defaults for the rest
SEED0 = 4211
ZERO_ROW = 17                                     # the channel with g = 0 and v = 0
STORED_ROWS = (0, 1, ZERO_ROW, 128, 254)


def adam_inputs(seed, t):
    """(w, g, m, v) float32 [255, 512]: w ~ 0.05 N(0, 1); g, m and sqrt(v) scaled per channel by 10^U(-6, 2); m = v = 0 at t = 1;
    row ZERO_ROW has g = 0 and v = 0."""
    rng = np.random.RandomState(seed)
    w = (0.05 * rng.standard_normal(SHAPE)).astype(F)
    s = (10.0 ** rng.uniform(-6.0, 2.0, (SHAPE[0], 1)))
    g = (s * rng.standard_normal(SHAPE)).astype(F)
    m = (s * rng.standard_normal(SHAPE)).astype(F)
    r = (s * np.abs(rng.standard_normal(SHAPE))).astype(F)
    v = (r.astype(np.float64) ** 2).astype(F)
    if t == 1:
        m[:] = 0
        v[:] = 0
    g[ZERO_ROW] = 0
    v[ZERO_ROW] = 0
    return w, g, m, v


def inputs_crc(arrays):
    return zlib.crc32(b"".join(np.ascontiguousarray(a).tobytes() for a in arrays))


def torch_adam(w, g, m, v, t, dtype, lr=LR, betas=BETAS, eps=EPS):
    """One ``torch.optim.Adam`` step (the reference's construction: no weight decay, no amsgrad) on the CPU in ``dtype`` from the
    float32 state after t - 1 steps.  Returns (w', m', v') as numpy arrays of that dtype."""
    import torch
    p = torch.nn.Parameter(torch.from_numpy(np.array(w)).to(dtype))
    p.grad = torch.from_numpy(np.array(g)).to(dtype)
    opt = torch.optim.Adam([p], lr=lr, betas=betas, eps=eps)
    opt.state[p] = {"step": torch.tensor(float(t - 1)), "exp_avg": torch.from_numpy(np.array(m)).to(dtype), "exp_avg_sq": torch.from_numpy(np.array(v)).to(dtype)}
    opt.step()
    st = opt.state[p]
    assert int(st["step"]) == t
    return p.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()


def adam_ref64(w, g, m, v, t, lr=LR, betas=BETAS, eps=EPS):
    """The same step in numpy float64, from the formulas: what the tests compare with (held to the fixture's stored rows first)."""
    w, g, m, v = (np.asarray(a, np.float64) for a in (w, g, m, v))
    b1, b2 = betas
    m1 = m + (g - m) * (1 - b1)
    v1 = b2 * v + (1 - b2) * g * g
    w1 = w - (lr / (1 - b1 ** t)) * m1 / (np.sqrt(v1) / np.sqrt(1 - b2 ** t) + eps)
    return w1, m1, v1


def scales(w, g, m, ref, betas=BETAS):
    """(D_w, D_m, D_v) of the module docstring from the float32 inputs and the float64 result ``ref`` = (w', m', v')."""
    w, g, m = (np.asarray(a, np.float64) for a in (w, g, m))
    return U * (np.abs(ref[0]) + np.abs(ref[0] - w)), U * (betas[0] * np.abs(m) + (1 - betas[0]) * np.abs(g)), U * ref[2]


def errors(value, ref, d):
    """(max, rms) of |value - ref| / d over d > 0, and whether every element with d == 0 is exact."""
    e = np.abs(np.asarray(value, np.float64) - ref)
    sel = d > 0
    q = e[sel] / d[sel]
    return float(q.max()), float(np.sqrt(np.mean(q * q))), bool((e[~sel] == 0).all())


def load_adam_cases(golden_dir):
    import os
    z = np.load(os.path.join(golden_dir, "adam_step.npz"))
    assert tuple(z["steps"].tolist()) == STEPS and tuple(z["stored_rows"].tolist()) == STORED_ROWS
    cases = []
    for idx, t in enumerate(STEPS):
        k = "c%d_" % idx
        seed = int(z[k + "seed"])
        inp = adam_inputs(seed, t)
        assert inputs_crc(inp) == int(z[k + "crc"]), t
        ref = adam_ref64(*inp, t)
        d = scales(inp[0], inp[1], inp[2], ref)
        rows = list(STORED_ROWS)
        for name, r, dd in zip(("w64", "m64", "v64"), ref, d):                # the recomputed float64 result is the recorded one
            gap = np.abs(r[rows] - z[k + name])
            assert (gap <= 1e-12 * dd[rows] / U).all(), (t, name, float(gap.max()))
        cases.append({"t": t, "seed": seed, "inputs": inp, "ref": ref, "d": d,
                      "floor": {n: (float(z[k + "floor_" + n][0]), float(z[k + "floor_" + n][1])) for n in ("w", "m", "v")}})
    return cases


# ---------------------------------------------------------------------------------------------- adversarial head weights (pack test)
def adversarial_head(cout, cin, seed):
    """Float32 (weight [cout, cin], bias [cout]) whose channels walk the corners of the split packing: an all-zero channel, a maximum
    that is exactly a power of two, one weight of 2^10 over a tail from 2^-30 to 2^-10 of it (low parts that are subnormal halves,
    some vanish), a maximum of 2^-45 (the pre-scale exponent clamps at 40), a maximum of 2^30, negative zeros; random elsewhere."""
    rng = np.random.RandomState(seed)
    w = (0.05 * rng.standard_normal((cout, cin))).astype(F)
    b = rng.standard_normal(cout).astype(F)
    w[0] = 0
    w[1] = np.clip(w[1], -0.2, 0.2)
    w[1, 5] = F(0.25)
    w[2] = (F(1024.0) * 2.0 ** rng.uniform(-30, -10, cin) * rng.choice([-1.0, 1.0], cin)).astype(F)
    w[2, 3] = F(1024.0)
    w[3] = (2.0 ** -45 * rng.uniform(-1, 1, cin)).astype(F)
    w[3, 7] = F(2.0 ** -45)
    w[4] = (2.0 ** 30 * rng.uniform(-1, 1, cin)).astype(F)
    w[4, 0] = F(-(2.0 ** 30))
    w[5, ::3] = F(-0.0)
    w[6] = F(-0.0)
    w[7, :8] = F(2.0 ** -20) * (1 + 2.0 ** -11 * np.arange(8)).astype(F)        # halfway cases of the f16 rounding after the pre-scale
    b[3] = F(-0.0)
    return w, b
