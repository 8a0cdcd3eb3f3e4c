"""NumPy restatement of the field-statistics kernel (blitzdg_amd/csrc/hip/sw2d_stats_kernel.hpp), bit for bit: every step is one
rounded float64 operation, in the kernel's order. Per sample and entry
    eta = h - H (h without H),  u = hu / h,  v = hv / h
    sum[f] = sum[f] + f                                         f = eta, u, v
    etaMax = fmax(etaMax, eta), hMin = fmin(hMin, h), speedMax = fmax(speedMax, sqrt(u u + v v))     (fmax / fmin skip NaNs)
    cos[j][f] = cos[j][f] + f c_j,  sin[j][f] = sin[j][f] + f s_j
with c_j, s_j taken from the sample log (the values the library passed to its kernel), not recomputed. Nothing depends on the
order of the elements, so the arrays are in the caller's numbering.

Also the synthetic accumulators of tests/test_fieldstats_fit.py, which need no device."""
import numpy as np


def accumulate(states, H, trig, mean=True, envelope=True):
    """The accumulators after the samples `states` (a list of (h, hu, hv[, hN]), each (Np, K)) with the depth `H` ((Np, K) or
    None) and the sample log `trig` ((n, 2 m): c_1, s_1, .. per sample): a dict with the keys of RunRecords.fieldStats that hold
    accumulators (`sum`, `etaMax`, `hMin`, `speedMax`, `cos`, `sin`), those of a group that is off left out."""
    trig = np.asarray(trig, dtype=np.float64).reshape(len(states), -1)
    m = trig.shape[1] // 2
    shape = np.asarray(states[0][0]).shape
    total = np.zeros((3,) + shape)
    eta_max, h_min, speed_max = np.full(shape, -np.inf), np.full(shape, np.inf), np.zeros(shape)
    cos, sin = np.zeros((m, 3) + shape), np.zeros((m, 3) + shape)
    with np.errstate(all="ignore"):
        for q, row in zip(states, trig):
            h, hu, hv = (np.asarray(a, dtype=np.float64) for a in q[:3])
            f = (h - H if H is not None else h.copy(), hu / h, hv / h)
            for c in range(3):
                total[c] = total[c] + f[c]
            eta_max = np.fmax(eta_max, f[0])
            h_min = np.fmin(h_min, h)
            speed_max = np.fmax(speed_max, np.sqrt(f[1] * f[1] + f[2] * f[2]))
            for j in range(m):
                for c in range(3):
                    cos[j, c] = cos[j, c] + f[c] * row[2 * j]
                    sin[j, c] = sin[j, c] + f[c] * row[2 * j + 1]
    out = {}
    if mean:
        out["sum"] = total
    if envelope:
        out.update(etaMax=eta_max, hMin=h_min, speedMax=speed_max)
    if m:
        out.update(cos=cos, sin=sin)
    return out


def trig_log(t, periods):
    """(n, 2 m): cos and sin of (2 pi / T_j) t per period, the row layout of the library's sample log."""
    t = np.asarray(t, dtype=np.float64)
    out = np.empty((t.size, 2 * len(periods)))
    for j, T in enumerate(periods):
        om = 2.0 * np.pi / T
        out[:, 2 * j], out[:, 2 * j + 1] = np.cos(om * t), np.sin(om * t)
    return out


def same(a, b):
    """Bit-for-bit equality of two arrays, NaNs compared by position."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


def synthetic(periods, span, seed, shape=(2, 5, 50), step=(210.0, 300.0), amplitude=(0.1, 3.0)):
    """prod(shape) signals a0 + sum_j A_j cos(omega_j t - phi_j) sampled over [0, span] at irregular steps drawn from `step`, as
    the dict `stats` of RunRecords.fieldStats with accumulators of `shape`, and the truth: (stats, a0, A, phi) with a0 of `shape`
    and A, phi of (m,) + shape."""
    rng = np.random.default_rng(seed)
    t = [0.0]
    while t[-1] < span:
        t.append(t[-1] + rng.uniform(*step))
    t = np.array(t[:-1])
    m = len(periods)
    a0 = rng.uniform(-2.0, 2.0, shape)
    A = rng.uniform(amplitude[0], amplitude[1], (m,) + shape)
    phi = rng.uniform(-np.pi, np.pi, (m,) + shape)
    trig = trig_log(t, periods)
    total, cos, sin = np.zeros(shape), np.zeros((m,) + shape), np.zeros((m,) + shape)
    for i, ti in enumerate(t):
        f = a0.copy()
        for j, T in enumerate(periods):
            f = f + A[j] * np.cos(2.0 * np.pi / T * ti - phi[j])
        total = total + f
        for j in range(m):
            cos[j] = cos[j] + f * trig[i, 2 * j]
            sin[j] = sin[j] + f * trig[i, 2 * j + 1]
    stats = {"n": t.size, "t": t, "trig": trig, "sum": total}
    if m:
        stats.update(cos=cos, sin=sin)
    return stats, a0, A, phi
