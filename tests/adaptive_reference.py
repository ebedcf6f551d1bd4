"""The stopping rule of pt_render_adaptive (include/pt_api.h) restated in numpy, on per-sample radiance.  TEST INFRASTRUCTURE ONLY.

Nothing here touches a GPU or the device half of the package: the samples come from the CPU oracle (one frame per sample index),
the rule runs in fp64 in the order the header writes it, and z is the true quantile from mpmath — not the library's bisection.
`expected` brackets that z by 1e-12 relative (tests/test_adaptive_reference.py keeps the measurement that justifies the bracket)
and reports, per pixel, the sample count, the float32 interval err_map must lie in, and whether the bracket leaves the pixel's
count open ("undecided": the cases the GPU tests use are chosen so that no pixel is)."""
import collections

import mpmath
import numpy as np

Z_BRACKET = 1e-12


def quantile(p_value):
    """z = Phi^-1(1 - p/2) = sqrt(2) erfinv(1 - p) for the p the library sees: 0 means the double 0.05, anything else is a float
    field of pt_adaptive_params, widened to double.  50 digits, rounded to double."""
    p = 0.05 if p_value == 0 else float(np.float32(p_value))
    with mpmath.workdps(50):
        return float(mpmath.sqrt(2) * mpmath.erfinv(1 - mpmath.mpf(p)))


def defaults(spp, batch, max_spp):
    """The header's defaults: batch_spp 0 -> spp, max_spp 0 -> 32 * spp."""
    return int(batch) if batch > 0 else int(spp), int(max_spp) if max_spp > 0 else 32 * int(spp)


def checkpoints(spp, batch, max_spp):
    """n = spp, spp + batch, spp + 2 batch, ..., the last one cut to max_spp."""
    batch, max_spp = defaults(spp, batch, max_spp)
    c = [int(spp)]
    while c[-1] < max_spp:
        c.append(min(c[-1] + batch, max_spp))
    return c


def samples(oracle, d, p, max_spp, stride):
    """[rows * W, max_spp, 3] float32: sample k of every selected pixel, as the oracle's frame at spp = 1, sample_offset = k and
    stream_stride = stride gives it.  Row selection, flags and everything else are p's."""
    out = np.zeros((p.num_rows() * p.width, max_spp, 3), np.float32)
    for k in range(max_spp):
        q = p.copy()
        q.spp, q.sample_offset, q.stream_stride = 1, k, int(stride)
        img, _ = oracle.render(d, q)
        out[:, k] = img.reshape(-1, 3)
    return out


def luminance(samples):
    """Y = 0.2126 R + 0.7152 G + 0.0722 B in fp64, left to right (numpy never contracts)."""
    d = np.asarray(samples, dtype=np.float32).astype(np.float64)
    return 0.2126 * d[..., 0] + 0.7152 * d[..., 1] + 0.0722 * d[..., 2]


def rule_luminance(Y, spp, batch, max_spp, max_error, min_luminance, z):
    """The header rule on per-sample luminance Y [P, >= max_spp] fp64, step for step at every checkpoint:
    (n [P] int64, err at n [P] fp64)."""
    batch, max_spp = defaults(spp, batch, max_spp)
    max_error = float(np.float32(max_error))               # floats in the struct
    min_luminance = float(np.float32(min_luminance))
    Y = np.asarray(Y, dtype=np.float64)
    P = Y.shape[0]
    assert Y.shape[1] >= max_spp
    n_stop = np.zeros(P, np.int64)
    e_stop = np.zeros(P)
    done = np.zeros(P, bool)
    s1, s2 = np.zeros(P), np.zeros(P)
    k = 0
    for n in checkpoints(spp, batch, max_spp):
        while k < n:                                        # sample by sample, in sample order
            s1 = s1 + Y[:, k]
            s2 = s2 + Y[:, k] * Y[:, k]
            k += 1
        nn = float(n)
        with np.errstate(all="ignore"):
            if n > 1:
                v = (s2 - s1 * s1 / nn) / (nn - 1.0)
                var = np.where(v < 0.0, 0.0, v)             # max(0, .)
            else:
                var = np.full(P, np.inf)
            half = z * np.sqrt(var / nn)
            mean = s1 / nn
            den = np.where(mean < min_luminance, min_luminance, mean)
            err = np.where(half == 0.0, 0.0, half / den)
        stop = ~done & ((err <= max_error) | (n == max_spp))
        n_stop[stop], e_stop[stop] = n, err[stop]
        done |= stop
    assert done.all()
    return n_stop, e_stop


def mean_image(samples, n):
    """fb: the fp32 sum of the first n[P] samples in sample order, ((0 + s0) + s1) + ..., times 1.0f / (float)n."""
    s = np.asarray(samples, dtype=np.float32)
    fb = np.zeros((s.shape[0], 3), np.float32)
    fsum = np.zeros((s.shape[0], 3), np.float32)
    for k in range(int(n.max())):
        fsum = fsum + s[:, k]
        stop = n == k + 1
        fb[stop] = (fsum * (np.float32(1.0) / np.float32(k + 1)))[stop]
    return fb


def rule(samples, spp, batch, max_spp, max_error, min_luminance, z):
    """The header rule on per-sample radiance [P, >= max_spp, 3] float32: (n [P] int64, err at n [P] fp64, fb [P, 3] float32)."""
    n, err = rule_luminance(luminance(samples), spp, batch, max_spp, max_error, min_luminance, z)
    return n, err, mean_image(samples, n)


def plan_passes(spp, batch, max_spp, list_sizes, scratch_bytes):
    """Launches of the trace kernel under an explicit "scratch_bytes" (info "passes"): every round splits its samples so that one
    pass's float4 per (listed pixel, sample) fits the budget, at most 2^30 of them, at least one sample."""
    cps = checkpoints(spp, batch, max_spp)
    total = 0
    for r, n_list in enumerate(list_sizes):
        spp_r = cps[r] - (cps[r - 1] if r else 0)
        spp_pass = min(spp_r, max(1, min(int(scratch_bytes) // (16 * n_list), 2 ** 30 // n_list)))
        total += -(-spp_r // spp_pass)
    return total


Expected = collections.namedtuple("Expected", "n err_lo err_hi decided fb rounds list_sizes passes err")


def expected(samples, spp, batch, max_spp, max_error, min_luminance, p_value, scratch_bytes=None):
    """What pt_render_adaptive must give for these samples, per packed pixel:
      n                sample count (at the true z)
      err_lo, err_hi   float32: err_map lies in [err_lo, err_hi] (err is monotone in z; both ends at the bracket's n)
      decided          the three z of the bracket agree on n
      fb               float32 [P, 3]
      rounds           1 + index of max(n) among the checkpoints
      list_sizes       pixels entering round 0, 1, ... (rounds entries)
      passes           info "passes" under the explicit scratch_bytes (None where none was given)
      err              fp64 err at n, at the true z"""
    z = quantile(p_value)
    args = (samples, spp, batch, max_spp, max_error, min_luminance)
    n_lo, e_lo, _ = rule(*args, z * (1.0 - Z_BRACKET))
    n, e, fb = rule(*args, z)
    n_hi, e_hi, _ = rule(*args, z * (1.0 + Z_BRACKET))
    decided = (n_lo == n) & (n_hi == n)
    cps = checkpoints(spp, batch, max_spp)
    rounds = 1 + cps.index(int(n.max()))
    list_sizes = [int(n.shape[0])] + [int((n > cps[r - 1]).sum()) for r in range(1, rounds)]
    passes = None if scratch_bytes is None else plan_passes(spp, batch, max_spp, list_sizes, scratch_bytes)
    with np.errstate(over="ignore"):
        lo, hi = e_lo.astype(np.float32), e_hi.astype(np.float32)
    return Expected(n, lo, hi, decided, fb, rounds, list_sizes, passes, e)


def threshold_for(err0, k):
    """A float32 max_error strictly between the k-th and the (k+1)-th largest of the first-checkpoint errors err0 (fp64), so that
    exactly k pixels continue after round 0; None where those two ranks tie or no float32 separates them by more than the z
    bracket."""
    e = np.sort(np.asarray(err0, dtype=np.float64))[::-1]
    below = e[k] if k < e.size else 0.0
    if k == 0:
        t = np.float32(2.0 * e[0]) if e[0] > 0 else np.float32(1.0)
    else:
        t = np.float32(0.5 * (e[k - 1] + below))
        if not float(t) * (1.0 + 1e-9) < e[k - 1]:
            return None
    if not np.isfinite(t) or not t > 0 or not below * (1.0 + 1e-9) < float(t):
        return None
    return t
