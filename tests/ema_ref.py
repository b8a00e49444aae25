"""The weight average's update (include/acgan_ema.h) restated on the host: float32 exactly as the kernels round it, and float64.

    k == 0:  shadow = p
    k  > 0:  d = min((double)decay, (1 + k) / (10 + k));  omd = (float)(1 - d)
             shadow = fsub(shadow, fmul(omd, fsub(shadow, p)))          three float32 roundings, no FMA
    counter: k + 1

The kernels' __fsub_rn / __fmul_rn round to nearest even like numpy's float32 arithmetic, with one difference the restatement
cannot express: what the hardware does with SUBNORMAL float32 intermediates depends on the kernel's denormal mode.  `update`
therefore reports where an intermediate (shadow - p, the product) is a non-zero subnormal, and asserts that there is none
unless the caller asks for the mask.
"""
import numpy as np

TINY = np.float32(2.0 ** -126)          # the smallest normal float32


def coefficient(k, decay):
    """-> (d as float64, omd as float32) for the counter value ``k`` > 0 and the float32 launch argument ``decay``."""
    d = min(np.float64(np.float32(decay)), (1.0 + np.float64(k)) / (10.0 + np.float64(k)))
    return d, np.float32(1.0 - d)


def update(shadow, p, k, decay, return_subnormal=False):
    """One update in float32: -> the new shadow (and, with ``return_subnormal``, the bool mask of elements with a non-zero
    subnormal intermediate; without it such an element is an AssertionError)."""
    shadow, p = np.asarray(shadow, np.float32), np.asarray(p, np.float32)
    if int(k) == 0:
        out, sub = p.copy(), np.zeros(p.shape, bool)
    else:
        _, omd = coefficient(k, decay)
        diff = shadow - p                       # float32 - float32 -> float32, round to nearest even
        prod = omd * diff
        assert diff.dtype == np.float32 and prod.dtype == np.float32
        sub = ((diff != 0) & (np.abs(diff) < TINY)) | ((prod != 0) & (np.abs(prod) < TINY))
        out = shadow - prod
    if return_subnormal:
        return out, sub
    assert not sub.any(), '%d elements with a subnormal intermediate' % int(sub.sum())
    return out


def update64(shadow, p, k, decay):
    """The same update in float64 (the coefficient still min(float32 decay, warm-up), 1 - d not rounded to float32)."""
    shadow, p = np.asarray(shadow, np.float64), np.asarray(p, np.float64)
    if int(k) == 0:
        return p.copy()
    d, _ = coefficient(k, decay)
    return shadow - (1.0 - d) * (shadow - p)


def fold(trajectory, decay, k0=0, shadow=None):
    """The float32 update folded over ``trajectory`` (the parameters after each update, in order), the counter starting at
    ``k0``: -> (shadow, bool mask of elements that met a subnormal intermediate in any step, final counter)."""
    sub_any = np.zeros(np.asarray(trajectory[0]).shape, bool)
    k = int(k0)
    for p in trajectory:
        shadow, sub = update(shadow if shadow is not None else np.zeros_like(p), p, k, decay, return_subnormal=True)
        sub_any |= sub
        k += 1
    return shadow, sub_any, k


def kernel_values(rng, n):
    """n float32 values of magnitude in [2^-10, 2^7] with random signs: what the kernel cases are fed."""
    mag = np.exp2(rng.uniform(-10.0, 7.0, size=n))
    return (mag * rng.choice([-1.0, 1.0], size=n)).astype(np.float32)
