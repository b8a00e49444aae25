"""Float64 restatement of the SSIM the GPU kernel computes (include/acgan_metrics.h), for the tests: tf.image.ssim's
definition - 11x11 Gaussian window (sigma 1.5, sum 1), VALID positions, population moments, C1 = (k1 L)^2, C2 = (k2 L)^2,
mean of the map over positions and then channels.  Written from the definition, the direct way (no shifts, no Var(x - y)
rewrite), so that it checks the kernel's arithmetic rather than repeating it."""
import numpy as np

TAPS, SIGMA = 11, 1.5


def window_1d():
    t = np.arange(TAPS, dtype=np.float64) - (TAPS - 1) / 2
    g = np.exp(-t * t / (2 * SIGMA * SIGMA))
    return g / g.sum()


def window_2d():
    g = window_1d()
    return np.outer(g, g)


def _filter_valid(a):
    """[..., H, W, C] float64 -> [..., H-10, W-10, C]: the separable 11x11 Gaussian, VALID."""
    g = window_1d()
    h, w = a.shape[-3], a.shape[-2]
    rows = sum(g[k] * a[..., k:h - TAPS + 1 + k, :, :] for k in range(TAPS))
    return sum(g[k] * rows[..., :, k:w - TAPS + 1 + k, :] for k in range(TAPS))


def ssim_map(x, y, data_range=2.0, k1=0.01, k2=0.03):
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    if x.shape[-3] < TAPS or x.shape[-2] < TAPS:
        raise ValueError('frames smaller than the 11x11 window')
    c1, c2 = (k1 * data_range) ** 2, (k2 * data_range) ** 2
    mx, my = _filter_valid(x), _filter_valid(y)
    vx = _filter_valid(x * x) - mx * mx
    vy = _filter_valid(y * y) - my * my
    cxy = _filter_valid(x * y) - mx * my
    return ((2 * mx * my + c1) * (2 * cxy + c2)) / ((mx * mx + my * my + c1) * (vx + vy + c2))


def ssim(x, y, data_range=2.0, k1=0.01, k2=0.03):
    """Per-frame SSIM of [..., H, W, C] frames -> [...]."""
    return ssim_map(x, y, data_range, k1, k2).mean(axis=(-3, -2, -1))


def sqerr(x, y):
    """Per-frame sum of squared differences -> [...]."""
    d = np.asarray(x, np.float64) - np.asarray(y, np.float64)
    return (d * d).sum(axis=(-3, -2, -1))
