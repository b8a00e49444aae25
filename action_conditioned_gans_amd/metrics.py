"""Frame-quality metrics on the GPU: per-frame SSIM and squared error (include/acgan_metrics.h, csrc/metrics.hip).

The reference publishes quality curves only - SSIM and PSNR per rollout step for the DNA generator and an identity baseline
(report Fig. 4).  SSIM here is tf.image.ssim's definition (equally skimage's with ``gaussian_weights=True,
use_sample_covariance=False``): 11x11 Gaussian window, sigma 1.5, normalised to sum 1; VALID filtering ((H-10) x (W-10)
positions); population moments; C1 = (0.01 L)^2, C2 = (0.03 L)^2 with L = ``data_range`` (2.0 for the project's [-1, 1]
frames); the per-frame value is the mean of the map over positions, then channels.  There is no host fallback: a library
without the entry point raises.
"""
import ctypes

import numpy as np
import torch

from . import _lib

DATA_RANGE = 2.0          # the project's frames lie in [-1, 1]
K1, K2 = 0.01, 0.03
SSIM_DEFINITION = ('tf.image.ssim: 11x11 Gaussian window (sigma 1.5, sum 1), VALID positions, population moments, '
                   'C1=(0.01 L)^2, C2=(0.03 L)^2, L=data_range; mean over positions, then channels')


def _stream_handle(stream, device):
    if stream is None:
        return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    if isinstance(stream, torch.cuda.Stream):
        return ctypes.c_void_p(stream.cuda_stream)
    if isinstance(stream, ctypes.c_void_p):
        return stream
    return ctypes.c_void_p(int(stream))


def frame_metrics(pred, truth, data_range=DATA_RANGE, stream=None, channels=None, lib=None):
    """Per-frame (SSIM, sum of squared errors) of device tensors ``pred`` / ``truth`` ``[..., H, W, C]`` (float32 or bfloat16,
    each on its own) -> two float32 device tensors of the leading shape.  ``channels``: the channels to score when the last
    axis is a wider channel pitch (the zero-padded pitch-4 copies of the frames); default all of them.  ``stream``: the
    stream to run on (a ``torch.cuda.Stream``, a raw ``hipStream_t`` or the session's ``rt.stream_ptr()``); default the
    current torch stream.  One partial pass and one per-frame sum, no float atomics: bit-identical across launches."""
    lib = lib or _lib.get()
    run, size = _lib.entry(lib, 'frame_metrics'), _lib.entry(lib, 'frame_metrics_workspace_bytes')
    if not (torch.is_tensor(pred) and torch.is_tensor(truth)):
        raise TypeError('frame_metrics takes device tensors')
    if pred.shape != truth.shape or pred.dim() < 3:
        raise ValueError('frame_metrics: pred %s and truth %s must have one shape [..., H, W, C]' % (tuple(pred.shape), tuple(truth.shape)))
    if pred.device != truth.device or pred.device.type != 'cuda':
        raise ValueError('frame_metrics: both tensors must be on one GPU (got %s, %s)' % (pred.device, truth.device))
    *lead, h, w, pitch = pred.shape
    c = pitch if channels is None else int(channels)
    n = int(np.prod(lead)) if lead else 1
    dtype = _lib.dtype2(_lib.code(pred.dtype), _lib.code(truth.dtype))
    pred, truth = pred.contiguous(), truth.contiguous()
    ssim = torch.empty(n, dtype=torch.float32, device=pred.device)
    sqerr = torch.empty(n, dtype=torch.float32, device=pred.device)
    if n == 0:
        return ssim.view(lead), sqerr.view(lead)
    ws_bytes = size(n, h, w)
    ws = torch.empty(max(int(ws_bytes), 16), dtype=torch.uint8, device=pred.device)
    run(ctypes.c_void_p(pred.data_ptr()), ctypes.c_void_p(truth.data_ptr()), ctypes.c_void_p(ssim.data_ptr()),
        ctypes.c_void_p(sqerr.data_ptr()), n, h, w, c, pitch, dtype, float(data_range), K1, K2,
        ctypes.c_void_p(ws.data_ptr()), ws.numel(), _stream_handle(stream, pred.device))
    return ssim.view(lead), sqerr.view(lead)


def psnr_from_sqerr(sqerr_sum, count):
    """PSNR by the reference's formula, ``10 log10(1 / MSE)`` with MSE = ``sqerr_sum / count`` (``build_psnr``, ops.py:19-20).
    The reference applies it to frames in [-1, 1] without rescaling, so it reads 20 log10(2) ~ 6.02 dB BELOW the PSNR of the
    same frames mapped to [0, 1].  Works elementwise on arrays."""
    mse = np.maximum(np.asarray(sqerr_sum, dtype=np.float64) / float(count), 1e-30)
    return 10.0 * np.log10(1.0 / mse)
