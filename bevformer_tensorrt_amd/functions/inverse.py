"""inverse -- drop-in for det2trt/models/functions/inverse.py:23 (the InverseTRT plugin; torch.linalg.inv in the
reference's eager path) on csrc/inverse.hip through `bevops_inverse_forward`."""
import torch

from ..utils import lib as _lib


def inverse(inputs):
    """inputs [..., n, n] fp32 on the GPU, 1 <= n <= 32 -> the inverse of every matrix, same shape and dtype.
    Partial pivoting.  A matrix with an exactly zero pivot comes back all NaN (torch.linalg.inv raises instead; the
    plugin cannot report a failure per matrix); its neighbours in the batch are unaffected.  fp16 / int8 / n > 32
    raise BevopsError (NOT_SUPPORTED)."""
    assert inputs.is_cuda, "inverse: inputs must be on the GPU"
    if inputs.ndim < 2 or inputs.shape[-1] != inputs.shape[-2]:
        raise ValueError(f"inverse: expected [..., n, n], got {tuple(inputs.shape)}")
    n = inputs.shape[-1]
    dt = _lib.torch_dtype_code(inputs)
    out = torch.empty(inputs.shape, dtype=inputs.dtype, device=inputs.device)
    if out.numel() == 0:
        return out
    x = inputs.reshape(-1, n, n).contiguous()
    if x.data_ptr() % 16:
        x = x.clone()
    handle = _lib.load_library()
    with torch.cuda.device(inputs.device):
        st = handle.bevops_inverse_forward(dt, x.data_ptr(), out.data_ptr(), x.shape[0], n,
                                           _lib.current_stream_ptr(inputs.device))
    _lib.check(st, "bevops_inverse_forward")
    return out
