"""PTQ calibration state on the device (csrc/calibrate.hip, include/bevops.h "PTQ calibration on the device"): a running
2048-bin histogram of |x| per site, collected without a host synchronisation, and the threshold searches over it.
Not a reference plugin: the reference hands calibration to TensorRT (det2trt/quantization/calibrator_trt.py:6-92)."""
import torch

from ..utils import lib as _lib
from ..utils import workspace as _ws

METHODS = {"entropy": 0, "percentile": 1}


def calib_state_size():
    """Bytes of one calibration state (64-byte header + uint64 hist[2048]); states are 64-byte aligned and a
    zero-filled one is empty."""
    return int(_lib.load_library().bevops_calib_state_size())


def _device_tensor(t, what):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise TypeError(f"{what}: expected a CUDA tensor")
    return t


def calib_collect(x, state):
    """One batch into `state` (a uint8 device tensor of at least calib_state_size() bytes at a 64-byte aligned address):
    three launches on the current stream, no host read, capturable.  x: fp16 or fp32, any shape; a non-contiguous x is
    made contiguous, an empty one is ignored."""
    _device_tensor(x, "calib_collect x")
    _device_tensor(state, "calib_collect state")
    if state.dtype != torch.uint8 or not state.is_contiguous() or state.numel() < calib_state_size():
        raise ValueError("calib_collect: state must be a contiguous uint8 tensor of calib_state_size() bytes")
    if x.dtype not in (torch.float16, torch.float32):
        raise TypeError(f"calib_collect: unsupported dtype {x.dtype}; expected float16 or float32")
    if x.numel() == 0:
        return
    x = x.detach()
    # a histogram does not depend on the order of the elements: channels-last memory is read as it lies
    if not (x.is_contiguous() or (x.dim() == 4 and x.is_contiguous(memory_format=torch.channels_last))):
        x = x.contiguous()
    handle = _lib.load_library()
    with torch.cuda.device(x.device):
        st = handle.bevops_calib_collect(_lib.torch_dtype_code(x), x.data_ptr(), x.numel(), state.data_ptr(),
                                         _lib.current_stream_ptr(x.device))
    _lib.check(st, "bevops_calib_collect")


def calib_threshold(states, method="entropy", percentile=99.99):
    """Clip bins of `states` (uint8 [S, stride] on the device, stride >= calib_state_size() and a multiple of 64, rows
    contiguous) -> (bins int32 [S], kl float64 [S]) on the device: one search over all states, no host read.  bins is
    -1 for a state without data; kl is the minimum of the entropy curve (0 for the percentile rule)."""
    _device_tensor(states, "calib_threshold states")
    if method not in METHODS:
        raise ValueError(f"calib_threshold: method should be in {sorted(METHODS)}")
    if states.dtype != torch.uint8 or states.dim() != 2 or states.stride(1) != 1 or states.shape[0] == 0:
        raise ValueError("calib_threshold: states must be a uint8 [S, stride] tensor with contiguous rows, S >= 1")
    n = int(states.shape[0])
    dev = states.device
    bins = torch.empty(n, dtype=torch.int32, device=dev)
    kl = torch.empty(n, dtype=torch.float64, device=dev)
    handle = _lib.load_library()
    stream = _lib.current_stream_ptr(dev)
    need = int(handle.bevops_calib_threshold_workspace_size(n))
    scratch = _ws.lend("calib_threshold", need, dev, stream)
    with torch.cuda.device(dev):
        st = handle.bevops_calib_threshold(METHODS[method], float(percentile), states.data_ptr(), n, int(states.stride(0)),
                                           bins.data_ptr(), kl.data_ptr(), scratch.data_ptr(), scratch.numel(), stream)
    _lib.check(st, "bevops_calib_threshold")
    return bins, kl
