"""qkv / qkv2 -- drop-in for det2trt/models/functions/multi_head_attn.py:29-54 (the QKVTRT / QKVTRT2 plugins):
out[b, i, :] = softmax_j(<q[b, i], k[b, j]> / sqrt(E)) v[b, j] on the matrix cores (csrc/qkv.hip, reached through
`bevops_qkv_forward`): one launch, two when few query tiles meet many keys and the keys are split across blocks."""
import torch

from ..utils import lib as _lib
from ..utils import workspace as _ws


def _dense(t):
    """Contiguous and 16-byte aligned, as the C ABI wants its tensors."""
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


def _qkv(query, key, value):
    assert query.is_cuda and key.is_cuda and value.is_cuda, "qkv: tensors must be on the GPU"
    if query.ndim != 3 or key.ndim != 3 or value.ndim != 3:
        raise ValueError("qkv: query, key and value must be 3-D [batch, len, embed_dim]")
    if key.shape != value.shape or key.shape[0] != query.shape[0] or key.shape[2] != query.shape[2]:
        raise ValueError(f"qkv: shapes {tuple(query.shape)}, {tuple(key.shape)}, {tuple(value.shape)} do not match")
    if key.dtype != query.dtype or value.dtype != query.dtype:
        raise TypeError(f"qkv: dtypes {query.dtype}, {key.dtype}, {value.dtype} differ")
    if key.device != query.device or value.device != query.device:
        raise ValueError("qkv: tensors are on different devices")
    B, Lq, E = query.shape
    Lkv = key.shape[1]
    dt = _lib.torch_dtype_code(query)
    out = torch.empty((B, Lq, E), dtype=query.dtype, device=query.device)
    if B == 0 or Lq == 0:
        return out
    if Lkv == 0:
        raise ValueError("qkv: no keys (a softmax over an empty set)")
    handle = _lib.load_library()
    q, k, v = _dense(query), _dense(key), _dense(value)
    stream = _lib.current_stream_ptr(query.device)
    nws = handle.bevops_qkv_workspace_size(dt, B, Lq, Lkv, E)
    ws = _ws.lend("qkv", nws, query.device, stream) if nws else None
    with torch.cuda.device(query.device):
        st = handle.bevops_qkv_forward(dt, q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), B, Lq, Lkv, E,
                                       1.0, 1.0, 1.0, 1.0, ws.data_ptr() if ws is not None else None, nws, stream)
    _lib.check(st, "bevops_qkv_forward")
    return out


def qkv(query, key, value):
    """
    Args:
        query: [batch_size, q_len, embed_dim]
        key: [batch_size, kv_len, embed_dim]
        value: [batch_size, kv_len, embed_dim]

    Returns: [batch_size, q_len, embed_dim] = softmax(query key^T / sqrt(embed_dim)) value, in the inputs' dtype.
    fp32 or fp16; embed_dim % 16 == 0 and 16 <= embed_dim <= 128 (else BevopsError NOT_SUPPORTED, as for int8)."""
    return _qkv(query, key, value)


def qkv2(query, key, value):
    """Same op under the reference's half2 plugin name QKVTRT2 (functions/multi_head_attn.py:43)."""
    return _qkv(query, key, value)
