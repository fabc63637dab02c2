"""FlashOcc's occupancy predictor (BEVOCCHead2D behind final_conv: Linear(C, Hd) + Softplus + Linear(Hd, Dz Ncls), then the
arg-max over the classes of every voxel) as ONE launch of bevops_occ_head_f16 (csrc/occ_head.hip, design/flashocc.md): the
hidden tensor stays in registers, the logits are reduced in registers, a pixel leaves as Dz class bytes.  Not a reference
plugin (the reference tree has no FlashOcc code)."""
from collections import namedtuple

import torch
import torch.nn.functional as F

from ..utils import lib as _lib
from .linear import _call, _ptr
from .multi_scale_deformable_attn import _TensorCache

OccHeadPacked = namedtuple("OccHeadPacked", "w1 b1 w2 b2 C Hd Dz Ncls nb")
_PACKED = _TensorCache()   # W2 -> (stamps of the other three, OccHeadPacked)


def occ_head_blocks(Dz, Ncls):
    """32-column blocks of the packed second layer (bevops_occ_head_blocks): a lane half walks ceil(Dz / 2) voxels of Ncls
    slots, 16 slots a block; 0 outside 1 <= Dz <= 16, 1 <= Ncls <= 32, Dz Ncls <= 320."""
    if not (1 <= Dz <= 16 and 1 <= Ncls <= 32 and Dz * Ncls <= 320):
        return 0
    return ((Dz + 1) // 2 * Ncls + 15) // 16


def occ_head_column_map(Dz, Ncls):
    """int64 [32 nb]: the logit column z Ncls + cls that physical row P of the packed W2 holds, -1 for a row of padding.
    P = 32 i + 8 g + 4 hb + c is slot t = 16 i + 4 g + c of lane half hb: voxel z = 2 (t // Ncls) + hb, class t % Ncls."""
    P = torch.arange(32 * occ_head_blocks(Dz, Ncls))
    t, hb = 16 * (P // 32) + 4 * (P % 32 // 8) + P % 4, P % 8 // 4
    z = 2 * (t // Ncls) + hb
    return torch.where(z < Dz, z * Ncls + t % Ncls, torch.full_like(P, -1))


def occ_head_k_map():
    """int64 [64]: the hidden column (inside a slab of 64) at position j of the packed W2's k axis: bits 2 and 3 of j
    swapped (position 32 i + 16 p + 8 hb + 4 q + c holds column 32 i + 16 p + 8 q + 4 hb + c)."""
    j = torch.arange(64)
    return (j & ~12) | ((j & 4) << 1) | ((j & 8) >> 1)


def pack_occ_head_tensors(W1, b1, W2, b2, Dz, Ncls):
    """W1 [Hd, C], b1 [Hd], W2 [Dz Ncls, Hd], b2 [Dz Ncls] (any device / float dtype) -> OccHeadPacked of fp16 tensors:
    w1 [Hd, C] and b1 [Hd] as they are, w2 [Hd / 64, 32 nb, 64] and b2 [32 nb] in the kernel's row and k order
    (include/bevops.h), zero rows where padding is.  Not cached."""
    Hd, C = W1.shape
    nb = occ_head_blocks(Dz, Ncls)
    if nb == 0 or C % 32 or not 32 <= C <= 256 or Hd % 64 or not 64 <= Hd <= 1024:
        raise _lib.BevopsError("bevops_occ_head_f16: C % 32 == 0 in [32, 256], Hd % 64 == 0 in [64, 1024], Dz <= 16, "
                               "Ncls <= 32, Dz Ncls <= 320", _lib.NOT_SUPPORTED)
    if tuple(W2.shape) != (Dz * Ncls, Hd) or b1.numel() != Hd or b2.numel() != Dz * Ncls:
        raise ValueError("pack_occ_head: W1 [Hd, C], b1 [Hd], W2 [Dz Ncls, Hd], b2 [Dz Ncls]")
    col = occ_head_column_map(Dz, Ncls).to(W2.device)
    rows = W2.detach().to(torch.float16)[col.clamp_min(0)] * (col >= 0).to(torch.float16)[:, None]
    w2 = rows.view(32 * nb, Hd // 64, 64)[:, :, occ_head_k_map().to(W2.device)].permute(1, 0, 2).contiguous()
    b2p = b2.detach().to(torch.float16)[col.clamp_min(0)] * (col >= 0).to(torch.float16)
    return OccHeadPacked(W1.detach().to(torch.float16).contiguous(), b1.detach().to(torch.float16).contiguous(), w2,
                         b2p.contiguous(), C, Hd, Dz, Ncls, nb)


def pack_occ_head(W1, b1, W2, b2, Dz, Ncls, build=True):
    """`pack_occ_head_tensors` cached per weight tensors (keyed by W2, stamped with all four, as deconv_packed_weight's
    cache); rebuilt when one of them changes.  build=False: None when missing or stale.  Packing allocates and copies:
    never inside a stream capture (RuntimeError)."""
    stamp = tuple(_TensorCache._stamp(t) for t in (W1, b1, b2)) + (Dz, Ncls)
    hit = _PACKED.get(W2)
    if hit is not None and hit[0] == stamp:
        return hit[1]
    if not build:
        return None
    if W2.is_cuda and torch.cuda.is_current_stream_capturing():
        raise RuntimeError("occ_head: the packed weights are missing or stale and the stream is capturing; call "
                           "pack_occ_head(...) (or the layer once, eagerly) before the capture")
    return _PACKED.put(W2, (stamp, pack_occ_head_tensors(W1, b1, W2, b2, Dz, Ncls)))[1]


def occ_head_nhwc(y, packed, logits=False, out=None):
    """y [B, C, H, W] fp16 on the GPU, channels-last or a channel slice of a channels-last tensor; packed = pack_occ_head(...)
    -> occ [B, H, W, Dz] uint8, and with logits=True (or a dense fp16 [B, H, W, Dz Ncls] tensor to fill) (occ, logits).
    out: a uint8 [B, H, W, Dz] tensor or view to fill, any strides with a unit last one (a permuted view of a
    [B, W, H, Dz] tensor gives the library's axis order)."""
    if not (y.is_cuda and y.dtype == torch.float16 and y.dim() == 4):
        raise ValueError("occ_head_nhwc: y an fp16 CUDA tensor [B, C, H, W]")
    B, C, H, W = y.shape
    pitch = y.stride(3)
    if C != packed.C or y.stride(1) != 1 or pitch < C or (H > 1 and y.stride(2) != W * pitch) or \
            (B > 1 and y.stride(0) != H * W * pitch):
        raise ValueError("occ_head_nhwc: y channels-last (or a channel slice of such a tensor) with the packed C channels")
    if out is None:
        out = torch.empty((B, H, W, packed.Dz), dtype=torch.uint8, device=y.device)
    if out.dtype != torch.uint8 or tuple(out.shape) != (B, H, W, packed.Dz) or out.device != y.device or \
            (packed.Dz > 1 and out.stride(3) != 1):
        raise ValueError("occ_head_nhwc: out uint8 [B, H, W, Dz] on y's device with a unit last stride")
    lg = None
    if logits is not False and logits is not None:
        lg = torch.empty((B, H, W, packed.Dz * packed.Ncls), dtype=torch.float16, device=y.device) if logits is True else logits
        if lg.dtype != torch.float16 or tuple(lg.shape) != (B, H, W, packed.Dz * packed.Ncls) or not lg.is_contiguous():
            raise ValueError("occ_head_nhwc: logits a dense fp16 [B, H, W, Dz Ncls] tensor")
    if B * H * W:
        _call("bevops_occ_head_f16", y.device, y.data_ptr(), pitch, packed.w1.data_ptr(), packed.b1.data_ptr(),
              packed.w2.data_ptr(), packed.b2.data_ptr(), out.data_ptr(), out.stride(0), out.stride(1), out.stride(2),
              _ptr(lg), B, H, W, C, packed.Hd, packed.Dz, packed.Ncls)
    return out if lg is None else (out, lg)


def occ_head_plain(y, W1, b1, W2, b2, Dz, Ncls, logits=False):
    """The statement in torch, in y's dtype, on y's device: y [B, C, H, W] -> occ [B, H, W, Dz] uint8 (and the logits
    [B, H, W, Dz Ncls]).  Per pixel: h = softplus(W1 y + b1), logit = W2 h + b2 viewed [Dz, Ncls], occ = the lowest class
    among the largest logits of a voxel."""
    W1, b1, W2, b2 = (t.detach().to(y.dtype) for t in (W1, b1, W2, b2))
    lg = F.linear(F.softplus(F.linear(y.permute(0, 2, 3, 1), W1, b1)), W2, b2)
    v = lg.reshape(lg.shape[:3] + (Dz, Ncls))
    cls = torch.arange(Ncls, device=y.device).expand_as(v)
    occ = torch.where(v == v.amax(-1, keepdim=True), cls, Ncls - 1).amin(-1).to(torch.uint8)
    return (occ, lg) if logits else occ
