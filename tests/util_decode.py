"""Shared by test_decode_cpu.py / test_decode_gpu.py: the golden cases of tests/golden/make_decode_golden.py as
python objects, the padded form of what the reference returned, and fp64 evaluations of the golden inputs."""
import numpy as np
import torch

from conftest import golden

NF_RANGE = [-61.2, -61.2, -10.0, 61.2, 61.2, 10.0]
# box columns that are copies of an input value / that go through a transcendental or an fp32 multiply-add
NF_COPIED, NF_COMPUTED = (0, 1, 2, 7, 8), (3, 4, 5, 6)
CP_COPIED, CP_COMPUTED = (2, 7, 8), (0, 1, 3, 4, 5, 6)


def _items(g, name, batch):
    return [{k: g[f"{name}_{k}{b}"] for k in ("bboxes", "scores", "labels", "index")} for b in range(batch)]


def nf_cases():
    g = golden("decode_nms_free")
    out = []
    for name in g["names"].tolist():
        K, thr = g[f"{name}_params"].tolist()
        cls, box = torch.from_numpy(g[f"{name}_cls"]), torch.from_numpy(g[f"{name}_box"])
        out.append(dict(name=name, cls=cls, box=box, max_num=int(K), thr=None if thr < 0 else thr,
                        items=_items(g, name, cls.shape[0])))
    return out


def cp_cases():
    g = golden("decode_centerpoint")
    out = []
    for name in g["names"].tolist():
        p = g[f"{name}_params"].tolist()
        heat = torch.from_numpy(g[f"{name}_heat"])
        maps = {k: (torch.from_numpy(g[f"{name}_{k}"]).float() if f"{name}_{k}" in g else None)
                for k in ("reg", "height", "dim", "rot", "vel")}
        out.append(dict(name=name, heat=heat, max_num=int(p[0]), thr=None if p[1] < 0 else p[1], osf=int(p[2]),
                        voxel=p[3:5], pc=p[5:7], range=p[7:13], items=_items(g, name, heat.shape[0]), **maps))
    return out


def cp_args(c, device=None, dtype=None, channels_last=False):
    """Positional arguments of centerpoint_decode / centerpoint_decode_torch for a golden case."""
    def mv(t):
        if t is None or device is None:
            return t
        t = t.to(device=device, dtype=dtype or t.dtype)
        return t.contiguous(memory_format=torch.channels_last) if channels_last else t
    return ([mv(c[k]) for k in ("reg", "height", "dim", "rot", "vel")] + [mv(c["heat"])] +
            [c["max_num"], c["range"], c["pc"], c["osf"], c["voxel"], c["thr"]])


def golden_padded(items, max_num, label_columns=9):
    """What the reference returned per item, laid out as the padded form (numpy)."""
    B = len(items)
    boxes, scores = np.zeros((B, max_num, 9), np.float32), np.zeros((B, max_num), np.float32)
    labels, count = np.zeros((B, max_num), np.int32), np.zeros(B, np.int32)
    for b, it in enumerate(items):
        n = it["scores"].shape[0]
        boxes[b, :n, :it["bboxes"].shape[1]] = it["bboxes"]
        scores[b, :n], labels[b, :n], count[b] = it["scores"], it["labels"].astype(np.int32), n
    return boxes, scores, labels, count


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def nf_fp64(cls, box, index, num_classes):
    """fp64 (score, e^w, e^l, e^h, angle) of the candidates `index` [K] of one item (inputs widened exactly)."""
    cls, box = cls.double().reshape(-1), box.double()
    p = box[torch.div(index, num_classes, rounding_mode="trunc")]
    return dict(score=torch.sigmoid(cls[index]), w=p[:, 2].exp(), l=p[:, 3].exp(), h=p[:, 5].exp(),
                rot=torch.atan2(p[:, 6], p[:, 7]))


def cp_fp64(c, b, index, maps=None):
    """fp64 (score, x, y, dims, angle) of the cells `index` [K] of item b of a CenterPoint case."""
    m = maps or c
    heat = m["heat"].double()
    _, nc, H, W = heat.shape
    cell = index % (H * W)
    at = lambda t, ch: t[b, ch].double().reshape(-1)[cell]
    rx = at(m["reg"], 0) if m["reg"] is not None else 0.5
    ry = at(m["reg"], 1) if m["reg"] is not None else 0.5
    x = ((cell % W).double() + rx) * c["osf"] * c["voxel"][0] + c["pc"][0]
    y = (torch.div(cell, W, rounding_mode="trunc").double() + ry) * c["osf"] * c["voxel"][1] + c["pc"][1]
    return dict(score=torch.sigmoid(heat[b].reshape(-1)[index]), x=x, y=y, d0=at(m["dim"], 0).exp(),
                d1=at(m["dim"], 1).exp(), d2=at(m["dim"], 2).exp(), rot=torch.atan2(at(m["rot"], 0), at(m["rot"], 1)))


def ulp32(v):
    return np.spacing(np.abs(np.asarray(v, np.float64)).astype(np.float32)).astype(np.float64)
