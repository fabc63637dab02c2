"""Graph capture of a fixed-shape forward, and the runner of the two 2-D detectors built on it.

`capture` is the warm-up-then-capture routine of every runner whose frame is one function of static buffers
(YOLOXRunner, CenterNetRunner, BEVDetRunner and the timing tools).  bevformer.FrameRunner keeps its own: its capture
differs in substance (RCCL, prev_bev, decode in the warm-up)."""
import torch

from .functions.image import DETECT2D_IMAGE_PIPELINES


def capture(forward, warmup=2):
    """`forward()` `warmup` times on a side stream (allocations, packed and merged operands, library algorithm search),
    then once under torch.cuda.graph -> (graph, the outputs of the captured call: the graph's static tensors)."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(warmup):
            forward()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = forward()
    return graph, outs


class Detect2DRunner:
    """The network, its decode and its NMS captured once for images of one shape, and once more from raw camera frames.

    A subclass gives `_forward(raw)` -> the head maps followed by the four fixed-size detection outputs, and
      _detector   the detector's name in the error messages,
      _heads      the slice bound between the two: outputs[:_heads] are head maps, outputs[_heads:] the detections,
      _geometry   the geometry function of its test pipeline (functions.image), as a staticmethod,
      _pipeline   its key in functions.image.DETECT2D_IMAGE_PIPELINES,
    and may refuse a size in `_check_size(model, height, width)`.  A graph is captured at the first call of its entry point
    (`step`: _graph / _outs, `step_raw`: _graph_raw / _outs_raw), so a runner that only ever calls one pays for one."""
    _detector = _heads = _geometry = _pipeline = None

    def __init__(self, model, batch, height, width, graph=True, clone_outputs=True, raw_size=None, img_scale=None):
        if height % 32 or width % 32:
            raise ValueError(f"{type(self).__name__}: height and width are multiples of 32")
        self._check_size(model, height, width)
        p = next(model.parameters())
        self.model, self.use_graph, self.clone_outputs = model, graph, clone_outputs
        self.image_buffer = torch.zeros((batch, 3, height, width), device=p.device, dtype=p.dtype)
        self._graph, self._outs, self._last = None, None, None
        self.raw_size, self.geometry, self.raw_buffer, self._graph_raw, self._outs_raw = None, None, None, None, None
        if raw_size is not None:
            self.pipeline = DETECT2D_IMAGE_PIPELINES[self._pipeline]
            self.raw_size = (int(raw_size[0]), int(raw_size[1]))
            self.geometry = self._geometry(*self.raw_size, img_scale or self.pipeline["img_scale"])
            if tuple(self.geometry["pad_shape"][:2]) != (height, width):
                raise ValueError(f"raw_size {self.raw_size}: {self._detector}'s test pipeline gives a network input of "
                                 f"{tuple(self.geometry['pad_shape'][:2])}, the runner was asked for {(height, width)}")
            self.raw_buffer = torch.zeros((batch,) + self.raw_size + (3,), device=p.device, dtype=torch.uint8)

    def _check_size(self, model, height, width):
        pass

    def _capture(self, raw=False):
        graph, outs = capture(lambda: self._forward(raw))
        if raw:
            self._graph_raw, self._outs_raw = graph, outs
        else:
            self._graph, self._outs = graph, outs

    def _detections(self, outs):
        self._last = outs
        dets = outs[self._heads:]
        return tuple(t.clone() for t in dets) if self.clone_outputs and self.use_graph else dets

    def step(self, image):
        if tuple(image.shape) != tuple(self.image_buffer.shape):
            raise ValueError(f"the runner was built for images {tuple(self.image_buffer.shape)}")
        if image.data_ptr() != self.image_buffer.data_ptr():
            self.image_buffer.copy_(image, non_blocking=True)
        if not self.use_graph:
            self._outs = self._forward()
        else:
            if self._graph is None:
                self._capture()
            self._graph.replay()
        return self._detections(self._outs)

    def step_raw(self, raw):
        """`step` from the RAW camera images [B, H0, W0, 3] uint8 BGR on the device (raw_size=(H0, W0) at construction;
        passing `raw_buffer` itself saves the copy): the letterbox launch, the network and the detector's post-processing
        with the geometry's border / scale_factor as one graph of its own.  The boxes are in the raw image's pixels."""
        if self.raw_size is None:
            raise RuntimeError(f"step_raw needs {type(self).__name__}(..., raw_size=(H0, W0))")
        if raw.dtype != torch.uint8 or tuple(raw.shape) != tuple(self.raw_buffer.shape):
            raise ValueError(f"raw must be uint8 {tuple(self.raw_buffer.shape)}")
        if raw.data_ptr() != self.raw_buffer.data_ptr():
            self.raw_buffer.copy_(raw, non_blocking=True)
        if not self.use_graph:
            self._outs_raw = self._forward(True)
        else:
            if self._graph_raw is None:
                self._capture(True)
            self._graph_raw.replay()
        return self._detections(self._outs_raw)

    @property
    def head_outputs(self):
        """The head maps of the last `step` / `step_raw` (YOLOX: the nine head outputs; CenterNet: center_heatmap_preds,
        wh_preds, offset_preds): the graph's static tensors, overwritten by the next one."""
        return None if self._last is None else self._last[:self._heads]
