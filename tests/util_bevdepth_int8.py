"""Stand-in operator sets for the tests of the INT8 BEVDepth (tests/test_bevdepth_int8_cpu.py): tests/util_bevdet_int8.py's
`ShapeOps` and `ScaleRecorder` with the entries the DepthNet's int8 plan adds -- the dilation / image_bias keywords of
conv_slice_q_taps, se_gate2_nhwc_q, global_avgpool_nhwc_q, and the fp32 / fp16 entries that carry no scale
(lss_camera_gate, dense_auto)."""
import torch

import util_bevdet_int8 as U


class ShapeOps(U.ShapeOps):
    def conv_slice_q_taps(self, x_q, scale_x, w, ws, bias, act, residual_q=None, scale_res=1.0, stride=1, out=None,
                          scale_out=None, out_dtype=torch.int8, res_first=False, dilation=1, image_bias=None):
        if image_bias is not None:
            assert bias is None and image_bias.dtype == torch.float16 and tuple(image_bias.shape) == (x_q.shape[0], w.shape[0])
        assert dilation == 1 or (w.shape[1] == 3 and stride == 1)
        return super().conv_slice_q_taps(x_q, scale_x, w, ws, bias, act, residual_q, scale_res, stride, out, scale_out,
                                         out_dtype, res_first)

    def lss_camera_gate(self, mlp_input, packed, mid, out=None):
        assert mlp_input.dtype == torch.float32 and mlp_input.shape[1] == 27
        return torch.zeros((2, mlp_input.shape[0], mid), dtype=torch.float32, device=mlp_input.device)

    def se_gate2_nhwc_q(self, x_q, scale_x, gates, scale_a, scale_b, out_a=None, out_b=None):
        n, c, H, W = x_q.shape
        assert x_q.dtype == torch.int8 and tuple(gates.shape) == (2, n, c)
        return U._nhwc(n, c, H, W, torch.int8, x_q.device), U._nhwc(n, c, H, W, torch.int8, x_q.device)

    def global_avgpool_nhwc_q(self, x_q, scale_x, out=None):
        assert x_q.dtype == torch.int8
        return torch.zeros(x_q.shape[:2], dtype=torch.float16, device=x_q.device)

    def dense_auto(self, x, w, b, res, relu):
        assert x.dtype == torch.float16 and x.shape[1] == w.shape[1] and res is None
        return torch.zeros((x.shape[0], w.shape[0]), dtype=torch.float16, device=x.device)


class ScaleRecorder(U.ScaleRecorder):
    def conv_slice_q_taps(self, x_q, scale_x, w, ws, bias, act, residual_q=None, scale_res=1.0, stride=1, out=None,
                          scale_out=None, out_dtype=torch.int8, res_first=False, dilation=1, image_bias=None):
        self._read(x_q, scale_x, "conv input")
        if residual_q is not None:
            self._read(residual_q, scale_res, "conv identity")
        y = self._call("conv_slice_q_taps", (x_q, scale_x, w, ws, bias, act, residual_q, scale_res, stride, out, scale_out,
                                             out_dtype), dict(res_first=res_first, dilation=dilation, image_bias=image_bias))
        return self._wrote(y, scale_out, "conv output")

    def lss_camera_gate(self, *args, **kw):
        return self._call("lss_camera_gate", args, kw)

    def dense_auto(self, *args, **kw):
        return self._call("dense_auto", args, kw)

    def se_gate2_nhwc_q(self, x_q, scale_x, gates, scale_a, scale_b, out_a=None, out_b=None):
        self._read(x_q, scale_x, "gate input")
        a, b = self._call("se_gate2_nhwc_q", (x_q, scale_x, gates, scale_a, scale_b), {})
        return self._wrote(a, scale_a, "gated depth copy"), self._wrote(b, scale_b, "gated context copy")

    def global_avgpool_nhwc_q(self, x_q, scale_x, out=None):
        self._read(x_q, scale_x, "average pool input")
        return self._call("global_avgpool_nhwc_q", (x_q, scale_x), {})
