"""The fused first-block route (bevformer.Bottleneck.forward_nhwc: relu(conv3(h) + downsample(x)) as one two-source GEMM)
inside ResNet-50 + FPN at 2 x 3 x 192 x 256, the case of test_model_gpu.py::test_channels_last_backbone_matches_
reference_layout_path: against the NCHW path under that test's bars, against the two-launch route (difference printed),
run to run bit for bit; and one first block per stage shape class against float64, where the fused launch (one rounding)
must not be further from the exact value than the pair (two roundings) on the same operands."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def backbone():
    import bevformer_tensorrt_amd.functions as hip_ops
    from bevformer_tensorrt_amd import bevformer as B
    from bevformer_tensorrt_amd.functions.dispatch import using as dispatch_using
    torch.manual_seed(0)
    net = B.ResNet(50, (False, False, True, True), (1, 2, 3), hip_ops).cuda().half().eval()
    neck = B.FPN([512, 1024, 2048], 256, 4).cuda().half().eval()
    x = torch.randn(2, 3, 192, 256, device="cuda", dtype=torch.half)
    with torch.no_grad():
        ref = neck(net(x))
        for m in list(net.modules()) + list(neck.modules()):
            if isinstance(m, torch.nn.Conv2d) and m.kernel_size != (1, 1):
                m.weight.data = m.weight.data.contiguous(memory_format=torch.channels_last)

    def nhwc(fused, rule=None):
        was = B._FUSED_DOWNSAMPLE["enabled"]
        B._FUSED_DOWNSAMPLE["enabled"] = fused
        try:
            with torch.no_grad(), dispatch_using(rule=rule):
                return neck.forward_nhwc(net.forward_nhwc(x, hip_ops), hip_ops)
        finally:
            B._FUSED_DOWNSAMPLE["enabled"] = was
    # one untimed pass per route first: the measured dispatch and the library convolutions choose their algorithms on the
    # first call of a shape, and the first call itself may run another one than the calls after it
    nhwc(True), nhwc(False)
    return dict(B=B, ops=hip_ops, net=net, ref=ref, nhwc=nhwc, fused=nhwc(True), pair=nhwc(False))


def test_fused_route_is_taken(backbone, monkeypatch):
    """Every first block whose shape class is enabled reaches the two-source entry, once per frame."""
    B, ops = backbone["B"], backbone["ops"]
    calls = []
    real = ops.gemm2
    monkeypatch.setattr(ops, "gemm2", lambda *a, **k: (calls.append((a[0].shape[-1], a[1].shape[1], a[4])), real(*a, **k))[1])
    backbone["nhwc"](True)
    want = [s for s in ((64, 64, 1), (128, 256, 2), (256, 512, 2), (512, 1024, 2)) if s in B._FUSED_DOWNSAMPLE_SHAPES]
    assert calls == want
    calls.clear()
    backbone["nhwc"](False)
    assert calls == []


def test_fused_backbone_matches_the_nchw_path(backbone):
    for a, b in zip(backbone["ref"], backbone["fused"]):
        assert a.shape == b.shape and b.is_contiguous(memory_format=torch.channels_last)
        scale = max(1.0, a.abs().max().item())
        assert (a.float() - b.float()).abs().max().item() <= 3e-2 * scale
        assert (a.float() - b.float()).abs().mean().item() <= 3e-3 * scale


def test_fused_against_the_two_launch_route(backbone):
    """The two routes differ by the rounding of the identity tensor: the difference is printed, and bounded by the bars
    the NCHW comparison uses (both routes meet them against the same reference)."""
    for i, (a, b) in enumerate(zip(backbone["pair"], backbone["fused"])):
        d = (a.float() - b.float()).abs()
        scale = max(1.0, a.abs().max().item())
        print(f"level {i}: fused vs pair max {d.max().item():.3e} mean {d.mean().item():.3e} (scale {scale:.3f})")
        assert d.max().item() <= 3e-2 * scale and d.mean().item() <= 3e-3 * scale


def test_two_fused_runs_are_bit_identical(backbone):
    """Under the rule-based dispatch (every layer on a hand-written kernel: functions/dispatch.py DETERMINISTIC).  Under
    the measured dispatch this network at this size is not reproducible run to run with EITHER route from stage 2 on (the
    shapes are not in the shipped table, and the library kernels the measurement picks for them do not repeat their bits:
    the two-launch route differs between runs in the same way), so the statement about the fused route is made where the
    layers around it repeat theirs."""
    first, again = backbone["nhwc"](True, rule=True), backbone["nhwc"](True, rule=True)
    for i, (a, b) in enumerate(zip(first, again)):
        assert torch.equal(a, b), (i, (a.float() - b.float()).abs().max().item())
    for a, b in zip(backbone["ref"], first):          # ... and it is the same network
        assert (a.float() - b.float()).abs().max().item() <= 3e-2 * max(1.0, a.abs().max().item())


@pytest.mark.parametrize("cin,planes,stride,hw", [(64, 64, 1, (12, 20)), (256, 128, 2, (11, 15)), (512, 256, 2, (10, 14)),
                                                  (1024, 512, 2, (6, 9))])
def test_first_block_is_not_further_from_float64_than_the_pair(backbone, cin, planes, stride, hw):
    """relu(conv3(h) + downsample(x)) of one first block per stage shape class on given fp16 operands h, x: the fused
    launch and the pair against the float64 value.  The pair rounds the identity to fp16 and then the sum; the fused
    launch rounds the sum only (its bias b3 + bd is formed in fp32 and stored as fp16, an error of at most half an fp16
    unit of the BIAS, against half a unit of the whole identity value in the pair).  Per element either can be the
    closer one by chance, so the statement is about the error summed over the tensor."""
    B, ops = backbone["B"], backbone["ops"]
    torch.manual_seed(cin + stride)
    blk = B.Bottleneck(cin, planes, stride, False, ops, True).cuda().half().eval()
    H, W = hw
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    x = torch.randn(2, cin, H, W, device="cuda").half().contiguous(memory_format=torch.channels_last)
    h = torch.randn(2, planes, Ho, Wo, device="cuda").half().contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        w, b = B._stacked_pair(blk)
        fused = B._from_rows(ops.gemm2(B._rows(h), x, w, b, stride, True), 2, Ho, Wo)
        pair = B._conv1x1_nhwc(ops, h, blk.conv3, True, residual=B._conv1x1_nhwc(ops, x, blk.downsample, False))
        xs = x[:, :, ::stride, ::stride].double()
        want = torch.relu(torch.einsum("bkhw,nk->bnhw", h.double(), blk.conv3.weight.double().view(-1, planes))
                          + torch.einsum("bkhw,nk->bnhw", xs, blk.downsample.weight.double().view(-1, cin))
                          + (blk.conv3.bias.double() + blk.downsample.bias.double()).view(1, -1, 1, 1))
    ef, ep = (fused.double() - want).abs(), (pair.double() - want).abs()
    print(f"{(planes, cin, stride)}: fused mean {ef.mean().item():.4e} max {ef.max().item():.4e}; "
          f"pair mean {ep.mean().item():.4e} max {ep.max().item():.4e}")
    assert ef.sum().item() <= ep.sum().item()
    assert ef.max().item() <= 2.0 ** -10 * max(1.0, want.abs().max().item())     # half an fp16 unit of the largest value, doubled
