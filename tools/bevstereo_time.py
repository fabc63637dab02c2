#!/usr/bin/env python3
"""BEVStereo's temporal-stereo cost volume (csrc/stereo_cost.hip) on one MI355X, under HIP-graph replay, arms replayed
alternately.

  op        stereo_cost_volume -- ONE launch, the grid computed inside it -- against the reference's op sequence as
            torch device ops (stereo_grid_plain + stereo_cost_volume_plain: 64 grid_sample calls on groups of four
            channels, abs, two sums, a masked add, a softmax; fp16 features as the reference would run them under
            autocast-free fp16), at (6, 256, 64, 176) with D = 59 and at 2 cameras.  And the launch fed an explicit grid.
  depthnet  LSSViewTransformer*._depth_feat (DepthNet + softmax / split) on fixed image features, BEVSTEREO_R50 against
            BEVDEPTH_R50

Per alternation the mean of `--replays` replays between two events; median and maximum per arm.  One JSON line per
record, appended to profiles/bevstereo/<step>.jsonl.  Every step is a child process of its own under `timeout`; the
script stops at the first step that fails.  The torch op sequence cannot be captured (its masked add reads a count
back to the host): that arm is timed as eager launches inside the same alternation, the record lists it in
`eager_arms` and its workload string says so -- such a ratio is graph replay against eager launches.  No ratio here
is a gate: the records say what was measured, slower included.

    python tools/bevstereo_time.py [--alternations 7] [--replays 20] [--out-dir profiles/bevstereo]
    python tools/bevstereo_time.py --step op      # one step, in this process"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bevdepth_time import _alternate, _capture, _record      # noqa: E402  (the protocol of tools/bevdepth_time.py)

STEPS = (("op", 420), ("depthnet", 300))      # (name, seconds)


def _stereo_inputs(view, n, seed=0):
    import torch
    from bevformer_tensorrt_amd import bevdet as D
    from bevformer_tensorrt_amd.functions import stereo_calibration, stereo_frustum_tables
    _, _, K, pr, pt, _ = D.jittered_rig(view, 2, n_cams=n)
    g = torch.Generator().manual_seed(seed)
    k2s = torch.eye(4).repeat(1, n, 1, 1)
    k2s[0, :, :3, 3] = (torch.rand(n, 3, generator=g) - 0.5) * torch.tensor([0.6, 0.05, 1.2])       # ego motion of a frame
    consts = stereo_calibration(k2s, K, pr, pt).cuda()
    tables = tuple(t.cuda() for t in stereo_frustum_tables(view.cv_frustum))
    return k2s, K, pr, pt, consts, tables


def step_op(a):
    import torch
    import bevformer_tensorrt_amd as bev
    from bevformer_tensorrt_amd import bevdet as D
    from bevformer_tensorrt_amd.bevdepth import LSSViewTransformerBEVStereo
    cfg = {k: D.BEVSTEREO_R50[k] for k in ("grid_config", "input_size", "downsample", "in_channels", "out_channels")}
    view = LSSViewTransformerBEVStereo(**cfg, ops=object(), depthnet_cfg=D.BEVSTEREO_R50["depthnet_cfg"])
    g = torch.Generator().manual_seed(0)
    recs = []
    for n in (6, 2):
        C, H, W, Dn, bias = 256, 64, 176, view.D, 5.0
        _, _, _, _, consts, tables = _stereo_inputs(view, n)
        feats = [(torch.relu(torch.randn(n, C, H, W, generator=g)) * 0.1).cuda().half().contiguous(
            memory_format=torch.channels_last) for _ in range(2)]
        prev, curr = feats
        prev_p, curr_p = prev.contiguous(), curr.contiguous()              # planar copies for the torch arm, made outside
        grid = bev.stereo_grid(consts, tables)

        def launch():
            return bev.stereo_cost_volume(prev, curr, consts, Dn, bias, frustum_tables=tables, dpad=64)

        def launch_grid():
            return bev.stereo_cost_volume(prev, curr, grid, Dn, bias, dpad=64)

        def torch_ops():
            return bev.stereo_cost_volume_plain(prev_p, curr_p, bev.stereo_grid_plain(consts, tables), bias)

        diff = (launch()[:, :Dn].float() - torch_ops().float()).abs().max().item()
        graphs = {"one_launch": _capture(launch)[0], "one_launch_explicit_grid": _capture(launch_grid)[0]}
        # the reference's masked add (`cost[invalid] = cost[invalid] + bias`) indexes with a boolean mask, which reads
        # a count back to the host: that op sequence cannot be captured, so its arm is eager launches, and is named so
        graphs["torch_op_sequence_eager"] = _Eager(torch_ops)
        eager_arms = ["torch_op_sequence_eager"]
        ms = _alternate(graphs, a)
        how = "HIP-graph replay" if not eager_arms else "HIP-graph replay except the arms in eager_arms (eager launches)"
        recs.append(_record("op", f"stereo cost volume, ({n}, 256, 64, 176), D 59, bias 5, channels-last fp16, {how}",
                            ms, a, cameras=n, max_abs_diff_vs_torch_fp16=diff, eager_arms=eager_arms))
    return recs


class _Eager:
    """An arm that cannot be captured, behind the replay interface."""

    def __init__(self, fn):
        self.fn = fn

    def replay(self):
        self.fn()


def step_depthnet(a):
    import torch
    from bevformer_tensorrt_amd import bevdet as D
    img = torch.randn(1, 6, 3, 256, 704, generator=torch.Generator().manual_seed(1)).cuda().half()
    graphs = {}
    for arm, cfg in (("stereo", D.BEVSTEREO_R50), ("no_stereo", D.BEVDEPTH_R50)):
        m = D.BEVDet(cfg, seed=0, bev_half="hip").cuda().half()
        calib = m.view.calibration_matrices(*D.synthetic_rig(m.view)).cuda()
        mlp = m.view.split_calibration(calib)[1]
        if arm == "stereo":
            k2s, K, pr, pt, _, _ = _stereo_inputs(m.view, 6)
            x, feat = m.image_features(img.flatten(0, 1), stereo=True)
            prev = feat.roll(2, 3).contiguous(memory_format=torch.channels_last)
            metas = m.view.stereo_metas(prev, feat, k2s, K, pr, pt, prepare=True)
            m.forward_calibrated(img, calib, metas)              # (eager: dispatch choices, packed operands)
            graphs[arm] = _capture(lambda m=m, x=x, mlp=mlp, metas=metas: m.view._depth_feat(x, mlp, metas)[:2])[0]
        else:
            m.forward_calibrated(img, calib)
            x = m.image_features(img.flatten(0, 1))
            graphs[arm] = _capture(lambda m=m, x=x, mlp=mlp: m.view._depth_feat(x, mlp)[:2])[0]
    ms = _alternate(graphs, a)
    return [_record("depthnet", "DepthNet + softmax / split at R50 (6 x 16 x 44, mid 256, D 59, C 64; stereo map 6 x 256 x 64 "
                    "x 176) on fixed image features, with and without the stereo branch, HIP-graph replay, fp16", ms, a)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--alternations", type=int, default=7)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "bevstereo"))
    ap.add_argument("--step", choices=[s for s, _ in STEPS])
    a = ap.parse_args()
    os.makedirs(a.out_dir, exist_ok=True)
    if a.step:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("bevstereo_time: needs a GPU (no timing without one)")
        recs = globals()["step_" + a.step](a)
        with open(os.path.join(a.out_dir, a.step + ".jsonl"), "a") as f:
            for r in recs:
                line = json.dumps(r)
                print(line)
                f.write(line + "\n")
        return
    for step, seconds in STEPS:
        cmd = ["timeout", "-k", "10", str(seconds), sys.executable, os.path.abspath(__file__), "--step", step,
               "--alternations", str(a.alternations), "--replays", str(a.replays), "--out-dir", a.out_dir]
        rc = subprocess.call(cmd)
        if rc != 0:
            raise SystemExit(f"bevstereo_time: step {step} ended with status {rc}; stopping")


if __name__ == "__main__":
    main()
