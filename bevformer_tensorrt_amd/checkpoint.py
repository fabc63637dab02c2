"""Loading the reference's checkpoints (the public BEVFormer / mmdet3d state dicts that
tools/bevformer/evaluate_pth.py:45 and the pth->onnx->trt flow start from) into the mmcv-free re-host.

The re-hosted modules (bevformer.py) carry the same parameters under shorter names and with every
frozen BatchNorm (`norm_eval=True`, configs/bevformer/bevformer_base.py:49) folded into the
convolution in front of it.  `reference_key_map(model)` lists, for every parameter of OUR model, the
reference key(s) it comes from; `load_reference_state_dict` applies it (folding the BN statistics)
and reports what was missing / left over.  Name sources in the reference tree:

  img_backbone.*      det2trt/models/backbones/resnet.py:106-260 (Bottleneck: conv1..3 + bn1..3 via
                      add_module(norm{1,2,3}_name), downsample = Sequential(conv, norm) from mmdet's
                      ResLayer), :507-509 (layer{i+1}); DCN pack: modules/cnn/dcn.py:31-86 (conv_offset)
  img_neck.*          third_party/bev_mmdet3d/models/necks/fpn.py:108-155 (lateral_convs / fpn_convs,
                      each an mmcv ConvModule -> `.conv`)
  pts_bbox_head.*     dense_heads/bevformer_head.py:121-209 (bev_embedding, query_embedding,
                      positional_encoding, cls_branches, reg_branches)
  ...transformer.*    modules/transformer.py:28-67 (level_embeds, cams_embeds, reference_points,
                      can_bus_mlp{0,2,norm}); encoder / decoder layers are mmcv BaseTransformerLayer
                      instances (attentions.{i}, ffns.0.layers.{0.0,1}, norms.{i}); SCA wraps its
                      sampler as `deformable_attention` (modules/spatial_cross_attention.py:58-104); the
                      decoder's self attention is mmcv MultiheadAttention (`attn` = nn.MultiheadAttention)
"""
import torch

BN_EPS = 1e-5   # mmcv build_norm_layer(dict(type="BN")) default


def _conv_bn(conv_key, bn_key):
    return ("conv_bn", conv_key, bn_key)


def reference_key_map(model):
    """{our parameter name: source}, source = a reference key (copied as is) or
    ("conv_bn", conv_prefix, bn_prefix) -> (weight, bias) of the convolution with the BN folded in.
    Folded entries are listed under OUR `<module>.weight`; the matching `<module>.bias` maps to the
    same tuple."""
    cfg = model.cfg
    m = {}

    def fold(ours, conv, bn):
        m[ours + ".weight"] = _conv_bn(conv, bn)
        m[ours + ".bias"] = _conv_bn(conv, bn)

    def copy(ours, ref, names=("weight", "bias")):
        for n in names:
            m[f"{ours}.{n}"] = f"{ref}.{n}"

    # ---- backbone
    fold("backbone.stem", "img_backbone.conv1", "img_backbone.bn1")
    for s, stage in enumerate(model.backbone.stages):
        for j, blk in enumerate(stage):
            ours, ref = f"backbone.stages.{s}.{j}", f"img_backbone.layer{s + 1}.{j}"
            fold(ours + ".conv1", ref + ".conv1", ref + ".bn1")
            fold(ours + ".conv2", ref + ".conv2", ref + ".bn2")
            if hasattr(blk.conv2, "conv_offset"):
                copy(ours + ".conv2.conv_offset", ref + ".conv2.conv_offset")
            fold(ours + ".conv3", ref + ".conv3", ref + ".bn3")
            if blk.downsample is not None:
                fold(ours + ".downsample", ref + ".downsample.0", ref + ".downsample.1")
    # ---- neck
    n_in = len(cfg["fpn_in"])
    for i in range(n_in):
        copy(f"neck.lateral.{i}", f"img_neck.lateral_convs.{i}.conv")
        copy(f"neck.fpn.{i}", f"img_neck.fpn_convs.{i}.conv")
    for k in range(len(model.neck.extra)):
        copy(f"neck.extra.{k}", f"img_neck.fpn_convs.{n_in + k}.conv")
    # ---- head
    H = "pts_bbox_head"
    m["bev_embedding.weight"] = f"{H}.bev_embedding.weight"
    m["query_embedding.weight"] = f"{H}.query_embedding.weight"
    m["row_embed.weight"] = f"{H}.positional_encoding.row_embed.weight"
    m["col_embed.weight"] = f"{H}.positional_encoding.col_embed.weight"
    for i in range(len(model.cls_branches)):
        for k in (0, 1, 3, 4, 6):     # Linear, LayerNorm, ReLU, Linear, LayerNorm, ReLU, Linear
            copy(f"cls_branches.{i}.{k}", f"{H}.cls_branches.{i}.{k}")
        for k in (0, 2, 4):           # Linear, ReLU, Linear, ReLU, Linear
            copy(f"reg_branches.{i}.{k}", f"{H}.reg_branches.{i}.{k}")
    # ---- transformer
    T = f"{H}.transformer"
    m["level_embeds"] = f"{T}.level_embeds"
    m["cams_embeds"] = f"{T}.cams_embeds"
    copy("reference_points", f"{T}.reference_points")
    copy("can_bus_mlp.0", f"{T}.can_bus_mlp.0")
    copy("can_bus_mlp.2", f"{T}.can_bus_mlp.2")
    copy("can_bus_mlp.4", f"{T}.can_bus_mlp.norm")
    att = ("sampling_offsets", "attention_weights", "value_proj", "output_proj")
    for i in range(len(model.encoder)):
        ours, ref = f"encoder.{i}", f"{T}.encoder.layers.{i}"
        for a in att:
            copy(f"{ours}.tsa.{a}", f"{ref}.attentions.0.{a}")
        for a in att[:3]:
            copy(f"{ours}.sca.{a}", f"{ref}.attentions.1.deformable_attention.{a}")
        copy(f"{ours}.sca.output_proj", f"{ref}.attentions.1.output_proj")
        copy(f"{ours}.ffn.fc1", f"{ref}.ffns.0.layers.0.0")
        copy(f"{ours}.ffn.fc2", f"{ref}.ffns.0.layers.1")
        for k in range(3):
            copy(f"{ours}.norms.{k}", f"{ref}.norms.{k}")
    for i in range(len(model.decoder)):
        ours, ref = f"decoder.{i}", f"{T}.decoder.layers.{i}"
        m[f"{ours}.self_attn.in_proj_weight"] = f"{ref}.attentions.0.attn.in_proj_weight"
        m[f"{ours}.self_attn.in_proj_bias"] = f"{ref}.attentions.0.attn.in_proj_bias"
        copy(f"{ours}.self_attn.out_proj", f"{ref}.attentions.0.attn.out_proj")
        for a in att:
            copy(f"{ours}.cross_attn.{a}", f"{ref}.attentions.1.{a}")
        copy(f"{ours}.ffn.fc1", f"{ref}.ffns.0.layers.0.0")
        copy(f"{ours}.ffn.fc2", f"{ref}.ffns.0.layers.1")
        for k in range(3):
            copy(f"{ours}.norms.{k}", f"{ref}.norms.{k}")
    return m


def centernet_key_map(model):
    """`reference_key_map` for centernet.CenterNet: {our parameter name: source} from mmdet 2.x's CenterNet state dict
    (backbone = ResNet-18, neck = CTResNetNeck with use_dcn, bbox_head = CenterNetHead).  Key names as mmdet 2.x's
    modules register them:

      backbone.conv1 / bn1, backbone.layer{1..4}.{0,1}.conv{1,2} / bn{1,2}, .downsample.{0,1}   (mmdet ResNet, BasicBlock)
      neck.deconv_layers.{0,2,4}.conv (+ .conv_offset) / .bn     the DCN packs (mmcv ConvModule -> `.conv`, `.bn`)
      neck.deconv_layers.{1,3,5}.conv / .bn                       the transposed convolutions
      bbox_head.{heatmap,wh,offset}_head.{0,2}                     Sequential(conv3x3, ReLU, conv1x1)

    ("deconv_bn", conv, bn): the BN behind a ConvTranspose2d, folded with `fold_deconv_bn`.  Neither mmdet nor a
    checkpoint is available to this repository's tests: parity with the library's names is unpinned."""
    m = {}

    def fold(ours, conv, bn, tag="conv_bn"):
        m[ours + ".weight"] = (tag, conv, bn)
        m[ours + ".bias"] = (tag, conv, bn)

    fold("backbone.stem", "backbone.conv1", "backbone.bn1")
    for s, stage in enumerate(model.backbone.stages):
        for j, blk in enumerate(stage):
            ours, ref = f"backbone.stages.{s}.{j}", f"backbone.layer{s + 1}.{j}"
            fold(ours + ".conv1", ref + ".conv1", ref + ".bn1")
            fold(ours + ".conv2", ref + ".conv2", ref + ".bn2")
            if blk.downsample is not None:
                fold(ours + ".downsample", ref + ".downsample.0", ref + ".downsample.1")
    for i in range(len(model.neck.dcn)):
        ref = f"neck.deconv_layers.{2 * i}"
        fold(f"neck.dcn.{i}", ref + ".conv", ref + ".bn")
        for n in ("weight", "bias"):
            m[f"neck.dcn.{i}.conv_offset.{n}"] = f"{ref}.conv.conv_offset.{n}"
        ref = f"neck.deconv_layers.{2 * i + 1}"
        fold(f"neck.deconv.{i}", ref + ".conv", ref + ".bn", "deconv_bn")
    for k, head in model.heads.items():
        for ours, ref in ((0, 0), (1, 2)):
            for n in ("weight", "bias"):
                m[f"heads.{k}.{ours}.{n}"] = f"bbox_head.{k}_head.{ref}.{n}"
    return m


YOLOX_BN_EPS = 1e-3   # norm_cfg=dict(type="BN", momentum=0.03, eps=0.001) of every YOLOX ConvModule


def yolox_key_map(model):
    """`reference_key_map` for yolox.YOLOX: {our parameter name: source} from mmdet 2.x's YOLOX state dict (backbone =
    CSPDarknet, neck = YOLOXPAFPN, bbox_head = YOLOXHead).  Every ConvModule registers `.conv` and `.bn`; key names as
    mmdet 2.x's modules register them:

      backbone.stem.conv                                             Focus' ConvModule
      backbone.stage{1..4}.0                                         the 3x3 / 2 ConvModule
      backbone.stage4.1.conv{1,2}                                    SPPBottleneck
      backbone.stage{i}.{1 | 2}.{main,short,final}_conv, .blocks.{j}.conv{1,2}     CSPLayer (index 2 behind the SPP)
      neck.reduce_layers.{i}, neck.top_down_blocks.{i}, neck.downsamples.{i}, neck.bottom_up_blocks.{i}, neck.out_convs.{i}
      bbox_head.multi_level_cls_convs.{l}.{0,1}, .multi_level_reg_convs.{l}.{0,1}  the towers
      bbox_head.multi_level_conv_{cls,reg,obj}.{l}                    the predictors (plain convolutions, copied)

    ("conv_bn_yolox", conv, bn): folded with `fold_conv_bn` at eps 1e-3.  Neither mmdet nor a checkpoint is available
    to this repository's tests: parity with the library's names is unpinned."""
    m = {}

    def fold(ours, ref):
        m[ours + ".weight"] = ("conv_bn_yolox", ref + ".conv", ref + ".bn")
        m[ours + ".bias"] = ("conv_bn_yolox", ref + ".conv", ref + ".bn")

    def csp(ours, ref, layer):
        for n in ("main_conv", "short_conv", "final_conv"):
            fold(f"{ours}.{n}", f"{ref}.{n}")
        for j in range(len(layer.blocks)):
            fold(f"{ours}.blocks.{j}.conv1", f"{ref}.blocks.{j}.conv1")
            fold(f"{ours}.blocks.{j}.conv2", f"{ref}.blocks.{j}.conv2")

    fold("backbone.stem.conv", "backbone.stem.conv")
    for i, stage in enumerate(model.backbone.stages):
        ours, ref = f"backbone.stages.{i}", f"backbone.stage{i + 1}"
        fold(ours + ".0", ref + ".0")
        if len(stage) == 3:
            fold(ours + ".1.conv1", ref + ".1.conv1")
            fold(ours + ".1.conv2", ref + ".1.conv2")
        k = len(stage) - 1
        csp(f"{ours}.{k}", f"{ref}.{k}", stage[k])
    neck = model.neck
    for i in range(len(neck.reduce_layers)):
        fold(f"neck.reduce_layers.{i}", f"neck.reduce_layers.{i}")
        fold(f"neck.downsamples.{i}", f"neck.downsamples.{i}")
        csp(f"neck.top_down_blocks.{i}", f"neck.top_down_blocks.{i}", neck.top_down_blocks[i])
        csp(f"neck.bottom_up_blocks.{i}", f"neck.bottom_up_blocks.{i}", neck.bottom_up_blocks[i])
    for i in range(len(neck.out_convs)):
        fold(f"neck.out_convs.{i}", f"neck.out_convs.{i}")
    head = model.bbox_head
    for l in range(len(head.cls_convs)):
        for j in range(len(head.cls_convs[l])):
            fold(f"bbox_head.cls_convs.{l}.{j}", f"bbox_head.multi_level_cls_convs.{l}.{j}")
            fold(f"bbox_head.reg_convs.{l}.{j}", f"bbox_head.multi_level_reg_convs.{l}.{j}")
        for k in ("cls", "reg", "obj"):
            for n in ("weight", "bias"):
                m[f"bbox_head.conv_{k}.{l}.{n}"] = f"bbox_head.multi_level_conv_{k}.{l}.{n}"
    return m


def load_yolox_state_dict(model, state_dict, strict=True):
    """`load_reference_state_dict` for yolox.YOLOX and mmdet's YOLOX checkpoint (`yolox_key_map`)."""
    return load_reference_state_dict(model, state_dict, strict, yolox_key_map(model))


def fold_deconv_bn(weight, conv_bias, gamma, beta, mean, var, eps=BN_EPS):
    """`fold_conv_bn` behind a ConvTranspose2d: its weight is [Cin, Cout, kh, kw], so the scale goes to dimension 1."""
    w = weight.double()
    scale = gamma.double() / torch.sqrt(var.double() + eps)
    shift = beta.double() - mean.double() * scale
    if conv_bias is not None:
        shift = shift + conv_bias.double() * scale
    return w * scale.view(1, -1, *([1] * (w.dim() - 2))), shift


def fold_conv_bn(weight, conv_bias, gamma, beta, mean, var, eps=BN_EPS):
    """Frozen BatchNorm behind a convolution as the convolution's own scale and shift (float64)."""
    w = weight.double()
    scale = gamma.double() / torch.sqrt(var.double() + eps)
    shift = beta.double() - mean.double() * scale
    if conv_bias is not None:
        shift = shift + conv_bias.double() * scale
    return w * scale.view(-1, *([1] * (w.dim() - 1))), shift


def load_centernet_state_dict(model, state_dict, strict=True):
    """`load_reference_state_dict` for centernet.CenterNet and mmdet's CenterNet checkpoint (`centernet_key_map`)."""
    return load_reference_state_dict(model, state_dict, strict, centernet_key_map(model))


def load_reference_state_dict(model, state_dict, strict=True, key_map=None):
    """Fill `model` (bevformer.BEVFormer, or another model with its `key_map`) from a reference checkpoint's state
    dict (the value of its "state_dict" entry, or the dict itself).  Returns (missing, unexpected): our parameters that found
    no source, and reference tensors nothing asked for (BN `num_batches_tracked` and the head's
    `code_weights` buffer are expected leftovers and not reported).  strict: raise on either."""
    sd = state_dict.get("state_dict", state_dict)
    kmap = reference_key_map(model) if key_map is None else key_map
    own = dict(model.named_parameters())
    used, missing = set(), []
    with torch.no_grad():
        for name, p in own.items():
            src = kmap.get(name)
            if src is None:
                missing.append(name)
                continue
            if isinstance(src, tuple):
                tag, conv, bn = src
                keys = [conv + ".weight", bn + ".weight", bn + ".bias", bn + ".running_mean", bn + ".running_var"]
                if any(k not in sd for k in keys):
                    missing.append(name)
                    continue
                fold = fold_deconv_bn if tag == "deconv_bn" else fold_conv_bn
                eps = YOLOX_BN_EPS if tag == "conv_bn_yolox" else BN_EPS
                w, b = fold(sd[keys[0]], sd.get(conv + ".bias"), *(sd[k] for k in keys[1:]), eps=eps)
                used.update(keys)
                if conv + ".bias" in sd:
                    used.add(conv + ".bias")
                val = w if name.endswith(".weight") else b
            else:
                if src not in sd:
                    missing.append(name)
                    continue
                used.add(src)
                val = sd[src]
            if name == "level_embeds" and val.dim() == 2 and val.shape[0] > p.shape[0] and val.shape[1:] == p.shape[1:]:
                # tiny / small configs never pass num_feature_levels, so PerceptionTransformer allocates its default
                # 4 rows (modules/transformer.py:15,55) although only level_embeds[lvl] for lvl < the FPN's levels is
                # ever read (:313-321): take the rows that are used
                val = val[:p.shape[0]]
            if tuple(val.shape) != tuple(p.shape):
                raise ValueError(f"{name}: shape {tuple(p.shape)} vs reference {tuple(val.shape)}")
            p.copy_(val.to(p.dtype))
    ignorable = ("num_batches_tracked", "code_weights")
    unexpected = sorted(k for k in sd if k not in used and not k.endswith(ignorable))
    if strict and (missing or unexpected):
        raise KeyError(f"missing {missing[:8]}{'...' if len(missing) > 8 else ''}; "
                       f"unexpected {unexpected[:8]}{'...' if len(unexpected) > 8 else ''}")
    model._static = None          # cached geometry / packed weights are rebuilt on the next frame
    return missing, unexpected


def depthnet_key_map(depth_net, prefix="img_view_transformer.depth_net."):
    """`reference_key_map` for bevdepth.DepthNet: {our parameter name: source} from the names the reference's classes
    spell (view_transformer.py: DepthNet, mmdet's BasicBlock, ASPP / _ASPPModule, Mlp, SELayer) under `prefix`.  Every
    BatchNorm2d is folded into the convolution in front of it; the BatchNorm1d of the camera inputs stays a module
    (its running statistics are buffers: `load_depthnet_state_dict` copies them)."""
    m = {}

    def fold(ours, conv, bn):
        m[ours + ".weight"] = m[ours + ".bias"] = _conv_bn(prefix + conv, prefix + bn)

    def copy(name):
        for n in ("weight", "bias"):
            m[f"{name}.{n}"] = f"{prefix}{name}.{n}"

    fold("reduce_conv", "reduce_conv.0", "reduce_conv.1")
    for name in ("context_conv", "bn"):
        copy(name)
    for br in ("depth", "context"):
        for name in (f"{br}_mlp.fc1", f"{br}_mlp.fc2", f"{br}_se.conv_reduce", f"{br}_se.conv_expand"):
            copy(name)
    for i in range(3):
        fold(f"depth_conv.{i}.conv1", f"depth_conv.{i}.conv1", f"depth_conv.{i}.bn1")
        fold(f"depth_conv.{i}.conv2", f"depth_conv.{i}.conv2", f"depth_conv.{i}.bn2")
    last = 3
    if depth_net.use_aspp:
        for k in (1, 2, 3, 4):
            fold(f"depth_conv.3.aspp{k}", f"depth_conv.3.aspp{k}.atrous_conv", f"depth_conv.3.aspp{k}.bn")
        fold("depth_conv.3.global_avg_pool", "depth_conv.3.global_avg_pool.1", "depth_conv.3.global_avg_pool.2")
        fold("depth_conv.3.conv1", "depth_conv.3.conv1", "depth_conv.3.bn1")
        last = 4
    if getattr(depth_net, "use_dcn", False):      # mmcv's DCN pack: weight (no bias) and conv_offset, no BatchNorm behind it
        m[f"depth_conv.{last}.weight"] = f"{prefix}depth_conv.{last}.weight"
        copy(f"depth_conv.{last}.conv_offset")
        last += 1
    copy(f"depth_conv.{last}")
    if getattr(depth_net, "stereo", False):       # BEVStereo: two stride-2 convolutions with their BatchNorms, a biased 1 x 1
        fold("cost_volumn_net.0", "cost_volumn_net.0", "cost_volumn_net.1")
        fold("cost_volumn_net.1", "cost_volumn_net.2", "cost_volumn_net.3")
        copy("depth_conv.0.downsample")
    return m


def depthnet_reference_keys(depth_net, prefix="img_view_transformer.depth_net."):
    """Every tensor name a reference checkpoint holds for this DepthNet (num_batches_tracked left out), sorted."""
    keys = set()
    for src in depthnet_key_map(depth_net, prefix).values():
        if isinstance(src, tuple):
            _, conv, bn = src
            keys.update([conv + ".weight"] + [f"{bn}.{n}" for n in ("weight", "bias", "running_mean", "running_var")])
            if conv.endswith("reduce_conv.0") or "cost_volumn_net." in conv:
                keys.add(conv + ".bias")          # (the only folded convolutions that have a bias of their own)
        else:
            keys.add(src)
    keys.update(f"{prefix}bn.{n}" for n in ("running_mean", "running_var"))
    return sorted(keys)


def load_depthnet_state_dict(depth_net, state_dict, strict=True, prefix="img_view_transformer.depth_net."):
    """Fill a bevdepth.DepthNet from a reference checkpoint's state dict: `depthnet_key_map`, plus the running
    statistics of the BatchNorm1d.  Returns (missing, unexpected) among the keys under `prefix`."""
    sd = state_dict.get("state_dict", state_dict)
    sd = {k: v for k, v in sd.items() if k.startswith(prefix)}
    missing, unexpected = load_reference_state_dict(depth_net, sd, False, depthnet_key_map(depth_net, prefix))
    with torch.no_grad():
        for n in ("running_mean", "running_var"):
            k = f"{prefix}bn.{n}"
            if k in sd:
                getattr(depth_net.bn, n).copy_(sd[k].to(getattr(depth_net.bn, n).dtype))
                unexpected.remove(k)
            else:
                missing.append("bn." + n)
    if strict and (missing or unexpected):
        raise KeyError(f"missing {missing[:8]}; unexpected {unexpected[:8]}")
    return missing, unexpected
