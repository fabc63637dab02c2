// 2-D detection decode on the device: CenterNetHead.get_bboxes / decode_heatmap, YOLOXHead.get_bboxes up to the NMS
// (_bbox_decode, score and label).  The statement is the published algorithm of mmdet 2.x, read against how the
// reference calls it (det2trt/models/detector/{centernet,yolox}.py: post_process, rescale=True); parity with the
// library itself is unpinned (design/postprocess.md).  Fixed-capacity outputs, no host round trip, no launch sized by a
// device value: every entry can be captured.
//
// bevops_centernet_decode, two launches:
//   1. partial: block (x, b) takes kCnChunk cells of item b's C x H x W map, applies the local-maximum test while it
//      reads (each cell and its window once; the thinned values of the chunk live in LDS as 32-bit ranking keys, so
//      the radix passes of topk.h re-read LDS, not the window), and writes the top k of its chunk to the workspace.
//   2. decode: one block per item selects the top k among the partial winners, sorts, gathers wh / offset at the
//      winning cells and writes the boxes.
//   A constant map ties every key; the flat index in the key's low half then decides, chunk by chunk and again in
//   launch 2, so the first k flat indices come out.
// bevops_yolox_decode, one launch: one thread per (item, prior), level found by comparing the prior number with the
//   level offsets (unrolled over the 8 possible levels: no runtime-indexed argument array).
// The NMS behind both, bevops_box_nms, is the box instantiation of the pipeline in csrc/nms.hip.  The selection is
// csrc/topk.h; the partial-selection kernel, the emit routine and the entries' common checks are csrc/detect.h.
// No atomics apart from the LDS histogram of topk.h, whose order is erased by a sort.
#include "detect.h"

namespace bevops {
namespace {

constexpr int kCnChunk = 8192;             // cells per block of the CenterNet partial selection (32 KiB of LDS keys)
constexpr int kCnMaxK = 4096;              // k of bevops_centernet_decode
constexpr long long kCnMaxCells = 1ll << 24;
constexpr int kCnMaxKernel = 7;            // local-maximum windows 1, 3, 5, 7
constexpr int kYxMaxLevels = 8;
constexpr int kYxThreads = 256;
constexpr long long kYxMaxPriors = 1ll << 24;

// ---------------------------------------------------------------------------------------------------- CenterNet
struct ChunkKeySrc {   // keys of a chunk whose 32-bit rank halves sit in LDS
  const unsigned *v;
  unsigned base;
  __device__ __forceinline__ u64 operator()(unsigned i) const { return ((u64)v[i] << 32) | (base + i); }
};

// Launch 1 (partial_topk_kernel of detect.h): a chunk of kCnChunk cells, thinned into LDS as 32-bit rank halves before
// the selection reads it.  radius = (kernel - 1) / 2.
template <typename T>
struct CnChunk {
  static constexpr int kChunk = kCnChunk;
  const T *heat;
  unsigned C, H, W;
  size_t cs, ps;
  int radius;
  __device__ __forceinline__ ChunkKeySrc prepare(char *lds, unsigned b, unsigned base, unsigned n) const {
    const unsigned hw = H * W;
    unsigned *vals = reinterpret_cast<unsigned *>(lds);
    const T *item = heat + (size_t)b * C * hw;
    for (unsigned i = threadIdx.x; i < n; i += kDecThreads) {
      const unsigned f = base + i;
      const unsigned c = f / hw, cell = f % hw;
      const int y = (int)(cell / W), x = (int)(cell % W);
      const T *plane = item + (size_t)c * cs;
      const float v = ld(plane, (size_t)cell * ps);
      const int y0 = max(y - radius, 0), y1 = min(y + radius, (int)H - 1);
      const int x0 = max(x - radius, 0), x1 = min(x + radius, (int)W - 1);
      bool keep = true;   // no cell of the window compares greater (a NaN never does)
      for (int yy = y0; yy <= y1; ++yy)
        for (int xx = x0; xx <= x1; ++xx) keep = keep && !(ld(plane, ((size_t)yy * W + (unsigned)xx) * ps) > v);
      vals[i] = rank_bits(keep ? v : 0.f);
    }
    __syncthreads();
    return ChunkKeySrc{vals, base};
  }
};

struct CnMaps {
  const void *wh, *off;
  int cs[2], ps[2];   // channel / pixel strides in elements of wh, offset
};
struct CnMeta {   // per-image host values of the call
  float rx, ry;
  int has_border, has_scale;
  float border[kD2MaxBatch][2];   // (x, y) = mmdet's border[2], border[0]
  ScaleTable scale;
};

// Launch 2: one block per item; the candidates are the partial winners in ws (nkeys per item).
template <typename T>
__global__ __launch_bounds__(kDecThreads) void centernet_decode_kernel(CnMaps m, const u64 *__restrict__ ws, unsigned nkeys,
                                                                        float *__restrict__ boxes, float *__restrict__ scores,
                                                                        int32_t *__restrict__ labels,
                                                                        int32_t *__restrict__ count, unsigned C, unsigned H,
                                                                        unsigned W, unsigned K, unsigned cap, int idx_bytes,
                                                                        CnMeta g, float score_threshold) {
  const unsigned b = blockIdx.x;
  const unsigned hw = H * W;
  const DecLds l = carve(det_smem, cap);
  const KeySrc src{ws + (size_t)b * nkeys};
  block_topk(src, nkeys, K, cap, idx_bytes, true, l);
  const T *wh = static_cast<const T *>(m.wh) + (size_t)b * 2 * hw;
  const T *off = static_cast<const T *>(m.off) + (size_t)b * 2 * hw;
  emit_ranked<4>(l, K, b, boxes, scores, labels, count,
                 [&](u64 key, unsigned idx, float *box, float &s, int &label) __attribute__((always_inline)) {
    if (idx >= C * hw) return false;   // (never, for r < K: k <= C H W; a sentinel must never become an address)
    s = rank_logit((unsigned)(key >> 32));
    label = (int)(idx / hw);
    const unsigned cell = idx % hw;
    const float col = (float)(cell % W), row = (float)(cell / W);
    const float w0 = ld(wh, (size_t)cell * m.ps[0]), w1 = ld(wh, (size_t)m.cs[0] + (size_t)cell * m.ps[0]);
    const float o0 = ld(off, (size_t)cell * m.ps[1]), o1 = ld(off, (size_t)m.cs[1] + (size_t)cell * m.ps[1]);
    // every step rounded on its own, as mmdet's tensor ops round it
    const float xs = add_rn(col, o0), ys = add_rn(row, o1);
    const float hx = mul_rn(w0, 0.5f), hy = mul_rn(w1, 0.5f);   // (wh / 2, exact either way)
    box[0] = mul_rn(sub_rn(xs, hx), g.rx);
    box[1] = mul_rn(sub_rn(ys, hy), g.ry);
    box[2] = mul_rn(add_rn(xs, hx), g.rx);
    box[3] = mul_rn(add_rn(ys, hy), g.ry);
    if (g.has_border) {
#pragma unroll
      for (int c = 0; c < 4; ++c) box[c] = sub_rn(box[c], g.border[b][c & 1]);
    }
    if (g.has_scale) {
#pragma unroll
      for (int c = 0; c < 4; ++c) box[c] = box[c] / g.scale.v[b][c];
    }
    return score_threshold < 0.f || s > score_threshold;
  });
}

inline unsigned cn_blocks(long long total) { return (unsigned)((total + kCnChunk - 1) / kCnChunk); }

template <typename T>
int launch_centernet(const void *heat, const CnMaps &m, size_t hcs, size_t hps, float *boxes, float *scores,
                     int32_t *labels, int32_t *count, int batch, int C, int H, int W, int K, int kernel, const CnMeta &g,
                     float thr, void *workspace, hipStream_t st) {
  const unsigned total = (unsigned)(C * H * W);
  const int ib = index_bytes(total);
  const unsigned cap = pow2_at_least((unsigned)K);
  const size_t lds1 = lds_bytes(cap) + (size_t)kCnChunk * sizeof(unsigned), lds2 = lds_bytes(cap);
  const unsigned nblk = cn_blocks(total);
  u64 *ws = static_cast<u64 *>(workspace);
  const CnChunk<T> chunk{static_cast<const T *>(heat), (unsigned)C, (unsigned)H, (unsigned)W, hcs, hps, (kernel - 1) / 2};
  if (!ensure_dynamic_lds<partial_topk_kernel<CnChunk<T>>>(lds1)) return BEVOPS_FAILURE;
  if (!ensure_dynamic_lds<centernet_decode_kernel<T>>(lds2)) return BEVOPS_FAILURE;
  hipLaunchKernelGGL(partial_topk_kernel<CnChunk<T>>, dim3(nblk, (unsigned)batch), dim3(kDecThreads), lds1, st, chunk, ws,
                     total, (unsigned)K, cap, ib);
  if (hipGetLastError() != hipSuccess) return BEVOPS_FAILURE;
  hipLaunchKernelGGL(centernet_decode_kernel<T>, dim3((unsigned)batch), dim3(kDecThreads), lds2, st, m, ws,
                     nblk * (unsigned)K, boxes, scores, labels, count, (unsigned)C, (unsigned)H, (unsigned)W, (unsigned)K,
                     cap, ib, g, thr);
  return launch_status();
}

// ---------------------------------------------------------------------------------------------------- YOLOX
struct YxLevels {
  const void *cls[kYxMaxLevels], *bbox[kYxMaxLevels], *obj[kYxMaxLevels];
  unsigned start[kYxMaxLevels];   // first prior of the level
  int H[kYxMaxLevels], W[kYxMaxLevels], stride[kYxMaxLevels];
  int cs[kYxMaxLevels][3], ps[kYxMaxLevels][3];   // cls, bbox, obj
  int n;
};
struct YxScale {
  int on;
  ScaleTable s;
};

template <typename T>
__global__ __launch_bounds__(kYxThreads) void yolox_decode_kernel(YxLevels lv, YxScale sc, float *__restrict__ boxes,
                                                                   float *__restrict__ scores,
                                                                   int32_t *__restrict__ labels, unsigned P, unsigned C) {
  const unsigned p = blockIdx.x * (unsigned)kYxThreads + threadIdx.x, b = blockIdx.y;
  if (p >= P) return;
  // the level of prior p (levels ascend, so the last start at or below p wins); constant indices only
  const T *cls = nullptr, *bbox = nullptr, *obj = nullptr;
  unsigned start = 0;
  int H = 1, W = 1, stride = 1, ccs = 1, cps = 1, bcs = 1, bps = 1, ops = 1;
#pragma unroll
  for (int k = 0; k < kYxMaxLevels; ++k) {
    if (k < lv.n && p >= lv.start[k]) {
      cls = static_cast<const T *>(lv.cls[k]), bbox = static_cast<const T *>(lv.bbox[k]);
      obj = static_cast<const T *>(lv.obj[k]);
      start = lv.start[k], H = lv.H[k], W = lv.W[k], stride = lv.stride[k];
      ccs = lv.cs[k][0], cps = lv.ps[k][0], bcs = lv.cs[k][1], bps = lv.ps[k][1], ops = lv.ps[k][2];
    }
  }
  const unsigned cell = p - start, hw = (unsigned)(H * W);
  const unsigned row = cell / (unsigned)W, col = cell % (unsigned)W;
  const T *pc = cls + (size_t)b * C * hw + (size_t)cell * cps;
  const T *pb = bbox + (size_t)b * 4 * hw + (size_t)cell * bps;
  float best = ld(pc, 0);
  int label = 0;
  for (unsigned c = 1; c < C; ++c) {   // first maximum: ties go to the lower class
    const float v = ld(pc, (size_t)c * ccs);
    if (v > best) best = v, label = (int)c;
  }
  const float fs = (float)stride;
  const float p0 = ld(pb, 0), p1 = ld(pb, (size_t)bcs), p2 = ld(pb, 2 * (size_t)bcs), p3 = ld(pb, 3 * (size_t)bcs);
  const float cx = add_rn(mul_rn(p0, fs), (float)(col * (unsigned)stride));
  const float cy = add_rn(mul_rn(p1, fs), (float)(row * (unsigned)stride));
  const float hx = mul_rn(mul_rn(expf(p2), fs), 0.5f), hy = mul_rn(mul_rn(expf(p3), fs), 0.5f);
  float box[4] = {sub_rn(cx, hx), sub_rn(cy, hy), add_rn(cx, hx), add_rn(cy, hy)};
  if (sc.on) {
#pragma unroll
    for (int c = 0; c < 4; ++c) box[c] = box[c] / sc.s.v[b][c];
  }
  const float s = mul_rn(sigmoid_f32(ld(obj, (size_t)b * hw + (size_t)cell * ops)), sigmoid_f32(best));
  const size_t o = (size_t)b * P + p;
#pragma unroll
  for (int c = 0; c < 4; ++c) boxes[o * 4 + c] = box[c];
  scores[o] = s;
  labels[o] = label;
}

}  // namespace
}  // namespace bevops

using namespace bevops;

extern "C" size_t bevops_centernet_decode_workspace_size(int batch, int num_classes, int height, int width, int k) {
  if (batch < 1 || batch > kD2MaxBatch || num_classes < 1 || height < 1 || width < 1 || k < 1) return 0;
  const long long total = (long long)num_classes * height * width;
  if ((long long)num_classes * height > kCnMaxCells || total > kCnMaxCells || k > kCnMaxK || k > total) return 0;
  return (size_t)batch * cn_blocks(total) * (size_t)k * sizeof(u64);
}

extern "C" int bevops_centernet_decode(int dtype, const void *heatmap, const void *wh, const void *offset,
                                       const int32_t *strides_host, float *boxes, float *scores, int32_t *labels,
                                       int32_t *count, int batch, int num_classes, int map_h, int map_w, int k, int kernel,
                                       int inp_h, int inp_w, const float *border_host, const float *scale_factor_host,
                                       float score_threshold, void *workspace, size_t workspace_bytes, void *stream) {
  if (!heatmap || !wh || !offset || !strides_host || !boxes || !scores || !labels || !count) return BEVOPS_BAD_PARAM;
  if (batch < 1 || num_classes < 1 || map_h < 1 || map_w < 1 || inp_h < 1 || inp_w < 1 || kernel < 1)
    return BEVOPS_BAD_PARAM;
  if (const int st = dtype_status(dtype)) return st;
  if (score_threshold != score_threshold) return BEVOPS_BAD_PARAM;
  for (int i = 0; i < 6; ++i)
    if (strides_host[i] < 1) return BEVOPS_BAD_PARAM;
  const long long total = (long long)num_classes * map_h * map_w;
  if ((long long)num_classes * map_h > kCnMaxCells || total > kCnMaxCells || k < 1 || k > kCnMaxK || k > total ||
      batch > kD2MaxBatch || kernel > kCnMaxKernel || (kernel & 1) == 0)
    return BEVOPS_NOT_SUPPORTED;
  CnMeta g;
  g.rx = (float)((double)inp_w / map_w), g.ry = (float)((double)inp_h / map_h);
  g.has_border = border_host != nullptr, g.has_scale = scale_factor_host != nullptr;
  for (int i = 0; i < kD2MaxBatch * 2; ++i) g.border[i / 2][i % 2] = 0.f;
  for (int i = 0; border_host && i < batch * 2; ++i) {
    if (!finite_f(border_host[i])) return BEVOPS_BAD_PARAM;
    g.border[i / 2][i % 2] = border_host[i];
  }
  if (!fill_scale(g.scale, scale_factor_host, batch)) return BEVOPS_BAD_PARAM;
  const size_t need = bevops_centernet_decode_workspace_size(batch, num_classes, map_h, map_w, k);
  if (!workspace_ok(workspace, workspace_bytes, need)) return BEVOPS_BAD_PARAM;
  CnMaps m;
  m.wh = wh, m.off = offset;
  m.cs[0] = strides_host[2], m.ps[0] = strides_host[3], m.cs[1] = strides_host[4], m.ps[1] = strides_host[5];
  const hipStream_t st = static_cast<hipStream_t>(stream);
  if (dtype == BEVOPS_F32)
    return launch_centernet<float>(heatmap, m, (size_t)strides_host[0], (size_t)strides_host[1], boxes, scores, labels,
                                   count, batch, num_classes, map_h, map_w, k, kernel, g, score_threshold, workspace, st);
  return launch_centernet<__half>(heatmap, m, (size_t)strides_host[0], (size_t)strides_host[1], boxes, scores, labels,
                                  count, batch, num_classes, map_h, map_w, k, kernel, g, score_threshold, workspace, st);
}

extern "C" int bevops_yolox_decode(int dtype, const void *const *cls_host, const void *const *bbox_host,
                                   const void *const *obj_host, const int32_t *level_shapes_host,
                                   const int32_t *strides_host, float *boxes, float *scores, int32_t *labels, int batch,
                                   int num_levels, int num_classes, const float *scale_factor_host, void *stream) {
  if (!cls_host || !bbox_host || !obj_host || !level_shapes_host || !strides_host || !boxes || !scores || !labels)
    return BEVOPS_BAD_PARAM;
  if (batch < 1 || num_levels < 1 || num_classes < 1) return BEVOPS_BAD_PARAM;
  if (const int st = dtype_status(dtype)) return st;
  if (num_levels > kYxMaxLevels || batch > kD2MaxBatch) return BEVOPS_NOT_SUPPORTED;
  YxLevels lv;
  lv.n = num_levels;
  long long priors = 0;
  for (int k = 0; k < kYxMaxLevels; ++k) {
    lv.cls[k] = lv.bbox[k] = lv.obj[k] = nullptr;
    lv.start[k] = 0, lv.H[k] = lv.W[k] = lv.stride[k] = 1;
    for (int c = 0; c < 3; ++c) lv.cs[k][c] = lv.ps[k][c] = 1;
  }
  for (int k = 0; k < num_levels; ++k) {
    const int H = level_shapes_host[3 * k], W = level_shapes_host[3 * k + 1], s = level_shapes_host[3 * k + 2];
    if (!cls_host[k] || !bbox_host[k] || !obj_host[k] || H < 1 || W < 1 || s < 1) return BEVOPS_BAD_PARAM;
    for (int c = 0; c < 6; ++c)
      if (strides_host[6 * k + c] < 1) return BEVOPS_BAD_PARAM;
    if ((long long)H * W > kYxMaxPriors || (long long)(H > W ? H : W) * s > kYxMaxPriors) return BEVOPS_NOT_SUPPORTED;
    lv.cls[k] = cls_host[k], lv.bbox[k] = bbox_host[k], lv.obj[k] = obj_host[k];
    lv.start[k] = (unsigned)priors, lv.H[k] = H, lv.W[k] = W, lv.stride[k] = s;
    for (int c = 0; c < 3; ++c) lv.cs[k][c] = strides_host[6 * k + 2 * c], lv.ps[k][c] = strides_host[6 * k + 2 * c + 1];
    priors += (long long)H * W;
    if (priors > kYxMaxPriors) return BEVOPS_NOT_SUPPORTED;
  }
  YxScale sc;
  sc.on = scale_factor_host != nullptr;
  if (!fill_scale(sc.s, scale_factor_host, batch)) return BEVOPS_BAD_PARAM;
  const unsigned P = (unsigned)priors;
  const dim3 grid((P + kYxThreads - 1) / kYxThreads, (unsigned)batch);
  const hipStream_t st = static_cast<hipStream_t>(stream);
  if (dtype == BEVOPS_F32)
    hipLaunchKernelGGL(yolox_decode_kernel<float>, grid, dim3(kYxThreads), 0, st, lv, sc, boxes, scores, labels, P,
                       (unsigned)num_classes);
  else
    hipLaunchKernelGGL(yolox_decode_kernel<__half>, grid, dim3(kYxThreads), 0, st, lv, sc, boxes, scores, labels, P,
                       (unsigned)num_classes);
  return launch_status();
}
