// Detection decode on the device: NMSFreeCoder.decode_single (+ the z shift of BEVFormerHead.get_bboxes) and
// CenterHead.get_bboxes up to the NMS (sigmoid, exp(dim), CenterPointBBoxCoder.decode).  Reference:
//   third_party/bev_mmdet3d/core/bbox/coders/nms_free_coder.py:42-98, core/bbox/util.py:26-53,
//   third_party/bev_mmdet3d/models/dense_heads/bevformer_head.py:556, centerpoint_head.py:716-746,
//   third_party/bev_mmdet3d/core/bbox/coders/centerpoint_bbox_coders.py:61-230.
// Fixed-capacity outputs (boxes [batch, max_num, 9], scores, labels, count), kept rows compacted to the front in
// rank order, rows at and behind count[b] zero: no data-dependent shape, no host round trip, capturable.
//
// Ranking rule (include/bevops.h, design/postprocess.md): candidates rank by their fp32 LOGIT, larger first; equal
// logits (-0 counts as +0) rank by lower flat index first.  Both go into one 64-bit key,
//   key = (~monotone(logit) << 32) | flat_index,
// so "rank order" is ascending key order, all keys of one batch item are distinct, and the top max_num is a unique set.
//
// One block routine does the selection for both decoders: an 8-bit radix select over the 64-bit keys (the candidates
// are re-read per pass -- they sit in L2 -- so LDS holds only the winners), a collect of the max_num winners and a
// bitonic sort of them in LDS.  The LDS histogram uses integer atomics; counts do not depend on their order, and the
// order in which winners are collected is erased by the sort, so results are bit-reproducible.
// NMS-free: one launch, one block per batch item.  CenterPoint with more candidates than one block's chunk: every
// block selects the top max_num of its chunk into the caller's workspace, then one block per batch item selects among
// those, sorts, gathers the heads at the winning cells and decodes.
// Shared with csrc/decode2d.hip and csrc/nms.hip through csrc/detect.h: the typed loads, the partial-selection kernel,
// the emit routine behind the selection (compaction, row write, zero tail, count) and the host entries' common checks.
#include "detect.h"

namespace bevops {
namespace {

constexpr int kNmsFreeMaxCand = 16384;      // num_query * num_classes of bevops_nms_free_decode
constexpr int kMaxWinners = 16384;          // max_num of bevops_nms_free_decode: 128 KiB of keys in LDS
constexpr int kCpChunk = 4096;              // candidates per block of the CenterPoint partial selection
constexpr int kCpMaxWinners = 4096;         // max_num of bevops_centerpoint_decode

// key sources of block_topk: element i of the block's n candidates
template <typename T>
struct LogitSrc {   // logits at p[(i / inner) * outer_stride + (i % inner) * inner_stride], flat index base + i
  const T *p;
  unsigned base, inner;
  size_t outer_stride, inner_stride;
  __device__ __forceinline__ u64 operator()(unsigned i) const {
    const unsigned f = base + i;
    const size_t at = (size_t)(f / inner) * outer_stride + (size_t)(f % inner) * inner_stride;
    return ((u64)rank_bits(ld(p, at)) << 32) | f;
  }
};
struct Range6 {
  float v[6];
};
__device__ __forceinline__ bool in_range(float x, float y, float z, const Range6 &r) {
  return x >= r.v[0] && y >= r.v[1] && z >= r.v[2] && x <= r.v[3] && y <= r.v[4] && z <= r.v[5];
}
template <typename T>
__global__ __launch_bounds__(kDecThreads) void nms_free_decode_kernel(
    const T *__restrict__ cls, const T *__restrict__ bbox, float *__restrict__ boxes, float *__restrict__ scores,
    int32_t *__restrict__ labels, int32_t *__restrict__ count, unsigned num_query, unsigned num_classes, unsigned K,
    unsigned cap, int idx_bytes, Range6 range, float score_threshold, int bottom_center) {
  const unsigned b = blockIdx.x;
  const unsigned n = num_query * num_classes;
  const DecLds l = carve(det_smem, cap);
  const LogitSrc<T> src{cls + (size_t)b * n, 0u, n, 0, 1};
  block_topk(src, n, K, cap, idx_bytes, true, l);

  // score threshold with the reference's relaxation (nms_free_coder.py:67-75): scores descend with the rank, so
  // "nothing passes" is decided by rank 0 alone.  mode 0: score > thr, 1: score >= thr, 2: keep all.
  int mode = 2;
  float thr = 0.f;
  if (score_threshold >= 0.f) {
    const float top = sigmoid_f32(rank_logit((unsigned)(l.list[0] >> 32)));
    mode = 0;
    thr = score_threshold;
    if (!(top > thr)) {
      double tmp = (double)score_threshold;
      for (;;) {
        tmp *= 0.9;
        if (tmp < 0.01) {
          mode = 2;
          break;
        }
        thr = (float)tmp;
        mode = 1;
        if (top >= thr) break;
      }
    }
  }

  emit_ranked<9>(l, K, b, boxes, scores, labels, count,
                 [&](u64 key, unsigned idx, float *box, float &s, int &label) __attribute__((always_inline)) {
    if (idx >= n) return false;   // (never, for r < K: max_num <= n; a sentinel must never become an address)
    s = sigmoid_f32(rank_logit((unsigned)(key >> 32)));
    const unsigned q = idx / num_classes;
    label = (int)(idx % num_classes);
    const T *p = bbox + ((size_t)b * num_query + q) * 10;
    float v[10];
#pragma unroll
    for (int c = 0; c < 10; ++c) v[c] = ld(p, c);
    box[0] = v[0], box[1] = v[1], box[2] = v[4];
    box[3] = expf(v[2]), box[4] = expf(v[3]), box[5] = expf(v[5]);
    box[6] = atan2f(v[6], v[7]);
    box[7] = v[8], box[8] = v[9];
    const bool keep = in_range(box[0], box[1], box[2], range) && (mode == 2 || (mode == 0 ? s > thr : s >= thr));
    if (bottom_center) box[2] = sub_rn(box[2], mul_rn(box[5], 0.5f));
    return keep;
  });
}

// CenterPoint, first launch (partial_topk_kernel of detect.h): a chunk of kCpChunk cells of the heat map itself.
template <typename T>
struct CpChunk {
  static constexpr int kChunk = kCpChunk;
  const T *heat;
  unsigned hw, num_classes;
  size_t cs, ps, is;   // channel, pixel, batch-item stride in elements
  __device__ __forceinline__ LogitSrc<T> prepare(char *, unsigned b, unsigned base, unsigned) const {
    return LogitSrc<T>{heat + (size_t)b * is, base, hw, cs, ps};
  }
};

struct CpMaps {
  const void *reg, *height, *dim, *rot, *vel, *heat;
  int cs[6], ps[6];   // channel / pixel strides in elements, order reg, height, dim, rot, vel, heatmap
  long long is[6];    // batch-item strides in elements: channels * H * W for a map that is dense per item
};
struct CpGeom {
  float out_size_factor, voxel_x, voxel_y, pc_x, pc_y;
};

// CenterPoint, last launch: one block per batch item.  FROM_WS: the candidates are the partial winners in ws
// (nkeys per item), else the heat map itself.
template <typename T, bool FROM_WS>
__global__ __launch_bounds__(kDecThreads) void centerpoint_decode_kernel(
    CpMaps m, const u64 *__restrict__ ws, unsigned nkeys, float *__restrict__ boxes, float *__restrict__ scores,
    int32_t *__restrict__ labels, int32_t *__restrict__ count, unsigned num_classes, unsigned H, unsigned W, unsigned K,
    unsigned cap, int idx_bytes, CpGeom g, Range6 range, float score_threshold, int norm_bbox, int heat_is_score) {
  const unsigned b = blockIdx.x;
  const unsigned hw = H * W;
  const DecLds l = carve(det_smem, cap);
  if (FROM_WS) {
    const KeySrc src{ws + (size_t)b * nkeys};
    block_topk(src, nkeys, K, cap, idx_bytes, true, l);
  } else {
    const LogitSrc<T> src{static_cast<const T *>(m.heat) + (size_t)b * (size_t)m.is[5], 0u, hw, (size_t)m.cs[5],
                          (size_t)m.ps[5]};
    block_topk(src, num_classes * hw, K, cap, idx_bytes, true, l);
  }
  const T *reg = static_cast<const T *>(m.reg), *hei = static_cast<const T *>(m.height);
  const T *dim = static_cast<const T *>(m.dim), *rot = static_cast<const T *>(m.rot);
  const T *vel = static_cast<const T *>(m.vel);
  emit_ranked<9>(l, K, b, boxes, scores, labels, count,
                 [&](u64 key, unsigned idx, float *box, float &s, int &label) __attribute__((always_inline)) {
    if (idx >= num_classes * hw) return false;   // (never, for r < K; a sentinel must never become an address)
    s = rank_logit((unsigned)(key >> 32));
    if (!heat_is_score) s = sigmoid_f32(s);
    label = (int)(idx / hw);
    const unsigned cell = idx % hw;
    const float col = (float)(cell % W), row = (float)(cell / W);
    // channel c of a map at this cell
    auto at = [&](const T *p, int which, unsigned c) {
      return ld(p, (size_t)b * (size_t)m.is[which] + (size_t)c * m.cs[which] + (size_t)cell * m.ps[which]);
    };
    const float rx = reg ? at(reg, 0, 0) : 0.5f, ry = reg ? at(reg, 0, 1) : 0.5f;
    // (col + reg) * out_size_factor * voxel + pc_range, every step rounded as the reference's tensor ops round it
    box[0] = add_rn(mul_rn(mul_rn(add_rn(col, rx), g.out_size_factor), g.voxel_x), g.pc_x);
    box[1] = add_rn(mul_rn(mul_rn(add_rn(row, ry), g.out_size_factor), g.voxel_y), g.pc_y);
    box[2] = at(hei, 1, 0);
#pragma unroll
    for (unsigned c = 0; c < 3; ++c) {
      const float d = at(dim, 2, c);
      box[3 + c] = norm_bbox ? expf(d) : d;
    }
    box[6] = atan2f(at(rot, 3, 0), at(rot, 3, 1));
    box[7] = vel ? at(vel, 4, 0) : 0.f;
    box[8] = vel ? at(vel, 4, 1) : 0.f;
    return in_range(box[0], box[1], box[2], range) && (score_threshold < 0.f || s > score_threshold);
  });
}

inline unsigned cp_blocks(long long total) { return (unsigned)((total + kCpChunk - 1) / kCpChunk); }

template <typename T>
int launch_nms_free(const void *cls, const void *bbox, float *boxes, float *scores, int32_t *labels, int32_t *count,
                    int batch, int nq, int nc, int K, const Range6 &range, float thr, int bottom, hipStream_t st) {
  const unsigned cap = pow2_at_least((unsigned)K);
  const size_t lds = lds_bytes(cap);
  if (!ensure_dynamic_lds<nms_free_decode_kernel<T>>(lds)) return BEVOPS_FAILURE;
  hipLaunchKernelGGL(nms_free_decode_kernel<T>, dim3((unsigned)batch), dim3(kDecThreads), lds, st,
                     static_cast<const T *>(cls), static_cast<const T *>(bbox), boxes, scores, labels, count, (unsigned)nq,
                     (unsigned)nc, (unsigned)K, cap, index_bytes((unsigned)(nq * nc)), range, thr, bottom);
  return launch_status();
}

template <typename T>
int launch_centerpoint(const CpMaps &m, float *boxes, float *scores, int32_t *labels, int32_t *count, int batch, int nc,
                       int H, int W, int K, const CpGeom &g, const Range6 &range, float thr, int norm_bbox, int heat_is_score,
                       void *workspace, hipStream_t st) {
  const unsigned total = (unsigned)(nc * H * W), hw = (unsigned)(H * W);
  const int ib = index_bytes(total);
  const unsigned cap = pow2_at_least((unsigned)K);
  const size_t lds = lds_bytes(cap);
  if (total <= (unsigned)kCpChunk) {
    if (!ensure_dynamic_lds<centerpoint_decode_kernel<T, false>>(lds)) return BEVOPS_FAILURE;
    hipLaunchKernelGGL((centerpoint_decode_kernel<T, false>), dim3((unsigned)batch), dim3(kDecThreads), lds, st, m,
                       (const u64 *)nullptr, 0u, boxes, scores, labels, count, (unsigned)nc, (unsigned)H, (unsigned)W,
                       (unsigned)K, cap, ib, g, range, thr, norm_bbox, heat_is_score);
    return launch_status();
  }
  const unsigned nblk = cp_blocks(total);
  u64 *ws = static_cast<u64 *>(workspace);
  // K <= kCpMaxWinners = kCpChunk, so a slot holds K keys and the same LDS carve serves both launches
  const CpChunk<T> chunk{static_cast<const T *>(m.heat), hw, (unsigned)nc, (size_t)m.cs[5], (size_t)m.ps[5],
                           (size_t)m.is[5]};
  if (!ensure_dynamic_lds<partial_topk_kernel<CpChunk<T>>>(lds)) return BEVOPS_FAILURE;
  if (!ensure_dynamic_lds<centerpoint_decode_kernel<T, true>>(lds)) return BEVOPS_FAILURE;
  hipLaunchKernelGGL(partial_topk_kernel<CpChunk<T>>, dim3(nblk, (unsigned)batch), dim3(kDecThreads), lds, st, chunk, ws,
                     total, (unsigned)K, cap, ib);
  if (hipGetLastError() != hipSuccess) return BEVOPS_FAILURE;
  hipLaunchKernelGGL((centerpoint_decode_kernel<T, true>), dim3((unsigned)batch), dim3(kDecThreads), lds, st, m, ws,
                     nblk * (unsigned)K, boxes, scores, labels, count, (unsigned)nc, (unsigned)H, (unsigned)W, (unsigned)K,
                     cap, ib, g, range, thr, norm_bbox, heat_is_score);
  return launch_status();
}

}  // namespace
}  // namespace bevops

using namespace bevops;

extern "C" int bevops_nms_free_decode(int dtype, const void *cls_logits, const void *bbox_preds, float *boxes,
                                      float *scores, int32_t *labels, int32_t *count, int batch, int num_query,
                                      int num_classes, int max_num, const float *post_center_range_host,
                                      float score_threshold, int bottom_center, void *stream) {
  if (!cls_logits || !bbox_preds || !boxes || !scores || !labels || !count || !post_center_range_host)
    return BEVOPS_BAD_PARAM;
  if (batch < 1 || num_query < 1 || num_classes < 1 || max_num < 1) return BEVOPS_BAD_PARAM;
  if (const int st = dtype_status(dtype)) return st;
  const long long cand = (long long)num_query * num_classes;
  if (max_num > cand || !(score_threshold <= 3.0e38f)) return BEVOPS_BAD_PARAM;   // (NaN / inf: the relaxation needs a finite start)
  if (cand > kNmsFreeMaxCand || max_num > kMaxWinners || batch > 65535) return BEVOPS_NOT_SUPPORTED;
  Range6 range;
  for (int i = 0; i < 6; ++i) range.v[i] = post_center_range_host[i];
  const hipStream_t st = static_cast<hipStream_t>(stream);
  if (dtype == BEVOPS_F32)
    return launch_nms_free<float>(cls_logits, bbox_preds, boxes, scores, labels, count, batch, num_query, num_classes,
                                  max_num, range, score_threshold, bottom_center, st);
  return launch_nms_free<__half>(cls_logits, bbox_preds, boxes, scores, labels, count, batch, num_query, num_classes,
                                 max_num, range, score_threshold, bottom_center, st);
}

extern "C" size_t bevops_centerpoint_decode_workspace_size(int batch, int num_classes, int height, int width,
                                                           int max_num) {
  if (batch < 1 || num_classes < 1 || height < 1 || width < 1 || max_num < 1) return 0;
  const long long total = (long long)num_classes * height * width;
  if (total <= kCpChunk || max_num > kCpMaxWinners) return 0;
  return (size_t)batch * cp_blocks(total) * (size_t)max_num * sizeof(u64);
}

extern "C" int bevops_centerpoint_decode_ex(int dtype, const void *reg, const void *height, const void *dim,
                                            const void *rot, const void *vel, const void *heatmap,
                                            const int64_t *strides_host, float *boxes, float *scores, int32_t *labels,
                                            int32_t *count, int batch, int num_classes, int map_h, int map_w,
                                            int max_num, float out_size_factor, float voxel_x, float voxel_y, float pc_x,
                                            float pc_y, const float *post_center_range_host, float score_threshold,
                                            int norm_bbox, int heatmap_is_score, void *workspace, size_t workspace_bytes,
                                            void *stream) {
  if (!height || !dim || !rot || !heatmap || !strides_host || !boxes || !scores || !labels || !count ||
      !post_center_range_host)
    return BEVOPS_BAD_PARAM;
  if (batch < 1 || num_classes < 1 || map_h < 1 || map_w < 1 || max_num < 1) return BEVOPS_BAD_PARAM;
  if (const int st = dtype_status(dtype)) return st;
  const long long total = (long long)num_classes * map_h * map_w;
  if (max_num > total || score_threshold != score_threshold) return BEVOPS_BAD_PARAM;
  for (int i = 0; i < 18; ++i)
    if (strides_host[i] < 1 || (i % 3 != 2 && strides_host[i] > 0x7fffffffLL)) return BEVOPS_BAD_PARAM;
  if (total > 0x7fffffffLL || max_num > kCpMaxWinners || batch > 65535) return BEVOPS_NOT_SUPPORTED;
  const size_t need = bevops_centerpoint_decode_workspace_size(batch, num_classes, map_h, map_w, max_num);
  if (need && !workspace_ok(workspace, workspace_bytes, need)) return BEVOPS_BAD_PARAM;
  CpMaps m;
  m.reg = reg, m.height = height, m.dim = dim, m.rot = rot, m.vel = vel, m.heat = heatmap;
  for (int i = 0; i < 6; ++i)
    m.cs[i] = (int)strides_host[3 * i], m.ps[i] = (int)strides_host[3 * i + 1], m.is[i] = strides_host[3 * i + 2];
  const CpGeom g{out_size_factor, voxel_x, voxel_y, pc_x, pc_y};
  Range6 range;
  for (int i = 0; i < 6; ++i) range.v[i] = post_center_range_host[i];
  const hipStream_t st = static_cast<hipStream_t>(stream);
  if (dtype == BEVOPS_F32)
    return launch_centerpoint<float>(m, boxes, scores, labels, count, batch, num_classes, map_h, map_w, max_num, g,
                                     range, score_threshold, norm_bbox, heatmap_is_score, workspace, st);
  return launch_centerpoint<__half>(m, boxes, scores, labels, count, batch, num_classes, map_h, map_w, max_num, g, range,
                                    score_threshold, norm_bbox, heatmap_is_score, workspace, st);
}

extern "C" int bevops_centerpoint_decode(int dtype, const void *reg, const void *height, const void *dim,
                                         const void *rot, const void *vel, const void *heatmap,
                                         const int32_t *strides_host, float *boxes, float *scores, int32_t *labels,
                                         int32_t *count, int batch, int num_classes, int map_h, int map_w, int max_num,
                                         float out_size_factor, float voxel_x, float voxel_y, float pc_x, float pc_y,
                                         const float *post_center_range_host, float score_threshold, int norm_bbox,
                                         int heatmap_is_score, void *workspace, size_t workspace_bytes, void *stream) {
  if (!strides_host) return BEVOPS_BAD_PARAM;
  if (batch < 1 || num_classes < 1 || map_h < 1 || map_w < 1 || max_num < 1) return BEVOPS_BAD_PARAM;
  // every map dense per batch item: item stride = channels * H * W
  const long long chans[6] = {2, 1, 3, 2, 2, num_classes};
  int64_t ex[18];
  for (int i = 0; i < 6; ++i) {
    ex[3 * i] = strides_host[2 * i];
    ex[3 * i + 1] = strides_host[2 * i + 1];
    ex[3 * i + 2] = chans[i] * map_h * map_w;
  }
  return bevops_centerpoint_decode_ex(dtype, reg, height, dim, rot, vel, heatmap, ex, boxes, scores, labels, count,
                                      batch, num_classes, map_h, map_w, max_num, out_size_factor, voxel_x, voxel_y, pc_x,
                                      pc_y, post_center_range_host, score_threshold, norm_bbox, heatmap_is_score,
                                      workspace, workspace_bytes, stream);
}
