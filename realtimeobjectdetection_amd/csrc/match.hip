// Scoring detections against ground truth on the GPU: class / size filters, thresholded IoU matrix, greedy one-to-one matching,
// TP / FP / FN per image and over the batch.
//
// Replaces DarknetValidator.target_filter / pred_filter / compare_boxes / get_img_scores (reference: test.py:62-151, 182-208),
// which run a Python double loop with a host round trip per (prediction, target) pair and per matching step.  The counts are
// integer results of fp32 comparisons and must equal the reference's, so this file is compiled like nms.hip: -ffp-contract=off
// and correctly-rounded fp32 division (iou_ref.h).
//
// One launch, one workgroup of SCORE_BLOCK threads per image, no inter-workgroup communication:
//   filter   detection rows of the image whose class (column 7) is permitted, targets with w, h > min_box_size and a permitted
//            first arg-max class; both compacted in order (ballot + prefix over the waves), targets converted to corners in LDS
//   matrix   thread i owns kept prediction i: M[i][j] = iou if (double)iou > threshold else 0 for every kept target j, written to
//            the workspace ([target][prediction]: a column is one coalesced store) and reduced to the row's (maximum, FIRST column)
//   match    at most P_f rounds: block-wide arg-max over the rows' cached maxima (value desc, row asc: torch's first-occurrence
//            max / argmax), stop at 0; the winner's row and column die (the reference zeroes them, so dead entries count as 0);
//            only rows whose cached column died re-read their row of M.  One barrier per round (partials double-buffered).
// Results do not depend on the batch an image rides in; the only atomics are the integer adds into the totals and the status OR.
#include "rtod_internal.h"
#include "iou_ref.h"

namespace rtod {

constexpr int SCORE_BLOCK = 1024;              // one thread per kept prediction
constexpr int SCORE_MAX_PRED = SCORE_BLOCK;    // kept predictions per image
constexpr int SCORE_MAX_TGT = 256;             // kept targets per image (column index: 8 bits of the arg-max key)
constexpr int SCORE_MAX_CLASSES = 4096;        // what write_results accepts
constexpr int SCORE_WAVES = SCORE_BLOCK / 64;

struct ClassMask { uint32_t w[SCORE_MAX_CLASSES / 32]; };

void score_limits(int* max_pred, int* max_tgt) { *max_pred = SCORE_MAX_PRED; *max_tgt = SCORE_MAX_TGT; }

// floats between consecutive target columns of an image's matrix: the kept predictions an image can have, whole waves
static size_t score_ld(int cap) { return ((size_t)std::min(std::max(cap, 1), SCORE_MAX_PRED) + 63) & ~(size_t)63; }

size_t score_workspace_bytes(int batch, int cap, int max_targets) { return sizeof(float) * (size_t)batch * max_targets * score_ld(cap); }

__device__ __forceinline__ bool class_permitted(const ClassMask& m, int c) { return (m.w[c >> 5] >> (c & 31)) & 1u; }

// Order-preserving compaction step of one chunk of SCORE_BLOCK items: returns the place of this thread's item among the kept
// ones so far (valid where keep), advances `base` by the chunk's kept items.  s_cnt: [SCORE_WAVES] scratch.
__device__ __forceinline__ int compact_place(bool keep, int& base, int* s_cnt, int lane, int wave) {
    const unsigned long long m = __ballot(keep);
    if (lane == 0) s_cnt[wave] = __popcll(m);
    __syncthreads();
    int before = 0, total = 0;
    for (int q = 0; q < SCORE_WAVES; ++q) { const int v = s_cnt[q]; if (q < wave) before += v; total += v; }
    const int place = base + before + __popcll(m & ((1ull << lane) - 1));
    base += total;
    __syncthreads();                               // s_cnt is free again
    return place;
}

__global__ __launch_bounds__(SCORE_BLOCK)
void score_detections_kernel(const float* __restrict__ det, const int32_t* __restrict__ counts, int cap, int batch,
                             const float* __restrict__ tgt, const int32_t* __restrict__ tgt_off, int num_class, ClassMask mask,
                             float min_box, double thr, int max_tgt, int corners, int ld, int32_t* __restrict__ scores, int32_t* __restrict__ totals,
                             int32_t* __restrict__ match, float* __restrict__ match_iou, int32_t* __restrict__ status, float* __restrict__ ws) {
    __shared__ f32x4 s_tbox[SCORE_MAX_TGT];        // kept targets, corners
    __shared__ int s_tidx[SCORE_MAX_TGT];          // ... their index in the image's unfiltered list
    __shared__ int s_pidx[SCORE_MAX_PRED];         // kept predictions: row within the image
    __shared__ uint8_t s_coldead[SCORE_MAX_TGT];
    __shared__ int s_cnt[SCORE_WAVES];
    __shared__ float s_rv[2][SCORE_WAVES];         // per-wave arg-max partials, double-buffered over the rounds
    __shared__ int s_rk[2][SCORE_WAVES];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    int32_t* sc = scores + 4 * b;

    // rows of this image; counts that do not fit the buffer are answered like counts[0] > cap: nothing is read beyond cap rows
    const int D = counts[0];
    int64_t start = 0;
    bool bad = D > cap || D < 0;
    for (int i = 0; i <= b; ++i) { const int v = counts[2 + i]; if (v < 0) bad = true; if (i < b) start += v; }
    const int nd = counts[2 + b];
    if (bad || start + nd > cap) {
        if (tid < 4) sc[tid] = -1;
        if (tid == 0) atomicOr(status, 1);
        return;
    }
    const float* rows = det + start * 8;

    // ---- prediction filter: pred[i, -1] in permitted_classes (test.py:94-104), order kept
    int P = 0;
    for (int c0 = 0; c0 < nd; c0 += SCORE_BLOCK) {
        const int r = c0 + tid;
        bool keep = false;
        if (r < nd) {
            const float c = rows[(int64_t)r * 8 + 7];
            if (c >= 0.0f && c < (float)num_class) { const int ci = (int)c; keep = (float)ci == c && class_permitted(mask, ci); }
            if (match) match[start + r] = keep ? -1 : -2;
            if (match_iou) match_iou[start + r] = 0.0f;
        }
        const int place = compact_place(keep, P, s_cnt, lane, wave);
        if (keep && place < SCORE_MAX_PRED) s_pidx[place] = r;
    }
    // ---- target filter: w, h > min_box_size (strict, fp32), FIRST arg-max class permitted (test.py:73-81); xywh2xyxy (src/util.py:39-43)
    const int t0 = tgt_off[b], nt = tgt_off[b + 1] - t0;
    const int attrs = 5 + num_class;
    int T = 0;
    for (int c0 = 0; c0 < nt; c0 += SCORE_BLOCK) {
        const int r = c0 + tid;
        bool keep = false;
        f32x4 box = {0.f, 0.f, 0.f, 0.f};
        if (r < nt) {
            const float* t = tgt + (int64_t)(t0 + r) * attrs;
            const float cx = t[0], cy = t[1], w = t[2], h = t[3];
            if (w > min_box && h > min_box) {
                float best = t[5]; int bi = 0;
                for (int c = 1; c < num_class; ++c) { const float v = t[5 + c]; if (v > best) { best = v; bi = c; } }
                keep = class_permitted(mask, bi);
            }
            const float hw = w / 2.0f, hh = h / 2.0f;
            box = corners ? f32x4{cx, cy, w, h} : f32x4{cx - hw, cy - hh, cx + hw, cy + hh};
        }
        const int place = compact_place(keep, T, s_cnt, lane, wave);
        if (keep && place < max_tgt) { s_tbox[place] = box; s_tidx[place] = r; }
    }
    if (tid < SCORE_MAX_TGT) s_coldead[tid] = 0;
    __syncthreads();
    if (P > SCORE_MAX_PRED || T > max_tgt) {
        if (tid < 4) sc[tid] = -1;
        if (tid == 0) atomicOr(status, 2);
        return;
    }

    // ---- thresholded IoU matrix: iou.item() > threshold is a double compare of the float32 value (test.py:143-147)
    const bool have = tid < P;
    float* M = ws + (int64_t)b * max_tgt * ld + tid;          // M[j * ld]: this thread's row, column j (tid < P <= ld)
    const int prow = have ? s_pidx[tid] : 0;
    float val = -INFINITY; int col = 0;
    if (have && T > 0) {
        const float* p = rows + (int64_t)prow * 8;
        const f32x4 pb = {p[1], p[2], p[3], p[4]};
        for (int j = 0; j < T; ++j) {
            const float iou = iou_ref(pb, s_tbox[j]);
            const float v = (double)iou > thr ? iou : 0.0f;
            M[(int64_t)j * ld] = v;
            if (v > val) { val = v; col = j; }                   // first maximum
        }
    }

    // ---- greedy matching (test.py:126-137)
    int tp = 0, mcol = -1;
    float miou = 0.0f;
    bool dead = false;
    const int rounds = T > 0 ? P : 0;
    const int nwaves = (P + 63) >> 6;
    for (int it = 0; it < rounds; ++it) {
        float v = val; int k = (tid << 8) | col;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float ov = __shfl_xor(v, off); const int ok = __shfl_xor(k, off);
            if (ov > v || (ov == v && ok < k)) { v = ov; k = ok; }
        }
        const int par = it & 1;
        if (lane == 0) { s_rv[par][wave] = v; s_rk[par][wave] = k; }
        __syncthreads();
        v = s_rv[par][0]; k = s_rk[par][0];
        for (int q = 1; q < nwaves; ++q) { const float ov = s_rv[par][q]; const int ok = s_rk[par][q]; if (ov > v || (ov == v && ok < k)) { v = ov; k = ok; } }
        if (v == 0.0f) break;                                    // torch.max(box_ious) == 0
        const int wi = k >> 8, wj = k & 255;
        ++tp;
        if (tid == wi) { mcol = wj; miou = val; dead = true; val = 0.0f; col = 0; }   // the row is zeroed
        if (tid == 0) s_coldead[wj] = 1;                         // read from the next round on (this round's readers skip wj themselves)
        if (have && !dead && (col == wj || val < 0.0f)) {        // the column is zeroed: rows whose maximum sat there look again
            val = -INFINITY; col = 0;
            for (int j = 0; j < T; ++j) {
                const float e = (j == wj || s_coldead[j]) ? 0.0f : M[(int64_t)j * ld];
                if (e > val) { val = e; col = j; }
            }
        }
    }

    // ---- scores: one formula for the four branches of get_img_scores (test.py:182-208)
    if (have && mcol >= 0) {
        if (match) match[start + prow] = s_tidx[mcol];
        if (match_iou) match_iou[start + prow] = miou;
    }
    if (tid == 0) {
        const int s4[4] = {T, tp, P - tp, T - tp};
        for (int q = 0; q < 4; ++q) { sc[q] = s4[q]; if (totals) atomicAdd(totals + q, s4[q]); }
    }
}

int launch_score_detections(const float* det, const int32_t* counts, int cap, int batch, const float* tgt, const int32_t* tgt_off,
                            int num_class, const uint32_t* class_mask, float min_box_size, double iou_threshold, int max_targets, int target_corners,
                            int32_t* scores, int32_t* totals, int32_t* match, float* match_iou, int32_t* status,
                            void* ws, size_t ws_bytes, hipStream_t s) {
    if (!det || !counts || !tgt || !tgt_off || !class_mask || !scores || !status || !ws) { set_error("score_detections: null pointer"); return RTOD_E_ARG; }
    if (batch < 1 || cap < 0) { set_error("score_detections: unsupported shape (batch=%d cap=%d)", batch, cap); return RTOD_E_ARG; }
    if (num_class < 1 || num_class > SCORE_MAX_CLASSES) { set_error("score_detections: unsupported number of classes (%d)", num_class); return RTOD_E_ARG; }
    if (max_targets < 1 || max_targets > SCORE_MAX_TGT) { set_error("score_detections: max_targets_per_image %d outside 1..%d", max_targets, SCORE_MAX_TGT); return RTOD_E_ARG; }
    if (iou_threshold != iou_threshold) { set_error("score_detections: iou_threshold is not a number"); return RTOD_E_ARG; }
    if (ws_bytes < score_workspace_bytes(batch, cap, max_targets)) { set_error("score_detections: workspace too small"); return RTOD_E_ARG; }
    if (((uintptr_t)ws & 15) || ((uintptr_t)det & 15)) { set_error("score_detections: workspace/detections must be 16-byte aligned"); return RTOD_E_ARG; }
    ClassMask m;
    const int words = (num_class + 31) / 32;
    for (int i = 0; i < SCORE_MAX_CLASSES / 32; ++i) m.w[i] = i < words ? class_mask[i] : 0u;
    hipLaunchKernelGGL(score_detections_kernel, dim3(batch), dim3(SCORE_BLOCK), 0, s, det, counts, cap, batch, tgt, tgt_off, num_class, m,
                       min_box_size, iou_threshold, max_targets, target_corners ? 1 : 0, (int)score_ld(cap), scores, totals, match, match_iou, status, (float*)ws);
    return hip_fail(hipGetLastError(), "score_detections launch");
}

}  // namespace rtod
