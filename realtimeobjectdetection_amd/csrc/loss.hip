// The reference's YOLO training loss, forward value only: targets from ground-truth boxes and the five-term sum of squares.
//
// Replaces DarknetTrainer.target_creator / target_layer / anchor_fit (reference: train.py:129-209) with xywh2YOLO and bbox_iou_wh
// (src/util.py:48-75, 156-172), a Python loop over boxes that fills a dense [B,N,5+C] target on the host, and
// DarknetTrainer.darknet_loss (train.py:211-230).  The reference's behaviour is kept as it is, quirks included:
// only boxes whose class-0 slot is 1 and whose w, h are not below min_box_size pass; anchor_fit compares the box with a SQUARE of
// the anchor's width (bbox_iou_wh reads wh2[0] twice), first maximum wins; target slot 0 holds the y fraction and slot 1 the x
// fraction; of two boxes of an image on one (cell, anchor) the later one wins.  A box whose cell lies outside the grid is skipped
// and sets status bit 0 (the reference wraps into the next grid row or raises).
//
// Arithmetic parity: anchor_fit, the cell and the centre fractions are Python doubles in the reference, so this file is compiled
// like nms.hip / match.hip (-ffp-contract=off, correctly rounded fp32 division): one rounding per operation, no FMA.
//
// Launch sequence of rtod_yolo_loss (enqueue only; kernel boundaries order the phases, nothing is handed over inside a launch):
//   memset    owner[B][N] = -1 (all bytes 0xFF), n_obj = 0
//   assign    one workgroup per image, a thread per box: filters, per head anchor_fit, cell, row; integer atomicMax of the box
//             index into owner[b][row] ("the later box wins" is "the larger index wins", whatever the arrival order)
//   reduce    LOSS_ROWS rows of one image per workgroup.  A row without owner reads p4 only; an owned row is read by its wave
//             (lane <-> column) against the owning box's row, whose four coordinates are recomputed from the box.  Five double
//             accumulators per lane, fixed shuffle tree, waves added in order: one partial [5] per workgroup, plain stores
//   finalize  one wave: the partials of an image added in a fixed order, then the images in order.  No floating-point atomics,
//             so the six doubles are bit-identical from call to call
//   dense     (optional) target [B,N,5+C] and mask [B,N] from the owner map: zero fill and scatter in one pass
// rtod_darknet_loss_dense runs reduce + finalize on a caller's dense target / mask instead (darknet_loss's own signature).
// The head table and the target arithmetic of one box live in loss_common.h: loss_grad.hip (the gradient) shares them and enters
// the memset / assign / reduce / finalize sequence through enqueue_loss_core.
#include "loss_common.h"

namespace rtod {

static int64_t loss_blocks(int64_t rows) { return (rows + LOSS_ROWS - 1) / LOSS_ROWS; }

size_t yolo_loss_workspace_bytes(int batch, int n_rows) {
    const size_t partials = sizeof(double) * 5 * (size_t)batch * (size_t)loss_blocks(n_rows);
    return (partials + sizeof(int32_t) * (size_t)batch * n_rows + 15) & ~(size_t)15;
}

__global__ __launch_bounds__(LOSS_BLOCK)
void loss_assign_kernel(const float* __restrict__ boxes, const int32_t* __restrict__ box_off, int N, int attrs, LossHeads H,
                        float min_box, int32_t* __restrict__ owner, int32_t* __restrict__ status) {
    const int b = blockIdx.x;
    const int t0 = box_off[b], t1 = box_off[b + 1];
    if (t0 < 0 || t1 < t0) { if (threadIdx.x == 0) atomicOr(status, 2); return; }
    int32_t* own = owner + (int64_t)b * N;
    bool outside = false;
    for (int i = t0 + (int)threadIdx.x; i < t1; i += LOSS_BLOCK) {
        const float* bx = boxes + (int64_t)i * attrs;
        if (bx[5] != 1.0f) continue;                                 // box[5] != 1: only class 0 passes (train.py:181)
        const float w = bx[2], hh = bx[3];
        if (w < min_box || hh < min_box) continue;                   // train.py:183
        for (int h = 0; h < H.n; ++h) {
            const int a = anchor_fit((double)w, (double)hh, H.aw[h], H.na[h]);
            int gx, gy; double fx, fy;
            if (!box_cell(bx[0], bx[1], H.stride[h], H.gw[h], H.gh[h], gx, gy, fx, fy)) { outside = true; continue; }
            const int n = (gy * H.gw[h] + gx) * H.na[h] + a;         // < gh * gw * na = off[h + 1] - off[h]
            atomicMax(own + H.off[h] + n, i);
        }
    }
    if (outside) atomicOr(status, 1);
}

// DENSE: target / mask are the caller's tensors; else owner map + box list.  grid (blocks of an image, images); N rows per image.
template <bool DENSE>
__global__ __launch_bounds__(LOSS_BLOCK)
void loss_reduce_kernel(const float* __restrict__ pred, int64_t N, int attrs, const int32_t* __restrict__ owner,
                        const float* __restrict__ boxes, LossHeads H, const float* __restrict__ target, const uint8_t* __restrict__ mask,
                        double* __restrict__ partials, int32_t* __restrict__ n_obj) {
    __shared__ double s_part[LOSS_WAVES][5];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.y;
    const int64_t img = (int64_t)b * N;
    const int64_t row0 = (int64_t)blockIdx.x * LOSS_ROWS + wave * (LOSS_ROWS / LOSS_WAVES);
    double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};                      // xy, wh, obj, noobj, cls
    int cnt = 0;
    for (int it = 0; it < LOSS_ROWS / LOSS_WAVES / 64; ++it) {
        const int64_t base = row0 + it * 64;
        if (base >= N) break;                                        // uniform over the wave
        const int64_t r = base + lane;
        const bool valid = r < N;
        int own = -1;
        if (valid) own = DENSE ? (mask[img + r] ? 0 : -1) : owner[img + r];
        if (valid && own < 0) {
            const float p4 = pred[(img + r) * attrs + 4];
            const float t4 = DENSE ? target[(img + r) * attrs + 4] : 0.0f;
            const double d = (double)p4 - (double)t4;
            acc[3] += d * d;
        }
        unsigned long long m = __ballot(valid && own >= 0);
        cnt += __popcll(m);
        while (m) {                                                  // owned rows in ascending order, the wave on one row
            const int j = __ffsll((long long)m) - 1;
            m &= m - 1;
            const int64_t g = img + base + j;
            const float* p = pred + g * attrs;
            const float* trow;
            float t4[4] = {0.f, 0.f, 0.f, 0.f};
            if (DENSE) trow = target + g * attrs;
            else {
                const int o = __shfl(own, j);
                trow = boxes + (int64_t)o * attrs;
                int a;
                const int h = head_of_row(H, (int)(base + j), a);
                target_xywh(H, h, a, trow, t4);
            }
            for (int c = lane; c < attrs; c += 64) {
                float t = trow[c];
                if (!DENSE && c < 4) t = c == 0 ? t4[0] : c == 1 ? t4[1] : c == 2 ? t4[2] : t4[3];
                const double d = (double)p[c] - (double)t;
                const double dd = d * d;
                if (c < 2) acc[0] += dd;
                else if (c < 4) acc[1] += dd;
                else if (c == 4) acc[2] += dd;
                else acc[4] += dd;
            }
        }
    }
#pragma unroll
    for (int q = 0; q < 5; ++q) {
        double v = acc[q];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
        if (lane == 0) s_part[wave][q] = v;
    }
    if (n_obj && lane == 0 && cnt) atomicAdd(n_obj + b, cnt);
    __syncthreads();
    if (tid < 5) {
        double v = s_part[0][tid];
        for (int w = 1; w < LOSS_WAVES; ++w) v += s_part[w][tid];
        partials[((int64_t)b * gridDim.x + blockIdx.x) * 5 + tid] = v;
    }
}

// One wave.  loss[6] = total, xy, wh, obj, noobj, cls; per_image [B][6] likewise (may be NULL).
__global__ __launch_bounds__(64)
void loss_finalize_kernel(const double* __restrict__ partials, int B, int64_t nblk, double* __restrict__ loss, double* __restrict__ per_image) {
    const int lane = threadIdx.x;
    const double wgt[5] = {5.0, 5.0, 1.0, 0.5, 1.0};
    double tot[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int b = 0; b < B; ++b) {
        const double* p = partials + (int64_t)b * nblk * 5;
        double img[5];
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            double v = 0.0;
            for (int64_t k = lane; k < nblk; k += 64) v += p[k * 5 + q];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
            img[q] = v;
            tot[q] += v;
        }
        if (per_image && lane == 0) {
            double* o = per_image + (int64_t)b * 6;
            double s = 0.0;
            for (int q = 0; q < 5; ++q) { const double v = wgt[q] * img[q]; o[1 + q] = v; s = q ? s + v : v; }
            o[0] = s;
        }
    }
    if (lane == 0) {
        double s = 0.0;
        for (int q = 0; q < 5; ++q) { const double v = wgt[q] * tot[q]; loss[1 + q] = v; s = q ? s + v : v; }   // train.py:220-229: the terms in this order
        loss[0] = s;
    }
}

__global__ __launch_bounds__(LOSS_BLOCK)
void loss_dense_kernel(const int32_t* __restrict__ owner, const float* __restrict__ boxes, int B, int N, int attrs, LossHeads H,
                       float* __restrict__ target, uint8_t* __restrict__ mask) {
    const int64_t total = (int64_t)B * N * attrs;
    for (int64_t t = blockIdx.x * (int64_t)LOSS_BLOCK + threadIdx.x; t < total; t += (int64_t)gridDim.x * LOSS_BLOCK) {
        const int64_t g = t / attrs;
        const int c = (int)(t - g * attrs);
        const int o = owner[g];
        float v = 0.0f;
        if (o >= 0 && target) {
            const float* bx = boxes + (int64_t)o * attrs;
            if (c < 4) {
                int a;
                const int h = head_of_row(H, (int)(g % N), a);
                float t4[4];
                target_xywh(H, h, a, bx, t4);
                v = c == 0 ? t4[0] : c == 1 ? t4[1] : c == 2 ? t4[2] : t4[3];
            } else v = bx[c];
        }
        if (target) target[t] = v;
        if (mask && c == 0) mask[g] = o >= 0 ? 1 : 0;
    }
}

int make_heads(const rtod_yolo_head* heads, int n_heads, int n_rows, LossHeads& H, const char* who) {
    if (n_heads < 1 || n_heads > LOSS_MAX_HEADS) { set_error("%s: %d heads outside 1..%d", who, n_heads, LOSS_MAX_HEADS); return RTOD_E_ARG; }
    H.n = n_heads;
    int64_t off = 0;
    for (int h = 0; h < LOSS_MAX_HEADS; ++h) {
        H.gh[h] = H.gw[h] = H.stride[h] = H.na[h] = 1;
        H.off[h] = H.off[h + 1] = 0;
        for (int a = 0; a < LOSS_MAX_ANCHORS; ++a) H.aw[h][a] = H.ah[h][a] = 1;
    }
    for (int h = 0; h < n_heads; ++h) {
        const rtod_yolo_head& q = heads[h];
        if (q.grid_h < 1 || q.grid_w < 1 || q.stride < 1 || q.n_anchors < 1 || q.n_anchors > LOSS_MAX_ANCHORS) {
            set_error("%s: head %d: grid %dx%d stride %d anchors %d (1..%d anchors, positive grid and stride)", who, h, q.grid_h, q.grid_w, q.stride, q.n_anchors, LOSS_MAX_ANCHORS);
            return RTOD_E_ARG;
        }
        for (int a = 0; a < q.n_anchors; ++a) {
            if (q.anchors[2 * a] < 1 || q.anchors[2 * a + 1] < 1) { set_error("%s: head %d: anchor %d is not positive", who, h, a); return RTOD_E_ARG; }
            H.aw[h][a] = q.anchors[2 * a]; H.ah[h][a] = q.anchors[2 * a + 1];
        }
        H.gh[h] = q.grid_h; H.gw[h] = q.grid_w; H.stride[h] = q.stride; H.na[h] = q.n_anchors;
        H.off[h] = (int)off;
        off += (int64_t)q.grid_h * q.grid_w * q.n_anchors;
        if (off > n_rows) break;
    }
    if (off != n_rows) { set_error("%s: the heads hold %lld rows, n_rows is %d", who, (long long)off, n_rows); return RTOD_E_ARG; }
    for (int h = n_heads; h <= LOSS_MAX_HEADS; ++h) H.off[h] = n_rows;
    return RTOD_OK;
}

int32_t* loss_owner_map(void* ws, int batch, int n_rows) {
    return (int32_t*)((double*)ws + 5 * (int64_t)batch * loss_blocks(n_rows));
}

int enqueue_loss_core(const float* pred, int batch, int n_rows, int attrs, const LossHeads& H, const float* boxes, const int32_t* box_off,
                      float min_box_size, double* loss, double* per_image, int32_t* n_obj, int32_t* status, void* ws, hipStream_t s) {
    const int64_t nblk = loss_blocks(n_rows);
    double* partials = (double*)ws;
    int32_t* owner = loss_owner_map(ws, batch, n_rows);
    RTOD_HIP(hipMemsetAsync(owner, 0xFF, sizeof(int32_t) * (size_t)batch * n_rows, s));
    if (n_obj) RTOD_HIP(hipMemsetAsync(n_obj, 0, sizeof(int32_t) * (size_t)batch, s));
    hipLaunchKernelGGL(loss_assign_kernel, dim3(batch), dim3(LOSS_BLOCK), 0, s, boxes, box_off, n_rows, attrs, H, min_box_size, owner, status);
    if (loss || n_obj)
        hipLaunchKernelGGL(loss_reduce_kernel<false>, dim3((unsigned)nblk, batch), dim3(LOSS_BLOCK), 0, s, pred, (int64_t)n_rows, attrs, owner, boxes, H,
                           (const float*)nullptr, (const uint8_t*)nullptr, partials, n_obj);
    if (loss) hipLaunchKernelGGL(loss_finalize_kernel, dim3(1), dim3(64), 0, s, partials, batch, nblk, loss, per_image);
    return hip_fail(hipGetLastError(), "yolo_loss launch");
}

int launch_yolo_loss(const float* pred, int batch, int n_rows, int num_class, const rtod_yolo_head* heads, int n_heads,
                     const float* boxes, const int32_t* box_off, float min_box_size, double* loss, double* per_image,
                     float* target, uint8_t* mask, int32_t* n_obj, int32_t* status, void* ws, size_t ws_bytes, hipStream_t s) {
    if (!pred || !heads || !boxes || !box_off || !loss || !status || !ws) { set_error("yolo_loss: null pointer"); return RTOD_E_ARG; }
    if (batch < 1 || n_rows < 1 || num_class < 1) { set_error("yolo_loss: unsupported shape (batch=%d n_rows=%d num_class=%d)", batch, n_rows, num_class); return RTOD_E_ARG; }
    if ((int64_t)batch * n_rows > INT32_MAX) { set_error("yolo_loss: batch * n_rows exceeds 2^31 - 1"); return RTOD_E_ARG; }
    if (min_box_size != min_box_size) { set_error("yolo_loss: min_box_size is not a number"); return RTOD_E_ARG; }
    LossHeads H;
    if (int rc = make_heads(heads, n_heads, n_rows, H, "yolo_loss")) return rc;
    if (ws_bytes < yolo_loss_workspace_bytes(batch, n_rows)) { set_error("yolo_loss: workspace too small"); return RTOD_E_ARG; }
    if ((uintptr_t)ws & 7) { set_error("yolo_loss: workspace must be 8-byte aligned"); return RTOD_E_ARG; }
    const int attrs = 5 + num_class;
    if (int rc = enqueue_loss_core(pred, batch, n_rows, attrs, H, boxes, box_off, min_box_size, loss, per_image, n_obj, status, ws, s)) return rc;
    const int32_t* owner = loss_owner_map(ws, batch, n_rows);
    if (target || mask) {
        const int64_t total = (int64_t)batch * n_rows * attrs;
        const int64_t blocks = std::min<int64_t>((total + LOSS_BLOCK - 1) / LOSS_BLOCK, 4096);
        hipLaunchKernelGGL(loss_dense_kernel, dim3((unsigned)blocks), dim3(LOSS_BLOCK), 0, s, owner, boxes, batch, n_rows, attrs, H, target, mask);
    }
    return hip_fail(hipGetLastError(), "yolo_loss launch");
}

int launch_darknet_loss_dense(const float* pred, const float* target, const uint8_t* mask, int64_t rows, int attrs, double* loss,
                              void* ws, size_t ws_bytes, hipStream_t s) {
    if (!pred || !target || !mask || !loss || !ws) { set_error("darknet_loss_dense: null pointer"); return RTOD_E_ARG; }
    if (rows < 1 || attrs < 5) { set_error("darknet_loss_dense: unsupported shape (rows=%lld attrs=%d; attrs = 5 + classes)", (long long)rows, attrs); return RTOD_E_ARG; }
    const int64_t nblk = loss_blocks(rows);
    if (nblk > INT32_MAX) { set_error("darknet_loss_dense: too many rows"); return RTOD_E_ARG; }
    if (ws_bytes < sizeof(double) * 5 * (size_t)nblk) { set_error("darknet_loss_dense: workspace too small"); return RTOD_E_ARG; }
    if ((uintptr_t)ws & 7) { set_error("darknet_loss_dense: workspace must be 8-byte aligned"); return RTOD_E_ARG; }
    LossHeads H = {};
    double* partials = (double*)ws;
    hipLaunchKernelGGL(loss_reduce_kernel<true>, dim3((unsigned)nblk, 1), dim3(LOSS_BLOCK), 0, s, pred, rows, attrs, (const int32_t*)nullptr,
                       (const float*)nullptr, H, target, mask, partials, (int32_t*)nullptr);
    hipLaunchKernelGGL(loss_finalize_kernel, dim3(1), dim3(64), 0, s, partials, 1, nblk, loss, (double*)nullptr);
    return hip_fail(hipGetLastError(), "darknet_loss_dense launch");
}

}  // namespace rtod
