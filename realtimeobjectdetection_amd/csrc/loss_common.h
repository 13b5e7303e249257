// What loss.hip (the loss value) and loss_grad.hip (its gradient) share: the head table, the target arithmetic of one box and the
// host-side entry to the assignment phase.  Both files are compiled with the parity flags (-ffp-contract=off, correctly rounded
// fp32 division), so the device functions below round the same way in either.
#pragma once
#include "rtod_internal.h"

namespace rtod {

constexpr int LOSS_BLOCK = 256;
constexpr int LOSS_WAVES = LOSS_BLOCK / 64;
constexpr int LOSS_ROWS = 1024;                   // rows per workgroup of the reduce phase: 4 x 64 per wave
constexpr int LOSS_MAX_HEADS = 4;
constexpr int LOSS_MAX_ANCHORS = 8;

struct LossHeads {
    int n;
    int gh[LOSS_MAX_HEADS], gw[LOSS_MAX_HEADS], stride[LOSS_MAX_HEADS], na[LOSS_MAX_HEADS];
    int off[LOSS_MAX_HEADS + 1];                  // first row of each head; off[n] = N
    int aw[LOSS_MAX_HEADS][LOSS_MAX_ANCHORS], ah[LOSS_MAX_HEADS][LOSS_MAX_ANCHORS];
};

#ifdef __HIPCC__
// bbox_iou_wh (src/util.py:168-172) on Python doubles; the anchor's second side is its WIDTH again (wh2[0] read twice)
__device__ __forceinline__ int anchor_fit(double w1, double h1, const int* aw, int na) {
    int best = 0;
    double bestv = 0.0;
    for (int a = 0; a < na; ++a) {
        const double w2 = (double)aw[a], h2 = w2;
        const double inter = fmin(w1, w2) * fmin(h1, h2);
        const double uni = (w1 * h1 + w2 * h2) - inter;
        const double v = inter / uni;
        if (a == 0 || v > bestv) { bestv = v; best = a; }           // list.index(max(...)): the first maximum
    }
    return best;
}

// xywh2YOLO's cell and centre fractions (src/util.py:67-72), doubles.  False: the cell lies outside the grid (also for NaN).
__device__ __forceinline__ bool box_cell(float cx, float cy, int stride, int gw, int gh, int& gx, int& gy, double& fx, double& fy) {
    const double x = (double)cx / (double)stride, y = (double)cy / (double)stride;
    if (!(x >= 0.0 && x < (double)gw && y >= 0.0 && y < (double)gh)) return false;
    gx = (int)x; gy = (int)y;
    fx = x - (double)gx; fy = y - (double)gy;
    return true;
}

// torch.log(box / anchor + 1e-16) on a float32 tensor (src/util.py:73-74): float32 quotient and sum, then the correctly rounded
// logarithm of that float32 value
__device__ __forceinline__ float log_ratio(float v, int anchor) {
    const float q = v / (float)anchor + 1e-16f;
    return (float)log((double)q);
}

// the head that holds row r of an image, and the anchor of that row
__device__ __forceinline__ int head_of_row(const LossHeads& H, int r, int& a) {
    int h = 0;
    while (h + 1 < H.n && r >= H.off[h + 1]) ++h;
    a = (r - H.off[h]) % H.na[h];
    return h;
}

// columns 0-3 of the target row that box `bx` leaves on (head h, anchor a): (y fraction, x fraction, tw, th) — the centre slots
// are swapped in the reference (train.py:187: the caller unpacks xywh2YOLO's (y_coor, x_coor, y, x, w, h) as w-first)
__device__ __forceinline__ void target_xywh(const LossHeads& H, int h, int a, const float* bx, float t[4]) {
    int gx = 0, gy = 0;
    double fx = 0.0, fy = 0.0;
    box_cell(bx[0], bx[1], H.stride[h], H.gw[h], H.gh[h], gx, gy, fx, fy);
    t[0] = (float)fy; t[1] = (float)fx;
    t[2] = log_ratio(bx[2], H.aw[h][a]);
    t[3] = log_ratio(bx[3], H.ah[h][a]);
}

#endif

// loss.hip.  make_heads: the argument checks of rtod_yolo_loss on the head list (RTOD_E_ARG with a message that starts with `who`).
// enqueue_loss_core: owner[B][N] = -1, n_obj = 0, loss_assign_kernel (owner map, status bits) and, unless loss == nullptr, the
// reduce + finalize kernels of rtod_yolo_loss (the six doubles; n_obj is counted by the reduce kernel, so it runs when either
// is asked for).  ws: yolo_loss_workspace_bytes(batch, n_rows) bytes, checked by the caller; the owner map lies behind the partials.
int make_heads(const rtod_yolo_head* heads, int n_heads, int n_rows, LossHeads& H, const char* who);
int32_t* loss_owner_map(void* ws, int batch, int n_rows);
int enqueue_loss_core(const float* pred, int batch, int n_rows, int attrs, const LossHeads& H, const float* boxes, const int32_t* box_off,
                      float min_box_size, double* loss, double* per_image, int32_t* n_obj, int32_t* status, void* ws, hipStream_t s);

}  // namespace rtod
