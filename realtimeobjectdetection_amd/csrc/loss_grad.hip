// Gradient of the reference's YOLO training loss (loss.hip) with respect to the RAW head maps: what autograd gives when the maps go
// through predict_transform(TRAIN=True) (src/util.py:175-239) and the five MSELoss(reduction='sum') terms of darknet_loss
// (train.py:211-230).  Closed form, per prediction row p (TRAIN=True decode) with target row t and w = (5, 5, 5, 5, 1, 1, ...):
//   object row      g_c = 2 w_c (p_c - t_c)                         c = 0 .. 4 + C
//   no-object row   g_4 = p_4 (= 2 * 0.5 * (p_4 - 0)), every other g_c = 0
//   dz_c = g_c p_c (1 - p_c) on the sigmoid columns c in {0, 1, 4, 5, ...};  dz_c = g_c for c in {2, 3}
// Raw map channel a * attrs + c at cell (gy, gx) of a head <-> prediction row (gy * GW + gx) * A + a of that head.
//
// Targets, filters, the owner map and the status bits are rtod_yolo_loss's own: the assignment phase is the same launch
// (enqueue_loss_core, loss_common.h), and the six doubles, when asked for, come from its reduce + finalize kernels, so they are
// bit-identical to rtod_yolo_loss.  Compiled with loss.hip's flags: float32, one rounding per operation, no FMA, in the order of
// the formulas above ((2 w_c) is exact; g p, then (1 - p), then their product).  A value the formula makes zero is stored as +0.
//
// Launch sequence (enqueue only): the memsets and kernels of enqueue_loss_core, then
//   raw    one thread per element of grad_raw (x fastest: coalesced stores).  Every element is written; a no-object row reads
//          p_4 alone, an object row reads its prediction row and the owning box
//   pred   (optional) one thread per element of grad_pred [B, N, attrs]: g before the sigmoid factor
#include "loss_common.h"

namespace rtod {

// g_c of row r (image-relative) of image b, and p_c where g is not structurally zero (p = 0 otherwise: dz is then 0 too)
__device__ __forceinline__ float loss_grad_g(const float* __restrict__ pred, const int32_t* __restrict__ owner, const float* __restrict__ boxes,
                                             const LossHeads& H, int h, int a, int64_t row, int attrs, int c, float& p) {
    const int own = owner[row];
    p = 0.0f;
    if (own < 0) {
        if (c != 4) return 0.0f;
        p = pred[row * attrs + 4];
        return p;
    }
    p = pred[row * attrs + c];
    const float* bx = boxes + (int64_t)own * attrs;
    float t;
    if (c < 4) {
        float t4[4];
        target_xywh(H, h, a, bx, t4);
        t = c == 0 ? t4[0] : c == 1 ? t4[1] : c == 2 ? t4[2] : t4[3];
    } else t = bx[c];
    const float w2 = c < 4 ? 10.0f : 2.0f;                          // 2 * w_c
    return w2 * (p - t);
}

__device__ __forceinline__ float plus_zero(float v) { return v == 0.0f ? 0.0f : v; }

// grid: (blocks over A*attrs*GH*GW of one head, batch, head)
__global__ __launch_bounds__(LOSS_BLOCK)
void loss_grad_raw_kernel(const float* __restrict__ pred, const int32_t* __restrict__ owner, const float* __restrict__ boxes, int N, int attrs,
                          int batch, LossHeads H, float* __restrict__ grad_raw) {
    const int h = blockIdx.z, b = blockIdx.y;
    const int cells = H.gh[h] * H.gw[h], A = H.na[h];
    const int64_t per_img = (int64_t)A * attrs * cells;
    const int64_t e = (int64_t)blockIdx.x * LOSS_BLOCK + threadIdx.x;
    if (e >= per_img) return;
    int64_t head_off = 0;                                           // batch * sum over the earlier heads of A * attrs * GH * GW
    for (int q = 0; q < h; ++q) head_off += (int64_t)batch * H.na[q] * attrs * H.gh[q] * H.gw[q];
    const int ch = (int)(e / cells), cell = (int)(e - (int64_t)ch * cells);
    const int a = ch / attrs, c = ch - a * attrs;
    const int64_t row = (int64_t)b * N + H.off[h] + (int64_t)cell * A + a;
    float p;
    const float g = loss_grad_g(pred, owner, boxes, H, h, a, row, attrs, c, p);
    float dz = g;
    if (c != 2 && c != 3) {
        const float gp = g * p;
        const float q = 1.0f - p;
        dz = gp * q;
    }
    grad_raw[head_off + (int64_t)b * per_img + e] = plus_zero(dz);
}

__global__ __launch_bounds__(LOSS_BLOCK)
void loss_grad_pred_kernel(const float* __restrict__ pred, const int32_t* __restrict__ owner, const float* __restrict__ boxes, int N, int attrs,
                           int64_t total, LossHeads H, float* __restrict__ grad_pred) {
    const int64_t t = (int64_t)blockIdx.x * LOSS_BLOCK + threadIdx.x;
    if (t >= total) return;
    const int64_t row = t / attrs;
    const int c = (int)(t - row * attrs);
    int a;
    const int h = head_of_row(H, (int)(row % N), a);
    float p;
    grad_pred[t] = plus_zero(loss_grad_g(pred, owner, boxes, H, h, a, row, attrs, c, p));
}

int launch_yolo_loss_grad(const float* pred, int batch, int n_rows, int num_class, const rtod_yolo_head* heads, int n_heads,
                          const float* boxes, const int32_t* box_off, float min_box_size, float* grad_raw, float* grad_pred, double* loss,
                          int32_t* n_obj, int32_t* status, void* ws, size_t ws_bytes, hipStream_t s) {
    if (!pred || !heads || !boxes || !box_off || !grad_raw || !status || !ws) { set_error("yolo_loss_grad: null pointer"); return RTOD_E_ARG; }
    if (batch < 1 || n_rows < 1 || num_class < 1) { set_error("yolo_loss_grad: unsupported shape (batch=%d n_rows=%d num_class=%d)", batch, n_rows, num_class); return RTOD_E_ARG; }
    if ((int64_t)batch * n_rows > INT32_MAX) { set_error("yolo_loss_grad: batch * n_rows exceeds 2^31 - 1"); return RTOD_E_ARG; }
    if (min_box_size != min_box_size) { set_error("yolo_loss_grad: min_box_size is not a number"); return RTOD_E_ARG; }
    LossHeads H;
    if (int rc = make_heads(heads, n_heads, n_rows, H, "yolo_loss_grad")) return rc;
    if (ws_bytes < yolo_loss_workspace_bytes(batch, n_rows)) { set_error("yolo_loss_grad: workspace too small"); return RTOD_E_ARG; }
    if ((uintptr_t)ws & 7) { set_error("yolo_loss_grad: workspace must be 8-byte aligned"); return RTOD_E_ARG; }
    const int attrs = 5 + num_class;
    if (int rc = enqueue_loss_core(pred, batch, n_rows, attrs, H, boxes, box_off, min_box_size, loss, nullptr, n_obj, status, ws, s)) return rc;
    const int32_t* owner = loss_owner_map(ws, batch, n_rows);
    int64_t most = 0;
    for (int h = 0; h < n_heads; ++h) most = std::max(most, (int64_t)H.na[h] * attrs * H.gh[h] * H.gw[h]);
    hipLaunchKernelGGL(loss_grad_raw_kernel, dim3((unsigned)((most + LOSS_BLOCK - 1) / LOSS_BLOCK), batch, n_heads), dim3(LOSS_BLOCK), 0, s,
                       pred, owner, boxes, n_rows, attrs, batch, H, grad_raw);
    if (grad_pred) {
        const int64_t total = (int64_t)batch * n_rows * attrs;
        hipLaunchKernelGGL(loss_grad_pred_kernel, dim3((unsigned)((total + LOSS_BLOCK - 1) / LOSS_BLOCK)), dim3(LOSS_BLOCK), 0, s,
                           pred, owner, boxes, n_rows, attrs, total, H, grad_pred);
    }
    return hip_fail(hipGetLastError(), "yolo_loss_grad launch");
}

}  // namespace rtod
