// KITTI result rows on the device: the decode's kept boxes -> the packed rows of the KITTI annotation dicts
// (mc_kitti_format).  The same arithmetic as utils/kitti_convert_utils.py (convert_to_kitti_3d / convert_to_kitti_2d),
// which tests/test_engine.py pins to the reference:
//
//   * 3D rows, decode order: the 8 corners of the bottom-centred box in float32, in project_boxes_3d's operation order
//     (sinf / cosf, no fused multiply-add), projected with P2 in float64 and divided by the projected depth with no special
//     case for points behind the camera; min / max over the corners, the visibility test x1 < w, y1 < h, x2 > 0, y2 > 0,
//     clip to [0, w] x [0, h], scale by the inverse resize factors; alpha = -atan2(x, z) + rot_y in float32.
//   * 2D rows: the kept box2d rows grouped by class 0, 1, 2, each class in decode order, scaled the same way.
//
// One workgroup per image.  The rows are compacted in decode order: a wave64 ballot / popcount gives a lane its rank among
// the wave's survivors, the waves' totals in LDS give the wave's base, and a running base carries the count across
// chunks of 256 boxes (K <= 1024, so at most four chunks).  The 2D grouping needs each class's start, so a first pass
// counts the kept boxes per class.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mc_internal.h"

namespace mc {

constexpr int KF_THREADS = 256;
constexpr int KF_WAVES = KF_THREADS / 64;
constexpr int KF_CLASSES = 3;          // ('Pedestrian', 'Cyclist', 'Car'): the groups of convert_to_kitti_2d

// rank of this lane's `pred` among all true predicates of the workgroup (lanes in thread order); *total: their number.
// Every thread of the workgroup must call it.
__device__ __forceinline__ int block_rank(bool pred, int *wave_cnt, int *total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long m = __ballot(pred);
    const int within = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wave_cnt[wave] = __popcll(m);
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < KF_WAVES; ++w) {
        const int c = wave_cnt[w];
        before += w < wave ? c : 0;
        all += c;
    }
    __syncthreads();                   // wave_cnt is reused by the next call
    *total = all;
    return before + within;
}

struct Proj { double x1, y1, x2, y2; };

// project_boxes_3d for one (x, y_bottom, z, l, h, w, rot_y) box
__device__ Proj project_box(const float *b, const float *P) {
#pragma clang fp contract(off)
    const float s = sinf(b[6]), c = cosf(b[6]);
    double lo_u = 0.0, lo_v = 0.0, hi_u = 0.0, hi_v = 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float ux = (k & 4) ? 0.5f : -0.5f, uy = (k & 2) ? 0.0f : -1.0f, uz = (k & 1) ? 0.5f : -0.5f;
        const float cx = b[3] * ux, cy = b[4] * uy, cz = b[5] * uz;
        const float x = cx * c + cz * s;
        const float z = -cx * s + cz * c;
        const double px = (double)(x + b[0]), py = (double)(cy + b[1]), pz = (double)(z + b[2]);
        const double p0 = px * (double)P[0] + py * (double)P[1] + pz * (double)P[2] + (double)P[3];
        const double p1 = px * (double)P[4] + py * (double)P[5] + pz * (double)P[6] + (double)P[7];
        const double p2 = px * (double)P[8] + py * (double)P[9] + pz * (double)P[10] + (double)P[11];
        const double u = p0 / p2, v = p1 / p2;
        if (k == 0) {
            lo_u = hi_u = u;
            lo_v = hi_v = v;
        } else {
            lo_u = fmin(lo_u, u); hi_u = fmax(hi_u, u);
            lo_v = fmin(lo_v, v); hi_v = fmax(hi_v, v);
        }
    }
    return {lo_u, lo_v, hi_u, hi_v};
}

__global__ void __launch_bounds__(KF_THREADS)
kitti_format_kernel(const float *__restrict__ box2d, const float *__restrict__ box3d, const int64_t *__restrict__ cls,
                    const uint8_t *__restrict__ keep, const float *__restrict__ P2, const float *__restrict__ hw_scale, int K,
                    float *__restrict__ rows3d, int *__restrict__ n3d, float *__restrict__ rows2d, int *__restrict__ n2d) {
#pragma clang fp contract(off)
    __shared__ int wave_cnt[KF_WAVES];
    const int b = blockIdx.x;
    const size_t base = (size_t)b * K;
    const float *P = P2 + (size_t)b * 12;
    const double ori_h = hw_scale[b * 4 + 0], ori_w = hw_scale[b * 4 + 1];
    const double inv_x = hw_scale[b * 4 + 2], inv_y = hw_scale[b * 4 + 3];

    // pass 1: kept boxes per class -> the start of each class's group among the 2D rows
    int start[KF_CLASSES];
    {
        int cnt[KF_CLASSES] = {0, 0, 0};
        for (int i0 = 0; i0 < K; i0 += KF_THREADS) {
            const int i = i0 + threadIdx.x;
            const int c = (i < K && keep[base + i]) ? (int)cls[base + i] : -1;
#pragma unroll
            for (int g = 0; g < KF_CLASSES; ++g) cnt[g] += __syncthreads_count(c == g);
        }
        start[0] = 0;
        start[1] = cnt[0];
        start[2] = cnt[0] + cnt[1];
    }

    // pass 2: rows
    int out3 = 0;
    for (int i0 = 0; i0 < K; i0 += KF_THREADS) {
        const int i = i0 + threadIdx.x;
        const bool kept = i < K && keep[base + i];
        const int c = kept ? (int)cls[base + i] : -1;
        float bx[7];
        Proj pr{0.0, 0.0, 0.0, 0.0};
        bool vis = false;
        if (kept) {
#pragma unroll
            for (int j = 0; j < 7; ++j) bx[j] = box3d[(base + i) * 7 + j];
            pr = project_box(bx, P);
            vis = pr.x1 < ori_w && pr.y1 < ori_h && pr.x2 > 0.0 && pr.y2 > 0.0;
        }
        int tot;
        const int r3 = block_rank(vis, wave_cnt, &tot);
        if (vis) {
            float *o = rows3d + (base + out3 + r3) * 14;
            const double x1 = fmax(pr.x1, 0.0), y1 = fmax(pr.y1, 0.0);
            const double x2 = fmin(pr.x2, ori_w), y2 = fmin(pr.y2, ori_h);
            o[0] = (float)c;
            o[1] = -atan2f(bx[0], bx[2]) + bx[6];
            o[2] = (float)(x1 * inv_x);
            o[3] = (float)(y1 * inv_y);
            o[4] = (float)(x2 * inv_x);
            o[5] = (float)(y2 * inv_y);
#pragma unroll
            for (int j = 0; j < 3; ++j) o[6 + j] = bx[3 + j];      // l, h, w
#pragma unroll
            for (int j = 0; j < 3; ++j) o[9 + j] = bx[j];          // x, y, z
            o[12] = bx[6];
            o[13] = box2d[(base + i) * 5 + 4];
        }
        out3 += tot;
#pragma unroll
        for (int g = 0; g < KF_CLASSES; ++g) {
            const int r2 = block_rank(c == g, wave_cnt, &tot);
            if (c == g) {
                const float *s = box2d + (base + i) * 5;
                float *o = rows2d + (base + start[g] + r2) * 6;
                o[0] = (float)g;
                o[1] = (float)((double)s[0] * inv_x);
                o[2] = (float)((double)s[1] * inv_y);
                o[3] = (float)((double)s[2] * inv_x);
                o[4] = (float)((double)s[3] * inv_y);
                o[5] = s[4];
            }
            start[g] += tot;
        }
    }
    if (threadIdx.x == 0) {
        n3d[b] = out3;
        n2d[b] = start[KF_CLASSES - 1];     // the last group ends after every kept box of classes 0..2
    }
}

}  // namespace mc

using namespace mc;

extern "C" {

int mc_kitti_format(mc_handle *h, const float *box2d, const float *box3d, const int64_t *cls, const uint8_t *keep_thr,
                    const float *P2, const float *img_hw_scale, int B, int K, float *rows3d, int *n3d, float *rows2d,
                    int *n2d, void *stream) {
    if (!h) return -1;
    if (!box2d || !box3d || !cls || !keep_thr || !P2 || !img_hw_scale || !rows3d || !n3d || !rows2d || !n2d)
        return fail(h, "mc_kitti_format: null argument");
    if (B < 1 || K < 1 || K > 1024) return fail(h, "mc_kitti_format: bad shape B=%d K=%d (B >= 1, 1 <= K <= 1024)", B, K);
    HIPCHK(h, hipSetDevice(h->device));
    hipLaunchKernelGGL(kitti_format_kernel, dim3(B), dim3(KF_THREADS), 0, static_cast<hipStream_t>(stream), box2d, box3d, cls,
                       keep_thr, P2, img_hw_scale, K, rows3d, n3d, rows2d, n2d);
    HIPCHK(h, hipGetLastError());
    return 0;
}

}  // extern "C"
