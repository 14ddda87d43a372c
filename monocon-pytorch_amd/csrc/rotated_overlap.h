// Overlap of two rotated rectangles, the device functions shared by the KITTI evaluation kernels (kitti_eval.hip) and the
// 3D-box NMS (nms3d.hip): corners, the intersection polygon's area, and the two criterion expressions.  ONE implementation:
// what the NMS compares with its threshold is the very value mc_rotate_iou_eval / mc_box3d_overlap write.
//
// Arithmetic follows the reference kernel's float32 formulation step by step (corner rotation, the >= tests of
// point-in-quadrilateral, the determinant form of the segment intersection, centroid-angle insertion sort, triangle fan
// area accumulated in double); kitti_eval.hip's header says what pins it.
//
// Floating-point contraction is OFF from here to the end of the including file (kitti_eval.hip gives the measured reason:
// a fused multiply-add rounds once where the reference rounds twice and flips the vertex tests).
#pragma once
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

namespace mc {

constexpr int OVERLAP_MAXV = 16;    // vertex slots of a lane's stripes: at most 8 corners inside the other box + 8 edge
                                    // crossings (kitti_eval.hip's MAXV, where the measurements behind it are written down)

struct RBox { float cx, cy, dx, dy, ang; };

__device__ __forceinline__ void rbox_corners(const RBox b, float *c /* [8] in LDS or registers */, int stride) {
    const float a_cos = (float)cos((double)b.ang), a_sin = (float)sin((double)b.ang);
    const float hx = b.dx / 2, hy = b.dy / 2;
    const float px[4] = {-hx, -hx, hx, hx};
    const float py[4] = {-hy, hy, hy, -hy};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        c[(2 * i) * stride] = a_cos * px[i] + a_sin * py[i] + b.cx;
        c[(2 * i + 1) * stride] = -a_sin * px[i] + a_cos * py[i] + b.cy;
    }
}

__device__ __forceinline__ bool point_in_quad(float x, float y, const float (&q)[8]) {
    const float ab0 = q[2] - q[0], ab1 = q[3] - q[1];
    const float ad0 = q[6] - q[0], ad1 = q[7] - q[1];
    const float ap0 = x - q[0], ap1 = y - q[1];
    const float abab = ab0 * ab0 + ab1 * ab1, abap = ab0 * ap0 + ab1 * ap1;
    const float adad = ad0 * ad0 + ad1 * ad1, adap = ad0 * ap0 + ad1 * ap1;
    return abab >= abap && abap >= 0.f && adad >= adap && adap >= 0.f;
}

// edge i of quadrilateral p against edge j of quadrilateral q
__device__ __forceinline__ bool edge_cross(const float (&p)[8], const float (&q)[8], int i, int j, float &ox, float &oy) {
    const float A0 = p[2 * i], A1 = p[2 * i + 1], B0 = p[2 * ((i + 1) & 3)], B1 = p[2 * ((i + 1) & 3) + 1];
    const float C0 = q[2 * j], C1 = q[2 * j + 1], D0 = q[2 * ((j + 1) & 3)], D1 = q[2 * ((j + 1) & 3) + 1];
    const float BA0 = B0 - A0, BA1 = B1 - A1, DA0 = D0 - A0, CA0 = C0 - A0, DA1 = D1 - A1, CA1 = C1 - A1;
    const bool acd = DA1 * CA0 > CA1 * DA0;
    const bool bcd = (D1 - B1) * (C0 - B0) > (C1 - B1) * (D0 - B0);
    if (acd == bcd) return false;
    const bool abc = CA1 * BA0 > BA1 * CA0;
    const bool abd = DA1 * BA0 > BA1 * DA0;
    if (abc == abd) return false;
    const float DC0 = D0 - C0, DC1 = D1 - C1;
    const float ABBA = A0 * B1 - B0 * A1, CDDC = C0 * D1 - D0 * C1;
    const float DH = BA1 * DC0 - BA0 * DC1;
    ox = (ABBA * DC0 - BA0 * CDDC) / DH;
    oy = (ABBA * DC1 - BA1 * CDDC) / DH;
    return true;
}

// area of the intersection of quadrilaterals p (the query) and q (the box); vx / vy / vs: this lane's LDS stripes, slot s
// of a stripe at [s * STRIDE] (STRIDE = the lanes of the workgroup: slot-major, so the data-dependent indexing of the
// vertex sort is a conflict-free ds_read / ds_write instead of scratch memory)
template <int STRIDE>
__device__ inline double quad_intersection_area(const float (&p)[8], const float (&q)[8], float *vx, float *vy, float *vs) {
    int n = 0;
    auto push = [&](float x, float y) {
        if (n < OVERLAP_MAXV) {
            vx[n * STRIDE] = x;
            vy[n * STRIDE] = y;
            ++n;
        }
    };
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (point_in_quad(p[2 * i], p[2 * i + 1], q)) push(p[2 * i], p[2 * i + 1]);
        if (point_in_quad(q[2 * i], q[2 * i + 1], p)) push(q[2 * i], q[2 * i + 1]);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float x, y;
            if (edge_cross(p, q, i, j, x, y)) push(x, y);
        }
    if (n == 0) return 0.0;
    // order the vertices by the angle around their centroid (key: cosine, mirrored for the lower half plane)
    float c0 = 0.f, c1 = 0.f;
    for (int i = 0; i < n; ++i) { c0 += vx[i * STRIDE]; c1 += vy[i * STRIDE]; }
    c0 = (float)((double)c0 / (double)n);
    c1 = (float)((double)c1 / (double)n);
    for (int i = 0; i < n; ++i) {
        float v0 = vx[i * STRIDE] - c0, v1 = vy[i * STRIDE] - c1;
        const float d = sqrtf(v0 * v0 + v1 * v1);
        v0 = v0 / d;
        v1 = v1 / d;
        if (v1 < 0.f) v0 = -2.f - v0;
        vs[i * STRIDE] = v0;
    }
    for (int i = 1; i < n; ++i) {
        if (vs[(i - 1) * STRIDE] > vs[i * STRIDE]) {
            const float key = vs[i * STRIDE], tx = vx[i * STRIDE], ty = vy[i * STRIDE];
            int j = i;
            while (j > 0 && vs[(j - 1) * STRIDE] > key) {
                vs[j * STRIDE] = vs[(j - 1) * STRIDE];
                vx[j * STRIDE] = vx[(j - 1) * STRIDE];
                vy[j * STRIDE] = vy[(j - 1) * STRIDE];
                --j;
            }
            vs[j * STRIDE] = key;
            vx[j * STRIDE] = tx;
            vy[j * STRIDE] = ty;
        }
    }
    // triangle fan from vertex 0; each triangle's area in float32, the sum in double (the reference's typing)
    double area = 0.0;
    const float a0 = vx[0], a1 = vy[0];
    for (int i = 0; i < n - 2; ++i) {
        const float b0 = vx[(i + 1) * STRIDE], b1 = vy[(i + 1) * STRIDE];
        const float e0 = vx[(i + 2) * STRIDE], e1 = vy[(i + 2) * STRIDE];
        const float cr = (a0 - e0) * (b1 - e1) - (a1 - e1) * (b0 - e0);
        area += fabs((double)cr / 2.0);
    }
    return area;
}

// Bird's-eye-view criterion, rotate_iou.py:252-277 (rbox1 = the QUERY box): ai = the intersection area (a double in the
// reference's expression), area1 = dx * dy of the query, area2 = of the box (float32).  -1: IoU, 0: / area(query),
// 1: / area(box), other: the bare area.
__device__ __forceinline__ float bev_overlap_value(double ai, float area1, float area2, int criterion) {
    double r;
    if (criterion == -1) r = ai / ((double)(area1 + area2) - ai);
    else if (criterion == 0) r = ai / (double)area1;
    else if (criterion == 1) r = ai / (double)area2;
    else r = ai;
    return (float)r;
}

// 3D criterion, eval.py:128-157: ai = the bird's-eye-view intersection area; the box spans [by - bh, by] in height (camera
// frame: y points down, y = the bottom face) and has dims (bl, bh, bw), the query (qy; ql, qh, qw).  -1: 3D IoU,
// 0: / volume(box), 1: / volume(query), other: 1 wherever the boxes meet.
__device__ __forceinline__ double box3d_overlap_value(double ai, double by, double bl, double bh, double bw, double qy, double ql,
                                                      double qh, double qw, int criterion) {
    const float inter = (float)ai;       // the reference passes the bare area through a float32 array
    double r = 0.0;
    if (inter > 0.f) {
        const double iw = fmin(by, qy) - fmax(by - bh, qy - qh);
        if (iw > 0.0) {
            const double area1 = bl * bh * bw, area2 = ql * qh * qw;
            const double inc = iw * (double)inter;
            double ua;
            if (criterion == -1) ua = area1 + area2 - inc;
            else if (criterion == 0) ua = area1;
            else if (criterion == 1) ua = area2;
            else ua = inc;
            r = inc / ua;
        }
    }
    return r;
}

}  // namespace mc
