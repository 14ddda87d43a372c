// Greedy non-maximum suppression of the decode's 3D boxes on the device (mc_nms3d): rotated bird's-eye-view IoU or 3D IoU,
// per image, between mc_decode and mc_kitti_format.  The reference has no counterpart (it ships every box above the score
// threshold); the feature is opt-in and include/monocon_hip.h states its semantics.
//
// The overlap of a pair is formed by rotated_overlap.h, the device functions of mc_rotate_iou_eval / mc_box3d_overlap:
// the value compared with the threshold is the value those kernels write at criterion -1 (box = the higher-ranked
// participant, query = the lower-ranked one).  Contraction is off for this file as for kitti_eval.hip, and for its reason.
//
// One workgroup of 128 lanes per image (the design point, B = 64, K = 100 with 5 .. 30 participants per image, is bound by
// launch latency, not by work):
//   1. compact the participants in slot order (wave ballot / popcount), rank-sort them by (score key descending, slot
//      ascending) -- the keys are the order-preserving integer images of the scores (f2key of kernels_decode.hip), so
//      the order is total for any bit pattern;
//   2. the corners and the class of every participant ONCE into LDS, in sorted order;
//   3. the pairs i < j of the sorted list spread over the lanes: class test, a cheap reject on the corners, else the
//      clipping; a pair with ov > thr sets bit j of row i of an n x n bit matrix;
//   4. one wave scans the rows in order: a row whose box is still alive is OR-ed into the `removed` words (lane w owns word
//      w), and the newly removed boxes get their suppressor;
//   5. all lanes write keep_out / suppressed_by.
//
// LDS (static, < 64 KB): vertex stripes 3 x 16 x 128 x 4 B = 24 KB (the sort's keys and slots live there before step 3),
// corners 8 x 1024 x 4 B = 32 KB, sorted slots 2 KB, their classes as 16-bit values 2 KB (a pair loop that fetched the two
// int64 classes from memory spent its time waiting for them: 44 us at 46 participants per image, B = 64), the bit matrix for
// n <= 128 (128 rows x 2 words) 2 KB, removed words 128 B: 63.6 KB.  For n > 128 (up to 1024 rows x 16 words = 128 KB) the matrix is in the handle's workspace, B x K x ceil(K / 64)
// words, allocated when it first grows: the workgroup zeroes its rows, sets bits with atomics and reads them back after
// a barrier, all within one workgroup.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "mc_internal.h"
#include "rotated_overlap.h"

#pragma clang fp contract(off)

namespace mc {

constexpr int NMS_THREADS = 128;
constexpr int NMS_WAVES = NMS_THREADS / 64;
constexpr int NMS_MAXK = 1024;              // the decode's own limit
constexpr int NMS_LDS_N = 128;              // participants up to which the bit matrix lives in LDS
constexpr int NMS_LDS_WORDS = NMS_LDS_N / 64;
constexpr int NMS_SCAN_ROWS = 8;            // rows the scan fetches ahead of its serial walk

typedef unsigned long long u64;

__device__ __forceinline__ unsigned nms_f2key(float f) {      // kernels_decode.hip f2key
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// May the clipping of two boxes be skipped?  Only where the reference formulation gives an intersection of exactly 0:
// every corner of a box lies on the circle around its centre through its corners, so two boxes whose circles are apart
// by 1 % of their radii and 1 mm meet nowhere -- no corner passes point_in_quad, no edges cross.  The margin is far above
// the float32 round-off of those tests for the boxes admitted here: both sides of both boxes >= 0.1 mm (the >= tests of a
// box with a zero side hold for points far outside it) and coordinates within 1e4.  NaN / inf make a comparison false
// and the pair takes the full path.
__device__ __forceinline__ bool nms_far_apart(const float (&p)[8], const float (&q)[8]) {
    const float pcx = (p[0] + p[4]) * 0.5f, pcy = (p[1] + p[5]) * 0.5f, qcx = (q[0] + q[4]) * 0.5f, qcy = (q[1] + q[5]) * 0.5f;
    const float pr = 0.5f * sqrtf((p[4] - p[0]) * (p[4] - p[0]) + (p[5] - p[1]) * (p[5] - p[1]));
    const float qr = 0.5f * sqrtf((q[4] - q[0]) * (q[4] - q[0]) + (q[5] - q[1]) * (q[5] - q[1]));
    const float ps1 = (p[2] - p[0]) * (p[2] - p[0]) + (p[3] - p[1]) * (p[3] - p[1]);
    const float ps2 = (p[6] - p[0]) * (p[6] - p[0]) + (p[7] - p[1]) * (p[7] - p[1]);
    const float qs1 = (q[2] - q[0]) * (q[2] - q[0]) + (q[3] - q[1]) * (q[3] - q[1]);
    const float qs2 = (q[6] - q[0]) * (q[6] - q[0]) + (q[7] - q[1]) * (q[7] - q[1]);
    const bool sane = ps1 >= 1e-8f && ps2 >= 1e-8f && qs1 >= 1e-8f && qs2 >= 1e-8f && fabsf(pcx) <= 1e4f && fabsf(pcy) <= 1e4f &&
                      fabsf(qcx) <= 1e4f && fabsf(qcy) <= 1e4f && pr <= 1e4f && qr <= 1e4f;
    const float d = sqrtf((pcx - qcx) * (pcx - qcx) + (pcy - qcy) * (pcy - qcy));
    return sane && d > 1.01f * (pr + qr) + 1e-3f;
}

__global__ void __launch_bounds__(NMS_THREADS)
nms3d_kernel(const float *__restrict__ box2d, const float *__restrict__ box3d, const int64_t *__restrict__ cls,
             const uint8_t *keep_in, int K, int mode, float thr, int class_agnostic, u64 *__restrict__ ws, uint8_t *keep_out,
             int *__restrict__ suppressed_by) {
    __shared__ float vbuf[3][OVERLAP_MAXV][NMS_THREADS];        // vertex x, vertex y, sort key -- one stripe per lane
    __shared__ float corners[8][NMS_MAXK];               // [coordinate][rank]
    __shared__ unsigned short sslot[NMS_MAXK];           // rank -> slot
    __shared__ short scls[NMS_MAXK];                     // rank -> class, -1: a value outside [0, 32767) (read from memory)
    __shared__ u64 lmat[NMS_LDS_N * NMS_LDS_WORDS];
    __shared__ u64 removed[NMS_MAXK / 64];
    __shared__ int wave_cnt[NMS_WAVES];
    // before the pair phase the vertex stripes hold the compacted keys and slots (4 KB + 2 KB of 24 KB)
    unsigned *ckey = reinterpret_cast<unsigned *>(&vbuf[0][0][0]);
    unsigned short *cslot = reinterpret_cast<unsigned short *>(&vbuf[1][0][0]);

    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t base = (size_t)b * K;

    // ---- 1. participants in slot order.  Every read of keep_in happens here, before the first write of keep_out (they may
    //         be one buffer)
    int n = 0;
    for (int t0 = 0; t0 < K; t0 += NMS_THREADS) {
        const int t = t0 + tid;
        const bool part = t < K && keep_in[base + t] != 0;
        const u64 m = __ballot(part);
        if (lane == 0) wave_cnt[wave] = __popcll(m);
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < NMS_WAVES; ++w) {
            const int c = wave_cnt[w];
            before += w < wave ? c : 0;
            all += c;
        }
        if (part) {
            const int r = n + before + __popcll(m & ((1ull << lane) - 1ull));
            ckey[r] = nms_f2key(box2d[(base + t) * 5 + 4]);
            cslot[r] = (unsigned short)t;
        }
        n += all;
        __syncthreads();                                 // wave_cnt is reused by the next chunk
    }
    // defaults: nothing kept, nobody a participant; steps 4 and 5 overwrite the participants' entries
    for (int t = tid; t < K; t += NMS_THREADS) {
        keep_out[base + t] = 0;
        if (suppressed_by) suppressed_by[base + t] = -2;
    }
    // rank sort: key descending, slot ascending (the compacted list is in slot order)
    for (int r = tid; r < n; r += NMS_THREADS) {
        const unsigned kr = ckey[r];
        int rank = 0;
        for (int j = 0; j < n; ++j) {
            const unsigned kj = ckey[j];
            rank += (kj > kr) || (kj == kr && j < r);
        }
        sslot[rank] = cslot[r];
    }
    const bool in_lds = n <= NMS_LDS_N;
    const int stride = in_lds ? NMS_LDS_WORDS : (K + 63) / 64;       // words per row
    u64 *gmat = in_lds ? nullptr : ws + (size_t)b * K * ((K + 63) / 64);   // (ws may be null when K <= 128)
    for (int i = tid; i < n * stride; i += NMS_THREADS) {
        if (in_lds) lmat[i] = 0;
        else gmat[i] = 0;
    }
    if (tid < NMS_MAXK / 64) removed[tid] = 0;
    __syncthreads();

    // ---- 2. corners of the bird's-eye-view footprint (x, z, dim0, dim2, rot_y), once per participant
    for (int r = tid; r < n; r += NMS_THREADS) {
        const float *s = box3d + (base + sslot[r]) * 7;
        rbox_corners(RBox{s[0], s[2], s[3], s[5], s[6]}, &corners[0][r], NMS_MAXK);
        const int64_t c = cls[base + sslot[r]];
        scls[r] = (c >= 0 && c < 32767) ? (short)c : (short)-1;
    }
    __syncthreads();                                     // also: the last reads of ckey / cslot are behind us

    // ---- 3. pairs i < j (ranks): box = i, query = j.  Row i of the triangle has n - 1 - i pairs; rows r and n - 2 - r
    //         together have n, so the triangle folds into n / 2 rows of n (the middle row of an even n stands alone)
    float *vx = &vbuf[0][0][tid], *vy = &vbuf[1][0][tid], *vs = &vbuf[2][0][tid];
    for (int pi = tid; pi < (n / 2) * n; pi += NMS_THREADS) {
        const int r = pi / n, c = pi - r * n;
        int i, j;
        if (c < n - 1 - r) {
            i = r;
            j = r + 1 + c;
        } else {
            i = n - 2 - r;
            if (i == r) continue;
            j = i + 1 + (c - (n - 1 - r));
        }
        const size_t si = base + sslot[i], sj = base + sslot[j];
        if (!class_agnostic) {      // the staged classes decide; a value they cannot hold is compared as it is
            const short ci = scls[i], cj = scls[j];
            if ((ci >= 0 && cj >= 0) ? ci != cj : cls[si] != cls[sj]) continue;
        }
        float q[8], p[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) { q[k] = corners[k][i]; p[k] = corners[k][j]; }
        if (nms_far_apart(p, q)) continue;
        const float *bb = box3d + si * 7, *qq = box3d + sj * 7;
        // a footprint without area takes no part: the IoU expression is a / (a - a) or 0 / 0 there, and its value round-off
        // (measured with the CPU restatement: 5.05 for a point inside a box, -8.4e6 for one 30 m away)
        if (!(bb[3] > 0.f && bb[5] > 0.f && qq[3] > 0.f && qq[5] > 0.f)) continue;
        // one footprint twice (a pixel that peaks in two class channels decodes to the same box): it meets itself in its own
        // area.  The clipping cannot say so -- every vertex test of such a pair is a tie that round-off decides, and the CPU
        // restatement gives less than 0.99 for 291 of 300 rotated boxes against themselves.
        const bool same = bb[0] == qq[0] && bb[2] == qq[2] && bb[3] == qq[3] && bb[5] == qq[5] && bb[6] == qq[6];
        const double ai = same ? (double)(bb[3] * bb[5]) : quad_intersection_area<NMS_THREADS>(p, q, vx, vy, vs);
        bool hit;
        if (mode == 0)
            hit = bev_overlap_value(ai, qq[3] * qq[5], bb[3] * bb[5], -1) > thr;
        else
            hit = box3d_overlap_value(ai, (double)bb[1], (double)bb[3], (double)bb[4], (double)bb[5], (double)qq[1],
                                      (double)qq[3], (double)qq[4], (double)qq[5], -1) > (double)thr;
        if (hit) {                                       // (a NaN overlap compares false)
            const u64 bit = 1ull << (j & 63);
            if (in_lds) atomicOr(&lmat[i * stride + (j >> 6)], bit);
            else atomicOr(&gmat[(size_t)i * stride + (j >> 6)], bit);
        }
    }
    __syncthreads();

    // ---- 4. the greedy pass: one wave, lane w owns word w of `removed`
    if (wave == 0) {
        const int nwords = (n + 63) / 64;
        u64 rem = 0;
        for (int i0 = 0; i0 < n; i0 += NMS_SCAN_ROWS) {
            u64 rows[NMS_SCAN_ROWS];
#pragma unroll
            for (int u = 0; u < NMS_SCAN_ROWS; ++u) {
                const int i = i0 + u;
                rows[u] = 0;
                if (i < n && lane < nwords) rows[u] = in_lds ? lmat[i * stride + lane] : gmat[(size_t)i * stride + lane];
            }
#pragma unroll
            for (int u = 0; u < NMS_SCAN_ROWS; ++u) {
                const int i = i0 + u;
                if (i >= n) break;
                const u64 w = __shfl(rem, i >> 6);
                if ((w >> (i & 63)) & 1ull) continue;    // suppressed itself: suppresses nothing (uniform over the wave)
                u64 fresh = rows[u] & ~rem;
                rem |= fresh;
                if (suppressed_by) {
                    const int by = (int)sslot[i];
                    while (fresh) {
                        const int bitpos = __ffsll((long long)fresh) - 1;
                        fresh &= fresh - 1;
                        suppressed_by[base + sslot[lane * 64 + bitpos]] = by;
                    }
                }
            }
        }
        if (lane < nwords) removed[lane] = rem;
    }
    __syncthreads();

    // ---- 5. the kept participants
    for (int r = tid; r < n; r += NMS_THREADS) {
        if ((removed[r >> 6] >> (r & 63)) & 1ull) continue;
        keep_out[base + sslot[r]] = 1;
        if (suppressed_by) suppressed_by[base + sslot[r]] = -1;
    }
}

}  // namespace mc

using namespace mc;

extern "C" {

int mc_nms3d(mc_handle *h, const float *box2d, const float *box3d, const int64_t *cls, const uint8_t *keep_in, int B, int K,
             int mode, float iou_thr, int class_agnostic, uint8_t *keep_out, int *suppressed_by, void *stream) {
    if (!h) return -1;
    if (!box2d || !box3d || !cls || !keep_in || !keep_out) return fail(h, "mc_nms3d: null argument");
    if (B < 1 || K < 1 || K > NMS_MAXK) return fail(h, "mc_nms3d: bad shape B=%d K=%d (B >= 1, 1 <= K <= 1024)", B, K);
    if (mode != 0 && mode != 1) return fail(h, "mc_nms3d: mode %d (0 bird's-eye-view IoU, 1 3D IoU)", mode);
    if (!(iou_thr >= 0.f && iou_thr <= 1.f)) return fail(h, "mc_nms3d: iou_thr %g outside [0, 1]", (double)iou_thr);
    HIPCHK(h, hipSetDevice(h->device));
    if (K > NMS_LDS_N) {                       // more participants than the LDS matrix holds are possible
        const size_t words = (size_t)B * K * ((K + 63) / 64);
        if (words > h->nms_ws_words) {
            if (h->nms_ws) HIPCHK(h, hipFree(h->nms_ws));
            h->nms_ws = nullptr;
            h->nms_ws_words = 0;
            void *q = nullptr;
            HIPCHK(h, hipMalloc(&q, words * sizeof(unsigned long long)));
            h->nms_ws = static_cast<unsigned long long *>(q);
            h->nms_ws_words = words;
        }
    }
    hipLaunchKernelGGL(nms3d_kernel, dim3(B), dim3(NMS_THREADS), 0, static_cast<hipStream_t>(stream), box2d, box3d, cls, keep_in,
                       K, mode, iou_thr, class_agnostic, h->nms_ws, keep_out, suppressed_by);
    HIPCHK(h, hipGetLastError());
    return 0;
}

}  // extern "C"
