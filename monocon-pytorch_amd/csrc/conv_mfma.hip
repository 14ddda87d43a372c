// The fp32 kernels of the fused MFMA convolution (contract, helpers and epilogue: conv_mfma.h) and their launch
// (launch_conv_fp32; the choice among the family's kernels: conv_plan.hip).
#include "conv_mfma.h"

namespace mc {

template <int KS, int S, int CK, int WM, int WN, int WTM, int WTN, bool BM = false>
__global__ __launch_bounds__(64 * WM * WN, 3) void conv_mfma_kernel(const ConvArgs a) {
    using Cfg = ConvCfg<KS, S, CK, WM, WN, WTM, WTN>;
    constexpr int PB = Cfg::PB, BNT = Cfg::BNT, NT = Cfg::NT, PAD = Cfg::PAD;
    constexpr int IW = Cfg::IW, NPIX = Cfg::NPIX, CKP = Cfg::CKP;
    constexpr int C4 = CK / 4;
    static_assert(NT % C4 == 0, "a thread keeps one channel group across its staging elements");

    extern __shared__ __attribute__((aligned(16))) float lds[];
    int *pinfo = reinterpret_cast<int *>(lds + PB * NPIX * CKP);   // [PB][4] = b, oy0, ox0, valid

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int g = lane >> 5, li = lane & 31;

    int img, chunk, n0;
    conv_wg<BNT>(a, img, chunk, n0);

    if (tid < PB) {
        const int pp = chunk * PB + tid;
        const int valid = pp < a.ppi;
        const int py = pp / a.ppr, px = pp % a.ppr;
        pinfo[tid * 4 + 0] = img;
        pinfo[tid * 4 + 1] = py * 4;
        pinfo[tid * 4 + 2] = px * 8;
        pinfo[tid * 4 + 3] = valid;
    }
    __syncthreads();

    f32x16 acc[WTM][WTN];
#pragma unroll
    for (int tm = 0; tm < WTM; ++tm)
#pragma unroll
        for (int tn = 0; tn < WTN; ++tn)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[tm][tn][r] = 0.f;

    // ---- staging plan: element e = tid + NT*i of the [PB][NPIX][C4] halo tile.  Its input pixel
    //      does not depend on the K-chunk, so the lane offsets are resolved once per source; inside
    //      the K loop a chunk is NIT buffer loads (SGPR chunk offset) + NIT ds_write_b128 at
    //      immediate offsets.
    constexpr int TOTAL = PB * NPIX * C4;
    constexpr int NIT = (TOTAL + NT - 1) / NT;
    const int c4 = tid % C4;
    float *stage_dst = lds + (tid / C4) * CKP + c4 * 4;

    // A-fragment base offsets (floats) inside the LDS image for this lane
    int a_off[WTM];
#pragma unroll
    for (int tm = 0; tm < WTM; ++tm)
        a_off[tm] = ((wm * WTM + tm) * NPIX + ((li >> 3) * S) * IW + (li & 7) * S) * CKP + 4 * g;

    const int Cin4 = a.Cin >> 2;
    const __amdgpu_buffer_rsrc_t r_w = make_rsrc(a.wpk, (unsigned)(Cfg::KH * Cfg::KW * a.Cin * a.CoutP) * 4u);
    const int w_lane = (g * a.CoutP + n0 + wn * WTN * 32 + li) * 16;   // bytes

    // B fragment of step s (= tap * CK/8 + k8) of the K-chunk starting at concat channel kc
    constexpr int K8 = CK / 8, NS = Cfg::KH * Cfg::KW * K8;
    auto load_b = [&](f32x4(&dst)[WTN], int kc, int s) {
        const int tap = s / K8, k8 = s % K8;
        const int soff = (tap * Cin4 + ((kc + k8 * 8) >> 2)) * a.CoutP * 16;
#pragma unroll
        for (int tn = 0; tn < WTN; ++tn) dst[tn] = buf_load4(r_w, w_lane + tn * 32 * 16, soff);
    };
    auto load_a = [&](f32x4(&dst)[WTM], int s) {
        const int tap = s / K8, k8 = s % K8;
#pragma unroll
        for (int tm = 0; tm < WTM; ++tm)
            dst[tm] = *reinterpret_cast<const f32x4 *>(
                &lds[a_off[tm] + ((tap / Cfg::KW) * IW + (tap % Cfg::KW)) * CKP + k8 * 8]);
    };
    f32x4 bcur[WTN];
    load_b(bcur, 0, 0);   // weights do not depend on the staged tile: in flight across the barriers
    const EpiCoef<WTN> coef = conv_epi_coef<WN, WTN, BM>(a, n0, wn, li);

    int kbase = 0;   // channel offset of the current source inside the virtual concat
    for (int si = 0; si < a.nsrc; ++si) {
        const int Cs = a.src[si].C;
        const __amdgpu_buffer_rsrc_t r_in =
            make_rsrc(a.src[si].p + (size_t)img * a.Hin * a.Win * Cs, (unsigned)(a.Hin * a.Win * Cs) * 4u);
        int voff[NIT];
#pragma unroll
        for (int i = 0; i < NIT; ++i) {
            const int e = tid + NT * i;
            const int t = e / C4;
            const int pix = t % NPIX;
            const int p = (t / NPIX) % PB;
            const int iy = pix / IW, ix = pix % IW;
            const int y = pinfo[p * 4 + 1] * S - PAD + iy;
            const int x = pinfo[p * 4 + 2] * S - PAD + ix;
            const bool ok = e < TOTAL && pinfo[p * 4 + 3] && y >= 0 && y < a.Hin && x >= 0 && x < a.Win;
            voff[i] = ok ? ((y * a.Win + x) * Cs + c4 * 4) * 4 : BUF_OOB;
        }
        for (int c0 = 0; c0 < Cs; c0 += CK) {
            if (kbase + c0 > 0) __syncthreads();   // previous chunk's fragment reads done
            // ---- stage [PB][NPIX][CK] input halo, zero-filled outside the image
            constexpr int UB = NIT > 8 ? 8 : NIT;   // loads in flight per batch
#pragma unroll
            for (int i0 = 0; i0 < NIT; i0 += UB) {
                f32x4 v[UB];
#pragma unroll
                for (int u = 0; u < UB; ++u)
                    if (i0 + u < NIT) v[u] = buf_load4(r_in, voff[i0 + u], c0 * 4);
#pragma unroll
                for (int u = 0; u < UB; ++u) {
                    const int i = i0 + u;
                    if (i < NIT && (NT * (i + 1) <= TOTAL || tid + NT * i < TOTAL))
                        *reinterpret_cast<f32x4 *>(stage_dst + i * (NT / C4) * CKP) = v[u];
                }
            }
            __syncthreads();
            // ---- MFMA over taps x channel groups of 8; both operands are fetched one step ahead
            //      (explicit register double-buffering: hipcc otherwise issues each weight load
            //      right in front of the MFMA that consumes it and exposes the full L2 latency)
            const int kc = kbase + c0;
            const int kc_next = (kc + CK < a.Cin) ? kc + CK : kc;   // last chunk: harmless re-load
            f32x4 acur[WTM];
            load_a(acur, 0);
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                f32x4 anext[WTM], bnext[WTN];
                if (s + 1 < NS) {
                    load_a(anext, s + 1);
                    load_b(bnext, kc, s + 1);
                } else {
                    load_b(bnext, kc_next, 0);
                }
                __builtin_amdgcn_sched_barrier(0);   // keep the prefetch ahead of this step's MFMAs
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int tm = 0; tm < WTM; ++tm)
#pragma unroll
                        for (int tn = 0; tn < WTN; ++tn)
                            acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(
                                acur[tm][j], bcur[tn][j], acc[tm][tn], 0, 0, 0);
                if (s + 1 < NS) {
#pragma unroll
                    for (int tm = 0; tm < WTM; ++tm) acur[tm] = anext[tm];
                }
#pragma unroll
                for (int tn = 0; tn < WTN; ++tn) bcur[tn] = bnext[tn];
            }
        }
        kbase += Cs;
    }

    conv_epilogue<WM, WN, WTM, WTN, BNT, BM>(a, acc, pinfo, chunk * PB, img, n0, wm, wn, g, li, coef);
}

// ---- wave-specialised variant -------------------------------------------------------------
// Same math, same operand layouts and the same accumulation order as conv_mfma_kernel (results are
// bit-identical), but the workgroup carries one extra PRODUCER wave that stages K-chunk i+1 into
// the second half of a double-buffered LDS tile while the WM*WN consumer waves run the MFMA steps
// of chunk i.  One barrier per chunk instead of two, and no MFMA wave ever waits on HBM.
template <int KS, int S, int CK, int WM, int WN, int WTM, int WTN>
struct ConvCfgWS : ConvCfg<KS, S, CK, WM, WN, WTM, WTN> {
    using Base = ConvCfg<KS, S, CK, WM, WN, WTM, WTN>;
    static constexpr int NT = 64 * (WM * WN + 1);
    static constexpr int TILE = Base::PB * Base::NPIX * Base::CKP;
    static constexpr int LDS_FLOATS = 2 * TILE + Base::PB * 4;
    static constexpr size_t LDS_BYTES = sizeof(float) * LDS_FLOATS;
};

template <int KS, int S, int CK, int WM, int WN, int WTM, int WTN>
__global__ __launch_bounds__(64 * (WM * WN + 1), 3) void conv_mfma_ws_kernel(const ConvArgs a) {
    using Cfg = ConvCfgWS<KS, S, CK, WM, WN, WTM, WTN>;
    constexpr int PB = Cfg::PB, BNT = Cfg::BNT, PAD = Cfg::PAD;
    constexpr int IW = Cfg::IW, NPIX = Cfg::NPIX, CKP = Cfg::CKP, TILE = Cfg::TILE;
    constexpr int C4 = CK / 4;

    extern __shared__ __attribute__((aligned(16))) float lds[];
    int *pinfo = reinterpret_cast<int *>(lds + 2 * TILE);   // [PB][4] = b, oy0, ox0, valid

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool producer = wave == WM * WN;
    const int wm = wave / WN, wn = wave % WN;
    const int g = lane >> 5, li = lane & 31;

    int img, chunk, n0;
    conv_wg<BNT>(a, img, chunk, n0);

    if (tid < PB) {
        const int pp = chunk * PB + tid;
        const int valid = pp < a.ppi;
        const int py = pp / a.ppr, px = pp % a.ppr;
        pinfo[tid * 4 + 0] = img;
        pinfo[tid * 4 + 1] = py * 4;
        pinfo[tid * 4 + 2] = px * 8;
        pinfo[tid * 4 + 3] = valid;
    }
    __syncthreads();

    if (producer) {
        // ---- producer wave: element e = lane + 64*i of the [PB][NPIX][C4] tile (see
        //      conv_mfma_kernel: lane offsets once per source, then loads + LDS writes only)
        constexpr int TOTAL = PB * NPIX * C4;
        constexpr int NIT = (TOTAL + 63) / 64;
        constexpr int UB = NIT > 8 ? 8 : NIT;   // loads kept in flight per batch
        static_assert(64 % C4 == 0, "a lane keeps one channel group across its elements");
        const int c4 = lane % C4;
        int ci = 0;
        for (int si = 0; si < a.nsrc; ++si) {
            const int Cs = a.src[si].C;
            const __amdgpu_buffer_rsrc_t r_in =
                make_rsrc(a.src[si].p + (size_t)img * a.Hin * a.Win * Cs, (unsigned)(a.Hin * a.Win * Cs) * 4u);
            int voff[NIT];
#pragma unroll
            for (int i = 0; i < NIT; ++i) {
                const int e = lane + 64 * i;
                const int t = e / C4;
                const int pix = t % NPIX;
                const int p = (t / NPIX) % PB;
                const int iy = pix / IW, ix = pix % IW;
                const int y = pinfo[p * 4 + 1] * S - PAD + iy;
                const int x = pinfo[p * 4 + 2] * S - PAD + ix;
                const bool ok = e < TOTAL && pinfo[p * 4 + 3] && y >= 0 && y < a.Hin && x >= 0 && x < a.Win;
                voff[i] = ok ? ((y * a.Win + x) * Cs + c4 * 4) * 4 : BUF_OOB;
            }
            for (int c0 = 0; c0 < Cs; c0 += CK, ++ci) {
                float *dst = lds + (ci & 1) * TILE + (lane / C4) * CKP + c4 * 4;
#pragma unroll
                for (int i0 = 0; i0 < NIT; i0 += UB) {
                    f32x4 v[UB];
#pragma unroll
                    for (int u = 0; u < UB; ++u)
                        if (i0 + u < NIT) v[u] = buf_load4(r_in, voff[i0 + u], c0 * 4);
#pragma unroll
                    for (int u = 0; u < UB; ++u) {
                        const int i = i0 + u;
                        if (i < NIT && (64 * (i + 1) <= TOTAL || lane + 64 * i < TOTAL))
                            *reinterpret_cast<f32x4 *>(dst + i * (64 / C4) * CKP) = v[u];
                    }
                }
                __syncthreads();   // chunk ci is published; consumers are done with chunk ci-1
            }
        }
    } else {
        f32x16 acc[WTM][WTN];
#pragma unroll
        for (int tm = 0; tm < WTM; ++tm)
#pragma unroll
            for (int tn = 0; tn < WTN; ++tn)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[tm][tn][r] = 0.f;

        int a_off[WTM];
#pragma unroll
        for (int tm = 0; tm < WTM; ++tm)
            a_off[tm] = ((wm * WTM + tm) * NPIX + ((li >> 3) * S) * IW + (li & 7) * S) * CKP + 4 * g;

        const int Cin4 = a.Cin >> 2;
        const __amdgpu_buffer_rsrc_t r_w = make_rsrc(a.wpk, (unsigned)(Cfg::KH * Cfg::KW * a.Cin * a.CoutP) * 4u);
        const int w_lane = (g * a.CoutP + n0 + wn * WTN * 32 + li) * 16;   // bytes

        constexpr int K8 = CK / 8, NS = Cfg::KH * Cfg::KW * K8;
        auto load_b = [&](f32x4(&dst)[WTN], int kc, int s) {
            const int tap = s / K8, k8 = s % K8;
            const int soff = (tap * Cin4 + ((kc + k8 * 8) >> 2)) * a.CoutP * 16;
#pragma unroll
            for (int tn = 0; tn < WTN; ++tn) dst[tn] = buf_load4(r_w, w_lane + tn * 32 * 16, soff);
        };
        f32x4 bcur[WTN];
        load_b(bcur, 0, 0);
        const EpiCoef<WTN> coef = conv_epi_coef<WN, WTN, false>(a, n0, wn, li);
        const int nch = a.Cin / CK;
        __syncthreads();   // chunk 0 staged
        for (int ci = 0; ci < nch; ++ci) {
            const float *tile = lds + (ci & 1) * TILE;
            auto load_a = [&](f32x4(&dst)[WTM], int s) {
                const int tap = s / K8, k8 = s % K8;
#pragma unroll
                for (int tm = 0; tm < WTM; ++tm)
                    dst[tm] = *reinterpret_cast<const f32x4 *>(
                        &tile[a_off[tm] + ((tap / Cfg::KW) * IW + (tap % Cfg::KW)) * CKP + k8 * 8]);
            };
            const int kc = ci * CK;
            const int kc_next = (ci + 1 < nch) ? kc + CK : kc;
            f32x4 acur[WTM];
            load_a(acur, 0);
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                f32x4 anext[WTM], bnext[WTN];
                if (s + 1 < NS) {
                    load_a(anext, s + 1);
                    load_b(bnext, kc, s + 1);
                } else {
                    load_b(bnext, kc_next, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int tm = 0; tm < WTM; ++tm)
#pragma unroll
                        for (int tn = 0; tn < WTN; ++tn)
                            acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(
                                acur[tm][j], bcur[tn][j], acc[tm][tn], 0, 0, 0);
                if (s + 1 < NS) {
#pragma unroll
                    for (int tm = 0; tm < WTM; ++tm) acur[tm] = anext[tm];
                }
#pragma unroll
                for (int tn = 0; tn < WTN; ++tn) bcur[tn] = bnext[tn];
            }
            if (ci + 1 < nch) __syncthreads();   // chunk ci+1 staged, chunk ci released
        }
        conv_epilogue<WM, WN, WTM, WTN, BNT>(a, acc, pinfo, chunk * PB, img, n0, wm, wn, g, li, coef);
    }
}

// ---- launch: the build conv_plan() chose (p.shape, p.ck, p.bm; CONV_FP32_WS: the wave-specialised kernel)
template <int KS, int S, int CK, class Sh>
static hipError_t launch_one(const ConvPlan &p, hipStream_t st) {
    using Cfg = ConvCfg<KS, S, CK, Sh::WM, Sh::WN, Sh::WTM, Sh::WTN>;
    using CfgWS = ConvCfgWS<KS, S, CK, Sh::WM, Sh::WN, Sh::WTM, Sh::WTN>;
    static_assert(Cfg::PB == Sh::PB && Cfg::BNT == Sh::BNT, "the shape table and the kernel agree on the tile");
    const ConvArgs &a = p.a;
    const dim3 grid((unsigned)(a.B * a.chunks * (a.CoutP / Cfg::BNT)));
    if constexpr (KS == 3 || KS == 1)
        if (p.kernel == CONV_FP32_WS)
            return launch_dyn_lds<conv_mfma_ws_kernel<KS, S, CK, Sh::WM, Sh::WN, Sh::WTM, Sh::WTN>>(CfgWS::LDS_BYTES, grid, dim3(CfgWS::NT), st, a);
    // backward-statistics epilogue (ConvArgs::bm_y): its own instantiation, so that every other launch keeps the lean
    // epilogue (the y / z loads cost ~25 VGPRs)
    if constexpr (S == 1 && (KS == 3 || KS == 1))
        if (p.bm) return launch_dyn_lds<conv_mfma_kernel<KS, S, CK, Sh::WM, Sh::WN, Sh::WTM, Sh::WTN, true>>(Cfg::LDS_BYTES, grid, dim3(Cfg::NT), st, a);
    return launch_dyn_lds<conv_mfma_kernel<KS, S, CK, Sh::WM, Sh::WN, Sh::WTM, Sh::WTN, false>>(Cfg::LDS_BYTES, grid, dim3(Cfg::NT), st, a);
}

hipError_t launch_conv_fp32(const ConvPlan &p, hipStream_t st) {
    return with_conv_window(p.ks, p.stride, [&](auto win) {
        constexpr int KS = decltype(win)::KS, S = decltype(win)::S;
        return with_conv_shape(p.shape, [&](auto sh) {
            if constexpr (!(KS == 3 && S == 2))      // (conv_ck: a stride-2 3x3 always stages 16-channel chunks)
                if (p.ck == 32) return launch_one<KS, S, 32, decltype(sh)>(p, st);
            return launch_one<KS, S, 16, decltype(sh)>(p, st);
        });
    });
}

int conv_pick_cfg(int Cout, int CoutP, int ks, int stride, int B, int Hout, int Wout) {
    // Measured on MI355X at B=32 (scratch/tune_conv.py, profiles/r1_conv_shapes.txt): the shapes
    // are within ~10 % of each other; small 64-pixel groups win where the K loop is short (1x1)
    // because more, shorter workgroups balance better across the 256 CUs.
    (void)B; (void)Hout; (void)Wout; (void)CoutP;
    const int nt = conv_ntile(Cout);
    if (nt == 128) return ks == 1 ? CFG_64x128 : CFG_128x128;
    if (nt == 64) return (ks == 1 || stride == 2) ? CFG_64x64 : CFG_128x64m;
    return CFG_128x32;
}

}  // namespace mc
