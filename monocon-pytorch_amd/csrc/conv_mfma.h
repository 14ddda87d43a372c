// Fused implicit-GEMM convolution for gfx950 on the fp32 MFMA pipe: contract, dispatch tables and shared device helpers.
//
//   out[b,y,x,n] = act( scale[n] * sum_{src,c,r,s} in_src[b, y*S-P+r, x*S-P+s, c] * W[n, c, r, s]
//                       + bias[n] + residual[b,y,x,n] )
//
// Replaces nn.Conv2d(+torch.cat)+BatchNorm2d(eval)+ReLU(+residual) of the reference's BasicBlock /
// Root / Conv2dBlock / head 3x3 (model/backbone/dla.py:34-51,124-132; dla_neck.py:34-38;
// monocon_heads.py:114-120).
//
// Mapping (M = output pixels, N = output channels, K = taps x input channels):
//   * M is cut into 4x8-pixel patches (one 32-row MFMA tile each); a workgroup owns PB = WM*WTM
//     consecutive patches of ONE image and BNT = WN*WTN*32 output channels.
//   * v_mfma_f32_32x32x2_f32: exact fp32 FMA chain, 157 TF peak == the fp32 VALU peak but issued
//     from one wave per SIMD with the VALU left free for address math and the epilogue.
//   * A operand: the patch's input halo (IHxIW pixels x CK channels) is staged once per K-chunk in
//     LDS as [patch][pixel][CK+4] (NHWC => channels contiguous); every lane pulls 4 consecutive
//     channels of "its" pixel with one ds_read_b128, re-used across the 9 taps by address offset.
//   * B operand: weights are pre-packed as [tap][Cin/4][CoutP][4] so that the same lane->k mapping
//     (k-pair {c+j, c+4+j} for MFMA j of a group of 4) is one 16-byte global load per 32-column
//     tile straight from L2 -- the weights never occupy LDS.
//   * virtual concat: up to 4 source tensors are walked chunk by chunk; torch.cat is never
//     materialised.
//   * epilogue: folded-BN scale/shift or conv bias, residual add, ReLU, optional per-(image,
//     channel) sum / sum-of-squares partials (for AttnBN instance statistics / train-mode BN);
//     output (and residual) may be a strided scatter (o_px / o_row), used by the stride-2 data gradient.
//   * every global access is a buffer instruction: descriptor in SGPRs, lane offset resolved once,
//     wave-uniform SGPR offset per K-chunk / tap -- no vector address arithmetic in the K loop.
// Family: conv_mfma_kernel (this tiling) and conv_mfma_ws_kernel (producer wave + double-buffered LDS), both in
// conv_mfma.hip; conv_small_kernel (conv_small.hip: 16/32-channel layers on 16x16x4, no LDS), conv_bf16_kernel
// (conv_bf16.hip: bf16 operands, or fp32 emulated by a bf16 / fp16 split), conv_wres_kernel (conv_wres.hip) and
// conv_thin16_kernel (conv_thin.hip).  conv_plan() (conv_plan.hip) chooses among them once per launch description, from
// ConvArgs::cfg / ::prec and what each kernel file says it can run; launch_conv() looks the choice up.  Results of the fp32
// variants are bit-identical across workgroup shapes.
// This header is what the family shares: the contract (ConvArgs, ConvPlan, the shape ids and their table CONV_SHAPES, the
// prototypes), the host-side visitors and the one dynamic-LDS launcher (with_conv_shape, with_conv_window,
// launch_dyn_lds), and the device helpers every kernel file uses (the 16-bit vector types, Piece / mfma_k16, split_pair, buffer
// access, max-|x| slots, xcd_order, conv_wg, conv_epilogue).  No kernel is defined here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>
#include <type_traits>
#include <utility>

namespace mc {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// element type / vectors / MFMA of a split mode (conv_bf16.hip, wgrad_bf16.hip): SPL 1, 3 = bf16 pieces, SPL 2 = fp16 pieces
template <int SPL> struct Piece { typedef __bf16 T; typedef bf16x8 V8; typedef bf16x4 V4; typedef bf16x2 V2; };
template <> struct Piece<2> { typedef _Float16 T; typedef f16x8 V8; typedef f16x4 V4; typedef f16x2 V2; };
__device__ __forceinline__ f32x16 mfma_k16(bf16x8 a, bf16x8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f32x16 mfma_k16(f16x8 a, f16x8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }

// (x0, x1) * s -> packed fp16 pair of the hi pieces and of the lo pieces, four instructions: v_fma_mix{lo,hi}_f16 computes
// fma(a, b, c) in fp32 (sources fp32 or one half of a register) and rounds once to fp16 -- hi = f16(x * s), lo = f16(x * s - hi),
// each ONE rounding of an exact fp32 value: the same bits as the cvt / sub / cvt sequence of conv_bf16_kernel
// (conv_wres.hip, wgrad_pipe.hip)
__device__ __forceinline__ void split_pair(float x0, float x1, float s, unsigned &hi, unsigned &lo) {
    unsigned h, l;
    asm("v_fma_mixlo_f16 %0, %1, %2, 0" : "=v"(h) : "v"(x0), "v"(s));
    asm("v_fma_mixhi_f16 %0, %1, %2, 0" : "+v"(h) : "v"(x1), "v"(s));
    asm("v_fma_mixlo_f16 %0, %1, %2, -%3 op_sel_hi:[0,0,1]" : "=v"(l) : "v"(x0), "v"(s), "v"(h));
    asm("v_fma_mixhi_f16 %0, %1, %2, -%3 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "+v"(l) : "v"(x1), "v"(s), "v"(h));
    hi = h;
    lo = l;
}

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is a property of (function, DEVICE): a process-wide "already set" flag would
// launch a second handle's kernels on another GPU without it.  One bit per device in a per-instantiation mask;
// racing threads at worst set the attribute twice.
struct DynLdsOnce {
    std::atomic<unsigned long long> done{0};
    hipError_t ensure(const void *fn, int bytes) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
        if ((done.load(std::memory_order_acquire) >> dev) & 1ull) return hipSuccess;
        const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
        if (e == hipSuccess) done.fetch_or(1ull << dev, std::memory_order_release);
        return e;
    }
};

struct ConvSrc {
    const float *p;
    int C;
    // "Lazy" activation (train plans of precision mode 3, round 6): p holds the RAW conv output y of the producing layer and
    // the tensor's value is max(fma(y, la[c], lb[c]), 0) -- train-mode BatchNorm apply + ReLU, formed by the CONSUMER
    // while it stages the operand (one fma + one v_med3 on top of the scale-and-split it pays anyway), so the activation is
    // never written to HBM.  Zero padding stays zero (not relu(lb)): lazy_act()'s `cap`.  null: p holds the values.
    // Scaling by a power of two commutes with the fma's rounding, so the staged pieces are bit-identical to those of the
    // stored activation under the same operand scale (the scale itself comes from a sound BOUND of max |z| in this case,
    // written by bn_finalize_kernel; the stored activation's slot holds its exact maximum).
    const float *la, *lb;
};
// one lazy element: a = la[c] * 2^e, b = lb[c] * 2^e (the operand scale folded into the coefficients), cap = +inf inside the
// image, 0 on padding.  v_med3_f32(t, 0, cap) = min(max(t, 0), cap) is the ReLU and the padding mask in one instruction.
__device__ __forceinline__ float lazy_act(float y, float a, float b, float cap) {
    return __builtin_amdgcn_fmed3f(__builtin_fmaf(y, a, b), 0.f, cap);
}

struct ConvArgs {
    ConvSrc src[4];
    int nsrc;
    int B, Hin, Win, Hout, Wout;
    int Cin;                 // total input channels of the virtual concat
    int Cout, CoutP;         // CoutP: packed/padded column count (multiple of the N tile)
    const float *wpk;        // [k*k][Cin/4][CoutP][4]
    const float *scale;      // [Cout] or null (1)
    const float *bias;       // [Cout] or null (0)
    const float *res;        // NHWC [B,Hout,Wout,res_ld] or null
    int res_ld;
    float *out;              // NHWC, channel stride out_ld, channel offset out_coff
    int out_ld, out_coff;
    int relu;
    float *stats;            // optional [B][patches per image][CoutP][2] partial (sum, sumsq) of (v - shift), per 4x8 patch
    const float *stat_shift; // [Cout] or null
    // 1: the second partial is the patch's CENTRED second moment sum (d - m)^2, d = v - shift, m = (patch sum) / 32, instead of
    // sum d^2: a consumer combines the patches by Chan's formula (head_attn_kernel), and a map that is flat beside its offset
    // from `shift` no longer cancels in fp32 ((mean - shift)^2 / var = 1e4 cost 3e-4 of s = mean / sqrt(var), now 1e-6).
    // Whole 4x8 patches without a residual only: the eval plan's fused head conv.  The order within a patch is fixed by the
    // MFMA layout as before, so the partials stay independent of the workgroup shape.
    int stats_centred;
    int ppr, ppi, chunks;    // patches per row / per image, workgroup chunks per image
    int cfg;                 // ConvCfgId workgroup shape (CFG_AUTO = conv_pick_cfg)
    // output / residual pixel mapping in floats (0 = dense NHWC: img = Hout*Wout*ld, row = Wout*ld, px = ld);
    // the stride-2 data-gradient classes scatter to every second pixel of a larger map
    int o_img, o_row, o_px, r_img, r_row, r_px;
    // conv_bf16.hip: prec 1 = bf16 MFMA operands from the bf16 panel wpk16 (fp32 everything else); prec 2 = fp32
    // emulated by a 3-way bf16 split of both operands (six bf16 MFMAs per product, three panels in wpk16)
    const void *wpk16;       // [pieces][k*k][Cin/8][CoutP][8] bf16 or null
    int prec;
    // backward-statistics mode, for a data gradient whose output completes the gradient of a BatchNorm'd map (dense
    // NHWC, Cout channels): the epilogue applies that map's ReLU mask to the total (accumulated) gradient d, stores
    // the masked d, and writes the (sum d, sum d*y) partials of the BatchNorm backward to `stats` (per 4x8 patch) --
    // the separate three-tensor reduction pass over the activation disappears
    const float *bm_y;       // pre-BN conv output y of the forward, or null (mode off)
    const float *bm_z;       // post-BN map z (mask z > 0), bm_relu == 1
    // round 6: the same mask BIT-PACKED, [pixel][Cout / 32] words (bit c % 32 of word c / 32 = z[pixel][c] > 0), written by the
    // forward's affine_act pass of a residual layer (the only layers whose mask cannot be recomputed from y alone): the
    // epilogue then reads one broadcast word per row instead of one float per lane -- 1/32 of the bytes (252 MB -> 8 MB for a
    // 64-channel 96x320 map at B = 32).  Optional; with it bm_z is not read.  Cout % 32 == 0.
    const unsigned *bm_zbits;
    const float *bm_a, *bm_b;// forward BN coefficients (mask fma(y, a, b) > 0, bit-identical to z > 0), bm_relu == 2
    int bm_relu;             // 0: no ReLU (no mask), 1, 2
    // prec 3 (conv_bf16.hip, fp32 emulated by a 2-way fp16 split): both operands are scaled by a power of two derived
    // from their tensor's max |x| so that they sit in fp16's range; the slots hold the BIT PATTERN of that maximum
    // (a non-negative float orders like its bits), written by whoever produced the tensor (amax_update_* below; a
    // tensor's slot is AMAX_SUB sub-slots, a weight's slot one word)
    const unsigned *amax_in[4];   // per source of the virtual concat
    const unsigned *amax_w;       // of the master weight(s) the panel was cut from
    unsigned *amax_out;           // optional: max |out| of this launch is folded in (eval plans: the consumer's amax_in)
    unsigned long long *phase_prof;   // measurement aid (-DMC_PHASE_TIMERS, mc_bench_conv): per workgroup and wave, cycles spent in
                                      // [0] staging, [1] barriers, [2] MFMA phases, [3] epilogue, [4] total
};

// ---- power-of-two operand scaling of the fp16-split mode ---------------------------------------------------------
// scale exponent of a tensor whose max |x| has the bit pattern `amax_bits`: max |x| * 2^e lands in [2^14, 2^15) (fp16
// overflows at 65504).  An all-zero (or denormal-max) tensor keeps e = 0; e stays within what exp2i() can represent.
// The output rescale is formed as the PRODUCT 2^-e_a * 2^-e_w, which leaves the float range only where the true
// result does.
__host__ __device__ __forceinline__ int f16_scale_exp(unsigned amax_bits) {
    const int E = (int)((amax_bits >> 23) & 0xffu);
    if (E == 0) return 0;
    const int e = 141 - E;
    return e > 126 ? 126 : e;
}
__host__ __device__ __forceinline__ float exp2i(int e) {     // 2^e, -126 <= e <= 127
    const unsigned u = (unsigned)(127 + e) << 23;
    return __builtin_bit_cast(float, u);
}
// ---- the max-|x| slots ------------------------------------------------------------------------------------------
// A tensor's slot is AMAX_SUB words, AMAX_STRIDE words (256 bytes) apart; its maximum is the largest of them.  Every
// workgroup of a producing launch folds its own maximum into sub-slot (blockIdx.x % AMAX_SUB), and only when that can
// still raise it (a relaxed read first; a stale value merely costs a redundant atomic).  Why not one word and one
// atomic per lane: measured (round 3, rocprofv3) -- ~32 k same-address requests per launch serialise in one L2 channel
// at ~1.5 ns each: +55 us on a 55 us element-wise pass.  One request per workgroup, spread over 16 channels, is noise.
// Inf / NaN never enter a slot (they propagate through the data instead).  Weight slots are single words (amax_w).
constexpr int AMAX_SUB = 16, AMAX_STRIDE = 64, AMAX_WORDS = AMAX_SUB * AMAX_STRIDE;
__device__ __forceinline__ void amax_commit(unsigned *slot, unsigned bits) {       // call from ONE lane per workgroup / wave
    unsigned *p = slot + (blockIdx.x % AMAX_SUB) * AMAX_STRIDE;
    if (bits < 0x7f800000u && bits > __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(p, bits);
}
// every thread of the workgroup calls this (partially filled waves are fine: the reduction goes through LDS atomics)
__device__ __forceinline__ void amax_update_block(unsigned *slot, float v) {
    __shared__ unsigned s_amax;
    if (threadIdx.x == 0) s_amax = 0u;
    __syncthreads();
    const unsigned bits = __builtin_bit_cast(unsigned, v);
    if (bits < 0x7f800000u && bits != 0u) atomicMax(&s_amax, bits);
    __syncthreads();
    if (threadIdx.x == 0) amax_commit(slot, s_amax);
}
// full 64-lane waves only (the MFMA kernels' epilogues): one commit per wave
__device__ __forceinline__ void amax_update_wave(unsigned *slot, float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    if ((threadIdx.x & 63) == 0) amax_commit(slot, __builtin_bit_cast(unsigned, v));
}
// the tensor's maximum (bit pattern), wave-uniform; full 64-lane waves only
__device__ __forceinline__ unsigned amax_read(const unsigned *slot) {
    const int lane = threadIdx.x & 63;
    unsigned v = lane < AMAX_SUB ? slot[lane * AMAX_STRIDE] : 0u;
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) { const unsigned t = (unsigned)__shfl_xor((int)v, o); v = t > v ? t : v; }
    return (unsigned)__builtin_amdgcn_readfirstlane((int)v);
}

// Filter window code KS: 3 = 3x3 (pad 1), 1 = 1x1; 12 / 21 / 22 = 1x2, 2x1, 2x2 windows without padding --
// the four output-parity classes of a stride-2 3x3 data gradient (dX[2i+py][2j+px] only sees the taps
// of matching parity, see mc_train_plan.hip emit_dgrad), launched with a strided output mapping.
constexpr int win_h(int ks) { return ks >= 10 ? ks / 10 : ks; }
constexpr int win_w(int ks) { return ks >= 10 ? ks % 10 : ks; }
constexpr int win_pad(int ks) { return ks == 3 ? 1 : 0; }

template <int KS, int S, int CK, int WM, int WN, int WTM, int WTN>
struct ConvCfg {
    static constexpr int PB = WM * WTM;
    static constexpr int BNT = WN * WTN * 32;
    static constexpr int NT = 64 * WM * WN;
    static constexpr int KH = win_h(KS), KW = win_w(KS);
    static constexpr int PAD = win_pad(KS);
    static constexpr int IH = 3 * S + KH;
    static constexpr int IW = 7 * S + KW;
    static constexpr int NPIX = IH * IW;
    static constexpr int CKP = CK + 4;
    static constexpr int LDS_FLOATS = PB * NPIX * CKP + PB * 4;
    static constexpr size_t LDS_BYTES = sizeof(float) * LDS_FLOATS;
};

// Buffer-addressed memory access: every global access of the kernel goes through a buffer
// resource (SGPR descriptor) + one lane offset kept in a VGPR + a wave-uniform SGPR offset, so
// the K loop issues no vector-ALU address arithmetic at all -- on CDNA the MFMA shares the VALU
// issue port, and every v_mad/v_cndmask of ANY wave on the SIMD displaces matrix issue slots
// (measured: a staging wave next to an MFMA wave advances ~10x slower than alone).  Offsets
// >= num_records read as zero / drop the store, which also replaces the halo and edge branches.
constexpr int BUF_OOB = (int)0x80000000;
typedef int i32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void *base, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(base), 0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ f32x4 buf_load4(__amdgpu_buffer_rsrc_t r, int voff, int soff) {
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0));
}
__device__ __forceinline__ float buf_load1(__amdgpu_buffer_rsrc_t r, int voff, int soff) {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, 0));
}
__device__ __forceinline__ void buf_store1(float v, __amdgpu_buffer_rsrc_t r, int voff, int soff) {
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, v), r, voff, soff, 0);
}

// Workgroup b is observed to run on XCD b % 8 (MI355X_MICROARCH.md, "Workgroup dispatch, XCD placement": a speed
// hint, never relied on for correctness).  xcd_order() renumbers the grid so that every XCD walks ONE contiguous
// range of logical workgroups: neighbouring pixel chunks (shared halo rows) and the column tiles of a chunk (same
// input) then meet in the same 4 MB L2 instead of being fetched once per XCD.  Bijective for any grid size.
// MEASURED (A/B on one box, B=32; scratch/traffic_ab.sh): HBM read traffic per launch 458 -> 264 MB for the conv /
// data-gradient kernels (algorithmic: ~240 MB of reads), 700 -> 373 MB for the weight gradients, 1421 -> 1080 MB for
// the 16-channel row kernel -- i.e. the halo and column-tile re-reads that used to go out to the fabric once per
// XCD now hit in L2.  These kernels are MFMA-bound, so the time barely moves (train step 105.3-106.0 vs 105.6-105.9
// ms, eval forward B=32 +1 %, B=8 -1 %); the remap is kept for the traffic (-DMC_XCD_ORDER=0 compiles it out).
#ifndef MC_XCD_ORDER
#define MC_XCD_ORDER 1
#endif
__device__ __forceinline__ int xcd_order(int b, int n) {
    if (!MC_XCD_ORDER) return b;
    const int xcd = b & 7, idx = b >> 3, q = n >> 3, r = n & 7;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

// The workgroup's place in the launch: image, chunk of PB patches, first column n0 of its BNT-column tile.  Shared by
// conv_mfma_kernel, conv_mfma_ws_kernel and conv_bf16_kernel.  (Results as reference parameters, statements in this order:
// returning them as a struct, or factoring the pinfo fill that follows in the kernels the same way, moved the kernarg load
// of a.chunks and with it the schedule of the prologue in some instantiations.)
template <int BNT>
__device__ __forceinline__ void conv_wg(const ConvArgs &a, int &img, int &chunk, int &n0) {
    const int ntiles = a.CoutP / BNT;
    const int bid = xcd_order(blockIdx.x, gridDim.x);
    const int nt = bid % ntiles;
    const int mchunk = bid / ntiles;
    img = mchunk / a.chunks, chunk = mchunk % a.chunks;
    n0 = nt * BNT;
}

// Epilogue shared by both kernel variants.  C/D layout of v_mfma_f32_32x32x2: column = lane&31,
// row m = (r&3) + 8*(r>>2) + 4*(lane>>5); row m of a 4x8 patch is pixel (oy0 + (m>>3), ox0 + (m&7))
// = (oy0 + (r>>2), ox0 + (r&3) + 4*(lane>>5)).
// per-column coefficients of the epilogue.  Loaded BEFORE the K loop (conv_epi_coef): they are plain global loads, and
// fetched at the top of the epilogue each workgroup paid a full memory round trip for them with nothing to overlap
// (measured with the phase timers of mc_bench_conv, round 3: the epilogue took half as long as the workgroup's own MFMAs).
template <int WTN>
struct EpiCoef {
    float sc[WTN], bi[WTN], sh[WTN], ma[WTN], mb[WTN];
};
template <int WN, int WTN, bool BM>
__device__ __forceinline__ EpiCoef<WTN> conv_epi_coef(const ConvArgs &a, int n0, int wn, int li) {
    EpiCoef<WTN> c;
#pragma unroll
    for (int tn = 0; tn < WTN; ++tn) {
        const int n = n0 + (wn * WTN + tn) * 32 + li;
        const bool nok = n < a.Cout;
        c.sc[tn] = (a.scale && nok) ? a.scale[n] : 1.f;
        c.bi[tn] = (a.bias && nok) ? a.bias[n] : 0.f;
        c.sh[tn] = (a.stat_shift && nok) ? a.stat_shift[n] : 0.f;
        c.ma[tn] = (BM && a.bm_relu == 2 && nok) ? a.bm_a[n] : 0.f;
        c.mb[tn] = (BM && a.bm_relu == 2 && nok) ? a.bm_b[n] : 0.f;
    }
    return c;
}

template <int WM, int WN, int WTM, int WTN, int BNT, bool BM = false>
__device__ __forceinline__ void conv_epilogue(const ConvArgs &a, f32x16 (&acc)[WTM][WTN], const int *pinfo,
                                              int patch0, int img, int n0, int wm, int wn, int g, int li,
                                              const EpiCoef<WTN> &coef, float omul = 1.f, float *vmax_acc = nullptr) {
    // Every multiply-add below is written as the fma it is meant to be, and nothing else may be contracted: with
    // -ffp-contract=fast the choice is the optimiser's, PER INSTANTIATION -- and the kernels that share this epilogue
    // promise bit-identical results (round 5: one copy of `v = acc * sc + bi; v += res` came out differently for one r).
#pragma clang fp contract(off)
    // omul: power-of-two rescale of the accumulator (fp16-split mode: undoes the operand scaling, exact); 1 otherwise
    // vmax_acc: a persistent caller (conv_wres.hip) collects this lane's max |stored value| over its calls here and commits
    // ConvArgs::amax_out once itself (amax_commit waits for a returned load: once per workgroup, not once per tile)
    const bool do_stats = a.stats != nullptr;
    float vmax = 0.f;                            // max |stored value| of this lane (ConvArgs::amax_out)
    const bool has_res = a.res != nullptr;
    constexpr bool bm = BM;                      // backward-statistics mode (see ConvArgs): its own instantiation
    const int bm_relu = a.bm_relu;
    const float floor_v = a.relu ? 0.f : -__builtin_inff();
    const __amdgpu_buffer_rsrc_t r_out = make_rsrc(a.out + (size_t)img * a.o_img, (unsigned)a.o_img * 4u);
    const __amdgpu_buffer_rsrc_t r_res =
        make_rsrc(has_res ? a.res + (size_t)img * a.r_img : a.out, has_res ? (unsigned)a.r_img * 4u : 0u);
    const __amdgpu_buffer_rsrc_t r_y = make_rsrc(bm ? a.bm_y + (size_t)img * a.o_img : a.out, bm ? (unsigned)a.o_img * 4u : 0u);
    // the stored mask: floats (dense layout of the output) or, when bm_zbits is given, one word per pixel and 32 channels
    const bool zbits = bm && bm_relu == 1 && a.bm_zbits != nullptr;
    const int zwords = a.Cout >> 5;                                     // words per pixel of the bit-packed mask
    const unsigned zimg = zbits ? (unsigned)(a.Hout * a.Wout * zwords) * 4u : (unsigned)a.o_img * 4u;      // bytes per image
    const __amdgpu_buffer_rsrc_t r_z =
        make_rsrc(bm && bm_relu == 1 ? (zbits ? reinterpret_cast<const float *>(a.bm_zbits) + (size_t)img * a.Hout * a.Wout * zwords
                                              : a.bm_z + (size_t)img * a.o_img)
                                     : a.out,
                  bm && bm_relu == 1 ? zimg : 0u);
    // statistics partials are per 4x8 PATCH and channel: stats[b][patch][CoutP][2].  A patch's 32 values are
    // summed in an order fixed by the MFMA layout, so the partials -- and with them train-mode BN -- do not depend
    // on the workgroup shape the autotuner picked.
#pragma unroll
    for (int tn = 0; tn < WTN; ++tn) {
        const int n = n0 + (wn * WTN + tn) * 32 + li;
        const bool nok = n < a.Cout;
        const float sc = coef.sc[tn] * omul, bi = coef.bi[tn], sh = coef.sh[tn], ma = coef.ma[tn], mb = coef.mb[tn];
        const int v_out = nok ? (4 * g * a.o_px + a.out_coff + n) * 4 : BUF_OOB;
        const int v_res = nok ? (4 * g * a.r_px + n) * 4 : BUF_OOB;
        const int v_bm = nok ? (4 * g * a.o_px + n) * 4 : BUF_OOB;      // y / z share the dense layout of the output
        const int v_zb = nok ? (4 * g * zwords + (n >> 5)) * 4 : BUF_OOB;   // bit-packed mask: word n / 32 of pixel (ox0 + 4g + ..)
#pragma unroll
        for (int tm = 0; tm < WTM; ++tm) {
            const int p = wm * WTM + tm;
            const int oy0 = __builtin_amdgcn_readfirstlane(pinfo[p * 4 + 1]);
            const int ox0 = __builtin_amdgcn_readfirstlane(pinfo[p * 4 + 2]);
            const int pv = __builtin_amdgcn_readfirstlane(pinfo[p * 4 + 3]);
            if (!pv) continue;
            float ssum = 0.f, ssq = 0.f;
            if (oy0 + 4 <= a.Hout && ox0 + 8 <= a.Wout) {
                // whole patch inside the image: wave-uniform offsets only.  One straight-line copy of the body per
                // (residual, stored-mask) combination: with the optional loads under run-time conditions in ONE body, hipcc
                // places the s_waitcnt vmcnt(N) of the loaded values behind the join -- and on the paths WITHOUT those loads
                // the same waits then count the patch's own stores (gfx950 retires stores on vmcnt too): every second store
                // waited for the write acknowledgement of an earlier one (round 5, found in the ISA of conv_wres_kernel).
                const int s_out = (oy0 * a.o_row + ox0 * a.o_px) * 4;
                const int s_res = (oy0 * a.r_row + ox0 * a.r_px) * 4;
                auto body = [&](auto res_c, auto zmask_c) {
                    constexpr bool RES = decltype(res_c)::value, ZMASK = decltype(zmask_c)::value;
                    float rv[16], yv[16], zv[16];
                    if constexpr (RES) {
#pragma unroll
                        for (int r = 0; r < 16; ++r)
                            rv[r] = buf_load1(r_res, v_res, s_res + ((r >> 2) * a.r_row + (r & 3) * a.r_px) * 4);
                    }
                    if constexpr (bm) {
#pragma unroll
                        for (int r = 0; r < 16; ++r)
                            yv[r] = buf_load1(r_y, v_bm, s_out + ((r >> 2) * a.o_row + (r & 3) * a.o_px) * 4);
                        if constexpr (ZMASK) {
                            if (zbits) {       // (wave-uniform) one word per row, the same for the 32 lanes of a half wave
                                const int s_zb = (oy0 * a.Wout + ox0) * zwords * 4;
#pragma unroll
                                for (int r = 0; r < 16; ++r) {
                                    const unsigned w = __builtin_bit_cast(unsigned, buf_load1(r_z, v_zb, s_zb + ((r >> 2) * a.Wout + (r & 3)) * zwords * 4));
                                    zv[r] = ((w >> (n & 31)) & 1u) ? 1.f : 0.f;
                                }
                            } else {
#pragma unroll
                                for (int r = 0; r < 16; ++r)
                                    zv[r] = buf_load1(r_z, v_bm, s_out + ((r >> 2) * a.o_row + (r & 3) * a.o_px) * 4);
                            }
                        }
                    }
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        float v = __builtin_fmaf(acc[tm][tn][r], sc, bi);
                        if constexpr (RES) v += rv[r];
                        if constexpr (bm) {
                            const bool on = ZMASK ? zv[r] > 0.f : (bm_relu == 0 || fmaf(yv[r], ma, mb) > 0.f);
                            v = on ? v : 0.f;
                            ssum += v;
                            ssq = fmaf(v, yv[r], ssq);
                        } else if (do_stats) {
                            const float d = v - sh;
                            ssum += d;
                            ssq += d * d;      // (two roundings: contraction is off in this function)
                        }
                        v = fmaxf(v, floor_v);
                        vmax = fmaxf(vmax, fabsf(v));
                        buf_store1(v, r_out, v_out, s_out + ((r >> 2) * a.o_row + (r & 3) * a.o_px) * 4);
                    }
                };
                using T = std::true_type;
                using Fz = std::false_type;
                const bool zmask = bm && bm_relu == 1;
                if (has_res) { if (zmask) body(T{}, T{}); else body(T{}, Fz{}); }
                else { if (zmask) body(Fz{}, T{}); else body(Fz{}, Fz{}); }
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int y = oy0 + (r >> 2), x = ox0 + (r & 3) + 4 * g;
                    if (nok && y < a.Hout && x < a.Wout) {
                        float v = __builtin_fmaf(acc[tm][tn][r], sc, bi);
                        if (has_res) v += buf_load1(r_res, (y * a.r_row + x * a.r_px + n) * 4, 0);
                        if (bm) {
                            const float yy = buf_load1(r_y, (y * a.o_row + x * a.o_px + n) * 4, 0);
                            bool on = true;
                            if (bm_relu == 1)
                                on = zbits ? ((__builtin_bit_cast(unsigned, buf_load1(r_z, ((y * a.Wout + x) * zwords + (n >> 5)) * 4, 0)) >> (n & 31)) & 1u) != 0u
                                           : buf_load1(r_z, (y * a.o_row + x * a.o_px + n) * 4, 0) > 0.f;
                            else if (bm_relu == 2) on = fmaf(yy, ma, mb) > 0.f;
                            v = on ? v : 0.f;
                            ssum += v;
                            ssq = fmaf(v, yy, ssq);
                        } else {
                            const float d = v - sh;
                            ssum += d;
                            ssq += d * d;      // (two roundings: contraction is off in this function)
                        }
                        v = fmaxf(v, floor_v);
                        vmax = fmaxf(vmax, fabsf(v));
                        buf_store1(v, r_out, (y * a.o_row + x * a.o_px + a.out_coff + n) * 4, 0);
                    }
                }
            }
            if (do_stats) {
                ssum += __shfl_xor(ssum, 32);
                if constexpr (!bm) {
                    if (a.stats_centred) {       // (wave-uniform) ConvArgs::stats_centred: a second pass over the accumulators
                        const float m = ssum * 0.03125f;
                        ssq = 0.f;
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const float e = (__builtin_fmaf(acc[tm][tn][r], sc, bi) - sh) - m;
                            ssq = __builtin_fmaf(e, e, ssq);
                        }
                    }
                }
                ssq += __shfl_xor(ssq, 32);
                if (g == 0 && nok) {
                    float *dst = a.stats + (((size_t)img * a.ppi + patch0 + p) * a.CoutP + n) * 2;
                    dst[0] = ssum;
                    dst[1] = ssq;
                }
            }
        }
    }
    if (vmax_acc) *vmax_acc = fmaxf(*vmax_acc, vmax);
    else if (a.amax_out) amax_update_wave(a.amax_out, vmax);
}

// ---- host-side tile selection ---------------------------------------------------------
// Workgroup shapes (WM x WN waves, each wave WTM x WTN 32x32 MFMA tiles).  A shape owns
// PB = WM*WTM patches (32 output pixels each) and BNT = WN*WTN*32 output channels.
enum ConvCfgId {
    CFG_AUTO = 0,
    CFG_128x128 = 1,    // 2x2 waves, 2x2 tiles : 128 px x 128 ch
                        // (2, 3 -- 256 x 64, 256 x 32 -- are retired and no shape id any more: 8-patch shapes never won and
                        // spill under the 3-waves/SIMD cap)
    CFG_128x64 = 4,     // 2x2 waves, 2x1 tiles : 128 px x  64 ch
    CFG_128x64m = 5,    // 4x1 waves, 1x2 tiles : 128 px x  64 ch (waves split M only)
    CFG_128x32 = 6,     // 4x1 waves, 1x1 tiles : 128 px x  32 ch
    CFG_64x128 = 7,     // 1x4 waves, 2x1 tiles :  64 px x 128 ch
    CFG_64x64 = 8,      // 2x2 waves, 1x1 tiles :  64 px x  64 ch
    CFG_SHAPE_BITS = 15,
    CFG_WS = 16,        // flag: wave-specialised kernel (producer wave + double-buffered LDS)
    CFG_SMALL = 32,     // LDS-free 16x16x4 kernel for 16/32-channel 3x3 layers (conv_small.hip)
    CFG_WRES = 64       // flag: weight-resident persistent kernel (conv_wres.hip) where the launch is eligible; the shape
                        // bits name the tiling every other launch with this id takes (results are bit-identical)
};
// THE table of tilings: an id is a shape id exactly when it has an entry, and every entry has a kernel in each family
// (conv_mfma.hip plain + WS, conv_bf16.hip).  conv_shape() reads it at run time, with_conv_shape() at compile time.
struct ConvShape {
    int id, WM, WN, WTM, WTN;
    constexpr int PB() const { return WM * WTM; }
    constexpr int BNT() const { return WN * WTN * 32; }
};
constexpr ConvShape CONV_SHAPES[] = {
    {CFG_128x128, 2, 2, 2, 2}, {CFG_128x64, 2, 2, 2, 1}, {CFG_128x64m, 4, 1, 1, 2},
    {CFG_128x32, 4, 1, 1, 1},  {CFG_64x128, 1, 4, 2, 1}, {CFG_64x64, 2, 2, 1, 1},
};
constexpr int CONV_NSHAPES = (int)(sizeof(CONV_SHAPES) / sizeof(CONV_SHAPES[0]));
// the shape the bits `cfg & CFG_SHAPE_BITS` name; all zero (id 0) when they name none
inline ConvShape conv_shape(int cfg) {
    for (const ConvShape &s : CONV_SHAPES)
        if (s.id == (cfg & CFG_SHAPE_BITS)) return s;
    return {0, 0, 0, 0, 0};
}
// entry I as a type: what a kernel family instantiates on
template <int I>
struct ConvShapeC {
    static constexpr int WM = CONV_SHAPES[I].WM, WN = CONV_SHAPES[I].WN, WTM = CONV_SHAPES[I].WTM, WTN = CONV_SHAPES[I].WTN;
    static constexpr int PB = CONV_SHAPES[I].PB(), BNT = CONV_SHAPES[I].BNT();
};
template <typename F, int... I>
inline hipError_t with_conv_shape_seq(int id, F &f, std::integer_sequence<int, I...>) {
    hipError_t e = hipErrorInvalidValue;
    (void)((CONV_SHAPES[I].id == id && ((e = f(ConvShapeC<I>{})), true)) || ...);
    return e;
}
// f(ConvShapeC<I>{}) for the entry `cfg`'s shape bits name; hipErrorInvalidValue when they name none
template <typename F>
inline hipError_t with_conv_shape(int cfg, F &&f) {
    return with_conv_shape_seq(cfg & CFG_SHAPE_BITS, f, std::make_integer_sequence<int, CONV_NSHAPES>{});
}
// The filter window as a type.  f(ConvWin<KS, S>{}) for the (window code, stride) pairs that have kernels: 3x3 stride 1 / 2,
// 1x1, and the three parity classes of a stride-2 data gradient; hipErrorInvalidValue otherwise.
template <int KS_, int S_>
struct ConvWin { static constexpr int KS = KS_, S = S_; };
template <typename F>
inline hipError_t with_conv_window(int ks, int stride, F &&f) {
    if (ks == 3 && stride == 1) return f(ConvWin<3, 1>{});
    if (ks == 3 && stride == 2) return f(ConvWin<3, 2>{});
    if (stride != 1) return hipErrorInvalidValue;
    if (ks == 1) return f(ConvWin<1, 1>{});
    if (ks == 12) return f(ConvWin<12, 1>{});
    if (ks == 21) return f(ConvWin<21, 1>{});
    if (ks == 22) return f(ConvWin<22, 1>{});
    return hipErrorInvalidValue;
}

// One launch of a kernel with dynamic LDS.  Owns the DynLdsOnce of its kernel (one instantiation per kernel: Kern is a
// template argument), refuses a request above the 160 KB of a CU, launches and returns hipGetLastError().
template <auto Kern, typename... Args>
inline hipError_t launch_dyn_lds(size_t lds_bytes, dim3 grid, dim3 block, hipStream_t st, const Args &...args) {
    if (lds_bytes > 160 * 1024) return hipErrorInvalidValue;
    static DynLdsOnce attr_set;
    const hipError_t e = attr_set.ensure(reinterpret_cast<const void *>(Kern), (int)lds_bytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(Kern, grid, block, lds_bytes, st, args...);
    return hipGetLastError();
}

// Column padding of the packed weights for a layer with Cout columns (every shape's BNT that
// may be chosen for the layer divides it).
inline int conv_ntile(int Cout) { return Cout >= 128 ? 128 : (Cout > 32 ? 64 : 32); }
inline int conv_coutp(int Cout) {
    const int t = conv_ntile(Cout);
    return (Cout + t - 1) / t * t;
}
// output extent of a k x k window with padding k / 2
inline int conv_out_dim(int in, int ks, int stride) { return (in + 2 * (ks / 2) - ks) / stride + 1; }
// 16-bit pieces per weight / activation element in precision mode `prec`: one bf16, three bf16 (mode 2), two fp16 (mode 3)
inline int split_pieces(int prec) { return prec == 2 ? 3 : (prec == 3 ? 2 : 1); }
// K-chunk: 32 when every source is a multiple of 32 channels and the 3x3 is stride 1 (or 1x1).
inline int conv_ck(int ks, int stride, const int *src_c, int nsrc) {
    bool all32 = true;
    for (int i = 0; i < nsrc; ++i) all32 = all32 && (src_c[i] % 32 == 0);
    if (ks == 3 && stride == 2) return 16;
    return all32 ? 32 : 16;
}
// Default shape for a layer (tuned on MI355X): depends on the column count, the
// stride (stride-2 halos are 9x17 pixels per patch, so fewer patches per workgroup keep several
// workgroups resident per CU) and on how many workgroups the launch would have.
int conv_pick_cfg(int Cout, int CoutP, int ks, int stride, int B, int Hout, int Wout);
// does any source carry lazy coefficients (ConvSrc::la)?
inline bool any_lazy_src(const ConvSrc *src, int nsrc) {
    for (int i = 0; i < nsrc; ++i)
        if (src[i].la) return true;
    return false;
}
inline bool conv_any_lazy(const ConvArgs &a) { return any_lazy_src(a.src, a.nsrc); }

// ---- one conv launch: the block and, host side, what conv_plan() decided (conv_plan.hip).  conv_fwd_args() (mc_internal.h) and
//      dgrad_conv_args() (train.h) fill one.  ConvArgs is the kernels' parameter block: the hidden arguments (gridDim) lie
//      behind it, so its layout is part of their machine code.
static_assert(sizeof(ConvArgs) == 416, "ConvArgs is the kernels' parameter block: keep its layout");
enum ConvKernel {
    CONV_FP32,        // conv_mfma_kernel (conv_mfma.hip): the fp32 tilings
    CONV_FP32_WS,     // conv_mfma_ws_kernel: the same tilings, wave-specialised
    CONV_SPLIT,       // conv_bf16_kernel (conv_bf16.hip): the tilings on 16-bit pieces, modes 1..3
    CONV_WRES,        // conv_wres_kernel (conv_wres.hip): weight-resident, persistent
    CONV_ROW,         // conv_small_kernel (conv_small.hip): the 16 / 32-channel row kernel
    CONV_ROW_LAZY,    // conv_small_kernel<2, 16, 2, true>: its build that forms a lazy source
    CONV_THIN16       // conv_thin16_kernel (conv_thin.hip): the 16 -> 16 row kernel on the fp16 pipe
};
struct ConvPlan {
    ConvArgs a;               // conv_plan() alone writes ppr / ppi / chunks and the dense pixel mapping (o_* / r_* given as 0)
    int ks, stride;           // window code (win_h / win_w) and stride
    int kernel;               // ConvKernel
    int shape, ck, spl;       // the tilings: shape id (CFG_AUTO and the flags resolved), K-chunk (fp32), 16-bit pieces (CONV_SPLIT)
    bool bm, lz;              // the build with the backward-statistics epilogue / that forms lazy sources (tilings, CONV_WRES)
    bool ok;                  // false: no kernel runs this description -- launch_conv() returns hipErrorInvalidValue
    bool lazy_ok;             // lazy sources (ConvSrc::la): a kernel that forms them on load exists for this layer once its id is chosen
                              // (mode 3: conv_thin16, the lazy row build, conv_bf16<SPL = 2> for 3x3 stride 1 / 2 and 1x1, conv_wres;
                              // independent of a.cfg); a launch with lazy sources that reaches any other kernel is not ok
    bool bm_ok;               // the chosen kernel has a build with the backward-statistics epilogue (ConvArgs::bm_y) for this window
    bool row_ok, b16;         // what the layer is eligible for whatever a.cfg says: the row family; the 16-bit tilings in this mode
    int stat_rows;            // statistics partial rows per image (a.stats): one per output row (row family) or per 4x8 patch
};
// conv_plan.hip.  conv_plan(): the operands, sizes, mode, id and epilogue of p.a and p.ks / p.stride are set; chooses the kernel
// and fills everything else.  What a source holds does not enter the choice; a caller that changes what does (a source's lazy
// coefficients, a.cfg, a.stats, the bm_* fields, the pixel mapping) plans again.  launch_conv(): that kernel.
void conv_plan(ConvPlan &p);
hipError_t launch_conv(const ConvPlan &p, hipStream_t st);
// What a kernel file says about its kernels (conv_plan() alone asks) and its launch (launch_conv() alone calls)
bool conv_small_ok(const ConvArgs &a, int ks, int stride);          // conv_small.hip: the row family
bool conv_small_lazy_ok(const ConvArgs &a, int ks, int stride);     // conv_small_kernel<2, 16, 2, LZ>: lazy source (ConvSrc::la)
bool conv_thin_ok(const ConvArgs &a, int ks, int stride);           // conv_thin.hip
bool conv_bf16_ok(const ConvArgs &a, int ks, int stride);           // conv_bf16.hip (modes 1..3)
bool conv_wres_ok(const ConvArgs &a, int ks, int stride);           // conv_wres.hip: mode 3, 3x3 stride 1, one 64-channel source
hipError_t launch_conv_fp32(const ConvPlan &p, hipStream_t st);     // CONV_FP32, CONV_FP32_WS
hipError_t launch_conv_bf16(const ConvPlan &p, hipStream_t st);
hipError_t launch_conv_wres(const ConvPlan &p, hipStream_t st);
hipError_t launch_conv_small(const ConvPlan &p, hipStream_t st);    // CONV_ROW, CONV_ROW_LAZY
hipError_t launch_conv_thin(const ConvPlan &p, hipStream_t st);
// max |x| of a dense fp32 tensor folded into *slot (bit pattern; the caller zeroes the slot): for tensors that enter the
// fp16-split mode from outside the plans' own producers (op-level entry points, stage-level forwards)
// (single_word: a weight slot -- one word; otherwise a tensor slot of AMAX_WORDS words)
hipError_t launch_absmax(const float *x, size_t n, unsigned *slot, hipStream_t st, bool single_word = false);
// the four parity classes of a thin stride-2 data gradient (dY 32 -> 16 or 64 -> 32 channels) in one pass (conv_thin.hip)
bool dgrad_s2_thin_ok(int prec, int ks, int stride, int dyC, int srcC, int CinTotal, int c_off, const unsigned *amax_dy,
                      const unsigned *amax_w, int H, int W);
hipError_t launch_dgrad_s2_thin(const float *dy, int B, int H, int W, int dyC, const float *w_master, int CinTotal, int c_off, float *out,
                                int accumulate, const unsigned *amax_dy, const unsigned *amax_w, hipStream_t st);

// Measurement aid (mc_profile_train): the last launch_conv / launch_wgrad on this host thread notes
// its kernel family (1 = fused conv incl. dgrad, 2 = wgrad) and algorithmic FLOPs here.
struct ProfLast { int kind; double flops, bytes; };   // bytes: algorithmic (inputs + outputs + weights, each once)
extern thread_local ProfLast prof_last;

}  // namespace mc
