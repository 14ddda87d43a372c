// What the weight-gradient kernels on 16-bit pieces share, device side: wgrad_bf16_kernel (wgrad_bf16.hip, two barriers per
// pixel group) and wgrad_pipe_kernel (wgrad_pipe.hip, its software-pipelined form for mode 3).  Both stage a group of 4x8-pixel
// patches of dY and the halo of X into the same channel-major LDS image and run the same MFMAs out of it; here are the image
// (WgLds, lds_skew, lane_chan), the in-row test of the staging loads (wg_in_row) and the tap construction of a halo row and the
// order of the partial products (wg_taps, WgProducts).  Everything here leaves the machine code of the kernels as it was.  The
// workgroup prologue, the staging plan, the loads of a patch, the lazy-source preparation and the store of the partials stay
// in each kernel: as functions of this header they compile differently (profiles/wgrad_tile_symbols.txt), the loads measurably
// slower.  No kernel is defined here.
#pragma once
#include "conv_mfma.h"
#include "train.h"

namespace mc {

__device__ __forceinline__ int lds_skew(int channel) { return ((channel >> 4) & 3) * 16; }
// Which channel of its wave's 32 a lane reads (MFMA row / column li <-> channel lane_chan(li), an involution).  The LDS
// serves a ds_read_b128 in the lane groups {0-3, 12-15, 20-27} and {4-11, 16-19, 28-31} (+32): with the identity mapping
// a group straddles two 16-channel blocks, whose rows lds_skew() shifts against each other by 16 bytes -- half the 16-byte
// windows of a group then collide (PMC, rounds 2 / 3: SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE = 0.67).  Swapping lanes
// 4-11 with 20-27 gives every group the 16 channels of ONE block: window = (7 or 15) * channel + const mod 16, a bijection.
__device__ __forceinline__ int lane_chan(int li) { return ((li & 15) >= 4 && (li & 15) < 12) ? (li ^ 16) : li; }

// The LDS image of one patch: X as [channel][halo row][pixel], dY as [channel][patch row][8 px], 16-bit elements.
template <int KS, int S>
struct WgLds {
    static_assert(S == 1 || (S == 2 && KS == 3), "stride 2: 3x3 only");
    static constexpr int PAD = KS / 2, T = KS * KS;
    // stride 1: halo tile 6 x 10 (3x3) or 4 x 8 (1x1).  stride 2: the 4 x 8 output patch reads input rows 2y-1 .. 2y+7 and
    // columns 2x-1 .. 2x+15; a staged row holds the ODD columns (2x-1+2j, j = 0..8, 16 slots) followed by the EVEN ones
    // (2x+2j, j = 0..7), so that the 8 pixels a tap column needs are again 8 consecutive slots: tap 0 = odd slots 0..7,
    // tap 1 = even slots 0..7, tap 2 = odd slots 1..8
    static constexpr int IH = S == 2 ? 9 : 3 + KS, IW = 7 + KS;
    static constexpr int XROW = S == 2 ? 48 : (KS == 3 ? 32 : 16);   // bytes per staged halo row
    // Bytes per channel row.  The staging writes of a wave go to 16 channel groups x 4 pixel pairs: with 16-byte aligned
    // rows the 4-channel stride is a multiple of 16 banks whatever the padding, i.e. 4 distinct banks for 16 lanes (a
    // 4-way conflict on every ds_write_b32; PMC: SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE = 0.75).  Every group of 16
    // channels is therefore skewed by another 16 bytes (lds_skew): the 16 channel groups land on 16 distinct multiples
    // of 4 banks and the pixel pairs fill the gaps -- conflict-free writes; the fragment reads (8 lanes = 8 consecutive
    // channels, same skew) keep their disjoint banks.  Rows grow by the largest skew (48 bytes).
    // (stride 2: 9 * 48 + 64 = 496 = 31 * 16 -- an odd number of 16-byte windows per channel keeps the fragment reads of 16
    //  consecutive channels on 16 distinct windows, as 15 does for stride 1)
    static constexpr int XCH = IH * XROW + (S == 2 ? 64 : 48);   // 240 (3x3) / 112 (1x1) / 496 (3x3 stride 2)
    static constexpr int DCH = 4 * 16 + 48;                     // bytes per dY channel: 112
};

// Does column xx lie in a row W pixels wide?  Selects between a pixel's buffer offset and BUF_OOB, which reads as zero.
// (one UNSIGNED compare per pixel: with `xx >= 0 && xx < W` hipcc branches on the shared half of the two conditions
//  and, since both arms load into the same registers, puts s_waitcnt vmcnt(0) between them -- a full memory latency
//  in front of the MFMAs of every group.  Dead items carry a column far outside either way.)
__device__ __forceinline__ bool wg_in_row(int xx, int W) { return (unsigned)xx < (unsigned)W; }

// The three tap columns of one staged halo row of one piece plane (KS == 1: b0 alone).  For tap column s the 8 pixels
// x+s..x+s+7 start at a 2-byte offset, which LDS cannot serve in one aligned read: a lane reads pixels 0..7 and builds the
// operands in registers -- s = 0 as read, s = 2 the same registers shifted by one dword (free), s = 1 four v_alignbit.
template <int KS, int S>
__device__ __forceinline__ void wg_taps(const unsigned char *row, u32x4 &b0, u32x4 &b1, u32x4 &b2) {
    const u32x4 lo = *reinterpret_cast<const u32x4 *>(row);
    b0 = lo;
    if (KS == 3) {
        // pixels 8, 9 of the row: a second 16-byte read (conflict-free, 4 LDS cycles) rather than a
        // ds_read_b32, whose 32-lane groups meet 4-way on channel rows that are multiples of 16 bytes
        // (the empty asm keeps the compiler from narrowing it back to the one dword that is used)
        u32x4 hi4 = *reinterpret_cast<const u32x4 *>(row + 16);
        asm volatile("" : "+v"(hi4));
        const unsigned hi = hi4[0];
        u32x4 sh;                        // slots 1..8 of the plane `lo` starts
        sh[0] = __builtin_amdgcn_alignbit(lo[1], lo[0], 16);
        sh[1] = __builtin_amdgcn_alignbit(lo[2], lo[1], 16);
        sh[2] = __builtin_amdgcn_alignbit(lo[3], lo[2], 16);
        sh[3] = __builtin_amdgcn_alignbit(hi, lo[3], 16);
        if (S == 2) {                    // odd columns: taps 0 and 2; even columns: tap 1
            b1 = *reinterpret_cast<const u32x4 *>(row + 32);
            b2 = sh;
        } else {
            b1 = sh;
            b2[0] = lo[1]; b2[1] = lo[2]; b2[2] = lo[3]; b2[3] = hi;
        }
    }
}

// The partial products (piece of dY, piece of X) every tap accumulates, smallest first.  SPL 1: the single (0, 0); SPL 2:
// (lo, hi), (hi, lo), (hi, hi); SPL 3: the six of weight >= 2^-16
template <int SPL>
struct WgProducts {
    static constexpr int NP = SPL == 1 ? 1 : (SPL == 2 ? 3 : 6);
    static constexpr int PA[6] = {SPL == 2 ? 1 : 0, SPL == 2 ? 0 : 2, SPL == 2 ? 0 : 1, 0, 1, 0};
    static constexpr int PX[6] = {SPL == 2 ? 0 : 2, SPL == 2 ? 1 : 0, SPL == 2 ? 0 : 1, 1, 0, 0};
};

}  // namespace mc
