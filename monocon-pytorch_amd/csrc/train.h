// Training-side launch argument blocks (targets, losses, BatchNorm train mode, backward, optimizer).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cstdlib>
#include <vector>

#include "conv_mfma.h"

namespace mc {

// ---- target generator (reference utils/target_generator.py:30-177)
struct TargetArgs {
    // labels, fp32 (B, max_objs, .) as collate_fn delivers them (dataset/monocon_dataset.py:160-171)
    const float *gt_bboxes, *gt_labels, *gt_bboxes_3d, *depths, *gt_kpts_2d, *gt_kpts_valid, *mask;
    int B, max_objs, num_kpt, num_classes, fh, fw;
    float h_ratio, w_ratio;
    // outputs (zero-filled by the caller before the launch)
    float *center_heatmap, *kpt_heatmap;                 // (B,3,fh,fw), (B,9,fh,fw)
    float *wh, *offset, *dim, *alpha_cls, *alpha_offset, *depth, *c2k, *kho;
    long long *indices, *indices_kpt;                    // (B,30), (B,270)
    uint8_t *mask_target;                                // (B,30)
    float *mask_c2k, *mask_kho;                          // (B,30,18)
};
hipError_t launch_make_targets(const TargetArgs &a, hipStream_t st);

// ---- losses
hipError_t launch_focal(const float *p, const float *t, size_t n, float *partial, float *loss_out, float *aux,
                        hipStream_t st);
hipError_t launch_focal_grad(const float *p, const float *t, size_t n, const float *aux, const float *gscale, int gidx,
                             float *dlogit, hipStream_t st, int wrt_pred = 0);
int focal_partial_floats();

struct GatherLossArgs {
    const float *pred[10];       // NCHW prediction maps (pred order)
    float *dpred[10];            // NCHW gradient wrt the raw 1x1 outputs (mode 1), zero-filled
    const long long *indices, *indices_kpt;
    const uint8_t *mask_target;
    const float *wh, *offset, *dim, *alpha_cls, *alpha_offset, *depth, *c2k, *kho, *mask_c2k, *mask_kho;
    int B, max_objs, HW;
    float *losses;               // [10] LOSS order
    float *aux;                  // [1] number of valid objects
    const float *gscale;         // [10] upstream gradient of each loss (mode 1)
    int wrt_pred;                // mode 1: 0 = gradient wrt the raw 1x1 outputs, 1 = wrt the prediction maps themselves
    double *partial;             // workspace of gathered_loss_ws_doubles() doubles (per-workgroup sums, then the totals)
    int nwg;                     // (set by the launcher)
};
size_t gathered_loss_ws_doubles();
hipError_t launch_gathered_losses(const GatherLossArgs &a, int mode, hipStream_t st);

// ---- batched weight packing / BatchNorm folding (pack_batch.hip)
struct PackJobDesc {
    const float *w;        // master weight, OIHW fp32
    float *dst32;          // fp32 panel or null
    void *dst16;           // bf16 piece planes or null
    int kind;              // 0: forward panel, 1: data-gradient panel
    int Cout, Cin, k;      // forward: shape of w.  data gradient: Cin = channels of the source (Cs)
    int CinTotal;          // forward: channels of the panel (virtual concat).  data gradient: Cin of the forward weight
    int CoutP;             // forward: padded columns.  data gradient: CoutPad (K of the data gradient)
    int n_off, c_off;      // forward: column / channel offset in the panel.  data gradient: c_off of the source
    int CsP, cls, nsplit;  // data gradient: padded source channels, parity class (-1: stride 1); pieces: 1 / 3 bf16, 2 fp16
    int block_begin, nblocks;
    unsigned *amax;        // nsplit == 2: slot holding max |w| of the master weight(s) behind the panel (conv_mfma.h)
};
// does a panel whose K dimension (forward: its channels, data gradient: CoutPad) is K get 16-bit piece planes in mode prec?
inline bool panel_has_pieces(int prec, int K) { return prec >= 1 && K % 8 == 0; }
// taps of a data-gradient panel: the whole flipped kernel (cls < 0) or the window of one output-parity class
inline int dgrad_taps(int k, int cls) { return cls < 0 ? k * k : (1 + (cls >> 1)) * (1 + (cls & 1)); }
// elements of a panel (one fp32 plane; a piece plane has as many 16-bit elements)
inline size_t fwd_panel_elems(int k, int CinPanel, int CoutP) { return (size_t)k * k * CinPanel * CoutP; }
inline size_t dgrad_panel_elems(int k, int cls, int CoutPad, int Cs) { return (size_t)dgrad_taps(k, cls) * CoutPad * conv_coutp(Cs); }
// forward panel: w (Cout, Cin, k, k) -> columns [n_off, n_off + Cout) of a panel of CinPanel channels x CoutP columns.
// dst16 is ignored where the panel has no piece planes; amax: the weight's max-|w| slot (mode 3)
inline PackJobDesc pack_job_fwd(const float *w, int Cout, int Cin, int k, float *dst32, void *dst16, int CinPanel, int CoutP,
                                int n_off, int prec, unsigned *amax) {
    PackJobDesc j{};
    j.w = w; j.dst32 = dst32; j.dst16 = panel_has_pieces(prec, CinPanel) ? dst16 : nullptr;
    j.kind = 0; j.Cout = Cout; j.Cin = Cin; j.k = k; j.CinTotal = CinPanel; j.CoutP = CoutP; j.n_off = n_off;
    j.cls = -1; j.nsplit = split_pieces(prec); j.amax = amax;
    return j;
}
// data-gradient panel of ONE source (channels [c_off, c_off + Cs) of the forward weight w (Cout, CinTotal, k, k)) and one
// class (-1: stride 1; 0..3: output-parity class of a stride-2 3x3 data gradient); dY has CoutPad >= Cout channels
inline PackJobDesc pack_job_dgrad(const float *w, int Cout, int CinTotal, int k, int c_off, int Cs, int CoutPad, int cls,
                                  float *dst32, void *dst16, int prec, unsigned *amax) {
    PackJobDesc j{};
    j.w = w; j.dst32 = dst32; j.dst16 = panel_has_pieces(prec, CoutPad) ? dst16 : nullptr;
    j.kind = 1; j.Cout = Cout; j.Cin = Cs; j.k = k; j.CinTotal = CinTotal; j.CoutP = CoutPad; j.c_off = c_off;
    j.CsP = conv_coutp(Cs); j.cls = cls; j.nsplit = split_pieces(prec); j.amax = amax;
    return j;
}
// The launch of one data-gradient panel: a stride-1 conv over dY (B, Hd, Wd, Cd channels, max-|dY| slot dy_amax) with the
// panel of job `p` in precision mode prec, into g, the NHWC gradient (Hs x Ws) of the panel's source -- dense for the
// stride-1 panel, every second pixel from (py, px) for a parity class; accumulate: on top of what g holds.  Fills d, window
// code included, and plans it (conv_plan); the shape id and epilogue extras stay the caller's, who plans again after setting them.
inline void dgrad_conv_args(ConvPlan &dp, const PackJobDesc &p, int prec, const float *dy, const unsigned *dy_amax, int B, int Hd,
                            int Wd, int Cd, float *g, int Hs, int Ws, bool accumulate) {
    const int ld = p.Cin, py = p.cls >> 1, px = p.cls & 1;
    dp = ConvPlan{};
    ConvArgs &d = dp.a;
    d.nsrc = 1; d.src[0].p = dy; d.src[0].C = Cd;
    d.B = B; d.Hin = Hd; d.Win = Wd; d.Hout = Hd; d.Wout = Wd;
    d.Cin = Cd; d.Cout = ld; d.CoutP = p.CsP; d.wpk = p.dst32;
    d.wpk16 = p.dst16; d.prec = p.dst16 ? prec : 0;
    d.amax_in[0] = dy_amax; d.amax_w = p.amax;
    d.out = g; d.out_ld = ld;
    if (p.cls >= 0) {
        d.out = g + ((size_t)py * Ws + px) * ld;
        d.o_px = 2 * ld; d.o_row = 2 * Ws * ld; d.o_img = Hs * Ws * ld;
    }
    if (accumulate) { d.res = d.out; d.res_ld = ld; d.r_px = d.o_px; d.r_row = d.o_row; d.r_img = d.o_img; }
    const int code = (1 + py) * 10 + (1 + px);      // window KH x KW as KH * 10 + KW; 1 x 1 is the plain 1x1 conv
    dp.ks = p.cls < 0 ? p.k : (code == 11 ? 1 : code);
    dp.stride = 1;
    conv_plan(dp);
}
struct PackBatch {
    std::vector<PackJobDesc> jobs;
    PackJobDesc *dev = nullptr;
    int total_blocks = 0;
    bool uploaded = false;
    void clear();
    void add(PackJobDesc j);
    // with_amax: first fold max |w| of every forward job into its slot (slots zeroed by the caller)
    hipError_t launch(hipStream_t st, bool with_amax = false);
    PackBatch() = default;
    PackBatch(const PackBatch &) = delete;
    PackBatch &operator=(const PackBatch &) = delete;
    ~PackBatch();
};
struct FoldJobDesc {
    const float *g, *b, *rm, *rv;
    float eps;
    int C;
    float *scale, *shift;
};
struct FoldBatch {
    std::vector<FoldJobDesc> jobs;
    FoldJobDesc *dev = nullptr;
    bool uploaded = false;
    int maxC = 0;
    void clear();
    void add(const FoldJobDesc &j);
    hipError_t launch(hipStream_t st);
    FoldBatch() = default;
    FoldBatch(const FoldBatch &) = delete;
    FoldBatch &operator=(const FoldBatch &) = delete;
    ~FoldBatch();
};

// ---- fused clip + AdamW (reference engine/monocon_engine.py:94-102)
// vmax: max_exp_avg_sq of an amsgrad class (null otherwise); cls: the tensor's hyper-parameter class (row of AdamTable);
// e: the tensor's weight average (mc_optim_bind_ema; null: it has none)
struct OptTensor { float *p, *g, *m, *v, *vmax; int cls; float *e; };
struct OptChunk { int tensor, begin, count; };
struct AdamHyper { float decay, beta1, one_minus_beta1, beta2, one_minus_beta2, sqrt_bc2, eps, step_size; };
constexpr int OPT_MAX_CLASSES = 16;     // == MC_OPT_MAX_CLASSES
// One row per distinct (lr, betas, eps, weight_decay, step, amsgrad, maximize), folded on the host in double; passed to the
// step kernel BY VALUE (kernel-argument segment): lr moves every step, and an argument has no buffer to race on.
struct AdamTable { AdamHyper hp[OPT_MAX_CLASSES]; unsigned amsgrad, maximize; /* bit c: class c */ };
// The non-finite guard's device-resident record of one step (== mc_guard_report).  The guarded final norm kernel writes it
// whole (skipped = !isfinite(norm), first_tensor -1, n_elements 0); the guarded AdamW kernels of a skipped step add what
// they find in the gradients: the smallest table index of a tensor with a NaN/inf element, and how many such elements.
struct GuardRecord { int skipped, first_tensor; unsigned long long n_elements; float norm; int pad_; };
// `guard` (null: off) on every launcher below selects the guarded instantiations: the same number of launches, the same
// bits while guard->skipped is clear; once it is set the AdamW pass only reads g and the stand-alone average does nothing.
hipError_t launch_clip_adamw(const OptTensor *tab, const OptChunk *chunks, int nchunks, float *partial, float *normcoef,
                             float max_norm, const AdamHyper &hp, hipStream_t st, float ema_w = 0.f, GuardRecord *guard = nullptr);
// the pieces of the general path: global p-norm (p = 1, 2, +inf or any finite p > 0) + clip coefficient into
// normcoef[0..1]; the per-class step; the in-place gradient scale of a stand-alone clip_grad_norm_
hipError_t launch_grad_norm(const OptTensor *tab, const OptChunk *chunks, int nchunks, float *partial, float *normcoef,
                            float max_norm, double norm_type, hipStream_t st, GuardRecord *guard = nullptr);
hipError_t launch_adamw_classes(const OptTensor *tab, const OptChunk *chunks, int nchunks, const float *normcoef,
                                const AdamTable &tb, hipStream_t st, float ema_w = 0.f, GuardRecord *guard = nullptr);
// LAMB (mc_clip_lamb_step_classes): one row per class, folded on the host in double and passed by value like AdamTable.
// Unlike AdamHyper nothing is pre-multiplied into p: u = (m / bc1) / (sqrt(v) / sqrt_bc2 + eps) + wd * p, p -= lr * r * u.
struct LambHyper { float beta1, one_minus_beta1, beta2, one_minus_beta2, sqrt_bc2, eps, bc1, wd, lr; };
struct LambTable { LambHyper hp[OPT_MAX_CLASSES]; unsigned maximize, adapt; /* bit c: class c */ float trust_clip; /* 0: no cap */ };
// device workspace of the LAMB step: (sum p^2, sum u^2) per chunk of the table, the ratio per tensor, and the index of every
// tensor's first chunk in the chunk list ([ntensors + 1])
struct LambWorkspace { float *chunk_sums, *ratio; int *first_chunk; };
// the three passes behind launch_grad_norm: moments + per-chunk norms, per-tensor ratio, apply (+ the average when ema_w > 0)
hipError_t launch_lamb_classes(const OptTensor *tab, const OptChunk *chunks, int nchunks, int ntensors, const float *normcoef,
                               const LambTable &tb, const LambWorkspace &ws, hipStream_t st, float ema_w = 0.f,
                               GuardRecord *guard = nullptr);
// stand-alone weight average e = ema_one(e, src, w) over a table whose .p is e and whose .g is src (mc_ema_bind)
hipError_t launch_ema(const OptTensor *tab, const OptChunk *chunks, int nchunks, float w, hipStream_t st,
                      const GuardRecord *guard = nullptr);
// gradient accumulation over a table whose .p is the accumulator and whose .g is the gradient (mc_accum_bind); mode is
// MC_ACCUM_BEGIN (acc = g), MC_ACCUM_ADD (acc += g) or MC_ACCUM_FINISH (g = (acc + g) * scale): one launch
hipError_t launch_grad_accum(const OptTensor *tab, const OptChunk *chunks, int nchunks, int mode, float scale, hipStream_t st);
hipError_t launch_grad_scale(const OptTensor *tab, const OptChunk *chunks, int nchunks, const float *normcoef, hipStream_t st);
int opt_partial_floats();

// ---- train-mode element-wise / reduction kernels (kernels_train.hip)
int chan_reduce_blocks(int B, int rows_per_img);
hipError_t launch_chan_reduce(const float *y, const float *dz, const float *z, const float *shift, int B, int rows_per_img,
                              int C, int mode, int relu, float *partial, int Cstride, hipStream_t st, const float *fa = nullptr,
                              const float *fb = nullptr);
hipError_t launch_bn_finalize(const float *partial, int nb, int Cstride, double n, int C, const float *shift,
                              const float *gamma, const float *beta, float eps, float momentum, float *rm, float *rv,
                              long long *nbt, float *a, float *b, float *mean, float *rstd, hipStream_t st,
                              double *fold = nullptr, const unsigned *ymax = nullptr, unsigned *zmax = nullptr, int zrelu = 1);
// (ymax / zmax: a lazy activation's bound of max |z| from max |y| -- see bn_finalize_kernel)
size_t partial_fold_doubles(int nb, int C);   // scratch for `fold` (0: the partial list is short, no pre-pass)
hipError_t launch_affine_act(const float *y, const float *a, const float *b, const float *res, int B, size_t rows_per_img,
                             int C, int per_sample, int relu, float *z, hipStream_t st, unsigned *amax = nullptr,
                             const float *res_a = nullptr, const float *res_b = nullptr, int res_relu = 0,    // lazy residual
                             unsigned *zbits = nullptr);      // also the ReLU mask bit-packed, [row][C / 32] words (ConvArgs::bm_zbits)
hipError_t launch_bn_bwd_finalize(const float *partial, int nb, int Cstride, double n, int C, const float *gamma,
                                  const float *mean, const float *rstd, float *dgamma, float *dbeta, float *coef,
                                  hipStream_t st, double *fold = nullptr);
hipError_t launch_affine_bwd(const float *dz, const float *z, const float *y, const float *coef, int B, size_t rows_per_img,
                             int C, int per_sample, int relu, float *dy, float *gres, int gres_mode, hipStream_t st,
                             const float *fa = nullptr, const float *fb = nullptr, float *csum = nullptr, float *csum_out = nullptr,
                             unsigned *amax = nullptr);   // amax: max |z| / max |dy| folded into the slot (see ConvArgs::amax_in)
// csum: scratch of affine_bwd_blocks(B, rows, C) * C * 2 floats -> csum_out[C] = column sums of dy (the conv bias gradient)
int affine_bwd_blocks(int B, size_t rows_per_img, int C);
size_t colsum_partial_floats(size_t rows, int ld);
hipError_t launch_colsum(const float *x, size_t rows, int C, int ld, float *partial, float *out, hipStream_t st);
hipError_t launch_colsum_final(const float *partial, int nb, int C, float *out, hipStream_t st);   // partial [nb][C][2] -> out[C]
hipError_t launch_maxpool2_bwd(const float *x, const float *dout, int B, int H, int W, int C, float *dx, int accumulate,
                               hipStream_t st, const float *la = nullptr, const float *lb = nullptr,    // la / lb: lazy x (ConvSrc::la)
                               float *stats_partial = nullptr);   // [maxpool2_bwd_blocks()][C][2]: also mask + BatchNorm-backward partials
int maxpool2_bwd_blocks(int B, int H, int W, int C);
size_t deconv4_bwd_w_partial_floats(int B, int H, int C);
hipError_t launch_deconv4_bwd_w(const float *in, const float *dout, int B, int H, int W, int C, float *partial, float *dw,
                                hipStream_t st, const float *la, const float *lb,    // la / lb: lazy in (or null)
                                const float *wpk, float *din,   // the same pass also writes din, the gradient wrt the input
                                float *stats = nullptr);   // [B * H][C][2] (lazy `in` only): din masked by its ReLU + its BatchNorm-backward partials

// ---- head / stem train kernels (kernels_head_train.hip)
// nz (both variants; may be null): [B][ceil(HW / 64)] words, bit h set when any row of head h is != 0.f in that aligned
// 64-pixel tile of `out` -- the map launch_head_bwd / launch_head_dx skip all-zero tiles by
hipError_t launch_dpred_pack(const float *const dpred[10], int ld, int B, int HW, float *out, hipStream_t st,
                             unsigned *nz = nullptr);
// the same pack with a caller's gradients wrt the prediction maps added in (grad[k] NCHW like pred[k], nullptr: none): row r
// of map k gets dpred + (d map / d raw output, from pred[k]) * grad, in the same single pass
hipError_t launch_dpred_pack_user(const float *const dpred[10], const float *const pred[10], const float *const grad[10], int ld,
                                  int B, int HW, float *out, hipStream_t st, unsigned *nz = nullptr);
struct AttnTrainArgs {
    const float *stats;            // [B][chunks][stat_ld][2] partial (sum, sumsq) of (x - running_mean)
    int chunks, stat_ld, B, HW;
    double *stats64;               // [B][stat_ld][2] scratch: the partials of every image summed in fp64 (fixed order)
    float *rm[9], *rv[9];          // AttnBN running statistics (updated in place, momentum 0.03)
    long long *nbt[9];
    const float *att_w[9], *att_g[9], *att_b[9];
    float *att_rm[9], *att_rv[9];  // attention BN(10) running statistics (momentum 0.1)
    long long *att_nbt[9];
    const float *weight_[9], *bias_[9];
    // saved for backward
    float *sv_inst;                // [B][576][3]  s, instance mean, instance (unbiased) variance
    float *mu_r;                   // [576][2]     batch mean, rstd
    float *bn10;                   // [9][10][2]   attention batch mean, rstd
    float *that, *yatt;            // [B][9][10]   normalised attention logits, hard-sigmoid outputs
    float *gamma_p;                // [B][576]     per-sample gamma'
    float *scale, *shift;          // [B][576]     folded per-sample affine
};
struct AttnGradPtrs { float *d_weight_[9], *d_bias_[9], *d_att_w[9], *d_att_g[9], *d_att_b[9]; };
hipError_t launch_attn_train_fwd(const AttnTrainArgs &a, hipStream_t st);
hipError_t launch_attn_train_bwd(const AttnTrainArgs &a, const float *partial, int rb_per_img, const AttnGradPtrs &gp,
                                 float *coef, hipStream_t st);
hipError_t launch_head_bwd(const float *draw, int ld, const float *z, const float *x, const float *w1, int B, int HW,
                           int blocks, float *d, float *dw_partial, float *red_partial, hipStream_t st,
                           const float *scale = nullptr, const float *shift = nullptr, const unsigned *nz = nullptr);
hipError_t launch_head_dx(const float *draw, int ld, const float *x, const float *w1, const float *coef, int B, int HW, int blocks,
                          float *dx, float *csum, float *csum_out, unsigned *amax, hipStream_t st, const float *scale,
                          const float *shift, const unsigned *nz = nullptr);
hipError_t launch_splitk_reduce(const float *partial, int ksplit, int T, int Cout, int Cin, float *dw, hipStream_t st);
int stem_wgrad_blocks(int B, int H, int W);
// img_amax / dy_amax (mode 3): max-|x| slots of the image and of dY -> the fp16-pipe kernel (stem_f16.hip)
// (fused form, mode 3 only: y / coef / y_amax non-null -- see launch_stem_wgrad_f16)
hipError_t launch_stem_wgrad(const float *img, const float *dy, int B, int H, int W, float *partial, float *dw,
                             hipStream_t st, const unsigned *img_amax = nullptr, const unsigned *dy_amax = nullptr,
                             const float *y = nullptr, const float *coef = nullptr, const unsigned *y_amax = nullptr);
// the stem's data gradient: dY NHWC (B,H,W,16) x the OIHW master weight (16,3,7,7) -> dX NCHW (B,3,H,W), fp32 operands and
// accumulation in every precision mode, any H, W >= 1.  Stored form: `dy` is the gradient wrt the raw conv output.  Fused form
// (y and coef non-null, the convention of launch_stem_wgrad_f16): `dy` is the masked gradient d of the stem's activation and
// dY = P d + Q y + R is formed while the tile is staged, coef[16][4] = (P, Q, R, -) per channel.
hipError_t launch_stem_dgrad(const float *dy, const float *w_oihw, int B, int H, int W, float *dx, hipStream_t st,
                             const float *y = nullptr, const float *coef = nullptr);

// ---- conv weight gradient: wgrad_plan.hip chooses and launches; kernels in wgrad_mfma.hip (WG_FP32, WG_SMALL), wgrad_bf16.hip
//      (WG_SPLIT: modes 1..3), wgrad_pipe.hip (WG_PIPE), conv_thin.hip (WG_THIN16).  WgradArgs is the kernels' parameter block:
//      the hidden arguments (gridDim) lie behind it, so its layout is part of their machine code.  wgrad_plan() alone writes ksplit .. pipe.
enum WgKernel { WG_FP32, WG_SPLIT, WG_PIPE, WG_SMALL, WG_THIN16 };
struct WgradArgs {
    ConvSrc src[4];
    int nsrc;
    int B, Hin, Win, Hout, Wout, Cin, Cout;
    const float *dy;          // NHWC (B,Hout,Wout,dy_ld); channels >= Cout must be zero / are ignored
    int dy_ld;
    float *partial;           // [ksplit][k*k][Cout][Cin]
    int ksplit, n_tiles, c_tiles, ppr, ppi, groups_per_img;
    int kernel;               // WgKernel (no kernel reads it).  WG_SMALL / WG_THIN16: ksplit = workgroups
    int prec;                 // 1: bf16 MFMA operands, 2: 3-way bf16 split, 3: 2-way fp16 split -- where a kernel for the mode exists
    int pb;                   // 32-pixel patches per staged group (2, or 1 for the split kernels)
    int pipe;                 // WG_PIPE: the tile (wgrad_pipe_tile()); ksplit = slices
    const unsigned *amax_x[4], *amax_dy;   // prec 3: max |x| (bit patterns) of every source and of dY (see ConvArgs::amax_in)
};
static_assert(sizeof(WgradArgs) == 264, "WgradArgs is the kernels' parameter block: keep its layout");
// One weight-gradient launch: the block and, host side, what wgrad_plan() decided.  wgrad_args() (mc_internal.h) fills one.
struct WgradPlan {
    WgradArgs a;
    int ks, stride;
    int WN, WC;               // wave grid of the workgroup, 32 channels of dY x 32 of X per wave (WG_FP32, WG_SPLIT, WG_PIPE)
    bool lazy_ok;             // the chosen kernel forms lazy sources (ConvSrc::la) on load
    bool ok;                  // false: no kernel runs these arguments -- launch_wgrad() returns hipErrorInvalidValue
    size_t partial_floats;    // size of a.partial
};
// the patch grid of dY (WgradArgs::ppr / ppi) and the staged pixel groups per image of a kernel that stages pb patches
inline void wgrad_set_patches(WgradArgs &a, int pb) {
    a.ppr = (a.Wout + 7) / 8;
    a.ppi = a.ppr * ((a.Hout + 3) / 4);
    a.groups_per_img = (a.ppi + pb - 1) / pb;
}
inline bool wgrad_any_lazy(const WgradArgs &a) { return any_lazy_src(a.src, a.nsrc); }
// The (WN, WC) wave grid wgrad_shape() planned, as a type: f(WgTile<WN, WC>{}) -- 64n x 64c, 128n x 32c, 64n x 32c, 32n x 32c.
template <int WN_, int WC_>
struct WgTile { static constexpr int WN = WN_, WC = WC_; };
template <typename F>
inline hipError_t with_wgrad_tile(int WN, int WC, F &&f) {
    if (WN == 2 && WC == 2) return f(WgTile<2, 2>{});
    if (WN == 4) return f(WgTile<4, 1>{});
    if (WN == 2) return f(WgTile<2, 1>{});
    return f(WgTile<1, 1>{});
}
// the dynamic LDS request of a weight-gradient kernel that needs `need` bytes.  Experiment knob (only with -DMC_DEBUG_HOOKS):
// MONOCON_HIP_WGRAD_LDS_KB pads the request, i.e. caps the workgroups per CU
inline size_t wgrad_lds_request(size_t need) {
#ifdef MC_DEBUG_HOOKS
    static const size_t pad = [] { const char *e = std::getenv("MONOCON_HIP_WGRAD_LDS_KB"); return e ? (size_t)std::atoi(e) * 1024 : (size_t)0; }();
    return pad > need ? pad : need;
#else
    return need;
#endif
}
// wgrad_plan.hip.  wgrad_plan(): the operands, sizes and mode of p.a and p.ks / p.stride are set; chooses the kernel and fills
// everything else (what a source holds does not enter the choice).  launch_wgrad(): that kernel + the split-K reduce.
void wgrad_plan(WgradPlan &p);
hipError_t launch_wgrad(const WgradPlan &p, float *dw_oihw, hipStream_t st);
inline size_t wgrad_partial_floats(const WgradPlan &p) { return p.partial_floats; }
// lazy X sources (ConvSrc::la in conv_mfma.h): does the chosen kernel form them on load?  (mode 3: wgrad_pipe_kernel's default
// tile, wgrad_bf16_kernel<SPL = 2>, wgrad_thin16_kernel, wgrad_small_kernel<2, 2>; anything else fails such a launch)
inline bool wgrad_lazy_capable(const WgradPlan &p) { return p.lazy_ok; }
// What a kernel file says about its kernels (wgrad_plan() alone asks, in this order) and its launch (launch_wgrad() alone calls)
bool wgrad_is_small(const WgradArgs &a, int ks, int stride);      // wgrad_mfma.hip: a 16-input-channel 3x3 layer
bool wgrad_thin_ok(const WgradArgs &a, int ks, int stride);       // conv_thin.hip: the small 16 -> 16 layer on the fp16 pipe (mode 3)
int wgrad_pipe_tile(const WgradArgs &a, int ks, int stride);      // wgrad_pipe.hip: 0 = not eligible
void wgrad_shape(const WgradArgs &a, int *WN, int *WC);           // wgrad_mfma.hip: the wave grid of WG_FP32 and WG_SPLIT
bool wgrad_sources_ok(const WgradArgs &a);                        // ... and what both ask of the sources
bool wgrad_bf16_ok(const WgradArgs &a, int ks, int stride);       // wgrad_bf16.hip (modes 1..3)
hipError_t launch_wgrad_fp32(const WgradPlan &p, hipStream_t st);
hipError_t launch_wgrad_small(const WgradPlan &p, hipStream_t st);
hipError_t launch_wgrad_bf16(const WgradPlan &p, hipStream_t st);
hipError_t launch_wgrad_pipe(const WgradPlan &p, hipStream_t st);
hipError_t launch_wgrad_thin(const WgradPlan &p, hipStream_t st);

}  // namespace mc
