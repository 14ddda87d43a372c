// Training-side C-ABI: target generation, losses (+ gradients wrt the prediction maps).
#include "mc_internal.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

static int check_targets(mc_handle *h, const mc_targets *t, const char *who) {
    if (!t) return fail(h, "%s: targets is NULL", who);
    const void *p[] = {t->center_heatmap_target, t->wh_target, t->offset_target, t->dim_target, t->alpha_cls_target,
                       t->alpha_offset_target, t->depth_target, t->center2kpt_offset_target, t->kpt_heatmap_target,
                       t->kpt_heatmap_offset_target, t->indices, t->indices_kpt, t->mask_target,
                       t->mask_center2kpt_offset, t->mask_kpt_heatmap_offset};
    for (size_t i = 0; i < sizeof(p) / sizeof(p[0]); ++i)
        if (!p[i]) return fail(h, "%s: targets field %d is NULL", who, (int)i);
    return 0;
}

extern "C" {

int mc_make_targets(mc_handle *h, const mc_labels *lab, int B, int max_objs, int pad_h, int pad_w, int fh, int fw,
                    const mc_targets *t, void *stream) {
    if (!h) return -1;
    if (!lab || !lab->gt_bboxes || !lab->gt_labels || !lab->gt_bboxes_3d || !lab->depths || !lab->gt_kpts_2d ||
        !lab->gt_kpts_valid_mask || !lab->mask)
        return fail(h, "mc_make_targets: a label pointer is NULL");
    if (check_targets(h, t, "mc_make_targets")) return -1;
    if (B < 1 || max_objs < 1 || fh < 1 || fw < 1 || pad_h < 1 || pad_w < 1)
        return fail(h, "mc_make_targets: bad shape");
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t HW = (size_t)fh * fw, R = (size_t)B * max_objs;
    if (h->tgt_arena && t->center_heatmap_target == h->tgt_arena) {
        HIPCHK(h, hipMemsetAsync(h->tgt_arena, 0, h->tgt_arena_bytes, st));
    } else {
        HIPCHK(h, hipMemsetAsync(t->center_heatmap_target, 0, B * 3 * HW * 4, st));
        HIPCHK(h, hipMemsetAsync(t->kpt_heatmap_target, 0, B * 9 * HW * 4, st));
        HIPCHK(h, hipMemsetAsync(t->wh_target, 0, R * 2 * 4, st));
        HIPCHK(h, hipMemsetAsync(t->offset_target, 0, R * 2 * 4, st));
        HIPCHK(h, hipMemsetAsync(t->dim_target, 0, R * 3 * 4, st));
        HIPCHK(h, hipMemsetAsync(t->alpha_cls_target, 0, R * 4, st));
        HIPCHK(h, hipMemsetAsync(t->alpha_offset_target, 0, R * 4, st));
        HIPCHK(h, hipMemsetAsync(t->depth_target, 0, R * 4, st));
        HIPCHK(h, hipMemsetAsync(t->center2kpt_offset_target, 0, R * 18 * 4, st));
        HIPCHK(h, hipMemsetAsync(t->kpt_heatmap_offset_target, 0, R * 18 * 4, st));
        HIPCHK(h, hipMemsetAsync(t->indices, 0, R * 8, st));
        HIPCHK(h, hipMemsetAsync(t->indices_kpt, 0, R * 9 * 8, st));
        HIPCHK(h, hipMemsetAsync(t->mask_target, 0, R, st));
        HIPCHK(h, hipMemsetAsync(t->mask_center2kpt_offset, 0, R * 18 * 4, st));
        HIPCHK(h, hipMemsetAsync(t->mask_kpt_heatmap_offset, 0, R * 18 * 4, st));
    }
    mc::TargetArgs a{};
    a.gt_bboxes = lab->gt_bboxes; a.gt_labels = lab->gt_labels; a.gt_bboxes_3d = lab->gt_bboxes_3d;
    a.depths = lab->depths; a.gt_kpts_2d = lab->gt_kpts_2d; a.gt_kpts_valid = lab->gt_kpts_valid_mask; a.mask = lab->mask;
    a.B = B; a.max_objs = max_objs; a.num_kpt = 9; a.num_classes = 3; a.fh = fh; a.fw = fw;
    a.h_ratio = (float)((double)fh / (double)pad_h);
    a.w_ratio = (float)((double)fw / (double)pad_w);
    a.center_heatmap = t->center_heatmap_target; a.kpt_heatmap = t->kpt_heatmap_target;
    a.wh = t->wh_target; a.offset = t->offset_target; a.dim = t->dim_target; a.alpha_cls = t->alpha_cls_target;
    a.alpha_offset = t->alpha_offset_target; a.depth = t->depth_target; a.c2k = t->center2kpt_offset_target;
    a.kho = t->kpt_heatmap_offset_target;
    a.indices = reinterpret_cast<long long *>(t->indices);
    a.indices_kpt = reinterpret_cast<long long *>(t->indices_kpt);
    a.mask_target = t->mask_target; a.mask_c2k = t->mask_center2kpt_offset; a.mask_kho = t->mask_kpt_heatmap_offset;
    HIPCHK(h, mc::launch_make_targets(a, st));
    return 0;
}

static int ensure_loss_ws(mc_handle *h) {
    if (h->loss_ws) return 0;
    void *q = nullptr;
    // focal partials (2 x npf), 64 floats of small results (aux, scratch losses), then the gathered losses' fp64 workspace
    const size_t n = (size_t)2 * mc::focal_partial_floats() + 64 + 2 * mc::gathered_loss_ws_doubles() + 2;
    HIPCHK(h, hipMalloc(&q, n * sizeof(float)));
    h->loss_ws = static_cast<float *>(q);
    return 0;
}

static void fill_gather_args(mc::GatherLossArgs &g, const float *const preds[10], float *const dpreds[10],
                             const mc_targets *t, int B, int max_objs, int HW, float *losses, float *aux,
                             const float *gscale) {
    for (int i = 0; i < 10; ++i) { g.pred[i] = preds[i]; g.dpred[i] = dpreds ? dpreds[i] : nullptr; }
    g.indices = reinterpret_cast<const long long *>(t->indices);
    g.indices_kpt = reinterpret_cast<const long long *>(t->indices_kpt);
    g.mask_target = t->mask_target;
    g.wh = t->wh_target; g.offset = t->offset_target; g.dim = t->dim_target; g.alpha_cls = t->alpha_cls_target;
    g.alpha_offset = t->alpha_offset_target; g.depth = t->depth_target; g.c2k = t->center2kpt_offset_target;
    g.kho = t->kpt_heatmap_offset_target; g.mask_c2k = t->mask_center2kpt_offset; g.mask_kho = t->mask_kpt_heatmap_offset;
    g.B = B; g.max_objs = max_objs; g.HW = HW; g.losses = losses; g.aux = aux; g.gscale = gscale;
}
static double *gather_ws(mc_handle *h) {       // 8-byte aligned, behind the float part of the loss workspace
    uintptr_t p = reinterpret_cast<uintptr_t>(h->loss_ws + 2 * mc::focal_partial_floats() + 64);
    return reinterpret_cast<double *>((p + 7) & ~(uintptr_t)7);
}

int mc_losses(mc_handle *h, const float *const preds[MC_NUM_PREDS], const mc_targets *t, int B, int max_objs, int fh,
              int fw, float *losses, void *stream) {
    if (!h) return -1;
    if (!preds || !losses) return fail(h, "mc_losses: null argument");
    for (int i = 0; i < MC_NUM_PREDS; ++i)
        if (!preds[i]) return fail(h, "mc_losses: preds[%d] is NULL", i);
    if (check_targets(h, t, "mc_losses")) return -1;
    HIPCHK(h, hipSetDevice(h->device));
    if (ensure_loss_ws(h)) return -1;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t HW = (size_t)fh * fw;
    const int npf = mc::focal_partial_floats();
    float *aux = h->loss_ws + 2 * npf;   // [0] npos center, [1] npos kpt, [2] n objects
    HIPCHK(h, mc::launch_focal(preds[0], t->center_heatmap_target, (size_t)B * 3 * HW, h->loss_ws, losses + 0, aux + 0, st));
    HIPCHK(h, mc::launch_focal(preds[1], t->kpt_heatmap_target, (size_t)B * 9 * HW, h->loss_ws + npf, losses + 5, aux + 1, st));
    mc::GatherLossArgs g{};
    fill_gather_args(g, preds, nullptr, t, B, max_objs, (int)HW, losses, aux + 2, nullptr);
    g.partial = gather_ws(h);
    HIPCHK(h, mc::launch_gathered_losses(g, 0, st));
    return 0;
}

static int losses_backward_impl(mc_handle *h, const float *const preds[MC_NUM_PREDS], const mc_targets *t, int B, int max_objs,
                                int fh, int fw, const float *grad_losses, float *const dpreds[MC_NUM_PREDS], void *stream,
                                int wrt_pred) {
    if (!h) return -1;
    if (!preds || !dpreds || !grad_losses) return fail(h, "mc_losses_backward: null argument");
    for (int i = 0; i < MC_NUM_PREDS; ++i)
        if (!preds[i] || !dpreds[i]) return fail(h, "mc_losses_backward: preds/dpreds[%d] is NULL", i);
    if (check_targets(h, t, "mc_losses_backward")) return -1;
    HIPCHK(h, hipSetDevice(h->device));
    if (ensure_loss_ws(h)) return -1;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t HW = (size_t)fh * fw;
    const int npf = mc::focal_partial_floats();
    float *aux = h->loss_ws + 2 * npf;
    float *scratch_losses = aux + 8;
    // recompute the reductions the gradients need (npos, object count, dim compensation weight)
    HIPCHK(h, mc::launch_focal(preds[0], t->center_heatmap_target, (size_t)B * 3 * HW, h->loss_ws, scratch_losses + 0, aux + 0, st));
    HIPCHK(h, mc::launch_focal(preds[1], t->kpt_heatmap_target, (size_t)B * 9 * HW, h->loss_ws + npf, scratch_losses + 5, aux + 1, st));
    if (h->dp_arena && dpreds[2] == h->dp_arena) {
        HIPCHK(h, hipMemsetAsync(h->dp_arena, 0, h->dp_arena_bytes, st));
    } else {
        for (int i = 2; i < 10; ++i) HIPCHK(h, hipMemsetAsync(dpreds[i], 0, (size_t)B * mc::PRED_CH[i] * HW * 4, st));
    }
    HIPCHK(h, mc::launch_focal_grad(preds[0], t->center_heatmap_target, (size_t)B * 3 * HW, aux + 0, grad_losses, 0, dpreds[0], st, wrt_pred));
    HIPCHK(h, mc::launch_focal_grad(preds[1], t->kpt_heatmap_target, (size_t)B * 9 * HW, aux + 1, grad_losses, 5, dpreds[1], st, wrt_pred));
    mc::GatherLossArgs g{};
    fill_gather_args(g, preds, dpreds, t, B, max_objs, (int)HW, scratch_losses, aux + 2, grad_losses);
    g.wrt_pred = wrt_pred;
    g.partial = gather_ws(h);
    HIPCHK(h, mc::launch_gathered_losses(g, 1, st));
    return 0;
}

int mc_losses_backward(mc_handle *h, const float *const preds[MC_NUM_PREDS], const mc_targets *t, int B, int max_objs,
                       int fh, int fw, const float *grad_losses, float *const dpreds[MC_NUM_PREDS], void *stream) {
    return losses_backward_impl(h, preds, t, B, max_objs, fh, fw, grad_losses, dpreds, stream, 0);
}

int mc_losses_backward_pred(mc_handle *h, const float *const preds[MC_NUM_PREDS], const mc_targets *t, int B, int max_objs,
                            int fh, int fw, const float *grad_losses, float *const dpreds[MC_NUM_PREDS], void *stream) {
    return losses_backward_impl(h, preds, t, B, max_objs, fh, fw, grad_losses, dpreds, stream, 1);
}

int mc_op_conv_wgrad(mc_handle *h, const float *const src[], const int src_channels[], int nsrc, int B, int Hin, int Win,
                     const float *dy, int Cout, int ksize, int stride, float *dw_oihw, void *stream) {
    if (!h) return -1;
    if (!src || !src_channels || !dy || !dw_oihw || nsrc < 1 || nsrc > 4) return fail(h, "mc_op_conv_wgrad: bad argument");
    if (!((ksize == 3 && (stride == 1 || stride == 2)) || (ksize == 1 && stride == 1)))
        return fail(h, "mc_op_conv_wgrad: unsupported k=%d stride=%d", ksize, stride);
    if (Cout % 4) return fail(h, "mc_op_conv_wgrad: Cout must be a multiple of 4");
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    Tensor x[4];
    std::vector<const Tensor *> xs;
    for (int i = 0; i < nsrc; ++i) {
        if (!src[i] || src_channels[i] % 16) return fail(h, "mc_op_conv_wgrad: source %d needs C %% 16 == 0", i);
        x[i] = operand_tensor(src[i], B, Hin, Win, src_channels[i]);
        xs.push_back(&x[i]);
    }
    Tensor dyt = operand_tensor(dy, B, mc::conv_out_dim(Hin, ksize, stride), mc::conv_out_dim(Win, ksize, stride), Cout);
    ScratchBuf slots;       // mode 3: max |x| of every source and of dY
    if (h->prec == 3) {
        size_t n[4];
        for (int i = 0; i < nsrc; ++i) n[i] = x[i].numel();
        HIPCHK(h, op_amax_slots(slots, src, n, nsrc, dy, dyt.numel(), false, st));
        for (int i = 0; i < nsrc; ++i) x[i].amax = slots.as<unsigned>() + i * mc::AMAX_WORDS;
        dyt.amax = slots.as<unsigned>() + 4 * mc::AMAX_WORDS;
    }
    mc::WgradPlan p{};
    wgrad_args(p, xs, dyt, Cout, Cout, ksize, stride, h->prec);
    void *part = nullptr;
    HIPCHK(h, hipMalloc(&part, mc::wgrad_partial_floats(p) * sizeof(float)));
    p.a.partial = static_cast<float *>(part);
    hipError_t e = mc::launch_wgrad(p, dw_oihw, st);
    hipError_t e2 = hipStreamSynchronize(st);
    (void)hipFree(part);
    HIPCHK(h, e);
    HIPCHK(h, e2);
    return 0;
}

int mc_op_conv_dgrad(mc_handle *h, const float *dy, const float *weight_oihw, int B, int Hin, int Win, int CinTotal,
                     int c_off, int Cs, int Cout, int ksize, int stride, int accumulate, float *dx, void *stream) {
    if (!h) return -1;
    if (!dy || !weight_oihw || !dx) return fail(h, "mc_op_conv_dgrad: null argument");
    if (!((ksize == 3 && (stride == 1 || stride == 2)) || (ksize == 1 && stride == 1)))
        return fail(h, "mc_op_conv_dgrad: unsupported k=%d stride=%d", ksize, stride);
    if (Cout % 16 || Cs % 4 || c_off < 0 || c_off + Cs > CinTotal) return fail(h, "mc_op_conv_dgrad: bad channel arguments");
    if (stride == 2 && ((Hin | Win) & 1)) return fail(h, "mc_op_conv_dgrad: stride 2 needs even Hin, Win");
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int Ho = mc::conv_out_dim(Hin, ksize, stride), Wo = mc::conv_out_dim(Win, ksize, stride);
    const int nclass = stride == 2 ? 4 : 1;
    ScratchBuf slots;       // mode 3: max |dy| and max |w| (a data-gradient job takes its scale from an existing slot)
    unsigned *dy_amax = nullptr, *w_amax = nullptr;
    if (h->prec == 3) {
        const size_t ndy = (size_t)B * Ho * Wo * Cout;
        HIPCHK(h, op_amax_slots(slots, &dy, &ndy, 1, weight_oihw, (size_t)Cout * CinTotal * ksize * ksize, true, st));
        dy_amax = slots.as<unsigned>();
        w_amax = dy_amax + 4 * mc::AMAX_WORDS;
    }
    // one panel per class (stride 2: the four output-parity classes), packed by the plans' packer in one grid
    ScratchBuf panel[4], panel16[4];
    mc::PackBatch pack;
    for (int c = 0; c < nclass; ++c) {
        const int cls = stride == 2 ? c : -1;
        const size_t pn = mc::dgrad_panel_elems(ksize, cls, Cout, Cs);
        HIPCHK(h, panel[c].alloc(pn * 4));
        HIPCHK(h, hipMemsetAsync(panel[c].p, 0, pn * 4, st));
        if (mc::panel_has_pieces(h->prec, Cout)) {
            const size_t bytes16 = pn * 2 * mc::split_pieces(h->prec);
            HIPCHK(h, panel16[c].alloc(bytes16));
            HIPCHK(h, hipMemsetAsync(panel16[c].p, 0, bytes16, st));
        }
        pack.add(mc::pack_job_dgrad(weight_oihw, Cout, CinTotal, ksize, c_off, Cs, Cout, cls, panel[c].as<float>(), panel16[c].p,
                                    h->prec, w_amax));
    }
    hipError_t e = pack.launch(st);
    for (int c = 0; c < nclass && e == hipSuccess; ++c) {
        mc::ConvPlan d;
        mc::dgrad_conv_args(d, pack.jobs[c], h->prec, dy, dy_amax, B, Ho, Wo, Cout, dx, Hin, Win, accumulate != 0);
        d.a.cfg = h->force_cfg;
        mc::conv_plan(d);
        e = mc::launch_conv(d, st);
    }
    hipError_t e2 = hipStreamSynchronize(st);   // test entry point: the panels are temporaries
    HIPCHK(h, e);
    HIPCHK(h, e2);
    return 0;
}

// uploads a tensor table with its 65536-element chunk list (replacing the one *dtab / *dchunks hold)
static int upload_opt_table(mc_handle *h, const std::vector<mc::OptTensor> &tab, const int64_t numel[], mc::OptTensor **dtab,
                            mc::OptChunk **dchunks, int *nchunks) {
    std::vector<mc::OptChunk> chunks;
    const int CH = 1 << 16;
    for (int i = 0; i < (int)tab.size(); ++i)
        for (int64_t b = 0; b < numel[i]; b += CH)
            chunks.push_back(mc::OptChunk{i, (int)b, (int)std::min<int64_t>(CH, numel[i] - b)});
    if (*dtab) (void)hipFree(*dtab);
    if (*dchunks) (void)hipFree(*dchunks);
    *dtab = nullptr; *dchunks = nullptr; *nchunks = 0;
    void *q = nullptr;
    HIPCHK(h, hipMalloc(&q, tab.size() * sizeof(mc::OptTensor)));
    *dtab = static_cast<mc::OptTensor *>(q);
    HIPCHK(h, hipMalloc(&q, chunks.size() * sizeof(mc::OptChunk)));
    *dchunks = static_cast<mc::OptChunk *>(q);
    HIPCHK(h, hipMemcpy(*dtab, tab.data(), tab.size() * sizeof(mc::OptTensor), hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(*dchunks, chunks.data(), chunks.size() * sizeof(mc::OptChunk), hipMemcpyHostToDevice));
    *nchunks = (int)chunks.size();
    if (!h->opt_ws) {
        HIPCHK(h, hipMalloc(&q, (mc::opt_partial_floats() + 8) * sizeof(float)));
        h->opt_ws = static_cast<float *>(q);
    }
    return 0;
}

static int optim_bind(mc_handle *h, const char *who, int n, float *const params[], float *const grads[], float *const exp_avg[],
                      float *const exp_avg_sq[], float *const max_exp_avg_sq[], const int64_t numel[], const int cls[]) {
    if (!h) return -1;
    if (n < 1 || !params || !grads || !exp_avg || !exp_avg_sq || !numel) return fail(h, "%s: bad argument", who);
    HIPCHK(h, hipSetDevice(h->device));
    std::vector<mc::OptTensor> tab(n);
    int max_cls = 0;
    unsigned novmax = 0;
    for (int i = 0; i < n; ++i) {
        if (!params[i] || !grads[i] || !exp_avg[i] || !exp_avg_sq[i] || numel[i] < 1)
            return fail(h, "%s: tensor %d has a null pointer / empty size", who, i);
        if (numel[i] > INT32_MAX) return fail(h, "%s: tensor %d has more than 2^31-1 elements", who, i);
        const int c = cls ? cls[i] : 0;
        if (c < 0 || c >= MC_OPT_MAX_CLASSES)
            return fail(h, "%s: tensor %d has class index %d, outside [0, %d)", who, i, c, MC_OPT_MAX_CLASSES);
        float *vmax = max_exp_avg_sq ? max_exp_avg_sq[i] : nullptr;
        tab[i] = mc::OptTensor{params[i], grads[i], exp_avg[i], exp_avg_sq[i], vmax, c};
        max_cls = std::max(max_cls, c);
        if (!vmax) novmax |= 1u << c;
    }
    h->opt_ntensors = 0;
    h->opt_has_ema = false;     // a new table has no averages: mc_optim_bind_ema attaches them again
    if (h->lamb_ws.chunk_sums) (void)hipFree(h->lamb_ws.chunk_sums);    // the LAMB workspace goes with the table it was sized for
    h->lamb_ws = mc::LambWorkspace{nullptr, nullptr, nullptr};
    h->lamb_ran = false;
    h->opt_host.clear();
    h->opt_numel.clear();
    if (upload_opt_table(h, tab, numel, &h->opt_tab, &h->opt_chunks, &h->opt_nchunks)) return -1;
    h->opt_ntensors = n;
    h->opt_max_cls = max_cls;
    h->opt_novmax = novmax;
    h->opt_host = tab;
    h->opt_numel.assign(numel, numel + n);
    return 0;
}

static bool ranges_overlap(const float *a, const float *b, int64_t n) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b), len = (uintptr_t)n * sizeof(float);
    return x < y + len && y < x + len;
}

int mc_optim_bind_ema(mc_handle *h, int n, float *const ema[]) {
    if (!h) return -1;
    if (!h->opt_tab || h->opt_ntensors < 1) return fail(h, "mc_optim_bind_ema: call mc_optim_bind or mc_optim_bind_classes first");
    if (!ema) return fail(h, "mc_optim_bind_ema: bad argument");
    if (n != h->opt_ntensors)
        return fail(h, "mc_optim_bind_ema: %d averages for a bound table of %d tensors", n, h->opt_ntensors);
    bool any = false;
    for (int i = 0; i < n; ++i) {
        if (!ema[i]) continue;
        if (ranges_overlap(ema[i], h->opt_host[i].p, h->opt_numel[i]))
            return fail(h, "mc_optim_bind_ema: the average of tensor %d aliases its parameter", i);
        any = true;
    }
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipDeviceSynchronize());      // a step in flight still reads the table
    std::vector<mc::OptTensor> tab = h->opt_host;
    for (int i = 0; i < n; ++i) tab[i].e = ema[i];
    HIPCHK(h, hipMemcpy(h->opt_tab, tab.data(), tab.size() * sizeof(mc::OptTensor), hipMemcpyHostToDevice));
    h->opt_host.swap(tab);
    h->opt_has_ema = any;
    return 0;
}

int mc_optim_bind(mc_handle *h, int n, float *const params[], float *const grads[], float *const exp_avg[],
                  float *const exp_avg_sq[], const int64_t numel[]) {
    return optim_bind(h, "mc_optim_bind", n, params, grads, exp_avg, exp_avg_sq, nullptr, numel, nullptr);
}

int mc_optim_bind_classes(mc_handle *h, int n, float *const params[], float *const grads[], float *const exp_avg[],
                          float *const exp_avg_sq[], float *const max_exp_avg_sq[], const int64_t numel[], const int cls[]) {
    if (h && !cls) return fail(h, "mc_optim_bind_classes: bad argument");
    return optim_bind(h, "mc_optim_bind_classes", n, params, grads, exp_avg, exp_avg_sq, max_exp_avg_sq, numel, cls);
}

static void fold_hyper(mc::AdamHyper &hp, double lr, double beta1, double beta2, double eps, double weight_decay, int step) {
    const double bc1 = 1.0 - std::pow(beta1, (double)step), bc2 = 1.0 - std::pow(beta2, (double)step);
    hp.decay = (float)(1.0 - lr * weight_decay);
    hp.beta1 = (float)beta1; hp.one_minus_beta1 = (float)(1.0 - beta1);
    hp.beta2 = (float)beta2; hp.one_minus_beta2 = (float)(1.0 - beta2);
    hp.sqrt_bc2 = (float)std::sqrt(bc2);
    hp.eps = (float)eps;
    hp.step_size = (float)(lr / bc1);
}

int mc_clip_adamw_step(mc_handle *h, double lr, double beta1, double beta2, double eps, double weight_decay,
                       double max_norm, int step, float *out_norm, void *stream) {
    if (!h) return -1;
    if (!h->opt_tab) return fail(h, "mc_clip_adamw_step: call mc_optim_bind first");
    if (step < 1) return fail(h, "mc_clip_adamw_step: step must be >= 1 (1-based, as torch.optim counts)");
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    mc::AdamHyper hp;
    fold_hyper(hp, lr, beta1, beta2, eps, weight_decay, step);
    float *normcoef = h->opt_ws + mc::opt_partial_floats();
    mc::GuardRecord *guard = h->opt_guard_on ? h->opt_guard : nullptr;    // null: the launches of always
    HIPCHK(h, mc::launch_clip_adamw(h->opt_tab, h->opt_chunks, h->opt_nchunks, h->opt_ws, normcoef, (float)max_norm, hp, st, 0.f, guard));
    if (guard) h->opt_guard_ran = true;
    if (out_norm) HIPCHK(h, hipMemcpyAsync(out_norm, normcoef, sizeof(float), hipMemcpyDeviceToDevice, st));
    h->pack_clean = false;   // parameters changed: the packed panels are stale
    return 0;
}

static bool bad_norm_type(double p) { return !(p > 0.0); }   // p <= 0 and NaN

// ema_weight: w = 1 - decay of this step's weight average; 0 (or a table without averages) is the step without it
static int step_classes(mc_handle *h, const char *who, const mc_optim_class *classes, int ncls, double max_norm, double norm_type,
                        double ema_weight, float *out_norm, void *stream) {
    if (!h) return -1;
    if (!(ema_weight >= 0.0 && ema_weight <= 1.0)) return fail(h, "%s: ema_weight must lie in [0, 1], got %g", who, ema_weight);
    if (!h->opt_tab) return fail(h, "%s: call mc_optim_bind_classes first", who);
    if (!classes || ncls < 1) return fail(h, "%s: bad argument", who);
    if (ncls > MC_OPT_MAX_CLASSES)
        return fail(h, "%s: %d hyper-parameter classes (distinct lr / betas / eps / weight_decay / step / amsgrad / maximize), "
                       "at most %d fit one launch", who, ncls, MC_OPT_MAX_CLASSES);
    if (bad_norm_type(norm_type)) return fail(h, "%s: norm_type must be > 0 (inf allowed), got %g", who, norm_type);
    if (max_norm != max_norm) return fail(h, "%s: max_norm is NaN", who);
    if (h->opt_max_cls >= ncls)
        return fail(h, "%s: the bound table uses class index %d but only %d classes were given", who, h->opt_max_cls, ncls);
    mc::AdamTable tb{};
    for (int c = 0; c < ncls; ++c) {
        const mc_optim_class &k = classes[c];
        if (k.step < 1) return fail(h, "%s: class %d: step must be >= 1 (1-based, as torch.optim counts)", who, c);
        if (k.amsgrad && ((h->opt_novmax >> c) & 1u))
            return fail(h, "%s: class %d is amsgrad but one of its tensors was bound without max_exp_avg_sq", who, c);
        fold_hyper(tb.hp[c], k.lr, k.beta1, k.beta2, k.eps, k.weight_decay, k.step);
        if (k.amsgrad) tb.amsgrad |= 1u << c;
        if (k.maximize) tb.maximize |= 1u << c;
    }
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    float *normcoef = h->opt_ws + mc::opt_partial_floats();
    // the EMA instantiations only when there is something to average: in every other case the launches are the old ones
    const float ema_w = h->opt_has_ema ? (float)ema_weight : 0.f;
    mc::GuardRecord *guard = h->opt_guard_on ? h->opt_guard : nullptr;    // null: the launches of always
    if (ncls == 1 && !tb.amsgrad && !tb.maximize && norm_type == 2.0) {
        // the reference recipe: the very launch mc_clip_adamw_step makes
        HIPCHK(h, mc::launch_clip_adamw(h->opt_tab, h->opt_chunks, h->opt_nchunks, h->opt_ws, normcoef, (float)max_norm, tb.hp[0], st, ema_w, guard));
    } else {
        HIPCHK(h, mc::launch_grad_norm(h->opt_tab, h->opt_chunks, h->opt_nchunks, h->opt_ws, normcoef, (float)max_norm, norm_type, st, guard));
        HIPCHK(h, mc::launch_adamw_classes(h->opt_tab, h->opt_chunks, h->opt_nchunks, normcoef, tb, st, ema_w, guard));
    }
    if (guard) h->opt_guard_ran = true;
    if (out_norm) HIPCHK(h, hipMemcpyAsync(out_norm, normcoef, sizeof(float), hipMemcpyDeviceToDevice, st));
    h->pack_clean = false;   // parameters changed: the packed panels are stale
    return 0;
}

int mc_clip_adamw_step_classes(mc_handle *h, const mc_optim_class *classes, int ncls, double max_norm, double norm_type,
                               float *out_norm, void *stream) {
    return step_classes(h, "mc_clip_adamw_step_classes", classes, ncls, max_norm, norm_type, 0.0, out_norm, stream);
}

int mc_clip_adamw_ema_step_classes(mc_handle *h, const mc_optim_class *classes, int ncls, double max_norm, double norm_type,
                                   double ema_weight, float *out_norm, void *stream) {
    return step_classes(h, "mc_clip_adamw_ema_step_classes", classes, ncls, max_norm, norm_type, ema_weight, out_norm, stream);
}

// ---- LAMB: the per-tensor trust ratio on the same table, the same global norm and the same guard
// chunk sums [2 * nchunks], ratio [n] (1 before the first step), first_chunk [n + 1]: one allocation per bound table
static int ensure_lamb_ws(mc_handle *h) {
    if (h->lamb_ws.chunk_sums) return 0;
    const int n = h->opt_ntensors;
    const size_t nsums = 2 * (size_t)h->opt_nchunks;
    std::vector<float> host(nsums + n + n + 1, 0.f);
    std::fill(host.begin() + nsums, host.begin() + nsums + n, 1.f);
    int first = 0;      // upload_opt_table lists the chunks tensor by tensor, 65536 elements each
    for (int i = 0; i <= n; ++i) {
        std::memcpy(&host[nsums + n + i], &first, sizeof(int));
        if (i < n) first += (int)((h->opt_numel[i] + 65535) >> 16);
    }
    if (first != h->opt_nchunks) return fail(h, "mc_clip_lamb_step_classes: the chunk list does not match the bound sizes");
    void *q = nullptr;
    HIPCHK(h, hipMalloc(&q, host.size() * sizeof(float)));
    const hipError_t e = hipMemcpy(q, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) (void)hipFree(q);
    HIPCHK(h, e);
    float *base = static_cast<float *>(q);
    h->lamb_ws = mc::LambWorkspace{base, base + nsums, reinterpret_cast<int *>(base + nsums + n)};
    return 0;
}

int mc_clip_lamb_step_classes(mc_handle *h, const mc_optim_class *classes, int ncls, unsigned adapt_mask, double trust_clip,
                              double max_norm, double norm_type, double ema_weight, float *out_norm, void *stream) {
    const char *who = "mc_clip_lamb_step_classes";
    if (!h) return -1;
    if (!h->opt_tab || h->opt_ntensors < 1) return fail(h, "%s: call mc_optim_bind_classes first", who);
    if (!classes || ncls < 1) return fail(h, "%s: bad argument", who);
    if (ncls > MC_OPT_MAX_CLASSES)
        return fail(h, "%s: %d hyper-parameter classes (distinct lr / betas / eps / weight_decay / step / maximize / adapts), "
                       "at most %d fit one launch", who, ncls, MC_OPT_MAX_CLASSES);
    if (h->opt_max_cls >= ncls)
        return fail(h, "%s: the bound table uses class index %d but only %d classes were given", who, h->opt_max_cls, ncls);
    mc::LambTable tb{};
    for (int c = 0; c < ncls; ++c) {
        const mc_optim_class &k = classes[c];
        if (k.step < 1) return fail(h, "%s: class %d: step must be >= 1 (1-based, as torch.optim counts)", who, c);
        mc::LambHyper &hp = tb.hp[c];
        hp.beta1 = (float)k.beta1; hp.one_minus_beta1 = (float)(1.0 - k.beta1);
        hp.beta2 = (float)k.beta2; hp.one_minus_beta2 = (float)(1.0 - k.beta2);
        hp.sqrt_bc2 = (float)std::sqrt(1.0 - std::pow(k.beta2, (double)k.step));
        hp.eps = (float)k.eps;
        hp.bc1 = (float)(1.0 - std::pow(k.beta1, (double)k.step));
        hp.wd = (float)k.weight_decay;
        hp.lr = (float)k.lr;
        if (k.maximize) tb.maximize |= 1u << c;
    }
    if (bad_norm_type(norm_type)) return fail(h, "%s: norm_type must be > 0 (inf allowed), got %g", who, norm_type);
    if (max_norm != max_norm) return fail(h, "%s: max_norm is NaN", who);
    for (int c = 0; c < ncls; ++c)
        if (classes[c].amsgrad) return fail(h, "%s: class %d is amsgrad, which the LAMB step does not support", who, c);
    if (ncls < 32 && (adapt_mask >> ncls)) return fail(h, "%s: adapt_mask 0x%x has bits at or above ncls = %d", who, adapt_mask, ncls);
    if (!(trust_clip >= 0.0) || std::isinf(trust_clip))
        return fail(h, "%s: trust_clip must be finite and >= 0 (0: no cap), got %g", who, trust_clip);
    if (trust_clip > 0.0 && !((float)trust_clip > 0.f && !std::isinf((float)trust_clip)))
        return fail(h, "%s: trust_clip %g is no positive finite float", who, trust_clip);
    if (!(ema_weight >= 0.0 && ema_weight <= 1.0)) return fail(h, "%s: ema_weight must lie in [0, 1], got %g", who, ema_weight);
    tb.adapt = adapt_mask;
    tb.trust_clip = (float)trust_clip;
    HIPCHK(h, hipSetDevice(h->device));
    if (ensure_lamb_ws(h)) return -1;
    hipStream_t st = static_cast<hipStream_t>(stream);
    float *normcoef = h->opt_ws + mc::opt_partial_floats();
    const float ema_w = h->opt_has_ema ? (float)ema_weight : 0.f;
    mc::GuardRecord *guard = h->opt_guard_on ? h->opt_guard : nullptr;
    HIPCHK(h, mc::launch_grad_norm(h->opt_tab, h->opt_chunks, h->opt_nchunks, h->opt_ws, normcoef, (float)max_norm, norm_type, st, guard));
    HIPCHK(h, mc::launch_lamb_classes(h->opt_tab, h->opt_chunks, h->opt_nchunks, h->opt_ntensors, normcoef, tb, h->lamb_ws, st, ema_w, guard));
    if (guard) h->opt_guard_ran = true;
    h->lamb_ran = true;
    if (out_norm) HIPCHK(h, hipMemcpyAsync(out_norm, normcoef, sizeof(float), hipMemcpyDeviceToDevice, st));
    h->pack_clean = false;   // parameters changed: the packed panels are stale
    return 0;
}

int mc_lamb_ratios(mc_handle *h, float *dst, int n, void *stream) {
    if (!h) return -1;
    if (!h->opt_tab || !h->lamb_ran) return fail(h, "mc_lamb_ratios: no mc_clip_lamb_step_classes has run on the bound table");
    if (!dst) return fail(h, "mc_lamb_ratios: bad argument");
    if (n != h->opt_ntensors) return fail(h, "mc_lamb_ratios: room for %d ratios, the bound table has %d tensors", n, h->opt_ntensors);
    HIPCHK(h, hipSetDevice(h->device));
    // an asynchronous copy needs device or page-locked host memory (as mc_optim_guard_report)
    hipPointerAttribute_t attr{};
    const hipError_t e = hipPointerGetAttributes(&attr, dst);
    if (e != hipSuccess) (void)hipGetLastError();
    if (e != hipSuccess || (attr.type != hipMemoryTypeDevice && attr.type != hipMemoryTypeHost))
        return fail(h, "mc_lamb_ratios: dst must be device memory or page-locked host memory");
    HIPCHK(h, hipMemcpyAsync(dst, h->lamb_ws.ratio, (size_t)n * sizeof(float), hipMemcpyDefault, static_cast<hipStream_t>(stream)));
    return 0;
}

int mc_clip_bind(mc_handle *h, int n, float *const grads[], const int64_t numel[]) {
    if (!h) return -1;
    if (n < 1 || !grads || !numel) return fail(h, "mc_clip_bind: bad argument");
    HIPCHK(h, hipSetDevice(h->device));
    std::vector<mc::OptTensor> tab(n);
    for (int i = 0; i < n; ++i) {
        if (!grads[i] || numel[i] < 1) return fail(h, "mc_clip_bind: tensor %d has a null pointer / empty size", i);
        if (numel[i] > INT32_MAX) return fail(h, "mc_clip_bind: tensor %d has more than 2^31-1 elements", i);
        tab[i] = mc::OptTensor{nullptr, grads[i], nullptr, nullptr, nullptr, 0};
    }
    return upload_opt_table(h, tab, numel, &h->clip_tab, &h->clip_chunks, &h->clip_nchunks);
}

int mc_clip_grad_norm(mc_handle *h, double max_norm, double norm_type, float *out_norm, void *stream) {
    if (!h) return -1;
    if (!h->clip_tab) return fail(h, "mc_clip_grad_norm: call mc_clip_bind first");
    if (bad_norm_type(norm_type)) return fail(h, "mc_clip_grad_norm: norm_type must be > 0 (inf allowed), got %g", norm_type);
    if (max_norm != max_norm) return fail(h, "mc_clip_grad_norm: max_norm is NaN");
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    float *normcoef = h->opt_ws + mc::opt_partial_floats();
    HIPCHK(h, mc::launch_grad_norm(h->clip_tab, h->clip_chunks, h->clip_nchunks, h->opt_ws, normcoef, (float)max_norm, norm_type, st));
    if (max_norm > 0.0) HIPCHK(h, mc::launch_grad_scale(h->clip_tab, h->clip_chunks, h->clip_nchunks, normcoef, st));
    if (out_norm) HIPCHK(h, hipMemcpyAsync(out_norm, normcoef, sizeof(float), hipMemcpyDeviceToDevice, st));
    return 0;
}

int mc_ema_bind(mc_handle *h, int n, float *const ema[], const float *const src[], const int64_t numel[]) {
    if (!h) return -1;
    if (n < 1 || !ema || !src || !numel) return fail(h, "mc_ema_bind: bad argument");
    HIPCHK(h, hipSetDevice(h->device));
    std::vector<mc::OptTensor> tab(n);
    for (int i = 0; i < n; ++i) {
        if (!ema[i] || !src[i] || numel[i] < 1) return fail(h, "mc_ema_bind: tensor %d has a null pointer / empty size", i);
        if (numel[i] > INT32_MAX) return fail(h, "mc_ema_bind: tensor %d has more than 2^31-1 elements", i);
        if (ranges_overlap(ema[i], src[i], numel[i])) return fail(h, "mc_ema_bind: the average of tensor %d aliases its source", i);
        // the table's .p is the average, its .g the source it follows
        tab[i] = mc::OptTensor{ema[i], const_cast<float *>(src[i]), nullptr, nullptr, nullptr, 0};
    }
    return upload_opt_table(h, tab, numel, &h->ema_tab, &h->ema_chunks, &h->ema_nchunks);
}

int mc_ema_update(mc_handle *h, double ema_weight, void *stream) {
    if (!h) return -1;
    if (!h->ema_tab) return fail(h, "mc_ema_update: call mc_ema_bind first");
    if (!(ema_weight >= 0.0 && ema_weight <= 1.0)) return fail(h, "mc_ema_update: ema_weight must lie in [0, 1], got %g", ema_weight);
    if ((float)ema_weight == 0.f) return 0;     // the average stays as it is, bit for bit (fmaf(0, x, -0) would be +0)
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, mc::launch_ema(h->ema_tab, h->ema_chunks, h->ema_nchunks, (float)ema_weight, static_cast<hipStream_t>(stream)));
    return 0;
}

// ---- gradient accumulation over a window of micro-batches
int mc_accum_bind(mc_handle *h, int n, float *const grads[], float *const acc[], const int64_t numel[]) {
    if (!h) return -1;
    if (n < 1 || !grads || !acc || !numel) return fail(h, "mc_accum_bind: bad argument");
    std::vector<mc::OptTensor> tab(n);
    for (int i = 0; i < n; ++i) {
        if (!grads[i] || !acc[i] || numel[i] < 1) return fail(h, "mc_accum_bind: tensor %d has a null pointer / empty size", i);
        if (numel[i] > INT32_MAX) return fail(h, "mc_accum_bind: tensor %d has more than 2^31-1 elements", i);
        if (ranges_overlap(acc[i], grads[i], numel[i])) return fail(h, "mc_accum_bind: the accumulator of tensor %d aliases its gradient", i);
        // the table's .p is the accumulator, its .g the gradient
        tab[i] = mc::OptTensor{acc[i], grads[i], nullptr, nullptr, nullptr, 0};
    }
    HIPCHK(h, hipSetDevice(h->device));
    h->accum_open = false;      // a window does not survive its table: ADD / FINISH need a BEGIN on the new one
    return upload_opt_table(h, tab, numel, &h->accum_tab, &h->accum_chunks, &h->accum_nchunks);
}

int mc_grad_accumulate(mc_handle *h, int mode, double scale, void *stream) {
    if (!h) return -1;
    if (!h->accum_tab) return fail(h, "mc_grad_accumulate: call mc_accum_bind first");
    if (mode != MC_ACCUM_BEGIN && mode != MC_ACCUM_ADD && mode != MC_ACCUM_FINISH)
        return fail(h, "mc_grad_accumulate: unknown mode %d (MC_ACCUM_BEGIN, MC_ACCUM_ADD or MC_ACCUM_FINISH)", mode);
    if (mode != MC_ACCUM_BEGIN && !h->accum_open)
        return fail(h, "mc_grad_accumulate: %s without an open window (MC_ACCUM_BEGIN first; mc_accum_bind and MC_ACCUM_FINISH close it)",
                    mode == MC_ACCUM_ADD ? "MC_ACCUM_ADD" : "MC_ACCUM_FINISH");
    // !(scale > 0) is NaN, zero and negative; a float that overflows or underflows is no mean of a window either
    if (mode == MC_ACCUM_FINISH && (!(scale > 0.0) || std::isinf(scale) || !((float)scale > 0.f) || std::isinf((float)scale)))
        return fail(h, "mc_grad_accumulate: MC_ACCUM_FINISH needs a finite scale > 0 (1 / micro-batches of the window), got %g", scale);
    HIPCHK(h, hipSetDevice(h->device));
    const float s = mode == MC_ACCUM_FINISH ? (float)scale : 1.f;      // BEGIN and ADD ignore it
    HIPCHK(h, mc::launch_grad_accum(h->accum_tab, h->accum_chunks, h->accum_nchunks, mode, s, static_cast<hipStream_t>(stream)));
    h->accum_open = mode != MC_ACCUM_FINISH;
    return 0;
}

// ---- non-finite guard
int mc_optim_set_guard(mc_handle *h, int on) {
    if (!h) return -1;
    if (!on) {
        h->opt_guard_on = h->opt_guard_ran = false;
        return 0;
    }
    if (h->opt_guard_on) return 0;
    HIPCHK(h, hipSetDevice(h->device));
    if (!h->opt_guard) {
        void *q = nullptr;
        HIPCHK(h, hipMalloc(&q, sizeof(mc::GuardRecord)));
        h->opt_guard = static_cast<mc::GuardRecord *>(q);
    } else {
        HIPCHK(h, hipDeviceSynchronize());      // a report of the guard's earlier life may still read the record
    }
    const mc::GuardRecord none{0, -1, 0ull, 0.f, 0};
    HIPCHK(h, hipMemcpy(h->opt_guard, &none, sizeof(none), hipMemcpyHostToDevice));
    h->opt_guard_on = true;
    h->opt_guard_ran = false;
    return 0;
}

static_assert(sizeof(mc_guard_report) == sizeof(mc::GuardRecord), "mc_guard_report is the device record");

int mc_optim_guard_report(mc_handle *h, mc_guard_report *dst, void *stream) {
    if (!h) return -1;
    if (!h->opt_guard_on || !h->opt_guard) return fail(h, "mc_optim_guard_report: the guard is off (mc_optim_set_guard)");
    if (!dst) return fail(h, "mc_optim_guard_report: bad argument");
    HIPCHK(h, hipSetDevice(h->device));
    // an asynchronous copy needs device or page-locked host memory: into pageable memory it would block, or land late
    hipPointerAttribute_t attr{};
    const hipError_t e = hipPointerGetAttributes(&attr, dst);
    if (e != hipSuccess) (void)hipGetLastError();       // an address the runtime does not know
    if (e != hipSuccess || (attr.type != hipMemoryTypeDevice && attr.type != hipMemoryTypeHost))
        return fail(h, "mc_optim_guard_report: dst must be device memory or page-locked host memory");
    HIPCHK(h, hipMemcpyAsync(dst, h->opt_guard, sizeof(mc_guard_report), hipMemcpyDefault, static_cast<hipStream_t>(stream)));
    return 0;
}

int mc_ema_update_guarded(mc_handle *h, double ema_weight, void *stream) {
    if (!h) return -1;
    if (!h->opt_guard_on || !h->opt_guard_ran) return mc_ema_update(h, ema_weight, stream);
    if (!h->ema_tab) return fail(h, "mc_ema_update_guarded: call mc_ema_bind first");
    if (!(ema_weight >= 0.0 && ema_weight <= 1.0)) return fail(h, "mc_ema_update_guarded: ema_weight must lie in [0, 1], got %g", ema_weight);
    if ((float)ema_weight == 0.f) return 0;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, mc::launch_ema(h->ema_tab, h->ema_chunks, h->ema_nchunks, (float)ema_weight, static_cast<hipStream_t>(stream), h->opt_guard));
    return 0;
}

}  // extern "C"
