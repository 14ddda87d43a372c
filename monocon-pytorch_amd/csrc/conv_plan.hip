// Which kernel runs a conv launch (forward conv or data gradient) and with which build: decided HERE, once per launch
// description, and only looked up afterwards (host code only).  What a kernel can run stays beside it (conv_small_ok,
// conv_small_lazy_ok, conv_thin_ok, conv_bf16_ok, conv_wres_ok, conv_pick_cfg, conv_ck) and is asked here alone.
// A new kernel: one ConvKernel id, one branch, one launch_conv_*.
#include <cstdlib>
#include "conv_mfma.h"

namespace mc {

thread_local ProfLast prof_last = {0, 0.0, 0.0};
static ProfLast conv_cost(const ConvArgs &a, int ks) {
    const double px_in = (double)a.B * a.Hin * a.Win, px_out = (double)a.B * a.Hout * a.Wout;
    const double taps = win_h(ks) * win_w(ks);
    // algorithmic bytes: the input, the output (+ the residual / the gradient accumulated into), the weights, and for a
    // backward-statistics launch the forward's y (and z where the ReLU mask is the stored activation's)
    const int extra = (a.res ? 1 : 0) + (a.bm_y ? 1 : 0) + ((a.bm_y && a.bm_relu == 1 && !a.bm_zbits) ? 1 : 0);      // (a bit-packed mask is 1/32 of a map: not counted)
    return {1, 2.0 * px_out * a.Cout * a.Cin * taps,
            4.0 * (px_in * a.Cin + px_out * a.Cout * (1 + extra) + taps * a.Cin * a.Cout)};
}

void conv_plan(ConvPlan &p) {
    ConvArgs &a = p.a;
    const int ks = p.ks, stride = p.stride;
    const bool lazy = conv_any_lazy(a), bm = a.bm_y != nullptr;
    // dense NHWC output / residual: given as 0, or as the mapping an earlier plan of this block wrote
    const bool dense_out = a.o_px == 0 || (a.o_px == a.out_ld && a.o_row == a.Wout * a.out_ld && a.o_img == a.Hout * a.Wout * a.out_ld);
    if (dense_out) { a.o_px = a.out_ld; a.o_row = a.Wout * a.out_ld; a.o_img = a.Hout * a.Wout * a.out_ld; }
    if (a.r_px == 0) { a.r_px = a.res_ld; a.r_row = a.Wout * a.res_ld; a.r_img = a.Hout * a.Wout * a.res_ld; }
    a.ppr = (a.Wout + 7) / 8;
    a.ppi = a.chunks = a.ppr * ((a.Hout + 3) / 4);      // (chunks: workgroup chunks per image, the tilings own PB patches each)
    const bool row = conv_small_ok(a, ks, stride), thin = conv_thin_ok(a, ks, stride), row_lazy = conv_small_lazy_ok(a, ks, stride);
    const bool b16 = a.prec >= 1 && conv_bf16_ok(a, ks, stride);
    const bool s1_31 = stride == 1 && (ks == 3 || ks == 1);      // the windows with a backward-statistics build of the tilings
    // the tiling the id names (CFG_AUTO: the default for the layer), whether or not the launch ends up on a tiled kernel
    int cfg = a.cfg == CFG_AUTO ? conv_pick_cfg(a.Cout, a.CoutP, ks, stride, a.B, a.Hout, a.Wout) : a.cfg;
    p.kernel = CONV_FP32; p.shape = conv_shape(cfg).id; p.ck = p.spl = 0; p.bm = p.lz = p.ok = p.bm_ok = false;
    p.row_ok = row; p.b16 = b16;
    p.lazy_ok = a.prec == 3 && !bm && (thin || row_lazy || (b16 && (ks == 3 || ks == 1)));
    p.stat_rows = a.cfg == CFG_SMALL ? a.Hout : a.ppi;
    // everything below mirrors ONE chain; `return` with p.ok false = the launch is refused
    if (a.cfg == CFG_SMALL && !dense_out) return;
    int sc[4];
    for (int i = 0; i < a.nsrc; ++i) sc[i] = a.src[i].C;
    const int ck = conv_ck(ks, stride, sc, a.nsrc);
    for (int i = 0; i < a.nsrc; ++i)
        if (sc[i] % ck) return;
    if (a.cfg == CFG_SMALL) {       // the row family: mode 3's fp16-pipe kernel where it qualifies, else the fp32 row kernel
        if (!row || (lazy && !thin && !row_lazy)) return;
        p.kernel = thin ? CONV_THIN16 : (a.src[0].la ? CONV_ROW_LAZY : CONV_ROW);
        a.chunks = a.Hout;      // one statistics partial per output row
        p.ok = true; p.bm_ok = thin && !lazy;      // (the fp32 row kernel has no backward-statistics epilogue and ignores bm_y)
        return;
    }
    if (cfg & CFG_WRES) {
        // MONOCON_HIP_WRES=0: A/B switch, every launch takes the tiling its shape bits name
        static const bool wres_on = [] { const char *e = std::getenv("MONOCON_HIP_WRES"); return !e || std::atoi(e) != 0; }();
        if (wres_on && conv_wres_ok(a, ks, stride)) {
            p.kernel = CONV_WRES; p.bm = bm; p.lz = a.src[0].la != nullptr;
            p.ok = !(p.lz && (bm || !a.src[0].lb));      // lazy source: forward launches (no backward-statistics twin reads an activation)
            p.bm_ok = p.ok && !lazy;
            return;
        }
        cfg &= ~CFG_WRES;       // not eligible: the tiling the shape bits name
    }
    if (b16) {
        p.kernel = CONV_SPLIT; p.spl = split_pieces(a.prec);
        // lazy sources: forward launches of the fp16-split mode (3x3 stride 1 / 2 and 1x1), never a data gradient
        if (lazy && (p.spl != 2 || !(ks == 3 || ks == 1) || bm)) return;
        p.lz = lazy;
    } else {
        if (lazy) return;      // (nor do the fp32 MFMA kernels)
        if (ks >= 10) cfg &= ~CFG_WS;      // the stride-2 data-gradient parity classes have no wave-specialised build
        if (with_conv_window(ks, stride, [](auto) { return hipSuccess; }) != hipSuccess) return;
        if (cfg & ~(CFG_SHAPE_BITS | CFG_WS)) return;
        if ((cfg & CFG_WS) && !bm) p.kernel = CONV_FP32_WS;      // (the WS variant has no bm epilogue: such a launch runs plain)
        p.ck = ck;
    }
    const ConvShape sh = conv_shape(cfg);      // (ids 2, 3 are retired: no entry)
    if (!sh.id || (bm && !s1_31)) return;
    p.bm = bm;
    a.chunks = (a.ppi + sh.PB() - 1) / sh.PB();
    if (a.CoutP % sh.BNT()) return;
    p.ok = true; p.bm_ok = s1_31 && !lazy;
}

hipError_t launch_conv(const ConvPlan &p, hipStream_t st) {
    if (!p.ok) return hipErrorInvalidValue;
    prof_last = conv_cost(p.a, p.ks);
    switch (p.kernel) {
    case CONV_FP32: case CONV_FP32_WS: return launch_conv_fp32(p, st);
    case CONV_SPLIT: return launch_conv_bf16(p, st);
    case CONV_WRES: return launch_conv_wres(p, st);
    case CONV_ROW: case CONV_ROW_LAZY: return launch_conv_small(p, st);
    case CONV_THIN16: return launch_conv_thin(p, st);
    }
    return hipErrorInvalidValue;
}

}  // namespace mc
