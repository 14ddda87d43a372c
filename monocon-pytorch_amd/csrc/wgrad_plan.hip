// Which kernel runs a conv's weight gradient and how its launch is tiled: decided HERE, once per launch description, and only
// looked up afterwards (host code only).  What a kernel can run stays beside it (wgrad_is_small, wgrad_thin_ok, wgrad_pipe_tile,
// wgrad_shape, wgrad_sources_ok, wgrad_bf16_ok) and is asked here alone.  A new kernel: one WgKernel id, one branch, one launch_wgrad_*.
#include <algorithm>
#include <cstdlib>
#include "conv_mfma.h"
#include "train.h"

namespace mc {

// (the knobs are read per plan, not cached: the tests change them between two launches of one process)
static int env_int(const char *name, int unset) { const char *e = std::getenv(name); return e ? std::atoi(e) : unset; }

void wgrad_plan(WgradPlan &p) {
    WgradArgs &a = p.a;
    const int ks = p.ks, stride = p.stride;
    a.pipe = p.WN = p.WC = 0; p.ok = true;
    if (wgrad_is_small(a, ks, stride)) {
        a.kernel = wgrad_thin_ok(a, ks, stride) ? WG_THIN16 : WG_SMALL;
        // (wgrad_small_kernel<2, 2, LZ>: the stride-2 16 -> 32 layer, DLA level1, is the one that needs it)
        p.lazy_ok = a.prec == 3 && (a.kernel == WG_THIN16 || (stride == 2 && a.Cout == 32));
        const int rows = a.B * a.Hout;
        a.ksplit = std::min(rows / 4 > 0 ? rows / 4 : 1, 1024);   // >= 4 rows (one per wave) per workgroup
        a.n_tiles = a.c_tiles = 1; a.ppr = a.ppi = a.groups_per_img = 0;
    } else {
        int budget, WK = 1;      // workgroups to spread over the (n, c) tiles; K halves inside a workgroup
        if (const int tile = wgrad_pipe_tile(a, ks, stride)) {
            a.kernel = WG_PIPE; a.pipe = tile; a.pb = 1;
            p.WN = tile == 1 ? 4 : 2; p.WC = tile == 2 ? 4 : 2; WK = tile == 3 ? 2 : 1;
            p.lazy_ok = tile == 4;
            budget = env_int("MONOCON_HIP_WGRAD_PIPE_BLOCKS", 256);      // one resident 8-wave workgroup per CU
        } else {
            wgrad_shape(a, &p.WN, &p.WC);
            const bool b16 = a.prec >= 1 && wgrad_bf16_ok(a, ks, stride), src_ok = wgrad_sources_ok(a);
            a.kernel = b16 ? WG_SPLIT : WG_FP32;
            a.pb = (b16 && a.prec >= 2) ? 1 : 2;      // (WgB16Cfg::PB: the split builds stage one patch per group)
            p.lazy_ok = a.prec == 3 && b16 && src_ok;
            // (wgrad_mfma_kernel is built for 3x3 stride 1 / 2 and 1x1)
            p.ok = src_ok && (b16 || (ks == 3 && (stride == 1 || stride == 2)) || (ks == 1 && stride == 1));
            // two resident 4-wave workgroups per CU (MONOCON_HIP_WGRAD_BLOCKS: experiment knob, e.g. 256 = one per CU, which
            // leaves half of every SIMD's registers to whatever the main stream runs beside it)
            budget = env_int("MONOCON_HIP_WGRAD_BLOCKS", 512) * 4 / (p.WN * p.WC);
        }
        a.n_tiles = (a.Cout + 32 * p.WN - 1) / (32 * p.WN);
        a.c_tiles = (a.Cin + 32 * p.WC - 1) / (32 * p.WC);
        wgrad_set_patches(a, a.pb);
        const long long G = (long long)a.B * a.groups_per_img;
        a.ksplit = (int)std::min<long long>(std::max(budget / (a.n_tiles * a.c_tiles), 1), G) * WK;
    }
    if (wgrad_any_lazy(a) && !p.lazy_ok) p.ok = false;
    p.partial_floats = (size_t)a.ksplit * ks * ks * a.Cout * a.Cin;
}

hipError_t launch_wgrad(const WgradPlan &p, float *dw_oihw, hipStream_t st) {
    const WgradArgs &a = p.a;
    if (!p.ok) return hipErrorInvalidValue;
    prof_last = {2, 2.0 * a.B * a.Hout * a.Wout * (double)a.Cout * a.Cin * p.ks * p.ks,
                 4.0 * ((double)a.B * a.Hin * a.Win * a.Cin + (double)a.B * a.Hout * a.Wout * a.Cout + (double)p.ks * p.ks * a.Cin * a.Cout)};
    hipError_t e = hipErrorInvalidValue;
    switch (a.kernel) {
    case WG_FP32: e = launch_wgrad_fp32(p, st); break;
    case WG_SPLIT: e = launch_wgrad_bf16(p, st); break;
    case WG_PIPE: e = launch_wgrad_pipe(p, st); break;
    case WG_SMALL: e = launch_wgrad_small(p, st); break;
    case WG_THIN16: e = launch_wgrad_thin(p, st); break;
    }
    if (e != hipSuccess) return e;
    return launch_splitk_reduce(a.partial, a.ksplit, p.ks * p.ks, a.Cout, a.Cin, dw_oihw, st);
}

}  // namespace mc
