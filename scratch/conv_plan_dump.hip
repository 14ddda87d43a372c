// What the conv planner decides, one line per case: a stand-alone host program (its own main, needs no device, never loaded
// into Python) that links a built libmonocon_hip.so, plans and "launches" forward convs and data gradients, and prints for each
// whether the library refuses the launch or hands it to the runtime, and then WHICH kernel instantiation with which grid, block,
// dynamic LDS and chunks / ppr / ppi in its parameter block, beside the statistics rows per image and the lazy / BM answers.
// No kernel ever runs: this program defines the launch entry points of the HIP runtime itself (hipLaunchKernel & co. below), so
// the library's launches end here and are printed instead -- the kernel by the name of its host stub.
// Cases:
//   * the train plan's forward convs, data-gradient launches (parity classes included) at B = 32, 384x1280 and B = 4, 128x224,
//     the eval plan's convs at B = 8, 384x1280,
//   * CONV_CASES / DGRAD_CASES (tests/test_hip_ops.py) and CONV_EXTRA / DGRAD_EXTRA (tests/test_hip_conv_tilings.py),
//   * `--sweep N` fixed-seed random shapes, ineligible ones included (channels no multiple of 16 / 32, unaligned concat sources,
//     Wout % 16 != 0, missing max-|x| slots or piece panels, strided output, unsupported k / stride),
// each in precision modes 0..3, with no / all / only the first source lazy (and the first lazy without its second coefficient
// table), with the backward-statistics fields off / on, under CFG_AUTO, the tuner's twelve candidates, the retired ids 2 and 3
// and one id with unknown bits.  MONOCON_HIP_WRES is read once per process: run once with it unset and once with =0.
// `--table`: the short matrix kept in profiles/conv_plan_pr.txt (B = 32 train plan, mode 3, three ids, launches that reach a
// kernel only); `--kernels` appends the plan's own record (ConvKernel id and coordinates).  Two builds of the library that print the same lines plan the same launches.  Build lines: scratch/README.md.
// -DCONV_DUMP_OLD_API: the same program against the signatures before the planner owned the choice
// (launch_conv(a, ks, stride, st, resolved), conv_lazy_capable, conv_chunks_per_image).
#include <cxxabi.h>
#include <dlfcn.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "train.h"

using namespace mc;

// ---- the runtime's launch entry points, defined here: the library's calls bind to these
static struct { bool seen; std::string kernel; dim3 grid, block; size_t lds; ConvArgs a; int extra[5]; } g_launch;
static struct { dim3 grid, block; size_t lds; hipStream_t st; } g_cfg;
extern "C" hipError_t __hipPushCallConfiguration(dim3 grid, dim3 block, size_t lds, hipStream_t st) {
    g_cfg.grid = grid; g_cfg.block = block; g_cfg.lds = lds; g_cfg.st = st;
    return hipSuccess;
}
extern "C" hipError_t __hipPopCallConfiguration(dim3 *grid, dim3 *block, size_t *lds, hipStream_t *st) {
    *grid = g_cfg.grid; *block = g_cfg.block; *lds = g_cfg.lds; *st = g_cfg.st;
    return hipSuccess;
}
extern "C" hipError_t hipLaunchKernel(const void *fn, dim3 grid, dim3 block, void **args, size_t lds, hipStream_t) {
    Dl_info info{};
    std::string name = "?";
    if (dladdr(fn, &info) && info.dli_sname) {
        int status = 0;
        char *d = abi::__cxa_demangle(info.dli_sname, nullptr, nullptr, &status);
        name = d ? d : info.dli_sname;
        std::free(d);
        if (name.rfind("void mc::", 0) == 0) name = name.substr(9);       // "void mc::kernel<...>(mc::ConvArgs, ...)" -> "kernel<...>"
        if (name.find('(') != std::string::npos) name = name.substr(0, name.rfind('('));
    }
    g_launch.seen = true; g_launch.kernel = name; g_launch.grid = grid; g_launch.block = block; g_launch.lds = lds;
    g_launch.a = *static_cast<const ConvArgs *>(args[0]);
    const bool wres = name.find("conv_wres_kernel") != std::string::npos;     // (a, tpr, tpi, total, per_wg, ngroups)
    for (int i = 0; i < 5; ++i) g_launch.extra[i] = wres ? *static_cast<const int *>(args[1 + i]) : 0;
    return hipSuccess;
}
extern "C" hipError_t hipFuncSetAttribute(const void *, hipFuncAttribute, int) { return hipSuccess; }
extern "C" hipError_t hipGetLastError(void) { return hipSuccess; }
extern "C" hipError_t hipGetDevice(int *dev) { *dev = 0; return hipSuccess; }
extern "C" hipError_t hipDeviceGetAttribute(int *v, hipDeviceAttribute_t, int) { *v = 256; return hipSuccess; }

struct Case {
    std::string name;
    int B, H, W;               // the input map
    std::vector<int> cins;
    int Cout, ks, stride;      // ks: window code
    bool res = false, stats = false;
    int scatter = 0;           // 1: output (and residual) to every second pixel of a 2H x 2W map (a parity class)
    bool amax = true, panels = true;      // max-|x| slots / 16-bit piece panels present where the mode wants them
    int coutp = 0;             // 0: conv_coutp(Cout)
};

static unsigned g_slot[4];       // stands for every buffer, slot and coefficient table: the planner compares pointers with null only
static bool g_kernels = false, g_table = false;

static int out_dim(int in, int ks, int stride) { return ks >= 10 ? in : conv_out_dim(in, ks, stride); }

static void fill(ConvArgs &a, const Case &c, int prec, int lazy, bool bm, int cfg) {
    const float *f = reinterpret_cast<const float *>(g_slot);
    float *fw = reinterpret_cast<float *>(g_slot);
    a.nsrc = (int)c.cins.size();
    a.Cin = 0;
    for (int i = 0; i < a.nsrc; ++i) {
        const bool lz = lazy == 1 || (lazy >= 2 && i == 0);
        a.src[i] = ConvSrc{f, c.cins[i], lz ? f : nullptr, (lz && !(lazy == 3)) ? f : nullptr};
        a.Cin += c.cins[i];
    }
    a.B = c.B; a.Hin = c.H; a.Win = c.W;
    a.Hout = out_dim(c.H, c.ks, c.stride); a.Wout = out_dim(c.W, c.ks, c.stride);
    a.Cout = c.Cout; a.CoutP = c.coutp ? c.coutp : conv_coutp(c.Cout); a.wpk = f;
    a.wpk16 = (prec >= 1 && c.panels && a.Cin % 8 == 0) ? f : nullptr;
    a.prec = a.wpk16 ? prec : 0;
    if (a.prec == 3 && c.amax) {
        for (int i = 0; i < a.nsrc; ++i) a.amax_in[i] = g_slot;
        a.amax_w = g_slot;
    }
    a.scale = f; a.bias = f; a.out = fw; a.out_ld = c.Cout; a.relu = 1;
    if (c.scatter) { a.o_px = 2 * c.Cout; a.o_row = 2 * (2 * a.Wout) * c.Cout; a.o_img = (2 * a.Hout) * (2 * a.Wout) * c.Cout; }
    if (c.res) { a.res = f; a.res_ld = c.Cout; a.r_px = a.o_px; a.r_row = a.o_row; a.r_img = a.o_img; }
    if (c.stats || bm) a.stats = fw;
    if (bm) { a.bm_y = f; a.bm_a = f; a.bm_b = f; a.bm_relu = 2; a.relu = 0; }
    a.cfg = cfg;
}

static void dump(const Case &c, int prec, int lazy, bool bm, int cfg) {
    int stat_rows;
    bool lazy_ok, bm_ok;
    hipError_t e;
    char extra[96] = "";
    g_launch.seen = false;
#ifdef CONV_DUMP_OLD_API
    ConvArgs a{};
    fill(a, c, prec, lazy, bm, cfg);
    stat_rows = conv_chunks_per_image(a.cfg, a.Hout, a.Wout);
    lazy_ok = conv_lazy_capable(a, c.ks, c.stride);
    e = launch_conv(a, c.ks, c.stride, nullptr);
    // a backward-statistics build of the kernel that ran: conv_thin16 in the row family (emit_dgrad's rule), the tilings for
    // 3x3 / 1x1 at stride 1 (launch_one / launch_b16_one), conv_wres; never with lazy sources
    bm_ok = e == hipSuccess && !conv_any_lazy(a) &&
            (a.cfg == CFG_SMALL ? conv_thin_ok(a, c.ks, c.stride) : (c.stride == 1 && (c.ks == 3 || c.ks == 1)));
#else
    ConvPlan p{};
    fill(p.a, c, prec, lazy, bm, cfg);
    p.ks = c.ks; p.stride = c.stride;
    conv_plan(p);
    stat_rows = p.stat_rows; lazy_ok = p.lazy_ok; bm_ok = p.bm_ok;
    e = launch_conv(p, nullptr);
    static const char *const names[] = {"fp32", "fp32_ws", "split", "wres", "row", "row_lazy", "thin16"};
    if (g_kernels && p.ok)
        std::snprintf(extra, sizeof extra, " plan=%s shape=%d ck=%d spl=%d bm=%d lz=%d row_ok=%d b16=%d", names[p.kernel], p.shape, p.ck, p.spl,
                      (int)p.bm, (int)p.lz, (int)p.row_ok, (int)p.b16);
#endif
    if (g_table && !(e == hipSuccess && g_launch.seen)) return;      // the short matrix: launches that reach a kernel only
    std::printf("%s prec=%d lazy=%d bm=%d cfg=%d: ", c.name.c_str(), prec, lazy, (int)bm, cfg);
    if (e == hipSuccess && g_launch.seen) {
        const auto &L = g_launch;
        std::printf("%s grid=%u block=%u lds=%zu chunks=%d ppr=%d ppi=%d", L.kernel.c_str(), L.grid.x, L.block.x, L.lds, L.a.chunks, L.a.ppr, L.a.ppi);
        if (L.extra[0]) std::printf(" tiles=%d,%d,%d,%d,%d", L.extra[0], L.extra[1], L.extra[2], L.extra[3], L.extra[4]);
        if (!g_table) std::printf(" o=%d,%d,%d r=%d,%d,%d", L.a.o_px, L.a.o_row, L.a.o_img, L.a.r_px, L.a.r_row, L.a.r_img);
    } else {
        std::printf("%s", e == hipErrorInvalidValue ? "refused" : (e == hipSuccess ? "no-launch" : "error"));
    }
    std::printf(" stat_rows=%d lazy_ok=%d bm_ok=%d%s\n", stat_rows, (int)lazy_ok, (int)bm_ok, extra);
}

struct Cases {
    std::vector<Case> v;
    void fwd(const std::string &name, int B, int H, int W, std::vector<int> cins, int Cout, int ks, int stride, bool res, bool stats) {
        Case c{name, B, H, W, std::move(cins), Cout, ks, stride};
        c.res = res; c.stats = stats;
        v.push_back(c);
    }
    // the data gradient of a k x k conv of the given stride towards one source of Cs channels (Hs x Ws): a conv over dY (Cd channels)
    void dgrad(const std::string &name, int B, int Hs, int Ws, int Cs, int Cd, int k, int stride, bool acc) {
        if (stride == 2 && k == 3) {
            static const int code[4] = {1, 12, 21, 22};
            for (int cls = 0; cls < 4; ++cls) {
                Case c{name + "_cls" + std::to_string(cls), B, (Hs + 1) / 2, (Ws + 1) / 2, {Cd}, Cs, code[cls], 1};
                c.scatter = 1; c.res = acc;
                v.push_back(c);
            }
            return;
        }
        Case c{name, B, Hs, Ws, {Cd}, Cs, k, 1};
        c.res = acc;
        v.push_back(c);
    }
};

// every distinct conv of a plan (DLA-34 + DLAUp + the fused head conv) on a B x H x W batch, and for a train plan its data gradients
static void plan_cases(Cases &out, const char *kind, bool train, int B, int H, int W) {
    char tag[48];
    std::snprintf(tag, sizeof tag, "%s_b%d_%dx%d", kind, B, H, W);
    auto add = [&](const std::string &what, int level, std::vector<int> cins, int Cout, int ks, int stride, bool res = false) {
        const int h = H >> level, w = W >> level;
        out.fwd(std::string(tag) + "_" + what, B, h, w, cins, Cout, ks, stride, res, train);
        if (!train) return;
        for (size_t i = 0; i < cins.size(); ++i) {
            if (i > 0 && cins[i] == cins[0]) continue;      // (sources of one width plan alike)
            const std::string n = std::string(tag) + "_dg_" + what + "_src" + std::to_string(i);
            out.dgrad(n, B, h, w, cins[i], Cout, ks, stride, false);
            if (stride == 1) out.dgrad(n + "_acc", B, h, w, cins[i], Cout, ks, stride, true);
        }
    };
    add("level0", 0, {16}, 16, 3, 1);
    add("level1", 0, {16}, 32, 3, 2);
    const int ch[6] = {16, 32, 64, 128, 256, 512};
    for (int lv = 2; lv <= 5; ++lv) {          // a level's input lies at level lv - 1, its maps at lv
        const int ci = ch[lv - 1], co = ch[lv];
        const std::string l = "level" + std::to_string(lv);
        add(l + "_down", lv - 1, {ci}, co, 3, 2);
        add(l + "_block", lv, {co}, co, 3, 1);
        add(l + "_block_res", lv, {co}, co, 3, 1, true);
        add(l + "_project", lv, {ci}, co, 1, 1);
        add(l + "_root", lv, lv == 5 ? std::vector<int>{co, co, ci} : std::vector<int>{co, co}, co, 1, 1);
        if (lv == 3 || lv == 4) add(l + "_root4", lv, {co, co, ci, co}, co, 1, 1);
    }
    for (int lv = 5; lv >= 3; --lv) {          // DLAUp: proj at the coarse level, node on the concat one level finer
        const int co = ch[lv - 1];
        add("ida_proj_" + std::to_string(ch[lv]) + "_" + std::to_string(co), lv, {ch[lv]}, co, 3, 1);
        add("ida_node_" + std::to_string(co), lv - 1, {co, co}, co, 3, 1);
    }
    add("heads_64_576", 2, {64}, 576, 3, 1);
}

static void test_cases(Cases &out) {
    struct F { const char *n; int B, H, W; std::vector<int> cins; int Cout, k, s; bool res; };
    const F f[] = {
        {"s1_64_64", 2, 16, 24, {64}, 64, 3, 1, true}, {"s1_128_128_t128", 1, 12, 40, {128}, 128, 3, 1, true},
        {"s1_16_16_t32", 1, 20, 24, {16}, 16, 3, 1, false}, {"s1_cat_64_64_to64", 2, 8, 16, {64, 64}, 64, 3, 1, false},
        {"s1_odd_edges", 1, 6, 10, {32}, 64, 3, 1, false}, {"s1_tiny_2x4", 2, 2, 4, {256}, 512, 3, 1, true},
        {"s2_32_64", 2, 16, 32, {32}, 64, 3, 2, false}, {"s2_16_32", 1, 24, 16, {16}, 32, 3, 2, false},
        {"s2_256_512", 1, 8, 8, {256}, 512, 3, 2, false}, {"k1_root4", 1, 12, 16, {128, 128, 64, 128}, 128, 1, 1, false},
        {"k1_project", 2, 8, 8, {32}, 64, 1, 1, false}, {"k1_root3_512", 1, 4, 8, {512, 512, 256}, 512, 1, 1, false},
        {"head_576", 1, 8, 16, {64}, 576, 3, 1, false},
        {"s1_9x17_rem1", 2, 9, 17, {64}, 64, 3, 1, true}, {"s1_7x20_rem2", 2, 7, 20, {32}, 128, 3, 1, false},
        {"s1_3x50_rem3_c48", 2, 3, 50, {48}, 64, 3, 1, true}, {"s1_c16_to64", 1, 8, 24, {16}, 64, 3, 1, false},
        {"s2_odd_13x35", 2, 13, 35, {32}, 64, 3, 2, false}, {"s2_64_128", 2, 12, 20, {64}, 128, 3, 2, true},
        {"s2_c16_to64", 2, 10, 12, {16}, 64, 3, 2, false}, {"k1_c16_c48_to128", 2, 5, 12, {16, 48}, 128, 1, 1, false},
        {"head_576_b2_rem2", 2, 7, 20, {64}, 576, 3, 1, false}};
    for (const F &c : f) out.fwd(c.n, c.B, c.H, c.W, c.cins, c.Cout, c.k, c.s, c.res, false);
    struct D { const char *n; int B, H, W, Cs, Cout, k, s; };
    const D d[] = {
        {"dg_s1_64_64", 2, 16, 24, 64, 64, 3, 1}, {"dg_s1_128_128", 1, 12, 40, 128, 128, 3, 1}, {"dg_s1_source_slice", 2, 8, 16, 64, 64, 3, 1},
        {"dg_s1_odd_edges", 1, 6, 10, 32, 64, 3, 1}, {"dg_k1_root_slice", 1, 12, 16, 64, 128, 1, 1}, {"dg_s2_32_64", 2, 16, 32, 32, 64, 3, 2},
        {"dg_s2_64_128", 1, 24, 48, 64, 128, 3, 2}, {"dg_s2_16_32", 1, 24, 32, 16, 32, 3, 2}, {"dg_s2_256_512_tiny", 1, 8, 8, 256, 512, 3, 2},
        {"dg_head_576_64", 1, 8, 16, 64, 576, 3, 1}, {"dg_s1_16_16", 1, 6, 32, 16, 16, 3, 1},
        {"dg_s1_9x17_rem1", 2, 9, 17, 64, 64, 3, 1}, {"dg_s1_7x20_rem2", 2, 7, 20, 128, 32, 3, 1}, {"dg_s1_3x50_rem3_dy48", 2, 3, 50, 64, 48, 3, 1},
        {"dg_s1_dy16_2x4", 2, 2, 4, 64, 16, 3, 1}, {"dg_s2_14x36_32_64", 2, 14, 36, 32, 64, 3, 2}, {"dg_s2_14x36_64_128", 2, 14, 36, 64, 128, 3, 2},
        {"dg_s2_128_256", 2, 12, 20, 128, 256, 3, 2}, {"dg_k1_slice_128", 2, 5, 12, 128, 64, 1, 1}};
    for (const D &c : d) {
        out.dgrad(c.n, c.B, c.H, c.W, c.Cs, c.Cout, c.k, c.s, false);
        out.dgrad(std::string(c.n) + "_acc", c.B, c.H, c.W, c.Cs, c.Cout, c.k, c.s, true);
    }
}

static void random_cases(Cases &out, int n) {
    unsigned long long s = 0x9e3779b97f4a7c15ull;       // fixed seed
    auto rnd = [&](int m) { s = s * 6364136223846793005ull + 1442695040888963407ull; return (int)((s >> 33) % (unsigned)m); };
    const int cs[] = {4, 8, 12, 16, 16, 16, 20, 32, 32, 32, 48, 64, 64, 64, 96, 128, 128, 192, 256, 512};
    const int ns[] = {4, 8, 16, 16, 16, 32, 32, 32, 48, 64, 64, 96, 128, 128, 192, 256, 512, 576};
    const int codes[] = {3, 3, 3, 3, 1, 1, 12, 21, 22, 5, 2, 11};
    for (int i = 0; i < n; ++i) {
        Case c;
        c.name = "rand" + std::to_string(i);
        c.B = 1 + rnd(4);
        const int nsrc = rnd(3) ? 1 : 2 + rnd(3);
        for (int k = 0; k < nsrc; ++k) c.cins.push_back(cs[rnd(sizeof cs / sizeof *cs)]);
        c.Cout = ns[rnd(sizeof ns / sizeof *ns)];
        c.ks = codes[rnd(sizeof codes / sizeof *codes)];
        c.stride = rnd(12) ? 1 + (rnd(3) == 0) : 3;
        c.H = rnd(4) ? 1 + rnd(48) : 32 + 32 * rnd(8);
        c.W = rnd(3) ? 1 + rnd(80) : 32 + 16 * rnd(24);
        c.res = rnd(3) == 0; c.stats = rnd(3) == 0;
        c.scatter = rnd(6) == 0;
        c.amax = rnd(10) != 0; c.panels = rnd(10) != 0;
        if (rnd(12) == 0) c.coutp = c.Cout + 32 * rnd(3);       // a padding that is not the layer table's
        out.v.push_back(c);
    }
}

int main(int argc, char **argv) {
    int sweep = 0;
    bool table = false;
    for (int i = 1; i < argc; ++i) {
        if (!std::strcmp(argv[i], "--sweep") && i + 1 < argc) sweep = std::atoi(argv[++i]);
        else if (!std::strcmp(argv[i], "--kernels")) g_kernels = true;
        else if (!std::strcmp(argv[i], "--table")) table = g_table = true;
        else { std::fprintf(stderr, "usage: %s [--sweep N] [--table] [--kernels]\n", argv[0]); return 2; }
    }
    const char *wres = std::getenv("MONOCON_HIP_WRES");
    std::printf("# MONOCON_HIP_WRES=%s\n", wres ? wres : "(unset)");
    Cases cases;
    plan_cases(cases, "train", true, 32, 384, 1280);
    if (!table) {
        plan_cases(cases, "train", true, 4, 128, 224);
        plan_cases(cases, "eval", false, 8, 384, 1280);
        test_cases(cases);
        random_cases(cases, sweep);
    }
    static const int ids[] = {CFG_AUTO, CFG_128x128, CFG_128x64, CFG_128x64m, CFG_128x32, CFG_64x128, CFG_64x64,
                              CFG_WS | CFG_128x128, CFG_WS | CFG_128x64m, CFG_WS | CFG_64x128, CFG_WS | CFG_64x64, CFG_SMALL,
                              CFG_WRES | CFG_128x64, 2, 3, 128 | CFG_128x128};
    static const int table_ids[] = {CFG_AUTO, CFG_SMALL, CFG_WRES | CFG_128x64};
    for (const Case &c : cases.v) {
        if (table && (c.res || c.name.find("_src1") != std::string::npos)) continue;      // (the residual / accumulating twin and a second source plan alike)
        for (int prec = table ? 3 : 0; prec < 4; ++prec)
            for (int lazy = 0; lazy < (table ? 2 : 4); ++lazy)
                for (int bm = 0; bm < 2; ++bm) {
                    if (table && lazy && bm) continue;
                    if (table) { for (int id : table_ids) dump(c, prec, lazy, bm != 0, id); }
                    else { for (int id : ids) dump(c, prec, lazy, bm != 0, id); }
                }
    }
    return 0;
}
