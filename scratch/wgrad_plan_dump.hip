// What the weight-gradient planner decides, one line per case: a stand-alone host program (its own main, needs no device,
// never loaded into Python) that links a built libmonocon_hip.so and calls wgrad_plan / wgrad_lazy_capable /
// wgrad_partial_floats / launch_wgrad over
//   * every distinct conv of the train plan at B = 32, 384x1280 and at B = 4, 128x224,
//   * WGRAD_CASES (tests/test_hip_ops.py), WG_CASES and the stride-2 cases (tests/test_hip_bf16.py),
//   * `--sweep N` fixed-seed random shapes, ineligible ones included (C % 4 != 0, unaligned concat sources, Wout % 4 != 0,
//     maps with fewer pixel groups than workgroups, odd dy_ld, unsupported k / stride, missing max-|x| slots),
// each in precision modes 0..3, with no / all / only the first source lazy, and (`--env`) under every setting of the three
// MONOCON_HIP_WGRAD_* knobs.  `--kernels` appends the chosen kernel id and wave grid: the table of what runs where.
// Two builds of the library that print the same lines plan the same launches.  Build lines: scratch/README.md.
// -DWGRAD_DUMP_OLD_API: the same program against the signatures before the planner owned the choice (wgrad_plan(a, ks, stride)).
//
// launch=: launch_wgrad is called with null buffers -- ONLY when the process sees no device -- to tell the launches the
// library refuses up front (hipErrorInvalidValue, "invalid") from those it hands to the runtime ("ok").
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "train.h"

using namespace mc;

struct Case { std::string name; int B, H, W; std::vector<int> cins; int Cout, ks, stride, dy_ld = 0; bool amax = true; };

static unsigned g_slot[4];       // stands for every max-|x| slot / coefficient table: the planner compares pointers with null only
static bool g_probe = false, g_kernels = false;

static void fill(WgradArgs &a, const Case &c, int prec, int lazy) {
    a.nsrc = (int)c.cins.size();
    a.Cin = 0;
    const float *f = reinterpret_cast<const float *>(g_slot);
    for (int i = 0; i < a.nsrc; ++i) {
        const bool lz = lazy == 1 || (lazy == 2 && i == 0);
        a.src[i] = ConvSrc{f, c.cins[i], lz ? f : nullptr, lz ? f : nullptr};
        a.amax_x[i] = (prec == 3 && c.amax) ? g_slot : nullptr;
        a.Cin += c.cins[i];
    }
    a.amax_dy = (prec == 3 && c.amax) ? g_slot : nullptr;
    a.B = c.B; a.Hin = c.H; a.Win = c.W;
    a.Hout = conv_out_dim(c.H, c.ks, c.stride); a.Wout = conv_out_dim(c.W, c.ks, c.stride);
    a.Cout = c.Cout; a.dy = f; a.dy_ld = c.dy_ld ? c.dy_ld : c.Cout;
    a.prec = prec;
}

static void dump(const Case &c, int prec, int lazy) {
    size_t partial;
    bool lazy_ok;
    int small, pipe, bf16;
    hipError_t e = hipSuccess;
    char extra[64] = "";
#ifdef WGRAD_DUMP_OLD_API
    WgradArgs a{};
    fill(a, c, prec, lazy);
    wgrad_plan(a, c.ks, c.stride);
    partial = wgrad_partial_floats(a, c.ks);
    lazy_ok = wgrad_lazy_capable(a, c.ks, c.stride);
    small = a.small; pipe = a.pipe;
    bf16 = !a.small && !a.pipe && a.prec >= 1 && wgrad_bf16_ok(a, c.ks, c.stride);      // (launch_wgrad's own condition)
    if (g_probe) e = launch_wgrad(a, c.ks, c.stride, nullptr, 0);
#else
    WgradPlan p{};
    fill(p.a, c, prec, lazy);
    p.ks = c.ks; p.stride = c.stride;
    wgrad_plan(p);
    const WgradArgs &a = p.a;
    partial = wgrad_partial_floats(p);
    lazy_ok = wgrad_lazy_capable(p);
    small = a.kernel == WG_SMALL || a.kernel == WG_THIN16; pipe = a.pipe; bf16 = a.kernel == WG_SPLIT;
    if (g_probe) e = launch_wgrad(p, nullptr, 0);
    static const char *const names[] = {"fp32", "split", "pipe", "small", "thin16"};
    if (g_kernels) std::snprintf(extra, sizeof extra, " kernel=%s waves=%dx%d", names[a.kernel], p.WN, p.WC);
#endif
    std::printf("%s prec=%d lazy=%d ksplit=%d n_tiles=%d c_tiles=%d pb=%d ppr=%d ppi=%d groups_per_img=%d partial=%zu lazy_ok=%d "
                "small=%d pipe=%d bf16=%d launch=%s%s\n",
                c.name.c_str(), prec, lazy, a.ksplit, a.n_tiles, a.c_tiles, a.pb, a.ppr, a.ppi, a.groups_per_img, partial, (int)lazy_ok,
                small, pipe, bf16, !g_probe ? "-" : (e == hipErrorInvalidValue ? "invalid" : "ok"), extra);
}

// every distinct weight-gradient launch of the train plan (DLA-34 + DLAUp + the fused head conv) on a B x H x W batch
static void train_plan_cases(std::vector<Case> &out, int B, int H, int W) {
    char tag[32];
    std::snprintf(tag, sizeof tag, "plan_b%d_%dx%d", B, H, W);
    auto add = [&](const char *what, int level, std::vector<int> cins, int Cout, int ks, int stride, int dy_ld = 0) {
        out.push_back({std::string(tag) + "_" + what, B, H >> level, W >> level, std::move(cins), Cout, ks, stride, dy_ld});
    };
    add("level0", 0, {16}, 16, 3, 1);
    add("level1", 0, {16}, 32, 3, 2);
    const int ch[6] = {16, 32, 64, 128, 256, 512};
    for (int lv = 2; lv <= 5; ++lv) {          // a level's input lies at level lv - 1, its maps at lv
        const int ci = ch[lv - 1], co = ch[lv];
        const std::string l = "level" + std::to_string(lv);
        add((l + "_down").c_str(), lv - 1, {ci}, co, 3, 2);
        add((l + "_block").c_str(), lv, {co}, co, 3, 1);
        add((l + "_project").c_str(), lv, {ci}, co, 1, 1);
        add((l + "_root").c_str(), lv, lv == 5 ? std::vector<int>{co, co, ci} : std::vector<int>{co, co}, co, 1, 1);
        if (lv == 3 || lv == 4) add((l + "_root4").c_str(), lv, {co, co, ci, co}, co, 1, 1);
    }
    for (int lv = 5; lv >= 3; --lv) {          // DLAUp: proj at the coarse level, node on the concat one level finer
        const int co = ch[lv - 1];
        add(("ida_proj_" + std::to_string(ch[lv]) + "_" + std::to_string(co)).c_str(), lv, {ch[lv]}, co, 3, 1);
        add(("ida_node_" + std::to_string(co)).c_str(), lv - 1, {co, co}, co, 3, 1);
    }
    add("heads_64_576", 2, {64}, 576, 3, 1, 576);
}

static void test_cases(std::vector<Case> &out) {
    out.insert(out.end(), {
        {"wg_s1_64_64", 2, 16, 24, {64}, 64, 3, 1}, {"wg_s1_128_128", 2, 12, 40, {128}, 128, 3, 1},
        {"wg_s1_cat_64_64_to64", 2, 8, 16, {64, 64}, 64, 3, 1}, {"wg_s1_16_16", 1, 20, 24, {16}, 16, 3, 1},
        {"wg_s1_odd", 1, 6, 10, {32}, 64, 3, 1}, {"wg_s2_32_64", 2, 16, 32, {32}, 64, 3, 2}, {"wg_s2_16_32", 1, 24, 16, {16}, 32, 3, 2},
        {"wg_s2_256_512", 1, 8, 8, {256}, 512, 3, 2}, {"wg_k1_root4", 1, 12, 16, {128, 128, 64, 128}, 128, 1, 1},
        {"wg_k1_32_64", 2, 8, 8, {32}, 64, 1, 1}, {"wg_head_64_576", 1, 8, 16, {64}, 576, 3, 1},
        {"wg_s2_128_256_24x48", 2, 24, 48, {128}, 256, 3, 2}, {"wg_s1_256_256_12x24", 2, 12, 24, {256}, 256, 3, 1},
        {"wg_s2_64_128_48x96", 2, 48, 96, {64}, 128, 3, 2},
        {"b16wg_64_64", 2, 16, 24, {64}, 64, 3, 1}, {"b16wg_128_128", 2, 12, 40, {128}, 128, 3, 1},
        {"b16wg_cat_64_64", 2, 8, 16, {64, 64}, 64, 3, 1}, {"b16wg_odd_edges", 1, 6, 10, {32}, 64, 3, 1},
        {"b16wg_head_64_576", 1, 8, 16, {64}, 576, 3, 1}, {"b16wg_k1_root4", 1, 12, 16, {128, 128, 64, 128}, 128, 1, 1},
        {"b16wg_k1_32_64", 2, 8, 8, {32}, 64, 1, 1}, {"b16wg_256_256_12x24", 2, 12, 24, {256}, 256, 3, 1},
        {"b16wg_128_64", 1, 8, 16, {128}, 64, 3, 1}, {"b16wg_odd_64_128", 1, 6, 10, {64}, 128, 3, 1},
        {"b16wg_cat_64_64_128", 1, 10, 20, {64, 64}, 128, 3, 1},
        {"s2_32_64", 2, 16, 32, {32}, 64, 3, 2}, {"s2_64_128", 1, 24, 48, {64}, 128, 3, 2}, {"s2_128_256", 2, 8, 16, {128}, 256, 3, 2},
        {"s2_ragged_patches", 1, 10, 24, {64}, 64, 3, 2}, {"s2_256_512", 1, 12, 40, {256}, 512, 3, 2},
        {"s2_two_sources", 1, 16, 16, {32, 32}, 64, 3, 2}});
}

static void random_cases(std::vector<Case> &out, int n) {
    unsigned long long s = 0x9e3779b97f4a7c15ull;       // fixed seed
    auto rnd = [&](int m) { s = s * 6364136223846793005ull + 1442695040888963407ull; return (int)((s >> 33) % (unsigned)m); };
    const int cs[] = {4, 6, 8, 12, 16, 16, 20, 32, 32, 48, 64, 64, 64, 96, 128, 128, 192, 256, 512};
    const int ns[] = {4, 8, 12, 16, 16, 32, 32, 48, 64, 64, 96, 128, 128, 192, 256, 512, 576};
    for (int i = 0; i < n; ++i) {
        Case c;
        c.name = "rand" + std::to_string(i);
        c.B = 1 + rnd(4);
        const int nsrc = rnd(3) ? 1 : 2 + rnd(3);
        for (int k = 0; k < nsrc; ++k) c.cins.push_back(cs[rnd(sizeof cs / sizeof *cs)]);
        c.Cout = ns[rnd(sizeof ns / sizeof *ns)];
        c.ks = rnd(16) ? (rnd(3) ? 3 : 1) : 5;
        c.stride = rnd(16) ? 1 + rnd(2) : 3;
        c.H = rnd(4) ? 1 + rnd(48) : 64 + 32 * rnd(8);
        c.W = rnd(4) ? 1 + rnd(64) : 64 + 32 * rnd(16);
        c.dy_ld = rnd(6) ? 0 : c.Cout + (rnd(2) ? 2 : 4 * (1 + rnd(8)));
        c.amax = rnd(10) != 0;
        out.push_back(c);
    }
}

int main(int argc, char **argv) {
    int sweep = 0;
    bool env = false;
    for (int i = 1; i < argc; ++i) {
        if (!std::strcmp(argv[i], "--sweep") && i + 1 < argc) sweep = std::atoi(argv[++i]);
        else if (!std::strcmp(argv[i], "--env")) env = true;
        else if (!std::strcmp(argv[i], "--kernels")) g_kernels = true;
        else { std::fprintf(stderr, "usage: %s [--sweep N] [--env] [--kernels]\n", argv[0]); return 2; }
    }
    int ndev = 0;
    g_probe = hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0;      // null buffers: never where a kernel could run
    std::vector<Case> cases;
    train_plan_cases(cases, 32, 384, 1280);
    train_plan_cases(cases, 4, 128, 224);
    test_cases(cases);
    random_cases(cases, sweep);
    const char *const pipe[] = {nullptr, "0", "1", "2", "3"}, *const pblocks[] = {nullptr, "1", "7"}, *const blocks[] = {nullptr, "256", "1024"};
    auto set = [](const char *k, const char *v) { v ? setenv(k, v, 1) : unsetenv(k); };
    for (int ip = 0; ip < (env ? 5 : 1); ++ip)
        for (int ib = 0; ib < (env ? 3 : 1); ++ib)
            for (int ik = 0; ik < (env ? 3 : 1); ++ik) {
                set("MONOCON_HIP_WGRAD_PIPE", pipe[ip]);
                set("MONOCON_HIP_WGRAD_PIPE_BLOCKS", pblocks[ib]);
                set("MONOCON_HIP_WGRAD_BLOCKS", blocks[ik]);
                std::printf("# MONOCON_HIP_WGRAD_PIPE=%s MONOCON_HIP_WGRAD_PIPE_BLOCKS=%s MONOCON_HIP_WGRAD_BLOCKS=%s\n",
                            pipe[ip] ? pipe[ip] : "(unset)", pblocks[ib] ? pblocks[ib] : "(unset)", blocks[ik] ? blocks[ik] : "(unset)");
                for (const Case &c : cases)
                    for (int prec = 0; prec < 4; ++prec)
                        for (int lazy = 0; lazy < 3; ++lazy) dump(c, prec, lazy);
            }
    return 0;
}
