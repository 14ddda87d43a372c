// C-ABI of libmonocon_hip.so (include/monocon_hip.h): handle, parameter binding/packing, the
// DLA-34 -> DLAUp -> dense-head launch plan, decode and the op-level test entry points.
//
// The network is described once per handle as a table of layers keyed by the reference's
// state_dict names; a launch plan (list of fully-resolved kernel launches + handle-owned NHWC
// activation buffers) is built per input shape and replayed on the caller's stream.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <map>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/monocon_hip.h"
#include "conv_mfma.h"
#include "kernels.h"

#include <cstdint>
#include "mc_internal.h"

std::string g_create_err;

// ------------------------------------------------------------------------------ allocation
float *PlanAlloc::alloc(size_t nfloats) {
    const size_t bytes = (nfloats ? nfloats : empty_floats) * sizeof(float);
    if (h->dry_alloc) {                       // mc_query_workspace: count only
        h->dry_next += (bytes + 255) / 256 * 256;
        m.bytes += bytes;
        return reinterpret_cast<float *>((uintptr_t)0x100000 + h->dry_next);
    }
    void *q = nullptr;
    hipError_t e = hipMalloc(&q, bytes);
    if (e == hipSuccess) {
        m.bufs.push_back(q);
        e = hipMemset(q, 0, bytes);
    }
    if (e != hipSuccess) {
        ok = false;
        fail(h, "plan: %zu bytes of device memory: %s", bytes, hipGetErrorString(e));
        return nullptr;
    }
    m.bytes += bytes;
    return static_cast<float *>(q);
}

unsigned *PlanAlloc::slot() {
    if (h->prec != 3) return nullptr;
    if (!m.amax_arena) m.amax_arena = reinterpret_cast<unsigned *>(alloc((size_t)amax_slots * AMAX_WORDS));
    if (m.amax_used >= amax_slots) { ok = false; h->err = "plan: amax slot table overflow"; return nullptr; }
    return m.amax_arena ? m.amax_arena + (size_t)(m.amax_used++) * AMAX_WORDS : nullptr;
}

void *mc_param(mc_handle *h, const std::string &name, int64_t numel, int dtype) {
    auto it = h->bound.find(name);
    if (it == h->bound.end()) { fail(h, "parameter not bound: %s", name.c_str()); return nullptr; }
    const Bound &b = it->second;
    if (b.dtype != dtype) {
        fail(h, "parameter is not %s: %s", dtype == MC_I64 ? "int64" : "fp32", name.c_str());
        return nullptr;
    }
    if (b.numel != numel) {
        fail(h, "parameter has wrong size: %s (%lld elements bound, %lld expected)", name.c_str(), (long long)b.numel,
             (long long)numel);
        return nullptr;
    }
    return b.ptr;
}

ConvLayer &mc_conv_layer(mc_handle *h, const std::string &name, bool &ok) {
    auto it = h->convs.find(name);
    if (it == h->convs.end()) { ok = false; h->err = "no layer " + name; static ConvLayer d; return d; }
    return it->second;
}

int mc_head_conv_args(mc_handle *h, PlanAlloc &mem, const Tensor &feat, float *hidden, ConvPlan &p) {
    const ConvLayer &L = h->head3;
    ConvArgs &a = p.a;
    a.bias = h->head_bias;
    a.out = hidden; a.out_ld = L.cout;
    a.cfg = L.cfg;
    a.stat_shift = h->head_rm;
    conv_fwd_args(p, L, {&feat}, h->prec);
    const int chunks = p.stat_rows;
    a.stats = mem.alloc((size_t)a.B * chunks * L.coutp * 2);
    conv_plan(p);
    return chunks;
}

// ------------------------------------------------------------------------------ network graph
namespace {
struct GraphBuilder {
    NetGraph g;
    std::map<int, int> pooled;   // node -> its 2x2 max-pool (a nested tree pools its input again)

    int node(int C) {
        g.node_c.push_back(C);
        return (int)g.node_c.size() - 1;
    }
    int push(NetStep s, int C) {
        s.out = s.dead ? -1 : node(C);
        g.steps.push_back(std::move(s));
        return g.steps.back().out;
    }
    int conv(const std::string &n, const std::string &bn, std::vector<int> srcs, int res, bool relu, int cout, int ks,
             int stride, bool dead = false) {
        NetStep s{STEP_CONV, n, bn, std::move(srcs)};
        s.res = res; s.relu = relu; s.cout = cout; s.ks = ks; s.stride = stride; s.dead = dead;
        return push(std::move(s), cout);
    }
    int pool(int x) {
        auto it = pooled.find(x);
        if (it != pooled.end()) return it->second;
        return pooled[x] = push(NetStep{STEP_POOL, "", "", {x}}, g.node_c[x]);
    }
    int deconv(const std::string &n, int x) { return push(NetStep{STEP_DECONV, n, "", {x}}, g.node_c[x]); }

    // reference model/backbone/dla.py:34-51
    int block(const std::string &n, int x, int residual, int cout, int stride) {
        const int y = conv(n + ".conv1", n + ".bn1", {x}, -1, true, cout, 3, stride);
        return conv(n + ".conv2", n + ".bn2", {y}, residual, true, cout, 3, 1);
    }
    // reference model/backbone/dla.py:187-205
    int tree(const std::string &n, int levels, int cout, int stride, bool level_root, int x, std::vector<int> children) {
        const int cin = g.node_c[x];
        const int bottom = stride > 1 ? pool(x) : x;
        if (level_root) children.push_back(bottom);
        if (levels == 1) {
            const int residual = cin != cout ? conv(n + ".project.0", n + ".project.1", {bottom}, -1, false, cout, 1, 1) : bottom;
            const int x1 = block(n + ".tree1", x, residual, cout, stride);
            const int x2 = block(n + ".tree2", x1, x1, cout, 1);
            std::vector<int> cat = {x2, x1};
            cat.insert(cat.end(), children.begin(), children.end());
            return conv(n + ".root.conv", n + ".root.bn", cat, -1, true, cout, 1, 1);
        }
        // the outer `project` of a two-level tree is dead: the nested tree recomputes its own residual (dla.py:193-194)
        if (cin != cout) conv(n + ".project.0", n + ".project.1", {bottom}, -1, false, cout, 1, 1, /*dead=*/true);
        const int x1 = tree(n + ".tree1", levels - 1, cout, stride, false, x, {});
        children.push_back(x1);
        return tree(n + ".tree2", levels - 1, cout, 1, false, x1, children);
    }
};
}  // namespace

static NetGraph build_net() {
    GraphBuilder b;
    int *lv = b.g.lv;
    b.node(16);                               // node 0: the stem's output (reference dla.py:231-234)
    lv[0] = b.conv("backbone.level0.0", "backbone.level0.1", {0}, -1, true, 16, 3, 1);
    lv[1] = b.conv("backbone.level1.0", "backbone.level1.1", {lv[0]}, -1, true, 32, 3, 2);
    lv[2] = b.tree("backbone.level2", 1, 64, 2, false, lv[1], {});
    lv[3] = b.tree("backbone.level3", 2, 128, 2, true, lv[2], {});
    lv[4] = b.tree("backbone.level4", 2, 256, 2, true, lv[3], {});
    lv[5] = b.tree("backbone.level5", 1, 512, 2, true, lv[4], {});
    b.g.n_backbone = (int)b.g.steps.size();
    // DLAUp (reference dla_neck.py:94-106,136-143): layers = [l2, l3, l4, l5]
    int layers[4] = {lv[2], lv[3], lv[4], lv[5]};
    for (int i = 0; i < 3; ++i) {
        const int j = 4 - i - 2;              // first level of this IDA
        const int out = b.g.node_c[layers[j]];
        const std::string pre = "neck.ida_" + std::to_string(i) + ".";
        for (int t = 1; t < 4 - j; ++t) {
            const std::string ts = std::to_string(t);
            const int p = b.conv(pre + "proj_" + ts + ".conv", pre + "proj_" + ts + ".bn1", {layers[j + t]}, -1, true, out, 3, 1);
            b.g.steps.back().elementwise_consumers = true;
            const int u = b.deconv(pre + "up_" + ts, p);
            layers[j + t] = b.conv(pre + "node_" + ts + ".conv", pre + "node_" + ts + ".bn1", {layers[j + t - 1], u}, -1, true,
                                   out, 3, 1);
        }
    }
    b.g.feat = layers[3];
    // `feat` feeds the fused head conv and its weight gradient, the two longest launches of the train step (mc_train_plan.hip)
    b.g.steps.back().never_lazy = true;
    return b.g;
}

// ------------------------------------------------------------------------------ layer table
static int build_layers(mc_handle *h) {
    if (h->layers_built) return 0;
    h->net = build_net();
    for (const NetStep &s : h->net.steps) {
        if (s.kind == STEP_CONV) {
            ConvLayer L;
            L.conv = s.name; L.bn = s.bn; L.cout = s.cout; L.ks = s.ks; L.stride = s.stride;
            for (int x : s.srcs) L.cin += h->net.node_c[x];
            L.coutp = conv_coutp(L.cout);
            h->convs[s.name] = L;
        } else if (s.kind == STEP_DECONV) {
            DeconvLayer D;
            D.name = s.name;
            D.C = h->net.node_c[s.srcs[0]];
            h->deconvs[D.name] = D;
        }
    }
    bool ok = true;
    PlanAlloc mem{h, h->params, ok, 4, 0};
    for (auto &kv : h->convs) {
        ConvLayer &L = kv.second;
        const size_t wn = (size_t)L.ks * L.ks * L.cin * L.coutp;
        L.wpk = mem.alloc(wn);
        L.wpk16 = mem.alloc((3 * wn + 1) / 2);   // up to 3 bf16 pieces
        L.scale = mem.alloc(L.cout);
        L.shift = mem.alloc(L.cout);
    }
    for (auto &kv : h->deconvs) kv.second.wpk = mem.alloc((size_t)16 * kv.second.C);
    h->stem_w = mem.alloc(147 * 16);
    h->stem_scale = mem.alloc(16);
    h->stem_shift = mem.alloc(16);
    ConvLayer &H3 = h->head3;
    H3.conv = "head.*.0"; H3.ks = 3; H3.stride = 1; H3.cin = 64; H3.cout = NUM_HEADS * HEAD_CH;
    H3.cfg = CFG_128x64m | CFG_WRES;      // one head per 64-column tile (weight-resident kernel where the launch is eligible)
    H3.coutp = H3.cout;
    H3.wpk = mem.alloc((size_t)9 * 64 * H3.coutp);
    H3.wpk16 = mem.alloc((size_t)3 * 9 * 64 * H3.coutp / 2);
    h->head_bias = mem.alloc(H3.cout);
    h->head_rm = mem.alloc(H3.cout);
    h->att_scale = mem.alloc(NUM_HEADS * NUM_AFFINE);
    h->att_shift = mem.alloc(NUM_HEADS * NUM_AFFINE);
    h->head_w1 = mem.alloc(NUM_OUT_ROWS * HEAD_CH);
    h->head_w1t = mem.alloc(NUM_OUT_ROWS * HEAD_CH);
    h->head_b1 = mem.alloc(NUM_OUT_ROWS);
    // precision mode 3: one max-|w| slot per conv layer + one for the fused head panel
    h->w_amax_n = (int)h->convs.size() + 1;
    h->w_amax_arena = reinterpret_cast<unsigned *>(mem.alloc((size_t)h->w_amax_n));
    if (!ok) return -1;
    int i = 0;
    for (auto &kv : h->convs) kv.second.w_amax = h->w_amax_arena + i++;
    H3.w_amax = h->w_amax_arena + i;
    HIPCHK(h, hipDeviceSynchronize());   // zero-fills above ran on the null stream
    h->layers_built = true;
    return 0;
}

// ------------------------------------------------------------------------------ plan builder
namespace {
struct Builder {
    mc_handle *h;
    Plan *pl;
    bool ok = true;
    PlanAlloc mem{h, pl->mem, ok, 4, 256};

    Tensor alloc(int B, int H, int W, int C) {
        Tensor t;
        t.B = B; t.H = H; t.W = W; t.C = C;
        t.p = mem.alloc(t.numel());
        t.amax = mem.slot();       // mode 3: max |x| of the tensor (operand scale of the convs that read it)
        return t;
    }

    // a conv launch whose arguments op.cp holds, planned once more here (its id and epilogue are set), with its algorithmic cost
    void push_conv(Op &op) {
        conv_plan(op.cp);
        const ConvArgs &a = op.cp.a;
        op.kind = OP_CONV;
        const double out_elems = (double)a.B * a.Hout * a.Wout * a.Cout;
        op.flops = 2.0 * out_elems * a.Cin * op.cp.ks * op.cp.ks;
        op.bytes = 4.0 * ((double)a.B * a.Hin * a.Win * a.Cin + out_elems * (a.res ? 2 : 1));
        pl->ops.push_back(op);
    }

    Tensor conv(const ConvLayer &L, const std::vector<const Tensor *> &srcs, const Tensor *res, bool relu) {
        Op op{};
        ConvArgs &a = op.cp.a;
        if (!conv_fwd_args(op.cp, L, srcs, h->prec)) { ok = false; h->err = "channel mismatch at " + L.conv; }
        Tensor out = alloc(a.B, a.Hout, a.Wout, L.cout);
        a.amax_out = out.amax;
        a.scale = L.scale; a.bias = L.shift;
        a.res = res ? res->p : nullptr;
        a.res_ld = res ? res->C : 0;
        a.out = out.p; a.out_ld = out.C;
        a.relu = relu ? 1 : 0;
        a.cfg = L.cfg ? L.cfg : (ok ? mc_choose_conv_cfg(h, op.cp) : CFG_128x32);
        push_conv(op);
        return out;
    }

    // heads pass 1: the fused 3x3 64 -> 9x64 (+bias) with per-(image, patch, channel) statistics for head_attn_kernel
    Tensor head_conv(const Tensor &feat) {
        const ConvLayer &L = h->head3;
        Tensor hidden = alloc(feat.B, feat.H, feat.W, L.cout);
        Op op{};
        ConvArgs &a = op.cp.a;
        pl->head_chunks = mc_head_conv_args(h, mem, feat, hidden.p, op.cp);
        pl->head_stats = a.stats;
        a.amax_out = hidden.amax;
        // per-patch centred second moments (head_attn_kernel combines them): whole 4x8 patches, no residual, and one partial
        // per patch -- true of the head conv on any map the plan accepts (H, W multiples of 32: a quarter-resolution map of 8s)
        a.stats_centred = 1;
        if (a.Hout % 4 || a.Wout % 8 || pl->head_chunks != (a.Hout / 4) * (a.Wout / 8)) { ok = false; h->err = "statistics of partial patches at " + L.conv; }
        push_conv(op);
        return hidden;
    }

    Tensor pool(const Tensor &x) {
        Tensor o = alloc(x.B, x.H / 2, x.W / 2, x.C);
        o.amax = x.amax;           // max |pool(x)| <= max |x|: the input's slot serves
        Op op{};
        op.kind = OP_POOL;
        op.in = x.p; op.out = o.p; op.B = x.B; op.H = x.H; op.W = x.W; op.C = x.C;
        op.bytes = 4.0 * ((double)x.numel() + (double)o.numel());
        pl->ops.push_back(op);
        return o;
    }

    Tensor deconv(const DeconvLayer &D, const Tensor &x) {
        Tensor o = alloc(x.B, x.H * 2, x.W * 2, x.C);
        Op op{};
        op.kind = OP_DECONV;
        op.in = x.p; op.out = o.p; op.w = D.wpk; op.B = x.B; op.H = x.H; op.W = x.W; op.C = x.C;
        op.amax = o.amax;
        op.flops = 2.0 * 4.0 * (double)o.numel();
        op.bytes = 4.0 * ((double)x.numel() + (double)o.numel());
        pl->ops.push_back(op);
        return o;
    }
};
}  // namespace

// The shape id of a planned launch description (the id it carries is ignored).  conv_plan() is asked under CFG_AUTO for what
// the layer is eligible for and for the default tiling, and under every candidate for whether it runs and on which family.
int mc_choose_conv_cfg(mc_handle *h, const ConvPlan &p) {
    ConvPlan t = p;
    ConvArgs &a = t.a;
    a.stats = nullptr;
    auto plan_as = [&](int cfg) -> const ConvPlan & { a.cfg = cfg; conv_plan(t); return t; };
    const int picked = plan_as(CFG_AUTO).shape;
    const bool small_ok = t.row_ok, b16 = t.b16;
    if (h->dry_alloc)    // mc_query_workspace: nothing is launched; only row-kernel eligibility matters for buffer sizes
        return (small_ok && !b16) ? (int)CFG_SMALL : picked;
    // the 16x16x4 row kernel sums K in a different order than the 32x32x2 tilings: choosing it by eligibility, not by
    // timing, keeps results independent of the batch size / of autotuning noise (it is also the faster one)
    if (small_ok && !b16) return CFG_SMALL;
    if (h->force_cfg) return h->force_cfg;   // mc_set_conv_cfg: every other layer
    const int heuristic = small_ok ? (int)CFG_SMALL : picked;
    if (!h->autotune) return heuristic;
    const bool lazy = conv_any_lazy(a);      // lazy sources (ConvSrc::la) stage differently: their own entry
    std::vector<int> key = {a.B, a.Hin, a.Win, t.ks, t.stride, a.Cout, a.CoutP, a.nsrc,
                            (a.res ? 1 : 0) | (b16 ? 2 * a.prec : 0) | (lazy ? 64 : 0)};
    for (int i = 0; i < a.nsrc; ++i) key.push_back(a.src[i].C);
    auto it = h->tuned.find(key);
    if (it != h->tuned.end()) return it->second;
    static const int cand[] = {CFG_128x128, CFG_128x64, CFG_128x64m, CFG_128x32, CFG_64x128, CFG_64x64,
                               CFG_WS | CFG_128x128, CFG_WS | CFG_128x64m, CFG_WS | CFG_64x128, CFG_WS | CFG_64x64, CFG_SMALL,
                               CFG_WRES | CFG_128x64};
    hipEvent_t e0, e1;
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return heuristic;
    int best = heuristic;
    float best_ms = 1e30f;
    for (int c : cand) {
        if (!plan_as(c).ok) continue;
        // a flag that this launch would run without (no wave-specialised / weight-resident kernel for it) is no candidate of its own
        if (((c & CFG_WS) && t.kernel != CONV_FP32_WS) || ((c & CFG_WRES) && t.kernel != CONV_WRES)) continue;
        if (launch_conv(t, nullptr) != hipSuccess) { (void)hipGetLastError(); continue; }   // warm
        float t_min = 1e30f;
        for (int rep = 0; rep < 3; ++rep) {
            (void)hipEventRecord(e0, nullptr);
            (void)launch_conv(t, nullptr);
            (void)hipEventRecord(e1, nullptr);
            if (hipEventSynchronize(e1) != hipSuccess) { t_min = 1e30f; break; }
            float ms = 0.f;
            (void)hipEventElapsedTime(&ms, e0, e1);
            t_min = std::min(t_min, ms);
        }
        if (t_min < best_ms) { best_ms = t_min; best = c; }
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    h->tuned[key] = best;
    if (const char *path = std::getenv("MONOCON_HIP_TUNE_CACHE")) {   // optional: persist across processes
        if (FILE *f = std::fopen(path, "a")) {
            for (int v : key) std::fprintf(f, "%d ", v);
            std::fprintf(f, ": %d\n", best);
            std::fclose(f);
        }
    }
    return best;
}

static void load_tune_cache(mc_handle *h) {
    const char *path = std::getenv("MONOCON_HIP_TUNE_CACHE");
    if (!path) return;
    FILE *f = std::fopen(path, "r");
    if (!f) return;
    char line[512];
    while (std::fgets(line, sizeof line, f)) {
        std::vector<int> key;
        char *p = line;
        int cfg = -1;
        for (;;) {
            while (*p == ' ') ++p;
            if (*p == ':') { cfg = std::atoi(p + 1); break; }
            if (!*p || *p == '\n') break;
            key.push_back((int)std::strtol(p, &p, 10));
        }
        if (cfg > 0 && key.size() >= 10) h->tuned[key] = cfg;
    }
    std::fclose(f);
}

static Plan *get_plan(mc_handle *h, int B, int H, int W) {
    auto key = std::make_tuple(B, H, W);
    auto it = h->plans.find(key);
    if (it != h->plans.end()) return it->second.get();
    std::unique_ptr<Plan> pl(new Plan());
    pl->B = B; pl->H = H; pl->W = W;
    Builder bd{h, pl.get()};

    // stem: NCHW image -> NHWC 16ch (reference dla.py:231-234)
    Tensor x0 = bd.alloc(B, H, W, 16);
    {
        Op op{};
        op.kind = OP_STEM;
        op.out = x0.p; op.B = B; op.H = H; op.W = W;
        op.w = h->stem_w; op.scale = h->stem_scale; op.shift = h->stem_shift;
        op.amax = x0.amax;
        op.flops = 2.0 * B * H * W * 16.0 * 147.0;
        op.bytes = 4.0 * ((double)B * 3 * H * W + (double)x0.numel());
        pl->stem_op = (int)pl->ops.size();
        pl->ops.push_back(op);
    }
    // backbone and neck: the steps of the network graph, one op each (dead steps skipped)
    const NetGraph &g = h->net;
    std::vector<Tensor> t(g.node_c.size());
    t[0] = x0;
    for (size_t i = 0; i < g.steps.size(); ++i) {
        const NetStep &s = g.steps[i];
        if ((int)i == g.n_backbone) pl->n_backbone_ops = (int)pl->ops.size();
        if (s.dead) continue;
        if (s.kind == STEP_CONV) {
            std::vector<const Tensor *> srcs;
            for (int x : s.srcs) srcs.push_back(&t[x]);
            t[s.out] = bd.conv(mc_conv_layer(h, s.name, bd.ok), srcs, s.res >= 0 ? &t[s.res] : nullptr, s.relu);
        } else if (s.kind == STEP_POOL) {
            t[s.out] = bd.pool(t[s.srcs[0]]);
        } else {
            t[s.out] = bd.deconv(h->deconvs[s.name], t[s.srcs[0]]);
        }
    }
    for (int i = 0; i < 6; ++i) pl->lv[i] = t[g.lv[i]];
    const Tensor feat = t[g.feat];
    pl->feat = feat;
    pl->nodes = t;
    pl->n_neck_ops = (int)pl->ops.size();

    const Tensor hidden = bd.head_conv(feat);
    float *hs_scale = bd.mem.alloc((size_t)B * NUM_HEADS * HEAD_CH);
    float *hs_shift = bd.mem.alloc((size_t)B * NUM_HEADS * HEAD_CH);
    pl->hidden = hidden; pl->hs_scale = hs_scale; pl->hs_shift = hs_shift;
    {
        Op op{};
        op.kind = OP_HEAD_ATTN;
        op.in = pl->head_stats; op.B = B; op.chunks = pl->head_chunks; op.H = feat.H; op.W = feat.W;
        op.out = hs_scale; op.out2 = hs_shift;
        pl->ops.push_back(op);
    }
    {
        Op op{};
        op.kind = OP_HEAD_APPLY;
        HeadApplyArgs &a = op.ha;
        a.hidden = hidden.p; a.scale = hs_scale; a.shift = hs_shift;
        a.w = h->head_w1t; a.b = h->head_b1;
        a.B = B; a.HW = feat.H * feat.W;
        for (int i = 0; i < MC_NUM_PREDS; ++i) a.pred_c[i] = PRED_CH[i];
        op.flops = 2.0 * B * a.HW * 64.0 * NUM_OUT_ROWS;
        op.bytes = 4.0 * ((double)hidden.numel() + (double)B * a.HW * NUM_OUT_ROWS);
        pl->head_apply_op = (int)pl->ops.size();
        pl->ops.push_back(op);
    }
    if (!bd.ok) {
        pl->mem.release();
        return nullptr;
    }
    for (auto &op : pl->ops) {
        pl->flops += op.flops;
        pl->hbm_bytes += op.bytes;
    }
    if (h->dry_alloc) {                       // counted only: hand the size back through dry_next, keep nothing
        h->dry_next = pl->mem.bytes;
        return nullptr;
    }
    if (hipDeviceSynchronize() != hipSuccess) return nullptr;   // buffer zero-fills ran on the null stream
    Plan *ret = pl.get();
    h->plans[key] = std::move(pl);
    return ret;
}

// precision mode 3: the max-|x| slots of a plan's tensors start every forward at zero (producers only raise them)
static int plan_reset_amax(mc_handle *h, Plan *pl, hipStream_t st) {
    if (pl->mem.amax_arena && pl->mem.amax_used)
        HIPCHK(h, hipMemsetAsync(pl->mem.amax_arena, 0, (size_t)pl->mem.amax_used * AMAX_WORDS * sizeof(unsigned), st));
    return 0;
}
// ... and a tensor that enters a plan from outside (stage-level forwards) gets its maximum from a pass of its own
static int plan_absmax(mc_handle *h, const Tensor &t, hipStream_t st) {
    if (t.amax) HIPCHK(h, launch_absmax(t.p, t.numel(), t.amax, st));
    return 0;
}

static int run_op(mc_handle *h, const Op &op, hipStream_t st) {
    switch (op.kind) {
        case OP_STEM:
            HIPCHK(h, launch_stem(op.in, op.B, op.H, op.W, op.w, op.scale, op.shift, op.out, st, 1, h->prec, op.amax));
            break;
        case OP_CONV:
            HIPCHK(h, launch_conv(op.cp, st));
            break;
        case OP_POOL:
            HIPCHK(h, launch_maxpool2(op.in, op.B, op.H, op.W, op.C, op.out, st));
            break;
        case OP_DECONV:
            HIPCHK(h, launch_deconv4(op.in, op.B, op.H, op.W, op.C, op.w, op.out, st, op.amax));
            break;
        case OP_HEAD_ATTN:
            HIPCHK(h, launch_head_attn(op.in, op.B, op.chunks, op.H * op.W, h->hap, op.out, op.out2, st));
            break;
        case OP_HEAD_APPLY:
            HIPCHK(h, launch_head_apply(op.ha, st));
            break;
    }
    return 0;
}

// ================================================================================== C ABI
// Tuning aid: sustained rate of v_mfma_f32_32x32x2_f32 with no memory traffic (the practical
// ceiling the conv kernel is measured against on this box: clocks follow the power budget).
__global__ __launch_bounds__(256) void mfma_peak_kernel(float *out, int iters, float seed) {
    f32x16 acc[4];
    for (int i = 0; i < 4; ++i)
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
    // seed > 0: nearly constant operands (low toggle rate); seed < 0: full-range pseudo-random
    // operands refreshed every MFMA group (DVFS: random data draws more power, lower clocks)
    unsigned ua = 1234567u + threadIdx.x * 7919u + blockIdx.x * 104729u, ub = ua * 2654435761u;
    float a = fabsf(seed) + threadIdx.x * 1e-3f, b = fabsf(seed) * 0.5f + threadIdx.x * 2e-3f;
    for (int it = 0; it < iters; ++it) {
        if (seed < 0.f) {
            ua = ua * 1664525u + 1013904223u;
            ub = ub * 22695477u + 1u;
            a = __uint_as_float((ua >> 9) | 0x3F800000u) - 1.5f;
            b = __uint_as_float((ub >> 9) | 0x3F800000u) - 1.5f;
        }
#pragma unroll
        for (int u = 0; u < 16; ++u) acc[u & 3] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[u & 3], 0, 0, 0);
        if (seed >= 0.f) a += 1e-6f;
    }
    float s = 0.f;
    for (int i = 0; i < 4; ++i)
        for (int r = 0; r < 16; ++r) s += acc[i][r];
    if (s == 12345.678f) out[0] = s;
}

extern "C" {

int mc_version(void) { return 1; }

int mc_create(int device, mc_handle **out) {
    if (!out) return fail(nullptr, "mc_create: out is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) return fail(nullptr, "mc_create: no HIP device visible (%s)", hipGetErrorString(e));
    if (device < 0 || device >= n) return fail(nullptr, "mc_create: device %d out of range (%d visible)", device, n);
    e = hipSetDevice(device);
    if (e != hipSuccess) return fail(nullptr, "hipSetDevice: %s", hipGetErrorString(e));
    hipDeviceProp_t prop;
    e = hipGetDeviceProperties(&prop, device);
    if (e != hipSuccess) return fail(nullptr, "hipGetDeviceProperties: %s", hipGetErrorString(e));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, "mc_create: device is %s; this library is built for gfx950 only", prop.gcnArchName);
    mc_handle *h = new mc_handle();
    h->device = device;
    if (const char *e = std::getenv("MONOCON_HIP_AUTOTUNE")) h->autotune = std::atoi(e) != 0;
    if (const char *e = std::getenv("MONOCON_HIP_PRECISION")) {
        if (std::strcmp(e, "bf16") == 0 || std::strcmp(e, "1") == 0) h->prec = 1;
        else if (std::strcmp(e, "bf16x3") == 0 || std::strcmp(e, "2") == 0) h->prec = 2;
        else if (std::strcmp(e, "f16x2") == 0 || std::strcmp(e, "3") == 0) h->prec = 3;
        else h->prec = 0;
    }
    load_tune_cache(h);
    *out = h;
    return 0;
}

int mc_destroy(mc_handle *h) {
    if (!h) return 0;
    (void)hipSetDevice(h->device);
    for (auto &kv : h->plans) kv.second->mem.release();
    h->params.release();
    if (h->decode_filt) (void)hipFree(h->decode_filt);
    if (h->nms_ws) (void)hipFree(h->nms_ws);
    if (h->loss_ws) (void)hipFree(h->loss_ws);
    if (h->train && h->train_free) h->train_free(h->train);
    if (h->comm && h->comm_free) h->comm_free(h->comm);
    if (h->opt_tab) (void)hipFree(h->opt_tab);
    if (h->opt_chunks) (void)hipFree(h->opt_chunks);
    if (h->clip_tab) (void)hipFree(h->clip_tab);
    if (h->clip_chunks) (void)hipFree(h->clip_chunks);
    if (h->ema_tab) (void)hipFree(h->ema_tab);
    if (h->ema_chunks) (void)hipFree(h->ema_chunks);
    if (h->accum_tab) (void)hipFree(h->accum_tab);
    if (h->accum_chunks) (void)hipFree(h->accum_chunks);
    if (h->opt_ws) (void)hipFree(h->opt_ws);
    if (h->opt_guard) (void)hipFree(h->opt_guard);
    if (h->lamb_ws.chunk_sums) (void)hipFree(h->lamb_ws.chunk_sums);
    delete h;
    return 0;
}

const char *mc_last_error(mc_handle *h) { return h ? h->err.c_str() : g_create_err.c_str(); }

int mc_bind_params(mc_handle *h, const mc_tensor_desc *descs, int n) {
    if (!h || !descs) return fail(h, "mc_bind_params: null argument");
    for (int i = 0; i < n; ++i) {
        if (!descs[i].name || !descs[i].ptr) return fail(h, "mc_bind_params: entry %d has a null name/pointer", i);
        h->bound[descs[i].name] = Bound{descs[i].ptr, descs[i].numel, descs[i].dtype};
    }
    h->packed = false;
    h->pack_clean = false;
    h->bind_gen++;
    return 0;
}

int mc_pack_params(mc_handle *h, int train_mode, void *stream) {
    if (!h) return -1;
    (void)train_mode;   // the same panels serve both modes; train mode ignores the folded BN scale/shift
    HIPCHK(h, hipSetDevice(h->device));
    if (build_layers(h)) return -1;
    hipStream_t st = static_cast<hipStream_t>(stream);
#define NEEDP(var, name, numel)                    \
    float *var = static_cast<float *>(mc_param(h, (name), (numel))); \
    if (!var) return -1;
    const bool has_bb = h->bound.count("backbone.base_layer.0.weight") != 0;
    const bool has_neck = h->bound.count("neck.ida_0.proj_1.conv.weight") != 0;
    const bool has_head = h->bound.count("head.heatmap_head.0.weight") != 0;
    if (!has_bb && !has_neck && !has_head) return fail(h, "mc_pack_params: no backbone./neck./head. parameters bound");
    const bool rebuild = h->pack_tab_gen != h->bind_gen || h->pack_tab_prec != h->prec;
    if (rebuild) { h->fwd_pack.clear(); h->folds.clear(); }
    if (rebuild) h->w_amax_of.clear();
    auto add_fwd = [&](const float *w, int Cout, int Cin, int ks, float *dst32, void *dst16, int CinPanel, int CoutP, int n_off,
                       unsigned *amax) {
        h->w_amax_of[w] = amax;
        h->fwd_pack.add(mc::pack_job_fwd(w, Cout, Cin, ks, dst32, dst16, CinPanel, CoutP, n_off, h->prec, amax));
    };
    for (auto &kv : h->convs) {
        if (!rebuild) break;
        ConvLayer &L = kv.second;
        const bool is_bb = L.conv.compare(0, 9, "backbone.") == 0;
        if ((is_bb && !has_bb) || (!is_bb && !has_neck)) continue;
        NEEDP(w, L.conv + ".weight", (int64_t)L.cout * L.cin * L.ks * L.ks);
        add_fwd(w, L.cout, L.cin, L.ks, L.wpk, L.wpk16, L.cin, L.coutp, 0, L.w_amax);
        NEEDP(g, L.bn + ".weight", L.cout);
        NEEDP(b, L.bn + ".bias", L.cout);
        NEEDP(rm, L.bn + ".running_mean", L.cout);
        NEEDP(rv, L.bn + ".running_var", L.cout);
        h->folds.add(mc::FoldJobDesc{g, b, rm, rv, 1e-5f, L.cout, L.scale, L.shift});
    }
    for (auto &kv : h->deconvs) {
        if (!has_neck) break;
        NEEDP(w, kv.second.name + ".weight", (int64_t)kv.second.C * 16);
        HIPCHK(h, launch_pack_deconv_w(w, kv.second.C, kv.second.wpk, st));
    }
    if (has_bb) {
        NEEDP(w, "backbone.base_layer.0.weight", 16 * 147);
        HIPCHK(h, launch_pack_stem_w(w, h->stem_w, st));
        NEEDP(g, "backbone.base_layer.1.weight", 16);
        NEEDP(b, "backbone.base_layer.1.bias", 16);
        NEEDP(rm, "backbone.base_layer.1.running_mean", 16);
        NEEDP(rv, "backbone.base_layer.1.running_var", 16);
        if (rebuild) h->folds.add(mc::FoldJobDesc{g, b, rm, rv, 1e-5f, 16, h->stem_scale, h->stem_shift});
    }
    // heads
    CopyBatch headcb;      // the 1x1 head weights / biases -> the fused [65][64] / [65] tables, one launch
    CopyBatch headcb2;     // 3x3 head biases and AttnBN running means -> their concatenated tables
    for (int hd = 0; hd < NUM_HEADS && has_head; ++hd) {
        const HeadKeys keys = mc_head_keys(hd);
        NEEDP(w3, keys.conv3 + ".weight", 64 * 64 * 9);
        NEEDP(b3, keys.conv3 + ".bias", 64);
        if (rebuild) add_fwd(w3, 64, 64, 3, h->head3.wpk, h->head3.wpk16, 64, h->head3.coutp, hd * HEAD_CH, h->head3.w_amax);
        if (!headcb2.add(b3, h->head_bias + hd * HEAD_CH, 64)) return fail(h, "mc_pack_params: head copy table overflow");
        const std::string &an = keys.attn;
        NEEDP(rm, an + ".running_mean", 64);
        NEEDP(rv, an + ".running_var", 64);
        if (!headcb2.add(rm, h->head_rm + hd * HEAD_CH, 64)) return fail(h, "mc_pack_params: head copy table overflow");
        NEEDP(wg, an + ".weight_", 640);
        NEEDP(wb, an + ".bias_", 640);
        NEEDP(aw, an + ".attn_weights.attention.0.weight", 640);
        NEEDP(ag, an + ".attn_weights.attention.1.weight", 10);
        NEEDP(ab, an + ".attn_weights.attention.1.bias", 10);
        NEEDP(arm, an + ".attn_weights.attention.1.running_mean", 10);
        NEEDP(arv, an + ".attn_weights.attention.1.running_var", 10);
        if (rebuild) h->folds.add(mc::FoldJobDesc{ag, ab, arm, arv, 1e-5f, 10, h->att_scale + hd * NUM_AFFINE, h->att_shift + hd * NUM_AFFINE});
        h->hap.att_w[hd] = aw;
        h->hap.att_scale[hd] = h->att_scale + hd * NUM_AFFINE;
        h->hap.att_shift[hd] = h->att_shift + hd * NUM_AFFINE;
        h->hap.weight_[hd] = wg;
        h->hap.bias_[hd] = wb;
        h->hap.rm[hd] = rm;
        h->hap.rv[hd] = rv;
        for (const HeadOutLayer &o : keys.out) {
            NEEDP(w1, o.layer + ".weight", (int64_t)o.rows * HEAD_CH);
            NEEDP(b1, o.layer + ".bias", o.rows);
            if (!headcb.add(w1, h->head_w1 + (size_t)o.row0 * HEAD_CH, (size_t)o.rows * HEAD_CH) || !headcb.add(b1, h->head_b1 + o.row0, o.rows))
                return fail(h, "mc_pack_params: head copy table overflow");
        }
    }
    if (rebuild) { h->pack_tab_gen = h->bind_gen; h->pack_tab_prec = h->prec; }
    if (h->prec == 3) HIPCHK(h, hipMemsetAsync(h->w_amax_arena, 0, (size_t)h->w_amax_n * sizeof(unsigned), st));
    HIPCHK(h, h->fwd_pack.launch(st, h->prec == 3));     // every forward panel (fp32 + bf16 / fp16 pieces) in one grid
    HIPCHK(h, h->folds.launch(st));        // every eval-mode BatchNorm fold in one grid
    HIPCHK(h, launch_copy_batch(headcb, st));
    HIPCHK(h, launch_copy_batch(headcb2, st));
    // [65][64] -> [64][65]: the second head pass reads one input channel against all rows of a head
    if (has_head) HIPCHK(h, launch_nchw_to_nhwc(h->head_w1, 1, NUM_OUT_ROWS, 1, HEAD_CH, h->head_w1t, st));
#undef NEEDP
    h->packed_groups = (has_bb ? 1 : 0) | (has_neck ? 2 : 0) | (has_head ? 4 : 0);
    h->packed = h->packed_groups == 7;
    h->pack_clean = true;
    return 0;
}

int mc_forward_infer(mc_handle *h, const float *img, int B, int H, int W, float *const preds[MC_NUM_PREDS],
                     float *feat_nchw, void *stream) {
    if (!h) return -1;
    if (!img || !preds) return fail(h, "mc_forward_infer: null argument");
    if (B < 1 || H < 32 || W < 32 || (H % 32) || (W % 32))
        return fail(h, "mc_forward_infer: bad shape B=%d H=%d W=%d (H, W must be multiples of 32)", B, H, W);
    if (!h->packed) return fail(h, "mc_forward_infer: call mc_bind_params + mc_pack_params first");
    HIPCHK(h, hipSetDevice(h->device));
    Plan *pl = get_plan(h, B, H, W);
    if (!pl) return -1;
    h->last_plan = pl;
    hipStream_t st = static_cast<hipStream_t>(stream);
    pl->ops[pl->stem_op].in = img;
    for (int i = 0; i < MC_NUM_PREDS; ++i) {
        if (!preds[i]) return fail(h, "mc_forward_infer: preds[%d] is NULL", i);
        pl->ops[pl->head_apply_op].ha.pred[i] = preds[i];
    }
    if (plan_reset_amax(h, pl, st)) return -1;
    for (const Op &op : pl->ops)
        if (run_op(h, op, st)) return -1;
    if (feat_nchw) HIPCHK(h, launch_nhwc_to_nchw(pl->feat.p, B, pl->feat.C, pl->feat.H, pl->feat.W, feat_nchw, st));
    return 0;
}

// debugging aid: read the eval plan of the last forward (h->last_plan) as NCHW, on the calling convention of
// mc_train_debug_node.  The eval plan gives every tensor a buffer of its own, so everything stays readable after the forward.
//   which = 0: the activation of graph node `node` (NetGraph ids, the train plan's: 0 = stem output, 1 = level0, ...)
//   which = 1: the raw hidden map of the fused head conv, (B, 9 * 64, H/4, W/4): bias added, before AttnBN (`node` ignored)
//   which = 2: head_attn_kernel's AttnBN affine as (B, 2, 9, 64): [b][0] the scale, [b][1] the shift of every
//              (head, channel) of image b (`node` ignored)
//   which = 3: the AttnBN statistic s = mean / sqrt(var + 1e-3) as (B, 1, 9, 64), folded on the HOST in fp64 from the conv
//              epilogue's per-patch fp32 partials exactly as head_attn_kernel folds them (no launch; synchronises `stream`)
int mc_infer_debug_node(mc_handle *h, int node, int which, float *out_nchw, int dims[4], void *stream) {
    if (!h || !h->last_plan) return fail(h, "mc_infer_debug_node: no eval plan has run");
    const Plan *pl = h->last_plan;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (which == 2) {
        if (dims) { dims[0] = pl->B; dims[1] = 2; dims[2] = NUM_HEADS; dims[3] = HEAD_CH; }
        if (!out_nchw) return 0;
        const size_t n = (size_t)NUM_HEADS * HEAD_CH;
        HIPCHK(h, hipMemcpy2DAsync(out_nchw, 2 * n * sizeof(float), pl->hs_scale, n * sizeof(float), n * sizeof(float), pl->B,
                                   hipMemcpyDeviceToDevice, st));
        HIPCHK(h, hipMemcpy2DAsync(out_nchw + n, 2 * n * sizeof(float), pl->hs_shift, n * sizeof(float), n * sizeof(float), pl->B,
                                   hipMemcpyDeviceToDevice, st));
        return 0;
    }
    if (which == 3) {
        if (dims) { dims[0] = pl->B; dims[1] = 1; dims[2] = NUM_HEADS; dims[3] = HEAD_CH; }
        if (!out_nchw) return 0;
        const int CP = NUM_HEADS * HEAD_CH, chunks = pl->head_chunks;
        std::vector<float> part((size_t)pl->B * chunks * CP * 2), rm(CP), s((size_t)pl->B * CP);
        HIPCHK(h, hipStreamSynchronize(st));
        HIPCHK(h, hipMemcpy(part.data(), pl->head_stats, part.size() * sizeof(float), hipMemcpyDeviceToHost));
        HIPCHK(h, hipMemcpy(rm.data(), h->head_rm, rm.size() * sizeof(float), hipMemcpyDeviceToHost));
        const double n = (double)pl->feat.H * pl->feat.W;
        for (int b = 0; b < pl->B; ++b)
            for (int c = 0; c < CP; ++c) {
                double s1 = 0.0, s2 = 0.0;
                for (int k = 0; k < chunks; ++k) {
                    const float *q = &part[(((size_t)b * chunks + k) * CP + c) * 2];
                    s1 += (double)q[0];
                    s2 += (double)q[1] + (double)q[0] * (double)q[0] * 0.03125;       // (centred per-patch moments: Chan's formula)
                }
                const double mean = (double)rm[c] + s1 / n, var = (s2 - s1 * s1 / n) / (n - 1.0);
                s[(size_t)b * CP + c] = (float)(mean / std::sqrt(var + 1e-3));
            }
        HIPCHK(h, hipMemcpy(out_nchw, s.data(), s.size() * sizeof(float), hipMemcpyHostToDevice));
        return 0;
    }
    if (which != 0 && which != 1) return fail(h, "mc_infer_debug_node: which = %d (0 node, 1 hidden, 2 AttnBN affine, 3 s)", which);
    if (!which && (node < 0 || node >= (int)pl->nodes.size()))
        return fail(h, "mc_infer_debug_node: node %d of %d", node, (int)pl->nodes.size());
    const Tensor &t = which ? pl->hidden : pl->nodes[node];
    if (dims) { dims[0] = t.B; dims[1] = t.C; dims[2] = t.H; dims[3] = t.W; }
    if (!out_nchw) return 0;
    if (!t.p) return fail(h, "mc_infer_debug_node: node has no buffer");
    HIPCHK(h, launch_nhwc_to_nchw(t.p, t.B, t.C, t.H, t.W, out_nchw, st));
    return 0;
}

// ---- stage-level forwards (sub-module API parity: DLA.forward / DLAUp.forward / head._get_predictions)
static Plan *stage_plan(mc_handle *h, int need_groups, int B, int H, int W, const char *who) {
    if (B < 1 || H < 32 || W < 32 || (H % 32) || (W % 32)) {
        fail(h, "%s: bad shape B=%d H=%d W=%d (H, W must be multiples of 32)", who, B, H, W);
        return nullptr;
    }
    if ((h->packed_groups & need_groups) != need_groups) {
        fail(h, "%s: parameters of this stage are not bound/packed", who);
        return nullptr;
    }
    if (hipSetDevice(h->device) != hipSuccess) { fail(h, "%s: hipSetDevice failed", who); return nullptr; }
    Plan *pl = get_plan(h, B, H, W);
    if (pl) h->last_plan = pl;
    return pl;
}

int mc_backbone_forward(mc_handle *h, const float *img, int B, int H, int W, float *const levels[6], void *stream) {
    if (!h) return -1;
    if (!img || !levels) return fail(h, "mc_backbone_forward: null argument");
    Plan *pl = stage_plan(h, 1, B, H, W, "mc_backbone_forward");
    if (!pl) return -1;
    hipStream_t st = static_cast<hipStream_t>(stream);
    pl->ops[pl->stem_op].in = img;
    if (plan_reset_amax(h, pl, st)) return -1;
    for (int i = 0; i < pl->n_backbone_ops; ++i)
        if (run_op(h, pl->ops[i], st)) return -1;
    for (int i = 0; i < 6; ++i)
        if (levels[i]) {
            const Tensor &t = pl->lv[i];
            HIPCHK(h, launch_nhwc_to_nchw(t.p, t.B, t.C, t.H, t.W, levels[i], st));
        }
    return 0;
}

int mc_neck_forward(mc_handle *h, const float *const levels[6], int B, int H, int W, float *feat, void *stream) {
    if (!h) return -1;
    if (!levels || !feat) return fail(h, "mc_neck_forward: null argument");
    Plan *pl = stage_plan(h, 2, B, H, W, "mc_neck_forward");
    if (!pl) return -1;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (plan_reset_amax(h, pl, st)) return -1;
    for (int i = 2; i < 6; ++i) {
        if (!levels[i]) return fail(h, "mc_neck_forward: levels[%d] is NULL", i);
        const Tensor &t = pl->lv[i];
        HIPCHK(h, launch_nchw_to_nhwc(levels[i], t.B, t.C, t.H, t.W, t.p, st));
        if (plan_absmax(h, t, st)) return -1;
    }
    for (int i = pl->n_backbone_ops; i < pl->n_neck_ops; ++i)
        if (run_op(h, pl->ops[i], st)) return -1;
    HIPCHK(h, launch_nhwc_to_nchw(pl->feat.p, B, pl->feat.C, pl->feat.H, pl->feat.W, feat, st));
    return 0;
}

int mc_head_forward(mc_handle *h, const float *feat, int B, int H, int W, float *const preds[MC_NUM_PREDS],
                    void *stream) {
    if (!h) return -1;
    if (!feat || !preds) return fail(h, "mc_head_forward: null argument");
    Plan *pl = stage_plan(h, 4, B, H, W, "mc_head_forward");
    if (!pl) return -1;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (plan_reset_amax(h, pl, st)) return -1;
    HIPCHK(h, launch_nchw_to_nhwc(feat, B, pl->feat.C, pl->feat.H, pl->feat.W, pl->feat.p, st));
    if (plan_absmax(h, pl->feat, st)) return -1;
    for (int i = 0; i < MC_NUM_PREDS; ++i) {
        if (!preds[i]) return fail(h, "mc_head_forward: preds[%d] is NULL", i);
        pl->ops[pl->head_apply_op].ha.pred[i] = preds[i];
    }
    for (int i = pl->n_neck_ops; i < (int)pl->ops.size(); ++i)
        if (run_op(h, pl->ops[i], st)) return -1;
    return 0;
}

int mc_decode(mc_handle *h, const float *const preds[MC_NUM_PREDS], const float *P2, const float *P2inv, int B, int C,
              int H, int W, int K, float thr, float pad_h, float pad_w, float *scores, int64_t *flat_index,
              int64_t *cls, float *box2d, float *box3d, uint8_t *keep_localmax, uint8_t *keep_thr, void *stream) {
    if (!h) return -1;
    if (!preds || !P2 || !P2inv || !scores || !flat_index || !cls || !box2d || !box3d)
        return fail(h, "mc_decode: null argument");
    const int need[] = {0, 2, 3, 5, 6, 7, 8, 9};
    for (int i : need)
        if (!preds[i]) return fail(h, "mc_decode: preds[%d] is NULL", i);
    if (B < 1 || C < 1 || H < 1 || W < 1 || K < 1 || K > 1024 || (int64_t)K > (int64_t)C * H * W)
        return fail(h, "mc_decode: bad shape B=%d C=%d H=%d W=%d K=%d (1 <= K <= min(1024, C*H*W))", B, C, H, W, K);
    HIPCHK(h, hipSetDevice(h->device));
    const size_t n = (size_t)B * C * H * W;
    const size_t ncnt = (size_t)B * decode_chunks(C * H * W);
    if (n > h->decode_filt_n || ncnt > h->decode_count_n) {
        // one block: filtered map, candidate keys, candidate indices (n words each), per-(image, chunk) candidate counts
        if (h->decode_filt) HIPCHK(h, hipFree(h->decode_filt));
        h->decode_filt = nullptr;
        h->decode_filt_n = 0;
        h->decode_count_n = 0;
        void *q = nullptr;
        HIPCHK(h, hipMalloc(&q, (3 * n + ncnt) * sizeof(float)));
        h->decode_filt = static_cast<float *>(q);
        h->decode_filt_n = n;
        h->decode_count_n = ncnt;
    }
    DecodeArgs a{};
    for (int i = 0; i < MC_NUM_PREDS; ++i) a.pred[i] = preds[i];
    a.P2 = P2; a.P2inv = P2inv;
    a.B = B; a.C = C; a.H = H; a.W = W; a.K = K;
    a.lm_kernel = h->lm_kernel;
    a.thr = thr; a.pad_h = pad_h; a.pad_w = pad_w;
    a.scores = scores; a.flat_index = flat_index; a.cls = cls;
    a.box2d = box2d; a.box3d = box3d;
    a.keep_localmax = keep_localmax; a.keep_thr = keep_thr;
    a.filt = h->decode_filt;
    a.cand_key = reinterpret_cast<unsigned *>(h->decode_filt + h->decode_filt_n);
    a.cand_idx = reinterpret_cast<int *>(h->decode_filt + 2 * h->decode_filt_n);
    a.cand_count = reinterpret_cast<unsigned *>(h->decode_filt + 3 * h->decode_filt_n);
    HIPCHK(h, launch_decode(a, static_cast<hipStream_t>(stream)));
    return 0;
}

// ---------------------------------------------------------------------------- op-level
int mc_op_conv(mc_handle *h, const float *const src[], const int src_channels[], int nsrc, int B, int Hin, int Win,
               const float *weight_oihw, int Cout, int ksize, int stride, const float *scale, const float *bias,
               const float *residual, int relu, float *out, void *stream) {
    if (!h) return -1;
    if (!src || !src_channels || !weight_oihw || !out) return fail(h, "mc_op_conv: null argument");
    if (nsrc < 1 || nsrc > 4) return fail(h, "mc_op_conv: nsrc=%d (1..4)", nsrc);
    if (!((ksize == 3 && (stride == 1 || stride == 2)) || (ksize == 1 && stride == 1)))
        return fail(h, "mc_op_conv: unsupported k=%d stride=%d", ksize, stride);
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    Tensor x[4];
    std::vector<const Tensor *> xs;
    ConvLayer L;            // the temporary panel, described the way the plans describe a layer's
    L.ks = ksize; L.stride = stride; L.cout = Cout; L.coutp = conv_coutp(Cout);
    for (int i = 0; i < nsrc; ++i) {
        if (!src[i] || src_channels[i] % 16) return fail(h, "mc_op_conv: source %d needs C %% 16 == 0", i);
        x[i] = operand_tensor(src[i], B, Hin, Win, src_channels[i]);
        xs.push_back(&x[i]);
        L.cin += src_channels[i];
    }
    const size_t wn = fwd_panel_elems(ksize, L.cin, L.coutp);
    ScratchBuf wpk, wpk16;
    HIPCHK(h, wpk.alloc(wn * sizeof(float)));
    HIPCHK(h, hipMemsetAsync(wpk.p, 0, wn * sizeof(float), st));
    L.wpk = wpk.as<float>();
    ScratchBuf slots;       // mode 3: max |x| of every source from a pass of its own; the pack finds max |w|
    if (panel_has_pieces(h->prec, L.cin)) {
        if (h->prec == 3) {
            size_t n[4];
            for (int i = 0; i < nsrc; ++i) n[i] = x[i].numel();
            HIPCHK(h, op_amax_slots(slots, src, n, nsrc, nullptr, 0, true, st));
            for (int i = 0; i < nsrc; ++i) x[i].amax = slots.as<unsigned>() + i * AMAX_WORDS;
            L.w_amax = slots.as<unsigned>() + 4 * AMAX_WORDS;
        }
        const size_t bytes16 = wn * 2 * split_pieces(h->prec);
        HIPCHK(h, wpk16.alloc(bytes16));
        HIPCHK(h, hipMemsetAsync(wpk16.p, 0, bytes16, st));
        L.wpk16 = wpk16.p;
    }
    PackBatch pack;         // the plans' packer, one job
    pack.add(pack_job_fwd(weight_oihw, Cout, L.cin, ksize, L.wpk, L.wpk16, L.cin, L.coutp, 0, h->prec, L.w_amax));
    HIPCHK(h, pack.launch(st, h->prec == 3));
    ConvPlan cp{};
    ConvArgs &a = cp.a;
    a.scale = scale; a.bias = bias; a.res = residual; a.res_ld = Cout;
    a.out = out; a.out_ld = Cout; a.relu = relu;
    a.cfg = h->force_cfg;
    conv_fwd_args(cp, L, xs, h->prec);
    hipError_t e = launch_conv(cp, st);
    hipError_t e2 = hipStreamSynchronize(st);   // test entry point: the packed weights are a temporary
    HIPCHK(h, e);
    HIPCHK(h, e2);
    return 0;
}

int mc_op_stem(mc_handle *h, const float *img, int B, int H, int W, const float *weight_oihw, const float *scale,
               const float *bias, float *out, void *stream) {
    if (!h) return -1;
    if (!img || !weight_oihw || !scale || !bias || !out) return fail(h, "mc_op_stem: null argument");
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    ScratchBuf wpk;
    HIPCHK(h, wpk.alloc(147 * 16 * sizeof(float)));
    HIPCHK(h, launch_pack_stem_w(weight_oihw, wpk.as<float>(), st));
    hipError_t e = launch_stem(img, B, H, W, wpk.as<float>(), scale, bias, out, st, 1, h->prec);
    hipError_t e2 = hipStreamSynchronize(st);
    HIPCHK(h, e);
    HIPCHK(h, e2);
    return 0;
}

int mc_op_stem_dgrad(mc_handle *h, const float *dy_nhwc, const float *weight_oihw, int B, int H, int W, float *dx_nchw,
                     void *stream) {
    if (!h) return -1;
    if (!dy_nhwc || !weight_oihw || !dx_nchw) return fail(h, "mc_op_stem_dgrad: null argument");
    if (B < 1 || H < 1 || W < 1) return fail(h, "mc_op_stem_dgrad: B, H, W must be >= 1 (got %d, %d, %d)", B, H, W);
    if (reinterpret_cast<uintptr_t>(dy_nhwc) % 16) return fail(h, "mc_op_stem_dgrad: dy_nhwc must be 16-byte aligned");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, launch_stem_dgrad(dy_nhwc, weight_oihw, B, H, W, dx_nchw, static_cast<hipStream_t>(stream)));
    return 0;
}

int mc_op_stem_dgrad_fused(mc_handle *h, const float *d_nhwc, const float *y_nhwc, const float *coef, const float *weight_oihw,
                           int B, int H, int W, float *dx_nchw, void *stream) {
    if (!h) return -1;
    if (!d_nhwc || !y_nhwc || !coef || !weight_oihw || !dx_nchw) return fail(h, "mc_op_stem_dgrad_fused: null argument");
    if (B < 1 || H < 1 || W < 1) return fail(h, "mc_op_stem_dgrad_fused: B, H, W must be >= 1 (got %d, %d, %d)", B, H, W);
    if (reinterpret_cast<uintptr_t>(d_nhwc) % 16 || reinterpret_cast<uintptr_t>(y_nhwc) % 16 || reinterpret_cast<uintptr_t>(coef) % 16)
        return fail(h, "mc_op_stem_dgrad_fused: d_nhwc, y_nhwc and coef must be 16-byte aligned");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, launch_stem_dgrad(d_nhwc, weight_oihw, B, H, W, dx_nchw, static_cast<hipStream_t>(stream), y_nhwc, coef));
    return 0;
}

int mc_op_maxpool2(mc_handle *h, const float *in, int B, int H, int W, int C, float *out, void *stream) {
    if (!h) return -1;
    if (!in || !out || (C % 4) || (H % 2) || (W % 2)) return fail(h, "mc_op_maxpool2: bad argument");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, launch_maxpool2(in, B, H, W, C, out, static_cast<hipStream_t>(stream)));
    return 0;
}

int mc_op_deconv4x4(mc_handle *h, const float *in, int B, int H, int W, int C, const float *weight, float *out,
                    void *stream) {
    if (!h) return -1;
    if (!in || !out || !weight || (C % 4)) return fail(h, "mc_op_deconv4x4: bad argument");
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    ScratchBuf wpk;
    HIPCHK(h, wpk.alloc((size_t)16 * C * sizeof(float)));
    HIPCHK(h, launch_pack_deconv_w(weight, C, wpk.as<float>(), st));
    hipError_t e = launch_deconv4(in, B, H, W, C, wpk.as<float>(), out, st);
    hipError_t e2 = hipStreamSynchronize(st);
    HIPCHK(h, e);
    HIPCHK(h, e2);
    return 0;
}

int mc_op_nchw_to_nhwc(mc_handle *h, const float *in, int B, int C, int H, int W, float *out, void *stream) {
    if (!h) return -1;
    if (!in || !out) return fail(h, "mc_op_nchw_to_nhwc: null argument");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, launch_nchw_to_nhwc(in, B, C, H, W, out, static_cast<hipStream_t>(stream)));
    return 0;
}

int mc_op_nhwc_to_nchw(mc_handle *h, const float *in, int B, int C, int H, int W, float *out, void *stream) {
    if (!h) return -1;
    if (!in || !out) return fail(h, "mc_op_nhwc_to_nchw: null argument");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, launch_nhwc_to_nchw(in, B, C, H, W, out, static_cast<hipStream_t>(stream)));
    return 0;
}

int mc_preprocess(mc_handle *h, const void *img_hwc, int dtype, int H, int W, const double mean[3], const double std[3],
                  int pad_h, int pad_w, float *out_chw, void *stream) {
    if (!h) return -1;
    if (!img_hwc || !mean || !std || !out_chw) return fail(h, "mc_preprocess: null argument");
    if (dtype != 0 && dtype != 2) return fail(h, "mc_preprocess: dtype must be 0 (float32) or 2 (uint8)");
    if (H < 1 || W < 1 || pad_h < H || pad_w < W) return fail(h, "mc_preprocess: bad shape %dx%d -> %dx%d", H, W, pad_h, pad_w);
    for (int c = 0; c < 3; ++c)
        if (std[c] == 0.0) return fail(h, "mc_preprocess: std[%d] is zero", c);
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, launch_preprocess(img_hwc, dtype == 2, H, W, mean, std, pad_h, pad_w, out_chw, static_cast<hipStream_t>(stream)));
    return 0;
}

int mc_preprocess_augmented(mc_handle *h, const unsigned char *frames_hwc, const float *params, int B, int src_h, int src_w,
                            const double mean[3], const double std[3], int pad_h, int pad_w, float *out_bchw, void *stream) {
    if (!h) return -1;
    if (!frames_hwc || !params || !mean || !std || !out_bchw) return fail(h, "mc_preprocess_augmented: null argument");
    if (B < 1 || src_h < 1 || src_w < 1 || pad_h < 1 || pad_w < 1 || B > 65535 || pad_h > 65535)
        return fail(h, "mc_preprocess_augmented: bad shape B=%d %dx%d -> %dx%d", B, src_h, src_w, pad_h, pad_w);
    for (int c = 0; c < 3; ++c)
        if (std[c] == 0.0) return fail(h, "mc_preprocess_augmented: std[%d] is zero", c);
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, launch_preprocess_aug(frames_hwc, params, B, src_h, src_w, mean, std, pad_h, pad_w, out_bchw, static_cast<hipStream_t>(stream)));
    return 0;
}

int mc_bench_mfma_peak(mc_handle *h, int waves_per_simd, int iters, float *tflops) {
    if (!h || !tflops) return fail(h, "mc_bench_mfma_peak: null argument");
    HIPCHK(h, hipSetDevice(h->device));
    void *out = nullptr;
    HIPCHK(h, hipMalloc(&out, 64));
    hipEvent_t e0, e1;
    HIPCHK(h, hipEventCreate(&e0));
    HIPCHK(h, hipEventCreate(&e1));
    const int blocks = 256 * (waves_per_simd < 0 ? -waves_per_simd : waves_per_simd);   // < 0: random operands
    hipLaunchKernelGGL(mfma_peak_kernel, dim3(blocks), dim3(256), 0, nullptr, (float *)out, 100, waves_per_simd < 0 ? -1.0f : 1.0f);
    (void)hipEventRecord(e0, nullptr);
    hipLaunchKernelGGL(mfma_peak_kernel, dim3(blocks), dim3(256), 0, nullptr, (float *)out, iters, waves_per_simd < 0 ? -1.0f : 1.0f);
    (void)hipEventRecord(e1, nullptr);
    (void)hipEventSynchronize(e1);
    float ms = 0;
    (void)hipEventElapsedTime(&ms, e0, e1);
    *tflops = (float)((double)blocks * 4 * iters * 16 * 4096.0 / (ms * 1e-3) / 1e12);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    (void)hipFree(out);
    return 0;
}

// Tuning aid: time one fused conv launch shape on synthetic data (random, non-zero operands).
int mc_bench_conv(mc_handle *h, int B, int Hin, int Win, int nsrc, const int src_channels[], int Cout, int ksize,
                  int stride, int cfg, int iters, float *ms_avg) {
    if (!h || !src_channels || !ms_avg) return fail(h, "mc_bench_conv: null argument");
    HIPCHK(h, hipSetDevice(h->device));
    ConvPlan cp{};
    ConvArgs &a = cp.a;
    std::vector<void *> bufs;
    // MONOCON_BENCH_ZERO=1: all-zero operands (same instruction stream, minimal toggling): how much of a launch's time is
    // the power limit (DVFS) rather than stalls
    const bool zero_data = std::getenv("MONOCON_BENCH_ZERO") != nullptr;
    auto alloc_fill = [&](size_t n, float scale) -> float * {
        if (zero_data) scale = 0.f;
        void *q = nullptr;
        if (hipMalloc(&q, n * sizeof(float)) != hipSuccess) return nullptr;
        bufs.push_back(q);
        std::vector<float> hst(std::min<size_t>(n, (size_t)1 << 22));
        unsigned s = 12345u + (unsigned)bufs.size();
        for (auto &v : hst) { s = s * 1664525u + 1013904223u; v = scale * (((s >> 8) & 0xFFFF) / 32768.0f - 1.0f); }
        for (size_t off = 0; off < n; off += hst.size())
            (void)hipMemcpy((float *)q + off, hst.data(), std::min(hst.size(), n - off) * sizeof(float), hipMemcpyHostToDevice);
        return (float *)q;
    };
    Tensor x[4];
    std::vector<const Tensor *> xs;
    ConvLayer L;            // the synthetic panel, described the way the plans describe a layer's
    L.ks = ksize; L.stride = stride; L.cout = Cout; L.coutp = conv_coutp(Cout);
    for (int i = 0; i < nsrc; ++i) {
        x[i] = operand_tensor(alloc_fill((size_t)B * Hin * Win * src_channels[i], 1.0f), B, Hin, Win, src_channels[i]);
        if (!x[i].p) return fail(h, "mc_bench_conv: out of memory");
        xs.push_back(&x[i]);
        L.cin += src_channels[i];
    }
    const int Ho = conv_out_dim(Hin, ksize, stride), Wo = conv_out_dim(Win, ksize, stride);
    const size_t wn = fwd_panel_elems(ksize, L.cin, L.coutp), on = (size_t)B * Ho * Wo * Cout;
    const size_t stats_n = (size_t)B * ((Wo + 7) / 8) * ((Ho + 3) / 4) * L.coutp * 2;     // one partial per 4x8 patch
    L.wpk = alloc_fill(wn, 0.05f);
    a.scale = alloc_fill(Cout, 1.0f);
    a.bias = alloc_fill(Cout, 1.0f);
    a.out = alloc_fill(on, 0.0f);
    if (!L.wpk || !a.scale || !a.bias || !a.out) return fail(h, "mc_bench_conv: out of memory");
    a.out_ld = Cout; a.relu = 1; a.cfg = cfg;
    // MONOCON_BENCH_STATS=1: the train-mode forward's statistics partials; MONOCON_BENCH_BM=1 / 2: the backward-statistics
    // epilogue (mask recomputed from y / read from a stored activation), =3: the latter with an accumulated gradient
    if (const char *e = std::getenv("MONOCON_BENCH_STATS")) {
        if (std::atoi(e)) a.stats = alloc_fill(stats_n, 0.f);
    }
    if (const char *e = std::getenv("MONOCON_BENCH_BM")) {
        const int m = std::atoi(e);
        if (m) {
            a.relu = 0;
            a.stats = alloc_fill(stats_n, 0.f);
            a.bm_y = alloc_fill(on, 1.0f);
            a.bm_a = a.scale; a.bm_b = a.bias; a.bm_relu = m == 1 ? 2 : 1;
            if (m >= 2) a.bm_z = alloc_fill(on, 1.0f);
            if (m >= 3) { a.res = alloc_fill(on, 1.0f); a.res_ld = Cout; }
            if (!a.stats || !a.bm_y || (m >= 2 && !a.bm_z) || (m >= 3 && !a.res)) return fail(h, "mc_bench_conv: out of memory");
        }
    }
    if (h->prec >= 1 && L.cin % 32 == 0) {        // bf16 / fp16 pipe: piece panels (random finite bit patterns) + unit maxima
        std::vector<unsigned short> hw(wn * 3);
        unsigned s16 = 777u;
        for (auto &v : hw) { s16 = s16 * 1664525u + 1013904223u; v = zero_data ? 0 : (unsigned short)(0x2c00u + ((s16 >> 12) & 0x3ffu) + ((s16 >> 31) << 15)); }
        void *q = nullptr;
        if (hipMalloc(&q, hw.size() * 2) != hipSuccess) return fail(h, "mc_bench_conv: out of memory");
        bufs.push_back(q);
        (void)hipMemcpy(q, hw.data(), hw.size() * 2, hipMemcpyHostToDevice);
        L.wpk16 = q;
        std::vector<unsigned> one((size_t)5 * AMAX_WORDS, 0x3f800000u);
        if (hipMalloc(&q, one.size() * 4) != hipSuccess) return fail(h, "mc_bench_conv: out of memory");
        bufs.push_back(q);
        (void)hipMemcpy(q, one.data(), one.size() * 4, hipMemcpyHostToDevice);
        for (int i = 0; i < nsrc; ++i) x[i].amax = static_cast<unsigned *>(q) + (size_t)i * AMAX_WORDS;
        L.w_amax = static_cast<unsigned *>(q) + (size_t)4 * AMAX_WORDS;
    }
    conv_fwd_args(cp, L, xs, h->prec);
#ifdef MC_PHASE_TIMERS
    const size_t prof_n = (size_t)1 << 22;          // (workgroups x waves x 5) upper bound
    {
        void *q = nullptr;
        if (hipMalloc(&q, prof_n * 8) != hipSuccess) return fail(h, "mc_bench_conv: out of memory");
        bufs.push_back(q);
        (void)hipMemset(q, 0, prof_n * 8);
        a.phase_prof = static_cast<unsigned long long *>(q);
    }
#endif
    hipEvent_t e0, e1;
    HIPCHK(h, hipEventCreate(&e0));
    HIPCHK(h, hipEventCreate(&e1));
    hipError_t e = launch_conv(cp, nullptr);
    if (e == hipSuccess) e = launch_conv(cp, nullptr);
    if (e == hipSuccess) {
        (void)hipEventRecord(e0, nullptr);
        for (int i = 0; i < iters && e == hipSuccess; ++i) e = launch_conv(cp, nullptr);
        (void)hipEventRecord(e1, nullptr);
        (void)hipEventSynchronize(e1);
        float ms = 0;
        (void)hipEventElapsedTime(&ms, e0, e1);
        *ms_avg = ms / iters;
#ifdef MC_PHASE_TIMERS
        if (a.phase_prof) {
            std::vector<unsigned long long> hp(prof_n);
            (void)hipMemcpy(hp.data(), a.phase_prof, prof_n * 8, hipMemcpyDeviceToHost);
            double sum[5] = {0, 0, 0, 0, 0};
            size_t n = 0;
            for (size_t i = 0; i + 5 <= prof_n; i += 5)
                if (hp[i + 4]) { for (int k = 0; k < 5; ++k) sum[k] += (double)hp[i + k]; ++n; }
            if (n) std::fprintf(stderr, "[phase] waves %zu  avg cycles per wave: stage %.0f  barriers %.0f  mfma-phase %.0f  epilogue %.0f  total %.0f\n",
                                n, sum[0] / n, sum[1] / n, sum[2] / n, sum[3] / n, sum[4] / n);
        }
#endif
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    for (void *q : bufs) (void)hipFree(q);
    HIPCHK(h, e);
    return 0;
}

int mc_set_conv_cfg(mc_handle *h, int cfg) {
    if (!h) return -1;
    const int shape_bits = cfg & CFG_SHAPE_BITS;
    if (cfg != CFG_SMALL && (cfg < 0 || (shape_bits && !conv_shape(cfg).id) || (cfg & ~(CFG_SHAPE_BITS | CFG_WS | CFG_WRES))))
        return fail(h, "mc_set_conv_cfg: unknown shape id");
    if ((cfg & (CFG_WS | CFG_WRES)) && !shape_bits) return fail(h, "mc_set_conv_cfg: the kernel-variant flags need a shape");
    h->force_cfg = cfg;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipDeviceSynchronize());
    for (auto &kv : h->plans) kv.second->mem.release();   // plans bake the shape into their launch arguments
    h->plans.clear();
    return 0;
}

// The autotuned workgroup shapes as a flat int table: per entry [key length, key..., shape id].  Data-parallel ranks exchange
// it (rank 0 tunes, the others import before they build their plans) so that every replica runs the SAME tilings: the
// timing-based choice can differ between ranks that tune concurrently -- results would stay bit-identical (the shapes
// do not change the arithmetic), the step times would not.
int mc_tune_export(mc_handle *h, int *buf, int cap, int *n_ints) {
    if (!h || !n_ints) return -1;
    int n = 0;
    for (auto &kv : h->tuned) n += 2 + (int)kv.first.size();
    *n_ints = n;
    if (!buf) return 0;                       // size query
    if (cap < n) return fail(h, "mc_tune_export: buffer of %d ints, %d needed", cap, n);
    int o = 0;
    for (auto &kv : h->tuned) {
        buf[o++] = (int)kv.first.size();
        for (int v : kv.first) buf[o++] = v;
        buf[o++] = kv.second;
    }
    return 0;
}

int mc_tune_import(mc_handle *h, const int *buf, int n_ints) {
    if (!h || (!buf && n_ints > 0)) return -1;
    // A table is adopted as a whole or not at all: every entry is checked before the first one is stored.
    std::vector<std::pair<std::vector<int>, int>> entries;
    int o = 0;
    while (o < n_ints) {
        const int kl = buf[o++];
        if (kl < 10 || kl > 16 || o + kl + 1 > n_ints) return fail(h, "mc_tune_import: malformed table at int %d", o - 1);
        std::vector<int> key(buf + o, buf + o + kl);
        o += kl;
        const int cfg = buf[o++];
        // (a shape id is CFG_SMALL, or an entry of CONV_SHAPES with optional kernel-variant flags: a flag alone is no shape)
        if (cfg != CFG_SMALL && (cfg <= 0 || !conv_shape(cfg).id || (cfg & ~(CFG_SHAPE_BITS | CFG_WS | CFG_WRES))))
            return fail(h, "mc_tune_import: unknown shape id %d", cfg);
        // a tiling whose column tile does not divide the signature's padded column count (key[6]) has no launch: every
        // dispatch refuses it -- but only when the plan RUNS, after the launches in front of it.  Refused here instead.
        const int bnt = cfg == CFG_SMALL ? 0 : conv_shape(cfg).BNT();
        if (cfg != CFG_SMALL && (bnt <= 0 || key[6] <= 0 || key[6] % bnt))
            return fail(h, "mc_tune_import: the %d-column tile of shape id %d does not divide CoutP = %d of its entry", bnt, cfg, key[6]);
        entries.emplace_back(std::move(key), cfg);
    }
    for (auto &e : entries) h->tuned[e.first] = e.second;
    return (int)entries.size();
}

int mc_set_local_maximum_kernel(mc_handle *h, int kernel) {
    if (!h) return -1;
    // max_pool2d(heat, k, stride 1, padding (k - 1) / 2) has the heat map's size for odd k only: with an even k the
    // reference's `hmax == heat` (utils/tensor_ops.py:19-20) does not broadcast and raises
    if (kernel < 1 || kernel > 31 || kernel % 2 == 0)
        return fail(h, "mc_set_local_maximum_kernel: the window must be odd, 1 .. 31 (got %d)", kernel);
    h->lm_kernel = kernel;
    return 0;
}

int mc_set_precision(mc_handle *h, int mode) {
    if (!h) return -1;
    // (mode 4 of round 4 -- mode 3 on activations stored pre-split, DMA-staged -- was retired in round 5: slower in the step,
    //  and its weight gradients were not bit-reproducible beside the weight-gradient stream)
    if (mode < 0 || mode > 3)
        return fail(h, "mc_set_precision: mode must be 0 (fp32 MFMA), 1 (bf16 MFMA operands), 2 (fp32 emulated by a 3-way bf16 "
                       "split) or 3 (fp32 emulated by a 2-way fp16 split)");
    if (mode == h->prec) return 0;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipDeviceSynchronize());
    h->prec = mode;
    for (auto &kv : h->plans) kv.second->mem.release();
    h->plans.clear();
    h->bind_gen++;          // the train plan bakes the precision into its launches: rebuilt on next use
    h->pack_clean = false;  // bf16 panels are packed by the next mc_pack_params
    h->packed = false;
    return 0;
}

// ---------------------------------------------------------------------------- introspection
int mc_train_query_workspace(mc_handle *h, int B, int H, int W, int head_only, size_t *bytes);   // mc_train_plan.hip

int mc_query_workspace(mc_handle *h, int B, int H, int W, int mode, size_t *bytes) {
    if (!h || !bytes) return -1;
    if (B < 1 || H < 32 || W < 32 || (H % 32) || (W % 32)) return fail(h, "mc_query_workspace: B >= 1, H and W multiples of 32");
    if (mode == 0) {
        if (!h->packed) return fail(h, "mc_query_workspace: bind all parameters and call mc_pack_params first");
        auto it = h->plans.find(std::make_tuple(B, H, W));
        if (it != h->plans.end()) { *bytes = it->second->mem.bytes; return 0; }
        h->dry_alloc = true; h->dry_next = 0;
        (void)get_plan(h, B, H, W);
        h->dry_alloc = false;
        *bytes = h->dry_next;
        return *bytes ? 0 : -1;
    }
    if (mode == 1 || mode == 2) return mc_train_query_workspace(h, B, H, W, mode == 2, bytes);
    return fail(h, "mc_query_workspace: mode %d (0 inference forward, 1 train step, 2 heads-only train step)", mode);
}

size_t mc_workspace_bytes(mc_handle *h) {
    if (!h) return 0;
    size_t n = h->params.bytes + (3 * h->decode_filt_n + h->decode_count_n) * sizeof(float) + h->train_bytes +
               h->nms_ws_words * sizeof(unsigned long long);
    for (auto &kv : h->plans) n += kv.second->mem.bytes;
    return n;
}

int mc_forward_cost(mc_handle *h, int B, int H, int W, double flops[2], double bytes[2]) {
    if (!h) return -1;
    if (!h->packed) return fail(h, "mc_forward_cost: pack parameters first");
    HIPCHK(h, hipSetDevice(h->device));
    Plan *pl = get_plan(h, B, H, W);
    if (!pl) return -1;
    double f[2] = {0, 0}, b[2] = {0, 0};
    for (const Op &op : pl->ops) {
        const int k = op.kind == OP_CONV ? 0 : 1;
        f[k] += op.flops;
        b[k] += op.bytes;
    }
    if (flops) { flops[0] = f[0]; flops[1] = f[1]; }
    if (bytes) { bytes[0] = b[0]; bytes[1] = b[1]; }
    return 0;
}

int mc_profile_forward(mc_handle *h, int iters, float out_ms[3], int out_n[3], void *stream) {
    if (!h) return -1;
    Plan *pl = h->last_plan;
    if (!pl) return fail(h, "mc_profile_forward: run mc_forward_infer first");
    if (iters < 1) iters = 1;
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t nops = pl->ops.size();
    std::vector<hipEvent_t> ev(nops + 1);
    for (auto &e : ev) HIPCHK(h, hipEventCreate(&e));
    double acc_conv = 0, acc_other = 0, acc_all = 0;
    int n_conv = 0, n_other = 0;
    for (int it = 0; it < iters; ++it) {
        HIPCHK(h, hipEventRecord(ev[0], st));
        for (size_t i = 0; i < nops; ++i) {
            if (run_op(h, pl->ops[i], st)) return -1;
            HIPCHK(h, hipEventRecord(ev[i + 1], st));
        }
        HIPCHK(h, hipEventSynchronize(ev[nops]));
        n_conv = n_other = 0;
        for (size_t i = 0; i < nops; ++i) {
            float ms = 0;
            HIPCHK(h, hipEventElapsedTime(&ms, ev[i], ev[i + 1]));
            if (pl->ops[i].kind == OP_CONV) { acc_conv += ms; ++n_conv; } else { acc_other += ms; ++n_other; }
            if (it == 0 && std::getenv("MONOCON_HIP_PROFILE_DUMP")) {       // measurement aid: one line per op of the eval plan
                const Op &o = pl->ops[i];
                if (o.kind == OP_CONV)
                    std::fprintf(stderr, "fprof %zu conv k%d s%d %4d -> %-4d (%d src) %3dx%-4d res %d cfg %3d  ms %.4f  gflop %.2f  TF(fp32-eq) %.1f\n", i, o.cp.ks,
                                 o.cp.stride, o.cp.a.Cin, o.cp.a.Cout, o.cp.a.nsrc, o.cp.a.Hout, o.cp.a.Wout, o.cp.a.res != nullptr, o.cp.a.cfg, ms, o.flops * 1e-9,
                                 o.flops / (ms * 1e-3) * 1e-12);
                else
                    std::fprintf(stderr, "fprof %zu kind %d  ms %.4f  mb %.1f\n", i, (int)o.kind, ms, o.bytes * 1e-6);
            }
        }
        float ms = 0;
        HIPCHK(h, hipEventElapsedTime(&ms, ev[0], ev[nops]));
        acc_all += ms;
    }
    for (auto &e : ev) (void)hipEventDestroy(e);
    if (out_ms) { out_ms[0] = (float)(acc_conv / iters); out_ms[1] = (float)(acc_other / iters); out_ms[2] = (float)(acc_all / iters); }
    if (out_n) { out_n[0] = n_conv; out_n[1] = n_other; out_n[2] = (int)nops; }
    return 0;
}

}  // extern "C"
