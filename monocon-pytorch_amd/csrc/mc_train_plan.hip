// Train-step plan: train-mode forward (BatchNorm batch statistics, running-stat updates,
// targets, losses) and the full backward pass, as two lists of kernel launches built once per
// input shape and replayed on the caller's stream.
//
// Replaces what autograd does for the reference's `_, loss_dict = self.model(data_dict);
// total_loss.backward()` (engine/monocon_engine.py:84-86): the graph here is static, gradients
// of tensors with several consumers (tree children, residuals, neck skips) accumulate in place
// through the fused conv's residual input, and every conv uses the MFMA dgrad (= the forward
// kernel on transposed/flipped panels) and the MFMA split-K wgrad.
#include <atomic>
#include <deque>
#include <functional>

#include "mc_internal.h"

using namespace mc;

namespace {

using Fn = std::function<int(mc_handle *, hipStream_t)>;

// ---- the planner's switches.  CONTRACT: a switch is read from the environment when a train plan is built (the dry build
// of mc_query_workspace included) -- by read_switches(), once, and nowhere else; the plan keeps its copy, so a plan never
// changes behaviour after its build and two plans of one process may differ.  Why a default is what it is stands next to
// the branch that tests the switch.
struct PlanSwitches {
    long long lazy_z;           // bit mask: which post-BatchNorm activations are never stored (TB::conv_bn)
    long long lazy_min;         // elements per image from which a ReLU'd map with conv consumers is lazy
    long long lazy_feat;        // the neck's last node lazy like the others
    long long zbits;            // residual layers leave their ReLU mask bit-packed
    long long grad_pool;        // gradient maps from a recycling pool (TB::g_acquire)
    long long grad_pool_cool;   // head start of a returned buffer, in younger buffers of its size
    long long head_dx_fuse;     // the heads' masked gradient is never stored
    long long head_zskip;       // 0 / 1 / 2: the heads' backward skips tiles whose raw gradient is all zero (2: not in head_dx)
    long long dgrad_s2_thin;    // level1's stride-2 data gradient in one pass
    long long stem_fuse;        // the stem's weight gradient forms dY on the fly
    long long bm_epilogue;      // 0 / 1 / <pixels per image>: BatchNorm-backward reductions in the data gradient's epilogue
    long long wres_bwd;         // 0 / 1 / 2: the weight-resident conv kernel in the backward
    long long dual_stream;      // weight gradients on a second stream
    int side_sync_lo = 0, side_sync_hi = 0;     // MONOCON_HIP_SIDE_SYNC=lo:hi (debugging): the caller's stream waits for side steps lo <= k < hi
    bool plan_debug = false;    // MONOCON_HIP_PLAN_DEBUG (set at all): the build prints its decisions to stderr, one "[plan]" line each
};
const struct { const char *name; long long PlanSwitches::*field; long long def; } SWITCH_TABLE[] = {
    {"MONOCON_HIP_LAZY_Z", &PlanSwitches::lazy_z, 3},
    {"MONOCON_HIP_LAZY_MIN", &PlanSwitches::lazy_min, 900000},
    {"MONOCON_HIP_LAZY_FEAT", &PlanSwitches::lazy_feat, 0},
    {"MONOCON_HIP_ZBITS", &PlanSwitches::zbits, 1},
    {"MONOCON_HIP_GRAD_POOL", &PlanSwitches::grad_pool, 1},
    {"MONOCON_HIP_GRAD_POOL_COOL", &PlanSwitches::grad_pool_cool, 2},
    {"MONOCON_HIP_HEAD_DX_FUSE", &PlanSwitches::head_dx_fuse, 1},
    {"MONOCON_HIP_HEAD_ZSKIP", &PlanSwitches::head_zskip, 1},
    {"MONOCON_HIP_DGRAD_S2_THIN", &PlanSwitches::dgrad_s2_thin, 1},
    {"MONOCON_HIP_STEM_FUSE", &PlanSwitches::stem_fuse, 1},
    {"MONOCON_HIP_BM_EPILOGUE", &PlanSwitches::bm_epilogue, 1},
    {"MONOCON_HIP_WRES_BWD", &PlanSwitches::wres_bwd, 0},
    {"MONOCON_HIP_DUAL_STREAM", &PlanSwitches::dual_stream, 1},
};
PlanSwitches read_switches() {
    PlanSwitches sw{};
    std::string changed;
    for (const auto &d : SWITCH_TABLE) {
        const char *e = std::getenv(d.name);
        sw.*d.field = e ? std::atoll(e) : d.def;
        if (sw.*d.field != d.def) changed += std::string(" ") + d.name + "=" + std::to_string(sw.*d.field);
    }
    if (const char *e = std::getenv("MONOCON_HIP_SIDE_SYNC")) {
        if (std::sscanf(e, "%d:%d", &sw.side_sync_lo, &sw.side_sync_hi) != 2) sw.side_sync_lo = sw.side_sync_hi = 0;
        if (sw.side_sync_lo < sw.side_sync_hi) changed += std::string(" MONOCON_HIP_SIDE_SYNC=") + e;
    }
    sw.plan_debug = std::getenv("MONOCON_HIP_PLAN_DEBUG") != nullptr;
    if (sw.plan_debug && !changed.empty()) fprintf(stderr, "[plan] switches off their defaults:%s\n", changed.c_str());
    return sw;
}

struct PoolBwdArgs {       // a max-pool backward launch (stable address: bn_backward may still attach `stats`)
    const float *x, *dout, *la, *lb;
    float *dx, *stats;
    int B, H, W, C, acc;
};

// The launch that wrote a gradient map LAST, when it is of a kind that sees the COMPLETE gradient and can take over the
// reductions of the BatchNorm backward (TB::bn_backward); NONE for every other writer.  Set by TB::wrote() only.
struct LastWriter {
    enum Kind { NONE, DGRAD_CONV, POOL_BWD, DECONV_BWD } kind = NONE;
    union {
        ConvPlan *conv;           // a generic stride-1 data-gradient conv: its epilogue masks the gradient and leaves the partials
        PoolBwdArgs *pool;        // a max-pool backward that accumulated into the map (launch_maxpool2_bwd's stats_partial)
        float **deconv_stats;     // the fused depthwise-deconv backward of the map's only consumer: where to attach `stats`
    };
    LastWriter() : conv(nullptr) {}
    LastWriter(ConvPlan *c) : kind(c ? DGRAD_CONV : NONE), conv(c) {}
    LastWriter(PoolBwdArgs *p) : kind(p ? POOL_BWD : NONE), pool(p) {}
    LastWriter(float **s) : kind(s ? DECONV_BWD : NONE), deconv_stats(s) {}
};

struct TNode {
    Tensor t;
    float *g = nullptr;
    bool ginit = false, needs_grad = true;
    LastWriter last;
    // (t may be a LAZY activation, Tensor::la: TB::materialise() turns such a node into a stored one -- an affine_act pass
    // appended to the forward -- for a consumer that cannot form it)
};

enum RecKind { REC_STEM, REC_CONV, REC_POOL, REC_DECONV, REC_HEAD };
struct Rec {
    RecKind kind;
    ConvLayer *L = nullptr;
    DeconvLayer *D = nullptr;
    std::vector<int> srcs;
    int res = -1, z = -1, in = -1;
    bool relu = true, dead = false;
    Tensor y;
    float *mean = nullptr, *rstd = nullptr;
    float *ca = nullptr, *cb = nullptr;   // forward BN coefficients z = act(ca*y + cb (+ res))
    unsigned *zbits = nullptr;            // residual layers: the ReLU mask of z, bit-packed by the forward (ConvArgs::bm_zbits)
    std::string bn;
};

// One step of the backward pass, in the order the steps are enqueued (TB::push_bwd is the only way one is appended).
enum BwdStream { ON_MAIN, ON_SIDE };
struct BwdStep {
    Fn fn;
    // ON_SIDE: the step only produces weight gradients (nothing downstream in the backward reads them) and runs on the
    // plan's second stream: MFMA-bound wgrad overlaps the HBM-bound BN passes and the tails of the dgrad chain
    BwdStream stream = ON_MAIN;
    // gradient-map pool (TB::g_acquire): this step is the first writer of a recycled buffer whose previous content was
    // read by side step `wait` (index in TrainState::bwd; -1: nothing to wait for)
    int wait = -1;
    // data parallelism: the gradient bucket (mc_internal.h) that is complete once this step has been enqueued, or -1
    int bucket = -1;
    bool feat_dgrad = false;         // head-only plan: the data gradient into the external feat node (TrainState::skip_feat_dgrad)
    bool img_dgrad = false;          // the stem's data gradient: runs only in a backward that asked for the image gradient (TrainState::gimg_ext)
    hipEvent_t ready = nullptr;      // side step: everything it reads is complete at this point of the caller's stream
    hipEvent_t fin = nullptr;        // side step some later step waits for: it has finished
};

}  // namespace

struct TrainState {
    int B = 0, H = 0, W = 0;
    unsigned long long bind_gen = 0;
    PlanSwitches sw{};
    PlanMem mem;
    std::vector<TNode> nodes;
    std::vector<Rec> recs;
    std::vector<Fn> fwd;
    std::vector<BwdStep> bwd;
    std::deque<ConvPlan> dgrads;     // data-gradient launches (stable addresses: bn_backward may still patch them)
    std::deque<PoolBwdArgs> pool_bwds;
    std::deque<float *> deconv_stats;      // per fused deconv backward: its statistics buffer (null until bn_backward attaches one)
    hipStream_t side = nullptr;      // the weight-gradient stream
    hipEvent_t side_done = nullptr;
    bool dual = true;                // side steps run on `side` (false: MONOCON_HIP_DUAL_STREAM=0, or the stream / an event could not be created)
    unsigned *img_amax = nullptr;      // mode 3: max |image| slot (written by the forward stem, read by its weight gradient)
    mc::PackBatch pack_batch;        // the data-gradient panels, refreshed from the master weights in one grid per forward
    std::vector<Fn> pack_fns;
    // per-call external pointers
    const float *img = nullptr;
    mc_labels labels{};
    float *preds[10] = {nullptr};
    float *losses = nullptr;
    const float *grad_losses = nullptr;
    // caller's gradients wrt the ten prediction maps (mc_backward_pred_grads): set for one backward_impl call only
    const float *grad_preds[10] = {nullptr};
    int pad_h = 0, pad_w = 0, max_objs = 30;
    // head-only plan (mc_head_forward_train): the neck output comes in as an external NCHW tensor, its gradient
    // goes out the same way
    bool head_only = false;
    const float *feat_ext = nullptr;
    float *gfeat_ext = nullptr;
    bool skip_feat_dgrad = false;    // head-only plan, mc_head_backward(grad_feat = NULL)
    // mc_backward_image_grad: where the gradient of the image goes, (B,3,H,W) NCHW.  Caller-owned like gfeat_ext: set by the
    // entry point for ONE backward and cleared by the step that wrote it
    float *gimg_ext = nullptr;
    // plan-owned
    mc_targets targets{};
    float *dpred[10] = {nullptr};
    bool ok = true;
};

// generation of the activations the plan currently holds: bumped by every mc_forward_train on the handle (the plan
// keeps ONE set of saved activations, so mc_backward always differentiates the LATEST forward)
static std::atomic<unsigned long long> g_train_generation{0};

static void train_free(TrainState *t) {
    if (!t) return;
    for (const BwdStep &s : t->bwd) {
        if (s.ready) (void)hipEventDestroy(s.ready);
        if (s.fin) (void)hipEventDestroy(s.fin);
    }
    if (t->side_done) (void)hipEventDestroy(t->side_done);
    if (t->side) (void)hipStreamDestroy(t->side);
    t->mem.release();
    delete t;
}

namespace {

struct TB {   // train plan builder
    mc_handle *h;
    TrainState *ts;
    PlanAlloc mem{h, ts->mem, ts->ok, 1, 1024};
    const PlanSwitches &sw = ts->sw;
    const int B = ts->B, H = ts->H, W = ts->W, fh = H / 4, fw = W / 4, HW = fh * fw;

    float *alloc(size_t n) { return mem.alloc(n); }
    unsigned *slot() { return mem.slot(); }
    unsigned *w_slot(const float *w_master) {
        if (h->prec != 3) return nullptr;
        auto it = h->w_amax_of.find(w_master);
        if (it == h->w_amax_of.end()) { ts->ok = false; h->err = "train plan: no max-|w| slot for a master weight"; return nullptr; }
        return it->second;
    }

    // ---- backward steps
    int cur_bucket = 0;       // gradient bucket of the layer group whose steps are being pushed (build_train keeps the last of each)
    int pending_wait = -1;    // g_acquire() handed out a recycled buffer: the next step pushed is its first writer
    int push_bwd(Fn fn, BwdStream stream = ON_MAIN) {
        BwdStep s;
        s.fn = std::move(fn); s.stream = stream; s.bucket = cur_bucket; s.wait = pending_wait;
        pending_wait = -1;
        ts->bwd.push_back(std::move(s));
        return (int)ts->bwd.size() - 1;
    }

    // ---- gradient maps.  The backward steps are BUILT in the order they run, so the life of a map's gradient is known
    // while building: it starts at its first writer (a data-gradient conv, a pooling / deconv backward, the residual
    // share of an affine pass) and ends with the layer that produced the map (whose affine pass turns dZ into dY in
    // place; dY is then read by that layer's data- and weight-gradient launches).  Buffers are handed out at the first
    // write and returned after the producing layer, oldest first; a buffer whose last reader ran on the weight-gradient
    // stream carries that step's index, and its next first writer waits for it (BwdStep::wait).
    // MONOCON_HIP_GRAD_POOL=0: one private buffer per map.  Measured at B=32 (one session, scratch/ab/pool_ab.sh):
    // 37.7 GB / 59.77 ms without the pool, 32.9 GB / 60.09 ms recycling immediately, 33.8 GB / 59.89 ms with two buffers
    // of head start (the default).
    struct PoolBuf { float *p; int side_step; };
    std::map<size_t, std::deque<PoolBuf>> gpool;
    float *g_acquire(int node) {
        TNode &n = ts->nodes[node];
        if (n.g) return n.g;
        const size_t ne = n.t.numel();
        auto &q = gpool[ne];
        // a returned buffer is handed out again only once MONOCON_HIP_GRAD_POOL_COOL younger ones of its size wait behind it:
        // the weight gradient that still reads it has then had that many layers of head start, and the wait is a formality
        if (sw.grad_pool && (long long)q.size() > sw.grad_pool_cool) {
            const PoolBuf b = q.front();
            q.pop_front();
            pending_wait = std::max(pending_wait, b.side_step);
            n.g = b.p;
        } else {
            n.g = alloc(ne);
        }
        return n.g;
    }
    // the map's gradient has had its last reader: side step `side_step` (-1: a step on the caller's stream)
    void g_release(int node, int side_step) {
        TNode &n = ts->nodes[node];
        if (!sw.grad_pool || !n.g) return;
        gpool[n.t.numel()].push_back({n.g, side_step});
        n.g = nullptr;
    }
    // EVERY writer of a gradient map calls this after pushing its step(s): `by` names the launch if it can carry the
    // BatchNorm-backward reductions of the map (see LastWriter), and is left out by every other writer
    void wrote(int node, LastWriter by = {}) {
        ts->nodes[node].ginit = true;
        ts->nodes[node].last = by;
    }

    int n_lazy = 0, n_materialised = 0;
    // a consumer that cannot form a lazy activation on load: store it after all (one element-wise pass appended to the
    // forward at this point of the build -- i.e. before the consumer's own launch -- and the node is an ordinary one from
    // here on; earlier consumers keep reading y).  Its max-|z| slot already holds bn_finalize's bound.
    void materialise(int node_i) {
        TNode &n = ts->nodes[node_i];
        if (!n.t.la) return;
        float *z = alloc(n.t.numel());
        const float *y = n.t.p, *la = n.t.la, *lb = n.t.lb;
        const int B = n.t.B, C = n.t.C, rl = n.t.lrelu ? 1 : 0;
        const size_t rows = (size_t)n.t.H * n.t.W;
        ts->fwd.push_back([=](mc_handle *hh, hipStream_t st) {
            HIPCHK(hh, launch_affine_act(y, la, lb, nullptr, B, rows, C, 0, rl, z, st, nullptr));
            return 0;
        });
        if (sw.plan_debug)
            fprintf(stderr, "[plan] lazy node %d (%d ch %dx%d) materialised for a consumer that cannot form it on load\n", node_i, C, n.t.H, n.t.W);
        n.t.p = z; n.t.la = n.t.lb = nullptr;
        ++n_materialised;
    }
    // a conv (or its weight gradient) forms ReLU'd lazy maps only: any other lazy source is stored first.  Returns the
    // sources as the launch descriptions take them (valid until the next node() call)
    std::vector<const Tensor *> conv_sources(const std::vector<int> &srcs) {
        std::vector<const Tensor *> t;
        for (int s_ : srcs) {
            if (ts->nodes[s_].t.la && !ts->nodes[s_].t.lrelu) materialise(s_);
            t.push_back(&ts->nodes[s_].t);
        }
        return t;
    }
    int node(int B, int H, int W, int C, bool needs_grad = true, bool storage = true) {
        TNode n;
        n.t.B = B; n.t.H = H; n.t.W = W; n.t.C = C;
        n.t.p = storage ? alloc(n.t.numel()) : nullptr;
        n.t.amax = slot();
        n.needs_grad = needs_grad;
        if (needs_grad && !sw.grad_pool) n.g = alloc(n.t.numel());
        ts->nodes.push_back(n);
        return (int)ts->nodes.size() - 1;
    }
    // bound tensors, checked by mc_param: a missing or mismatched one fails the build
    void *bound(const std::string &name, int64_t numel, int dtype) {
        void *p = mc_param(h, name, numel, dtype);
        if (!p) ts->ok = false;
        return p;
    }
    float *P(const std::string &name, int64_t numel) { return static_cast<float *>(bound(name, numel, MC_F32)); }
    float *G(const std::string &name, int64_t numel) { return P(name + "#grad", numel); }
    long long *NBT(const std::string &name) { return static_cast<long long *>(bound(name, 1, MC_I64)); }

    // reserved: whether the partial list gets a fold buffer, i.e. partial_fold + the double finalise run (launch_bn_finalize)
    double *fold_scratch(int nb, int C, bool *reserved = nullptr) {
        const size_t nd = partial_fold_doubles(nb, C);
        if (reserved) *reserved = nd != 0;
        return nd ? reinterpret_cast<double *>(alloc(nd * 2)) : nullptr;
    }

    // ---------------------------------------------------------------- forward pieces
    // returns whether the partials are folded first (fold_scratch)
    bool bn_train_ops(const Tensor &y, const float *stats, int nb, int cstride, const std::string &bn, float eps,
                      float mom, float *a, float *b, float *mean, float *rstd, const unsigned *ymax = nullptr,
                      unsigned *zmax = nullptr, int zrelu = 1) {
        const int C = y.C;
        float *g = P(bn + ".weight", C), *be = P(bn + ".bias", C), *rm = P(bn + ".running_mean", C), *rv = P(bn + ".running_var", C);
        long long *nbt = NBT(bn + ".num_batches_tracked");
        const double n = (double)y.B * y.H * y.W;
        bool folds = false;
        double *fold = fold_scratch(nb, C, &folds);
        ts->fwd.push_back([=](mc_handle *hh, hipStream_t st) {
            HIPCHK(hh, launch_bn_finalize(stats, nb, cstride, n, C, rm, g, be, eps, mom, rm, rv, nbt, a, b, mean, rstd, st, fold,
                                          ymax, zmax, zrelu));
            return 0;
        });
        return folds;
    }

    // the max-|x| slots start every forward at zero: their producers only raise them (mode 3; the first step of the forward)
    void zero_amax_slots() {
        if (h->prec != 3) return;
        (void)slot();
        --ts->mem.amax_used;
        ts->fwd.push_back([ts = ts](mc_handle *hh, hipStream_t st) {
            HIPCHK(hh, hipMemsetAsync(ts->mem.amax_arena, 0, (size_t)ts->mem.amax_used * AMAX_WORDS * sizeof(unsigned), st));
            return 0;
        });
    }

    // the heads on their own (MonoConDenseHeads.forward_train, monocon_heads.py:150-157): the neck output is an
    // external NCHW tensor, copied into the plan's NHWC node; its gradient is copied out after the backward
    int external_feat() {
        const int feat = node(B, fh, fw, 64, true);
        float *fp = ts->nodes[feat].t.p;
        unsigned *fmax = ts->nodes[feat].t.amax;
        ts->fwd.push_back([=, ts = ts, B = B, fh = fh, fw = fw](mc_handle *hh, hipStream_t st) {
            HIPCHK(hh, launch_nchw_to_nhwc(ts->feat_ext, B, 64, fh, fw, fp, st));
            if (fmax) HIPCHK(hh, launch_absmax(fp, (size_t)B * fh * fw * 64, fmax, st));
            return 0;
        });
        return feat;
    }

    // BatchNorm of the raw conv output r.y from its statistics partials, then the activation: lazy (never stored: the node
    // points at y and carries the coefficients; ymax = the slot where the conv left max |y|), or one element-wise pass
    // (returns bn_train_ops' answer)
    bool bn_act(Rec &r, const float *stats, int nb, int cstride, bool lazy, const unsigned *ymax) {
        const int B = r.y.B, C = r.y.C, res = r.res, rl = r.relu;
        float *ca = alloc(C), *cb = alloc(C);
        r.ca = ca; r.cb = cb;
        r.mean = alloc(C); r.rstd = alloc(C);
        const bool folds = bn_train_ops(r.y, stats, nb, cstride, r.bn, 1e-5f, 0.1f, ca, cb, r.mean, r.rstd, ymax, lazy ? ts->nodes[r.z].t.amax : nullptr, rl);
        if (lazy) {
            TNode &zn = ts->nodes[r.z];
            zn.t.p = r.y.p; zn.t.la = ca; zn.t.lb = cb; zn.t.lrelu = r.relu;
            ++n_lazy;
        } else if (!r.dead) {
            const TNode &rn = ts->nodes[res >= 0 ? res : 0];
            const float *yp = r.y.p, *rp = res >= 0 ? rn.t.p : nullptr;
            const float *ra = res >= 0 ? rn.t.la : nullptr, *rb = res >= 0 ? rn.t.lb : nullptr;     // the residual may be lazy
            const int rrelu = (res >= 0 && rn.t.lrelu) ? 1 : 0;
            float *zp = ts->nodes[r.z].t.p;
            unsigned *zmax = ts->nodes[r.z].t.amax;
            const size_t rows = (size_t)r.y.H * r.y.W;
            // a residual layer's ReLU mask cannot be recomputed from y alone: the forward leaves it bit-packed for the
            // backward-statistics epilogue of the data gradient that completes this map's gradient (1/32 of the bytes of z;
            // MONOCON_HIP_ZBITS=0: that epilogue reads z)
            unsigned *zb = (sw.zbits && res >= 0 && rl && C % 32 == 0) ? reinterpret_cast<unsigned *>(alloc((size_t)B * rows * (C / 32))) : nullptr;
            r.zbits = zb;
            ts->fwd.push_back([=](mc_handle *hh, hipStream_t st) {
                HIPCHK(hh, launch_affine_act(yp, ca, cb, rp, B, rows, C, 0, rl, zp, st, zmax, ra, rb, rrelu, zb));
                return 0;
            });
        }
        return folds;
    }

    // MONOCON_HIP_PLAN_DEBUG: which launch leaves a layer's forward statistics partials (the conv kernel's name, or the
    // stem's), how many rows of them, which bn_finalize build finishes them (folds: bn_act's answer), and what becomes of z
    void say_forward(const Rec &r, const char *producer, int nb, bool folds, bool lazy) {
        if (!sw.plan_debug) return;
        fprintf(stderr, "[plan] forward %-40s node %3d  statistics by %-10s %6d partial rows  finalize %s  z %s\n", r.bn.c_str(), r.z,
                producer, nb, folds ? "double" : "float", r.dead ? "dead" : (lazy ? "lazy" : "stored"));
    }

    // ---- stem (raw conv -> batch stats -> normalise + ReLU)
    void stem() {
        Rec stem;
        stem.kind = REC_STEM; stem.bn = "backbone.base_layer.1"; stem.relu = true;
        stem.y.B = B; stem.y.H = H; stem.y.W = W; stem.y.C = 16;
        stem.y.p = alloc(stem.y.numel());
        // (mode 3 with the fp16-pipe stem, which leaves max |y|: the stem's activation is lazy like conv_bn's, TNode::la)
        const bool stem_lazy = h->prec == 3 && stem_f16_enabled() && (sw.lazy_z & 1);
        stem.z = node(B, H, W, 16, true, !stem_lazy);
        float *ones16 = alloc(16), *zeros16 = alloc(16);
        std::vector<float> one(16, 1.f);
        if (!h->dry_alloc && hipMemcpy(ones16, one.data(), 64, hipMemcpyHostToDevice) != hipSuccess) ts->ok = false;
        // mode 3: the fp16-pipe stem leaves the (sum, sum of squares) partials per output row itself; the other modes reduce
        // the raw map in a second pass
        const bool fused_stats = h->prec == 3 && stem_f16_enabled();
        const int nb = fused_stats ? B * H : chan_reduce_blocks(B, H * W);
        float *partial = alloc((size_t)nb * 16 * 2), *yp = stem.y.p, *rm = P(stem.bn + ".running_mean", 16);
        unsigned *imax = fused_stats ? slot() : nullptr;     // max |image|, left by the forward stem for its weight gradient
        ts->img_amax = imax;
        unsigned *ymax = fused_stats ? slot() : nullptr;     // max |raw stem output|: operand-scale bound of the fused weight gradient
        stem.y.amax = ymax;
        const float *sw_ = h->stem_w;
        ts->fwd.push_back([=, ts = ts, B = B, H = H, W = W](mc_handle *hh, hipStream_t st) {
            if (fused_stats) {
                HIPCHK(hh, launch_stem_f16(ts->img, B, H, W, sw_, ones16, zeros16, yp, st, 0, ymax, partial, rm, imax));
            } else {
                HIPCHK(hh, launch_stem(ts->img, B, H, W, sw_, ones16, zeros16, yp, st, 0, hh->prec));
                HIPCHK(hh, launch_chan_reduce(yp, nullptr, nullptr, rm, B, H * W, 16, 0, 0, partial, 16, st));
            }
            return 0;
        });
        const bool folds = bn_act(stem, partial, nb, 16, stem_lazy, stem_lazy ? ymax : nullptr);
        say_forward(stem, fused_stats ? "stem_f16" : "chan_reduce", nb, folds, stem_lazy);
        ts->recs.push_back(stem);
    }

    int conv_bn(const NetStep &s) {
        ConvLayer &Lr = mc_conv_layer(h, s.name, ts->ok);
        const std::vector<int> &srcs = s.srcs;
        const int res = s.res;
        // the neck's LAST node is `feat` (NetStep::never_lazy): its consumers are the fused 64 -> 576 head conv and that conv's
        // weight gradient, the two longest launches of the step -- formed on load it cost them 0.15 + 0.22 ms (alone) to save a
        // 0.095 ms pass: stored (MONOCON_HIP_LAZY_FEAT=1: lazy like the other nodes)
        const bool relu = s.relu, dead = s.dead, never_lazy = s.never_lazy && !sw.lazy_feat;
        const Tensor s0 = ts->nodes[srcs[0]].t;   // by value: node() below may reallocate ts->nodes
        const int B = s0.B;
        const int Ho = conv_out_dim(s0.H, Lr.ks, Lr.stride), Wo = conv_out_dim(s0.W, Lr.ks, Lr.stride);
        Rec r;
        r.kind = REC_CONV; r.L = &Lr; r.srcs = srcs; r.res = res; r.relu = relu; r.dead = dead; r.bn = Lr.bn;
        r.y.B = B; r.y.H = Ho; r.y.W = Wo; r.y.C = Lr.cout;
        r.y.p = alloc(r.y.numel());
        // lazy output: BatchNorm (+ ReLU) without residual in mode 3 (the convs of every kernel family leave max |y|).
        // MONOCON_HIP_LAZY_Z (bit mask, default 3): 1: the BatchNorm + ReLU outputs without residual (stem, level0 / level1,
        // BasicBlock conv1, Root, neck proj / node); 2: a Tree's `project` branch (BatchNorm without ReLU, consumed as the
        // residual of the block beside it); 0: every activation is stored.  Outputs of a residual add are always stored.
        // A lazy map costs its MFMA-kernel consumers one fma + one v_med3 per staged element (measured, B = 32: a 3x3 weight
        // gradient +0.03 ms, a conv +0.01 ms per launch) and saves one element-wise pass over the map (2 x its bytes at ~5.3
        // TB/s): worth it for the large maps only.  MONOCON_HIP_LAZY_MIN: elements per image from which a ReLU'd map whose
        // consumers are convolutions is lazy; maps with element-wise consumers only (neck proj -> deconv, project -> residual)
        // always are.  The default sits between the 256-channel 24x80 maps (491 520 elements: stored) and the 128-channel maps
        // of the quarter-resolution level (983 040 at the benchmark's width 1280, 958 464 at KITTI's 1248: lazy): with 983 040
        // itself a KITTI batch lost those maps and 0.3 ms per step (48.66 -> 48.35 ms at 384x1248, two runs each).
        const bool lazy = !dead && !never_lazy && res < 0 && h->prec == 3 && (sw.lazy_z & (relu ? 1 : 2)) != 0 &&
                          (!relu || s.elementwise_consumers || (long long)Ho * Wo * Lr.cout >= sw.lazy_min);
        r.z = dead ? -1 : node(B, Ho, Wo, Lr.cout, true, !lazy);
        ConvPlan cp{};
        ConvArgs &a = cp.a;
        const std::vector<const Tensor *> xs = conv_sources(srcs);
        if (!conv_fwd_args(cp, Lr, xs, h->prec)) { ts->ok = false; h->err = "train plan: channel mismatch at " + Lr.conv; }
        if (conv_any_lazy(a) && !cp.lazy_ok) {
            for (int s_ : srcs) materialise(s_);
            conv_fwd_args(cp, Lr, xs, h->prec);
        }
        a.out = r.y.p; a.out_ld = Lr.cout;
        unsigned *yslot = lazy ? slot() : nullptr;      // max |y|, left by the conv's epilogue: bn_finalize bounds max |z| with it
        a.amax_out = yslot;
        a.cfg = ts->ok ? mc_choose_conv_cfg(h, cp) : CFG_128x32;
        conv_plan(cp);
        const int chunks = cp.stat_rows;
        float *stats = alloc((size_t)B * chunks * Lr.coutp * 2);
        a.stats = stats;
        a.stat_shift = P(Lr.bn + ".running_mean", Lr.cout);
        conv_plan(cp);
        ts->fwd.push_back([=](mc_handle *hh, hipStream_t st) { HIPCHK(hh, launch_conv(cp, st)); return 0; });
        const bool folds = bn_act(r, stats, B * chunks, Lr.coutp, lazy, yslot);
        static const char *const KERNEL[] = {"fp32", "fp32_ws", "split", "wres", "row", "row_lazy", "thin16"};      // by ConvKernel
        static_assert(sizeof(KERNEL) / sizeof(KERNEL[0]) == CONV_THIN16 + 1 && CONV_FP32 == 0 && CONV_WRES == 3 && CONV_ROW == 4,
                      "one name per ConvKernel, in its order");
        say_forward(r, KERNEL[cp.kernel], B * chunks, folds, lazy);
        ts->recs.push_back(r);
        return r.z;
    }

    int pool(int x) {
        const Tensor t = ts->nodes[x].t;           // by value (see conv_bn)
        if (ts->nodes[x].t.la && !ts->nodes[x].t.lrelu) materialise(x);
        const Tensor tx = ts->nodes[x].t;
        const int o = node(t.B, t.H / 2, t.W / 2, t.C, true);
        ts->nodes[o].t.amax = t.amax;          // max |pool(x)| <= max |x|: the input's slot serves
        const float *ip = tx.p, *la = tx.la, *lb = tx.lb;      // (lazy x: pooled over relu(la * y + lb))
        float *op = ts->nodes[o].t.p;
        const int B = t.B, H = t.H, W = t.W, C = t.C;
        ts->fwd.push_back([=](mc_handle *hh, hipStream_t st) {
            HIPCHK(hh, launch_maxpool2(ip, B, H, W, C, op, st, la, lb));
            return 0;
        });
        Rec r;
        r.kind = REC_POOL; r.in = x; r.z = o;
        ts->recs.push_back(r);
        return o;
    }

    int deconv(DeconvLayer &D, int x) {
        if (ts->nodes[x].t.la && !ts->nodes[x].t.lrelu) materialise(x);
        const Tensor t = ts->nodes[x].t;           // by value (see conv_bn)
        const int o = node(t.B, t.H * 2, t.W * 2, t.C, true);
        const float *ip = t.p, *w = D.wpk, *la = t.la, *lb = t.lb;
        float *op = ts->nodes[o].t.p;
        unsigned *omax = ts->nodes[o].t.amax;
        const int B = t.B, H = t.H, W = t.W, C = t.C;
        ts->fwd.push_back([=](mc_handle *hh, hipStream_t st) {
            HIPCHK(hh, launch_deconv4(ip, B, H, W, C, w, op, st, omax, la, lb));
            return 0;
        });
        Rec r;
        r.kind = REC_DECONV; r.in = x; r.z = o; r.D = &D;
        ts->recs.push_back(r);
        return o;
    }

    // ---------------------------------------------------------------- backward pieces
    // a data-gradient panel (train.h: pack_job_dgrad), refreshed with the plan's other panels before every forward (the
    // precision mode is baked into a plan: mc_set_precision bumps bind_gen)
    const PackJobDesc &pack_job(const float *w, int Cout, int CinTotal, int k, int c_off, int Cs, int CoutPad, int cls) {
        const size_t pn = dgrad_panel_elems(k, cls, CoutPad, Cs);
        float *dst = alloc(pn);
        void *dst16 = panel_has_pieces(h->prec, CoutPad) ? alloc((3 * pn + 1) / 2) : nullptr;     // room for three planes
        ts->pack_batch.add(pack_job_dgrad(w, Cout, CinTotal, k, c_off, Cs, CoutPad, cls, dst, dst16, h->prec, w_slot(w)));
        return ts->pack_batch.jobs.back();
    }

    // dgrad: g_src (+)= conv_s1(dy (optionally dilated), flipped panel)
    void emit_dgrad(const float *w_master, const Tensor &dy, int Cout_fwd, int CinTotal, int ks, int stride, int c_off, int srcnode,
                    int CoutPad) {
        TNode &sn = ts->nodes[srcnode];
        if (!sn.needs_grad) return;
        g_acquire(srcnode);
        // a stride-1 conv over dY with the panel of one output-parity class (-1: the whole flipped kernel), its shape id chosen
        auto dgrad_conv = [&](int cls, ConvPlan &d) {
            const PackJobDesc &p = pack_job(w_master, Cout_fwd, CinTotal, ks, c_off, sn.t.C, CoutPad, cls);
            dgrad_conv_args(d, p, h->prec, dy.p, dy.amax, dy.B, dy.H, dy.W, dy.C, sn.g, sn.t.H, sn.t.W, sn.ginit);
            d.a.cfg = ts->ok ? mc_choose_conv_cfg(h, d) : CFG_128x32;
        };
        if (stride == 2 && ks == 3) {
            // four output-parity classes, each a small stride-1 window conv over dY that scatters to every
            // second pixel of g_src (no zero-dilated copy of dY, 9 instead of 36 tap-MACs per output quad)
            if (2 * dy.H != sn.t.H || 2 * dy.W != sn.t.W) { ts->ok = false; h->err = "train plan: stride-2 dgrad shape mismatch"; }
            // the 32 -> 16 layer at full resolution (level1): all four classes in one pass of its own kernel (conv_thin.hip;
            // MONOCON_HIP_DGRAD_S2_THIN=0: the four launches below)
            if (sw.dgrad_s2_thin && ts->ok && dgrad_s2_thin_ok(h->prec, ks, stride, dy.C, sn.t.C, CinTotal, c_off, dy.amax, w_slot(w_master), dy.H, dy.W)) {
                const float *dyp = dy.p;
                float *gp = sn.g;
                const int B = dy.B, Hd = dy.H, Wd = dy.W, Cd = dy.C, acc = sn.ginit ? 1 : 0;
                const unsigned *dmax = dy.amax, *wmax = w_slot(w_master);
                push_bwd([=](mc_handle *hh, hipStream_t st) {
                    HIPCHK(hh, launch_dgrad_s2_thin(dyp, B, Hd, Wd, Cd, w_master, CinTotal, c_off, gp, acc, dmax, wmax, st));
                    return 0;
                });
                wrote(srcnode);
                return;
            }
            for (int cls = 0; cls < 4; ++cls) {
                ConvPlan d;
                dgrad_conv(cls, d);
                conv_plan(d);
                push_bwd([=](mc_handle *hh, hipStream_t st) { HIPCHK(hh, launch_conv(d, st)); return 0; });
            }
            wrote(srcnode);
            return;
        }
        if (dy.H != sn.t.H || dy.W != sn.t.W) { ts->ok = false; h->err = "train plan: dgrad shape mismatch"; }
        ConvPlan d;
        dgrad_conv(-1, d);
        // The weight-resident kernel (conv_wres.hip) owns its CU -- four waves with the whole register file -- so beside the
        // weight-gradient stream it cannot share one the way the tiled kernels do and the two streams take
        // turns: measured in the step (rocprofv3) a plain 64 -> 64 data gradient takes ~595 us on it against 389 us
        // on conv_bf16_kernel, although it is the faster kernel alone (244 vs 284 us); its backward-statistics twins take
        // 546 us in the step (303 alone).  One-session A/B of the whole step: 52.61 ms without it in the backward, 53.24 ms
        // with the twins on it.  Backward launches therefore keep the tiled kernels.
        // MONOCON_HIP_WRES_BWD: 0 (default) = never in the backward, 1 = the twins (bn_backward sets the flag), 2 = wherever
        // the autotuner chose it
        if (sw.wres_bwd < 2) d.a.cfg &= ~CFG_WRES;
        conv_plan(d);
        ts->dgrads.push_back(d);
        ConvPlan *dp = &ts->dgrads.back();
        push_bwd([=](mc_handle *hh, hipStream_t st) { HIPCHK(hh, launch_conv(*dp, st)); return 0; });
        // (the fp32 row kernel has no backward-statistics epilogue; its fp16-pipe replacement for 16 -> 16 layers has)
        wrote(srcnode, d.bm_ok ? dp : nullptr);
    }

    // the weight gradient of a conv, on the weight-gradient stream: dy is not written again in this step.  Returns its step.
    int emit_wgrad(const std::vector<int> &srcs, const Tensor &dy, int dy_ld, int Cout, int ks, int stride, float *dw) {
        WgradPlan p{};
        const std::vector<const Tensor *> xs = conv_sources(srcs);
        wgrad_args(p, xs, dy, dy_ld, Cout, ks, stride, h->prec);
        if (wgrad_any_lazy(p.a) && !wgrad_lazy_capable(p)) {      // X is read by a kernel that cannot form it: store it after all
            for (int s_ : srcs) materialise(s_);
            wgrad_args(p, xs, dy, dy_ld, Cout, ks, stride, h->prec);
        }
        p.a.partial = alloc(wgrad_partial_floats(p));
        return push_bwd([=](mc_handle *hh, hipStream_t st) { HIPCHK(hh, launch_wgrad(p, dw, st)); return 0; }, ON_SIDE);
    }

    // BN(+ReLU)(+residual) backward, ONE step.  dy: the gradient wrt the raw conv output.  caller_forms_dy: the caller
    // consumes (d, y, coef) itself (the stem, whose dY is read by its weight gradient only) -- honoured on the
    // backward-statistics-epilogue path, where affine_skipped reports it: dy.p is then the masked gradient d, dy.amax max |d|
    struct BnBwd { Tensor dy; float *coef; bool affine_skipped; };
    BnBwd bn_backward(const Rec &r, const std::string &bn, bool caller_forms_dy = false) {
        TNode &zn = ts->nodes[r.z];
        Tensor dy = r.y;
        // dY (the gradient wrt the raw conv output) is written IN PLACE over dZ: the affine pass is elementwise and the
        // gradient of z has no reader after it (the residual branch receives its share in the same pass)
        dy.p = zn.g;
        dy.amax = slot();
        unsigned *dymax = dy.amax;
        const int B = r.y.B, C = r.y.C, rows = r.y.H * r.y.W;
        const float *yp = r.y.p, *gz = zn.g, *zp = zn.t.p, *gamma = P(bn + ".weight", C), *mean = r.mean, *rstd = r.rstd;
        float *dg = G(bn + ".weight", C), *db = G(bn + ".bias", C), *dyp = dy.p;
        float *coef = alloc((size_t)C * 4);
        // ReLU without residual: the mask is recomputed from y (bit-identical to z > 0), z is not read
        const int relu = r.relu ? ((r.res < 0 && r.ca && r.cb) ? 2 : 1) : 0;
        const float *fa = r.ca, *fb = r.cb;
        float *gres = nullptr;
        int gmode = 0;
        if (r.res >= 0 && ts->nodes[r.res].needs_grad) {
            gres = g_acquire(r.res);
            gmode = ts->nodes[r.res].ginit ? 2 : 1;
            wrote(r.res);
        }
        const double n = (double)B * rows;
        // every branch below only decides where the (sum d, sum d*y) partials come from; this pushes the ONE step of the
        // BatchNorm backward: the reduction pass (reduce: no launch of the step left them), bn_bwd_finalize, and the
        // affine pass (dZ -> dY in place, the residual's share; it applies the ReLU mask only after the reduction pass --
        // a launch that leaves the partials has masked the gradient already)
        auto step = [&](float *partial, int nbp, int cstride, bool reduce, bool affine) {
            double *fold = fold_scratch(nbp, C);  // (61 440 partial rows at full resolution: 16 workgroups walking them took 87 us)
            const int arelu = reduce ? relu : 0;
            const float *aa = reduce ? fa : nullptr, *ab = reduce ? fb : nullptr;
            push_bwd([=](mc_handle *hh, hipStream_t st) {
                if (reduce) HIPCHK(hh, launch_chan_reduce(yp, gz, zp, nullptr, B, rows, C, 1, relu, partial, C, st, fa, fb));
                HIPCHK(hh, launch_bn_bwd_finalize(partial, nbp, cstride, n, C, gamma, mean, rstd, dg, db, coef, st, fold));
                if (affine)
                    HIPCHK(hh, launch_affine_bwd(gz, zp, yp, coef, B, (size_t)rows, C, 0, arelu, dyp, gres, gmode, st, aa, ab, nullptr,
                                                 nullptr, dymax));
                return 0;
            });
            return BnBwd{dy, coef, !affine};
        };
        const LastWriter last = zn.last;
        ConvPlan *lp = last.kind == LastWriter::DGRAD_CONV ? last.conv : nullptr;
        ConvArgs *lc = lp ? &lp->a : nullptr;
        // MONOCON_HIP_BM_EPILOGUE: 0 = never take over the reductions in the data gradient's epilogue (always the reduction
        // pass), N > 1 = only for maps of at most N pixels per image
        if (sw.bm_epilogue == 0 || (sw.bm_epilogue > 1 && r.y.H * r.y.W > sw.bm_epilogue)) lc = nullptr;
        if (sw.plan_debug)
            fprintf(stderr, "[plan] bn_backward %-40s %4d ch %4dx%-4d relu %d res %d last-writer-conv %d\n", bn.c_str(), C, r.y.H,
                    r.y.W, relu, r.res >= 0, lc != nullptr);
        if (lc && lc->out == zn.g && lc->Cout == C && lc->out_ld == C && lc->Hout == r.y.H && lc->Wout == r.y.W && !lc->stats) {
            // the gradient of this map was completed by a data-gradient conv: its epilogue masks it and emits the
            // (sum d, sum d*y) partials per 4x8 patch -- no reduction pass, and the affine pass needs no mask
            const int ppi = lp->stat_rows, nbp = B * ppi, cstride = lc->CoutP;   // per 4x8 patch / per row
            float *partial = alloc((size_t)nbp * cstride * 2);
            lc->stats = partial;
            lc->bm_y = yp; lc->bm_z = zp; lc->bm_a = fa; lc->bm_b = fb; lc->bm_relu = relu;
            lc->bm_zbits = relu == 1 ? r.zbits : nullptr;
            // (see emit_dgrad) the twin takes the weight-resident kernel where it is eligible
            const bool try_wres = sw.wres_bwd >= 1 && !(lc->cfg & (CFG_SMALL | CFG_WS | CFG_WRES));
            if (try_wres) lc->cfg |= CFG_WRES;
            conv_plan(*lp);
            if (try_wres && lp->kernel != CONV_WRES) { lc->cfg &= ~CFG_WRES; conv_plan(*lp); }
            if (!lp->ok && ts->ok) { ts->ok = false; h->err = "train plan: no conv kernel carries the backward-statistics epilogue of " + bn; }
            if (sw.plan_debug)
                fprintf(stderr, "[plan]   twin of %-36s cfg %3d  K %4d  Cout %3d  %dx%d  res %d  nsrc %d srcC %d wres %d\n", bn.c_str(), lc->cfg,
                        lc->Cin, lc->Cout, lc->Hout, lc->Wout, lc->res != nullptr, lc->nsrc, lc->src[0].C, (lc->cfg & CFG_WRES) != 0);
            const bool skip_affine = caller_forms_dy && !gres;
            // the epilogue then also leaves max |d| (for the consumer's operand scale); only the coefficients are computed here
            if (skip_affine) lc->amax_out = dymax;      // (no part of the kernel choice)
            return step(partial, nbp, cstride, false, !skip_affine);
        }
        // the gradient of this map was completed by a max-pool backward over a LAZY map (it holds y, forms z for its window
        // comparison anyway): that launch masks the total and leaves the partials -- no reduction pass
        PoolBwdArgs *pl = last.kind == LastWriter::POOL_BWD ? last.pool : nullptr;
        if (pl && relu == 2 && pl->la == fa && pl->lb == fb && pl->x == yp && pl->acc && pl->dx == zn.g && pl->C == C &&
            pl->H * pl->W == rows && !pl->stats && !caller_forms_dy && C % 4 == 0 && 256 % (C / 4) == 0) {
            const int nbp = maxpool2_bwd_blocks(B, pl->H, pl->W, C);
            float *partial = alloc((size_t)nbp * C * 2);
            pl->stats = partial;
            if (sw.plan_debug)
                fprintf(stderr, "[plan]   statistics of %-36s left by the max-pool backward (%d partial rows)\n", bn.c_str(), nbp);
            return step(partial, nbp, C, false, true);
        }
        // ... or by the fused backward of the depthwise deconv that is its only consumer (neck proj -> up): same contract
        float **ds = last.kind == LastWriter::DECONV_BWD ? last.deconv_stats : nullptr;
        if (ds && relu == 2 && zn.t.la == fa && zn.t.lb == fb && !*ds && !caller_forms_dy && !gres) {
            const int nbp = B * r.y.H;            // one workgroup per (image, row) of the deconv's input
            float *partial = alloc((size_t)nbp * C * 2);
            *ds = partial;
            if (sw.plan_debug)
                fprintf(stderr, "[plan]   statistics of %-36s left by the deconv backward (%d partial rows)\n", bn.c_str(), nbp);
            return step(partial, nbp, C, false, true);       // (gres is null here)
        }
        const int nb = chan_reduce_blocks(B, rows);
        return step(alloc((size_t)nb * C * 2), nb, C, true, true);
    }

    // ---------------------------------------------------------------- heads
    static constexpr int CP = NUM_HEADS * HEAD_CH, LD = 80;
    Tensor xh;                 // the hidden maps of the nine heads (output of the fused 64 -> 576 conv); the normalised maps are
                               // not stored: head_bwd_kernel recomputes relu(scale*x + shift) from the conv output it reads anyway
    AttnTrainArgs at{};
    AttnGradPtrs gp{};
    float *w3dense = nullptr;  // dense OIHW (576,64,3,3) copy of the nine head convs for the dgrad panel
    size_t raw_numel = 0;

    void heads_forward(int feat) {
        xh.B = B; xh.H = fh; xh.W = fw; xh.C = CP; xh.p = alloc(xh.numel());
        Tensor raw; raw.B = B; raw.H = fh; raw.W = fw; raw.C = LD; raw.p = alloc(raw.numel());
        raw_numel = raw.numel();
        for (int hd = 0; hd < NUM_HEADS; ++hd) {
            const std::string an = mc_head_keys(hd).attn;
            const int A = NUM_AFFINE, AC = NUM_AFFINE * HEAD_CH;
            at.rm[hd] = P(an + ".running_mean", HEAD_CH); at.rv[hd] = P(an + ".running_var", HEAD_CH);
            at.nbt[hd] = NBT(an + ".num_batches_tracked");
            at.att_w[hd] = P(an + ".attn_weights.attention.0.weight", AC);
            at.att_g[hd] = P(an + ".attn_weights.attention.1.weight", A);
            at.att_b[hd] = P(an + ".attn_weights.attention.1.bias", A);
            at.att_rm[hd] = P(an + ".attn_weights.attention.1.running_mean", A);
            at.att_rv[hd] = P(an + ".attn_weights.attention.1.running_var", A);
            at.att_nbt[hd] = NBT(an + ".attn_weights.attention.1.num_batches_tracked");
            at.weight_[hd] = P(an + ".weight_", AC); at.bias_[hd] = P(an + ".bias_", AC);
            gp.d_weight_[hd] = G(an + ".weight_", AC); gp.d_bias_[hd] = G(an + ".bias_", AC);
            gp.d_att_w[hd] = G(an + ".attn_weights.attention.0.weight", AC);
            gp.d_att_g[hd] = G(an + ".attn_weights.attention.1.weight", A);
            gp.d_att_b[hd] = G(an + ".attn_weights.attention.1.bias", A);
        }
        ConvPlan c3{};
        at.chunks = mc_head_conv_args(h, mem, ts->nodes[feat].t, xh.p, c3);
        if (conv_any_lazy(c3.a) && (!ts->nodes[feat].t.lrelu || !c3.lazy_ok)) {
            materialise(feat);
            conv_fwd_args(c3, h->head3, {&ts->nodes[feat].t}, h->prec);
        }
        at.stat_ld = h->head3.coutp;
        at.stats = c3.a.stats; at.B = B; at.HW = HW;
        at.stats64 = reinterpret_cast<double *>(alloc((size_t)B * at.stat_ld * 4));   // [B][stat_ld][2] doubles
        at.sv_inst = alloc((size_t)B * CP * 3); at.mu_r = alloc((size_t)CP * 2); at.bn10 = alloc(NUM_HEADS * NUM_AFFINE * 2);
        at.that = alloc((size_t)B * NUM_HEADS * NUM_AFFINE); at.yatt = alloc((size_t)B * NUM_HEADS * NUM_AFFINE);
        at.gamma_p = alloc((size_t)B * CP); at.scale = alloc((size_t)B * CP); at.shift = alloc((size_t)B * CP);
        w3dense = alloc((size_t)CP * 64 * 9);
        // AttnBN apply + ReLU + the nine 1x1 convs + prediction epilogues in ONE pass over the hidden maps
        // (head_apply_kernel, the inference kernel)
        HeadApplyArgs ha{};
        ha.hidden = xh.p; ha.scale = at.scale; ha.shift = at.shift; ha.w = h->head_w1t; ha.b = h->head_b1;
        ha.B = B; ha.HW = HW; ha.z_out = nullptr;
        for (int i = 0; i < 10; ++i) ha.pred_c[i] = PRED_CH[i];     // the prediction pointers are per call (ts->preds)
        // one closure per kernel family so that mc_profile_train attributes the durations correctly
        ts->fwd.push_back([=](mc_handle *hh, hipStream_t st) { HIPCHK(hh, launch_conv(c3, st)); return 0; });
        ts->fwd.push_back([=, ts = ts, at = at](mc_handle *hh, hipStream_t st) {
            HIPCHK(hh, launch_attn_train_fwd(at, st));
            HeadApplyArgs a2 = ha;
            for (int i = 0; i < 10; ++i) a2.pred[i] = ts->preds[i];
            HIPCHK(hh, launch_head_apply(a2, st));
            return 0;
        });
    }

    // ---- targets + losses
    void targets_and_losses() {
        mc_targets &T = ts->targets;
        const size_t R = (size_t)B * ts->max_objs;
        // one arena for the targets, one for the regression-gradient maps (single zero fill each)
        auto up = [](size_t n) { return (n + 63) / 64 * 64; };
        const size_t tn[15] = {(size_t)B * 3 * HW, (size_t)B * 9 * HW, R * 2, R * 2, R * 3, R, R, R, R * 18, R * 18,
                               R * 2, R * 18, R / 4 + 1, R * 18, R * 18};
        size_t ttot = 0;
        for (size_t n : tn) ttot += up(n);
        float *ta = alloc(ttot);
        float *tp[15];
        { size_t o = 0; for (int i = 0; i < 15; ++i) { tp[i] = ta ? ta + o : nullptr; o += up(tn[i]); } }
        T.center_heatmap_target = tp[0]; T.kpt_heatmap_target = tp[1];
        T.wh_target = tp[2]; T.offset_target = tp[3]; T.dim_target = tp[4];
        T.alpha_cls_target = tp[5]; T.alpha_offset_target = tp[6]; T.depth_target = tp[7];
        T.center2kpt_offset_target = tp[8]; T.kpt_heatmap_offset_target = tp[9];
        T.indices = reinterpret_cast<int64_t *>(tp[10]); T.indices_kpt = reinterpret_cast<int64_t *>(tp[11]);
        T.mask_target = reinterpret_cast<uint8_t *>(tp[12]);
        T.mask_center2kpt_offset = tp[13]; T.mask_kpt_heatmap_offset = tp[14];
        h->tgt_arena = ta; h->tgt_arena_bytes = ttot * sizeof(float);
        ts->dpred[0] = alloc((size_t)B * PRED_CH[0] * HW);
        ts->dpred[1] = alloc((size_t)B * PRED_CH[1] * HW);
        size_t dtot = 0;
        for (int i = 2; i < 10; ++i) dtot += up((size_t)B * PRED_CH[i] * HW);
        float *da = alloc(dtot);
        { size_t o = 0; for (int i = 2; i < 10; ++i) { ts->dpred[i] = da ? da + o : nullptr; o += up((size_t)B * PRED_CH[i] * HW); } }
        h->dp_arena = da; h->dp_arena_bytes = dtot * sizeof(float);
        ts->fwd.push_back([ts = ts, B = B, fh = fh, fw = fw](mc_handle *hh, hipStream_t st) {
            if (mc_make_targets(hh, &ts->labels, B, ts->max_objs, ts->pad_h, ts->pad_w, fh, fw, &ts->targets, st)) return -1;
            if (mc_losses(hh, ts->preds, &ts->targets, B, ts->max_objs, fh, fw, ts->losses, st)) return -1;
            return 0;
        });
    }

    // ---- losses -> raw gradients -> heads -> the gradient of feat
    void heads_backward(int feat) {
        float *draw = alloc(raw_numel);
        // MONOCON_HIP_HEAD_ZSKIP (default 1): seven of the nine heads take their loss gradient at the objects' centres and key
        // points only, so their rows of draw are zero in all but a few dozen pixels.  The pack leaves one word per aligned
        // 64-pixel tile (bit h: head h has a non-zero row there), and the two passes below branch around a head's all-zero
        // tiles -- the statistics pass does not read x there at all.  Results are those of 0 up to the sign of a zero
        // (DESIGN.md 3f.1).  2: the statistics pass only.  0: no map, every tile is visited.
        const size_t nz_words = (size_t)B * ((HW + 63) / 64);
        unsigned *nz = sw.head_zskip ? reinterpret_cast<unsigned *>(alloc(nz_words)) : nullptr;
        const unsigned *nz_bwd = nz, *nz_dx = sw.head_zskip == 1 ? nz : nullptr;
        if (sw.plan_debug)
            fprintf(stderr, "[plan] heads backward: zero-tile skip %s (%zu tile words)\n",
                    !sw.head_zskip ? "off" : sw.head_zskip == 1 ? "on" : "on in the statistics pass only", sw.head_zskip ? nz_words : (size_t)0);
        float *cs1 = alloc(colsum_partial_floats((size_t)B * HW, LD));
        float *db1 = alloc(NUM_OUT_ROWS), *dw1 = alloc((size_t)NUM_OUT_ROWS * HEAD_CH);
        push_bwd([=, ts = ts, B = B, fh = fh, fw = fw, HW = HW](mc_handle *hh, hipStream_t st) {
            if (mc_losses_backward(hh, ts->preds, &ts->targets, B, ts->max_objs, fh, fw, ts->grad_losses, ts->dpred, st)) return -1;
            // a caller's gradients wrt the maps enter here, in the same pass: everything downstream starts from draw
            bool user = false;
            for (const float *g : ts->grad_preds) user = user || g != nullptr;
            if (user)
                HIPCHK(hh, launch_dpred_pack_user(ts->dpred, ts->preds, ts->grad_preds, LD, B, HW, draw, st, nz));
            else
                HIPCHK(hh, launch_dpred_pack(ts->dpred, LD, B, HW, draw, st, nz));
            HIPCHK(hh, launch_colsum(draw, (size_t)B * HW, NUM_OUT_ROWS, LD, cs1, db1, st));
            return 0;
        });
        // the nine 1x1 convs backwards in one pass (head_bwd_kernel): weight-gradient partials, the ReLU-masked
        // data gradient d, and the (sum d, sum d*x) partials of the AttnBN backward
        const int nbr = chan_reduce_blocks(B, HW), rb_per_img = nbr / B;
        // MONOCON_HIP_HEAD_DX_FUSE=0: head_bwd_kernel stores the masked gradient d, affine_bwd_kernel reads it back.
        // Default: d is never stored -- the AttnBN backward forms it again from the 65 raw-gradient rows
        // (launch_head_dx; 7 fma per element on average against 4.3 GB less traffic per step at B = 32)
        const bool dx_fuse = sw.head_dx_fuse != 0;
        float *dh = alloc(xh.numel());
        float *dw1p = alloc((size_t)nbr * NUM_OUT_ROWS * HEAD_CH);
        float *partial = alloc((size_t)nbr * CP * 2), *coef = alloc((size_t)B * CP * 4);
        float *dx = dh;        // the AttnBN backward (an elementwise affine pass) runs in place on the masked gradient
        // scatter dw1 / db1 rows to the parameter gradient tensors (rows are in concatenation order)
        CopyBatch segcb;
        auto seg = [&](const std::string &layer, int r0, int nr) {
            if (!segcb.add(dw1 + (size_t)r0 * HEAD_CH, G(layer + ".weight", nr * HEAD_CH), (size_t)nr * HEAD_CH) ||
                !segcb.add(db1 + r0, G(layer + ".bias", nr), nr))
                ts->ok = false;
        };
        for (int hd = 0; hd < NUM_HEADS; ++hd)
            for (const HeadOutLayer &o : mc_head_keys(hd).out) seg(o.layer, o.row0, o.rows);
        const float *xp = xh.p, *w1 = h->head_w1, *zsc = at.scale, *zsh = at.shift;
        push_bwd([=, B = B, HW = HW](mc_handle *hh, hipStream_t st) {
            HIPCHK(hh, launch_head_bwd(draw, LD, nullptr, xp, w1, B, HW, nbr, dx_fuse ? nullptr : dh, dw1p, partial, st, zsc, zsh, nz_bwd));
            HIPCHK(hh, launch_splitk_reduce(dw1p, nbr, 1, NUM_OUT_ROWS, HEAD_CH, dw1, st));
            HIPCHK(hh, launch_copy_batch(segcb, st));
            return 0;
        });
        float *db3 = alloc(CP), *dw3 = alloc((size_t)CP * 64 * 9);
        float *cs3 = alloc((size_t)std::max(affine_bwd_blocks(B, (size_t)HW, CP), nbr) * CP * 2);
        Tensor dxT = xh; dxT.p = dx; dxT.amax = slot();
        unsigned *dxmax = dxT.amax;
        push_bwd([=, at = at, gp = gp, B = B, HW = HW](mc_handle *hh, hipStream_t st) {
            // d is already masked: the AttnBN backward is the plain per-(image, channel) affine map; the same pass
            // leaves the column sums of dx (the 3x3 convs' bias gradients) instead of a second read of dx
            HIPCHK(hh, launch_attn_train_bwd(at, partial, rb_per_img, gp, coef, st));
            if (dx_fuse)
                HIPCHK(hh, launch_head_dx(draw, LD, xp, w1, coef, B, HW, nbr, dx, cs3, db3, dxmax, st, zsc, zsh, nz_dx));
            else
                HIPCHK(hh, launch_affine_bwd(dh, nullptr, xp, coef, B, (size_t)HW, CP, 1, 0, dx, nullptr, 0, st, nullptr, nullptr, cs3, db3,
                                             dxmax));
            return 0;
        });
        // the fused 64 -> 576 weight gradient (2 ms at B = 32, the longest launch of the backward) and the scatter of its
        // result go to the weight-gradient stream like every other layer's: dx is a private buffer, nothing writes it again
        // in this step
        emit_wgrad({feat}, dxT, CP, CP, 3, 1, dw3);
        CopyBatch g3cb;
        for (int hd = 0; hd < NUM_HEADS; ++hd) {
            const std::string layer = mc_head_keys(hd).conv3;
            if (!g3cb.add(dw3 + (size_t)hd * 64 * 64 * 9, G(layer + ".weight", 9 * HEAD_CH * HEAD_CH), (size_t)64 * 64 * 9) ||
                !g3cb.add(db3 + hd * 64, G(layer + ".bias", HEAD_CH), 64))
                ts->ok = false;
        }
        push_bwd([=](mc_handle *hh, hipStream_t st) { HIPCHK(hh, launch_copy_batch(g3cb, st)); return 0; }, ON_SIDE);
        CopyBatch w3cb;
        for (int hd = 0; hd < NUM_HEADS; ++hd)
            if (!w3cb.add(P(mc_head_keys(hd).conv3 + ".weight", 9 * HEAD_CH * HEAD_CH), w3dense + (size_t)hd * 64 * 64 * 9,
                          (size_t)64 * 64 * 9))
                ts->ok = false;
        ts->pack_fns.push_back([=](mc_handle *hh, hipStream_t st) { HIPCHK(hh, launch_copy_batch(w3cb, st)); return 0; });
        if (h->prec == 3) h->w_amax_of[w3dense] = h->head3.w_amax;     // the dense copy shares the fused head panel's maximum
        emit_dgrad(w3dense, dxT, CP, 64, 3, 1, 0, feat, CP);
        if (ts->head_only) ts->bwd.back().feat_dgrad = true;
    }

    // ---------------------------------------------------------------- neck + backbone backwards: one method per record kind
    void pool_backward(const Rec &r) {
        TNode &in = ts->nodes[r.in];
        const TNode &o = ts->nodes[r.z];
        if (!o.ginit || !in.needs_grad) return;
        float *gi = g_acquire(r.in);
        PoolBwdArgs pa{in.t.p, o.g, in.t.la, in.t.lb, gi, nullptr, in.t.B, in.t.H, in.t.W, in.t.C, in.ginit ? 1 : 0};     // (lazy x: its ReLU'd values are compared)
        ts->pool_bwds.push_back(pa);
        PoolBwdArgs *pp = &ts->pool_bwds.back();
        push_bwd([=](mc_handle *hh, hipStream_t st) {
            HIPCHK(hh, launch_maxpool2_bwd(pp->x, pp->dout, pp->B, pp->H, pp->W, pp->C, pp->dx, pp->acc, st, pp->la, pp->lb, pp->stats));
            return 0;
        });
        wrote(r.in, pp);
        g_release(r.z, -1);
    }

    // the depthwise deconv: data and weight gradient in one pass
    void deconv_backward(const Rec &r) {
        TNode &in = ts->nodes[r.in];
        const TNode &o = ts->nodes[r.z];
        if (!o.ginit) return;
        if (in.ginit) { ts->ok = false; h->err = "train plan: deconv input has more than one consumer"; }
        const float *xp = in.t.p, *go = o.g, *wp = r.D->wpk, *xla = in.t.la, *xlb = in.t.lb;
        float *gi = g_acquire(r.in), *dw = G(r.D->name + ".weight", (int64_t)r.D->C * 16);
        const int Bq = in.t.B, Hq = in.t.H, Wq = in.t.W, Cq = in.t.C;
        float *part = alloc(deconv4_bwd_w_partial_floats(Bq, Hq, Cq));
        ts->deconv_stats.push_back(nullptr);
        float **dstats = &ts->deconv_stats.back();
        push_bwd([=](mc_handle *hh, hipStream_t st) {
            HIPCHK(hh, launch_deconv4_bwd_w(xp, go, Bq, Hq, Wq, Cq, part, dw, st, xla, xlb, wp, gi, *dstats));
            return 0;
        });
        wrote(r.in, (xla && xlb) ? dstats : nullptr);       // (the statistics need the lazy input's y)
        g_release(r.z, -1);
    }

    void conv_backward(const Rec &r) {
        if (r.dead || !ts->nodes[r.z].ginit) return;
        const Tensor dy = bn_backward(r, r.bn).dy;
        const int64_t wn = (int64_t)r.L->cout * r.L->cin * r.L->ks * r.L->ks;
        const int wgrad = emit_wgrad(r.srcs, dy, r.L->cout, r.L->cout, r.L->ks, r.L->stride, G(r.L->conv + ".weight", wn));
        const float *wm = P(r.L->conv + ".weight", wn);
        int c_off = 0;
        for (int s : r.srcs) {
            emit_dgrad(wm, dy, r.L->cout, r.L->cin, r.L->ks, r.L->stride, c_off, s, r.L->cout);
            c_off += ts->nodes[s].t.C;
        }
        g_release(r.z, wgrad);     // dZ / dY of this layer: last read by its weight gradient
    }

    void stem_backward(const Rec &r) {
        if (!ts->nodes[r.z].ginit) return;
        // mode 3: the stem's dY has ONE reader, its weight gradient -- which forms it on the fly from (d, y, coefficients)
        // instead of reading what an element-wise pass wrote (MONOCON_HIP_STEM_FUSE=0: the separate pass)
        const bool want_fused = sw.stem_fuse && h->prec == 3 && ts->img_amax && r.y.amax && W % 4 == 0 && W >= 16;
        const BnBwd bb = bn_backward(r, r.bn, want_fused);
        const bool fused = bb.affine_skipped;
        float *part = alloc((size_t)stem_wgrad_blocks(B, H, W) * 147 * 16), *dw = G("backbone.base_layer.0.weight", 16 * 147);
        const float *dyp = bb.dy.p, *yfp = fused ? r.y.p : nullptr, *cfp = fused ? bb.coef : nullptr;
        const unsigned *imax = ts->img_amax, *dymax = bb.dy.amax, *yfmax = fused ? r.y.amax : nullptr;
        const int wgrad = push_bwd([=, ts = ts, B = B, H = H, W = W](mc_handle *hh, hipStream_t st) {
            HIPCHK(hh, launch_stem_wgrad(ts->img, dyp, B, H, W, part, dw, st, imax, imax ? dymax : nullptr, yfp, cfp, yfmax));
            return 0;
        }, ON_SIDE);
        // the data gradient of the image, for a backward that asked for it (BwdStep::img_dgrad; any other backward launches
        // exactly what it launched without this step).  It reads the same buffer as the weight gradient, in the same form
        // (dY, or d with (y, coef)), on the caller's stream while the weight gradient runs on the side stream; it is pushed
        // before the buffer's release, whose last reader for the pool stays the side step (a later writer on the caller's
        // stream is ordered behind this step anyway).  fp32 in every mode; no gradient bucket: nothing is exchanged for it,
        // the image gradient is the rank's own and unscaled.
        const float *wm = P("backbone.base_layer.0.weight", 16 * 147);
        const int dgrad = push_bwd([=, ts = ts, B = B, H = H, W = W](mc_handle *hh, hipStream_t st) {
            if (ts->gimg_ext) HIPCHK(hh, launch_stem_dgrad(dyp, wm, B, H, W, ts->gimg_ext, st, yfp, cfp));
            ts->gimg_ext = nullptr;       // written once, for the call that asked for it: never a stale pointer later
            return 0;
        });
        ts->bwd[dgrad].img_dgrad = true;
        ts->bwd[dgrad].bucket = -1;
        g_release(r.z, wgrad);
    }

    // head-only plan: the gradient of the external feat goes out as NCHW
    void feat_grad_out(int feat) {
        const float *gp = ts->nodes[feat].g;
        push_bwd([=, ts = ts, B = B, fh = fh, fw = fw](mc_handle *hh, hipStream_t st) {
            if (ts->gfeat_ext) HIPCHK(hh, launch_nhwc_to_nchw(gp, B, 64, fh, fw, ts->gfeat_ext, st));
            ts->gfeat_ext = nullptr;      // written once, for the call that asked for it: never a stale pointer later
            return 0;
        });
    }
};

}  // namespace

// ------------------------------------------------------------------------------------ build
static TrainState *build_train(mc_handle *h, int B, int H, int W, bool head_only = false) {
    std::unique_ptr<TrainState, void (*)(TrainState *)> tsp(new TrainState(), train_free);
    TrainState *ts = tsp.get();
    ts->B = B; ts->H = H; ts->W = W; ts->bind_gen = h->bind_gen; ts->head_only = head_only;
    ts->sw = read_switches();
    TB b{h, ts};
    // ---- forward
    b.zero_amax_slots();
    int feat;
    if (head_only) {
        feat = b.external_feat();
    } else {
        b.stem();
        // backbone and neck: the steps of the network graph (the nodes they make are the graph's; node 0 is the stem's)
        for (const NetStep &s : h->net.steps) {
            const int o = s.kind == STEP_CONV ? b.conv_bn(s) : s.kind == STEP_POOL ? b.pool(s.srcs[0]) : b.deconv(h->deconvs[s.name], s.srcs[0]);
            if (o != s.out) { ts->ok = false; h->err = "train plan: node order differs from the network graph"; }
        }
        feat = h->net.feat;
    }
    b.heads_forward(feat);
    b.targets_and_losses();
    // ---- backward: the heads (gradient bucket 0), then neck + backbone in reverse forward order
    b.cur_bucket = 0;
    b.heads_backward(feat);
    for (int ri = (int)ts->recs.size() - 1; ri >= 0; --ri) {
        const Rec r = ts->recs[ri];
        b.cur_bucket = mc_grad_bucket_of(r.kind == REC_DECONV ? r.D->name : (r.kind == REC_POOL ? std::string("backbone.") : r.bn));
        if (r.kind == REC_POOL) b.pool_backward(r);
        else if (r.kind == REC_DECONV) b.deconv_backward(r);
        else if (r.kind == REC_CONV) b.conv_backward(r);
        else if (r.kind == REC_STEM) b.stem_backward(r);
    }
    if (head_only) b.feat_grad_out(feat);
    // a gradient bucket is complete once the LAST step pushed for its layer groups has been enqueued
    {
        bool seen[MC_NUM_GRAD_BUCKETS] = {};
        for (auto s = ts->bwd.rbegin(); s != ts->bwd.rend(); ++s) {
            if (s->bucket < 0) continue;         // (the image's data gradient: in no bucket)
            if (seen[s->bucket]) s->bucket = -1;
            else seen[s->bucket] = true;
        }
    }
    if (!ts->ok) return nullptr;
    if (ts->sw.plan_debug)
        fprintf(stderr, "[plan] lazy activations: %d never stored, %d stored after all (lazy mask %d), %.2f GB\n", b.n_lazy - b.n_materialised,
                b.n_materialised, (int)ts->sw.lazy_z, ts->mem.bytes * 1e-9);
    if (h->dry_alloc) return tsp.release();   // mc_query_workspace: sizes only
    // ---- the weight-gradient stream and its events (any failure: everything on the caller's stream)
    ts->dual = ts->sw.dual_stream != 0;
    if (ts->dual && (hipStreamCreateWithFlags(&ts->side, hipStreamNonBlocking) != hipSuccess ||
                     hipEventCreateWithFlags(&ts->side_done, hipEventDisableTiming) != hipSuccess))
        ts->dual = false;
    for (BwdStep &s : ts->bwd) {
        if (!ts->dual) break;
        if (s.stream == ON_SIDE && hipEventCreateWithFlags(&s.ready, hipEventDisableTiming) != hipSuccess) ts->dual = false;
        hipEvent_t *fin = s.wait >= 0 ? &ts->bwd[s.wait].fin : nullptr;
        if (fin && !*fin && hipEventCreateWithFlags(fin, hipEventDisableTiming) != hipSuccess) ts->dual = false;
    }
    if (hipDeviceSynchronize() != hipSuccess) return nullptr;
    return tsp.release();
}

// ====================================================================================== C ABI
extern "C" {

// the train plan of this shape (built -- and its convolution shapes autotuned -- on first use)
static TrainState *ensure_train_plan(mc_handle *h, int B, int H, int W, bool head_only) {
    TrainState *ts = h->train;
    if (!ts || ts->B != B || ts->H != H || ts->W != W || ts->bind_gen != h->bind_gen || ts->head_only != head_only) {
        if (ts && h->train_free) h->train_free(ts);
        h->train = nullptr;
        h->tgt_arena = h->dp_arena = nullptr;
        h->train_bytes = 0;
        h->tgt_arena_bytes = h->dp_arena_bytes = 0;
        ts = build_train(h, B, H, W, head_only);
        if (!ts) return nullptr;
        h->train = ts;
        h->train_bytes = ts->mem.bytes;
        h->train_free = train_free;
    }
    return ts;
}

// Build (and autotune) the train plan of a shape WITHOUT running it: no kernel of the step, no collective.  Data-parallel
// start-up: rank 0 calls this, exports its tune table (mc_tune_export), the other ranks import it and build theirs.
int mc_build_train_plan(mc_handle *h, int B, int H, int W) {
    if (!h) return -1;
    if (B < 2 || B > 64) return fail(h, "mc_build_train_plan: batch %d (2..64 per GPU)", B);
    if (H < 32 || W < 32 || (H % 32) || (W % 32)) return fail(h, "mc_build_train_plan: H, W must be multiples of 32");
    if (h->packed_groups != 7) return fail(h, "mc_build_train_plan: bind all parameters and call mc_pack_params first");
    HIPCHK(h, hipSetDevice(h->device));
    return ensure_train_plan(h, B, H, W, false) ? 0 : -1;
}

static int forward_train_impl(mc_handle *h, const float *img, const mc_labels *labels, int B, int H, int W, int max_objs,
                              float *const preds[MC_NUM_PREDS], float *losses, void *stream, bool head_only) {
    if (!h) return -1;
    const char *fn = head_only ? "mc_head_forward_train" : "mc_forward_train";
    if (!img || !labels || !preds || !losses) return fail(h, "%s: null argument", fn);
    if (B < 2 || B > 64) return fail(h, "%s: batch %d (2..64 per GPU; BatchNorm over the attention vector needs >= 2)", fn, B);
    if (H < 32 || W < 32 || (H % 32) || (W % 32)) return fail(h, "%s: H, W must be multiples of 32", fn);
    if (max_objs != 30) return fail(h, "%s: max_objs=%d (the MonoCon configuration uses 30)", fn, max_objs);
    if (head_only ? !(h->packed_groups & 4) : h->packed_groups != 7)
        return fail(h, "%s: bind all %sparameters and call mc_pack_params first", fn, head_only ? "head. " : "");
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    TrainState *ts = ensure_train_plan(h, B, H, W, head_only);
    if (!ts) return -1;
    ts->img = img; ts->feat_ext = img; ts->labels = *labels; ts->losses = losses; ts->pad_h = H; ts->pad_w = W; ts->max_objs = max_objs;
    for (int i = 0; i < MC_NUM_PREDS; ++i) {
        if (!preds[i]) return fail(h, "%s: preds[%d] is NULL", fn, i);
        ts->preds[i] = preds[i];
    }
    // refresh derived weights: forward panels (no BN folding in train mode), dgrad panels
    if (!h->pack_clean && mc_pack_params(h, 1, stream)) return -1;   // mc_pack_params / the optimizer step track staleness
    for (auto &f : ts->pack_fns)       // dense head weight copies first: some dgrad panels are cut from them
        if (f(h, st)) return -1;
    HIPCHK(h, ts->pack_batch.launch(st));
    h->train_generation = ++g_train_generation;
    ts->gfeat_ext = nullptr;      // (a previous mc_head_backward's output tensor may be gone by now)
    ts->gimg_ext = nullptr;
    for (auto &f : ts->fwd)
        if (f(h, st)) return -1;
    return 0;
}

int mc_forward_train(mc_handle *h, const float *img, const mc_labels *labels, int B, int H, int W, int max_objs,
                     float *const preds[MC_NUM_PREDS], float *losses, void *stream) {
    return forward_train_impl(h, img, labels, B, H, W, max_objs, preds, losses, stream, false);
}

int mc_head_forward_train(mc_handle *h, const float *feat, const mc_labels *labels, int B, int pad_h, int pad_w, int max_objs,
                          float *const preds[MC_NUM_PREDS], float *losses, void *stream) {
    return forward_train_impl(h, feat, labels, B, pad_h, pad_w, max_objs, preds, losses, stream, true);
}

// sizes of the train plan (mc_query_workspace modes 1 / 2): the builder runs dry, nothing is allocated or launched
int mc_train_query_workspace(mc_handle *h, int B, int H, int W, int head_only, size_t *bytes) {
    if (!h || !bytes) return -1;
    if (B < 2 || B > 64) return fail(h, "mc_query_workspace: train batch %d (2..64 per GPU)", B);
    if (head_only ? !(h->packed_groups & 4) : h->packed_groups != 7)
        return fail(h, "mc_query_workspace: bind the parameters (and their \"#grad\" buffers) and call mc_pack_params first");
    TrainState *cur = h->train;
    if (cur && cur->B == B && cur->H == H && cur->W == W && cur->head_only == (head_only != 0) && cur->bind_gen == h->bind_gen) {
        *bytes = cur->mem.bytes;
        return 0;
    }
    void *ta = h->tgt_arena, *da = h->dp_arena;
    const size_t tb = h->tgt_arena_bytes, db = h->dp_arena_bytes;
    h->dry_alloc = true; h->dry_next = 0;
    TrainState *ts = build_train(h, B, H, W, head_only != 0);
    h->dry_alloc = false;
    h->tgt_arena = ta; h->dp_arena = da; h->tgt_arena_bytes = tb; h->dp_arena_bytes = db;   // (the builder points these at its arenas)
    if (!ts) return -1;
    *bytes = ts->mem.bytes;
    ts->mem.bufs.clear();
    train_free(ts);
    return 0;
}

int mc_train_generation(mc_handle *h, unsigned long long *out) {
    if (!h || !out) return -1;
    *out = h->train_generation;
    return 0;
}

// debugging aid: copy activation node `node` (train plan order: 0 = stem output, 1 = level0, ...) as NCHW;
// which = 0 activation (a lazy one is formed for the caller), 1 the node's gradient buffer.  dims[4] receives (B, C, H, W).
// The gradient buffer is readable only with MONOCON_HIP_GRAD_POOL=0 (pooled buffers are handed on during the backward; a
// node without a private buffer fails with "no such buffer").  After a backward it holds
//   - conv + BatchNorm node: dY, the gradient wrt the RAW conv output (the affine pass writes it in place over dZ);
//   - pool / deconv output node: dZ, the plain sum of its consumers' data gradients;
//   - the stem (node 0): dY like any conv node, except where its weight gradient forms dY on the fly (mode f16x2,
//     MONOCON_HIP_STEM_FUSE=1 and the statistics left by level0's data-gradient epilogue): the affine pass is skipped and
//     the buffer keeps the masked gradient d = dZ * [z > 0].
int mc_train_debug_node(mc_handle *h, int node, int which, float *out_nchw, int dims[4], void *stream) {
    if (!h || !h->train) return fail(h, "mc_train_debug_node: no train plan");
    TrainState *ts = h->train;
    if (node < 0 || node >= (int)ts->nodes.size()) return fail(h, "mc_train_debug_node: node %d of %d", node, (int)ts->nodes.size());
    const TNode &n = ts->nodes[node];
    if (dims) { dims[0] = n.t.B; dims[1] = n.t.C; dims[2] = n.t.H; dims[3] = n.t.W; }
    if (!out_nchw) return 0;
    const float *src = which ? n.g : n.t.p;
    if (!src) return fail(h, "mc_train_debug_node: node has no such buffer");
    hipStream_t dst_st = static_cast<hipStream_t>(stream);
    if (!which && n.t.la) {       // a lazy activation exists nowhere in memory: form it for the caller
        ScratchBuf tmp;
        HIPCHK(h, tmp.alloc(n.t.numel() * sizeof(float)));
        HIPCHK(h, launch_affine_act(n.t.p, n.t.la, n.t.lb, nullptr, n.t.B, (size_t)n.t.H * n.t.W, n.t.C, 0, n.t.lrelu ? 1 : 0, tmp.as<float>(),
                                    dst_st, nullptr));
        HIPCHK(h, launch_nhwc_to_nchw(tmp.as<float>(), n.t.B, n.t.C, n.t.H, n.t.W, out_nchw, dst_st));
        HIPCHK(h, hipStreamSynchronize(dst_st));
        return 0;
    }
    HIPCHK(h, launch_nhwc_to_nchw(src, n.t.B, n.t.C, n.t.H, n.t.W, out_nchw, dst_st));
    return 0;
}

static int backward_impl(mc_handle *h, TrainState *ts, const float *grad_losses, const float *const grad_preds[MC_NUM_PREDS],
                         void *stream);

static int full_backward(mc_handle *h, const char *who, const float *grad_losses, const float *const grad_preds[MC_NUM_PREDS],
                         void *stream) {
    if (!h) return -1;
    if (!grad_losses) return fail(h, "%s: grad_losses is NULL", who);
    if (h->train && h->train->head_only)
        return fail(h, "%s: the handle holds a heads-only plan (mc_head_forward_train): use %s", who,
                    grad_preds ? "mc_head_backward_pred_grads" : "mc_head_backward");
    TrainState *ts = h->train;
    if (!ts || !ts->img) return fail(h, "%s: call mc_forward_train first", who);
    return backward_impl(h, ts, grad_losses, grad_preds, stream);
}

int mc_backward(mc_handle *h, const float *grad_losses, void *stream) {
    return full_backward(h, "mc_backward", grad_losses, nullptr, stream);
}

int mc_backward_pred_grads(mc_handle *h, const float *grad_losses, const float *const grad_preds[MC_NUM_PREDS], void *stream) {
    return full_backward(h, "mc_backward_pred_grads", grad_losses, grad_preds, stream);
}

int mc_backward_image_grad(mc_handle *h, const float *grad_losses, const float *const grad_preds[MC_NUM_PREDS], float *grad_img,
                           void *stream) {
    if (!h) return -1;
    if (h->train && h->train->head_only)
        return fail(h, "mc_backward_image_grad: the handle holds a heads-only plan (mc_head_forward_train), which has no image: "
                       "mc_head_backward returns the gradient of feat");
    if (h->train) h->train->gimg_ext = grad_img;
    const int rc = full_backward(h, "mc_backward_image_grad", grad_losses, grad_preds, stream);
    // the step that writes grad_img clears the pointer: still set after a backward that succeeded means the plan has no such
    // step (no gradient reached the stem) -- an error, never an output left unwritten
    const bool unwritten = h->train && h->train->gimg_ext != nullptr;
    if (h->train) h->train->gimg_ext = nullptr;      // (a backward that failed before the step: no stale pointer either)
    if (!rc && unwritten) return fail(h, "mc_backward_image_grad: the plan has no data-gradient step for the image (no gradient reaches the stem)");
    return rc;
}

static int backward_run(mc_handle *h, TrainState *ts, const float *grad_losses, void *stream);

static int backward_impl(mc_handle *h, TrainState *ts, const float *grad_losses, const float *const grad_preds[MC_NUM_PREDS],
                         void *stream) {
    for (int i = 0; i < MC_NUM_PREDS; ++i) ts->grad_preds[i] = grad_preds ? grad_preds[i] : nullptr;
    const int rc = backward_run(h, ts, grad_losses, stream);
    // caller-owned: neither mc_profile_train's replay of the closures nor the next backward may read them again
    for (const float *&g : ts->grad_preds) g = nullptr;
    return rc;
}

static int backward_run(mc_handle *h, TrainState *ts, const float *grad_losses, void *stream) {
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    ts->grad_losses = grad_losses;
    int k = 0;                // number of the side step (MONOCON_HIP_SIDE_SYNC counts them)
    bool used_side = false;
    unsigned fired = 0;       // gradient buckets handed to the communicator so far
    // data parallelism with a communicator owned by the handle: every gradient bucket is exchanged (averaged over the
    // ranks) on the communicator's stream as soon as its last writer has been enqueued
    const bool dp = !ts->head_only && mc_comm_overlap_active(h);
    if (dp && mc_comm_prepare(h)) return -1;
    for (const BwdStep &s : ts->bwd) {
        if (s.feat_dgrad && ts->skip_feat_dgrad) continue;
        if (s.img_dgrad && !ts->gimg_ext) continue;
        if (ts->dual && s.stream == ON_SIDE) {
            // everything this step reads (dY of its layer, forward activations) is ready at this point of
            // the main stream; its outputs (the weight gradient) are first needed after mc_backward
            HIPCHK(h, hipEventRecord(s.ready, st));
            HIPCHK(h, hipStreamWaitEvent(ts->side, s.ready, 0));
            if (s.fn(h, ts->side)) return -1;
            if (s.fin) HIPCHK(h, hipEventRecord(s.fin, ts->side));
            if (k >= ts->sw.side_sync_lo && k < ts->sw.side_sync_hi) {
                HIPCHK(h, hipEventRecord(ts->side_done, ts->side));
                HIPCHK(h, hipStreamWaitEvent(st, ts->side_done, 0));
            }
            ++k;
            used_side = true;
        } else {
            // a recycled gradient buffer: its previous content was read on the side stream
            if (used_side && s.wait >= 0 && ts->bwd[s.wait].fin) HIPCHK(h, hipStreamWaitEvent(st, ts->bwd[s.wait].fin, 0));
            if (s.fn(h, st)) return -1;
        }
        if (dp && s.bucket >= 0) {
            if (mc_comm_fire_bucket(h, s.bucket, st, used_side ? ts->side : nullptr)) return -1;
            fired |= 1u << s.bucket;
        }
    }
    if (used_side) {
        HIPCHK(h, hipEventRecord(ts->side_done, ts->side));
        HIPCHK(h, hipStreamWaitEvent(st, ts->side_done, 0));
    }
    if (dp) {
        for (int b = 0; b < MC_NUM_GRAD_BUCKETS; ++b)       // a bucket no step of this plan writes into still has to be exchanged
            if (!(fired >> b & 1) && mc_comm_fire_bucket(h, b, st, nullptr)) return -1;
        if (mc_comm_join(h, st)) return -1;
    }
    return 0;
}

static int head_backward(mc_handle *h, const char *who, const float *grad_losses, const float *const grad_preds[MC_NUM_PREDS],
                         float *grad_feat, void *stream) {
    if (!h) return -1;
    TrainState *ts = h->train;
    if (!ts || !ts->head_only || !ts->feat_ext) return fail(h, "%s: call mc_head_forward_train first", who);
    if (!grad_losses) return fail(h, "%s: grad_losses is NULL", who);
    ts->gfeat_ext = grad_feat;
    ts->skip_feat_dgrad = grad_feat == nullptr;      // feat does not require grad: its 3x3 data gradient is not computed
    return backward_impl(h, ts, grad_losses, grad_preds, stream);
}

int mc_head_backward(mc_handle *h, const float *grad_losses, float *grad_feat, void *stream) {
    return head_backward(h, "mc_head_backward", grad_losses, nullptr, grad_feat, stream);
}

int mc_head_backward_pred_grads(mc_handle *h, const float *grad_losses, const float *const grad_preds[MC_NUM_PREDS],
                                float *grad_feat, void *stream) {
    return head_backward(h, "mc_head_backward_pred_grads", grad_losses, grad_preds, grad_feat, stream);
}

int mc_profile_train(mc_handle *h, int iters, double ms[3], double flops[3], double bytes[3], int launches[3],
                     void *stream) {
    if (!h || !ms || !flops || !bytes || !launches) return -1;
    TrainState *ts = h->train;
    if (!ts || !ts->img || !ts->grad_losses) return fail(h, "mc_profile_train: run mc_forward_train + mc_backward first");
    if (iters < 1) iters = 1;
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    std::vector<const Fn *> all;      // every closure of the step in launch order, all on the caller's stream
    for (const Fn &f : ts->fwd) all.push_back(&f);
    for (const BwdStep &s : ts->bwd)
        if (!s.img_dgrad) all.push_back(&s.fn);      // (the image's data gradient: no replay has an output for it)
    const size_t n = all.size();
    std::vector<hipEvent_t> ev(2 * n);
    for (auto &e : ev) HIPCHK(h, hipEventCreate(&e));
    std::vector<ProfLast> tag(n);
    for (int k = 0; k < 3; ++k) { ms[k] = 0; flops[k] = 0; bytes[k] = 0; launches[k] = 0; }
    int rc = 0;
    for (int it = 0; it < iters && !rc; ++it) {
        size_t i = 0;
        for (const Fn *f : all) {
            prof_last = {0, 0.0, 0.0};
            (void)hipEventRecord(ev[2 * i], st);
            if ((*f)(h, st)) { rc = -1; break; }
            (void)hipEventRecord(ev[2 * i + 1], st);
            tag[i++] = prof_last;
        }
        if (hipStreamSynchronize(st) != hipSuccess) rc = fail(h, "mc_profile_train: stream error");
        for (size_t j = 0; j < i && !rc; ++j) {
            float t = 0.f;
            (void)hipEventElapsedTime(&t, ev[2 * j], ev[2 * j + 1]);
            const int k = tag[j].kind;
            ms[k] += t; flops[k] += tag[j].flops; bytes[k] += tag[j].bytes; launches[k] += 1;
            if (it == 0 && std::getenv("MONOCON_HIP_PROFILE_DUMP"))
                std::fprintf(stderr, "prof %zu %s kind %d ms %.4f gflop %.3f mb %.2f\n", j, j < ts->fwd.size() ? "fwd" : "bwd", k, t,
                             tag[j].flops * 1e-9, tag[j].bytes * 1e-6);
        }
    }
    for (auto &e : ev) (void)hipEventDestroy(e);
    for (int k = 0; k < 3; ++k) { ms[k] /= iters; flops[k] /= iters; bytes[k] /= iters; launches[k] /= iters; }
    return rc;
}

}  // extern "C"
