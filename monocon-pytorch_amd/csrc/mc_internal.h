// Internal definitions shared by the C-ABI translation units (not part of the public ABI).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <map>
#include <memory>
#include <string>
#include <tuple>
#include <unordered_map>
#include <vector>

#include "../../include/monocon_hip.h"
#include "conv_mfma.h"
#include "kernels.h"
#include "train.h"

using namespace mc;

struct TrainState;   // mc_train_plan.hip
struct CommState;    // mc_comm.hip

// data parallelism: the bound "<key>#grad" tensors in groups, in the order the backward pass completes them
// (0: heads + neck, 1: backbone.level5, 2: backbone.level4, 3: the rest of the backbone)
constexpr int MC_NUM_GRAD_BUCKETS = 4;
struct GradBucket {
    float *p = nullptr;                                  // dense address range [p, p + n) ...
    size_t n = 0;
    std::vector<std::pair<float *, size_t>> parts;       // ... or, when the tensors are scattered, one entry per tensor
    int tensors = 0;
};
int mc_grad_bucket_of(const std::string &param_name);
bool mc_comm_overlap_active(mc_handle *h);               // a communicator exists and mc_backward overlaps the exchange
int mc_comm_prepare(mc_handle *h);
int mc_comm_fire_bucket(mc_handle *h, int bucket, hipStream_t main, hipStream_t side);
int mc_comm_join(mc_handle *h, hipStream_t main);

struct Bound {
    void *ptr;
    int64_t numel;
    int dtype;
};

struct Tensor {   // NHWC activation
    float *p = nullptr;
    int B = 0, H = 0, W = 0, C = 0;
    unsigned *amax = nullptr;   // slot receiving max |x| of the tensor (precision mode 3: operand scale of its consumers)
    // LAZY activation (train plans of precision mode 3; always null in eval plans): the post-BatchNorm map
    // z = act(la[c] * y + lb[c]) is never written -- p is the producing layer's raw conv output y, and every consumer forms z
    // while it loads its operand (ConvSrc::la in conv_mfma.h; act = ReLU when lrelu).  null: p holds the values.
    const float *la = nullptr, *lb = nullptr;
    bool lrelu = true;
    size_t numel() const { return (size_t)B * H * W * C; }
};
// a caller's (B, H, W, C) map as an operand of a launch description (the op-level entry points; such a tensor is only read)
inline Tensor operand_tensor(const float *p, int B, int H, int W, int C) {
    Tensor t;
    t.p = const_cast<float *>(p); t.B = B; t.H = H; t.W = W; t.C = C;
    return t;
}

struct ConvLayer {
    std::string conv, bn;   // state_dict prefixes ("" bn => bias-only / raw)
    int ks = 1, stride = 1, cin = 0, cout = 0, coutp = 0, cfg = 0;
    float bn_eps = 1e-5f;
    float *wpk = nullptr, *scale = nullptr, *shift = nullptr;
    void *wpk16 = nullptr;   // bf16 / fp16 piece panels (precision modes 1..3)
    unsigned *w_amax = nullptr;   // max |w| of the master weight(s) (mode 3: the panel's power-of-two scale)
};

// The operands and geometry of the forward conv of layer L over the virtual concat of srcs (1..4 maps of one size) in precision
// mode prec: every field of `p.a` that follows from them -- sources, sizes, panels, a.prec (the mode where L has piece planes, 0
// otherwise) and in mode 3 the max-|x| slots of the operands -- and L's window, then plans (conv_plan).  Everything else is left
// as it is: the shape id and the epilogue (scale, bias, res, relu, out, stats, amax_out, cfg) are the caller's, who plans again
// after setting a.cfg or a.stats; a caller that has changed a source (TB::materialise) calls again.  false: the sources do not
// add up to L.cin channels.  (The data gradient's counterpart: dgrad_conv_args, train.h.)
inline bool conv_fwd_args(ConvPlan &p, const ConvLayer &L, const std::vector<const Tensor *> &srcs, int prec) {
    ConvArgs &a = p.a;
    const Tensor &s0 = *srcs[0];
    a.nsrc = (int)srcs.size();
    a.Cin = 0;
    for (int i = 0; i < a.nsrc; ++i) {
        a.src[i] = ConvSrc{srcs[i]->p, srcs[i]->C, srcs[i]->la, srcs[i]->lb};
        a.Cin += srcs[i]->C;
    }
    a.B = s0.B; a.Hin = s0.H; a.Win = s0.W;
    a.Hout = conv_out_dim(s0.H, L.ks, L.stride); a.Wout = conv_out_dim(s0.W, L.ks, L.stride);
    a.Cout = L.cout; a.CoutP = L.coutp; a.wpk = L.wpk;
    a.wpk16 = L.wpk16; a.prec = L.wpk16 ? prec : 0;
    if (a.prec == 3) {
        for (int i = 0; i < a.nsrc; ++i) a.amax_in[i] = srcs[i]->amax;
        a.amax_w = L.w_amax;
    }
    p.ks = L.ks; p.stride = L.stride;
    conv_plan(p);
    return a.Cin == L.cin;
}
// The weight gradient of a ks x ks conv of the given stride in precision mode prec: X = the virtual concat of srcs, dY = the
// first Cout of dy's dy_ld channels.  Fills sources, sizes and max-|x| slots, chooses the kernel and plans the tiling (wgrad_plan);
// `p.a.partial` stays the caller's.  A caller that has changed a source calls again (the plan does not depend on what a source holds).
inline void wgrad_args(WgradPlan &p, const std::vector<const Tensor *> &srcs, const Tensor &dy, int dy_ld, int Cout, int ks,
                       int stride, int prec) {
    WgradArgs &a = p.a;
    const Tensor &s0 = *srcs[0];
    a.nsrc = (int)srcs.size();
    a.Cin = 0;
    for (int i = 0; i < a.nsrc; ++i) {
        a.src[i] = ConvSrc{srcs[i]->p, srcs[i]->C, srcs[i]->la, srcs[i]->lb};
        a.amax_x[i] = srcs[i]->amax;
        a.Cin += srcs[i]->C;
    }
    a.amax_dy = dy.amax;
    a.B = s0.B; a.Hin = s0.H; a.Win = s0.W; a.Hout = dy.H; a.Wout = dy.W; a.Cout = Cout;
    a.dy = dy.p; a.dy_ld = dy_ld;
    a.prec = prec; p.ks = ks; p.stride = stride;
    wgrad_plan(p);
}

struct DeconvLayer {
    std::string name;
    int C = 0;
    float *wpk = nullptr;
};

constexpr const char *HEAD_NAMES[NUM_HEADS] = {"heatmap_head", "wh_head", "offset_head", "center2kpt_offset_head",
                                               "kpt_heatmap_head", "kpt_heatmap_offset_head", "dim_head", "depth_head",
                                               "dir_feat"};
// The state_dict prefixes of head hd: its 3x3 conv, its AttnBN, and its 1x1 output layers with their rows of the fused
// [NUM_OUT_ROWS][HEAD_CH] table (head_row_begin()) -- one layer, or for the last head (dir_feat) dir_cls and dir_reg, half each
struct HeadOutLayer { std::string layer; int row0, rows; };
struct HeadKeys { std::string conv3, attn; std::vector<HeadOutLayer> out; };
inline HeadKeys mc_head_keys(int hd) {
    const std::string pre = std::string("head.") + HEAD_NAMES[hd];
    const int r0 = head_row_begin()[hd], nr = head_row_begin()[hd + 1] - r0;
    HeadKeys k{pre + ".0", pre + ".1", {{pre + ".3", r0, nr}}};
    if (hd == NUM_HEADS - 1) k.out = {{"head.dir_cls.0", r0, nr / 2}, {"head.dir_reg.0", r0 + nr / 2, nr / 2}};
    return k;
}

// The backbone (DLA-34) and neck (DLAUp) as one list of steps in forward order, from the stem's output (node 0) to `feat`.
// Built once per handle (build_layers): the layer table, the eval plan and the train plan are all derived from it.  Every
// step that is not dead makes one new node; node ids are the train plan's TNode indices.
enum StepKind { STEP_CONV, STEP_POOL, STEP_DECONV };
struct NetStep {
    StepKind kind;
    std::string name, bn;     // conv: layer-table key and its BatchNorm prefix; deconv: its name
    std::vector<int> srcs;    // input nodes (pool / deconv: one)
    int res = -1;             // conv: residual node (-1: none)
    int out = -1;             // output node (-1: dead)
    int ks = 1, stride = 1, cout = 0;
    bool relu = true;
    bool dead = false;                    // output never read (the outer `project` of a two-level tree: its BatchNorm
                                          // statistics still tick in train mode)
    bool elementwise_consumers = false;   // read by element-wise kernels only (a neck projection: by its deconv)
    bool never_lazy = false;              // stored even where a lazy activation would do (`feat`)
};
struct NetGraph {
    std::vector<NetStep> steps;
    std::vector<int> node_c;    // channels of every node
    int lv[6] = {};             // nodes of the level outputs l0..l5
    int n_backbone = 0;         // steps [0, n_backbone) are the backbone, the rest the neck
    int feat = -1;
};

// Device memory of a launch plan (or of the handle's parameter tables).
struct PlanMem {
    std::vector<void *> bufs;
    size_t bytes = 0;                  // requested sizes, summed (mc_query_workspace / mc_workspace_bytes)
    unsigned *amax_arena = nullptr;    // precision mode 3: one max-|x| slot per tensor, zeroed at the start of every forward
    int amax_used = 0;
    void release() {
        for (void *q : bufs) (void)hipFree(q);
        bufs.clear();
    }
};

// The allocator of every plan builder: zero-filled buffers owned by `m`.  With h->dry_alloc (mc_query_workspace) a buffer
// is only counted: its address is a fake that is never dereferenced.  A failed request sets h->err, clears `ok` and
// returns null.
struct PlanAlloc {
    mc_handle *h;
    PlanMem &m;
    bool &ok;
    size_t empty_floats;    // the size of an empty request (eval plan and parameter tables: 4 floats, train plan: 1)
    int amax_slots;         // capacity of the slot arena
    float *alloc(size_t nfloats);
    unsigned *slot();       // mode 3: a fresh max-|x| slot (null in the other modes)
};

// A bound tensor checked against what a plan reads: `dtype` (MC_F32; MC_I64 for num_batches_tracked) and `numel`
// elements, also for "<key>#grad" buffers.  Missing or mismatched: h->err names the key, null is returned.
void *mc_param(mc_handle *h, const std::string &name, int64_t numel, int dtype = MC_F32);
// The layer-table entry `name`.  Missing: h->err names it, `ok` is cleared and an empty layer is returned.
ConvLayer &mc_conv_layer(mc_handle *h, const std::string &name, bool &ok);
// The fused head conv (64 -> 9 x 64, 3x3) of a plan on `feat` into `hidden`: head3's panels and shape id, head_bias, and the
// per-patch statistics of (v - head_rm), whose buffer it takes from `mem`: [B][patches per image][head3.coutp][2] (p.a.stats).
// Returns the patches per image.
int mc_head_conv_args(mc_handle *h, PlanAlloc &mem, const Tensor &feat, float *hidden, ConvPlan &p);

enum OpKind { OP_STEM, OP_CONV, OP_POOL, OP_DECONV, OP_HEAD_ATTN, OP_HEAD_APPLY };

struct Op {
    OpKind kind;
    // conv
    ConvPlan cp{};
    // generic
    const float *in = nullptr;
    float *out = nullptr, *out2 = nullptr;   // out2: OP_HEAD_ATTN's second output (the AttnBN shift beside the scale)
    const float *w = nullptr, *scale = nullptr, *shift = nullptr;
    int B = 0, H = 0, W = 0, C = 0;
    int chunks = 0;
    HeadApplyArgs ha{};
    double flops = 0, bytes = 0;
    unsigned *amax = nullptr;   // OP_DECONV in mode 3: slot of the output tensor
};

struct Plan {
    int B = 0, H = 0, W = 0;
    std::vector<Op> ops;
    PlanMem mem;
    Tensor feat, lv[6];
    std::vector<Tensor> nodes;   // activation of every graph node (mc_infer_debug_node)
    Tensor hidden;               // the fused head conv's raw output: 9 x 64 channels, bias added, before AttnBN
    float *hs_scale = nullptr, *hs_shift = nullptr;   // head_attn_kernel's per-(image, head, channel) AttnBN affine
    const float *head_stats = nullptr;                // the head conv's per-patch (sum, sum of squares) of v - rm
    int head_chunks = 0;                              // patches per image
    int stem_op = -1, head_apply_op = -1;
    int n_backbone_ops = 0, n_neck_ops = 0;
    double flops = 0, hbm_bytes = 0;
};

struct mc_handle {
    int device = 0;
    std::string err;
    std::unordered_map<std::string, Bound> bound;
    NetGraph net;
    std::map<std::string, ConvLayer> convs;
    std::map<std::string, DeconvLayer> deconvs;
    // stem
    float *stem_w = nullptr, *stem_scale = nullptr, *stem_shift = nullptr;
    // fused head 3x3 (64 -> 9*64) and second pass
    ConvLayer head3;
    float *head_bias = nullptr, *head_rm = nullptr;
    float *att_scale = nullptr, *att_shift = nullptr;   // [9][10]
    float *head_w1 = nullptr, *head_w1t = nullptr, *head_b1 = nullptr;   // [65][64], transposed [64][65], [65]
    HeadAttnParams hap{};
    bool layers_built = false, packed = false;
    int packed_groups = 0;   // bit0 backbone, bit1 neck, bit2 head
    PlanMem params;
    std::map<std::tuple<int, int, int>, std::unique_ptr<Plan>> plans;
    Plan *last_plan = nullptr;
    float *decode_filt = nullptr;
    size_t decode_filt_n = 0;
    size_t decode_count_n = 0;
    unsigned long long *nms_ws = nullptr;   // mc_nms3d: the suppression bit matrices of a batch with K > 128 (nms3d.hip)
    size_t nms_ws_words = 0;
    int force_cfg = 0;   // tuning aid (mc_bench_conv)
    int lm_kernel = 3;   // mc_set_local_maximum_kernel: window of the decode's local-maximum filter (test_config['local_maximum_kernel'])
    int prec = 0;        // mc_set_precision: 0 fp32 MFMA, 1 bf16 operands, 2 three-way bf16 split, 3 two-way fp16 split
    unsigned *w_amax_arena = nullptr;                    // mode 3: max |w| per conv layer (+ the fused head panel)
    int w_amax_n = 0;
    std::map<const float *, unsigned *> w_amax_of;       // master weight -> its slot (train plan: data-gradient panels)
    int autotune = 1;    // time the workgroup shapes of every distinct conv once (MONOCON_HIP_AUTOTUNE=0: heuristic)
    std::map<std::vector<int>, int> tuned;   // conv signature -> shape id
    float *loss_ws = nullptr;   // focal partials + small reduction scratch
    // fused optimizer tables (device)
    mc::OptTensor *opt_tab = nullptr;
    mc::OptChunk *opt_chunks = nullptr;
    int opt_nchunks = 0, opt_ntensors = 0;
    int opt_max_cls = 0;        // largest class index of the bound table
    unsigned opt_novmax = 0;    // bit c: some tensor of class c was bound without max_exp_avg_sq
    float *opt_ws = nullptr;    // partials + [norm, coef]
    // gradient-only table of the stand-alone clip (mc_clip_bind)
    mc::OptTensor *clip_tab = nullptr;
    mc::OptChunk *clip_chunks = nullptr;
    int clip_nchunks = 0;
    // weight averages: the optimizer table's host copy (mc_optim_bind_ema fills its .e and uploads it again) and the
    // (average, source) table of the stand-alone update (mc_ema_bind)
    std::vector<mc::OptTensor> opt_host;
    std::vector<int64_t> opt_numel;
    bool opt_has_ema = false;   // some tensor of the bound optimizer table has an average
    mc::OptTensor *ema_tab = nullptr;
    mc::OptChunk *ema_chunks = nullptr;
    int ema_nchunks = 0;
    // gradient accumulation (mc_accum_bind): the (accumulator, gradient) table and whether a window is open
    mc::OptTensor *accum_tab = nullptr;
    mc::OptChunk *accum_chunks = nullptr;
    int accum_nchunks = 0;
    bool accum_open = false;
    // non-finite guard (mc_optim_set_guard): the step entries launch the guarded instantiations while it is on
    mc::GuardRecord *opt_guard = nullptr;   // the last guarded step's record (device)
    bool opt_guard_on = false;
    bool opt_guard_ran = false; // a guarded step has run since the guard was switched on: the record is a step's
    // LAMB (mc_clip_lamb_step_classes): one allocation, made by the first LAMB step after a bind and freed with the table
    mc::LambWorkspace lamb_ws{nullptr, nullptr, nullptr};
    bool lamb_ran = false;      // a LAMB step has been enqueued on the bound table: lamb_ws.ratio holds a step's ratios
    // train-step plan (mc_train_plan.hip)
    TrainState *train = nullptr;
    size_t train_bytes = 0;   // device memory owned by the train plan
    // mc_query_workspace: plan builders run "dry" -- buffers are counted, not allocated (fake addresses that are never
    // dereferenced), nothing is launched or cached
    bool dry_alloc = false;
    size_t dry_next = 0;
    unsigned long long train_generation = 0;   // id of the forward whose activations the train plan holds (0: none)
    void (*train_free)(TrainState *) = nullptr;
    unsigned long long bind_gen = 0;
    bool pack_clean = false;   // packed panels match the bound parameters (cleared by bind / optimizer step)
    // job tables of mc_pack_params (forward panels of all layers, BatchNorm folds): rebuilt when the binding or the
    // precision mode changes, launched as one grid each
    mc::PackBatch fwd_pack;
    mc::FoldBatch folds;
    unsigned long long pack_tab_gen = ~0ull;
    int pack_tab_prec = -1;
    // RCCL communicator owned by the handle (mc_comm_init)
    CommState *comm = nullptr;
    void (*comm_free)(CommState *) = nullptr;
    // train plan: all target tensors / all regression-gradient maps live in one arena each, so the
    // per-step zero fill is one memset instead of 17 + 8 (mc_make_targets / mc_losses_backward)
    void *tgt_arena = nullptr, *dp_arena = nullptr;
    size_t tgt_arena_bytes = 0, dp_arena_bytes = 0;
};

extern std::string g_create_err;

static inline int fail(mc_handle *h, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (h) h->err = buf; else g_create_err = buf;
    return -1;
}

// device scratch of the op-level (test) entry points: released on every return path
struct ScratchBuf {
    void *p = nullptr;
    ScratchBuf() = default;
    ScratchBuf(const ScratchBuf &) = delete;
    ScratchBuf &operator=(const ScratchBuf &) = delete;
    ~ScratchBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes); }
    template <class T> T *as() const { return static_cast<T *>(p); }
};

// The mode-3 max-|x| slots of an op-level entry point, zeroed on `st`: slot i < 4 <- max |src[i]| (n[i] elements), slot 4 is
// the one more operand's -- `extra` non-null: max |extra| (n_extra elements; single_word: a weight's slot), null: left
// zeroed for the caller's own pass.  Slot i is at buf.as<unsigned>() + i * AMAX_WORDS.
static inline hipError_t op_amax_slots(ScratchBuf &buf, const float *const src[], const size_t n[], int nsrc, const float *extra,
                                       size_t n_extra, bool single_word, hipStream_t st) {
    const size_t bytes = 5 * mc::AMAX_WORDS * sizeof(unsigned);
    hipError_t e = buf.alloc(bytes);
    if (e == hipSuccess) e = hipMemsetAsync(buf.p, 0, bytes, st);
    unsigned *sl = buf.as<unsigned>();
    for (int i = 0; i < nsrc && e == hipSuccess; ++i) e = mc::launch_absmax(src[i], n[i], sl + i * mc::AMAX_WORDS, st);
    if (extra && e == hipSuccess) e = mc::launch_absmax(extra, n_extra, sl + 4 * mc::AMAX_WORDS, st, single_word);
    return e;
}

#define HIPCHK(h, expr)                                                                      \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess) return fail(h, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

// Workgroup shape for a fused conv launch: h->force_cfg if set, else (autotune on) the fastest of the
// candidate shapes timed on the device with these very arguments, cached per conv signature; else
// the static heuristic.  The accumulation order of an output element does not depend on the shape,
// so the choice never changes results (per-image statistics partials are regrouped, not reordered
// within a partial).  `a.stats` must be null while tuning (callers attach it afterwards).
int mc_choose_conv_cfg(mc_handle *h, const mc::ConvPlan &p);

