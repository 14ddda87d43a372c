// Fused gradient-norm clip + AdamW over a table of parameter tensors.
// Replaces torch.nn.utils.clip_grad_norm_(max_norm, norm_type) + torch.optim.AdamW.step of the reference's
// train loop (engine/monocon_engine.py:94-102): two launches per step instead of several
// hundred per-tensor kernels; 16 B/param of traffic (p, g, m, v read; p, m, v written), 20 B/param with amsgrad.
//
// Every kernel is a template whose all-default instantiation (L2 norm; one hyper-parameter set, no amsgrad) is the
// reference recipe's path: launch_clip_adamw reaches only those, and their arithmetic, chunk walk and partial order are
// the ones the committed goldens were recorded against.  The other instantiations add the norm kinds of
// clip_grad_norm_ and torch.optim.AdamW's per-group options, and (EMA) the exponential moving average of the weights that
// long runs keep for evaluation: formed in the step's own pass, 8 B/param more, no launch and no second read of p.
// The *_guarded kernels (mc_optim_set_guard, off by default) are further instantiations beside those: the step skips
// itself when the norm is not finite, decided on the device from the norm that is already there.  The unguarded
// kernels are launched exactly as before while the guard is off.
// grad_accum_kernel (mc_grad_accumulate) sums the gradients of a window of micro-batches in a table of its own and leaves
// their mean in the gradient tensors: no kernel above gains an instantiation for it.
// The lamb_* kernels (mc_clip_lamb_step_classes, opt-in) are the layer-wise adaptive step: kernels of their own behind the
// same global-norm pass; the AdamW, EMA, guard and accumulation kernels keep their code and their launches.
#include <stdint.h>
#include "conv_mfma.h"
#include "train.h"

namespace mc {

// Every tensor of the table starts 16-byte aligned (FlatGrads pads each gradient to a multiple of 4 floats, torch
// allocations are 256-byte aligned) and every chunk starts at a multiple of 65536 elements, so a chunk is walked as
// float4 with a scalar tail: the passes run at the HBM roof instead of at the dword-load issue rate.
__device__ __forceinline__ bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// ---- global gradient norm: sum |g|^p (NORM_L2: g*g) or max |g| per workgroup, then one wave over the partials
enum { NORM_L2 = 0, NORM_L1 = 1, NORM_INF = 2, NORM_P = 3 };

template <int KIND> __device__ __forceinline__ float norm_term(float x, float p) {
    if constexpr (KIND == NORM_L2) return x * x;
    else if constexpr (KIND == NORM_P) return powf(fabsf(x), p);
    else return fabsf(x);
}
// NORM_INF: a maximum that keeps a NaN once it has seen one (torch's max does; fmax alone would drop it)
template <int KIND, typename T> __device__ __forceinline__ T norm_join(T a, T b) {
    if constexpr (KIND == NORM_INF) return a != a ? a : (b != b ? b : (a > b ? a : b));
    else return a + b;
}

template <int KIND>
__global__ __launch_bounds__(256) void gradnorm_partial_kernel(const OptTensor *tab, const OptChunk *chunks, int nchunks,
                                                               float *partial, float p) {
    float s = 0.f;
    for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const OptChunk ck = chunks[c];
        const float *g = tab[ck.tensor].g + ck.begin;
        int i0 = 0;
        if (aligned16(g)) {
            const int n4 = ck.count >> 2;
            const f32x4 *g4 = reinterpret_cast<const f32x4 *>(g);
            for (int i = threadIdx.x; i < n4; i += 256) {
                const f32x4 v = g4[i];
                s = norm_join<KIND>(s, norm_join<KIND>(norm_join<KIND>(norm_join<KIND>(norm_term<KIND>(v[0], p), norm_term<KIND>(v[1], p)),
                                                                       norm_term<KIND>(v[2], p)), norm_term<KIND>(v[3], p)));
            }
            i0 = n4 << 2;
        }
        for (int i = i0 + threadIdx.x; i < ck.count; i += 256) s = norm_join<KIND>(s, norm_term<KIND>(g[i], p));
    }
    __shared__ float red[4];
    for (int o = 32; o > 0; o >>= 1) s = norm_join<KIND>(s, __shfl_xor(s, o));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = norm_join<KIND>(norm_join<KIND>(norm_join<KIND>(red[0], red[1]), red[2]), red[3]);
}

// the root is taken in double; coef = max_norm / (norm + 1e-6) clamped to 1 is clip_grad_norm_'s formula
template <int KIND>
__global__ void gradnorm_final_kernel(const float *partial, int n, float max_norm, float *out /*[2]: norm, coef*/, double inv_p) {
    double s = 0;
    for (int i = threadIdx.x; i < n; i += 64) s = norm_join<KIND>(s, (double)partial[i]);
    for (int o = 32; o > 0; o >>= 1) s = norm_join<KIND>(s, __shfl_xor(s, o));
    if (threadIdx.x == 0) {
        float norm;
        if constexpr (KIND == NORM_L2) norm = (float)sqrt(s);
        else if constexpr (KIND == NORM_P) norm = (float)pow(s, inv_p);
        else norm = (float)s;
        out[0] = norm;
        const float coef = max_norm / (norm + 1e-6f);
        out[1] = (max_norm > 0.f && coef < 1.f) ? coef : 1.f;
    }
}

// ---- non-finite guard (mc_optim_set_guard).  An element with an all-ones exponent is a NaN or an infinity.
__device__ __forceinline__ unsigned nonfinite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u ? 1u : 0u; }

// gradnorm_final_kernel (its reduction, its root, its coefficient: the same bits in out[0..1]) that also opens the step's
// guard record: skipped when the norm AS COMPUTED is not finite -- a NaN or infinite element, or finite squares whose fp32
// sum overflowed -- as clip_grad_norm_(error_if_nonfinite=True) judges it.  The AdamW pass that follows reads the flag.
template <int KIND>
__global__ void gradnorm_final_guarded_kernel(const float *partial, int n, float max_norm, float *out /*[2]: norm, coef*/, double inv_p,
                                              GuardRecord *rec) {
    double s = 0;
    for (int i = threadIdx.x; i < n; i += 64) s = norm_join<KIND>(s, (double)partial[i]);
    for (int o = 32; o > 0; o >>= 1) s = norm_join<KIND>(s, __shfl_xor(s, o));
    if (threadIdx.x == 0) {
        float norm;
        if constexpr (KIND == NORM_L2) norm = (float)sqrt(s);
        else if constexpr (KIND == NORM_P) norm = (float)pow(s, inv_p);
        else norm = (float)s;
        out[0] = norm;
        const float coef = max_norm / (norm + 1e-6f);
        out[1] = (max_norm > 0.f && coef < 1.f) ? coef : 1.f;
        rec->skipped = (int)nonfinite(norm);
        rec->first_tensor = -1;
        rec->n_elements = 0ull;
        rec->norm = norm;
    }
}

// ---- the AdamW step.  AMS: torch's amsgrad (vmax = max(vmax, v); the denominator uses vmax)
template <bool AMS>
__device__ __forceinline__ void adamw_one(float &p, float g, float &m, float &v, float &vmax, float coef, const AdamHyper &hp) {
    g *= coef;
    p *= hp.decay;                               // p *= 1 - lr*wd   (decoupled weight decay)
    m = m * hp.beta1 + g * hp.one_minus_beta1;
    v = v * hp.beta2 + g * g * hp.one_minus_beta2;
    float d = v;
    if constexpr (AMS) { vmax = fmaxf(vmax, v); d = vmax; }
    const float denom = sqrtf(d) / hp.sqrt_bc2 + hp.eps;
    p -= hp.step_size * (m / denom);
}

// ---- weight average (solver/model_ema.py): the only place it is formed.  w = 1 - decay_t, folded on the host in double.
// w == 1 (decay 0) is the copy it means: (p - e) + e rounds twice and misses p by an ulp where |e| << |p|.  w is a kernel
// argument, so the select is on a scalar condition.  (w == 0 never gets here: the entry points launch nothing for it.)
__device__ __forceinline__ void ema_one(float &e, float p, float w) { e = w == 1.f ? p : fmaf(w, p - e, e); }

// EMA: a chunk whose tensor has an average (t.e, uniform per chunk: a scalar branch) updates it with the new p still in
// registers -- in the float4 body and in the scalar tail alike.  Whether an element is walked by the body or by the tail
// never depends on e: the two round p differently (contraction), and attaching an average must not move a bit of the
// update.  So an e that is not 16-byte aligned like the other pointers (no torch allocation is) is read and written
// with four dword accesses inside the body.
template <bool AMS, bool EMA = false>
__device__ __forceinline__ void adamw_chunk(const OptTensor &t, const OptChunk &ck, float coef, const AdamHyper &hp, float w = 0.f) {
    float *p = t.p + ck.begin, *m = t.m + ck.begin, *v = t.v + ck.begin;
    const float *g = t.g + ck.begin;
    float *x = AMS ? t.vmax + ck.begin : nullptr;
    float *e = (EMA && t.e) ? t.e + ck.begin : nullptr;
    int i0 = 0;
    if (aligned16(p) && aligned16(g) && aligned16(m) && aligned16(v) && (!AMS || aligned16(x))) {
        const int n4 = ck.count >> 2;
        const bool e16 = aligned16(e);
        for (int i = threadIdx.x; i < n4; i += 256) {
            f32x4 p4 = reinterpret_cast<f32x4 *>(p)[i], m4 = reinterpret_cast<f32x4 *>(m)[i], v4 = reinterpret_cast<f32x4 *>(v)[i];
            const f32x4 g4 = reinterpret_cast<const f32x4 *>(g)[i];
            f32x4 x4 = {0.f, 0.f, 0.f, 0.f}, e4 = {0.f, 0.f, 0.f, 0.f};
            if constexpr (AMS) x4 = reinterpret_cast<f32x4 *>(x)[i];
            if constexpr (EMA) {
                if (e && e16) e4 = reinterpret_cast<f32x4 *>(e)[i];
                else if (e) { e4[0] = e[4 * i]; e4[1] = e[4 * i + 1]; e4[2] = e[4 * i + 2]; e4[3] = e[4 * i + 3]; }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float pj = p4[j], mj = m4[j], vj = v4[j], xj = x4[j];
                adamw_one<AMS>(pj, g4[j], mj, vj, xj, coef, hp);
                p4[j] = pj; m4[j] = mj; v4[j] = vj; x4[j] = xj;
                if constexpr (EMA) { float ej = e4[j]; ema_one(ej, pj, w); e4[j] = ej; }
            }
            reinterpret_cast<f32x4 *>(p)[i] = p4;
            reinterpret_cast<f32x4 *>(m)[i] = m4;
            reinterpret_cast<f32x4 *>(v)[i] = v4;
            if constexpr (AMS) reinterpret_cast<f32x4 *>(x)[i] = x4;
            if constexpr (EMA) {
                if (e && e16) reinterpret_cast<f32x4 *>(e)[i] = e4;
                else if (e) { e[4 * i] = e4[0]; e[4 * i + 1] = e4[1]; e[4 * i + 2] = e4[2]; e[4 * i + 3] = e4[3]; }
            }
        }
        i0 = n4 << 2;
    }
    for (int i = i0 + threadIdx.x; i < ck.count; i += 256) {
        float xi = 0.f;
        if constexpr (AMS) xi = x[i];
        adamw_one<AMS>(p[i], g[i], m[i], v[i], xi, coef, hp);
        if constexpr (AMS) x[i] = xi;
        if constexpr (EMA) if (e) ema_one(e[i], p[i], w);
    }
}

__global__ __launch_bounds__(256) void adamw_kernel(const OptTensor *tab, const OptChunk *chunks, int nchunks,
                                                    const float *normcoef, AdamHyper hp) {
    const float coef = normcoef[1];
    for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const OptChunk ck = chunks[c];
        const OptTensor t = tab[ck.tensor];
        adamw_chunk<false>(t, ck, coef, hp);
    }
}

// the same walk with the weight average folded in (w > 0 and some bound tensor has one: the launchers choose)
__global__ __launch_bounds__(256) void adamw_ema_kernel(const OptTensor *tab, const OptChunk *chunks, int nchunks,
                                                        const float *normcoef, AdamHyper hp, float w) {
    const float coef = normcoef[1];
    for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const OptChunk ck = chunks[c];
        const OptTensor t = tab[ck.tensor];
        adamw_chunk<false, true>(t, ck, coef, hp, w);
    }
}

// Per-class hyper-parameters.  A chunk belongs to one tensor, so its class is the same for the whole workgroup: it is
// forced into a scalar register, and the row of the by-value table is then fetched with scalar loads from the
// kernel-argument segment once per chunk -- never per element.  maximize flips the sign of g AFTER the clip coefficient
// (as torch does), which is exactly the coefficient's sign.  AMSGRAD: some class of the launch is amsgrad.
template <bool AMSGRAD>
__global__ __launch_bounds__(256) void adamw_classes_kernel(const OptTensor *tab, const OptChunk *chunks, int nchunks,
                                                            const float *normcoef, AdamTable tb) {
    const float coef0 = normcoef[1];
    for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const OptChunk ck = chunks[c];
        const OptTensor t = tab[ck.tensor];
        const int k = __builtin_amdgcn_readfirstlane(t.cls) & (OPT_MAX_CLASSES - 1);
        const AdamHyper hp = tb.hp[k];
        const float coef = ((tb.maximize >> k) & 1u) ? -coef0 : coef0;
        if (AMSGRAD && ((tb.amsgrad >> k) & 1u)) adamw_chunk<true>(t, ck, coef, hp);
        else adamw_chunk<false>(t, ck, coef, hp);
    }
}

template <bool AMSGRAD>
__global__ __launch_bounds__(256) void adamw_classes_ema_kernel(const OptTensor *tab, const OptChunk *chunks, int nchunks,
                                                                const float *normcoef, AdamTable tb, float w) {
    const float coef0 = normcoef[1];
    for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const OptChunk ck = chunks[c];
        const OptTensor t = tab[ck.tensor];
        const int k = __builtin_amdgcn_readfirstlane(t.cls) & (OPT_MAX_CLASSES - 1);
        const AdamHyper hp = tb.hp[k];
        const float coef = ((tb.maximize >> k) & 1u) ? -coef0 : coef0;
        if (AMSGRAD && ((tb.amsgrad >> k) & 1u)) adamw_chunk<true, true>(t, ck, coef, hp, w);
        else adamw_chunk<false, true>(t, ck, coef, hp, w);
    }
}

// ---- the guarded step.  The flag is read once per workgroup, as a uniform value.  Clear: the very walk of the kernels
// above over the same adamw_chunk bodies, so every bit of p, m, v, vmax and e is theirs.  Set: nothing is written to any of
// them; the workgroups walk g alone (4 B/param, the norm pass's float4-body / scalar-tail split) and name the culprit with
// one vector-memory atomic pair per workgroup that found something: the smallest table index of a tensor holding a NaN/inf
// element (first_tensor is -1 = 0xffffffff before: an unsigned minimum) and the number of such elements.  A norm that
// overflowed from finite elements finds nothing and leaves -1 / 0.
__device__ __forceinline__ void guard_scan(const OptTensor *tab, const OptChunk *chunks, int nchunks, GuardRecord *rec) {
    unsigned long long cnt = 0ull;
    unsigned first = ~0u;
    for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const OptChunk ck = chunks[c];
        const float *g = tab[ck.tensor].g + ck.begin;
        unsigned here = 0u;
        int i0 = 0;
        if (aligned16(g)) {
            const int n4 = ck.count >> 2;
            const f32x4 *g4 = reinterpret_cast<const f32x4 *>(g);
            for (int i = threadIdx.x; i < n4; i += 256) {
                const f32x4 v = g4[i];
                here += nonfinite(v[0]) + nonfinite(v[1]) + nonfinite(v[2]) + nonfinite(v[3]);
            }
            i0 = n4 << 2;
        }
        for (int i = i0 + threadIdx.x; i < ck.count; i += 256) here += nonfinite(g[i]);
        if (here) {
            cnt += here;
            if ((unsigned)ck.tensor < first) first = (unsigned)ck.tensor;
        }
    }
    __shared__ unsigned long long red_cnt[4];
    __shared__ unsigned red_first[4];
    for (int o = 32; o > 0; o >>= 1) {
        cnt += __shfl_xor(cnt, o);
        const unsigned f = __shfl_xor(first, o);
        first = f < first ? f : first;
    }
    if ((threadIdx.x & 63) == 0) { red_cnt[threadIdx.x >> 6] = cnt; red_first[threadIdx.x >> 6] = first; }
    __syncthreads();
    if (threadIdx.x == 0) {
        cnt = red_cnt[0] + red_cnt[1] + red_cnt[2] + red_cnt[3];
        for (int k = 1; k < 4; ++k) first = red_first[k] < first ? red_first[k] : first;
        if (cnt) {
            atomicAdd(&rec->n_elements, cnt);
            atomicMin(reinterpret_cast<unsigned *>(&rec->first_tensor), first);
        }
    }
}

template <bool EMA>
__global__ __launch_bounds__(256) void adamw_guarded_kernel(const OptTensor *tab, const OptChunk *chunks, int nchunks,
                                                            const float *normcoef, AdamHyper hp, float w, GuardRecord *rec) {
    if (__builtin_amdgcn_readfirstlane(rec->skipped)) { guard_scan(tab, chunks, nchunks, rec); return; }
    const float coef = normcoef[1];
    for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const OptChunk ck = chunks[c];
        const OptTensor t = tab[ck.tensor];
        if constexpr (EMA) adamw_chunk<false, true>(t, ck, coef, hp, w);
        else adamw_chunk<false>(t, ck, coef, hp);
    }
}

template <bool AMSGRAD, bool EMA>
__global__ __launch_bounds__(256) void adamw_classes_guarded_kernel(const OptTensor *tab, const OptChunk *chunks, int nchunks,
                                                                    const float *normcoef, AdamTable tb, float w, GuardRecord *rec) {
    if (__builtin_amdgcn_readfirstlane(rec->skipped)) { guard_scan(tab, chunks, nchunks, rec); return; }
    const float coef0 = normcoef[1];
    for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const OptChunk ck = chunks[c];
        const OptTensor t = tab[ck.tensor];
        const int k = __builtin_amdgcn_readfirstlane(t.cls) & (OPT_MAX_CLASSES - 1);
        const AdamHyper hp = tb.hp[k];
        const float coef = ((tb.maximize >> k) & 1u) ? -coef0 : coef0;
        if constexpr (EMA) {
            if (AMSGRAD && ((tb.amsgrad >> k) & 1u)) adamw_chunk<true, true>(t, ck, coef, hp, w);
            else adamw_chunk<false, true>(t, ck, coef, hp, w);
        } else {
            if (AMSGRAD && ((tb.amsgrad >> k) & 1u)) adamw_chunk<true>(t, ck, coef, hp);
            else adamw_chunk<false>(t, ck, coef, hp);
        }
    }
}

// stand-alone weight average over a table of its own (mc_ema_bind: e in .p, its source in .g): e = ema_one(e, src, w) for
// everything the optimizer did not step -- BatchNorm running statistics, parameters without a gradient, loops with another
// optimizer -- and the yardstick of the fused path.  12 B/element.
__device__ __forceinline__ void ema_walk(const OptTensor *tab, const OptChunk *chunks, int nchunks, float w) {
    for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const OptChunk ck = chunks[c];
        const OptTensor t = tab[ck.tensor];
        float *e = t.p + ck.begin;
        const float *src = t.g + ck.begin;
        int i0 = 0;
        if (aligned16(e) && aligned16(src)) {
            const int n4 = ck.count >> 2;
            for (int i = threadIdx.x; i < n4; i += 256) {
                f32x4 e4 = reinterpret_cast<f32x4 *>(e)[i];
                const f32x4 s4 = reinterpret_cast<const f32x4 *>(src)[i];
#pragma unroll
                for (int j = 0; j < 4; ++j) { float ej = e4[j]; ema_one(ej, s4[j], w); e4[j] = ej; }
                reinterpret_cast<f32x4 *>(e)[i] = e4;
            }
            i0 = n4 << 2;
        }
        for (int i = i0 + threadIdx.x; i < ck.count; i += 256) ema_one(e[i], src[i], w);
    }
}

__global__ __launch_bounds__(256) void ema_kernel(const OptTensor *tab, const OptChunk *chunks, int nchunks, float w) {
    ema_walk(tab, chunks, nchunks, w);
}

// mc_ema_update_guarded: nothing at all when the handle's last guarded step was skipped -- the rest of the average
// (BatchNorm running statistics, parameters without a gradient) then stays where the stepped part stayed
__global__ __launch_bounds__(256) void ema_guarded_kernel(const OptTensor *tab, const OptChunk *chunks, int nchunks, float w,
                                                          const GuardRecord *rec) {
    if (__builtin_amdgcn_readfirstlane(rec->skipped)) return;
    ema_walk(tab, chunks, nchunks, w);
}

// stand-alone clip_grad_norm_: every bound gradient times the clip coefficient, in place
__global__ __launch_bounds__(256) void grad_scale_kernel(const OptTensor *tab, const OptChunk *chunks, int nchunks,
                                                         const float *normcoef) {
    const float coef = normcoef[1];
    if (coef == 1.f) return;                     // not clipped: x * 1 is x
    for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const OptChunk ck = chunks[c];
        float *g = tab[ck.tensor].g + ck.begin;
        int i0 = 0;
        if (aligned16(g)) {
            const int n4 = ck.count >> 2;
            f32x4 *g4 = reinterpret_cast<f32x4 *>(g);
            for (int i = threadIdx.x; i < n4; i += 256) {
                f32x4 v = g4[i];
                v[0] *= coef; v[1] *= coef; v[2] *= coef; v[3] *= coef;
                g4[i] = v;
            }
            i0 = n4 << 2;
        }
        for (int i = i0 + threadIdx.x; i < ck.count; i += 256) g[i] *= coef;
    }
}

// ---- gradient accumulation over a window of micro-batches (mc_accum_bind: the accumulator in .p, the gradient mc_backward
// writes in .g).  BEGIN: acc = g (8 B/element).  ADD: acc = acc + g (12 B/element).  FINISH: g = (acc + g) * scale, acc only
// read (12 B/element): the window's mean lands in the gradient tensors themselves, so the norm, the clip, every AdamW
// instantiation, the guard and the gradient exchange run on it unchanged.
// The arithmetic is one fp32 round-to-nearest add and (FINISH) one fp32 round-to-nearest multiply, each an instruction of
// its own: contraction is switched off for the function (an add feeding a multiply is no fma pattern either way; the ISA of
// FINISH shows v_add_f32 then v_mul_f32 per element).  Element-wise and the same two operations in the float4
// body and in the scalar tail, so an element's bits depend neither on who walked it nor on the alignment of acc or g: the
// body always runs, and a pointer that is not 16-byte aligned is read and written there with four dword accesses (as the
// EMA pointer of adamw_chunk).
enum { ACCUM_BEGIN = 0, ACCUM_ADD = 1, ACCUM_FINISH = 2 };      // == MC_ACCUM_*

template <int MODE> __device__ __forceinline__ float accum_one(float a, float g, float scale) {
#pragma clang fp contract(off)
    if constexpr (MODE == ACCUM_BEGIN) return g;
    const float s = a + g;
    if constexpr (MODE == ACCUM_FINISH) return s * scale;
    return s;
}

__device__ __forceinline__ f32x4 load4(const float *p, int i, bool a16) {
    if (a16) return reinterpret_cast<const f32x4 *>(p)[i];
    f32x4 v = {p[4 * i], p[4 * i + 1], p[4 * i + 2], p[4 * i + 3]};
    return v;
}
__device__ __forceinline__ void store4(float *p, int i, bool a16, const f32x4 &v) {
    if (a16) reinterpret_cast<f32x4 *>(p)[i] = v;
    else { p[4 * i] = v[0]; p[4 * i + 1] = v[1]; p[4 * i + 2] = v[2]; p[4 * i + 3] = v[3]; }
}

// ALIGNED: acc and g of the chunk are both 16-byte aligned (a uniform choice, made once per chunk): the body is the plain
// float4 loop of the other passes.  Otherwise the same loop with the misaligned pointer's accesses as dwords.
template <int MODE, bool ALIGNED>
__device__ __forceinline__ void accum_chunk(float *a, float *g, int count, float scale, bool a16, bool g16) {
    float *dst = MODE == ACCUM_FINISH ? g : a;
    const bool d16 = MODE == ACCUM_FINISH ? g16 : a16;
    const int n4 = count >> 2;
    for (int i = threadIdx.x; i < n4; i += 256) {
        const f32x4 g4 = load4(g, i, ALIGNED || g16);
        f32x4 a4 = {0.f, 0.f, 0.f, 0.f};
        if constexpr (MODE != ACCUM_BEGIN) a4 = load4(a, i, ALIGNED || a16);
        f32x4 r;
#pragma unroll
        for (int j = 0; j < 4; ++j) r[j] = accum_one<MODE>(a4[j], g4[j], scale);
        store4(dst, i, ALIGNED || d16, r);
    }
    for (int i = (n4 << 2) + threadIdx.x; i < count; i += 256)
        dst[i] = accum_one<MODE>(MODE != ACCUM_BEGIN ? a[i] : 0.f, g[i], scale);
}

template <int MODE>
__global__ __launch_bounds__(256) void grad_accum_kernel(const OptTensor *tab, const OptChunk *chunks, int nchunks, float scale) {
    for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const OptChunk ck = chunks[c];
        const OptTensor t = tab[ck.tensor];
        float *a = t.p + ck.begin, *g = t.g + ck.begin;
        const bool a16 = aligned16(a), g16 = aligned16(g);
        if (a16 && g16) accum_chunk<MODE, true>(a, g, ck.count, scale, true, true);
        else accum_chunk<MODE, false>(a, g, ck.count, scale, a16, g16);
    }
}

// ---- LAMB (mc_clip_lamb_step_classes): the Adam update u of every tensor rescaled by its trust ratio r = |p| / |u|.
// r needs both norms over the WHOLE tensor before one element of p moves, so the step is three launches behind the global
// norm: lamb_moments_kernel (m, v and each chunk's (sum p^2, sum u^2): 24 B/param), lamb_ratio_kernel (one wave per tensor
// over its chunks' sums) and lamb_apply_kernel (u again from p, m, v; p -= lr * r * u; the average: 16 or 24 B/param).  u is
// recomputed, not stored: 40 B/param over the two passes against 48 with a stored u.
// Determinism: a chunk's sums are left in the chunk's OWN slot, never added across workgroups with atomics, and every level
// of the sum has a fixed order -- an element's lane follows from its index in the chunk alone (the float4 body always runs;
// a pointer that is not 16-byte aligned is accessed there as four dwords, as in accum_chunk), then the wave's shuffles, the
// four LDS partials in order, the chunks of a tensor in double in a fixed lane order.  Every fp32 expression below has its
// fused operations spelled out (fmaf) and contraction off for the rest, so body and tail give an element the same bits.
__device__ __forceinline__ void lamb_moments_one(float g, float &m, float &v, float coef, const LambHyper &hp) {
#pragma clang fp contract(off)
    g *= coef;
    m = fmaf(m, hp.beta1, g * hp.one_minus_beta1);
    v = fmaf(v, hp.beta2, (g * g) * hp.one_minus_beta2);
}
// u = (m / bc1) / (sqrt(v) / sqrt(bc2) + eps) + wd * p: the one statement of it, for the norms of pass 1 and the step of pass 3
__device__ __forceinline__ float lamb_u(float p, float m, float v, const LambHyper &hp) {
#pragma clang fp contract(off)
    const float denom = sqrtf(v) / hp.sqrt_bc2 + hp.eps;
    return fmaf(hp.wd, p, (m / hp.bc1) / denom);
}
__device__ __forceinline__ float lamb_sq4(float s, const f32x4 &x) {
#pragma clang fp contract(off)
    return s + (((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]) + x[3] * x[3]);
}
__device__ __forceinline__ float lamb_sq1(float s, float x) {
#pragma clang fp contract(off)
    return s + x * x;
}

// pass 1 over one chunk: m and v written, (sum p^2, sum u^2) of the lane's elements returned in sp / su
template <bool ALIGNED>
__device__ __forceinline__ void lamb_moments_chunk(const OptTensor &t, const OptChunk &ck, float coef, const LambHyper &hp,
                                                   float &sp, float &su) {
    const float *p = t.p + ck.begin, *g = t.g + ck.begin;
    float *m = t.m + ck.begin, *v = t.v + ck.begin;
    const bool p16 = ALIGNED || aligned16(p), g16 = ALIGNED || aligned16(g), m16 = ALIGNED || aligned16(m), v16 = ALIGNED || aligned16(v);
    const int n4 = ck.count >> 2;
    for (int i = threadIdx.x; i < n4; i += 256) {
        const f32x4 p4 = load4(p, i, p16), g4 = load4(g, i, g16);
        f32x4 m4 = load4(m, i, m16), v4 = load4(v, i, v16), u4;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float mj = m4[j], vj = v4[j];
            lamb_moments_one(g4[j], mj, vj, coef, hp);
            m4[j] = mj; v4[j] = vj;
            u4[j] = lamb_u(p4[j], mj, vj, hp);
        }
        store4(m, i, m16, m4);
        store4(v, i, v16, v4);
        sp = lamb_sq4(sp, p4);
        su = lamb_sq4(su, u4);
    }
    for (int i = (n4 << 2) + threadIdx.x; i < ck.count; i += 256) {
        float mi = m[i], vi = v[i];
        const float pi = p[i];
        lamb_moments_one(g[i], mi, vi, coef, hp);
        m[i] = mi; v[i] = vi;
        sp = lamb_sq1(sp, pi);
        su = lamb_sq1(su, lamb_u(pi, mi, vi, hp));
    }
}

// GUARD: the step's guard record decides first (set: only the gradients are scanned for the culprit, nothing else is written)
template <bool GUARD>
__global__ __launch_bounds__(256) void lamb_moments_kernel(const OptTensor *tab, const OptChunk *chunks, int nchunks,
                                                           const float *normcoef, LambTable tb, float *chunk_sums /*[nchunks][2]*/,
                                                           GuardRecord *rec) {
    if constexpr (GUARD) {
        if (__builtin_amdgcn_readfirstlane(rec->skipped)) { guard_scan(tab, chunks, nchunks, rec); return; }
    }
    __shared__ float red[4][2];
    const float coef0 = normcoef[1];
    for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const OptChunk ck = chunks[c];
        const OptTensor t = tab[ck.tensor];
        const int k = __builtin_amdgcn_readfirstlane(t.cls) & (OPT_MAX_CLASSES - 1);
        const LambHyper hp = tb.hp[k];
        const float coef = ((tb.maximize >> k) & 1u) ? -coef0 : coef0;
        float sp = 0.f, su = 0.f;
        if (aligned16(t.p + ck.begin) && aligned16(t.g + ck.begin) && aligned16(t.m + ck.begin) && aligned16(t.v + ck.begin))
            lamb_moments_chunk<true>(t, ck, coef, hp, sp, su);
        else lamb_moments_chunk<false>(t, ck, coef, hp, sp, su);
        for (int o = 32; o > 0; o >>= 1) { sp += __shfl_xor(sp, o); su += __shfl_xor(su, o); }
        if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = sp; red[threadIdx.x >> 6][1] = su; }
        __syncthreads();
        if (threadIdx.x == 0) {
            chunk_sums[2 * c] = ((red[0][0] + red[1][0]) + red[2][0]) + red[3][0];
            chunk_sums[2 * c + 1] = ((red[0][1] + red[1][1]) + red[2][1]) + red[3][1];
        }
        __syncthreads();                         // red is written again by the workgroup's next chunk
    }
}

// pass 2, one wave per tensor: its chunks' sums (contiguous in the chunk list: first_chunk[t] .. first_chunk[t + 1]) joined
// in double, both roots in double.  r = |p| / |u| where the tensor's class adapts and both norms are > 0 -- false for a NaN,
// which then reaches p through u, not through r -- else 1; capped at trust_clip when that is > 0.
template <bool GUARD>
__global__ __launch_bounds__(64) void lamb_ratio_kernel(const OptTensor *tab, int ntensors, const int *first_chunk,
                                                        const float *chunk_sums, unsigned adapt, float trust_clip, float *ratio,
                                                        const GuardRecord *rec) {
    if constexpr (GUARD) {
        if (__builtin_amdgcn_readfirstlane(rec->skipped)) return;
    }
    const int t = blockIdx.x;
    if (t >= ntensors) return;
    double sp = 0, su = 0;
    for (int c = first_chunk[t] + threadIdx.x; c < first_chunk[t + 1]; c += 64) {
        sp += (double)chunk_sums[2 * c];
        su += (double)chunk_sums[2 * c + 1];
    }
    for (int o = 32; o > 0; o >>= 1) { sp += __shfl_xor(sp, o); su += __shfl_xor(su, o); }
    if (threadIdx.x == 0) {
        const double pn = sqrt(sp), un = sqrt(su);
        const int k = tab[t].cls & (OPT_MAX_CLASSES - 1);
        double r = (((adapt >> k) & 1u) && pn > 0.0 && un > 0.0) ? pn / un : 1.0;
        if (trust_clip > 0.f && r > (double)trust_clip) r = (double)trust_clip;
        ratio[t] = (float)r;
    }
}

__device__ __forceinline__ float lamb_apply_one(float p, float m, float v, float step, const LambHyper &hp) {
    return fmaf(-step, lamb_u(p, m, v, hp), p);          // p - (lr * r) * u
}

// pass 3 over one chunk; EMA: the tensor's average (e, may be null) follows the new p from the same registers
template <bool ALIGNED, bool EMA>
__device__ __forceinline__ void lamb_apply_chunk(const OptTensor &t, const OptChunk &ck, float step, const LambHyper &hp, float w) {
    float *p = t.p + ck.begin;
    const float *m = t.m + ck.begin, *v = t.v + ck.begin;
    float *e = (EMA && t.e) ? t.e + ck.begin : nullptr;
    const bool p16 = ALIGNED || aligned16(p), m16 = ALIGNED || aligned16(m), v16 = ALIGNED || aligned16(v), e16 = aligned16(e);
    const int n4 = ck.count >> 2;
    for (int i = threadIdx.x; i < n4; i += 256) {
        f32x4 p4 = load4(p, i, p16);
        const f32x4 m4 = load4(m, i, m16), v4 = load4(v, i, v16);
        f32x4 e4 = {0.f, 0.f, 0.f, 0.f};
        if constexpr (EMA) { if (e) e4 = load4(e, i, e16); }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            p4[j] = lamb_apply_one(p4[j], m4[j], v4[j], step, hp);
            if constexpr (EMA) { float ej = e4[j]; ema_one(ej, p4[j], w); e4[j] = ej; }
        }
        store4(p, i, p16, p4);
        if constexpr (EMA) { if (e) store4(e, i, e16, e4); }
    }
    for (int i = (n4 << 2) + threadIdx.x; i < ck.count; i += 256) {
        const float pi = lamb_apply_one(p[i], m[i], v[i], step, hp);
        p[i] = pi;
        if constexpr (EMA) { if (e) ema_one(e[i], pi, w); }
    }
}

template <bool EMA, bool GUARD>
__global__ __launch_bounds__(256) void lamb_apply_kernel(const OptTensor *tab, const OptChunk *chunks, int nchunks, LambTable tb,
                                                         const float *ratio, float w, const GuardRecord *rec) {
    if constexpr (GUARD) {
        if (__builtin_amdgcn_readfirstlane(rec->skipped)) return;
    }
    for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const OptChunk ck = chunks[c];
        const OptTensor t = tab[ck.tensor];
        const int k = __builtin_amdgcn_readfirstlane(t.cls) & (OPT_MAX_CLASSES - 1);
        const LambHyper hp = tb.hp[k];
        const float step = hp.lr * ratio[ck.tensor];
        if (aligned16(t.p + ck.begin) && aligned16(t.m + ck.begin) && aligned16(t.v + ck.begin))
            lamb_apply_chunk<true, EMA>(t, ck, step, hp, w);
        else lamb_apply_chunk<false, EMA>(t, ck, step, hp, w);
    }
}

constexpr int OPT_BLOCKS = 2048;
static int opt_blocks(int nchunks) { return nchunks < OPT_BLOCKS ? nchunks : OPT_BLOCKS; }

template <int KIND>
static void launch_norm_kind(const OptTensor *tab, const OptChunk *chunks, int nchunks, float *partial, float *normcoef,
                             float max_norm, double norm_type, hipStream_t st, GuardRecord *guard = nullptr) {
    const int blocks = opt_blocks(nchunks);
    hipLaunchKernelGGL(gradnorm_partial_kernel<KIND>, dim3(blocks), dim3(256), 0, st, tab, chunks, nchunks, partial, (float)norm_type);
    if (guard) hipLaunchKernelGGL(gradnorm_final_guarded_kernel<KIND>, dim3(1), dim3(64), 0, st, partial, blocks, max_norm, normcoef, 1.0 / norm_type, guard);
    else hipLaunchKernelGGL(gradnorm_final_kernel<KIND>, dim3(1), dim3(64), 0, st, partial, blocks, max_norm, normcoef, 1.0 / norm_type);
}

hipError_t launch_grad_norm(const OptTensor *tab, const OptChunk *chunks, int nchunks, float *partial, float *normcoef,
                            float max_norm, double norm_type, hipStream_t st, GuardRecord *guard) {
    if (norm_type == 2.0) launch_norm_kind<NORM_L2>(tab, chunks, nchunks, partial, normcoef, max_norm, norm_type, st, guard);
    else if (norm_type == 1.0) launch_norm_kind<NORM_L1>(tab, chunks, nchunks, partial, normcoef, max_norm, norm_type, st, guard);
    else if (norm_type == INFINITY) launch_norm_kind<NORM_INF>(tab, chunks, nchunks, partial, normcoef, max_norm, norm_type, st, guard);
    else if (norm_type > 0.0) launch_norm_kind<NORM_P>(tab, chunks, nchunks, partial, normcoef, max_norm, norm_type, st, guard);
    else return hipErrorInvalidValue;            // p <= 0 or NaN (the entry points reject it before this)
    return hipGetLastError();
}

// ema_w: the step's weight of the average, 0 unless it is > 0 AND some bound tensor has one (the entry points see to that);
// 0 launches the instantiations without EMA, as before
hipError_t launch_clip_adamw(const OptTensor *tab, const OptChunk *chunks, int nchunks, float *partial, float *normcoef,
                             float max_norm, const AdamHyper &hp, hipStream_t st, float ema_w, GuardRecord *guard) {
    launch_norm_kind<NORM_L2>(tab, chunks, nchunks, partial, normcoef, max_norm, 2.0, st, guard);
    if (guard) {
        if (ema_w > 0.f) hipLaunchKernelGGL(adamw_guarded_kernel<true>, dim3(opt_blocks(nchunks)), dim3(256), 0, st, tab, chunks, nchunks, normcoef, hp, ema_w, guard);
        else hipLaunchKernelGGL(adamw_guarded_kernel<false>, dim3(opt_blocks(nchunks)), dim3(256), 0, st, tab, chunks, nchunks, normcoef, hp, 0.f, guard);
    } else if (ema_w > 0.f) hipLaunchKernelGGL(adamw_ema_kernel, dim3(opt_blocks(nchunks)), dim3(256), 0, st, tab, chunks, nchunks, normcoef, hp, ema_w);
    else hipLaunchKernelGGL(adamw_kernel, dim3(opt_blocks(nchunks)), dim3(256), 0, st, tab, chunks, nchunks, normcoef, hp);
    return hipGetLastError();
}

hipError_t launch_adamw_classes(const OptTensor *tab, const OptChunk *chunks, int nchunks, const float *normcoef,
                                const AdamTable &tb, hipStream_t st, float ema_w, GuardRecord *guard) {
    const int blocks = opt_blocks(nchunks);
    if (guard) {
        if (ema_w > 0.f) {
            if (tb.amsgrad) hipLaunchKernelGGL((adamw_classes_guarded_kernel<true, true>), dim3(blocks), dim3(256), 0, st, tab, chunks, nchunks, normcoef, tb, ema_w, guard);
            else hipLaunchKernelGGL((adamw_classes_guarded_kernel<false, true>), dim3(blocks), dim3(256), 0, st, tab, chunks, nchunks, normcoef, tb, ema_w, guard);
        } else if (tb.amsgrad) hipLaunchKernelGGL((adamw_classes_guarded_kernel<true, false>), dim3(blocks), dim3(256), 0, st, tab, chunks, nchunks, normcoef, tb, 0.f, guard);
        else hipLaunchKernelGGL((adamw_classes_guarded_kernel<false, false>), dim3(blocks), dim3(256), 0, st, tab, chunks, nchunks, normcoef, tb, 0.f, guard);
    } else if (ema_w > 0.f) {
        if (tb.amsgrad) hipLaunchKernelGGL(adamw_classes_ema_kernel<true>, dim3(blocks), dim3(256), 0, st, tab, chunks, nchunks, normcoef, tb, ema_w);
        else hipLaunchKernelGGL(adamw_classes_ema_kernel<false>, dim3(blocks), dim3(256), 0, st, tab, chunks, nchunks, normcoef, tb, ema_w);
    } else if (tb.amsgrad) hipLaunchKernelGGL(adamw_classes_kernel<true>, dim3(blocks), dim3(256), 0, st, tab, chunks, nchunks, normcoef, tb);
    else hipLaunchKernelGGL(adamw_classes_kernel<false>, dim3(blocks), dim3(256), 0, st, tab, chunks, nchunks, normcoef, tb);
    return hipGetLastError();
}

// the three LAMB passes behind launch_grad_norm; ema_w as in launch_adamw_classes
template <bool GUARD>
static void launch_lamb_passes(const OptTensor *tab, const OptChunk *chunks, int nchunks, int ntensors, const float *normcoef,
                               const LambTable &tb, const LambWorkspace &ws, hipStream_t st, float ema_w, GuardRecord *guard) {
    const int blocks = opt_blocks(nchunks);
    hipLaunchKernelGGL(lamb_moments_kernel<GUARD>, dim3(blocks), dim3(256), 0, st, tab, chunks, nchunks, normcoef, tb, ws.chunk_sums, guard);
    hipLaunchKernelGGL(lamb_ratio_kernel<GUARD>, dim3(ntensors), dim3(64), 0, st, tab, ntensors, ws.first_chunk, ws.chunk_sums, tb.adapt,
                       tb.trust_clip, ws.ratio, guard);
    if (ema_w > 0.f) hipLaunchKernelGGL((lamb_apply_kernel<true, GUARD>), dim3(blocks), dim3(256), 0, st, tab, chunks, nchunks, tb, ws.ratio, ema_w, guard);
    else hipLaunchKernelGGL((lamb_apply_kernel<false, GUARD>), dim3(blocks), dim3(256), 0, st, tab, chunks, nchunks, tb, ws.ratio, 0.f, guard);
}

hipError_t launch_lamb_classes(const OptTensor *tab, const OptChunk *chunks, int nchunks, int ntensors, const float *normcoef,
                               const LambTable &tb, const LambWorkspace &ws, hipStream_t st, float ema_w, GuardRecord *guard) {
    if (guard) launch_lamb_passes<true>(tab, chunks, nchunks, ntensors, normcoef, tb, ws, st, ema_w, guard);
    else launch_lamb_passes<false>(tab, chunks, nchunks, ntensors, normcoef, tb, ws, st, ema_w, nullptr);
    return hipGetLastError();
}

hipError_t launch_ema(const OptTensor *tab, const OptChunk *chunks, int nchunks, float w, hipStream_t st, const GuardRecord *guard) {
    if (guard) hipLaunchKernelGGL(ema_guarded_kernel, dim3(opt_blocks(nchunks)), dim3(256), 0, st, tab, chunks, nchunks, w, guard);
    else hipLaunchKernelGGL(ema_kernel, dim3(opt_blocks(nchunks)), dim3(256), 0, st, tab, chunks, nchunks, w);
    return hipGetLastError();
}

hipError_t launch_grad_accum(const OptTensor *tab, const OptChunk *chunks, int nchunks, int mode, float scale, hipStream_t st) {
    const int blocks = opt_blocks(nchunks);
    if (mode == ACCUM_BEGIN) hipLaunchKernelGGL(grad_accum_kernel<ACCUM_BEGIN>, dim3(blocks), dim3(256), 0, st, tab, chunks, nchunks, scale);
    else if (mode == ACCUM_ADD) hipLaunchKernelGGL(grad_accum_kernel<ACCUM_ADD>, dim3(blocks), dim3(256), 0, st, tab, chunks, nchunks, scale);
    else if (mode == ACCUM_FINISH) hipLaunchKernelGGL(grad_accum_kernel<ACCUM_FINISH>, dim3(blocks), dim3(256), 0, st, tab, chunks, nchunks, scale);
    else return hipErrorInvalidValue;            // (the entry point rejects it before this)
    return hipGetLastError();
}

hipError_t launch_grad_scale(const OptTensor *tab, const OptChunk *chunks, int nchunks, const float *normcoef, hipStream_t st) {
    hipLaunchKernelGGL(grad_scale_kernel, dim3(opt_blocks(nchunks)), dim3(256), 0, st, tab, chunks, nchunks, normcoef);
    return hipGetLastError();
}
int opt_partial_floats() { return OPT_BLOCKS; }

}  // namespace mc
