// The optimizer on the device: Adam / AdamW (dep_adam_step), global-norm gradient clipping (dep_grad_sqnorm, dep_adam_step_clipped,
// dep_grad_clip_scale), gradient accumulation over micro-batches (dep_grad_accumulate), and AMSGrad plus a fused average of the
// parameters (dep_adam_step_ext, dep_swap), and the value clamp, per-group norms and the device-side count of landed updates
// (dep_adam_step_opt, dep_grad_clip_value); include/dep_rnn.h.
//
// Two equalities hold by construction.  adam_kernel and adam_clipped_kernel both call adam_element, the one Adam expression, so a clip
// coefficient of one gives the plain step's bits; adam_ext_kernel and adam_clipped_ext_kernel are the same two kernel bodies around
// adam_element<true>, which adds the running maximum and the average to that expression and repeats none of it; adam_opt_kernel and
// adam_opt_ext_kernel are a third body around the same two instances, whose clamp and coefficients only prepare gv.  grad_sqnorm_kernel
// and grad_accumulate_kernel are both gn_walk<> over their ranges, so the partial sums the accumulate launch leaves are the ones
// dep_grad_sqnorm forms from the accumulator.
//
// The sum of squares is a pure function of the data.  The ranges are read as ONE concatenated array cut into chunks of
// GN_CHUNK floats; partial slot s holds the sum over chunks s, s + GN_SLOTS, ... in that order, and ONE workgroup owns a slot
// whatever the size (the grid is always GN_SLOTS workgroups).  Inside a chunk thread t squares elements 4t .. 4t+3 in fp64 (the
// product of two fp32 values is exact there), adds them as (p0 + p1) + (p2 + p3), and the workgroup sums its threads through a
// fixed butterfly in the wave and a fixed tree over the four waves.  No atomics, no cross-workgroup hand-off: the partials are
// plain stores that the kernel boundary publishes.  The consumers re-sum the GN_SLOTS partials with the same fixed tree in EVERY
// workgroup, so every workgroup -- and every data-parallel rank, which holds the same reduced gradients -- forms the same bits.
#include "dep_common.h"

namespace {

constexpr int GN_SLOTS = 256;              // partial sums (doubles) the caller provides: dep_grad_norm_slots()
constexpr int GN_THREADS = 256;
constexpr int GN_CHUNK = GN_THREADS * 4;   // floats per chunk, one 16-byte load per thread: dep_grad_norm_chunk()
constexpr int GN_MAXR = 16;
static_assert(GN_SLOTS == GN_THREADS, "the consumers load one partial per thread");

struct GradRanges {
    const float* ptr[GN_MAXR];
    long start[GN_MAXR + 1];               // start[r] = index of range r's first element in the concatenation; start[count] = total
    int count;
};
struct GradRangesRW { float* ptr[GN_MAXR]; long n[GN_MAXR]; int count; };
struct AccumRanges {                       // GradRanges with an accumulator beside every gradient range (same counts, same concatenation)
    float* acc[GN_MAXR];
    const float* g[GN_MAXR];
    long start[GN_MAXR + 1];
    int count;
};

// sum over the workgroup's GN_THREADS threads, the same bits in every thread: xor butterfly in the wave (commutative pairs, so all
// lanes agree), then (w0 + w1) + (w2 + w3) over the waves
__device__ __forceinline__ double gn_block_sum(double v, double* red) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// The walk of both range kernels.  Ranges: GradRanges or AccumRanges (start[], count).  one(r, off): the value of element off of range r;
// four(r, off): the four values from off on, which sit in range r at a 16-byte boundary.  The callables may store as well as load.
// Returns this thread's sum of squares over the chunks of its workgroup's slot, (p0 + p1) + (p2 + p3) per chunk.
template <class Ranges, class One, class Four>
__device__ __forceinline__ double gn_walk(const Ranges& R, One one, Four four) {
    const long total = R.start[R.count];
    const long nchunks = (total + GN_CHUNK - 1) / GN_CHUNK;
    double acc = 0.0;
    for (long c = blockIdx.x; c < nchunks; c += GN_SLOTS) {
        const long i = c * GN_CHUNK + (long)threadIdx.x * 4;
        double p0 = 0.0, p1 = 0.0, p2 = 0.0, p3 = 0.0;
        if (i < total) {
            int r = 0;
            while (i >= R.start[r + 1]) ++r;                       // i < total = start[count]: stops at r < count
            const long off = i - R.start[r];
            if (i + 3 < R.start[r + 1] && (off & 3) == 0) {        // the four elements sit in one range at a 16-byte boundary
                const f32x4 x = four(r, off);
                p0 = (double)x[0] * (double)x[0]; p1 = (double)x[1] * (double)x[1];
                p2 = (double)x[2] * (double)x[2]; p3 = (double)x[3] * (double)x[3];
            } else {                                               // a range boundary or the tail: element by element (absent = +0)
                double p[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const long k = i + e;
                    if (k < total) {
                        while (k >= R.start[r + 1]) ++r;
                        const double x = (double)one(r, k - R.start[r]);
                        p[e] = x * x;
                    }
                }
                p0 = p[0]; p1 = p[1]; p2 = p[2]; p3 = p[3];
            }
        }
        acc += (p0 + p1) + (p2 + p3);
    }
    return acc;
}

__global__ __launch_bounds__(GN_THREADS) void grad_sqnorm_kernel(GradRanges R, double* __restrict__ partials) {
    __shared__ double red[4];
    const double acc = gn_walk(R, [&](int r, long off) { return R.ptr[r][off]; },
                               [&](int r, long off) { return *reinterpret_cast<const f32x4*>(R.ptr[r] + off); });
    const double s = gn_block_sum(acc, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;                // every slot is written (0 for a slot without a chunk)
}

// acc = first ? g * scale : acc + g * scale over the ranges, and (partials != NULL) grad_sqnorm_kernel's partial sums of the STORED result in
// the same pass: both kernels are gn_walk and gn_block_sum, this one with callables that store what they return, so the partials carry
// the bits dep_grad_sqnorm forms afterwards from the accumulator.  The product and the sum are two fp32 roundings (no FMA): numpy float32
// reproduces the result, and scale == 1 is the plain IEEE add.  `first`: acc is written without being read.
__device__ __forceinline__ float ga_value(float a, float g, float scale, int first) {
    // contraction off for THESE two operations: hipcc's __fmul_rn / __fadd_rn are inline * and + compiled under the default
    // (contract = fast), and their pair came out as one v_fmac_f32 -- 12 ulp from numpy's float32 where the sum cancels
#pragma clang fp contract(off)
    const float t = g * scale;
    return first ? t : a + t;
}
__global__ __launch_bounds__(GN_THREADS) void grad_accumulate_kernel(AccumRanges R, float scale, int first, double* __restrict__ partials) {
    __shared__ double red[4];
    const double acc = gn_walk(R,
        [&](int r, long off) {
            float* ap = R.acc[r] + off;
            const float x = ga_value(first ? 0.f : *ap, R.g[r][off], scale, first);
            *ap = x;
            return x;
        },
        [&](int r, long off) {
            const f32x4 gv = *reinterpret_cast<const f32x4*>(R.g[r] + off);
            f32x4 a = {0.f, 0.f, 0.f, 0.f};
            if (!first) a = *reinterpret_cast<const f32x4*>(R.acc[r] + off);
            f32x4 x;
#pragma unroll
            for (int e = 0; e < 4; ++e) x[e] = ga_value(a[e], gv[e], scale, first);
            *reinterpret_cast<f32x4*>(R.acc[r] + off) = x;
            return x;
        });
    if (partials == nullptr) return;                               // uniform over the grid
    const double s = gn_block_sum(acc, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;                // every slot is written (0 for a slot without a chunk)
}

// What every consumer workgroup derives from the partials: S, norm = sqrt(S), and torch's clip coefficient
//     coef = (float) min(1, max_norm / (norm + 1e-6))          (division in double, ONE rounding to fp32; a NaN quotient stays NaN)
// max_norm <= 0 ("measure only", +inf arrives here as 0): coef = 1.
struct ClipCoef { float coef; double norm; bool finite; };
// from S itself: the one place the formula stands (adam_opt_body has S of every group in hand and needs their sum as well)
__device__ __forceinline__ ClipCoef gn_coef_of(double S, double max_norm) {
    ClipCoef c;
    c.norm = sqrt(S);
    c.finite = S - S == 0.0;                                        // false for inf and NaN
    if (max_norm > 0.0) {
        const double q = max_norm / (c.norm + 1e-6);
        c.coef = (float)(q > 1.0 ? 1.0 : q);
    } else {
        c.coef = 1.0f;
    }
    return c;
}
__device__ __forceinline__ ClipCoef gn_coef(const double* __restrict__ partials, double max_norm, double* red) {
    return gn_coef_of(gn_block_sum(partials[threadIdx.x], red), max_norm);     // blockDim.x == GN_THREADS == GN_SLOTS
}
// clip_out = [coef, norm, finite, 0]; stats (doubles) = [steps, clipped steps, skipped steps, largest finite norm]
__device__ __forceinline__ void gn_report(const ClipCoef& c, bool skipped, float* clip_out, double* stats) {
    if (clip_out) { clip_out[0] = c.coef; clip_out[1] = (float)c.norm; clip_out[2] = c.finite ? 1.f : 0.f; clip_out[3] = 0.f; }
    if (stats) {
        stats[0] += 1.0;
        if (skipped) stats[2] += 1.0;
        else if (c.coef < 1.0f) stats[1] += 1.0;
        if (c.finite && c.norm > stats[3]) stats[3] = c.norm;
    }
}

// ------------------------------------------------------------------------------ Adam / AdamW
// The bias correction of update `step`, as the kernels take it.
struct AdamBias { float step_size, inv_sqrt_bc2; };
// from the two powers beta1^t and beta2^t (double): each factor is rounded to fp32 once
__host__ __device__ inline AdamBias adam_bias_of(float lr, double pow1, double pow2) {
    const double bc1 = 1.0 - pow1;
    const double bc2 = 1.0 - pow2;
    return {(float)((double)lr / bc1), (float)(1.0 / sqrt(bc2))};
}
inline AdamBias adam_bias(float lr, float beta1, float beta2, int step) {
    return adam_bias_of(lr, pow((double)beta1, (double)step), pow((double)beta2, (double)step));
}
// beta^t on the device (the landed count t is known only there): the integer power by squaring, in double.  Neither a device pow nor a
// running product: a product kept across steps would be one more word of state per (group, beta) pair that a checkpoint has to carry
// and a skipped step must not touch, and ocml's pow is a few hundred instructions whose last bit is not the host's pow's either.  This
// is at most 2 * 31 multiplications, each within 2^-53: beta^t within 7e-15 relative, far below the fp32 rounding of the factors.
__device__ __forceinline__ double ipow(double b, int t) {
    double r = 1.0;
    for (; t > 0; t >>= 1) { if (t & 1) r *= b; b *= b; }
    return r;
}
// What dep_adam_step_ext adds, as the kernels take it: pointers are NULL for a part that is off (uniform over the launch).
struct AdamExt { float* vmax; float* ema; float ema_w; int ema_first; };   // ema_w = 1 - decay
// The update of element i, the ONE Adam expression of the library.  The caller loads pv = p[i] and gv = g[i] (the clipped kernels: times
// the clip coefficient; g * 1.0f is exact, so a coefficient of one gives the plain step's bits) in that order and passes the values.
// EXT (dep_adam_step_ext): AMSGrad puts max(vmax, v) in v's place under the root; the average follows the stored parameter,
// ema += w * (p_new - ema) in one fma (p_new == ema: ema + w * 0 keeps ema), or ema = p_new without reading ema when `first`.
template <bool EXT>
__device__ __forceinline__ void adam_element(float pv, float gv, float* __restrict__ p, float* __restrict__ m, float* __restrict__ v,
                                             long i, float lr, float b1, float b2, float eps, float wd, int decoupled, float step_size,
                                             float inv_sqrt_bc2, const AdamExt& x) {
    // The fused products are written out (fmaf): they are the ones the compiler chose for adam_kernel and adam_clipped_kernel under the
    // default contraction, where left to itself it fused the OTHER product of m in the EXT instances -- and an AMSGrad step whose
    // maximum is v itself has to give the plain step's bits.  v is two products and a sum in every instance (tools/isa_diff.py).
    if (decoupled) pv *= fmaf(-lr, wd, 1.0f);
    else if (wd != 0.f) gv = fmaf(wd, pv, gv);
    const float mv = fmaf(b1, m[i], (1.0f - b1) * gv);
    const float vv = b2 * v[i] + (1.0f - b2) * gv * gv;
    m[i] = mv; v[i] = vv;
    float dv = vv;
    if (EXT && x.vmax) { dv = fmaxf(x.vmax[i], vv); x.vmax[i] = dv; }
    const float denom = fmaf(sqrtf(dv), inv_sqrt_bc2, eps);
    const float pn = fmaf(-step_size, mv / denom, pv);
    p[i] = pn;
    if (EXT && x.ema) x.ema[i] = x.ema_first ? pn : fmaf(x.ema_w, pn - x.ema[i], x.ema[i]);
}

// the body of the plain kernels: one element per thread
template <bool EXT>
__device__ __forceinline__ void adam_plain_body(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                float* __restrict__ v, long n, float lr, float b1, float b2, float eps, float wd,
                                                int decoupled, float step_size, float inv_sqrt_bc2, const AdamExt& x) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float pv = p[i], gv = g[i];
    adam_element<EXT>(pv, gv, p, m, v, i, lr, b1, b2, eps, wd, decoupled, step_size, inv_sqrt_bc2, x);
}
__global__ void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                            float* __restrict__ v, long n, float lr, float b1, float b2, float eps, float wd,
                            int decoupled, float step_size, float inv_sqrt_bc2) {
    adam_plain_body<false>(p, g, m, v, n, lr, b1, b2, eps, wd, decoupled, step_size, inv_sqrt_bc2, AdamExt{});
}
__global__ void adam_ext_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                float* __restrict__ v, long n, float lr, float b1, float b2, float eps, float wd,
                                int decoupled, float step_size, float inv_sqrt_bc2, AdamExt x) {
    adam_plain_body<true>(p, g, m, v, n, lr, b1, b2, eps, wd, decoupled, step_size, inv_sqrt_bc2, x);
}

constexpr int AC_PER_THREAD = 8;           // elements per thread: the partials are re-summed once per 2048 elements
// the body of the clipped kernels (GN_THREADS threads)
template <bool EXT>
__device__ __forceinline__ void adam_clipped_body(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                  float* __restrict__ v, long n, float lr, float b1, float b2, float eps, float wd,
                                                  int decoupled, float step_size, float inv_sqrt_bc2,
                                                  const double* __restrict__ partials, double max_norm, int skip_nonfinite,
                                                  float* clip_out, double* stats, const AdamExt& x) {
    __shared__ double red[4];
    const ClipCoef c = gn_coef(partials, max_norm, red);
    const bool skipped = skip_nonfinite && !c.finite;
    if (blockIdx.x == 0 && threadIdx.x == 0) gn_report(c, skipped, clip_out, stats);
    if (skipped) return;                                           // p, m, v (and vmax, ema) untouched
    const float coef = c.coef;
    const long base = (long)blockIdx.x * (GN_THREADS * AC_PER_THREAD) + threadIdx.x;
#pragma unroll
    for (int k = 0; k < AC_PER_THREAD; ++k) {
        const long i = base + (long)k * GN_THREADS;
        if (i >= n) break;
        const float pv = p[i], gv = g[i] * coef;
        adam_element<EXT>(pv, gv, p, m, v, i, lr, b1, b2, eps, wd, decoupled, step_size, inv_sqrt_bc2, x);
    }
}
__global__ __launch_bounds__(GN_THREADS) void adam_clipped_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                                  float* __restrict__ m, float* __restrict__ v, long n, float lr,
                                                                  float b1, float b2, float eps, float wd, int decoupled,
                                                                  float step_size, float inv_sqrt_bc2,
                                                                  const double* __restrict__ partials, double max_norm,
                                                                  int skip_nonfinite, float* clip_out, double* stats) {
    adam_clipped_body<false>(p, g, m, v, n, lr, b1, b2, eps, wd, decoupled, step_size, inv_sqrt_bc2, partials, max_norm, skip_nonfinite,
                             clip_out, stats, AdamExt{});
}
__global__ __launch_bounds__(GN_THREADS) void adam_clipped_ext_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                                      float* __restrict__ m, float* __restrict__ v, long n, float lr,
                                                                      float b1, float b2, float eps, float wd, int decoupled,
                                                                      float step_size, float inv_sqrt_bc2,
                                                                      const double* __restrict__ partials, double max_norm,
                                                                      int skip_nonfinite, float* clip_out, double* stats, AdamExt x) {
    adam_clipped_body<true>(p, g, m, v, n, lr, b1, b2, eps, wd, decoupled, step_size, inv_sqrt_bc2, partials, max_norm, skip_nonfinite,
                            clip_out, stats, x);
}

// ------------------------------------------------------------------------------ value clamp, per-group norms, landed count
constexpr int GN_MAXG = 8;                 // param groups with a norm of their own
// Tensor.clamp_(-c, c) by comparisons: a NaN fails both and stays, +-inf becomes +-c, -0.0f stays -0.0f
__device__ __forceinline__ float clamp_value(float x, float c) { return x > c ? c : (x < -c ? -c : x); }
// What dep_adam_step_opt adds, as the kernels take it (everything uniform over the launch).
struct AdamOpt {
    float clamp;                           // > 0: gv = clamp_value(g * coef, clamp); 0: off
    int ngroups, group;                    // partials holds ngroups slices of GN_SLOTS doubles; this launch updates a range of `group`
    double max_norm[GN_MAXG];              // kernel_max_norm of every group's bound
    float* group_out;                      // [coef_g, norm_g] per group, or NULL: written by workgroup 0 (the step's first launch)
    const int* landed_in;                  // updates landed before this step, or NULL: the bias factors are the host's
    int* landed_out;                       // where workgroup 0 leaves the count after this step, or NULL; never landed_in
};
// The body of dep_adam_step_opt's kernels (GN_THREADS threads, AC_PER_THREAD elements each, as adam_clipped_body).  partials == NULL:
// coefficient 1, no record.  Otherwise every workgroup sums EVERY group's slice with gn_coef's tree (a __syncthreads between two
// uses of `red`): its own group's coefficient scales g, "any S_g not finite" skips the whole step, and workgroup 0 writes the record
// -- the top level as adam_clipped_body writes it, from the smallest coefficient and sqrt(sum of S_g); one group: those ARE
// gn_coef's values, and the bits of adam_clipped_body follow.  The landed count is read from landed_in by everyone and written to
// landed_out (another word) by workgroup 0: nothing reads what a workgroup of this launch, or of another launch of the step, writes.
template <bool EXT>
__device__ __forceinline__ void adam_opt_body(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                              float* __restrict__ v, long n, float lr, float b1, float b2, float eps, float wd,
                                              int decoupled, float step_size, float inv_sqrt_bc2,
                                              const double* __restrict__ partials, int skip_nonfinite, float* clip_out, double* stats,
                                              const AdamOpt& o, const AdamExt& x) {
    __shared__ double red[4];
    const bool writer = blockIdx.x == 0 && threadIdx.x == 0;
    float coef = 1.0f;
    bool skipped = false;
    if (partials) {                                                // uniform over the grid
        ClipCoef top{1.0f, 0.0, true};
        double Ssum = 0.0;
        bool any_nan = false;
        float nan_coef = 0.f;
        for (int k = 0; k < o.ngroups; ++k) {
            if (k) __syncthreads();                                // everyone has read red[] of the previous group
            const double S = gn_block_sum(partials[(long)k * GN_SLOTS + threadIdx.x], red);
            const ClipCoef c = gn_coef_of(S, o.max_norm[k]);
            if (k == o.group) coef = c.coef;
            if (c.coef != c.coef) { any_nan = true; nan_coef = c.coef; }               // (S NaN, no skip)
            else if (c.coef < top.coef) top.coef = c.coef;                             // the smallest; none is above 1
            top.finite = top.finite && c.finite;
            Ssum += S;
            if (writer && o.group_out) { o.group_out[2 * k] = c.coef; o.group_out[2 * k + 1] = (float)c.norm; }
        }
        top.norm = sqrt(Ssum);
        skipped = skip_nonfinite && !top.finite;
        if (writer) {
            // "clipped" counts a step in which any group's coefficient is below 1; a NaN coefficient of any group then shows in
            // clip_out[0] whatever the others are (one group: gn_report's own value, NaN < 1 being false there as well)
            gn_report(top, skipped, clip_out, stats);
            if (any_nan && clip_out) clip_out[0] = nan_coef;
        }
    }
    if (o.landed_in) {
        const int landed = *o.landed_in;
        if (writer && o.landed_out) *o.landed_out = skipped ? landed : landed + 1;
        if (!skipped) {                                            // this update lands as number landed + 1
            const AdamBias bc = adam_bias_of(lr, ipow((double)b1, landed + 1), ipow((double)b2, landed + 1));
            step_size = bc.step_size; inv_sqrt_bc2 = bc.inv_sqrt_bc2;
        }
    }
    if (skipped) return;                                           // p, m, v (and vmax, ema) untouched
    const float cl = o.clamp;
    const long base = (long)blockIdx.x * (GN_THREADS * AC_PER_THREAD) + threadIdx.x;
#pragma unroll
    for (int k = 0; k < AC_PER_THREAD; ++k) {
        const long i = base + (long)k * GN_THREADS;
        if (i >= n) break;
        const float pv = p[i];
        float gv = g[i] * coef;
        if (cl > 0.f) gv = clamp_value(gv, cl);
        adam_element<EXT>(pv, gv, p, m, v, i, lr, b1, b2, eps, wd, decoupled, step_size, inv_sqrt_bc2, x);
    }
}
__global__ __launch_bounds__(GN_THREADS) void adam_opt_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                              float* __restrict__ v, long n, float lr, float b1, float b2, float eps,
                                                              float wd, int decoupled, float step_size, float inv_sqrt_bc2,
                                                              const double* __restrict__ partials, int skip_nonfinite,
                                                              float* clip_out, double* stats, AdamOpt o) {
    adam_opt_body<false>(p, g, m, v, n, lr, b1, b2, eps, wd, decoupled, step_size, inv_sqrt_bc2, partials, skip_nonfinite, clip_out,
                         stats, o, AdamExt{});
}
__global__ __launch_bounds__(GN_THREADS) void adam_opt_ext_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                                  float* __restrict__ m, float* __restrict__ v, long n, float lr,
                                                                  float b1, float b2, float eps, float wd, int decoupled,
                                                                  float step_size, float inv_sqrt_bc2,
                                                                  const double* __restrict__ partials, int skip_nonfinite,
                                                                  float* clip_out, double* stats, AdamOpt o, AdamExt x) {
    adam_opt_body<true>(p, g, m, v, n, lr, b1, b2, eps, wd, decoupled, step_size, inv_sqrt_bc2, partials, skip_nonfinite, clip_out,
                        stats, o, x);
}

// g = clamp_value(g, c) in place over the ranges, blockIdx.y = range (torch.nn.utils.clip_grad_value_)
__global__ __launch_bounds__(GN_THREADS) void grad_clip_value_kernel(GradRangesRW R, float c) {
    float* __restrict__ gp = R.ptr[blockIdx.y];
    const long n = R.n[blockIdx.y], stride = (long)gridDim.x * GN_THREADS;
    for (long i = (long)blockIdx.x * GN_THREADS + threadIdx.x; i < n; i += stride) gp[i] = clamp_value(gp[i], c);
}

// a[i] <-> b[i] as 32-bit words (no arithmetic touches them): four per thread where four are left, one by one in the tail
__global__ __launch_bounds__(GN_THREADS) void swap_kernel(uint32_t* __restrict__ a, uint32_t* __restrict__ b, long n) {
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    const long i = ((long)blockIdx.x * GN_THREADS + threadIdx.x) * 4;
    if (i + 3 < n) {
        const u32x4 x = *reinterpret_cast<const u32x4*>(a + i), y = *reinterpret_cast<const u32x4*>(b + i);
        *reinterpret_cast<u32x4*>(a + i) = y; *reinterpret_cast<u32x4*>(b + i) = x;
    } else {
        for (long k = i; k < n; ++k) { const uint32_t x = a[k]; a[k] = b[k]; b[k] = x; }
    }
}

// g *= coef over the ranges, blockIdx.y = range (torch.nn.utils.clip_grad_norm_ leaves .grad clipped)
__global__ __launch_bounds__(GN_THREADS) void grad_clip_scale_kernel(GradRangesRW R, const double* __restrict__ partials,
                                                                     double max_norm, float* clip_out) {
    __shared__ double red[4];
    const ClipCoef c = gn_coef(partials, max_norm, red);
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) gn_report(c, false, clip_out, nullptr);
    const float coef = c.coef;
    if (coef == 1.0f) return;                                      // g * 1.0f is g
    float* __restrict__ gp = R.ptr[blockIdx.y];
    const long n = R.n[blockIdx.y], stride = (long)gridDim.x * GN_THREADS;
    for (long i = (long)blockIdx.x * GN_THREADS + threadIdx.x; i < n; i += stride) gp[i] = gp[i] * coef;
}

// the argument checks of the three entry points that take ranges: before any HIP call
int check_ranges(const float* const* bufs, const long* counts, int nranges) {
    DEP_CHECK_ARG(bufs && counts && nranges >= 1 && nranges <= GN_MAXR);
    for (int r = 0; r < nranges; ++r) DEP_CHECK_ARG(bufs[r] && counts[r] > 0 && ((uintptr_t)bufs[r] & 15) == 0);
    return DEP_OK;
}
// start[] of the concatenation the walk reads, and count
template <class Ranges>
void set_starts(Ranges& R, const long* counts, int nranges) {
    long at = 0;
    for (int r = 0; r < nranges; ++r) { R.start[r] = at; at += counts[r]; }
    for (int r = nranges; r <= GN_MAXR; ++r) R.start[r] = at;
    R.count = nranges;
}
// "measure only": max_norm <= 0 or +inf -> 0 for the kernels
// true when [a, a + n) and [b, b + n) floats share a byte
inline bool ranges_overlap(const float* a, const float* b, long n) {
    const uintptr_t ua = (uintptr_t)a, ub = (uintptr_t)b, bytes = (uintptr_t)n * sizeof(float);
    return ua < ub + bytes && ub < ua + bytes;
}
inline double kernel_max_norm(float max_norm) { return (max_norm > 0.f && max_norm <= 3.402823466e38f) ? (double)max_norm : 0.0; }

}  // namespace

#define S_ ((hipStream_t)stream)

extern "C" int dep_grad_norm_slots(void) { return GN_SLOTS; }
extern "C" int dep_grad_norm_chunk(void) { return GN_CHUNK; }

extern "C" int dep_grad_sqnorm(const float* const* bufs, const long* counts, int nranges, double* partials, void* stream) {
    if (int rc = check_ranges(bufs, counts, nranges)) return rc;
    DEP_CHECK_ARG(partials);
    GradRanges R{};
    for (int r = 0; r < nranges; ++r) R.ptr[r] = bufs[r];
    set_starts(R, counts, nranges);
    DEP_LAUNCH(grad_sqnorm_kernel, dim3(GN_SLOTS), dim3(GN_THREADS), 0, S_, R, partials);
    DEP_CHECK_LAUNCH();
    return DEP_OK;
}

extern "C" int dep_grad_accumulate(float* const* acc, const float* const* g, const long* counts, int nranges, float scale, int first,
                                   double* partials, void* stream) {
    if (int rc = check_ranges(g, counts, nranges)) return rc;
    DEP_CHECK_ARG(acc && scale == scale);
    for (int r = 0; r < nranges; ++r) DEP_CHECK_ARG(acc[r] && ((uintptr_t)acc[r] & 15) == 0);
    AccumRanges R{};
    for (int r = 0; r < nranges; ++r) { R.acc[r] = acc[r]; R.g[r] = g[r]; }
    set_starts(R, counts, nranges);
    DEP_LAUNCH(grad_accumulate_kernel, dim3(GN_SLOTS), dim3(GN_THREADS), 0, S_, R, scale, first ? 1 : 0, partials);
    DEP_CHECK_LAUNCH();
    return DEP_OK;
}

// The launches of the three Adam entry points.  x == NULL: the kernels dep_adam_step / dep_adam_step_clipped always launched.
static int adam_launch(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2, float eps,
                       float weight_decay, int decoupled, int step, const AdamExt* x, void* stream) {
    const AdamBias bc = adam_bias(lr, beta1, beta2, step);
    if (x)
        DEP_LAUNCH(adam_ext_kernel, dim3(dep_cdiv(n, 256)), dim3(256), 0, S_, p, g, m, v, n, lr, beta1, beta2, eps, weight_decay,
                   decoupled, bc.step_size, bc.inv_sqrt_bc2, *x);
    else
        DEP_LAUNCH(adam_kernel, dim3(dep_cdiv(n, 256)), dim3(256), 0, S_, p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, decoupled,
                   bc.step_size, bc.inv_sqrt_bc2);
    DEP_CHECK_LAUNCH();
    return DEP_OK;
}
static int adam_clipped_launch(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2, float eps,
                               float weight_decay, int decoupled, int step, const AdamExt* x, const double* partials, float max_norm,
                               int skip_nonfinite, float* clip_out, double* stats, void* stream) {
    const AdamBias bc = adam_bias(lr, beta1, beta2, step);
    const dim3 grid(dep_cdiv(n, GN_THREADS * AC_PER_THREAD));
    if (x)
        DEP_LAUNCH(adam_clipped_ext_kernel, grid, dim3(GN_THREADS), 0, S_, p, g, m, v, n, lr, beta1, beta2, eps, weight_decay,
                   decoupled, bc.step_size, bc.inv_sqrt_bc2, partials, kernel_max_norm(max_norm), skip_nonfinite, clip_out, stats, *x);
    else
        DEP_LAUNCH(adam_clipped_kernel, grid, dim3(GN_THREADS), 0, S_, p, g, m, v, n, lr,
                   beta1, beta2, eps, weight_decay, decoupled, bc.step_size, bc.inv_sqrt_bc2, partials, kernel_max_norm(max_norm),
                   skip_nonfinite, clip_out, stats);
    DEP_CHECK_LAUNCH();
    return DEP_OK;
}

extern "C" int dep_adam_step(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2,
                             float eps, float weight_decay, int decoupled, int step, void* stream) {
    DEP_CHECK_ARG(p && g && m && v && n > 0 && step >= 1);
    return adam_launch(p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, decoupled, step, nullptr, stream);
}

extern "C" int dep_adam_step_clipped(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2,
                                     float eps, float weight_decay, int decoupled, int step, const double* partials,
                                     float max_norm, int skip_nonfinite, float* clip_out, double* stats, void* stream) {
    DEP_CHECK_ARG(p && g && m && v && n > 0 && step >= 1 && partials && max_norm == max_norm);
    return adam_clipped_launch(p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, decoupled, step, nullptr, partials, max_norm,
                               skip_nonfinite, clip_out, stats, stream);
}

// dep_adam_ext as the kernels take it, after its checks; on = false: nothing of it is switched on
static int adam_ext_args(const float* p, const float* g, const float* m, const float* v, long n, const dep_adam_ext* ext, AdamExt& x,
                         bool& on) {
    on = false;
    if (ext && (ext->vmax || ext->ema)) {
        const float* const others[4] = {p, g, m, v};
        if (ext->vmax)
            for (const float* o : others) DEP_CHECK_ARG(!ranges_overlap(ext->vmax, o, n));
        if (ext->ema) {
            DEP_CHECK_ARG(ext->ema_decay >= 0.f && ext->ema_decay < 1.f);              // false for a NaN
            for (const float* o : others) DEP_CHECK_ARG(!ranges_overlap(ext->ema, o, n));
            if (ext->vmax) DEP_CHECK_ARG(!ranges_overlap(ext->ema, ext->vmax, n));
        }
        // a decay of zero is "the average is the parameter": e + 1 * (p - e) rounds twice, the `first` form is exact
        x = AdamExt{ext->vmax, ext->ema, 1.0f - ext->ema_decay, (ext->ema_first || ext->ema_decay == 0.f) ? 1 : 0};
        on = true;
    }
    return DEP_OK;
}

extern "C" int dep_adam_step_ext(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2, float eps,
                                 float weight_decay, int decoupled, int step, const dep_adam_ext* ext, const double* partials,
                                 float max_norm, int skip_nonfinite, float* clip_out, double* stats, void* stream) {
    DEP_CHECK_ARG(p && g && m && v && n > 0 && step >= 1);
    if (partials) DEP_CHECK_ARG(max_norm == max_norm);
    AdamExt x{};
    bool on = false;
    if (int rc = adam_ext_args(p, g, m, v, n, ext, x, on)) return rc;
    // nothing switched on: the launches (and so the bits) of the two entry points above
    if (partials)
        return adam_clipped_launch(p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, decoupled, step, on ? &x : nullptr, partials,
                                   max_norm, skip_nonfinite, clip_out, stats, stream);
    return adam_launch(p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, decoupled, step, on ? &x : nullptr, stream);
}

extern "C" int dep_adam_step_opt(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2, float eps,
                                 float weight_decay, int decoupled, int step, const dep_adam_ext* ext, const double* partials,
                                 float max_norm, int skip_nonfinite, float* clip_out, double* stats, const dep_adam_opt* opt,
                                 void* stream) {
    const bool off = !opt || (opt->max_grad_value == 0.f && opt->ngroups == 1 && opt->group == 0 && !opt->group_out &&
                              !opt->landed_in && !opt->landed_out);
    if (off)                                                       // dep_adam_step_ext: its checks, its launches, its bits
        return dep_adam_step_ext(p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, decoupled, step, ext, partials, max_norm,
                                 skip_nonfinite, clip_out, stats, stream);
    DEP_CHECK_ARG(p && g && m && v && n > 0 && step >= 1);
    DEP_CHECK_ARG(opt->max_grad_value >= 0.f && opt->max_grad_value <= 3.402823466e38f);      // false for a NaN
    DEP_CHECK_ARG(opt->ngroups >= 1 && opt->ngroups <= GN_MAXG && opt->group >= 0 && opt->group < opt->ngroups);
    DEP_CHECK_ARG(opt->ngroups == 1 || (partials && opt->group_max_norm));
    DEP_CHECK_ARG(!opt->group_out || partials);
    DEP_CHECK_ARG(!opt->landed_in || (partials && skip_nonfinite));
    DEP_CHECK_ARG(!opt->landed_out || (opt->landed_in && opt->landed_out != opt->landed_in));
    AdamOpt o{};
    o.clamp = opt->max_grad_value; o.ngroups = opt->ngroups; o.group = opt->group;
    o.group_out = opt->group_out; o.landed_in = opt->landed_in; o.landed_out = opt->landed_out;
    if (partials) {
        for (int k = 0; k < o.ngroups; ++k) {
            const float mx = opt->group_max_norm ? opt->group_max_norm[k] : max_norm;      // (NULL: ngroups == 1, checked above)
            DEP_CHECK_ARG(mx == mx);
            o.max_norm[k] = kernel_max_norm(mx);
        }
    }
    AdamExt x{};
    bool on = false;
    if (int rc = adam_ext_args(p, g, m, v, n, ext, x, on)) return rc;
    const AdamBias bc = adam_bias(lr, beta1, beta2, step);          // replaced on the device when landed_in is given
    const dim3 grid(dep_cdiv(n, GN_THREADS * AC_PER_THREAD));
    if (on)
        DEP_LAUNCH(adam_opt_ext_kernel, grid, dim3(GN_THREADS), 0, S_, p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, decoupled,
                   bc.step_size, bc.inv_sqrt_bc2, partials, partials ? skip_nonfinite : 0, clip_out, stats, o, x);
    else
        DEP_LAUNCH(adam_opt_kernel, grid, dim3(GN_THREADS), 0, S_, p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, decoupled,
                   bc.step_size, bc.inv_sqrt_bc2, partials, partials ? skip_nonfinite : 0, clip_out, stats, o);
    DEP_CHECK_LAUNCH();
    return DEP_OK;
}

extern "C" int dep_grad_clip_value(float* const* bufs, const long* counts, int nranges, float clip_value, void* stream) {
    if (int rc = check_ranges(bufs, counts, nranges)) return rc;
    DEP_CHECK_ARG(clip_value > 0.f && clip_value <= 3.402823466e38f);                          // false for a NaN
    GradRangesRW R{};
    long mx = 0;
    for (int r = 0; r < nranges; ++r) { R.ptr[r] = bufs[r]; R.n[r] = counts[r]; if (counts[r] > mx) mx = counts[r]; }
    R.count = nranges;
    int gx = dep_cdiv(mx, GN_THREADS * 4); if (gx > 512) gx = 512;
    DEP_LAUNCH(grad_clip_value_kernel, dim3(gx, nranges), dim3(GN_THREADS), 0, S_, R, clip_value);
    DEP_CHECK_LAUNCH();
    return DEP_OK;
}

extern "C" int dep_swap(float* a, float* b, long n, void* stream) {
    DEP_CHECK_ARG(a && b && n > 0 && (((uintptr_t)a | (uintptr_t)b) & 15) == 0 && !ranges_overlap(a, b, n));
    DEP_LAUNCH(swap_kernel, dim3(dep_cdiv(dep_cdiv(n, 4), GN_THREADS)), dim3(GN_THREADS), 0, S_, reinterpret_cast<uint32_t*>(a),
               reinterpret_cast<uint32_t*>(b), n);
    DEP_CHECK_LAUNCH();
    return DEP_OK;
}

extern "C" int dep_grad_clip_scale(float* const* bufs, const long* counts, int nranges, const double* partials, float max_norm,
                                   float* clip_out, void* stream) {
    if (int rc = check_ranges(bufs, counts, nranges)) return rc;
    DEP_CHECK_ARG(partials && max_norm == max_norm);
    GradRangesRW R{};
    long mx = 0;
    for (int r = 0; r < nranges; ++r) { R.ptr[r] = bufs[r]; R.n[r] = counts[r]; if (counts[r] > mx) mx = counts[r]; }
    R.count = nranges;
    int gx = dep_cdiv(mx, GN_THREADS * 4); if (gx > 512) gx = 512;
    DEP_LAUNCH(grad_clip_scale_kernel, dim3(gx, nranges), dim3(GN_THREADS), 0, S_, R, partials, kernel_max_norm(max_norm), clip_out);
    DEP_CHECK_LAUNCH();
    return DEP_OK;
}
