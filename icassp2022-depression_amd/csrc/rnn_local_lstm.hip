// Exchange-free forward sweep of the (Bi)LSTM at H = 128 (impl = 8; nn.LSTM gates i,f,g,o).  ONE workgroup owns a (direction,
// 16-utterance tile) AND the whole recurrent weight of its direction: wave w of eight keeps the W_hh rows of hidden units
// [16w, 16w+16), all four gates and all of K, in 128 VGPRs for the whole sweep, so nothing crosses CUs per step -- no exchange buffer,
// no hello, no flags, no spins, no status word, and no assumption about what else runs on the card.  h_t travels through LDS, double-
// buffered by step parity, behind ONE workgroup barrier per step; c stays in registers.  A lane (j = lane & 15, q = lane >> 4) holds
// units 16w + 4q .. + 3 of utterance j, all four gates (A = W_hh rows, B = h^T, as in lstm_fwd_cluster), so the gate phase needs no
// shuffle and every HBM access of a lane is one 16-byte piece: four loads of the input projection per step, prefetched PF steps
// ahead into registers, and the posted stores of h and dropout(h).  Both biases are folded into the input projection by the caller.
// Forward only: it saves no gates.  Recurrent state in (hx, cx: the prologue) and out (h_n, c_n) costs nothing here.
//
// impl = 9 adds the training pair of the same family: lstm_fwd_save_local, the same step body with five more posted 16-byte stores per
// lane and step (the four activated gates and c_t, which the lane holds in registers anyway), and lstm_bwd_local, the BPTT sweep below
// -- again one workgroup per (direction, tile) and nothing across CUs.
#include <limits.h>
#include "rnn_cluster_launch.h"

namespace {
using namespace depc;

struct LL {
    int B, T, H, dirs, nbtp, b0;      // one launch covers the batch: b0 = 0, nbtp = tiles padded to whole groups of 8 (launch_chunks)
    const f32x4* wp[2];
    const float* gi; int ldgi;
    float* y; int ldy;                 // null: not kept (a lower layer of a dropout-only stack)
    float* ydrop; float drop_p, drop_scale; uint64_t seed; uint32_t site;
    const float* hx; const float* cx;  // (dirs,B,H) state before the first step, or null = zeros; may be the buffers of h_n / c_n
    float* h_n; float* c_n;
    const int* lengths;                // ragged instances (RAG): row b is live for t < lengths[b]
    float* svg; float* svc;            // saving instances (SAVE): activated gates (B,T,dirs*4H) and cell state (B,T,dirs*H) of every step
};

constexpr int LL_H = 128;
constexpr int LL_THREADS = 512;                      // eight compute waves, two per SIMD
constexpr int LL_PF = 2;                             // steps the input projection is requested ahead of its use (a register ring)
constexpr int LL_KS = LL_H / 32;                     // SPLIT: k-steps of 32
constexpr int LL_KC = LL_H / 16;                     // !SPLIT: k-chunks of 16
constexpr int LL_LDH = LL_H + LPAD;                  // !SPLIT: row stride of the fp32 h plane
constexpr int LL_FRAG_BYTES = 2 * LL_KS * 64 * 16;   // SPLIT: one parity of h as B fragments, [plane hi / lo][k-step][64 lanes][16 B] = 8 KB
constexpr size_t LL_LDS_SPLIT = 2 * (size_t)LL_FRAG_BYTES;
constexpr size_t LL_LDS_EXACT = 2 * (size_t)BT * LL_LDH * sizeof(float);

// SPLIT: the recurrent products on the bf16 matrix cores with the 3-term split (hi*lo + lo*hi + hi*hi): 48 v_mfma_f32_16x16x32_bf16 per
// wave and step on the forward image of pack_lstm_split_kernel, of which a wave reads both K halves of its tile jt = w.  A lane publishes
// its four units as two (hi, lo) word pairs straight into the B-fragment order the MFMAs read (8 bytes per plane, conflict-free), and
// every wave reads the four k-steps of both planes back: 128 B per lane.
// !SPLIT: exact fp32, 128 v_mfma_f32_16x16x4_f32 per wave and step on the fragment image of dep_pack_whh; h is an fp32 LDS plane.
// RAG: live = t < lengths[b] per lane, as in lstm_fwd_cluster: (h, c) = live ? new : previous is what is published, carried and returned,
// h and dropout(h) go out as 0 at dead positions, the reverse direction walks its padding with the initial state.
// SAVE: the step also stores i, f, g, o and c_t for the backward (lstm_bwd_local); a dead position saves zero gates and c = 0, as
// lstm_fwd_cluster<.., RAG> saves its c (the backward reads c_{t-1} there).  Same arithmetic, same bits in everything else.
template <bool SPLIT, bool RAG, bool SAVE>
__device__ __forceinline__ void lstm_fwd_local_body(const LL& p) {
    // contraction by syntax: see DEP_FP_CONTRACT_NOTE in dep_common.h
#pragma clang fp contract(on)
    extern __shared__ __attribute__((aligned(16))) float smem[];
    typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
    constexpr int H = LL_H;
    const int T = p.T;
    const int bt = blockIdx.x % p.nbtp, dir = blockIdx.x / p.nbtp;
    if (p.b0 + bt * BT >= p.B) return;                // (whole workgroup: the padding tiles of the grid)
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int j = lane & 15, q = lane >> 4;
    const int col = 16 * w + 4 * q;
    const int b = p.b0 + bt * BT + j;
    const bool valid = b < p.B;
    int len = T;
    if constexpr (RAG) len = valid ? dep_row_len(p.lengths, b, T) : 0;

    f32x4 wr[SPLIT ? 1 : 4][SPLIT ? 1 : LL_KC];
    u32x4 wq[SPLIT ? 4 : 1][SPLIT ? LL_KS : 1][2];    // [gate][k-step][hi, lo]
    if constexpr (SPLIT) {
        const u32x4* wpq = reinterpret_cast<const u32x4*>(p.wp[dir]);
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int ks = 0; ks < LL_KS; ++ks)          // (k-step ks = 2 kh + ks' of the image's K halves)
#pragma unroll
                for (int pl = 0; pl < 2; ++pl)
                    wq[g][ks][pl] = wpq[(size_t)(((w * 4 + g) * LL_KS + ks) * 2 + pl) * 64 + lane];
    } else {
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int k = 0; k < LL_KC; ++k)
                wr[g][k] = p.wp[dir][(size_t)((w * 4 + g) * LL_KC + k) * 64 + lane];
    }

    // this lane's four units of h_t -> the parity's LDS image
    char* const fragw = reinterpret_cast<char*>(smem) + (w >> 1) * 1024 + ((2 * (w & 1) + (q >> 1)) * 16 + j) * 16 + (q & 1) * 8;
    auto publish = [&](int par, const f32x4& h) {
        if constexpr (SPLIT) {
            unsigned h0, l0, h1, l1;
            split_pair(h[0], h[1], h0, l0); split_pair(h[2], h[3], h1, l1);
            const u32x2 hv = {h0, h1}, lv = {l0, l1};
            *reinterpret_cast<u32x2*>(fragw + par * LL_FRAG_BYTES) = hv;
            *reinterpret_cast<u32x2*>(fragw + par * LL_FRAG_BYTES + LL_KS * 1024) = lv;
        } else {
            *reinterpret_cast<f32x4*>(smem + par * BT * LL_LDH + j * LL_LDH + col) = h;
        }
    };

    // state before the first step: the direction's own slices, ordered like h_n; rows past B of the last tile read nothing
    const size_t so = ((size_t)dir * p.B + b) * H + col;
    f32x4 c = (p.cx && valid) ? ld4(p.cx + so) : zero4();
    f32x4 hlast = (p.hx && valid) ? ld4(p.hx + so) : zero4();
    publish(0, hlast);

    const float* const gbase = p.gi + (size_t)dir * 4 * H + col;
    auto gload = [&](int s, f32x4 (&dst)[4]) {          // input projection of sweep step s (zeros past the sweep and past the batch)
        const bool on = valid && s < T;
        const float* src = gbase + ((size_t)b * T + (dir ? T - 1 - s : s)) * p.ldgi;
#pragma unroll
        for (int g = 0; g < 4; ++g) dst[g] = on ? ld4(src + g * H) : zero4();
    };
    f32x4 gq[LL_PF][4];
#pragma unroll
    for (int u = 0; u < LL_PF; ++u) gload(u, gq[u]);
    __syncthreads();

    auto step = [&](int s, f32x4 (&gi)[4]) {
        const int t = dir ? T - 1 - s : s;
        const bool more = s + 1 < T;
        f32x4 acc[4] = {zero4(), zero4(), zero4(), zero4()};
        if constexpr (SPLIT) {
            const u32x4* hf = reinterpret_cast<const u32x4*>(reinterpret_cast<const char*>(smem) + (s & 1) * LL_FRAG_BYTES) + lane;
            u32x4 hfr[LL_KS][2];
#pragma unroll
            for (int ks = 0; ks < LL_KS; ++ks)
#pragma unroll
                for (int pl = 0; pl < 2; ++pl) hfr[ks][pl] = hf[(pl * LL_KS + ks) * 64];
#pragma unroll
            for (int ks = 0; ks < LL_KS; ++ks) {
                const bf16x8 hh = __builtin_bit_cast(bf16x8, hfr[ks][0]), hl = __builtin_bit_cast(bf16x8, hfr[ks][1]);
                // (the four gates' accumulators interleaved: a dependent MFMA is three independent ones away)
#pragma unroll
                for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wq[g][ks][0]), hl, acc[g], 0, 0, 0);
#pragma unroll
                for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wq[g][ks][1]), hh, acc[g], 0, 0, 0);
#pragma unroll
                for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wq[g][ks][0]), hh, acc[g], 0, 0, 0);
            }
        } else {
            const float* hrow = smem + (s & 1) * BT * LL_LDH + j * LL_LDH + q * 4;
            f32x4 hv[LL_KC];
#pragma unroll
            for (int k = 0; k < LL_KC; ++k) hv[k] = ld4(hrow + k * 16);
#pragma unroll
            for (int k = 0; k < LL_KC; ++k)
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int g = 0; g < 4; ++g)
                        acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[g][k][e], hv[k][e], acc[g], 0, 0, 0);
        }
        f32x4 h, cn;
        f32x4 sg[SAVE ? 4 : 1];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float ig = fast_sigmoid(acc[0][e] + gi[0][e]);
            const float fg = fast_sigmoid(acc[1][e] + gi[1][e]);
            const float gg = fast_tanh(acc[2][e] + gi[2][e]);
            const float og = fast_sigmoid(acc[3][e] + gi[3][e]);
            cn[e] = fg * c[e] + ig * gg;
            h[e] = og * fast_tanh(cn[e]);
            if constexpr (SAVE) { sg[0][e] = ig; sg[1][e] = fg; sg[2][e] = gg; sg[3][e] = og; }
        }
        if constexpr (SAVE) {
            if (valid) {
                f32x4 cs = cn;
                if constexpr (RAG) {
                    const bool live = t < len;
#pragma unroll
                    for (int g = 0; g < 4; ++g) sg[g] = dep_sel4(live, sg[g], zero4());
                    cs = dep_sel4(live, cn, zero4());
                }
                const size_t row = (size_t)b * T + t;
                float* gs = p.svg + row * ((size_t)p.dirs * 4 * H) + (size_t)dir * 4 * H + col;
#pragma unroll
                for (int g = 0; g < 4; ++g) *reinterpret_cast<f32x4*>(gs + g * H) = sg[g];
                *reinterpret_cast<f32x4*>(p.svc + row * ((size_t)p.dirs * H) + (size_t)dir * H + col) = cs;
            }
        }
        f32x4 hy = h;                                   // what y and dropout(y) show of this step
        if constexpr (RAG) {
            const bool live = t < len;
            hlast = dep_sel4(live, h, hlast); c = dep_sel4(live, cn, c);
            hy = dep_sel4(live, h, zero4());
        } else {
            hlast = h; c = cn;
        }
        if (more) publish((s + 1) & 1, hlast);          // (the other parity: a wave still reading this step's fragments is not disturbed)
        if (valid) {
            const size_t o = ((size_t)b * T + t) * p.ldy + (size_t)dir * H + col;
            if (p.y) *reinterpret_cast<f32x4*>(p.y + o) = hy;
            if (p.ydrop) *reinterpret_cast<f32x4*>(p.ydrop + o) = hy * dep_dropmask4(p.seed, p.site, o >> 2, p.drop_p, p.drop_scale);
        }
        gload(s + LL_PF, gi);                           // this slot's next tenant
        if (more) bar_lds();                            // the ONE barrier of the step: h_t is in LDS (global stores stay in flight)
    };
    for (int s0 = 0; s0 < T; s0 += LL_PF) {
#pragma unroll
        for (int u = 0; u < LL_PF; ++u)
            if (s0 + u < T) step(s0 + u, gq[u]);        // (workgroup-uniform)
    }
    if (valid) {
        if (p.h_n) *reinterpret_cast<f32x4*>(p.h_n + so) = hlast;
        if (p.c_n) *reinterpret_cast<f32x4*>(p.c_n + so) = c;
    }
}

// one step body behind two kernel names: the forwards no backward follows (impl 8, and impl 9 outside DEP_RUN_TRAIN) ...
template <bool SPLIT, bool RAG>
__global__ __launch_bounds__(LL_THREADS) void lstm_fwd_local(LL p) { lstm_fwd_local_body<SPLIT, RAG, false>(p); }
// ... and the DEP_RUN_TRAIN forward of impl 9
template <bool SPLIT, bool RAG>
__global__ __launch_bounds__(LL_THREADS) void lstm_fwd_save_local(LL p) { lstm_fwd_local_body<SPLIT, RAG, true>(p); }

// =============================================================================== backward (impl = 9)
// BPTT of one (direction, 16-utterance tile) per workgroup: sweep step k is t = T-1-k for direction 0 and t = k for direction 1.  FOUR
// waves, one per SIMD, each with the SIMD's whole register file: wave w keeps W_hh^T for the output units [32w, 32w+32) of dh -- two
// 16-unit tiles, all of K = 4H -- in 256 registers for the whole sweep.  A lane (j = lane & 15, q = lane >> 4) owns the units
// 32w + 16i + 4q .. + 3 (i = 0, 1) of utterance j: exactly the rows of the two MFMA result tiles it receives, so dh and dc are carried
// in registers, the gate phase needs no shuffle and every HBM access is one 16-byte piece (per piece and step: four gates, c, dy in; four
// gate gradients out).  c_prev of a step is c_t of the next one, so the 2-deep input ring holds it already.  The four gate gradients of
// a step go through LDS, double-buffered by step parity, behind ONE workgroup barrier per step.
//   dh = dy * mask + dh_rec ; tc = tanh(c_t) ; do~ = dh tc o(1-o) ; dc = dc_rec + dh o (1 - tc^2) ; di~ = dc g i(1-i) ;
//   df~ = dc c_prev f(1-f) ; dg~ = dc i (1-g^2) ; dc_rec = dc f ; dh_rec = W_hh^T [di~ df~ dg~ do~]
// SPLIT: the backward image of pack_lstm_split_kernel as it is, [member c][output tile][gate][hi, lo]: the 16 k-steps (c, g) of a tile are
// 32 units of gate g.  A lane publishes its pieces as (hi, lo) word pairs straight into B-fragment order ([plane][k-step][64 lanes][16 B],
// 8 bytes per store, conflict-free; wave w's units are member w's), every wave reads the 32 KB back once: 96 v_mfma_f32_16x16x32_bf16 per
// wave and step in eight independent chains (tile x member, summed in member order as lstm_bwd_cluster gathers its partials).
// !SPLIT: exact fp32 on the transposed fragment image of dep_pack_whh, 256 v_mfma_f32_16x16x4_f32 per wave and step, the gate gradients
// as an fp32 LDS plane; chains are (tile x gate).
// RAG: a dead step's gate gradients are exact zeros and dh, dc pass through it (selects, so dy is ignored there, not added).  The first
// forward step of a row -- sweep step T-1, or t = len-1 for direction 1 -- takes cx (or 0) as c_prev, not a neighbour's saved c.
struct LBL {
    int B, T, H, dirs, nbtp, b0;
    const f32x4* wp[2];
    const float* dy; int lddy;
    float drop_p, drop_scale; uint64_t seed; uint32_t site;
    const float* dh_n; const float* dc_n; const float* cx;      // (dirs,B,H) or null; a lane reads its own slices only, before it stores ...
    float* dhx; float* dcx;                                     // ... these, which may be the same buffers
    const float* svg; const float* svc;
    float* dgi; int lddg;
    float* dbpart; int nwg;
    const int* lengths;
};

constexpr int LBL_THREADS = 256;                     // four waves, one per SIMD
constexpr int LBL_PF = 2;                            // steps the inputs are requested ahead of their use (a register ring)
constexpr int LBL_NT = 2;                            // output tiles of dh per wave
constexpr int LBL_K = 4 * LL_H;                      // the contraction: four gates of H units
constexpr int LBL_KS = LBL_K / 32;                   // SPLIT: k-steps of 32 = (member, gate)
constexpr int LBL_KC = LBL_K / 16;                   // !SPLIT: k-chunks of 16
constexpr int LBL_PLANE_BYTES = LBL_KS * 64 * 16;    // SPLIT: one plane (hi or lo) of a step's gate gradients as B fragments = 16 KB
constexpr int LBL_FRAG_BYTES = 2 * LBL_PLANE_BYTES;
constexpr int LBL_LDG = LBL_K + LPAD;                // !SPLIT: row stride of the fp32 plane
constexpr size_t LBL_LDS_DB = (size_t)LBL_NT * 4 * LBL_THREADS * 16;      // every lane's bias partial sums, [piece][gate][thread][16 B]: own slots, conflict-free
constexpr size_t LBL_LDS_SPLIT = 2 * (size_t)LBL_FRAG_BYTES + LBL_LDS_DB;
constexpr size_t LBL_LDS_EXACT = 2 * (size_t)BT * LBL_LDG * sizeof(float) + LBL_LDS_DB;

struct LBLIn { f32x4 g[4], c, dy; };                // one piece's inputs of one step

template <bool SPLIT, bool RAG>
__global__ __launch_bounds__(LBL_THREADS) void lstm_bwd_local(LBL p) {
    // contraction by syntax (DEP_FP_CONTRACT_NOTE in dep_common.h): the dense and the ragged instance round alike
#pragma clang fp contract(on)
    extern __shared__ __attribute__((aligned(16))) float smem[];
    typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
    constexpr int H = LL_H;
    const int T = p.T;
    const int bt = blockIdx.x % p.nbtp, dir = blockIdx.x / p.nbtp;
    if (p.b0 + bt * BT >= p.B) return;                // (whole workgroup: the padding tiles of the grid)
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int j = lane & 15, q = lane >> 4;
    const int col0 = 32 * w + 4 * q;                  // piece i: units col0 + 16 i .. + 3
    const int b = p.b0 + bt * BT + j;
    const bool valid = b < p.B;
    int len = T;
    if constexpr (RAG) len = valid ? dep_row_len(p.lengths, b, T) : 0;
    const int ldsg = p.dirs * 4 * H, ldsc = p.dirs * H;

    f32x4 wr[SPLIT ? 1 : LBL_NT][SPLIT ? 1 : LBL_KC];
    u32x4 wq[SPLIT ? LBL_NT : 1][SPLIT ? 4 : 1][SPLIT ? 4 : 1][2];      // [tile][member][gate][hi, lo]
    if constexpr (SPLIT) {
        const u32x4* wpq = reinterpret_cast<const u32x4*>(p.wp[dir]);
#pragma unroll
        for (int i = 0; i < LBL_NT; ++i)
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int g = 0; g < 4; ++g)
#pragma unroll
                    for (int pl = 0; pl < 2; ++pl)
                        wq[i][c][g][pl] = wpq[(size_t)(((c * (H / 16) + w * LBL_NT + i) * 4 + g) * 2 + pl) * 64 + lane];
    } else {
#pragma unroll
        for (int i = 0; i < LBL_NT; ++i)
#pragma unroll
            for (int k = 0; k < LBL_KC; ++k)
                wr[i][k] = p.wp[dir][(size_t)((w * LBL_NT + i) * LBL_KC + k) * 64 + lane];
    }

    // the state gradients entering the sweep: this lane's own slices, ordered like h_n; rows past B of the last tile read nothing
    const size_t so = ((size_t)dir * p.B + b) * H + col0;
    // (the 32 bias partial sums of a lane live in LDS, each lane in slots of its own: with the weights' 256 registers, the ring's 96 and
    // the carried state they do not fit the file)
    f32x4* const dbs = reinterpret_cast<f32x4*>(reinterpret_cast<char*>(smem) + (SPLIT ? 2 * (size_t)LBL_FRAG_BYTES : 2 * (size_t)BT * LBL_LDG * sizeof(float))) + tid;
    f32x4 dh[LBL_NT], dc[LBL_NT];
#pragma unroll
    for (int i = 0; i < LBL_NT; ++i) {
        dh[i] = (p.dh_n && valid) ? ld4(p.dh_n + so + 16 * i) : zero4();
        dc[i] = (p.dc_n && valid) ? ld4(p.dc_n + so + 16 * i) : zero4();
#pragma unroll
        for (int g = 0; g < 4; ++g) dbs[(i * 4 + g) * LBL_THREADS] = zero4();
    }

    auto tstep = [&](int k) { return dir ? k : T - 1 - k; };
    auto gload = [&](int k, LBLIn (&dst)[LBL_NT]) {    // inputs of sweep step k (zeros past the sweep and past the batch)
        const bool on = valid && k < T;
        const size_t row = (size_t)b * T + tstep(k);
#pragma unroll
        for (int i = 0; i < LBL_NT; ++i) {
            const float* gs = p.svg + row * ldsg + (size_t)dir * 4 * H + col0 + 16 * i;
#pragma unroll
            for (int g = 0; g < 4; ++g) dst[i].g[g] = on ? ld4(gs + g * H) : zero4();
            dst[i].c = on ? ld4(p.svc + row * ldsc + (size_t)dir * H + col0 + 16 * i) : zero4();
            dst[i].dy = (on && p.dy) ? ld4(p.dy + row * p.lddy + (size_t)dir * H + col0 + 16 * i) : zero4();
        }
    };
    // the inter-layer dropout mask of the incoming dy: the forward's site / seed / element offset, drawn a step ahead under the MFMAs
    // and applied to the ring slot that waits for its step
    const bool masked = p.dy && p.drop_p > 0.f;         // (uniform)
    auto mask_dy = [&](int k, LBLIn (&slot)[LBL_NT]) {
        const size_t row = (size_t)b * T + tstep(k);
#pragma unroll
        for (int i = 0; i < LBL_NT; ++i) {
            const size_t o = row * p.lddy + (size_t)dir * H + col0 + 16 * i;
            slot[i].dy *= dep_dropmask4(p.seed, p.site, o >> 2, p.drop_p, p.drop_scale);
        }
    };

    LBLIn gq[LBL_PF][LBL_NT];
    static_assert(LBL_PF == 2, "the step reads c_prev from the other slot of the ring");
#pragma unroll
    for (int u = 0; u < LBL_PF; ++u) gload(u, gq[u]);
    if (masked) mask_dy(0, gq[0]);

    // this lane's piece i of the gate gradients -> the parity's LDS image (SPLIT: member w, k-group 2i + (q >> 1), words 2 (q & 1) ..)
    char* const fragw = reinterpret_cast<char*>(smem) + w * 4 * 1024 + ((q >> 1) * 16 + j) * 16 + (q & 1) * 8;

    auto step = [&](int k, LBLIn (&cur)[LBL_NT], LBLIn (&nxt)[LBL_NT]) {
        const int t = tstep(k), par = k & 1;
        const bool live = !RAG || t < len;
        const bool first = dir ? t == len - 1 : k == T - 1;      // the row's first FORWARD step: c_prev is the initial state
        const size_t row = (size_t)b * T + t;
#pragma unroll
        for (int i = 0; i < LBL_NT; ++i) {
            f32x4 cp = nxt[i].c;
            if (first) cp = (p.cx && valid) ? ld4(p.cx + so + 16 * i) : zero4();
            f32x4 dg[4], dcn;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float ig = cur[i].g[0][e], fg = cur[i].g[1][e], gg = cur[i].g[2][e], og = cur[i].g[3][e];
                const float d = cur[i].dy[e] + dh[i][e];
                const float tc = fast_tanh(cur[i].c[e]);
                const float dct = d * og * (1.0f - tc * tc) + dc[i][e];
                dg[3][e] = d * tc * og * (1.0f - og);
                dg[0][e] = dct * gg * ig * (1.0f - ig);
                dg[1][e] = dct * cp[e] * fg * (1.0f - fg);
                dg[2][e] = dct * ig * (1.0f - gg * gg);
                dcn[e] = dct * fg;
            }
            if constexpr (RAG) {
#pragma unroll
                for (int g = 0; g < 4; ++g) dg[g] = dep_sel4(live, dg[g], zero4());
                dc[i] = dep_sel4(live, dcn, dc[i]);
            } else {
                dc[i] = dcn;
            }
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                if constexpr (SPLIT) {
                    unsigned h0, l0, h1, l1;
                    split_pair(dg[g][0], dg[g][1], h0, l0); split_pair(dg[g][2], dg[g][3], h1, l1);
                    const u32x2 hv = {h0, h1}, lv = {l0, l1};
                    char* f = fragw + par * LBL_FRAG_BYTES + g * 1024 + i * 512;
                    *reinterpret_cast<u32x2*>(f) = hv;
                    *reinterpret_cast<u32x2*>(f + LBL_PLANE_BYTES) = lv;
                } else {
                    *reinterpret_cast<f32x4*>(smem + par * BT * LBL_LDG + j * LBL_LDG + g * H + col0 + 16 * i) = dg[g];
                }
                dbs[(i * 4 + g) * LBL_THREADS] += dg[g];
            }
            if (valid) {
                float* go = p.dgi + row * p.lddg + (size_t)dir * 4 * H + col0 + 16 * i;
#pragma unroll
                for (int g = 0; g < 4; ++g) *reinterpret_cast<f32x4*>(go + g * H) = dg[g];
            }
        }
        __builtin_amdgcn_sched_barrier(0);              // (the requests below reuse the slot's registers: not hoisted over its last reads)
        gload(k + LBL_PF, cur);                         // this slot's next tenant
        __builtin_amdgcn_sched_barrier(0);
        if (k + 1 == T && !p.dhx) return;              // (uniform) nobody reads what the last step would carry on
        bar_lds();                                      // the ONE barrier of the step: the gate gradients are in LDS
        f32x4 acc[LBL_NT][4];
#pragma unroll
        for (int i = 0; i < LBL_NT; ++i)
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[i][c] = zero4();
        if constexpr (SPLIT) {
            const u32x4* gf = reinterpret_cast<const u32x4*>(reinterpret_cast<const char*>(smem) + par * LBL_FRAG_BYTES) + lane;
#pragma unroll
            for (int c = 0; c < 4; ++c) {               // a member's four k-steps at a time: 32 registers of fragments
                u32x4 fr[4][2];
#pragma unroll
                for (int g = 0; g < 4; ++g)
#pragma unroll
                    for (int pl = 0; pl < 2; ++pl) fr[g][pl] = gf[(pl * LBL_KS + c * 4 + g) * 64];
#pragma unroll
                for (int g = 0; g < 4; ++g)
#pragma unroll
                    for (int term = 0; term < 3; ++term)      // hi*lo, lo*hi, hi*hi: the order of every split sweep
#pragma unroll
                        for (int i = 0; i < LBL_NT; ++i) {
                            const bf16x8 wv = __builtin_bit_cast(bf16x8, wq[i][c][g][term == 1 ? 1 : 0]);
                            const bf16x8 gv = __builtin_bit_cast(bf16x8, fr[g][term == 0 ? 1 : 0]);
                            acc[i][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wv, gv, acc[i][c], 0, 0, 0);
                        }
            }
        } else {
            const float* drow = smem + par * BT * LBL_LDG + j * LBL_LDG + q * 4;
#pragma unroll
            for (int g = 0; g < 4; ++g) {               // chain (tile, gate): k-chunks 8g .. 8g+7
                f32x4 hv[8];
#pragma unroll
                for (int kk = 0; kk < 8; ++kk) hv[kk] = ld4(drow + (g * 8 + kk) * 16);
#pragma unroll
                for (int kk = 0; kk < 8; ++kk)
#pragma unroll
                    for (int e = 0; e < 4; ++e)
#pragma unroll
                        for (int i = 0; i < LBL_NT; ++i)
                            acc[i][g] = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[i][g * 8 + kk][e], hv[kk][e], acc[i][g], 0, 0, 0);
            }
        }
        if (masked && k + 1 < T) mask_dy(k + 1, nxt);   // (VALU work beside the matrix pipe)
#pragma unroll
        for (int i = 0; i < LBL_NT; ++i) {
            const f32x4 sum = ((acc[i][0] + acc[i][1]) + acc[i][2]) + acc[i][3];
            if constexpr (RAG) dh[i] = dep_sel4(live, sum, dh[i]);      // dead step: the incoming dh passes through
            else dh[i] = sum;
        }
    };
    for (int k0 = 0; k0 < T; k0 += LBL_PF) {
        step(k0, gq[0], gq[1]);
        if (k0 + 1 < T) step(k0 + 1, gq[1], gq[0]);    // (workgroup-uniform)
    }
    // what is carried past the last BPTT step, W_hh^T dG and dc * f, are the gradients of the initial state: the sweep owns the whole
    // W_hh, so there is no host-side recurrent term
    if (valid) {
#pragma unroll
        for (int i = 0; i < LBL_NT; ++i) {
            if (p.dhx) *reinterpret_cast<f32x4*>(p.dhx + so + 16 * i) = dh[i];
            if (p.dcx) *reinterpret_cast<f32x4*>(p.dcx + so + 16 * i) = dc[i];
        }
    }
    // bias partials: the tile's rows in a fixed butterfly order, one row of dbpart per (direction, tile)
    float* const dbo = p.dbpart + ((size_t)dir * p.nwg + p.b0 / BT + bt) * 4 * H + col0;
#pragma unroll
    for (int i = 0; i < LBL_NT; ++i)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            f32x4 s = dbs[(i * 4 + g) * LBL_THREADS];
#pragma unroll
            for (int m = 1; m < 16; m <<= 1)
#pragma unroll
                for (int e = 0; e < 4; ++e) s[e] += __shfl_xor(s[e], m, 64);
            if (j == 0) *reinterpret_cast<f32x4*>(dbo + g * H + 16 * i) = s;
        }
}

// ---- the launchable instances: [split][ragged]
Instance<LL>& local_instance(bool split, bool rag) {
    static Instance<LL> exact[2] = { DEP_INSTANCE((lstm_fwd_local<false, false>), LL_LDS_EXACT), DEP_INSTANCE((lstm_fwd_local<false, true>), LL_LDS_EXACT) };
    static Instance<LL> split3[2] = { DEP_INSTANCE((lstm_fwd_local<true, false>), LL_LDS_SPLIT), DEP_INSTANCE((lstm_fwd_local<true, true>), LL_LDS_SPLIT) };
    return split ? split3[rag] : exact[rag];
}
Instance<LL>& save_instance(bool split, bool rag) {
    static Instance<LL> exact[2] = { DEP_INSTANCE((lstm_fwd_save_local<false, false>), LL_LDS_EXACT), DEP_INSTANCE((lstm_fwd_save_local<false, true>), LL_LDS_EXACT) };
    static Instance<LL> split3[2] = { DEP_INSTANCE((lstm_fwd_save_local<true, false>), LL_LDS_SPLIT), DEP_INSTANCE((lstm_fwd_save_local<true, true>), LL_LDS_SPLIT) };
    return split ? split3[rag] : exact[rag];
}
Instance<LBL>& bwd_instance(bool split, bool rag) {
    static Instance<LBL> exact[2] = { DEP_INSTANCE((lstm_bwd_local<false, false>), LBL_LDS_EXACT), DEP_INSTANCE((lstm_bwd_local<false, true>), LBL_LDS_EXACT) };
    static Instance<LBL> split3[2] = { DEP_INSTANCE((lstm_bwd_local<true, false>), LBL_LDS_SPLIT), DEP_INSTANCE((lstm_bwd_local<true, true>), LBL_LDS_SPLIT) };
    return split ? split3[rag] : exact[rag];
}

}  // namespace

void dep_local_lstm_instance_texts(dep_instance_sink add) {
    for (int m = 0; m < 4; ++m) { add(local_instance(m & 1, m & 2).text); add(save_instance(m & 1, m & 2).text); add(bwd_instance(m & 1, m & 2).text); }
}

bool dep_local_lstm_ok(int cell, int H, int dirs) { return cell == DEP_CELL_LSTM && H == LL_H && (dirs == 1 || dirs == 2); }

int dep_launch_local_lstm_fwd(const dep_sweep_args& a) {
    DEP_CHECK_ARG(dep_local_lstm_ok(a.cell, a.H, a.dirs) && a.B > 0 && a.T > 0);
    DEP_CHECK_ARG(a.gi && a.wp[0] && (a.dirs == 1 || a.wp[1]));
    DEP_CHECK_ARG(dep_cdiv(a.B, BT) + 7 <= INT_MAX / a.dirs);
    // one launch whatever the batch: `dirs` workgroups per tile, no residency bound (launch_chunks pads the tiles to whole groups of 8)
    ChunkGeometry g{a.B, a.dirs, INT_MAX, a.B, 0};
    g.nbtp_max = g.nbtp(0);
    LL p{};
    p.B = a.B; p.T = a.T; p.H = a.H; p.dirs = a.dirs;
    for (int d = 0; d < a.dirs; ++d) p.wp[d] = (const f32x4*)a.wp[d];
    p.gi = a.gi; p.ldgi = a.dirs * 4 * a.H; p.y = a.y; p.ldy = a.ldy;
    p.ydrop = (a.drop_p > 0.f) ? a.ydrop : nullptr;
    p.drop_p = a.drop_p; p.drop_scale = a.drop_p > 0.f ? 1.0f / (1.0f - a.drop_p) : 1.0f; p.seed = a.seed; p.site = a.site;
    p.hx = a.hx; p.cx = a.cx; p.h_n = a.h_n; p.c_n = a.c_n; p.lengths = a.lengths;
    // a DEP_RUN_TRAIN forward (impl 9) saves the gates and c for lstm_bwd_local: the saving instance of the same step body
    const bool save = a.training == DEP_RUN_TRAIN;
    DEP_CHECK_ARG(!save || (a.sv0 && a.sv1));
    if (save) { p.svg = a.sv0; p.svc = a.sv1; }
    DepProfScope prof(DEP_PROF_LSTM_FWD, a.stream);
    return launch_chunks(save ? save_instance(a.split != 0, a.lengths != nullptr) : local_instance(a.split != 0, a.lengths != nullptr), g,
                         dim3(LL_THREADS), p, a.stream, __PRETTY_FUNCTION__, [](int) { return DEP_OK; });
}

int dep_launch_local_lstm_bwd(const dep_sweep_bwd_args& a) {
    DEP_CHECK_ARG(dep_local_lstm_ok(a.cell, a.H, a.dirs) && a.B > 0 && a.T > 0);
    DEP_CHECK_ARG(a.sv0 && a.sv1 && a.dgi && a.dbpart && a.wpT[0] && (a.dirs == 1 || a.wpT[1]));
    DEP_CHECK_ARG(!a.dpooled && !a.dg_pk && !a.sv16 && !a.bf16st);      // fp32 saved gates in, fp32 gate-gradient rows out
    DEP_CHECK_ARG(dep_cdiv(a.B, BT) + 7 <= INT_MAX / a.dirs);
    const int nbt = dep_cdiv(a.B, BT);
    DEP_CHECK_ARG(a.dbpart_rows >= nbt * a.dirs);
    // one launch whatever the batch, as the forward
    ChunkGeometry g{a.B, a.dirs, INT_MAX, a.B, 0};
    g.nbtp_max = g.nbtp(0);
    LBL p{};
    p.B = a.B; p.T = a.T; p.H = a.H; p.dirs = a.dirs;
    for (int d = 0; d < a.dirs; ++d) p.wp[d] = (const f32x4*)a.wpT[d];
    p.dy = a.dy; p.lddy = a.lddy;
    p.drop_p = a.dy ? a.drop_p : 0.f; p.drop_scale = a.drop_p > 0.f ? 1.0f / (1.0f - a.drop_p) : 1.0f;
    p.seed = a.seed; p.site = a.site;
    p.dh_n = a.dh_n; p.dc_n = a.dc_n; p.cx = a.cx; p.dhx = a.dhx; p.dcx = a.dcx;
    p.svg = a.sv0; p.svc = a.sv1;
    p.dgi = a.dgi; p.lddg = a.lddg ? a.lddg : a.dirs * 4 * a.H; p.dbpart = a.dbpart; p.nwg = nbt; p.lengths = a.lengths;
    DepProfScope prof(DEP_PROF_LSTM_BWD, a.stream);
    return launch_chunks(bwd_instance(a.split != 0, a.lengths != nullptr), g, dim3(LBL_THREADS), p, a.stream, __PRETTY_FUNCTION__,
                         [](int) { return DEP_OK; });
}
