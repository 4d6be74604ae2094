// Exchange-free forward sweep of the (Bi)LSTM at H = 128 (impl = 8; nn.LSTM gates i,f,g,o).  ONE workgroup owns a (direction,
// 16-utterance tile) AND the whole recurrent weight of its direction: wave w of eight keeps the W_hh rows of hidden units
// [16w, 16w+16), all four gates and all of K, in 128 VGPRs for the whole sweep, so nothing crosses CUs per step -- no exchange buffer,
// no hello, no flags, no spins, no status word, and no assumption about what else runs on the card.  h_t travels through LDS, double-
// buffered by step parity, behind ONE workgroup barrier per step; c stays in registers.  A lane (j = lane & 15, q = lane >> 4) holds
// units 16w + 4q .. + 3 of utterance j, all four gates (A = W_hh rows, B = h^T, as in lstm_fwd_cluster), so the gate phase needs no
// shuffle and every HBM access of a lane is one 16-byte piece: four loads of the input projection per step, prefetched PF steps
// ahead into registers, and the posted stores of h and dropout(h).  Both biases are folded into the input projection by the caller.
// Forward only: it saves no gates.  Recurrent state in (hx, cx: the prologue) and out (h_n, c_n) costs nothing here.
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
template <bool SPLIT, bool RAG>
__global__ __launch_bounds__(LL_THREADS) void lstm_fwd_local(LL p) {
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
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float ig = fast_sigmoid(acc[0][e] + gi[0][e]);
            const float fg = fast_sigmoid(acc[1][e] + gi[1][e]);
            const float gg = fast_tanh(acc[2][e] + gi[2][e]);
            const float og = fast_sigmoid(acc[3][e] + gi[3][e]);
            cn[e] = fg * c[e] + ig * gg;
            h[e] = og * fast_tanh(cn[e]);
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

// ---- the launchable instances: [split][ragged]
Instance<LL>& local_instance(bool split, bool rag) {
    static Instance<LL> exact[2] = { DEP_INSTANCE((lstm_fwd_local<false, false>), LL_LDS_EXACT), DEP_INSTANCE((lstm_fwd_local<false, true>), LL_LDS_EXACT) };
    static Instance<LL> split3[2] = { DEP_INSTANCE((lstm_fwd_local<true, false>), LL_LDS_SPLIT), DEP_INSTANCE((lstm_fwd_local<true, true>), LL_LDS_SPLIT) };
    return split ? split3[rag] : exact[rag];
}

}  // namespace

void dep_local_lstm_instance_texts(dep_instance_sink add) {
    for (int m = 0; m < 4; ++m) add(local_instance(m & 1, m & 2).text);
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
    DepProfScope prof(DEP_PROF_LSTM_FWD, a.stream);
    return launch_chunks(local_instance(a.split != 0, a.lengths != nullptr), g, dim3(LL_THREADS), p, a.stream, __PRETTY_FUNCTION__,
                         [](int) { return DEP_OK; });
}
