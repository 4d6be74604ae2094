// Persistent recurrent sweeps for nn.GRU / nn.LSTM (forward and BPTT) on gfx950.
//
// One launch walks all T time steps of one layer (both directions of a BiLSTM or a bidirectional GRU
// run side by side in blockIdx.y; the BiGRU on the tile-MFMA kernels only).  A workgroup owns a tile of 16 utterances (the MFMA N dimension) and the whole
// recurrent matrix: per step it computes   G^T (gates x 16) = W_hh (gates x H) * h_{t-1}^T (H x 16)
// with v_mfma_f32_16x16x4_f32 (exact f32, == fmaf chain), W_hh streamed from L2 in a pre-packed
// MFMA-fragment order (one coalesced 1 KiB load per wave per 16x16 k-chunk), h_{t-1} resident in
// LDS, and the gate nonlinearities / state update fused in the epilogue of the same step.
// The time-parallel parts (x_t W_ih^T, dW, dX) are hoisted out to the MFMA GEMM (gemm.hip).
//
// Reference semantics: torch.nn.GRU at Classification/audio_gru_whole.py:59-60,105 and
// torch.nn.LSTM at Classification/text_bilstm_whole.py:54-56,105 (gate order r,z,n / i,f,g,o,
// h0 = c0 = 0 unless a dep_rnn_*_state call brings them, inter-layer dropout on the layer output in training mode).
// The state (FwdP / BwdP hx, cx, c_n, dc_n, dhx, dcx) is a set of run-time pointers read once before the step loop; null pointers
// leave every instance the arithmetic of the stateless call.
#include "dep_common.h"

namespace {

constexpr int BT = 16;       // utterances per workgroup = MFMA N
constexpr int LPAD = 4;      // LDS row padding (floats): keeps rows 16-B aligned, de-phases banks

struct DirP {                 // per-direction pointers
    const f32x4* wp;          // packed recurrent weights (fwd: W_hh ; bwd: W_hh^T)
    const float* w;           // plain (G*H, H) weights (generic kernels)
    const float* b_hh;        // GRU recurrent bias (3H) or nullptr
};

struct FwdP {
    int B, T, H, dirs;
    DirP d[2];
    const float* gi; int ldgi;          // (B,T,ldgi), direction d uses columns [d*G*H, (d+1)*G*H)
    float* y; int ldy;                   // (B,T,ldy),  direction d writes columns [d*H, (d+1)*H)
    float* ydrop; float drop_p, drop_scale; uint64_t seed; uint32_t site;
    float* pooled; float pool_scale;     // (B,dirs*H) GRU only, direction d in columns [d*H, (d+1)*H)
    float* h_n;                          // (dirs,B,H)
    float* sv0; float* sv1; float* sv2; float* sv3;   // GRU: r,z,n,hn (B,T,dirs*H) ; LSTM: gates (B,T,dirs*4H), c (B,T,dirs*H)
    const int* lengths; int pool_mean;   // ragged instances (RAG): row b is live for t < lengths[b]
    const float* hx; const float* cx;    // (dirs,B,H) state before the sweep's first step (LSTM: and c), null = zeros; read once, before the step loop
    float* c_n;                          // LSTM (dirs,B,H) c after the last step, or null
};

struct BwdP {
    int B, T, H, dirs;
    DirP d[2];
    const float* y; int ldy;
    const float* dy; int lddy;
    float drop_p, drop_scale; uint64_t seed; uint32_t site;
    const float* dpooled; float pool_scale;   // (B,dirs*H) GRU only
    const float* dh_n;                         // (dirs,B,H)
    const float* sv0; const float* sv1; const float* sv2; const float* sv3;
    float* dgi; int lddg;                // (B,T,lddg) lddg = dirs*G*H
    float* dghn;                         // GRU (B,T,dirs*H)
    float* dbpart;                       // [dirs][nwg][G'][H]  G' = 4
    int nwg;
    const int* lengths; int pool_mean;   // ragged instances (RAG)
    const float* hx; const float* cx;    // (dirs,B,H) what the forward started from (h_prev / c_prev of sweep step 0), null = zeros
    const float* dc_n;                   // LSTM (dirs,B,H), enters where dh_n enters, or null
    float* dhx; float* dcx;              // (dirs,B,H) the recurrent dh / dc left after the last step of the walk, written, or null
};

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }
__device__ __forceinline__ f32x4 zero4() { f32x4 z = {0.f, 0.f, 0.f, 0.f}; return z; }

// acc[t] += Wtile[t] (16 x K) * v^T (K x 16).  wp: this wave's first packed tile + lane, tile t
// chunk kc at wp[(t*KC + kc)*64].  vs: LDS row (lane&15) + (lane>>4)*4 of the 16 x K operand.
template <int NTL>
__device__ __forceinline__ void matvec_tiles(f32x4 (&acc)[NTL], const f32x4* __restrict__ wp, int KC,
                                             const float* vs) {
    f32x4 wc[NTL], wn[NTL];
#pragma unroll
    for (int t = 0; t < NTL; ++t) wc[t] = wp[(size_t)(t * KC) * 64];
#pragma unroll 2
    for (int kc = 0; kc < KC; ++kc) {
        if (kc + 1 < KC) {
#pragma unroll
            for (int t = 0; t < NTL; ++t) wn[t] = wp[(size_t)(t * KC + kc + 1) * 64];
        }
        const f32x4 hv = ld4(vs + kc * 16);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int t = 0; t < NTL; ++t)
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(wc[t][e], hv[e], acc[t], 0, 0, 0);
#pragma unroll
        for (int t = 0; t < NTL; ++t) wc[t] = wn[t];
    }
}

__device__ __forceinline__ f32x4 sig4(f32x4 x) {
    f32x4 r; r[0] = dep_sigmoid(x[0]); r[1] = dep_sigmoid(x[1]); r[2] = dep_sigmoid(x[2]); r[3] = dep_sigmoid(x[3]); return r;
}
__device__ __forceinline__ f32x4 tanh4(f32x4 x) {
    f32x4 r; r[0] = tanhf(x[0]); r[1] = tanhf(x[1]); r[2] = tanhf(x[2]); r[3] = tanhf(x[3]); return r;
}

// sum over the 16 lanes that share (lane>>4): lanes differ in batch row j = lane&15
__device__ __forceinline__ f32x4 rowsum16(f32x4 v) {
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] += __shfl_xor(v[e], m, 64);
    }
    return v;
}

// RAG (every kernel of this file): the ragged-batch instances (dep_rnn_forward_varlen).  One per-row predicate, live = t < lengths[b]:
//   forward : state (h, c) = live ? new : previous ; y[b,t] = live ? h_t : 0 ; the pool takes live steps only ; saved c = live ? c_t : 0
//   backward: gate gradients of (b,t) = live ? computed : 0 ; dh (dc) carried to the previous step = live ? computed : incoming
// Selects, never value * 0: the saved gates / dy of dead positions may be anything.  Every workgroup still runs all T steps.
// With a state (dep_rnn_*_state_varlen) the same selects carry hx / cx through dead steps: a reverse sweep, which meets them first, reaches
// t = len - 1 with its state, and an empty row hands h, c (backward: dh, dc) through bit for bit.  The backward takes h_prev / c_prev of
// that first live step from the state, as at sweep step 0, not from the dead position behind it.
// RAG = false is the dense text: the predicate is compiled out.
// =============================================================================== GRU forward
// BI: the bidirectional instances (grid.y = 2, dir = blockIdx.y): direction 1 sweeps t = T-1 .. 0 on p.d[1], and every array is the
// direction-interleaved one -- gi (B,T,2*3H), y / dropout(y) / saved gates (B,T,2H), pool (B,2H), h_n (2,B,H).  A ragged row's reverse
// sweep meets its dead steps first: the state stays 0 through them (the same live select).  BI = false is the unidirectional text.
template <int JPW, bool RAG = false, bool BI = false>
__global__ __launch_bounds__(512) void gru_fwd_mfma(FwdP p) {
    // contraction by syntax: see DEP_FP_CONTRACT_NOTE in dep_common.h (why, and how to re-verify the dense instances after a compiler change)
#pragma clang fp contract(on)
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int H = p.H, T = p.T, LDH = H + LPAD, KC = H / 16;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int j = lane & 15, q = lane >> 4;
    const int dir = BI ? (int)blockIdx.y : 0;
    const int SW = BI ? 2 * H : H;            // row width of the saved gates and the pool
    const int b = blockIdx.x * BT + j;
    const bool valid = b < p.B;
    int len = T;
    if constexpr (RAG) len = valid ? dep_row_len(p.lengths, b, T) : 0;
    float* hs0 = smem; float* hs1 = smem + BT * LDH;
    for (int i = threadIdx.x; i < 2 * BT * LDH; i += blockDim.x) smem[i] = 0.f;

    const f32x4* wp = p.d[dir].wp + (size_t)(w * JPW * 3) * KC * 64 + lane;
    f32x4 bh[JPW][3], hprev[JPW], pool[JPW];
#pragma unroll
    for (int jj = 0; jj < JPW; ++jj) {
        const int col0 = (w * JPW + jj) * 16 + q * 4;
#pragma unroll
        for (int g = 0; g < 3; ++g) bh[jj][g] = ld4(p.d[dir].b_hh + g * H + col0);
        // the direction's own slice of hx; rows past B of the last tile read nothing (hx has exactly B rows)
        hprev[jj] = (p.hx && valid) ? ld4(p.hx + ((size_t)dir * p.B + b) * H + col0) : zero4();
        pool[jj] = zero4();
    }
    if (p.hx) {
        // the first LDS plane is h before step 0.  The zero fill above wrote the same words from other threads: barrier first.
        // (p.hx is uniform over the launch.  Every (row, column) of hs0 the matvec reads is stored here, rows past B as zeros.)
        __syncthreads();
#pragma unroll
        for (int jj = 0; jj < JPW; ++jj) st4(hs0 + j * LDH + (w * JPW + jj) * 16 + q * 4, hprev[jj]);
    }
    __syncthreads();

    for (int s = 0; s < T; ++s) {
        const int t = (BI && dir) ? T - 1 - s : s;
        const float* hcur = (s & 1) ? hs1 : hs0;
        float* hnext = (s & 1) ? hs0 : hs1;
        const size_t row = (size_t)b * T + t;
        f32x4 gi[JPW][3];
#pragma unroll
        for (int jj = 0; jj < JPW; ++jj) {
            const int col0 = (w * JPW + jj) * 16 + q * 4;
#pragma unroll
            for (int g = 0; g < 3; ++g)
                gi[jj][g] = valid ? ld4(p.gi + row * p.ldgi + dir * 3 * H + g * H + col0) : zero4();
        }
        f32x4 acc[JPW * 3];
#pragma unroll
        for (int i = 0; i < JPW * 3; ++i) acc[i] = zero4();
        matvec_tiles<JPW * 3>(acc, wp, KC, hcur + j * LDH + q * 4);
#pragma unroll
        for (int jj = 0; jj < JPW; ++jj) {
            const int col0 = (w * JPW + jj) * 16 + q * 4;
            const f32x4 r = sig4(gi[jj][0] + acc[jj * 3 + 0] + bh[jj][0]);
            const f32x4 z = sig4(gi[jj][1] + acc[jj * 3 + 1] + bh[jj][1]);
            const f32x4 hn = acc[jj * 3 + 2] + bh[jj][2];
            const f32x4 n = tanh4(gi[jj][2] + r * hn);
            f32x4 h = z * hprev[jj] + (1.0f - z) * n;         // (the fused product is z * h_{t-1}: contraction by syntax, see above)
            if constexpr (RAG) {
                const bool live = t < len;
                hprev[jj] = dep_sel4(live, h, hprev[jj]);      // the state freezes behind the row's last step
                h = dep_sel4(live, h, zero4());                // what y, dropout(y) and the pool see
            } else {
                hprev[jj] = h;
            }
            pool[jj] += h;
            st4(hnext + j * LDH + col0, hprev[jj]);
            if (valid) {
                const size_t o = row * p.ldy + dir * H + col0;
                st4(p.y + o, h);
                if (p.ydrop) st4(p.ydrop + o, h * dep_dropmask4(p.seed, p.site, o >> 2, p.drop_p, p.drop_scale));
                if (p.sv0) {
                    const size_t so = row * SW + dir * H + col0;
                    st4(p.sv0 + so, r); st4(p.sv1 + so, z); st4(p.sv2 + so, n); st4(p.sv3 + so, hn);
                }
            }
        }
        __syncthreads();
    }
    if (valid) {
#pragma unroll
        for (int jj = 0; jj < JPW; ++jj) {
            const int col0 = (w * JPW + jj) * 16 + q * 4;
            const float ps = RAG ? dep_ragged_pool_scale(p.pool_mean, len, T, p.pool_scale) : p.pool_scale;
            if (p.pooled) st4(p.pooled + (size_t)b * SW + dir * H + col0, pool[jj] * ps);
            if (p.h_n) st4(p.h_n + ((size_t)dir * p.B + b) * H + col0, hprev[jj]);
        }
    }
}

// =============================================================================== GRU backward
// BI: as in gru_fwd_mfma.  Direction 1 walks its sweep backwards, t = 0 .. T-1, with h_prev = y[t+1] (none at t = T-1; behind a ragged
// row's end y is 0); dgi (B,T,2*3H), dghn (B,T,2H), dh_n (2,B,H), dpooled (B,2H), bias partials at row dir*nwg + blockIdx.x.
template <int JPW, bool RAG = false, bool BI = false>
__global__ __launch_bounds__(512) void gru_bwd_mfma(BwdP p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int H = p.H, T = p.T, G3 = 3 * H, LDG = G3 + LPAD, KC = G3 / 16;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int j = lane & 15, q = lane >> 4;
    const int dir = BI ? (int)blockIdx.y : 0;
    const int SW = BI ? 2 * H : H;            // row width of the saved gates, dghn and dpooled
    const int b = blockIdx.x * BT + j;
    const bool valid = b < p.B;
    int len = T;
    if constexpr (RAG) len = valid ? dep_row_len(p.lengths, b, T) : 0;
    const float dps = RAG ? dep_ragged_pool_scale(p.pool_mean, len, T, p.pool_scale) : p.pool_scale;
    float* ds0 = smem; float* ds1 = smem + BT * LDG;

    const f32x4* wp = p.d[dir].wp + (size_t)(w * JPW) * KC * 64 + lane;
    f32x4 dhrec[JPW], dbr[JPW], dbz[JPW], dbn[JPW], dbh[JPW], dpl[JPW], hx0[JPW];
#pragma unroll
    for (int jj = 0; jj < JPW; ++jj) {
        const int col0 = (w * JPW + jj) * 16 + q * 4;
        dhrec[jj] = (p.dh_n && valid) ? ld4(p.dh_n + ((size_t)dir * p.B + b) * H + col0) : zero4();
        hx0[jj] = (p.hx && valid) ? ld4(p.hx + ((size_t)dir * p.B + b) * H + col0) : zero4();      // h_prev of sweep step 0 (t = 0, reverse: t = T-1)
        dpl[jj] = (p.dpooled && valid) ? ld4(p.dpooled + (size_t)b * SW + dir * H + col0) * dps : zero4();
        dbr[jj] = zero4(); dbz[jj] = zero4(); dbn[jj] = zero4(); dbh[jj] = zero4();
    }

    for (int s = T - 1; s >= 0; --s) {
        const int t = (BI && dir) ? T - 1 - s : s;
        float* dcur = (s & 1) ? ds1 : ds0;
        const size_t row = (size_t)b * T + t;
        f32x4 dzt[JPW];
#pragma unroll
        for (int jj = 0; jj < JPW; ++jj) {
            const int col0 = (w * JPW + jj) * 16 + q * 4;
            f32x4 r = zero4(), z = zero4(), n = zero4(), hn = zero4(), hp = zero4(), d = dhrec[jj] + dpl[jj];
            if (valid) {
                const size_t so = row * SW + dir * H + col0;
                r = ld4(p.sv0 + so); z = ld4(p.sv1 + so); n = ld4(p.sv2 + so); hn = ld4(p.sv3 + so);
                hp = s > 0 ? ld4(p.y + ((BI && dir) ? row + 1 : row - 1) * p.ldy + dir * H + col0) : hx0[jj];
                // a ragged row's reverse sweep starts at t = len - 1: its h_prev is the state, not the dead position behind it (which holds 0)
                // Read again from memory, on a branch only that step takes (most waves skip it in most steps): as a per-value select of
                // hx0 it cost the ragged bidirectional backward 0.7 % at H = 256
                if constexpr (RAG && BI) {
                    if (dir && s > 0 && t == len - 1) hp = p.hx ? ld4(p.hx + ((size_t)dir * p.B + b) * H + col0) : zero4();
                }
                if (p.dy) {
                    const size_t o = row * p.lddy + dir * H + col0;
                    f32x4 dyv = ld4(p.dy + o);
                    if (p.drop_p > 0.f) dyv *= dep_dropmask4(p.seed, p.site, o >> 2, p.drop_p, p.drop_scale);
                    d += dyv;
                }
            }
            f32x4 dn = d * (1.0f - z) * (1.0f - n * n);
            f32x4 dz = d * (hp - n) * z * (1.0f - z);
            f32x4 dr = dn * hn * r * (1.0f - r);
            f32x4 dnr = dn * r;
            dzt[jj] = d * z;
            if constexpr (RAG) {
                const bool live = t < len;
                dn = dep_sel4(live, dn, zero4()); dz = dep_sel4(live, dz, zero4());
                dr = dep_sel4(live, dr, zero4()); dnr = dep_sel4(live, dnr, zero4());
            }
            st4(dcur + j * LDG + col0, dr);
            st4(dcur + j * LDG + H + col0, dz);
            st4(dcur + j * LDG + 2 * H + col0, dnr);
            if (valid) {
                float* g = p.dgi + row * p.lddg + dir * 3 * H;
                st4(g + col0, dr); st4(g + H + col0, dz); st4(g + 2 * H + col0, dn);
                st4(p.dghn + row * SW + dir * H + col0, dnr);
            }
            dbr[jj] += dr; dbz[jj] += dz; dbn[jj] += dn; dbh[jj] += dnr;
        }
        __syncthreads();
        f32x4 acc[JPW];
#pragma unroll
        for (int i = 0; i < JPW; ++i) acc[i] = zero4();
        matvec_tiles<JPW>(acc, wp, KC, dcur + j * LDG + q * 4);
#pragma unroll
        for (int jj = 0; jj < JPW; ++jj) {
            if constexpr (RAG) dhrec[jj] = dep_sel4(t < len, dzt[jj] + acc[jj], dhrec[jj]);      // dead step: the incoming dh passes through
            else dhrec[jj] = dzt[jj] + acc[jj];
        }
    }
    // what is carried past sweep step 0, d * z + W_hh^T dG, is the gradient of the initial state
    if (p.dhx && valid) {
#pragma unroll
        for (int jj = 0; jj < JPW; ++jj) st4(p.dhx + ((size_t)dir * p.B + b) * H + (w * JPW + jj) * 16 + q * 4, dhrec[jj]);
    }
    // bias-gradient partials of this workgroup: dbpart[wg][4][H]  (r, z, n_input, n_hidden)
#pragma unroll
    for (int jj = 0; jj < JPW; ++jj) {
        const int col0 = (w * JPW + jj) * 16 + q * 4;
        const f32x4 s0 = rowsum16(dbr[jj]), s1 = rowsum16(dbz[jj]), s2 = rowsum16(dbn[jj]), s3 = rowsum16(dbh[jj]);
        if (j == 0) {
            float* o = p.dbpart + ((size_t)dir * p.nwg + blockIdx.x) * 4 * H;
            st4(o + col0, s0); st4(o + H + col0, s1); st4(o + 2 * H + col0, s2); st4(o + 3 * H + col0, s3);
        }
    }
}

// =============================================================================== LSTM forward
template <int JPW, bool RAG = false>
__global__ __launch_bounds__(512) void lstm_fwd_mfma(FwdP p) {
    // contraction by syntax: see DEP_FP_CONTRACT_NOTE in dep_common.h (why, and how to re-verify the dense instances after a compiler change)
#pragma clang fp contract(on)
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int H = p.H, T = p.T, LDH = H + LPAD, KC = H / 16;
    const int dir = blockIdx.y;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int j = lane & 15, q = lane >> 4;
    const int b = blockIdx.x * BT + j;
    const bool valid = b < p.B;
    int len = T;
    if constexpr (RAG) len = valid ? dep_row_len(p.lengths, b, T) : 0;
    float* hs0 = smem; float* hs1 = smem + BT * LDH;
    for (int i = threadIdx.x; i < 2 * BT * LDH; i += blockDim.x) smem[i] = 0.f;
    const f32x4* wp = p.d[dir].wp + (size_t)(w * JPW * 4) * KC * 64 + lane;
    const int ldsg = p.dirs * 4 * H, ldsc = p.dirs * H;
    f32x4 c[JPW], hlast[JPW];
#pragma unroll
    for (int jj = 0; jj < JPW; ++jj) {
        // the direction's own slices of hx / cx; rows past B of the last tile read nothing (the state has exactly B rows)
        const size_t so = ((size_t)dir * p.B + b) * H + (w * JPW + jj) * 16 + q * 4;
        c[jj] = (p.cx && valid) ? ld4(p.cx + so) : zero4();
        hlast[jj] = (p.hx && valid) ? ld4(p.hx + so) : zero4();
    }
    if (p.hx) {
        // the first LDS plane is h before step 0; the zero fill above wrote the same words from other threads: barrier first (as in gru_fwd_mfma)
        __syncthreads();
#pragma unroll
        for (int jj = 0; jj < JPW; ++jj) st4(hs0 + j * LDH + (w * JPW + jj) * 16 + q * 4, hlast[jj]);
    }
    __syncthreads();

    for (int s = 0; s < T; ++s) {
        const int t = dir ? (T - 1 - s) : s;
        const float* hcur = (s & 1) ? hs1 : hs0;
        float* hnext = (s & 1) ? hs0 : hs1;
        const size_t row = (size_t)b * T + t;
        f32x4 gi[JPW][4];
#pragma unroll
        for (int jj = 0; jj < JPW; ++jj) {
            const int col0 = (w * JPW + jj) * 16 + q * 4;
#pragma unroll
            for (int g = 0; g < 4; ++g)
                gi[jj][g] = valid ? ld4(p.gi + row * p.ldgi + dir * 4 * H + g * H + col0) : zero4();
        }
        f32x4 acc[JPW * 4];
#pragma unroll
        for (int i = 0; i < JPW * 4; ++i) acc[i] = zero4();
        matvec_tiles<JPW * 4>(acc, wp, KC, hcur + j * LDH + q * 4);
#pragma unroll
        for (int jj = 0; jj < JPW; ++jj) {
            const int col0 = (w * JPW + jj) * 16 + q * 4;
            const f32x4 ig = sig4(gi[jj][0] + acc[jj * 4 + 0]);
            const f32x4 fg = sig4(gi[jj][1] + acc[jj * 4 + 1]);
            const f32x4 gg = tanh4(gi[jj][2] + acc[jj * 4 + 2]);
            const f32x4 og = sig4(gi[jj][3] + acc[jj * 4 + 3]);
            f32x4 cn = fg * c[jj] + ig * gg;
            f32x4 h = og * tanh4(cn);
            if constexpr (RAG) {
                const bool live = t < len;
                c[jj] = dep_sel4(live, cn, c[jj]); hlast[jj] = dep_sel4(live, h, hlast[jj]);
                h = dep_sel4(live, h, zero4()); cn = dep_sel4(live, cn, zero4());      // y and the saved c are 0 at dead positions (the backward reads c_{t-1} there)
            } else {
                c[jj] = cn; hlast[jj] = h;
            }
            st4(hnext + j * LDH + col0, hlast[jj]);
            if (valid) {
                const size_t o = row * p.ldy + dir * H + col0;
                st4(p.y + o, h);
                if (p.ydrop) st4(p.ydrop + o, h * dep_dropmask4(p.seed, p.site, o >> 2, p.drop_p, p.drop_scale));
                if (p.sv0) {
                    float* gs = p.sv0 + row * ldsg + dir * 4 * H + col0;
                    st4(gs, ig); st4(gs + H, fg); st4(gs + 2 * H, gg); st4(gs + 3 * H, og);
                    st4(p.sv1 + row * ldsc + dir * H + col0, cn);
                }
            }
        }
        __syncthreads();
    }
    if (valid) {
#pragma unroll
        for (int jj = 0; jj < JPW; ++jj) {
            const size_t so = ((size_t)dir * p.B + b) * H + (w * JPW + jj) * 16 + q * 4;
            if (p.h_n) st4(p.h_n + so, hlast[jj]);
            if (p.c_n) st4(p.c_n + so, c[jj]);
        }
    }
}

// =============================================================================== LSTM backward
template <int JPW, bool RAG = false>
__global__ __launch_bounds__(512) void lstm_bwd_mfma(BwdP p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int H = p.H, T = p.T, G4 = 4 * H, LDG = G4 + LPAD, KC = G4 / 16;
    const int dir = blockIdx.y;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int j = lane & 15, q = lane >> 4;
    const int b = blockIdx.x * BT + j;
    const bool valid = b < p.B;
    int len = T;
    if constexpr (RAG) len = valid ? dep_row_len(p.lengths, b, T) : 0;
    float* ds0 = smem; float* ds1 = smem + BT * LDG;
    const f32x4* wp = p.d[dir].wp + (size_t)(w * JPW) * KC * 64 + lane;
    const int ldsg = p.dirs * 4 * H, ldsc = p.dirs * H;
    f32x4 dhrec[JPW], dcrec[JPW], db[JPW][4];
#pragma unroll
    for (int jj = 0; jj < JPW; ++jj) {
        const int col0 = (w * JPW + jj) * 16 + q * 4;
        dhrec[jj] = (p.dh_n && valid) ? ld4(p.dh_n + ((size_t)dir * p.B + b) * H + col0) : zero4();
        dcrec[jj] = (p.dc_n && valid) ? ld4(p.dc_n + ((size_t)dir * p.B + b) * H + col0) : zero4();
#pragma unroll
        for (int g = 0; g < 4; ++g) db[jj][g] = zero4();
    }
    for (int s = T - 1; s >= 0; --s) {
        const int t = dir ? (T - 1 - s) : s;
        float* dcur = (s & 1) ? ds1 : ds0;
        const size_t row = (size_t)b * T + t;
#pragma unroll
        for (int jj = 0; jj < JPW; ++jj) {
            const int col0 = (w * JPW + jj) * 16 + q * 4;
            f32x4 ig = zero4(), fg = zero4(), gg = zero4(), og = zero4(), ct = zero4(), cp = zero4(), d = dhrec[jj];
            if (valid) {
                const float* gs = p.sv0 + row * ldsg + dir * 4 * H + col0;
                ig = ld4(gs); fg = ld4(gs + H); gg = ld4(gs + 2 * H); og = ld4(gs + 3 * H);
                ct = ld4(p.sv1 + row * ldsc + dir * H + col0);
                // (RAG: a ragged row's reverse sweep starts at t = len - 1; c_prev of that step is the state too, not the dead position behind it)
                if (s > 0 && !(RAG && dir && t == len - 1)) {
                    const size_t rowp = dir ? row + 1 : row - 1;
                    cp = ld4(p.sv1 + rowp * ldsc + dir * H + col0);
                } else if (p.cx) {
                    // c_prev of sweep step 0 (t = 0, reverse: t = T-1) is the forward's cx: read once, here, on a branch that is uniform
                    // over the launch and not taken in any other step (held in registers across the loop it cost the H = 256 sweep 1.6 %)
                    cp = ld4(p.cx + ((size_t)dir * p.B + b) * H + col0);
                }
                if (p.dy) {
                    const size_t o = row * p.lddy + dir * H + col0;
                    f32x4 dyv = ld4(p.dy + o);
                    if (p.drop_p > 0.f) dyv *= dep_dropmask4(p.seed, p.site, o >> 2, p.drop_p, p.drop_scale);
                    d += dyv;
                }
            }
            const f32x4 tc = tanh4(ct);
            const f32x4 dog = d * tc * og * (1.0f - og);
            const f32x4 dct = d * og * (1.0f - tc * tc) + dcrec[jj];
            f32x4 dig = dct * gg * ig * (1.0f - ig);
            f32x4 dfg = dct * cp * fg * (1.0f - fg);
            f32x4 dgg = dct * ig * (1.0f - gg * gg);
            f32x4 dogl = dog;
            if constexpr (RAG) {
                const bool live = t < len;
                dig = dep_sel4(live, dig, zero4()); dfg = dep_sel4(live, dfg, zero4());
                dgg = dep_sel4(live, dgg, zero4()); dogl = dep_sel4(live, dog, zero4());
                dcrec[jj] = dep_sel4(live, dct * fg, dcrec[jj]);
            } else {
                dcrec[jj] = dct * fg;
            }
            float* dl = dcur + j * LDG + col0;
            st4(dl, dig); st4(dl + H, dfg); st4(dl + 2 * H, dgg); st4(dl + 3 * H, dogl);
            if (valid) {
                float* g = p.dgi + row * p.lddg + dir * 4 * H + col0;
                st4(g, dig); st4(g + H, dfg); st4(g + 2 * H, dgg); st4(g + 3 * H, dogl);
            }
            db[jj][0] += dig; db[jj][1] += dfg; db[jj][2] += dgg; db[jj][3] += dogl;
        }
        __syncthreads();
        f32x4 acc[JPW];
#pragma unroll
        for (int i = 0; i < JPW; ++i) acc[i] = zero4();
        matvec_tiles<JPW>(acc, wp, KC, dcur + j * LDG + q * 4);
#pragma unroll
        for (int jj = 0; jj < JPW; ++jj) {
            if constexpr (RAG) dhrec[jj] = dep_sel4(t < len, acc[jj], dhrec[jj]);      // dead step: the incoming dh passes through
            else dhrec[jj] = acc[jj];
        }
    }
    // what is carried past sweep step 0, W_hh^T dG and dc_t * f, are the gradients of the initial state
    if (valid) {
#pragma unroll
        for (int jj = 0; jj < JPW; ++jj) {
            const size_t so = ((size_t)dir * p.B + b) * H + (w * JPW + jj) * 16 + q * 4;
            if (p.dhx) st4(p.dhx + so, dhrec[jj]);
            if (p.dcx) st4(p.dcx + so, dcrec[jj]);
        }
    }
#pragma unroll
    for (int jj = 0; jj < JPW; ++jj) {
        const int col0 = (w * JPW + jj) * 16 + q * 4;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f32x4 s = rowsum16(db[jj][g]);
            if (j == 0) st4(p.dbpart + ((size_t)dir * p.nwg + blockIdx.x) * 4 * H + g * H + col0, s);
        }
    }
}

// =============================================================================== generic kernels
// Any H (no alignment requirement): one workgroup per utterance, threads over hidden units,
// plain fmaf dot products against the row-major weights.  Used for shapes the MFMA tiling does
// not cover (H % 16 != 0) and as an in-library cross-check (desc.impl = 1).
constexpr int GEN_T = 128;

template <bool RAG = false>
__global__ __launch_bounds__(GEN_T) void gru_fwd_generic(FwdP p) {
    // contraction by syntax: see DEP_FP_CONTRACT_NOTE in dep_common.h (why, and how to re-verify the dense instances after a compiler change)
#pragma clang fp contract(on)
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int H = p.H, T = p.T, b = blockIdx.x;
    const int len = RAG ? dep_row_len(p.lengths, b, T) : T;
    float* hs = smem;            // [H] h_{t-1}
    float* hnew = smem + H;      // [H]
    const float* W = p.d[0].w; const float* bh = p.d[0].b_hh;
    for (int i = threadIdx.x; i < H; i += GEN_T) hs[i] = p.hx ? p.hx[(size_t)b * H + i] : 0.f;      // h before step 0
    __syncthreads();
    for (int t = 0; t < T; ++t) {
        const size_t row = (size_t)b * T + t;
        for (int i = threadIdx.x; i < H; i += GEN_T) {
            float ar = 0.f, az = 0.f, an = 0.f;
            for (int k = 0; k < H; ++k) {
                const float hv = hs[k];
                ar = fmaf(W[(size_t)i * H + k], hv, ar);
                az = fmaf(W[(size_t)(H + i) * H + k], hv, az);
                an = fmaf(W[(size_t)(2 * H + i) * H + k], hv, an);
            }
            const float* g = p.gi + row * p.ldgi;
            const float r = dep_sigmoid(g[i] + ar + bh[i]);
            const float z = dep_sigmoid(g[H + i] + az + bh[H + i]);
            const float hn = an + bh[2 * H + i];
            const float n = tanhf(g[2 * H + i] + r * hn);
            float h = (1.0f - z) * n + z * hs[i];
            const bool live = !RAG || t < len;
            hnew[i] = live ? h : hs[i];
            h = live ? h : 0.f;
            const size_t o = row * p.ldy + i;
            p.y[o] = h;
            if (p.ydrop) p.ydrop[o] = h * dep_dropmask1(p.seed, p.site, o, p.drop_p, p.drop_scale);
            if (p.sv0) { const size_t so = row * H + i; p.sv0[so] = r; p.sv1[so] = z; p.sv2[so] = n; p.sv3[so] = hn; }
        }
        __syncthreads();
        for (int i = threadIdx.x; i < H; i += GEN_T) hs[i] = hnew[i];
        __syncthreads();
    }
    if (p.h_n) for (int i = threadIdx.x; i < H; i += GEN_T) p.h_n[(size_t)b * H + i] = hs[i];
    if (p.pooled) {
        for (int i = threadIdx.x; i < H; i += GEN_T) {
            float s = 0.f;
            for (int t = 0; t < T; ++t) s += p.y[((size_t)b * T + t) * p.ldy + i];
            p.pooled[(size_t)b * H + i] = s * (RAG ? dep_ragged_pool_scale(p.pool_mean, len, T, p.pool_scale) : p.pool_scale);
        }
    }
}

template <bool RAG = false>
__global__ __launch_bounds__(GEN_T) void gru_bwd_generic(BwdP p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int H = p.H, T = p.T, b = blockIdx.x, G3 = 3 * H;
    const int len = RAG ? dep_row_len(p.lengths, b, T) : T;
    const float dps = RAG ? dep_ragged_pool_scale(p.pool_mean, len, T, p.pool_scale) : p.pool_scale;
    float* dg = smem;            // [3H] dgh of this step
    float* dh = smem + G3;       // [H] recurrent dh
    float* hx0 = smem + G3 + 2 * H;      // [H] h_prev of step 0 (the forward's hx, or zeros); element i is thread i's own
    float* dbp = p.dbpart + (size_t)b * 4 * H;
    const float* W = p.d[0].w;
    for (int i = threadIdx.x; i < H; i += GEN_T) {
        dh[i] = p.dh_n ? p.dh_n[(size_t)b * H + i] : 0.f;
        hx0[i] = p.hx ? p.hx[(size_t)b * H + i] : 0.f;
    }
    for (int i = threadIdx.x; i < 4 * H; i += GEN_T) dbp[i] = 0.f;
    __syncthreads();
    for (int t = T - 1; t >= 0; --t) {
        const size_t row = (size_t)b * T + t;
        for (int i = threadIdx.x; i < H; i += GEN_T) {
            const size_t so = row * H + i;
            const float r = p.sv0[so], z = p.sv1[so], n = p.sv2[so], hn = p.sv3[so];
            const float hp = t > 0 ? p.y[(row - 1) * p.ldy + i] : hx0[i];
            float d = dh[i];
            if (p.dpooled) d += p.dpooled[(size_t)b * H + i] * dps;
            if (p.dy) {
                const size_t o = row * p.lddy + i;
                float dyv = p.dy[o];
                if (p.drop_p > 0.f) dyv *= dep_dropmask1(p.seed, p.site, o, p.drop_p, p.drop_scale);
                d += dyv;
            }
            if constexpr (RAG) {
                if (t >= len) {           // dead step (uniform over the workgroup): no gate gradient, the incoming dh stays
                    dg[i] = 0.f; dg[H + i] = 0.f; dg[2 * H + i] = 0.f;
                    float* g0 = p.dgi + row * p.lddg;
                    g0[i] = 0.f; g0[H + i] = 0.f; g0[2 * H + i] = 0.f;
                    p.dghn[row * H + i] = 0.f;
                    continue;
                }
            }
            const float dn = d * (1.0f - z) * (1.0f - n * n);
            const float dz = d * (hp - n) * z * (1.0f - z);
            const float dr = dn * hn * r * (1.0f - r);
            const float dnr = dn * r;
            dg[i] = dr; dg[H + i] = dz; dg[2 * H + i] = dnr;
            float* g = p.dgi + row * p.lddg;
            g[i] = dr; g[H + i] = dz; g[2 * H + i] = dn;
            p.dghn[row * H + i] = dnr;
            dbp[i] += dr; dbp[H + i] += dz; dbp[2 * H + i] += dn; dbp[3 * H + i] += dnr;
            dh[i] = d * z;           // own element only; the matvec term is added after the barrier
        }
        __syncthreads();
        for (int i = threadIdx.x; i < H; i += GEN_T) {
            float s = 0.f;
            for (int k = 0; k < G3; ++k) s = fmaf(dg[k], W[(size_t)k * H + i], s);
            if (!RAG || t < len) dh[i] += s;      // (dead step: the incoming dh passes through bit for bit, -0.0 included)
        }
        __syncthreads();
    }
    // dh past step 0, d * z + W_hh^T dG, is the gradient of the initial state (element i was last written by this thread)
    if (p.dhx) for (int i = threadIdx.x; i < H; i += GEN_T) p.dhx[(size_t)b * H + i] = dh[i];
}

template <bool RAG = false>
__global__ __launch_bounds__(GEN_T) void lstm_fwd_generic(FwdP p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int H = p.H, T = p.T, b = blockIdx.x, dir = blockIdx.y;
    const int len = RAG ? dep_row_len(p.lengths, b, T) : T;
    float* hs = smem; float* hnew = smem + H; float* cs = smem + 2 * H;
    const float* W = p.d[dir].w;
    const int ldsg = p.dirs * 4 * H, ldsc = p.dirs * H;
    for (int i = threadIdx.x; i < H; i += GEN_T) {      // h, c before the sweep's first step: the direction's own slice
        const size_t so = ((size_t)dir * p.B + b) * H + i;
        hs[i] = p.hx ? p.hx[so] : 0.f; cs[i] = p.cx ? p.cx[so] : 0.f;
    }
    __syncthreads();
    for (int s = 0; s < T; ++s) {
        const int t = dir ? (T - 1 - s) : s;
        const size_t row = (size_t)b * T + t;
        for (int i = threadIdx.x; i < H; i += GEN_T) {
            float a[4] = {0.f, 0.f, 0.f, 0.f};
            for (int k = 0; k < H; ++k) {
                const float hv = hs[k];
#pragma unroll
                for (int g = 0; g < 4; ++g) a[g] = fmaf(W[(size_t)(g * H + i) * H + k], hv, a[g]);
            }
            const float* gi = p.gi + row * p.ldgi + dir * 4 * H;
            const float ig = dep_sigmoid(gi[i] + a[0]), fg = dep_sigmoid(gi[H + i] + a[1]);
            const float gg = tanhf(gi[2 * H + i] + a[2]), og = dep_sigmoid(gi[3 * H + i] + a[3]);
            // (no contract(on) here, unlike gru_fwd_generic: the dead step is a workgroup-uniform branch, so the live path below IS the
            // dense instance's statement sequence and rounds like it; gru_fwd_generic selects per value and needs the pragma)
            if constexpr (RAG) {
                if (t >= len) {           // dead step (uniform over the workgroup): the state stays, y / dropout(y) / the saved c are 0
                    hnew[i] = hs[i];
                    const size_t o0 = row * p.ldy + dir * H + i;
                    p.y[o0] = 0.f;
                    if (p.ydrop) p.ydrop[o0] = 0.f;
                    if (p.sv0) p.sv1[row * ldsc + dir * H + i] = 0.f;
                    continue;
                }
            }
            const float c = fg * cs[i] + ig * gg;
            const float h = og * tanhf(c);
            cs[i] = c; hnew[i] = h;
            const size_t o = row * p.ldy + dir * H + i;
            p.y[o] = h;
            if (p.ydrop) p.ydrop[o] = h * dep_dropmask1(p.seed, p.site, o, p.drop_p, p.drop_scale);
            if (p.sv0) {
                float* gs = p.sv0 + row * ldsg + dir * 4 * H;
                gs[i] = ig; gs[H + i] = fg; gs[2 * H + i] = gg; gs[3 * H + i] = og;
                p.sv1[row * ldsc + dir * H + i] = c;
            }
        }
        __syncthreads();
        for (int i = threadIdx.x; i < H; i += GEN_T) hs[i] = hnew[i];
        __syncthreads();
    }
    if (p.h_n) for (int i = threadIdx.x; i < H; i += GEN_T) p.h_n[((size_t)dir * p.B + b) * H + i] = hs[i];
    if (p.c_n) for (int i = threadIdx.x; i < H; i += GEN_T) p.c_n[((size_t)dir * p.B + b) * H + i] = cs[i];
}

template <bool RAG = false>
__global__ __launch_bounds__(GEN_T) void lstm_bwd_generic(BwdP p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int H = p.H, T = p.T, b = blockIdx.x, dir = blockIdx.y, G4 = 4 * H;
    const int len = RAG ? dep_row_len(p.lengths, b, T) : T;
    float* dg = smem; float* dh = smem + G4; float* dc = smem + G4 + H;
    float* cx0 = smem + G4 + 2 * H;      // [H] c_prev of sweep step 0 (the forward's cx, or zeros); element i is thread i's own
    const float* W = p.d[dir].w;
    const int ldsg = p.dirs * 4 * H, ldsc = p.dirs * H;
    float* dbp = p.dbpart + ((size_t)dir * p.nwg + b) * 4 * H;
    for (int i = threadIdx.x; i < H; i += GEN_T) {
        const size_t so = ((size_t)dir * p.B + b) * H + i;
        dh[i] = p.dh_n ? p.dh_n[so] : 0.f;
        dc[i] = p.dc_n ? p.dc_n[so] : 0.f;
        cx0[i] = p.cx ? p.cx[so] : 0.f;
    }
    for (int i = threadIdx.x; i < 4 * H; i += GEN_T) dbp[i] = 0.f;
    __syncthreads();
    for (int s = T - 1; s >= 0; --s) {
        const int t = dir ? (T - 1 - s) : s;
        const size_t row = (size_t)b * T + t;
        for (int i = threadIdx.x; i < H; i += GEN_T) {
            const float* gs = p.sv0 + row * ldsg + dir * 4 * H;
            const float ig = gs[i], fg = gs[H + i], gg = gs[2 * H + i], og = gs[3 * H + i];
            const float ct = p.sv1[row * ldsc + dir * H + i];
            float cp = cx0[i];
            // (RAG: a ragged row's reverse sweep starts at t = len - 1, whose c_prev is the state as well)
            if (s > 0 && !(RAG && dir && t == len - 1)) { const size_t rowp = dir ? row + 1 : row - 1; cp = p.sv1[rowp * ldsc + dir * H + i]; }
            float d = dh[i];
            if (p.dy) {
                const size_t o = row * p.lddy + dir * H + i;
                float dyv = p.dy[o];
                if (p.drop_p > 0.f) dyv *= dep_dropmask1(p.seed, p.site, o, p.drop_p, p.drop_scale);
                d += dyv;
            }
            const float tc = tanhf(ct);
            if constexpr (RAG) {
                if (t >= len) {           // dead step (uniform over the workgroup): no gate gradient, dc and dh pass through
                    dg[i] = 0.f; dg[H + i] = 0.f; dg[2 * H + i] = 0.f; dg[3 * H + i] = 0.f;
                    float* g0 = p.dgi + row * p.lddg + dir * 4 * H;
                    g0[i] = 0.f; g0[H + i] = 0.f; g0[2 * H + i] = 0.f; g0[3 * H + i] = 0.f;
                    continue;
                }
            }
            const float dog = d * tc * og * (1.0f - og);
            const float dct = d * og * (1.0f - tc * tc) + dc[i];
            const float dig = dct * gg * ig * (1.0f - ig);
            const float dfg = dct * cp * fg * (1.0f - fg);
            const float dgg = dct * ig * (1.0f - gg * gg);
            dc[i] = dct * fg;
            dg[i] = dig; dg[H + i] = dfg; dg[2 * H + i] = dgg; dg[3 * H + i] = dog;
            float* g = p.dgi + row * p.lddg + dir * 4 * H;
            g[i] = dig; g[H + i] = dfg; g[2 * H + i] = dgg; g[3 * H + i] = dog;
            dbp[i] += dig; dbp[H + i] += dfg; dbp[2 * H + i] += dgg; dbp[3 * H + i] += dog;
        }
        __syncthreads();
        for (int i = threadIdx.x; i < H; i += GEN_T) {
            float sum = 0.f;
            for (int k = 0; k < G4; ++k) sum = fmaf(dg[k], W[(size_t)k * H + i], sum);
            if (!RAG || t < len) dh[i] = sum;      // (dead step: the incoming dh passes through)
        }
        __syncthreads();
    }
    // dh / dc past sweep step 0 are the gradients of the initial state (element i of either was last written by this thread)
    for (int i = threadIdx.x; i < H; i += GEN_T) {
        const size_t so = ((size_t)dir * p.B + b) * H + i;
        if (p.dhx) p.dhx[so] = dh[i];
        if (p.dcx) p.dcx[so] = dc[i];
    }
}

// =============================================================================== weight packing
// fwd: wp[((jt*G + g)*KC + kc)*256 + l*4 + e]  = W[(g*H + jt*16 + (l&15))*H + kc*16 + (l>>4)*4 + e],  KC = H/16
// bwd: wpT[(jt*KC2 + kc)*256 + l*4 + e]        = W[(kc*16 + (l>>4)*4 + e)*H + jt*16 + (l&15)],        KC2 = G*H/16
__global__ void pack_whh_kernel(const float* __restrict__ W, float* __restrict__ wp, float* __restrict__ wpT, int G, int H) {
    const long n = (long)G * H * H;
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    const int e = idx & 3, l = (idx >> 2) & 63;
    const long blk = idx >> 8;
    {
        const int KC = H / 16;
        const int kc = blk % KC; const long tg = blk / KC;
        const int g = tg % G; const int jt = tg / G;
        wp[idx] = W[(size_t)(g * H + jt * 16 + (l & 15)) * H + kc * 16 + (l >> 4) * 4 + e];
    }
    if (wpT) {                                        // (null: no backward reads this reserve, DEP_RUN_DROPOUT_ONLY)
        const int KC2 = G * H / 16;
        const int kc = blk % KC2; const int jt = blk / KC2;
        wpT[idx] = W[(size_t)(kc * 16 + (l >> 4) * 4 + e) * H + jt * 16 + (l & 15)];
    }
}

__global__ void finish_db_kernel(const float* __restrict__ part, int nrows, int H, int G, int cell,
                                 float* db_ih, float* db_hh) {
    // part: [nrows][4][H].  GRU (G=3): db_ih = [r,z,n_in], db_hh = [r,z,n_hid].  LSTM (G=4): both = gates.
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 4 * H) return;
    float s = 0.f;
    int r = 0;
    for (; r + 8 <= nrows; r += 8) {                          // eight loads in flight, added in row order (same sum as a plain loop)
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = part[(size_t)(r + k) * 4 * H + i];
#pragma unroll
        for (int k = 0; k < 8; ++k) s += v[k];
    }
    for (; r < nrows; ++r) s += part[(size_t)r * 4 * H + i];
    const int g = i / H, c = i % H;
    if (cell == DEP_CELL_GRU) {
        if (g < 2) { db_ih[g * H + c] = s; db_hh[g * H + c] = s; }
        else if (g == 2) db_ih[2 * H + c] = s;
        else db_hh[2 * H + c] = s;
    } else {
        db_ih[i] = s; db_hh[i] = s;
    }
}

// =============================================================================== the state's dW_hh term of a ragged call
// C[m, k] += sum over rows b with len_b > 0 of A[b, t0_b, m] * hx[b, k]   (m < M gate-gradient columns, k < H), t0_b = 0 or, for the
// reverse direction, len_b - 1: the gate gradients of each row's first sweep step against the state that step started from.  The dense
// state call forms this with a GEMM over the rows of ONE time step; here the step is per row, so the rows are gathered through LDS.
// Exact fp32 (fmaf chain), rows added in the order b = 0 .. B-1 by one thread per output element: no atomics, a pure function of the
// data.  Read-modify-write of C in stream order behind the main contraction, which wrote it with beta = 0.
constexpr int SDW = 16;      // output tile edge and rows per LDS stage
__global__ __launch_bounds__(SDW * SDW) void state_dwhh_ragged(const float* __restrict__ A, int lda, const int* __restrict__ lengths, int T, int rev,
                                                               const float* __restrict__ hx, int B, int M, int H, float* __restrict__ C) {
    __shared__ float As[SDW][SDW + 1];      // [row][gate-gradient column]
    __shared__ float Hs[SDW][SDW + 1];      // [row][hidden unit]
    const int tx = threadIdx.x & (SDW - 1), ty = threadIdx.x / SDW;
    const int m0 = blockIdx.y * SDW, k0 = blockIdx.x * SDW;
    float acc = 0.f;
    for (int b0 = 0; b0 < B; b0 += SDW) {
        const int b = b0 + ty;
        const int len = b < B ? dep_row_len(lengths, b, T) : 0;
        const bool live = len > 0;            // an empty row has no first step: it contributes nothing (a select, never value * 0)
        const size_t row = (size_t)b * T + (rev ? len - 1 : 0);
        As[ty][tx] = (live && m0 + tx < M) ? A[row * lda + m0 + tx] : 0.f;
        Hs[ty][tx] = (live && k0 + tx < H) ? hx[(size_t)b * H + k0 + tx] : 0.f;
        __syncthreads();
#pragma unroll
        for (int r = 0; r < SDW; ++r) acc = fmaf(As[r][ty], Hs[r][tx], acc);
        __syncthreads();
    }
    if (m0 + ty < M && k0 + tx < H) C[(size_t)(m0 + ty) * H + k0 + tx] += acc;
}

int pick_jpw(int H, int* nw) {
    if (H % 16) return 0;
    const int tiles = H / 16;
    for (int w = 8; w >= 1; w >>= 1) {
        if (tiles % w == 0 && tiles / w <= 4) { *nw = w; return tiles / w; }
    }
    return 0;
}

}  // namespace

bool dep_sweep_use_mfma(int H, int impl) {
    if (impl == 1) return false;
    int nw; const int jpw = pick_jpw(H, &nw);
    if (!jpw) return false;
    // backward LDS: 2 * 16 * (4H + 4) floats must fit the 160 KiB LDS
    return (size_t)2 * BT * (4 * H + LPAD) * sizeof(float) <= 160 * 1024;
}

int dep_sweep_num_wg(int B, int H, int impl) { return dep_sweep_use_mfma(H, impl) ? dep_cdiv(B, BT) : B; }

size_t dep_pack_floats(int G, int H) { return (size_t)G * H * H; }

int dep_pack_whh(const float* w_hh, float* wp, float* wpT, int G, int H, hipStream_t s) {
    const long n = (long)G * H * H;
    DEP_LAUNCH(pack_whh_kernel, dim3(dep_cdiv(n, 256)), dim3(256), 0, s, w_hh, wp, wpT, G, H);
    DEP_CHECK_LAUNCH();
    return DEP_OK;
}

#define LAUNCH_JPW(kern, grid, nthr, lds, s, P)                                                    \
    do {                                                                                           \
        if (P.lengths) {                                                                           \
            switch (jpw) {                                                                         \
                case 1: (void)hipFuncSetAttribute((const void*)kern<1, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(lds)); \
                        DEP_LAUNCH((kern<1, true>), grid, dim3(nthr), lds, s, P); break;           \
                case 2: (void)hipFuncSetAttribute((const void*)kern<2, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(lds)); \
                        DEP_LAUNCH((kern<2, true>), grid, dim3(nthr), lds, s, P); break;           \
                case 3: (void)hipFuncSetAttribute((const void*)kern<3, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(lds)); \
                        DEP_LAUNCH((kern<3, true>), grid, dim3(nthr), lds, s, P); break;           \
                default: (void)hipFuncSetAttribute((const void*)kern<4, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(lds)); \
                        DEP_LAUNCH((kern<4, true>), grid, dim3(nthr), lds, s, P); break;           \
            }                                                                                      \
        } else                                                                                     \
        switch (jpw) {                                                                             \
            case 1: (void)hipFuncSetAttribute((const void*)kern<1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(lds)); \
                    DEP_LAUNCH(kern<1>, grid, dim3(nthr), lds, s, P); break;               \
            case 2: (void)hipFuncSetAttribute((const void*)kern<2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(lds)); \
                    DEP_LAUNCH(kern<2>, grid, dim3(nthr), lds, s, P); break;               \
            case 3: (void)hipFuncSetAttribute((const void*)kern<3>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(lds)); \
                    DEP_LAUNCH(kern<3>, grid, dim3(nthr), lds, s, P); break;               \
            default: (void)hipFuncSetAttribute((const void*)kern<4>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(lds)); \
                    DEP_LAUNCH(kern<4>, grid, dim3(nthr), lds, s, P); break;               \
        }                                                                                          \
    } while (0)

// the bidirectional GRU instances kern<JPW, RAG, true> (grid.y = 2)
#define LAUNCH_JPW_BI_CASE(kern, J, RAG, grid, nthr, lds, s, P)                                    \
    (void)hipFuncSetAttribute((const void*)kern<J, RAG, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(lds)); \
    DEP_LAUNCH((kern<J, RAG, true>), grid, dim3(nthr), lds, s, P); break
#define LAUNCH_JPW_BI(kern, grid, nthr, lds, s, P)                                                 \
    do {                                                                                           \
        if (P.lengths) {                                                                           \
            switch (jpw) {                                                                         \
                case 1: LAUNCH_JPW_BI_CASE(kern, 1, true, grid, nthr, lds, s, P);                  \
                case 2: LAUNCH_JPW_BI_CASE(kern, 2, true, grid, nthr, lds, s, P);                  \
                case 3: LAUNCH_JPW_BI_CASE(kern, 3, true, grid, nthr, lds, s, P);                  \
                default: LAUNCH_JPW_BI_CASE(kern, 4, true, grid, nthr, lds, s, P);                 \
            }                                                                                      \
        } else                                                                                     \
        switch (jpw) {                                                                             \
            case 1: LAUNCH_JPW_BI_CASE(kern, 1, false, grid, nthr, lds, s, P);                     \
            case 2: LAUNCH_JPW_BI_CASE(kern, 2, false, grid, nthr, lds, s, P);                     \
            case 3: LAUNCH_JPW_BI_CASE(kern, 3, false, grid, nthr, lds, s, P);                     \
            default: LAUNCH_JPW_BI_CASE(kern, 4, false, grid, nthr, lds, s, P);                    \
        }                                                                                          \
    } while (0)

int dep_launch_sweep_fwd(const dep_sweep_args& a) {
    const int G = a.cell == DEP_CELL_GRU ? 3 : 4;
    FwdP p{};
    p.B = a.B; p.T = a.T; p.H = a.H; p.dirs = a.dirs;
    for (int d = 0; d < a.dirs; ++d) { p.d[d].wp = (const f32x4*)a.wp[d]; p.d[d].w = a.w_hh[d]; p.d[d].b_hh = a.b_hh[d]; }
    p.gi = a.gi; p.ldgi = a.dirs * G * a.H; p.y = a.y; p.ldy = a.ldy;
    p.ydrop = (a.drop_p > 0.f) ? a.ydrop : nullptr;
    p.drop_p = a.drop_p; p.drop_scale = a.drop_p > 0.f ? 1.0f / (1.0f - a.drop_p) : 1.0f; p.seed = a.seed; p.site = a.site;
    p.pooled = a.pooled; p.pool_scale = a.pool_scale; p.h_n = a.h_n;
    p.sv0 = a.training ? a.sv0 : nullptr; p.sv1 = a.sv1; p.sv2 = a.sv2; p.sv3 = a.sv3;
    p.lengths = a.lengths; p.pool_mean = a.pool_mean;
    p.hx = a.hx; p.cx = a.cx; p.c_n = a.c_n;
    DEP_CHECK_ARG(a.y && a.gi);
    DEP_CHECK_ARG(a.cell == DEP_CELL_LSTM || (!a.cx && !a.c_n));                  // a GRU has no cell state
    const bool bigru = a.cell == DEP_CELL_GRU && a.dirs == 2;
    DEP_CHECK_ARG(!bigru || dep_sweep_use_mfma(a.H, a.impl));      // a bidirectional GRU has tile-MFMA instances only
    DepProfScope prof(a.cell == DEP_CELL_GRU ? DEP_PROF_GRU_FWD : DEP_PROF_LSTM_FWD, a.stream);
    if (dep_sweep_use_mfma(a.H, a.impl)) {
        int nw = 0; const int jpw = pick_jpw(a.H, &nw);
        const size_t lds = (size_t)2 * BT * (a.H + LPAD) * sizeof(float);
        dim3 grid(dep_cdiv(a.B, BT), a.dirs);
        if (bigru) LAUNCH_JPW_BI(gru_fwd_mfma, grid, nw * 64, lds, a.stream, p);
        else if (a.cell == DEP_CELL_GRU) LAUNCH_JPW(gru_fwd_mfma, grid, nw * 64, lds, a.stream, p);
        else LAUNCH_JPW(lstm_fwd_mfma, grid, nw * 64, lds, a.stream, p);
    } else {
        dim3 grid(a.B, a.dirs);
        const size_t lds = (size_t)3 * a.H * sizeof(float);
        if (a.lengths) {
            if (a.cell == DEP_CELL_GRU) DEP_LAUNCH(gru_fwd_generic<true>, grid, dim3(GEN_T), lds, a.stream, p);
            else DEP_LAUNCH(lstm_fwd_generic<true>, grid, dim3(GEN_T), lds, a.stream, p);
        } else if (a.cell == DEP_CELL_GRU) DEP_LAUNCH(gru_fwd_generic<>, grid, dim3(GEN_T), lds, a.stream, p);
        else DEP_LAUNCH(lstm_fwd_generic<>, grid, dim3(GEN_T), lds, a.stream, p);
    }
    DEP_CHECK_LAUNCH();
    return DEP_OK;
}

int dep_launch_sweep_bwd(const dep_sweep_bwd_args& a) {
    const int G = a.cell == DEP_CELL_GRU ? 3 : 4;
    BwdP p{};
    p.B = a.B; p.T = a.T; p.H = a.H; p.dirs = a.dirs;
    for (int d = 0; d < a.dirs; ++d) { p.d[d].wp = (const f32x4*)a.wpT[d]; p.d[d].w = a.w_hh[d]; p.d[d].b_hh = nullptr; }
    p.y = a.y; p.ldy = a.ldy; p.dy = a.dy; p.lddy = a.lddy;
    p.drop_p = a.dy ? a.drop_p : 0.f; p.drop_scale = a.drop_p > 0.f ? 1.0f / (1.0f - a.drop_p) : 1.0f;
    p.seed = a.seed; p.site = a.site;
    p.dpooled = a.dpooled; p.pool_scale = a.pool_scale; p.dh_n = a.dh_n;
    p.sv0 = a.sv0; p.sv1 = a.sv1; p.sv2 = a.sv2; p.sv3 = a.sv3;
    p.dgi = a.dgi; p.lddg = a.dirs * G * a.H; p.dghn = a.dghn; p.dbpart = a.dbpart;
    p.nwg = dep_sweep_num_wg(a.B, a.H, a.impl);
    p.lengths = a.lengths; p.pool_mean = a.pool_mean;
    p.hx = a.hx; p.cx = a.cx; p.dc_n = a.dc_n; p.dhx = a.dhx; p.dcx = a.dcx;
    DEP_CHECK_ARG(a.cell == DEP_CELL_LSTM || (!a.cx && !a.dc_n && !a.dcx));       // a GRU has no cell state
    DEP_CHECK_ARG(a.dbpart_rows >= p.nwg * a.dirs);
    DEP_CHECK_ARG(a.sv0 && a.dgi && a.dbpart);
    const bool bigru = a.cell == DEP_CELL_GRU && a.dirs == 2;
    DEP_CHECK_ARG(!bigru || dep_sweep_use_mfma(a.H, a.impl));      // a bidirectional GRU has tile-MFMA instances only
    DepProfScope prof(a.cell == DEP_CELL_GRU ? DEP_PROF_GRU_BWD : DEP_PROF_LSTM_BWD, a.stream);
    if (dep_sweep_use_mfma(a.H, a.impl)) {
        int nw = 0; const int jpw = pick_jpw(a.H, &nw);
        const size_t lds = (size_t)2 * BT * (G * a.H + LPAD) * sizeof(float);
        dim3 grid(dep_cdiv(a.B, BT), a.dirs);
        if (bigru) LAUNCH_JPW_BI(gru_bwd_mfma, grid, nw * 64, lds, a.stream, p);
        else if (a.cell == DEP_CELL_GRU) LAUNCH_JPW(gru_bwd_mfma, grid, nw * 64, lds, a.stream, p);
        else LAUNCH_JPW(lstm_bwd_mfma, grid, nw * 64, lds, a.stream, p);
    } else {
        dim3 grid(a.B, a.dirs);
        const size_t lds = (size_t)(G * a.H + 3 * a.H) * sizeof(float);      // gate gradients, dh, dc, and h / c before step 0
        if (a.lengths) {
            if (a.cell == DEP_CELL_GRU) DEP_LAUNCH(gru_bwd_generic<true>, grid, dim3(GEN_T), lds, a.stream, p);
            else DEP_LAUNCH(lstm_bwd_generic<true>, grid, dim3(GEN_T), lds, a.stream, p);
        } else if (a.cell == DEP_CELL_GRU) DEP_LAUNCH(gru_bwd_generic<>, grid, dim3(GEN_T), lds, a.stream, p);
        else DEP_LAUNCH(lstm_bwd_generic<>, grid, dim3(GEN_T), lds, a.stream, p);
    }
    DEP_CHECK_LAUNCH();
    return DEP_OK;
}

int dep_state_dwhh_ragged(const float* dg, int lddg, const int* lengths, int B, int T, int reverse, const float* hx, int M, int H, float* dw_hh,
                          hipStream_t s) {
    DEP_CHECK_ARG(dg && lengths && hx && dw_hh && B > 0 && T > 0 && M > 0 && H > 0 && lddg >= M);
    DEP_LAUNCH(state_dwhh_ragged, dim3(dep_cdiv(H, SDW), dep_cdiv(M, SDW)), dim3(SDW * SDW), 0, s, dg, lddg, lengths, T, reverse ? 1 : 0, hx, B, M, H,
               dw_hh);
    DEP_CHECK_LAUNCH();
    return DEP_OK;
}

int dep_finish_db(const dep_sweep_bwd_args& a, float* const* db_ih, float* const* db_hh) {
    const int G = a.cell == DEP_CELL_GRU ? 3 : 4;
    DEP_CHECK_ARG(a.dirs >= 1 && a.dbpart_rows >= a.dirs && a.dbpart_rows % a.dirs == 0);
    const int nwg = a.dbpart_rows / a.dirs;           // rows per direction the sweep that ran has written
    for (int d = 0; d < a.dirs; ++d) {
        DEP_LAUNCH(finish_db_kernel, dim3(dep_cdiv(4 * a.H, 128)), dim3(128), 0, a.stream,
                           a.dbpart + (size_t)d * nwg * 4 * a.H, nwg, a.H, G, a.cell, db_ih[d], db_hh[d]);
        DEP_CHECK_LAUNCH();
    }
    return DEP_OK;
}
