// Cluster-parallel sweeps for the bidirectional LSTM (nn.LSTM of Classification/text_bilstm_whole.py:54-56,105;
// gates i,f,g,o; h0 = c0 = 0).  Same scheme as the GRU kernels of rnn_cluster_bwd.hip: a (direction, 16-utterance
// tile) pair is owned by a cluster of NC = H/32 workgroups, member c keeps the W_hh rows of hidden units
// [32c, 32c+32) (all four gates) in VGPRs for the whole sweep, h_t (forward) / the partial dh (backward) travel
// through flag-published fp32 payloads with the same-XCD fast path, parity double-buffering and bounded spins.
// Both directions run in the same launch: at H = 128, B = 512 that is 2 x 32 tiles x 4 members = 256 workgroups.
// Both biases are folded into the input projection by the caller (dep_rnn_forward), as in rnn_sweep.hip.
#include "rnn_cluster_launch.h"

namespace {
using namespace depc;

struct LF {
    int B, T, H, dirs, nbtp, b0;      // b0: first utterance of this launch's batch chunk (B is the whole batch)
    const f32x4* wp[2];
    const float* gi; int ldgi;
    float* y; int ldy;
    float* ydrop; float drop_p, drop_scale; uint64_t seed; uint32_t site;
    float* h_n;
    float* svg; float* svc;                        // activated gates (B,T,dirs*4H), cell state (B,T,dirs*H); null in inference
    unsigned* status; unsigned* flags; unsigned* hello; float* payload; unsigned payload_bytes;
    int nofast;
    long long* trace;        // debug: shader-clock stamps of workgroup 0 (DEP_TRACE=1, tools/trace_lstm.py), else nullptr
    const int* lengths;      // ragged instances (RAG): row b is live for t < lengths[b]
};

struct LB {
    int B, T, H, dirs, nbtp, b0;      // b0: first utterance of this launch's batch chunk (B is the whole batch)
    const f32x4* wp[2];
    const float* dy; int lddy;
    float drop_p, drop_scale; uint64_t seed; uint32_t site;
    const float* dh_n;
    const float* svg; const float* svc;
    float* dgi; int lddg;
    float* dbpart; int nwg;
    unsigned* status; unsigned* flags; unsigned* hello; float* payload; unsigned payload_bytes;
    int nofast;
    int dgpk;                // gate gradients as the PK image of gemm_bf16x3.hip (burst kernel, T even)
    long long* trace;        // debug: shader-clock stamps of workgroup 0 (DEP_TRACE=1, tools/trace_lstm.py bwd), else nullptr
    const int* lengths;      // ragged instances (RAG): row b is live for t < lengths[b]
};

// block id = (dir*NC + c)*nbtp + bt  (nbtp a multiple of 8: all members of a cluster share blockIdx % 8)
// The launchers take H == 128 only (DEP_CHECK_ARG in dep_launch_cluster_lstm_fwd / _bwd, dep_cluster_lstm_ok), which fixes
constexpr int KCH = 4;                               // forward: k-chunks of 16 per wave = H/32
constexpr int NTW = 2;                               // backward: output tiles per wave = H/64
constexpr int KB = 4;                                // slots of the service waves' input ring = steps per burst of the exact-fp32 sweeps
// =============================================================================== forward
// Service waves, as in gru_bwd_cluster_r1 (a CU returns vector loads in issue order across its waves, so every HBM request
// of a step would sit in front of that step's flag polls and gather).  Four service waves (threads CT .. CT+255) own every HBM access of
// the member: they bring the input projection into the LDS ring `ibuf' (step k in slot k % KB) and write h, dropout(h), the four
// activated gates and c out of the LDS ring `obuf' (KB+1 slots), which is all the compute waves touch.  Two sweeps share that frame:
//
// !SPLIT, the exact-fp32 sweep through LDS planes.  64 v_mfma_f32_16x16x4_f32 per wave and step.  A member publishes its 32 units of h_t
// as fp32 into the parity-double-buffered payload, raises ONE flag behind a workgroup barrier, every wave polls the NC flags, and the
// 16 x H block is copied into an fp32 LDS plane: three barriers per step.  The service waves move KB steps at a time -- on a cluster's
// dirty step (every KB-th; the clusters of an XCD take turns) they request steps k+KB .. k+2KB-1 (registers for KB-1 steps, then the
// ring) and write out the last KB steps.
//
// SPLIT, the split-precision direct-fragment sweep.  Recurrent products on the bf16 matrix cores with the 3-term split, as in the GRU
// sweeps (rnn_cluster16.hip): 24 v_mfma_f32_16x16x32_bf16 per wave and step (384 vs 2048 cycles); gates, c and h themselves stay fp32.
// A member publishes h_t ONCE as the (hi, lo) bf16 words in the matrix cores' B-fragment order ([plane][64 lanes][16 B] = 2 KB per member
// and step: lane (k-group u / 8, utterance j), word (u % 8) / 2), and a consumer wave loads the four 1 KB blocks of the two source members
// of its K half straight into registers -- no LDS planes, no unpacking, ONE workgroup barrier per step (behind the K-half partial sums).
// The data are their own flag: a member publishes into one of FOUR slots (step k -> slot k % 4) whose words hold a SENTINEL until they
// are written -- 0xffffffff, a pair of bf16 NaNs no finite h produces (a NaN input is published as 0x7fc07fc0) -- and a consumer simply
// loads its four fragment blocks until none of its sixteen words is the sentinel: no acknowledgement wait, no flag store, no separate
// poll.  With step k's data a member re-arms its slot (k + 2) % 4 (it held step k-2: every reader of that finished before the member
// could gate step k); that store is acknowledged before the member's next publish is even issued (the load loop's vmcnt(0)), and nobody
// polls slot (k + 2) % 4 before having consumed that next publish -- so a poll never meets the slot's previous tenant.  The slots are
// armed in the kernel's prologue, in front of the hello rendezvous.  The service waves stream EVERY step where it hurts nothing
// (rnn_fused2_bwd.hip's schedule): the write-out of step k-1 (14 KB of posted stores) at the top of step k, the input projection of
// step k+2 (8 KB) once the four compute waves have nothing in the CU's queue any more (an LDS counter), landing in the ring a step
// later; the odd service waves draw the inter-layer dropout mask and form dropout(h) at write-out.  (How the sweep got here -- planes,
// flags, bursts -- is in DESIGN_HISTORY.md.)
constexpr int L_SVC = 256;
constexpr int LROW = 36, LARR = 16 * LROW;           // LDS row stride / array size (floats) of ibuf / obuf
constexpr int LF_TRACE_F = 144;                      // floats behind the rings: 64 debug stamps, then the issue-signal word of the per-step streams
constexpr int LF_RINGS = KB * 4 * LARR + (KB + 1) * 7 * LARR + LF_TRACE_F;
constexpr size_t LF_LDS_PLANES = ((size_t)BT * (128 + 8) + 4 * 4 * 64 * 4 + LF_RINGS) * sizeof(float);      // h plane (16 rows of H + LPAD, allotted as H + 8), K-half partial sums, rings
constexpr size_t LF_LDS_DIRECT = ((size_t)4096 + LF_RINGS) * sizeof(float);                                 // partial sums of two step parities, rings
constexpr int DF_MEMBER_BYTES = 2 * 1024;
constexpr unsigned DF_SENT = 0xffffffffu;

// SV16: the saved activated gates are 16-bit fixed point -- i, f, o in (0, 1) as unorm16, g in (-1, 1) as snorm16
// (rnn_cluster_common.h; same element positions inside the (B,T,dirs*4H) array, 2 bytes each); c stays fp32.
// RAG: the ragged-batch instances (dep_rnn_forward_varlen).  live = t < lengths[b], per lane, in the gate phase of the compute waves:
// (h, c) = live ? new : previous -- what is published, carried and returned as h_n, so the forward direction freezes behind its last
// step and the reverse direction walks the padding with its zero state and starts for real at t = lengths[b] - 1; h, dropout(h) and
// the saved c go out as 0 at dead positions (the backward reads c_{t-1} there).  The hand-off is the dense instance's, step for step.
template <bool SPLIT, bool SV16 = false, bool RAG = false>
__global__ __launch_bounds__(CT + L_SVC) void lstm_fwd_cluster(LF p) {
    // contraction by syntax: see DEP_FP_CONTRACT_NOTE in dep_common.h (why, and how to re-verify the dense instances after a compiler change)
#pragma clang fp contract(on)
    static_assert(SPLIT || !SV16, "16-bit saved gates: split-precision mode");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int H = p.H, T = p.T, LDH = H + LPAD, KC = H / 16, NC = H / 32;
    const int bt = blockIdx.x % p.nbtp, dc = blockIdx.x / p.nbtp, c = dc % NC, dir = dc / NC;
    if (p.b0 + bt * BT >= p.B) return;
    if (ld_agent(p.status) != 0) return;           // an earlier sweep of this step gave up: the status word is sticky until the next dep_rnn_forward
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int j = lane & 15, q = lane >> 4, jl = w >> 1, kh = w & 1;
    const int jt = c * 2 + jl;
    const int b = p.b0 + bt * BT + j;
    const bool valid = b < p.B;
    int len = T;
    if constexpr (RAG) len = (valid && tid < CT) ? dep_row_len(p.lengths, b, T) : 0;
    float* hs = smem;                                 // !SPLIT: [16][LDH] fp32
    const int hs_floats = BT * LDH;
    float* red = SPLIT ? smem : smem + hs_floats;     // [4 waves][4 gates][64][4]   (SPLIT: [step parity][4 waves][4 gates][64][2], no plane)
    float* ibuf = red + (SPLIT ? 4096 : 4 * 4 * 64 * 4);      // [KB][4 gates][16][LROW]: input projection of step k in slot k % KB
    float* obuf = ibuf + KB * 4 * LARR;               // [KB+1][7][16][LROW]: h, dropout(h), i, f, g, o, c of step k in slot k % (KB+1)
    long long* trl = reinterpret_cast<long long*>(obuf + (KB + 1) * 7 * LARR);       // debug stamps (LF_TRACE_F floats)
    unsigned* sig = reinterpret_cast<unsigned*>(trl) + 128;                          // SPLIT: compute waves whose fragment loads have landed, summed over the steps
    if (SPLIT && tid == 0) *sig = 0;                  // (ordered by the prologue's __syncthreads)
    const bool svc = tid >= CT;                       // wave-uniform
    if constexpr (!SPLIT) for (int i = tid; i < hs_floats; i += CT + L_SVC) hs[i] = 0.f;

    constexpr int KS2 = KCH / 2;                      // 32-wide k-steps per wave (SPLIT)
    f32x4 wr[SPLIT ? 1 : 4][SPLIT ? 1 : KCH];
    u32x4 wq[SPLIT ? 4 : 1][SPLIT ? KS2 : 1][2];      // [gate][k-step][hi, lo]
    if (svc) {
    } else if constexpr (SPLIT) {
        const u32x4* wpq = reinterpret_cast<const u32x4*>(p.wp[dir]);
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int ks = 0; ks < KS2; ++ks)
#pragma unroll
                for (int pl = 0; pl < 2; ++pl)
                    wq[g][ks][pl] = wpq[(size_t)((((jt * 4 + g) * 2 + kh) * KS2 + ks) * 2 + pl) * 64 + lane];
    } else {
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int k = 0; k < KCH; ++k)
                wr[g][k] = p.wp[dir][(size_t)((jt * 4 + g) * KC + kh * KCH + k) * 64 + lane];
    }
    const int col = jt * 16 + q * 4 + 2 * kh;
    float2 cst = f2(0.f, 0.f), hlast = f2(0.f, 0.f);
    const int cl = dir * p.nbtp + bt;                 // cluster index
    const size_t pstride = (size_t)p.dirs * p.nbtp * BT * H;
    const size_t tile_base = (size_t)cl * BT * H;
    __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)p.payload, 0, p.payload_bytes, 0x00020000);
    const int m0 = cl * NC;                           // the cluster's first member (SPLIT: its place in the exchange buffer)
    unsigned* tflags = nullptr, * myflag = nullptr;   // !SPLIT: one flag per member
    if constexpr (!SPLIT) { tflags = p.flags + cl * NC; myflag = tflags + c; }
    const int hshift = __ffs(H) - 1;
    const int ldsg = p.dirs * 4 * H, ldsc = p.dirs * H;
    if constexpr (SPLIT) {
        // arm this member's words of all four slots (write-through: the placement is not known yet), then the hello is the rendezvous
        if (!svc) {
            const int ulc0 = jt * 16 + q * 4 + 2 * kh - 32 * c;
            const unsigned pw0 = (unsigned)((((ulc0 >> 3) * 16 + j) << 2) + ((ulc0 & 7) >> 1));
            const unsigned pb0 = (unsigned)(m0 + c) * DF_MEMBER_BYTES + pw0 * 4, pbs = (unsigned)p.dirs * p.nbtp * NC * DF_MEMBER_BYTES;
#pragma unroll
            for (int sl = 0; sl < 4; ++sl) {
                __builtin_amdgcn_raw_buffer_store_b32(DF_SENT, rsrc, pb0 + sl * pbs, 0, 16);
                __builtin_amdgcn_raw_buffer_store_b32(DF_SENT, rsrc, pb0 + sl * pbs + 1024, 0, 16);
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __syncthreads();
    }
    const int sx = (p.nofast && !SPLIT) ? 0 : cluster_same_xcd(p.hello + cl * NC, NC, c, p.status);     // (SPLIT: the rendezvous is needed either way)
    if (sx < 0) return;
    const bool fast = sx == 1 && !p.nofast;
    if (svc) {
        // ---- the service waves' whole life.  Thread st: piece idx = st + 256 i of a step's pieces -> array idx / 128 (wave-
        // uniform: waves 4, 5 even arrays, waves 6, 7 odd ones), utterance row (idx % 128) / 8, 16-byte piece idx % 8.
        const int st = tid - CT, sr = (st >> 3) & 15, sp = st & 7;
        const bool sodd = __builtin_amdgcn_readfirstlane((st >> 7) & 1) != 0;
        const int sb = p.b0 + bt * BT + sr;
        const bool svalid = sb < p.B;
        const int scol = 32 * c + sp * 4;
        const int phi = (bt >> 3) % KB;               // the clusters of an XCD take their dirty steps in turn
        f32x4 sreg[KB][2];
        auto tstep = [&](int k) { return dir ? T - 1 - k : k; };
        // the tile's rows of every streamed array, non-temporal (rnn_cluster_common.h)
        const size_t trow0 = (size_t)(p.b0 + bt * BT) * T, trows = (size_t)BT * T;
        const NtArr a_gi = nt_arr(p.gi, trow0 * p.ldgi * 4, trows * p.ldgi * 4);
        const NtArr a_y = nt_arr(sodd ? p.ydrop : p.y, trow0 * p.ldy * 4, trows * p.ldy * 4);
        const NtArr a_g = nt_arr(p.svg, trow0 * ldsg * (SV16 ? 2 : 4), trows * ldsg * (SV16 ? 2 : 4));
        const NtArr a_c = nt_arr(p.svc, trow0 * ldsc * 4, trows * ldsc * 4);
        auto svc_issue = [&](int k0, int n) {         // input projection of steps k0 .. k0+n-1 -> registers (gates sodd, sodd + 2)
#pragma unroll
            for (int d = 0; d < KB; ++d)
                if (d < n) {
                    const int k = k0 + d;
                    const bool on = svalid && k < T;
                    const float* src = p.gi + ((size_t)sb * T + tstep(k)) * p.ldgi + dir * 4 * H + (sodd ? H : 0) + scol;
                    sreg[d][0] = on ? nt_ld4(a_gi, src) : zero4();
                    sreg[d][1] = on ? nt_ld4(a_gi, src + 2 * H) : zero4();
                }
        };
        auto svc_put = [&](int k0, int n) {
#pragma unroll
            for (int d = 0; d < KB; ++d)
                if (d < n) {
                    float* dst = ibuf + ((k0 + d) % KB) * 4 * LARR + (sodd ? LARR : 0) + sr * LROW + sp * 4;
                    *reinterpret_cast<f32x4*>(dst) = sreg[d][0];
                    *reinterpret_cast<f32x4*>(dst + 2 * LARR) = sreg[d][1];
                }
        };
        // write-out arrays: 0 h, 1 dropout(h), 2..5 the activated gates, 6 c.  Even waves: 0, 2, 4, 6; odd waves: 1, 3, 5.
        float* const ybase = sodd ? p.ydrop : p.y;
        // mk4 (SPLIT): the odd waves form dropout(h) themselves -- h times the mask of the piece's four positions -- instead of reading a second array
        auto svc_flush = [&](int k0, int k1, const f32x4* mk4 = nullptr) {
            if (!svalid) return;
            for (int k = k0 < 0 ? 0 : k0; k < k1; ++k) {
                const size_t row = (size_t)sb * T + tstep(k);
                const float* o = obuf + (k % (KB + 1)) * 7 * LARR + sr * LROW + sp * 4;
                if (ybase) {
                    f32x4 v = ld4(o + ((sodd && !mk4) ? LARR : 0));
                    if (sodd && mk4) { v[0] *= (*mk4)[0]; v[1] *= (*mk4)[1]; v[2] *= (*mk4)[2]; v[3] *= (*mk4)[3]; }
                    nt_st4(a_y, ybase + row * p.ldy + dir * H + scol, v);
                }
                if (p.svg) {
                    if constexpr (SV16) {                 // even waves: i (unorm), g (snorm) ; odd waves: f, o (unorm)
                        unsigned short* gs16 = reinterpret_cast<unsigned short*>(p.svg) + row * ldsg + dir * 4 * H + scol;
                        const f32x4 v0 = ld4(o + (sodd ? 3 : 2) * LARR), v1 = ld4(o + (sodd ? 5 : 4) * LARR);
                        nt_st2w(a_g, gs16 + (sodd ? H : 0), pack_unorm2(v0[0], v0[1]), pack_unorm2(v0[2], v0[3]));
                        if (sodd) nt_st2w(a_g, gs16 + 3 * H, pack_unorm2(v1[0], v1[1]), pack_unorm2(v1[2], v1[3]));
                        else nt_st2w(a_g, gs16 + 2 * H, pack_snorm2(v1[0], v1[1]), pack_snorm2(v1[2], v1[3]));
                    } else {
                        float* gs = p.svg + row * ldsg + dir * 4 * H + scol;
                        nt_st4(a_g, gs + (sodd ? H : 0), ld4(o + (sodd ? 3 : 2) * LARR));
                        nt_st4(a_g, gs + (sodd ? 3 * H : 2 * H), ld4(o + (sodd ? 5 : 4) * LARR));
                    }
                    if (!sodd) nt_st4(a_c, p.svc + row * ldsc + dir * H + scol, ld4(o + 6 * LARR));
                }
            }
        };
        if constexpr (SPLIT) {
            // per-step streams (see above): one register set, one step in flight.  Iteration k, between barrier(k-1) and barrier(k):
            // ring <- gi(k+1) (requested a step ago); write-out of step k-1; wait for the issue signal; request gi(k+2).
            // The inter-layer dropout mask is drawn HERE (odd waves, one Philox call per 16-byte piece, an iteration ahead, behind the
            // requests): on the compute waves the draw (~700 ticks of VALU for half as many useful values) would sit between the
            // fragment requests and the MFMAs, and the requests return in less than that.
            const bool sdrop = sodd && p.ydrop != nullptr;        // wave-uniform
            auto sdraw = [&](int k) {
                const size_t o = ((size_t)sb * T + tstep(k)) * p.ldy + dir * H + scol;
                return dep_dropmask4(p.seed, p.site, o >> 2, p.drop_p, p.drop_scale);
            };
            f32x4 mk4 = {1.f, 1.f, 1.f, 1.f};                     // mask of the step the next iteration writes out
            svc_issue(0, 1); svc_put(0, 1); svc_issue(1, 1);
            __syncthreads();
            for (int k = 0; k < T; ++k) {
                if (k + 1 < T) svc_put(k + 1, 1);
                if (k > 0) svc_flush(k - 1, k, &mk4);
                if (k + 2 < T) {
                    const unsigned want = 4u * ((unsigned)k + 1u);
                    // (a scheduling hint, not a dependency: give up after ~1 ms -- a compute wave that left on a raised status never raises it)
                    for (int spin = 0; spin < 20000 && sig_read(sig) < want; ++spin) __builtin_amdgcn_s_sleep(1);
                }
                if (k + 2 < T) svc_issue(k + 2, 1);
                if (sdrop) mk4 = sdraw(k);
                bar_lds();
            }
            svc_flush(T - 1, T, &mk4);
            return;
        }
        svc_issue(0, KB); svc_put(0, KB);             // steps 0 .. KB-1 straight into the ring
        svc_issue(KB, phi);                           // steps KB .. KB+phi-1: written at step phi-1, before the first dirty step (k = phi)
        __syncthreads();
        for (int k = 0; k < T; ++k) {                 // same barrier sequence as the compute waves: three per step, one in the last
            const int jj = (k + KB - phi) % KB, last = k - jj;
            if (jj == 0) { svc_issue(k + KB, KB); svc_flush(k - KB, k); }
            bar_lds();                               // #1 (partial sums)
            if (k == T - 1) break;
            bar_lds();                               // #2 (the compute waves' drain barrier): step k's ring slot is consumed
            if (jj == KB - 1) { if (last >= 0) svc_put(last + KB, KB); else svc_put(KB, phi); }
            bar_lds();                               // #3 (gathered h in LDS)
        }
        __syncthreads();                              // the last step's results are in obuf
        svc_flush(T - 1 - (T - 1 + KB - phi) % KB, T);
        return;
    }
    __syncthreads();                                  // (shared with the service waves' prologue)

    // debug stamps (DEP_TRACE=1, tools/trace_lstm.py): workgroup 0, wave 0, steps 196 .. 199, buffered in LDS, copied out after the sweep
    long long* trb = (p.trace && blockIdx.x == 0 && tid == 0) ? p.trace : nullptr;
#define LSTAMP(k_, slot) do { if (trb && (k_) >= 196 && (k_) < 200) trl[((k_) - 196) * 8 + (slot)] = (long long)__builtin_readcyclecounter(); } while (0)
    if (trb) { for (int i = 0; i < 64; ++i) trl[i] = 0; trl[7] = (long long)__builtin_readcyclecounter(); }
    if constexpr (SPLIT) {
        // ---- direct-fragment sweep.  Exchange buffer: [slot][cluster][member][plane][64 lanes][16 B]; this thread's pair (units ulc,
        // ulc+1 of utterance j) is word `pw' of its member's two 1 KB blocks.
        const int ulc = col - 32 * c;                 // = 16 jl + 4 q + 2 kh
        const unsigned pw = (unsigned)((((ulc >> 3) * 16 + j) << 2) + ((ulc & 7) >> 1));
        const unsigned par_bytes = (unsigned)p.dirs * p.nbtp * NC * DF_MEMBER_BYTES;
        const unsigned pub0 = (unsigned)(m0 + c) * DF_MEMBER_BYTES + pw * 4;
        const unsigned ld0 = (unsigned)(m0 + 2 * kh) * DF_MEMBER_BYTES + lane * 16;      // this wave's four blocks are contiguous: members 2kh, 2kh+1
        const bool khu = __builtin_amdgcn_readfirstlane(kh) != 0;
        float2 rec[4] = {f2(0.f, 0.f), f2(0.f, 0.f), f2(0.f, 0.f), f2(0.f, 0.f)};      // W_hh h_{k-1} of this thread's pair (h_{-1} = 0)
        for (int k = 0; k < T; ++k) {
            const bool more = k + 1 < T;
            LSTAMP(k, 0);
            const float* ib = ibuf + (k % KB) * 4 * LARR + j * LROW + ulc;
            float2 tot[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) { const float2 gv = ld2(ib + g * LARR); tot[g] = f2(rec[g].x + gv.x, rec[g].y + gv.y); }
            float2 ig, fg, gg, og, h;
            ig.x = fast_sigmoid(tot[0].x); ig.y = fast_sigmoid(tot[0].y);
            fg.x = fast_sigmoid(tot[1].x); fg.y = fast_sigmoid(tot[1].y);
            gg.x = fast_tanh(tot[2].x); gg.y = fast_tanh(tot[2].y);
            og.x = fast_sigmoid(tot[3].x); og.y = fast_sigmoid(tot[3].y);
            float2 cn = f2(fg.x * cst.x + ig.x * gg.x, fg.y * cst.y + ig.y * gg.y);
            h.x = og.x * fast_tanh(cn.x); h.y = og.y * fast_tanh(cn.y);
            float2 hy = h;                            // what h, dropout(h) and the saved c show of this step
            if constexpr (RAG) {
                const bool live = (dir ? T - 1 - k : k) < len;
                h = dep_sel2(live, h, hlast); cst = dep_sel2(live, cn, cst);
                hy = dep_sel2(live, h, f2(0.f, 0.f)); cn = dep_sel2(live, cn, f2(0.f, 0.f));
            } else {
                cst = cn;
            }
            hlast = h;
            if (more) {       // publish first: the (hi, lo) pair words of h_k -- what every member's MFMAs read -- and re-arm slot (k + 2) % 4
                unsigned hw, lw;
                split_pair(h.x, h.y, hw, lw);
                if (hw == DF_SENT) hw = 0x7fc07fc0u;          // (NaN inputs only) never the sentinel
                if (lw == DF_SENT) lw = 0x7fc07fc0u;
                const unsigned po = (unsigned)(k & 3) * par_bytes + pub0, pr = (unsigned)((k + 2) & 3) * par_bytes + pub0;
                if (fast) {   // same-XCD clusters: plain stores (that XCD's L2 is the coherence point)
                    __builtin_amdgcn_raw_buffer_store_b32(hw, rsrc, po, 0, 0); __builtin_amdgcn_raw_buffer_store_b32(lw, rsrc, po + 1024, 0, 0);
                    __builtin_amdgcn_raw_buffer_store_b32(DF_SENT, rsrc, pr, 0, 0); __builtin_amdgcn_raw_buffer_store_b32(DF_SENT, rsrc, pr + 1024, 0, 0);
                } else {      // write-through
                    __builtin_amdgcn_raw_buffer_store_b32(hw, rsrc, po, 0, 16); __builtin_amdgcn_raw_buffer_store_b32(lw, rsrc, po + 1024, 0, 16);
                    __builtin_amdgcn_raw_buffer_store_b32(DF_SENT, rsrc, pr, 0, 16); __builtin_amdgcn_raw_buffer_store_b32(DF_SENT, rsrc, pr + 1024, 0, 16);
                }
            }
            {
                float* ob = obuf + (k % (KB + 1)) * 7 * LARR + j * LROW + ulc;
                st2(ob, hy);                          // (dropout(h): the service waves form it at write-out)
                if (p.svg) { st2(ob + 2 * LARR, ig); st2(ob + 3 * LARR, fg); st2(ob + 4 * LARR, gg); st2(ob + 5 * LARR, og); st2(ob + 6 * LARR, cn); }
            }
            LSTAMP(k, 1);
            if (!more) { bar_lds(); break; }          // (the service waves' final flush reads obuf behind this barrier)
            u32x4 hfr[KS2][2];
            {                                         // the hand-off: load this wave's four fragment blocks of step k until none of them shows the sentinel
                LSTAMP(k, 2); LSTAMP(k, 3);
                const unsigned lo_ = (unsigned)(k & 3) * par_bytes + ld0;
                for (unsigned spins = 0;; ++spins) {
#pragma unroll
                    for (int ks = 0; ks < KS2; ++ks)
#pragma unroll
                        for (int pl = 0; pl < 2; ++pl)
                            hfr[ks][pl] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, lo_ + (unsigned)(ks * 2 + pl) * 1024, 0, 16 /* sc1: served by L2 */);
                    unsigned mn = 0xffffffffu;            // min over the sixteen words of ~word: 0 <=> one of them is still the sentinel (branch-free)
#pragma unroll
                    for (int ks = 0; ks < KS2; ++ks)
#pragma unroll
                        for (int pl = 0; pl < 2; ++pl) {
                            const u32x4 v = hfr[ks][pl];
                            mn = min(min(min(mn, ~v.x), min(~v.y, ~v.z)), ~v.w);
                        }
                    if (!__any(mn == 0u)) break;
                    if (spins > SPIN_LIMIT) { st_agent(p.status, 6); return; }
                    if ((spins & 63) == 63 && ld_agent(p.status) != 0) return;
                }
                LSTAMP(k, 4);
                if (lane == 0) sig_raise(sig);            // nothing of this wave is in the CU's queue any more: the service waves may issue their requests
            }
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_sched_barrier(0);
            f32x4 acc[4] = {zero4(), zero4(), zero4(), zero4()};
#pragma unroll
            for (int ks = 0; ks < KS2; ++ks) {
                const bf16x8 hh = __builtin_bit_cast(bf16x8, hfr[ks][0]), hl = __builtin_bit_cast(bf16x8, hfr[ks][1]);
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const bf16x8 wh = __builtin_bit_cast(bf16x8, wq[g][ks][0]), wl = __builtin_bit_cast(bf16x8, wq[g][ks][1]);
                    acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh, hl, acc[g], 0, 0, 0);
                    acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wl, hh, acc[g], 0, 0, 0);
                    acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh, hh, acc[g], 0, 0, 0);
                }
            }
            // the partner wave (other K half, same tile) needs the two units this wave does NOT keep.  (khu: a SCALAR copy of kh -- with the
            // per-lane value hipcc indexes the sixteen accumulator registers dynamically: 128 v_cmp / v_cndmask pairs, 1600 ticks a step)
            float2 keep[4], send[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                if (khu) { keep[g] = f2(acc[g][2], acc[g][3]); send[g] = f2(acc[g][0], acc[g][1]); }
                else     { keep[g] = f2(acc[g][0], acc[g][1]); send[g] = f2(acc[g][2], acc[g][3]); }
            }
            float* rw = red + (((k & 1) * 4 + w) * 4) * 128 + lane * 2;
#pragma unroll
            for (int g = 0; g < 4; ++g) st2(rw + g * 128, send[g]);
            LSTAMP(k, 5);
            bar_lds();
            const float* rr = red + (((k & 1) * 4 + (w ^ 1)) * 4) * 128 + lane * 2;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float2 pv = ld2(rr + g * 128);
                rec[g] = f2(keep[g].x + pv.x, keep[g].y + pv.y);
            }
            LSTAMP(k, 6);
        }
    } else {
        // ---- exact-fp32 sweep through the LDS plane
        for (int s = 0; s < T; ++s) {
            const int t = dir ? (T - 1 - s) : s;
            const size_t row = (size_t)b * T + t;
            const bool more = s + 1 < T;
            LSTAMP(s, 0);
            f32x4 acc[4] = {zero4(), zero4(), zero4(), zero4()};
            const float* hrow = hs + j * LDH + kh * KCH * 16 + q * 4;
            f32x4 hv[KCH];
#pragma unroll
            for (int k = 0; k < KCH; ++k) hv[k] = ld4(hrow + k * 16);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int k = 0; k < KCH; ++k)
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int g = 0; g < 4; ++g)
                        acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[g][k][e], hv[k][e], acc[g], 0, 0, 0);
#pragma unroll
            for (int g = 0; g < 4; ++g) *reinterpret_cast<f32x4*>(red + ((w * 4 + g) * 64 + lane) * 4) = acc[g];
            LSTAMP(s, 1);
            bar_lds();
            const int ulc = col - 32 * c;             // this lane's pair of units inside the member's 32
            const float* ib = ibuf + (s % KB) * 4 * LARR + j * LROW + ulc;
            float2 gi[4], tot[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) gi[g] = ld2(ib + g * LARR);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float2 pv = ld2(red + (((w ^ 1) * 4 + g) * 64 + lane) * 4 + 2 * kh);
                tot[g].x = (kh ? acc[g][2] : acc[g][0]) + pv.x + gi[g].x;
                tot[g].y = (kh ? acc[g][3] : acc[g][1]) + pv.y + gi[g].y;
            }
            float2 ig, fg, gg, og, h;
            ig.x = fast_sigmoid(tot[0].x); ig.y = fast_sigmoid(tot[0].y);
            fg.x = fast_sigmoid(tot[1].x); fg.y = fast_sigmoid(tot[1].y);
            gg.x = fast_tanh(tot[2].x); gg.y = fast_tanh(tot[2].y);
            og.x = fast_sigmoid(tot[3].x); og.y = fast_sigmoid(tot[3].y);
            float2 cn = f2(fg.x * cst.x + ig.x * gg.x, fg.y * cst.y + ig.y * gg.y);
            h.x = og.x * fast_tanh(cn.x); h.y = og.y * fast_tanh(cn.y);
            float2 hy = h;                            // what h, dropout(h) and the saved c show of this step
            if constexpr (RAG) {
                const bool live = t < len;
                h = dep_sel2(live, h, hlast); cst = dep_sel2(live, cn, cst);
                hy = dep_sel2(live, h, f2(0.f, 0.f)); cn = dep_sel2(live, cn, f2(0.f, 0.f));
            } else {
                cst = cn;
            }
            hlast = h;
            const unsigned epoch = (unsigned)s + 1u;
            const size_t pbase = (size_t)(s & 1) * pstride + tile_base;
            if (more) {
                const u64 bits = (u64)__float_as_uint(h.x) | ((u64)__float_as_uint(h.y) << 32);
                gu64* dst = (gu64*)(p.payload + pbase + (size_t)j * H + col);
                if (fast) __hip_atomic_store(dst, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                else __hip_atomic_store(dst, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                LSTAMP(s, 2);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();
                if (tid == 0) { if (fast) st_local(myflag, epoch); else st_agent(myflag, epoch); }
                LSTAMP(s, 3);
            }
            {
                float* ob = obuf + (s % (KB + 1)) * 7 * LARR + j * LROW + ulc;
                st2(ob, hy);
                if (p.ydrop) {
                    const size_t o = row * p.ldy + dir * H + col;
                    const f32x4 m = dep_dropmask4(p.seed, p.site, o >> 2, p.drop_p, p.drop_scale);
                    st2(ob + LARR, f2(hy.x * (kh ? m[2] : m[0]), hy.y * (kh ? m[3] : m[1])));
                }
                if (p.svg) { st2(ob + 2 * LARR, ig); st2(ob + 3 * LARR, fg); st2(ob + 4 * LARR, gg); st2(ob + 5 * LARR, og); st2(ob + 6 * LARR, cn); }
            }
            if (more) {
                LSTAMP(s, 4);
                if (!wait_flags(tflags, NC, epoch, p.status, 6)) return;      // every wave polls: no verdict-broadcast barrier
                LSTAMP(s, 5);
                constexpr int PER = KCH / 2;          // 16-byte pieces per thread = 16*H/4/256
#pragma unroll
                for (int k = 0; k < PER; ++k) {
                    const int i4 = (tid + CT * k) * 4;
                    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (unsigned)((pbase + i4) * 4), 0, 16 /* sc1 */);
                    f32x4 f;
                    f[0] = __uint_as_float(v.x); f[1] = __uint_as_float(v.y); f[2] = __uint_as_float(v.z); f[3] = __uint_as_float(v.w);
                    *reinterpret_cast<f32x4*>(hs + (i4 >> hshift) * LDH + (i4 & (H - 1))) = f;
                }
                bar_lds();
                LSTAMP(s, 6);
            }
        }
        __syncthreads();                              // the service waves flush the last steps after this (SPLIT: barrier(T-1) was that)
    }
    if (valid && p.h_n) st2(p.h_n + ((size_t)dir * p.B + b) * H + col, hlast);
    if (trb) { trl[15] = (long long)__builtin_readcyclecounter(); for (int i = 0; i < 32; ++i) trb[i] = trl[i]; }
#undef LSTAMP
}

// =============================================================================== backward
struct StepIn { float2 ig, fg, gg, og, ct, cp, dy; };

// The service waves (see lstm_fwd_cluster / gru_bwd_cluster_r1) bring the saved gates, c_t, c_{t-1} and dy into the LDS ring `ibuf'
// (step k = T-1-s in slot k % KB) and write the four gate gradients out of the ring `obuf'.  The exchange is the reduce-scatter of fp32
// partial dh in both modes (with H = 128 a member's gate gradients are as large as its partials: an all-gather form has nothing to save).
// !SPLIT, exact fp32: bursts of KB steps on a cluster's dirty step, one flag per member behind a drain barrier, two barriers per step.
// SPLIT: the 3-term bf16 products, with per-step streams and per-wave flags --
// * every compute wave raises its OWN epoch flag once its two partial tiles are acknowledged and every wave polls all 4 NC flags (which also
//   orders a step's reads of the gate-gradient planes before the next step's writes): no drain barrier, ONE barrier per step;
// * the service waves stream every step: the gate gradients of step k-1 (8 KB, or a PK pair every other step) go out at the top of their
//   iteration, the saved gates / c / dy of step k+2 (14 KB) are requested once the four compute waves have their gather loads of step k-1
//   in the CU's queue (an LDS counter) and land in the ring an iteration later -- no dirty step; the even service waves draw the dropout
//   mask of the incoming dy and apply it as dy enters the ring.
constexpr int LB_IBUF = 2304;                        // float offset of ibuf (the gate-gradient planes live in [0, 2304))
constexpr int LB_OSLOTS = KB + 2;                    // KB + 1 would do for fp32 rows; the PK flush works on step pairs and may lag one step
constexpr size_t LB_LDS = ((size_t)LB_IBUF + KB * 7 * LARR + LB_OSLOTS * 4 * LARR + LF_TRACE_F) * sizeof(float);
// RAG: the ragged-batch instances (dep_rnn_backward_varlen): a dead step's four gate gradients are 0 and its incoming dh, dc pass through
// to the next BPTT step unchanged (selects in the compute waves' gate phase; the hand-off and the streams are the dense instance's).
template <bool SPLIT, bool SV16 = false, bool RAG = false>      // SV16: 16-bit saved gates, as in the forward
__global__ __launch_bounds__(CT + L_SVC) void lstm_bwd_cluster(LB p) {
    static_assert(SPLIT || !SV16, "16-bit saved gates: split-precision mode");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int KS = 128, KCB = KS / 16, LDG = KS + LPAD;
    constexpr int LDGB = KS + 8;                      // bf16 elements per row of a split plane
    const int H = p.H, T = p.T, NC = H / 32, NTT = H / 16;
    const int bt = blockIdx.x % p.nbtp, dc = blockIdx.x / p.nbtp, c = dc % NC, dir = dc / NC;
    if (p.b0 + bt * BT >= p.B) return;
    if (ld_agent(p.status) != 0) return;           // an earlier sweep of this step gave up: the status word is sticky until the next dep_rnn_forward
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int jl = tid >> 7, lp = (tid >> 1) & 63, half = tid & 1;
    const int j = lp & 15, ul = jl * 16 + (lp >> 4) * 4 + 2 * half;
    const int col = 32 * c + ul;
    const int b = p.b0 + bt * BT + j;
    const bool valid = b < p.B;
    float* dgs = smem;                                // [16][LDG] fp32, or (SPLIT) two bf16 planes [16][LDGB]
    unsigned short* dg_hi = reinterpret_cast<unsigned short*>(smem);
    unsigned short* dg_lo = dg_hi + BT * LDGB;

    const bool svc = tid >= CT;                       // wave-uniform
    float* ibuf = smem + LB_IBUF;                     // [KB][7][16][LROW]: i, f, g, o, c_t, c_{t-1}, dy of step k (k = T-1-s) in slot k % KB
    float* obuf = ibuf + KB * 7 * LARR;              // [KB+1][4][16][LROW]: di, df, dg, do of step k in slot k % (KB+1)
    long long* trl = reinterpret_cast<long long*>(obuf + LB_OSLOTS * 4 * LARR);      // debug stamps (LF_TRACE_F floats)
    unsigned* sig = reinterpret_cast<unsigned*>(trl) + 128;                                     // SPLIT: gather loads issued so far, all compute waves
    if (SPLIT && tid == 0) *sig = 0;                     // (ordered by the prologue's __syncthreads)
    f32x4 wr[SPLIT ? 1 : NTW][SPLIT ? 1 : KCB];
    u32x4 wq[SPLIT ? NTW : 1][SPLIT ? 4 : 1][2];      // [tile][k-step = gate][hi, lo]
    if (svc) {
    } else if constexpr (SPLIT) {
        const u32x4* wpq = reinterpret_cast<const u32x4*>(p.wp[dir]);
#pragma unroll
        for (int i = 0; i < NTW; ++i)
#pragma unroll
            for (int ks = 0; ks < 4; ++ks)
#pragma unroll
                for (int pl = 0; pl < 2; ++pl)
                    wq[i][ks][pl] = wpq[(size_t)(((c * NTT + w * NTW + i) * 4 + ks) * 2 + pl) * 64 + lane];
    } else {
#pragma unroll
        for (int i = 0; i < NTW; ++i)
#pragma unroll
            for (int k = 0; k < KCB; ++k)
                wr[i][k] = p.wp[dir][(size_t)((c * NTT + w * NTW + i) * KCB + k) * 64 + lane];
    }
    float2 dhrec = (p.dh_n && valid && !svc) ? ld2(p.dh_n + ((size_t)dir * p.B + b) * H + col) : f2(0.f, 0.f);
    float2 dcrec = f2(0.f, 0.f);
    int len = T;
    if constexpr (RAG) len = (valid && !svc) ? dep_row_len(p.lengths, b, T) : 0;
    float2 db[4] = {f2(0.f, 0.f), f2(0.f, 0.f), f2(0.f, 0.f), f2(0.f, 0.f)};
    const int cl = dir * p.nbtp + bt;
    const size_t pstride = (size_t)p.dirs * p.nbtp * NC * BT * H;
    const size_t tile_base = (size_t)cl * NC * BT * H;
    __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)p.payload, 0, p.payload_bytes, 0x00020000);
    unsigned* tflags = SPLIT ? p.flags + cl * NC * 4 : p.flags + cl * NC;    // SPLIT: one flag per compute wave
    unsigned* myflag = SPLIT ? tflags + c * 4 + (w & 3) : tflags + c;
    const int ml = lane & 15, mq = lane >> 4;
    const int ldsg = p.dirs * 4 * H, ldsc = p.dirs * H;
    const int sx = p.nofast ? 0 : cluster_same_xcd(p.hello + cl * NC, NC, c, p.status);
    if (sx < 0) return;
    const bool fast = sx == 1;

    if (svc) {
        // ---- the service waves' whole life (thread -> piece mapping as in lstm_fwd_cluster; step counter k = T-1-s)
        const int st = tid - CT, sr = (st >> 3) & 15, sp = st & 7;
        const bool sodd = __builtin_amdgcn_readfirstlane((st >> 7) & 1) != 0;
        const int sb = p.b0 + bt * BT + sr;
        const bool svalid = sb < p.B;
        const int scol = 32 * c + sp * 4;
        const int phi = (bt >> 3) % KB;
        f32x4 sreg[KB][4];
        // the tile's rows of every streamed array, non-temporal (rnn_cluster_common.h)
        const size_t trow0 = (size_t)(p.b0 + bt * BT) * T, trows = (size_t)BT * T;
        const NtArr a_g = nt_arr(p.svg, trow0 * ldsg * (SV16 ? 2 : 4), trows * ldsg * (SV16 ? 2 : 4));
        const NtArr a_c = nt_arr(p.svc, trow0 * ldsc * 4, trows * ldsc * 4);
        const NtArr a_dy = nt_arr(p.dy, trow0 * p.lddy * 4, trows * p.lddy * 4);
        const NtArr a_dg = nt_arr(p.dgi, trow0 * p.lddg * 4, trows * p.lddg * 4);
        // input arrays: even waves 0 i, 2 g, 4 c_t, 6 dy ; odd waves 1 f, 3 o, 5 c_{t-1}
        auto svc_issue = [&](int k0, int n) {
#pragma unroll
            for (int d = 0; d < KB; ++d)
                if (d < n) {
                    const int sstep = T - 1 - (k0 + d);
                    const bool on = svalid && sstep >= 0;
                    const int t = dir ? (T - 1 - sstep) : sstep;
                    const size_t row = (size_t)sb * T + t;
                    if constexpr (SV16) {                 // four 16-bit values = 8 bytes per slot, decoded in svc_put
                        const unsigned short* gs16 = reinterpret_cast<const unsigned short*>(p.svg) + row * ldsg + dir * 4 * H + (sodd ? H : 0) + scol;
                        const float2 w0 = on ? nt_ld2w(a_g, gs16) : f2(0.f, 0.f), w1 = on ? nt_ld2w(a_g, gs16 + 2 * H) : f2(0.f, 0.f);
                        sreg[d][0][0] = w0.x; sreg[d][0][1] = w0.y; sreg[d][1][0] = w1.x; sreg[d][1][1] = w1.y;
                    } else {
                        const float* gs = p.svg + row * ldsg + dir * 4 * H + (sodd ? H : 0) + scol;
                        sreg[d][0] = on ? nt_ld4(a_g, gs) : zero4();
                        sreg[d][1] = on ? nt_ld4(a_g, gs + 2 * H) : zero4();
                    }
                    const size_t rowc = sodd ? (dir ? row + 1 : row - 1) : row;       // odd waves: c of the previous time step of this direction
                    sreg[d][2] = (on && (!sodd || sstep > 0)) ? nt_ld4(a_c, p.svc + rowc * ldsc + dir * H + scol) : zero4();
                    sreg[d][3] = (on && !sodd && p.dy) ? nt_ld4(a_dy, p.dy + row * p.lddy + dir * H + scol) : zero4();
                }
        };
        // mk4 (SPLIT): the even waves apply the inter-layer dropout mask to the incoming dy as they put it into the ring
        auto svc_put = [&](int k0, int n, const f32x4* mk4 = nullptr) {
#pragma unroll
            for (int d = 0; d < KB; ++d)
                if (d < n) {
                    float* dst = ibuf + ((k0 + d) % KB) * 7 * LARR + (sodd ? LARR : 0) + sr * LROW + sp * 4;
                    if constexpr (SV16) {                 // slot 0: i / f (unorm) ; slot 1: g (snorm, even waves) / o (unorm, odd waves)
                        const unsigned a0 = __float_as_uint(sreg[d][0][0]), a1 = __float_as_uint(sreg[d][0][1]);
                        const unsigned b0 = __float_as_uint(sreg[d][1][0]), b1 = __float_as_uint(sreg[d][1][1]);
                        const float2 x0 = unpack_unorm2(a0), x1 = unpack_unorm2(a1);
                        const float2 y0 = sodd ? unpack_unorm2(b0) : unpack_snorm2(b0), y1 = sodd ? unpack_unorm2(b1) : unpack_snorm2(b1);
                        const f32x4 v0 = {x0.x, x0.y, x1.x, x1.y}, v1 = {y0.x, y0.y, y1.x, y1.y};
                        *reinterpret_cast<f32x4*>(dst) = v0;
                        *reinterpret_cast<f32x4*>(dst + 2 * LARR) = v1;
                    } else {
                        *reinterpret_cast<f32x4*>(dst) = sreg[d][0];
                        *reinterpret_cast<f32x4*>(dst + 2 * LARR) = sreg[d][1];
                    }
                    *reinterpret_cast<f32x4*>(dst + 4 * LARR) = sreg[d][2];
                    if (!sodd) {
                        f32x4 v = sreg[d][3];
                        if (mk4) { v[0] *= (*mk4)[0]; v[1] *= (*mk4)[1]; v[2] *= (*mk4)[2]; v[3] *= (*mk4)[3]; }
                        *reinterpret_cast<f32x4*>(dst + 6 * LARR) = v;
                    }
                }
        };
        auto svc_flush = [&](int k0, int k1) {    // gate gradients of steps k0 .. k1-1: even waves di, dg ; odd waves df, do
            if (!svalid) return;
            for (int k = k0 < 0 ? 0 : k0; k < k1; ++k) {
                const int sstep = T - 1 - k, t = dir ? (T - 1 - sstep) : sstep;
                const float* o = obuf + (k % LB_OSLOTS) * 4 * LARR + (sodd ? LARR : 0) + sr * LROW + sp * 4;
                float* g = p.dgi + ((size_t)sb * T + t) * p.lddg + dir * 4 * H + (sodd ? H : 0) + scol;
                nt_st4(a_dg, g, ld4(o));
                nt_st4(a_dg, g + 2 * H, ld4(o + 2 * LARR));
            }
        };
        // PK image of the gate gradients (p.dgpk; gemm_bf16x3.hip FMT_PK, see gru_bwd_cluster_r1): the steps (ka, ka + 1), ka even,
        // are two adjacent time steps of the utterance -- rows (T-2-ka, T-1-ka) for the forward direction, (ka, ka+1) for the reverse
        // one; the even row holds the bf16 hi pairs of both, the odd row the residual pairs.  Same bytes, same bits in the GEMMs.
        auto svc_flush_pk = [&](int k0, int k1) {
            if (!svalid) return;
            for (int ka = k0 < 0 ? 0 : k0; ka + 1 < k1; ka += 2) {
                const int t_even = dir ? ka : T - 2 - ka;
                const float* o0 = obuf + (ka % LB_OSLOTS) * 4 * LARR + (sodd ? LARR : 0) + sr * LROW + sp * 4;
                const float* o1 = obuf + ((ka + 1) % LB_OSLOTS) * 4 * LARR + (sodd ? LARR : 0) + sr * LROW + sp * 4;
                const float* oe = dir ? o0 : o1;      // the step that is row t_even
                const float* oo = dir ? o1 : o0;      // ... row t_even + 1
                float* g = p.dgi + ((size_t)sb * T + t_even) * p.lddg + dir * 4 * H + (sodd ? H : 0) + scol;
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    const f32x4 xe = ld4(oe + q * 2 * LARR), xo = ld4(oo + q * 2 * LARR);
                    u32x4 hw, lw;
#pragma unroll
                    for (int e = 0; e < 4; ++e) { unsigned hh, ll; split_pair(xe[e], xo[e], hh, ll); hw[e] = hh; lw[e] = ll; }
                    nt_st4(a_dg, g + q * 2 * H, __builtin_bit_cast(f32x4, hw));
                    nt_st4(a_dg, g + q * 2 * H + p.lddg, __builtin_bit_cast(f32x4, lw));
                }
            }
        };
        if constexpr (SPLIT) {
            // per-step streams (see above): one register set, one step in flight.  Iteration k, between barrier(k-1) and barrier(k):
            // ring <- inputs of step k+1 (requested an iteration ago); gate gradients of step k-1 (PK: of the pair (k-2, k-1), k even);
            // wait for the compute waves' gather loads of step k-1 to be in the queue; request the inputs of step k+2.
            // The dropout mask of the incoming dy is drawn HERE (even waves, one Philox call per 16-byte piece, behind the requests of the step
            // it belongs to) and applied as dy enters the ring: on the compute waves the draw is the floor of the poll phase.
            const bool sdrop = !sodd && p.dy && p.drop_p > 0.f;   // wave-uniform
            auto sdraw = [&](int k) {
                const int sstep = T - 1 - k, t = dir ? (T - 1 - sstep) : sstep;
                const size_t o = ((size_t)sb * T + t) * p.lddy + dir * H + scol;
                return dep_dropmask4(p.seed, p.site, o >> 2, p.drop_p, p.drop_scale);
            };
            f32x4 mk4 = {1.f, 1.f, 1.f, 1.f};                     // mask of the step the next put moves into the ring
            svc_issue(0, 1); if (sdrop) mk4 = sdraw(0);
            svc_put(0, 1, &mk4);
            svc_issue(1, 1); if (sdrop && T > 1) mk4 = sdraw(1);
            __syncthreads();
            for (int k = 0; k < T; ++k) {
                if (k + 1 < T) svc_put(k + 1, 1, &mk4);
                if (p.dgpk) { if (k >= 2 && !(k & 1)) svc_flush_pk(k - 2, k); }
                else if (k > 0) svc_flush(k - 1, k);
                if (k + 2 < T) {
                    const unsigned want = 4u * (unsigned)k;
                    // (a scheduling hint, not a dependency: give up after ~1 ms -- a compute wave that left on a raised status never raises it)
                    for (int spin = 0; spin < 20000 && sig_read(sig) < want; ++spin) __builtin_amdgcn_s_sleep(1);
                    svc_issue(k + 2, 1);
                    if (sdrop) mk4 = sdraw(k + 2);
                }
                bar_lds();
            }
            if (p.dgpk) svc_flush_pk(T - 2, T); else svc_flush(T - 1, T);
            return;
        }
        svc_issue(0, KB); svc_put(0, KB);
        svc_issue(KB, phi);
        __syncthreads();
        for (int k = 0; k < T; ++k) {             // same barrier sequence as the compute waves: two per step, one in the last
            const int jj = (k + KB - phi) % KB, last = k - jj;
            if (jj == 0) { svc_issue(k + KB, KB); if (p.dgpk) svc_flush_pk(k - KB - (phi & 1), k - (phi & 1)); else svc_flush(k - KB, k); }
            bar_lds();                           // #1
            if (jj == KB - 1) { if (last >= 0) svc_put(last + KB, KB); else svc_put(KB, phi); }
            if (k == T - 1) break;
            bar_lds();                           // #2 (the compute waves' drain barrier)
        }
        if (p.dgpk) svc_flush_pk(T - 1 - (T - 1 + KB - phi) % KB - (phi & 1), T);
        else svc_flush(T - 1 - (T - 1 + KB - phi) % KB, T);
        return;
    }
    __syncthreads();
    StepIn cur;
    // dropout mask of the incoming dy: drawn one step ahead while waiting for the other members (see rnn_cluster_bwd.hip)
    const bool masked = !SPLIT && p.dy && p.drop_p > 0.f && valid;   // (SPLIT: the service waves draw the mask and apply it as dy enters the ring)
    auto draw = [&](int s) {
        const int t = dir ? (T - 1 - s) : s;
        const size_t o = ((size_t)b * T + t) * p.lddy + dir * H + col;
        const f32x4 m = dep_dropmask4(p.seed, p.site, o >> 2, p.drop_p, p.drop_scale);
        return f2(half ? m[2] : m[0], half ? m[3] : m[1]);
    };
    float2 mk = masked ? draw(T - 1) : f2(1.f, 1.f);
    // debug stamps (DEP_TRACE=1, tools/trace_lstm.py bwd): workgroup 0, wave 0, steps k = 196 .. 199, buffered in LDS, copied out after the sweep
    long long* trb = (p.trace && blockIdx.x == 0 && tid == 0) ? p.trace : nullptr;
#define LSTAMP(k_, slot) do { if (trb && (k_) >= 196 && (k_) < 200) trl[((k_) - 196) * 8 + (slot)] = (long long)__builtin_readcyclecounter(); } while (0)
    if (trb) { for (int i = 0; i < 64; ++i) trl[i] = 0; trl[7] = (long long)__builtin_readcyclecounter(); }

    for (int s = T - 1; s >= 0; --s) {
        const int t = dir ? (T - 1 - s) : s;
        LSTAMP(T - 1 - s, 0);
        const float* ib = ibuf + ((T - 1 - s) % KB) * 7 * LARR + j * LROW + ul;
        cur.ig = ld2(ib); cur.fg = ld2(ib + LARR); cur.gg = ld2(ib + 2 * LARR); cur.og = ld2(ib + 3 * LARR);
        cur.ct = ld2(ib + 4 * LARR); cur.cp = ld2(ib + 5 * LARR); cur.dy = ld2(ib + 6 * LARR);
        const float2 dyv = f2(cur.dy.x * mk.x, cur.dy.y * mk.y);
        const float2 ig = cur.ig, fg = cur.fg, gg = cur.gg, og = cur.og, cp = cur.cp;
        const float2 d = f2(dhrec.x + dyv.x, dhrec.y + dyv.y);
        const float2 tc = f2(fast_tanh(cur.ct.x), fast_tanh(cur.ct.y));
        float2 dog, dct, dig, dfg, dgg;
        dog.x = d.x * tc.x * og.x * (1.0f - og.x); dog.y = d.y * tc.y * og.y * (1.0f - og.y);
        dct.x = d.x * og.x * (1.0f - tc.x * tc.x) + dcrec.x; dct.y = d.y * og.y * (1.0f - tc.y * tc.y) + dcrec.y;
        dig.x = dct.x * gg.x * ig.x * (1.0f - ig.x); dig.y = dct.y * gg.y * ig.y * (1.0f - ig.y);
        dfg.x = dct.x * cp.x * fg.x * (1.0f - fg.x); dfg.y = dct.y * cp.y * fg.y * (1.0f - fg.y);
        dgg.x = dct.x * ig.x * (1.0f - gg.x * gg.x); dgg.y = dct.y * ig.y * (1.0f - gg.y * gg.y);
        const bool live = !RAG || t < len;
        const float2 digr = dig, dfgr = dfg, dggr = dgg, dogr = dog;
        if constexpr (RAG) {
            const float2 z2 = f2(0.f, 0.f);
            dog = dep_sel2(live, dog, z2); dig = dep_sel2(live, dig, z2); dfg = dep_sel2(live, dfg, z2); dgg = dep_sel2(live, dgg, z2);
            dcrec = dep_sel2(live, f2(dct.x * fg.x, dct.y * fg.y), dcrec);
        } else {
            dcrec.x = dct.x * fg.x; dcrec.y = dct.y * fg.y;
        }
        if constexpr (SPLIT) {
            unsigned hh[4], ll[4];
            if constexpr (RAG) {          // the words of the unselected values (rounded as the dense instance rounds them), zeroed for a dead step
                split_pair(digr.x, digr.y, hh[0], ll[0]); split_pair(dfgr.x, dfgr.y, hh[1], ll[1]);
                split_pair(dggr.x, dggr.y, hh[2], ll[2]); split_pair(dogr.x, dogr.y, hh[3], ll[3]);
                if (!live) { for (int g = 0; g < 4; ++g) { hh[g] = 0u; ll[g] = 0u; } }
            } else {
                split_pair(dig.x, dig.y, hh[0], ll[0]); split_pair(dfg.x, dfg.y, hh[1], ll[1]);
                split_pair(dgg.x, dgg.y, hh[2], ll[2]); split_pair(dog.x, dog.y, hh[3], ll[3]);
            }
            const int o = j * LDGB + ul;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                *reinterpret_cast<unsigned*>(dg_hi + o + 32 * g) = hh[g]; *reinterpret_cast<unsigned*>(dg_lo + o + 32 * g) = ll[g];
            }
        } else {
            float* dl = dgs + j * LDG + ul;
            st2(dl, dig); st2(dl + 32, dfg); st2(dl + 64, dgg); st2(dl + 96, dog);
        }
        float* ob = obuf + ((T - 1 - s) % LB_OSLOTS) * 4 * LARR + j * LROW + ul;
        st2(ob, dig); st2(ob + LARR, dfg); st2(ob + 2 * LARR, dgg); st2(ob + 3 * LARR, dog);
        db[0].x += dig.x; db[0].y += dig.y; db[1].x += dfg.x; db[1].y += dfg.y;
        db[2].x += dgg.x; db[2].y += dgg.y; db[3].x += dog.x; db[3].y += dog.y;
        LSTAMP(T - 1 - s, 1);
        bar_lds();
        LSTAMP(T - 1 - s, 2);
        if (s == 0) break;
        f32x4 acc[NTW];
#pragma unroll
        for (int i = 0; i < NTW; ++i) acc[i] = zero4();
        if constexpr (SPLIT) {
            const int go = ml * LDGB + mq * 8;
            bf16x8 gh[4], gl[4];
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                gh[ks] = *reinterpret_cast<const bf16x8*>(dg_hi + go + ks * 32);
                gl[ks] = *reinterpret_cast<const bf16x8*>(dg_lo + go + ks * 32);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int ks = 0; ks < 4; ++ks)
#pragma unroll
                for (int i = 0; i < NTW; ++i) {
                    const bf16x8 wh = __builtin_bit_cast(bf16x8, wq[i][ks][0]), wl = __builtin_bit_cast(bf16x8, wq[i][ks][1]);
                    acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh, gl[ks], acc[i], 0, 0, 0);
                    acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wl, gh[ks], acc[i], 0, 0, 0);
                    acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh, gh[ks], acc[i], 0, 0, 0);
                }
        } else {
            const float* drow = dgs + ml * LDG + mq * 4;
            f32x4 hv[KCB];
#pragma unroll
            for (int k = 0; k < KCB; ++k) hv[k] = ld4(drow + k * 16);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int k = 0; k < KCB; ++k)
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int i = 0; i < NTW; ++i)
                        acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[i][k][e], hv[k][e], acc[i], 0, 0, 0);
        }
        const unsigned epoch = (unsigned)(T - s);
        const size_t pbase = (size_t)(s & 1) * pstride + tile_base;
#pragma unroll
        for (int i = 0; i < NTW; ++i) {
            const size_t fo = pbase + ((size_t)(c * NTT + w * NTW + i) * 64 + lane) * 4;
            u32x4 v;
            v.x = __float_as_uint(acc[i][0]); v.y = __float_as_uint(acc[i][1]);
            v.z = __float_as_uint(acc[i][2]); v.w = __float_as_uint(acc[i][3]);
            if (fast) __builtin_amdgcn_raw_buffer_store_b128(v, rsrc, (unsigned)(fo * 4), 0, 0);
            else __builtin_amdgcn_raw_buffer_store_b128(v, rsrc, (unsigned)(fo * 4), 0, 16);
        }
        LSTAMP(T - 1 - s, 3);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if constexpr (SPLIT) {
            // per-wave flags: this wave's partial tiles are acknowledged -> say so; nobody waits for the sibling waves here (their flags are
            // among the 4 NC words every wave polls below: a sibling raises its flag only after its MFMAs have read the gate-gradient planes)
            if (lane == 0) { if (fast) st_local(myflag, epoch); else st_agent(myflag, epoch); }
        } else {
            __builtin_amdgcn_s_barrier();
            if (tid == 0) { if (fast) st_local(myflag, epoch); else st_agent(myflag, epoch); }
        }
        LSTAMP(T - 1 - s, 4);
        if (masked) mk = draw(s - 1);                // next step's mask, in the shadow of the wait below
        if (!wait_flags(tflags, SPLIT ? 4 * NC : NC, epoch, p.status, 7)) return;
        LSTAMP(T - 1 - s, 5);
        const float* src = p.payload + pbase + ((size_t)(2 * c + jl) * 64 + lp) * 4 + 2 * half;
        float2 part[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) part[m] = (m < NC) ? ld2_agent(src + (size_t)m * NTT * 256) : f2(0.f, 0.f);
        if constexpr (SPLIT) {
            __builtin_amdgcn_sched_barrier(0);
            if (lane == 0) sig_raise(sig);           // this wave's gather loads are in the CU's queue: the service waves may issue theirs
            __builtin_amdgcn_sched_barrier(0);
        }
        float2 sum = f2(0.f, 0.f);
#pragma unroll
        for (int m = 0; m < 4; ++m) { sum.x += part[m].x; sum.y += part[m].y; }
        if constexpr (RAG) dhrec = dep_sel2(live, sum, dhrec);      // dead step: the incoming dh passes through
        else dhrec = sum;
        LSTAMP(T - 1 - s, 6);
    }
    if (trb) { trl[15] = (long long)__builtin_readcyclecounter(); for (int i = 0; i < 32; ++i) trb[i] = trl[i]; }
#undef LSTAMP
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int m = 2; m <= 16; m <<= 1) { db[k].x += __shfl_xor(db[k].x, m, 64); db[k].y += __shfl_xor(db[k].y, m, 64); }
    if (j == 0) {
        float* o = p.dbpart + ((size_t)dir * p.nwg + p.b0 / BT + bt) * 4 * H;
#pragma unroll
        for (int k = 0; k < 4; ++k) st2(o + k * H + col, db[k]);
    }
}

// split-precision weight images (rnn_cluster_common.h, G = 4): the forward's, and the backward's when `bwd` is set -- equally many pieces
__global__ void pack_lstm_split_kernel(const float* __restrict__ W, u32x4* __restrict__ fwd, u32x4* __restrict__ bwd, int H) {
    const long n = pack_fwd_split_pieces(4, H);
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    pack_fwd_split_piece<4>(W, fwd, H, idx);
    if (bwd) pack_bwd_split_piece<4>(W, bwd, H, idx);
}

// ---- the launchable instances (H = 128; the service waves own the HBM streams -- DESIGN 4.1c)
// exact-fp32 mode: h_t through the LDS plane; split products: the direct-fragment exchange with sentinel slots
Instance<LF>& fwd_instance(bool split, bool sv16, bool rag) {
    static Instance<LF> exact DEP_INSTANCE((lstm_fwd_cluster<false>), LF_LDS_PLANES);
    static Instance<LF> direct[2] = { DEP_INSTANCE((lstm_fwd_cluster<true, false>), LF_LDS_DIRECT), DEP_INSTANCE((lstm_fwd_cluster<true, true>), LF_LDS_DIRECT) };
    // ... and the ragged-batch instances of the same forms (dep_rnn_forward_varlen)
    static Instance<LF> rexact DEP_INSTANCE((lstm_fwd_cluster<false, false, true>), LF_LDS_PLANES);
    static Instance<LF> rdirect[2] = { DEP_INSTANCE((lstm_fwd_cluster<true, false, true>), LF_LDS_DIRECT), DEP_INSTANCE((lstm_fwd_cluster<true, true, true>), LF_LDS_DIRECT) };
    if (rag) return split ? rdirect[sv16] : rexact;
    return split ? direct[sv16] : exact;
}
// exact-fp32 mode: burst streams, one flag per member behind a drain barrier; split products: per-step streams + per-wave flags
Instance<LB>& bwd_instance(bool split, bool sv16, bool rag) {
    static Instance<LB> exact DEP_INSTANCE((lstm_bwd_cluster<false>), LB_LDS);
    static Instance<LB> perstep[2] = { DEP_INSTANCE((lstm_bwd_cluster<true, false>), LB_LDS), DEP_INSTANCE((lstm_bwd_cluster<true, true>), LB_LDS) };
    static Instance<LB> rexact DEP_INSTANCE((lstm_bwd_cluster<false, false, true>), LB_LDS);
    static Instance<LB> rperstep[2] = { DEP_INSTANCE((lstm_bwd_cluster<true, false, true>), LB_LDS), DEP_INSTANCE((lstm_bwd_cluster<true, true, true>), LB_LDS) };
    if (rag) return split ? rperstep[sv16] : rexact;
    return split ? perstep[sv16] : exact;
}

// the backward's two parities of NC x 16 x H fp32 per cluster; the forward's four slots of 16 x H (the direct sweep; the exact one uses two)
ChunkGeometry lstm_geometry(int H, int dirs, int B) { return chunk_geometry(dirs * (H / 32), 1, 256, B); }      // one workgroup per CU per launch
size_t lstm_bwd_payload_bytes(const ChunkGeometry& g, int H) { return (size_t)2 * g.nbtp_max * g.members * BT * H * sizeof(float); }
size_t lstm_fwd_payload_bytes(const ChunkGeometry& g, int H, int dirs) { return (size_t)4 * dirs * g.nbtp_max * BT * H * sizeof(float); }

}  // namespace

void dep_cluster_lstm_instance_texts(dep_instance_sink add) {
    for (int m = 0; m < 8; ++m) { add(fwd_instance(m & 1, m & 2, m & 4).text); add(bwd_instance(m & 1, m & 2, m & 4).text); }
}

int dep_pack_cluster_lstm_split(const float* w_hh, float* wp, float* wpT, int H, hipStream_t s) {
    DEP_LAUNCH(pack_lstm_split_kernel, dim3(dep_cdiv(pack_fwd_split_pieces(4, H), 256)), dim3(256), 0, s, w_hh, (u32x4*)wp, (u32x4*)wpT, H);
    DEP_CHECK_LAUNCH();
    return DEP_OK;
}

bool dep_cluster_lstm_ok(int H, int, int) {      // any batch: the launchers chunk it
    return dep_rnn_switches().cluster_lstm && H == 128;                           // KCH, NTW above; NC = 4 (backward gathers exactly 4 partials)
}

// the larger of the two sweeps' payloads (the backward's from two members per direction on); the 256 bytes on top are slack
size_t dep_cluster_lstm_xbuf_bytes(int H, int B, int dirs) {
    const ChunkGeometry g = lstm_geometry(H, dirs, B);
    const size_t fwd = lstm_fwd_payload_bytes(g, H, dirs), bwd = lstm_bwd_payload_bytes(g, H);
    return PAYLOAD_OFF + (fwd > bwd ? fwd : bwd) + 256;
}

int dep_launch_cluster_lstm_fwd(const dep_sweep_args& a, void* xbuf, size_t xbuf_bytes) {
    DEP_CHECK_ARG(a.H == 128);
    const ChunkGeometry g = lstm_geometry(a.H, a.dirs, a.B);      // larger batches in chunks
    LF p{};
    p.B = a.B; p.T = a.T; p.H = a.H; p.dirs = a.dirs;
    for (int d = 0; d < a.dirs; ++d) p.wp[d] = (const f32x4*)a.wp[d];
    p.gi = a.gi; p.ldgi = a.dirs * 4 * a.H; p.y = a.y; p.ldy = a.ldy;
    p.ydrop = (a.drop_p > 0.f) ? a.ydrop : nullptr;
    p.drop_p = a.drop_p; p.drop_scale = a.drop_p > 0.f ? 1.0f / (1.0f - a.drop_p) : 1.0f; p.seed = a.seed; p.site = a.site;
    p.h_n = a.h_n;
    p.svg = a.training ? a.sv0 : nullptr; p.svc = a.sv1; p.lengths = a.lengths;
    const size_t pay = lstm_fwd_payload_bytes(g, a.H, a.dirs);
    DEP_CHECK_ARG(xbuf && PAYLOAD_OFF + pay <= xbuf_bytes && g.resident());
    p.flags = bind_exchange(p, xbuf, a.hdr_slot, pay);
    DepProfScope prof(DEP_PROF_LSTM_FWD, a.stream);
    return launch_chunks(fwd_instance(a.split, a.sv16 && a.training, a.lengths != nullptr), g, dim3(CT + L_SVC), p, a.stream, __PRETTY_FUNCTION__,
                         [&](int b0) { return hdr_prepare(xbuf, a.hdr_slot, a.hdr_clean && b0 == 0, a.stream); });
}

// the 16-bit saved gates (dep_sweep_args.sv16): both sweeps, split-precision mode
// OPT-IN (DEP_LSTM_SV16=1): measured at cfg3 it buys 1.5 % on each sweep (1.18 -> 1.16, 1.35 -> 1.33 ms; the BiLSTM sweeps are less
// byte-bound than the GRU backward), and it moves the text model's parameters after two AdamW steps by up to 8.6e-5 from the reference
// fixture -- inside the path's 1e-4 bar but outside tests/test_scripts_gpu.py's tighter 7.1e-5 -- so the default keeps fp32 gates.
bool dep_cluster_lstm_sv16_ok() { return dep_rnn_switches().lstm_sv16; }

bool dep_cluster_lstm_bwd_pk_ok(int T) { return T % 2 == 0; }

int dep_launch_cluster_lstm_bwd(const dep_sweep_bwd_args& a, void* xbuf, size_t xbuf_bytes) {
    DEP_CHECK_ARG(a.H == 128);
    const ChunkGeometry g = lstm_geometry(a.H, a.dirs, a.B);
    const int nbt = dep_cdiv(a.B, BT);
    LB p{};
    p.B = a.B; p.T = a.T; p.H = a.H; p.dirs = a.dirs;
    for (int d = 0; d < a.dirs; ++d) p.wp[d] = (const f32x4*)a.wpT[d];
    p.dy = a.dy; p.lddy = a.lddy;
    p.drop_p = a.dy ? a.drop_p : 0.f; p.drop_scale = a.drop_p > 0.f ? 1.0f / (1.0f - a.drop_p) : 1.0f;
    p.seed = a.seed; p.site = a.site;
    p.dh_n = a.dh_n; p.svg = a.sv0; p.svc = a.sv1;
    p.dgi = a.dgi; p.lddg = a.dirs * 4 * a.H; p.dbpart = a.dbpart; p.nwg = nbt; p.dgpk = a.dg_pk; p.lengths = a.lengths;
    DEP_CHECK_ARG(a.dbpart_rows >= nbt * a.dirs);
    const size_t pay = lstm_bwd_payload_bytes(g, a.H);
    DEP_CHECK_ARG(xbuf && PAYLOAD_OFF + pay <= xbuf_bytes && g.resident());
    p.flags = bind_exchange(p, xbuf, a.hdr_slot, pay);
    DepProfScope prof(DEP_PROF_LSTM_BWD, a.stream);
    DEP_CHECK_ARG(!a.dg_pk || a.T % 2 == 0);         // the PK image comes out of the service waves' flush in whole step pairs (dep_cluster_lstm_bwd_pk_ok)
    DEP_CHECK_ARG(!a.sv16 || a.split);               // 16-bit saved gates: split-precision mode
    return launch_chunks(bwd_instance(a.split, a.sv16, a.lengths != nullptr), g, dim3(CT + L_SVC), p, a.stream, __PRETTY_FUNCTION__,
                         [&](int b0) { return hdr_prepare(xbuf, a.hdr_slot, a.hdr_clean && b0 == 0, a.stream); });
}
