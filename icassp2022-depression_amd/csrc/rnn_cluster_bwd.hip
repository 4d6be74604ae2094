// Cluster-parallel GRU BPTT sweep, flag-published exchange (cdna_hip_programming.md G16 recipe R1).
//
// Same decomposition as rnn_cluster.hip (member c of a 16-utterance tile's cluster keeps the W_hh rows of
// hidden units [32c, 32c+32) in VGPRs and turns ITS 16x96 slice of dgh_t into a partial dh_{t-1} for all H
// columns), but the reduce-scatter of the partials moves 4096 values per member per step, too many for
// 8-byte tagged granules (each narrow write-through store is its own fabric write).  Here the partials are
// plain fp32 written in MFMA-fragment order with wave-contiguous 16-byte sc1 (write-through) stores, every
// wave drains (s_waitcnt vmcnt(0)), the workgroup barriers, and one lane publishes the step's epoch in the
// member's flag word; consumers poll the NC flags with relaxed agent-scope loads (>= epoch: flags only grow)
// and then read their two columns of every member's partial with sc1 loads, summing in member order
// (deterministic).  Payload buffers alternate by step parity; only the status/flag words are zeroed per launch.
#include "rnn_cluster_launch.h"

namespace {
using namespace depc;

constexpr size_t EXCLUSIVE_LDS = 84 * 1024;
#define DEP_STAMP(slot) do { if (tr && t >= 100 && t < 104) tr[(t - 100) * 8 + (slot)] = (long long)__builtin_readcyclecounter(); } while (0)

struct P2 {
    int B, T, H, nbtp, b0;      // b0: first utterance of this launch's batch chunk (B is the whole batch)
    const f32x4* wp;
    const float* y; int ldy;
    const float* dy; int lddy;
    float drop_p, drop_scale; uint64_t seed; uint32_t site;
    const float* dpooled; float pool_scale;
    const float* dh_n;
    const float* sv0; const float* sv1; const float* sv2; const float* sv3;
    float* dgi; int lddg;
    float* dghn; int lddghn;
    float* dbpart;
    unsigned* status; unsigned* flags; unsigned* hello; float* payload; unsigned payload_bytes;
    int nofast;              // DEP_CLUSTER_NOFAST=1: always use the write-through (placement-agnostic) stores
    long long* trace;        // debug: s_memtime stamps of workgroup 0 (DEP_TRACE=1), else nullptr
    int trall_off;           // debug: LDS offset (32-bit words) of the per-step stamp array
    int dgpk;                // round 4: write the gate gradients as the PK image the bf16x3 GEMMs read without converting (gemm_bf16x3.hip FMT_PK): rows (t even, t+1) of an utterance hold the (hi, lo) bf16 pairs of both steps; burst kernel, 4H-wide layout, T even
    const int* lengths; int pool_mean;      // ragged instances (RAG): row b is live for t < lengths[b]; dpooled of a mean is scaled by 1 / lengths[b]
    // state (dep_rnn_backward_state[_varlen] on impl 5; run-time pointers like F2::hx, no instance of their own): hx is h_prev of step 0
    // instead of zeros -- a global input every thread reads at its own units, on a branch only the t = 0 request takes; dhx receives the
    // direct term of the gradient entering step 0, d_0 * z_0 (a ragged row that never was live: the dh_n it loaded), stored at t == 0 by
    // the thread that owns the two columns.  The recurrent term dG[:, 0, :] W_hh is added by the host behind the sweep.  dhx may be
    // dh_n's buffer: the same thread read that address in front of the loop.  Neither touches the exchange, a flag or a trip count.
    const float* hx; float* dhx;
};
// The parameters of the bidirectional instances (BI, impl 7), as F2B is the forward's: direction 1's backward weight image, the row stride
// of the saved gates (2H) and the bias-partial rows per direction (ceil(B / 16): direction d's rows follow direction d-1's).  A struct of
// their own, so that the unidirectional instances keep their kernel arguments and with them their ISA.
struct P2B : P2 { const f32x4* wp1; int ldsv; int nbt; };

struct StepIn { float2 r, z, n, hn, hp, dy; };

// Thread -> element map (matches the fragment order of the published partials, so the gather is coalesced):
//   jl = tid>>7 (which of the member's two 16-column tiles), lp = (tid>>1)&63 (MFMA lane id: row lp&15, quad lp>>4),
//   half = tid&1 -> columns (2c+jl)*16 + (lp>>4)*4 + 2*half + {0,1} of utterance row lp&15.
//
// SPLIT: dgates W_hh runs on the bf16 matrix cores with the 3-term split (see gru_fwd_cluster16): the member's 96 gate
// rows are exactly three 32-wide k-steps (r, z, n), 4 tiles x 3 k-steps x 3 products = 36 v_mfma_f32_16x16x32_bf16
// (576 cycles) replace 96 v_mfma_f32_16x16x4_f32 (3072 cycles, close to half of the step).  The thread that produces a
// gate gradient splits it once and writes the (hi, lo) bf16 planes the MFMA B fragments are read from.
//
// KB > 0: BURST STREAMS.  A CU returns vector loads in issue order ACROSS its waves (tools/micro/inorder.hip: a load that hits
// in L2 comes back after 200 cycles on a quiet CU, after 600-4000 when another wave of the CU has HBM loads or stores in
// flight), so every HBM stream request of a step sits in front of that step's flag polls and gather loads, whichever wave
// issues it: the sweep pays HBM time and exchange latency one after the other.  With KB > 0 four service waves (threads
// CT .. CT+255) own every stream and move KB steps at a time: on a tile's `dirty' step (every KB-th, the tiles of an XCD
// staggered) they request the inputs of KB steps (registers for KB-1 steps, then the LDS ring `ibuf') and write out the
// gate gradients of the last KB steps (LDS ring `obuf'); the other KB-1 steps of the tile run with nothing but the
// exchange in the CU's memory pipeline.  The compute waves read their inputs from ibuf and leave dr, dz, dn, dn*r in obuf.
constexpr int SVC_THREADS = 256;
constexpr int SROW = 36;                             // LDS row stride (floats) of ibuf / obuf: 16-byte aligned rows, conflict-free columns
constexpr int SARR = 16 * SROW;
constexpr int TRACE_F = 2048, IBUF_F = 2304;         // float offsets into the workgroup's LDS (planes: [0, 2048))
constexpr int obuf_slots(int KB) { return KB == 4 ? KB + 2 : KB + 1; }      // KB + 1 does for fp32 rows; the PK flush (KB = 4 only) works on step PAIRS and may lag one step
constexpr size_t burst_lds_bytes(int KB) { return (size_t)(IBUF_F + KB * 6 * SARR + obuf_slots(KB) * 4 * SARR) * sizeof(float); }
// AG (round 5): the all-gather form of the exchange.  Member c keeps the W_hh COLUMNS of its 32 hidden units (all 3H rows), every member
// publishes its own 16 x 96 gate gradients dgh_t = (dr, dz, dn*r) ONCE, as the (hi, lo) bf16 planes the MFMAs read, in MFMA B-fragment order
// (6 KB per member and step instead of 16 KB of fp32 partial dh; no sum over members at the consumer), and computes its own 32 columns of
// dh_{t-1} = dgh_t W_hh completely: K = 3H = 768 split into four quarters over the four compute waves (wave w = the 192 k of source members
// 2w, 2w+1: 6 k-steps x 2 output tiles x 3 products = the same 36 MFMAs per wave), the B fragments read STRAIGHT from the exchange buffer
// into registers (12 wave-contiguous 1 KB loads per wave; no LDS staging), the four K-quarter partials summed through a double-buffered
// LDS block `red' behind the step's only workgroup barrier.  LDS: red occupies [0, 4096) floats, so the trace / ring offsets move up.
constexpr int AG_TRACE_F = 4096, AG_IBUF_F = 4352, AG_MEMBER_BYTES = 6 * 1024;
constexpr size_t burst_lds_bytes_ag(int KB) { return (size_t)(AG_IBUF_F + KB * 6 * SARR + obuf_slots(KB) * 4 * SARR) * sizeof(float); }

// SV16: the saved gates r, z, n are 16-bit fixed point (rnn_cluster_common.h).  A template parameter, not a kernel argument: as a
// run-time switch the two load widths met in copies of the loaded registers and the service waves waited for every load they had
// just issued (both settings 5-20 % slower than the kernel without the switch, profiles/r04_ab_pairs.txt).
// BF (bf16-storage mode, dep_set_gemm_mode(3); implies SV16, burst kernel only): hn and the hidden sequence y are bf16 arrays (2-byte
// elements at the same positions), and the gate gradients go out as the PKH image (only the hi rows of the PK image).
// RAG: the ragged-batch instances (dep_rnn_backward_varlen).  The row is owned by a lane, so the predicate live = t < lengths[b] is a
// handful of selects in the gate phase: a dead step's gate gradients are 0 (what the members exchange, the write-out and the bias sums
// see) and its incoming dh passes through to step t-1 unchanged.  Trip counts, epochs, flags, the service waves and the burst write-out
// are those of the dense instances: every workgroup runs all T steps.
// BI: the bidirectional instances (impl 7), the geometry of gru_fwd_cluster_r1<.., BI = true>.  A cluster is a (direction, tile) PAIR, both
// directions of a batch chunk in one launch: block = (c * 2 + dir) * nbtp + bt, and the pair dir * nbtp + bt indexes the flag words, the
// hello words, the payload and the all-gather blocks.  The loop counter t counts the sweep DOWN in both directions (sweep step k = T-1-t:
// epochs, payload parity, ring slots, the dirty-step phase and the last-step test t == 0 follow it); the TIME of the step is tm = t for
// direction 0 and T-1-t for direction 1, whose h_prev is y[b, tm+1] (the last sweep step: its hx slice, or zeros; a ragged row's first
// live step tm = len-1 likewise: the position behind it holds 0, not the state the forward carried through the dead steps).  Every array
// is the tile BiGRU's: y, dy, the fp32 saved gates (ldsv) and the dropout index over (B,T,2H) with the direction in columns, dpooled
// (B,2H), dh_n / hx / dhx (2,B,H), dgi (B T, 6H) and dghn (B T, 2H) as gru_bwd_mfma<.., true> writes them, bias partials [dir][tile].  A
// ragged row's direction-1 dead steps come LAST: their gate gradients are 0 and dh passes through, so what is stored as dhx then already
// holds the recurrent term.  Trip counts, epochs, flags and barriers do not know the direction.  BI = false is the unidirectional text.
template <int NTW, bool SPLIT, int KB, bool SV16 = false, bool BF = false, bool AG = false, bool RAG = false, bool BI = false>      // output tiles per wave = H/64
__global__ __launch_bounds__(KB ? CT + SVC_THREADS : CT) void gru_bwd_cluster_r1(std::conditional_t<BI, P2B, P2> p) {
    static_assert(!BF || (SV16 && KB > 0), "bf16 storage: 16-bit gates, burst kernel");
    static_assert(!BI || (!SV16 && !BF), "bidirectional: fp32 saved gates and storage");
    static_assert(!AG || (SPLIT && KB == 4 && NTW == 4), "all-gather exchange: H = 256, split products, burst length 4");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int KS = 96, KCB = KS / 16, LDG = KS + LPAD;
    constexpr int LDGB = KS + 8;                      // bf16 elements per row of a split plane (208-byte rows)
    const int H = p.H, T = p.T, NC = H / 32, NTT = H / 16;
    const int c = BI ? blockIdx.x / (2 * p.nbtp) : blockIdx.x / p.nbtp, bt = blockIdx.x % p.nbtp;
    const int dir = BI ? (int)(blockIdx.x / p.nbtp) & 1 : 0;
    const int pt = BI ? dir * p.nbtp + bt : bt;      // the cluster's (direction, tile) pair: flags, hello words, payload
    if (p.b0 + bt * BT >= p.B) return;
    if (ld_agent(p.status) != 0) return;           // an earlier sweep of this step gave up: the status word is sticky until the next dep_rnn_forward
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int jl = tid >> 7, lp = (tid >> 1) & 63, half = tid & 1;
    const int j = lp & 15, ul = jl * 16 + (lp >> 4) * 4 + 2 * half;      // unit inside the member's 32
    const int col = 32 * c + ul;
    const int dcol = BI ? dir * H + col : col;      // the column in the direction-interleaved rows of y, dy, the saved gates and dpooled
    const int b = p.b0 + bt * BT + j;
    const bool valid = b < p.B;
    // this thread's pair in the (dirs,B,H) state arrays dh_n, hx, dhx (formed where it is used, as the unidirectional text forms it)
    const auto sat = [&](auto* q) { if constexpr (BI) return q + ((size_t)dir * p.B + b) * H + col; else return q + (size_t)b * H + col; };
    int ldsv = H;                                    // row stride of the saved gates
    if constexpr (BI) ldsv = p.ldsv;
    float* dgs = smem;                                                     // [16][LDG] fp32, or (SPLIT) two bf16 planes [16][LDGB]
    unsigned short* dg_hi = reinterpret_cast<unsigned short*>(smem);
    unsigned short* dg_lo = dg_hi + BT * LDGB;

    constexpr bool BURST = KB > 0;
    constexpr int KBX = BURST ? KB : 1;
    const bool svc = BURST && tid >= CT;              // wave-uniform
    float* ibuf = smem + (AG ? AG_IBUF_F : IBUF_F);   // [KB][6][16][SROW]: r, z, n, hn, h_{t-1}, dy of step k in slot k % KB
    constexpr int OSL = obuf_slots(KBX);
    float* obuf = ibuf + KBX * 6 * SARR;              // [OSL][4][16][SROW]: dr, dz, dn, dn*r of step k in slot k % OSL
    f32x4 wr[SPLIT ? 1 : NTW][SPLIT ? 1 : KCB];
    u32x4 wq[SPLIT ? NTW : 1][SPLIT ? 3 : 1][2];       // [tile][k-step = gate][hi, lo]   (AG: unused, wa below)
    u32x4 wa[AG ? 2 : 1][AG ? 6 : 1][2];               // AG: [own output tile][k-step = (source member 2w + ks/3, gate ks%3)][hi, lo]
    if (!svc) {
        // the direction's own backward image
        const auto wsel = [&]() -> const f32x4* { if constexpr (BI) return dir ? p.wp1 : p.wp; else return p.wp; };
        if constexpr (AG) {
            // the SAME packed image as the reduce-scatter kernel's ([K member][output tile][gate][plane][lane]); this member takes the
            // two output tiles of its own 32 columns and, per wave, the K rows of source members 2w, 2w+1
            const u32x4* wpq = reinterpret_cast<const u32x4*>(wsel());
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int ks = 0; ks < 6; ++ks)
#pragma unroll
                    for (int pl = 0; pl < 2; ++pl)
                        wa[i][ks][pl] = wpq[(size_t)((((2 * w + ks / 3) * NTT + 2 * c + i) * 3 + ks % 3) * 2 + pl) * 64 + lane];
        } else if constexpr (SPLIT) {
            const u32x4* wpq = reinterpret_cast<const u32x4*>(wsel());
#pragma unroll
            for (int i = 0; i < NTW; ++i)
#pragma unroll
                for (int ks = 0; ks < 3; ++ks)
#pragma unroll
                    for (int pl = 0; pl < 2; ++pl)
                        wq[i][ks][pl] = wpq[(size_t)(((c * NTT + w * NTW + i) * 3 + ks) * 2 + pl) * 64 + lane];
        } else {
#pragma unroll
            for (int i = 0; i < NTW; ++i)
#pragma unroll
                for (int k = 0; k < KCB; ++k)
                    if constexpr (BI) wr[i][k] = wsel()[(size_t)((c * NTT + w * NTW + i) * KCB + k) * 64 + lane];
                    else wr[i][k] = p.wp[(size_t)((c * NTT + w * NTW + i) * KCB + k) * 64 + lane];
        }
    }
    float2 dhrec = (p.dh_n && valid && !svc) ? ld2(sat(p.dh_n)) : f2(0.f, 0.f);
    float2 dpl = f2(0.f, 0.f);
    int len = T;
    if constexpr (RAG) len = (valid && !svc) ? dep_row_len(p.lengths, b, T) : 0;
    const float dps = RAG ? dep_ragged_pool_scale(p.pool_mean, len, T, p.pool_scale) : p.pool_scale;
    if (p.dpooled && valid && !svc) {
        if constexpr (BI) dpl = ld2(p.dpooled + (size_t)b * 2 * H + dcol);      // (B,2H)
        else dpl = ld2(p.dpooled + (size_t)b * H + col);
        dpl.x *= dps; dpl.y *= dps;
    }
    float2 dbr = f2(0.f, 0.f), dbz = dbr, dbn = dbr, dbh = dbr;
    const size_t pstride = (size_t)(BI ? 2 * p.nbtp : p.nbtp) * NC * BT * H;      // floats per parity buffer
    const size_t tile_base = (size_t)pt * NC * BT * H;                     // this tile's [NC][NTT][64][4] block
    __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)p.payload, 0, p.payload_bytes, 0x00020000);
    // per-wave flags: every compute wave raises its OWN epoch flag once its own payload stores are acknowledged (no workgroup barrier
    // in front of the flag); the pollers watch all 4 NC words of the tile
    unsigned* tflags = p.flags + pt * NC * 4;
    unsigned* myflag = tflags + c * 4 + (w & 3);
    const int nflags = NC * 4;
    const int ml = lane & 15, mq = lane >> 4;
    const int sx = p.nofast ? 0 : cluster_same_xcd(p.hello + pt * NC, NC, c, p.status);
    if (sx < 0) return;
    const bool fast = sx == 1;

    auto load_step = [&](int t, StepIn& s) {
        s.r = s.z = s.n = s.hn = s.hp = s.dy = f2(0.f, 0.f);
        if (valid && t >= 0) {
            const size_t row = (size_t)b * T + t;
            const size_t so = BI ? row * ldsv + dcol : row * H + col;
            if constexpr (SV16) {
                s.r = unpack_unorm2(*reinterpret_cast<const unsigned*>(reinterpret_cast<const unsigned short*>(p.sv0) + so));
                s.z = unpack_unorm2(*reinterpret_cast<const unsigned*>(reinterpret_cast<const unsigned short*>(p.sv1) + so));
                s.n = unpack_snorm2(*reinterpret_cast<const unsigned*>(reinterpret_cast<const unsigned short*>(p.sv2) + so));
            } else { s.r = ld2(p.sv0 + so); s.z = ld2(p.sv1 + so); s.n = ld2(p.sv2 + so); }
            s.hn = ld2(p.sv3 + so);
            if constexpr (BI) {       // (the sweep's last step, and a ragged row's first live step in direction 1: the state, not a neighbour)
                const bool inner = dir ? (t < T - 1 && !(RAG && t == len - 1)) : t > 0;
                if (inner) s.hp = ld2(p.y + (dir ? row + 1 : row - 1) * p.ldy + dcol);
                else if (p.hx) s.hp = ld2(sat(p.hx));
            } else {
                if (t > 0) s.hp = ld2(p.y + (row - 1) * p.ldy + col);
                else if (p.hx) s.hp = ld2(p.hx + (size_t)b * H + col);
            }
            if (p.dy) s.dy = ld2(p.dy + row * p.lddy + dcol);
        }
    };
    // dhx at t == 0: the direct term d * z of this thread's two columns (a ragged row that never was live: the dh_n it loaded).  The
    // product is formed HERE, from a copy of z the optimiser cannot see through: shared with the step loop's dzt it would give that
    // product a second use, and the loop's fused d * z + s (one v_pk_fma_f32 per step) would become a multiply and an add -- other bits
    // in every call, with or without state.  A toolchain change: re-run tools/isa_diff.py (profiles/state_cluster_bwd_isa.txt counts the fma).
    auto store_dhx = [&](float2 d, float2 z) {
        asm volatile("" : "+v"(z.x), "+v"(z.y));
        const float2 v = f2(d.x * z.x, d.y * z.y);
        st2(sat(p.dhx), RAG ? dep_sel2(((BI && dir) ? T - 1 : 0) < len, v, dhrec) : v);
    };
    StepIn cur, nxt;
    if constexpr (!BURST) load_step((BI && dir) ? 0 : T - 1, cur);
    // ---- service waves.  Step counter k = T-1-t.  Service thread st: piece idx = st + 256 i (i < 3) of a step's 768 input
    // pieces -> array idx / 128, utterance row (idx % 128) / 8, 16-byte piece idx % 8; likewise 512 write-out pieces (i < 2).
    const int st = tid - CT, sarr0 = (st >> 7) & 1, sr = (st >> 3) & 15, sp = st & 7;
    const int sb = p.b0 + bt * BT + sr;
    const bool svalid = sb < p.B;
    const int scol = 32 * c + sp * 4;
    const int sdcol = BI ? dir * H + scol : scol;     // ... in the direction-interleaved rows
    int slen = T;                                     // BI, ragged: the service thread's own row (h_prev of its first live step in direction 1)
    if constexpr (BI && RAG) slen = (svc && svalid) ? dep_row_len(p.lengths, sb, T) : 0;
    const int phi = (bt >> 3) % KBX;                  // the tiles of an XCD (bt = xcd mod 8) take their dirty steps in turn
    f32x4 sreg[KBX][3];
    // wave-uniform array choice (waves 4, 5: arrays 0, 2, 4 = r, n, h_{t-1}; waves 6, 7: 1, 3, 5 = z, hn, dy), made scalar so
    // that the base pointers are selected in SGPRs (a per-lane choice makes hipcc index the kernel arguments in memory and
    // wait for that pointer load -- vmcnt(0) -- in front of every data load)
    const bool sodd = __builtin_amdgcn_readfirstlane(sarr0) != 0;
    // SV16: the wave pair 4, 5 (sodd = 0) streams the three fp32 arrays hn, h_{t-1}, dy (ring arrays 3, 4, 5), the pair 6, 7 the three
    // 16-bit arrays r, z, n (ring arrays 0, 1, 2; 8-byte pieces, decoded when they go into the ring): one load width per wave
    const float* sbase0 = SV16 ? (sodd ? p.sv0 : p.sv3) : (sodd ? p.sv1 : p.sv0);
    const float* sbase1 = SV16 ? (sodd ? p.sv1 : p.y) : (sodd ? p.sv3 : p.sv2);
    const float* sbase2 = SV16 ? (sodd ? p.sv2 : p.dy) : (sodd ? p.dy : p.y);
    const int sld2 = sodd ? p.lddy : p.ldy;
    // The service waves' one-touch streams carry the non-temporal hint, so that they do not displace the exchange payload
    // (rewritten every other step) from this XCD's L2 and turn it into HBM write-backs.  The gate-gradient write-out goes out as
    // buffer stores with the nt bit (tools/micro/l2wb.hip + PMC: one-touch stores that allocate in L2 are what evicts the payload
    // -- 1 MB per XCD, rewritten in place every other step -- before its next rewrite: 0.8 GB of write-backs per launch; with nt
    // stores the payload stays.  __builtin_nontemporal_store compiles to PLAIN stores here -- no nt bit in the ISA.)
    // (resources are TILE-relative -- base = the tile's first row, extent = its 16 utterances -- so 32-bit offsets always suffice)
    const size_t trow0 = (size_t)(p.b0 + bt * BT) * T;
    float* const dgi_t = p.dgi + trow0 * p.lddg; float* const dghn_t = p.dghn + trow0 * p.lddghn;
    __amdgpu_buffer_rsrc_t rs_dgi = __builtin_amdgcn_make_buffer_rsrc((void*)dgi_t, 0, (unsigned)((size_t)BT * T * p.lddg * 4), 0x00020000);
    __amdgpu_buffer_rsrc_t rs_dghn = __builtin_amdgcn_make_buffer_rsrc((void*)dghn_t, 0, (unsigned)((size_t)BT * T * p.lddghn * 4), 0x00020000);
    // q inside the tile's rows of the array of `rs` (tile base `base`): 16-byte nt store
    auto stnt2 = [&](__amdgpu_buffer_rsrc_t rs, const float* base, float* q, f32x4 v) {
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rs, (unsigned)((const char*)q - (const char*)base), 0, 2 /* nt */);
    };
    // ... and so do the service waves' one-touch READS (the saved gates, h_{t-1}, dy).
    const int mld0 = H > p.ldy ? (H > p.lddy ? H : p.lddy) : (p.ldy > p.lddy ? p.ldy : p.lddy);
    const int mld = BI ? (mld0 > ldsv ? mld0 : ldsv) : mld0;
    const unsigned span = (unsigned)((size_t)(BT * T + 1) * mld * 4);        // bounds the tile's rows of every input array (+ the h_{t-1} row in front)
    // bases one row in front of the tile's first row (h_{t-1} of t = 0 is never read; the offset stays non-negative)
    // (the 16-bit arrays of the SV16 wave pair have 2-byte elements: their rows are H / 2 floats apart)
    const bool w16 = SV16 && sodd;
    // byte offset of the tile's first row in each of this wave's three input arrays (element size x row stride)
    const size_t es0 = (w16 || BF) ? 2 : 4, es1 = (w16 || BF) ? 2 : 4, es2 = w16 ? 2 : 4;
    const size_t rs0 = BI ? (size_t)ldsv : (size_t)H;
    const size_t rs1 = SV16 ? (sodd ? (size_t)H : (size_t)p.ldy) : rs0, rs2 = SV16 ? (sodd ? (size_t)H : (size_t)p.lddy) : (size_t)sld2;
    const float* const in0_t = sbase0 ? reinterpret_cast<const float*>(reinterpret_cast<const char*>(sbase0) + trow0 * rs0 * es0) : nullptr;
    const float* const in1_t = sbase1 ? reinterpret_cast<const float*>(reinterpret_cast<const char*>(sbase1) + trow0 * rs1 * es1) : nullptr;
    const float* const in2_t = sbase2 ? reinterpret_cast<const float*>(reinterpret_cast<const char*>(sbase2) + trow0 * rs2 * es2) : nullptr;
    __amdgpu_buffer_rsrc_t rs_in0 = __builtin_amdgcn_make_buffer_rsrc((void*)in0_t, 0, span, 0x00020000);
    __amdgpu_buffer_rsrc_t rs_in1 = __builtin_amdgcn_make_buffer_rsrc((void*)in1_t, 0, span, 0x00020000);
    __amdgpu_buffer_rsrc_t rs_in2 = __builtin_amdgcn_make_buffer_rsrc((void*)in2_t, 0, span, 0x00020000);
    auto ldnt = [&](int which, const float* q) -> f32x4 {      // 16 bytes at q, inside input array `which` of this wave
        const float* base = which == 0 ? in0_t : (which == 1 ? in1_t : in2_t);
        const unsigned off = (unsigned)((const char*)q - (const char*)base);
        const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(which == 0 ? rs_in0 : (which == 1 ? rs_in1 : rs_in2), off, 0, 2 /* nt */);
        return __builtin_bit_cast(f32x4, v);
    };
    auto ldnt8 = [&](int which, const unsigned short* q) -> float2 {
        typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
        const float* base = which == 0 ? in0_t : (which == 1 ? in1_t : in2_t);
        const unsigned off = (unsigned)((const char*)q - (const char*)base);
        const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(which == 0 ? rs_in0 : (which == 1 ? rs_in1 : rs_in2), off, 0, 2 /* nt */);
        return make_float2(__uint_as_float(v[0]), __uint_as_float(v[1]));
    };
    // h_prev of step 0 for the service waves' piece: the caller's hx (plain 16-byte load, outside the tile-relative resources), or zeros
    auto svc_hx = [&]() -> f32x4 { return p.hx ? *reinterpret_cast<const f32x4*>(p.hx + (BI ? (size_t)dir * p.B + sb : (size_t)sb) * H + scol) : zero4(); };
    // W16 (a std::bool_constant): this wave streams the 16-bit arrays
    auto svc_load1 = [&](auto W16, int k, int i) -> f32x4 {     // input i of this wave for step k
        if constexpr (BI) {                                   // fp32 arrays only; k counts the sweep, t is the step's time
            if (!svalid || k >= T) return zero4();
            const int t = dir ? k : T - 1 - k;
            const size_t row = (size_t)sb * T + t;
            if (i == 0) return ldnt(0, sbase0 + row * ldsv + sdcol);
            if (i == 1) return ldnt(1, sbase1 + row * ldsv + sdcol);
            if (sodd) return sbase2 ? ldnt(2, sbase2 + row * sld2 + sdcol) : zero4();
            const bool inner = k < T - 1 && !(RAG && dir && t == slen - 1);
            return inner ? ldnt(2, sbase2 + (dir ? row + 1 : row - 1) * sld2 + sdcol) : svc_hx();
        }
        const int t = T - 1 - k;
        if (!svalid || t < 0) return zero4();
        const size_t row = (size_t)sb * T + t;
        if constexpr (SV16) {
            if constexpr (decltype(W16)::value) {             // four 16-bit values = 8 bytes
                const float* base = i == 0 ? sbase0 : (i == 1 ? sbase1 : sbase2);
                const float2 w = ldnt8(i, reinterpret_cast<const unsigned short*>(base) + row * H + scol);
                const f32x4 r4 = {w.x, w.y, 0.f, 0.f};
                return r4;
            } else {
                if constexpr (BF) {                           // hn, h_{t-1}: bf16 arrays, four values = 8 bytes (decoded in svc_put)
                    if (i == 0) { const float2 w = ldnt8(0, reinterpret_cast<const unsigned short*>(sbase0) + row * H + scol); const f32x4 r4 = {w.x, w.y, 0.f, 0.f}; return r4; }
                    if (i == 1) {
                        if (t <= 0) return zero4();
                        const float2 w = ldnt8(1, reinterpret_cast<const unsigned short*>(sbase1) + (row - 1) * p.ldy + scol);
                        const f32x4 r4 = {w.x, w.y, 0.f, 0.f}; return r4;
                    }
                    return sbase2 ? ldnt(2, sbase2 + row * p.lddy + scol) : zero4();
                } else {
                    if (i == 0) return ldnt(0, sbase0 + row * H + scol);
                    if (i == 1) return t > 0 ? ldnt(1, sbase1 + (row - 1) * p.ldy + scol) : svc_hx();
                    return sbase2 ? ldnt(2, sbase2 + row * p.lddy + scol) : zero4();
                }
            }
        } else {
            if (i == 0) return ldnt(0, sbase0 + row * H + scol);
            if (i == 1) return ldnt(1, sbase1 + row * H + scol);
            if (sodd) return sbase2 ? ldnt(2, sbase2 + row * sld2 + scol) : zero4();
            return t > 0 ? ldnt(2, sbase2 + (row - 1) * sld2 + scol) : svc_hx();
        }
    };
    auto svc_issue = [&](auto W16, int k0, int n) {   // inputs of steps k0 .. k0+n-1 -> registers
#pragma unroll
        for (int d = 0; d < KBX; ++d)
            if (d < n) {
#pragma unroll
                for (int i = 0; i < 3; ++i) sreg[d][i] = svc_load1(W16, k0 + d, i);
            }
    };
    auto svc_put = [&](auto W16, int k0, int n, int dlo = 0) {     // registers -> ibuf slots of steps k0+dlo .. k0+n-1
#pragma unroll
        for (int d = 0; d < KBX; ++d)
            if (d >= dlo && d < n) {
                float* dst = ibuf + ((k0 + d) % KBX) * 6 * SARR + sr * SROW + sp * 4;
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    if constexpr (SV16) {
                        if constexpr (decltype(W16)::value) {
                            const unsigned w0 = __float_as_uint(sreg[d][i][0]), w1 = __float_as_uint(sreg[d][i][1]);
                            const float2 a = i < 2 ? unpack_unorm2(w0) : unpack_snorm2(w0), b = i < 2 ? unpack_unorm2(w1) : unpack_snorm2(w1);
                            const f32x4 v = {a.x, a.y, b.x, b.y};
                            *reinterpret_cast<f32x4*>(dst + i * SARR) = v;
                        } else if (BF && i < 2) {               // bf16 pairs -> fp32 (the value sits in the upper half)
                            const unsigned w0 = __float_as_uint(sreg[d][i][0]), w1 = __float_as_uint(sreg[d][i][1]);
                            const f32x4 v = {__uint_as_float(w0 << 16), __uint_as_float(w0 & 0xffff0000u), __uint_as_float(w1 << 16), __uint_as_float(w1 & 0xffff0000u)};
                            *reinterpret_cast<f32x4*>(dst + (3 + i) * SARR) = v;
                        } else {
                            *reinterpret_cast<f32x4*>(dst + (3 + i) * SARR) = sreg[d][i];
                        }
                    } else {
                        *reinterpret_cast<f32x4*>(dst + (sarr0 + 2 * i) * SARR) = sreg[d][i];
                    }
                }
            }
    };
    auto svc_flush = [&](int k0, int k1) {            // gate gradients of steps k0 .. k1-1: obuf -> dgi (dr, dz, dn), dghn (dn * r)
        if (!svalid) return;
        for (int k = k0 < 0 ? 0 : k0; k < k1; ++k) {
            const size_t row = (size_t)sb * T + ((BI && dir) ? k : T - 1 - k);
            const float* o = obuf + (k % OSL) * 4 * SARR + sr * SROW + sp * 4;
            const int gcol = BI ? dir * 3 * H + scol : scol;      // the direction's three gate blocks of the (B T, 6H) rows
            // arrays sarr0 (dr / dz) and 2 + sarr0 (dn / dn*r)
            stnt2(rs_dgi, dgi_t, p.dgi + row * p.lddg + (sodd ? H : 0) + gcol, ld4(o + (sodd ? SARR : 0)));
            if (sodd) stnt2(rs_dghn, dghn_t, p.dghn + row * p.lddghn + sdcol, ld4(o + 3 * SARR));
            else stnt2(rs_dgi, dgi_t, p.dgi + row * p.lddg + 2 * H + gcol, ld4(o + 2 * SARR));
        }
    };
    // PK image (p.dgpk): steps (ka, ka+1), ka even, are rows t_even + 1, t_even (t_even = T-2-ka) of the utterance; physical row
    // t_even holds bf16hi(x[t_even]) | bf16hi(x[t_even+1]) << 16 per column, row t_even + 1 the residual (lo) pairs -- exactly the
    // (hi, lo) the GEMM's split4 would form (same v_cvt_pk_bf16_f32 roundings), so the contractions' bits do not change.
    auto svc_flush_pk = [&](int k0, int k1) {         // complete step pairs in [k0, k1): both even
        if (!svalid) return;
        for (int ka = k0 < 0 ? 0 : k0; ka + 1 < k1; ka += 2) {
            const size_t row = (size_t)sb * T + (T - 2 - ka);                    // the even row of the pair
            const float* oo = obuf + (ka % OSL) * 4 * SARR + sr * SROW + sp * 4;        // step ka   = row t_even + 1
            const float* oe = obuf + ((ka + 1) % OSL) * 4 * SARR + sr * SROW + sp * 4;  // step ka+1 = row t_even
#pragma unroll
            for (int q = 0; q < 2; ++q) {             // arrays sarr0 (dr / dz) and 2 + sarr0 (dn / dn*r)
                const int ao = (q ? 2 : 0) + (sodd ? 1 : 0);
                const f32x4 xe = ld4(oe + ao * SARR), xo = ld4(oo + ao * SARR);
                u32x4 h, l;
#pragma unroll
                for (int e = 0; e < 4; ++e) { unsigned hh, ll; split_pair(xe[e], xo[e], hh, ll); h[e] = hh; l[e] = ll; }
                float* g = p.dgi + row * p.lddg + ao * H + scol;                 // 4H-wide rows [dr | dz | dn | dn*r]
                stnt2(rs_dgi, dgi_t, g, __builtin_bit_cast(f32x4, h));
                if constexpr (!BF) stnt2(rs_dgi, dgi_t, g + p.lddg, __builtin_bit_cast(f32x4, l));      // (PKH: the hi rows only)
            }
        }
    };
    if constexpr (BURST) {
        // the service waves' whole life (W16: this wave pair streams the 16-bit arrays)
        auto svc_life = [&](auto W16) {
            // the service waves' whole life: same barrier sequence as the compute waves' loop below (one per step)
            svc_issue(W16, 0, KBX); svc_put(W16, 0, KBX);       // steps 0 .. KB-1 straight into the ring
            svc_issue(W16, KBX, phi);                      // steps KB .. KB+phi-1: written at step phi-1, before the first dirty step (k = phi)
            __syncthreads();
            for (int k = 0; k < T; ++k) {
                const int jj = (k + KBX - phi) % KBX;                  // jj == 0: this tile's dirty step
                const int last = k - jj;                               // the dirty step this burst started with (< 0: the prologue)
                const bool trs = p.trace && blockIdx.x == 0 && st == 0 && k >= 100 && k < 104;
                if (trs) p.trace[32 + (k - 100) * 4 + 0] = (long long)__builtin_readcyclecounter();
                if (jj == 0) {
                    // everything the next KB steps need from HBM, and everything the last KB produced.  (The service waves run
                    // ahead of the compute waves -- nothing holds them after barrier #2 -- so the burst starts during the
                    // previous step's poll; holding it back until the compute waves reach the dirty step's gate phase
                    // measured the same launch time: the burst occupies the CU's memory pipeline for ~1.3 steps either way.)
                    svc_issue(W16, k + KBX, KBX);
                    if (trs) p.trace[32 + (k - 100) * 4 + 1] = (long long)__builtin_readcyclecounter();
                    if (!BI && p.dgpk) svc_flush_pk(k - KBX - (phi & 1), k - (phi & 1));      // whole pairs: one step later for the tiles with an odd phase
                    else svc_flush(k - KBX, k);
                }
                if (trs) p.trace[32 + (k - 100) * 4 + 2] = (long long)__builtin_readcyclecounter();
                bar_lds();                           // #1
                if (trs) p.trace[32 + (k - 100) * 4 + 3] = (long long)__builtin_readcyclecounter();
                if constexpr (AG) {
                    // The all-gather step has ONE barrier, at its end, and the compute waves read ring slot (k+1) % KB right behind
                    // barrier(k): step s may be written only between barrier(s - KB) (its slot's previous occupant consumed) and
                    // barrier(s - 1).  For the burst requested at dirty step L = last (steps L+KB .. L+2KB-1) that is: the first
                    // KB-1 behind barrier(L + KB - 2), the last one behind barrier(L + KB - 1).  No race window at all.
                    if (jj == KBX - 2 && last >= 0) svc_put(W16, last + KBX, KBX - 1);
                    if (jj == KBX - 1) {
                        if (last >= 0) svc_put(W16, last + KBX, KBX, KBX - 1);
                        else svc_put(W16, KBX, phi);         // the prologue's steps KB .. KB+phi-1 (their slots were consumed by barrier(phi-1))
                    }
                    if (k == T - 1) break;
                    continue;
                }
                if (jj == KBX - 1) {
                    // last step of the burst: the ring slots of steps last .. k are consumed; the registers (requested at step
                    // `last', KB-1 steps ago) become steps last+KB .. k+KB
                    if (last >= 0) svc_put(W16, last + KBX, KBX);
                    else svc_put(W16, KBX, phi);
                }
                if (k == T - 1) break;                // (per-wave flags: the compute waves have no drain barrier)
            }
            const int jl2 = (T - 1 + KBX - phi) % KBX;
            if (!BI && p.dgpk) svc_flush_pk(T - 1 - jl2 - (phi & 1), T);      // T is even: the last pair is complete
            else svc_flush(T - 1 - jl2, T);           // the gate gradients since the last dirty step
        };
        if (svc) {
            if constexpr (SV16) {
                if (sodd) svc_life(std::true_type{}); else svc_life(std::false_type{});
            } else {
                svc_life(std::false_type{});
            }
            return;
        }
        __syncthreads();
    }
    // inter-layer dropout on the incoming dy: the Philox draw of step t-1 is made while step t waits for the other members
    // (it depends on nothing but the position), so it never sits on the step's critical path
    const bool masked = p.dy && p.drop_p > 0.f && valid;
    auto draw = [&](int t) {
        const size_t o = ((size_t)b * T + t) * p.lddy + dcol;
        const f32x4 m = dep_dropmask4(p.seed, p.site, o >> 2, p.drop_p, p.drop_scale);
        return f2(half ? m[2] : m[0], half ? m[3] : m[1]);
    };
    float2 mk = masked ? draw((BI && dir) ? 0 : T - 1) : f2(1.f, 1.f);
    // debug stamps (DEP_TRACE=1, tools/trace_bwd.py): buffered in otherwise unused LDS, copied out after the sweep
    long long* trb = (p.trace && blockIdx.x == 0 && tid == 0) ? p.trace : nullptr;
    long long* trlb = reinterpret_cast<long long*>(smem + (AG ? AG_TRACE_F : BURST ? TRACE_F : 8192));
#define BSTAMP(slot) do { if (trb && t <= 199 && t > 195) trlb[(199 - t) * 8 + (slot)] = (long long)__builtin_readcyclecounter(); } while (0)

    if (trb) trlb[7] = (long long)__builtin_readcyclecounter();
    unsigned* trall = reinterpret_cast<unsigned*>(smem) + p.trall_off;      // DEP_TRACE: low 32 bits of the tick counter at the top of every step
    if constexpr (AG) {
        // ---- all-gather sweep (see AG_MEMBER_BYTES above).  Exchange buffer: [parity][tile][member][gate][plane][64 lanes][16 B]; this
        // thread's pair (units ul, ul+1 of utterance j) is word `pw' of each of its member's six 1 KB blocks -- B-fragment order: lane
        // (k-group ul / 8, utterance j), word (ul % 8) / 2 -- and a wave's 64 words are 256 contiguous bytes.
        float* red = smem;                                  // [step parity][K quarter = wave][own tile][64 lanes][4]
        const unsigned pw = (unsigned)(half + 2 * ((lp >> 4) & 1) + 4 * j + 64 * (lp >> 5) + 128 * jl);
        const unsigned par_bytes = (unsigned)(BI ? 2 * p.nbtp : p.nbtp) * NC * AG_MEMBER_BYTES;
        const unsigned pub0 = (unsigned)(pt * NC + c) * AG_MEMBER_BYTES + pw * 4;
        const unsigned ld0 = (unsigned)(pt * NC + 2 * w) * AG_MEMBER_BYTES + lane * 16;     // this wave's 12 blocks are contiguous: members 2w, 2w+1
        unsigned* srcflags = tflags + 8 * w;                // the eight per-wave flags of source members 2w, 2w+1
        const int rdo = (jl * 64 + (lp >> 4) * 16 + j) * 4 + 2 * half;      // own pair inside a K quarter's two accumulator tiles
        for (int t = T - 1; t >= 0; --t) {
            const int k = T - 1 - t;
            const int tm = (BI && dir) ? k : t;              // the step's time (t counts the sweep down)
            BSTAMP(0);
            if (trb && k < 360) trall[k] = (unsigned)__builtin_readcyclecounter();
            const float* ib = ibuf + (k % KBX) * 6 * SARR + j * SROW + ul;
            const float2 r = ld2(ib), z = ld2(ib + SARR), n = ld2(ib + 2 * SARR), hn = ld2(ib + 3 * SARR), hp = ld2(ib + 4 * SARR), dyi = ld2(ib + 5 * SARR);
            const float2 d = f2(dhrec.x + dpl.x + dyi.x * mk.x, dhrec.y + dpl.y + dyi.y * mk.y);
            float2 dn, dz, dr, dnr, dzt;
            dn.x = d.x * (1.0f - z.x) * (1.0f - n.x * n.x); dn.y = d.y * (1.0f - z.y) * (1.0f - n.y * n.y);
            dz.x = d.x * (hp.x - n.x) * z.x * (1.0f - z.x); dz.y = d.y * (hp.y - n.y) * z.y * (1.0f - z.y);
            dr.x = dn.x * hn.x * r.x * (1.0f - r.x); dr.y = dn.y * hn.y * r.y * (1.0f - r.y);
            dnr.x = dn.x * r.x; dnr.y = dn.y * r.y;
            dzt.x = d.x * z.x; dzt.y = d.y * z.y;
            const float2 drr = dr, dzr = dz, dnrr = dnr;
            if constexpr (RAG) {
                const bool live = tm < len;
                const float2 z2 = f2(0.f, 0.f);
                dn = dep_sel2(live, dn, z2); dz = dep_sel2(live, dz, z2); dr = dep_sel2(live, dr, z2); dnr = dep_sel2(live, dnr, z2);
            }
            const unsigned epoch = (unsigned)(k + 1);
            if (t > 0) {      // publish first: the (hi, lo) pair words of dr, dz, dn*r -- what every member's MFMAs read
                unsigned h0, l0, h1, l1, h2, l2;
                if constexpr (RAG) {      // the words of the unselected values (rounded as the dense instance rounds them), zeroed for a dead step
                    split_pair(drr.x, drr.y, h0, l0); split_pair(dzr.x, dzr.y, h1, l1); split_pair(dnrr.x, dnrr.y, h2, l2);
                    if (tm >= len) { h0 = l0 = h1 = l1 = h2 = l2 = 0u; }
                } else {
                    split_pair(dr.x, dr.y, h0, l0); split_pair(dz.x, dz.y, h1, l1); split_pair(dnr.x, dnr.y, h2, l2);
                }
                const unsigned po = (unsigned)(t & 1) * par_bytes + pub0;
                const unsigned wds[6] = {h0, l0, h1, l1, h2, l2};
                if (fast) {           // same-XCD clusters: plain stores (that XCD's L2 is the coherence point)
#pragma unroll
                    for (int e = 0; e < 6; ++e) __builtin_amdgcn_raw_buffer_store_b32(wds[e], rsrc, po + e * 1024, 0, 0);
                } else {              // write-through
#pragma unroll
                    for (int e = 0; e < 6; ++e) __builtin_amdgcn_raw_buffer_store_b32(wds[e], rsrc, po + e * 1024, 0, 16);
                }
            }
            {
                float* ob = obuf + (k % OSL) * 4 * SARR + j * SROW + ul;
                st2(ob, dr); st2(ob + SARR, dz); st2(ob + 2 * SARR, dn); st2(ob + 3 * SARR, dnr);
            }
            dbr.x += dr.x; dbr.y += dr.y; dbz.x += dz.x; dbz.y += dz.y; dbn.x += dn.x; dbn.y += dn.y; dbh.x += dnr.x; dbh.y += dnr.y;
            BSTAMP(1);
            if (t == 0) {
                if (p.dhx && valid) store_dhx(d, z);
                bar_lds(); break;                            // (the service waves' final flush reads obuf behind this barrier)
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's six stores are acknowledged
            BSTAMP(2);
            if (lane == 0) { if (fast) st_local(myflag, epoch); else st_agent(myflag, epoch); }
            BSTAMP(3);
            // One vector poll of the eight per-wave flags of both source members, then all twelve requests; the Philox draw of the next
            // step's dropout mask (layer 0 only, ~150 VALU instructions) goes behind the requests, into the loads' shadow.  Measured and
            // dropped (profiles/r05_s2_allgather_poll_variants.txt): member-by-member poll + requests (the second poll returns behind the
            // first six loads: +2 %), polling through the scalar path (s_load ... glc: the flags arrive thousands of ticks late, 2x slower).
            const unsigned lo_ = (unsigned)(t & 1) * par_bytes + ld0;
            u32x4 gfr[6][2];
            if (!wait_flags(srcflags, 8, epoch, p.status, 3)) return;
            BSTAMP(4);
#pragma unroll
            for (int ks = 0; ks < 6; ++ks)
#pragma unroll
                for (int pl = 0; pl < 2; ++pl)
                    gfr[ks][pl] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, lo_ + (unsigned)(ks * 2 + pl) * 1024, 0, 16 /* sc1: served by L2 */);
            __builtin_amdgcn_sched_barrier(0);               // all twelve requests first (hipcc otherwise sinks each load next to its MFMAs: twelve round trips in a row)
            if (masked) mk = draw((BI && dir) ? tm + 1 : t - 1);
            __builtin_amdgcn_sched_barrier(0);
            f32x4 acc[2] = {zero4(), zero4()};
#pragma unroll
            for (int ks = 0; ks < 6; ++ks) {
                const bf16x8 gh = __builtin_bit_cast(bf16x8, gfr[ks][0]), gl = __builtin_bit_cast(bf16x8, gfr[ks][1]);
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const bf16x8 wh = __builtin_bit_cast(bf16x8, wa[i][ks][0]), wl = __builtin_bit_cast(bf16x8, wa[i][ks][1]);
                    acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh, gl, acc[i], 0, 0, 0);
                    acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wl, gh, acc[i], 0, 0, 0);
                    acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh, gh, acc[i], 0, 0, 0);
                }
            }
            float* rw = red + ((k & 1) * 8 + w * 2) * 256 + lane * 4;
            *reinterpret_cast<f32x4*>(rw) = acc[0]; *reinterpret_cast<f32x4*>(rw + 256) = acc[1];
            BSTAMP(5);
            bar_lds();
            const float* rr = red + (k & 1) * 2048 + rdo;
            float2 s = f2(0.f, 0.f);
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) { const float2 v = ld2(rr + q4 * 512); s.x += v.x; s.y += v.y; }      // fixed order: deterministic
            if constexpr (RAG) dhrec = dep_sel2(tm < len, f2(dzt.x + s.x, dzt.y + s.y), dhrec);      // dead step: the incoming dh passes through
            else dhrec = f2(dzt.x + s.x, dzt.y + s.y);
            BSTAMP(6);
        }
    } else
    for (int t = T - 1; t >= 0; --t) {
        const int tm = (BI && dir) ? T - 1 - t : t;      // the step's time (t counts the sweep down)
        const size_t row = (size_t)b * T + tm;
        BSTAMP(0);
        if (trb && T - 1 - t < 360) trall[T - 1 - t] = (unsigned)__builtin_readcyclecounter();
        if constexpr (BURST) {
            const float* ib = ibuf + ((T - 1 - t) % KBX) * 6 * SARR + j * SROW + ul;
            cur.r = ld2(ib); cur.z = ld2(ib + SARR); cur.n = ld2(ib + 2 * SARR); cur.hn = ld2(ib + 3 * SARR);
            cur.hp = ld2(ib + 4 * SARR); cur.dy = ld2(ib + 5 * SARR);
        }
        const float2 dyv = f2(cur.dy.x * mk.x, cur.dy.y * mk.y);
        const float2 r = cur.r, z = cur.z, n = cur.n, hn = cur.hn, hp = cur.hp;
        const float2 d = f2(dhrec.x + dpl.x + dyv.x, dhrec.y + dpl.y + dyv.y);
        float2 dn, dz, dr, dnr, dzt;
        dn.x = d.x * (1.0f - z.x) * (1.0f - n.x * n.x); dn.y = d.y * (1.0f - z.y) * (1.0f - n.y * n.y);
        dz.x = d.x * (hp.x - n.x) * z.x * (1.0f - z.x); dz.y = d.y * (hp.y - n.y) * z.y * (1.0f - z.y);
        dr.x = dn.x * hn.x * r.x * (1.0f - r.x); dr.y = dn.y * hn.y * r.y * (1.0f - r.y);
        dnr.x = dn.x * r.x; dnr.y = dn.y * r.y;
        dzt.x = d.x * z.x; dzt.y = d.y * z.y;
        const float2 drr = dr, dzr = dz, dnrr = dnr;
        if constexpr (RAG) {
            const bool live = tm < len;
            const float2 z2 = f2(0.f, 0.f);
            dn = dep_sel2(live, dn, z2); dz = dep_sel2(live, dz, z2); dr = dep_sel2(live, dr, z2); dnr = dep_sel2(live, dnr, z2);
        }
        if constexpr (SPLIT) {                        // one (hi, lo) bf16 pair word per gate: units ul, ul+1
            unsigned h0, l0, h1, l1, h2, l2;
            if constexpr (RAG) {          // the words of the unselected values (rounded as the dense instance rounds them), zeroed for a dead step
                split_pair(drr.x, drr.y, h0, l0); split_pair(dzr.x, dzr.y, h1, l1); split_pair(dnrr.x, dnrr.y, h2, l2);
                if (tm >= len) { h0 = l0 = h1 = l1 = h2 = l2 = 0u; }
            } else {
                split_pair(dr.x, dr.y, h0, l0); split_pair(dz.x, dz.y, h1, l1); split_pair(dnr.x, dnr.y, h2, l2);
            }
            const int o = j * LDGB + ul;
            *reinterpret_cast<unsigned*>(dg_hi + o) = h0; *reinterpret_cast<unsigned*>(dg_lo + o) = l0;
            *reinterpret_cast<unsigned*>(dg_hi + o + 32) = h1; *reinterpret_cast<unsigned*>(dg_lo + o + 32) = l1;
            *reinterpret_cast<unsigned*>(dg_hi + o + 64) = h2; *reinterpret_cast<unsigned*>(dg_lo + o + 64) = l2;
        } else {
            st2(dgs + j * LDG + ul, dr); st2(dgs + j * LDG + 32 + ul, dz); st2(dgs + j * LDG + 64 + ul, dnr);
        }
        if constexpr (BURST) {
            float* ob = obuf + ((T - 1 - t) % OSL) * 4 * SARR + j * SROW + ul;
            st2(ob, dr); st2(ob + SARR, dz); st2(ob + 2 * SARR, dn); st2(ob + 3 * SARR, dnr);
        } else if (valid) {
            float* g = p.dgi + row * p.lddg + (BI ? dir * 3 * H : 0);
            st2(g + col, dr); st2(g + H + col, dz); st2(g + 2 * H + col, dn);
            st2(p.dghn + row * p.lddghn + dcol, dnr);
        }
        dbr.x += dr.x; dbr.y += dr.y; dbz.x += dz.x; dbz.y += dz.y; dbn.x += dn.x; dbn.y += dn.y; dbh.x += dnr.x; dbh.y += dnr.y;
        bar_lds();                                   // LDS only: the dgi/dghn stores above stay in flight
        BSTAMP(1);
        if (t == 0) {
            if (p.dhx && valid) store_dhx(d, z);
            break;
        }
        if constexpr (!BURST) load_step((BI && dir) ? tm + 1 : t - 1, nxt); // independent of the recurrence: in flight under the MFMAs
        f32x4 acc[NTW];
#pragma unroll
        for (int i = 0; i < NTW; ++i) acc[i] = zero4();
        if constexpr (SPLIT) {
            const int go = ml * LDGB + mq * 8;        // lane (utterance ml, k-group mq): 8 consecutive k of each k-step
            bf16x8 gh[3], gl[3];
#pragma unroll
            for (int ks = 0; ks < 3; ++ks) {
                gh[ks] = *reinterpret_cast<const bf16x8*>(dg_hi + go + ks * 32);
                gl[ks] = *reinterpret_cast<const bf16x8*>(dg_lo + go + ks * 32);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int ks = 0; ks < 3; ++ks)
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
            for (int k = 0; k < KCB; ++k) {
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int i = 0; i < NTW; ++i)
                        acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[i][k][e], hv[k][e], acc[i], 0, 0, 0);
            }
        }
        BSTAMP(2);
        // publish: payload[parity][tile][src c][out tile][lane][4]
        const unsigned epoch = (unsigned)(T - t);
        const size_t pbase = (size_t)(t & 1) * pstride + tile_base;
#pragma unroll
        for (int i = 0; i < NTW; ++i) {
            const size_t fo = pbase + ((size_t)(c * NTT + w * NTW + i) * 64 + lane) * 4;
            u32x4 v;
            v.x = __float_as_uint(acc[i][0]); v.y = __float_as_uint(acc[i][1]);
            v.z = __float_as_uint(acc[i][2]); v.w = __float_as_uint(acc[i][3]);
            if (fast) __builtin_amdgcn_raw_buffer_store_b128(v, rsrc, (unsigned)(fo * 4), 0, 0 /* plain: stays in this XCD's L2 */);
            else __builtin_amdgcn_raw_buffer_store_b128(v, rsrc, (unsigned)(fo * 4), 0, 16 /* sc1: write-through */);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // every storing wave drains its write-through stores
        BSTAMP(3);
        // per-wave flags: this wave's partials are acknowledged -> say so; nobody waits for the sibling waves here (their
        // flags are among the 4 NC words every wave polls below, which also orders this step's LDS reads before the next
        // step's LDS writes: a sibling raises its flag only after its MFMAs have read the gate-gradient planes)
        if (lane == 0) { if (fast) st_local(myflag, epoch); else st_agent(myflag, epoch); }
        if (masked) mk = draw((BI && dir) ? tm + 1 : t - 1);      // next step's mask, in the shadow of the wait below
        BSTAMP(4);
        // wait for every member's flag (one wave polls, relaxed; flags are monotonic)
        // every wave polls the flags itself (no verdict-broadcast barrier); a wave that gives up leaves, the hardware
        // barrier only counts live waves and the others give up too (status word raised)
        if (!wait_flags(tflags, nflags, epoch, p.status, 3)) return;
        BSTAMP(5);
        // gather this thread's two columns from the NC partials, sum in member order
        float2 s = f2(0.f, 0.f);
        const float* src = p.payload + pbase + ((size_t)(2 * c + jl) * 64 + lp) * 4 + 2 * half;
        constexpr int NCM = 2 * NTW;                  // members of a cluster = H / 32
        float2 part[NCM];
#pragma unroll
        for (int m = 0; m < NCM; ++m) part[m] = ld2_agent(src + (size_t)m * NTT * 256);
#pragma unroll
        for (int m = 0; m < NCM; ++m) { s.x += part[m].x; s.y += part[m].y; }
        if constexpr (RAG) dhrec = dep_sel2(tm < len, f2(dzt.x + s.x, dzt.y + s.y), dhrec);      // dead step: the incoming dh passes through
        else dhrec = f2(dzt.x + s.x, dzt.y + s.y);
        if constexpr (!BURST) cur = nxt;
        BSTAMP(6);
    }
    if (trb) {
        trlb[15] = (long long)__builtin_readcyclecounter();
        for (int i = 0; i < 32; ++i) trb[i] = trlb[i];
        unsigned* o = reinterpret_cast<unsigned*>(trb + 64);
        for (int i = 0; i < T && i < 360; ++i) o[i] = trall[i];
    }
    // bias-gradient partials dbpart[bt][4][H]: sum over the 16 utterance rows = lanes that differ in bits 1..4
    float2 a[4] = {dbr, dbz, dbn, dbh};
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int m = 2; m <= 16; m <<= 1) { a[k].x += __shfl_xor(a[k].x, m, 64); a[k].y += __shfl_xor(a[k].y, m, 64); }
    if (j == 0) {
        size_t brow = (size_t)(p.b0 / BT + bt);      // one row of partials per tile (BI: per direction and tile)
        if constexpr (BI) brow += (size_t)dir * p.nbt;
        float* o = p.dbpart + brow * 4 * H;
        st2(o + col, a[0]); st2(o + H + col, a[1]); st2(o + 2 * H + col, a[2]); st2(o + 3 * H + col, a[3]);
    }
}

// =============================================================================== GRU forward, flag-published
// Same member/wave roles as gru_fwd_cluster (rnn_cluster.hip): wave w = (hidden tile jl = w>>1, K half kh = w&1).
// h_t travels as plain fp32 rows payload[parity][tile][16][H]: each lane stores its two values with one 8-byte
// sc1 store, the workgroup drains + barriers, one lane raises the member's flag; after the NC flags are seen the
// whole 16xH block is read once with 16-byte sc1 loads into LDS (no per-value polling traffic).
struct F2 {
    int B, T, H, nbtp, b0;      // b0: first utterance of this launch's batch chunk (B is the whole batch)
    const f32x4* wp; const float* b_hh;
    const float* gi; int ldgi;
    float* y; int ldy;
    float* ydrop; float drop_p, drop_scale; uint64_t seed; uint32_t site;
    float* pooled; float pool_scale;
    float* h_n;
    float* sv0; float* sv1; float* sv2; float* sv3;
    unsigned* status; unsigned* flags; unsigned* hello; float* payload; unsigned payload_bytes;
    int nofast;              // DEP_CLUSTER_NOFAST=1: always use the write-through (placement-agnostic) stores
    long long* trace;        // debug: s_memtime stamps of workgroup 0 (DEP_TRACE=1), else nullptr
    const unsigned* only_if; // run only if this word is set (fallback behind an exclusive forward kernel), or nullptr
    int sv16;                // saved gates r, z, n written as 16-bit fixed point
    const int* lengths; int pool_mean;      // ragged instances (RAG): row b is live for t < lengths[b]; a mean pool divides by lengths[b]
    const float* hx;         // this layer's (B, H) initial state (dep_rnn_forward_state[_varlen] on impl 4 / 5), or nullptr = zeros
};
// The parameters of the bidirectional instances (BI, impl 6): direction 1's W_hh image and b_hh, and the row stride of the saved gates
// (2H).  A struct of their own, so that the unidirectional instances keep their kernel arguments (and with them their ISA: the implicit
// arguments sit behind the struct).
struct F2B : F2 { const f32x4* wp1; const float* b_hh1; int ldsv; };

// RAG: the ragged-batch instances (dep_rnn_forward_varlen): h = live ? new : previous (what is published, kept and returned as h_n),
// y / dropout(y) / the pool take live ? h : 0.  Everything about the hand-off is the dense instance's.
// hx (a run-time pointer, as in rnn_sweep.hip): a global INPUT, so every member fills its LDS copy of the tile's 16 x H block from it in
// front of the step loop, with no exchange -- as fp32, or (SPLIT) as the two bf16 planes of split_word(hx), the bits a previous step
// would have published -- and starts hprev from its own two columns.  The loop, the hand-off and every trip count are untouched; a
// ragged row with len = 0 never leaves hprev, so it returns hx bit for bit.  Rows b >= B of the last tile read nothing and stay 0.
// BI: the bidirectional instances (impl 6), as in gru_fwd_mfma.  A cluster is a (direction, tile) PAIR, both directions of a batch chunk in
// one launch: block = (c * 2 + dir) * nbtp + bt (nbtp, the padded tiles PER DIRECTION, is a multiple of 8: block id -> XCD stays member- and
// direction-invariant), and the pair dir * nbtp + bt indexes the flag words, the hello words and the payload.  Direction 1 takes wp1 / b_hh1,
// visits t = T-1-s at sweep step s (epochs, payload parity and the gi prefetch follow s) and every array is the direction-interleaved one:
// gi (B,T,2*3H), y / dropout(y) (B,T,2H; ldy) and the saved gates (B,T,2H; ldsv), pool (B,2H), hx / h_n (2,B,H).  The dropout draw is the
// element's index in (B,T,2H), as gru_fwd_mfma draws it.  A ragged row's reverse sweep meets its dead steps first and carries hx (or 0)
// through them by the same live select.  BI = false is the unidirectional text.
template <int KCH, bool SPLIT, bool RAG = false, bool BI = false>      // SPLIT: 3-term bf16 split of the recurrent product, as in gru_fwd_cluster16
__global__ __launch_bounds__(CT) void gru_fwd_cluster_r1(std::conditional_t<BI, F2B, F2> p) {
    // contraction by syntax: see DEP_FP_CONTRACT_NOTE in dep_common.h (why, and how to re-verify the dense instances after a compiler change)
#pragma clang fp contract(on)
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int H = p.H, T = p.T, LDH = H + LPAD, KC = H / 16, NC = H / 32;
    const int c = BI ? blockIdx.x / (2 * p.nbtp) : blockIdx.x / p.nbtp, bt = blockIdx.x % p.nbtp;
    const int dir = BI ? (int)(blockIdx.x / p.nbtp) & 1 : 0;
    const int pt = BI ? dir * p.nbtp + bt : bt;      // the cluster's (direction, tile) pair: flags, hello words, payload
    if (p.b0 + bt * BT >= p.B) return;
    if (ld_agent(p.status) != 0) return;           // an earlier sweep of this step gave up: the status word is sticky until the next dep_rnn_forward
    if (p.only_if && ld_agent(const_cast<unsigned*>(p.only_if)) == 0) return;      // the exclusive kernel in front of us did the work
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int j = lane & 15, q = lane >> 4, jl = w >> 1, kh = w & 1;
    const int jt = c * 2 + jl;
    const int b = p.b0 + bt * BT + j;
    const bool valid = b < p.B;
    int len = T;
    if constexpr (RAG) len = valid ? dep_row_len(p.lengths, b, T) : 0;
    const int LDHB = H + 8;                           // bf16 elements per row of a split plane
    float* hs = smem;                                 // [16][LDH] fp32, or (SPLIT) two bf16 planes [16][LDHB]
    const int hs_floats = SPLIT ? BT * LDHB : BT * LDH;
    unsigned short* hs_hi = reinterpret_cast<unsigned short*>(smem);
    unsigned short* hs_lo = hs_hi + BT * LDHB;
    float* red = smem + hs_floats;                    // [4][3][64][4]
    for (int i = tid; i < hs_floats; i += CT) hs[i] = 0.f;
    const float* const hxd = BI ? (p.hx ? p.hx + (size_t)dir * p.B * H : nullptr) : p.hx;      // the direction's own slice of hx (2,B,H)
    if (p.hx) {
        __syncthreads();                              // (the zero fill walks the planes in another order)
        const int xshift = __ffs(H) - 1;
#pragma unroll
        for (int k = 0; k < KCH / 2; ++k) {           // the gather's piece map: 16-byte piece tid + CT k of the 16 x H block
            const int i4 = (tid + CT * k) * 4;
            const int xr = i4 >> xshift, xc = i4 & (H - 1);
            const int xb = p.b0 + bt * BT + xr;
            if (xb < p.B) {
                const float* src = hxd + (size_t)xb * H + xc;
                const float2 x01 = ld2(src), x23 = ld2(src + 2);
                if constexpr (SPLIT) {
                    const unsigned v0 = split_word(x01.x), v1 = split_word(x01.y), v2 = split_word(x23.x), v3 = split_word(x23.y);
                    const int o = xr * LDHB + xc;
                    uint2 hi2, lo2;
                    hi2.x = (v0 >> 16) | (v1 & 0xffff0000u); hi2.y = (v2 >> 16) | (v3 & 0xffff0000u);
                    lo2.x = (v0 & 0xffffu) | (v1 << 16);      lo2.y = (v2 & 0xffffu) | (v3 << 16);
                    *reinterpret_cast<uint2*>(hs_hi + o) = hi2; *reinterpret_cast<uint2*>(hs_lo + o) = lo2;
                } else {
                    const f32x4 f = {x01.x, x01.y, x23.x, x23.y};
                    *reinterpret_cast<f32x4*>(hs + xr * LDH + xc) = f;
                }
            }
        }
    }

    constexpr int KS2 = KCH / 2;                      // 32-wide k-steps per wave (SPLIT)
    f32x4 wr[SPLIT ? 1 : 3][SPLIT ? 1 : KCH];
    u32x4 wq[SPLIT ? 3 : 1][SPLIT ? KS2 : 1][2];      // [gate][k-step][hi, lo]
    const f32x4* wpd = p.wp; const float* bhd = p.b_hh;      // the direction's own W_hh image and b_hh
    if constexpr (BI) { if (dir) { wpd = p.wp1; bhd = p.b_hh1; } }
    if constexpr (SPLIT) {
        const u32x4* wpq = reinterpret_cast<const u32x4*>(wpd);
#pragma unroll
        for (int g = 0; g < 3; ++g)
#pragma unroll
            for (int ks = 0; ks < KS2; ++ks)
#pragma unroll
                for (int pl = 0; pl < 2; ++pl)
                    wq[g][ks][pl] = wpq[(size_t)((((jt * 3 + g) * 2 + kh) * KS2 + ks) * 2 + pl) * 64 + lane];
    } else {
#pragma unroll
        for (int g = 0; g < 3; ++g)
#pragma unroll
            for (int k = 0; k < KCH; ++k)
                wr[g][k] = wpd[(size_t)((jt * 3 + g) * KC + kh * KCH + k) * 64 + lane];
    }
    const int col = jt * 16 + q * 4 + 2 * kh;
    const int dcol = BI ? dir * H + col : col;        // the column in the direction-interleaved rows of y, dropout(y), the saved gates and the pool
    float2 bh[3];
#pragma unroll
    for (int g = 0; g < 3; ++g) bh[g] = ld2(bhd + g * H + col);
    float2 hprev = (p.hx && valid) ? ld2(hxd + (size_t)b * H + col) : f2(0.f, 0.f), pool = f2(0.f, 0.f);
    const size_t pstride = (size_t)(BI ? 2 * p.nbtp : p.nbtp) * BT * H;
    const size_t tile_base = (size_t)pt * BT * H;
    __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)p.payload, 0, p.payload_bytes, 0x00020000);
    unsigned* myflag = p.flags + pt * NC + c;
    unsigned* tflags = p.flags + pt * NC;
    const int hshift = __ffs(H) - 1;
    const int sx = p.nofast ? 0 : cluster_same_xcd(p.hello + pt * NC, NC, c, p.status);
    if (sx < 0) return;
    const bool fast = sx == 1;
    const float* const gid = BI ? p.gi + dir * 3 * H : p.gi;      // the direction's three gate blocks of the (B,T,2*3H) rows
    float2 gin[3];
#pragma unroll
    for (int g = 0; g < 3; ++g)
        gin[g] = valid ? ld2(gid + ((size_t)b * T + ((BI && dir) ? T - 1 : 0)) * p.ldgi + g * H + col) : f2(0.f, 0.f);
    __syncthreads();

    long long* tr = (p.trace && blockIdx.x == 0 && tid == 0) ? p.trace : nullptr;
    for (int s = 0; s < T; ++s) {
        const int t = (BI && dir) ? T - 1 - s : s;
        const size_t row = (size_t)b * T + t;
        DEP_STAMP(0);
        float2 gi[3];
#pragma unroll
        for (int g = 0; g < 3; ++g) gi[g] = gin[g];
        if (valid && s + 1 < T) {      // the next SWEEP step's row: t + 1, or (reverse) t - 1
#pragma unroll
            for (int g = 0; g < 3; ++g) gin[g] = ld2(gid + ((BI && dir) ? row - 1 : row + 1) * p.ldgi + g * H + col);
        }
        f32x4 acc[3] = {zero4(), zero4(), zero4()};
        if constexpr (SPLIT) {
            const int ho = j * LDHB + kh * KCH * 16 + q * 8;
            bf16x8 hh[KS2], hl[KS2];
#pragma unroll
            for (int ks = 0; ks < KS2; ++ks) {
                hh[ks] = *reinterpret_cast<const bf16x8*>(hs_hi + ho + ks * 32);
                hl[ks] = *reinterpret_cast<const bf16x8*>(hs_lo + ho + ks * 32);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int ks = 0; ks < KS2; ++ks)
#pragma unroll
                for (int g = 0; g < 3; ++g) {
                    const bf16x8 wh = __builtin_bit_cast(bf16x8, wq[g][ks][0]), wl = __builtin_bit_cast(bf16x8, wq[g][ks][1]);
                    acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh, hl[ks], acc[g], 0, 0, 0);
                    acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wl, hh[ks], acc[g], 0, 0, 0);
                    acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh, hh[ks], acc[g], 0, 0, 0);
                }
        } else {
            const float* hrow = hs + j * LDH + kh * KCH * 16 + q * 4;
            f32x4 hv[KCH];                             // all B fragments first: one LDS latency, not KCH of them
#pragma unroll
            for (int k = 0; k < KCH; ++k) hv[k] = ld4(hrow + k * 16);
            __builtin_amdgcn_sched_barrier(0);         // keep the loads grouped: hipcc otherwise sinks each next to its MFMAs
#pragma unroll
            for (int k = 0; k < KCH; ++k) {
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int g = 0; g < 3; ++g)
                        acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[g][k][e], hv[k][e], acc[g], 0, 0, 0);
            }
        }
        DEP_STAMP(1);
#pragma unroll
        for (int g = 0; g < 3; ++g) *reinterpret_cast<f32x4*>(red + ((w * 3 + g) * 64 + lane) * 4) = acc[g];
        bar_lds();
        DEP_STAMP(2);
        float2 tot[3];
#pragma unroll
        for (int g = 0; g < 3; ++g) {
            const float2 pv = ld2(red + (((w ^ 1) * 3 + g) * 64 + lane) * 4 + 2 * kh);
            tot[g].x = (kh ? acc[g][2] : acc[g][0]) + pv.x;
            tot[g].y = (kh ? acc[g][3] : acc[g][1]) + pv.y;
        }
        float2 r, z, hn, n, h;
        r.x = fast_sigmoid(gi[0].x + tot[0].x + bh[0].x); r.y = fast_sigmoid(gi[0].y + tot[0].y + bh[0].y);
        z.x = fast_sigmoid(gi[1].x + tot[1].x + bh[1].x); z.y = fast_sigmoid(gi[1].y + tot[1].y + bh[1].y);
        hn.x = tot[2].x + bh[2].x; hn.y = tot[2].y + bh[2].y;
        n.x = fast_tanh(gi[2].x + r.x * hn.x); n.y = fast_tanh(gi[2].y + r.y * hn.y);
        h.x = z.x * hprev.x + (1.0f - z.x) * n.x; h.y = z.y * hprev.y + (1.0f - z.y) * n.y;      // (the fused product is z * h_{t-1}: contraction by syntax, see above)
        float2 hy = h;                                // what y, dropout(y) and the pool see
        if constexpr (RAG) {
            const bool live = t < len;
            h = dep_sel2(live, h, hprev);             // the state freezes behind the row's last step: published and kept as it is
            hy = dep_sel2(live, h, f2(0.f, 0.f));
        }
        hprev = h; pool.x += hy.x; pool.y += hy.y;
        const unsigned epoch = (unsigned)s + 1u;
        const size_t pbase = (size_t)(s & 1) * pstride + tile_base;
        const bool more = s + 1 < T;
        DEP_STAMP(3);
        if (more) {       // publish first: it is on the critical path of the other members
            const u64 bits = SPLIT ? ((u64)split_word(h.x) | ((u64)split_word(h.y) << 32))
                                   : ((u64)__float_as_uint(h.x) | ((u64)__float_as_uint(h.y) << 32));
            if (fast) __hip_atomic_store((gu64*)(p.payload + pbase + (size_t)j * H + col), bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            else __hip_atomic_store((gu64*)(p.payload + pbase + (size_t)j * H + col), bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            DEP_STAMP(4);
            __builtin_amdgcn_s_barrier();
            if (tid == 0) { if (fast) st_local(myflag, epoch); else st_agent(myflag, epoch); }
        }
        if (valid) {
            const size_t o = row * p.ldy + dcol;
            st2(p.y + o, hy);
            if (p.ydrop) {
                const f32x4 m = dep_dropmask4(p.seed, p.site, o >> 2, p.drop_p, p.drop_scale);
                st2(p.ydrop + o, f2(hy.x * (kh ? m[2] : m[0]), hy.y * (kh ? m[3] : m[1])));
            }
            if (p.sv0) {
                size_t so = row * H + col;
                if constexpr (BI) so = row * p.ldsv + dcol;
                if (p.sv16) {
                    *reinterpret_cast<unsigned*>(reinterpret_cast<unsigned short*>(p.sv0) + so) = pack_unorm2(r.x, r.y);
                    *reinterpret_cast<unsigned*>(reinterpret_cast<unsigned short*>(p.sv1) + so) = pack_unorm2(z.x, z.y);
                    *reinterpret_cast<unsigned*>(reinterpret_cast<unsigned short*>(p.sv2) + so) = pack_snorm2(n.x, n.y);
                } else { st2(p.sv0 + so, r); st2(p.sv1 + so, z); st2(p.sv2 + so, n); }
                st2(p.sv3 + so, hn);
            }
        }
        if (more) {
            if (!wait_flags(tflags, NC, epoch, p.status, 4)) return;      // every wave polls
            DEP_STAMP(5);
            DEP_STAMP(6);
            constexpr int PER = KCH / 2;              // 16-byte pieces per thread = 16*H/4/256
#pragma unroll
            for (int k = 0; k < PER; ++k) {
                const int i4 = (tid + CT * k) * 4;    // float index inside the 16xH block
                const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (unsigned)((pbase + i4) * 4), 0, 16 /* sc1 */);
                if constexpr (SPLIT) {
                    const int o = (i4 >> hshift) * LDHB + (i4 & (H - 1));
                    uint2 hi2, lo2;
                    hi2.x = (v.x >> 16) | (v.y & 0xffff0000u); hi2.y = (v.z >> 16) | (v.w & 0xffff0000u);
                    lo2.x = (v.x & 0xffffu) | (v.y << 16);      lo2.y = (v.z & 0xffffu) | (v.w << 16);
                    *reinterpret_cast<uint2*>(hs_hi + o) = hi2; *reinterpret_cast<uint2*>(hs_lo + o) = lo2;
                } else {
                    f32x4 f;
                    f[0] = __uint_as_float(v.x); f[1] = __uint_as_float(v.y); f[2] = __uint_as_float(v.z); f[3] = __uint_as_float(v.w);
                    *reinterpret_cast<f32x4*>(hs + (i4 >> hshift) * LDH + (i4 & (H - 1))) = f;
                }
            }
            bar_lds();
            DEP_STAMP(7);
        }
    }
    if (valid) {
        const float ps = RAG ? dep_ragged_pool_scale(p.pool_mean, len, T, p.pool_scale) : p.pool_scale;
        if (p.pooled) st2(p.pooled + (BI ? (size_t)b * 2 * H + dcol : (size_t)b * H + col), f2(pool.x * ps, pool.y * ps));
        if (p.h_n) st2(p.h_n + (BI ? (size_t)dir * p.B + b : (size_t)b) * H + col, hprev);
    }
}

// split-precision images (rnn_cluster_common.h), G = 3
__global__ void pack_cluster_bwd_split_kernel(const float* __restrict__ W, u32x4* __restrict__ out, int H) {
    const long n = pack_bwd_split_pieces(3, H);
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    pack_bwd_split_piece<3>(W, out, H, idx);
}
__global__ void pack_cluster_fwd_split_kernel(const float* __restrict__ W, u32x4* __restrict__ out, int H) {
    const long n = pack_fwd_split_pieces(3, H);
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    pack_fwd_split_piece<3>(W, out, H, idx);
}

// all split-precision images of a step in ONE launch (blockIdx.y = job): five ~4.5 us launches per training step otherwise
struct PackJobs { const float* src[8]; u32x4* dst[8]; int bwd[8]; int n; };
__global__ void pack_cluster_split_multi_kernel(PackJobs j, int H) {
    const int k = blockIdx.y;
    if (k >= j.n) return;
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const float* W = j.src[k]; u32x4* out = j.dst[k];
    if (j.bwd[k]) {
        if (idx >= pack_bwd_split_pieces(3, H)) return;
        pack_bwd_split_piece<3>(W, out, H, idx);
    } else {
        if (idx >= pack_fwd_split_pieces(3, H)) return;
        pack_fwd_split_piece<3>(W, out, H, idx);
    }
}

// ---- the launchable instances.  Every one asks for more than half of the CU's 160 KiB LDS: the dispatcher can then never co-locate
// two members on one CU (they would share the four matrix pipes and stretch every step of BOTH clusters).
Instance<F2>& fwd_instance(int H, bool split, bool rag) {      // KCH = H / 32; exact fp32 | split products
    static Instance<F2> rows[4][2] = {
        { DEP_INSTANCE((gru_fwd_cluster_r1<2, false>), EXCLUSIVE_LDS), DEP_INSTANCE((gru_fwd_cluster_r1<2, true>), EXCLUSIVE_LDS) },
        { DEP_INSTANCE((gru_fwd_cluster_r1<4, false>), EXCLUSIVE_LDS), DEP_INSTANCE((gru_fwd_cluster_r1<4, true>), EXCLUSIVE_LDS) },
        { DEP_INSTANCE((gru_fwd_cluster_r1<8, false>), EXCLUSIVE_LDS), DEP_INSTANCE((gru_fwd_cluster_r1<8, true>), EXCLUSIVE_LDS) },
        { DEP_INSTANCE((gru_fwd_cluster_r1<16, false>), EXCLUSIVE_LDS), DEP_INSTANCE((gru_fwd_cluster_r1<16, true>), EXCLUSIVE_LDS) } };
    // ... and the ragged-batch instances of the same forms (dep_rnn_forward_varlen)
    static Instance<F2> ragged[4][2] = {
        { DEP_INSTANCE((gru_fwd_cluster_r1<2, false, true>), EXCLUSIVE_LDS), DEP_INSTANCE((gru_fwd_cluster_r1<2, true, true>), EXCLUSIVE_LDS) },
        { DEP_INSTANCE((gru_fwd_cluster_r1<4, false, true>), EXCLUSIVE_LDS), DEP_INSTANCE((gru_fwd_cluster_r1<4, true, true>), EXCLUSIVE_LDS) },
        { DEP_INSTANCE((gru_fwd_cluster_r1<8, false, true>), EXCLUSIVE_LDS), DEP_INSTANCE((gru_fwd_cluster_r1<8, true, true>), EXCLUSIVE_LDS) },
        { DEP_INSTANCE((gru_fwd_cluster_r1<16, false, true>), EXCLUSIVE_LDS), DEP_INSTANCE((gru_fwd_cluster_r1<16, true, true>), EXCLUSIVE_LDS) } };
    return (rag ? ragged : rows)[H == 64 ? 0 : H == 128 ? 1 : H == 256 ? 2 : 3][split];
}
// ... and the bidirectional instances (impl 6), dense and ragged
Instance<F2B>& fwd_bi_instance(int H, bool split, bool rag) {
    static Instance<F2B> bidir[4][2] = {
        { DEP_INSTANCE((gru_fwd_cluster_r1<2, false, false, true>), EXCLUSIVE_LDS), DEP_INSTANCE((gru_fwd_cluster_r1<2, true, false, true>), EXCLUSIVE_LDS) },
        { DEP_INSTANCE((gru_fwd_cluster_r1<4, false, false, true>), EXCLUSIVE_LDS), DEP_INSTANCE((gru_fwd_cluster_r1<4, true, false, true>), EXCLUSIVE_LDS) },
        { DEP_INSTANCE((gru_fwd_cluster_r1<8, false, false, true>), EXCLUSIVE_LDS), DEP_INSTANCE((gru_fwd_cluster_r1<8, true, false, true>), EXCLUSIVE_LDS) },
        { DEP_INSTANCE((gru_fwd_cluster_r1<16, false, false, true>), EXCLUSIVE_LDS), DEP_INSTANCE((gru_fwd_cluster_r1<16, true, false, true>), EXCLUSIVE_LDS) } };
    static Instance<F2B> bidir_ragged[4][2] = {
        { DEP_INSTANCE((gru_fwd_cluster_r1<2, false, true, true>), EXCLUSIVE_LDS), DEP_INSTANCE((gru_fwd_cluster_r1<2, true, true, true>), EXCLUSIVE_LDS) },
        { DEP_INSTANCE((gru_fwd_cluster_r1<4, false, true, true>), EXCLUSIVE_LDS), DEP_INSTANCE((gru_fwd_cluster_r1<4, true, true, true>), EXCLUSIVE_LDS) },
        { DEP_INSTANCE((gru_fwd_cluster_r1<8, false, true, true>), EXCLUSIVE_LDS), DEP_INSTANCE((gru_fwd_cluster_r1<8, true, true, true>), EXCLUSIVE_LDS) },
        { DEP_INSTANCE((gru_fwd_cluster_r1<16, false, true, true>), EXCLUSIVE_LDS), DEP_INSTANCE((gru_fwd_cluster_r1<16, true, true, true>), EXCLUSIVE_LDS) } };
    return (rag ? bidir_ragged : bidir)[H == 64 ? 0 : H == 128 ? 1 : H == 256 ? 2 : 3][split];
}

// NTW = H / 64.  Burst length 4 up to H = 256; H = 512 keeps the round-1 schedule (KB = 0): 192 weight registers per
// compute wave leave no room for a second wave per SIMD.  H = 256 with split products: the all-gather exchange of the members' gate
// gradients (round 5); every other shape / the exact-fp32 mode: the reduce-scatter of fp32 partial dh.  The last 2048 bytes of a
// launch's LDS hold the trace stamps.
constexpr int bwd_burst(int H) { return H >= 512 ? 0 : 4; }
Instance<P2>& bwd_instance(int H, bool split, bool sv16, bool bf16st, bool rag) {
    constexpr size_t R1 = EXCLUSIVE_LDS + 2048, AG = burst_lds_bytes_ag(4) + 2048;
    constexpr size_t BURST = (burst_lds_bytes(4) > EXCLUSIVE_LDS ? burst_lds_bytes(4) : EXCLUSIVE_LDS) + 2048;
    // per H: exact fp32 | split products, 16-bit saved gates | split products
    static Instance<P2> h64[3] = { DEP_INSTANCE((gru_bwd_cluster_r1<1, false, 4, false>), BURST), DEP_INSTANCE((gru_bwd_cluster_r1<1, true, 4, true>), BURST),
                                   DEP_INSTANCE((gru_bwd_cluster_r1<1, true, 4, false>), BURST) };
    static Instance<P2> h128[3] = { DEP_INSTANCE((gru_bwd_cluster_r1<2, false, 4, false>), BURST), DEP_INSTANCE((gru_bwd_cluster_r1<2, true, 4, true>), BURST),
                                    DEP_INSTANCE((gru_bwd_cluster_r1<2, true, 4, false>), BURST) };
    static Instance<P2> h256_exact DEP_INSTANCE((gru_bwd_cluster_r1<4, false, 4, false>), BURST);
    static Instance<P2> h512[3] = { DEP_INSTANCE((gru_bwd_cluster_r1<8, false, 0>), R1), DEP_INSTANCE((gru_bwd_cluster_r1<8, true, 0, true>), R1),
                                    DEP_INSTANCE((gru_bwd_cluster_r1<8, true, 0>), R1) };
    // H = 256, split products (all-gather): fp32 saved gates | 16-bit saved gates | 16-bit saved gates and bf16 storage
    static Instance<P2> h256_ag[3] = { DEP_INSTANCE((gru_bwd_cluster_r1<4, true, 4, false, false, true>), AG), DEP_INSTANCE((gru_bwd_cluster_r1<4, true, 4, true, false, true>), AG),
                                       DEP_INSTANCE((gru_bwd_cluster_r1<4, true, 4, true, true, true>), AG) };
    const int form = !split ? 0 : sv16 ? 1 : 2;
    if (rag) {      // the ragged-batch instances of the same forms (dep_rnn_backward_varlen; no bf16-storage variant: modes 2 / 3 refuse a ragged call)
        static Instance<P2> r64[3] = { DEP_INSTANCE((gru_bwd_cluster_r1<1, false, 4, false, false, false, true>), BURST), DEP_INSTANCE((gru_bwd_cluster_r1<1, true, 4, true, false, false, true>), BURST),
                                       DEP_INSTANCE((gru_bwd_cluster_r1<1, true, 4, false, false, false, true>), BURST) };
        static Instance<P2> r128[3] = { DEP_INSTANCE((gru_bwd_cluster_r1<2, false, 4, false, false, false, true>), BURST), DEP_INSTANCE((gru_bwd_cluster_r1<2, true, 4, true, false, false, true>), BURST),
                                        DEP_INSTANCE((gru_bwd_cluster_r1<2, true, 4, false, false, false, true>), BURST) };
        static Instance<P2> r256[3] = { DEP_INSTANCE((gru_bwd_cluster_r1<4, false, 4, false, false, false, true>), BURST), DEP_INSTANCE((gru_bwd_cluster_r1<4, true, 4, true, false, true, true>), AG),
                                        DEP_INSTANCE((gru_bwd_cluster_r1<4, true, 4, false, false, true, true>), AG) };
        static Instance<P2> r512[3] = { DEP_INSTANCE((gru_bwd_cluster_r1<8, false, 0, false, false, false, true>), R1), DEP_INSTANCE((gru_bwd_cluster_r1<8, true, 0, true, false, false, true>), R1),
                                        DEP_INSTANCE((gru_bwd_cluster_r1<8, true, 0, false, false, false, true>), R1) };
        return (H == 64 ? r64 : H == 128 ? r128 : H == 256 ? r256 : r512)[form];
    }
    switch (H) {
        case 64: return h64[form];
        case 128: return h128[form];
        case 256: return !split ? h256_exact : h256_ag[bf16st ? 2 : sv16 ? 1 : 0];
        default: return h512[form];
    }
}
// ... and the bidirectional instances (impl 7), dense and ragged: the unidirectional table's exchange form per H and mode, fp32 saved
// gates, fp32 gate-gradient rows.  Per H: exact fp32 | split products.
Instance<P2B>& bwd_bi_instance(int H, bool split, bool rag) {
    constexpr size_t R1 = EXCLUSIVE_LDS + 2048, AG = burst_lds_bytes_ag(4) + 2048;
    constexpr size_t BURST = (burst_lds_bytes(4) > EXCLUSIVE_LDS ? burst_lds_bytes(4) : EXCLUSIVE_LDS) + 2048;
    static Instance<P2B> bidir[4][2] = {
        { DEP_INSTANCE((gru_bwd_cluster_r1<1, false, 4, false, false, false, false, true>), BURST), DEP_INSTANCE((gru_bwd_cluster_r1<1, true, 4, false, false, false, false, true>), BURST) },
        { DEP_INSTANCE((gru_bwd_cluster_r1<2, false, 4, false, false, false, false, true>), BURST), DEP_INSTANCE((gru_bwd_cluster_r1<2, true, 4, false, false, false, false, true>), BURST) },
        { DEP_INSTANCE((gru_bwd_cluster_r1<4, false, 4, false, false, false, false, true>), BURST), DEP_INSTANCE((gru_bwd_cluster_r1<4, true, 4, false, false, true, false, true>), AG) },
        { DEP_INSTANCE((gru_bwd_cluster_r1<8, false, 0, false, false, false, false, true>), R1), DEP_INSTANCE((gru_bwd_cluster_r1<8, true, 0, false, false, false, false, true>), R1) } };
    static Instance<P2B> bidir_ragged[4][2] = {
        { DEP_INSTANCE((gru_bwd_cluster_r1<1, false, 4, false, false, false, true, true>), BURST), DEP_INSTANCE((gru_bwd_cluster_r1<1, true, 4, false, false, false, true, true>), BURST) },
        { DEP_INSTANCE((gru_bwd_cluster_r1<2, false, 4, false, false, false, true, true>), BURST), DEP_INSTANCE((gru_bwd_cluster_r1<2, true, 4, false, false, false, true, true>), BURST) },
        { DEP_INSTANCE((gru_bwd_cluster_r1<4, false, 4, false, false, false, true, true>), BURST), DEP_INSTANCE((gru_bwd_cluster_r1<4, true, 4, false, false, true, true, true>), AG) },
        { DEP_INSTANCE((gru_bwd_cluster_r1<8, false, 0, false, false, false, true, true>), R1), DEP_INSTANCE((gru_bwd_cluster_r1<8, true, 0, false, false, false, true, true>), R1) } };
    return (rag ? bidir_ragged : bidir)[H == 64 ? 0 : H == 128 ? 1 : H == 256 ? 2 : 3][split];
}
}  // namespace

void dep_cluster_gru_instance_texts(dep_instance_sink add) {
    const int sizes[] = {64, 128, 256, 512};       // dep_cluster_ok
    for (const int H : sizes)
        for (int m = 0; m < 16; ++m) {
            if (m < 4) { add(fwd_instance(H, m & 1, m & 2).text); add(fwd_bi_instance(H, m & 1, m & 2).text); add(bwd_bi_instance(H, m & 1, m & 2).text); }
            add(bwd_instance(H, m & 1, m & 2, m & 4, m & 8).text);
        }
}

// (H x 3H recurrent / input weight) -> forward (bwd[k] = 0) or backward (1) split image, up to 8 jobs in one launch
int dep_pack_cluster_split_multi(int n, const float* const* src, float* const* dst, const int* bwd, int H, hipStream_t s) {
    DEP_CHECK_ARG(n > 0 && n <= 8 && src && dst && bwd);
    PackJobs j{};
    j.n = n;
    for (int k = 0; k < n; ++k) { DEP_CHECK_ARG(src[k] && dst[k]); j.src[k] = src[k]; j.dst[k] = (u32x4*)dst[k]; j.bwd[k] = bwd[k]; }
    const long nf = pack_fwd_split_pieces(3, H), nb = pack_bwd_split_pieces(3, H);
    DEP_LAUNCH(pack_cluster_split_multi_kernel, dim3(dep_cdiv(nf > nb ? nf : nb, 256), n), dim3(256), 0, s, j, H);
    DEP_CHECK_LAUNCH();
    return DEP_OK;
}

int dep_pack_cluster_fwd_split(const float* w_hh, float* out, int H, hipStream_t s) {
    DEP_LAUNCH(pack_cluster_fwd_split_kernel, dim3(dep_cdiv(pack_fwd_split_pieces(3, H), 256)), dim3(256), 0, s, w_hh, (u32x4*)out, H);
    DEP_CHECK_LAUNCH();
    return DEP_OK;
}

int dep_pack_cluster_bwd_split(const float* w_hh, float* out, int H, hipStream_t s) {
    DEP_LAUNCH(pack_cluster_bwd_split_kernel, dim3(dep_cdiv(pack_bwd_split_pieces(3, H), 256)), dim3(256), 0, s, w_hh, (u32x4*)out, H);
    DEP_CHECK_LAUNCH();
    return DEP_OK;
}

int dep_launch_cluster_fwd(const dep_sweep_args& a, void* xbuf, size_t xbuf_bytes) {
    DEP_CHECK_ARG(dep_cluster_ok(a.cell, a.H, a.B, a.dirs) && xbuf && xbuf_bytes >= dep_cluster_xbuf_bytes(a.cell, a.H, a.B, a.dirs));
    DEP_CHECK_ARG(a.dirs == 1 || a.dirs == 2);
    const bool bi = a.dirs == 2;                           // both directions in one launch: a (direction, tile) pair per cluster
    // one workgroup per CU: 256 / NC tiles per launch (bidirectional: per direction half as many), larger batches in chunks
    const ChunkGeometry g = bi ? gru32_bi_geometry(a.H, a.B) : gru32_geometry(a.H, a.B);
    F2B p{};
    p.B = a.B; p.T = a.T; p.H = a.H;
    p.wp = (const f32x4*)a.wp[0]; p.b_hh = a.b_hh[0];
    p.wp1 = (const f32x4*)a.wp[1]; p.b_hh1 = a.b_hh[1]; p.ldsv = a.dirs * a.H;
    DEP_CHECK_ARG(!bi || (a.wp[1] && a.b_hh[1] && !a.only_if && !a.sv16 && a.ldy == 2 * a.H));
    p.gi = a.gi; p.ldgi = a.dirs * 3 * a.H; p.y = a.y; p.ldy = a.ldy;
    p.ydrop = (a.drop_p > 0.f) ? a.ydrop : nullptr;
    p.drop_p = a.drop_p; p.drop_scale = a.drop_p > 0.f ? 1.0f / (1.0f - a.drop_p) : 1.0f; p.seed = a.seed; p.site = a.site;
    p.pooled = a.pooled; p.pool_scale = a.pool_scale; p.h_n = a.h_n;
    p.sv0 = a.training ? a.sv0 : nullptr; p.sv1 = a.sv1; p.sv2 = a.sv2; p.sv3 = a.sv3;
    const size_t pay = bi ? gru_fwd_bi_payload_bytes(g, a.H) : gru_fwd_payload_bytes(g, a.H);
    DEP_CHECK_ARG(PAYLOAD_OFF + pay <= xbuf_bytes && g.resident());
    p.flags = bind_exchange(p, xbuf, a.hdr_slot, pay);
    p.only_if = a.only_if; p.sv16 = a.training ? a.sv16 : 0;
    p.lengths = a.lengths; p.pool_mean = a.pool_mean;
    DEP_CHECK_ARG(!a.hx || (!a.only_if && (reinterpret_cast<uintptr_t>(a.hx) & 7) == 0));      // a state never travels with the fused forward's fallback; 8-byte loads
    p.hx = a.hx;
    DepProfScope prof(DEP_PROF_GRU_FWD, a.stream, a.only_if == nullptr);     // a conditional fallback launch is not a sweep of the step
    const auto prepare = [&](int b0) { return hdr_prepare(xbuf, a.hdr_slot, a.hdr_clean && b0 == 0, a.stream); };
    if (bi) return launch_chunks(fwd_bi_instance(a.H, a.split, a.lengths != nullptr), g, dim3(CT), p, a.stream, __PRETTY_FUNCTION__, prepare);
    return launch_chunks(fwd_instance(a.H, a.split, a.lengths != nullptr), g, dim3(CT), static_cast<F2&>(p), a.stream, __PRETTY_FUNCTION__, prepare);
}

// May dep_launch_cluster_bwd write the gate gradients as the PK image (dep_sweep_bwd_args.dg_pk)?  Needs the burst-stream kernel
// (its service waves' flush forms the pairs), i.e. H <= 256, and whole step pairs.
bool dep_cluster_bwd_pk_ok(int H, int T) { return H <= 256 && T % 2 == 0; }

// dirs = 2 (impl 7): the bidirectional instances, both directions of a batch chunk in one launch -- the forward's pair geometry, the
// backward's payload per (direction, tile) pair.  They have fp32 saved gates and fp32 gate-gradient rows only.
size_t dep_cluster_bwd_bi_xbuf_bytes(int H, int B) {
    if (!dep_cluster_ok(DEP_CELL_GRU, H, B, 2)) return 0;
    return PAYLOAD_OFF + gru_bwd_payload_bytes(gru32_bi_geometry(H, B), H);
}

int dep_launch_cluster_bwd(const dep_sweep_bwd_args& a, void* xbuf, size_t xbuf_bytes) {
    DEP_CHECK_ARG(a.dirs == 1 || a.dirs == 2);
    const bool bi = a.dirs == 2;
    DEP_CHECK_ARG(dep_cluster_ok(a.cell, a.H, a.B, a.dirs) && xbuf &&
                  xbuf_bytes >= (bi ? dep_cluster_bwd_bi_xbuf_bytes(a.H, a.B) : dep_cluster_xbuf_bytes(a.cell, a.H, a.B, a.dirs)));
    DEP_CHECK_ARG(!bi || (!a.dg_pk && !a.sv16 && !a.bf16st));      // refused before any launch
    const ChunkGeometry g = bi ? gru32_bi_geometry(a.H, a.B) : gru32_geometry(a.H, a.B);
    const int nbt = dep_cdiv(a.B, BT);
    P2B p{};
    p.B = a.B; p.T = a.T; p.H = a.H;
    p.wp = (const f32x4*)a.wpT[0];
    p.wp1 = (const f32x4*)a.wpT[1]; p.ldsv = a.dirs * a.H; p.nbt = nbt;
    DEP_CHECK_ARG(!bi || (a.wpT[1] && a.ldy == 2 * a.H && a.lddy == 2 * a.H));
    p.y = a.y; p.ldy = a.ldy; p.dy = a.dy; p.lddy = a.lddy;
    p.drop_p = a.dy ? a.drop_p : 0.f; p.drop_scale = a.drop_p > 0.f ? 1.0f / (1.0f - a.drop_p) : 1.0f;
    p.seed = a.seed; p.site = a.site;
    p.dpooled = a.dpooled; p.pool_scale = a.pool_scale; p.dh_n = a.dh_n;
    p.sv0 = a.sv0; p.sv1 = a.sv1; p.sv2 = a.sv2; p.sv3 = a.sv3;
    p.dgi = a.dgi; p.lddg = a.lddg ? a.lddg : a.dirs * 3 * a.H; p.dghn = a.dghn; p.lddghn = a.lddghn ? a.lddghn : a.dirs * a.H; p.dbpart = a.dbpart;
    DEP_CHECK_ARG(!bi || (p.lddg >= 6 * a.H && p.lddghn >= 2 * a.H));
    p.dgpk = a.dg_pk;
    p.lengths = a.lengths; p.pool_mean = a.pool_mean;
    p.hx = a.hx; p.dhx = a.dhx;
    DEP_CHECK_ARG(!a.hx || (reinterpret_cast<uintptr_t>(a.hx) & 15) == 0);      // the service waves read 16-byte pieces of it
    DEP_CHECK_ARG(!a.dhx || (reinterpret_cast<uintptr_t>(a.dhx) & 7) == 0);
    DEP_CHECK_ARG(!((a.hx || a.dhx) && a.bf16st));   // the bf16-storage instance takes no state
    DEP_CHECK_ARG(!(a.lengths && a.bf16st));         // no ragged bf16-storage instance
    DEP_CHECK_ARG(!a.sv16 || a.split);               // the 16-bit saved gates exist in split-precision mode only
    DEP_CHECK_ARG(!a.bf16st || (a.H == 256 && a.split && a.sv16 && a.dg_pk));      // bf16-storage mode: H = 256, burst kernel (checked below via dg_pk)
    DEP_CHECK_ARG(a.dbpart_rows >= a.dirs * nbt);
    const size_t pay = gru_bwd_payload_bytes(g, a.H);      // (the pair geometry counts both directions' members)
    DEP_CHECK_ARG(PAYLOAD_OFF + pay <= xbuf_bytes && g.resident());
    p.flags = bind_exchange(p, xbuf, a.hdr_slot, pay);
    DepProfScope prof(DEP_PROF_GRU_BWD, a.stream);
    // (one tile's rows of the widest array must fit a 32-bit buffer offset)
    { const int mxl = p.lddg > p.lddy ? p.lddg : p.lddy; DEP_CHECK_ARG((size_t)(BT * a.T + 1) * (mxl > p.ldy ? mxl : p.ldy) * 4 < 0xffffffffull); }
    const int kb = bwd_burst(a.H);
    const auto prepare = [&](int b0) { return hdr_prepare(xbuf, a.hdr_slot, a.hdr_clean && b0 == 0, a.stream); };
    if (bi) {
        Instance<P2B>& k2 = bwd_bi_instance(a.H, a.split, a.lengths != nullptr);
        p.trall_off = (int)((k2.lds - 2048) / 4);
        return launch_chunks(k2, g, dim3(kb ? CT + SVC_THREADS : CT), p, a.stream, __PRETTY_FUNCTION__, prepare);
    }
    Instance<P2>& k = bwd_instance(a.H, a.split, a.sv16, a.bf16st, a.lengths != nullptr);
    p.trall_off = (int)((k.lds - 2048) / 4);
    if (p.dgpk) {       // the PK image needs the burst kernel's flush, the 4H-wide rows and whole step pairs (dep_cluster_bwd_pk_ok)
        DEP_CHECK_ARG(kb == 4 && a.split && a.T % 2 == 0 && a.lddg == 4 * a.H && a.lddghn == 4 * a.H && a.dghn == a.dgi + 3 * a.H);
    }
    return launch_chunks(k, g, dim3(kb ? CT + SVC_THREADS : CT), static_cast<P2&>(p), a.stream, __PRETTY_FUNCTION__, prepare);
}
