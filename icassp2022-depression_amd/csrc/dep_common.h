// Internal helpers shared by the gfx950 kernels of libdep_rnn.so (not part of the C-ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/dep_rnn.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

void dep_set_error(const char* fmt, ...);

#define DEP_CHECK_ARG(cond)                                                          \
    do {                                                                             \
        if (!(cond)) {                                                               \
            dep_set_error("%s:%d: bad argument: %s", __FILE__, __LINE__, #cond);     \
            return DEP_ERR_ARG;                                                      \
        }                                                                            \
    } while (0)

#define DEP_CHECK_LAUNCH()                                                           \
    do {                                                                             \
        hipError_t e__ = hipGetLastError();                                          \
        if (e__ != hipSuccess) {                                                     \
            dep_set_error("%s:%d: HIP: %s", __FILE__, __LINE__, hipGetErrorString(e__)); \
            return DEP_ERR_HIP;                                                      \
        }                                                                            \
    } while (0)

static inline size_t dep_align(size_t x, size_t a = 256) { return (x + a - 1) / a * a; }
static inline int dep_cdiv(long a, long b) { return (int)((a + b - 1) / b); }

// ---- device math ------------------------------------------------------------------
__device__ __forceinline__ float dep_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// ---- Philox4x32-10 counter-based RNG (dropout masks) --------------------------------
// key = seed ; counter = (group index lo, hi, site, 0).  One call yields the 4 uniforms of the
// 4-element group `g4` (element indices 4*g4 .. 4*g4+3) of dropout site `site`.
__device__ __forceinline__ void dep_philox4(uint64_t seed, uint32_t site, uint64_t g4, uint32_t (&r)[4]) {
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    uint32_t c0 = (uint32_t)g4, c1 = (uint32_t)(g4 >> 32), c2 = site, c3 = 0x2545F491u;
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        const uint32_t n0 = hi1 ^ c1 ^ k0, n1 = lo1, n2 = hi0 ^ c3 ^ k1, n3 = lo0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    r[0] = c0; r[1] = c1; r[2] = c2; r[3] = c3;
}
// pre-scaled keep mask (0 or 1/(1-p)) for the 4 elements of group g4
__device__ __forceinline__ f32x4 dep_dropmask4(uint64_t seed, uint32_t site, uint64_t g4, float p, float scale) {
    uint32_t r[4];
    dep_philox4(seed, site, g4, r);
    f32x4 m;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float u = (float)(r[i] >> 8) * (1.0f / 16777216.0f);   // [0,1)
        m[i] = (u >= p) ? scale : 0.0f;
    }
    return m;
}
__device__ __forceinline__ float dep_dropmask1(uint64_t seed, uint32_t site, uint64_t idx, float p, float scale) {
    const f32x4 m = dep_dropmask4(seed, site, idx >> 2, p, scale);
    return m[idx & 3];
}

// ---- ragged batches (dep_rnn_*_varlen, include/dep_rnn.h) ---------------------------------------------
// Row b's length as the kernels use it: clamped to [0, T] on the device (the host never sees the values).
__device__ __forceinline__ int dep_row_len(const int* lengths, int b, int T) { const int n = lengths[b]; return n < 0 ? 0 : (n > T ? T : n); }
// Pool scale of a ragged row: 1 / len for the mean (the dense call's own 1 / T when len == T, so that a ragged call with
// every length T reproduces the dense call's bits; 0 for an empty row, which divides by nothing), 1 for the sum.
__device__ __forceinline__ float dep_ragged_pool_scale(int pool_mean, int len, int T, float dense_scale) {
    return !pool_mean ? 1.0f : len == T ? dense_scale : len > 0 ? 1.0f / (float)len : 0.f;
}
__device__ __forceinline__ float2 dep_sel2(bool c, float2 a, float2 b) { return make_float2(c ? a.x : b.x, c ? a.y : b.y); }
__device__ __forceinline__ f32x4 dep_sel4(bool c, f32x4 a, f32x4 b) { f32x4 r = {c ? a[0] : b[0], c ? a[1] : b[1], c ? a[2] : b[2], c ? a[3] : b[3]}; return r; }

// DEP_FP_CONTRACT_NOTE.  The forward sweeps that have a ragged instance (gru_fwd_mfma<JPW, RAG>, lstm_fwd_mfma<JPW, RAG>, gru_fwd_generic<RAG>
// of rnn_sweep.hip, gru_fwd_cluster_r1<KCH, SPLIT, RAG> of rnn_cluster_bwd.hip, lstm_fwd_cluster<SPLIT, SV16, RAG> of rnn_cluster_lstm.hip) open with `#pragma clang fp contract(on)`: a * b + c written in ONE expression is one fma (the product on the left
// of the sum is the fused one) and nothing else is fused.  Under the default (contract = fast) the backend decides, and its choice
// depends on what surrounds the expression -- the selects of a ragged instance, or a neighbouring product the vectoriser pairs it
// with -- so the dense and the ragged instance of one kernel rounded differently; a ragged call whose lengths all equal T must reproduce
// the dense call's bits (tests/test_varlen_gpu.py).  The expressions are written so that the dense instances keep the operations the
// backend chose before (h = z * h_prev + (1 - z) * n: the fused product first).  To re-verify after a compiler change: run
// `tools/isa_diff.py <csrc file> <the commit before the pragma>` (it compiles both sides with the build's flags and prints, per kernel,
// `identical` or the first differing lines) and compare the dense instances' v_fma / v_mul / v_add / v_pk_* instructions (same multiset;
// operands of a product may swap); tests/golden/device_bits.json (tests/test_presplit_gpu.py) anchors the results on the device.  The backward sweeps keep the default: there the ragged instances
// select on final results only (the split words, the summed dh), which leaves the arithmetic of a live step as the dense instance has it.

// dropout sites (Philox counter word 2): distinct per place a mask is drawn in one step
enum { DEP_SITE_RNN0 = 16 /* + layer */, DEP_SITE_USER = 0 };

// ---- XCD-aware tile order -----------------------------------------------------------------------
// Blocks are dispatched round-robin over the 8 XCDs (block b -> XCD b % 8, observed, speed only).  Remap the
// linear block id so that every XCD walks a contiguous run of the (x fastest, y, z) tile order: neighbouring
// tiles share an operand panel and now hit the same 4 MB L2 instead of refetching it on 6-8 different XCDs.
// Bijective for any block count (cdna_hip_programming.md T1).
__device__ __forceinline__ void dep_xcd_tile(int gx, int gy, int gz, int& bx, int& by, int& bz) {
    const int n = gx * gy * gz, orig = blockIdx.x;
    const int q = n / 8, r = n % 8, xcd = orig % 8;
    const int id = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + orig / 8;
    bx = id % gx; by = (id / gx) % gy; bz = id / (gx * gy);
}

// ---- launch-instance log (dep_instance_log_*, include/dep_rnn.h) ------------------------------------
// Every kernel launch of the library goes through DEP_LAUNCH: while the log is on it records the kernel expression as written at the
// launch site plus the enclosing function's signature (which carries the template arguments of templated launchers), once per distinct
// pair.  tests/test_step_coverage_gpu.py uses it to tie the template instances a bench.py step launches to the ones the
// oracle-comparing tests launched.  Off (the default): one relaxed atomic load per launch.
bool dep_ilog_on();
void dep_ilog_note(const char* kern, const char* where);
// (dep_order_log_*: the same hook also appends "K <kernel>" to the enqueue-order log while that is on; collectives add "C ..." in comm.hip)
void dep_olog_add(char kind, const char* text, long n);
#define DEP_LAUNCH(kern, grid, blk, lds, stream, ...)                                          \
    do {                                                                                       \
        if (dep_ilog_on()) dep_ilog_note(#kern, __PRETTY_FUNCTION__);                          \
        hipLaunchKernelGGL(kern, grid, blk, lds, stream, __VA_ARGS__);                         \
    } while (0)

// ---- optional per-kernel timing with HIP events on the launch stream (bench.py roofline leg) ----
enum { DEP_PROF_GRU_FWD = 0, DEP_PROF_GRU_BWD = 1, DEP_PROF_LSTM_FWD = 2, DEP_PROF_LSTM_BWD = 3,
       DEP_PROF_GEMM_NT = 4, DEP_PROF_GEMM_NN = 5, DEP_PROF_GEMM_TN = 6, DEP_PROF_NCAT = 7 };
// ---- GEMM call options (gemm.hip, gemm_bf16x3.hip) ----------------------------------------------------------------
// Operand storage formats of the split-precision kernel (gemm_bf16x3.hip describes them); its FMT template parameters take these values.
enum { FMT_F32 = 0, FMT_PK = 1, FMT_PKH = 2, FMT_BF16 = 3 };
enum { DEP_PREC_MODE = 0, DEP_PREC_EXACT = 1, DEP_PREC_X3 = 2 };
// Everything a contraction takes besides its operands.  The default value is the plain call: fp32 operands, precision by dep_set_gemm_mode.
struct DepGemmOpts {
    int prec = DEP_PREC_MODE;            // follow the mode | exact fp32 | three-term bf16x3 whatever the mode
    int fmt_a = FMT_F32, fmt_b = FMT_F32;    // anything but FMT_F32 needs the split kernel: dep_gemm_internal refuses it elsewhere
    int skip_at = 0, skip_by = 0;        // TN A operand (split kernel only): logical column m is stored at m + (m >= skip_at ? skip_by : 0)
    long split_target = 0;               // split-K target in 128x128 tile-chunks (0 = DEP_GEMM_SPLIT_TARGET, default 1024)
    const unsigned* only_if = nullptr;   // the launches return at kernel entry unless this device word is non-zero
    void* scratch = nullptr; size_t scratch_bytes = 0;      // unsplit calls without a workspace: room for the DMA kernels' weight image
};
// The DEP_GEMM_* / DEP_DW_PAIR switches, read once per process.
struct DepGemmSwitches {
    int mode;                 // DEP_GEMM_MODE: initial precision mode (dep_set_gemm_mode changes it)
    bool naive, pair, tn_dma, nt_dma, bm256, nt256;
    long split_target;
    int ablate, persist;
};
const DepGemmSwitches& dep_gemm_switches();
bool dep_gemm_bf16x3_pair_ok();
// true when dep_gemm_internal would run the split kernel for a plain contraction of this size (the one that reads PK and honours the skip)
bool dep_gemm_uses_bf16x3(int M, int N, int K, int seq_T);
// two TN contractions of equal shape over PK A operands in one launch (gemm.hip), the column skip on problem 1: 1 = enqueued, 0 = not covered, < 0 = error
int dep_gemm_tn_pair(int M, int N, int K, const float* A0, const float* A1, int lda,
                     const float* B0, int ldb0, int seq_T0, int shift0, const float* B1, int ldb1, int seq_T1, int shift1,
                     float* C0, int ldc0, float* C1, int ldc1, const DepGemmOpts& o, void* ws, size_t ws_bytes, hipStream_t s);
int dep_gemm_bf16x3_tn_pair_launch(int M, int N, int K, const float* A0, const float* A1, int lda,
                                   const float* B0, int ldb0, int seq_T0, int shift0, const float* B1, int ldb1, int seq_T1, int shift1,
                                   float* C0, int ldc0, float* C1, int ldc1, const DepGemmOpts& o, int splits, int kchunk, float* part0, float* part1,
                                   hipStream_t s);
// The switches of the RNN call path, read once per process.
struct RnnSwitches {
    bool sv16, lstm_sv16;             // DEP_SV16 (default on), DEP_LSTM_SV16 (opt-in, rnn_cluster_lstm.hip): 16-bit saved gates
    bool fused2, fused2_bwd;          // DEP_FUSED2, DEP_FUSED2_BWD ("1" on, anything else off, unset: DEP_FUSED2_BWD_DEFAULT)
    bool cluster16, cluster_lstm;     // DEP_CLUSTER16, DEP_CLUSTER_LSTM
    bool dgi_pk;                      // DEP_DGI_PK: gate gradients as the PK image where the contractions take it
    bool comm_beside_sweeps;          // DEP_COMM_OVERLAP=sweep
    bool exclusive;                   // DEP_EXCLUSIVE: initial value (dep_rnn_set_exclusive changes it)
};
const RnnSwitches& dep_rnn_switches();
bool dep_prof_on();
void dep_prof_begin(int cat, hipStream_t s);
void dep_prof_end(hipStream_t s);
struct DepProfScope {
    hipStream_t s; bool on;
    DepProfScope(int cat, hipStream_t st, bool enable = true) : s(st), on(enable && dep_prof_on()) { if (on) dep_prof_begin(cat, s); }
    ~DepProfScope() { if (on) dep_prof_end(s); }
};

// ---- internal launchers shared across translation units ---------------------------
struct dep_sweep_args {
    int B, T, H;
    int cell, dirs;          // dirs = 2: both directions in one launch (GRU: the tile-MFMA sweeps of rnn_sweep.hip, and dep_launch_cluster_fwd for impl 6)
    int training;
    int impl;
    // per direction d
    const float* w_hh[2];    // (G*H, H) row-major
    const float* b_hh[2];    // (G*H)  GRU only, per direction (LSTM biases are folded into GI by the GEMM)
    const float* wp[2];      // packed fragment-order copies (MFMA path), see pack kernels
    int split;               // cluster sweeps: recurrent product on the bf16 matrix cores (3-term split), wp packed to match
    // activations
    const float* gi;         // (B,T,dirs*G*H): input projection incl. bias_ih (LSTM: + bias_hh)
    float* y;  int ldy;      // (B,T,ldy) hidden sequence; direction d writes columns [d*H,(d+1)*H)
    float* ydrop;            // same layout: dropout(y) for the next layer, or NULL
    float drop_p; uint64_t seed; uint32_t site;
    float* pooled; float pool_scale;    // GRU top layer: (B,dirs*H) sum_t y_t * scale, or NULL
    float* h_n;              // (dirs,B,H) final states or NULL
    // initial state of this layer (dep_rnn_forward_state[_varlen]; rnn_sweep.hip, and hx alone on dep_launch_cluster_fwd for an impl 4 / 5 / 6
    // descriptor -- the other cluster launchers are never given one)
    const float* hx;         // (dirs,B,H) h before the sweep's first step, or NULL = zeros; may be h_n's buffer
    const float* cx;         // LSTM: (dirs,B,H) c before the first step, or NULL = zeros; may be c_n's buffer
    float* c_n;              // LSTM: (dirs,B,H) c after the last step, or NULL
    // reserve (training): GRU r,z,n,hn each (B,T,dirs*H) ; LSTM gates (B,T,dirs*4H) + c (B,T,dirs*H)
    float* sv0; float* sv1; float* sv2; float* sv3;
    const unsigned* only_if;  // cluster forward: run only when this device word is non-zero (fallback behind an exclusive kernel), or NULL
    int sv16;                 // GRU cluster sweeps: sv0..sv2 (r, z, n) are 16-bit fixed point (rnn_cluster_common.h), sv3 (hn) stays fp32
    int hdr_slot, hdr_clean;  // cluster sweeps: exchange-header slot of this launch; clean = the caller zeroed it (rnn_cluster_common.h)
    const int* lengths;       // ragged call: (B) int32 device array, row b is live for t < lengths[b]; NULL = dense (the dense instances)
    int pool_mean;            // ragged call: the pool is a mean (scale 1 / lengths[b]), not a sum
    hipStream_t stream;
};
int dep_launch_sweep_fwd(const dep_sweep_args& a);

struct dep_sweep_bwd_args {
    int B, T, H;
    int cell, dirs;          // dirs = 2: both directions in one launch (GRU: the tile-MFMA sweeps of rnn_sweep.hip, and dep_launch_cluster_bwd for impl 7)
    int impl;
    const float* w_hh[2];
    const float* wpT[2];     // packed transposed copies (MFMA path)
    int split;               // GRU cluster sweep: dgates W_hh on the bf16 matrix cores (3-term split), wpT packed to match
    const float* y; int ldy; // forward hidden sequence of this layer (h_{t-1} operand)
    const float* dy; int lddy;           // (B,T,lddy) grad of y (columns [d*H,(d+1)*H) per direction) or NULL
    float drop_p; uint64_t seed; uint32_t site;   // dropout applied to dy on load (p == 0: none)
    const float* dpooled; float pool_scale;       // GRU top layer (B,dirs*H) or NULL
    const float* dh_n;       // (dirs,B,H) or NULL
    // state of this layer (dep_rnn_backward_state[_varlen]; rnn_sweep.hip, and hx / dhx on dep_launch_cluster_bwd for impl 5 / 7): what the forward started from, and the state gradients
    const float* hx; const float* cx;     // (dirs,B,H) the forward's initial h / c (LSTM), or NULL = zeros
    const float* dc_n;       // LSTM: (dirs,B,H) grad of c_n, enters where dh_n enters, or NULL
    float* dhx; float* dcx;  // (dirs,B,H) grad of hx / cx (LSTM), WRITTEN, or NULL
    const float* sv0; const float* sv1; const float* sv2; const float* sv3;
    float* dgi;              // (B,T,dirs*G*H) written: grad of the input projection
    float* dghn;             // GRU: (B,T,dirs*H) grad of the n-gate recurrent pre-activation (dn*r)
    int lddg, lddghn;        // row strides of dgi / dghn (0 = packed: dirs*G*H and dirs*H).  The GRU cluster sweep accepts 4H / 4H with
                             // dghn = dgi + 3H: one (B,T,4H) array [dr | dz | dn | dn*r], so that dW_hh is ONE contraction
    float* dbpart;           // partial bias sums, see dep_sweep_dbpart_floats
    int dbpart_rows;         // number of partial rows provided
    int hdr_slot, hdr_clean; // cluster sweeps: exchange-header slot of this launch; clean = the caller zeroed it
    int sv16;                // saved gates r, z, n are 16-bit fixed point (must match the forward that wrote them)
    int dg_pk;               // GRU cluster sweep (burst kernel, 4H-wide rows): dgi / dghn as the PK image of gemm_bf16x3.hip instead of fp32
    int bf16st;              // bf16-storage mode (dep_set_gemm_mode(3)): y and hn are bf16 arrays, the gate gradients the PKH image (hi rows only)
    const int* lengths;      // ragged call (the lengths of the forward that wrote the reserve), or NULL
    int pool_mean;           // ragged call: dpooled is the gradient of a mean (scaled by 1 / lengths[b])
    hipStream_t stream;
};
bool dep_cluster_bwd_pk_ok(int H, int T);
#define DEP_FUSED2_BWD_DEFAULT 1      /* both GRU layers' BPTT as one all-gather launch (rnn_fused2_bwd.hip); DEP_FUSED2_BWD overrides */
bool dep_cluster_lstm_bwd_pk_ok(int T);
bool dep_cluster_lstm_sv16_ok();
int dep_launch_sweep_bwd(const dep_sweep_bwd_args& a);
int dep_sweep_num_wg(int B, int H, int impl);       // batch tiles (rows of dbpart) per direction
bool dep_sweep_use_mfma(int H, int impl);

// packed weight sizes / kernels (MFMA path)
size_t dep_pack_floats(int G, int H);               // floats of one packed (G*H x H) matrix
int dep_pack_whh(const float* w_hh, float* wp, float* wpT, int G, int H, hipStream_t s);
// bias-gradient finish: sums partial rows
int dep_finish_db(const dep_sweep_bwd_args& a, float* const* db_ih, float* const* db_hh);
// ragged state call: dw_hh (M, H) += sum_{b : len_b > 0} dg[b, t0_b, :M]^T hx[b, :], t0_b = 0 or (reverse) len_b - 1; dg rows are lddg wide, T per batch row
int dep_state_dwhh_ragged(const float* dg, int lddg, const int* lengths, int B, int T, int reverse, const float* hx, int M, int H, float* dw_hh,
                          hipStream_t s);

// cluster-parallel sweeps (rnn_cluster.hip)
bool dep_cluster_ok(int cell, int H, int B, int dirs);
size_t dep_cluster_xbuf_bytes(int cell, int H, int B, int dirs);
size_t dep_cluster_bwd_bi_xbuf_bytes(int H, int B);      // rnn_cluster_bwd.hip: headers + the bidirectional backward's payload (impl 7; dirs = 2 above is the forward's alone)
int dep_pack_cluster_bwd(const float* w_hh, float* out, int G, int H, hipStream_t s);
int dep_launch_cluster_fwd(const dep_sweep_args& a, void* xbuf, size_t xbuf_bytes);
int dep_launch_cluster_bwd(const dep_sweep_bwd_args& a, void* xbuf, size_t xbuf_bytes);
bool dep_cluster16_ok(int cell, int H, int B);
bool dep_cluster_lstm_ok(int H, int B, int dirs);
size_t dep_cluster_lstm_xbuf_bytes(int H, int B, int dirs);
int dep_launch_cluster_lstm_fwd(const dep_sweep_args& a, void* xbuf, size_t xbuf_bytes);
int dep_launch_cluster_lstm_bwd(const dep_sweep_bwd_args& a, void* xbuf, size_t xbuf_bytes);
// Utterances one co-resident cluster launch may cover: `members` workgroups per 16-utterance tile, `per_cu` of them resident
// per CU (rnn_cluster.hip; CU count from the device, DEP_NUM_CUS overrides), at most `max_wgs` workgroups (flag words).
int dep_cluster_chunk(int members, int per_cu, int max_wgs);
// rnn_fused2.hip: both layers of a 2-layer GRU (H = 256) in one cluster launch, layer 1 one step behind layer 0
struct dep_fused2_args {
    int B, T, training;
    const float* wp0; const float* wp1; const float* wpi;   // packed W_hh l0, W_hh l1, W_ih l1 (dep_pack_cluster_fwd_split images)
    const float* b_hh0; const float* b_ih1; const float* b_hh1;
    const float* gi;                                          // layer-0 input projection incl. b_ih (B*T, 3H)
    float* y0; float* y0d; float* y1;
    size_t ostride;                                           // floats between consecutive per-layer arrays of the reserve
    float drop_p; uint64_t seed; uint32_t site;
    float* pooled; float pool_scale; float* hn0; float* hn1;
    float* sv[2][4];
    int sv16;                                                 // saved gates r, z, n as 16-bit fixed point (rnn_cluster_common.h)
    int bf16st;                                               // bf16-storage mode: h, dropout(h), hn are written as bf16 (2-byte elements at the same positions)
    int soft_fallback;                                        // 1: a failed hello sets the workspace's soft flag instead of the status word
    int hdr_clean;                                            // slot 0 was zeroed by the caller (dep_cluster_reset_status)
    hipStream_t stream;
};
bool dep_fused2_ok(int cell, int H, int L, int dirs);
size_t dep_fused2_xbuf_bytes(int B);
int dep_launch_fused2_fwd(const dep_fused2_args& a, void* xbuf, size_t xbuf_bytes);
// rnn_fused2_bwd.hip: BPTT of both layers in one cluster launch, layer 0 one step behind layer 1
struct dep_fused2_bwd_args {
    int B, T;
    const float* wh1; const float* wi1; const float* wh0;     // dep_pack_cluster_bwd_split images of W_hh l1, W_ih l1, W_hh l0
    const float* y1; const float* y0; const float* sv1; const float* sv0; size_t svstride;
    const float* dy; const float* dpooled; float pool_scale; const float* dhn1; const float* dhn0;
    float drop_p; uint64_t seed; uint32_t site;
    float* dgi1; float* dghn1; float* dgi0; float* dghn0; float* dbpart1; float* dbpart0; int dbpart_rows;
    int lddg, lddghn;        // row strides of dgi / dghn: 3H / H, or 4H / 4H with dghn = dgi + 3H (one (B*T, 4H) array [dr | dz | dn | dn*r] per layer)
    int sv16;                // saved gates r, z, n are 16-bit fixed point (must match the forward that wrote them)
    int bf16st;              // bf16-storage mode (dep_set_gemm_mode(3)): y and hn are bf16 arrays, the gate gradients the PKH image (needs sv16 and dg_pk)
    int dg_pk;               // dgi1 / dgi0 are (B*T, 4H) arrays [dr | dz | dn | dn*r] written as the PK image of gemm_bf16x3.hip (needs sv16, T even); dghn unused
    hipStream_t stream;
};
size_t dep_fused2_bwd_xbuf_bytes(int B);
bool dep_fused2_bwd_fits(int B, int T);       // 32-bit offsets into a layer's arrays: else the per-layer sweeps
int dep_launch_fused2_bwd(const dep_fused2_bwd_args& a, void* xbuf, size_t xbuf_bytes);
// comm.hip: all-reduce of [buf, buf+n) on comm_stream after everything enqueued so far on `compute`
int dep_comm_enqueue_after(dep_comm* c, float* buf, long n, hipStream_t compute, hipStream_t comm_stream);
// clears the sticky status word of a cluster exchange buffer (once per dep_rnn_forward; the sweeps themselves never clear it)
constexpr int DEP_HDR_SLOTS = 4;                              // exchange-header slots at the head of the buffer (rnn_cluster_common.h)
int dep_cluster_reset_status(void* xbuf, hipStream_t s);      // status, soft flag and EVERY header slot
int dep_cluster_reset_flags(void* xbuf, hipStream_t s);       // every header slot, status words kept (dep_rnn_backward)
int dep_pack_cluster16_fwd_split(const float* w_hh, float* out, int H, hipStream_t s);
int dep_pack_cluster_bwd_split(const float* w_hh, float* out, int H, hipStream_t s);
int dep_pack_cluster_split_multi(int n, const float* const* src, float* const* dst, const int* bwd, int H, hipStream_t s);
int dep_multi_copy(int count, const float* const* src, const float* const* add, float* const* dst, const long* n, hipStream_t s);
// attention.hip: the loads-in-flight attention kernels (H in {64,128,256,512}); 1 = launched, 0 = shape left to elementwise.hip's
int dep_attn2_fwd(const float* out, const float* pre, float* ctx, float* alpha, int B, int T, int H, const int* lengths, hipStream_t s);
int dep_attn2_bwd(const float* dctx, const float* out, const float* alpha, const float* pre, float* dout, float* dpre, int B,
                  int T, int H, const int* lengths, hipStream_t s);
int dep_pack_cluster_fwd_split(const float* w_hh, float* out, int H, hipStream_t s);
int dep_pack_cluster_lstm_split(const float* w_hh, float* wp, float* wpT, int H, hipStream_t s);
int dep_launch_cluster16_fwd(const dep_sweep_args& a, void* xbuf, size_t xbuf_bytes);
// rnn_local_lstm.hip: the exchange-free LSTM forward (impl 8 / 9; takes a.hx, a.cx, a.c_n and a.lengths, any batch in one launch; with
// a.training == DEP_RUN_TRAIN it also fills a.sv0 / a.sv1) and backward (impl 9; fp32 saved gates and gate-gradient rows, every state member)
bool dep_local_lstm_ok(int cell, int H, int dirs);
int dep_launch_local_lstm_fwd(const dep_sweep_args& a);
int dep_launch_local_lstm_bwd(const dep_sweep_bwd_args& a);
// dep_instance_table_read: each cluster-family file hands `add` the text of every row its selection functions can return (it calls
// them over their whole argument domain; duplicates are the caller's to drop).  Host only, no device call.
typedef void (*dep_instance_sink)(const char* text);
void dep_cluster_gru_instance_texts(dep_instance_sink add);       // rnn_cluster_bwd.hip: the per-layer GRU forward and backward
void dep_cluster16_instance_texts(dep_instance_sink add);         // rnn_cluster16.hip
void dep_cluster_lstm_instance_texts(dep_instance_sink add);      // rnn_cluster_lstm.hip
void dep_fused2_fwd_instance_texts(dep_instance_sink add);        // rnn_fused2.hip
void dep_fused2_bwd_instance_texts(dep_instance_sink add);        // rnn_fused2_bwd.hip
void dep_local_lstm_instance_texts(dep_instance_sink add);        // rnn_local_lstm.hip

int dep_gemm_internal(int transA, int transB, int M, int N, int K, const float* A, int lda,
                      const float* B, int ldb, float* C, int ldc, const float* bias, float beta,
                      int seq_T, int shiftB, void* ws, size_t ws_bytes, const DepGemmOpts& o, hipStream_t s);
