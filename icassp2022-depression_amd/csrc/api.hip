// C-ABI orchestration of the stacked GRU / BiLSTM operator (dep_rnn_forward / dep_rnn_backward):
// per layer  [pack W_hh] -> input-projection GEMM -> persistent sweep ; backward mirrors it.
// See include/dep_rnn.h for the contract and the reference call sites each entry replaces.
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>
#include <atomic>
#include <mutex>
#include <set>
#include <string>
#include <utility>
#include <vector>
#include "dep_common.h"

static thread_local char g_err[512] = "";

void dep_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" const char* dep_last_error(void) { return g_err; }
extern "C" int dep_version(void) { return 100; }
extern "C" const char* dep_arch(void) { return "gfx950"; }

// ---- event-based kernel timing -------------------------------------------------------
// Process-wide recorder, safe to use from several host threads / streams at once (SURVEY 8b "reentrant per stream"): the open
// begin/end pair is per thread, the event pool and the record list are guarded by one mutex (taken only while profiling is on).
namespace {
struct ProfRec { hipEvent_t a, b; int cat; };
std::atomic<bool> g_prof_on{false};
std::mutex g_prof_mu;
std::vector<ProfRec> g_recs;
std::vector<std::pair<hipEvent_t, hipEvent_t>> g_pool;
thread_local ProfRec g_cur;
}  // namespace
bool dep_prof_on() { return g_prof_on.load(std::memory_order_relaxed); }
void dep_prof_begin(int cat, hipStream_t s) {
    {
        std::lock_guard<std::mutex> lk(g_prof_mu);
        if (g_pool.empty()) {
            hipEvent_t a, b;
            (void)hipEventCreate(&a); (void)hipEventCreate(&b);
            g_pool.push_back({a, b});
        }
        g_cur.a = g_pool.back().first; g_cur.b = g_pool.back().second; g_cur.cat = cat;
        g_pool.pop_back();
    }
    (void)hipEventRecord(g_cur.a, s);
}
void dep_prof_end(hipStream_t s) {
    (void)hipEventRecord(g_cur.b, s);
    std::lock_guard<std::mutex> lk(g_prof_mu);
    g_recs.push_back(g_cur);
}
extern "C" int dep_profile_enable(int on) { g_prof_on.store(on != 0); return DEP_OK; }
// Sums the recorded launch durations per category (ms) and resets; blocks until the events completed.
extern "C" int dep_profile_read(double* total_ms, int* counts, int ncat) {
    for (int i = 0; i < ncat; ++i) { total_ms[i] = 0.0; counts[i] = 0; }
    std::vector<ProfRec> recs;
    { std::lock_guard<std::mutex> lk(g_prof_mu); recs.swap(g_recs); }
    for (auto& r : recs) {
        (void)hipEventSynchronize(r.b);
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, r.a, r.b);
        if (r.cat < ncat) { total_ms[r.cat] += ms; counts[r.cat] += 1; }
    }
    std::lock_guard<std::mutex> lk(g_prof_mu);
    for (auto& r : recs) g_pool.push_back({r.a, r.b});
    return DEP_OK;
}

// ---- launch-instance log (DEP_LAUNCH, dep_common.h) ------------------------------------------------
namespace {
std::atomic<bool> g_ilog_on{false};
std::mutex g_ilog_mu;
std::set<std::string> g_ilog;
}  // namespace
std::atomic<int> g_ilog_any{0};          // bit 0: instance log, bit 1: enqueue-order log (one relaxed load per launch when both are off)
bool dep_ilog_on() { return g_ilog_any.load(std::memory_order_relaxed) != 0; }
namespace { std::vector<std::string> g_olog; }
void dep_olog_add(char kind, const char* text, long n) {
    if (!(g_ilog_any.load(std::memory_order_relaxed) & 2)) return;
    std::string e(1, kind); e += ' '; e += text;
    if (n >= 0) { e += " n="; e += std::to_string(n); }
    std::lock_guard<std::mutex> lk(g_ilog_mu);
    g_olog.push_back(std::move(e));
}
extern "C" int dep_order_log_enable(int on) {
    std::lock_guard<std::mutex> lk(g_ilog_mu);
    if (on) { g_olog.clear(); g_ilog_any.fetch_or(2); } else g_ilog_any.fetch_and(~2);
    return DEP_OK;
}
extern "C" int dep_order_log_note(const char* text) { if (!text) return DEP_ERR_ARG; dep_olog_add('N', text, -1); return DEP_OK; }
extern "C" long dep_order_log_read(char* buf, long cap, int reset) {
    std::lock_guard<std::mutex> lk(g_ilog_mu);
    std::string all;
    for (const auto& s : g_olog) { all += s; all += '\n'; }
    if (buf && cap > 0) {
        const long n = (long)all.size() < cap - 1 ? (long)all.size() : cap - 1;
        memcpy(buf, all.data(), (size_t)n); buf[n] = 0;
    }
    if (reset) g_olog.clear();
    return (long)all.size() + 1;
}
void dep_ilog_note(const char* kern, const char* where) {
    dep_olog_add('K', kern, -1);
    if (!g_ilog_on.load(std::memory_order_relaxed)) return;
    std::string k(kern);
    // the kernel as written is enough when it names every template argument; launchers that are templates themselves
    // (kernel<TA, TB, ..>) are told apart by their own signature
    bool symbolic = false;
    for (size_t i = 0; i + 1 < k.size(); ++i)
        if ((k[i] == '<' || k[i] == ' ' ) && k[i + 1] >= 'A' && k[i + 1] <= 'Z') symbolic = true;
    if (symbolic) { k += " @ "; k += where; }
    std::lock_guard<std::mutex> lk(g_ilog_mu);
    g_ilog.insert(std::move(k));
}
extern "C" int dep_instance_log_enable(int on) {
    std::lock_guard<std::mutex> lk(g_ilog_mu);
    if (on) { g_ilog.clear(); g_ilog_any.fetch_or(1); } else g_ilog_any.fetch_and(~1);
    g_ilog_on.store(on != 0);
    return DEP_OK;
}
// Newline-separated distinct launch instances recorded so far -> buf (NUL-terminated, truncated to cap); returns the bytes the
// full list needs (incl. the NUL).  reset != 0 empties the log afterwards.
extern "C" long dep_instance_log_read(char* buf, long cap, int reset) {
    std::lock_guard<std::mutex> lk(g_ilog_mu);
    std::string all;
    for (const auto& s : g_ilog) { all += s; all += '\n'; }
    if (buf && cap > 0) {
        const long n = (long)all.size() < cap - 1 ? (long)all.size() : cap - 1;
        memcpy(buf, all.data(), (size_t)n); buf[n] = 0;
    }
    if (reset) g_ilog.clear();
    return (long)all.size() + 1;
}
// Newline-separated texts of every row of the cluster families' instance tables, as launch_chunks logs them (none of them is symbolic,
// so dep_ilog_note adds nothing to a row's text); buf, cap and the return value as dep_instance_log_read.  Needs no device.
extern "C" long dep_instance_table_read(char* buf, long cap) {
    static std::mutex mu;
    static std::set<std::string> rows;
    std::lock_guard<std::mutex> lk(mu);
    if (rows.empty()) {
        const dep_instance_sink add = [](const char* text) { rows.insert(text); };
        dep_cluster_gru_instance_texts(add); dep_cluster16_instance_texts(add); dep_cluster_lstm_instance_texts(add);
        dep_fused2_fwd_instance_texts(add); dep_fused2_bwd_instance_texts(add); dep_local_lstm_instance_texts(add);
    }
    std::string all;
    for (const auto& s : rows) { all += s; all += '\n'; }
    if (buf && cap > 0) {
        const long n = (long)all.size() < cap - 1 ? (long)all.size() : cap - 1;
        memcpy(buf, all.data(), (size_t)n); buf[n] = 0;
    }
    return (long)all.size() + 1;
}

namespace {

constexpr int MAXL = 8;
constexpr size_t NOT_KEPT = (size_t)-1;         // Layout offset of an array the run mode does not keep

// Sizes and offsets of a descriptor's reserve and workspace.  A function of the descriptor and the switches alone: the size queries
// answer the same whatever precision mode or exclusivity the calls run under (what a call runs is its RnnPlan, below).
struct Layout {
    int G, D, L;
    size_t BT;                       // B*T rows
    // reserve (float offsets)
    size_t y[MAXL], ydrop[MAXL], sv[MAXL][4], wp[MAXL][2], wpT[MAXL][2];
    size_t reserve_floats;
    // workspace (float offsets)
    size_t gi, dghn, dx[2], dbpart, biastmp, gemm, xbuf;
    size_t wstack[MAXL], bstack[MAXL], dwstack;   // bidirectional: both directions' W_ih / (b_ih + b_hh) stacked (2 G H x in), one dW_ih scratch
    size_t gi2, dghn2, dbpart2;      // second set of gate-gradient buffers: the fused backward keeps both layers' dgi / dghn
    size_t gemm_bytes, xbuf_bytes, ws_floats;
    int nwg;
    bool drop;
    bool keep;                       // DEP_RUN_TRAIN: the reserve holds everything the backward reads
    bool donly;                      // DEP_RUN_DROPOUT_ONLY: dropout as in training, the reserve holds what the forward itself reads
    bool cluster;                    // cluster-parallel sweeps (rnn_cluster*.hip): the workspace has their exchange buffer
    bool cluster_fwd;                // impl 6: the FORWARD alone runs on the cluster (a bidirectional GRU); the workspace has its exchange buffer, and
                                     // nothing else of `cluster` holds: the backward, its weight images, bias partials and gate gradients are the tile sweeps'
    bool cluster_bwd2;               // impl 7: ... and the BACKWARD too, on the bidirectional instances of gru_bwd_cluster_r1: the exchange buffer covers its
                                     // payload, the bias partials are one row per (direction, tile), wpT holds the cluster backward's images
    bool fused2;                     // 2-layer GRU, H = 256: both layers in one launch (rnn_fused2*.hip) where the call's plan allows it
    size_t wih_img;                  // workspace: packed W_ih of layer 1 for the fused launches
    size_t hxstage;                  // workspace (impl 4 / 5 / 6 only): dirs x B x H floats, a layer's hx copied aside when T = 1 and h_n overlaps it
    bool local_lstm;                 // impl 8 / 9: every forward on lstm_fwd_local (rnn_local_lstm.hip); no exchange buffer, nothing of `cluster` holds
    bool local_train;                // impl 9: ... a DEP_RUN_TRAIN forward on its saving instance, the backward on lstm_bwd_local; wpT holds that sweep's image
};

// A bidirectional GRU runs the tile-MFMA sweeps (gru_*_mfma<JPW, RAG, true>) and nothing else: it has no generic, cluster or fused
// instances, so the descriptor is good exactly where those sweeps can run.
bool bigru_ok(const dep_rnn_desc* d) { return (d->impl == 0 || d->impl == 2) && dep_sweep_use_mfma(d->H, d->impl); }

// dep_last_error for a descriptor refused by the rule above (the entry points and the size queries; DEP_OK for any other descriptor)
int bigru_refusal(const dep_rnn_desc* d, const char* who) {
    if (!d || d->cell != DEP_CELL_GRU || d->dirs != 2 || d->H <= 0 || d->impl == 6 || d->impl == 7 || bigru_ok(d)) return DEP_OK;      // (impl 6 / 7: bicluster_refusal)
    dep_set_error("%s: a bidirectional GRU (dirs = 2) runs the tile-MFMA sweeps only: impl must be 0 or 2 and H a multiple of 16 those sweeps can "
                  "tile (H / 16 = waves x tiles per wave, waves in {1, 2, 4, 8}, tiles <= 4, within the LDS bound: 16 .. 64, 96, 128, 192, 256); got H = %d, impl = %d", who, d->H, d->impl);
    return DEP_ERR_ARG;
}

// impl = 4, "the per-layer cluster sweeps": the unidirectional GRU where gru_fwd_cluster_r1 / gru_bwd_cluster_r1 have instances.
// impl = 5, "the per-layer cluster sweeps, state through training": impl = 4 in every respect (descriptors, layout, plan, launches, bits)
// that also takes hx in a DEP_RUN_TRAIN forward and hx / dhx in the backward state calls (state_refusal).
bool percluster_impl(const dep_rnn_desc* d) { return d->impl == 4 || d->impl == 5; }
bool percluster_ok(const dep_rnn_desc* d) { return d->cell == DEP_CELL_GRU && d->dirs == 1 && dep_cluster_ok(d->cell, d->H, d->B, d->dirs); }

// dep_last_error for an impl = 4 / 5 descriptor refused by the rule above (DEP_OK for any other descriptor)
int percluster_refusal(const dep_rnn_desc* d, const char* who) {
    if (!d || !percluster_impl(d) || d->H <= 0 || percluster_ok(d)) return DEP_OK;
    dep_set_error("%s: impl = %d (the per-layer cluster sweeps%s) is a unidirectional GRU with H in {64, 128, 256, 512}: cell must be DEP_CELL_GRU and "
                  "dirs 1; got cell = %d, H = %d, dirs = %d", who, d->impl, d->impl == 5 ? ", state through training" : "", d->cell, d->H, d->dirs);
    return DEP_ERR_ARG;
}

// impl = 6, "the per-layer cluster forward of a bidirectional GRU": gru_fwd_cluster_r1<.., BI = true> runs every forward, both directions
// of a layer in one launch; the backward is the tile-MFMA BiGRU's (gru_bwd_mfma<.., true>) on the reserve that forward leaves -- the same
// four fp32 (B,T,2H) saved-gate arrays.  H = 512 has the forward only: the tile sweeps stop at 256, dep_rnn_backward refuses it.
// impl = 7, "the per-layer cluster sweeps of a bidirectional GRU, forward and backward": impl = 6 in every forward (launches, outputs, reserve
// layout, bit for bit); a DEP_RUN_TRAIN forward packs the cluster backward's image of each direction into wpT, and the backward runs ONE launch
// per layer of gru_bwd_cluster_r1<.., BI = true>, both directions of a batch chunk side by side, at all four H.  The sweep writes the fp32
// gate-gradient rows of the tile BiGRU backward, so everything behind it is the code impl 2 / 6 run.
bool bicluster_impl(const dep_rnn_desc* d) { return d->impl == 6 || d->impl == 7; }
bool bicluster_train_impl(const dep_rnn_desc* d) { return d->impl == 7; }
bool bicluster_ok(const dep_rnn_desc* d) { return d->cell == DEP_CELL_GRU && d->dirs == 2 && dep_cluster_ok(d->cell, d->H, d->B, d->dirs); }

// dep_last_error for an impl = 6 / 7 descriptor refused by the rule above (DEP_OK for any other descriptor)
int bicluster_refusal(const dep_rnn_desc* d, const char* who) {
    if (!d || !bicluster_impl(d) || d->H <= 0 || bicluster_ok(d)) return DEP_OK;
    dep_set_error("%s: impl = %d (the per-layer cluster %s of a bidirectional GRU) is a bidirectional GRU with H in {64, 128, 256, 512}: cell must be "
                  "DEP_CELL_GRU and dirs 2; got cell = %d, H = %d, dirs = %d", who, d->impl, d->impl == 7 ? "sweeps, forward and backward," : "forward", d->cell, d->H, d->dirs);
    return DEP_ERR_ARG;
}

// impl = 8, "the exchange-free per-layer LSTM forward": lstm_fwd_local runs every forward, one workgroup per (direction, 16-utterance tile)
// with the whole W_hh of its direction in registers -- no exchange buffer, no co-residency, any batch in one launch.  Forward only: the run
// modes no backward follows (DEP_RUN_EVAL, DEP_RUN_DROPOUT_ONLY), LSTM, H = 128, dirs 1 or 2.  It takes hx, cx and c_n, dense and ragged.
bool local_impl(const dep_rnn_desc* d) { return d->impl == 8; }
bool local_ok(const dep_rnn_desc* d) {
    return dep_local_lstm_ok(d->cell, d->H, d->dirs) && (d->training == DEP_RUN_EVAL || d->training == DEP_RUN_DROPOUT_ONLY) && d->L >= 1 && d->L <= MAXL;
}

// dep_last_error for an impl = 8 descriptor refused by the rule above (DEP_OK for any other descriptor)
int local_refusal(const dep_rnn_desc* d, const char* who) {
    if (!d || !local_impl(d) || local_ok(d)) return DEP_OK;
    dep_set_error("%s: impl = 8 (the exchange-free per-layer LSTM forward) is a forward-only LSTM with H = 128: cell must be DEP_CELL_LSTM, dirs 1 or 2, "
                  "L 1 .. %d and the run mode DEP_RUN_EVAL or DEP_RUN_DROPOUT_ONLY (DEP_RUN_TRAIN needs a backward, which it does not have); "
                  "got cell = %d, H = %d, dirs = %d, L = %d, run mode = %d", who, MAXL, d->cell, d->H, d->dirs, d->L, d->training);
    return DEP_ERR_ARG;
}

// impl = 9, "the exchange-free per-layer LSTM sweeps, forward and backward": impl = 8 in every forward no backward follows (the same
// lstm_fwd_local instances, the same bits), plus DEP_RUN_TRAIN: that forward runs lstm_fwd_save_local, which also stores the fp32 activated
// gates and c where the layout keeps the LSTM's saved gates, and packs the backward's W_hh image beside the forward's; every backward entry
// point runs ONE launch of lstm_bwd_local per layer, which writes the fp32 gate-gradient rows (ldg = dirs*4H) and one dbpart row per
// (direction, tile), so everything behind the sweep is the unpaired code the tile sweeps run.  It takes every state member, dense and ragged.
bool local_train_impl(const dep_rnn_desc* d) { return d->impl == 9; }
bool local_train_ok(const dep_rnn_desc* d) {
    return dep_local_lstm_ok(d->cell, d->H, d->dirs) && d->L >= 1 && d->L <= MAXL &&
           (d->training == DEP_RUN_EVAL || d->training == DEP_RUN_TRAIN || d->training == DEP_RUN_DROPOUT_ONLY);
}

// dep_last_error for an impl = 9 descriptor refused by the rule above (DEP_OK for any other descriptor)
int local_train_refusal(const dep_rnn_desc* d, const char* who) {
    if (!d || !local_train_impl(d) || local_train_ok(d)) return DEP_OK;
    dep_set_error("%s: impl = 9 (the exchange-free per-layer LSTM sweeps, forward and backward) is an LSTM with H = 128: cell must be DEP_CELL_LSTM, "
                  "dirs 1 or 2, L 1 .. %d and the run mode DEP_RUN_EVAL, DEP_RUN_TRAIN or DEP_RUN_DROPOUT_ONLY; "
                  "got cell = %d, H = %d, dirs = %d, L = %d, run mode = %d", who, MAXL, d->cell, d->H, d->dirs, d->L, d->training);
    return DEP_ERR_ARG;
}

// impl = 9 trains in the parity modes only: the saving forward and the backward have no single-product instances
int local_train_mode_refusal(const dep_rnn_desc* d, const char* who, int mode) {
    if (!local_train_impl(d) || mode <= 1) return DEP_OK;
    dep_set_error("%s: impl = 9 (the exchange-free per-layer LSTM sweeps, forward and backward) runs its DEP_RUN_TRAIN forward and its backward in GEMM "
                  "modes 0 and 1 only; the current mode is %d (dep_set_gemm_mode).  Its DEP_RUN_EVAL and DEP_RUN_DROPOUT_ONLY forwards run in all four", who, mode);
    return DEP_ERR_ARG;
}

bool make_layout(const dep_rnn_desc* d, Layout& lo) {
    if (!d || d->B <= 0 || d->T <= 0 || d->F <= 0 || d->H <= 0 || d->L < 1 || d->L > MAXL) return false;
    if (local_impl(d) && !local_ok(d)) return false;
    if (local_train_impl(d) && !local_train_ok(d)) return false;
    lo.local_train = local_train_impl(d);
    lo.local_lstm = local_impl(d) || lo.local_train;
    if (percluster_impl(d) && !percluster_ok(d)) return false;
    if (bicluster_impl(d) && !bicluster_ok(d)) return false;
    if (d->cell == DEP_CELL_GRU) { if (d->dirs != 1 && !(d->dirs == 2 && (bigru_ok(d) || bicluster_impl(d)))) return false; }
    else if (d->cell == DEP_CELL_LSTM) { if (d->dirs != 1 && d->dirs != 2) return false; }
    else return false;
    if (d->dropout_p < 0.f || d->dropout_p >= 1.f) return false;
    if (d->training != DEP_RUN_EVAL && d->training != DEP_RUN_TRAIN && d->training != DEP_RUN_DROPOUT_ONLY) return false;
    lo.G = d->cell == DEP_CELL_GRU ? 3 : 4; lo.D = d->dirs; lo.L = d->L;
    lo.BT = (size_t)d->B * d->T;
    lo.keep = d->training == DEP_RUN_TRAIN;
    lo.donly = d->training == DEP_RUN_DROPOUT_ONLY;
    lo.drop = d->training != DEP_RUN_EVAL && d->dropout_p > 0.f;
    const size_t H = d->H, D = d->dirs, G = lo.G;
    const size_t maxin = D * H > (size_t)d->F ? D * H : (size_t)d->F;      // the widest layer input
    auto al = [](size_t f) { return (f + 63) / 64 * 64; };
    size_t off = 0;
    for (int l = 0; l < d->L; ++l) {
        // dropout-only: a lower layer keeps the copy the next layer's projection reads (dropout(y), or y when p = 0); the top layer
        // keeps y (the caller's zero-copy view) unless it is a pooled GRU, whose pooled output is all that leaves the forward
        const bool top = l == d->L - 1;
        const bool ykept = !lo.donly || (top ? !(d->cell == DEP_CELL_GRU && d->pool != DEP_POOL_NONE) : !lo.drop);
        lo.y[l] = NOT_KEPT; if (ykept) { lo.y[l] = off; off += al(lo.BT * D * H); }
        lo.ydrop[l] = off; if (lo.drop && l < d->L - 1) off += al(lo.BT * D * H);
        for (int k = 0; k < 4; ++k) lo.sv[l][k] = NOT_KEPT;
        if (lo.keep) {
            if (d->cell == DEP_CELL_GRU) { for (int k = 0; k < 4; ++k) { lo.sv[l][k] = off; off += al(lo.BT * D * H); } }
            else { lo.sv[l][0] = off; off += al(lo.BT * D * 4 * H); lo.sv[l][1] = off; off += al(lo.BT * D * H); lo.sv[l][2] = lo.sv[l][3] = 0; }
        }
        for (size_t dd = 0; dd < D; ++dd) {
            lo.wp[l][dd] = off; off += al(G * H * H);
            lo.wpT[l][dd] = NOT_KEPT; if (!lo.donly) { lo.wpT[l][dd] = off; off += al(G * H * H); }
        }
    }
    // bidirectional stacks: the two directions share their input, so their input projections, dX and dW_ih are ONE contraction
    // each over stacked weights [W_ih(fwd); W_ih(bwd)] (2 G H x in) -- the input (629 MB at cfg3's layer 0) is read once, and
    // dX needs no read-modify-write.  The stacked copies live in the reserve (the backward's dX reads them again).
    for (int l = 0; l < d->L; ++l) {
        lo.wstack[l] = lo.bstack[l] = 0;
        if (d->dirs == 2) {
            const size_t in = l == 0 ? (size_t)d->F : D * H;
            lo.wstack[l] = off; off += al(D * G * H * in);
            lo.bstack[l] = off; off += al(D * G * H);
        }
    }
    lo.reserve_floats = off;
    // workspace
    // rows of bias-gradient partials: one per 16-utterance tile for the tile-MFMA and the cluster sweeps, one per utterance for
    // the generic sweep.  (Sized for the larger; dep_finish_db sums the rows the sweep that ran has written: dbpart_rows.)
    lo.nwg = dep_sweep_num_wg(d->B, d->H, d->impl);
    lo.cluster_bwd2 = bicluster_train_impl(d);
    if (lo.cluster_bwd2) lo.nwg = dep_cdiv(d->B, 16);      // the bidirectional cluster backward: one row per (direction, tile) at every H
    if (lo.local_train) lo.nwg = dep_cdiv(d->B, 16);       // lstm_bwd_local: likewise
    size_t w = 0;
    lo.gi = w; w += al(lo.BT * D * (G + (d->cell == DEP_CELL_GRU && lo.keep ? 1 : 0)) * H);     // GI (fwd) / dGI (bwd; GRU: room for the 4H-wide [dr|dz|dn|dn*r] rows)
    lo.dghn = w; w += al(lo.BT * (d->cell == DEP_CELL_GRU ? D : 1) * H);      // GRU: (B,T,dirs*H)
    lo.dx[0] = w; w += al(lo.BT * D * H);
    lo.dx[1] = w; w += al(lo.BT * D * H);
    lo.dbpart = w; w += al((size_t)D * lo.nwg * 4 * H);
    lo.biastmp = w; w += al(G * H);
    lo.dwstack = w; if (d->dirs == 2 && lo.keep) w += al(D * G * H * maxin);
    // split-K scratch: the largest weight-gradient contraction
    size_t gb = 0;
    {   // every (rows, cols) block dep_rnn_backward contracts over B*T: dW_ih (G H x F | D H), dW_hh whole or as the GRU's
        // (2H x H) + (H x H) pair -- the split count depends on the block shape, so take the maximum over all of them
        const int Ms[4] = {(int)(D * G * H), (int)(G * H), (int)(2 * H), (int)H};      // (D G H: the direction-stacked dW_ih of a bidirectional stack)
        const int Ns[3] = {d->F, (int)(D * H), (int)H};
        for (int i = 0; i < 4; ++i)
            for (int j = 0; j < 3; ++j) {
                const size_t b1 = dep_gemm_workspace_bytes(1, 0, Ms[i], Ns[j], (int)lo.BT);
                if (b1 > gb) gb = b1;
            }
    }
    if (lo.keep && ((d->cell == DEP_CELL_GRU && d->dirs == 1) || (d->cell == DEP_CELL_LSTM && d->dirs == 2))) {
        // dW_ih + dW_hh of a GRU layer / dW_hh of both directions of a BiLSTM layer as one launch (dep_gemm_tn_pair): two sets of partials
        const size_t b2 = 2 * dep_gemm_workspace_bytes(1, 0, (int)(G * H), (int)H, (int)lo.BT);
        if (b2 > gb) gb = b2;
    }
    {   // ... and the forward's use of the same scratch: the stage image of a layer's (direction-stacked) W_ih (gemm_bf16x3_nt_dma)
        const size_t b3 = (size_t)D * G * H * maxin * sizeof(float);
        if (b3 > gb) gb = b3;
    }
    lo.gemm = w; lo.gemm_bytes = gb; w += al(gb / sizeof(float) + 64);
    // impl: 0 auto (cluster > tile-MFMA > generic), 1 generic, 2 tile-MFMA, 3 cluster (must be supported), 4 / 5 the per-layer cluster
    // sweeps (GRU, dirs = 1, checked above): the cluster layout without the fused two-layer extras, plus the hx staging area
    // (a bidirectional GRU is never planned onto the cluster, 16-unit-member or fused kernels: dep_cluster_ok does not look at dirs)
    const bool cok = d->cell == DEP_CELL_GRU ? d->dirs == 1 && dep_cluster_ok(d->cell, d->H, d->B, d->dirs) : dep_cluster_lstm_ok(d->H, d->B, d->dirs);
    if (d->impl == 3 && !cok) return false;
    lo.cluster = cok && (d->impl == 0 || d->impl == 3 || percluster_impl(d));      // (impl 8 / 9: none of the cluster parts)
    // impl 6 (checked above): the bidirectional forward's exchange buffer and the hx staging area, and none of what `cluster` selects
    lo.cluster_fwd = bicluster_impl(d);
    // impl 7: the larger of the bidirectional forward's buffer and the bidirectional backward's
    const size_t bixb = !lo.cluster_bwd2 ? 0 : dep_cluster_bwd_bi_xbuf_bytes(d->H, d->B);
    lo.xbuf = w; lo.xbuf_bytes = lo.cluster_fwd ? (bixb > dep_cluster_xbuf_bytes(d->cell, d->H, d->B, d->dirs) ? bixb : dep_cluster_xbuf_bytes(d->cell, d->H, d->B, d->dirs))
                               : !lo.cluster ? 0 : (d->cell == DEP_CELL_GRU ? dep_cluster_xbuf_bytes(d->cell, d->H, d->B, d->dirs)
                                                                : dep_cluster_lstm_xbuf_bytes(d->H, d->B, d->dirs));
    if (lo.cluster) lo.nwg = dep_cdiv(d->B, 16);      // the cluster sweeps write one row per tile whatever the tile-MFMA sweep could do at this H
    lo.fused2 = lo.cluster && !percluster_impl(d) && dep_fused2_ok(d->cell, d->H, d->L, d->dirs);
    if (lo.fused2) {
        size_t fb = dep_fused2_xbuf_bytes(d->B); if (fb > lo.xbuf_bytes) lo.xbuf_bytes = fb;
        if (lo.keep) { fb = dep_fused2_bwd_xbuf_bytes(d->B); if (fb > lo.xbuf_bytes) lo.xbuf_bytes = fb; }
    }
    w += al(lo.xbuf_bytes / sizeof(float) + 64);
    lo.wih_img = w; if (lo.fused2) w += al(G * H * H);
    lo.gi2 = lo.dghn2 = lo.dbpart2 = 0;
    if (lo.fused2 && lo.keep) {
        lo.gi2 = w; w += al(lo.BT * (G + 1) * H);      // (room for the 4H-wide [dr | dz | dn | dn*r] rows, like lo.gi)
        lo.dghn2 = w; w += al(lo.BT * H);
        lo.dbpart2 = w; w += al((size_t)lo.nwg * 4 * H);
    }
    lo.hxstage = w; if (percluster_impl(d) || lo.cluster_fwd) w += al(D * d->B * H);
    lo.ws_floats = w;
    return true;
}

}  // namespace

extern "C" size_t dep_rnn_reserve_bytes(const dep_rnn_desc* d) {
    Layout lo;
    if (!make_layout(d, lo)) {
        if (!percluster_refusal(d, "dep_rnn_reserve_bytes") && !bicluster_refusal(d, "dep_rnn_reserve_bytes") && !local_refusal(d, "dep_rnn_reserve_bytes") &&
            !local_train_refusal(d, "dep_rnn_reserve_bytes"))
            (void)bigru_refusal(d, "dep_rnn_reserve_bytes");
        return 0;
    }
    return lo.reserve_floats * sizeof(float);
}
extern "C" size_t dep_rnn_workspace_bytes(const dep_rnn_desc* d) {
    Layout lo;
    if (!make_layout(d, lo)) {
        if (!percluster_refusal(d, "dep_rnn_workspace_bytes") && !bicluster_refusal(d, "dep_rnn_workspace_bytes") && !local_refusal(d, "dep_rnn_workspace_bytes"))
            (void)local_train_refusal(d, "dep_rnn_workspace_bytes");
        return 0;
    }
    return lo.ws_floats * sizeof(float);
}
// byte offset of layer l's output sequence (B,T,H*dirs) inside the reserve (zero-copy access for the caller)
extern "C" size_t dep_rnn_reserve_y_offset(const dep_rnn_desc* d, int layer) {
    Layout lo;
    if (!make_layout(d, lo) || layer < 0 || layer >= d->L || lo.y[layer] == NOT_KEPT) return (size_t)-1;
    return lo.y[layer] * sizeof(float);
}
extern "C" size_t dep_rnn_reserve_ydrop_offset(const dep_rnn_desc* d, int layer) {
    Layout lo;
    if (!make_layout(d, lo) || layer < 0 || layer >= d->L - 1 || !lo.drop) return (size_t)-1;
    return lo.ydrop[layer] * sizeof(float);
}

// Byte offset of the cluster exchange buffer inside the workspace (debug tooling: DEP_TRACE stamps live at +4096).
extern "C" size_t dep_rnn_workspace_xbuf_offset(const dep_rnn_desc* d) {
    Layout lo;
    if (!make_layout(d, lo) || !(lo.cluster || lo.cluster_fwd)) return (size_t)-1;
    return lo.xbuf * sizeof(float);
}

// Status of the cluster sweeps that ran on (workspace): 0 ok, 2 = a bounded spin gave up (a cluster member was
// not resident or died).  Synchronises the stream.
extern "C" int dep_rnn_status(const dep_rnn_desc* d, void* workspace, void* stream) {
    Layout lo;
    DEP_CHECK_ARG(make_layout(d, lo) && workspace);
    if (!(lo.cluster || lo.cluster_fwd)) return DEP_OK;
    unsigned st = 0;
    if (hipMemcpyAsync(&st, (float*)workspace + lo.xbuf, sizeof(st), hipMemcpyDeviceToHost, (hipStream_t)stream) != hipSuccess ||
        hipStreamSynchronize((hipStream_t)stream) != hipSuccess) {
        dep_set_error("dep_rnn_status: HIP copy failed"); return DEP_ERR_HIP;
    }
    if (st != 0) { dep_set_error("cluster sweep gave up waiting for a member (status %u)", st); return DEP_ERR_HIP; }
    return DEP_OK;
}

const RnnSwitches& dep_rnn_switches() {
    static const RnnSwitches sw = [] {
        RnnSwitches w;
        const char* e = getenv("DEP_SV16"); w.sv16 = !(e && e[0] == '0');
        e = getenv("DEP_LSTM_SV16"); w.lstm_sv16 = e && e[0] == '1';
        e = getenv("DEP_FUSED2"); w.fused2 = !(e && e[0] == '0');
        e = getenv("DEP_FUSED2_BWD"); w.fused2_bwd = e ? e[0] == '1' : DEP_FUSED2_BWD_DEFAULT != 0;
        e = getenv("DEP_CLUSTER16"); w.cluster16 = !(e && e[0] == '0');
        e = getenv("DEP_CLUSTER_LSTM"); w.cluster_lstm = !(e && e[0] == '0');
        e = getenv("DEP_DGI_PK"); w.dgi_pk = !(e && e[0] == '0');
        e = getenv("DEP_COMM_OVERLAP"); w.comm_beside_sweeps = e && e[0] == 's';
        e = getenv("DEP_EXCLUSIVE"); w.exclusive = !(e && e[0] == '0');
        return w;
    }();
    return sw;
}

// Kernels that need every CU to themselves (the fused two-layer GRU forward, the 16-unit-member forward): allowed unless the
// process said otherwise (DEP_EXCLUSIVE=0 / dep_rnn_set_exclusive(0): the GPU is shared with other streams or processes).
static std::atomic<int> g_exclusive{-1};             // -1 = not set: DEP_EXCLUSIVE
static bool dep_exclusive_on() { const int v = g_exclusive.load(std::memory_order_relaxed); return v >= 0 ? v == 1 : dep_rnn_switches().exclusive; }
extern "C" int dep_rnn_set_exclusive(int on) { g_exclusive.store(on ? 1 : 0); return DEP_OK; }
extern "C" int dep_rnn_get_exclusive(void) { return dep_exclusive_on() ? 1 : 0; }

namespace {

// ---- the plan of one call ----------------------------------------------------------------------------------------------------
// Which kernels a dep_rnn_forward / dep_rnn_backward call runs and on which weight images, decided once from the descriptor, the
// switches and the call's snapshot of the two process-wide settings (dep_set_gemm_mode, dep_rnn_set_exclusive): the entry points
// take the snapshot at entry and read neither again, so another thread changing them mid-call cannot mix two modes in one call.
// (The GEMM layer follows the mode on its own -- its documented contract.)
enum FwdKernel { FWD_FUSED2,          // both GRU layers in one launch, the per-layer cluster kernels enqueued behind it as its on-device fallback
                 FWD_CLUSTER16,       // GRU, 16-unit members (rnn_cluster16.hip)
                 FWD_CLUSTER_GRU,     // GRU, 32-unit members (rnn_cluster.hip)
                 FWD_CLUSTER_LSTM,    // (Bi)LSTM cluster (rnn_cluster_lstm.hip)
                 FWD_LOCAL_LSTM,      // (Bi)LSTM, one workgroup per (direction, tile), no exchange (rnn_local_lstm.hip; impl 8 / 9)
                 FWD_TILE };          // tile-MFMA / generic sweep (rnn_sweep.hip picks by impl and H)
enum BwdKernel { BWD_FUSED2, BWD_CLUSTER_GRU, BWD_CLUSTER_LSTM,
                 BWD_LOCAL_LSTM,      // (Bi)LSTM, one workgroup per (direction, tile), no exchange (lstm_bwd_local, rnn_local_lstm.hip; impl 9)
                 BWD_TILE };
// the split-precision recurrent-weight images (the fp32 fragment images of dep_pack_whh are RnnPlan::whh_f32)
enum WhhImage { WHH_NONE, WHH_SPLIT16, WHH_SPLIT32, WHH_LSTM_PAIR /* forward and backward image in one launch */, WHH_BWD_SPLIT, WHH_BWD_F32 /* fp32, member-sliced */ };
// What a forward leaves behind in its reserve: dep_rnn_backward must run kernels of the same kind (reserve_tag_refusal).
enum ReserveTag { TAG_SPLIT = 1, TAG_SV16 = 4, TAG_BF16ST = 8, TAG_DONLY = 16 };

struct RnnPlan {
    bool excl;                       // the snapshot of dep_rnn_set_exclusive (the mode's is in the fields below)
    bool split;                      // recurrent products of the cluster sweeps: 3-term bf16 split on the bf16 matrix cores (mode >= 1; mode 2 / 3 keep it), else exact fp32 MFMA
    FwdKernel fwd; BwdKernel bwd;
    bool whh_f32;                    // a layer packs the fp32 fragment images (kernels that are not running on split-precision images)
    WhhImage whh_fwd, whh_bwd;       // ... and these (FWD_FUSED2 packs the same two kinds for both layers in one launch)
    bool sv16;                       // saved gates r, z, n as 16-bit fixed point: reserve tag, fused launches, backward sweeps
    bool sv16_fwd;                   // ... and the per-layer forward launches: the 16-unit-member kernel has no 16-bit path
    bool dg4;                        // GRU cluster backward: gate gradients as ONE (B*T, 4H) array [dr | dz | dn | dn*r] (dW_hh is then one contraction)
    bool bf16st;                     // dep_set_gemm_mode(3) on a stack whose kernels have the bf16-storage variants (2-layer GRU, H = 256, fused forward): y, hn as bf16, gate gradients as PKH
    bool pk;                         // gate gradients may be the PK image of gemm_bf16x3.hip: what the descriptor decides of it (operand alignment and GEMM paths are checked per layer)
    int pk_fmt;                      // ... read by the contractions as FMT_PK, or through its hi rows (FMT_PKH) in the single-product modes
    bool dw_pair;                    // layers with H inputs ask split-K target 512 for their weight gradients (the dW_ih + dW_hh pair's; bf16x3 mode only)
    int tag;                         // ReserveTag bits
};

// ragged: the call has a lengths array (dep_rnn_*_varlen).  It is planned only onto kernels that implement the per-row predicate -- the
// tile / generic sweeps, the per-layer cluster GRU sweeps and the cluster BiLSTM sweeps, each of which launches its RAG instance when
// the sweep arguments carry lengths -- never onto the fused two-layer launches or the 16-unit-member forward (so it enqueues no
// soft-fallback launches either).  Everything else (images, saved-gate format, PK gate gradients) is decided as for a dense call.
// impl = 4 / 5 (the per-layer cluster sweeps) is planned like a ragged call, dense or not: FWD_CLUSTER_GRU / BWD_CLUSTER_GRU and what follows
// from them.  Its layout has no fused2 part, and the 16-unit-member kernel does not belong to the descriptor, so the 32-unit-member image
// and the 16-bit saved gates are chosen as on a shape without that kernel.
// impl = 6 (lo.cluster_fwd): FWD_CLUSTER_GRU on the bidirectional instance, dense or ragged, with each direction's 32-unit-member image (split
// products) or the fp32 fragment image (exact mode), fp32 saved gates; everything of the backward is the tile BiGRU's of impl = 2 -- BWD_TILE on
// the wpT image of dep_pack_whh, packed by a DEP_RUN_TRAIN forward in either mode -- because lo.cluster is off.
// impl = 7 (lo.cluster_bwd2): impl = 6's forward; BWD_CLUSTER_GRU on the bidirectional instances, dense or ragged, on each direction's cluster
// backward image in wpT (WHH_BWD_SPLIT in split mode, the member-sliced fp32 image in exact mode) instead of the tile backward's; fp32 saved
// gates, fp32 gate-gradient rows (pk = false: dg4 is off), the unpaired contractions.  Modes 2 / 3 keep the split instance; the contractions
// behind the sweep follow the mode on their own (a mode-3 backward is refused by dep_rnn_backward: no PK image to take the hi rows of).
// impl = 8 (lo.local_lstm): FWD_LOCAL_LSTM, dense or ragged, whatever `excl` says: the split instance on the forward image of
// pack_lstm_split_kernel in modes 1 / 2 / 3, the exact instance on the fp32 fragment image in mode 0.  No backward is ever planned on it.
// impl = 9 (lo.local_train): impl = 8's plan, and BWD_LOCAL_LSTM, dense or ragged.  A DEP_RUN_TRAIN forward packs both images of a direction:
// WHH_LSTM_PAIR (one launch of pack_lstm_split_kernel with `bwd` set) in split mode, the two fp32 fragment images of dep_pack_whh in mode 0.
// fp32 saved gates (sv16 off), fp32 gate-gradient rows (pk off, dg4 off), the unpaired contractions.  Modes 2 / 3 are refused for the training
// forward and the backward (local_train_mode_refusal) before anything is launched.
RnnPlan make_plan(const dep_rnn_desc* d, const Layout& lo, int mode, bool excl, bool ragged) {
    const RnnSwitches& sw = dep_rnn_switches();
    const bool gru = d->cell == DEP_CELL_GRU;
    RnnPlan p{};
    p.excl = excl; p.split = mode >= 1;
    const bool csplit = (lo.cluster || lo.cluster_fwd || lo.local_lstm) && p.split;      // the forward's recurrent-weight image is a split-precision one
    // the kernels that fill every CU (fused forward, 16-unit members) are not for a shared GPU; the fused BACKWARD does not care
    const bool cluster16 = lo.cluster && !percluster_impl(d) && dep_cluster16_ok(d->cell, d->H, d->B);
    p.fwd = (lo.fused2 && p.split && excl && !ragged) ? FWD_FUSED2 : (cluster16 && excl && !ragged) ? FWD_CLUSTER16
          : lo.cluster_fwd ? FWD_CLUSTER_GRU : lo.local_lstm ? FWD_LOCAL_LSTM : !lo.cluster ? FWD_TILE : gru ? FWD_CLUSTER_GRU : FWD_CLUSTER_LSTM;
    p.bwd = (lo.fused2 && sw.fused2_bwd && p.split && dep_fused2_bwd_fits(d->B, d->T) && !ragged) ? BWD_FUSED2
          : lo.cluster_bwd2 ? BWD_CLUSTER_GRU : lo.local_train ? BWD_LOCAL_LSTM : !lo.cluster ? BWD_TILE : gru ? BWD_CLUSTER_GRU : BWD_CLUSTER_LSTM;
    p.whh_f32 = (lo.cluster || lo.local_lstm) ? !p.split : lo.cluster_fwd ? (!p.split || (lo.keep && !lo.cluster_bwd2)) : dep_sweep_use_mfma(d->H, d->impl);
    p.whh_fwd = !csplit ? WHH_NONE : !gru ? WHH_LSTM_PAIR : p.fwd == FWD_CLUSTER16 ? WHH_SPLIT16 : WHH_SPLIT32;
    p.whh_bwd = (!(lo.cluster || lo.cluster_bwd2) || !lo.keep || p.whh_fwd == WHH_LSTM_PAIR) ? WHH_NONE : p.split ? WHH_BWD_SPLIT : WHH_BWD_F32;
    // 16-bit saved gates: the kernels that implement them are the fused forward, the 32-unit-member forward and the 32-unit-member
    // backward (burst or not); the 16-unit-member kernels and exact-fp32 mode read / write fp32 gates.  Follows the DESCRIPTOR's
    // cluster16, not whether this call may run that kernel.  An INSTANCE choice: a dropout-only forward launches the instance
    // training launches, though it saves no gates.
    p.sv16 = p.split && sw.sv16 && d->training != DEP_RUN_EVAL && lo.cluster && (gru ? (lo.fused2 || !cluster16) : dep_cluster_lstm_sv16_ok());
    p.sv16_fwd = p.sv16 && p.fwd != FWD_CLUSTER16;
    p.dg4 = lo.cluster && gru && d->dirs == 1;
    // bf16-STORAGE mode (dep_set_gemm_mode(3); a labelled throughput mode, never the parity path): only where every kernel of the
    // stack has the variant -- the fused 2-layer GRU forward and the burst backward with the 4H-wide gate-gradient rows.  Other
    // stacks run mode 3 exactly like mode 2 (single bf16 products, fp32 storage).
    p.bf16st = mode == 3 && lo.keep && p.sv16 && lo.fused2 && p.dg4 && d->T % 2 == 0 && dep_cluster_bwd_pk_ok(d->H, d->T);
    p.pk = sw.dgi_pk && csplit && !lo.local_lstm && lo.BT % 2 == 0 &&
           (gru ? p.dg4 && d->T % 2 == 0 && (p.bwd == BWD_FUSED2 || dep_cluster_bwd_pk_ok(d->H, d->T)) : d->dirs == 2 && dep_cluster_lstm_bwd_pk_ok(d->T));
    p.pk_fmt = (p.bf16st || mode >= 2) ? FMT_PKH : FMT_PK;
    p.dw_pair = p.dg4 && mode == 1;      // (the other precision modes never pair: they keep the single launches' target)
    p.tag = (p.split ? TAG_SPLIT : 0) | (p.sv16 ? TAG_SV16 : 0) | (p.bf16st ? TAG_BF16ST : 0) | (lo.donly ? TAG_DONLY : 0);
    return p;
}

// what layer l's input projection (and its dW_ih) reads: x, or the layer below's (dropped) output in the reserve; K = its width
struct LayerIn { const float* p; int K; };
LayerIn layer_input(const dep_rnn_desc* d, const Layout& lo, const float* x, const float* R, int l) {
    if (l == 0) return {x, d->F};
    return {R + (lo.drop ? lo.ydrop[l - 1] : lo.y[l - 1]), d->dirs * d->H};
}

// The tag of the plan whose forward wrote a reserve (host-side record, no device traffic): the recurrent-weight images and saved
// gates in it are precision-mode specific, and a caller flipping dep_set_gemm_mode between a forward and its backward would
// otherwise get silently wrong gradients.  Small ring: the newest record of a pointer wins; a reserve with no record (evicted
// after 256 other forwards) is trusted.
struct TagRec { const void* p; int tag; };
TagRec g_tags[256];
int g_tag_next = 0;
std::mutex g_tag_mu;
void record_reserve_tag(const void* reserve, int tag) {
    std::lock_guard<std::mutex> lk(g_tag_mu);
    for (auto& r : g_tags) if (r.p == reserve) { r.tag = tag; return; }
    g_tags[g_tag_next] = {reserve, tag};
    g_tag_next = (g_tag_next + 1) % 256;
}
// dep_rnn_backward: DEP_OK unless the reserve's recorded tag and this call's differ in one of `bits`
int reserve_tag_refusal(const void* reserve, int want, int bits) {
    int have = -1;
    {
        std::lock_guard<std::mutex> lk(g_tag_mu);
        for (auto& r : g_tags) if (r.p == reserve) { have = r.tag; break; }
    }
    if (have < 0) return DEP_OK;
    const int diff = (have ^ want) & bits;
    if (diff & TAG_DONLY)
        dep_set_error("dep_rnn_backward: the reserve was last written by a DEP_RUN_DROPOUT_ONLY forward, which keeps no saved gates; "
                      "run the forward with DEP_RUN_TRAIN before a backward");
    else if (diff & TAG_SPLIT)
        dep_set_error("dep_rnn_backward: the reserve was produced by a forward in %s mode, the current mode is %s "
                      "(dep_set_gemm_mode must not change between a forward and its backward)",
                      (have & TAG_SPLIT) ? "bf16x3" : "f32", (have & TAG_SPLIT) ? "f32" : "bf16x3");
    else if (diff & TAG_BF16ST)
        dep_set_error("dep_rnn_backward: the reserve was %swritten in bf16-storage mode (dep_set_gemm_mode(3)), this call runs in the other", (have & TAG_BF16ST) ? "" : "not ");
    else if (diff & TAG_SV16)
        dep_set_error("dep_rnn_backward: the reserve holds %s saved gates, this call expects the other format (DEP_SV16 / DEP_EXCLUSIVE changed?)",
                      (have & TAG_SV16) ? "16-bit" : "fp32");
    return diff ? DEP_ERR_ARG : DEP_OK;
}

// ragged calls run in the parity modes only: the single-product modes' storage variants have no ragged instances
int ragged_mode_refusal(const char* who, const int32_t* lengths, int mode) {
    if (!lengths || mode <= 1) return DEP_OK;
    dep_set_error("%s: a ragged call (lengths given) runs in GEMM modes 0 and 1 only; the current mode is %d (dep_set_gemm_mode)", who, mode);
    return DEP_ERR_ARG;
}

// dep_rnn_*_state: a call that brings a state (any member non-NULL) runs where the per-layer sweeps of rnn_sweep.hip run the stack, and
// the cell state belongs to the LSTM.  Checked before anything is launched (and before any HIP call); DEP_OK for a call without state.
// impl = 8 and impl = 9 have no exchange buffer (lo.cluster is off), so they pass: impl 8's forwards take hx / cx / c_n, and impl 9 takes every
// member in every forward and backward -- lstm_bwd_local owns the whole W_hh, so dhx / dcx are what it carries past its last step and there is
// no host-side recurrent term; the hx term of dW_hh is the code behind the sweep.
int state_refusal(const dep_rnn_desc* d, const Layout& lo, const char* who, bool any, bool any_c, bool backward, int mode) {
    if (!any) return DEP_OK;
    if (any_c && bicluster_train_impl(d)) {
        dep_set_error("%s: impl = 7 (the per-layer cluster sweeps of a bidirectional GRU) takes hx / dhx only: cx, c_n, dc_n and dcx are the LSTM's cell state "
                      "and its gradients", who);
        return DEP_ERR_ARG;
    }
    if (any_c && d->cell != DEP_CELL_LSTM) {
        dep_set_error("%s: cx, c_n, dc_n and dcx are the LSTM's cell state and its gradients; a GRU takes hx / dhx only", who);
        return DEP_ERR_ARG;
    }
    if (lo.cluster && d->impl == 5) {
        // state through training: hx in every forward; hx / dhx in the backward (gru_bwd_cluster_r1 takes hx as h_prev of step 0 and stores
        // the direct term of dhx, rnn_backward_impl adds the two host-side terms).  The bf16-storage / single-product instances get no hx.
        if (!backward || mode <= 1) return DEP_OK;
        dep_set_error("%s: a backward with a state (hx / dhx given) on impl = 5 runs in GEMM modes 0 and 1 only; the current mode is %d (dep_set_gemm_mode)", who, mode);
        return DEP_ERR_ARG;
    }
    if (lo.cluster && d->impl == 4) {
        // the per-layer cluster FORWARD takes hx (gru_fwd_cluster_r1); the cluster backward has neither hx as h_prev of step 0 nor dhx
        if (!backward && d->training != DEP_RUN_TRAIN) return DEP_OK;
        dep_set_error("%s: on impl = 4 (the per-layer cluster sweeps) hx is taken by the forward in DEP_RUN_EVAL and DEP_RUN_DROPOUT_ONLY only, the run "
                      "modes no backward follows: the cluster backward takes no state (no hx term in dW_hh, no dhx).  A DEP_RUN_TRAIN forward with hx "
                      "and every backward with a state member need impl 1 or 2; got run mode %d, H = %d", who, d->training, d->H);
        return DEP_ERR_ARG;
    }
    if (lo.cluster) {
        dep_set_error("%s: a recurrent state (hx / cx / c_n and their gradients) is taken only where the per-layer tile-MFMA or generic sweeps "
                      "run the stack, i.e. on a descriptor without a cluster exchange buffer (dep_rnn_workspace_xbuf_offset(d) == (size_t)-1): "
                      "impl 1 or 2, or impl 0 at a shape without cluster kernels; got cell = %d, H = %d, dirs = %d, impl = %d.  "
                      "(A GRU forward that no backward follows takes hx on the per-layer cluster sweeps too: impl = 4.)",
                      who, d->cell, d->H, d->dirs, d->impl);
        return DEP_ERR_ARG;
    }
    return DEP_OK;
}

}  // namespace

static int rnn_forward_impl(const dep_rnn_desc* d, const float* x, const int32_t* lengths, const float* const* weights, float* y,
                            float* pooled, float* h_n, const dep_rnn_state* state, void* reserve, size_t reserve_bytes, void* workspace,
                            size_t workspace_bytes, void* stream) {
    Layout lo;
    if (const int rf = percluster_refusal(d, "dep_rnn_forward")) return rf;
    if (const int rf = bicluster_refusal(d, "dep_rnn_forward")) return rf;
    if (const int rf = local_refusal(d, "dep_rnn_forward")) return rf;
    if (const int rf = local_train_refusal(d, "dep_rnn_forward")) return rf;
    if (const int rf = bigru_refusal(d, "dep_rnn_forward")) return rf;
    DEP_CHECK_ARG(make_layout(d, lo));
    const dep_rnn_state st = state ? *state : dep_rnn_state{nullptr, nullptr, nullptr};      // NULL and a struct of NULLs are the plain call
    // (state together with lengths is dep_rnn_forward_state_varlen: the ragged instances of rnn_sweep.hip carry the state through dead steps)
    if (const int rf = state_refusal(d, lo, lengths ? "dep_rnn_forward_state_varlen" : "dep_rnn_forward_state", st.hx || st.cx || st.c_n, st.cx || st.c_n, false, dep_get_gemm_mode())) return rf;
    const int mode = dep_get_gemm_mode();
    if (lo.keep) { if (const int rf = local_train_mode_refusal(d, "dep_rnn_forward", mode)) return rf; }
    if (const int rf = ragged_mode_refusal("dep_rnn_forward_varlen", lengths, mode)) return rf;
    const RnnPlan p = make_plan(d, lo, mode, dep_exclusive_on(), lengths != nullptr);
    DEP_CHECK_ARG(x && weights && reserve && workspace);
    DEP_CHECK_ARG(!(pooled && (d->cell != DEP_CELL_GRU || d->pool == DEP_POOL_NONE)));
    if (reserve_bytes < lo.reserve_floats * sizeof(float) || workspace_bytes < lo.ws_floats * sizeof(float)) {
        dep_set_error("dep_rnn_forward: reserve/workspace too small (%zu/%zu given, %zu/%zu needed)", reserve_bytes,
                      workspace_bytes, lo.reserve_floats * sizeof(float), lo.ws_floats * sizeof(float));
        return DEP_ERR_WORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    float* R = (float*)reserve; float* W = (float*)workspace;
    const int B = d->B, T = d->T, H = d->H, D = d->dirs, G = lo.G, L = d->L;
    const int BTr = (int)lo.BT;
    // the unsplit projections' scratch (the weight's stage image of gemm_bf16x3_nt_dma): the split-K region, idle during the forward
    DepGemmOpts proj; proj.scratch = W + lo.gemm; proj.scratch_bytes = lo.gemm_bytes;
    float* const gi = W + lo.gi;
    int rc;
    if (lo.cluster || lo.cluster_fwd) { rc = dep_cluster_reset_status(W + lo.xbuf, s); if (rc) return rc; }
    if (p.bf16st && (!p.excl || y)) {
        dep_set_error("dep_rnn_forward: bf16-storage mode (dep_set_gemm_mode(3)) runs the exclusive fused forward only (dep_rnn_set_exclusive(1)) "
                      "and has no fp32 copy of the output sequence (y must be NULL)");
        return DEP_ERR_ARG;
    }
    record_reserve_tag(reserve, p.tag);
    // Dropout-only: where a layer's output sequence goes when the reserve does not keep it.  The cluster BiLSTM sweep and the fused
    // GRU forward take a null pointer (nothing written); the other sweeps read their own output back (h_{t-1}, the pool) and get the
    // workspace's dX region, idle in a forward; the top layer of a pooled GRU writes straight into the caller's y when one is given.
    auto yout = [&](int l, bool null_ok) -> float* {
        if (lo.y[l] != NOT_KEPT) return R + lo.y[l];
        if (l == L - 1 && y) return y;
        return null_ok ? nullptr : W + lo.dx[0];
    };
    const bool ytop_kept = lo.y[L - 1] != NOT_KEPT;
    const float pool_scale = d->pool == DEP_POOL_MEAN ? 1.0f / (float)T : 1.0f;
    // layer l's sweep; only_if: as a fallback launch behind the fused one, which runs only when that device word is set
    auto sweep_args = [&](int l, const unsigned* only_if) {
        dep_sweep_args a{};
        a.B = B; a.T = T; a.H = H; a.cell = d->cell; a.dirs = D; a.training = d->training; a.impl = d->impl;
        a.split = ((lo.cluster || lo.cluster_fwd || lo.local_lstm) && p.split) ? 1 : 0;
        for (int dd = 0; dd < D; ++dd) {
            const float* const* wl = weights + (size_t)(l * D + dd) * 4;
            a.w_hh[dd] = wl[1]; a.b_hh[dd] = wl[3]; a.wp[dd] = R + lo.wp[l][dd];
        }
        const bool dropl = lo.drop && l < L - 1;
        a.gi = gi; a.y = yout(l, (p.fwd == FWD_CLUSTER_LSTM || p.fwd == FWD_LOCAL_LSTM) && dropl); a.ldy = D * H;
        a.ydrop = dropl ? R + lo.ydrop[l] : nullptr;
        a.drop_p = dropl ? d->dropout_p : 0.f; a.seed = d->seed; a.site = DEP_SITE_RNN0 + l;
        a.pooled = l == L - 1 ? pooled : nullptr;
        a.pool_scale = pool_scale;
        a.h_n = h_n ? h_n + (size_t)l * D * B * H : nullptr;
        // layer l's slice of the state arrays, ordered like h_n (a non-NULL member implies the tile / generic sweeps, or hx on the
        // per-layer cluster forward of impl 4 / 5: state_refusal)
        a.hx = st.hx ? st.hx + (size_t)l * D * B * H : nullptr;
        a.cx = st.cx ? st.cx + (size_t)l * D * B * H : nullptr;
        a.c_n = st.c_n ? st.c_n + (size_t)l * D * B * H : nullptr;
        if (lo.keep) { a.sv0 = R + lo.sv[l][0]; a.sv1 = R + lo.sv[l][1]; a.sv2 = R + lo.sv[l][2]; a.sv3 = R + lo.sv[l][3]; }
        a.only_if = only_if; a.stream = s; a.sv16 = p.sv16_fwd ? 1 : 0;
        a.lengths = lengths; a.pool_mean = d->pool == DEP_POOL_MEAN ? 1 : 0;
        // one exchange-header slot per layer, all zeroed by the call's one memset; the fused launch has slot 0, its fallbacks 1 + l
        a.hdr_slot = only_if ? 1 + l : (l < DEP_HDR_SLOTS ? l : 0); a.hdr_clean = only_if || l < DEP_HDR_SLOTS;
        return a;
    };
    if (p.fwd == FWD_FUSED2) {
        // both layers in one launch: layer 1 runs one step behind layer 0 and takes its input straight from the exchanged
        // h0_t (no layer-1 input-projection GEMM, no GI round trip through HBM for it)
        const float* const* w0 = weights; const float* const* w1 = weights + 4;
        for (int k = 0; k < 4; ++k) DEP_CHECK_ARG(w0[k] && w1[k]);
        {   // every weight image of the step in one launch: W_hh(l0), W_hh(l1), W_ih(l1) forward images; the backward's two
            const float* srcs[5] = {w0[1], w1[1], w1[0], w0[1], w1[1]};
            float* dsts[5] = {R + lo.wp[0][0], R + lo.wp[1][0], W + lo.wih_img, R + lo.wpT[0][0], R + lo.wpT[1][0]};
            const int kinds[5] = {0, 0, 0, 1, 1};
            rc = dep_pack_cluster_split_multi(p.whh_bwd == WHH_BWD_SPLIT ? 5 : 3, srcs, dsts, kinds, H, s); if (rc) return rc;
        }
        rc = dep_gemm_internal(0, 1, BTr, G * H, d->F, x, d->F, w0[0], d->F, gi, G * H, w0[2], 0.f, 0, 0, nullptr, 0, proj, s);
        if (rc) return rc;
        dep_fused2_args f{};
        f.B = B; f.T = T; f.training = d->training;
        f.wp0 = R + lo.wp[0][0]; f.wp1 = R + lo.wp[1][0]; f.wpi = W + lo.wih_img;
        f.b_hh0 = w0[3]; f.b_ih1 = w1[2]; f.b_hh1 = w1[3];
        f.ostride = (lo.BT * H + 63) / 64 * 64;
        f.gi = gi; f.y0 = lo.donly ? nullptr : R + lo.y[0]; f.y0d = (lo.drop && !lo.donly) ? R + lo.ydrop[0] : nullptr; f.y1 = yout(1, true);
        f.drop_p = lo.drop ? d->dropout_p : 0.f; f.seed = d->seed; f.site = DEP_SITE_RNN0;
        f.pooled = pooled; f.pool_scale = pool_scale;
        f.hn0 = h_n; f.hn1 = h_n ? h_n + (size_t)B * H : nullptr;
        for (int l = 0; l < 2; ++l) for (int k = 0; k < 4; ++k) f.sv[l][k] = lo.keep ? R + lo.sv[l][k] : nullptr;
        f.stream = s;
        f.soft_fallback = p.bf16st ? 0 : 1;           // (the tolerant per-layer kernels have no bf16-storage variant: a failed hello raises the status)
        f.sv16 = p.sv16 ? 1 : 0; f.bf16st = p.bf16st ? 1 : 0;
        f.hdr_clean = 1;                                   // dep_cluster_reset_status above zeroed every header slot
        rc = dep_launch_fused2_fwd(f, W + lo.xbuf, lo.xbuf_bytes); if (rc) return rc;
        // Fallback, decided ON THE DEVICE (no host synchronisation, identical on every data-parallel rank): the launch above
        // needs every CU to itself; if a foreign workgroup kept its clusters from assembling it has set the workspace's soft
        // flag and left.  The per-layer kernels that tolerate co-scheduled work are enqueued behind it in any case and return
        // at entry unless the flag is set (3 near-empty launches per forward, ~10 us); they write the same reserve layout, so
        // the backward does not care which of the two produced it.
        const unsigned* soft = reinterpret_cast<const unsigned*>(W + lo.xbuf) + 1;
        for (int l = 0; l < 2 && !p.bf16st; ++l) {
            if (l == 1) {
                const LayerIn in = layer_input(d, lo, x, R, 1);
                DepGemmOpts fallback = proj; fallback.only_if = soft;
                rc = dep_gemm_internal(0, 1, BTr, G * H, in.K, in.p, in.K, w1[0], in.K, gi, G * H, w1[2], 0.f, 0, 0, nullptr, 0, fallback, s);
                if (rc) return rc;
            }
            rc = dep_launch_cluster_fwd(sweep_args(l, soft), W + lo.xbuf, lo.xbuf_bytes); if (rc) return rc;
        }
        if (y && ytop_kept) { rc = dep_axpby(R + lo.y[1], y, (long)lo.BT * H, 1.f, 0.f, s); if (rc) return rc; }
        return DEP_OK;
    }
    if (D == 2) {
        // gather every layer's direction-stacked W_ih and folded bias (b_ih [+ b_hh]) in one launch (16 jobs at a time)
        const float* src[16]; const float* add[16]; float* dst[16]; long cnt[16]; int nj = 0;
        for (int l = 0; l < L; ++l) {
            const int Kl = layer_input(d, lo, x, R, l).K;
            for (int dd = 0; dd < D; ++dd) {
                const float* const* wl = weights + (size_t)(l * D + dd) * 4;
                DEP_CHECK_ARG(wl[0] && wl[1] && wl[2] && wl[3]);
                src[nj] = wl[0]; add[nj] = nullptr; dst[nj] = R + lo.wstack[l] + (size_t)dd * G * H * Kl; cnt[nj++] = (long)G * H * Kl;
                src[nj] = wl[2]; add[nj] = d->cell == DEP_CELL_LSTM ? wl[3] : nullptr; dst[nj] = R + lo.bstack[l] + (size_t)dd * G * H; cnt[nj++] = (long)G * H;
                if (nj == 16) { rc = dep_multi_copy(nj, src, add, dst, cnt, s); if (rc) return rc; nj = 0; }
            }
        }
        if (nj) { rc = dep_multi_copy(nj, src, add, dst, cnt, s); if (rc) return rc; }
    }
    for (int l = 0; l < L; ++l) {
        const LayerIn in = layer_input(d, lo, x, R, l);
        const int Kl = in.K;
        const bool stacked = D == 2;                   // both directions' projections as one GEMM over stacked weights
        for (int dd = 0; dd < D; ++dd) {
            const float* const* wl = weights + (size_t)(l * D + dd) * 4;
            DEP_CHECK_ARG(wl[0] && wl[1] && wl[2] && wl[3]);
            // recurrent weight images in MFMA fragment order (precision / clustering decide the format: RnnPlan)
            float* const wp = R + lo.wp[l][dd]; float* const wpT = lo.wpT[l][dd] == NOT_KEPT ? nullptr : R + lo.wpT[l][dd];
            // (impl 8 / 9: the transposed image is the backward's, packed only by the forward a backward follows)
            if (p.whh_f32) { rc = dep_pack_whh(wl[1], wp, (lo.local_lstm && !(lo.local_train && lo.keep)) ? nullptr : wpT, G, H, s); if (rc) return rc; }
            rc = p.whh_fwd == WHH_LSTM_PAIR ? dep_pack_cluster_lstm_split(wl[1], wp, lo.keep ? wpT : nullptr, H, s)
               : p.whh_fwd == WHH_SPLIT16 ? dep_pack_cluster16_fwd_split(wl[1], wp, H, s)
               : p.whh_fwd == WHH_SPLIT32 ? dep_pack_cluster_fwd_split(wl[1], wp, H, s) : DEP_OK;
            if (rc) return rc;
            // the cluster backward wants its own member-sliced image
            rc = p.whh_bwd == WHH_BWD_SPLIT ? dep_pack_cluster_bwd_split(wl[1], wpT, H, s)
               : p.whh_bwd == WHH_BWD_F32 ? dep_pack_cluster_bwd(wl[1], wpT, G, H, s) : DEP_OK;
            if (rc) return rc;
            const float* bias = wl[2];
            if (stacked) continue;                     // weights and biases were stacked above; the GEMM follows the loop
            if (d->cell == DEP_CELL_LSTM) {          // both biases fold into the projection
                float* tb = W + lo.biastmp;
                rc = dep_axpby(wl[2], tb, (long)G * H, 1.f, 0.f, s); if (rc) return rc;
                rc = dep_axpby(wl[3], tb, (long)G * H, 1.f, 1.f, s); if (rc) return rc;
                bias = tb;
            }
            rc = dep_gemm_internal(0, 1, BTr, G * H, Kl, in.p, Kl, wl[0], Kl, gi + (size_t)dd * G * H, D * G * H, bias,
                                   0.f, 0, 0, nullptr, 0, proj, s);
            if (rc) return rc;
            // the bias scratch is reused by the next direction: stream order keeps this safe
        }
        if (stacked) {
            rc = dep_gemm_internal(0, 1, BTr, D * G * H, Kl, in.p, Kl, R + lo.wstack[l], Kl, gi, D * G * H, R + lo.bstack[l],
                                   0.f, 0, 0, nullptr, 0, proj, s);
            if (rc) return rc;
        }
        dep_sweep_args a = sweep_args(l, nullptr);
        if (p.fwd == FWD_CLUSTER_GRU && a.hx && a.h_n && T == 1 && a.hx < a.h_n + (size_t)D * B * H && a.h_n < a.hx + (size_t)D * B * H) {
            // h_n over hx at T = 1: the sweep has no exchange, so nothing keeps a member's h_n store behind another member's read of that
            // row of hx.  The kernel reads a copy (T >= 2: every member reads hx before it raises its first flag, and no member stores
            // h_n before it has seen all of them)
            if (hipMemcpyAsync(W + lo.hxstage, a.hx, (size_t)D * B * H * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess) {
                dep_set_error("dep_rnn_forward_state: staging copy of hx failed"); return DEP_ERR_HIP;
            }
            a.hx = W + lo.hxstage;
        }
        rc = p.fwd == FWD_CLUSTER16 ? dep_launch_cluster16_fwd(a, W + lo.xbuf, lo.xbuf_bytes)
           : p.fwd == FWD_CLUSTER_LSTM ? dep_launch_cluster_lstm_fwd(a, W + lo.xbuf, lo.xbuf_bytes)
           : p.fwd == FWD_LOCAL_LSTM ? dep_launch_local_lstm_fwd(a)
           : p.fwd == FWD_CLUSTER_GRU ? dep_launch_cluster_fwd(a, W + lo.xbuf, lo.xbuf_bytes) : dep_launch_sweep_fwd(a);
        if (rc) return rc;
    }
    if (y && ytop_kept) {
        rc = dep_axpby(R + lo.y[L - 1], y, (long)lo.BT * D * H, 1.f, 0.f, s);
        if (rc) return rc;
    }
    return DEP_OK;
}

extern "C" int dep_rnn_forward(const dep_rnn_desc* d, const float* x, const float* const* weights, float* y,
                               float* pooled, float* h_n, void* reserve, size_t reserve_bytes, void* workspace,
                               size_t workspace_bytes, void* stream) {
    return rnn_forward_impl(d, x, nullptr, weights, y, pooled, h_n, nullptr, reserve, reserve_bytes, workspace, workspace_bytes, stream);
}

extern "C" int dep_rnn_forward_state(const dep_rnn_desc* d, const float* x, const float* const* weights, float* y,
                                     float* pooled, float* h_n, const dep_rnn_state* st, void* reserve, size_t reserve_bytes,
                                     void* workspace, size_t workspace_bytes, void* stream) {
    return rnn_forward_impl(d, x, nullptr, weights, y, pooled, h_n, st, reserve, reserve_bytes, workspace, workspace_bytes, stream);
}

extern "C" int dep_rnn_forward_varlen(const dep_rnn_desc* d, const float* x, const int32_t* lengths, const float* const* weights,
                                      float* y, float* pooled, float* h_n, void* reserve, size_t reserve_bytes, void* workspace,
                                      size_t workspace_bytes, void* stream) {
    DEP_CHECK_ARG(lengths);
    return rnn_forward_impl(d, x, lengths, weights, y, pooled, h_n, nullptr, reserve, reserve_bytes, workspace, workspace_bytes, stream);
}

extern "C" int dep_rnn_forward_state_varlen(const dep_rnn_desc* d, const float* x, const int32_t* lengths, const float* const* weights,
                                            float* y, float* pooled, float* h_n, const dep_rnn_state* st, void* reserve, size_t reserve_bytes,
                                            void* workspace, size_t workspace_bytes, void* stream) {
    if (!lengths) {
        dep_set_error("dep_rnn_forward_state_varlen: lengths is NULL; the dense call with a state is dep_rnn_forward_state");
        return DEP_ERR_ARG;
    }
    return rnn_forward_impl(d, x, lengths, weights, y, pooled, h_n, st, reserve, reserve_bytes, workspace, workspace_bytes, stream);
}

static int rnn_backward_impl(const dep_rnn_desc* d, const float* x, const int32_t* lengths, const float* const* weights, const float* dy,
                             const float* dpooled, const float* dh_n, const dep_rnn_state_grad* state, float* const* dweights, float* dx,
                             void* reserve, size_t reserve_bytes, void* workspace, size_t workspace_bytes,
                             void* stream, const dep_grad_sync* gs) {
    Layout lo;
    if (const int rf = percluster_refusal(d, "dep_rnn_backward")) return rf;
    if (const int rf = bicluster_refusal(d, "dep_rnn_backward")) return rf;
    if (d && local_impl(d)) {
        if (const int rf = local_refusal(d, "dep_rnn_backward")) return rf;
        dep_set_error("dep_rnn_backward: impl = 8 (the exchange-free per-layer LSTM forward) has no backward: its forwards run in DEP_RUN_EVAL and "
                      "DEP_RUN_DROPOUT_ONLY and save no gates; train on impl 0 .. 3");
        return DEP_ERR_ARG;
    }
    if (d && bicluster_train_impl(d) && dep_get_gemm_mode() == 3 && bicluster_ok(d)) {
        dep_set_error("dep_rnn_backward: impl = 7 (the per-layer cluster sweeps of a bidirectional GRU) has no backward in GEMM mode 3: the bidirectional "
                      "sweep writes fp32 gate-gradient rows, not the PK image whose hi rows that mode reads; modes 0, 1 and 2 run (dep_set_gemm_mode)");
        return DEP_ERR_ARG;
    }
    if (d && d->impl == 6 && !dep_sweep_use_mfma(d->H, d->impl)) {
        dep_set_error("dep_rnn_backward: impl = 6 runs the tile-MFMA backward of the bidirectional GRU, which tiles H up to 256; H = %d has the forward only", d->H);
        return DEP_ERR_ARG;
    }
    if (const int rf = local_train_refusal(d, "dep_rnn_backward")) return rf;
    if (const int rf = bigru_refusal(d, "dep_rnn_backward")) return rf;
    DEP_CHECK_ARG(make_layout(d, lo));
    const dep_rnn_state_grad st = state ? *state : dep_rnn_state_grad{nullptr, nullptr, nullptr, nullptr, nullptr};      // NULL and a struct of NULLs are the plain call
    const bool has_state = st.hx || st.cx || st.dc_n || st.dhx || st.dcx;
    const int mode = dep_get_gemm_mode();
    if (const int rf = state_refusal(d, lo, lengths ? "dep_rnn_backward_state_varlen" : "dep_rnn_backward_state", has_state, st.cx || st.dc_n || st.dcx, true, mode)) return rf;
    // the dense call's dW_hh state term reads the gate-gradient rows of one time step as a (B x rows) matrix of row stride T * ldg
    // (a ragged call gathers each row's own step with 64-bit offsets, dep_state_dwhh_ragged: no such bound)
    DEP_CHECK_ARG(!st.hx || lengths || (long)d->T * d->dirs * (d->cell == DEP_CELL_GRU ? 3 : 4) * d->H <= 0x7fffffffL);
    // (the cluster sweeps' rows are 4H wide; the recurrent term of dhx reads the t = 0 rows the same way, dense or ragged)
    DEP_CHECK_ARG(!(has_state && lo.cluster) || (long)d->T * 4 * d->H <= 0x7fffffffL);
    DEP_CHECK_ARG(!(has_state && lo.cluster_bwd2) || (long)d->T * 6 * d->H <= 0x7fffffffL);      // (impl 7: the tile BiGRU's 6H-wide rows)
    if (lo.keep) { if (const int rf = local_train_mode_refusal(d, "dep_rnn_backward", mode)) return rf; }      // (another run mode: the message below)
    if (const int rf = ragged_mode_refusal("dep_rnn_backward_varlen", lengths, mode)) return rf;
    const RnnPlan p = make_plan(d, lo, mode, dep_exclusive_on(), lengths != nullptr);
    if (d->training != DEP_RUN_TRAIN) {
        dep_set_error("dep_rnn_backward: the descriptor's run mode is %d; a backward needs a DEP_RUN_TRAIN (1) forward's reserve%s", d->training,
                      d->training == DEP_RUN_DROPOUT_ONLY ? " (DEP_RUN_DROPOUT_ONLY keeps no saved gates)" : "");
        return DEP_ERR_ARG;
    }
    int rc = reserve_tag_refusal(reserve, p.tag, TAG_DONLY); if (rc) return rc;
    DEP_CHECK_ARG(x && weights && dweights && reserve && workspace);
    DEP_CHECK_ARG(dy || dpooled || dh_n || st.dc_n);
    DEP_CHECK_ARG(!(dpooled && (d->cell != DEP_CELL_GRU || d->pool == DEP_POOL_NONE)));
    if (reserve_bytes < lo.reserve_floats * sizeof(float) || workspace_bytes < lo.ws_floats * sizeof(float)) {
        dep_set_error("dep_rnn_backward: reserve/workspace too small");
        return DEP_ERR_WORKSPACE;
    }
    // the cluster kernels must match the images and saved gates dep_rnn_forward left
    if (lo.cluster || lo.cluster_bwd2 || lo.local_train) { rc = reserve_tag_refusal(reserve, p.tag, TAG_SPLIT | TAG_BF16ST | TAG_SV16); if (rc) return rc; }
    hipStream_t s = (hipStream_t)stream;
    float* R = (float*)reserve; float* W = (float*)workspace;
    const int B = d->B, T = d->T, H = d->H, D = d->dirs, G = lo.G, L = d->L;
    const int BTr = (int)lo.BT;
    const bool gru = d->cell == DEP_CELL_GRU;
    void* gws = W + lo.gemm; const size_t gwsb = lo.gemm_bytes;
    // (dX's weight image shares the region with the split-K partials of the contractions enqueued behind it: stream order keeps them apart)
    const float pool_scale = d->pool == DEP_POOL_MEAN ? 1.0f / (float)T : 1.0f;
    const int ldg = p.dg4 ? 4 * H : D * G * H;                  // row stride of the gate-gradient arrays
    const char* const no_pk = "dep_rnn_backward: bf16-storage mode needs the pre-split gate-gradient path (aligned operands, DEP_DGI_PK not 0, contractions above the split threshold)";
    // The fused two-layer backward (rnn_fused2_bwd.hip; round 5: all-gather form): both layers' BPTT in ONE launch, layer 1's dX -- the gradient
    // entering layer 0 -- formed in-kernel.  It writes the same gate-gradient arrays as the per-layer sweeps (4H-wide rows, PK image when the
    // contractions take it), so everything behind the sweeps -- bias finish, dW GEMMs (paired), layer 0's dX, the gradient ranges -- is the
    // per-layer loop below with the sweep launches and layer 1's dX GEMM left out.  DEP_FUSED2_BWD=1 / 0.
    const bool fused = p.bwd == BWD_FUSED2;
    auto al16 = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
    // Round 4: the sweep writes the gate gradients as the PK image (rows (t even, t + 1) = (hi, lo) bf16 pairs of both steps,
    // gemm_bf16x3.hip) -- the three contractions that read them (dX, dW_ih, dW_hh) then stage them without converting; same
    // bytes, same bits.  Only when all three really run the three-term kernel on its vector path: may layer l's be?  (dxl: its dX,
    // if formed.  The BiLSTM cluster sweep -- both directions in one launch, direction-stacked contractions -- takes the same image.)
    auto pk_ok = [&](int l, const float* dxl) {
        const LayerIn in = layer_input(d, lo, x, R, l);
        const int M = D * G * H;
        bool ok = p.pk && (in.K % 4 == 0) && al16(in.p) &&
                  (gru ? al16(weights[(size_t)l * 4]) && al16(dweights[(size_t)l * 4]) : lo.wstack[l] != 0 && al16(W + lo.dwstack)) &&
                  dep_gemm_uses_bf16x3(M, in.K, BTr, 0) && dep_gemm_uses_bf16x3(G * H, H, BTr, T) &&
                  (!dxl || (dep_gemm_uses_bf16x3(BTr, in.K, M, 0) && al16(dxl)));
        for (int dd = 0; dd < D && ok; ++dd) ok = al16(dweights[(size_t)(l * D + dd) * 4 + 1]);
        return ok;
    };
    bool fused_pk = false;
    if (fused) {
        const float* const* w0 = weights; const float* const* w1 = weights + 4;
        float* const* g0 = dweights; float* const* g1 = dweights + 4;
        for (int k = 0; k < 4; ++k) DEP_CHECK_ARG(w0[k] && w1[k] && g0[k] && g1[k]);
        fused_pk = p.sv16 && pk_ok(1, nullptr) && pk_ok(0, dx);      // one kernel writes both layers: both or neither
        rc = dep_pack_cluster_bwd_split(w1[0], W + lo.wih_img, H, s); if (rc) return rc;
        dep_fused2_bwd_args f{};
        f.B = B; f.T = T;
        f.wh1 = R + lo.wpT[1][0]; f.wi1 = W + lo.wih_img; f.wh0 = R + lo.wpT[0][0];
        f.y1 = R + lo.y[1]; f.y0 = R + lo.y[0]; f.sv1 = R + lo.sv[1][0]; f.sv0 = R + lo.sv[0][0];
        f.svstride = (lo.BT * H + 63) / 64 * 64;
        f.dy = dy; f.dpooled = dpooled; f.pool_scale = pool_scale;
        f.dhn1 = dh_n ? dh_n + (size_t)B * H : nullptr; f.dhn0 = dh_n;
        f.drop_p = lo.drop ? d->dropout_p : 0.f; f.seed = d->seed; f.site = DEP_SITE_RNN0;
        f.dgi1 = W + lo.gi; f.dgi0 = W + lo.gi2;
        f.dghn1 = p.dg4 ? f.dgi1 + 3 * H : W + lo.dghn; f.dghn0 = p.dg4 ? f.dgi0 + 3 * H : W + lo.dghn2;
        f.lddg = ldg; f.lddghn = p.dg4 ? ldg : H;
        f.dbpart1 = W + lo.dbpart; f.dbpart0 = W + lo.dbpart2; f.dbpart_rows = lo.nwg; f.stream = s;
        if (p.bf16st && !fused_pk) { dep_set_error(no_pk); return DEP_ERR_ARG; }
        f.sv16 = p.sv16 ? 1 : 0; f.dg_pk = fused_pk ? 1 : 0; f.bf16st = p.bf16st ? 1 : 0;
        rc = dep_launch_fused2_bwd(f, W + lo.xbuf, lo.xbuf_bytes); if (rc) return rc;
    }
    // layer l's sweep (fused: not launched, but dep_finish_db and the contractions read where its gate gradients are from the same struct)
    auto sweep_args = [&](int l, bool pk) {
        const bool top = l == L - 1;
        const bool second = fused && l == 0;                  // (the fused launch left both layers' gate gradients behind)
        dep_sweep_bwd_args a{};
        a.B = B; a.T = T; a.H = H; a.cell = d->cell; a.dirs = D; a.impl = d->impl;
        a.split = ((lo.cluster || lo.cluster_bwd2 || lo.local_train) && p.split) ? 1 : 0;
        for (int dd = 0; dd < D; ++dd) {
            const float* const* wl = weights + (size_t)(l * D + dd) * 4;
            a.w_hh[dd] = wl[1]; a.wpT[dd] = R + lo.wpT[l][dd];
        }
        a.y = R + lo.y[l]; a.ldy = D * H;
        if (top) { a.dy = dy; a.drop_p = 0.f; }
        else { a.dy = W + lo.dx[(l + 1) & 1]; a.drop_p = lo.drop ? d->dropout_p : 0.f; }
        a.lddy = D * H; a.seed = d->seed; a.site = DEP_SITE_RNN0 + l;
        a.dpooled = top ? dpooled : nullptr;
        a.pool_scale = pool_scale;
        a.dh_n = dh_n ? dh_n + (size_t)l * D * B * H : nullptr;
        {   // layer l's slice of the state arrays, ordered like h_n (a non-NULL member implies the tile / generic sweeps, or hx / dhx on impl 5: state_refusal)
            const size_t so = (size_t)l * D * B * H;
            a.hx = st.hx ? st.hx + so : nullptr; a.cx = st.cx ? st.cx + so : nullptr; a.dc_n = st.dc_n ? st.dc_n + so : nullptr;
            a.dhx = st.dhx ? st.dhx + so : nullptr; a.dcx = st.dcx ? st.dcx + so : nullptr;
        }
        a.sv0 = R + lo.sv[l][0]; a.sv1 = R + lo.sv[l][1]; a.sv2 = R + lo.sv[l][2]; a.sv3 = R + lo.sv[l][3];
        a.dgi = W + (second ? lo.gi2 : lo.gi);
        a.dghn = p.dg4 ? a.dgi + 3 * H : W + (second ? lo.dghn2 : lo.dghn);
        a.lddg = p.dg4 ? ldg : 0; a.lddghn = p.dg4 ? ldg : 0;
        a.dbpart = W + (second ? lo.dbpart2 : lo.dbpart); a.dbpart_rows = D * lo.nwg; a.stream = s;
        // one exchange-header slot per layer, all zeroed by the call's one memset; layers past the slots share slot 0 and clear it
        // themselves.  The backward walks DOWN, so in a stack of more than DEP_HDR_SLOTS layers those layers have used slot 0 by the
        // time layer 0 comes to it: it is not clean then (flags only grow: stale ones let every wait of the sweep pass at once)
        a.hdr_slot = l < DEP_HDR_SLOTS ? l : 0; a.hdr_clean = l < DEP_HDR_SLOTS && !(l == 0 && L > DEP_HDR_SLOTS);
        a.dg_pk = pk ? 1 : 0; a.bf16st = p.bf16st ? 1 : 0; a.sv16 = p.sv16 ? 1 : 0;
        a.lengths = lengths; a.pool_mean = d->pool == DEP_POOL_MEAN ? 1 : 0;
        return a;
    };
    float* pending_ptr = nullptr; long pending_n = 0;      // data parallel: a finished layer's gradient range waiting for the next sweep to be enqueued
    if ((lo.cluster || lo.cluster_bwd2) && !fused) { rc = dep_cluster_reset_flags(W + lo.xbuf, s); if (rc) return rc; }      // every layer's header slot in one memset (the status words stay)
    for (int l = L - 1; l >= 0; --l) {
        const LayerIn lin = layer_input(d, lo, x, R, l);
        const float* const in = lin.p; const int Kl = lin.K;
        float* dxl = l == 0 ? dx : (fused ? nullptr : W + lo.dx[l & 1]);      // (fused: the gradient entering layer 0 never left the chip)
        // a call with a state on the cluster sweeps (impl 5) takes the fp32 gate-gradient rows odd T and H = 512 take: the t = 0 rows are
        // operands of the hx term of dW_hh and of the recurrent term of dhx below (the contractions are then the unpaired ones)
        const bool pk = fused ? fused_pk : (pk_ok(l, dxl) && !(has_state && lo.cluster));
        if (p.bf16st && !pk) { dep_set_error(no_pk); return DEP_ERR_ARG; }
        const dep_sweep_bwd_args a = sweep_args(l, pk);
        float* const dgi = a.dgi; float* const dghn = a.dghn;
        if (!fused) {
            rc = p.bwd == BWD_CLUSTER_LSTM ? dep_launch_cluster_lstm_bwd(a, W + lo.xbuf, lo.xbuf_bytes)
               : p.bwd == BWD_CLUSTER_GRU ? dep_launch_cluster_bwd(a, W + lo.xbuf, lo.xbuf_bytes)
               : p.bwd == BWD_LOCAL_LSTM ? dep_launch_local_lstm_bwd(a) : dep_launch_sweep_bwd(a);
            if (rc) return rc;
        }
        if (pending_ptr) {
            // the layer above's gradient range: the event recorded here completes with this sweep, the all-reduce then runs
            // beside this layer's GEMMs.  A cluster sweep needs every one of its workgroups resident (one per CU, most of a CU's
            // registers and LDS): a collective kernel that holds CUs when the sweep is dispatched delays the members that
            // cannot be placed -- and with them the whole launch -- until the collective's peers on the other GPUs let it finish.
            rc = dep_comm_enqueue_after((dep_comm*)gs->comm, pending_ptr, pending_n, s, (hipStream_t)gs->comm_stream);
            if (rc) return rc;
            pending_ptr = nullptr;
        }
        float* dbi[2]; float* dbh[2];
        for (int dd = 0; dd < D; ++dd) {
            float* const* gl = dweights + (size_t)(l * D + dd) * 4;
            DEP_CHECK_ARG(gl[0] && gl[1] && gl[2] && gl[3]);
            dbi[dd] = gl[2]; dbh[dd] = gl[3];
        }
        rc = dep_finish_db(a, dbi, dbh);
        if (rc) return rc;
        // A = the PK gate gradients in dX, dW_ih and dW_hh below.  Round 6: the single-product modes (dep_set_gemm_mode(2 / 3)) read the sweep's PK
        // image through its hi rows (FMT_PKH) on every stack (the same bf16 values their on-the-fly conversion formed: bit-identical, without the fp32
        // staging path that made cfg3's weight gradients slower in that mode than with three products)
        DepGemmOpts go; go.scratch = gws; go.scratch_bytes = gwsb;
        if (pk) go.fmt_a = p.pk_fmt;
        // dX (B*T, Kl) (+)= dG * W_ih first: it is the only product the next layer's sweep waits for
        const bool stacked = D == 2 && lo.wstack[l] != 0;
        if (dxl && stacked) {
            // dX = [dG_fwd | dG_bwd] [W_ih(fwd); W_ih(bwd)]: one contraction over K = 2 G H (the forward left the stacked copy in
            // the reserve) instead of two with a read-modify-write of dX in between
            rc = dep_gemm_internal(0, 0, BTr, Kl, D * G * H, dgi, ldg, R + lo.wstack[l], Kl, dxl, Kl, nullptr, 0.f, 0, 0, nullptr, 0, go, s);
            if (rc) return rc;
        } else if (dxl) {
            for (int dd = 0; dd < D; ++dd) {
                const float* const* wl = weights + (size_t)(l * D + dd) * 4;
                rc = dep_gemm_internal(0, 0, BTr, Kl, G * H, dgi + (size_t)dd * G * H, ldg, wl[0], Kl, dxl, Kl, nullptr,
                                       dd == 0 ? 0.f : 1.f, 0, 0, nullptr, 0, go, s);
                if (rc) return rc;
            }
        }
        if (stacked) {
            // dW_ih of both directions: (2 G H x Kl) = dG^T in, the input read once; rows [0, G H) / [G H, 2 G H) are the two tensors
            float* dws = W + lo.dwstack;
            rc = dep_gemm_internal(1, 0, D * G * H, Kl, BTr, dgi, ldg, in, Kl, dws, Kl, nullptr, 0.f, 0, 0, gws, gwsb, go, s);
            if (rc) return rc;
            const float* src[2]; float* dst[2]; long cnt[2];
            for (int dd = 0; dd < D; ++dd) {
                src[dd] = dws + (size_t)dd * G * H * Kl; dst[dd] = (dweights + (size_t)(l * D + dd) * 4)[0]; cnt[dd] = (long)G * H * Kl;
            }
            rc = dep_multi_copy(D, src, nullptr, dst, cnt, s); if (rc) return rc;
        }
        bool paired = false;
        // (the split-K target follows the layer's SHAPE, not whether the pair really runs: the fp32-row path (DEP_DGI_PK=0) and the unpaired path
        // (DEP_DW_PAIR=0) must keep summing in the same order as the pair -- tests/test_presplit_gpu.py holds them bit-identical)
        const bool pair_layer = p.dw_pair && Kl == H;
        const bool pair_shape = pair_layer && pk && !p.bf16st;
        DepGemmOpts dwo = go; dwo.split_target = pair_layer ? 512 : 0;       // the weight gradients below
        if (pair_shape) {
            // Round 5: dW_ih and dW_hh of this layer in ONE launch -- both read the PK gate gradients, [dr | dz] are the same bytes
            // (gemm_bf16x3_tn_pair; bit-identical to the two calls below, which remain the path for every other configuration)
            float* const* gl = dweights + (size_t)l * 4;
            DepGemmOpts po = dwo; po.skip_at = 2 * H; po.skip_by = H;       // problem 1 (dW_hh) reads [dr | dz] and [dn*r]
            const int pr = dep_gemm_tn_pair(G * H, H, BTr, dgi, dgi, ldg, in, Kl, 0, 0, R + lo.y[l], H, T, -1, gl[0], Kl, gl[1], H, po, gws, gwsb, s);
            if (pr < 0) return pr;
            paired = pr == 1;
        }
        bool paired_hh = false;
        if (pk && !gru) {
            // Round 5: dW_hh of the two directions of a BiLSTM layer (4H x H each: 254 tile-jobs, half of the persistent grid) as ONE paired launch;
            // tiles, K chunks and split-K order per direction are those of the single launches (bit-identical)
            float* const* gf = dweights + (size_t)(l * D) * 4; float* const* gb = dweights + (size_t)(l * D + 1) * 4;
            const int pr = dep_gemm_tn_pair(G * H, H, BTr, dgi, dgi + (size_t)G * H, ldg, R + lo.y[l], D * H, T, -1, R + lo.y[l] + H, D * H, T, 1,
                                            gf[1], H, gb[1], H, dwo, gws, gwsb, s);
            if (pr < 0) return pr;
            paired_hh = pr == 1;
        }
        for (int dd = 0; dd < D && !paired && !paired_hh; ++dd) {
            float* const* gl = dweights + (size_t)(l * D + dd) * 4;
            const float* dg = dgi + (size_t)dd * G * H;
            // dW_ih (G*H, Kl) = dG^T * in
            if (!stacked) {
                DepGemmOpts io = dwo; io.fmt_b = (p.bf16st && l > 0) ? FMT_BF16 : FMT_F32;       // the layer below's (dropped) output is a bf16 array
                rc = dep_gemm_internal(1, 0, G * H, Kl, BTr, dg, ldg, in, Kl, gl[0], Kl, nullptr, 0.f, 0, 0, gws, gwsb, io, s);
                if (rc) return rc;
            }
            DepGemmOpts ho = dwo; ho.fmt_b = p.bf16st ? FMT_BF16 : FMT_F32;          // dW_hh: B = this layer's bf16 output, shifted one step
            // dW_hh (G*H, H) = dGH^T * h_prev   (h_prev = layer output shifted by one step along the sweep)
            const float* yl = R + lo.y[l] + (size_t)dd * H;
            const int shift = dd == 0 ? -1 : 1;
            if (p.dg4 && dep_gemm_uses_bf16x3(3 * H, H, BTr, T)) {
                // ONE contraction over the 4H-wide rows: op(A) columns [dr | dz] and [dn*r] (the dn block in between is skipped by
                // the loader).  The separate (H x H) call for the n rows cost 100 us for a third of the (2H x H) call's 165 us work.
                DepGemmOpts so = ho; so.skip_at = 2 * H; so.skip_by = H;
                rc = dep_gemm_internal(1, 0, 3 * H, H, BTr, dg, ldg, yl, D * H, gl[1], H, nullptr, 0.f, T, shift, gws, gwsb, so, s);
                if (rc) return rc;
            } else if (gru) {
                rc = dep_gemm_internal(1, 0, 2 * H, H, BTr, dg, ldg, yl, D * H, gl[1], H, nullptr, 0.f, T, shift, gws, gwsb, ho, s);
                if (rc) return rc;
                // (the tile sweeps' dghn is (B*T, D*H), direction dd in columns [dd*H, (dd+1)*H); D = 1 unless the GRU is bidirectional)
                rc = dep_gemm_internal(1, 0, H, H, BTr, dghn + (size_t)dd * H, p.dg4 ? ldg : D * H, yl, D * H, gl[1] + (size_t)2 * H * H, H, nullptr,
                                       0.f, T, shift, gws, gwsb, ho, s);
                if (rc) return rc;
            } else {
                rc = dep_gemm_internal(1, 0, 4 * H, H, BTr, dg, ldg, yl, D * H, gl[1], H, nullptr, 0.f, T, shift, gws, gwsb, ho, s);
                if (rc) return rc;
            }
            if (a.hx) {
                // The initial state's term, dW_hh += dG[:, t0, :]^T hx: the shifted contractions above give sweep step 0 (t0 = 0; reverse
                // direction t0 = T-1) a zero h_prev.  Same blocks as above, K = B: op(A) = the gate-gradient rows at t0 (row stride
                // T * ld), B = this direction's hx slice; added (beta = 1) behind the main contraction, which wrote with beta = 0.
                // (state_refusal: the tile / generic sweeps ran, or the per-layer cluster sweep of impl 5 with pk = false: the rows are fp32 and
                // the contractions above unpaired.  Row strides are the sweep's own: the cluster layout's rows are 4H wide, dghn their block 3.)
                const float* hxd = a.hx + (size_t)dd * B * H;
                const int ldhn = p.dg4 ? ldg : D * H;
                const size_t t0 = dd == 0 ? 0 : (size_t)T - 1;
                if (lengths) {
                    // ragged: the first sweep step is per row (t0_b = 0; reverse direction len_b - 1, none for an empty row), so the rows
                    // cannot be one strided GEMM operand: a direct exact-fp32 kernel gathers them (fixed order over b, no workspace)
                    rc = dep_state_dwhh_ragged(dg, ldg, lengths, B, T, dd, hxd, gru ? 2 * H : 4 * H, H, gl[1], s);
                    if (rc) return rc;
                    if (gru) { rc = dep_state_dwhh_ragged(dghn + (size_t)dd * H, ldhn, lengths, B, T, dd, hxd, H, H, gl[1] + (size_t)2 * H * H, s); if (rc) return rc; }
                } else if (gru) {
                    rc = dep_gemm_internal(1, 0, 2 * H, H, B, dg + t0 * ldg, T * ldg, hxd, H, gl[1], H, nullptr, 1.f, 0, 0, gws, gwsb, ho, s);
                    if (rc) return rc;
                    rc = dep_gemm_internal(1, 0, H, H, B, dghn + (size_t)dd * H + t0 * ldhn, T * ldhn, hxd, H, gl[1] + (size_t)2 * H * H, H, nullptr,
                                           1.f, 0, 0, gws, gwsb, ho, s);
                    if (rc) return rc;
                } else {
                    rc = dep_gemm_internal(1, 0, 4 * H, H, B, dg + t0 * ldg, T * ldg, hxd, H, gl[1], H, nullptr, 1.f, 0, 0, gws, gwsb, ho, s);
                    if (rc) return rc;
                }
            }
        }
        if (a.dhx && p.bwd == BWD_CLUSTER_GRU && lo.cluster_bwd2) {
            // impl 7: the same two products per direction on the tile BiGRU's rows -- direction dd's [dr | dz] in columns [3 dd H, 3 dd H + 2H) of
            // dgi, its dn*r in columns [dd H, (dd+1) H) of dghn -- at the sweep's LAST step, t = 0 or (direction 1) T-1.  A ragged row whose last
            // sweep steps of direction 1 were dead has exact zeros there, and its stored dhx already holds the recurrent term (gathered in-kernel
            // at its first dead step), so one strided product serves dense and ragged.
            DepGemmOpts xo; xo.scratch = gws; xo.scratch_bytes = gwsb;
            for (int dd = 0; dd < D; ++dd) {
                const float* whh = weights[(size_t)(l * D + dd) * 4 + 1];
                const size_t tl = dd == 0 ? 0 : (size_t)T - 1;
                float* dhxd = a.dhx + (size_t)dd * B * H;
                rc = dep_gemm_internal(0, 0, B, H, 2 * H, dgi + (size_t)dd * G * H + tl * ldg, T * ldg, whh, H, dhxd, H, nullptr, 1.f, 0, 0, nullptr, 0, xo, s);
                if (rc) return rc;
                rc = dep_gemm_internal(0, 0, B, H, H, dghn + (size_t)dd * H + tl * D * H, T * D * H, whh + (size_t)2 * H * H, H, dhxd, H, nullptr, 1.f, 0, 0, nullptr, 0, xo, s);
                if (rc) return rc;
            }
        } else if (a.dhx && p.bwd == BWD_CLUSTER_GRU) {
            // The recurrent term of dhx: the sweep stored the direct term d_0 * z_0 (a dead ragged row: its dh_n); the other one,
            // dG[:, 0, :] W_hh, is a (B x 3H x H) product behind the sweep on the same stream: A = the t = 0 rows (row stride T * ld) of
            // [dr | dz] and of dn*r, added with beta = 1.  The sweep is unidirectional, so t0 = 0 for dense and ragged alike; a dead row's
            // gate gradients are 0, so nothing is gathered.
            const float* whh = weights[(size_t)l * 4 + 1];
            DepGemmOpts xo; xo.scratch = gws; xo.scratch_bytes = gwsb;
            rc = dep_gemm_internal(0, 0, B, H, 2 * H, dgi, T * ldg, whh, H, a.dhx, H, nullptr, 1.f, 0, 0, nullptr, 0, xo, s);
            if (rc) return rc;
            rc = dep_gemm_internal(0, 0, B, H, H, dghn, T * ldg, whh + (size_t)2 * H * H, H, a.dhx, H, nullptr, 1.f, 0, 0, nullptr, 0, xo, s);
            if (rc) return rc;
        }
        // data parallel: layer l's gradients are complete -- their range of the caller's flat gradient buffer goes to RCCL on the
        // communication stream.  Not right away: the collective is enqueued behind the NEXT layer's sweep (see `pending' above),
        // so that it travels over xGMI beside that layer's weight-gradient GEMMs and never beside a sweep.  The bottom layer's
        // range has nothing left to hide behind and goes out at once.
        if (gs && gs->comm && gs->range_ptr[l] && gs->range_count[l] > 0) {
            if (l > 0 && !dep_rnn_switches().comm_beside_sweeps && !fused) { pending_ptr = gs->range_ptr[l]; pending_n = gs->range_count[l]; }
            else {
                rc = dep_comm_enqueue_after((dep_comm*)gs->comm, gs->range_ptr[l], gs->range_count[l], s, (hipStream_t)gs->comm_stream);
                if (rc) return rc;
            }
        }
    }
    return DEP_OK;
}

extern "C" int dep_rnn_backward(const dep_rnn_desc* d, const float* x, const float* const* weights, const float* dy,
                                const float* dpooled, const float* dh_n, float* const* dweights, float* dx,
                                void* reserve, size_t reserve_bytes, void* workspace, size_t workspace_bytes,
                                void* stream) {
    return rnn_backward_impl(d, x, nullptr, weights, dy, dpooled, dh_n, nullptr, dweights, dx, reserve, reserve_bytes, workspace, workspace_bytes,
                             stream, nullptr);
}

extern "C" int dep_rnn_backward_state(const dep_rnn_desc* d, const float* x, const float* const* weights, const float* dy,
                                      const float* dpooled, const float* dh_n, const dep_rnn_state_grad* st, float* const* dweights, float* dx,
                                      void* reserve, size_t reserve_bytes, void* workspace, size_t workspace_bytes,
                                      void* stream, const dep_grad_sync* gs) {
    DEP_CHECK_ARG(!gs || (gs->comm && gs->comm_stream && gs->comm_stream != stream));      // (gs given: dep_rnn_backward_overlapped's rule)
    return rnn_backward_impl(d, x, nullptr, weights, dy, dpooled, dh_n, st, dweights, dx, reserve, reserve_bytes, workspace, workspace_bytes,
                             stream, gs);
}

extern "C" int dep_rnn_backward_varlen(const dep_rnn_desc* d, const float* x, const int32_t* lengths, const float* const* weights,
                                       const float* dy, const float* dpooled, const float* dh_n, float* const* dweights, float* dx,
                                       void* reserve, size_t reserve_bytes, void* workspace, size_t workspace_bytes, void* stream) {
    DEP_CHECK_ARG(lengths);
    return rnn_backward_impl(d, x, lengths, weights, dy, dpooled, dh_n, nullptr, dweights, dx, reserve, reserve_bytes, workspace, workspace_bytes,
                             stream, nullptr);
}

extern "C" int dep_rnn_backward_state_varlen(const dep_rnn_desc* d, const float* x, const int32_t* lengths, const float* const* weights,
                                             const float* dy, const float* dpooled, const float* dh_n, const dep_rnn_state_grad* st,
                                             float* const* dweights, float* dx, void* reserve, size_t reserve_bytes, void* workspace,
                                             size_t workspace_bytes, void* stream, const dep_grad_sync* gs) {
    if (!lengths) {
        dep_set_error("dep_rnn_backward_state_varlen: lengths is NULL; the dense call with a state is dep_rnn_backward_state");
        return DEP_ERR_ARG;
    }
    DEP_CHECK_ARG(!gs || (gs->comm && gs->comm_stream && gs->comm_stream != stream));      // (gs given: dep_rnn_backward_overlapped's rule)
    return rnn_backward_impl(d, x, lengths, weights, dy, dpooled, dh_n, st, dweights, dx, reserve, reserve_bytes, workspace, workspace_bytes,
                             stream, gs);
}

extern "C" int dep_rnn_backward_overlapped(const dep_rnn_desc* d, const float* x, const float* const* weights, const float* dy,
                                           const float* dpooled, const float* dh_n, float* const* dweights, float* dx,
                                           void* reserve, size_t reserve_bytes, void* workspace, size_t workspace_bytes,
                                           void* stream, const dep_grad_sync* gs) {
    DEP_CHECK_ARG(gs && gs->comm && gs->comm_stream && gs->comm_stream != stream);
    return rnn_backward_impl(d, x, nullptr, weights, dy, dpooled, dh_n, nullptr, dweights, dx, reserve, reserve_bytes, workspace, workspace_bytes,
                             stream, gs);
}

extern "C" int dep_rnn_backward_overlapped_varlen(const dep_rnn_desc* d, const float* x, const int32_t* lengths, const float* const* weights,
                                                  const float* dy, const float* dpooled, const float* dh_n, float* const* dweights,
                                                  float* dx, void* reserve, size_t reserve_bytes, void* workspace,
                                                  size_t workspace_bytes, void* stream, const dep_grad_sync* gs) {
    DEP_CHECK_ARG(lengths);
    DEP_CHECK_ARG(gs && gs->comm && gs->comm_stream && gs->comm_stream != stream);
    return rnn_backward_impl(d, x, lengths, weights, dy, dpooled, dh_n, nullptr, dweights, dx, reserve, reserve_bytes, workspace, workspace_bytes,
                             stream, gs);
}
