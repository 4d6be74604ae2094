// Host side shared by the co-resident ("cluster") sweep launchers (rnn_cluster16.hip, rnn_cluster_bwd.hip, rnn_cluster_lstm.hip,
// rnn_fused2.hip, rnn_fused2_bwd.hip): their switches, the batch-chunk geometry, the table row that names a launchable template
// instance, the exchange-header binder and the chunk loop.  Each kernel file keeps its instance table, its selection function and
// its payload size.
#pragma once
#include <mutex>
#include "rnn_cluster_common.h"

namespace depc {

// The switches of the cluster sweeps, read once per process (rnn_cluster.hip).
struct ClusterSwitches {
    int nofast;         // DEP_CLUSTER_NOFAST=1: always the write-through (placement-agnostic) stores
    bool trace;         // DEP_TRACE=1: workgroup 0 leaves clock stamps in the header slot's trace words
    int num_cus;        // DEP_NUM_CUS, else the device's CU count, else 256
    int force_soft;     // DEP_FORCE_SOFT_FALLBACK=1..3: the fused forward gives up on purpose (tests of the fallback path)
};
const ClusterSwitches& cluster_switches();

// How a batch is cut into launches that keep every member of every cluster resident: `members` workgroups per 16-utterance tile,
// at most `cap` workgroups (flag words) per launch.
struct ChunkGeometry {
    int B, members, cap;
    int CH;             // utterances per launch
    int nbtp_max;       // tiles of the largest chunk, padded to whole groups of 8
    int nbtp(int b0) const { const int cb = B - b0 < CH ? B - b0 : CH; return (dep_cdiv(cb, BT) + 7) / 8 * 8; }      // chunk starting at b0
    bool resident() const { return (size_t)nbtp_max * members <= (size_t)cap; }
};
inline ChunkGeometry chunk_geometry(int members, int per_cu, int cap, int B) {
    ChunkGeometry g{B, members, cap, dep_cluster_chunk(members, per_cu, cap), 0};
    g.nbtp_max = g.nbtp(0);
    return g;
}

// The GRU per-layer sweeps share one exchange buffer (dep_cluster_xbuf_bytes): 32-unit members, one per CU (rnn_cluster_bwd.hip), and
// the 16-unit-member forward, two per CU (rnn_cluster16.hip).
inline ChunkGeometry gru32_geometry(int H, int B) { return chunk_geometry(H / 32, 1, 256, B); }
inline ChunkGeometry gru16_geometry(int H, int B) { return chunk_geometry(H / 16, 2, 512, B); }
// The bidirectional forward (gru_fwd_cluster_r1<.., BI = true>, impl 6) runs both directions of a batch chunk in ONE launch: a direction
// doubles the clusters of a 16-utterance tile, 2 * H / 32 workgroups per tile, so the cap of 256 resident workgroups holds as it is and
// CH / nbtp count the tiles PER DIRECTION (padded to whole groups of 8, like every chunk).  Its payload is the forward's, per direction.
inline ChunkGeometry gru32_bi_geometry(int H, int B) { return chunk_geometry(2 * (H / 32), 1, 256, B); }
// forward: two parities of a tile's 16 x H block of h_t, whatever the member size; backward: two parities of every member's 16 x H partial dh
inline size_t gru_fwd_payload_bytes(const ChunkGeometry& g, int H) { return (size_t)2 * g.nbtp_max * BT * H * sizeof(float); }
inline size_t gru_fwd_bi_payload_bytes(const ChunkGeometry& g, int H) { return 2 * gru_fwd_payload_bytes(g, H); }      // g = gru32_bi_geometry
inline size_t gru_bwd_payload_bytes(const ChunkGeometry& g, int H) { return (size_t)2 * g.nbtp_max * g.members * BT * H * sizeof(float); }

// One launchable template instance: the kernel expression as text (what the launch-instance and order logs record), its address and
// the dynamic LDS it is launched with.  A family's table is the only place that names its instances.
template <class P> struct Instance {
    const char* text; void (*kernel)(P); size_t lds;
    std::once_flag lds_granted;
};
#define DEP_INSTANCE(kern, lds) { #kern, kern, lds }
constexpr size_t DEFAULT_DYNAMIC_LDS = 64 * 1024;      // what HIP grants a launch without hipFuncAttributeMaxDynamicSharedMemorySize

inline unsigned* hdr_words(void* xbuf, int slot, size_t off) { return (unsigned*)(hdr_base(xbuf, slot) + off); }
// status word, the slot's hello / trace words and the payload behind the headers -> the kernel's parameter struct.  Returns the
// slot's flag words, which the caller stores under the struct's own name for them (the fused backward has one pointer per layer).
template <class P> unsigned* bind_exchange(P& p, void* xbuf, int slot, size_t payload_bytes) {
    const ClusterSwitches& sw = cluster_switches();
    p.status = (unsigned*)xbuf; p.hello = hdr_words(xbuf, slot, HELLO_OFF);
    p.trace = sw.trace ? (long long*)hdr_words(xbuf, slot, TRACE_OFF) : nullptr;
    p.payload = (float*)((char*)xbuf + PAYLOAD_OFF); p.payload_bytes = (unsigned)payload_bytes; p.nofast = sw.nofast;
    return hdr_words(xbuf, slot, FLAG_OFF);
}

// One launch of `k` per batch chunk.  `prepare(b0)` runs in front of each launch and returns DEP_OK or an error: it leaves the
// flags / hello words of the launch's header slot(s) zero (hdr_prepare; never the status word, which is sticky over every sweep of
// a step and cleared by dep_rnn_forward) and sets what else of `p` depends on the chunk.
template <class P, class Prepare>
int launch_chunks(Instance<P>& k, const ChunkGeometry& g, dim3 block, P& p, hipStream_t s, const char* where, Prepare prepare) {
    if (k.lds > DEFAULT_DYNAMIC_LDS)
        std::call_once(k.lds_granted, [&k] { (void)hipFuncSetAttribute((const void*)k.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)k.lds); });
    for (int b0 = 0; b0 < g.B; b0 += g.CH) {
        p.b0 = b0; p.nbtp = g.nbtp(b0);
        if (const int rc = prepare(b0)) return rc;
        if (dep_ilog_on()) dep_ilog_note(k.text, where);
        hipLaunchKernelGGL(k.kernel, dim3(g.members * p.nbtp), block, k.lds, s, p);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) { dep_set_error("%s: launch of %s: HIP: %s", where, k.text, hipGetErrorString(e)); return DEP_ERR_HIP; }
    }
    return DEP_OK;
}

}  // namespace depc
