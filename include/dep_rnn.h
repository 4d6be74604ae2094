/*
 * dep_rnn.h -- C-ABI of libdep_rnn.so: the MI355X (gfx950) operator library that replaces the
 * PyTorch operator layer (torch.nn.GRU / LSTM / LayerNorm / Linear / Softmax / losses / Adam[W] +
 * autograd) under the reference's five training scripts.
 *
 * The reference (speechandlanguageprocessing/ICASSP2022-Depression) has no FFI layer of its own:
 * its boundary is the torch.nn operator contract used at the call sites cited on every entry
 * point below (paths relative to DepressionCollected/).  A maintainer binds these entry points
 * with ctypes; nothing torch-specific crosses the boundary.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to fp32 (or int32 where stated), row-major, caller-owned;
 *   - sequences are batch-first: row (b,t) of a (B,T,X) tensor sits at ((b*T + t) * ld);
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it, nothing synchronises;
 *   - return 0 on success, negative dep_status on error; dep_last_error() returns a message;
 *   - no allocation happens inside the library: workspace / reserve sizes come from the *_bytes
 *     queries and the caller provides the buffers (16-byte aligned);
 *   - gate order is PyTorch's: GRU r,z,n ; LSTM i,f,g,o ; h0 = c0 = 0 unless a *_state call says otherwise;
 *   - batches are dense (all B utterances T steps long) unless an entry point takes `lengths` (the *_varlen calls).
 *   - threads: entry points may be called concurrently from several host threads as long as each call has its own stream,
 *     workspace and reserve (dep_last_error is per thread; the launch-time recorder behind dep_profile_* and the
 *     reserve-mode record are mutex-guarded).  PROCESS-GLOBAL, not per stream: dep_set_gemm_mode (precision mode of every
 *     later call on any thread), dep_profile_enable, and the DEP_* environment switches, which are read once per process.
 */
#ifndef DEP_RNN_H
#define DEP_RNN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    DEP_OK = 0,
    DEP_ERR_ARG = -1,      /* bad argument (null pointer, size <= 0, unsupported combination) */
    DEP_ERR_WORKSPACE = -2, /* workspace / reserve too small */
    DEP_ERR_HIP = -3       /* a HIP call failed; see dep_last_error() */
} dep_status;

const char* dep_last_error(void);
/* library/ABI version and compiled arch string ("gfx950") */
int dep_version(void);
const char* dep_arch(void);

/* ------------------------------------------------------------------ descriptors ---- */
enum { DEP_POOL_NONE = 0, DEP_POOL_MEAN = 1, DEP_POOL_SUM = 2 };
enum { DEP_CELL_GRU = 0, DEP_CELL_LSTM = 1 };
/* Run modes (dep_rnn_desc.training):
 *   DEP_RUN_EVAL          no dropout; the reserve is scratch for the forward (output sequences, weight images).
 *   DEP_RUN_TRAIN         inter-layer dropout, and the reserve keeps everything dep_rnn_backward reads.
 *   DEP_RUN_DROPOUT_ONLY  inter-layer dropout drawn exactly as in DEP_RUN_TRAIN (same Philox key, sites and masks: y, pooled and
 *                         h_n are bit-identical to a DEP_RUN_TRAIN forward with the same seed), but no backward follows -- a frozen
 *                         encoder run under torch.no_grad() in train() mode (Classification/fuse_net_whole.py:336-366,
 *                         fusion_net.pretrained_feature).  The reserve keeps only what the forward itself reads: the packed
 *                         forward W_hh images, the direction-stacked W_ih / bias of a bidirectional stack, the copy of layer l
 *                         that feeds layer l+1 (dropout(y), or y when dropout_p = 0) and the top layer's output sequence -- except
 *                         for a GRU with pool != DEP_POOL_NONE, whose top sequence is not kept and is written only into the
 *                         caller's y, if one is given.  Not kept: saved gates / c, the backward W_hh images, the undropped outputs
 *                         of the lower layers; dep_rnn_reserve_y_offset / _ydrop_offset return (size_t)-1 for every array not
 *                         kept.  The workspace drops its backward-only parts (the 4H-wide gate-gradient room, the second set of
 *                         gate-gradient buffers, the dW_ih scratch of a bidirectional stack, the fused backward's exchange
 *                         room).  dep_rnn_backward / _overlapped refuse (DEP_ERR_ARG) a descriptor in this mode and a reserve
 *                         whose last forward ran in it.
 * Any other value is a bad descriptor (the size queries return 0, the entry points DEP_ERR_ARG). */
enum { DEP_RUN_EVAL = 0, DEP_RUN_TRAIN = 1, DEP_RUN_DROPOUT_ONLY = 2 };

/* One stacked recurrent network: torch.nn.GRU(F,H,num_layers=L,dropout=p,batch_first=True)
 * (Classification/audio_gru_whole.py:59-60) or torch.nn.LSTM(F,H,num_layers=L,dropout=p,
 * bidirectional=True) (Classification/text_bilstm_whole.py:54-56).
 * cell = DEP_CELL_GRU with dirs = 2 is torch.nn.GRU(F,H,num_layers=L,dropout=p,bidirectional=True,batch_first=True): the weight
 * order below (.._l0, .._l0_reverse, .._l1, ...; weight_ih of layer l > 0 is (3H, 2H)), y = [fwd | rev] columns, h_n ordered
 * [l0_fwd, l0_rev, l1_fwd, ...] with the reverse entry the state after step 0, pooled / dpooled (B,2H), inter-layer dropout drawn
 * over the element index of (b, t, col) in the (B,T,2H) array at site DEP_SITE_RNN0 + l like the BiLSTM's.  It runs the
 * tile-MFMA sweeps and nothing else (see impl). */
typedef struct {
    int32_t cell;        /* DEP_CELL_GRU | DEP_CELL_LSTM */
    int32_t B, T, F, H;  /* batch, steps, input features, hidden units */
    int32_t L;           /* stacked layers (>=1) */
    int32_t dirs;        /* 1 (unidirectional) or 2 (bidirectional: LSTM at any H; GRU where the tile-MFMA sweeps run, see impl) */
    int32_t training;    /* run mode: DEP_RUN_EVAL | DEP_RUN_TRAIN | DEP_RUN_DROPOUT_ONLY (see above) */
    float   dropout_p;   /* inter-layer dropout probability (applied to layers 0..L-2 outputs) */
    uint64_t seed;       /* Philox key for this call's dropout masks */
    int32_t pool;        /* GRU only: DEP_POOL_* over T of the top layer's y, (B,H*dirs) (fused in the sweep) */
    int32_t impl;        /* 0 auto (cluster > tile-MFMA > generic), 1 generic kernels, 2 one-workgroup-per-tile
                            MFMA kernels, 3 cluster-parallel MFMA kernels (GRU with H in {128,256}, BiLSTM with
                            H = 128; any B -- batches beyond one co-resident launch run as consecutive chunks),
                            4 the per-layer cluster sweeps: a unidirectional GRU (dirs = 1) with H in {64,128,256,512}, any B, T, L,
                            every run mode.  The cluster layout without the fused two-layer parts; every call on it, dense or
                            ragged, runs the plan a ragged call takes on a cluster descriptor -- one co-schedule-tolerant
                            32-unit-member sweep per layer (gru_fwd_cluster_r1 / gru_bwd_cluster_r1), never the fused two-layer or
                            16-unit-member launches -- and its forward is the cluster forward that takes hx (dep_rnn_forward_state
                            below).  dep_rnn_status and dep_rnn_workspace_xbuf_offset work as on impl 3.  Any other cell, dirs or
                            H with impl = 4 is a bad descriptor (size queries 0, entry points DEP_ERR_ARG, the rule in
                            dep_last_error).
                            5 the per-layer cluster sweeps, state through training: impl = 4 in every respect -- the same descriptors
                            exist, the same layout and sizes, the same plan, plain calls launch the same instances and give the same
                            bits, any other cell, dirs or H is a bad descriptor with the rule naming impl = 5 -- that also takes hx
                            in a DEP_RUN_TRAIN forward and hx / dhx in dep_rnn_backward_state[_varlen] (the state contract below).
                            6 the per-layer cluster forward of a bidirectional GRU: cell = DEP_CELL_GRU, dirs = 2, H in {64,128,256,512},
                            any B, T, L, every run mode.  Every forward on it, dense or ragged, runs one launch of the bidirectional
                            instance of gru_fwd_cluster_r1 per layer -- both directions of a batch chunk side by side, each
                            (direction, 16-utterance tile) pair a cluster of H / 32 co-resident workgroups with its W_hh in registers --
                            and takes hx in all three run modes (slices ordered like h_n, l * 2 + d).  The backward is the tile-MFMA
                            BiGRU backward of impl = 2, on the reserve that forward leaves (the same fp32 (B,T,2H) saved gates, the same
                            reserve offsets; hx / dhx as on impl = 2), so dep_rnn_backward[_state][_varlen] needs H <= 256: at H = 512
                            the descriptor has the forward only and a backward returns DEP_ERR_ARG.  The workspace has a cluster
                            exchange buffer (dep_rnn_status and dep_rnn_workspace_xbuf_offset work on it) and nothing else of the
                            cluster layouts.  Any other cell, dirs or H with impl = 6 is a bad descriptor (size queries 0, entry
                            points DEP_ERR_ARG, the rule in dep_last_error).  Outputs agree with impl = 2 to rounding (fast gate
                            nonlinearities, split or exact recurrent products as on impl = 4), the dropout masks bit for bit.
                            7 the per-layer cluster sweeps of a bidirectional GRU, forward and backward: impl = 6 in every forward -- the
                            same descriptors exist, the same launches, outputs and dropout masks bit for bit, the same reserve size and
                            offsets -- whose dep_rnn_backward[_state][_varlen] (and _overlapped) runs one launch per layer of the
                            bidirectional instance of gru_bwd_cluster_r1: both directions of a batch chunk side by side, each
                            (direction, 16-utterance tile) pair a cluster of H / 32 co-resident workgroups with its W_hh slice in
                            registers, at H in {64,128,256,512} -- H = 512 trains here -- any B, T, L, dense and ragged.  A
                            DEP_RUN_TRAIN forward packs the cluster backward's weight image of each direction where impl = 6 packs the
                            tile backward's, so a reserve goes with the impl that wrote it.  The sweep writes the fp32 gate-gradient
                            rows of the tile BiGRU backward ((B T, 6H) and (B T, 2H)), and everything behind it -- bias sums, the
                            direction-stacked dX and dW_ih, the per-direction dW_hh -- is the code impl 2 / 6 run; gradients agree with
                            impl = 6 to rounding.  Saved gates are fp32; there is no 16-bit or bf16 storage and no PK gate-gradient
                            image.  GEMM modes: 0 and 1 for every call; a dense backward also runs in mode 2 (the split-product sweep
                            instance, single-product contractions behind it); a backward in mode 3 is refused (its contractions read
                            the hi rows of a PK image this sweep does not write), and a ragged call in modes 2 / 3 as on every plan.
                            hx / dhx go through the backward at all four H; cx / c_n / dc_n / dcx are refused with the rule naming
                            impl = 7, as is any other cell, dirs or H.  The workspace is at least impl = 6's: its exchange buffer also
                            covers the backward's payload (dep_rnn_status and dep_rnn_workspace_xbuf_offset work as on impl = 6).
                            8 the exchange-free per-layer LSTM forward: an LSTM (cell = DEP_CELL_LSTM) with H = 128, dirs 1 or 2, any B,
                            T, F and L, in DEP_RUN_EVAL and DEP_RUN_DROPOUT_ONLY -- the run modes no backward follows.  Every forward,
                            dense or ragged, runs one projection GEMM and ONE launch of lstm_fwd_local per layer: a workgroup owns a
                            (direction, 16-utterance tile) and the whole W_hh of its direction, so nothing is exchanged between
                            workgroups -- the sweep needs no co-residency, runs the same beside other streams or processes
                            (dep_rnn_set_exclusive has no effect on it), covers any B in one launch and cannot give up: there is no
                            exchange buffer (dep_rnn_workspace_xbuf_offset is (size_t)-1) and dep_rnn_status is always DEP_OK.  It
                            takes hx, cx and c_n (dep_rnn_forward_state[_varlen] below).  The reserve offsets of y / dropout(y) are
                            those of impl = 3; outputs agree with impl = 3 to rounding, the dropout masks bit for bit.  GEMM mode 0
                            runs the exact-fp32 instance, modes 1 / 2 / 3 the three-term split instance (a ragged call in modes
                            2 / 3 is refused as on every plan).  DEP_RUN_TRAIN, any other cell or H, and every backward entry point
                            are refused (size queries 0, entry points DEP_ERR_ARG) with the rule naming impl = 8 in dep_last_error.
                            9 the exchange-free per-layer LSTM sweeps, forward and backward: the same LSTMs (H = 128, dirs 1 or 2, L 1 .. 8)
                            in all three run modes.  DEP_RUN_EVAL and DEP_RUN_DROPOUT_ONLY forwards are impl = 8's in every respect (the
                            same lstm_fwd_local launches, the same bits, all four GEMM modes).  A DEP_RUN_TRAIN forward launches the
                            saving instance lstm_fwd_save_local of the same sweep, which also stores the four activated gates as fp32
                            (B,T,dirs*4H) and c_t as (B,T,dirs*H) into the reserve, and packs the backward's W_hh image beside the
                            forward's; y, dropout(y), h_n and c_n are bit for bit those of a DEP_RUN_DROPOUT_ONLY forward.  Every
                            backward entry point runs ONE launch of lstm_bwd_local per layer -- again one workgroup per (direction,
                            16-utterance tile) with the whole W_hh^T of its direction in registers, nothing exchanged -- which writes
                            fp32 gate-gradient rows; the bias sums, the direction-stacked dX / dW_ih and the per-direction dW_hh behind
                            it are the code the tile sweeps run.  No exchange buffer (dep_rnn_workspace_xbuf_offset is (size_t)-1),
                            dep_rnn_status is always DEP_OK, dep_rnn_set_exclusive has no effect.  The reserve is laid out like any
                            DEP_RUN_TRAIN LSTM descriptor's with fp32 saved gates (y / dropout(y) offsets are impl = 3's) and goes with
                            the impl that wrote it.  The training forward and the backward run in GEMM modes 0 (exact fp32) and 1
                            (three-term split) only, dense and ragged; modes 2 / 3 are refused before any launch with the rule naming
                            impl = 9, and the mode must not change between a forward and its backward.  It takes every state member
                            (below).  Any other cell, H or L is a bad descriptor with the rule naming impl = 9.  Gradients agree with
                            impl = 3 to rounding; there are no 16-bit saved gates, no PK gate gradients and no paired dW_hh on it.
                            A bidirectional GRU otherwise has tile-MFMA kernels only: impl must be 0 or 2 (both mean those kernels)
                            and H a multiple of 16 they can tile -- H / 16 = waves x tiles per wave with waves in
                            {1,2,4,8} and at most 4 tiles per wave, inside the LDS bound: H in {16,32,48,64,96,128,192,256}.
                            Any other H, impl = 1 and impl = 3 are a bad descriptor (size queries 0, entry points
                            DEP_ERR_ARG with the rule in dep_last_error); on impl 0 / 2 it never takes the cluster, 16-unit-member
                            or fused two-layer kernels, and dep_rnn_workspace_xbuf_offset is (size_t)-1 for it. */
} dep_rnn_desc;

size_t dep_rnn_reserve_bytes(const dep_rnn_desc* d);     /* activations kept fwd -> bwd */
size_t dep_rnn_workspace_bytes(const dep_rnn_desc* d);   /* scratch, either direction */
/* Byte offset, inside the reserve, of layer `layer`'s output sequence (B,T,H*dirs) -- zero-copy
 * access to `output` for the caller (attention reads it in place); (size_t)-1 on bad arguments. */
size_t dep_rnn_reserve_y_offset(const dep_rnn_desc* d, int layer);
/* Same for the dropped-out copy that feeds layer+1 (DEP_RUN_TRAIN / DEP_RUN_DROPOUT_ONLY with dropout_p > 0 only). */
size_t dep_rnn_reserve_ydrop_offset(const dep_rnn_desc* d, int layer);

/* Health of the cluster-parallel sweeps that ran on `workspace` since the last dep_rnn_forward (desc.impl 0/3/4/5/6/7 with a
 * supported H): they exchange data between workgroups inside one launch with bounded spins; if a spin ever gives up
 * the kernels exit early and this returns DEP_ERR_HIP.  The status is STICKY over a step: dep_rnn_forward clears it once,
 * every later sweep (the other layers, the whole backward) leaves it alone and exits at entry when it is raised, so one
 * query after forward + backward sees a failure of any of the step's sweeps.  Synchronises `stream`.  Always DEP_OK for
 * the single-workgroup kernels. */
int dep_rnn_status(const dep_rnn_desc* d, void* workspace, void* stream);
/* Debug tooling: byte offset of the cluster exchange buffer inside the workspace ((size_t)-1 if unused).
 * With DEP_TRACE=1 workgroup 0 of the GRU sweeps leaves shader-clock stamps of its phases at +6400
 * (tools/trace_fwd.py, tools/trace_bwd.py). */
size_t dep_rnn_workspace_xbuf_offset(const dep_rnn_desc* d);
/* Kernels that need every CU to themselves.  The default GRU forward at H = 256 (both layers fused into one launch of twelve
 * 168-register waves per CU) cannot share the GPU: a foreign workgroup in the dispatcher keeps its clusters from assembling.
 * It then gives up within a few ms WITHOUT an error -- it sets the "soft" word (the uint32 after the status word, i.e. at
 * dep_rnn_workspace_xbuf_offset() + 4) and the per-layer kernels enqueued behind it, which tolerate co-scheduled work and are
 * no-ops otherwise, redo the forward: same reserve layout, results within the same 1e-4 of the reference, no host
 * synchronisation, every data-parallel rank decides for itself on the device.  A host that finds the soft word set at a
 * synchronisation point it has anyway should call dep_rnn_set_exclusive(0): later forwards then skip the attempt (and its
 * time-out) for the rest of the process.  PROCESS-GLOBAL; default 1, or 0 with DEP_EXCLUSIVE=0 in the environment. */
int dep_rnn_set_exclusive(int on);
int dep_rnn_get_exclusive(void);

/* ------------------------------------------------------------------ RNN stacks ----- */
/* weights: array of 4*L*dirs device pointers ordered, for layer l and direction d (index
 * (l*dirs+d)*4 + {0,1,2,3}): weight_ih (G*H, in), weight_hh (G*H, H), bias_ih (G*H), bias_hh (G*H),
 * in = F for l = 0 else H*dirs; G = 3 (GRU) or 4 (LSTM)  -- the tensors of
 * state_dict()['lstm_net_audio.weight_ih_l0'] ... / ['lstm_net.weight_ih_l0_reverse'] ...
 *
 * Precision: the recurrent products of the cluster sweeps follow the GEMM mode (dep_set_gemm_mode below): 3-term bf16
 * split by default, exact fp32 MFMA in mode 0.  The packed recurrent weights in the reserve are mode-specific, so the
 * mode must not change between a dep_rnn_forward and the dep_rnn_backward that consumes its reserve: the library records
 * the mode each reserve was produced in and dep_rnn_backward returns DEP_ERR_ARG on a mismatch.
 *
 * dep_rnn_forward replaces `x, _ = self.lstm_net_audio(x)` (audio_gru_whole.py:105) and
 * `output, (h_n, _) = self.lstm_net(x)` (text_bilstm_whole.py:105).
 *   x      (B,T,F)
 *   y      (B,T,H*dirs) top-layer output, may be NULL when only `pooled` is wanted
 *   pooled (B,H*dirs) mean/sum over T of the top layer's y (GRU, desc.pool != NONE; what x.mean(dim=1) / x.sum(dim=1) gives), else NULL
 *   h_n    (L*dirs, B, H) final hidden states ordered [l0_fwd, l0_bwd, l1_fwd, ...], may be NULL
 */
int dep_rnn_forward(const dep_rnn_desc* d, const float* x, const float* const* weights,
                    float* y, float* pooled, float* h_n,
                    void* reserve, size_t reserve_bytes, void* workspace, size_t workspace_bytes,
                    void* stream);

/* Backward of dep_rnn_forward (what loss.backward() does through nn.GRU/nn.LSTM,
 * audio_gru_whole.py:190).  Gradients are WRITTEN (not accumulated) to dweights (same order and
 * shapes as weights); dep_grad_accumulate adds them into an accumulator of the caller's.
 *   dy      (B,T,H*dirs) grad of y, or NULL
 *   dpooled (B,H*dirs) grad of pooled, or NULL  (the 1/T of a mean pool is applied inside)
 *   dh_n    (L*dirs,B,H) grad of h_n, or NULL
 *   dx      (B,T,F) grad of x, or NULL to skip it (the reference computes it but never uses it)
 */
int dep_rnn_backward(const dep_rnn_desc* d, const float* x, const float* const* weights,
                     const float* dy, const float* dpooled, const float* dh_n,
                     float* const* dweights, float* dx,
                     void* reserve, size_t reserve_bytes, void* workspace, size_t workspace_bytes,
                     void* stream);

/* ------------------------------------------------------------------ ragged batches -- */
/* Variable-length batches: x is a padded (B,T,F) batch and `lengths` a DEVICE pointer to B int32 values, caller-owned and read by the
 * kernels (no host copy, no synchronisation); row b is len_b = lengths[b] steps long, clamped on the device to [0, T].  The contract:
 *
 *   row b of every result equals what the dense entry point gives for that utterance alone, x[b:b+1, :len_b], at T' = len_b;
 *   positions t >= len_b of every output sequence (y, the layers' outputs in the reserve, alpha, dout) are exactly 0.0;
 *   weight gradients are the sum over rows of the per-row gradients; dx is exactly 0.0 at padded positions.
 *
 * i.e. pack_padded_sequence(enforce_sorted=False) -> nn.GRU / nn.LSTM -> pad_packed_sequence(total_length=T):
 *   - h_n is the state after step len_b - 1 (forward direction) / after step 0 (reverse direction, which STARTS at t = len_b - 1);
 *     dh_n enters there;
 *   - pooled (DEP_POOL_MEAN / _SUM) sums t < len_b and the mean divides by len_b; dpooled is scaled by 1 / len_b and reaches live steps only;
 *   - inter-layer dropout draws the masks of the dense call (the Philox element index of (b, t, col) is unchanged: a ragged call whose
 *     lengths all equal T draws the dense call's masks); padded positions are 0 before and after the mask;
 *   - len_b = 0: the row's y, pooled, h_n are 0, it contributes no gradient and divides by nothing.
 * The PADDED POSITIONS OF x MUST BE FINITE (zeros are customary): the weight-gradient contractions multiply them by exact zeros.  What
 * the reserve holds at dead positions besides the output sequences (saved gates) is unspecified.
 * All three run modes; GEMM modes 0 and 1 (modes 2 / 3 return DEP_ERR_ARG).  Reserve / workspace sizes and offsets are those of the
 * dense call.  A ragged call never runs a kernel without the length predicate: it takes the per-layer sweeps (tile, generic, cluster
 * GRU, cluster BiLSTM), not the fused two-layer GRU launches or the 16-unit-member forward.  A ragged bidirectional GRU takes the ragged
 * bidirectional instances of the tile-MFMA sweeps (its only kernels), under the same H / impl rule as its dense call.  A reserve written by a ragged forward is
 * consumed by a ragged backward with the SAME lengths; mixing a dense forward with a ragged backward (or the reverse) is the
 * caller's error and is not detected.  lengths == NULL is DEP_ERR_ARG here: the dense call is dep_rnn_forward / dep_rnn_backward. */
int dep_rnn_forward_varlen(const dep_rnn_desc* d, const float* x, const int32_t* lengths, const float* const* weights,
                           float* y, float* pooled, float* h_n,
                           void* reserve, size_t reserve_bytes, void* workspace, size_t workspace_bytes,
                           void* stream);
int dep_rnn_backward_varlen(const dep_rnn_desc* d, const float* x, const int32_t* lengths, const float* const* weights,
                            const float* dy, const float* dpooled, const float* dh_n,
                            float* const* dweights, float* dx,
                            void* reserve, size_t reserve_bytes, void* workspace, size_t workspace_bytes,
                            void* stream);

/* ------------------------------------------------------------------ data parallel -- */
/* RCCL over xGMI, one process per GPU (north_star; SURVEY 8b `dep_comm_{init,allreduce,destroy}`, 8e).  The reference has no
 * distributed code: these entry points are what a data-parallel `train()` binds -- the utterances of every global
 * mini-batch are split over the ranks, every rank normalises its loss gradient by the GLOBAL batch size, and the flat
 * fp32 gradient buffer is SUM all-reduced (the reference's `loss.backward(); optimizer.step()`,
 * Classification/audio_gru_whole.py:190-191, then sees the batch-mean gradient on every rank).
 * librccl is loaded at the first call (dlopen): single-GPU processes never touch it.
 *   dep_comm_available : 1 if librccl resolves in this process, else 0 (dep_last_error says why); not a collective -- the
 *                        host agrees on it across ranks before anyone enters dep_comm_init;
 *   dep_comm_unique_id : rank 0 obtains the 128-byte rendezvous id (ncclGetUniqueId) and hands it to the other ranks
 *                        through whatever side channel the host has (the Python layer broadcasts it with torch.distributed);
 *   dep_comm_init      : collective over all ranks (ncclCommInitRank), binds the communicator to HIP device `device`;
 *   dep_comm_allreduce : in-place SUM of n fp32 values, enqueued on `stream` (nothing synchronises);
 *   dep_comm_allreduce_ranges : several ranges as one grouped RCCL operation (one launch);
 *   dep_comm_destroy   : releases the communicator. */
typedef struct dep_comm dep_comm;
int dep_comm_available(void);
int dep_comm_unique_id(void* id_out, size_t bytes);                    /* bytes >= 128 */
int dep_comm_init(dep_comm** comm, int world, int rank, const void* unique_id, size_t id_bytes, int device);
int dep_comm_world(const dep_comm* comm);
int dep_comm_rank(const dep_comm* comm);
int dep_comm_allreduce(dep_comm* comm, float* buf, long n, void* stream);
int dep_comm_allreduce_ranges(dep_comm* comm, float* const* bufs, const long* counts, int nranges, void* stream);
int dep_comm_destroy(dep_comm* comm);

/* Gradient exchange overlapped with the backward pass ("overlapped with layer-0 backward").  range_ptr[l] /
 * range_count[l] name the contiguous span of the caller's flat gradient buffer that is FINAL once layer l's weight
 * gradients are written (the layer's own four tensors per direction plus whatever neighbours of the bucket were already
 * final, e.g. the head's gradients next to the top layer); count 0 skips a layer.  dep_rnn_backward_overlapped is
 * dep_rnn_backward plus: once layer l's dW are enqueued on `stream` AND the sweep of the layer below has been enqueued behind
 * them, `comm_stream` is made to wait for that point (event) and the SUM all-reduce of range l is enqueued there -- it runs
 * beside the weight-gradient GEMMs of the layer below (the bottom layer's range goes out at once).  The caller makes its
 * compute stream wait for `comm_stream` before the optimizer reads the gradients.
 * Co-scheduling: a cluster sweep needs all of its workgroups resident (one per CU, most of the CU's registers and LDS); a
 * collective kernel that holds CUs when a sweep is dispatched would stall it until the collective's peers let it finish.  So
 * collectives are ordered behind the sweeps and only ever run beside GEMMs (DEP_COMM_OVERLAP=sweep restores the earlier
 * enqueue point, beside the next backward sweep); the forward sweeps never have a collective beside them because the
 * optimizer step that precedes the next forward waits for the communication stream. */
typedef struct {
    dep_comm* comm;
    void* comm_stream;           /* hipStream_t, different from the compute stream */
    float* range_ptr[8];         /* indexed by layer */
    long range_count[8];
} dep_grad_sync;
int dep_rnn_backward_overlapped(const dep_rnn_desc* d, const float* x, const float* const* weights,
                                const float* dy, const float* dpooled, const float* dh_n,
                                float* const* dweights, float* dx,
                                void* reserve, size_t reserve_bytes, void* workspace, size_t workspace_bytes,
                                void* stream, const dep_grad_sync* gs);

/* dep_rnn_backward_overlapped for a ragged batch (dep_rnn_backward_varlen above; a rank passes its own shard of lengths). */
int dep_rnn_backward_overlapped_varlen(const dep_rnn_desc* d, const float* x, const int32_t* lengths, const float* const* weights,
                                       const float* dy, const float* dpooled, const float* dh_n,
                                       float* const* dweights, float* dx,
                                       void* reserve, size_t reserve_bytes, void* workspace, size_t workspace_bytes,
                                       void* stream, const dep_grad_sync* gs);

/* ------------------------------------------------------------------ recurrent state in and out -- */
/* The rest of torch.nn.GRU / torch.nn.LSTM's contract: `output, h_n = gru(x, hx)`, `output, (h_n, c_n) = lstm(x, (hx, cx))` and the
 * gradients that flow through them.  What it is for: scoring a long recording in chunks of bounded memory (carry h_n -> hx across the
 * cut), truncated BPTT (a detached state in, its dW_hh contribution kept), exact BPTT across a chunk boundary, learned initial states
 * and an encoder-to-decoder hand-over (dhx / dcx out, dh_n / dc_n in).
 *
 * Layout and NULL
 *   - every state array is (L*dirs, B, H), ordered like h_n: [l0_fwd, l0_rev, l1_fwd, ...];
 *   - any pointer may be NULL: for an input (hx, cx, dc_n) that means zeros, for an output (c_n, dhx, dcx) "not wanted";
 *   - cx, c_n, dc_n, dcx belong to the LSTM: with a GRU a non-NULL one is DEP_ERR_ARG.
 * Semantics
 *   - layer l, direction d starts its sweep from hx[l*dirs+d] (and cx[l*dirs+d]); the reverse direction starts at t = T-1 with its own slice;
 *   - h_n / c_n are the states after the sweep's last step (t = T-1 forward, t = 0 reverse);
 *   - dhx / dcx are the gradients with respect to hx / cx.  They are WRITTEN, not accumulated;
 *   - dc_n enters where dh_n enters;
 *   - the weight gradients include the state's term: dW_hh += dG[:, t0, :]^T hx with t0 = 0 (forward direction) / T-1 (reverse direction);
 *   - a backward must be given the hx / cx of the forward that wrote the reserve (hx feeds dW_hh and the GRU's dz at step t0, cx the
 *     LSTM's df at t0).  This is the caller's responsibility, as with `lengths`, and is not detected.
 * Plain calls
 *   - st == NULL, or a struct of NULLs, is dep_rnn_forward / dep_rnn_backward (dep_rnn_backward_overlapped when gs is given) on EVERY
 *     descriptor, cluster and fused ones included: the same launches, the same bits.
 * Where state is accepted
 *   - a non-NULL member is accepted exactly where the per-layer tile-MFMA / generic sweeps (rnn_sweep.hip) run the stack: a descriptor
 *     whose layout has no cluster exchange buffer, dep_rnn_workspace_xbuf_offset(d) == (size_t)-1.  In practice impl 1 or 2, or impl 0
 *     at a shape without cluster kernels (a bidirectional GRU on impl 0 / 2 is always such a descriptor);
 *   - on an impl = 6 descriptor (the per-layer cluster forward of a bidirectional GRU) hx is accepted by every forward, in all three run
 *     modes: each direction's clusters read that direction's slice, (l * 2 + d) like h_n.  hx / dhx in dep_rnn_backward_state go to the
 *     tile-MFMA backward, which takes them for a bidirectional GRU on impl = 2 already.  cx / c_n / dc_n / dcx are refused (a GRU);
 *   - on an impl = 7 descriptor (the per-layer cluster sweeps of a bidirectional GRU, forward and backward) the forward takes hx as
 *     on impl = 6, and dep_rnn_backward_state[_varlen] takes hx and dhx at H in {64,128,256,512}, dense and ragged, in every GEMM mode
 *     the backward runs in: the bidirectional gru_bwd_cluster_r1 takes a direction's hx slice as h_prev of that direction's last
 *     sweep step (t = 0; reverse direction t = T-1, or a ragged row's t = len_b - 1) and stores the direct term of dhx there; the call
 *     adds the hx term of dW_hh and, per direction, the recurrent term dG[:, t_last, :] W_hh (t_last = 0 / T-1) behind the sweep on
 *     `stream`.  A ragged row whose reverse sweep ends in dead steps has zero gate gradients at t_last and its stored dhx is already
 *     complete; a row of length 0 gets dhx = dh_n.  dhx may be dh_n's buffer; hx must be 16-byte aligned.  cx / c_n / dc_n / dcx are
 *     refused with the rule naming impl = 7;
 *   - hx alone is also accepted by dep_rnn_forward_state on an impl = 4 descriptor (the per-layer cluster sweeps) in DEP_RUN_EVAL and
 *     DEP_RUN_DROPOUT_ONLY, the run modes no backward follows: every member of a tile's cluster reads the tile's rows of hx in front
 *     of its first step.  Still refused there, before anything is launched: hx in DEP_RUN_TRAIN, and any non-NULL member in
 *     dep_rnn_backward_state -- on impl = 4 the cluster backward takes no state;
 *   - on an impl = 5 descriptor (the per-layer cluster sweeps, state through training) hx is accepted by the forward in every run
 *     mode, DEP_RUN_TRAIN included, and hx and dhx by dep_rnn_backward_state: gru_bwd_cluster_r1 takes hx as h_prev of step 0 and
 *     stores the direct term of dhx (d_0 * z_0) at its last step; the call adds the hx term of dW_hh and the recurrent term of dhx,
 *     dG[:, 0, :] W_hh, as small contractions behind the sweep on `stream`.  Such a call writes fp32 gate-gradient rows (never the
 *     pre-split PK image), so its contractions are the unpaired ones; a call without state keeps its plan and its bits.  dhx may be
 *     dh_n's buffer (the thread that stores a value read that address before the sweep); hx must be 16-byte aligned.  Refused there
 *     before anything is launched: cx / c_n / dc_n / dcx (a GRU), and a state-bearing backward in GEMM modes 2 / 3 (the bf16-storage
 *     and single-product instances take no hx);
 *   - on an impl = 8 descriptor (the exchange-free per-layer LSTM forward) hx, cx and c_n are accepted by dep_rnn_forward_state and
 *     dep_rnn_forward_state_varlen: a workgroup loads its tile's rows of the direction's hx / cx slice in front of its first step and
 *     stores h_n / c_n behind its last, so h_n may be hx's buffer and c_n cx's at every T; a ragged row of length 0 returns its state
 *     bit for bit.  It has no backward, so every dep_rnn_backward* call is refused with the rule naming impl = 8;
 *   - on an impl = 9 descriptor (the exchange-free per-layer LSTM sweeps, forward and backward) every member is accepted: hx, cx and c_n by
 *     every forward as on impl = 8, DEP_RUN_TRAIN included, and hx, cx, dc_n, dhx and dcx (beside dh_n) by dep_rnn_backward_state and
 *     dep_rnn_backward_state_varlen, in GEMM modes 0 and 1.  The backward sweep owns the whole W_hh, so dhx and dcx are simply what it
 *     carries past its last step, stored by the kernel (no host-side recurrent term); a lane reads its own slice of dh_n / dc_n before it
 *     stores, so dhx may be dh_n's buffer and dcx dc_n's.  c_prev of a row's first forward step is cx (direction 1 of a ragged row:
 *     at t = len_b - 1).  A ragged row of length 0 returns dhx = dh_n and dcx = dc_n bit for bit and contributes exact zeros to every
 *     gate gradient; dy at dead positions is ignored;
 *   - on any other descriptor (impl 0 / 3 with cluster kernels) the call returns DEP_ERR_ARG before anything is launched, with the rule
 *     in dep_last_error.
 * Scope
 *   - dense calls only (there is no `lengths` parameter: the ragged pair is dep_rnn_*_state_varlen below); all three run modes for the
 *     forward; the GEMM modes of the dense call;
 *   - h_n may be the same buffer as hx, and c_n the same as cx: every workgroup reads its rows of the state before the first step
 *     and writes them after the last (chunked streaming carries the state in place this way).  On impl = 4 a row of hx is read by all
 *     H / 32 members of its tile: for T >= 2 the hand-off orders every member's read in front of any member's h_n store (a member
 *     finishes only after all members of its tile raised their first flag); for T = 1 there is no hand-off, so when h_n overlaps hx the
 *     call first copies the layer's B x H slice of hx into a staging area of its workspace (one device-to-device copy on `stream`)
 *     and the sweep reads the copy (impl = 6 likewise, with the layer's 2 x B x H slice);
 *   - reserve and workspace sizes and every offset are those of dep_rnn_forward / dep_rnn_backward;
 *   - gs: NULL, or as for dep_rnn_backward_overlapped. */
typedef struct { const float* hx; const float* cx; float* c_n; } dep_rnn_state;
typedef struct { const float* hx; const float* cx; const float* dc_n; float* dhx; float* dcx; } dep_rnn_state_grad;
int dep_rnn_forward_state(const dep_rnn_desc* d, const float* x, const float* const* weights,
                          float* y, float* pooled, float* h_n, const dep_rnn_state* st,
                          void* reserve, size_t reserve_bytes, void* workspace, size_t workspace_bytes,
                          void* stream);
int dep_rnn_backward_state(const dep_rnn_desc* d, const float* x, const float* const* weights,
                           const float* dy, const float* dpooled, const float* dh_n, const dep_rnn_state_grad* st,
                           float* const* dweights, float* dx,
                           void* reserve, size_t reserve_bytes, void* workspace, size_t workspace_bytes,
                           void* stream, const dep_grad_sync* gs);

/* Recurrent state together with `lengths`: `gru(pack_padded_sequence(x, lengths, enforce_sorted=False), hx)` as one call.  What it is
 * for: scoring a padded batch of recordings of different lengths chunk by chunk, and truncated or exact BPTT across a chunk boundary of
 * a padded batch.  `lengths` is the device array of the *_varlen calls (B int32 values, clamped on the device to [0, T]); the state
 * structs, their layout and their NULL rules are those of dep_rnn_forward_state / dep_rnn_backward_state above.
 * Row equivalence
 *   - row b of every result equals what dep_rnn_forward_state / dep_rnn_backward_state give for that row alone: x[b:b+1, :len_b],
 *     hx[:, b:b+1], cx[:, b:b+1] (and dh_n[:, b:b+1], dc_n[:, b:b+1]) at T' = len_b.
 * Padding
 *   - padded positions (t >= len_b) of every output sequence and of dx are exactly 0.0; pooled follows the varlen rule (sum over
 *     t < len_b, the mean divides by len_b); dropout draws the dense call's masks (unchanged element index).  The padded positions of x
 *     must be finite, as for every ragged call.
 * Directions
 *   - the forward direction starts from its slice of hx / cx at t = 0; the reverse direction starts from its own slice at t = len_b - 1.
 * Final states
 *   - h_n / c_n are the states after the row's last live sweep step (t = len_b - 1 forward, t = 0 reverse); dh_n / dc_n enter there.
 * len_b = 0: the state passes through
 *   - h_n[:, b] = hx[:, b] and c_n[:, b] = cx[:, b], bit for bit; dhx[:, b] = dh_n[:, b] and dcx[:, b] = dc_n[:, b], bit for bit (zeros
 *     for a NULL input); y, pooled and dx of the row are 0 and it contributes to no weight gradient.  This is the rule under which
 *     chunks compose: a recording that has ended pushes length 0 from then on and its state and state gradient travel through
 *     unchanged.  With a NULL hx it is the "h_n is 0" rule of the varlen contract.
 * Weight gradients
 *   - they include the state's term per row: dW_hh += sum_b dG[b, t0_b, :]^T hx[b] with t0_b = 0 (forward direction) / len_b - 1
 *     (reverse direction), over the rows with len_b > 0 only.  Exact fp32, summed in the order b = 0 .. B-1, no atomics.
 * Aliasing and responsibility
 *   - h_n may be the same buffer as hx and c_n the same as cx, as in the dense state call;
 *   - the backward must be given the forward's hx / cx AND lengths.  This is the caller's responsibility and is not detected.
 * Where it is accepted
 *   - exactly where the dense state call is accepted: a descriptor whose layout has no cluster exchange buffer
 *     (dep_rnn_workspace_xbuf_offset(d) == (size_t)-1), and hx in the forward on an impl = 4 descriptor in DEP_RUN_EVAL /
 *     DEP_RUN_DROPOUT_ONLY (the ragged instances of the same sweep: a row with len_b = 0 returns hx bit for bit; the T = 1 aliasing
 *     rule is the dense call's), and hx in every forward and hx / dhx in the backward on an impl = 5 descriptor (a row with len_b = 0
 *     never was live: its dhx is the dh_n it was given, bit for bit); elsewhere a non-NULL member is DEP_ERR_ARG before anything is
 *     launched, with the rule in dep_last_error;
 *   - also refused before any launch: cx / c_n / dc_n / dcx on a GRU, lengths == NULL (the dense call is dep_rnn_*_state), and GEMM
 *     modes 2 / 3 (as for every ragged call).
 * All-NULL state
 *   - st == NULL, or a struct of NULLs, is dep_rnn_forward_varlen / dep_rnn_backward_varlen (dep_rnn_backward_overlapped_varlen when gs
 *     is given) on every descriptor: the same launches, the same bits.
 * Unchanged surroundings
 *   - all three run modes for the forward; gs: NULL, or as for dep_rnn_backward_overlapped; reserve and workspace sizes and every offset
 *     are those of dep_rnn_forward / dep_rnn_backward; the kernel instances launched are those of the plain ragged call. */
int dep_rnn_forward_state_varlen(const dep_rnn_desc* d, const float* x, const int32_t* lengths, const float* const* weights,
                                 float* y, float* pooled, float* h_n, const dep_rnn_state* st,
                                 void* reserve, size_t reserve_bytes, void* workspace, size_t workspace_bytes,
                                 void* stream);
int dep_rnn_backward_state_varlen(const dep_rnn_desc* d, const float* x, const int32_t* lengths, const float* const* weights,
                                  const float* dy, const float* dpooled, const float* dh_n, const dep_rnn_state_grad* st,
                                  float* const* dweights, float* dx,
                                  void* reserve, size_t reserve_bytes, void* workspace, size_t workspace_bytes,
                                  void* stream, const dep_grad_sync* gs);

/* ------------------------------------------------------------------ dense --------- */
/* C[M,N] = opA(A)[M,K] * opB(B)[K,N] + bias[N] + beta*C      (fp32 MFMA, exact f32 products)
 *   transA = 0: A is (M,K) row-major ; 1: A is stored (K,M)
 *   transB = 0: B is stored (K,N)    ; 1: B is stored (N,K)   [nn.Linear weight layout]
 * Replaces nn.Linear forward/backward (audio_gru_whole.py:67,70) and the time-parallel
 * input-projection / weight-gradient contractions inside nn.GRU / nn.LSTM.
 * seq_T/shiftB: when seq_T > 0 and transB == 0, row r of B is read from row r+shiftB and is taken
 * as zero when (r % seq_T)+shiftB falls outside [0,seq_T)  (h_{t-1} operand of dW_hh).
 * workspace is needed for split-K (dep_gemm_workspace_bytes), may be NULL otherwise.  A call that does not split may
 * still use a workspace it is given as scratch: calls that may run concurrently need one workspace each (one per stream). */
size_t dep_gemm_workspace_bytes(int transA, int transB, int M, int N, int K);
int dep_gemm_f32(int transA, int transB, int M, int N, int K,
                 const float* A, int lda, const float* B, int ldb, float* C, int ldc,
                 const float* bias, float beta, int seq_T, int shiftB,
                 void* workspace, size_t workspace_bytes, void* stream);

/* Same contract with split-precision products: every fp32 operand element is split on the fly into
 * bf16 hi + bf16 lo and a*b is formed as a_hi*b_hi + a_hi*b_lo + a_lo*b_hi on the bf16 matrix cores with
 * fp32 accumulation (relative error per product ~1e-5, inside the path's 1e-4 parity budget; 5x the MFMA
 * rate of the exact kernel).  dep_rnn_forward/backward use it for their time-parallel contractions of at
 * least `min_macs` multiply-adds when the mode is 1 (default; DEP_GEMM_MODE=f32 or dep_set_gemm_mode(0,-1)
 * selects the exact fp32 kernel everywhere).  dep_gemm_f32 itself is always exact. */
int dep_gemm_bf16x3(int transA, int transB, int M, int N, int K,
                    const float* A, int lda, const float* B, int ldb, float* C, int ldc,
                    const float* bias, float beta, int seq_T, int shiftB,
                    void* workspace, size_t workspace_bytes, void* stream);
/* Same contract, precision chosen exactly as dep_rnn_forward / dep_rnn_backward choose it for a contraction of this size under
 * the current dep_set_gemm_mode (0: exact, 1: three-term split above min_macs, 2: single bf16 products).  dep_gemm_bf16x3 above
 * never follows the mode: where the split kernel runs it forms all three terms.
 * A SMALL problem runs one exact fp32 kernel (gemm_small: 32x32 output tiles, exact f32 products) under EVERY entry and EVERY mode,
 * dep_gemm_bf16x3 and mode 2 included -- the plan tests this first, before it looks at the precision:
 *     seq_T <= 0  and  ceil(M/128) * ceil(N/128) < 32  and  K <= 8192  and  M*N*K <= 2^27.
 * Such a call splits no K and needs no workspace.  Every other shape takes the kernel of its entry / mode: exact fp32 MFMA tiles, or the
 * split-precision kernel (tests/test_gemm_forms_gpu.py pins the routing of each form through the launch-instance log). */
int dep_gemm(int transA, int transB, int M, int N, int K,
             const float* A, int lda, const float* B, int ldb, float* C, int ldc,
             const float* bias, float beta, int seq_T, int shiftB,
             void* workspace, size_t workspace_bytes, void* stream);
/* Experiment hook (tools/exp_overlap2.py): confine the working workgroups of the calling thread's next
 * split-precision GEMMs to XCDs [lo, lo + n) -- block index % 8 is the XCD.  (0, 8) = whole chip, the default. */
int dep_gemm_set_xcds(int lo, int n);
/* mode 2 (DEP_GEMM_MODE=bf16) is the THROUGHPUT mode BASELINE configs[1] calls "bf16": the large contractions form a_hi * b_hi only
 * (plain bf16 products, fp32 accumulation; a third of the MFMAs).  Relative error per product ~4e-3: it cannot meet the path's
 * 1e-4 parity bar, is never the default and is benchmarked on its own labelled line (bench.py extra.bf16_products).
 * mode 3 (DEP_GEMM_MODE=bf16s) adds bf16 STORAGE to mode 2 for the stack whose kernels have the variants (2-layer GRU, H = 256, T even,
 * the exclusive fused forward): the hidden sequences y / dropout(y), hn and the gate gradients live in the reserve / workspace as bf16
 * (2-byte elements at the positions of the fp32 arrays; the gate gradients as the hi rows of the PK image), the saved gates as 16-bit
 * fixed point; state, accumulation and the recurrence stay fp32.  dep_rnn_forward then takes y == NULL only and
 * dep_rnn_reserve_y_offset points at bf16 data.  Other stacks run mode 3 exactly like mode 2.  Gradients within ~1e-2 of their scale
 * (tests/test_presplit_gpu.py); bench.py extra.bf16_storage. */
int dep_set_gemm_mode(int mode, long min_macs);   /* PROCESS-GLOBAL. mode 0 exact f32 | 1 bf16x3 split | 2 bf16 products | 3 bf16 products + storage ; min_macs < 0 keeps it */
int dep_get_gemm_mode(void);

/* nn.LayerNorm(F) over the last axis (audio_gru_whole.py:62,104). rows = B*T.
 * mean_rstd: (rows,2) saved statistics (may be NULL in inference). */
int dep_layernorm_fwd(const float* x, const float* gamma, const float* beta, float* y,
                      float* mean_rstd, int rows, int F, float eps, void* stream);
/* gamma == beta == NULL: plain x-hat (no affine), used with the fold below.
 *
 * LayerNorm feeding a linear map (ln -> gru.weight_ih_l0, audio_gru_whole.py:104-105) with the affine folded into the map:
 *     (xhat*gamma + beta) W^T + b  ==  xhat (W*gamma)^T + (b + W beta)
 * dep_ln_fold_fwd builds Wf (J,F) = W*gamma and bf (J) = b + W beta; the recurrent stack then runs on x-hat with
 * (Wf, bf) in place of (W, b) and its backward returns dWf, dbf; dep_ln_fold_bwd turns those into
 *     dW = dWf*gamma + dbf beta^T, db = dbf, dgamma[f] = sum_j dWf[j,f] W[j,f], dbeta[f] = sum_j W[j,f] dbf[j]
 * -- the gradients nn.LayerNorm + nn.GRU would produce, without ever forming dL/d(xn) (B*T x F) or walking it. */
int dep_ln_fold_fwd(const float* W, const float* b, const float* gamma, const float* beta,
                    float* Wf, float* bf, int J, int F, void* stream);
int dep_ln_fold_bwd(const float* W, const float* dWf, const float* dbf, const float* gamma, const float* beta,
                    float* dW, float* db, float* dgamma, float* dbeta, int J, int F, void* stream);
/* The fold for npieces in {1, 2} maps W_k (J,F), b_k (J) that consume the SAME LayerNorm (weight_ih_l0 and weight_ih_l0_reverse of
 * a bidirectional stack).  W, b, Wf, bf, dWf, dbf, dW, db are HOST arrays of npieces device pointers (read during the call, as
 * dep_grad_sqnorm reads its ranges); gamma, beta, dgamma, dbeta are device vectors (F).  One launch each.
 *   forward : Wf_k = W_k*gamma, bf_k = b_k + W_k beta
 *   backward: dW_k = dWf_k*gamma + dbf_k beta^T, db_k = dbf_k, and -- WRITTEN, not added --
 *             dgamma[f] = sum_k sum_j dWf_k[j,f] W_k[j,f], dbeta[f] = sum_k sum_j W_k[j,f] dbf_k[j]
 *             in a fixed order: piece 0's sum, then piece 1's, added once; no atomics, the same bits on every run.
 * npieces == 1 gives the bits of dep_ln_fold_fwd / dep_ln_fold_bwd.  Arguments are checked before any HIP call. */
int dep_ln_fold_fwd_multi(const float* const* W, const float* const* b, const float* gamma, const float* beta,
                          float* const* Wf, float* const* bf, int npieces, int J, int F, void* stream);
int dep_ln_fold_bwd_multi(const float* const* W, const float* const* dWf, const float* const* dbf, const float* gamma,
                          const float* beta, float* const* dW, float* const* db, float* dgamma, float* dbeta,
                          int npieces, int J, int F, void* stream);
/* dgamma/dbeta are written; dx may be NULL (the reference never consumes it).
 * workspace: dep_layernorm_bwd_workspace_bytes. */
size_t dep_layernorm_bwd_workspace_bytes(int rows, int F);
int dep_layernorm_bwd(const float* dy, const float* x, const float* gamma, const float* mean_rstd,
                      float* dx, float* dgamma, float* dbeta, int rows, int F,
                      void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ attention ------ */
/* attention_net_with_w (text_bilstm_whole.py:74-99).
 *   out (B,T,2H), h_n (K,B,H), Wa (H,H), ba (H)  ->  ctx (B,H)
 *   saved: alpha (B,T), pre (B,H) = Wa*sum_k(h_n)+ba, hsum (B,H)     [needed by the backward] */
int dep_attn_fwd(const float* out, const float* h_n, int K, const float* Wa, const float* ba,
                 float* ctx, float* alpha, float* pre, float* hsum, int B, int T, int H,
                 void* stream);
/*   dctx (B,H) -> dout (B,T,2H) written, dh_n (K,B,H) written, dWa (H,H), dba (H) written.
 *   workspace: dep_attn_bwd_workspace_bytes. */
size_t dep_attn_bwd_workspace_bytes(int B, int T, int H);
int dep_attn_bwd(const float* dctx, const float* out, const float* Wa, const float* alpha,
                 const float* pre, const float* hsum, int K,
                 float* dout, float* dh_n, float* dWa, float* dba, int B, int T, int H,
                 void* workspace, size_t workspace_bytes, void* stream);

/* Ragged batches (see dep_rnn_forward_varlen): `lengths` is a device pointer to B int32 values.  The softmax runs over t < len_b only,
 * alpha[b, t >= len_b] and dout[b, t >= len_b] are exactly 0; a row with len_b = 0 gives ctx = 0 and zero gradients.  `out` is never
 * read at padded positions. */
int dep_attn_fwd_varlen(const float* out, const int32_t* lengths, const float* h_n, int K, const float* Wa, const float* ba,
                        float* ctx, float* alpha, float* pre, float* hsum, int B, int T, int H,
                        void* stream);
int dep_attn_bwd_varlen(const float* dctx, const float* out, const int32_t* lengths, const float* Wa, const float* alpha,
                        const float* pre, const float* hsum, int K,
                        float* dout, float* dh_n, float* dWa, float* dba, int B, int T, int H,
                        void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ heads / losses - */
/* Dropout as nn.Dropout(p) in training mode: y = x * m / (1-p), m ~ Bernoulli(1-p) from
 * Philox4x32-10(seed, site, element index).  The same call on a gradient applies the same mask.
 * p == 0 copies.  x may alias y.  */
int dep_dropout(const float* x, float* y, long n, float p, uint64_t seed, uint32_t site, void* stream);
/* The pre-scaled mask itself (0 or 1/(1-p)), for tests that feed the oracle the same masks. */
int dep_dropout_mask(float* mask, long n, float p, uint64_t seed, uint32_t site, void* stream);
/* a = relu(z) then dropout (nn.ReLU + nn.Dropout, audio_gru_whole.py:68-69); z and a may alias. */
int dep_relu_dropout_fwd(const float* z, float* a, long n, float p, uint64_t seed, uint32_t site, void* stream);
/* dz = da * mask * (z > 0) */
int dep_relu_dropout_bwd(const float* da, const float* z, float* dz, long n, float p, uint64_t seed,
                         uint32_t site, void* stream);
/* column sums of a (M,N) matrix (bias gradients): out[n] = sum_m x[m*ld+n] */
int dep_colsum(const float* x, int M, int N, int ld, float* out, void* stream);

enum { DEP_LOSS_CE_ON_SOFTMAX = 0, DEP_LOSS_L1_RELU = 1, DEP_LOSS_SMOOTHL1_RELU = 2, DEP_LOSS_CE_LOGITS = 3,
       DEP_LOSS_SMOOTHL1 = 4,
       DEP_LOSS_LABELS_I64 = 0x100 /* OR into a CE kind: target holds int64 labels (torch.long, as the reference's loops make
                                      them: audio_gru_whole.py:178) instead of int32 -- no cast kernel per mini-batch */ };
/* Output nonlinearity + loss + its gradient w.r.t. the pre-activation z (B,C), one kernel:
 *   CE_ON_SOFTMAX : out = softmax(z) ; loss = CrossEntropyLoss(out, y)  (double softmax,
 *                   audio_gru_whole.py:72,188,308)              target = int32 labels (int64 with DEP_LOSS_LABELS_I64)
 *   L1_RELU       : out = relu(z) ; L1Loss(out, y)   (audio_bilstm_perm.py:91,251)  target = float
 *   SMOOTHL1_RELU : out = relu(z) ; SmoothL1Loss(out, y) (text_bilstm_perm.py:247)   target = float
 *   CE_LOGITS / SMOOTHL1 : plain losses on z (MyLoss halves, fuse_net_whole.py:384-395)
 * out (B,C) written; loss_rows (B) per-row loss; dz (B,C) = dLoss/dz with Loss = sum_rows / norm
 * (norm = global batch size so that data-parallel shards sum to the reference's batch mean);
 * dz may be NULL (evaluate); target may be NULL when dz and loss_rows are NULL (pure forward). */
int dep_head_loss(int kind, const float* z, const void* target, float* out, float* loss_rows,
                  float* dz, int B, int C, float norm, void* stream);
/* loss = sum(loss_rows[0..B)) / norm, deterministic single-block tree; result on device. */
int dep_reduce_loss(const float* loss_rows, int B, float norm, float* loss_out, int accumulate, void* stream);
/* dep_head_loss for the two CE kinds (with or without DEP_LOSS_LABELS_I64) with torch.nn.CrossEntropyLoss's options, reduction
 * 'mean'.  a = z (CE_LOGITS) or softmax(z) (CE_ON_SOFTMAX), lq = log_softmax(a), q = exp(lq), w = class_weight (C floats on the
 * device; NULL = ones), W = sum_c w_c, eps = label_smoothing; a row is live when its label != ignore_index:
 *     loss_rows[i] = live_i [ (1-eps) w[y_i] (-lq[i,y_i]) + (eps/C) sum_c w_c (-lq[i,c]) ]
 *     dL/da        = live_i [ (1-eps) w[y_i] (q - onehot(y_i)) + (eps/C) (q W - w) ] / den ,   dz = dL/da through the first softmax
 * den is `norm`, or *norm_dev when norm_dev != NULL (a device float, e.g. dep_ce_weight_sum's: no host read).  For torch's mean it
 * is sum_i live_i w[y_i] over the WHOLE global / accumulated batch, so that shards and micro-batches sum to the big batch's
 * gradient.  An ignored row still writes `out`; its loss_rows entry and its dz row are exactly 0.  den == 0 (no live row) gives
 * NaN, as in torch.  One thread per row, the per-class values in registers; one launch.
 * With class_weight == NULL, label_smoothing == 0 and no row ignored, out / loss_rows / dz are bit-identical to dep_head_loss.
 * DEP_ERR_ARG, before anything is launched: any other kind, C > 16, label_smoothing outside [0, 1), z == NULL, norm <= 0 with
 * norm_dev == NULL.  A label outside [0, C) that is not ignore_index is the caller's error (it gives NaN, never a stray access). */
int dep_head_loss_ce(int kind, const float* z, const void* target, const float* class_weight, float label_smoothing,
                     long long ignore_index, float* out, float* loss_rows, float* dz, int B, int C, float norm,
                     const float* norm_dev, void* stream);
/* den_out[0] = sum_i [target_i != ignore_index] w[target_i] over B labels (int32, or int64 when labels_i64): the denominator
 * dep_head_loss_ce / dep_reduce_loss_by take through their device pointer.  Deterministic single-block tree; C <= 16. */
int dep_ce_weight_sum(const void* target, int labels_i64, const float* class_weight, long long ignore_index, int B, int C,
                      float* den_out, void* stream);
/* dep_reduce_loss with the divisor read from a device float: loss = sum(loss_rows[0..B)) / norm_dev[0]. */
int dep_reduce_loss_by(const float* loss_rows, int B, const float* norm_dev, float* loss_out, int accumulate, void* stream);

enum { DEP_REG_L1 = 0, DEP_REG_SMOOTHL1 = 1, DEP_REG_HUBER = 2, DEP_REG_MSE = 3 };
/* The regression criteria with torch's parameters and per-row sample weights, reduction 'mean': one launch, one thread per row.
 * o = relu ? max(z, 0) : z, d = o - target, a = |d|, per element (torch's CPU formulas, the knees included):
 *     L1                        l = a                                             dl/do = sgn(d)   (0 at d == 0)
 *     SMOOTHL1, param = beta    l = a < beta  ? 0.5 d^2 / beta : a - 0.5 beta     dl/do = a < beta  ? d / beta : sgn(d)
 *     HUBER,    param = delta   l = a < delta ? 0.5 d^2 : delta (a - 0.5 delta)   dl/do = a < delta ? d : delta sgn(d)
 *     MSE                       l = d^2                                           dl/do = 2 d
 * beta == 0 is L1, as in torch.  With w_i = row_weight[i] (B floats on the device; NULL = ones):
 *     loss_rows[i] = w_i sum_c l[i,c]
 *     dz[i,c]      = w_i dl/do (relu && !(z > 0) ? 0 : 1) / den
 * den is `norm`, or *norm_dev when norm_dev != NULL (a device float, e.g. dep_row_weight_sum's: no host read).  For the weighted
 * mean over elements it is C sum_i w_i over the WHOLE global / accumulated batch.  A row whose weight is exactly 0 is an ignored
 * row, the counterpart of ignore_index: its loss_rows entry and its dz row are exactly 0.0 -- selected, not multiplied, whatever
 * its target holds (NaN included) -- and its `out` row is still written.  den == 0 on the device gives NaN, as in dep_head_loss_ce.
 * `out` is written whenever it is given; target may be NULL when dz and loss_rows are NULL (pure forward).
 * With row_weight == NULL and norm_dev == NULL, L1 and SMOOTHL1 with param == 1 write the bits dep_head_loss writes for
 * DEP_LOSS_L1_RELU / DEP_LOSS_SMOOTHL1_RELU (relu = 1) and DEP_LOSS_SMOOTHL1 (relu = 0).
 * DEP_ERR_ARG, before anything is launched: an unknown form, relu not 0 or 1, param NaN or negative, param == 0 for HUBER,
 * z == NULL, B <= 0, C <= 0 or C > 16, norm <= 0 or NaN with norm_dev == NULL, target == NULL with loss_rows or dz given. */
int dep_head_loss_reg(int form, int relu, float param, const float* z, const float* target, const float* row_weight,
                      float* out, float* loss_rows, float* dz, int B, int C, float norm, const float* norm_dev, void* stream);
/* den_out[0] = scale * sum_i row_weight[i] over B floats (scale > 0; C for the mean over elements): the denominator
 * dep_head_loss_reg / dep_reduce_loss_by take through their device pointer.  Deterministic single-block tree, the scale applied
 * once after it. */
int dep_row_weight_sum(const float* row_weight, int B, float scale, float* den_out, void* stream);

/* The models' MLP head as three launches (one forward, two backward) instead of fifteen:
 *     [Dropout(p)] -> Linear(Hin,H1) -> ReLU -> Dropout(p) -> [Linear(H1,C)]
 * (fc_audio: Classification/audio_gru_whole.py:66-73, Regression/audio_bilstm_perm.py:60-67 -- first_dropout = 1;
 *  fc_out: Classification/text_bilstm_whole.py:60-66 -- first_dropout = 0).  Exact fp32, fixed summation order; the masks are the
 * draws dep_dropout / dep_relu_dropout_* make at (seed, site0) / (seed, site1).  W1 (H1,Hin), W2 (C,H1) row-major as
 * torch.nn.Linear holds them; W1 16-byte aligned.  dep_head_mlp_supported says which widths are covered (Hin and H1 powers of
 * two in [8, 256], C <= 16); other shapes are composed from dep_gemm_f32 / dep_relu_dropout_* / dep_colsum.
 *   fwd : a0 (B,Hin) = dropout(x) (written only if first_dropout && p > 0; otherwise x itself is the saved input),
 *         z1, a1 (B,H1) saved for the backward, z2 (B,C) the pre-activation dep_head_loss takes (C = 0: stop at a1).
 *   bwd : dz2 (B,C) from dep_head_loss; a0 = what the forward saved (x when no first dropout ran); dW1, db1, dW2, db2
 *         OVERWRITTEN; dx (B,Hin) or NULL; dz1 (B,H1) scratch. */
int dep_head_mlp_supported(int Hin, int H1, int C);
int dep_head_mlp_fwd(const float* x, const float* W1, const float* b1, const float* W2, const float* b2, float* a0,
                     float* z1, float* a1, float* z2, int B, int Hin, int H1, int C, float p, uint64_t seed,
                     uint32_t site0, uint32_t site1, int first_dropout, void* stream);
int dep_head_mlp_bwd(const float* dz2, const float* a0, const float* z1, const float* a1, const float* W1,
                     const float* W2, float* dW1, float* db1, float* dW2, float* db2, float* dx, float* dz1, int B,
                     int Hin, int H1, int C, float p, uint64_t seed, uint32_t site0, uint32_t site1, int first_dropout,
                     void* stream);

/* ------------------------------------------------------------------ optimizer ------ */
/* torch.optim.Adam / AdamW update on a contiguous parameter range (audio_gru_whole.py:307 AdamW
 * with two weight-decay groups; audio_bilstm_perm.py:250 Adam).  step is the 1-based count. */
int dep_adam_step(float* p, const float* g, float* m, float* v, long n, float lr, float beta1,
                  float beta2, float eps, float weight_decay, int decoupled, int step, void* stream);

/* Global-norm gradient clipping (torch.nn.utils.clip_grad_norm_, norm_type 2, error_if_nonfinite=False) without a host read.
 *   dep_grad_sqnorm       : S = sum of g^2 over up to 16 ranges (bufs[r], counts[r]) -- HOST arrays of 16-byte aligned device
 *                           pointers and element counts >= 1 -- accumulated in fp64 (the product of two fp32 values is exact
 *                           there) into `partials`: dep_grad_norm_slots() doubles on the device, caller-owned, all overwritten.
 *                           Slot s sums the chunks s, s + slots, ... (dep_grad_norm_chunk() floats each) of the CONCATENATED
 *                           ranges in that order, one workgroup per slot, fixed tree, plain stores, no atomics: the result is a
 *                           pure function of the data -- the same bits on every run and every rank, and the same bits however
 *                           the data is cut into ranges.  One launch.
 *   dep_adam_step_clipped : dep_adam_step on g * coef.  Every workgroup sums the partials in slot order (fixed tree: the same bits
 *                           everywhere) and forms, in double,
 *                               norm = sqrt(S) ;  coef = (float) min(1, max_norm / (norm + 1e-6))         (torch's formula)
 *                           with ONE rounding to fp32; g is not written.  coef == 1 gives dep_adam_step's bits.  max_norm <= 0
 *                           or +inf: measure only (coef = 1).  skip_nonfinite != 0 and S not finite: p, m, v are left untouched
 *                           bit for bit; the caller's step number still advances, i.e. a skipped step counts in the bias
 *                           correction (dep_adam_step_opt's landed count is the form in which it does not).  skip_nonfinite == 0: the arithmetic follows (coef = 0 for S = inf, NaN for S = NaN).
 *                           clip_out (4 floats, or NULL) = [coef, norm, S finite ? 1 : 0, 0].  stats (4 doubles, or NULL), a
 *                           running record: [0] += 1, [1] += 1 if coef < 1, [2] += 1 if the step was skipped, [3] = max([3], norm)
 *                           over finite norms; pass it to ONE launch per optimizer step.  Both are written by workgroup 0.
 *   dep_grad_clip_scale   : g *= coef in place over the ranges (coef as above), one launch; what clip_grad_norm_ leaves in .grad.
 *                           dep_grad_clip_scale followed by dep_adam_step gives dep_adam_step_clipped's bits.
 * Nothing allocates or synchronises; the argument checks (NULL, nranges outside 1..16, count <= 0, a NaN max_norm) come before any
 * HIP call. */
int dep_grad_norm_slots(void);
int dep_grad_norm_chunk(void);
int dep_grad_sqnorm(const float* const* bufs, const long* counts, int nranges, double* partials, void* stream);
int dep_adam_step_clipped(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2,
                          float eps, float weight_decay, int decoupled, int step, const double* partials, float max_norm,
                          int skip_nonfinite, float* clip_out, double* stats, void* stream);
int dep_grad_clip_scale(float* const* bufs, const long* counts, int nranges, const double* partials, float max_norm,
                        float* clip_out, void* stream);

/* Gradient accumulation over micro-batches: every backward WRITES its gradients, so a caller that wants K backward passes per
 * update adds each pass's gradients into an accumulator of its own and steps from that.
 *   dep_grad_accumulate   : over up to 16 range pairs (acc[r], g[r], counts[r]) -- HOST arrays of 16-byte aligned device pointers,
 *                           counts >= 1, acc and g not overlapping -- in ONE launch
 *                               t = fp32(g[i] * scale) ;  acc[i] = first ? t : fp32(acc[i] + t)
 *                           two roundings, never contracted into an FMA: numpy float32 gives the same bits, and scale == 1 is the
 *                           plain IEEE add.  first != 0: acc is not read (it may hold anything, NaN included: no memset needed).
 *                           scale serves the `loss / K` idiom; a caller whose losses already divide by the rows of the whole
 *                           accumulated batch passes 1.  partials != NULL (dep_grad_norm_slots() doubles): the same pass also
 *                           leaves the partial sums of squares of the STORED result, bit-identical to dep_grad_sqnorm(acc, counts,
 *                           nranges, ...) run afterwards (the same chunks per slot, the same vector / element paths, the same
 *                           fixed trees, no atomics), so that the last accumulation of a group feeds dep_adam_step_clipped
 *                           without a launch of its own for the norm.
 * Nothing allocates or synchronises; the argument checks (NULL, nranges outside 1..16, count <= 0, a misaligned pointer, a NaN
 * scale) come before any HIP call. */
int dep_grad_accumulate(float* const* acc, const float* const* g, const long* counts, int nranges, float scale, int first,
                        double* partials, void* stream);

/* AMSGrad and a fused average of the parameters (torch.optim.Adam[W](amsgrad=True); torch.optim.swa_utils.AveragedModel with
 * get_ema_multi_avg_fn(d)), inside the ONE launch per range the optimizer already makes.
 *   dep_adam_step_ext     : partials == NULL: dep_adam_step (its grid; max_norm, skip_nonfinite, clip_out, stats are ignored).
 *                           partials != NULL: dep_adam_step_clipped, its contract in every word -- coefficient, measure-only mode,
 *                           the clip_out / stats record, workgroup 0 as the writer.  `ext` adds, per element and after v is updated:
 *                               vmax != NULL:  vmax = max(vmax, v) ;  denom = sqrtf(vmax) * inv_sqrt_bc2 + eps
 *                                              (torch's non-capturable single-tensor path; vmax is zero before step 1)
 *                               ema  != NULL:  ema = fma(1 - d, p_new - ema, ema)   with d = ema_decay in [0, 1)
 *                                              (Tensor.lerp_'s form for a weight below one half, no bias correction; p_new == ema
 *                                              keeps ema).  ema_first != 0, or d == 0: ema = p_new exactly and ema is NOT read (it
 *                                              may hold anything, NaN included) -- AveragedModel's first update, and the `first`
 *                                              idiom of dep_grad_accumulate: no initialisation launch.
 *                           A skipped step (skip_nonfinite, S not finite) leaves p, m, v, vmax and ema untouched bit for bit.
 *                           ext == NULL, or both pointers NULL: the launches, and so the bits, of dep_adam_step / dep_adam_step_clipped.
 *   dep_swap              : a[i] <-> b[i] for n floats, as 32-bit words (NaN payloads and signed zeros survive); one launch.  The
 *                           optimizer's averaged() exchanges a parameter buffer with its average through it, and back.
 * Nothing allocates or synchronises; refused before any HIP call: what dep_adam_step / dep_adam_step_clipped refuse, ema != NULL
 * with a NaN ema_decay or one outside [0, 1), vmax or ema overlapping p / g / m / v or each other; dep_swap with NULL, n <= 0, a
 * pointer that is not 16-byte aligned, or overlapping ranges. */
typedef struct {
    float* vmax;       /* AMSGrad: running element-wise maximum of v, n floats, caller-owned, zero before step 1; NULL = off */
    float* ema;        /* average of p, n floats, caller-owned; NULL = off */
    float  ema_decay;  /* d in [0, 1) */
    int    ema_first;  /* != 0: ema is NOT read (it may hold anything, NaN included) and becomes p_new exactly */
} dep_adam_ext;
int dep_adam_step_ext(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2, float eps,
                      float weight_decay, int decoupled, int step, const dep_adam_ext* ext,
                      const double* partials, float max_norm, int skip_nonfinite, float* clip_out, double* stats, void* stream);
int dep_swap(float* a, float* b, long n, void* stream);   /* a[i] <-> b[i], bits exchanged; a, b 16-byte aligned, not overlapping */

/* Value clamp (torch.nn.utils.clip_grad_value_), a norm per parameter group, and skipped steps that do not count in the bias
 * correction (the torch loop that calls step() only when the norm is finite), inside the launches the update already makes.
 *   dep_grad_clip_value   : g = clamp(g) in place over up to 16 ranges (as dep_grad_clip_scale takes them), one launch, with
 *                               clamp(x) = x > c ? c : (x < -c ? -c : x)
 *                           by comparisons, as Tensor.clamp_: a NaN stays NaN, +-inf becomes +-c, -0.0f stays -0.0f.
 *                           dep_grad_clip_value followed by dep_adam_step gives the bits of dep_adam_step_opt's fused clamp.
 *   dep_adam_step_opt     : dep_adam_step_ext with `opt`'s three additions; every other argument has dep_adam_step_ext's meaning.
 *                           opt == NULL, or {0, 1, 0, NULL, NULL, NULL, NULL}: dep_adam_step_ext itself, its launches and its bits.
 *                           Otherwise ONE launch (partials == NULL too: coefficient 1, no record; max_norm, skip_nonfinite, clip_out
 *                           and stats are ignored then).
 *                             max_grad_value c > 0: the update sees clamp(g * coef); g is not written.  Torch's order: the norm is
 *                               that of the raw gradients, the clamp follows the coefficient, coupled weight decay follows the clamp.
 *                               A clamp that never binds gives the bits of the same call without it.
 *                             ngroups G in 1..8, group in [0, G): `partials` holds G slices of dep_grad_norm_slots() doubles, slice k
 *                               written by a dep_grad_sqnorm over group k's ranges.  Every workgroup sums EVERY slice with the fixed
 *                               tree of dep_adam_step_clipped and applies its formula with group_max_norm[k] (group_max_norm == NULL,
 *                               allowed for G == 1 only: with max_norm; otherwise max_norm is not read).  This launch scales g by coef[group].  skip_nonfinite is a decision
 *                               about the whole step: it is skipped iff ANY S_k is not finite.  clip_out = [smallest coef,
 *                               sqrt(sum of S_k) formed in double, all finite ? 1 : 0, 0]; stats as in dep_adam_step_clipped with
 *                               "clipped" = smallest coef < 1; group_out (2 G floats, or NULL) = [coef_k, norm_k] per group, written
 *                               by workgroup 0 like the other two.  G == 1 gives dep_adam_step_ext's bits, record included.
 *                             landed_in != NULL (needs partials and skip_nonfinite): one int on the device, the number of updates
 *                               that landed before this step.  `step` no longer enters the arithmetic: the bias factors are formed
 *                               on the device in double from t = *landed_in + 1,
 *                                   step_size = (float)(lr / (1 - beta1^t)) ;  inv_sqrt_bc2 = (float)(1 / sqrt(1 - beta2^t))
 *                               with the fp32 betas widened and beta^t the integer power by squaring (at most 62 products: within
 *                               7e-15 of the exact power; it need not have the bits of the host's pow).  landed_out (NULL in all
 *                               but ONE launch of an optimizer step) receives, from workgroup 0, *landed_in for a skipped step and
 *                               *landed_in + 1 otherwise.  It must be ANOTHER word than landed_in, because the other launches of
 *                               the step still read that one: the caller alternates between two words from step to step.  No
 *                               atomics, no host read; every launch of a step reads the same count.
 *                           A skipped step leaves p, m, v, vmax, ema and *landed_in untouched bit for bit.
 * Nothing allocates or synchronises; refused before any HIP call: what dep_adam_step_ext / dep_grad_clip_scale refuse, a clip_value
 * or max_grad_value that is negative, NaN or infinite (clip_value: zero as well), ngroups outside 1..8, group outside [0, ngroups),
 * ngroups > 1 without partials or without group_max_norm, a NaN bound, group_out without partials, landed_in without partials and
 * skip_nonfinite, landed_out without landed_in or equal to it. */
typedef struct {
    float        max_grad_value;  /* c > 0: clamp g * coef to [-c, c]; 0 = off */
    int          ngroups;         /* G in 1..8: slices of dep_grad_norm_slots() doubles in `partials` (1: the global norm) */
    int          group;           /* the group this range belongs to */
    const float* group_max_norm;  /* HOST array of G bounds (<= 0 or +inf: measured, not clipped), used whenever given; NULL (G == 1): max_norm */
    float*       group_out;       /* device, 2 G floats [coef_k, norm_k], or NULL */
    const int*   landed_in;       /* device, updates landed so far, or NULL: `step` counts as in dep_adam_step */
    int*         landed_out;      /* device, the count after this step, or NULL; never landed_in */
} dep_adam_opt;
int dep_grad_clip_value(float* const* bufs, const long* counts, int nranges, float clip_value, void* stream);
int dep_adam_step_opt(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2, float eps,
                      float weight_decay, int decoupled, int step, const dep_adam_ext* ext,
                      const double* partials, float max_norm, int skip_nonfinite, float* clip_out, double* stats,
                      const dep_adam_opt* opt, void* stream);

/* ------------------------------------------------------------------ feature front-end */
/* wav2vlad of Classification/audio_features_whole.py:57-72: log-mel spectrogram (librosa.feature.melspectrogram defaults:
 * n_fft 2048, hop 512, periodic Hann, centred frames with reflect padding, power 2, 80 Slaney mel filters) followed by
 * loupe_keras.NetVLAD(feature_size 80, cluster_size 16, output_dim 256).  The five contractions run on dep_gemm_f32
 * (windowed frames x [cos | -sin] DFT basis, power x mel filters, frames x cluster weights, assignment^T x frames,
 * VLAD x hidden weights); these entry points are the passes between them.
 *   dep_frame_window   : out (n_frames, n_fft) = reflect-padded y framed at `hop`, times the periodic Hann window.  The padding is
 *                        n_fft/2 samples on each side (integer division, numpy 'reflect'), so n > n_fft/2 and
 *                        1 <= n_frames <= 1 + (n + 2*(n_fft/2) - n_fft) / hop; one frame more is DEP_ERR_ARG (odd n_fft included)
 *   dep_power_spectrum : reim (rows, ld) = [re(0..bins) | im(0..bins)], ld >= 2*bins -> power (rows, bins) = re^2 + im^2;
 *                        (one fma: within 1 ulp); columns from 2*bins on are never read
 *   dep_log_floor      : y = log(max(floor, x)), floor > 0               (np.log(np.maximum(1e-6, melspec)))
 *                        with numpy's semantics: a NaN stays a NaN, +inf stays +inf, anything below the floor (0, negative
 *                        values, denormals, -inf) gives log(floor).  x == y (in place) is allowed
 *   dep_row_softmax    : softmax over the last axis, 1 <= C <= 64        (NetVLAD soft assignment).  z == p (in place) is allowed.
 *                        The shift by the row maximum is compensated (exact), so small probabilities keep their relative accuracy:
 *                        |p - softmax| <= (C + 8) 2^-24 softmax; an entry of -inf gives exactly 0
 *   dep_vlad_normalize : vkf (K,F) = assignment^T x frames, a_sum (K), w2 (F,K) -> out (F*K) = l2norm_all(l2norm_f(vkf^T - a_sum*w2)),
 *                        l2norm = x * rsqrt(max(sum x^2, 1e-12)).  One workgroup with the whole tensor in LDS: any K >= 1 (also
 *                        above the 256 threads of the block), and (F*K + K + 1) * 4 bytes <= 64 KiB, computed in 64 bits;
 *                        more is DEP_ERR_ARG
 * A refused call launches nothing and writes nothing. */
int dep_frame_window(const float* y, long n, int n_fft, int hop, int n_frames, float* out, void* stream);
int dep_power_spectrum(const float* reim, int rows, int bins, int ld, float* power, void* stream);
int dep_log_floor(const float* x, float* y, long n, float floor_value, void* stream);
int dep_row_softmax(const float* z, float* p, int rows, int C, void* stream);
int dep_vlad_normalize(const float* vkf, const float* a_sum, const float* w2, float* out, int F, int K, void* stream);

/* ------------------------------------------------------------------ profiling ------ */
/* Optional per-kernel timing with HIP events recorded on the launch stream (used by bench.py for the
 * roofline figure).  Categories: 0 GRU fwd sweep, 1 GRU bwd sweep, 2 LSTM fwd sweep, 3 LSTM bwd sweep,
 * 4 GEMM NT (input projection / Linear), 5 GEMM NN (dX), 6 GEMM TN (weight gradients; the split-K
 * reduce pass is not included).  dep_profile_read sums launch durations (ms) and counts per
 * category, then resets. */
int dep_profile_enable(int on);
int dep_profile_read(double* total_ms, int* counts, int ncat);

/* Launch-instance log (test infrastructure of the parity suite, tests/test_step_coverage_gpu.py): while enabled, every
 * kernel launch of the library records its template instance (kernel expression + launcher signature), once per distinct
 * instance.  dep_instance_log_enable(1) clears and starts, (0) stops.  dep_instance_log_read copies the newline-separated
 * list into buf (NUL-terminated, truncated to cap; buf may be NULL) and returns the bytes the full list needs; reset != 0
 * empties the log afterwards.  Process-wide, thread-safe; one relaxed atomic load per launch when off. */
int dep_instance_log_enable(int on);
long dep_instance_log_read(char* buf, long cap, int reset);
/* Every row of the instance tables of the co-resident ("cluster") sweep families -- the per-layer GRU sweeps, the 16-unit-member GRU
 * forward, the BiLSTM sweeps and the fused two-layer GRU forward / backward -- under the text the launch-instance log records for it,
 * rows that only an environment switch selects included (tests/test_zz_instance_tables_gpu.py: every row must have been launched by an
 * oracle-comparing test).  Newline-separated, no duplicates; buf, cap and the return value as dep_instance_log_read.  Needs no GPU. */
long dep_instance_table_read(char* buf, long cap);

/* Enqueue-order log (test infrastructure of the data-parallel path, tests/test_dp_gpu.py): while enabled, every kernel launch and every
 * collective the library enqueues ("K <kernel>" / "C <what> n=<floats>") is appended IN HOST ENQUEUE ORDER, together with the notes the
 * host adds through dep_order_log_note ("N <text>": the stream joins, the phases of a train step).  The two launches that need every CU
 * (the fused GRU forward / backward) must never have a collective enqueued in front of them that is not joined: the test asserts that on
 * this log.  dep_order_log_enable(1) clears and starts, (0) stops; dep_order_log_read as dep_instance_log_read (newline-separated). */
int dep_order_log_enable(int on);
int dep_order_log_note(const char* text);
long dep_order_log_read(char* buf, long cap, int reset);

/* ------------------------------------------------------------------ misc ----------- */
int dep_fill(float* p, long n, float value, void* stream);
/* y = a*x + b*y */
int dep_axpby(const float* x, float* y, long n, float a, float b, void* stream);
/* sigmoid gating of the regression fusion head: y = sigmoid(g) * x (Regression/fuse_net.py:345-351) */
int dep_sigmoid_gate(const float* g, const float* x, float* y, long n, void* stream);
/* Host-loop bookkeeping of train() / evaluate() as HIP kernels (round 4), so that the tensors really are storage only:
 *   dep_gather_rows  : dst[r] = src[idx[r]] for nrows <= 65535 rows of row_floats floats -- the mini-batch
 *                      X_train[lo:hi] of Classification/audio_gru_whole.py:170-172 out of the HBM-resident corpus
 *   dep_copy2d       : dst[r*ldd + c] = src[r*lds + c] -- torch.cat((text_feature, audio_feature), dim=1), fuse_net_whole.py:434
 *   dep_argmax_count : pred[b] = first arg-max of row b (output.data.max(1)[1]); *count += #(pred == label)
 *                      (pred.eq(y).sum(), audio_gru_whole.py:185-187); labels int32 or (labels_i64) int64; pred / count may be NULL */
/* Epoch-level loss bookkeeping in ONE launch per step (nn.LossSum): acc[0] += *loss in float64 (`total_loss += loss.item()`,
 * audio_gru_whole.py:195, without the per-step host sync), acc[1] = max(acc[1], *status), acc[2] = max(acc[2], *soft) -- the cluster
 * sweeps' status word (dep_rnn_status) and fallback word (dep_rnn_set_exclusive) of the step.  Any of loss / status / soft may be NULL. */
int dep_loss_accumulate(const float* loss, const unsigned* status, const unsigned* soft, double* acc, void* stream);
int dep_gather_rows(const float* src, const long long* idx, float* dst, long nrows, long row_floats, void* stream);
int dep_copy2d(const float* src, long lds, float* dst, long ldd, long rows, long cols, void* stream);
int dep_argmax_count(const float* p, const void* labels, int labels_i64, int B, int C, long long* count, long long* pred,
                     void* stream);
/* Bookkeeping of a chunked scoring run over a padded batch (AudioGRU.stream() with per-chunk lengths), no host read anywhere:
 *   dep_stream_accumulate : acc[b, :] += part[b, :] (one chunk's sum pool, (B,H)) and totals[b] += min(max(lengths[b], 0), Tc) -- the
 *                           frames of recording b seen so far; lengths and totals are device int32 vectors of B values;
 *   dep_stream_finish     : pooled[b, :] = acc[b, :] * (1 / totals[b]) when mean != 0 (a total of 0 gives a row of 0.0: it divides by
 *                           nothing), acc[b, :] when mean == 0. */
int dep_stream_accumulate(const float* part, const int32_t* lengths, float* acc, int32_t* totals, int B, int H, int Tc, void* stream);
int dep_stream_finish(const float* acc, const int32_t* totals, float* pooled, int B, int H, int mean, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DEP_RNN_H */
