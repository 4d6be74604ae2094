"""The three model families of the hot path, each a forward + explicit backward over libdep_rnn.so.

  AudioGRU   -- `AudioBiLSTM` of Classification/audio_gru_whole.py:24-108 (variant 'clf': LayerNorm,
                mean pool, Softmax) and Regression/audio_bilstm_perm.py:45-127 ('reg': no LN, sum pool, ReLU);
                config['bidirectional'] = True: [LN] -> BiGRU -> attention_net_with_w(output, h_n) in place of the pool
  TextBiLSTM -- Classification/text_bilstm_whole.py:23-114 ('clf') / Regression/text_bilstm_perm.py:37-124 ('reg')
  FusionNet  -- `fusion_net` + `MyLoss` of Classification/fuse_net_whole.py:245-395 ('clf') and
                Regression/fuse_net.py:224-366 ('reg')

Parameter names, shapes and order reproduce the reference's state_dict() (they are API: the fusion
script transplants weights by name, fuse_net_whole.py:566-588).  Dropout masks come from Philox keyed
by a per-forward seed; `eval()` disables them like nn.Dropout / nn.GRU(dropout=...).
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib as L
from . import nn
from . import parallel


def _rnn_names(prefix, F, H, Lyr, dirs, G):
    out = []
    for l in range(Lyr):
        for d in range(dirs):
            s = f'l{l}' + ('_reverse' if d else '')
            inp = F if l == 0 else H * dirs
            out += [(f'{prefix}.weight_ih_{s}', (G * H, inp)), (f'{prefix}.weight_hh_{s}', (G * H, H)),
                    (f'{prefix}.bias_ih_{s}', (G * H,)), (f'{prefix}.bias_hh_{s}', (G * H,))]
    return out


def _local_lstm_choice(value, what, F, H, Lyr):
    """A model's choice of forward-only text sweeps: None -> impl 0 (the default plan: the cluster BiLSTM where it exists), 8 ->
    L.IMPL_LOCAL_LSTM, the exchange-free forward that needs no co-resident workgroups (H = 128).  Anything else is a DepError."""
    if value is None:
        return L.IMPL_AUTO
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or int(value) != L.IMPL_LOCAL_LSTM:
        raise L.DepError(f'{what}: None (the default sweeps) or {L.IMPL_LOCAL_LSTM} (the exchange-free LSTM forward), got {value!r}')
    probe = L.RnnDesc(L.CELL_LSTM, 1, 1, F, H, Lyr, 2, L.RUN_EVAL, 0.0, 0, L.POOL_NONE, L.IMPL_LOCAL_LSTM)
    lib = L.load()
    if lib.dep_rnn_workspace_bytes(probe) == 0:
        raise L.DepError(f'{what} = {L.IMPL_LOCAL_LSTM}: ' + lib.dep_last_error().decode())
    return L.IMPL_LOCAL_LSTM


def _local_lstm_train_choice(value, what, F, H, Lyr):
    """A model's choice of training sweeps for its text BiLSTM: None -> impl 0 (the default plan), 9 -> L.IMPL_LOCAL_LSTM_TRAIN, the
    exchange-free forward and backward that need no co-resident workgroups (H = 128).  Anything else is a DepError."""
    if value is None:
        return L.IMPL_AUTO
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or int(value) != L.IMPL_LOCAL_LSTM_TRAIN:
        raise L.DepError(f'{what}: None (the default sweeps) or {L.IMPL_LOCAL_LSTM_TRAIN} (the exchange-free LSTM sweeps, forward and backward), got {value!r}')
    probe = L.RnnDesc(L.CELL_LSTM, 1, 1, F, H, Lyr, 2, L.RUN_TRAIN, 0.0, 0, L.POOL_NONE, L.IMPL_LOCAL_LSTM_TRAIN)
    lib = L.load()
    if lib.dep_rnn_workspace_bytes(probe) == 0:
        raise L.DepError(f'{what} = {L.IMPL_LOCAL_LSTM_TRAIN}: ' + lib.dep_last_error().decode())
    return L.IMPL_LOCAL_LSTM_TRAIN


class _RnnCache:
    """dep_rnn descriptors + reserve/workspace per (B,T,run mode) so steady-state steps never allocate."""

    def __init__(self, cell, F, H, Lyr, dirs, p, pool, device, impl=0):
        self.args = (cell, F, H, Lyr, dirs, p, pool, device)
        self.impl = impl             # dep_rnn_desc.impl of every descriptor of this cache
        self.cache = {}

    @staticmethod
    def lengths_on(lengths, B, device):
        """A model call's `lengths` (None = dense; a sequence / array / tensor of B ints) as the int32 device vector the ragged
        entry points read."""
        if lengths is None:
            return None
        t = lengths if torch.is_tensor(lengths) else torch.as_tensor(np.asarray(lengths))
        if t.is_floating_point() or t.dim() != 1 or t.numel() != B:
            raise L.DepError(f'lengths: expected {B} integers, one per utterance, got {tuple(t.shape)} {t.dtype}')
        return t.to(device=device, dtype=torch.int32).contiguous()

    def get(self, B, T, training):
        """training: a run mode (L.RUN_*); a bool means RUN_TRAIN / RUN_EVAL."""
        training = int(training)
        key = (B, T, training)
        r = self.cache.get(key)
        if r is None:
            cell, F, H, Lyr, dirs, p, pool, device = self.args
            if len(self.cache) > 6:
                self.cache.clear()
            r = L.Rnn(cell, B, T, F, H, Lyr, dirs, training, p if training else 0.0, pool, device, impl=self.impl)
            self.cache[key] = r
        self.last = r
        return r

    def check(self):
        """dep_rnn_status of the most recently used stack (synchronises; raises DepError if a sweep gave up)."""
        if getattr(self, 'last', None) is not None:
            self.last.check()

    def status_word(self):
        return self.last.status_word() if getattr(self, 'last', None) is not None else None

    def fallback_word(self):
        return self.last.fallback_word() if getattr(self, 'last', None) is not None else None


def _mlp_feature(x, W1, b1, p, seed, sites):
    """Dropout(p) -> Linear -> ReLU -> Dropout(p), forward only (the frozen encoders' heads in fusion_net.pretrained_feature):
    one launch when csrc/head.hip covers the widths, the three composed launches otherwise."""
    if x.is_contiguous() and W1.is_contiguous() and L.head_mlp_supported(W1.shape[1], W1.shape[0], 0):
        first = p > 0
        z1 = torch.empty(x.shape[0], W1.shape[0], dtype=torch.float32, device=x.device); a1 = torch.empty_like(z1)
        L.head_mlp_fwd(x, W1, b1, None, None, torch.empty_like(x) if first else None, z1, a1, None, p, seed, sites, first)
        return a1
    a0 = x
    if p > 0:
        a0 = torch.empty_like(x); L.dropout(x, a0, p, seed, sites[0])
    z = L.linear_fwd(a0, W1, b1)
    a1 = torch.empty_like(z); L.relu_dropout_fwd(z, a1, p, seed, sites[1])
    return a1


class _MLPHead:
    """[Dropout] -> Linear(H,H) -> ReLU -> Dropout -> [Linear(H,C)]   (fc_audio / fc_out Sequentials)."""

    def __init__(self, owner, n1, n2, p, first_dropout, sites):
        self.o = owner; self.n1 = n1; self.n2 = n2; self.p = p; self.first = first_dropout; self.sites = sites

    def forward(self, x, seed, training):
        o = self.o; P = o._params
        p = self.p if training else 0.0
        W1, b1 = P[self.n1 + '.weight'].data, P[self.n1 + '.bias'].data
        W2 = P[self.n2 + '.weight'].data if self.n2 is not None else None
        if x.is_contiguous() and W1.is_contiguous() and L.head_mlp_supported(W1.shape[1], W1.shape[0], 0 if W2 is None else W2.shape[0]):
            # one launch (csrc/head.hip): both dropouts, both Linears, the ReLU
            B, H1 = x.shape[0], W1.shape[0]
            first = bool(self.first and p > 0)
            a0 = torch.empty_like(x) if first else x
            z1 = torch.empty(B, H1, dtype=torch.float32, device=x.device); a1 = torch.empty_like(z1)
            z2 = torch.empty(B, W2.shape[0], dtype=torch.float32, device=x.device) if W2 is not None else None
            L.head_mlp_fwd(x, W1, b1, W2, P[self.n2 + '.bias'].data if W2 is not None else None, a0 if first else None,
                           z1, a1, z2, p, seed, self.sites, first)
            self.saved = (a0, z1, a1, p, seed)
            return z2 if W2 is not None else a1
        if self.first and p > 0:
            a0 = torch.empty_like(x); L.dropout(x, a0, p, seed, self.sites[0])
        else:
            a0 = x
        z1 = L.linear_fwd(a0, W1, b1)
        a1 = torch.empty_like(z1)
        L.relu_dropout_fwd(z1, a1, p, seed, self.sites[1])
        z2 = None
        if self.n2 is not None:
            z2 = L.linear_fwd(a1, W2, P[self.n2 + '.bias'].data)
        self.saved = (a0, z1, a1, p, seed)
        return z2 if self.n2 is not None else a1

    def backward(self, dz2):
        """dz2: grad of the second Linear's output (B,C). Returns grad of the head input (B,H)."""
        o = self.o; P = o._params
        a0, z1, a1, p, seed = self.saved
        W1, W2 = P[self.n1 + '.weight'], P[self.n2 + '.weight']
        B, Cc = dz2.shape; H = a1.shape[1]
        if (dz2.is_contiguous() and a0.is_contiguous() and W1.data.is_contiguous() and W1._grad.is_contiguous()
                and L.head_mlp_supported(a0.shape[1], H, Cc)):
            dx = torch.empty_like(a0); dz1 = torch.empty_like(z1)
            L.head_mlp_bwd(dz2, a0, z1, a1, W1.data, W2.data, W1._grad, P[self.n1 + '.bias']._grad, W2._grad,
                           P[self.n2 + '.bias']._grad, dx, dz1, p, seed, self.sites, bool(self.first and p > 0))
            return dx
        L.gemm(1, 0, Cc, H, B, dz2, Cc, a1, H, W2._grad, H)                       # dW2 = dz2^T a1
        L.colsum(dz2, P[self.n2 + '.bias']._grad)
        da1 = torch.empty_like(a1)
        L.gemm(0, 0, B, H, Cc, dz2, Cc, W2.data, H, da1, H)                        # da1 = dz2 W2
        dz1 = torch.empty_like(z1)
        L.relu_dropout_bwd(da1, z1, dz1, p, seed, self.sites[1])
        Hin = a0.shape[1]
        L.gemm(1, 0, H, Hin, B, dz1, H, a0, Hin, W1._grad, Hin)                    # dW1 = dz1^T a0
        L.colsum(dz1, P[self.n1 + '.bias']._grad)
        dx = torch.empty_like(a0)
        L.gemm(0, 0, B, Hin, H, dz1, H, W1.data, Hin, dx, Hin)
        if self.first and p > 0:
            L.dropout(dx, dx, p, seed, self.sites[0])
        return dx


class _AudioStream:
    """AudioGRU.stream(): chunked scoring of one batch of recordings with the memory of one chunk.  push() runs a chunk through the
    stack on the per-layer sweeps with the recurrent state carried in place (h_n written over hx, dep_rnn_forward_state) and adds the
    chunk's sum pool into an accumulator; output() is what model(x) returns for the chunks concatenated along T.
    Recordings of different lengths: push(chunk, lengths) with the live frames of each recording inside the chunk (0 once it has ended)
    runs the chunk through dep_rnn_forward_state_varlen -- an ended recording's state passes through -- and keeps per-row frame totals on
    the device; output() is then model(x_padded, lengths=totals).  No host read anywhere.
    Where the stream's descriptors run the per-layer cluster sweeps (impl 4) every push's status word is folded into a device-side
    accumulator (dep_loss_accumulate, one launch: each dep_rnn_forward clears the word); check_health() reads it."""

    def __init__(self, model, rnns):
        self.m = model
        self.rnns = rnns                           # the descriptor cache of this stream's impl
        self.health = None                         # float64 (3,) on the device once a push ran on a descriptor with a status word
        self.B = None
        self.T = 0
        self.totals = None                         # ragged pushes: int32 device vector (B), the frames of each recording so far
        if model.variant == 'clf':                 # LayerNorm's affine folded into layer 0, as encode() does (eval: the weights stand still)
            P = model._params
            L.ln_fold_fwd(model._rnn_w[0], model._rnn_w[2], P['ln.weight'].data, P['ln.bias'].data, *model._fold[:2])

    def push(self, chunk, lengths=None):
        """chunk: (B, Tc, F), host or device; Tc >= 1 and may differ from push to push, B is fixed by the first push.
        lengths: None (every recording has Tc frames in this chunk), or B integers in [0, Tc] -- a host array / sequence or an int32 device
        tensor: the live frames of each recording inside this chunk, contiguous from the recording's start (the caller's responsibility,
        as with every `lengths`); a recording that has ended pushes 0 from then on.  A stream takes lengths on every push or on none."""
        m = self.m
        x = m._to_dev(chunk)
        if x.dim() != 3 or x.shape[1] < 1 or x.shape[2] != m.embedding_size:
            raise L.DepError(f'stream.push: expected a (B, Tc >= 1, {m.embedding_size}) chunk, got {tuple(x.shape)}')
        B, Tc, F = x.shape
        if self.B is None:
            if B < 1:
                raise L.DepError('stream.push: an empty batch')
            self.B = B
            mk = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=m.device)
            self.h = mk(m.rnn_layers, B, m.hidden_dims)          # the carried state: zeros before the first chunk
            self.acc = mk(B, m.hidden_dims)                      # sum over all steps so far of the top layer's output
            self.part = mk(B, m.hidden_dims)                     # one chunk's sum
            if lengths is not None:
                self.totals = torch.zeros(B, dtype=torch.int32, device=m.device)
        elif B != self.B:
            raise L.DepError(f'stream.push: the batch size is fixed by the first push ({self.B}), got {B}')
        if (lengths is not None) != (self.totals is not None):
            raise L.DepError('stream.push: a stream takes lengths on every push or on none (the first push decides)')
        if lengths is not None:
            if torch.is_tensor(lengths) and lengths.is_cuda:
                lengths = L.check_lengths(lengths, B, m.device)              # a device vector is read in place: int32, B values
            else:
                lengths = _RnnCache.lengths_on(lengths, B, m.device)
        if m.variant == 'clf':                                   # LayerNorm is per row: per chunk, as encode() runs it
            xn, _ = L.layernorm_fwd(x.view(B * Tc, F), None, None, save=False)
            weights = m._rnn_w_fold
        else:
            xn, weights = x.view(B * Tc, F), m._rnn_w
        rnn = self.rnns.get(B, Tc, L.RUN_EVAL)
        if lengths is not None:
            rnn.forward_state_varlen(xn, weights, lengths, pooled=self.part, h_n=self.h, hx=self.h)
            L.stream_accumulate(self.part, lengths, self.acc, self.totals, Tc)
        else:
            rnn.forward(xn, weights, pooled=self.part, h_n=self.h, hx=self.h)
            L.axpby(self.part, self.acc, 1.0, 1.0)
        sw = rnn.status_word()
        if sw is not None:                         # cluster sweeps: the next push's forward clears the word, so keep its maximum
            if self.health is None:
                self.health = torch.zeros(3, dtype=torch.float64, device=m.device)
            L.loss_accumulate(None, sw, None, self.health)
        self.T += Tc

    def check_health(self):
        """Synchronises and raises DepError if a cluster sweep of any push so far gave up on a bounded spin (as model.check_health()
        does for model(x)); nothing to check on the tile-MFMA / generic sweeps."""
        if self.health is not None and float(self.health[1].item()) != 0:
            raise L.DepError('stream: a recurrent sweep gave up waiting for a cluster member during a push (status word %d): the GPU was '
                             'shared with another kernel; model.stream(impl=2) runs the sweeps that need no co-resident workgroups'
                             % int(self.health[1].item()))

    def output(self):
        m = self.m
        if self.T == 0:
            raise L.DepError('stream.output: nothing was pushed')
        pooled = torch.empty_like(self.acc)
        if self.totals is not None:                # the classifier's mean is over each recording's own frames (none: a row of zeros)
            L.stream_finish(self.acc, self.totals, pooled, m.variant == 'clf')
        else:
            L.axpby(self.acc, pooled, 1.0 / self.T if m.variant == 'clf' else 1.0, 0.0)      # the classifier pools by the mean over all steps
        z = m._head.forward(pooled, 0, False)
        out = torch.empty_like(z)
        L.head_loss(L.LOSS_CE_ON_SOFTMAX if m.variant == 'clf' else L.LOSS_L1_RELU, z, None, out, None, None, 1.0)
        return nn.Output(out, None, z)


class AudioGRU(nn.Module):
    def __init__(self, config, variant='clf', seed=None):
        super().__init__()
        self.variant = variant
        self.num_classes = config['num_classes']; self.learning_rate = config['learning_rate']
        self.dropout = float(config['dropout']); self.hidden_dims = H = config['hidden_dims']
        self.rnn_layers = Lyr = config['rnn_layers']; self.embedding_size = F = config['embedding_size']
        self.bidirectional = bi = bool(config.get('bidirectional', False))
        if bi:
            # ln -> BiGRU -> attention_net_with_w(output, h_n) -> fc_audio: the one bidirectional forward the reference class can express
            # without changing the shape of a parameter; fails here, by name, for a width no bidirectional sweep runs
            self._bi_impl = self._bidirectional_impl(F, H, Lyr)
        gen = nn.make_generator(seed)
        init = {}
        # definition order of the reference (named_parameters order); the attention pair is live in the bidirectional model alone
        self._add('attention_layer.0.weight', (H, H), live=bi); self._add('attention_layer.0.bias', (H,), live=bi)
        init.update(nn.default_linear_init('attention_layer.0.weight', 'attention_layer.0.bias', H, H, gen))
        rn = _rnn_names('lstm_net_audio', F, H, Lyr, 2 if bi else 1, 3)
        for n, s in rn:
            self._add(n, s)
        init.update(nn.default_rnn_init(rn, H, gen))
        self._buffers = {}
        if variant == 'clf':
            self._add('ln.weight', (F,)); self._add('ln.bias', (F,))
            init['ln.weight'] = np.ones(F, np.float32); init['ln.bias'] = np.zeros(F, np.float32)
        else:
            self._add('bn.weight', (3,), live=False); self._add('bn.bias', (3,), live=False)
            init['bn.weight'] = np.ones(3, np.float32); init['bn.bias'] = np.zeros(3, np.float32)
            self._buffers = {'bn.running_mean': torch.zeros(3), 'bn.running_var': torch.ones(3),
                             'bn.num_batches_tracked': torch.zeros((), dtype=torch.long)}
        self._add('fc_audio.1.weight', (H, H)); self._add('fc_audio.1.bias', (H,))
        self._add('fc_audio.4.weight', (self.num_classes, H)); self._add('fc_audio.4.bias', (self.num_classes,))
        init.update(nn.default_linear_init('fc_audio.1.weight', 'fc_audio.1.bias', H, H, gen))
        init.update(nn.default_linear_init('fc_audio.4.weight', 'fc_audio.4.bias', self.num_classes, H, gen))
        self._finalize(init)
        self._rnn_w = [self._params[n].data for n, _ in rn]
        self._rnn_g = [self._params[n]._grad for n, _ in rn]
        if bi:
            self._chunk_health = self._chunked = None            # (what check_health() and backward() look at; never set here)
            self._head = _MLPHead(self, 'fc_audio.1', 'fc_audio.4', self.dropout, True, (L.SITE_FC0, L.SITE_FC1))
            if variant == 'clf':
                # the fold as below, for the two first-layer maps (entries 0 / 2 and 4 / 6 of the weight list) in one launch each way:
                # dep_ln_fold_bwd_multi sums dgamma / dbeta over both directions
                mk = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=self.device)
                mat, vec = (lambda: [mk(3 * H, F), mk(3 * H, F)]), (lambda: [mk(3 * H), mk(3 * H)])
                self._fold2 = Wf, bf, dWf, dbf = mat(), vec(), mat(), vec()          # one per direction
                self._rnn_w_fold = list(self._rnn_w); self._rnn_g_fold = list(self._rnn_g)
                for d in (0, 1):
                    self._rnn_w_fold[4 * d], self._rnn_w_fold[4 * d + 2] = Wf[d], bf[d]
                    self._rnn_g_fold[4 * d], self._rnn_g_fold[4 * d + 2] = dWf[d], dbf[d]
            # eval and train on the same impl: a reserve goes with the impl that wrote it
            self._rnns = _RnnCache(L.CELL_GRU, F, H, Lyr, 2, self.dropout, L.POOL_NONE, self.device, impl=self._bi_impl)
            return
        if variant == 'clf':
            # LayerNorm's affine is folded into gru.weight_ih_l0 / bias_ih_l0 (dep_ln_fold_*): the stack runs on x-hat
            # with the folded pair and hands back their gradients, from which dW, db, dgamma, dbeta follow exactly --
            # no dL/d(xn) contraction and no pass over (B*T, F) for the two LayerNorm parameter gradients.
            mk = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=self.device)
            self._fold = (mk(3 * H, F), mk(3 * H), mk(3 * H, F), mk(3 * H))          # Wf, bf, dWf, dbf
            self._rnn_w_fold = [self._fold[0], self._rnn_w[1], self._fold[1]] + self._rnn_w[3:]
            self._rnn_g_fold = [self._fold[2], self._rnn_g[1], self._fold[3]] + self._rnn_g[3:]
        pool = L.POOL_MEAN if variant == 'clf' else L.POOL_SUM
        self._rnns = _RnnCache(L.CELL_GRU, F, H, Lyr, 1, self.dropout, pool, self.device)
        # stream(): descriptors on the per-layer sweeps, the kernels that take a recurrent state, eval mode, the chunk's SUM as its pool.
        # impl 4 (the per-layer cluster sweeps, W_hh in registers) where that descriptor exists -- its size query is non-zero: H in
        # {64, 128, 256, 512} -- and impl 2 elsewhere (the tile-MFMA sweeps where they can tile H, the generic sweeps otherwise)
        probe = L.RnnDesc(L.CELL_GRU, 1, 1, F, H, Lyr, 1, L.RUN_EVAL, 0.0, 0, L.POOL_SUM, L.IMPL_CLUSTER_PER_LAYER)
        self._stream_impl = L.IMPL_CLUSTER_PER_LAYER if L.load().dep_rnn_workspace_bytes(probe) != 0 else L.IMPL_TILE
        self._stream_rnns = {}                     # impl -> _RnnCache
        # forward_chunked(): the same choice among the sweeps that take a state through TRAINING -- impl 5 (the per-layer cluster sweeps,
        # state through training) where it exists, impl 2 elsewhere; chunk descriptors pool by the sum, like the stream's
        probe = L.RnnDesc(L.CELL_GRU, 1, 1, F, H, Lyr, 1, L.RUN_TRAIN, 0.0, 0, L.POOL_SUM, L.IMPL_CLUSTER_PER_LAYER_STATE)
        self._chunk_impl = L.IMPL_CLUSTER_PER_LAYER_STATE if L.load().dep_rnn_workspace_bytes(probe) != 0 else L.IMPL_TILE
        self._chunk_rnns = {}                      # impl -> _RnnCache
        self._chunk_health = None                  # float64 (3,) on the device once a chunk ran on a descriptor with a status word
        self._chunked = None                       # what forward_chunked() left for backward()
        self.keep_chunk_states = False             # debugging / tests: backward() keeps each recomputed chunk's h_n in _chunked['h_n_recomputed']
        self._head = _MLPHead(self, 'fc_audio.1', 'fc_audio.4', self.dropout, True, (L.SITE_FC0, L.SITE_FC1))

    @staticmethod
    def _bidirectional_impl(F, H, Lyr):
        """The sweeps of the bidirectional model: impl 7 (the per-layer cluster sweeps of a bidirectional GRU, forward and backward)
        where that descriptor exists -- its size query is non-zero -- else impl 2 where the tile-MFMA sweeps can tile H; else a
        DepError.  What impl 7 refuses later (a backward in GEMM mode 3, a ragged call in modes 2 / 3) is raised with the library's
        own message: the plan never changes silently."""
        def exists(impl):
            probe = L.RnnDesc(L.CELL_GRU, 1, 1, F, H, Lyr, 2, L.RUN_TRAIN, 0.0, 0, L.POOL_NONE, impl)
            return L.load().dep_rnn_workspace_bytes(probe) != 0
        if exists(L.IMPL_CLUSTER_BIGRU_TRAIN):
            return L.IMPL_CLUSTER_BIGRU_TRAIN
        if exists(L.IMPL_TILE):
            return L.IMPL_TILE
        raise L.DepError(f'AudioBiLSTM(bidirectional=True): no bidirectional GRU sweep runs hidden_dims = {H}: the per-layer cluster sweeps '
                         'take 64, 128, 256 and 512, the tile-MFMA sweeps 16, 32, 48, 96 and 192')

    def _refuse_chunks(self, what):
        if self.bidirectional:
            raise L.DepError(f'AudioGRU.{what}: a bidirectional encoder cannot be cut into chunks -- the reverse direction starts at the '
                             'last frame, so no chunk is final before the recording ends; model(x) scores the whole recording')

    def stream(self, impl=None):
        """Chunked scoring with bounded memory (eval mode only): s = model.stream(); s.push(chunk) ...; s.output() is model(x) for
        the chunks concatenated along T.  See _AudioStream.  impl: None = the model's choice (see __init__), or L.IMPL_TILE /
        L.IMPL_CLUSTER_PER_LAYER to name the sweeps (the latter only where the descriptor exists)."""
        self._refuse_chunks('stream')
        if self.training:
            raise L.DepError('AudioGRU.stream: streaming scores in eval() mode only (no dropout, no backward)')
        impl = self._stream_impl if impl is None else int(impl)
        if impl not in (L.IMPL_TILE, L.IMPL_CLUSTER_PER_LAYER):
            raise L.DepError(f'AudioGRU.stream: impl must name sweeps that take a recurrent state (2 or 4), got {impl}')
        if impl not in self._stream_rnns:
            self._stream_rnns[impl] = _RnnCache(L.CELL_GRU, self.embedding_size, self.hidden_dims, self.rnn_layers, 1, self.dropout,
                                                L.POOL_SUM, self.device, impl=impl)
        return _AudioStream(self, self._stream_rnns[impl])

    def state_dict(self):
        sd = super().state_dict()
        if self._buffers:
            out = type(sd)()
            for k, v in sd.items():
                out[k] = v
                if k == 'bn.bias':
                    out.update(self._buffers)
            return out
        return sd

    def load_state_dict(self, sd, strict=True):
        sd = {k: v for k, v in sd.items() if k not in self._buffers}
        return super().load_state_dict(sd, strict)

    def check_health(self):
        self._rnns.check()
        if self._chunk_health is not None and float(self._chunk_health[1].item()) != 0:
            raise L.DepError('forward_chunked: a recurrent sweep gave up waiting for a cluster member during a chunk (status word %d): the '
                             'GPU was shared with another kernel; forward_chunked(impl=2) runs the sweeps that need no co-resident workgroups'
                             % int(self._chunk_health[1].item()))

    def status_words(self):
        w = self._rnns.status_word()
        return [] if w is None else [w]

    def fallback_words(self):
        w = self._rnns.fallback_word()
        return [] if w is None else [w]

    # encoder part shared with FusionNet
    def encode(self, x, training, seed, lengths=None):
        """lengths: int32 device vector (B), the utterances' own lengths inside the padded batch (None: dense).  The padding
        must be finite (pad_ragged pads with zeros; LayerNorm maps a zero row to a zero row)."""
        if self.bidirectional:
            return self._encode_bidirectional(x, training, seed, lengths)
        B, T, F = x.shape
        P = self._params
        if self.variant == 'clf':
            xn, _ = L.layernorm_fwd(x.view(B * T, F), None, None, save=False)           # x-hat
            L.ln_fold_fwd(self._rnn_w[0], self._rnn_w[2], P['ln.weight'].data, P['ln.bias'].data, *self._fold[:2])
            weights = self._rnn_w_fold
        else:
            xn, weights = x.view(B * T, F), self._rnn_w
        rnn = self._rnns.get(B, T, training)
        pooled = torch.empty(B, self.hidden_dims, dtype=torch.float32, device=self.device)
        rnn.forward(xn, weights, seed=seed, pooled=pooled, lengths=lengths)
        return pooled, (x, xn, rnn, lengths)

    def _encode_bidirectional(self, x, training, seed, lengths):
        """x-hat (clf) -> BiGRU stack (no pool, h_n wanted) -> attention_net_with_w over the top sequence, read in place: the halves
        of the output summed, attention over the row's own steps, the final states of all layers and directions summed into the
        query.  A row of length 0 has ctx = 0."""
        B, T, F = x.shape
        P = self._params
        if self.variant == 'clf':
            xn, _ = L.layernorm_fwd(x.view(B * T, F), None, None, save=False)
            w = self._rnn_w
            L.ln_fold_fwd_multi([w[0], w[4]], [w[2], w[6]], P['ln.weight'].data, P['ln.bias'].data, *self._fold2[:2])
            weights = self._rnn_w_fold
        else:
            xn, weights = x.view(B * T, F), self._rnn_w
        rnn = self._rnns.get(B, T, training)
        h_n = torch.empty(2 * self.rnn_layers, B, self.hidden_dims, dtype=torch.float32, device=self.device)
        rnn.forward(xn, weights, seed=seed, h_n=h_n, lengths=lengths)
        out = rnn.layer_output()
        ctx, att = L.attn_fwd(out, h_n, P['attention_layer.0.weight'].data, P['attention_layer.0.bias'].data, lengths=lengths)
        return ctx, (x, xn, rnn, lengths, out, att)

    def forward(self, x, lengths=None):
        """lengths: the ragged call -- x is padded to its longest utterance, row b is lengths[b] steps long (mean / sum pool over
        its own steps; bidirectional: the reverse direction starts at its last step, the attention runs over its own steps); see
        _common.pad_ragged."""
        x = self._to_dev(x)
        lengths = _RnnCache.lengths_on(lengths, x.shape[0], self.device)
        training = self.training
        seed = nn.next_dropout_seed() if training else 0
        pooled, enc = self.encode(x, training, seed, lengths)
        z = self._head.forward(pooled, seed, training)
        out = torch.empty_like(z)
        kind = L.LOSS_CE_ON_SOFTMAX if self.variant == 'clf' else L.LOSS_L1_RELU
        L.head_loss(kind, z, None, out, None, None, 1.0)
        self._saved = enc
        self._chunked = None
        if self.bidirectional:
            self.last_alpha = enc[5][0]
        return nn.Output(out, self, z)

    def forward_chunked(self, x, chunk_steps, lengths=None, impl=None):
        """An exact training step over a long recording with the reserve of ONE chunk: the usual nn.Output, so criterion(out, y).backward()
        and the optimizers work as they are; chunk_steps >= T is one chunk and equals model(x).
        The forward runs the chunks of chunk_steps frames (the last may be shorter) in RUN_DROPOUT_ONLY -- the train masks bit for bit, no
        reserve kept -- with the recurrent state carried, keeps every chunk's incoming state hx_k (L, B, H) and its dropout seed, and
        accumulates the chunks' sum pools as stream() does (LayerNorm per chunk; mean / sum as encode(), per-row totals with lengths:
        chunk k gets clip(len - k * chunk_steps, 0, chunk)).  backward() then walks the chunks in reverse: re-runs chunk k in RUN_TRAIN
        from hx_k with its seed, runs the backward state call with the per-frame pool gradient, dh_n = the gradient that left chunk k + 1
        and dhx written back in place, and adds the chunk's weight gradients into the parameters' (the backward writes with beta = 0).
        impl: None = the model's choice (IMPL_CLUSTER_PER_LAYER_STATE where that descriptor exists, else IMPL_TILE: 43.4 ms against 364.9 ms
        at H = F = 256, B = 64, T = 3000 in chunks of 300, profiles/chunked_step_ab.txt), or one of the two, as stream(impl=) names its sweeps.
        check_health() covers the chunks of the latest step."""
        self._refuse_chunks('forward_chunked')
        if not self.training:
            raise L.DepError('AudioGRU.forward_chunked: a training step (model.train()); eval-mode chunked scoring is model.stream()')
        x = self._to_dev(x)
        if x.dim() != 3 or x.shape[1] < 1 or x.shape[2] != self.embedding_size or int(chunk_steps) < 1:
            raise L.DepError(f'forward_chunked: expected a (B, T >= 1, {self.embedding_size}) batch and chunk_steps >= 1, got {tuple(x.shape)}, {chunk_steps}')
        B, T, F = x.shape
        H, Lyr, chunk = self.hidden_dims, self.rnn_layers, min(int(chunk_steps), T)
        impl = self._chunk_impl if impl is None else int(impl)
        if impl not in (L.IMPL_TILE, L.IMPL_CLUSTER_PER_LAYER_STATE):
            raise L.DepError(f'AudioGRU.forward_chunked: impl must name sweeps that take a state through training (2 or 5), got {impl}')
        if impl not in self._chunk_rnns:
            self._chunk_rnns[impl] = _RnnCache(L.CELL_GRU, F, H, Lyr, 1, self.dropout, L.POOL_SUM, self.device, impl=impl)
        rnns = self._chunk_rnns[impl]
        lengths = _RnnCache.lengths_on(lengths, B, self.device)
        clf = self.variant == 'clf'
        P = self._params
        if clf:                                    # the weights stand still during the step: one fold for all chunks, forward and recompute
            L.ln_fold_fwd(self._rnn_w[0], self._rnn_w[2], P['ln.weight'].data, P['ln.bias'].data, *self._fold[:2])
        weights = self._rnn_w_fold if clf else self._rnn_w
        mk = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=self.device)
        h, acc, part = mk(Lyr, B, H), mk(B, H), mk(B, H)
        totals = torch.zeros(B, dtype=torch.int32, device=self.device) if lengths is not None else None
        if self._chunk_health is not None:         # a step's health is its own chunks', as model(x)'s status word is that call's
            self._chunk_health.zero_()
        cuts, seeds, hxs, lens = [], [], [], []
        for t0 in range(0, T, chunk):
            Tc = min(chunk, T - t0)
            xn = self._chunk_input(x, t0, Tc)
            lk = None if lengths is None else (lengths - t0).clamp_(0, Tc).to(torch.int32)
            seed = nn.next_dropout_seed()
            cuts.append((t0, Tc)); seeds.append(seed); hxs.append(h.clone()); lens.append(lk)
            rnn = rnns.get(B, Tc, L.RUN_DROPOUT_ONLY)
            if lk is not None:
                rnn.forward_state_varlen(xn, weights, lk, seed=seed, pooled=part, h_n=h, hx=h)
                L.stream_accumulate(part, lk, acc, totals, Tc)
            else:
                rnn.forward(xn, weights, seed=seed, pooled=part, h_n=h, hx=h)
                L.axpby(part, acc, 1.0, 1.0)
            self._fold_chunk_status(rnn)
        pooled = torch.empty_like(acc)
        if totals is not None:
            L.stream_finish(acc, totals, pooled, clf)
        else:
            L.axpby(acc, pooled, 1.0 / T if clf else 1.0, 0.0)
        z = self._head.forward(pooled, seeds[0], True)
        out = torch.empty_like(z)
        L.head_loss(L.LOSS_CE_ON_SOFTMAX if clf else L.LOSS_L1_RELU, z, None, out, None, None, 1.0)
        self._chunked = dict(x=x, T=T, cuts=cuts, seeds=seeds, hxs=hxs, lens=lens, totals=totals, rnns=rnns, impl=impl, h_end=h)
        return nn.Output(out, self, z)

    def _chunk_input(self, x, t0, Tc):
        """Frames [t0, t0 + Tc) of the batch as the (B * Tc, F) array the stack reads: LayerNorm's x-hat for the classifier (per row, so
        per chunk as encode() runs it on the whole batch)."""
        B, _, F = x.shape
        xc = x[:, t0:t0 + Tc].contiguous().view(B * Tc, F)
        if self.variant == 'clf':
            xc, _ = L.layernorm_fwd(xc, None, None, save=False)
        return xc

    def _fold_chunk_status(self, rnn):
        sw = rnn.status_word()
        if sw is not None:                         # cluster sweeps: the next chunk's forward clears the word, so keep its maximum
            if self._chunk_health is None:
                self._chunk_health = torch.zeros(3, dtype=torch.float64, device=self.device)
            L.loss_accumulate(None, sw, None, self._chunk_health)

    def _backward_chunked(self, dz):
        c = self._chunked
        x, T, rnns, totals = c['x'], c['T'], c['rnns'], c['totals']
        B = x.shape[0]
        clf = self.variant == 'clf'
        P = self._params
        dpool = self._head.backward(dz)
        # the gradient of one frame's contribution to the pool (the chunks' descriptors pool by the SUM): the classifier's mean divides
        # by T, or row by row by the recording's own frames
        dframe = torch.empty_like(dpool)
        if totals is not None:
            L.stream_finish(dpool, totals, dframe, clf)
        else:
            L.axpby(dpool, dframe, 1.0 / T if clf else 1.0, 0.0)
        weights = self._rnn_w_fold if clf else self._rnn_w
        grads = self._rnn_g_fold if clf else self._rnn_g
        scratch = [torch.empty_like(g) for g in grads]
        dh = torch.empty(self.rnn_layers, B, self.hidden_dims, dtype=torch.float32, device=self.device)
        # (dhx over dh_n in place is the cluster backward's rule; the tile sweeps get two buffers)
        dh_out = dh if c['impl'] == L.IMPL_CLUSTER_PER_LAYER_STATE else torch.empty_like(dh)
        K = len(c['cuts'])
        keep = self.keep_chunk_states
        c['h_n_recomputed'] = [None] * K if keep else None
        for k in range(K - 1, -1, -1):
            t0, Tc = c['cuts'][k]
            xn = self._chunk_input(x, t0, Tc)
            rnn = rnns.get(B, Tc, L.RUN_TRAIN)
            h_n = torch.empty_like(dh) if keep else None
            dh_n = None if k == K - 1 else dh
            kw = dict(dpooled=dframe, dh_n=dh_n, dx=None, hx=c['hxs'][k], dhx=dh_out)
            if c['lens'][k] is not None:
                rnn.forward_state_varlen(xn, weights, c['lens'][k], seed=c['seeds'][k], h_n=h_n, hx=c['hxs'][k])
                rnn.backward_state_varlen(xn, weights, scratch, c['lens'][k], **kw)
            else:
                rnn.forward(xn, weights, seed=c['seeds'][k], h_n=h_n, hx=c['hxs'][k])
                rnn.backward(xn, weights, scratch, **kw)
            self._fold_chunk_status(rnn)
            if keep:
                c['h_n_recomputed'][k] = h_n
            for s, g in zip(scratch, grads):
                L.axpby(s, g, 1.0, 0.0 if k == K - 1 else 1.0)
            dh, dh_out = dh_out, dh
        if clf:
            L.ln_fold_bwd(self._rnn_w[0], self._fold[2], self._fold[3], P['ln.weight'].data, P['ln.bias'].data,
                          self._rnn_g[0], self._rnn_g[2], P['ln.weight']._grad, P['ln.bias']._grad)
        self._grad_ready = True
        in_call, post = self.sync_plan()           # data parallel: nothing is final inside a chunk's call, every range goes out at the end
        parallel.finish_grad_sync(self, {}, list(in_call.values()) + list(post))

    def sync_plan(self):
        """Flat layout [ln | l0 | l1 | .. | fc_audio]: the top layer's range ends with the head (final before the stack's
        backward starts); layer 0 of the classifier is final only after dep_ln_fold_bwd, together with the LayerNorm pair that
        sits right in front of it -- ONE contiguous range, so a 2-layer step is two all-reduces."""
        Lyr, px = self.rnn_layers, 'lstm_net_audio'
        in_call, post = {}, []
        if self.bidirectional:
            # [ln | attention | l0 (both directions) | l1 .. | fc_audio]: the attention pair sits in front of layer 0 and goes with it,
            # as in TextBiLSTM.sync_plan; the classifier's layer 0 waits for dep_ln_fold_bwd_multi, so there LayerNorm pair, attention
            # pair and layer 0 are ONE contiguous range reduced after the backward.  The head rides with the top layer.
            for l in range(Lyr):
                first = 'attention_layer.0.weight' if l == 0 else f'{px}.weight_ih_l{l}'
                last = 'fc_audio.4.bias' if l == Lyr - 1 else f'{px}.bias_hh_l{l}_reverse'
                if l == 0 and self.variant == 'clf':
                    post.append(self._span('ln.weight', last))
                else:
                    in_call[l] = self._span(first, last)
            return in_call, post
        for l in range(Lyr):
            first, last = f'{px}.weight_ih_l{l}', ('fc_audio.4.bias' if l == Lyr - 1 else f'{px}.bias_hh_l{l}')
            if l == 0 and self.variant == 'clf':
                post.append(self._span('ln.weight', last))
            else:
                in_call[l] = self._span(first, last)
        return in_call, post

    def backward(self, dz):
        if self._chunked is not None:
            return self._backward_chunked(dz)
        if self.bidirectional:
            return self._backward_bidirectional(dz)
        x, xn, rnn, lengths = self._saved
        dpool = self._head.backward(dz)
        P = self._params
        in_call, post = self.sync_plan()
        gs = parallel.make_grad_sync(self, in_call)
        if self.variant == 'clf':
            rnn.backward(xn, self._rnn_w_fold, self._rnn_g_fold, dpooled=dpool, dx=None, grad_sync=gs, lengths=lengths)
            L.ln_fold_bwd(self._rnn_w[0], self._fold[2], self._fold[3], P['ln.weight'].data, P['ln.bias'].data,
                          self._rnn_g[0], self._rnn_g[2], P['ln.weight']._grad, P['ln.bias']._grad)
        else:
            rnn.backward(xn, self._rnn_w, self._rnn_g, dpooled=dpool, dx=None, grad_sync=gs, lengths=lengths)
        self._grad_ready = True
        parallel.finish_grad_sync(self, in_call, post)

    def _backward_bidirectional(self, dz):
        x, xn, rnn, lengths, out, att = self._saved
        P = self._params
        dctx = self._head.backward(dz)
        dout, dh_n = L.attn_bwd(dctx, out, P['attention_layer.0.weight'].data, att, 2 * self.rnn_layers,
                                P['attention_layer.0.weight']._grad, P['attention_layer.0.bias']._grad, lengths=lengths)
        in_call, post = self.sync_plan()
        gs = parallel.make_grad_sync(self, in_call)
        if self.variant == 'clf':
            rnn.backward(xn, self._rnn_w_fold, self._rnn_g_fold, dy=dout, dh_n=dh_n, dx=None, grad_sync=gs, lengths=lengths)
            w, g = self._rnn_w, self._rnn_g
            L.ln_fold_bwd_multi([w[0], w[4]], self._fold2[2], self._fold2[3], P['ln.weight'].data, P['ln.bias'].data,
                                [g[0], g[4]], [g[2], g[6]], P['ln.weight']._grad, P['ln.bias']._grad)
        else:
            rnn.backward(xn, self._rnn_w, self._rnn_g, dy=dout, dh_n=dh_n, dx=None, grad_sync=gs, lengths=lengths)
        self._grad_ready = True
        parallel.finish_grad_sync(self, in_call, post)


class TextBiLSTM(nn.Module):
    def __init__(self, config, variant='clf', seed=None, head_out=True, fc_idx=None):
        super().__init__()
        self.variant = variant
        self.num_classes = config['num_classes']; self.learning_rate = config['learning_rate']
        self.dropout = float(config['dropout']); self.hidden_dims = H = config['hidden_dims']
        self.rnn_layers = Lyr = config['rnn_layers']; self.embedding_size = F = config['embedding_size']
        self.bidirectional = config.get('bidirectional', True)
        if not self.bidirectional:
            raise L.DepError('TextBiLSTM: the reference runs a bidirectional LSTM (bidirectional=True)')
        i1, i2 = fc_idx if fc_idx else ((0, 3) if variant == 'clf' else (1, 4))
        self._fc = (f'fc_out.{i1}', f'fc_out.{i2}')
        gen = nn.make_generator(seed)
        shapes = [('attention_layer.0.weight', (H, H)), ('attention_layer.0.bias', (H,))]
        rn = _rnn_names('lstm_net', F, H, Lyr, 2, 4)
        shapes += rn
        shapes += [(self._fc[0] + '.weight', (H, H)), (self._fc[0] + '.bias', (H,)),
                   (self._fc[1] + '.weight', (self.num_classes, H)), (self._fc[1] + '.bias', (self.num_classes,))]
        init = {}
        for n, s in shapes:
            self._add(n, s)
            # init_weight(): xavier_uniform on every weight, 0 on every bias (text_bilstm_whole.py:37-43)
            init[n] = nn.xavier_uniform(s, gen) if 'weight' in n else np.zeros(s, np.float32)
        if variant == 'clf':
            for n, s in (('ln1.weight', (F,)), ('ln1.bias', (F,)), ('ln2.weight', (H,)), ('ln2.bias', (H,))):
                self._add(n, s, live=False)
                init[n] = np.ones(s, np.float32) if 'weight' in n else np.zeros(s, np.float32)
        self._finalize(init)
        self._rnn_w = [self._params[n].data for n, _ in rn]
        self._rnn_g = [self._params[n]._grad for n, _ in rn]
        # config['train_impl'] = 9: the model's one cache is built on the exchange-free sweeps -- train() and eval() forwards and the backward
        # all run on it, dense and ragged, single GPU or data parallel
        train_impl = _local_lstm_train_choice(config.get('train_impl'), "TextBiLSTM: config['train_impl']", F, H, Lyr)
        self._rnns = _RnnCache(L.CELL_LSTM, F, H, Lyr, 2, self.dropout, L.POOL_NONE, self.device, impl=train_impl)
        # config['eval_impl'] = 8: a forward in eval() mode runs the exchange-free LSTM forward (no backward follows it); training keeps its cache
        eval_impl = _local_lstm_choice(config.get('eval_impl'), "TextBiLSTM: config['eval_impl']", F, H, Lyr)
        self._eval_rnns = None if eval_impl == L.IMPL_AUTO else _RnnCache(L.CELL_LSTM, F, H, Lyr, 2, self.dropout, L.POOL_NONE, self.device, impl=eval_impl)
        self._head = _MLPHead(self, self._fc[0], self._fc[1], self.dropout, variant == 'reg', (L.SITE_FC0, L.SITE_FC1))

    def check_health(self):
        self._rnns.check()

    def status_words(self):
        w = self._rnns.status_word()
        return [] if w is None else [w]

    def fallback_words(self):
        w = self._rnns.fallback_word()
        return [] if w is None else [w]

    def sync_plan(self):
        """Flat layout [attention | l0 (both directions) | l1 .. | fc_out]: the attention pair (final before the stack's
        backward) rides with layer 0, the head with the top layer."""
        Lyr, px = self.rnn_layers, 'lstm_net'
        in_call = {}
        for l in range(Lyr):
            first = 'attention_layer.0.weight' if l == 0 else f'{px}.weight_ih_l{l}'
            last = (self._fc[1] + '.bias') if l == Lyr - 1 else f'{px}.bias_hh_l{l}_reverse'
            in_call[l] = self._span(first, last)
        return in_call, []

    def encode(self, x, training, seed, lengths=None):
        B, T, F = x.shape
        P = self._params
        rnns = self._eval_rnns if (self._eval_rnns is not None and int(training) == L.RUN_EVAL) else self._rnns
        rnn = rnns.get(B, T, training)
        h_n = torch.empty(2 * self.rnn_layers, B, self.hidden_dims, dtype=torch.float32, device=self.device)
        rnn.forward(x, self._rnn_w, seed=seed, h_n=h_n, lengths=lengths)
        out = rnn.layer_output()
        ctx, att = L.attn_fwd(out, h_n, P['attention_layer.0.weight'].data, P['attention_layer.0.bias'].data, lengths=lengths)
        return ctx, (x, rnn, out, att, lengths)

    def forward(self, x, lengths=None):
        """x: (B,T,F) batch-first like the reference's call site (it permutes to time-first internally,
        text_bilstm_whole.py:103; the HIP operator consumes batch-first directly).
        lengths: the ragged call -- row b is lengths[b] steps long (the reverse direction starts at its last step, the attention
        softmax runs over its own steps); see _common.pad_ragged."""
        x = self._to_dev(x)
        lengths = _RnnCache.lengths_on(lengths, x.shape[0], self.device)
        training = self.training
        seed = nn.next_dropout_seed() if training else 0
        ctx, enc = self.encode(x, training, seed, lengths)
        z = self._head.forward(ctx, seed, training)
        out = torch.empty_like(z)
        kind = L.LOSS_CE_ON_SOFTMAX if self.variant == 'clf' else L.LOSS_SMOOTHL1_RELU
        L.head_loss(kind, z, None, out, None, None, 1.0)
        self._saved = enc
        self.last_alpha = enc[3][0]
        return nn.Output(out, self, z)

    def backward(self, dz):
        x, rnn, out, att, lengths = self._saved
        if rnn.desc.impl == L.IMPL_LOCAL_LSTM:
            raise L.DepError("TextBiLSTM.backward: the last forward ran in eval() mode on config['eval_impl'] = 8, the exchange-free LSTM "
                             'forward, which saves no gates and has no backward; call train() and run the forward again')
        P = self._params
        dctx = self._head.backward(dz)
        dout, dh_n = L.attn_bwd(dctx, out, P['attention_layer.0.weight'].data, att, 2 * self.rnn_layers,
                                P['attention_layer.0.weight']._grad, P['attention_layer.0.bias']._grad, lengths=lengths)
        in_call, post = self.sync_plan()
        rnn.backward(x, self._rnn_w, self._rnn_g, dy=dout, dh_n=dh_n, dx=None, grad_sync=parallel.make_grad_sync(self, in_call),
                     lengths=lengths)
        self._grad_ready = True
        parallel.finish_grad_sync(self, in_call, post)


class FusionNet(nn.Module):
    """Frozen audio-GRU + text-BiLSTM encoders -> concat(text, audio) -> Linear(no bias) head.
    Only `fc_final.0.weight` trains (fuse_net_whole.py:590-593); the encoders run forward only.
    audio_bidirectional: the audio branch is the frozen encoder of the bidirectional AudioGRU -- [LayerNorm] -> BiGRU ->
    attention_net_with_w(output, h_n) -> fc_audio.1 -- with `lstm_net_audio.*_reverse` keys and the attention pair under
    `attention_layer_audio.0.*` (the reference's fusion class gives `attention_layer.0.*` to the text attention)."""

    def __init__(self, text_embed_size, text_hidden_dims, rnn_layers, dropout, num_classes, audio_hidden_dims,
                 audio_embed_size, variant='clf', seed=None, audio_bidirectional=False, text_impl=None):
        super().__init__()
        self.variant = variant
        # text_impl = 8: the frozen text BiLSTM on the exchange-free forward (same parameters, same state dict); None: the default plan
        self.text_impl = _local_lstm_choice(text_impl, 'FusionNet: text_impl', text_embed_size, text_hidden_dims, rnn_layers)
        self.audio_bidirectional = bi = bool(audio_bidirectional)
        if bi:          # the sweeps AudioGRU chooses for this width; a DepError by name where no bidirectional sweep runs it
            self._bi_impl = AudioGRU._bidirectional_impl(audio_embed_size, audio_hidden_dims, rnn_layers)
        self.text_embed_size = Ft = text_embed_size; self.audio_embed_size = Fa = audio_embed_size
        self.text_hidden_dims = Ht = text_hidden_dims; self.audio_hidden_dims = Ha = audio_hidden_dims
        self.rnn_layers = Lyr = rnn_layers; self.dropout = float(dropout); self.num_classes = num_classes
        gen = nn.make_generator(seed)
        init = {}

        def lin(nw, nb, o, i, live, bias=True):
            self._add(nw, (o, i), live=live)
            if bias:
                self._add(nb, (o,), live=live)
            init.update(nn.default_linear_init(nw, nb, o, i, gen, bias=bias))

        lin('attention_layer.0.weight', 'attention_layer.0.bias', Ht, Ht, False)
        rt = _rnn_names('lstm_net', Ft, Ht, Lyr, 2, 4)
        for n, s in rt:
            self._add(n, s, live=False)
        init.update(nn.default_rnn_init(rt, Ht, gen))
        lin('fc_out.1.weight', 'fc_out.1.bias', Ht, Ht, False)
        ra = _rnn_names('lstm_net_audio', Fa, Ha, Lyr, 2 if bi else 1, 3)
        for n, s in ra:
            self._add(n, s, live=False)
        init.update(nn.default_rnn_init(ra, Ha, gen))
        if bi:
            lin('attention_layer_audio.0.weight', 'attention_layer_audio.0.bias', Ha, Ha, False)
        lin('fc_audio.1.weight', 'fc_audio.1.bias', Ha, Ha, False)
        if variant == 'clf':
            self._add('ln.weight', (Fa,), live=False); self._add('ln.bias', (Fa,), live=False)
            init['ln.weight'] = np.ones(Fa, np.float32); init['ln.bias'] = np.zeros(Fa, np.float32)
        lin('modal_attn.weight', None, Ht + Ha, Ht + Ha, False, bias=False)
        lin('fc_final.0.weight', None, num_classes, Ht + Ha, True, bias=False)
        self._finalize(init)
        self._wt = [self._params[n].data for n, _ in rt]
        self._wa = [self._params[n].data for n, _ in ra]
        self._rnn_t = _RnnCache(L.CELL_LSTM, Ft, Ht, Lyr, 2, self.dropout, L.POOL_NONE, self.device, impl=self.text_impl)
        if bi:
            self._rnn_a = _RnnCache(L.CELL_GRU, Fa, Ha, Lyr, 2, self.dropout, L.POOL_NONE, self.device, impl=self._bi_impl)
        else:
            self._rnn_a = _RnnCache(L.CELL_GRU, Fa, Ha, Lyr, 1, self.dropout, L.POOL_SUM, self.device)
        self.fc_final = [self._params['fc_final.0.weight']]       # `model.fc_final[0].weight`-style access
        self._params['fc_final.0.weight'].weight = self._params['fc_final.0.weight']

    def check_health(self):
        self._rnn_t.check(); self._rnn_a.check()

    def status_words(self):
        return [w for w in (self._rnn_t.status_word(), self._rnn_a.status_word()) if w is not None]

    def fallback_words(self):
        return [w for w in (self._rnn_a.fallback_word(),) if w is not None]

    def _split(self, x):
        """Accept the reference's list of (audio_i, text_i) pairs or an (audio, text) pair of arrays."""
        if isinstance(x, (tuple, list)) and len(x) == 2 and hasattr(x[0], 'shape') and len(x[0].shape) == 3:
            return self._to_dev(x[0]), self._to_dev(x[1])
        xa = np.stack([np.asarray(e[0]) for e in x]); xt = np.stack([np.asarray(e[1]) for e in x])
        return self._to_dev(xa), self._to_dev(xt)

    def pretrained_feature(self, x, lengths=None):
        """fusion_net.pretrained_feature (fuse_net_whole.py:336-366): no gradients; Dropout stays active in
        train() mode exactly as in the reference.
        lengths: (audio_lengths, text_lengths) of a ragged batch -- each None or B integers (a host sequence or an int32 device
        vector): x is padded (_common.pad_ragged), row b of a modality is its own lengths[b] steps long.  The reverse sweeps start
        at a row's last step, both attentions and the unidirectional audio pool run over its own steps; a row of length 0 has
        context / pool 0, and the head is applied to that zero vector."""
        xa, xt = self._split(x)
        if lengths is None:
            la = lt = None
        else:
            if not isinstance(lengths, (tuple, list)) or len(lengths) != 2:
                raise L.DepError('pretrained_feature: lengths is the pair (audio_lengths, text_lengths), each None or B integers')
            la = _RnnCache.lengths_on(lengths[0], xa.shape[0], self.device)
            lt = _RnnCache.lengths_on(lengths[1], xt.shape[0], self.device)
        training = self.training
        seed = nn.next_dropout_seed() if training else 0
        p = self.dropout if training else 0.0
        P = self._params
        B, T, _ = xt.shape
        # frozen encoders: dropout drawn as in training, but no backward follows -- the dropout-only run mode keeps no saved gates
        mode = L.RUN_DROPOUT_ONLY if training else L.RUN_EVAL
        # text encoder
        rnn = self._rnn_t.get(B, T, mode)
        h_n = torch.empty(2 * self.rnn_layers, B, self.text_hidden_dims, dtype=torch.float32, device=self.device)
        rnn.forward(xt, self._wt, seed=seed, h_n=h_n, lengths=lt)
        ctx, _ = L.attn_fwd(rnn.layer_output(), h_n, P['attention_layer.0.weight'].data, P['attention_layer.0.bias'].data, lengths=lt)
        tf = _mlp_feature(ctx, P['fc_out.1.weight'].data, P['fc_out.1.bias'].data, p, seed, (L.SITE_FC0, L.SITE_FC1))
        # audio encoder
        Ba, Ta, Fa = xa.shape
        if self.variant == 'clf':
            xn, _ = L.layernorm_fwd(xa.view(Ba * Ta, Fa), P['ln.weight'].data, P['ln.bias'].data, save=False)
        else:
            xn = xa.view(Ba * Ta, Fa)
        rna = self._rnn_a.get(Ba, Ta, mode)
        if self.audio_bidirectional:
            # nothing trains, so no LayerNorm fold: the affine above and the raw weights; the top sequence is read in place
            h_na = torch.empty(2 * self.rnn_layers, Ba, self.audio_hidden_dims, dtype=torch.float32, device=self.device)
            rna.forward(xn, self._wa, seed=seed + 1, h_n=h_na, lengths=la)
            pooled, _ = L.attn_fwd(rna.layer_output(), h_na, P['attention_layer_audio.0.weight'].data,
                                   P['attention_layer_audio.0.bias'].data, lengths=la)
        else:
            pooled = torch.empty(Ba, self.audio_hidden_dims, dtype=torch.float32, device=self.device)
            rna.forward(xn, self._wa, seed=seed + 1, pooled=pooled, lengths=la)
        af = _mlp_feature(pooled, P['fc_audio.1.weight'].data, P['fc_audio.1.bias'].data, p, seed, (L.SITE_FC2, L.SITE_FC3))
        return tf, af

    def forward(self, x):
        """x: concat(text_feature, audio_feature) (B, Ht+Ha) -> probabilities / score."""
        x = x.data if isinstance(x, nn.Output) else x
        x = x.contiguous()
        P = self._params
        W = P['fc_final.0.weight'].data
        B = x.shape[0]
        if self.variant == 'clf':
            z = L.linear_fwd(x, W, None)
            out = torch.empty_like(z)
            L.head_loss(L.LOSS_CE_LOGITS, z, None, out, None, None, 1.0)      # Softmax(dim=1)
        else:
            g = L.linear_fwd(x, P['modal_attn.weight'].data, None)
            gx = torch.empty_like(x); L.sigmoid_gate(g, x, gx)
            z = L.linear_fwd(gx, W, None)
            out = torch.empty_like(z)
            L.head_loss(L.LOSS_L1_RELU, z, None, out, None, None, 1.0)        # ReLU
        return nn.Output(out, None, z)


class MyLoss:
    """Split-weight loss (fuse_net_whole.py:376-395 ; Regression/fuse_net.py:353-366):
    loss(text_feature W[:, :Ht]^T, y) + loss(audio_feature W[:, Ht:]^T, y), gradient to W only.
    The classification variant takes torch.nn.CrossEntropyLoss's weight / ignore_index / label_smoothing (nn.CEOptions): both halves
    then run dep_head_loss_ce over ONE shared denominator.  The regression variant takes `loss` ('l1', 'smooth_l1', 'huber', 'mse'),
    `beta`, `delta` (nn.RegOptions) and, on its call, `weight`: B row weights; both plain halves (no ReLU) then run dep_head_loss_reg
    over ONE shared denominator C sum_i w_i.  All defaults and no weight: the launches it always enqueued.  The target, the
    denominator and the launches are nn.criterion_call's, on both halves at once; its own are the GEMMs around them."""
    kind = L.LOSS_CE_LOGITS                     # what nn.criterion_call reads: the halves are logits / plain outputs (no ReLU)
    relu = 0

    def __init__(self, variant='clf', weight=None, ignore_index=-100, label_smoothing=0.0, reduction='mean', loss='smooth_l1',
                 beta=1.0, delta=1.0):
        self.variant = variant
        self.target_dtype = 'int' if variant == 'clf' else 'float'
        self.options = nn.CEOptions(weight, ignore_index, label_smoothing, reduction)
        if variant != 'clf' and self.options.active:
            raise ValueError('class weights, ignore_index and label_smoothing belong to the classification loss')
        self.reg_options = nn.RegOptions(loss, beta, delta, reduction)
        if variant == 'clf' and (loss, float(beta), float(delta)) != ('smooth_l1', 1.0, 1.0):
            raise ValueError('loss, beta and delta belong to the regression loss')

    def __call__(self, text_feature, audio_feature, target, model, weight=None):
        if self.variant == 'clf' and weight is not None:
            raise ValueError('row weights belong to the regression loss (the classification loss takes class weights)')
        Wp = model._params['fc_final.0.weight']
        W = Wp.data
        Cc, D = W.shape
        Ht = text_feature.shape[1]; Ha = audio_feature.shape[1]
        B = text_feature.shape[0]
        dev = W.device
        train = model.training and Wp.requires_grad
        zt = torch.empty(B, Cc, dtype=torch.float32, device=dev); za = torch.empty_like(zt)
        L.gemm(0, 1, B, Cc, Ht, text_feature, Ht, W, D, zt, Cc)
        L.gemm(0, 1, B, Cc, Ha, audio_feature, Ha, W[:, Ht:], D, za, Cc)

        def bw(dzt, dza):
            g = Wp._grad
            L.gemm(1, 0, Cc, Ht, B, dzt, Cc, text_feature, Ht, g, D)               # dW[:, :Ht] = dzt^T text
            L.gemm(1, 0, Cc, Ha, B, dza, Cc, audio_feature, Ha, g[:, Ht:], D)      # dW[:, Ht:] = dza^T audio
            model._grad_ready = True
            parallel.finish_grad_sync(model, *model.sync_plan())
        loss, dzs = nn.criterion_call(self, (zt, za), target, weight, model, train, bw)
        loss.dz_halves = tuple(dzs)             # dLoss/dz of the text and the audio half (None under evaluate())
        return loss
