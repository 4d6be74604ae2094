"""Host-side module / loss / optimizer layer over libdep_rnn.so.

This is the part of torch.nn / torch.optim / autograd the reference scripts lean on, restated so
that their `model(x)`, `criterion(output, y)`, `loss.backward()`, `optimizer.step()`,
`state_dict()` / `load_state_dict(strict=False)` / `named_parameters()` call surface keeps working
while every FLOP runs in the HIP library.  No torch.nn layer, no autograd: each Module owns

  * one flat fp32 parameter buffer and one flat gradient buffer on the GPU (Parameters are views),
    laid out [live + no-decay ('ln') | live + weight-decay | dead] so that Adam/AdamW is at most
    two kernel launches and the data-parallel gradient all-reduce is ONE contiguous bucket;
  * an explicit backward() that the Loss object returned by a criterion triggers.

"Dead" parameters are the ones the reference defines but never uses in forward() (SURVEY 2.1
quirk 1): they exist in state_dict(), never receive a gradient (`.grad is None`) and are skipped
by the optimizers exactly like torch skips parameters whose grad is None.
"""
from __future__ import annotations

import contextlib
import math
from collections import OrderedDict

import numpy as np
import torch

from . import _lib as L
from . import parallel


def _device():
    if not torch.cuda.is_available():
        raise L.DepError('no MI355X visible (torch.cuda.is_available() is False): the HIP path has no CPU fallback')
    L.load()
    return torch.device('cuda', torch.cuda.current_device())


class Parameter:
    """A named view into the owning module's flat buffers."""

    def __init__(self, name, shape, owner):
        self.name = name
        self.shape = tuple(shape)
        self.numel = int(np.prod(shape))
        self.owner = owner
        self.offset = -1
        self.live = True             # receives a gradient in backward()
        self.requires_grad = True
        self.data = None             # torch view, set by Module._finalize
        self._grad = None

    @property
    def grad(self):
        if not self.live or not self.requires_grad or not self.owner._grad_ready:
            return None
        return self._grad

    def __repr__(self):
        return f'Parameter({self.name}, shape={self.shape}, live={self.live})'


class Module:
    def __init__(self):
        self._params = OrderedDict()
        self.training = True
        self._grad_ready = False
        self._flat = None
        self._flat_grad = None

    def check_health(self):
        """Raise if a kernel of the last step reported trouble (the recurrent cluster sweeps bound their in-launch
        waits and raise a status word instead of hanging).  Called from Loss.item(), i.e. at the host sync the training
        loops already have; models that own recurrent stacks override it."""

    # -- construction ------------------------------------------------------------------
    def _add(self, name, shape, live=True):
        p = Parameter(name, shape, self)
        p.live = live
        self._params[name] = p
        return p

    def _finalize(self, init_values):
        """Lay the parameters out in the flat buffers and upload `init_values` (name -> ndarray)."""
        dev = _device()
        # [live no-decay ('ln') | live weight-decay | dead]: each optimizer group stays one contiguous range, and the audio
        # classifier's LayerNorm pair sits next to GRU layer 0 -- the two gradient ranges that become final together (after
        # dep_ln_fold_bwd) are ONE contiguous all-reduce (round 4; VERDICT r3 item 6: two collectives per step, not three)
        order = ([p for p in self._params.values() if p.live and 'ln' in p.name] +
                 [p for p in self._params.values() if p.live and 'ln' not in p.name] +
                 [p for p in self._params.values() if not p.live])
        off = 0
        for p in order:
            p.offset = off
            off += (p.numel + 3) // 4 * 4            # keep every tensor 16-byte aligned
        # The alignment pads between tensors are LOAD-BEARING zeros in _flat_grad: the optimizer's ranges run over them, so the global
        # gradient norm of a clipped step (dep_grad_sqnorm) sums them too.  The buffer is allocated zeroed below and every kernel writes
        # gradients through the per-tensor views only (tests/test_clip_gpu.py holds the pads at exactly zero after a step).
        self._n_live = sum((p.numel + 3) // 4 * 4 for p in order if p.live)
        host = np.zeros(off, np.float32)
        for p in order:
            host[p.offset:p.offset + p.numel] = np.asarray(init_values[p.name], np.float32).reshape(-1)
        self._flat = torch.from_numpy(host).to(dev)
        self._flat_grad = torch.zeros(max(self._n_live, 4), dtype=torch.float32, device=dev)
        for p in order:
            p.data = self._flat[p.offset:p.offset + p.numel].view(p.shape)
            p._grad = self._flat_grad[p.offset:p.offset + p.numel].view(p.shape) if p.live else None
        self.device = dev

    # -- torch.nn.Module surface ----------------------------------------------------------
    def named_parameters(self):
        return iter(self._params.items())

    def parameters(self):
        return iter(self._params.values())

    def state_dict(self):
        return OrderedDict((k, p.data) for k, p in self._params.items())

    def load_state_dict(self, sd, strict=True):
        """Name-based load.  strict=False ignores missing/unexpected keys like torch does
        (Classification/fuse_net_whole.py:586-588 relies on this)."""
        missing = [k for k in self._params if k not in sd]
        unexpected = [k for k in sd if k not in self._params]
        if strict and (missing or unexpected):
            raise RuntimeError(f'load_state_dict: missing {missing}, unexpected {unexpected}')
        for k, v in sd.items():
            if k in self._params:
                p = self._params[k]
                t = v if torch.is_tensor(v) else torch.as_tensor(np.asarray(v))
                if tuple(t.shape) != p.shape:
                    raise RuntimeError(f'size mismatch for {k}: {tuple(t.shape)} vs {p.shape}')
                p.data.copy_(t.to(dtype=torch.float32))
        return missing, unexpected

    def train(self, mode=True):
        self.training = bool(mode)
        return self

    def eval(self):
        return self.train(False)

    def zero_grad(self):
        self._grad_ready = False

    def __call__(self, *a, **k):
        return self.forward(*a, **k)

    def cuda(self):
        return self

    # -- helpers -------------------------------------------------------------------------
    def _span(self, first, last):
        """(start, count) of the contiguous run of live parameters from `first` to `last` in the flat gradient buffer."""
        a, b = self._params[first], self._params[last]
        start, end = a.offset, b.offset + (b.numel + 3) // 4 * 4
        if not (a.live and b.live and 0 <= start < end <= self._n_live):
            raise RuntimeError(f'gradient span {first}..{last} is not inside the live bucket')
        return start, end - start

    def sync_plan(self):
        """({layer: (start, count)} reduced inside dep_rnn_backward_overlapped, [(start, count), ...] reduced after the
        backward).  Default: the whole live bucket after the backward."""
        return {}, [(0, self._n_live)]

    def live_grad_bucket(self):
        """The single contiguous gradient bucket the data-parallel all-reduce operates on."""
        return self._flat_grad[:self._n_live]

    def _to_dev(self, x):
        if torch.is_tensor(x):
            t = x
        else:
            t = torch.from_numpy(np.ascontiguousarray(x))
        return t.to(device=self.device, dtype=torch.float32).contiguous()


class Output:
    """What `model(x)` returns: the result tensor plus the owner that can run backward for it.
    `.data` is the plain device tensor (the reference reads `output.data.max(1, keepdim=True)[1]`)."""

    def __init__(self, data, owner=None, z=None):
        self.data = data
        self._owner = owner
        self._z = z              # pre-activation the fused loss kernel starts from

    @property
    def shape(self):
        return self.data.shape

    def cpu(self):
        return self.data.cpu()

    def detach(self):
        return self.data

    def flatten(self):
        return self.data.flatten()

    def numpy(self):
        return self.data.cpu().numpy()

    def max(self, *a, **k):
        return self.data.max(*a, **k)


class Loss:
    def __init__(self, value_dev, backward_fn, reduce=False, health=None, dz=None):
        self._v = value_dev
        self.dz = dz                        # dLoss/dz (B, C) the backward starts from (the tensor `backward_fn` reads), or None
        self._bw = backward_fn
        self._reduce = reduce               # data parallel: the local part of a global batch mean
        self._health = health               # model.check_health: the host sync below is where a failed sweep surfaces

    def item(self):
        """Host sync point, as in the reference (loss.item()).  Under data parallelism every rank calls it
        (train() does) and the per-rank parts are summed here, lazily, off the critical path."""
        if self._reduce:
            parallel.all_reduce_sum(self._v)
            self._reduce = False
        v = float(self._v.item())
        if self._health is not None:
            self._health()
        return v

    def backward(self):
        if self._bw is None:
            raise RuntimeError('loss computed under evaluate(): nothing to backpropagate')
        L.order_note('backward begin')
        self._bw()
        L.order_note('backward end')

    def __float__(self):
        return self.item()


class LossSum:
    """`total_loss += loss.item()` of the reference's loops (audio_gru_whole.py:195) without a host synchronisation per
    mini-batch: the step losses are added on the device in float64 and read ONCE with item().  On one rank that is exactly what
    Python's float accumulation of the fp32 `loss.item()` values computes, in the same order; under data parallelism the
    per-rank float64 partial sums are added by ONE all-reduce in item() (every rank calls it), which can differ in the last bits
    from all-reducing every step loss first.  The sweeps' status word and the fused forward's fallback word are folded into two
    device flags by the same launch (dep_loss_accumulate: one kernel per step and model stack), and they travel with the sum
    in that all-reduce: a sweep that gave up on ANY rank raises on EVERY rank, at item() -- no rank goes on to the next
    collective alone -- and every rank switches the exclusive forward off together."""

    def __init__(self, device):
        self._acc = torch.zeros(3, dtype=torch.float64, device=device)       # [loss sum, max status word, max fallback word]
        self._reduce = False
        self._value = None                                # result of the last item(), valid until the next add()

    def add(self, loss, model=None):
        self._value = None
        v = loss._v.reshape(-1)
        self._reduce = self._reduce or loss._reduce
        loss._reduce = False                              # summed here, once
        sw = list(model.status_words()) if model is not None and hasattr(model, 'status_words') else []
        fw = list(model.fallback_words()) if model is not None and hasattr(model, 'fallback_words') else []
        if not v.is_cuda:                                 # host tensors: only the CPU stand-in model of tests/test_host_cpu.py
            self._acc[0] += v[0].double()
            for w in sw:
                self._acc[1] = torch.maximum(self._acc[1], w.double())
            for w in fw:
                self._acc[2] = torch.maximum(self._acc[2], w.double())
            return self
        n = max(1, len(sw), len(fw))
        for i in range(n):                                # one launch per recurrent stack of the model (fusion: two)
            L.loss_accumulate(v if i == 0 else None, sw[i] if i < len(sw) else None, fw[i] if i < len(fw) else None, self._acc)
        return self

    def item(self):
        """EVERY rank must call item() at the same point of its loop (it is a collective whenever world_size > 1 -- the flags travel
        even when the loss itself is already global); a rank-0-only call would wait for the others for ever.  The
        accumulator is cleared: a second item() without an add() in between returns the same value again WITHOUT a collective, and a
        LossSum reused for the next epoch starts from zero."""
        if self._value is not None:
            return self._value
        acc = self._acc
        if parallel.world_size() > 1:
            t = acc.clone()
            if not self._reduce:
                t[0] = 0.0                                # a loss that is already global: only the flags are shared
            parallel.all_reduce_sum(t)                    # flags: a sum of non-negative words is non-zero iff one of them is
            acc = t if self._reduce else torch.stack((acc[0], t[1], t[2]))
            self._reduce = False
        v, bad, fell = (float(x) for x in acc.tolist())
        self._acc.zero_()
        if fell != 0:
            L.note_fallback()                             # right results, but stop paying the hello time-out (every rank together)
        if bad != 0:
            # (under data parallelism `bad` is the SUM of the ranks' status words: non-zero iff a sweep gave up on some rank, not a code)
            raise L.DepError('a recurrent sweep gave up waiting for a cluster member during this epoch (status words summed over %d rank(s): %d): '
                             'the GPU was shared with another kernel; DEP_FUSED2=0 DEP_CLUSTER16=0 selects the sweeps that tolerate it'
                             % (parallel.world_size(), int(bad)))
        self._value = v
        return v


def _check_labels(t, num_classes, ignore_index=None):
    """torch's CrossEntropyLoss raises on a class index outside [0, C); the loss kernel indexes with the label, so the
    range is validated here, on the host copy the training loops hand over (device-resident labels are the caller's).
    ignore_index: labels equal to it are exempt (a criterion that ignores rows)."""
    if not t.is_cuda and t.numel() > 0:
        if ignore_index is not None:
            t = t[t != ignore_index]
            if t.numel() == 0:
                return
        lo, hi = int(t.min()), int(t.max())
        if lo < 0 or hi >= num_classes:
            raise IndexError(f'Target {lo if lo < 0 else hi} is out of bounds for {num_classes} classes')


class CEOptions:
    """torch.nn.CrossEntropyLoss's `weight`, `ignore_index` and `label_smoothing` (reduction 'mean') for the fused CE criteria
    (CrossEntropyLoss below, models.MyLoss): validation and the values, with the device copy of the weights -- uploaded once, here.
    What a call does with them is criterion_call's."""

    def __init__(self, weight=None, ignore_index=-100, label_smoothing=0.0, reduction='mean'):
        if reduction != 'mean':
            raise ValueError(f"only reduction='mean' is implemented, got {reduction!r}")
        eps = float(label_smoothing)
        if not 0.0 <= eps < 1.0:
            raise ValueError(f'label_smoothing must be in [0, 1), got {label_smoothing!r}')
        if isinstance(ignore_index, bool) or not isinstance(ignore_index, (int, np.integer)):
            raise ValueError(f'ignore_index must be an integer, got {ignore_index!r}')
        self.label_smoothing = eps
        self.ignore_index = int(ignore_index)
        self.weight = None                  # host float64 copy (what row weights and host denominators are made from)
        self.weight_dev = None
        if weight is not None:
            w = np.asarray(weight.detach().cpu().numpy() if torch.is_tensor(weight) else weight, dtype=np.float64).reshape(-1)
            if w.size == 0 or not np.all(np.isfinite(w)) or np.any(w < 0):
                raise ValueError('weight must be a non-empty vector of finite, non-negative class weights')
            self.weight = w
            self.weight_dev = torch.from_numpy(w.astype(np.float32)).to(_device())
        self.active = self.weight is not None or eps != 0.0 or self.ignore_index != -100

    def row_weight(self, targets):
        """Host vector for _common.train_epoch(row_weight=): w[y_i] per row, 0 for an ignored one."""
        from ._common import class_row_weight
        t = np.asarray(targets.cpu().numpy() if torch.is_tensor(targets) else targets).reshape(-1)
        w = self.weight
        if w is None:
            live = t[t != self.ignore_index]
            w = np.ones(int(live.max()) + 1 if live.size else 1)
        return class_row_weight(t, w, self.ignore_index)


class RegOptions:
    """The regression criteria's form and parameter (dep_head_loss_reg: L1, SmoothL1(beta), Huber(delta), MSE; reduction 'mean') and
    per-row sample weights (L1Loss / SmoothL1Loss / HuberLoss / MSELoss below, models.MyLoss('reg')): validation, the values, and the
    weights' way to the device.  What a call does with them is criterion_call's."""
    FORMS = {'l1': L.REG_L1, 'smooth_l1': L.REG_SMOOTHL1, 'huber': L.REG_HUBER, 'mse': L.REG_MSE}

    def __init__(self, loss='smooth_l1', beta=1.0, delta=1.0, reduction='mean'):
        if reduction != 'mean':
            raise ValueError(f"only reduction='mean' is implemented, got {reduction!r}")
        if loss not in self.FORMS:
            raise ValueError(f"loss must be one of {sorted(self.FORMS)}, got {loss!r}")
        beta, delta = float(beta), float(delta)
        if loss == 'smooth_l1' and not beta >= 0.0:
            raise ValueError(f'SmoothL1Loss: beta must be non-negative, got {beta!r}')
        if loss == 'huber' and not delta > 0.0:
            raise ValueError(f'HuberLoss: delta must be positive, got {delta!r}')
        if not np.isfinite(beta if loss == 'smooth_l1' else delta if loss == 'huber' else 0.0):
            raise ValueError(f'{loss}: the parameter must be finite')
        self.loss = loss
        self.form = self.FORMS[loss]
        self.param = beta if loss == 'smooth_l1' else delta if loss == 'huber' else 0.0
        # the forms dep_head_loss itself computes: without row weights they keep its launches
        self.neutral = loss == 'l1' or (loss == 'smooth_l1' and beta == 1.0)

    @staticmethod
    def rows(weight, B, dev):
        """(device weights, host float64 copy or None) of a criterion call's `weight`: B non-negative finite floats as a sequence, an
        array or a tensor.  A host-side vector is validated here; a device tensor is the caller's responsibility."""
        if weight is None:
            return None, None
        if torch.is_tensor(weight) and weight.is_cuda:
            w = weight.reshape(-1)
            if w.numel() != B:
                raise ValueError(f'weight has {w.numel()} entries for {B} rows')
            return w.to(device=dev, dtype=torch.float32).contiguous(), None
        w = np.asarray(weight.detach().numpy() if torch.is_tensor(weight) else weight, dtype=np.float64).reshape(-1)
        if w.size != B:
            raise ValueError(f'weight has {w.size} entries for {B} rows')
        if not np.all(np.isfinite(w)) or np.any(w < 0):
            raise ValueError('weight must hold finite, non-negative row weights')
        return torch.from_numpy(w.astype(np.float32)).to(dev), w


# ----------------------------------------------------------------------------- the criteria's one call path
# A criterion is a declaration: target_dtype ('int': class labels, anything else: values), kind (its dep_head_loss kind), options
# (CEOptions or None), reg_options (RegOptions or None) and relu.  criterion_call is what every one of them does with a target.
_PLAIN_REG = {('l1', 1): L.LOSS_L1_RELU, ('smooth_l1', 1): L.LOSS_SMOOTHL1_RELU, ('smooth_l1', 0): L.LOSS_SMOOTHL1}


def _plain_kind(crit, weight):
    """The choice of the entry point: the dep_head_loss kind of a call with everything at its defaults -- the launches it always
    enqueued -- or None for dep_head_loss_ce (class labels) / dep_head_loss_reg (values).
        class labels, no option active                                               crit.kind
        values without reg_options (a bare _HeadLoss subclass)                       crit.kind
        values without `weight`: L1 or SmoothL1 with beta 1 on relu(z), SmoothL1 with beta 1 on z      _PLAIN_REG
    Everything else, L1 on z among it, has no plain kind."""
    if crit.target_dtype == 'int':
        return None if crit.options is not None and crit.options.active else crit.kind
    reg = crit.reg_options
    if reg is None:
        return crit.kind
    return _PLAIN_REG.get((reg.loss, crit.relu)) if weight is None and reg.neutral else None


def _label_target(target, num_classes, dev, ignore_index):
    """(device labels, LOSS_LABELS_I64 or 0, host labels or None) of a sequence, an ndarray or a tensor of class indices.  The range is
    checked on the host copy (ignore_index exempt); torch.long, as the reference's loops make them, is read in place."""
    t = torch.as_tensor(np.asarray(target) if not torch.is_tensor(target) else target).reshape(-1)
    _check_labels(t, num_classes, ignore_index)
    host = None if t.is_cuda else t
    if t.dtype == torch.int64:
        return t.to(device=dev).contiguous(), L.LOSS_LABELS_I64, host
    return t.to(device=dev, dtype=torch.int32).contiguous(), 0, host


def _denominator(train, B, Cc, labels, plain, opt, t_dev, t_host, w_dev, w_host):
    """What the loss and dz of a criterion call are divided by.
    Unweighted call (`plain`: the dep_head_loss kinds): parallel.loss_count(B, per_row) while training -- the rows of the global /
    accumulated batch -- else B * per_row; per_row is 1 for class labels and C for the regression means.
    Weighted call (CE with any option active, label smoothing or ignore_index alone among them; a regression call with `weight`), with
    scale 1 for CE and C for regression: while training a declared parallel.loss_weight() times scale; else, on more than one rank, a
    DepError; else the batch's own sum -- from a host copy a number summed in float64 and rounded to float32, or, when that is not
    positive, a 1-element device tensor holding it (NaN, as in torch: the host `norm` must be > 0); from device-resident labels or
    weights one dep_ce_weight_sum / dep_row_weight_sum launch into a device scalar (one launch more, no host read).  evaluate()
    (train False) always takes the batch's own.
    Quirk, kept: a regression form without a plain kind (MSELoss, say) called WITHOUT `weight` still consults parallel.loss_weight()
    first while training and only then falls back to the unweighted count; on more than one rank it is not refused."""
    per_row = scale = 1 if labels else Cc
    weighted = not plain and (labels or w_dev is not None)
    if train and not plain:
        w = parallel.loss_weight()
        if w is not None:
            return w * scale
        if weighted and parallel.world_size() > 1:
            raise L.DepError(f"a criterion with {'class weights / label smoothing / ignore_index' if labels else 'row weights'} under data "
                             "parallelism needs the global mini-batch's denominator: declare it with parallel.set_global_weight (or pass "
                             'row_weight= to _common.train_epoch)')
    if not weighted:
        return parallel.loss_count(B, per_row) if train else B * per_row
    dev = t_dev.device if labels else w_dev.device
    if labels and t_host is not None:
        y = t_host.numpy().astype(np.int64)
        live = y != opt.ignore_index
        den = live.sum() if opt.weight is None else opt.weight[y[live]].sum()
    elif w_host is not None:
        den = Cc * w_host.sum()
    else:
        den = torch.empty(1, dtype=torch.float32, device=dev)
        if labels:
            L.ce_weight_sum(t_dev, opt.weight_dev, opt.ignore_index, Cc, den)
        else:
            L.row_weight_sum(w_dev, Cc, den)
        return den
    den = float(np.float32(den))
    return den if den > 0.0 else torch.full((1,), den, dtype=torch.float32, device=dev)


def criterion_call(crit, zs, target, weight, owner, train, backward):
    """One criterion call on the pre-activations `zs` -- one (B, C) tensor, or the fusion loss's two halves -- which share the target,
    the denominator, `rows` and the value: bring the target (and the row weights) to the device, choose the denominator and the entry
    point, then per z one head-loss launch and one reduce (accumulating after the first).  Returns (Loss, [dLoss/dz per z]); the
    Loss runs backward(*dzs) when `train`."""
    B, Cc = zs[0].shape
    dev = zs[0].device
    labels = crit.target_dtype == 'int'
    plain = _plain_kind(crit, weight)
    opt = reg = t_host = w_dev = w_host = None
    if labels:
        if plain is None:
            opt = crit.options
            if opt.weight is not None and opt.weight.size != Cc:
                raise ValueError(f'weight has {opt.weight.size} entries, the model has {Cc} classes')
        t, wide, t_host = _label_target(target, Cc, dev, None if opt is None else opt.ignore_index)
    else:
        t = torch.as_tensor(np.asarray(target) if not torch.is_tensor(target) else target)
        t = t.to(device=dev, dtype=torch.float32).contiguous().view(B, Cc)
        wide = 0
        if plain is None:
            reg = crit.reg_options
            w_dev, w_host = reg.rows(weight, B, dev)
    norm = _denominator(train, B, Cc, labels, plain is not None, opt, t, t_host, w_dev, w_host)
    rows = torch.empty(B, dtype=torch.float32, device=dev)
    val = torch.empty(1, dtype=torch.float32, device=dev)             # the first reduce overwrites it
    dzs = []
    for z in zs:
        dz = torch.empty_like(z) if train else None
        if plain is not None:
            L.head_loss(plain | wide, z, t, None, rows, dz, norm)
        elif labels:
            L.head_loss_ce(crit.kind | wide, z, t, None, rows, dz, norm, opt.weight_dev, opt.label_smoothing, opt.ignore_index)
        else:
            L.head_loss_reg(reg.form, crit.relu, reg.param, z, t, None, rows, dz, norm, w_dev)
        L.reduce_loss(rows, norm, val, bool(dzs))                     # every z after the first adds to the value
        dzs.append(dz)
    # data parallel: every rank normalised by the GLOBAL batch, so the value is the local part of the global mean (Loss.item sums them)
    loss = Loss(val, (lambda: backward(*dzs)) if train else None, reduce=train and parallel.world_size() > 1,
                health=getattr(owner, 'check_health', None), dz=dzs[0] if len(zs) == 1 else None)
    return loss, dzs


class _HeadLoss:
    """Loss on a model output; the output nonlinearity, the loss and dLoss/dz are one HIP kernel (criterion_call)."""
    kind = None
    target_dtype = None
    options = None
    reg_options = None
    relu = 1

    def __call__(self, output, target):
        return self._on(output, target, None)

    def _on(self, output, target, weight):
        owner = output._owner
        return criterion_call(self, (output._z,), target, weight, owner, owner is not None and owner.training,
                              lambda dz: owner.backward(dz))[0]


class CrossEntropyLoss(_HeadLoss):
    """nn.CrossEntropyLoss on the model's Softmax output (audio_gru_whole.py:308), with torch's `weight`, `ignore_index` and
    `label_smoothing` (reduction 'mean').  All defaults: dep_head_loss + dep_reduce_loss, the launches it always enqueued, and a label
    -100 is out of range as it always was.  Any option set: dep_head_loss_ce, divided by sum_i live_i w[y_i] (_denominator); rows
    whose label is ignore_index then count for nothing."""
    kind = L.LOSS_CE_ON_SOFTMAX
    target_dtype = 'int'

    def __init__(self, weight=None, ignore_index=-100, label_smoothing=0.0, reduction='mean'):
        self.options = CEOptions(weight, ignore_index, label_smoothing, reduction)


class _RegLoss(_HeadLoss):
    """A regression criterion on the model's ReLU output: criterion(output, target, weight=None), the weighted mean over elements
    sum_i w_i sum_c l_ic / (C sum_i w_i) (all weights 1: torch's mean).  A row of weight 0 is an ignored row.  The forms
    dep_head_loss computes (L1, SmoothL1 with beta 1) called without `weight` are dep_head_loss + dep_reduce_loss, the launches they
    always enqueued; everything else is dep_head_loss_reg + dep_reduce_loss (_plain_kind)."""
    target_dtype = 'float'

    def __call__(self, output, target, weight=None):
        return self._on(output, target, weight)


class L1Loss(_RegLoss):
    """nn.L1Loss on the ReLU output (Regression/audio_bilstm_perm.py:251)."""

    def __init__(self, reduction='mean'):
        self.reg_options = RegOptions('l1', reduction=reduction)


class SmoothL1Loss(_RegLoss):
    """nn.SmoothL1Loss(beta) on the ReLU output (Regression/text_bilstm_perm.py:247); beta = 0 is L1, as in torch."""

    def __init__(self, beta=1.0, reduction='mean'):
        self.reg_options = RegOptions('smooth_l1', beta=beta, reduction=reduction)


class HuberLoss(_RegLoss):
    """nn.HuberLoss(delta) on the ReLU output."""

    def __init__(self, delta=1.0, reduction='mean'):
        self.reg_options = RegOptions('huber', delta=delta, reduction=reduction)


class MSELoss(_RegLoss):
    """nn.MSELoss on the ReLU output."""

    def __init__(self, reduction='mean'):
        self.reg_options = RegOptions('mse', reduction=reduction)


def empty_shard_step(model, optimizer):
    """Data parallel, global mini-batch smaller than the world size: this rank owns no row of it.  It still joins every
    collective of the step with a zero contribution (gradient ranges in the same order as the working ranks, the lazy loss
    reduce in Loss.item) and applies the same optimizer update, so the replicas stay identical and nobody hangs."""
    optimizer.zero_grad()
    model.live_grad_bucket().zero_()
    model._grad_ready = True
    in_call, post = model.sync_plan()
    parallel.reduce_zero_contribution(model, in_call, post)
    optimizer.step()
    val = torch.zeros(1, dtype=torch.float32, device=model.device)
    return Loss(val, None, reduce=parallel.world_size() > 1)


# ----------------------------------------------------------------------------- optimizers
class _AdamBase:
    decoupled = False

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=None, max_grad_norm=None, skip_nonfinite=False,
                 accumulate_steps=1, amsgrad=False, ema_decay=None, max_grad_value=None, clip_per_group=False, count_skipped=True):
        """max_grad_norm: clip the GLOBAL 2-norm of the gradients of all groups to it inside the update (torch's
        clip_grad_norm_(all parameters, max_grad_norm) in front of step(), without its host read; None = no clipping).
        skip_nonfinite: a step whose gradient norm is inf / NaN leaves parameters and moments untouched (it still counts in the bias
        correction).  With both at their defaults step() enqueues exactly the dep_adam_step launches it always did.
        accumulate_steps: K > 1 makes step() a MICRO-step: it adds the gradients the last backward wrote into a flat accumulator
        per owner module (one dep_grad_accumulate launch over the ranges of all groups) and only every K-th call -- or flush() --
        updates, from the accumulator; clipping and skip_nonfinite then act on the accumulated gradient.  The criteria must divide
        by the rows of the whole accumulated batch (parallel.set_accumulated_count), not by their own.  1: step() is what it was.
        amsgrad: torch's option -- the running maximum of v takes v's place under the root.
        ema_decay: d in [0, 1) keeps an average of the parameters, avg += (1 - d) * (p - avg) after every update (torch's
        AveragedModel with get_ema_multi_avg_fn(d): no bias correction, the first update copies), in one flat buffer per owner module
        laid out like its parameters; averaged() puts it in the parameters' place.  Either option makes every range's launch a
        dep_adam_step_ext -- the same number of launches; with both at their defaults the launches are the ones above.
        max_grad_value: c > 0 clamps every element of g * coef to [-c, c] inside the update launch (torch's clip_grad_value_ between
        clip_grad_norm_ and step(); a NaN stays NaN); on its own it adds no launch and measures no norm.
        clip_per_group: every param group is clipped against the 2-norm of ITS gradients, bound group['max_grad_norm'] (default: the
        optimizer's max_grad_norm; None: measured, not clipped) -- one dep_grad_sqnorm per group with a gradient (at most 8), then
        the one launch per range.  skip_nonfinite stays a decision about the whole step: skipped iff any group's norm is not finite.
        count_skipped=False (needs skip_nonfinite): a skipped step does not advance the step number of the bias correction, as in
        the torch loop that calls step() only on a finite norm; the count of landed updates lives on the device (landed_steps()).
        Any of the three makes every range's launch a dep_adam_step_opt; all at their defaults: the launches above, unchanged."""
        params = list(params)
        if max_grad_value is not None and not (_is_number(max_grad_value) and 0.0 < float(max_grad_value) < float('inf')):
            raise ValueError(f'max_grad_value must be None or a finite number > 0, got {max_grad_value!r}')
        self.max_grad_value = None if max_grad_value is None else float(max_grad_value)
        self.clip_per_group = bool(clip_per_group)
        self.count_skipped = bool(count_skipped)
        if not self.count_skipped and not skip_nonfinite:
            raise ValueError('count_skipped=False needs skip_nonfinite=True: without it no step is ever skipped')
        self._clip2 = None        # device side of the new options: (partials of 8 groups, [coef, norm] per group, two landed counts)
        self._landed_at = 0       # which of the two landed counts the next step reads
        self._group_slots = []    # param_groups indices of the slices the last per-group step measured
        if ema_decay is not None and not 0.0 <= float(ema_decay) < 1.0:
            raise ValueError(f'ema_decay must be None or a number in [0, 1), got {ema_decay!r}')
        self.amsgrad = bool(amsgrad)
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        self._ext = {}            # id(module) -> (vmax or None, ema or None), made by the first update
        self._ema_updates = 0     # updates the average has been through
        self._averaged = False    # inside averaged(): the parameters and the average are exchanged
        if isinstance(accumulate_steps, bool) or not isinstance(accumulate_steps, (int, np.integer)) or accumulate_steps < 1:
            raise ValueError(f'accumulate_steps must be an integer >= 1, got {accumulate_steps!r}')
        self.accumulate_steps = int(accumulate_steps)
        self._pending = 0         # micro-steps in the accumulator since the last update
        self._accum = {}          # id(module) -> flat accumulator, laid out like the module's _flat_grad
        self._accum_plan = None   # [(group, [(owner, start, end), ...]), ...] of the group being accumulated / last updated from
        if max_grad_norm is not None and not float(max_grad_norm) >= 0.0:
            raise ValueError(f'max_grad_norm must be None or a non-negative number, got {max_grad_norm!r}')
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self._clip = None         # device side of the clipped step: (partials, clip_out, stats), made by the first such step
        default_wd = (1e-2 if self.decoupled else 0.0) if weight_decay is None else weight_decay
        if params and isinstance(params[0], dict):
            groups = [dict(g) for g in params]
        else:
            groups = [{'params': params}]
        self.param_groups = []
        for g in groups:
            g = dict(g)
            g['params'] = list(g['params'])
            g.setdefault('lr', lr); g.setdefault('betas', betas); g.setdefault('eps', eps)
            g.setdefault('weight_decay', default_wd)
            if 'max_grad_norm' in g:
                if not self.clip_per_group:
                    raise ValueError("a param group carries 'max_grad_norm' but clip_per_group is False: it would be ignored")
                if g['max_grad_norm'] is not None and not float(g['max_grad_norm']) >= 0.0:
                    raise ValueError(f"a group's max_grad_norm must be None or a non-negative number, got {g['max_grad_norm']!r}")
            self.param_groups.append(g)
        if self.clip_per_group and not self.skip_nonfinite and all(self._bound_of(g) is None for g in self.param_groups):
            raise ValueError('clip_per_group=True with no max_grad_norm anywhere and skip_nonfinite=False measures norms nobody uses')
        self._step = 0
        self._state = {}          # id(module) -> (m, v)
        if self.accumulate_steps > 1:                      # data parallel: ONE gradient exchange per update, of the accumulator
            for g in self.param_groups:
                for p in g['params']:
                    p.owner._defer_grad_sync = True

    def zero_grad(self):
        for g in self.param_groups:
            for p in g['params']:
                p.owner._grad_ready = False

    def _state_of(self, owner):
        st = self._state.get(id(owner))
        if st is None:
            st = (torch.zeros_like(owner._flat_grad), torch.zeros_like(owner._flat_grad))
            self._state[id(owner)] = st
        return st

    def _plan(self):
        """[(group, [(owner, start, end), ...]), ...]: per group the ranges (_grad_ranges) that hold a gradient right now."""
        return [(g, _grad_ranges(g['params'])) for g in self.param_groups]

    def _clips(self):
        return self.max_grad_norm is not None or self.skip_nonfinite or self.clip_per_group

    def _bound_of(self, group):
        """The group's own bound under clip_per_group (None: measured, not clipped)."""
        b = group.get('max_grad_norm', self.max_grad_norm)
        return None if b is None else float(b)

    def _options(self):
        """True when max_grad_value, clip_per_group or count_skipped=False is on: the launches are dep_adam_step_opt's."""
        return self.max_grad_value is not None or self.clip_per_group or not self.count_skipped

    @staticmethod
    def _spans(plan, what):
        """The ranges of all groups in launch order; `what` names the feature whose single launch has to take them all (None: no limit)."""
        spans = [r for _, rs in plan for r in rs]
        if what and len(spans) > _MAX_CLIP_RANGES:
            raise L.DepError(f'gradient {what} covers at most {_MAX_CLIP_RANGES} contiguous gradient ranges per step, this optimizer has {len(spans)}')
        return spans

    def step(self):
        self._refuse_averaged('step()')
        if self.accumulate_steps > 1:
            return self._micro_step()
        self._step += 1
        L.order_note('optimizer step')
        self._update(self._plan(), lambda owner: owner._flat_grad, 'clipping' if self._clips() and not self.clip_per_group else None)

    def _update(self, plan, grad_of, what, have_partials=False):
        """THE update, of every path: one launch per range of `plan`, reading grad_of(owner) -- the owner's _flat_grad or its accumulator.
        Without clipping that is dep_adam_step and nothing else.  With it: ONE dep_grad_sqnorm over the ranges of ALL groups (a global
        norm, as torch's function takes all parameters at once; none when have_partials says the accumulate launch left the sums), then
        dep_adam_step_clipped per range -- one launch more than the plain step.  Every launch derives the coefficient from the same
        partial sums, with the same bits; the first one also updates the statistics record.  Under data parallelism this runs after
        the compute stream joined the communication stream, on the reduced gradients every rank holds alike: the ranks form the same
        coefficient without a collective.  No parameter holds a gradient: nothing is launched."""
        spans = self._spans(plan, what)
        if not spans:
            return
        if self._options():
            return self._update_opt(plan, grad_of, have_partials)
        clip = self._clips()
        if clip:
            partials, clip_out, stats = self._clip_buffers(spans[0][0]._flat_grad.device)
            if not have_partials:
                L.grad_sqnorm([grad_of(o)[s:e] for o, s, e in spans], partials)
            max_norm = 0.0 if self.max_grad_norm is None else self.max_grad_norm          # 0: measure only (skip_nonfinite alone)
        ext = self._extended()
        first = True
        for g, rs in plan:
            b1, b2 = g['betas']
            for owner, s, e in rs:
                m, v = self._state_of(owner)
                args = (owner._flat[s:e], grad_of(owner)[s:e], m[s:e], v[s:e], g['lr'], b1, b2, g['eps'], g['weight_decay'],
                        self.decoupled, self._step)
                if ext:
                    vmax, ema = self._ext_of(owner)
                    L.adam_step_ext(*args, vmax=None if vmax is None else vmax[s:e], ema=None if ema is None else ema[s:e],
                                    ema_decay=self.ema_decay or 0.0, ema_first=self._ema_updates == 0,
                                    partials=partials if clip else None, max_norm=max_norm if clip else 0.0,
                                    skip_nonfinite=self.skip_nonfinite, clip_out=clip_out if clip and first else None,
                                    stats=stats if clip and first else None)
                elif clip:
                    L.adam_step_clipped(*args, partials, max_norm, self.skip_nonfinite, clip_out if first else None,
                                        stats if first else None)
                else:
                    L.adam_step(*args)
                first = False
        if ext:
            self._ema_updates += 1

    def _update_opt(self, plan, grad_of, have_partials):
        """_update with max_grad_value, clip_per_group or count_skipped=False: the same launches in the same order, each a
        dep_adam_step_opt.  Per group: one dep_grad_sqnorm per group that holds a gradient, in param_groups order, into that group's
        slice of one buffer (the accumulate launch's partials describe all ranges together and are not asked for), then every launch
        reads all slices and takes its own group's coefficient.  The landed count: every launch of this step reads one of two device
        words, the first launch -- the one that writes the record -- leaves the new count in the other, and the next step reads
        that one; an update that launches nothing does not turn them."""
        active = [(gi, g, rs) for gi, (g, rs) in enumerate(plan) if rs]
        dev = active[0][2][0][0]._flat_grad.device
        clip = self._clips()
        partials = clip_out = stats = bounds = group_out = landed = None
        ngroups, max_norm = 1, 0.0
        if clip:
            partials, clip_out, stats = self._clip_buffers(dev)
            max_norm = 0.0 if self.max_grad_norm is None else self.max_grad_norm
        if self.clip_per_group:
            ngroups = len(active)
            if ngroups > _MAX_CLIP_GROUPS:
                raise L.DepError(f'clip_per_group covers at most {_MAX_CLIP_GROUPS} param groups with a gradient, this optimizer has {ngroups}')
            for _, _, rs in active:
                if len(rs) > _MAX_CLIP_RANGES:
                    raise L.DepError(f'gradient clipping covers at most {_MAX_CLIP_RANGES} contiguous gradient ranges per group, a group has {len(rs)}')
            partials, group_out, _ = self._clip2_buffers(dev)
            slots = L.grad_norm_slots()
            for k, (_, g, rs) in enumerate(active):
                L.grad_sqnorm([grad_of(o)[s:e] for o, s, e in rs], partials[k * slots:(k + 1) * slots])
            bounds = [0.0 if self._bound_of(g) is None else self._bound_of(g) for _, g, _ in active]
            max_norm = bounds[0] if ngroups == 1 else 0.0       # the bounds are the groups' own; the optimizer's is only their default
            self._group_slots = [gi for gi, _, _ in active]
        elif clip and not have_partials:
            L.grad_sqnorm([grad_of(o)[s:e] for o, s, e in self._spans(plan, None)], partials)
        if not self.count_skipped:
            landed = self._clip2_buffers(dev)[2]
        ext = self._extended()
        first = True
        for k, (_, g, rs) in enumerate(active):
            b1, b2 = g['betas']
            for owner, s, e in rs:
                m, v = self._state_of(owner)
                vmax, ema = self._ext_of(owner) if ext else (None, None)
                at = self._landed_at
                L.adam_step_opt(owner._flat[s:e], grad_of(owner)[s:e], m[s:e], v[s:e], g['lr'], b1, b2, g['eps'], g['weight_decay'],
                                self.decoupled, self._step, vmax=None if vmax is None else vmax[s:e], ema=None if ema is None else ema[s:e],
                                ema_decay=self.ema_decay or 0.0, ema_first=ext and self._ema_updates == 0, partials=partials,
                                max_norm=max_norm, skip_nonfinite=self.skip_nonfinite, clip_out=clip_out if first else None,
                                stats=stats if first else None, max_grad_value=self.max_grad_value, ngroups=ngroups,
                                group=k if self.clip_per_group else 0, group_max_norms=bounds, group_out=group_out if first else None,
                                landed_in=None if landed is None else landed[at:at + 1],
                                landed_out=None if landed is None or not first else landed[1 - at:2 - at])
                first = False
        if landed is not None:
            self._landed_at = 1 - self._landed_at
        if ext:
            self._ema_updates += 1

    def _clip2_buffers(self, dev):
        """(partials of _MAX_CLIP_GROUPS groups, [coef, norm] per group, the two landed counts): made by the first step that needs them."""
        if self._clip2 is None:
            self._clip2 = (torch.empty(_MAX_CLIP_GROUPS * L.grad_norm_slots(), dtype=torch.float64, device=dev),
                           torch.zeros(2 * _MAX_CLIP_GROUPS, dtype=torch.float32, device=dev), torch.zeros(2, dtype=torch.int32, device=dev))
        return self._clip2

    def landed_steps(self):
        """The number of updates that landed (count_skipped=False): read from the device, a host synchronisation like grad_stats()."""
        if self.count_skipped:
            raise L.DepError('landed_steps() needs an optimizer built with count_skipped=False')
        return 0 if self._clip2 is None else int(self._clip2[2][self._landed_at].item())

    # -- AMSGrad and the average of the parameters (amsgrad, ema_decay) -----------------------------------------------
    def _extended(self):
        return self.amsgrad or self.ema_decay is not None

    def _owners(self):
        """The owner modules, in param_groups order."""
        return list({id(p.owner): p.owner for g in self.param_groups for p in g['params']}.values())

    def _ext_of(self, owner):
        """(vmax, ema) of an owner: vmax zeros beside (m, v); ema a flat buffer laid out like owner._flat.  The first update makes the
        averages of ALL owners, each as a copy of the parameters before that update -- one dep_grad_accumulate launch in its `first`
        form (acc = g * 1), no ATen kernel.  The copy is what makes the rest simple: a range the optimizer never updates (dead
        parameters, parameters without a gradient) averages to itself, as AveragedModel's average of a constant does, and the host
        needs no device word to learn whether the first update was skipped (skip_nonfinite): ema_first goes with the optimizer's
        first update whatever became of it, and a skipped one leaves average = parameters, which is what the copy put there.  The
        average then starts at the unchanged parameters instead of at the first update that lands; the two differ by (1 - d) of one
        step's movement."""
        if id(owner) not in self._ext:
            for o in self._owners():
                vmax = torch.zeros_like(o._flat_grad) if self.amsgrad else None
                ema = None
                if self.ema_decay is not None:
                    ema = torch.empty_like(o._flat)
                    L.grad_accumulate([ema], [o._flat], 1.0, True, None)
                self._ext[id(o)] = (vmax, ema)
        return self._ext[id(owner)]

    def _refuse_averaged(self, what):
        if self._averaged:
            raise L.DepError(f'{what} inside averaged(): the parameters hold the average there; leave the context first')

    @contextlib.contextmanager
    def averaged(self):
        """with optimizer.averaged(): every owner's parameters and their average are exchanged in place (one dep_swap per owner) and
        exchanged back on exit, exceptions included.  Inside, model.state_dict(), forward and _common.save see the averaged weights
        (the models rebuild their packed weight images and the LayerNorm fold from the parameters in every forward: nothing stale
        survives the exchange).  step(), flush(), state_dict() and a nested averaged() raise DepError inside.  Before the first
        update the average is the parameters themselves."""
        if self.ema_decay is None:
            raise L.DepError('averaged() needs an optimizer built with ema_decay')
        self._refuse_averaged('averaged()')
        pairs = [(o, self._ext_of(o)[1]) for o in self._owners()]
        done = []
        self._averaged = True
        try:
            for o, ema in pairs:
                L.swap(o._flat, ema)
                done.append((o, ema))
            yield self
        finally:
            for o, ema in done:
                L.swap(o._flat, ema)
            self._averaged = False

    # -- checkpoints ---------------------------------------------------------------------------------------------------
    def state_dict(self):
        """Everything a resumed run needs to continue with the bits of the uninterrupted one, as CPU tensors and plain numbers: the
        step count, the options, each group's hyper-parameters, and per owner (param_groups order) m, v and -- where the options
        ask for them -- vmax, the average and its update count.  Saving in the middle of an accumulation group (pending > 0) is
        refused, not saved: call it after the group's update or after flush().  The record grad_stats() reads is not part of it."""
        self._refuse_averaged('state_dict()')
        if self._pending:
            raise L.DepError(f'state_dict() in the middle of an accumulation group ({self._pending} micro-steps pending): save after the update or flush()')
        cpu = lambda t: None if t is None else t.detach().cpu().clone()
        state = []
        for o in self._owners():
            mv, x = self._state.get(id(o)), self._ext.get(id(o), (None, None))
            state.append({'numel': int(o._flat.numel()), 'm': cpu(mv and mv[0]), 'v': cpu(mv and mv[1]), 'vmax': cpu(x[0]), 'ema': cpu(x[1])})
        sd = {'step': self._step, 'ema_updates': self._ema_updates, 'amsgrad': self.amsgrad, 'ema_decay': self.ema_decay,
              'decoupled': bool(self.decoupled), 'accumulate_steps': self.accumulate_steps,
              'param_groups': [{'lr': g['lr'], 'betas': tuple(g['betas']), 'eps': g['eps'], 'weight_decay': g['weight_decay'],
                                'numel': [int(p.numel) for p in g['params']]} for g in self.param_groups],
              'state': state}
        if not self.count_skipped:
            sd['landed'] = self.landed_steps()          # present when and only when count_skipped is False
        return sd

    def load_state_dict(self, sd):
        """Into an optimizer built the same way over an identically built model.  The groups' hyper-parameters and ema_decay's value
        come from `sd` (torch's rule); a difference in amsgrad, in ema_decay present / absent, in Adam / AdamW, or in any size is a ValueError."""
        self._refuse_averaged('load_state_dict()')
        if bool(sd['amsgrad']) != self.amsgrad:
            raise ValueError(f"load_state_dict: amsgrad is {sd['amsgrad']} in the checkpoint, {self.amsgrad} in this optimizer")
        if (sd['ema_decay'] is None) != (self.ema_decay is None):
            raise ValueError(f"load_state_dict: ema_decay is {sd['ema_decay']} in the checkpoint, {self.ema_decay} in this optimizer")
        if ('landed' in sd) == self.count_skipped:
            raise ValueError(f"load_state_dict: count_skipped is {'landed' not in sd} in the checkpoint, {self.count_skipped} in this optimizer")
        if bool(sd['decoupled']) != bool(self.decoupled):
            raise ValueError('load_state_dict: decoupled weight decay (AdamW) in one of checkpoint and optimizer, not in the other')
        owners = self._owners()
        sizes = [[int(p.numel) for p in g['params']] for g in self.param_groups]
        if [g['numel'] for g in sd['param_groups']] != sizes:
            raise ValueError(f"load_state_dict: parameter group sizes {[g['numel'] for g in sd['param_groups']]} in the checkpoint, {sizes} in this optimizer")
        if [st['numel'] for st in sd['state']] != [int(o._flat.numel()) for o in owners]:
            raise ValueError(f"load_state_dict: owner sizes {[st['numel'] for st in sd['state']]} in the checkpoint, "
                             f'{[int(o._flat.numel()) for o in owners]} in this optimizer')
        for o, st in zip(owners, sd['state']):
            for k, like in (('m', o._flat_grad), ('v', o._flat_grad), ('vmax', o._flat_grad), ('ema', o._flat)):
                if st[k] is not None and st[k].numel() != like.numel():
                    raise ValueError(f'load_state_dict: {k} has {st[k].numel()} elements in the checkpoint, {like.numel()} in this optimizer')
        put = lambda t, like: None if t is None else torch.empty_like(like).copy_(t)
        self._state, self._ext = {}, {}
        for o, st in zip(owners, sd['state']):
            if st['m'] is not None:
                self._state[id(o)] = (put(st['m'], o._flat_grad), put(st['v'], o._flat_grad))
            if st['vmax'] is not None or st['ema'] is not None:
                self._ext[id(o)] = (put(st['vmax'], o._flat_grad), put(st['ema'], o._flat))
        for g, h in zip(self.param_groups, sd['param_groups']):
            g.update(lr=h['lr'], betas=tuple(h['betas']), eps=h['eps'], weight_decay=h['weight_decay'])
        self.ema_decay = sd['ema_decay']
        self._step, self._ema_updates, self._pending = int(sd['step']), int(sd['ema_updates']), 0
        if not self.count_skipped:                       # both words: whichever the next step reads holds the count
            self._clip2_buffers(owners[0]._flat_grad.device)[2].fill_(int(sd['landed']))

    # -- accumulation over micro-batches (accumulate_steps > 1) -------------------------------------------------------
    @property
    def pending(self):
        """Micro-steps accumulated since the last update."""
        return self._pending

    def accumulated_grad(self, p):
        """View of p's accumulated gradient (None for a parameter that receives none): the sum over the micro-steps so far, and after
        an update what that update was made from -- valid until the next group's first micro-step overwrites it."""
        acc = self._accum.get(id(p.owner))
        if acc is None or not p.live or not p.requires_grad:
            return None
        return acc[p.offset:p.offset + p.numel].view(p.shape)

    def _clip_buffers(self, dev):
        """(partials, clip_out, stats): the device side of the clipped update, made by the first step that needs it."""
        if self._clip is None:
            self._clip = (torch.empty(L.grad_norm_slots(), dtype=torch.float64, device=dev),
                          torch.zeros(4, dtype=torch.float32, device=dev), torch.zeros(4, dtype=torch.float64, device=dev))
        return self._clip

    def _micro_step(self):
        """accumulator (+)= the gradients of the last backward: ONE launch over the ranges of all groups (`first` on a group's first
        micro-step: the accumulator is overwritten, nothing clears it).  The K-th micro-step updates; on one rank its launch also
        leaves the partial sums of squares a clipped update needs, so that update launches no dep_grad_sqnorm."""
        L.order_note('optimizer micro-step')
        plan = self._plan()
        spans = self._spans(plan, 'accumulation')
        if not spans:
            return
        first = self._pending == 0
        if first:
            self._accum_plan = plan
        elif spans != self._spans(self._accum_plan, None):
            raise L.DepError('the parameters that hold a gradient changed inside an accumulation group')
        for owner, _, _ in spans:
            if id(owner) not in self._accum:
                self._accum[id(owner)] = torch.zeros_like(owner._flat_grad)
        boundary = self._pending + 1 == self.accumulate_steps
        partials = None
        if boundary and self._clips() and not self.clip_per_group and parallel.transport() == 'none':   # (an exchange follows otherwise: the norm is the reduced sums')
            partials = self._clip_buffers(spans[0][0]._flat_grad.device)[0]
        L.grad_accumulate([self._accum[id(o)][s:e] for o, s, e in spans], [o._flat_grad[s:e] for o, s, e in spans], 1.0, first, partials)
        self._pending += 1
        if boundary:
            self._update_from_accumulator(partials is not None)

    def flush(self):
        """Update from a partial group (an epoch whose number of mini-batches is no multiple of accumulate_steps); nothing pending:
        nothing is launched.  Under data parallelism every rank calls it at the same point (it holds the group's one collective)."""
        self._refuse_averaged('flush()')
        if self._pending:
            self._update_from_accumulator(False)

    def _update_from_accumulator(self, have_partials):
        """_update with the accumulator in the place of _flat_grad, over the plan saved (and its range count checked) at the group's
        first micro-step.  Data parallel: each owner's live bucket of the accumulator is all-reduced first, ONCE, and the norm is that
        of the reduced sums (dep_grad_sqnorm after the join), which every rank holds alike."""
        self._step += 1
        self._pending = 0
        if parallel.transport() != 'none':
            for owner in {id(o): o for o, _, _ in self._spans(self._accum_plan, None)}.values():
                parallel.all_reduce_accumulated(owner, self._accum[id(owner)][:owner._n_live])
        L.order_note('optimizer step')
        self._update(self._accum_plan, lambda owner: self._accum[id(owner)], None, have_partials)

    def grad_stats(self):
        """The record of the clipped steps so far, read from the device: the ONLY host synchronisation of the clipping path.
        steps / clipped / skipped count optimizer steps (clipped: coefficient < 1; skipped: non-finite norm under skip_nonfinite);
        max_norm is the largest finite gradient norm seen, last_norm / last_coef / last_finite describe the latest step."""
        if self._clip is None:
            out = {'steps': 0, 'clipped': 0, 'skipped': 0, 'max_norm': 0.0, 'last_norm': None, 'last_coef': None, 'last_finite': None}
            if self.clip_per_group:
                out['groups'] = self._group_stats()
            return out
        _, clip_out, stats = self._clip
        st, co = stats.tolist(), clip_out.tolist()
        out = {'steps': int(st[0]), 'clipped': int(st[1]), 'skipped': int(st[2]), 'max_norm': float(st[3]),
               'last_norm': float(co[1]), 'last_coef': float(co[0]), 'last_finite': bool(co[2])}
        if self.clip_per_group:
            out['groups'] = self._group_stats()
        return out

    def _group_stats(self):
        """grad_stats()['groups']: per param group the norm and the coefficient of the latest step (None for a group that held no
        gradient in it); last_norm / last_coef at the top are then sqrt(sum of S_g) and the smallest coefficient."""
        out = [{'last_norm': None, 'last_coef': None} for _ in self.param_groups]
        if self._clip2 is not None:
            rec = self._clip2[1].tolist()
            for k, gi in enumerate(self._group_slots):
                out[gi] = {'last_norm': float(rec[2 * k + 1]), 'last_coef': float(rec[2 * k])}
        return out


_MAX_CLIP_RANGES = 16          # dep_grad_sqnorm takes up to 16 ranges per launch (include/dep_rnn.h)
_MAX_CLIP_GROUPS = 8           # dep_adam_step_opt reads up to 8 groups' partial sums per launch


def _is_number(x):
    """A real number, not a bool and not a string: the check _common.optim_options applies to the same values."""
    return not isinstance(x, (bool, np.bool_)) and isinstance(x, (int, float, np.integer, np.floating))


def _grad_ranges(params):
    """[(owner, start, end), ...]: the contiguous runs, in each owner's flat buffers, of those of `params` that currently hold a
    gradient.  The runs include the alignment pads between tensors (Module._finalize keeps them zero)."""
    per_owner = {}
    for p in params:
        if p.grad is None:
            continue
        per_owner.setdefault(id(p.owner), (p.owner, []))[1].append((p.offset, p.offset + (p.numel + 3) // 4 * 4))
    out = []
    for owner, rs in per_owner.values():
        rs.sort()
        cur_s, cur_e = rs[0]
        for s, e in rs[1:]:
            if s == cur_e:
                cur_e = e
            else:
                out.append((owner, cur_s, cur_e)); cur_s, cur_e = s, e
        out.append((owner, cur_s, cur_e))
    return out


class GradNorm:
    """What clip_grad_norm_ returns: the total norm, still on the device.  item() reads it (a host synchronisation, like Loss.item())."""

    def __init__(self, clip_out=None):
        self._out = clip_out            # [coef, norm, finite, 0] written by dep_grad_clip_scale, or None: no gradient at all

    def item(self):
        return 0.0 if self._out is None else float(self._out[1].item())

    def coef(self):
        return 1.0 if self._out is None else float(self._out[0].item())

    def __float__(self):
        return self.item()


def clip_grad_norm_(parameters, max_norm):
    """torch.nn.utils.clip_grad_norm_(parameters, max_norm) (norm_type 2, error_if_nonfinite=False) for hand-written loops: scales the
    gradients of `parameters` in place so that their global 2-norm is at most max_norm, in two launches (dep_grad_sqnorm,
    dep_grad_clip_scale) and without a host read; the returned GradNorm reads the norm lazily.  Parameters whose grad is None are
    left out, as torch leaves them out.  Training loops that step with nn.Adam / nn.AdamW pass max_grad_norm to the optimizer instead:
    that clips inside the update and costs one launch, not two plus a pass over the gradients."""
    if isinstance(parameters, Parameter):
        parameters = [parameters]
    rs = _grad_ranges(list(parameters))
    if not rs:
        return GradNorm()
    if len(rs) > _MAX_CLIP_RANGES:
        raise L.DepError(f'clip_grad_norm_ covers at most {_MAX_CLIP_RANGES} contiguous gradient ranges, got {len(rs)}')
    grads = [owner._flat_grad[s:e] for owner, s, e in rs]
    dev = grads[0].device
    partials = torch.empty(L.grad_norm_slots(), dtype=torch.float64, device=dev)
    clip_out = torch.empty(4, dtype=torch.float32, device=dev)
    L.grad_sqnorm(grads, partials)
    L.grad_clip_scale(grads, partials, float(max_norm), clip_out)
    return GradNorm(clip_out)


def clip_grad_value_(parameters, clip_value):
    """torch.nn.utils.clip_grad_value_(parameters, clip_value) for hand-written loops: clamps the gradients of `parameters` in place to
    [-clip_value, clip_value] in one launch (dep_grad_clip_value) over their merged ranges; a NaN stays NaN.  Parameters whose grad is
    None are left out; nothing is launched when none holds a gradient.  Training loops that step with nn.Adam / nn.AdamW pass
    max_grad_value to the optimizer instead: that clamps inside the update and costs no launch and no pass over the gradients."""
    if not (_is_number(clip_value) and 0.0 < float(clip_value) < float('inf')):
        raise ValueError(f'clip_value must be a finite number > 0, got {clip_value!r}')
    if isinstance(parameters, Parameter):
        parameters = [parameters]
    rs = _grad_ranges(list(parameters))
    if not rs:
        return
    if len(rs) > _MAX_CLIP_RANGES:
        raise L.DepError(f'clip_grad_value_ covers at most {_MAX_CLIP_RANGES} contiguous gradient ranges, got {len(rs)}')
    L.grad_clip_value([owner._flat_grad[s:e] for owner, s, e in rs], float(clip_value))


class Adam(_AdamBase):
    """torch.optim.Adam (Regression/audio_bilstm_perm.py:250, Classification/fuse_net_whole.py:416)."""
    decoupled = False


class AdamW(_AdamBase):
    """torch.optim.AdamW with per-group decoupled weight decay (audio_gru_whole.py:247-255,307)."""
    decoupled = True


# ----------------------------------------------------------------------------- initialisers
def _uniform(shape, bound, gen):
    return ((torch.rand(*shape, generator=gen) * 2 - 1) * bound).numpy()


def default_rnn_init(names_shapes, H, gen):
    """nn.GRU / nn.LSTM reset_parameters: U(-1/sqrt(H), 1/sqrt(H)) for every tensor."""
    k = 1.0 / math.sqrt(H)
    return {n: _uniform(s, k, gen) for n, s in names_shapes}


def default_linear_init(name_w, name_b, out_f, in_f, gen, bias=True):
    """nn.Linear reset_parameters: kaiming_uniform(a=sqrt(5)) == U(-1/sqrt(fan_in), 1/sqrt(fan_in))."""
    k = 1.0 / math.sqrt(in_f)
    d = {name_w: _uniform((out_f, in_f), k, gen)}
    if bias:
        d[name_b] = _uniform((out_f,), k, gen)
    return d


def xavier_uniform(shape, gen):
    fan_out, fan_in = shape[0], shape[1]
    return _uniform(shape, math.sqrt(6.0 / (fan_in + fan_out)), gen)


def make_generator(seed=None):
    """Initialisation RNG of one model.  seed=None draws a sub-seed from torch's GLOBAL generator, which advances it: like
    the reference (whose nn.Module constructors consume the global RNG) every model built in a process -- e.g. the three
    folds of main() -- starts from different weights, and torch.manual_seed() makes the whole sequence reproducible."""
    g = torch.Generator()
    if seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    g.manual_seed(int(seed) & 0x7fffffffffffffff)
    return g


_seed_counter = [0]


def next_dropout_seed():
    """A fresh Philox key per training forward; distinct per data-parallel rank."""
    _seed_counter[0] += 1
    return (int(torch.initial_seed()) * 0x9E3779B97F4A7C15 + _seed_counter[0] * 1000003 + parallel.rank() * 7919) \
        & 0xFFFFFFFFFFFFFFFF
