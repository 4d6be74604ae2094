"""Bits shared by the script-shaped modules: metrics, checkpoint I/O, mini-batch slicing and the training epoch loop,
permutation augmentation.  (Reference: the duplicated helpers at Classification/audio_gru_whole.py:123-159,
text_bilstm_whole.py:116-152, fuse_net_whole.py:30-68.)"""
import contextlib
import functools
import itertools
import os

import numpy as np
import torch

from . import nn, parallel
from . import _lib as L


def save(model, filename):
    """Reference `save()` pickles the whole nn.Module (audio_gru_whole.py:123-126).  The HIP-backed module is
    not picklable as a torch module, so the checkpoint holds what every consumer of those files actually reads:
    the state_dict (name -> CPU tensor) plus the config needed to rebuild the module."""
    save_filename = '{}.pt'.format(filename)
    os.makedirs(os.path.dirname(save_filename) or '.', exist_ok=True)
    payload = _model_payload(model)
    if parallel.rank() == 0:
        torch.save(payload, save_filename)
        print('Saved as %s' % save_filename)


def _model_payload(model):
    return {'state_dict': {k: v.detach().cpu() for k, v in model.state_dict().items()},
            'class': type(model).__name__, 'variant': getattr(model, 'variant', None)}


def save_checkpoint(model, optimizer, filename):
    """`<filename>.pt` = the payload of save() plus 'optimizer': optimizer.state_dict() (step count, moments, and with amsgrad /
    ema_decay the running maximum and the average): what a stopped run needs to continue with the bits it would have had.  Every
    entry is a CPU tensor or a plain number, so load_checkpoint reads it with weights_only=True."""
    save_filename = '{}.pt'.format(filename)
    os.makedirs(os.path.dirname(save_filename) or '.', exist_ok=True)
    payload = dict(_model_payload(model), optimizer=optimizer.state_dict())
    if parallel.rank() == 0:
        torch.save(payload, save_filename)
    return save_filename


def load_checkpoint(model, optimizer, filename):
    """Read `<filename>.pt` of save_checkpoint into a model and an optimizer built the way the saved ones were; returns the payload."""
    payload = torch.load('{}.pt'.format(filename), map_location='cpu', weights_only=True)
    if 'optimizer' not in payload:
        raise ValueError('%s.pt holds no optimizer state (written by save(), not save_checkpoint())' % filename)
    model.load_state_dict(payload['state_dict'])
    optimizer.load_state_dict(payload['optimizer'])
    return payload


def optim_options(config):
    """The scripts' optional config keys as keyword arguments of nn.Adam / nn.AdamW: `amsgrad` (default False), `ema_decay` (default
    None; d in [0, 1) keeps an average of the weights that evaluate() then measures and saves), and the clipping options
    `max_grad_value` (default None; c > 0 clamps the gradients' values inside the update), `clip_per_group` (default False; every
    param group is clipped against its own norm -- a group's own bound goes into the dict get_param_group returns for it, under
    'max_grad_norm'), `skip_nonfinite` (default False) and `count_skipped` (default True; False needs skip_nonfinite).  All absent
    or at their defaults: {} -- the optimizer built is the one it always was."""
    amsgrad, d = config.get('amsgrad', False), config.get('ema_decay')
    if not isinstance(amsgrad, (bool, np.bool_)):
        raise ValueError(f'amsgrad must be True or False, got {amsgrad!r}')
    number = lambda x: not isinstance(x, bool) and isinstance(x, (int, float, np.integer, np.floating))
    if d is not None and (not number(d) or not 0.0 <= float(d) < 1.0):
        raise ValueError(f'ema_decay must be None or a number in [0, 1), got {d!r}')
    out = {}
    if amsgrad:
        out['amsgrad'] = True
    if d is not None:
        out['ema_decay'] = float(d)
    c = config.get('max_grad_value')
    if c is not None and (not number(c) or not 0.0 < float(c) < float('inf')):
        raise ValueError(f'max_grad_value must be None or a finite number > 0, got {c!r}')
    if c is not None:
        out['max_grad_value'] = float(c)
    flags = {}
    for key, default in (('clip_per_group', False), ('skip_nonfinite', False), ('count_skipped', True)):
        flags[key] = config.get(key, default)
        if not isinstance(flags[key], (bool, np.bool_)):
            raise ValueError(f'{key} must be True or False, got {flags[key]!r}')
        if bool(flags[key]) != default:
            out[key] = bool(flags[key])
    if not flags['count_skipped'] and not flags['skip_nonfinite']:
        raise ValueError('count_skipped=False needs skip_nonfinite=True')
    return out


def on_averaged_weights(get_optimizer):
    """Decorator of the scripts' evaluate(): with config['ema_decay'] set the call runs inside optimizer.averaged(), so the metric, the
    save gate and the saved checkpoint are those of the averaged weights.  get_optimizer() returns the module-global optimizer at
    call time; one without an average (or none at all) leaves the call as it is."""
    def wrap(fn):
        @functools.wraps(fn)
        def evaluate(*args, **kwargs):
            opt = get_optimizer()
            ctx = opt.averaged() if getattr(opt, 'ema_decay', None) is not None else contextlib.nullcontext()
            with ctx:
                return fn(*args, **kwargs)
        return evaluate
    return wrap


class StateDictModule(torch.nn.Module):
    """A stock torch.nn.Module whose only content is a state_dict: nested plain modules carrying the tensors under the
    same dotted names, in the same order.  What `export_reference_checkpoint` pickles: the reference's consumers of a
    checkpoint (fuse_net_whole.py:566-588, the *ModelChecking.py scripts) do `torch.load(path).state_dict()`, which works on
    this object wherever this package is importable.  It has no forward()."""

    def __init__(self, state_dict=None, source_class=None):
        super().__init__()
        self.source_class = source_class
        for name, value in (state_dict or {}).items():
            mod, parts = self, name.split('.')
            for part in parts[:-1]:
                if part not in mod._modules:
                    mod.add_module(part, torch.nn.Module())
                mod = mod._modules[part]
            mod.register_parameter(parts[-1], torch.nn.Parameter(value.detach().cpu().clone(), requires_grad=False))

    def forward(self, *args, **kwargs):
        raise NotImplementedError('StateDictModule only carries weights (source: %s); rebuild the model with '
                                  'icassp2022_depression_amd and load_state_dict()' % self.source_class)


def export_reference_checkpoint(model, filename):
    """Write `<filename>.pt` the way the reference's `save()` does -- ONE pickled torch module (the dict payload of
    `save()` cannot be read by code that expects `torch.load(p).state_dict()`)."""
    save_filename = '{}.pt'.format(filename)
    os.makedirs(os.path.dirname(save_filename) or '.', exist_ok=True)
    shell = StateDictModule(model.state_dict(), type(model).__name__)
    if parallel.rank() == 0:
        torch.save(shell, save_filename)
    return save_filename


def load_checkpoint_state_dict(path, allow_pickle=None):
    """state_dict of a checkpoint written by `save()` (a dict of tensors: loaded with weights_only=True, nothing is
    executed), by `export_reference_checkpoint`, or by the reference itself (a pickled nn.Module).  Unpickling a module
    runs code from the file and needs the pickled classes importable under their original path (`__main__.AudioBiLSTM`
    for the reference's scripts); it is only attempted when `allow_pickle` is true (default: env DEP_ALLOW_PICKLE, on unless
    set to 0 -- the reference's own loaders do the same)."""
    try:
        obj = torch.load(path, map_location='cpu', weights_only=True)
    except Exception as safe_err:                      # not a plain tensor container
        if allow_pickle is None:
            allow_pickle = os.environ.get('DEP_ALLOW_PICKLE', '1') != '0'
        if not allow_pickle:
            raise RuntimeError('%s is not a tensor-only checkpoint (%s); pass allow_pickle=True / DEP_ALLOW_PICKLE=1 to '
                               'unpickle it as a module' % (path, type(safe_err).__name__)) from safe_err
        try:
            obj = torch.load(path, map_location='cpu', weights_only=False)
        except AttributeError as e:
            raise RuntimeError('%s pickles a module whose class cannot be found (%s): import or define the class under '
                               'the module path it was saved from (the reference saves `__main__.AudioBiLSTM` / '
                               '`__main__.TextBiLSTM`) before loading' % (path, e)) from e
    if isinstance(obj, dict) and 'state_dict' in obj:
        return obj['state_dict']
    if hasattr(obj, 'state_dict'):          # a pickle of a whole torch module
        return obj.state_dict()
    return obj


def standard_confusion_matrix(y_test, y_test_pred):
    """[[TP, FP], [FN, TN]] (audio_gru_whole.py:128-146).  Like sklearn's confusion_matrix followed by the 2x2
    unpack, this raises ValueError when only one class is present in y_true and y_pred together."""
    yt = np.asarray(y_test.cpu().numpy() if torch.is_tensor(y_test) else y_test).reshape(-1).astype(np.int64)
    yp = np.asarray(y_test_pred.cpu().numpy() if torch.is_tensor(y_test_pred) else y_test_pred).reshape(-1).astype(np.int64)
    labels = np.unique(np.concatenate([yt, yp]))
    if labels.size != 2:
        raise ValueError('not enough values to unpack: confusion matrix is %dx%d' % (labels.size, labels.size))
    lo, hi = labels
    tp = int(np.sum((yt == hi) & (yp == hi))); tn = int(np.sum((yt == lo) & (yp == lo)))
    fp = int(np.sum((yt == lo) & (yp == hi))); fn = int(np.sum((yt == hi) & (yp == lo)))
    return np.array([[tp, fp], [fn, tn]])


def prf(conf_matrix):
    """accuracy / precision / recall / F1 exactly as the reference computes them (audio_gru_whole.py:223-226):
    0/0 gives nan (with numpy's RuntimeWarning), not an exception."""
    tp, fp = conf_matrix[0]; fn, tn = conf_matrix[1]
    accuracy = float(tp + tn) / np.sum(conf_matrix)
    with np.errstate(invalid='ignore', divide='ignore'):
        precision = np.float64(tp) / np.float64(tp + fp)
        recall = np.float64(tp) / np.float64(tp + fn)
        f1 = 2 * (precision * recall) / (precision + recall)
    return accuracy, float(precision), float(recall), float(f1)


# The helpers below are HIP launches on device tensors.  Host tensors only ever reach them from the CPU stand-in model of
# tests/test_host_cpu.py (the real models cannot be built without a GPU: nn._device raises); those take plain host indexing.
def _gather(X, sel):
    return L.gather_rows(X, sel) if X.is_cuda else X[sel]


def predict(output, out=None):
    """`output.data.max(1, keepdim=True)[1]` of the reference loops (audio_gru_whole.py:185) as one HIP launch: (B, 1) int64 first
    arg-max per row, on the device.  `out`: a (B, 1) int64 device view to write into (epoch-level prediction buffers)."""
    probs = output.data if hasattr(output, 'data') else output
    if not probs.is_cuda:
        p = probs.max(1, keepdim=True)[1]
        if out is not None:
            out.copy_(p); return out
        return p
    if out is not None:
        assert out.is_contiguous() and out.dtype == torch.int64 and out.numel() == probs.shape[0]
        assert probs.is_contiguous() and probs.dtype == torch.float32 and probs.dim() == 2
        if probs.shape[0]:
            L.check(L.load().dep_argmax_count(probs.data_ptr(), None, 0, probs.shape[0], probs.shape[1], None, out.data_ptr(),
                                              L.stream()), 'dep_argmax_count')
        return out
    return L.argmax_count(probs, want_pred=True)


def count_correct(output, y_dev, counter):
    """`correct += pred.eq(y.view_as(pred)).sum()` (audio_gru_whole.py:186-187): arg-max, comparison with the device labels and
    the running count in ONE launch (dep_argmax_count); `counter` is a 0-dim int64 device tensor read once per epoch."""
    probs = output.data if hasattr(output, 'data') else output
    if not probs.is_cuda:
        pred = probs.max(1, keepdim=True)[1]
        counter += pred.eq(y_dev.view_as(pred)).sum()
        return
    L.argmax_count(probs, labels=y_dev, count=counter)


def concat_features(text_feature, audio_feature):
    """torch.cat((text_feature, audio_feature), dim=1) (fuse_net_whole.py:434) as two strided copies (dep_copy2d)."""
    if not text_feature.is_cuda:
        return torch.cat((text_feature, audio_feature), dim=1)
    return L.concat2(text_feature, audio_feature)


def prediction_buffer(n, device):
    """(n,) fp32 zeros on the device: the regression loops' predictions of one epoch (audio_bilstm_perm.py:150-160)."""
    if torch.device(device).type != 'cuda':
        return torch.zeros(n, dtype=torch.float32)
    buf = torch.empty(max(n, 1), dtype=torch.float32, device=device)
    L.fill(buf, 0.0)
    return buf[:n]


def store_predictions(buf, at, output):
    """buf[at : at + B] = output.flatten() for a (B, 1) head output (dep_copy2d)."""
    o = output.data if hasattr(output, 'data') else output
    n = o.numel()
    if n and not o.is_cuda:
        buf[at:at + n] = o.reshape(-1)
    elif n:
        assert 0 <= at and at + n <= buf.numel() and buf.dtype == torch.float32 and o.dtype == torch.float32 and o.is_contiguous() \
            and buf.is_contiguous(), 'store_predictions: fp32 contiguous tensors, at + n <= len(buf)'
        L.check(L.load().dep_copy2d(o.data_ptr(), 1, buf.data_ptr() + 4 * at, 1, n, 1, L.stream()), 'dep_copy2d')


def minibatches(n, batch_size):
    """(start, stop) of the reference's python-slice mini-batching; the last batch may be ragged."""
    for i in range(0, n, batch_size):
        yield i, min(n, i + batch_size)


def rank_slice(lo, hi):
    """Rows of the global mini-batch [lo, hi) this data-parallel rank works on."""
    a, b = parallel.shard_slice(hi - lo)
    return lo + a, lo + b


def accumulation_groups(counts, k):
    """Pure helper: cut the epoch's mini-batches (`counts` = their global row counts, in order) into consecutive groups of `k` --
    the last one may be shorter -- and return [(first, stop, rows), ...]: mini-batches first .. stop - 1 form one optimizer update
    whose criteria divide by `rows`, the rows of the whole group."""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1:
        raise ValueError(f'accumulation_groups: k must be an integer >= 1, got {k!r}')
    counts = [int(c) for c in counts]
    return [(i, min(i + k, len(counts)), sum(counts[i:i + k])) for i in range(0, len(counts), int(k))]


def class_row_weight(targets, class_weight, ignore_index=-100):
    """Pure helper: the float64 vector train_epoch(row_weight=) takes -- class_weight[y_i] for a live row, 0 for a row whose label is
    `ignore_index`.  Its sums are the denominators of torch's weighted-mean cross-entropy."""
    y = np.asarray(targets).reshape(-1).astype(np.int64)
    w = np.asarray(class_weight, dtype=np.float64).reshape(-1)
    live = y != ignore_index
    if live.any() and (y[live].min() < 0 or y[live].max() >= w.size):
        bad = int(y[live].min()) if y[live].min() < 0 else int(y[live].max())
        raise IndexError(f'Target {bad} is out of bounds for {w.size} classes')
    out = np.zeros(y.size, dtype=np.float64)
    out[live] = w[y[live]]
    return out


def balanced_class_weight(targets, num_classes, ignore_index=-100):
    """Pure helper: n_live / (C * count_c) per class (sklearn's 'balanced' heuristic) over the rows whose label is not
    `ignore_index`; a class without a row has no finite weight: ValueError."""
    y = np.asarray(targets).reshape(-1).astype(np.int64)
    y = y[y != ignore_index]
    if y.size and (y.min() < 0 or y.max() >= num_classes):
        raise IndexError(f'Target {int(y.min()) if y.min() < 0 else int(y.max())} is out of bounds for {num_classes} classes')
    counts = np.bincount(y, minlength=num_classes).astype(np.float64)
    if np.any(counts == 0):
        raise ValueError('balanced_class_weight: no row of class(es) %s' % np.flatnonzero(counts == 0).tolist())
    return y.size / (num_classes * counts)


def ce_options(config, targets):
    """The scripts' two optional config keys as keyword arguments of the CE criteria: `class_weights` (None, a list of num_classes
    floats, or 'balanced' = balanced_class_weight of `targets`, the labels of the fold being trained AFTER augmentation: the set train()
    iterates) and `label_smoothing` (default 0.0).  Both absent or at their defaults: {} -- the criterion built is the one it always was."""
    cw, eps = config.get('class_weights'), float(config.get('label_smoothing', 0.0) or 0.0)
    if cw is None and eps == 0.0:
        return {}
    if isinstance(cw, str):
        if cw != 'balanced':
            raise ValueError(f"class_weights must be None, a list of num_classes floats or 'balanced', got {cw!r}")
        cw = balanced_class_weight(targets, config['num_classes'])
    elif cw is not None and len(cw) != config['num_classes']:
        raise ValueError(f"class_weights has {len(cw)} entries for {config['num_classes']} classes")
    return {'weight': cw, 'label_smoothing': eps}


def criterion_row_weight(criterion, targets):
    """row_weight for train_epoch: None for a criterion without options (the loop then declares counts only), else the criterion's
    weight of every training row in loop order."""
    opt = getattr(criterion, 'options', None)
    return opt.row_weight(targets) if opt is not None and opt.active else None


def balanced_group_weight(groups):
    """Pure helper: the float64 row weights of sample_weights='balanced' -- n / (G * len(group)) for every row of each of the G groups,
    in the groups' order (the order train() iterates: the fold's depressed list, then its non-depressed list, both after
    augmentation).  Their sum is n; an empty group has no finite weight: ValueError."""
    sizes = [len(g) for g in groups]
    if not sizes or min(sizes) == 0:
        raise ValueError(f'balanced_group_weight: group sizes {sizes} (every group needs a row)')
    n = float(sum(sizes))
    return np.concatenate([np.full(k, n / (len(sizes) * k), dtype=np.float64) for k in sizes])


REG_LOSSES = ('l1', 'smooth_l1', 'huber', 'mse')


def reg_options(config):
    """The regression scripts' optional config keys `loss` (None, 'l1', 'smooth_l1', 'huber', 'mse'), `loss_beta` and `loss_delta`
    (default 1.0) as keyword arguments of nn.RegOptions / models.MyLoss('reg').  `loss` absent or None: {} -- the criterion built is
    the script's own, the one it always was (a beta or delta without a loss would be ignored silently: ValueError)."""
    loss = config.get('loss')
    if loss is None:
        if config.get('loss_beta') is not None or config.get('loss_delta') is not None:
            raise ValueError("loss_beta / loss_delta need config['loss'] ('smooth_l1' / 'huber')")
        return {}
    if loss not in REG_LOSSES:
        raise ValueError(f'loss must be None or one of {list(REG_LOSSES)}, got {loss!r}')
    beta, delta = config.get('loss_beta'), config.get('loss_delta')
    return {'loss': loss, 'beta': 1.0 if beta is None else float(beta), 'delta': 1.0 if delta is None else float(delta)}


def reg_criterion(config, default):
    """The fold's criterion of a regression script: default() (nn.L1Loss or nn.SmoothL1Loss, as the reference builds it) unless
    config['loss'] names another one."""
    o = reg_options(config)
    if not o:
        return default()
    return {'l1': lambda: nn.L1Loss(), 'smooth_l1': lambda: nn.SmoothL1Loss(beta=o['beta']),
            'huber': lambda: nn.HuberLoss(delta=o['delta']), 'mse': lambda: nn.MSELoss()}[o['loss']]()


def sample_row_weight(config, groups):
    """config['sample_weights'] as the row weights of one train() call, in loop order: None (absent: no weights, nothing new is
    called) or 'balanced' = balanced_group_weight(groups)."""
    how = config.get('sample_weights')
    if how is None:
        return None
    if how != 'balanced':
        raise ValueError(f"sample_weights must be None or 'balanced', got {how!r}")
    return balanced_group_weight(groups)


def train_epoch(model, optimizer, n_rows, batch_size, step, after_step=None, row_weight=None):
    """The mini-batch loop of every script's train() (audio_gru_whole.py:161-201 of the reference), which is also the data-parallel
    protocol: per global mini-batch every rank issues the gradient ranges, then (lazily, in LossSum.item) the loss reduce; a rank
    that owns no row of a small mini-batch joins both with a zero contribution.  Returns the summed loss, read from the device
    once -- the epoch's only host synchronisation in here (it raises if a sweep gave up); the caller's ONE epoch-end collective
    (correct count / prediction buffer) follows it on every rank.
      step(a, b, then) -> (loss, output): forward, whatever is enqueued BEFORE the criterion (count_correct), the criterion.
                                          `then` = the next mini-batch's rank slice, None after the last one, for
                                          FeatureFeeder.rows(a, b, then=): a streamed feeder starts that upload beside this step.
      after_step(a, b, output):           whatever is enqueued AFTER optimizer.step() (store_predictions).
    The scripts differ in two ways only: the classification loops count before the criterion and the regression loops store
    after the update (hence two hooks), and the fusion loops ignore `then` (PairFeeder.rows takes none: the pairs are resident).
    An optimizer built with accumulate_steps = K > 1 turns K consecutive mini-batches into one update: the rows of each group are
    declared before its criteria run (every micro-loss is then its rows' sum over the GROUP's rows, so the summed epoch loss is the
    big-batch loop's), optimizer.step() is still called per mini-batch (it accumulates, and updates on the K-th), and flush()
    updates from a shorter last group.  Both hooks, the count and the prediction buffers stay per mini-batch.
      row_weight: for a criterion with class weights / label smoothing / ignore_index (class_row_weight: w[y_i] per training row in
                  loop order, 0 for an ignored row), or a regression criterion called with row weights (those weights).  Its sum over each global mini-batch and over each accumulation group is declared
                  beside the counts (parallel.set_global_weight / set_accumulated_weight): the criteria divide by those sums.  None:
                  none of that is called."""
    total = nn.LossSum(model.device)                 # device-side sum of the step losses
    bounds = list(minibatches(n_rows, batch_size))
    batches = [(rank_slice(lo, hi), hi - lo) for lo, hi in bounds]
    accum = getattr(optimizer, 'accumulate_steps', 1)
    groups = accumulation_groups([n for _, n in batches], accum) if accum > 1 else []
    group_rows = {first: rows for first, _, rows in groups}
    if row_weight is not None:
        row_weight = np.asarray(row_weight, dtype=np.float64).reshape(-1)
        if row_weight.size != n_rows:
            raise ValueError(f'row_weight has {row_weight.size} entries for {n_rows} training rows')
        batch_weight = [float(row_weight[lo:hi].sum()) for lo, hi in bounds]
        group_weight = {first: float(row_weight[bounds[first][0]:bounds[stop - 1][1]].sum()) for first, stop, _ in groups}
    for bi, ((a, b), n_glob) in enumerate(batches):
        parallel.set_global_count(n_glob)
        if row_weight is not None:
            parallel.set_global_weight(batch_weight[bi])
        if bi in group_rows:
            parallel.set_accumulated_count(group_rows[bi])
            if row_weight is not None:
                parallel.set_accumulated_weight(group_weight[bi])
        if b <= a:                                  # this rank owns no row of a small (ragged) mini-batch: zero-contribution step
            total.add(nn.empty_shard_step(model, optimizer))
            continue
        optimizer.zero_grad()
        loss, output = step(a, b, batches[bi + 1][0] if bi + 1 < len(batches) else None)
        loss.backward()
        optimizer.step()
        if after_step is not None:
            after_step(a, b, output)
        total.add(loss, model)
    if accum > 1:
        optimizer.flush()                           # a last group shorter than K (every rank: it holds that group's collective)
        parallel.set_accumulated_count(None)
    parallel.set_global_count(None)
    if row_weight is not None:
        parallel.set_accumulated_weight(None)
        parallel.set_global_weight(None)
    return total.item()


def fusion_forward(model, rows, lengths=None):
    """pretrained_feature -> cat(text, audio) -> head of the fusion loops (fuse_net_whole.py:441-448): `rows` is what
    fusion_net.pretrained_feature takes, PairFeeder rows or a list slice of pairs; `lengths` the (audio_lengths, text_lengths) of a
    ragged batch (PairFeeder.lengths_rows), None for a dense one.  Returns (text_feature, audio_feature, output)."""
    text_feature, audio_feature = model.pretrained_feature(rows) if lengths is None else model.pretrained_feature(rows, lengths=lengths)
    return text_feature, audio_feature, model(concat_features(text_feature, audio_feature))


def fusion_audio_state(model, audio_state_dict, listed):
    """What the fusion scripts' transplant() loads from an audio checkpoint.  A unidirectional model and checkpoint: the `listed`
    keys, as the reference lists them.  A model built with audio_bidirectional=True: every `lstm_net_audio.*` key of the checkpoint,
    `_reverse` ones included, the checkpoint's `attention_layer.0.*` under the fusion model's `attention_layer_audio.0.*`, and the
    listed keys that are not the stack's.  A unidirectional checkpoint offered to a bidirectional model, or the reverse, is a
    DepError naming the first key without a counterpart: strict=False would leave random reverse weights."""
    bi = bool(getattr(model, 'audio_bidirectional', False))
    rev = [k for k in audio_state_dict if k.startswith('lstm_net_audio.') and k.endswith('_reverse')]
    if not bi:
        if rev:
            raise L.DepError(f'transplant: the audio checkpoint is bidirectional ({rev[0]} has no counterpart in this model): build the '
                             "fusion model with audio_bidirectional=True (config['audio_bidirectional'])")
        return {k: audio_state_dict[k] for k in listed}
    want = [k for k in model.state_dict() if k.startswith('lstm_net_audio.')]
    out = {}
    for k in want:
        if k not in audio_state_dict:
            raise L.DepError(f'transplant: the fusion model is bidirectional in its audio branch and the audio checkpoint has no {k}: '
                             "it is a unidirectional checkpoint (config['bidirectional'] = False)")
        out[k] = audio_state_dict[k]
    for k in ('weight', 'bias'):
        if f'attention_layer.0.{k}' not in audio_state_dict:
            raise L.DepError(f'transplant: the audio checkpoint has no attention_layer.0.{k} for attention_layer_audio.0.{k}')
        out[f'attention_layer_audio.0.{k}'] = audio_state_dict[f'attention_layer.0.{k}']
    out.update({k: audio_state_dict[k] for k in listed if not k.startswith('lstm_net_audio.')})
    return out


def mae_rmse(y, pred):
    """(MAE, RMSE) in float64, as sklearn's mean_absolute_error / sqrt(mean_squared_error) give them (Regression/audio_bilstm_perm.py:167-171)."""
    y =np.asarray(y, np.float64); pred = np.asarray(pred, np.float64)
    return float(np.mean(np.abs(y - pred))), float(np.sqrt(np.mean((y - pred) ** 2)))


def epoch_mae_rmse(y, pred_dev):
    """Epoch end of the regression train() loops: the ranks' prediction buffers (own rows, zeros elsewhere) are assembled by ONE
    all-reduce, on every rank -- same sequence on working and empty-shard ranks, no per-step host copy."""
    pred = parallel.all_reduce_sum(pred_dev).cpu().numpy().astype(np.float64) if len(y) else np.array([])
    return mae_rmse(y, pred)


def report_prf(conf_matrix):
    """The metric block the classification evaluate()s print after the confusion matrix (audio_gru_whole.py:227-231)."""
    accuracy, precision, recall, f1_score = prf(conf_matrix)
    print("Accuracy: {}".format(accuracy))
    print("Precision: {}".format(precision))
    print("Recall: {}".format(recall))
    print("F1-Score: {}\n".format(f1_score))
    print('=' * 89)
    return accuracy, precision, recall, f1_score


def permutation_augment(features, targets, idxs, is_positive, keep, label=None):
    """Append time-axis permutations of the selected samples (audio_gru_whole.py:268-299): for every idx in
    `idxs` with is_positive(idx) the permutations numbered `keep` (lexicographic order of
    itertools.permutations) are appended to features/targets and their new indices returned; other
    indices pass through.  Returns (features, targets, out_idxs)."""
    out = []
    new_f = []; new_t = []
    n0 = len(features)
    for idx in idxs:
        if is_positive(idx):
            feat = features[idx]
            for count, perm in enumerate(itertools.permutations(range(feat.shape[0]))):
                if count in keep:
                    new_f.append(feat[list(perm)])
                    new_t.append(targets[idx] if label is None else label)
                    out.append(n0 + len(new_f) - 1)
        else:
            out.append(idx)
    if new_f:
        features = np.concatenate([features, np.stack(new_f)], 0)
        targets = np.concatenate([targets, np.asarray(new_t, dtype=targets.dtype)])
    return features, targets, out


# ------------------------------------------------------------------------------------------------------ input pipeline
# The reference builds every mini-batch on the host and converts it per step (`torch.from_numpy(x).type(FloatTensor)`,
# audio_gru_whole.py:170-179); on a GPU that is a synchronous pageable upload in front of every step -- 157 MB = 2.5 ms at
# BASELINE cfg2 against a 4.4 ms step.  An MI355X has 288 GB of HBM: the fp32 feature array is uploaded ONCE
# (it only changes when a fold appends permutations, which makes a new ndarray) and a mini-batch is a device-side row gather.
# Arrays beyond the budget (DEP_FEATURES_HBM_GB, default 64) are fed from a pinned fp32 host copy by a copy stream, one
# mini-batch ahead of the step that consumes it.
_dev_cache = {}


def invalidate_device_features():
    """Forget the HBM-resident feature copies (call after modifying a feature array IN PLACE; the scripts never do)."""
    _dev_cache.clear()


def _fingerprint(arr):
    """Content check of a cached array.  Default: a strided sample (<= 64k elements) PLUS one probe element of EVERY row (at a
    row-dependent column) -- catches whole-array edits and the replacement / edit of any single row at the probed position;
    an in-place edit that misses every probe is NOT seen: call invalidate_device_features() after editing a feature array in
    place (the scripts never do: their fold loops build new arrays).  DEP_FEATURES_HASH=1 hashes the whole array instead
    (xxh3, ~0.15 s per GB on the host)."""
    if os.environ.get('DEP_FEATURES_HASH', '0') == '1':
        try:
            import xxhash
            return ('xxh3', xxhash.xxh3_64_intdigest(memoryview(np.ascontiguousarray(arr)).cast('B')))
        except Exception:                                   # noqa: BLE001 -- no xxhash: the sampled check below
            pass
    flat = arr.reshape(-1)
    step = max(1, flat.size // 65536)
    s = float(np.asarray(flat[::step], dtype=np.float64).sum())
    if arr.ndim >= 2 and arr.shape[0] > 0 and flat.size > 0:          # (zero-width rows have nothing to probe)
        rows = arr.reshape(arr.shape[0], -1)
        cols = (np.arange(rows.shape[0], dtype=np.int64) * 2654435761) % rows.shape[1]
        s2 = float(np.asarray(rows[np.arange(rows.shape[0]), cols], dtype=np.float64).sum())
        return (s, s2)
    return (s, 0.0)


def device_features(arr, device, role='x'):
    """fp32 HBM copy of a host feature array, cached per `role` and refreshed when the array object / shape / sampled
    content changes (the cache keeps a reference to the host array, so its id cannot be recycled).  None when the array does
    not fit the budget."""
    arr = np.asarray(arr)
    budget = float(os.environ.get('DEP_FEATURES_HBM_GB', '64')) * 2 ** 30
    if arr.size * 4 > budget:
        return None
    hit = _dev_cache.get(role)
    if hit is not None and hit[0] is arr and hit[1] == (arr.shape, str(arr.dtype), str(device), _fingerprint(arr)):
        return hit[2]
    t = torch.from_numpy(np.ascontiguousarray(arr, dtype=np.float32)).to(device)
    _dev_cache[role] = (arr, (arr.shape, str(arr.dtype), str(device), _fingerprint(arr)), t)
    return t


def pad_ragged(seqs):
    """A ragged corpus -> (x, lengths): `seqs` is a list of (T_i, F) arrays, or the object array a ragged Python list becomes in
    `np.savez` (load it with `np.load(path, allow_pickle=True)`: numpy refuses object arrays otherwise) -- e.g. one NetVLAD vector
    per interview topic, DAICFeatureExtarction/feature_extraction.py:31-64 of the reference.  x is the zero-padded float32
    (N, max T_i, F) array, lengths the int32 (N,) vector the models' `lengths=` argument takes.  The padding is zeros: the ragged
    entry points need it finite (include/dep_rnn.h).  An empty sequence (T_i = 0) needs an explicit (0, F) shape."""
    items = [np.asarray(s, dtype=np.float32) for s in seqs]
    if not items:
        raise ValueError('pad_ragged: no sequences')
    for i, a in enumerate(items):
        if a.ndim != 2:
            raise ValueError(f'pad_ragged: sequence {i} has shape {a.shape}, expected (T_i, F)')
    F = items[0].shape[1]
    if any(a.shape[1] != F for a in items):
        raise ValueError('pad_ragged: the sequences differ in their feature width')
    lengths = np.asarray([a.shape[0] for a in items], dtype=np.int32)
    x = np.zeros((len(items), max(1, int(lengths.max())), F), dtype=np.float32)
    for i, a in enumerate(items):
        x[i, :a.shape[0]] = a
    return x, lengths


class FeatureFeeder:
    """Mini-batch inputs of one epoch, already on the device.  rows(a, b) = fp32 features of idxs[a:b] -- the rows the
    reference slices out of `features[idxs]` -- as a (b-a, T, F) device tensor.
    lengths: the int32 lengths of a padded ragged corpus (pad_ragged), one per row of `features`; the lengths of `idxs` are kept on
    the device and lengths_rows(a, b) is the slice that belongs to rows(a, b)."""

    def __init__(self, features, idxs, device, role='x', lengths=None):
        self.idxs = np.asarray(idxs, dtype=np.int64).reshape(-1)
        self.device = device
        n_rows = len(features)
        self.len_dev = None
        if lengths is not None:
            ln = np.asarray(lengths)
            if ln.shape != (n_rows,) or not np.issubdtype(ln.dtype, np.integer):
                raise ValueError(f'lengths: expected {n_rows} integers, one per feature row, got {ln.shape} {ln.dtype}')
        if self.idxs.size and (self.idxs.min() < 0 or self.idxs.max() >= n_rows):      # the device gather does not range-check (index_select did)
            bad = int(self.idxs.min()) if self.idxs.min() < 0 else int(self.idxs.max())
            raise IndexError(f'index {bad} is out of bounds for a feature array of {n_rows} rows')
        self.Xd = device_features(features, device, role)
        self.contiguous = self.idxs.size > 0 and bool(np.all(np.diff(self.idxs) == 1))
        if self.Xd is not None:
            self.idx_dev = torch.as_tensor(self.idxs, device=device)
        else:                                         # too large for HBM: pinned fp32 copy of the epoch's rows, streamed
            self.host = torch.from_numpy(np.ascontiguousarray(np.asarray(features)[self.idxs], dtype=np.float32)).pin_memory()
            self.copy_stream = torch.cuda.Stream(device=device)
            self.inflight = {}
        if lengths is not None:                       # gathered once, on the host: lengths_rows is then always a view
            self.len_dev = torch.as_tensor(np.ascontiguousarray(ln[self.idxs], dtype=np.int32), device=device)

    def lengths_rows(self, a, b):
        """int32 device lengths of rows(a, b) (a view: no gather, no host synchronisation); None for a dense corpus."""
        return None if self.len_dev is None else self.len_dev[a:b]

    def _start(self, a, b):
        if (a, b) in self.inflight or b <= a:
            return
        with torch.cuda.stream(self.copy_stream):
            t = self.host[a:b].to(self.device, non_blocking=True)
            ev = torch.cuda.Event(); ev.record(self.copy_stream)
        self.inflight[(a, b)] = (t, ev)

    def rows(self, a, b, then=None):
        """`then` = (a2, b2) of the NEXT mini-batch: its upload is started now, beside this step (streamed mode only)."""
        if self.Xd is not None:
            if self.contiguous:                    # idxs is a run i, i+1, ...: a view, no gather
                return self.Xd[int(self.idxs[0]) + a:int(self.idxs[0]) + b]
            return _gather(self.Xd, self.idx_dev[a:b])                       # dep_gather_rows: the mini-batch out of the HBM-resident corpus
        self._start(a, b)
        t, ev = self.inflight.pop((a, b))
        torch.cuda.current_stream().wait_event(ev)
        t.record_stream(torch.cuda.current_stream())
        if then is not None:
            self._start(*then)
        return t


def device_labels(targets, device, num_classes=None):
    """The epoch's labels on the device, uploaded once (a per-step `y.to(device)` of a pageable host tensor is a blocking copy
    behind everything already queued: the host could never run ahead of the GPU).  Class labels are range-checked here, on the
    host, like torch's CrossEntropyLoss would per batch (IndexError)."""
    t = np.asarray(targets)
    if num_classes is not None:
        t = t.astype(np.int64)
        if t.size and (t.min() < 0 or t.max() >= num_classes):
            bad = int(t.min()) if t.min() < 0 else int(t.max())
            raise IndexError(f'Target {bad} is out of bounds for {num_classes} classes')
        return torch.as_tensor(t, device=device)
    return torch.as_tensor(t.astype(np.float32), device=device)


class PairFeeder:
    """The fusion scripts' list of [audio_i, text_i] pairs (fuse_net_whole.py:27, grown by append in the fold loop) as two
    HBM-resident fp32 tensors, stacked and uploaded once per (list object, length); rows(a, b) = the (audio, text) tensors of
    idxs[a:b], which `fusion_net.pretrained_feature` accepts in place of the list slice.  Lists whose items differ in shape keep
    the per-batch path (rows() then returns the list slice itself).
    ragged=True: the items may differ in length, audio_i (Ta_i, Fa) and text_i (Tt_i, Ft).  Each modality is padded once with
    pad_ragged, the two int32 length vectors of `idxs` stay on the device, rows(a, b) are the padded tensors and lengths_rows(a, b)
    the (audio_lengths, text_lengths) views that go with them -- `pretrained_feature(rows, lengths=...)`."""

    def __init__(self, pairs, idxs, device, ragged=False):
        self.pairs = pairs
        self.idxs = [int(i) for i in idxs]
        self.device = device
        self.ok = False
        self.len_dev = None
        n = len(pairs)
        if ragged:
            self._init_ragged(n)
            return
        if n == 0:
            return
        hit = _dev_cache.get('fuse_pairs')
        # every pair contributes two probe elements per modality (first / middle), the first and last pairs their full sums: replacing
        # or editing a middle pair in place is seen unless it misses all probes (then: invalidate_device_features())
        def probe(e):
            a, t = np.asarray(e[0]).reshape(-1), np.asarray(e[1]).reshape(-1)
            if a.size == 0 or t.size == 0:                # an empty modality array has nothing to probe
                return 0.0
            return float(a[0]) + float(a[a.size // 2]) + float(t[0]) + float(t[t.size // 2])
        if any(i < 0 or i >= n for i in self.idxs):       # the device gather does not range-check
            raise IndexError(f'pair index out of bounds for a list of {n} pairs')
        key = (n, np.asarray(pairs[0][0]).shape, np.asarray(pairs[0][1]).shape, str(device),
               float(np.asarray(pairs[0][0], dtype=np.float64).sum() + np.asarray(pairs[-1][1], dtype=np.float64).sum()),
               float(sum(probe(e) for e in pairs)))
        if hit is not None and hit[0] is pairs and hit[1] == key:
            self.Xa, self.Xt = hit[2]
        else:
            try:
                xa = np.stack([np.asarray(e[0], dtype=np.float32) for e in pairs])
                xt = np.stack([np.asarray(e[1], dtype=np.float32) for e in pairs])
            except ValueError:                            # ragged items: no stacked copy
                return
            if (xa.size + xt.size) * 4 > float(os.environ.get('DEP_FEATURES_HBM_GB', '64')) * 2 ** 30:
                return
            self.Xa, self.Xt = torch.from_numpy(xa).to(device), torch.from_numpy(xt).to(device)
            _dev_cache['fuse_pairs'] = (pairs, key, (self.Xa, self.Xt))
        self.idx_dev = torch.as_tensor(np.asarray(self.idxs, dtype=np.int64), device=device)
        self.ok = True

    def _init_ragged(self, n):
        if n == 0:
            raise ValueError('PairFeeder(ragged=True): no pairs')
        if any(i < 0 or i >= n for i in self.idxs):       # the device gather does not range-check
            raise IndexError(f'pair index out of bounds for a list of {n} pairs')
        shapes = tuple((np.shape(e[0]), np.shape(e[1])) for e in self.pairs)
        def probe(e):
            a, t = np.asarray(e[0]).reshape(-1), np.asarray(e[1]).reshape(-1)
            return (float(a[0]) + float(a[a.size // 2]) if a.size else 0.0) + (float(t[0]) + float(t[t.size // 2]) if t.size else 0.0)
        # the key covers what the padded arrays are made of: every item's shape (so every length), and the dense feeder's probes
        key = (n, shapes, str(self.device), float(np.asarray(self.pairs[0][0], dtype=np.float64).sum() + np.asarray(self.pairs[-1][1], dtype=np.float64).sum()),
               float(sum(probe(e) for e in self.pairs)))
        hit = _dev_cache.get('fuse_pairs_ragged')
        if hit is not None and hit[0] is self.pairs and hit[1] == key:
            self.Xa, self.Xt, la, lt = hit[2]
        else:
            xa, la = pad_ragged([e[0] for e in self.pairs])
            xt, lt = pad_ragged([e[1] for e in self.pairs])
            if (xa.size + xt.size) * 4 > float(os.environ.get('DEP_FEATURES_HBM_GB', '64')) * 2 ** 30:
                raise ValueError('PairFeeder(ragged=True): the padded pair arrays exceed DEP_FEATURES_HBM_GB; a ragged corpus has no streamed path')
            self.Xa, self.Xt = torch.from_numpy(xa).to(self.device), torch.from_numpy(xt).to(self.device)
            _dev_cache['fuse_pairs_ragged'] = (self.pairs, key, (self.Xa, self.Xt, la, lt))
        sel = np.asarray(self.idxs, dtype=np.int64)
        self.idx_dev = torch.as_tensor(sel, device=self.device)
        # gathered once, on the host: lengths_rows is then always a pair of views
        self.len_dev = (torch.as_tensor(np.ascontiguousarray(la[sel], dtype=np.int32), device=self.device),
                        torch.as_tensor(np.ascontiguousarray(lt[sel], dtype=np.int32), device=self.device))
        self.ok = True

    def lengths_rows(self, a, b):
        """(audio_lengths, text_lengths) of rows(a, b), int32 device views (no gather, no host synchronisation); None for a dense feeder."""
        return None if self.len_dev is None else (self.len_dev[0][a:b], self.len_dev[1][a:b])

    def rows(self, a, b):
        if not self.ok:
            return [self.pairs[i] for i in self.idxs[a:b]]
        sel = self.idx_dev[a:b]
        return (_gather(self.Xa, sel), _gather(self.Xt, sel))
