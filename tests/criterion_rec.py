"""The call trace of the criteria on the CPU: what tests/test_criterion_calls_cpu.py replays and tests/golden/make_criterion_calls.py records.

A criterion call touches the device through nn._device and eight functions of the binding only.  With nn._device answering 'cpu', those
eight replaced by recorders and a stand-in owner, the whole host path runs without a GPU and every launch it would enqueue is logged: the
entry point, its scalar arguments, which buffers it gets (the index of a buffer's first appearance in the trace: the `rows` a head launch
writes are the `rows` the reduce reads), the target's and the weights' dtype and values, and the denominator as float.hex() or 'device'.
Arguments pass through Python signatures with the binding's defaults, so positional or keyword spelling does not matter.  On the CPU
is_cuda is never true: the device-resident labels / weights branch is not in this trace (the GPU tests pin its kernel names and numbers).

Only names that exist before and after the criteria's call path was made one are used: the public criterion classes, nn.Output,
models.MyLoss and the parallel setters."""
import contextlib
import itertools

import numpy as np
import torch

B = 5
HT, HA = 3, 2                                     # the fusion loss's text / audio feature widths


@contextlib.contextmanager
def patched(obj, name, value):
    old = getattr(obj, name)
    setattr(obj, name, value)
    try:
        yield
    finally:
        setattr(obj, name, old)


class Trace:
    def __init__(self):
        self.calls = []
        self.tensors = {}                         # buffer index -> [dtype, values] of the targets and weights
        self._ids = {}
        self._keep = []                           # the buffers stay alive: an address names one buffer for the whole trace

    def buf(self, t, values=False):
        if t is None:
            return None
        key = (t.untyped_storage().data_ptr(), t.storage_offset(), t.numel())
        if key not in self._ids:
            self._ids[key] = len(self._ids)
            self._keep.append(t)
        i = self._ids[key]
        if values:
            self.tensors[str(i)] = [str(t.dtype).replace('torch.', ''), list(t.shape), t.reshape(-1).tolist()]
        return i

    def norm(self, norm):
        if torch.is_tensor(norm):
            assert norm.dtype == torch.float32 and norm.numel() == 1
            return ['device', self.buf(norm), float(norm).hex()]
        return float(norm).hex()

    # the eight entry points, with the binding's signatures
    def head_loss(self, kind, z, target, out, loss_rows, dz, norm):
        self.calls.append(['head_loss', int(kind), self.buf(z), self.buf(target, True), self.buf(out), self.buf(loss_rows), self.buf(dz),
                           self.norm(norm)])

    def head_loss_ce(self, kind, z, target, out, loss_rows, dz, norm, class_weight=None, label_smoothing=0.0, ignore_index=-100):
        self.calls.append(['head_loss_ce', int(kind), self.buf(z), self.buf(target, True), self.buf(out), self.buf(loss_rows), self.buf(dz),
                           self.norm(norm), self.buf(class_weight, True), float(label_smoothing).hex(), int(ignore_index)])

    def head_loss_reg(self, form, relu, param, z, target, out, loss_rows, dz, norm, row_weight=None):
        self.calls.append(['head_loss_reg', int(form), int(relu), float(param).hex(), self.buf(z), self.buf(target, True), self.buf(out),
                           self.buf(loss_rows), self.buf(dz), self.norm(norm), self.buf(row_weight, True)])

    def reduce_loss_by(self, loss_rows, norm_dev, loss_out, accumulate=False):
        assert torch.is_tensor(norm_dev)
        self.calls.append(['reduce_loss_by', self.buf(loss_rows), self.norm(norm_dev), self.buf(loss_out), bool(accumulate)])

    def reduce_loss_of(self, binding_reduce_loss):
        def reduce_loss(loss_rows, norm, loss_out, accumulate=False):
            if torch.is_tensor(norm):             # a binding that takes a device scalar here hands it on itself: to the recorder above
                return binding_reduce_loss(loss_rows, norm, loss_out, accumulate)
            self.calls.append(['reduce_loss', self.buf(loss_rows), self.norm(norm), self.buf(loss_out), bool(accumulate)])
        return reduce_loss

    def ce_weight_sum(self, target, class_weight, ignore_index, num_classes, den_out):
        self.calls.append(['ce_weight_sum', self.buf(target, True), self.buf(class_weight, True), int(ignore_index), int(num_classes),
                           self.buf(den_out)])

    def row_weight_sum(self, row_weight, scale, den_out):
        self.calls.append(['row_weight_sum', self.buf(row_weight, True), float(scale).hex(), self.buf(den_out)])

    def gemm(self, transA, transB, M, N, K, A, lda, B, ldb, Cm, ldc, bias=None, beta=0.0, seq_T=0, shiftB=0, ws=None):
        self.calls.append(['gemm', transA, transB, M, N, K, self.buf(A), lda, self.buf(B), ldb, self.buf(Cm), ldc, self.buf(bias), float(beta),
                           seq_T, shiftB, self.buf(ws)])


class Owner:
    """What a criterion needs of the module behind an Output."""

    def __init__(self, trace, training):
        self.training = training
        self._trace = trace

    def backward(self, dz):
        self._trace.calls.append(['owner.backward', self._trace.buf(dz)])

    def check_health(self):
        pass


class _Weight:
    def __init__(self, Cc):
        g = torch.Generator().manual_seed(3)
        self.data = torch.randn(Cc, HT + HA, generator=g)
        self._grad = torch.zeros(Cc, HT + HA)
        self.requires_grad = True


class FusionOwner(Owner):
    """What models.MyLoss needs of the fusion net."""

    def __init__(self, trace, training, Cc):
        super().__init__(trace, training)
        self._params = {'fc_final.0.weight': _Weight(Cc)}
        self._grad_ready = False

    def sync_plan(self):
        return {}, []


# ---------------------------------------------------------------------------------------------------------------- the cases
Y = [0, 1, 1, 0, 1]
Y_SOME = [0, 1, -1, 0, 1]                          # with ignore_index -1: one ignored row
Y_NONE = [-1] * B                                 # ... every row ignored
V = [0.05, 0.3, 0.0, 1.5, 0.2]
W_ROWS = [0.5, 0.0, 2.0, 1.25, 3.0]
LABEL_SPELLINGS = {'i64_tensor': lambda y: torch.tensor(y, dtype=torch.int64), 'i32_ndarray': lambda y: np.array(y, dtype=np.int32),
                   'list': lambda y: list(y)}
VALUE_SPELLINGS = {'f64_ndarray': lambda v: np.array(v, dtype=np.float64).reshape(B, 1),
                   'f32_tensor': lambda v: torch.tensor(v, dtype=torch.float32).reshape(B, 1)}


def _criteria():
    """[(name, family, make(nn, models), target, call keywords)]: family 'labels' | 'values' | 'fusion_labels' | 'fusion_values'."""
    res = [('ce', 'labels', lambda nn, m: nn.CrossEntropyLoss(), Y, {}),
           ('ce_weight', 'labels', lambda nn, m: nn.CrossEntropyLoss(weight=[0.5, 2.0]), Y, {}),
           ('ce_smoothing', 'labels', lambda nn, m: nn.CrossEntropyLoss(label_smoothing=0.1), Y, {}),
           ('ce_ignore', 'labels', lambda nn, m: nn.CrossEntropyLoss(ignore_index=-1), Y_SOME, {}),
           ('ce_all_ignored', 'labels', lambda nn, m: nn.CrossEntropyLoss(weight=[0.5, 2.0], ignore_index=-1), Y_NONE, {})]
    regs = [('l1', lambda nn, m: nn.L1Loss()), ('smoothl1', lambda nn, m: nn.SmoothL1Loss()),
            ('smoothl1_half', lambda nn, m: nn.SmoothL1Loss(beta=0.5)), ('smoothl1_zero', lambda nn, m: nn.SmoothL1Loss(beta=0.0)),
            ('huber', lambda nn, m: nn.HuberLoss()), ('mse', lambda nn, m: nn.MSELoss())]
    for name, make in regs:
        res.append((name, 'values', make, V, {}))
        res.append((name + '_weight', 'values', make, V, {'weight': W_ROWS}))
    res.append(('mse_zero_weights', 'values', lambda nn, m: nn.MSELoss(), V, {'weight': [0.0] * B}))
    res += [('fusion_clf', 'fusion_labels', lambda nn, m: m.MyLoss('clf'), Y, {}),
            ('fusion_clf_options', 'fusion_labels', lambda nn, m: m.MyLoss('clf', weight=[0.5, 2.0], label_smoothing=0.1, ignore_index=-1), Y_SOME, {}),
            ('fusion_reg', 'fusion_values', lambda nn, m: m.MyLoss('reg'), V, {}),
            ('fusion_reg_l1', 'fusion_values', lambda nn, m: m.MyLoss('reg', loss='l1'), V, {}),
            ('fusion_reg_mse', 'fusion_values', lambda nn, m: m.MyLoss('reg', loss='mse'), V, {}),
            ('fusion_reg_weight', 'fusion_values', lambda nn, m: m.MyLoss('reg'), V, {'weight': W_ROWS})]
    return res


MODES = ('train', 'eval', 'no_owner')             # no_owner: the Output of FusionNet.forward; the fusion loss always has its model
STATES = ('nothing', 'accumulated_count', 'accumulated_weight', 'two_ranks_global_count', 'two_ranks_global_weight', 'two_ranks_nothing')


def cases():
    """[(case name, criterion, spelling, mode, state)]: the product of the four axes."""
    res = []
    for crit in _criteria():
        spellings = LABEL_SPELLINGS if crit[1].endswith('labels') else VALUE_SPELLINGS
        for sp, mode, state in itertools.product(spellings, MODES, STATES):
            if mode == 'no_owner' and crit[1].startswith('fusion'):
                continue
            res.append(('%s/%s/%s/%s' % (crit[0], sp, mode, state), crit, sp, mode, state))
    return res


@contextlib.contextmanager
def _declared(parallel, state):
    with contextlib.ExitStack() as st:
        if state.startswith('two_ranks'):
            st.enter_context(patched(parallel, 'world_size', lambda: 2))
        try:
            if state == 'accumulated_count':
                parallel.set_accumulated_count(12)
            elif state == 'accumulated_weight':
                parallel.set_accumulated_weight(7.5)
            elif state == 'two_ranks_global_count':
                parallel.set_global_count(9)
            elif state == 'two_ranks_global_weight':
                parallel.set_global_weight(6.25)
            yield
        finally:
            parallel.set_accumulated_count(None); parallel.set_accumulated_weight(None)
            parallel.set_global_count(None); parallel.set_global_weight(None)


def record(case):
    """The trace of one case: {'calls': [...], 'tensors': {...}, 'loss': {...}} or, for a refused call, {..., 'raises': type name}."""
    from icassp2022_depression_amd import models, nn, parallel
    _, (_, family, make, target, kw), spelling, mode, state = case
    tr = Trace()
    Lb = nn.L
    with contextlib.ExitStack() as st:
        st.enter_context(patched(nn, '_device', lambda: torch.device('cpu')))
        for name in ('head_loss', 'head_loss_ce', 'head_loss_reg', 'reduce_loss_by', 'ce_weight_sum', 'row_weight_sum', 'gemm'):
            st.enter_context(patched(Lb, name, getattr(tr, name)))
        st.enter_context(patched(Lb, 'reduce_loss', tr.reduce_loss_of(Lb.reduce_loss)))
        st.enter_context(patched(parallel, 'finish_grad_sync', lambda model, in_call, post: tr.calls.append(['finish_grad_sync', in_call, post])))
        st.enter_context(_declared(parallel, state))
        crit = make(nn, models)
        labels = family.endswith('labels')
        Cc = 2 if labels else 1
        t = (LABEL_SPELLINGS if labels else VALUE_SPELLINGS)[spelling](target)
        g = torch.Generator().manual_seed(1)
        res = {}
        try:
            if family.startswith('fusion'):
                owner = FusionOwner(tr, mode == 'train', Cc)
                tf, af = torch.randn(B, HT, generator=g), torch.randn(B, HA, generator=g)
                loss = crit(tf, af, t, owner, **kw)
            else:
                owner = None if mode == 'no_owner' else Owner(tr, mode == 'train')
                z = torch.randn(B, Cc, generator=g)
                loss = crit(nn.Output(z.clone(), owner, z), t, **kw)
            halves = getattr(loss, 'dz_halves', None)
            res['loss'] = {'value': tr.buf(loss._v), 'reduce': bool(loss._reduce), 'backward': loss._bw is not None,
                           'health': loss._health is not None, 'dz': tr.buf(loss.dz),
                           'dz_halves': None if halves is None else [tr.buf(h) for h in halves]}
            if loss._bw is not None:
                loss.backward()
                if family.startswith('fusion'):
                    res['loss']['grad_ready'] = owner._grad_ready
        except Exception as e:  # noqa: BLE001 -- a refused call is part of the record
            res['raises'] = type(e).__name__
    res['calls'] = tr.calls
    res['tensors'] = tr.tensors
    return res


def record_all():
    return {c[0]: record(c) for c in cases()}
