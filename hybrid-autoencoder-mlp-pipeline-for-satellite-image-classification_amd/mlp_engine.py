"""Host side of the external-MLP engine (R.md:2549-2566): flat arenas + C context, mirroring engine.py."""
from __future__ import annotations

import ctypes as C
import weakref

import torch

from . import _lib
from ._lib import check
from .engine import _ptr, _stream, _require_gpu, class_weight_args
from .modules import MLP_HIDDEN, MLP_DROPOUT

_ENGINES = weakref.WeakKeyDictionary()


class MLPEngine:
    """general: None takes the fixed 128 / 64 kernel (eae_mlp_create) exactly when the architecture is the default one, hidden (128, 64)
    with dropout (0.3, 0), and the layer-table kernel (eae_mlp_create_ex) otherwise; True forces the layer-table kernel.
    drop_mask (forward, train_step): None for the kernel's own Philox masks, or one float32 tensor holding the keep masks [B, w_l] of
    the layers with a rate above 0, in layer order, back to back ([B, 128] for the default architecture)."""

    def __init__(self, mlp, max_batch=256, general=None):
        self.lib = _lib.load()
        p0 = next(mlp.parameters())
        self.device = p0.device
        _require_gpu(self.device)
        self.input_dim, self.classes, self.max_batch = mlp.input_dim, mlp.num_classes, int(max_batch)
        self.hidden, self.dropout = tuple(mlp.hidden), tuple(mlp.dropout)
        default = (self.hidden, self.dropout) == (MLP_HIDDEN, MLP_DROPOUT)
        if general is None:
            general = not default
        elif not general and not default:
            raise RuntimeError(f"the fixed kernel serves hidden={MLP_HIDDEN}, dropout={MLP_DROPOUT} only; this MLP has "
                               f"hidden={self.hidden}, dropout={self.dropout}")
        self.general = bool(general)
        nh = len(self.hidden)
        widths = (C.c_int * nh)(*self.hidden)
        poff = (C.c_longlong * (4 * nh + 3))()
        boff = (C.c_longlong * (2 * nh + 1))()
        check(self.lib.eae_mlp_layout_ex(self.input_dim, self.classes, nh, widths, poff, boff))
        self.poff, self.boff = list(poff), list(boff)
        n = self.poff[-1]
        dev = self.device
        self.params = torch.zeros(n, dtype=torch.float32, device=dev)
        self.grads = torch.zeros(n, dtype=torch.float32, device=dev)
        self.adam_m = torch.zeros(n, dtype=torch.float32, device=dev)
        self.adam_v = torch.zeros(n, dtype=torch.float32, device=dev)
        self.bn_running = torch.zeros(self.boff[-1], dtype=torch.float32, device=dev)
        self.bn_nbt = torch.zeros(nh, dtype=torch.int64, device=dev)
        self.stats = torch.zeros(8, dtype=torch.float32, device=dev)
        self.valid = torch.zeros((), dtype=torch.int64, device=dev)
        self.class_weights, self.ignore_index = None, None
        # the Linear / BatchNorm1d modules of mlp.net in order: W, b, gamma, beta per hidden layer, then the last W, b
        linears = [m for m in mlp.net if isinstance(m, torch.nn.Linear)]
        bns = [m for m in mlp.net if isinstance(m, torch.nn.BatchNorm1d)]
        if len(linears) != nh + 1 or len(bns) != nh:
            raise RuntimeError(f"MLP.net holds {len(linears)} Linear and {len(bns)} BatchNorm1d modules; hidden={self.hidden} needs "
                               f"{nh + 1} and {nh}")
        self._slots = []
        for l, (lin, bn) in enumerate(zip(linears, bns)):
            self._slots += [(lin.weight, 4 * l), (lin.bias, 4 * l + 1), (bn.weight, 4 * l + 2), (bn.bias, 4 * l + 3)]
        self._slots += [(linears[-1].weight, 4 * nh), (linears[-1].bias, 4 * nh + 1)]
        self._bn = [(bn, l) for l, bn in enumerate(bns)]
        with torch.no_grad():
            for p, i in self._slots:
                v = self.params[self.poff[i]: self.poff[i] + p.numel()].view(p.shape)
                v.copy_(p.data)
                p.data = v
                p.grad = None
            for bn, l in self._bn:
                c = bn.num_features
                rm = self.bn_running[self.boff[2 * l]: self.boff[2 * l] + c]
                rv = self.bn_running[self.boff[2 * l + 1]: self.boff[2 * l + 1] + c]
                rm.copy_(bn.running_mean)
                rv.copy_(bn.running_var)
                self.bn_nbt[l] = bn.num_batches_tracked.to(dev)
                bn._buffers["running_mean"], bn._buffers["running_var"] = rm, rv
                bn._buffers["num_batches_tracked"] = self.bn_nbt[l]
        h = C.c_void_p()
        if self.general:
            rates = (C.c_float * nh)(*self.dropout)
            check(self.lib.eae_mlp_create_ex(self.input_dim, self.classes, nh, widths, rates, self.max_batch, C.byref(h)))
        else:
            check(self.lib.eae_mlp_create(self.input_dim, self.classes, self.max_batch, C.byref(h)))
        self.ctx = h
        check(self.lib.eae_mlp_bind(self.ctx, _ptr(self.params), _ptr(self.grads), _ptr(self.adam_m), _ptr(self.adam_v),
                                    _ptr(self.bn_running), _ptr(self.bn_nbt)))
        check(self.lib.eae_mlp_set_valid_counter(self.ctx, _ptr(self.valid)))       # written by the kernel while class weights / ignore_index are set
        self._finalizer = weakref.finalize(self, _destroy, self.lib, self.ctx)
        self.seed = int(torch.initial_seed()) & 0xFFFFFFFFFFFFFFFF

    def attached(self):
        base = self.params.data_ptr()
        return all(p.data_ptr() == base + 4 * self.poff[i] for p, i in self._slots) and \
            self._bn[0][0].running_mean.data_ptr() == self.bn_running.data_ptr()

    def _check(self, x, labels=None):
        if x.device != self.device or x.dtype != torch.float32 or x.dim() != 2 or x.shape[1] != self.input_dim:
            raise RuntimeError(f"expected float32 input [B,{self.input_dim}] on {self.device}, got {tuple(x.shape)} {x.dtype} on {x.device}")
        if x.shape[0] > self.max_batch:
            raise RuntimeError(f"batch {x.shape[0]} exceeds the engine's max_batch {self.max_batch}")
        if labels is not None and (labels.dtype != torch.int64 or labels.shape != (x.shape[0],) or labels.device != self.device):
            raise RuntimeError("labels must be int64 [B] on the model's device")
        return x.contiguous(), (None if labels is None else labels.contiguous())

    def set_class_weights(self, weights=None, ignore_index=None):
        """CrossEntropyLoss(weight=weights, ignore_index=ignore_index) in train_step and eval_step (include/eae.h
        eae_mlp_set_class_weights); arguments and the labelled-sample count as for AEEngine.set_class_weights."""
        w, ign = class_weight_args(weights, ignore_index, self.classes, self.device)
        check(self.lib.eae_mlp_set_class_weights(self.ctx, _ptr(w), ign))
        self.class_weights, self.ignore_index = w, (None if ignore_index is None else int(ignore_index))
        self.valid.zero_()          # the count starts with the setting (a reset while the feature is off leaves the word alone)

    @property
    def weighted(self):
        return self.class_weights is not None or self.ignore_index is not None

    def read_valid(self):
        """Number of counted (labelled) samples since reset_stats(), counted by the kernel (accuracy over them: read_stats()[1] *
        read_stats()[2] / read_valid()); with the feature off every sample counts: read_stats()[2].  One D2H sync."""
        if not self.weighted:
            return int(self.stats[1].item())
        return int(self.valid.item())

    def forward(self, x, train=False, drop_mask=None):
        x, _ = self._check(x)
        logits = torch.empty((x.shape[0], self.classes), dtype=torch.float32, device=self.device)
        check(self.lib.eae_mlp_forward(self.ctx, _stream(), _ptr(x), x.shape[0], int(train), self.seed, _ptr(drop_mask), _ptr(logits)))
        return logits

    def train_step(self, x, labels, lr, weight_decay=1e-4, drop_mask=None, want_logits=False):
        """One iteration of R.md:2641-2649; loss*B, B and #correct accumulate in self.stats on the device."""
        x, labels = self._check(x, labels)
        logits = torch.empty((x.shape[0], self.classes), dtype=torch.float32, device=self.device) if want_logits else None
        check(self.lib.eae_mlp_train_step(self.ctx, _stream(), _ptr(x), _ptr(labels), x.shape[0], float(lr), float(weight_decay),
                                          self.seed, _ptr(drop_mask), _ptr(logits), _ptr(self.stats)))
        return logits

    def eval_step(self, x, labels, want_logits=False):
        x, labels = self._check(x, labels)
        logits = torch.empty((x.shape[0], self.classes), dtype=torch.float32, device=self.device) if want_logits else None
        check(self.lib.eae_mlp_eval_step(self.ctx, _stream(), _ptr(x), _ptr(labels), x.shape[0], _ptr(logits), _ptr(self.stats)))
        return logits

    def reset_optimizer(self):
        self.adam_m.zero_()
        self.adam_v.zero_()
        check(self.lib.eae_mlp_set_adam_step(self.ctx, 0))

    def reset_stats(self):
        self.stats.zero_()
        if self.weighted:
            self.valid.zero_()

    def read_stats(self):
        """(mean loss, accuracy, n) since reset_stats(); one D2H sync."""
        s = self.stats.tolist()
        n = max(s[1], 1.0)
        return s[0] / n, s[2] / n, int(s[1])


def _destroy(lib, ctx):
    try:
        lib.eae_mlp_destroy(ctx)
    except Exception:
        pass


def mlp_engine_for(mlp, max_batch=None, general=None):
    """The engine attached to `mlp` (built on first use; rebuilt for a bigger max_batch, another device or another kernel choice).
    general: as for MLPEngine; None keeps whatever kernel an attached engine runs."""
    eng = _ENGINES.get(mlp)
    dev = next(mlp.parameters()).device
    _require_gpu(dev)
    want = max_batch or 256
    old = None
    if eng is not None and (not eng.attached() or eng.device != dev or eng.max_batch < want
                            or (general is not None and bool(general) != eng.general)):
        old, eng = eng, None
    if eng is None:
        if general is None and old is not None:
            general = old.general                   # a rebuild for a bigger workspace or another device keeps the kernel choice
        eng = MLPEngine(mlp, max_batch=want, general=general)
        if old is not None and old.device == dev and (old.class_weights is not None or old.ignore_index is not None):
            eng.set_class_weights(old.class_weights, old.ignore_index)      # the criterion's setting survives a bigger workspace
        _ENGINES[mlp] = eng
    return eng


class _MLPFunction(torch.autograd.Function):
    """Autograd bridge for the reference's own MLP loop (`logits = clf(xb)` ... `loss.backward()`, R.md:2643-2645)."""

    @staticmethod
    def forward(ctx, eng, x, *params):
        x = x.contiguous()
        eng._autograd_calls = getattr(eng, "_autograd_calls", 0) + 1
        seed = (eng.seed + eng._autograd_calls) & 0xFFFFFFFFFFFFFFFF      # fresh dropout mask per forward call
        logits = torch.empty((x.shape[0], eng.classes), dtype=torch.float32, device=eng.device)
        check(eng.lib.eae_mlp_forward(eng.ctx, _stream(), _ptr(x), x.shape[0], 1, seed, None, _ptr(logits)))
        ctx.eng, ctx.seed = eng, seed
        ctx.save_for_backward(x)
        ctx.need = [p.requires_grad for p in params]
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        eng = ctx.eng
        (x,) = ctx.saved_tensors
        dlogits = dlogits.to(torch.float32).contiguous()
        check(eng.lib.eae_mlp_backward(eng.ctx, _stream(), _ptr(x), x.shape[0], ctx.seed, None, _ptr(dlogits)))
        grads = [eng.grads[eng.poff[i]: eng.poff[i] + p.numel()].view(p.shape).clone() if need else None
                 for (p, i), need in zip(eng._slots, ctx.need)]
        return (None, None, *grads)


def mlp_forward(module, x):
    eng = mlp_engine_for(module, max_batch=max(256, x.shape[0]))
    if torch.is_grad_enabled() and any(p.requires_grad for p in module.parameters()):
        if not module.training:
            raise RuntimeError("differentiating through an eval-mode MLP is not supported by the HIP engine; call clf.train() "
                               "or use torch.no_grad()")
        eng._check(x)
        return _MLPFunction.apply(eng, x, *[p for p, _ in eng._slots])
    return eng.forward(x, train=module.training)
