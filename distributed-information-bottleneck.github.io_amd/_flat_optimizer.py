"""FlatOptimizer: the optimizer state over ONE flat parameter buffer (the slots of include/dib_optimizers.h, step count, learning
rate, bound rule) and the launches that read and write it: HipEngine, DenseStack, the measurement models and the circuit models
each hold one.  The parameters and gradients
are the caller's: every step takes them as arguments (MeasurementIB rebinds its stacks' buffers to views of one allocation)."""
from __future__ import annotations

from ctypes import byref
from typing import Optional

import torch

from . import _lib
from ._lib import check
from .grad_transform import _ptr, eval_lr


def _hyper(opt) -> "_lib.OptimizerHyper":
    return _lib.OptimizerHyper(**opt.hyper())


def _key(opt):
    """the rule: kind and hyper-parameters, not the learning rate or the clip / decay settings; None: Adam / plain SGD"""
    return None if opt is None or opt.native else (opt.kind, tuple(sorted(opt.hyper().items())))


class FlatOptimizer:
    def __init__(self, lib, stream, n_alloc: int, device, learning_rate: float = 1e-3, m=None, v=None):
        """m, v: the caller's own zeroed tensors of n_alloc floats (views of a larger allocation) in place of fresh ones; every
        method, reset() and bind() included, works on them where they lie"""
        self.lib, self._stream = lib, stream
        self.m, self.v = (t if t is not None else torch.zeros(n_alloc, dtype=torch.float32, device=device) for t in (m, v))
        self.s2: Optional[torch.Tensor] = None        # third slot (AMSGrad's vhat, RMSprop centred with momentum)
        self.scalar: Optional[torch.Tensor] = None    # Nadam's running product P of its momentum schedule: one float64
        self.t_dev = torch.zeros(1, dtype=torch.int64, device=device)
        self.lr_dev = torch.full((1,), learning_rate, dtype=torch.float32, device=device)
        self._lr_host: Optional[float] = learning_rate   # what lr_dev holds if only set_lr wrote it; None: a schedule did
        self.opt = None                               # the bound rule of include/dib_optimizers.h; None: Adam / plain SGD
        self._sync: Optional[torch.Tensor] = None     # dib_reduce_adam_step's grid-sync words, allocated by its first call

    def _slots(self, opt):
        n = opt.slots()
        if n > 2 and self.s2 is None:
            self.s2 = torch.zeros_like(self.m)
        return [b if k < n else None for k, b in enumerate((self.m, self.v, self.s2))]

    def _scalar(self, opt):
        if opt.name == "nadam" and self.scalar is None:
            self.scalar = torch.ones(1, dtype=torch.float64, device=self.m.device)
        return self.scalar if opt.name == "nadam" else None

    def bind(self, opt) -> None:
        """Bind an optimizers.Optimizer: the buffers change meaning with the rule, so a CHANGE of rule (_key) re-initialises them
        and the step count.  Binding the rule already bound is free; Adam and momentum-free SGD are the initial binding."""
        key = _key(opt)
        if key != _key(self.opt):
            self.opt = None if key is None else opt
            self.reset()

    def reset(self) -> None:
        """the state before the first step: zeros for Adam / plain SGD, else dib_optimizer_init over the whole allocation; t = 0"""
        opt = self.opt
        if opt is None:
            self.m.zero_()
            self.v.zero_()
        else:
            check(self.lib.dib_optimizer_init(opt.kind, byref(_hyper(opt)), *(_ptr(b) for b in self._slots(opt)), self.m.numel(),
                                              _ptr(self._scalar(opt)), self._stream()), "dib_optimizer_init")
        self.t_dev.zero_()

    def set_lr(self, v: float) -> None:
        """device learning rate; a repeated value costs nothing (fit sets it every step: a 4 us fill kernel otherwise)"""
        if self._lr_host != float(v):
            self.lr_dev.fill_(float(v))
            self._lr_host = float(v)

    def take_state(self, other: "FlatOptimizer", elements: slice = slice(None)) -> None:
        """m and v <- those `elements` of another instance's, with its step count and learning rate (a replica leaving an
        ensemble); the learning rate arrives behind set_lr's back, so its host cache is void"""
        self.m.copy_(other.m[elements])
        self.v.copy_(other.v[elements])
        self.t_dev.copy_(other.t_dev)
        self.lr_dev.copy_(other.lr_dev)
        self._lr_host = None

    def eval_lr(self, descriptor: dict) -> None:
        """lr_dev <- the schedule (fields of dib_lr_schedule) at the device step count, in a one-thread launch"""
        eval_lr(self.lib, descriptor, self.t_dev, self.lr_dev, self._stream())
        self._lr_host = None

    def step_range(self, opt, params, grads, offset: int, count: int, grad_scale: float = 1.0) -> None:
        """the rule on the elements [offset, offset + count) of the flat buffers: one launch, reads t and P, writes neither"""
        sl = lambda b: None if b is None else b[offset:]
        check(self.lib.dib_optimizer_step(opt.kind, byref(_hyper(opt)), _ptr(sl(params)), _ptr(sl(grads)),
                                          *(_ptr(sl(b)) for b in self._slots(opt)), int(count), _ptr(self.lr_dev),
                                          _ptr(self.t_dev), _ptr(self._scalar(opt)), float(grad_scale), self._stream()),
              "dib_optimizer_step")

    def advance(self, opt) -> None:
        """ends a step of the rule: t += 1 (and Nadam's P) in a one-thread launch, after every range has been stepped"""
        check(self.lib.dib_optimizer_advance(opt.kind, byref(_hyper(opt)), _ptr(self.t_dev), _ptr(self._scalar(opt)),
                                             self._stream()), "dib_optimizer_advance")

    def adam(self, params, grads, n: int, beta1=0.9, beta2=0.999, eps=1e-7, grad_scale=1.0, stream=None) -> None:
        """stream: the launch stream a step already asked for (asking torch again costs about a microsecond)"""
        check(self.lib.dib_adam_step(_ptr(params), _ptr(grads), _ptr(self.m), _ptr(self.v), n, _ptr(self.lr_dev),
                                     _ptr(self.t_dev), beta1, beta2, eps, float(grad_scale),
                                     stream if stream is not None else self._stream()), "dib_adam_step")

    def sgd(self, params, grads, n: int, grad_scale=1.0) -> None:
        check(self.lib.dib_sgd_step(_ptr(params), _ptr(grads), n, _ptr(self.lr_dev), float(grad_scale), self._stream()),
              "dib_sgd_step")

    def reduce_adam(self, slabs, nsplit: int, params, grads, n: int, beta1=0.9, beta2=0.999, eps=1e-7, stream=None) -> None:
        """one launch: grads <- the fixed-order sum of `nsplit` slabs of n floats (none: grads as they are), Keras-Adam, t += 1
        (stream: as in adam)"""
        if self._sync is None:
            self._sync = torch.zeros(_lib.SYNC_WORDS, dtype=torch.int32, device=self.m.device)
        check(self.lib.dib_reduce_adam_step(_ptr(slabs), nsplit, n, _ptr(params), _ptr(grads),
                                            _ptr(self.m), _ptr(self.v), n, _ptr(self.lr_dev), _ptr(self.t_dev), beta1, beta2,
                                            eps, 1.0, _ptr(self._sync), stream if stream is not None else self._stream()),
              "dib_reduce_adam_step")


class HoldsFlatOptimizer:
    """For a class with a FlatOptimizer in `self.opt_state`: the names its state has always had, and the plain delegations.
    The circuit and measurement models take the names and set_lr from it; their steps always launch Adam, so a rule bound with
    set_optimizer is not something those steps honour."""
    adam_m = property(lambda self: self.opt_state.m, lambda self, t: setattr(self.opt_state, "m", t))
    adam_v = property(lambda self: self.opt_state.v, lambda self, t: setattr(self.opt_state, "v", t))
    opt_s2 = property(lambda self: self.opt_state.s2)
    opt_scalar = property(lambda self: self.opt_state.scalar)
    t_dev = property(lambda self: self.opt_state.t_dev)
    lr_dev = property(lambda self: self.opt_state.lr_dev)

    def set_optimizer(self, opt) -> None:
        """bind the rule of `opt`: a change of rule re-initialises the state and the step count (FlatOptimizer.bind)"""
        self.opt_state.bind(opt)

    def reset_optimizer(self) -> None:
        self.opt_state.reset()

    def set_lr(self, v: float) -> None:
        self.opt_state.set_lr(v)

    def apply_lr_descriptor(self, descriptor: dict) -> None:
        """lr_dev <- the schedule (fields of dib_lr_schedule) at the device step count; the host cache of set_lr is void after it"""
        self.opt_state.eval_lr(descriptor)
