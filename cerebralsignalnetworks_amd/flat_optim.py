"""Fused optimiser steps over the flat buffers of ``trainer.FlatGrads(..., flatten_params=True)``: AdamW / Adam
(LstmDistillFromDinoV2TrainSpampinato.py:378, LSTMDistill.py:322, LstmDistillation.py:141-150 with the DINO per-tensor
clip) and LARS (EEG-BarlowNetworks/optim.py) as one to three HIP launches per step over the whole model
(csrc/optim.hip) instead of torch's multi-tensor kernels, with the interface of ``trainer.FlatRMSprop``: ``step()``,
``zero_grad()``, one ``param_groups`` dict that schedulers write, ``state_dict()`` / ``load_state_dict()``.

Every parameter of the flat buffer is stepped on every call (its gradient is a view into the flat gradient buffer and
always exists): there is no ``grad is None`` skip."""
import torch

from . import cabi


def segment_ends(flat):
    """Exclusive end offset of every tensor of a FlatGrads inside its flat buffers."""
    ends, off = [], 0
    for p in flat.params:
        off += p.numel()
        ends.append(off)
    return ends


def adam_segment_flags(params, no_decay=None, clip=None):
    """Per-tensor flags of FlatAdamW: weight decay everywhere but on the tensors listed in ``no_decay`` (compared by
    identity); with ``clip`` every tensor is clipped."""
    skip = {id(p) for p in (no_decay or ())}
    scaled = cabi.SEG_SCALED if clip else 0
    return [(0 if id(p) in skip else cabi.SEG_DECAYED) | scaled for p in params]


def lars_segment_flags(params, weight_decay_filter=False, lars_adaptation_filter=False):
    """Per-tensor flags of FlatLARS: the two filters of the reference's LARS exempt 1-D tensors (biases, norm scales)
    from the decay / from the trust-ratio scaling."""
    return [(0 if (weight_decay_filter and p.ndim == 1) else cabi.SEG_DECAYED) |
            (0 if (lars_adaptation_filter and p.ndim == 1) else cabi.SEG_SCALED) for p in params]


def _plain(v):
    """A hyper-parameter as plain Python: numpy scalars become float / int / bool, tuples element by element."""
    if isinstance(v, (tuple, list)):
        return type(v)(_plain(x) for x in v)
    if type(v) in (bool, int, float, str) or v is None:        # (numpy.float64 is a float subclass: exact types only)
        return v
    return v.item() if hasattr(v, "item") else v


def check_max_grad_norm(max_grad_norm):
    """None (off) or a number > 0 (inf: measure and gate only), as csn_grad_guard accepts it."""
    if max_grad_norm is None:
        return None
    if isinstance(max_grad_norm, bool) or not float(max_grad_norm) > 0.0:          # (False for NaN)
        raise ValueError(f"max_grad_norm must be None or > 0, got {max_grad_norm!r}")
    return max_grad_norm


def guard_restatement(grads, max_norm=None):
    """csn_grad_guard restated in torch (any device): ``(norm, scale, finite)`` as 0-dim tensors -- the float64 sum of
    squares S, norm = float32(sqrt S), scale = float32(min(1, max_norm / (sqrt S + 1e-6))) where S is finite and 0 where it
    is not; ``max_norm`` None: infinite (scale 1 or 0).  What DistillTrainer steps with on CPU buffers, and the oracle of
    the device record's tests."""
    s = grads.detach().double().pow(2).sum()
    finite = torch.isfinite(s)
    root = s.sqrt()
    coef = torch.clamp((float("inf") if max_norm is None else float(max_norm)) / (root + 1e-6), max=1.0)
    return root.float(), torch.where(finite, coef, torch.zeros_like(coef)).float(), finite


class StepGuarded:
    """``max_grad_norm`` / ``skip_nonfinite`` of the flat optimisers.  With either set, ``step()``
    enqueues csn_grad_guard over the flat gradient buffer -- the global L2 norm, the coefficient of
    ``torch.nn.utils.clip_grad_norm_`` and a finiteness flag, left in a 16-byte device record -- and then the GUARDED step,
    which reads scale * g wherever the plain step reads g and writes NOTHING (parameters and state keep their bits) when
    the gradient holds a NaN or an Inf: the step that ``fp16_scaler.step(optimizer)`` would not take
    (LstmDistillation.py:606-613).  No host read: ``last_grad_norm`` is a 0-dim device tensor (the pre-clip norm of the
    last step), ``skipped_steps()`` the one blocking read.  The gradient buffer is never written.

    ``max_grad_norm`` lives in ``param_groups[0]`` and is read on every step, like ``lr``; None there means "measure and
    gate only".  A non-finite gradient is skipped whenever the guard is on, ALSO with a finite ``max_grad_norm`` and
    ``skip_nonfinite=False``: its coefficient is 0, and 0 * Inf would write NaN into every parameter.  ``skip_nonfinite``
    itself only decides whether DistillTrainer's status check tolerates such steps or reports the run as diverged.
    The guard cannot be switched on after construction (``step()`` raises); with both options off nothing changes: the
    same launches, the same bits, the same ``state_dict`` keys."""

    guard = None
    skip_nonfinite = False
    last_grad_norm = None

    def _init_guard(self, max_grad_norm, skip_nonfinite):
        check_max_grad_norm(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        if max_grad_norm is not None or self.skip_nonfinite:
            self.guard = cabi.StepGuard(self.flat.flat.device)
            self.last_grad_norm = self.guard.norm
            self.param_groups[0]["max_grad_norm"] = max_grad_norm

    def _measure(self):
        """The measured guard of this step, or None when the guard is off."""
        max_norm = self.param_groups[0].get("max_grad_norm")
        if self.guard is None:
            if max_norm is not None:
                raise ValueError(f"{type(self).__name__}: max_grad_norm can be changed through param_groups, not switched "
                                 "on: build the optimiser with max_grad_norm= or skip_nonfinite=")
            return None
        self.guard.measure(self.flat.flat, check_max_grad_norm(max_norm))
        return self.guard

    def skipped_steps(self):
        """Steps not taken because the gradient was non-finite (one blocking host read; 0 with the guard off)."""
        return self.guard.skipped() if self.guard is not None else 0

    def _guard_state(self, sd):
        if self.guard is not None:
            sd.update(max_grad_norm=_plain(self.param_groups[0]["max_grad_norm"]), skip_nonfinite=self.skip_nonfinite,
                      skipped=self.guard.skipped())
        return sd

    def _guard_load(self, sd):
        if self.guard is not None and "skipped" in sd:
            self.guard.set_skipped(sd["skipped"])
            self.param_groups[0]["max_grad_norm"] = sd["max_grad_norm"]


class _FlatOptimizer(StepGuarded):
    """What the fused optimisers share: the FlatGrads, its segment table, the re-homing check and zero_grad."""

    def __init__(self, flat, flags, defaults, max_grad_norm=None, skip_nonfinite=False):
        if flat.flat_params is None:
            raise ValueError(f"{type(self).__name__} needs FlatGrads(..., flatten_params=True)")
        if not flat.flat.is_cuda:
            raise cabi.CsnError(f"{type(self).__name__}: libcsn_hip needs device tensors (no CPU fallback)")
        self.flat = flat
        self.flags = list(flags)
        self.table = cabi.SegmentTable(segment_ends(flat), self.flags, flat.flat.device)
        self.param_groups = [dict(defaults, params=flat.params)]
        self._init_guard(max_grad_norm, skip_nonfinite)

    def check_views(self):
        """The parameters must still BE the views into the flat buffer this optimiser steps (model.float() / .to(dtype)
        / load_state_dict(assign=True) after construction re-home them and the model would silently stop training)."""
        base, off = self.flat.flat_params.data_ptr(), 0
        for p in self.flat.params:
            if p.data_ptr() != base + 4 * off:
                raise RuntimeError(f"{type(self).__name__}: a parameter no longer lives in the flat buffer (re-homed after "
                                   "the trainer was built); rebuild the trainer")
            off += p.numel()

    def zero_grad(self, set_to_none=False):
        self.flat.zero()

    def _state(self, tensors):
        # schedulers write numpy scalars (dino.cosine_scheduler): saved as plain Python numbers, same value, so that
        # the checkpoint loads with torch.load(weights_only=True)
        sd = {k: _plain(v) for k, v in self.param_groups[0].items() if k != "params"}
        sd.update(tensors)
        sd["flags"] = list(self.flags)
        return self._guard_state(sd) if getattr(self, "guard", None) is not None else sd

    def _load(self, sd, tensors):
        if list(sd["flags"]) != self.flags:        # (which tensors decay / are scaled is part of the state)
            self.flags = list(sd["flags"])
            self.table = cabi.SegmentTable(segment_ends(self.flat), self.flags, self.flat.flat.device)
        for name in tensors:
            getattr(self, name).copy_(sd[name])
        for k in self.param_groups[0]:
            if k not in ("params", "max_grad_norm"):
                self.param_groups[0][k] = sd[k]
        self._guard_load(sd)


class FlatAdamW(_FlatOptimizer):
    """``torch.optim.AdamW`` (``decoupled=False``: ``torch.optim.Adam``, L2 decay added to the gradient) as ONE fused
    HIP pass over the flat parameter / gradient / moment buffers (csn_adam_step), with torch's single-tensor arithmetic.
    ``no_decay``: parameters with weight decay 0 (the ``not_reg`` group of the DINO CLI / ``get_params_groups``).
    ``clip``: the DINO per-tensor gradient clip (utils/utils.py:132-141) fused in front -- a norm pass (two launches), then
    the step scales each tensor's gradient on the fly; the gradient buffer itself is left as it was, and
    ``last_grad_norms`` is the device tensor of the pre-clip norms (no host round trip).
    ``param_groups[0]`` (lr, betas, eps, weight_decay, clip) is read on every step; a ``clip`` given at construction can
    be changed or set to None there, one that was not given cannot be switched on later (``step()`` raises).
    ``max_grad_norm`` / ``skip_nonfinite``: the global-norm clip and the non-finite skip of ``StepGuarded`` (csn_grad_guard
    + csn_adam_step_guarded, two launches more).  With ``clip`` as well the two compose in sequence: the global clip first,
    then the per-tensor clip of the scaled gradient (``last_grad_norms`` are then the norms of the SCALED gradient, and a
    skipped step leaves them as they were).  ``steps`` -- the t of the bias corrections -- counts every ``step()`` call,
    skipped ones included: counting only the steps taken would need a host read of the record."""

    def __init__(self, flat, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, decoupled=True, no_decay=None,
                 clip=None, max_grad_norm=None, skip_nonfinite=False):
        flags = adam_segment_flags(flat.params, no_decay, clip)
        super().__init__(flat, flags, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, clip=clip),
                         max_grad_norm, skip_nonfinite)
        self.decoupled = bool(decoupled)
        self.exp_avg = torch.zeros_like(flat.flat)
        self.exp_avg_sq = torch.zeros_like(flat.flat)
        self.steps = 0
        self.last_grad_norms = torch.zeros(len(flags), dtype=torch.float32, device=flat.flat.device) if clip else None

    @torch.no_grad()
    def step(self):
        self.check_views()
        g = self.param_groups[0]
        if g["clip"] and self.last_grad_norms is None:
            raise ValueError("FlatAdamW: clip can be changed or switched off through param_groups, not switched on: "
                             "build the optimiser with clip= (the segments carry the flag)")
        clip = g["clip"] if self.last_grad_norms is not None else None
        guard = self._measure()
        args = (self.table, self.flat.flat_params, self.flat.flat, self.exp_avg, self.exp_avg_sq, self.steps + 1, g["lr"],
                g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"], self.decoupled, clip,
                self.last_grad_norms if clip else None)
        if guard is None:
            cabi.adam_step(*args)
        else:
            cabi.adam_step_guarded(guard, *args)
        self.steps += 1

    def state_dict(self):
        return self._state({"exp_avg": self.exp_avg, "exp_avg_sq": self.exp_avg_sq, "step": self.steps,
                            "decoupled": self.decoupled})

    def load_state_dict(self, sd):
        self._load(sd, ("exp_avg", "exp_avg_sq"))
        self.steps, self.decoupled = int(sd["step"]), bool(sd["decoupled"])
        if sd["clip"] and self.last_grad_norms is None:
            self.last_grad_norms = torch.zeros(len(self.flags), dtype=torch.float32, device=self.flat.flat.device)
        elif not sd["clip"]:
            self.last_grad_norms = None


class FlatLARS(_FlatOptimizer):
    """``losses.LARS`` (EEG-BarlowNetworks/optim.py:5-44) as a norm pass and ONE fused update over the flat buffers
    (csn_lars_step: three launches) instead of about ten multi-tensor launches and a gradient clone per parameter.
    ``param_groups[0]`` (lr, weight_decay, momentum, eta) is read on every step.
    ``max_grad_norm`` / ``skip_nonfinite``: the global-norm clip and the non-finite skip of ``StepGuarded`` (csn_grad_guard
    + csn_lars_step_guarded: the trust ratios are those of the scaled gradient)."""

    def __init__(self, flat, lr, weight_decay=0, momentum=0.9, eta=0.001, weight_decay_filter=False,
                 lars_adaptation_filter=False, max_grad_norm=None, skip_nonfinite=False):
        flags = lars_segment_flags(flat.params, weight_decay_filter, lars_adaptation_filter)
        super().__init__(flat, flags, dict(lr=lr, weight_decay=weight_decay, momentum=momentum, eta=eta,
                                           weight_decay_filter=weight_decay_filter,
                                           lars_adaptation_filter=lars_adaptation_filter), max_grad_norm, skip_nonfinite)
        self.mu = torch.zeros_like(flat.flat)

    @torch.no_grad()
    def step(self):
        self.check_views()
        g = self.param_groups[0]
        guard = self._measure()
        args = (self.table, self.flat.flat_params, self.flat.flat, self.mu, g["lr"], g["weight_decay"], g["momentum"], g["eta"])
        if guard is None:
            cabi.lars_step(*args)
        else:
            cabi.lars_step_guarded(guard, *args)

    def state_dict(self):
        return self._state({"mu": self.mu})

    def load_state_dict(self, sd):
        self._load(sd, ("mu",))


def flat_clip_gradients(flat, clip):
    """``runtime.clip_gradients`` on the flat gradient buffer of a FlatGrads: every tensor's gradient whose L2 norm
    exceeds ``clip`` is scaled to it, in place, in three launches; returns the pre-clip norms as a DEVICE tensor (one per
    tensor, in ``flat.params`` order) -- nothing is copied to the host.  The segment table is built on the first call
    and kept on ``flat``."""
    if not flat.flat.is_cuda:
        raise cabi.CsnError("flat_clip_gradients: libcsn_hip needs device tensors (no CPU fallback)")
    table = flat.clip_table
    if table is None:
        table = flat.clip_table = cabi.SegmentTable(segment_ends(flat), [cabi.SEG_SCALED] * len(flat.params),
                                                     flat.flat.device)
    return cabi.flat_clip(table, flat.flat, clip)


def flat_clip_grad_norm_(flat, max_norm):
    """``torch.nn.utils.clip_grad_norm_(params, max_norm)`` on the flat gradient buffer of a FlatGrads, in place, for an
    optimiser that reads the gradients itself (the torch ones): csn_grad_guard (two launches), then one multiply of the
    buffer by the DEVICE coefficient.  Returns the pre-clip global norm as a 0-dim device tensor; nothing is copied to the
    host.  As with ``error_if_nonfinite=False`` a non-finite buffer stays non-finite (its coefficient is 0, and
    0 * Inf = NaN): skipping such a step takes a flat optimiser (``skip_nonfinite``).  The record is kept on ``flat``."""
    if not flat.flat.is_cuda:
        raise cabi.CsnError("flat_clip_grad_norm_: libcsn_hip needs device tensors (no CPU fallback)")
    if check_max_grad_norm(max_norm) is None:
        raise ValueError("flat_clip_grad_norm_: max_norm must be > 0")
    if flat.step_guard is None:
        flat.step_guard = cabi.StepGuard(flat.flat.device)
    flat.step_guard.measure(flat.flat, max_norm)
    flat.flat.mul_(flat.step_guard.scale)
    return flat.step_guard.norm
