"""Host mirror of the reference's LSTM encoders, running on the HIP kernels.

``Model`` fills the place of the reference's missing ``models/lstm.py`` (imported at
/root/reference/LstmDistillFromDinoV2Train.py:5, constructed at :323,
LstmDistillFromDinoV2TrainSpampinato.py:368, LstmDistillFromDinoV2Eval.py:308) with the
call-site contract of SURVEY.md section 8(b): ``Model(input_size, lstm_size, lstm_layers, output_size,
include_top)``; ``forward(x[B,T,C]) -> [B,output_size]`` or ``([B,output_size],
[B,n_classes])``.  Parameter names and layouts follow the in-tree precedent
(/root/reference/LSTMDistill.py:118-120): ``lstm.{weight_ih,weight_hh,bias_ih,bias_hh}_l{k}``,
``fc.*``, ``class_pred.*`` -- checkpoints round-trip with a stock ``nn.LSTM``.
"""
import warnings

import torch
import torch.nn as nn

from . import cabi


class _Lease:
    """Holds a plan (= its workspace) for one autograd node.  Released by the node's backward -- or, when the
    graph is dropped without a backward (a skipped step, a validation pass without no_grad, an exception between
    forward and backward), when the node itself is collected, so such a forward never pins a workspace for good."""

    def __init__(self, plan):
        self.plan = plan
        plan.busy = True

    def release(self):
        if self.plan is not None:
            self.plan.busy = False
            self.plan = None

    __del__ = release


class _PlanPool(dict):
    """key -> list of plans; plan.busy marks a forward awaiting its backward.  Workspaces are large (10 GB at cfg2), so
    only a few idle ones are kept."""

    def checkout(self, key, make, max_idle):
        """-> an idle plan of ``key``, or make() after dropping idle plans of OTHER keys, oldest first, while at least
        ``max_idle`` of them are idle.  A busy plan and a plan of ``key`` are never dropped."""
        plans = self.setdefault(key, [])
        for plan in plans:
            if not plan.busy:
                return plan
        idle = [(k, pl) for k, lst in self.items() for pl in lst if not pl.busy and k != key]
        while len(idle) >= max_idle:
            k, pl = idle.pop(0)
            self[k].remove(pl)
        plans.append(make())
        return plans[-1]

    def all(self):
        return [pl for lst in self.values() for pl in lst]


class _Call:
    """What one forward asks of its plan(s).  Kept on ctx: the backward runs with the lengths and dropout of its forward.
    ``B, T``: the plan's shape -- x's, or with ``views = (rows, starts)`` (x is then the source) the windows'.  ``drop``:
    _draw_dropout's.  ``outputs``: which of (y_last, y_all, h_n, c_n) the entry point takes -- the library is asked for no
    other, and only their gradients go to plan.backward.  ``state_plan``: HipLSTM._checkout's ``state``.  ``overwrite``: is
    ``direct_grads = True`` honoured?  ``bi``: BiLSTM's (L, H).  ``readout``: what y_last is -- "last", "mean" or "max" over
    each row's valid steps (csn_lstm_plan_set_readout); BiLSTM's top-layer plans then hand back their pooled halves.
    "attn": the attention readout (csn_lstm_plan_set_attention) with ``attn``, the query of each direction ([H] float32
    parameters: one, or BiLSTM's two); ``want_weights``: the forward also fills ``attn_out``, one [B, T] float32 tensor of
    attention weights per direction (the backward writes the same bits into them again)."""
    __slots__ = ("B", "T", "training", "drop", "lengths", "views", "outputs", "state_plan", "overwrite", "bi", "readout", "attn",
                 "want_weights", "attn_out")

    def __init__(self, x, training, drop, lengths=None, views=None, outputs=(True, False, False, False), state_plan=None,
                 overwrite=True, bi=None, readout="last", attn=None, want_weights=False):
        self.readout = _check_readout("LSTM call", readout)
        self.attn = tuple(attn) if readout == "attn" and attn is not None else None
        if readout == "attn" and (self.attn is None or len(self.attn) != (1 if bi is None else 2)):
            raise ValueError("LSTM call: the attention readout needs one query per direction")
        self.want_weights, self.attn_out = bool(want_weights) and self.attn is not None, None
        self.B, self.T = (x.shape[0], x.shape[1]) if views is None else (len(lengths), max(1, max(lengths)))
        self.training, self.drop, self.lengths, self.views = training, drop, lengths, views
        self.outputs, self.state_plan, self.overwrite, self.bi = outputs, state_plan, overwrite, bi

    def weights(self):
        """The attention weights of the call's forward, detached: [B, T], or [B, T, 2] for the two directions."""
        return self.attn_out[0] if len(self.attn_out) == 1 else torch.stack(self.attn_out, dim=2)


def _armed(plan, call, fn, grad=None, k=None, src=None, dq=None):
    """fn() -- ``call``'s plan.forward or plan.backward -- with everything it depends on set on the plan first.  Plans are
    shared between calls and every setter of cabi.LstmPlan is sticky, so a pooled plan still carries whatever its last
    user set: nothing is assumed, all of it is set in front of every forward and backward.  That is: the readout (on
    BiLSTM's plans below the top layer always "last": their y_last is not used) and the attention readout -- the query of
    the plan's direction, the call's weights tensor and, on a backward, ``dq`` (where the query's gradient goes) on the top
    plan(s) of an "attn" call, off on every other plan and call; the lengths (None =
    every row is T; on CSN_LSTM_STATE plans only, the library refuses set_lengths on others); on a stack's plan the
    inter-layer dropout (None = p 0, which a plan without the bit takes too); on BiLSTM's plan ``k`` = 2 * layer +
    direction the io pitches -- on a backward the reverse direction adds its dx to the forward one's -- and the output
    dropout of its half of the [B,T,2H] interface (one Philox stream per call covers the concatenated interfaces, as torch
    drops each once; the top layer's is never dropped); on a backward ``grad`` = (callback, accumulate).  ``src``: the
    source tensor of a forward through input windows, which are cleared again, also when fn raises -- a backward reads no
    x, so it sets none."""
    top = k is None or k // 2 == call.bi[0] - 1
    attn = top and call.readout == "attn"
    plan.set_readout(call.readout if top and not attn else "last")
    if attn:
        d = 0 if k is None else k % 2
        plan.set_attention(call.attn[d], None, dq, None if call.attn_out is None else call.attn_out[d])
    else:
        plan.set_attention()
    if plan.state:
        plan.set_lengths(call.lengths)
    if k is None:
        plan.set_dropout(*(call.drop or (0.0,)))
    else:
        (L, H), l, d = call.bi, k // 2, k % 2
        plan.set_io(2 * H, 2 * H, grad is not None and d == 1)
        if call.drop is None or l >= L - 1:
            plan.set_output_dropout(0.0)
        else:
            plan.set_output_dropout(*call.drop, first=l * call.B * call.T * 2 * H + d * H, index_pitch=2 * H)
    if grad is not None:
        plan.set_grad_callback(grad[0])
        plan.set_grad_mode(grad[1])
    if src is None:
        return fn()
    plan.set_views(call.views[0], call.views[1], src.shape[0], src.shape[1])
    try:
        return fn()
    finally:
        plan.set_views(None)


def _refuse_second_backward(owner, leases):
    if not leases or leases[0].plan is None:
        raise RuntimeError(f"{type(owner).__name__}: second backward through one forward -- its workspace was handed back "
                           "after the first (retain_graph / double backward are not supported)")


def _direct_grads(owner, params, overwrite=True):
    """-> (direct, accumulate): does this backward write into the parameters' .grad, and does it add to them?
    ``owner.direct_grads``: False = temporaries handed to autograd; True = the library OVERWRITES .grad -- valid while this
    is the only forward of the step that uses these parameters, so a caller whose forwards are chained through their state
    passes ``overwrite=False`` and gets temporaries; "accumulate" = it adds (CSN_GRAD_ACCUMULATE: the bits of autograd's
    p.grad += g), for any number of forwards between two zeroings of the buffer."""
    mode = owner.direct_grads
    accumulate = mode == "accumulate"
    if not mode or not (accumulate or overwrite) or not all(p.grad is not None and p.grad.is_contiguous() and
                                                            p.grad.dtype == torch.float32 for p in params):
        return False, False
    return True, accumulate


def _grad_targets(params, direct):
    """Where a backward writes the parameter gradients: straight into the parameters' .grad (the views into the trainer's
    flat buffer: no temporaries, no accumulation pass), or into temporaries handed to autograd."""
    return [p.grad for p in params] if direct else [torch.empty_like(p) for p in params]


def _training(x, h0, c0, params):
    """Is a backward coming?  (Grad mode is off inside Function.forward, so it is decided by the entry point.)"""
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, h0, c0, *params))


def _dropout_p(owner):
    """``owner.dropout`` as it is now (the attribute may have been assigned since construction): a float in [0, 1]."""
    return _check_dropout_p(owner.dropout)


def _check_dropout_p(p):
    if isinstance(p, bool) or not isinstance(p, (int, float)) or not 0 <= p <= 1:
        raise ValueError(f"dropout should be a number in range [0, 1] representing the probability of an element being "
                         f"zeroed, got {p!r}")
    return float(p)


def _check_readout(name, readout):
    """``readout``: which summary of the top layer's output sequence a module hands back -- "last" (each row's last valid
    step), "mean" / "max" over each row's valid steps, reduced inside the library (csn_lstm_plan_set_readout), or "attn":
    their weighted mean under a learned query (csn_lstm_plan_set_attention; the module owns ``attn_query``)."""
    if not isinstance(readout, str) or (readout not in cabi.READOUTS and readout != "attn"):
        raise ValueError(f"{name}: readout must be one of {sorted([*cabi.READOUTS, 'attn'])}, got {readout!r}")
    return readout


def _attn_queries(module, name):
    """The attention queries a module owns, one per direction -- or ValueError: it was built without them."""
    qs = [getattr(module, n, None) for n in (("attn_query", "attn_query_reverse") if getattr(module, "bidirectional", False) else ("attn_query",))]
    if any(q is None for q in qs):
        raise ValueError(f'{name}: readout="attn" on a module built without the attention parameter (attention=True)')
    return qs


def _check_resident(name, resident, hidden_size):
    """``resident=True`` (CSN_LSTM_RESIDENT plans: the CU-resident recurrence, path 5) takes hidden sizes up to 128."""
    if resident and hidden_size > cabi.RESIDENT_MAX_H:
        raise ValueError(f"{name}: resident=True takes hidden_size <= {cabi.RESIDENT_MAX_H}, got {hidden_size}")
    return bool(resident)


def _draw_dropout(owner):
    """-> None when inter-layer dropout is off for this call, else (p, seed, subsequence) for plan.set_dropout.  On, as in
    nn.LSTM.forward: the module is in train() mode, ``owner.dropout`` (read now) > 0 and there is a layer to drop into --
    grad mode does not enter.  The 64-bit seed comes from the default CPU generator (no device sync, reproducible under
    torch.manual_seed); the subsequence is ``owner.dropout_subsequence``, or the torch.distributed rank, so that ranks
    seeded alike still draw different masks."""
    p = _dropout_p(owner)
    if not owner.training or p == 0.0 or owner.num_layers < 2:
        return None
    lo, hi = torch.randint(0, 2 ** 32, (2,), dtype=torch.int64).tolist()
    sub = owner.dropout_subsequence
    if sub is None:
        dist = torch.distributed
        sub = dist.get_rank() if dist.is_available() and dist.is_initialized() else 0
    return p, (hi << 32) | lo, int(sub)


def _adopt_lstm(module, input_size, hidden_size, num_layers, compute_dtype, dropout, bidirectional):
    """The attributes HipLSTM and BiLSTM share, the parameters of a reference nn.LSTM (same init, key names and order) and
    an empty plan pool."""
    module.input_size, module.hidden_size, module.num_layers = input_size, hidden_size, num_layers
    module.compute_dtype = compute_dtype
    module.dropout, module.dropout_subsequence = dropout, None
    ref = nn.LSTM(input_size, hidden_size, num_layers=num_layers, batch_first=True, bidirectional=bidirectional)
    for name, p in ref.named_parameters():
        module.register_parameter(name, nn.Parameter(p.detach().clone()))
    module._plans = _PlanPool()


class _LstmFunction(torch.autograd.Function):
    """Stacked LSTM over libcsn_hip: (x, h0, c0, params) -> (y_last, y_all, h_n, c_n), the ones ``call.outputs`` does not
    take as empty placeholders.  A training forward keeps its state in a workspace that stays checked out until the
    matching backward has run, so several forwards (e.g. the multi-crop views of the DINO trainer) can be outstanding at
    once.  The entry points differ in their _Call alone: HipLSTM.forward takes y_last (y_all with want_all),
    forward_views y_last of the windowed rows on a CSN_LSTM_STATE plan, LSTM.forward y_all and the final state and never
    lets the library overwrite .grad."""

    @staticmethod
    def forward(ctx, x, h0, c0, owner, call, L, *params):
        """``params``: the 4 L parameters of the stack, then under "attn" the query (an input so that autograd asks for its
        gradient; the plan reads ``call.attn``)."""
        plan = owner._checkout(call.B, call.T, x.device, call.training, dropout=call.drop is not None, state=call.state_plan)
        if call.want_weights:
            call.attn_out = [torch.empty((call.B, call.T), dtype=torch.float32, device=x.device)]
        got = _armed(plan, call, lambda: plan.forward(x, *(params[g * L:(g + 1) * L] for g in range(4)), want_all=call.outputs[1],
                                                      h0=h0, c0=c0, want_state=call.outputs[2]),
                     src=x if call.views is not None else None)
        ctx.lease, ctx.owner, ctx.call, ctx.L, ctx.param_like = _Lease(plan), owner, call, L, params
        ctx.need = tuple(t is not None and t.requires_grad for t in (x, h0, c0))
        ctx.x_shape = x.shape
        if not call.training:
            ctx.lease.release()
        return tuple(t if take else got[0].new_empty(0) for t, take in zip((got + (None, None))[:4], call.outputs))

    @staticmethod
    def backward(ctx, *dys):
        owner, call, L, params = ctx.owner, ctx.call, ctx.L, ctx.param_like
        _refuse_second_backward(owner, (ctx.lease,))
        plan = ctx.lease.plan
        direct, accumulate = _direct_grads(owner, params, call.overwrite)
        grads = _grad_targets(params, direct)
        state_shape = (L, plan.desc.B, plan.desc.H)
        dx, dh0, dc0 = (torch.empty(shape, dtype=torch.float32, device=params[0].device) if need else None
                        for need, shape in zip(ctx.need, (ctx.x_shape, state_shape, state_shape)))
        dy_last, dy_all, dh_n, dc_n = (dy if take else None for dy, take in zip(dys, call.outputs))
        # (the query's gradient is written like the weights': into attn_query.grad -- overwritten or added to -- or a temporary)
        _armed(plan, call, lambda: plan.backward(dy_last, dy_all, [grads[g * L:(g + 1) * L] for g in range(4)], dx=dx,
                                                 dh_n=dh_n, dc_n=dc_n, dh0=dh0, dc0=dc0),
               grad=(owner.grad_ready_hook if direct else None, accumulate), dq=grads[4 * L] if len(grads) > 4 * L else None)
        ctx.lease.release()
        return (dx, dh0, dc0, None, None, None, *([None] * len(params) if direct else grads))


class HipLSTM(nn.Module):
    """nn.LSTM(batch_first=True) parameter-compatible stacked LSTM on the HIP path.

    ``compute_dtype``: torch.bfloat16 (bf16 MFMA operands, f32 accumulate and cell state -- the
    fast path) or torch.float32 (exact-f32 MFMA -- the parity path).

    ``dropout``: nn.LSTM's inter-layer dropout -- in train() mode the output sequence of every layer but the top one is
    masked with probability ``dropout`` and scaled by 1/(1 - dropout) before the next layer reads it, inside the fused
    multi-layer launches.  The attribute is read on every call, as nn.LSTM.forward reads it.
    ``dropout_subsequence``: None = the torch.distributed rank.

    ``resident=True`` (hidden_size <= 128): every plan of the module is a CSN_LSTM_RESIDENT one -- the steps of a chunk
    run inside one launch per layer, W_hh in registers, with the results of the per-step cells bit for bit (DESIGN.md
    section 21).  A property of the plans, not of the parameters: state_dicts are unchanged.

    ``readout``: "last" (the default), "mean" or "max" -- what ``forward`` and ``forward_views`` return as [B, H]: the top
    layer's output at each row's last step, or its mean / maximum over the row's steps, reduced from the workspace inside
    the library with no [B, T, H] tensor written or read.  No parameter depends on these three.
    "attn": the weighted mean over the row's steps under the weights softmax_t(hidden_size ** -0.5 <h_t, attn_query>),
    fused in the library likewise.  The module then owns ``attn_query`` [H], initialised to zeros --
    mean pooling at the start --, and its state_dict holds that key; ``attention=True`` gives the parameter to a module
    whose ``readout`` is another (LSTM.pooled).  ``forward(x, return_weights=True)`` also returns the detached weights.
    """

    MAX_IDLE_PLANS = 4      # workspaces are large (10 GB at cfg2): keep only a few idle ones
    _STATE_PLANS = False    # LSTM: plans created with CSN_LSTM_STATE

    def __init__(self, input_size, hidden_size, num_layers=1, compute_dtype=torch.bfloat16, dropout=0.0, resident=False,
                 readout="last", attention=False):
        super().__init__()
        self.readout = _check_readout(type(self).__name__, readout)
        self.resident = _check_resident(type(self).__name__, resident, hidden_size)
        _check_dropout_p(dropout)
        if dropout > 0 and num_layers == 1:
            warnings.warn("dropout option adds dropout after all but last recurrent layer, so non-zero dropout expects "
                          f"num_layers greater than 1, but got dropout={dropout} and num_layers={num_layers}")
        _adopt_lstm(self, input_size, hidden_size, num_layers, compute_dtype, float(dropout), bidirectional=False)
        if attention or readout == "attn":
            self.attn_query = nn.Parameter(torch.zeros(hidden_size))
        # set by a trainer that owns the gradient buffers (trainer.DistillTrainer): the backward writes each parameter's
        # gradient straight into its .grad and calls grad_ready_hook(layer) as soon as a layer's gradients are enqueued
        # direct_grads: False = temporaries; True = .grad is overwritten (one forward per step); "accumulate" = .grad is
        # added to in the library, so several forwards per step (views, micro-batches, chunks of a recording) are summed
        self.direct_grads = False
        self.grad_ready_hook = None

    def _checkout(self, B, T, device, training, dropout=False, state=None):
        """state: None = the class's kind of plan; True = a CSN_LSTM_STATE plan (the views form of HipLSTM: lengths)."""
        state = self._STATE_PLANS if state is None else bool(state)
        key = ((B, T, str(device), bool(training), self.compute_dtype) + (("dropout plan",) if dropout else ()) +
               (("state plan",) if state != self._STATE_PLANS else ()) + (("resident plan",) if self.resident else ()))
        return self._plans.checkout(key, lambda: cabi.LstmPlan(
            B, T, self.input_size, self.hidden_size, self.num_layers, self.compute_dtype, device, training=training, state=state,
            dropout=dropout, resident=self.resident), self.MAX_IDLE_PLANS)

    def all_plans(self):
        return self._plans.all()

    def _flat_params(self):
        return [getattr(self, f"{n}_l{k}") for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh") for k in range(self.num_layers)]

    def _own_queries(self):
        """[attn_query] under the attention readout (an input of the autograd function behind the stack's parameters), else []."""
        return _attn_queries(self, type(self).__name__) if self.readout == "attn" else []

    def forward_views(self, x, views, lengths):
        """Input windows: ``x`` is a SOURCE [S, Tsrc, I]; row b of the LSTM batch is ``x[rows[b], starts[b]:starts[b] +
        lengths[b]]`` with ``views = (rows, starts)``, read in place (csn_lstm_plan_set_views: no slice, no copy, no read
        past a window).  -> y_last [B', H], each row's top-layer output at its own last step: the bits of ``forward`` on
        the gathered rows.  The batch is B' = len(rows) and the plan runs T' = max(lengths) steps, so all the multi-crop
        views of a batch are ONE recurrence pass.  No gradient reaches x (``x.requires_grad`` raises)."""
        _dropout_p(self)
        rows, starts, lengths = _check_views("HipLSTM", x, views, lengths, self.input_size)
        params = self._flat_params() + self._own_queries()
        call = _Call(x, _training(None, None, None, params), _draw_dropout(self), lengths, (rows, starts), state_plan=True,
                     readout=self.readout, attn=self._own_queries())
        return _LstmFunction.apply(x, None, None, self, call, self.num_layers, *params)[0]

    def forward(self, x, want_all=False, return_weights=False):
        """-> y_last [B, H] (the readout); with ``want_all`` (y_all, y_last); with ``return_weights`` (readout "attn" only)
        the detached attention weights [B, T] come last."""
        _dropout_p(self)
        if return_weights and self.readout != "attn":
            raise ValueError(f'{type(self).__name__}: return_weights needs readout="attn"')
        if not x.is_cuda:
            raise cabi.CsnError("HipLSTM runs on the GPU only (no CPU fallback); move the module and input to cuda")
        params = self._flat_params() + self._own_queries()
        call = _Call(x, _training(x, None, None, params), _draw_dropout(self), outputs=(True, bool(want_all), False, False),
                     readout=self.readout, attn=self._own_queries(), want_weights=return_weights)
        y_last, y_all, _, _ = _LstmFunction.apply(x, None, None, self, call, self.num_layers, *params)
        out = (y_all, y_last) if want_all else (y_last,)
        if return_weights:
            out += (call.weights(),)
        return out if len(out) > 1 else out[0]


def _check_views(name, x, views, lengths, input_size):
    """The ``views`` / ``lengths`` arguments of the window forms -> (rows, starts, lengths), tuples of B' ints.  What the
    library checks itself (rows and windows inside the source) is left to it."""
    if isinstance(x, nn.utils.rnn.PackedSequence) or x.dim() != 3 or x.shape[2] != input_size:
        raise ValueError(f"{name}: with views the input is the source tensor [S, Tsrc, {input_size}]")
    if x.requires_grad:
        raise ValueError(f"{name}: views on an input that requires grad (the gradient of shared source rows would need a "
                         "scatter-add: not supported)")
    if lengths is None:
        raise ValueError(f"{name}: views need lengths (the steps of every row's window)")
    if not x.is_cuda:
        raise cabi.CsnError(f"{name} runs on the GPU only (no CPU fallback); move the module and input to cuda")
    rows, starts = ([int(v) for v in (t.tolist() if isinstance(t, torch.Tensor) else t)] for t in views)
    if len(rows) != len(starts) or not rows:
        raise ValueError(f"{name}: views = (rows, starts) with {len(rows)} rows and {len(starts)} starts")
    return tuple(rows), tuple(starts), _check_lengths(name, lengths, len(rows), x.shape[1])


def _forward_packed(module, name, x, hx, lengths):
    """LSTM / BiLSTM on a PackedSequence: the padded batch with the lengths it carries, and the output packed again with
    the input's batch_sizes and indices; (h_n, c_n) come back in the original batch order, as from nn.LSTM."""
    if lengths is not None:
        raise ValueError(f"{name}: lengths given together with a PackedSequence (it carries its own)")
    padded, lens = nn.utils.rnn.pad_packed_sequence(x, batch_first=True)
    output, state = module.forward(padded, hx, lengths=lens)
    # pad_packed_sequence gave the rows in the original batch order: back into the input's own (sorted) order, so
    # that the data lines up with its batch_sizes whatever order it gave to rows of equal length
    if x.sorted_indices is not None:
        output, lens = output.index_select(0, x.sorted_indices), lens[x.sorted_indices.cpu()]
    packed = nn.utils.rnn.pack_padded_sequence(output, lens, batch_first=True, enforce_sorted=True)
    return nn.utils.rnn.PackedSequence(packed.data, x.batch_sizes, x.sorted_indices, x.unsorted_indices), state


def _check_lengths(name, lengths, B, T):
    """The ``lengths`` argument of LSTM / BiLSTM -> None or a tuple of B ints in [0, T]."""
    if lengths is None:
        return None
    if isinstance(lengths, torch.Tensor):
        if lengths.is_cuda:
            raise ValueError(f"{name}: lengths must be a CPU int tensor or a sequence of ints (pass CPU lengths, as "
                             "pack_padded_sequence takes them)")
        if lengths.dim() != 1 or lengths.dtype.is_floating_point or lengths.dtype in (torch.bool,):
            raise ValueError(f"{name}: lengths must be a 1-d int tensor, got {lengths.dtype} of shape {list(lengths.shape)}")
        lengths = lengths.tolist()
    lengths = tuple(int(n) for n in lengths)
    if len(lengths) != B:
        raise ValueError(f"{name}: {len(lengths)} lengths for a batch of {B}")
    bad = [n for n in lengths if n < 0 or n > T]
    if bad:
        raise ValueError(f"{name}: length {bad[0]} outside [0, T = {T}]")
    return lengths


def _forward_stateful(module, name, dirs, function, x, hx, lengths, views, **form):
    """The call contract of LSTM (``dirs`` = 1) and BiLSTM (2) -- views, PackedSequence, x, hx [dirs * L, B, H], lengths,
    the dropout attribute, the device -- and then the call: ``function`` on a _Call of ``form``."""
    if views is not None:
        rows, starts, lengths = _check_views(name, x, views, lengths, module.input_size)
        views = (rows, starts)
    if isinstance(x, nn.utils.rnn.PackedSequence):
        return _forward_packed(module, name, x, hx, lengths)
    if x.dim() != 3:
        raise ValueError(f"{name}: input must be batched [B, T, {module.input_size}] (batch_first); got shape "
                         f"{list(x.shape)} (unbatched input is not supported)")
    if x.shape[2] != module.input_size:
        raise ValueError(f"{name}: input has {x.shape[2]} features, expected {module.input_size}")
    B, L, H = (x.shape[0] if views is None else len(views[0])), module.num_layers, module.hidden_size
    h0 = c0 = None
    if hx is not None:
        h0, c0 = hx
        for which, t in (("h0", h0), ("c0", c0)):
            if tuple(t.shape) != (dirs * L, B, H):
                raise ValueError(f"{name}: {which} must be [{'2 * ' if dirs == 2 else ''}num_layers, B, hidden_size] = "
                                 f"{[dirs * L, B, H]}, got {list(t.shape)}")
    if views is None:
        lengths = _check_lengths(name, lengths, B, x.shape[1])
    _dropout_p(module)
    if not x.is_cuda:
        raise cabi.CsnError(f"{name} runs on the GPU only (no CPU fallback); move the module and input to cuda")
    params = module._flat_params() + list(form.get("attn") or ())
    call = _Call(x, _training(x, h0, c0, params), _draw_dropout(module), lengths, views, **form)
    got = function.apply(x, h0, c0, module, call, L, *params)
    if call.readout != "last":
        return (got[0], call.weights()) if call.want_weights else got[0]       # (pooled: the [B, H] / [B, 2H] readout alone)
    *_, output, h_n, c_n = got
    return output, (h_n, c_n)


def _pooled(module, name, x, hx, lengths, views, readout, return_weights=False):
    """``pooled`` of LSTM / BiLSTM: a PackedSequence is padded with the lengths it carries, the readout is checked.
    -> (x, lengths, what the readout adds to the call's form)."""
    if _check_readout(name, readout) == "last":
        raise ValueError(f"{name}.pooled: readout must be 'mean' or 'max', or 'attn' on a module built with attention=True "
                         "(the last step is what forward's h_n[-1] holds)")
    if return_weights and readout != "attn":
        raise ValueError(f'{name}.pooled: return_weights needs readout="attn"')
    form = dict(readout=readout)
    if readout == "attn":
        form.update(attn=_attn_queries(module, f"{name}.pooled"), want_weights=return_weights)
    if isinstance(x, nn.utils.rnn.PackedSequence):
        if lengths is not None or views is not None:
            raise ValueError(f"{name}: lengths or views given together with a PackedSequence (it carries its own lengths)")
        x, lengths = nn.utils.rnn.pad_packed_sequence(x, batch_first=True)
    return x, lengths, form


class LSTM(HipLSTM):
    """Drop-in for ``torch.nn.LSTM(input_size, hidden_size, num_layers, batch_first=True)`` on the HIP path, with the
    whole of its call contract: ``forward(x[B,T,I], hx=None) -> (output[B,T,H], (h_n[L,B,H], c_n[L,B,H]))``, hx =
    (h0, c0) or None (zeros); gradients reach x, h0, c0 and every parameter.  Parameter names, shapes and init are
    nn.LSTM's, so state_dicts load both ways.  ``compute_dtype`` as in HipLSTM.

    Variable-length batches: ``forward(x, hx, lengths=...)`` with B ints (a sequence or a CPU int tensor, as
    ``pack_padded_sequence`` takes them) gives what nn.LSTM gives on the packed batch, padded back to T: the output is
    zero past each row's length, (h_n, c_n) are each row's state after its last step, and nothing in the padding is read
    or receives a gradient.  A length of 0 (beyond torch) passes the row's state through.  ``x`` may also be a
    ``PackedSequence``; the output is then a PackedSequence with the same batch_sizes and indices and (h_n, c_n) come
    back in the original batch order, as from nn.LSTM.  The plan is still keyed by (B, T): lengths are per call, and the
    work follows the longest row.

    Inter-layer dropout: the constructor still refuses ``dropout != 0``; set the attribute (``lstm.dropout = p``), which is
    read on every call as nn.LSTM.forward reads it, and is active in train() mode (HipLSTM).

    Runs on CSN_LSTM_STATE plans (include/csn_hip.h): with bf16 compute the path HipLSTM takes for the shape (the
    weight-stationary kernels where they apply), with float32 the per-step cells (path 0).  With bf16 compute, h0 is rounded to bf16 as
    every h is and c stays float32, so (h_n, c_n) fed back as hx continues a sequence exactly.
    """

    _STATE_PLANS = True

    def __init__(self, input_size, hidden_size, num_layers=1, bias=True, batch_first=True, dropout=0.0,
                 bidirectional=False, proj_size=0, compute_dtype=torch.bfloat16, resident=False, attention=False):
        unsupported = [name for name, bad in (("bias=False", not bias), ("batch_first=False", not batch_first),
                                              ("dropout != 0", dropout != 0), ("bidirectional=True", bidirectional),
                                              ("proj_size != 0", proj_size != 0)) if bad]
        if unsupported:
            raise ValueError(f"LSTM: {', '.join(unsupported)} is not supported (batch-first, biased, unidirectional "
                             f"stacks without projection or inter-layer dropout only; for bidirectional=True use BiLSTM)")
        super().__init__(input_size, hidden_size, num_layers, compute_dtype=compute_dtype, resident=resident, attention=attention)
        self.bias, self.batch_first, self.dropout, self.bidirectional, self.proj_size = True, True, 0.0, False, 0

    def forward(self, x, hx=None, lengths=None, views=None):
        """``views = (rows, starts)``, each B' ints, with ``lengths`` (B' ints, required): x is a SOURCE [S, Tsrc, I] and
        row b of the LSTM batch is ``x[rows[b], starts[b]:starts[b] + lengths[b]]``, read in place.  The batch is then
        B' = len(rows), T' = max(lengths): output [B', T', H], hx and (h_n, c_n) [L, B', H], all with the bits of the call
        on the gathered rows.  No gradient reaches x through views (``x.requires_grad`` raises ValueError)."""
        return _forward_stateful(self, "LSTM", 1, _LstmFunction, x, hx, lengths, views, outputs=(False, True, True, True),
                                 overwrite=False)

    def pooled(self, x, hx=None, lengths=None, views=None, readout="mean", return_weights=False):
        """-> [B, H]: the mean (``readout="mean"``) or maximum ("max") of ``forward``'s output over each row's valid steps --
        ``output.sum(1) / n`` in float64 rounded once, or ``output.max over t < n``; rows of length 0 give zeros.  The
        library reduces the top layer's saved steps itself: no [B, T, H] output is written, and the backward expands the
        gradient inside the pass that lays it out for the recurrence.  Arguments as in ``forward``; gradients reach x, h0,
        c0 and every parameter (under "max" at the first step that attains the maximum, as torch.max's).
        ``readout="attn"`` (a module built with ``attention=True``): the weighted mean under softmax_t(H ** -0.5 <output_t,
        attn_query>) over the valid steps, float64 inside and rounded once; gradients also reach ``attn_query``.  With
        ``return_weights`` -> (pooled, weights [B, T]): the detached float32 weights, zero past each row's length (no
        gradient flows through them)."""
        x, lengths, form = _pooled(self, "LSTM", x, hx, lengths, views, readout, return_weights)
        return _forward_stateful(self, "LSTM", 1, _LstmFunction, x, hx, lengths, views, outputs=(True, False, False, False),
                                 overwrite=False, **form)


class _BiLstmFunction(torch.autograd.Function):
    """Bidirectional stacked LSTM: (x, h0, c0, params) -> (output[B,T,2H], h_n[2L,B,H], c_n[2L,B,H]) as 2L single-layer
    plans, a plain and a CSN_LSTM_REVERSE one per layer, one after the other on the current stream.  The two directions
    of a layer write their halves of one [B,T,2H] tensor in place (csn_lstm_plan_set_io), which is the next layer's x;
    the backward reads the halves of its gradient in place and the second direction adds its input gradient to the
    first's.  No torch op touches a [B,T,.] tensor here apart from allocating it.

    ``call.drop`` = (p, seed, subsequence) or None: inter-layer dropout.  The plans of every layer below the top one store
    their half of the interface tensor masked and scaled, and read their half of its gradient masked and scaled, inside the
    layout passes they run anyway (csn_lstm_plan_set_output_dropout; _armed).  ``call.views`` = (rows, starts) or None: x is
    a source tensor and layer 0's two plans read their rows' windows of it in place (csn_lstm_plan_set_views).
    ``call.readout`` "mean" / "max" (BiLSTM.pooled): the first result is the pooled [B,2H] instead -- the two top-layer plans
    write no y_all and hand back their pooled y_last, which are concatenated, and the backward gives each its half of the
    [B,2H] gradient as dy_last.  Under "attn" the two queries follow the 8 L parameters, and each top-layer plan pools its
    half under its own query and its own softmax."""

    @staticmethod
    def forward(ctx, x, h0, c0, owner, call, L, *params):
        B, T, H = call.B, call.T, owner.hidden_size
        h_n = torch.empty((2 * L, B, H), dtype=torch.float32, device=x.device)
        c_n = torch.empty((2 * L, B, H), dtype=torch.float32, device=x.device)
        leases, inp, halves = [], x, []
        if call.want_weights:
            call.attn_out = [torch.empty((B, T), dtype=torch.float32, device=x.device) for _ in range(2)]
        for l in range(L):
            pooled = call.readout != "last" and l == L - 1
            out = None if pooled else torch.empty((B, T, 2 * H), dtype=torch.float32, device=x.device)
            for d in range(2):
                k = 2 * l + d
                plan = owner._checkout(B, T, inp.shape[2], x.device, call.training, reverse=d == 1)
                lease = _Lease(plan)        # (at once: the next direction / layer of the same shape must take another plan)
                run = lambda: plan.forward(inp, *([p] for p in params[4 * k:4 * k + 4]),                   # noqa: E731
                                           h0=None if h0 is None else h0[k:k + 1], c0=None if c0 is None else c0[k:k + 1],
                                           want_state=True, y_all=None if pooled else out[:, :, d * H:(d + 1) * H],
                                           state_out=(h_n[k:k + 1], c_n[k:k + 1]))
                try:
                    halves.append(_armed(plan, call, run, k=k, src=x if call.views is not None and l == 0 else None)[0])
                except BaseException:
                    for held in leases + [lease]:       # (a refused call, e.g. a window past the source: nothing stays leased)
                        held.release()
                    raise
                if call.training:
                    leases.append(lease)
                else:
                    lease.release()
            inp = torch.cat(halves[-2:], dim=1) if pooled else out
        ctx.leases, ctx.L, ctx.owner, ctx.call = leases, L, owner, call
        ctx.need = tuple(t is not None and t.requires_grad for t in (x, h0, c0))
        ctx.x_width = x.shape[2]
        ctx.param_like = params
        return inp, h_n, c_n

    @staticmethod
    def backward(ctx, dy, dh_n, dc_n):
        L, leases, call = ctx.L, ctx.leases, ctx.call
        _refuse_second_backward(ctx.owner, leases)
        B, T, H = call.B, call.T, ctx.owner.hidden_size
        dev = ctx.param_like[0].device
        need_dx, need_dh0, need_dc0 = ctx.need
        grads = _grad_targets(ctx.param_like, False)
        dh0 = torch.empty((2 * L, B, H), dtype=torch.float32, device=dev) if need_dh0 else None
        dc0 = torch.empty((2 * L, B, H), dtype=torch.float32, device=dev) if need_dc0 else None
        if dy.dtype != torch.float32 or not dy.is_contiguous():
            dy = dy.float().contiguous()    # (autograd hands a dense gradient as a rule: an expanded or sliced one is copied once)
        if dy.data_ptr() % 16:
            dy = dy.clone()                 # (a pitched dy_all is taken on 16 bytes, and the masked load moves 16: a dense gradient
                                            # at an odd storage offset is copied once)
        for l in range(L - 1, -1, -1):
            pooled = call.readout != "last" and l == L - 1
            dinp = torch.empty((B, T, ctx.x_width if l == 0 else 2 * H), dtype=torch.float32, device=dev) if (l > 0 or need_dx) else None
            for d in range(2):
                k = 2 * l + d
                plan = leases[k].plan
                _armed(plan, call, lambda: plan.backward(
                    dy[:, d * H:(d + 1) * H] if pooled else None, None if pooled else dy[:, :, d * H:(d + 1) * H], [[g] for g in grads[4 * k:4 * k + 4]], dx=dinp, dh_n=dh_n[k:k + 1],
                    dc_n=dc_n[k:k + 1], dh0=None if dh0 is None else dh0[k:k + 1], dc0=None if dc0 is None else dc0[k:k + 1]),
                       grad=(None, False), k=k, dq=grads[8 * L + d] if pooled and call.readout == "attn" else None)
                leases[k].release()
            dy = dinp
        return (dy, dh0, dc0, None, None, None, *grads)


class BiLSTM(nn.Module):
    """``torch.nn.LSTM(input_size, hidden_size, num_layers, batch_first=True, bidirectional=True)`` on the HIP path:
    ``forward(x[B,T,I] | PackedSequence, hx=None, lengths=None) -> (output[B,T,2H], (h_n[2L,B,H], c_n[2L,B,H]))``, hx
    and h_n indexed ``2 * layer + direction`` as in torch; gradients reach x, h0, c0 and every parameter.  Parameter
    names, order, shapes and init are nn.LSTM's (``weight_ih_l{k}``, ..., ``bias_hh_l{k}``, then the same with
    ``_reverse``, layer by layer; ``weight_ih_l{k>=1}`` is [4H, 2H]), so state_dicts load both ways.  Lengths, a
    PackedSequence and a length of 0 mean what they mean for ``LSTM``: the reverse direction of a row starts at that
    row's own last valid step.  ``output[:, 0, H:]`` is therefore the reverse direction's final output and
    ``output[:, -1, H:]`` its first: the summary of a sequence is ``cat(h_n[-2], h_n[-1])``.

    Runs as 2L single-layer CSN_LSTM_STATE plans, a plain and a CSN_LSTM_REVERSE one per layer, sequentially on the
    current stream (the weight-stationary launches need the whole chip, so the directions do not overlap); no recurrence
    kernel differs from ``LSTM``'s, only the layout passes around it index time backwards.  The
    upper layers read an input of width 2H, which the fused input projection (I <= 128) does not take: they project
    through the GEMM.  All 2L workspaces stay leased from a training forward to its backward: at B 256, T 500, I 128,
    H 768, L 2 in bf16 that is 2 x 4.32 GB (layer 0) + 2 x 5.42 GB (layer 1, input width 2H) = 19.48 GB, against 8.47 GB
    for the unidirectional two-layer plan (csn_lstm_workspace_bytes; 22.77 GB at B 256, T 440, H 1024).

    Inter-layer dropout, as on ``LSTM``: the constructor still refuses ``dropout != 0``; set the attribute
    (``bilstm.dropout = p``), which is read on every call as nn.LSTM.forward reads it and is active in train() mode with
    ``num_layers >= 2``, also under no_grad.  The concatenated [B,T,2H] output of every layer but the top one is masked
    once and scaled by 1/(1 - p), inside the layout passes the plans run anyway (csn_lstm_plan_set_output_dropout,
    DESIGN.md section 23).  ``dropout_subsequence``: None = the torch.distributed rank.

    Input windows: ``forward(x, hx, lengths, views=(rows, starts))`` has ``LSTM.forward``'s contract.

    Not in this class: the direct / accumulating gradient writes of ``HipLSTM`` (gradients go to autograd temporaries).
    """

    MAX_IDLE_PLANS = 4

    def __init__(self, input_size, hidden_size, num_layers=1, compute_dtype=torch.bfloat16, dropout=0.0, resident=False,
                 attention=False):
        super().__init__()
        self.resident = _check_resident("BiLSTM", resident, hidden_size)     # passed to all 2L single-layer plans
        if dropout != 0:
            raise ValueError("BiLSTM: dropout != 0 is not supported (the inter-layer dropout of this library lives "
                             "between the layers of one plan; a bidirectional stack runs one plan per layer and direction)")
        _adopt_lstm(self, input_size, hidden_size, num_layers, compute_dtype, 0.0, bidirectional=True)
        self.bias, self.batch_first, self.bidirectional, self.proj_size = True, True, True, 0
        if attention:
            self.attn_query = nn.Parameter(torch.zeros(hidden_size))
            self.attn_query_reverse = nn.Parameter(torch.zeros(hidden_size))

    def _checkout(self, B, T, I, device, training, reverse):
        key = (B, T, I, str(device), bool(training), self.compute_dtype, bool(reverse)) + (("resident plan",) if self.resident else ())
        return self._plans.checkout(key, lambda: cabi.LstmPlan(
            B, T, I, self.hidden_size, 1, self.compute_dtype, device, training=training, state=True, reverse=reverse,
            resident=self.resident), self.MAX_IDLE_PLANS)

    def all_plans(self):
        return self._plans.all()

    def _flat_params(self):
        return [getattr(self, f"{n}_l{k}{sfx}") for k in range(self.num_layers) for sfx in ("", "_reverse")
                for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]

    def forward(self, x, hx=None, lengths=None, views=None):
        """``views = (rows, starts)``, each B' ints, with ``lengths`` (B' ints, required): x is a SOURCE [S, Tsrc, I] and
        row b of the batch is ``x[rows[b], starts[b]:starts[b] + lengths[b]]``, read in place by layer 0's two plans.  The
        batch is then B' = len(rows), T' = max(lengths): output [B', T', 2H], hx and (h_n, c_n) [2L, B', H], all with the
        bits of the call on the gathered rows.  No gradient reaches x through views (``x.requires_grad`` raises)."""
        return _forward_stateful(self, "BiLSTM", 2, _BiLstmFunction, x, hx, lengths, views, bi=(self.num_layers, self.hidden_size))

    def pooled(self, x, hx=None, lengths=None, views=None, readout="mean", return_weights=False):
        """-> [B, 2H]: the mean ("mean") or maximum ("max") of ``forward``'s output over each row's valid steps, as
        ``LSTM.pooled``: each direction's top-layer plan pools its half and the two [B, H] results are concatenated, which
        equals pooling the [B, T, 2H] output.  The top layer writes no output tensor.  Arguments as in ``forward``.
        ``readout="attn"`` (a module built with ``attention=True``, which owns ``attn_query`` and ``attn_query_reverse``):
        each direction's top-layer plan pools ITS half with its own query and its own softmax over time, and the two
        [B, H] halves are concatenated.  This is NOT one softmax over the concatenated [B, T, 2H] output (one query of 2H
        entries scoring both halves together): that joint form is left out.  With ``return_weights`` -> (pooled, weights
        [B, T, 2]), the detached weights of the forward and the reverse direction, both indexed by the caller's time."""
        x, lengths, form = _pooled(self, "BiLSTM", x, hx, lengths, views, readout, return_weights)
        return _forward_stateful(self, "BiLSTM", 2, _BiLstmFunction, x, hx, lengths, views, bi=(self.num_layers, self.hidden_size),
                                 **form)


class Model(nn.Module):
    """``models.lstm.Model``.  ``head``/``fc`` may be reassigned by
    ``MultiCropWrapper`` (utils/utils.py:607-612) without breaking forward."""

    def __init__(self, input_size=128, lstm_size=128, lstm_layers=1, output_size=128, include_top=True,
                 n_classes=40, compute_dtype=torch.bfloat16, dropout=0.0, bidirectional=False, resident=False,
                 readout="last"):
        """``bidirectional=True``: the encoder is a ``BiLSTM`` and ``fc`` has 2 * lstm_size inputs.  The feature fed to
        ``fc`` is then ``cat(h_n[-2], h_n[-1])``, the top layer's FINAL state in each direction -- not ``output[:, -1]``,
        whose reverse half has seen one step only.  ``resident=True`` (lstm_size <= 128): the encoder's plans run the
        CU-resident recurrence (HipLSTM).  ``readout`` "mean" / "max": the feature fed to ``fc`` is the top layer's output
        pooled over each row's steps instead (HipLSTM's ``readout``; bidirectional: ``BiLSTM.pooled``).  These add no
        parameter: checkpoints are unchanged.  ``readout="attn"``: the attention readout; the encoder then owns
        ``lstm.attn_query`` (and ``lstm.attn_query_reverse``, each direction pooling its half under its own softmax), which
        the state_dict holds -- a checkpoint is evaluated with the readout it was trained with."""
        super().__init__()
        self.readout = _check_readout("Model", readout)
        self.input_size, self.lstm_size, self.lstm_layers = input_size, lstm_size, lstm_layers
        self.output_size, self.include_top, self.bidirectional = output_size, include_top, bool(bidirectional)
        if self.bidirectional:
            self.lstm = BiLSTM(input_size, lstm_size, lstm_layers, compute_dtype=compute_dtype, resident=resident,
                               attention=readout == "attn")
            # (the attribute, as on the LSTM drop-in: its constructor takes 0 only)
            self.lstm.dropout = _check_dropout_p(dropout)
        else:
            self.lstm = HipLSTM(input_size, lstm_size, lstm_layers, compute_dtype=compute_dtype, dropout=dropout, resident=resident,
                                readout=readout)
        self.fc = nn.Linear((2 if self.bidirectional else 1) * lstm_size, output_size)
        if include_top:
            self.class_pred = nn.Linear(output_size, n_classes)

    def forward(self, x, views=None, lengths=None):
        """``views = (rows, starts)`` with ``lengths``: x is a source [S, Tsrc, C] and the result has one row per window
        (HipLSTM.forward_views, or BiLSTM.forward with views) -- feature rows [B', output_size], and the class logits with
        include_top."""
        if views is None and lengths is not None:
            raise ValueError("Model: lengths are taken with views only")
        if self.bidirectional and self.readout != "last":
            last = self.lstm.pooled(x, None, lengths, views, readout=self.readout)      # [B, 2H]
        elif self.bidirectional:
            _, (h_n, _) = self.lstm(x, None, lengths, views)
            last = torch.cat((h_n[-2], h_n[-1]), dim=1)    # [B, 2H]
        elif views is not None:
            last = self.lstm.forward_views(x, views, lengths)      # [B', H] = top layer at each window's last step
        else:
            last = self.lstm(x)                # [B, H] = top layer at the last timestep
        feat = self.fc(last)
        if self.include_top and hasattr(self, "class_pred"):
            return feat, self.class_pred(feat)
        return feat


class LSTMModel(nn.Module):
    """/root/reference/LSTMDistillRetreival.py:85-110 / LSTMDistill.py:112-142 on the HIP LSTM.

    Keeps the reference's ``x.view(B, C, T)`` (a reshape, not a transpose: the sequence then runs
    over the *channel* axis with ``input_size`` = time samples).  ``all_steps=True`` gives the
    LSTMDistill.py variant: fc on every step, class_pred, ReLU on the features.
    """

    def __init__(self, input_size, hidden_size, n_layers=2, out_features=384, number_of_classes=None,
                 all_steps=False, compute_dtype=torch.bfloat16, dropout=0.0, resident=False, readout="last"):
        """``readout`` "mean" / "max" / "attn" (the form without ``all_steps`` only): ``fc`` reads the LSTM output pooled over
        the sequence instead of its last step (HipLSTM's ``readout``; "attn" adds ``lstm.attn_query`` to the state_dict)."""
        super().__init__()
        if _check_readout("LSTMModel", readout) != "last" and all_steps:
            raise ValueError("LSTMModel: readout applies to the form without all_steps (all_steps feeds every step to fc)")
        self.hidden_size, self.n_layer, self.input_size, self.all_steps = hidden_size, n_layers, input_size, all_steps
        self.lstm = HipLSTM(input_size, hidden_size, n_layers, compute_dtype=compute_dtype, dropout=dropout, resident=resident,
                            readout=readout)
        self.fc = nn.Linear(hidden_size, out_features)
        if number_of_classes:
            self.class_pred = nn.Linear(out_features, number_of_classes)

    def forward(self, x):
        batch_size, timespan, channels = x.size()
        x = x.reshape(batch_size, channels, timespan)
        if self.all_steps:
            y_all, _ = self.lstm(x, want_all=True)
            feat = self.fc(y_all)
            cls_pred = self.class_pred(feat)
            return nn.functional.relu(feat), cls_pred
        return self.fc(self.lstm(x))


class CustomModel(nn.Module):
    """/root/reference/utils/CustomModel.py:4-17 (3-layer MLP; keys fc.0/2/4.*)."""

    def __init__(self, input_size, output_size):
        super().__init__()
        self.fc = nn.Sequential(nn.Linear(input_size, 2000), nn.ReLU(), nn.Linear(2000, 2000), nn.ReLU(),
                                nn.Linear(2000, output_size))

    def forward(self, x):
        return self.fc(x)
