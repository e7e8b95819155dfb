"""Losses of the distillation path, same names / argument meaning as the reference classes.

  CosineSimilarityLoss       LstmDistillFromDinoV2Train.py:36-43   (fused HIP forward+gradient)
  FeatureDistributionLoss    LstmDistillFromDinoV2Train.py:107-140 (torch ops; fused=True: csn_distill_loss)
  loss_fn_kd                 LstmDistillFromDinoV2TrainSpampinato.py:107-121
  FeatureDistributionLossKD  LstmDistillFromDinoV2TrainSpampinato.py:125-184 (soft-target KL + CE)
  FeatureDistributionLossSoft LstmDistillFromDinoV2Eval.py:106-146 (soft-target KL alone)
  FeatureDistributionLossMSE LstmDistillation.py:161-172 (global mean / std / MSE match)
  BarlowTwinsLoss            EEG-BarlowNetworks/net.py:33-42 (HIP off-diagonal reduction; fused=True: csn_barlow_corr + _grad)
  LARS, barlow_learning_rate EEG-BarlowNetworks/optim.py:5-44, barlow_utils.py:8-21
  ContrastiveLoss            not in the reference: the symmetric InfoNCE loss against frozen teacher rows, global negatives
                             (torch ops; fused=True: csn_contrastive_lse + csn_contrastive_grad)
  BankContrastiveLoss        not in the reference: InfoNCE against the fixed bank of every image's teacher row
                             (torch ops; fused=True: csn_bank_contrastive)
Every class is checked against values and gradients obtained by executing the reference's own definition
(tests/golden/ref_losses.npz, tests/test_ref_pinned.py).
Reference quirks are kept on purpose.

``fused=True`` on FeatureDistributionLoss, its KD and Soft variants and loss_fn_kd: value and gradient come from ONE
csn_distill_loss call (float64 arithmetic, two launches) when every tensor input is a float32
device tensor; anything else (CPU tensors, float64) takes the torch form.  Opt-in: the default keeps the torch form.
``fused=True`` on BarlowTwinsLoss: batch norm, correlation, loss and both gradients from csn_barlow_corr + csn_barlow_grad
(float64 arithmetic, five launches) under the same rule, in training mode.
``fused=True`` on ContrastiveLoss: value and gradient from csn_contrastive_lse + csn_contrastive_grad (float64 arithmetic,
seven launches) under the same rule.
``fused=True`` on BankContrastiveLoss: value and gradient from one csn_bank_contrastive call (float64 arithmetic, six
launches) under the same rule.
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import cabi


class HyperParams:          # LstmDistillFromDinoV2Train.py:16-25
    learning_rate = 0.001
    T = 0.5
    soft_target_loss_weight = 0.25
    ce_loss_weight = 0.75
    warmup_teacher_temp = 1.5
    teacher_temp = 0.22
    warmup_teacher_temp_epochs = 50
    alpha = 0.5
    beta = 0.5


class _CosineLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, student, teacher):
        loss, ds = cabi.cosine_loss(student, teacher, want_grad=student.requires_grad)
        ctx.save_for_backward(ds) if ds is not None else None
        ctx.has_grad = ds is not None
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        if not ctx.has_grad:
            return None, None
        (ds,) = ctx.saved_tensors
        return ds * g, None


class CosineSimilarityLoss(nn.Module):
    def __init__(self):
        super().__init__()

    def forward(self, student_outputs, teacher_outputs):
        return _CosineLossFn.apply(student_outputs, teacher_outputs)


def _fusable(*tensors):
    """Every given tensor is on a GPU, and float32 unless it holds integers (labels)."""
    return all(t is not None and t.is_cuda and (t.dtype == torch.float32 or not t.is_floating_point()) for t in tensors)


class _DistillLossFn(torch.autograd.Function):
    """csn_distill_loss: the gradients are computed in the forward, saved, and multiplied by the incoming scalar.
    ``logits is None`` with ``alias``: the student tensor is also the logits of the CE term."""

    @staticmethod
    def forward(ctx, student, teacher, logits, labels, soft_mode, T, w_soft, w_ce, alias):
        want = (ctx.needs_input_grad[0], ctx.needs_input_grad[2])
        loss, ds, dl = cabi.distill_loss(student, teacher, soft_mode, T, w_soft, logits=student if alias else logits,
                                         labels=labels, w_ce=w_ce, want_grad=want)
        ctx.have = (ds is not None, dl is not None)
        ctx.save_for_backward(*[g for g in (ds, dl) if g is not None])
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        saved = list(ctx.saved_tensors)
        ds = saved.pop(0) * g if ctx.have[0] else None
        dl = saved.pop(0) * g if ctx.have[1] else None
        return ds, None, dl, None, None, None, None, None, None


class FeatureDistributionLoss(nn.Module):
    def __init__(self, nepochs, warmup_teacher_temp, teacher_temp, warmup_teacher_temp_epochs, fused=False):
        super().__init__()
        self.mse = nn.MSELoss()
        self.fused = bool(fused)
        self.teacher_temp_schedule = np.concatenate((
            np.linspace(warmup_teacher_temp, teacher_temp, warmup_teacher_temp_epochs),
            np.ones(max(0, nepochs - warmup_teacher_temp_epochs)) * teacher_temp))

    def forward(self, student_outputs, teacher_outputs, epoch, label, pred_label=None):
        HyperParams.T = self.teacher_temp_schedule[epoch]
        if self.fused and _fusable(student_outputs, teacher_outputs, label, pred_label):
            return _DistillLossFn.apply(student_outputs, teacher_outputs, pred_label, label, cabi.SOFT_CE_OF_PROBS,
                                        float(HyperParams.T), HyperParams.beta, HyperParams.alpha, False)
        teacher_logits_with_T = F.softmax(teacher_outputs / HyperParams.T, dim=-1)
        student_logits_with_T = F.softmax(student_outputs / HyperParams.T, dim=-1)
        term1 = HyperParams.alpha * F.cross_entropy(pred_label, label)
        # reference: probabilities of the teacher used as *logits*, student probabilities as targets
        term2 = HyperParams.beta * F.cross_entropy(teacher_logits_with_T, student_logits_with_T)
        return term1 + term2


def _soft_target_kl(student_outputs, teacher_outputs, T):
    """sum p_t (log p_t - log_softmax(s / T)) / B * T^2 -- the soft-target term both variants below share."""
    soft_targets = F.softmax(teacher_outputs / T, dim=-1)
    soft_prob = F.log_softmax(student_outputs / T, dim=-1)
    return torch.sum(soft_targets * (soft_targets.log() - soft_prob)) / soft_prob.size()[0] * (T ** 2)


class FeatureDistributionLossKD(FeatureDistributionLoss):
    """The Spampinato trainer's variant (LstmDistillFromDinoV2TrainSpampinato.py:125-184; its HyperParams :16-25
    give the 0.25 / 0.75 weights and a 1.65 -> 0.22 temperature ramp over 50 epochs): student outputs are class logits."""
    SCHEDULE = dict(warmup_teacher_temp=1.65, teacher_temp=0.22, warmup_teacher_temp_epochs=50)

    def forward(self, student_outputs, teacher_outputs, epoch, label):
        HyperParams.T = self.teacher_temp_schedule[epoch]
        if self.fused and _fusable(student_outputs, teacher_outputs, label):
            T = float(HyperParams.T)
            return _DistillLossFn.apply(student_outputs, teacher_outputs, None, label, cabi.SOFT_KL, T,
                                        HyperParams.soft_target_loss_weight * T * T, HyperParams.ce_loss_weight, True)
        return HyperParams.soft_target_loss_weight * _soft_target_kl(student_outputs, teacher_outputs, HyperParams.T) \
            + HyperParams.ce_loss_weight * F.cross_entropy(student_outputs, label)


class FeatureDistributionLossSoft(FeatureDistributionLoss):
    """The Eval script's variant (LstmDistillFromDinoV2Eval.py:106-146; temperatures of its HyperParams :18-25:
    1.7 -> 0.23 over 50 epochs): the soft-target term alone."""
    SCHEDULE = dict(warmup_teacher_temp=1.7, teacher_temp=0.23, warmup_teacher_temp_epochs=50)

    def forward(self, student_outputs, teacher_outputs, epoch):
        HyperParams.T = self.teacher_temp_schedule[epoch]
        if self.fused and _fusable(student_outputs, teacher_outputs):
            T = float(HyperParams.T)
            return _DistillLossFn.apply(student_outputs, teacher_outputs, None, None, cabi.SOFT_KL, T, T * T, 0.0, False)
        return _soft_target_kl(student_outputs, teacher_outputs, HyperParams.T)


class FeatureDistributionLossMSE(nn.Module):
    """LstmDistillation.py:161-172: 0.4 (std_s - std_t)^2 + 0.4 (mean_s - mean_t)^2 + 0.2 MSE, global statistics."""

    def forward(self, student_outputs, teacher_outputs):
        d_mean = student_outputs.mean() - teacher_outputs.mean()
        d_std = student_outputs.std() - teacher_outputs.std()
        return 0.4 * d_std * d_std + 0.4 * d_mean * d_mean + 0.2 * F.mse_loss(student_outputs, teacher_outputs)


def loss_fn_kd(outputs, labels, teacher_outputs, params, fused=False):
    alpha, T = params.alpha, params.temperature
    if fused and outputs.dim() == 2 and _fusable(outputs, teacher_outputs, labels):
        # nn.KLDivLoss() keeps reduction='mean': the mean over all B * D elements
        return _DistillLossFn.apply(outputs, teacher_outputs, None, labels, cabi.SOFT_KL, float(T),
                                    alpha * T * T / outputs.shape[1], 1. - alpha, True)
    return nn.KLDivLoss()(F.log_softmax(outputs / T, dim=1), F.softmax(teacher_outputs / T, dim=1)) * (alpha * T * T) \
        + F.cross_entropy(outputs, labels) * (1. - alpha)


class _BarlowReduce(torch.autograd.Function):
    """(sum_i (c_ii-1)^2, sum_{i!=j} c_ij^2) by the HIP reduction; gradient 2(c-I) on / 2c off the diagonal."""

    @staticmethod
    def forward(ctx, c):
        ctx.save_for_backward(c)
        out = cabi.barlow_offdiag_sqsum(c)
        return out[0], out[1]

    @staticmethod
    def backward(ctx, g_on, g_off):
        (c,) = ctx.saved_tensors
        eye = torch.eye(c.shape[0], device=c.device, dtype=c.dtype)
        return (2 * (c - eye)) * eye * g_on + (2 * c) * (1 - eye) * g_off


def _barlow_reduce_torch(c):
    """The same two sums in torch ops: for CPU tensors only (host-logic tests of the multi-rank plumbing over gloo;
    a device tensor always takes the HIP reduction)."""
    d = torch.diagonal(c)
    on = (d - 1).pow(2).sum()
    return on, c.pow(2).sum() - d.pow(2).sum()


class _AllReduceSum(torch.autograd.Function):
    """c <- sum over ranks of c.  The reference all-reduces c in place, outside autograd (net.py:38), so each rank
    back-propagates d loss(c_global) / d c through its OWN term only and DDP then averages the parameter
    gradients: the backward here is the identity (the gradient all-reduce of the trainer does the averaging)."""

    @staticmethod
    def forward(ctx, x):
        x = x.clone()
        torch.distributed.all_reduce(x)
        return x

    @staticmethod
    def backward(ctx, g):
        return g


def _dist_world():
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        return torch.distributed.get_world_size()
    return 1


class _BarlowFusedFn(torch.autograd.Function):
    """csn_barlow_corr, the all-reduce of the float64 c, csn_barlow_grad: like _DistillLossFn the gradients are computed in
    the forward, saved, and multiplied by the incoming scalar.  Each rank's gradient goes through its own term of c only
    (the _AllReduceSum contract).  The kernel updates the running statistics of ``bn`` (for z1, then for z2)."""

    @staticmethod
    def forward(ctx, z1, z2, bn, batch_size, lambd):
        want = (ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        z1, z2 = z1.contiguous(), z2.contiguous()
        track = bn.track_running_stats and bn.running_mean is not None
        c_local, saved = cabi.barlow_corr(z1, z2, batch_size, eps=bn.eps, running_mean=bn.running_mean if track else None,
                                          running_var=bn.running_var if track else None, momentum=float(bn.momentum))
        if track and bn.num_batches_tracked is not None:
            bn.num_batches_tracked.add_(2)
        c = c_local
        if _dist_world() > 1:
            c = c_local.clone()
            torch.distributed.all_reduce(c)
        loss, dz1, dz2 = cabi.barlow_grad(z1, z2, c, c_local, saved, batch_size, lambd, want=want)
        ctx.have = (dz1 is not None, dz2 is not None)
        ctx.save_for_backward(*[g for g in (dz1, dz2) if g is not None])
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        grads = list(ctx.saved_tensors)
        dz1 = grads.pop(0) * g if ctx.have[0] else None
        dz2 = grads.pop(0) * g if ctx.have[1] else None
        return dz1, dz2, None, None, None


class BarlowTwinsLoss(nn.Module):
    """net.py:33-42 on two embedding batches: bn(z1).T @ bn(z2) / batch_size, all_reduce, on + lambd*off.
    ``batch_size`` is the GLOBAL batch (args.batch_size there); BatchNorm statistics stay per rank, as there.

    ``fused=True``: value and both gradients in float64 from csn_barlow_corr + csn_barlow_grad when
    both inputs are float32 device tensors, the module and its ``bn`` are in training mode and ``bn.momentum`` is a number;
    anything else takes the torch form below, bit for bit."""

    def __init__(self, dim, batch_size, lambd=0.0051, fused=False):
        super().__init__()
        self.bn = nn.BatchNorm1d(dim, affine=False)
        self.batch_size, self.lambd = batch_size, lambd
        self.fused = bool(fused)

    def _fused_applies(self, z1, z2):
        return self.fused and self.training and self.bn.training and isinstance(self.bn.momentum, (int, float)) \
            and z1.dim() == 2 and z1.shape == z2.shape and _fusable(z1, z2)

    def forward(self, z1, z2):
        if self._fused_applies(z1, z2):
            return _BarlowFusedFn.apply(z1, z2, self.bn, self.batch_size, self.lambd)
        c = self.bn(z1).T @ self.bn(z2)
        c = c / self.batch_size
        if torch.distributed.is_available() and torch.distributed.is_initialized() \
                and torch.distributed.get_world_size() > 1:
            c = _AllReduceSum.apply(c)
        on_diag, off_diag = _BarlowReduce.apply(c.float()) if c.is_cuda else _barlow_reduce_torch(c)
        return on_diag + self.lambd * off_diag


def _gather_rows(x, world):
    """Every rank's ``x`` (equal shapes) concatenated along dimension 0 in rank order."""
    parts = [torch.empty_like(x) for _ in range(world)]
    torch.distributed.all_gather(parts, x.contiguous())
    return torch.cat(parts, dim=0)


def _contrastive_left_out(groups_all, row0, B):
    """[B,N] bool: key j is left out of local query i (the same group id, another row); None without group ids."""
    if groups_all is None:
        return None
    N = groups_all.shape[0]
    rows = torch.arange(row0, row0 + B, device=groups_all.device)
    same = groups_all[row0:row0 + B, None] == groups_all[None, :]
    return same & (rows[:, None] != torch.arange(N, device=groups_all.device)[None, :])


def _contrastive_lse_torch(s_all, t_all, groups_all, row0, B, scale, w_a, w_b):
    """Call 1 in torch ops, in the dtype of the inputs -> (rows [3,B] = lA, lB, p, loss_part: the local rows' part of L)."""
    sh, th = F.normalize(s_all, dim=1, eps=1e-12), F.normalize(t_all, dim=1, eps=1e-12)
    N = sh.shape[0]
    za, zb = scale * (sh[row0:row0 + B] @ th.T), scale * (th[row0:row0 + B] @ sh.T)
    p = scale * (sh[row0:row0 + B] * th[row0:row0 + B]).sum(1)
    out = _contrastive_left_out(groups_all, row0, B)
    if out is not None:
        za, zb = za.masked_fill(out, float("-inf")), zb.masked_fill(out, float("-inf"))
    lA, lB = torch.logsumexp(za, dim=1), torch.logsumexp(zb, dim=1)
    return torch.stack([lA, lB, p]), (w_a * (lA - p) + w_b * (lB - p)).sum() / N


def _contrastive_grad_torch(s_all, t_all, groups_all, row0, B, scale, lse_a, lse_b_all, w_a, w_b, grad_scale, want_dscale):
    """Call 2 in torch ops -> (ds [B,D] holding grad_scale, dscale_part | None)."""
    sh, th = F.normalize(s_all, dim=1, eps=1e-12), F.normalize(t_all, dim=1, eps=1e-12)
    N = sh.shape[0]
    shl, thl = sh[row0:row0 + B], th[row0:row0 + B]
    out = _contrastive_left_out(groups_all, row0, B)
    keep = (lambda x: x) if out is None else (lambda x: x.masked_fill(out, 0.0))
    da = shl @ th.T
    PA, PBt = keep(torch.exp(scale * da - lse_a[:, None])), keep(torch.exp(scale * da - lse_b_all[None, :]))
    g = (scale / N) * ((w_a * PA + w_b * PBt) @ th - (w_a + w_b) * thl)
    nrm = s_all[row0:row0 + B].norm(dim=1, keepdim=True)
    ds = grad_scale * (g - shl * (shl * g).sum(1, keepdim=True) * (nrm > 1e-12)) / nrm.clamp_min(1e-12)
    if not want_dscale:
        return ds, None
    db = thl @ sh.T
    PBq = keep(torch.exp(scale * db - lse_b_all[row0:row0 + B, None]))
    dii = (shl * thl).sum(1)
    return ds, (w_a * ((PA * da).sum(1) - dii) + w_b * ((PBq * db).sum(1) - dii)).sum() / N


class _ContrastiveFn(torch.autograd.Function):
    """The two calls (csn_contrastive_lse / _grad, or the same in torch ops) with the all-gather of lB and the all-reduce of the
    float64 loss partial between them: like _BarlowFusedFn the gradient is computed in the forward, saved, and multiplied by
    the incoming scalar.  ``log_scale`` is the learnable parameter or None; ``scale`` is the logit scale in effect and
    ``scale_grad`` whether the clamp lets a gradient through to ``log_scale``."""

    @staticmethod
    def forward(ctx, student, teacher, groups, log_scale, scale, scale_grad, w_a, w_b, fused):
        dist, world = torch.distributed, _dist_world()
        s, t = student.detach().contiguous(), teacher.detach().contiguous()
        B, row0 = s.shape[0], 0
        if groups is not None:
            groups = groups.to(device=s.device, dtype=torch.int32).contiguous()
        if world > 1:
            sizes = [torch.zeros(1, dtype=torch.int64, device=s.device) for _ in range(world)]
            dist.all_gather(sizes, torch.tensor([B], dtype=torch.int64, device=s.device))
            sizes = [int(v) for v in sizes]
            if any(v != B for v in sizes):
                raise ValueError(f"ContrastiveLoss needs the same number of rows on every rank, got {sizes}")
            row0 = dist.get_rank() * B
            s, t = _gather_rows(s, world), _gather_rows(t, world)
            groups = None if groups is None else _gather_rows(groups, world)
        want_dscale = log_scale is not None and ctx.needs_input_grad[3]
        if fused:
            rows, loss = cabi.contrastive_lse(s, t, scale, groups, row0, B, w_a, w_b)
        else:
            rows, loss = _contrastive_lse_torch(s, t, groups, row0, B, scale, w_a, w_b)
        loss = loss.double().reshape(1)
        if world > 1:
            dist.all_reduce(loss)
        ctx.want_dscale = want_dscale
        if not (ctx.needs_input_grad[0] or want_dscale):        # evaluation: the value alone, no second call
            return loss[0].to(student.dtype)
        lse_b_all = _gather_rows(rows[1], world) if world > 1 else rows[1]
        if fused:
            ds, dscale = cabi.contrastive_grad(s, t, scale, rows[0], lse_b_all, groups, row0, B, w_a, w_b, grad_scale=world,
                                               want_dscale=want_dscale)
        else:
            ds, dscale = _contrastive_grad_torch(s, t, groups, row0, B, scale, rows[0], lse_b_all, w_a, w_b, float(world),
                                                 want_dscale)
        saved = [ds]
        if want_dscale:
            dscale = dscale.double().reshape(1)
            if world > 1:
                dist.all_reduce(dscale)
            # d L / d log_scale = scale dL/dscale where the clamp at log(max_scale) is not in effect
            saved.append((dscale[0] * (scale if scale_grad else 0.0)).to(log_scale.dtype).reshape(log_scale.shape))
        ctx.save_for_backward(*saved)
        return loss[0].to(student.dtype)

    @staticmethod
    def backward(ctx, g):
        saved = ctx.saved_tensors
        ds = saved[0] * g if ctx.needs_input_grad[0] else None
        dlog = saved[1] * g.to(saved[1].dtype) if ctx.want_dscale else None
        return ds, None, None, dlog, None, None, None, None, None


class ContrastiveLoss(nn.Module):
    """The symmetric in-batch contrastive loss (InfoNCE, the CLIP loss) of student rows against FROZEN teacher rows, both
    L2-normalised, at logit scale 1 / temperature:
        L = (1/N) sum_i [ w_s2t (lse_j(a s^_i . t^_j) - a s^_i . t^_i) + w_t2s (lse_j(a t^_i . s^_j) - a s^_i . t^_i) ].
    ``forward(student[B,D], teacher[B,D], groups=None)`` returns a scalar; the teacher gets no gradient.  ``groups`` ([B]
    integers, e.g. the image index): key j is left out of query i's softmax when groups[i] == groups[j] and j != i, so a
    duplicate of the positive in the batch is not pushed away as a false negative.

    With torch.distributed initialised the negatives are the GLOBAL batch: the module all-gathers ``student.detach()``,
    ``teacher`` and ``groups`` (every rank must bring the same B), computes the log-sum-exps of its own rows, all-gathers
    lB (N float64 values), all-reduces the float64 loss partial and returns the global loss on every rank.  The gradient
    it hands to autograd is ``world`` times this rank's rows of the gradient of the global loss (grad_scale = world): the
    MEAN all-reduce of the parameter gradients that FlatGrads / DDP perform then gives exactly the gradient of the global
    loss -- the other ranks' rows of it come from those ranks.

    ``learnable_temperature=True`` keeps ``log_scale`` = log(1 / temperature) as an nn.Parameter; the scale in effect is
    exp(min(log_scale, log(max_scale))) and its gradient is scale * dL/dscale from float64 partials all-reduced over the
    ranks (already global: the parameter is not averaged again).  Reading the scale synchronises with the device.

    Default, and always for CPU or non-float32 tensors: the two-phase algorithm in torch ops in the dtype of the inputs.
    ``fused=True`` on float32 device tensors: value and gradient in float64 from csn_contrastive_lse + csn_contrastive_grad
    (seven launches), each float32 output rounded once."""

    def __init__(self, temperature=0.07, learnable_temperature=False, max_scale=100.0, w_s2t=0.5, w_t2s=0.5, fused=False):
        super().__init__()
        if not (temperature > 0 and np.isfinite(temperature)) or not (max_scale > 0 and np.isfinite(max_scale)):
            raise ValueError(f"ContrastiveLoss: temperature {temperature} and max_scale {max_scale} must be finite and positive")
        self.max_scale, self.w_s2t, self.w_t2s = float(max_scale), float(w_s2t), float(w_t2s)
        self.fused = bool(fused)
        log_scale = torch.tensor(float(np.log(1.0 / temperature)))
        if learnable_temperature:
            self.log_scale = nn.Parameter(log_scale)
        else:
            self.log_scale = None
            self._scale = min(1.0 / float(temperature), self.max_scale)

    def scale(self):
        """(the logit scale in effect, whether log_scale is below the clamp)."""
        if self.log_scale is None:
            return self._scale, False
        v, top = float(self.log_scale.detach()), float(np.log(self.max_scale))
        return (float(np.exp(v)), True) if v <= top else (self.max_scale, False)

    def forward(self, student, teacher, groups=None):
        if student.dim() != 2 or student.shape != teacher.shape:
            raise ValueError(f"ContrastiveLoss: student {tuple(student.shape)} and teacher {tuple(teacher.shape)} must be equal [B,D]")
        if groups is not None and tuple(groups.shape) != (student.shape[0],):
            raise ValueError(f"ContrastiveLoss: groups {tuple(groups.shape)} must be [{student.shape[0]}]")
        scale, below = self.scale()
        fused = self.fused and _fusable(student, teacher) and (groups is None or groups.is_cuda)
        return _ContrastiveFn.apply(student, teacher, groups, self.log_scale, scale, below, self.w_s2t, self.w_t2s, fused)


class _BankContrastiveFn(torch.autograd.Function):
    """csn_bank_contrastive: like _ContrastiveFn the gradient is computed in the forward, saved, and multiplied by the
    incoming scalar; nothing crosses ranks.  ``log_scale`` is the learnable parameter or None; ``scale`` is the logit scale
    in effect and ``scale_grad`` whether the clamp lets a gradient through to ``log_scale``."""

    @staticmethod
    def forward(ctx, student, log_scale, pos, bank, inv_norm, group, scale, scale_grad):
        want_ds = ctx.needs_input_grad[0]
        want_dscale = log_scale is not None and ctx.needs_input_grad[1]
        _, loss, ds, dscale = cabi.bank_contrastive(student.detach(), bank, inv_norm, pos, scale, group, want_grad=want_ds,
                                                    want_dscale=want_dscale)
        ctx.want_ds, ctx.want_dscale = want_ds, want_dscale
        saved = [ds] if want_ds else []
        if want_dscale:         # d L / d log_scale = scale dL/dscale where the clamp at log(max_scale) is not in effect
            saved.append((dscale[0] * (scale if scale_grad else 0.0)).to(log_scale.dtype).reshape(log_scale.shape))
        ctx.save_for_backward(*saved)
        return loss[0].to(student.dtype)

    @staticmethod
    def backward(ctx, g):
        saved = ctx.saved_tensors
        ds = saved[0] * g if ctx.want_ds else None
        dlog = saved[-1] * g.to(saved[-1].dtype) if ctx.want_dscale else None
        return ds, dlog, None, None, None, None, None, None


class BankContrastiveLoss(nn.Module):
    """The contrastive loss (InfoNCE) of student rows against a fixed BANK: the frozen teacher's rows of the M distinct
    images of the dataset, L2-normalised like the student rows, at logit scale 1 / temperature:
        L = (1/B) sum_i [ lse_{m allowed}(a s^_i . t^_m) - a s^_i . t^_pos_i ].
    Every image is a negative of every query at every step, and with a frozen teacher the bank is exact, never stale.
    ``set_bank(bank[M,D], bank_group=None)`` keeps the bank (no copy) and computes its inverse norms once; they are computed
    again when another tensor is set or the tensor's ``_version`` changes.  ``bank_group`` ([M] integers, e.g. the class):
    key m is left out of query i when bank_group[m] == bank_group[pos_i] and m != pos_i.
    ``forward(student[B,D], pos[B])`` (``pos``: each row's positive as an index into the bank) returns the mean over the
    given rows.  The loss is a plain mean over rows, as the cosine loss is: micro-batches sum to the full batch, a ragged
    batch is fine, and there is no collective -- the mean all-reduce of the parameter gradients that FlatGrads / DDP perform
    gives the gradient of the global mean.  The bank gets no gradient.

    ``learnable_temperature=True`` keeps ``log_scale`` = log(1 / temperature) as an nn.Parameter, as ContrastiveLoss does:
    the scale in effect is exp(min(log_scale, log(max_scale))), its gradient scale * dL/dscale of the local rows.

    Default, and always for CPU or non-float32 tensors: torch ops in the dtype of the student rows (F.normalize x 2, one
    matmul, masked_fill(-inf), cross_entropy).  ``fused=True`` on float32 device tensors: value and gradient in float64
    from one csn_bank_contrastive call (six launches; four under no_grad), each float32 output rounded once."""

    def __init__(self, temperature=0.07, learnable_temperature=False, max_scale=100.0, fused=False):
        super().__init__()
        if not (temperature > 0 and np.isfinite(temperature)) or not (max_scale > 0 and np.isfinite(max_scale)):
            raise ValueError(f"BankContrastiveLoss: temperature {temperature} and max_scale {max_scale} must be finite and positive")
        self.max_scale, self.fused = float(max_scale), bool(fused)
        log_scale = torch.tensor(float(np.log(1.0 / temperature)))
        if learnable_temperature:
            self.log_scale = nn.Parameter(log_scale)
        else:
            self.log_scale = None
            self._scale = min(1.0 / float(temperature), self.max_scale)
        self.bank = self.bank_group = self._inv_norm = self._normed = None

    def scale(self):
        """(the logit scale in effect, whether log_scale is below the clamp)."""
        if self.log_scale is None:
            return self._scale, False
        v, top = float(self.log_scale.detach()), float(np.log(self.max_scale))
        return (float(np.exp(v)), True) if v <= top else (self.max_scale, False)

    def set_bank(self, bank, bank_group=None):
        if bank.dim() != 2 or bank.shape[0] < 1:
            raise ValueError(f"BankContrastiveLoss: bank {tuple(bank.shape)} must be [M,D]")
        if bank_group is not None:
            if tuple(bank_group.shape) != (bank.shape[0],) or bank_group.is_floating_point():
                raise ValueError(f"BankContrastiveLoss: bank_group {tuple(bank_group.shape)} {bank_group.dtype} must be "
                                 f"[{bank.shape[0]}] integers")
            bank_group = bank_group.to(device=bank.device, dtype=torch.int32).contiguous()
        self.bank, self.bank_group = bank.detach(), bank_group
        self._inv_norm = self._normed = None
        self.bank_inv_norm()

    def bank_inv_norm(self):
        """1 / max(|t_m|, 1e-12) of the bank rows, float64 [M]: csn_bank_norms for a float32 device bank, torch ops
        otherwise; computed once per (tensor, version)."""
        if self.bank is None:
            raise ValueError("BankContrastiveLoss: set_bank() first")
        key = (self.bank.data_ptr(), tuple(self.bank.shape), self.bank._version)
        if self._normed != key:
            if self.bank.is_cuda and self.bank.dtype == torch.float32:
                self._inv_norm = cabi.bank_norms(self.bank)
            else:
                self._inv_norm = 1.0 / self.bank.double().norm(dim=1).clamp_min(1e-12)
            self._normed = key
        return self._inv_norm

    def forward(self, student, pos):
        if self.bank is None:
            raise ValueError("BankContrastiveLoss: set_bank() first")
        if student.dim() != 2 or student.shape[1] != self.bank.shape[1]:
            raise ValueError(f"BankContrastiveLoss: student {tuple(student.shape)} must be [B,{self.bank.shape[1]}]")
        if tuple(pos.shape) != (student.shape[0],) or pos.is_floating_point():
            raise ValueError(f"BankContrastiveLoss: pos {tuple(pos.shape)} {pos.dtype} must be [{student.shape[0]}] integers")
        scale, below = self.scale()
        if self.fused and _fusable(student, self.bank, pos) and student.device == self.bank.device:
            inv_norm = self.bank_inv_norm()
            return _BankContrastiveFn.apply(student, self.log_scale, pos.to(torch.int32).contiguous(), self.bank, inv_norm,
                                            self.bank_group, scale, below)
        if self.log_scale is not None:
            scale = torch.exp(torch.clamp(self.log_scale, max=float(np.log(self.max_scale)))).to(student.dtype)
        pos = pos.long()
        bank = self.bank.to(student.dtype)
        z = scale * (F.normalize(student, dim=1, eps=1e-12) @ F.normalize(bank, dim=1, eps=1e-12).T)
        if self.bank_group is not None:
            keys = torch.arange(bank.shape[0], device=pos.device)
            out = (self.bank_group[None, :] == self.bank_group[pos][:, None]) & (keys[None, :] != pos[:, None])
            z = z.masked_fill(out, float("-inf"))
        return F.cross_entropy(z, pos)


class LARS(torch.optim.Optimizer):
    """Layer-wise adaptive rate scaling with the interface and semantics of the reference's optimizer
    (/root/reference/EEG-BarlowNetworks/optim.py:5-44): per parameter
        d = grad (+ weight_decay * p),   d *= eta |p| / |d|  (when both norms are positive),
        mu = momentum * mu + d,          p -= lr * mu,
    where the two ``*_filter`` switches exempt 1-D parameters (biases, norm scales) from the decay / the scaling.
    Written as a multi-tensor step: one fused ``_foreach`` call per phase over all parameters of a group instead
    of a Python loop of small kernels per parameter (the cfg2 model has 10 tensors, a DINO student 20+)."""

    def __init__(self, params, lr, weight_decay=0, momentum=0.9, eta=0.001, weight_decay_filter=False,
                 lars_adaptation_filter=False):
        super().__init__(params, dict(lr=lr, weight_decay=weight_decay, momentum=momentum, eta=eta,
                                      weight_decay_filter=weight_decay_filter,
                                      lars_adaptation_filter=lars_adaptation_filter))

    @staticmethod
    def exclude_bias_and_norm(p):
        return p.ndim == 1

    @torch.no_grad()
    def step(self):
        for group in self.param_groups:
            params = [p for p in group["params"] if p.grad is not None]
            if not params:
                continue
            one_d = [self.exclude_bias_and_norm(p) for p in params]
            updates = [p.grad.clone() for p in params]
            decayed = [i for i, flat in enumerate(one_d) if not (group["weight_decay_filter"] and flat)]
            if decayed and group["weight_decay"] != 0:
                torch._foreach_add_([updates[i] for i in decayed], [params[i] for i in decayed], alpha=group["weight_decay"])
            scaled = [i for i, flat in enumerate(one_d) if not (group["lars_adaptation_filter"] and flat)]
            if scaled:
                p_norm = torch.stack(torch._foreach_norm([params[i] for i in scaled]))
                u_norm = torch.stack(torch._foreach_norm([updates[i] for i in scaled]))
                trust = torch.where((p_norm > 0) & (u_norm > 0), group["eta"] * p_norm / u_norm, torch.ones_like(p_norm))
                torch._foreach_mul_([updates[i] for i in scaled], list(trust.unbind(0)))
            mus = []
            for p in params:
                state = self.state[p]
                if "mu" not in state:
                    state["mu"] = torch.zeros_like(p)
                mus.append(state["mu"])
            torch._foreach_mul_(mus, group["momentum"])
            torch._foreach_add_(mus, updates)
            torch._foreach_add_(params, mus, alpha=-group["lr"])


def barlow_learning_rate(step, epochs, steps_per_epoch, batch_size):
    """The schedule of adjust_learning_rate (EEG-BarlowNetworks/barlow_utils.py:8-21) before the per-group weights:
    linear warm-up over 10 epochs to batch_size / 256, then a cosine from there down to 0.1 % of it."""
    import math
    peak = batch_size / 256
    warm, total = 10 * steps_per_epoch, epochs * steps_per_epoch
    if step < warm:
        return peak * step / warm
    phase = 0.5 * (1 + math.cos(math.pi * (step - warm) / (total - warm)))
    return peak * phase + peak * 0.001 * (1 - phase)
