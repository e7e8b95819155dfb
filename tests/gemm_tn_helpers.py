"""Shared by tests/test_gpu_gemm_tn_w4.py and tests/test_gpu_gemm_tn_splits.py (not a test module): the environment
switch holder, the float64 product, and the pieces of one bf16 LSTM plan's weight and bias gradients."""
import os

import numpy as np
import torch

from cerebralsignalnetworks_amd import cabi


class env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def float64_product(a, b, rows=512):
    """a^T b in float64 from the bf16 operands, by row blocks of the result (the float64 copies stay small)."""
    b64 = b.double()
    out = torch.empty(a.shape[1], b.shape[1], dtype=torch.float64, device=a.device)
    for m in range(0, a.shape[1], rows):
        out[m:m + rows] = a[:, m:m + rows].double().t() @ b64
    return out


def plan_inputs(cuda, B, T, C, H, L):
    """Parameters (four groups of L float32 tensors), input and incoming gradients of plan_gradients."""
    g = torch.Generator(device=cuda).manual_seed(B + T + H)
    k = 1.0 / np.sqrt(H)

    def uni(*s):
        return (torch.rand(*s, device=cuda, generator=g) * 2 - 1) * k

    w_ih = [uni(4 * H, C if l == 0 else H) for l in range(L)]
    w_hh = [uni(4 * H, H) for l in range(L)]
    b_ih = [uni(4 * H) for l in range(L)]
    b_hh = [uni(4 * H) for l in range(L)]
    x = torch.randn(B, T, C, device=cuda, generator=g)
    dy_all = torch.randn(B, T, H, device=cuda, generator=g) * 0.1
    dy_last = torch.randn(B, H, device=cuda, generator=g)
    return (w_ih, w_hh, b_ih, b_hh), x, dy_all, dy_last


def plan_create(cuda, B, T, C, H, L, switches, params, x):
    """A bf16 LSTM plan created under `switches` (a plan reads its options once), after its forward."""
    with env(**switches):
        plan = cabi.LstmPlan(B, T, C, H, L, torch.bfloat16, cuda)
    plan.forward(x, *params, want_all=True)
    return plan


def plan_backward(plan, params, dy_last, dy_all):
    """Weight and bias gradients of one backward of `plan`, into tensors that held NaN."""
    grads = [[torch.full_like(p, float("nan")) for p in group] for group in params]
    plan.backward(dy_last, dy_all, grads)
    torch.cuda.synchronize()
    assert plan.status() == 0
    return {f"{name}_l{l}": t.cpu().numpy() for name, group in zip(("dw_ih", "dw_hh", "db_ih", "db_hh"), grads)
            for l, t in enumerate(group)}


def plan_gradients(cuda, B, T, C, H, L, switches):
    """Weight and bias gradients of one bf16 LSTM plan created under `switches`."""
    params, x, dy_all, dy_last = plan_inputs(cuda, B, T, C, H, L)
    return plan_backward(plan_create(cuda, B, T, C, H, L, switches, params, x), params, dy_last, dy_all)
