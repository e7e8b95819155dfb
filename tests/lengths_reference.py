"""References for variable-length LSTM batches, shared by tests/test_lstm_lengths_cpu.py and tests/test_gpu_lstm_lengths.py
(not a test module).  Both are built from parts that exist without the feature: float64 torch.nn.LSTM on the packed batch,
and the unmodified bf16-faithful emulator (oracle.lstm) run on each row's valid steps alone -- rows of an LSTM batch are
independent, so a ragged batch IS its rows run one by one, with the parameter gradients summed."""
import numpy as np
import torch
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

from oracle import lstm as olstm


def packed_nn_lstm(ref, x, lengths, h0, c0, dy, dh, dc):
    """float64 nn.LSTM `ref` (CPU) on pack_padded_sequence(enforce_sorted=False) of the rows with n > 0, padded back to T;
    rows with n = 0 (which torch refuses) are left out and get their pass-through values: zero output, (h_n, c_n) =
    (h0, c0).  Loss <out, dy> + <h_n, dh> + <c_n, dc>.  Tensors are float64 CPU; returns outputs and every gradient."""
    B, T = x.shape[0], x.shape[1]
    lengths = [int(n) for n in lengths]
    keep = [b for b, n in enumerate(lengths) if n > 0]
    x = x.clone().requires_grad_(True)
    h0 = h0.clone().requires_grad_(True)
    c0 = c0.clone().requires_grad_(True)
    for p in ref.parameters():
        p.grad = None
    out = torch.zeros(B, T, ref.hidden_size, dtype=torch.float64)
    h_n, c_n = h0.clone(), c0.clone()
    if keep:
        packed = pack_padded_sequence(x[keep], torch.tensor([lengths[b] for b in keep]), batch_first=True,
                                      enforce_sorted=False)
        out_p, (h_k, c_k) = ref(packed, (h0[:, keep].contiguous(), c0[:, keep].contiguous()))
        out_k, _ = pad_packed_sequence(out_p, batch_first=True, total_length=T)
        out[keep] = out_k
        h_n[:, keep] = h_k
        c_n[:, keep] = c_k
    ((out * dy).sum() + (h_n * dh).sum() + (c_n * dc).sum()).backward()
    grads = {k: (p.grad if p.grad is not None else torch.zeros_like(p)).detach().clone() for k, p in ref.named_parameters()}
    dx = x.grad if x.grad is not None else torch.zeros_like(x)          # (no row ran: nothing reached x)
    return dict(out=out.detach(), h_n=h_n.detach(), c_n=c_n.detach(), dx=dx, dh0=h0.grad, dc0=c0.grad, **grads)


def rows_emulator(lp, L, x, lengths, h0, c0, dy, dh, dc, rounding=True, per_row=False):
    """The emulator (oracle.lstm.lstm_forward_bf16 / lstm_backward_bf16, unmodified) on x[rows, :n] for the rows of each
    distinct length n (``per_row``: for every row on its own) with those rows' state and gradients; parameter gradients
    summed over the runs.  n = 0: the row passes through (h_n = h0 -- bf16-rounded when rounding --, c_n = c0, dh0 = dh,
    dc0 = dc).  numpy in, numpy float64 out, the keys of packed_nn_lstm."""
    x, h0, c0, dy, dh, dc = (np.asarray(a) for a in (x, h0, c0, dy, dh, dc))
    B, T, I = x.shape
    H = h0.shape[2]
    lengths = [int(n) for n in lengths]
    res = dict(out=np.zeros((B, T, H)), h_n=np.zeros((L, B, H)), c_n=np.zeros((L, B, H)), dx=np.zeros((B, T, I)),
               dh0=np.zeros((L, B, H)), dc0=np.zeros((L, B, H)))
    groups = [[b] for b in range(B)] if per_row else [[b for b in range(B) if lengths[b] == n] for n in sorted(set(lengths))]
    dt = np.float32 if rounding else np.float64       # (the library forms dy in float32)
    for rows in groups:
        n = lengths[rows[0]]
        if n == 0:
            res["h_n"][:, rows] = olstm.bf16_round(h0[:, rows]) if rounding else h0[:, rows]
            res["c_n"][:, rows] = c0[:, rows]
            res["dh0"][:, rows] = dh[:, rows]
            res["dc0"][:, rows] = dc[:, rows]
            continue
        y, saved = olstm.lstm_forward_bf16(x[rows, :n], lp, L, rounding=rounding, h0=h0[:, rows], c0=c0[:, rows])
        h_n, c_n = olstm.final_state(saved)
        dx, g, _, dh0, dc0 = olstm.lstm_backward_bf16(dy[rows, :n].astype(dt), saved, L, rounding=rounding,
                                                     dh_n=dh[:, rows], dc_n=dc[:, rows], return_state=True)
        res["out"][rows, :n] = y
        res["dx"][rows, :n] = dx
        for k, v in (("h_n", h_n), ("c_n", c_n), ("dh0", dh0), ("dc0", dc0)):
            res[k][:, rows] = v
        for k, v in g.items():
            res[k] = res.get(k, 0.0) + np.asarray(v, np.float64)
    if not any(lengths):          # no row ran: zero parameter gradients of the right shapes
        for k, v in lp.items():
            res[k] = np.zeros(np.shape(v))
    return res
