"""Oracle: stacked LSTM written out as an explicit recurrence (test infrastructure only).

Restates the arithmetic of ``torch.nn.LSTM(input, hidden, num_layers, batch_first=True)``
as the reference uses it (/root/reference/LSTMDistill.py:112-142,
/root/reference/LSTMDistillRetreival.py:85-110): zero initial state, gate order
i,f,g,o, parameters ``weight_ih_l{k}[4H,I] weight_hh_l{k}[4H,H] bias_ih_l{k}[4H]
bias_hh_l{k}[4H]``, followed by ``fc = Linear(H, D)`` on the last timestep (or
all timesteps) and the optional ``class_pred = Linear(D, n_classes)``.

Forward and the hand-derived backward are plain numpy (float64 by default) so
that the HIP kernels are checked against something that shares no code with
them.  Pinned against ``torch.nn.LSTM`` CPU outputs/grads in
tests/golden/lstm_*.npz.
"""
import numpy as np


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def lstm_forward(x_btc, params, num_layers, dtype=np.float64, return_saved=False):
    """x[B,T,I]; params: dict with torch.nn.LSTM key names (numpy arrays).

    Returns y[B,T,H] of the top layer (and the per-layer saved tensors).
    """
    x = np.asarray(x_btc, dtype=dtype)
    B, T, _ = x.shape
    saved = []
    inp = x
    for l in range(num_layers):
        w_ih = np.asarray(params[f"weight_ih_l{l}"], dtype)
        w_hh = np.asarray(params[f"weight_hh_l{l}"], dtype)
        bias = np.asarray(params[f"bias_ih_l{l}"], dtype) + np.asarray(params[f"bias_hh_l{l}"], dtype)
        H = w_hh.shape[1]
        h = np.zeros((B, H), dtype)
        c = np.zeros((B, H), dtype)
        hs = np.empty((B, T, H), dtype)
        gates = np.empty((B, T, 4 * H), dtype)
        cs = np.empty((B, T, H), dtype)
        for t in range(T):
            a = inp[:, t, :] @ w_ih.T + h @ w_hh.T + bias
            i = _sigmoid(a[:, 0 * H:1 * H])
            f = _sigmoid(a[:, 1 * H:2 * H])
            g = np.tanh(a[:, 2 * H:3 * H])
            o = _sigmoid(a[:, 3 * H:4 * H])
            c = f * c + i * g
            h = o * np.tanh(c)
            hs[:, t] = h
            cs[:, t] = c
            gates[:, t] = np.concatenate([i, f, g, o], axis=1)
        saved.append(dict(inp=inp, hs=hs, cs=cs, gates=gates))
        inp = hs
    if return_saved:
        return inp, saved
    return inp


def lstm_backward(dy_bth, params, saved, num_layers, dtype=np.float64):
    """Backward of :func:`lstm_forward`.  dy[B,T,H] = dLoss/dy(top layer, every step).

    Returns (dx[B,T,I], grads dict with torch key names).
    """
    grads = {}
    dout = np.asarray(dy_bth, dtype)
    for l in reversed(range(num_layers)):
        w_ih = np.asarray(params[f"weight_ih_l{l}"], dtype)
        w_hh = np.asarray(params[f"weight_hh_l{l}"], dtype)
        s = saved[l]
        inp, hs, cs, gates = s["inp"], s["hs"], s["cs"], s["gates"]
        B, T, H = hs.shape
        dh_rec = np.zeros((B, H), dtype)
        dc_next = np.zeros((B, H), dtype)
        da_all = np.empty((B, T, 4 * H), dtype)
        for t in reversed(range(T)):
            i = gates[:, t, 0 * H:1 * H]
            f = gates[:, t, 1 * H:2 * H]
            g = gates[:, t, 2 * H:3 * H]
            o = gates[:, t, 3 * H:4 * H]
            c = cs[:, t]
            c_prev = cs[:, t - 1] if t > 0 else np.zeros_like(c)
            tc = np.tanh(c)
            dh = dout[:, t] + dh_rec
            do = dh * tc
            dc = dh * o * (1.0 - tc * tc) + dc_next
            di = dc * g
            df = dc * c_prev
            dg = dc * i
            da = np.concatenate([di * i * (1 - i), df * f * (1 - f), dg * (1 - g * g), do * o * (1 - o)], axis=1)
            da_all[:, t] = da
            dh_rec = da @ w_hh
            dc_next = dc * f
        da2 = da_all.reshape(B * T, 4 * H)
        h_prev = np.concatenate([np.zeros((B, 1, H), dtype), hs[:, :-1]], axis=1).reshape(B * T, H)
        grads[f"weight_ih_l{l}"] = da2.T @ inp.reshape(B * T, -1)
        grads[f"weight_hh_l{l}"] = da2.T @ h_prev
        grads[f"bias_ih_l{l}"] = da2.sum(axis=0)
        grads[f"bias_hh_l{l}"] = da2.sum(axis=0)
        dout = (da2 @ w_ih).reshape(B, T, -1)
    return dout, grads


def model_forward(x_btc, params, num_layers, include_top=False, dtype=np.float64, return_saved=False):
    """``models.lstm.Model`` contract (precedent
    LSTMDistillRetreival.py:103-108): fc(lstm(x)[:, -1, :]) -> [B,D]; with
    ``include_top`` also class_pred(fc_out) -> [B,n_classes] (LSTMDistill.py:139-140).
    Param keys: ``lstm.*``, ``fc.weight/bias``, ``class_pred.weight/bias``.
    """
    lstm_p = {k[len("lstm."):]: v for k, v in params.items() if k.startswith("lstm.")}
    y, saved = lstm_forward(x_btc, lstm_p, num_layers, dtype, return_saved=True)
    last = y[:, -1, :]
    feat = last @ np.asarray(params["fc.weight"], dtype).T + np.asarray(params["fc.bias"], dtype)
    out = (feat,)
    if include_top:
        cls = feat @ np.asarray(params["class_pred.weight"], dtype).T + np.asarray(params["class_pred.bias"], dtype)
        out = (feat, cls)
    result = out if include_top else feat
    if return_saved:
        return result, dict(lstm=saved, y=y, last=last, feat=feat)
    return result


def model_backward(dfeat, params, saved, num_layers, dcls=None, dtype=np.float64):
    """Backward through head + LSTM.  Returns grads dict with ``Model`` key names."""
    grads = {}
    dfeat = np.asarray(dfeat, dtype).copy()
    feat, last, y = saved["feat"], saved["last"], saved["y"]
    if dcls is not None:
        dcls = np.asarray(dcls, dtype)
        grads["class_pred.weight"] = dcls.T @ feat
        grads["class_pred.bias"] = dcls.sum(axis=0)
        dfeat = dfeat + dcls @ np.asarray(params["class_pred.weight"], dtype)
    grads["fc.weight"] = dfeat.T @ last
    grads["fc.bias"] = dfeat.sum(axis=0)
    dlast = dfeat @ np.asarray(params["fc.weight"], dtype)
    dy = np.zeros_like(y)
    dy[:, -1, :] = dlast
    lstm_p = {k[len("lstm."):]: v for k, v in params.items() if k.startswith("lstm.")}
    dx, g = lstm_backward(dy, lstm_p, saved["lstm"], num_layers, dtype)
    for k, v in g.items():
        grads["lstm." + k] = v
    return dx, grads


def reference_lstm_model(x_b_ts_ch, params, num_layers, target=None, dtype=np.float64):
    """``LSTMModel`` of LSTMDistillRetreival.py:85-110: the input [B, timespan, channels] is *viewed* (memory
    reinterpreted, not transposed) as [B, channels, timespan] (:97-98), i.e. the recurrence runs over ``channels``
    steps with ``timespan`` features; zero initial state; fc on the last step.  With ``target``: also the
    CosineSimilarityLoss (LstmDistillFromDinoV2Train.py:36-43) and every parameter gradient.
    """
    from . import losses
    x = np.ascontiguousarray(np.asarray(x_b_ts_ch))
    B, TS, CH = x.shape
    seq = x.reshape(B, CH, TS)
    feat, saved = model_forward(seq, params, num_layers, dtype=dtype, return_saved=True)
    if target is None:
        return feat
    loss = losses.cosine_similarity_loss(feat, target)
    _, grads = model_backward(losses.cosine_similarity_loss_grad(feat, target), params, saved, num_layers, dtype=dtype)
    return feat, loss, grads


def reference_lstm_model_all_steps(x_b_ts_ch, params, num_layers, dfeat=None, dcls=None, dtype=np.float64):
    """``LSTMModel`` of LSTMDistill.py:112-142: same view, then fc on EVERY step, class_pred on the un-rectified
    fc output, ReLU on the returned features (:137-141).  With (dfeat, dcls) = dLoss/d(returned feat, cls):
    the parameter gradients.
    """
    x = np.ascontiguousarray(np.asarray(x_b_ts_ch))
    B, TS, CH = x.shape
    seq = x.reshape(B, CH, TS)
    lstm_p = {k[len("lstm."):]: v for k, v in params.items() if k.startswith("lstm.")}
    y, saved = lstm_forward(seq, lstm_p, num_layers, dtype, return_saved=True)            # [B, CH, H]
    wf, bf = np.asarray(params["fc.weight"], dtype), np.asarray(params["fc.bias"], dtype)
    wc, bc = np.asarray(params["class_pred.weight"], dtype), np.asarray(params["class_pred.bias"], dtype)
    pre = y @ wf.T + bf
    cls = pre @ wc.T + bc
    feat = np.maximum(pre, 0.0)
    if dfeat is None:
        return feat, cls
    dpre = np.asarray(dfeat, dtype) * (pre > 0) + np.asarray(dcls, dtype) @ wc
    grads = {"class_pred.weight": np.einsum("btn,btd->nd", np.asarray(dcls, dtype), pre),
             "class_pred.bias": np.asarray(dcls, dtype).sum(axis=(0, 1)),
             "fc.weight": np.einsum("btd,bth->dh", dpre, y), "fc.bias": dpre.sum(axis=(0, 1))}
    _, g = lstm_backward(dpre @ wf, lstm_p, saved, num_layers, dtype)
    for k, v in g.items():
        grads["lstm." + k] = v
    return feat, cls, grads


def init_params(input_size, hidden, num_layers, out_features, n_classes=None, seed=43, dtype=np.float32):
    """Deterministic numpy init with nn.LSTM / nn.Linear's U(-1/sqrt(fan), 1/sqrt(fan)) ranges."""
    rng = np.random.default_rng(seed)
    p = {}
    k = 1.0 / np.sqrt(hidden)
    for l in range(num_layers):
        i_sz = input_size if l == 0 else hidden
        p[f"lstm.weight_ih_l{l}"] = rng.uniform(-k, k, (4 * hidden, i_sz)).astype(dtype)
        p[f"lstm.weight_hh_l{l}"] = rng.uniform(-k, k, (4 * hidden, hidden)).astype(dtype)
        p[f"lstm.bias_ih_l{l}"] = rng.uniform(-k, k, (4 * hidden,)).astype(dtype)
        p[f"lstm.bias_hh_l{l}"] = rng.uniform(-k, k, (4 * hidden,)).astype(dtype)
    p["fc.weight"] = rng.uniform(-k, k, (out_features, hidden)).astype(dtype)
    p["fc.bias"] = rng.uniform(-k, k, (out_features,)).astype(dtype)
    if n_classes:
        kc = 1.0 / np.sqrt(out_features)
        p["class_pred.weight"] = rng.uniform(-kc, kc, (n_classes, out_features)).astype(dtype)
        p["class_pred.bias"] = rng.uniform(-kc, kc, (n_classes,)).astype(dtype)
    return p


# ----------------------------------------------------------------------------------------------
# bf16-faithful emulation of the HIP kernels' bf16 path
# ----------------------------------------------------------------------------------------------
# The float64 oracle above rounds nothing, so the bf16 kernels can only be held to it within the ~2e-3 (of the norm)
# that bf16 quantisation alone costs.  The functions below round exactly where the bf16 kernels round and compute in
# float64 everywhere else, so what is left between a kernel and them is float32 accumulation order, the fast
# exp2 / rcp activations and the bf16 rounding flips those cause -- 10-100 x less than the quantisation.
# Rounding points (the same in every bf16 kernel: lstm_cell.hip v1 cells, lstm_cell_blk.hip per-diagonal cells,
# lstm_fwd_persist.hip K-split, lstm_fwd_ns.hip N-split, fused x or projection GEMM, lstm_bwd_persist.hip):
#   * x, W_ih, W_hh -> bf16 (round to nearest even, float32 -> bf16); bias = b_ih + b_hh summed in float32;
#   * forward: the pre-activations and gates are float32 (not rounded), c is float32, h_t is rounded to bf16 and that
#     value is the next step's recurrent operand, the next layer's input and the output (y_all / y_last);
#   * the gates saved for the backward are the post-activation gates rounded to bf16;
#   * backward: bf16 saved gates, tanh(c) recomputed from the float32 c, dc carried in float32, the gate gradients
#     (dgates) rounded to bf16 -- that bf16 value feeds dh_{t-1} = dgates W_hh, dx = dgates W_ih (float32 out, the dy
#     of the layer below), dW_ih = dgates^T inp (bf16 layer input), dW_hh = dgates^T h_{t-1} (bf16) and db.
# State (CSN_LSTM_STATE plans; the same on every path -- v1 cells, per-diagonal cells, weight-stationary -- so no switch):
#   * h0 -> bf16 where the host writes slot 0 of h_all (lstm.hip:589 forward_v1, :894-895 forward_il, :1053-1054
#     forward_persist); that value is step 0's recurrent operand and the h_{-1} of dW_hh (lstm.hip:695, :1188, :1348);
#   * c0 float32, copied into slot 0 of c_all (lstm.hip:594, :898, :1060): step 0's c_prev and the backward's df_0
#     (lstm.hip:671 v1, :1238 per-diagonal, lstm_bwd_persist.hip:204);
#   * h_n = the bf16 h of slot T upcast (lstm.hip:1525), c_n = the float32 c of slot T (lstm.hip:1528);
#   * dh_n[L-1] is added in float32 to row T-1 of the top layer's dy, after dy_last (lstm.hip:1588, :1593; it IS that row
#     when dy_all and dy_last are NULL, :1597); dh_n[l < L-1] is added in float32 to row T-1 of layer l+1's float32 dx,
#     i.e. the dy of layer l (lstm.hip:684, :1267, :1332);
#   * dc_n seeds the float32 carried dc (lstm.hip:647, :1171, :1327); dc0 = that carry after step 0 (lstm.hip:1623);
#   * dh0 = bf16 dgates_0 . bf16 W_hh with a float32 result (lstm_dh0_kernel, lstm.hip:224, launched at :1615-1619).
#   NULL means zeros for every one of them.
# With ``rounding=False`` every rounding is the identity and the results are those of lstm_forward / lstm_backward (with
# a state: those of float64 torch.nn.LSTM given (h0, c0)).

def bf16_round(a):
    """Round to the nearest bf16 value (ties to even) the way the kernels' ``(bf16_t)float`` cast does: the value is
    first a float32 (what the kernel holds), then the low 16 bits are rounded away.  Returns float64.  NaN stays NaN,
    +-inf stay, finite values past the largest bf16 round to +-inf, float32 subnormals round like any other value."""
    f = np.ascontiguousarray(np.asarray(a, np.float64).astype(np.float32))
    u = f.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    out = r.view(np.float32).astype(np.float64)
    nan = np.isnan(f)
    if nan.any():
        out[nan] = np.nan
    return out.reshape(np.shape(a))


def f32_round(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def _rounders(rounding):
    if rounding:
        return bf16_round, f32_round
    ident = lambda v: np.asarray(v, np.float64)      # noqa: E731
    return ident, ident


def lstm_forward_bf16(x_btc, params, num_layers, rounding=True, acc=np.float64, defect=None, h0=None, c0=None):
    """Forward of the bf16 kernels (rounding points above).  x[B,T,I]; params with torch.nn.LSTM key names; h0, c0:
    [L,B,H] initial state or None (zeros).  Returns (y[B,T,H] of the top layer -- bf16 values --, saved) for
    :func:`lstm_backward_bf16`; :func:`final_state` gives (h_n, c_n) from `saved`.

    For the tests of the tests: ``acc=np.float32`` runs the two products in float32 (a stand-in for a kernel's own
    accumulation noise); ``defect(kind, l, t, value, hs)`` may replace the recurrent operand (kind "h_prev", value
    h_{t-1}, hs = the layer's h of the steps before), the gates (kind "gates", value (i, f, g, o)) or the h a step
    publishes (kind "h", value h_t); it returns the value to use."""
    rb, rf = _rounders(rounding)
    inp = rb(x_btc)
    B, T, _ = inp.shape
    saved = []
    for l in range(num_layers):
        w_ih = rb(params[f"weight_ih_l{l}"])
        w_hh = rb(params[f"weight_hh_l{l}"])
        if rounding:
            bias = (np.asarray(params[f"bias_ih_l{l}"], np.float32) + np.asarray(params[f"bias_hh_l{l}"], np.float32)).astype(np.float64)
        else:
            bias = np.asarray(params[f"bias_ih_l{l}"], np.float64) + np.asarray(params[f"bias_hh_l{l}"], np.float64)
        H = w_hh.shape[1]
        h = np.zeros((B, H)) if h0 is None else rb(np.asarray(h0)[l])
        c = np.zeros((B, H)) if c0 is None else rf(np.asarray(c0)[l])
        h_init, c_init = h, c
        hs = np.empty((B, T, H))
        gates = np.empty((B, T, 4 * H))
        cs = np.empty((B, T, H))
        xp =(inp.reshape(B * T, -1).astype(acc) @ w_ih.T.astype(acc)).astype(np.float64).reshape(B, T, 4 * H)
        w_hh_t = w_hh.T.astype(acc)
        for t in range(T):
            hp = h if defect is None else defect("h_prev", l, t, h, hs[:, :t])
            a = xp[:, t] + (hp.astype(acc) @ w_hh_t).astype(np.float64) + bias
            i = _sigmoid(a[:, 0 * H:1 * H])
            f = _sigmoid(a[:, 1 * H:2 * H])
            g = np.tanh(a[:, 2 * H:3 * H])
            o = _sigmoid(a[:, 3 * H:4 * H])
            if defect is not None:
                i, f, g, o = defect("gates", l, t, (i, f, g, o), None)
            c = rf(f * c + i * g)
            h = rb(o * np.tanh(c))
            if defect is not None:
                h = defect("h", l, t, h, hs[:, :t])
            hs[:, t] = h
            cs[:, t] = c
            gates[:, t, 0 * H:1 * H] = i
            gates[:, t, 1 * H:2 * H] = f
            gates[:, t, 2 * H:3 * H] = g
            gates[:, t, 3 * H:4 * H] = o
        saved.append(dict(inp=inp, hs=hs, cs=cs, gates=rb(gates), w_ih=w_ih, w_hh=w_hh, h0=h_init, c0=c_init))
        inp = hs
    return inp, saved


def final_state(saved):
    """(h_n, c_n) [L,B,H] of a :func:`lstm_forward_bf16` run: each layer's h (bf16 values) and c after the last step."""
    return np.stack([s["hs"][:, -1] for s in saved]), np.stack([s["cs"][:, -1] for s in saved])


def lstm_backward_bf16(dy_bth, saved, num_layers, rounding=True, dh_n=None, dc_n=None, return_state=False):
    """Backward of the bf16 kernels.  dy[B,T,H] = dLoss/dy of the top layer (float32 values, as the caller hands them
    over: dy_all with dy_last added to row T-1); dh_n, dc_n: [L,B,H] gradients w.r.t. h_n / c_n or None (zeros).
    Returns (dx[B,T,I], grads with torch key names, dgates per layer [B,T,4H] (bf16 values)); with ``return_state``
    also dh0 and dc0 [L,B,H], the gradients w.r.t. the initial state (zero or not)."""
    rb, rf = _rounders(rounding)
    grads, dgates = {}, {}
    dout = np.array(dy_bth, np.float64)
    B, T, H = saved[-1]["hs"].shape
    dh0, dc0 = np.empty((num_layers, B, H)), np.empty((num_layers, B, H))
    for l in reversed(range(num_layers)):
        if dh_n is not None:        # layer l's dy row T-1: dy_all + dy_last (top) or layer l+1's dx, then + dh_n[l]
            dout[:, T - 1] = rf(dout[:, T - 1] + np.asarray(dh_n, np.float64)[l])
        s = saved[l]
        inp, hs, cs, gates, w_ih, w_hh = s["inp"], s["hs"], s["cs"], s["gates"], s["w_ih"], s["w_hh"]
        dh_rec = np.zeros((B, H))
        dc_next = np.zeros((B, H)) if dc_n is None else rf(np.asarray(dc_n)[l])
        da_all = np.empty((B, T, 4 * H))
        for t in reversed(range(T)):
            i = gates[:, t, 0 * H:1 * H]
            f = gates[:, t, 1 * H:2 * H]
            g = gates[:, t, 2 * H:3 * H]
            o = gates[:, t, 3 * H:4 * H]
            c = cs[:, t]
            c_prev = cs[:, t - 1] if t > 0 else s["c0"]
            tc = np.tanh(c)
            dh = dout[:, t] + dh_rec
            do = dh * tc
            dc = dh * o * (1.0 - tc * tc) + dc_next
            da = rb(np.concatenate([dc * g * i * (1 - i), dc * c_prev * f * (1 - f), dc * i * (1 - g * g),
                                    do * o * (1 - o)], axis=1))
            da_all[:, t] = da
            dh_rec = da @ w_hh
            dc_next = rf(dc * f)
        dh0[l], dc0[l] = rf(dh_rec), dc_next          # past step 0
        da2 = da_all.reshape(B * T, 4 * H)
        h_prev = np.concatenate([s["h0"][:, None], hs[:, :-1]], axis=1).reshape(B * T, H)
        grads[f"weight_ih_l{l}"] = da2.T @ inp.reshape(B * T, -1)
        grads[f"weight_hh_l{l}"] = da2.T @ h_prev
        grads[f"bias_ih_l{l}"] = da2.sum(axis=0)
        grads[f"bias_hh_l{l}"] = da2.sum(axis=0)
        dgates[l] = da_all
        dout = rf(da2 @ w_ih).reshape(B, T, -1)
    if return_state:
        return dout, grads, dgates, dh0, dc0
    return dout, grads, dgates
