"""References for the LSTM's inter-layer dropout, shared by tests/test_lstm_dropout_cpu.py and tests/test_gpu_lstm_dropout.py
(not a test module).  Built from parts that exist without the feature: a numpy Philox4x32-10 and keep rule written from
the specification in include/csn_hip.h (csn_lstm_plan_set_dropout), the unmodified bf16-faithful emulator (oracle.lstm)
run ONE LAYER AT A TIME with the mask and scale applied between the runs, and a float64 chain of single-layer
torch.nn.LSTMs with the same mask."""
import numpy as np
import torch

from oracle import lstm as olstm

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LO = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """counter: 4 uint32 arrays (or ints) of one shape, key: 2 ints -> 4 uint32 arrays.  Ten rounds; the key is bumped by
    the Weyl constants between rounds."""
    c = [np.atleast_1d(np.asarray(v, np.uint64)) & _LO for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = _M0 * c[0], _M1 * c[2]             # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> _S32) ^ c[1] ^ np.uint64(k0), p1 & _LO, (p0 >> _S32) ^ c[3] ^ np.uint64(k1), p0 & _LO]
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return [v.astype(np.uint32) for v in c]


def threshold(p):
    """thr of the keep rule: floor(float32(p) 2^32) -- exact in float64; 2^32 at p = 1 (no word reaches it)."""
    return int(np.floor(np.float64(np.float32(p)) * 4294967296.0))


def scale(p):
    """s = 1.0f / (1.0f - p) in float32 arithmetic (as a Python float; inf at p = 1)."""
    with np.errstate(divide="ignore"):
        return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def keep(seed, subsequence, p, first, n):
    """keep[i] (bool) of element e = first + i, i in [0, n): word e & 3 of philox(counter (lo32(e >> 2), hi32(e >> 2),
    subsequence, 0), key (lo32(seed), hi32(seed))) >= thr."""
    e = np.uint64(first) + np.arange(n, dtype=np.uint64)
    quad = e >> np.uint64(2)
    uq, inv = np.unique(quad, return_inverse=True)
    words = philox4x32_10((uq & _LO, uq >> _S32, int(subsequence), 0), (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF))
    w = np.stack(words, axis=1)[inv, (e & np.uint64(3)).astype(np.int64)]
    return w.astype(np.uint64) >= np.uint64(threshold(p))


def interface_masks(seed, subsequence, p, L, T, B, H):
    """[L-1, B, T, H] bool (batch-first, as the emulator holds a layer's outputs): element (l, t, b, u) has the index
    e = ((l T + t) B + b) H + u."""
    k = keep(seed, subsequence, p, 0, (L - 1) * T * B * H).reshape(L - 1, T, B, H)
    return np.ascontiguousarray(k.transpose(0, 2, 1, 3))


def _layer_params(lp, l):
    return {f"{n}_l0": lp[f"{n}_l{l}"] for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")}


def composed_emulator(lp, L, x, h0, c0, dy, dh, dc, masks, s, rounding=True):
    """The stack as L runs of the emulator's single-layer forward / backward (layer l's parameters re-keyed as _l0, with
    h0[l:l+1], dh_n[l:l+1], dc_n[l:l+1]).  Between the runs, with masks[l] [B,T,H] bool and the float32 scale s:
      forward : input of layer l+1 = keep ? bf16(float32(h * s)) : 0   (rounding=False: h * s in float64)
      backward: dy of layer l = keep ? float32(dx_{l+1} * s) : 0, before dh_n[l] joins it (the single-layer run adds it).
    masks = None: nothing between the runs.  numpy in; float64 out with the keys of test_gpu_lstm_state._run."""
    rb, rf = olstm._rounders(rounding)
    x = np.asarray(x)
    h0 = np.zeros((L,) + (x.shape[0], lp["weight_hh_l0"].shape[1])) if h0 is None else np.asarray(h0)
    c0 = np.zeros_like(h0) if c0 is None else np.asarray(c0)
    inp, saved = x, []
    for l in range(L):
        y, sv = olstm.lstm_forward_bf16(inp, _layer_params(lp, l), 1, rounding=rounding, h0=h0[l:l + 1], c0=c0[l:l + 1])
        saved.append(sv)
        inp = y
        if masks is not None and l + 1 < L:
            inp = np.where(masks[l], rb(rf(y * s)) if np.isfinite(s) else 0.0, 0.0)
    h_n = np.concatenate([olstm.final_state(sv)[0] for sv in saved])
    c_n = np.concatenate([olstm.final_state(sv)[1] for sv in saved])
    res = dict(out=y, h_n=h_n, c_n=c_n)
    if dy is None:
        return res
    grads, dh0, dc0 = {}, [None] * L, [None] * L
    dout = np.asarray(dy, np.float32 if rounding else np.float64)
    for l in reversed(range(L)):
        dout, g, _, a, b = olstm.lstm_backward_bf16(dout, saved[l], 1, rounding=rounding, dh_n=None if dh is None else np.asarray(dh)[l:l + 1],
                                                    dc_n=None if dc is None else np.asarray(dc)[l:l + 1], return_state=True)
        dh0[l], dc0[l] = a[0], b[0]
        for k, v in g.items():
            grads[k.replace("_l0", f"_l{l}")] = v
        if masks is not None and l > 0:
            dout = np.where(masks[l - 1], rf(dout * s) if np.isfinite(s) else 0.0, 0.0)
    res.update(dx=dout, dh0=np.stack(dh0), dc0=np.stack(dc0), **grads)
    return res


def rows_composed_emulator(lp, L, x, lengths, h0, c0, dy, dh, dc, masks, s, rounding=True):
    """composed_emulator on x[rows, :n] for the rows of each distinct length n, with those rows' state, gradients and rows
    of the mask (masks [L-1,B,T,H] over the plan's T: the mask of the call without lengths); parameter gradients summed.
    n = 0 passes the row through, as tests/lengths_reference.rows_emulator does."""
    x, h0, c0, dy, dh, dc = (np.asarray(a) for a in (x, h0, c0, dy, dh, dc))
    B, T, I = x.shape
    H = h0.shape[2]
    lengths = [int(n) for n in lengths]
    res = dict(out=np.zeros((B, T, H)), h_n=np.zeros((L, B, H)), c_n=np.zeros((L, B, H)), dx=np.zeros((B, T, I)),
               dh0=np.zeros((L, B, H)), dc0=np.zeros((L, B, H)))
    for n in sorted(set(lengths)):
        rows = [b for b in range(B) if lengths[b] == n]
        if n == 0:
            res["h_n"][:, rows] = olstm.bf16_round(h0[:, rows]) if rounding else h0[:, rows]
            res["c_n"][:, rows] = c0[:, rows]
            res["dh0"][:, rows] = dh[:, rows]
            res["dc0"][:, rows] = dc[:, rows]
            continue
        r = composed_emulator(lp, L, x[rows, :n], h0[:, rows], c0[:, rows], dy[rows, :n], dh[:, rows], dc[:, rows],
                              None if masks is None else masks[:, rows, :n], s, rounding=rounding)
        res["out"][rows, :n] = r["out"]
        res["dx"][rows, :n] = r["dx"]
        for k in ("h_n", "c_n", "dh0", "dc0"):
            res[k][:, rows] = r[k]
        for k in lp:
            res[k] = res.get(k, 0.0) + np.asarray(r[k], np.float64)
    if not any(lengths):
        for k, v in lp.items():
            res[k] = np.zeros(np.shape(v))
    return res


def nn_lstm_chain(lp, L, x, h0, c0, dy, dh, dc, masks, s, dtype=torch.float64):
    """A chain of L single-layer torch.nn.LSTMs (CPU, `dtype`) holding the layers' parameters, the output of layer l
    multiplied by masks[l] * s before layer l+1; loss <out, dy> + <h_n, dh> + <c_n, dc>.  The keys of composed_emulator,
    as float64 numpy."""
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=dtype)      # noqa: E731
    x = t(x).clone().requires_grad_(True)
    B = x.shape[0]
    H = lp["weight_hh_l0"].shape[1]
    h0 = (torch.zeros(L, B, H, dtype=dtype) if h0 is None else t(h0)).clone().requires_grad_(True)
    c0 = (torch.zeros(L, B, H, dtype=dtype) if c0 is None else t(c0)).clone().requires_grad_(True)
    layers, inp, hs, cs = [], x, [], []
    for l in range(L):
        m = torch.nn.LSTM(lp[f"weight_ih_l{l}"].shape[1], H, 1, batch_first=True).to(dtype)
        m.load_state_dict({k: t(v) for k, v in _layer_params(lp, l).items()})
        layers.append(m)
        y, (h, c) = m(inp, (h0[l:l + 1], c0[l:l + 1]))
        hs.append(h)
        cs.append(c)
        inp = y
        if masks is not None and l + 1 < L:
            inp = torch.where(torch.as_tensor(masks[l]), y * s, torch.zeros_like(y)) if np.isfinite(s) else torch.zeros_like(y) * y
    h_n, c_n = torch.cat(hs), torch.cat(cs)
    loss = (y * t(dy)).sum()
    if dh is not None:
        loss = loss + (h_n * t(dh)).sum()
    if dc is not None:
        loss = loss + (c_n * t(dc)).sum()
    loss.backward()
    n = lambda a: a.detach().double().numpy()      # noqa: E731
    res = dict(out=n(y), h_n=n(h_n), c_n=n(c_n), dx=n(x.grad), dh0=n(h0.grad), dc0=n(c0.grad))
    for l, m in enumerate(layers):
        for k, p in m.named_parameters():
            res[k.replace("_l0", f"_l{l}")] = n(p.grad) if p.grad is not None else np.zeros(tuple(p.shape))
    return res
