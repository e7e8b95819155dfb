"""References for the bidirectional LSTM, shared by tests/test_bilstm_cpu.py and tests/test_gpu_bilstm.py (not a test
module).  All of it is built from parts that exist without the feature: the per-row time reversal R as a torch index
gather, the bidirectional stack COMPOSED from plain single-layer LSTM calls on explicitly reversed tensors, and float64
torch.nn.LSTM(bidirectional=True) on the packed batch."""
import torch
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

NAMES = ("weight_ih", "weight_hh", "bias_ih", "bias_hh")


def R(t, lengths=None):
    """t[B, T, ...] with the first lengths[b] steps of every row b reversed and the rest left where it is (lengths = None:
    every row is T).  Differentiable; R(R(t)) = t."""
    B, T = t.shape[0], t.shape[1]
    n = torch.full((B,), T, dtype=torch.int64) if lengths is None else torch.tensor([int(v) for v in lengths], dtype=torch.int64)
    steps = torch.arange(T).expand(B, T)
    idx = torch.where(steps < n[:, None], n[:, None] - 1 - steps, steps).to(t.device)
    return t[torch.arange(B, device=t.device)[:, None], idx]


def sub_name(name):
    """Parameter name of a bidirectional nn.LSTM -> (layer, direction, name in a single-layer unidirectional LSTM)."""
    base, rest = name.rsplit("_l", 1)
    rev = rest.endswith("_reverse")
    return int(rest[:-len("_reverse")] if rev else rest), int(rev), base + "_l0"


def single_layer_modules(bi, make):
    """layers[l][d] = make(input width, H): a single-layer unidirectional LSTM module holding copies of the parameters of
    layer l, direction d of the bidirectional module `bi` (nn.LSTM's names)."""
    H, L = bi.hidden_size, bi.num_layers
    sd = bi.state_dict()
    layers = []
    for l in range(L):
        pair = []
        for sfx in ("", "_reverse"):
            m = make(sd[f"weight_ih_l{l}{sfx}"].shape[1], H)
            m.load_state_dict({f"{n}_l0": sd[f"{n}_l{l}{sfx}"].to(m.weight_hh_l0.dtype) for n in NAMES})
            pair.append(m)
        layers.append(pair)
    return layers


def composed(layers, call, x, hx=None, lengths=None):
    """The bidirectional stack as a user composes it from unidirectional single-layer modules: the reverse direction of a
    layer is the plain module on R(input), its output reversed back; the next layer reads the concatenation.
    call(module, x, (h0[1,B,H], c0[1,B,H]) or None, lengths) -> (out[B,T,H], (h_n[1,B,H], c_n[1,B,H])).
    -> (output[B,T,2H], (h_n[2L,B,H], c_n[2L,B,H])), states indexed 2 * layer + direction."""
    inp, hs, cs = x, [], []
    for l, (fwd, bwd) in enumerate(layers):
        state = [None if hx is None else (hx[0][k:k + 1], hx[1][k:k + 1]) for k in (2 * l, 2 * l + 1)]
        out_f, (h_f, c_f) = call(fwd, inp, state[0], lengths)
        out_b, (h_b, c_b) = call(bwd, R(inp, lengths), state[1], lengths)
        inp = torch.cat([out_f, R(out_b, lengths)], dim=2)
        hs += [h_f, h_b]
        cs += [c_f, c_b]
    return inp, (torch.cat(hs, 0), torch.cat(cs, 0))


def call_packed(mod, x, hx, lengths):
    """`call` of composed() for torch.nn.LSTM modules (any direction count): the rows with n > 0 packed (torch packs no
    empty rows: they are left out, as tests/lengths_reference.py does), padded back to T; a row with n = 0 passes
    through: zero output, (h_n, c_n) = (h0, c0)."""
    B, T = x.shape[0], x.shape[1]
    D = 2 if mod.bidirectional else 1
    if hx is None:
        zeros = x.new_zeros(D * mod.num_layers, B, mod.hidden_size)
        hx = (zeros, zeros.clone())
    if lengths is None:
        return mod(x, hx)
    lengths = [int(n) for n in lengths]
    keep = [b for b, n in enumerate(lengths) if n > 0]
    out = x.new_zeros(B, T, D * mod.hidden_size)
    h_n, c_n = hx[0].clone(), hx[1].clone()
    if keep:
        packed = pack_padded_sequence(x[keep], torch.tensor([lengths[b] for b in keep]), batch_first=True, enforce_sorted=False)
        out_p, (h_k, c_k) = mod(packed, (hx[0][:, keep].contiguous(), hx[1][:, keep].contiguous()))
        out_k, _ = pad_packed_sequence(out_p, batch_first=True, total_length=T)
        out[keep] = out_k
        h_n[:, keep] = h_k
        c_n[:, keep] = c_k
    return out, (h_n, c_n)


def call_lengths(mod, x, hx, lengths):
    """`call` of composed() for cerebralsignalnetworks_amd.LSTM modules."""
    return mod(x, hx) if lengths is None else mod(x, hx, lengths=lengths)


def run(fn, named_params, x, h0, c0, dy, dh, dc):
    """fn(x, (h0, c0) or None) -> (out, (h_n, c_n)), then the backward of <out, dy> + <h_n, dh> + <c_n, dc>: the dict of
    outputs and gradients of tests/test_gpu_lstm_state.py::_run (h0 = c0 = None: no dh0 / dc0).  A gradient that nothing
    reached is zeros."""
    named_params = list(named_params)
    x = x.clone().requires_grad_(True)
    hx = None if h0 is None else (h0.clone().requires_grad_(True), c0.clone().requires_grad_(True))
    for _, p in named_params:
        p.grad = None
    out, (h_n, c_n) = fn(x, hx)
    torch.autograd.backward([out, h_n, c_n], [dy, dh, dc])
    res = dict(out=out.detach(), h_n=h_n.detach(), c_n=c_n.detach(), dx=x.grad if x.grad is not None else torch.zeros_like(x))
    if hx is not None:
        res.update(dh0=hx[0].grad, dc0=hx[1].grad)
    res.update({k: (p.grad if p.grad is not None else torch.zeros_like(p)).detach().clone() for k, p in named_params})
    return res


def composed_named_params(layers):
    """The parameters of single_layer_modules(...) under the bidirectional module's names."""
    return [(f"{n}_l{l}{sfx}", getattr(pair[d], f"{n}_l0")) for l, pair in enumerate(layers)
            for d, sfx in enumerate(("", "_reverse")) for n in NAMES]


def nn_bilstm_f64(ref, x, lengths, h0, c0, dy, dh, dc):
    """float64 torch.nn.LSTM(bidirectional=True) `ref` on the CPU, on the packed batch when lengths are given; tensors
    float64 CPU (h0 = c0 = None: zero state).  -> run()'s dict."""
    return run(lambda xx, hx: call_packed(ref, xx, hx, lengths), ref.named_parameters(), x, h0, c0, dy, dh, dc)
