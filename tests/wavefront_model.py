"""The six layer wavefronts of csrc/lstm.hip as the host functions wrote them out by hand before they shared
csn::wavefront_schedule (not a test module): forward_v1 / backward_v1 (path 0), forward_resident / backward_resident
(path 5), forward_il / backward_il (path 1 and the backward fall-back of paths 2 / 3), each transcribed loop for loop
-- the diagonal loop, the layer-range test, the flush of a full launch at np == 4, the second walk over the layers for
what follows the diagonal -- and NOT derived from lstm_schedule.h, which tests/test_wavefront_schedule_cpu.py holds to
this model.

run(variant, T, L, chunk) returns the launches in enqueue order, each a dict

    cells  [(layer, chunk, t, nsteps)]   the problems of the launch in problem order; backward: chunk is the reverse
                                         chunk and the cell covers the steps t, t - 1, ..., t - nsteps + 1
    waits  [(layer, chunk)]              il pair: the events waited for in front of the launch (xproj_ready / dx_ready of
                                         a cell that enters a chunk), in wait order
    follow [(layer, chunk, last)]        what the function walks behind the launch, in order: forward -- the input
                                         projection of layer + 1 for the chunk; backward_v1 / _resident -- the input
                                         gradient GEMM of the layer (layers above 0); backward_il -- every layer that
                                         ended a chunk, layer 0 included, last = its recurrence is complete

A launch with cells of a split diagonal (more than four layers in range) has no follow-ups unless it is the second one.
counts(variant, T, L, chunk) is what csn_lstm_profile_read reports for the pass: (launches, cells)."""

VARIANTS = ("forward_v1", "backward_v1", "forward_resident", "backward_resident", "forward_il", "backward_il")


def ends_chunk(T, chunk, t):
    return (t + 1) % chunk == 0 or t == T - 1


def chunk_at(T, chunk, c):
    t0 = c * chunk
    return t0, (chunk if t0 + chunk <= T else T - t0)


def forward_v1(T, NL, Cz):
    out = []
    lag = Cz
    D = T + lag * (NL - 1)
    for dg in range(D):
        cells = []
        for l in range(NL):
            t = dg - lag * l
            if t < 0 or t >= T:
                continue
            if len(cells) == 4:
                out.append({"cells": cells, "waits": [], "follow": []})
                cells = []
            cells.append((l, t // Cz, t, 1))
        follow = []
        for l in range(NL - 1):
            t = dg - lag * l
            if t < 0 or t >= T or not ends_chunk(T, Cz, t):
                continue
            follow.append((l, t // Cz, t == T - 1))
        if len(cells) > 0:
            out.append({"cells": cells, "waits": [], "follow": follow})
        else:
            assert not follow
    return out


def backward_v1(T, NL, Cz):
    out = []
    lag = Cz
    D = T + lag * (NL - 1)
    for dg in range(D):
        cells = []
        for l in range(NL - 1, -1, -1):
            r = dg - lag * (NL - 1 - l)
            if r < 0 or r >= T:
                continue
            t = T - 1 - r
            if len(cells) == 4:
                out.append({"cells": cells, "waits": [], "follow": []})
                cells = []
            cells.append((l, r // Cz, t, 1))
        follow = []
        for l in range(NL - 1, 0, -1):
            r = dg - lag * (NL - 1 - l)
            if r < 0 or r >= T or not ends_chunk(T, Cz, r):
                continue
            follow.append((l, r // Cz, r == T - 1))
        if len(cells) > 0:
            out.append({"cells": cells, "waits": [], "follow": follow})
        else:
            assert not follow
    return out


def forward_resident(T, NL, Cz):
    out = []
    nch = (T + Cz - 1) // Cz
    D = nch + NL - 1
    for dg in range(D):
        cells = []
        for l in range(NL):
            c = dg - l
            if c < 0 or c >= nch:
                continue
            t0, nsteps = chunk_at(T, Cz, c)
            if len(cells) == 4:
                out.append({"cells": cells, "waits": [], "follow": []})
                cells = []
            cells.append((l, c, t0, nsteps))
        follow = []
        for l in range(NL - 1):
            c = dg - l
            if c < 0 or c >= nch:
                continue
            follow.append((l, c, c == nch - 1))
        if len(cells) > 0:
            out.append({"cells": cells, "waits": [], "follow": follow})
        else:
            assert not follow
    return out


def backward_resident(T, NL, Cz):
    out = []
    nch = (T + Cz - 1) // Cz
    D = nch + NL - 1
    for dg in range(D):
        cells = []
        for l in range(NL - 1, -1, -1):
            c = dg - (NL - 1 - l)
            if c < 0 or c >= nch:
                continue
            t0, nsteps = chunk_at(T, Cz, c)
            if len(cells) == 4:
                out.append({"cells": cells, "waits": [], "follow": []})
                cells = []
            cells.append((l, c, T - 1 - t0, nsteps))
        follow = []
        for l in range(NL - 1, 0, -1):
            c = dg - (NL - 1 - l)
            if c < 0 or c >= nch:
                continue
            follow.append((l, c, c == nch - 1))
        if len(cells) > 0:
            out.append({"cells": cells, "waits": [], "follow": follow})
        else:
            assert not follow
    return out


def forward_il(T, NL, Cz):
    out = []
    lag = 2 * Cz
    D = T + lag * (NL - 1)
    for dg in range(D):
        cells, waits = [], []
        for l in range(NL):
            t = dg - lag * l
            if t < 0 or t >= T:
                continue
            if len(cells) == 4:
                out.append({"cells": cells, "waits": waits, "follow": []})
                cells, waits = [], []
            if l > 0 and t % Cz == 0:
                waits.append((l, t // Cz))
            cells.append((l, t // Cz, t, 1))
        if len(cells) == 0:
            continue
        follow = []
        for l in range(NL - 1):
            t = dg - lag * l
            if t < 0 or t >= T or not ends_chunk(T, Cz, t):
                continue
            follow.append((l, t // Cz, t == T - 1))
        out.append({"cells": cells, "waits": waits, "follow": follow})
    return out


def backward_il(T, NL, Cz):
    out = []
    lag = 2 * Cz
    D = T + lag * (NL - 1)
    for dg in range(D):
        cells, waits = [], []
        for l in range(NL - 1, -1, -1):
            r = dg - lag * (NL - 1 - l)
            if r < 0 or r >= T:
                continue
            t = T - 1 - r
            top = l == NL - 1
            if len(cells) == 4:
                out.append({"cells": cells, "waits": waits, "follow": []})
                cells, waits = [], []
            if not top and r % Cz == 0:
                waits.append((l + 1, r // Cz))
            cells.append((l, r // Cz, t, 1))
        if len(cells) == 0:
            continue
        follow = []
        for l in range(NL - 1, -1, -1):
            r = dg - lag * (NL - 1 - l)
            if r < 0 or r >= T or not ends_chunk(T, Cz, r):
                continue
            follow.append((l, r // Cz, r == T - 1))
        out.append({"cells": cells, "waits": waits, "follow": follow})
    return out


def run(variant, T, L, chunk):
    assert variant in VARIANTS, variant
    return globals()[variant](T, L, chunk)


def counts(variant, T, L, chunk):
    """(launches, cells) of csn_lstm_profile_read: the il pair counts what it launched, the resident pair reports T L
    cells, the v1 pair keeps no counts."""
    launches = run(variant, T, L, chunk)
    if variant.endswith("_v1"):
        return 0, 0
    if variant.endswith("_resident"):
        return len(launches), T * L
    return len(launches), sum(len(q["cells"]) for q in launches)
