"""Plain-Python restatement of the two infill rules (include/musehip_infill.h, csrc/infill.hip), the model the device kernels are
compared with bit for bit.  Everything is written with explicit indices and Python lists, one token at a time, the way the rule is
worded and NOT the way the kernel computes it (no scans, no closed forms): the row is rebuilt by appending."""
import numpy as np

OK, NO_EOS, BAD_MASK, BAD_RANGE, OVERFLOW = range(5)
EOS, BAR = 1, 2
ALL = 15


def token_class(t):
    """position 0, velocity 1, pitch 2, duration 3, everything else -1"""
    t = int(t)
    if 432 <= t <= 559:
        return 0
    if 131 <= t <= 194:
        return 1
    if 3 <= t <= 130:
        return 2
    if 304 <= t <= 431:
        return 3
    return -1


def layout(tokens, prefix_mask):
    """-> (status, m, e, bars): bars = the indices in [m, e) holding BAR"""
    L = len(tokens)
    m = 0
    while m < L and prefix_mask[m] == 0:
        m += 1
    for j in range(m, L):
        if prefix_mask[j] != 1:
            return BAD_MASK, m, None, None
    if not 0 < m < L:
        return BAD_MASK, m, None, None
    e = None
    for j in range(m, L):
        if tokens[j] == EOS:
            e = j
            break
    if e is None:
        return NO_EOS, m, None, None
    return OK, m, e, [j for j in range(m, e) if tokens[j] == BAR]


def plan_row(tokens, prefix_mask, lo, hi, room=0, fields=ALL):
    """-> (out_tokens [L], out_mask [L], status, info (4))"""
    tokens = [int(t) for t in tokens]
    prefix_mask = [int(t) for t in prefix_mask]
    L = len(tokens)
    assert room >= 0 and 1 <= fields <= 15 and (fields == ALL or room == 0)
    bad = lambda st: (list(tokens), [0] * L, st, (0, 0, 0, 0))  # noqa: E731
    st, m, e, bars = layout(tokens, prefix_mask)
    if st != OK:
        return bad(st)
    nb = len(bars)
    if not 0 <= lo < hi <= nb:
        return bad(BAD_RANGE)
    edge = bars + [e]                                      # p_0 .. p_nb
    interior = [-1] * L                                    # the bar whose interior j lies in
    for k in range(nb):
        for j in range(edge[k] + 1, edge[k + 1]):
            interior[j] = k
    if fields == ALL:
        g = 4 * room
        added = g * (hi - lo)
        if e + 1 + added > L:
            return bad(OVERFLOW)
        out, mask = [], []
        closes = {edge[k + 1]: k for k in range(nb)}        # index of the BAR / EOS behind bar k's interior -> k
        for j in range(L):
            if lo <= closes.get(j, -1) < hi:                # the interior of a selected bar ends here: its room goes in front
                out += [0] * g
                mask += [1] * g
            out.append(tokens[j])
            mask.append(1 if lo <= interior[j] < hi else 0)
        region_end = edge[hi] + added
        return out[:L], mask[:L], OK, (edge[lo] + 1, region_end, sum(mask[:L]), added)
    mask = [0] * L
    for j in range(L):
        c = token_class(tokens[j])
        if not lo <= interior[j] < hi or c < 0 or not (fields >> c) & 1:
            continue
        q = j - c
        if q < 0 or q + 3 >= L:
            continue
        if all(interior[q + i] == interior[j] and token_class(tokens[q + i]) == i for i in range(4)):
            mask[j] = 1
    return list(tokens), mask, OK, (edge[lo] + 1, edge[hi], sum(mask), 0)


def splice_row(sampled, plan_tokens, plan_mask, status, fields=ALL):
    """-> (out [L], counts (kept, pads, other, changed))"""
    L = len(plan_tokens)
    plan_tokens = [int(t) for t in plan_tokens]
    if status != OK:
        return list(plan_tokens), (0, 0, 0, 0)
    kept = pads = other = changed = 0
    if fields != ALL:
        out = []
        for j in range(L):
            v = plan_tokens[j]
            if plan_mask[j] != 0:
                s = int(sampled[j])
                if token_class(s) == token_class(v):
                    kept += 1
                    changed += s != v
                    v = s
                else:
                    other += 1
            out.append(v)
        return out, (kept, pads, other, changed)
    first = []                                             # (token, region) after stage (a)
    for j in range(L):
        if plan_mask[j] == 0:
            first.append((plan_tokens[j], False))
            continue
        s = int(sampled[j])
        if s == 0:
            pads += 1
        elif token_class(s) < 0:
            other += 1
        else:
            first.append((s, True))
    out = []
    for i, (v, region) in enumerate(first):
        if region:
            q = i - token_class(v)
            whole = q >= 0 and q + 3 < len(first) and all(first[q + t][1] and token_class(first[q + t][0]) == t for t in range(4))
            if not whole:
                other += 1
                continue
            kept += 1
        out.append(v)
    return out + [0] * (L - len(out)), (kept, pads, other, changed)


def plan_rows(tokens, prefix_mask, lo, hi, room=0, fields=ALL):
    """[B, L] arrays, lo / hi [B] -> dict of int32 arrays as mhi_infill_plan fills them"""
    rows = [plan_row(tokens[b], prefix_mask[b], int(lo[b]), int(hi[b]), room, fields) for b in range(len(tokens))]
    return dict(tokens=np.array([r[0] for r in rows], np.int32), mask=np.array([r[1] for r in rows], np.int32),
                status=np.array([r[2] for r in rows], np.int32), info=np.array([r[3] for r in rows], np.int32).reshape(-1, 4))


def splice_rows(sampled, plan_tokens, plan_mask, status, fields=ALL):
    rows = [splice_row(sampled[b], plan_tokens[b], plan_mask[b], int(status[b]), fields) for b in range(len(plan_tokens))]
    return np.array([r[0] for r in rows], np.int32), np.array([r[1] for r in rows], np.int32).reshape(-1, 4)
