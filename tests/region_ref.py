"""Plain-Python / numpy restatement of the region-constrained rounding (include/musehip_region.h, csrc/region.hip), the model the
kernel is compared with bit for bit, plus the brute-force enumeration it is itself checked against (tests/test_region_cpu.py).

Everything steps one position at a time in np.float32, in the order the header defines; nothing here knows how the kernel finds its
segments (no scans, no tables): a segment is found by walking the mask."""
import numpy as np

from infill_ref import token_class

# mirror of enum mhg_class and enum mhr_status
PAD, EOS, BAR, PITCH, VELOCITY, DURATION, POSITION, ANY = range(8)
OK, NOT_PLANNED, BAD_PLAN, NONFINITE, NO_ROOM = range(5)
STATUS_NAMES = ("OK", "NOT_PLANNED", "BAD_PLAN", "NONFINITE", "NO_ROOM")
ALL = 15
USED = (PAD, PITCH, VELOCITY, DURATION, POSITION)          # the slots a region reads
FIELD_SLOT = {0: POSITION, 1: VELOCITY, 2: PITCH, 3: DURATION}   # infill class -> mhg_class
QUAD = (POSITION, VELOCITY, PITCH, DURATION)

f32 = np.float32


def segments(masked):
    """the maximal runs of True -> [(start, length)] in ascending order"""
    out, j, L = [], 0, len(masked)
    while j < L:
        if masked[j]:
            k = j
            while k < L and masked[k]:
                k += 1
            out.append((j, k - j))
            j = k
        else:
            j += 1
    return out


def viterbi_segment(cs, ci):
    """cs / ci [n, 8]: the tables of one segment -> (classes [n] or None, final score fp32, notes, pads)"""
    n = len(cs)
    rS, rV, rP, rD = True, False, False, False
    sS = sV = sP = sD = f32(0)
    dec = [False] * n
    for t in range(n):
        ok = [int(ci[t][c]) >= 0 for c in range(8)]
        s = [f32(cs[t][c]) for c in range(8)]
        with np.errstate(invalid="ignore", over="ignore"):   # a score of an unreachable state is never looked at
            # into S: DURATION before PAD
            b1, f1 = rD and ok[DURATION], f32(sD + s[DURATION])
            b2, f2 = rS and ok[PAD], f32(sS + s[PAD])
            d = b2 and (not b1 or bool(f2 > f1))
            nV, nP, nD = f32(sS + s[POSITION]), f32(sV + s[VELOCITY]), f32(sP + s[PITCH])
        nrV, nrP, nrD = rS and ok[POSITION], rV and ok[VELOCITY], rP and ok[PITCH]
        dec[t] = d
        rS, sS = b1 or b2, (f2 if d else f1)
        rV, sV, rP, sP, rD, sD = nrV, nV, nrP, nP, nrD, nD
    if not rS:
        return None, f32(0), 0, 0
    classes, state, notes, pads = [0] * n, "S", 0, 0
    for t in range(n - 1, -1, -1):
        if state == "S":
            if dec[t]:
                c, pads = PAD, pads + 1
            else:
                c, state, notes = DURATION, "D", notes + 1
        elif state == "D":
            c, state = PITCH, "P"
        elif state == "P":
            c, state = VELOCITY, "V"
        else:
            c, state = POSITION, "S"
        classes[t] = c
    assert state == "S"
    return classes, sS, notes, pads


def constrain_row(cs, ci, plan_tokens, plan_mask, plan_status, fields=ALL):
    """cs / ci [L, 8] -> dict(tokens [L] int32, status, path_score fp32, counts (4,))"""
    assert 1 <= fields <= 15
    L = len(plan_tokens)
    cs, ci = np.asarray(cs, f32), np.asarray(ci, np.int32)
    out = dict(tokens=ci[:, ANY].copy(), status=OK, path_score=f32(0), counts=(0, 0, 0, 0))

    def left(st):
        out["status"] = st
        return out

    if int(plan_status) != 0:
        return left(NOT_PLANNED)
    masked = [int(plan_mask[j]) == 1 for j in range(L)]
    where = [j for j in range(L) if masked[j]]
    if fields != ALL and any(token_class(plan_tokens[j]) < 0 for j in where):
        return left(BAD_PLAN)
    for j in where:
        for c in USED:
            if not cs[j, c] < np.inf:                      # NaN or +inf
                return left(NONFINITE)
    segs = segments(masked)
    total, notes, pads = f32(0), 0, 0
    tokens = out["tokens"].copy()                          # a row that turns out to have no room leaves as the plain argmax
    if fields == ALL:
        for start, n in segs:
            classes, score, k, p = viterbi_segment(cs[start:start + n], ci[start:start + n])
            if classes is None:
                return left(NO_ROOM)
            total = f32(total + score)
            notes, pads = notes + k, pads + p
            for t, c in enumerate(classes):
                tokens[start + t] = ci[start + t, c]
    else:
        slots = [FIELD_SLOT[token_class(plan_tokens[j])] for j in where]
        if any(ci[j, c] < 0 for j, c in zip(where, slots)):
            return left(NO_ROOM)
        for j, c in zip(where, slots):
            total = f32(total + cs[j, c])
            tokens[j] = ci[j, c]
    out["tokens"] = tokens
    out["path_score"], out["counts"] = total, (len(where), notes, pads, len(segs))
    return out


def constrain_rows(cs, ci, plan_tokens, plan_mask, plan_status, fields=ALL):
    """cs / ci [B, L, 8], plan_tokens / plan_mask [B, L], plan_status [B] -> dict of arrays as mhr_constrain_regions fills them"""
    B = len(plan_tokens)
    rows = [constrain_row(cs[b], ci[b], plan_tokens[b], plan_mask[b], plan_status[b], fields) for b in range(B)]
    return dict(tokens=np.stack([r["tokens"] for r in rows]).astype(np.int32), status=np.array([r["status"] for r in rows], np.int32),
                path_score=np.array([r["path_score"] for r in rows], f32),
                counts=np.array([r["counts"] for r in rows], np.int32).reshape(B, 4))


# ------------------------------------------------------------------------------------------------------------------ brute force
def accepted_strings(n):
    """every class string of length n in ( PAD | POSITION VELOCITY PITCH DURATION )*; their number follows f(n) = f(n-1) + f(n-4)"""
    if n == 0:
        return [[]]
    out = [[PAD] + s for s in accepted_strings(n - 1)]
    if n >= 4:
        out += [list(QUAD) + s for s in accepted_strings(n - 4)]
    return out


def brute_force(cs, ci):
    """-> (best strings as tuples, best float64 score) over every accepted string all of whose slots have a token; ([], None) if none"""
    n = len(cs)
    best, which = None, []
    for s in accepted_strings(n):
        if any(int(ci[t][c]) < 0 for t, c in enumerate(s)):
            continue
        total = float(sum(float(cs[t][c]) for t, c in enumerate(s)))
        if best is None or total > best:
            best, which = total, [tuple(s)]
        elif total == best:
            which.append(tuple(s))
    return which, best
