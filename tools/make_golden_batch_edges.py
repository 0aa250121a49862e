#!/usr/bin/env python3
"""Generate tests/golden/batch_edges.npz: what the REFERENCE returns - or raises - on the short edge rows of tests/batch_cases.py.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_batch_edges.py

Same harness as tools/make_golden_batch.py (imported: its module stand-ins, its reference imports and its draw Recorder).  The
difference is where the draws come from: the case list fixes them (a draw exactly on float32(p), a token that fires at a given rank),
so the Recorder wraps a Replay that hands the case's draws out in the order the reference asks for them, and the fixture stores what
the Recorder logged - laid out as the device wrappers document their `u` / `new_tokens` / `pairs` arguments - next to the outputs.
Where the reference raises, the exception class is stored as a small integer (batch_cases.EXC) and the output is empty / NaN.

Data only; every family is stored row by row (ragged: `<family>_values` + `<family>_offsets`, outputs with offsets of their own, since a
flagged rotation changes the reference's row length).  Long rows are not stored: tests regenerate them from the case list's seeds.
"""
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_batch as mgb  # noqa: E402  (registers the stand-ins, imports the reference)

sys.path.insert(0, os.path.join(mgb.REPO, "tests"))
import batch_cases as bc  # noqa: E402

rcorr, rdec, rmetric, collate_batches = mgb.rcorr, mgb.rdec, mgb.rmetric, mgb.collate_batches


class Replay:
    """stands where the Recorder keeps its random.Random: the case's draws, in the order asked for"""

    def __init__(self, u=None, new=None, pairs=None):
        self.u, self.new, self.pairs, self.k, self.j, self.s = u, new, pairs, -1, 0, 0

    def random(self):
        self.k += 1
        return float(self.u[self.k])

    def randint(self, a, b):
        v = int(self.new[self.k][self.j % 3])
        self.j += 1
        assert a <= v <= b
        return v

    def sample(self, pop, k):
        first, second = (int(v) for v in self.pairs[self.s])
        self.s += 1
        assert k == 2 and first in pop and second in pop and first != second
        return [second, first]          # unsorted on purpose: the reference sorts


def recorder(**kw):
    rec = mgb.Recorder(0)
    rec.r = Replay(**kw)
    rcorr.generator = rec
    return rec


def attempt(fn):
    """(result or None, exception class as an integer)"""
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return fn(), 0
    except Exception as e:  # noqa: BLE001 - the class is the datum
        return None, bc.exc_code(e)


def cat(parts, dtype, width=None):
    parts = [np.asarray(p, dtype).reshape((-1,) if width is None else (-1, width)) for p in parts]
    off = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    return (np.concatenate(parts) if parts else np.zeros(0, dtype)), off


def names(rows):
    return np.array(["%s/%s" % (b["name"], r["name"]) for b, r in rows])


def corruption(out, fam):
    rows = bc.stored_rows(fam)
    res, exc, logged_u, logged_new, used = [], [], [], [], []
    for b, r in rows:
        seq, p = torch.tensor(r["seq"], dtype=torch.long), float(np.float32(b.get("p", 0)))
        if fam == "rr":
            rec = recorder(pairs=r["pairs"])
            got, e = attempt(lambda: rcorr.random_rotating(seq, count=b["count"]))
            assert e or [sorted(v) for _, v in rec.log] == r["pairs"].tolist()
        else:
            rec = recorder(u=r["u"], new=r.get("new"))
            fn = {"mt": rcorr.masking_token, "mn": rcorr.masking_note, "rn": rcorr.randomize_note}[fam]
            got, e = attempt(lambda: fn(seq, p=p))
            us = [v for k, v in rec.log if k == "u"]
            n = len(r["seq"])
            u, new, k = np.array(us + [bc.NEVER] * (n - len(us)), np.float32), np.zeros((n, 3), np.int32), -1
            ints = []
            for kind, v in rec.log:          # the three integers that follow a firing draw belong to its rank
                if kind == "u":
                    if ints:
                        new[k] = ints
                    k, ints = k + 1, []
                else:
                    ints.append(v)
            if ints:
                new[k] = ints
            logged_u.append(u)
            logged_new.append(new)
            used.append(len(us))
        res.append(np.zeros(0, np.int32) if got is None else got.numpy().astype(np.int32))
        exc.append(e)
    out[fam + "_names"] = names(rows)
    out[fam + "_values"], out[fam + "_offsets"] = cat([r["seq"] for _, r in rows], np.int32)
    out[fam + "_out"], out[fam + "_out_offsets"] = cat(res, np.int32)
    out[fam + "_exc"] = np.array(exc, np.int32)
    if fam == "rr":
        out["rr_pairs"], out["rr_pairs_offsets"] = cat([r["pairs"] for _, r in rows], np.int32, 2)
        out["rr_count"] = np.array([b["count"] for b, _ in rows], np.int32)
    else:
        out[fam + "_p"] = np.array([b["p"] for b, _ in rows], np.float32)
        out[fam + "_u"] = np.concatenate(logged_u)                  # u[offsets[b] + k]: draw k of row b; NEVER past the last one made
        out[fam + "_draws"] = np.array(used, np.int32)
        if fam == "rn":
            out["rn_new"] = np.concatenate(logged_new)              # new[offsets[b] + k] = (velocity, pitch, duration) of draw k; 0 if unused


def main():
    out = {}
    for fam in ("mt", "mn", "rn", "rr"):
        corruption(out, fam)

    # ---- collate_batches, one row at a time (data/wrapper.py:90-127): a row longer than seq_len raises
    rows = bc.stored_rows("r2p")
    res, exc, length = [], [], []
    for b, r in rows:
        ids = torch.tensor(r["seq"], dtype=torch.long)
        sample = {"input_ids": ids, "input_mask": ids.clone(), "length": len(ids)}
        got, e = attempt(lambda: collate_batches([sample], seq_len=b["L"]))
        key = "input_mask" if b["pad"] == 1 else "input_ids"        # the mask is the field padded with ones
        res.append(np.zeros(0, np.int32) if got is None else got[key][0].numpy().astype(np.int32))
        length.append(-1 if got is None else int(got["length"][0]))
        exc.append(e)
    out["r2p_names"] = names(rows)
    out["r2p_values"], out["r2p_offsets"] = cat([r["seq"] for _, r in rows], np.int32)
    out["r2p_L"], out["r2p_pad"] = np.array([b["L"] for b, _ in rows], np.int32), np.array([b["pad"] for b, _ in rows], np.int32)
    out["r2p_out"], out["r2p_out_offsets"] = cat(res, np.int32)
    out["r2p_length"], out["r2p_exc"] = np.array(length, np.int32), np.array(exc, np.int32)

    # ---- meta_to_batch's layout (utils/decode_util.py:221-230) on already encoded tokens, as tools/make_golden_batch.py states it
    rows = bc.stored_rows("m2b")
    ids_all, msk_all = [], []
    for b, _ in rows:
        enc = torch.tensor(b["meta"], dtype=torch.int)
        ids = torch.zeros(b["B"], b["L"], dtype=torch.int)
        ids[:, :len(enc)] = enc
        msk = torch.ones(b["B"], b["L"], dtype=torch.int)
        msk[:, :len(enc) + 1] = 0
        ids_all.append(ids.numpy().ravel())
        msk_all.append(msk.numpy().ravel())
    out["m2b_names"] = names(rows)
    out["m2b_meta"], out["m2b_meta_offsets"] = cat([b["meta"] for b, _ in rows], np.int32)
    out["m2b_B"], out["m2b_L"] = np.array([b["B"] for b, _ in rows], np.int32), np.array([b["L"] for b, _ in rows], np.int32)
    out["m2b_ids"], out["m2b_out_offsets"] = cat(ids_all, np.int32)
    out["m2b_mask"], _ = cat(msk_all, np.int32)

    # ---- remove_padding -> validate_once / validate_rigidly (utils/decode_util.py:73-84, :142-183)
    S = rdec.SequenceToMidi
    rows = bc.stored_rows("val")
    res = np.zeros((len(rows), 3), np.int32)
    for i, (b, r) in enumerate(rows):
        c = r["seq"][:r["len"]].astype(np.int64)
        cut, e = attempt(lambda: S.remove_padding(c))
        assert e in (0, bc.EXC["SequenceToMidiError"])
        res[i, 0] = -1 if cut is None else len(cut) - 1
        if cut is not None:
            for j, f in ((1, S.validate_once), (2, S.validate_rigidly)):
                _, e = attempt(lambda: f(cut))
                assert e in (0, bc.EXC["SequenceToMidiError"], bc.EXC["IndexError"])
                res[i, j] = {0: 1, bc.EXC["SequenceToMidiError"]: 0, bc.EXC["IndexError"]: -2}[e]
    out["val_names"] = names(rows)
    out["val_tokens"], out["val_offsets"] = cat([r["seq"] for _, r in rows], np.int32)
    out["val_len"], out["val_result"] = np.array([r["len"] for _, r in rows], np.int32), res

    # ---- get_vectors (metric.py:4-71)
    rows = bc.stored_rows("msim")
    vec, exc = np.full((len(rows), 56), np.nan, np.float32), []
    for i, (b, r) in enumerate(rows):
        midi = r["seq"][:r["len"]].astype(np.int64)
        got, e = attempt(lambda: torch.cat(rmetric.get_vectors(midi, note_len=b["note_len"])).numpy())
        if got is not None:
            vec[i] = got
        exc.append(e)
    out["msim_names"] = names(rows)
    out["msim_tokens"], out["msim_offsets"] = cat([r["seq"] for _, r in rows], np.int32)
    out["msim_len"] = np.array([r["len"] for _, r in rows], np.int32)
    out["msim_note_len"] = np.array([b["note_len"] for b, _ in rows], np.float32)
    out["msim_vectors"], out["msim_exc"] = vec, np.array(exc, np.int32)

    # ---- Controllability_Pitch / _Velocity (metric.py:120-168), one (meta, row) pair at a time
    rows = bc.stored_rows("ctrl")
    pitch, velo = np.full((len(rows), 2), -1, np.int32), np.full((len(rows), 2), -1, np.int32)
    exc = []
    for i, (b, r) in enumerate(rows):
        meta, midi = [int(v) for v in r["meta"][:11]], r["seq"][:r["len"]].astype(np.int64)
        gp, ep = attempt(lambda: rmetric.Controllability_Pitch([meta], [midi]))
        gv, ev = attempt(lambda: rmetric.Controllability_Velocity([meta], [midi]))
        if gp is not None:
            pitch[i] = gp
        if gv is not None:
            velo[i] = gv
        exc.append(ep or ev)
    out["ctrl_names"] = names(rows)
    out["ctrl_tokens"], out["ctrl_offsets"] = cat([r["seq"] for _, r in rows], np.int32)
    out["ctrl_len"] = np.array([r["len"] for _, r in rows], np.int32)
    out["ctrl_metas"] = np.stack([r["meta"][:11] for _, r in rows]).astype(np.int32)
    out["ctrl_pitch"], out["ctrl_velocity"], out["ctrl_exc"] = pitch, velo, np.array(exc, np.int32)

    path = os.path.join(mgb.REPO, "tests", "golden", "batch_edges.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
