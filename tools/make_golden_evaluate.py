#!/usr/bin/env python3
"""Generate tests/golden/evaluate.npz: what the REFERENCE's per-batch evaluation (run/sample.py:231-273) answers on seeded batches.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_evaluate.py

Imports the reference read-only (MUSE_REFERENCE) through tools/make_golden_decode.py, which registers the stand-ins for
`miditoolkit` the decode half needs, and runs the reference's own decode_batch, split_meta_midi, ONNC, Controllability_Pitch and
Controllability_Velocity.  The block run/sample.py:245-273 is not restated here: its source lines are read from the reference at run
time (from the `if metric_total is not None and valid_count:` line up to the `finally:` that closes it) and executed as they are,
with the names the block uses bound to this script's values.  Nothing of that text is written anywhere; the fixture holds arrays.

Four modification batches of 8 to 24 ComMU-shaped rows (tests/decode_ref.py's seeded generator): correct_ids = a clean row, the
sample = that row with notes moved, a few samples broken so that strict validation rejects them, one batch with every sample broken,
one batch whose first ground-truth row has chords only (its harmony vector is the reference's 0 / 0: the NaN behaviour of the run is
what is recorded).  Three generation batches of 8 rows around ONE meta + chord prefix, decoded without strict validation.

Condition on the modification batches (checked here, asserted by tests/test_evaluate_cpu.py): in float64, over the reference's own
vectors, every row without a NaN similarity has best > second best by a relative 1e-4; a draw that violates it is rejected and the
seed moves on."""
import contextlib
import io
import os
import sys
import textwrap
from collections import OrderedDict

import numpy as np
import torch

TOOLS = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, TOOLS)
import make_golden_decode as mgd  # noqa: E402  (registers the stand-ins, puts the reference and tests/ on the path)

from MuseDiffusion import metric as rmetric  # noqa: E402

rdec, dr, REF, REPO = mgd.rdec, mgd.dr, mgd.REF, mgd.REPO
L = 160
GAP = 1e-4
SIZES = (8, 24, 12, 16)
OK_OR_INVALID = (dr.OK, dr.NO_EOS, dr.RESTORE_FAILED, dr.ONCE_FAILED, dr.STRICT_FAILED)

written = []
mgd.MidiFile.dump = lambda self, path: written.append(os.path.basename(path))


def reference_block():
    """the source of run/sample.py's per-batch metric block, dedented, found by its first line and the `finally:` behind it"""
    with open(os.path.join(REF, "MuseDiffusion", "run", "sample.py")) as f:
        lines = f.read().splitlines()
    start = next(i for i, ln in enumerate(lines) if ln.strip() == "if metric_total is not None and valid_count:")
    stop = next(i for i in range(start, len(lines)) if lines[i].strip() == "finally:")
    return compile(textwrap.dedent("\n".join(lines[start:stop])), "run/sample.py:%d-%d" % (start + 1, stop), "exec")


def move_notes(g, row, mask):
    """the sample of a ground-truth row: some notes get another pitch, velocity, duration or position"""
    out = row.copy()
    first = int(len(row) - mask.sum())
    for j in range(first, len(row) - 3):
        if 432 <= row[j] <= 559 and 131 <= row[j + 1] <= 194 and g.random() < 0.5:
            out[j] = 432 + int(g.integers(0, 128)) if g.random() < 0.3 else row[j]
            out[j + 1] = int(g.integers(131, 195))
            out[j + 2] = int(np.clip(row[j + 2] + g.integers(-7, 8), 3, 130))
            out[j + 3] = int(g.integers(304, 432))
    return out


def break_row(g, row, mask, how):
    out = row.copy()
    first = int(len(row) - mask.sum())
    eos = first + int(np.argmax(row[first:] == 1))
    if how == "no_eos":
        out[eos] = 0
    elif how == "no_notes":                          # bars only: validate_once finds no note
        out[first:eos] = np.where(row[first:eos] == 2, 2, 0)
        keep = out[first:eos][out[first:eos] == 2]
        out[first:] = 0
        out[first:first + len(keep)] = keep
        out[first + len(keep)] = 1
    else:                                            # "bad_order": a pitch where a velocity belongs - only the strict validator minds
        vel = [j for j in range(first, eos) if 131 <= row[j] <= 194 and 432 <= row[j - 1] <= 559]
        j = vel[int(g.integers(2, len(vel) - 2))]
        out[j] = 60
    return out


def chords_only(row, mask):
    """a ground-truth row whose note part holds its bars and nothing else"""
    return break_row(None, row, mask, "no_notes")


def draw_batch(g, B, n_broken, all_broken, nan_row):
    correct, sample, masks = np.zeros((B, L), np.int64), np.zeros((B, L), np.int64), np.zeros((B, L), np.int64)
    broken = set(range(B)) if all_broken else set(g.choice(np.arange(1, B), size=n_broken, replace=False).tolist())
    for b in range(B):
        row, mask = dr.make_row(g, L, "clean" if g.random() < 0.6 else "extra_bar", n_bars=4, notes_per_bar=int(g.integers(4, 7)))
        row, mask = row.astype(np.int64), mask.astype(np.int64)
        s = move_notes(g, row, mask)
        if b in broken:
            s = break_row(g, s, mask, ("no_eos", "no_notes", "bad_order")[int(g.integers(0, 3))])
        if nan_row and b == 0:
            row = chords_only(row, mask)
        correct[b], sample[b], masks[b] = row, s, mask
    return correct, sample, masks


def acceptable(sample, masks):
    """the reference's decode_batch raises on the statuses outside OK_OR_INVALID: such a draw is not a fixture"""
    return all(dr.decode_row(sample[b], masks[b], 2 * L, L, L, strict=True)["status"] in OK_OR_INVALID for b in range(len(sample)))


def gap_ok(vec):
    v = vec.astype(np.float64)
    sim = (v[:, :32] @ v[:, :32].T) * (v[:, 32:44] @ v[:, 32:44].T) * (v[:, 44:] @ v[:, 44:].T)
    np.fill_diagonal(sim, 0.0)
    for i in range(len(sim)):
        if np.isnan(sim[i]).any():
            continue
        a = np.sort(sim[i])[::-1]
        if not a[0] > 0 or not (a[0] - a[1]) > GAP * a[0]:
            return False
    return True


def run_reference_batch(block, metric_total, batch_index, batch_size, correct, sample, masks):
    """run/sample.py:231-273 on one batch -> what it left behind (None for the metric outputs when the block did not run)"""
    del written[:]
    with contextlib.redirect_stdout(io.StringIO()):
        valid_count, invalid_idxes = rdec.decode_batch(mode="modification", sequences=sample.copy(), input_ids_mask_ori=masks.copy(),
                                                       output_dir="out", batch_index=batch_index, previous_count=batch_index * batch_size,
                                                       return_indices=True, strict_validation=True)
    names = list(written)
    ns = dict(metric_total=metric_total, valid_count=valid_count, invalid_idxes=invalid_idxes, correct_ids=torch.from_numpy(correct.copy()),
              sample_tokens=sample.copy(), input_ids_mask_ori=masks.copy(), np=np, split_meta_midi=rdec.split_meta_midi, ONNC=rmetric.ONNC,
              Controllability_Pitch=rmetric.Controllability_Pitch, Controllability_Velocity=rmetric.Controllability_Velocity, dev="cpu",
              batch_index=batch_index)
    with contextlib.redirect_stdout(io.StringIO()) as out:
        exec(block, ns)
    rec = dict(valid_count=valid_count, invalid=invalid_idxes, names=names, printed=out.getvalue())
    if valid_count:
        midis = ns["ground_truth_midis"] + ns["generated_midis"]
        onnc, vecs, most = rmetric.ONNC(midis, return_vectors=True, return_mostsim=True, device="cpu")
        assert float(onnc) == float(ns["onnc"])
        r, m, h = vecs[0]
        rec.update(onnc=np.float32(ns["onnc"]), most=most.numpy().astype(np.int32), vec=torch.cat([r, m, h], dim=1).numpy().astype(np.float32),
                   cp=(ns["total_p"], ns["wrong_p"]), cv=(ns["total_v"], ns["wrong_v"]))
    return rec


def generation_batches(g):
    """three batches of 8 rows around one meta + chord prefix (meta_to_batch's layout), decoded as run/sample.py does in generation mode"""
    meta, chord = dr.make_meta(g, 4, 1)
    pre = meta + chord
    mask = np.array([0] * (len(pre) + 1) + [1] * (L - len(pre) - 1), np.int64)
    tokens, counts, names, total = [], [], [], 0
    for t, n_bad in enumerate((6, 3, 1)):
        rows = np.zeros((8, L), np.int64)
        bad = set(g.choice(8, size=n_bad, replace=False).tolist())
        for b in range(8):
            notes = dr.make_notes(g, 4, int(g.integers(3, 6)))
            rows[b, :len(pre)] = pre
            rows[b, len(pre) + 1:len(pre) + 1 + len(notes)] = notes
            if b in bad:
                rows[b] = break_row(g, rows[b], mask, ("no_eos", "no_notes")[b % 2])
        assert all(dr.decode_row(rows[b], mask, 2 * L, L, L)["status"] in OK_OR_INVALID for b in range(8))
        del written[:]
        with contextlib.redirect_stdout(io.StringIO()):
            vc = rdec.decode_batch(mode="generation", sequences=rows.copy(), input_ids_mask_ori=np.tile(mask, (8, 1)), output_dir="out",
                                   batch_index=t, previous_count=total, strict_validation=False)
        assert vc == 8 - n_bad
        total += vc
        tokens.append(rows)
        counts.append(vc)
        names += list(written)
    return np.array(pre, np.int32), np.concatenate(tokens).astype(np.int32), np.array(counts, np.int32), names


def main():
    block = reference_block()
    plans = [dict(n_broken=2, all_broken=False, nan_row=False), dict(n_broken=5, all_broken=False, nan_row=False),
             dict(n_broken=0, all_broken=True, nan_row=False), dict(n_broken=3, all_broken=False, nan_row=True)]
    metric_total = OrderedDict((k, torch.tensor(0.0 if k == "onnc_sum" else 0)) for k in
                               ("onnc_sum", "onnc_count", "total_total_p", "total_total_v", "total_wrong_p", "total_wrong_v"))
    out = {k: [] for k in ("correct", "sample", "mask", "valid_count", "onnc", "cp", "cv", "totals", "invalid", "most", "vec", "names",
                           "names_n", "printed", "seed")}
    batch_size = max(SIZES)                          # the loader's batch size: the last batches of a split are smaller
    for batch_index, (B, plan) in enumerate(zip(SIZES, plans)):
        seed = 1000 * (batch_index + 1)
        while True:
            g = np.random.default_rng(seed)
            correct, sample, masks = draw_batch(g, B, **plan)
            if acceptable(sample, masks):
                trial = OrderedDict((k, v.clone()) for k, v in metric_total.items())
                rec = run_reference_batch(block, trial, batch_index, batch_size, correct, sample, masks)
                if not rec["valid_count"] or gap_ok(rec["vec"]):
                    break
            seed += 1
        metric_total = trial
        invalid = np.zeros(B, bool)
        invalid[rec["invalid"]] = True
        assert rec["valid_count"] == B - invalid.sum() and (rec["valid_count"] == 0) == plan["all_broken"]
        if plan["nan_row"]:
            assert np.isnan(rec["vec"][0]).any() and not invalid[0]
        for k, v in (("correct", correct), ("sample", sample), ("mask", masks)):
            out[k].append(v.astype(np.int32))
        out["valid_count"].append(rec["valid_count"])
        out["onnc"].append(rec.get("onnc", np.float32("nan")))
        out["cp"].append(rec.get("cp", (0, 0)))
        out["cv"].append(rec.get("cv", (0, 0)))
        out["totals"].append([float(v) for v in metric_total.values()])
        out["invalid"].append(invalid)
        out["most"].append(rec.get("most", np.zeros(0, np.int32)))
        out["vec"].append(rec.get("vec", np.zeros((0, 56), np.float32)))
        out["names"] += rec["names"]
        out["names_n"].append(len(rec["names"]))
        out["printed"].append(rec["printed"])
        out["seed"].append(seed)
        print("batch %d: B=%d seed=%d valid=%d onnc=%s cp=%s cv=%s totals=%s" % (batch_index, B, seed, rec["valid_count"], rec.get("onnc"),
                                                                               rec.get("cp"), rec.get("cv"), out["totals"][-1]))
    total_onnc = float(metric_total["onnc_sum"] / metric_total["onnc_count"])
    total_cp = float(metric_total["total_wrong_p"] / metric_total["total_total_p"])
    total_cv = float(metric_total["total_wrong_v"] / metric_total["total_total_v"])
    gen_prefix, gen_tokens, gen_counts, gen_names = generation_batches(np.random.default_rng(77))
    cat = lambda k, dt: np.concatenate(out[k]).astype(dt)
    off = lambda k: np.concatenate([[0], np.cumsum([len(a) for a in out[k]])]).astype(np.int64)
    fix = dict(correct=cat("correct", np.int32), sample=cat("sample", np.int32), mask=cat("mask", np.int32), batch_off=off("correct"),
               batch_size=np.int32(batch_size), valid_count=np.array(out["valid_count"], np.int32), onnc=np.array(out["onnc"], np.float32),
               cp=np.array(out["cp"], np.int64), cv=np.array(out["cv"], np.int64), totals=np.array(out["totals"], np.float64),
               onnc_sum=np.array([t[0] for t in out["totals"]], np.float32), invalid=cat("invalid", bool), most=cat("most", np.int32),
               most_off=off("most"), vec=cat("vec", np.float32), names=np.array(out["names"], dtype="U40"),
               names_off=np.concatenate([[0], np.cumsum(out["names_n"])]).astype(np.int64), printed=np.array(out["printed"], dtype="U400"),
               summary=np.array([total_onnc, total_cp, total_cv], np.float64), seed=np.array(out["seed"], np.int32),
               gen_prefix=gen_prefix, gen_tokens=gen_tokens, gen_counts=gen_counts, gen_names=np.array(gen_names, dtype="U40"))
    path = os.path.join(REPO, "tests", "golden", "evaluate.npz")
    np.savez_compressed(path, **fix)
    print("summary onnc=%.6f cp=%.6f cv=%.6f; generation counts %s" % (total_onnc, total_cp, total_cv, gen_counts.tolist()))
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
