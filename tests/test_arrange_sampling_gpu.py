"""GPU: from single tracks to songs above the kernel.  sampling.arrange against sampling.generate on the concatenated batch with the
same noise, bit for bit (the tiny random model of tests/test_infill_sampling_gpu.py); sampling.run_arrangement with a stub sampler
that replays rows made by encode_batch from known note lists - one row without its first BAR (a pickup: the other tracks of its song
wait one bar), one row broken on purpose - the files and their numbering, keep_partial, read_song against the decode restatement's
notes plus the shifts, the report against a restatement that never touches the device (tests/decode_ref.py decodes,
tests/interplay_ref.py aligns, counts and sums); with interplay one more launch per batch and one more copy per run, without it
neither; run_generation launches what it launched; one pass with the real sampler."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import decode_ref as dr  # noqa: E402
import interplay_ref as ir  # noqa: E402
from musediffusion_amd import evaluation, metric, sampling  # noqa: E402
from musediffusion_amd.utils import arrange_util as au, decode_util as du  # noqa: E402
from musediffusion_amd.utils.encode_util import MetaToSequence, encode_batch  # noqa: E402
from test_evaluate_cpu import fixture  # noqa: E402
from test_evaluate_gpu import _fatal, dev, library_launches  # noqa: E402
from test_harmony_sampling_gpu import CopyCounter  # noqa: E402
from test_infill_sampling_gpu import STEP, fixed_draws, setup  # noqa: E402,F401

DEV = "cuda"
L = 160
# one chord a bar: MetaToSequence writes a change inside a bar without its chord token, the encoder writes it with one
BASE = dict(bpm=100, audio_key="aminor", time_signature="4/4", pitch_range="mid", num_measures=4, inst="acoustic_piano", genre="newage",
            min_velocity=40, max_velocity=100, track_role="main_melody", rhythm="standard",
            chord_progression="-".join(["Am"] * 8 + ["G"] * 8 + ["F"] * 8 + ["E"] * 8))
TRACKS = [dict(), dict(inst="acoustic_bass", track_role="bass", pitch_range="low"), dict(inst="string_ensemble", track_role="pad"),
          dict(inst="drums_full", track_role="riff")]
T, N_SONGS = len(TRACKS), 2
LOWEST = (60, 36, 48, 36)
NO_BAR, BROKEN = 1, T + 2                                              # rows of the first batch: song 0's bass, song 1's pad


def notes_of(g, lowest):
    """four bars of four notes on the sixteenth-note grid, one voice: a note ends where the next one starts at the latest, so that a
    file's note-offs cannot be taken for another note's"""
    starts = [bar * 1920 + int(s) * 120 for bar in range(4) for s in sorted(g.choice(16, size=4, replace=False))]
    out = []
    for k, start in enumerate(starts):
        room = (starts[k + 1] if k + 1 < len(starts) else 4 * 1920) - start
        out.append([start, start + min(int(g.integers(1, 5)) * 120, room), lowest + int(g.integers(0, 12)), 2 * int(g.integers(20, 50))])
    return np.array(out, np.int32)


def replay_batches():
    """two batches of N_SONGS songs x T tracks as host token rows [B, L], made by encode_batch from note lists; in the first batch row
    NO_BAR loses the BAR in front of its first note and row BROKEN its EOS"""
    g = np.random.default_rng(7)
    items = [(notes_of(g, LOWEST[t]), {**BASE, **TRACKS[t]}) for _ in range(2 * N_SONGS) for t in range(T)]
    cond, report = encode_batch(items, L)
    assert report["kept"].tolist() == list(range(len(items)))
    ids, mask = cond["input_ids"].cpu().numpy(), cond["input_mask"].cpu().numpy()
    prefix = len(MetaToSequence().execute(BASE))
    assert (mask[:, :prefix + 1] == 0).all() and (mask[:, prefix + 1:] == 1).all() and (ids[:, prefix + 1] == dr.BAR).all()
    row = ids[NO_BAR].tolist()
    del row[prefix + 1]
    ids[NO_BAR] = row + [0]
    last = int(np.nonzero(ids[BROKEN] == dr.EOS)[0][-1])
    assert last > prefix
    ids[BROKEN, last] = 0
    B = N_SONGS * T
    return [ids[:B].copy(), ids[B:].copy()], mask[:B].copy()


def restate(batch_list, mask):
    """what run_arrangement reports and writes, without the device: per batch the decoded rows (status, notes, chords, meta), the
    shifts, and the interplay totals over all batches"""
    totals, batches = ir.Totals(), []
    song = [b // T for b in range(N_SONGS * T)]
    for tokens in batch_list:
        ld = min(2 * L, dr.MAX_ROW)
        rows = [dr.decode_row(tokens[b], mask[b], ld, ld // 4 + 1, ld // 2 + 1, False) for b in range(len(tokens))]
        ok = [r["status"] == dr.OK for r in rows]
        first = [ir.first_bar_shift(r["restored"], len(r["restored"])) for r in rows]
        meta = [r["meta"] for r in rows]
        shift = ir.align_shift(first, ok, song, meta)
        cap = ld // 4 + 1
        notes, counts3 = np.zeros((len(rows), cap, 4), np.int32), np.zeros((len(rows), 3), np.int32)
        for b, r in enumerate(rows):
            if ok[b]:
                notes[b, :len(r["notes"])], counts3[b, 0] = r["notes"], len(r["notes"])
        valid = [ok[b] and int(meta[b][5]) != ir.DRUMS for b in range(len(rows))]
        out = ir.batch_counts(notes, counts3, np.array(meta, np.int32), valid, song, shift)
        totals.update(out, meta, songs=len({song[b] for b in range(len(rows)) if out["status"][b] == ir.OK}))
        batches.append(dict(rows=rows, ok=ok, shift=shift, first=first))
    return totals, batches


# ------------------------------------------------------------------------------------------------ arrange
def test_arrange_is_generate_on_the_concatenated_batch_bit_for_bit(setup):  # noqa: F811
    m, diff, _, tokens, _, noise, steps = setup
    fixed_draws(diff, steps)
    Lm = tokens.shape[1]
    tracks = TRACKS[:3]
    tok, song, track, cond = sampling.arrange(m, diff, BASE, tracks, 2, Lm, step=STEP, noise=noise, sharded=False)
    assert tok.dtype == torch.int64 and tok.shape == (6, Lm) and song.tolist() == [0, 0, 0, 1, 1, 1] and track.tolist() == [0, 1, 2] * 2
    assert song.dtype == torch.int32 and track.dtype == torch.int32 and song.is_cuda
    singles = [du.meta_to_batch({**BASE, **tracks[t]}, 1, Lm) for _ in range(2) for t in range(3)]
    cat = {k: torch.cat([c[k] for c in singles]) for k in ("input_ids", "input_mask")}
    assert torch.equal(cond["input_ids"], cat["input_ids"]) and torch.equal(cond["input_mask"], cat["input_mask"]) and set(cond) == set(cat)
    want = sampling.generate(m, diff, cat, step=STEP, noise=noise, sharded=False)
    assert torch.equal(tok, want)
    m2s = MetaToSequence()
    for b in range(6):
        assert tok[b, :11].tolist() == m2s.encode_meta({**BASE, **tracks[b % 3]}), "the anchored prefix is the track's meta"
    assert cond["input_ids"][1, 5].item() == 645 and cond["input_ids"][1, 9].item() == 723
    for bad in (dict(tracks=[]), dict(n_songs=0), dict(tracks=[dict(bpm=90)])):
        args = dict(tracks=tracks, n_songs=2)
        args.update(bad)
        with pytest.raises(ValueError):
            au.arrangement_batch(BASE, args["tracks"], args["n_songs"], Lm)


# ------------------------------------------------------------------------------------------------ the loop
def test_run_arrangement_replays_known_rows(tmp_path, monkeypatch):
    batch_list, mask = replay_batches()
    want_totals, want = restate(batch_list, mask)
    first = want[0]
    assert [int(not x) for x in first["ok"]] == [int(b == BROKEN) for b in range(N_SONGS * T)] and all(want[1]["ok"])
    assert first["first"] == [int(b == NO_BAR) for b in range(N_SONGS * T)]
    assert first["shift"] == [1920, 0, 1920, 1920, 0, 0, 0, 0] and want[1]["shift"] == [0] * 8
    copies = CopyCounter(monkeypatch)
    reps, logs, launches, n_copies = {}, {}, {}, {}
    for key, kw in (("plain", {}), ("partial", dict(keep_partial=True)), ("off", dict(interplay=False))):
        trials = iter([dev(t) for t in batch_list] * 2)
        logs[key] = []
        out = str(tmp_path / key)
        run = lambda: reps.update({key: sampling.run_arrangement(  # noqa: E731
            None, None, BASE, TRACKS, n_songs=N_SONGS, seq_len=L, num_songs=3, out_dir=out, sampler=lambda cond: next(trials),
            log=logs[key].append, **kw)})
        before = copies.n
        launches[key] = library_launches(run)
        n_copies[key] = copies.n - before
        logs[key] = [ln.replace(out, "<out>") for ln in logs[key]]
    # the files and their numbering: song 1 of the first batch has a broken row
    for key, n_files, members in (("plain", 3, [(0, 0), (1, 0), (1, 1)]), ("partial", 4, [(0, 0), (0, 1), (1, 0), (1, 1)]), ("off", 3, None)):
        rep = reps[key]
        assert sorted(os.listdir(tmp_path / key)) == ["song_%07d.midi" % n for n in range(n_files)]
        assert (rep.songs, rep.batches, rep.total_valid_count, rep.totals, rep.summary) == (n_files, 2, 2 * N_SONGS * T - 1, None, None)
    for name in os.listdir(tmp_path / "off"):
        assert open(tmp_path / "off" / name, "rb").read() == open(tmp_path / "plain" / name, "rb").read()
    for key, members in (("plain", [(0, 0), (1, 0), (1, 1)]), ("partial", [(0, 0), (0, 1), (1, 0), (1, 1)])):
        for n, (batch, s) in enumerate(members):
            tpb, tracks = au.read_song(tmp_path / key / ("song_%07d.midi" % n))
            rows = [b for b in range(s * T, (s + 1) * T) if want[batch]["ok"][b]]
            assert tpb == 480 and len(tracks) == len(rows) and len(rows) == (T - 1 if (batch, s) == (0, 1) else T)
            channels = iter(c for c in range(16) if c != 9)
            for (name, channel, program, notes), b in zip(tracks, rows):
                r, t = want[batch]["rows"][b], b % T
                known = r["notes"].astype(np.int64)
                known[:, :2] += want[batch]["shift"][b]
                assert notes.tolist() == known[np.argsort(known[:, 0], kind="stable")].tolist() and len(notes) == 16
                assert name == ("main_melody", "bass", "pad", "riff")[t] + "_%d" % t and program == (0, 32, 48, 0)[t]
                assert channel == (9 if t == 3 else next(channels))
            # the conductor track: the first decoded row's chord markers, moved with that row
            single = tmp_path / "single.midi"
            r0 = want[batch]["rows"][rows[0]]
            du.write_midi(single, r0["notes"], r0["chords"] + [want[batch]["shift"][rows[0]], 0], r0["meta"])
            a, b_ = open(tmp_path / key / ("song_%07d.midi" % n), "rb").read(), open(single, "rb").read()
            end0 = 22 + int.from_bytes(b_[18:22], "big")
            assert a[14:end0] == b_[14:end0]
    # the report against the restatement
    for key in ("plain", "partial"):
        assert reps[key].interplay == evaluation.InterplayTotals.ratios(want_totals.vector())
        assert logs[key][-1] == evaluation.interplay_block(reps[key].interplay)
    s = reps["plain"].interplay
    assert s["songs"] == 4 and s["rows"] == 2 * N_SONGS * (T - 1) - 1 and s["notes"] == 16 * s["rows"] and s["pairs"] > 50
    assert 0 < s["dissonance"] < 1 and s["bass_above"] == 0.0 and 0.0 <= s["melody_below"] < 0.2 and s["accompanied"] > 0.5
    assert reps["off"].interplay is None and [ln for ln in logs["plain"] if ln in logs["off"]] == logs["off"]
    assert [ln for ln in logs["plain"] if ln not in logs["off"]] == [evaluation.interplay_block(s)]
    # one more launch per batch and one more copy per run; neither without interplay
    per_batch = ["restore_chord_kernel", "decode_events_kernel"]
    assert launches["off"] == ["meta_to_batch_kernel"] * T + per_batch * 2
    assert launches["plain"] == launches["partial"] == ["meta_to_batch_kernel"] * T + (per_batch + ["interplay_counts_kernel"]) * 2
    assert n_copies["plain"] == n_copies["partial"] == n_copies["off"] + 1
    # max_batches holds, no batch at all, no output directory
    trials = iter([dev(t) for t in batch_list])
    rep = sampling.run_arrangement(None, None, BASE, TRACKS, n_songs=N_SONGS, seq_len=L, num_songs=100, out_dir=None, max_batches=1,
                                   sampler=lambda cond: next(trials), log=lambda s: None)
    assert (rep.songs, rep.batches, rep.total_valid_count) == (1, 1, N_SONGS * T - 1)
    assert rep.interplay == evaluation.InterplayTotals.ratios(restate(batch_list[:1], mask)[0].vector())
    none = sampling.run_arrangement(None, None, BASE, TRACKS, n_songs=N_SONGS, seq_len=L, num_songs=0, out_dir=None, log=lambda s: None)
    assert (none.songs, none.batches, none.interplay) == (0, 0, None)


def test_interplay_totals_take_a_mask_and_shifts_of_the_caller(tmp_path):
    batch_list, mask = replay_batches()
    song = torch.arange(N_SONGS * T, device=DEV, dtype=torch.int32) // T
    dec = du.decode_tokens(dev(batch_list[0]), dev(mask))
    shift = au.align_shift(dec, song)
    assert shift.dtype == torch.int32 and shift.is_cuda and shift.tolist() == restate(batch_list[:1], mask)[1][0]["shift"]
    totals = evaluation.InterplayTotals(DEV)
    assert totals.update(dec, song, shift=shift) is totals
    vec = totals.vector()
    assert vec.dtype == torch.int64 and vec.shape == (166,) and vec.is_cuda
    assert vec.cpu().tolist() == restate(batch_list[:1], mask)[0].vector()
    assert totals.summary() == totals.summary()
    empty = evaluation.InterplayTotals(DEV).update(dec, song, valid=torch.zeros(N_SONGS * T, device=DEV)).summary()
    assert empty["rows"] == 0 and empty["songs"] == 0 and all(np.isnan(empty[k]) for k in evaluation.InterplayTotals.RATIO_NAMES)
    with_drums = metric.interplay_counts(dec, song, shift=shift, pitched_only=False)
    assert (with_drums.status.cpu().numpy() == ir.OK).sum() == N_SONGS * T - 1
    assert with_drums.counts[:, 2].tolist() == [3, 3, 3, 3, 2, 2, 0, 2]


def test_run_generation_launches_what_it_launched():
    f = fixture()
    Lf = f["gen_tokens"].shape[1]
    trials = iter(dev(f["gen_tokens"]).view(3, 8, -1))
    box = []
    seen = library_launches(lambda: box.append(sampling.run_generation(
        None, None, f["gen_prefix"].tolist(), batch_size=8, seq_len=Lf, num_samples=6, out_dir=None, sampler=lambda cond: next(trials),
        log=lambda s: None)))
    assert seen == ["meta_to_batch_kernel"] + ["restore_chord_kernel", "decode_events_kernel"] * 2 and box[0].batches == 2
    assert not hasattr(box[0], "songs") and not hasattr(box[0], "interplay")


def test_one_pass_with_the_real_sampler(setup, monkeypatch, tmp_path):  # noqa: F811
    m, diff, _, tokens, _, _, _ = setup
    diff.noise_fn, diff.rng_mode = None, "philox"
    torch.manual_seed(17)
    Lm = tokens.shape[1]
    seen = []
    real = sampling.generate
    monkeypatch.setattr(sampling, "generate", lambda *a, **k: seen.append(real(*a, **k)) or seen[-1])
    try:
        rep = sampling.run_arrangement(m, diff, BASE, TRACKS[:3], n_songs=2, seq_len=Lm, num_songs=5, out_dir=str(tmp_path / "real"), step=STEP,
                                       max_batches=1, keep_partial=True, log=lambda s: None)
    except (IndexError, KeyError, RuntimeError):
        rep = None
    assert len(seen) == 1 and seen[0].shape == (6, Lm)
    cond, song, _ = au.arrangement_batch(BASE, TRACKS[:3], 2, Lm)
    if _fatal(seen[0], cond["input_mask"], False):
        assert rep is None
    else:
        # the tokens are what a random model makes of noise: mostly invalid rows - the loop ends, max_batches holds, the report is whole
        dec = du.decode_tokens(seen[0], cond["input_mask"])
        ok = (dec.status == du.OK).cpu().numpy().reshape(2, 3).sum(1)
        assert rep.batches == 1 and rep.total_valid_count == int(ok.sum()) and rep.songs == int((ok >= 2).sum())
        assert sorted(os.listdir(tmp_path / "real")) == ["song_%07d.midi" % n for n in range(rep.songs)]
        want = evaluation.InterplayTotals(DEV).update(dec, song, shift=au.align_shift(dec, song)).summary()
        assert set(rep.interplay) == set(want) and all(rep.interplay[k] == want[k] or (np.isnan(rep.interplay[k]) and np.isnan(want[k])) for k in want)
