"""The denoiser engine's path matrix (GPU): csrc/engine.hip composes the library's kernels into mh_denoiser_forward / _forward_sqnorm /
_forward_round, mh_denoiser_head / _layers / _tail and mh_time_embed over ONE carved workspace with deliberate aliasing (the residual
stream in place, the FFN intermediate on top of q | k | V^T | attention output, a slack behind V^T, two statistics buffers).  The
kernels have their own parity matrices; this one proves the wiring.  For every path the chooser can take (tests/engine_chain.py CASES;
tests/test_engine_plan_cpu.py checks that the table reaches them all):

  1. the workspace is exactly mh_denoiser_workspace_bytes between 64 KiB guard bands, the outputs NaN / -1 with slack behind them:
     bands and slack untouched, outputs finite; one byte less is refused with nothing written
  2. the outputs do not depend on what the workspace held: 0x00, 0xFF (NaN in every storage type), the residue of another shape
  3. engine == chain, bit for bit: the same C-ABI calls issued by the test over fresh, NaN-filled, unaliased, not-in-place buffers
     (engine_chain.run_chain), and the same launches (kernel text, detail, grid, block) in the same order, which agree with the plan key
  4. head / layers over uneven row windows of caller-owned row buffers / tail == the monolithic forward, rows outside the windows untouched
  5. the coarse one: against oracle.denoiser.forward evaluated in float64, at the tolerances the project already states
     (tests/test_engine_gpu.py, tests/test_defer_ln_gpu.py): fp32 and split precision max < 2e-4; bf16 mean <= 0.02, max <= 0.25
  6. mh_time_embed with and without padded hidden columns: the same guards, pre-fills and chain; fp32 within 2e-5 of float64
  7. error paths on the device: every argument check returns before the first launch (tests/test_engine_plan_cpu.py has them all), so
     what remains here is "refused and nothing written" for the short workspace of each entry point (inside checks 1, 4 and 6)

A case that sets a switch of the debug library runs inside engine_chain.switches: the debug library for the block (what the dbg_lib
fixture does), the engine built with the switch on, the default back in `finally`.  An A/B build of the library without the aliasing
(-DMH_WS_INPLACE=0 -DMH_WS_ALIAS=0) passes the matrix unchanged (engine_chain.build_macros reads the build off the workspace size).
Measured figures, the launch list per case and the mutations of engine.hip the matrix catches: profiles/engine_matrix.txt."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import engine_chain as ec  # noqa: E402
from gpu_helpers import same  # noqa: E402
from musediffusion_amd import _lib  # noqa: E402
from musediffusion_amd._lib import MH_BF16, MH_BF16X3, MH_ERR_INVALID, MH_F32  # noqa: E402
from musediffusion_amd.engine import DenoiserEngine  # noqa: E402
from oracle import denoiser as odn  # noqa: E402

DEV = "cuda"
CASES = ec.CASES
IDS = [c["name"] for c in CASES]
BAND, SENTINEL, SLACK = 65536, 0xA5, 1024          # guard bands of the workspace (bytes, byte value); elements behind every output
FILLS = ("zero", "ones", "residue")
every_case = pytest.mark.parametrize("c", CASES, ids=IDS)


def knob_args(c):
    return {k: v for k, v in c["knobs"].items() if k == "prescale_q"}


# ------------------------------------------------------------------------------------------------------------------ buffers
class GuardedBytes:
    """`nbytes` of workspace inside one allocation, 64 KiB of a sentinel byte on both sides: a region misplaced by less than a band lands
    in a band, not outside the allocation"""

    def __init__(self, nbytes, fill=0xFF):
        self.n = int(nbytes)
        self.buf = torch.full((self.n + 2 * BAND,), SENTINEL, dtype=torch.uint8, device=DEV)
        self.ws = self.buf[BAND:BAND + self.n]
        if isinstance(fill, torch.Tensor):          # residue of another run, repeated / cut to size
            reps = -(-self.n // max(1, fill.numel()))
            self.ws.copy_(fill.repeat(reps)[:self.n])
        else:
            self.ws.fill_(fill)
        self.ptr = self.ws.data_ptr()
        assert self.ptr % 256 == 0

    def check_bands(self, what):
        assert bool((self.buf[:BAND] == SENTINEL).all()), "%s: guard band below the workspace written" % what
        assert bool((self.buf[BAND + self.n:] == SENTINEL).all()), "%s: guard band above the workspace written" % what


class Out:
    """n elements of fp32 NaN / int32 -1 (every byte 0xFF) with SLACK more behind them"""

    def __init__(self, n, dtype=torch.float32):
        self.n = n
        self.buf = torch.full(((n + SLACK) * 4,), 0xFF, dtype=torch.uint8, device=DEV).view(dtype)
        self.ptr = self.buf.data_ptr()

    def untouched(self):
        return bool((self.buf.view(torch.uint8) == 0xFF).all())

    def get(self, what):
        assert bool((self.buf[self.n:].view(torch.uint8) == 0xFF).all()), "%s: written behind its end" % what
        return self.buf[:self.n].cpu().numpy()


def nan_rows(H, n_rows, fill=0xFF):
    """a K32-panel row buffer [H / 32][n_rows][32] bf16, every byte `fill`"""
    return torch.full((H // 32, n_rows, 64), fill, dtype=torch.uint8, device=DEV)


# ------------------------------------------------------------------------------------------------------------------ per-case context
def state_dict(c):
    """oracle.denoiser.random_state_dict with every LayerNorm's gain in [0.7, 1.3] and shift ~ 0.2 N(0, 1), each vector its own draw:
    swapped gain / shift vectors change the result"""
    sd = odn.random_state_dict(c["E"], c["H"], c["F"], c["nL"], c["V"], c["L"] + ec.L_EXTRA, c["Tt"], seed=41, emb_std=0.5)
    g = torch.Generator().manual_seed(42)
    for k in sorted(sd):
        if "LayerNorm.weight" in k:
            sd[k] = 0.7 + 0.6 * torch.rand(c["H"], generator=g)
        elif "LayerNorm.bias" in k:
            sd[k] = 0.2 * torch.randn(c["H"], generator=g)
    return sd


class Ctx:
    def __init__(self, c):
        self.c = c
        self.sd = state_dict(c)
        # (built inside the caller's ec.switches block: defer_ln = 2 at construction makes the engine pack the folded operands)
        self.eng = DenoiserEngine(ec.engine_cfg(c), c["dtype"], DEV, panel=c["panel"])
        self.eng.load_state_dict({k: v.to(DEV) for k, v in self.sd.items()})
        g = torch.Generator().manual_seed(7)
        B, L, E = c["B"], c["L"], c["E"]
        self.x_host = torch.randn(B + 1, L + 8, E, generator=g)
        self.t_host = torch.tensor([900.0, 15.5, 333.0, 1.25])[:B + 1]
        self.x = self.x_host[:B, :L].contiguous().to(DEV)
        self.emb_t = self.eng.time_embed(self.t_host.to(DEV))
        torch.cuda.synchronize()
        self.desc = self.eng._desc
        self.need = int(_lib.lib().mh_denoiser_workspace_bytes(C.byref(self.desc), B, L))
        self.memo = {}

    def round_operands(self):
        """the split table of mh_denoiser_forward_round for this model's word embedding (+ what an update reads)"""
        if "round" not in self.memo:
            c = self.c
            table = self.sd["word_embedding.weight"].to(DEV).contiguous()
            buf = torch.empty(int(_lib.lib().mh_round_split_bytes(c["E"], c["V"])), dtype=torch.uint8, device=DEV)
            _lib.check(_lib.lib().mh_round_split_table(table.data_ptr(), None, c["V"], c["E"], buf.data_ptr(), _lib.current_stream()), "mh_round_split_table")
            g = torch.Generator().manual_seed(9)
            noise = torch.randn(c["B"], c["L"], c["E"], generator=g).to(DEV)
            coef = torch.tensor([0.3, 0.7, 0.05, 1.1, 0.4, 0.9, 0.2, 0.0], dtype=torch.float32, device=DEV)      # one mh_step_coef row
            torch.cuda.synchronize()
            self.memo["round"] = (table, buf, noise, coef)
        return self.memo["round"]


_CTX = {}


def ctx_of(c):
    if c["name"] not in _CTX:
        _CTX[c["name"]] = Ctx(c)
    return _CTX[c["name"]]


class Update:
    """an mh_step_update over buffers of its own: x_t (a copy of the forward's input, stepped in place), pred_xstart, mean"""

    def __init__(self, ctx):
        table, _, noise, coef = ctx.round_operands()
        n = ctx.x.numel()
        self.x, self.pred, self.mean = Out(n), Out(n), Out(n)
        self.x.buf[:n].copy_(ctx.x.view(-1))
        u = self.u = _lib.StepUpdate()
        u.x, u.x_start, u.mask, u.mask_per_elem = self.x.ptr, None, None, 0
        u.table, u.coef, u.clip, u.ddim = table.data_ptr(), coef.data_ptr(), 1, 0
        u.pred_xstart, u.mean_out, u.noise, u.rng = self.pred.ptr, self.mean.ptr, noise.data_ptr(), None

    def get(self):
        return dict(x_next=self.x.get("x_t"), pred_xstart=self.pred.get("pred_xstart"), mean=self.mean.get("mean"))


def engine_forward(ctx, want, ws, nbytes, x=None, emb_row=None, B=None, L=None):
    """one entry point of the engine, called directly (exact workspace size, return code back).  -> (rc, dict of Out, Update or None)"""
    c, lib, d = ctx.c, _lib.lib(), C.byref(ctx.desc)
    B, L = B or c["B"], L or c["L"]
    x = ctx.x if x is None else x
    N, st = B * L, _lib.current_stream()
    o = dict(out=Out(N * c["E"]))
    upd = None
    if want == "out":
        rc = lib.mh_denoiser_forward(d, x.data_ptr(), ctx.emb_t.data_ptr(), _lib.ptr(emb_row), o["out"].ptr, B, L, ws, nbytes, st)
    elif want == "sqnorm":
        o["sqnorm"] = Out(N)
        rc = lib.mh_denoiser_forward_sqnorm(d, x.data_ptr(), ctx.emb_t.data_ptr(), _lib.ptr(emb_row), o["out"].ptr, o["sqnorm"].ptr, B, L, ws, nbytes, st)
    else:
        o["idx"] = Out(N, torch.int32)
        upd = Update(ctx) if want == "round+upd" else None
        rc = lib.mh_denoiser_forward_round(d, x.data_ptr(), ctx.emb_t.data_ptr(), _lib.ptr(emb_row), o["out"].ptr, ctx.round_operands()[1].data_ptr(), c["V"],
                                           o["idx"].ptr, C.byref(upd.u) if upd else None, B, L, ws, nbytes, st)
    torch.cuda.synchronize()
    return rc, o, upd


def results(o, upd, what):
    r = {k: v.get("%s %s" % (what, k)) for k, v in o.items()}
    if upd is not None:
        r.update(upd.get())
    return r


def engine_results(ctx, want, fill=0xFF):
    """the entry point on an exact guarded workspace -> host arrays; bands, slack and finiteness checked"""
    what = "%s %s" % (ctx.c["name"], want)
    gw = GuardedBytes(ctx.need, fill)
    rc, o, upd = engine_forward(ctx, want, gw.ptr, gw.n)
    assert rc == 0, (what, rc, _lib.lib().mh_last_error())
    gw.check_bands(what)
    r = results(o, upd, what)
    for k, v in r.items():
        assert np.isfinite(v).all() if v.dtype != np.int32 else ((v >= 0) & (v < ctx.c["V"])).all(), "%s: %s not all written" % (what, k)
    return r


def mono(ctx, want="out"):
    """the monolithic forward's results, computed once per case and entry point and shared (never modified)"""
    if ("mono", want) not in ctx.memo:
        ctx.memo["mono", want] = engine_results(ctx, want)
    return ctx.memo["mono", want]


def residue(ctx):
    """the bytes a forward of ANOTHER shape (B + 1, L + 8) leaves in its workspace"""
    if "residue" not in ctx.memo:
        c = ctx.c
        B, L = c["B"] + 1, c["L"] + 8
        need = int(_lib.lib().mh_denoiser_workspace_bytes(C.byref(ctx.desc), B, L))
        gw = GuardedBytes(need, 0x00)
        rc, o, _ = engine_forward(ctx, "out", gw.ptr, gw.n, x=ctx.x_host.to(DEV), B=B, L=L)
        assert rc == 0, _lib.lib().mh_last_error()
        gw.check_bands("residue run")
        assert np.isfinite(o["out"].get("residue run")).all()
        ctx.memo["residue"] = gw.ws.clone()
    return ctx.memo["residue"]


def fill_of(ctx, fill):
    return residue(ctx) if fill == "residue" else {"zero": 0x00, "ones": 0xFF}[fill]


def wants_of(c):
    return [(c, w) for w in c["wants"]]


CASE_WANTS = [cw for c in CASES for cw in wants_of(c)]
CW_IDS = ["%s-%s" % (c["name"], w) for c, w in CASE_WANTS]
every_entry = pytest.mark.parametrize("c,want", CASE_WANTS, ids=CW_IDS)


# ------------------------------------------------------------------------------------------------------------------ 1. guards
@every_entry
def test_exact_workspace_between_guards(c, want):
    with ec.switches(c["knobs"]):
        ctx = ctx_of(c)
        lay = ec.workspace_layout(ctx.desc, c["B"], c["L"], *ec.build_macros())
        assert lay.total == ctx.need
        mono(ctx, want)                              # bands, slack, finiteness (engine_results)


@every_entry
def test_short_workspace_is_refused_and_nothing_written(c, want):
    with ec.switches(c["knobs"]):
        ctx = ctx_of(c)
        gw = GuardedBytes(ctx.need, 0x3C)
        rc, o, upd = engine_forward(ctx, want, gw.ptr, gw.n - 1)
        assert rc == MH_ERR_INVALID and b"too small" in _lib.lib().mh_last_error()
        assert all(v.untouched() for v in o.values()), "refused call wrote an output"
        assert bool((gw.ws == 0x3C).all()), "refused call wrote the workspace"
        gw.check_bands("refused call")
        if upd is not None:
            assert upd.pred.untouched() and upd.mean.untouched() and torch.equal(upd.x.buf[:ctx.x.numel()], ctx.x.view(-1))


# ------------------------------------------------------------------------------------------------------------------ 2. pre-fill
@every_entry
@pytest.mark.parametrize("fill", FILLS)
def test_result_independent_of_workspace_contents(c, want, fill):
    with ec.switches(c["knobs"]):
        ctx = ctx_of(c)
        got = engine_results(ctx, want, fill_of(ctx, fill))
        same(got, mono(ctx, want), "%s %s workspace pre-filled with %s" % (c["name"], want, fill))


# ------------------------------------------------------------------------------------------------------------------ 3. engine == chain
def launches(fn):
    return [(r.kernel, r.detail, r.grid, r.block) for r in _lib.record_launches(fn)]


def chain(ctx, want):
    """run_chain's results and launches, once per case and entry point"""
    if ("chain", want) not in ctx.memo:
        c, box, upd = ctx.c, {}, None
        round_to = None
        if want.startswith("round"):
            upd = Update(ctx) if want == "round+upd" else None
            round_to = (ctx.round_operands()[1].data_ptr(), c["V"], upd.u if upd else None)

        def go():
            box["r"] = ec.run_chain(ctx.eng, ctx.x, ctx.emb_t, None, c["B"], c["L"], want="round" if round_to else want, knobs=knob_args(c), round_to=round_to)
        rec = launches(go)
        r = {k: box["r"][k] for k in ("out", "sqnorm", "idx") if box["r"][k] is not None}
        r["out"] = r["out"].reshape(-1)
        if upd is not None:
            r.update(upd.get())
        ctx.memo["chain", want] = (r, rec, box["r"]["key"])
    return ctx.memo["chain", want]


@every_entry
def test_engine_equals_unaliased_chain(c, want):
    with ec.switches(c["knobs"]):
        ctx = ctx_of(c)
        want_r, _, key = chain(ctx, want)
        assert key == (ec.ROUND_KEY if want.startswith("round") else c["key"]), key
        got = mono(ctx, want)
        assert set(got) == set(want_r)
        same(got, want_r, "%s %s engine vs chain" % (c["name"], want))


def path_of_launches(rec, c, want):
    """the path key the recorded launch details spell (panel path), from the notes the kernels leave with the recorder"""
    det = [r[1] for r in rec]
    nL = c["nL"]
    n_head, n_add = sum(d.startswith("head rows=") for d in det), sum(" add=1 " in d for d in det)
    n_stream, n_small = sum(d.startswith("attn_stream ") for d in det), sum(d.startswith("attn_small ") for d in det)
    n_pre = sum(d.startswith("attn_stream ") and " pre=1 " in d for d in det)
    n_ln = sum(" add=0 " in d and d.startswith("x=") for d in det)
    assert n_head + n_add == 1 and n_stream + n_small == nL and n_pre in (0, nL), det
    head = "fused" if n_head else ("chain" if c["E"] != c["H"] else "none")
    attn = "none" if nL == 0 else ("tiled" if n_small else ("stream-prescaled" if n_pre else "stream"))
    n_epi = sum(" epi=3 " in d for d in det)          # the GEMM with the LayerNorm epilogue (gemm_args.h)
    assert (n_ln, n_epi) in ((0, 2 * nL), (1, 0), (2 * nL, 0)), det
    ln = "none" if nL == 0 else ("epilogue" if n_epi else ("kernel" if n_ln == 2 * nL else "defer"))
    last = det[-1]
    tail = "round" if last.startswith("tail+round") else ("fused" if last.startswith("tail rows=") else ("unpack" if c["E"] == c["H"] else "chain"))
    return ec.PANEL % (head, attn, ln, tail)


@every_entry
def test_engine_launches_equal_chain_launches(c, want):
    with ec.switches(c["knobs"]):
        ctx = ctx_of(c)
        _, chain_rec, key = chain(ctx, want)
        gw = GuardedBytes(ctx.need)
        box = {}

        def go():
            box["rc"] = engine_forward(ctx, want, gw.ptr, gw.n)[0]
        eng_rec = launches(go)
        assert box["rc"] == 0
        print("\nengine_matrix launches %s %s | %s" % (c["name"], want, key))
        for r in eng_rec:
            print("    %s <<<%d, %d>>> %s" % (r[0], r[2], r[3], r[1]))
        assert eng_rec == chain_rec, [(i, a, b) for i, (a, b) in enumerate(zip(eng_rec, chain_rec)) if a != b][:3] or (len(eng_rec), len(chain_rec))
        if key.startswith("panel"):
            assert path_of_launches(eng_rec, c, want) == key
        elif key.startswith("split"):
            assert all(r[1].startswith("split ") for r in eng_rec) and sum("+LN" in r[1] for r in eng_rec) == (2 * c["nL"] if key.endswith("ln=fused") else 0)
        else:
            assert not any(r[1].startswith(("split ", "head ", "tail ", "attn_stream")) for r in eng_rec)


# ------------------------------------------------------------------------------------------------------------------ 4. phases
PHASED = [c for c in CASES if c["E"] != c["H"] and c["nL"] > 0 and c["dtype"] == MH_BF16 and c["panel"]]


def phased(ctx, fill, emb_row=None, x=None):
    """head over the full batch -> rows A; layers over the slices [0, 1) and [1, B) of A -> B, each on an exact guarded workspace of its own;
    tail over the full batch.  Both row buffers have 24 rows beyond B L and start as `fill` bytes."""
    c, lib, d, st = ctx.c, _lib.lib(), C.byref(ctx.desc), _lib.current_stream()
    B, L, H = c["B"], c["L"], c["H"]
    N, ld = B * L, B * L + 24
    x = ctx.x if x is None else x
    ra, rb = nan_rows(H, ld, fill), nan_rows(H, ld, fill)
    out = Out(N * c["E"])
    need = lambda b: int(lib.mh_denoiser_workspace_bytes(d, b, L))
    gw = GuardedBytes(need(B))
    short = lib.mh_denoiser_head(d, x.data_ptr(), ctx.emb_t.data_ptr(), _lib.ptr(emb_row), ra.data_ptr(), ld, B, L, gw.ptr, gw.n - 1, st)
    assert short == MH_ERR_INVALID and bool((ra == fill).all())
    _lib.check(lib.mh_denoiser_head(d, x.data_ptr(), ctx.emb_t.data_ptr(), _lib.ptr(emb_row), ra.data_ptr(), ld, B, L, gw.ptr, gw.n, st), "mh_denoiser_head")
    gw.check_bands("head")
    for first, items in ((0, 1), (1, B - 1)):
        if items == 0:
            continue
        gs = GuardedBytes(need(items), 0x00 if first else 0xFF)
        off = first * L * 64                          # first row of the window, in bytes of one panel
        short = lib.mh_denoiser_layers(d, ra.data_ptr() + off, ld, rb.data_ptr() + off, ld, items, L, gs.ptr, gs.n - 1, st)
        assert short == MH_ERR_INVALID and bool((rb[:, first * L:(first + items) * L] == fill).all())
        _lib.check(lib.mh_denoiser_layers(d, ra.data_ptr() + off, ld, rb.data_ptr() + off, ld, items, L, gs.ptr, gs.n, st), "mh_denoiser_layers")
        gs.check_bands("layers")
    gt = GuardedBytes(need(B), 0x00)
    short = lib.mh_denoiser_tail(d, rb.data_ptr(), ld, out.ptr, B, L, gt.ptr, gt.n - 1, st)
    assert short == MH_ERR_INVALID and out.untouched()
    _lib.check(lib.mh_denoiser_tail(d, rb.data_ptr(), ld, out.ptr, B, L, gt.ptr, gt.n, st), "mh_denoiser_tail")
    torch.cuda.synchronize()
    gt.check_bands("tail")
    for name, r in (("head's", ra), ("layers'", rb)):
        assert bool((r[:, N:] == fill).all()), "%s row buffer written outside [0, B L)" % name
        if fill == 0xFF:          # (no bf16 row of 32 NaNs with every bit set is ever computed)
            assert not bool((r[:, :N] == fill).all(dim=-1).any()), "%s row buffer has unwritten rows" % name
    return dict(out=out.get("phased out"))


@pytest.mark.parametrize("fill", (0xFF, 0x00), ids=("ones", "zero"))
@pytest.mark.parametrize("c", PHASED, ids=[c["name"] for c in PHASED])
def test_phases_over_uneven_windows_equal_monolithic(c, fill):
    with ec.switches(c["knobs"]):
        ctx = ctx_of(c)
        assert _lib.lib().mh_denoiser_phases_supported(C.byref(ctx.desc)) == 1
        same(phased(ctx, fill), dict(out=mono(ctx)["out"]), "%s phased vs monolithic" % c["name"])


@pytest.mark.parametrize("c", PHASED, ids=[c["name"] for c in PHASED])
def test_phases_with_permuted_rows(c):
    """the head with a permuted emb_row on the permuted input gives the permuted rows of the forward"""
    with ec.switches(c["knobs"]):
        ctx = ctx_of(c)
        B = c["B"]
        perm = list(range(B))[::-1] if B > 1 else [0]
        if B == 1:                                        # one item: take its time row from elsewhere in the table instead
            rows = torch.tensor([1], dtype=torch.int32, device=DEV)
            got = phased(ctx, 0xFF, emb_row=rows)
            gw = GuardedBytes(ctx.need)
            rc, o, _ = engine_forward(ctx, "out", gw.ptr, gw.n, emb_row=rows)
            assert rc == 0 and ctx.emb_t.shape[0] > 1
            want = o["out"].get("out")
            assert not np.array_equal(want, mono(ctx)["out"])
        else:
            rows = torch.tensor(perm, dtype=torch.int32, device=DEV)
            got = phased(ctx, 0xFF, emb_row=rows, x=ctx.x[perm].contiguous())
            want = mono(ctx)["out"].reshape(B, -1)[perm].reshape(-1)
        same(got, dict(out=want), "%s phased, permuted" % c["name"])


def test_phases_unsupported_where_the_plan_says_so():
    for c in CASES:
        if c not in PHASED and not c["knobs"]:
            assert _lib.lib().mh_denoiser_phases_supported(C.byref(ctx_of(c).desc)) == 0, c["name"]


# ------------------------------------------------------------------------------------------------------------------ 5. float64 reference
_REF = {}


def reference(ctx):
    c = ctx.c
    k = (c["E"], c["H"], c["nh"], c["F"], c["nL"], c["B"], c["L"], c["Tt"], c["V"])
    if k not in _REF:
        with torch.no_grad():
            _REF[k] = ec.forward64(ctx.sd, ctx.x_host[:c["B"], :c["L"]], ctx.t_host[:c["B"]], c["nh"], c["Tt"]).numpy()
    return _REF[k]


@every_case
def test_chain_against_float64_oracle(c):
    with ec.switches(c["knobs"]):
        ctx = ctx_of(c)
        got = chain(ctx, "out")[0]["out"].astype(np.float64)
    err = np.abs(got - reference(ctx).reshape(-1))
    print("\nengine_matrix float64 %s | %s | mean %.3e max %.3e" % (c["name"], c["key"], err.mean(), err.max()))
    if c["dtype"] == MH_BF16:
        assert err.mean() <= 0.02 and err.max() <= 0.25
    else:
        assert err.max() < 2e-4


# ------------------------------------------------------------------------------------------------------------------ 6. time embedding
TIME_CASES = [(Tt, dt) for Tt in (24, 16) for dt in (MH_F32, MH_BF16, MH_BF16X3)]
_TIME = {}


def time_ctx(Tt, dtype):
    if (Tt, dtype) not in _TIME:
        c = ec.case("time", 32, 128, 4, 256, 1, 5, 8, "", dtype=dtype, Tt=Tt)
        sd = state_dict(c)
        eng = DenoiserEngine(ec.engine_cfg(c), dtype, DEV).load_state_dict({k: v.to(DEV) for k, v in sd.items()})
        t = torch.tensor([0.0, 1.0, 15.5, 999.0, 1999.0])
        _TIME[Tt, dtype] = (eng, sd, t, t.to(DEV))
    return _TIME[Tt, dtype]


def time_embed(eng, t_dev, fill, short=0):
    B, H = t_dev.numel(), eng.cfg["H"]
    hid, need = ec.time_layout(eng._desc, B)
    gw = GuardedBytes(need, fill)
    out = Out(B * H)
    rc = _lib.lib().mh_time_embed(C.byref(eng._desc), t_dev.data_ptr(), out.ptr, B, gw.ptr, gw.n - short, _lib.current_stream())
    torch.cuda.synchronize()
    gw.check_bands("time_embed")
    return rc, out, gw


@pytest.mark.parametrize("Tt,dtype", TIME_CASES, ids=["Tt%d-%s" % (Tt, ec.DTYPE_NAME[dt]) for Tt, dt in TIME_CASES])
def test_time_embed(Tt, dtype):
    eng, sd, t, t_dev = time_ctx(Tt, dtype)
    d = eng._desc
    assert (d.Tt_pad, d.T4_pad) == (64, 128 if Tt == 24 else 64) and (d.T4_pad != 4 * Tt) == (Tt == 24)
    rc, out, gw = time_embed(eng, t_dev, 0x3C, short=1)
    assert rc == MH_ERR_INVALID and out.untouched() and bool((gw.ws == 0x3C).all())
    want = ec.time_chain(eng, t_dev).reshape(-1)
    residue = torch.full((4096,), 0x7F, dtype=torch.uint8, device=DEV)         # 0x7F7F...: large finite values in every storage type
    for name, fill in (("zero", 0x00), ("ones", 0xFF), ("residue", residue)):
        rc, out, gw = time_embed(eng, t_dev, fill)
        assert rc == 0, _lib.lib().mh_last_error()
        got = out.get("emb_t")
        assert np.isfinite(got).all(), name
        same(dict(emb_t=got), dict(emb_t=want), "time_embed Tt=%d, workspace pre-filled with %s" % (Tt, name))
    ref = ec.time_embed64(sd, t, Tt).numpy().reshape(-1)
    err = np.abs(want.astype(np.float64) - ref)
    print("\nengine_matrix time_embed Tt=%d %s | mean %.3e max %.3e" % (Tt, ec.DTYPE_NAME[dtype], err.mean(), err.max()))
    if dtype != MH_BF16:                   # (split precision runs the time MLP in fp32)
        assert err.max() < 2e-5
