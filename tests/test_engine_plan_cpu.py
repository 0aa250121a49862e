"""The denoiser engine without a device (the library loads without one, as tests/test_grammar_cpu.py relies on): the Python restatement of
its workspace carving (tests/engine_chain.py) against mh_denoiser_workspace_bytes, the path key of every case of the GPU matrix
(tests/test_engine_matrix_gpu.py) against the full set of paths, and the argument checks that return before any device call - each
called with a descriptor whose pointers are dummies, so a check that did reach the device would fault here, not pass.

None of the argument checks had to move to the GPU file: check_model, the shape checks, carve and the workspace-size check all run
before denoiser_run's first launch, and the wrappers' own checks before denoiser_run."""
import ctypes as C
import itertools

import pytest

import engine_chain as ec
from musediffusion_amd import _lib
from musediffusion_amd._lib import MH_BF16, MH_BF16X3, MH_ERR_INVALID, MH_F16X3, MH_F32
from test_engine_matrix_gpu import CASES

PANEL = ec.PANEL
# every path the engine can take that the matrix must reach (head / attention / LayerNorm / tail forms of the bf16 panel path, the
# row-major paths, split precision with both LayerNorm forms)
ALL_KEYS = {
    PANEL % ("fused", "stream", "epilogue", "fused"),
    PANEL % ("fused", "stream", "epilogue", "round"),
    PANEL % ("chain", "tiled", "epilogue", "chain"),
    PANEL % ("chain", "stream", "epilogue", "chain"),
    PANEL % ("fused", "stream", "defer", "fused"),
    PANEL % ("fused", "tiled", "kernel", "fused"),
    PANEL % ("fused", "stream", "kernel", "fused"),
    PANEL % ("none", "stream", "defer", "unpack"),
    PANEL % ("fused", "none", "none", "fused"),
    PANEL % ("fused", "stream-prescaled", "epilogue", "fused"),
    PANEL % ("fused", "stream-prescaled", "defer", "fused"),
    "rowmajor-f32 | proj=1", "rowmajor-f32 | proj=0", "rowmajor-bf16 | proj=1",
    "split-bf16x3 | proj=1 ln=kernel", "split-f16x3 | proj=0 ln=kernel", "split-bf16x3 | proj=1 ln=fused",
}


def lib():
    return _lib.lib()


def desc(dtype=MH_BF16, E=128, H=512, nh=8, F=1024, nL=2, Tt=32, panel=True, L=64):
    return ec.dummy_desc(ec.case("t", E, H, nh, F, nL, 2, L, "", dtype=dtype, panel=panel, Tt=Tt))


# ------------------------------------------------------------------------------------------------------------------ workspace size
def test_workspace_layout_equals_workspace_bytes():
    n = 0
    shapes = [(1, 8), (2, 8), (1, 24), (3, 40), (2, 64), (3, 528)]       # B L H es on both sides of a multiple of 256 bytes
    for dtype, H in itertools.product((MH_F32, MH_BF16, MH_BF16X3, MH_F16X3), (64, 128, 512, 768)):
        for F in (4 * H - 64, 4 * H, 4 * H + 64, 8 * H):
            for panel, (B, L) in itertools.product((True, False), shapes):
                nh = H // 64
                d, keep = desc(dtype, E=36 if H > 64 else 64, H=H, nh=nh, F=F, panel=panel, L=L)
                lay = ec.workspace_layout(d, B, L)
                assert lay.total == lib().mh_denoiser_workspace_bytes(C.byref(d), B, L), (dtype, H, F, panel, B, L)
                assert lay.ffn_aliased == (F <= 4 * H), (H, F, B, L)          # the alias condition: F <= 4H up to the V^T slack and the padding
                starts = sorted(set(lay.regions.values()))
                assert all(off % 256 == 0 for off, _ in starts)
                for (o0, s0), (o1, _) in zip(starts, starts[1:]):             # distinct regions do not overlap except the FFN alias
                    assert o0 + s0 <= o1 or lay.regions["ffn"] in ((o0, s0), (o1, _)), (lay.regions,)
                unaligned = any(s % 256 for _, s in lay.regions.values())
                n += unaligned
    assert n > 0, "no shape with a region that is not a multiple of 256 bytes"


def test_workspace_alias_condition_at_the_boundary():
    """N F es <= the bytes of q | k | V^T (+ 256) | attention output after alignment: F = 4H is aliased, and so is F = 4H + 64 only when
    N is small enough for the slack and padding to hold the extra columns"""
    d, keep = desc(H=128, nh=4, F=4 * 128 + 64)
    assert ec.workspace_layout(d, 1, 8).ffn_aliased == (8 * 576 * 2 <= 4 * ec.align256(8 * 128 * 2) + 256)
    assert not ec.workspace_layout(d, 3, 40).ffn_aliased
    d, keep = desc(H=128, nh=4, F=4 * 128)
    assert ec.workspace_layout(d, 3, 40).ffn_aliased
    for B, L in ((1, 8), (3, 40)):
        assert ec.workspace_layout(d, B, L).total == lib().mh_denoiser_workspace_bytes(C.byref(d), B, L)


def test_workspace_time_embedding_need_can_exceed_the_forward():
    d, keep = desc(MH_F32, E=64, H=64, nh=2, F=64, nL=1, Tt=2048)
    lay = ec.workspace_layout(d, 1, 8)
    assert lay.time_embed > lay.forward and lay.total == lay.time_embed == lib().mh_denoiser_workspace_bytes(C.byref(d), 1, 8)
    assert ec.time_layout(d, 1)[1] <= lay.total
    lay = ec.workspace_layout(d, 2, 512)
    assert lay.time_embed < lay.forward and lay.total == lib().mh_denoiser_workspace_bytes(C.byref(d), 2, 512)


def test_product_build_aliases():
    assert ec.build_macros() == (True, True)


def test_workspace_layout_without_aliasing():
    """the restatement follows the build macros by parameter: two residual buffers, the FFN buffer on its own"""
    d, keep = desc()
    a, b = ec.workspace_layout(d, 2, 64), ec.workspace_layout(d, 2, 64, inplace=False, alias=False)
    N, H, F = 128, 512, 1024
    assert a.regions["bufX1"] == a.regions["bufX"] and a.regions["ffn"][0] == a.regions["q"][0]
    assert b.regions["bufX1"] != b.regions["bufX"] and not b.ffn_aliased
    assert b.forward == a.forward + ec.align256(N * H * 2) + ec.align256(N * F * 2)


def test_workspace_bytes_of_nothing():
    d, keep = desc()
    assert lib().mh_denoiser_workspace_bytes(None, 2, 64) == 0
    for B, L in ((0, 64), (-1, 64), (2, 0), (2, -8)):
        assert lib().mh_denoiser_workspace_bytes(C.byref(d), B, L) == 0


# ------------------------------------------------------------------------------------------------------------------ coverage
def test_matrix_reaches_every_path():
    keys = set()
    for c in CASES:
        with ec.switches(c["knobs"]):
            d, keep = ec.dummy_desc(c)
            for want in c["wants"]:
                key = ec.plan(d, c["B"], c["L"], dict(c["knobs"], want="round" if want.startswith("round") else "out"))
                if not want.startswith("round"):
                    assert key == c["key"], (c["name"], key)
                keys.add(key)
            if any(w.startswith("round") for w in c["wants"]):
                assert lib().mh_denoiser_rounds_in_forward(C.byref(d), c["V"]) == 1, c["name"]
            if "sqnorm" in c["wants"]:
                assert lib().mh_denoiser_gives_sqnorm(C.byref(d)) == 1, c["name"]
    assert keys == ALL_KEYS, (sorted(keys - ALL_KEYS), sorted(ALL_KEYS - keys))
    assert lib().mh_denoiser_get_fuse_ln() == 1 and lib().mh_denoiser_get_defer_ln() == 1          # the switches are back


def test_matrix_reaches_both_ffn_placements_and_phase_support():
    aliased, phased = set(), set()
    for c in CASES:
        with ec.switches(c["knobs"]):
            d, keep = ec.dummy_desc(c)
            aliased.add(ec.workspace_layout(d, c["B"], c["L"]).ffn_aliased)
            phased.add((lib().mh_denoiser_phases_supported(C.byref(d)), bool(d.panel), bool(d.has_proj), d.nL > 0))
    assert aliased == {True, False}
    assert {(1, True, True, True), (0, True, True, False), (0, True, False, True), (0, False, True, True)} <= phased


# ------------------------------------------------------------------------------------------------------------------ argument checks
X = 0x1000          # a dummy device pointer: none of these calls may get as far as using it


def refused(rc, what):
    assert rc == MH_ERR_INVALID, (what, rc)
    assert lib().mh_last_error(), what


def forward(d, B=2, L=64, ws=X, nbytes=None, x=X, emb_t=X, out=X):
    nbytes = lib().mh_denoiser_workspace_bytes(C.byref(d), B, L) if nbytes is None else nbytes
    return lib().mh_denoiser_forward(C.byref(d) if d is not None else None, x, emb_t, None, out, B, L, ws, nbytes, None)


BAD_MODELS = [
    ("unknown dtype", dict(dtype=7)), ("H not a multiple of 64", dict(H=96, nh=3)), ("H too large", dict(H=4096, nh=64)), ("H zero", dict(H=0)),
    ("F not a multiple of 64", dict(F=1000)), ("F zero", dict(F=0)), ("heads do not divide", dict(nh=7)), ("no heads", dict(nh=0)),
    ("E_pad not a multiple of 64", dict(E_pad=136)), ("E_pad below E", dict(E=132, E_pad=128)), ("Tt_pad below Tt", dict(Tt=80)),
    ("Tt_pad not a multiple of 64", dict(Tt_pad=96)), ("T4_pad below 4 Tt", dict(T4_pad=64)), ("T4_pad not a multiple of 64", dict(T4_pad=160)),
    ("has_proj with E == H", dict(E=512, E_pad=512)), ("no proj with E != H", dict(has_proj=0)),
    ("panel with E % 4", dict(E=126)), ("panel with head dim 16", dict(nh=32)), ("panel in fp32", dict(dtype=MH_F32)),
    ("null layer table", dict(layers=None)),
    ("split with panel", dict(dtype=MH_BF16X3)), ("split with head dim 128", dict(dtype=MH_F16X3, panel=0, nh=4)),
]


@pytest.mark.parametrize("what,fields", BAD_MODELS, ids=[w for w, _ in BAD_MODELS])
def test_check_model_refuses(what, fields):
    d, keep = desc()
    for k, v in fields.items():
        if k == "layers":
            d.layers = C.cast(None, C.POINTER(_lib.LayerWeights))
        else:
            setattr(d, k, v)
    refused(lib().mh_denoiser_forward(C.byref(d), X, X, None, X, 2, 64, X, 1 << 40, None), what)
    refused(lib().mh_time_embed(C.byref(d), X, X, 2, X, 1 << 40, None), what + " (time_embed)")


def test_null_layer_table_is_fine_without_layers():
    """check_model lets a null table pass when nL == 0; the next check (the workspace) then refuses"""
    d, keep = desc(nL=0)
    d.layers = C.cast(None, C.POINTER(_lib.LayerWeights))
    refused(forward(d, ws=None), "null workspace")
    assert b"workspace" in lib().mh_last_error()


def test_forward_refuses_bad_shapes_and_workspaces():
    d, keep = desc(L=64)                      # L_max = 64 + ec.L_EXTRA
    refused(forward(None, nbytes=1 << 20), "null descriptor")
    refused(forward(d, L=20, nbytes=1 << 30), "L % 8 != 0")
    refused(forward(d, L=d.L_max + 8, nbytes=1 << 30), "L > L_max")
    refused(forward(d, B=0, nbytes=1 << 30), "B == 0")
    refused(forward(d, B=-2, nbytes=1 << 30), "B < 0")
    refused(forward(d, L=0, nbytes=1 << 30), "L == 0")
    refused(forward(d, ws=None), "null workspace")
    need = lib().mh_denoiser_workspace_bytes(C.byref(d), 2, 64)
    refused(forward(d, nbytes=need - 1), "workspace one byte short")
    assert b"too small" in lib().mh_last_error()
    refused(forward(d, nbytes=0), "empty workspace")
    for null in ("x", "emb_t", "out"):
        refused(forward(d, **{null: None}), "null " + null)


def test_time_embed_refuses():
    d, keep = desc()
    hid, need = ec.time_layout(d, 5)
    refused(lib().mh_time_embed(C.byref(d), X, X, 5, X, need - 1, None), "time_embed workspace one byte short")
    refused(lib().mh_time_embed(C.byref(d), X, X, 5, None, need, None), "time_embed null workspace")
    refused(lib().mh_time_embed(C.byref(d), X, X, 0, X, need, None), "time_embed B == 0")
    refused(lib().mh_time_embed(C.byref(d), None, X, 5, X, need, None), "time_embed null t")


def phased_calls(d, ld=128, B=2, L=64):
    n = 1 << 30
    return [("head", lib().mh_denoiser_head(C.byref(d), X, X, None, X, ld, B, L, X, n, None)),
            ("layers", lib().mh_denoiser_layers(C.byref(d), X, ld, X, ld, B, L, X, n, None)),
            ("tail", lib().mh_denoiser_tail(C.byref(d), X, ld, X, B, L, X, n, None))]


def test_phased_entry_points_refuse():
    models = [("row-major bf16", desc(panel=False)), ("fp32", desc(MH_F32)), ("split", desc(MH_BF16X3, H=128, nh=4, F=256, E=32)),
              ("no projections", desc(E=64, H=64, nh=2, F=128)), ("no layers", desc(nL=0))]
    for what, (d, keep) in models:
        assert lib().mh_denoiser_phases_supported(C.byref(d)) == 0, what
        for name, rc in phased_calls(d):
            refused(rc, "%s on a %s model" % (name, what))
    d, keep = desc()
    assert lib().mh_denoiser_phases_supported(C.byref(d)) == 1 and lib().mh_denoiser_phases_supported(None) == 0
    for name, rc in phased_calls(d, ld=127):
        refused(rc, "%s with ld < B L" % name)
    refused(lib().mh_denoiser_layers(C.byref(d), X, 128, X, 127, 2, 64, X, 1 << 30, None), "layers with ld_out < B L")
    refused(lib().mh_denoiser_head(C.byref(d), X, X, None, None, 128, 2, 64, X, 1 << 30, None), "head with null rows")
    # ... and with good arguments they still go through denoiser_run's own checks
    refused(lib().mh_denoiser_head(C.byref(d), X, X, None, X, 128, 2, 64, X, 16, None), "head with a short workspace")
    refused(lib().mh_denoiser_layers(C.byref(d), X, 128, X, 128, 2, 64, None, 1 << 30, None), "layers with a null workspace")
    refused(lib().mh_denoiser_tail(C.byref(d), X, 160, X, 2, 80, X, 16, None), "tail with a short workspace")


def test_forward_round_and_sqnorm_refuse_unserved_models():
    d, keep = desc()
    assert lib().mh_denoiser_rounds_in_forward(C.byref(d), 729) == 1 and lib().mh_denoiser_gives_sqnorm(C.byref(d)) == 1
    for V in (97, 640, 769):
        assert lib().mh_denoiser_rounds_in_forward(C.byref(d), V) == 0
        refused(lib().mh_denoiser_forward_round(C.byref(d), X, X, None, X, X, V, X, None, 2, 64, X, 1 << 30, None), "forward_round V=%d" % V)
    refused(lib().mh_denoiser_forward_round(C.byref(d), X, X, None, X, X, 729, None, None, 2, 64, X, 1 << 30, None), "forward_round null idx")
    refused(lib().mh_denoiser_forward_round(C.byref(d), X, X, None, X, None, 729, X, None, 2, 64, X, 1 << 30, None), "forward_round null table")
    refused(lib().mh_denoiser_forward_sqnorm(C.byref(d), X, X, None, X, None, 2, 64, X, 1 << 30, None), "forward_sqnorm null sqnorm")
    for what, (m, keep2) in (("E_pad 192", desc(E=132)), ("row-major", desc(panel=False)), ("fp32", desc(MH_F32)), ("no projections", desc(E=64, H=64, nh=2, F=128)),
                             ("d_model 128", desc(E=32, H=128, nh=4, F=256))):
        assert lib().mh_denoiser_gives_sqnorm(C.byref(m)) == 0, what
        refused(lib().mh_denoiser_forward_sqnorm(C.byref(m), X, X, None, X, X, 2, 64, X, 1 << 30, None), "forward_sqnorm on " + what)
        refused(lib().mh_denoiser_forward_round(C.byref(m), X, X, None, X, X, 729, X, None, 2, 64, X, 1 << 30, None), "forward_round on " + what)
    assert lib().mh_denoiser_gives_sqnorm(None) == 0 and lib().mh_denoiser_rounds_in_forward(None, 729) == 0
