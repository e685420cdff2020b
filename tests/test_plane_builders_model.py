"""CPU: the matrix of tests/test_plane_builders_gpu.py (tests/plane_builder_model.py) reaches every phase-plane builder, and its content
tells a flawed builder from the layout model.  Conditions on the INPUT and on the restated decision, not measurements of the product.

  * the layout restated in tests/phase_plane_model.py is the compiled header's for every case, and the shapes are what their names say;
  * plane_builder_model.builder equals hf_launch_plan.h plane_fast_geometry (through tests/launch_plan_probe.cpp) for every case and over
    W 16 .. 2100, rs 0 .. 4, both element types and four row pitches at H = 64; plane_emission_geometry is that answer at rs 3 .. 4;
  * REACHED below names, per builder instantiation and per reason for the generic kernel, the case that reaches it;
  * the two deferred cases are the batches of fewest frame bytes that defer, and their warp launch is planned with the plane of every
    member but the misaligned one;
  * for every case, a builder with one of six flaws (plane_builder_model.wrong_plane) writes a plane that differs from the model's.

What the suite reached before this matrix, from the same model (python tests/test_plane_builders_model.py prints it;
test_what_the_older_suite_reaches keeps it true):
  tests/test_update_host_path_gpu.py   180 x 320 SDR: rs 0, lw 320, mx 588 > lw: generic.  360 x 640 HDR: fast.u16.rs1.  180 x 322: generic.
  tests/test_random_gpu.py             4 of 64 seeds reach the fast kernel (48, 58, 60 at rs 0, 51 at rs 2), none at rs 1 or 3
  mx == lw on the fast kernel: nowhere.  Both compare a plane with a twin's or judge it by the flow, none with the model."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import launch_plan_probe  # noqa: E402
import phase_plane_model as P  # noqa: E402
import plane_builder_model as B  # noqa: E402

ALL = B.CASES + B.DEFERRED_CASES

# builder instantiation or generic reason -> the case that reaches it (lone context: .st, batch of three: .nt)
REACHED = {
    "fast.u8.rs0.st": "fast-u8-rs0", "fast.u8.rs0.nt": "fast-u8-rs0", "fast.u16.rs0.st": "fast-u16-rs0", "fast.u16.rs0.nt": "fast-u16-rs0",
    "fast.u8.rs1.st": "fast-u8-rs1", "fast.u8.rs1.nt": "fast-u8-rs1", "fast.u16.rs1.st": "fast-u16-rs1", "fast.u16.rs1.nt": "fast-u16-rs1",
    "fast.u8.rs2.st": "fast-u8-rs2", "fast.u8.rs2.nt": "fast-u8-rs2", "fast.u16.rs2.st": "fast-u16-rs2", "fast.u16.rs2.nt": "fast-u16-rs2",
    "fast.u8.rs3.st": "fast-u8-rs3", "fast.u8.rs3.nt": "fast-u8-rs3", "fast.u16.rs3.st": "fast-u16-rs3", "fast.u16.rs3.nt": "fast-u16-rs3",
    "warp.u16.rs3": "deferred-u16-rs3", "warp.u8.rs4": "deferred-u8-rs4",
    B.RAGGED: "ragged-u8-rs3", B.LW4: "lw4-u16-rs1", B.MARGIN: "edge-u16-rs1-mx-gt-lw", B.PITCH: "pitch-u8-rs2", B.BASE: "base8-u16-rs2",
    "one misaligned member": "middle8-u8-rs1", "mx == lw": "edge-u8-rs1-mx-eq-lw", "mx < lw / 2": "fast-u8-rs3-w2048",
    "padded rows": "padded-u16-rs1", "odd chroma rows": "oddrows-u16-rs1", "narrower than a task group": "narrow-u8-rs0",
}


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    return launch_plan_probe.load(tmp_path_factory.mktemp("launch_plan_probe"))


def iters(c):
    return P.max_iterations(*B.geometry(c)[1:3])


# ------------------------------------------------------------------------------------------------
# layout and shapes
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", ALL, ids=lambda c: c.name)
def test_layout_model_equals_the_header(probe, c):
    from oracle import oracle
    rs, lw, lh, L = B.geometry(c)
    g = oracle.make_geom(c.hdr, c.H, c.W, c.in_stride, 0, c.max_res)
    assert (g.rs, g.lw, g.lh, g.in_stride) == (rs, lw, lh, B.stride(c))
    assert iters(c) == oracle.lib().hfo_initial_window(lw, lh).bit_length() - 1
    want = probe.phase_layout(B.g_tuple(c), iters(c))
    assert tuple(L) == tuple(want), (c.name, L, want)
    assert want.lwp >= lw + 2 * want.mx + 4 and c.W % 2 == 0 and c.H % 2 == 0


def test_shapes_are_what_the_matrix_says():
    names = [c.name for c in ALL]
    assert len(set(names)) == len(names)
    at = lambda name: (lambda rs, lw, lh, L: (rs, lw, L.mx))(*B.geometry(B.case(name)))
    for e in ("u8", "u16"):
        assert [at("fast-%s-rs%d" % (e, rs)) for rs in range(4)] == [(0, 1024, 652), (1, 512, 296), (2, 256, 132), (3, 128, 60)]
        assert at("fast-%s-rs3-w2048" % e) == (3, 256, 68)
    assert at("edge-u8-rs1-mx-eq-lw") == (1, 296, 296) and at("edge-u16-rs1-mx-gt-lw") == (1, 292, 296)
    assert B.stride(B.case("edge-u16-rs1-mx-gt-lw")) * 2 == 1168
    assert at("narrow-u8-rs0") == (0, 16, 268) and at("narrow-u16-rs1") == (1, 16, 136)
    assert at("lw4-u8-rs0")[:2] == (0, 1026) and at("lw4-u16-rs1")[:2] == (1, 514)
    for c in B.CASES:                                                        # a few dozen rows, kilobytes
        assert c.H <= 70 and (c.H + c.H // 2) * B.stride(c) * (2 if c.hdr else 1) <= 384 << 10, c.name
        assert len(c.offs) == 3 and set(c.offs) <= {0, 8}
    assert at("deferred-u16-rs3")[0] == 3 and at("deferred-u8-rs4")[0] == 4
    for c in B.DEFERRED_CASES:
        assert c.H == B.geometry(c)[2] << B.geometry(c)[0] and 0 < c.odd < c.n


# ------------------------------------------------------------------------------------------------
# the restated decision against the compiled one
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", ALL, ids=lambda c: c.name)
def test_builder_equals_the_compiled_predicate(probe, c):
    fast, emits = probe.plane_fast_geometry(B.g_tuple(c), iters(c))
    assert fast == (not B.geometry_reasons(c)), (c.name, B.geometry_reasons(c))
    rs = B.geometry(c)[0]
    assert emits == (fast and 3 <= rs <= 4 and (c.H * B.stride(c) * (2 if c.hdr else 1)) % 16 == 0), c.name
    if isinstance(c, B.Case):
        for batch in (False, True):
            b = B.builder(c, batch)
            offs = c.offs if batch else c.offs[:1]
            assert (b.kind == "fast") == (fast and not any(o & 15 for o in offs)), (c.name, batch, b)
            assert b.name.endswith(".nt" if batch else ".st") == (b.kind == "fast") and (b.kind == "generic") == bool(b.reasons)
        assert B.builder(c, False, copied=True).kind == ("fast" if fast else "generic")


def test_builder_equals_the_compiled_predicate_over_a_sweep_of_widths(probe):
    n, seen = 0, set()
    for hdr in (0, 1):
        for rs in range(5):
            for pad in (0, 2, 8, 16):
                for W in range(16, 2101, 2):
                    c = B.Case("sweep", hdr, 64, W, 64 >> rs, W + pad if pad else 0)
                    assert B.geometry(c)[0] == rs
                    why = B.geometry_reasons(c)
                    assert probe.plane_fast_geometry(B.g_tuple(c), iters(c))[0] == (not why), (hdr, rs, pad, W, why)
                    seen.update(why)
                    n += not why
    assert n > 1000 and seen == {B.RAGGED, B.LW4, B.MARGIN, B.PITCH}
    for H, rs, why in ((65, 0, [B.ODD_H]), (2048, 5, [B.DEEP])):         # (the remaining two conditions, at a width that meets all others)
        c = B.Case("sweep", 0, H, 2048 << max(rs - 3, 0), H >> rs)
        assert B.geometry_reasons(c) == why and not probe.plane_fast_geometry(B.g_tuple(c), iters(c))[0], (H, rs, B.geometry_reasons(c))


# ------------------------------------------------------------------------------------------------
# what the matrix reaches
# ------------------------------------------------------------------------------------------------
def test_matrix_reaches_every_builder(probe):
    lone = {c.name: B.builder(c, False) for c in B.CASES}
    batch = {c.name: B.builder(c, True) for c in B.CASES}
    # all 16 fast instantiations of rs 0 .. 3, each by the case REACHED names
    got = {b.name for b in list(lone.values()) + list(batch.values()) if b.kind == "fast"}
    assert got == B.FAST_INSTANTIATIONS, sorted(B.FAST_INSTANTIATIONS ^ got)
    for inst in B.FAST_INSTANTIATIONS:
        assert (lone if inst.endswith(".st") else batch)[REACHED[inst]].name == inst, inst
    # the generic kernel for each reason on its own, both element types, rs 0 .. 3 between them
    for why in (B.RAGGED, B.LW4, B.MARGIN, B.PITCH, B.BASE):
        assert lone[REACHED[why]].reasons == (why,) and batch[REACHED[why]].reasons == (why,), why
        for hdr in (0, 1):
            assert any(lone[c.name].reasons == (why,) for c in B.CASES if c.hdr == hdr), (why, hdr)
    assert {B.geometry(c)[0] for c in B.CASES if lone[c.name].kind == "generic"} == {0, 1, 2, 3}
    ragged = B.case(REACHED[B.RAGGED])
    rs, lw = B.geometry(ragged)[:2]
    assert (lw << rs) > ragged.W > ((lw - 1) << rs)                           # the last column's higher phases lie beyond the frame
    for c in B.CASES:
        if B.PITCH in lone[c.name].reasons:
            assert c.in_stride == c.W + (4 if c.hdr else 2), c.name
    # one misaligned member sends the whole batch to the generic kernel, whichever member it is
    c = B.case(REACHED["one misaligned member"])
    assert c.offs == (0, 8, 0) and lone[c.name].kind == "fast" and batch[c.name].reasons == (B.BASE,)
    assert {x.hdr for x in B.CASES if x.offs == (0, 8, 0)} == {0, 1}
    assert any(x.offs[0] == 8 and x.offs[1:] == (0, 0) for x in B.CASES)
    # both margin regimes, and the boundary: mx == lw with the last margin store ending at mx + 2 lw - 1 < lwp
    fast = [c for c in B.CASES if lone[c.name].kind == "fast"]
    regime = lambda c: (lambda rs, lw, lh, L: (2 * L.mx > lw) - (2 * L.mx < lw))(*B.geometry(c))
    for rs in range(3):
        assert regime(B.case("fast-u8-rs%d" % rs)) == 1 and regime(B.case("fast-u16-rs%d" % rs)) == 1
    assert regime(B.case(REACHED["mx < lw / 2"])) == -1 and {c.hdr for c in fast if regime(c) == -1} == {0, 1}
    c = B.case(REACHED["mx == lw"])
    rs, lw, lh, L = B.geometry(c)
    assert L.mx == lw and lone[c.name].kind == "fast" and L.mx + 2 * lw - 1 < L.lwp
    n = B.case(REACHED[B.MARGIN])
    assert B.geometry(n)[1] == B.geometry(n)[3].mx - 4 and (n.W, n.H, n.max_res) == (c.W - 8, c.H, c.max_res)
    # rows of padding behind a fast shape, an odd number of chroma rows, grids narrower than one group of tasks and than mx by far
    c = B.case(REACHED["padded rows"])
    assert c.in_stride == c.W + 16 and lone[c.name].kind == "fast" and {x.hdr for x in fast if x.in_stride == x.W + 16} == {0, 1}
    c = B.case(REACHED["odd chroma rows"])
    assert (c.H // 2) % 2 == 1 and lone[c.name].kind == "fast" and {x.hdr for x in fast if (x.H // 2) % 2} == {0, 1}
    for c in (B.case("narrow-u8-rs0"), B.case("narrow-u16-rs1")):
        rs, lw, lh, L = B.geometry(c)
        assert lone[c.name].reasons == (B.MARGIN,) and lw < 128 * 4 and L.mx > 8 * lw and c.W < L.mx << rs
    assert {k: v for k, v in REACHED.items() if v not in [c.name for c in ALL]} == {}


@pytest.mark.parametrize("c", B.DEFERRED_CASES, ids=lambda c: c.name)
def test_deferred_cases_are_the_smallest_that_defer(probe, c):
    """... and their period warp is the staged launch with the plane of every member but the one at base + 8 bytes."""
    rs = B.geometry(c)[0]
    cost, n, W, H = B.smallest_deferring(probe, c.hdr, rs)
    assert (n, W, H) == (c.n, c.W, c.H), (c.name, cost, n, W, H)
    g = B.g_tuple(c)
    assert probe.can_build_planes(g, iters(c), c.n) and not probe.can_build_planes(g, iters(c), c.n - 1)
    assert not any(probe.can_build_planes(B.g_tuple(x), iters(x), 3) for x in B.CASES)       # no small case defers
    ms = [launch_plan_probe.member(2, (0.25, 0.75), src_off=0, wants_plane=True, src21_off=8 if m == c.odd else 0) for m in range(c.n)]
    launch, = probe.plan_warp(g, 2, ms, have_pl=True, max_iters=iters(c))
    assert launch.family == launch_plan_probe.STAGED and launch.count == c.n and launch.plane_blocks > 0
    assert launch.planes == ((1 << c.n) - 1) & ~(1 << c.odd)
    assert REACHED["warp.%s.rs%d" % ("u16" if c.hdr else "u8", rs)] == c.name
    assert {"warp.%s.rs%d" % ("u16" if x.hdr else "u8", B.geometry(x)[0]) for x in B.DEFERRED_CASES} == B.DEFERRED_INSTANTIATIONS


# ------------------------------------------------------------------------------------------------
# the cases discriminate
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", ALL, ids=lambda c: c.name)
def test_a_flawed_builder_shows(c):
    rs, lw, lh, L = B.geometry(c)
    f = B.frames(c, 0, 1)[0]
    full = 65535 if c.hdr else 255                                               # full-range noise, P010 low bytes included
    assert int(f.max()) - int(f.min()) >= full * 9 // 10 and len(np.unique(f & 0xFF)) >= min(f.size // 4, 250)
    want = P.plane(f, bool(c.hdr), c.H, c.W, c.in_stride, L, lw)
    assert np.array_equal(B.wrong_plane(f, c, None), want)
    j = np.arange(-L.mx, lw + L.mx)
    margin = (j < 0) | (j >= lw)
    n = 0
    for v in B.VARIANTS:
        if not B.applies(v, c):
            continue
        bad = B.wrong_plane(f, c, v) != want
        assert bad.any(), (c.name, v)
        if v in B.MARGIN_VARIANTS:
            assert bad[:, :, margin].any(), (c.name, v)
        n += 1
    assert n >= 3


# ------------------------------------------------------------------------------------------------
# what the older suite reaches (the figures of this file's docstring)
# ------------------------------------------------------------------------------------------------
def older_suite():
    import test_random_gpu as R
    import test_update_host_path_gpu as U
    host = {k: B.Case(k, hdr, H, W, 270) for k, (hdr, H, W) in (("SDR", U.SDR), ("HDR", U.HDR), ("GENERIC", U.GENERIC), ("UHD", U.UHD))}
    seeds = {}
    for s in range(64):
        k = R._case(s)
        seeds[s] = B.Case("seed%d" % s, k["hdr"], k["H"], k["W"], k["max_res"], k["si"])
    return host, seeds


def test_what_the_older_suite_reaches():
    host, seeds = older_suite()
    assert B.geometry(host["SDR"])[:2] == (0, 320) and B.geometry(host["SDR"])[3].mx == 588
    assert B.builder(host["SDR"], False).reasons == (B.MARGIN,) and B.builder(host["SDR"], True).reasons == (B.MARGIN,)
    assert B.builder(host["HDR"], False).name == "fast.u16.rs1.st" and B.builder(host["GENERIC"], False).kind == "generic"
    fast = {s: B.builder(c, False).name for s, c in seeds.items() if B.builder(c, False).kind == "fast"}
    assert len(fast) == 4 and not any(".rs1." in n or ".rs3." in n for n in fast.values()), fast
    assert not any(B.geometry(c)[1] == B.geometry(c)[3].mx and B.builder(c, False).kind == "fast"                    # mx == lw on the fast kernel: nowhere
                   for c in list(seeds.values()) + list(host.values()))


if __name__ == "__main__":
    host, seeds = older_suite()
    for c in list(host.values()) + list(seeds.values()):
        rs, lw, lh, L = B.geometry(c)
        b = B.builder(c, False)
        print(f"  {c.name:8s} {c.H} x {c.W} {'P010' if c.hdr else 'SDR'} stride {B.stride(c)}: rs {rs} lw {lw} mx {L.mx}  {b.name} {', '.join(b.reasons)}")
