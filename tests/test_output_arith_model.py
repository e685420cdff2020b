"""CPU: the model of blend, output levels and the flow views (tests/output_arith_model.py) against the C oracle over the whole input domain,
and the proof that the committed inputs bite.

  levels and blend  model == oracle.warp_frames at zero flow and oracle.copy_frame, bit for bit, on every ramp phase, every entry of LEVELS
                    and every blend scalar, with the correctly rounded reciprocal on both sides; again for 0 / 180 with the reciprocal
                    1 ulp low on both sides (what the device gives for that span)
  flow views        the oracle's mode 4 == the model; the oracle's mode 3 lies in the model's accepted set for every vector, channel, gain
                    and element type
  condition         at the committed DELTA at most 3 % of the flow domain's vectors have more than one accepted value
  flawed variants   each of the listed wrong variants changes at least one output element of the committed inputs (flow view: leaves
                    the accepted set)
tests/test_output_arith_gpu.py runs the same inputs on the device."""
import os
import sys
from concurrent.futures import ThreadPoolExecutor
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import output_arith_model as M  # noqa: E402
import warp_variant_model as V  # noqa: E402

_pool = ThreadPoolExecutor(8)      # (the oracle is plain C behind ctypes)
_cache = {}


@pytest.fixture(autouse=True)
def _default_flavour():
    from oracle import oracle
    try:
        yield
    finally:
        oracle.set_flavour(1, 1, None)


def ramps(hdr):
    """[(ramp, reversed ramp)] per phase, computed once and never modified."""
    if ("ramps", hdr) not in _cache:
        _cache["ramps", hdr] = [(f, M.partner_frame(f, hdr)) for f in (M.ramp_frame(hdr, p) for p in range(M.PHASES[hdr]))]
    return _cache["ramps", hdr]


def blended(hdr, phase, t, flavour=1):
    k = ("blend", hdr, phase, t, flavour)
    if k not in _cache:
        _cache[k] = M.blend_zero_flow(*ramps(hdr)[phase], t, flavour)
    return _cache[k]


def geom(hdr, max_res=128):
    from oracle import oracle
    return oracle.make_geom(hdr, M.H, M.W, 0, 0, max_res)


def zero_flow(g):
    return np.zeros((2, g.lh, g.lw), np.int16)


def test_the_fused_multiply_add_is_one_rounding():
    """Against exact rational arithmetic, with addends that cancel the product to a few bits (where a double rounding would show)."""
    rng = np.random.default_rng(1)
    a = rng.standard_normal(4000).astype(np.float32) * np.float32(1000)
    b = rng.standard_normal(4000).astype(np.float32)
    c = np.concatenate([(-(a[:2000].astype(np.float64) * b[:2000])).astype(np.float32) * np.float32(1 + 2.0 ** -12), rng.standard_normal(2000).astype(np.float32)])
    got = M.fma(a, b, c)
    for x, y, z, r in zip(a, b, c, got):
        exact = Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))
        w = np.float32(float(exact))
        near = [np.nextafter(w, np.float32(-np.inf)), w, np.nextafter(w, np.float32(np.inf))]
        best = min(near, key=lambda q: (abs(Fraction(float(q)) - exact), int(np.float32(q).view(np.uint32)) & 1))
        assert best == r, (x, y, z, r, best)


def test_the_inputs_are_what_the_model_says():
    assert len(M.LEVELS) == 36 and len(set(M.LEVELS)) == 36 and set(M.SCENE_LEVELS) <= set(M.LEVELS)
    for bk, wh in M.LEVELS[12:]:
        assert 0 <= bk <= 64 and 128 <= wh <= 255 and (bk * 4).is_integer() and (wh * 4).is_integer()
    assert all(wh != bk and wh != 0 for bk, wh in M.LEVELS)                    # "sane": warp_variant_model.warp_fast_shape keeps the fast kernel
    assert M.T[-1] < 1.0 and np.float32(M.T[-1]) == np.nextafter(np.float32(1), np.float32(0))
    ym, cm = M.interior_masks(M.H, M.W)
    for hdr in (0, 1):
        want = set(range(M.code_max(hdr) + 1))
        got = [set(), set(), set()]
        for f, p in ramps(hdr):
            y, c = M.planes(f)
            got[0] |= set(y[ym].tolist())
            got[1] |= set(c[:, 0::2][cm[:, 0::2]].tolist())
            got[2] |= set(c[:, 1::2][cm[:, 1::2]].tolist())
            assert np.array_equal(p.astype(np.int64) + f, np.full(f.shape, M.code_max(hdr)))
        assert got == [want] * 3, hdr
    for rs in (1, 3):
        g = M.FLOW_GEOMS[rs]
        case = V.Case("x", 0, M.H, M.W, 0, 0, g.max_res, 1, (1,), (3,), (0,), (0,), (0.0, 255.0), ("uniform:0:0",), (0.0,), "single1")
        vg = V.geometry(case)
        assert (vg.rs, vg.lw, vg.lh) == (g.rs, g.lw, g.lh)
        d = max(vg.lw, vg.lh)
        ws0 = d if d & (d - 1) == 0 else 1 << d.bit_length()
        assert M.chain_reach(g) == (V.ilog2(ws0) + 1) * 64 + 8                  # warp_variant_model.phase_layout's reach
        v = M.flow_domain(rs).astype(np.int64)
        assert len(np.unique(v, axis=0)) == len(v)
        have = set(map(tuple, v.tolist()))
        assert all((x, y) in have for x in range(-48, 49) for y in range(-48, 49))
        for m in (100, 300, M.chain_reach(g)):
            assert sum(1 for x, y in have if abs(np.hypot(x, y) - m) <= 0.75) >= 352, (rs, m)
        assert np.abs(v).sum(1).max() >= 64 > np.abs(v).sum(1).min() == 0        # mode 4 on both sides of its saturation
        # every vector is seen by luma, U and V of some field
        hit = np.zeros((3, len(v)), bool)
        for field, idx in M.flow_fields(rs):
            assert field.shape == (2, g.lh, g.lw) and np.array_equal(field[0], v[idx, 0]) and np.array_equal(field[1], v[idx, 1])
            which, channel = M.seen(rs, idx)
            for ch in range(3):
                hit[ch, np.unique(which[channel == ch])] = True
        assert hit.all(), rs


@pytest.mark.parametrize("hdr", [0, 1], ids=["u8", "u16"])
def test_levels_and_blend_equal_the_oracle(hdr):
    from oracle import oracle
    g = geom(hdr)
    flow = zero_flow(g)
    y180, w180 = M.rcp_inputs(0.0, 180.0, hdr)
    low = {float(y180): float(M.rcp_one_low(y180)), float(w180): float(M.rcp_one_low(w180))}
    for (bk, wh), rcp in [(lv, None) for lv in M.LEVELS] + [((0.0, 180.0), low)]:
        oracle.set_flavour(1, 1, rcp)
        jobs = [(p, t) for p in range(M.PHASES[hdr]) for t in M.T]
        want = list(_pool.map(lambda j: oracle.warp_frames(*ramps(hdr)[j[0]], flow, g, np.float32(j[1]), 2, bk, wh), jobs))
        for (p, t), w in zip(jobs, want):
            got = M.levels_frame(blended(hdr, p, t), hdr, bk, wh, rcp)
            assert np.array_equal(got.reshape(-1), w), (hdr, bk, wh, p, t, int((got.reshape(-1) != w).sum()))
        for p in range(M.PHASES[hdr]):
            got = M.copy_frame(ramps(hdr)[p][0], hdr, bk, wh, rcp)
            assert np.array_equal(got.reshape(-1), oracle.copy_frame(ramps(hdr)[p][0], g, bk, wh)), (hdr, bk, wh, p, "copy")


def test_the_one_low_reciprocal_at_white_180_shows():
    """The correctly rounded reciprocal is a flawed variant at white 180: the inputs tell it from the device's (1 ulp low)."""
    for hdr in (0, 1):
        y180, w180 = M.rcp_inputs(0.0, 180.0, hdr)
        assert y180 == w180 == (46080 if hdr else 180)
        low = {float(y180): float(M.rcp_one_low(y180))}
        a = [M.copy_frame(f, hdr, 0.0, 180.0, low) for f, _ in ramps(hdr)]
        b = [M.copy_frame(f, hdr, 0.0, 180.0, None) for f, _ in ramps(hdr)]
        y = [(p[:M.H] != q[:M.H]).any() for p, q in zip(a, b)]
        c = [(p[M.H:] != q[M.H:]).any() for p, q in zip(a, b)]
        assert any(y) and any(c), (hdr, y, c)


def _levels_flaw_shows(flaw=None, flavour=1):
    """Some output element of the committed inputs differs between the model and the flawed variant: (found, where)."""
    for hdr in (0, 1):
        for p in range(M.PHASES[hdr]):
            for t in M.T:
                if flavour != 1:
                    if any(not np.array_equal(a, b) for a, b in zip(blended(hdr, p, t), blended(hdr, p, t, flavour))):
                        return True, (hdr, p, t)
                    continue
                for bk, wh in M.LEVELS:
                    if not np.array_equal(M.levels_frame(blended(hdr, p, t), hdr, bk, wh), M.levels_frame(blended(hdr, p, t), hdr, bk, wh, None, flaw)):
                        return True, (hdr, p, t, bk, wh)
    return False, None


@pytest.mark.parametrize("flaw", ["round_to_nearest", "negative_wraps", "above_max_wraps", "chroma_by_span"])
def test_flawed_levels_are_told_from_the_model(flaw):
    assert _levels_flaw_shows(flaw)[0], flaw


@pytest.mark.parametrize("hdr", [0, 1], ids=["u8", "u16"])
@pytest.mark.parametrize("flaw", ["round_to_nearest", "negative_wraps", "above_max_wraps", "chroma_by_span"])
def test_flawed_levels_show_in_each_element_type(flaw, hdr):
    """... and in each element type on its own, at 16 / 235 of the copy path already (what every body is run at on the device)."""
    hit = False
    for f, _ in ramps(hdr):
        for bk, wh in M.LEVELS:
            hit = hit or not np.array_equal(M.copy_frame(f, hdr, bk, wh), M.copy_frame(f, hdr, bk, wh, None, flaw))
    assert hit, (flaw, hdr)


@pytest.mark.parametrize("flavour", [2, 0])
def test_flawed_blends_are_told_from_the_model(flavour):
    """fma(b, t, a * (1 - t)) and the unfused blend: the model's variant equals the oracle's flavour, and the inputs tell it from flavour 1."""
    from oracle import oracle
    found, where = _levels_flaw_shows(flavour=flavour)
    assert found, flavour
    hdr, p, t = where
    g = geom(hdr)
    oracle.set_flavour(flavour, 1, None)
    want = oracle.warp_frames(*ramps(hdr)[p], zero_flow(g), g, np.float32(t), 2, 0.0, 255.0)
    assert np.array_equal(M.levels_frame(blended(hdr, p, t, flavour), hdr, 0.0, 255.0).reshape(-1), want)
    assert not np.array_equal(M.levels_frame(blended(hdr, p, t, 1), hdr, 0.0, 255.0).reshape(-1), want)


def test_negative_and_above_maximum_levels_values_exist_on_16_bit_frames():
    """Where the packed 16-bit body leans on the conversion instructions: 16 / 235 and 200 / 100 hold elements below 0 and above 65535."""
    for bk, wh in ((16.0, 235.0), (200.0, 100.0)):
        for cz in (0, 1):
            v = np.concatenate([M.levels_values(f, 1, bk, wh, cz).reshape(-1) for f, _ in ramps(1)])
            assert (v < 0).any() and (v > 65535).any(), (bk, wh, cz)


# ---- flow views ----
def oracle_views(rs, hdr):
    """(mode 3, mode 4) of every field through the oracle: constant frames, t = 0, levels 0 / 255."""
    from oracle import oracle
    if ("views", rs, hdr) not in _cache:
        g = geom(hdr, M.FLOW_GEOMS[rs].max_res)
        assert (g.rs, g.lw, g.lh) == M.FLOW_GEOMS[rs][:3]
        f = M.const_frame(hdr)
        jobs = [(field, mode) for field, _ in M.flow_fields(rs) for mode in (3, 4)]
        res = list(_pool.map(lambda j: oracle.warp_frames(f, f, j[0], g, np.float32(0.0), j[1], 0.0, 255.0), jobs))
        _cache["views", rs, hdr] = (res[0::2], res[1::2])
    return _cache["views", rs, hdr]


def outside(rs, hdr, frames3, tables=None):
    """Number of elements of the mode 3 frames (one per field) outside the accepted sets."""
    m3, _ = tables or M.view_tables(rs, hdr)
    n = 0
    for (_, idx), got in zip(M.flow_fields(rs), frames3):
        which, channel = M.seen(rs, idx)
        acc = m3[:, channel, which]
        n += int((~(acc == got.reshape(which.shape)[None]).any(0)).sum())
    return n


@pytest.mark.parametrize("hdr", [0, 1], ids=["u8", "u16"])
@pytest.mark.parametrize("rs", [1, 3], ids=["rs1-gain4", "rs3-gain1"])
def test_flow_views_of_the_oracle_lie_in_the_model(rs, hdr):
    from oracle import oracle
    oracle.set_flavour(1, 1, None)
    got3, got4 = oracle_views(rs, hdr)
    _, m4 = M.view_tables(rs, hdr)
    for (_, idx), g4 in zip(M.flow_fields(rs), got4):
        which, channel = M.seen(rs, idx)
        assert np.array_equal(g4.reshape(which.shape), m4[channel, which]), (rs, hdr, "mode 4")
    assert outside(rs, hdr, got3) == 0


def multi_valued_share(rs):
    v = M.flow_domain(rs).astype(np.int64)
    multi = np.zeros(len(v), bool)
    for hdr in (0, 1):
        for ch in range(3):
            multi |= ~M.single_valued(M.flow_view(-v[:, 0], -v[:, 1], M.CONST[hdr], ch, M.gain_of(rs), hdr))
    return float(multi.mean())


def test_at_most_3_percent_of_the_vectors_have_two_accepted_values():
    """A CONDITION on the committed DELTA, not a measurement: at least 97 % of the domain is held exactly (before the levels, in some
    channel of some element type: the widest count).  And DELTA is what it is said to be: eight times the float32 chain's deviation."""
    for rs in (1, 3):
        share = multi_valued_share(rs)
        print(f"rs {rs}: {100 * share:.3f} % of {len(M.flow_domain(rs))} vectors have two accepted values at DELTA = {M.DELTA:.4e}")
        assert share <= 0.03, (rs, share)
        v = M.flow_domain(rs).astype(np.int64)
        dev = M.hue_deviation(v[:, 0], v[:, 1])
        print(f"rs {rs}: float32 hue chain deviates by {dev:.4e}")
        assert M.DELTA == 8 * 1.8653e-4 and dev <= M.DELTA / 4, (rs, dev)       # (a factor of two for another libm's float32 arctan2)


@pytest.mark.parametrize("flaw,gain", [("sextant_low_at_boundary", None), ("green_by_magnitude", None), ("to_byte_unclamped", None), (None, 4)],
                         ids=["sextant", "green-weight", "to_byte-unclamped", "gain4-at-rs3"])
def test_flawed_flow_views_leave_the_accepted_sets(flaw, gain):
    """The flawed variant's own value (at u) is outside the model's accepted set for some vector, channel and element type."""
    hit = 0
    for rs in ((3,) if gain else (1, 3)):
        for hdr in (0, 1):
            good, _ = M.view_tables(rs, hdr)
            bad, _ = M.view_tables(rs, hdr, gain=gain, flaw=flaw)
            hit += int((~(good == bad[1][None]).any(0)).sum())
    assert hit > 0, (flaw, gain)
