"""CPU: planar 4:2:0 frames at the boundary (HF_FLAG_PLANAR_IN / HF_FLAG_PLANAR_OUT, include/hopperflow.h) -- the flags, the .y4m
reader / writer modes that move planar frames unconverted, --pix-fmt, and the strided reference the GPU tests hold the device to."""
import io
import os
import re

import numpy as np
import pytest

from hopperrender_amd import capi, cli, y4m

import planar_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_flags_equal_capi():
    src = open(os.path.join(ROOT, "include", "hopperflow.h")).read()
    flags = {m.group(1): int(m.group(2), 16) for m in re.finditer(r"#define (HF_FLAG_\w+) (0x[0-9a-fA-F]+)", src)}
    assert flags["HF_FLAG_PLANAR_IN"] == capi.HF_FLAG_PLANAR_IN == 0x8000
    assert flags["HF_FLAG_PLANAR_OUT"] == capi.HF_FLAG_PLANAR_OUT == 0x10000
    others = [v for k, v in flags.items() if not k.startswith("HF_FLAG_PLANAR")]
    assert not ({0x8000, 0x10000} & set(others)), "the planar flags must not collide with another flag"
    assert not ({0x10, 0x20, 0x100, 0x400} & {0x8000, 0x10000})


def _stream(H, W, hdr, n, seed=3):
    rng = np.random.default_rng(seed)
    dt = "<u2" if hdr else "u1"
    frames = [rng.integers(0, 1024 if hdr else 256, H * W * 3 // 2).astype(dt) for _ in range(n)]
    head = f"YUV4MPEG2 W{W} H{H} F24000:1001 Ip A1:1 C{'420p10 XYSCSS=420P10' if hdr else '420jpeg'}\n".encode()
    return head, frames, head + b"".join(b"FRAME\n" + f.tobytes() for f in frames)


@pytest.mark.parametrize("hdr", [False, True])
def test_y4m_planar_modes_round_trip_the_file_bytes(hdr):
    H, W = 6, 10
    head, frames, blob = _stream(H, W, hdr, 3)
    r = y4m.Y4MReader(io.BytesIO(blob), planar=True)
    got = list(r)
    assert len(got) == 3 and all((g == f).all() for g, f in zip(got, frames))
    r2 = y4m.Y4MReader(io.BytesIO(blob))
    for f in frames:
        assert (r2.read_planar() == f).all()
    assert r2.read_planar() is None
    out = io.BytesIO()
    w = y4m.Y4MWriter(out, W, H, 24000, 1001, hdr, r.extra)
    for f in got:
        w.write_planar(f)
    assert out.getvalue() == blob
    # the NV12 / P010 path of the same stream is unchanged: its frames are the planar ones re-laid
    for f, nv in zip(frames, y4m.Y4MReader(io.BytesIO(blob))):
        yy, uu, vv = planar_ref.planar_planes(f, H, W, W)
        assert (nv == y4m.planar_to_semiplanar(yy, uu, vv, hdr)).all()


def test_y4m_planar_reader_stops_at_a_partial_frame():
    head, frames, blob = _stream(4, 6, False, 2)
    assert len(list(y4m.Y4MReader(io.BytesIO(blob[:-3]), planar=True))) == 1


@pytest.mark.parametrize("fmt,hdr", [("yuv420p", False), ("yuv420p10le", True), ("nv12", False), ("p010", True)])
def test_pix_fmt_parsing(fmt, hdr):
    _, a = cli.parse_args(["in.yuv", "out.yuv", "--width", "64", "--height", "32", "--pix-fmt", fmt])
    assert a.hdr == hdr and a.pix_fmt == fmt
    planar = fmt.startswith("yuv")
    assert cli._planar_flags(a) == ((capi.HF_FLAG_PLANAR_IN | capi.HF_FLAG_PLANAR_OUT) if planar else 0)


def test_pix_fmt_defaults_and_y4m_sides():
    _, a = cli.parse_args(["in.nv12", "out.nv12", "--width", "64", "--height", "32"])
    assert a.pix_fmt == "nv12" and not a.hdr and cli._planar_flags(a) == 0
    _, a = cli.parse_args(["in.p010", "out.p010", "--width", "64", "--height", "32", "--hdr"])
    assert a.pix_fmt == "p010" and a.hdr
    _, a = cli.parse_args(["in.y4m", "out.nv12"])
    assert cli._planar_flags(a) == capi.HF_FLAG_PLANAR_IN
    _, a = cli.parse_args(["in.nv12", "out.Y4M", "--width", "64", "--height", "32"])
    assert cli._planar_flags(a) == capi.HF_FLAG_PLANAR_OUT
    with pytest.raises(SystemExit):
        cli.parse_args(["in.yuv", "out.yuv", "--width", "64", "--height", "32", "--pix-fmt", "yuv420p", "--hdr"])


@pytest.mark.parametrize("hdr", [False, True])
def test_strided_reference_agrees_with_y4m(hdr):
    H, W = 8, 12
    rng = np.random.default_rng(7)
    hi = 1024 if hdr else 256
    dt = np.uint16 if hdr else np.uint8
    y, u, v = rng.integers(0, hi, (H, W)).astype(dt), rng.integers(0, hi, (H // 2, W // 2)).astype(dt), rng.integers(0, hi, (H // 2, W // 2)).astype(dt)
    p = np.concatenate([y.reshape(-1), u.reshape(-1), v.reshape(-1)])
    nv = planar_ref.planar_to_semiplanar(p, H, W, W, hdr)
    assert (nv == y4m.planar_to_semiplanar(y, u, v, hdr)).all()
    back = planar_ref.semiplanar_to_planar(nv, H, W, W, hdr)
    assert (back == p).all()
    y2, u2, v2 = y4m.semiplanar_to_planar(nv, H, W, hdr)
    assert (back == np.concatenate([y2.reshape(-1), u2.reshape(-1), v2.reshape(-1)])).all()


def test_strided_reference_layout_and_hdr_wrap():
    H, W, S = 4, 6, 10
    p = (np.arange(H * S * 3 // 2, dtype=np.uint32) * 977 % 65536).astype(np.uint16)
    nv = planar_ref.planar_to_semiplanar(p, H, W, S, True)
    n_y, n_c = H * S, (H // 2) * (S // 2)
    for m in range(H // 2):
        for k in range(W // 2):
            assert nv[n_y + m * S + 2 * k] == (int(p[n_y + m * (S // 2) + k]) << 6) & 0xFFFF
            assert nv[n_y + m * S + 2 * k + 1] == (int(p[n_y + n_c + m * (S // 2) + k]) << 6) & 0xFFFF
    assert nv[1 * S + 3] == (int(p[1 * S + 3]) << 6) & 0xFFFF
    back = planar_ref.semiplanar_to_planar(nv, H, W, S, True)
    y, u, v = planar_ref.planar_planes(back, H, W, S)
    y0, u0, v0 = planar_ref.planar_planes(p, H, W, S)
    assert (y == (y0 & 1023)).all() and (u == (u0 & 1023)).all() and (v == (v0 & 1023)).all()
