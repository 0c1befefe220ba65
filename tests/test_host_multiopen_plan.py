"""The host-side plan of the two-element multiproof (kzg_amd/csrc/multiopen_plan.h: the claims sorted by point, the distinct points, the
points of the domain behind the others, the chunk size, r^k, the weights w_k = r^k / (t - z_k) formed in chunks with one inversion each,
W_m) as a stand-alone program, plain and under -fsanitize=address,undefined on the CPU, against the python model
(tests/multiopen_model.py)."""
import os
import random
import struct
import subprocess

import pytest

from tests import multiopen_model as MO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = MO.R


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("mop") / ("host_multiopen_plan_" + request.param))
    flags = ["-O1"] if request.param == "plain" else ["-O0", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.check_call(["g++", "-std=c++17"] + flags + ["-o", path, os.path.join(ROOT, "tests", "host_multiopen_plan.cpp")])
    return path


def run(exe, tmp_path, tag, n_polys, d, option, wchunk, r, t, zs, on, idx):
    count = len(zs)
    blob = struct.pack("<6I", count, n_polys, d, option, wchunk, 1 if idx is not None else 0)
    blob += r.to_bytes(32, "little") + t.to_bytes(32, "little") + b"".join(z.to_bytes(32, "little") for z in zs) + bytes(on)
    if idx is not None:
        blob += struct.pack("<%dI" % count, *idx)
    src, dst = str(tmp_path / ("in" + tag)), str(tmp_path / ("out" + tag))
    with open(src, "wb") as f:
        f.write(blob)
    res = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert res.returncode == 0 and not res.stderr, res.stderr  # a sanitizer report ends the program with a message
    out = open(dst, "rb").read()
    U, n_off, cap, hit = struct.unpack_from("<4I", out, 0)
    at = 16
    order = list(struct.unpack_from("<%dI" % count, out, at))
    at += 4 * count
    pstart = list(struct.unpack_from("<%dI" % (U + 1), out, at))
    at += 4 * (U + 1)

    def scalars(n):
        nonlocal at
        v = [int.from_bytes(out[at + 32 * i:at + 32 * i + 32], "little") for i in range(n)]
        at += 32 * n
        return v

    points, rk, w, W = scalars(U), scalars(count), scalars(count), scalars(n_polys)
    assert at == len(out)
    return U, n_off, cap, hit, order, pstart, points, rk, w, W


CASES = [
    # count, n_polys, distinct points, d, option, wchunk, identity indices
    (0, 3, 1, 8, 0, 0, False),
    (1, 1, 1, 1, 0, 0, True),
    (7, 3, 3, 256, 0, 0, False),
    (33, 4, 33, 1 << 20, 0, 5, False),
    (17, 17, 2, 1 << 19, 3, 16, True),
    (40, 5, 9, 64, 16, 7, False),
]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_plan_matches_the_model(exe, tmp_path, case):
    count, n_polys, n_points, d, option, wchunk, identity = CASES[case]
    rng = random.Random(200 + case)
    pts = [rng.randrange(R) for _ in range(n_points)]
    pts[0] = R - 1  # the largest scalar
    on_pts = {p for i, p in enumerate(pts) if i % 3 == 1}  # which points the caller calls "on the domain"
    zs = [pts[rng.randrange(n_points)] for _ in range(count)]
    idx = None if identity else [rng.randrange(n_polys) for _ in range(count)]
    r, t = rng.randrange(1, R), rng.randrange(R)
    while t in zs:
        t = rng.randrange(R)
    U, n_off, cap, hit, order, pstart, points, rk, w, W = run(exe, tmp_path, str(case), n_polys, d, option, wchunk, r, t, zs,
                                                               [1 if z in on_pts else 0 for z in zs], idx)
    m_order, m_pstart, m_points, m_chunks = MO.plan(zs, cap, on=lambda z: z in on_pts)
    assert (order, pstart, points) == (m_order, m_pstart, m_points)
    assert U == len(m_points) and n_off == sum(1 for p in m_points if p not in on_pts)
    assert cap == min(max(1, min(16, (1 << 22) // d)), option or 16)
    assert rk == [pow(r, k, R) for k in range(count)]
    assert hit == 0 and (w, W) == MO.poly_weights(zs, idx, n_polys, r, t)
    assert (w, W) == MO.poly_weights(zs, idx, n_polys, r, t, wchunk or None)


def test_t_equal_to_a_point_is_reported_and_nothing_is_written(exe, tmp_path):
    rng = random.Random(9)
    zs = [rng.randrange(R) for _ in range(6)]
    for where in (0, 3, 5):
        out = run(exe, tmp_path, "hit%d" % where, 2, 8, 0, 4, 5, zs[where], zs, [0] * 6, [0, 1, 0, 1, 0, 1])
        assert out[3] == 1 and not any(out[8]) and not any(out[9])
