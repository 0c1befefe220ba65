"""The host-side logic of the one-pairing verify calls (kzg_amd/csrc/vcb_host.h: the counting sort of a chunk's openings by commitment,
the weight walk of kzg_verify_fold) as a stand-alone program, plain and under -fsanitize=address,undefined on the CPU: the sort against
a brute-force grouping, chunk after chunk through one object, the walk against r^g gamma_g^i computed directly."""
import os
import random
import struct
import subprocess

import pytest

from oracle import kzg_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = M.R


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("vcbh") / ("host_vcb_host_" + request.param))
    flags = ["-O1"] if request.param == "plain" else ["-O0", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.check_call(["g++", "-std=c++17"] + flags + ["-o", path, os.path.join(ROOT, "tests", "host_vcb_host.cpp")])
    return path


def run(exe, tmp_path, blob):
    src, dst = str(tmp_path / "in"), str(tmp_path / "out")
    with open(src, "wb") as f:
        f.write(blob)
    res = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert res.returncode == 0 and not res.stderr, res.stderr  # a sanitizer report ends the program with a message
    return open(dst, "rb").read()


def sort_chunks(exe, tmp_path, n_commitments, B0, chunks):
    """[(which, start, order, non-zero entries of cnt after the build)] per chunk, all chunks through one object"""
    blob = struct.pack("<4I", 0, n_commitments, B0, len(chunks))
    for cm in chunks:
        blob += struct.pack("<%dI" % (1 + len(cm)), len(cm), *cm)
    out, at, res = run(exe, tmp_path, blob), 0, []
    for cm in chunks:
        lists, dirty = struct.unpack_from("<2I", out, at)
        body = struct.unpack_from("<%dI" % (2 * lists + 1 + len(cm)), out, at + 8)
        at += 8 + 4 * len(body)
        res.append((list(body[:lists]), list(body[lists:2 * lists + 1]), list(body[2 * lists + 1:]), dirty))
    assert at == len(out)
    return res


def grouped(cm):
    """brute force: the commitments in the order of their first opening, each with its chunk-local openings in ascending order"""
    which = []
    for m in cm:
        if m not in which:
            which.append(m)
    per = [[k for k in range(len(cm)) if cm[k] == m] for m in which]
    start = [sum(len(p) for p in per[:g]) for g in range(len(which) + 1)]
    return which, start, [k for p in per for k in p]


LIST15 = [3, 0, 3, 7, 7, 1, 0, 3, 9, 9, 9, 2, 7, 0, 5]  # commitments below 10; 4, 6 and 8 are never named

SORT_CASES = {
    "one opening": (1, 1, [[0]]),
    "one commitment": (3, 9, [[2] * 9]),
    "all distinct": (6, 6, [[4, 2, 5, 0, 3, 1]]),
    "unnamed commitments": (40, 5, [[39, 7, 39, 0, 7]]),
    "15 entries in chunks of 4": (10, 4, [LIST15[k:k + 4] for k in range(0, 15, 4)]),
    "15 entries in chunks of 7": (10, 7, [LIST15[k:k + 7] for k in range(0, 15, 7)]),
}


@pytest.mark.parametrize("case", sorted(SORT_CASES))
def test_counting_sort_matches_a_brute_force_grouping_and_leaves_cnt_zero(exe, tmp_path, case):
    n_commitments, B0, chunks = SORT_CASES[case]
    got = sort_chunks(exe, tmp_path, n_commitments, B0, chunks)
    for cm, (which, start, order, dirty) in zip(chunks, got):
        assert (which, start, order) == grouped(cm), cm
        assert len(start) == len(which) + 1 and start[-1] == len(cm)
        assert dirty == 0, "cnt is not zero again after the build"


@pytest.mark.parametrize("chunk", [1, 4, 7, 64])
@pytest.mark.parametrize("t,groups", [(1, 5), (3, 5), (4, 1)])
def test_weight_walk_across_chunks_is_r_g_gamma_g_i(exe, tmp_path, t, groups, chunk):
    rng = random.Random(1000 * t + 10 * groups + chunk)
    r, gammas = rng.randrange(1, R), [rng.randrange(1, R) for _ in range(groups)]
    gammas[0] = R - 1  # the largest scalar
    blob = struct.pack("<4I", 1, t, groups, chunk) + b"".join(x.to_bytes(32, "little") for x in [r] + gammas)
    out = run(exe, tmp_path, blob)
    got = [int.from_bytes(out[32 * k:32 * k + 32], "little") for k in range(len(out) // 32)]
    assert got == [pow(r, g, R) * pow(gammas[g], i, R) % R for g in range(groups) for i in range(t)]
