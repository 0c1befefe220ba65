"""The host finish of kzg_verify_cosets_batch (kzg_amd/csrc/vcb_finish.h: Horner over the window sums, P2 + Cagg - Ragg, the pairing
product) as a stand-alone program under -fsanitize=address,undefined on the CPU, against the python oracle (oracle/pairing_model.py)
on one accepting and one rejecting input."""
import os
import random
import subprocess

import pytest

from oracle import kzg_model as M, pairing_model as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = M.R
TAU, L_COSET = 0x5EEDF00D, 16


def g1b(p):
    return bytes(96) if p is None else p[0].to_bytes(48, "little") + p[1].to_bytes(48, "little")


def g1u(b):
    p = (int.from_bytes(b[:48], "little"), int.from_bytes(b[48:96], "little"))
    return None if p == (0, 0) else p


def g2b(p):
    return b"".join(c.to_bytes(48, "little") for xy in p for c in xy)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("vcb") / "host_vcb_finish")
    subprocess.check_call(["g++", "-O0", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", path,
                           os.path.join(ROOT, "tests", "host_vcb_finish.cpp")])
    return path


def test_finish_under_sanitizers_matches_the_oracle(exe, tmp_path):
    rng = random.Random(11)
    # window sums as scalars (discrete logs): digits windows of three sets, with the identity and equal neighbours among them
    wins = [[rng.randrange(R) for _ in range(32)] for _ in range(3)]
    wins[0][5] = 0
    wins[1][7] = wins[1][8]
    wins[2][31] = 0
    total = [sum(w << (8 * k) for k, w in enumerate(ws)) % R for ws in wins]  # P1, P2, Cagg
    tl = pow(TAU, L_COSET, R)
    hs0, hsl = P.G2, P.g2_mul(P.G2, tl)
    good = (total[1] + total[2] - total[0] * tl) % R  # Ragg that balances e(P1, hs[l]) e(-(P2 + Cagg - Ragg), hs[0]) == 1
    for ragg, want in ((good, 1), ((good + 1) % R, 0)):
        blob = b"".join(g1b(M.g1_mul(M.G1, w)) for ws in wins for w in ws) + g1b(M.g1_mul(M.G1, ragg)) + g2b(hs0) + g2b(hsl)
        src, dst = str(tmp_path / ("in%d" % want)), str(tmp_path / ("out%d" % want))
        with open(src, "wb") as f:
            f.write(blob)
        run = subprocess.run([exe, src, dst], capture_output=True, text=True)
        assert run.returncode == 0 and not run.stderr, run.stderr  # a sanitizer report ends the program with a message
        out = open(dst, "rb").read()
        parts = [g1u(out[1 + 96 * i:1 + 96 * (i + 1)]) for i in range(4)]
        assert parts == [M.g1_mul(M.G1, s) for s in total + [ragg]]
        acc = M.g1_mul(M.G1, (total[1] + total[2] - ragg) % R)
        oracle = P.pairing_product_is_one([(parts[0], hsl), (M.g1_neg(acc), hs0)])
        assert out[0] == want == int(oracle)
