"""The sign-tracked mixed addition of curve30.h (k_accum_affine's loop body) on the host, no GPU: tests/host_madd_signed.cpp is a
stand-alone program -- chains of 64 table entries under 35 sign patterns against g1_madd30, with doublings, inverses, identity
entries and restarts inside, every limb checked against the bound of the next operation after every step; mul30_sgn limb for limb
against mul30_sub (t = -1) and mul30 + add30 (t = +1).  Built with UBSan on its own compile line and run as a child process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sign_tracked_madd_chains_and_mul30_sgn(tmp_path):
    exe = str(tmp_path / "host_madd_signed")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "host_madd_signed.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert " 0 failed, 35 sign patterns" in r.stdout
