"""The generated sources and the build record of the post-processed device code (no GPU needed)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kzg_amd", "csrc")


def test_generated_files_match_their_generators(tmp_path):
    """Every "do not edit" file under kzg_amd/csrc is what its generator writes today, byte for byte: a hand edit of one would
    escape both the generator and the tests of the portable branch (tests/host_math.cpp does not compile the inline asm)."""
    runs = [("gen_mul.py", ["mul_gfx950.inc"]), ("gen_mul30.py", ["mul30_gfx950.inc", "mul29r_gfx950.inc"]),
            ("gen_fq30.py", ["fq30_consts.inc"]), ("gen_fr29.py", ["fr29_consts.inc"])]
    for tool, outs in runs:
        subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool)] + [str(tmp_path / o) for o in outs], check=True, cwd=ROOT,
                       capture_output=True, timeout=120)
        for o in outs:
            with open(tmp_path / o, "rb") as f, open(os.path.join(CSRC, o), "rb") as g:
                assert f.read() == g.read(), "%s differs from the output of tools/%s" % (o, tool)


def test_arith_hooks_built_through_the_nop_post_processing():
    """kzg_test_arith's kernels run the generated asm in the form msm.hip / ntt.hip run it: with the validated compiler, the build
    sent arith_hooks.hip through strip_asm_nops and removed nops; otherwise it was built with every nop in place (and says so)."""
    from kzg_amd import build as kb
    kb.build()      # up to date after build(): only reads the record
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with open(os.path.join(os.path.dirname(kb.__file__), "build", kb.NOPS_FILE)) as f:
        rec = json.load(f)
    if kb.asm_path_ok(hipcc):
        assert rec.get("arith_hooks.hip", 0) > 0, rec
        assert rec.get("msm.hip", 0) > 0 and rec.get("ntt.hip", 0) > 0, rec
    else:
        assert rec.get("arith_hooks.hip") == 0, rec


def test_product_library_exports_no_test_hook():
    from kzg_amd import build as kb
    kb.build()
    r = subprocess.run(["nm", "-D", "--defined-only", kb.OUT], capture_output=True, text=True, check=True)
    assert "kzg_test_" not in r.stdout
    r = subprocess.run(["nm", "-D", "--defined-only", kb.OUT_HOOKS], capture_output=True, text=True, check=True)
    assert " kzg_test_arith" in r.stdout
