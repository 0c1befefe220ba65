"""kzg_test_tower (kzg_amd/csrc/tower_hooks.hip): the pairing tower of kzg_amd/csrc/tower.h as gfx950 runs it -- the inline-asm
multiply, out-of-line functions on operands in scratch memory, called aliased as the verifier kernels call them -- against
oracle/pairing_model.py value by value.  The vectors and their expected bytes are tests/tower_vectors.py, the set that
tests/test_host_tower.py puts through the host build of the same record bodies.  One launch per op carries all of the op's records, the
aliasing forms among them; every comparison is byte-exact."""
import ctypes

import pytest

from kzg_amd import _lib as L
from tests import tower_vectors as TV
from tests.gpu_common import HooksEngine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hooks_engine():  # noqa: F811
    """a hooks context of this module's own: in the suite's order (tests/conftest.py ORDER) the file runs behind the tests that close
    the session's contexts"""
    h = HooksEngine(0)
    yield h
    h.close()


def run(hooks, name, records):
    in_rec, out_rec = TV.SHAPES[name]
    out = ctypes.create_string_buffer(len(records) * out_rec)
    rc = hooks.lib.kzg_test_tower(hooks.ctx, TV.OP[name], b"".join(records), in_rec, len(records), out, out_rec)
    assert rc == 0, hooks.last_error()
    return [out.raw[i * out_rec:(i + 1) * out_rec] for i in range(len(records))]


@pytest.mark.parametrize("name", TV.OPS)
def test_tower_op_matches_the_model(hooks_engine, name):
    """Names the record index, the aliasing form and the first differing coefficient on failure (tower_vectors.check)."""
    TV.check(name, run(hooks_engine, name, [rec for rec, _, _ in TV.vectors(name)]))


def test_tower_rejects_bad_shapes(hooks_engine):
    """Unknown ops, record sizes of another op, no records, and alias / power / np / mask words outside the documented contract:
    KZG_ERR_SHAPE, nothing launched."""
    lib, ctx = hooks_engine.lib, hooks_engine.ctx
    rec = bytes(1160)
    out = ctypes.create_string_buffer(13056)
    for op, in_rec, out_rec in [(-1, 196, 96), (len(TV.OPS), 196, 96), (TV.OP["f2_mul"], 100, 96), (TV.OP["f2_mul"], 196, 576),
                                (TV.OP["f12_mul"], 580, 576), (TV.OP["f12_is_one"], 576, 576), (TV.OP["miller_loop"], 1160, 4),
                                (TV.OP["pairing_product_is_one"], 1160, 576), (TV.OP["g2_precompute_lines"], 192, 192)]:
        assert lib.kzg_test_tower(ctx, op, rec, in_rec, 1, out, out_rec) == L.KZG_ERR_SHAPE, (op, in_rec, out_rec)
    for name, bad in TV.BAD_RECORDS:
        assert lib.kzg_test_tower(ctx, TV.OP[name], bad, TV.SHAPES[name][0], 1, out, TV.SHAPES[name][1]) == L.KZG_ERR_SHAPE, name
    # a bad record behind good ones is found too
    good = TV.vectors("f12_sqr")[0][0]
    bad = dict(TV.BAD_RECORDS)["f12_sqr"]
    assert lib.kzg_test_tower(ctx, TV.OP["f12_sqr"], good + good + bad, 580, 3, out, 576) == L.KZG_ERR_SHAPE
    assert lib.kzg_test_tower(ctx, TV.OP["f2_mul"], rec, 196, 0, out, 96) == L.KZG_ERR_SHAPE
    assert lib.kzg_test_tower(ctx, TV.OP["f2_mul"], None, 196, 1, out, 96) == L.KZG_ERR_SHAPE
