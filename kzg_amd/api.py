"""Host-side mirror of the reference's prover surface over the C ABI (include/kzg_mi355x.h).

Names, argument meaning and error behaviour follow proxima-one/kzg:
  setup / KZGParams                      src/lib.rs:14-55
  Polynomial                             src/polynomial.rs:24-165
  EvaluationDomain                       src/ft.rs:17-140
  KZGProver / KZGVerifier.verify_poly    src/coeff_form.rs:37-124
  KZGProverEvalForm / verify_poly        src/eval_form.rs:39-171
Scalars cross this layer as python ints (canonical, < r) or as packed 32-byte little-endian blobs;
G1 points as 96-byte affine-Montgomery blobs (`bytes`), identity = 96 zero bytes.  All arithmetic
happens on the GPU in libkzg_mi355x.so; nothing here computes field or curve operations.
"""
import ctypes
import os
import secrets

from . import _lib as L

R_MODULUS = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
FR_MONT_R = (1 << 256) % R_MODULUS  # blst_fr / KZG_FR_MONT_LE_32: a * 2^256 mod r


class KZGError(Exception):
    """src/lib.rs:26-36"""


class PointNotOnPolynomial(KZGError):
    pass


class PolynomialDegreeTooLarge(KZGError):
    pass


class ReferencePanic(Exception):
    """A condition on which the reference panics (slice out of range, failed assert!, ...)."""


class EngineError(RuntimeError):
    pass


def _raise(engine, rc):
    msg = engine.last_error() if engine is not None else ""
    if rc == L.KZG_ERR_POINT_NOT_ON_POLY:
        raise PointNotOnPolynomial(msg or "point not on polynomial!")
    if rc == L.KZG_ERR_DEGREE_TOO_LARGE:
        raise PolynomialDegreeTooLarge(msg or "polynomial degree too large")
    if rc == L.KZG_ERR_SHAPE:
        raise ReferencePanic(msg)
    raise EngineError(f"kzg_mi355x error {rc}: {msg}")


def pack_scalars(xs):
    """list of ints -> canonical LE blob; bytes-like passes through."""
    if isinstance(xs, (bytes, bytearray, memoryview)):
        return bytes(xs)
    return b"".join((int(x) % R_MODULUS).to_bytes(32, "little") for x in xs)


def unpack_scalars(b):
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


class DeviceBuffer:
    """Scalars resident in HBM (n x 32 B), owned by an Engine."""

    def __init__(self, engine, n, sfmt=L.FR_CANONICAL):
        self.engine, self.n, self.sfmt = engine, n, sfmt
        p = ctypes.c_void_p()
        rc = engine.lib.kzg_dev_alloc(engine.ctx, n * 32, ctypes.byref(p))
        if rc:
            _raise(engine, rc)
        self.ptr = p

    def upload(self, blob):
        assert len(blob) == self.n * 32
        rc = self.engine.lib.kzg_dev_upload(self.engine.ctx, self.ptr, blob, len(blob))
        if rc:
            _raise(self.engine, rc)
        return self

    def download(self, n=None, offset=0):
        n = self.n - offset if n is None else n
        out = ctypes.create_string_buffer(n * 32)
        src = ctypes.c_void_p(self.ptr.value + offset * 32)
        rc = self.engine.lib.kzg_dev_download(self.engine.ctx, out, src, n * 32)
        if rc:
            _raise(self.engine, rc)
        return out.raw

    def fill_random(self, seed, u64_valued=False):
        rc = self.engine.lib.kzg_fill_random_fr(self.engine.ctx, self.ptr, self.n, seed, 1 if u64_valued else 0, self.sfmt)
        if rc:
            _raise(self.engine, rc)
        return self

    def free(self):
        if self.ptr:
            self.engine.lib.kzg_dev_free(self.engine.ctx, self.ptr)
            self.ptr = None


def splitmix_scalar(seed, i, u64_valued=False):
    """The element kzg_fill_random_fr writes at index i (definition in include/kzg_mi355x.h)."""
    M = (1 << 64) - 1

    def sm(z):
        z = (z + 0x9E3779B97F4A7C15) & M
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        return z ^ (z >> 31)

    v = 0
    for k in range(1 if u64_valued else 4):
        v |= sm((seed + 4 * i + k) & M) << (64 * k)
    return v % R_MODULUS


class Engine:
    """One kzg_ctx bound to one GPU."""

    def __init__(self, device=0):
        self.lib = L.load()
        ctx = ctypes.c_void_p()
        rc = self.lib.kzg_ctx_create(device, ctypes.byref(ctx))
        if rc:
            raise EngineError(f"kzg_ctx_create(device={device}) failed with {rc}: no usable HIP device "
                              "(kzg_amd has no CPU fallback)")
        self.ctx = ctx
        self.device = device

    def close(self):
        if self.ctx and not getattr(self, "_borrowed", False):
            self.lib.kzg_ctx_destroy(self.ctx)
        self.ctx = None

    def last_error(self):
        return (self.lib.kzg_last_error(self.ctx) or b"").decode()

    def set_option(self, key, value):
        rc = self.lib.kzg_ctx_set_option(self.ctx, key.encode(), value)
        if rc:
            _raise(self, rc)

    def info(self):
        """the batched pipeline's plan and whether the process' hardware-queue pool narrowed it (kzg_ctx_info)"""
        buf = ctypes.create_string_buffer(512)
        rc = self.lib.kzg_ctx_info(self.ctx, buf, 512)
        if rc:
            _raise(self, rc)
        return buf.value.decode()

    def sync(self):
        rc = self.lib.kzg_sync(self.ctx)
        if rc:
            _raise(self, rc)

    def alloc_scalars(self, n, sfmt=L.FR_CANONICAL):
        return DeviceBuffer(self, n, sfmt)

    # --- profiling ---
    def prof_enable(self, on=True):
        """True / 1: HIP events around every kernel; 2: around the bucket-accumulation kernel only; False / 0: off"""
        self.lib.kzg_prof_enable(self.ctx, int(on))

    def prof_reset(self):
        self.lib.kzg_prof_reset(self.ctx)

    def prof_get(self, name):
        n, ms = ctypes.c_uint64(), ctypes.c_double()
        self.lib.kzg_prof_get(self.ctx, name.encode(), ctypes.byref(n), ctypes.byref(ms))
        return n.value, ms.value

    def prof_all(self):
        buf = ctypes.create_string_buffer(8192)
        self.lib.kzg_prof_names(self.ctx, buf, 8192)
        names = [s for s in buf.value.decode().split(",") if s]
        return {k: self.prof_get(k) for k in names}

    # --- raw operations used by the classes below and by bench.py ---
    def _scalars_arg(self, scalars):
        if isinstance(scalars, DeviceBuffer):
            return scalars.ptr, scalars.n, scalars.sfmt, L.IN_DEVICE, None
        blob = pack_scalars(scalars)
        return blob, len(blob) // 32, L.FR_CANONICAL, 0, blob

    def msm(self, srs, scalars, n=None, offset=0, ofmt=L.G1_AFFINE_MONT):
        ptr, nn, sfmt, flags, _keep = self._scalars_arg(scalars)
        n = nn if n is None else n
        out = ctypes.create_string_buffer(L.POINT_BYTES[ofmt])
        rc = self.lib.kzg_msm_g1(self.ctx, srs.handle, offset, ptr, n, sfmt, flags, out, ofmt)
        if rc:
            _raise(self, rc)
        return out.raw

    def msm_batch(self, srs, scalars, n, batch, offset=0, ofmt=L.G1_AFFINE_MONT):
        ptr, nn, sfmt, flags, _keep = self._scalars_arg(scalars)
        assert nn >= n * batch
        out = ctypes.create_string_buffer(L.POINT_BYTES[ofmt] * batch)
        rc = self.lib.kzg_msm_g1_batch(self.ctx, srs.handle, offset, ptr, n, batch, sfmt, flags, out, ofmt)
        if rc:
            _raise(self, rc)
        psz = L.POINT_BYTES[ofmt]
        return [out.raw[i * psz:(i + 1) * psz] for i in range(batch)]

    def g1_sum(self, blobs, pfmt=L.G1_AFFINE_MONT, ofmt=L.G1_AFFINE_MONT):
        raw = b"".join(blobs)
        out = ctypes.create_string_buffer(L.POINT_BYTES[ofmt])
        rc = self.lib.kzg_g1_sum(self.ctx, raw, len(blobs), pfmt, 0, out, ofmt)
        if rc:
            _raise(self, rc)
        return out.raw

    def g1_sum_batch(self, blobs, count, groups, pfmt=L.G1_AFFINE_MONT, ofmt=L.G1_AFFINE_MONT):
        """out[g] = sum_i blobs[g*count + i]."""
        raw = b"".join(blobs)
        psz = L.POINT_BYTES[ofmt]
        out = ctypes.create_string_buffer(psz * groups)
        rc = self.lib.kzg_g1_sum_batch(self.ctx, raw, count, groups, pfmt, 0, out, ofmt)
        if rc:
            _raise(self, rc)
        return [out.raw[i * psz:(i + 1) * psz] for i in range(groups)]

    def _ntt_group(self, fn, sizes, points, log_n, batch, inverse, pfmt, ofmt):
        d = 1 << log_n
        if batch is None:
            batch = len(points) // (d * sizes[pfmt])
        assert len(points) == batch * d * sizes[pfmt], "points must hold batch x 2^log_n points in pfmt"
        out = ctypes.create_string_buffer(max(batch * d * sizes[ofmt], 1))
        rc = fn(self.ctx, points, log_n, batch, 1 if inverse else 0, pfmt, 0, out, ofmt)
        if rc:
            _raise(self, rc)
        return out.raw[: batch * d * sizes[ofmt]]

    def ntt_g1(self, points, log_n, batch=None, inverse=False, pfmt=L.G1_AFFINE_MONT, ofmt=L.G1_AFFINE_MONT):
        """kzg_ntt_g1: the DFT of `batch` arrays of 2^log_n G1 points (a blob in pfmt, arrays one after the other) over
        compute_omega(2^log_n): out[m] = sum_j [w^(jm)] P[j]; inverse: out[j] = [1/d] sum_m [w^(-jm)] P[m].  Natural order in and out;
        returns the blob in ofmt."""
        return self._ntt_group(self.lib.kzg_ntt_g1, L.POINT_BYTES, points, log_n, batch, inverse, pfmt, ofmt)

    def ntt_g2(self, points, log_n, batch=None, inverse=False, pfmt=L.G2_AFFINE_MONT, ofmt=L.G2_AFFINE_MONT):
        """kzg_ntt_g2: the same over G2 (log_n <= 20)."""
        return self._ntt_group(self.lib.kzg_ntt_g2, L.G2_POINT_BYTES, points, log_n, batch, inverse, pfmt, ofmt)

    def ntt(self, data, log_n, inverse=False):
        """data: DeviceBuffer (in place) or ints/blob (returns list of ints)."""
        if isinstance(data, DeviceBuffer):
            rc = self.lib.kzg_ntt_fr(self.ctx, data.ptr, log_n, 1 if inverse else 0, L.IN_DEVICE)
            if rc:
                _raise(self, rc)
            return data
        blob = pack_scalars(data)
        assert len(blob) == 32 << log_n
        buf = ctypes.create_string_buffer(blob, len(blob))
        rc = self.lib.kzg_ntt_fr(self.ctx, buf, log_n, 1 if inverse else 0, 0)
        if rc:
            _raise(self, rc)
        return unpack_scalars(buf.raw)

    def coset_ntt(self, data, log_n, inverse=False):
        blob = pack_scalars(data)
        buf = ctypes.create_string_buffer(blob, len(blob))
        rc = self.lib.kzg_coset_ntt_fr(self.ctx, buf, log_n, 1 if inverse else 0, L.FR_CANONICAL, 0)
        if rc:
            _raise(self, rc)
        return unpack_scalars(buf.raw)

    def _ntt_batch(self, coset, data, log_n, batch, stride, inverse):
        n = 1 << log_n
        if isinstance(data, DeviceBuffer):
            assert batch is not None and data.n >= ((batch - 1) * (stride or n) + n if batch else 0)
            if coset:
                rc = self.lib.kzg_coset_ntt_fr_batch(self.ctx, data.ptr, log_n, batch, stride or 0, 1 if inverse else 0, data.sfmt, L.IN_DEVICE)
            else:
                rc = self.lib.kzg_ntt_fr_batch(self.ctx, data.ptr, log_n, batch, stride or 0, 1 if inverse else 0, L.IN_DEVICE)
            if rc:
                _raise(self, rc)
            return data
        vectors = [pack_scalars(v) for v in data]
        if any(len(v) != 32 * n for v in vectors) or (batch is not None and batch != len(vectors)):
            raise ValueError("ntt_batch: every vector must hold 2^log_n scalars, and batch (if given) must be their number")
        if stride not in (None, 0, n):
            raise ValueError("ntt_batch: stride applies to device buffers; vectors given as lists are contiguous")
        blob = b"".join(vectors)
        buf = ctypes.create_string_buffer(blob, len(blob) or 1)
        if coset:
            rc = self.lib.kzg_coset_ntt_fr_batch(self.ctx, buf, log_n, len(vectors), 0, 1 if inverse else 0, L.FR_CANONICAL, 0)
        else:
            rc = self.lib.kzg_ntt_fr_batch(self.ctx, buf, log_n, len(vectors), 0, 1 if inverse else 0, 0)
        if rc:
            _raise(self, rc)
        out = unpack_scalars(buf.raw[:len(blob)])
        return [out[i * n:(i + 1) * n] for i in range(len(vectors))]

    def ntt_batch(self, data, log_n, batch=None, stride=None, inverse=False):
        """kzg_ntt_fr_batch: `batch` transforms of 2^log_n points in one call.  data: a DeviceBuffer (in place; vector b at element
        b * stride, stride None = 2^log_n) or a list of equal-length scalar lists / canonical blobs (returns a list of int lists)."""
        return self._ntt_batch(False, data, log_n, batch, stride, inverse)

    def coset_ntt_batch(self, data, log_n, batch=None, stride=None, inverse=False):
        """kzg_coset_ntt_fr_batch: as ntt_batch, on the coset 7 H (coset_fft / icoset_fft of every vector)."""
        return self._ntt_batch(True, data, log_n, batch, stride, inverse)

    def poly_eval(self, coeffs, x, n=None):
        ptr, nn, sfmt, flags, _keep = self._scalars_arg(coeffs)
        n = nn if n is None else n
        out = ctypes.create_string_buffer(32)
        xb = self._host_scalar(x, sfmt)
        rc = self.lib.kzg_poly_eval(self.ctx, ptr, n, xb, sfmt, flags, out)
        if rc:
            _raise(self, rc)
        return self._scalar_from(out.raw, sfmt)

    def poly_multi_eval(self, coeffs, xs, n=None, batch=1, out=None):
        """kzg_poly_multi_eval: the values p_b(xs[i]) of `batch` polynomials of n coefficients each (coeffs: ints, a canonical blob or
        a DeviceBuffer of batch x n scalars back to back) at the points xs (ints below R), in one call.  Returns a list of `batch`
        lists of len(xs) ints -- one flat list for batch = 1 -- or `out` (a DeviceBuffer of batch x len(xs) scalars in the
        coefficients' format) when one is given."""
        ptr, nn, sfmt, flags, _keep = self._scalars_arg(coeffs)
        if n is None:
            if batch < 1 or nn % batch:
                raise ReferencePanic("%d scalars are not %d polynomials of equal length" % (nn, batch))
            n = nn // batch
        if nn < n * batch:  # the call would read past the buffer
            raise ReferencePanic("%d scalars given, batch * n = %d" % (nn, batch * n))
        k = len(xs)
        xb = b"".join(self._host_scalar(int(x), sfmt) if 0 <= int(x) < R_MODULUS else (int(x) % (1 << 256)).to_bytes(32, "little") for x in xs)
        if out is not None:
            if out.n < batch * k or out.sfmt != sfmt:
                raise ReferencePanic("poly_multi_eval: out holds %d scalars, batch * k = %d (and has the coefficients' format)" % (out.n, batch * k))
            rc = self.lib.kzg_poly_multi_eval(self.ctx, ptr, n, batch, xb, k, sfmt, flags | L.OUT_DEVICE, out.ptr)
            if rc:
                _raise(self, rc)
            return out
        buf = ctypes.create_string_buffer(32 * max(batch * k, 1))
        rc = self.lib.kzg_poly_multi_eval(self.ctx, ptr, n, batch, xb, k, sfmt, flags, buf)
        if rc:
            _raise(self, rc)
        ys = [self._scalar_from(buf.raw[32 * j:32 * j + 32], sfmt) for j in range(batch * k)]
        return ys if batch == 1 else [ys[b * k:(b + 1) * k] for b in range(batch)]

    def interpolate(self, xs, ys):
        """kzg_interpolate: the coefficients (k ints, lowest first) of the polynomial of degree < k through (xs[i], ys[i]); ys may be
        a list of value vectors on the one point set (then a list of coefficient lists comes back).  One point gives the constant."""
        k = len(xs)
        many = k > 0 and len(ys) > 0 and isinstance(ys[0], (list, tuple))
        rows = [list(v) for v in ys] if many else [list(ys)]
        if any(len(v) != k for v in rows):
            raise ReferencePanic("assert_eq!(xs.len(), ys.len())")
        xb = b"".join(int(x).to_bytes(32, "little") if 0 <= int(x) < (1 << 256) else pack_scalars([x]) for x in xs)
        out = ctypes.create_string_buffer(32 * max(len(rows) * k, 1))
        rc = self.lib.kzg_interpolate(self.ctx, xb, pack_scalars([y for v in rows for y in v]), k, len(rows), L.FR_CANONICAL, 0, out)
        if rc:
            _raise(self, rc)
        cs = unpack_scalars(out.raw[: 32 * len(rows) * k])
        return [cs[b * k:(b + 1) * k] for b in range(len(rows))] if many else cs

    def point_tree(self, xs):
        """kzg_point_tree_setup: the reusable sub-product tree of the points xs (ints below R, 1 <= len(xs) <= 2^22) as a PointTree."""
        return PointTree(self, xs)

    def quotient_linear(self, coeffs, x, y):
        blob = pack_scalars(coeffs)
        n = len(blob) // 32
        out = ctypes.create_string_buffer(max(1, n - 1) * 32)
        rc = self.lib.kzg_quotient_linear(self.ctx, blob, n, (x % R_MODULUS).to_bytes(32, "little"),
                                          (y % R_MODULUS).to_bytes(32, "little"), L.FR_CANONICAL, 0, out)
        if rc:
            _raise(self, rc)
        return unpack_scalars(out.raw[: (n - 1) * 32])

    def poly_mul(self, a, b):
        """Polynomial::fft_mul / best_mul: coefficient list of a * b."""
        ab, bb = pack_scalars(a), pack_scalars(b)
        na, nb = len(ab) // 32, len(bb) // 32
        out = ctypes.create_string_buffer(32 * (na + nb - 1))
        rc = self.lib.kzg_poly_mul(self.ctx, ab, na, bb, nb, L.FR_CANONICAL, 0, out)
        if rc:
            _raise(self, rc)
        return unpack_scalars(out.raw)

    def poly_divide(self, a, b, batch=1, na=None, q_out=None, r_out=None):
        """kzg_poly_divide: `batch` dividends of na coefficients each (a: ints, a canonical blob or a DeviceBuffer of batch x na
        scalars back to back) by the one divisor b (lowest coefficient first, b[-1] != 0; ints, a blob, or a DeviceBuffer when a is
        one).  Returns (q, r, exact): the quotients zero-padded to na - nb + 1 and the remainders zero-padded to nb - 1 coefficients
        -- flat lists of ints for batch = 1, lists of `batch` lists otherwise, or the DeviceBuffers q_out / r_out (in the dividends'
        format) when both are given -- and exact, a list of `batch` bools: the remainder is zero (the reference's None).  na < nb
        leaves q empty and r the dividend."""
        ptr, nn, sfmt, flags, _keep = self._scalars_arg(a)
        if na is None:
            if batch < 1 or nn % batch:
                raise ReferencePanic("%d scalars are not %d dividends of equal length" % (nn, batch))
            na = nn // batch
        if nn < na * batch:  # the call would read past the buffer
            raise ReferencePanic("%d scalars given, batch * na = %d" % (nn, batch * na))
        tmp = None
        if isinstance(b, DeviceBuffer):
            if not flags or b.sfmt != sfmt:
                raise ReferencePanic("poly_divide: a device-resident divisor needs device-resident dividends of the same format")
            bptr, nb = b.ptr, b.n
        else:
            bptr = bytes(b) if isinstance(b, (bytes, bytearray)) else b"".join(self._host_scalar(int(x), sfmt) for x in b)
            nb = len(bptr) // 32
            if flags:  # KZG_IN_DEVICE covers both inputs
                tmp = DeviceBuffer(self, max(nb, 1), sfmt).upload(bptr) if nb else None
                bptr = tmp.ptr if tmp else None
        m, nr = (na - nb + 1 if na >= nb else 0), max(nb - 1, 0)
        ex = (ctypes.c_int * max(batch, 1))()
        try:
            if q_out is not None or r_out is not None:
                if q_out is None or r_out is None or q_out.n < batch * m or r_out.n < batch * nr or q_out.sfmt != sfmt or r_out.sfmt != sfmt:
                    raise ReferencePanic("poly_divide: q_out and r_out hold batch * (na - nb + 1) and batch * (nb - 1) scalars of the dividends' format")
                rc = self.lib.kzg_poly_divide(self.ctx, ptr, na, batch, bptr, nb, sfmt, flags | L.OUT_DEVICE, q_out.ptr, r_out.ptr, ex)
                if rc:
                    _raise(self, rc)
                return q_out, r_out, [bool(v) for v in ex[:batch]]
            qb, rb = ctypes.create_string_buffer(32 * max(batch * m, 1)), ctypes.create_string_buffer(32 * max(batch * nr, 1))
            rc = self.lib.kzg_poly_divide(self.ctx, ptr, na, batch, bptr, nb, sfmt, flags, qb, rb, ex)
            if rc:
                _raise(self, rc)
        finally:
            if tmp is not None:
                tmp.free()
        q = [self._scalar_from(qb.raw[32 * j:32 * j + 32], sfmt) for j in range(batch * m)]
        r = [self._scalar_from(rb.raw[32 * j:32 * j + 32], sfmt) for j in range(batch * nr)]
        exact = [bool(v) for v in ex[:batch]]
        if batch == 1:
            return q, r, exact
        return [q[i * m:(i + 1) * m] for i in range(batch)], [r[i * nr:(i + 1) * nr] for i in range(batch)], exact

    def quotient_eval(self, evals, i):
        blob = pack_scalars(evals)
        d = len(blob) // 32
        out = ctypes.create_string_buffer(d * 32)
        rc = self.lib.kzg_quotient_eval(self.ctx, blob, d, i, L.FR_CANONICAL, 0, out)
        if rc:
            _raise(self, rc)
        return unpack_scalars(out.raw)

    def eval_form_eval(self, evals, zs, d=None):
        """kzg_eval_form_eval: the values p_b(zs[b]) of `len(zs)` polynomials given by their evaluations over the size-d domain
        (any z in Fr, on the domain or off it).  evals: a list of evaluation lists / EvaluationDomains, or a flat list of ints / a
        canonical blob / a DeviceBuffer of len(zs) x d scalars (d then given)."""
        ptr, d, sfmt, flags, _keep = self._eval_vectors_arg(evals, len(zs), d)
        out = ctypes.create_string_buffer(32 * max(len(zs), 1))
        zb = b"".join(self._host_scalar(int(z), sfmt) for z in zs)
        rc = self.lib.kzg_eval_form_eval(self.ctx, ptr, d, len(zs), zb, sfmt, flags, out)
        if rc:
            _raise(self, rc)
        return [self._scalar_from(out.raw[32 * b:32 * b + 32], sfmt) for b in range(len(zs))]

    def fr_fold(self, vecs, d, t, gammas, out=None):
        """kzg_fr_fold: out[g d + j] = sum_{i < t} gammas[g]^i vecs[(g t + i) d + j] for len(gammas) groups of t vectors of d scalars.
        vecs: a flat list of ints, a canonical blob or a DeviceBuffer; gammas: ints in [1, R).  Returns the len(gammas) x d sums as
        ints, or `out` (a DeviceBuffer of the inputs' scalar format) when one is given."""
        groups = len(gammas)
        ptr, have, sfmt, flags, _keep = self._scalars_arg(vecs)
        if have < groups * t * d:  # the call would read past the buffer
            raise ReferencePanic("%d scalars given, groups * t * d = %d" % (have, groups * t * d))
        gb = b"".join(self._host_scalar(int(g), sfmt) if 0 < int(g) < R_MODULUS else int(g).to_bytes(32, "little") for g in gammas)
        if out is not None:
            if out.n < groups * d or out.sfmt != sfmt:
                raise ReferencePanic("fr_fold: out holds %d scalars, groups * d = %d (and has the inputs' format)" % (out.n, groups * d))
            rc = self.lib.kzg_fr_fold(self.ctx, ptr, d, t, groups, gb, sfmt, flags | L.OUT_DEVICE, out.ptr)
            if rc:
                _raise(self, rc)
            return out
        buf = ctypes.create_string_buffer(32 * max(groups * d, 1))
        rc = self.lib.kzg_fr_fold(self.ctx, ptr, d, t, groups, gb, sfmt, flags, buf)
        if rc:
            _raise(self, rc)
        return [self._scalar_from(buf.raw[32 * k:32 * k + 32], sfmt) for k in range(groups * d)]

    def _fold_groups_arg(self, groups_vecs, groups, t=None, d=None, pad=True):
        """(pointer, d, t, sfmt, flags, keep-alive) of `groups` groups of t vectors of d scalars: a list of groups, each a list of t
        vectors (lists of ints, EvaluationDomains or Polynomials), or a flat blob / DeviceBuffer (t then given)."""
        if not isinstance(groups_vecs, (DeviceBuffer, bytes, bytearray, memoryview)):
            if len(groups_vecs) != groups:
                raise ReferencePanic("one group of vectors per point")
            rows = [[v.coeffs if isinstance(v, EvaluationDomain) else (v.slice_coeffs() if isinstance(v, Polynomial) else list(v)) for v in grp]
                    for grp in groups_vecs]
            t = len(rows[0]) if rows else (t or 1)
            d = d if rows else (d or 1)
            if rows and (t == 0 or any(len(grp) != t for grp in rows)):
                raise ReferencePanic("every group holds the same number t >= 1 of vectors")
            if rows and d is None:
                d = max(len(v) for grp in rows for v in grp)
            if any(len(v) > d or (not pad and len(v) != d) for grp in rows for v in grp):
                raise ReferencePanic("a vector does not fit d = %d" % d)
            groups_vecs = [x for grp in rows for v in grp for x in list(v) + [0] * (d - len(v))]
        ptr, have, sfmt, flags, keep = self._scalars_arg(groups_vecs)
        if t is None or d is None:
            raise ReferencePanic("t and d are needed with a flat buffer")
        if have < groups * t * d:  # the call would read past the buffer
            raise ReferencePanic("%d scalars given, groups * t * d = %d" % (have, groups * t * d))
        return ptr, d, t, sfmt, flags, keep

    def _open_fold(self, fn, srs, groups_vecs, zs, gammas, ofmt, t, d, pad):
        """the body of KZGProverEvalForm.open_fold_batch and KZGProver.open_fold_batch"""
        groups = len(zs)
        if len(gammas) != groups:
            raise ReferencePanic("one challenge gamma per group")
        ptr, d, t, sfmt, flags, _keep = self._fold_groups_arg(groups_vecs, groups, t, d, pad)
        psz = L.POINT_BYTES[ofmt]
        ys = ctypes.create_string_buffer(32 * max(groups * t, 1))
        out = ctypes.create_string_buffer(psz * max(groups, 1))
        zb = b"".join(self._host_scalar(int(z), sfmt) for z in zs)
        gb = b"".join(self._host_scalar(int(g), sfmt) if 0 < int(g) < R_MODULUS else int(g).to_bytes(32, "little") for g in gammas)
        rc = fn(self.ctx, srs.handle, ptr, d, t, groups, zb, gb, sfmt, flags, ys, out, ofmt)
        if rc:
            _raise(self, rc)
        return ([[self._scalar_from(ys.raw[32 * (g * t + i):32 * (g * t + i) + 32], sfmt) for i in range(t)] for g in range(groups)],
                [out.raw[g * psz:(g + 1) * psz] for g in range(groups)])

    def _enc_scalar(self, x, sfmt):
        """a host scalar in sfmt; a value outside [0, R) goes through as it is, for the library to refuse"""
        x = int(x)
        if not 0 <= x < (1 << 256):
            raise ReferencePanic("a scalar is no 256-bit unsigned value")
        return self._host_scalar(x, sfmt) if x < R_MODULUS else x.to_bytes(32, "little")

    def fr_lincomb(self, vecs, d, idx, weights, out=None):
        """kzg_fr_lincomb: out[j] = sum_k weights[k] vecs[idx[k] d + j] for j < d.  vecs: a flat list of ints, a canonical blob or a
        DeviceBuffer of n_vecs x d scalars; idx: vector indices; weights: ints in [0, R).  Returns the d sums as ints, or `out` (a
        DeviceBuffer of the inputs' scalar format) when one is given."""
        count = len(idx)
        if len(weights) != count:
            raise ReferencePanic("fr_lincomb: one weight per index")
        ptr, have, sfmt, flags, _keep = self._scalars_arg(vecs)
        n_vecs = have // d if d else 0
        ia = (ctypes.c_uint32 * max(count, 1))(*[int(i) % (1 << 32) for i in idx])
        wb = b"".join(self._enc_scalar(w, sfmt) for w in weights)
        if out is not None:
            if out.n < d or out.sfmt != sfmt:
                raise ReferencePanic("fr_lincomb: out holds %d scalars, d = %d (and has the inputs' format)" % (out.n, d))
            rc = self.lib.kzg_fr_lincomb(self.ctx, ptr, d, n_vecs, ia, wb, count, sfmt, flags | L.OUT_DEVICE, out.ptr)
            if rc:
                _raise(self, rc)
            return out
        buf = ctypes.create_string_buffer(32 * max(d, 1))
        rc = self.lib.kzg_fr_lincomb(self.ctx, ptr, d, n_vecs, ia, wb, count, sfmt, flags, buf)
        if rc:
            _raise(self, rc)
        return [self._scalar_from(buf.raw[32 * k:32 * k + 32], sfmt) for k in range(d)]

    def batch_inverse(self, values, out=None):
        """kzg_fr_batch_inverse: 1 / v for every v of `values` (a list of ints, a canonical blob or a DeviceBuffer); a zero maps to
        zero.  Returns (inverses, zeros): the inverses as ints, or `out` (a DeviceBuffer of the inputs' scalar format, which may be
        `values` itself) when one is given, and the number of zeros met."""
        ptr, n, sfmt, flags, _keep = self._scalars_arg(values)
        zeros = ctypes.c_size_t(0)
        if out is not None:
            if out.n < n or out.sfmt != sfmt:
                raise ReferencePanic("batch_inverse: out holds %d scalars, n = %d (and has the inputs' format)" % (out.n, n))
            rc = self.lib.kzg_fr_batch_inverse(self.ctx, ptr, n, sfmt, flags | L.OUT_DEVICE, out.ptr, ctypes.byref(zeros))
            if rc:
                _raise(self, rc)
            return out, zeros.value
        buf = ctypes.create_string_buffer(32 * max(n, 1))
        rc = self.lib.kzg_fr_batch_inverse(self.ctx, ptr, n, sfmt, flags, buf, ctypes.byref(zeros))
        if rc:
            _raise(self, rc)
        return [self._scalar_from(buf.raw[32 * k:32 * k + 32], sfmt) for k in range(n)], zeros.value

    def fr_scan(self, vecs, n, op="product", exclusive=False, out=None):
        """kzg_fr_scan: the running products (op = "product") or sums ("sum") of len(vecs) / n vectors of n scalars, vector b at element
        b n; exclusive: every vector's scan starts from the identity and leaves its last element out.  vecs: a flat list of ints, a
        canonical blob or a DeviceBuffer.  Returns (out, totals): the scans as ints, or `out` (a DeviceBuffer of the inputs' scalar
        format, which may be `vecs` itself) when one is given, and every vector's total as ints."""
        ops = {"product": L.SCAN_PRODUCT, "sum": L.SCAN_SUM}
        if op not in ops:
            raise ReferencePanic("fr_scan: op is 'product' or 'sum'")
        ptr, have, sfmt, flags, _keep = self._scalars_arg(vecs)
        if n <= 0 or have % n:
            raise ReferencePanic("fr_scan: %d scalars are no whole number of vectors of n = %d" % (have, n))
        batch = have // n
        tb = ctypes.create_string_buffer(32 * max(batch, 1))
        if out is not None:
            if out.n < have or out.sfmt != sfmt:
                raise ReferencePanic("fr_scan: out holds %d scalars, batch * n = %d (and has the inputs' format)" % (out.n, have))
            rc = self.lib.kzg_fr_scan(self.ctx, ptr, n, batch, ops[op], int(bool(exclusive)), sfmt, flags | L.OUT_DEVICE, out.ptr, tb)
            if rc:
                _raise(self, rc)
            return out, [self._scalar_from(tb.raw[32 * b:32 * b + 32], sfmt) for b in range(batch)]
        buf = ctypes.create_string_buffer(32 * max(have, 1))
        rc = self.lib.kzg_fr_scan(self.ctx, ptr, n, batch, ops[op], int(bool(exclusive)), sfmt, flags, buf, tb)
        if rc:
            _raise(self, rc)
        return ([self._scalar_from(buf.raw[32 * k:32 * k + 32], sfmt) for k in range(have)],
                [self._scalar_from(tb.raw[32 * b:32 * b + 32], sfmt) for b in range(batch)])

    def prefix_product(self, vecs, n, exclusive=False, out=None):
        return self.fr_scan(vecs, n, "product", exclusive, out)

    def prefix_sum(self, vecs, n, exclusive=False, out=None):
        return self.fr_scan(vecs, n, "sum", exclusive, out)

    def grand_product(self, num, den, n, t, out=None, strict=True):
        """kzg_fr_grand_product: z[b n] = 1, z[b n + i] = prod_{k < i} prod_j num[b][j][k] / den[b][j][k] for the len(num) / (t n) vectors
        of t columns of n scalars (column j of vector b at element (b t + j) n), and every vector's total (1 for a valid permutation).
        num, den: flat lists of ints, canonical blobs or DeviceBuffers, both of one kind.  Returns (z, totals, zero_den): z as ints, or
        `out` (a DeviceBuffer of the inputs' scalar format) when one is given.  strict: a zero denominator raises; otherwise the
        vectors that hold one are flagged in zero_den and their rows and totals are zero."""
        ptr, have, sfmt, flags, _keep = self._scalars_arg(num)
        dptr, dhave, dsfmt, dflags, _dkeep = self._scalars_arg(den)
        if (sfmt, flags) != (dsfmt, dflags) or have != dhave:
            raise ReferencePanic("grand_product: num and den have one size, format and residence")
        if n <= 0 or t <= 0 or have % (t * n):
            raise ReferencePanic("grand_product: %d scalars are no whole number of vectors of t * n = %d" % (have, t * n))
        batch = have // (t * n)
        tb = ctypes.create_string_buffer(32 * max(batch, 1))
        zd = None if strict else (ctypes.c_int * max(batch, 1))()
        if out is not None:
            if out.n < batch * n or out.sfmt != sfmt:
                raise ReferencePanic("grand_product: out holds %d scalars, batch * n = %d (and has the inputs' format)" % (out.n, batch * n))
            buf, oflags = out.ptr, flags | L.OUT_DEVICE
        else:
            buf, oflags = ctypes.create_string_buffer(32 * max(batch * n, 1)), flags
        rc = self.lib.kzg_fr_grand_product(self.ctx, ptr, dptr, n, t, batch, sfmt, oflags, buf, tb, zd)
        if rc:
            _raise(self, rc)
        z = out if out is not None else [self._scalar_from(buf.raw[32 * k:32 * k + 32], sfmt) for k in range(batch * n)]
        return z, [self._scalar_from(tb.raw[32 * b:32 * b + 32], sfmt) for b in range(batch)], [0] * batch if zd is None else [int(v) for v in zd[:batch]]

    def lookup_table(self, table):
        """kzg_lookup_setup: a LookupTable over `table` (a list of ints, a canonical blob or a DeviceBuffer)."""
        return LookupTable(self, table)

    def logup_terms(self, values, n, t, beta, table=None, mult=None, out=None, strict=True):
        """kzg_logup_terms: out[b n + i] = sum_{j < t} 1 / (beta + values[b][j][i]) - mult[b][i] / (beta + table[i]) for the
        len(values) / (t n) vectors of t columns of n scalars (column j of vector b at element (b t + j) n; with t = 0 the batch is
        len(mult) / n).  values, table, mult: flat lists of ints, canonical blobs or DeviceBuffers, all of one kind; table and mult
        may both be None.  Returns (terms, zero_den): the terms as ints, or `out` (a DeviceBuffer of the inputs' scalar format) when
        one is given.  strict: a zero denominator raises; otherwise the vectors that hold one are flagged and their rows are zero."""
        if (table is None) != (mult is None):
            raise ReferencePanic("logup_terms: table and mult go together")
        if n <= 0 or t < 0 or (t == 0 and table is None):
            raise ReferencePanic("logup_terms: n >= 1, and columns or a table")
        args = [self._scalars_arg(x) if x is not None else None for x in ((values if t else None), table, mult)]
        kinds = {(a[2], a[3]) for a in args if a is not None}
        if len(kinds) != 1:
            raise ReferencePanic("logup_terms: values, table and mult have one format and residence")
        (sfmt, flags), = kinds
        have = args[0][1] if t else args[2][1]
        per = t * n if t else n
        if have % per or (table is not None and (args[1][1] != n or args[2][1] * per != have * n)):
            raise ReferencePanic("logup_terms: the sizes are no whole number of vectors of t = %d columns of n = %d" % (t, n))
        batch = have // per
        zd = None if strict else (ctypes.c_int * max(batch, 1))()
        if out is not None:
            if out.n < batch * n or out.sfmt != sfmt:
                raise ReferencePanic("logup_terms: out holds %d scalars, batch * n = %d (and has the inputs' format)" % (out.n, batch * n))
            buf, oflags = out.ptr, flags | L.OUT_DEVICE
        else:
            buf, oflags = ctypes.create_string_buffer(32 * max(batch * n, 1)), flags
        ptrs = [a[0] if a is not None else None for a in args]
        rc = self.lib.kzg_logup_terms(self.ctx, ptrs[0], ptrs[1], ptrs[2], self._enc_scalar(beta, sfmt), n, t, batch, sfmt, oflags, buf, zd)
        if rc:
            _raise(self, rc)
        terms = out if out is not None else [self._scalar_from(buf.raw[32 * k:32 * k + 32], sfmt) for k in range(batch * n)]
        return terms, [0] * batch if zd is None else [int(v) for v in zd[:batch]]

    def logup_accumulator(self, plan, table, columns, beta):
        """The logUp argument of `columns` (t lists of n ints each) against `table` (n ints, the rows `plan` was set up from), without
        the data leaving the device between the three calls: the multiplicities m of the table rows among all t n values
        (kzg_lookup_count; every value must be in the table), the terms sum_j 1 / (beta + columns[j][i]) - m_i / (beta + table[i])
        (kzg_logup_terms) and their exclusive running sum (kzg_fr_scan).  Returns (m, accumulator, total) as ints; total is 0."""
        n, t = len(table), len(columns)
        if t == 0 or any(len(c) != n for c in columns) or len(plan) != n:
            raise ReferencePanic("logup_accumulator: t >= 1 columns of len(table) values, and a plan over the table")
        bufs = [DeviceBuffer(self, n).upload(pack_scalars(table)), DeviceBuffer(self, t * n).upload(pack_scalars([x for c in columns for x in c])),
                DeviceBuffer(self, n), DeviceBuffer(self, n)]
        try:
            d_table, d_cols, d_m, d_acc = bufs
            plan.count(d_cols, out=d_m, strict=True)
            self.logup_terms(d_cols, n, t, beta, table=d_table, mult=d_m, out=d_acc)
            _, totals = self.fr_scan(d_acc, n, "sum", True, out=d_acc)
            return unpack_scalars(d_m.download()), unpack_scalars(d_acc.download()), totals[0]
        finally:
            for b in bufs:
                b.free()

    def fr_program(self, program, n_cols=None, n_consts=None, n_out=None):
        """kzg_fr_program_setup: a FrProgram from a kzg_amd.frp.Compiled (frp.compile([...])), or from a flat list of instruction
        words with the three sizes."""
        return FrProgram(self, program, n_cols, n_consts, n_out)

    def _columns_arg(self, cols, what):
        """(pointer array, elements per column, sfmt, flags, keep-alive) of a set of columns of one length, format and residence"""
        args = [self._scalars_arg(c) for c in cols]
        kinds = {(a[1], a[2], a[3]) for a in args}
        if len(kinds) != 1:
            raise ReferencePanic("%s: the columns have one length, format and residence" % what)
        n, sfmt, flags = kinds.pop()
        cp = (ctypes.c_void_p * len(args))(*[ctypes.cast(a[0], ctypes.c_void_p) for a in args])
        return cp, n, sfmt, flags, args

    def mle_eq(self, point, sfmt=L.FR_CANONICAL, out=None):
        """kzg_mle_eq: the table eq(point, .) of 2^m values, point[j] for variable j (bit j of the index).  Returns ints, or `out` (a
        DeviceBuffer of 2^m scalars, whose format then counts) when one is given."""
        m = len(point)
        sfmt = out.sfmt if out is not None else sfmt
        if out is not None and out.n < (1 << m):
            raise ReferencePanic("mle_eq: out holds %d scalars, 2^m = %d" % (out.n, 1 << m))
        pb = b"".join(self._enc_scalar(u, sfmt) for u in point) or None
        buf = None if out is not None else ctypes.create_string_buffer(32 << m)
        rc = self.lib.kzg_mle_eq(self.ctx, pb, m, sfmt, L.OUT_DEVICE if out is not None else 0, out.ptr if out is not None else buf)
        if rc:
            _raise(self, rc)
        return out if out is not None else [self._scalar_from(buf.raw[32 * k:32 * k + 32], sfmt) for k in range(1 << m)]

    def mle_bind(self, cols, rho, outs=None):
        """kzg_mle_bind: every column (n scalars each, n a power of two; all lists of ints or canonical blobs, or all DeviceBuffers of
        one format) folded at its top variable, lo + rho (hi - lo).  Host columns: returns one list of n / 2 ints per column.
        DeviceBuffers: folded IN PLACE (the first n / 2 scalars; the rest stay) unless `outs` gives one buffer of n / 2 scalars per
        column; returns the buffers that hold the results."""
        cp, n, sfmt, flags, keep = self._columns_arg(cols, "mle_bind")
        rb = self._enc_scalar(rho, sfmt)
        if flags & L.IN_DEVICE:
            dst = list(cols) if outs is None else list(outs)
            if len(dst) != len(cols) or any(o.sfmt != sfmt or o.n < n // 2 for o in dst):
                raise ReferencePanic("mle_bind: one output of n / 2 scalars in the columns' format per column")
            op = (ctypes.c_void_p * len(dst))(*[o.ptr.value for o in dst])
            rc = self.lib.kzg_mle_bind(self.ctx, cp, len(cols), n, rb, sfmt, flags | L.OUT_DEVICE, op)
            if rc:
                _raise(self, rc)
            return dst
        if outs is not None:
            raise ReferencePanic("mle_bind: outs go with device columns")
        bufs = [ctypes.create_string_buffer(16 * max(n, 2)) for _ in cols]
        op = (ctypes.c_void_p * max(len(bufs), 1))(*[ctypes.cast(b, ctypes.c_void_p) for b in bufs])
        rc = self.lib.kzg_mle_bind(self.ctx, cp, len(cols), n, rb, sfmt, flags, op)
        if rc:
            _raise(self, rc)
        return [[self._scalar_from(b.raw[32 * k:32 * k + 32], sfmt) for k in range(n // 2)] for b in bufs]

    def mle_eval(self, tables, point, batch=1, quotients=False):
        """kzg_mle_eval: f_b(point) for `batch` tables of 2^m scalars each (m = len(point)), contiguous: a list of ints, a canonical
        blob or a DeviceBuffer.  Returns the values, or (values, quotients) with quotients=True: per table the n - 1 Zeromorph
        quotient values, q_k at [2^k - 1, 2^(k + 1) - 1)."""
        m = len(point)
        n = 1 << m
        ptr, have, sfmt, flags, _keep = self._scalars_arg(tables)
        if have < batch * n:
            raise ReferencePanic("mle_eval: %d scalars are fewer than batch x 2^m = %d" % (have, batch * n))
        pb = b"".join(self._enc_scalar(u, sfmt) for u in point) or None
        ys = ctypes.create_string_buffer(32 * max(batch, 1))
        qb = ctypes.create_string_buffer(32 * max(batch * (n - 1), 1)) if quotients else None
        rc = self.lib.kzg_mle_eval(self.ctx, ptr, m, batch, pb, sfmt, flags, ys, qb)
        if rc:
            _raise(self, rc)
        vals = [self._scalar_from(ys.raw[32 * b:32 * b + 32], sfmt) for b in range(batch)]
        if not quotients:
            return vals
        return vals, [[self._scalar_from(qb.raw[32 * k:32 * k + 32], sfmt) for k in range(b * (n - 1), (b + 1) * (n - 1))] for b in range(batch)]

    def sumcheck_round(self, plan, cols, consts=(), n_eval=None):
        """kzg_sumcheck_round: for every output o of `plan` (a FrProgram without rotations) the sums over the pairs (i, i + n / 2) of
        the output at X = 0 .. n_eval - 1 (default: the largest degree + 1).  Returns one list of n_eval ints per output."""
        return plan.sumcheck_round(cols, consts, n_eval)

    def _multiopen_vectors_arg(self, vecs, length, pad):
        """(pointer, length, n_polys, sfmt, flags, keep-alive) of the polynomials of a multiopen call: a list of vectors (lists of ints,
        EvaluationDomains or Polynomials; with `pad` filled with zeros to the longest) or a flat blob / DeviceBuffer (length given)"""
        if not isinstance(vecs, (DeviceBuffer, bytes, bytearray, memoryview)):
            rows = [v.coeffs if isinstance(v, EvaluationDomain) else (v.slice_coeffs() if isinstance(v, Polynomial) else list(v)) for v in vecs]
            if length is None:
                length = max([len(v) for v in rows] + [1])
            if any(len(v) > length or (not pad and len(v) != length) for v in rows):
                raise ReferencePanic("a vector does not fit the length %d" % length)
            vecs = [x for v in rows for x in list(v) + [0] * (length - len(v))]
        ptr, have, sfmt, flags, keep = self._scalars_arg(vecs)
        if not length:
            raise ReferencePanic("the length of the vectors is needed with a flat buffer")
        return ptr, length, have // length, sfmt, flags, keep

    @staticmethod
    def _index_arg(poly_idx, count):
        if poly_idx is None:
            return None
        if len(poly_idx) != count:
            raise ReferencePanic("one polynomial index per claim")
        return (ctypes.c_uint32 * max(count, 1))(*[int(i) % (1 << 32) for i in poly_idx])

    def _multiopen_commit(self, fn, srs, vecs, length, glen_of, pad, zs, r, poly_idx, ofmt):
        """the body of multiopen_commit of both provers -> (ys, g, D); g: ints, or a DeviceBuffer when the polynomials are one"""
        count = len(zs)
        ptr, length, n_polys, sfmt, flags, _keep = self._multiopen_vectors_arg(vecs, length, pad)
        glen = glen_of(length)
        ys = ctypes.create_string_buffer(32 * max(count, 1))
        out = ctypes.create_string_buffer(L.POINT_BYTES[ofmt])
        zb = b"".join(self._enc_scalar(z, sfmt) for z in zs)
        g_dev = DeviceBuffer(self, max(glen, 1), sfmt) if flags & L.IN_DEVICE else None
        g_host = None if g_dev else ctypes.create_string_buffer(32 * max(glen, 1))
        rc = fn(self.ctx, srs.handle, ptr, length, n_polys, self._index_arg(poly_idx, count), zb, count, self._enc_scalar(r, sfmt), sfmt, flags, ys,
                g_dev.ptr if g_dev else g_host, out, ofmt)
        if rc:
            if g_dev:
                g_dev.free()
            _raise(self, rc)
        g = g_dev if g_dev else [self._scalar_from(g_host.raw[32 * j:32 * j + 32], sfmt) for j in range(glen)]
        return [self._scalar_from(ys.raw[32 * k:32 * k + 32], sfmt) for k in range(count)], g, out.raw

    def _multiopen_finish(self, fn, srs, vecs, length, glen_of, pad, zs, r, t, g, poly_idx, ofmt):
        """the body of multiopen_finish of both provers -> (pi, v(t))"""
        count = len(zs)
        ptr, length, n_polys, sfmt, flags, _keep = self._multiopen_vectors_arg(vecs, length, pad)
        glen = glen_of(length)
        if isinstance(g, DeviceBuffer) != bool(flags & L.IN_DEVICE):
            raise ReferencePanic("multiopen_finish: g lives where the polynomials live (host lists, or DeviceBuffers)")
        if isinstance(g, DeviceBuffer):
            if g.n < glen or g.sfmt != sfmt:
                raise ReferencePanic("multiopen_finish: g holds %d scalars of format %d, the call needs %d of format %d" % (g.n, g.sfmt, glen, sfmt))
            gp = g.ptr
        else:
            if len(g) != glen:
                raise ReferencePanic("multiopen_finish: g has %d scalars, the call needs %d" % (len(g), glen))
            gp = pack_scalars(g) + bytes(32)
        y = ctypes.create_string_buffer(32)
        out = ctypes.create_string_buffer(L.POINT_BYTES[ofmt])
        zb = b"".join(self._enc_scalar(z, sfmt) for z in zs)
        rc = fn(self.ctx, srs.handle, ptr, length, n_polys, self._index_arg(poly_idx, count), zb, count, self._enc_scalar(r, sfmt),
                self._enc_scalar(t, sfmt), gp, sfmt, flags, y, out, ofmt)
        if rc:
            _raise(self, rc)
        return out.raw, self._scalar_from(y.raw, sfmt)

    def _multiopen(self, commit, finish, vecs, zs, r, challenge_t, poly_idx, ofmt, **kw):
        ys, g, D = commit(vecs, zs, r, poly_idx, ofmt, **kw)
        try:
            t = challenge_t(D)  # t is drawn AFTER D exists: the caller's hash of D (and of whatever else the protocol binds)
            pi, _ = finish(vecs, zs, r, t, g, poly_idx, ofmt, **kw)
        finally:
            if isinstance(g, DeviceBuffer):
                g.free()
        return ys, D, pi, t

    def _eval_vectors_arg(self, evals, batch, d=None):
        """(pointer, d, sfmt, flags, keep-alive) of `batch` evaluation vectors, stride d"""
        if not isinstance(evals, (DeviceBuffer, bytes, bytearray, memoryview)) and len(evals) and not isinstance(evals[0], int):
            vecs = [ev.coeffs if isinstance(ev, EvaluationDomain) else list(ev) for ev in evals]
            if len(vecs) != batch or any(len(v) != len(vecs[0]) for v in vecs):
                raise ReferencePanic("one evaluation vector per point, all of one length")
            d = len(vecs[0])
            evals = [v for vec in vecs for v in vec]
        ptr, have, sfmt, flags, keep = self._scalars_arg(evals)
        if d is None:
            d = have // max(batch, 1)
        if have < batch * d:  # the call would read past the buffer
            raise ReferencePanic("%d scalars given, batch * d = %d" % (have, batch * d))
        return ptr, d, sfmt, flags, keep

    def recover_cosets(self, log_n, log_l, n, coset_ids, cells, want_evals=False):
        """kzg_recover_cosets for one polynomial: the Polynomial of n coefficients whose values on coset coset_ids[j] (the points
        of FK20CosetPlan.coset_points) are cells[j]; with want_evals also its 2^log_n evaluations in natural domain order.
        cells: a list of `known` lists of l ints, a canonical blob or a DeviceBuffer.  Raises PointNotOnPolynomial if the cells
        are not the values of such a polynomial, ReferencePanic on a shape the call rejects."""
        if not isinstance(cells, (DeviceBuffer, bytes, bytearray, memoryview)):
            cells = [v for cell in cells for v in cell]
        res = self.recover_cosets_batch(log_n, log_l, n, coset_ids, cells, 1, want_evals)
        return (res[0][0], res[1][0]) if want_evals else res[0]

    def recover_cosets_batch(self, log_n, log_l, n, coset_ids, cells, batch=None, want_evals=False):
        """`batch` polynomials over one id set.  cells: a list of polynomials (each a list of `known` lists of l ints), or a flat
        list of ints / a canonical blob / a DeviceBuffer of batch x known x l scalars (batch then given).  Returns the list of
        Polynomials, and with want_evals the pair (polynomials, list of evaluation lists)."""
        ids = [int(i) for i in coset_ids]
        known = len(ids)
        if batch is None:
            batch = len(cells)
            cells = [v for poly in cells for cell in poly for v in cell]
        if n < 0 or batch < 0 or not 0 <= log_l <= log_n <= 22:
            raise ReferencePanic("recover_cosets: 0 <= log_l <= log_n <= 22, n >= 0 and batch >= 0")
        ptr, have, sfmt, flags, _keep = self._scalars_arg(cells)
        if have < (batch * known) << log_l:  # the call would read past the buffer
            raise ReferencePanic("recover_cosets: %d scalars given, batch * known * l = %d" % (have, (batch * known) << log_l))
        N = 1 << log_n
        id_arr = (ctypes.c_size_t * max(known, 1))(*[i % (1 << 64) for i in ids])
        coeffs = ctypes.create_string_buffer(32 * max(n * batch, 1))
        evals = ctypes.create_string_buffer(32 * max(N * batch, 1)) if want_evals else None
        rc = self.lib.kzg_recover_cosets(self.ctx, log_n, log_l, n, id_arr, known, ptr, batch, sfmt, flags, coeffs, evals, None)
        if rc:
            _raise(self, rc)
        conv = (lambda b: [self._scalar_from(b[i:i + 32], sfmt) for i in range(0, len(b), 32)]) if sfmt == L.FR_MONT else unpack_scalars
        polys = [Polynomial.new_from_coeffs(conv(coeffs.raw[b * n * 32:(b + 1) * n * 32]), n - 1) for b in range(batch)]
        if not want_evals:
            return polys
        return polys, [conv(evals.raw[b * N * 32:(b + 1) * N * 32]) for b in range(batch)]

    _MONT_R = (1 << 256) % R_MODULUS

    def _host_scalar(self, x, sfmt):
        x %= R_MODULUS
        if sfmt == L.FR_MONT:
            x = x * self._MONT_R % R_MODULUS
        return x.to_bytes(32, "little")

    def _scalar_from(self, b, sfmt):
        v = int.from_bytes(b, "little")
        if sfmt == L.FR_MONT:
            v = v * pow(self._MONT_R, -1, R_MODULUS) % R_MODULUS
        return v


def compute_omega(d):
    """EvaluationDomain::compute_omega (src/ft.rs:55-76) -> (m, exp, omega)."""
    lib = L.load()
    m, exp, w = ctypes.c_size_t(), ctypes.c_uint32(), ctypes.create_string_buffer(32)
    rc = lib.kzg_compute_omega(d, ctypes.byref(m), ctypes.byref(exp), w, L.FR_CANONICAL)
    if rc:
        _raise(None, rc)
    return m.value, exp.value, int.from_bytes(w.raw, "little")


class Srs:
    """A resident G1 SRS (kzg_srs)."""

    def __init__(self, engine, handle):
        self.engine, self.handle = engine, handle

    def __len__(self):
        return self.engine.lib.kzg_srs_len(self.handle)

    def table_rows(self):
        return self.engine.lib.kzg_srs_table_rows(self.handle)

    def window_info(self):
        c, w = ctypes.c_int(), ctypes.c_int()
        self.engine.lib.kzg_srs_window_info(self.handle, ctypes.byref(c), ctypes.byref(w))
        return c.value, w.value

    def download(self, offset=0, n=None):
        n = len(self) - offset if n is None else n
        out = ctypes.create_string_buffer(96 * max(n, 1))
        rc = self.engine.lib.kzg_srs_download_g1(self.engine.ctx, self.handle, offset, n, out, L.G1_AFFINE_MONT)
        if rc:
            _raise(self.engine, rc)
        return out.raw[: 96 * n]

    def dft(self, inverse=False):
        """A new Srs holding the group DFT (kzg_ntt_g1) of these points; len(self) must be a power of two.  The inverse of a monomial
        SRS is its Lagrange basis (compute_lagrange_basis), the forward transform goes back."""
        n = len(self)
        assert n and n & (n - 1) == 0, "the DFT needs a power-of-two number of points"
        return Srs.upload(self.engine, self.engine.ntt_g1(self.download(), n.bit_length() - 1, 1, inverse), n)

    def free(self):
        if self.handle:
            self.engine.lib.kzg_srs_free(self.engine.ctx, self.handle)
            self.handle = None

    @staticmethod
    def upload(engine, blob, n, pfmt=L.G1_AFFINE_MONT):
        h = ctypes.c_void_p()
        assert len(blob) == n * L.POINT_BYTES[pfmt]
        rc = engine.lib.kzg_srs_upload_g1(engine.ctx, blob, n, pfmt, ctypes.byref(h))
        if rc:
            _raise(engine, rc)
        return Srs(engine, h)


class PointTree:
    """SubProductTree (src/polynomial.rs:303-365) as a device-resident plan (kzg_point_tree): the sub-product tree of a point set,
    kept between calls.  Evaluation of polynomials at all its points, linear_mod_combination, interpolation and the product
    polynomial each take O(k log^2 k) field products."""

    def __init__(self, engine, xs):
        self.engine, self.handle = engine, None
        self.xs = [int(x) for x in xs]
        xb = b"".join(x.to_bytes(32, "little") if 0 <= x < (1 << 256) else pack_scalars([x]) for x in self.xs)
        h = ctypes.c_void_p()
        rc = engine.lib.kzg_point_tree_setup(engine.ctx, xb, len(self.xs), L.FR_CANONICAL, ctypes.byref(h))
        if rc:
            _raise(engine, rc)
        self.handle = h

    @staticmethod
    def new_from_points(engine, xs):  # :310-327
        return PointTree(engine, xs)

    def shape(self):
        """(k, padded size, bytes the plan holds in HBM, distinct)."""
        k, padded, nbytes, distinct = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_int()
        rc = self.engine.lib.kzg_point_tree_shape(self.handle, ctypes.byref(k), ctypes.byref(padded), ctypes.byref(nbytes), ctypes.byref(distinct))
        if rc:
            _raise(self.engine, rc)
        return k.value, padded.value, nbytes.value, bool(distinct.value)

    def __len__(self):
        return len(self.xs)

    @property
    def product(self):
        """tree.product: M = prod (X - x_i), a Polynomial of degree k."""
        k = len(self.xs)
        out = ctypes.create_string_buffer(32 * (k + 1))
        rc = self.engine.lib.kzg_point_tree_product(self.engine.ctx, self.handle, L.FR_CANONICAL, 0, out)
        if rc:
            _raise(self.engine, rc)
        return Polynomial.new_from_coeffs(unpack_scalars(out.raw), k)

    def eval_batch(self, coeffs, n=None, batch=1, out=None):
        """kzg_point_tree_eval: the values p_b(xs[i]) of `batch` polynomials of n coefficients each (coeffs: ints, a canonical blob or
        a DeviceBuffer of batch x n scalars back to back).  Returns a list of `batch` lists of k ints -- one flat list for
        batch = 1 -- or `out` (a DeviceBuffer of batch x k scalars in the coefficients' format) when one is given."""
        e = self.engine
        ptr, nn, sfmt, flags, _keep = e._scalars_arg(coeffs)
        if n is None:
            if batch < 1 or nn % batch:
                raise ReferencePanic("%d scalars are not %d polynomials of equal length" % (nn, batch))
            n = nn // batch
        if nn < n * batch:  # the call would read past the buffer
            raise ReferencePanic("%d scalars given, batch * n = %d" % (nn, batch * n))
        k = len(self.xs)
        if out is not None:
            if out.n < batch * k or out.sfmt != sfmt:
                raise ReferencePanic("PointTree.eval_batch: out holds %d scalars, batch * k = %d (and has the coefficients' format)" % (out.n, batch * k))
            rc = e.lib.kzg_point_tree_eval(e.ctx, self.handle, ptr, n, batch, sfmt, flags | L.OUT_DEVICE, out.ptr)
            if rc:
                _raise(e, rc)
            return out
        buf = ctypes.create_string_buffer(32 * max(batch * k, 1))
        rc = e.lib.kzg_point_tree_eval(e.ctx, self.handle, ptr, n, batch, sfmt, flags, buf)
        if rc:
            _raise(e, rc)
        ys = [e._scalar_from(buf.raw[32 * j:32 * j + 32], sfmt) for j in range(batch * k)]
        return ys if batch == 1 else [ys[b * k:(b + 1) * k] for b in range(batch)]

    def eval(self, f):  # :329-348, without its panic on a zero remainder
        """The values of the Polynomial (or coefficient list) f at the tree's points."""
        return self.eval_batch(f.slice_coeffs() if isinstance(f, Polynomial) else f)

    def _vectors(self, fn, vs):
        k = len(self.xs)
        many = len(vs) > 0 and isinstance(vs[0], (list, tuple))
        rows = [list(v) for v in vs] if many else [list(vs)]
        if any(len(v) != k for v in rows):
            raise ReferencePanic("assert_eq!(xs.len(), ys.len())")
        out = ctypes.create_string_buffer(32 * max(len(rows) * k, 1))
        rc = fn(self.engine.ctx, self.handle, pack_scalars([c for v in rows for c in v]), len(rows), L.FR_CANONICAL, 0, out)
        if rc:
            _raise(self.engine, rc)
        cs = unpack_scalars(out.raw[: 32 * len(rows) * k])
        return [cs[b * k:(b + 1) * k] for b in range(len(rows))] if many else cs

    def linear_mod_combination(self, cs):  # :350-364
        """sum_i cs[i] M / (X - x_i) as a Polynomial (a list of value vectors gives a list of Polynomials)."""
        res = self._vectors(self.engine.lib.kzg_point_tree_combine, cs)
        return [Polynomial(r) for r in res] if res and isinstance(res[0], list) else Polynomial(res)

    def interpolate(self, ys):
        """kzg_point_tree_interpolate: the k coefficients (lowest first) of the polynomial of degree < k through (xs[i], ys[i]); a list
        of value vectors gives a list of coefficient lists.  One point gives the constant."""
        return self._vectors(self.engine.lib.kzg_point_tree_interpolate, ys)

    def create_witness_batch(self, srs, coeffs, n=None, batch=1, ys=None, ofmt=L.G1_AFFINE_MONT, with_status=False):
        """kzg_witness_coeff_tree: `batch` polynomials of n coefficients each (coeffs: ints, a canonical blob or a DeviceBuffer of
        batch x n scalars back to back) opened at the tree's points against the SRS `srs`.  Returns (witnesses, remainders): `batch`
        point blobs in ofmt and `batch` lists of k ints, r_b = p_b mod M zero-padded (the interpolant through the values).  ys
        (optional: batch x k claimed values, flat, of the coefficients' kind): a claim that fails raises KZGError, or with
        with_status=True a third element is returned, the list of `batch` status words (0 or KZG_ERR_POINT_NOT_ON_POLY)."""
        e = self.engine
        ptr, nn, sfmt, flags, _keep = e._scalars_arg(coeffs)
        if n is None:
            if batch < 1 or nn % batch:
                raise ReferencePanic("%d scalars are not %d polynomials of equal length" % (nn, batch))
            n = nn // batch
        if nn < n * batch:  # the call would read past the buffer
            raise ReferencePanic("%d scalars given, batch * n = %d" % (nn, batch * n))
        k = len(self.xs)
        yptr = None
        if ys is not None:
            yptr, yn, ysf, yfl, _ykeep = e._scalars_arg(ys)
            if yn < batch * k or (yfl, ysf) != (flags, sfmt):
                raise ReferencePanic("create_witness_batch: ys must be batch x k scalars of the coefficients' kind")
        psz = L.POINT_BYTES[ofmt]
        out_w, out_r = ctypes.create_string_buffer(psz * max(batch, 1)), ctypes.create_string_buffer(32 * max(batch * k, 1))
        st = (ctypes.c_int * max(batch, 1))()
        rc = e.lib.kzg_witness_coeff_tree(e.ctx, srs.handle, self.handle, ptr, n, batch, yptr, sfmt, flags, out_w, ofmt, out_r,
                                          st if with_status else None)
        if rc:
            _raise(e, rc)
        ws = [out_w.raw[i * psz:(i + 1) * psz] for i in range(batch)]
        rs = [[e._scalar_from(out_r.raw[32 * (b * k + j):32 * (b * k + j) + 32], sfmt) for j in range(k)] for b in range(batch)]
        return (ws, rs, list(st[:batch])) if with_status else (ws, rs)

    def create_witness(self, srs, polynomial, ys=None, ofmt=L.G1_AFFINE_MONT):
        """One polynomial opened at the tree's points: a KZGBatchWitness (r = p mod M, w = [p / M]_1); ys: its claimed values."""
        ws, rs = self.create_witness_batch(srs, polynomial.slice_coeffs(), ys=ys, ofmt=ofmt)
        return KZGBatchWitness(Polynomial(rs[0]), ws[0])

    def close(self):
        if self.handle:
            self.engine.lib.kzg_point_tree_free(self.engine.ctx, self.handle)
            self.handle = None

    free = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


class LookupTable:
    """A table of scalars prepared for membership queries (kzg_lookup): its keys and an open-addressing hash table over them in HBM,
    kept between calls.  The table may hold duplicates; a value's owner is the lowest row that holds it."""

    def __init__(self, engine, table):
        self.engine, self.handle = engine, None
        ptr, n_t, sfmt, flags, _keep = engine._scalars_arg(table)
        h = ctypes.c_void_p()
        rc = engine.lib.kzg_lookup_setup(engine.ctx, ptr, n_t, sfmt, flags, ctypes.byref(h))
        if rc:
            _raise(engine, rc)
        self.handle = h

    def shape(self):
        """(rows, distinct residues, bytes the plan holds in HBM)."""
        n_t, distinct, nbytes = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
        rc = self.engine.lib.kzg_lookup_shape(self.handle, ctypes.byref(n_t), ctypes.byref(distinct), ctypes.byref(nbytes))
        if rc:
            _raise(self.engine, rc)
        return n_t.value, distinct.value, nbytes.value

    def __len__(self):
        return self.shape()[0]

    def count(self, values, n=None, out=None, strict=False):
        """kzg_lookup_count: `values` (a flat list of ints, a canonical blob or a DeviceBuffer) is len(values) / n vectors of n scalars
        (one vector by default).  Returns (multiplicities, indices, missing, first_missing): per vector the number of values each
        row owns -- ints, or `out` (a DeviceBuffer of batch x rows scalars in the values' format) when one is given --, every
        value's owner row (None for a value that is not in the table; no indices at all with `out`), how many values are not in
        the table and the position of the first of them (None if there is none).  strict: a missing value raises."""
        eng = self.engine
        ptr, have, sfmt, flags, _keep = eng._scalars_arg(values)
        n = have if n is None else n
        if n <= 0 or have % n:
            raise ReferencePanic("lookup count: %d scalars are no whole number of vectors of n = %d" % (have, n))
        batch, n_t = have // n, len(self)
        miss, first = (ctypes.c_size_t * batch)(), (ctypes.c_size_t * batch)()
        report = (None, None) if strict else (miss, first)
        if out is not None:
            if out.n < batch * n_t or out.sfmt != sfmt:
                raise ReferencePanic("lookup count: out holds %d scalars, batch * rows = %d (and has the values' format)" % (out.n, batch * n_t))
            rc = eng.lib.kzg_lookup_count(eng.ctx, self.handle, ptr, n, batch, sfmt, flags | L.OUT_DEVICE, out.ptr, None, *report)
            mults, idx = out, None
        else:
            mb, ib = ctypes.create_string_buffer(32 * batch * n_t), (ctypes.c_uint32 * have)()
            rc = eng.lib.kzg_lookup_count(eng.ctx, self.handle, ptr, n, batch, sfmt, flags, mb, ib, *report)
            mults = [eng._scalar_from(mb.raw[32 * k:32 * k + 32], sfmt) for k in range(batch * n_t)]
            idx = [None if v == 0xFFFFFFFF else int(v) for v in ib]
        if rc:
            _raise(eng, rc)
        return mults, idx, [int(v) for v in miss], [None if v == (1 << (8 * ctypes.sizeof(ctypes.c_size_t))) - 1 else int(v) for v in first] if not strict else [None] * batch

    def free(self):
        if self.handle:
            self.engine.lib.kzg_lookup_free(self.engine.ctx, self.handle)
            self.handle = None

    close = free

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()
        return False


class FrProgram:
    """A straight-line program over Fr (kzg_fr_program), validated once and run for every row of a set of columns in one pass: the
    constraint expressions of a quotient round.  The words come from kzg_amd.frp.compile or are written by hand (frp.insn)."""

    def __init__(self, engine, program, n_cols=None, n_consts=None, n_out=None):
        self.engine, self.handle = engine, None
        if hasattr(program, "words"):
            words, n_cols, n_consts, n_out = program.words, program.n_cols, program.n_consts, program.n_out
        else:
            words = list(program)
        if None in (n_cols, n_consts, n_out) or len(words) % L.FRP_WORDS:
            raise ReferencePanic("fr_program: whole instructions of %d words, and n_cols, n_consts, n_out" % L.FRP_WORDS)
        arr = (ctypes.c_uint32 * max(len(words), 1))(*[int(w) & 0xFFFFFFFF for w in words])
        h = ctypes.c_void_p()
        rc = engine.lib.kzg_fr_program_setup(engine.ctx, arr, len(words) // L.FRP_WORDS, n_cols, n_consts, n_out, ctypes.byref(h))
        if rc:
            _raise(engine, rc)
        self.handle = h

    def shape(self):
        """(instructions, columns, consts, outputs, temporaries in use, multiplications)"""
        v = [ctypes.c_size_t() for _ in range(6)]
        rc = self.engine.lib.kzg_fr_program_shape(self.handle, *[ctypes.byref(x) for x in v])
        if rc:
            _raise(self.engine, rc)
        return tuple(x.value for x in v)

    def run(self, cols, consts=(), n=None, outs=None):
        """kzg_fr_program_run over rows 0 .. n - 1 (n: the longest column by default).  cols: one entry per column, all lists of ints
        (or canonical blobs) or all DeviceBuffers of one scalar format; a column holds n elements, or a power of two that divides n
        (periodic).  consts: ints in [0, R).  Returns one list of n ints per output, or `outs` (one DeviceBuffer of the columns'
        format per output) when given."""
        eng = self.engine
        _, n_cols, n_consts, n_out, _, _ = self.shape()
        if len(cols) != n_cols or len(consts) != n_consts or (outs is not None and len(outs) != n_out):
            raise ReferencePanic("fr_program: the plan takes %d columns and %d consts and writes %d outputs" % (n_cols, n_consts, n_out))
        args = [eng._scalars_arg(c) for c in cols]
        kinds = {(a[2], a[3]) for a in args}
        if len(kinds) > 1:
            raise ReferencePanic("fr_program: the columns have one format and residence")
        sfmt, flags = kinds.pop() if kinds else ((outs[0].sfmt if outs is not None else L.FR_CANONICAL), 0)
        if outs is not None and any(o.sfmt != sfmt for o in outs):
            raise ReferencePanic("fr_program: outs have the columns' format")
        n = max([a[1] for a in args], default=0) if n is None else n
        if outs is not None and any(o.n < n for o in outs):
            raise ReferencePanic("fr_program: an output buffer is shorter than n = %d" % n)
        cp = (ctypes.c_void_p * max(n_cols, 1))(*[ctypes.cast(a[0], ctypes.c_void_p) for a in args])
        cl = (ctypes.c_size_t * max(n_cols, 1))(*[a[1] for a in args])
        kb = b"".join(eng._enc_scalar(k, sfmt) for k in consts) or None
        bufs = None if outs is not None else [ctypes.create_string_buffer(32 * max(n, 1)) for _ in range(n_out)]
        op = (ctypes.c_void_p * n_out)(*[ctypes.cast(b, ctypes.c_void_p) for b in (bufs or [o.ptr for o in outs])])
        rc = eng.lib.kzg_fr_program_run(eng.ctx, self.handle, cp, cl, kb, n, sfmt, flags | (L.OUT_DEVICE if outs is not None else 0), op)
        if rc:
            _raise(eng, rc)
        if outs is not None:
            return outs
        return [[eng._scalar_from(b.raw[32 * k:32 * k + 32], sfmt) for k in range(n)] for b in bufs]

    def degrees(self):
        """kzg_fr_program_degree: per output an upper bound of its total degree in the columns (a sumcheck needs degree + 1 points)"""
        n_out = self.shape()[3]
        d = (ctypes.c_size_t * n_out)()
        rc = self.engine.lib.kzg_fr_program_degree(self.handle, d)
        if rc:
            _raise(self.engine, rc)
        return [int(x) for x in d]

    def sumcheck_round(self, cols, consts=(), n_eval=None):
        """Engine.sumcheck_round"""
        eng = self.engine
        _, n_cols, n_consts, n_out, _, _ = self.shape()
        if len(cols) != n_cols or len(consts) != n_consts:
            raise ReferencePanic("sumcheck_round: the plan takes %d columns and %d consts" % (n_cols, n_consts))
        n_eval = max(self.degrees()) + 1 if n_eval is None else n_eval
        if n_cols:
            cp, n, sfmt, flags, _keep = eng._columns_arg(cols, "sumcheck_round")
        else:
            raise ReferencePanic("sumcheck_round: a plan without columns has no rows")
        kb = b"".join(eng._enc_scalar(k, sfmt) for k in consts) or None
        sums = ctypes.create_string_buffer(32 * max(n_out * n_eval, 1))
        rc = eng.lib.kzg_sumcheck_round(eng.ctx, self.handle, cp, kb, n, n_eval, sfmt, flags, sums)
        if rc:
            _raise(eng, rc)
        return [[eng._scalar_from(sums.raw[32 * k:32 * k + 32], sfmt) for k in range(o * n_eval, (o + 1) * n_eval)] for o in range(n_out)]

    def free(self):
        if self.handle:
            self.engine.lib.kzg_fr_program_free(self.engine.ctx, self.handle)
            self.handle = None

    close = free

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()
        return False


class _Fk20Handle:
    """What FK20Plan and FK20CosetPlan share: the opaque handle from the kind's setup entry point and its release."""
    _setup = _free = None  # names of the two entry points

    def __init__(self, engine, srs, *shape):
        self.engine = engine
        h = ctypes.c_void_p()
        rc = getattr(engine.lib, self._setup)(engine.ctx, srs.handle, *shape, ctypes.byref(h))
        if rc:
            _raise(engine, rc)
        self.handle = h

    def free(self):
        if self.handle:
            getattr(self.engine.lib, self._free)(self.engine.ctx, self.handle)
            self.handle = None


class FK20Plan(_Fk20Handle):
    """kzg_fk20: the per-domain tables of FK20 (every opening of a polynomial over its size-2^log_n domain in one call) for one
    monomial SRS.  Not a reference type."""
    _setup, _free = "kzg_fk20_setup", "kzg_fk20_free"

    def __init__(self, engine, srs, log_n):
        super().__init__(engine, srs, log_n)

    def domain(self):
        return self.engine.lib.kzg_fk20_domain(self.handle)


def _witness_all(engine, fn, plan, blob, n, batch, ofmt):
    N = plan.domain()
    psz = L.POINT_BYTES[ofmt]
    out = ctypes.create_string_buffer(psz * N * max(batch, 1))
    rc = fn(engine.ctx, plan.handle, blob, n, batch, L.FR_CANONICAL, 0, out, ofmt)
    if rc:
        _raise(engine, rc)
    return [[out.raw[(b * N + m) * psz:(b * N + m + 1) * psz] for m in range(N)] for b in range(batch)]


class FK20CosetPlan(_Fk20Handle):
    """kzg_fk20_cosets: the per-domain tables of multi-point FK20 (every opening of a polynomial at every coset of 2^log_l points
    of its size-2^log_n domain in one call) for one monomial SRS.  Coset i is {w^(i + tK) : t < l}, K = N / l.  Not a reference
    type."""

    _setup, _free = "kzg_fk20_cosets_setup", "kzg_fk20_cosets_free"

    def __init__(self, engine, srs, log_n, log_l):
        super().__init__(engine, srs, log_n, log_l)
        self._shape = None

    def _dims(self):
        if self._shape is None:
            N, l = ctypes.c_size_t(), ctypes.c_size_t()
            rc = self.engine.lib.kzg_fk20_cosets_shape(self.handle, ctypes.byref(N), ctypes.byref(l))
            if rc:
                _raise(self.engine, rc)
            self._shape = (N.value, l.value)
        return self._shape

    def domain(self):
        return self._dims()[0]

    def coset_size(self):
        return self._dims()[1]

    def num_cosets(self):
        N, l = self._dims()
        return N // l

    def coset_points(self, i):
        """the l points of coset i, in the order t = 0 .. l-1: w^(i + tK)"""
        N, l = self._dims()
        K = N // l
        w = compute_omega(N)[2]
        return [pow(w, i + t * K, R_MODULUS) for t in range(l)]


def _witness_cosets(engine, fn, plan, blob, n, batch, ofmt):
    N, l = plan.domain(), plan.coset_size()
    K = N // l
    psz = L.POINT_BYTES[ofmt]
    out = ctypes.create_string_buffer(psz * K * max(batch, 1))
    rbuf = ctypes.create_string_buffer(32 * N * max(batch, 1))
    rc = fn(engine.ctx, plan.handle, blob, n, batch, L.FR_CANONICAL, 0, out, ofmt, rbuf)
    if rc:
        _raise(engine, rc)
    res = []
    for b in range(batch):
        ws = []
        for i in range(K):
            r = unpack_scalars(rbuf.raw[((b * K + i) * l) * 32:((b * K + i + 1) * l) * 32])
            ws.append(KZGBatchWitness(Polynomial.new_from_coeffs(r, l - 1), out.raw[(b * K + i) * psz:(b * K + i + 1) * psz]))
        res.append(ws)
    return res


class CosetVerifier:
    """kzg_cosets_verifier: bulk verification of coset openings for one KZGParams (gs and hs), one domain 2^log_n and one coset
    size 2^log_l (<= 256): the fixed-base window table of gs[0 .. l), the stored Miller lines of hs[0] and hs[l] and the powers of
    w.  Coset i is FK20CosetPlan.coset_points(i).  Not a reference type."""

    def __init__(self, engine, params, log_n, log_l):
        self.engine = engine
        if params.hs is None:
            raise ReferencePanic("KZGParams.hs is empty (index out of bounds)")
        h = ctypes.c_void_p()
        rc = engine.lib.kzg_cosets_verifier_setup(engine.ctx, params.gs.handle, params.hs.handle, log_n, log_l, ctypes.byref(h))
        if rc:
            _raise(engine, rc)
        self.handle = h
        N, l, tb = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
        engine.lib.kzg_cosets_verifier_shape(h, ctypes.byref(N), ctypes.byref(l), ctypes.byref(tb))
        self._shape = (N.value, l.value, tb.value)

    def domain(self):
        return self._shape[0]

    def coset_size(self):
        return self._shape[1]

    def table_bytes(self):
        return self._shape[2]

    def free(self):
        if self.handle:
            self.engine.lib.kzg_cosets_verifier_free(self.engine.ctx, self.handle)
            self.handle = None

    def verify(self, commitments, commitment_idx, coset_ids, cells, proofs, pfmt=L.G1_AFFINE_MONT):
        """One verdict per cell.  Cell k: commitments[commitment_idx[k]], coset coset_ids[k], proof proofs[k] (bytes in pfmt) and
        its l values.  cells: a list of cells (each a list of l ints), or a flat list of ints / a canonical blob / a DeviceBuffer
        of len(proofs) x l scalars.  Raises EngineError on a malformed point, ReferencePanic on a shape the call rejects."""
        e = self.engine
        count = len(proofs)
        if len(commitment_idx) != count or len(coset_ids) != count:
            raise ReferencePanic("verify_cosets: one commitment index, coset id and proof per cell")
        if not isinstance(cells, (DeviceBuffer, bytes, bytearray, memoryview)) and len(cells) and isinstance(cells[0], (list, tuple)):
            cells = [v for cell in cells for v in cell]
        ptr, have, sfmt, flags, _keep = e._scalars_arg(cells)
        if have < count * self.coset_size():  # the call would read past the buffer
            raise ReferencePanic("verify_cosets: %d scalars given, count * l = %d" % (have, count * self.coset_size()))
        idx = (ctypes.c_uint32 * max(count, 1))(*[int(i) % (1 << 32) for i in commitment_idx])
        ids = (ctypes.c_size_t * max(count, 1))(*[int(i) % (1 << 64) for i in coset_ids])
        ok = ctypes.create_string_buffer(max(count, 1))
        rc = e.lib.kzg_verify_cosets(e.ctx, self.handle, b"".join(commitments), len(commitments), idx, ids, ptr, b"".join(proofs), count,
                                     sfmt, pfmt, flags, ok)
        if rc:
            _raise(e, rc)
        return [bool(b) for b in ok.raw[:count]]

    def verify_batch(self, commitments, commitment_idx, coset_ids, cells, proofs, r=None, pfmt=L.G1_AFFINE_MONT):
        """kzg_verify_cosets_batch: True iff ALL the cells verify, from one pairing check of their combination with the weights
        r^k.  The arguments of verify(); r: the challenge, an int in [1, R).  r=None draws it here with `secrets` -- sound because it
        is drawn after the cells were handed over; a protocol that needs a reproducible verdict passes the hash of all inputs.
        False says nothing about which cell is bad: verify() does (verify_with_fallback)."""
        e = self.engine
        count = len(proofs)
        if len(commitment_idx) != count or len(coset_ids) != count:
            raise ReferencePanic("verify_cosets_batch: one commitment index, coset id and proof per cell")
        if not isinstance(cells, (DeviceBuffer, bytes, bytearray, memoryview)) and len(cells) and isinstance(cells[0], (list, tuple)):
            cells = [v for cell in cells for v in cell]
        ptr, have, sfmt, flags, _keep = e._scalars_arg(cells)
        if have < count * self.coset_size():  # the call would read past the buffer
            raise ReferencePanic("verify_cosets_batch: %d scalars given, count * l = %d" % (have, count * self.coset_size()))
        if r is None:
            r = secrets.randbelow(R_MODULUS - 1) + 1
        if not 0 <= int(r) < (1 << 256):
            raise ReferencePanic("verify_cosets_batch: the challenge r must be in [1, R)")
        r = int(r)
        if sfmt == L.FR_MONT and r < R_MODULUS:  # the challenge travels in the scalar format of the cells (0 and r >= R: the call's error)
            r = r * (1 << 256) % R_MODULUS
        idx = (ctypes.c_uint32 * max(count, 1))(*[int(i) % (1 << 32) for i in commitment_idx])
        ids = (ctypes.c_size_t * max(count, 1))(*[int(i) % (1 << 64) for i in coset_ids])
        ok = ctypes.c_int(-1)
        rc = e.lib.kzg_verify_cosets_batch(e.ctx, self.handle, b"".join(commitments), len(commitments), idx, ids, ptr, b"".join(proofs),
                                           count, r.to_bytes(32, "little"), sfmt, pfmt, flags, ctypes.byref(ok))
        if rc:
            _raise(e, rc)
        return bool(ok.value)

    def verify_with_fallback(self, commitments, commitment_idx, coset_ids, cells, proofs, r=None, pfmt=L.G1_AFFINE_MONT):
        """One verdict per cell, as verify(): the batch check first, and the per-cell checks only when it says no."""
        if self.verify_batch(commitments, commitment_idx, coset_ids, cells, proofs, r, pfmt):
            return [True] * len(proofs)
        return self.verify(commitments, commitment_idx, coset_ids, cells, proofs, pfmt)


class SrsG2:
    """Resident G2 points (kzg_srs_g2): the `hs` half of KZGParams or a G2 Lagrange basis."""

    def __init__(self, engine, handle):
        self.engine, self.handle = engine, handle

    def __len__(self):
        return self.engine.lib.kzg_srs_g2_len(self.handle)

    def download(self, offset=0, n=None, pfmt=L.G2_AFFINE_MONT):
        n = len(self) - offset if n is None else n
        sz = L.G2_POINT_BYTES[pfmt]
        out = ctypes.create_string_buffer(sz * max(n, 1))
        rc = self.engine.lib.kzg_srs_download_g2(self.engine.ctx, self.handle, offset, n, out, pfmt)
        if rc:
            _raise(self.engine, rc)
        return out.raw[: sz * n]

    def msm(self, scalars, offset=0, ofmt=L.G2_AFFINE_MONT):
        """G2Projective::multi_exp(&hs[offset..offset+len], scalars) (call site src/coeff_form.rs:156)"""
        blob = pack_scalars(scalars)
        out = ctypes.create_string_buffer(L.G2_POINT_BYTES[ofmt])
        rc = self.engine.lib.kzg_msm_g2(self.engine.ctx, self.handle, offset, blob, len(blob) // 32, L.FR_CANONICAL, out, ofmt)
        if rc:
            _raise(self.engine, rc)
        return out.raw

    def msm_bucket(self, scalars, offset=0, n=None, ofmt=L.G2_AFFINE_MONT):
        """kzg_msm_g2_bucket: the same group element (the same bytes) by the bucket method, for large n; scalars: a list of ints, a blob
        of canonical scalars or a DeviceBuffer in either format."""
        ptr, nn, sfmt, flags, _keep = self.engine._scalars_arg(scalars)
        n = nn if n is None else n
        out = ctypes.create_string_buffer(L.G2_POINT_BYTES[ofmt])
        rc = self.engine.lib.kzg_msm_g2_bucket(self.engine.ctx, self.handle, offset, ptr, n, sfmt, flags, out, ofmt)
        if rc:
            _raise(self.engine, rc)
        return out.raw

    def dft(self, inverse=False):
        """A new SrsG2 holding the group DFT (kzg_ntt_g2) of these points; len(self) must be a power of two, at most 2^20."""
        n = len(self)
        assert n and n & (n - 1) == 0, "the DFT needs a power-of-two number of points"
        return SrsG2.upload(self.engine, self.engine.ntt_g2(self.download(), n.bit_length() - 1, 1, inverse), n)

    def free(self):
        if self.handle:
            self.engine.lib.kzg_srs_g2_free(self.engine.ctx, self.handle)
            self.handle = None

    @staticmethod
    def upload(engine, blob, n, pfmt=L.G2_AFFINE_MONT):
        h = ctypes.c_void_p()
        assert len(blob) == n * L.G2_POINT_BYTES[pfmt]
        rc = engine.lib.kzg_srs_upload_g2(engine.ctx, blob, n, pfmt, ctypes.byref(h))
        if rc:
            _raise(engine, rc)
        return SrsG2(engine, h)


class KZGParams:
    """src/lib.rs:14-19: gs = [s^i]G (resident G1 SRS), hs = [s^i]H (resident G2 points; None if not generated)."""

    def __init__(self, gs, hs=None):
        self.gs, self.hs = gs, hs


def setup_g2(engine, s, n):
    """the hs half of setup() (src/lib.rs:48-52): hs[i] = [s^i]H for i < n."""
    h = ctypes.c_void_p()
    rc = engine.lib.kzg_srs_setup_g2(engine.ctx, (s % R_MODULUS).to_bytes(32, "little"), L.FR_CANONICAL, n, ctypes.byref(h))
    if rc:
        _raise(engine, rc)
    return SrsG2(engine, h)


def setup_lagrange_g2(engine, s, d):
    """lagrange_basis_h for a known secret: same elements as compute_lagrange_basis(&setup(s, d)).1."""
    h = ctypes.c_void_p()
    rc = engine.lib.kzg_srs_setup_lagrange_g2(engine.ctx, (s % R_MODULUS).to_bytes(32, "little"), L.FR_CANONICAL, d,
                                              ctypes.byref(h))
    if rc:
        _raise(engine, rc)
    return SrsG2(engine, h)


def setup(engine, s, num_coeffs, g2_len=None):
    """setup(s, num_coeffs) (src/lib.rs:38-55): gs[i] = [s^i]G and hs[i] = [s^i]H, generated on the GPU.
    The reference always builds num_coeffs G2 powers; only the verifier reads them (hs[0], hs[1], and hs[..k+1] for a
    k-point batched opening), so `g2_len` caps that half (default min(num_coeffs, 257): enough for 256-point batches;
    pass g2_len=num_coeffs for the reference's full vector, 0 to skip it)."""
    h = ctypes.c_void_p()
    rc = engine.lib.kzg_srs_setup_g1(engine.ctx, (s % R_MODULUS).to_bytes(32, "little"), L.FR_CANONICAL, num_coeffs,
                                     ctypes.byref(h))
    if rc:
        _raise(engine, rc)
    if g2_len is None:
        g2_len = min(num_coeffs, 257)
    return KZGParams(Srs(engine, h), setup_g2(engine, s, g2_len) if g2_len else None)


def setup_shard(engine, s, first, n):
    """gs[first .. first+n) of setup(s, first+n): the contiguous SRS shard one rank holds."""
    h = ctypes.c_void_p()
    rc = engine.lib.kzg_srs_setup_g1_shard(engine.ctx, (s % R_MODULUS).to_bytes(32, "little"), L.FR_CANONICAL, first, n,
                                           ctypes.byref(h))
    if rc:
        _raise(engine, rc)
    return Srs(engine, h)


def setup_lagrange(engine, s, d):
    """lagrange_basis_g for a known secret: same elements as compute_lagrange_basis(&setup(s, d)).0."""
    h = ctypes.c_void_p()
    rc = engine.lib.kzg_srs_setup_lagrange_g1(engine.ctx, (s % R_MODULUS).to_bytes(32, "little"), L.FR_CANONICAL, d,
                                              ctypes.byref(h))
    if rc:
        _raise(engine, rc)
    return Srs(engine, h)


def compute_lagrange_basis(params):
    """compute_lagrange_basis (src/eval_form.rs:254-280), G1 half, from the monomial SRS."""
    e = params.gs.engine
    h = ctypes.c_void_p()
    rc = e.lib.kzg_srs_lagrange_from_monomial_g1(e.ctx, params.gs.handle, ctypes.byref(h))
    if rc:
        _raise(e, rc)
    return Srs(e, h)


def compute_lagrange_basis_g2(params):
    """compute_lagrange_basis (src/eval_form.rs:254-280), G2 half, from hs alone (hs must hold all d powers).  Any power-of-two d up
    to 2^20: sizes from 2048 on (option "g2_lagrange_dft_from") run the G2 inverse DFT, smaller ones one d-term sum per row; with
    compute_lagrange_basis this gives KZGVerifierEvalForm its two bases from a ceremony SRS, with no secret."""
    e = params.gs.engine
    if params.hs is None:
        raise ReferencePanic("KZGParams.hs is empty")
    h = ctypes.c_void_p()
    rc = e.lib.kzg_srs_lagrange_from_monomial_g2(e.ctx, params.hs.handle, ctypes.byref(h))
    if rc:
        _raise(e, rc)
    return SrsG2(e, h)


class ShardedSrs:
    """An SRS sharded contiguously over a DeviceGroup (kzg_msrs)."""

    def __init__(self, group, handle):
        self.group, self.handle = group, handle

    def __len__(self):
        return self.group.lib.kzg_msrs_len(self.handle)

    def shard(self, local_index=0):
        """(Srs view of the resident shard of local GPU `local_index`, index of its first point); owned by this object."""
        first = ctypes.c_size_t()
        h = self.group.lib.kzg_msrs_shard(self.handle, local_index, ctypes.byref(first))
        return Srs(self.group.engine(local_index), ctypes.c_void_p(h)), first.value

    def free(self):
        if self.handle:
            self.group.lib.kzg_msrs_free(self.group.handle, self.handle)
            self.handle = None


class DeviceGroup:
    """kzg_mctx: a group of GPUs holding a sharded SRS; partial commitments are combined over RCCL inside the library.
    DeviceGroup(devices=[0, 1, ...]) -- one process drives all of them;
    DeviceGroup.for_rank(device, rank, world, unique_id) -- one process per GPU (unique_id from DeviceGroup.unique_id()
    on rank 0, distributed by the host)."""

    def __init__(self, devices=(0,), _handle=None):
        self.lib = L.load()
        if _handle is None:
            self._host_env()
            arr = (ctypes.c_int * len(devices))(*devices)
            h = ctypes.c_void_p()
            rc = self.lib.kzg_mctx_create(arr, len(devices), ctypes.byref(h))
            if rc:
                raise EngineError(f"kzg_mctx_create({list(devices)}) failed with {rc}: {self._create_error(self.lib)} "
                                  "(kzg_amd has no CPU fallback)")
            _handle = h
            self._flush_c_stdio()
        self.handle = _handle
        self._engines = {}
        self._flushed = False

    @staticmethod
    def _flush_c_stdio():
        """RCCL prints its version banner (NCCL_DEBUG=VERSION, exported on some images) with printf: into a pipe or file that is
        block-buffered and would surface at process exit, after whatever the host printed last.  Flush it where it was caused."""
        try:
            ctypes.CDLL(None).fflush(None)
        except (OSError, AttributeError):
            pass

    @staticmethod
    def _host_env():
        """This module is the host: the one-node RCCL knobs go into the environment before the first RCCL call."""
        from .distributed import single_node_rccl_env
        return single_node_rccl_env()

    @staticmethod
    def _create_error(lib):
        return (lib.kzg_mctx_create_error() or b"").decode()

    @staticmethod
    def _node_local(single_node):
        """single_node=None (default): the world is taken to live on this node unless the launcher says otherwise -- MASTER_ADDR set and
        not a loopback address.  A world that spans nodes must NOT get the loopback bootstrap knobs (NCCL_SOCKET_IFNAME=lo,
        NCCL_IB_DISABLE=1, NCCL_NET_PLUGIN=none): with them it cannot form its communicator and just meets the formation deadline
        (ADVICE r5).  Pass single_node=False (or export KZG_RCCL_SINGLE_NODE_ENV=0) there and bring your own NCCL_* environment."""
        if single_node is not None:
            return bool(single_node)
        addr = os.environ.get("MASTER_ADDR", "")
        return addr in ("", "localhost") or addr.startswith("127.") or addr == "::1"

    @staticmethod
    def unique_id(single_node=None):
        lib = L.load()
        if DeviceGroup._node_local(single_node):
            DeviceGroup._host_env()
        buf = ctypes.create_string_buffer(128)
        rc = lib.kzg_mctx_unique_id(buf)
        if rc:
            raise EngineError(f"kzg_mctx_unique_id failed with {rc}: {DeviceGroup._create_error(lib)}")
        return buf.raw

    @staticmethod
    def for_rank(device, rank, world, unique_id, single_node=None):
        """One process per GPU.  The one-node RCCL environment is applied only when the world is node-local (_node_local)."""
        lib = L.load()
        if DeviceGroup._node_local(single_node):
            DeviceGroup._host_env()
        h = ctypes.c_void_p()
        rc = lib.kzg_mctx_create_rank(device, rank, world, unique_id, ctypes.byref(h))
        if rc:
            raise EngineError(f"kzg_mctx_create_rank(device={device}, rank={rank}/{world}) failed with {rc}: "
                              f"{DeviceGroup._create_error(lib)}")
        DeviceGroup._flush_c_stdio()
        return DeviceGroup(_handle=h)

    def last_error(self):
        return (self.lib.kzg_mctx_last_error(self.handle) or b"").decode()

    def _check(self, rc):
        # the communicator is formed inside the first call that needs it: RCCL's banner is flushed ONCE, after the first call that
        # succeeded -- not a dlopen and a flush of all the host's stdio on every group call
        if not self._flushed:
            if rc == 0:
                self._flushed = True
            self._flush_c_stdio()
        if rc:
            _raise(self, rc)

    @property
    def world(self):
        return self.lib.kzg_mctx_world(self.handle)

    @property
    def local_count(self):
        return self.lib.kzg_mctx_local_count(self.handle)

    def rank(self, local_index=0):
        return self.lib.kzg_mctx_rank(self.handle, local_index)

    def engine(self, local_index=0):
        """The single-GPU Engine of a local GPU (borrowed: closed with the group)."""
        if local_index not in self._engines:
            e = Engine.__new__(Engine)
            e.lib = self.lib
            e.ctx = ctypes.c_void_p(self.lib.kzg_mctx_ctx(self.handle, local_index))
            e.device = None
            e._borrowed = True
            self._engines[local_index] = e
        return self._engines[local_index]

    def set_option(self, key, value):
        self._check(self.lib.kzg_mctx_set_option(self.handle, key.encode(), value))

    def setup(self, s, n):
        """setup(s, n).gs sharded over the group (src/lib.rs:38-47)."""
        h = ctypes.c_void_p()
        self._check(self.lib.kzg_srs_setup_g1_sharded(self.handle, (s % R_MODULUS).to_bytes(32, "little"), L.FR_CANONICAL, n,
                                                      ctypes.byref(h)))
        return ShardedSrs(self, h)

    def upload(self, blob, n, pfmt=L.G1_AFFINE_MONT):
        assert len(blob) == n * L.POINT_BYTES[pfmt]
        h = ctypes.c_void_p()
        self._check(self.lib.kzg_srs_upload_g1_sharded(self.handle, blob, n, pfmt, ctypes.byref(h)))
        return ShardedSrs(self, h)

    def commit(self, srs, coeffs, ofmt=L.G1_AFFINE_MONT):
        """KZGProver::commit over the group; coeffs: ints / canonical blob (host)."""
        blob = pack_scalars(coeffs)
        return self.commit_batch(srs, blob, len(blob) // 32, 1, ofmt=ofmt)[0]

    def commit_batch(self, srs, coeffs, n, batch, ofmt=L.G1_AFFINE_MONT, sfmt=L.FR_CANONICAL):
        """coeffs: host blob of batch * n scalars, or a list of DeviceBuffer (one per local GPU, [batch][shard] slices)."""
        psz = L.POINT_BYTES[ofmt]
        out = ctypes.create_string_buffer(psz * max(batch, 1))
        if isinstance(coeffs, (list, tuple)) and coeffs and isinstance(coeffs[0], DeviceBuffer):
            ptrs = (ctypes.c_void_p * len(coeffs))(*[c.ptr.value for c in coeffs])
            rc = self.lib.kzg_commit_coeff_sharded_batch(self.handle, srs.handle, ptrs, n, batch, coeffs[0].sfmt, L.IN_DEVICE, out, ofmt)
        else:
            blob = pack_scalars(coeffs)
            assert len(blob) == 32 * n * batch
            rc = self.lib.kzg_commit_coeff_sharded_batch(self.handle, srs.handle, blob, n, batch, sfmt, 0, out, ofmt)
        self._check(rc)
        return [out.raw[i * psz:(i + 1) * psz] for i in range(batch)]

    def _whole_poly_arg(self, coeffs):
        """host blob / ints, or a list of DeviceBuffer (one per local GPU, each the WHOLE polynomial)"""
        if isinstance(coeffs, (list, tuple)) and coeffs and isinstance(coeffs[0], DeviceBuffer):
            ptrs = (ctypes.c_void_p * len(coeffs))(*[c.ptr.value for c in coeffs])
            return ptrs, coeffs[0].n, coeffs[0].sfmt, L.IN_DEVICE
        blob = pack_scalars(coeffs)
        return blob, len(blob) // 32, L.FR_CANONICAL, 0

    def create_witness(self, srs, coeffs, point, ofmt=L.G1_AFFINE_MONT):
        """KZGProver::create_witness over the group (replicated quotient, sharded MSM)."""
        arg, n, sfmt, flags = self._whole_poly_arg(coeffs)
        x, y = point
        conv = (lambda v: (v % R_MODULUS).to_bytes(32, "little")) if sfmt == L.FR_CANONICAL else (lambda v: (v * FR_MONT_R % R_MODULUS).to_bytes(32, "little"))
        out = ctypes.create_string_buffer(L.POINT_BYTES[ofmt])
        self._check(self.lib.kzg_witness_coeff_sharded(self.handle, srs.handle, arg, n, conv(x), conv(y), sfmt, flags, out, ofmt))
        return out.raw

    def create_witness_batched(self, srs, coeffs, points, ofmt=L.G1_AFFINE_MONT):
        """KZGProver::create_witness_batched over the group: (witness bytes, interpolant coefficients)."""
        arg, n, sfmt, flags = self._whole_poly_arg(coeffs)
        k = len(points)
        conv = (lambda v: (v % R_MODULUS).to_bytes(32, "little")) if sfmt == L.FR_CANONICAL else (lambda v: (v * FR_MONT_R % R_MODULUS).to_bytes(32, "little"))
        xs = b"".join(conv(p[0]) for p in points)
        ys = b"".join(conv(p[1]) for p in points)
        out = ctypes.create_string_buffer(L.POINT_BYTES[ofmt])
        rbuf = ctypes.create_string_buffer(32 * max(k, 2))
        rlen = ctypes.c_size_t()
        self._check(self.lib.kzg_witness_coeff_batched_sharded(self.handle, srs.handle, arg, n, xs, ys, k, sfmt, flags, out, ofmt,
                                                               rbuf, ctypes.byref(rlen)))
        r = unpack_scalars(rbuf.raw[:32 * rlen.value])
        if sfmt != L.FR_CANONICAL:
            rinv = pow(FR_MONT_R, -1, R_MODULUS)
            r = [v * rinv % R_MODULUS for v in r]
        return out.raw, r

    def create_witness_eval(self, lagrange_srs, evals, index, ofmt=L.G1_AFFINE_MONT):
        """KZGProverEvalForm::create_witness over the group (src/eval_form.rs:124-140): replicated div_by_omega_i, sharded MSM
        against the Lagrange-basis SRS `lagrange_srs` (DeviceGroup.upload of the basis)."""
        arg, d, sfmt, flags = self._whole_poly_arg(evals)
        out = ctypes.create_string_buffer(L.POINT_BYTES[ofmt])
        self._check(self.lib.kzg_witness_eval_sharded(self.handle, lagrange_srs.handle, arg, d, index, sfmt, flags, out, ofmt))
        return out.raw

    def info(self):
        """which RCCL / HIP runtime the group runs on and what forming its communicator cost (kzg_mctx_info)"""
        buf = ctypes.create_string_buffer(2048)
        self._check(self.lib.kzg_mctx_info(self.handle, buf, 2048))
        return buf.value.decode()

    def formation(self):
        """{'formation_ms': f, 'load': .., 'uid': .., 'init': .., 'first_exchange': .., 'destroy': ..} parsed from info() (ms; -1 =
        has not happened)"""
        import re
        s = self.info()
        d = {"formation_ms": float(re.search(r"formation_ms=(-?[0-9.]+)", s).group(1))}
        for k, v in re.findall(r"(load|uid|init|first_exchange|destroy)=(-?[0-9.]+)", s):
            d[k] = float(v)
        return d

    def close(self):
        if self.handle:
            self.lib.kzg_mctx_destroy(self.handle)
            self.handle = None
            for e in self._engines.values():
                e.ctx = None


class Polynomial:
    """src/polynomial.rs:24-27: dense coefficients + explicit degree."""

    def __init__(self, coeffs, degree=None):
        self.coeffs = [int(c) % R_MODULUS for c in coeffs]
        if degree is None:  # Polynomial::new (:83-87) via compute_degree (:94-105)
            degree = len(self.coeffs) - 1
            while degree > 0 and self.coeffs[degree] == 0:
                degree -= 1
        self.degree = degree

    @staticmethod
    def new_from_coeffs(coeffs, degree):
        return Polynomial(coeffs, degree)

    def num_coeffs(self):  # :135-137
        return self.degree + 1

    def slice_coeffs(self):  # :148-150
        return self.coeffs[: self.num_coeffs()]

    def eval(self, engine, x):  # :156-165
        return engine.poly_eval(self.slice_coeffs(), x)

    def multi_eval(self, engine, xs):  # :229-233
        if len(xs) <= self.degree:
            raise ReferencePanic("assert!(xs.len() > self.degree())")
        return engine.poly_multi_eval(self.slice_coeffs(), xs)

    @staticmethod
    def lagrange_interpolation(engine, xs, ys):  # :266-293
        if len(xs) != len(ys):
            raise ReferencePanic("assert_eq!(xs.len(), ys.len())")
        if len(xs) == 1:  # :269-272: the reference returns X + (y - x) for one point
            return Polynomial.new_from_coeffs([(int(ys[0]) - int(xs[0])) % R_MODULUS, 1], 1)
        return Polynomial(engine.interpolate(xs, ys))

    @staticmethod
    def lagrange_interpolation_with_tree(engine, xs, ys, tree):  # :237-264; tree = PointTree.new_from_points(engine, xs)
        if len(xs) != len(ys):
            raise ReferencePanic("assert_eq!(xs.len(), ys.len())")
        if len(xs) == 1:  # :244-247: X + (y - x) for one point
            return Polynomial.new_from_coeffs([(int(ys[0]) - int(xs[0])) % R_MODULUS, 1], 1)
        if len(tree) != len(xs):
            raise ReferencePanic("lagrange_interpolation_with_tree: the tree was built from another point set")
        return Polynomial(tree.interpolate(ys))

    def fft_mul(self, engine, other):  # :167-183 (and best_mul :185-191: the product is the same polynomial)
        coeffs = engine.poly_mul(self.slice_coeffs(), other.slice_coeffs())
        return Polynomial(coeffs)  # From<EvaluationDomain> = Polynomial::new (src/ft.rs:27-31)

    best_mul = fft_mul

    @staticmethod
    def new_zero():  # :49-54
        return Polynomial([0], 0)

    def is_zero(self):  # :45-47
        return self.degree == 0 and self.coeffs[0] == 0

    def long_division(self, engine, divisor):  # :193-227 -> (quotient, remainder or None)
        if self.is_zero():
            return Polynomial.new_zero(), None
        if divisor.is_zero():
            raise ReferencePanic("divisor must not be zero!")
        if self.degree < divisor.degree:
            return Polynomial.new_zero(), Polynomial(list(self.coeffs), self.degree)
        q, r, exact = engine.poly_divide(self.slice_coeffs(), divisor.slice_coeffs())
        quotient = Polynomial.new_from_coeffs(q, self.degree - divisor.degree)
        # the reference's remainder keeps the dividend's vector with its degree shrunk (:204-222): Polynomial() fixes the degree up
        return quotient, (None if exact[0] else Polynomial(r))

    def __eq__(self, other):  # :29-40
        return self.degree == other.degree and all(a == b for a, b in zip(self.coeffs, other.coeffs))


class EvaluationDomain:
    """src/ft.rs:17-25"""

    def __init__(self, coeffs, d, exp, omega):
        self.coeffs, self.d, self.exp, self.omega = [int(c) % R_MODULUS for c in coeffs], d, exp, omega

    @staticmethod
    def from_coeffs(coeffs):  # :94-109
        m, exp, omega = compute_omega(len(coeffs))
        coeffs = list(coeffs) + [0] * (m - len(coeffs))
        return EvaluationDomain(coeffs, m, exp, omega)

    def __len__(self):
        return len(self.coeffs)

    def fft(self, engine):  # :111-113
        self.coeffs = engine.ntt(self.coeffs, self.exp, inverse=False)

    def ifft(self, engine):  # :115-140
        self.coeffs = engine.ntt(self.coeffs, self.exp, inverse=True)

    def coset_fft(self, engine):  # :168-171
        self.coeffs = engine.coset_ntt(self.coeffs, self.exp, inverse=False)

    def icoset_fft(self, engine):  # :173-178
        self.coeffs = engine.coset_ntt(self.coeffs, self.exp, inverse=True)

    @staticmethod
    def _many(engine, domains, coset, inverse):
        domains = list(domains)
        if len({d.exp for d in domains}) > 1 or len({len(d.coeffs) for d in domains}) > 1:
            raise ValueError("the domains of one batched transform must have one size")
        if not domains:
            return
        fn = engine.coset_ntt_batch if coset else engine.ntt_batch
        for d, c in zip(domains, fn([d.coeffs for d in domains], domains[0].exp, inverse=inverse)):
            d.coeffs = c

    @staticmethod
    def fft_many(engine, domains):
        """fft of every domain (all of one size) in one kzg_ntt_fr_batch call; not a reference method"""
        EvaluationDomain._many(engine, domains, False, False)

    @staticmethod
    def ifft_many(engine, domains):
        EvaluationDomain._many(engine, domains, False, True)

    @staticmethod
    def coset_fft_many(engine, domains):
        EvaluationDomain._many(engine, domains, True, False)

    @staticmethod
    def icoset_fft_many(engine, domains):
        EvaluationDomain._many(engine, domains, True, True)

    def z(self, tau):  # :182-187
        out = ctypes.create_string_buffer(32)
        rc = L.load().kzg_domain_z(len(self.coeffs), (tau % R_MODULUS).to_bytes(32, "little"), L.FR_CANONICAL, out)
        if rc:
            _raise(None, rc)
        return int.from_bytes(out.raw, "little")

    def _vec(self, engine, fn, other=None):
        buf = ctypes.create_string_buffer(pack_scalars(self.coeffs), 32 * len(self.coeffs))
        if other is None:
            rc = fn(engine.ctx, buf, self.exp, L.FR_CANONICAL, 0)
        else:
            if len(other.coeffs) != len(self.coeffs):
                raise ReferencePanic("assert_eq!(self.coeffs.len(), other.coeffs.len())")
            rc = fn(engine.ctx, buf, pack_scalars(other.coeffs), len(self.coeffs), L.FR_CANONICAL, 0)
        if rc:
            _raise(engine, rc)
        self.coeffs = unpack_scalars(buf.raw)

    def divide_by_z_on_coset(self, engine):  # :192-217
        self._vec(engine, engine.lib.kzg_divide_by_z_on_coset)

    def mul_assign(self, engine, other):  # :220-244
        self._vec(engine, engine.lib.kzg_fr_vec_mul, other)

    def sub_assign(self, engine, other):  # :247-271
        self._vec(engine, engine.lib.kzg_fr_vec_sub, other)


class KZGBatchWitness:
    """src/coeff_form.rs:12-35"""

    def __init__(self, r, w):
        self.r, self.w = r, w

    def elem(self):
        return self.w

    def polynomial(self):
        return self.r


class KZGProver:
    """src/coeff_form.rs:37-112"""

    def __init__(self, parameters):
        self.parameters = parameters
        self.engine = parameters.gs.engine

    def commit(self, polynomial, ofmt=L.G1_AFFINE_MONT):  # :59-64
        e = self.engine
        blob = pack_scalars(polynomial.slice_coeffs())
        out = ctypes.create_string_buffer(L.POINT_BYTES[ofmt])
        rc = e.lib.kzg_commit_coeff(e.ctx, self.parameters.gs.handle, blob, polynomial.num_coeffs(), L.FR_CANONICAL, 0,
                                    out, ofmt)
        if rc:
            _raise(e, rc)
        return out.raw

    def create_witness(self, polynomial, point, ofmt=L.G1_AFFINE_MONT):  # :66-81
        e = self.engine
        x, y = point
        blob = pack_scalars(polynomial.slice_coeffs())
        out = ctypes.create_string_buffer(L.POINT_BYTES[ofmt])
        rc = e.lib.kzg_witness_coeff(e.ctx, self.parameters.gs.handle, blob, polynomial.num_coeffs(),
                                     (x % R_MODULUS).to_bytes(32, "little"), (y % R_MODULUS).to_bytes(32, "little"),
                                     L.FR_CANONICAL, 0, out, ofmt)
        if rc:
            _raise(e, rc)
        return out.raw

    def open_fold(self, polynomials, z, gamma, ofmt=L.G1_AFFINE_MONT):
        """(ys, witness): the values p_i(z) of the polynomials and ONE witness for all of them, the witness of F = sum_i gamma^i p_i
        at (z, F(z)) (kzg_open_fold_coeff; not a reference method).  KZGVerifier.verify_fold checks it; gamma is the protocol's
        challenge, a hash of the commitments, z and the values in practice."""
        ys, ws = self.open_fold_batch([polynomials], [z], [gamma], ofmt)
        return ys[0], ws[0]

    def open_fold_batch(self, groups, zs, gammas, ofmt=L.G1_AFFINE_MONT, t=None, n=None):
        """open_fold for len(zs) groups of t polynomials each in one call -> (list of lists of y, list of witnesses).  groups: a list
        of lists of Polynomials / coefficient lists (padded here to the longest), or a canonical blob / DeviceBuffer of len(zs) x t x n
        coefficients (t and n then given)."""
        e = self.engine
        return e._open_fold(e.lib.kzg_open_fold_coeff, self.parameters.gs, groups, zs, gammas, ofmt, t, n, True)

    def multiopen_commit(self, polynomials, zs, r, poly_idx=None, ofmt=L.G1_AFFINE_MONT, n=None):
        """First phase of the two-element multiproof (kzg_multiopen_coeff_commit; not a reference method): claim k is polynomial
        poly_idx[k] (None: k) at zs[k].  -> (ys, g, D): the values, the n - 1 coefficients of g = sum_k r^k (p - y_k)/(X - z_k) (the
        caller carries them to multiopen_finish; a DeviceBuffer when the polynomials are one) and D = [g(tau)].  polynomials: a list of
        Polynomials / coefficient lists (padded here to the longest), or a canonical blob / DeviceBuffer of n_polys x n coefficients (n
        given).  r must be unpredictable to whoever chose polynomials, points and values."""
        e = self.engine
        return e._multiopen_commit(e.lib.kzg_multiopen_coeff_commit, self.parameters.gs, polynomials, n, lambda n_: n_ - 1, True, zs, r, poly_idx, ofmt)

    def multiopen_finish(self, polynomials, zs, r, t, g, poly_idx=None, ofmt=L.G1_AFFINE_MONT, n=None):
        """Second phase (kzg_multiopen_coeff_finish) -> (pi, v(t)).  t MUST have been drawn after D existed (a hash that includes D):
        see the header.  t equal to a z_k raises ReferencePanic; draw another."""
        e = self.engine
        return e._multiopen_finish(e.lib.kzg_multiopen_coeff_finish, self.parameters.gs, polynomials, n, lambda n_: n_ - 1, True, zs, r, t, g, poly_idx, ofmt)

    def multiopen(self, polynomials, zs, r, challenge_t, poly_idx=None, ofmt=L.G1_AFFINE_MONT, n=None):
        """Both phases -> (ys, D, pi, t): challenge_t(D) is called between them and returns t, the caller's hash of D."""
        return self.engine._multiopen(self.multiopen_commit, self.multiopen_finish, polynomials, zs, r, challenge_t, poly_idx, ofmt, n=n)

    def create_witness_many(self, polynomial, points, ofmt=L.G1_AFFINE_MONT, coeffs_device=None):
        """Throughput form of create_witness (not a reference method): one witness per (x, y) in `points`, all for the same
        polynomial, pipelined on the engine's lanes.  Returns (witnesses, ok) with ok[j] False where the reference would
        return Err(PointNotOnPolynomial).  coeffs_device: a DeviceBuffer already holding the coefficients."""
        e = self.engine
        k = len(points)
        n = polynomial.num_coeffs() if coeffs_device is None else coeffs_device.n
        out = ctypes.create_string_buffer(L.POINT_BYTES[ofmt] * max(k, 1))
        status = (ctypes.c_int * max(k, 1))()
        if coeffs_device is None:
            src, sfmt, flags = pack_scalars(polynomial.slice_coeffs()), L.FR_CANONICAL, 0
        else:
            src, sfmt, flags = coeffs_device.ptr, coeffs_device.sfmt, L.IN_DEVICE
        if sfmt != L.FR_CANONICAL:
            raise ValueError("create_witness_many takes canonical scalars")
        rc = e.lib.kzg_witness_coeff_many(e.ctx, self.parameters.gs.handle, src, n, pack_scalars([p[0] for p in points]),
                                          pack_scalars([p[1] for p in points]), k, sfmt, flags, out, ofmt, status)
        if rc:
            _raise(e, rc)
        psz = L.POINT_BYTES[ofmt]
        return [out.raw[j * psz:(j + 1) * psz] for j in range(k)], [status[j] == 0 for j in range(k)]

    def create_witness_all_points(self, polynomial, plan, ofmt=L.G1_AFFINE_MONT):
        """Every witness over the plan's domain (FK20; not a reference method): element m is create_witness(polynomial,
        (w^m, p(w^m))) with w = compute_omega(N).omega."""
        return self.create_witness_all_points_batch([polynomial], plan, ofmt)[0]

    def create_witness_all_points_batch(self, polynomials, plan, ofmt=L.G1_AFFINE_MONT):
        """create_witness_all_points for several polynomials (zero-padded to the longest): one list of N witnesses each."""
        n = max(p.num_coeffs() for p in polynomials)
        blob = b"".join(pack_scalars(p.slice_coeffs() + [0] * (n - p.num_coeffs())) for p in polynomials)
        return _witness_all(self.engine, self.engine.lib.kzg_witness_all_coeff, plan, blob, n, len(polynomials), ofmt)

    def create_witness_all_cosets(self, polynomial, plan, ofmt=L.G1_AFFINE_MONT):
        """Every coset opening over the plan's domain (multi-point FK20; not a reference method): element i is
        create_witness_batched(polynomial, plan.coset_points(i), their values), as a KZGBatchWitness."""
        return self.create_witness_all_cosets_batch([polynomial], plan, ofmt)[0]

    def create_witness_all_cosets_batch(self, polynomials, plan, ofmt=L.G1_AFFINE_MONT):
        """create_witness_all_cosets for several polynomials (zero-padded to the longest): one list of K witnesses each."""
        n = max(p.num_coeffs() for p in polynomials)
        blob = b"".join(pack_scalars(p.slice_coeffs() + [0] * (n - p.num_coeffs())) for p in polynomials)
        return _witness_cosets(self.engine, self.engine.lib.kzg_witness_cosets_coeff, plan, blob, n, len(polynomials), ofmt)

    def open_at_points(self, polynomial, xs, ofmt=L.G1_AFFINE_MONT):
        """(ys, KZGBatchWitness): the values of the polynomial at xs from one kzg_poly_multi_eval call, then create_witness_batched
        at (xs, ys) (not a reference method: the reference's caller evaluates point by point)."""
        ys = self.engine.poly_multi_eval(polynomial.slice_coeffs(), xs)
        return ys, self.create_witness_batched(polynomial, xs, ys, ofmt)

    def create_witness_batched_with_tree(self, polynomial, tree, ys, ofmt=L.G1_AFFINE_MONT):
        """create_witness_batched at the points of a PointTree (kzg_witness_coeff_tree): any number of points up to the plan's 2^22.
        One point gives the reference's r = X + (y - x) (src/polynomial.rs:244-247) and the witness that goes with it, through
        create_witness_batched: kzg_witness_coeff_tree itself returns the constant and [(p - y) / (X - x)]_1."""
        if len(ys) != len(tree):
            raise ReferencePanic("assert_eq!(xs.len(), ys.len())")
        if len(tree) == 1:  # the reference interpolates one point as X + (y - x), so its witness is [(p - y) / (X - x) - 1]_1: the
            return self.create_witness_batched(polynomial, tree.xs, ys, ofmt)  # reference-shaped call reproduces both halves
        return tree.create_witness(self.parameters.gs, polynomial, ys=[int(y) % R_MODULUS for y in ys], ofmt=ofmt)

    def create_witness_batched(self, polynomial, xs, ys, ofmt=L.G1_AFFINE_MONT):  # :83-111
        e = self.engine
        assert len(xs) == len(ys)
        k = len(xs)
        blob = pack_scalars(polynomial.slice_coeffs())
        out = ctypes.create_string_buffer(L.POINT_BYTES[ofmt])
        r = ctypes.create_string_buffer(32 * max(k, 2))
        rlen = ctypes.c_size_t()
        rc = e.lib.kzg_witness_coeff_batched(e.ctx, self.parameters.gs.handle, blob, polynomial.num_coeffs(),
                                             pack_scalars(xs), pack_scalars(ys), k, L.FR_CANONICAL, 0, out, ofmt, r,
                                             ctypes.byref(rlen))
        if rc:
            _raise(e, rc)
        coeffs = unpack_scalars(r.raw[: 32 * rlen.value])
        return KZGBatchWitness(Polynomial.new_from_coeffs(coeffs, len(coeffs) - 1), out.raw)


class KZGVerifier:
    """src/coeff_form.rs:114-183; the pairing checks run on the GPU, one thread per opening."""

    def __init__(self, parameters):
        self.parameters = parameters
        self.engine = parameters.gs.engine

    def _hs(self):
        if self.parameters.hs is None:
            raise ReferencePanic("KZGParams.hs is empty (index out of bounds)")
        return self.parameters.hs

    def verify_eval(self, point, commitment, witness, pfmt=L.G1_AFFINE_MONT):  # :126-142
        return self.verify_eval_many([point], [commitment], [witness], pfmt)[0]

    def verify_eval_many(self, points, commitments, witnesses, pfmt=L.G1_AFFINE_MONT):
        """verify_eval for many independent openings in one launch -> list of bool"""
        e = self.engine
        n = len(points)
        assert len(commitments) == n and len(witnesses) == n
        ok = ctypes.create_string_buffer(max(n, 1))
        rc = e.lib.kzg_verify_eval(e.ctx, self.parameters.gs.handle, self._hs().handle,
                                   pack_scalars([p[0] for p in points]), pack_scalars([p[1] for p in points]),
                                   L.FR_CANONICAL, b"".join(commitments), b"".join(witnesses), pfmt, n, ok)
        if rc:
            _raise(e, rc)
        return [bool(b) for b in ok.raw[:n]]

    def verify_eval_batch(self, points, commitments, witnesses, r=None, commitment_idx=None, pfmt=L.G1_AFFINE_MONT):
        """kzg_verify_eval_batch (not a reference method): True iff ALL the openings verify, from one pairing check of their
        combination with the weights r^k.  points[k] = (x_k, y_k) and witnesses[k] open commitments[commitment_idx[k]];
        commitment_idx=None: one commitment per opening.  r: the challenge, an int in [1, R).  r=None draws it here with `secrets`
        -- sound because it is drawn after the openings were handed over; a protocol that needs a reproducible verdict passes the
        hash of all inputs.  False says nothing about which opening is bad: verify_eval_many() does (verify_eval_with_fallback)."""
        e = self.engine
        count = len(points)
        if len(witnesses) != count or (commitment_idx is not None and len(commitment_idx) != count):
            raise ReferencePanic("verify_eval_batch: one point, witness and commitment index per opening")
        if r is None:
            r = secrets.randbelow(R_MODULUS - 1) + 1
        if not 1 <= int(r) < R_MODULUS:
            raise ReferencePanic("verify_eval_batch: the challenge r must be in [1, R)")
        idx = None
        if commitment_idx is not None:
            idx = (ctypes.c_uint32 * max(count, 1))(*[int(i) % (1 << 32) for i in commitment_idx])
        ok = ctypes.c_int(-1)
        rc = e.lib.kzg_verify_eval_batch(e.ctx, self.parameters.gs.handle, self._hs().handle, pack_scalars([p[0] for p in points]),
                                         pack_scalars([p[1] for p in points]), L.FR_CANONICAL, b"".join(commitments), len(commitments),
                                         idx, b"".join(witnesses), pfmt, count, int(r).to_bytes(32, "little"), ctypes.byref(ok))
        if rc:
            _raise(e, rc)
        return bool(ok.value)

    def verify_fold(self, z, ys, commitments, witness, gamma, pfmt=L.G1_AFFINE_MONT):
        """kzg_verify_fold for one group (not a reference method): True iff `witness` opens sum_i gamma^i commitments[i] at z to
        sum_i gamma^i ys[i] -- what open_fold produced.  Sound for the single values only if gamma was unpredictable to whoever
        chose the polynomials and the claimed values (a hash of the commitments, z and ys)."""
        return self.verify_fold_batch([z], [ys], commitments, [witness], [gamma], 1, pfmt=pfmt)

    def verify_fold_batch(self, zs, ys, commitments, witnesses, gammas, r=None, commitment_idx=None, pfmt=L.G1_AFFINE_MONT):
        """kzg_verify_fold: ONE verdict from one pairing check for len(zs) folded openings.  ys[g]: the t claimed values of group g,
        witnesses[g] its folded witness, gammas[g] its challenge; value (g, i) belongs to commitments[commitment_idx[g * t + i]]
        (None: commitments[g * t + i]).  r: the challenge that combines the groups, an int in [1, R); r=None draws it here with
        `secrets`, sound because it is drawn after everything was handed over."""
        e = self.engine
        groups = len(zs)
        t = len(ys[0]) if groups else 1
        if len(ys) != groups or len(witnesses) != groups or len(gammas) != groups or any(len(y) != t for y in ys):
            raise ReferencePanic("verify_fold: one point, witness, challenge and list of t values per group")
        if commitment_idx is not None and len(commitment_idx) != groups * t:
            raise ReferencePanic("verify_fold: one commitment index per value")
        if r is None:
            r = secrets.randbelow(R_MODULUS - 1) + 1
        idx = None
        if commitment_idx is not None:
            idx = (ctypes.c_uint32 * max(groups * t, 1))(*[int(i) % (1 << 32) for i in commitment_idx])
        ok = ctypes.c_int(-1)
        rc = e.lib.kzg_verify_fold(e.ctx, self.parameters.gs.handle, self._hs().handle, pack_scalars(zs), pack_scalars([y for g in ys for y in g]),
                                   L.FR_CANONICAL, b"".join(commitments), len(commitments), idx, b"".join(witnesses), pfmt, t, groups,
                                   b"".join(int(g).to_bytes(32, "little") for g in gammas), int(r).to_bytes(32, "little"), ctypes.byref(ok))
        if rc:
            _raise(e, rc)
        return bool(ok.value)

    def verify_multiopen(self, zs, ys, commitments, D, pi, r, t, commitment_idx=None, pfmt=L.G1_AFFINE_MONT):
        """kzg_verify_multiopen (not a reference method): ONE verdict from one pairing check for the claims p_{m(k)}(zs[k]) = ys[k]
        answered by the two elements (D, pi) of multiopen; m(k) = commitment_idx[k] (None: k).  r: the challenge the prover used,
        unpredictable to whoever chose polynomials, points and values; t MUST have been drawn after D was received (a hash that
        includes D): with a predictable t one wrong claim passes, see the header."""
        e = self.engine
        count = len(zs)
        if len(ys) != count:
            raise ReferencePanic("verify_multiopen: one value per point")
        idx = Engine._index_arg(commitment_idx, count)
        ok = ctypes.c_int(-1)
        enc = lambda x: int(x).to_bytes(32, "little")
        rc = e.lib.kzg_verify_multiopen(e.ctx, self.parameters.gs.handle, self._hs().handle, b"".join(enc(z) for z in zs), pack_scalars(ys),
                                        L.FR_CANONICAL, b"".join(commitments), len(commitments), idx, count, enc(r), enc(t), D, pi, pfmt,
                                        ctypes.byref(ok))
        if rc:
            _raise(e, rc)
        return bool(ok.value)

    def verify_eval_with_fallback(self, points, commitments, witnesses, r=None, commitment_idx=None, pfmt=L.G1_AFFINE_MONT):
        """One verdict per opening, as verify_eval_many(): the batch check first, and the per-opening checks only when it says no."""
        if self.verify_eval_batch(points, commitments, witnesses, r, commitment_idx, pfmt):
            return [True] * len(points)
        if commitment_idx is not None:
            commitments = [commitments[i] for i in commitment_idx]
        return self.verify_eval_many(points, commitments, witnesses, pfmt)

    def verify_eval_batched(self, xs, commitment, witness, pfmt=L.G1_AFFINE_MONT):  # :144-182
        e = self.engine
        r = witness.r
        ok = ctypes.c_int()
        rc = e.lib.kzg_verify_eval_batched(e.ctx, self.parameters.gs.handle, self._hs().handle, pack_scalars(xs), len(xs),
                                           pack_scalars(r.slice_coeffs()), r.num_coeffs(), L.FR_CANONICAL, commitment,
                                           witness.w, pfmt, ctypes.byref(ok))
        if rc:
            _raise(e, rc)
        return bool(ok.value)

    def verify_eval_batched_with_tree(self, tree, commitment, witness, pfmt=L.G1_AFFINE_MONT):
        """verify_eval_batched at the points of a PointTree (kzg_verify_eval_tree): any number of points up to the plan's 2^22."""
        return self.verify_eval_batched_with_tree_many(tree, [commitment], [witness], pfmt)[0]

    def verify_eval_batched_with_tree_many(self, tree, commitments, witnesses, pfmt=L.G1_AFFINE_MONT):
        """`count` openings at the tree's points in one call (hz is computed once) -> list of bool"""
        e = self.engine
        k, n = len(tree), len(commitments)
        assert len(witnesses) == n
        rs = []
        for w in witnesses:
            c = list(w.r.slice_coeffs())
            if len(c) > k:
                raise ReferencePanic("verify_eval_batched_with_tree: witness.r has more coefficients than the tree has points")
            rs.append(pack_scalars(c + [0] * (k - len(c))))
        ok = ctypes.create_string_buffer(max(n, 1))
        rc = e.lib.kzg_verify_eval_tree(e.ctx, self.parameters.gs.handle, self._hs().handle, tree.handle, b"".join(rs) or bytes(32),
                                        L.FR_CANONICAL, b"".join(commitments) or bytes(96), b"".join(w.w for w in witnesses) or bytes(96), pfmt, n, ok)
        if rc:
            _raise(e, rc)
        return [bool(b) for b in ok.raw[:n]]

    def verify_cosets(self, verifier, commitment, coset_ids, cells, proofs, pfmt=L.G1_AFFINE_MONT):
        """kzg_verify_cosets for the cells of ONE commitment: cells[k] (l values) and proofs[k] open coset coset_ids[k] of the
        CosetVerifier's domain -> list of bool.  Not a reference method."""
        return verifier.verify([commitment], [0] * len(proofs), coset_ids, cells, proofs, pfmt)

    def verify_cosets_batch(self, verifier, commitment, coset_ids, cells, proofs, r=None, pfmt=L.G1_AFFINE_MONT):
        """kzg_verify_cosets_batch for the cells of ONE commitment -> bool (CosetVerifier.verify_batch).  Not a reference method."""
        return verifier.verify_batch([commitment], [0] * len(proofs), coset_ids, cells, proofs, r, pfmt)

    def verify_poly(self, commitment, polynomial, pfmt=L.G1_AFFINE_MONT):
        e = self.engine
        ok = ctypes.c_int()
        rc = e.lib.kzg_verify_poly_coeff(e.ctx, self.parameters.gs.handle, commitment, pfmt,
                                         pack_scalars(polynomial.slice_coeffs()), polynomial.num_coeffs(),
                                         L.FR_CANONICAL, 0, ctypes.byref(ok))
        if rc:
            _raise(e, rc)
        return bool(ok.value)


class KZGProverEvalForm:
    """src/eval_form.rs:39-147"""

    def __init__(self, parameters, lagrange_basis_g):  # :88-100
        self.parameters = parameters
        self.lagrange_basis_g = lagrange_basis_g
        self.engine = parameters.gs.engine
        self.d, self.exp, self._omega = compute_omega(len(parameters.gs))

    def degree(self):
        return self.d

    def omega(self):
        return self._omega

    def commit(self, evals, ofmt=L.G1_AFFINE_MONT):  # :114-122
        e = self.engine
        if self.d != evals.d:
            raise ReferencePanic("assert!(self.d == evals.d) (src/eval_form.rs:115)")
        out = ctypes.create_string_buffer(L.POINT_BYTES[ofmt])
        rc = e.lib.kzg_commit_eval(e.ctx, self.lagrange_basis_g.handle, pack_scalars(evals.coeffs), len(evals),
                                   L.FR_CANONICAL, 0, out, ofmt)
        if rc:
            _raise(e, rc)
        return out.raw

    def create_witness(self, evals, i, ofmt=L.G1_AFFINE_MONT):  # :124-140
        e = self.engine
        out = ctypes.create_string_buffer(L.POINT_BYTES[ofmt])
        rc = e.lib.kzg_witness_eval(e.ctx, self.lagrange_basis_g.handle, pack_scalars(evals.coeffs), len(evals), i,
                                    L.FR_CANONICAL, 0, out, ofmt)
        if rc:
            _raise(e, rc)
        return out.raw

    def open_at(self, evals, z, ofmt=L.G1_AFFINE_MONT):
        """(y, witness) at ANY point z of Fr (kzg_open_eval; not a reference method): y = p(z) and the opening proof, against the
        Lagrange SRS alone.  At z = omega^i the witness is create_witness(evals, i)."""
        ys, ws = self.open_at_batch([evals], [z], ofmt)
        return ys[0], ws[0]

    def open_at_batch(self, evals, zs, ofmt=L.G1_AFFINE_MONT):
        """open_at for len(zs) polynomials in one call -> (list of y, list of witnesses).  evals: a list of EvaluationDomains /
        evaluation lists, or a canonical blob / a DeviceBuffer of len(zs) x d scalars."""
        e = self.engine
        batch = len(zs)
        ptr, d, sfmt, flags, _keep = e._eval_vectors_arg(evals, batch, len(self.lagrange_basis_g))
        psz = L.POINT_BYTES[ofmt]
        ys = ctypes.create_string_buffer(32 * max(batch, 1))
        out = ctypes.create_string_buffer(psz * max(batch, 1))
        zb = b"".join(e._host_scalar(int(z), sfmt) for z in zs)
        rc = e.lib.kzg_open_eval(e.ctx, self.lagrange_basis_g.handle, ptr, d, batch, zb, sfmt, flags, ys, out, ofmt)
        if rc:
            _raise(e, rc)
        return ([e._scalar_from(ys.raw[32 * b:32 * b + 32], sfmt) for b in range(batch)],
                [out.raw[b * psz:(b + 1) * psz] for b in range(batch)])

    def open_fold(self, evals_list, z, gamma, ofmt=L.G1_AFFINE_MONT):
        """(ys, witness): the values p_i(z) of the polynomials with the evaluations evals_list[i], at ANY point z of Fr, and ONE
        witness for all of them: open_at of the folded vector sum_i gamma^i evals_i (kzg_open_fold_eval; not a reference method)."""
        ys, ws = self.open_fold_batch([evals_list], [z], [gamma], ofmt)
        return ys[0], ws[0]

    def open_fold_batch(self, groups, zs, gammas, ofmt=L.G1_AFFINE_MONT, t=None):
        """open_fold for len(zs) groups of t evaluation vectors each in one call -> (list of lists of y, list of witnesses).  groups: a
        list of lists of EvaluationDomains / evaluation lists, or a canonical blob / DeviceBuffer of len(zs) x t x d scalars (t given)."""
        e = self.engine
        return e._open_fold(e.lib.kzg_open_fold_eval, self.lagrange_basis_g, groups, zs, gammas, ofmt, t, len(self.lagrange_basis_g), False)

    def multiopen_commit(self, evals, zs, r, poly_idx=None, ofmt=L.G1_AFFINE_MONT):
        """First phase of the two-element multiproof (kzg_multiopen_eval_commit; not a reference method): claim k is the polynomial with
        the evaluations evals[poly_idx[k]] (None: k) at zs[k], ANY point of Fr.  -> (ys, g, D): the values, the d values of
        g = sum_k r^k (p - y_k)/(X - z_k) on the domain (the caller carries them to multiopen_finish; a DeviceBuffer when the
        evaluations are one) and D = [g(tau)].  evals: a list of EvaluationDomains / evaluation lists, or a canonical blob / DeviceBuffer
        of n_polys x d scalars.  r must be unpredictable to whoever chose polynomials, points and values."""
        e = self.engine
        return e._multiopen_commit(e.lib.kzg_multiopen_eval_commit, self.lagrange_basis_g, evals, len(self.lagrange_basis_g), lambda d: d, False, zs, r,
                                   poly_idx, ofmt)

    def multiopen_finish(self, evals, zs, r, t, g, poly_idx=None, ofmt=L.G1_AFFINE_MONT):
        """Second phase (kzg_multiopen_eval_finish) -> (pi, v(t)).  t MUST have been drawn after D existed (a hash that includes D):
        see the header.  t equal to a z_k raises ReferencePanic; draw another."""
        e = self.engine
        return e._multiopen_finish(e.lib.kzg_multiopen_eval_finish, self.lagrange_basis_g, evals, len(self.lagrange_basis_g), lambda d: d, False, zs, r, t,
                                   g, poly_idx, ofmt)

    def multiopen(self, evals, zs, r, challenge_t, poly_idx=None, ofmt=L.G1_AFFINE_MONT):
        """Both phases -> (ys, D, pi, t): challenge_t(D) is called between them and returns t, the caller's hash of D."""
        return self.engine._multiopen(self.multiopen_commit, self.multiopen_finish, evals, zs, r, challenge_t, poly_idx, ofmt)

    def create_witness_many(self, evals, indices, ofmt=L.G1_AFFINE_MONT):
        """Throughput form of create_witness (not a reference method): one witness per index, same evaluation vector."""
        e = self.engine
        k = len(indices)
        out = ctypes.create_string_buffer(L.POINT_BYTES[ofmt] * max(k, 1))
        idx = (ctypes.c_size_t * max(k, 1))(*indices)
        rc = e.lib.kzg_witness_eval_many(e.ctx, self.lagrange_basis_g.handle, pack_scalars(evals.coeffs), len(evals), idx, k,
                                         L.FR_CANONICAL, 0, out, ofmt)
        if rc:
            _raise(e, rc)
        psz = L.POINT_BYTES[ofmt]
        return [out.raw[j * psz:(j + 1) * psz] for j in range(k)]

    def create_witness_all_points(self, evals, plan, ofmt=L.G1_AFFINE_MONT):
        """Every witness over the domain (FK20 against `plan`, built from the monomial SRS; not a reference method): element m
        equals create_witness(evals, m)."""
        return self.create_witness_all_points_batch([evals], plan, ofmt)[0]

    def create_witness_all_points_batch(self, evals_list, plan, ofmt=L.G1_AFFINE_MONT):
        d = len(evals_list[0])
        if any(len(ev) != d for ev in evals_list):
            raise ReferencePanic("assert!(self.d == evals.d): evaluation vectors of different lengths")
        blob = b"".join(pack_scalars(ev.coeffs) for ev in evals_list)
        return _witness_all(self.engine, self.engine.lib.kzg_witness_all_eval, plan, blob, d, len(evals_list), ofmt)

    def create_witness_all_cosets(self, evals, plan, ofmt=L.G1_AFFINE_MONT):
        """Every coset opening over the domain (multi-point FK20 against `plan`, built from the monomial SRS; not a reference
        method): element i opens plan.coset_points(i), as a KZGBatchWitness."""
        d = len(evals)
        blob = pack_scalars(evals.coeffs)
        return _witness_cosets(self.engine, self.engine.lib.kzg_witness_cosets_eval, plan, blob, d, 1, ofmt)[0]

    def create_witness_all(self):  # :142-146: identity
        return bytes(96)


class KZGVerifierEvalForm:
    """src/eval_form.rs:149-218"""

    def __init__(self, parameters, lagrange_basis_g, lagrange_basis_h=None):
        self.parameters = parameters
        self.lagrange_basis_g = lagrange_basis_g
        self.lagrange_basis_h = lagrange_basis_h
        self.engine = parameters.gs.engine
        self.d, self.exp, self.omega = compute_omega(len(parameters.gs))

    def verify_eval(self, point, commitment, witness, pfmt=L.G1_AFFINE_MONT):  # :173-190
        i, y = point
        return KZGVerifier(self.parameters).verify_eval((pow(self.omega, i, R_MODULUS), y), commitment, witness, pfmt)

    def _at_omega(self, points):
        return [(pow(self.omega, i, R_MODULUS), y) for i, y in points]

    def verify_eval_batch(self, points, commitments, witnesses, r=None, commitment_idx=None, pfmt=L.G1_AFFINE_MONT):
        """KZGVerifier.verify_eval_batch with points[k] = (i_k, y_k) as verify_eval takes them: opening k is at omega^i_k."""
        return KZGVerifier(self.parameters).verify_eval_batch(self._at_omega(points), commitments, witnesses, r, commitment_idx, pfmt)

    def verify_fold(self, z, ys, commitments, witness, gamma, pfmt=L.G1_AFFINE_MONT):
        """KZGVerifier.verify_fold: z is a point of Fr as KZGProverEvalForm.open_fold takes it (not a domain index)."""
        return KZGVerifier(self.parameters).verify_fold(z, ys, commitments, witness, gamma, pfmt)

    def verify_fold_batch(self, zs, ys, commitments, witnesses, gammas, r=None, commitment_idx=None, pfmt=L.G1_AFFINE_MONT):
        """KZGVerifier.verify_fold_batch for what KZGProverEvalForm.open_fold_batch produced."""
        return KZGVerifier(self.parameters).verify_fold_batch(zs, ys, commitments, witnesses, gammas, r, commitment_idx, pfmt)

    def verify_multiopen(self, zs, ys, commitments, D, pi, r, t, commitment_idx=None, pfmt=L.G1_AFFINE_MONT):
        """KZGVerifier.verify_multiopen: zs are points of Fr as KZGProverEvalForm.multiopen takes them (not domain indices)."""
        return KZGVerifier(self.parameters).verify_multiopen(zs, ys, commitments, D, pi, r, t, commitment_idx, pfmt)

    def verify_eval_with_fallback(self, points, commitments, witnesses, r=None, commitment_idx=None, pfmt=L.G1_AFFINE_MONT):
        """One verdict per opening (points[k] = (i_k, y_k)): the batch check first, the per-opening checks only when it says no."""
        return KZGVerifier(self.parameters).verify_eval_with_fallback(self._at_omega(points), commitments, witnesses, r, commitment_idx, pfmt)

    def verify_open_at_batch(self, evals, zs, commitments, witnesses, r=None, pfmt=L.G1_AFFINE_MONT):
        """The blob-level check: witnesses[b] opens the polynomial with the evaluations evals[b] and the commitment commitments[b]
        at zs[b] (any point of Fr; what KZGProverEvalForm.open_at_batch produced).  The claimed values p_b(zs[b]) are computed from
        the evaluations (Engine.eval_form_eval; 32 bytes each come back to the host), then one verify_eval_batch.  evals as
        eval_form_eval takes them; r as verify_eval_batch."""
        ys = self.engine.eval_form_eval(evals, zs, self.d)
        return KZGVerifier(self.parameters).verify_eval_batch(list(zip(zs, ys)), commitments, witnesses, r, None, pfmt)

    def verify_eval_all(self, ys, commitment, witness, pfmt=L.G1_AFFINE_MONT):  # :192-217
        e = self.engine
        if self.lagrange_basis_h is None or self.parameters.hs is None:
            raise ReferencePanic("lagrange_basis_h / hs missing (index out of bounds)")
        ok = ctypes.c_int()
        rc = e.lib.kzg_verify_eval_all(e.ctx, self.lagrange_basis_g.handle, self.lagrange_basis_h.handle,
                                       self.parameters.hs.handle, pack_scalars(ys), len(ys), L.FR_CANONICAL, commitment,
                                       witness, pfmt, ctypes.byref(ok))
        if rc:
            _raise(e, rc)
        return bool(ok.value)

    def verify_poly(self, commitment, evals, pfmt=L.G1_AFFINE_MONT):
        e = self.engine
        ok = ctypes.c_int()
        rc = e.lib.kzg_verify_poly_eval(e.ctx, self.parameters.gs.handle, commitment, pfmt, pack_scalars(evals.coeffs),
                                        len(evals), L.FR_CANONICAL, 0, ctypes.byref(ok))
        if rc:
            _raise(e, rc)
        return bool(ok.value)
