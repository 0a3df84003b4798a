"""Host-side mirror of the reference crate's API for the accelerated path.

Names and argument meaning follow /root/reference/src/lib.rs:
  Point{x,y}.mul_scalar(n)      lib.rs:149-164   -> Point.mul_scalar / mul_scalar_batch
  Point.projective()/.equals()  lib.rs:141-147, 180-185
  PointProjective.add/.affine   lib.rs:70-131    -> point_add_batch (add + affine)
  Signature{r_b8, s}            lib.rs:239-243
  verify(pk, sig, msg) -> bool  lib.rs:395-412   -> verify / verify_batch
  B8.mul_scalar(k) (PrivateKey::public, lib.rs:304-306) -> mul_fixed_base_batch

Everything numeric happens in libbjj_hip.so on the GPU.  This file only marshals
Python ints / numpy byte arrays to the 32-byte little-endian records of the C ABI.
Like the reference, mul_scalar and add are infallible and verify() folds every
failure into False; BjjError is raised only for API misuse / HIP errors.
"""
import ctypes

import numpy as np

from . import _lib

Q = 21888242871839275222246405745257275088548364400416034343698204186575808495617  # lib.rs:33-36
B8 = (
    5299619240641551281634865583518297030282874472190772894086521144482721001553,
    16950150798460657717958625567821834550301663161624707787222815936182638968203,
)  # lib.rs:37-46
SUBORDER = 21888242871839275222246405745257275088614511777268538073601725287587578984328 >> 3  # lib.rs:53-58


class BjjError(RuntimeError):
    """API misuse or a failed library call; `code` is the library's return code (a BJJ_E_* value) when a call returned one"""

    def __init__(self, msg, code=None):
        super().__init__(msg)
        self.code = code


def _as_u8(a, width, name):
    """Accepts an (n, width) / (n*width,) uint8 array, or a list of ints / int tuples."""
    if isinstance(a, np.ndarray):
        if a.dtype != np.uint8:
            # a value cast would keep only the low byte of every element: reinterpret little-endian unsigned
            # limbs (e.g. the natural (n, 4) uint64 layout of Fr::into_repr().0) and refuse everything else
            if a.dtype.kind != "u" or 32 % a.dtype.itemsize or (a.dtype.itemsize > 1 and a.dtype.byteorder == ">"):
                raise BjjError("%s: array dtype %s is neither uint8 bytes nor little-endian unsigned limbs" % (name, a.dtype))
            if a.dtype.byteorder == "=" and a.dtype.itemsize > 1:
                import sys as _sys
                if _sys.byteorder != "little":
                    raise BjjError("%s: native-endian limbs on a big-endian host" % name)
            a = np.ascontiguousarray(a).view(np.uint8)
        arr = np.ascontiguousarray(a).reshape(-1)
        if arr.size % width:
            raise BjjError("%s: byte length %d is not a multiple of %d" % (name, arr.size, width))
        return arr
    if isinstance(a, (bytes, bytearray)):
        return _as_u8(np.frombuffer(bytes(a), dtype=np.uint8), width, name)
    out = bytearray()
    for item in a:
        vals = item if isinstance(item, (tuple, list)) else (item,)
        if len(vals) * 32 != width:
            raise BjjError("%s: expected %d integers per item" % (name, width // 32))
        for v in vals:
            v = int(v)
            if v < 0 or v >> 256:
                raise BjjError("%s: integer out of the unsigned 256-bit range" % name)
            out += v.to_bytes(32, "little")
    return np.frombuffer(bytes(out), dtype=np.uint8).copy()


def _negate_x(points):
    """(n, 64) canonical affine points (x, y < Q, as the library writes them) -> (-x mod Q, y): Q - x over eight 32-bit limbs with a
    borrow, vectorised; x = 0 stays 0"""
    p = np.ascontiguousarray(points, dtype=np.uint8).reshape(-1, 64).copy()
    x = p[:, :32].copy().view("<u4").astype(np.int64)                      # (n, 8) limbs, little-endian
    out = np.empty_like(x)
    borrow = np.zeros(x.shape[0], dtype=np.int64)
    for i in range(8):
        d = ((Q >> (32 * i)) & 0xFFFFFFFF) - x[:, i] - borrow
        borrow = (d < 0).astype(np.int64)
        out[:, i] = d + (borrow << 32)
    out[~x.any(axis=1)] = 0
    p[:, :32] = out.astype("<u4").view(np.uint8)
    return p


def _ints(arr, per_item):
    b = arr.tobytes()
    vals = [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]
    if per_item == 1:
        return vals
    return [tuple(vals[i:i + per_item]) for i in range(0, len(vals), per_item)]


class Context:
    """One GPU + stream + fixed-base table (bjj_init / bjj_free).
    window_bits: 0 = the library default (23 bits, 5.9 GB), WINDOW_AUTO = widest table that fits in 60 % of the free
    HBM, or an explicit width 4..28 (28 = 154.6 GB, what bench.py measures)."""

    def __init__(self, device=0, window_bits=0, _borrowed=None):
        self.lib = _lib.load()
        self._owned = _borrowed is None
        self._sets = []                                               # SignerSet objects that are still open
        self._dlogs = []                                              # DlogTable objects that are still open
        if _borrowed is not None:  # a per-device context owned by a MultiContext
            self.handle = ctypes.c_void_p(_borrowed)
            return
        h = ctypes.c_void_p()
        rc = self.lib.bjj_init(int(device), int(window_bits), ctypes.byref(h))
        if rc != _lib.BJJ_OK:
            raise BjjError("bjj_init failed (%d): %s" % (rc, self.lib.bjj_last_error().decode()))
        self.handle = h

    def close(self):
        if getattr(self, "handle", None):
            for b in list(getattr(self, "_bases", [])):               # FixedBase objects that were never closed
                b.close()
            for t in list(self._sets):                                # ... and SignerSet objects
                t.close()
            for t in list(self._dlogs):                               # ... and DlogTable objects
                t.close()
            for ptr in list(getattr(self, "_pinned", {}).values()):   # arrays from host_empty that were never released
                self.lib.bjj_host_free(self.handle, ptr)
            self._pinned = {}
            if self._owned:
                self.lib.bjj_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc, what):
        if rc != _lib.BJJ_OK:
            raise BjjError("%s failed (%d): %s" % (what, rc, self.lib.bjj_last_error().decode()), rc)

    def info(self):
        i = _lib.BjjInfo()
        i.struct_size = ctypes.sizeof(_lib.BjjInfo)
        self._ck(self.lib.bjj_get_info(self.handle, ctypes.byref(i)), "bjj_get_info")
        return i

    def check_table(self):
        """number of violated link conditions of the fixed-base table (0 = sound), checked on the device"""
        bad = ctypes.c_uint64(0)
        self._ck(self.lib.bjj_check_table(self.handle, ctypes.byref(bad)), "bjj_check_table")
        return bad.value

    def sync(self):
        self._ck(self.lib.bjj_sync(self.handle), "bjj_sync")

    def reserve(self, n):
        self._ck(self.lib.bjj_reserve(self.handle, n), "bjj_reserve")

    # ---- pinned host memory (bjj_host_alloc / bjj_host_register): host-pointer calls copy such arrays directly ----
    def host_empty(self, nbytes):
        """uint8 numpy array of `nbytes` bytes in page-locked memory owned by the library; release with host_free(array).
        Host-pointer calls whose arrays live in such memory skip the staging copy (include/bjj_hip.h)."""
        p = ctypes.c_void_p()
        self._ck(self.lib.bjj_host_alloc(self.handle, int(nbytes), ctypes.byref(p)), "bjj_host_alloc")
        buf = (ctypes.c_uint8 * int(nbytes)).from_address(p.value)
        a = np.frombuffer(buf, dtype=np.uint8)
        self._pinned = getattr(self, "_pinned", {})
        self._pinned[a.ctypes.data] = p.value
        return a

    def host_free(self, a):
        """release an array from host_empty (the array must not be used afterwards)"""
        ptr = getattr(self, "_pinned", {}).pop(a.ctypes.data, None)
        if ptr is None:
            raise BjjError("host_free: not an array from host_empty")
        self._ck(self.lib.bjj_host_free(self.handle, ptr), "bjj_host_free")

    def host_register(self, a):
        """pin the memory of an existing contiguous numpy array in place (hipHostRegister)"""
        self._ck(self.lib.bjj_host_register(self.handle, a.ctypes.data, a.nbytes), "bjj_host_register")

    def host_unregister(self, a):
        self._ck(self.lib.bjj_host_unregister(self.handle, a.ctypes.data), "bjj_host_unregister")

    def host_is_pinned(self, a):
        rc = self.lib.bjj_host_is_pinned(self.handle, a.ctypes.data, a.nbytes)
        if rc < 0:
            self._ck(rc, "bjj_host_is_pinned")
        return bool(rc)

    # ---- host-buffer batch calls (numpy uint8 in / out) ----
    def mul_fixed_base(self, scalars):
        s = _as_u8(scalars, 32, "scalars")
        n = s.size // 32
        out = np.empty(n * 64, dtype=np.uint8)
        self._ck(self.lib.bjj_mul_fixed_base(self.handle, s.ctypes.data, n, out.ctypes.data), "bjj_mul_fixed_base")
        return out.reshape(n, 64)

    def mul_fixed_base_compressed(self, scalars):
        """B8.mul_scalar(n).compress() in one pass (lib.rs:149-164 + 166-178) -> (n, 32)"""
        s = _as_u8(scalars, 32, "scalars")
        n = s.size // 32
        out = np.empty(n * 32, dtype=np.uint8)
        self._ck(self.lib.bjj_mul_fixed_base_compressed(self.handle, s.ctypes.data, n, out.ctypes.data), "bjj_mul_fixed_base_compressed")
        return out.reshape(n, 32)

    def mul_var_base(self, points, scalars):
        p = _as_u8(points, 64, "points")
        s = _as_u8(scalars, 32, "scalars")
        n = s.size // 32
        if p.size != n * 64:
            raise BjjError("mul_var_base: %d points vs %d scalars" % (p.size // 64, n))
        out = np.empty(n * 64, dtype=np.uint8)
        self._ck(self.lib.bjj_mul_var_base(self.handle, p.ctypes.data, s.ctypes.data, n, out.ctypes.data),
                 "bjj_mul_var_base")
        return out.reshape(n, 64)

    def mul_var_base_wide(self, points, scalars, scalar_bytes):
        """Point::mul_scalar for scalars of scalar_bytes (a multiple of 32) little-endian bytes each (lib.rs:149, 156-157)."""
        p = _as_u8(points, 64, "points")
        s = _as_u8(scalars, scalar_bytes, "scalars")
        n = p.size // 64
        if s.size != n * scalar_bytes:
            raise BjjError("mul_var_base_wide: %d points vs %d scalars" % (n, s.size // scalar_bytes))
        out = np.empty(n * 64, dtype=np.uint8)
        self._ck(self.lib.bjj_mul_var_base_wide(self.handle, p.ctypes.data, s.ctypes.data, scalar_bytes, n, out.ctypes.data),
                 "bjj_mul_var_base_wide")
        return out.reshape(n, 64)

    def proj_add(self, p, q):
        """raw PointProjective::add (lib.rs:88-131): (n, 96) x/y/z records in and out, any z"""
        a = _as_u8(p, 96, "p")
        b = _as_u8(q, 96, "q")
        n = a.size // 96
        if b.size != a.size:
            raise BjjError("proj_add: array lengths disagree")
        out = np.empty(n * 96, dtype=np.uint8)
        self._ck(self.lib.bjj_proj_add(self.handle, a.ctypes.data, b.ctypes.data, n, out.ctypes.data), "bjj_proj_add")
        return out.reshape(n, 96)

    def proj_affine(self, p):
        """PointProjective::affine (lib.rs:70-85): (n, 96) -> (n, 64); z == 0 -> (0, 0)"""
        a = _as_u8(p, 96, "p")
        n = a.size // 96
        out = np.empty(n * 64, dtype=np.uint8)
        self._ck(self.lib.bjj_proj_affine(self.handle, a.ctypes.data, n, out.ctypes.data), "bjj_proj_affine")
        return out.reshape(n, 64)

    def poseidon5(self, inputs):
        a = _as_u8(inputs, 160, "inputs")
        n = a.size // 160
        out = np.empty(n * 32, dtype=np.uint8)
        self._ck(self.lib.bjj_poseidon5(self.handle, a.ctypes.data, n, out.ctypes.data), "bjj_poseidon5")
        return out.reshape(n, 32)

    def eddsa_verify(self, pk, r_b8, s, msg):
        a = _as_u8(pk, 64, "pk")
        r = _as_u8(r_b8, 64, "r_b8")
        sv = _as_u8(s, 32, "s")
        m = _as_u8(msg, 32, "msg")
        n = sv.size // 32
        if a.size != n * 64 or r.size != n * 64 or m.size != n * 32:
            raise BjjError("eddsa_verify: array lengths disagree")
        ok = np.empty(n, dtype=np.uint8)
        self._ck(self.lib.bjj_eddsa_verify(self.handle, a.ctypes.data, r.ctypes.data, sv.ctypes.data, m.ctypes.data, n,
                                           ok.ctypes.data), "bjj_eddsa_verify")
        return ok

    def schnorr_verify(self, pk, r, s, msg):
        """verify_schnorr in bulk: 1 / 0 = Ok(true / false), 2 = Err (msg > Q).  s: 32-byte integers."""
        a = _as_u8(pk, 64, "pk")
        rr = _as_u8(r, 64, "r")
        sv = _as_u8(s, 32, "s")
        m = _as_u8(msg, 32, "msg")
        n = sv.size // 32
        if a.size != n * 64 or rr.size != n * 64 or m.size != n * 32:
            raise BjjError("schnorr_verify: array lengths disagree")
        ok = np.empty(n, dtype=np.uint8)
        self._ck(self.lib.bjj_schnorr_verify(self.handle, a.ctypes.data, rr.ctypes.data, sv.ctypes.data, m.ctypes.data, n,
                                             ok.ctypes.data), "bjj_schnorr_verify")
        return ok

    def point_add(self, p, q):
        a = _as_u8(p, 64, "p")
        b = _as_u8(q, 64, "q")
        n = a.size // 64
        if b.size != a.size:
            raise BjjError("point_add: array lengths disagree")
        out = np.empty(n * 64, dtype=np.uint8)
        self._ck(self.lib.bjj_point_add(self.handle, a.ctypes.data, b.ctypes.data, n, out.ctypes.data), "bjj_point_add")
        return out.reshape(n, 64)

    def msm(self, points, scalars, window_bits=0):
        """Q = sum k_i * P_i as ONE (1, 64) record (bjj_msm): the fold of P_i.mul_scalar(k_i) with PointProjective::add from the
        identity, then affine() (lib.rs:149-164, 88-131, 70-85).  n == 0 gives (0, 1).  An off-curve point raises BjjError naming
        the smallest such index (the library returns (0, 0) and that index as data).  window_bits: 0 = the library's choice, 4..20
        forces the bucket width."""
        a = _as_u8(points, 64, "points")
        s = _as_u8(scalars, 32, "scalars")
        n = a.size // 64
        if s.size != n * 32:
            raise BjjError("msm: %d points but %d scalars" % (n, s.size // 32))
        out = np.empty(64, dtype=np.uint8)
        first = ctypes.c_int64(-1)
        self._ck(self.lib.bjj_msm(self.handle, a.ctypes.data if n else None, s.ctypes.data if n else None, n, int(window_bits),
                                  out.ctypes.data, ctypes.byref(first)), "bjj_msm")
        if first.value != -1:
            raise BjjError("msm: point %d is not on the curve" % first.value)
        return out.reshape(1, 64)

    def msm_batch(self, points, scalars, offsets, window_bits=0):
        """m sums over the CSR segments [offsets[s], offsets[s + 1]) of one point / scalar array (bjj_msm_batch): returns
        (out (m, 64) uint8, status (m,) int64).  out[s] and status[s] are what bjj_msm gives for that slice: an empty segment is
        (0, 1) / -1, an off-curve point makes ITS segment (0, 0) with status[s] = its smallest index in `points` -- returned as
        data, not raised.  offsets: m + 1 values, offsets[0] == 0, non-decreasing, offsets[m] == n (BjjError otherwise).
        window_bits: 0 = the library's choice from the mean segment length, 4..20 forces the bucket width."""
        a = _as_u8(points, 64, "points")
        s = _as_u8(scalars, 32, "scalars")
        n = a.size // 64
        if s.size != n * 32:
            raise BjjError("msm_batch: %d points but %d scalars" % (n, s.size // 32))
        try:
            off = np.ascontiguousarray(np.asarray(offsets, dtype=np.uint64).reshape(-1))
        except (OverflowError, ValueError, TypeError) as e:
            raise BjjError("msm_batch: offsets are unsigned 64-bit integers (%s)" % e)
        if off.size < 1:
            raise BjjError("msm_batch: offsets holds m + 1 values")
        m = off.size - 1
        out = np.empty(m * 64, dtype=np.uint8)
        status = np.empty(m, dtype=np.int64)
        self._ck(self.lib.bjj_msm_batch(self.handle, a.ctypes.data if n else None, s.ctypes.data if n else None, n, off.ctypes.data, m,
                                        int(window_bits), out.ctypes.data if m else None, status.ctypes.data if m else None),
                 "bjj_msm_batch")
        return out.reshape(m, 64), status

    def point_sum(self, points, offsets, neg=None):
        """m signed point sums over the CSR segments [offsets[s], offsets[s + 1]) of one point array (bjj_point_sum): returns
        (out (m, 64) uint8, status (m,) int64).  Term i is subtracted where neg[i] != 0 (-(x, y) = (-x, y)); neg=None adds every
        term.  out[s] and status[s] are what msm_batch gives with the scalars 1 and 8l - 1: an empty segment is (0, 1) / -1, an
        off-curve point makes ITS segment (0, 0) with status[s] = its smallest index in `points` -- returned as data, not raised.
        offsets: m + 1 values, offsets[0] == 0, non-decreasing, offsets[m] == n (BjjError otherwise)."""
        a = _as_u8(points, 64, "points")
        n = a.size // 64
        g = None
        if neg is not None:
            g = np.ascontiguousarray(np.asarray(neg).reshape(-1) != 0, dtype=np.uint8)
            if g.size != n:
                raise BjjError("point_sum: %d points but %d signs" % (n, g.size))
        try:
            off = np.ascontiguousarray(np.asarray(offsets, dtype=np.uint64).reshape(-1))
        except (OverflowError, ValueError, TypeError) as e:
            raise BjjError("point_sum: offsets are unsigned 64-bit integers (%s)" % e)
        if off.size < 1:
            raise BjjError("point_sum: offsets holds m + 1 values")
        m = off.size - 1
        out = np.empty(m * 64, dtype=np.uint8)
        status = np.empty(m, dtype=np.int64)
        self._ck(self.lib.bjj_point_sum(self.handle, a.ctypes.data if n else None, g.ctypes.data if g is not None and n else None, n,
                                        off.ctypes.data, m, out.ctypes.data if m else None, status.ctypes.data if m else None),
                 "bjj_point_sum")
        return out.reshape(m, 64), status

    def elgamal_sum(self, c1, c2, offsets, neg=None):
        """the homomorphic sum of exponential-ElGamal ciphertexts per segment: both components summed over the same segments and
        signs (point_sum) -> (C1 (m, 64), C2 (m, 64), status (m,)); (C1[s], C2[s]) decrypts to the signed sum of the segment's
        plaintexts.  status[s]: the smaller non-negative of the two components' status words, or -1."""
        a = _as_u8(c1, 64, "c1")
        b = _as_u8(c2, 64, "c2")
        if b.size != a.size:
            raise BjjError("elgamal_sum: array lengths disagree")
        s1, st1 = self.point_sum(a, offsets, neg)
        s2, st2 = self.point_sum(b, offsets, neg)
        both = (st1 >= 0) & (st2 >= 0)
        status = np.where(both, np.minimum(st1, st2), np.maximum(st1, st2))
        return s1, s2, status

    # ---- fixed-base tables for caller-chosen points (include/bjj_hip_bases.h) ----
    def base(self, point, window_bits=0):
        """a reusable fixed-base table for `point` ((x, y) ints, a Point, or a 64-byte record) -> FixedBase (bjj_base_create).
        window_bits: 0 = 16, or 4..28.  BjjError for a point that is not on the curve.  Freed with close() or with the context."""
        if isinstance(point, Point):
            point = (point.x, point.y)
        rec = _as_u8([tuple(point)] if isinstance(point, (tuple, list)) else point, 64, "point")
        if rec.size != 64:
            raise BjjError("base: exactly one point")
        h = ctypes.c_void_p()
        self._ck(self.lib.bjj_base_create(self.handle, rec.ctypes.data, int(window_bits), ctypes.byref(h)), "bjj_base_create")
        b = FixedBase(self, h)
        self._bases = getattr(self, "_bases", [])
        self._bases.append(b)
        return b

    def _base_args(self, bases, arrays, what):
        t = len(bases)
        if len(arrays) != t:
            raise BjjError("%s: %d bases but %d scalar arrays" % (what, t, len(arrays)))
        handles = []
        for b in bases:
            if b is not None and (not isinstance(b, FixedBase) or b.ctx is not self or not b.handle):
                raise BjjError("%s: a base is a live FixedBase of this context, or None for B8" % what)
            handles.append(b.handle.value if b is not None else None)
        return (ctypes.c_void_p * max(t, 1))(*handles), (ctypes.c_void_p * max(t, 1))(*arrays)

    def mul_bases(self, bases, scalars):
        """out[i] = sum_j scalars[j][i] * P_j in one launch (bjj_mul_bases): bases = FixedBase objects, None = B8; scalars = one
        array of n 32-byte records (or n ints) per base.  Byte for byte the fold of mul_scalar with PointProjective::add, then
        affine() (lib.rs:149-164, 88-131, 70-85).  -> (n, 64)"""
        arrs = [_as_u8(s, 32, "scalars") for s in scalars]
        n = arrs[0].size // 32 if arrs else 0
        if any(a.size != n * 32 for a in arrs):
            raise BjjError("mul_bases: the scalar arrays differ in length")
        hb, hs = self._base_args(list(bases), [a.ctypes.data for a in arrs], "mul_bases")
        out = np.empty(n * 64, dtype=np.uint8)
        self._ck(self.lib.bjj_mul_bases(self.handle, hb, len(arrs), hs, n, out.ctypes.data), "bjj_mul_bases")
        return out.reshape(n, 64)

    def mul_bases_dev(self, bases, d_scalars, n, d_out, stream=0):
        """bjj_mul_bases_dev: d_scalars = one device address per base (n 32-byte records each), d_out = n 64-byte records"""
        hb, hs = self._base_args(list(bases), [int(p) for p in d_scalars], "mul_bases_dev")
        self._ck(self.lib.bjj_mul_bases_dev(self.handle, hb, len(d_scalars), hs, n, d_out, stream), "bjj_mul_bases_dev")

    # ---- verification against one signer's table (include/bjj_hip_signer.h) ----
    def _signer_handle(self, base, what):
        if not isinstance(base, FixedBase) or base.ctx is not self or not base.handle:
            raise BjjError("%s: the signer is a live FixedBase of this context" % what)
        return base.handle.value

    def _verify_signer(self, fn, name, base, r, s, msg):
        h = self._signer_handle(base, name)
        rr = _as_u8(r, 64, "r")
        sv = _as_u8(s, 32, "s")
        m = _as_u8(msg, 32, "msg")
        n = sv.size // 32
        if rr.size != n * 64 or m.size != n * 32:
            raise BjjError("%s: array lengths disagree" % name)
        ok = np.empty(n, dtype=np.uint8)
        self._ck(fn(self.handle, h, rr.ctypes.data, sv.ctypes.data, m.ctypes.data, n, ok.ctypes.data), "bjj_" + name)
        return ok

    def eddsa_verify_signer(self, base, r_b8, s, msg):
        """eddsa_verify for the ONE public key whose table `base` (a FixedBase of this context) holds: the same bytes as
        eddsa_verify with that key repeated, from table gathers alone (bjj_eddsa_verify_signer).  -> (n,) uint8"""
        return self._verify_signer(self.lib.bjj_eddsa_verify_signer, "eddsa_verify_signer", base, r_b8, s, msg)

    def schnorr_verify_signer(self, base, r, s, msg):
        """schnorr_verify for the one public key of `base`: 1 / 0 = Ok(true / false), 2 = Err (msg > Q)"""
        return self._verify_signer(self.lib.bjj_schnorr_verify_signer, "schnorr_verify_signer", base, r, s, msg)

    def eddsa_verify_signer_dev(self, base, d_r, d_s, d_msg, n, d_ok, stream=0):
        self._ck(self.lib.bjj_eddsa_verify_signer_dev(self.handle, self._signer_handle(base, "eddsa_verify_signer_dev"), d_r, d_s, d_msg, n,
                                                      d_ok, stream), "bjj_eddsa_verify_signer_dev")

    def schnorr_verify_signer_dev(self, base, d_r, d_s, d_msg, n, d_ok, stream=0):
        self._ck(self.lib.bjj_schnorr_verify_signer_dev(self.handle, self._signer_handle(base, "schnorr_verify_signer_dev"), d_r, d_s, d_msg,
                                                        n, d_ok, stream), "bjj_schnorr_verify_signer_dev")

    # ---- verification against a set of signers' tables, by per-item index (include/bjj_hip_signer_set.h) ----
    def signer_set(self, pks, window_bits=0):
        """the fixed-base tables of k public keys in one device allocation -> SignerSet (bjj_signer_set_create).  pks: k points
        ((x, y) ints) or k 64-byte records.  window_bits: 0 = 8, or 4..16.  BjjError names the first key that is not on the curve.
        BjjError.code is the library's return code (BJJ_E_NOMEM when the device refuses the allocation).  Freed with close() or with
        the context."""
        rec = _as_u8(pks, 64, "pks")
        k = rec.size // 64
        h, first = ctypes.c_void_p(), ctypes.c_int64(-1)
        rc = self.lib.bjj_signer_set_create(self.handle, rec.ctypes.data if k else None, k, int(window_bits), ctypes.byref(h), ctypes.byref(first))
        if rc != _lib.BJJ_OK and first.value >= 0:
            raise BjjError("signer_set: key %d is not on the curve" % first.value, rc)
        self._ck(rc, "bjj_signer_set_create")
        t = SignerSet(self, h)
        self._sets.append(t)
        return t

    def _set_handle(self, sset, what):
        if not isinstance(sset, SignerSet) or sset.ctx is not self or not sset.handle:
            raise BjjError("%s: the set is a live SignerSet of this context" % what)
        return sset.handle.value

    def _verify_set(self, fn, name, sset, idx, r, s, msg):
        h = self._set_handle(sset, name)
        a = np.asarray(idx).reshape(-1)
        if a.dtype.kind not in "ui" or (a.size and (int(a.min()) < 0 or int(a.max()) > 0xFFFFFFFF)):
            raise BjjError("%s: signer indices are unsigned 32-bit integers" % name)
        ix = np.ascontiguousarray(a, dtype=np.uint32)
        rr = _as_u8(r, 64, "r")
        sv = _as_u8(s, 32, "s")
        m = _as_u8(msg, 32, "msg")
        n = sv.size // 32
        if ix.size != n or rr.size != n * 64 or m.size != n * 32:
            raise BjjError("%s: array lengths disagree" % name)
        ok = np.empty(n, dtype=np.uint8)
        self._ck(fn(self.handle, h, ix.ctypes.data, rr.ctypes.data, sv.ctypes.data, m.ctypes.data, n, ok.ctypes.data), "bjj_" + name)
        return ok

    def eddsa_verify_set_dev(self, sset, d_idx, d_r, d_s, d_msg, n, d_ok, stream=0):
        """bjj_eddsa_verify_set_dev: d_idx = n uint32 signer indices; the other arrays as eddsa_verify_signer_dev"""
        self._ck(self.lib.bjj_eddsa_verify_set_dev(self.handle, self._set_handle(sset, "eddsa_verify_set_dev"), d_idx, d_r, d_s, d_msg, n,
                                                   d_ok, stream), "bjj_eddsa_verify_set_dev")

    def schnorr_verify_set_dev(self, sset, d_idx, d_r, d_s, d_msg, n, d_ok, stream=0):
        self._ck(self.lib.bjj_schnorr_verify_set_dev(self.handle, self._set_handle(sset, "schnorr_verify_set_dev"), d_idx, d_r, d_s, d_msg, n,
                                                     d_ok, stream), "bjj_schnorr_verify_set_dev")

    # ---- small-range discrete logarithms (include/bjj_hip_dlog.h) ----
    def dlog_table(self, point=None, baby_bits=0):
        """the baby-step table of a base point G -> DlogTable (bjj_dlog_table_create).  point: (x, y) ints or a 64-byte record,
        None = B8.  baby_bits: 0 = 24 (512 MiB), or 4..28.  BjjError (code BJJ_E_INVALID) for a point off the curve or of order <= 8.  Freed
        with close() or with the context."""
        rec = None if point is None else _as_u8([point] if isinstance(point, tuple) else point, 64, "point")
        if rec is not None and rec.size != 64:
            raise BjjError("dlog_table: one point")
        h = ctypes.c_void_p()
        self._ck(self.lib.bjj_dlog_table_create(self.handle, None if rec is None else rec.ctypes.data, int(baby_bits), ctypes.byref(h)),
                 "bjj_dlog_table_create")
        t = DlogTable(self, h)
        self._dlogs.append(t)
        return t

    def _dlog_handle(self, table, what):
        if not isinstance(table, DlogTable) or table.ctx is not self or not table.handle:
            raise BjjError("%s: the table is a live DlogTable of this context" % what)
        return table.handle.value

    def dlog(self, table, points, range_bits):
        """m with m * G = points[i], 0 <= m < 2^range_bits -> (m: (n,) uint64, ok: (n,) uint8): ok 1 = found, 0 = not in range
        (m = 2^64 - 1), 2 = the point is not on the curve (bjj_dlog)"""
        h = self._dlog_handle(table, "dlog")
        p = _as_u8(points, 64, "points")
        n = p.size // 64
        m = np.empty(n, dtype=np.uint64)
        ok = np.empty(n, dtype=np.uint8)
        self._ck(self.lib.bjj_dlog(self.handle, h, p.ctypes.data, n, int(range_bits), m.ctypes.data, ok.ctypes.data), "bjj_dlog")
        return m, ok

    def dlog_dev(self, table, d_pts, n, range_bits, d_out_m, d_ok, stream=0):
        """bjj_dlog_dev: d_pts = n 64-byte records, d_out_m = n uint64, d_ok = n bytes, all on the device"""
        self._ck(self.lib.bjj_dlog_dev(self.handle, self._dlog_handle(table, "dlog_dev"), d_pts, n, int(range_bits), d_out_m, d_ok, stream),
                 "bjj_dlog_dev")

    def elgamal_decrypt(self, table, sk, c1, c2, range_bits):
        """exponential ElGamal: m from (C1, C2) = (r * G, m * G + r * PK) with PK = sk * G and `table` the DlogTable of G ->
        (m, ok) as dlog().  M = C2 - sk * C1 by mul_var_base and point_add (-(x, y) = (-x, y), negated on the host), then the
        logarithm of M.  A wrong key gives ok = 0, not a wrong m."""
        a = _as_u8(c1, 64, "c1")
        b = _as_u8(c2, 64, "c2")
        n = a.size // 64
        if b.size != a.size:
            raise BjjError("elgamal_decrypt: array lengths disagree")
        if n == 0:
            return np.empty(0, dtype=np.uint64), np.empty(0, dtype=np.uint8)
        t = self.mul_var_base(a, np.tile(_as_u8([int(sk)], 32, "sk"), n))
        return self.dlog(table, self.point_add(b, _negate_x(t)), range_bits)

    # ---- one scalar, many points (include/bjj_hip_common_scalar.h) ----
    @staticmethod
    def _scalar32(scalar, name):
        """one 32-byte little-endian scalar on the host: an int below 2^256 or 32 bytes"""
        a = _as_u8([int(scalar)] if isinstance(scalar, int) else scalar, 32, name)
        if a.size != 32:
            raise BjjError("%s: one 32-byte scalar" % name)
        return a

    def mul_common(self, scalar, points, add=None, subtract=False):
        """out[i] = add[i] + scalar * points[i] (subtract: add[i] - scalar * points[i]; add=None: the identity) with ONE scalar for
        the call -> (out: (n, 64) uint8, ok: (n,) uint8).  ok 1 = computed, 2 = points[i] or add[i] is not on the curve and
        out[i] = (0, 0) (bjj_mul_common).  Not constant time in the scalar."""
        k = self._scalar32(scalar, "scalar")
        p = _as_u8(points, 64, "points")
        n = p.size // 64
        a = None if add is None else _as_u8(add, 64, "add")
        if a is not None and a.size != p.size:
            raise BjjError("mul_common: array lengths disagree")
        out = np.empty(n * 64, dtype=np.uint8)
        ok = np.empty(n, dtype=np.uint8)
        self._ck(self.lib.bjj_mul_common(self.handle, k.ctypes.data, p.ctypes.data, None if a is None else a.ctypes.data, 1 if subtract else 0,
                                         n, out.ctypes.data, ok.ctypes.data), "bjj_mul_common")
        return out.reshape(n, 64), ok

    def mul_common_dev(self, scalar, d_pts, d_add, n, d_out, d_ok, subtract=False, stream=0):
        """bjj_mul_common_dev: the scalar on the HOST (int or 32 bytes, read before the call returns); d_add = None for no addend;
        d_out = n 64-byte records, d_ok = n bytes, on the device"""
        k = self._scalar32(scalar, "scalar")
        self._ck(self.lib.bjj_mul_common_dev(self.handle, k.ctypes.data, d_pts, d_add, 1 if subtract else 0, n, d_out, d_ok, stream),
                 "bjj_mul_common_dev")

    def in_subgroup(self, points):
        """l * points[i] == identity -> ok: (n,) uint8: 1 = in the prime-order subgroup, 0 = on the curve but not in it, 2 = not on
        the curve (bjj_in_subgroup)"""
        p = _as_u8(points, 64, "points")
        n = p.size // 64
        ok = np.empty(n, dtype=np.uint8)
        self._ck(self.lib.bjj_in_subgroup(self.handle, p.ctypes.data, n, ok.ctypes.data), "bjj_in_subgroup")
        return ok

    def in_subgroup_dev(self, d_pts, n, d_ok, stream=0):
        self._ck(self.lib.bjj_in_subgroup_dev(self.handle, d_pts, n, d_ok, stream), "bjj_in_subgroup_dev")

    def decrypt(self, table, sk, c1, c2, range_bits):
        """exponential ElGamal in one call: (m, ok) as dlog() for M = c2 - sk * c1 (bjj_elgamal_decrypt); elgamal_decrypt() is
        the same result by four calls"""
        h = self._dlog_handle(table, "decrypt")
        k = self._scalar32(sk, "sk")
        a = _as_u8(c1, 64, "c1")
        b = _as_u8(c2, 64, "c2")
        n = a.size // 64
        if b.size != a.size:
            raise BjjError("decrypt: array lengths disagree")
        m = np.empty(n, dtype=np.uint64)
        ok = np.empty(n, dtype=np.uint8)
        self._ck(self.lib.bjj_elgamal_decrypt(self.handle, h, k.ctypes.data, a.ctypes.data, b.ctypes.data, n, int(range_bits), m.ctypes.data,
                                              ok.ctypes.data), "bjj_elgamal_decrypt")
        return m, ok

    def decrypt_dev(self, table, sk, d_c1, d_c2, n, range_bits, d_out_m, d_ok, stream=0):
        """bjj_elgamal_decrypt_dev: sk on the HOST; d_c1, d_c2 = n 64-byte records, d_out_m = n uint64, d_ok = n bytes, on the device"""
        k = self._scalar32(sk, "sk")
        self._ck(self.lib.bjj_elgamal_decrypt_dev(self.handle, self._dlog_handle(table, "decrypt_dev"), k.ctypes.data, d_c1, d_c2, n,
                                                  int(range_bits), d_out_m, d_ok, stream), "bjj_elgamal_decrypt_dev")

    # ---- encryption and re-randomisation in one launch (include/bjj_hip_elgamal.h) ----
    def _elgamal_handles(self, g, pk, what):
        for b, name in ((g, "g"), (pk, "pk")):
            if b is None and name == "g":
                continue
            if not isinstance(b, FixedBase) or b.ctx is not self or not b.handle:
                raise BjjError("%s: %s is a live FixedBase of this context%s" % (what, name, ", or None for B8" if name == "g" else ""))
        return (None if g is None else g.handle.value), pk.handle.value

    def elgamal_encrypt(self, pk, m, r, g=None, add=None):
        """exponential ElGamal to the key whose table `pk` is (a FixedBase): c1[i] = r[i] * G, c2[i] = m[i] * G + r[i] * PK in ONE
        launch (bjj_elgamal_encrypt) -> (c1, c2), (n, 64) uint8 each.  m: n integers below 2^64 (or a uint64 array), None = all 0;
        r: n 32-byte records (or ints); g: the FixedBase of G, None = B8.  add=(a1, a2): c1[i] = a1[i] + .., c2[i] = a2[i] + .. and
        -> (c1, c2, ok) with ok 1 = computed, 2 = a1[i] or a2[i] is not on the curve and both outputs are (0, 0).  Byte for byte
        the composition of mul_bases and point_add.  Not constant time."""
        hg, hpk = self._elgamal_handles(g, pk, "elgamal_encrypt")
        rr = _as_u8(r, 32, "r")
        n = rr.size // 32
        mm = None
        if m is not None:
            mm = np.ascontiguousarray(m if isinstance(m, np.ndarray) and m.dtype == np.uint64 else np.array([int(x) for x in m], dtype=np.uint64))
            if mm.size != n:
                raise BjjError("elgamal_encrypt: array lengths disagree")
        a1 = a2 = None
        if add is not None:
            a1, a2 = _as_u8(add[0], 64, "add c1"), _as_u8(add[1], 64, "add c2")
            if a1.size != n * 64 or a2.size != n * 64:
                raise BjjError("elgamal_encrypt: array lengths disagree")
        c1, c2 = np.empty(n * 64, dtype=np.uint8), np.empty(n * 64, dtype=np.uint8)
        ok = np.empty(n, dtype=np.uint8)
        self._ck(self.lib.bjj_elgamal_encrypt(self.handle, hg, hpk, None if mm is None else mm.ctypes.data, rr.ctypes.data,
                                              None if a1 is None else a1.ctypes.data, None if a2 is None else a2.ctypes.data, n,
                                              c1.ctypes.data, c2.ctypes.data, ok.ctypes.data), "bjj_elgamal_encrypt")
        c1, c2 = c1.reshape(n, 64), c2.reshape(n, 64)
        return (c1, c2) if add is None else (c1, c2, ok)

    def elgamal_rerandomize(self, pk, c1, c2, r, g=None):
        """C' = C + Enc(0, r): c1 + r * G, c2 + r * PK -> (c1, c2, ok), as elgamal_encrypt(pk, None, r, g, add=(c1, c2)); the m-chain
        is not run"""
        return self.elgamal_encrypt(pk, None, r, g=g, add=(c1, c2))

    def elgamal_encrypt_dev(self, pk, d_m, d_r, n, d_c1, d_c2, g=None, d_add_c1=None, d_add_c2=None, d_ok=None, stream=0):
        """bjj_elgamal_encrypt_dev: d_m = n uint64 or None, d_r = n 32-byte records, d_add_c1 / d_add_c2 = n 64-byte records each
        or both None, d_c1 / d_c2 = n 64-byte records (they may BE d_add_c1 / d_add_c2: in place), d_ok = n bytes (required with add
        arrays), on the device"""
        hg, hpk = self._elgamal_handles(g, pk, "elgamal_encrypt_dev")
        self._ck(self.lib.bjj_elgamal_encrypt_dev(self.handle, hg, hpk, d_m, d_r, d_add_c1, d_add_c2, n, d_c1, d_c2, d_ok, stream),
                 "bjj_elgamal_encrypt_dev")

    # ---- a * P + b * Q and proofs of correct decryption (include/bjj_hip_dleq.h) ----
    def mul_pair(self, p, a, q, b, add=None):
        """out[i] = add[i] + a[i] * p[i] + b[i] * q[i] in ONE launch (bjj_mul_pair; add=None: the identity) -> (out: (n, 64) uint8,
        ok: (n,) uint8).  a, b: n 32-byte records (or ints) of any value, reduced mod 8l.  ok 1 = computed, 2 = p[i], q[i] or add[i] is
        not on the curve and out[i] = (0, 0).  Byte for byte the composition of mul_var_base and point_add for on-curve points.  Not
        constant time."""
        pp, qq = _as_u8(p, 64, "p"), _as_u8(q, 64, "q")
        aa, bb = _as_u8(a, 32, "a"), _as_u8(b, 32, "b")
        n = pp.size // 64
        ad = None if add is None else _as_u8(add, 64, "add")
        if qq.size != n * 64 or aa.size != n * 32 or bb.size != n * 32 or (ad is not None and ad.size != n * 64):
            raise BjjError("mul_pair: array lengths disagree")
        out = np.empty(n * 64, dtype=np.uint8)
        ok = np.empty(n, dtype=np.uint8)
        self._ck(self.lib.bjj_mul_pair(self.handle, pp.ctypes.data, aa.ctypes.data, qq.ctypes.data, bb.ctypes.data,
                                       None if ad is None else ad.ctypes.data, n, out.ctypes.data, ok.ctypes.data), "bjj_mul_pair")
        return out.reshape(n, 64), ok

    def mul_pair_dev(self, d_p, d_a, d_q, d_b, d_add, n, d_out, d_ok, stream=0):
        """bjj_mul_pair_dev: d_p, d_q, d_out = n 64-byte records, d_a, d_b = n 32-byte records, d_add = n 64-byte records or None,
        d_ok = n bytes, on the device"""
        self._ck(self.lib.bjj_mul_pair_dev(self.handle, d_p, d_a, d_q, d_b, d_add, n, d_out, d_ok, stream), "bjj_mul_pair_dev")

    def dleq_tag(self, g_xy, pk_xy, label=0):
        """a transcript tag that binds G and PK: Poseidon5(G.x, G.y, PK.x, PK.y, label) through bjj_poseidon5 -> 32 bytes (uint8).
        g_xy, pk_xy: one 64-byte point (or an (x, y) pair of ints) each; label: an int below 2^256."""
        gg, kk = _as_u8([tuple(g_xy)] if isinstance(g_xy, (tuple, list)) else g_xy, 64, "g_xy"), \
            _as_u8([tuple(pk_xy)] if isinstance(pk_xy, (tuple, list)) else pk_xy, 64, "pk_xy")
        if gg.size != 64 or kk.size != 64:
            raise BjjError("dleq_tag: one 64-byte point each for G and PK")
        rec = np.concatenate([gg, kk, self._scalar32(label, "label")])
        return np.ascontiguousarray(self.poseidon5(rec.reshape(1, 160))).reshape(-1).view(np.uint8)[:32].copy()

    def dleq_verify(self, pk, tag, c1, d, a, b, z, g=None):
        """ok[i] for the proof (a[i], b[i], z[i]) that log_G PK = log_c1[i] d[i] (bjj_dleq_verify): 1 = accepted, 0 = rejected (the
        equations fail, or a proof field is not canonical), 2 = c1[i] or d[i] is not on the curve.  pk: the FixedBase of PK; g: the
        FixedBase of G, None = B8; tag: an int or 32 bytes (dleq_tag).  Check c1 and d with in_subgroup first."""
        hg, hpk = self._elgamal_handles(g, pk, "dleq_verify")
        t = self._scalar32(tag, "tag")
        cc, dd, aa, bb = _as_u8(c1, 64, "c1"), _as_u8(d, 64, "d"), _as_u8(a, 64, "a"), _as_u8(b, 64, "b")
        zz = _as_u8(z, 32, "z")
        n = cc.size // 64
        if dd.size != n * 64 or aa.size != n * 64 or bb.size != n * 64 or zz.size != n * 32:
            raise BjjError("dleq_verify: array lengths disagree")
        ok = np.empty(n, dtype=np.uint8)
        self._ck(self.lib.bjj_dleq_verify(self.handle, hg, hpk, t.ctypes.data, cc.ctypes.data, dd.ctypes.data, aa.ctypes.data, bb.ctypes.data,
                                          zz.ctypes.data, n, ok.ctypes.data), "bjj_dleq_verify")
        return ok

    def dleq_verify_dev(self, pk, tag, d_c1, d_d, d_a, d_b, d_z, n, d_ok, g=None, stream=0):
        """bjj_dleq_verify_dev: the tag on the HOST; d_c1, d_d, d_a, d_b = n 64-byte records, d_z = n 32-byte records, d_ok = n bytes,
        on the device"""
        hg, hpk = self._elgamal_handles(g, pk, "dleq_verify_dev")
        t = self._scalar32(tag, "tag")
        self._ck(self.lib.bjj_dleq_verify_dev(self.handle, hg, hpk, t.ctypes.data, d_c1, d_d, d_a, d_b, d_z, n, d_ok, stream),
                 "bjj_dleq_verify_dev")

    def _dleq_g(self, g, what):
        if g is None:
            return None
        if not isinstance(g, FixedBase) or g.ctx is not self or not g.handle:
            raise BjjError("%s: g is a live FixedBase of this context, or None for B8" % what)
        return g.handle.value

    def dleq_prove(self, sk, tag, c1, w, g=None):
        """the partial decryptions d[i] = sk * c1[i] with their proofs (bjj_dleq_prove) -> (d, a, b: (n, 64) uint8, z: (n, 32) uint8,
        ok: (n,) uint8).  sk, tag: an int or 32 bytes; w: n 32-byte nonces (or ints) -- fresh, uniform and secret per item; g: the
        FixedBase of G, None = B8.  ok 1 = computed, 2 = c1[i] is not on the curve and the four outputs are zero.  Not constant time."""
        hg = self._dleq_g(g, "dleq_prove")
        k, t = self._scalar32(sk, "sk"), self._scalar32(tag, "tag")
        cc, ww = _as_u8(c1, 64, "c1"), _as_u8(w, 32, "w")
        n = cc.size // 64
        if ww.size != n * 32:
            raise BjjError("dleq_prove: array lengths disagree")
        d, a, b = (np.empty(n * 64, dtype=np.uint8) for _ in range(3))
        z = np.empty(n * 32, dtype=np.uint8)
        ok = np.empty(n, dtype=np.uint8)
        self._ck(self.lib.bjj_dleq_prove(self.handle, hg, k.ctypes.data, t.ctypes.data, cc.ctypes.data, ww.ctypes.data, n, d.ctypes.data,
                                         a.ctypes.data, b.ctypes.data, z.ctypes.data, ok.ctypes.data), "bjj_dleq_prove")
        return d.reshape(n, 64), a.reshape(n, 64), b.reshape(n, 64), z.reshape(n, 32), ok

    def dleq_prove_dev(self, sk, tag, d_c1, d_w, n, d_d, d_a, d_b, d_z, d_ok, g=None, stream=0):
        """bjj_dleq_prove_dev: sk and the tag on the HOST (read before the call returns); d_c1, d_d, d_a, d_b = n 64-byte records,
        d_w, d_z = n 32-byte records, d_ok = n bytes, on the device"""
        hg = self._dleq_g(g, "dleq_prove_dev")
        k, t = self._scalar32(sk, "sk"), self._scalar32(tag, "tag")
        self._ck(self.lib.bjj_dleq_prove_dev(self.handle, hg, k.ctypes.data, t.ctypes.data, d_c1, d_w, n, d_d, d_a, d_b, d_z, d_ok, stream),
                 "bjj_dleq_prove_dev")

    def set_signer_constant_time(self, on=True):
        """signer hardening: public_keys / sign / sign_schnorr scan a small 4-bit table instead of indexing the big one
        with secret digits -- no secret-dependent address or branch; bit-identical results, ~2x slower sign"""
        self._ck(self.lib.bjj_set_signer_constant_time(self.handle, 1 if on else 0), "bjj_set_signer_constant_time")

    def scalar_keys(self, keys):
        a = _as_u8(keys, 32, "keys")
        n = a.size // 32
        out = np.empty(n * 32, dtype=np.uint8)
        self._ck(self.lib.bjj_scalar_keys(self.handle, a.ctypes.data, n, out.ctypes.data), "bjj_scalar_keys")
        return out.reshape(n, 32)

    def public_keys(self, keys):
        a = _as_u8(keys, 32, "keys")
        n = a.size // 32
        out = np.empty(n * 64, dtype=np.uint8)
        self._ck(self.lib.bjj_public_keys(self.handle, a.ctypes.data, n, out.ctypes.data), "bjj_public_keys")
        return out.reshape(n, 64)

    def public_keys_compressed(self, keys):
        """sk.public().compress() in one pass (lib.rs:304-306 + 166-178) -> (n, 32)"""
        a = _as_u8(keys, 32, "keys")
        n = a.size // 32
        out = np.empty(n * 32, dtype=np.uint8)
        self._ck(self.lib.bjj_public_keys_compressed(self.handle, a.ctypes.data, n, out.ctypes.data), "bjj_public_keys_compressed")
        return out.reshape(n, 32)

    def sign_compressed(self, keys, msgs):
        """sk.sign(msg)?.compress() in one pass (lib.rs:308-342 + 245-258) -> (sig (n, 64), ok (n,)); ok == 0 (sig all-zero) for Err"""
        a = _as_u8(keys, 32, "keys")
        m = _as_u8(msgs, 32, "msgs")
        n = a.size // 32
        if m.size != a.size:
            raise BjjError("sign_compressed: array lengths disagree")
        sig = np.empty(n * 64, dtype=np.uint8)
        ok = np.empty(n, dtype=np.uint8)
        self._ck(self.lib.bjj_sign_compressed(self.handle, a.ctypes.data, m.ctypes.data, n, sig.ctypes.data, ok.ctypes.data), "bjj_sign_compressed")
        return sig.reshape(n, 64), ok

    def sign(self, keys, msgs):
        """-> (r_b8 (n, 64), s (n, 32), ok (n,)); ok == 0 where the reference returns Err (msg > Q)"""
        a = _as_u8(keys, 32, "keys")
        m = _as_u8(msgs, 32, "msgs")
        n = a.size // 32
        if m.size != a.size:
            raise BjjError("sign: array lengths disagree")
        r = np.empty(n * 64, dtype=np.uint8)
        s = np.empty(n * 32, dtype=np.uint8)
        ok = np.empty(n, dtype=np.uint8)
        self._ck(self.lib.bjj_sign(self.handle, a.ctypes.data, m.ctypes.data, n, r.ctypes.data, s.ctypes.data,
                                   ok.ctypes.data), "bjj_sign")
        return r.reshape(n, 64), s.reshape(n, 32), ok

    def sign_schnorr(self, keys, msgs, nonces):
        """PrivateKey::sign_schnorr in bulk with caller-supplied 1024-bit nonces (n x 128 bytes, little-endian).
        -> (r (n, 64), s (n, 160): the reference's unreduced k + scalar_key*h, ok (n,): 0 = Err (msg > Q))"""
        a = _as_u8(keys, 32, "keys")
        m = _as_u8(msgs, 32, "msgs")
        k = np.ascontiguousarray(np.asarray(nonces, dtype=np.uint8)).reshape(-1)
        n = a.size // 32
        if m.size != a.size or k.size != n * 128:
            raise BjjError("sign_schnorr: array lengths disagree (nonces are 128 bytes each)")
        r = np.empty(n * 64, dtype=np.uint8)
        s = np.empty(n * 160, dtype=np.uint8)
        ok = np.empty(n, dtype=np.uint8)
        self._ck(self.lib.bjj_sign_schnorr(self.handle, a.ctypes.data, m.ctypes.data, k.ctypes.data, n, r.ctypes.data,
                                           s.ctypes.data, ok.ctypes.data), "bjj_sign_schnorr")
        return r.reshape(n, 64), s.reshape(n, 160), ok

    def sign_schnorr_dev(self, d_keys, d_msgs, d_nonces, n, d_r, d_s, d_ok, stream=0):
        self._ck(self.lib.bjj_sign_schnorr_dev(self.handle, d_keys, d_msgs, d_nonces, n, d_r, d_s, d_ok, stream),
                 "bjj_sign_schnorr_dev")

    def sign_dev(self, d_keys, d_msgs, n, d_r, d_s, d_ok, stream=0):
        self._ck(self.lib.bjj_sign_dev(self.handle, d_keys, d_msgs, n, d_r, d_s, d_ok, stream), "bjj_sign_dev")

    def compress_points(self, points):
        a = _as_u8(points, 64, "points")
        n = a.size // 64
        out = np.empty(n * 32, dtype=np.uint8)
        self._ck(self.lib.bjj_compress_points(self.handle, a.ctypes.data, n, out.ctypes.data), "bjj_compress_points")
        return out.reshape(n, 32)

    def decompress_points(self, comp):
        """-> (points (n, 64), ok (n,)): ok == 0 where the reference's decompress_point returns Err"""
        a = _as_u8(comp, 32, "compressed points")
        n = a.size // 32
        out = np.empty(n * 64, dtype=np.uint8)
        ok = np.empty(n, dtype=np.uint8)
        self._ck(self.lib.bjj_decompress_points(self.handle, a.ctypes.data, n, out.ctypes.data, ok.ctypes.data),
                 "bjj_decompress_points")
        return out.reshape(n, 64), ok

    def eddsa_verify_compressed(self, pk, sig, msg):
        """pk (n, 32), sig (n, 64) = compressed R then s, msg (n, 32) -> 1 / 0 / 2 (decompression Err)"""
        a = _as_u8(pk, 32, "pk")
        g = _as_u8(sig, 64, "sig")
        m = _as_u8(msg, 32, "msg")
        n = a.size // 32
        if g.size != n * 64 or m.size != n * 32:
            raise BjjError("eddsa_verify_compressed: array lengths disagree")
        ok = np.empty(n, dtype=np.uint8)
        self._ck(self.lib.bjj_eddsa_verify_compressed(self.handle, a.ctypes.data, g.ctypes.data, m.ctypes.data, n,
                                                      ok.ctypes.data), "bjj_eddsa_verify_compressed")
        return ok

    # ---- device-pointer calls (integers: device addresses / hipStream_t) ----
    def mul_fixed_base_dev(self, d_scalars, n, d_out, stream=0):
        self._ck(self.lib.bjj_mul_fixed_base_dev(self.handle, d_scalars, n, d_out, stream), "bjj_mul_fixed_base_dev")

    def mul_var_base_dev(self, d_pts, d_scalars, n, d_out, stream=0):
        self._ck(self.lib.bjj_mul_var_base_dev(self.handle, d_pts, d_scalars, n, d_out, stream), "bjj_mul_var_base_dev")

    def poseidon5_dev(self, d_in, n, d_out, stream=0):
        self._ck(self.lib.bjj_poseidon5_dev(self.handle, d_in, n, d_out, stream), "bjj_poseidon5_dev")

    def eddsa_verify_dev(self, d_pk, d_r, d_s, d_msg, n, d_ok, stream=0):
        self._ck(self.lib.bjj_eddsa_verify_dev(self.handle, d_pk, d_r, d_s, d_msg, n, d_ok, stream),
                 "bjj_eddsa_verify_dev")

    def eddsa_verify_compressed_dev(self, d_pk, d_sig, d_msg, n, d_ok, stream=0):
        self._ck(self.lib.bjj_eddsa_verify_compressed_dev(self.handle, d_pk, d_sig, d_msg, n, d_ok, stream),
                 "bjj_eddsa_verify_compressed_dev")

    def decompress_points_dev(self, d_in, n, d_out, d_ok, stream=0):
        self._ck(self.lib.bjj_decompress_points_dev(self.handle, d_in, n, d_out, d_ok, stream),
                 "bjj_decompress_points_dev")

    def compress_points_dev(self, d_pts, n, d_out, stream=0):
        self._ck(self.lib.bjj_compress_points_dev(self.handle, d_pts, n, d_out, stream), "bjj_compress_points_dev")

    def msm_batch_dev(self, d_pts, d_scalars, n, d_offsets, m, d_out, d_first_off_curve, window_bits=0, stream=0):
        """bjj_msm_batch_dev: m 64-byte results and m int64 status words written by the device (-1, the smallest off-curve index of
        the segment, or -2 in every word when the (m + 1) uint64 offsets break their contract)"""
        self._ck(self.lib.bjj_msm_batch_dev(self.handle, d_pts, d_scalars, n, d_offsets, m, int(window_bits), d_out, d_first_off_curve,
                                            stream), "bjj_msm_batch_dev")

    def point_sum_dev(self, d_pts, d_neg, n, d_offsets, m, d_out, d_first_off_curve, stream=0):
        """bjj_point_sum_dev: d_neg = n sign bytes at any address, or None; m 64-byte results and m int64 status words written by
        the device (-1, the smallest off-curve index of the segment, or -2 in every word when the (m + 1) uint64 offsets break
        their contract)"""
        self._ck(self.lib.bjj_point_sum_dev(self.handle, d_pts, d_neg, n, d_offsets, m, d_out, d_first_off_curve, stream),
                 "bjj_point_sum_dev")

    def msm_dev(self, d_pts, d_scalars, n, d_out, d_first_off_curve, window_bits=0, stream=0):
        """bjj_msm_dev: 64-byte result and the int64 status word (-1, or the smallest off-curve index) written by the device"""
        self._ck(self.lib.bjj_msm_dev(self.handle, d_pts, d_scalars, n, int(window_bits), d_out, d_first_off_curve, stream),
                 "bjj_msm_dev")

    def point_add_dev(self, d_p, d_q, n, d_out, stream=0):
        self._ck(self.lib.bjj_point_add_dev(self.handle, d_p, d_q, n, d_out, stream), "bjj_point_add_dev")

    def proj_add_dev(self, d_p, d_q, n, d_out, stream=0):
        self._ck(self.lib.bjj_proj_add_dev(self.handle, d_p, d_q, n, d_out, stream), "bjj_proj_add_dev")

    def proj_affine_dev(self, d_p, n, d_out, stream=0):
        self._ck(self.lib.bjj_proj_affine_dev(self.handle, d_p, n, d_out, stream), "bjj_proj_affine_dev")

    def mul_var_base_wide_dev(self, d_pts, d_scalars, scalar_bytes, n, d_out, stream=0):
        self._ck(self.lib.bjj_mul_var_base_wide_dev(self.handle, d_pts, d_scalars, scalar_bytes, n, d_out, stream),
                 "bjj_mul_var_base_wide_dev")

    def public_keys_dev(self, d_keys, n, d_out, stream=0):
        self._ck(self.lib.bjj_public_keys_dev(self.handle, d_keys, n, d_out, stream), "bjj_public_keys_dev")

    def mul_fixed_base_compressed_dev(self, d_scalars, n, d_out32, stream=0):
        self._ck(self.lib.bjj_mul_fixed_base_compressed_dev(self.handle, d_scalars, n, d_out32, stream), "bjj_mul_fixed_base_compressed_dev")

    def public_keys_compressed_dev(self, d_keys, n, d_out32, stream=0):
        self._ck(self.lib.bjj_public_keys_compressed_dev(self.handle, d_keys, n, d_out32, stream), "bjj_public_keys_compressed_dev")

    def sign_compressed_dev(self, d_keys, d_msgs, n, d_sig64, d_ok, stream=0):
        self._ck(self.lib.bjj_sign_compressed_dev(self.handle, d_keys, d_msgs, n, d_sig64, d_ok, stream), "bjj_sign_compressed_dev")

    def scalar_keys_dev(self, d_keys, n, d_out, stream=0):
        self._ck(self.lib.bjj_scalar_keys_dev(self.handle, d_keys, n, d_out, stream), "bjj_scalar_keys_dev")

    def schnorr_verify_dev(self, d_pk, d_r, d_s, d_msg, n, d_ok, stream=0):
        self._ck(self.lib.bjj_schnorr_verify_dev(self.handle, d_pk, d_r, d_s, d_msg, n, d_ok, stream),
                 "bjj_schnorr_verify_dev")


class FixedBase:
    """A fixed-base table for one curve point (bjj_base, include/bjj_hip_bases.h); made by Context.base()."""

    def __init__(self, ctx, handle):
        self.ctx, self.handle = ctx, handle

    def close(self):
        """bjj_base_free: waits for the context's enqueued work, then releases the table"""
        if getattr(self, "handle", None) and getattr(self.ctx, "handle", None):
            self.ctx._ck(self.ctx.lib.bjj_base_free(self.ctx.handle, self.handle), "bjj_base_free")
            self.ctx._bases.remove(self)
        self.handle = None

    def info(self):
        """-> (window_bits, n_windows, table_bytes)"""
        w, nw, tb = ctypes.c_int(), ctypes.c_int(), ctypes.c_uint64()
        self.ctx._ck(self.ctx.lib.bjj_base_info(self.handle, ctypes.byref(w), ctypes.byref(nw), ctypes.byref(tb)), "bjj_base_info")
        return w.value, nw.value, tb.value

    def check(self):
        """number of violated link conditions of the table (0 = sound), checked on the device"""
        bad = ctypes.c_uint64(0)
        self.ctx._ck(self.ctx.lib.bjj_base_check(self.ctx.handle, self.handle, ctypes.byref(bad)), "bjj_base_check")
        return bad.value

    def mul(self, scalars):
        """scalars[i] * P for every i -> (n, 64): Context.mul_bases with this one base"""
        return self.ctx.mul_bases([self], [scalars])

    def encrypt(self, m, r, g=None, add=None):
        """exponential ElGamal to THIS point as the public key (Context.elgamal_encrypt)"""
        return self.ctx.elgamal_encrypt(self, m, r, g=g, add=add)

    def verify(self, r_b8, s, msg):
        """EdDSA-Poseidon signatures (R, s) over msg under THIS point as the public key -> (n,) uint8 (Context.eddsa_verify_signer)"""
        return self.ctx.eddsa_verify_signer(self, r_b8, s, msg)

    def verify_schnorr(self, r, s, msg):
        """Schnorr signatures under this point as the public key -> (n,) uint8, 2 = Err (Context.schnorr_verify_signer)"""
        return self.ctx.schnorr_verify_signer(self, r, s, msg)


class SignerSet:
    """The fixed-base tables of a set of public keys (bjj_signer_set, include/bjj_hip_signer_set.h); made by Context.signer_set()."""

    def __init__(self, ctx, handle):
        self.ctx, self.handle = ctx, handle

    def close(self):
        """bjj_signer_set_free: waits for the context's enqueued work, then releases the tables"""
        if getattr(self, "handle", None) and getattr(self.ctx, "handle", None):
            self.ctx._ck(self.ctx.lib.bjj_signer_set_free(self.ctx.handle, self.handle), "bjj_signer_set_free")
            self.ctx._sets.remove(self)
        self.handle = None

    def _live(self, what):
        if not self.handle:
            raise BjjError("%s: the signer set is closed" % what)

    def info(self):
        """-> (n_signers, window_bits, n_windows, table_bytes)"""
        self._live("info")
        k, w, nw, tb = ctypes.c_uint64(), ctypes.c_int(), ctypes.c_int(), ctypes.c_uint64()
        self.ctx._ck(self.ctx.lib.bjj_signer_set_info(self.handle, ctypes.byref(k), ctypes.byref(w), ctypes.byref(nw), ctypes.byref(tb)),
                     "bjj_signer_set_info")
        return k.value, w.value, nw.value, tb.value

    def check(self):
        """number of violated link conditions over the tables of all signers (0 = sound), checked on the device"""
        self._live("check")
        bad = ctypes.c_uint64(0)
        self.ctx._ck(self.ctx.lib.bjj_signer_set_check(self.ctx.handle, self.handle, ctypes.byref(bad)), "bjj_signer_set_check")
        return bad.value

    def verify(self, idx, r_b8, s, msg):
        """EdDSA-Poseidon signatures (R, s) over msg, item i under key idx[i] of the set -> (n,) uint8: what eddsa_verify gives with
        the keys gathered by index, 3 where idx[i] is not an index of the set (bjj_eddsa_verify_set)"""
        return self.ctx._verify_set(self.ctx.lib.bjj_eddsa_verify_set, "eddsa_verify_set", self, idx, r_b8, s, msg)

    def verify_schnorr(self, idx, r, s, msg):
        """Schnorr signatures, item i under key idx[i] -> (n,) uint8: 1 / 0, 2 = Err (msg > Q), 3 = no such signer"""
        return self.ctx._verify_set(self.ctx.lib.bjj_schnorr_verify_set, "schnorr_verify_set", self, idx, r, s, msg)


class DlogTable:
    """The baby-step table of one base point (bjj_dlog_table, include/bjj_hip_dlog.h); made by Context.dlog_table()."""

    def __init__(self, ctx, handle):
        self.ctx, self.handle = ctx, handle

    def close(self):
        """bjj_dlog_table_free: waits for the context's enqueued work, then releases the table"""
        if getattr(self, "handle", None) and getattr(self.ctx, "handle", None):
            self.ctx._ck(self.ctx.lib.bjj_dlog_table_free(self.ctx.handle, self.handle), "bjj_dlog_table_free")
            self.ctx._dlogs.remove(self)
        self.handle = None

    def _live(self, what):
        if not self.handle:
            raise BjjError("%s: the table is closed" % what)

    def info(self):
        """-> (baby_bits, entries, table_bytes)"""
        self._live("info")
        b, e, tb = ctypes.c_int(), ctypes.c_uint64(), ctypes.c_uint64()
        self.ctx._ck(self.ctx.lib.bjj_dlog_table_info(self.handle, ctypes.byref(b), ctypes.byref(e), ctypes.byref(tb)), "bjj_dlog_table_info")
        return b.value, e.value, tb.value

    def base(self):
        """the base point as (x, y), coordinates reduced"""
        self._live("base")
        out = np.empty(64, dtype=np.uint8)
        self.ctx._ck(self.ctx.lib.bjj_dlog_table_base(self.handle, out.ctypes.data), "bjj_dlog_table_base")
        return _ints(out, 2)[0]

    def max_range_bits(self):
        self._live("max_range_bits")
        return self.ctx.lib.bjj_dlog_max_range_bits(self.handle)

    def check(self):
        """number of violated conditions of the table's self-check (0 = sound), checked on the device"""
        self._live("check")
        bad = ctypes.c_uint64(0)
        self.ctx._ck(self.ctx.lib.bjj_dlog_table_check(self.ctx.handle, self.handle, ctypes.byref(bad)), "bjj_dlog_table_check")
        return bad.value

    def dlog(self, points, range_bits):
        """-> (m: (n,) uint64, ok: (n,) uint8), see Context.dlog"""
        return self.ctx.dlog(self, points, range_bits)


class MultiContext:
    """All (or the listed) GPUs of this process behind one handle (bjj_multi_init): contiguous ceil(n/G) blocks per
    device, replicated tables.  Host arrays -> one pipeline thread per device; *_dev -> arrays resident on the first
    device, RCCL scatter / kernels / gather (BASELINE cfg 5)."""

    def __init__(self, devices=None, window_bits=0, transport="rccl"):
        self.lib = _lib.load()
        h = ctypes.c_void_p()
        if devices is None:
            arr, n = None, 0
        else:
            devices = [int(d) for d in devices]
            arr, n = (ctypes.c_int * len(devices))(*devices), len(devices)
        rc = self.lib.bjj_multi_init(arr, n, int(window_bits), ctypes.byref(h))
        if rc != _lib.BJJ_OK:
            raise BjjError("bjj_multi_init failed (%d): %s" % (rc, self.lib.bjj_last_error().decode()))
        self.handle = h
        if transport != "rccl":
            self.set_transport(transport)

    def set_transport(self, transport):
        """"rccl" (grouped ncclScatter / ncclGather) or "peer" (hipMemcpyPeerAsync of the same blocks) for the *_dev form"""
        t = {"rccl": _lib.BJJ_TRANSPORT_RCCL, "peer": _lib.BJJ_TRANSPORT_PEER_COPY}[transport]
        self._ck(self.lib.bjj_multi_set_transport(self.handle, t), "bjj_multi_set_transport")

    def set_chunks(self, chunks, min_chunk_items=1 << 15):
        """pipeline depth of the *_dev form: pieces per peer block (1 = serial scatter -> kernels -> gather)"""
        self._ck(self.lib.bjj_multi_set_chunks(self.handle, int(chunks), int(min_chunk_items)), "bjj_multi_set_chunks")

    def close(self):
        if getattr(self, "handle", None):
            self.lib.bjj_multi_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc, what):
        if rc != _lib.BJJ_OK:
            raise BjjError("%s failed (%d): %s" % (what, rc, self.lib.bjj_last_error().decode()))

    @property
    def size(self):
        return self.lib.bjj_multi_size(self.handle)

    def device(self, rank):
        return self.lib.bjj_multi_device(self.handle, rank)

    def ctx(self, rank):
        return Context(_borrowed=self.lib.bjj_multi_ctx(self.handle, rank))

    def shard_bounds(self, n, rank):
        lo, hi = ctypes.c_size_t(), ctypes.c_size_t()
        self.lib.bjj_shard_bounds(n, self.size, rank, ctypes.byref(lo), ctypes.byref(hi))
        return lo.value, hi.value

    def last_timing(self):
        s, c, g, v = ctypes.c_double(), ctypes.c_double(), ctypes.c_double(), ctypes.c_int()
        self._ck(self.lib.bjj_multi_last_timing(self.handle, ctypes.byref(s), ctypes.byref(c), ctypes.byref(g), ctypes.byref(v)),
                 "bjj_multi_last_timing")
        tot, wall, ch = ctypes.c_double(), ctypes.c_double(), ctypes.c_int()
        self._ck(self.lib.bjj_multi_last_overlap(self.handle, ctypes.byref(tot), ctypes.byref(wall), ctypes.byref(ch)),
                 "bjj_multi_last_overlap")
        return {"scatter_ms": s.value, "compute_ms": c.value, "gather_ms": g.value, "rccl_version": v.value,
                "total_ms": tot.value, "wall_ms": wall.value, "chunks": ch.value}

    def mul_fixed_base(self, scalars):
        s = _as_u8(scalars, 32, "scalars")
        n = s.size // 32
        out = np.empty(n * 64, dtype=np.uint8)
        self._ck(self.lib.bjj_mul_fixed_base_multi(self.handle, s.ctypes.data, n, out.ctypes.data), "bjj_mul_fixed_base_multi")
        return out.reshape(n, 64)

    def mul_var_base(self, points, scalars):
        p = _as_u8(points, 64, "points")
        s = _as_u8(scalars, 32, "scalars")
        n = s.size // 32
        if p.size != n * 64:
            raise BjjError("mul_var_base: %d points vs %d scalars" % (p.size // 64, n))
        out = np.empty(n * 64, dtype=np.uint8)
        self._ck(self.lib.bjj_mul_var_base_multi(self.handle, p.ctypes.data, s.ctypes.data, n, out.ctypes.data),
                 "bjj_mul_var_base_multi")
        return out.reshape(n, 64)

    def eddsa_verify(self, pk, r_b8, s, msg):
        a, r, sv, m = _as_u8(pk, 64, "pk"), _as_u8(r_b8, 64, "r_b8"), _as_u8(s, 32, "s"), _as_u8(msg, 32, "msg")
        n = sv.size // 32
        if a.size != n * 64 or r.size != n * 64 or m.size != n * 32:
            raise BjjError("eddsa_verify: array lengths disagree")
        ok = np.empty(n, dtype=np.uint8)
        self._ck(self.lib.bjj_eddsa_verify_multi(self.handle, a.ctypes.data, r.ctypes.data, sv.ctypes.data, m.ctypes.data, n,
                                                 ok.ctypes.data), "bjj_eddsa_verify_multi")
        return ok

    # device-resident form: integer device addresses on the handle's first device; synchronous
    def mul_fixed_base_dev(self, d_scalars, n, d_out):
        self._ck(self.lib.bjj_mul_fixed_base_multi_dev(self.handle, d_scalars, n, d_out), "bjj_mul_fixed_base_multi_dev")

    def mul_var_base_dev(self, d_pts, d_scalars, n, d_out):
        self._ck(self.lib.bjj_mul_var_base_multi_dev(self.handle, d_pts, d_scalars, n, d_out), "bjj_mul_var_base_multi_dev")

    def eddsa_verify_dev(self, d_pk, d_r, d_s, d_msg, n, d_ok):
        self._ck(self.lib.bjj_eddsa_verify_multi_dev(self.handle, d_pk, d_r, d_s, d_msg, n, d_ok),
                 "bjj_eddsa_verify_multi_dev")


_DEFAULT = None


def default_context():
    global _DEFAULT
    if _DEFAULT is None:
        _DEFAULT = Context()
    return _DEFAULT


# ---- crate-shaped objects ----------------------------------------------------
class Point:
    """`pub struct Point { pub x: Fr, pub y: Fr }` (lib.rs:134-138); x, y are canonical ints."""

    __slots__ = ("x", "y")

    def __init__(self, x, y):
        self.x = int(x) % Q
        self.y = int(y) % Q

    def projective(self):  # lib.rs:141-147
        return PointProjective(self.x, self.y, 1)

    def mul_scalar(self, n, ctx=None):  # lib.rs:149-164 (sign of n dropped; n of any size)
        n = abs(int(n))
        ctx = ctx or default_context()
        if n >> 256:
            # `n: &BigInt` is unbounded (lib.rs:149): wide records of 32 k bytes; the device reduces mod 8l for an
            # on-curve point (exact) and replays all n.bits() bits of the reference's loop for an off-curve one
            nbytes = ((n.bit_length() + 255) // 256) * 32
            if nbytes > _lib.BJJ_MAX_SCALAR_BYTES:
                raise BjjError("mul_scalar: scalars wider than %d bits are outside the accelerated boundary"
                               % (8 * _lib.BJJ_MAX_SCALAR_BYTES))
            out = ctx.mul_var_base_wide([(self.x, self.y)], np.frombuffer(n.to_bytes(nbytes, "little"), np.uint8), nbytes)
        elif (self.x, self.y) == B8:
            out = ctx.mul_fixed_base([n])
        else:
            out = ctx.mul_var_base([(self.x, self.y)], [n])
        x, y = _ints(out, 2)[0]
        return Point(x, y)

    def compress(self, ctx=None):  # lib.rs:166-178 -> 32 bytes
        return bytes((ctx or default_context()).compress_points([(self.x, self.y)])[0])

    def equals(self, p):  # lib.rs:180-185
        return self.x == p.x and self.y == p.y

    def __eq__(self, o):
        return isinstance(o, Point) and self.equals(o)

    def __repr__(self):
        return "Point(x=%d, y=%d)" % (self.x, self.y)


class PointProjective:
    """`pub struct PointProjective { pub x, pub y, pub z }` (lib.rs:62-67): any z, like the reference."""

    __slots__ = ("x", "y", "z")

    def __init__(self, x, y, z=1):
        self.x, self.y, self.z = int(x) % Q, int(y) % Q, int(z) % Q

    def affine(self, ctx=None):  # lib.rs:70-85 (z == 0 -> (0, 0))
        x, y = _ints((ctx or default_context()).proj_affine([(self.x, self.y, self.z)]), 2)[0]
        return Point(x, y)

    def add(self, q, ctx=None):  # lib.rs:88-131: the raw (x, y, z) of the reference's formula sequence
        x, y, z = _ints((ctx or default_context()).proj_add([(self.x, self.y, self.z)], [(q.x, q.y, q.z)]), 3)[0]
        return PointProjective(x, y, z)


class Signature:
    """`pub struct Signature { pub r_b8: Point, pub s: BigInt }` (lib.rs:239-243)."""

    __slots__ = ("r_b8", "s")

    def __init__(self, r_b8, s):
        self.r_b8 = r_b8
        self.s = int(s)

    def compress(self, ctx=None):  # lib.rs:245-258 -> 64 bytes: compressed R, then the first 32 little-endian bytes of s
        s_le = self.s.to_bytes(max(32, (self.s.bit_length() + 7) // 8), "little")[:32]
        return self.r_b8.compress(ctx) + s_le


class PrivateKey:
    """`pub struct PrivateKey { pub key: [u8; 32] }` (lib.rs:270-342)."""

    __slots__ = ("key",)

    def __init__(self, key):
        self.key = bytes(key)

    @staticmethod
    def import_(b):  # PrivateKey::import, lib.rs:275-282
        if len(b) != 32:
            raise ValueError("imported key can not be bigger than 32 bytes")
        return PrivateKey(bytes(b))

    def scalar_key(self, ctx=None):  # lib.rs:284-302
        return _ints((ctx or default_context()).scalar_keys(np.frombuffer(self.key, np.uint8)), 1)[0]

    def public(self, ctx=None):  # lib.rs:304-306
        x, y = _ints((ctx or default_context()).public_keys(np.frombuffer(self.key, np.uint8)), 2)[0]
        return Point(x, y)

    def sign(self, msg, ctx=None):  # lib.rs:308-342 -> Signature; ValueError for the reference's Err
        msg = int(msg)
        if msg < 0:
            raise BjjError("sign: negative msg")
        if msg > Q:
            raise ValueError("msg outside the Finite Field")
        r, s, ok = (ctx or default_context()).sign(np.frombuffer(self.key, np.uint8), [msg])
        if not ok[0]:
            raise ValueError("msg outside the Finite Field")
        x, y = _ints(r, 2)[0]
        return Signature(Point(x, y), _ints(s, 1)[0])

    def sign_schnorr(self, m, k=None, ctx=None):  # lib.rs:344-361 -> (Point, BigInt); ValueError for Err
        """k: the 1024-bit nonce; None draws it from the OS generator as the reference does from
        rand::thread_rng (lib.rs:347-348).  s is the reference's unreduced integer k + scalar_key*h."""
        m = int(m)
        if m < 0:
            raise BjjError("sign_schnorr: negative msg")
        if m > Q:
            raise ValueError("msg outside the Finite Field")
        if k is None:
            import secrets
            k = secrets.randbits(1024)
        k = int(k)
        if k < 0 or k >> 1024:
            raise BjjError("sign_schnorr: nonce outside the 1024-bit record of the C ABI")
        r, s, ok = (ctx or default_context()).sign_schnorr(np.frombuffer(self.key, np.uint8), [m],
                                                           np.frombuffer(k.to_bytes(128, "little"), np.uint8))
        if not ok[0]:
            raise ValueError("msg outside the Finite Field")
        x, y = _ints(r, 2)[0]
        return Point(x, y), int.from_bytes(s[0].tobytes(), "little")


def decompress_point(bb, ctx=None):
    """decompress_point(bb: [u8; 32]) -> Result<Point, String>  (lib.rs:192-224); raises ValueError for Err"""
    if len(bb) != 32:
        raise BjjError("decompress_point: need exactly 32 bytes")
    pts, ok = (ctx or default_context()).decompress_points(np.frombuffer(bytes(bb), np.uint8))
    if not ok[0]:
        raise ValueError("decompress_point: y outside the field or x^2 not a (non-zero) square")
    x, y = _ints(pts, 2)[0]
    return Point(x, y)


def decompress_signature(b, ctx=None):
    """decompress_signature(b: &[u8; 64]) -> Result<Signature, String>  (lib.rs:260-268)"""
    if len(b) != 64:
        raise BjjError("decompress_signature: need exactly 64 bytes")
    return Signature(decompress_point(bytes(b[:32]), ctx), int.from_bytes(bytes(b[32:]), "little"))


def new_key():
    """new_key() -> PrivateKey (lib.rs:387-393): 1024 random bits, the first 32 big-endian bytes kept."""
    import secrets
    raw = secrets.randbits(1024).to_bytes(128, "big").lstrip(b"\x00")
    while len(raw) < 32:  # probability 2^-768; the reference would panic on the slice here
        raw = secrets.randbits(1024).to_bytes(128, "big").lstrip(b"\x00")
    return PrivateKey.import_(raw[:32])


def verify(pk, sig, msg, ctx=None):
    """verify(pk: Point, sig: Signature, msg: BigInt) -> bool  (lib.rs:395-412)."""
    msg = int(msg)
    if msg < 0:
        raise BjjError("verify: negative msg (the reference panics at lib.rs:399)")
    if msg > Q:  # lib.rs:396-398; also keeps msg inside the 32-byte record
        return False
    if sig.s < 0 or sig.s >> 256:
        raise BjjError("verify: s outside the 32-byte record of the C ABI")
    ctx = ctx or default_context()
    ok = ctx.eddsa_verify([(pk.x, pk.y)], [(sig.r_b8.x, sig.r_b8.y)], [sig.s], [msg])
    return bool(ok[0])


def verify_schnorr(pk, m, r, s, ctx=None):
    """verify_schnorr(pk: Point, m: BigInt, r: Point, s: BigInt) -> Result<bool, String>  (lib.rs:375-385).
    ValueError for the reference's Err.  s may be any non-negative integer: it is reduced mod 8l on the
    host, which is exact because it only multiplies B8 (lib.rs:377)."""
    m, s = int(m), int(s)
    if m < 0 or s < 0:
        raise BjjError("verify_schnorr: negative integer")
    if m > Q:
        raise ValueError("msg outside the Finite Field")
    ok = (ctx or default_context()).schnorr_verify([(pk.x, pk.y)], [(r.x, r.y)], [s % (8 * SUBORDER)], [m])
    if ok[0] == 2:
        raise ValueError("msg outside the Finite Field")
    return bool(ok[0])


# ---- batch forms ---------------------------------------------------------------
def mul_fixed_base_batch(scalars, ctx=None):
    return (ctx or default_context()).mul_fixed_base(scalars)


def mul_scalar_batch(points, scalars, ctx=None):
    return (ctx or default_context()).mul_var_base(points, scalars)


def poseidon5_batch(inputs, ctx=None):
    return (ctx or default_context()).poseidon5(inputs)


def verify_batch(pk, r_b8, s, msg, ctx=None):
    return (ctx or default_context()).eddsa_verify(pk, r_b8, s, msg)


def point_add_batch(p, q, ctx=None):
    return (ctx or default_context()).point_add(p, q)


def msm(points, scalars, ctx=None):
    """sum of points[i].mul_scalar(scalars[i]) as a Point (bjj_msm); points: Points or (x, y) pairs, scalars: ints < 2^256.
    BjjError for an off-curve point (the reference fold over non-group elements has no meaning here)."""
    pts = [(p.x, p.y) if isinstance(p, Point) else tuple(p) for p in points]
    sc = [int(k) for k in scalars]
    if len(pts) != len(sc):
        raise BjjError("msm: %d points but %d scalars" % (len(pts), len(sc)))
    if any(k < 0 or k >> 256 for k in sc):
        raise BjjError("msm: scalars are 256-bit unsigned integers")
    x, y = _ints((ctx or default_context()).msm(pts, sc), 2)[0]
    return Point(x, y)


def msm_batch(segments, ctx=None):
    """[sum of points[i].mul_scalar(scalars[i]) for (points, scalars) in segments] as Points, in one call (bjj_msm_batch).
    BjjError names the segment and the index inside it of an off-curve point."""
    pts, sc, offsets = [], [], [0]
    for t, (points, scalars) in enumerate(segments):
        p = [(q.x, q.y) if isinstance(q, Point) else tuple(q) for q in points]
        k = [int(v) for v in scalars]
        if len(p) != len(k):
            raise BjjError("msm_batch: segment %d has %d points but %d scalars" % (t, len(p), len(k)))
        if any(v < 0 or v >> 256 for v in k):
            raise BjjError("msm_batch: scalars are 256-bit unsigned integers (segment %d)" % t)
        pts += p
        sc += k
        offsets.append(len(pts))
    if len(offsets) == 1:
        return []
    out, status = (ctx or default_context()).msm_batch(pts, sc, offsets)
    for t, st in enumerate(status):
        if st != -1:
            raise BjjError("msm_batch: segment %d: point %d is not on the curve" % (t, int(st) - offsets[t]))
    return [Point(x, y) for x, y in _ints(out, 2)]


def point_sum(segments, ctx=None):
    """[the sum of a segment's points for every segment] as Points, in one call (bjj_point_sum).  A segment is a list of Points or
    (x, y) pairs; an item (point, True) is subtracted.  BjjError names the segment and the index inside it of an off-curve point."""
    pts, neg, offsets = [], [], [0]
    for points in segments:
        for q in points:
            minus = False
            if isinstance(q, tuple) and len(q) == 2 and isinstance(q[1], bool):
                q, minus = q
            pts.append((q.x, q.y) if isinstance(q, Point) else tuple(q))
            neg.append(1 if minus else 0)
        offsets.append(len(pts))
    if len(offsets) == 1:
        return []
    out, status = (ctx or default_context()).point_sum(pts, offsets, neg if any(neg) else None)
    for t, st in enumerate(status):
        if st != -1:
            raise BjjError("point_sum: segment %d: point %d is not on the curve" % (t, int(st) - offsets[t]))
    return [Point(x, y) for x, y in _ints(out, 2)]
