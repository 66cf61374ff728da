"""ctypes binding of include/rabe_hip.h (plumbing only).

`Engine()` fails loudly -- EngineError -- when librabe_hip.so is missing or there is no HIP device;
there is no CPU fallback.
"""
import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))

FR, G1, G2, GT = 32, 64, 128, 384
R_ORDER = 21888242871839275222246405745257275088548364400416034343698204186575808495617


class EngineError(RuntimeError):
    pass


def lib_path():
    # RABE_HIP_LIB selects an alternative build of the same library (kernel-tuning A/B runs)
    return os.environ.get("RABE_HIP_LIB") or os.path.join(HERE, "librabe_hip.so")


_LIB = None


def _share_hip_runtime_with_torch():
    """One process must hold ONE HIP runtime.  PyTorch-ROCm wheels bundle their own libamdhip64.so
    (same SONAME as /opt/rocm's); whichever is loaded first wins, and if ours came first torch would
    later find "No HIP GPUs".  So when torch is installed, map its runtime before librabe_hip.so is
    resolved -- import order then no longer matters (bench.py and smoke() need torch for streams and
    torch.distributed in the same process)."""
    import importlib.util
    spec = importlib.util.find_spec("torch")
    if spec is None or not spec.origin:
        return
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            ctypes.CDLL(cand, mode=ctypes.RTLD_GLOBAL)
        except OSError:
            pass


def load_library():
    """dlopen the engine (works without a GPU; only rhip_ctx_create needs one)."""
    global _LIB
    if _LIB is None:
        path = lib_path()
        if not os.path.exists(path):
            raise EngineError("HIP engine not built: %s missing (run `python -m rabe_amd.build`)" % path)
        _share_hip_runtime_with_torch()
        lib = ctypes.CDLL(path)
        lib.rhip_last_error.restype = ctypes.c_char_p
        _LIB = lib
    return _LIB


def fr_bytes(x):
    return int(x % R_ORDER).to_bytes(32, "little")


class DevBuf:
    """A device allocation owned by an Engine."""

    def __init__(self, eng, nbytes):
        self.eng = eng
        self.nbytes = nbytes
        p = ctypes.c_void_p()
        eng._check(eng.lib.rhip_malloc(eng.ctx, ctypes.c_size_t(nbytes), ctypes.byref(p)))
        self.ptr = p

    def free(self):
        if self.ptr:
            self.eng.lib.rhip_free(self.eng.ctx, self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Engine:
    def __init__(self, device=0):
        self.lib = load_library()
        ctx = ctypes.c_void_p()
        rc = self.lib.rhip_ctx_create(ctypes.c_int32(device), ctypes.byref(ctx))
        if rc != 0:
            why = self.lib.rhip_last_error(None)
            raise EngineError("rhip_ctx_create(device=%d) failed with %d [%s]: no usable HIP device "
                              "(the engine has no CPU fallback)" % (device, rc, why.decode() if why else "?"))
        self.ctx = ctx

    def close(self):
        if self.ctx:
            self.lib.rhip_ctx_destroy(self.ctx)
            self.ctx = None

    def _check(self, rc):
        if rc != 0:
            raise EngineError("rabe_hip call failed (%d): %s" % (rc, self.lib.rhip_last_error(self.ctx).decode()))

    # ------------------------------------------------------------------ memory
    def alloc(self, nbytes):
        return DevBuf(self, max(int(nbytes), 4))

    def upload(self, data):
        data = bytes(data)
        b = self.alloc(len(data))
        if data:
            self._check(self.lib.rhip_upload(self.ctx, b.ptr, data, ctypes.c_size_t(len(data))))
        return b

    def upload_u32(self, values):
        import array
        return self.upload(array.array("I", values).tobytes())

    def download(self, buf, nbytes=None):
        n = buf.nbytes if nbytes is None else nbytes
        out = ctypes.create_string_buffer(n)
        if n:
            self._check(self.lib.rhip_download(self.ctx, out, buf.ptr, ctypes.c_size_t(n)))
        return out.raw

    def sync(self):
        self._check(self.lib.rhip_sync(self.ctx))

    def set_stream(self, hip_stream_ptr):
        self._check(self.lib.rhip_ctx_set_stream(self.ctx, ctypes.c_void_p(hip_stream_ptr)))

    def set_pairing_mode(self, mode):
        """0 auto, 1 one lane per pairing, 3 three cooperating lanes per pairing, 6 six lanes per accumulator, 29 reduced radix (same
        results); 99 cross-check: auto, then every family forced on the same inputs, compared on the device (a difference fails the call)."""
        self._check(self.lib.rhip_ctx_set_pairing_mode(self.ctx, ctypes.c_int32(mode)))

    def timing(self, enable):
        self._check(self.lib.rhip_ctx_timing(self.ctx, ctypes.c_int32(1 if enable else 0)))

    def timing_read(self):
        """{kernel_name: (total_ms, launches)} since the last read."""
        buf = ctypes.create_string_buffer(1 << 16)
        self._check(self.lib.rhip_ctx_timing_read(self.ctx, buf, ctypes.c_size_t(len(buf))))
        out = {}
        for line in buf.value.decode().splitlines():
            name, ms, cnt = line.split()
            out[name] = (float(ms), int(cnt))
        return out

    def device_info(self):
        n = ctypes.c_int32()
        name = ctypes.create_string_buffer(128)
        self._check(self.lib.rhip_device_info(self.ctx, ctypes.byref(n), name, ctypes.c_size_t(128)))
        return n.value, name.value.decode()

    # ------------------------------------------------------------------ Level E helpers (host bytes in, host bytes out)
    def _elem(self, fn, n, ins, out_elem_bytes, extra_first=()):
        bufs = [self.upload(b"".join(x)) if not isinstance(x, (bytes, bytearray)) else self.upload(x) for x in ins]
        out = self.alloc(n * out_elem_bytes)
        args = list(extra_first) + [ctypes.c_size_t(n)] + [b.ptr for b in bufs] + [out.ptr]
        self._check(getattr(self.lib, fn)(self.ctx, *args))
        raw = self.download(out, n * out_elem_bytes)
        return [raw[i * out_elem_bytes:(i + 1) * out_elem_bytes] for i in range(n)]

    def fr_op(self, op, a, b=None):
        n = len(a)
        bb = b if b is not None else a
        return self._elem("rhip_fr_op", n, [a, bb], FR, extra_first=(ctypes.c_int32(op),))

    def fr_from_be32_reduce(self, digests):
        return self._elem("rhip_fr_from_be32_reduce", len(digests), [digests], FR)

    def fp_dot2(self, a0, b0, a1, b1):
        """diagnostic: a0 b0 + a1 b1 over the base field through the device's two-term dot product (canonical 32-byte records < p)"""
        return self._elem("rhip_fp_dot2", len(a0), [a0, b0, a1, b1], FR)

    def g1_add(self, a, b): return self._elem("rhip_g1_add", len(a), [a, b], G1)
    def g1_neg(self, a): return self._elem("rhip_g1_neg", len(a), [a], G1)
    def g1_mul(self, p, k): return self._elem("rhip_g1_mul", len(p), [p, k], G1)
    def g2_add(self, a, b): return self._elem("rhip_g2_add", len(a), [a, b], G2)
    def g2_neg(self, a): return self._elem("rhip_g2_neg", len(a), [a], G2)
    def g2_mul(self, p, k): return self._elem("rhip_g2_mul", len(p), [p, k], G2)

    def g2_mul_rows(self, points, item_row_off, scalars):
        """out[t] = scalars[i] * points[t] for the rows t of item i (rhip_g2_mul_rows: one four-way split per scalar, one joint chain per
        row); item_row_off: len(scalars) + 1 non-decreasing offsets ending at len(points).  The points must be members of G2."""
        n_rows, n_items = len(points), len(scalars)
        if len(item_row_off) != n_items + 1 or item_row_off[0] != 0 or item_row_off[-1] != n_rows:
            raise ValueError("g2_mul_rows: item_row_off must run from 0 to len(points) in len(scalars) + 1 entries")
        if any(item_row_off[i] > item_row_off[i + 1] for i in range(n_items)):
            raise ValueError("g2_mul_rows: item_row_off must not decrease")
        if not n_rows:
            return []
        dp, dk, doff = self.upload(b"".join(points)), self.upload(b"".join(scalars)), self.upload_u32(item_row_off)
        out = self.alloc(n_rows * G2)
        self._check(self.lib.rhip_g2_mul_rows(self.ctx, ctypes.c_size_t(n_rows), doff.ptr, dp.ptr, ctypes.c_size_t(n_items), dk.ptr, out.ptr))
        raw = self.download(out, n_rows * G2)
        return [raw[i * G2:(i + 1) * G2] for i in range(n_rows)]

    def g1_mul_rows(self, points, item_row_off, scalars):
        """out[t] = scalars[i] * points[t] for the rows t of item i (rhip_g1_mul_rows: one GLV decomposition per scalar, one joint chain per
        row, one inversion per block); item_row_off: len(scalars) + 1 non-decreasing offsets ending at len(points).  Same bytes as g1_mul."""
        n_rows, n_items = len(points), len(scalars)
        if len(item_row_off) != n_items + 1 or item_row_off[0] != 0 or item_row_off[-1] != n_rows:
            raise ValueError("g1_mul_rows: item_row_off must run from 0 to len(points) in len(scalars) + 1 entries")
        if any(item_row_off[i] > item_row_off[i + 1] for i in range(n_items)):
            raise ValueError("g1_mul_rows: item_row_off must not decrease")
        if not n_rows:
            return []
        dp, dk, doff = self.upload(b"".join(points)), self.upload(b"".join(scalars)), self.upload_u32(item_row_off)
        out = self.alloc(n_rows * G1)
        self._check(self.lib.rhip_g1_mul_rows(self.ctx, ctypes.c_size_t(n_rows), doff.ptr, dp.ptr, ctypes.c_size_t(n_items), dk.ptr, out.ptr))
        raw = self.download(out, n_rows * G1)
        return [raw[i * G1:(i + 1) * G1] for i in range(n_rows)]

    def _mul_rows_at(self, g, elem, points, row_src, item_row_off, scalars, row_dst, out_rows, fill):
        what = "%s_mul_rows_at" % g
        n_rows, n_items = len(row_src), len(scalars)
        out_rows = n_rows if out_rows is None else out_rows
        if len(row_dst) != n_rows:
            raise ValueError("%s: row_src and row_dst must hold one entry per row" % what)
        if len(item_row_off) != n_items + 1 or item_row_off[0] != 0 or item_row_off[-1] != n_rows:
            raise ValueError("%s: item_row_off must run from 0 to len(row_src) in len(scalars) + 1 entries" % what)
        if any(item_row_off[i] > item_row_off[i + 1] for i in range(n_items)):
            raise ValueError("%s: item_row_off must not decrease" % what)
        if any(not 0 <= s < len(points) for s in row_src):
            raise ValueError("%s: row_src must index into points" % what)
        if any(not 0 <= d < out_rows for d in row_dst):
            raise ValueError("%s: row_dst must index into the out_rows output elements" % what)
        dp, dk, doff = self.upload(b"".join(points)), self.upload(b"".join(scalars)), self.upload_u32(item_row_off)
        dsrc, ddst = self.upload_u32(row_src), self.upload_u32(row_dst)
        out = self.alloc(out_rows * elem) if fill is None else self.upload(bytes([fill]) * (out_rows * elem))
        self._check(getattr(self.lib, "rhip_" + what)(self.ctx, ctypes.c_size_t(n_rows), doff.ptr, dp.ptr, dsrc.ptr, ctypes.c_size_t(n_items), dk.ptr,
                                                      ddst.ptr, out.ptr))
        raw = self.download(out, out_rows * elem)
        return [raw[i * elem:(i + 1) * elem] for i in range(out_rows)]

    def g2_mul_rows_at(self, points, row_src, item_row_off, scalars, row_dst, out_rows=None, fill=None):
        """out[row_dst[t]] = scalars[i] * points[row_src[t]] for the rows t of item i (rhip_g2_mul_rows_at); the rows are len(row_src), the
        points may be fewer.  Returns the out_rows (default: the rows) output elements; with `fill` the output buffer starts as that repeated
        byte, so a slot no row was written to shows it."""
        return self._mul_rows_at("g2", G2, points, row_src, item_row_off, scalars, row_dst, out_rows, fill)

    def g1_mul_rows_at(self, points, row_src, item_row_off, scalars, row_dst, out_rows=None, fill=None):
        """out[row_dst[t]] = scalars[i] * points[row_src[t]] for the rows t of item i (rhip_g1_mul_rows_at), as g2_mul_rows_at"""
        return self._mul_rows_at("g1", G1, points, row_src, item_row_off, scalars, row_dst, out_rows, fill)

    def _upload_ptrs(self, bufs):
        import array
        return self.upload(array.array("Q", [b.ptr.value or 0 for b in bufs]).tobytes())

    def assemble_records(self, out_size, out_off, layout, layout_off, map_words, sources, src_item_off, fill=None):
        """rhip_assemble_records on host bytes: byte b of record i (at out_off[i] of an output of out_size bytes) = map word
        map_words[layout_off[layout[i]] + b], 0xFF0000vv the literal vv, k << 24 | o byte o of sources[k] from src_item_off[k * n + i] on.
        The array of source pointers is made here.  Returns the output bytes (started as the repeated byte `fill`, if given)."""
        import array
        n, n_src = len(out_off), len(sources)
        if len(layout) != n or len(src_item_off) != n_src * n:
            raise ValueError("assemble_records: one layout index per record and one source offset per (source, record)")
        if any(not 0 <= l < len(layout_off) - 1 for l in layout) or any(not 0 <= o <= len(map_words) for o in layout_off):
            raise ValueError("assemble_records: layout / layout_off out of range")
        for i in range(n):
            m0, m1 = layout_off[layout[i]], layout_off[layout[i] + 1]
            if m1 < m0 or out_off[i] < 0 or out_off[i] + (m1 - m0) > out_size:
                raise ValueError("assemble_records: record %d does not lie inside the output" % i)
            for v in map_words[m0:m1]:
                k = v >> 24
                if k != 0xFF and (k >= n_src or not 0 <= src_item_off[k * n + i] + (v & 0xFFFFFF) < len(sources[k])):
                    raise ValueError("assemble_records: record %d reads outside source %d" % (i, k))
        up = {}
        for s in sources:          # one object named twice is uploaded once
            if id(s) not in up:
                up[id(s)] = self.upload(s)
        dsrc = [up[id(s)] for s in sources]
        out =self.alloc(out_size) if fill is None else self.upload(bytes([fill]) * out_size)
        doo, dsio, dptr = self.upload(array.array("Q", out_off).tobytes()), self.upload(array.array("Q", src_item_off).tobytes()), self._upload_ptrs(dsrc)
        dl, dlo, dmap = self.upload_u32(layout), self.upload_u32(layout_off), self.upload_u32(map_words)
        self._check(self.lib.rhip_assemble_records(self.ctx, ctypes.c_size_t(n), out.ptr, doo.ptr, dl.ptr, dlo.ptr, dmap.ptr, ctypes.c_uint32(n_src),
                                                   dptr.ptr, dsio.ptr))
        return self.download(out, out_size)

    def gather_parts(self, blob, rec_off, layout, layout_off, part_src, part_dst, part_len, part_k, dst_sizes, dst_item_off, fill=None):
        """rhip_gather_parts on host bytes: part p of layout[i] (the parts layout_off[l] .. layout_off[l + 1]) copies part_len[p] bytes from
        blob[rec_off[i] + part_src[p]] to destination part_k[p] at dst_item_off[k * n + i] + part_dst[p].  The destinations (dst_sizes bytes
        each, started as the repeated byte `fill`, if given) and the array of their pointers are made here.  Returns the destinations."""
        import array
        n, n_dst, n_parts = len(rec_off), len(dst_sizes), len(part_k)
        if len(layout) != n or len(dst_item_off) != n_dst * n or not len(part_src) == len(part_dst) == len(part_len) == n_parts:
            raise ValueError("gather_parts: one layout index per record, one offset per (destination, record), four entries per part")
        if any(not 0 <= l < len(layout_off) - 1 for l in layout) or any(not 0 <= o <= n_parts for o in layout_off) or \
                any(not 0 <= k < n_dst for k in part_k):
            raise ValueError("gather_parts: layout / layout_off / part_k out of range")
        for i in range(n):
            for p in range(layout_off[layout[i]], layout_off[layout[i] + 1]):
                s, d = rec_off[i] + part_src[p], dst_item_off[part_k[p] * n + i] + part_dst[p]
                if part_len[p] < 0 or min(s, d) < 0 or s + part_len[p] > len(blob) or d + part_len[p] > dst_sizes[part_k[p]]:
                    raise ValueError("gather_parts: part %d of record %d leaves the blob or its destination" % (p, i))
        ddst = [self.alloc(s) if fill is None else self.upload(bytes([fill]) * s) for s in dst_sizes]
        dblob, dro, ddio = self.upload(blob), self.upload(array.array("Q", rec_off).tobytes()), self.upload(array.array("Q", dst_item_off).tobytes())
        dl, dlo, dptr = self.upload_u32(layout), self.upload_u32(layout_off), self._upload_ptrs(ddst)
        dps, dpd, dpl, dpk = self.upload_u32(part_src), self.upload_u32(part_dst), self.upload_u32(part_len), self.upload_u32(part_k)
        self._check(self.lib.rhip_gather_parts(self.ctx, ctypes.c_size_t(n), dblob.ptr, dro.ptr, dl.ptr, dlo.ptr, dps.ptr, dpd.ptr, dpl.ptr, dpk.ptr,
                                               dptr.ptr, ddio.ptr))
        return [self.download(d, s) for d, s in zip(ddst, dst_sizes)]

    def _ghw11_rows_in(self, what, item_row_off, item_hash_off, hashes, per_item):
        n_items = len(item_hash_off)
        if len(item_row_off) != n_items + 1 or item_row_off[0] != 0 or any(len(x) != n_items for x in per_item):
            raise ValueError("%s: item_row_off must hold len(item_hash_off) + 1 offsets from 0, and one scalar per item" % what)
        for i in range(n_items):
            cnt = item_row_off[i + 1] - item_row_off[i] - 2
            if cnt < 1 or item_hash_off[i] + cnt > len(hashes):
                raise ValueError("%s: item %d needs L, K and at least one attribute row, with its hashes inside `hashes`" % (what, i))
        return n_items, (item_row_off[-1] if n_items else 0)

    def ghw11_keygen_dev(self, keys, item_row_off, item_hash_off, hashes, r):
        """rhip_ghw11_keygen_batch on host bytes: the rows L, K, K_x... of every item under `keys` (Ghw11Keys), 128 bytes each"""
        n_items, n_rows = self._ghw11_rows_in("ghw11_keygen_dev", item_row_off, item_hash_off, hashes, [r])
        if not n_rows:
            return []
        doff, dho, dh, dr = self.upload_u32(item_row_off), self.upload_u32(item_hash_off), self.upload(b"".join(hashes)), self.upload(b"".join(r))
        out = self.alloc(n_rows * G2)
        self._check(self.lib.rhip_ghw11_keygen_batch(self.ctx, keys.h, ctypes.c_size_t(n_items), ctypes.c_size_t(n_rows), doff.ptr, dho.ptr, dh.ptr,
                                                     dr.ptr, out.ptr))
        raw = self.download(out, n_rows * G2)
        return [raw[i * G2:(i + 1) * G2] for i in range(n_rows)]

    def ghw11_provision_dev(self, keys, item_row_off, item_hash_off, hashes, r, z, want_sk=True):
        """rhip_ghw11_provision_batch on host bytes: (sk_rows or None, tk_rows, flags) -- the secret-key rows of ghw11_keygen_dev, the
        transform-key rows L_z = g2 * (r / z), K_z = g2_alpha / z + g2_a * (r / z), K_x_z = g2 * (h(x) r / z) in the same layout, and
        flags[i] = 1 where z[i] = 0.  The first call with `keys` builds its window table of g2_alpha."""
        n_items, n_rows = self._ghw11_rows_in("ghw11_provision_dev", item_row_off, item_hash_off, hashes, [r, z])
        if not n_rows:
            return ([] if want_sk else None), [], []
        doff, dho, dh = self.upload_u32(item_row_off), self.upload_u32(item_hash_off), self.upload(b"".join(hashes))
        dr, dz = self.upload(b"".join(r)), self.upload(b"".join(z))
        sk = self.alloc(n_rows * G2) if want_sk else None
        tk, fl = self.alloc(n_rows * G2), self.alloc(4 * n_items)
        self._check(self.lib.rhip_ghw11_provision_batch(self.ctx, keys.h, ctypes.c_size_t(n_items), ctypes.c_size_t(n_rows), doff.ptr, dho.ptr, dh.ptr,
                                                        dr.ptr, dz.ptr, sk.ptr if want_sk else None, tk.ptr, fl.ptr))
        rows = lambda raw: [raw[i * G2:(i + 1) * G2] for i in range(n_rows)]
        flags = self.download(fl, 4 * n_items)
        return (rows(self.download(sk, n_rows * G2)) if want_sk else None), rows(self.download(tk, n_rows * G2)), \
            [int.from_bytes(flags[4 * i:4 * i + 4], "little") for i in range(n_items)]

    def dnf_keygen_dev(self, keys, r):
        """rhip_dnf_keygen_batch on host bytes: (g1_rows, g2_rows) under `keys` (DnfKeys) -- item i owns rows 2 i, 2 i + 1 of both:
        sk.u1 = a1 + p1 * r_i, pk.u1 = g1 * r_i (64 bytes each) and sk.u2 = a2 + p2 * r_i, pk.u2 = g2 * r_i (128 bytes each)"""
        n_items = len(r)
        if not n_items:
            return [], []
        dr = self.upload(b"".join(r))
        o1, o2 = self.alloc(2 * n_items * G1), self.alloc(2 * n_items * G2)
        self._check(self.lib.rhip_dnf_keygen_batch(self.ctx, keys.h, ctypes.c_size_t(n_items), dr.ptr, o1.ptr, o2.ptr))
        raw1, raw2 = self.download(o1, 2 * n_items * G1), self.download(o2, 2 * n_items * G2)
        return [raw1[i * G1:(i + 1) * G1] for i in range(2 * n_items)], [raw2[i * G2:(i + 1) * G2] for i in range(2 * n_items)]

    def gt_mul(self, a, b): return self._elem("rhip_gt_mul", len(a), [a, b], GT)
    def gt_inv(self, a): return self._elem("rhip_gt_inv", len(a), [a], GT)
    def gt_pow(self, a, k): return self._elem("rhip_gt_pow", len(a), [a, k], GT)
    def pairing(self, p, q): return self._elem("rhip_pairing", len(p), [p, q], GT)

    def gt_pow_rows(self, a, item_row_off, scalars, mul=None, invert=False):
        """out[t] = (mul[t] if mul else 1) * a[t]^(+-scalars[i]) for the rows t of item i, minus with invert (rhip_gt_pow_rows: one four-way
        split over the Frobenius map per scalar, one joint chain of at most 66 squarings per row); item_row_off: len(scalars) + 1
        non-decreasing offsets ending at len(a).  The elements of `a` must be members of Gt.  Same bytes as gt_pow + gt_inv / gt_mul."""
        n_rows, n_items = len(a), len(scalars)
        if len(item_row_off) != n_items + 1 or item_row_off[0] != 0 or item_row_off[-1] != n_rows:
            raise ValueError("gt_pow_rows: item_row_off must run from 0 to len(a) in len(scalars) + 1 entries")
        if any(item_row_off[i] > item_row_off[i + 1] for i in range(n_items)):
            raise ValueError("gt_pow_rows: item_row_off must not decrease")
        if mul is not None and len(mul) != n_rows:
            raise ValueError("gt_pow_rows: one mul element per row")
        if not n_rows:
            self._check(self.lib.rhip_gt_pow_rows(self.ctx, ctypes.c_size_t(0), None, None, ctypes.c_size_t(n_items), None, None,
                                                  ctypes.c_uint32(1 if invert else 0), None))
            return []
        da, dk, doff = self.upload(b"".join(a)), self.upload(b"".join(scalars)), self.upload_u32(item_row_off)
        dm = self.upload(b"".join(mul)) if mul is not None else None
        out = self.alloc(n_rows * GT)
        self._check(self.lib.rhip_gt_pow_rows(self.ctx, ctypes.c_size_t(n_rows), doff.ptr, da.ptr, ctypes.c_size_t(n_items), dk.ptr,
                                              dm.ptr if dm is not None else None, ctypes.c_uint32(1 if invert else 0), out.ptr))
        raw = self.download(out, n_rows * GT)
        return [raw[i * GT:(i + 1) * GT] for i in range(n_rows)]

    def gt_multiexp_rows(self, a, item_row_off, scalars, mul=None, invert=False, chunk_terms=0):
        """out[i] = (mul[i] if mul else 1) * prod of a[t]^(+-scalars[t]) over the rows t of item i, minus with invert (rhip_gt_multiexp_rows:
        width-4 signed digits per scalar, the table a, a^3, a^5, a^7 per row, lane (chunk, item) on one chain of cyclotomic squarings);
        item_row_off: n_items + 1 non-decreasing offsets from 0 to len(a); chunk_terms 0 lets the engine choose the chunking, another value
        forces the rows per lane.  The elements of `a` must be members of Gt.  Same bytes as gt_pow + gt_inv + gt_product + gt_mul."""
        n_rows, n_items = len(a), len(item_row_off) - 1
        if len(scalars) != n_rows:
            raise ValueError("gt_multiexp_rows: one scalar per row")
        if n_items < 0 or item_row_off[0] != 0 or item_row_off[-1] != n_rows:
            raise ValueError("gt_multiexp_rows: item_row_off must run from 0 to len(a)")
        if any(item_row_off[i] > item_row_off[i + 1] for i in range(n_items)):
            raise ValueError("gt_multiexp_rows: item_row_off must not decrease")
        if mul is not None and len(mul) != n_items:
            raise ValueError("gt_multiexp_rows: one mul element per item")
        if not n_items:
            return []
        doff = self.upload_u32(item_row_off)
        da = self.upload(b"".join(a)) if n_rows else None
        dk = self.upload(b"".join(scalars)) if n_rows else None
        dm = self.upload(b"".join(mul)) if mul is not None else None
        out = self.alloc(n_items * GT)
        self._check(self.lib.rhip_gt_multiexp_rows(self.ctx, ctypes.c_size_t(n_rows), doff.ptr, da.ptr if da is not None else None,
                                                   dk.ptr if dk is not None else None, ctypes.c_size_t(n_items), dm.ptr if dm is not None else None,
                                                   ctypes.c_uint32(1 if invert else 0), ctypes.c_uint32(chunk_terms), out.ptr))
        raw = self.download(out, n_items * GT)
        return [raw[i * GT:(i + 1) * GT] for i in range(n_items)]

    def g1_on_curve(self, p):
        return [int.from_bytes(x, "little") for x in self._elem("rhip_g1_on_curve", len(p), [p], 4)]

    def g2_on_curve(self, p):
        return [int.from_bytes(x, "little") for x in self._elem("rhip_g2_on_curve", len(p), [p], 4)]

    def pairing_product(self, offsets, p, q):
        n_items = len(offsets) - 1
        off = self.upload_u32(offsets)
        bp, bq = self.upload(b"".join(p)), self.upload(b"".join(q))
        out = self.alloc(n_items * GT)
        self._check(self.lib.rhip_pairing_product(self.ctx, ctypes.c_size_t(n_items), off.ptr, ctypes.c_size_t(len(p)),
                                                  bp.ptr, bq.ptr, out.ptr))
        raw = self.download(out, n_items * GT)
        return [raw[i * GT:(i + 1) * GT] for i in range(n_items)]

    def pairing_jobs(self, offsets, p, q, scal=None, lead=None, sum_offsets=None, s_base=None, s_scal=None, s_q=None):
        """rhip_pairing_jobs: out[i] = lead[i] * FE(prod_j ML(scal[j] * p[j], q[j]) * ML(sum_t s_scal[t] * s_base[t], s_q[i])), j over item
        i's pairs [offsets[i], offsets[i+1]) and t over its terms [sum_offsets[i], sum_offsets[i+1]).  Without sum_offsets there is no
        summed pair; with them s_base / s_scal hold one record per term and s_q one G2 point per item (max_terms and n_terms are derived).
        A pair with an argument at infinity -- the sum included -- contributes one."""
        n_items = len(offsets) - 1
        off = self.upload_u32(offsets)
        bp, bq = self.upload(b"".join(p) or b"\0"), self.upload(b"".join(q) or b"\0")
        bs = self.upload(b"".join(scal)) if scal else None
        bl = self.upload(b"".join(lead)) if lead else None
        out = self.alloc(n_items * GT)
        mx = max(offsets[i + 1] - offsets[i] for i in range(n_items))
        max_terms = n_terms = 0
        soff = sb = sk = sq = None
        if sum_offsets is not None:
            n_terms = sum_offsets[-1]
            if len(sum_offsets) != n_items + 1 or sum_offsets[0] != 0 or any(sum_offsets[i] > sum_offsets[i + 1] for i in range(n_items)):
                raise ValueError("pairing_jobs: sum_offsets must run from 0 in len(offsets) non-decreasing entries")
            if len(s_base) != n_terms or len(s_scal) != n_terms or len(s_q) != n_items:
                raise ValueError("pairing_jobs: one s_base and one s_scal per term, one s_q per item")
            max_terms = max(sum_offsets[i + 1] - sum_offsets[i] for i in range(n_items))
            soff, sq = self.upload_u32(sum_offsets), self.upload(b"".join(s_q))
            sb, sk = self.upload(b"".join(s_base) or b"\0"), self.upload(b"".join(s_scal) or b"\0")
        self._check(self.lib.rhip_pairing_jobs(self.ctx, ctypes.c_size_t(n_items), ctypes.c_size_t(mx), ctypes.c_size_t(len(p)), off.ptr, bp.ptr,
                                               bs.ptr if bs else None, bq.ptr, ctypes.c_size_t(max_terms), ctypes.c_size_t(n_terms),
                                               soff.ptr if soff else None, sb.ptr if sb else None, sk.ptr if sk else None,
                                               sq.ptr if sq else None, bl.ptr if bl else None, out.ptr))
        raw = self.download(out, n_items * GT)
        return [raw[i * GT:(i + 1) * GT] for i in range(n_items)]

    # ------------------------------------------------------------------ pinned host buffers / stream-ordered copies
    def host_alloc(self, nbytes):
        p = ctypes.c_void_p()
        self._check(self.lib.rhip_host_alloc(self.ctx, ctypes.c_size_t(nbytes), ctypes.byref(p)))
        return p

    def host_free(self, p):
        self._check(self.lib.rhip_host_free(self.ctx, p))

    def release_before_final_exp(self, waiter):
        """one-shot: `waiter`'s stream is held until this context's next decrypt has issued its Miller loops (rhip_ctx_release_before_final_exp)"""
        self._check(self.lib.rhip_ctx_release_before_final_exp(self.ctx, waiter.ctx))

    def release_when_miller_resident(self, waiter):
        """one-shot: `waiter`'s stream goes on as soon as the blocks of this context's next Miller launch are resident
        (rhip_ctx_release_when_miller_resident); waiter None withdraws"""
        self._check(self.lib.rhip_ctx_release_when_miller_resident(self.ctx, waiter.ctx if waiter is not None else None))

    def wait_for(self, other):
        """order this context's future work after everything submitted to `other` so far (no host wait)"""
        self._check(self.lib.rhip_ctx_wait_for(self.ctx, other.ctx))

    def upload_async(self, dev, host_ptr, nbytes):
        self._check(self.lib.rhip_upload_async(self.ctx, dev.ptr, host_ptr, ctypes.c_size_t(nbytes)))

    def download_async(self, host_ptr, dev, nbytes):
        self._check(self.lib.rhip_download_async(self.ctx, host_ptr, dev.ptr, ctypes.c_size_t(nbytes)))

    # ------------------------------------------------------------------ tables
    def g1_table(self, base): return _Table(self, "g1", base)
    def g2_table(self, base): return _Table(self, "g2", base)
    def gt_table(self, base): return _Table(self, "gt", base)

    def calibrate(self, variant, iters):
        ms, ops = ctypes.c_double(), ctypes.c_double()
        self._check(self.lib.rhip_calibrate_mad(self.ctx, ctypes.c_int32(variant), ctypes.c_uint32(iters),
                                                ctypes.byref(ms), ctypes.byref(ops)))
        return ms.value, ops.value


class _Table:
    _OUT = {"g1": G1, "g2": G2, "gt": GT}

    def __init__(self, eng, kind, base):
        self.eng, self.kind = eng, kind
        self.h = ctypes.c_void_p()
        eng._check(getattr(eng.lib, "rhip_%s_table_create" % kind)(eng.ctx, bytes(base), ctypes.byref(self.h)))

    def mul(self, scalars):
        fn = "rhip_%s_table_%s" % (self.kind, "pow" if self.kind == "gt" else "mul")
        eng = self.eng
        n = len(scalars)
        k = eng.upload(b"".join(scalars))
        sz = self._OUT[self.kind]
        out = eng.alloc(n * sz)
        eng._check(getattr(eng.lib, fn)(eng.ctx, self.h, ctypes.c_size_t(n), k.ptr, out.ptr))
        raw = eng.download(out, n * sz)
        return [raw[i * sz:(i + 1) * sz] for i in range(n)]

    def add_w16(self):
        """16-bit windows beside the 8-bit ones (rhip_{g1,g2,gt}_table_add_w16)"""
        self.eng._check(getattr(self.eng.lib, "rhip_%s_table_add_w16" % self.kind)(self.eng.ctx, self.h))

    def add_wide(self, w_bits):
        """signed w_bits-wide windows (G1 only, rhip_g1_table_add_wide)"""
        assert self.kind == "g1"
        self.eng._check(self.eng.lib.rhip_g1_table_add_wide(self.eng.ctx, self.h, ctypes.c_int32(int(w_bits))))

    def destroy(self):
        if self.h:
            getattr(self.eng.lib, "rhip_%s_table_destroy" % self.kind)(self.h)
            self.h = None


# ---------------------------------------------------------------------- Level B: AC17 (device-buffer level)
class Ac17Pk:
    """Device tables of an Ac17PublicKey (g, h_a[3], e_gh_ka[2])."""

    def __init__(self, eng, g, h_a, e_gh_ka):
        self.eng = eng
        self.h = ctypes.c_void_p()
        eng._check(eng.lib.rhip_ac17_pk_create(eng.ctx, bytes(g), b"".join(h_a), b"".join(e_gh_ka), ctypes.byref(self.h)))

    def set_g_window(self, w_bits):
        """signed w_bits-wide windows for g (rhip_ac17_pk_set_g_window): fewer additions per row, more HBM"""
        self.eng._check(self.eng.lib.rhip_ac17_pk_set_g_window(self.eng.ctx, self.h, ctypes.c_int32(int(w_bits))))

    def destroy(self):
        if self.h:
            self.eng.lib.rhip_ac17_pk_destroy(self.h)
            self.h = None


class Ghw11Keys:
    """Device tables of the G2 side of a GHW11 key pair (rhip_ghw11_keys: g2, g2_a, the master key's g2_alpha), 128 host bytes each."""

    def __init__(self, eng, g2, g2_a, g2_alpha):
        self.eng = eng
        self.h = ctypes.c_void_p()
        eng._check(eng.lib.rhip_ghw11_keys_create(eng.ctx, bytes(g2), bytes(g2_a), bytes(g2_alpha), ctypes.byref(self.h)))

    def destroy(self):
        if self.h:
            self.eng.lib.rhip_ghw11_keys_destroy(self.h)
            self.h = None


class DnfKeys:
    """Device tables of a BDABE authority's / the MKE08 master's user-key bases (rhip_dnf_keys: p1, g1, a1 in G1 with 64 host bytes each,
    p2, g2, a2 in G2 with 128)."""

    def __init__(self, eng, p1, g1, p2, g2, a1, a2):
        self.eng = eng
        self.h = ctypes.c_void_p()
        eng._check(eng.lib.rhip_dnf_keys_create(eng.ctx, bytes(p1), bytes(g1), bytes(p2), bytes(g2), bytes(a1), bytes(a2), ctypes.byref(self.h)))

    def destroy(self):
        if self.h:
            self.eng.lib.rhip_dnf_keys_destroy(self.h)
            self.h = None


def _sz(n):
    return ctypes.c_size_t(int(n))


def wide_windows(w):
    """number of signed w-bit windows of a 254-bit scalar (engine.hip: wide_windows)"""
    return (254 + w - 1) // w


def wide_count(w, i):
    """entries of window i of the signed w-bit table (engine.hip: wide_count)"""
    n = wide_windows(w)
    return (1 << (w - 1)) if i < n - 1 else (1 << (254 - w * (n - 1)))


def ac17_encrypt_dev(eng, pk, n_items, dA, ditem_A_off, dct_row_off, total_rows, ds, dmsg, dc0, dc, dcp):
    eng._check(eng.lib.rhip_ac17_cp_encrypt_batch(eng.ctx, pk.h, _sz(n_items), dA.ptr, ditem_A_off.ptr, dct_row_off.ptr,
                                                  _sz(total_rows), ds.ptr, dmsg.ptr, dc0.ptr, dc.ptr, dcp.ptr))


def ac17_keygen_dev(eng, g_table, h_table, dgk, dainv, db, n_items, n_attrs, dH, dH01, dr, dsigma, dsigmap, dk0, dk, dkp):
    eng._check(eng.lib.rhip_ac17_cp_keygen_batch(eng.ctx, g_table.h, h_table.h, dgk.ptr, dainv.ptr, db.ptr, _sz(n_items),
                                                 _sz(n_attrs), dH.ptr, dH01.ptr, dr.ptr, dsigma.ptr, dsigmap.ptr,
                                                 dk0.ptr, dk.ptr, dkp.ptr))


def ac17_decrypt_dev(eng, n_items, dct_c0, dct_c, dct_row_off, dct_cp, dsk_k0, dsk_k, dsk_row_off, dsk_kp, dsk_idx,
                     dct_sel, dct_sel_off, dsk_sel, dsk_sel_off, dout):
    eng._check(eng.lib.rhip_ac17_cp_decrypt_batch(eng.ctx, _sz(n_items), dct_c0.ptr, dct_c.ptr, dct_row_off.ptr, dct_cp.ptr,
                                                  dsk_k0.ptr, dsk_k.ptr, dsk_row_off.ptr, dsk_kp.ptr, dsk_idx.ptr,
                                                  dct_sel.ptr, dct_sel_off.ptr, dsk_sel.ptr, dsk_sel_off.ptr, dout.ptr))


class Ac17SkLines:
    """Prepared Miller-loop lines of n_sk secret keys' k_0 (rhip_ac17_sk_prepare)."""

    def __init__(self, eng, n_sk, dsk_k0):
        self.eng = eng
        self.h = ctypes.c_void_p()
        eng._check(eng.lib.rhip_ac17_sk_prepare(eng.ctx, _sz(n_sk), dsk_k0.ptr, ctypes.byref(self.h)))

    def destroy(self):
        if self.h:
            self.eng.lib.rhip_ac17_sk_lines_destroy(self.h)
            self.h = None


def ac17_decrypt_prepared_dev(eng, n_items, dct_c0, dct_c, dct_row_off, dct_cp, sk_lines, dsk_k, dsk_row_off, dsk_kp, dsk_idx,
                              dct_sel, dct_sel_off, dsk_sel, dsk_sel_off, dout):
    eng._check(eng.lib.rhip_ac17_cp_decrypt_batch_prepared(eng.ctx, _sz(n_items), dct_c0.ptr, dct_c.ptr, dct_row_off.ptr, dct_cp.ptr,
                                                           sk_lines.h, dsk_k.ptr, dsk_row_off.ptr, dsk_kp.ptr, dsk_idx.ptr,
                                                           dct_sel.ptr, dct_sel_off.ptr, dsk_sel.ptr, dsk_sel_off.ptr, dout.ptr))


# ---------------------------------------------------------------------- Level B: bsw / lsw / aw11 (device-buffer level)
def _p(x):
    """DevBuf / handle / None -> pointer argument"""
    if x is None:
        return ctypes.c_void_p(0)
    if hasattr(x, "ptr"):
        return x.ptr
    if hasattr(x, "h"):
        return x.h
    return x


class DevTreeTables:
    """hostprep.TreeTables uploaded once (flattened policy trees: include/rabe_hip.h)."""

    def __init__(self, eng, tt):
        self.tt = tt
        self.path_off = eng.upload_u32(tt.path_off)
        self.path_gate = eng.upload_u32(tt.path_gate or [0])
        self.path_x = eng.upload_u32(tt.path_x or [0])
        self.gate_k = eng.upload_u32(tt.gate_k or [0])
        self.gate_coef_off = eng.upload_u32(tt.gate_coef_off or [0])
        self.leaf_hash = eng.upload(b"".join(fr_bytes(h) for h in tt.leaf_hash))


class G2Lines:
    """Prepared Miller-loop lines of n G2 points (rhip_g2_lines_prepare)."""

    def __init__(self, eng, n, dq):
        self.eng = eng
        self.h = ctypes.c_void_p()
        eng._check(eng.lib.rhip_g2_lines_prepare(eng.ctx, _sz(n), dq.ptr, ctypes.byref(self.h)))

    @classmethod
    def reserve(cls, eng, capacity):
        """a handle with room for `capacity` points, every block empty (rhip_g2_lines_reserve)"""
        self = cls.__new__(cls)
        self.eng = eng
        self.h = ctypes.c_void_p()
        eng._check(eng.lib.rhip_g2_lines_reserve(eng.ctx, _sz(capacity), ctypes.byref(self.h)))
        return self

    def prepare_range(self, first, n, dq):
        """the lines of the n points at dq (a device buffer, or None for n = 0) into blocks [first, first + n) (rhip_g2_lines_prepare_range)"""
        self.eng._check(self.eng.lib.rhip_g2_lines_prepare_range(self.eng.ctx, self.h, _sz(first), _sz(n), _p(dq)))

    def scrub_range(self, first, n):
        """blocks [first, first + n) back to empty (rhip_g2_lines_scrub_range)"""
        self.eng._check(self.eng.lib.rhip_g2_lines_scrub_range(self.eng.ctx, self.h, _sz(first), _sz(n)))

    def range_is_zero(self, first, n):
        """True iff every line word of the range is zero in both copies and every flag says empty (rhip_g2_lines_range_is_zero)"""
        out = ctypes.c_int32(-1)
        self.eng._check(self.eng.lib.rhip_g2_lines_range_is_zero(self.eng.ctx, self.h, _sz(first), _sz(n), ctypes.byref(out)))
        return bool(out.value)

    def nbytes(self):
        """device memory the handle holds (rhip_g2_lines_bytes)"""
        self.eng.lib.rhip_g2_lines_bytes.restype = ctypes.c_size_t
        return int(self.eng.lib.rhip_g2_lines_bytes(self.h))

    def destroy(self):
        if self.h:
            self.eng.lib.rhip_g2_lines_destroy(self.h)
            self.h = None


def ghw11_transform_dev(eng, n_items, max_pairs, total_pairs, n_sel, d_pair_off, d_sel_start, d_sel_ct_row, d_sel_tk_attr, d_sel_coeff, d_ct_c1, d_ct_c,
                        d_ct_d, d_ct_row_off, tk_lines, d_out):
    """n transforms under ONE key (rhip_ghw11_transform_batch); tk_lines: G2Lines over k_z, l_z, k_x[0], ..."""
    eng._check(eng.lib.rhip_ghw11_transform_batch(eng.ctx, _sz(n_items), _sz(max_pairs), _sz(total_pairs), _sz(n_sel), _p(d_pair_off), _p(d_sel_start),
                                                  _p(d_sel_ct_row), _p(d_sel_tk_attr), _p(d_sel_coeff), _p(d_ct_c1), _p(d_ct_c), _p(d_ct_d),
                                                  _p(d_ct_row_off), _p(tk_lines), _p(d_out)))


def ghw11_transform_keyed_dev(eng, n_items, max_pairs, total_pairs, n_sel, d_pair_off, d_sel_start, d_sel_ct_row, d_sel_tk_attr, d_sel_coeff, d_ct_c1,
                              d_ct_c, d_ct_d, d_ct_row_off, d_item_line_base, d_item_ok, store_lines, d_out):
    """the same under MANY keys (rhip_ghw11_transform_batch_keyed): store_lines = G2Lines over the elements of all keys, key after key;
    d_item_line_base[i] = the index of the k_z of item i's key; d_item_ok (or None): 0 = the item is skipped and its output is zeros"""
    eng._check(eng.lib.rhip_ghw11_transform_batch_keyed(eng.ctx, _sz(n_items), _sz(max_pairs), _sz(total_pairs), _sz(n_sel), _p(d_pair_off),
                                                        _p(d_sel_start), _p(d_sel_ct_row), _p(d_sel_tk_attr), _p(d_sel_coeff), _p(d_ct_c1), _p(d_ct_c),
                                                        _p(d_ct_d), _p(d_ct_row_off), _p(d_item_line_base), _p(d_item_ok), _p(store_lines), _p(d_out)))


class BswPk:
    """Device tables of a CpAbePublicKey (g1, g2, h, e_gg_alpha)."""

    def __init__(self, eng, g1, g2, h, e_gg_alpha):
        self.eng = eng
        self.h = ctypes.c_void_p()
        eng._check(eng.lib.rhip_bsw_pk_create(eng.ctx, bytes(g1), bytes(g2), bytes(h), bytes(e_gg_alpha), ctypes.byref(self.h)))

    def destroy(self):
        if self.h:
            self.eng.lib.rhip_bsw_pk_destroy(self.h)
            self.h = None


class BswSkLines:
    def __init__(self, eng, n_sk, total_attrs, dsk_d, dsk_dj_g2):
        self.eng = eng
        self.h = ctypes.c_void_p()
        eng._check(eng.lib.rhip_bsw_sk_prepare(eng.ctx, _sz(n_sk), _sz(total_attrs), dsk_d.ptr, dsk_dj_g2.ptr, ctypes.byref(self.h)))

    def destroy(self):
        if self.h:
            self.eng.lib.rhip_bsw_sk_lines_destroy(self.h)
            self.h = None


def bsw_encrypt_dev(eng, pk, n_items, total_leaves, d_item_leaf_off, d_item_tree_leaf, d_item_tree_gate, dtt, d_secret, d_coef,
                    d_item_coef_off, d_msg, d_c, d_cp, d_cy_g1, d_cy_g2):
    eng._check(eng.lib.rhip_bsw_encrypt_batch(eng.ctx, pk.h, _sz(n_items), _sz(total_leaves), _p(d_item_leaf_off), _p(d_item_tree_leaf),
                                              _p(d_item_tree_gate), _p(dtt.path_off), _p(dtt.path_gate), _p(dtt.path_x), _p(dtt.gate_k),
                                              _p(dtt.gate_coef_off), _p(dtt.leaf_hash), _p(d_secret), _p(d_coef), _p(d_item_coef_off),
                                              _p(d_msg), _p(d_c), _p(d_cp), _p(d_cy_g1), _p(d_cy_g2)))


class Ghw11Pk:
    """Device tables of the G1 / Gt side of a Ghw11PublicKey (g1, g1_a, e_gg_alpha)."""

    def __init__(self, eng, g1, g1_a, e_gg_alpha):
        self.eng = eng
        self.h = ctypes.c_void_p()
        eng._check(eng.lib.rhip_ghw11_pk_create(eng.ctx, bytes(g1), bytes(g1_a), bytes(e_gg_alpha), ctypes.byref(self.h)))

    def destroy(self):
        if self.h:
            self.eng.lib.rhip_ghw11_pk_destroy(self.h)
            self.h = None


def ghw11_encrypt_dev(eng, pk, n_items, total_leaves, d_item_leaf_off, d_item_tree_leaf, d_item_tree_gate, dtt, d_secret, d_coef,
                      d_item_coef_off, d_t, d_msg, d_c, d_c1, d_cd):
    """rhip_ghw11_encrypt_batch: d_t holds one draw per leaf row, d_cd takes C and D of every row (2 x 64 bytes per row)"""
    eng._check(eng.lib.rhip_ghw11_encrypt_batch(eng.ctx, pk.h, _sz(n_items), _sz(total_leaves), _p(d_item_leaf_off), _p(d_item_tree_leaf),
                                                _p(d_item_tree_gate), _p(dtt.path_off), _p(dtt.path_gate), _p(dtt.path_x), _p(dtt.gate_k),
                                                _p(dtt.gate_coef_off), _p(dtt.leaf_hash), _p(d_secret), _p(d_coef), _p(d_item_coef_off),
                                                _p(d_t), _p(d_msg), _p(d_c), _p(d_c1), _p(d_cd)))


def bsw_decrypt_dev(eng, n_items, max_pairs, total_pairs, d_pair_off, d_sel_start, d_sel_ct_leaf, d_sel_sk_attr, d_sel_coeff,
                    d_ct_c, d_ct_cp, d_ct_cy_g1, d_ct_cy_g2, d_ct_leaf_off, d_sk_d, d_sk_dj_g1, d_sk_dj_g2, d_sk_attr_off, d_sk_idx,
                    sk_lines, d_out):
    eng._check(eng.lib.rhip_bsw_decrypt_batch(eng.ctx, _sz(n_items), _sz(max_pairs), _sz(total_pairs), _p(d_pair_off), _p(d_sel_start),
                                              _p(d_sel_ct_leaf), _p(d_sel_sk_attr), _p(d_sel_coeff), _p(d_ct_c), _p(d_ct_cp), _p(d_ct_cy_g1),
                                              _p(d_ct_cy_g2), _p(d_ct_leaf_off), _p(d_sk_d), _p(d_sk_dj_g1), _p(d_sk_dj_g2),
                                              _p(d_sk_attr_off), _p(d_sk_idx), _p(sk_lines), _p(d_out)))


def bsw_decrypt_one_sk_dev(eng, n_items, max_pairs, total_pairs, n_sel, d_pair_off, d_sel_start, d_sel_ct_leaf, d_sel_sk_attr, d_sel_coeff,
                           d_ct_c, d_ct_cp, d_ct_cy_g1, d_ct_cy_g2, d_ct_leaf_off, d_sk_d, d_sk_dj_g1, d_sk_dj_g2, d_sk_attr_off, sk_lines, d_out):
    """every item is decrypted with the SAME key (rhip_bsw_decrypt_batch_one_sk): -z_e * Dj.g1 is computed once per selection entry"""
    eng._check(eng.lib.rhip_bsw_decrypt_batch_one_sk(eng.ctx, _sz(n_items), _sz(max_pairs), _sz(total_pairs), _sz(n_sel), _p(d_pair_off), _p(d_sel_start),
                                                     _p(d_sel_ct_leaf), _p(d_sel_sk_attr), _p(d_sel_coeff), _p(d_ct_c), _p(d_ct_cp), _p(d_ct_cy_g1),
                                                     _p(d_ct_cy_g2), _p(d_ct_leaf_off), _p(d_sk_d), _p(d_sk_dj_g1), _p(d_sk_dj_g2), _p(d_sk_attr_off),
                                                     _p(sk_lines), _p(d_out)))


class LswPk:
    def __init__(self, eng, g1, g2):
        self.eng = eng
        self.h = ctypes.c_void_p()
        eng._check(eng.lib.rhip_lsw_pk_create(eng.ctx, bytes(g1), bytes(g2), ctypes.byref(self.h)))

    def destroy(self):
        if self.h:
            self.eng.lib.rhip_lsw_pk_destroy(self.h)
            self.h = None


def lsw_keygen_dev(eng, pk, n_items, total_leaves, d_item_leaf_off, d_item_tree_leaf, d_item_tree_gate, dtt, d_alpha, d_coef, d_item_coef_off,
                   d_rand, d_d1, d_d2):
    eng._check(eng.lib.rhip_lsw_keygen_batch(eng.ctx, pk.h, _sz(n_items), _sz(total_leaves), _p(d_item_leaf_off), _p(d_item_tree_leaf),
                                             _p(d_item_tree_gate), _p(dtt.path_off), _p(dtt.path_gate), _p(dtt.path_x), _p(dtt.gate_k),
                                             _p(dtt.gate_coef_off), _p(dtt.leaf_hash), _p(d_alpha), _p(d_coef), _p(d_item_coef_off), _p(d_rand),
                                             _p(d_d1), _p(d_d2)))


def lsw_keygen_signed_dev(eng, pk, n_items, total_leaves, d_item_leaf_off, d_item_tree_leaf, d_item_tree_gate, dtt, d_leaf_neg, d_alpha, d_b, h_g1,
                          d_coef, d_item_coef_off, d_rand, d_d1, d_d2, d_d3, d_d4, d_d5):
    """rhip_lsw_keygen_batch_signed: policies with negative leaves ("!x"); h_g1 = the master key's h_g1 (64 host bytes)"""
    eng._check(eng.lib.rhip_lsw_keygen_batch_signed(eng.ctx, pk.h, _sz(n_items), _sz(total_leaves), _p(d_item_leaf_off), _p(d_item_tree_leaf),
                                                    _p(d_item_tree_gate), _p(dtt.path_off), _p(dtt.path_gate), _p(dtt.path_x), _p(dtt.gate_k),
                                                    _p(dtt.gate_coef_off), _p(dtt.leaf_hash), _p(d_leaf_neg), _p(d_alpha), _p(d_b), bytes(h_g1),
                                                    _p(d_coef), _p(d_item_coef_off), _p(d_rand), _p(d_d1), _p(d_d2), _p(d_d3), _p(d_d4), _p(d_d5)))


def lsw_decrypt_dev(eng, n_items, max_pairs, total_pairs, n_sel, d_pair_off, d_sel_start, d_sel_sk_leaf, d_sel_ct_attr, d_sel_coeff, d_ct_e1,
                    d_ct_e2, d_ct_e1j, d_ct_attr_off, d_ct_idx, d_sk_d1, d_sk_d2, d_sk_leaf_off, d_sk_idx, e2_lines, d_out):
    eng._check(eng.lib.rhip_lsw_decrypt_batch(eng.ctx, _sz(n_items), _sz(max_pairs), _sz(total_pairs), _sz(n_sel), _p(d_pair_off), _p(d_sel_start),
                                              _p(d_sel_sk_leaf), _p(d_sel_ct_attr), _p(d_sel_coeff), _p(d_ct_e1), _p(d_ct_e2), _p(d_ct_e1j),
                                              _p(d_ct_attr_off), _p(d_ct_idx), _p(d_sk_d1), _p(d_sk_d2), _p(d_sk_leaf_off), _p(d_sk_idx),
                                              _p(e2_lines), _p(d_out)))


def lsw_decrypt_one_ct_dev(eng, n_items, max_pairs, total_pairs, n_sel, d_pair_off, d_sel_start, d_sel_sk_leaf, d_sel_ct_attr, d_sel_coeff, d_ct_e1,
                           d_ct_e2, d_ct_e1j, d_sk_d1, d_sk_d2, d_sk_leaf_off, d_sk_idx, e2_lines, d_out):
    """every item decrypts the SAME ciphertext (rhip_lsw_decrypt_batch_one_ct): the scaled G1 arguments are computed once per selection entry"""
    eng._check(eng.lib.rhip_lsw_decrypt_batch_one_ct(eng.ctx, _sz(n_items), _sz(max_pairs), _sz(total_pairs), _sz(n_sel), _p(d_pair_off), _p(d_sel_start),
                                                     _p(d_sel_sk_leaf), _p(d_sel_ct_attr), _p(d_sel_coeff), _p(d_ct_e1), _p(d_ct_e2), _p(d_ct_e1j),
                                                     _p(d_sk_d1), _p(d_sk_d2), _p(d_sk_leaf_off), _p(d_sk_idx), _p(e2_lines), _p(d_out)))


def lsw_decrypt_one_sk_dev(eng, n_items, max_pairs, total_pairs, n_sel, d_pair_off, d_sel_start, d_sel_sk_leaf, d_sel_ct_attr, d_sel_coeff, n_groups,
                           d_group_off, d_item_group, d_ct_e1, d_ct_e2, d_ct_e1j, d_ct_attr_off, d_sk_d1, sk_d2_lines, d_out):
    """every item is decrypted with the SAME key (rhip_lsw_decrypt_batch_one_sk): the key-side Miller loops replay sk_d2_lines (G2Lines over the
    key's D2 rows) and sum -c_e D1_e is computed once per selection group (entries of group g: [group_off[g], group_off[g+1]))"""
    eng._check(eng.lib.rhip_lsw_decrypt_batch_one_sk(eng.ctx, _sz(n_items), _sz(max_pairs), _sz(total_pairs), _sz(n_sel), _p(d_pair_off), _p(d_sel_start),
                                                     _p(d_sel_sk_leaf), _p(d_sel_ct_attr), _p(d_sel_coeff), _sz(n_groups), _p(d_group_off),
                                                     _p(d_item_group), _p(d_ct_e1), _p(d_ct_e2), _p(d_ct_e1j), _p(d_ct_attr_off), _p(d_sk_d1),
                                                     _p(sk_d2_lines), _p(d_out)))


def dnf_decrypt_one_uk_dev(eng, n_items, n_classes, d_item_class, d_class_s1, d_class_skip, d_neg_u1, key_lines, d_ct_g1, d_ct_g2, d_lead, d_out):
    """BDABE / MKE08 decrypt under ONE user key in the four-pair form (rhip_dnf_decrypt_batch_one_uk): out[i] = lead[i] * e(e2, S2) * e(S1, e3) *
    e(-e4, u2) * e(-u1, e5).  key_lines: G2Lines over [sk.u2, S2 of class 0, S2 of class 1, ...]; d_ct_g1 = (e2, e4) and d_ct_g2 = (e3, e5) per
    item; d_class_skip[c]: bit 0 S1 = O, bit 1 S2 = O"""
    eng._check(eng.lib.rhip_dnf_decrypt_batch_one_uk(eng.ctx, _sz(n_items), _sz(n_classes), _p(d_item_class), _p(d_class_s1), _p(d_class_skip), _p(d_neg_u1),
                                                     _p(key_lines), _p(d_ct_g1), _p(d_ct_g2), _p(d_lead), _p(d_out)))


def lsw_encrypt_rows_dev(eng, g1_tbl, g1_b_tbl, g1_b2_tbl, h_b_tbl, n_items, total_rows, d_item_row_off, d_item_hash_off, d_hash, d_secret, d_sx,
                         d_out):
    """rhip_lsw_encrypt_rows: the attribute rows of n_items lsw::encrypt calls, one lane per row (k_lsw_enc_rows).  The four tables are
    Engine.g1_table objects with 16-bit windows (add_w16) of g1, g1_b, g1_b2 and h_b; d_out takes e3, e4, e5 of every row (3 x 64 bytes)"""
    eng._check(eng.lib.rhip_lsw_encrypt_rows(eng.ctx, g1_tbl.h, g1_b_tbl.h, g1_b2_tbl.h, h_b_tbl.h, _sz(n_items), _sz(total_rows), _p(d_item_row_off),
                                             _p(d_item_hash_off), _p(d_hash), _p(d_secret), _p(d_sx), _p(d_out)))


class Aw11Pk:
    def __init__(self, eng, g1, g2, egg_alpha, g2_y):
        self.eng = eng
        self.h = ctypes.c_void_p()
        eng._check(eng.lib.rhip_aw11_pk_create(eng.ctx, bytes(g1), bytes(g2), _sz(len(egg_alpha)), b"".join(egg_alpha), b"".join(g2_y),
                                               ctypes.byref(self.h)))

    def table_form(self):
        """rhip_aw11_pk_table_form: 0 plain 8-bit per-attribute tables, 1 16-bit ones, 9 ... 14 signed windows of that width"""
        form = ctypes.c_int32(-1)
        self.eng._check(self.eng.lib.rhip_aw11_pk_table_form(self.h, ctypes.byref(form)))
        return form.value

    def destroy(self):
        if self.h:
            self.eng.lib.rhip_aw11_pk_destroy(self.h)
            self.h = None


def aw11_encrypt_dev(eng, pk, n_items, total_rows, d_item_row_off, d_item_tree_leaf, d_item_tree_gate, d_item_n_coef, dtt, d_leaf_attr, d_s,
                     d_coef, d_item_coef_off, d_rand, d_msg, d_c0, d_c1, d_c2, d_c3):
    eng._check(eng.lib.rhip_aw11_encrypt_batch(eng.ctx, pk.h, _sz(n_items), _sz(total_rows), _p(d_item_row_off), _p(d_item_tree_leaf),
                                               _p(d_item_tree_gate), _p(d_item_n_coef), _p(dtt.path_off), _p(dtt.path_gate), _p(dtt.path_x),
                                               _p(dtt.gate_k), _p(dtt.gate_coef_off), _p(d_leaf_attr), _p(d_s), _p(d_coef), _p(d_item_coef_off),
                                               _p(d_rand), _p(d_msg), _p(d_c0), _p(d_c1), _p(d_c2), _p(d_c3)))


def aw11_decrypt_dev(eng, n_items, max_pairs, total_pairs, n_sel, d_pair_off, d_sel_start, d_sel_ct_row, d_sel_sk_attr, d_sel_coeff, d_ct_c0,
                     d_ct_c1, d_ct_c2, d_ct_c3, d_ct_row_off, d_sk_hash, d_sk_k, d_sk_attr_off, d_sk_idx, d_out, w4=False):
    """rhip_aw11_decrypt_batch; w4: rhip_aw11_decrypt_batch_w4, the same call with the leading factor over width-4 windows"""
    fn = eng.lib.rhip_aw11_decrypt_batch_w4 if w4 else eng.lib.rhip_aw11_decrypt_batch
    eng._check(fn(eng.ctx, _sz(n_items), _sz(max_pairs), _sz(total_pairs), _sz(n_sel), _p(d_pair_off), _p(d_sel_start),
                  _p(d_sel_ct_row), _p(d_sel_sk_attr), _p(d_sel_coeff), _p(d_ct_c0), _p(d_ct_c1), _p(d_ct_c2),
                  _p(d_ct_c3), _p(d_ct_row_off), _p(d_sk_hash), _p(d_sk_k), _p(d_sk_attr_off), _p(d_sk_idx), _p(d_out)))
