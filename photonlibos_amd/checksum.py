"""Host-side mirror of PhotonLibOS common/checksum (CRC32C) over the C-ABI
library libphoton_checksum.so.

Two layers, both thin bindings (no arithmetic in Python):

* Drop-in entry points with the reference's names and meaning
  (common/checksum/crc32c.h:20-92): crc32c, crc32c_extend, crc32c_series,
  crc32c_combine, crc32c_combine_series, crc32c_trim (+ the _sw/_hw engines),
  bound to the library's exported C++ symbols and dispatch pointers.
* The batched device engine (include/photon_crc/crc32c_gpu.h):
  batch_strided / batch_iov / batch_msg / combine_batch. Arguments are device
  pointers (ints) or objects exposing .data_ptr() (e.g. torch tensors);
  `stream` is a hipStream_t handle (int) or an object with .cuda_stream.
  Errors raise CrcError; nothing falls back to the CPU.
"""
import ctypes

from ._native import lib

__all__ = [
    "CrcError",
    "crc32c", "crc32c_extend", "crc32c_sw", "crc32c_hw", "crc32c_hw_simple", "crc32c_hw_portable",
    "crc32c_series", "crc32c_series_sw", "crc32c_series_hw",
    "crc32c_combine", "crc32c_combine_sw", "crc32c_combine_hw",
    "crc32c_combine_series", "crc32c_combine_series_sw", "crc32c_combine_series_hw",
    "crc32c_trim", "crc32c_trim_sw", "crc32c_trim_hw", "is_crc32c_hw_available",
    "device_count", "set_lanes_per_buffer", "host_batch_strided", "host_batch_strided_multi", "batch_strided_shards",
    "Shard", "batch_strided", "batch_strided_sync", "batch_iov", "batch_msg",
    "copy_batch_strided", "copy_batch_iov", "gather_msg_n",
    "crc64ecma", "crc64ecma_extend", "crc64ecma_sw", "crc64ecma_hw", "crc64ecma_combine", "crc64ecma_series",
    "crc64ecma_combine_series", "crc64ecma_trim",
    "copy_batch64_strided", "copy_batch64_iov", "gather64_msg_n",
    "copy_msg_iov_n", "copy_msg64_iov_n",
    "copy_msg_iov_seg_n", "copy_msg64_iov_seg_n", "SEG_OF_SRC", "SEG_OF_DST",
    "copy_msg_iov_seg2_n", "copy_msg64_iov_seg2_n",
    "copy_msg_iov_window_n", "copy_msg64_iov_window_n", "window_work_bytes",
    "copy_extend_device", "copy_extend64_device",
    "copy_parts_device", "copy_parts64_device", "batch_parts_device", "batch_parts64_device", "parts_work_bytes",
    "set_parts_piece", "set_host_stage_bytes", "set_file_chunk_bytes",
    "copy_parts_packed_device", "copy_parts64_packed_device", "batch_parts_packed_device",
    "batch_parts64_packed_device", "parts_packed_work_bytes",
    "series64_device", "combine_series64_device", "fold_parts_device", "fold_parts64_device",
    "overwrite_batch_strided", "overwrite_batch_iov", "overwrite_batch64_strided", "overwrite_batch64_iov",
    "patch_device", "patch64_device",
    "xor_batch_strided", "xor_batch_ptr", "xor_batch64_strided", "xor_batch64_ptr",
    "xor_expect_device", "xor_expect64_device",
    "crc64ecma_series_at", "crc64ecma_combine_series_at",
    "scan_work_bytes", "set_scan_tile", "scan_parts_device", "scan_parts64_device",
    "VerifyReport", "verify_work_bytes", "set_verify_tile",
    "verify_device", "verify64_device", "verify_ptr_device", "verify64_ptr_device",
    "stamp_device", "stamp64_device", "stamp_ptr_device", "stamp64_ptr_device",
    "batch64_strided", "batch64_iov", "combine64_batch", "trim64_batch", "batch64_msg_n", "host_batch64_strided", "extend64_device", "extend_spans", "extend64_spans", "Span", "combine_batch", "fill_splitmix", "read_stream", "IOVEC_DTYPE",
]

_CRC_FN = ctypes.CFUNCTYPE(ctypes.c_uint32, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint32)
_SERIES_FN = ctypes.CFUNCTYPE(None, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint32,
                              ctypes.POINTER(ctypes.c_uint32))
_COMB_FN = ctypes.CFUNCTYPE(ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32)
_CSER_FN = ctypes.CFUNCTYPE(ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint32, ctypes.c_uint32)
_TRIM_FN = ctypes.CFUNCTYPE(ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64)


class CrcError(RuntimeError):
    def __init__(self, code, what):
        super().__init__(f"photon_crc error {code}: {what}")
        self.code = code


def _auto(name, proto):
    return proto(lib().auto[name].value)


def _buf(data):
    if isinstance(data, str):
        data = data.encode()
    mv = memoryview(data).cast("B")
    if mv.readonly:
        return bytes(mv), len(mv)
    return (ctypes.c_char * len(mv)).from_buffer(mv), len(mv)


# ---------------------------------------------------------------- drop-in API

def crc32c_extend(data, crc):
    """crc32c_extend(data, nbytes, crc) (crc32c.h:30-33, 39-41)."""
    b, n = _buf(data)
    return _auto("crc32c_auto", _CRC_FN)(ctypes.cast(b, ctypes.c_char_p) if not isinstance(b, bytes) else b,
                                         n, crc & 0xFFFFFFFF)


def crc32c(data):
    """crc32c(data, nbytes) == crc32c_extend(data, nbytes, 0) (crc32c.h:35-45)."""
    return crc32c_extend(data, 0)


def _engine(name):
    def f(data, crc=0):
        b, n = _buf(data)
        return lib().cpp[name](ctypes.cast(b, ctypes.c_char_p) if not isinstance(b, bytes) else b, n,
                               crc & 0xFFFFFFFF)
    f.__name__ = name
    f.__doc__ = f"{name}(buffer, nbytes, crc) (crc32c.h:20-22)."
    return f


crc32c_sw = _engine("crc32c_sw")
crc32c_hw = _engine("crc32c_hw")
crc32c_hw_simple = _engine("crc32c_hw_simple")
crc32c_hw_portable = _engine("crc32c_hw_portable")


def _series(fn, buffer, part_size, n_parts):
    b, n = _buf(buffer)
    out = (ctypes.c_uint32 * max(n_parts, 1))()
    fn(ctypes.cast(b, ctypes.c_char_p) if not isinstance(b, bytes) else b, part_size, n_parts, out)
    return list(out)[:n_parts]


def crc32c_series(buffer, part_size, n_parts):
    """crc32c_series (crc32c.h:47-57): CRCs of n_parts consecutive parts."""
    return _series(_auto("crc32c_series_auto", _SERIES_FN), buffer, part_size, n_parts)


def crc32c_series_sw(buffer, part_size, n_parts):
    return _series(lib().cpp["crc32c_series_sw"], buffer, part_size, n_parts)


def crc32c_series_hw(buffer, part_size, n_parts):
    return _series(lib().cpp["crc32c_series_hw"], buffer, part_size, n_parts)


def crc32c_combine(crc1, crc2, len2):
    """crc32c_combine (crc32c.h:59-66): crc(A||B) from crc(A), crc(B), |B|."""
    return _auto("crc32c_combine_auto", _COMB_FN)(crc1, crc2, len2)


def crc32c_combine_sw(crc1, crc2, len2):
    return lib().cpp["crc32c_combine_sw"](crc1, crc2, len2)


def crc32c_combine_hw(crc1, crc2, len2):
    return lib().cpp["crc32c_combine_hw"](crc1, crc2, len2)


def _cseries(fn, crcs, part_size):
    arr = (ctypes.c_uint32 * max(len(crcs), 1))(*crcs)
    return fn(arr, part_size, len(crcs))


def crc32c_combine_series(crcs, part_size):
    """crc32c_combine_series (crc32c.h:68-74); 0 for an empty list."""
    return _cseries(_auto("crc32c_combine_series_auto", _CSER_FN), crcs, part_size)


def crc32c_combine_series_sw(crcs, part_size):
    return _cseries(lib().cpp["crc32c_combine_series_sw"], crcs, part_size)


def crc32c_combine_series_hw(crcs, part_size):
    return _cseries(lib().cpp["crc32c_combine_series_hw"], crcs, part_size)


def _comp(c):
    crc, size = c
    return (crc & 0xFFFFFFFF) | ((size & 0xFFFFFFFF) << 32)


def _trim(fn, all_, prefix, suffix):
    return fn(_comp(all_), _comp(prefix), _comp(suffix))


def crc32c_trim(all_, prefix, suffix):
    """crc32c_trim (crc32c.h:76-87); components are (crc, size) pairs.
    Inconsistent sizes: returns 0 with errno = EINVAL, like the reference."""
    return _trim(_auto("crc32c_trim_auto", _TRIM_FN), all_, prefix, suffix)


def crc32c_trim_sw(all_, prefix, suffix):
    return _trim(lib().cpp["crc32c_trim_sw"], all_, prefix, suffix)


def crc32c_trim_hw(all_, prefix, suffix):
    return _trim(lib().cpp["crc32c_trim_hw"], all_, prefix, suffix)


def is_crc32c_hw_available():
    """crc32c.h:89-92."""
    L = lib()
    return L.auto["crc32c_auto"].value != ctypes.cast(L.cpp["crc32c_sw"], ctypes.c_void_p).value


# ------------------------------------------------------------ CRC-64/ECMA drop-in

_CRC64_FN = ctypes.CFUNCTYPE(ctypes.c_uint64, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint64)
_COMB64_FN = ctypes.CFUNCTYPE(ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32)
_TRIM64_FN = ctypes.CFUNCTYPE(ctypes.c_uint64, *([ctypes.c_uint64] * 6))


def _cp(b):
    return ctypes.cast(b, ctypes.c_char_p) if not isinstance(b, bytes) else b


def crc64ecma_extend(data, crc):
    """crc64ecma_extend (crc64ecma.h:23-30): inverted in and out (crc.cpp:119-122)."""
    b, n = _buf(data)
    return _auto("crc64ecma_auto", _CRC64_FN)(_cp(b), n, crc & 0xFFFFFFFFFFFFFFFF)


def crc64ecma(data, crc=0):
    """crc64ecma(buffer, nbytes, crc) (crc64ecma.h:36-38)."""
    return crc64ecma_extend(data, crc)


def crc64ecma_sw(data, crc=0):
    b, n = _buf(data)
    return lib().cpp["crc64ecma_sw"](_cp(b), n, crc & 0xFFFFFFFFFFFFFFFF)


def crc64ecma_hw(data, crc=0):
    b, n = _buf(data)
    return lib().cpp["crc64ecma_hw"](_cp(b), n, crc & 0xFFFFFFFFFFFFFFFF)


def crc64ecma_combine(crc1, crc2, len2):
    """crc64ecma_combine (crc64ecma.h:53-58)."""
    return _auto("crc64ecma_combine_auto", _COMB64_FN)(crc1, crc2, len2)


def crc64ecma_series(buffer, part_size, n_parts):
    b, n = _buf(buffer)
    out = (ctypes.c_uint64 * max(n_parts, 1))()
    lib().cpp["crc64ecma_series_sw"](_cp(b), part_size, n_parts, out)
    return list(out)[:n_parts]


def crc64ecma_combine_series(crcs, part_size):
    arr = (ctypes.c_uint64 * max(len(crcs), 1))(*crcs)
    return lib().cpp["crc64ecma_combine_series_sw"](arr, part_size, len(crcs))


def crc64ecma_trim(all_, prefix, suffix):
    """crc64ecma_trim (crc64ecma.h:68-87); components are (crc, size)."""
    return _auto("crc64ecma_trim_auto", _TRIM64_FN)(all_[0], all_[1], prefix[0], prefix[1], suffix[0], suffix[1])


# ---------------------------------------------------------- batched device API

IOVEC_DTYPE = [("base", "<u8"), ("len", "<u8")]  # == struct iovec / photon_crc_iovec


def _ptr(x):
    if x is None:
        return None
    if isinstance(x, int):
        return x
    if hasattr(x, "data_ptr"):
        return x.data_ptr()
    raise TypeError(f"expected a device pointer (int) or an object with data_ptr(), got {type(x)!r}")


def _stream(s):
    if s is None:
        return None
    if isinstance(s, int):
        return s
    return s.cuda_stream


def _check(rc):
    if rc != 0:
        raise CrcError(rc, lib().photon_crc_last_error().decode(errors="replace"))


def device_count():
    """Number of usable gfx950 devices; raises CrcError if there is none."""
    n = lib().photon_crc_device_count()
    if n < 0:
        _check(n)
    return n


def set_lanes_per_buffer(g):
    """Lanes per buffer for the batch kernels (0 = automatic, else 4..64)."""
    _check(lib().photon_crc_set_lanes_per_buffer(g))


def set_batch_grid(workgroups):
    """Workgroups of the persistent batch grids (0 = one per CU, the default)."""
    _check(lib().photon_crc_set_batch_grid(workgroups))


def batch_strided(base, stride, nbytes, count, out, seed=0, seeds=None, stream=None):
    """out[i] = crc32c_extend(base + i*stride, nbytes, seeds[i] or seed). Async."""
    _check(lib().photon_crc32c_batch_strided(_ptr(base), stride, nbytes, count, seed & 0xFFFFFFFF, _ptr(seeds),
                                             _ptr(out), _stream(stream)))


def batch_strided_sync(base, stride, nbytes, count, out, seed=0, seeds=None, stream=None):
    _check(lib().photon_crc32c_batch_strided_sync(_ptr(base), stride, nbytes, count, seed & 0xFFFFFFFF,
                                                  _ptr(seeds), _ptr(out), _stream(stream)))


def host_batch_strided(base, stride, nbytes, count, out, seed=0, seeds=None):
    """Host-memory batch through the device (chunked H2D + kernel + D2H). Synchronous.
    base/out/seeds are host pointers (ints) or objects with data_ptr() (pinned tensors)."""
    _check(lib().photon_crc32c_host_batch_strided(_ptr(base), stride, nbytes, count, seed & 0xFFFFFFFF,
                                                  _ptr(seeds), _ptr(out)))


def host_batch_strided_multi(base, stride, nbytes, count, out, seed=0, seeds=None, ndev=0):
    """host_batch_strided sharded over `ndev` devices of this process (0 = all),
    one host thread per device. Synchronous."""
    _check(lib().photon_crc32c_host_batch_strided_multi(_ptr(base), stride, nbytes, count, seed & 0xFFFFFFFF,
                                                        _ptr(seeds), _ptr(out), ndev))


class Shard(ctypes.Structure):
    """photon_crc_shard (include/photon_crc/crc32c_gpu.h)."""
    _fields_ = [("device", ctypes.c_int), ("d_base", ctypes.c_void_p), ("stride", ctypes.c_uint64),
                ("nbytes", ctypes.c_uint64), ("count", ctypes.c_uint64), ("seed0", ctypes.c_uint32),
                ("d_seeds", ctypes.c_void_p), ("d_out", ctypes.c_void_p), ("stream", ctypes.c_void_p)]


def batch_strided_shards(shards):
    """shards: list of dicts with Shard's fields (pointers as ints or .data_ptr()
    objects). Enqueues batch_strided on every shard's device. Async."""
    arr = (Shard * len(shards))()
    for a, s in zip(arr, shards):
        a.device = s.get("device", 0)
        a.d_base = _ptr(s["d_base"])
        a.stride, a.nbytes, a.count = s["stride"], s["nbytes"], s["count"]
        a.seed0 = s.get("seed0", 0) & 0xFFFFFFFF
        a.d_seeds = _ptr(s.get("d_seeds"))
        a.d_out = _ptr(s["d_out"])
        a.stream = _stream(s.get("stream"))
    _check(lib().photon_crc32c_batch_strided_shards(arr, len(shards)))


def batch_iov(iov, count, out, seed=0, seeds=None, stream=None):
    """out[i] = crc32c_extend(iov[i].base, iov[i].len, seed_i). Async."""
    _check(lib().photon_crc32c_batch_iov(_ptr(iov), count, seed & 0xFFFFFFFF, _ptr(seeds), _ptr(out),
                                         _stream(stream)))


def batch_msg(iov, msg_start, nmsg, seg_out, out, seed=0, seeds=None, stream=None):
    """out[m] = chained crc32c_extend over message m's segments. Async."""
    _check(lib().photon_crc32c_batch_msg(_ptr(iov), _ptr(msg_start), nmsg, seed & 0xFFFFFFFF, _ptr(seeds),
                                         _ptr(seg_out), _ptr(out), _stream(stream)))


def batch_msg_n(iov, msg_start, nmsg, nseg, seg_out, out, seed=0, seeds=None, stream=None):
    """batch_msg with the total segment count supplied (fully asynchronous)."""
    _check(lib().photon_crc32c_batch_msg_n(_ptr(iov), _ptr(msg_start), nmsg, nseg, seed & 0xFFFFFFFF, _ptr(seeds),
                                           _ptr(seg_out), _ptr(out), _stream(stream)))


def copy_batch_strided(src, src_stride, dst, dst_stride, nbytes, count, out, seed=0, seeds=None, stream=None):
    """dst + i*dst_stride receives the nbytes at src + i*src_stride, and out[i] =
    crc32c_extend of them (seeds[i] or seed): copy + CRC in one read. Async."""
    _check(lib().photon_crc32c_copy_batch_strided(_ptr(src), src_stride, _ptr(dst), dst_stride, nbytes, count,
                                                  seed & 0xFFFFFFFF, _ptr(seeds), _ptr(out), _stream(stream)))


def copy_batch_iov(src_iov, dst_ptrs, count, out, seed=0, seeds=None, stream=None):
    """dst_ptrs[i] (a device array of pointers) receives src_iov[i].len bytes from
    src_iov[i].base; out[i] = crc32c_extend(src_i, len_i, seed_i). Async."""
    _check(lib().photon_crc32c_copy_batch_iov(_ptr(src_iov), _ptr(dst_ptrs), count, seed & 0xFFFFFFFF, _ptr(seeds),
                                              _ptr(out), _stream(stream)))


def gather_msg_n(iov, msg_start, nmsg, nseg, dst_ptrs, seg_out, out, seed=0, seeds=None, stream=None):
    """batch_msg_n that also gathers: message m's segments are written back to
    back at dst_ptrs[m] (iovector_view::memcpy_to + Crc32Hasher in one pass). Async."""
    _check(lib().photon_crc32c_gather_msg_n(_ptr(iov), _ptr(msg_start), nmsg, nseg, _ptr(dst_ptrs),
                                            seed & 0xFFFFFFFF, _ptr(seeds), _ptr(seg_out), _ptr(out),
                                            _stream(stream)))


def batch64_strided(base, stride, nbytes, count, out, seed=0, seeds=None, stream=None):
    """out[i] = crc64ecma_extend(base + i*stride, nbytes, seeds[i] or seed) (uint64 out). Async."""
    _check(lib().photon_crc64ecma_batch_strided(_ptr(base), stride, nbytes, count, seed & 0xFFFFFFFFFFFFFFFF,
                                                _ptr(seeds), _ptr(out), _stream(stream)))


def batch64_iov(iov, count, out, seed=0, seeds=None, stream=None):
    """out[i] = crc64ecma_extend(iov[i].base, iov[i].len, seed_i) (uint64 out). Async."""
    _check(lib().photon_crc64ecma_batch_iov(_ptr(iov), count, seed & 0xFFFFFFFFFFFFFFFF, _ptr(seeds), _ptr(out),
                                            _stream(stream)))


def host_batch64_strided(base, stride, nbytes, count, out, seed=0, seeds=None):
    """CRC-64/ECMA host-memory batch (chunked H2D + kernel + D2H). Synchronous."""
    _check(lib().photon_crc64ecma_host_batch_strided(_ptr(base), stride, nbytes, count, seed & 0xFFFFFFFFFFFFFFFF,
                                                     _ptr(seeds), _ptr(out)))


def trim64_batch(all_, prefix, suffix, count, out, nerr=None, stream=None):
    """out[i] = crc64ecma_trim(all_[i], prefix[i], suffix[i]); arrays of 16-byte
    {crc, size} components (device). Async."""
    _check(lib().photon_crc64ecma_trim_batch(_ptr(all_), _ptr(prefix), _ptr(suffix), count, _ptr(out), _ptr(nerr),
                                             _stream(stream)))


def combine64_batch(crc1, crc2, len2, count, out, stream=None):
    """out[i] = crc64ecma_combine(crc1[i], crc2[i], len2[i]) (uint64 crcs, uint32 lengths). Async."""
    _check(lib().photon_crc64ecma_combine_batch(_ptr(crc1), _ptr(crc2), _ptr(len2), count, _ptr(out),
                                                _stream(stream)))


def batch64_msg_n(iov, msg_start, nmsg, nseg, seg_out, out, seed=0, seeds=None, stream=None):
    """out[m] = crc64ecma_extend chained over message m's segments (uint64). Async."""
    _check(lib().photon_crc64ecma_batch_msg_n(_ptr(iov), _ptr(msg_start), nmsg, nseg, seed & 0xFFFFFFFFFFFFFFFF,
                                              _ptr(seeds), _ptr(seg_out), _ptr(out), _stream(stream)))


def copy_batch64_strided(src, src_stride, dst, dst_stride, nbytes, count, out, seed=0, seeds=None, stream=None):
    """copy_batch_strided for CRC-64/ECMA: dst + i*dst_stride receives the nbytes at
    src + i*src_stride, out[i] = crc64ecma_extend of them (uint64 seeds / out). Async."""
    _check(lib().photon_crc64ecma_copy_batch_strided(_ptr(src), src_stride, _ptr(dst), dst_stride, nbytes, count,
                                                     seed & 0xFFFFFFFFFFFFFFFF, _ptr(seeds), _ptr(out),
                                                     _stream(stream)))


def copy_batch64_iov(src_iov, dst_ptrs, count, out, seed=0, seeds=None, stream=None):
    """copy_batch_iov for CRC-64/ECMA: dst_ptrs[i] receives src_iov[i]'s bytes, out[i] =
    crc64ecma_extend(src_i, len_i, seed_i) (uint64). Async."""
    _check(lib().photon_crc64ecma_copy_batch_iov(_ptr(src_iov), _ptr(dst_ptrs), count, seed & 0xFFFFFFFFFFFFFFFF,
                                                 _ptr(seeds), _ptr(out), _stream(stream)))


def gather64_msg_n(iov, msg_start, nmsg, nseg, dst_ptrs, seg_out, out, seed=0, seeds=None, stream=None):
    """batch64_msg_n that also gathers: message m's segments (an object's parts) are
    written back to back at dst_ptrs[m]; seg_out (optional) = crc64ecma per segment. Async."""
    _check(lib().photon_crc64ecma_gather_msg_n(_ptr(iov), _ptr(msg_start), nmsg, nseg, _ptr(dst_ptrs),
                                               seed & 0xFFFFFFFFFFFFFFFF, _ptr(seeds), _ptr(seg_out), _ptr(out),
                                               _stream(stream)))


def copy_msg_iov_n(src_iov, src_start, nsrc, dst_iov, dst_start, ndst, nmsg, out, size=None, seed=0, seeds=None,
                   copied=None, stream=None):
    """iovector_view::memcpy_iov + CRC-32C: message m's source segments
    src_iov[src_start[m]:src_start[m+1]] are copied as one byte stream into its
    destination segments dst_iov[dst_start[m]:dst_start[m+1]], at most size[m]
    bytes (no cap without size); out[m] = crc32c_extend over the copied bytes
    from seed_m, copied[m] (optional, uint64) = their count. Async."""
    _check(lib().photon_crc32c_copy_msg_iov_n(_ptr(src_iov), _ptr(src_start), nsrc, _ptr(dst_iov), _ptr(dst_start),
                                              ndst, nmsg, _ptr(size), seed & 0xFFFFFFFF, _ptr(seeds), _ptr(out),
                                              _ptr(copied), _stream(stream)))


def copy_msg64_iov_n(src_iov, src_start, nsrc, dst_iov, dst_start, ndst, nmsg, out, size=None, seed=0, seeds=None,
                     copied=None, stream=None):
    """copy_msg_iov_n for CRC-64/ECMA (uint64 seeds / out). Async."""
    _check(lib().photon_crc64ecma_copy_msg_iov_n(_ptr(src_iov), _ptr(src_start), nsrc, _ptr(dst_iov),
                                                 _ptr(dst_start), ndst, nmsg, _ptr(size), seed & 0xFFFFFFFFFFFFFFFF,
                                                 _ptr(seeds), _ptr(out), _ptr(copied), _stream(stream)))


SEG_OF_SRC, SEG_OF_DST = 0, 1  # PHOTON_CRC_SEG_OF_SRC / PHOTON_CRC_SEG_OF_DST


def copy_msg_iov_seg_n(src_iov, src_start, nsrc, dst_iov, dst_start, ndst, nmsg, seg_side, seg_out, out, size=None,
                       seed=0, seeds=None, copied=None, stream=None):
    """copy_msg_iov_n that also returns one CRC-32C per segment of one side:
    seg_out has nsrc entries for seg_side = SEG_OF_SRC (0), ndst for SEG_OF_DST
    (1), indexed like that side's descriptors; seg_out[s] = crc32c_extend from
    seed 0 over the bytes of segment s that were copied (0 behind the end of
    the copy), every entry written. out / copied as copy_msg_iov_n. Async."""
    _check(lib().photon_crc32c_copy_msg_iov_seg_n(_ptr(src_iov), _ptr(src_start), nsrc, _ptr(dst_iov),
                                                  _ptr(dst_start), ndst, nmsg, _ptr(size), seed & 0xFFFFFFFF,
                                                  _ptr(seeds), seg_side, _ptr(seg_out), _ptr(out), _ptr(copied),
                                                  _stream(stream)))


def copy_msg64_iov_seg_n(src_iov, src_start, nsrc, dst_iov, dst_start, ndst, nmsg, seg_side, seg_out, out, size=None,
                         seed=0, seeds=None, copied=None, stream=None):
    """copy_msg_iov_seg_n for CRC-64/ECMA (uint64 seeds / seg_out / out). Async."""
    _check(lib().photon_crc64ecma_copy_msg_iov_seg_n(_ptr(src_iov), _ptr(src_start), nsrc, _ptr(dst_iov),
                                                     _ptr(dst_start), ndst, nmsg, _ptr(size),
                                                     seed & 0xFFFFFFFFFFFFFFFF, _ptr(seeds), seg_side, _ptr(seg_out),
                                                     _ptr(out), _ptr(copied), _stream(stream)))


def copy_msg_iov_seg2_n(src_iov, src_start, nsrc, dst_iov, dst_start, ndst, nmsg, src_seg_out, dst_seg_out, out,
                        size=None, seed=0, seeds=None, copied=None, stream=None):
    """copy_msg_iov_n that also returns one CRC-32C per segment of BOTH sides
    from the same read: src_seg_out (nsrc entries) is what copy_msg_iov_seg_n
    writes for SEG_OF_SRC, dst_seg_out (ndst entries) what it writes for
    SEG_OF_DST; every entry of both is written. The two arrays must not overlap
    each other or anything else the call touches. out / copied as
    copy_msg_iov_n. Async."""
    _check(lib().photon_crc32c_copy_msg_iov_seg2_n(_ptr(src_iov), _ptr(src_start), nsrc, _ptr(dst_iov),
                                                   _ptr(dst_start), ndst, nmsg, _ptr(size), seed & 0xFFFFFFFF,
                                                   _ptr(seeds), _ptr(src_seg_out), _ptr(dst_seg_out), _ptr(out),
                                                   _ptr(copied), _stream(stream)))


def copy_msg64_iov_seg2_n(src_iov, src_start, nsrc, dst_iov, dst_start, ndst, nmsg, src_seg_out, dst_seg_out, out,
                          size=None, seed=0, seeds=None, copied=None, stream=None):
    """copy_msg_iov_seg2_n for CRC-64/ECMA (uint64 seeds / seg outs / out). Async."""
    _check(lib().photon_crc64ecma_copy_msg_iov_seg2_n(_ptr(src_iov), _ptr(src_start), nsrc, _ptr(dst_iov),
                                                      _ptr(dst_start), ndst, nmsg, _ptr(size),
                                                      seed & 0xFFFFFFFFFFFFFFFF, _ptr(seeds), _ptr(src_seg_out),
                                                      _ptr(dst_seg_out), _ptr(out), _ptr(copied), _stream(stream)))


def window_work_bytes(nmsg):
    """Bytes of device workspace copy_msg_iov_window_n / copy_msg64_iov_window_n need for nmsg messages."""
    return lib().photon_crc_window_work_bytes(nmsg)


def copy_msg_iov_window_n(src_iov, src_start, nsrc, dst_iov, dst_start, ndst, nmsg, src_seg_out, out, work,
                          skip=None, size=None, seed=0, seeds=None, copied=None, stream=None):
    """The ranged read from checksummed blocks: every source segment of a
    message is read in full and checksummed (src_seg_out, nsrc entries: the
    CRC-32C from seed 0 of each WHOLE segment, to verify against the blocks'
    stored words), and only the window [a, a + k) of the source stream lands in
    the destination iovector, a = min(skip[m], L), k = min(size[m], D, L - a).
    out[m] = the CRC-32C of exactly the window bytes from the message's seed,
    copied[m] = k. work: device memory of at least window_work_bytes(nmsg)
    bytes, 8-byte aligned. Async, capturable."""
    _check(lib().photon_crc32c_copy_msg_iov_window_n(_ptr(src_iov), _ptr(src_start), nsrc, _ptr(dst_iov),
                                                     _ptr(dst_start), ndst, nmsg, _ptr(skip), _ptr(size),
                                                     seed & 0xFFFFFFFF, _ptr(seeds), _ptr(src_seg_out), _ptr(out),
                                                     _ptr(copied), _ptr(work), _stream(stream)))


def copy_msg64_iov_window_n(src_iov, src_start, nsrc, dst_iov, dst_start, ndst, nmsg, src_seg_out, out, work,
                            skip=None, size=None, seed=0, seeds=None, copied=None, stream=None):
    """copy_msg_iov_window_n for CRC-64/ECMA (uint64 seeds / src_seg_out / out). Async."""
    _check(lib().photon_crc64ecma_copy_msg_iov_window_n(_ptr(src_iov), _ptr(src_start), nsrc, _ptr(dst_iov),
                                                        _ptr(dst_start), ndst, nmsg, _ptr(skip), _ptr(size),
                                                        seed & 0xFFFFFFFFFFFFFFFF, _ptr(seeds), _ptr(src_seg_out),
                                                        _ptr(out), _ptr(copied), _ptr(work), _stream(stream)))


def extend64_device(data, nbytes, out, seed=0, stream=None):
    """*out = crc64ecma_extend(data, nbytes, seed) for one long device buffer. Async."""
    _check(lib().photon_crc64ecma_extend_device(_ptr(data), nbytes, seed & 0xFFFFFFFFFFFFFFFF, _ptr(out),
                                                _stream(stream)))


def combine_batch(crc1, crc2, len2, count, out, stream=None):
    """out[i] = crc32c_combine(crc1[i], crc2[i], len2[i]). Async."""
    _check(lib().photon_crc32c_combine_batch(_ptr(crc1), _ptr(crc2), _ptr(len2), count, _ptr(out),
                                             _stream(stream)))


def series_device(buffer, part_size, n_parts, out, stream=None):
    """crc32c_series over device memory (crc32c.h:52-57). Async."""
    _check(lib().photon_crc32c_series_device(_ptr(buffer), part_size, n_parts, _ptr(out), _stream(stream)))


def combine_series_device(crcs, part_size, n_parts, result, stream=None):
    """*result = crc32c_combine_series(crcs, part_size, n_parts) on the device (crc32c.h:71-74). Async."""
    _check(lib().photon_crc32c_combine_series_device(_ptr(crcs), part_size, n_parts, _ptr(result),
                                                     _stream(stream)))


def trim_batch(all_, prefix, suffix, count, out, nerr=None, stream=None):
    """out[i] = crc32c_trim(all_[i], prefix[i], suffix[i]); components are {u32 crc, u32 size}
    pairs (crc32c.h:76-87). *nerr counts inconsistent elements (their out is 0). Async."""
    _check(lib().photon_crc32c_trim_batch(_ptr(all_), _ptr(prefix), _ptr(suffix), count, _ptr(out),
                                          _ptr(nerr) if nerr is not None else None, _stream(stream)))


def extend_device(data, nbytes, seed, out, stream=None):
    """*out = crc32c_extend(data, nbytes, seed) for one long device buffer. Async."""
    _check(lib().photon_crc32c_extend_device(_ptr(data), nbytes, seed & 0xFFFFFFFF, _ptr(out), _stream(stream)))


def copy_extend_device(src, dst, nbytes, seed, out, stream=None):
    """Copy + CRC-32C of one long buffer over the whole device: dst receives the nbytes at src and
    *out = crc32c_extend(src, nbytes, seed), what extend_device gives for the same bytes. Any
    alignment; the payload is read once when (dst - src) % 16 == 0. nbytes == 0 writes the seed. Async."""
    _check(lib().photon_crc32c_copy_extend_device(_ptr(src), _ptr(dst), nbytes, seed & 0xFFFFFFFF, _ptr(out),
                                                  _stream(stream)))


def copy_extend64_device(src, dst, nbytes, out, seed=0, stream=None):
    """copy_extend_device for CRC-64/ECMA: *out = crc64ecma_extend(src, nbytes, seed). Async."""
    _check(lib().photon_crc64ecma_copy_extend_device(_ptr(src), _ptr(dst), nbytes, seed & 0xFFFFFFFFFFFFFFFF,
                                                     _ptr(out), _stream(stream)))


def parts_work_bytes(nparts, max_part_bytes, crc64=False):
    """Bytes of workspace copy_parts*_device / batch_parts*_device need for these arguments under
    the current piece setting (set_parts_piece)."""
    return lib().photon_crc_parts_work_bytes(nparts, max_part_bytes, int(bool(crc64)))


def set_parts_piece(nbytes):
    """Piece size of the parts calls: 0 = automatic (32 KiB), else a multiple of 4 KiB (tuning.h)."""
    _check(lib().photon_crc_set_parts_piece(nbytes))


def set_host_stage_bytes(nbytes):
    """Span of a staging chunk of the host-memory pipeline: 0 = the default (256 MiB), else a multiple of
    256 from 64 KiB to 256 MiB (tuning.h; tests reach the reuse of the staging slots with it)."""
    _check(lib().photon_crc_set_host_stage_bytes(nbytes))


def set_file_chunk_bytes(nbytes):
    """Payload span per chunk of file_strided: 0 = the default (64 MiB), else a multiple of 4 KiB up to
    64 MiB (tuning.h; tests reach the reuse of the two chunk buffers with it)."""
    _check(lib().photon_crc_set_file_chunk_bytes(nbytes))


def _work_bytes(work, work_bytes):
    if work_bytes is not None:
        return work_bytes
    return work.numel() * work.element_size() if hasattr(work, "numel") else 0


def copy_parts_device(src_iov, dst_ptrs, nparts, max_part_bytes, out, work, work_bytes=None, seed=0, seeds=None,
                      stream=None):
    """Copy + CRC-32C of many large parts in one pass over the whole device: dst_ptrs[i] receives the
    first n_i = min(src_iov[i].len, max_part_bytes) bytes of part i and out[i] = crc32c_extend over them
    from seeds[i] or seed, what copy_extend_device gives per part. work: device workspace of at least
    parts_work_bytes(nparts, max_part_bytes) bytes (work_bytes, or the tensor's size). Async, capturable."""
    _check(lib().photon_crc32c_copy_parts_n(_ptr(src_iov), _ptr(dst_ptrs), nparts, max_part_bytes,
                                            seed & 0xFFFFFFFF, _ptr(seeds), _ptr(out), _ptr(work),
                                            _work_bytes(work, work_bytes), _stream(stream)))


def copy_parts64_device(src_iov, dst_ptrs, nparts, max_part_bytes, out, work, work_bytes=None, seed=0, seeds=None,
                        stream=None):
    """copy_parts_device for CRC-64/ECMA (uint64 seeds / out; parts_work_bytes(..., crc64=True))."""
    _check(lib().photon_crc64ecma_copy_parts_n(_ptr(src_iov), _ptr(dst_ptrs), nparts, max_part_bytes,
                                               seed & 0xFFFFFFFFFFFFFFFF, _ptr(seeds), _ptr(out), _ptr(work),
                                               _work_bytes(work, work_bytes), _stream(stream)))


def batch_parts_device(iov, nparts, max_part_bytes, out, work, work_bytes=None, seed=0, seeds=None, stream=None):
    """copy_parts_device without the copy: out[i] = crc32c_extend(iov[i].base, n_i, seed_i), every part
    cut over the chip. Async, capturable."""
    _check(lib().photon_crc32c_batch_parts_n(_ptr(iov), nparts, max_part_bytes, seed & 0xFFFFFFFF, _ptr(seeds),
                                             _ptr(out), _ptr(work), _work_bytes(work, work_bytes),
                                             _stream(stream)))


def batch_parts64_device(iov, nparts, max_part_bytes, out, work, work_bytes=None, seed=0, seeds=None, stream=None):
    """batch_parts_device for CRC-64/ECMA (uint64 seeds / out)."""
    _check(lib().photon_crc64ecma_batch_parts_n(_ptr(iov), nparts, max_part_bytes, seed & 0xFFFFFFFFFFFFFFFF,
                                                _ptr(seeds), _ptr(out), _ptr(work), _work_bytes(work, work_bytes),
                                                _stream(stream)))


def parts_packed_work_bytes(nparts, max_total_bytes, crc64=False):
    """Bytes of workspace copy_parts*_packed_device / batch_parts*_packed_device need for nparts parts of at
    most max_total_bytes bytes in all under the current piece setting (set_parts_piece)."""
    return lib().photon_crc_parts_packed_work_bytes(nparts, max_total_bytes, int(bool(crc64)))


def copy_parts_packed_device(src_iov, dst_ptrs, nparts, max_part_bytes, max_total_bytes, out, report, work,
                             work_bytes=None, seed=0, seeds=None, stream=None):
    """copy_parts_device for parts of mixed sizes: the piece tasks are packed on the device, so the work and
    the workspace follow the SUM of the lengths (max_total_bytes, the host's bound on it) and max_part_bytes
    may be ~0. report: 4 uint64 on the device, {overflow, tasks, bytes, piece slots}; with report[0] == 1
    (the parts were longer in sum than max_total_bytes allowed for) nothing else was written. work: device
    workspace of at least parts_packed_work_bytes(nparts, max_total_bytes) bytes. Async, capturable."""
    _check(lib().photon_crc32c_copy_parts_packed_n(_ptr(src_iov), _ptr(dst_ptrs), nparts, max_part_bytes,
                                                   max_total_bytes, seed & 0xFFFFFFFF, _ptr(seeds), _ptr(out),
                                                   _ptr(report), _ptr(work), _work_bytes(work, work_bytes),
                                                   _stream(stream)))


def copy_parts64_packed_device(src_iov, dst_ptrs, nparts, max_part_bytes, max_total_bytes, out, report, work,
                               work_bytes=None, seed=0, seeds=None, stream=None):
    """copy_parts_packed_device for CRC-64/ECMA (uint64 seeds / out; parts_packed_work_bytes(..., crc64=True))."""
    _check(lib().photon_crc64ecma_copy_parts_packed_n(_ptr(src_iov), _ptr(dst_ptrs), nparts, max_part_bytes,
                                                      max_total_bytes, seed & 0xFFFFFFFFFFFFFFFF, _ptr(seeds),
                                                      _ptr(out), _ptr(report), _ptr(work),
                                                      _work_bytes(work, work_bytes), _stream(stream)))


def batch_parts_packed_device(iov, nparts, max_part_bytes, max_total_bytes, out, report, work, work_bytes=None,
                              seed=0, seeds=None, stream=None):
    """copy_parts_packed_device without the copy. Async, capturable."""
    _check(lib().photon_crc32c_batch_parts_packed_n(_ptr(iov), nparts, max_part_bytes, max_total_bytes,
                                                    seed & 0xFFFFFFFF, _ptr(seeds), _ptr(out), _ptr(report),
                                                    _ptr(work), _work_bytes(work, work_bytes), _stream(stream)))


def batch_parts64_packed_device(iov, nparts, max_part_bytes, max_total_bytes, out, report, work, work_bytes=None,
                                seed=0, seeds=None, stream=None):
    """batch_parts_packed_device for CRC-64/ECMA (uint64 seeds / out)."""
    _check(lib().photon_crc64ecma_batch_parts_packed_n(_ptr(iov), nparts, max_part_bytes, max_total_bytes,
                                                       seed & 0xFFFFFFFFFFFFFFFF, _ptr(seeds), _ptr(out),
                                                       _ptr(report), _ptr(work), _work_bytes(work, work_bytes),
                                                       _stream(stream)))


def series64_device(buffer, part_size, n_parts, out, stream=None):
    """out[i] = crc64ecma(buffer + i*part_size, part_size, 0) over device memory (uint64 out). Async."""
    _check(lib().photon_crc64ecma_series_device(_ptr(buffer), part_size, n_parts, _ptr(out), _stream(stream)))


def combine_series64_device(crcs, part_size, n_parts, result, stream=None):
    """*result = crc64ecma_combine_series(crcs, part_size, n_parts) on the device (uint64). Async."""
    _check(lib().photon_crc64ecma_combine_series_device(_ptr(crcs), part_size, n_parts, _ptr(result),
                                                        _stream(stream)))


def fold_parts_device(crcs, lens, obj_start, nobj, nparts, out, seed=0, seeds=None, total=None, stream=None):
    """Fold part CRC-32Cs into object CRCs on the device: object m is the parts
    obj_start[m]..obj_start[m+1]-1 (obj_start None: one object of all nparts), out[m] = the
    fold acc = acc * x^(8 lens[s]) ^ crcs[s] from seeds[m] or seed; lens are uint64 byte
    counts; total (optional, uint64) = the objects' byte lengths. Async, capturable."""
    _check(lib().photon_crc32c_fold_parts_n(_ptr(crcs), _ptr(lens), _ptr(obj_start), nobj, nparts,
                                            seed & 0xFFFFFFFF, _ptr(seeds), _ptr(out), _ptr(total),
                                            _stream(stream)))


def fold_parts64_device(crcs, lens, obj_start, nobj, nparts, out, seed=0, seeds=None, total=None, stream=None):
    """fold_parts_device for CRC-64/ECMA (uint64 crcs / seeds / out). Async, capturable."""
    _check(lib().photon_crc64ecma_fold_parts_n(_ptr(crcs), _ptr(lens), _ptr(obj_start), nobj, nparts,
                                               seed & 0xFFFFFFFFFFFFFFFF, _ptr(seeds), _ptr(out), _ptr(total),
                                               _stream(stream)))


def overwrite_batch_strided(src, src_stride, dst, dst_stride, nbytes, count, delta, stream=None):
    """Overwrite + CRC-32C delta: dst + i*dst_stride receives the nbytes at src + i*src_stride,
    and delta[i] (uint32) = crc32c_extend(old xor new, 0) = the XOR of the range's old and new
    CRC from any common seed; neither range is read a second time. Destinations must not
    overlap each other or a source. Async, capturable."""
    _check(lib().photon_crc32c_overwrite_batch_strided(_ptr(src), src_stride, _ptr(dst), dst_stride, nbytes, count,
                                                       _ptr(delta), _stream(stream)))


def overwrite_batch_iov(src_iov, dst_ptrs, count, delta, stream=None):
    """overwrite_batch_strided over descriptors: dst_ptrs[i] (a device array of pointers)
    receives src_iov[i].len bytes from src_iov[i].base. Async, capturable."""
    _check(lib().photon_crc32c_overwrite_batch_iov(_ptr(src_iov), _ptr(dst_ptrs), count, _ptr(delta),
                                                   _stream(stream)))


def overwrite_batch64_strided(src, src_stride, dst, dst_stride, nbytes, count, delta, stream=None):
    """overwrite_batch_strided for CRC-64/ECMA: delta[i] (uint64) = crc64ecma(old) ^ crc64ecma(new)
    from any common seed. Async, capturable."""
    _check(lib().photon_crc64ecma_overwrite_batch_strided(_ptr(src), src_stride, _ptr(dst), dst_stride, nbytes,
                                                          count, _ptr(delta), _stream(stream)))


def overwrite_batch64_iov(src_iov, dst_ptrs, count, delta, stream=None):
    """overwrite_batch_iov for CRC-64/ECMA (uint64 deltas). Async, capturable."""
    _check(lib().photon_crc64ecma_overwrite_batch_iov(_ptr(src_iov), _ptr(dst_ptrs), count, _ptr(delta),
                                                      _stream(stream)))


def patch_device(delta, tail, nwrites, tgt_start, ntgt, crc_in, crc_out, stream=None):
    """Patch stored CRC-32Cs by the deltas of overwrites: crc_out[t] = crc_in[t] ^ XOR over the
    writes tgt_start[t]..tgt_start[t+1]-1 of delta[i] * x^(8 tail[i]); tail[i] (uint64) = the
    bytes of target t behind the end of write i. tgt_start None: write i patches word i
    (ntgt == nwrites). crc_out may be crc_in. Async, capturable."""
    _check(lib().photon_crc32c_patch_n(_ptr(delta), _ptr(tail), nwrites, _ptr(tgt_start), ntgt, _ptr(crc_in),
                                       _ptr(crc_out), _stream(stream)))


def patch64_device(delta, tail, nwrites, tgt_start, ntgt, crc_in, crc_out, stream=None):
    """patch_device for CRC-64/ECMA (uint64 delta / crc_in / crc_out). Async, capturable."""
    _check(lib().photon_crc64ecma_patch_n(_ptr(delta), _ptr(tail), nwrites, _ptr(tgt_start), ntgt, _ptr(crc_in),
                                          _ptr(crc_out), _stream(stream)))


def xor_batch_strided(src, stripe_stride, block_stride, k, dst, dst_stride, nbytes, count, out, seed=0, seeds=None,
                      stream=None):
    """Stripe parity + CRC-32C in one read: dst + s*dst_stride receives the byte-wise XOR of the k
    blocks src + s*stripe_stride + i*block_stride (nbytes each), and out[s] (uint32) =
    crc32c_extend(parity, nbytes, seed_s). 1 <= k <= 64. A parity may coincide exactly with one
    source of its own stripe (P ^= D). Async, capturable."""
    _check(lib().photon_crc32c_xor_batch_strided(_ptr(src), stripe_stride, block_stride, k, _ptr(dst), dst_stride,
                                                 nbytes, count, seed, _ptr(seeds), _ptr(out), _stream(stream)))


def xor_batch_ptr(src_ptrs, k, dst_iov, count, out, seed=0, seeds=None, stream=None):
    """xor_batch_strided over pointers: stripe s XORs the blocks at src_ptrs[s*k .. s*k+k-1] (a
    device array of pointers; a null pointer is an all-zero block that is not read) into
    dst_iov[s].base, dst_iov[s].len bytes each. A rebuild is the same call with the survivors and
    the parity as sources. Async, capturable."""
    _check(lib().photon_crc32c_xor_batch_ptr(_ptr(src_ptrs), k, _ptr(dst_iov), count, seed, _ptr(seeds), _ptr(out),
                                             _stream(stream)))


def xor_batch64_strided(src, stripe_stride, block_stride, k, dst, dst_stride, nbytes, count, out, seed=0, seeds=None,
                        stream=None):
    """xor_batch_strided for CRC-64/ECMA (uint64 seeds / out). Async, capturable."""
    _check(lib().photon_crc64ecma_xor_batch_strided(_ptr(src), stripe_stride, block_stride, k, _ptr(dst), dst_stride,
                                                    nbytes, count, seed, _ptr(seeds), _ptr(out), _stream(stream)))


def xor_batch64_ptr(src_ptrs, k, dst_iov, count, out, seed=0, seeds=None, stream=None):
    """xor_batch_ptr for CRC-64/ECMA (uint64 seeds / out). Async, capturable."""
    _check(lib().photon_crc64ecma_xor_batch_ptr(_ptr(src_ptrs), k, _ptr(dst_iov), count, seed, _ptr(seeds), _ptr(out),
                                                _stream(stream)))


def xor_expect_device(crcs, ncrc, grp_start, k, lens, nbytes, count, want, seed=0, stream=None):
    """The CRC-32C a stripe's XOR parity must have, from the stored CRCs of its blocks alone:
    want[s] = XOR of crcs[grp_start[s] .. grp_start[s+1]-1] (grp_start None: k words per stripe)
    ^ (group size even ? crc32c_extend(n_s zero bytes, seed) : 0), n_s = lens[s] (uint64) or
    nbytes when lens is None. Compare with xor_batch_*'s out through verify_device. Async,
    capturable."""
    _check(lib().photon_crc32c_xor_expect_n(_ptr(crcs), ncrc, _ptr(grp_start), k, _ptr(lens), nbytes, count, seed,
                                            _ptr(want), _stream(stream)))


def xor_expect64_device(crcs, ncrc, grp_start, k, lens, nbytes, count, want, seed=0, stream=None):
    """xor_expect_device for CRC-64/ECMA (uint64 crcs / seed / want). Async, capturable."""
    _check(lib().photon_crc64ecma_xor_expect_n(_ptr(crcs), ncrc, _ptr(grp_start), k, _ptr(lens), nbytes, count, seed,
                                               _ptr(want), _stream(stream)))


def scan_work_bytes(nparts):
    """Bytes of workspace scan_parts*_device needs for `nparts` parts under the current tile (set_scan_tile)."""
    return lib().photon_crc_scan_work_bytes(nparts)


def set_scan_tile(entries):
    """Tile of the scan calls: 0 = the default (1,024), else a power of two from 64 to 65,536 (tuning.h)."""
    _check(lib().photon_crc_set_scan_tile(entries))


def scan_parts_device(crcs, lens, obj_start, nobj, nparts, run, work, work_bytes=None, seed=0, seeds=None, end=None,
                      stream=None):
    """The running CRC-32Cs of objects over their parts, on the device: inputs as fold_parts_device;
    run[s] (uint32) = the fold of the object's parts up to and including s from seeds[m] or seed, end[s]
    (optional, uint64) = the object's bytes through part s. The last entry of an object is what
    fold_parts_device gives; an empty object writes nothing. work: device workspace of at least
    scan_work_bytes(nparts) bytes (work_bytes, or the tensor's size). Async, capturable."""
    _check(lib().photon_crc32c_scan_parts_n(_ptr(crcs), _ptr(lens), _ptr(obj_start), nobj, nparts,
                                            seed & 0xFFFFFFFF, _ptr(seeds), _ptr(run), _ptr(end), _ptr(work),
                                            _work_bytes(work, work_bytes), _stream(stream)))


def scan_parts64_device(crcs, lens, obj_start, nobj, nparts, run, work, work_bytes=None, seed=0, seeds=None,
                        end=None, stream=None):
    """scan_parts_device for CRC-64/ECMA (uint64 crcs / seeds / run). Async, capturable."""
    _check(lib().photon_crc64ecma_scan_parts_n(_ptr(crcs), _ptr(lens), _ptr(obj_start), nobj, nparts,
                                               seed & 0xFFFFFFFFFFFFFFFF, _ptr(seeds), _ptr(run), _ptr(end),
                                               _ptr(work), _work_bytes(work, work_bytes), _stream(stream)))


class VerifyReport(ctypes.Structure):
    """photon_crc_verify_report (include/photon_crc/crc32c_gpu.h)."""
    _fields_ = [("nbad", ctypes.c_uint64), ("first_bad", ctypes.c_uint64), ("nlisted", ctypes.c_uint64),
                ("count", ctypes.c_uint64)]


def verify_work_bytes(count):
    """Bytes of workspace verify*_device needs for `count` entries under the current tile (set_verify_tile)."""
    return lib().photon_crc_verify_work_bytes(count)


def set_verify_tile(entries):
    """Tile of the verify calls: 0 = the default (1,024), else a power of two from 64 to 65,536 (tuning.h)."""
    _check(lib().photon_crc_set_verify_tile(entries))


def verify_device(crcs, expected, expected_stride, count, report, bad_idx, bad_cap, work, work_bytes=None,
                  stream=None):
    """Check `count` computed CRC-32C words (uint32, device) against stored ones on the device: entry i is
    bad when crcs[i] differs from the little-endian word at expected + i*expected_stride (any address, any
    stride >= 4). report: a VerifyReport's four uint64 words (device or pinned host memory): nbad, first_bad
    (~0 if none), nlisted, count; bad_idx[0:nlisted] (uint64) = the bad indices in ascending order, nlisted =
    min(nbad, bad_cap); bad_idx may be None with bad_cap 0. work: device workspace of at least
    verify_work_bytes(count) bytes (work_bytes, or the tensor's size). Async, capturable."""
    _check(lib().photon_crc32c_verify_n(_ptr(crcs), _ptr(expected), expected_stride, count, _ptr(report),
                                        _ptr(bad_idx), bad_cap, _ptr(work), _work_bytes(work, work_bytes),
                                        _stream(stream)))


def verify64_device(crcs, expected, expected_stride, count, report, bad_idx, bad_cap, work, work_bytes=None,
                    stream=None):
    """verify_device for CRC-64/ECMA (uint64 words, any stride >= 8)."""
    _check(lib().photon_crc64ecma_verify_n(_ptr(crcs), _ptr(expected), expected_stride, count, _ptr(report),
                                           _ptr(bad_idx), bad_cap, _ptr(work), _work_bytes(work, work_bytes),
                                           _stream(stream)))


def verify_ptr_device(crcs, expected_ptrs, count, report, bad_idx, bad_cap, work, work_bytes=None, stream=None):
    """verify_device with entry i's expected word at expected_ptrs[i] (a device array of pointers, any
    alignment); a null pointer means the entry is not compared: neither bad nor in report.count."""
    _check(lib().photon_crc32c_verify_ptr_n(_ptr(crcs), _ptr(expected_ptrs), count, _ptr(report), _ptr(bad_idx),
                                            bad_cap, _ptr(work), _work_bytes(work, work_bytes), _stream(stream)))


def verify64_ptr_device(crcs, expected_ptrs, count, report, bad_idx, bad_cap, work, work_bytes=None, stream=None):
    """verify_ptr_device for CRC-64/ECMA (uint64 words)."""
    _check(lib().photon_crc64ecma_verify_ptr_n(_ptr(crcs), _ptr(expected_ptrs), count, _ptr(report),
                                               _ptr(bad_idx), bad_cap, _ptr(work), _work_bytes(work, work_bytes),
                                               _stream(stream)))


def stamp_device(crcs, count, dst, dst_stride, stream=None):
    """Write CRC-32C word i little-endian at dst + i*dst_stride, any alignment, exactly 4 bytes each (the
    trailer behind each payload of a strided batch). Async, capturable."""
    _check(lib().photon_crc32c_stamp_n(_ptr(crcs), count, _ptr(dst), dst_stride, _stream(stream)))


def stamp64_device(crcs, count, dst, dst_stride, stream=None):
    """stamp_device for CRC-64/ECMA (uint64 words, 8 bytes each)."""
    _check(lib().photon_crc64ecma_stamp_n(_ptr(crcs), count, _ptr(dst), dst_stride, _stream(stream)))


def stamp_ptr_device(crcs, count, dst_ptrs, stream=None):
    """stamp_device with word i written at dst_ptrs[i] (a device array of pointers; null skips the entry)."""
    _check(lib().photon_crc32c_stamp_ptr_n(_ptr(crcs), count, _ptr(dst_ptrs), _stream(stream)))


def stamp64_ptr_device(crcs, count, dst_ptrs, stream=None):
    """stamp_ptr_device for CRC-64/ECMA (uint64 words)."""
    _check(lib().photon_crc64ecma_stamp_ptr_n(_ptr(crcs), count, _ptr(dst_ptrs), _stream(stream)))


class Span(ctypes.Structure):
    """photon_crc_span (include/photon_crc/crc32c_gpu.h)."""
    _fields_ = [("device", ctypes.c_int), ("d_data", ctypes.c_void_p), ("nbytes", ctypes.c_uint64)]


def _spans(spans):
    arr = (Span * max(1, len(spans)))()
    for a, (dev, ptr, n) in zip(arr, spans):
        a.device, a.d_data, a.nbytes = dev, _ptr(ptr), n
    return arr


def extend_spans(spans, seed=0):
    """crc32c_extend over ONE buffer whose bytes lie on several devices:
    spans = [(device, device_pointer, nbytes), ...] in buffer order. Synchronous."""
    res = ctypes.c_uint32(0)
    _check(lib().photon_crc32c_extend_spans(_spans(spans), len(spans), seed & 0xFFFFFFFF, ctypes.byref(res)))
    return res.value


def extend64_spans(spans, seed=0):
    """crc64ecma_extend over ONE buffer spanning devices (see extend_spans). Synchronous."""
    res = ctypes.c_uint64(0)
    _check(lib().photon_crc64ecma_extend_spans(_spans(spans), len(spans), seed & 0xFFFFFFFFFFFFFFFF,
                                               ctypes.byref(res)))
    return res.value


def set_device_dispatch(on):
    """Route crc32c_auto / crc32c_series_auto / crc32c_combine_series_auto and
    crc64ecma_auto / crc64ecma_series_auto / crc64ecma_combine_series_auto to the
    device for device pointers (photon_crc_set_device_dispatch). Raises
    CrcError(-EIO) if a routed call failed on the device since the last switch
    (it was recomputed on the host: dispatch_fallbacks())."""
    _check(lib().photon_crc_set_device_dispatch(1 if on else 0))


def dispatch_fallbacks():
    """Routed calls whose device work failed and were recomputed on the host."""
    return int(lib().photon_crc_dispatch_fallbacks())


def lanes_for(nbytes):
    """Lanes per buffer the engine picks for buffers of nbytes (tuning.h)."""
    return int(lib().photon_crc_lanes_for(nbytes))


def inject_failures(n):
    """tuning.h failure injection: the next n device entry points called on
    this thread return -EIO before enqueuing anything."""
    lib().photon_crc_test_fail_next(n)


_CRC_PTR_FN = ctypes.CFUNCTYPE(ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32)
_SERIES_PTR_FN = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p)
_CSER_PTR_FN = ctypes.CFUNCTYPE(ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32)


def crc32c_extend_at(addr, nbytes, crc=0):
    """crc32c_extend through the crc32c_auto pointer on a raw address (what a
    C++ caller holding a device pointer would call)."""
    return _auto("crc32c_auto", _CRC_PTR_FN)(addr, nbytes, crc & 0xFFFFFFFF)


_CRC64_PTR_FN = ctypes.CFUNCTYPE(ctypes.c_uint64, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint64)


def crc64ecma_extend_at(addr, nbytes, crc=0):
    """crc64ecma_extend through the crc64ecma_auto pointer on a raw address."""
    return _auto("crc64ecma_auto", _CRC64_PTR_FN)(addr, nbytes, crc & 0xFFFFFFFFFFFFFFFF)


def crc32c_series_at(addr, part_size, n_parts, out_addr):
    """crc32c_series through crc32c_series_auto on raw addresses."""
    _auto("crc32c_series_auto", _SERIES_PTR_FN)(addr, part_size, n_parts, out_addr)


def crc32c_combine_series_at(addr, part_size, n_parts):
    """crc32c_combine_series through crc32c_combine_series_auto on a raw address."""
    return _auto("crc32c_combine_series_auto", _CSER_PTR_FN)(addr, part_size, n_parts)


_SERIES64_PTR_FN = _SERIES_PTR_FN
_CSER64_PTR_FN = ctypes.CFUNCTYPE(ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32)


def crc64ecma_series_at(addr, part_size, n_parts, out_addr):
    """crc64ecma_series through crc64ecma_series_auto on raw addresses."""
    _auto("crc64ecma_series_auto", _SERIES64_PTR_FN)(addr, part_size, n_parts, out_addr)


def crc64ecma_combine_series_at(addr, part_size, n_parts):
    """crc64ecma_combine_series through crc64ecma_combine_series_auto on a raw address."""
    return _auto("crc64ecma_combine_series_auto", _CSER64_PTR_FN)(addr, part_size, n_parts)


def host_register(addr, nbytes):
    """Make host memory [addr, addr+nbytes) device-readable in place."""
    _check(lib().photon_crc_host_register(addr, nbytes))


def host_unregister(addr):
    _check(lib().photon_crc_host_unregister(addr))


def file_strided(fd, offset, stride, nbytes, count, seed=0):
    """CRC32C of `count` records of `nbytes` at offset + i*stride of file descriptor fd
    (pread into pinned chunks + GPU pipeline). Returns a list of ints."""
    out = (ctypes.c_uint32 * max(count, 1))()
    _check(lib().photon_crc32c_file_strided(fd, offset, stride, nbytes, count, seed & 0xFFFFFFFF, out))
    return list(out)[:count]


def set_generic_rows(u):
    """Batch kernel variant: -1 (default) = by lane-group size; 2, 4, 8 = rows
    per step of the generic kernel."""
    _check(lib().photon_crc_set_generic_rows(u))


def set_msg_mode(mode):
    """Message batches: 0 automatic, 1 one fused kernel, 2 segment + fold kernels."""
    _check(lib().photon_crc_set_msg_mode(mode))


def set_long_shape(lanes=0, rounds=0):
    """One long buffer (extend_device / extend64_device): lanes per chunk (0 =
    automatic, 32, 64) and chunks per lane group of the grid (0 = automatic)."""
    _check(lib().photon_crc_set_long_shape(lanes, rounds))


def set_routed_wait(spin_us=40, sleep_ahead=True):
    """Routed drop-in calls: tag-polling window in µs, then a blocking wait;
    sleep_ahead: long calls sleep through their expected time first (tuning)."""
    _check(lib().photon_crc_set_routed_wait(spin_us, 1 if sleep_ahead else 0))


def set_mid_kernel(on=True):
    """Spans over 256 KiB up to 16 MiB: the mid layout (default) or, off, the
    long kernel (tuning; tests of the long kernel's plan)."""
    _check(lib().photon_crc_set_mid_kernel(1 if on else 0))


SMALL_PLAN_FIELDS = ("layout", "nb", "s0", "eoff", "k", "rows", "grid", "wg0", "fits_service",
                     "small_v", "small_wg", "mid_v", "mid_wg", "small_blocks", "mid_blocks",
                     "small_rows", "mid_rows", "svc_max_blocks", "seed_bytes")


def small_plan(addr, nbytes, crc64=False):
    """photon_crc_test_small_plan (tuning.h) as a dict of SMALL_PLAN_FIELDS: the one-buffer
    layout (0 small, 1 mid, 2 the long kernel) and geometry the launch paths would take for
    nbytes at address addr (not dereferenced), and the layout constants (tests)."""
    out = (ctypes.c_uint64 * len(SMALL_PLAN_FIELDS))()
    k = lib().photon_crc_test_small_plan(addr, nbytes, 1 if crc64 else 0, out, len(out))
    _check(k if k < 0 else 0)
    assert k == len(SMALL_PLAN_FIELDS), k
    return dict(zip(SMALL_PLAN_FIELDS, (int(x) for x in out)))


def set_small_service(idle_us):
    """Routed small crc32c_extend / crc64ecma_extend calls through a resident
    service launch that ends after idle_us without a call; 0 = off, a launch
    per call; default 200 or PHOTON_CRC_SMALL_SERVICE (tuning)."""
    _check(lib().photon_crc_set_small_service(int(idle_us)))


def set_small_service_life(life_us):
    """Life of one service launch (default 2000 us): the bound on how long a
    device-wide wait stalls behind it under steady routed traffic (tuning)."""
    _check(lib().photon_crc_set_small_service_life(int(life_us)))


def set_service_doorbell(bar):
    """The service's doorbell: True = device memory through the PCIe BAR (the
    default, when the host mapping was verified), False = pinned host memory.
    Ends running launches (tuning)."""
    _check(lib().photon_crc_set_service_doorbell(1 if bar else 0))


def small_service_doorbell(kind=0):
    """'bar' or 'pinned': the doorbell the current device's service of `kind`
    (0 CRC-32C, 1 CRC-64) rings; None if that service was never started."""
    r = lib().photon_crc_small_service_doorbell(int(kind))
    if r == -2:  # -ENOENT
        return None
    _check(r if r < 0 else 0)
    return "bar" if r == 1 else "pinned"


def small_service_deferred():
    """Routed small calls that took the launch path because a batch / long
    launch of the library was in flight when they would have started a
    service launch (tests)."""
    return int(lib().photon_crc_small_service_deferred())


def small_service_stats():
    """(served, starts, missed): routed small calls the service served, its
    launches, calls that found it ending (tests)."""
    import ctypes
    v = [ctypes.c_uint64(0) for _ in range(3)]
    _check(lib().photon_crc_small_service_stats(*[ctypes.byref(x) for x in v]))
    return tuple(x.value for x in v)


def set_full_rows64(mode, rows_per_step=2):
    """CRC-64 whole-step uniform batches: 0 generic kernel, 1 full-row kernel,
    2 full-row kernel with cross-buffer prefetch, 3 automatic (the default:
    2 for buffers up to 8 KiB) (tuning)."""
    _check(lib().photon_crc64_set_full_rows(mode, rows_per_step))


def set_msg_rows(u):
    """Rows per step of the one-kernel message form (2 or 4; tuning)."""
    _check(lib().photon_crc_set_msg_rows(u))


def read_stream(base, nbytes, sink, sink_words, stream=None):
    """Bench utility: HBM read-only stream over nbytes (achievable-roofline probe)."""
    _check(lib().photon_crc_util_read_stream(_ptr(base), nbytes, _ptr(sink), sink_words, _stream(stream)))


def fill_splitmix(base, stride, nbytes, count, seed_base, stream=None):
    """Test/bench utility: device buffers = photonlibos_amd.datagen streams."""
    _check(lib().photon_crc_util_fill_splitmix(_ptr(base), stride, nbytes, count, seed_base, _stream(stream)))


def scratch_release():
    """Free the device scratch buffers the library keeps idle (bytes freed)."""
    return int(lib().photon_crc_scratch_release())
