"""The two host-side pipelines where their buffers are reused:
photon_crc32c_host_batch_strided / photon_crc64ecma_host_batch_strided with the
staging span set to 1 MiB (photon_crc_set_host_stage_bytes), so that a few MiB
run through up to 13 chunks and every staging slot is reused, and
photon_crc32c_file_strided with the chunk span set to 256 KiB (parallel reads)
and 64 KiB (serial reads), so that a 3 MiB file runs through many chunks and
both chunk buffers are reused. Every host area and the file hold one
non-repeating stream, so bytes of any other chunk give another CRC, and EVERY
buffer / record is compared with the oracle's C loops. Bit-exact."""
import os
import threading

import numpy as np
import pytest

from photonlibos_amd import checksum as ck
from photonlibos_amd import datagen
from photonlibos_amd.checksum import CrcError

pytestmark = pytest.mark.gpu

MIB = 1 << 20
SEED32, SEED64 = 0x9E3779B1, 0xFEDCBA9876543210


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available()
    assert ck.device_count() >= 1
    return torch


@pytest.fixture()
def stage_span():
    yield ck.set_host_stage_bytes
    ck.set_host_stage_bytes(0)


@pytest.fixture()
def file_chunk():
    yield ck.set_file_chunk_bytes
    ck.set_file_chunk_bytes(0)


def stage_chunks(nbytes, count, span):
    pitch = (nbytes + 255) // 256 * 256
    per = max(1, span // pitch)
    return -(-count // per)


_areas = {}


def host_area(torch, stream, nbytes, stride, count):
    """A pinned area of `count` buffers filled with ONE stream over its whole length, and its numpy view."""
    key = (stream, nbytes, stride, count)
    if key not in _areas:
        t = torch.empty(stride * count, dtype=torch.uint8, pin_memory=True)
        t.numpy()[:] = datagen.stream_bytes(stream, stride * count)
        _areas[key] = t
    return _areas[key], _areas[key].numpy()


def seeds_of(width, count):
    k = np.arange(1, count + 1, dtype=np.uint64)
    with np.errstate(over="ignore"):
        s = k * np.uint64(0x9E3779B97F4A7C15)
    return s.astype(np.uint32) if width == 32 else s


def run_host(torch, width, host, stride, nbytes, count, mode, multi_ndev=None):
    """One host-pipeline call; returns (got, seeds or None, seed0) as unsigned numpy words."""
    u, i = (np.uint32, np.int32) if width == 32 else (np.uint64, np.int64)
    out = torch.from_numpy(np.full(count, 0x5A, i)).pin_memory()
    seeds = seed0 = None
    kw = {}
    if mode == "seeds":
        seeds = seeds_of(width, count)
        kw["seeds"] = torch.from_numpy(seeds.view(i).copy()).pin_memory()
    elif mode == "seed0":
        seed0 = SEED32 if width == 32 else SEED64
        kw["seed"] = seed0
    if multi_ndev is not None:
        assert width == 32
        ck.host_batch_strided_multi(host, stride, nbytes, count, out, ndev=multi_ndev, **kw)
    else:
        (ck.host_batch_strided if width == 32 else ck.host_batch64_strided)(host, stride, nbytes, count, out, **kw)
    return out.numpy().view(u).copy(), seeds, seed0


def expected(oracle, width, h, stride, nbytes, count, seeds, seed0):
    """Every buffer's CRC: the strided C loop, or with per-buffer seeds the per-record oracle over all indices."""
    if seeds is None:
        f = oracle.crc32c_strided if width == 32 else oracle.crc64ecma_strided
        return f(h, stride, nbytes, count, seed0 or 0)
    one = oracle.crc32c if width == 32 else oracle.crc64ecma
    return np.array([one(h[k * stride:k * stride + nbytes], int(seeds[k])) for k in range(count)],
                    np.uint32 if width == 32 else np.uint64)


def check_host(torch, oracle, width, stream, nbytes, stride, count, mode, **kw):
    host, h = host_area(torch, stream, nbytes, stride, count)
    got, seeds, seed0 = run_host(torch, width, host, stride, nbytes, count, mode, **kw)
    want = expected(oracle, width, h, stride, nbytes, count, seeds, seed0)
    wrong = np.flatnonzero(got != want)
    assert wrong.size == 0, (wrong.size, wrong[:8].tolist())


# (nbytes, stride, count, chunks at a 1 MiB span)
SHAPES = [
    (65544, 65560, 15 * 7 + 1, 8),   # every slot reused twice, the last chunk has one buffer
    (65544, 65560, 15 * 3, 3),       # exactly three full chunks, no reuse
    (65544, 65560, 15 * 3 + 1, 4),   # the first reuse
    (4104, 4104, 3000, 13),          # many small rows per chunk, packed
    (600000, 600064, 7, 7),          # one buffer per chunk
    (1, 16, 5000, 2),                # chunks of tiny rows
]


@pytest.mark.parametrize("mode", ["seeds", "seed0", "none"])
@pytest.mark.parametrize("width", [32, 64])
@pytest.mark.parametrize("nbytes,stride,count,chunks", SHAPES)
def test_host_pipeline_small_span(torch_dev, oracle, stage_span, nbytes, stride, count, chunks, width, mode):
    assert stage_chunks(nbytes, count, MIB) == chunks
    stage_span(MIB)
    check_host(torch_dev, oracle, width, 0x57A6E, nbytes, stride, count, mode)


@pytest.mark.parametrize("mode", ["seeds", "seed0", "none"])
@pytest.mark.parametrize("width", [32, 64])
def test_host_pipeline_pitch_above_span(torch_dev, oracle, stage_span, width, mode):
    """A 64 KiB span under buffers of 100,000 bytes: buffers per chunk clamps to 1, ten chunks."""
    assert stage_chunks(100000, 10, 64 << 10) == 10
    stage_span(64 << 10)
    check_host(torch_dev, oracle, width, 0xC1A3, 100000, 100016, 10, mode)


@pytest.mark.parametrize("width", [32, 64])
def test_host_pipeline_back_to_back(torch_dev, oracle, stage_span, width):
    """The same shape twice with other bytes: the slots and the result array hold the previous call's data."""
    stage_span(MIB)
    nbytes, stride, count, _ = SHAPES[0]
    for stream in (0xB2B1, 0xB2B2, 0xB2B1):
        check_host(torch_dev, oracle, width, stream, nbytes, stride, count, "seeds")


def test_host_pipeline_widths_alternate(torch_dev, oracle, stage_span):
    """CRC-32C and CRC-64 calls share the pipeline's result and seed arrays: 32, 64, 32 at a growing count (each
    beyond what any earlier call of the suite left, so the arrays are grown again), then a smaller CRC-64 call."""
    stage_span(MIB)
    for width, count, mode in ((32, 20000, "seed0"), (64, 30000, "none"), (32, 100000, "seed0"), (64, 1000, "seeds"),
                               (32, 1000, "seeds")):
        assert stage_chunks(1, count, MIB) == -(-count // 4096)
        check_host(torch_dev, oracle, width, 0xA17 + count, 1, 16, count, mode)


@pytest.mark.parametrize("ndev", [0, 1])
def test_host_pipeline_multi(torch_dev, oracle, stage_span, ndev):
    stage_span(MIB)
    nbytes, stride, count, _ = SHAPES[0]
    check_host(torch_dev, oracle, 32, 0x57A6E, nbytes, stride, count, "seeds", multi_ndev=ndev)


def test_host_pipeline_two_threads(torch_dev, oracle, stage_span):
    """Two threads on the 8-chunk shape at once (other bytes each): the device's pipeline takes one call at a time,
    both results exact."""
    stage_span(MIB)
    nbytes, stride, count, _ = SHAPES[0]
    areas = [host_area(torch_dev, s, nbytes, stride, count) for s in (0x7A1, 0x7A2)]
    want = [expected(oracle, 32, h, stride, nbytes, count, seeds_of(32, count), None) for _, h in areas]
    for _ in range(3):
        got, errs = [None, None], []

        def run(k):
            try:
                got[k] = run_host(torch_dev, 32, areas[k][0], stride, nbytes, count, "seeds")[0]
            except Exception as e:  # noqa: BLE001
                errs.append(e)
        th = [threading.Thread(target=run, args=(k,)) for k in range(2)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not errs, errs
        for k in range(2):
            assert np.array_equal(got[k], want[k]), (k, np.flatnonzero(got[k] != want[k])[:8].tolist())


# ---------------------------------------------------------------- file records
FILE_BYTES = 3 * MIB + 1234


@pytest.fixture(scope="module")
def data_file(tmp_path_factory):
    blob = datagen.stream_bytes(0xF11E5, FILE_BYTES)
    p = tmp_path_factory.mktemp("src") / "records.bin"
    p.write_bytes(blob.tobytes())
    return str(p), blob


def file_chunks(stride, count, span):
    per = min(max(1, span // stride), count)
    return -(-count // per)


def file_records(path, offset, stride, nbytes, count, seed):
    fd = os.open(path, os.O_RDONLY)
    try:
        return np.array(ck.file_strided(fd, offset, stride, nbytes, count, seed=seed), np.uint32)
    finally:
        os.close(fd)


LAST = FILE_BYTES - (46 * 65552 + 65536)  # 47 records from here end on the file's last byte

# (offset, stride, nbytes, count, chunks at 256 KiB, chunks at 64 KiB)
FILE_SHAPES = [
    (0, 4096, 4096, 768, 12, 48),         # whole chunks
    (777, 65552, 65536, 47, 16, 47),      # records straddle chunk ends
    (5, 300000, 299997, 10, 10, 10),      # the stride is above the chunk span: one record per chunk
    (123, 100, 37, 20000, 8, 31),         # tiny records, many chunks
    (LAST, 65552, 65536, 47, 16, 47),     # the last record ends on the file's last byte
]


@pytest.mark.parametrize("span", [256 << 10, 64 << 10])
@pytest.mark.parametrize("offset,stride,nbytes,count,chunks256,chunks64", FILE_SHAPES)
def test_file_records_small_chunks(torch_dev, oracle, data_file, file_chunk, offset, stride, nbytes, count, chunks256,
                                   chunks64, span):
    path, blob = data_file
    assert offset + (count - 1) * stride + nbytes <= FILE_BYTES
    assert file_chunks(stride, count, span) == (chunks256 if span == 256 << 10 else chunks64)
    file_chunk(span)
    got = file_records(path, offset, stride, nbytes, count, 0x1234)
    want = oracle.crc32c_strided(blob[offset:], stride, nbytes, count, 0x1234)
    wrong = np.flatnonzero(got != want)
    assert wrong.size == 0, (wrong.size, wrong[:8].tolist())


@pytest.mark.parametrize("span", [256 << 10, 64 << 10])
def test_file_end_in_a_later_chunk(torch_dev, data_file, file_chunk, span):
    """The last record one byte past the end of the file: -EIO out of the last of many chunks, while the consumer
    works on earlier ones, and the call returns."""
    path, _ = data_file
    assert file_chunks(65552, 47, span) >= 16
    assert LAST + 1 + 46 * 65552 + 65536 == FILE_BYTES + 1
    file_chunk(span)
    res = []

    def run():
        try:
            file_records(path, LAST + 1, 65552, 65536, 47, 0)
            res.append(None)
        except Exception as e:  # noqa: BLE001
            res.append(e)
    t = threading.Thread(target=run, daemon=True)
    t.start()
    t.join(60)
    assert not t.is_alive(), "file_strided did not return"
    assert isinstance(res[0], CrcError) and res[0].code == -5, res
    assert "end of file before the last record" in str(res[0])


def test_concurrent_file_callers_small_chunks(torch_dev, oracle, data_file, file_chunk):
    """tests/test_gpu_sources.py::test_concurrent_file_callers' shape at a 256 KiB span: 12 and 10 chunks a caller,
    each with its own chunk buffers, over the shared reader pool."""
    path, blob = data_file
    shapes = [(0, 4096, 4096, 768), (4096 * 3 + 1, 65536, 65000, 40)]
    assert [file_chunks(s[1], s[3], 256 << 10) for s in shapes] == [12, 10]
    file_chunk(256 << 10)
    want = [oracle.crc32c_strided(blob[off:], stride, n, cnt, k) for k, (off, stride, n, cnt) in enumerate(shapes)]
    for _ in range(3):
        res, errs = [None, None], []

        def run(k):
            try:
                res[k] = file_records(path, *shapes[k], seed=k)
            except Exception as e:  # noqa: BLE001
                errs.append(e)
        th = [threading.Thread(target=run, args=(k,)) for k in range(2)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not errs, errs
        for k in range(2):
            assert np.array_equal(res[k], want[k]), (k, np.flatnonzero(res[k] != want[k])[:8].tolist())
