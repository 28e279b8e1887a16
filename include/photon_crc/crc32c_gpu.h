/*
 * crc32c_gpu.h -- C-ABI of the MI355X CRC32C engine (libphoton_checksum.so).
 *
 * Plain pointers and sizes only; no HIP or torch types in the signatures
 * (`stream` is a hipStream_t passed as void*, NULL = the default stream).
 *
 * Semantics are PhotonLibOS's raw CRC-32C (common/checksum/crc32c.h:30-45):
 * reflected polynomial 0x82F63B78, init = caller's seed, no final xor.
 *   out[i] = crc32c_extend(buffer_i, nbytes_i, seed_i)
 * Every entry point below replaces a host loop over that reference call:
 *   photon_crc32c_batch_strided  <- loop of crc32c_extend (crc32c.h:30-33) over
 *                                   base + i*stride; with stride == nbytes and
 *                                   seeds == 0 it is crc32c_series
 *                                   (crc32c.h:52-57, crc.cpp:474-509)
 *   photon_crc32c_batch_iov      <- loop of crc32c_extend over struct iovec[]
 *                                   (common/iovector.h:56-230)
 *   photon_crc32c_batch_msg      <- Crc32Hasher::extend_hash over each
 *                                   message's iovector (rpc/serialize.h:239-252):
 *                                   per-segment CRC + crc32c_combine fold
 *                                   (crc.cpp:393-430)
 *   photon_crc32c_combine_batch  <- loop of crc32c_combine (crc32c.h:61-66)
 *
 * All batch calls are asynchronous on `stream`: inputs must stay valid and
 * outputs are ready only after the stream is synchronised. Buffers and
 * descriptor arrays must be device-accessible (hipMalloc'd or registered /
 * pinned host memory).
 *
 * Per device, the library keeps ≈1.3 MiB of constant table images for the
 * life of the process (the LDS tables every batch / long kernel copies
 * instead of building them, written on the device's first call) and, for
 * the small and mid kernels, ≈1.3 MiB more on the first call that needs them.
 *
 * Return value: 0 on success, a negative errno-style code otherwise
 * (-ENODEV no usable gfx950 device, -EINVAL bad arguments, -EIO HIP runtime
 * error; photon_crc_last_error() has the text). There is NO silent CPU
 * fallback: on error nothing is computed.
 */
#ifndef PHOTON_CRC32C_GPU_H
#define PHOTON_CRC32C_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Same layout as struct iovec {void *iov_base; size_t iov_len;}
 * (common/iovector.h:56-230 uses struct iovec); a struct iovec array may be
 * passed directly. */
typedef struct photon_crc_iovec {
    const void* base;
    uint64_t len;
} photon_crc_iovec;

/* Same layout as CRC32C_Component {uint32_t crc; uint32_t size;}
 * (common/checksum/crc32c.h:76-79); a CRC32C_Component array may be passed. */
typedef struct photon_crc_component {
    uint32_t crc;
    uint32_t size;
} photon_crc_component;

/* Number of usable gfx950 devices (>0), or a negative error code. */
int photon_crc_device_count(void);

/* Text of the last error on this thread ("" if none). */
const char* photon_crc_last_error(void);

/* Device scratch the library keeps between calls (segment CRCs of two-kernel
 * message batches, long-buffer state): idle buffers over 64 MiB, and idle
 * scratch beyond 256 MiB per device, are freed automatically; this frees
 * every idle buffer whose last use has completed. Returns the bytes freed. */
int64_t photon_crc_scratch_release(void);

/* (i) Equal-length buffers: buffer i = d_base + i*stride, nbytes each.
 * seed_i = d_seeds ? d_seeds[i] : seed0. d_out[count] receives the CRCs. */
int photon_crc32c_batch_strided(const void* d_base, uint64_t stride, uint64_t nbytes, uint64_t count,
                                uint32_t seed0, const uint32_t* d_seeds, uint32_t* d_out, void* stream);

/* (i-h) Host-memory batch, the path's real source (socket / file buffers in
 * host RAM feeding rpc/ and fs/): chunks of the batch are copied to the
 * device (stream-ordered, 2-D so any stride packs densely) while earlier
 * chunks are checksummed; the CRCs come back to h_out[count]. Synchronous.
 * h_base should be pinned (hipHostMalloc / hipHostRegister) for the copies to
 * overlap; h_seeds (optional) and h_out are host arrays. Buffers up to 256 MiB. */
int photon_crc32c_host_batch_strided(const void* h_base, uint64_t stride, uint64_t nbytes, uint64_t count,
                                     uint32_t seed0, const uint32_t* h_seeds, uint32_t* h_out);

/* (i-h, many GPUs) The same host-memory batch sharded over the first `ndev`
 * gfx950 devices (0 = every device) of THIS process -- Photon runs one
 * process per host, not one per GPU: contiguous slices of the buffer indices,
 * one host thread per device driving that device's pipeline over its own
 * host link, results in h_out[count] exactly as the single-device call.
 * No collective. Synchronous. */
int photon_crc32c_host_batch_strided_multi(const void* h_base, uint64_t stride, uint64_t nbytes, uint64_t count,
                                           uint32_t seed0, const uint32_t* h_seeds, uint32_t* h_out, int ndev);

/* (i-d, many GPUs) Device-resident shards, each on its own device: shard i is
 * photon_crc32c_batch_strided on `device` (pointers of that device, stream of
 * that device or NULL). Enqueues every shard and returns (async); the caller's
 * current device is restored. */
typedef struct photon_crc_shard {
    int device;
    const void* d_base;
    uint64_t stride;
    uint64_t nbytes;
    uint64_t count;
    uint32_t seed0;
    const uint32_t* d_seeds;
    uint32_t* d_out;
    void* stream;
} photon_crc_shard;
int photon_crc32c_batch_strided_shards(const photon_crc_shard* shards, int nshards);

/* (ii) Arbitrary buffers: d_iov[count] (device-resident descriptors); any
 * alignment, any length (0 returns the seed). */
int photon_crc32c_batch_iov(const photon_crc_iovec* d_iov, uint64_t count, uint32_t seed0,
                            const uint32_t* d_seeds, uint32_t* d_out, void* stream);

/* (iii) Scatter-gather messages: message m is segments
 * [d_msg_start[m], d_msg_start[m+1]) of d_iov (d_msg_start has nmsg+1
 * entries, d_msg_start[nmsg] = total segments). d_out[m] = the chained
 * crc32c_extend over the message's segments starting from seed_m.
 * d_seg_out (total segments entries), if non-NULL, receives each segment's
 * own CRC32C (seed 0); with NULL the segments are chained through the seed
 * (the faster form when there are many short messages). */
int photon_crc32c_batch_msg(const photon_crc_iovec* d_iov, const uint64_t* d_msg_start, uint64_t nmsg,
                            uint32_t seed0, const uint32_t* d_seeds, uint32_t* d_seg_out, uint32_t* d_out,
                            void* stream);
/* As photon_crc32c_batch_msg, with the total segment count nseg
 * (== d_msg_start[nmsg]) supplied by the caller: fully asynchronous
 * (photon_crc32c_batch_msg reads it back from the device and waits). */
int photon_crc32c_batch_msg_n(const photon_crc_iovec* d_iov, const uint64_t* d_msg_start, uint64_t nmsg,
                              uint64_t nseg, uint32_t seed0, const uint32_t* d_seeds, uint32_t* d_seg_out,
                              uint32_t* d_out, void* stream);

/* (iv) Copy + CRC-32C in one pass: the payload is landed at a destination
 * and checksummed from the same read (the unfused pair, photon_crc_memcpy_async
 * then a batch, reads every byte twice). Asynchronous on `stream` like the
 * batches above: nothing is allocated or synchronised inside the call, so
 * each can be captured into a graph; 0 or a negative errno; no CPU fallback
 * (without a usable gfx950 device: a negative code).
 *   - Sources are device-accessible memory: HBM, or pinned / registered host
 *     memory, which the kernel reads over the link in place. Destinations
 *     are device-accessible.
 *   - A source and a destination range must not overlap, nor may two
 *     destinations: the caller's responsibility, not checked.
 *   - Bytes outside [dst, dst + len) are never written.
 *   - A zero-length buffer writes nothing and returns the seed.
 *   - Null pointers with a non-zero count give -EINVAL; count == 0 /
 *     nmsg == 0 return 0.
 *   - Any alignment is correct; the payload is read exactly once when source
 *     and destination are co-aligned ((dst - src) % 16 == 0), else the
 *     buffer is copied first and checksummed from the cache.
 *
 * dst buffer i = d_dst_base + i*dst_stride receives the nbytes of src buffer
 * i = src_base + i*src_stride; d_out[i] = crc32c_extend(src_i, nbytes, seed_i). */
int photon_crc32c_copy_batch_strided(const void* src_base, uint64_t src_stride,
                                     void* d_dst_base, uint64_t dst_stride,
                                     uint64_t nbytes, uint64_t count, uint32_t seed0,
                                     const uint32_t* d_seeds, uint32_t* d_out, void* stream);

/* d_dst[i] receives d_src[i].len bytes from d_src[i].base (d_src and d_dst:
 * device-resident arrays of count entries). */
int photon_crc32c_copy_batch_iov(const photon_crc_iovec* d_src, void* const* d_dst,
                                 uint64_t count, uint32_t seed0, const uint32_t* d_seeds,
                                 uint32_t* d_out, void* stream);

/* iovector_view::memcpy_to + Crc32Hasher in one pass: message m's segments
 * are written back to back at d_dst[m]; d_out / d_seg_out exactly as
 * photon_crc32c_batch_msg_n (d_seg_out optional). */
int photon_crc32c_gather_msg_n(const photon_crc_iovec* d_iov, const uint64_t* d_msg_start,
                               uint64_t nmsg, uint64_t nseg, void* const* d_dst,
                               uint32_t seed0, const uint32_t* d_seeds,
                               uint32_t* d_seg_out, uint32_t* d_out, void* stream);

/* iovector_view::memcpy_iov (common/iovector.cpp:301-318) + the checksum in
 * one pass: copy between two iovectors whose segment boundaries are unrelated.
 * Message m has source segments d_src[d_src_start[m] .. d_src_start[m+1]) and
 * destination segments d_dst[d_dst_start[m] .. d_dst_start[m+1]); both start
 * arrays have nmsg + 1 entries, nsrc / ndst are the totals. With size_m =
 * d_size ? d_size[m] : unlimited, k_m = min(size_m, sum of dst lengths, sum of
 * src lengths) bytes are copied, byte j of the source stream to byte j of
 * the destination stream; zero-length segments on either side are skipped
 * (their base may be null). d_out[m] = crc32c_extend over exactly those k_m
 * source bytes from seed_m (the seed when k_m == 0); d_copied[m] = k_m when
 * d_copied is non-NULL. Destination bytes past k_m are not written, source
 * segments past k_m are not read. memcpy_to (one destination segment: the
 * gather above), memcpy_from (scatter: ONE SOURCE SEGMENT per message) and
 * any re-segmentation are special cases.
 * Contract (iv): a null d_src_start, d_dst_start or d_out, a null d_src with
 * nsrc > 0 or a null d_dst with ndst > 0 give -EINVAL. No byte outside a
 * destination segment is written and nothing is read-modify-written, so
 * destination segments may sit back to back at odd addresses. The alignment
 * rule holds per piece (a run of bytes inside one source and one destination
 * segment): a piece with (dst - src) % 16 == 0 is read once, any other is
 * copied first and checksummed from the cache. No per-segment CRCs here (a
 * piece is in general neither a source nor a destination segment); for one
 * CRC per segment of ONE side see photon_crc32c_copy_msg_iov_seg_n below, for
 * the segment CRCs of BOTH sides photon_crc32c_copy_msg_iov_seg2_n. */
int photon_crc32c_copy_msg_iov_n(const photon_crc_iovec* d_src, const uint64_t* d_src_start, uint64_t nsrc,
                                 const photon_crc_iovec* d_dst, const uint64_t* d_dst_start, uint64_t ndst,
                                 uint64_t nmsg, const uint64_t* d_size,
                                 uint32_t seed0, const uint32_t* d_seeds,
                                 uint32_t* d_out, uint64_t* d_copied, void* stream);

/* photon_crc32c_copy_msg_iov_n that also returns one CRC per segment of one
 * side, from the same read. The copy, k_m, d_out[m] (bit-identical) and
 * d_copied[m] are those of the call above, and so are the alignment rule and
 * contract (iv). seg_side chooses the side: PHOTON_CRC_SEG_OF_SRC (d_seg_out
 * has nsrc entries, indexed like d_src: the read direction, blocks that carry
 * a stored CRC each assembled into a caller's iovector) or
 * PHOTON_CRC_SEG_OF_DST (ndst entries, indexed like d_dst: the write
 * direction, a payload scattered into blocks that are stored with a CRC each).
 * d_seg_out[s] = crc32c_extend from seed 0 over the bytes of segment s that
 * took part in the copy: the whole segment where the copy covered it, the
 * copied prefix for the segment in which the copy ended, 0 (the CRC of no
 * bytes) for a zero-length segment and for every segment behind the end of
 * the copy. Every entry of all nmsg messages is written, none beyond them.
 * d_out[m] equals the fold acc = seed_m; acc = crc32c_combine(acc,
 * d_seg_out[s], landed length of s) over message m's segments of that side.
 * A null d_seg_out, or a seg_side other than the two above, gives -EINVAL. */
#define PHOTON_CRC_SEG_OF_SRC 0
#define PHOTON_CRC_SEG_OF_DST 1
int photon_crc32c_copy_msg_iov_seg_n(const photon_crc_iovec* d_src, const uint64_t* d_src_start, uint64_t nsrc,
                                     const photon_crc_iovec* d_dst, const uint64_t* d_dst_start, uint64_t ndst,
                                     uint64_t nmsg, const uint64_t* d_size,
                                     uint32_t seed0, const uint32_t* d_seeds,
                                     int seg_side, uint32_t* d_seg_out,
                                     uint32_t* d_out, uint64_t* d_copied, void* stream);

/* photon_crc32c_copy_msg_iov_n that also returns one CRC per segment of BOTH
 * sides, from the same read: exactly the sum of the two one-side calls above
 * (re-blocking between two block-checksummed layouts: the source-side CRCs
 * check the stored words, photon_crc32c_verify_n, the destination-side CRCs
 * stamp the new blocks, photon_crc32c_stamp_n). The copy, k_m, d_out[m]
 * (bit-identical) and d_copied[m] are those of photon_crc32c_copy_msg_iov_n,
 * and so are the alignment rule and contract (iv). d_src_seg_out (nsrc
 * entries, indexed like d_src) holds what the PHOTON_CRC_SEG_OF_SRC call
 * writes to d_seg_out, d_dst_seg_out (ndst entries, indexed like d_dst) what
 * the PHOTON_CRC_SEG_OF_DST call writes: crc32c_extend from seed 0 over the
 * bytes of the segment that took part in the copy -- the whole segment where
 * the copy covered it, the landed prefix for the segment in which the copy
 * ended, 0 for a zero-length segment and for every segment of which nothing
 * landed. Every entry of both arrays for all nmsg messages is written (no
 * pre-clearing), nothing beyond them. While the call runs the two arrays hold
 * intermediate values; they must not overlap each other or anything else the
 * call touches. A null d_src_seg_out or d_dst_seg_out gives -EINVAL.
 * Asynchronous on `stream` (two kernels), nothing is allocated or
 * synchronised, no workspace; capturable and replayable. */
int photon_crc32c_copy_msg_iov_seg2_n(const photon_crc_iovec* d_src, const uint64_t* d_src_start, uint64_t nsrc,
                                      const photon_crc_iovec* d_dst, const uint64_t* d_dst_start, uint64_t ndst,
                                      uint64_t nmsg, const uint64_t* d_size,
                                      uint32_t seed0, const uint32_t* d_seeds,
                                      uint32_t* d_src_seg_out, uint32_t* d_dst_seg_out,
                                      uint32_t* d_out, uint64_t* d_copied, void* stream);

/* The ranged read from checksummed blocks: every source segment of a message
 * (the blocks that cover the range) is read in full, exactly once, and
 * checksummed, and only a window of the source stream lands in the
 * destination iovector. With L = the sum of message m's source lengths, D =
 * the sum of its destination lengths (both saturating), skip_m = d_skip ?
 * d_skip[m] : 0 and size_m = d_size ? d_size[m] : unlimited,
 *   a = min(skip_m, L),   k = min(size_m, D, L - a)
 * (no sum of skip_m and size_m is formed), the window is source-stream bytes
 * [a, a + k): byte a + j goes to byte j of the destination stream for j < k,
 * and nothing else is written to any destination. Zero-length segments on
 * either side are skipped (their base may be null).
 *   - d_src_seg_out[s] (nsrc entries, indexed like d_src) = crc32c_extend
 *     from seed 0 over the WHOLE segment s, inside the window or not; 0 for a
 *     zero-length segment. Every entry of all nmsg messages is written (no
 *     pre-clearing). Compare them with the blocks' stored words by
 *     photon_crc32c_verify_n.
 *   - d_out[m] = crc32c_extend over exactly the k window bytes from seed_m
 *     (d_seeds ? d_seeds[m] : seed0); the seed itself when k == 0.
 *   - d_copied[m] = k (optional).
 *   - d_work: device memory of at least photon_crc_window_work_bytes(nmsg) =
 *     16 * nmsg bytes, 8-byte aligned; it needs no clearing, keeps nothing
 *     between calls, and its contents afterwards are unspecified. While the
 *     call runs d_src_seg_out holds intermediate values; neither may overlap
 *     anything else the call touches.
 * The alignment rule of photon_crc32c_copy_msg_iov_n holds per window piece:
 * one with (dst - src) % 16 == 0 is stored from the registers that feed the
 * CRC, any other is copied first and checksummed from the cache; bytes outside
 * the window are loaded once and never stored. Contract (iv) otherwise:
 * nmsg == 0 returns 0 before any check; a null d_src_start, d_dst_start,
 * d_out, d_src_seg_out or d_work, a null d_src with nsrc > 0 or a null d_dst
 * with ndst > 0 gives -EINVAL; no CPU fallback. Asynchronous on `stream` (two
 * kernels), nothing is allocated or synchronised; capturable, and replayable
 * with descriptors, d_skip and d_size that change between replays. */
uint64_t photon_crc_window_work_bytes(uint64_t nmsg);
int photon_crc32c_copy_msg_iov_window_n(const photon_crc_iovec* d_src, const uint64_t* d_src_start, uint64_t nsrc,
                                        const photon_crc_iovec* d_dst, const uint64_t* d_dst_start, uint64_t ndst,
                                        uint64_t nmsg, const uint64_t* d_skip, const uint64_t* d_size,
                                        uint32_t seed0, const uint32_t* d_seeds,
                                        uint32_t* d_src_seg_out, uint32_t* d_out, uint64_t* d_copied,
                                        void* d_work, void* stream);

/* d_out[i] = crc32c_combine(d_crc1[i], d_crc2[i], d_len2[i]) with the
 * reference's shortcuts (crc1 == 0 -> crc2, len2 == 0 -> crc1). */
int photon_crc32c_combine_batch(const uint32_t* d_crc1, const uint32_t* d_crc2, const uint32_t* d_len2,
                                uint64_t count, uint32_t* d_out, void* stream);

/* Device forms of the contiguous-batch calls (crc32c.h:52-57, 71-74, 84-87),
 * same results as the drop-in host functions for the same inputs:
 *   series:          d_crc_parts[i] = crc32c(d_buffer + i*part_size, part_size)
 *                    with crc32c_series' semantics (the SSE4.2 engine that
 *                    crc32c_series_auto selects: part_size < 8 gives 0s);
 *   combine_series:  *d_result = crc32c_combine_series(d_crc, part_size,
 *                    n_parts), including n_parts == 0 -> 0 and the
 *                    part_size == 0 shortcut behaviour;
 *   trim_batch:      d_out[i] = crc32c_trim(d_all[i], d_prefix[i],
 *                    d_suffix[i]); an element whose sizes are inconsistent
 *                    gives 0 (the reference's EINVAL result) and, when d_nerr
 *                    is non-null, increments *d_nerr (zero it beforehand);
 *   extend_device:   *d_out = crc32c_extend(d_data, nbytes, seed) for ONE
 *                    long buffer in ONE launch over the whole device: chunks
 *                    on a grid anchored at a 4 KiB boundary, each lane group's
 *                    chunks folded in registers, the workgroups' values
 *                    XOR-combined by the last workgroup to finish; up to a
 *                    256 KiB block span, the latency path (up to 32 small
 *                    workgroups, no table prologue). Launches of more than
 *                    one workgroup share, per stream, the reduce's state (a
 *                    ticket counting every workgroup of the stream's
 *                    launches, a slot per workgroup): the calls are safe
 *                    from any number of streams and threads. Every call may
 *                    be captured into a HIP graph (even a process's first:
 *                    the per-device setup runs in relaxed capture mode); a
 *                    captured launch of more than one workgroup uses a
 *                    reduce state owned by the graph, reset by the launch
 *                    itself, so the graph replays any number of times, one
 *                    replay at a time: two executable graphs instantiated
 *                    from the same captured graph share those states and
 *                    must not run concurrently.
 * Asynchronous on `stream` like the batches. */
int photon_crc32c_series_device(const void* d_buffer, uint32_t part_size, uint32_t n_parts, uint32_t* d_crc_parts,
                                void* stream);
int photon_crc32c_combine_series_device(const uint32_t* d_crc, uint32_t part_size, uint32_t n_parts,
                                        uint32_t* d_result, void* stream);
int photon_crc32c_trim_batch(const photon_crc_component* d_all, const photon_crc_component* d_prefix,
                             const photon_crc_component* d_suffix, uint64_t count, uint32_t* d_out,
                             uint32_t* d_nerr, void* stream);
int photon_crc32c_extend_device(const void* d_data, uint64_t nbytes, uint32_t seed, uint32_t* d_out, void* stream);

/* Copy + CRC-32C of ONE long buffer in ONE launch over the whole device:
 * [d_dst, d_dst + nbytes) receives the nbytes at src, and *d_out =
 * crc32c_extend(src, nbytes, seed), bit-identical to
 * photon_crc32c_extend_device on the same bytes. The copy + CRC calls at (iv)
 * give one buffer to one lane group, which is right for many small payloads;
 * this one cuts the buffer over the chip on extend_device's plan (chunks on
 * a grid anchored at a 4 KiB boundary of the source; every size takes it, so
 * photon_crc_set_long_shape applies and photon_crc_set_mid_kernel does not).
 * Contract (iv) holds: the source is HBM, or pinned / registered host memory
 * read in place; the destination is device-accessible; source and
 * destination must not overlap (the caller's responsibility, not checked);
 * no byte outside [d_dst, d_dst + nbytes) is written and nothing is
 * read-modify-written; any alignment is correct; with (d_dst - src) % 16 == 0
 * the payload is read exactly once, otherwise each chunk is copied first and
 * checksummed from the cache. Asynchronous on `stream`; nothing is allocated
 * or synchronised beyond what extend_device does, and a call is capturable
 * into a graph under extend_device's rules (the reduce state is owned by the
 * graph, one replay at a time). No CPU fallback.
 *   - A null d_out, or a null src or d_dst with nbytes > 0, gives -EINVAL.
 *   - nbytes == 0 (src and d_dst may be null) writes the seed to *d_out and
 *     touches nothing else.
 * An object assembled from parts: one call per part with seed 0 into
 * dst + offset, on one stream; the outputs are the part CRCs, and the
 * object's CRC is their fold by ONE photon_crc32c_fold_parts_n call on the
 * same stream (below; no synchronisation, parts of any length). */
int photon_crc32c_copy_extend_device(const void* src, void* d_dst, uint64_t nbytes,
                                     uint32_t seed, uint32_t* d_out, void* stream);

/* Copy + CRC-32C of MANY large parts in ONE pass over the whole device: the
 * middle between the batch calls at (iv) (one lane group per buffer: right
 * for 64 Ki x 64 KiB, wrong for 256 x 16 MiB) and a loop of
 * photon_crc32c_copy_extend_device (one launch per part, whose fixed cost
 * dominates parts of a few MiB). The descriptors are device-resident, as in
 * photon_crc32c_copy_batch_iov: part i is d_src[i] = {base, len} and lands at
 * d_dst[i]. max_part_bytes caps every part, n_i = min(d_src[i].len,
 * max_part_bytes) (a cap like d_size in photon_crc32c_copy_msg_iov_n, and all
 * the host knows of the lengths): [d_dst[i], d_dst[i] + n_i) receives the
 * first n_i bytes of part i, and
 *     d_out[i] = crc32c_extend(src_i, n_i, seed_i),
 * seed_i = d_seeds ? d_seeds[i] : seed0, bit-identical to
 * photon_crc32c_copy_extend_device / photon_crc32c_extend_device on the same
 * bytes. Every part is cut into pieces (32 KiB unless
 * photon_crc_set_parts_piece says otherwise) anchored at a 4 KiB boundary of
 * its source, one lane group per piece over a persistent grid; a second
 * kernel folds each part's piece CRCs with its seed. Two launches per call.
 * Contract (iv) holds: sources are HBM, or pinned / registered host memory
 * read in place; destinations are device-accessible; no source overlaps a
 * destination and no two destinations overlap (the caller's responsibility,
 * not checked); no byte outside a destination range is written and nothing
 * is read-modify-written, so parts may land back to back at odd addresses;
 * any alignment is correct; a part with (d_dst[i] - base_i) % 16 == 0 is read
 * exactly once, any other is copied piece by piece first and checksummed
 * from the cache. d_work is the call's workspace of at least
 * photon_crc_parts_work_bytes(nparts, max_part_bytes, 0) bytes of device
 * memory (one CRC word per piece slot), 8-byte aligned; it needs no clearing
 * and holds nothing between calls. Asynchronous on `stream`; the calls
 * allocate nothing, synchronise nothing and use plain stores only (no
 * atomics, no memset, no per-stream state), so a call is capturable into a
 * graph and replayable any number of times, and calls may run concurrently
 * with distinct d_out / d_work. No CPU fallback.
 *   - nparts == 0 returns 0 and touches nothing.
 *   - A part with n_i == 0 writes its seed to d_out[i] and nothing else (its
 *     base may be null); max_part_bytes == 0 makes every part empty.
 *   - A null d_src / d_iov, d_out or d_work, or a null d_dst in the copying
 *     forms, with nparts > 0 gives -EINVAL ("null ..."); work_bytes below
 *     photon_crc_parts_work_bytes(...) gives -EINVAL naming both numbers; more
 *     than 2^40 piece slots (nparts x slots per part) gives -EINVAL.
 * The object's CRC is ONE photon_crc32c_fold_parts_n call over d_out on the
 * same stream (below), as after the per-part loop. */
int photon_crc32c_copy_parts_n(const photon_crc_iovec* d_src, void* const* d_dst, uint64_t nparts,
                               uint64_t max_part_bytes, uint32_t seed0, const uint32_t* d_seeds,
                               uint32_t* d_out, void* d_work, uint64_t work_bytes, void* stream);
/* The same without the copy: d_out[i] = crc32c_extend(d_iov[i].base, n_i,
 * seed_i), every part cut over the chip (photon_crc32c_batch_iov gives a part
 * to one lane group). */
int photon_crc32c_batch_parts_n(const photon_crc_iovec* d_iov, uint64_t nparts, uint64_t max_part_bytes,
                                uint32_t seed0, const uint32_t* d_seeds, uint32_t* d_out,
                                void* d_work, uint64_t work_bytes, void* stream);
/* Bytes of d_work the four _parts_n calls need for these arguments under the
 * current piece setting: nparts x max(1, ceil(max_part_bytes / piece)) words
 * of 4 bytes, or 8 if crc64 (~0 when that is more than 2^40 words). */
uint64_t photon_crc_parts_work_bytes(uint64_t nparts, uint64_t max_part_bytes, int crc64);

/* Copy + CRC-32C of MIXED-SIZE parts: photon_crc32c_copy_parts_n with the
 * piece tasks PACKED on the device. The calls above give
 * every part the slots of the longest (nparts x ceil(max_part_bytes / piece)
 * tasks and workspace words): right for parts of about one length, wrong for
 * a few thousand buffers from 4 KiB to tens of MiB, or for a cap far above
 * the real lengths. Here the host passes a bound on the SUM of the lengths
 * (a pool's size, an object's size, a Content-Length), the piece count of
 * every part is summed on the device, and the piece kernel runs exactly
 *     T = sum_i pieces(src_i, n_i)
 * tasks. The contract of photon_crc32c_copy_parts_n carries over word for
 * word: n_i = min(d_src[i].len, max_part_bytes) (max_part_bytes may be ~0 at
 * no cost), [d_dst[i], d_dst[i] + n_i) receives part i, d_out[i] =
 * crc32c_extend(src_i, n_i, seed_i) bit-identical to that call, the same cut
 * (pieces anchored at 4 KiB of the source, photon_crc_set_parts_piece),
 * contract (iv), plain stores only (no atomics, no memset, no per-stream
 * state), nothing allocated or synchronised, capturable and replayable (the
 * plan is rebuilt on the device by every replay: the descriptors may change
 * between replays), concurrent calls with distinct d_out / d_report / d_work,
 * no CPU fallback. Three things differ:
 *   - Capacity from the total. A part has at most n_i / piece + 1 pieces
 *     (its head merges into the first piece; a short last piece needs a
 *     slot), so for any parts with sum n_i <= max_total_bytes
 *         T <= C = floor(max_total_bytes / piece) + nparts
 *     piece slots suffice. d_work holds at least
 *     photon_crc_parts_packed_work_bytes(nparts, max_total_bytes, crc64)
 *         = 8 (nparts + 1) + 16 ceil(nparts / 1024) + 8 ceil(C w / 8) + 8 ceil(C / 2)
 *     bytes of device memory, 8-byte aligned (w = 4, or 8 if crc64): the
 *     first task of every part and T (nparts + 1 words of 64 bits), two
 *     64-bit words per plan tile of 1,024 parts, C CRC words, C 32-bit words
 *     of the task-to-part map. It needs no clearing and holds nothing
 *     between calls.
 *   - The report. d_report is four uint64_t of device memory, written by every
 *     call with nparts > 0: [0] = 1 if T > C, else 0; [1] = T; [2] = sum n_i;
 *     [3] = C (sums beyond 2^64 saturate at ~0).
 *   - Overflow writes nothing else. If [0] == 1 (the parts were longer in sum
 *     than max_total_bytes allowed for), no destination byte and no d_out word
 *     is written: all or nothing. Looking at [0] before trusting d_out is the
 *     caller's job, on stream-ordered terms, as with photon_crc_verify_report.
 *   - nparts == 0 returns 0 and touches nothing, d_report included.
 *   - -EINVAL before anything is enqueued: a null d_src / d_iov, d_out,
 *     d_report or d_work, or a null d_dst in the copying forms ("null ...");
 *     nparts above 2^31; C above 2^40; work_bytes below the size above (both
 *     numbers in the text); a d_work that is not 8-byte aligned.
 * Six launches per call (four small plan kernels, the piece kernel, the part
 * fold). For parts of one length the calls above are the ones to take. */
int photon_crc32c_copy_parts_packed_n(const photon_crc_iovec* d_src, void* const* d_dst, uint64_t nparts,
                                      uint64_t max_part_bytes, uint64_t max_total_bytes, uint32_t seed0,
                                      const uint32_t* d_seeds, uint32_t* d_out, uint64_t* d_report,
                                      void* d_work, uint64_t work_bytes, void* stream);
/* The same without the copy. */
int photon_crc32c_batch_parts_packed_n(const photon_crc_iovec* d_iov, uint64_t nparts, uint64_t max_part_bytes,
                                       uint64_t max_total_bytes, uint32_t seed0, const uint32_t* d_seeds,
                                       uint32_t* d_out, uint64_t* d_report, void* d_work,
                                       uint64_t work_bytes, void* stream);
/* Bytes of d_work the four _parts_packed_n calls need under the current piece
 * setting (the formula above); 0 for nparts == 0, ~0 when nparts is above
 * 2^31 or C above 2^40. */
uint64_t photon_crc_parts_packed_work_bytes(uint64_t nparts, uint64_t max_total_bytes, int crc64);

/* (many GPUs) ONE logical buffer whose bytes lie on several devices of this
 * process: span i = [d_data, d_data + nbytes) on `device`, the spans in
 * buffer order. Every span runs photon_crc32c_extend_device (from seed 0) on
 * its own device, all devices at once; the host folds the span CRCs with
 * crc32c_combine's identity (crc.cpp:393-405): acc = seed, then acc =
 * acc * x^(8 len_i) ^ crc_i. 4 bytes per device cross the host link; no
 * collective. Synchronous: *h_result = crc32c_extend(buffer, total, seed).
 * The caller's current device is restored. */
typedef struct photon_crc_span {
    int device;
    const void* d_data;
    uint64_t nbytes;
} photon_crc_span;
int photon_crc32c_extend_spans(const photon_crc_span* spans, int nspans, uint32_t seed, uint32_t* h_result);

/* Route the drop-in entry points to the device when handed device memory:
 * with on != 0, crc32c_auto / crc32c_series_auto / crc32c_combine_series_auto
 * (crc.cpp:126-134) and crc64ecma_auto / crc64ecma_series_auto /
 * crc64ecma_combine_series_auto point to wrappers that ask HIP whether the data pointer
 * is device memory (hipMemoryTypeDevice) and, if so, run the calls above
 * synchronously on that pointer's device, else call the host engine. A
 * routed call runs on a non-blocking stream leased from a per-device pool
 * (never the legacy default stream, so it does not serialise against the
 * process's other streams; concurrent routed calls get streams of their
 * own) and its result is written by the kernel into pinned host memory. The
 * calling thread (a photon vCPU: its coroutines wait with it) does not spin
 * through a long kernel: a call whose bytes would take longer than the poll
 * window first sleeps through most of its expected time, then polls the
 * result words with a pause between reads for at most 40 us, then sleeps in
 * 10 us slices between reads (photon_crc_set_routed_wait, tuning.h). Off (the
 * default, also at load time) restores the host engines. The reference signatures have no error channel and the reference
 * always computes (crc.cpp:114-117), so a routed call whose device work
 * fails NEVER returns a made-up value: it is reported on stderr, counted,
 * errno is set to EIO, and the bytes are copied to the host and checksummed
 * by the host engine (same result as the reference); if even that copy fails
 * the process aborts with a message. Returns 0, or -EIO if a routed call
 * failed since the last switch (photon_crc_dispatch_fallbacks() counts them).
 * Ordering: like the reference's crc32c_extend (crc32c.h:30-33), a routed
 * call checksums the bytes that exist when it is called. It takes no stream
 * and orders against none of the caller's: the caller must have COMPLETED
 * every write to the buffer (kernel, copy, vDMA, peer write) before the call,
 * e.g. hipStreamSynchronize / hipEventSynchronize on the producer's stream.
 * A write still in flight may or may not be seen. For stream-ordered work use
 * photon_crc32c_extend_device / photon_crc64ecma_extend_device on the
 * producer's stream instead. */
int photon_crc_set_device_dispatch(int on);
/* Number of routed calls so far whose device work failed and that were
 * recomputed on the host (0 in a healthy process; tests assert it). */
uint64_t photon_crc_dispatch_fallbacks(void);

/* CRC-64/ECMA batches (reference crc64ecma.h:20-38: reflected polynomial
 * 0xC96C5795D7870F42, init and result inverted):
 *   out[i] = crc64ecma_extend(buffer_i, nbytes_i, seed_i)
 * Same shapes and rules as the CRC32C strided / iovec batches. */
int photon_crc64ecma_batch_strided(const void* d_base, uint64_t stride, uint64_t nbytes, uint64_t count,
                                   uint64_t seed0, const uint64_t* d_seeds, uint64_t* d_out, void* stream);
int photon_crc64ecma_batch_iov(const photon_crc_iovec* d_iov, uint64_t count, uint64_t seed0,
                               const uint64_t* d_seeds, uint64_t* d_out, void* stream);

/* CRC-64/ECMA forms of the CRC32C calls above (crc64ecma.h:20-87):
 *   combine_batch: d_out[i] = crc64ecma_combine(d_crc1[i], d_crc2[i], d_len2[i])
 *                  (crc1 == 0 -> crc2, as the reference);
 *   batch_msg_n:   d_out[m] = crc64ecma_extend chained over message m's
 *                  segments from seed_m (e.g. an OSS object's iovector,
 *                  ecosystem/oss.h:217 expected_crc64); d_seg_out[s] = each
 *                  segment's crc64ecma(seg, 0); nseg == d_msg_start[nmsg];
 *   extend_device: *d_out = crc64ecma_extend(d_data, nbytes, seed) for ONE
 *                  long device buffer (one launch, as the CRC32C call). */
/* Same layout as CRC64ECMA_Component {uint64_t crc; uint64_t size;}
 * (common/checksum/crc64ecma.h:68-71). */
typedef struct photon_crc64_component {
    uint64_t crc;
    uint64_t size;
} photon_crc64_component;

/* d_out[i] = crc64ecma_trim(d_all[i], d_prefix[i], d_suffix[i])
 * (crc64ecma.h:73-87); inconsistent sizes give 0 and count in *d_nerr. */
int photon_crc64ecma_trim_batch(const photon_crc64_component* d_all, const photon_crc64_component* d_prefix,
                                const photon_crc64_component* d_suffix, uint64_t count, uint64_t* d_out,
                                uint32_t* d_nerr, void* stream);

/* photon_crc32c_host_batch_strided for CRC-64/ECMA: host (e.g. an OSS
 * upload's) buffers through the same chunked H2D + kernel + D2H pipeline. */
int photon_crc64ecma_host_batch_strided(const void* h_base, uint64_t stride, uint64_t nbytes, uint64_t count,
                                        uint64_t seed0, const uint64_t* h_seeds, uint64_t* h_out);
int photon_crc64ecma_combine_batch(const uint64_t* d_crc1, const uint64_t* d_crc2, const uint32_t* d_len2,
                                   uint64_t count, uint64_t* d_out, void* stream);
/* photon_crc32c_batch_msg_n for CRC-64/ECMA: d_out[m] = crc64ecma_extend
 * chained over message m's segments from seed_m. d_seg_out (per-segment CRCs
 * from seed 0) is optional. */
int photon_crc64ecma_batch_msg_n(const photon_crc_iovec* d_iov, const uint64_t* d_msg_start, uint64_t nmsg,
                                 uint64_t nseg, uint64_t seed0, const uint64_t* d_seeds, uint64_t* d_seg_out,
                                 uint64_t* d_out, void* stream);
/* Copy + CRC-64/ECMA in one pass: photon_crc32c_copy_batch_strided / _iov and
 * photon_crc32c_gather_msg_n for CRC-64/ECMA, under the contract written at
 * (iv) above (asynchronous, nothing allocated or synchronised, capturable; no
 * byte outside [dst, dst + len) written; any alignment, one read when
 * (dst - src) % 16 == 0). Values are crc64ecma_extend's (crc.cpp:119-122):
 * d_out[i] / d_out[m] what photon_crc64ecma_batch_strided / _batch_iov /
 * _batch_msg_n give for the same inputs, d_seg_out[s] (optional) =
 * crc64ecma(seg_s, 0). An OSS multipart upload's parts assembled back to
 * back, with a CRC per part and the object's CRC, is one gather call. */
int photon_crc64ecma_copy_batch_strided(const void* src_base, uint64_t src_stride,
                                        void* d_dst_base, uint64_t dst_stride,
                                        uint64_t nbytes, uint64_t count, uint64_t seed0,
                                        const uint64_t* d_seeds, uint64_t* d_out, void* stream);
int photon_crc64ecma_copy_batch_iov(const photon_crc_iovec* d_src, void* const* d_dst,
                                    uint64_t count, uint64_t seed0, const uint64_t* d_seeds,
                                    uint64_t* d_out, void* stream);
int photon_crc64ecma_gather_msg_n(const photon_crc_iovec* d_iov, const uint64_t* d_msg_start,
                                  uint64_t nmsg, uint64_t nseg, void* const* d_dst,
                                  uint64_t seed0, const uint64_t* d_seeds,
                                  uint64_t* d_seg_out, uint64_t* d_out, void* stream);
/* photon_crc32c_copy_msg_iov_n for CRC-64/ECMA: the same arguments, walk and
 * contract; d_out[m] = crc64ecma_extend over the k_m copied bytes from seed_m. */
int photon_crc64ecma_copy_msg_iov_n(const photon_crc_iovec* d_src, const uint64_t* d_src_start, uint64_t nsrc,
                                    const photon_crc_iovec* d_dst, const uint64_t* d_dst_start, uint64_t ndst,
                                    uint64_t nmsg, const uint64_t* d_size,
                                    uint64_t seed0, const uint64_t* d_seeds,
                                    uint64_t* d_out, uint64_t* d_copied, void* stream);
/* photon_crc32c_copy_msg_iov_seg_n for CRC-64/ECMA: the same arguments and
 * contract; d_seg_out[s] = crc64ecma_extend from seed 0 over the bytes of
 * segment s that took part in the copy. */
int photon_crc64ecma_copy_msg_iov_seg_n(const photon_crc_iovec* d_src, const uint64_t* d_src_start, uint64_t nsrc,
                                        const photon_crc_iovec* d_dst, const uint64_t* d_dst_start, uint64_t ndst,
                                        uint64_t nmsg, const uint64_t* d_size,
                                        uint64_t seed0, const uint64_t* d_seeds,
                                        int seg_side, uint64_t* d_seg_out,
                                        uint64_t* d_out, uint64_t* d_copied, void* stream);
/* photon_crc32c_copy_msg_iov_seg2_n for CRC-64/ECMA: the same arguments and
 * contract; the entries of both arrays are crc64ecma_extend from seed 0. */
int photon_crc64ecma_copy_msg_iov_seg2_n(const photon_crc_iovec* d_src, const uint64_t* d_src_start, uint64_t nsrc,
                                         const photon_crc_iovec* d_dst, const uint64_t* d_dst_start, uint64_t ndst,
                                         uint64_t nmsg, const uint64_t* d_size,
                                         uint64_t seed0, const uint64_t* d_seeds,
                                         uint64_t* d_src_seg_out, uint64_t* d_dst_seg_out,
                                         uint64_t* d_out, uint64_t* d_copied, void* stream);
/* photon_crc32c_copy_msg_iov_window_n for CRC-64/ECMA: the same arguments,
 * window, workspace and contract; d_src_seg_out and d_out are
 * crc64ecma_extend values (uint64_t seeds and outputs). */
int photon_crc64ecma_copy_msg_iov_window_n(const photon_crc_iovec* d_src, const uint64_t* d_src_start, uint64_t nsrc,
                                           const photon_crc_iovec* d_dst, const uint64_t* d_dst_start, uint64_t ndst,
                                           uint64_t nmsg, const uint64_t* d_skip, const uint64_t* d_size,
                                           uint64_t seed0, const uint64_t* d_seeds,
                                           uint64_t* d_src_seg_out, uint64_t* d_out, uint64_t* d_copied,
                                           void* d_work, void* stream);
/* photon_crc32c_extend_device for CRC-64/ECMA (crc64ecma_extend, crc.cpp:
 * 119-122): the same latency path for spans up to 256 KiB (a small kernel of
 * up to 33 workgroups), one launch over the chip above, the same per-stream
 * state and capture rules. */
int photon_crc64ecma_extend_device(const void* d_data, uint64_t nbytes, uint64_t seed, uint64_t* d_out,
                                   void* stream);
/* photon_crc32c_copy_extend_device for CRC-64/ECMA: the same arguments, plan
 * and contract; *d_out = crc64ecma_extend(src, nbytes, seed), bit-identical
 * to photon_crc64ecma_extend_device on the same bytes. An OSS object part of
 * tens of MiB to GiB is landed and given its x-oss-hash-crc64ecma by one
 * call; the object's CRC is the parts' fold: one
 * photon_crc64ecma_fold_parts_n call on the same stream (below). */
int photon_crc64ecma_copy_extend_device(const void* src, void* d_dst, uint64_t nbytes,
                                        uint64_t seed, uint64_t* d_out, void* stream);
/* photon_crc32c_copy_parts_n / photon_crc32c_batch_parts_n for CRC-64/ECMA:
 * the same arguments, cut, workspace rule (photon_crc_parts_work_bytes(...,
 * 1): 8-byte words) and contract; d_out[i] = crc64ecma_extend(src_i, n_i,
 * seed_i). The parts of an OSS multipart upload are landed and given their
 * x-oss-hash-crc64ecma by one call; the object's CRC is one
 * photon_crc64ecma_fold_parts_n call on the same stream. */
int photon_crc64ecma_copy_parts_n(const photon_crc_iovec* d_src, void* const* d_dst, uint64_t nparts,
                                  uint64_t max_part_bytes, uint64_t seed0, const uint64_t* d_seeds,
                                  uint64_t* d_out, void* d_work, uint64_t work_bytes, void* stream);
int photon_crc64ecma_batch_parts_n(const photon_crc_iovec* d_iov, uint64_t nparts, uint64_t max_part_bytes,
                                   uint64_t seed0, const uint64_t* d_seeds, uint64_t* d_out,
                                   void* d_work, uint64_t work_bytes, void* stream);
/* photon_crc32c_copy_parts_packed_n / photon_crc32c_batch_parts_packed_n for
 * CRC-64/ECMA: the same arguments, report, overflow rule and workspace
 * (photon_crc_parts_packed_work_bytes(..., 1): 8-byte CRC words); d_out[i] =
 * crc64ecma_extend(src_i, n_i, seed_i). */
int photon_crc64ecma_copy_parts_packed_n(const photon_crc_iovec* d_src, void* const* d_dst, uint64_t nparts,
                                         uint64_t max_part_bytes, uint64_t max_total_bytes, uint64_t seed0,
                                         const uint64_t* d_seeds, uint64_t* d_out, uint64_t* d_report,
                                         void* d_work, uint64_t work_bytes, void* stream);
int photon_crc64ecma_batch_parts_packed_n(const photon_crc_iovec* d_iov, uint64_t nparts, uint64_t max_part_bytes,
                                          uint64_t max_total_bytes, uint64_t seed0, const uint64_t* d_seeds,
                                          uint64_t* d_out, uint64_t* d_report, void* d_work,
                                          uint64_t work_bytes, void* stream);
/* photon_crc32c_extend_spans for CRC-64/ECMA (crc64ecma_combine's identity:
 * the inverted CRC folds the same way). */
int photon_crc64ecma_extend_spans(const photon_crc_span* spans, int nspans, uint64_t seed, uint64_t* h_result);

/* photon_crc32c_series_device / photon_crc32c_combine_series_device for
 * CRC-64/ECMA, with the semantics of this library's host definitions
 * (crc64_cpu.cpp; the reference declares crc64ecma_series /
 * crc64ecma_combine_series and never defines them):
 *   series:         d_crc_parts[i] = crc64ecma(d_buffer + i*part_size,
 *                   part_size, 0), for every part_size (no part_size < 8
 *                   quirk); part_size == 0 writes zeros and reads nothing;
 *                   n_parts == 0 returns 0 and touches nothing;
 *   combine_series: *d_result = crc64ecma_combine_series(d_crc, part_size,
 *                   n_parts) = XOR_i crc[i] * K^(n-1-i), K = x^(8*part_size)
 *                   (K = 1 for part_size 0); n_parts == 0 gives 0.
 * Asynchronous on `stream`; a null required pointer gives -EINVAL. */
int photon_crc64ecma_series_device(const void* d_buffer, uint32_t part_size, uint32_t n_parts,
                                   uint64_t* d_crc_parts, void* stream);
int photon_crc64ecma_combine_series_device(const uint64_t* d_crc, uint32_t part_size, uint32_t n_parts,
                                           uint64_t* d_result, void* stream);

/* Fold the CRCs of objects' parts into the objects' CRCs on the device: the
 * step after one photon_crc32c_copy_extend_device /
 * photon_crc64ecma_copy_extend_device call per part (seed 0), on the same
 * stream, with nothing in between. Object m is the parts s in
 * [d_obj_start[m], d_obj_start[m+1]) of the nparts (CRC, length) pairs
 * d_crc[s], d_len[s]; d_obj_start has nobj + 1 entries and its last must
 * equal nparts (the caller's duty, as in the _msg_n calls; no part outside
 * [0, nparts) is read in any case). A null d_obj_start means ONE object of all
 * nparts parts, and nobj must then be 1. With acc = seed_m (d_seeds[m], or
 * seed0 when d_seeds is null):
 *     acc = acc * x^(8 * d_len[s]) ^ d_crc[s]   over the parts in order,
 *     d_out[m] = acc
 * -- the identity of extend_spans (crc.cpp:393-405): for part CRCs computed
 * from seed 0, d_out[m] = crc32c_extend / crc64ecma_extend of the
 * concatenated bytes from seed_m (the inverted CRC-64 folds the same way).
 * Lengths are 64-bit byte counts: a part of 4 GiB or more is one step. The
 * definition is this linear one for arbitrary pairs: it equals a chain of
 * crc32c_combine calls except where a part has length 0 and a non-zero CRC
 * (the chain's len2 == 0 shortcut ignores that CRC; no real part has one),
 * and it equals the crc64ecma_combine chain always. d_total (optional):
 * d_total[m] = the object's byte length, wrapping mod 2^64 (the CRC is that
 * of the definition above only while an object's lengths sum to less than
 * 2^64). An object with no parts gives its seed and a total of 0.
 *   - nobj == 0 returns 0 and touches nothing.
 *   - d_crc and d_len may be null only when nparts == 0; a null d_out, or a
 *     null d_obj_start with nobj != 1, gives -EINVAL ("null ..." in
 *     photon_crc_last_error()).
 * All arrays are device-accessible memory (HBM, or pinned / registered host
 * memory read in place). Asynchronous on `stream`. The calls allocate
 * nothing and synchronise nothing, and write only d_out[0..nobj) and
 * d_total[0..nobj), with plain stores: no memset, no atomics, no per-stream
 * state -- so they are capturable into a graph and replayable any number of
 * times, also concurrently on different outputs. No CPU fallback. One
 * workgroup folds one object, its parts spread over the workgroup's threads
 * (64, 256 or 1,024 of them, by nparts / nobj): an object of millions of
 * parts stays correct but runs on that one workgroup. */
int photon_crc32c_fold_parts_n(const uint32_t* d_crc, const uint64_t* d_len,
                               const uint64_t* d_obj_start, uint64_t nobj, uint64_t nparts,
                               uint32_t seed0, const uint32_t* d_seeds,
                               uint32_t* d_out, uint64_t* d_total, void* stream);
int photon_crc64ecma_fold_parts_n(const uint64_t* d_crc, const uint64_t* d_len,
                                  const uint64_t* d_obj_start, uint64_t nobj, uint64_t nparts,
                                  uint64_t seed0, const uint64_t* d_seeds,
                                  uint64_t* d_out, uint64_t* d_total, void* stream);

/* The running CRCs of objects over their parts: photon_crc32c_fold_parts_n /
 * photon_crc64ecma_fold_parts_n with every intermediate value kept. Inputs as
 * the fold's: nparts (CRC from seed 0, 64-bit length) pairs, d_obj_start with
 * nobj + 1 entries or null for ONE object of all parts (nobj must then be 1),
 * seed_m = d_seeds ? d_seeds[m] : seed0. For object m over its parts s in
 * order, with A = seed_m and E = 0:
 *     A = A * x^(8 * d_len[s]) ^ d_crc[s];   d_run[s] = A;
 *     E += d_len[s];                         d_end[s] = E;   (optional; mod 2^64)
 * -- the fold's linear definition (the same remark about a part of length 0
 * with a non-zero CRC), so the last entry of every non-empty object is
 * bit-identical to the fold's d_out[m] and d_total[m] on the same inputs. For
 * part CRCs over real bytes d_run[s] = crc32c_extend / crc64ecma_extend of
 * the object's bytes through part s from seed_m: the value
 * x-oss-hash-crc64ecma carries after that append (ecosystem/oss.cpp:1271-1298),
 * and d_end[s] is the next append's position. An empty object writes nothing
 * (its CRC is its seed). Any range of whole parts follows from two running
 * values through photon_crc32c_trim_batch.
 *   - nobj == 0 or nparts == 0 returns 0 and touches nothing.
 *   - A null d_crc, d_len, d_run or d_work, or a null d_obj_start with
 *     nobj != 1, gives -EINVAL ("null ..." in photon_crc_last_error()).
 *   - d_work: device memory of at least photon_crc_scan_work_bytes(nparts)
 *     bytes (work_bytes says how many it has), 8-byte aligned; it needs no
 *     clearing and keeps nothing between calls. A work_bytes too small gives
 *     -EINVAL (both numbers in the error text), and so does an nparts for
 *     which photon_crc_scan_work_bytes returns ~0 (more than 2^40 parts).
 *   - d_obj_start must be non-decreasing, start at 0 and end at nparts (the
 *     caller's duty). If it does not, the values are unspecified, but no entry
 *     outside [0, nparts) of any array (and none outside d_obj_start[0..nobj),
 *     d_seeds[0..nobj)) is read or written.
 *   - d_run and d_end must not overlap the inputs (not checked).
 * All arrays are device-accessible memory; d_len and d_obj_start may be
 * pinned host memory. Asynchronous on `stream`. The calls allocate nothing and
 * synchronise nothing and write with plain stores only: no atomics, no
 * memset, no per-stream state; every workspace word a call reads, that call
 * wrote -- the result is deterministic, a call is capturable into a graph and
 * replayable, and calls may run concurrently with distinct d_run / d_end /
 * d_work. No CPU fallback. A segmented scan in tiles of the index space,
 * whatever objects a tile holds: one object of N parts is
 * spread over about N / tile workgroups. At most three launches (reduce the
 * tiles, carry across them, apply); one when everything is one tile. */
uint64_t photon_crc_scan_work_bytes(uint64_t nparts);

int photon_crc32c_scan_parts_n(const uint32_t* d_crc, const uint64_t* d_len,
                               const uint64_t* d_obj_start, uint64_t nobj, uint64_t nparts,
                               uint32_t seed0, const uint32_t* d_seeds,
                               uint32_t* d_run, uint64_t* d_end,
                               void* d_work, uint64_t work_bytes, void* stream);
int photon_crc64ecma_scan_parts_n(const uint64_t* d_crc, const uint64_t* d_len,
                                  const uint64_t* d_obj_start, uint64_t nobj, uint64_t nparts,
                                  uint64_t seed0, const uint64_t* d_seeds,
                                  uint64_t* d_run, uint64_t* d_end,
                                  void* d_work, uint64_t work_bytes, void* stream);

/* Check stored CRCs on the device: the step after any call above that left
 * `count` computed words in d_crc, on the same stream, with nothing in
 * between. Entry i is BAD when d_crc[i] differs from its expected word.
 *   verify_n: the expected word of entry i is the little-endian word at
 *     (const char*)d_expected + i * expected_stride, at ANY address (it is
 *     read by a word load where aligned and bytewise elsewhere, never by a
 *     misaligned word load) and with any stride >= the word width (4, or 8
 *     for CRC-64). Stride = width is a dense array; stride 8 / 16 with the CRC
 *     first is a CRC32C_Component / CRC64ECMA_Component array; d_expected =
 *     base + nbytes with expected_stride = stride is the trailer behind each
 *     payload of a strided batch (net/test/zerocopy-client.cpp:112-118). A
 *     stride below the width with count > 1 gives -EINVAL.
 *   verify_ptr_n: d_expected_ptr[i] points at entry i's expected word, any
 *     alignment (e.g. iov[i].base + iov[i].len, built by the caller like the
 *     d_dst[] lists). A null pointer means entry i is NOT COMPARED: neither
 *     bad nor counted in the report's count (blocks with no stored CRC).
 * Result: all four words of *d_report are written by every call with count >
 * 0; d_bad_idx[0 .. nlisted) holds the bad indices in ASCENDING order, and
 * nothing at or beyond d_bad_idx[nlisted] is written. d_bad_idx may be null
 * when bad_cap == 0 (count only). d_report and d_bad_idx may be pinned host
 * memory: the host reads them after the stream's sync with no copy.
 *   - count == 0 returns 0 and touches NOTHING, the report included.
 *   - A null d_crc, d_expected / d_expected_ptr, d_report or d_work, or a null
 *     d_bad_idx with bad_cap > 0, gives -EINVAL ("null ..." in
 *     photon_crc_last_error()).
 *   - d_work: device memory of at least photon_crc_verify_work_bytes(count)
 *     bytes (work_bytes says how many it has), 8-byte aligned; it needs no
 *     clearing and keeps nothing between calls. A work_bytes too small gives
 *     -EINVAL (both numbers in the error text), and so does a count for which
 *     photon_crc_verify_work_bytes returns ~0 (more than 2^40 entries).
 * Asynchronous on `stream`. The calls allocate nothing and synchronise
 * nothing and write with plain stores only: no atomics, no memset, no
 * per-stream state -- the result is deterministic, a call is capturable into
 * a graph and replayable any number of times, and calls may run concurrently
 * with distinct d_report / d_bad_idx / d_work. No CPU fallback. At most three
 * launches (mark the tiles, scan their counts and write the report, list the
 * indices; the last one only with bad_cap > 0). */
typedef struct photon_crc_verify_report {
    uint64_t nbad;      /* compared entries whose computed word != expected word */
    uint64_t first_bad; /* the lowest such index, ~0ull when nbad == 0 */
    uint64_t nlisted;   /* min(nbad, bad_cap): entries written to d_bad_idx */
    uint64_t count;     /* entries compared (count minus the entries with a null pointer) */
} photon_crc_verify_report;

uint64_t photon_crc_verify_work_bytes(uint64_t count);

int photon_crc32c_verify_n(const uint32_t* d_crc, const void* d_expected, uint64_t expected_stride,
                           uint64_t count, photon_crc_verify_report* d_report,
                           uint64_t* d_bad_idx, uint64_t bad_cap,
                           void* d_work, uint64_t work_bytes, void* stream);
int photon_crc32c_verify_ptr_n(const uint32_t* d_crc, const void* const* d_expected_ptr,
                               uint64_t count, photon_crc_verify_report* d_report,
                               uint64_t* d_bad_idx, uint64_t bad_cap,
                               void* d_work, uint64_t work_bytes, void* stream);
int photon_crc64ecma_verify_n(const uint64_t* d_crc, const void* d_expected, uint64_t expected_stride,
                              uint64_t count, photon_crc_verify_report* d_report,
                              uint64_t* d_bad_idx, uint64_t bad_cap,
                              void* d_work, uint64_t work_bytes, void* stream);
int photon_crc64ecma_verify_ptr_n(const uint64_t* d_crc, const void* const* d_expected_ptr,
                                  uint64_t count, photon_crc_verify_report* d_report,
                                  uint64_t* d_bad_idx, uint64_t bad_cap,
                                  void* d_work, uint64_t work_bytes, void* stream);

/* The mirror of the verify calls, for the write side: word i of d_crc is
 * written little-endian to (char*)d_dst + i * dst_stride (stamp_n) or to
 * d_dst_ptr[i] (stamp_ptr_n; a null pointer skips the entry), at any
 * alignment -- e.g. the dense d_out[] of photon_crc32c_copy_batch_strided
 * placed behind each landed payload. Exactly 4 (CRC-64: 8) bytes are written
 * per entry, as one word where aligned and bytewise elsewhere; nothing is
 * read-modify-written. A dst_stride below the width with count > 1 gives
 * -EINVAL; a null d_crc or d_dst / d_dst_ptr gives -EINVAL ("null ..."); count
 * == 0 returns 0 and touches nothing. Asynchronous on `stream`, one launch,
 * no workspace; allocation, capture and concurrency as the verify calls. */
int photon_crc32c_stamp_n(const uint32_t* d_crc, uint64_t count, void* d_dst, uint64_t dst_stride, void* stream);
int photon_crc32c_stamp_ptr_n(const uint32_t* d_crc, uint64_t count, void* const* d_dst_ptr, void* stream);
int photon_crc64ecma_stamp_n(const uint64_t* d_crc, uint64_t count, void* d_dst, uint64_t dst_stride, void* stream);
int photon_crc64ecma_stamp_ptr_n(const uint64_t* d_crc, uint64_t count, void* const* d_dst_ptr, void* stream);

/* Synchronous convenience: photon_crc32c_batch_strided + stream sync. */
int photon_crc32c_batch_strided_sync(const void* d_base, uint64_t stride, uint64_t nbytes, uint64_t count,
                                     uint32_t seed0, const uint32_t* d_seeds, uint32_t* d_out, void* stream);

/* Tuning knobs, the failure-injection hook and the bench data utilities are
 * declared in <photon_crc/tuning.h> (not for production callers). */

/* Producers outside device memory.
 * photon_crc_host_register: make an existing host range (e.g. the iovec
 * targets of IFile::preadv, fs/filesystem.h:54-70) readable by the kernels in
 * place (hipHostRegister, mapped); undo with photon_crc_host_unregister.
 * photon_crc32c_file_strided: h_out[i] = crc32c_extend(record i, nbytes,
 * seed0) for the records at file offset + i*stride of fd. A reader thread
 * pread()s 4 KiB-aligned chunks (so an O_DIRECT fd works: the device reads
 * what the disk DMA'd, the CPU touches no payload byte) into two pinned chunk
 * buffers while the GPU pipeline checksums the previous chunk. Synchronous;
 * -EIO if the file ends before the last record, -errno on a read error.
 * Concurrent callers each check out their own pinned chunk pair (pairs are
 * cached for reuse) and share one persistent pool of reader threads. */
int photon_crc_host_register(void* ptr, uint64_t len);
int photon_crc_host_unregister(void* ptr);
int photon_crc32c_file_strided(int fd, uint64_t offset, uint64_t stride, uint64_t nbytes, uint64_t count,
                               uint32_t seed0, uint32_t* h_out);

/* Overwrite + CRC delta: the write of a sub-range into a
 * block or object that already has a stored CRC, without rereading the block.
 * Write i has length n_i (nbytes, or d_src[i].len); O_i = the n_i bytes at
 * its destination (d_dst_base + i*dst_stride, or d_dst[i]) when the call
 * starts, N_i = its source bytes. After the call the destination holds N_i and
 *   d_delta[i] = R(O_i xor N_i),
 * R = the raw CRC from a zero register (CRC-32C: crc32c_extend(., 0); CRC-64:
 * ~crc64ecma_extend(., ~0)), which is crc(O_i, s) ^ crc(N_i, s) for every
 * common seed s. n_i == 0 writes nothing and gives 0. Each of the two streams
 * is read once and the destination is written once when source and
 * destination are co-aligned ((dst - src) % 16 == 0); other buffers are
 * correct, with no performance claim, as for the copy calls.
 * Contract (iv) applies unchanged: sources are HBM, or pinned / registered
 * host memory; no byte outside [dst, dst + n) is written; null pointers with
 * a non-zero count give -EINVAL ("null ..." in photon_crc_last_error());
 * count == 0 returns 0 and touches nothing; asynchronous on `stream`, nothing
 * allocated or synchronised; plain stores only and no atomics: capturable and
 * replayable; no CPU fallback. New here, and the caller's duty: two
 * destination ranges must not overlap, and a source must not overlap a
 * destination (with overlap the deltas would depend on the order).
 * photon_crc_set_lanes_per_buffer and photon_crc_set_batch_grid apply as to
 * the copy calls; the rows knobs do not. */
int photon_crc32c_overwrite_batch_strided(const void* src_base, uint64_t src_stride, void* d_dst_base,
                                          uint64_t dst_stride, uint64_t nbytes, uint64_t count, uint32_t* d_delta,
                                          void* stream);
int photon_crc32c_overwrite_batch_iov(const photon_crc_iovec* d_src, void* const* d_dst, uint64_t count,
                                      uint32_t* d_delta, void* stream);
int photon_crc64ecma_overwrite_batch_strided(const void* src_base, uint64_t src_stride, void* d_dst_base,
                                             uint64_t dst_stride, uint64_t nbytes, uint64_t count, uint64_t* d_delta,
                                             void* stream);
int photon_crc64ecma_overwrite_batch_iov(const photon_crc_iovec* d_src, void* const* d_dst, uint64_t count,
                                         uint64_t* d_delta, void* stream);

/* Stored CRCs patched by the deltas of overwrites:
 *   d_crc_out[t] = d_crc_in[t] ^ XOR over the writes i in
 *                  [d_tgt_start[t], d_tgt_start[t+1]) of d_delta[i] * x^(8 * d_tail[i]),
 * d_tail[i] = the 64-bit count of bytes of target t (a block, a whole object)
 * behind the end of write i; a tail of 0 and a tail >= 2^32 are ordinary. A
 * null d_tgt_start: write i patches word i, and ntgt must equal nwrites. An
 * empty group copies the word. d_crc_out may be d_crc_in itself and may not
 * otherwise overlap it. Called once with block tails grouped by block, and
 * again with object tails as one group per object, behind the overwrite call
 * on the same stream with no synchronisation in between, it brings the stored
 * block CRCs and the objects' CRCs up to date; photon_crc32c_verify_n /
 * _stamp_n take the words from there.
 * As the fold calls: ntgt == 0 returns 0 and touches nothing; a null d_delta
 * or d_tail with nwrites > 0, a null d_crc_in or d_crc_out, or a null
 * d_tgt_start with ntgt != nwrites gives -EINVAL; one launch, no workspace,
 * plain stores only (every output word is written by the one workgroup that
 * owns the target, whose threads share the target's writes); capturable and
 * replayable. d_tgt_start (ntgt + 1 entries) must be non-decreasing from 0 to
 * nwrites -- the caller's duty; whatever it holds, nothing outside the arrays
 * is read or written. A target with millions of writes stays correct but is
 * the work of one workgroup. */
int photon_crc32c_patch_n(const uint32_t* d_delta, const uint64_t* d_tail, uint64_t nwrites,
                          const uint64_t* d_tgt_start, uint64_t ntgt, const uint32_t* d_crc_in, uint32_t* d_crc_out,
                          void* stream);
int photon_crc64ecma_patch_n(const uint64_t* d_delta, const uint64_t* d_tail, uint64_t nwrites,
                             const uint64_t* d_tgt_start, uint64_t ntgt, const uint64_t* d_crc_in, uint64_t* d_crc_out,
                             void* stream);

/* Stripe parity + CRC in one read: the XOR parity of a
 * stripe of k equal-length blocks (RAID-5 style, k data blocks plus one
 * parity), and its mirror, the rebuild of a lost block from the survivors.
 * Stripe s has k sources of n_s bytes:
 *   strided: source i = src_base + s*stripe_stride + i*block_stride, n_s =
 *            nbytes, parity s = d_dst_base + s*dst_stride;
 *   ptr:     source i = d_src[s*k + i] (count*k device-resident pointers,
 *            stripe-major), d_dst[s] = {parity address, n_s}.
 * After the call the n_s bytes at parity s hold P_s, the byte-wise XOR of the
 * stripe's sources, and
 *   d_out[s] = crc32c_extend(P_s, n_s, seed_s)   (CRC-64: crc64ecma_extend),
 * the ordinary CRC of the parity bytes with the usual seed rule (d_seeds[s],
 * or seed0 when d_seeds is null), computed from the very registers that are
 * stored. 1 <= k <= 64, else -EINVAL; k = 1 is copy + CRC. In the ptr form a
 * NULL source pointer is an all-zero block that is not read (the short last
 * stripe of an object); a stripe whose sources are all NULL writes n_s zero
 * bytes and returns the CRC of n_s zero bytes from the seed. n_s == 0 writes
 * nothing and returns the seed.
 * Both CRCs are affine, so d_out[s] must equal the XOR of the sources' stored
 * CRCs (plus a zero-run term for an even count): photon_crc32c_xor_expect_n
 * below computes that word, and photon_crc32c_verify_n on the two arrays is
 * an end-to-end check of all k source reads. A rebuild is the same call:
 * sources = the k-1 survivors plus the parity, destination = the lost block,
 * and d_out[s] is compared with the lost block's stored word.
 * Contract (iv) of the copy calls applies unchanged: sources are HBM, or
 * pinned / registered host memory; no byte outside [dst, dst + n) is written;
 * null arrays with a non-zero count give -EINVAL ("null ..." in
 * photon_crc_last_error()); count == 0 returns 0 and touches nothing;
 * asynchronous on `stream`, nothing allocated or synchronised; plain stores
 * only and no atomics: capturable and replayable; no CPU fallback.
 * Overlap: two parity ranges must not overlap (the caller's duty). A parity
 * range may coincide EXACTLY, same address and length, with ONE source of its
 * own stripe: the in-place accumulate P ^= D, or the RAID-5 small write
 * P' = P ^ D_old ^ D_new with k = 3. Any other overlap of a parity with a
 * source is the caller's error.
 * Every source byte is read once and every parity byte written once when all
 * non-null sources of a stripe and its parity are congruent modulo 16, or
 * n_s < 64; any other stripe is correct, with no performance claim (the parity
 * is landed byte by byte and then checksummed from the cache).
 * photon_crc_set_lanes_per_buffer and photon_crc_set_batch_grid apply as to
 * the copy calls; the rows knobs do not. */
int photon_crc32c_xor_batch_strided(const void* src_base, uint64_t stripe_stride, uint64_t block_stride, uint32_t k,
                                    void* d_dst_base, uint64_t dst_stride, uint64_t nbytes, uint64_t count,
                                    uint32_t seed0, const uint32_t* d_seeds, uint32_t* d_out, void* stream);
int photon_crc32c_xor_batch_ptr(const void* const* d_src, uint32_t k, const photon_crc_iovec* d_dst, uint64_t count,
                                uint32_t seed0, const uint32_t* d_seeds, uint32_t* d_out, void* stream);
int photon_crc64ecma_xor_batch_strided(const void* src_base, uint64_t stripe_stride, uint64_t block_stride, uint32_t k,
                                       void* d_dst_base, uint64_t dst_stride, uint64_t nbytes, uint64_t count,
                                       uint64_t seed0, const uint64_t* d_seeds, uint64_t* d_out, void* stream);
int photon_crc64ecma_xor_batch_ptr(const void* const* d_src, uint32_t k, const photon_crc_iovec* d_dst,
                                   uint64_t count, uint64_t seed0, const uint64_t* d_seeds, uint64_t* d_out,
                                   void* stream);

/* The CRC a stripe's parity must have, from stored block CRCs alone, no
 * payload read. Group s = the words [d_grp_start[s],
 * d_grp_start[s+1]) of d_crc, or [s*k, (s+1)*k) with a null d_grp_start (then
 * 1 <= k <= 64); both ends are clamped into [0, ncrc], so whatever the array
 * holds nothing outside d_crc is read. n_s = d_len ? d_len[s] : nbytes (64-bit
 * lengths). With m = the group's size,
 *   d_want[s] = XOR of the group's words ^ (m even ? crc_extend(n_s zero bytes, seed) : 0),
 * the CRC from `seed` of the XOR of those blocks when every stored word was
 * taken from `seed`. An empty group gives the CRC of n_s zero bytes; a NULL
 * source of the call above is simply left out of its group. Behind that call
 * on the same stream with no synchronisation, photon_crc32c_verify_n(d_out,
 * d_want, ...) reports the stripes whose sources do not match their stored
 * CRCs (batch_* plus verify_n then say which source); for a rebuild,
 * verify_n(d_out, the lost block's stored word) accepts or rejects the
 * rebuilt bytes.
 * count == 0 returns 0 and touches nothing; a null d_want, a null d_crc with
 * ncrc > 0, or a null d_grp_start with k outside 1..64 gives -EINVAL ("null
 * ..."); one launch, a thread per stripe, no workspace, plain stores only:
 * capturable and replayable. */
int photon_crc32c_xor_expect_n(const uint32_t* d_crc, uint64_t ncrc, const uint64_t* d_grp_start, uint32_t k,
                               const uint64_t* d_len, uint64_t nbytes, uint64_t count, uint32_t seed,
                               uint32_t* d_want, void* stream);
int photon_crc64ecma_xor_expect_n(const uint64_t* d_crc, uint64_t ncrc, const uint64_t* d_grp_start, uint32_t k,
                                  const uint64_t* d_len, uint64_t nbytes, uint64_t count, uint64_t seed,
                                  uint64_t* d_want, void* stream);

/* Runtime shim so that Photon code drives the batches without HIP headers
 * (host code stays Photon C++; HIP stays behind this library):
 *   stream_create / _destroy / _sync: a non-blocking stream of the current
 *       device (the `stream` argument of the calls above);
 *   stream_on_complete: run fn(arg) on a runtime thread once everything
 *       enqueued on `stream` so far has finished (fn may call
 *       photon::semaphore::signal, thread/thread.h:511-520; it must not call
 *       into this library or HIP);
 *   device_alloc / _free: device memory of the current device;
 *   memcpy_async: copy n bytes between any host/device pointers, ordered on
 *       `stream` (pinned host memory for true asynchrony).
 * 0 or a negative errno-style code, as everywhere. */
int photon_crc_stream_create(void** stream);
int photon_crc_stream_destroy(void* stream);
int photon_crc_stream_sync(void* stream);
int photon_crc_stream_on_complete(void* stream, void (*fn)(void* arg), void* arg);
int photon_crc_device_alloc(void** ptr, uint64_t nbytes);
int photon_crc_device_free(void* ptr);
int photon_crc_memcpy_async(void* dst, const void* src, uint64_t nbytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* PHOTON_CRC32C_GPU_H */
