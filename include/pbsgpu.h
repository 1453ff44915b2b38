/*
 * include/pbsgpu.h — C ABI of libpbsgpu: the MI355X (gfx950) content-defined
 * chunker + per-chunk SHA-256 engine.
 *
 * This is the drop-in boundary for the reference's pxar stream path. The
 * reference (pure Go, CGO disabled) reaches the chunker only through the Go
 * package API of github.com/pbs-plus/pxar v0.34.0 (go.mod:30); the entry
 * points below are what a cgo binding inside that module's `buzhash` /
 * `backupproxy` packages would bind (INTEGRATION.md shows the stub). Every
 * declaration cites the reference interface it stands behind.
 *
 * Conventions: plain pointers and sizes only; every function returns an int
 * status (PBSGPU_OK == 0, negative = error, text via pbsgpu_strerror); opaque
 * handles; no thread-local state — a handle may be used from any OS thread
 * (cgo calls arrive on arbitrary threads). An ENGINE may be used from several
 * threads at once (submit / collect / helper calls / any number of streams and
 * chunkers created from it: the library never holds a lock across a device
 * wait or a copy, and helper calls queue for a work context instead of failing);
 * calls on ONE stream or chunker handle must be serialised by the caller, like
 * a Go writer owned by one goroutine (internal/tapeio/converter.go:672-680).
 * Streams and chunkers keep their engine alive: destroy order does not matter. Host memory passed in is never
 * retained after the call returns (cgo pointer rule): it is copied into
 * library-owned pinned staging first. Device pointers are borrowed until the
 * ticket they were submitted under has been collected.
 *
 * There is NO CPU fallback: without a usable HIP device every engine call
 * fails with PBSGPU_E_NO_DEVICE.
 */
#ifndef PBSGPU_H
#define PBSGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PBSGPU_ABI_VERSION 5

/* ---- status codes ------------------------------------------------------- */
#define PBSGPU_OK 0
#define PBSGPU_E_INVALID (-1)      /* bad argument (NULL, not a power of two, ...) */
#define PBSGPU_E_NO_DEVICE (-2)    /* no HIP device / HIP runtime error at init */
#define PBSGPU_E_HIP (-3)          /* a HIP call failed (see pbsgpu_last_hip_error) */
#define PBSGPU_E_NOMEM (-4)        /* host or device allocation failed */
#define PBSGPU_E_CAPACITY (-5)     /* caller's output buffer too small (needed size reported) */
#define PBSGPU_E_BUSY (-6)         /* pbsgpu_submit_*: all in-flight tickets used, collect one first (nothing else returns it) */
#define PBSGPU_E_TICKET (-7)       /* unknown / already collected ticket */
/* (-8 is retired: it was PBSGPU_E_DENSITY until ABI v4 — no byte content fails a call any more: candidate-dense data is
 * resolved exactly by on-demand re-scans, on every path) */
#define PBSGPU_E_STATE (-9)        /* call not valid in the handle's current state */

const char *pbsgpu_strerror(int status);
int pbsgpu_abi_version(void);
/* hipError_t of the most recent failing HIP call on this process (diagnostic). */
int pbsgpu_last_hip_error(void);
/* Number of visible HIP devices (0 when there is no GPU / no driver). */
int pbsgpu_device_count(void);

/* ---- chunker configuration ---------------------------------------------
 * Mirrors buzhash.NewConfig(avgSize int) (buzhash.Config, error) — reference
 * call sites internal/pxarmount/commit_orchestrate.go:143-149 and
 * internal/tapeio/converter.go:248 (both avg = 4 << 20), tests
 * internal/pxarmount/commit_walk_test.go:25,380 (avg = 4096).
 * Derived values follow the published Proxmox/casync chunker: window 64,
 * min = avg/4, max = avg*4, mask = 2*avg-1, break when (h & mask) >= mask-2.
 * The 256-word table is an INPUT (NULL selects the built-in casync table). */
typedef struct pbsgpu_config {
    uint32_t avg;
    uint32_t min;
    uint32_t max;
    uint32_t window;    /* 64 */
    uint32_t mask;      /* break_test_mask; must be 2^k - 1 */
    uint32_t break_min; /* break_test_minimum */
    uint32_t table[256];
} pbsgpu_config;

/* PBSGPU_E_INVALID unless avg is a power of two in [256, 2^28]
 * (the error return of buzhash.NewConfig). */
int pbsgpu_config_init(uint64_t avg, const uint32_t *table, pbsgpu_config *out);
const uint32_t *pbsgpu_default_table(void);

/* ---- records -------------------------------------------------------------
 * One record per chunk = one dynamic-index entry: datastore.ChunkInfo{End,
 * Digest} (internal/pxarmount/commit_reuse.go:105-115) plus the segment it
 * belongs to and its size (backupproxy.KnownChunkRef{Digest, Size},
 * commit_reuse.go:316-332). `end` is exclusive and relative to the start of
 * the record's segment. Records come out ordered by (segment, end). */
typedef struct pbsgpu_record {
    uint64_t end;
    uint8_t digest[32]; /* SHA-256 of the raw chunk bytes (CryptModeNone, commit_orchestrate.go:157) */
    uint32_t segment;
    uint32_t size;
} pbsgpu_record;

/* A segment is one independent stream inside the submitted byte range: fresh
 * chunker state at `offset`, forced cut at `offset + length`. One segment =
 * one archive payload stream, or the bytes between two InjectChunks calls
 * (commit_reuse.go:315-341), or one file of a many-file batch. Segments must
 * be sorted by offset and must not overlap. */
typedef struct pbsgpu_segment {
    uint64_t offset;
    uint64_t length;
} pbsgpu_segment;

/* ---- engine ---------------------------------------------------------------
 * One engine per (process, device): owns HIP streams, device work buffers and
 * pinned staging. Stands where backupproxy's session holds its chunker +
 * hasher (constructed from the Config at commit_orchestrate.go:137-149). */
typedef struct pbsgpu_engine pbsgpu_engine;

/* `device` = HIP ordinal; `inflight` = number of batches that may be in
 * flight at once (1..16; 0 -> default 2). */
int pbsgpu_engine_create(int device, const pbsgpu_config *cfg, uint32_t inflight, pbsgpu_engine **out);
/* ... with every tuning value an engine has (ABI v5). Until v4 these were process-wide PBSGPU_* environment variables,
 * read once — invisible to a host that runs two engines with different needs. 0 / 0.0 = the default everywhere. The
 * variables named in the comments still work as DEBUG overrides of whatever the caller passed (one table in engine.cpp). */
typedef struct pbsgpu_engine_options {
    uint32_t inflight;               /* batches in flight at once (1..16; 0 = 2) */
    uint32_t sha_form;               /* batch-path hash kernel: 0 = wave pairs (default), 1 = single-wave lanes, 2 = express
                                      * (two lanes per chunk). Parity tests and A/B runs; PBSGPU_SHA_MODE=lane|pair|xpair */
    uint32_t sha_slack_pct;          /* workgroup budget of a batch's hash launch over total work / longest chain, in percent
                                      * + 1 (0 = default 25 %; 1 = none); PBSGPU_SHA_SLACK_PCT */
    uint32_t sha_dense_pct;          /* work per pair lane, in percent of the longest chain, from which a batch's hash launch
                                      * takes the dense form (0 = default 150; 0xffffffff = never); PBSGPU_SHA_DENSE_PCT */
    uint64_t resolve_par_min;        /* smallest single stream whose cut chain is resolved by pointer doubling (0 = default
                                      * 64 MiB; UINT64_MAX = always the serial walk); PBSGPU_RESOLVE_PAR_MIN / _SERIAL */
    uint32_t sha_many_files_per_core;/* pbsgpu_sha256_many_pays: files in flight per host core from which a GPU batch wins
                                      * (0 = default 55); PBSGPU_SHA_MANY_FILES_PER_CORE */
    /* the engine's own page ring behind pbsgpu_stream_* (created by the first stream) */
    uint32_t stream_sha_cus;         /* CUs of its pair service (0 = default 32); PBSGPU_STREAM_SHA_CUS */
    uint32_t stream_express_cus;     /* ... of its express service (0 = default 8; 0xffffffff = none); PBSGPU_STREAM_XP_CUS */
    uint32_t stream_ring_slots;      /* ring streams (sections of all payload streams) open at once (0 = 256); PBSGPU_STREAM_RING_SLOTS */
    uint32_t stream_ctx_pool;        /* closed stream contexts kept for re-use (0 = default 8; 0xffffffff = none); PBSGPU_STREAM_CTX_POOL */
    uint32_t zstd_seq_tables;        /* how this engine's zstd encoder (pbsgpu_zstd_encode_device, pbsgpu_blob_encode2_device, the two
                                      * *_upload_new2_device calls) writes a block's sequences: 0 = predefined tables, explicit
                                      * offsets (default; `reserved0` before); 1 = repeat offsets and per-block FSE / RLE tables
                                      * where they pay: shorter frames, never longer. Any other value: PBSGPU_E_INVALID.
                                      * PBSGPU_ZSTD_SEQ_TABLES overrides. */
    double stream_ring_gib;          /* its arena (0 = default 48 GiB); PBSGPU_STREAM_RING_GIB */
    uint64_t stream_page_bytes;      /* its page size (0 = default); PBSGPU_STREAM_PAGE_BYTES */
    uint32_t zstd_window_log;        /* how far this engine's zstd encoder (the same four calls) looks for repeats: 0 = inside the
                                      * 128 KiB block (default); 17, 18, 19 = a block's matches may start up to 2^log bytes in
                                      * front of the block's first byte, within the same chunk, with a larger match table
                                      * (the first word of `reserved[4]` before). Combines freely with zstd_seq_tables. Any
                                      * other value: PBSGPU_E_INVALID. PBSGPU_ZSTD_WINDOW_LOG overrides. */
    uint32_t reserved1;
    uint64_t reserved[3];
} pbsgpu_engine_options;
int pbsgpu_engine_create_opt(int device, const pbsgpu_config *cfg, const pbsgpu_engine_options *opt /* NULL = defaults */,
                             pbsgpu_engine **out);
void pbsgpu_engine_destroy(pbsgpu_engine *eng);
int pbsgpu_engine_config(const pbsgpu_engine *eng, pbsgpu_config *out);
/* Release what the engine only holds for re-use: the page ring of its payload streams (arena of PBSGPU_STREAM_RING_GIB,
 * default 48 GiB, created by the first pbsgpu_stream_create; released only while no payload stream is alive) and the
 * parked contexts of closed streams (pinned staging). *freed_bytes = device memory that came back. Waits for the device
 * to go idle: call it between jobs. */
int pbsgpu_engine_trim(pbsgpu_engine *eng, uint64_t *freed_bytes);

/* Batch path (the data-parallel form of WriteEntryReader's chunk loop —
 * internal/pxarmount/commit_reuse.go:457, commit_walk.go:475,
 * internal/tapeio/converter.go:836): cut every segment, hash every chunk.
 * `*_device`: bytes already resident in HBM at `dptr` (borrowed until collect).
 * `*_host`: bytes in host memory, copied H2D through pinned staging.
 * Asynchronous: returns a ticket as soon as the work is enqueued. */
int pbsgpu_submit_device(pbsgpu_engine *eng, const void *dptr, uint64_t nbytes,
                         const pbsgpu_segment *segs, uint32_t nseg, uint64_t *ticket);
int pbsgpu_submit_host(pbsgpu_engine *eng, const void *hptr, uint64_t nbytes,
                       const pbsgpu_segment *segs, uint32_t nseg, uint64_t *ticket);
/* The same with SUGGESTED BOUNDARIES (the payload chunker of the Proxmox lineage: cut at a suggested offset — a file
 * start in the .ppxar stream, internal/pxarmount/commit_types.go:24-32, commit_reuse.go:265 — when the open chunk
 * would then be within [min, max]; otherwise keep scanning). suggested[suggested_index[s] .. suggested_index[s+1])
 * are the ascending boundaries of segment s, relative to its start; suggested_index has nseg + 1 entries (2 when
 * segs == NULL). Definition = the serial payload chunker fed byte by byte (oracle_payload_chunker_scan): after a
 * cut at s the next cut is the EARLIER of the hash/max cut and the first suggested b with min <= b - s <= max;
 * boundaries closer than min to s are dropped. Whether github.com/pbs-plus/pxar v0.34.0 cuts at suggested
 * boundaries is open: the plain entry points above never do. */
int pbsgpu_submit_device_suggested(pbsgpu_engine *eng, const void *dptr, uint64_t nbytes, const pbsgpu_segment *segs,
                                   uint32_t nseg, const uint64_t *suggested, const uint32_t *suggested_index,
                                   uint64_t *ticket);
int pbsgpu_submit_host_suggested(pbsgpu_engine *eng, const void *hptr, uint64_t nbytes, const pbsgpu_segment *segs,
                                 uint32_t nseg, const uint64_t *suggested, const uint32_t *suggested_index,
                                 uint64_t *ticket);
/* Which READER the suggested-boundary rule emulates. Upstream's payload chunker looks at its pending boundary once per
 * `scan` call, before the hash scan of the bytes that call brings: a boundary inside the call's buffer is cut at even
 * if a hash boundary lies EARLIER in the same buffer, while a hash boundary found by an earlier call wins. The result
 * therefore depends on how many bytes one call sees. feed_bytes = 1 (the default): byte-serial feed, the
 * feed-independent limit (the earlier position wins); N > 1: every call sees N bytes; 0: one call sees everything
 * that is left. absolute_grid = 0: the buffer grid restarts at every cut (oracle_chunk_stream_suggested's feeding
 * loop); 1: buffers end at multiples of feed_bytes from the stream start (a reader appending fixed-size reads, as a
 * Go io.Reader loop with a fixed buffer does: internal/agent/verification/handler.go:15-20 uses 256 KiB). Applies to
 * everything enqueued afterwards. Whether github.com/pbs-plus/pxar cuts at suggested boundaries at all is open. */
int pbsgpu_engine_set_suggested_feed(pbsgpu_engine *eng, uint64_t feed_bytes, int absolute_grid);
/* Block until the ticket's work is done; report its record count. */
int pbsgpu_wait(pbsgpu_engine *eng, uint64_t ticket, uint64_t *nrecords);
/* Non-blocking: *done = 1 when everything enqueued for the ticket has finished on the device (collect will not
 * wait, except for the rare density retry), 0 while it is still running. Lets a host that keeps several
 * tickets in flight collect whichever finishes first instead of first-in-first-out. */
int pbsgpu_ticket_done(pbsgpu_engine *eng, uint64_t ticket, int *done);
/* Wait, copy the records out (PBSGPU_E_CAPACITY + *nrecords if cap is too
 * small; the ticket stays valid), release the ticket. */
int pbsgpu_collect(pbsgpu_engine *eng, uint64_t ticket, pbsgpu_record *out, uint64_t cap,
                   uint64_t *nrecords);

/* Per-stage device time of a finished ticket, from HIP events recorded on the
 * stream the kernels ran on (milliseconds). */
typedef struct pbsgpu_timing {
    float h2d_ms;     /* host->device staging (0 for *_device submits) */
    float scan_ms;    /* Buzhash candidate kernel */
    float resolve_ms; /* candidate compaction + min/max resolution */
    float sha_ms;     /* SHA-256 kernel */
    float total_ms;   /* first kernel start -> records ready */
    uint64_t ncandidates;
    uint64_t nrecords;
    uint32_t retries; /* density retries taken */
    uint32_t reserved;
} pbsgpu_timing;
int pbsgpu_ticket_timing(pbsgpu_engine *eng, uint64_t ticket, pbsgpu_timing *out);

/* Kernel-level entry used by the parity tests: raw Buzhash candidates of a
 * flat device byte range, i.e. every END offset e (64 <= e <= nbytes) whose
 * 64-byte window [e-64, e) satisfies the break test, ascending. Synchronous. */
int pbsgpu_candidates_device(pbsgpu_engine *eng, const void *dptr, uint64_t nbytes,
                             uint64_t *out, uint64_t cap, uint64_t *n);

/* The resolve step alone: cut ONE stream of `stream_len` bytes from an explicit ascending list of
 * candidate END offsets (as returned by pbsgpu_candidates_device, in stream coordinates). Used when
 * one stream's candidates were found piecewise — e.g. a stream split over several GPUs, each scanning
 * its byte range and all-gathering the lists. Records come back without digests. */
int pbsgpu_resolve_candidates(pbsgpu_engine *eng, const uint64_t *cands, uint64_t ncand, uint64_t stream_len,
                              pbsgpu_record *out, uint64_t cap, uint64_t *nrecords);

/* ---- upstream-style streaming chunker --------------------------------------
 * `scan` semantics of the chunker behind buzhash.Config (Proxmox
 * ChunkerImpl::scan): consume `len` bytes; *pos = 0 when no boundary was
 * found (everything consumed), else the boundary is after data[*pos - 1] and
 * only *pos bytes were consumed (state reset). Compatibility path: the scan
 * itself runs on the GPU but is only efficient for large buffers. */
typedef struct pbsgpu_chunker pbsgpu_chunker;
int pbsgpu_chunker_create(pbsgpu_engine *eng, pbsgpu_chunker **out);
void pbsgpu_chunker_destroy(pbsgpu_chunker *c);
int pbsgpu_chunker_scan(pbsgpu_chunker *c, const void *data, size_t len, size_t *pos);
int pbsgpu_chunker_reset(pbsgpu_chunker *c);

/* ---- payload-stream writer ---------------------------------------------------
 * The seam WriteEntryReader feeds (transfer.ArchiveWriter, mocked at
 * internal/pxarmount/commit_test.go:33-67): bytes are appended to ONE
 * continuous stream; finished (end, digest) records become available as the
 * stream advances. `end` in the records is the absolute stream offset
 * (payload position: written + injected), `segment` the section (number of
 * pbsgpu_stream_cut calls before the chunk).
 * All payload streams of an engine are clients of ONE engine-owned page ring
 * (see "page ring" below): host bytes are staged in pinned memory and copied
 * straight into a reserved page; cut rounds, the persistent SHA-256 service, page-granular
 * release and record delivery are shared. `window_bytes` is accepted for
 * compatibility and ignored (rounds 1-3: bytes per private device window).
 * No byte content makes a call fail (the reference's WriteEntryReader has no content-dependent
 * error either: internal/pxarmount/commit_reuse.go:457, internal/tapeio/converter.go:836): data
 * with more candidates than a scan tile has slots (periodic / crafted: one per 128 bytes and
 * more) is resolved exactly by on-demand re-scans inside the cut round — slower for that
 * stretch, bit-identical to the serial chunker. */
typedef struct pbsgpu_stream pbsgpu_stream;
int pbsgpu_stream_create(pbsgpu_engine *eng, uint64_t window_bytes, pbsgpu_stream **out);
void pbsgpu_stream_destroy(pbsgpu_stream *s);
int pbsgpu_stream_write(pbsgpu_stream *s, const void *data, size_t len);
/* Zero-copy feed: borrow library-owned pinned memory, fill it (e.g. io.ReadFull straight from the
 * source file, the reader side of WriteEntryReader), then commit the first `len` bytes. Saves the
 * caller-buffer -> staging copy of pbsgpu_stream_write. One reservation at a time. */
int pbsgpu_stream_reserve(pbsgpu_stream *s, void **buf, size_t *cap);
int pbsgpu_stream_commit(pbsgpu_stream *s, size_t len);
/* Force a cut at the current position (InjectChunks flushes the open chunk:
 * commit_reuse.go:315-341) and skip `inject_bytes` of injected, already
 * known chunk payload in the stream offsets. */
int pbsgpu_stream_cut(pbsgpu_stream *s, uint64_t inject_bytes);
/* End of stream: the tail becomes the final chunk; returns when every record is available to poll (the serial SHA-256
 * chain of the last chunks: up to ~0.5 s at 16 MiB maximum chunks). */
int pbsgpu_stream_finish(pbsgpu_stream *s);
/* The same without the wait, for a writer that goes on with its NEXT archive while this one drains (one goroutine per
 * archive, archives back to back: internal/tapeio/converter.go:672-680): finish_begin closes the input (tail chunk cut,
 * every chunk handed to the hash jobs; later writes fail with PBSGPU_E_STATE) and returns; records keep arriving
 * through poll; pbsgpu_stream_done is non-blocking, *done = 1 once the last record can be polled. pbsgpu_stream_finish
 * after finish_begin waits for exactly that. */
int pbsgpu_stream_finish_begin(pbsgpu_stream *s);
int pbsgpu_stream_done(pbsgpu_stream *s, int *done);
/* Pop up to `cap` finished records (in stream order). */
int pbsgpu_stream_poll(pbsgpu_stream *s, pbsgpu_record *out, uint64_t cap, uint64_t *n);
/* Encoder().PayloadPosition() (commit_reuse.go:265): bytes written PLUS bytes injected so far — the coordinate
 * system of the records' `end` and of PAYLOAD_REF offsets (InjectChunks advances the position by the injected
 * sizes: keepLast_chunk_test.go mock, enc.Advance(total)). */
int pbsgpu_stream_position(const pbsgpu_stream *s, uint64_t *position);
/* Bytes handed to write/commit only (no injected bytes). */
int pbsgpu_stream_bytes_written(const pbsgpu_stream *s, uint64_t *bytes_written);
/* Suggest a chunk boundary at absolute payload position `offset` (same coordinates as pbsgpu_stream_position;
 * typically the current position = "a file starts here"). Ascending; see pbsgpu_submit_device_suggested. */
int pbsgpu_stream_suggest(pbsgpu_stream *s, uint64_t offset);

/* Per-file XXH3-64 tee of the stream (writeBackedFile: hash := xxh3.New(); tee := io.TeeReader(f, hash);
 * writer.WriteEntryReader(entry, tee, size); backedHashes[path] = hash.Sum64() — internal/pxarmount/
 * commit_reuse.go:450-461): the bytes written between begin_file and end_file are hashed ON THE DEVICE from the
 * same window the chunker reads (one H2D copy, two consumers; a file may span any number of windows). The hash is
 * reported asynchronously — with the window that holds the file's last byte — through poll_files, in file order
 * (the reference only reads backedHashes after the commit: verifyBackedFileHashes, commit_orchestrate.go:485-562). */
typedef struct pbsgpu_file_hash {
    uint64_t index; /* as returned by end_file / end_entry (0, 1, 2, ... per stream) */
    uint64_t size;
    uint64_t xxh3;  /* XXH3-64, seed 0 */
} pbsgpu_file_hash;
int pbsgpu_stream_begin_file(pbsgpu_stream *s);
int pbsgpu_stream_end_file(pbsgpu_stream *s, uint64_t *file_index);
int pbsgpu_stream_poll_files(pbsgpu_stream *s, pbsgpu_file_hash *out, uint64_t cap, uint64_t *n);
/* pxar payload entries written straight into the stream (the layout pbsgpu_payload_pack_device produces for resident
 * files): begin_entry appends the 16-byte {payload_type, 16 + content_len} header, reports the header's payload
 * position (what WriteEntryRef / PAYLOAD_REF records, commit_walk.go:455) and opens the file tee; exactly
 * content_len bytes must follow (write / reserve+commit) before end_entry (else PBSGPU_E_STATE = the Go writer's
 * unexpected EOF). write_marker appends the start (tail = 0) or tail (tail = 1) marker. fmt NULL = defaults. */
struct pbsgpu_payload_format;
int pbsgpu_stream_begin_entry(pbsgpu_stream *s, const struct pbsgpu_payload_format *fmt, uint64_t content_len,
                              uint64_t *payload_offset);
int pbsgpu_stream_end_entry(pbsgpu_stream *s, uint64_t *file_index);
int pbsgpu_stream_write_marker(pbsgpu_stream *s, const struct pbsgpu_payload_format *fmt, int tail);

/* ---- page ring: many payload streams, page-granular memory release, persistent SHA-256 service ------------------
 * The data-parallel form of the chunk loop behind WriteEntryReader for SEVERAL archives at once (one writer per
 * archive: internal/pxarmount/commit_reuse.go:457, internal/tapeio/converter.go:836) when the bytes are (or arrive)
 * in device memory. A batch submitted with pbsgpu_submit_device stays resident until its LONGEST chunk is hashed
 * (SHA-256 is serial inside a chunk: up to ~0.45 s for 16 MiB); the ring gives memory back PAGE by page:
 *   - the arena is cut into pages (>= max chunk size); a stream = pages in logical order, anywhere in the arena;
 *   - reserve / commit (or fill, the synthetic producer) hand the stream's next page to the ring; pump cuts the newly
 *     committed pages of all streams in one round on the device and feeds every cut chunk to the SHA-256 service, a
 *     persistent kernel whose lanes take the next chunk the moment they finish one;
 *   - a page is free again as soon as every chunk touching it has been READ by the service (not when a batch ends);
 *   - poll returns the stream's finished (end, digest) records in stream order; `end` is the absolute stream offset.
 * Results are bit-identical to one pbsgpu_submit_* / pbsgpu_stream_* pass over the same bytes.
 * One thread drives a ring. While the service runs, hipDeviceSynchronize / hipFree of the process block (the library's own
 * frees are parked meanwhile): call quiesce or park first. A ring that is not called at all for
 * PBSGPU_RING_IDLE_TIMEOUT_S (default 20 s) while its service has nothing to do — a writer in a blocking tape read,
 * internal/tapeio/converter.go:672-680 — loses NOTHING: the service stops on its own (a handshake with the host
 * guarantees that no chunk is left behind) and the next pump starts it again.
 * Candidate-dense data (more than one candidate per 128 bytes over a whole scan tile: a crafted short period) is cut
 * exactly like everything else: the control kernel re-scans such a tile on demand for the one candidate the cut rule needs
 * (ABI v4 failed the stream with PBSGPU_E_DENSITY). A stream is limited to 4 PiB (52-bit offsets inside a round, 12 bits
 * for the slot); PBSGPU_E_INVALID beyond. */
typedef struct pbsgpu_ring pbsgpu_ring;
typedef struct pbsgpu_ring_options {
    uint64_t arena_bytes;  /* device memory for pages; 0 = what is free minus 8 GiB */
    uint64_t page_bytes;   /* 0 = default: max chunk rounded up to whole scan tiles (16.2 MiB at avg 4 MiB) */
    uint32_t max_streams;  /* streams open at once; 0 = 64 */
    uint32_t sha_cus;      /* CUs of the SHA-256 service; 0 = three quarters of the chip (the rest runs the cut rounds) */
    uint32_t round_pages;  /* most pages one round cuts; 0 = 256 */
    uint32_t express_cus;  /* CUs of the EXPRESS service (two lanes per chunk: the SHA-256 chain of a chunk runs ~1.4x faster at
                            * ~0.65 of the throughput per CU) for the longest chunks (>= 13/16 of the maximum size: 1.3 % of
                            * the chunks of random data; PBSGPU_RING_LONG_BYTES). 0 = the default: 16 CUs out of the default
                            * service share when sha_cus is 0 too (measured: throughput unchanged, a lone 64 GiB file 15 %
                            * sooner, the drain of a burst 0.08 s shorter), none when sha_cus is given. A value given here
                            * comes ON TOP of a given sha_cus. PBSGPU_RING_XP_CUS overrides (0 = off). (`reserved` before.) */
    /* ---- ABI v5: what used to be PBSGPU_RING_* environment variables (still honoured as debug overrides: one table in
     * ring.cpp). 0 / 0.0 = the default; PBSGPU_RING_OFF where "none" must be expressible. ---- */
    uint32_t min_round_pages;  /* a round is launched as soon as this many pages wait (0 = round_pages / 4) */
    uint32_t max_inflight;     /* rounds in flight (0 = 3) */
    uint32_t long_bytes;       /* chunk size from which a chunk takes the express service (0 = 13/16 of the maximum) */
    uint32_t long_lo_bytes;    /* ... while the express pairs are mostly idle (0 = 11/16 of the maximum on bulk rings; OFF = never) */
    uint32_t long_spill;       /* long chunks waiting beyond which the pair lanes help (0 = default rule) */
    uint32_t poll_every;       /* block steps between two looks at the queue of a service wave that carries work (0 = 8..64 by chunker) */
    uint32_t flags;            /* PBSGPU_RING_F_* */
    uint32_t lanes_cus;        /* CUs of the LANES service (one lane per chunk, four independent waves per CU: ~1.1x the bytes per
                                * CU-second of the pair service, every chain ~1.8x slower) for chunks of at most short_bytes, taken
                                * out of sha_cus' share; 0 = none (`reserved0` before). PBSGPU_RING_LANES_CUS overrides. */
    double backlog_mib;        /* bytes waiting in front of the service beyond which no page is handed out (0 = 128 MiB per
                                * service CU; < 0 = no limit) */
    double lone_defer_ms;      /* how long the first rounds of bulk streams on an idle ring are cut ahead of the service (0 = 25; < 0 = never) */
    double idle_timeout_s;     /* the service stops on its own after this long without work or a call (0 = 20 s) */
    double autopark_ms;        /* > 0: the ring parks its service when nothing has been anywhere in it for this long */
    uint64_t short_bytes;      /* largest chunk the lanes service takes (0 = 3/2 of the average chunk size; first word of `reserved` before) */
    uint32_t fill_cus;         /* experiments: > 0 = while a service runs the synthetic refill is that many whole-CU workgroups on
                                * its own stream BESIDE the scan, which gets the rest of the cut side (0 = the default: refill and
                                * scan one after the other, each on the whole cut side). PBSGPU_RING_FILL_CUS overrides. (first
                                * word of `reserved` before) */
    uint32_t reserved1;
    uint64_t reserved[2];
} pbsgpu_ring_options;
#define PBSGPU_RING_OFF 0xffffffffu
#define PBSGPU_RING_F_NO_OVERLAP 1u      /* scan of round n + 1 NOT beside the control kernel of round n (one scan set) */
#define PBSGPU_RING_F_NO_STAGE 2u        /* the round's kernels read its tables from mapped host memory (rounds 3-4) */
#define PBSGPU_RING_F_NO_CUT_PRIO 4u     /* refill and scan streams at normal priority */
#define PBSGPU_RING_F_NO_SPLIT_AUTO 8u   /* the pair / express CU split does not follow the data */
#define PBSGPU_RING_F_DEFER_SERVICE 16u  /* profiling: rounds only fill the queue, quiesce runs the services alone */
#define PBSGPU_RING_F_FILL_SERIAL 32u    /* the synthetic refill in stream order behind the previous scan also while NO service runs (the default while one does) */
#define PBSGPU_RING_F_DENSE_SERVICE 64u  /* the pair service with FOUR pairs (eight waves) per CU: more bytes per CU-second, every chain slower */
#define PBSGPU_RING_F_DENSE_LANES 128u   /* the lanes service (lanes_cus) with EIGHT waves per CU: 84 instead of 77-81 chain-blocks per us and CU, 6 us per block */
#define PBSGPU_RING_F_TIER_TAG 256u      /* diagnostics: pbsgpu_ring_poll* report the queue a chunk went through in bits 28-29 of `segment` (0 main, 1 long, 2 short) */
#define PBSGPU_RING_F_HOLD_PAGES 512u    /* pages the services are done with stay with their stream until pbsgpu_ring_release (see "held pages" below) */
typedef struct pbsgpu_ring_stats {
    uint64_t page_bytes, bytes_enqueued, chunks, candidates, pages_enqueued, pages_recycled, service_bytes_last;
    uint32_t pages_total, pages_free, sha_cus, rounds, rounds_done, rounds_in_flight, streams_opened, service_launches;
    double service_ms_last;  /* duration of the most recent service launch (HIP events on its stream), set by quiesce */
    double service_ms_total;
} pbsgpu_ring_stats;
int pbsgpu_ring_create(pbsgpu_engine *eng, const pbsgpu_ring_options *opt /* NULL = defaults */, pbsgpu_ring **out);
void pbsgpu_ring_destroy(pbsgpu_ring *ring);
/* A new stream (fresh chunker state). PBSGPU_E_BUSY when max_streams are open. */
int pbsgpu_ring_open(pbsgpu_ring *ring, uint32_t *stream);
/* The stream's next page: a device pointer to write up to *cap (= page size) bytes to — by a kernel, a DMA, a peer.
 * PBSGPU_E_BUSY when no page is free right now, or when enough bytes already wait in front of the SHA-256 service
 * (committed pages not yet in a round + rounds in flight + published chunks no lane has claimed > the backlog limit,
 * default 128 MiB per service CU, PBSGPU_RING_BACKLOG_MIB, 0 = no limit): pump / poll and retry. */
int pbsgpu_ring_reserve(pbsgpu_ring *ring, uint32_t stream, void **dptr, uint64_t *cap);
/* The first nbytes of the reserved page are the stream's next bytes and are VISIBLE to the device (the producer has
 * finished). Every page but the stream's last must be full; final != 0 ends the stream (nbytes may then be 0, also
 * without a reservation). */
int pbsgpu_ring_commit(pbsgpu_ring *ring, uint32_t stream, uint64_t nbytes, int final);
/* Synthetic producer (benchmarks, parity tests): the stream's next nbytes come from the generator of
 * pbsgpu_fill_device (seed, kind) at the stream's current offset, written by the round itself. Takes as many whole
 * pages as are free: *taken bytes were accepted, call again with the rest after a pump. */
int pbsgpu_ring_fill(pbsgpu_ring *ring, uint32_t stream, uint64_t seed, uint32_t kind, uint64_t nbytes, int final,
                     uint64_t *taken);
/* Synthetic producer for EDITED streams (benchmarks: BASELINE.json configs[4], the re-chunk after byte edits, through the
 * ring): the stream's bytes are a piece table over generator 4 of pbsgpu_fill_device — kept extents of a base file and
 * newly written extents in stream order, pieces contiguous from 0, every offset and length a multiple of 16. The first
 * call hands the table over (copied), later calls pass NULL / 0 and continue; nbytes / final / *taken as pbsgpu_ring_fill. */
typedef struct pbsgpu_fill_piece {
    uint64_t dst_off; /* offset in the stream */
    uint64_t len;
    uint64_t src_off; /* generator offset the piece's first byte comes from */
    uint64_t seed;    /* generator seed (the base file's, or the new bytes') */
} pbsgpu_fill_piece;
int pbsgpu_ring_fill_pieces(pbsgpu_ring *ring, uint32_t stream, const pbsgpu_fill_piece *pieces, uint32_t npieces,
                            uint64_t nbytes, int final, uint64_t *taken);
/* Enqueue the committed pages as cut rounds, collect finished rounds and freed pages. Never blocks. */
int pbsgpu_ring_pump(pbsgpu_ring *ring);
/* Up to cap finished records of the stream, in stream order; *finished = 1 once the stream has ended and every record
 * has been handed out. */
int pbsgpu_ring_poll(pbsgpu_ring *ring, uint32_t stream, pbsgpu_record *out, uint64_t cap, uint64_t *n, int *finished);
/* The same for ANY open stream in one call (each stream's records in its own order, `segment` = stream id): for callers
 * that keep hundreds or thousands of short streams open — one per file of a many-file job (BASELINE.json configs[2]) —
 * and cannot ask each of them after every pump. Streams that have ended and handed out their last record are listed
 * once in `finished` (up to fcap per call); close them afterwards. */
int pbsgpu_ring_poll_any(pbsgpu_ring *ring, pbsgpu_record *out, uint64_t cap, uint64_t *n, uint32_t *finished, uint32_t fcap,
                         uint32_t *nfinished);
/* Release a finished, fully polled stream's slot (PBSGPU_E_STATE before that). */
int pbsgpu_ring_close(pbsgpu_ring *ring, uint32_t stream);
/* Suggested boundary (see pbsgpu_submit_device_suggested) at `offset` bytes from the stream's start; ascending; announce
 * it before the bytes around it are committed. The reader-buffer rule of pbsgpu_engine_set_suggested_feed applies. */
int pbsgpu_ring_suggest(pbsgpu_ring *ring, uint32_t stream, uint64_t offset);
/* Wait until everything enqueued is hashed and stop the service kernel (the device is then idle as far as the ring is
 * concerned); the next pump starts it again. */
int pbsgpu_ring_quiesce(pbsgpu_ring *ring);
/* The same without the wait: the service ends by itself once it has hashed what is enqueued; the next pump starts a new
 * one. For a binding that is about to sit in a blocking read, or that wants hipFree / device-wide synchronisation of the
 * process to be possible again soon. */
int pbsgpu_ring_park(pbsgpu_ring *ring);
int pbsgpu_ring_get_stats(pbsgpu_ring *ring, pbsgpu_ring_stats *out);
/* How the ring's service is laid out: CUs of the express service (0 = none) and the chunk size from which a chunk takes it. */
int pbsgpu_ring_express(pbsgpu_ring *ring, uint32_t *express_cus, uint64_t *long_bytes);
/* Which regime is the ring running in? Cumulative counters of the two SHA-256 services since pbsgpu_ring_create: one
 * wave of each service samples the shader clock and the 100 MHz wall clock once per 4096 block steps and, when it carried a
 * block in every step of the interval, adds the interval to these sums. ticks / steps x 10 = ns per block step of a chain
 * UNDER LOAD (an express step is two blocks of a chunk); cycles / ticks x 100 = the shader clock in MHz that chain ran at.
 * Read it twice and subtract to look at a phase (bench.py: feed phase and drain of the timed region -> `roofline`).
 * Safe while the service runs: the answer then comes from the newest finished cut round's status block (the control kernel
 * copies the counters there, at most one round old) and no HIP call is made beside the persistent kernels; with the service
 * stopped (after pbsgpu_ring_quiesce) the device counters are read directly. Same thread rule as every pbsgpu_ring_* call. */
typedef struct pbsgpu_ring_probe {
    uint64_t pair_steps, pair_cycles, pair_ticks;
    uint64_t express_steps, express_cycles, express_ticks;
} pbsgpu_ring_probe;
int pbsgpu_ring_get_probe(pbsgpu_ring *ring, pbsgpu_ring_probe *out);
/* Diagnostic text snapshot of the ring's device-side state (queue words, page reference counts, stream states). Debugging
 * only: it copies from the device on the null stream, which may wait for a running service's idle time-out. */
int pbsgpu_ring_debug(pbsgpu_ring *ring, char *buf, uint64_t cap);

/* ---- held pages: upload the new chunks of a ring stream (PBSGPU_RING_F_HOLD_PAGES) -------------------------------
 * Without the flag a page is free the moment the services have read every chunk that touches it: by the time a record has
 * been polled and pbsgpu_known_classify has called its chunk new, the bytes may be another page's. With the flag a page
 * the services are done with stays with its stream, under its logical index (page k = stream bytes [k * page_bytes,
 * (k + 1) * page_bytes)), until the caller releases it. The loop of an incremental writer then never takes the payload
 * off the device before it is known to be new:
 *   poll -> pbsgpu_known_classify -> pbsgpu_ring_blob_encode_device(skip = known) -> copy out / upload -> release(last end)
 * (pbsgpu_ring_upload_new_device, below the blob calls, is the two calls in the middle as one device-side call)
 * THE CALLER'S DUTY: held pages are arena pages. A holder that does not release makes reserve answer PBSGPU_E_BUSY and
 * fill take 0 bytes, exactly like a full arena; that is no error state, releasing resumes the ring. The arena must hold
 * what is between two releases (plus what is in flight). Without the flag every call below returns PBSGPU_E_STATE.
 * Same thread rule as every pbsgpu_ring_* call. */
#define PBSGPU_HAS_RING_UPLOAD 1
#define PBSGPU_RING_ANY_STREAM 0xffffffffu
/* The caller is done with the stream's bytes below offset `upto`: every page wholly below it — logical pages k with
 * (k + 1) * page_bytes <= upto — goes back to the free list, at once if the services have handed it back, otherwise the
 * moment they do. The watermark only moves forward (a lower value is a no-op) and may not pass the `end` of the last
 * record pbsgpu_ring_poll* has handed out for the stream (PBSGPU_E_INVALID). A stream's last page, when it is short, and
 * everything else it still holds go back with pbsgpu_ring_close. */
int pbsgpu_ring_release(pbsgpu_ring *ring, uint32_t stream, uint64_t upto);
/* Diagnostics: the stream offset from which bytes are still available (the watermark rounded down to a page) and the
 * number of handed-back pages the stream is holding. */
int pbsgpu_ring_held(pbsgpu_ring *ring, uint32_t stream, uint64_t *first_offset, uint32_t *pages_held);
/* Uncompressed blobs (pbsgpu_blob_encode_device: magic, CRC-32 little endian, data) of polled records, straight out of
 * the ring's pages, back to back into device memory dst. recs[i] as pbsgpu_ring_poll returned it (`end` absolute, `size`);
 * with stream == PBSGPU_RING_ANY_STREAM every record's stream is the low 28 bits of its `segment`, as
 * pbsgpu_ring_poll_any reports it. skip (n bytes, may be NULL): 1 = leave record i out (it is known). blob_off[i] = offset of
 * record i's blob in dst and crcs[i] (may be NULL) its CRC-32; both untouched for skipped records. *used = bytes written.
 * PBSGPU_E_CAPACITY when dst_cap is too small: *used is the size needed, nothing is written. PBSGPU_E_STATE, nothing
 * written, when a selected record has not been polled yet or begins below the offset pbsgpu_ring_held reports.
 * Runs on a leased stream of the engine and waits only for that: usable between pumps while the services run. */
int pbsgpu_ring_blob_encode_device(pbsgpu_ring *ring, uint32_t stream, const pbsgpu_record *recs, uint64_t n,
                                   const uint8_t *skip, void *dst, uint64_t dst_cap, uint64_t *blob_off, uint32_t *crcs,
                                   uint64_t *used);
/* The raw bytes [offset, offset + length) of the stream into device memory dst, for consumers that compress on the host
 * or want the bytes unframed; the range must be covered by polled records and begin at or above the offset
 * pbsgpu_ring_held reports (PBSGPU_E_STATE otherwise). */
int pbsgpu_ring_copy_device(pbsgpu_ring *ring, uint32_t stream, uint64_t offset, uint64_t length, void *dst);

/* ---- held pages of a payload stream: frame the new chunks of what pbsgpu_stream_write was given ------------------------
 * A payload stream (pbsgpu_stream_*, above) is a client of the engine's own page ring, and a page of that ring is free the
 * moment the SHA-256 services have read it: a writer whose bytes came from an io.Reader has nothing left to upload once
 * poll and classify call a chunk new. A stream that HOLDS keeps its pages, like a stream of a PBSGPU_RING_F_HOLD_PAGES
 * ring, until it releases them:
 *   hold -> { write -> poll -> pbsgpu_stream_upload_new2_device -> upload the blobs -> pbsgpu_stream_release(last end) }
 * Positions are payload positions — written plus injected bytes, the coordinates of pbsgpu_stream_position and of the
 * polled records' `end`. The switch is per stream; the engine's other streams are not affected, their pages go back the
 * moment the services hand them back, in the same order as before. On a stream that never called pbsgpu_stream_hold the
 * other four calls return PBSGPU_E_STATE and change nothing.
 * NEVER WAIT FOR YOURSELF. A stream call that needs a page waits, pumping, until the ring has one. A holding stream does
 * not wait for a page that only a release can bring: when the ring has no free page and no page still with the services
 * will become free as they hand it back (such a page belongs to a stream that does not hold, or lies below its stream's
 * watermark), the call returns PBSGPU_E_BUSY instead. That status is not sticky and no byte is lost:
 * pbsgpu_stream_write may have taken a prefix (pbsgpu_stream_bytes_written says how much; pass the rest again after a
 * release); a committed reservation is library memory and is taken whole; cut, finish, finish_begin, begin_entry,
 * end_entry and write_marker happen entirely or not at all. The arena (pbsgpu_engine_options::stream_ring_gib) must hold
 * what lies between two releases, plus what is in flight. Same thread rule as every pbsgpu_stream_* call. */
#define PBSGPU_HAS_STREAM_UPLOAD 1
struct pbsgpu_known;
struct pbsgpu_dedup_stats;
struct pbsgpu_encode_stats;
/* Only before the stream's first byte, marker or cut (PBSGPU_E_STATE later). A recycled stream context starts not
 * holding. Destroying a holding stream gives everything back. */
int pbsgpu_stream_hold(pbsgpu_stream *s);
/* The caller is done with the payload below position `upto`: every page wholly below it goes back to the ring, at once or
 * the moment the services hand it back. The watermark only moves forward (a lower value is a no-op) and may not pass the
 * `end` of the last record pbsgpu_stream_poll has handed out (PBSGPU_E_INVALID). A position inside an injected gap counts
 * as the end of the section in front of it. A section that lies wholly below the watermark gives back its ring slot and
 * every page, its short last page included. */
int pbsgpu_stream_release(pbsgpu_stream *s, uint64_t upto);
/* *first_position: the lowest position whose bytes are still available; *pages_held: handed-back pages the stream is
 * holding; *ring_pages_free (may be NULL): free pages of the engine's ring. */
int pbsgpu_stream_held(pbsgpu_stream *s, uint64_t *first_position, uint32_t *pages_held, uint32_t *ring_pages_free);
/* pbsgpu_ring_upload_new2_device (below: the fused calls) for records of this stream, word for word: flags 0 or
 * PBSGPU_ENCODE_F_ZSTD, the slots of the uncompressed layout, the verdict rule, PBSGPU_E_CAPACITY leaving dst and the set
 * untouched, the sizing call (dst = NULL, dst_cap = 0), one lease and one synchronisation. recs exactly as
 * pbsgpu_stream_poll returned them (`end` a payload position, `segment` the section number); a batch may span sections.
 * PBSGPU_E_STATE, nothing written: a record begins below *first_position or has not been polled yet. PBSGPU_E_INVALID: an
 * unknown section, or size > end - base of its section. The engine's other streams keep writing while the call runs. */
int pbsgpu_stream_upload_new2_device(pbsgpu_stream *s, struct pbsgpu_known *known, const pbsgpu_record *recs, uint64_t n,
                                     int insert, uint32_t flags, void *dst, uint64_t dst_cap, uint8_t *known_out,
                                     uint64_t *blob_off, uint32_t *lens, uint8_t *kinds, uint32_t *crcs, uint64_t *used,
                                     struct pbsgpu_dedup_stats *stats, struct pbsgpu_encode_stats *enc_stats);
/* The raw bytes [position, position + length) into device memory dst. The range must lie in one section, be covered by
 * polled records and begin at or above *first_position (PBSGPU_E_STATE otherwise: an injected gap has no bytes). */
int pbsgpu_stream_copy_device(pbsgpu_stream *s, uint64_t position, uint64_t length, void *dst);

/* ---- whole-stream SHA-256 batch ---------------------------------------------
 * verification.HashFile (internal/agent/verification/handler.go:36-68) and
 * extractFileHash (internal/server/verification/job.go:1273-1303) for many
 * files at once: digest[i] = SHA-256(base[segs[i].offset .. +length)). */
int pbsgpu_sha256_many_device(pbsgpu_engine *eng, const void *dptr, uint64_t nbytes,
                              const pbsgpu_segment *segs, uint32_t nseg, uint8_t *digests /* 32*nseg */);
int pbsgpu_sha256_many_host(pbsgpu_engine *eng, const void *hptr, uint64_t nbytes,
                            const pbsgpu_segment *segs, uint32_t nseg, uint8_t *digests);
/* POLICY for the two calls above. SHA-256 is serial inside a file: the GPU hashes ONE file per lane at 0.036 GiB/s
 * whatever its size, a SHA-NI host core does ~2 GiB/s, so a batch only wins with more than ~55 files in flight per
 * host core that would otherwise hash (measured). The reference's verify job keeps FOUR files in
 * flight (internal/server/verification/job.go:493): routed to the GPU it would run ~50x slower than sha256-simd.
 * *pays = 1 when a batch of `nfiles` beats `host_cores` (0 = 1) host cores, else 0 — a binding keeps the host hash
 * when it says 0 (go/pbsgpu: Engine.HashFiles returns ErrHostFaster). The hash calls themselves never refuse. */
int pbsgpu_sha256_many_pays(const pbsgpu_engine *eng, uint32_t nfiles, uint32_t host_cores, int *pays);

/* ---- whole-stream XXH3-64 batch ---------------------------------------------------
 * The per-file hash the commit path tees new file bodies through and re-checks afterwards:
 * xxh3.New() ... Sum64() (internal/pxarmount/commit_reuse.go:450-461), verifyBackedFileHashes
 * (internal/pxarmount/commit_orchestrate.go:485-562). out[i] = XXH3-64(seed 0) of segs[i]. */
int pbsgpu_xxh3_many_device(pbsgpu_engine *eng, const void *dptr, uint64_t nbytes,
                            const pbsgpu_segment *segs, uint32_t nseg, uint64_t *out /* nseg */);
int pbsgpu_xxh3_many_host(pbsgpu_engine *eng, const void *hptr, uint64_t nbytes,
                          const pbsgpu_segment *segs, uint32_t nseg, uint64_t *out);

/* ---- digest-set operations (cross-file duplicate detection) -----------------
 * Flag duplicates on the device: dup[i] = 1 when an earlier record (lower index)
 * carries the same digest; exact (all 32 bytes) and deterministic. This is the
 * known-chunk set's classify (below) against an empty set, with insert = 0.
 * Used on the all-gathered (digest, size) set of all ranks. */
typedef struct pbsgpu_dedup_stats {
    uint64_t nrecords;
    uint64_t nunique;
    uint64_t total_bytes;
    uint64_t unique_bytes;
} pbsgpu_dedup_stats;
int pbsgpu_dedup_host(pbsgpu_engine *eng, const pbsgpu_record *recs, uint64_t n, uint8_t *dup /* n, may be NULL */,
                      pbsgpu_dedup_stats *stats);
/* The same on records that already are in device memory (the receive buffer of the RCCL all-gather): the gathered set
 * never takes a host round trip. `dup` (host, may be NULL) and `stats` as above. */
int pbsgpu_dedup_device(pbsgpu_engine *eng, const void *drecs, uint64_t n, uint8_t *dup /* n, may be NULL */,
                        pbsgpu_dedup_stats *stats);

/* ---- known-chunk set (incremental dedup) ---------------------------------------------
 * The "known-chunk check" of the writer's inner loop (scan -> cut -> SHA-256 -> known-chunk check ->
 * upload -> DIDX append). A session starts from the previous snapshot's indexes (PreviousBackup,
 * commit_orchestrate.go:127-158): every digest in them, and every chunk already sent in this session, is known; only the
 * rest is uploaded, and InjectChunks refs (commit_reuse.go:315-341) are known by construction. The set lives in device
 * memory (a hash table the library grows by itself, load factor <= 1/2: 80-160 bytes per digest) and keeps its engine alive.
 * One thread per set at a time (the engine's rule); different sets may be used concurrently. A classify call beside a
 * running page-ring service does not wait for the service: its work runs on a leased stream of the engine.
 * Limits: n < 2^32 per call; the set holds fewer than 2^32 digests (PBSGPU_E_CAPACITY on an insert that would reach it). */
#define PBSGPU_HAS_KNOWN_SET 1
typedef struct pbsgpu_known pbsgpu_known;
/* `capacity` = digests expected (0 = default, 64 Ki); only sizes the first table, the set grows past it. */
int pbsgpu_known_create(pbsgpu_engine *eng, uint64_t capacity, pbsgpu_known **out);
void pbsgpu_known_destroy(pbsgpu_known *k); /* NULL: no-op */
int pbsgpu_known_count(const pbsgpu_known *k, uint64_t *n);
/* Insert every digest (idempotent): a previous snapshot's index, InjectChunks refs. Growth that fails to allocate
 * returns PBSGPU_E_NOMEM and leaves the set exactly as it was. */
int pbsgpu_known_add_host(pbsgpu_known *k, const pbsgpu_record *recs, uint64_t n);
int pbsgpu_known_add_device(pbsgpu_known *k, const void *drecs, uint64_t n); /* device records, 8-byte aligned */
/* The digests of a .didx image (datastore.ParseDynamicIndex, commit_orchestrate.go:127-158). Validates exactly what
 * pbsgpu_didx_decode validates — magic, body a multiple of 40 bytes, ascending ends — and, like it, does NOT verify the
 * index checksum. */
int pbsgpu_known_add_didx(pbsgpu_known *k, const uint8_t *didx, uint64_t nbytes);
/* known[i] = 1 when the digest of record i was in the set before the call, or an earlier record of the SAME call (j < i)
 * carries it; 0 = new (the first occurrence of a digest the set lacked: the chunk to upload). insert != 0: every new
 * digest is in the set afterwards; insert = 0: the set is unchanged. Exact (all 32 bytes) and deterministic.
 * stats: nrecords / total_bytes over all records, nunique / unique_bytes over the new ones. `known` (host) may be NULL. */
int pbsgpu_known_classify_host(pbsgpu_known *k, const pbsgpu_record *recs, uint64_t n, int insert,
                               uint8_t *known /* n, may be NULL */, pbsgpu_dedup_stats *stats);
/* The same on records in device memory (e.g. what a ring delivered into a device buffer); a host pointer: E_INVALID. */
int pbsgpu_known_classify_device(pbsgpu_known *k, const void *drecs, uint64_t n, int insert,
                                 uint8_t *known /* host, n, may be NULL */, pbsgpu_dedup_stats *stats);

/* ---- data blobs: CRC-32, upload framing and chunk verification -----------------------------------
 * The "upload" step of the writer's inner loop and the chunk check of the read side. A PBS server takes
 * a chunk as a data blob; the commit path uploads uncompressed ones (compress=false, commit_orchestrate.go:137-149):
 *   [8-byte magic | CRC-32 of the bytes after the header, little endian | chunk bytes]        (12-byte header)
 * The encrypted kinds add a 16-byte IV and a 16-byte tag (44-byte header). Each magic is the first 8 bytes of SHA-256 of
 * the kind's name ("Proxmox Backup uncompressed blob v1.0", ...); the layout is recalled from PBS data_blob.rs [EXTERNAL].
 * The read side (datastore.NewChunkStore / NewChunkStoreSource: internal/server/verification/job.go:931,
 * internal/pxar/format.go:101, commit_orchestrate.go:356) checks a chunk as PBS verification does: CRC, decoded size
 * against the index, SHA-256 against the index digest.
 * The CRC is CRC-32/ISO-HDLC (zlib crc32, Go crc32.ChecksumIEEE): reflected 0xEDB88320, init and final xor 0xFFFFFFFF.
 * Device work runs on a leased stream of the engine, so a call beside a running page-ring service does not wait for it. */
#define PBSGPU_HAS_BLOB 1
#define PBSGPU_BLOB_UNCOMPRESSED 0
#define PBSGPU_BLOB_COMPRESSED 1          /* zstd */
#define PBSGPU_BLOB_ENCRYPTED 2
#define PBSGPU_BLOB_ENCRYPTED_COMPRESSED 3
#define PBSGPU_BLOB_HEADER_SIZE 12u           /* uncompressed and compressed kinds */
#define PBSGPU_BLOB_ENCRYPTED_HEADER_SIZE 44u /* + IV[16] + tag[16] */
/* verify status per blob, in the order the checks run */
#define PBSGPU_BLOB_OK 0
#define PBSGPU_BLOB_BAD_MAGIC 1   /* unknown magic, or shorter than its header */
#define PBSGPU_BLOB_BAD_CRC 2
#define PBSGPU_BLOB_BAD_SIZE 3    /* uncompressed: data length != sizes[i] */
#define PBSGPU_BLOB_BAD_DIGEST 4  /* uncompressed: SHA-256 of the data != digests[i] */
#define PBSGPU_BLOB_CRC_ONLY 5    /* compressed or encrypted, CRC good: the content needs zstd / AES (not done here) */
#define PBSGPU_BLOB_NSTATUS 6
typedef struct pbsgpu_blob_stats {
    uint64_t count[PBSGPU_BLOB_NSTATUS]; /* blobs per status */
    uint64_t blob_bytes;                 /* sum of the blob lengths */
    uint64_t crc_bytes;                  /* bytes the CRC was computed over (every blob with a known magic and header) */
    uint64_t sha_bytes;                  /* bytes hashed (uncompressed blobs, when digests are given) */
} pbsgpu_blob_stats;
/* out = the magic of `kind` (PBSGPU_BLOB_*); host only. */
int pbsgpu_blob_magic(int kind, uint8_t out[8]);
/* zlib's crc32_combine: *out = CRC-32(A || B) from crc_a = CRC-32(A), crc_b = CRC-32(B), len_b = |B|; host only. */
int pbsgpu_crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b, uint32_t *out);
/* out[i] = CRC-32 of base[segs[i].offset .. +length) (any length, 0 included; any alignment; ranges may overlap): the
 * header CRC of each chunk the commit path uploads (commit_orchestrate.go:137-149). The _host variant stages the bytes
 * through pinned memory (the Go uploader's chunks live on the host). */
int pbsgpu_crc32_many_device(pbsgpu_engine *eng, const void *dptr, uint64_t nbytes, const pbsgpu_segment *segs,
                             uint32_t nseg, uint32_t *out /* nseg */);
int pbsgpu_crc32_many_host(pbsgpu_engine *eng, const void *hptr, uint64_t nbytes, const pbsgpu_segment *segs,
                           uint32_t nseg, uint32_t *out);
/* *nbytes = sum over segs of (12 + length): the size of their uncompressed blobs. E_INVALID on overflow; host only. */
int pbsgpu_blob_encoded_size(const pbsgpu_segment *segs, uint32_t nseg, uint64_t *nbytes);
/* The upload framing of the commit path (compress=false, commit_orchestrate.go:137-149):
 * uncompressed blob i of the chunk segs[i] of device buffer src, written to device memory dst at offsets[i]
 * (offsets[0] = 0, offsets[i + 1] = offsets[i] + 12 + length): [uncompressed magic | CRC-32 LE | bytes]. One pass: each
 * chunk byte is read once, copied and folded into its CRC. *out_len = the encoded size, always; when dst_cap is smaller,
 * E_CAPACITY and nothing is written. offsets (nseg + 1) and crcs (nseg) are host arrays and may be NULL. */
int pbsgpu_blob_encode_device(pbsgpu_engine *eng, const void *src, uint64_t src_bytes, const pbsgpu_segment *segs,
                              uint32_t nseg, void *dst, uint64_t dst_cap, uint64_t *out_len,
                              uint64_t *offsets /* nseg + 1, may be NULL */, uint32_t *crcs /* nseg, may be NULL */);
/* The chunk check of a chunk-store read (NewChunkStore: internal/server/verification/job.go:931,
 * internal/pxar/format.go:101, commit_orchestrate.go:356). Verify whole blobs blobs[i] (offset, length) inside a buffer:
 * magic and header length, then the CRC, then for uncompressed blobs the data length against sizes[i] and its SHA-256
 * against digests[32 i] (either may be NULL: that check is skipped). status[i] = the first check that failed
 * (PBSGPU_BLOB_*); stats (may be NULL) counts them.
 * The SHA-256 runs through the pbsgpu_sha256_many_* kernels and their policy applies unchanged
 * (pbsgpu_sha256_many_pays): one lane per chunk, so the batch wins with thousands of chunks, not with a handful. */
int pbsgpu_blob_verify_device(pbsgpu_engine *eng, const void *dptr, uint64_t nbytes, const pbsgpu_segment *blobs,
                              uint32_t nblob, const uint8_t *digests /* 32 * nblob, may be NULL */,
                              const uint32_t *sizes /* nblob, may be NULL */, uint8_t *status /* nblob */,
                              pbsgpu_blob_stats *stats);
int pbsgpu_blob_verify_host(pbsgpu_engine *eng, const void *hptr, uint64_t nbytes, const pbsgpu_segment *blobs,
                            uint32_t nblob, const uint8_t *digests, const uint32_t *sizes, uint8_t *status,
                            pbsgpu_blob_stats *stats);

/* ---- restore a stream from its index and data blobs ---------------------------------------------------------------
 * The read every consumer of a snapshot makes: datastore.NewChunkStore + transfer.NewChunkedReader(idx, source) /
 * NewSplitReader (internal/server/verification/job.go:931-966, internal/pxar/format.go:101-129,
 * internal/pxarmount/commit_orchestrate.go:356-368) and the 4 MiB ranged content reads of the restore client
 * (internal/pxar/client.go:236: DynamicIndexReader.ChunkFromOffset, then a partial read of the first and the last chunk).
 * The mirror image of pbsgpu_blob_encode_device: one pass reads a blob's data once, folds its CRC and stores the bytes at
 * their place in the stream, so the payload is never reassembled on the host; pbsgpu_sha256_many_device /
 * pbsgpu_xxh3_many_device over dst then give the file hashes of the verification flow.
 *
 * idx is a contiguous slice of an index (as pbsgpu_didx_decode returns it): entry i is the stream bytes
 * [idx[i].end - idx[i].size, idx[i].end), idx[i].end - idx[i].size == idx[i - 1].end for i > 0, `segment` is ignored. The
 * slice spans [S, E) = [idx[0].end - idx[0].size, idx[nidx - 1].end); S <= range_start <= range_end <= E. The blob that
 * carries entry i is blobs[blob_of[i]] (offset, length inside the device buffer, header included); blob_of NULL is the
 * identity and needs nblob == nidx. dst[0] is stream byte range_start.
 *
 * status[i] is exactly what pbsgpu_blob_verify_device reports for the single blob blobs[blob_of[i]] with
 * sizes = idx[i].size and digests = idx[i].digest (digests = NULL with check_digest = 0): the same checks in the same
 * order, the same PBSGPU_BLOB_* codes, PBSGPU_BLOB_CRC_ONLY for the compressed and encrypted kinds. Several entries may
 * name one blob; each gets the blob's status against its own size and digest.
 * The bytes of entry i inside the range go to dst + (max(start_i, range_start) - range_start) if and only if the blob has
 * the uncompressed magic, a whole header, and a data length equal to idx[i].size; they are the blob's data bytes as found,
 * whatever the CRC or the digest say afterwards (read status). An entry's part of dst is left untouched on BAD_MAGIC,
 * BAD_SIZE, CRC_ONLY, and on a BAD_CRC that hides a size mismatch. Nothing outside dst[0, range_end - range_start) is
 * written, an entry writes nothing outside its own clipped part, and entries wholly outside the range are checked and
 * write nothing. A blob referenced by k entries is read once for its CRC and hashed once (crc_bytes, sha_bytes); the
 * other k - 1 copies are made by a copy pass. Blobs no entry references are neither checked nor counted.
 * The SHA-256 runs through the pbsgpu_sha256_many_* kernels and their policy applies unchanged (pbsgpu_sha256_many_pays).
 *
 * Decided on the host before any device work, with dst untouched: PBSGPU_E_INVALID for a NULL where a value is needed, a
 * blob outside the buffer, blob_of[i] >= nblob, a slice that is not contiguous, a range outside [S, E) or reversed, a host
 * pointer for the buffer or for dst, nidx >= 2^32, dst[0, range_end - range_start) overlapping the blob buffer;
 * PBSGPU_E_CAPACITY when dst_cap < range_end - range_start. nidx == 0 or an empty range is PBSGPU_OK (with an empty range
 * the entries are still checked; dst may then be NULL).
 * Runs on one leased stream of the engine and synchronises it ONCE, at the end: kind, header length and stored CRC of
 * every blob are read on the device and nothing comes back in between. It waits only for that stream, so it is usable
 * between the pumps of a running ring. */
#define PBSGPU_HAS_BLOB_DECODE 1
typedef struct pbsgpu_decode_stats {
    uint64_t count[PBSGPU_BLOB_NSTATUS]; /* index entries per status */
    uint64_t blob_bytes;  /* lengths of the DISTINCT blobs that some entry references */
    uint64_t crc_bytes;   /* bytes a CRC was computed over: once per distinct referenced blob */
    uint64_t sha_bytes;   /* bytes hashed: once per distinct referenced uncompressed blob; 0 with check_digest = 0 */
    uint64_t out_bytes;   /* bytes written to dst */
} pbsgpu_decode_stats;
int pbsgpu_blob_decode_device(pbsgpu_engine *eng,
                              const void *blobs_dptr, uint64_t nbytes,     /* device buffer the blobs were loaded into */
                              const pbsgpu_segment *blobs, uint32_t nblob, /* blob b = [offset, offset + length) of it */
                              const pbsgpu_record *idx, uint64_t nidx,     /* host: a contiguous slice of an index */
                              const uint32_t *blob_of,                     /* nidx, host; NULL = identity */
                              uint64_t range_start, uint64_t range_end,    /* stream bytes wanted */
                              int check_digest,
                              void *dst, uint64_t dst_cap,                 /* device memory */
                              uint8_t *status /* nidx */, pbsgpu_decode_stats *stats /* may be NULL */);

/* ---- zstd frames on the device -------------------------------------------------------------------------------------
 * The chunks the stock client writes are zstd frames: the reference's main backup path shells out to
 * proxmox-backup-client (internal/server/backup/command.go), which compresses by default, so the blobs that
 * datastore.NewChunkStore + transfer.NewChunkedReader read back (internal/server/verification/job.go:931-966,
 * internal/pxar/format.go:101-129, internal/pxarmount/commit_orchestrate.go:356-368) and the ranged reads of the restore
 * client (internal/pxar/client.go:236) find behind the "zstd compressed" magic one zstd frame each (RFC 8878).
 * The decoder (pbs_plus_amd/csrc/zstd_decode.h, one source for the kernel and for the CPU build that is fuzzed) takes
 * everything a conforming encoder may put into one frame. Decisions:
 *   - the content checksum (XXH64) is parsed and accounted for, NOT verified: the blob's CRC-32 covers the compressed
 *     bytes and the index digest covers the content;
 *   - a nonzero dictionary id, a skippable frame, a second frame or trailing bytes behind the frame are UNSUPPORTED;
 *   - an offset is valid if and only if it does not reach before the frame's first output byte (the output so far is the
 *     window); a declared window size is read, not enforced and not allocated;
 *   - the decoder knows the room it may write: a declared content size above it is refused before anything is written,
 *     and no byte is stored outside it;
 *   - reading past either end of a backward bit stream, an FSE distribution that does not sum and an incomplete Huffman
 *     weight set are BAD_FRAME. */
#define PBSGPU_HAS_ZSTD_DECODE 1
#define PBSGPU_ZSTD_OK 0
#define PBSGPU_ZSTD_BAD_FRAME 1   /* malformed or truncated */
#define PBSGPU_ZSTD_BAD_SIZE 2    /* needs more room than given, or the declared content size is not what was decoded */
#define PBSGPU_ZSTD_UNSUPPORTED 3 /* dictionary, skippable frame, more than one frame, trailing bytes */
/* What the header of the frame at frame[0, nbytes) declares; returns a PBSGPU_ZSTD_* status (PBSGPU_E_INVALID for a NULL
 * frame): what a caller without an index sizes a destination with. *content_size = UINT64_MAX when the frame does not
 * declare one; *window_size = the content size for a single-segment frame. Every out pointer may be NULL. Host only. */
int pbsgpu_zstd_frame_info(const uint8_t *frame, uint64_t nbytes, uint64_t *content_size /* UINT64_MAX: not declared */,
                           uint64_t *window_size, uint32_t *header_bytes, int *has_checksum);
/* Decode many frames in one launch: frame i = src[frames[i].offset .. +length) goes to dst[out[i].offset .. ), which has
 * out[i].length bytes of room. status[i] = PBSGPU_ZSTD_*, decoded[i] (may be NULL) = the bytes produced (0 unless OK). A
 * frame writes nothing outside out[i]; on a status other than OK the contents of out[i] are unspecified; everything else
 * is untouched. Decided on the host before any device work, with dst untouched: PBSGPU_E_INVALID for a NULL where a value
 * is needed, a frame outside src, an out[i] outside dst_cap, out ranges that overlap one another or the source, a host
 * pointer for src or dst, a frame or a room of 4 GiB or more. nframe == 0 is PBSGPU_OK.
 * One wave per frame; one leased stream of the engine and ONE synchronisation of it, at the end; it waits only for that
 * stream, so it is usable between the pumps of a running ring (a call that has to grow the slot's literal scratch, 128 KiB per
 * workgroup, frees the old one first, which waits for the device: DESIGN.md §15). */
int pbsgpu_zstd_decode_device(pbsgpu_engine *eng, const void *src, uint64_t nbytes, const pbsgpu_segment *frames,
                              uint32_t nframe, const pbsgpu_segment *out /* nframe: offset and room inside dst */,
                              void *dst, uint64_t dst_cap, uint8_t *status /* nframe */,
                              uint64_t *decoded /* nframe, may be NULL */);

/* ---- zstd content checksums and whole streams ---------------------------------------------------------------------------
 * For the same call sites as above (internal/server/verification/job.go:931-966, internal/pxar/format.go:101-129,
 * internal/pxarmount/commit_orchestrate.go:356-368, internal/pxar/client.go:236) when a frame is NOT a blob of an index:
 * there no CRC-32 and no digest cover it, and the frame's own content checksum (the low 32 bits of XXH64 of the content,
 * seed 0) is all there is. pbsgpu_zstd_decode_device and pbsgpu_blob_decode2_device are unchanged: inside a restore the
 * blob's CRC covers the frame and the index digest covers the content, so the restore still does not verify the frame's
 * checksum. DESIGN.md §20. */
#define PBSGPU_HAS_ZSTD_CHECKSUM 1
#define PBSGPU_ZSTD_BAD_CHECKSUM 4 /* pbsgpu_zstd_decode2_device with F_CHECKSUM only: decoded, but not to what the frame's checksum says */
#define PBSGPU_ZSTD_F_CHECKSUM 1u
#define PBSGPU_ZSTD_F_STREAM 2u
/* out[i] = XXH64 with `seed` of dptr[segs[i].offset .. +length): the sibling of pbsgpu_xxh3_many_device. Ranges may have any
 * length (0 included) and alignment and may overlap. Argument checks as for pbsgpu_crc32_many_device and
 * pbsgpu_xxh3_many_device. Four lanes per range (pbs_plus_amd/csrc/xxh64.h); one leased stream, ONE synchronisation. */
int pbsgpu_xxh64_many_device(pbsgpu_engine *eng, const void *dptr, uint64_t nbytes, const pbsgpu_segment *segs,
                             uint32_t nseg, uint64_t seed, uint64_t *out /* nseg, host */);
/* pbsgpu_zstd_decode_device with flags. flags = 0 is that call, output for output. An unknown bit is PBSGPU_E_INVALID.
 *   PBSGPU_ZSTD_F_CHECKSUM  a frame that carries a content checksum is checked against it after everything else about the
 *       frame is OK (libzstd's order). A mismatch is PBSGPU_ZSTD_BAD_CHECKSUM with decoded[i] = 0; the contents of out[i]
 *       are then unspecified and nothing outside it is written. A frame without a checksum is unaffected.
 *   PBSGPU_ZSTD_F_STREAM    segment i is a whole zstd stream, decoded as ZSTD_decompress does it: its frames one after the
 *       other into out[i]; skippable frames (magic 0x184D2A5?, a 4-byte length) skipped; an empty segment or skippable
 *       frames alone are OK with 0 bytes. status[i] is that of the first frame that is not OK. A skippable frame cut short,
 *       trailing bytes that are no frame and an unknown magic are BAD_FRAME; only a dictionary id stays UNSUPPORTED. An
 *       offset may not reach in front of ITS OWN frame's first output byte: libzstd's one-shot call lets a later frame
 *       reach into the output of the frame before it, this call answers BAD_FRAME. A deliberate difference.
 *   With both, every frame's checksum is checked.
 * Everything else as for pbsgpu_zstd_decode_device: the refusals, one wave per segment, one leased stream, ONE
 * synchronisation, usable between the pumps of a running ring. The verdict is the device's. */
int pbsgpu_zstd_decode2_device(pbsgpu_engine *eng, const void *src, uint64_t nbytes, const pbsgpu_segment *frames,
                               uint32_t nframe, const pbsgpu_segment *out /* nframe: offset and room inside dst */,
                               void *dst, uint64_t dst_cap, uint8_t *status /* nframe */,
                               uint64_t *decoded /* nframe, may be NULL */, uint32_t flags);
/* What the headers of the stream at stream[0, nbytes) declare, for sizing a destination of pbsgpu_zstd_decode2_device with
 * F_STREAM without an index; returns a PBSGPU_ZSTD_* status as the headers alone decide it (PBSGPU_E_INVALID for a NULL
 * stream). *content_size = the sum over the frames, UINT64_MAX if any frame declares none; *nframes and *nskippable count
 * what was walked (also up to a failure); *any_checksum = 1 if a frame carries a checksum. Frame and block headers are
 * walked, nothing is decoded. Every out pointer may be NULL. Host only. */
int pbsgpu_zstd_stream_info(const uint8_t *stream, uint64_t nbytes, uint64_t *content_size /* sum; UINT64_MAX if any frame declares none */,
                            uint32_t *nframes, uint32_t *nskippable, int *any_checksum);

/* Restore with the compressed blobs decoded: pbsgpu_blob_decode_device's arguments with `int check_digest` replaced by
 * flags, and statistics with two more fields. The same call sites (internal/server/verification/job.go:931-966,
 * internal/pxar/format.go:101-129, internal/pxarmount/commit_orchestrate.go:356-368, internal/pxar/client.go:236), now for
 * the chunks internal/server/backup/command.go's client stored compressed.
 * Without PBSGPU_DECODE_F_ZSTD every output equals the old call's with check_digest = (flags & F_DIGEST), byte for byte and
 * status for status. With it, a blob of the zstd-compressed kind whose CRC is good is decoded on the device; the checks of
 * such a blob, in order: magic, header, CRC, frame, size, digest.
 *   - the CRC is bad: PBSGPU_BLOB_BAD_CRC, the blob is not decoded and its part of dst stays untouched;
 *   - the frame is PBSGPU_ZSTD_BAD_FRAME or _UNSUPPORTED: PBSGPU_BLOB_BAD_DATA;
 *   - the frame needs more room than the largest entry that names the blob, or does not produce exactly idx[i].size
 *     bytes: PBSGPU_BLOB_BAD_SIZE;
 *   - with F_DIGEST, the SHA-256 of the DECODED bytes differs from idx[i].digest: PBSGPU_BLOB_BAD_DIGEST.
 * Both encrypted kinds stay PBSGPU_BLOB_CRC_ONLY. Decoded bytes go to the entry's place in the stream: a blob whose first
 * entry inside the range lies wholly inside it (and is the largest entry naming the blob) is decoded straight into dst;
 * any other (an entry clipped by the range's ends, entries outside the range, entries of differing sizes) is decoded into
 * engine scratch and its entries' clipped parts are copied. A blob named by k entries is decoded once; a copy pass makes
 * the rest. On BAD_DATA and on a compressed BAD_SIZE the entry's own clipped part of dst is unspecified; nothing outside
 * it is written. Everything the old section promises for uncompressed blobs holds unchanged. All of it is decided on
 * the device — which blobs are compressed, the CRC verdict that gates the decode, the statuses — with ONE synchronisation
 * at the end. Argument errors as for the old call, plus PBSGPU_E_INVALID with F_ZSTD for a blob or an entry of 4 GiB or more. */
#define PBSGPU_DECODE_F_DIGEST 1u
#define PBSGPU_DECODE_F_ZSTD 2u
#define PBSGPU_BLOB_BAD_DATA 6 /* pbsgpu_blob_decode2_device only: a compressed blob whose frame is malformed or unsupported */
typedef struct pbsgpu_decode_stats2 {
    uint64_t count[8];       /* index entries per status (PBSGPU_BLOB_*, BAD_DATA included) */
    uint64_t blob_bytes;     /* as pbsgpu_decode_stats */
    uint64_t crc_bytes;
    uint64_t sha_bytes;      /* with F_ZSTD also the decoded bytes hashed, once per distinct blob */
    uint64_t out_bytes;
    uint64_t zstd_in_bytes;  /* frame bytes handed to the decoder: once per distinct compressed blob with a good CRC */
    uint64_t zstd_out_bytes; /* bytes those frames decoded to (status OK) */
} pbsgpu_decode_stats2;
int pbsgpu_blob_decode2_device(pbsgpu_engine *eng, const void *blobs_dptr, uint64_t nbytes, const pbsgpu_segment *blobs,
                               uint32_t nblob, const pbsgpu_record *idx, uint64_t nidx, const uint32_t *blob_of,
                               uint64_t range_start, uint64_t range_end, uint32_t flags, void *dst, uint64_t dst_cap,
                               uint8_t *status /* nidx */, pbsgpu_decode_stats2 *stats /* may be NULL */);

/* ---- zstd frames written on the device ------------------------------------------------------------------------------
 * The writers of the reference that compress: the tape converter's local store compresses every chunk
 * (backupproxy.NewLocalStore(storeDir, c.chunkCfg, true), internal/tapeio/converter.go:399), and its PBS store and
 * session take Compress from the command line (converter.go:410-435; the flag is cmd/bkf2pxar/main.go:33, "useful for
 * remote PBS"). The commit path does not (commit_orchestrate.go:137-149, compress=false: pbsgpu_blob_encode_device).
 * The encoder (pbs_plus_amd/csrc/zstd_encode.h, one source for the kernels and for the CPU build that runs under
 * sanitizers) writes one frame per chunk: single segment, content size declared, no dictionary, no checksum; blocks of
 * 128 KiB that are independent of one another (no match reaches before its own block, so repeats more than 128 KiB
 * apart are not found); per block RLE, raw or compressed, whichever applies first; greedy matching with a minimum match
 * of 4; Huffman literals with directly described or FSE-compressed weights. A block's sequences are written in one of
 * two ways, by the ENGINE's option pbsgpu_engine_options.zstd_seq_tables, for every call below and for the two
 * *_upload_new2_device calls alike: 0 (default), predefined sequence tables and no repeat offsets; 1, repeat offsets
 * against a history that starts unknown in every block (blocks stay independent) and per block and symbol type the
 * predefined table, RLE_Mode or an FSE table described in the block, whichever is estimated shortest, never Repeat_Mode.
 * Both find the same matches; frames of mode 1 are never longer and on text about a fifth shorter. Slots, capacities,
 * verdict rules and synchronisations do not depend on the mode; frame bytes, lens, kinds and crcs may.
 * DESIGN.md §16 has the decisions and what they cost in ratio.
 * Where the matches are looked for is the engine's second option, pbsgpu_engine_options.zstd_window_log, for the same
 * calls and in either way of writing the sequences: 0 (default), inside the block, as above; 17, 18 or 19, a long-range
 * mode in which a block's matches may start up to 2^log bytes in front of the block's first byte, within the same chunk
 * and never before the chunk's first byte, found through a table four times as large that lies in the call's scratch
 * (64 KiB per workgroup more). All of a chunk's content is on the device before its first block is encoded, so blocks
 * are still encoded independently of one another, and the frame is single-segment, so any decoder takes such offsets.
 * This mode finds a file, or a part of one, that occurs again further on in the same chunk; on content without far
 * repeats it may write a slightly LONGER frame than window 0 (a few dozen bytes either way), and it is slower. The blob
 * rule "compressed only if strictly shorter than the chunk" is unaffected, as are slots, capacities, the bound and the
 * synchronisations; a ring chunk's frame is that of pbsgpu_zstd_encode_device of the same bytes on the same engine,
 * also when its pages split it. DESIGN.md §18 has the ratios and what the mode costs. */
#define PBSGPU_HAS_ZSTD_ENCODE 1
#define PBSGPU_HAS_ZSTD_SEQ_TABLES 1
#define PBSGPU_HAS_ZSTD_WINDOW 1
/* No frame of n bytes of content is longer: the frame header, three bytes per block, the content. Host only. */
uint64_t pbsgpu_zstd_encode_bound(uint64_t n);
/* Encode many chunks in one call: chunk i = src[chunks[i].offset .. +length) becomes one frame at dst + out[i].offset, which
 * has out[i].length bytes of room. status[i] = PBSGPU_ZSTD_OK, or PBSGPU_ZSTD_BAD_SIZE when the frame needs more room
 * (a room of pbsgpu_zstd_encode_bound(length) always suffices); frame_len[i] (may be NULL) = the frame's length, 0 unless
 * OK. A frame writes nothing outside out[i]; on BAD_SIZE the contents of out[i] are unspecified. Argument checks as for
 * pbsgpu_zstd_decode_device, before any device work: PBSGPU_E_INVALID for a NULL where a value is needed, a chunk outside
 * src, an out[i] outside dst_cap, out ranges that overlap one another or the source, a host pointer for src or dst, a
 * chunk or a room of 4 GiB or more. n == 0 is PBSGPU_OK. One wave per 128 KiB block, then one workgroup per chunk that
 * puts the frame together; one leased stream and ONE synchronisation of it, at the end. */
int pbsgpu_zstd_encode_device(pbsgpu_engine *eng, const void *src, uint64_t src_bytes, const pbsgpu_segment *chunks,
                              uint32_t n, const pbsgpu_segment *out /* n: offset and room inside dst */, void *dst,
                              uint64_t dst_cap, uint8_t *status /* n */, uint64_t *frame_len /* n, may be NULL */);
/* pbsgpu_zstd_encode_device with flags, for the same writers (internal/tapeio/converter.go:399, 410-435) when the frames are
 * kept outside a blob. flags = 0 is that call. With PBSGPU_ZSTD_F_CHECKSUM the frame is that call's frame for the same
 * engine (whatever zstd_seq_tables and zstd_window_log are) with bit 2 of the frame header descriptor (byte 4) set and the
 * low 32 bits of XXH64(content, 0) behind the last block, little endian; frame_len[i] counts them, and a room of
 * pbsgpu_zstd_encode_bound2(length, flags) always suffices. The checksum is taken from the chunk's source bytes on the same
 * stream, before the frame is put together. Any other bit is PBSGPU_E_INVALID. The blob and fused upload calls write no
 * checksum: a blob's CRC-32 covers its frame. */
uint64_t pbsgpu_zstd_encode_bound2(uint64_t n, uint32_t flags);
int pbsgpu_zstd_encode2_device(pbsgpu_engine *eng, const void *src, uint64_t src_bytes, const pbsgpu_segment *chunks,
                               uint32_t n, const pbsgpu_segment *out /* n: offset and room inside dst */, void *dst,
                               uint64_t dst_cap, uint8_t *status /* n */, uint64_t *frame_len /* n, may be NULL */,
                               uint32_t flags);
/* pbsgpu_blob_encode_device with the blob's kind decided on the device. Without PBSGPU_ENCODE_F_ZSTD it is that call output
 * for output (dst, offsets, crcs), with lens[i] = 12 + length and kinds[i] = PBSGPU_BLOB_UNCOMPRESSED. With it, blob i lies
 * in the same slot [offsets[i], offsets[i] + 12 + length) that the uncompressed layout gives it, and the verdict is the one
 * of the PBS client's DataBlob encoder (data_blob.rs, recalled, not checked against a fixture: EXTERNAL): the chunk is
 * compressed, and if the frame is strictly shorter than the chunk the blob is [compressed magic | CRC-32 LE of the frame |
 * frame]; otherwise it is the uncompressed blob, byte for byte what the plain call writes. lens[i] = the blob's length
 * either way, kinds[i] = PBSGPU_BLOB_COMPRESSED or _UNCOMPRESSED. Slots are not compacted: the server takes one chunk per
 * request, so the caller sends dst + offsets[i], lens[i]; the bytes of a slot behind lens[i] are unspecified. Frame
 * lengths, CRCs and headers are all made on the device, from lengths only the device knows, with ONE synchronisation at
 * the end. offsets (nseg + 1), lens, kinds, crcs (nseg each) and stats are host arrays and may be NULL. Errors as for the
 * plain call (PBSGPU_E_CAPACITY when dst_cap is below offsets[nseg], nothing written; offsets is filled in before), plus
 * PBSGPU_E_INVALID for an unknown flag, for a chunk of 4 GiB - 12 or more (lens is 32 bits wide) and, with F_ZSTD, for a dst
 * that overlaps src (the frames are read again for their CRC). */
#define PBSGPU_ENCODE_F_ZSTD 1u
typedef struct pbsgpu_encode_stats {
    uint64_t blobs[2];       /* blobs per kind: PBSGPU_BLOB_UNCOMPRESSED, PBSGPU_BLOB_COMPRESSED */
    uint64_t blob_bytes[2];  /* sum of lens per kind */
    uint64_t chunk_bytes[2]; /* sum of the chunk lengths per kind */
    uint64_t frame_bytes;    /* frame bytes of the compressed blobs */
    uint64_t crc_bytes;      /* bytes the CRC was computed over: the payload of every blob */
} pbsgpu_encode_stats;
int pbsgpu_blob_encode2_device(pbsgpu_engine *eng, const void *src, uint64_t src_bytes, const pbsgpu_segment *segs,
                               uint32_t nseg, uint32_t flags, void *dst, uint64_t dst_cap,
                               uint64_t *offsets /* nseg + 1 */, uint32_t *lens /* nseg */, uint8_t *kinds /* nseg */,
                               uint32_t *crcs /* nseg */, pbsgpu_encode_stats *stats);

/* ---- classify and frame in one device-side call --------------------------------------------------------------------
 * The middle of the incremental writer's loop — known-chunk check, then upload framing of what is new (SURVEY.md §3A;
 * the upload of commit_orchestrate.go:137-158 behind the known-chunk check, refs of commit_reuse.go:315-341 being known by
 * construction) — without the host in between: the flags stay on the device, the encode plan is built there, and the
 * call comes back once. On success every output is what pbsgpu_known_classify_host(known, recs, n, insert, flags, stats)
 * followed by the encode over the records flagged 0 produces: blobs in record order, back to back from dst; blob_off[i]
 * and crcs[i] (may be NULL) untouched for known records; *used = bytes written; the set afterwards as classify leaves it.
 * Decided on the host before any device work, with dst and the set untouched: PBSGPU_E_INVALID / PBSGPU_E_STATE as for
 * the two calls, except that EVERY record has to be available (which ones are new is not known on the host), plus
 * PBSGPU_E_INVALID for a host dst, a chunk of 2 GiB or more, or a set of another engine than the ring's.
 * Whether the blobs fit is known only on the device: PBSGPU_E_CAPACITY when they need more than dst_cap — *used is then
 * the size needed, no byte of dst is written and the set is UNCHANGED (insert has not taken effect, or the chunks would
 * never be uploaded), while known_out and stats are valid: retry with a buffer of *used bytes for the same answer.
 * dst may be NULL with dst_cap = 0 (a sizing call). One leased stream of the engine and one synchronisation of it (two
 * when the set has to grow); waits only for that stream, so it is usable between pumps while the services run.
 * Threads: the ring's rule and the set's rule (one thread per set at a time). n < 2^32. */
#define PBSGPU_HAS_UPLOAD_NEW 1
/* classify recs against `known`, then frame the NEW ones as uncompressed blobs straight out of the ring's held pages
 * (PBSGPU_RING_F_HOLD_PAGES; recs as pbsgpu_ring_poll / _poll_any returned them, see pbsgpu_ring_blob_encode_device).
 * A chunk in two pages gets one CRC over both parts. */
int pbsgpu_ring_upload_new_device(pbsgpu_ring *ring, pbsgpu_known *known, uint32_t stream /* or PBSGPU_RING_ANY_STREAM */,
                                  const pbsgpu_record *recs /* host, as polled */, uint64_t n, int insert,
                                  void *dst, uint64_t dst_cap,
                                  uint8_t *known_out /* n, may be NULL */, uint64_t *blob_off /* n */,
                                  uint32_t *crcs /* n, may be NULL */, uint64_t *used, pbsgpu_dedup_stats *stats);
/* the same for chunks in one contiguous device buffer (the batch path): chunk i = src[chunks[i].offset .. +length),
 * framed as pbsgpu_blob_encode_device frames it; every chunks[i] must lie inside src */
int pbsgpu_known_upload_new_device(pbsgpu_known *known, const void *src, uint64_t src_bytes,
                                   const pbsgpu_record *recs /* host: the digests */, const pbsgpu_segment *chunks /* n */,
                                   uint64_t n, int insert, void *dst, uint64_t dst_cap, uint8_t *known_out,
                                   uint64_t *blob_off, uint32_t *crcs, uint64_t *used, pbsgpu_dedup_stats *stats);

/* ---- the fused calls with the blob's kind decided on the device ----------------------------------------------------------
 * The two calls above for the writers of the reference that compress (the tape converter's local store,
 * backupproxy.NewLocalStore(storeDir, c.chunkCfg, true), internal/tapeio/converter.go:399, and its PBS store and session
 * with Compress: c.cfg.Compress, converter.go:410-435): what pbsgpu_blob_encode2_device is to pbsgpu_blob_encode_device.
 * flags = 0: the call above output for output (dst, blob_off, crcs, *used, known_out, stats, the set afterwards), with
 * lens[i] = 12 + size and kinds[i] = PBSGPU_BLOB_UNCOMPRESSED for every new record.
 * flags = PBSGPU_ENCODE_F_ZSTD: blob i of a new record lies in the slot [blob_off[i], blob_off[i] + 12 + size) that the
 * uncompressed layout gives it, so *used, the capacity verdict and the sizing call (dst = NULL, dst_cap = 0) are exactly
 * those of the plain call; slots are not compacted and the bytes of a slot behind lens[i] are unspecified. The kind
 * follows pbsgpu_blob_encode2_device's rule: the chunk is compressed, and only when the frame is strictly shorter than the
 * chunk the blob is [compressed magic | CRC-32 LE of the frame | frame], the frame byte for byte the one
 * pbsgpu_zstd_encode_device makes of the chunk's bytes; otherwise it is the uncompressed blob, byte for byte. A ring chunk
 * in two pages is one chunk to the encoder. blob_off, lens, kinds and crcs (lens, kinds, crcs may be NULL) are untouched
 * for known records; enc_stats (may be NULL) as in pbsgpu_blob_encode2_device, over the new records.
 * Everything the section above promises holds: refusals are decided on the host before any device work (the ones above,
 * plus PBSGPU_E_INVALID for an unknown flag bit and, in the contiguous form with F_ZSTD, for a dst that overlaps src: the
 * frames are read again for their CRC); on PBSGPU_E_CAPACITY no byte of dst is written, no block is encoded and the set
 * is unchanged, while known_out, stats and *used are final; one leased stream and one synchronisation (two when the set
 * grows); usable between pumps while the services run. The encoder's scratch is the engine's (up to 256 MiB of blocks
 * per round and 448 KiB per workgroup); a call that has to grow it waits for the device once. */
#define PBSGPU_HAS_UPLOAD_NEW2 1
int pbsgpu_ring_upload_new2_device(pbsgpu_ring *ring, pbsgpu_known *known, uint32_t stream /* or PBSGPU_RING_ANY_STREAM */,
                                   const pbsgpu_record *recs /* host, as polled */, uint64_t n, int insert, uint32_t flags,
                                   void *dst, uint64_t dst_cap, uint8_t *known_out /* n, may be NULL */,
                                   uint64_t *blob_off /* n */, uint32_t *lens /* n */, uint8_t *kinds /* n */,
                                   uint32_t *crcs /* n, may be NULL */, uint64_t *used, pbsgpu_dedup_stats *stats,
                                   pbsgpu_encode_stats *enc_stats /* may be NULL */);
int pbsgpu_known_upload_new2_device(pbsgpu_known *known, const void *src, uint64_t src_bytes,
                                    const pbsgpu_record *recs /* host: the digests */, const pbsgpu_segment *chunks /* n */,
                                    uint64_t n, int insert, uint32_t flags, void *dst, uint64_t dst_cap,
                                    uint8_t *known_out, uint64_t *blob_off, uint32_t *lens, uint8_t *kinds, uint32_t *crcs,
                                    uint64_t *used, pbsgpu_dedup_stats *stats, pbsgpu_encode_stats *enc_stats);

/* ---- AES-256-GCM on the device --------------------------------------------------------------------------------------------
 * The cipher of the two encrypted blob kinds ([EXTERNAL] PBS data_blob.rs / crypt_config.rs: magic 8 | CRC-32 LE 4 |
 * IV 16 | tag 16 | ciphertext; AES-256-GCM, empty AAD, 16-byte tag, 16-byte IV). A datastore written by a stock
 * proxmox-backup-client with a key file holds such blobs; the reference's pxar-mount takes -keyfile "for CLI compat" and
 * drops it (cmd/pxar-mount/main.go:43, :76). With this call their payload is decrypted where it lies, on the device.
 * The format core is pbs_plus_amd/csrc/aes_gcm.h (one source for the kernels and for the CPU build that runs under
 * sanitizers); how a message is cut into pieces of 64 KiB and their partial hashes folded: DESIGN.md §21. Decisions:
 *   - the AAD is always empty and the tag 16 bytes;
 *   - an IV of 12 bytes gives J0 = IV || 0^31 1; one of 16 bytes gives J0 = GHASH(IV || 0^64 || [128]_64), whose low word is
 *     arbitrary: the 32-bit counter may wrap inside a message and does so correctly;
 *   - the tag is compared on the device over all 16 bytes without an early exit; a message whose tag is bad has the first
 *     `length` bytes of its out range ZEROED before the call returns: unauthenticated plaintext is never handed out;
 *   - the AES table is indexed by secret-dependent bytes: a timing channel that is NOT addressed here;
 *   - the key never appears in options, environment, trace output or error strings. pbsgpu_aes_key_create expands it on
 *     the host, copies the tables to device memory the key object owns, and wipes the host copy before it returns.
 * Writing encrypted blobs: pbsgpu_blob_encode3_device, below. Not here (NEXT.md): the keyed chunk digest
 * SHA-256(content || id_key), the key-file KDF, pbsgpu_blob_verify_* with a key (they keep answering
 * PBSGPU_BLOB_CRC_ONLY for encrypted blobs, as pbsgpu_blob_decode_device and pbsgpu_blob_decode2_device do), and a
 * constant-time AES. */
#define PBSGPU_HAS_AES_GCM 1
typedef struct pbsgpu_aes_key pbsgpu_aes_key;
/* The round keys, H = E_K(0) and the multiplier tables of `key` in device memory of eng's device. The key keeps the engine
 * alive until it is destroyed. PBSGPU_E_INVALID for a NULL. */
int pbsgpu_aes_key_create(pbsgpu_engine *eng, const uint8_t key[32], pbsgpu_aes_key **out);
/* Zeroes the key's device memory, then frees it (the host holds no copy). No call may be using the key. NULL is allowed. */
void pbsgpu_aes_key_destroy(pbsgpu_aes_key *k);
#define PBSGPU_AES_OK 0
#define PBSGPU_AES_BAD_TAG 1
#define PBSGPU_AES_F_ENCRYPT 1u
/* Decrypt (flags = 0) or encrypt (PBSGPU_AES_F_ENCRYPT) many messages in one call: message i =
 * src[msgs[i].offset .. +length) with the IV ivs[i * iv_len .. +iv_len) goes to dst[out[i].offset .. +msgs[i].length); the
 * rest of the room out[i] is never written. Decrypting reads tags[16 i .. +16) and sets status[i] = PBSGPU_AES_OK or
 * PBSGPU_AES_BAD_TAG (output zeroed, see above); encrypting writes the tags and sets every status to OK. The caller
 * supplies the IVs in both directions and answers for their uniqueness. Messages are independent: a bad tag, and whatever
 * bytes a message holds, leave every other message and every byte outside its own out range as they were.
 * Decided on the host before any device work, with dst untouched: PBSGPU_E_INVALID for a NULL where a value is needed,
 * iv_len other than 12 or 16, an unknown flag bit, a message outside src, an out[i] outside dst_cap or shorter than its
 * message, out ranges that overlap one another or the source, a host pointer for src or dst, a message or a room of
 * 4 GiB or more. nmsg == 0 is PBSGPU_OK.
 * One leased stream of the key's engine and ONE synchronisation of it, at the end; it waits only for that stream, so it is
 * usable between the pumps of a running ring. */
int pbsgpu_aes_gcm_many_device(pbsgpu_aes_key *k, const void *src, uint64_t nbytes,
        const pbsgpu_segment *msgs, uint32_t nmsg,
        const uint8_t *ivs /* host, iv_len * nmsg */, uint32_t iv_len /* 12 or 16 */,
        uint8_t *tags /* host, 16 * nmsg: read when decrypting, written with F_ENCRYPT */,
        const pbsgpu_segment *out /* nmsg: offset and room inside dst; room >= length */,
        void *dst, uint64_t dst_cap, uint8_t *status /* nmsg */, uint32_t flags);

/* Restore with the encrypted blobs decrypted: pbsgpu_blob_decode2_device plus a key, one flag, one status and one statistic.
 * Without PBSGPU_DECODE_F_AES it is that call, output for output, and key may be NULL. With it (key NULL, or a key of another
 * engine: PBSGPU_E_INVALID before any device work) a blob of the encrypted kind whose CRC is good is decrypted on the
 * device under `key`; one of the encrypted-compressed kind as well, if PBSGPU_DECODE_F_ZSTD is set too (its plaintext is one
 * zstd frame; without F_ZSTD such a blob stays PBSGPU_BLOB_CRC_ONLY). The checks of such a blob, in order: magic, header, CRC,
 * tag, then for the compressed kind the frame, then the size:
 *   - the CRC is bad: PBSGPU_BLOB_BAD_CRC, the blob is not decrypted and its part of dst stays untouched;
 *   - the tag is bad (a wrong key, a damaged blob): PBSGPU_BLOB_BAD_TAG. The entry's part of dst is ZERO where the blob was
 *     decrypted in place (the case in which pbsgpu_blob_decode2_device decodes a frame straight into dst: the blob's first
 *     entry inside the range lies wholly inside it and is the largest entry naming the blob) and UNTOUCHED otherwise;
 *     unauthenticated plaintext is never handed out;
 *   - the frame is malformed or unsupported: PBSGPU_BLOB_BAD_DATA;
 *   - the plaintext, or what its frame decodes to, is not exactly idx[i].size bytes: PBSGPU_BLOB_BAD_SIZE. (A plain encrypted
 *     blob longer than the largest entry naming it still has its tag checked: GHASH reads the ciphertext only.)
 * PBSGPU_DECODE_F_DIGEST is NOT applied to entries of the encrypted kinds: their index digest is the keyed
 * SHA-256(content || id_key), which this library does not compute (NEXT.md), and the tag already authenticates the content.
 * Everything pbsgpu_blob_decode2_device promises holds: the clipping at the range's ends, one decryption per distinct blob
 * with a copy pass for the other entries, nothing written outside dst[0, range_end - range_start), every verdict on the
 * device, ONE synchronisation. The plaintext of an encrypted-compressed blob lies in engine scratch, as large as the blobs
 * of the call together. pbsgpu_blob_decode_device, pbsgpu_blob_decode2_device and pbsgpu_blob_verify_* keep answering
 * PBSGPU_BLOB_CRC_ONLY for both kinds. Argument errors as for pbsgpu_blob_decode2_device with F_ZSTD, plus an unknown flag.
 * (Since PBSGPU_HAS_KEYED_DIGEST: pbsgpu_blob_decode4_device, below, is this call plus the id key, and with it the keyed
 * digest of the encrypted entries IS computed and checked. This call stays as described.) */
#define PBSGPU_DECODE_F_AES 4u
#define PBSGPU_BLOB_BAD_TAG 7 /* pbsgpu_blob_decode3_device only: an encrypted blob whose tag does not authenticate it */
typedef struct pbsgpu_decode_stats3 {
    uint64_t count[8];       /* index entries per status (PBSGPU_BLOB_*, BAD_DATA and BAD_TAG included) */
    uint64_t blob_bytes;     /* as pbsgpu_decode_stats2 */
    uint64_t crc_bytes;
    uint64_t sha_bytes;
    uint64_t out_bytes;
    uint64_t zstd_in_bytes;  /* also the frames of encrypted-compressed blobs with a good tag */
    uint64_t zstd_out_bytes;
    uint64_t aes_bytes;      /* ciphertext bytes decrypted: once per distinct encrypted blob with a good CRC */
} pbsgpu_decode_stats3;
int pbsgpu_blob_decode3_device(pbsgpu_engine *eng, const void *blobs_dptr, uint64_t nbytes, const pbsgpu_segment *blobs,
                               uint32_t nblob, const pbsgpu_record *idx, uint64_t nidx, const uint32_t *blob_of,
                               uint64_t range_start, uint64_t range_end, uint32_t flags, pbsgpu_aes_key *key /* may be NULL */,
                               void *dst, uint64_t dst_cap, uint8_t *status /* nidx */,
                               pbsgpu_decode_stats3 *stats /* may be NULL */);

/* ---- encrypted data blobs written on the device ----------------------------------------------------------------------------
 * The writer's side of the two encrypted kinds: pbsgpu_blob_encode2_device plus a key, the IVs and one flag. A caller that
 * backs up with a key file gets [magic 8 | CRC-32 LE 4 | IV 16 | tag 16 | ciphertext] per chunk without the host in between:
 * cipher, tag, CRC and header are made on one stream, from lengths only the device knows.
 * Without PBSGPU_ENCODE_F_AES the call is pbsgpu_blob_encode2_device, output for output; key and ivs are not looked at.
 * With PBSGPU_ENCODE_F_AES alone, blob i lies in the slot [offsets[i], offsets[i] + 44 + length), the slots back to back:
 * encrypted magic | CRC | ivs[16 i .. +16) | tag | AES-256-GCM(chunk) under `key`, empty AAD. The CRC covers the CIPHERTEXT
 * only (what pbsgpu_blob_decode3_device checks). lens[i] = 44 + length, kinds[i] = PBSGPU_BLOB_ENCRYPTED.
 * With PBSGPU_ENCODE_F_AES | PBSGPU_ENCODE_F_ZSTD the slots are the same; the chunk is compressed exactly as
 * pbsgpu_blob_encode2_device compresses it (the frame is byte for byte pbsgpu_zstd_encode_device's on the same engine), and
 * when the frame is strictly shorter than the chunk the blob is encrypted-compressed magic | CRC | IV | tag | E(frame),
 * lens[i] = 44 + the frame's length, kinds[i] = PBSGPU_BLOB_ENCRYPTED_COMPRESSED; otherwise it is the plain encrypted blob
 * of the chunk. Slots are not compacted; the bytes of a slot behind lens[i] are unspecified.
 * IVs. The caller supplies them, 16 bytes per blob, as the stock client's form has it and as pbsgpu_aes_gcm_many_device
 * takes them. The library keeps NO counter: a counter would not survive a session, and two sessions share one key. It does
 * refuse a call in which two of the nseg IVs are equal (PBSGPU_E_INVALID, decided on the host by a sort). Uniqueness
 * ACROSS calls under one key is the caller's to answer for: a repeated IV gives away the xor of two plaintexts and the
 * hash key. The bindings supply the default: Python draws os.urandom(16 n) for ivs=None, Go draws from crypto/rand for nil.
 * Decided on the host before any device work, with dst untouched: every refusal of pbsgpu_blob_encode2_device; an unknown
 * flag bit; with F_AES a NULL key or a key of another engine, NULL ivs, two equal IVs, a dst that overlaps src, a chunk of
 * 4 GiB - 44 or more. PBSGPU_E_CAPACITY when dst_cap is below offsets[nseg]; offsets is filled in first, as in the plain
 * call. pbsgpu_blob_encoded_size3 is that sum for either layout, host only.
 * One leased stream and ONE synchronisation, at the end. The key never appears in a trace or an error string. The AES
 * table is indexed by secret-dependent bytes: the timing channel of the section above is NOT addressed here either.
 * Still left (NEXT.md): the keyed chunk digest SHA-256(content || id_key), the key-file KDF, encryption inside the fused
 * upload calls (pbsgpu_*_upload_new2_device) and the ring (pbsgpu_ring_blob_encode_device), pbsgpu_blob_verify_* with a key. */
#define PBSGPU_HAS_BLOB_ENCRYPT 1
#define PBSGPU_ENCODE_F_AES 2u
typedef struct pbsgpu_encode_stats3 {
    uint64_t blobs[4];       /* blobs per kind, PBSGPU_BLOB_UNCOMPRESSED .. PBSGPU_BLOB_ENCRYPTED_COMPRESSED */
    uint64_t blob_bytes[4];  /* sum of lens per kind */
    uint64_t chunk_bytes[4]; /* sum of the chunk lengths per kind */
    uint64_t frame_bytes;    /* frame bytes of the two compressed kinds */
    uint64_t crc_bytes;      /* bytes the CRC was computed over: the payload of every blob */
    uint64_t aes_bytes;      /* plaintext bytes encrypted */
} pbsgpu_encode_stats3;
/* host only: the bytes dst needs for these chunks, 12 + length each without PBSGPU_ENCODE_F_AES in flags, 44 + length with */
int pbsgpu_blob_encoded_size3(const pbsgpu_segment *segs, uint32_t nseg, uint32_t flags, uint64_t *nbytes);
int pbsgpu_blob_encode3_device(pbsgpu_engine *eng, const void *src, uint64_t src_bytes, const pbsgpu_segment *segs,
                               uint32_t nseg, uint32_t flags, pbsgpu_aes_key *key /* may be NULL without F_AES */,
                               const uint8_t *ivs /* host, 16 * nseg; may be NULL without F_AES */, void *dst,
                               uint64_t dst_cap, uint64_t *offsets /* nseg + 1 */, uint32_t *lens /* nseg */,
                               uint8_t *kinds /* nseg */, uint32_t *crcs /* nseg */,
                               pbsgpu_encode_stats3 *stats /* may be NULL */);

/* ---- keyed chunk digests: SHA-256(content || id_key) -------------------------------------------------------------------------
 * A backup made with a key file names a chunk in its index by SHA-256(content || id_key): 32 secret bytes appended behind the
 * content, NOT SHA-256(content) ([EXTERNAL], recalled from the stock client's CryptConfig::compute_digest).
 * These entry points make the digest at both ends of an encrypted session the keyed one: the batch path and the whole-range
 * hash with a key, and the restore's digest check for the encrypted kinds. The hot path is the batch SHA-256 kernels
 * themselves, instantiated a second time for keyed sources: only the tail block(s) of a chunk differ (last data bytes | key |
 * 0x80 | zeros | bit length of len + 32; pbs_plus_amd/csrc/sha256_suffix.h, one function for the kernels and for the CPU
 * build that runs under sanitizers). The plain kernels are not touched.
 * The library takes the 32 bytes and derives nothing. Where they come from is UNVERIFIED [EXTERNAL]: the last 32 bytes of a
 * 64-byte key-file payload by one reading, PBKDF2-HMAC-SHA256 of the 32-byte encryption key (salt "_id_key", 10 iterations)
 * by another; the key-file KDF stays with the caller.
 * Not here (NEXT.md): keyed digests from the page ring's services and so from pbsgpu_stream_* and pbsgpu_ring_*, keyed
 * _suggested submits, pbsgpu_blob_verify_* with keys, the key-file KDF, the encrypted kinds inside the fused upload calls. */
#define PBSGPU_HAS_KEYED_DIGEST 1
typedef struct pbsgpu_id_key pbsgpu_id_key;
/* The 32 bytes of `id_key` in device memory of eng's device that the object owns; the host copy the call makes is wiped before it
 * returns. The key keeps the engine alive until it is destroyed, and never appears in options, the environment, trace output
 * or error strings. PBSGPU_E_INVALID for a NULL. */
int pbsgpu_id_key_create(pbsgpu_engine *eng, const uint8_t id_key[32], pbsgpu_id_key **out);
/* Zeroes the key's device memory, then frees it. No call may be using the key, and no ticket submitted with it may be
 * uncollected. NULL is allowed. */
void pbsgpu_id_key_destroy(pbsgpu_id_key *key);
/* pbsgpu_sha256_many_device / _host with the key: digests[32 i] = SHA-256(range i || id_key); an empty range gives the digest
 * of the key alone. The same argument checks (plus PBSGPU_E_INVALID for a NULL key), the same kernel form and dense selection
 * from the options of the key's engine, one leased stream and ONE synchronisation. */
int pbsgpu_sha256_keyed_many_device(pbsgpu_id_key *key, const void *dptr, uint64_t nbytes,
        const pbsgpu_segment *segs, uint32_t nseg, uint8_t *digests /* host, 32*nseg */);
int pbsgpu_sha256_keyed_many_host(pbsgpu_id_key *key, const void *hptr, uint64_t nbytes,
        const pbsgpu_segment *segs, uint32_t nseg, uint8_t *digests);
/* pbsgpu_submit_device / _host with every record's digest keyed. Cut points, `end`, `size` and `segment` are exactly those of
 * the plain call; only `digest` differs. The key is fixed per ticket at submit time (the re-run of a batch whose scan tiles
 * overflowed hashes with the same key); the caller keeps it alive until the ticket is collected. Plain and keyed tickets may
 * be in flight together on one engine. PBSGPU_E_INVALID for a NULL key or a key of another engine. */
int pbsgpu_submit_device_keyed(pbsgpu_engine *eng, pbsgpu_id_key *key, const void *dptr, uint64_t nbytes,
                               const pbsgpu_segment *segs, uint32_t nseg, uint64_t *ticket);
int pbsgpu_submit_host_keyed(pbsgpu_engine *eng, pbsgpu_id_key *key, const void *hptr, uint64_t nbytes,
                             const pbsgpu_segment *segs, uint32_t nseg, uint64_t *ticket);
/* pbsgpu_blob_decode3_device plus the id key. With idkey == NULL it is that call, output for output; an idkey without
 * PBSGPU_DECODE_F_AES, or without PBSGPU_DECODE_F_DIGEST, is ignored. With F_AES | F_DIGEST and an id key (of another engine:
 * PBSGPU_E_INVALID before any device work), an entry whose blob is of an encrypted kind and has passed magic, header, CRC, tag,
 * frame and size is checked against idx[i].digest == SHA-256(plaintext content || id_key); a mismatch gives
 * PBSGPU_BLOB_BAD_DIGEST, so the order of the checks becomes magic, header, CRC, tag, frame, size, digest. As with every other
 * digest verdict of the restore the bytes already stored stay: the caller reads the status. Entries of the two plain kinds
 * keep the plain digest. The keyed hash runs once per distinct encrypted blob over the plaintext where the AES leg or its
 * frame decode left it, the comparison is made on the device, stats->sha_bytes counts these bytes, and there is still ONE
 * synchronisation. */
int pbsgpu_blob_decode4_device(pbsgpu_engine *eng, const void *blobs_dptr, uint64_t nbytes, const pbsgpu_segment *blobs,
                               uint32_t nblob, const pbsgpu_record *idx, uint64_t nidx, const uint32_t *blob_of,
                               uint64_t range_start, uint64_t range_end, uint32_t flags, pbsgpu_aes_key *key /* may be NULL */,
                               pbsgpu_id_key *idkey /* may be NULL */, void *dst, uint64_t dst_cap, uint8_t *status /* nidx */,
                               pbsgpu_decode_stats3 *stats /* may be NULL */);

/* ---- multi-GPU digest-set reduce (RCCL over xGMI) ----------------------------------
 * The path shards at file / archive granularity with no data-path collective: one engine per GPU (one process per GPU, or
 * several engines in one process) ingests its own streams. The one exchange step is the digest-set reduce for cross-file
 * duplicate detection: ONE RCCL all-gather of fixed-size slots [count | records] + the device dedup.
 * A Go host (one session per process, pure Go: internal/tapeio/converter.go:396-439) binds this directly — no Python, no
 * torch: rank 0 asks for a unique id, ships its 128 bytes to the other ranks over the channel it already has (the
 * agent's aRPC session), every rank creates its communicator, and every rank calls the reduce in the same order.
 * RCCL is resolved at run time (dlopen): a single-GPU host never loads it; PBSGPU_E_NO_DEVICE when it is not installed. */
#define PBSGPU_COMM_ID_BYTES 128
typedef struct pbsgpu_comm pbsgpu_comm;
int pbsgpu_comm_unique_id(uint8_t id[PBSGPU_COMM_ID_BYTES]);
/* Collective over `world` ranks (blocks until all of them have called it). The communicator keeps its engine alive. */
int pbsgpu_comm_create(pbsgpu_engine *eng, const uint8_t id[PBSGPU_COMM_ID_BYTES], int rank, int world, pbsgpu_comm **out);
void pbsgpu_comm_destroy(pbsgpu_comm *comm);
int pbsgpu_comm_rank(const pbsgpu_comm *comm, int *rank, int *world);
/* What RCCL reported when a pbsgpu_comm_* call of this process last failed ("" = nothing yet), e.g.
 * "ncclCommInitRank: unhandled system error (ncclResult 2)". The pointer stays valid for the calling thread. */
const char *pbsgpu_comm_last_error(void);
/* Collective. recs[0..n) (HOST or DEVICE memory — device records travel device to device —, n <= cap_records) = this rank's
 * records; cap_records must be the SAME on every
 * rank (bytes per rank / minimum chunk size is a bound every rank can compute). *stats describes the union over all
 * ranks and is identical on every rank; dup_own[i] (may be NULL) = 1 when an earlier record of the union — a lower rank's,
 * or this rank's with a lower index — carries the same digest. ~48 B per chunk travel: 12 MB per TiB of corpus.
 * Errors are collective too: bad arguments (n > cap_records, recs NULL with n > 0), capacities that differ between ranks or
 * an allocation that fails on ONE rank make EVERY rank return that error from this call — the ranks agree over two 64-byte
 * all-gathers before the large one, so no rank is left waiting inside it. (Only comm / stats NULL fail locally.) */
int pbsgpu_digest_allgather_dedup(pbsgpu_comm *comm, const pbsgpu_record *recs, uint64_t n, uint64_t cap_records,
                                  uint8_t *dup_own /* n, may be NULL */, pbsgpu_dedup_stats *stats);
/* One stream split over the ranks (BASELINE.json configs[1] at N > 1 when the stream is larger than one GPU's memory;
 * rounds 2-5 had this in Python only). pbsgpu_split_plan is arithmetic: rank `rank` of `world` OWNS [*own_start, *own_end)
 * and must HOLD [*lo, *hi) in device memory — 63 bytes of window halo to the left, one maximum chunk to the right.
 * pbsgpu_comm_split_stream is collective: `local` = device pointer to this rank's bytes [lo, hi); every rank scans its own
 * bytes, the candidate END offsets and later the digests are all-gathered (two small exchanges, errors collective as
 * above), the cut chain is resolved identically everywhere, each rank hashes the chunks that START in its range.
 * out[0 .. *nrecords) = the WHOLE stream's records in stream order, identical on every rank. */
int pbsgpu_split_plan(uint64_t total_len, int world, int rank, uint32_t max_chunk, uint64_t *own_start, uint64_t *own_end,
                      uint64_t *lo, uint64_t *hi);
int pbsgpu_comm_split_stream(pbsgpu_comm *comm, const void *local, uint64_t total_len, pbsgpu_record *out, uint64_t cap,
                             uint64_t *nrecords);

/* ---- dynamic index (.didx) encoding ------------------------------------------
 * On-disk form of the record list: datastore.NewDynamicIndexWriter(ctime)
 * .Add(end, digest).Finish() / datastore.ParseDynamicIndex
 * (internal/pxarmount/commit_bottleneck_test.go:773-793,
 * commit_orchestrate.go:219). 4096-byte header + 40-byte entries. */
#define PBSGPU_DIDX_HEADER_SIZE 4096u
int pbsgpu_didx_size(uint64_t nrecords, uint64_t *nbytes);
int pbsgpu_didx_encode(pbsgpu_engine *eng, const pbsgpu_record *recs, uint64_t n, const uint8_t uuid[16],
                       int64_t ctime, uint8_t *out, uint64_t cap);
int pbsgpu_didx_decode(const uint8_t *in, uint64_t nbytes, pbsgpu_record *out, uint64_t cap, uint64_t *n,
                       int64_t *ctime, uint8_t index_csum[32]);

/* ---- payload-stream assembly ----------------------------------------------------
 * The step before the chunker: the .ppxar payload stream WriteEntryReader appends to
 * (one continuous stream per archive, files separated by format.HeaderSize = 16-byte
 * headers: internal/pxarmount/commit_types.go:24-32 rangeEnd = offset + FileSize +
 * format.HeaderSize; keepLast_chunk_test.go:105). Layout written to `dst`:
 *   [start marker {start_type, 16}]  { [{payload_type, 16 + len_i}] [file i bytes] }*  [tail {tail_type, 16}]
 * Each header is {type u64 LE, full size u64 LE}. The three type constants default to the
 * pxar v2 values (EXTERNAL, injectable). payload_offsets[i] = stream offset of file i's
 * header = what WriteEntryRef / PAYLOAD_REF records (commit_walk.go:455). */
typedef struct pbsgpu_payload_format {
    uint64_t payload_type;  /* PXAR_PAYLOAD */
    uint64_t start_type;    /* PXAR_PAYLOAD_START_MARKER */
    uint64_t tail_type;     /* PXAR_PAYLOAD_TAIL_MARKER */
    uint32_t with_start;    /* emit the start marker */
    uint32_t with_tail;     /* emit the tail marker */
} pbsgpu_payload_format;
int pbsgpu_payload_format_default(pbsgpu_payload_format *out);
int pbsgpu_payload_size(const pbsgpu_segment *files, uint32_t nfiles, const pbsgpu_payload_format *fmt,
                        uint64_t *nbytes);
int pbsgpu_payload_pack_device(pbsgpu_engine *eng, const void *src, uint64_t src_bytes, const pbsgpu_segment *files,
                               uint32_t nfiles, const pbsgpu_payload_format *fmt, void *dst, uint64_t dst_cap,
                               uint64_t *out_len, uint64_t *payload_offsets /* nfiles or NULL */);

/* ---- chunk-reuse planner (host-side index arithmetic) --------------------------------
 * What the commit walk does with the PREVIOUS snapshot's dynamic index before it decides
 * to splice old chunks in (InjectChunks) or to re-feed the bytes to the chunker:
 *   lookupDynamicEntries(idx, rangeStart, rangeEnd) -> chunks, startPadding, endPadding
 *     (internal/pxarmount/commit_reuse.go:84-135; table test commit_bottleneck_test.go:795-835)
 *   shouldReuse: padding / (range + padding) <= chunkPaddingThreshold = 0.1
 *     (commit_reuse.go:152-183, commit_types.go:14; test commit_bottleneck_test.go:837-895)
 * `idx` is the record list of one stream (ascending `end`, e.g. from pbsgpu_didx_decode). */
typedef struct pbsgpu_reuse_chunk {
    uint64_t size;       /* chunk length */
    uint64_t padding;    /* bytes of the chunk outside the requested range */
    uint64_t end_offset; /* chunk end in the old payload stream */
    uint8_t digest[32];
} pbsgpu_reuse_chunk;
int pbsgpu_reuse_lookup(const pbsgpu_record *idx, uint64_t n, uint64_t range_start, uint64_t range_end,
                        pbsgpu_reuse_chunk *out, uint64_t cap, uint64_t *nchunks, uint64_t *start_padding,
                        uint64_t *end_padding);
/* saved = the chunk kept from the previous batch (keepLastChunk), or NULL. *reuse = 1/0. */
int pbsgpu_reuse_should(const pbsgpu_record *idx, uint64_t n, uint64_t range_start, uint64_t range_end,
                        const pbsgpu_reuse_chunk *saved, double threshold, int *reuse);

/* ---- synthetic corpus generator ----------------------------------------------
 * Fills device memory with the deterministic byte stream the benchmarks and
 * parity tests use (the oracle has the CPU twin). kind: 0 random, 1 zeros,
 * 2 repeating 4 KiB block, 3 random with ~30 % zero extents, 4 random from a cheap ARX generator
 * (two ChaCha quarter-rounds per 16-byte block; the page ring's refill). `stream_off`
 * and `dptr` must be 8-byte aligned. */
int pbsgpu_fill_device(pbsgpu_engine *eng, void *dptr, uint64_t stream_off, uint64_t nbytes, uint64_t seed,
                       uint32_t kind);

/* Piece-table copy inside device memory: dst[dst_off .. +len) = src[src_off .. +len) for every item (items may be
 * given in any order; destination ranges must not overlap). Builds the edited corpus of BASELINE.json configs[4]
 * (overwrite / insert / delete extents applied to a resident base corpus) without a host round trip. */
typedef struct pbsgpu_copy_item {
    uint64_t src_off;
    uint64_t dst_off;
    uint64_t len;
} pbsgpu_copy_item;
int pbsgpu_gather_device(pbsgpu_engine *eng, const void *src, uint64_t src_bytes, void *dst, uint64_t dst_bytes,
                         const pbsgpu_copy_item *items, uint32_t nitems);

/* Host -> device copy rate of this box through pinned memory, in GB/s (what bounds every host-fed entry point). */
int pbsgpu_measure_h2d(pbsgpu_engine *eng, uint64_t nbytes, double *gb_per_s);

/* Library-owned device buffers for callers without their own allocator. */
int pbsgpu_device_alloc(pbsgpu_engine *eng, uint64_t nbytes, void **dptr);
int pbsgpu_device_free(pbsgpu_engine *eng, void *dptr);
int pbsgpu_memcpy_h2d(pbsgpu_engine *eng, void *dptr, const void *hptr, uint64_t nbytes);
int pbsgpu_memcpy_d2h(pbsgpu_engine *eng, void *hptr, const void *dptr, uint64_t nbytes);

#ifdef __cplusplus
}
#endif
#endif /* PBSGPU_H */
