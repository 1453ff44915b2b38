//go:build cgo && gpuchunk

// Package pbsgpu is the cgo binding of libpbsgpu (include/pbsgpu.h), the MI355X engine that
// stands in for the chunk loop of github.com/pbs-plus/pxar (buzhash scan + per-chunk SHA-256)
// behind the writers pbs-plus drives:
//
//	internal/pxarmount/commit_orchestrate.go:143-149  buzhash.NewConfig(4 << 20) -> NewPBSStore
//	internal/tapeio/converter.go:248,399,420          buzhash.NewConfig(4 << 20) -> New{Local,PBS}Store
//	internal/pxarmount/commit_reuse.go:457            writer.WriteEntryReader(entry, tee, size)
//
// SOURCE ONLY: this image has no Go toolchain and pbs-plus builds with CGO_ENABLED=0
// (.goreleaser.yaml:30), so the binding is opt-in behind the `gpuchunk` build tag; see
// INTEGRATION.md for the replace directive and the fallback file.
package pbsgpu

/*
#cgo CFLAGS: -I${SRCDIR}/../../include
#cgo LDFLAGS: -L${SRCDIR}/../../pbs_plus_amd/lib -lpbsgpu -Wl,-rpath,${SRCDIR}/../../pbs_plus_amd/lib
#include <stdlib.h>
#include "pbsgpu.h"
*/
import "C"

import (
	"crypto/rand"
	"errors"
	"fmt"
	"io"
	"runtime"
	"unsafe"
)

// Config mirrors buzhash.Config: a plain value handed to NewPBSStore / NewLocalStore /
// BackupConfig.ChunkConfig (commit_orchestrate.go:137-149, converter.go:399-438).
type Config struct {
	AvgSize, MinSize, MaxSize, WindowSize int
	BreakTestMask, BreakTestMinimum       uint32
	c                                     C.pbsgpu_config
}

// NewConfig mirrors buzhash.NewConfig(avgSize int) (Config, error).
func NewConfig(avgSize int) (Config, error) {
	var cfg Config
	if st := C.pbsgpu_config_init(C.uint64_t(avgSize), nil, &cfg.c); st != C.PBSGPU_OK {
		return Config{}, fmt.Errorf("buzhash: invalid average chunk size %d: %s", avgSize, strerror(st))
	}
	cfg.AvgSize, cfg.MinSize, cfg.MaxSize = int(cfg.c.avg), int(cfg.c.min), int(cfg.c.max)
	cfg.WindowSize = int(cfg.c.window)
	cfg.BreakTestMask, cfg.BreakTestMinimum = uint32(cfg.c.mask), uint32(cfg.c.break_min)
	return cfg, nil
}

// WithTable injects the module's own BUZHASH table (the built-in default is the casync table).
func (c Config) WithTable(t [256]uint32) Config {
	for i, v := range t {
		c.c.table[i] = C.uint32_t(v)
	}
	return c
}

func strerror(st C.int) string { return C.GoString(C.pbsgpu_strerror(st)) }

func check(st C.int, what string) error {
	if st == C.PBSGPU_OK {
		return nil
	}
	return fmt.Errorf("pbsgpu: %s: %s (hip %d)", what, strerror(st), int(C.pbsgpu_last_hip_error()))
}

// ChunkInfo is one dynamic-index entry: datastore.ChunkInfo{End, Digest}
// (internal/pxarmount/commit_reuse.go:105-115) plus the chunk size (KnownChunkRef.Size).
type ChunkInfo struct {
	End     uint64
	Digest  [32]byte
	Segment uint32
	Size    uint32
}

// Engine owns the device state for one GPU. It may be shared by any number of goroutines: batch submits,
// helper calls and any number of Streams / Chunkers created from it run concurrently (the library holds no lock
// across device waits); one Stream or Chunker is for one goroutine at a time, like the reference's writers
// (internal/tapeio/converter.go:672-680).
type Engine struct{ h *C.pbsgpu_engine }

func NewEngine(device int, cfg Config, inflight int) (*Engine, error) {
	return NewEngineOpt(device, cfg, EngineOptions{Inflight: uint32(inflight)})
}

// EngineOptions mirrors pbsgpu_engine_options (ABI v5): every tuning value an engine has, per engine — two engines of one
// process may differ (rounds 1-5 read them from process-wide PBSGPU_* environment variables). Zero values = the defaults.
type EngineOptions struct {
	Inflight            uint32  // batches in flight at once (1..16; 0 = 2)
	ShaForm             uint32  // batch-path hash kernel: 0 wave pairs, 1 single-wave lanes, 2 express (tests, A/B)
	ShaSlackPct         uint32  // percent + 1 (0 = default)
	ShaDensePct         uint32  // 0 = default 150; ^uint32(0) = never
	ResolveParMin       uint64  // 0 = default 64 MiB; ^uint64(0) = always the serial walk
	ShaManyFilesPerCore uint32  // HashFiles policy: files in flight per host core from which the GPU wins (0 = 55)
	StreamShaCUs        uint32  // the engine's own ring behind Stream: CUs of its pair service (0 = 32)
	StreamExpressCUs    uint32  // ... of its express service (0 = 8; ^uint32(0) = none)
	StreamRingSlots     uint32  // ring streams open at once (0 = 256)
	StreamCtxPool       uint32  // closed stream contexts kept for re-use (0 = 8; ^uint32(0) = none)
	StreamRingGiB       float64 // its arena (0 = 48)
	StreamPageBytes     uint64  // its page size (0 = default)
	ZstdSeqTables       uint32  // the zstd encoder's sequences: 0 predefined tables, explicit offsets; 1 repeat offsets and per-block tables
	ZstdWindowLog       uint32  // ... and its matches: 0 inside the 128 KiB block; 17, 18, 19 up to 2^log bytes in front of the block, within the chunk
}

func NewEngineOpt(device int, cfg Config, o EngineOptions) (*Engine, error) {
	e := &Engine{}
	co := C.pbsgpu_engine_options{inflight: C.uint32_t(o.Inflight), sha_form: C.uint32_t(o.ShaForm),
		sha_slack_pct: C.uint32_t(o.ShaSlackPct), sha_dense_pct: C.uint32_t(o.ShaDensePct),
		resolve_par_min: C.uint64_t(o.ResolveParMin), sha_many_files_per_core: C.uint32_t(o.ShaManyFilesPerCore),
		stream_sha_cus: C.uint32_t(o.StreamShaCUs), stream_express_cus: C.uint32_t(o.StreamExpressCUs),
		stream_ring_slots: C.uint32_t(o.StreamRingSlots), stream_ctx_pool: C.uint32_t(o.StreamCtxPool),
		stream_ring_gib: C.double(o.StreamRingGiB), stream_page_bytes: C.uint64_t(o.StreamPageBytes),
		zstd_seq_tables: C.uint32_t(o.ZstdSeqTables), zstd_window_log: C.uint32_t(o.ZstdWindowLog)}
	if err := check(C.pbsgpu_engine_create_opt(C.int(device), &cfg.c, &co, &e.h), "engine_create"); err != nil {
		return nil, err
	}
	runtime.SetFinalizer(e, func(e *Engine) { e.Close() })
	return e, nil
}

// Close releases the handle. Streams and Chunkers created from the engine keep the device state alive until
// they are closed too (the C library reference-counts), so finalizer order does not matter.
func (e *Engine) Close() {
	runtime.SetFinalizer(e, nil)
	if e.h != nil {
		C.pbsgpu_engine_destroy(e.h)
		e.h = nil
	}
}

func toSegments(offsets, lengths []uint64) ([]C.pbsgpu_segment, error) {
	if len(offsets) != len(lengths) {
		return nil, errors.New("pbsgpu: offsets/lengths differ in length")
	}
	segs := make([]C.pbsgpu_segment, len(offsets))
	for i := range segs {
		segs[i].offset, segs[i].length = C.uint64_t(offsets[i]), C.uint64_t(lengths[i])
	}
	return segs, nil
}

func fromRecords(buf []C.pbsgpu_record, n int) []ChunkInfo {
	out := make([]ChunkInfo, n)
	for i := range out {
		out[i].End, out[i].Segment, out[i].Size = uint64(buf[i].end), uint32(buf[i].segment), uint32(buf[i].size)
		copy(out[i].Digest[:], C.GoBytes(unsafe.Pointer(&buf[i].digest[0]), 32))
	}
	return out
}

func toRecords(in []ChunkInfo) []C.pbsgpu_record {
	out := make([]C.pbsgpu_record, len(in))
	for i, ci := range in {
		out[i].end, out[i].segment, out[i].size = C.uint64_t(ci.End), C.uint32_t(ci.Segment), C.uint32_t(ci.Size)
		for b := 0; b < 32; b++ {
			out[i].digest[b] = C.uint8_t(ci.Digest[b])
		}
	}
	return out
}

// ---- batch path: many files / segments of one buffer at once (BASELINE configs[2]) -------------------------------

// Ticket identifies an asynchronous batch.
type Ticket uint64

// ErrBusy: every in-flight ticket slot is taken; Collect one first.
var ErrBusy = errors.New("pbsgpu: all in-flight tickets used")

// Submit cuts and hashes every segment buf[offsets[i] : offsets[i]+lengths[i]] as an independent stream (fresh
// chunker state, forced cut at its end). The Go slice is copied to pinned staging before the call returns.
// suggested (optional): one ascending list of suggested boundaries per segment, relative to the segment start.
func (e *Engine) Submit(buf []byte, offsets, lengths []uint64, suggested [][]uint64) (Ticket, error) {
	defer runtime.KeepAlive(e) // the finalizer must not run Close while the C call is executing
	segs, err := toSegments(offsets, lengths)
	if err != nil {
		return 0, err
	}
	var base unsafe.Pointer
	if len(buf) > 0 {
		base = unsafe.Pointer(&buf[0])
	}
	var sp *C.pbsgpu_segment
	if len(segs) > 0 {
		sp = &segs[0]
	}
	var t C.uint64_t
	var st C.int
	if suggested == nil {
		st = C.pbsgpu_submit_host(e.h, base, C.uint64_t(len(buf)), sp, C.uint32_t(len(segs)), &t)
	} else {
		nseg := len(segs)
		if nseg == 0 {
			nseg = 1
		}
		if len(suggested) != nseg {
			return 0, errors.New("pbsgpu: one suggested-boundary list per segment")
		}
		idx := make([]C.uint32_t, nseg+1)
		var flat []C.uint64_t
		for i, l := range suggested {
			for _, v := range l {
				flat = append(flat, C.uint64_t(v))
			}
			idx[i+1] = C.uint32_t(len(flat))
		}
		var fp *C.uint64_t
		if len(flat) > 0 {
			fp = &flat[0]
		}
		st = C.pbsgpu_submit_host_suggested(e.h, base, C.uint64_t(len(buf)), sp, C.uint32_t(len(segs)), fp, &idx[0], &t)
	}
	runtime.KeepAlive(buf)
	if st == C.PBSGPU_E_BUSY {
		return 0, ErrBusy
	}
	return Ticket(t), check(st, "submit_host")
}

// Done reports, without blocking, whether Collect would return at once.
func (e *Engine) Done(t Ticket) (bool, error) {
	defer runtime.KeepAlive(e) // the finalizer must not run Close while the C call is executing
	var d C.int
	err := check(C.pbsgpu_ticket_done(e.h, C.uint64_t(t), &d), "ticket_done")
	return d != 0, err
}

// Collect waits for the batch and returns its records ordered by (segment, end); the ticket is released.
func (e *Engine) Collect(t Ticket) ([]ChunkInfo, error) {
	defer runtime.KeepAlive(e) // the finalizer must not run Close while the C call is executing
	var n C.uint64_t
	if err := check(C.pbsgpu_wait(e.h, C.uint64_t(t), &n), "wait"); err != nil {
		return nil, err
	}
	buf := make([]C.pbsgpu_record, int(n)+1)
	if err := check(C.pbsgpu_collect(e.h, C.uint64_t(t), &buf[0], n, &n), "collect"); err != nil {
		return nil, err
	}
	return fromRecords(buf, int(n)), nil
}

// ---- digest set, dynamic index, reuse planner ---------------------------------------------------------------------

// DedupStats mirrors pbsgpu_dedup_stats.
type DedupStats struct{ Records, Unique, TotalBytes, UniqueBytes uint64 }

// Dedup flags every record whose digest already occurred at a lower index (device sort + compare): the digest-set
// reduce of cross-file duplicate detection, run on the all-gathered records of all GPUs.
func (e *Engine) Dedup(recs []ChunkInfo) ([]bool, DedupStats, error) {
	defer runtime.KeepAlive(e) // the finalizer must not run Close while the C call is executing
	if len(recs) == 0 {
		return nil, DedupStats{}, nil
	}
	cr := toRecords(recs)
	dup := make([]C.uint8_t, len(recs))
	var st C.pbsgpu_dedup_stats
	if err := check(C.pbsgpu_dedup_host(e.h, &cr[0], C.uint64_t(len(cr)), &dup[0], &st), "dedup_host"); err != nil {
		return nil, DedupStats{}, err
	}
	out := make([]bool, len(recs))
	for i := range out {
		out[i] = dup[i] != 0
	}
	return out, DedupStats{uint64(st.nrecords), uint64(st.nunique), uint64(st.total_bytes), uint64(st.unique_bytes)}, nil
}

// EncodeDynamicIndex is datastore.NewDynamicIndexWriter(ctime).Add(end, digest)...Finish()
// (internal/pxarmount/commit_bottleneck_test.go:773-793): the .didx image of one stream's records.
func (e *Engine) EncodeDynamicIndex(recs []ChunkInfo, uuid [16]byte, ctime int64) ([]byte, error) {
	defer runtime.KeepAlive(e) // the finalizer must not run Close while the C call is executing
	var nb C.uint64_t
	C.pbsgpu_didx_size(C.uint64_t(len(recs)), &nb)
	out := make([]byte, int(nb))
	cr := toRecords(recs)
	var rp *C.pbsgpu_record
	if len(cr) > 0 {
		rp = &cr[0]
	}
	err := check(C.pbsgpu_didx_encode(e.h, rp, C.uint64_t(len(cr)), (*C.uint8_t)(unsafe.Pointer(&uuid[0])), C.int64_t(ctime),
		(*C.uint8_t)(unsafe.Pointer(&out[0])), nb), "didx_encode")
	return out, err
}

// ParseDynamicIndex is datastore.ParseDynamicIndex (internal/pxarmount/commit_orchestrate.go:219).
func ParseDynamicIndex(blob []byte) (recs []ChunkInfo, ctime int64, csum [32]byte, err error) {
	if len(blob) == 0 {
		return nil, 0, csum, errors.New("pbsgpu: empty index")
	}
	var n C.uint64_t
	var ct C.int64_t
	st := C.pbsgpu_didx_decode((*C.uint8_t)(unsafe.Pointer(&blob[0])), C.uint64_t(len(blob)), nil, 0, &n, &ct,
		(*C.uint8_t)(unsafe.Pointer(&csum[0])))
	if st != C.PBSGPU_OK && st != C.PBSGPU_E_CAPACITY {
		return nil, 0, csum, check(st, "didx_decode")
	}
	buf := make([]C.pbsgpu_record, int(n)+1)
	if err = check(C.pbsgpu_didx_decode((*C.uint8_t)(unsafe.Pointer(&blob[0])), C.uint64_t(len(blob)), &buf[0], n, &n, &ct,
		(*C.uint8_t)(unsafe.Pointer(&csum[0]))), "didx_decode"); err != nil {
		return nil, 0, csum, err
	}
	return fromRecords(buf, int(n)), int64(ct), csum, nil
}

// ReuseChunk mirrors the chunks lookupDynamicEntries returns (internal/pxarmount/commit_reuse.go:84-135).
type ReuseChunk struct {
	Size, Padding, EndOffset uint64
	Digest                   [32]byte
}

// LookupDynamicEntries is lookupDynamicEntries(idx, rangeStart, rangeEnd).
func LookupDynamicEntries(idx []ChunkInfo, rangeStart, rangeEnd uint64) (chunks []ReuseChunk, startPadding, endPadding uint64, err error) {
	cr := toRecords(idx)
	var rp *C.pbsgpu_record
	if len(cr) > 0 {
		rp = &cr[0]
	}
	buf := make([]C.pbsgpu_reuse_chunk, len(idx)+1)
	var n, sp, ep C.uint64_t
	if err = check(C.pbsgpu_reuse_lookup(rp, C.uint64_t(len(cr)), C.uint64_t(rangeStart), C.uint64_t(rangeEnd), &buf[0],
		C.uint64_t(len(buf)), &n, &sp, &ep), "reuse_lookup"); err != nil {
		return nil, 0, 0, err
	}
	chunks = make([]ReuseChunk, int(n))
	for i := range chunks {
		chunks[i].Size, chunks[i].Padding, chunks[i].EndOffset = uint64(buf[i].size), uint64(buf[i].padding), uint64(buf[i].end_offset)
		copy(chunks[i].Digest[:], C.GoBytes(unsafe.Pointer(&buf[i].digest[0]), 32))
	}
	return chunks, uint64(sp), uint64(ep), nil
}

// ShouldReuse is shouldReuse with chunkPaddingThreshold (commit_reuse.go:152-183, commit_types.go:14).
func ShouldReuse(idx []ChunkInfo, rangeStart, rangeEnd uint64, saved *ReuseChunk, threshold float64) (bool, error) {
	cr := toRecords(idx)
	var rp *C.pbsgpu_record
	if len(cr) > 0 {
		rp = &cr[0]
	}
	var sv *C.pbsgpu_reuse_chunk
	var tmp C.pbsgpu_reuse_chunk
	if saved != nil {
		tmp.size, tmp.padding, tmp.end_offset = C.uint64_t(saved.Size), C.uint64_t(saved.Padding), C.uint64_t(saved.EndOffset)
		for b := 0; b < 32; b++ {
			tmp.digest[b] = C.uint8_t(saved.Digest[b])
		}
		sv = &tmp
	}
	var r C.int
	err := check(C.pbsgpu_reuse_should(rp, C.uint64_t(len(cr)), C.uint64_t(rangeStart), C.uint64_t(rangeEnd), sv,
		C.double(threshold), &r), "reuse_should")
	return r != 0, err
}

// ---- payload-stream writer -----------------------------------------------------------------------------------------

// Stream is the payload-stream seam WriteEntryReader feeds: Write appends bytes, Poll returns
// finished (end, digest) entries in stream order, Inject mirrors ArchiveWriter.InjectChunks
// (commit_reuse.go:315-341: the open chunk is flushed, offsets skip the injected payload).
type Stream struct {
	h   *C.pbsgpu_stream
	eng *Engine // keeps the Go handle reachable while the stream lives
	// OnBusy, for a stream that holds its pages (Hold): called when a call needs a page and only a Release can bring one.
	// It polls, uploads and releases (Poll -> UploadNew2 -> Release); the call that met the full ring then goes on where
	// it stood. With OnBusy nil such a call returns ErrBusy.
	OnBusy func() error
}

// busy runs call until it no longer answers PBSGPU_E_BUSY, making room through OnBusy in between.
func (s *Stream) busy(what string, call func() C.int) error {
	for {
		st := call()
		if st != C.PBSGPU_E_BUSY {
			return check(st, what)
		}
		if s.OnBusy == nil {
			return ErrBusy
		}
		if err := s.OnBusy(); err != nil {
			return err
		}
	}
}

func (e *Engine) NewStream(windowBytes uint64) (*Stream, error) {
	defer runtime.KeepAlive(e) // the finalizer must not run Close while the C call is executing
	s := &Stream{eng: e}
	if err := check(C.pbsgpu_stream_create(e.h, C.uint64_t(windowBytes), &s.h), "stream_create"); err != nil {
		return nil, err
	}
	runtime.SetFinalizer(s, func(s *Stream) { s.Close() })
	return s, nil
}

// Write implements io.Writer. The Go slice is not retained: the library copies it into its own
// pinned staging before returning (cgo pointer rule).
func (s *Stream) Write(p []byte) (int, error) {
	defer runtime.KeepAlive(s) // the finalizer must not run Close while the C call is executing
	if len(p) == 0 {
		return 0, nil
	}
	var w0, w1 C.uint64_t
	C.pbsgpu_stream_bytes_written(s.h, &w0)
	st := C.pbsgpu_stream_write(s.h, unsafe.Pointer(&p[0]), C.size_t(len(p)))
	runtime.KeepAlive(p)
	if st == C.PBSGPU_E_BUSY { // a holding stream whose ring is full: a prefix was taken (io.Writer's n); Release, write the rest
		C.pbsgpu_stream_bytes_written(s.h, &w1)
		return int(w1 - w0), ErrBusy
	}
	if err := check(st, "stream_write"); err != nil {
		return 0, err
	}
	return len(p), nil
}

// ReadFrom implements io.ReaderFrom without the extra copy of Write: the reader fills the
// library's pinned staging memory directly (zero-copy feed of WriteEntryReader's io.Reader).
func (s *Stream) ReadFrom(r io.Reader) (int64, error) {
	defer runtime.KeepAlive(s) // the finalizer must not run Close while the C call is executing
	var total int64
	for {
		var buf unsafe.Pointer
		var capacity C.size_t
		if err := s.busy("stream_reserve", func() C.int { return C.pbsgpu_stream_reserve(s.h, &buf, &capacity) }); err != nil {
			return total, err
		}
		if capacity == 0 { // inside an entry whose announced size has been reached
			_ = C.pbsgpu_stream_commit(s.h, 0)
			return total, nil
		}
		n, rerr := io.ReadFull(r, unsafe.Slice((*byte)(buf), int(capacity)))
		if st := C.pbsgpu_stream_commit(s.h, C.size_t(n)); st == C.PBSGPU_E_BUSY {
			total += int64(n) // a committed reservation is taken whole; the next reserve lands it once there is room
		} else if err := check(st, "stream_commit"); err != nil {
			return total, err
		} else {
			total += int64(n)
		}
		if rerr == io.EOF || rerr == io.ErrUnexpectedEOF {
			return total, nil
		}
		if rerr != nil {
			return total, rerr
		}
	}
}

// WriteEntryReader is the payload half of ArchiveWriter.WriteEntryReader(entry, r, size): 16-byte payload header,
// exactly size bytes from r (zero-copy), per-file XXH3-64 tee. Returns the entry's payload offset (the PAYLOAD_REF /
// WriteEntryRef value, commit_walk.go:455) and the file index under which PollFiles reports the hash — what
// writeBackedFile keeps in backedHashes[path] (commit_reuse.go:450-461).
func (s *Stream) WriteEntryReader(r io.Reader, size uint64) (payloadOffset, fileIndex uint64, err error) {
	defer runtime.KeepAlive(s) // the finalizer must not run Close while the C call is executing
	var off, idx C.uint64_t
	err = s.busy("stream_begin_entry", func() C.int { return C.pbsgpu_stream_begin_entry(s.h, nil, C.uint64_t(size), &off) })
	if err != nil {
		return 0, 0, err
	}
	n, err := s.ReadFrom(io.LimitReader(r, int64(size)))
	if err != nil {
		return uint64(off), 0, err
	}
	if uint64(n) != size {
		return uint64(off), 0, io.ErrUnexpectedEOF
	}
	err = check(C.pbsgpu_stream_end_entry(s.h, &idx), "stream_end_entry")
	return uint64(off), uint64(idx), err
}

// BeginFile / EndFile bracket a file body for the XXH3 tee when the caller writes the bytes itself.
func (s *Stream) BeginFile() error {
	defer runtime.KeepAlive(s) // the finalizer must not run Close while the C call is executing
	return check(C.pbsgpu_stream_begin_file(s.h), "stream_begin_file")
}
func (s *Stream) EndFile() (uint64, error) {
	defer runtime.KeepAlive(s) // the finalizer must not run Close while the C call is executing
	var idx C.uint64_t
	err := check(C.pbsgpu_stream_end_file(s.h, &idx), "stream_end_file")
	return uint64(idx), err
}

// FileHash is one finished file of the tee.
type FileHash struct{ Index, Size, XXH3 uint64 }

func (s *Stream) PollFiles(max int) ([]FileHash, error) {
	defer runtime.KeepAlive(s) // the finalizer must not run Close while the C call is executing
	if max <= 0 {
		return nil, errors.New("pbsgpu: PollFiles(max <= 0)")
	}
	buf := make([]C.pbsgpu_file_hash, max)
	var n C.uint64_t
	if err := check(C.pbsgpu_stream_poll_files(s.h, &buf[0], C.uint64_t(max), &n), "stream_poll_files"); err != nil {
		return nil, err
	}
	out := make([]FileHash, int(n))
	for i := range out {
		out[i] = FileHash{uint64(buf[i].index), uint64(buf[i].size), uint64(buf[i].xxh3)}
	}
	return out, nil
}

// WriteMarker appends the payload start (tail = false) or tail marker.
func (s *Stream) WriteMarker(tail bool) error {
	defer runtime.KeepAlive(s) // the finalizer must not run Close while the C call is executing
	t := C.int(0)
	if tail {
		t = 1
	}
	return s.busy("stream_write_marker", func() C.int { return C.pbsgpu_stream_write_marker(s.h, nil, t) })
}

// Inject mirrors InjectChunks: forced cut, the payload position advances by the injected sizes.
func (s *Stream) Inject(injectedBytes uint64) error {
	defer runtime.KeepAlive(s) // the finalizer must not run Close while the C call is executing
	return s.busy("stream_cut", func() C.int { return C.pbsgpu_stream_cut(s.h, C.uint64_t(injectedBytes)) })
}

// PayloadPosition is Encoder().PayloadPosition() (commit_reuse.go:265): written + injected bytes.
func (s *Stream) PayloadPosition() uint64 {
	defer runtime.KeepAlive(s) // the finalizer must not run Close while the C call is executing
	var n C.uint64_t
	C.pbsgpu_stream_position(s.h, &n)
	return uint64(n)
}

// SuggestBoundary suggests a chunk boundary at the current position (payload chunker; a file starts here).
func (s *Stream) SuggestBoundary() error {
	defer runtime.KeepAlive(s) // the finalizer must not run Close while the C call is executing
	return check(C.pbsgpu_stream_suggest(s.h, C.uint64_t(s.PayloadPosition())), "stream_suggest")
}

func (s *Stream) Finish() error {
	defer runtime.KeepAlive(s) // the finalizer must not run Close while the C call is executing
	return s.busy("stream_finish", func() C.int { return C.pbsgpu_stream_finish(s.h) })
}

// FinishBegin closes the input without waiting for the last chunks' digests: the goroutine goes on with its next
// archive while this one drains; Poll keeps delivering, Done reports when the last entry is out.
func (s *Stream) FinishBegin() error {
	defer runtime.KeepAlive(s)
	return s.busy("stream_finish_begin", func() C.int { return C.pbsgpu_stream_finish_begin(s.h) })
}

// Done never blocks: true once every entry of a stream closed by Finish / FinishBegin can be polled.
func (s *Stream) Done() (bool, error) {
	defer runtime.KeepAlive(s)
	var d C.int
	if err := check(C.pbsgpu_stream_done(s.h, &d), "stream_done"); err != nil {
		return false, err
	}
	return d != 0, nil
}

func (s *Stream) Poll(max int) ([]ChunkInfo, error) {
	defer runtime.KeepAlive(s) // the finalizer must not run Close while the C call is executing
	if max <= 0 {
		return nil, errors.New("pbsgpu: Poll(max <= 0)")
	}
	buf := make([]C.pbsgpu_record, max)
	var n C.uint64_t
	if err := check(C.pbsgpu_stream_poll(s.h, &buf[0], C.uint64_t(max), &n), "stream_poll"); err != nil {
		return nil, err
	}
	return fromRecords(buf, int(n)), nil
}

// ---- held pages of a payload stream (PBSGPU_HAS_STREAM_UPLOAD) ------------------------------------------------------

// Hold makes the stream keep its pages until Release: UploadNew2 then frames the new chunks of what Write was given
// straight out of them, and the payload never leaves the device before it is known to be new. Only before the stream's
// first byte, marker or cut. The writer's loop: Write -> Poll -> UploadNew2 -> upload the blobs -> Release(last End).
// A call that needs a page calls OnBusy (or, without one, returns ErrBusy) instead of waiting for a page that only
// Release can bring; no byte is lost
// (Write reports the prefix it took; Inject, Finish, FinishBegin, WriteEntryReader's header and WriteMarker happen
// entirely or not at all).
func (s *Stream) Hold() error {
	defer runtime.KeepAlive(s)
	return check(C.pbsgpu_stream_hold(s.h), "stream_hold")
}

// Release says that the payload below position upto (at most the End of the last polled entry) is no longer needed.
func (s *Stream) Release(upto uint64) error {
	defer runtime.KeepAlive(s)
	return check(C.pbsgpu_stream_release(s.h, C.uint64_t(upto)), "stream_release")
}

// Held returns the lowest payload position whose bytes are still available, the handed-back pages the stream holds and
// the free pages of the engine's ring.
func (s *Stream) Held() (firstPosition uint64, pages, ringPagesFree uint32, err error) {
	defer runtime.KeepAlive(s)
	var f C.uint64_t
	var p, fr C.uint32_t
	err = check(C.pbsgpu_stream_held(s.h, &f, &p, &fr), "stream_held")
	return uint64(f), uint32(p), uint32(fr), err
}

// UploadNew2 is Ring.UploadNew2 for entries of this stream exactly as Poll returned them (End a payload position, Segment
// the section number; a batch may span sections).
func (s *Stream) UploadNew2(known *KnownChunks, recs []ChunkInfo, insert, zstd bool, dst unsafe.Pointer, dstCap uint64) (Uploaded2, error) {
	defer runtime.KeepAlive(s)
	defer runtime.KeepAlive(known)
	if len(recs) == 0 || known == nil {
		return Uploaded2{}, errors.New("pbsgpu: UploadNew2 needs entries and a known-chunk set")
	}
	cr := toRecords(recs)
	o := newUpload2Out(len(recs))
	ins := C.int(0)
	if insert {
		ins = 1
	}
	err := check(C.pbsgpu_stream_upload_new2_device(s.h, known.h, &cr[0], C.uint64_t(len(cr)), ins, encodeFlags(zstd), dst,
		C.uint64_t(dstCap), &o.flags[0], (*C.uint64_t)(unsafe.Pointer(&o.offsets[0])), (*C.uint32_t)(unsafe.Pointer(&o.lens[0])),
		(*C.uint8_t)(unsafe.Pointer(&o.kinds[0])), (*C.uint32_t)(unsafe.Pointer(&o.crcs[0])), &o.used, &o.st, &o.enc),
		"stream_upload_new2_device")
	return o.result(), err
}

// Copy writes the raw payload bytes [position, position + length) into device memory dst; the range lies in one section,
// is covered by polled entries and no Release has passed it.
func (s *Stream) Copy(position, length uint64, dst unsafe.Pointer) error {
	defer runtime.KeepAlive(s)
	return check(C.pbsgpu_stream_copy_device(s.h, C.uint64_t(position), C.uint64_t(length), dst), "stream_copy_device")
}

func (s *Stream) Close() {
	runtime.SetFinalizer(s, nil)
	if s.h != nil {
		C.pbsgpu_stream_destroy(s.h)
		s.h = nil
	}
	s.eng = nil
}

// Chunker mirrors the module's streaming chunker: Scan returns 0 when no boundary was found
// in data (all of it consumed) or the boundary position (bytes consumed, state reset).
type Chunker struct {
	h   *C.pbsgpu_chunker
	eng *Engine
}

func (e *Engine) NewChunker() (*Chunker, error) {
	defer runtime.KeepAlive(e) // the finalizer must not run Close while the C call is executing
	c := &Chunker{eng: e}
	if err := check(C.pbsgpu_chunker_create(e.h, &c.h), "chunker_create"); err != nil {
		return nil, err
	}
	runtime.SetFinalizer(c, func(c *Chunker) { c.Close() })
	return c, nil
}

func (c *Chunker) Scan(data []byte) (int, error) {
	defer runtime.KeepAlive(c) // the finalizer must not run Close while the C call is executing
	if len(data) == 0 {
		return 0, nil
	}
	var pos C.size_t
	err := check(C.pbsgpu_chunker_scan(c.h, unsafe.Pointer(&data[0]), C.size_t(len(data)), &pos), "chunker_scan")
	runtime.KeepAlive(data)
	return int(pos), err
}

func (c *Chunker) Reset() error {
	defer runtime.KeepAlive(c) // the finalizer must not run Close while the C call is executing
	return check(C.pbsgpu_chunker_reset(c.h), "chunker_reset")
}

func (c *Chunker) Close() {
	runtime.SetFinalizer(c, nil)
	if c.h != nil {
		C.pbsgpu_chunker_destroy(c.h)
		c.h = nil
	}
	c.eng = nil
}

// ---- whole-file hashes (verification) -------------------------------------------------------------------------------

// HashFiles is verification.HashFile (internal/agent/verification/handler.go:36-68) for many
// files of one buffer: digests[i] = SHA-256(buf[offsets[i] : offsets[i]+lengths[i]]). One GPU lane per file:
// worth it for MANY files per call (see DESIGN.md, crossover), not for a handful of huge ones.
//
// POLICY: SHA-256 is serial inside a file (one GPU lane per file, 0.036 GiB/s each), so a batch only beats the host's
// SHA-NI cores with more than ~55 files per core in flight. The reference's verify job keeps FOUR files in flight
// (internal/server/verification/job.go:493) — routed here it would be ~50x slower than sha256-simd. HashFiles therefore
// returns ErrHostFaster (and hashes nothing) when pbsgpu_sha256_many_pays says the host wins for this batch size on
// runtime.NumCPU() cores; HashFilesForced skips the question.
func (e *Engine) HashFiles(buf []byte, offsets, lengths []uint64) ([][32]byte, error) {
	defer runtime.KeepAlive(e) // the finalizer must not run Close while the C call is executing
	var pays C.int
	if err := check(C.pbsgpu_sha256_many_pays(e.h, C.uint32_t(len(offsets)), C.uint32_t(runtime.NumCPU()), &pays), "sha256_many_pays"); err != nil {
		return nil, err
	}
	if pays == 0 {
		return nil, ErrHostFaster
	}
	return e.HashFilesForced(buf, offsets, lengths)
}

// ErrHostFaster: the batch is too small for the GPU to beat the host's SHA-NI cores; hash on the host.
var ErrHostFaster = errors.New("pbsgpu: too few files in flight for the GPU to beat host SHA-256; hash on the host")

// Trim releases device memory the engine only keeps for re-use (window buffers of closed streams).
func (e *Engine) Trim() (uint64, error) {
	defer runtime.KeepAlive(e)
	var n C.uint64_t
	err := check(C.pbsgpu_engine_trim(e.h, &n), "engine_trim")
	return uint64(n), err
}

// HashFilesForced hashes on the GPU whatever the batch size.
func (e *Engine) HashFilesForced(buf []byte, offsets, lengths []uint64) ([][32]byte, error) {
	defer runtime.KeepAlive(e)
	segs, err := toSegments(offsets, lengths)
	if err != nil || len(segs) == 0 {
		return nil, errors.New("pbsgpu: HashFiles needs matching, non-empty offsets/lengths")
	}
	out := make([][32]byte, len(segs))
	var base unsafe.Pointer
	if len(buf) > 0 {
		base = unsafe.Pointer(&buf[0])
	}
	err = check(C.pbsgpu_sha256_many_host(e.h, base, C.uint64_t(len(buf)), &segs[0], C.uint32_t(len(segs)),
		(*C.uint8_t)(unsafe.Pointer(&out[0][0]))), "sha256_many_host")
	runtime.KeepAlive(buf)
	return out, err
}

// XXH3Files is the per-file XXH3-64 of verifyBackedFileHashes (internal/pxarmount/commit_orchestrate.go:485-562).
func (e *Engine) XXH3Files(buf []byte, offsets, lengths []uint64) ([]uint64, error) {
	defer runtime.KeepAlive(e) // the finalizer must not run Close while the C call is executing
	segs, err := toSegments(offsets, lengths)
	if err != nil || len(segs) == 0 {
		return nil, errors.New("pbsgpu: XXH3Files needs matching, non-empty offsets/lengths")
	}
	out := make([]uint64, len(segs))
	var base unsafe.Pointer
	if len(buf) > 0 {
		base = unsafe.Pointer(&buf[0])
	}
	err = check(C.pbsgpu_xxh3_many_host(e.h, base, C.uint64_t(len(buf)), &segs[0], C.uint32_t(len(segs)),
		(*C.uint64_t)(unsafe.Pointer(&out[0]))), "xxh3_many_host")
	runtime.KeepAlive(buf)
	return out, err
}

// ---- page ring: several archives at once, page-granular memory release ---------------------------------------------

// Ring runs the chunk loop for SEVERAL payload streams through one device arena (pbsgpu_ring_*): memory is given
// back page by page as soon as the chunks touching a page have been read by the persistent SHA-256 service, not when a
// whole batch has been hashed. One goroutine drives a Ring (like one goroutine owns a writer,
// internal/tapeio/converter.go:672-680); bytes reach a stream's pages through Reserve/Commit (a device pointer for
// a DMA, a peer GPU or a kernel). HOST bytes go through PayloadStream (pbsgpu_stream_*), which is a client of the engine's
// own ring: pinned staging, H2D straight into a reserved page, the same cut rounds and SHA-256 service.
// The goroutine may block in a Read for as long as it likes: a ring that is not called for the idle timeout stops its idle
// service by itself and the next Pump starts it again (nothing is lost); Park does so at once. No byte content fails
// a stream: candidate-dense data (a crafted short period) is cut exactly, by on-demand re-scans inside the cut round.
type Ring struct {
	h   *C.pbsgpu_ring
	eng *Engine
}

// RingOptions mirrors pbsgpu_ring_options; zero values select the library defaults.
type RingOptions struct {
	ArenaBytes, PageBytes         uint64
	MaxStreams, ShaCUs, RoundPages uint32
	// ExpressCUs run the two-lanes-per-chunk SHA-256 form on the long chunks (>= 5/8 of the maximum size): the chain of a
	// chunk ~1.4x faster at ~0.65 of the throughput per CU. For rings whose latency matters more than their CU-time.
	ExpressCUs uint32
	// ABI v5: what used to be PBSGPU_RING_* environment variables (pbsgpu.h); zero = default, RingOff = "none"
	MinRoundPages, MaxInflight, LongBytes, LongLoBytes, LongSpill, PollEvery, Flags uint32
	BacklogMiB, LoneDeferMs, IdleTimeoutS, AutoparkMs                                float64
	// LanesCUs of the pair service's share run the LANES service (one lane per chunk) for chunks of at most ShortBytes
	// (0 = 3/2 of the average chunk size). Off by default: measured neutral on bulk rings (DESIGN.md 5.5).
	LanesCUs   uint32
	ShortBytes uint64
	// FillCUs > 0 (experiments): the synthetic refill runs as that many whole-CU workgroups beside the scan instead of in turn with it.
	FillCUs uint32
	// HoldPages (PBSGPU_RING_F_HOLD_PAGES): pages the services are done with stay with their stream until Release, so
	// that EncodeBlobs / Copy can still read the polled chunks' bytes. The holder must release, or the ring stalls (ErrBusy).
	HoldPages bool
}

// RingOff expresses "none" for RingOptions fields whose zero value means "default" (PBSGPU_RING_OFF).
const RingOff = ^uint32(0)

func (e *Engine) NewRing(o RingOptions) (*Ring, error) {
	defer runtime.KeepAlive(e)
	co := C.pbsgpu_ring_options{arena_bytes: C.uint64_t(o.ArenaBytes), page_bytes: C.uint64_t(o.PageBytes),
		max_streams: C.uint32_t(o.MaxStreams), sha_cus: C.uint32_t(o.ShaCUs), round_pages: C.uint32_t(o.RoundPages),
		express_cus: C.uint32_t(o.ExpressCUs), min_round_pages: C.uint32_t(o.MinRoundPages),
		max_inflight: C.uint32_t(o.MaxInflight), long_bytes: C.uint32_t(o.LongBytes), long_lo_bytes: C.uint32_t(o.LongLoBytes),
		long_spill: C.uint32_t(o.LongSpill), poll_every: C.uint32_t(o.PollEvery), flags: C.uint32_t(o.Flags),
		backlog_mib: C.double(o.BacklogMiB), lone_defer_ms: C.double(o.LoneDeferMs), idle_timeout_s: C.double(o.IdleTimeoutS),
		autopark_ms: C.double(o.AutoparkMs), lanes_cus: C.uint32_t(o.LanesCUs), short_bytes: C.uint64_t(o.ShortBytes),
		fill_cus: C.uint32_t(o.FillCUs)}
	if o.HoldPages {
		co.flags |= C.PBSGPU_RING_F_HOLD_PAGES
	}
	r := &Ring{eng: e}
	if err := check(C.pbsgpu_ring_create(e.h, &co, &r.h), "ring_create"); err != nil {
		return nil, err
	}
	runtime.SetFinalizer(r, func(r *Ring) { r.Close() })
	return r, nil
}

// Open starts a new stream (fresh chunker state); ErrBusy when MaxStreams are open.
func (r *Ring) Open() (uint32, error) {
	defer runtime.KeepAlive(r)
	var s C.uint32_t
	st := C.pbsgpu_ring_open(r.h, &s)
	if st == C.PBSGPU_E_BUSY {
		return 0, ErrBusy
	}
	return uint32(s), check(st, "ring_open")
}

// Reserve returns the device address and capacity of the stream's next page; ErrBusy when no page is free right now.
func (r *Ring) Reserve(stream uint32) (dptr uintptr, capacity uint64, err error) {
	defer runtime.KeepAlive(r)
	var p unsafe.Pointer
	var c C.uint64_t
	st := C.pbsgpu_ring_reserve(r.h, C.uint32_t(stream), &p, &c)
	if st == C.PBSGPU_E_BUSY {
		return 0, 0, ErrBusy
	}
	return uintptr(p), uint64(c), check(st, "ring_reserve")
}

// Commit hands the first nbytes of the reserved page to the ring; final ends the stream.
func (r *Ring) Commit(stream uint32, nbytes uint64, final bool) error {
	defer runtime.KeepAlive(r)
	f := C.int(0)
	if final {
		f = 1
	}
	return check(C.pbsgpu_ring_commit(r.h, C.uint32_t(stream), C.uint64_t(nbytes), f), "ring_commit")
}

// FillSynthetic is the benchmark producer (pbsgpu_ring_fill); returns the bytes accepted.
func (r *Ring) FillSynthetic(stream uint32, seed uint64, kind uint32, nbytes uint64, final bool) (uint64, error) {
	defer runtime.KeepAlive(r)
	f := C.int(0)
	if final {
		f = 1
	}
	var taken C.uint64_t
	err := check(C.pbsgpu_ring_fill(r.h, C.uint32_t(stream), C.uint64_t(seed), C.uint32_t(kind), C.uint64_t(nbytes), f, &taken),
		"ring_fill")
	return uint64(taken), err
}

// Pump enqueues the committed pages as cut rounds and collects finished rounds and freed pages; never blocks.
func (r *Ring) Pump() error {
	defer runtime.KeepAlive(r)
	return check(C.pbsgpu_ring_pump(r.h), "ring_pump")
}

// Poll returns up to max finished (end, digest) entries of the stream in stream order; done once the stream has ended
// and every entry has been handed out.
func (r *Ring) Poll(stream uint32, max int) (recs []ChunkInfo, done bool, err error) {
	defer runtime.KeepAlive(r)
	if max <= 0 {
		return nil, false, errors.New("pbsgpu: Poll(max <= 0)")
	}
	buf := make([]C.pbsgpu_record, max)
	var n C.uint64_t
	var fin C.int
	if err = check(C.pbsgpu_ring_poll(r.h, C.uint32_t(stream), &buf[0], C.uint64_t(max), &n, &fin), "ring_poll"); err != nil {
		return nil, false, err
	}
	return fromRecords(buf, int(n)), fin != 0, nil
}

// PollAny returns finished entries of ANY open stream (Segment = stream id, each stream's entries in order) and the ids
// of the streams that have just handed out their last entry — for jobs with one stream per file.
func (r *Ring) PollAny(max, maxFinished int) (recs []ChunkInfo, finished []uint32, err error) {
	defer runtime.KeepAlive(r)
	if max <= 0 || maxFinished <= 0 {
		return nil, nil, errors.New("pbsgpu: PollAny(max <= 0)")
	}
	buf := make([]C.pbsgpu_record, max)
	fin := make([]C.uint32_t, maxFinished)
	var n C.uint64_t
	var nf C.uint32_t
	if err = check(C.pbsgpu_ring_poll_any(r.h, &buf[0], C.uint64_t(max), &n, &fin[0], C.uint32_t(maxFinished), &nf), "ring_poll_any"); err != nil {
		return nil, nil, err
	}
	finished = make([]uint32, int(nf))
	for i := range finished {
		finished[i] = uint32(fin[i])
	}
	return fromRecords(buf, int(n)), finished, nil
}

// CloseStream releases a finished, fully polled stream's slot.
func (r *Ring) CloseStream(stream uint32) error {
	defer runtime.KeepAlive(r)
	return check(C.pbsgpu_ring_close(r.h, C.uint32_t(stream)), "ring_close")
}

// RingAnyStream as EncodeBlobs' stream: every entry's stream is its Segment, as PollAny reports it.
const RingAnyStream = ^uint32(0)

// Release tells a HoldPages ring that the stream's bytes below upto (at most the End of the last entry Poll has handed
// out) are no longer needed: pages that lie wholly below go back to the free list. The watermark only moves forward.
func (r *Ring) Release(stream uint32, upto uint64) error {
	defer runtime.KeepAlive(r)
	return check(C.pbsgpu_ring_release(r.h, C.uint32_t(stream), C.uint64_t(upto)), "ring_release")
}

// Held reports the stream offset from which bytes are still available and how many handed-back pages the stream holds.
func (r *Ring) Held(stream uint32) (firstOffset uint64, pages uint32, err error) {
	defer runtime.KeepAlive(r)
	var f C.uint64_t
	var p C.uint32_t
	err = check(C.pbsgpu_ring_held(r.h, C.uint32_t(stream), &f, &p), "ring_held")
	return uint64(f), uint32(p), err
}

// EncodeBlobs frames the polled entries recs whose skip flag is not set (skip may be nil; true = known, leave it out) as
// uncompressed blobs, straight out of the ring's pages, back to back into device memory dst. It returns each kept
// entry's offset in dst (0 for skipped ones), its CRC and the bytes used. A dst that is too small is an error that names
// the size needed in used, and nothing is written. The loop of an incremental writer:
// Poll -> KnownChunks.Classify -> EncodeBlobs(skip = isKnown) -> copy out / upload -> append to the index -> Release(last End).
func (r *Ring) EncodeBlobs(stream uint32, recs []ChunkInfo, skip []bool, dst unsafe.Pointer, dstCap uint64) (offsets []uint64,
	crcs []uint32, used uint64, err error) {
	defer runtime.KeepAlive(r)
	if len(recs) == 0 || (skip != nil && len(skip) != len(recs)) {
		return nil, nil, 0, errors.New("pbsgpu: EncodeBlobs needs entries and, if given, one skip flag per entry")
	}
	cr := toRecords(recs)
	var sk *C.uint8_t
	if skip != nil {
		flags := make([]uint8, len(skip))
		for i, b := range skip {
			if b {
				flags[i] = 1
			}
		}
		sk = (*C.uint8_t)(unsafe.Pointer(&flags[0]))
	}
	offsets = make([]uint64, len(recs))
	crcs = make([]uint32, len(recs))
	var u C.uint64_t
	err = check(C.pbsgpu_ring_blob_encode_device(r.h, C.uint32_t(stream), &cr[0], C.uint64_t(len(cr)), sk, dst, C.uint64_t(dstCap),
		(*C.uint64_t)(unsafe.Pointer(&offsets[0])), (*C.uint32_t)(unsafe.Pointer(&crcs[0])), &u), "ring_blob_encode_device")
	if err != nil {
		return nil, nil, uint64(u), err
	}
	return offsets, crcs, uint64(u), nil
}

// Uploaded is what UploadNew returns: the classify result and the blobs of the new chunks. Offsets and CRCs are per
// entry and 0 for known ones; Used is the bytes written to dst — or, with a dst that is too small (an error: nothing is
// written and the set is unchanged, while Known and Stats are valid), the bytes needed.
type Uploaded struct {
	Known   []bool
	Offsets []uint64
	CRCs    []uint32
	Used    uint64
	Stats   DedupStats
}

func uploadedFrom(flags []C.uint8_t, offsets []uint64, crcs []uint32, used C.uint64_t, st C.pbsgpu_dedup_stats) Uploaded {
	known := make([]bool, len(flags))
	for i := range known {
		known[i] = flags[i] != 0
	}
	return Uploaded{known, offsets, crcs, uint64(used),
		DedupStats{uint64(st.nrecords), uint64(st.nunique), uint64(st.total_bytes), uint64(st.unique_bytes)}}
}

// UploadNew is KnownChunks.Classify and EncodeBlobs(skip = isKnown) in one device-side call: the polled entries recs are
// classified against known and the new ones framed straight out of the ring's pages into device memory dst. The flags
// stay on the device in between and the encode plan is built there, so the call comes back to the host once. The loop of
// an incremental writer: Poll -> UploadNew -> copy out / upload -> append to the index -> Release(last End).
func (r *Ring) UploadNew(known *KnownChunks, stream uint32, recs []ChunkInfo, insert bool, dst unsafe.Pointer,
	dstCap uint64) (Uploaded, error) {
	defer runtime.KeepAlive(r)
	defer runtime.KeepAlive(known)
	if len(recs) == 0 || known == nil {
		return Uploaded{}, errors.New("pbsgpu: UploadNew needs entries and a known-chunk set")
	}
	cr := toRecords(recs)
	flags := make([]C.uint8_t, len(recs))
	offsets := make([]uint64, len(recs))
	crcs := make([]uint32, len(recs))
	ins := C.int(0)
	if insert {
		ins = 1
	}
	var u C.uint64_t
	var st C.pbsgpu_dedup_stats
	err := check(C.pbsgpu_ring_upload_new_device(r.h, known.h, C.uint32_t(stream), &cr[0], C.uint64_t(len(cr)), ins, dst,
		C.uint64_t(dstCap), &flags[0], (*C.uint64_t)(unsafe.Pointer(&offsets[0])), (*C.uint32_t)(unsafe.Pointer(&crcs[0])),
		&u, &st), "ring_upload_new_device")
	return uploadedFrom(flags, offsets, crcs, u, st), err
}

// Uploaded2 is what UploadNew2 returns: Uploaded, and per new entry the blob's length and kind (0 uncompressed, 1 zstd
// compressed). Blob i lies at Offsets[i], in the slot the uncompressed layout gives it, and is Lens[i] long; slots are not
// compacted, so Used, the capacity verdict and a sizing call are those of UploadNew.
type Uploaded2 struct {
	Uploaded
	Lens    []uint32
	Kinds   []uint8
	Encoded EncodeStats
}

// upload2Out holds the C outputs of the two UploadNew2 calls.
type upload2Out struct {
	flags   []C.uint8_t
	offsets []uint64
	lens    []uint32
	kinds   []uint8
	crcs    []uint32
	used    C.uint64_t
	st      C.pbsgpu_dedup_stats
	enc     C.pbsgpu_encode_stats
}

func newUpload2Out(n int) *upload2Out {
	return &upload2Out{flags: make([]C.uint8_t, n), offsets: make([]uint64, n), lens: make([]uint32, n), kinds: make([]uint8, n),
		crcs: make([]uint32, n)}
}

func (o *upload2Out) result() Uploaded2 {
	out := Uploaded2{Uploaded: uploadedFrom(o.flags, o.offsets, o.crcs, o.used, o.st), Lens: o.lens, Kinds: o.kinds}
	for k := 0; k < 2; k++ {
		out.Encoded.Blobs[k], out.Encoded.BlobBytes[k] = uint64(o.enc.blobs[k]), uint64(o.enc.blob_bytes[k])
		out.Encoded.ChunkBytes[k] = uint64(o.enc.chunk_bytes[k])
	}
	out.Encoded.FrameBytes, out.Encoded.CRCBytes = uint64(o.enc.frame_bytes), uint64(o.enc.crc_bytes)
	return out
}

func encodeFlags(zstd bool) C.uint32_t {
	if zstd {
		return C.PBSGPU_ENCODE_F_ZSTD
	}
	return 0
}

// UploadNew2 is UploadNew for the writers that compress (internal/tapeio/converter.go:399, :410-435): with zstd true a new
// chunk whose zstd frame is strictly shorter than the chunk becomes a compressed blob, straight out of the ring's pages;
// every other one is the uncompressed blob UploadNew writes. The loop of a compressing writer: Poll -> UploadNew2 -> send
// dst + Offsets[i], Lens[i] for every new entry -> append to the index -> Release(last End). With zstd false every
// output is UploadNew's.
func (r *Ring) UploadNew2(known *KnownChunks, stream uint32, recs []ChunkInfo, insert, zstd bool, dst unsafe.Pointer,
	dstCap uint64) (Uploaded2, error) {
	defer runtime.KeepAlive(r)
	defer runtime.KeepAlive(known)
	if len(recs) == 0 || known == nil {
		return Uploaded2{}, errors.New("pbsgpu: UploadNew2 needs entries and a known-chunk set")
	}
	cr := toRecords(recs)
	o := newUpload2Out(len(recs))
	ins := C.int(0)
	if insert {
		ins = 1
	}
	err := check(C.pbsgpu_ring_upload_new2_device(r.h, known.h, C.uint32_t(stream), &cr[0], C.uint64_t(len(cr)), ins,
		encodeFlags(zstd), dst, C.uint64_t(dstCap), &o.flags[0], (*C.uint64_t)(unsafe.Pointer(&o.offsets[0])),
		(*C.uint32_t)(unsafe.Pointer(&o.lens[0])), (*C.uint8_t)(unsafe.Pointer(&o.kinds[0])),
		(*C.uint32_t)(unsafe.Pointer(&o.crcs[0])), &o.used, &o.st, &o.enc), "ring_upload_new2_device")
	return o.result(), err
}

// Copy writes the raw stream bytes [offset, offset + length), which polled entries must cover and no Release may have
// passed, into device memory dst — for consumers that compress on the host or want the bytes unframed.
func (r *Ring) Copy(stream uint32, offset, length uint64, dst unsafe.Pointer) error {
	defer runtime.KeepAlive(r)
	return check(C.pbsgpu_ring_copy_device(r.h, C.uint32_t(stream), C.uint64_t(offset), C.uint64_t(length), dst), "ring_copy_device")
}

// Quiesce waits until everything enqueued is hashed and stops the service kernel; the next Pump restarts it.
func (r *Ring) Quiesce() error {
	defer runtime.KeepAlive(r)
	return check(C.pbsgpu_ring_quiesce(r.h), "ring_quiesce")
}

// Park is Quiesce without the wait: the service ends by itself once it has hashed what is enqueued and the next Pump
// starts a new one. Call it before the driving goroutine sits in a blocking Read (internal/tapeio/converter.go:672-680)
// if hipFree / device-wide synchronisation elsewhere in the process must not wait for this ring. Not calling it is safe
// too: a ring that is not called for PBSGPU_RING_IDLE_TIMEOUT_S stops its idle service on its own and loses nothing.
func (r *Ring) Park() error {
	defer runtime.KeepAlive(r)
	return check(C.pbsgpu_ring_park(r.h), "ring_park")
}

// Suggest announces a suggested chunk boundary `offset` bytes into the stream (ascending, ahead of the bytes around it).
func (r *Ring) Suggest(stream uint32, offset uint64) error {
	defer runtime.KeepAlive(r)
	return check(C.pbsgpu_ring_suggest(r.h, C.uint32_t(stream), C.uint64_t(offset)), "ring_suggest")
}

// RingStats mirrors the counters of pbsgpu_ring_stats a caller sizes its feed with.
type RingStats struct {
	PageBytes, BytesEnqueued, Chunks uint64
	PagesTotal, PagesFree, Rounds    uint32
	ServiceMsLast                    float64
}

func (r *Ring) Stats() (RingStats, error) {
	defer runtime.KeepAlive(r)
	var st C.pbsgpu_ring_stats
	if err := check(C.pbsgpu_ring_get_stats(r.h, &st), "ring_get_stats"); err != nil {
		return RingStats{}, err
	}
	return RingStats{uint64(st.page_bytes), uint64(st.bytes_enqueued), uint64(st.chunks), uint32(st.pages_total),
		uint32(st.pages_free), uint32(st.rounds), float64(st.service_ms_last)}, nil
}

// Express reports the CUs of the ring's express service (0 = none) and the chunk size from which a chunk takes it.
func (r *Ring) Express() (cus uint32, longBytes uint64, err error) {
	defer runtime.KeepAlive(r)
	var c C.uint32_t
	var l C.uint64_t
	if err = check(C.pbsgpu_ring_express(r.h, &c, &l), "ring_express"); err != nil {
		return 0, 0, err
	}
	return uint32(c), uint64(l), nil
}

// RingProbe: cumulative regime counters of the ring's two SHA-256 services (pbsgpu_ring_get_probe). Ticks / Steps x 10 = ns
// per block step of a chain under load (an express step is two blocks), Cycles / Ticks x 100 = the shader clock in MHz.
type RingProbe struct {
	PairSteps, PairCycles, PairTicks          uint64
	ExpressSteps, ExpressCycles, ExpressTicks uint64
}

// Probe reads the counters (safe while the service runs); read twice and subtract to look at a phase.
func (r *Ring) Probe() (RingProbe, error) {
	defer runtime.KeepAlive(r)
	var p C.pbsgpu_ring_probe
	if err := check(C.pbsgpu_ring_get_probe(r.h, &p), "ring_get_probe"); err != nil {
		return RingProbe{}, err
	}
	return RingProbe{uint64(p.pair_steps), uint64(p.pair_cycles), uint64(p.pair_ticks), uint64(p.express_steps),
		uint64(p.express_cycles), uint64(p.express_ticks)}, nil
}

func (r *Ring) Close() {
	runtime.SetFinalizer(r, nil)
	if r.h != nil {
		C.pbsgpu_ring_destroy(r.h)
		r.h = nil
	}
	r.eng = nil
}

// ---- multi-GPU digest-set reduce (RCCL over xGMI, behind the C ABI) ---------------------------------------------------

// CommIDBytes is the size of the opaque id rank 0 creates and ships to the other ranks (over the agent's own RPC).
const CommIDBytes = C.PBSGPU_COMM_ID_BYTES

// Comm is one rank's end of the cross-GPU digest-set reduce (pbsgpu_comm_*): the path shards at archive granularity with
// no data-path collective — one Engine per GPU ingests its own streams (internal/tapeio/converter.go:396-439: one session
// per process) — and the (digest, size) records of all ranks meet in ONE all-gather + device dedup for cross-file
// duplicate detection. Every method is collective: all ranks call it, in the same order.
type Comm struct {
	h   *C.pbsgpu_comm
	eng *Engine
}

// NewCommID is called on rank 0 only.
func NewCommID() ([CommIDBytes]byte, error) {
	var id [CommIDBytes]byte
	err := check(C.pbsgpu_comm_unique_id((*C.uint8_t)(unsafe.Pointer(&id[0]))), "comm_unique_id")
	return id, err
}

func (e *Engine) NewComm(id [CommIDBytes]byte, rank, world int) (*Comm, error) {
	defer runtime.KeepAlive(e)
	c := &Comm{eng: e}
	if err := check(C.pbsgpu_comm_create(e.h, (*C.uint8_t)(unsafe.Pointer(&id[0])), C.int(rank), C.int(world), &c.h), "comm_create"); err != nil {
		return nil, err
	}
	runtime.SetFinalizer(c, (*Comm).Close)
	return c, nil
}

// Dedup contributes this rank's records (at most capRecords, the same bound on every rank: bytes per rank / minimum chunk
// size) and returns, for each of them, whether an earlier record of the union carries the same digest, plus the statistics
// of the union (identical on every rank).
func (c *Comm) Dedup(recs []ChunkInfo, capRecords uint64) ([]bool, DedupStats, error) {
	defer runtime.KeepAlive(c)
	var st C.pbsgpu_dedup_stats
	var rp *C.pbsgpu_record
	var dp *C.uint8_t
	cr := toRecords(recs)
	dup := make([]C.uint8_t, len(recs))
	if len(recs) > 0 {
		rp, dp = &cr[0], &dup[0]
	}
	if err := check(C.pbsgpu_digest_allgather_dedup(c.h, rp, C.uint64_t(len(recs)), C.uint64_t(capRecords), dp, &st), "digest_allgather_dedup"); err != nil {
		return nil, DedupStats{}, err
	}
	out := make([]bool, len(recs))
	for i := range out {
		out[i] = dup[i] != 0
	}
	return out, DedupStats{uint64(st.nrecords), uint64(st.nunique), uint64(st.total_bytes), uint64(st.unique_bytes)}, nil
}

// SplitPlan says which bytes of ONE stream of totalLen bytes rank `rank` of `world` owns, [ownStart, ownEnd), and which it
// must hold in device memory, [lo, hi): 63 bytes of window halo to the left, one maximum chunk to the right (arithmetic only).
func SplitPlan(totalLen uint64, world, rank int, maxChunk uint32) (ownStart, ownEnd, lo, hi uint64, err error) {
	var a, b, l, h C.uint64_t
	err = check(C.pbsgpu_split_plan(C.uint64_t(totalLen), C.int(world), C.int(rank), C.uint32_t(maxChunk), &a, &b, &l, &h), "split_plan")
	return uint64(a), uint64(b), uint64(l), uint64(h), err
}

// SplitStream cuts and hashes ONE stream of totalLen bytes that is split over the ranks of the communicator (collective;
// BASELINE configs[1] at N > 1 when the stream does not fit one GPU). local = DEVICE pointer to this rank's bytes [lo, hi) of
// SplitPlan. Every rank gets the whole stream's records, in stream order.
func (c *Comm) SplitStream(local unsafe.Pointer, totalLen uint64, capRecords uint64) ([]ChunkInfo, error) {
	defer runtime.KeepAlive(c)
	buf := make([]C.pbsgpu_record, capRecords+1)
	var n C.uint64_t
	if err := check(C.pbsgpu_comm_split_stream(c.h, local, C.uint64_t(totalLen), &buf[0], C.uint64_t(capRecords), &n), "comm_split_stream"); err != nil {
		return nil, err
	}
	return fromRecords(buf, int(n)), nil
}

// CommLastError is what RCCL reported when a communicator call of this process last failed ("" = nothing yet): a
// PBSGPU_E_HIP from NewComm / Dedup does not say whether the bootstrap found no network interface or the device faulted.
func CommLastError() string { return C.GoString(C.pbsgpu_comm_last_error()) }

func (c *Comm) Close() {
	runtime.SetFinalizer(c, nil)
	if c.h != nil {
		C.pbsgpu_comm_destroy(c.h)
		c.h = nil
	}
	c.eng = nil
}

// ---- known-chunk set (incremental dedup) --------------------------------------------------------------------------

// KnownChunks is the device-resident known-chunk set of an incremental session (pbsgpu_known_*): the digests of the
// previous snapshot's indexes (PreviousBackup, internal/pxarmount/commit_orchestrate.go:127-158) plus every chunk already
// sent or injected (InjectChunks refs, commit_reuse.go:315-341). Classify says, per polled record, whether the server
// already has the chunk; only the rest is uploaded. The set keeps its engine alive; one goroutine per set at a time.
type KnownChunks struct {
	h   *C.pbsgpu_known
	eng *Engine
}

// NewKnownChunks creates an empty set sized for `capacity` digests (0 = default); it grows by itself.
func (e *Engine) NewKnownChunks(capacity uint64) (*KnownChunks, error) {
	defer runtime.KeepAlive(e)
	k := &KnownChunks{eng: e}
	if err := check(C.pbsgpu_known_create(e.h, C.uint64_t(capacity), &k.h), "known_create"); err != nil {
		return nil, err
	}
	runtime.SetFinalizer(k, (*KnownChunks).Close)
	return k, nil
}

// Add inserts every digest of recs (idempotent).
func (k *KnownChunks) Add(recs []ChunkInfo) error {
	defer runtime.KeepAlive(k)
	if len(recs) == 0 {
		return nil
	}
	cr := toRecords(recs)
	return check(C.pbsgpu_known_add_host(k.h, &cr[0], C.uint64_t(len(cr))), "known_add_host")
}

// AddDynamicIndex inserts the digests of a .didx image (a previous snapshot's .mpxar.didx / .ppxar.didx). It validates
// what ParseDynamicIndex validates and, like it, does not verify the index checksum.
func (k *KnownChunks) AddDynamicIndex(blob []byte) error {
	defer runtime.KeepAlive(k)
	if len(blob) == 0 {
		return errors.New("pbsgpu: empty index")
	}
	return check(C.pbsgpu_known_add_didx(k.h, (*C.uint8_t)(unsafe.Pointer(&blob[0])), C.uint64_t(len(blob))), "known_add_didx")
}

// Classify reports known[i] = true when the set held the digest of recs[i] or an earlier record of this call carries it;
// false marks the first occurrence of a new chunk (upload it). With insert, the new digests are in the set afterwards.
// Stats: Records / TotalBytes over all records, Unique / UniqueBytes over the new ones.
func (k *KnownChunks) Classify(recs []ChunkInfo, insert bool) ([]bool, DedupStats, error) {
	defer runtime.KeepAlive(k)
	if len(recs) == 0 {
		return nil, DedupStats{}, nil
	}
	cr := toRecords(recs)
	flags := make([]C.uint8_t, len(recs))
	ins := C.int(0)
	if insert {
		ins = 1
	}
	var st C.pbsgpu_dedup_stats
	if err := check(C.pbsgpu_known_classify_host(k.h, &cr[0], C.uint64_t(len(cr)), ins, &flags[0], &st), "known_classify_host"); err != nil {
		return nil, DedupStats{}, err
	}
	out := make([]bool, len(recs))
	for i := range out {
		out[i] = flags[i] != 0
	}
	return out, DedupStats{uint64(st.nrecords), uint64(st.nunique), uint64(st.total_bytes), uint64(st.unique_bytes)}, nil
}

// UploadNew is Classify and Engine.EncodeBlobsDevice over the new chunks in one device-side call: chunk i =
// src[offsets[i], offsets[i]+lengths[i]) of device memory carries the digest of recs[i]; the blobs of the new ones go
// back to back into device memory dst.
func (k *KnownChunks) UploadNew(src unsafe.Pointer, srcBytes uint64, recs []ChunkInfo, offsets, lengths []uint64, insert bool,
	dst unsafe.Pointer, dstCap uint64) (Uploaded, error) {
	defer runtime.KeepAlive(k)
	segs, err := toSegments(offsets, lengths)
	if err != nil || len(segs) == 0 || len(segs) != len(recs) {
		return Uploaded{}, errors.New("pbsgpu: UploadNew needs entries and one (offset, length) per entry")
	}
	cr := toRecords(recs)
	flags := make([]C.uint8_t, len(recs))
	boff := make([]uint64, len(recs))
	crcs := make([]uint32, len(recs))
	ins := C.int(0)
	if insert {
		ins = 1
	}
	var u C.uint64_t
	var st C.pbsgpu_dedup_stats
	err = check(C.pbsgpu_known_upload_new_device(k.h, src, C.uint64_t(srcBytes), &cr[0], &segs[0], C.uint64_t(len(cr)), ins,
		dst, C.uint64_t(dstCap), &flags[0], (*C.uint64_t)(unsafe.Pointer(&boff[0])), (*C.uint32_t)(unsafe.Pointer(&crcs[0])),
		&u, &st), "known_upload_new_device")
	return uploadedFrom(flags, boff, crcs, u, st), err
}

// UploadNew2 is UploadNew with the blob's kind decided on the device (zstd true), as Engine.EncodeBlobs2 decides it: see
// Ring.UploadNew2. dst must not overlap src: the frames are read again for their CRC.
func (k *KnownChunks) UploadNew2(src unsafe.Pointer, srcBytes uint64, recs []ChunkInfo, offsets, lengths []uint64, insert, zstd bool,
	dst unsafe.Pointer, dstCap uint64) (Uploaded2, error) {
	defer runtime.KeepAlive(k)
	segs, err := toSegments(offsets, lengths)
	if err != nil || len(segs) == 0 || len(segs) != len(recs) {
		return Uploaded2{}, errors.New("pbsgpu: UploadNew2 needs entries and one (offset, length) per entry")
	}
	cr := toRecords(recs)
	o := newUpload2Out(len(recs))
	ins := C.int(0)
	if insert {
		ins = 1
	}
	err = check(C.pbsgpu_known_upload_new2_device(k.h, src, C.uint64_t(srcBytes), &cr[0], &segs[0], C.uint64_t(len(cr)), ins,
		encodeFlags(zstd), dst, C.uint64_t(dstCap), &o.flags[0], (*C.uint64_t)(unsafe.Pointer(&o.offsets[0])),
		(*C.uint32_t)(unsafe.Pointer(&o.lens[0])), (*C.uint8_t)(unsafe.Pointer(&o.kinds[0])),
		(*C.uint32_t)(unsafe.Pointer(&o.crcs[0])), &o.used, &o.st, &o.enc), "known_upload_new2_device")
	return o.result(), err
}

// Len is the number of digests in the set.
func (k *KnownChunks) Len() int {
	defer runtime.KeepAlive(k)
	var n C.uint64_t
	if C.pbsgpu_known_count(k.h, &n) != C.PBSGPU_OK {
		return 0
	}
	return int(n)
}

func (k *KnownChunks) Close() {
	runtime.SetFinalizer(k, nil)
	if k.h != nil {
		C.pbsgpu_known_destroy(k.h)
		k.h = nil
	}
	k.eng = nil
}

// DedupDevice flags duplicates among n records that already are in device memory (the receive buffer of an RCCL
// all-gather): the digest-set reduce without a host round trip of the set.
func (e *Engine) DedupDevice(drecs uintptr, n uint64) ([]bool, DedupStats, error) {
	defer runtime.KeepAlive(e)
	if n == 0 {
		return nil, DedupStats{}, nil
	}
	dup := make([]C.uint8_t, n)
	var st C.pbsgpu_dedup_stats
	if err := check(C.pbsgpu_dedup_device(e.h, unsafe.Pointer(drecs), C.uint64_t(n), &dup[0], &st), "dedup_device"); err != nil {
		return nil, DedupStats{}, err
	}
	out := make([]bool, n)
	for i := range out {
		out[i] = dup[i] != 0
	}
	return out, DedupStats{uint64(st.nrecords), uint64(st.nunique), uint64(st.total_bytes), uint64(st.unique_bytes)}, nil
}

// ---- data blobs: CRC-32, upload framing, chunk verification -------------------------------------------------------

// Blob kinds (PBSGPU_BLOB_*) and the status VerifyBlobs reports per blob, in the order the checks run.
const (
	BlobUncompressed        = 0
	BlobCompressed          = 1
	BlobEncrypted           = 2
	BlobEncryptedCompressed = 3

	BlobOK        = 0 // every check passed
	BlobBadMagic  = 1 // unknown magic, or shorter than its header
	BlobBadCRC    = 2
	BlobBadSize   = 3 // uncompressed: data length differs from the expected size
	BlobBadDigest = 4 // uncompressed: SHA-256 differs from the expected digest
	BlobCRCOnly   = 5 // compressed or encrypted with a good CRC: the content needs zstd / AES
)

// BlobStats counts VerifyBlobs' statuses (indexed by Blob*) and the bytes checked.
type BlobStats struct {
	Count                            [6]uint64
	BlobBytes, CRCBytes, SHA256Bytes uint64
}

// BlobMagic is the 8-byte magic of a blob kind: the first 8 bytes of SHA-256 of its name (PBS data_blob.rs).
func BlobMagic(kind int) ([8]byte, error) {
	var out [8]byte
	err := check(C.pbsgpu_blob_magic(C.int(kind), (*C.uint8_t)(unsafe.Pointer(&out[0]))), "blob_magic")
	return out, err
}

// CRC32Combine is zlib's crc32_combine: crc32.ChecksumIEEE(A || B) from the checksums of A and B and len(B).
func CRC32Combine(crcA, crcB uint32, lenB uint64) uint32 {
	var out C.uint32_t
	C.pbsgpu_crc32_combine(C.uint32_t(crcA), C.uint32_t(crcB), C.uint64_t(lenB), &out)
	return uint32(out)
}

// BlobEncodedSize is the size of the uncompressed blobs of chunks of these lengths: the sum of 12 + length.
func BlobEncodedSize(lengths []uint64) (uint64, error) {
	segs, err := toSegments(make([]uint64, len(lengths)), lengths)
	if err != nil {
		return 0, err
	}
	var n C.uint64_t
	var p *C.pbsgpu_segment
	if len(segs) > 0 {
		p = &segs[0]
	}
	err = check(C.pbsgpu_blob_encoded_size(p, C.uint32_t(len(segs)), &n), "blob_encoded_size")
	return uint64(n), err
}

// CRC32Files is crc32.ChecksumIEEE of many chunks of one host buffer: the CRC an uploader puts into each chunk's blob
// header (compress=false, internal/pxarmount/commit_orchestrate.go:137-149).
func (e *Engine) CRC32Files(buf []byte, offsets, lengths []uint64) ([]uint32, error) {
	defer runtime.KeepAlive(e)
	segs, err := toSegments(offsets, lengths)
	if err != nil || len(segs) == 0 {
		return nil, errors.New("pbsgpu: CRC32Files needs matching, non-empty offsets/lengths")
	}
	out := make([]uint32, len(segs))
	var base unsafe.Pointer
	if len(buf) > 0 {
		base = unsafe.Pointer(&buf[0])
	}
	err = check(C.pbsgpu_crc32_many_host(e.h, base, C.uint64_t(len(buf)), &segs[0], C.uint32_t(len(segs)),
		(*C.uint32_t)(unsafe.Pointer(&out[0]))), "crc32_many_host")
	runtime.KeepAlive(buf)
	return out, err
}

// EncodeBlobsDevice writes the uncompressed blobs of the chunks (offsets, lengths) of device memory src back to back
// into device memory dst. It returns each blob's offset in dst (one more entry: the total) and the chunks' CRCs; a dst
// smaller than BlobEncodedSize is an error and nothing is written.
func (e *Engine) EncodeBlobsDevice(src unsafe.Pointer, srcBytes uint64, offsets, lengths []uint64, dst unsafe.Pointer,
	dstCap uint64) ([]uint64, []uint32, error) {
	defer runtime.KeepAlive(e)
	segs, err := toSegments(offsets, lengths)
	if err != nil || len(segs) == 0 {
		return nil, nil, errors.New("pbsgpu: EncodeBlobsDevice needs matching, non-empty offsets/lengths")
	}
	offs := make([]uint64, len(segs)+1)
	crcs := make([]uint32, len(segs))
	var total C.uint64_t
	err = check(C.pbsgpu_blob_encode_device(e.h, src, C.uint64_t(srcBytes), &segs[0], C.uint32_t(len(segs)), dst,
		C.uint64_t(dstCap), &total, (*C.uint64_t)(unsafe.Pointer(&offs[0])), (*C.uint32_t)(unsafe.Pointer(&crcs[0]))),
		"blob_encode_device")
	if err != nil {
		return nil, nil, err
	}
	return offs, crcs, nil
}

func (e *Engine) verifyBlobs(device bool, base unsafe.Pointer, nbytes uint64, offsets, lengths []uint64,
	digests [][32]byte, sizes []uint32) ([]uint8, BlobStats, error) {
	segs, err := toSegments(offsets, lengths)
	if err != nil || len(segs) == 0 || (digests != nil && len(digests) != len(segs)) || (sizes != nil && len(sizes) != len(segs)) {
		return nil, BlobStats{}, errors.New("pbsgpu: VerifyBlobs needs matching, non-empty offsets/lengths/digests/sizes")
	}
	var dg *C.uint8_t
	if digests != nil {
		dg = (*C.uint8_t)(unsafe.Pointer(&digests[0][0]))
	}
	var sz *C.uint32_t
	if sizes != nil {
		sz = (*C.uint32_t)(unsafe.Pointer(&sizes[0]))
	}
	status := make([]uint8, len(segs))
	var st C.pbsgpu_blob_stats
	if device {
		err = check(C.pbsgpu_blob_verify_device(e.h, base, C.uint64_t(nbytes), &segs[0], C.uint32_t(len(segs)), dg, sz,
			(*C.uint8_t)(unsafe.Pointer(&status[0])), &st), "blob_verify_device")
	} else {
		err = check(C.pbsgpu_blob_verify_host(e.h, base, C.uint64_t(nbytes), &segs[0], C.uint32_t(len(segs)), dg, sz,
			(*C.uint8_t)(unsafe.Pointer(&status[0])), &st), "blob_verify_host")
	}
	if err != nil {
		return nil, BlobStats{}, err
	}
	var out BlobStats
	for i := range out.Count {
		out.Count[i] = uint64(st.count[i])
	}
	out.BlobBytes, out.CRCBytes, out.SHA256Bytes = uint64(st.blob_bytes), uint64(st.crc_bytes), uint64(st.sha_bytes)
	return status, out, nil
}

// VerifyBlobs checks whole blobs of a host buffer as a chunk-store read does (datastore.NewChunkStore,
// internal/server/verification/job.go:931): magic, CRC, then for uncompressed blobs the size and SHA-256 against the
// index (digests and sizes may be nil: that check is skipped). The SHA-256 follows HashFiles' policy: one GPU lane per
// chunk, so it pays with thousands of chunks per call.
func (e *Engine) VerifyBlobs(buf []byte, offsets, lengths []uint64, digests [][32]byte, sizes []uint32) ([]uint8, BlobStats, error) {
	defer runtime.KeepAlive(e)
	var base unsafe.Pointer
	if len(buf) > 0 {
		base = unsafe.Pointer(&buf[0])
	}
	status, st, err := e.verifyBlobs(false, base, uint64(len(buf)), offsets, lengths, digests, sizes)
	runtime.KeepAlive(buf)
	return status, st, err
}

// VerifyBlobsDevice is VerifyBlobs on blobs in device memory.
func (e *Engine) VerifyBlobsDevice(dptr unsafe.Pointer, nbytes uint64, offsets, lengths []uint64, digests [][32]byte,
	sizes []uint32) ([]uint8, BlobStats, error) {
	defer runtime.KeepAlive(e)
	return e.verifyBlobs(true, dptr, nbytes, offsets, lengths, digests, sizes)
}

// DecodeStats counts DecodeBlobs' statuses per index entry (indexed by Blob*) and the bytes it touched: BlobBytes,
// CRCBytes and SHA256Bytes once per distinct referenced blob, OutBytes what was written to dst.
type DecodeStats struct {
	Count                                      [6]uint64
	BlobBytes, CRCBytes, SHA256Bytes, OutBytes uint64
}

// DecodeBlobs restores the stream bytes [rangeStart, rangeEnd) into device memory dst from a contiguous slice idx of a
// dynamic index and the blobs (offsets, lengths) of a device buffer: what datastore.NewChunkStore +
// transfer.NewChunkedReader(idx, source) deliver (internal/server/verification/job.go:931-966,
// internal/pxar/format.go:101-129) and the ranged reads of internal/pxar/client.go:236. blobOf[i] is the blob that carries
// entry i (nil: blob i). The status per entry is VerifyBlobsDevice's for that blob with the entry's size and digest
// (checkDigest false: without the digest). An entry whose blob is not an uncompressed one of its size leaves its part of
// dst untouched.
func (e *Engine) DecodeBlobs(dptr unsafe.Pointer, nbytes uint64, offsets, lengths []uint64, idx []ChunkInfo, blobOf []uint32,
	rangeStart, rangeEnd uint64, checkDigest bool, dst unsafe.Pointer, dstCap uint64) ([]uint8, DecodeStats, error) {
	defer runtime.KeepAlive(e)
	segs, err := toSegments(offsets, lengths)
	if err != nil {
		return nil, DecodeStats{}, err
	}
	if blobOf != nil && len(blobOf) != len(idx) {
		return nil, DecodeStats{}, errors.New("pbsgpu: DecodeBlobs needs one blobOf per index entry")
	}
	cr := toRecords(idx)
	var sp *C.pbsgpu_segment
	if len(segs) > 0 {
		sp = &segs[0]
	}
	var rp *C.pbsgpu_record
	var bo *C.uint32_t
	status := make([]uint8, len(cr)+1)
	if len(cr) > 0 {
		rp = &cr[0]
		if blobOf != nil {
			bo = (*C.uint32_t)(unsafe.Pointer(&blobOf[0]))
		}
	}
	chk := C.int(0)
	if checkDigest {
		chk = 1
	}
	var st C.pbsgpu_decode_stats
	err = check(C.pbsgpu_blob_decode_device(e.h, dptr, C.uint64_t(nbytes), sp, C.uint32_t(len(segs)), rp, C.uint64_t(len(cr)), bo,
		C.uint64_t(rangeStart), C.uint64_t(rangeEnd), chk, dst, C.uint64_t(dstCap), (*C.uint8_t)(unsafe.Pointer(&status[0])),
		&st), "blob_decode_device")
	if err != nil {
		return nil, DecodeStats{}, err
	}
	var out DecodeStats
	for i := range out.Count {
		out.Count[i] = uint64(st.count[i])
	}
	out.BlobBytes, out.CRCBytes, out.SHA256Bytes = uint64(st.blob_bytes), uint64(st.crc_bytes), uint64(st.sha_bytes)
	out.OutBytes = uint64(st.out_bytes)
	return status[:len(cr)], out, nil
}

// Statuses of DecodeZstd and ZstdFrameInfo (PBSGPU_ZSTD_*).
const (
	ZstdOK          = 0
	ZstdBadFrame    = 1 // malformed or truncated
	ZstdBadSize     = 2 // needs more room than given, or the declared content size is not what was decoded
	ZstdUnsupported = 3 // dictionary, skippable frame, more than one frame, trailing bytes
)

// ZstdFrame is what the header of one zstd frame declares. ContentSize is valid when HasContentSize is set.
type ZstdFrame struct {
	Status         int
	ContentSize    uint64
	HasContentSize bool
	WindowSize     uint64
	HeaderBytes    uint32
	HasChecksum    bool
}

// ZstdFrameInfo reads the header of the zstd frame in `frame` (host only): what a caller without an index sizes the
// destination of DecodeZstd with.
func ZstdFrameInfo(frame []byte) (ZstdFrame, error) {
	var size, window C.uint64_t
	var hb C.uint32_t
	var ck C.int
	var p *C.uint8_t
	if len(frame) > 0 {
		p = (*C.uint8_t)(unsafe.Pointer(&frame[0]))
	}
	st := C.pbsgpu_zstd_frame_info(p, C.uint64_t(len(frame)), &size, &window, &hb, &ck)
	if st < 0 {
		return ZstdFrame{}, check(st, "zstd_frame_info")
	}
	return ZstdFrame{Status: int(st), ContentSize: uint64(size), HasContentSize: uint64(size) != ^uint64(0), WindowSize: uint64(window),
		HeaderBytes: uint32(hb), HasChecksum: ck != 0}, nil
}

// DecodeZstd decodes the zstd frames (offsets, lengths) of a device buffer in one launch: frame i goes to dst +
// outOffsets[i], which has outRooms[i] bytes of room. These are the chunks the stock client stores compressed
// (internal/server/backup/command.go) and that datastore.NewChunkStore reads back (internal/server/verification/job.go:931-966,
// internal/pxar/format.go:101-129). Returns the status (Zstd*) and the bytes produced per frame; a frame whose status is
// not ZstdOK leaves unspecified bytes in its own room and nothing anywhere else.
func (e *Engine) DecodeZstd(dptr unsafe.Pointer, nbytes uint64, offsets, lengths, outOffsets, outRooms []uint64, dst unsafe.Pointer,
	dstCap uint64) ([]uint8, []uint64, error) {
	defer runtime.KeepAlive(e)
	segs, err := toSegments(offsets, lengths)
	if err != nil {
		return nil, nil, err
	}
	outs, err := toSegments(outOffsets, outRooms)
	if err != nil {
		return nil, nil, err
	}
	if len(outs) != len(segs) {
		return nil, nil, errors.New("pbsgpu: DecodeZstd needs one destination per frame")
	}
	status := make([]uint8, len(segs)+1)
	decoded := make([]uint64, len(segs)+1)
	var sp, op *C.pbsgpu_segment
	if len(segs) > 0 {
		sp, op = &segs[0], &outs[0]
	}
	err = check(C.pbsgpu_zstd_decode_device(e.h, dptr, C.uint64_t(nbytes), sp, C.uint32_t(len(segs)), op, dst, C.uint64_t(dstCap),
		(*C.uint8_t)(unsafe.Pointer(&status[0])), (*C.uint64_t)(unsafe.Pointer(&decoded[0]))), "zstd_decode_device")
	if err != nil {
		return nil, nil, err
	}
	return status[:len(segs)], decoded[:len(segs)], nil
}

// ZstdEncodeBound is the length no frame of EncodeZstd for n bytes of content exceeds (host only).
func ZstdEncodeBound(n uint64) uint64 { return uint64(C.pbsgpu_zstd_encode_bound(C.uint64_t(n))) }

// EncodeZstd compresses the chunks (offsets, lengths) of a device buffer to one zstd frame each in one call: chunk i goes
// to dst + outOffsets[i], which has outRooms[i] bytes of room (ZstdEncodeBound(length) always suffices). These are the
// writers of the reference that compress: the tape converter's local store (internal/tapeio/converter.go:399) and its PBS
// store and session with Compress set (converter.go:410-435, cmd/bkf2pxar/main.go:33). Returns the status (ZstdOK or
// ZstdBadSize) and the frame's length per chunk; a chunk whose status is ZstdBadSize leaves unspecified bytes in its own
// room and nothing anywhere else.
func (e *Engine) EncodeZstd(dptr unsafe.Pointer, nbytes uint64, offsets, lengths, outOffsets, outRooms []uint64, dst unsafe.Pointer,
	dstCap uint64) ([]uint8, []uint64, error) {
	defer runtime.KeepAlive(e)
	segs, err := toSegments(offsets, lengths)
	if err != nil {
		return nil, nil, err
	}
	outs, err := toSegments(outOffsets, outRooms)
	if err != nil {
		return nil, nil, err
	}
	if len(outs) != len(segs) {
		return nil, nil, errors.New("pbsgpu: EncodeZstd needs one destination per chunk")
	}
	status := make([]uint8, len(segs)+1)
	frameLen := make([]uint64, len(segs)+1)
	var sp, op *C.pbsgpu_segment
	if len(segs) > 0 {
		sp, op = &segs[0], &outs[0]
	}
	err = check(C.pbsgpu_zstd_encode_device(e.h, dptr, C.uint64_t(nbytes), sp, C.uint32_t(len(segs)), op, dst, C.uint64_t(dstCap),
		(*C.uint8_t)(unsafe.Pointer(&status[0])), (*C.uint64_t)(unsafe.Pointer(&frameLen[0]))), "zstd_encode_device")
	if err != nil {
		return nil, nil, err
	}
	return status[:len(segs)], frameLen[:len(segs)], nil
}

// ZstdBadChecksum is DecodeZstd2's status for a frame that decoded, but not to what its content checksum says
// (PBSGPU_ZSTD_BAD_CHECKSUM).
const ZstdBadChecksum = 4

// Flags of DecodeZstd2 and EncodeZstd2 (PBSGPU_ZSTD_F_*).
const (
	ZstdFlagChecksum = 1 // verify, or write, the frame's content checksum
	ZstdFlagStream   = 2 // DecodeZstd2 only: every segment is a whole zstd stream
)

// ZstdStream is what the headers of a whole zstd stream declare. ContentSize, the sum over the frames, is valid when
// HasContentSize is set: when every frame declares its size.
type ZstdStream struct {
	Status         int
	ContentSize    uint64
	HasContentSize bool
	Frames         uint32
	Skippable      uint32
	AnyChecksum    bool
}

// ZstdStreamInfo walks the headers of the zstd stream in `stream` (host only): what a caller without an index sizes the
// destination of DecodeZstd2 with ZstdFlagStream with.
func ZstdStreamInfo(stream []byte) (ZstdStream, error) {
	var size C.uint64_t
	var nf, ns C.uint32_t
	var ck C.int
	var p *C.uint8_t
	if len(stream) > 0 {
		p = (*C.uint8_t)(unsafe.Pointer(&stream[0]))
	}
	st := C.pbsgpu_zstd_stream_info(p, C.uint64_t(len(stream)), &size, &nf, &ns, &ck)
	if st < 0 {
		return ZstdStream{}, check(st, "zstd_stream_info")
	}
	return ZstdStream{Status: int(st), ContentSize: uint64(size), HasContentSize: uint64(size) != ^uint64(0), Frames: uint32(nf),
		Skippable: uint32(ns), AnyChecksum: ck != 0}, nil
}

// XXH64Device hashes the ranges (offsets, lengths) of a device buffer with XXH64 and `seed` in one call: what a zstd
// frame's content checksum is the low 32 bits of (seed 0). Ranges may be empty, unaligned and overlapping.
func (e *Engine) XXH64Device(dptr unsafe.Pointer, nbytes uint64, offsets, lengths []uint64, seed uint64) ([]uint64, error) {
	defer runtime.KeepAlive(e)
	segs, err := toSegments(offsets, lengths)
	if err != nil {
		return nil, err
	}
	out := make([]uint64, len(segs)+1)
	var sp *C.pbsgpu_segment
	if len(segs) > 0 {
		sp = &segs[0]
	}
	err = check(C.pbsgpu_xxh64_many_device(e.h, dptr, C.uint64_t(nbytes), sp, C.uint32_t(len(segs)), C.uint64_t(seed),
		(*C.uint64_t)(unsafe.Pointer(&out[0]))), "xxh64_many_device")
	if err != nil {
		return nil, err
	}
	return out[:len(segs)], nil
}

// zstdBatch is what DecodeZstd2 and EncodeZstd2 share: the segments, one room each, the result arrays, the call.
func zstdBatch(who string, offsets, lengths, outOffsets, outRooms []uint64,
	call func(sp *C.pbsgpu_segment, n C.uint32_t, op *C.pbsgpu_segment, status *C.uint8_t, lens *C.uint64_t) C.int) ([]uint8, []uint64, error) {
	segs, err := toSegments(offsets, lengths)
	if err != nil {
		return nil, nil, err
	}
	outs, err := toSegments(outOffsets, outRooms)
	if err != nil {
		return nil, nil, err
	}
	if len(outs) != len(segs) {
		return nil, nil, errors.New("pbsgpu: " + who + " needs one destination per segment")
	}
	status := make([]uint8, len(segs)+1)
	lens := make([]uint64, len(segs)+1)
	var sp, op *C.pbsgpu_segment
	if len(segs) > 0 {
		sp, op = &segs[0], &outs[0]
	}
	if err := check(call(sp, C.uint32_t(len(segs)), op, (*C.uint8_t)(unsafe.Pointer(&status[0])), (*C.uint64_t)(unsafe.Pointer(&lens[0]))), who); err != nil {
		return nil, nil, err
	}
	return status[:len(segs)], lens[:len(segs)], nil
}

// DecodeZstd2 is DecodeZstd with flags, for frames that are not blobs of an index (the same call sites:
// internal/server/verification/job.go:931-966, internal/pxar/format.go:101-129). With ZstdFlagChecksum a frame that carries a
// content checksum is checked against it (ZstdBadChecksum, 0 bytes decoded); with ZstdFlagStream every segment is a whole
// zstd stream, decoded as ZSTD_decompress does it: frames one after the other, skippable frames skipped, an empty segment
// ZstdOK with 0 bytes. With flags 0 it is DecodeZstd, output for output.
func (e *Engine) DecodeZstd2(dptr unsafe.Pointer, nbytes uint64, offsets, lengths, outOffsets, outRooms []uint64, dst unsafe.Pointer,
	dstCap uint64, flags uint32) ([]uint8, []uint64, error) {
	defer runtime.KeepAlive(e)
	return zstdBatch("zstd_decode2_device", offsets, lengths, outOffsets, outRooms,
		func(sp *C.pbsgpu_segment, n C.uint32_t, op *C.pbsgpu_segment, status *C.uint8_t, lens *C.uint64_t) C.int {
			return C.pbsgpu_zstd_decode2_device(e.h, dptr, C.uint64_t(nbytes), sp, n, op, dst, C.uint64_t(dstCap), status, lens, C.uint32_t(flags))
		})
}

// ZstdEncodeBound2 is ZstdEncodeBound for EncodeZstd2 with the same flags: 4 bytes more with ZstdFlagChecksum (host only).
func ZstdEncodeBound2(n uint64, flags uint32) uint64 {
	return uint64(C.pbsgpu_zstd_encode_bound2(C.uint64_t(n), C.uint32_t(flags)))
}

// EncodeZstd2 is EncodeZstd with flags, for the same writers (internal/tapeio/converter.go:399, :410-435) when the frames are
// kept outside a blob: with ZstdFlagChecksum every frame carries its content checksum, 4 bytes more (ZstdEncodeBound2). With
// flags 0 it is EncodeZstd.
func (e *Engine) EncodeZstd2(dptr unsafe.Pointer, nbytes uint64, offsets, lengths, outOffsets, outRooms []uint64, dst unsafe.Pointer,
	dstCap uint64, flags uint32) ([]uint8, []uint64, error) {
	defer runtime.KeepAlive(e)
	return zstdBatch("zstd_encode2_device", offsets, lengths, outOffsets, outRooms,
		func(sp *C.pbsgpu_segment, n C.uint32_t, op *C.pbsgpu_segment, status *C.uint8_t, lens *C.uint64_t) C.int {
			return C.pbsgpu_zstd_encode2_device(e.h, dptr, C.uint64_t(nbytes), sp, n, op, dst, C.uint64_t(dstCap), status, lens, C.uint32_t(flags))
		})
}

// Statuses and flags of AesGcmMany (PBSGPU_AES_*).
const (
	AesOK          = 0
	AesBadTag      = 1 // the tag does not authenticate the message: its output is zeroed
	AesFlagEncrypt = 1
)

// AesKey is an AES-256 key on the device (pbsgpu_aes_key_*): round keys, hash key and multiplier tables. The 32 key bytes
// are not kept on the host; Close zeroes the device copy. How to get the key out of a PBS key file: INTEGRATION.md §6.
type AesKey struct {
	h   *C.pbsgpu_aes_key
	eng *Engine
}

// NewAesKey expands key (32 bytes) for the engine's device.
func (e *Engine) NewAesKey(key []byte) (*AesKey, error) {
	defer runtime.KeepAlive(e)
	if len(key) != 32 {
		return nil, errors.New("pbsgpu: an AES-256 key is 32 bytes")
	}
	k := &AesKey{eng: e}
	if err := check(C.pbsgpu_aes_key_create(e.h, (*C.uint8_t)(unsafe.Pointer(&key[0])), &k.h), "aes_key_create"); err != nil {
		return nil, err
	}
	runtime.SetFinalizer(k, (*AesKey).Close)
	return k, nil
}

func (k *AesKey) Close() {
	runtime.SetFinalizer(k, nil)
	if k.h != nil {
		C.pbsgpu_aes_key_destroy(k.h)
		k.h = nil
	}
	k.eng = nil
}

// AesGcmMany decrypts (flags 0) or encrypts (AesFlagEncrypt) many messages of a device buffer in one call: AES-256-GCM with an
// empty AAD, the cipher of the encrypted blob kinds the reference's pxar-mount cannot read (cmd/pxar-mount/main.go:43, :76
// drop -keyfile). ivs holds ivLen (12 or 16) bytes per message, tags 16 per message: read when decrypting, written when
// encrypting. Message i goes to dst at outOffsets[i], which has outRooms[i] >= lengths[i] bytes. Returns the status per
// message; a message whose tag is bad (AesBadTag) has its output zeroed.
func (k *AesKey) AesGcmMany(dptr unsafe.Pointer, nbytes uint64, offsets, lengths []uint64, ivs []byte, ivLen uint32, tags []byte,
	outOffsets, outRooms []uint64, dst unsafe.Pointer, dstCap uint64, flags uint32) ([]uint8, error) {
	defer runtime.KeepAlive(k)
	segs, err := toSegments(offsets, lengths)
	if err != nil {
		return nil, err
	}
	outs, err := toSegments(outOffsets, outRooms)
	if err != nil {
		return nil, err
	}
	n := len(segs)
	if len(outs) != n || len(ivs) != n*int(ivLen) || len(tags) != 16*n {
		return nil, errors.New("pbsgpu: AesGcmMany: one room, one IV and one 16-byte tag per message")
	}
	if n == 0 {
		return nil, nil
	}
	status := make([]uint8, n)
	err = check(C.pbsgpu_aes_gcm_many_device(k.h, dptr, C.uint64_t(nbytes), &segs[0], C.uint32_t(n),
		(*C.uint8_t)(unsafe.Pointer(&ivs[0])), C.uint32_t(ivLen), (*C.uint8_t)(unsafe.Pointer(&tags[0])), &outs[0], dst,
		C.uint64_t(dstCap), (*C.uint8_t)(unsafe.Pointer(&status[0])), C.uint32_t(flags)), "aes_gcm_many_device")
	if err != nil {
		return nil, err
	}
	return status, nil
}

// EncodeStats counts what EncodeBlobs2 wrote, per kind (index 0 uncompressed, 1 compressed).
type EncodeStats struct {
	Blobs, BlobBytes, ChunkBytes [2]uint64
	FrameBytes, CRCBytes         uint64
}

// Encoded2 is what EncodeBlobs2 returns: blob i lies at Offsets[i], in the slot the uncompressed layout gives it, and is
// Lens[i] long; Kinds[i] is 0 (uncompressed) or 1 (zstd compressed).
type Encoded2 struct {
	Offsets []uint64
	Lens    []uint32
	Kinds   []uint8
	CRCs    []uint32
	Stats   EncodeStats
}

// EncodeBlobs2 is EncodeBlobsDevice with the blob's kind decided on the device (zstd true): a chunk whose zstd frame is strictly
// shorter than the chunk becomes a compressed blob, every other one the uncompressed blob EncodeBlobsDevice writes
// (internal/tapeio/converter.go:399, :410-435). The server takes one chunk per request: send dst + Offsets[i], Lens[i].
// With zstd false every output is EncodeBlobsDevice's.
func (e *Engine) EncodeBlobs2(src unsafe.Pointer, srcBytes uint64, offsets, lengths []uint64, zstd bool, dst unsafe.Pointer,
	dstCap uint64) (Encoded2, error) {
	defer runtime.KeepAlive(e)
	segs, err := toSegments(offsets, lengths)
	if err != nil {
		return Encoded2{}, err
	}
	n := len(segs)
	out := Encoded2{Offsets: make([]uint64, n+1), Lens: make([]uint32, n+1), Kinds: make([]uint8, n+1), CRCs: make([]uint32, n+1)}
	var sp *C.pbsgpu_segment
	if n > 0 {
		sp = &segs[0]
	}
	flags := C.uint32_t(0)
	if zstd {
		flags |= C.PBSGPU_ENCODE_F_ZSTD
	}
	var st C.pbsgpu_encode_stats
	err = check(C.pbsgpu_blob_encode2_device(e.h, src, C.uint64_t(srcBytes), sp, C.uint32_t(n), flags, dst, C.uint64_t(dstCap),
		(*C.uint64_t)(unsafe.Pointer(&out.Offsets[0])), (*C.uint32_t)(unsafe.Pointer(&out.Lens[0])),
		(*C.uint8_t)(unsafe.Pointer(&out.Kinds[0])), (*C.uint32_t)(unsafe.Pointer(&out.CRCs[0])), &st), "blob_encode2_device")
	if err != nil {
		return Encoded2{}, err
	}
	out.Lens, out.Kinds, out.CRCs = out.Lens[:n], out.Kinds[:n], out.CRCs[:n]
	for k := 0; k < 2; k++ {
		out.Stats.Blobs[k], out.Stats.BlobBytes[k] = uint64(st.blobs[k]), uint64(st.blob_bytes[k])
		out.Stats.ChunkBytes[k] = uint64(st.chunk_bytes[k])
	}
	out.Stats.FrameBytes, out.Stats.CRCBytes = uint64(st.frame_bytes), uint64(st.crc_bytes)
	return out, nil
}

// BlobBadData is DecodeBlobs2's status for a compressed blob whose zstd frame is malformed or unsupported.
const BlobBadData = 6

// DecodeStats2 is DecodeStats with a count for BlobBadData and the bytes that went into and came out of the zstd decoder.
type DecodeStats2 struct {
	Count                                      [8]uint64
	BlobBytes, CRCBytes, SHA256Bytes, OutBytes uint64
	ZstdInBytes, ZstdOutBytes                  uint64
}

// DecodeBlobs2 is DecodeBlobs with the zstd-compressed blobs decoded on the device (zstd true): the restore loop of a
// datastore the stock client wrote (internal/server/backup/command.go; the readers of internal/server/verification/job.go:931-966
// and internal/pxar/format.go:101-129). A compressed blob with a good CRC is decoded to its entries' places and checked for
// the entry's size and, with checkDigest, the SHA-256 of the decoded bytes; BlobCRCOnly then means encrypted only. With zstd
// false every output is DecodeBlobs'.
func (e *Engine) DecodeBlobs2(dptr unsafe.Pointer, nbytes uint64, offsets, lengths []uint64, idx []ChunkInfo, blobOf []uint32,
	rangeStart, rangeEnd uint64, checkDigest, zstd bool, dst unsafe.Pointer, dstCap uint64) ([]uint8, DecodeStats2, error) {
	defer runtime.KeepAlive(e)
	segs, err := toSegments(offsets, lengths)
	if err != nil {
		return nil, DecodeStats2{}, err
	}
	if blobOf != nil && len(blobOf) != len(idx) {
		return nil, DecodeStats2{}, errors.New("pbsgpu: DecodeBlobs2 needs one blobOf per index entry")
	}
	cr := toRecords(idx)
	var sp *C.pbsgpu_segment
	if len(segs) > 0 {
		sp = &segs[0]
	}
	var rp *C.pbsgpu_record
	var bo *C.uint32_t
	status := make([]uint8, len(cr)+1)
	if len(cr) > 0 {
		rp = &cr[0]
		if blobOf != nil {
			bo = (*C.uint32_t)(unsafe.Pointer(&blobOf[0]))
		}
	}
	flags := C.uint32_t(0)
	if checkDigest {
		flags |= C.PBSGPU_DECODE_F_DIGEST
	}
	if zstd {
		flags |= C.PBSGPU_DECODE_F_ZSTD
	}
	var st C.pbsgpu_decode_stats2
	err = check(C.pbsgpu_blob_decode2_device(e.h, dptr, C.uint64_t(nbytes), sp, C.uint32_t(len(segs)), rp, C.uint64_t(len(cr)), bo,
		C.uint64_t(rangeStart), C.uint64_t(rangeEnd), flags, dst, C.uint64_t(dstCap), (*C.uint8_t)(unsafe.Pointer(&status[0])),
		&st), "blob_decode2_device")
	if err != nil {
		return nil, DecodeStats2{}, err
	}
	var out DecodeStats2
	for i := range out.Count {
		out.Count[i] = uint64(st.count[i])
	}
	out.BlobBytes, out.CRCBytes, out.SHA256Bytes = uint64(st.blob_bytes), uint64(st.crc_bytes), uint64(st.sha_bytes)
	out.OutBytes, out.ZstdInBytes, out.ZstdOutBytes = uint64(st.out_bytes), uint64(st.zstd_in_bytes), uint64(st.zstd_out_bytes)
	return status[:len(cr)], out, nil
}

// BlobBadTag is DecodeBlobs3's status for an encrypted blob whose tag does not authenticate it: a wrong key or a damaged blob.
const BlobBadTag = 7

// DecodeStats3 is DecodeStats2 with a count for BlobBadTag and the ciphertext bytes decrypted, once per distinct blob.
type DecodeStats3 struct {
	Count                                      [8]uint64
	BlobBytes, CRCBytes, SHA256Bytes, OutBytes uint64
	ZstdInBytes, ZstdOutBytes                  uint64
	AesBytes                                   uint64
}

// DecodeBlobs3 is DecodeBlobs2 with the encrypted blobs decrypted on the device under key: the restore loop of a datastore a
// stock client wrote with a key file, which the reference's pxar-mount cannot read (cmd/pxar-mount/main.go:43, :76 drop
// -keyfile). An encrypted blob with a good CRC is decrypted to its entries' places; an encrypted-compressed one is then decoded
// as a zstd frame if zstd is set and stays BlobCRCOnly if not. BlobBadTag: the entry's part of dst is zero where the blob was
// decrypted in place and untouched otherwise. checkDigest is not applied to encrypted entries (their index digest is keyed).
// With key nil every output is DecodeBlobs2's.
func (e *Engine) DecodeBlobs3(dptr unsafe.Pointer, nbytes uint64, offsets, lengths []uint64, idx []ChunkInfo, blobOf []uint32,
	rangeStart, rangeEnd uint64, checkDigest, zstd bool, key *AesKey, dst unsafe.Pointer, dstCap uint64) ([]uint8, DecodeStats3, error) {
	return e.decodeBlobs(false, dptr, nbytes, offsets, lengths, idx, blobOf, rangeStart, rangeEnd, checkDigest, zstd, key, nil, dst, dstCap)
}

// DecodeBlobs4 is DecodeBlobs3 with the keyed digest check (pbsgpu_blob_decode4_device): with a key, checkDigest and idKey, an
// entry of an encrypted kind that passed tag, frame and size is compared with SHA-256(plaintext || id_key), the digest a
// session with a key file puts into its index; BlobBadDigest on a mismatch, the bytes already stored stay. Entries of the plain
// kinds keep the plain digest. With idKey nil every output is DecodeBlobs3's.
func (e *Engine) DecodeBlobs4(dptr unsafe.Pointer, nbytes uint64, offsets, lengths []uint64, idx []ChunkInfo, blobOf []uint32,
	rangeStart, rangeEnd uint64, checkDigest, zstd bool, key *AesKey, idKey *IdKey, dst unsafe.Pointer, dstCap uint64) ([]uint8, DecodeStats3, error) {
	return e.decodeBlobs(true, dptr, nbytes, offsets, lengths, idx, blobOf, rangeStart, rangeEnd, checkDigest, zstd, key, idKey, dst, dstCap)
}

func (e *Engine) decodeBlobs(four bool, dptr unsafe.Pointer, nbytes uint64, offsets, lengths []uint64, idx []ChunkInfo, blobOf []uint32,
	rangeStart, rangeEnd uint64, checkDigest, zstd bool, key *AesKey, idKey *IdKey, dst unsafe.Pointer, dstCap uint64) ([]uint8, DecodeStats3, error) {
	defer runtime.KeepAlive(e)
	defer runtime.KeepAlive(key)
	defer runtime.KeepAlive(idKey)
	segs, err := toSegments(offsets, lengths)
	if err != nil {
		return nil, DecodeStats3{}, err
	}
	if blobOf != nil && len(blobOf) != len(idx) {
		return nil, DecodeStats3{}, errors.New("pbsgpu: DecodeBlobs3 needs one blobOf per index entry")
	}
	cr := toRecords(idx)
	var sp *C.pbsgpu_segment
	if len(segs) > 0 {
		sp = &segs[0]
	}
	var rp *C.pbsgpu_record
	var bo *C.uint32_t
	status := make([]uint8, len(cr)+1)
	if len(cr) > 0 {
		rp = &cr[0]
		if blobOf != nil {
			bo = (*C.uint32_t)(unsafe.Pointer(&blobOf[0]))
		}
	}
	flags := C.uint32_t(0)
	if checkDigest {
		flags |= C.PBSGPU_DECODE_F_DIGEST
	}
	if zstd {
		flags |= C.PBSGPU_DECODE_F_ZSTD
	}
	var kh *C.pbsgpu_aes_key
	if key != nil {
		flags |= C.PBSGPU_DECODE_F_AES
		kh = key.h
	}
	var st C.pbsgpu_decode_stats3
	if four {
		var ik *C.pbsgpu_id_key
		if idKey != nil {
			ik = idKey.h
		}
		err = check(C.pbsgpu_blob_decode4_device(e.h, dptr, C.uint64_t(nbytes), sp, C.uint32_t(len(segs)), rp, C.uint64_t(len(cr)), bo,
			C.uint64_t(rangeStart), C.uint64_t(rangeEnd), flags, kh, ik, dst, C.uint64_t(dstCap), (*C.uint8_t)(unsafe.Pointer(&status[0])),
			&st), "blob_decode4_device")
	} else {
		err = check(C.pbsgpu_blob_decode3_device(e.h, dptr, C.uint64_t(nbytes), sp, C.uint32_t(len(segs)), rp, C.uint64_t(len(cr)), bo,
			C.uint64_t(rangeStart), C.uint64_t(rangeEnd), flags, kh, dst, C.uint64_t(dstCap), (*C.uint8_t)(unsafe.Pointer(&status[0])),
			&st), "blob_decode3_device")
	}
	if err != nil {
		return nil, DecodeStats3{}, err
	}
	var out DecodeStats3
	for i := range out.Count {
		out.Count[i] = uint64(st.count[i])
	}
	out.BlobBytes, out.CRCBytes, out.SHA256Bytes = uint64(st.blob_bytes), uint64(st.crc_bytes), uint64(st.sha_bytes)
	out.OutBytes, out.ZstdInBytes, out.ZstdOutBytes = uint64(st.out_bytes), uint64(st.zstd_in_bytes), uint64(st.zstd_out_bytes)
	out.AesBytes = uint64(st.aes_bytes)
	return status[:len(cr)], out, nil
}

// ---- keyed chunk digests: SHA-256(content || id_key) -------------------------------------------------------------------

// IdKey is the 32-byte id key of keyed chunk digests on the device (pbsgpu_id_key_*). A session with a key file names a chunk
// in its index by SHA-256(content || id_key), not SHA-256(content). The bytes are not kept on the host; Close zeroes the
// device copy. Nothing is derived here: where the 32 bytes come from is the caller's (INTEGRATION.md §6).
type IdKey struct {
	h   *C.pbsgpu_id_key
	eng *Engine
}

// NewIdKey puts idKey (32 bytes) onto the engine's device.
func (e *Engine) NewIdKey(idKey []byte) (*IdKey, error) {
	defer runtime.KeepAlive(e)
	if len(idKey) != 32 {
		return nil, errors.New("pbsgpu: an id key is 32 bytes")
	}
	k := &IdKey{eng: e}
	if err := check(C.pbsgpu_id_key_create(e.h, (*C.uint8_t)(unsafe.Pointer(&idKey[0])), &k.h), "id_key_create"); err != nil {
		return nil, err
	}
	runtime.SetFinalizer(k, (*IdKey).Close)
	return k, nil
}

// Close zeroes and frees the device copy. No call may be using the key and no ticket submitted with it may be uncollected.
func (k *IdKey) Close() {
	runtime.SetFinalizer(k, nil)
	if k.h != nil {
		C.pbsgpu_id_key_destroy(k.h)
		k.h = nil
	}
	k.eng = nil
}

// HashChunksKeyed is HashFilesForced with the key: digests[i] = SHA-256(buf[offsets[i] : offsets[i]+lengths[i]] || id_key).
func (k *IdKey) HashChunksKeyed(buf []byte, offsets, lengths []uint64) ([][32]byte, error) {
	defer runtime.KeepAlive(k)
	segs, err := toSegments(offsets, lengths)
	if err != nil || len(segs) == 0 {
		return nil, errors.New("pbsgpu: HashChunksKeyed needs matching, non-empty offsets/lengths")
	}
	out := make([][32]byte, len(segs))
	var base unsafe.Pointer
	if len(buf) > 0 {
		base = unsafe.Pointer(&buf[0])
	}
	err = check(C.pbsgpu_sha256_keyed_many_host(k.h, base, C.uint64_t(len(buf)), &segs[0], C.uint32_t(len(segs)),
		(*C.uint8_t)(unsafe.Pointer(&out[0][0]))), "sha256_keyed_many_host")
	runtime.KeepAlive(buf)
	return out, err
}

// HashChunksKeyedDevice is HashChunksKeyed over ranges of a device buffer.
func (k *IdKey) HashChunksKeyedDevice(dptr unsafe.Pointer, nbytes uint64, offsets, lengths []uint64) ([][32]byte, error) {
	defer runtime.KeepAlive(k)
	segs, err := toSegments(offsets, lengths)
	if err != nil || len(segs) == 0 {
		return nil, errors.New("pbsgpu: HashChunksKeyedDevice needs matching, non-empty offsets/lengths")
	}
	out := make([][32]byte, len(segs))
	err = check(C.pbsgpu_sha256_keyed_many_device(k.h, dptr, C.uint64_t(nbytes), &segs[0], C.uint32_t(len(segs)),
		(*C.uint8_t)(unsafe.Pointer(&out[0][0]))), "sha256_keyed_many_device")
	return out, err
}

// SubmitKeyed is Submit (without suggested boundaries) with every record's digest keyed: the cut points are the same, the
// digest is SHA-256(chunk || id_key). Keep the key open until the ticket is collected.
func (e *Engine) SubmitKeyed(key *IdKey, buf []byte, offsets, lengths []uint64) (Ticket, error) {
	defer runtime.KeepAlive(e)
	defer runtime.KeepAlive(key)
	if key == nil {
		return 0, errors.New("pbsgpu: SubmitKeyed needs an id key")
	}
	segs, err := toSegments(offsets, lengths)
	if err != nil {
		return 0, err
	}
	var base unsafe.Pointer
	if len(buf) > 0 {
		base = unsafe.Pointer(&buf[0])
	}
	var sp *C.pbsgpu_segment
	if len(segs) > 0 {
		sp = &segs[0]
	}
	var t C.uint64_t
	st := C.pbsgpu_submit_host_keyed(e.h, key.h, base, C.uint64_t(len(buf)), sp, C.uint32_t(len(segs)), &t)
	runtime.KeepAlive(buf)
	if st == C.PBSGPU_E_BUSY {
		return 0, ErrBusy
	}
	return Ticket(t), check(st, "submit_host_keyed")
}

// SubmitKeyedDevice is SubmitKeyed over a device buffer, which must stay as it is until the ticket is collected.
func (e *Engine) SubmitKeyedDevice(key *IdKey, dptr unsafe.Pointer, nbytes uint64, offsets, lengths []uint64) (Ticket, error) {
	defer runtime.KeepAlive(e)
	defer runtime.KeepAlive(key)
	if key == nil {
		return 0, errors.New("pbsgpu: SubmitKeyedDevice needs an id key")
	}
	segs, err := toSegments(offsets, lengths)
	if err != nil {
		return 0, err
	}
	var sp *C.pbsgpu_segment
	if len(segs) > 0 {
		sp = &segs[0]
	}
	var t C.uint64_t
	st := C.pbsgpu_submit_device_keyed(e.h, key.h, dptr, C.uint64_t(nbytes), sp, C.uint32_t(len(segs)), &t)
	if st == C.PBSGPU_E_BUSY {
		return 0, ErrBusy
	}
	return Ticket(t), check(st, "submit_device_keyed")
}

// EncodeStats3 is EncodeStats over all four kinds (index 2 encrypted, 3 encrypted-compressed), with the plaintext bytes
// encrypted.
type EncodeStats3 struct {
	Blobs, BlobBytes, ChunkBytes   [4]uint64
	FrameBytes, CRCBytes, AesBytes uint64
}

// Encoded3 is what EncodeBlobs3 returns: Encoded2 with Kinds up to 3 and the IVs the blobs were written with, 16 bytes each.
type Encoded3 struct {
	Offsets []uint64
	Lens    []uint32
	Kinds   []uint8
	CRCs    []uint32
	IVs     []byte
	Stats   EncodeStats3
}

// EncodeBlobs3 is EncodeBlobs2 with the blobs encrypted on the device under key (AES-256-GCM, empty AAD): blob i lies in the
// slot [Offsets[i], Offsets[i] + 44 + length) as magic, CRC-32 of the ciphertext, IV, tag, ciphertext. Kind 2 holds the chunk,
// kind 3 (zstd true and the frame strictly shorter than the chunk) its frame. ivs holds 16 bytes per chunk; nil draws them
// from crypto/rand. Two equal IVs in one call are refused; uniqueness across calls under one key is the caller's to answer
// for. With key nil every output is EncodeBlobs2's and no IV is used.
func (e *Engine) EncodeBlobs3(src unsafe.Pointer, srcBytes uint64, offsets, lengths []uint64, zstd bool, key *AesKey, ivs []byte,
	dst unsafe.Pointer, dstCap uint64) (Encoded3, error) {
	defer runtime.KeepAlive(e)
	defer runtime.KeepAlive(key)
	segs, err := toSegments(offsets, lengths)
	if err != nil {
		return Encoded3{}, err
	}
	n := len(segs)
	out := Encoded3{Offsets: make([]uint64, n+1), Lens: make([]uint32, n+1), Kinds: make([]uint8, n+1), CRCs: make([]uint32, n+1)}
	var sp *C.pbsgpu_segment
	if n > 0 {
		sp = &segs[0]
	}
	flags := C.uint32_t(0)
	if zstd {
		flags |= C.PBSGPU_ENCODE_F_ZSTD
	}
	var kh *C.pbsgpu_aes_key
	var ip *C.uint8_t
	if key != nil {
		flags |= C.PBSGPU_ENCODE_F_AES
		kh = key.h
		if ivs == nil {
			ivs = make([]byte, 16*n)
			if _, err := rand.Read(ivs); err != nil {
				return Encoded3{}, err
			}
		}
		if len(ivs) != 16*n {
			return Encoded3{}, errors.New("pbsgpu: EncodeBlobs3 needs one 16-byte IV per chunk")
		}
		if n > 0 {
			ip = (*C.uint8_t)(unsafe.Pointer(&ivs[0]))
		}
		out.IVs = ivs
	}
	var st C.pbsgpu_encode_stats3
	err = check(C.pbsgpu_blob_encode3_device(e.h, src, C.uint64_t(srcBytes), sp, C.uint32_t(n), flags, kh, ip, dst, C.uint64_t(dstCap),
		(*C.uint64_t)(unsafe.Pointer(&out.Offsets[0])), (*C.uint32_t)(unsafe.Pointer(&out.Lens[0])),
		(*C.uint8_t)(unsafe.Pointer(&out.Kinds[0])), (*C.uint32_t)(unsafe.Pointer(&out.CRCs[0])), &st), "blob_encode3_device")
	if err != nil {
		return Encoded3{}, err
	}
	out.Lens, out.Kinds, out.CRCs = out.Lens[:n], out.Kinds[:n], out.CRCs[:n]
	for k := 0; k < 4; k++ {
		out.Stats.Blobs[k], out.Stats.BlobBytes[k] = uint64(st.blobs[k]), uint64(st.blob_bytes[k])
		out.Stats.ChunkBytes[k] = uint64(st.chunk_bytes[k])
	}
	out.Stats.FrameBytes, out.Stats.CRCBytes, out.Stats.AesBytes = uint64(st.frame_bytes), uint64(st.crc_bytes), uint64(st.aes_bytes)
	return out, nil
}
