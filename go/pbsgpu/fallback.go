//go:build !(cgo && gpuchunk)

// Without cgo or without the gpuchunk tag (the project's default CGO_ENABLED=0 builds,
// .goreleaser.yaml:30) this package only reports that the GPU engine is not compiled in, so
// the fork of github.com/pbs-plus/pxar keeps using its pure-Go chunker. Nothing here chunks.
// The file mirrors the WHOLE exported surface of pbsgpu.go (tests/test_binding_sources.py checks it), so code written
// against the GPU build still compiles in the default build and gets ErrNotBuilt at run time.
package pbsgpu

import (
	"errors"
	"io"
	"unsafe"
)

// ErrNotBuilt is returned by every entry point in non-GPU builds.
var ErrNotBuilt = errors.New("pbsgpu: built without cgo/gpuchunk; GPU engine unavailable")

var (
	ErrBusy       = errors.New("pbsgpu: all in-flight tickets used")
	ErrHostFaster = errors.New("pbsgpu: too few files in flight for the GPU to beat host SHA-256; hash on the host")
)

// CommIDBytes mirrors PBSGPU_COMM_ID_BYTES.
const CommIDBytes = 128

type (
	Config struct {
		AvgSize, MinSize, MaxSize, WindowSize int
		BreakTestMask, BreakTestMinimum       uint32
	}
	ChunkInfo struct {
		End     uint64
		Digest  [32]byte
		Segment uint32
		Size    uint32
	}
	Engine     struct{}
	Stream     struct{}
	Chunker    struct{}
	Ring       struct{}
	Comm       struct{}
	Ticket     uint64
	DedupStats struct{ Records, Unique, TotalBytes, UniqueBytes uint64 }
	Uploaded   struct {
		Known   []bool
		Offsets []uint64
		CRCs    []uint32
		Used    uint64
		Stats   DedupStats
	}
	Uploaded2 struct {
		Uploaded
		Lens    []uint32
		Kinds   []uint8
		Encoded EncodeStats
	}
	ReuseChunk struct {
		Size, Padding, EndOffset uint64
		Digest                   [32]byte
	}
	FileHash    struct{ Index, Size, XXH3 uint64 }
	RingOptions struct {
		ArenaBytes, PageBytes                                                            uint64
		MaxStreams, ShaCUs, RoundPages                                                   uint32
		ExpressCUs                                                                       uint32
		MinRoundPages, MaxInflight, LongBytes, LongLoBytes, LongSpill, PollEvery, Flags uint32
		BacklogMiB, LoneDeferMs, IdleTimeoutS, AutoparkMs                                float64
		LanesCUs                                                                         uint32
		ShortBytes                                                                       uint64
		FillCUs                                                                          uint32
		HoldPages                                                                        bool
	}
	EngineOptions struct {
		Inflight, ShaForm, ShaSlackPct, ShaDensePct                      uint32
		ResolveParMin                                                    uint64
		ShaManyFilesPerCore                                              uint32
		StreamShaCUs, StreamExpressCUs, StreamRingSlots, StreamCtxPool   uint32
		StreamRingGiB                                                    float64
		StreamPageBytes                                                  uint64
		ZstdSeqTables                                                    uint32
		ZstdWindowLog                                                    uint32
	}
	RingStats struct {
		PageBytes, BytesEnqueued, Chunks uint64
		PagesTotal, PagesFree, Rounds    uint32
		ServiceMsLast                    float64
	}
	RingProbe struct {
		PairSteps, PairCycles, PairTicks          uint64
		ExpressSteps, ExpressCycles, ExpressTicks uint64
	}
)

func NewConfig(int) (Config, error)               { return Config{}, ErrNotBuilt }
func (c Config) WithTable([256]uint32) Config     { return c }
func NewEngine(int, Config, int) (*Engine, error) { return nil, ErrNotBuilt }
func NewEngineOpt(int, Config, EngineOptions) (*Engine, error) { return nil, ErrNotBuilt }

const RingOff = ^uint32(0)
const RingAnyStream = ^uint32(0)
func ParseDynamicIndex([]byte) ([]ChunkInfo, int64, [32]byte, error) {
	return nil, 0, [32]byte{}, ErrNotBuilt
}
func LookupDynamicEntries([]ChunkInfo, uint64, uint64) ([]ReuseChunk, uint64, uint64, error) {
	return nil, 0, 0, ErrNotBuilt
}
func ShouldReuse([]ChunkInfo, uint64, uint64, *ReuseChunk, float64) (bool, error) { return false, ErrNotBuilt }

func (e *Engine) Close()                                                          {}
func (e *Engine) Submit([]byte, []uint64, []uint64, [][]uint64) (Ticket, error)   { return 0, ErrNotBuilt }
func (e *Engine) Done(Ticket) (bool, error)                                       { return false, ErrNotBuilt }
func (e *Engine) Collect(Ticket) ([]ChunkInfo, error)                             { return nil, ErrNotBuilt }
func (e *Engine) Dedup([]ChunkInfo) ([]bool, DedupStats, error)                   { return nil, DedupStats{}, ErrNotBuilt }
func (e *Engine) DedupDevice(uintptr, uint64) ([]bool, DedupStats, error)         { return nil, DedupStats{}, ErrNotBuilt }
func (e *Engine) EncodeDynamicIndex([]ChunkInfo, [16]byte, int64) ([]byte, error) { return nil, ErrNotBuilt }
func (e *Engine) NewStream(uint64) (*Stream, error)                               { return nil, ErrNotBuilt }
func (e *Engine) NewChunker() (*Chunker, error)                                   { return nil, ErrNotBuilt }
func (e *Engine) NewRing(RingOptions) (*Ring, error)                              { return nil, ErrNotBuilt }
func (e *Engine) NewComm([CommIDBytes]byte, int, int) (*Comm, error)              { return nil, ErrNotBuilt }
func (e *Engine) HashFiles([]byte, []uint64, []uint64) ([][32]byte, error)        { return nil, ErrNotBuilt }
func (e *Engine) HashFilesForced([]byte, []uint64, []uint64) ([][32]byte, error)  { return nil, ErrNotBuilt }
func (e *Engine) XXH3Files([]byte, []uint64, []uint64) ([]uint64, error)          { return nil, ErrNotBuilt }
func (e *Engine) Trim() (uint64, error)                                           { return 0, ErrNotBuilt }

func (s *Stream) Write([]byte) (int, error)                                  { return 0, ErrNotBuilt }
func (s *Stream) ReadFrom(io.Reader) (int64, error)                          { return 0, ErrNotBuilt }
func (s *Stream) WriteEntryReader(io.Reader, uint64) (uint64, uint64, error) { return 0, 0, ErrNotBuilt }
func (s *Stream) BeginFile() error                                           { return ErrNotBuilt }
func (s *Stream) EndFile() (uint64, error)                                   { return 0, ErrNotBuilt }
func (s *Stream) PollFiles(int) ([]FileHash, error)                          { return nil, ErrNotBuilt }
func (s *Stream) WriteMarker(bool) error                                     { return ErrNotBuilt }
func (s *Stream) Inject(uint64) error                                        { return ErrNotBuilt }
func (s *Stream) PayloadPosition() uint64                                    { return 0 }
func (s *Stream) SuggestBoundary() error                                     { return ErrNotBuilt }
func (s *Stream) Finish() error                                              { return ErrNotBuilt }
func (s *Stream) FinishBegin() error                                         { return ErrNotBuilt }
func (s *Stream) Done() (bool, error)                                        { return false, ErrNotBuilt }
func (s *Stream) Poll(int) ([]ChunkInfo, error)                              { return nil, ErrNotBuilt }
func (s *Stream) Hold() error                                                { return ErrNotBuilt }
func (s *Stream) Release(uint64) error                                       { return ErrNotBuilt }
func (s *Stream) Held() (uint64, uint32, uint32, error)                      { return 0, 0, 0, ErrNotBuilt }
func (s *Stream) UploadNew2(*KnownChunks, []ChunkInfo, bool, bool, unsafe.Pointer, uint64) (Uploaded2, error) {
	return Uploaded2{}, ErrNotBuilt
}
func (s *Stream) Copy(uint64, uint64, unsafe.Pointer) error                  { return ErrNotBuilt }
func (s *Stream) Close()                                                     {}

func (c *Chunker) Scan([]byte) (int, error) { return 0, ErrNotBuilt }
func (c *Chunker) Reset() error             { return ErrNotBuilt }
func (c *Chunker) Close()                   {}

func NewCommID() ([CommIDBytes]byte, error)                                      { return [CommIDBytes]byte{}, ErrNotBuilt }
func (c *Comm) Dedup([]ChunkInfo, uint64) ([]bool, DedupStats, error)            { return nil, DedupStats{}, ErrNotBuilt }
func (c *Comm) Close()                                                           {}
func (c *Comm) SplitStream(unsafe.Pointer, uint64, uint64) ([]ChunkInfo, error)  { return nil, ErrNotBuilt }
func SplitPlan(uint64, int, int, uint32) (uint64, uint64, uint64, uint64, error) { return 0, 0, 0, 0, ErrNotBuilt }
func CommLastError() string                                                      { return "" }
func (r *Ring) Open() (uint32, error)                                            { return 0, ErrNotBuilt }
func (r *Ring) Reserve(uint32) (uintptr, uint64, error)                          { return 0, 0, ErrNotBuilt }
func (r *Ring) Commit(uint32, uint64, bool) error                                { return ErrNotBuilt }
func (r *Ring) FillSynthetic(uint32, uint64, uint32, uint64, bool) (uint64, error) { return 0, ErrNotBuilt }
func (r *Ring) Pump() error                                                      { return ErrNotBuilt }
func (r *Ring) Poll(uint32, int) ([]ChunkInfo, bool, error)                      { return nil, false, ErrNotBuilt }
func (r *Ring) PollAny(int, int) ([]ChunkInfo, []uint32, error)                  { return nil, nil, ErrNotBuilt }
func (r *Ring) CloseStream(uint32) error                                         { return ErrNotBuilt }
func (r *Ring) Release(uint32, uint64) error                                     { return ErrNotBuilt }
func (r *Ring) Held(uint32) (uint64, uint32, error)                              { return 0, 0, ErrNotBuilt }
func (r *Ring) EncodeBlobs(uint32, []ChunkInfo, []bool, unsafe.Pointer, uint64) ([]uint64, []uint32, uint64, error) {
	return nil, nil, 0, ErrNotBuilt
}
func (r *Ring) UploadNew(*KnownChunks, uint32, []ChunkInfo, bool, unsafe.Pointer, uint64) (Uploaded, error) {
	return Uploaded{}, ErrNotBuilt
}
func (r *Ring) UploadNew2(*KnownChunks, uint32, []ChunkInfo, bool, bool, unsafe.Pointer, uint64) (Uploaded2, error) {
	return Uploaded2{}, ErrNotBuilt
}
func (r *Ring) Copy(uint32, uint64, uint64, unsafe.Pointer) error                { return ErrNotBuilt }
func (r *Ring) Quiesce() error                                                   { return ErrNotBuilt }
func (r *Ring) Park() error                                                      { return ErrNotBuilt }
func (r *Ring) Suggest(uint32, uint64) error                                     { return ErrNotBuilt }
func (r *Ring) Stats() (RingStats, error)                                        { return RingStats{}, ErrNotBuilt }
func (r *Ring) Express() (uint32, uint64, error)                                 { return 0, 0, ErrNotBuilt }
func (r *Ring) Probe() (RingProbe, error)                                        { return RingProbe{}, ErrNotBuilt }
func (r *Ring) Close()                                                           {}

// KnownChunks is the known-chunk set of an incremental session.
type KnownChunks struct{}

func (e *Engine) NewKnownChunks(uint64) (*KnownChunks, error)                 { return nil, ErrNotBuilt }
func (k *KnownChunks) Add([]ChunkInfo) error                                  { return ErrNotBuilt }
func (k *KnownChunks) AddDynamicIndex([]byte) error                           { return ErrNotBuilt }
func (k *KnownChunks) Classify([]ChunkInfo, bool) ([]bool, DedupStats, error) { return nil, DedupStats{}, ErrNotBuilt }
func (k *KnownChunks) UploadNew(unsafe.Pointer, uint64, []ChunkInfo, []uint64, []uint64, bool, unsafe.Pointer, uint64) (Uploaded, error) {
	return Uploaded{}, ErrNotBuilt
}
func (k *KnownChunks) UploadNew2(unsafe.Pointer, uint64, []ChunkInfo, []uint64, []uint64, bool, bool, unsafe.Pointer, uint64) (Uploaded2, error) {
	return Uploaded2{}, ErrNotBuilt
}
func (k *KnownChunks) Len() int                                               { return 0 }
func (k *KnownChunks) Close()                                                 {}

// Blob kinds and VerifyBlobs statuses (PBSGPU_BLOB_*).
const (
	BlobUncompressed        = 0
	BlobCompressed          = 1
	BlobEncrypted           = 2
	BlobEncryptedCompressed = 3

	BlobOK        = 0
	BlobBadMagic  = 1
	BlobBadCRC    = 2
	BlobBadSize   = 3
	BlobBadDigest = 4
	BlobCRCOnly   = 5
)

// BlobStats counts VerifyBlobs' statuses and the bytes checked.
type BlobStats struct {
	Count                            [6]uint64
	BlobBytes, CRCBytes, SHA256Bytes uint64
}

func BlobMagic(int) ([8]byte, error)             { return [8]byte{}, ErrNotBuilt }
func CRC32Combine(uint32, uint32, uint64) uint32 { return 0 }
func BlobEncodedSize([]uint64) (uint64, error)   { return 0, ErrNotBuilt }
func (e *Engine) CRC32Files([]byte, []uint64, []uint64) ([]uint32, error) { return nil, ErrNotBuilt }
func (e *Engine) EncodeBlobsDevice(unsafe.Pointer, uint64, []uint64, []uint64, unsafe.Pointer, uint64) ([]uint64, []uint32, error) {
	return nil, nil, ErrNotBuilt
}
func (e *Engine) VerifyBlobs([]byte, []uint64, []uint64, [][32]byte, []uint32) ([]uint8, BlobStats, error) {
	return nil, BlobStats{}, ErrNotBuilt
}
func (e *Engine) VerifyBlobsDevice(unsafe.Pointer, uint64, []uint64, []uint64, [][32]byte, []uint32) ([]uint8, BlobStats, error) {
	return nil, BlobStats{}, ErrNotBuilt
}

// DecodeStats counts DecodeBlobs' statuses per index entry and the bytes it touched.
type DecodeStats struct {
	Count                                      [6]uint64
	BlobBytes, CRCBytes, SHA256Bytes, OutBytes uint64
}

func (e *Engine) DecodeBlobs(unsafe.Pointer, uint64, []uint64, []uint64, []ChunkInfo, []uint32, uint64, uint64, bool, unsafe.Pointer, uint64) ([]uint8, DecodeStats, error) {
	return nil, DecodeStats{}, ErrNotBuilt
}

// Statuses of DecodeZstd and ZstdFrameInfo.
const (
	ZstdOK          = 0
	ZstdBadFrame    = 1
	ZstdBadSize     = 2
	ZstdUnsupported = 3
)

// ZstdFrame is what the header of one zstd frame declares.
type ZstdFrame struct {
	Status         int
	ContentSize    uint64
	HasContentSize bool
	WindowSize     uint64
	HeaderBytes    uint32
	HasChecksum    bool
}

func ZstdFrameInfo([]byte) (ZstdFrame, error) { return ZstdFrame{}, ErrNotBuilt }
func (e *Engine) DecodeZstd(unsafe.Pointer, uint64, []uint64, []uint64, []uint64, []uint64, unsafe.Pointer, uint64) ([]uint8, []uint64, error) {
	return nil, nil, ErrNotBuilt
}

// ZstdEncodeBound is the length no frame of EncodeZstd for n bytes of content exceeds.
func ZstdEncodeBound(n uint64) uint64 { return 0 }

func (e *Engine) EncodeZstd(unsafe.Pointer, uint64, []uint64, []uint64, []uint64, []uint64, unsafe.Pointer, uint64) ([]uint8, []uint64, error) {
	return nil, nil, ErrNotBuilt
}

// ZstdBadChecksum is DecodeZstd2's status for a frame that decoded, but not to what its content checksum says.
const ZstdBadChecksum = 4

// Flags of DecodeZstd2 and EncodeZstd2.
const (
	ZstdFlagChecksum = 1
	ZstdFlagStream   = 2
)

// ZstdStream is what the headers of a whole zstd stream declare.
type ZstdStream struct {
	Status         int
	ContentSize    uint64
	HasContentSize bool
	Frames         uint32
	Skippable      uint32
	AnyChecksum    bool
}

func ZstdStreamInfo([]byte) (ZstdStream, error) { return ZstdStream{}, ErrNotBuilt }
func (e *Engine) XXH64Device(unsafe.Pointer, uint64, []uint64, []uint64, uint64) ([]uint64, error) {
	return nil, ErrNotBuilt
}
func (e *Engine) DecodeZstd2(unsafe.Pointer, uint64, []uint64, []uint64, []uint64, []uint64, unsafe.Pointer, uint64, uint32) ([]uint8, []uint64, error) {
	return nil, nil, ErrNotBuilt
}

// ZstdEncodeBound2 is ZstdEncodeBound for EncodeZstd2 with the same flags.
func ZstdEncodeBound2(n uint64, flags uint32) uint64 { return 0 }

func (e *Engine) EncodeZstd2(unsafe.Pointer, uint64, []uint64, []uint64, []uint64, []uint64, unsafe.Pointer, uint64, uint32) ([]uint8, []uint64, error) {
	return nil, nil, ErrNotBuilt
}

// Statuses and flags of AesGcmMany.
const (
	AesOK          = 0
	AesBadTag      = 1
	AesFlagEncrypt = 1
)

// AesKey is an AES-256 key on the device.
type AesKey struct{}

func (e *Engine) NewAesKey([]byte) (*AesKey, error) { return nil, ErrNotBuilt }
func (k *AesKey) Close()                            {}
func (k *AesKey) AesGcmMany(unsafe.Pointer, uint64, []uint64, []uint64, []byte, uint32, []byte, []uint64, []uint64, unsafe.Pointer, uint64, uint32) ([]uint8, error) {
	return nil, ErrNotBuilt
}

// EncodeStats counts what EncodeBlobs2 wrote, per kind (index 0 uncompressed, 1 compressed).
type EncodeStats struct {
	Blobs, BlobBytes, ChunkBytes [2]uint64
	FrameBytes, CRCBytes         uint64
}

// Encoded2 is what EncodeBlobs2 returns.
type Encoded2 struct {
	Offsets []uint64
	Lens    []uint32
	Kinds   []uint8
	CRCs    []uint32
	Stats   EncodeStats
}

func (e *Engine) EncodeBlobs2(unsafe.Pointer, uint64, []uint64, []uint64, bool, unsafe.Pointer, uint64) (Encoded2, error) {
	return Encoded2{}, ErrNotBuilt
}

// BlobBadData is DecodeBlobs2's status for a compressed blob whose zstd frame is malformed or unsupported.
const BlobBadData = 6

// DecodeStats2 is DecodeStats with a count for BlobBadData and the zstd decoder's byte counts.
type DecodeStats2 struct {
	Count                                      [8]uint64
	BlobBytes, CRCBytes, SHA256Bytes, OutBytes uint64
	ZstdInBytes, ZstdOutBytes                  uint64
}

func (e *Engine) DecodeBlobs2(unsafe.Pointer, uint64, []uint64, []uint64, []ChunkInfo, []uint32, uint64, uint64, bool, bool, unsafe.Pointer, uint64) ([]uint8, DecodeStats2, error) {
	return nil, DecodeStats2{}, ErrNotBuilt
}

// BlobBadTag is DecodeBlobs3's status for an encrypted blob whose tag does not authenticate it.
const BlobBadTag = 7

// DecodeStats3 is DecodeStats2 with a count for BlobBadTag and the ciphertext bytes decrypted.
type DecodeStats3 struct {
	Count                                      [8]uint64
	BlobBytes, CRCBytes, SHA256Bytes, OutBytes uint64
	ZstdInBytes, ZstdOutBytes                  uint64
	AesBytes                                   uint64
}

func (e *Engine) DecodeBlobs3(unsafe.Pointer, uint64, []uint64, []uint64, []ChunkInfo, []uint32, uint64, uint64, bool, bool, *AesKey, unsafe.Pointer, uint64) ([]uint8, DecodeStats3, error) {
	return nil, DecodeStats3{}, ErrNotBuilt
}

// EncodeStats3 is EncodeStats over all four kinds, with the plaintext bytes encrypted.
type EncodeStats3 struct {
	Blobs, BlobBytes, ChunkBytes   [4]uint64
	FrameBytes, CRCBytes, AesBytes uint64
}

// Encoded3 is what EncodeBlobs3 returns.
type Encoded3 struct {
	Offsets []uint64
	Lens    []uint32
	Kinds   []uint8
	CRCs    []uint32
	IVs     []byte
	Stats   EncodeStats3
}

func (e *Engine) DecodeBlobs4(unsafe.Pointer, uint64, []uint64, []uint64, []ChunkInfo, []uint32, uint64, uint64, bool, bool, *AesKey, *IdKey, unsafe.Pointer, uint64) ([]uint8, DecodeStats3, error) {
	return nil, DecodeStats3{}, ErrNotBuilt
}

// IdKey is the id key of keyed chunk digests on the device.
type IdKey struct{}

func (e *Engine) NewIdKey([]byte) (*IdKey, error) { return nil, ErrNotBuilt }
func (k *IdKey) Close()                          {}
func (k *IdKey) HashChunksKeyed([]byte, []uint64, []uint64) ([][32]byte, error) {
	return nil, ErrNotBuilt
}
func (k *IdKey) HashChunksKeyedDevice(unsafe.Pointer, uint64, []uint64, []uint64) ([][32]byte, error) {
	return nil, ErrNotBuilt
}
func (e *Engine) SubmitKeyed(*IdKey, []byte, []uint64, []uint64) (Ticket, error) { return 0, ErrNotBuilt }
func (e *Engine) SubmitKeyedDevice(*IdKey, unsafe.Pointer, uint64, []uint64, []uint64) (Ticket, error) {
	return 0, ErrNotBuilt
}

func (e *Engine) EncodeBlobs3(unsafe.Pointer, uint64, []uint64, []uint64, bool, *AesKey, []byte, unsafe.Pointer, uint64) (Encoded3, error) {
	return Encoded3{}, ErrNotBuilt
}
