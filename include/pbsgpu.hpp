// include/pbsgpu.hpp — header-only C++17 host mirror of the reference's Go interface for the pxar
// stream path, over the C ABI in pbsgpu.h (the reference is compiled Go; no Go toolchain exists in
// the build image, so the host side above the C ABI is C++ — names, argument meaning and error
// behaviour follow the module API as pbs-plus uses it):
//
//   buzhash::NewConfig(avg)                      internal/pxarmount/commit_orchestrate.go:143-149,
//                                                internal/tapeio/converter.go:248
//   datastore::NewDynamicIndexWriter(ctime).Add(end, digest).Finish()
//                                                internal/pxarmount/commit_bottleneck_test.go:773-793
//   datastore::ParseDynamicIndex / DynamicIndexReader{Count, ChunkInfo, ChunkFromOffset}
//                                                internal/pxarmount/commit_reuse.go:84-135, commit_orchestrate.go:219
//   transfer::PayloadWriter{WriteEntryReader, InjectChunks, Finish}  (the payload half of transfer.ArchiveWriter)
//                                                internal/pxarmount/commit_test.go:33-67, commit_reuse.go:315-341,457
//
// Go's (value, error) returns become a Result<T>{value, err}: err.empty() means success.
#pragma once

#include <algorithm>
#include <array>
#include <cstdint>
#include <cstring>
#include <functional>
#include <istream>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "pbsgpu.h"

namespace pbsgpu {

template <typename T> struct Result {
    T value{};
    std::string err;  // empty = nil error
    explicit operator bool() const { return err.empty(); }
};

inline std::string errorf(const char *what, int status) {
    return std::string("pbsgpu: ") + what + ": " + pbsgpu_strerror(status);
}

namespace buzhash {

// buzhash.Config: a plain value handed to NewPBSStore / NewLocalStore / BackupConfig.ChunkConfig
struct Config {
    int AvgSize = 0, MinSize = 0, MaxSize = 0, WindowSize = 0;
    uint32_t BreakTestMask = 0, BreakTestMinimum = 0;
    pbsgpu_config c{};
};

// buzhash.NewConfig(avgSize int) (Config, error)
inline Result<Config> NewConfig(int avgSize) {
    Result<Config> r;
    const int st = pbsgpu_config_init(avgSize < 0 ? 0 : (uint64_t)avgSize, nullptr, &r.value.c);
    if (st != PBSGPU_OK) {
        r.err = "buzhash: average chunk size must be a power of two in [256, 2^28]";
        return r;
    }
    const pbsgpu_config &c = r.value.c;
    r.value.AvgSize = (int)c.avg;
    r.value.MinSize = (int)c.min;
    r.value.MaxSize = (int)c.max;
    r.value.WindowSize = (int)c.window;
    r.value.BreakTestMask = c.mask;
    r.value.BreakTestMinimum = c.break_min;
    return r;
}

}  // namespace buzhash

namespace datastore {

using Digest = std::array<uint8_t, 32>;

// datastore.ChunkInfo{End, Digest}
struct ChunkInfo {
    uint64_t End = 0;
    Digest Digest_{};
};

// backupproxy.KnownChunkRef{Digest, Size}
struct KnownChunkRef {
    Digest Digest_{};
    uint64_t Size = 0;
};

// What KnownChunks::UploadNew / transfer::PageRing::UploadNew return: the classify result and the blobs of the new chunks
struct Uploaded {
    uint64_t bytes = 0;              // blob bytes written to dst — or, with a dst that is too small (an error: nothing
                                     // written, the set unchanged, known / stats valid), the bytes needed
    std::vector<uint8_t> known;      // per record: 1 = the server has the chunk
    std::vector<uint64_t> offsets;   // per new record: its blob's offset in dst
    std::vector<uint32_t> crcs;      // per new record
    pbsgpu_dedup_stats stats{};
};

// What the fused calls with the blob's kind decided on the device return (UploadNew2): Uploaded, and per new record
// the blob's length and kind; the blob lies at offsets[i] in the slot the uncompressed layout gives it.
struct Uploaded2 {
    uint64_t bytes = 0;              // as Uploaded::bytes: the slots' bytes, or the bytes needed
    std::vector<uint8_t> known;
    std::vector<uint64_t> offsets;   // per new record: its slot's offset in dst
    std::vector<uint32_t> lens;      // per new record: the blob's length, what is sent
    std::vector<uint8_t> kinds;      // per new record: PBSGPU_BLOB_UNCOMPRESSED or PBSGPU_BLOB_COMPRESSED
    std::vector<uint32_t> crcs;      // per new record
    pbsgpu_dedup_stats stats{};
    pbsgpu_encode_stats encoded{};
    void Resize(size_t n) {
        known.assign(n, 0);
        offsets.assign(n, 0);
        lens.assign(n, 0);
        kinds.assign(n, 0);
        crcs.assign(n, 0);
    }
};

// The known-chunk set of an incremental session (pbsgpu_known_*, device resident): the digests of the previous
// snapshot's indexes (PreviousBackup, commit_orchestrate.go:127-158) plus every chunk already sent or injected
// (InjectChunks refs, commit_reuse.go:315-341). Classify flags, per record, the chunks the server already has; the rest
// is uploaded. Keeps its engine alive; one thread per set at a time.
class KnownChunks {
  public:
    static Result<std::unique_ptr<KnownChunks>> New(pbsgpu_engine *eng, uint64_t capacity = 0) {
        Result<std::unique_ptr<KnownChunks>> r;
        pbsgpu_known *k = nullptr;
        const int st = pbsgpu_known_create(eng, capacity, &k);
        if (st != PBSGPU_OK) {
            r.err = errorf("known chunks", st);
            return r;
        }
        r.value.reset(new KnownChunks(k));
        return r;
    }
    ~KnownChunks() { pbsgpu_known_destroy(k_); }
    KnownChunks(const KnownChunks &) = delete;
    KnownChunks &operator=(const KnownChunks &) = delete;

    std::string Add(const std::vector<KnownChunkRef> &refs) {
        std::vector<pbsgpu_record> recs(refs.size());
        for (size_t i = 0; i < refs.size(); ++i) {
            std::memcpy(recs[i].digest, refs[i].Digest_.data(), 32);
            recs[i].size = (uint32_t)refs[i].Size;
        }
        return AddRecords(recs);
    }
    std::string AddRecords(const std::vector<pbsgpu_record> &recs) {
        const int st = pbsgpu_known_add_host(k_, recs.data(), recs.size());
        return st == PBSGPU_OK ? std::string() : errorf("known chunks add", st);
    }
    // the bytes of a previous snapshot's .didx (validated as ParseDynamicIndex does; the index checksum is not verified)
    std::string AddDynamicIndex(const std::vector<uint8_t> &didx) {
        const int st = pbsgpu_known_add_didx(k_, didx.data(), didx.size());
        return st == PBSGPU_OK ? std::string() : errorf("known chunks add dynamic index", st);
    }
    // known[i]: the set held the digest, or an earlier record of this call carries it; false = upload this chunk
    Result<std::vector<bool>> Classify(const std::vector<pbsgpu_record> &recs, bool insert,
                                       pbsgpu_dedup_stats *stats = nullptr) {
        Result<std::vector<bool>> r;
        std::vector<uint8_t> flags(recs.size());
        pbsgpu_dedup_stats st{};
        const int s = pbsgpu_known_classify_host(k_, recs.data(), recs.size(), insert ? 1 : 0, flags.data(), &st);
        if (s != PBSGPU_OK) {
            r.err = errorf("known chunks classify", s);
            return r;
        }
        if (stats) *stats = st;
        r.value.assign(flags.begin(), flags.end());
        return r;
    }
    // Classify and the upload framing of the new chunks in one device-side call (commit_orchestrate.go:137-158 behind the
    // known-chunk check; commit_reuse.go:315-341 refs are known): chunk i = chunks[i] of device buffer src carries the
    // digest of recs[i]; the blobs of the new ones go back to back into device buffer dst.
    Result<Uploaded> UploadNew(const void *src, uint64_t srcBytes, const std::vector<pbsgpu_record> &recs,
                               const std::vector<pbsgpu_segment> &chunks, bool insert, void *dst, uint64_t dstCap) {
        Result<Uploaded> r;
        if (chunks.size() != recs.size()) {
            r.err = errorf("known chunks upload new", PBSGPU_E_INVALID);
            return r;
        }
        r.value.known.assign(recs.size(), 0);
        r.value.offsets.assign(recs.size(), 0);
        r.value.crcs.assign(recs.size(), 0);
        const int st = pbsgpu_known_upload_new_device(k_, src, srcBytes, recs.data(), chunks.data(), recs.size(), insert ? 1 : 0,
                                                      dst, dstCap, r.value.known.data(), r.value.offsets.data(),
                                                      r.value.crcs.data(), &r.value.bytes, &r.value.stats);
        if (st != PBSGPU_OK) r.err = errorf("known chunks upload new", st);
        return r;
    }
    // UploadNew for the writers that compress (converter.go:399, 410-435): with zstd a new chunk whose frame is strictly
    // shorter than the chunk becomes a compressed blob in its slot; without, UploadNew's outputs with lens and kinds.
    Result<Uploaded2> UploadNew2(const void *src, uint64_t srcBytes, const std::vector<pbsgpu_record> &recs,
                                 const std::vector<pbsgpu_segment> &chunks, bool insert, bool zstd, void *dst, uint64_t dstCap) {
        Result<Uploaded2> r;
        if (chunks.size() != recs.size()) {
            r.err = errorf("known chunks upload new2", PBSGPU_E_INVALID);
            return r;
        }
        Uploaded2 &v = r.value;
        v.Resize(recs.size());
        const int st = pbsgpu_known_upload_new2_device(k_, src, srcBytes, recs.data(), chunks.data(), recs.size(), insert ? 1 : 0,
                                                       zstd ? PBSGPU_ENCODE_F_ZSTD : 0u, dst, dstCap, v.known.data(),
                                                       v.offsets.data(), v.lens.data(), v.kinds.data(), v.crcs.data(), &v.bytes,
                                                       &v.stats, &v.encoded);
        if (st != PBSGPU_OK) r.err = errorf("known chunks upload new2", st);
        return r;
    }
    uint64_t Len() const {
        uint64_t n = 0;
        pbsgpu_known_count(k_, &n);
        return n;
    }
    pbsgpu_known *Handle() const { return k_; }

  private:
    explicit KnownChunks(pbsgpu_known *k) : k_(k) {}
    pbsgpu_known *k_;
};

// Data blobs (pbsgpu_crc32_* / pbsgpu_blob_*): the CRC-32 of the uploader's chunks, the uncompressed blobs of chunks in
// device memory, and the chunk check of the read side (datastore.NewChunkStore: internal/server/verification/job.go:931).
// Thin wrappers; the Go module's own blob types are not mirrored.
namespace blob {

// the 8-byte magic of a blob kind (PBSGPU_BLOB_UNCOMPRESSED ...)
inline Result<std::array<uint8_t, 8>> Magic(int kind) {
    Result<std::array<uint8_t, 8>> r;
    const int st = pbsgpu_blob_magic(kind, r.value.data());
    if (st != PBSGPU_OK) r.err = errorf("blob magic", st);
    return r;
}

// crc32.ChecksumIEEE(A || B) from the two checksums and len(B) (zlib's crc32_combine)
inline uint32_t CRC32Combine(uint32_t crcA, uint32_t crcB, uint64_t lenB) {
    uint32_t out = 0;
    pbsgpu_crc32_combine(crcA, crcB, lenB, &out);
    return out;
}

// CRC-32 of every range of a host buffer (the uploader's chunks live on the host) or of a device buffer
inline Result<std::vector<uint32_t>> CRC32Many(pbsgpu_engine *eng, const void *buf, uint64_t nbytes,
                                               const std::vector<pbsgpu_segment> &segs, bool device = false) {
    Result<std::vector<uint32_t>> r;
    r.value.resize(segs.size());
    const int st = device ? pbsgpu_crc32_many_device(eng, buf, nbytes, segs.data(), (uint32_t)segs.size(), r.value.data())
                          : pbsgpu_crc32_many_host(eng, buf, nbytes, segs.data(), (uint32_t)segs.size(), r.value.data());
    if (st != PBSGPU_OK) r.err = errorf("crc32 many", st);
    return r;
}

inline Result<uint64_t> EncodedSize(const std::vector<pbsgpu_segment> &segs) {
    Result<uint64_t> r;
    const int st = pbsgpu_blob_encoded_size(segs.data(), (uint32_t)segs.size(), &r.value);
    if (st != PBSGPU_OK) r.err = errorf("blob encoded size", st);
    return r;
}

struct Encoded {
    uint64_t bytes = 0;              // blob bytes written to dst
    std::vector<uint64_t> offsets;   // blob i = dst[offsets[i], offsets[i + 1])
    std::vector<uint32_t> crcs;
};

// uncompressed blobs of the chunks segs of device buffer src, back to back in device buffer dst
inline Result<Encoded> EncodeDevice(pbsgpu_engine *eng, const void *src, uint64_t srcBytes,
                                    const std::vector<pbsgpu_segment> &segs, void *dst, uint64_t dstCap) {
    Result<Encoded> r;
    r.value.offsets.resize(segs.size() + 1);
    r.value.crcs.resize(segs.size());
    const int st = pbsgpu_blob_encode_device(eng, src, srcBytes, segs.data(), (uint32_t)segs.size(), dst, dstCap,
                                             &r.value.bytes, r.value.offsets.data(), r.value.crcs.data());
    if (st != PBSGPU_OK) r.err = errorf("blob encode", st);
    return r;
}

struct Verified {
    std::vector<uint8_t> status;  // PBSGPU_BLOB_* per blob
    pbsgpu_blob_stats stats{};
};

// check whole blobs of a host (or device) buffer; digests (32 per blob) and sizes may be empty: that check is skipped
inline Result<Verified> Verify(pbsgpu_engine *eng, const void *buf, uint64_t nbytes, const std::vector<pbsgpu_segment> &blobs,
                               const std::vector<uint8_t> &digests, const std::vector<uint32_t> &sizes,
                               bool device = false) {
    Result<Verified> r;
    r.value.status.resize(blobs.size());
    const uint8_t *dg = digests.empty() ? nullptr : digests.data();
    const uint32_t *sz = sizes.empty() ? nullptr : sizes.data();
    const int st = device ? pbsgpu_blob_verify_device(eng, buf, nbytes, blobs.data(), (uint32_t)blobs.size(), dg, sz,
                                                      r.value.status.data(), &r.value.stats)
                          : pbsgpu_blob_verify_host(eng, buf, nbytes, blobs.data(), (uint32_t)blobs.size(), dg, sz,
                                                    r.value.status.data(), &r.value.stats);
    if (st != PBSGPU_OK) r.err = errorf("blob verify", st);
    return r;
}

struct Decoded {
    std::vector<uint8_t> status;  // PBSGPU_BLOB_* per index entry
    pbsgpu_decode_stats stats{};
};

// the stream bytes [rangeStart, rangeEnd) into device buffer dst from a contiguous slice idx of an index and the blobs of
// a device buffer: transfer.NewChunkedReader(idx, source) over a datastore.NewChunkStore. blobOf[i] = the blob that
// carries entry i (empty: blob i). An entry whose blob is not an uncompressed one of its size leaves its part of dst
// untouched: read status.
inline Result<Decoded> Decode(pbsgpu_engine *eng, const void *blobsDev, uint64_t nbytes,
                              const std::vector<pbsgpu_segment> &blobs, const std::vector<pbsgpu_record> &idx,
                              const std::vector<uint32_t> &blobOf, uint64_t rangeStart, uint64_t rangeEnd, bool checkDigest,
                              void *dst, uint64_t dstCap) {
    Result<Decoded> r;
    r.value.status.resize(idx.size() + 1);
    const int st = pbsgpu_blob_decode_device(eng, blobsDev, nbytes, blobs.data(), (uint32_t)blobs.size(), idx.data(),
                                             idx.size(), blobOf.empty() ? nullptr : blobOf.data(), rangeStart, rangeEnd,
                                             checkDigest ? 1 : 0, dst, dstCap, r.value.status.data(), &r.value.stats);
    r.value.status.resize(idx.size());
    if (st != PBSGPU_OK) r.err = errorf("blob decode", st);
    return r;
}

struct Decoded2 {
    std::vector<uint8_t> status;  // PBSGPU_BLOB_* per index entry, PBSGPU_BLOB_BAD_DATA included
    pbsgpu_decode_stats2 stats{};
};

// Decode with the zstd-compressed blobs decoded on the device (zstd = true: PBSGPU_DECODE_F_ZSTD): the restore loop of a
// datastore the stock client wrote (internal/server/backup/command.go). BlobCRCOnly then means encrypted only.
inline Result<Decoded2> Decode2(pbsgpu_engine *eng, const void *blobsDev, uint64_t nbytes,
                                const std::vector<pbsgpu_segment> &blobs, const std::vector<pbsgpu_record> &idx,
                                const std::vector<uint32_t> &blobOf, uint64_t rangeStart, uint64_t rangeEnd, bool checkDigest,
                                bool zstd, void *dst, uint64_t dstCap) {
    Result<Decoded2> r;
    r.value.status.resize(idx.size() + 1);
    const uint32_t flags = (checkDigest ? PBSGPU_DECODE_F_DIGEST : 0u) | (zstd ? PBSGPU_DECODE_F_ZSTD : 0u);
    const int st = pbsgpu_blob_decode2_device(eng, blobsDev, nbytes, blobs.data(), (uint32_t)blobs.size(), idx.data(),
                                              idx.size(), blobOf.empty() ? nullptr : blobOf.data(), rangeStart, rangeEnd,
                                              flags, dst, dstCap, r.value.status.data(), &r.value.stats);
    r.value.status.resize(idx.size());
    if (st != PBSGPU_OK) r.err = errorf("blob decode2", st);
    return r;
}

struct ZstdDecoded {
    std::vector<uint8_t> status;    // PBSGPU_ZSTD_* per frame
    std::vector<uint64_t> decoded;  // bytes produced per frame (0 unless OK)
};

// many zstd frames of a device buffer into device buffer dst in one launch: frame i to dst + out[i].offset, which has
// out[i].length bytes of room (the chunks internal/server/backup/command.go's client stores compressed). A frame whose
// status is not PBSGPU_ZSTD_OK leaves unspecified bytes in its own room and nothing anywhere else.
inline Result<ZstdDecoded> DecodeZstd(pbsgpu_engine *eng, const void *src, uint64_t nbytes, const std::vector<pbsgpu_segment> &frames,
                                      const std::vector<pbsgpu_segment> &out, void *dst, uint64_t dstCap) {
    Result<ZstdDecoded> r;
    if (out.size() != frames.size()) {
        r.err = errorf("zstd decode", PBSGPU_E_INVALID);
        return r;
    }
    r.value.status.resize(frames.size() + 1);
    r.value.decoded.resize(frames.size() + 1);
    const int st = pbsgpu_zstd_decode_device(eng, src, nbytes, frames.data(), (uint32_t)frames.size(), out.data(), dst, dstCap,
                                             r.value.status.data(), r.value.decoded.data());
    r.value.status.resize(frames.size());
    r.value.decoded.resize(frames.size());
    if (st != PBSGPU_OK) r.err = errorf("zstd decode", st);
    return r;
}

struct ZstdEncoded {
    std::vector<uint8_t> status;     // PBSGPU_ZSTD_OK or PBSGPU_ZSTD_BAD_SIZE per chunk
    std::vector<uint64_t> frameLen;  // the frame's length (0 unless OK)
};

// many chunks of a device buffer to one zstd frame each in one call: chunk i to dst + out[i].offset, which has
// out[i].length bytes of room (pbsgpu_zstd_encode_bound(length) always suffices): the writers of the reference that
// compress (internal/tapeio/converter.go:399, :410-435). A chunk whose status is PBSGPU_ZSTD_BAD_SIZE leaves unspecified
// bytes in its own room and nothing anywhere else.
inline Result<ZstdEncoded> EncodeZstd(pbsgpu_engine *eng, const void *src, uint64_t nbytes, const std::vector<pbsgpu_segment> &chunks,
                                      const std::vector<pbsgpu_segment> &out, void *dst, uint64_t dstCap) {
    Result<ZstdEncoded> r;
    if (out.size() != chunks.size()) {
        r.err = errorf("zstd encode", PBSGPU_E_INVALID);
        return r;
    }
    r.value.status.resize(chunks.size() + 1);
    r.value.frameLen.resize(chunks.size() + 1);
    const int st = pbsgpu_zstd_encode_device(eng, src, nbytes, chunks.data(), (uint32_t)chunks.size(), out.data(), dst, dstCap,
                                             r.value.status.data(), r.value.frameLen.data());
    r.value.status.resize(chunks.size());
    r.value.frameLen.resize(chunks.size());
    if (st != PBSGPU_OK) r.err = errorf("zstd encode", st);
    return r;
}

// DecodeZstd with flags (PBSGPU_ZSTD_F_CHECKSUM: a frame's content checksum is verified, PBSGPU_ZSTD_BAD_CHECKSUM;
// PBSGPU_ZSTD_F_STREAM: every segment is a whole zstd stream, decoded as ZSTD_decompress does it), for frames that are not
// blobs of an index. flags = 0 is DecodeZstd, output for output.
inline Result<ZstdDecoded> DecodeZstd2(pbsgpu_engine *eng, const void *src, uint64_t nbytes, const std::vector<pbsgpu_segment> &frames,
                                       const std::vector<pbsgpu_segment> &out, void *dst, uint64_t dstCap, uint32_t flags) {
    Result<ZstdDecoded> r;
    r.value.status.resize(frames.size() + 1);
    r.value.decoded.resize(frames.size() + 1);
    const int st = out.size() != frames.size() ? PBSGPU_E_INVALID
                 : pbsgpu_zstd_decode2_device(eng, src, nbytes, frames.data(), (uint32_t)frames.size(), out.data(), dst, dstCap,
                                              r.value.status.data(), r.value.decoded.data(), flags);
    r.value.status.resize(frames.size());
    r.value.decoded.resize(frames.size());
    if (st != PBSGPU_OK) r.err = errorf("zstd decode2", st);
    return r;
}

// EncodeZstd with flags (PBSGPU_ZSTD_F_CHECKSUM: every frame carries its content checksum, 4 bytes more; a room of
// pbsgpu_zstd_encode_bound2(length, flags) always suffices). flags = 0 is EncodeZstd.
inline Result<ZstdEncoded> EncodeZstd2(pbsgpu_engine *eng, const void *src, uint64_t nbytes, const std::vector<pbsgpu_segment> &chunks,
                                       const std::vector<pbsgpu_segment> &out, void *dst, uint64_t dstCap, uint32_t flags) {
    Result<ZstdEncoded> r;
    r.value.status.resize(chunks.size() + 1);
    r.value.frameLen.resize(chunks.size() + 1);
    const int st = out.size() != chunks.size() ? PBSGPU_E_INVALID
                 : pbsgpu_zstd_encode2_device(eng, src, nbytes, chunks.data(), (uint32_t)chunks.size(), out.data(), dst, dstCap,
                                              r.value.status.data(), r.value.frameLen.data(), flags);
    r.value.status.resize(chunks.size());
    r.value.frameLen.resize(chunks.size());
    if (st != PBSGPU_OK) r.err = errorf("zstd encode2", st);
    return r;
}

// XXH64 with `seed` of many ranges of a device buffer in one call: what a zstd frame's content checksum is the low 32 bits
// of (seed 0).
inline Result<std::vector<uint64_t>> XXH64Device(pbsgpu_engine *eng, const void *src, uint64_t nbytes,
                                                 const std::vector<pbsgpu_segment> &segs, uint64_t seed = 0) {
    Result<std::vector<uint64_t>> r;
    r.value.resize(segs.size() + 1);
    const int st = pbsgpu_xxh64_many_device(eng, src, nbytes, segs.data(), (uint32_t)segs.size(), seed, r.value.data());
    r.value.resize(segs.size());
    if (st != PBSGPU_OK) r.err = errorf("xxh64", st);
    return r;
}

struct ZstdStream {
    int status = 0;             // PBSGPU_ZSTD_* as the headers alone decide it
    uint64_t contentSize = 0;   // the sum over the frames; UINT64_MAX if a frame declares none
    uint32_t frames = 0, skippable = 0;
    bool anyChecksum = false;
};

// what the headers of a whole zstd stream declare (host only): sizes the destination of DecodeZstd2 with PBSGPU_ZSTD_F_STREAM
inline ZstdStream ZstdStreamInfo(const uint8_t *stream, uint64_t nbytes) {
    ZstdStream s;
    int any = 0;
    s.status = pbsgpu_zstd_stream_info(stream, nbytes, &s.contentSize, &s.frames, &s.skippable, &any);
    s.anyChecksum = any != 0;
    return s;
}

struct Encoded2 {
    std::vector<uint64_t> offsets;  // segs.size() + 1: blob i lies at offsets[i], in the slot the uncompressed layout gives it
    std::vector<uint32_t> lens;     // the blob's length: what is sent
    std::vector<uint8_t> kinds;     // PBSGPU_BLOB_UNCOMPRESSED or PBSGPU_BLOB_COMPRESSED
    std::vector<uint32_t> crcs;
    pbsgpu_encode_stats stats{};
};

// EncodeDevice with the blob's kind decided on the device (zstd = true: PBSGPU_ENCODE_F_ZSTD): a chunk whose frame is strictly
// shorter than the chunk becomes a compressed blob, every other one the uncompressed blob EncodeDevice writes.
inline Result<Encoded2> Encode2(pbsgpu_engine *eng, const void *src, uint64_t srcBytes, const std::vector<pbsgpu_segment> &segs,
                                bool zstd, void *dst, uint64_t dstCap) {
    Result<Encoded2> r;
    r.value.offsets.resize(segs.size() + 1);
    r.value.lens.resize(segs.size() + 1);
    r.value.kinds.resize(segs.size() + 1);
    r.value.crcs.resize(segs.size() + 1);
    const int st = pbsgpu_blob_encode2_device(eng, src, srcBytes, segs.data(), (uint32_t)segs.size(), zstd ? PBSGPU_ENCODE_F_ZSTD : 0u,
                                              dst, dstCap, r.value.offsets.data(), r.value.lens.data(), r.value.kinds.data(),
                                              r.value.crcs.data(), &r.value.stats);
    r.value.lens.resize(segs.size());
    r.value.kinds.resize(segs.size());
    r.value.crcs.resize(segs.size());
    if (st != PBSGPU_OK) r.err = errorf("blob encode2", st);
    return r;
}

// ---- AES-256-GCM (the cipher of the encrypted blob kinds), in batch on the device ----

// An AES-256 key on the device: round keys, hash key and multiplier tables (pbsgpu_aes_key_*). The 32 key bytes are not
// kept on the host; the destructor zeroes the device copy. Create() returns nullptr and sets *status on failure.
class AesKey {
public:
    static std::unique_ptr<AesKey> Create(pbsgpu_engine *eng, const uint8_t key[32], int *status = nullptr) {
        pbsgpu_aes_key *h = nullptr;
        const int st = pbsgpu_aes_key_create(eng, key, &h);
        if (status) *status = st;
        if (st != PBSGPU_OK) return nullptr;
        return std::unique_ptr<AesKey>(new AesKey(h));
    }
    ~AesKey() { pbsgpu_aes_key_destroy(h_); }
    AesKey(const AesKey &) = delete;
    AesKey &operator=(const AesKey &) = delete;
    pbsgpu_aes_key *handle() const { return h_; }

private:
    explicit AesKey(pbsgpu_aes_key *h) : h_(h) {}
    pbsgpu_aes_key *h_;
};

struct AesResult {
    std::vector<uint8_t> status;  // PBSGPU_AES_OK or PBSGPU_AES_BAD_TAG (output zeroed)
    std::vector<uint8_t> tags;    // 16 per message: as given when decrypting, as computed when encrypting
};

// Decrypt (flags 0; tags: 16 bytes per message) or encrypt (PBSGPU_AES_F_ENCRYPT; tags ignored, returned) many messages
// of a device buffer in one call. ivs: ivLen (12 or 16) bytes per message, the caller's in both directions.
inline Result<AesResult> AesGcmMany(const AesKey &key, const void *src, uint64_t nbytes, const std::vector<pbsgpu_segment> &msgs,
                                    const std::vector<uint8_t> &ivs, uint32_t ivLen, const std::vector<uint8_t> &tags,
                                    const std::vector<pbsgpu_segment> &out, void *dst, uint64_t dstCap, uint32_t flags) {
    Result<AesResult> r;
    const size_t n = msgs.size();
    r.value.status.resize(n + 1);
    r.value.tags.assign(16 * n + 16, 0);
    const bool enc = (flags & PBSGPU_AES_F_ENCRYPT) != 0;
    int st = PBSGPU_E_INVALID;
    if (out.size() == n && ivs.size() == (size_t)ivLen * n && (enc || tags.size() == 16 * n)) {
        if (!enc) std::copy(tags.begin(), tags.end(), r.value.tags.begin());
        st = pbsgpu_aes_gcm_many_device(key.handle(), src, nbytes, msgs.data(), (uint32_t)n, ivs.data(), ivLen, r.value.tags.data(),
                                        out.data(), dst, dstCap, r.value.status.data(), flags);
    }
    r.value.status.resize(n);
    r.value.tags.resize(16 * n);
    if (st != PBSGPU_OK) r.err = errorf("aes gcm", st);
    return r;
}

struct Decoded3 {
    std::vector<uint8_t> status;  // PBSGPU_BLOB_* per index entry, PBSGPU_BLOB_BAD_TAG included
    pbsgpu_decode_stats3 stats{};
};

// Decode2 with the encrypted blobs decrypted on the device under `key` (PBSGPU_DECODE_F_AES; key nullptr: Decode2, output
// for output): the restore loop of a datastore written with a key file. An encrypted-compressed blob needs zstd = true as
// well; PBSGPU_BLOB_BAD_TAG is a wrong key or a damaged blob. checkDigest is not applied to encrypted entries.
inline Result<Decoded3> Decode3(pbsgpu_engine *eng, const void *blobsDev, uint64_t nbytes,
                                const std::vector<pbsgpu_segment> &blobs, const std::vector<pbsgpu_record> &idx,
                                const std::vector<uint32_t> &blobOf, uint64_t rangeStart, uint64_t rangeEnd, bool checkDigest,
                                bool zstd, const AesKey *key, void *dst, uint64_t dstCap) {
    Result<Decoded3> r;
    r.value.status.resize(idx.size() + 1);
    const uint32_t flags = (checkDigest ? PBSGPU_DECODE_F_DIGEST : 0u) | (zstd ? PBSGPU_DECODE_F_ZSTD : 0u) |
                           (key ? PBSGPU_DECODE_F_AES : 0u);
    const int st = pbsgpu_blob_decode3_device(eng, blobsDev, nbytes, blobs.data(), (uint32_t)blobs.size(), idx.data(),
                                              idx.size(), blobOf.empty() ? nullptr : blobOf.data(), rangeStart, rangeEnd,
                                              flags, key ? key->handle() : nullptr, dst, dstCap, r.value.status.data(),
                                              &r.value.stats);
    r.value.status.resize(idx.size());
    if (st != PBSGPU_OK) r.err = errorf("blob decode3", st);
    return r;
}

struct Encoded3 {
    std::vector<uint64_t> offsets;  // segs.size() + 1: blob i lies at offsets[i], in a slot of 44 + length bytes with a key
    std::vector<uint32_t> lens;     // the blob's length: what is sent
    std::vector<uint8_t> kinds;     // PBSGPU_BLOB_UNCOMPRESSED .. PBSGPU_BLOB_ENCRYPTED_COMPRESSED
    std::vector<uint32_t> crcs;
    pbsgpu_encode_stats3 stats{};
};

// Encode2 with the blobs encrypted on the device under `key` (PBSGPU_ENCODE_F_AES; key nullptr: Encode2, output for output,
// ivs not looked at). ivs: 16 bytes per chunk, the caller's (pbsgpu_blob_encode3_device: two equal ones in a call are
// refused, uniqueness across calls is the caller's to answer for). Kind 2 holds the chunk, kind 3 (zstd = true and the frame
// strictly shorter than the chunk) its frame; the CRC covers the ciphertext.
inline Result<Encoded3> Encode3(pbsgpu_engine *eng, const void *src, uint64_t srcBytes, const std::vector<pbsgpu_segment> &segs,
                                bool zstd, const AesKey *key, const std::vector<uint8_t> &ivs, void *dst, uint64_t dstCap) {
    Result<Encoded3> r;
    const size_t n = segs.size();
    r.value.offsets.resize(n + 1);
    r.value.lens.resize(n + 1);
    r.value.kinds.resize(n + 1);
    r.value.crcs.resize(n + 1);
    int st = PBSGPU_E_INVALID;
    if (!key || ivs.size() == 16 * n) {
        const uint32_t flags = (zstd ? PBSGPU_ENCODE_F_ZSTD : 0u) | (key ? PBSGPU_ENCODE_F_AES : 0u);
        st = pbsgpu_blob_encode3_device(eng, src, srcBytes, segs.data(), (uint32_t)n, flags, key ? key->handle() : nullptr,
                                        key && n ? ivs.data() : nullptr, dst, dstCap, r.value.offsets.data(), r.value.lens.data(),
                                        r.value.kinds.data(), r.value.crcs.data(), &r.value.stats);
    }
    r.value.lens.resize(n);
    r.value.kinds.resize(n);
    r.value.crcs.resize(n);
    if (st != PBSGPU_OK) r.err = errorf("blob encode3", st);
    return r;
}

// ---- keyed chunk digests, SHA-256(content || id_key): what an encrypted backup's index calls a chunk ----

// The 32-byte id key on the device (pbsgpu_id_key_*). The bytes are not kept on the host; the destructor zeroes the device
// copy. Nothing is derived: the caller brings the 32 bytes. Create() returns nullptr and sets *status on failure.
class IdKey {
public:
    static std::unique_ptr<IdKey> Create(pbsgpu_engine *eng, const uint8_t idKey[32], int *status = nullptr) {
        pbsgpu_id_key *h = nullptr;
        const int st = pbsgpu_id_key_create(eng, idKey, &h);
        if (status) *status = st;
        if (st != PBSGPU_OK) return nullptr;
        return std::unique_ptr<IdKey>(new IdKey(h));
    }
    ~IdKey() { pbsgpu_id_key_destroy(h_); }
    IdKey(const IdKey &) = delete;
    IdKey &operator=(const IdKey &) = delete;
    pbsgpu_id_key *handle() const { return h_; }

private:
    explicit IdKey(pbsgpu_id_key *h) : h_(h) {}
    pbsgpu_id_key *h_;
};

// SHA-256(range || id_key) of many ranges of a device buffer in one call: 32 bytes per range
inline Result<std::vector<uint8_t>> Sha256KeyedMany(const IdKey &key, const void *dptr, uint64_t nbytes,
                                                    const std::vector<pbsgpu_segment> &segs) {
    Result<std::vector<uint8_t>> r;
    r.value.resize(32 * segs.size() + 32);
    const int st = pbsgpu_sha256_keyed_many_device(key.handle(), dptr, nbytes, segs.data(), (uint32_t)segs.size(), r.value.data());
    r.value.resize(32 * segs.size());
    if (st != PBSGPU_OK) r.err = errorf("sha256 keyed many", st);
    return r;
}

// The batch path with every record's digest keyed: a ticket for pbsgpu_collect. Cut points are those of the plain submit; keep
// the key alive until the ticket is collected.
inline Result<uint64_t> SubmitDeviceKeyed(pbsgpu_engine *eng, const IdKey &key, const void *dptr, uint64_t nbytes,
                                          const std::vector<pbsgpu_segment> &segs) {
    Result<uint64_t> r;
    const int st = pbsgpu_submit_device_keyed(eng, key.handle(), dptr, nbytes, segs.empty() ? nullptr : segs.data(),
                                              (uint32_t)segs.size(), &r.value);
    if (st != PBSGPU_OK) r.err = errorf("submit device keyed", st);
    return r;
}

// Decode3 with the keyed digest check: with a key, checkDigest and idKey, an entry of an encrypted kind that passed tag, frame
// and size is compared with SHA-256(plaintext || id_key); PBSGPU_BLOB_BAD_DIGEST on a mismatch, its bytes stay restored.
// idKey nullptr: Decode3, output for output.
inline Result<Decoded3> Decode4(pbsgpu_engine *eng, const void *blobsDev, uint64_t nbytes,
                                const std::vector<pbsgpu_segment> &blobs, const std::vector<pbsgpu_record> &idx,
                                const std::vector<uint32_t> &blobOf, uint64_t rangeStart, uint64_t rangeEnd, bool checkDigest,
                                bool zstd, const AesKey *key, const IdKey *idKey, void *dst, uint64_t dstCap) {
    Result<Decoded3> r;
    r.value.status.resize(idx.size() + 1);
    const uint32_t flags = (checkDigest ? PBSGPU_DECODE_F_DIGEST : 0u) | (zstd ? PBSGPU_DECODE_F_ZSTD : 0u) |
                           (key ? PBSGPU_DECODE_F_AES : 0u);
    const int st = pbsgpu_blob_decode4_device(eng, blobsDev, nbytes, blobs.data(), (uint32_t)blobs.size(), idx.data(),
                                              idx.size(), blobOf.empty() ? nullptr : blobOf.data(), rangeStart, rangeEnd,
                                              flags, key ? key->handle() : nullptr, idKey ? idKey->handle() : nullptr, dst,
                                              dstCap, r.value.status.data(), &r.value.stats);
    r.value.status.resize(idx.size());
    if (st != PBSGPU_OK) r.err = errorf("blob decode4", st);
    return r;
}

}  // namespace blob

// datastore.DynamicIndexReader
class DynamicIndexReader {
  public:
    int Count() const { return (int)recs_.size(); }
    // (info, ok)
    std::pair<ChunkInfo, bool> ChunkInfoAt(int i) const {
        ChunkInfo ci;
        if (i < 0 || i >= Count()) return {ci, false};
        ci.End = recs_[(size_t)i].end;
        std::memcpy(ci.Digest_.data(), recs_[(size_t)i].digest, 32);
        return {ci, true};
    }
    // index of the chunk containing `offset`; ok = false past the end (commit_reuse.go:89-92)
    std::pair<int, bool> ChunkFromOffset(uint64_t offset) const {
        size_t lo = 0, hi = recs_.size();
        while (lo < hi) {
            const size_t mid = (lo + hi) / 2;
            if (recs_[mid].end <= offset) lo = mid + 1; else hi = mid;
        }
        if (lo >= recs_.size()) return {0, false};
        return {(int)lo, true};
    }
    int64_t CTime() const { return ctime_; }
    const Digest &IndexCsum() const { return csum_; }
    const std::vector<pbsgpu_record> &Records() const { return recs_; }

  private:
    friend Result<std::shared_ptr<DynamicIndexReader>> ParseDynamicIndex(const std::vector<uint8_t> &data);
    std::vector<pbsgpu_record> recs_;
    int64_t ctime_ = 0;
    Digest csum_{};
};

// datastore.ParseDynamicIndex(data) (*DynamicIndexReader, error)
inline Result<std::shared_ptr<DynamicIndexReader>> ParseDynamicIndex(const std::vector<uint8_t> &data) {
    Result<std::shared_ptr<DynamicIndexReader>> r;
    uint64_t n = 0;
    int st = pbsgpu_didx_decode(data.data(), data.size(), nullptr, 0, &n, nullptr, nullptr);
    if (st != PBSGPU_OK && st != PBSGPU_E_CAPACITY) {
        r.err = errorf("parse dynamic index", st);
        return r;
    }
    auto idx = std::make_shared<DynamicIndexReader>();
    idx->recs_.resize((size_t)n);
    st = pbsgpu_didx_decode(data.data(), data.size(), idx->recs_.data(), n, &n, &idx->ctime_, idx->csum_.data());
    if (st != PBSGPU_OK) {
        r.err = errorf("parse dynamic index", st);
        return r;
    }
    r.value = std::move(idx);
    return r;
}

// datastore.NewDynamicIndexWriter(ctime).Add(end, digest).Finish() — the index checksum is computed
// by the engine's SHA-256 kernel, so Finish needs an engine.
class DynamicIndexWriter {
  public:
    explicit DynamicIndexWriter(int64_t ctime) : ctime_(ctime) {}
    void Add(uint64_t endOffset, const Digest &digest) {
        pbsgpu_record r{};
        r.end = endOffset;
        std::memcpy(r.digest, digest.data(), 32);
        r.size = (uint32_t)(endOffset - (recs_.empty() ? 0 : recs_.back().end));
        recs_.push_back(r);
    }
    Result<std::vector<uint8_t>> Finish(pbsgpu_engine *eng, const std::array<uint8_t, 16> &uuid = {}) {
        Result<std::vector<uint8_t>> r;
        uint64_t nb = 0;
        pbsgpu_didx_size(recs_.size(), &nb);
        r.value.resize((size_t)nb);
        const int st = pbsgpu_didx_encode(eng, recs_.data(), recs_.size(), uuid.data(), ctime_, r.value.data(), nb);
        if (st != PBSGPU_OK) {
            r.value.clear();
            r.err = errorf("finish dynamic index", st);
        }
        return r;
    }

  private:
    int64_t ctime_;
    std::vector<pbsgpu_record> recs_;
};

inline DynamicIndexWriter NewDynamicIndexWriter(int64_t ctime) { return DynamicIndexWriter(ctime); }

}  // namespace datastore

// One engine per (process, GPU): stands where backupproxy's store/session owns chunker + hasher.
class Engine {
  public:
    static Result<std::shared_ptr<Engine>> New(int device, const buzhash::Config &cfg, unsigned inflight = 2) {
        Result<std::shared_ptr<Engine>> r;
        pbsgpu_engine *h = nullptr;
        const int st = pbsgpu_engine_create(device, &cfg.c, inflight, &h);
        if (st != PBSGPU_OK) {
            r.err = errorf("engine create", st);
            return r;
        }
        r.value = std::shared_ptr<Engine>(new Engine(h));
        return r;
    }
    // ... with every per-engine tuning value (pbsgpu_engine_options, ABI v5; zero fields = the defaults). Among them
    // zstd_seq_tables = 1: blob::EncodeZstd, blob::Encode2 and the fused uploads of this engine write repeat offsets and
    // per-block sequence tables (shorter frames, never longer); and zstd_window_log = 17, 18 or 19: their blocks' matches may
    // start up to 2^log bytes in front of the block, within the chunk (far repeats are found; slower, and on content without
    // far repeats a frame may come out slightly longer).
    static Result<std::shared_ptr<Engine>> New(int device, const buzhash::Config &cfg, const pbsgpu_engine_options &opt) {
        Result<std::shared_ptr<Engine>> r;
        pbsgpu_engine *h = nullptr;
        const int st = pbsgpu_engine_create_opt(device, &cfg.c, &opt, &h);
        if (st != PBSGPU_OK) {
            r.err = errorf("engine create", st);
            return r;
        }
        r.value = std::shared_ptr<Engine>(new Engine(h));
        return r;
    }
    ~Engine() { pbsgpu_engine_destroy(h_); }
    pbsgpu_engine *handle() const { return h_; }

  private:
    explicit Engine(pbsgpu_engine *h) : h_(h) {}
    Engine(const Engine &) = delete;
    pbsgpu_engine *h_;
};

namespace transfer {

// The payload half of transfer.ArchiveWriter: WriteEntryReader pulls `size` bytes from a reader and
// appends them to the payload stream; finished chunks arrive at the sink in stream order as
// (ChunkInfo, size) — exactly what the session appends to the .ppxar.didx.
class PayloadWriter {
  public:
    using Sink = std::function<void(const datastore::ChunkInfo &, uint32_t size)>;

    static Result<std::unique_ptr<PayloadWriter>> New(std::shared_ptr<Engine> eng, Sink sink, uint64_t windowBytes = 0) {
        Result<std::unique_ptr<PayloadWriter>> r;
        pbsgpu_stream *s = nullptr;
        const int st = pbsgpu_stream_create(eng->handle(), windowBytes, &s);
        if (st != PBSGPU_OK) {
            r.err = errorf("stream create", st);
            return r;
        }
        r.value.reset(new PayloadWriter(std::move(eng), s, std::move(sink)));
        return r;
    }
    ~PayloadWriter() { pbsgpu_stream_destroy(s_); }

    // WriteEntryReader(entry, r, size) error — reads exactly `size` bytes from r (zero-copy into the
    // library's pinned staging), error on a short read like the Go writer
    std::string WriteEntryReader(std::istream &r, uint64_t size) {
        uint64_t left = size;
        while (left) {
            void *buf = nullptr;
            size_t cap = 0;
            int st = pbsgpu_stream_reserve(s_, &buf, &cap);
            if (st != PBSGPU_OK) return errorf("write entry", st);
            const size_t want = (size_t)std::min<uint64_t>(cap, left);
            r.read(static_cast<char *>(buf), (std::streamsize)want);
            const size_t got = (size_t)r.gcount();
            st = pbsgpu_stream_commit(s_, got);
            if (st != PBSGPU_OK) return errorf("write entry", st);
            left -= got;
            if (got < want) return "write entry: unexpected EOF";
            if (std::string e = drain(); !e.empty()) return e;
        }
        return {};
    }
    // The whole payload half of ArchiveWriter.WriteEntryReader for a regular file: 16-byte pxar payload header, `size`
    // bytes from r (zero-copy), per-file XXH3-64 tee (writeBackedFile, commit_reuse.go:427-468). *payloadOffset = the
    // header's payload position (what WriteEntryRef / PAYLOAD_REF records, commit_walk.go:455); the hash arrives
    // later through BackedHashes() under *fileIndex.
    std::string WritePayloadEntry(std::istream &r, uint64_t size, uint64_t *payloadOffset, uint64_t *fileIndex) {
        int st = pbsgpu_stream_begin_entry(s_, nullptr, size, payloadOffset);
        if (st != PBSGPU_OK) return errorf("begin entry", st);
        if (std::string e = WriteEntryReader(r, size); !e.empty()) return e;
        st = pbsgpu_stream_end_entry(s_, fileIndex);
        return st == PBSGPU_OK ? drain() : errorf("end entry", st);
    }
    std::string WriteMarker(bool tail) {
        const int st = pbsgpu_stream_write_marker(s_, nullptr, tail ? 1 : 0);
        return st == PBSGPU_OK ? std::string() : errorf("write marker", st);
    }
    // backedHashes (commit_reuse.go:461): (file index, size, XXH3-64) of every file whose last byte has been cut
    std::vector<pbsgpu_file_hash> BackedHashes() {
        std::vector<pbsgpu_file_hash> out;
        pbsgpu_file_hash buf[256];
        for (;;) {
            uint64_t n = 0;
            if (pbsgpu_stream_poll_files(s_, buf, 256, &n) != PBSGPU_OK) break;
            out.insert(out.end(), buf, buf + n);
            if (n < 256) break;
        }
        return out;
    }
    // WriteEntry(entry, content []byte)
    std::string WriteEntry(const void *data, size_t len) {
        const int st = pbsgpu_stream_write(s_, data, len);
        if (st != PBSGPU_OK) return errorf("write entry", st);
        return drain();
    }
    // InjectChunks(refs): the open chunk is flushed, offsets skip the injected payload (commit_reuse.go:315-341)
    std::string InjectChunks(const std::vector<datastore::KnownChunkRef> &refs) {
        uint64_t total = 0;
        for (const auto &k : refs) total += k.Size;
        const int st = pbsgpu_stream_cut(s_, total);
        if (st != PBSGPU_OK) return errorf("inject chunks", st);
        return drain();
    }
    // Encoder().PayloadPosition() (commit_reuse.go:265): payload bytes written PLUS bytes injected so far — the
    // coordinate system of PAYLOAD_REF offsets and of the records' End (InjectChunks advances the position:
    // keepLast_chunk_test.go mock, enc.Advance(total))
    uint64_t PayloadPosition() const {
        uint64_t n = 0;
        pbsgpu_stream_position(s_, &n);
        return n;
    }
    // payload chunker: suggest a chunk boundary at the current position ("a file starts here"); taken when the open
    // chunk is then within [min, max], see pbsgpu_submit_device_suggested
    std::string SuggestBoundary() {
        const int st = pbsgpu_stream_suggest(s_, PayloadPosition());
        return st == PBSGPU_OK ? std::string() : errorf("suggest boundary", st);
    }
    std::string Finish() {
        const int st = pbsgpu_stream_finish(s_);
        if (st != PBSGPU_OK) return errorf("finish", st);
        return drain();
    }
    // the same in two steps, for a writer that starts its next archive while this one's last chunks are hashed:
    // FinishBegin closes the input and returns; Done() delivers what has arrived to the sink and reports whether the
    // last entry is out (never blocks)
    std::string FinishBegin() {
        const int st = pbsgpu_stream_finish_begin(s_);
        return st == PBSGPU_OK ? std::string() : errorf("finish begin", st);
    }
    Result<bool> Done() {
        Result<bool> r;
        int d = 0;
        const int st = pbsgpu_stream_done(s_, &d);
        if (st != PBSGPU_OK) {
            r.err = errorf("done", st);
            return r;
        }
        r.err = drain();
        r.value = d != 0;
        return r;
    }

    // ---- held pages (PBSGPU_HAS_STREAM_UPLOAD) ----
    // Hold: the writer keeps its pages until Release, so that UploadNewChunks can frame the new chunks of what it was given
    // straight out of them. Only before the first byte, marker or cut. The loop: WriteEntry... -> TakePolled -> UploadNewChunks
    // -> upload the blobs -> Release(last end). A call that needs a page then fails with PBSGPU_E_BUSY ("busy") instead of
    // waiting for a page only Release can bring; no byte is lost (WriteEntry: BytesWritten() names the prefix taken).
    std::string Hold() {
        const int st = pbsgpu_stream_hold(s_);
        if (st == PBSGPU_OK) holding_ = true;
        return st == PBSGPU_OK ? std::string() : errorf("stream hold", st);
    }
    // the entries delivered to the sink since the last call, as pbsgpu_stream_poll returned them (a holding writer only)
    std::vector<pbsgpu_record> TakePolled() {
        std::vector<pbsgpu_record> out;
        out.swap(polled_);
        return out;
    }
    uint64_t BytesWritten() const {
        uint64_t n = 0;
        pbsgpu_stream_bytes_written(s_, &n);
        return n;
    }
    // PageRing's fused call with the blob's kind decided on the device, for entries of this writer as TakePolled returned them
    Result<datastore::Uploaded2> UploadNewChunks(datastore::KnownChunks &known, const std::vector<pbsgpu_record> &recs, bool insert,
                                            bool zstd, void *dst, uint64_t dstCap) {
        Result<datastore::Uploaded2> r;
        datastore::Uploaded2 &v = r.value;
        v.Resize(recs.size());
        const int st = pbsgpu_stream_upload_new2_device(s_, known.Handle(), recs.data(), recs.size(), insert ? 1 : 0,
                                                        zstd ? PBSGPU_ENCODE_F_ZSTD : 0u, dst, dstCap, v.known.data(),
                                                        v.offsets.data(), v.lens.data(), v.kinds.data(), v.crcs.data(), &v.bytes,
                                                        &v.stats, &v.encoded);
        if (st != PBSGPU_OK) r.err = errorf("stream upload new2", st);
        return r;
    }
    // the payload below position `upto` (at most the end of the last delivered entry) is no longer needed
    std::string Release(uint64_t upto) {
        const int st = pbsgpu_stream_release(s_, upto);
        return st == PBSGPU_OK ? std::string() : errorf("stream release", st);
    }
    std::string Held(uint64_t *firstPosition, uint32_t *pagesHeld, uint32_t *ringPagesFree = nullptr) {
        const int st = pbsgpu_stream_held(s_, firstPosition, pagesHeld, ringPagesFree);
        return st == PBSGPU_OK ? std::string() : errorf("stream held", st);
    }
    // the raw payload bytes [position, position + length) into device buffer dst
    std::string Copy(uint64_t position, uint64_t length, void *dst) {
        const int st = pbsgpu_stream_copy_device(s_, position, length, dst);
        return st == PBSGPU_OK ? std::string() : errorf("stream copy", st);
    }

  private:
    PayloadWriter(std::shared_ptr<Engine> e, pbsgpu_stream *s, Sink sink) : eng_(std::move(e)), s_(s), sink_(std::move(sink)) {}
    std::string drain() {
        pbsgpu_record buf[256];
        for (;;) {
            uint64_t n = 0;
            const int st = pbsgpu_stream_poll(s_, buf, 256, &n);
            if (st != PBSGPU_OK) return errorf("poll", st);
            for (uint64_t i = 0; i < n; ++i) {
                datastore::ChunkInfo ci;
                ci.End = buf[i].end;
                std::memcpy(ci.Digest_.data(), buf[i].digest, 32);
                sink_(ci, buf[i].size);
            }
            if (holding_) polled_.insert(polled_.end(), buf, buf + n);
            if (n < 256) return {};
        }
    }
    std::shared_ptr<Engine> eng_;
    pbsgpu_stream *s_;
    Sink sink_;
    bool holding_ = false;
    std::vector<pbsgpu_record> polled_;
};

// Several archives at once on bytes that are (or arrive) in device memory: the page ring (pbsgpu_ring_*). One writer
// per archive in the reference (commit_reuse.go:457, converter.go:836); here each archive is a stream of the ring and
// the sink receives its (End, Digest) entries in stream order. One thread drives a PageRing.
class PageRing {
  public:
    using Sink = std::function<void(uint32_t stream, const datastore::ChunkInfo &, uint32_t size)>;

    static Result<std::unique_ptr<PageRing>> New(std::shared_ptr<Engine> eng, Sink sink, const pbsgpu_ring_options *opt = nullptr) {
        Result<std::unique_ptr<PageRing>> r;
        pbsgpu_ring *h = nullptr;
        const int st = pbsgpu_ring_create(eng->handle(), opt, &h);
        if (st != PBSGPU_OK) {
            r.err = errorf("ring create", st);
            return r;
        }
        r.value.reset(new PageRing(std::move(eng), h, std::move(sink)));
        return r;
    }
    ~PageRing() { pbsgpu_ring_destroy(r_); }

    Result<uint32_t> Open() {
        Result<uint32_t> r;
        const int st = pbsgpu_ring_open(r_, &r.value);
        if (st != PBSGPU_OK) r.err = errorf("ring open", st);
        return r;
    }
    // the stream's next page (device pointer, capacity); value.first == nullptr when no page is free right now
    Result<std::pair<void *, uint64_t>> Reserve(uint32_t stream) {
        Result<std::pair<void *, uint64_t>> r;
        r.value = {nullptr, 0};
        const int st = pbsgpu_ring_reserve(r_, stream, &r.value.first, &r.value.second);
        if (st != PBSGPU_OK && st != PBSGPU_E_BUSY) r.err = errorf("ring reserve", st);
        if (st == PBSGPU_E_BUSY) r.value = {nullptr, 0};
        return r;
    }
    std::string Commit(uint32_t stream, uint64_t nbytes, bool final) {
        const int st = pbsgpu_ring_commit(r_, stream, nbytes, final ? 1 : 0);
        return st == PBSGPU_OK ? std::string() : errorf("ring commit", st);
    }
    // synthetic producer (benchmarks / tests): bytes accepted
    Result<uint64_t> FillSynthetic(uint32_t stream, uint64_t seed, uint32_t kind, uint64_t nbytes, bool final) {
        Result<uint64_t> r;
        const int st = pbsgpu_ring_fill(r_, stream, seed, kind, nbytes, final ? 1 : 0, &r.value);
        if (st != PBSGPU_OK) r.err = errorf("ring fill", st);
        return r;
    }
    // enqueue what has been committed, deliver finished entries of `stream` to the sink; *done: the stream has ended
    // and everything has been delivered
    std::string Pump(uint32_t stream, bool *done) {
        int st = pbsgpu_ring_pump(r_);
        if (st != PBSGPU_OK) return errorf("ring pump", st);
        pbsgpu_record buf[256];
        for (;;) {
            uint64_t n = 0;
            int fin = 0;
            st = pbsgpu_ring_poll(r_, stream, buf, 256, &n, &fin);
            if (st != PBSGPU_OK) return errorf("ring poll", st);
            for (uint64_t i = 0; i < n; ++i) {
                datastore::ChunkInfo ci;
                ci.End = buf[i].end;
                std::memcpy(ci.Digest_.data(), buf[i].digest, 32);
                sink_(stream, ci, buf[i].size);
            }
            if (done) *done = fin != 0;
            if (n < 256) return {};
        }
    }
    std::string CloseStream(uint32_t stream) {
        const int st = pbsgpu_ring_close(r_, stream);
        return st == PBSGPU_OK ? std::string() : errorf("ring close", st);
    }
    std::string Quiesce() {
        const int st = pbsgpu_ring_quiesce(r_);
        return st == PBSGPU_OK ? std::string() : errorf("ring quiesce", st);
    }
    // Quiesce without the wait: for a writer about to sit in a blocking read (internal/tapeio/converter.go:672-680)
    std::string Park() {
        const int st = pbsgpu_ring_park(r_);
        return st == PBSGPU_OK ? std::string() : errorf("ring park", st);
    }
    // a suggested chunk boundary `offset` bytes into the stream ("a file starts here"), announced ahead of its bytes
    std::string Suggest(uint32_t stream, uint64_t offset) {
        const int st = pbsgpu_ring_suggest(r_, stream, offset);
        return st == PBSGPU_OK ? std::string() : errorf("ring suggest", st);
    }
    // {CUs of the express service (two lanes per chunk, the longest chunks), chunk size from which a chunk takes it}; {0, 0}: none
    std::pair<uint32_t, uint64_t> Express() const {
        std::pair<uint32_t, uint64_t> r{0, 0};
        (void)pbsgpu_ring_express(r_, &r.first, &r.second);
        return r;
    }

    // cumulative regime counters of the two services (ns per block step under load, shader clock): pbsgpu_ring_get_probe
    pbsgpu_ring_probe Probe() const {
        pbsgpu_ring_probe p{};
        (void)pbsgpu_ring_get_probe(r_, &p);
        return p;
    }

    // ---- held pages (a ring created with PBSGPU_RING_F_HOLD_PAGES in its options' flags): the upload side, beside
    // datastore::blob. The holder must Release, or the ring stalls like a full arena.
    // the stream's bytes below `upto` (at most the End of its last delivered entry) are no longer needed
    std::string Release(uint32_t stream, uint64_t upto) {
        const int st = pbsgpu_ring_release(r_, stream, upto);
        return st == PBSGPU_OK ? std::string() : errorf("ring release", st);
    }
    // {stream offset from which bytes are still available, handed-back pages the stream is holding}
    Result<std::pair<uint64_t, uint32_t>> Held(uint32_t stream) {
        Result<std::pair<uint64_t, uint32_t>> r;
        r.value = {0, 0};
        const int st = pbsgpu_ring_held(r_, stream, &r.value.first, &r.value.second);
        if (st != PBSGPU_OK) r.err = errorf("ring held", st);
        return r;
    }
    // uncompressed blobs of the delivered entries recs (skip[i] != 0: entry i is known, leave it out; skip may be empty),
    // straight out of the ring's pages, back to back in device buffer dst. offsets[i] / crcs[i] per kept entry; `bytes`
    // is what was written — or, with a dst that is too small (an error, nothing written), what is needed.
    // stream == PBSGPU_RING_ANY_STREAM: every entry's stream is its `segment`.
    Result<datastore::blob::Encoded> EncodeBlobs(uint32_t stream, const std::vector<pbsgpu_record> &recs,
                                                 const std::vector<uint8_t> &skip, void *dst, uint64_t dstCap) {
        Result<datastore::blob::Encoded> r;
        r.value.offsets.assign(recs.size(), 0);
        r.value.crcs.assign(recs.size(), 0);
        if (!skip.empty() && skip.size() != recs.size()) {
            r.err = errorf("ring blob encode", PBSGPU_E_INVALID);
            return r;
        }
        const int st = pbsgpu_ring_blob_encode_device(r_, stream, recs.data(), recs.size(), skip.empty() ? nullptr : skip.data(),
                                                      dst, dstCap, r.value.offsets.data(), r.value.crcs.data(), &r.value.bytes);
        if (st != PBSGPU_OK) r.err = errorf("ring blob encode", st);
        return r;
    }
    // Classify + EncodeBlobs(skip = known) in one device-side call: the delivered entries recs are classified against
    // `known` and the new ones framed out of the ring's pages; the flags never leave the device in between.
    Result<datastore::Uploaded> UploadNew(datastore::KnownChunks &known, uint32_t stream, const std::vector<pbsgpu_record> &recs,
                                          bool insert, void *dst, uint64_t dstCap) {
        Result<datastore::Uploaded> r;
        r.value.known.assign(recs.size(), 0);
        r.value.offsets.assign(recs.size(), 0);
        r.value.crcs.assign(recs.size(), 0);
        const int st = pbsgpu_ring_upload_new_device(r_, known.Handle(), stream, recs.data(), recs.size(), insert ? 1 : 0, dst,
                                                     dstCap, r.value.known.data(), r.value.offsets.data(),
                                                     r.value.crcs.data(), &r.value.bytes, &r.value.stats);
        if (st != PBSGPU_OK) r.err = errorf("ring upload new", st);
        return r;
    }
    // UploadNew for the writers that compress: the new chunks become compressed blobs where their frames are strictly
    // shorter, straight out of the ring's pages (a chunk in two pages is one chunk to the encoder).
    Result<datastore::Uploaded2> UploadNew2(datastore::KnownChunks &known, uint32_t stream, const std::vector<pbsgpu_record> &recs,
                                            bool insert, bool zstd, void *dst, uint64_t dstCap) {
        Result<datastore::Uploaded2> r;
        datastore::Uploaded2 &v = r.value;
        v.Resize(recs.size());
        const int st = pbsgpu_ring_upload_new2_device(r_, known.Handle(), stream, recs.data(), recs.size(), insert ? 1 : 0,
                                                      zstd ? PBSGPU_ENCODE_F_ZSTD : 0u, dst, dstCap, v.known.data(), v.offsets.data(),
                                                      v.lens.data(), v.kinds.data(), v.crcs.data(), &v.bytes, &v.stats, &v.encoded);
        if (st != PBSGPU_OK) r.err = errorf("ring upload new2", st);
        return r;
    }
    // the raw stream bytes [offset, offset + length) into device buffer dst
    std::string Copy(uint32_t stream, uint64_t offset, uint64_t length, void *dst) {
        const int st = pbsgpu_ring_copy_device(r_, stream, offset, length, dst);
        return st == PBSGPU_OK ? std::string() : errorf("ring copy", st);
    }

  private:
    PageRing(std::shared_ptr<Engine> eng, pbsgpu_ring *r, Sink sink) : eng_(std::move(eng)), r_(r), sink_(std::move(sink)) {}
    PageRing(const PageRing &) = delete;
    std::shared_ptr<Engine> eng_;
    pbsgpu_ring *r_;
    Sink sink_;
};

}  // namespace transfer

// The cross-GPU digest-set reduce (pbsgpu_comm_*): one Engine per GPU ingests its own archives (the reference runs one
// session per process, internal/tapeio/converter.go:396-439), the (digest, size) records of all ranks meet in ONE RCCL
// all-gather + device dedup. Every call is collective: all ranks, same order.
namespace distributed {

using CommID = std::array<uint8_t, PBSGPU_COMM_ID_BYTES>;

inline Result<CommID> NewCommID() {  // rank 0 only; ship the bytes to the other ranks
    Result<CommID> r;
    const int st = pbsgpu_comm_unique_id(r.value.data());
    if (st != PBSGPU_OK) r.err = errorf("comm unique id", st);
    return r;
}

inline std::string CommLastError() { return pbsgpu_comm_last_error(); }  // RCCL's own words for the last failure

class Comm {
  public:
    static Result<std::unique_ptr<Comm>> New(std::shared_ptr<Engine> eng, const CommID &id, int rank, int world) {
        Result<std::unique_ptr<Comm>> r;
        pbsgpu_comm *h = nullptr;
        const int st = pbsgpu_comm_create(eng->handle(), id.data(), rank, world, &h);
        if (st != PBSGPU_OK) {
            r.err = errorf("comm create", st);
            return r;
        }
        r.value.reset(new Comm(std::move(eng), h));
        return r;
    }
    ~Comm() { pbsgpu_comm_destroy(c_); }
    // this rank's records in, the statistics of the union out; dup[i] = an earlier record of the union has recs[i]'s digest
    Result<pbsgpu_dedup_stats> Dedup(const std::vector<pbsgpu_record> &recs, uint64_t cap_records, std::vector<uint8_t> *dup = nullptr) {
        Result<pbsgpu_dedup_stats> r;
        if (dup) dup->assign(recs.size(), 0);
        const int st = pbsgpu_digest_allgather_dedup(c_, recs.empty() ? nullptr : recs.data(), recs.size(), cap_records,
                                                     dup && !recs.empty() ? dup->data() : nullptr, &r.value);
        if (st != PBSGPU_OK) r.err = errorf("digest all-gather + dedup", st);
        return r;
    }

  private:
    Comm(std::shared_ptr<Engine> eng, pbsgpu_comm *c) : eng_(std::move(eng)), c_(c) {}
    Comm(const Comm &) = delete;
    std::shared_ptr<Engine> eng_;
    pbsgpu_comm *c_;
};

}  // namespace distributed
}  // namespace pbsgpu
