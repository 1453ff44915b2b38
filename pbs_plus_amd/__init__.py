"""pbs_plus_amd — MI355X-native content-defined chunker + SHA-256 dedup-hash engine.

Host-side mirror (Python over the C ABI in include/pbsgpu.h) of the interface the
pbs-plus reference uses for its pxar stream path:

* ``buzhash.NewConfig`` / ``buzhash.Config`` — github.com/pbs-plus/pxar ``buzhash``
  (reference internal/pxarmount/commit_orchestrate.go:143-149, internal/tapeio/converter.go:248)
* ``Engine`` — batch cut + digest (the chunk loop behind ``WriteEntryReader``)
* ``PayloadStream`` — the payload-stream writer seam (``transfer.ArchiveWriter``)
* ``PageRing`` — many streams, page-granular memory release, persistent SHA-256 service
* ``Chunker`` — upstream-style ``scan`` compatibility
* ``didx`` / ``dedup`` / ``Comm`` — dynamic index records and the cross-GPU digest-set reduce (RCCL, behind the C ABI)
* ``KnownChunks`` — the device-resident known-chunk set of an incremental session (which chunks to upload)
* ``Engine.crc32_many`` / ``blob_encode`` / ``blob_verify`` — data-blob framing of the uploads and the chunk check
  (``chunk_ranges`` turns records into the byte ranges of their chunks)
* ``Engine.zstd_decode`` / ``zstd_frame_info`` — the zstd frames behind the compressed blobs, decoded on the device
* ``Engine.zstd_encode`` / ``blob_encode2`` / ``zstd_encode_bound`` — chunks compressed to zstd frames on the device and
  framed as blobs whose kind the device decides
* ``Engine.zstd_decode2`` / ``zstd_encode2`` / ``xxh64_many`` / ``zstd_stream_info`` / ``zstd_encode_bound2`` — the frame's
  content checksum verified and written, whole zstd streams decoded, for frames that are not blobs of an index
* ``AesKey`` / ``Engine.aes_gcm_many`` / ``Engine.blob_decode3`` — AES-256-GCM, the cipher of the encrypted blob kinds, on
  the device: in batch in both directions, and inside the restore
* ``IdKey`` / ``Engine.sha256_keyed_many`` / ``Engine.chunk_and_digest(id_key=)`` / ``Engine.blob_decode4`` — the keyed chunk
  digest SHA-256(content || id_key) of an encrypted backup's index: in batch, on the batch path, and checked in the restore

Everything executes in the gfx950 kernels of ``lib/libpbsgpu.so``; there is no CPU path.
"""
from . import buzhash  # noqa: F401
from ._lib import RECORD_DTYPE, PbsGpuError  # noqa: F401
from .engine import AesKey, IdKey, Chunker, Comm, Engine, KnownChunks, PageRing, PayloadStream  # noqa: F401
from .engine import blob_index, blob_magic, chunk_ranges, crc32_combine, zstd_encode_bound, zstd_frame_info  # noqa: F401
from .engine import zstd_encode_bound2, zstd_stream_info  # noqa: F401

__all__ = ["buzhash", "Engine", "PayloadStream", "PageRing", "Chunker", "Comm", "KnownChunks", "RECORD_DTYPE", "PbsGpuError",
           "blob_index", "blob_magic", "chunk_ranges", "crc32_combine", "zstd_encode_bound", "zstd_frame_info",
           "zstd_encode_bound2", "zstd_stream_info", "AesKey", "IdKey"]
