// What pbsgpu_zstd_decode2_device adds to the frame decoder of zstd_decode.h (include/pbsgpu.h): the
// content checksum verified, and a whole zstd stream decoded the way ZSTD_decompress does it. ONE implementation,
// compiled twice like the headers it builds on: k_zstd_frames2 (zstd_checksum.hip) runs it with one wave per segment, the
// CPU build is what tests/native/test_zstd_checksum.cpp runs under AddressSanitizer, and pbsgpu_zstd_stream_info
// (hostonly.cpp) uses the header walk.
//
// Decisions:
//   * A checksum is verified after everything else about its frame is OK (libzstd's order), over the frame's output where
//     it lies in the destination, by xxh64.h on the first four lanes. A mismatch is BAD_CHECKSUM.
//   * A stream is frames one behind the other. Skippable frames (magic 0x184D2A5?, a 4-byte length) are skipped; no
//     bytes, or skippable frames alone, are OK with nothing decoded. The status is that of the first frame that is not
//     OK; a skippable frame cut short, fewer than four bytes behind a frame, or bytes that start no frame are BAD_FRAME.
//   * Every frame is decoded on its own: an offset may not reach in front of ITS frame's first output byte. libzstd's
//     one-shot call lets a later frame reach into the output of the frame before it; that is a deliberate difference.
//   * The room is the stream's: each frame gets what the frames before it left.
#pragma once

#include "xxh64.h"
#include "zstd_decode.h"

namespace pbsz {

enum : int { BAD_CHECKSUM = 4 };
enum : uint32_t { F_CHECKSUM = 1, F_STREAM = 2 };  // = PBSGPU_ZSTD_F_*

PBSZ_HD bool skippable_magic(uint32_t magic) { return (magic & 0xfffffff0u) == 0x184d2a50u; }

// the frame just decoded to dst[0, decoded): its checksum, if it has one and the caller asked
template <class P>
PBSZ_HD int verify_frame(const FrameEnd &end, const uint8_t *dst, uint32_t decoded, uint32_t flags, uint64_t *box) {
    if (!end.has_checksum) {
        PBSZ_COV2(K_SUM_ABSENT);
        return OK;
    }
    if (!(flags & F_CHECKSUM)) {
        PBSZ_COV2(K_SUM_NOT_ASKED);
        return OK;
    }
    const uint32_t low = P::uni((uint32_t)xxh64<P>(dst, decoded, 0, box));
    PBSZ_COV2(low == end.checksum ? K_SUM_GOOD : K_SUM_BAD);
    return low == P::uni(end.checksum) ? OK : BAD_CHECKSUM;
}

// The walk over a segment, shared by the lanes (LDS in the kernel): where the next frame starts, what has been decoded,
// the flags, and the five words of xxh64. It is kept here and not in the caller's registers: the kernel's frame decoder
// leaves no scalar register free, and what a caller holds across it would be spilled.
struct Walk {
    uint64_t box[5];
    uint32_t pos, out, flags, nframes;
};
enum : int { MORE = -1 };

template <class P>
PBSZ_HD void walk_begin(Walk &w, uint32_t flags) {
    if (P::lane() == 0) {
        w.pos = w.out = w.nframes = 0;
        w.flags = flags;
    }
    P::sync();
}

// One step of the walk over src[0, n) into dst[0, room): a skippable frame skipped or a frame decoded (and verified, if
// asked). MORE: call again with the same arguments; anything else is the segment's status, and with OK w.out is what was
// decoded. Without F_STREAM the one step is the one frame.
template <class P>
PBSZ_HD int walk_step(State &st, const uint8_t *src, uint32_t n, uint8_t *dst, uint32_t room, uint8_t *lit, Walk &w) {
    const uint32_t pos = P::uni(w.pos), out = P::uni(w.out);
    const bool stream = (P::uni(w.flags) & F_STREAM) != 0;
    if (stream) {
        if (pos == n) {
            PBSZ_COV2(n == 0 ? K_STREAM_EMPTY : out == 0 ? K_STREAM_NO_FRAME : K_STREAM_FRAME);
            return OK;
        }
        if (n - pos < 4) {
            PBSZ_COV2(K_STREAM_SHORT_TAIL);
            return BAD_FRAME;
        }
        if (skippable_magic((uint32_t)uload<P>(src + pos, 4))) {
            if (n - pos < 8 || n - pos - 8 < (uint32_t)uload<P>(src + pos + 4, 4)) {
                PBSZ_COV2(K_STREAM_SKIPPABLE_CUT);
                return BAD_FRAME;
            }
            PBSZ_COV2(K_STREAM_SKIPPABLE);
            P::sync();  // every lane has read w.pos
            if (P::lane() == 0) w.pos = pos + 8 + (uint32_t)load_le(src + pos + 4, 4);
            P::sync();
            return MORE;
        }
        if (P::uni(w.nframes)) PBSZ_COV2(K_STREAM_SECOND_FRAME);
    } else {
        PBSZ_COV2(K_ONE_FRAME);
    }
    FrameEnd end;
    uint32_t got = 0;
    uint8_t *to = dst + out;
    int r = decode_frame_at<P, false>(st, src + pos, n - pos, to, room - out, lit, &got, end);
    // the one frame of a segment that is no stream ends where the segment ends (decode_frame's order: before the size)
    if (!(P::uni(w.flags) & F_STREAM) && P::uni(end.used) && P::uni(end.used) != n) r = UNSUPPORTED;
    if (!r) r = verify_frame<P>(end, to, got, P::uni(w.flags), w.box);
    if (r) {
        if (P::uni(w.flags) & F_STREAM) PBSZ_COV2(K_STREAM_FRAME_FAILS);
        return r;
    }
    P::sync();  // every lane has read w.pos and w.out
    if (P::lane() == 0) {
        w.pos += end.used;
        w.out += got;
        w.nframes += 1;
    }
    P::sync();
    return (P::uni(w.flags) & F_STREAM) ? (int)MORE : (int)OK;
}

// src[0, n) into dst[0, room) as `flags` say: one frame, or with F_STREAM a stream. Otherwise as decode_frame: *decoded =
// bytes produced (valid with OK, 0 otherwise); never loads outside src[0, n), never stores outside dst[0, room) and
// lit[0, kLitMax). (The kernel makes the same steps and reads the segment's place anew before each.)
template <class P>
PBSZ_HD int decode2(State &st, const uint8_t *src, uint32_t n, uint8_t *dst, uint32_t room, uint8_t *lit, uint32_t flags,
                    Walk &w, uint32_t *decoded) {
    *decoded = 0;
    walk_begin<P>(w, flags);
    int r;
    do r = walk_step<P>(st, src, n, dst, room, lit, w);
    while (r == MORE);
    if (r == OK) *decoded = P::uni(w.out);
    return r;
}

// The headers of a stream alone, for sizing: frames and skippable frames counted, content sizes summed (kNoSize as soon
// as one frame declares none). BAD_FRAME / UNSUPPORTED as decode2 would answer from the headers alone: a frame's end is
// found by walking its blocks' headers, nothing is decoded. The counts hold up to a failure.
inline int stream_info(const uint8_t *src, uint64_t n, uint64_t *content, uint32_t *nframes, uint32_t *nskip, int *any_sum) {
    *content = 0;
    *nframes = *nskip = 0;
    *any_sum = 0;
    uint64_t pos = 0;
    while (pos < n) {
        if (n - pos < 4) return BAD_FRAME;
        if (skippable_magic((uint32_t)load_le(src + pos, 4))) {
            if (n - pos < 8 || n - pos - 8 < load_le(src + pos + 4, 4)) return BAD_FRAME;
            pos += 8 + load_le(src + pos + 4, 4);
            ++*nskip;
            continue;
        }
        FrameHeader h;
        const int r = parse_frame_header(src + pos, n - pos, h);
        if (r) return r;
        ++*nframes;
        *any_sum |= (int)h.has_checksum;
        if (h.content_size == kNoSize || *content == kNoSize || *content + h.content_size < *content) *content = kNoSize;
        else *content += h.content_size;  // (a sum past 2^64 is not known either)
        pos += h.header_bytes;
        for (;;) {  // the blocks by their headers
            if (n - pos < 3) return BAD_FRAME;
            const uint32_t bh = (uint32_t)load_le(src + pos, 3);
            const uint32_t type = (bh >> 1) & 3u, bsize = bh >> 3;
            if (type == 3 || bsize > kBlockMax) return BAD_FRAME;
            const uint32_t body = type == 1 ? 1u : bsize;
            if (n - pos - 3 < body) return BAD_FRAME;
            pos += 3 + body;
            if (bh & 1u) break;
        }
        if (h.has_checksum) {
            if (n - pos < 4) return BAD_FRAME;
            pos += 4;
        }
    }
    return OK;
}

}  // namespace pbsz
