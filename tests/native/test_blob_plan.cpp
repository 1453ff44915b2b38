// The host plans of the aux calls (pbs_plus_amd/csrc/blob_plan.h) on their own, under ASan + UBSan: the piece table, the
// restore plan and the packed blocks. Every case checks itself; "blob-plan-ok" at the end.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../pbs_plus_amd/csrc/blob_plan.h"

#define REQUIRE(c)                                                        \
    do {                                                                  \
        if (!(c)) {                                                       \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #c);          \
            std::exit(1);                                                 \
        }                                                                 \
    } while (0)

using namespace pbsp;

// ---- the piece table --------------------------------------------------------------------------------------------------

static void piece_cases() {
    const std::vector<uint64_t> lens = {0, 1, kPiece - 1, kPiece, kPiece + 1};
    const std::vector<uint64_t> want = {0, 1, 1, 1, 2};
    PieceTable t;
    REQUIRE(piece_table(lens.size(), [&](uint64_t i) { return lens[i]; }, t));
    REQUIRE(t.np == 5 && t.pbase.size() == 6 && t.owner.size() == 5);
    uint64_t at = 0;
    for (size_t i = 0; i < lens.size(); ++i) {
        REQUIRE(pieces_of(lens[i]) == want[i] && t.pbase[i] == at);
        for (uint64_t p = at; p < at + want[i]; ++p) REQUIRE(t.owner[p] == i);
        at += want[i];
    }
    REQUIRE(t.pbase[5] == 5);
    for (size_t i = 0; i < lens.size(); ++i) {  // each length alone
        PieceTable one;
        REQUIRE(piece_table(1, [&](uint64_t) { return lens[i]; }, one));
        REQUIRE(one.np == want[i] && one.pbase[0] == 0 && one.pbase[1] == want[i]);
    }
    PieceTable none;
    REQUIRE(piece_table(0, [](uint64_t) { return 0ull; }, none));
    REQUIRE(none.np == 0 && none.pbase.size() == 1 && none.pbase[0] == 0 && none.owner.empty());
    // 2^32 - 1 pieces pass, 2^32 do not: the counts only
    std::vector<uint64_t> pbase;
    const uint64_t most = ((1ull << 32) - 1) * kPiece;
    REQUIRE(piece_bases(1, [&](uint64_t) { return most; }, pbase) && pbase[1] == (1ull << 32) - 1);
    REQUIRE(piece_bases(2, [&](uint64_t i) { return i ? 1 : most - kPiece; }, pbase) && pbase[2] == (1ull << 32) - 1);
    REQUIRE(!piece_bases(1, [&](uint64_t) { return most + 1; }, pbase));
    REQUIRE(!piece_bases(2, [&](uint64_t i) { return i ? 1 : most; }, pbase) && pbase[2] == 1ull << 32);
}

// ---- the restore plan -------------------------------------------------------------------------------------------------

struct Index {
    std::vector<pbsgpu_record> idx;
    std::vector<uint32_t> blob_of;
    void add(uint32_t size, uint32_t blob) {
        pbsgpu_record r{};
        r.end = (idx.empty() ? 100 : idx.back().end) + size;  // the stream starts at 100
        r.size = size;
        idx.push_back(r);
        blob_of.push_back(blob);
    }
};

static pbsgpu_segment blob_at(uint64_t off, uint64_t data) { return pbsgpu_segment{off, data + PBSGPU_BLOB_HEADER_SIZE}; }

// what every plan must satisfy, whatever the case
static void check_plan(const Restore &r, const Index &ix, const std::vector<pbsgpu_segment> &blobs, bool by_position,
                       uint64_t rs, uint64_t re, bool zstd) {
    const size_t nidx = ix.idx.size();
    REQUIRE(r.ents.size() == nidx && r.clip.size() == nidx && r.prim.size() == r.nu());
    uint64_t clipped = 0, stores = 0;
    std::vector<int> seen(r.nu(), 0);
    for (size_t i = 0; i < nidx; ++i) {
        const uint32_t b = by_position ? (uint32_t)i : ix.blob_of[i];
        const uint32_t u = r.ents[i].u;
        REQUIRE(u < r.nu() && r.ub[u].offset == blobs[b].offset && r.ub[u].length == blobs[b].length);
        REQUIRE(r.ents[i].size == ix.idx[i].size);
        const uint64_t start = ix.idx[i].end - ix.idx[i].size, end = ix.idx[i].end;
        const uint64_t lo = start > rs ? start : rs, hi = end < re ? end : re;
        REQUIRE(r.clip[i] == (hi > lo ? hi - lo : 0));
        clipped += r.clip[i];
        if (r.clip[i] && !seen[u]) {  // the first entry with bytes in the range is the primary
            seen[u] = 1;
            const DecStore &p = r.prim[u];
            REQUIRE(p.u == u && p.size == ix.idx[i].size && p.dofs == (int64_t)(start - rs));
            REQUIRE(p.xlo == lo - start && p.xhi == hi - start);
        }
    }
    for (uint32_t u = 0; u < r.nu(); ++u) {
        if (!seen[u]) REQUIRE(r.prim[u].xlo == r.prim[u].xhi && r.prim[u].u == u);
        stores += r.prim[u].xhi - r.prim[u].xlo;
    }
    uint64_t longest = 0;
    for (const DecStore &c : r.copies) {
        REQUIRE(c.xlo < c.xhi && c.xhi <= c.size && seen[c.u]);
        REQUIRE((uint64_t)(c.dofs + (int64_t)c.xhi) <= re - rs && c.dofs + (int64_t)c.xlo >= 0);
        stores += c.xhi - c.xlo;
        longest = std::max(longest, c.xhi - c.xlo);
    }
    REQUIRE(stores == clipped && clipped == re - rs && longest == r.longest_copy);
    // the pieces and the SHA sums are over the data lengths for the short header
    ShaWork sha;
    uint64_t np = 0;
    for (uint32_t u = 0; u < r.nu(); ++u) {
        const uint64_t dl = r.ub[u].length > PBSGPU_BLOB_HEADER_SIZE ? r.ub[u].length - PBSGPU_BLOB_HEADER_SIZE : 0;
        REQUIRE(r.pieces.pbase[u] == np);
        np += (dl + 65535) / 65536;
        sha.add(dl);
    }
    REQUIRE(r.pieces.np == np && r.pieces.pbase[r.nu()] == np && r.pieces.owner.size() == np);
    REQUIRE(sha.total_blocks == r.sha.total_blocks && sha.longest == r.sha.longest);
    if (!zstd) {
        REQUIRE(r.jobs.empty() && r.zcopies.empty() && r.scratch_bytes == 0);
        return;
    }
    // zstd: a room per blob, straight in dst exactly when the primary is whole and no entry of the blob is larger
    REQUIRE(r.jobs.size() == r.nu() && r.zmax.size() == r.nu() && r.in_scratch.size() == r.nu());
    uint64_t sc = (uint64_t)r.lit_groups * pbsk::zstd::kLitBytes, zstores = 0;
    for (uint32_t u = 0; u < r.nu(); ++u) {
        uint32_t zmax = 0;
        for (size_t i = 0; i < nidx; ++i)
            if (r.ents[i].u == u) zmax = std::max(zmax, r.ents[i].size);
        const DecStore &p = r.prim[u];
        const bool direct = p.xlo < p.xhi && p.xlo == 0 && p.xhi == p.size && p.size == zmax;
        REQUIRE(r.zmax[u] == zmax && r.jobs[u].room == zmax && (r.in_scratch[u] != 0) == !direct);
        if (direct) {
            REQUIRE(r.jobs[u].place == (uint64_t)p.dofs);
            zstores += p.size;
        } else {
            REQUIRE(r.jobs[u].place == sc);
            sc += ((uint64_t)zmax + 15) & ~15ull;
        }
    }
    REQUIRE(sc == r.scratch_bytes);
    uint32_t zlongest = 0;
    for (const RestoreCopy &c : r.zcopies) {
        REQUIRE(c.len && c.to + c.len <= re - rs);
        zstores += c.len;
        zlongest = std::max(zlongest, c.len);
    }
    REQUIRE(zstores == clipped && zlongest == r.longest_zcopy);
    // the scratch base moves the scratch places and the copies out of them, and nothing else
    Restore moved = r;
    moved.place_scratch(1ull << 40);
    for (uint32_t u = 0; u < r.nu(); ++u) REQUIRE(moved.jobs[u].place == r.jobs[u].place + (r.in_scratch[u] ? 1ull << 40 : 0));
    for (size_t k = 0; k < r.zcopies.size(); ++k)
        REQUIRE(moved.zcopies[k].from == r.zcopies[k].from + (r.in_scratch[r.zcopies[k].u] ? 1ull << 40 : 0));
}

static Restore plan(const Index &ix, const std::vector<pbsgpu_segment> &blobs, bool by_position, uint64_t rs, uint64_t re,
                    bool zstd) {
    Restore r;
    REQUIRE(plan_restore(blobs.data(), (uint32_t)blobs.size(), ix.idx.data(), ix.idx.size(),
                         by_position ? nullptr : ix.blob_of.data(), rs, re, zstd, 3, r));
    check_plan(r, ix, blobs, by_position, rs, re, zstd);
    return r;
}

static void restore_cases() {
    for (int z = 0; z < 2; ++z) {
        const bool zstd = z != 0;
        {  // one blob behind many entries: the first in range is the primary, the rest are copies
            Index ix;
            for (int i = 0; i < 5; ++i) ix.add(1000, 0);
            const std::vector<pbsgpu_segment> blobs = {blob_at(0, 1000)};
            const Restore all = plan(ix, blobs, false, 100, 5100, zstd);
            REQUIRE(all.nu() == 1 && all.copies.size() == 4 && all.prim[0].dofs == 0);
            if (zstd) REQUIRE(!all.in_scratch[0] && all.zcopies.size() == 4);
            // the range begins and ends inside entries: entry 0 is out, entry 1 is cut in front, entry 4 behind
            const Restore cut = plan(ix, blobs, false, 1600, 4700, zstd);
            REQUIRE(cut.clip[0] == 0 && cut.clip[1] == 500 && cut.clip[4] == 600);
            REQUIRE(cut.prim[0].xlo == 500 && cut.prim[0].xhi == 1000 && cut.prim[0].dofs == -500 && cut.copies.size() == 3);
            if (zstd) REQUIRE(cut.in_scratch[0] && cut.zcopies.size() == 4);  // a clipped primary: through scratch
        }
        {  // a range with no byte of some blob, an empty range, and blobs by position
            Index ix;
            ix.add(3000, 0);
            ix.add(70000, 1);
            ix.add(0, 2);
            ix.add(5, 3);
            const std::vector<pbsgpu_segment> blobs = {blob_at(0, 3000), blob_at(4000, 70000), blob_at(80000, 0), blob_at(80100, 5)};
            const Restore part = plan(ix, blobs, true, 100, 3100, zstd);
            REQUIRE(part.nu() == 4 && part.prim[0].xhi == 3000 && part.copies.empty());
            for (uint32_t u = 1; u < 4; ++u) REQUIRE(part.prim[u].xlo == part.prim[u].xhi);
            if (zstd) REQUIRE(!part.in_scratch[0] && part.in_scratch[1] && part.in_scratch[2] && part.in_scratch[3]);
            const Restore empty = plan(ix, blobs, true, 3100, 3100, zstd);
            for (uint32_t u = 0; u < 4; ++u) REQUIRE(empty.prim[u].xlo == empty.prim[u].xhi);
            const Restore whole = plan(ix, blobs, true, 100, 73105, zstd);
            REQUIRE(whole.pieces.np == 1 + 2 + 0 + 1 && whole.copies.empty());
            if (zstd) REQUIRE(whole.zcopies.empty() && whole.in_scratch[2] && !whole.in_scratch[3]);
        }
        {  // encrypted-header lengths: blobs of 12 bytes and fewer have no data, pieces or hash blocks beyond the padding
            Index ix;
            std::vector<pbsgpu_segment> blobs;
            for (uint32_t len : {0u, 1u, 11u, 12u, 13u, 44u}) {
                ix.add(len > 12 ? len - 12 : 0, (uint32_t)blobs.size());
                blobs.push_back(pbsgpu_segment{blobs.size() * 64, len});
            }
            const Restore r = plan(ix, blobs, false, 100, ix.idx.back().end, zstd);
            REQUIRE(r.pieces.np == 2 && r.pieces.pbase[4] == 0 && r.pieces.pbase[5] == 1 && r.sha.total_blocks == 6);
        }
        if (!zstd) continue;
        {  // direct placement needs the first in-range entry whole AND the largest: a later entry larger by one spoils it
            Index same, larger;
            for (int i = 0; i < 3; ++i) same.add(500, 0);
            larger.add(500, 0);
            larger.add(500, 0);
            larger.add(501, 0);
            const std::vector<pbsgpu_segment> blobs = {blob_at(0, 500)};
            REQUIRE(!plan(same, blobs, false, 100, 1600, true).in_scratch[0]);
            const Restore l = plan(larger, blobs, false, 100, 1601, true);
            REQUIRE(l.in_scratch[0] && l.jobs[0].room == 501 && l.zcopies.size() == 3);
            REQUIRE(l.scratch_bytes == 1 * pbsk::zstd::kLitBytes + 512);
            // first entry outside the range: the primary is the second, which is whole: still direct
            const Restore second = plan(same, blobs, false, 600, 1600, true);
            REQUIRE(!second.in_scratch[0] && second.jobs[0].place == 0 && second.zcopies.size() == 1);
            // more blobs than literal workgroups: the literal buffers stop at lit_groups_max
            Index many;
            std::vector<pbsgpu_segment> mb;
            for (uint32_t i = 0; i < 5; ++i) {
                many.add(16, i);
                mb.push_back(blob_at(i * 100, 16));
            }
            const Restore m = plan(many, mb, false, 101, 180, true);
            REQUIRE(m.lit_groups == 3 && m.in_scratch[0] && !m.in_scratch[1] && m.scratch_bytes == 3 * pbsk::zstd::kLitBytes + 16);
        }
    }
}

// ---- the packed blocks: the offsets are the expressions they replaced ----------------------------------------------------

static void block_cases() {
    for (size_t n : {0, 1, 3, 4, 5}) {
        const UpBlock up(n, false), upz(n, true);
        const size_t lens_at = (64 + n * 13 + 3) & ~(size_t)3;
        REQUIRE(up.head == 0 && up.boff == 64 && up.crcs == 64 + n * 8 && up.known == 64 + n * 12 && up.total == 64 + n * 13);
        REQUIRE(upz.head == 0 && upz.boff == 64 && upz.crcs == 64 + n * 8 && upz.known == 64 + n * 12);
        REQUIRE(upz.lens == lens_at && upz.kinds == lens_at + n * 4 && upz.total == lens_at + n * 5);
        const Enc2Block e2(n);
        REQUIRE(e2.crcs == 0 && e2.lens == n * 4 && e2.kinds == n * 8 && e2.total == n * 9);
        for (size_t nidx : {1, 2, 7, 8, 9}) {
            const DecBlock d(n, nidx, false), dz(n, nidx, true);
            const size_t o_zres = (n * 8 + nidx + 7) & ~(size_t)7;
            REQUIRE(d.info == 0 && d.status == n * 8 && d.total == n * 8 + nidx);
            REQUIRE(dz.info == 0 && dz.status == n * 8 && dz.zres == o_zres && dz.total == o_zres + n * 8);
            for (size_t ncopy : {0, 2})
                for (size_t np : {0, 5}) {
                    const DecTables t(n, ncopy, nidx, np);
                    const size_t o_prim = (n + 1) * 8, o_cop = o_prim + n * 32, o_ent = o_cop + ncopy * 32, o_pseg = o_ent + nidx * 8;
                    REQUIRE(t.pbase == 0 && t.prim == o_prim && t.copies == o_cop && t.ents == o_ent && t.pseg == o_pseg);
                    REQUIRE(t.total == o_pseg + np * 4);
                    const ZTables zt(n, ncopy);
                    REQUIRE(zt.jobs == 0 && zt.copies == n * 16 && zt.total == n * 16 + ncopy * 32);
                }
        }
        const ZWork w(n);
        REQUIRE(w.sha == 0 && w.digs == n * 16 && w.queue == n * 16 + n * 32 && w.desc == n * 48 + 64 && w.total == n * 48 + 64 + n * 32);
    }
}

// ---- the small shared pieces ------------------------------------------------------------------------------------------

static void small_cases() {
    const pbsgpu_segment segs[3] = {{0, 0}, {10, 0}, {4, 6}};
    REQUIRE(ranges_ok(segs, 3, 10) && !ranges_ok(segs, 3, 9) && ranges_ok(nullptr, 0, 0));
    const pbsgpu_segment wrap[1] = {{~0ull, 2}};
    REQUIRE(!ranges_ok(wrap, 1, 100));
    const uint8_t *base = reinterpret_cast<const uint8_t *>(uintptr_t(1) << 20);
    REQUIRE(overlaps(base, 10, base + 9, 5) && !overlaps(base, 10, base + 10, 5) && overlaps(base + 4, 1, base, 10));
    REQUIRE(!overlaps(base, 0, base, 10) && !overlaps(base, 10, base + 3, 0));
    ShaWork w;
    for (uint64_t len : {0, 55, 56, 119, 120}) w.add(len);
    REQUIRE(w.total_blocks == 1 + 1 + 2 + 2 + 3 && w.longest == 3);
    pbsgpu_encode_stats st{};
    count_blob(st, PBSGPU_BLOB_UNCOMPRESSED, 112, 100);
    count_blob(st, PBSGPU_BLOB_COMPRESSED, 52, 100);
    REQUIRE(st.blobs[0] == 1 && st.blobs[1] == 1 && st.blob_bytes[0] == 112 && st.blob_bytes[1] == 52);
    REQUIRE(st.chunk_bytes[0] == 100 && st.chunk_bytes[1] == 100 && st.frame_bytes == 40 && st.crc_bytes == 140);
}

int main() {
    piece_cases();
    restore_cases();
    block_cases();
    small_cases();
    std::printf("blob-plan-ok\n");
    return 0;
}
