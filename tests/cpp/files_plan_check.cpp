// CPU check of the many-files planning (br-archive_amd/csrc/files_plan.h): for seeded random file
// lists the plan must cover every byte of every file by exactly one chunk, and its two tail
// distances per chunk must turn per-chunk CRC32C values into the per-file CRCs -- the chunk-stream
// CRC hdr0 || chunk0 || hdr1 || ... with random headers (orc_chunks_crc32c) and the plain CRC
// (orc_crc32c) -- when combined through orc_crc32c_combine, the way the segmented CRC kernel moves a
// piece's raw value to the end of the two streams.  Also: the long chunks' piece list, the output
// bound against the worst-case record sizes, and the rejected lists.  Test infrastructure only
// (tests/test_files_plan.py builds it with the address and undefined-behaviour sanitizers).
//
//   files_plan_check [lists] [seed]   -> "ok <lists> <files> <chunks>" or a first mismatch, exit 1
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../br-archive_amd/csrc/files_plan.h"
extern "C" {
#include "../../oracle/bra_oracle.h"
}

using namespace bra;

static uint64_t rng_state = 1;
static uint32_t rnd()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (uint32_t) (rng_state >> 16);
}

#define FAIL(...)                     \
    do                                \
    {                                 \
        fprintf(stderr, __VA_ARGS__); \
        fprintf(stderr, "\n");        \
        return false;                 \
    } while (0)

// a CRC value moved over `n` following bytes (crc(A || B) = move(crc(A), |B|) ^ crc(B))
static uint32_t move_crc(uint32_t crc, uint64_t n) { return orc_crc32c_combine(crc, 0, (uint32_t) n); }

static bool check_list(uint32_t block_size, uint32_t nfiles, uint64_t& files, uint64_t& chunks)
{
    std::vector<uint64_t> off(nfiles), len(nfiles);
    const bool            gaps = rnd() & 1;
    uint64_t              pos  = rnd() % 64;
    for (uint32_t f = 0; f < nfiles; ++f)
    {
        const uint32_t k = rnd() % 8;
        uint64_t       n = rnd() % (3ull * block_size + 8);  // 0 .. 3 * block_size + 7
        if (k == 0)
            n = 0;
        else if (k == 1)
            n = (uint64_t) block_size * (1 + rnd() % 3) + (rnd() % 3) - 1;  // around a multiple of the chunk size
        if (gaps)
            pos = (pos + 15) / 16 * 16 + 16 * (rnd() % 3);
        off[f] = pos;
        len[f] = n;
        pos += n;
    }
    FilesPlan p;
    if (!files_plan_build(off.data(), len.data(), nfiles, block_size, p))
        FAIL("plan rejected a valid list (block_size %u, %u files)", block_size, nfiles);
    if (p.first.size() != (size_t) nfiles + 1 || p.first[nfiles] != p.chunks.size())
        FAIL("first[] does not frame the chunks");
    // coverage: every byte of every file in exactly one chunk of that file, gaps in none
    std::vector<uint8_t> data(p.extent + 1), cover(p.extent + 1, 0);
    for (auto& b : data)
        b = (uint8_t) rnd();
    for (uint32_t f = 0; f < nfiles; ++f)
    {
        if (p.first[f + 1] - p.first[f] != files_num_chunks(len[f], block_size))
            FAIL("file %u has %u chunks", f, p.first[f + 1] - p.first[f]);
        uint64_t at = len[f] ? off[f] - p.base : 0;
        for (uint32_t b = p.first[f]; b < p.first[f + 1]; ++b)
        {
            const FileChunk& c = p.chunks[b];
            if (c.file != f || c.off != at || c.len == 0 || c.len > block_size || c.off + c.len > p.extent)
                FAIL("chunk %u of file %u misplaced", b, f);
            if (b + 1 < p.first[f + 1] && c.len != block_size)
                FAIL("chunk %u of file %u is short but not the last", b, f);
            for (uint64_t i = 0; i < c.len; ++i)
                ++cover[c.off + i];
            at += c.len;
        }
        if (len[f] && at != off[f] - p.base + len[f])
            FAIL("file %u not covered to its end", f);
    }
    {
        std::vector<uint8_t> want(p.extent + 1, 0);
        for (uint32_t f = 0; f < nfiles; ++f)
            for (uint64_t i = 0; i < len[f]; ++i)
                want[off[f] - p.base + i] = 1;
        if (cover != want)
            FAIL("coverage differs from the file list");
    }
    // the two CRCs of every file from per-chunk values and the tail distances
    for (uint32_t f = 0; f < nfiles; ++f)
    {
        const uint32_t       n = p.first[f + 1] - p.first[f];
        std::vector<uint8_t> hdr((size_t) n * FILES_HDR_MEM + 1);
        for (auto& b : hdr)
            b = (uint8_t) rnd();
        const uint8_t* src = data.data() + (len[f] ? off[f] - p.base : 0);
        // crc(P1 || ... || Pk) is the XOR of every crc(Pi) moved over the bytes that follow Pi
        uint32_t stream = 0, raw = 0;
        for (uint32_t b = p.first[f]; b < p.first[f + 1]; ++b)
        {
            const FileChunk& c  = p.chunks[b];
            const uint32_t   ch = orc_crc32c(hdr.data() + (size_t) (b - p.first[f]) * FILES_HDR_MEM, FILES_HDR_MEM, 0);
            const uint32_t   cd = orc_crc32c(data.data() + c.off, c.len, 0);
            stream ^= move_crc(ch, c.len + c.tail_stream) ^ move_crc(cd, c.tail_stream);
            raw ^= move_crc(cd, c.tail_raw);
        }
        const uint32_t want_stream = n ? orc_chunks_crc32c(hdr.data(), src, len[f], block_size, 0) : 0;
        const uint32_t want_raw    = orc_crc32c(src, len[f], 0);
        if (stream != want_stream)
            FAIL("chunk-stream CRC of file %u (%llu bytes, block_size %u): %08x, oracle %08x", f, (unsigned long long) len[f], block_size, stream,
                 want_stream);
        if (raw != want_raw)
            FAIL("plain CRC of file %u (%llu bytes, block_size %u): %08x, oracle %08x", f, (unsigned long long) len[f], block_size, raw, want_raw);
    }
    // pieces: every long chunk cut at multiples of 64 KiB from its end, short chunks in none
    std::vector<FilePiece> pieces;
    files_plan_pieces(p.chunks, pieces);
    std::vector<uint64_t> got(p.chunks.size(), 0);
    for (const FilePiece& pc : pieces)
    {
        if (pc.chunk >= p.chunks.size())
            FAIL("piece of chunk %u", pc.chunk);
        const int64_t end = (int64_t) p.chunks[pc.chunk].len - (int64_t) pc.after * FILES_PIECE;
        if (end <= 0)
            FAIL("empty piece of chunk %u", pc.chunk);
        got[pc.chunk] += (uint64_t) (end < (int64_t) FILES_PIECE ? end : FILES_PIECE);
    }
    for (size_t b = 0; b < p.chunks.size(); ++b)
        if (got[b] != (p.chunks[b].len > FILES_WAVE_CHUNK ? p.chunks[b].len : 0))
            FAIL("pieces of chunk %zu cover %llu of %u bytes", b, (unsigned long long) got[b], p.chunks[b].len);
    // the bound holds every chunk's record at its worst-case payload (RLE capacity, codes of <= 32 bits)
    uint64_t need = 0;
    for (const FileChunk& c : p.chunks)
        need += 4 * files_rle_capacity(c.len) + FILES_HDR_DISK;
    const uint64_t bound = files_bound(len.data(), nfiles, block_size);
    if (bound < need || bound > need + 4096)
        FAIL("bound %llu for a worst case of %llu", (unsigned long long) bound, (unsigned long long) need);
    files += nfiles;
    chunks += p.chunks.size();
    return true;
}

static bool check_rejections()
{
    FilesPlan      p;
    const uint64_t off[3] = {0, 100, 300}, len[3] = {100, 200, 50};
    if (!files_plan_build(off, len, 3, 4096, p))
        FAIL("valid list rejected");
    if (files_plan_build(off, len, 0, 4096, p) || files_plan_build(off, len, 3, 0, p) || files_plan_build(off, len, 3, 1u << 24, p) ||
        files_plan_build(nullptr, len, 3, 4096, p) || files_plan_build(off, nullptr, 3, 4096, p))
        FAIL("bad arguments accepted");
    const uint64_t desc[3] = {0, 300, 100};
    if (files_plan_build(desc, len, 3, 4096, p))
        FAIL("descending offsets accepted");
    const uint64_t over[3] = {0, 99, 300};
    if (files_plan_build(over, len, 3, 4096, p))
        FAIL("overlapping files accepted");
    const uint64_t big_off[2] = {4096, 4096 + (1ull << 30)}, big_len[2] = {1ull << 30, 1ull << 30};
    if (files_plan_build(big_off, big_len, 2, 262144, p))
        FAIL("an extent of 2^31 bytes accepted");
    const uint64_t ok_len[2] = {1ull << 30, (1ull << 30) - 1};
    if (!files_plan_build(big_off, ok_len, 2, 262144, p) || p.base != 4096 || p.extent != (1ull << 31) - 1)
        FAIL("an extent of 2^31 - 1 bytes rejected");
    const uint64_t empty_off[2] = {5, 5}, empty_len[2] = {0, 0};
    if (!files_plan_build(empty_off, empty_len, 2, 7, p) || !p.chunks.empty() || p.extent != 0)
        FAIL("empty files not planned as no chunks");
    return true;
}

int main(int argc, char** argv)
{
    const int lists = argc > 1 ? atoi(argv[1]) : 300;
    rng_state       = argc > 2 ? strtoull(argv[2], nullptr, 0) : 0x9E3779B97F4A7C15ull;
    if (rng_state == 0)
        rng_state = 1;
    if (!check_rejections())
        return 1;
    static const uint32_t sizes[4] = {1, 7, 4096, 262144};
    uint64_t              files = 0, chunks = 0;
    for (int i = 0; i < lists; ++i)
    {
        const uint32_t bs = sizes[i % 4];
        const uint32_t nf = bs == 262144 ? 1 + rnd() % 2 : bs == 4096 ? 1 + rnd() % 12 : 1 + rnd() % 40;
        if (!check_list(bs, nf, files, chunks))
        {
            fprintf(stderr, "list %d (block_size %u, %u files) failed\n", i, bs, nf);
            return 1;
        }
    }
    printf("ok %d %llu %llu\n", lists, (unsigned long long) files, (unsigned long long) chunks);
    return 0;
}
