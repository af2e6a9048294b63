// files_plan.h -- host planning of the many-files calls (bra_gpu_compress_files /
// bra_gpu_decompress_files, include/bra_hip_files.h).  No HIP dependency: the same header is
// compiled for the host alone by tests/cpp/files_plan_check.cpp.
//
// Every file is cut into chunks of its own (block_size bytes, its last one ragged); the chunks of
// all files form one batch.  Per chunk the plan keeps one 32-byte row, which is also the table the
// segmented CRC kernel (crc.hip, k_crc_files) walks: where the chunk's plain bytes are, which file it
// belongs to, and how far its end is from the end of that file's two CRC streams,
//   the chunk stream  hdr0 || chunk0 || hdr1 || chunk1 || ...   (268-byte in-memory headers), and
//   the plain stream  chunk0 || chunk1 || ...
// With L(X) the raw CRC of X, a chunk (or any piece of it) contributes L(piece) * x^(8 * tail) to a
// stream's CRC, `tail` being the stream bytes after the piece: the raw value is the same for both
// streams, only the power differs.
#pragma once

#include <cstdint>
#include <vector>

namespace bra {

constexpr uint32_t FILES_HDR_MEM    = 268;        // in-memory chunk header (folded into the chunk-stream CRC)
constexpr uint32_t FILES_HDR_DISK   = 267;        // on-disk chunk header
constexpr uint32_t FILES_PIECE      = 64 * 1024;  // CRC piece of a long chunk: one workgroup
constexpr uint32_t FILES_WAVE_CHUNK = 4096;       // chunks up to this size: one wave, with the chunk's header

struct FileChunk
{
    uint64_t off;          // the chunk's plain bytes, relative to the plan's base
    uint32_t len;
    uint32_t file;
    uint64_t tail_stream;  // bytes of the file's chunk stream after this chunk's end
    uint64_t tail_raw;     // bytes of the file's plain data after this chunk's end
};
static_assert(sizeof(FileChunk) == 32, "row of the segmented CRC table");

// Same layout as bra_gpu_file_result_t.
struct FileResult
{
    uint64_t off, size;
    uint32_t chunks_crc, raw_crc, num_chunks, compressed;
};
static_assert(sizeof(FileResult) == 32, "bra_gpu_file_result_t layout");

// A 64 KiB piece of a chunk longer than FILES_WAVE_CHUNK: `after` whole pieces of the chunk follow
// it (pieces are aligned to the chunk end, the first one ragged).
struct FilePiece
{
    uint32_t chunk, after;
};

struct FilesPlan
{
    uint64_t               base = 0;  // offset of the first byte of the first non-empty file
    uint64_t               extent = 0;  // end of the last file, relative to base
    std::vector<FileChunk> chunks;
    std::vector<uint32_t>  first;  // nfiles + 1: first chunk of every file
};

// Worst-case RLE output of an n-byte chunk (rle.h rle_capacity).
inline uint64_t files_rle_capacity(uint32_t n) { return (uint64_t) n + (n + 127) / 128 + 16; }

inline uint64_t files_num_chunks(uint64_t len, uint32_t block_size) { return (len + block_size - 1) / block_size; }

// The tail distances of every chunk from the chunk lengths and the file of each chunk.
inline void files_plan_tails(FilesPlan& p)
{
    for (size_t f = 0; f + 1 < p.first.size(); ++f)
    {
        uint64_t raw = 0, hdrs = 0;
        for (uint32_t b = p.first[f + 1]; b-- > p.first[f];)
        {
            p.chunks[b].tail_raw    = raw;
            p.chunks[b].tail_stream = raw + hdrs;
            raw += p.chunks[b].len;
            hdrs += FILES_HDR_MEM;
        }
    }
}

// Chunks of the files [off[f], off[f] + len[f]).  False when the list is not acceptable: no file,
// block_size outside [1, 2^24), offsets that descend or files that overlap, an extent (first byte
// of the first non-empty file to the end of the last) of 2^31 bytes or more.
inline bool files_plan_build(const uint64_t* off, const uint64_t* len, uint32_t nfiles, uint32_t block_size, FilesPlan& p)
{
    p = FilesPlan{};
    if (!off || !len || nfiles == 0 || block_size == 0 || block_size >= (1u << 24))
        return false;
    bool     any = false;
    uint64_t end = 0;  // absolute end of the files so far
    for (uint32_t f = 0; f < nfiles; ++f)
    {
        if (off[f] + len[f] < off[f] || (f && off[f] < off[f - 1]) || off[f] < end)
            return false;
        end = off[f] + len[f];
        if (len[f] && !any)
        {
            any    = true;
            p.base = off[f];
        }
        if (any && end - p.base >= (1ull << 31))
            return false;
    }
    p.extent = any ? end - p.base : 0;
    p.first.resize((size_t) nfiles + 1);
    for (uint32_t f = 0; f < nfiles; ++f)
    {
        p.first[f] = (uint32_t) p.chunks.size();
        for (uint64_t o = 0; o < len[f]; o += block_size)
        {
            const uint64_t n = len[f] - o < block_size ? len[f] - o : block_size;
            p.chunks.push_back(FileChunk{off[f] - p.base + o, (uint32_t) n, f, 0, 0});
        }
    }
    p.first[nfiles] = (uint32_t) p.chunks.size();
    files_plan_tails(p);
    return true;
}

// The work list of the segmented CRC's workgroup path: every 64 KiB piece of every long chunk.
inline void files_plan_pieces(const std::vector<FileChunk>& chunks, std::vector<FilePiece>& out)
{
    out.clear();
    for (uint32_t b = 0; b < (uint32_t) chunks.size(); ++b)
        if (chunks[b].len > FILES_WAVE_CHUNK)
            for (uint32_t k = (chunks[b].len + FILES_PIECE - 1) / FILES_PIECE; k-- > 0;)
                out.push_back(FilePiece{b, k});
}

// Payload capacity that one encode of all chunks never exceeds (no code is longer than 32 bits
// below ~3.5 M symbols per block), and the output capacity with the on-disk headers.
inline uint64_t files_payload_bound(const uint64_t* len, uint32_t nfiles, uint32_t block_size)
{
    uint64_t r = 64;
    for (uint32_t f = 0; f < nfiles; ++f)
    {
        const uint64_t full = len[f] / block_size, rest = len[f] % block_size;
        r += full * 4 * files_rle_capacity(block_size) + (rest ? 4 * files_rle_capacity((uint32_t) rest) : 0);
    }
    return r;
}

inline uint64_t files_bound(const uint64_t* len, uint32_t nfiles, uint32_t block_size)
{
    if (!len || block_size == 0)
        return 0;
    uint64_t r = files_payload_bound(len, nfiles, block_size);
    for (uint32_t f = 0; f < nfiles; ++f)
        r += FILES_HDR_DISK * files_num_chunks(len[f], block_size);
    return r;
}

}  // namespace bra
