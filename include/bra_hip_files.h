/*
 * bra_hip_files.h -- Part 5 of the C-ABI of libbra_hip.so: many files in one call.
 *
 * (A header of its own, included at the end of bra_hip.h: tests/test_abi.py pins the function list
 * of bra_hip.h itself to the drop-in ABI and the single-buffer batch calls.)
 *
 * bra_gpu_compress_chunks / bra_gpu_decompress_chunks take one file per call, and a call pays a
 * handful of host round trips whatever the file's size.  The two calls here take a list of files of
 * any sizes: every file is cut into block_size chunks of its own, the chunks of all files go
 * through one encode (or decode) of the batch, and one table in device memory tells the caller
 * where each file's result is.  file_off / file_len / stream_off / stream_size are host arrays;
 * everything prefixed d_ is device memory.  Streams as in Part 3: a NULL stream means the
 * context's stream and the call has completed when it returns.
 */
#pragma once

#include "bra_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One per file, in device memory. */
typedef struct bra_gpu_file_result_t
{
    uint64_t off;        /* compress: start of the file's chunk stream in d_out; decompress: start of its decoded bytes */
    uint64_t size;       /* bytes there */
    uint32_t chunks_crc; /* CRC32C of hdr0||chunk0||hdr1||chunk1... of this file (268-byte in-memory headers), chained
                            from 0: the `crc32` of the compress loop (lib_bra_io_file_chunks.c:214,248-249) and what the
                            decode loop folds in (:396-397) */
    uint32_t raw_crc;    /* CRC32C of the file's plain bytes chained from 0 (what a STORED entry folds in) */
    uint32_t num_chunks;
    uint32_t compressed; /* compress: 1 when size < file_len, else the reference stores the file (:274-278); decompress: 1 */
} bra_gpu_file_result_t;

#if defined(__cplusplus)
static_assert(sizeof(bra_gpu_file_result_t) == 32, "bra_gpu_file_result_t is 32 bytes");
#else
_Static_assert(sizeof(bra_gpu_file_result_t) == 32, "bra_gpu_file_result_t is 32 bytes");
#endif

/* Host only: a d_out capacity that bra_gpu_compress_files of these files never exceeds (0 when
 * block_size is 0 or file_len NULL). */
uint64_t bra_gpu_files_bound(const uint64_t* file_len, uint32_t nfiles, uint32_t block_size);

/*
 * The compress chunk loop over nfiles files in one call.  File f is d_in[file_off[f], file_off[f] +
 * file_len[f]); offsets ascend and files do not overlap, gaps and any alignment are allowed.  The
 * files' chunk streams land in d_out back to back in file order (*out_size = their total), and
 * d_results[f] is what bra_gpu_compress_chunks(d_in + file_off[f], file_len[f], block_size, ...)
 * gives for the file alone: the same stream bytes at [off, off + size), the same chunks_crc, and
 * compressed = its 1 / 0 return value.  A file of length 0 has num_chunks 0, size 0, compressed 0
 * and both CRCs 0.  me->crc32 of a compressed entry follows from chunks_crc with
 * bra_gpu_entry_crc32c, that of a stored one from raw_crc with bra_gpu_crc32c_combine(prev,
 * raw_crc, file_len).
 * Returns 0 on success, -2 when out_cap is too small (*out_size = the bytes needed; d_out is not
 * written), -1 otherwise.  Rejected with -1 before any device work: nfiles == 0, block_size outside
 * [1, 2^24), descending or overlapping files, and an input extent (first byte of the first
 * non-empty file to the end of the last file) of 2^31 bytes or more, the limit of one encode batch.
 */
int bra_gpu_compress_files(bra_gpu_ctx_t* ctx, const uint8_t* d_in, const uint64_t* file_off, const uint64_t* file_len, uint32_t nfiles,
                           uint32_t block_size, uint8_t* d_out, uint64_t out_cap, uint64_t* out_size, bra_gpu_file_result_t* d_results,
                           void* stream);

/*
 * The decode loop over nfiles chunk streams in one call.  File f's stream is d_streams[stream_off[f],
 * stream_off[f] + stream_size[f]); the decoded files land in d_out back to back in file order
 * (*out_size = their total, below 2^31) and d_results[f] holds the file's offset and decoded size,
 * the chunk-stream CRC over the decoded chunks and the plain CRC of the decoded bytes, both chained
 * from 0, and the chunk count.  The decode loop's me->crc32 update (:396-397) is
 *     bra_gpu_crc32c_combine(prev, chunks_crc, size + 268 * num_chunks).
 * Every rejection of bra_gpu_decompress_chunks applies to each file on its own: an empty stream, a
 * truncated record chain or one that overruns the file's stream, a header the reference validation
 * rejects, a Huffman or RLE failure, pi >= the chunk's decoded size, a chunk decoding to more than
 * block_size bytes, a decoded size not above the stream size (:423-427).  On a rejection the call
 * returns -1, *bad_file is the lowest rejected file index and nothing is decoded; the caller drops
 * that file and calls again.  *bad_file is UINT32_MAX when the call fails for another reason.
 * -2: out_cap too small, *out_size = the bytes needed.  The scratch the call uses is proportional
 * to the stream bytes plus the decoded bytes: the chunks' decoded sizes are found first (Huffman
 * decode, then the RLE decode's size pass into a zero capacity), then the chunks are laid out
 * exactly.
 */
int bra_gpu_decompress_files(bra_gpu_ctx_t* ctx, const uint8_t* d_streams, const uint64_t* stream_off, const uint64_t* stream_size,
                             uint32_t nfiles, uint32_t block_size, uint8_t* d_out, uint64_t out_cap, uint64_t* out_size,
                             bra_gpu_file_result_t* d_results, uint32_t* bad_file, void* stream);

#ifdef __cplusplus
}
#endif
