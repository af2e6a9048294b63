"""Inputs of the many-files tests (test_files_abi.py on the CPU, test_gpu_files.py on the GPU): seeded
file lists and their expected results from the oracle.  Not a test module."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOREM = os.path.join(ROOT, "tests", "golden", "lorem.txt")
CS = 256 * 1024

# every size at which the files path takes another route: 1..3 bytes, the 16-byte CRC unit, the
# 267 / 268-byte headers, the one-wave CRC threshold (4096), the 64 KiB CRC piece, the chunk size and
# its multiples with ragged tails
SIZE_LIST = [1, 2, 3, 19, 127, 128, 129, 267, 268, 300, 600, 1000, 3039, 4095, 4096, 4097, 65535, 65537, 262143, 262144, 262145,
             524288, 524295]
ZERO_SIZES = [5000, 262444]


def lorem() -> bytes:
    with open(LOREM, "rb") as f:
        return f.read()


def words(rng, n: int) -> bytes:
    """n bytes of Zipf-drawn words of the lorem vocabulary."""
    vocab = sorted(set(lorem().split()))
    w = 1.0 / np.arange(1, len(vocab) + 1)
    out, size = [], 0
    while size < n:
        for i in rng.choice(len(vocab), 256, p=w / w.sum()):
            out.append(vocab[i])
            size += len(vocab[i]) + 1
    return b" ".join(out)[:n]


def size_list_files():
    """The files of the 256 KiB size list, in list order, then the two all-zero files."""
    rng = np.random.default_rng(20240)
    files = []
    for n in SIZE_LIST:
        if n == 3039:
            files.append(lorem())
        elif n in (1, 2, 4096):
            files.append(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
        else:
            files.append(words(rng, n))
    files += [bytes(n) for n in ZERO_SIZES]
    assert [len(f) for f in files] == SIZE_LIST + ZERO_SIZES
    return files


def small_block_files():
    """About 40 files of 0..20000 bytes for block_size 4096, two of them empty."""
    rng = np.random.default_rng(4096)
    lens = [int(x) for x in rng.integers(1, 20001, 40)]
    lens[7] = lens[31] = 0
    return [words(rng, n) if i % 5 else rng.integers(0, 256, n, dtype=np.uint8).tobytes() for i, n in enumerate(lens)]


def pack(files, align: int = 1, lead: int = 0):
    """(buffer as np.uint8, offsets, lengths): the files back to back after `lead` bytes, or every
    file at an offset that is a multiple of `align` with gaps (filled with 0xEE) between them."""
    offs, pos = [], lead
    for f in files:
        if align > 1:
            pos = (pos + align - 1) // align * align
        offs.append(pos)
        pos += len(f) + (5 if align > 1 else 0)
    buf = np.full(pos + 16, 0xEE, dtype=np.uint8)
    for o, f in zip(offs, files):
        buf[o:o + len(f)] = np.frombuffer(f, np.uint8)
    return buf, offs, [len(f) for f in files]


def expected(orc, files, block_size: int):
    """Per file what the oracle's compress loop gives: dict(stream, chunks_crc, raw_crc, num_chunks,
    compressed); an empty file has an empty stream and zero CRCs."""
    out = []
    for f in files:
        if len(f) == 0:
            out.append(dict(stream=b"", chunks_crc=0, raw_crc=0, num_chunks=0, compressed=0))
            continue
        stream, crc, chunks = orc.compress_chunks(f, block_size)
        out.append(dict(stream=stream, chunks_crc=crc, raw_crc=orc.crc32c(f), num_chunks=len(chunks), compressed=int(len(stream) < len(f))))
    return out
