"""The many-files part of the C-ABI (include/bra_hip_files.h): the library exports it, the Python
record matches the 32-byte C record, and the host-only output bound covers what the oracle's compress
loop produces.

CPU-only: no function that touches the GPU is called here.
"""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np

import files_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bra_hip_files.h")


def test_library_exports_files_symbols():
    bra = importlib.import_module("br-archive_amd")
    out = subprocess.check_output(["nm", "-D", "--defined-only", bra.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(bra_gpu_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(["bra_gpu_compress_files", "bra_gpu_decompress_files", "bra_gpu_files_bound"])
    assert sorted(bra.FILES_ABI_SYMBOLS) == declared
    assert not [f for f in declared if f not in exported]
    # bra_hip.h pulls the part in, so a C caller sees it through the one header
    assert '#include "bra_hip_files.h"' in open(os.path.join(ROOT, "include", "bra_hip.h")).read()


def test_file_result_record_is_32_bytes():
    bra = importlib.import_module("br-archive_amd")
    assert C.sizeof(bra.FileResult) == 32
    assert [(n, getattr(bra.FileResult, n).offset) for n, _ in bra.FileResult._fields_] == [
        ("off", 0), ("size", 8), ("chunks_crc", 16), ("raw_crc", 20), ("num_chunks", 24), ("compressed", 28)]
    dt = np.dtype(bra.FILE_RESULT_FIELDS)
    assert dt.itemsize == 32 and [dt.fields[n][1] for n, _ in bra.FILE_RESULT_FIELDS] == [0, 8, 16, 20, 24, 28]


def test_header_compiles_as_c(tmp_path):
    """The header is C as well as C++ (its size assertion included)."""
    src = tmp_path / "t.c"
    src.write_text('#include "bra_hip.h"\nint main(void) { return sizeof(bra_gpu_file_result_t) == 32 ? 0 : 1; }\n')
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")],
                   check=True)


def test_files_bound_covers_the_oracle_streams(orc):
    """bra_gpu_files_bound through ctypes, no GPU: at least the total of the oracle's chunk streams
    for the size list, additive over the files, and 0 for a list it cannot size."""
    bra = importlib.import_module("br-archive_amd")
    files = fc.size_list_files()
    exp = fc.expected(orc, files, fc.CS)
    lens = [len(f) for f in files]
    bound = bra.BlockCodec.files_bound(lens, fc.CS)
    total = sum(len(e["stream"]) for e in exp)
    assert bound >= total
    # every file's own stream fits its own share, whatever the neighbours compress to
    for n, e in zip(lens, exp):
        assert bra.BlockCodec.files_bound([n], fc.CS) >= len(e["stream"])
    # and it is the worst case of the chain, not a guess: 4 payload bytes per RLE byte (n + n / 128 + 16), 267 per chunk
    assert bound <= 4 * (1 + 1 / 128) * sum(lens) + (267 + 4 * 17) * sum((n + fc.CS - 1) // fc.CS for n in lens) + 4096
    assert bra.BlockCodec.files_bound(lens, 4096) >= sum(len(e["stream"]) for e in fc.expected(orc, files[:16], 4096))
    assert bra.BlockCodec.files_bound([0, 0], fc.CS) <= 64
    assert bra.lib.bra_gpu_files_bound(None, 3, fc.CS) == 0
    assert bra.BlockCodec.files_bound(lens, 0) == 0
