"""The host planning of the many-files calls (br-archive_amd/csrc/files_plan.h: file list -> chunk
table, first-chunk indices, the two CRC tail distances per chunk, the long chunks' pieces, the output
bound) compiled for the host alone and checked against the oracle's CRC32C (oracle/bra_oracle.c) by
tests/cpp/files_plan_check.cpp: a stand-alone program built with the address and
undefined-behaviour sanitizers; no Python runs in the sanitised process.  The GPU kernels that walk
the table are checked in test_gpu_files.py."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    if not shutil.which("g++") or not shutil.which("gcc"):
        pytest.skip("no host compiler")
    d = tmp_path_factory.mktemp("files_plan")
    obj = str(d / "oracle.o")
    exe = str(d / "files_plan_check")
    subprocess.run(["gcc", "-O1", "-g", *SAN, "-c", os.path.join(ROOT, "oracle", "bra_oracle.c"), "-o", obj], check=True)
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", *SAN,
                    os.path.join(ROOT, "tests", "cpp", "files_plan_check.cpp"), obj, "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("seed", ["0x9E3779B97F4A7C15", "11"])
def test_files_plan_matches_oracle(checker, seed):
    r = subprocess.run([checker, "200", seed], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok 200 ")
